"""The Kandinsky 2.2 prior on the HIP engines: what `Kandinsky2_2.__init__` builds as `KandinskyV22PriorPipeline`
(kandinsky2/kandinsky2_2_model.py:24-31) and every generate_* calls twice (:69-76, :99-104, :130-136).

    PriorTransformerHIP     diffusers' PriorTransformer under its own state_dict keys, on the K22Prior engine of the 2.1 prior
                            (csrc/prior.hip, skinny.hip): the network is a port of kandinsky2/model/prior.py:159-270 - 77 + 4 tokens,
                            pre-LN blocks with erf GELU, [cos | sin] time embedding, last token -> out projection - at
                            clip_dim = clip_xf_width = 1280, so the keys are re-named and the three q / k / v matrices stacked; no kernel is new.
    UnCLIPSchedulerHIP      UnCLIPScheduler.step with prediction_type "sample", variance_type "fixed_small_log" as a 4-float table row per
                            step: the row format of k22_prior_sampler_step / K22_PRIOR_LOOP_ANCESTRAL.
    KandinskyV22PriorHIP    KandinskyV22PriorPipeline.__call__ / interpolate / get_zero_embed over the BPE tokenizer, the CLIP-bigG text
                            tower (encoders.CLIPTextModelWithProjectionHIP), the two classes above and the bigG image tower; with prior22 /
                            encode_image22 it IS the conditioner pipeline22.Kandinsky2_2HIP drives.

PARITY UNPINNED for the diffusers side: diffusers is not installed here, so PriorTransformer's key names and layout and UnCLIPScheduler's
arithmetic are stated from the published sources, like the 2.2 decoders (unet22.py).  Pinned: the text tower against the installed
transformers (tests/golden/enc_cliptext_hf_tiny.pt), the transformer arithmetic against oracle/prior_ref.py - the bit-exact restatement
of the reference network this one was ported from - and the engine against PriorDiffusionModelHIP on the re-keyed weights (same bits).
No CPU fallback.
"""
from __future__ import annotations

import json
import math
import os
from collections import OrderedDict
from types import SimpleNamespace
from typing import Dict, Optional

import numpy as np
import torch

from .prior import PriorEngineModule, prior_param_shapes, qkv_heads

# config.json of the `prior` sub-folder of kandinsky-community/kandinsky-2-2-prior (diffusers PriorTransformer) [published architecture]
PRIOR_TRANSFORMER_2_2 = {"num_attention_heads": 32, "attention_head_dim": 64, "num_layers": 20, "embedding_dim": 1280, "num_embeddings": 77,
                         "additional_embeddings": 4, "time_embed_act_fn": "silu", "norm_in_type": None, "embedding_proj_norm_type": None,
                         "encoder_hid_proj_type": "linear", "added_emb_type": "prd", "dropout": 0.0}
# the only values of these the engine's network has (prior.py:159-270 has no input norms, a Linear on the text sequence and the prd token)
_PRIOR22_FIXED = {"time_embed_act_fn": "silu", "norm_in_type": None, "embedding_proj_norm_type": None, "encoder_hid_proj_type": "linear",
                  "added_emb_type": "prd", "dropout": 0.0}
# optional widths of diffusers' class: None, or the value None stands for
_PRIOR22_DERIVED = {"time_embed_dim": "inner", "embedding_proj_dim": "embedding_dim", "clip_embed_dim": "embedding_dim"}

# scheduler/scheduler_config.json of the prior repository [recalled, not read: load_prior22_from_cache_dir prefers the file]
SCHEDULER_CONFIG_PRIOR_2_2 = {"num_train_timesteps": 1000, "variance_type": "fixed_small_log", "clip_sample": True, "clip_sample_range": 10.0,
                              "prediction_type": "sample", "beta_schedule": "squaredcos_cap_v2"}
UNCLIP_SCHEDULER_DEFAULTS = {"num_train_timesteps": 1000, "variance_type": "fixed_small_log", "clip_sample": True, "clip_sample_range": 1.0,
                             "prediction_type": "epsilon", "beta_schedule": "squaredcos_cap_v2"}      # UnCLIPScheduler.__init__'s defaults

CLIP_IMAGE_MEAN, CLIP_IMAGE_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


def tiny_prior22_config() -> dict:
    """Same structure at 8 heads x 64 (512 wide) x 2 layers; embedding_dim stays 1280, the dimension new to the engine."""
    return dict(PRIOR_TRANSFORMER_2_2, num_attention_heads=8, num_layers=2)


def resolve_prior22_config(config: Optional[dict] = None) -> dict:
    """diffusers config -> the checked config.  Refuses what the engine's network does not have, naming the key."""
    c = dict(PRIOR_TRANSFORMER_2_2)
    given = {k: v for k, v in dict(config or {}).items() if not k.startswith("_")}
    unknown = [k for k in given if k not in c and k not in _PRIOR22_DERIVED]
    if unknown:
        raise ValueError(f"PriorTransformer config: keys this class does not know: {unknown}")
    c.update(given)
    for key, want in _PRIOR22_FIXED.items():
        if c[key] != want:
            raise NotImplementedError(f"prior config {key}={c[key]!r}: the HIP engine is built for {want!r} (the Kandinsky 2.2 prior)")
    inner = c["num_attention_heads"] * c["attention_head_dim"]
    for key, what in _PRIOR22_DERIVED.items():
        want = inner if what == "inner" else c[what]
        if c.get(key) not in (None, want):
            raise NotImplementedError(f"prior config {key}={c[key]!r}: the HIP engine is built for None (= {want})")
    if c["attention_head_dim"] != 64:
        raise NotImplementedError(f"prior config attention_head_dim={c['attention_head_dim']!r}: the HIP engine is built for 64")
    if c["additional_embeddings"] != 4:
        raise NotImplementedError(f"prior config additional_embeddings={c['additional_embeddings']!r}: the HIP engine is built for 4")
    return c


def prior22_hparams(config: dict) -> dict:
    """the engine's hparams (prior.prior_param_shapes / K22PriorConfig) of a resolved config"""
    c = resolve_prior22_config(config)
    return {"text_ctx": c["num_embeddings"], "xf_width": c["num_attention_heads"] * c["attention_head_dim"], "xf_layers": c["num_layers"],
            "xf_heads": c["num_attention_heads"], "xf_final_ln": True, "xf_padding": False, "clip_dim": c["embedding_dim"],
            "clip_xf_width": c["embedding_dim"]}


# diffusers name -> prior_param_shapes name, outside the blocks and inside one (Linear / LayerNorm prefixes)
_TOP = {"time_embedding.linear_1": "time_embed.0", "time_embedding.linear_2": "time_embed.2", "proj_in": "clip_img_proj",
        "embedding_proj": "text_emb_proj", "encoder_hidden_states_proj": "text_enc_proj", "norm_out": "final_ln",
        "proj_to_clip_embeddings": "out_proj"}
_BLOCK = {"norm1": "ln_1", "attn1.to_out.0": "attn.c_proj", "norm3": "ln_2", "ff.net.0.proj": "mlp.c_fc", "ff.net.2": "mlp.c_proj"}


def prior22_param_shapes(config: dict) -> "OrderedDict[str, tuple]":
    """state_dict of diffusers' PriorTransformer (models/transformers/prior_transformer.py) with clip_mean / clip_std"""
    hp = prior22_hparams(config)
    W, D, nc = hp["xf_width"], hp["clip_dim"], hp["text_ctx"] + 4
    s: "OrderedDict[str, tuple]" = OrderedDict()

    def lin(name, o, i):
        s[name + ".weight"] = (o, i)
        s[name + ".bias"] = (o,)

    s["positional_embedding"] = (1, nc, W)
    s["prd_embedding"] = (1, 1, W)
    lin("time_embedding.linear_1", W, W)
    lin("time_embedding.linear_2", W, W)
    lin("proj_in", W, D)
    lin("embedding_proj", W, D)
    lin("encoder_hidden_states_proj", W, D)
    for l in range(hp["xf_layers"]):
        p = f"transformer_blocks.{l}."
        s[p + "norm1.weight"] = (W,); s[p + "norm1.bias"] = (W,)
        for nm in ("to_q", "to_k", "to_v", "to_out.0"):
            lin(p + "attn1." + nm, W, W)
        s[p + "norm3.weight"] = (W,); s[p + "norm3.bias"] = (W,)
        lin(p + "ff.net.0.proj", 4 * W, W)
        lin(p + "ff.net.2", W, 4 * W)
    s["norm_out.weight"] = (W,); s["norm_out.bias"] = (W,)
    lin("proj_to_clip_embeddings", D, W)
    s["clip_mean"] = (1, D)
    s["clip_std"] = (1, D)
    return s


def init_prior22_state_dict(config: dict, seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    g = torch.Generator(device="cpu").manual_seed(seed)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in prior22_param_shapes(config).items():
        leaf = name.rsplit(".", 1)[-1]
        if name == "clip_mean":
            t = torch.randn(shape, generator=g) * 0.1
        elif name == "clip_std":
            t = torch.rand(shape, generator=g) + 0.5
        elif ".norm" in name or name.startswith("norm_out"):
            t = torch.randn(shape, generator=g) * 0.1 + (1.0 if leaf == "weight" else 0.0)
        elif name in ("positional_embedding", "prd_embedding"):
            t = torch.randn(shape, generator=g) * 0.3
        elif leaf == "bias":
            t = torch.randn(shape, generator=g) * 0.02
        else:
            t = torch.randn(shape, generator=g) * (1.0 / math.sqrt(shape[1]))
        sd[name] = t
    return sd


def rekey_prior22(sd: Dict[str, torch.Tensor], config: dict, qkv_layout: str = "planes") -> "OrderedDict[str, torch.Tensor]":
    """diffusers PriorTransformer keys -> the keys of prior.prior_param_shapes (the reference's PriorTransformer).  to_q / to_k / to_v
    become the one attn.c_qkv entry: stacked Q | K | V ("planes": what the engine's arena holds, pack_prior_arena(qkv_layout="planes")),
    or re-interleaved per head as the reference stores it ("heads": loads into PriorDiffusionModelHIP and oracle/prior_ref.py).
    clip_mean / clip_std are not part of that network and are left out."""
    hp = prior22_hparams(config)
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    out["positional_embedding"] = sd["positional_embedding"]
    out["prd_emb"] = sd["prd_embedding"]
    for src, dst in _TOP.items():
        for leaf in (".weight", ".bias"):
            out[dst + leaf] = sd[src + leaf]
    for l in range(hp["xf_layers"]):
        p, q = f"transformer_blocks.{l}.", f"transformer.resblocks.{l}."
        for leaf in (".weight", ".bias"):
            qkv = torch.cat([sd[p + "attn1.to_q" + leaf], sd[p + "attn1.to_k" + leaf], sd[p + "attn1.to_v" + leaf]], 0)
            out[q + "attn.c_qkv" + leaf] = qkv_heads(qkv, hp["xf_heads"]) if qkv_layout == "heads" else qkv
            for src, dst in _BLOCK.items():
                out[q + dst + leaf] = sd[p + src + leaf]
    return OrderedDict((k, out[k]) for k in prior_param_shapes(hp))


class PriorTransformerHIP(PriorEngineModule):
    """diffusers' `PriorTransformer` (the `prior` folder of kandinsky-2-2-prior) on the K22Prior engine; parameters under diffusers' keys,
    clip_mean / clip_std [1, D] among them.  The attention mask: diffusers adds -10000 to the masked logits (padding keys and, through
    its causal_attention_mask buffer, later keys) where the reference adds -inf.  In fp32 exp(-10000 - max) is 0 and the causal diagonal
    keeps every row non-empty, so both give the masked keys exactly zero weight: the engine's mask is used unchanged."""

    def __init__(self, config: Optional[dict] = None, backend_dtype: torch.dtype = torch.bfloat16):
        self.config_dict = resolve_prior22_config(config)
        self.hp = prior22_hparams(self.config_dict)
        super().__init__(prior22_param_shapes(self.config_dict), backend_dtype)
        self._init_engine()
        self.config = SimpleNamespace(**self.config_dict)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        sd = {k: v for k, v in state_dict.items() if k != "causal_attention_mask"}     # a buffer of the class: the engine builds the mask in
        return super().load_state_dict(sd, strict=strict, **kw)

    def _engine_weights(self):
        return rekey_prior22(self.state_dict(), self.config_dict, "planes"), "planes"

    @torch.no_grad()
    def forward(self, hidden_states, timestep, proj_embedding, encoder_hidden_states, attention_mask=None, **_unused):
        """hidden_states [B, D], timestep (scalar or [B]), proj_embedding [B, D], encoder_hidden_states [B, 77, D], attention_mask
        [B, 77] (1 = token) -> namespace(predicted_image_embedding [B, D])"""
        B = hidden_states.shape[0]
        dev = hidden_states.device
        ts = torch.as_tensor(timestep, dtype=torch.float32, device=dev).reshape(-1)
        ts = ts.expand(B) if ts.numel() == 1 else ts
        if attention_mask is None:
            attention_mask = torch.ones(B, self.hp["text_ctx"], device=dev)
        return SimpleNamespace(predicted_image_embedding=self.transformer(hidden_states, ts, proj_embedding, encoder_hidden_states,
                                                                          attention_mask))

    def post_process_latents(self, prior_latents):
        return prior_latents * self.clip_std.to(prior_latents.device) + self.clip_mean.to(prior_latents.device)


def betas_for_alpha_bar(num_diffusion_timesteps: int, max_beta: float = 0.999) -> torch.Tensor:
    """diffusers' helper of that name (cosine alpha_bar): Python floats, then one conversion to float32"""
    ab = lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2  # noqa: E731
    T = num_diffusion_timesteps
    return torch.tensor([min(1 - ab((i + 1) / T) / ab(i / T), max_beta) for i in range(T)], dtype=torch.float32)


class UnCLIPSchedulerHIP:
    """diffusers' UnCLIPScheduler as the prior pipeline uses it: prediction_type "sample" (the model predicts x0), variance_type
    "fixed_small_log", the x0 prediction clamped to +-clip_sample_range.  One step is
        mean = c1 * clamp(x0) + c2 * x;   x' = mean + [t > 0] * exp(0.5 * logvar) * noise
    which k22_prior_sampler_step computes from the row (c1, c2, logvar, t > 0) of step_table(N).  The coefficients are float32 torch
    operations in the order of UnCLIPScheduler.step / _get_variance (PARITY UNPINNED: stated from the published source)."""

    def __init__(self, num_train_timesteps=1000, variance_type="fixed_small_log", clip_sample=True, clip_sample_range=1.0,
                 prediction_type="epsilon", beta_schedule="squaredcos_cap_v2"):
        if prediction_type != "sample":
            raise NotImplementedError(f"UnCLIPSchedulerHIP: prediction_type {prediction_type!r}: 'sample' only (the Kandinsky prior)")
        if variance_type != "fixed_small_log":
            raise NotImplementedError(f"UnCLIPSchedulerHIP: variance_type {variance_type!r}: 'fixed_small_log' only")
        if beta_schedule != "squaredcos_cap_v2":
            raise NotImplementedError(f"UnCLIPSchedulerHIP: beta_schedule {beta_schedule!r}: 'squaredcos_cap_v2' only")
        self.config = SimpleNamespace(num_train_timesteps=int(num_train_timesteps), variance_type=variance_type, clip_sample=bool(clip_sample),
                                      clip_sample_range=float(clip_sample_range), prediction_type=prediction_type, beta_schedule=beta_schedule)
        self.betas = betas_for_alpha_bar(int(num_train_timesteps))
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.clip = float(clip_sample_range) if clip_sample else float("inf")
        self.init_noise_sigma = 1.0
        self.timesteps = None
        self.missing_keys: tuple = ()

    @classmethod
    def from_config(cls, config: dict):
        """`UnCLIPScheduler.from_config(scheduler_config.json)`: the file's keys override the class defaults; the keys it does not hold
        are reported (self.missing_keys); keys the class does not have raise."""
        unknown = [k for k in config if k not in UNCLIP_SCHEDULER_DEFAULTS and not k.startswith("_")]
        if unknown:
            raise ValueError(f"UnCLIPSchedulerHIP.from_config: keys this scheduler does not know: {unknown}")
        cname = dict(config).get("_class_name", "UnCLIPScheduler")
        if cname != "UnCLIPScheduler":
            raise NotImplementedError(f"scheduler class {cname!r}: only UnCLIPScheduler (the prior repository's) is built")
        known = {k: v for k, v in dict(config).items() if k in UNCLIP_SCHEDULER_DEFAULTS}
        sch = cls(**dict(UNCLIP_SCHEDULER_DEFAULTS, **known))
        sch.missing_keys = tuple(sorted(k for k in UNCLIP_SCHEDULER_DEFAULTS if k not in known))
        return sch

    def set_timesteps(self, num_inference_steps: int, device=None):
        N, T = int(num_inference_steps), self.config.num_train_timesteps
        if N == 1:
            raise ValueError("UnCLIPSchedulerHIP: num_inference_steps = 1 divides by zero in UnCLIPScheduler.set_timesteps ((T - 1) / (N - 1))")
        if not 2 <= N <= T:
            raise ValueError(f"num_inference_steps must be in 2..{T}")
        self.num_inference_steps = N
        self.timesteps = torch.from_numpy((np.arange(0, N) * ((T - 1) / (N - 1))).round()[::-1].copy().astype(np.int64))
        return self.timesteps

    def step_row(self, t: int, prev: int) -> torch.Tensor:
        """(c1, c2, logvar, t > 0) of the step from t to prev (prev = t - 1 = -1 after the last timestep)"""
        one = torch.tensor(1.0)
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev] if prev >= 0 else one
        if prev == t - 1:
            beta, alpha = self.betas[t], self.alphas[t]
        else:
            beta = 1 - a_t / a_prev
            alpha = 1 - beta
        c1 = torch.sqrt(a_prev) * beta / (1 - a_t)
        c2 = torch.sqrt(alpha) * (1 - a_prev) / (1 - a_t)
        var = (1 - a_prev) / (1 - a_t) * beta
        logvar = torch.log(torch.clamp(var, min=1e-20))
        return torch.stack([c1, c2, logvar, torch.tensor(1.0 if t > 0 else 0.0)])

    def step_table(self, num_inference_steps: int) -> torch.Tensor:
        """[N, 4] float32 rows (c1, c2, logvar, t > 0) in execution order; sets the timesteps"""
        ts = self.set_timesteps(num_inference_steps).tolist()
        return torch.stack([self.step_row(t, ts[i + 1] if i + 1 < len(ts) else t - 1) for i, t in enumerate(ts)]).float().contiguous()


def clip_preprocess(image, size: int = 224) -> torch.Tensor:
    """CLIPImageProcessor of the prior repository on one PIL image: bicubic resize of the short side to `size`, centre crop, / 255,
    CLIP's mean / std -> [1, 3, size, size]"""
    from PIL import Image
    image = image.convert("RGB")
    w, h = image.size
    s = size / min(w, h)
    image = image.resize((max(size, round(w * s)), max(size, round(h * s))), Image.BICUBIC)
    w, h = image.size
    l, t = (w - size) // 2, (h - size) // 2
    a = torch.from_numpy(np.asarray(image.crop((l, t, l + size, t + size)), dtype=np.float32) / 255.0).permute(2, 0, 1)
    return ((a - torch.tensor(CLIP_IMAGE_MEAN)[:, None, None]) / torch.tensor(CLIP_IMAGE_STD)[:, None, None])[None]


class KandinskyV22PriorHIP:
    """`KandinskyV22PriorPipeline` (diffusers) on the HIP towers: __call__, interpolate, get_zero_embed with the pipeline's semantics, and
    prior22 / encode_image22 - the conditioner interface of pipeline22.Kandinsky2_2HIP.
    tokenizer: ClipBPETokenizer (padded_ids_and_mask); text_encoder: CLIPTextModelWithProjectionHIP; prior: PriorTransformerHIP;
    image_encoder: CLIPVisionModelWithProjectionHIP; scheduler: UnCLIPSchedulerHIP.
    The sampling loop is k22_prior_sample_loop(K22_PRIOR_LOOP_ANCESTRAL) on rows [cond | uncond] (diffusers orders them [uncond | cond];
    rows are independent): ONE captured graph by default, whole_loop_graph=False the same launches step by step.  The engine plans at
    most 8 rows, so a larger batch runs as independent chunks of at most 4 samples."""

    MAX_SAMPLES = 4

    def __init__(self, prior, image_encoder, text_encoder, tokenizer, scheduler: Optional[UnCLIPSchedulerHIP] = None, pad_id: int = 0,
                 whole_loop_graph: bool = True, device="cuda"):
        self.prior, self.image_encoder, self.text_encoder, self.tokenizer = prior, image_encoder, text_encoder, tokenizer
        self.scheduler = scheduler or UnCLIPSchedulerHIP.from_config(SCHEDULER_CONFIG_PRIOR_2_2)
        self.pad_id, self.whole_loop_graph, self.device = int(pad_id), bool(whole_loop_graph), device

    # ---- host logic ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def batch_prompts(prompt, negative_prompt, num_images_per_prompt=1):
        """-> (cond texts, uncond texts), one entry per sample: the pipeline's `prompt + negative_prompt` batch with every row's
        classifier-free branch on the negative prompt, or on "" when there is none; each text repeated num_images_per_prompt times"""
        prompt = [prompt] if isinstance(prompt, str) else list(prompt)
        if isinstance(negative_prompt, str):
            negative_prompt = [negative_prompt]
        if negative_prompt is not None:
            negative_prompt = list(negative_prompt)
            if len(negative_prompt) != len(prompt):
                raise ValueError(f"negative_prompt has {len(negative_prompt)} entries for {len(prompt)} prompts")
            prompt, uncond = prompt + negative_prompt, 2 * negative_prompt
        else:
            uncond = [""] * len(prompt)
        rep = lambda xs: [x for x in xs for _ in range(num_images_per_prompt)]  # noqa: E731
        return rep(prompt), rep(uncond)

    def _encode_prompt(self, cond, uncond, device):
        """text_encoder(ids) WITHOUT an attention mask (as the pipeline); the token mask goes to the transformer only.
        -> (text_embeds [2n, D], last_hidden_state [2n, 77, D], mask [2n, 77]) with rows [cond | uncond]"""
        ids, mask = self.tokenizer.padded_ids_and_mask(list(cond) + list(uncond), pad_id=self.pad_id)
        out = self.text_encoder(ids.to(device))
        return out.text_embeds, out.last_hidden_state, mask.to(device)

    def get_zero_embed(self, batch_size=1, device=None):
        dev = device or self.device
        r = self.image_encoder.config.image_size
        return self.image_encoder(torch.zeros(1, 3, r, r, device=dev)).image_embeds.repeat(batch_size, 1)

    # ---- the denoising loop on one chunk of <= 4 samples -----------------------------------------------------------------------------
    def _loop(self, x0, table, ts, noise, guidance_scale, emb, seq, mask, whole):
        bs, D = x0.shape
        dev = x0.device
        N, T = 2 * bs, table.shape[0]
        x = torch.cat([x0, x0], 0).float().contiguous()
        nzs = torch.zeros(T, N, D, device=dev)
        nzs[:, :bs] = noise            # the engine carries 2 bs latent rows and reads only the first half
        scales = torch.full((bs,), float(guidance_scale), device=dev)
        ts_rows = ts.to(dev).float()[:, None].expand(T, N).contiguous()
        out = self.prior._run_loop(False, table, ts_rows, x, nzs, scales, emb, seq, mask, whole, clamp=min(self.scheduler.clip, 3.0e38))
        return out[:bs].clone()

    @torch.no_grad()
    def __call__(self, prompt, negative_prompt=None, num_images_per_prompt=1, num_inference_steps=25, guidance_scale=4.0, latents=None,
                 generator=None, noise_seq=None, whole_loop_graph=None):
        dev = self.device
        cond, uncond = self.batch_prompts(prompt, negative_prompt, num_images_per_prompt)
        batch, D = len(cond), self.prior.hp["clip_dim"]
        table = self.scheduler.step_table(num_inference_steps).to(dev)
        ts, T = self.scheduler.timesteps, table.shape[0]
        emb, seq, mask = self._encode_prompt(cond, uncond, dev)
        gdev = generator.device if generator is not None else dev
        if latents is None:
            latents = torch.randn(batch, D, generator=generator, device=gdev)
        if tuple(latents.shape) != (batch, D):
            raise ValueError(f"latents must be {(batch, D)}, got {tuple(latents.shape)}")
        latents = latents.to(dev).float() * self.scheduler.init_noise_sigma
        if noise_seq is None:      # one draw of the whole batch per step, in step order, as UnCLIPScheduler.step makes them
            noise_seq = torch.stack([torch.randn(batch, D, generator=generator, device=gdev) for _ in range(T)])
        if tuple(noise_seq.shape) != (T, batch, D):
            raise ValueError(f"noise_seq must be {(T, batch, D)}, got {tuple(noise_seq.shape)}")
        noise_seq = noise_seq.to(dev).float()
        whole = self.whole_loop_graph if whole_loop_graph is None else bool(whole_loop_graph)
        out = []
        for s in range(0, batch, self.MAX_SAMPLES):
            e = min(batch, s + self.MAX_SAMPLES)
            rows = list(range(s, e)) + list(range(batch + s, batch + e))
            out.append(self._loop(latents[s:e], table, ts, noise_seq[:, s:e], guidance_scale, emb[rows].contiguous(), seq[rows].contiguous(),
                                  mask[rows].contiguous(), whole))
        image_embeds = self.prior.post_process_latents(torch.cat(out, 0))
        if negative_prompt is None:
            zero = self.get_zero_embed(image_embeds.shape[0], dev)
        else:
            image_embeds, zero = image_embeds.chunk(2)
        return SimpleNamespace(image_embeds=image_embeds, negative_image_embeds=zero)

    @torch.no_grad()
    def interpolate(self, images_and_prompts, weights, num_images_per_prompt=1, num_inference_steps=25, guidance_scale=4.0,
                    negative_prior_prompt=None, negative_prompt="", generator=None, latents=None, noise_seq=None):
        """KandinskyV22PriorPipeline.interpolate: sum of weight x (prior embedding of a text | image-tower embedding of an image);
        negative_image_embeds from the prior on negative_prompt"""
        if len(images_and_prompts) != len(weights):
            raise ValueError(f"`images_and_prompts` has length {len(images_and_prompts)} and `weights` has length {len(weights)}")
        total = None
        for cond, w in zip(images_and_prompts, weights):
            if isinstance(cond, str):
                e = self(cond, negative_prior_prompt, num_images_per_prompt, num_inference_steps, guidance_scale, latents, generator,
                         noise_seq).image_embeds
            else:
                e = self.encode_image22(cond, self.device).repeat(num_images_per_prompt, 1)
            total = e * w if total is None else total + e * w
        neg = self(negative_prompt, None, num_images_per_prompt, num_inference_steps, guidance_scale, latents, generator, noise_seq)
        return SimpleNamespace(image_embeds=total, negative_image_embeds=neg.negative_image_embeds if negative_prompt == "" else neg.image_embeds)

    # ---- the conditioner of pipeline22.Kandinsky2_2HIP -------------------------------------------------------------------------------
    def prior22(self, prompt, negative_prompt, batch_size, steps, guidance, device):
        r = self(prompt, negative_prompt, num_images_per_prompt=batch_size, num_inference_steps=steps, guidance_scale=guidance)
        return r.image_embeds.to(device), r.negative_image_embeds.to(device)

    def encode_image22(self, image, device):
        if not torch.is_tensor(image):
            image = clip_preprocess(image, self.image_encoder.config.image_size)
        if image.dim() == 3:
            image = image[None]
        return self.image_encoder(image.to(self.device).float()).image_embeds.to(device)


# ---- loading the prior repository ------------------------------------------------------------------------------------------------------
def _read_weights(folder, stem):
    """<stem>.safetensors when it is there and safetensors is importable, else <stem>.bin; None when neither can be read"""
    st, bn = os.path.join(folder, stem + ".safetensors"), os.path.join(folder, stem + ".bin")
    if os.path.exists(st):
        try:
            from safetensors.torch import load_file
            return load_file(st)
        except ImportError:
            pass
    if os.path.exists(bn):
        return torch.load(bn, map_location="cpu")
    return None


def _read_json(path):
    return json.load(open(path)) if os.path.exists(path) else None


def load_prior22_from_cache_dir(cache_dir, backend_dtype: torch.dtype = torch.bfloat16, device="cuda", whole_loop_graph: bool = True):
    """What `from_pretrained('kandinsky-community/kandinsky-2-2-prior', ...)` reads (kandinsky2_2_model.py:24-31), from a local copy
    `cache_dir/kandinsky-2-2-prior/{prior,text_encoder,image_encoder,tokenizer,scheduler}/` -> KandinskyV22PriorHIP.  Every config.json
    found drives its module; scheduler/scheduler_config.json is preferred to SCHEDULER_CONFIG_PRIOR_2_2.  Raises with the names of the
    missing files (no download path)."""
    from .encoders import CLIP_BIGG_TEXT, CLIP_BIGG_VISION, CLIPTextModelWithProjectionHIP, CLIPVisionModelWithProjectionHIP
    from .tokenizer import ClipBPETokenizer
    root = os.path.join(cache_dir, "kandinsky-2-2-prior")
    j = lambda *p: os.path.join(root, *p)  # noqa: E731
    weights = {"prior": _read_weights(j("prior"), "diffusion_pytorch_model"), "text_encoder": _read_weights(j("text_encoder"), "model"),
               "image_encoder": _read_weights(j("image_encoder"), "model")}
    for k in ("text_encoder", "image_encoder"):
        if weights[k] is None:
            weights[k] = _read_weights(j(k), "pytorch_model")
    missing = [j("prior", "diffusion_pytorch_model.safetensors | .bin")] if weights["prior"] is None else []
    missing += [j(k, "model.safetensors | pytorch_model.bin") for k in ("text_encoder", "image_encoder") if weights[k] is None]
    if not os.path.exists(j("tokenizer", "merges.txt")):
        missing.append(j("tokenizer", "merges.txt"))
    if missing:
        raise FileNotFoundError(f"Kandinsky 2.2 prior files not found (no download path in this build): {missing}")
    tcfg, vcfg = _read_json(j("text_encoder", "config.json")), _read_json(j("image_encoder", "config.json"))
    tcfg = dict(CLIP_BIGG_TEXT, **{k: v for k, v in (tcfg or {}).items() if k in CLIP_BIGG_TEXT})
    vcfg = dict(CLIP_BIGG_VISION, **{k: v for k, v in (vcfg or {}).items() if k in CLIP_BIGG_VISION})
    prior = PriorTransformerHIP(_read_json(j("prior", "config.json")), backend_dtype=backend_dtype)
    prior.load_state_dict(weights["prior"])
    text = CLIPTextModelWithProjectionHIP(tcfg, backend_dtype=backend_dtype)
    text.load_state_dict(weights["text_encoder"])
    image = CLIPVisionModelWithProjectionHIP(vcfg, backend_dtype=backend_dtype)
    image.load_state_dict(weights["image_encoder"])
    tok = ClipBPETokenizer(j("tokenizer", "merges.txt"))
    scfg = _read_json(j("scheduler", "scheduler_config.json"))
    return KandinskyV22PriorHIP(prior.to(device).eval(), image.to(device).eval(), text.to(device).eval(), tok,
                                UnCLIPSchedulerHIP.from_config(scfg if scfg is not None else SCHEDULER_CONFIG_PRIOR_2_2),
                                pad_id=tok.pad_id_from_folder(j("tokenizer")), whole_loop_graph=whole_loop_graph, device=device)
