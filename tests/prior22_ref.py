"""Independent restatements for the Kandinsky 2.2 prior (kandinsky-2_amd/prior22.py), for tests/test_prior22_cpu.py and
tests/test_prior22_gpu.py.  A plain module like skinny_ref.py / aux_ref.py, whose constants it reuses unchanged.

transformer64    diffusers' PriorTransformer.forward in float64, written in the diffusers layout from the published source - separate
                 to_q / to_k / to_v, softmax(q k^T d^-0.5 + mask), additive -10000 mask (padding keys and, causal_attention_mask, later
                 keys), norm1 / attn1 / norm3 / ff(GELU erf), norm_out on the last token, proj_to_clip_embeddings - straight from the
                 diffusers-keyed state dict.  It shares no code with the key map (prior22.rekey_prior22) or with oracle/prior_ref.py.
chain_bound      the fp32-against-float64 bound of one forward.  Not a new constant: the per-operation constants skinny_ref.py derives
                 (GEMM_C = 14.8 per Linear, LN_C = 8.92 per LayerNorm, ATT_C = 4 per attention, GELU_K = 17 per GELU, all in units of
                 2^-24 of the operation's magnitude) summed over the operations one value passes on its way through the network:
                     input: time_embedding's two Linears and the input projection        3 GEMM_C
                     per block: norm1, q/k/v, attention, to_out, norm3, ff.0, GELU, ff.2  2 LN_C + 4 GEMM_C + ATT_C + GELU_K
                     output: norm_out, proj_to_clip_embeddings                           LN_C + GEMM_C
                 To first order an error made in one operation reaches the output with gain <= 1 in units of the activations' scale (pre-LN
                 residual blocks: every branch is normalised on entry, norm_out on exit), so the sum times 2^-24 times the largest
                 |output| bounds the difference.  2 blocks: 264 x 2^-24 = 1.6e-5 of scale; a wrong key map moves the output by O(1).
step_table       UnCLIPScheduler.step / _get_variance (prediction_type "sample", variance_type "fixed_small_log") restated in float32
                 torch operations in diffusers' order (dtype = torch.float32), or in float64 (the deviation the CPU suite prints).
loop64           the sampling loop on RECORDED model outputs: per step the guided, clamped x0 and the restated step in float64, with the
                 per-step bound aux_ref.py derives for prior_sampler_step (SAMPLER_N roundings of the magnitude sum, one of the result,
                 the exp term).
hf_text_to_openai_clip   transformers CLIPTextModelWithProjection keys -> OpenAI clip.model.CLIP text keys (CLIPModelHIP)
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import aux_ref as ar
import skinny_ref as sr


# ---- PriorTransformer in float64, diffusers layout ---------------------------------------------------------------------------------------
def transformer64(sd, cfg, hidden_states, timestep, proj_embedding, encoder_hidden_states, attention_mask):
    f = lambda t: t.double()  # noqa: E731
    sd = {k: f(v) for k, v in sd.items()}
    H, hd = cfg["num_attention_heads"], cfg["attention_head_dim"]
    W = H * hd
    lin = lambda n, v: v @ sd[n + ".weight"].t() + sd[n + ".bias"]  # noqa: E731
    ln = lambda n, v: F.layer_norm(v, (W,), sd[n + ".weight"], sd[n + ".bias"], 1e-5)  # noqa: E731
    B = hidden_states.shape[0]
    # Timesteps(inner_dim, flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin] of t * 10000^(-i / half)
    half = W // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float64) / half)
    args = f(timestep).reshape(-1).expand(B)[:, None] * freqs[None]
    t_proj = torch.cat([torch.cos(args), torch.sin(args)], -1)
    t_emb = lin("time_embedding.linear_2", F.silu(lin("time_embedding.linear_1", t_proj)))
    x = torch.cat([lin("encoder_hidden_states_proj", f(encoder_hidden_states)), lin("embedding_proj", f(proj_embedding))[:, None], t_emb[:, None],
                   lin("proj_in", f(hidden_states))[:, None], sd["prd_embedding"].expand(B, -1, -1)], 1)
    x = x + sd["positional_embedding"]
    n = x.shape[1]
    am = (1 - f(attention_mask)) * -10000.0
    am = F.pad(am, (0, cfg["additional_embeddings"]), value=0.0)
    causal = torch.full((n, n), -10000.0, dtype=torch.float64).triu_(1)
    bias = (am[:, None, :] + causal[None])[:, None]                                      # [B, 1, n, n]
    for l in range(cfg["num_layers"]):
        p = f"transformer_blocks.{l}."
        y = ln(p + "norm1", x)
        q, k, v = (lin(p + "attn1." + nm, y).view(B, n, H, hd).transpose(1, 2) for nm in ("to_q", "to_k", "to_v"))
        a = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5 + bias, -1) @ v
        x = x + lin(p + "attn1.to_out.0", a.transpose(1, 2).reshape(B, n, W))
        y = ln(p + "norm3", x)
        x = x + lin(p + "ff.net.2", F.gelu(lin(p + "ff.net.0.proj", y)))
    return lin("proj_to_clip_embeddings", ln("norm_out", x)[:, -1])


def chain_c(num_layers: int) -> float:
    return 3 * sr.GEMM_C + num_layers * (2 * sr.LN_C + 4 * sr.GEMM_C + sr.ATT_C + sr.GELU_K) + sr.LN_C + sr.GEMM_C


def chain_bound(ref64: torch.Tensor, num_layers: int) -> float:
    return chain_c(num_layers) * sr.U24 * ref64.abs().max().item()


# ---- UnCLIPScheduler ----------------------------------------------------------------------------------------------------------------------
def timesteps(N, T=1000):
    return (np.arange(0, N) * ((T - 1) / (N - 1))).round()[::-1].copy().astype(np.int64).tolist()


def step_table(N, T=1000, dtype=torch.float32):
    """-> ([N, 4] rows (c1, c2, logvar, t > 0) of `dtype`, timesteps, branch taken per row: True = prev == t - 1)"""
    ab = lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2  # noqa: E731
    betas = torch.tensor([min(1 - ab((i + 1) / T) / ab(i / T), 0.999) for i in range(T)], dtype=dtype)
    alphas = 1.0 - betas
    ac = torch.cumprod(alphas, dim=0)
    ts = timesteps(N, T)
    rows, branch = [], []
    for i, t in enumerate(ts):
        prev = ts[i + 1] if i + 1 < N else t - 1
        a_t = ac[t]
        a_prev = ac[prev] if prev >= 0 else torch.tensor(1.0, dtype=dtype)
        if prev == t - 1:
            beta, alpha = betas[t], alphas[t]
        else:
            beta = 1 - a_t / a_prev
            alpha = 1 - beta
        branch.append(prev == t - 1)
        c1 = a_prev ** 0.5 * beta / (1 - a_t)
        c2 = alpha ** 0.5 * (1 - a_prev) / (1 - a_t)
        var = (1 - a_prev) / (1 - a_t) * beta
        rows.append(torch.stack([c1, c2, torch.log(torch.clamp(var, min=1e-20)), torch.tensor(1.0 if t > 0 else 0.0, dtype=dtype)]))
    return torch.stack(rows), ts, branch


# ---- the loop on recorded model outputs -----------------------------------------------------------------------------------------------------
def step64(x, model_out, noise, scales, row, clamp):
    """one step on rows [cond | uncond] in float64 -> x' ; both halves get the guided x0 of the pair"""
    x, mo, nz, s, r = x.double(), model_out.double(), noise.double(), scales.double()[:, None], row.double()
    bs = s.shape[0]
    c, u = mo[:bs], mo[bs:]
    x0 = (u + s * (c - u)).clamp(-clamp, clamp).repeat(2, 1)
    mean = r[0] * x0 + r[1] * x
    return mean + r[3] * torch.exp(0.5 * r[2]) * nz


def step_bound(x, model_out, noise, scales, row):
    """aux_ref's bound of prior_sampler_step for these operands (the clamp of its cases, SAMPLER_CLAMP, is the prior's 10)"""
    ref, S, e_act = ar.sampler_ref(ar.to64({"x": x, "mo": model_out, "noise": noise, "scales": scales, "tab": row}))
    return ref, ar.SAMPLER_N * ar.U24 * S + ar.U24 * ref.abs() + e_act


def loop64(recorded, scales, table, clamp=10.0):
    """recorded: per step (x_k, model_out_k, noise_k, x_{k+1}) as the engine had them -> largest |x_{k+1} - step64| / bound over the steps"""
    worst = 0.0
    for k, (x, mo, nz, x_next) in enumerate(recorded):
        ref = step64(x, mo, nz, scales, table[k], clamp)
        ref_ar, bound = step_bound(x.cpu(), mo.cpu(), nz.cpu(), scales.cpu(), table[k].cpu())
        assert clamp == ar.SAMPLER_CLAMP and torch.allclose(ref.cpu(), ref_ar, rtol=1e-13, atol=0)   # the two float64 restatements of the step coincide
        worst = max(worst, ((x_next.double().cpu() - ref.cpu()).abs() / bound.clamp_min(1e-300)).max().item())
    return worst


# ---- key maps of the checks ---------------------------------------------------------------------------------------------------------------
def hf_text_to_openai_clip(sd, cfg, clip_sd):
    """transformers CLIPTextModelWithProjection state dict -> a copy of `clip_sd` (clip.model.CLIP keys, CLIPModelHIP) whose text tower
    holds these weights: in_proj = [q; k; v], text_projection = text_projection.weight^T"""
    out = dict(clip_sd)
    out["token_embedding.weight"] = sd["text_model.embeddings.token_embedding.weight"]
    out["positional_embedding"] = sd["text_model.embeddings.position_embedding.weight"]
    for l in range(cfg["num_hidden_layers"]):
        s, d = f"text_model.encoder.layers.{l}.", f"transformer.resblocks.{l}."
        out[d + "attn.in_proj_weight"] = torch.cat([sd[s + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0)
        out[d + "attn.in_proj_bias"] = torch.cat([sd[s + f"self_attn.{n}_proj.bias"] for n in "qkv"], 0)
        for a, b in (("self_attn.out_proj", "attn.out_proj"), ("layer_norm1", "ln_1"), ("mlp.fc1", "mlp.c_fc"), ("mlp.fc2", "mlp.c_proj"),
                     ("layer_norm2", "ln_2")):
            out[d + b + ".weight"], out[d + b + ".bias"] = sd[s + a + ".weight"], sd[s + a + ".bias"]
    out["ln_final.weight"], out["ln_final.bias"] = sd["text_model.final_layer_norm.weight"], sd["text_model.final_layer_norm.bias"]
    out["text_projection"] = sd["text_projection.weight"].t().contiguous()
    return out
