"""Drop-in MoVQ *decoder* (the image_encoder.decode() half the sampling path uses) and *encoder* (image_encoder.encode(),
the img2img / inpainting pre-step) backed by the HIP engine.

Mirrors the reference interface for this path:
    Kandinsky2_1.image_encoder = MOVQ(**config["image_enc_params"]["params"])     (kandinsky2_1_model.py:107-113)
    samples = self.image_encoder.decode(samples / self.scale)                      (kandinsky2_1_model.py:288-289)
    process_images(samples)                                                        (kandinsky2/utils.py:57-70)
State-dict keys / shapes are those of the reference's MOVQ for `post_quant_conv` and `decoder.*`
(kandinsky2/vqgan/autoencoder.py:163-185, movq_modules.py:228-357); encoder / quantizer keys of a full MOVQ
checkpoint are accepted and ignored (load_state_dict(strict=False)).  No CPU fallback.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from .native import FAMILIES, NativeEngine, NativeModule, _pad_rows, layout_arena

MOVQ_CONFIG_2_1 = {  # CONFIG_2_1["image_enc_params"]["params"] (kandinsky2/configs.py:68-90)
    "embed_dim": 4, "n_embed": 16384,
    "ddconfig": {"double_z": False, "z_channels": 4, "resolution": 256, "in_channels": 3, "out_ch": 3, "ch": 128,
                 "ch_mult": [1, 2, 2, 4], "num_res_blocks": 2, "attn_resolutions": [32], "dropout": 0.0},
}


class MoVQArch:
    def __init__(self, ddconfig: dict, embed_dim: int = 4):
        self.ch = ddconfig["ch"]
        self.ch_mult = tuple(ddconfig["ch_mult"])
        self.num_res_blocks = ddconfig["num_res_blocks"]
        self.z_channels = ddconfig["z_channels"]
        self.out_ch = ddconfig["out_ch"]
        self.zq_ch = embed_dim
        res = ddconfig["resolution"]
        n = len(self.ch_mult)
        # MOVQDecoder.__init__ tracks a nominal resolution: level i runs at resolution / 2^i (movq_modules.py:258, 301-303)
        self.attn_levels = [i for i in range(n) if (res // 2 ** i) in ddconfig["attn_resolutions"]]
        if self.z_channels != 4 or embed_dim != 4:
            raise NotImplementedError("the engine supports z_channels == embed_dim == 4")

    def __repr__(self):     # by value: two architectures print alike exactly when they are alike (caches key on it)
        return (f"MoVQArch(ch={self.ch}, ch_mult={self.ch_mult}, num_res_blocks={self.num_res_blocks}, z_channels={self.z_channels}, "
                f"out_ch={self.out_ch}, zq_ch={self.zq_ch}, attn_levels={self.attn_levels})")

    def blocks(self):
        """(kind, prefix, cin, cout) in forward order: 'res' | 'attn' | 'up' (Upsample conv)."""
        n = len(self.ch_mult)
        out = []
        block_in = self.ch * self.ch_mult[n - 1]
        out += [("res", "decoder.mid.block_1", block_in, block_in), ("attn", "decoder.mid.attn_1", block_in, block_in),
                ("res", "decoder.mid.block_2", block_in, block_in)]
        for lvl in reversed(range(n)):
            block_out = self.ch * self.ch_mult[lvl]
            for i in range(self.num_res_blocks + 1):
                out.append(("res", f"decoder.up.{lvl}.block.{i}", block_in, block_out))
                block_in = block_out
                if lvl in self.attn_levels:
                    out.append(("attn", f"decoder.up.{lvl}.attn.{i}", block_in, block_in))
            if lvl != 0:
                out.append(("up", f"decoder.up.{lvl}.upsample.conv", block_in, block_in))
        return out, block_in


def movq_param_shapes(a: MoVQArch) -> "OrderedDict[str, tuple]":
    """state_dict keys -> shapes of post_quant_conv + decoder, in the reference's registration order."""
    s: "OrderedDict[str, tuple]" = OrderedDict()
    zq = a.zq_ch

    def conv(name, o, i, k):
        s[name + ".weight"] = (o, i, k, k)
        s[name + ".bias"] = (o,)

    def snorm(name, c):
        s[name + ".norm_layer.weight"] = (c,)
        s[name + ".norm_layer.bias"] = (c,)
        conv(name + ".conv_y", c, zq, 1)
        conv(name + ".conv_b", c, zq, 1)

    conv("post_quant_conv", a.z_channels, zq, 1)
    blocks, last = a.blocks()
    conv("decoder.conv_in", blocks[0][2], a.z_channels, 3)
    for kind, pfx, cin, cout in blocks:
        if kind == "res":
            snorm(pfx + ".norm1", cin)
            conv(pfx + ".conv1", cout, cin, 3)
            snorm(pfx + ".norm2", cout)
            conv(pfx + ".conv2", cout, cout, 3)
            if cin != cout:
                conv(pfx + ".nin_shortcut", cout, cin, 1)
        elif kind == "attn":
            snorm(pfx + ".norm", cin)
            for n in ("q", "k", "v", "proj_out"):
                conv(pfx + "." + n, cin, cin, 1)
        else:
            conv(pfx, cout, cin, 3)
    snorm("decoder.norm_out", last)
    conv("decoder.conv_out", a.out_ch, last, 3)
    return s


def init_movq_state_dict(a: MoVQArch, seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Seeded random weights (there are no checkpoints on the box): fan-in scaled convs, norms around 1, and
    conv_y biased to 1 so that SpatialNorm starts near a plain GroupNorm."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in movq_param_shapes(a).items():
        leaf = name.rsplit(".", 1)[1]
        if ".norm_layer." in name:
            t = torch.randn(shape, generator=g) * 0.1 + (1.0 if leaf == "weight" else 0.0)
        elif leaf == "bias":
            t = torch.randn(shape, generator=g) * 0.02 + (1.0 if ".conv_y." in name else 0.0)
        else:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            t = torch.randn(shape, generator=g) * (1.0 / math.sqrt(fan_in)) * (0.5 if (".conv_y." in name or ".conv_b." in name) else 1.0)
        sd[name] = t
    return sd


def pack_movq_arena(a: MoVQArch, sd: Dict[str, torch.Tensor], tdtype: torch.dtype, device) -> Tuple[torch.Tensor, "OrderedDict[str, Tuple[int, int]]"]:
    f32 = torch.float32
    ent: "OrderedDict[str, torch.Tensor]" = OrderedDict()

    def get(name):
        return sd[name].detach().to(device=device, dtype=f32)

    for name, shape in movq_param_shapes(a).items():
        w = get(name)
        if name == "decoder.conv_in.weight":
            wp = torch.zeros(w.shape[0], 3, 3, 64, device=device)
            wp[..., : w.shape[1]] = w.permute(0, 2, 3, 1)
            ent[name] = _pad_rows(wp.reshape(w.shape[0], -1)).to(tdtype).contiguous()
        elif name.startswith("post_quant_conv") or ".conv_y." in name or ".conv_b." in name or ".norm_layer." in name or name.endswith(".bias"):
            ent[name] = w.reshape(w.shape[0], -1).contiguous() if w.dim() == 4 else w.contiguous()
        elif len(shape) == 4 and shape[2] == 3:
            ent[name] = _pad_rows(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)).to(tdtype).contiguous()
        else:  # 1x1 projections feeding the MFMA GEMM
            ent[name] = _pad_rows(w.reshape(w.shape[0], -1)).to(tdtype).contiguous()
    return layout_arena(ent, device)


def _movq_config(a: MoVQArch, backend_dtype) -> _lib.K22MoVQConfig:
    cfg = _lib.K22MoVQConfig()
    cfg.dtype = _lib.dtype_code(backend_dtype)
    cfg.ch = a.ch
    cfg.n_levels = len(a.ch_mult)
    for i, v in enumerate(a.ch_mult):
        cfg.ch_mult[i] = v
    cfg.num_res_blocks = a.num_res_blocks
    cfg.attn_levels = sum(1 << i for i in a.attn_levels)
    cfg.z_channels = a.z_channels
    cfg.out_ch = a.out_ch
    return cfg


# attention= of the two modules -> k22_movq_set_attention's mode: "auto" = the fused kernel above 16384 keys (no [T][T] workspace), the
# scores route at every size up to it; "scores" / "fused" force one form at every size
ATTENTION_MODES = {"auto": 0, "scores": 1, "fused": 2}


def movq_family(kind: str, entries=None):
    """The (create, destroy, plan, bind) callables NativeEngine drives for the "movq" / "movq_encoder" family, with the AttnBlock form in
    the plan's key: plan(handle, B, h, w, mode, nbytes) sets the mode on the handle (k22_movq_set_attention holds from the next plan) and
    plans.  entries: (create, destroy, plan, bind, set_attention) in place of the C entries (the host tests pass recording fakes)."""
    create, destroy, plan, bind, set_attention = entries or [getattr(_lib.lib(), n) for n in FAMILIES[kind] + ("k22_movq_set_attention",)]

    def plan_with_mode(handle, B, h, w, mode, nbytes):
        rc = set_attention(handle, mode)
        return rc if rc else plan(handle, B, h, w, nbytes)

    return create, destroy, plan_with_mode, bind


class _MoVQAttention:
    """attention= of MoVQDecoderHIP / MoVQEncoderHIP: validated on assignment, part of the plan key (assigning it re-plans at the next call)"""

    @property
    def attention(self) -> str:
        return self._attention

    @attention.setter
    def attention(self, mode: str):
        if mode not in ATTENTION_MODES:
            raise ValueError(f"attention must be one of {sorted(ATTENTION_MODES)}, not {mode!r}")
        self._attention = mode

    def _ensure_plan(self, B, h, w):
        if not self._engines:
            self.prepare()
        self._engines["movq"].ensure_plan(B, h, w, ATTENTION_MODES[self._attention])


class MoVQDecoderHIP(_MoVQAttention, NativeModule):
    """MI355X-native `MOVQ.decode` (kandinsky2/vqgan/autoencoder.py:182-185).  attention: "auto" | "scores" | "fused" (ATTENTION_MODES)."""

    def __init__(self, ddconfig: Optional[dict] = None, n_embed: int = 16384, embed_dim: int = 4,
                 backend_dtype: torch.dtype = torch.bfloat16, attention: str = "auto"):
        self.arch = MoVQArch(ddconfig or MOVQ_CONFIG_2_1["ddconfig"], embed_dim)
        super().__init__(movq_param_shapes(self.arch), backend_dtype)
        self.attention = attention

    def load_state_dict(self, state_dict, strict: bool = False, **kw):
        own = set(movq_param_shapes(self.arch).keys())
        r = super().load_state_dict({k: v for k, v in state_dict.items() if k in own}, strict=False, **kw)
        if strict and r.missing_keys:
            raise RuntimeError(f"missing decoder keys: {r.missing_keys[:4]} ...")
        return r

    def prepare(self):
        dev = self._device()
        self._release()
        arena, table = pack_movq_arena(self.arch, self.state_dict(), self.backend_dtype, dev)
        self._engines["movq"] = NativeEngine(movq_family("movq"), _movq_config(self.arch, self.backend_dtype), arena, table)
        return self

    @torch.no_grad()
    def decode(self, quant: torch.Tensor, return_uint8: bool = False):
        """quant [B,4,h,w] -> image [B,3,8h,8w] float32 in about [-1,1] (and, with return_uint8, the NHWC uint8
        image of process_images)."""
        if quant.device.type != "cuda":
            raise RuntimeError("MoVQDecoderHIP.decode: input must be on the GPU (no CPU fallback)")
        B, Cz, h, w = quant.shape
        if Cz != 4:
            raise ValueError("expected a 4-channel latent")
        self._ensure_plan(B, h, w)
        z = quant.detach().float().contiguous()
        up = 1 << (len(self.arch.ch_mult) - 1)
        out = torch.empty(B, self.arch.out_ch, h * up, w * up, dtype=torch.float32, device=quant.device)
        u8 = torch.empty(B, h * up, w * up, self.arch.out_ch, dtype=torch.uint8, device=quant.device) if return_uint8 else None
        _lib.check(_lib.lib().k22_movq_decode(self._handle, z.data_ptr(), out.data_ptr(), _lib.ptr(u8), _lib.current_stream()))
        return (out, u8) if return_uint8 else out

    forward = decode


# ======================================================================================================================
# Encoder: MOVQ.encode = Encoder.forward + quant_conv (kandinsky2/vqgan/autoencoder.py:176-180, vqgan_blocks.py:253-367)
# ======================================================================================================================
def movq_encoder_blocks(a: MoVQArch):
    """(kind, prefix, cin, cout) in forward order: 'res' | 'attn' | 'down' (Downsample conv); and the final width."""
    out = []
    n = len(a.ch_mult)
    block_in = a.ch
    for lvl in range(n):
        block_out = a.ch * a.ch_mult[lvl]
        for i in range(a.num_res_blocks):
            out.append(("res", f"encoder.down.{lvl}.block.{i}", block_in, block_out))
            block_in = block_out
            if lvl in a.attn_levels:
                out.append(("attn", f"encoder.down.{lvl}.attn.{i}", block_in, block_in))
        if lvl != n - 1:
            out.append(("down", f"encoder.down.{lvl}.downsample.conv", block_in, block_in))
    out += [("res", "encoder.mid.block_1", block_in, block_in), ("attn", "encoder.mid.attn_1", block_in, block_in),
            ("res", "encoder.mid.block_2", block_in, block_in)]
    return out, block_in


def movq_encoder_param_shapes(a: MoVQArch, in_channels: int = 3) -> "OrderedDict[str, tuple]":
    """state_dict keys -> shapes of encoder.* + quant_conv.* as the reference's MOVQ registers them."""
    s: "OrderedDict[str, tuple]" = OrderedDict()

    def conv(name, o, i, k):
        s[name + ".weight"] = (o, i, k, k)
        s[name + ".bias"] = (o,)

    def norm(name, c):
        s[name + ".weight"] = (c,)
        s[name + ".bias"] = (c,)

    conv("encoder.conv_in", a.ch, in_channels, 3)
    blocks, last = movq_encoder_blocks(a)
    for kind, pfx, cin, cout in blocks:
        if kind == "res":
            norm(pfx + ".norm1", cin)
            conv(pfx + ".conv1", cout, cin, 3)
            norm(pfx + ".norm2", cout)
            conv(pfx + ".conv2", cout, cout, 3)
            if cin != cout:
                conv(pfx + ".nin_shortcut", cout, cin, 1)
        elif kind == "attn":
            norm(pfx + ".norm", cin)
            for n in ("q", "k", "v", "proj_out"):
                conv(pfx + "." + n, cin, cin, 1)
        else:
            conv(pfx, cout, cin, 3)
    norm("encoder.norm_out", last)
    conv("encoder.conv_out", a.z_channels, last, 3)
    conv("quant_conv", a.zq_ch, a.z_channels, 1)
    return s


def init_movq_encoder_state_dict(a: MoVQArch, seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    g = torch.Generator(device="cpu").manual_seed(seed)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in movq_encoder_param_shapes(a).items():
        leaf = name.rsplit(".", 1)[1]
        if len(shape) == 1 and (".norm" in name):
            t = torch.randn(shape, generator=g) * 0.1 + (1.0 if leaf == "weight" else 0.0)
        elif leaf == "bias":
            t = torch.randn(shape, generator=g) * 0.02
        else:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            t = torch.randn(shape, generator=g) * (1.0 / math.sqrt(fan_in))
        sd[name] = t
    return sd


def pack_movq_encoder_arena(a: MoVQArch, sd: Dict[str, torch.Tensor], tdtype: torch.dtype, device):
    f32 = torch.float32
    ent: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in movq_encoder_param_shapes(a).items():
        w = sd[name].detach().to(device=device, dtype=f32)
        if name == "encoder.conv_in.weight":      # Cin 3 -> 64 (the prepare kernel zero-extends the image the same way)
            wp = torch.zeros(w.shape[0], 3, 3, 64, device=device)
            wp[..., : w.shape[1]] = w.permute(0, 2, 3, 1)
            ent[name] = _pad_rows(wp.reshape(w.shape[0], -1)).to(tdtype).contiguous()
        elif name.startswith("quant_conv") or name.endswith(".bias") or len(shape) == 1:
            ent[name] = w.reshape(w.shape[0], -1).contiguous() if w.dim() == 4 else w.contiguous()
        elif shape[2] == 3:
            ent[name] = _pad_rows(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)).to(tdtype).contiguous()
        else:
            ent[name] = _pad_rows(w.reshape(w.shape[0], -1)).to(tdtype).contiguous()
    return layout_arena(ent, device)


class MoVQEncoderHIP(_MoVQAttention, NativeModule):
    """MI355X-native `MOVQ.encode` (kandinsky2/vqgan/autoencoder.py:176-180): image [B,3,H,W] in [-1,1] -> latent [B,4,H/8,W/8]
    (before the pipeline multiplies by its latent scale, kandinsky2_1_model.py:467).  State-dict keys are the reference's
    `encoder.*` and `quant_conv.*`; the other keys of a full MOVQ checkpoint are ignored.  attention: as MoVQDecoderHIP's."""

    def __init__(self, ddconfig: Optional[dict] = None, n_embed: int = 16384, embed_dim: int = 4,
                 backend_dtype: torch.dtype = torch.bfloat16, attention: str = "auto"):
        dd = ddconfig or MOVQ_CONFIG_2_1["ddconfig"]
        self.arch = MoVQArch(dd, embed_dim)
        self.in_channels = dd.get("in_channels", 3)
        if self.in_channels != 3:
            raise NotImplementedError("the encoder engine takes 3-channel images")
        super().__init__(movq_encoder_param_shapes(self.arch), backend_dtype)
        self.attention = attention

    def load_state_dict(self, state_dict, strict: bool = False, **kw):
        own = set(movq_encoder_param_shapes(self.arch).keys())
        r = super().load_state_dict({k: v for k, v in state_dict.items() if k in own}, strict=False, **kw)
        if strict and r.missing_keys:
            raise RuntimeError(f"missing encoder keys: {r.missing_keys[:4]} ...")
        return r

    def prepare(self):
        dev = self._device()
        self._release()
        arena, table = pack_movq_encoder_arena(self.arch, self.state_dict(), self.backend_dtype, dev)
        self._engines["movq"] = NativeEngine(movq_family("movq_encoder"), _movq_config(self.arch, self.backend_dtype), arena, table)
        return self

    @torch.no_grad()
    def encode(self, image: torch.Tensor) -> torch.Tensor:
        if image.device.type != "cuda":
            raise RuntimeError("MoVQEncoderHIP.encode: input must be on the GPU (no CPU fallback)")
        B, Ci, H, W = image.shape
        if Ci != 3:
            raise ValueError("expected a 3-channel image")
        self._ensure_plan(B, H, W)
        x = image.detach().float().contiguous()
        down = 1 << (len(self.arch.ch_mult) - 1)
        out = torch.empty(B, 4, H // down, W // down, dtype=torch.float32, device=image.device)
        _lib.check(_lib.lib().k22_movq_encode(self._handle, x.data_ptr(), out.data_ptr(), _lib.current_stream()))
        return out

    forward = encode
