"""What every Python mirror of a native engine shares - the host-side counterpart of csrc/plan.h:

    layout_arena / arena_size   the one arena layout (256-byte aligned entries, 256 spare bytes behind the last)
    NativeEngine                one native handle and its create -> plan -> bind -> destroy life cycle
    NativeModule                the nn.Module that holds the reference's parameters and drops its engines when they change

A mirror adds only what is its own: the packing of its weights, the fill of its config struct and its run calls.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, Tuple

import torch
import torch.nn as nn

from . import _lib

# engine family -> its (create, destroy, plan, bind) entries of include/k22.h
FAMILIES = {
    "unet": ("k22_unet_create", "k22_unet_destroy", "k22_unet_plan", "k22_unet_bind"),
    "movq": ("k22_movq_create", "k22_movq_destroy", "k22_movq_plan", "k22_movq_bind"),
    "movq_encoder": ("k22_movq_create", "k22_movq_destroy", "k22_movq_plan_encoder", "k22_movq_bind"),
    "prior": ("k22_prior_create", "k22_prior_destroy", "k22_prior_plan", "k22_prior_bind"),
    "encoder": ("k22_encoder_create", "k22_encoder_destroy", "k22_encoder_plan", "k22_encoder_bind"),
}


def _pad_rows(w: torch.Tensor, mult: int = 64) -> torch.Tensor:
    """rows of an MFMA GEMM weight, zero-padded to a multiple of the tile height"""
    o = w.shape[0]
    op = (o + mult - 1) // mult * mult
    if op == o:
        return w
    return torch.cat([w, torch.zeros((op - o,) + tuple(w.shape[1:]), dtype=w.dtype, device=w.device)], 0)


def arena_size(table) -> int:
    """bytes of the arena that `table` (name -> (byte offset, byte size)) describes"""
    off, nbytes = next(reversed(table.values()))
    return off + (nbytes + 255) // 256 * 256 + 256


def layout_arena(entries: "Dict[str, torch.Tensor]", device) -> Tuple[torch.Tensor, "OrderedDict[str, Tuple[int, int]]"]:
    """Packed tensors in engine order -> (arena: ONE zero-filled uint8 tensor on `device` holding their bytes, name -> (byte offset,
    byte size)).  device="meta" gives the table from shapes alone."""
    table: "OrderedDict[str, Tuple[int, int]]" = OrderedDict()
    off = 0
    for name, t in entries.items():
        nbytes = t.numel() * t.element_size()
        table[name] = (off, nbytes)
        off += (nbytes + 255) // 256 * 256
    arena = torch.zeros(arena_size(table), dtype=torch.uint8, device=device)
    for (o, nbytes), t in zip(table.values(), entries.values()):
        arena[o:o + nbytes] = t.reshape(-1).view(torch.uint8)
    return arena, table


def up2_fold(w9: torch.Tensor, opad: int) -> torch.Tensor:
    """k22_up2_fold: fp32 3x3 weights in pack order [O][9 * I] on the GPU -> the fp32 phase weights [4][opad][4 * I] of the four-phase
    upsampling convolution (csrc/conv3_up2.hip); the same sums, in the same order, as pack.fold_up2."""
    o, i = w9.shape[0], w9.shape[1] // 9
    w9 = w9.contiguous()
    out = torch.empty(4, opad, 4 * i, dtype=torch.float32, device=w9.device)
    _lib.check(_lib.lib().k22_up2_fold(w9.data_ptr(), out.data_ptr(), o, opad, i, _lib.current_stream()))
    return out


def conv3x3_up2(x_padded: torch.Tensor, wph: torch.Tensor, bias, out: torch.Tensor, B: int, H: int, W: int, Cin: int, Cout: int, dtype: int,
                splitk: int = 0, bm: int = 0, stats: "torch.Tensor | None" = None):
    """k22_conv3x3_up2: nearest 2x upsample + conv3x3 of the zero-bordered LOW-resolution x_padded [B][H+2][W+2][Cin] with the folded weights
    wph [4][Npad][4 * Cin] into `out` (the unpadded [B][2H][2W][Cout] rows; the caller's buffer).  stats: optional fp32 [rows][Cout][2]
    buffer for the GroupNorm partial sums.  Returns the stats rows per image (0 without stats)."""
    partial = torch.empty(max(1, splitk if splitk else 4) * B * 4 * H * W * Cout + 64, dtype=torch.float32, device=out.device)
    rpi = C.c_int(0)
    _lib.check(_lib.lib().k22_conv3x3_up2(
        x_padded.data_ptr(), wph.data_ptr(), _lib.ptr(bias), out.data_ptr(), partial.data_ptr(), B, H, W, Cin, Cout, wph.shape[1], splitk, bm,
        _lib.ptr(stats), 0 if stats is None else stats.shape[0], C.byref(rpi), dtype, _lib.current_stream()))
    return rpi.value


class NativeEngine:
    """One native engine: the handle, the arena its weights live in, the workspace of its current plan and `plan_key` - None while
    there is no finished plan.  `family` names the four C entries (FAMILIES), `cfg` is the filled K22*Config of that family."""

    def __init__(self, family, cfg, arena: torch.Tensor, table):
        self.handle, self.cfg, self.arena, self.ws, self.plan_key = None, cfg, arena, None, None
        if isinstance(family, str):      # anything else: the four callables themselves (the host tests pass recording fakes)
            family = [getattr(_lib.lib(), n) for n in FAMILIES[family]]
        create, self._destroy, self._plan, self._bind = family
        base, names = arena.data_ptr(), [n.encode() for n in table]       # the native side copies the names
        arr = (_lib.K22Weight * len(table))()
        for w, name, (off, _n) in zip(arr, names, table.values()):
            w.name, w.ptr = name, base + off
        h = C.c_void_p()
        _lib.check(create(C.byref(cfg), arr, len(table), C.byref(h)))
        self.handle = h

    def plan(self, *shape):
        """Plans for `shape` and binds a fresh workspace (the native side wants 256-byte alignment)."""
        self.plan_key = None   # a failed plan / bind leaves the native engine without a plan: never skip re-planning after it
        nbytes = C.c_size_t()
        _lib.check(self._plan(self.handle, *shape, C.byref(nbytes)))
        self.ws = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=self.arena.device)
        _lib.check(self._bind(self.handle, (self.ws.data_ptr() + 255) // 256 * 256, nbytes.value))
        self.plan_key = shape

    def ensure_plan(self, *shape):
        if self.plan_key != shape:
            self.plan(*shape)

    def close(self):
        if self.handle is not None:
            self._destroy(self.handle)
            self.handle = None
        self.arena = self.ws = self.plan_key = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _register(root: nn.Module, dotted: str, param: nn.Parameter) -> None:
    parts = dotted.split(".")
    m = root
    for p in parts[:-1]:
        if p not in m._modules:
            m.add_module(p, nn.Module())
        m = m._modules[p]
    m.register_parameter(parts[-1], param)


class NativeModule(nn.Module):
    """Parameters under the reference's state_dict keys (`shapes`: key -> shape) + the engines built from them.  Whatever changes the
    parameters (load_state_dict, a device move, a dtype change) releases the engines; the next call packs and plans again."""

    def __init__(self, shapes, backend_dtype, meta_params: bool = False):
        super().__init__()
        self.backend_dtype = backend_dtype
        self.dtype = torch.float32        # public tensors; the engine's arithmetic type is backend_dtype
        for name, shape in shapes.items():
            t = torch.empty(shape, device="meta") if meta_params else torch.zeros(shape)
            _register(self, name, nn.Parameter(t, requires_grad=False))
        self._engines: Dict[object, NativeEngine] = {}

    def _release(self):
        for e in self._engines.values():
            e.close()
        self._engines = {}

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def load_state_dict(self, *args, **kwargs):
        r = super().load_state_dict(*args, **kwargs)
        self._release()  # weights changed: re-pack lazily
        return r

    def _apply(self, fn, *args, **kwargs):
        r = super()._apply(fn, *args, **kwargs)
        self._release()  # device move: re-pack lazily
        return r

    def _device(self, dev=None):
        dev = next(self.parameters()).device if dev is None else dev
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on the GPU only (no CPU fallback): move it with .to('cuda')")
        return dev

    # the module's first engine (the only one of every mirror but the chained UNet and the towers) under the names its run calls use
    def _first(self, attr):
        e = next(iter(self._engines.values()), None)
        return None if e is None else getattr(e, attr)

    _handle = property(lambda self: self._first("handle"))
    _arena = property(lambda self: self._first("arena"))
    _ws = property(lambda self: self._first("ws"), lambda self, ws: setattr(next(iter(self._engines.values())), "ws", ws))
