"""Drop-in replacement of the reference's Text2ImUNet / InpaintText2ImUNet backed by the HIP engine.

Same constructor hyper-parameters (through create_model), same state_dict keys and shapes (reference
checkpoints load with load_state_dict), same call surface as the reference driver uses
(kandinsky2/kandinsky2_1_model.py:90-104, 208-225, 246-257):
    model(x, timesteps, full_emb=, pooled_emb=, image_emb= [, inpaint_image=, inpaint_mask=]) -> [B,8,h,w]
    model.del_cache(), model.convert_to_fp16(), model.eval(), model.to(device), model.dtype
Everything inside forward() runs in libk22hip.so; there is no PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _lib, sampling
from .arch import UNetArch, make_arch, param_shapes
from .native import NativeEngine, NativeModule, arena_size
from .pack import pack_arena


class Text2ImUNetHIP(NativeModule):
    """MI355X-native Text2ImUNet (kandinsky2/model/text2im_model2_1.py:13-103).

    backend_dtype: torch.bfloat16 (BASELINE's dtype, bf16 MFMA), torch.float16 (the reference's own use_fp16 mode: same MFMA rate,
    3 more mantissa bits - the mode that holds <= 3e-3 on the 50-step final latent), torch.float32 (parity path, exact-fp32 MFMA) or
    "f16x3" (kandinsky2_amd.F16X3, split precision: fp32 tensors, every MFMA operand as an fp16 (hi, lo) pair, three fp16 MFMAs per
    product - within 1e-3 of the reference p_sampler's final latent, BASELINE.json's gate, at several times the fp32 engine's speed).
    use_graph: replay each forward as one captured hipGraph.
    chains: 2 = an even batch runs as TWO half-batch engines (same arena, own workspaces and graphs) on two streams of the device - the two
    halves of the classifier-free-guidance pair never interact inside the UNet (GroupNorm and attention are per sample), so one chain's
    latency-bound stretches (GroupNorm coefficient / apply launches, the 20-us GEMMs of the AttentionBlocks, split-K finishes) overlap
    the other's MFMA-bound ones.  Default: env K22_CHAINS, else 1.  Each half runs the tile-table lines of ITS problem sizes, so the bits of a
    two-chain run differ from a one-chain run of the same inputs (other split-K factors); the distances from the reference do not.
    """

    def __init__(self, arch: UNetArch, backend_dtype: torch.dtype = torch.bfloat16, use_graph: bool = True,
                 cache_text_emb: bool = True, meta_params: bool = False, chains: Optional[int] = None):
        if backend_dtype not in (torch.bfloat16, torch.float16, torch.float32, _lib.F16X3, _lib.F16X2):
            raise ValueError('backend_dtype must be torch.bfloat16, torch.float16, torch.float32, "f16x3" (split precision) or "f16x2" '
                             '(asymmetric split: per-op precision plan)')
        super().__init__(param_shapes(arch), backend_dtype, meta_params)
        self.arch = arch
        self.use_graph = use_graph
        self.cache_text_emb = cache_text_emb
        self.model_channels = arch.model_channels
        self.chains = int(os.environ.get("K22_CHAINS", "1")) if chains is None else int(chains)
        if self.chains not in (1, 2):
            raise ValueError("chains must be 1 or 2")
        self._side = None                               # stream of the second half-batch engine of the two-chain mode
        self.cache = None  # mirrors the reference attribute; holds the key of the cached conditioning
        self._release()

    # ---- reference-compatible no-ops -------------------------------------------------------------
    def convert_to_fp16(self):
        """The reference casts its conv / attention / head weights to fp16 here and computes the torso in fp16
        (unet.py:566-572, text2im_model2_1.py:49-55).  Same meaning here: the engine's storage and MFMA operand type becomes fp16
        (fp32 accumulation, GroupNorm statistics, softmax and sampler state stay fp32, as in the reference's fp16 mode).  An engine
        built with backend_dtype=torch.float32 is the parity path and stays fp32 until convert_to_fp16() is asked for explicitly."""
        if self.backend_dtype != torch.float16:
            self._need_fp32_params("convert_to_fp16", "backend_dtype=torch.float16")
            self.backend_dtype = torch.float16
            self._release()   # re-pack lazily in fp16
        return self

    def convert_to_fp32(self):
        """unet.py:574-580: back to the fp32 parity path"""
        if self.backend_dtype != torch.float32:
            self._need_fp32_params("convert_to_fp32", "backend_dtype=torch.float32")
            self.backend_dtype = torch.float32
            self._release()
        return self

    def _need_fp32_params(self, what: str, ctor_hint: str):
        """A dtype change re-packs the arena from the fp32 parameters: refuse when they are gone (released after packing, never
        materialised - meta_params - or replaced by an arena adopted from a broadcast), instead of dropping a working engine."""
        ps = list(self.parameters())
        if any(p.is_meta for p in ps) or (getattr(self, "_adopted", False) and not any(p.numel() for p in ps)) or getattr(self, "_arena_adopted", False):
            raise RuntimeError(f"{what}: this module has no fp32 parameters to re-pack from (prepare(free_params=True), meta_params=True or "
                               f"an adopted / broadcast arena); construct it with {ctor_hint} instead")

    def del_cache(self):
        self.cache = None
        self._cond_key = None

    # ---- engine management -------------------------------------------------------------------------
    def _release(self):
        super()._release()
        self._plan_key = self._cond_key = None          # _plan_key: (B, H, W) of the whole batch, which two chains split between their engines
        # operand buffers of sample_loop, ddim_loop and dpmpp_loop: one set each, never shared (the engine's captured loop holds their addresses)
        self._loop_bufs, self._ddim_bufs, self._dpmpp_bufs = sampling.OwnedBuffers(), sampling.OwnedBuffers(), sampling.OwnedBuffers()

    def arena_table(self):
        """name -> (byte offset, byte size) of the packed arena, derived from shapes only."""
        meta_sd = {k: torch.empty(v, device="meta") for k, v in param_shapes(self.arch).items()}
        return pack_arena(self.arch, meta_sd, self.backend_dtype, "meta")[1]

    def arena_bytes(self) -> int:
        return arena_size(self.arena_table())

    def _engine_config(self):
        """K22UNetConfig of this architecture / dtype (host-side only: no device is touched)"""
        a = self.arch
        cfg = _lib.K22UNetConfig()
        cfg.dtype = _lib.dtype_code(self.backend_dtype)
        cfg.in_channels = a.in_channels
        cfg.model_channels = a.model_channels
        cfg.out_channels = a.out_channels
        cfg.num_res_blocks = a.num_res_blocks
        cfg.n_levels = len(a.channel_mult)
        for i, v in enumerate(a.channel_mult):
            cfg.channel_mult[i] = v
        cfg.n_attention_ds = len(a.attention_ds)
        for i, v in enumerate(a.attention_ds):
            cfg.attention_ds[i] = v
        cfg.num_head_channels = a.num_head_channels
        cfg.ctx_dim = a.model_dim
        cfg.ctx_len = a.ctx_len
        cfg.n_image_embs = a.num_image_embs
        cfg.text_dim1 = a.text_dim1
        cfg.text_dim2 = a.text_dim2
        cfg.image_dim = a.image_dim
        cfg.head_type = 1 if a.head == "2.2" else 0
        cfg.hint_channels = a.hint_channels
        return cfg

    def prepare(self, arena: Optional[torch.Tensor] = None, free_params: bool = False):
        """Packs the weights (or adopts a broadcast arena) and creates the native engine."""
        dev = self._device(None if arena is None else arena.device)
        self._release()
        self._arena_adopted = arena is not None
        if arena is None:
            arena, table = pack_arena(self.arch, self.state_dict(), self.backend_dtype, dev)
        else:
            table = self.arena_table()
            if arena.numel() < arena_size(table) or arena.dtype != torch.uint8:
                raise ValueError("arena does not match this architecture/dtype")
        cfg = self._engine_config()
        self._engines[0] = NativeEngine("unet", cfg, arena, table)
        if self.chains == 2:
            if _lib.lib().k22_build_flags() & 1:
                raise RuntimeError("chains=2 overlaps two engines on one device: this libk22hip.so was built with packed-fp32 instructions (NOPK=0)")
            self._engines[1] = NativeEngine("unet", cfg, arena, table)      # second half-batch engine: same arena, own workspace and graphs
        if free_params:
            for p in self.parameters():
                p.data = torch.empty(0, device=dev)
        self._adopted = True
        return self

    def _ensure_plan(self, B: int, H: int, W: int):
        if not self._engines:
            self.prepare()
        if self._plan_key != (B, H, W):
            self._plan_key = self._cond_key = None   # no batch key until every engine of the batch has its plan
            n = 2 if self._chained(B) else 1
            for e in list(self._engines.values())[:n]:      # the first engine's workspace before the second's
                e.plan(B // n, H, W)
            if n == 2 and self._side is None:
                self._side = torch.cuda.Stream(device=self._arena.device)
            self._plan_key = (B, H, W)

    def _chained(self, B: int) -> bool:
        return len(self._engines) == 2 and B >= 2 and B % 2 == 0

    def _parts(self, B: int):
        """(handle, first row, rows, stream handle) of every chain of a batch of B; the side stream is ordered behind the caller's first"""
        cur = torch.cuda.current_stream()
        if not self._chained(B):
            return [(self._handle, 0, B, cur.cuda_stream)]
        self._side.wait_stream(cur)
        return [(self._handle, 0, B // 2, cur.cuda_stream), (self._engines[1].handle, B // 2, B // 2, self._side.cuda_stream)]

    def _join(self, B: int):
        if self._chained(B):
            torch.cuda.current_stream().wait_stream(self._side)

    def num_ops(self) -> int:
        return _lib.lib().k22_unet_num_ops(self._handle) if self._handle is not None else 0

    def profile(self, reps: int = 3):
        """Per-op-class device time of one forward (HIP events around every op, eager replay)."""
        kinds = ["conv3x3", "gemm", "groupnorm", "attention", "other"]
        tot = {k: dict(ms=0.0, flops=0.0, bytes=0.0, launches=0) for k in kinds}
        # two chains: the halves are timed one after the other, op by op - ISOLATED device times of both, summed (the step itself overlaps
        # them, so the class times then add up to more than the step)
        handles = [self._handle] + ([self._engines[1].handle] if self._plan_key is not None and self._chained(self._plan_key[0]) else [])
        for h in handles:
            ms, fl, by = (C.c_double * 5)(), (C.c_double * 5)(), (C.c_double * 5)()
            ln = (C.c_int * 5)()
            _lib.check(_lib.lib().k22_unet_profile(h, reps, ms, fl, by, ln, _lib.current_stream()))
            for i, k in enumerate(kinds):
                tot[k]["ms"] += ms[i]; tot[k]["flops"] += fl[i]; tot[k]["bytes"] += by[i]; tot[k]["launches"] += ln[i]
        return tot

    def tuning_report(self) -> str:
        """Tile configuration chosen (by measurement at the first forward) for every distinct conv / GEMM problem."""
        buf = C.create_string_buffer(1 << 16)
        _lib.check(_lib.lib().k22_unet_tuning_report(self._handle, buf, len(buf)))
        return buf.value.decode()

    def workspace_bytes(self) -> int:
        return 0 if self._ws is None else self._ws.numel()

    def set_condition(self, full_emb, pooled_emb, image_emb):
        """Text2ImUNet.get_text_emb (text2im_model2_1.py:57-80) + hoisted encoder_kv projections."""
        L = _lib.lib()
        if self._plan_key is None:
            raise RuntimeError("set_condition: no plan yet (call forward, which plans for its input shape)")
        B, a = self._plan_key[0], self.arch
        ntext = a.ctx_len - a.num_image_embs
        for name, t, want in (("full_emb", full_emb, (B, ntext, a.text_dim1)), ("pooled_emb", pooled_emb, (B, a.text_dim2)),
                              ("image_emb", image_emb, (B, a.image_dim))):
            if tuple(t.shape) != want:   # the engine copies B * ... bytes from these pointers: a wrong batch would read out of bounds
                raise ValueError(f"{name} must have shape {want} for a batch of {B}; got {tuple(t.shape)}")
            if t.device.type != "cuda":
                raise RuntimeError(f"{name} must be on the GPU (no CPU fallback)")
        f = full_emb.detach().float().contiguous()
        p = pooled_emb.detach().float().contiguous()
        i = image_emb.detach().float().contiguous()
        for h, r0, n, st in self._parts(B):
            _lib.check(L.k22_unet_set_condition(h, f[r0:r0 + n].data_ptr(), p[r0:r0 + n].data_ptr(), i[r0:r0 + n].data_ptr(), st))
        self._join(B)
        return self

    def _ensure_condition(self, full_emb, pooled_emb, image_emb):
        """the reference caches the conditioning after the first call until del_cache() (text2im_model2_1.py:58-59, 82-83)"""
        if self._cond_key is None or not self.cache_text_emb:
            if full_emb is None or pooled_emb is None or image_emb is None:
                raise ValueError("full_emb, pooled_emb and image_emb are required")
            self.set_condition(full_emb, pooled_emb, image_emb)
            self._cond_key = True
            self.cache = {"cached": True}

    def _inpaint_operands(self, x, inpaint_image, inpaint_mask):
        """(inpaint_image, inpaint_mask) as fp32 views on x's device, broadcast the way the reference's torch.cat([x, inpaint_image *
        inpaint_mask, inpaint_mask], dim=1) would need them ([B,4,H,W], [B,1,H,W]); None = not given, which on the 9-channel UNet means
        zeros (InpaintText2ImUNet.forward defaults, text2im_model2_1.py:146-150).  A text2img UNet takes neither."""
        if not self.arch.inpainting:
            if inpaint_image is not None or inpaint_mask is not None:
                raise ValueError("inpaint_image / inpaint_mask given to a text2img UNet (create it with inpainting=True)")
            return None, None
        B, _, H, W = x.shape
        try:
            return tuple(None if t is None else t.detach().float().to(x.device).expand(B, c, H, W) for t, c in ((inpaint_image, 4), (inpaint_mask, 1)))
        except RuntimeError as e:
            raise ValueError(f"inpaint_image / inpaint_mask do not match x {tuple(x.shape)}: {e}") from None

    @torch.no_grad()
    def forward(self, x, timesteps, full_emb=None, pooled_emb=None, image_emb=None, inpaint_image=None, inpaint_mask=None):
        if x.device.type != "cuda":
            raise RuntimeError("Text2ImUNetHIP.forward: input must be on the GPU (no CPU fallback)")
        B, Cx, H, W = x.shape
        if Cx != 4:
            raise ValueError("expected a 4-channel latent")
        self._ensure_plan(B, H, W)
        self._ensure_condition(full_emb, pooled_emb, image_emb)
        if timesteps.numel() != B:
            raise ValueError(f"timesteps must hold one value per batch element ({B}); got {tuple(timesteps.shape)}")
        xf = x.detach().float().contiguous()
        tf = timesteps.detach().float().reshape(B).contiguous().to(x.device)
        img, msk = self._inpaint_operands(xf, inpaint_image, inpaint_mask)
        if self.arch.inpainting:
            img = torch.zeros_like(xf) if img is None else img.contiguous()
            msk = torch.zeros_like(xf[:, :1]) if msk is None else msk.contiguous()
        out = torch.empty(B, self.arch.out_channels, H, W, dtype=torch.float32, device=x.device)
        for h, r0, n, st in self._parts(B):      # one chain, or the two half-batch chains side by side (each replays its own graph on its stream)
            _lib.check(_lib.lib().k22_unet_forward(
                h, xf[r0:r0 + n].data_ptr(), tf[r0:r0 + n].data_ptr(), _lib.ptr(None if img is None else img[r0:r0 + n]),
                _lib.ptr(None if msk is None else msk[r0:r0 + n]), out[r0:r0 + n].data_ptr(), 1 if self.use_graph else 0, st))
        self._join(B)
        return out

    # ---- the whole-loop entries: one driver (_run_loop), three hooks the 2.2 module overrides, the two sampler bodies both modules share ----
    def _loop_x(self, name, x, cfg_batch=False):
        """(B, H, W) of a loop entry's x: [N,4,h,w] on the GPU (cfg_batch: the CFG pair, N even), before the entry checks its own operands"""
        B, Cx, H, W = x.shape
        if Cx != 4 or x.device.type != "cuda" or (cfg_batch and B % 2):
            raise ValueError(f"{name}: x must be {'the CFG batch [2 bs,4,h,w]' if cfg_batch else '[N,4,h,w]'} on the GPU")
        return B, H, W

    def _loop_condition(self, full_emb=None, pooled_emb=None, image_emb=None):
        self._ensure_condition(full_emb, pooled_emb, image_emb)

    def _loop_inpaint(self, name, x, inpaint_image, inpaint_mask):
        return self._inpaint_operands(x, inpaint_image, inpaint_mask)

    def _loop_model_call(self, ts_rows, cond, img, msk):
        return sampling.fused_call(self.forward, ts_rows, inpaint_image=img, inpaint_mask=msk)

    def _run_loop(self, name, owned, x, ts_rows, cond, inpaint, *, key, shapes, operands, host, native, results, keep=None):
        """What every whole-loop entry does once x (_loop_x) and its own operands are checked.  cond: _loop_condition's keywords; inpaint =
        (inpaint_image, inpaint_mask), which _loop_inpaint refuses or brings to [B,4,h,w] / [B,1,h,w]; keep: sampling.keep_operands' tuple.
        One chain: the operands are copied into the entry's OwnedBuffers (attribute `owned`; the common ones here, the entry's own by shapes(box) /
        operands), because the captured loop holds their addresses - a second generation under the same key replays it instead of capturing
        20 000 nodes again; native(bufs, the four keep pointers, use_graph, stream) is the entry's one C call, results(bufs) clones its returns.
        Two chains: host(model_call, a copy of x, keep as contiguous fp32) drives the same launches from sampling.py - per model call the two
        half-batch graphs side by side, a join, the step kernels (one captured graph with two branches runs them back to back: round 4)."""
        B, _, H, W = x.shape
        img, msk = self._loop_inpaint(name, x, *inpaint)
        self._ensure_plan(B, H, W)
        self._loop_condition(**cond)
        if self._chained(B):
            hk = None if keep is None else sampling.keep_operands(name, keep, B // 2, H, W, len(keep[3]), host=True)
            return host(self._loop_model_call(ts_rows, cond, img, msk), x.detach().float().clone(), hk)
        dev, box, one = x.device, (B, 4, H, W), (B, 1, H, W)
        on9, onk = (lambda s: s if self.arch.inpainting else None), (lambda s: s if keep is not None else None)
        k_init, k_noise, k_mask, coef = keep or (None, None, None, None)
        bufs = getattr(self, owned).stage(                       # read behind _ensure_plan: a first prepare() renews the buffer sets
            key + (B, H, W, tuple(ts_rows.shape), keep is not None, str(dev)), dev,
            lambda: dict(x=box, tmp=box, ts=tuple(ts_rows.shape), img=on9(box), msk=on9(one), kinit=onk((4, H, W)), knoise=onk((B // 2, 4, H, W)),
                         kmask=onk((H, W)), **shapes(box)),
            dict(x=x, ts=ts_rows, img=img, msk=msk, kinit=k_init, knoise=k_noise, kmask=k_mask, **operands))
        kp = (_lib.ptr(bufs["kinit"]), _lib.ptr(bufs["knoise"]), _lib.ptr(bufs["kmask"]),
              None if keep is None else coef.ctypes.data_as(C.POINTER(C.c_float)))
        _lib.check(native(bufs, kp, 1 if self.use_graph else 0, _lib.current_stream()))
        return results(bufs)

    def _ddpm_loop(self, owned, x, ts_rows, noise_seq, table, table_rows, guidance_scale, clamp, pct, cond, inpaint, init_img=None, img_mask=None,
                   keep=None, threshold_group=None):
        """sample_loop of both UNets behind their checks: k22_unet_sample_loop_keep, which with no keep IS k22_unet_sample_loop (one body, one
        loop key), or step_loop with sampler_step and, with a keep, keep_region on the freshly written latent.  threshold_group: the handle's
        k22_unet_set_threshold_group, set before every native call (None = 0, the whole batch: a value never outlives the call it was given to)."""
        B, _, H, W = x.shape
        group = sampling.threshold_group(threshold_group, B)
        if group is not None and self._chained(B):
            raise ValueError("sample_loop: threshold_group needs one chain (two chains split the batch between their engines)")
        n, rows, tshape, g = len(table_rows), [int(r) for r in table_rows], tuple(table.shape), float(guidance_scale)
        clip, pct = (float(clamp[0]), float(clamp[1])), (int(pct[0]), float(pct[1]))
        ii = None if init_img is None else init_img.float().expand(B, 4, H, W)
        mm = None if init_img is None else img_mask.float().expand(B, 1, H, W)

        def host(call, xc, hk):
            def step(xs, model_out, nz, krow, x_out, x0, **kw):
                sampling.sampler_step(xs, model_out, nz, krow[1], x_out, x0, **kw)
                if hk is not None:
                    sampling.keep_region(x_out, hk[0], hk[1], hk[2], hk[3][krow[0], 0], hk[3][krow[0], 1], x_out)

            return sampling.step_loop(call, xc, list(enumerate(rows)), noise_seq.float().contiguous(), None, step, table=table.float().contiguous(),
                                      guidance=g, use_cfg=1, clamp=clip, pct=pct, init=None if ii is None else ii.contiguous(),
                                      mask=None if mm is None else mm.contiguous(), scratch=sampling.sampler_scratch(xc))[0]

        def native(b, kp, *tail):
            _lib.check(_lib.lib().k22_unet_set_threshold_group(self._handle, group or 0))
            return _lib.lib().k22_unet_sample_loop_keep(
                self._handle, b["x"].data_ptr(), b["tmp"].data_ptr(), b["ts"].data_ptr(), b["noise"].data_ptr(), _lib.ptr(b["init"]), _lib.ptr(b["mask"]),
                _lib.ptr(b["img"]), _lib.ptr(b["msk"]), b["table"].data_ptr(), (C.c_int * n)(*rows), n, g, clip[0], clip[1], pct[0], pct[1],
                b["scratch"].data_ptr(), *kp, *tail)

        return self._run_loop(
            "sample_loop", owned, x, ts_rows, cond, inpaint, key=(n, tshape, ii is not None),
            shapes=lambda box: dict(noise=(n,) + box, table=tshape, scratch=_lib.lib().k22_sampler_scratch_bytes(B, H * W),
                                    init=box if ii is not None else None, mask=(B, 1, H, W) if ii is not None else None),
            operands=dict(noise=noise_seq, table=table, init=ii, mask=mm), host=host, native=native, results=lambda b: b["x"].clone(), keep=keep)

    def _dpm_loop(self, owned, x, ts_rows, table, orders, guidance_scale, clamp, cond, inpaint, keep=None):
        """dpmpp_loop of both UNets behind their checks.  clamp None: k22_unet_dpmpp_loop / dpmpp_step; (lo, hi): k22_unet_dpmpp_loop_keep /
        dpmpp_step(clamp=) and, with a keep, keep_region - sampling.dpmpp_loop_keep either way."""
        n, orders, g = table.shape[0], [int(o) for o in orders], float(guidance_scale)
        clip = None if clamp is None else (float(clamp[0]), float(clamp[1]))

        def host(call, xc, hk):
            return sampling.dpmpp_loop_keep(call, xc, table.float().contiguous(), orders, guidance=g, clamp=clip, keep=hk)

        def native(b, kp, *tail):
            head = (self._handle, b["x"].data_ptr(), b["tmp"].data_ptr(), b["hist"].data_ptr(), b["ts"].data_ptr(), b["table"].data_ptr(),
                    (C.c_int * n)(*orders), _lib.ptr(b["img"]), _lib.ptr(b["msk"]), n, g)
            L = _lib.lib()
            return L.k22_unet_dpmpp_loop(*head, *tail) if clip is None else L.k22_unet_dpmpp_loop_keep(*head, *clip, *kp, *tail)

        return self._run_loop("dpmpp_loop", owned, x, ts_rows, cond, inpaint, key=(n,), shapes=lambda box: dict(hist=(2,) + box, table=(n, 5)),
                              operands=dict(table=table), host=host, native=native,
                              results=lambda b: (b["x"].clone(), b["hist"][(n - 1) % 2].clone()), keep=keep)

    @torch.no_grad()
    def sample_loop(self, x, ts_rows, noise_seq, table, table_rows, guidance_scale, clamp, pct, *, full_emb=None, pooled_emb=None,
                    image_emb=None, inpaint_image=None, inpaint_mask=None, init_img=None, img_mask=None, threshold_group=None):
        """The whole guided p_sampler loop as ONE hipGraph replay (k22_unet_sample_loop); returns the final latent [N,4,h,w].
        x [N,4,h,w] = x_T; ts_rows [n_steps, N] and noise_seq [n_steps, N,4,h,w] in execution order; table [T,8] + table_rows (host ints):
        the schedule row of every step.  threshold_group: rows of the cond half per dynamic-threshold group (sampling.threshold_group; None:
        the whole batch from element 0).  Owned operand buffers, replay and the two-chain route: _run_loop."""
        B, H, W = self._loop_x("sample_loop", x)
        n_steps = len(table_rows)
        if tuple(ts_rows.shape) != (n_steps, B) or tuple(noise_seq.shape) != (n_steps, B, 4, H, W):
            raise ValueError("sample_loop: ts_rows must be [n_steps, N] and noise_seq [n_steps, N, 4, h, w]")
        return self._ddpm_loop("_loop_bufs", x, ts_rows, noise_seq, table, table_rows, guidance_scale, clamp, pct,
                               dict(full_emb=full_emb, pooled_emb=pooled_emb, image_emb=image_emb), (inpaint_image, inpaint_mask), init_img, img_mask,
                               threshold_group=threshold_group)

    @torch.no_grad()
    def ddim_loop(self, kind, x, ts_rows, table, guidance_scale, noise_seq=None, *, full_emb=None, pooled_emb=None, image_emb=None,
                  inpaint_image=None, inpaint_mask=None):
        """The whole guided DDIM (kind "ddim") or PLMS ("plms") loop as ONE hipGraph replay (k22_unet_ddim_loop); returns (final latent,
        predicted x0 of the last step), both [N,4,h,w].  x = x_T; table [n_steps, 4]: the k22_ddim_step rows in execution order; ts_rows
        [n_calls, N]: the timestep of every model call in execution order - n_calls = n_steps for DDIM, n_steps + 1 for PLMS (its first step
        calls the model a second time, at the next step's timestep); noise_seq [n_steps, N,4,h,w]: DDIM with eta > 0 only.  A second
        generation of the same shape, step count and kind replays the capture (_run_loop)."""
        if kind not in ("ddim", "plms"):
            raise ValueError('ddim_loop: kind must be "ddim" or "plms"')
        B, H, W = self._loop_x("ddim_loop", x)
        plms = kind == "plms"
        n_steps = table.shape[0]
        n_calls = n_steps + 1 if plms else n_steps
        if n_steps < 1 or tuple(table.shape) != (n_steps, 4) or tuple(ts_rows.shape) != (n_calls, B):
            raise ValueError("ddim_loop: table must be [n_steps, 4] and ts_rows [n_calls, N] (n_calls = n_steps, + 1 for PLMS)")
        if noise_seq is not None and (plms or tuple(noise_seq.shape) != (n_steps, B, 4, H, W)):
            raise ValueError("ddim_loop: noise_seq is [n_steps, N, 4, h, w], for DDIM only (PLMS is eta = 0)")
        g = float(guidance_scale)

        def host(call, xc, _keep):                     # the steps of k22_unet_ddim_loop
            tbl = table.float().contiguous()
            if plms:
                return sampling.plms_loop(call, xc, tbl, sampling.plms_step, guidance=g)
            nzs = None if noise_seq is None else noise_seq.float().contiguous()
            return sampling.step_loop(call, xc, tbl, nzs, torch.empty_like(xc), sampling.ddim_step, guidance=g)

        def native(b, _kp, *tail):
            return _lib.lib().k22_unet_ddim_loop(
                self._handle, _lib.K22_LOOP_PLMS if plms else _lib.K22_LOOP_DDIM, b["x"].data_ptr(), b["tmp"].data_ptr(), b["x0"].data_ptr(),
                b["ts"].data_ptr(), b["table"].data_ptr(), _lib.ptr(b["noise"]), _lib.ptr(b["img"]), _lib.ptr(b["msk"]), _lib.ptr(b["hist"]),
                n_steps, g, *tail)

        return self._run_loop(
            "ddim_loop", "_ddim_bufs", x, ts_rows, dict(full_emb=full_emb, pooled_emb=pooled_emb, image_emb=image_emb),
            (inpaint_image, inpaint_mask), key=(kind, n_steps, noise_seq is not None),
            shapes=lambda box: dict(x0=box, table=(n_steps, 4), noise=(n_steps,) + box if noise_seq is not None else None,
                                    hist=(4,) + box if plms else None),
            operands=dict(table=table, noise=noise_seq), host=host, native=native, results=lambda b: (b["x"].clone(), b["x0"].clone()))

    @torch.no_grad()
    def dpmpp_loop(self, x, ts_rows, table, orders, guidance_scale, *, full_emb=None, pooled_emb=None, image_emb=None, inpaint_image=None,
                   inpaint_mask=None):
        """The whole guided DPM-Solver++ loop as ONE hipGraph replay (k22_unet_dpmpp_loop); returns (final latent, predicted x0 of the last
        step), both [N,4,h,w].  x = x_T; table [n_steps, 5]: the k22_dpmpp_step rows and orders (host ints, 1 or 2): sampling.dpmpp_table's
        pair, in execution order; ts_rows [n_steps, N]: the timestep of every model call.  A second generation of the same shape,
        step count and orders replays the capture (_run_loop)."""
        B, H, W = self._loop_x("dpmpp_loop", x)
        n_steps, orders = table.shape[0], [int(o) for o in orders]
        if n_steps < 1 or tuple(table.shape) != (n_steps, 5) or tuple(ts_rows.shape) != (n_steps, B) or len(orders) != n_steps:
            raise ValueError("dpmpp_loop: table must be [n_steps, 5], ts_rows [n_steps, N] and orders n_steps ints")
        return self._dpm_loop("_dpmpp_bufs", x, ts_rows, table, orders, guidance_scale, None,
                              dict(full_emb=full_emb, pooled_emb=pooled_emb, image_emb=image_emb), (inpaint_image, inpaint_mask))


def create_model(backend_dtype: torch.dtype = torch.bfloat16, use_graph: bool = True, inpainting: bool = False,
                 up: bool = False, **model_config) -> Text2ImUNetHIP:
    """Same keyword schema as the reference's create_model (kandinsky2/model/model_creation.py:9-83);
    version must be "2.1"."""
    if model_config.get("version", "2.1") != "2.1":
        raise NotImplementedError("only the 2.1 UNet is implemented")
    arch = make_arch(model_config, inpainting=inpainting)
    return Text2ImUNetHIP(arch, backend_dtype=backend_dtype, use_graph=use_graph,
                          cache_text_emb=model_config.get("cache_text_emb", True))
