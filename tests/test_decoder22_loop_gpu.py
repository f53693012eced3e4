"""The 2.2 decoders' denoising loop as one captured graph (KandinskyV22*DecoderHIP(whole_loop_graph=True) -> UNet2DConditionHIP.sample_loop
-> k22_unet_sample_loop_keep), and the kernel it adds (k22_keep_region), on the GPU.  Everything runs on tiny_unet22_config().

PARITY UNPINNED, as tests/test_unet22_gpu.py: oracle/unet22_ref.py restates diffusers' arithmetic from memory of its source.  These tests
check that the one-graph route computes what the stepwise route computes - bit for bit where the kernels and operands are the same
(text2img, ControlNet-depth, img2img), to rounding where the new kernel replaces k22_blend_noised (inpainting) - and that it stays
within the project's 1e-3 of the written restatement.  Equal bits alone would also hold if whole_loop_graph= were ignored: the
"loop_captures" / "loop_launches" counters of k22_debug_counter show which route ran.
Bounds: tests/decoder22_ref.py (the kernel: 4 * 2^-24 * S, derived from its code)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decoder22_ref as dr
import kandinsky2_amd as k22
from kandinsky2_amd import _lib, pipeline22, sampling
from oracle import prestep_ref, unet22_ref

pytestmark = pytest.mark.gpu

SA, SB = float(np.float32(0.8311 ** 0.5)), float(np.float32((1 - 0.8311) ** 0.5))
SCHED = {"config_2_2": (k22.SCHEDULER_CONFIG_2_2, unet22_ref.SCHED_2_2),
         "learned_range": (k22.SCHEDULER_CONFIG_2_2_LEARNED_RANGE, unet22_ref.SCHED_2_2_LEARNED_RANGE)}
_UNETS, _REFS = {}, {}


def _counters():
    L = _lib.lib()
    return L.k22_debug_counter(b"loop_captures"), L.k22_debug_counter(b"loop_launches")


def _unet(kind, backend=torch.float32, use_graph=True):
    """(unet config, state dict, module) of the tiny 2.2 UNet: kind "plain" | "controlnet" | "inpaint"; one module per key for the file"""
    key = (kind, backend, use_graph)
    if key not in _UNETS:
        cfg = k22.tiny_unet22_config()
        arch = k22.make_arch22(cfg, controlnet=kind == "controlnet", inpainting=kind == "inpaint")
        sd = k22.init_unet22_state_dict(arch, seed=0)
        m = k22.UNet2DConditionHIP(arch, backend_dtype=backend, use_graph=use_graph)
        m.load_state_dict(sd)
        _UNETS[key] = (dict(cfg, in_channels=9) if kind == "inpaint" else cfg, sd, m.to("cuda").eval())
    return _UNETS[key]


def _ref_fn(cfg, sd):
    return lambda xx, t, e, hh: unet22_ref.unet22_forward(sd, cfg, xx, t, e, hh)


def _t2i_inputs(bs, h, w, steps, controlnet, seed=6):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(bs, 4, h, w, generator=g)
    pos, neg = torch.randn(bs, 1280, generator=g), torch.randn(bs, 1280, generator=g)
    hint = torch.rand(bs, 3, 8 * h, 8 * w, generator=g) if controlnet else None
    nz = torch.randn(steps, bs, 4, h, w, generator=g)
    return lat, pos, neg, hint, nz


def _t2i(m, sched_cfg, whole, inp, h, w, steps, gs=4.0, **kw):
    lat, pos, neg, hint, nz = inp
    dec = pipeline22.KandinskyV22DecoderHIP(m, None, scheduler=k22.DDPMSchedulerHIP.from_config(sched_cfg), whole_loop_graph=whole)
    args = dict(latents=lat.cuda(), noise_seq=None if nz is None else nz.cuda())
    args.update(kw)
    return dec(pos.cuda(), neg.cuda(), height=8 * h, width=8 * w, num_inference_steps=steps, guidance_scale=gs,
               hint=None if hint is None else hint.cuda(), output_type="latent", **args)


# ---- 1. the kernel alone -------------------------------------------------------------------------------------------------------------------
KERNEL_SHAPES = [(1, 12, 20, "binary"), (2, 12, 20, "fractional"), (3, 12, 20, "binary"), (2, 1, 1, "fractional"),
                 (1, 258, 256, "binary")]      # the last: 2 * 4 * 66048 = 528384 elements, beyond the launcher's cap of 2048 blocks x 256 threads


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("coef", [(SA, SB), (1.0, 0.0)])
@pytest.mark.parametrize("bs,H,W,kind", KERNEL_SHAPES)
def test_keep_region_kernel_vs_float64(bs, H, W, kind, coef, inplace):
    """k22_keep_region alone against the float64 restatement under the derived bound; NaN-prefilled buffers with guards on both sides;
    out of place the inputs stay as they were, in place (out == x) the result is the same bits."""
    sa, sb = coef
    d = dr.keep_inputs(bs, H, W, kind, seed=bs + H)
    ref, S = dr.keep_region_ref(d, sa, sb)
    bound = dr.keep_bound(S)
    G, n = 64, d["x"].numel()
    dev = {k: v.cuda().contiguous() for k, v in d.items()}
    xbuf = dr.with_guard(dev["x"], G)
    obuf = xbuf if inplace else torch.full((n + 2 * G,), dr.NAN, device="cuda")
    x_view, o_view = xbuf[G:G + n], obuf[G:G + n]
    _lib.check(_lib.lib().k22_keep_region(x_view.data_ptr(), dev["init"].data_ptr(), dev["noise0"].data_ptr(), dev["mask"].data_ptr(), sa, sb,
                                          o_view.data_ptr(), 2 * bs, H * W, _lib.current_stream()))
    out = o_view.reshape(d["x"].shape).cpu()
    ratio = dr.worst_ratio(out, ref, bound)
    print(f"keep_region bs {bs} {H}x{W} {kind} (sa, sb) = ({sa:.4f}, {sb:.4f}) {'in place' if inplace else 'out of place'}: "
          f"worst |d| / bound {ratio:.3f}, max|d| {(out.double() - ref).abs().max().item():.3e}")
    assert dr.violations(out, ref, bound) == 0
    for buf in (xbuf, obuf):
        assert torch.isnan(buf[:G]).all() and torch.isnan(buf[G + n:]).all()
    if not inplace:
        assert torch.equal(x_view.reshape(d["x"].shape).cpu(), d["x"])
    for k in ("init", "noise0", "mask"):
        assert torch.equal(dev[k].cpu(), d[k])
    # every operation of the kernel is rounded once, in the order torch's own fp32 evaluation on the host rounds them: the same bits
    v32, _ = dr.keep_region_ref(d, sa, sb, dtype=torch.float32)
    assert dr.violations(v32, ref, bound) == 0 and torch.equal(out, v32)


def test_keep_region_refuses_bad_arguments():
    t = torch.zeros(2, 4, 4, 4, device="cuda")
    p, L = t.data_ptr(), _lib.lib()
    for args in ((None, p, p, p, 1.0, 0.0, p, 2, 16), (p, p, p, p, 1.0, 0.0, p, 3, 16), (p, p, p, p, 1.0, 0.0, p, 0, 16), (p, p, p, p, 1.0, 0.0, p, 2, 0)):
        with pytest.raises(RuntimeError, match="keep_region"):
            _lib.check(L.k22_keep_region(*args, _lib.current_stream()))


# ---- 2. text2img and ControlNet-depth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(SCHED))
@pytest.mark.parametrize("controlnet,backend", [(False, torch.float32), (True, torch.float32), (False, torch.bfloat16)])
def test_text2img_graph_equals_stepwise_and_the_oracle(controlnet, backend, variant):
    """bs 2, 16 x 16 latents, 5 steps: the one-graph route gives the stepwise route's bits (counters: it was a loop, the stepwise one was
    not); the fp32 engine's final latent within 1e-3 of unet22_ref.decoder_loop."""
    cfg, sd, m = _unet("controlnet" if controlnet else "plain", backend)
    bs, h, w, steps, gs = 2, 16, 16, 5, 4.0
    inp = _t2i_inputs(bs, h, w, steps, controlnet)
    cfg_hip, cfg_ref = SCHED[variant]
    c0 = _counters()
    step = _t2i(m, cfg_hip, False, inp, h, w, steps)
    assert _counters() == c0
    whole = _t2i(m, cfg_hip, True, inp, h, w, steps)
    c1 = _counters()
    assert c1[1] == c0[1] + 1 and c1[0] >= c0[0]
    assert torch.equal(step, whole), (step - whole).abs().max().item()
    if backend == torch.float32:
        key = (controlnet, variant)
        if key not in _REFS:
            lat, pos, neg, hint, nz = inp
            _REFS[key] = unet22_ref.decoder_loop(_ref_fn(cfg, sd), lat, pos, neg, steps, gs, nz, hint, sched_cfg=cfg_ref)
        err = (whole.cpu() - _REFS[key]).abs().max().item()
        print(f"2.2 one-graph decoder loop {'controlnet ' if controlnet else ''}{variant} fp32: final latent max|d| {err:.3e} (oracle unpinned)")
        assert err <= 1e-3


def test_text2img_ragged_latent_bs1():
    cfg, sd, m = _unet("plain")
    bs, h, w, steps, gs = 1, 16, 24, 5, 4.0
    inp = _t2i_inputs(bs, h, w, steps, False, seed=12)
    cfg_hip, cfg_ref = SCHED["config_2_2"]
    step, whole = _t2i(m, cfg_hip, False, inp, h, w, steps), _t2i(m, cfg_hip, True, inp, h, w, steps)
    assert torch.equal(step, whole)
    lat, pos, neg, hint, nz = inp
    want = unet22_ref.decoder_loop(_ref_fn(cfg, sd), lat, pos, neg, steps, gs, nz, None, sched_cfg=cfg_ref)
    err = (whole.cpu() - want).abs().max().item()
    print(f"2.2 one-graph decoder loop 16x24 bs 1 fp32: final latent max|d| {err:.3e} (oracle unpinned)")
    assert err <= 1e-3


def test_counters_capture_once_replay_and_recapture_on_another_guidance():
    cfg, sd, m = _unet("plain")
    h, w, steps = 16, 16, 5
    inp = _t2i_inputs(2, h, w, steps, False, seed=14)
    cfg_hip = SCHED["config_2_2"][0]
    c0, l0 = _counters()
    a = _t2i(m, cfg_hip, True, inp, h, w, steps, gs=5.5)        # guidance scales no other test of this file uses: no cached loop has them
    assert _counters() == (c0 + 1, l0 + 1)
    b = _t2i(m, cfg_hip, True, inp, h, w, steps, gs=5.5)
    assert _counters() == (c0 + 1, l0 + 2) and torch.equal(a, b)
    c = _t2i(m, cfg_hip, True, inp, h, w, steps, gs=3.25)
    assert _counters() == (c0 + 2, l0 + 3) and not torch.equal(a, c)
    assert torch.equal(c, _t2i(m, cfg_hip, False, inp, h, w, steps, gs=3.25))


@pytest.mark.parametrize("where", ["cuda", "cpu"])
def test_generator_drawn_noise_gives_the_same_latent_on_both_routes(where):
    """no noise_seq: the stepwise route draws one randn per step inside DDPMSchedulerHIP.step, the one-graph route draws them all up front
    by the same calls; a CPU generator draws on the CPU (its initial latent is drawn from it first and handed in)."""
    cfg, sd, m = _unet("plain")
    h, w, steps = 16, 16, 5
    lat, pos, neg, hint, _ = _t2i_inputs(2, h, w, steps, False, seed=15)
    outs = []
    for whole in (False, True):
        g = torch.Generator(device=where).manual_seed(77)
        x = torch.randn(2, 4, h, w, generator=g, device=where)
        outs.append(_t2i(m, SCHED["learned_range"][0], whole, (x, pos, neg, None, None), h, w, steps, noise_seq=None, generator=g))
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()
    g = torch.Generator(device=where).manual_seed(78)
    x = torch.randn(2, 4, h, w, generator=g, device=where)
    assert not torch.equal(outs[0], _t2i(m, SCHED["learned_range"][0], True, (x, pos, neg, None, None), h, w, steps, noise_seq=None, generator=g))


# ---- 3. img2img ----------------------------------------------------------------------------------------------------------------------------------
def test_img2img_tail_graph_equals_stepwise_and_the_oracle():
    """10 steps, strength 0.5: the loop runs over timesteps[5:] (table rows 5 .. 9)"""
    cfg, sd, m = _unet("plain")
    bs, h, w, steps, strength, gs = 2, 16, 16, 10, 0.5, 4.0
    g = torch.Generator().manual_seed(10)
    lat0 = torch.randn(1, 4, h, w, generator=g).repeat(bs, 1, 1, 1)
    pos, neg = torch.randn(bs, 1280, generator=g), torch.randn(bs, 1280, generator=g)
    nz0, nzs = torch.randn(bs, 4, h, w, generator=g), torch.randn(steps, bs, 4, h, w, generator=g)
    outs = {}
    for whole in (False, True):
        pipe = pipeline22.KandinskyV22Img2ImgDecoderHIP(m, None, None, whole_loop_graph=whole)
        c0 = _counters()
        outs[whole] = pipe(pos.cuda(), neg.cuda(), image=lat0.cuda(), height=8 * h, width=8 * w, num_inference_steps=steps, guidance_scale=gs,
                           strength=strength, noise=nz0.cuda(), noise_seq=nzs.cuda(), output_type="latent")
        assert _counters()[1] - c0[1] == (1 if whole else 0)
    assert torch.equal(outs[False], outs[True])
    want = unet22_ref.img2img_loop(_ref_fn(cfg, sd), lat0, pos, neg, steps, strength, gs, nz0, nzs)
    err = (outs[True].cpu() - want).abs().max().item()
    print(f"2.2 one-graph img2img loop fp32: final latent max|d| {err:.3e} (oracle unpinned)")
    assert err <= 1e-3


# ---- 4. inpainting -------------------------------------------------------------------------------------------------------------------------------
def _inpaint_inputs(bs=2, h=16, w=16, steps=5):
    g = torch.Generator().manual_seed(11)
    lat0 = torch.randn(1, 4, h, w, generator=g)
    mask_px = torch.ones(8 * h, 8 * w)
    mask_px[24:90, 40:100] = 0.0                        # the mask of test_inpaint_decoder_vs_oracle_fp32
    pos, neg = torch.randn(bs, 1280, generator=g), torch.randn(bs, 1280, generator=g)
    x_T, nzs = torch.randn(bs, 4, h, w, generator=g), torch.randn(steps, bs, 4, h, w, generator=g)
    mlat = prestep_ref.prepare_mask(F.interpolate(mask_px[None, None], (h, w), mode="nearest"))
    return lat0, mask_px, mlat, pos, neg, x_T, nzs


def _inpaint(m, whole, inp, h=16, w=16, steps=5, gs=4.0):
    lat0, mask_px, mlat, pos, neg, x_T, nzs = inp
    pipe = pipeline22.KandinskyV22InpaintDecoderHIP(m, None, None, whole_loop_graph=whole)
    return pipe(pos.cuda(), neg.cuda(), image=lat0.cuda(), mask_image=mask_px.numpy(), height=8 * h, width=8 * w, num_inference_steps=steps,
                guidance_scale=gs, latents=x_T.cuda(), noise_seq=nzs.cuda(), output_type="latent")


def test_inpainting_graph_vs_oracle_known_region_and_eager_entry():
    """9-channel tiny UNet, bs 2: the one-graph route within 1e-3 of unet22_ref.inpaint_loop, the known region ends within 1e-5 of the image
    latents, and the captured loop equals the same entry with use_graph = 0 bit for bit.  Against the stepwise route (k22_blend_noised, whose
    multiply-adds may be contracted) it is equal to rounding only: the distance is printed."""
    cfg9, sd, m = _unet("inpaint")
    inp = _inpaint_inputs()
    lat0, mask_px, mlat, pos, neg, x_T, nzs = inp
    c0 = _counters()
    got = _inpaint(m, True, inp)
    c1 = _counters()
    assert c1[1] == c0[1] + 1 and c1[0] - c0[0] in (0, 1)      # 0: this module's cached loop was this very one
    want = unet22_ref.inpaint_loop(_ref_fn(cfg9, sd), lat0, mlat, x_T, pos, neg, 5, 4.0, nzs)
    err = (got.cpu() - want).abs().max().item()
    keep = mlat[0, 0] == 1
    kerr = (got.cpu()[:, :, keep] - lat0[:, :, keep]).abs().max().item()
    step = _inpaint(m, False, inp)
    print(f"2.2 one-graph inpainting loop fp32: final latent max|d| {err:.3e} from the oracle (unpinned), known region {kerr:.3e} from the image "
          f"latents, {(got - step).abs().max().item():.3e} from the stepwise route")
    assert err <= 1e-3 and kerr <= 1e-5
    assert (step.cpu() - want).abs().max().item() <= 1e-3
    _, _, eager_m = _unet("inpaint", use_graph=False)
    c1 = _counters()
    eager = _inpaint(eager_m, True, inp)                # whole_loop_graph=True on a use_graph=False module: the same launches, eagerly
    assert _counters() == (c1[0], c1[1] + 1)
    assert torch.equal(got, eager)


def test_inpainting_loop_step_is_sampler_step_then_keep_region_bit_for_bit():
    """the chain launch by launch: a one-step loop equals k22_unet_forward -> k22_sampler_step -> k22_keep_region on the same device operands"""
    cfg9, sd, m = _unet("inpaint")
    lat0, mask_px, mlat, pos, neg, x_T, nzs = _inpaint_inputs()
    bs, h, w = 2, 16, 16
    sch = k22.DDPMSchedulerHIP.from_config(k22.SCHEDULER_CONFIG_2_2_LEARNED_RANGE).set_timesteps(5, device="cuda")
    t = sch.timesteps.tolist()[1]
    ts_rows, rows, _ = sampling.ddpm_loop_operands(sch, [t], 2 * bs)
    coef = np.array([[SA, SB]], dtype=np.float32)       # a mid-loop pair: the last row's (1, 0) would hide the noise operand
    emb = torch.cat([pos, neg], 0).cuda()
    x2 = torch.cat([x_T, x_T], 0).cuda()
    g = torch.Generator().manual_seed(5)
    nz = torch.randn(1, 2 * bs, 4, h, w, generator=g).cuda()           # different noise in the two CFG halves
    lat0c, mc, noise0 = lat0.cuda(), mlat.cuda(), x_T.cuda()
    masked = (lat0c * mc).expand(2 * bs, 4, h, w).contiguous()
    mask_b = mc.expand(2 * bs, 1, h, w).contiguous()
    clip = (-sch.clip, sch.clip)
    got = m.sample_loop(x2, ts_rows.cuda(), nz, sch._table, rows, 4.0, clip, image_embeds=emb, inpaint_image=masked, inpaint_mask=mask_b,
                        keep=(lat0c, noise0, mc, coef))
    out = m(torch.cat([x2, masked, mask_b], 1), t, added_cond_kwargs={"image_embeds": emb}, return_dict=False)[0]
    x_next = torch.empty_like(x2)
    sampling.sampler_step(x2, out, nz[0].contiguous(), rows[0], x_next, None, table=sch._table, guidance=4.0, use_cfg=1, clamp=clip, pct=(-1, 0.0),
                          init=None, mask=None, scratch=sampling.sampler_scratch(x2))
    before = x_next.clone()
    sampling.keep_region(x_next, lat0c.reshape(4, h, w).contiguous(), noise0.contiguous(), mc.reshape(h, w).contiguous(), SA, SB, x_next)
    assert torch.equal(got, x_next) and not torch.equal(before, x_next)
    assert not torch.equal(got[:bs], got[bs:])                          # the halves keep their own unknown region


def test_two_chain_mode_falls_back_to_the_host_driven_loop(monkeypatch):
    """sample_loop under _chained(B) (two half-batch engines) drives the same steps from the host: no loop is counted, text2img gives the
    stepwise decoder's bits, inpainting the captured loop's (both re-impose with k22_keep_region)."""
    cfg, sd, m = _unet("plain")
    h, w, steps = 16, 16, 5
    inp = _t2i_inputs(2, h, w, steps, False, seed=16)
    cfg_hip = SCHED["learned_range"][0]
    step = _t2i(m, cfg_hip, False, inp, h, w, steps)
    cfg9, sd9, m9 = _unet("inpaint")
    inp9 = _inpaint_inputs()
    graph9 = _inpaint(m9, True, inp9)
    for mod in (m, m9):
        monkeypatch.setattr(mod, "_chained", lambda B: True)
    c0 = _counters()
    assert torch.equal(_t2i(m, cfg_hip, True, inp, h, w, steps), step)
    assert torch.equal(_inpaint(m9, True, inp9), graph9)
    assert _counters() == c0


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------
def _raw(m, bufs, n_steps, rows, coef0, **over):
    """k22_unet_sample_loop_keep on the module's own operand buffers, single arguments overridden"""
    a = dict(x=bufs["x"].data_ptr(), tmp=bufs["tmp"].data_ptr(), ts=bufs["ts"].data_ptr(), noise=bufs["noise"].data_ptr(), img=_lib.ptr(bufs["img"]),
             msk=_lib.ptr(bufs["msk"]), table=bufs["table"].data_ptr(), n=n_steps, pct=-1, scratch=bufs["scratch"].data_ptr(),
             kinit=_lib.ptr(bufs["kinit"]), knoise=_lib.ptr(bufs["knoise"]), kmask=_lib.ptr(bufs["kmask"]),
             coef=coef0.ctypes.data_as(C.POINTER(C.c_float)))
    a.update(over)
    return _lib.lib().k22_unet_sample_loop_keep(m._handle, a["x"], a["tmp"], a["ts"], a["noise"], None, None, a["img"], a["msk"], a["table"],
                                                (C.c_int * len(rows))(*rows), a["n"], 4.0, -2.0, 2.0, a["pct"], 0.0, a["scratch"], a["kinit"],
                                                a["knoise"], a["kmask"], a["coef"], 1, _lib.current_stream())


def test_refused_calls_leave_the_captured_loop_as_it_was():
    cfg9, sd, m = _unet("inpaint")
    inp = _inpaint_inputs()
    first = _inpaint(m, True, inp)                     # captures (or replays) the 5-step keep loop of this module's buffers
    bufs = m._loop22_bufs.bufs
    sch = k22.DDPMSchedulerHIP.from_config(k22.SCHEDULER_CONFIG_2_2).set_timesteps(5, device="cuda")
    _, rows, coef = sampling.ddpm_loop_operands(sch, sch.timesteps.tolist(), 4, keep=True)
    # _denoise dropped the conditioning on its way out (fixed_conditioning): the handle still holds it, the entry does not ask Python
    c0 = _counters()
    refused = [dict(kinit=None), dict(knoise=None), dict(kmask=None), dict(coef=None), dict(kinit=None, knoise=None, kmask=None),   # keep in part
               dict(img=None), dict(msk=None),                                                   # the 9-channel operands
               dict(x=None), dict(noise=None), dict(scratch=None), dict(n=0), dict(pct=4 * 16 * 16)]   # what k22_unet_sample_loop refuses
    for over in refused:
        with pytest.raises(RuntimeError, match="unet_sample_loop"):
            _lib.check(_raw(m, bufs, 5, rows, coef, **over))
        assert _counters() == c0, over
    # an odd batch: a module of its own (planning another batch on `m` would drop its loop by itself)
    _, _, odd = _unet("plain")
    emb1 = torch.randn(1, 1280, generator=torch.Generator().manual_seed(1)).cuda()
    odd(torch.zeros(1, 4, 16, 16, device="cuda"), 10, added_cond_kwargs={"image_embeds": emb1})
    z = torch.zeros(5, 4, 4, 16, 16, device="cuda")
    rc = _lib.lib().k22_unet_sample_loop_keep(odd._handle, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None, None, None, None, z.data_ptr(),
                                              (C.c_int * 5)(*rows), 5, 4.0, -2.0, 2.0, -1, 0.0, z.data_ptr(), None, None, None, None, 1,
                                              _lib.current_stream())
    assert rc == -1 and b"even" in _lib.lib().k22_last_error()
    assert _counters() == c0
    # the earlier capture still replays: no new capture, one launch, the same bits
    again = _inpaint(m, True, inp)
    assert _counters() == (c0[0], c0[1] + 1) and torch.equal(first, again)
