"""The DPM-Solver++ sampler on the Kandinsky 2.2 decoders, on the GPU: k22_dpmpp_step_clip against float64 under the derived bound of
tests/decoder22_dpm_ref.py, the decoders' sampler="dpm_sampler" stepwise and as one captured graph (UNet2DConditionHIP.dpmpp_loop ->
k22_unet_dpmpp_loop_keep) bit for bit, against a float64 driver around oracle.unet22_ref.unet22_forward, the refusals of the new loop entry,
and Kandinsky2_2HIP(sampler=).  Everything runs on tiny_unet22_config() at 16 x 16 latents with at most 6 steps.

PARITY UNPINNED (tests/decoder22_dpm_ref.py): the sampler has no counterpart in the reference and has never run on trained 2.2 weights.
Equal bits alone would also hold if whole_loop_graph= were ignored: the "loop_captures" / "loop_launches" counters show which route ran.
Nothing here skips when a symbol or keyword is missing: every test reaches for the new entry points and fails without them."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decoder22_dpm_ref as D
import dpmpp_ref as R
import kandinsky2_amd as k22
from kandinsky2_amd import _lib, pipeline22, sampling
from oracle import prestep_ref, unet22_ref

pytestmark = pytest.mark.gpu

AC = D.schedule_2_2()
GUARD = 1024
SCHED = {"config_2_2": k22.SCHEDULER_CONFIG_2_2, "learned_range": k22.SCHEDULER_CONFIG_2_2_LEARNED_RANGE}
CLIP = {"config_2_2": D.NO_CLIP, "learned_range": (-2.0, 2.0)}
SA, SB = float(np.float32(0.8311 ** 0.5)), float(np.float32((1 - 0.8311) ** 0.5))      # a mid-loop keep-region pair
H16 = W16 = 16
_UNETS = {}


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


def _oracle(cfg, sd, emb, hint2=None):
    """model(x_in, t) of the float64 drivers: the CPU restatement of the UNet on the CFG batch [cond | uncond]"""
    return lambda xx, t: unet22_ref.unet22_forward(sd, cfg, xx.float(), t, emb, hint2)


# ---- 1. the step kernel against float64 ------------------------------------------------------------------------------------------------------
def _real_rows():
    """float64 rows of the first (t = 999, alpha_s = 0.040), a middle and the last step of the real S = 20 table"""
    table, _ = sampling.dpmpp_table(*R.integer_grid(AC, sampling.dpmpp_grid(AC, 20, "logsnr")), lower_order_final=False)
    return [table[0], table[10], table[19]]


@pytest.mark.parametrize("N,HW", [(2, 1), (4, 257), (2, 66000)])
def test_dpmpp_step_clip_kernel_within_the_derived_bound_of_float64(N, HW):
    """use_cfg 0 / 1, x0_prev NULL / given, clamp +-2, three rows of the real table; every buffer sits between NaN guards and the outputs are
    NaN-prefilled.  (2, 66000) is past the 2048 blocks the launch is capped at.  At HW >= 257 the middle and the last row clamp between a
    tenth and nine tenths of x0 (float64: 0.67 and 0.19 - 0.20), so both sides of the clamp are exercised; the first row clamps about 0.99.
    Measured worst |kernel - float64| / bound on an MI355X: x_out 0.31, x0_out 0.43 (profiles/decoder22_dpm.txt)."""
    L, st = _lib.lib(), _lib.current_stream()
    d = R.step_inputs(N, HW, seed=N + HW)
    n = N * 4 * HW
    worst = [0.0, 0.0]
    for i, row in enumerate(_real_rows()):
        row_dev = torch.from_numpy(row.astype(np.float32)).cuda()
        for use_cfg in (0, 1):
            for with_prev in (False, True):
                bufs = {k: R.with_guard(d[k], GUARD).cuda() for k in ("x", "model_out", "x0_prev")}
                outs = [torch.full((n + 2 * GUARD,), R.NAN, device="cuda") for _ in range(2)]
                ptr = lambda t: t.data_ptr() + 4 * GUARD  # noqa: E731
                rc = L.k22_dpmpp_step_clip(ptr(bufs["x"]), ptr(bufs["model_out"]), ptr(bufs["x0_prev"]) if with_prev else None, row_dev.data_ptr(),
                                           4.0, use_cfg, -2.0, 2.0, ptr(outs[0]), ptr(outs[1]), N, HW, st)
                assert rc == 0, L.k22_last_error()
                torch.cuda.synchronize()
                ref, x0, S, S0, share = D.step64_clip(d["x"], d["model_out"], d["x0_prev"] if with_prev else None, row, 4.0, use_cfg, (-2.0, 2.0))
                if HW >= 257 and i > 0:
                    assert 0.1 <= share <= 0.9, (i, use_cfg, share)
                for j, (o, want, bound) in enumerate(((outs[0], ref, R.bound_out(S)), (outs[1], x0, R.bound_x0(S0)))):
                    o = o.cpu()
                    assert torch.isnan(o[:GUARD]).all() and torch.isnan(o[-GUARD:]).all(), "wrote outside its output"
                    got = o[GUARD:-GUARD].reshape(want.shape)
                    worst[j] = max(worst[j], R.worst_ratio(got, want, bound))
                    assert R.violations(got, want, bound) == 0, (N, HW, row[0], use_cfg, with_prev, j, R.worst_ratio(got, want, bound))
                got0 = outs[1][GUARD:-GUARD]
                assert got0.abs().max().item() <= 2.0
                if HW >= 257:
                    assert (got0 == 2.0).any() and (got0 == -2.0).any() and (got0.abs() < 2.0).any()
                for k in bufs:                                                       # the inputs stay as they were
                    assert torch.equal(bufs[k][GUARD:-GUARD].cpu(), d[k].reshape(-1))
    print(f"dpmpp_step_clip N={N} HW={HW}: worst |kernel - float64| / bound: x_out {worst[0]:.3f}, x0_out {worst[1]:.3f}")


@pytest.mark.parametrize("N,HW", [(4, 257), (2, 66000)])
def test_no_clip_bounds_give_the_bits_of_dpmpp_step(N, HW):
    L, st = _lib.lib(), _lib.current_stream()
    d = {k: v.cuda() for k, v in R.step_inputs(N, HW, seed=7).items()}
    d["x"][0, 0, 0] = float("nan")                       # a NaN passes through both
    for row in _real_rows():
        row_dev = torch.from_numpy(row.astype(np.float32)).cuda()
        for use_cfg in (0, 1):
            for prev in (None, d["x0_prev"]):
                a, a0, b, b0 = (torch.full_like(d["x"], 7.0) for _ in range(4))
                assert L.k22_dpmpp_step(d["x"].data_ptr(), d["model_out"].data_ptr(), _lib.ptr(prev), row_dev.data_ptr(), 4.0, use_cfg,
                                        a.data_ptr(), a0.data_ptr(), N, HW, st) == 0
                assert L.k22_dpmpp_step_clip(d["x"].data_ptr(), d["model_out"].data_ptr(), _lib.ptr(prev), row_dev.data_ptr(), 4.0, use_cfg,
                                             D.NO_CLIP[0], D.NO_CLIP[1], b.data_ptr(), b0.data_ptr(), N, HW, st) == 0
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a0.view(torch.int32), b0.view(torch.int32))
                assert torch.isnan(b0[0, 0, 0]) and torch.isfinite(b0[0, 0, 1:]).all()


def test_dpmpp_step_clip_refusals():
    L, st = _lib.lib(), _lib.current_stream()
    a, b, c = (torch.zeros(2 * 4 * 16, device="cuda") for _ in range(3))
    mo, row = torch.zeros(2 * 8 * 16, device="cuda"), torch.ones(5, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    nan = float("nan")
    ok = (p(a), p(mo), None, p(row), 4.0, 1, -2.0, 2.0, p(b), p(c), 2, 16, st)
    assert L.k22_dpmpp_step_clip(*ok) == 0
    assert L.k22_dpmpp_step_clip(*(ok[:6] + (2.0, 2.0) + ok[8:])) == 0                       # lo == hi is a clamp
    for args in ((p(a), p(mo), None, p(row), 4.0, 1, -2.0, 2.0, p(a), p(b), 2, 16, st),      # what k22_dpmpp_step refuses: x_out == x,
                 (p(a), p(mo), p(c), p(row), 4.0, 1, -2.0, 2.0, p(b), p(c), 2, 16, st),      # x0_prev == x0_out,
                 (p(a), p(mo), None, p(row), 4.0, 1, -2.0, 2.0, p(b), p(c), 1, 16, st),      # an odd CFG batch,
                 (p(a), p(mo), None, p(row), 4.0, 1, -2.0, 2.0, p(b), None, 2, 16, st),      # no x0_out,
                 (None, p(mo), None, p(row), 4.0, 1, -2.0, 2.0, p(b), p(c), 2, 16, st),
                 (p(a), p(mo), None, p(row), 4.0, 1, -2.0, 2.0, p(b), p(c), 2, 0, st),
                 ok[:6] + (2.0, -2.0) + ok[8:], ok[:6] + (nan, 2.0) + ok[8:], ok[:6] + (-2.0, nan) + ok[8:]):
        assert L.k22_dpmpp_step_clip(*args) == -1 and b"dpmpp_step_clip" in L.k22_last_error(), args
    torch.cuda.synchronize()


# ---- 2. text2img and ControlNet-depth ---------------------------------------------------------------------------------------------------------
def _t2i_inputs(bs, controlnet, seed=6):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(bs, 4, H16, W16, generator=g)
    pos, neg = torch.randn(bs, 1280, generator=g), torch.randn(bs, 1280, generator=g)
    hint = torch.rand(bs, 3, 8 * H16, 8 * W16, generator=g) if controlnet else None
    return lat, pos, neg, hint


def _t2i(m, variant, whole, inp, steps=6, gs=4.0, solver_order=2, sampler="dpm_sampler", lat=None):
    """(final latent, decoder) of one text2img generation"""
    lat0, pos, neg, hint = inp
    dec = pipeline22.KandinskyV22DecoderHIP(m, None, scheduler=k22.DDPMSchedulerHIP.from_config(SCHED[variant]), whole_loop_graph=whole,
                                            sampler=sampler, solver_order=solver_order)
    out = dec(pos.cuda(), neg.cuda(), height=8 * H16, width=8 * W16, num_inference_steps=steps, guidance_scale=gs,
              hint=None if hint is None else hint.cuda(), latents=(lat0 if lat is None else lat).cuda(), output_type="latent")
    return out, dec


@pytest.mark.parametrize("variant", list(SCHED))
@pytest.mark.parametrize("controlnet,backend", [(False, torch.float32), (True, torch.float32), (False, torch.bfloat16)])
def test_text2img_graph_equals_stepwise_replays_and_recaptures(controlnet, backend, variant):
    """bs 2, 6 steps (999, 794, 537, 246, 61, 8): one graph gives the stepwise route's bits - final latent and last x0 - and the counters show
    which route ran; a second generation replays; another solver_order or guidance re-captures."""
    cfg, sd, m = _unet("controlnet" if controlnet else "plain", backend)
    inp = _t2i_inputs(2, controlnet)
    c0 = _counters()
    step, dstep = _t2i(m, variant, False, inp)
    assert _counters() == c0                                              # the stepwise route is no loop
    whole, dwhole = _t2i(m, variant, True, inp)
    c1 = _counters()
    assert c1[1] == c0[1] + 1 and c1[0] - c0[0] in (0, 1)                 # 0: this module's cached loop was this very one
    assert torch.equal(step, whole), (step - whole).abs().max().item()
    assert torch.equal(dstep.last_x0, dwhole.last_x0) and dstep.last_timesteps == dwhole.last_timesteps == [999, 794, 537, 246, 61, 8]
    assert torch.isfinite(whole).all() and not torch.equal(whole, dwhole.last_x0)
    if variant == "learned_range":
        assert dwhole.last_x0.abs().max().item() <= 2.0
    other_lat = torch.randn(2, 4, H16, W16, generator=torch.Generator().manual_seed(61))
    again, _ = _t2i(m, variant, True, inp, lat=other_lat)
    assert _counters() == (c1[0], c1[1] + 1) and not torch.equal(again, whole)      # a replay, and it read the new x_T
    assert torch.equal(again, _t2i(m, variant, False, inp, lat=other_lat)[0])
    o1, _ = _t2i(m, variant, True, inp, solver_order=1)
    assert _counters() == (c1[0] + 1, c1[1] + 2) and not torch.equal(o1, whole)
    assert torch.equal(o1, _t2i(m, variant, False, inp, solver_order=1)[0])
    g2, _ = _t2i(m, variant, True, inp, gs=3.25)
    assert _counters() == (c1[0] + 2, c1[1] + 3) and not torch.equal(g2, whole)
    assert torch.equal(g2, _t2i(m, variant, False, inp, gs=3.25)[0])


def _checked_steps(monkeypatch, table64, guidance, clamp):
    """wraps sampling.dpmpp_step: every launch's outputs against step64_clip on the launch's OWN device operands, under the step bounds"""
    launch, seen, worst = sampling.dpmpp_step, [], [0.0, 0.0]

    def checked(x, model_out, x0_prev, row, x_out, x0_out, **kw):
        k = len(seen)
        launch(x, model_out, x0_prev, row, x_out, x0_out, **kw)
        seen.append(x0_prev is not None)
        assert kw["clamp"] == clamp and torch.equal(row.cpu(), torch.from_numpy(table64[k].astype(np.float32)))
        ref, x0, S, S0, _ = D.step64_clip(x.cpu(), model_out.cpu(), None if x0_prev is None else x0_prev.cpu(), table64[k], guidance, 1, clamp)
        for j, (o, want, bound) in enumerate(((x_out, ref, R.bound_out(S)), (x0_out, x0, R.bound_x0(S0)))):
            worst[j] = max(worst[j], R.worst_ratio(o.cpu(), want, bound))
            assert R.violations(o.cpu(), want, bound) == 0, (k, j)

    monkeypatch.setattr(sampling, "dpmpp_step", checked)
    return seen, worst


@pytest.mark.parametrize("controlnet,variant", [(False, "config_2_2"), (False, "learned_range"), (True, "learned_range")])
def test_text2img_meets_the_float64_driver_and_every_step_its_bound(monkeypatch, controlnet, variant):
    """the fp32 engine, stepwise, 6 steps (orders 1 2 2 2 2 1), against decoder22_dpm_ref.dpmpp_loop64_clip around the oracle UNet: 1e-3 of the
    latent scale, the bound of test_dpmpp_gpu.py's order-2 test.  Measured on an MI355X (profiles/decoder22_dpm.txt): no clip 2.1e-4 at a scale
    of 167, clip +-2 1.3e-4 at 2.1, ControlNet 1.2e-4 at 2.1; per step worst 0.26 / 0.34 of the step bounds."""
    cfg, sd, m = _unet("controlnet" if controlnet else "plain")
    inp = _t2i_inputs(2, controlnet)
    lat, pos, neg, hint = inp
    ts, table64, orders = sampling.dpmpp_schedule(AC, 6)
    seen, worst = _checked_steps(monkeypatch, table64, 4.0, CLIP[variant])
    out, dec = _t2i(m, variant, False, inp)
    assert seen == [False, True, True, True, True, False] and list(orders) == [1, 2, 2, 2, 2, 1]
    hint2 = None if hint is None else torch.cat([hint, hint], 0)
    want, want0 = D.dpmpp_loop64_clip(_oracle(cfg, sd, torch.cat([pos, neg], 0), hint2), torch.cat([lat, lat], 0), ts, table64, orders, 4.0,
                                      CLIP[variant])
    scale, scale0 = want.abs().max().item(), want0.abs().max().item()
    err, err0 = (out.cpu().double() - want[:2]).abs().max().item(), (dec.last_x0.cpu().double() - want0[:2]).abs().max().item()
    print(f"2.2 dpm_sampler text2img {'controlnet ' if controlnet else ''}{variant} fp32 vs float64 driver (oracle unpinned): final max|d|={err:.3e} "
          f"(scale {scale:.2f}), last x0 max|d|={err0:.3e} (scale {scale0:.2f}); per step worst |kernel - float64| / bound: x_out {worst[0]:.3f}, "
          f"x0_out {worst[1]:.3f}")
    assert err <= 1e-3 * max(1.0, scale) and err0 <= 1e-3 * max(1.0, scale0)


# ---- 3. img2img ----------------------------------------------------------------------------------------------------------------------------------
def test_img2img_starts_at_the_grid_keeps_to_init_step_and_meets_the_float64_driver(monkeypatch):
    """6 steps at strength 0.5: init_step 332, the grid keeps [246, 61, 8]; the image latents are noised at t = 246"""
    cfg, sd, m = _unet("plain")
    bs, steps, strength, gs = 2, 6, 0.5, 4.0
    g = torch.Generator().manual_seed(10)
    lat0 = torch.randn(1, 4, H16, W16, generator=g).repeat(bs, 1, 1, 1)
    pos, neg, nz0 = torch.randn(bs, 1280, generator=g), torch.randn(bs, 1280, generator=g), torch.randn(bs, 4, H16, W16, generator=g)
    calls, forward = [], m.forward

    def recording(sample, timestep, **kw):
        calls.append((float(torch.as_tensor(timestep).reshape(-1)[0]), sample[:bs, :4].clone()))
        return forward(sample, timestep, **kw)

    outs, decs = {}, {}
    for whole in (False, True):
        dec = pipeline22.KandinskyV22Img2ImgDecoderHIP(m, None, None, scheduler=k22.DDPMSchedulerHIP.from_config(SCHED["learned_range"]),
                                                       whole_loop_graph=whole, sampler="dpm_sampler")
        if not whole:
            monkeypatch.setattr(m, "forward", recording)
        c0 = _counters()
        outs[whole] = dec(pos.cuda(), neg.cuda(), image=lat0.cuda(), height=8 * H16, width=8 * W16, num_inference_steps=steps, guidance_scale=gs,
                          strength=strength, noise=nz0.cuda(), output_type="latent")
        assert _counters()[1] - c0[1] == (1 if whole else 0)
        monkeypatch.setattr(m, "forward", forward)
        decs[whole] = dec
    init_step = decs[True].get_timesteps(steps, strength)[0]
    assert init_step == 332 and decs[False].last_timesteps == decs[True].last_timesteps == [246, 61, 8]
    assert [c[0] for c in calls] == [246.0, 61.0, 8.0] and max(c[0] for c in calls) <= init_step
    start = decs[True].scheduler.add_noise(lat0.cuda(), nz0.cuda(), 246)
    assert torch.equal(calls[0][1], start)                                # the start latent is add_noise at the grid's first timestep
    start64 = np.sqrt(AC[246]) * lat0.double() + np.sqrt(1.0 - AC[246]) * nz0.double()
    assert (start.cpu().double() - start64).abs().max().item() <= 1e-6
    assert torch.equal(outs[False], outs[True]) and torch.equal(decs[False].last_x0, decs[True].last_x0)
    ts, table64, orders = sampling.dpmpp_schedule(AC, steps, init_step=init_step)
    want, want0 = D.dpmpp_loop64_clip(_oracle(cfg, sd, torch.cat([pos, neg], 0)), torch.cat([start64, start64], 0), ts, table64, orders, gs, (-2.0, 2.0))
    scale = want.abs().max().item()
    err, err0 = (outs[True].cpu().double() - want[:bs]).abs().max().item(), (decs[True].last_x0.cpu().double() - want0[:bs]).abs().max().item()
    print(f"2.2 dpm_sampler img2img fp32 vs float64 driver (oracle unpinned): final max|d|={err:.3e} (scale {scale:.2f}), last x0 max|d|={err0:.3e}")
    assert err <= 1e-3 * max(1.0, scale) and err0 <= 1e-3 * max(1.0, want0.abs().max().item())
    with pytest.raises(ValueError, match="strength too small"):
        decs[True](pos.cuda(), neg.cuda(), image=lat0.cuda(), height=8 * H16, width=8 * W16, num_inference_steps=steps, strength=0.0,
                   noise=nz0.cuda(), output_type="latent")


# ---- 4. inpainting -------------------------------------------------------------------------------------------------------------------------------
def _inpaint_inputs(bs=2):
    g = torch.Generator().manual_seed(11)
    lat0 = torch.randn(1, 4, H16, W16, generator=g)
    mask_px = torch.ones(8 * H16, 8 * W16)
    mask_px[24:90, 40:100] = 0.0
    pos, neg = torch.randn(bs, 1280, generator=g), torch.randn(bs, 1280, generator=g)
    x_T = torch.randn(bs, 4, H16, W16, generator=g)
    mlat = prestep_ref.prepare_mask(F.interpolate(mask_px[None, None], (H16, W16), mode="nearest"))
    return lat0, mask_px, mlat, pos, neg, x_T


def _inpaint(m, whole, inp, steps=6, gs=4.0):
    lat0, mask_px, mlat, pos, neg, x_T = inp
    dec = pipeline22.KandinskyV22InpaintDecoderHIP(m, None, None, scheduler=k22.DDPMSchedulerHIP.from_config(SCHED["learned_range"]),
                                                   whole_loop_graph=whole, sampler="dpm_sampler")
    out = dec(pos.cuda(), neg.cuda(), image=lat0.cuda(), mask_image=mask_px.numpy(), height=8 * H16, width=8 * W16, num_inference_steps=steps,
              guidance_scale=gs, latents=x_T.cuda(), output_type="latent")
    return out, dec


def test_inpainting_graph_equals_stepwise_the_known_region_and_the_eager_entry():
    """9-channel tiny UNet, bs 2, 6 steps: both routes re-impose with k22_keep_region, so they agree bit for bit; the known region ends within
    1e-5 of the image latents; the captured loop equals the same entry with use_graph = 0; the fp32 engine within 1e-3 of the float64 driver."""
    cfg9, sd, m = _unet("inpaint")
    inp = _inpaint_inputs()
    lat0, mask_px, mlat, pos, neg, x_T = inp
    c0 = _counters()
    step, dstep = _inpaint(m, False, inp)
    assert _counters() == c0
    got, dgot = _inpaint(m, True, inp)
    c1 = _counters()
    assert c1[1] == c0[1] + 1 and c1[0] - c0[0] in (0, 1)
    assert torch.equal(step, got) and torch.equal(dstep.last_x0, dgot.last_x0)
    keep = mlat[0, 0] == 1
    assert keep.any() and (~keep).any()
    kerr = (got.cpu()[:, :, keep] - lat0[:, :, keep]).abs().max().item()
    assert kerr <= 1e-5 and not torch.equal(got.cpu()[:, :, ~keep], lat0.expand(2, -1, -1, -1)[:, :, ~keep])
    _, _, eager_m = _unet("inpaint", use_graph=False)
    c2 = _counters()
    eager, _ = _inpaint(eager_m, True, inp)              # whole_loop_graph=True on a use_graph=False module: the same launches, eagerly
    assert _counters() == (c2[0], c2[1] + 1) and torch.equal(got, eager)
    ts, table64, orders = sampling.dpmpp_schedule(AC, 6)
    coef = sampling.dpmpp_keep_coef(AC, ts)
    extra = torch.cat([lat0 * mlat, mlat], 1).repeat(4, 1, 1, 1)
    want, _ = D.dpmpp_loop64_clip(_oracle(cfg9, sd, torch.cat([pos, neg], 0)), torch.cat([x_T, x_T], 0), ts, table64, orders, 4.0, (-2.0, 2.0),
                                  extra=extra, keep=(lat0, x_T, mlat, coef))
    scale = want.abs().max().item()
    err = (got.cpu().double() - want[:2]).abs().max().item()
    print(f"2.2 dpm_sampler inpainting fp32 vs float64 driver (oracle unpinned): final max|d|={err:.3e} (scale {scale:.2f}); known region "
          f"{kerr:.3e} from the image latents")
    assert err <= 1e-3 * max(1.0, scale)


def test_inpainting_loop_step_is_unet_then_step_clip_then_keep_region_bit_for_bit():
    """the chain launch by launch: a one-step loop equals k22_unet_forward -> k22_dpmpp_step_clip -> k22_keep_region on the same device
    operands, with a mid-loop coefficient pair (the last row's (1, 0) would hide the noise operand) and different latents in the two CFG
    halves, whose unknown regions stay their own"""
    cfg9, sd, m = _unet("inpaint")
    lat0, mask_px, mlat, pos, neg, x_T = _inpaint_inputs()
    bs = 2
    ts, table64, orders = sampling.dpmpp_schedule(AC, 6)
    t, row = float(ts[3]), torch.from_numpy(table64[3].astype(np.float32)).cuda()          # a mid-loop row, run as an order-1 step
    ts_rows = torch.full((1, 2 * bs), t, device="cuda")
    coef = np.array([[SA, SB]], dtype=np.float32)
    emb = torch.cat([pos, neg], 0).cuda()
    x2 = torch.cat([x_T, torch.randn(bs, 4, H16, W16, generator=torch.Generator().manual_seed(5))], 0).cuda()
    lat0c, mc, noise0 = lat0.cuda(), mlat.cuda(), x_T.cuda()
    masked = (lat0c * mc).expand(2 * bs, 4, H16, W16).contiguous()
    mask_b = mc.expand(2 * bs, 1, H16, W16).contiguous()
    got, got0 = m.dpmpp_loop(x2, ts_rows, row[None], [1], 4.0, (-2.0, 2.0), image_embeds=emb, inpaint_image=masked, inpaint_mask=mask_b,
                             keep=(lat0c, noise0, mc, coef))
    out = m(torch.cat([sampling.cfg_input(x2), masked, mask_b], 1), t, added_cond_kwargs={"image_embeds": emb}, return_dict=False)[0]
    x_next, x0 = torch.empty_like(x2), torch.empty_like(x2)
    sampling.dpmpp_step(x2, out, None, row, x_next, x0, guidance=4.0, clamp=(-2.0, 2.0))
    before = x_next.clone()
    sampling.keep_region(x_next, lat0c.reshape(4, H16, W16).contiguous(), noise0.contiguous(), mc.reshape(H16, W16).contiguous(), SA, SB, x_next)
    assert torch.equal(got, x_next) and torch.equal(got0, x0) and not torch.equal(before, x_next)
    assert x0.abs().max().item() <= 2.0 and (x0.abs() == 2.0).any() and (x0.abs() < 2.0).any()
    keep = (mlat[0, 0] == 1).cuda()
    assert torch.equal(got[:bs][:, :, keep], got[bs:][:, :, keep])                   # the known region is the same in both halves,
    assert not torch.equal(got[:bs][:, :, ~keep], got[bs:][:, :, ~keep])              # the halves keep their own unknown region
    want_known = SA * lat0c + SB * noise0
    assert (got[:bs][:, :, keep] - want_known[:, :, keep]).abs().max().item() <= 1e-5


def test_two_chain_mode_falls_back_to_the_host_driven_loop(monkeypatch):
    """dpmpp_loop under _chained(B) drives the same steps from the host: no loop is counted, the captured loop's bits"""
    cfg, sd, m = _unet("plain")
    inp = _t2i_inputs(2, False, seed=16)
    graph, dg = _t2i(m, "learned_range", True, inp)
    cfg9, sd9, m9 = _unet("inpaint")
    inp9 = _inpaint_inputs()
    graph9, dg9 = _inpaint(m9, True, inp9)
    for mod in (m, m9):
        monkeypatch.setattr(mod, "_chained", lambda B: True)
    c0 = _counters()
    host, dh = _t2i(m, "learned_range", True, inp)
    host9, dh9 = _inpaint(m9, True, inp9)
    assert _counters() == c0
    assert torch.equal(host, graph) and torch.equal(dh.last_x0, dg.last_x0)
    assert torch.equal(host9, graph9) and torch.equal(dh9.last_x0, dg9.last_x0)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------
def _raw(m, bufs, good, coef0, **over):
    """k22_unet_dpmpp_loop_keep on the module's own operand buffers, single arguments overridden"""
    a = dict(x=bufs["x"].data_ptr(), tmp=bufs["tmp"].data_ptr(), hist=bufs["hist"].data_ptr(), ts=bufs["ts"].data_ptr(), table=bufs["table"].data_ptr(),
             orders=good, img=_lib.ptr(bufs["img"]), msk=_lib.ptr(bufs["msk"]), n=len(good), lo=-2.0, hi=2.0, kinit=_lib.ptr(bufs["kinit"]),
             knoise=_lib.ptr(bufs["knoise"]), kmask=_lib.ptr(bufs["kmask"]), coef=coef0.ctypes.data_as(C.POINTER(C.c_float)), hd=m._handle)
    a.update(over)
    arr = None if a["orders"] is None else (C.c_int * len(a["orders"]))(*a["orders"])
    return _lib.lib().k22_unet_dpmpp_loop_keep(a["hd"], a["x"], a["tmp"], a["hist"], a["ts"], a["table"], arr, a["img"], a["msk"], a["n"], 4.0, a["lo"],
                                               a["hi"], a["kinit"], a["knoise"], a["kmask"], a["coef"], 1, _lib.current_stream())


def test_refused_calls_leave_the_captured_loop_as_it_was():
    cfg9, sd, m = _unet("inpaint")
    inp = _inpaint_inputs()
    first, _ = _inpaint(m, True, inp)                  # captures (or replays) the 6-step keep loop of this module's buffers
    bufs = m._dpmpp22_bufs.bufs
    ts, _, orders = sampling.dpmpp_schedule(AC, 6)
    good, coef = [int(o) for o in orders], sampling.dpmpp_keep_coef(AC, ts)
    nan = float("nan")
    c0 = _counters()
    refused = [dict(kinit=None), dict(knoise=None), dict(kmask=None), dict(coef=None), dict(kinit=None, knoise=None, kmask=None),   # keep in part
               dict(lo=2.0, hi=-2.0), dict(lo=nan), dict(hi=nan),                                                                  # the clamp
               dict(img=None), dict(msk=None), dict(img=None, msk=None),                                                           # the 9-channel operands
               dict(orders=good[:2] + [3] + good[3:]), dict(orders=good[:-1] + [0]), dict(orders=[2] + good[1:]), dict(orders=None),
               dict(x=None), dict(tmp=None), dict(hist=None), dict(ts=None), dict(table=None), dict(n=0), dict(hd=None)]
    for over in refused:
        rc = _raw(m, bufs, good, coef, **over)
        msg = _lib.lib().k22_last_error().decode()
        assert rc == -1 and "unet_dpmpp_loop_keep" in msg, (over, rc, msg)            # K22_EINVAL
        assert _counters() == c0, over
    # an odd batch: a module of its own (planning another batch on `m` would drop its loop by itself)
    _, _, odd = _unet("plain")
    emb1 = torch.randn(1, 1280, generator=torch.Generator().manual_seed(1)).cuda()
    odd(torch.zeros(1, 4, H16, W16, device="cuda"), 10, added_cond_kwargs={"image_embeds": emb1})
    z = torch.zeros(6, 4, 4, H16, W16, device="cuda")
    rc = _lib.lib().k22_unet_dpmpp_loop_keep(odd._handle, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), (C.c_int * 6)(*good),
                                             None, None, 6, 4.0, -2.0, 2.0, None, None, None, None, 1, _lib.current_stream())
    assert rc == -1 and b"even" in _lib.lib().k22_last_error()
    assert _counters() == c0
    # the earlier capture still replays: no new capture, one launch, the same bits
    again, _ = _inpaint(m, True, inp)
    assert _counters() == (c0[0], c0[1] + 1) and torch.equal(first, again)


# ---- 6. the public pipeline ----------------------------------------------------------------------------------------------------------------------
def test_kandinsky2_2_generate_text2img_with_dpm_sampler():
    marc = k22.MoVQArch(k22.MOVQ_CONFIG_2_1["ddconfig"])
    msd = dict(k22.init_movq_state_dict(marc, seed=0))
    msd.update(k22.init_movq_encoder_state_dict(marc, seed=0))
    ucfg = k22.tiny_unet22_config()
    usd = k22.init_unet22_state_dict(k22.make_arch22(ucfg), seed=0)
    mdl = pipeline22.Kandinsky2_2HIP("cuda", "text2img", unet_state_dict=usd, movq_state_dict=msd, unet_config=ucfg, conditioner="seeded",
                                     backend_dtype=torch.float32)
    assert mdl.decoder.sampler == "ddpm_sampler"
    g = torch.Generator().manual_seed(5)
    lat, nz = torch.randn(1, 4, H16, W16, generator=g).cuda(), torch.randn(6, 1, 4, H16, W16, generator=g).cuda()
    kw = dict(batch_size=1, decoder_steps=6, prior_steps=3, h=8 * H16, w=8 * W16, latents=lat, output_type="latent")
    c0 = _counters()
    a = mdl.generate_text2img("a red cat", sampler="dpm_sampler", **kw)
    assert _counters() == (c0[0] + 1, c0[1] + 1)                          # one captured loop ...
    assert mdl.decoder.last_timesteps == [999, 794, 537, 246, 61, 8]      # ... of 6 model calls
    b = mdl.generate_text2img("a red cat", sampler="dpm_sampler", **kw)
    assert _counters() == (c0[0] + 1, c0[1] + 2)
    assert tuple(a.shape) == (1, 4, H16, W16) and torch.isfinite(a).all() and torch.equal(a, b)
    ddpm = mdl.generate_text2img("a red cat", noise_seq=nz, **kw)
    assert not torch.equal(a, ddpm)
    with pytest.raises(ValueError, match="deterministic"):
        mdl.generate_text2img("a red cat", sampler="dpm_sampler", noise_seq=nz, **kw)
    with pytest.raises(ValueError, match="sampler must be one of"):
        mdl.generate_text2img("a red cat", sampler="ddim_sampler", **kw)
    mix = mdl.mix_images(["a red cat", "a dog"], [0.5, 0.5], batch_size=1, decoder_steps=6, prior_steps=3, h=8 * H16, w=8 * W16, latents=lat,
                         output_type="latent", sampler="dpm_sampler")
    assert torch.isfinite(mix).all() and not torch.equal(mix, a)
    dflt = pipeline22.Kandinsky2_2HIP("cuda", "text2img", unet_state_dict=usd, movq_state_dict=msd, unet_config=ucfg, conditioner="seeded",
                                      backend_dtype=torch.float32, sampler="dpm_sampler")
    assert torch.equal(dflt.generate_text2img("a red cat", **kw), a)
