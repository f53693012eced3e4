"""The DPM-Solver++ sampler on the GPU: k22_dpmpp_step against float64 under the derived bound of tests/dpmpp_ref.py, the sampler class
against the reference's DDIM golden (order 1 on the reference's grid IS eta = 0 DDIM) and against a float64 driver around the CPU oracle
UNet (order 2), the whole loop as one captured graph (k22_unet_dpmpp_loop) against the stepwise route bit for bit, the refusals of the C
entry, and the public pipeline (sampler="dpm_sampler").

Nothing here skips when a symbol or class is missing: every test reaches for the new entry points and fails without them.

Shapes: the tiny fixtures' 128-channel UNet at 16x16 (CFG batch 2) and, for the inpainting UNet, 16x24 (CFG batch 4), at most 8 steps.
"""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dpmpp_ref as R
import kandinsky2_amd as k22
from kandinsky2_amd import _lib, sampling
from oracle import unet_ref

pytestmark = pytest.mark.gpu

AC = R.schedule_2_1()
GUARD = 1024


def _load(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name + ".pt"), weights_only=False)


def _counters():
    L = _lib.lib()
    return L.k22_debug_counter(b"loop_captures"), L.k22_debug_counter(b"loop_launches")


def _model(fx, backend, use_graph=True, chains=None):
    """module + conditioning built as tests/test_sampler_loop_gpu.py does"""
    inp = bool(fx.get("inpainting", False))
    arch = k22.make_arch(fx["model_config"], inpainting=inp)
    m = k22.Text2ImUNetHIP(arch, backend_dtype=backend, use_graph=use_graph, chains=chains)
    m.load_state_dict(k22.init_unet_state_dict(arch, seed=fx["seed_w"]))
    m = m.to("cuda").eval()
    full, pooled, image = k22.make_conditioning(arch, fx["B"], seed=2)
    kw = dict(full_emb=full.cuda(), pooled_emb=pooled.cuda(), image_emb=image.cuda())
    if inp:
        g = torch.Generator().manual_seed(3)
        img = torch.randn(fx["B"], 4, fx["h"], fx["w"], generator=g)
        mask = (torch.rand(fx["B"], 1, fx["h"], fx["w"], generator=g) > 0.5).float()
        kw.update(inpaint_image=(img * mask).cuda(), inpaint_mask=mask.cuda())
    return m, kw


def _x_T(fx, seed):
    return torch.randn(fx["B"], 4, fx["h"], fx["w"], generator=torch.Generator().manual_seed(seed)).cuda()


def _sampler(m, fx):
    return k22.DPMSolverSamplerHIP(m, k22.create_gaussian_diffusion(**k22.DIFFUSION_CONFIG_2_1), fx["guidance"])


def _sample(m, fx, kw, x_T, whole, S=6, sampler=None, **extra):
    """(final latent, pred_x0) of one generation; the conditioning cache is dropped first, as generate_img does"""
    m.del_cache()
    sm = _sampler(m, fx) if sampler is None else sampler
    out, aux = sm.sample(S, fx["B"], (4, fx["h"], fx["w"]), conditioning=kw, x_T=x_T, whole_loop_graph=whole, **extra)
    return out, aux["pred_x0"][0]


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 6. the step kernel against float64 ------------------------------------------------------------------------------------------------
def _real_rows():
    """float64 rows of the first (t = 999, alpha_s = 0.040), a middle and the last step of the real S = 20 table"""
    table, _ = sampling.dpmpp_table(*R.integer_grid(AC, sampling.dpmpp_grid(AC, 20, "logsnr")), lower_order_final=False)
    return [table[0], table[10], table[19]]


@pytest.mark.parametrize("N,HW", [(2, 1), (4, 257), (2, 66000)])
def test_dpmpp_step_kernel_within_the_derived_bound_of_float64(N, HW):
    """use_cfg 0 / 1, x0_prev NULL / given, three rows of the real table; every buffer sits between NaN guards and the outputs are
    NaN-prefilled, so a read or write out of range or an element left unwritten shows.  (2, 66000) is 2062.5 blocks' worth: past the 2048
    the launch is capped at, so the stride loop runs.  Measured worst |kernel - float64| / bound on an MI355X: x_out 0.36, x0_out 0.49
    (DESIGN.md section 5)."""
    L, st = _lib.lib(), _lib.current_stream()
    d = R.step_inputs(N, HW, seed=N + HW)
    n = N * 4 * HW
    worst = [0.0, 0.0]
    for row in _real_rows():
        row_dev = torch.from_numpy(row.astype(np.float32)).cuda()
        for use_cfg in (0, 1):
            for with_prev in (False, True):
                bufs = {k: R.with_guard(d[k], GUARD).cuda() for k in ("x", "model_out", "x0_prev")}
                outs = [torch.full((n + 2 * GUARD,), R.NAN, device="cuda") for _ in range(2)]
                ptr = lambda t: t.data_ptr() + 4 * GUARD  # noqa: E731
                rc = L.k22_dpmpp_step(ptr(bufs["x"]), ptr(bufs["model_out"]), ptr(bufs["x0_prev"]) if with_prev else None, row_dev.data_ptr(),
                                      4.0, use_cfg, ptr(outs[0]), ptr(outs[1]), N, HW, st)
                assert rc == 0, L.k22_last_error()
                torch.cuda.synchronize()
                ref, x0, S, S0 = R.step64(d["x"], d["model_out"], d["x0_prev"] if with_prev else None, row, 4.0, use_cfg)
                for j, (o, want, bound) in enumerate(((outs[0], ref, R.bound_out(S)), (outs[1], x0, R.bound_x0(S0)))):
                    o = o.cpu()
                    assert torch.isnan(o[:GUARD]).all() and torch.isnan(o[-GUARD:]).all(), "wrote outside its output"
                    got = o[GUARD:-GUARD].reshape(want.shape)
                    worst[j] = max(worst[j], R.worst_ratio(got, want, bound))
                    assert R.violations(got, want, bound) == 0, (N, HW, row[0], use_cfg, with_prev, j, R.worst_ratio(got, want, bound))
    print(f"dpmpp_step N={N} HW={HW}: worst |kernel - float64| / bound: x_out {worst[0]:.3f}, x0_out {worst[1]:.3f}")


def test_dpmpp_step_refuses_aliased_buffers_and_an_odd_cfg_batch():
    L, st = _lib.lib(), _lib.current_stream()
    a, b, c = (torch.zeros(2 * 4 * 16, device="cuda") for _ in range(3))
    mo, row = torch.zeros(2 * 8 * 16, device="cuda"), torch.ones(5, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    for args in ((p(a), p(mo), None, p(row), 4.0, 1, p(a), p(b), 2, 16, st), (p(a), p(mo), p(c), p(row), 4.0, 1, p(b), p(c), 2, 16, st),
                 (p(a), p(mo), None, p(row), 4.0, 1, p(b), p(c), 1, 16, st), (p(a), p(mo), None, p(row), 4.0, 1, p(b), None, 2, 16, st)):
        assert L.k22_dpmpp_step(*args) == -1 and b"dpmpp_step" in L.k22_last_error()


# ---- 7. order 1 on the reference's grid against the reference's DDIM golden ----------------------------------------------------------------
@pytest.mark.parametrize("whole", [False, True])
def test_order_1_on_the_uniform_grid_meets_the_reference_ddim_golden_fp32(golden_dir, whole):
    """tiny_ddim.pt: the reference DDIMSampler's final latent (5 steps, eta 0); bound of the DDIM test itself"""
    fx = _load(golden_dir, "tiny_ddim")
    m, kw = _model(fx, torch.float32)
    out, _ = _sample(m, fx, kw, _x_T(fx, 42), whole, S=fx["steps"], solver_order=1, discretize="uniform")
    ref = fx["final"]
    scale = ref.abs().max().item()
    err = (out.cpu() - ref).abs().max().item()
    print(f"DPM++ order 1, uniform grid, {fx['steps']} steps, fp32 (whole loop: {whole}) vs the reference DDIM golden: max|d|={err:.3e} scale={scale:.2f}")
    assert err <= 1e-3 * max(1.0, scale)


# ---- 8. order 2 against the float64 driver around the CPU oracle UNet ------------------------------------------------------------------------
def test_order_2_on_the_logsnr_grid_meets_the_float64_driver_and_every_step_its_bound(golden_dir):
    """tiny_ddim.pt's weights, S = 6 (timesteps 999, 794, 537, 246, 61, 8; orders 1 2 2 2 2 1), stepwise on the fp32 engine.  Measured on an
    MI355X: final latent 1.9e-4 from the float64 driver at a scale of 154 (bound 0.154), pred_x0 1.9e-4; per step worst 0.19 / 0.28 of the step
    bounds."""
    fx = _load(golden_dir, "tiny_ddim")
    arch = k22.make_arch(fx["model_config"])
    sd = k22.init_unet_state_dict(arch, seed=fx["seed_w"])
    full, pooled, image = k22.make_conditioning(arch, fx["B"], seed=2)
    m, kw = _model(fx, torch.float32)
    sm = _sampler(m, fx)
    launch, worst, seen = sm._dpm_step, [0.0, 0.0], []

    def checked_step(x, model_out, x0_prev, row, x_out, x0_out):
        k = len(seen)
        launch(x, model_out, x0_prev, row, x_out, x0_out)
        seen.append(x0_prev is not None)
        assert torch.equal(row.cpu(), torch.from_numpy(sm.dpm_table[k].astype(np.float32)))
        ref, x0, S, S0 = R.step64(x.cpu(), model_out.cpu(), None if x0_prev is None else x0_prev.cpu(), sm.dpm_table[k], fx["guidance"])
        for j, (o, want, bound) in enumerate(((x_out, ref, R.bound_out(S)), (x0_out, x0, R.bound_x0(S0)))):
            worst[j] = max(worst[j], R.worst_ratio(o.cpu(), want, bound))
            assert R.violations(o.cpu(), want, bound) == 0, (k, j)

    sm._dpm_step = checked_step
    x_T = _x_T(fx, 42)
    out, x0 = _sample(m, fx, kw, x_T, False, S=6, sampler=sm)
    assert seen == [False, True, True, True, True, False] and list(sm.orders) == [1, 2, 2, 2, 2, 1] and len(sm.timesteps) == 6
    want, want0 = R.dpmpp_loop64(lambda xc, tt: unet_ref.unet_forward(sd, arch, xc.float(), tt, full, pooled, image), x_T.cpu(), sm.timesteps,
                                 sm.dpm_table, sm.orders, fx["guidance"])
    scale = want.abs().max().item()
    err, err0 = (out.cpu().double() - want).abs().max().item(), (x0.cpu().double() - want0).abs().max().item()
    print(f"DPM++ 2M, logsnr grid {list(sm.timesteps)}, fp32 vs float64 driver around the oracle UNet: final max|d|={err:.3e} (scale {scale:.2f}), "
          f"pred_x0 max|d|={err0:.3e}; per step worst |kernel - float64| / bound: x_out {worst[0]:.3f}, x0_out {worst[1]:.3f}")
    assert err <= 1e-3 * max(1.0, scale)
    assert err0 <= 1e-3 * max(1.0, want0.abs().max().item())


# ---- 9. one graph == stepwise, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", [torch.float32, torch.bfloat16])
def test_whole_loop_equals_the_stepwise_loop_and_the_second_generation_replays(golden_dir, backend):
    fx = _load(golden_dir, "tiny_ddim")
    m, kw = _model(fx, backend)
    xs = [_x_T(fx, 42), _x_T(fx, 43)]
    c0, l0 = _counters()
    step = [_sample(m, fx, kw, x, False) for x in xs]
    assert _counters() == (c0, l0)            # the stepwise path is no loop
    whole = [_sample(m, fx, kw, x, True) for x in xs]
    c1, l1 = _counters()
    assert (c1 - c0, l1 - l0) == (1, 2)
    for s, w in zip(step, whole):
        assert _same(s, w), (backend, (s[0] - w[0]).abs().max().item())
    assert not torch.equal(whole[0][0], whole[1][0])   # the replay read the new x_T
    assert torch.isfinite(whole[0][0]).all() and not torch.equal(whole[0][0], whole[0][1])
    # other orders: another capture, another result
    other = _sample(m, fx, kw, xs[0], True, lower_order_final=False)
    assert _counters() == (c1 + 1, l1 + 1)
    assert _same(other, _sample(m, fx, kw, xs[0], False, lower_order_final=False)) and not torch.equal(other[0], whole[0][0])
    m.use_graph = False
    eager = _sample(m, fx, kw, xs[0], True)
    assert _counters() == (c1 + 1, l1 + 2)
    assert _same(step[0], eager)


@pytest.mark.parametrize("backend", [torch.float32, torch.bfloat16])
def test_whole_loop_with_per_step_time_rows_equals_the_stepwise_loop(golden_dir, backend, monkeypatch):
    """K22_HOIST_TIME=0 (read when the engine is created): the captured loop keeps the per-call time-embedding / FiLM launches."""
    monkeypatch.setenv("K22_HOIST_TIME", "0")
    fx = _load(golden_dir, "tiny_ddim")
    m, kw = _model(fx, backend)
    x = _x_T(fx, 42)
    c0, l0 = _counters()
    step, whole = _sample(m, fx, kw, x, False), _sample(m, fx, kw, x, True)
    assert _counters() == (c0 + 1, l0 + 1)
    assert _same(step, whole)


@pytest.mark.parametrize("backend", [torch.float32, torch.bfloat16])
def test_inpainting_unet_loop_equals_stepwise(golden_dir, backend):
    fx = _load(golden_dir, "tiny_inpaint")
    assert (fx["B"], fx["h"], fx["w"]) == (4, 16, 24)
    m, kw = _model(fx, backend)
    x = _x_T(fx, 42)
    c0, l0 = _counters()
    step, whole = _sample(m, fx, kw, x, False), _sample(m, fx, kw, x, True)
    assert _counters() == (c0 + 1, l0 + 1)
    assert _same(step, whole)
    other = dict(kw, inpaint_mask=1.0 - kw["inpaint_mask"])      # the inpaint operands reach the UNet through the loop
    assert not torch.equal(_sample(m, fx, other, x, True)[0], whole[0])


def test_short_loops_equal_stepwise(golden_dir):
    """init_step leaves one, two and three of the six steps (999, 794, 537, 246, 61, 8 -> t <= 8 / 61 / 246): orders 1 | 1 1 | 1 2 1"""
    fx = _load(golden_dir, "tiny_ddim")
    m, kw = _model(fx, torch.float32)
    x = _x_T(fx, 42)
    grid = [int(t) for t in sampling.dpmpp_grid(AC, 6, "logsnr")]
    finals = []
    for n in (1, 2, 3):
        c0, l0 = _counters()
        step = _sample(m, fx, kw, x, False, init_step=grid[-n])
        whole = _sample(m, fx, kw, x, True, init_step=grid[-n])
        assert _counters() == (c0 + 1, l0 + 1)
        assert _same(step, whole), n
        finals.append(whole[0])
    assert not torch.equal(finals[0], finals[1]) and not torch.equal(finals[1], finals[2])


def test_two_chain_module_runs_the_host_driven_loop(golden_dir):
    fx = _load(golden_dir, "tiny_ddim")
    m, kw = _model(fx, torch.float32, chains=2)
    x = _x_T(fx, 42)
    c0, l0 = _counters()
    step, whole = _sample(m, fx, kw, x, False), _sample(m, fx, kw, x, True)
    assert _same(step, whole)
    assert _counters() == (c0, l0)                     # no single-graph loop under two chains


# ---- 10. the C entry refuses what it cannot run, and stays usable --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_ddim", "tiny_inpaint"])
def test_c_abi_refusals_leave_the_engine_usable(golden_dir, name):
    fx = _load(golden_dir, name)
    m, kw = _model(fx, torch.float32)
    B, h, w = fx["B"], fx["h"], fx["w"]
    x_T = _x_T(fx, 42)
    sm = _sampler(m, fx)
    want = _sample(m, fx, kw, x_T, False, S=6, sampler=sm)                     # plans, binds and conditions the engine
    L, handle, st = _lib.lib(), m._handle, _lib.current_stream()
    f32 = dict(dtype=torch.float32, device="cuda")
    n = len(sm.timesteps)
    table = torch.from_numpy(sm.dpm_table.astype(np.float32)).cuda()
    ts = torch.tensor(sm.timesteps.astype(np.float32), device="cuda")[:, None].expand(-1, B).contiguous()
    x, tmp, hist = torch.empty(B, 4, h, w, **f32), torch.empty(B, 4, h, w, **f32), torch.empty(2, B, 4, h, w, **f32)
    img = msk = None
    if fx.get("inpainting"):
        img, msk = kw["inpaint_image"].float().contiguous(), kw["inpaint_mask"].float().contiguous()
    good = [int(o) for o in sm.orders]

    def call(hd=handle, x_=x, tmp_=tmp, hist_=hist, ts_=ts, table_=table, orders=good, img_=img, msk_=msk, n_steps=n):
        arr = None if orders is None else (C.c_int * len(orders))(*orders)
        return L.k22_unet_dpmpp_loop(hd, _lib.ptr(x_), _lib.ptr(tmp_), _lib.ptr(hist_), _lib.ptr(ts_), _lib.ptr(table_), arr, _lib.ptr(img_),
                                     _lib.ptr(msk_), n_steps, float(fx["guidance"]), 1, st)

    x.copy_(x_T)
    c0, l0 = _counters()
    assert call() == 0 and _counters() == (c0 + 1, l0 + 1)                    # the capture the refusals must leave alone
    assert torch.equal(x, want[0]) and torch.equal(hist[(n - 1) % 2], want[1])
    refused = [("null x", lambda: call(x_=None)), ("null x_tmp", lambda: call(tmp_=None)), ("null x0_hist", lambda: call(hist_=None)),
               ("null timesteps", lambda: call(ts_=None)), ("null table", lambda: call(table_=None)), ("null orders", lambda: call(orders=None)),
               ("null handle", lambda: call(hd=None)), ("n_steps = 0", lambda: call(n_steps=0)),
               ("order 3", lambda: call(orders=good[:2] + [3] + good[3:])), ("order 0", lambda: call(orders=good[:-1] + [0])),
               ("orders[0] = 2", lambda: call(orders=[2] + good[1:]))]
    if fx.get("inpainting"):
        refused += [("9-channel UNet without inpaint operands", lambda: call(img_=None, msk_=None)), ("without the mask", lambda: call(msk_=None))]
    else:
        others = {}        # engines in the states the remaining refusals name; none of them ever runs a forward
        arch = k22.make_arch(fx["model_config"])
        odd = k22.Text2ImUNetHIP(arch, backend_dtype=torch.float32).to("cuda").eval()
        odd._ensure_plan(1, h, w)
        odd.set_condition(*(t.cuda() for t in k22.make_conditioning(arch, 1, seed=2)))
        others["odd B"] = odd
        bare = k22.Text2ImUNetHIP(arch, backend_dtype=torch.float32).to("cuda").eval()
        bare._ensure_plan(B, h, w)
        others["no condition"] = bare
        arch4 = k22.make_arch(dict(fx["model_config"], out_channels=4))
        eps_only = k22.Text2ImUNetHIP(arch4, backend_dtype=torch.float32).to("cuda").eval()
        eps_only._ensure_plan(B, h, w)
        eps_only.set_condition(*(t.cuda() for t in k22.make_conditioning(arch4, B, seed=2)))
        others["out_channels 4"] = eps_only
        arch22 = k22.make_arch22(k22.tiny_unet22_config(), controlnet=True)
        cn = k22.UNet2DConditionHIP(arch22, backend_dtype=torch.float32).to("cuda").eval()
        cn._ensure_plan(B, h, w)
        emb = torch.zeros(B, arch22.image_dim, **f32)
        _lib.check(L.k22_unet_set_condition(cn._handle, None, None, emb.data_ptr(), st))      # the condition, but no hint
        others["no hint"] = cn
        refused += [(what, lambda e=e: call(hd=e._handle)) for what, e in others.items()]
    c1, l1 = _counters()
    for what, fn in refused:
        rc = fn()
        msg = L.k22_last_error().decode()
        print(f"{what}: rc {rc}, '{msg}'")
        assert rc == -1 and "unet_dpmpp_loop" in msg, what           # K22_EINVAL
    assert _counters() == (c1, l1)
    x.copy_(_x_T(fx, 43))
    assert call() == 0 and _counters() == (c1, l1 + 1)                        # a replay of the earlier capture, on the new x_T
    assert _same((x, hist[(n - 1) % 2]), _sample(m, fx, kw, _x_T(fx, 43), False, S=6))


# ---- 11. the public pipeline ---------------------------------------------------------------------------------------------------------------
H = W = 128          # pixels -> 16x16 latents
PRIOR_STEPS = 4


def _pipe(task_type="text2img", backend=torch.float32, **kw):
    cfg = copy.deepcopy(k22.CONFIG_2_1)
    cfg["model_config"] = k22.tiny_model_config()
    hp = k22.tiny_prior_hparams()
    cfg["prior"]["params"]["model"]["hparams"] = hp
    g = torch.Generator().manual_seed(17)
    cfg["prior"]["clip_mean_std_path"] = (torch.randn(768, generator=g) * 0.1, torch.rand(768, generator=g) + 0.5)
    marc = k22.MoVQArch(k22.MOVQ_CONFIG_2_1["ddconfig"])
    movq_sd = dict(k22.init_movq_state_dict(marc, seed=0))
    movq_sd.update(k22.init_movq_encoder_state_dict(marc, seed=0))
    cfg["image_enc_params"]["ckpt_path"] = movq_sd
    arch = k22.make_arch(cfg["model_config"], inpainting=task_type == "inpainting")
    return k22.Kandinsky2_1HIP(cfg, k22.init_unet_state_dict(arch, seed=0), k22.init_prior_state_dict(hp, seed=0), "cuda", task_type=task_type,
                               conditioner="seeded", backend_dtype=backend, **kw)


def test_pipeline_routes_dpm_sampler_and_img2img_keeps_to_init_step():
    g = torch.Generator().manual_seed(5)
    x_T = torch.randn(2, 4, H // 8, W // 8, generator=g).cuda()
    image_emb = torch.randn(2, 768, generator=g).cuda()
    img = (torch.randn(1, 3, H, W, generator=g) * 0.5).clamp(-1, 1).cuda()
    qn = torch.randn(1, 4, H // 8, W // 8, generator=g).cuda()
    prompt = "a red cat, 4k photo"
    for whole in (False, True):
        pipe = _pipe(whole_loop_graph=whole)
        _, diffusion = pipe._diffusion("dpm_sampler", 6)
        assert diffusion.num_timesteps == 1000                                  # the un-respaced schedule, as for DDIM
        c0, l0 = _counters()
        got = pipe.generate_img(prompt, image_emb, batch_size=1, diffusion=diffusion, guidance_scale=4.0, noise=x_T, h=H, w=W,
                                sampler="dpm_sampler", num_steps=6, decode=False)
        assert _counters() == ((c0 + 1, l0 + 1) if whole else (c0, l0))
        full, pooled = pipe.encode_text(prompt, 1)
        pipe.model.del_cache()
        want, _ = k22.DPMSolverSamplerHIP(pipe.model, diffusion, 4.0).sample(
            6, 2, (4, H // 8, W // 8), conditioning=dict(full_emb=full, pooled_emb=pooled, image_emb=image_emb.float()), x_T=x_T,
            whole_loop_graph=whole)
        assert tuple(got.shape) == (1, 4, H // 8, W // 8) and torch.equal(got, want[:1]) and torch.isfinite(got).all()
        with pytest.raises(ValueError, match="Only ddim_sampler and plms_sampler is available"):
            pipe.generate_img(prompt, image_emb, batch_size=1, diffusion=diffusion, noise=x_T, h=H, w=W, sampler="euler_sampler", decode=False)
        if whole:
            continue
        # img2img: strength 0.5 -> init_step 500; the model is only ever called at the grid's timesteps <= 500 (246, 61, 8 of 999 .. 8)
        calls, forward = [], pipe.model.forward

        def recording(x, timesteps, **kw):
            calls.append(float(timesteps[0]))
            return forward(x, timesteps, **kw)

        pipe.model.forward = recording
        torch.manual_seed(21)   # generate_img2img draws the prior's noise itself
        im = pipe.generate_img2img("a blue bird", img, strength=0.5, num_steps=6, batch_size=1, guidance_scale=4.0, h=H, w=W,
                                   sampler="dpm_sampler", prior_steps=str(PRIOR_STEPS), q_noise=qn, output_type="tensor")
        pipe.model.forward = forward
        kept = [float(t) for t in sampling.dpmpp_grid(AC, 6, "logsnr") if t <= 500]
        assert kept == [246.0, 61.0, 8.0] and calls == kept and max(calls) <= 500
        assert tuple(im.shape) == (1, H, W, 3) and im.dtype == torch.uint8
