"""The DDIM and PLMS sampling loops as ONE captured graph (k22_unet_ddim_loop -> Text2ImUNetHIP.ddim_loop -> DDIMSamplerHIP /
PLMSSamplerHIP.sample(whole_loop_graph=True) -> Kandinsky2_1HIP.generate_img).

The captured loop issues the kernels of the stepwise Python path on the same operands, so every comparison between the two is
torch.equal.  Equal bits alone would also hold if whole_loop_graph= were ignored: the "loop_captures" / "loop_launches" counters of
k22_debug_counter are what proves that the one-graph path ran and that a second generation replayed its capture.  The only tolerance
in this file is the reference-golden bound the stepwise tests already use (tests/test_unet_gpu.py:
test_ddim_sampler_final_latent_vs_reference_golden_fp32): 1e-3 * max(1, scale of the reference latent).

Shapes: the tiny fixtures' 128-channel UNet at 16x16 (CFG batch 2) and, for the inpainting UNet, 16x24 (CFG batch 4), at most 8 steps.
"""
import copy
import os

import pytest
import torch

import kandinsky2_amd as k22
from kandinsky2_amd import _lib

pytestmark = pytest.mark.gpu

SAMPLERS = {"ddim": k22.DDIMSamplerHIP, "plms": k22.PLMSSamplerHIP}
STEPS = {"ddim": 5, "plms": 8}   # the step counts of tiny_ddim.pt / tiny_plms.pt


def _load(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name + ".pt"), weights_only=False)


def _counters():
    L = _lib.lib()
    return L.k22_debug_counter(b"loop_captures"), L.k22_debug_counter(b"loop_launches")


def _model(fx, backend, use_graph=True, chains=None):
    """module + conditioning built as tests/test_unet_gpu.py does"""
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


def _sample(kind, m, fx, kw, x_T, whole, S=None, **extra):
    """(final latent, pred_x0) of one generation; the conditioning cache is dropped first, as generate_img does"""
    old = k22.create_gaussian_diffusion(**k22.DIFFUSION_CONFIG_2_1)   # the un-respaced 1000-step schedule
    m.del_cache()
    out, aux = SAMPLERS[kind](m, old, fx["guidance"]).sample(STEPS[kind] if S is None else S, fx["B"], (4, fx["h"], fx["w"]), conditioning=kw,
                                                            x_T=x_T, whole_loop_graph=whole, **extra)
    return out, aux["pred_x0"][0]


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 1. loop == stepwise, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["ddim", "plms"])
def test_whole_loop_equals_the_stepwise_loop_and_the_second_generation_replays(golden_dir, kind, backend):
    """Two generations (x_T seeds 42, 43) on one module: final latent and pred_x0 equal the stepwise path's, ONE capture for the two
    (the second replays it with new operands copied into the module's buffers) and two launches; then the eager form of the same entry
    (use_graph=False: one more launch, no capture)."""
    fx = _load(golden_dir, "tiny_" + kind)
    m, kw = _model(fx, backend)
    xs = [_x_T(fx, 42), _x_T(fx, 43)]
    c0, l0 = _counters()
    step = [_sample(kind, m, fx, kw, x, False) for x in xs]
    assert _counters() == (c0, l0)            # the stepwise path is no loop
    whole = [_sample(kind, m, fx, kw, x, True) for x in xs]
    c1, l1 = _counters()
    print(f"{kind} {backend}: loop_captures +{c1 - c0}, loop_launches +{l1 - l0}")
    assert (c1 - c0, l1 - l0) == (1, 2)
    for s, w in zip(step, whole):
        assert _same(s, w), (kind, backend, (s[0] - w[0]).abs().max().item())
    assert not torch.equal(whole[0][0], whole[1][0])   # the replay read the new x_T
    m.use_graph = False
    eager = _sample(kind, m, fx, kw, xs[0], True)
    assert _counters() == (c1, l1 + 1)
    assert _same(step[0], eager)


@pytest.mark.parametrize("backend", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["ddim", "plms"])
def test_whole_loop_with_per_step_time_rows_equals_the_stepwise_loop(golden_dir, kind, backend, monkeypatch):
    """K22_HOIST_TIME=0 (read when the engine is created): the captured loop keeps the per-call time-embedding / FiLM launches."""
    monkeypatch.setenv("K22_HOIST_TIME", "0")
    fx = _load(golden_dir, "tiny_" + kind)
    m, kw = _model(fx, backend)
    x = _x_T(fx, 42)
    c0, l0 = _counters()
    step, whole = _sample(kind, m, fx, kw, x, False), _sample(kind, m, fx, kw, x, True)
    assert _counters() == (c0 + 1, l0 + 1)
    assert _same(step, whole)


# ---- 2. DDIM with eta > 0 ------------------------------------------------------------------------------------------------------------
def test_ddim_loop_with_eta_injected_and_generator_drawn_noise(golden_dir):
    fx = _load(golden_dir, "tiny_ddim")
    m, kw = _model(fx, torch.float32)
    x = _x_T(fx, 42)
    nz = torch.randn(STEPS["ddim"], fx["B"], 4, fx["h"], fx["w"], generator=torch.Generator().manual_seed(7)).cuda()
    quiet = _sample("ddim", m, fx, kw, x, False)
    c0, l0 = _counters()
    step, whole = _sample("ddim", m, fx, kw, x, False, eta=0.5, noise_seq=nz), _sample("ddim", m, fx, kw, x, True, eta=0.5, noise_seq=nz)
    assert _same(step, whole)
    assert not torch.equal(step[0], quiet[0])          # the noise took part
    # no noise_seq: the loop draws all noise up front by the calls the stepwise path makes one per step - same generator draws
    torch.manual_seed(1234)
    step_g = _sample("ddim", m, fx, kw, x, False, eta=0.5)
    torch.manual_seed(1234)
    whole_g = _sample("ddim", m, fx, kw, x, True, eta=0.5)
    assert _same(step_g, whole_g)
    assert not torch.equal(step_g[0], step[0])
    assert _counters() == (c0 + 1, l0 + 2)             # same buffers, same step count: the second loop replayed


# ---- 3. short loops: the eps ring and the orders 0/4 -> 1 -> 2 -> 3 hand-off ---------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddim", "plms"])
def test_short_loops_equal_stepwise(golden_dir, kind):
    """S = 5 keeps the timesteps 1, 201, 401, 601, 801; init_step = 1 / 201 / 401 leaves one, two and three steps.  With one step
    PLMS makes its second model call at the same timestep."""
    fx = _load(golden_dir, "tiny_" + kind)
    m, kw = _model(fx, torch.float32)
    x = _x_T(fx, 42)
    finals = []
    for init_step, n in ((1, 1), (201, 2), (401, 3)):
        c0, l0 = _counters()
        step = _sample(kind, m, fx, kw, x, False, S=5, init_step=init_step)
        whole = _sample(kind, m, fx, kw, x, True, S=5, init_step=init_step)
        assert _counters() == (c0 + 1, l0 + 1)         # another step count: another capture
        assert _same(step, whole), (kind, init_step)
        finals.append(whole[0])
    assert not torch.equal(finals[0], finals[1]) and not torch.equal(finals[1], finals[2])


# ---- 4. the 9-channel inpainting UNet: CFG batch 4 (two calls per batched time-row launch), non-square latent ------------------------
@pytest.mark.parametrize("backend", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["ddim", "plms"])
def test_inpainting_unet_loop_equals_stepwise(golden_dir, kind, backend):
    fx = _load(golden_dir, "tiny_inpaint")
    assert (fx["B"], fx["h"], fx["w"]) == (4, 16, 24)
    m, kw = _model(fx, backend)
    x = _x_T(fx, 42)
    c0, l0 = _counters()
    step, whole = _sample(kind, m, fx, kw, x, False), _sample(kind, m, fx, kw, x, True)
    assert _counters() == (c0 + 1, l0 + 1)
    assert _same(step, whole)
    # the inpaint operands reach the UNet through the loop
    other = dict(kw, inpaint_mask=1.0 - kw["inpaint_mask"])
    assert not torch.equal(_sample(kind, m, fx, other, x, True)[0], whole[0])


# ---- 5. the reference's own goldens through the loop ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,seed", [("ddim", 42), ("plms", 43)])
def test_reference_golden_through_the_whole_loop_fp32(golden_dir, kind, seed):
    """tiny_ddim.pt / tiny_plms.pt: the reference DDIMSampler / PLMSSampler final latent, bound of the stepwise tests"""
    fx = _load(golden_dir, "tiny_" + kind)
    m, kw = _model(fx, torch.float32)
    c0, l0 = _counters()
    out, _ = _sample(kind, m, fx, kw, _x_T(fx, seed), True)
    assert _counters() == (c0 + 1, l0 + 1)
    ref = fx["final"]
    scale = ref.abs().max().item()
    err = (out.cpu() - ref).abs().max().item()
    print(f"{kind} whole loop, fp32, vs the reference golden: max|d|={err:.3e} scale={scale:.2f}")
    assert err <= 1e-3 * max(1.0, scale)


@pytest.mark.slow
def test_whole_ddim_loop_equals_stepwise_at_the_full_size_unet_bf16(golden_dir):
    """The 1.23 B UNet at the c2_ddim shape (2x4x96x96), 20 steps, bf16: the real FiLM widths and a capture of ~10 000 nodes."""
    fx = _load(golden_dir, "c2_ddim")
    m, kw = _model(fx, torch.bfloat16)
    x = _x_T(fx, 42)
    c0, l0 = _counters()
    step, whole = _sample("ddim", m, fx, kw, x, False, S=fx["steps"]), _sample("ddim", m, fx, kw, x, True, S=fx["steps"])
    assert _counters() == (c0 + 1, l0 + 1)
    assert _same(step, whole), (step[0] - whole[0]).abs().max().item()


# ---- 6. one engine keeps one captured loop: a change of kind re-captures -------------------------------------------------------------
def test_alternating_loop_kinds_on_one_module_recapture(golden_dir):
    fx = _load(golden_dir, "tiny_text2img")
    m, kw = _model(fx, torch.float32)
    shape = (fx["B"], 4, fx["h"], fx["w"])
    x = _x_T(fx, 42)
    nz = torch.randn(fx["steps"], *shape, generator=torch.Generator().manual_seed(9)).cuda()
    d = k22.create_gaussian_diffusion(**dict(k22.DIFFUSION_CONFIG_2_1, timestep_respacing=str(fx["steps"])))

    def p_loop(whole):
        m.del_cache()
        return d.p_sample_loop(m, shape, model_kwargs=kw, guidance_scale=fx["guidance"], noise=x, noise_seq=nz, whole_loop_graph=whole)

    want_p, want_ddim, want_plms = p_loop(False), _sample("ddim", m, fx, kw, x, False), _sample("plms", m, fx, kw, x, False)
    for run, check in ((lambda: p_loop(True), lambda r: torch.equal(r, want_p)),
                       (lambda: _sample("ddim", m, fx, kw, x, True), lambda r: _same(r, want_ddim)),
                       (lambda: p_loop(True), lambda r: torch.equal(r, want_p)),
                       (lambda: _sample("plms", m, fx, kw, x, True), lambda r: _same(r, want_plms))):
        c0, l0 = _counters()
        got = run()
        assert _counters() == (c0 + 1, l0 + 1)
        assert check(got)


# ---- 7. two-chain mode: the host-driven fallback --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddim", "plms"])
def test_two_chain_module_runs_the_host_driven_loop(golden_dir, kind):
    fx = _load(golden_dir, "tiny_" + kind)
    m, kw = _model(fx, torch.float32, chains=2)
    x = _x_T(fx, 42)
    c0, l0 = _counters()
    step, whole = _sample(kind, m, fx, kw, x, False), _sample(kind, m, fx, kw, x, True)
    assert _same(step, whole)
    assert _counters() == (c0, l0)                     # no single-graph loop under two chains


# ---- 8. the public pipeline ----------------------------------------------------------------------------------------------------------
H = W = 128          # pixels -> 16x16 latents
PRIOR_STEPS = 4
_CACHE = {}


def _weights(task_type):
    if task_type not in _CACHE:
        cfg = copy.deepcopy(k22.CONFIG_2_1)
        cfg["model_config"] = k22.tiny_model_config()
        hp = k22.tiny_prior_hparams()
        cfg["prior"]["params"]["model"]["hparams"] = hp
        g = torch.Generator().manual_seed(17)
        cm, cs = torch.randn(768, generator=g) * 0.1, torch.rand(768, generator=g) + 0.5
        cfg["prior"]["clip_mean_std_path"] = (cm, cs)
        marc = k22.MoVQArch(k22.MOVQ_CONFIG_2_1["ddconfig"])
        movq_sd = dict(k22.init_movq_state_dict(marc, seed=0))
        movq_sd.update(k22.init_movq_encoder_state_dict(marc, seed=0))
        cfg["image_enc_params"]["ckpt_path"] = movq_sd
        arch = k22.make_arch(cfg["model_config"], inpainting=task_type == "inpainting")
        unet_sd = k22.init_unet_state_dict(arch, seed=0)
        prior_sd = k22.init_prior_state_dict(hp, seed=0)
        _CACHE.clear()
        _CACHE[task_type] = (cfg, unet_sd, prior_sd)
    return _CACHE[task_type]


def _pipe(task_type, backend=torch.float32, **kw):
    cfg, unet_sd, prior_sd = _weights(task_type)
    return k22.Kandinsky2_1HIP(cfg, unet_sd, prior_sd, "cuda", task_type=task_type, conditioner="seeded", backend_dtype=backend, **kw)


def test_pipeline_routes_ddim_and_plms_through_the_whole_loop():
    """generate_text2img (ddim_sampler - the default - and plms_sampler) and generate_img2img (init_step) on a pipeline with
    whole_loop_graph=True and on one with whole_loop_graph=False: equal images and latents; only the first runs loops."""
    g = torch.Generator().manual_seed(5)
    x_T = torch.randn(2, 4, H // 8, W // 8, generator=g).cuda()
    pn, pz = torch.randn(2, 768, generator=g).cuda(), torch.randn(PRIOR_STEPS, 2, 768, generator=g).cuda()
    img = (torch.randn(1, 3, H, W, generator=g) * 0.5).clamp(-1, 1).cuda()
    qn = torch.randn(1, 4, H // 8, W // 8, generator=g).cuda()

    def generations(pipe):
        outs = []
        for sampler, steps in (("ddim_sampler", 5), ("plms_sampler", 6)):
            im = pipe.generate_text2img("a red cat, 4k photo", num_steps=steps, batch_size=1, guidance_scale=4.0, h=H, w=W, sampler=sampler,
                                        prior_steps=str(PRIOR_STEPS), noise=x_T, prior_noise=pn, prior_noise_seq=pz, output_type="tensor")
            outs += [im.clone(), pipe.last_latent.clone()]
        torch.manual_seed(21)   # generate_img2img draws the prior's noise itself
        im = pipe.generate_img2img("a blue bird", img, strength=0.5, num_steps=5, batch_size=1, guidance_scale=4.0, h=H, w=W,
                                   sampler="ddim_sampler", prior_steps=str(PRIOR_STEPS), q_noise=qn, output_type="tensor")
        return outs + [im.clone(), pipe.last_latent.clone()]

    c0, l0 = _counters()
    off = generations(_pipe("text2img", whole_loop_graph=False))
    assert _counters() == (c0, l0)
    on = generations(_pipe("text2img", whole_loop_graph=True))
    c1, l1 = _counters()
    assert (c1 - c0, l1 - l0) == (3, 3)                # three generations of three different loops
    for a, b in zip(off, on):
        assert a.shape == b.shape and torch.equal(a, b)
    assert tuple(on[0].shape) == (1, H, W, 3) and on[0].dtype == torch.uint8


# ---- 9. the C entry refuses what it cannot run, and stays usable ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_ddim", "tiny_inpaint"])
def test_c_abi_refusals_leave_the_engine_usable(golden_dir, name):
    fx = _load(golden_dir, name)
    m, kw = _model(fx, torch.float32)
    B, h, w = fx["B"], fx["h"], fx["w"]
    x_T = _x_T(fx, 42)
    want = {k: _sample(k, m, fx, kw, x_T, False, S=5) for k in ("ddim", "plms")}     # plans, binds and conditions the engine
    L, handle, st = _lib.lib(), m._handle, _lib.current_stream()
    f32 = dict(dtype=torch.float32, device="cuda")
    old = k22.create_gaussian_diffusion(**k22.DIFFUSION_CONFIG_2_1)
    sm = k22.DDIMSamplerHIP(m, old, fx["guidance"])
    sm.make_schedule(5)
    table = torch.from_numpy(sm.table[::-1].copy()).cuda()
    tr = [float(t) for t in sm.ddim_timesteps[::-1]]
    calls = {"ddim": tr, "plms": [tr[0], tr[1]] + tr[1:]}
    ts = {k: torch.tensor(v, **f32)[:, None].expand(-1, B).contiguous() for k, v in calls.items()}
    x, tmp, x0 = torch.empty(B, 4, h, w, **f32), torch.empty(B, 4, h, w, **f32), torch.empty(B, 4, h, w, **f32)
    noise, hist = torch.zeros(5, B, 4, h, w, **f32), torch.empty(4, B, 4, h, w, **f32)
    img = msk = None
    if fx.get("inpainting"):
        img, msk = kw["inpaint_image"].float().contiguous(), kw["inpaint_mask"].float().contiguous()
    DDIM, PLMS = _lib.K22_LOOP_DDIM, _lib.K22_LOOP_PLMS

    def call(kind, x_, noise_, n_steps, img_=img, msk_=msk):
        return L.k22_unet_ddim_loop(handle, kind, _lib.ptr(x_), tmp.data_ptr(), x0.data_ptr(), ts["plms" if kind == PLMS else "ddim"].data_ptr(),
                                    table.data_ptr(), _lib.ptr(noise_), _lib.ptr(img_), _lib.ptr(msk_), hist.data_ptr(), n_steps,
                                    float(fx["guidance"]), 1, st)

    refused = [("PLMS with noise", lambda: call(PLMS, x, noise, 5)), ("n_steps = 0", lambda: call(DDIM, x, None, 0)),
               ("null x", lambda: call(DDIM, None, None, 5))]
    if fx.get("inpainting"):
        refused.append(("9-channel UNet without inpaint operands", lambda: call(DDIM, x, None, 5, None, None)))
    c0, l0 = _counters()
    for what, fn in refused:
        rc = fn()
        msg = L.k22_last_error().decode()
        print(f"{what}: rc {rc}, '{msg}'")
        assert rc == -1 and "unet_ddim_loop" in msg, what           # K22_EINVAL
    assert _counters() == (c0, l0)
    for kind, code in (("ddim", DDIM), ("plms", PLMS)):
        x.copy_(x_T)
        assert call(code, x, None, 5) == 0
        assert torch.equal(x, want[kind][0]) and torch.equal(x0, want[kind][1]), kind
    assert _counters() == (c0 + 2, l0 + 2)
