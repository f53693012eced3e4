"""The prior's DDIM route on the GPU: the step kernel (k22_prior_ddim_step) against float64, the whole loop
(PriorDiffusionModelHIP.forward(timestep_respacing="ddimN") -> k22_prior_sample_loop) against goldens of the REFERENCE's
PriorDiffusionModel.forward (tools/make_golden_prior_ddim.py), one graph against the stepwise loop bit for bit, replay / re-capture
through the "loop_captures" / "loop_launches" counters, the bf16 engine, and prior_steps="ddim5" through Kandinsky2_1HIP.

Bounds.  Step kernel: 8 * 2^-24 * S per element, derived in tests/prior_ddim_ref.py.  Loop against the golden (fp32 engine):
max|out - ref| / max|ref| <= min(2 x the value measured on an MI355X, 1e-3) - the margin of the project's regression bounds
(tests/test_full_size_gpu.py: tile choices outside the shipped table can change the summation order between boxes) under the gate
tests/test_prior_gpu.py holds for prior sampling.  Measured (profiles/prior_ddim.txt): see MEASURED below.  bf16: 0.1 of the sample
scale, the bound of test_prior_bf16_sample_drift_is_bounded.  Everything else is torch.equal.

Shapes: the 512 x 4 prior of the tiny fixtures at bs = 2 (CFG batch 4), 3 to 31 steps; the production prior once, 5 steps.
"""
import copy
import os

import numpy as np
import pytest
import torch

import kandinsky2_amd as k22
import prior_ddim_ref as R
from kandinsky2_amd import _lib
from kandinsky2_amd.prior import PriorSchedule

pytestmark = pytest.mark.gpu

# max|out - ref| / max|ref| of the fp32 engine against the reference golden, measured on an MI355X (profiles/prior_ddim.txt): the largest
# of four processes - the shipped tile table twice, K22_AUTOTUNE=0 (heuristic tiles), K22_TILE_TABLE=0 (every tile measured afresh)
MEASURED = {
    ("prior_tiny_ddim", "ddim5", 0.0): 1.528e-06,
    ("prior_tiny_ddim", "ddim30", 0.0): 2.048e-06,
    ("prior_tiny_ddim", "ddim5", 1.0): 1.477e-06,
    ("prior_tiny_ddim", "ddim3", 0.5): 2.048e-06,
    ("prior_full_ddim", "ddim5", 0.0): 2.416e-06,
}
GATE = 1e-3


def _counters():
    L = _lib.lib()
    return L.k22_debug_counter(b"loop_captures"), L.k22_debug_counter(b"loop_launches")


def _inputs(bs, seed=7):
    """oracle.make_golden.prior_inputs: seeded conditioning, rows [cond | uncond], padding masks of different lengths"""
    g = torch.Generator().manual_seed(seed)
    N = 2 * bs
    cm, cs = torch.randn(768, generator=g) * 0.1, torch.rand(768, generator=g) + 0.5
    txt_feat, txt_seq = torch.randn(N, 768, generator=g), torch.randn(N, 77, 768, generator=g)
    mask = torch.zeros(N, 77, dtype=torch.bool)
    for r in range(bs):
        mask[r, : 9 + 11 * r] = True
    mask[bs:, :2] = True
    return cm, cs, txt_feat.cuda(), txt_seq.cuda(), mask.cuda()


def _noise(seed, T, N):
    """x_T and the per-step noise of a golden case, from its noise_seed (tools/make_golden_prior_ddim.py)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, 768, generator=g).cuda(), torch.randn(T, N, 768, generator=g).cuda()


_FX, _MODELS = {}, {}


def _fixture(golden_dir, name):
    if name not in _FX:
        _FX[name] = torch.load(os.path.join(golden_dir, name + ".pt"), weights_only=False)
    return _FX[name]


def _model(fx, backend):
    """one module per (fixture, engine type) for the whole file: plans, measured tile choices and captured loops are reused"""
    key = (fx["name"], backend)
    if key not in _MODELS:
        cm, cs = _inputs(fx["bs"])[:2]
        m = k22.PriorDiffusionModelHIP(fx["hp"], k22.PRIOR_DIFFUSION_2_1, cm, cs, backend_dtype=backend)
        m.load_state_dict(k22.init_prior_state_dict(fx["hp"], seed=fx["seed_w"]))
        _MODELS[key] = m.to("cuda")
    return _MODELS[key]


def _case(fx, respacing, eta):
    return next(c for c in fx["cases"] if c["respacing"] == respacing and c["eta"] == eta)


def _run(m, fx, case, whole=None, x_T=None, **kw):
    _cm, _cs, txt_feat, txt_seq, mask = _inputs(fx["bs"])
    xt, nzs = _noise(case["noise_seed"], case["num_timesteps"], 2 * fx["bs"])
    return m(txt_feat, txt_seq, mask, fx["scales"].cuda(), timestep_respacing=case["respacing"], eta=case["eta"],
             noise=xt if x_T is None else x_T, noise_seq=nzs if case["eta"] > 0 else None, whole_loop_graph=whole, **kw)


# ---- 1. the step kernel against float64 ----------------------------------------------------------------------------------------------
STEP_ROWS = [  # (respacing, eta, schedule index or "first" / "mid" / "last", with noise)
    ("ddim10", 1.0, "first", True), ("ddim10", 1.0, "mid", True), ("ddim10", 1.0, "last", True),
    ("ddim1000", 1.0, "first", True),      # rm1 = 2e4: r x - x0 cancels to eps ~ x
    ("ddim3", 0.5, "last", True),
    ("ddim10", 0.0, "mid", False),         # noise = NULL on an eta = 0 row
    ("ddim1000", 0.0, "first", False),
]


@pytest.mark.parametrize("with_x0", [True, False])
@pytest.mark.parametrize("respacing,eta,which,with_noise", STEP_ROWS)
def test_ddim_step_kernel_against_float64(respacing, eta, which, with_noise, with_x0):
    bs, D, GUARD = 3, 70, 64          # 420 elements: one full block of 256 and a ragged one; rows j and j + bs differ
    n = 2 * bs * D
    s = PriorSchedule(**dict(k22.PRIOR_DIFFUSION_2_1, timestep_respacing=respacing), eta=eta)
    i = {"first": s.num_timesteps - 1, "mid": s.num_timesteps // 2, "last": 0}[which]
    row = torch.from_numpy(s.ddim_table()[i].copy())
    g = torch.Generator().manual_seed(11)
    x, noise = torch.randn(2 * bs, D, generator=g), torch.randn(2 * bs, D, generator=g)
    mo = torch.randn(2 * bs, D, generator=g) * 1.5
    mo[:, ::3] *= 6.0                 # a third of the columns: the guided prediction leaves +-10, the clamp is active there
    scales = torch.tensor([4.0, 2.5, 1.0])
    y64, x064, S, G = R.ddim_step64(x, mo, noise if with_noise else None, scales, row.double())
    clamped = x064.abs() == 10.0
    assert clamped.any() and not clamped.all()
    out = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    x0o = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    xd, mod, nzd, scd, rowd = x.cuda(), mo.cuda(), noise.cuda(), scales.cuda(), row.cuda()
    _lib.check(_lib.lib().k22_prior_ddim_step(xd.data_ptr(), mod.data_ptr(), nzd.data_ptr() if with_noise else None, scd.data_ptr(), rowd.data_ptr(),
                                              10.0, out.data_ptr() + 4 * GUARD, x0o.data_ptr() + 4 * GUARD if with_x0 else None, bs, D,
                                              _lib.current_stream()))
    torch.cuda.synchronize()
    out, x0o = out.cpu(), x0o.cpu()
    for buf, written in ((out, True), (x0o, with_x0)):
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all()     # nothing outside the launch's elements
        assert torch.isfinite(buf[GUARD:GUARD + n]).all() if written else torch.isnan(buf).all()
    y = out[GUARD:GUARD + n].view(2 * bs, D).double()
    ratio = ((y - y64).abs() / R.bound(S)).max().item()
    print(f"ddim_step {respacing} eta {eta} row {i} ({which}): rm1 {row[1].item():.4g} sigma {row[3].item():.4g} dir {row[4].item():.4g}  "
          f"worst |d| / (8 * 2^-24 * S) = {ratio:.3f}")
    assert ratio <= 1.0
    if with_x0:
        x0 = x0o[GUARD:GUARD + n].view(2 * bs, D).double()
        r0 = ((x0 - x064).abs() / R.bound_x0(G)).max().item()
        print(f"    x0_out: worst |d| / (3 * 2^-24 * G) = {r0:.3f}")
        assert r0 <= 1.0 and torch.equal(x0[:bs], x0[bs:])
        if which == "last":
            assert torch.equal(y, x0)               # ab_prev = 1: the step returns x0


# ---- 2. the loop against the reference golden, fp32 engine ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,respacing,eta", sorted(MEASURED))
def test_ddim_loop_vs_reference_golden_fp32(golden_dir, name, respacing, eta):
    fx = _fixture(golden_dir, name)
    case = _case(fx, respacing, eta)
    m = _model(fx, torch.float32)
    c0, l0 = _counters()
    out = _run(m, fx, case).cpu()
    assert _counters()[1] == l0 + 1                 # the default route of a "ddim" string is the loop entry
    ref = case["sample"]
    rel = (out - ref).abs().max().item() / ref.abs().max().item()
    bound = min(2 * MEASURED[(name, respacing, eta)], GATE)
    print(f"{name} {respacing} eta {eta} ({case['num_timesteps']} steps) fp32: max|d| / max|ref| = {rel:.3e}  (bound {bound:.3e})")
    assert out.shape == ref.shape and torch.isfinite(out).all() and rel <= bound


# ---- 3. one graph == stepwise == the eager loop entry, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("backend", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("respacing,eta", [("ddim5", 1.0), ("ddim30", 0.0)])
def test_one_graph_equals_stepwise_bit_for_bit(golden_dir, respacing, eta, backend):
    fx = _fixture(golden_dir, "prior_tiny_ddim")
    case = _case(fx, respacing, eta)
    m = _model(fx, backend)
    c0, l0 = _counters()
    step = _run(m, fx, case, whole=False)
    assert _counters() == (c0, l0)                  # the stepwise path is no loop
    graph = _run(m, fx, case, whole=True)
    c1, l1 = _counters()
    assert l1 == l0 + 1 and c1 - c0 in (0, 1)       # 0: another test of this file left this very loop captured on the shared module
    m.use_graph = False
    try:
        eager = _run(m, fx, case, whole=True)
    finally:
        m.use_graph = True
    assert _counters() == (c1, l1 + 1)              # the eager form: a loop run, no capture
    assert torch.isfinite(step).all()
    assert torch.equal(step, graph), (step - graph).abs().max().item()
    assert torch.equal(step, eager), (step - eager).abs().max().item()


def test_ancestral_route_through_the_loop_entry_equals_the_default_route(golden_dir):
    fx = _fixture(golden_dir, "prior_tiny_ddim")
    m = _model(fx, torch.float32)
    _cm, _cs, txt_feat, txt_seq, mask = _inputs(fx["bs"])
    xt, nzs = _noise(31, 5, 2 * fx["bs"])
    kw = dict(timestep_respacing="5", noise=xt, noise_seq=nzs)
    c0, l0 = _counters()
    default = m(txt_feat, txt_seq, mask, fx["scales"].cuda(), **kw)
    assert _counters() == (c0, l0)                  # today's route: untouched, no loop
    whole = m(txt_feat, txt_seq, mask, fx["scales"].cuda(), whole_loop_graph=True, **kw)
    assert _counters()[1] == l0 + 1
    assert torch.isfinite(default).all() and torch.equal(default, whole), (default - whole).abs().max().item()


# ---- 4. replay, re-capture --------------------------------------------------------------------------------------------------------------
def test_second_call_replays_and_a_new_binding_recaptures(golden_dir):
    fx = _fixture(golden_dir, "prior_tiny_ddim")
    case = _case(fx, "ddim5", 1.0)
    m = _model(fx, torch.float32)
    first = _run(m, fx, case)
    c1, l1 = _counters()
    second = _run(m, fx, case)
    assert _counters() == (c1, l1 + 1) and torch.equal(first, second)            # same string, same batch: replayed
    other = _run(m, fx, case, x_T=_noise(77, 1, 2 * fx["bs"])[0])
    assert _counters() == (c1, l1 + 2) and not torch.equal(first, other)          # the replay read the new x_T
    _run(m, fx, _case(fx, "ddim3", 0.5))
    assert _counters() == (c1 + 1, l1 + 3)                                       # another step count: captured again
    _run(m, fx, case)
    assert _counters() == (c1 + 2, l1 + 4)                                       # the handle keeps ONE loop
    m.prepare()                                                                   # a new engine, plan and binding
    again = _run(m, fx, case)
    assert _counters() == (c1 + 3, l1 + 5) and torch.equal(first, again)


# ---- 5. the bf16 engine ------------------------------------------------------------------------------------------------------------------
def test_ddim_bf16_sample_drift_is_bounded(golden_dir):
    fx = _fixture(golden_dir, "prior_tiny_ddim")
    case = _case(fx, "ddim5", 0.0)
    out = _run(_model(fx, torch.bfloat16), fx, case).cpu()
    ref = case["sample"]
    err = (out - ref).abs().max().item() / ref.abs().max().item()
    print(f"prior_tiny_ddim bf16 ddim5 eta 0 drift: {err:.3e} of the sample scale")
    assert torch.isfinite(out).all() and err <= 0.1


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------
def test_prior_steps_ddim_through_the_pipeline():
    cfg = copy.deepcopy(k22.CONFIG_2_1)
    cfg["model_config"] = k22.tiny_model_config()
    hp = k22.tiny_prior_hparams()
    cfg["prior"]["params"]["model"]["hparams"] = hp
    g = torch.Generator().manual_seed(17)
    cfg["prior"]["clip_mean_std_path"] = (torch.randn(768, generator=g) * 0.1, torch.rand(768, generator=g) + 0.5)
    marc = k22.MoVQArch(k22.MOVQ_CONFIG_2_1["ddconfig"])
    cfg["image_enc_params"]["ckpt_path"] = dict(k22.init_movq_state_dict(marc, seed=0))
    unet_sd = k22.init_unet_state_dict(k22.make_arch(cfg["model_config"], inpainting=False), seed=0)
    pipe = k22.Kandinsky2_1HIP(cfg, unet_sd, k22.init_prior_state_dict(hp, seed=0), "cuda", conditioner="seeded", backend_dtype=torch.float32)
    bs, prompt = 2, "a red cat, 4k photo"
    x_T = torch.randn(2 * bs, 768, generator=g).cuda()
    c0, l0 = _counters()
    emb = pipe.generate_clip_emb(prompt, batch_size=bs, prior_cf_scale=4, prior_steps="ddim5", noise=x_T)
    assert _counters()[1] == l0 + 1                 # the DDIM string reached the loop entry
    assert emb.shape == (bs, 768) and torch.isfinite(emb).all()
    txt_feat, txt_seq, mask = pipe.conditioner.clip_text([prompt] * bs, "", "cuda")
    direct = pipe.prior(txt_feat, txt_seq, mask, torch.full((bs,), 4.0, device="cuda"), timestep_respacing="ddim5", noise=x_T)
    assert torch.equal(emb, direct)
    img = pipe.generate_text2img(prompt, num_steps=3, batch_size=1, guidance_scale=4, h=128, w=128, sampler="p_sampler", prior_steps="ddim10",
                                 output_type="uint8")
    assert isinstance(img, np.ndarray) and img.shape == (1, 128, 128, 3) and img.dtype == np.uint8
