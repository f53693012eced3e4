"""Host side of the prior's DDIM route (no GPU): PriorSchedule("ddimN") against the reference's float64 schedule arrays, the float64
step restatement (tests/prior_ddim_ref.py) against a ddim_sample call recorded from the reference, the refusals, and the argument
checks of k22_prior_sample_loop.  Goldens: tools/make_golden_prior_ddim.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import kandinsky2_amd as k22
import prior_ddim_ref as R
from kandinsky2_amd import _lib
from kandinsky2_amd.prior import PriorSchedule

ARRAYS = ("alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")
STEPS = {"ddim3": 3, "ddim10": 10, "ddim25": 25, "ddim30": 31, "ddim1000": 999}   # what the reference runs, not what the string says


@pytest.fixture(scope="module")
def ref_tables(golden_dir):
    with open(os.path.join(golden_dir, "ref_prior_ddim_tables.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("respacing", sorted(STEPS))
def test_schedule_arrays_equal_the_reference_bit_for_bit(ref_tables, respacing):
    ref = ref_tables[respacing]
    s = PriorSchedule(**dict(k22.PRIOR_DIFFUSION_2_1, timestep_respacing=respacing))
    assert s.ddim and s.num_timesteps == ref["num_timesteps"] == STEPS[respacing]
    assert list(s.timestep_map) == ref["timestep_map"]
    for name in ARRAYS:
        ours, theirs = getattr(s, name), np.array([float.fromhex(h) for h in ref[name]], dtype=np.float64)
        assert ours.dtype == np.float64 and ours.shape == theirs.shape
        assert np.array_equal(ours, theirs), (respacing, name, np.abs(ours - theirs).max())


def test_float64_step_reproduces_the_recorded_reference_step(golden_dir):
    fx = torch.load(os.path.join(golden_dir, "prior_tiny_ddim.pt"), weights_only=False)
    rec = fx["record"]
    s = PriorSchedule(**dict(k22.PRIOR_DIFFUSION_2_1, timestep_respacing=rec["respacing"]))
    i = rec["index"]
    assert 0 < i < s.num_timesteps - 1                       # mid-loop: sigma, direction and noise all live
    row = R.table_rows(s.alphas_cumprod, s.alphas_cumprod_prev, rec["eta"])[i]
    assert row[3] > 0 and row[4] > 0 and row[5] == 1
    # the record holds the GUIDED model output (both halves equal): c = u, so the guidance term of the restatement is exactly 0
    assert torch.equal(rec["model_out"][: fx["bs"]], rec["model_out"][fx["bs"]:])
    y, x0, S, _G = R.ddim_step64(rec["x"], rec["model_out"], rec["noise"], rec["scales"], row)
    for name, got, ref in (("sample", y, rec["sample"]), ("pred_xstart", x0, rec["pred_xstart"])):
        ratio = ((got - ref.double()).abs() / R.bound(S)).max().item()
        print(f"recorded ddim_sample ({rec['respacing']}, eta {rec['eta']}, index {i}) {name}: worst |d| / bound = {ratio:.3f}")
        assert ratio <= 1.0, name


def test_fast_and_eta_outside_the_unit_interval_are_value_errors():
    with pytest.raises(ValueError, match="fast"):
        PriorSchedule(**dict(k22.PRIOR_DIFFUSION_2_1, timestep_respacing="fast27"))
    for eta in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="eta"):
            PriorSchedule(**dict(k22.PRIOR_DIFFUSION_2_1, timestep_respacing="ddim10"), eta=eta)
        with pytest.raises(ValueError, match="eta"):
            PriorSchedule(**dict(k22.PRIOR_DIFFUSION_2_1, timestep_respacing="ddim10")).ddim_table(eta)
    m = k22.PriorDiffusionModelHIP(k22.tiny_prior_hparams(), k22.PRIOR_DIFFUSION_2_1)
    z = torch.zeros(2, 768)
    with pytest.raises(ValueError, match="fast"):           # refused before anything touches a device
        m(z, torch.zeros(2, 77, 768), torch.ones(2, 77, dtype=torch.bool), torch.tensor([4.0]), timestep_respacing="fast27")


@pytest.mark.parametrize("respacing", ["ddim3", "ddim10", "ddim30", "ddim1000"])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_ddim_table_rows(respacing, eta):
    s = PriorSchedule(**dict(k22.PRIOR_DIFFUSION_2_1, timestep_respacing=respacing), eta=eta)
    tab = s.ddim_table()
    assert tab.dtype == np.float32 and tab.shape == (s.num_timesteps, 8) and np.isfinite(tab).all()
    # the last step run (schedule index 0): ab_prev = 1 -> the step returns x0
    assert tab[0, 2] == 1.0 and tab[0, 3] == 0.0 and tab[0, 4] == 0.0 and tab[0, 5] == 0.0
    assert (tab[1:, 5] == 1.0).all() and (tab[:, 6:] == 0.0).all()
    ref = R.table_rows(s.alphas_cumprod, s.alphas_cumprod_prev, eta)
    assert np.array_equal(tab, ref.astype(np.float32))      # float64, rounded once
    assert (tab[:, 3] == 0).all() if eta == 0 else (tab[1:, 3] > 0).all()
    assert np.array_equal(s.ddim_table(eta), tab)


def test_sample_loop_refuses_bad_calls_without_a_device():
    """k22_prior_sample_loop's argument checks, host logic only (nothing planned, nothing bound, nothing launched): a null argument, an
    unknown kind, n_steps < 1, the ancestral kind without noise and an unbound handle are K22_EINVAL with a text, each named for itself."""
    L = _lib.lib()

    def err():
        return (L.k22_last_error() or b"").decode()

    pc = _lib.K22PriorConfig(dtype=_lib.K22_BF16, text_ctx=77, xf_width=128, xf_layers=2, xf_heads=2, xf_final_ln=1, clip_dim=64, clip_xf_width=64)
    h = C.c_void_p()
    assert L.k22_prior_create(C.byref(pc), None, 0, C.byref(h)) == 0
    p = C.c_void_p(1 << 20)   # never dereferenced: every call below is refused before it reaches the device

    def loop(handle=h, kind=_lib.K22_PRIOR_LOOP_DDIM, x=p, noise=p, n_steps=3, key_valid=p):
        return L.k22_prior_sample_loop(handle, kind, x, p, None, p, p, noise, p, p, p, key_valid, 10.0, n_steps, 1, None)

    try:
        c0 = (L.k22_debug_counter(b"loop_captures"), L.k22_debug_counter(b"loop_launches"))
        rcs = []
        for kw, text in ((dict(handle=None), "null argument"), (dict(x=None), "null argument"), (dict(key_valid=None), "null argument"),
                         (dict(kind=2), "kind"), (dict(kind=-1), "kind"), (dict(n_steps=0), "n_steps"),
                         (dict(kind=_lib.K22_PRIOR_LOOP_ANCESTRAL, noise=None), "noise_seq"),
                         (dict(), "bind a workspace first"), (dict(noise=None), "bind a workspace first")):
            rc = loop(**kw)
            rcs.append(rc)
            assert rc != 0 and "prior_sample_loop" in err() and text in err(), (kw, rc, err())
        assert set(rcs) == {-1}                              # K22_EINVAL (include/k22.h), all of them
        n = C.c_size_t()
        assert L.k22_prior_plan(h, 2, C.byref(n)) != 0 and "missing weight" in err()
        assert loop() == rcs[0] and "bind a workspace first" in err()   # a plan that failed is no plan
        assert L.k22_prior_ddim_step(None, p, None, p, p, 10.0, p, None, 1, 8, None) == rcs[0] and "prior_ddim_step" in err()
        assert L.k22_prior_ddim_step(p, p, None, p, p, 10.0, p, None, 0, 8, None) == rcs[0]
        assert (L.k22_debug_counter(b"loop_captures"), L.k22_debug_counter(b"loop_launches")) == c0
    finally:
        L.k22_prior_destroy(h)
