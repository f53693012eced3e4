"""CPU half of the GroupNorm parity (tests/gn_ref.py, tests/test_gn_parity_gpu.py):
 (a) the float64 restatements, composed stage by stage, equal F.group_norm -> FiLM -> SiLU -> avg_pool2d / interpolate -> pad to 1e-12;
 (b) torch's own fp32 evaluation of every stage passes every bound on every family and shape the GPU half runs - the largest ratios are
     printed (gn_ref's docstring records them);
 (c) resolving power: every deliberately wrong restatement is rejected on the chosen inputs under the bound of every dtype (a correct
     kernel is stood in for by the right reference rounded once to what the stage stores);
 (d) the refusals of k22_gn_stats / k22_gn_coeff / k22_gn_apply (host logic: nothing is launched, no device is needed)."""
import ctypes as C

import pytest
import torch

import aux_ref as ar
import gn_ref as gr
import helpers as hp
from kandinsky2_amd import _lib

DT_IDS = [gr.DT_NAME[d] for d in gr.DTYPES]
ADT_IDS = [gr.DT_NAME[d] for d in gr.APPLY_DTYPES]


def close(a, b, tol=1e-12):
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


def as_T(ref, dtype):
    """what a correct kernel would store: the reference rounded once to T (fp32 stands in for the hi + lo of an x3 chunk)"""
    return ref.to(hp.tdt(gr.storage(dtype)))


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gr.E2E_CASES[:6], ids=lambda c: "-".join(str(v) for v in c))
def test_a_restatements_equal_torch_float64(case):
    C0, C1, B, H, W, fam, film, act, mode, pad = case
    d = gr.e2e_inputs(case, gr.F32)
    x = d["x"].double()
    Cn, HW = C0 + C1, H * W
    ns = gr.nsplit(B, HW)
    rows = gr.stats_ref(x.view(B, HW, Cn), ns)
    # the statistics rows as two sources of a virtual concat (when the case has one), through the coefficient and the apply restatements
    if C1:
        srcs = [(rows[..., :C0, :].reshape(B * ns, C0, 2), ns, C0), (rows[..., C0:, :].reshape(B * ns, C1, 2), ns, C1)]
    else:
        srcs = [(rows.reshape(B * ns, Cn, 2), ns, Cn)]
    c = gr.coeff_ref(srcs, B, HW, d["gamma"], d["beta"], d["film"], 1e-5)
    got, _ = gr.apply_ref(x, c["coeff"], act, mode, pad, gr.F32)
    want = gr.e2e_torch(x, d["gamma"], d["beta"], d["film"], 1e-5, act, mode, pad)
    assert got.shape == want.shape and close(got, want)
    zero = torch.zeros(B, Cn, dtype=torch.float64)
    assert close(gr.e2e_ref(x, d["gamma"], d["beta"], d["film"], 1e-5, act, mode, pad, gr.F32, zero, zero)[0], want)


def test_a_geometry():
    assert gr.nsplit(1, 2500) == 64 and gr.empty_ranges(2500, 64) == [63] and gr.nsplit(2, 70) == 2 and gr.nsplit(5, 25) == 1
    assert [gr.lanes(c) for c in gr.STATS_C] == [8, 4, 2, 1, 1, 1, 1, 1]
    # 35 pixels, one lane: 4 chain steps + the tree + 3 left over + the square; 40 pixels on 8 lanes: 5 each, one by one, + 8 lane sums
    assert gr.stats_n(70, 2, 1024) == 2 * (4 + 3 + 3 + 1) and gr.stats_n(2500, 64, 128) == 2 * (5 + 8 + 1)
    assert gr.out_hw(7, 9, 1) == (3, 4)                       # AvgPool2d's floor


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------
def test_b_statistics_fp32_inside_bounds():
    worst = {}
    for (C0, C1, B, HW) in gr.stats_cases():
        for dtype in gr.DTYPES:
            x = gr.stats_input(C0, C1, B, HW, dtype)
            ns = gr.nsplit(B, HW)
            nbad, ratio = gr.stats_check(gr.stats_ref(x, ns), x.double(), gr.stats_n(HW, ns, C0 + C1))
            assert nbad == 0, (C0, C1, B, HW, dtype, ratio)
            worst[dtype] = max(worst.get(dtype, 0.0), ratio)
    for dtype, r in worst.items():
        print(f"gn statistics, torch fp32 (CPU) {gr.DT_NAME[dtype]}: largest |error| / bound = {r:.3f}")
    assert max(worst.values()) < 1.0


def test_b_coefficients_fp32_inside_bounds():
    worst = 0.0
    for case in gr.COEFF_CASES:
        for dtype in gr.DTYPES:
            d = gr.coeff_inputs(case, dtype)
            B, HW, eps = case[4], case[5], case[6]
            assert gr.coeff_conditioned(d["srcs"], B, HW), case
            ref = gr.coeff_ref(d["srcs"], B, HW, d["gamma"], d["beta"], d["film"], eps)
            ev = gr.coeff_ref(d["srcs"], B, HW, d["gamma"], d["beta"], d["film"], eps, fp32=True)["coeff"]
            nbad, ratio = ar.violations(ev, ref["coeff"], ref["bound"])
            assert nbad == 0, (case, dtype, ratio)
            worst = max(worst, ratio)
    print(f"gn coefficients, torch fp32 after the two roundings (CPU): largest |error| / bound = {worst:.3f}")
    assert worst < 1.0


@pytest.mark.parametrize("dtype", gr.APPLY_DTYPES, ids=ADT_IDS)
def test_b_apply_fp32_inside_bounds(dtype):
    worst = 0.0
    for (C0, C1, B, H, W) in gr.apply_cases():
        d = gr.apply_inputs(C0, C1, B, H, W, dtype)
        x64, c64 = d["x"].double(), d["coeff"].double()
        for mode in (0, 1, 2):
            for act in (0, 1):
                ref, bound = gr.apply_ref(x64, c64, act, mode, 1, dtype)
                ev = as_T(gr.apply_torch32(d["x"], d["coeff"], act, mode, 1), dtype)
                nbad, ratio = ar.violations(ev, ref, bound)
                assert nbad == 0, (C0, C1, B, H, W, mode, act, ratio)
                worst = max(worst, ratio)
    print(f"gn apply, torch fp32 (CPU) {gr.DT_NAME[dtype]}: largest |error| / bound = {worst:.3f}")
    assert worst < 1.0


@pytest.mark.parametrize("dtype", gr.APPLY_DTYPES, ids=ADT_IDS)
def test_b_end_to_end_fp32_inside_bounds(dtype):
    worst = 0.0
    for case in gr.E2E_CASES:
        C0, C1, B, H, W, fam, film, act, mode, pad = case
        d = gr.e2e_inputs(case, dtype)
        x64 = d["x"].double()
        n = gr.stats_n(H * W, gr.nsplit(B, H * W), C0 + C1)
        ds, dq = gr.stats_bounds(x64.view(B, H * W, C0 + C1), n)
        ref, bound = gr.e2e_ref(x64, d["gamma"], d["beta"], d["film"], 1e-5, act, mode, pad, dtype, ds, dq)
        ev = as_T(gr.e2e_torch(d["x"], d["gamma"], d["beta"], d["film"], 1e-5, act, mode, pad), dtype)
        nbad, ratio = ar.violations(ev, ref, bound)
        assert nbad == 0, (case, ratio)
        worst = max(worst, ratio)
    print(f"gn end to end, torch fp32 (CPU) {gr.DT_NAME[dtype]}: largest |error| / bound = {worst:.3f}")
    assert worst < 1.0


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------------
def rejected(out, ref_mut, bound_mut):
    return ar.violations(out, ref_mut, bound_mut)[0] > 0


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=DT_IDS)
def test_c_statistics_and_coefficient_mutants_are_rejected(dtype):
    for (C0, C1, B, HW) in ((128, 0, 2, 70), (128, 0, 1, 2500), (1152, 768, 3, 70)):
        x = gr.stats_input(C0, C1, B, HW, dtype).double()
        ns = gr.nsplit(B, HW)
        n = gr.stats_n(HW, ns, C0 + C1)
        assert gr.stats_check(gr.stats_ref(x, ns).float(), x, n)[0] == 0
        assert gr.stats_check(gr.stats_ref(x, ns, "last_range_dropped").float(), x, n)[0] > 0
    muts = ("image_next", "rpi_other", "boundary_off_by_one", "second_ignored", "film_ld_2C", "film_row0", "film_swapped", "shift_first",
            "unbiased", "no_eps")
    for case in (gr.COEFF_CASES[1], gr.COEFF_CASES[4]):        # two sources, a straddling group, FiLM family b, B >= 2
        d = gr.coeff_inputs(case, dtype)
        B, HW, eps = case[4], case[5], case[6]
        args = (d["srcs"], B, HW, d["gamma"], d["beta"], d["film"], eps)
        good = gr.coeff_ref(*args, fp32=True)["coeff"]
        ref = gr.coeff_ref(*args)
        assert not rejected(good, ref["coeff"], ref["bound"])
        for mut in muts:
            m = gr.coeff_ref(*args, mut=mut)
            assert rejected(good, m["coeff"], m["bound"]), (case, mut)
    # eps on the near-constant group alone (family e, group 3)
    case = gr.COEFF_CASES[1]
    d = gr.coeff_inputs(case, dtype)
    args = (d["srcs"], case[4], case[5], d["gamma"], d["beta"], d["film"], case[6])
    good, m = gr.coeff_ref(*args, fp32=True)["coeff"], gr.coeff_ref(*args, mut="no_eps")
    cg = (case[0] + case[1]) // gr.GROUPS
    sl = slice(3 * cg, 4 * cg)
    assert rejected(good[:, sl], m["coeff"][:, sl], m["bound"][:, sl])


@pytest.mark.parametrize("dtype", gr.APPLY_DTYPES, ids=ADT_IDS)
def test_c_apply_mutants_are_rejected(dtype):
    for (C0, C1, B, H, W) in ((128, 0, 3, 7, 9), (128, 0, 1, 6, 10)):
        d = gr.apply_inputs(C0, C1, B, H, W, dtype)
        x64, c64 = d["x"].double(), d["coeff"].double()
        for (mut, act, mode) in (("silu_after_avg", 1, 1), ("up_plus_one", 0, 2), ("up_plus_one", 1, 2), ("xy_exchanged", 1, 0), ("xy_exchanged", 0, 2),
                                 ("border_in", 1, 0), ("border_in", 0, 1), ("border_in", 1, 2), ("border_nonzero", 1, 0), ("border_nonzero", 0, 2)):
            ref, bound = gr.apply_ref(x64, c64, act, mode, 1, dtype)
            good = as_T(ref, dtype)
            assert not rejected(good, ref, bound)
            rm, bm = gr.apply_ref(x64, c64, act, mode, 1, dtype, mut)
            assert rejected(good, rm, bm), (H, W, mut, act, mode)


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------------
def test_d_refusals():
    L = _lib.lib()
    P = 4096                                                   # a non-null pointer no refused call may touch
    EINVAL = -1
    ns = C.c_int(-7)
    for (C0, C1) in ((192, 0), (70, 58), (3200, 0), (64, 64 + 3072)):
        assert L.k22_gn_stats(P, P if C1 else None, C0, C1, 2, 16, P, C.byref(ns), gr.F32, None) == EINVAL, (C0, C1)
        assert L.k22_last_error()
    assert L.k22_gn_stats(P, None, 128, 128, 2, 16, P, C.byref(ns), gr.F32, None) == EINVAL          # C1 > 0 without x1
    assert L.k22_gn_stats(P, None, 128, 0, 2, 16, None, C.byref(ns), gr.F32, None) == EINVAL and ns.value == 0

    def coeff(st0=P, rpi0=2, C0=128, st1=P, rpi1=3, C1=256, B=2, HW=16, gamma=P, beta=P, film=P, film_ld=2 * 384 + 192, coeff=P):
        return L.k22_gn_coeff(st0, rpi0, C0, st1, rpi1, C1, B, HW, gamma, beta, film, film_ld, 1e-5, coeff, None)

    assert coeff(C1=240) == EINVAL                            # C % 32
    assert coeff(C0=8192, C1=32, film=None) == EINVAL                    # 257 channels per group
    assert coeff(rpi0=0) == EINVAL and coeff(rpi1=0) == EINVAL and coeff(rpi1=-1) == EINVAL
    assert coeff(st1=None) == EINVAL
    assert coeff(film_ld=2 * 384 - 1) == EINVAL
    assert coeff(gamma=None) == EINVAL and coeff(beta=None) == EINVAL and coeff(coeff=None) == EINVAL
    assert b"gn_coeff" in L.k22_last_error()

    def apply(C0=128, C1=0, x1=None, H=6, W=10, mode=0, pad=1, act=1, dtype=gr.BF16, coeff=P):
        return L.k22_gn_apply(P, x1, C0, C1, 2, H, W, coeff, act, mode, pad, P, dtype, None)

    assert apply(C0=132) == EINVAL and apply(C0=132, dtype=gr.F16) == EINVAL and apply(C0=130, dtype=gr.F32) == EINVAL and apply(C0=130, dtype=gr.X3) == EINVAL
    assert apply(C0=68, C1=60, x1=P) == EINVAL                # the first source's width splits a 16-byte vector
    assert apply(C1=128) == EINVAL and apply(mode=3) == EINVAL and apply(pad=2) == EINVAL and apply(act=2) == EINVAL and apply(coeff=None) == EINVAL
    assert apply(H=1, mode=1) == EINVAL and apply(dtype=7) == EINVAL
