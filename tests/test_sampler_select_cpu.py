"""CPU half of the single-kernel parity of k22_sampler_step (tests/sampler_ref.py, tests/test_sampler_select_gpu.py), on the reference alone:
 (a) the host model of the dispatch labels the select items so that every path of sampler_threshold_kernel occurs: the five labels, every
     KPT in {16, 36, 64} both filtered and fallen back, both sides of pct_gamma = 0.5, the template edges;
 (b) the conditions under which an item can tell a wrong select from a right one hold: percentile above 1, s changes in bits with the rank,
     image 1 gives another s;
 (c) a numpy emulation of the select passes the class-E comparison at every item, and each of five wrong variants fails it somewhere;
 (d) the restatements are numpy's percentile and the update formulas; an fp32 evaluation of a correct step passes the class-D / class-M
     comparators at every parity item, wrong operands do not; the CPU yardstick of class M is printed."""
import collections

import numpy as np
import pytest
import torch

import sampler_ref as sp
from kandinsky2_amd.diffusion import percentile_index

Item = collections.namedtuple("Item", "HW case N cfg x0 lo gamma disp s")


@pytest.fixture(scope="module")
def items():
    """every select item once: the stored x0 a correct x0 kernel leaves, the rank, the model's label, the reference s"""
    out = []
    for (HW, case, N, cfg) in sp.select_items():
        d = sp.select_input(HW, case, N)
        x0 = sp.select_x0(d).numpy().reshape(N, 4 * HW)
        lo, gamma = percentile_index(4 * HW)
        out.append(Item(HW, case, N, cfg, x0, lo, gamma, sp.dispatch(x0[0], lo), sp.s_ref(x0[0])))
    return out


# ---- (a) branch coverage by the host model ------------------------------------------------------------------------------------------------------
def test_a_template_edges():
    assert [sp.template_kpt(4 * hw) for hw in (1, 1024, 1025, 4096, 4097, 9216, 9217, 16384, 16385, 20000)] == [4, 4, 16, 16, 36, 36, 64, 64, 0, 0]
    # a key count that is no multiple of 1024 occurs under every KPT >= 16
    assert {sp.template_kpt(4 * hw) for hw in sp.SELECT_HW if (4 * hw) % 1024} >= {4, 16, 36, 64, 0}
    assert sp.sample_positions(4 * 1794).size == 449 and sp.sample_positions(4 * 2047).size == 512 and sp.sample_positions(4 * 4097).size < 512


def test_a_every_path_occurs(items):
    per_label = collections.Counter(it.disp.label for it in items)
    print("select items per path label:", dict(per_label), "of", len(items))
    assert set(per_label) == set(sp.LABELS)
    for K in (16, 36, 64):
        got = {it.disp.label for it in items if it.disp.KPT == K}
        assert {"filtered", "fall-back"} <= got, (K, got)
    assert {it.disp.KPT for it in items if it.disp.label == "few-samples"} == {16, 36}
    for it in items:
        if it.case == "sample_large":
            assert it.disp.label == ("fall-back" if it.disp.ns >= 512 else "few-samples"), it[:4]
        if it.case == "sample_small" and it.disp.ns >= 512:
            assert it.disp.label == "filtered", it[:4]
        if it.case == "sample_is_answer" and it.disp.ns >= 512:
            assert it.disp.label == "filtered" and it.disp.pivot == sp.f32bits(1.6), it[:4]
    fell = sorted({it.HW for it in items if it.disp.label == "fall-back"})
    assert fell == [2047, 2048, 2304, 4096, 9216, 9217, 16384]
    gammas = {hw: percentile_index(4 * hw)[1] for hw in sp.SELECT_HW}
    assert abs(gammas[1024] - 0.525) < 1e-3 and abs(gammas[2048] - 0.045) < 1e-3
    assert any(g >= 0.5 for g in gammas.values()) and any(0.0 < g < 0.5 for g in gammas.values())


# ---- (b) visibility and distinguishability ------------------------------------------------------------------------------------------------------
def test_b_conditions_hold_on_the_reference(items):
    for it in items:
        n = 4 * it.HW
        p = sp.percentile_at(it.x0[0], it.lo, it.gamma)
        assert sp.f32bits(max(p, np.float32(1))) == sp.f32bits(it.s), it[:4]          # lerp32 restates numpy's lerp
        assert p > 1.0, (it[:4], p)
        if it.case in sp.TIE_CASES:
            continue
        assert it.lo >= 1
        for other in (it.lo - 1, it.lo + 1):
            if other + 1 < n:          # both order statistics of the replaced rank exist (at n = 4, rank lo + 1 is the last key)
                q = sp.percentile_at(it.x0[0], other, it.gamma)
                assert sp.f32bits(max(q, np.float32(1))) != sp.f32bits(it.s), (it[:4], other)
        if it.case == "image0_only":
            assert sp.f32bits(sp.s_ref(it.x0[1])) != sp.f32bits(it.s), it[:4]
    assert {(it.N, it.cfg) for it in items if it.case == "image0_only"} == {(2, 1), (3, 0)}
    # the ramps put ranks lo and lo + 1 on the two sides of a digit edge of the radix plan (11 + 11 + 10 bits)
    for it in items:
        if it.case.startswith("ulp_ramp"):
            k = np.sort(sp.keys_of(it.x0[0]))
            a, b = int(k[it.lo]), int(k[it.lo + 1])
            assert b == a + 1 and (a >> 10) != (b >> 10) and ((a >> 21) != (b >> 21)) == (it.case == "ulp_ramp_top"), it[:4]
        if it.case == "binades":
            d = sp.keys_of(it.x0[0]) >> 21
            assert np.unique(d).size >= 38 * 4 - 8 and (np.abs(it.x0[0]) > 2).any()   # 40 binades x 4 top digits each, nearly all of them hit


# ---- (c) the emulation of the select and its wrong variants ---------------------------------------------------------------------------------------
def test_c_emulation_passes_and_wrong_variants_fail(items):
    caught = {v: [] for v in sp.VARIANTS}
    for it in items:
        assert sp.f32bits(sp.select_emul(it.x0, it.lo, it.gamma)) == sp.f32bits(it.s), it[:4]
        for v in sp.VARIANTS:
            if sp.f32bits(sp.select_emul(it.x0, it.lo, it.gamma, v)) != sp.f32bits(it.s):
                caught[v].append((it.HW, it.case))
    for v in sp.VARIANTS:
        print(f"wrong select '{v}': fails the class-E comparison at {len(caught[v])} of {len(items)} items")
        assert caught[v], v
    assert any(c == "two_values" for _, c in caught["next_distinct"])
    assert {hw for hw, c in caught["no_fall_back"]} >= {2047, 4096, 9216, 16384}
    assert any(c == "image0_only" for _, c in caught["image_1"])


# ---- (d) restatements, accepted fp32 evaluations, the class-M yardstick ----------------------------------------------------------------------------
def test_d_refs_are_the_update_formulas():
    """gaussian_diffusion's step written out per element in numpy float64"""
    N, HW = 4, 35
    d = sp.parity_input(N, HW)
    g = float(np.float32(sp.GUIDANCE))
    x, mo, nz, init, m = (d[k].double().numpy() for k in ("x", "mo", "noise", "init", "mask"))
    e = np.empty_like(x)
    for n in range(N):
        e[n] = mo[n % 2 + 2, :4] + g * (mo[n % 2, :4] - mo[n % 2 + 2, :4])
    for k in sp.PARITY_ROWS:
        sr, srm1, c1, c2, mnl, mxl, nonzero, _ = (float(v) for v in sp.table()[k])
        x0 = np.clip(sr * x - srm1 * e, -2.0, 2.0)
        x0 = x0 * (1 - m) + init * m
        got, bound = sp.x0_ref(d, sp.table()[k], 1, 2.0, True)
        assert np.abs(got.numpy() - x0).max() <= 1e-12 and bool((bound > 0).all())
        s = sp.s_ref(got[0].float().numpy())
        x0t = np.clip(x0, -float(s), float(s)) / float(s)
        frac = (mo[:, 4:] + 1) / 2
        want = c1 * x0t + c2 * x + nonzero * np.exp(0.5 * (frac * mxl + (1 - frac) * mnl)) * nz
        out, z, S = sp.final_ref(torch.from_numpy(x0), s, d, sp.table()[k])
        assert np.abs(out.numpy() - want).max() <= 1e-12 and np.abs(z.numpy() - x0t).max() <= 1e-12 and bool((S >= out.abs() - 1e-12).all())
    rows = sp.table()
    assert rows.dtype == np.float32 and rows[2, 6] == 0 and rows[0, 6] == 1 and rows[sp.SELECT_ROW, 0] == 1 and rows[sp.SELECT_ROW, 1] == 0
    assert sp.x0_n(1, False) == 12 and sp.x0_n(0, False) == 6 and sp.x0_n(1, True) == 20 and sp.x0_n(0, True) == 14


def test_d_fp32_step_is_accepted_wrong_operands_are_not():
    yard = 0.0
    for HW in sp.PARITY_HW:
        for (N, cfg) in sp.PARITY_BATCH:
            d = sp.parity_input(N, HW)
            for k in sp.PARITY_ROWS:
                row = sp.table()[k]
                for masked in (False, True):
                    ref, bound = sp.x0_ref(d, row, cfg, sp.PARITY_CLAMP, masked)
                    x0 = sp.x0_ref(d, row, cfg, sp.PARITY_CLAMP, masked, dtype=torch.float32)[0]
                    assert sp.violations(x0, ref, bound)[0] == 0, ("x0", N, HW, cfg, k, masked)
                    for thr in (True, False):
                        s = sp.s_ref(x0[0].numpy()) if thr else None
                        out, z, S = sp.final_ref(x0, s, d, row)
                        b_out, b_z = sp.final_bounds(z, S, thr)
                        o32, z32, _ = sp.final_ref(x0, s, d, row, dtype=torch.float32)
                        assert sp.violations(o32, out, b_out)[0] == 0 and sp.violations(z32, z, b_z)[0] == 0, ("final", N, HW, cfg, k, masked, thr)
                        yard = max(yard, sp.yardstick(x0, s, d, row))
                    # resolving power on these operands: a dropped mask, the other half's eps rows, dropped noise, a threshold not applied
                    if masked:
                        assert sp.violations(x0, *sp.x0_ref(d, row, cfg, sp.PARITY_CLAMP, False))[0] > 0
                    if cfg and N > 2:
                        swapped = dict(d, mo=torch.cat([d["mo"][1:2], d["mo"][0:1], d["mo"][2:]]))
                        assert sp.violations(x0, *sp.x0_ref(swapped, row, cfg, sp.PARITY_CLAMP, masked))[0] > 0
                    s = sp.s_ref(x0[0].numpy())
                    o32 = sp.final_ref(x0, s, d, row, dtype=torch.float32)[0]
                    if row[6] != 0:
                        out, z, S = sp.final_ref(x0, s, dict(d, noise=torch.zeros_like(d["noise"])), row)
                        assert sp.violations(o32, out, sp.final_bounds(z, S, True)[0])[0] > 0
                    if s > 1:
                        out, z, S = sp.final_ref(x0, None, d, row)
                        assert sp.violations(o32, out, sp.final_bounds(z, S, False)[0])[0] > 0
    print(f"sampler_final x_out yardstick (CPU), parity items: {yard:.3f} (c = {sp.SAMPLER_C})")
    assert yard < sp.SAMPLER_C


def test_d_yardstick_on_the_select_items(items):
    yard = 0.0
    row = sp.table()[sp.SELECT_ROW]
    for it in items:
        d = sp.select_input(it.HW, it.case, it.N)
        x0 = torch.from_numpy(it.x0).view(it.N, 4, it.HW)
        out, z, S = sp.final_ref(x0, it.s, d, row)
        b_out, b_z = sp.final_bounds(z, S, True)
        o32, z32, _ = sp.final_ref(x0, it.s, d, row, dtype=torch.float32)
        assert sp.violations(o32, out, b_out)[0] == 0 and sp.violations(z32, z, b_z)[0] == 0, it[:4]
        yard = max(yard, sp.yardstick(x0, it.s, d, row))
    print(f"sampler_final x_out yardstick (CPU), select items: {yard:.3f} (c = {sp.SAMPLER_C})")
    assert yard < sp.SAMPLER_C
