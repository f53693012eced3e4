"""CPU part of the skinny family's float64 parity (tests/skinny_ref.py; the device part is tests/test_skinny_parity_gpu.py):
 (a) torch's own fp32 evaluation of every operation - outputs rounded to T where the kernel stores T, GELU through the fp32 restatement of
     gelu_fast - lies inside every bound on every case and family in both types: the inputs are fit and the bounds are not tight by accident;
     the yardsticks that set the constants are printed;
 (b) every mutant of the restatements is rejected by the bound in bf16 and in fp16;
 (c) the index functions are bijections onto [0, 32 MA K) and [0, Npad K), and k22_afrag_bytes agrees."""
import pytest
import torch

import skinny_ref as sr
from kandinsky2_amd import _lib

ar, atr, hp = sr.ar, sr.atr, sr.hp
DT_IDS = [sr.DT_NAME[d] for d in sr.DTYPES]


def stored(x, dtype):
    return x.to(hp.tdt(dtype)).double()


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------
def test_c_index_functions_are_bijections():
    for M, K in ((1, 64), (31, 128), (32, 64), (33, 128), (81, 192), (193, 320)):
        idx = sr.afrag_index(32 * ((M + 31) // 32), K).reshape(-1)          # all rows of every m-atom, padding included
        assert torch.equal(idx.sort().values, torch.arange(sr.afrag_elems(M, K)))
        assert torch.equal(sr.afrag_index(M, K), sr.afrag_index(32 * ((M + 31) // 32), K)[:M])
        assert _lib.lib().k22_afrag_bytes(M, K) == 2 * sr.afrag_elems(M, K)
        v = torch.arange(M * K, dtype=torch.float64).reshape(M, K)
        buf = sr.afrag_expected(v)
        assert torch.equal(sr.from_afrag(buf, M, K), v) and int(torch.isnan(buf).sum()) == sr.afrag_elems(M, K) - M * K
    for Npad, K in ((64, 128), (128, 64), (256, 320)):
        idx = sr.wfrag_index(Npad, K).reshape(-1)
        assert torch.equal(idx.sort().values, torch.arange(Npad * K))
    # one 32 x 16 MFMA fragment is 1 KB contiguous: lane l holds row l & 31, k-values 8 (l >> 5) .. + 7
    f = sr.wfrag_index(64, 128)[32:64, 80:96].reshape(-1).sort().values
    assert int(f[0]) % 512 == 0 and torch.equal(f - f[0], torch.arange(512))
    assert int(sr.wfrag_index(64, 128)[37, 89]) - int(f[0]) == (5 + 32) * 8 + 1


def test_c_cases_cover_what_they_claim():
    cs = sr.GEMM_CASES
    assert {(c.mt, c.nb) for c in cs} == set(sr.TILES) | {(0, 0)}
    assert {c.M for c in cs} == {1, 31, 32, 33, 96, 97, 162, 193} and {c.N for c in cs} == {4, 60, 64, 68, 200}
    assert {sr.npad(c) for c in cs} >= {64, 128, 256} and {c.act for c in cs} == {0, 1, 2} and {c.bias for c in cs if c.epi != 2} == {0, 1}
    for tile in sr.TILES:
        mine = [c for c in cs if (c.mt, c.nb) == tile]
        D = sr.ring_depth(mine[0])
        lens = {c1 - c0 for c in mine for (c0, c1) in sr.chunk_ranges(c.K, c.splitk)}
        assert lens >= {1, D - 1, D, D + 1, 3 * D - 1}, (tile, sorted(lens))
        assert {c.epi for c in mine} == {0, 1, 2}, tile
        assert all(sr.npad(c) % (32 * c.nb) == 0 for c in mine)
    assert any(min(c1 - c0 for (c0, c1) in sr.chunk_ranges(c.K, c.splitk)) <= 0 for c in cs)           # an empty split
    assert any([c1 - c0 for (c0, c1) in sr.chunk_ranges(c.K, c.splitk)] == [5, 4] for c in cs)
    assert any(c.M == 193 and c.mt in (3, 6) for c in cs) and any(c.M == 162 and c.mt == 6 for c in cs)
    assert any(c.epi == 0 and c.slack for c in cs) and all(c.N % 64 == 0 for c in cs if c.epi == 1)
    assert any(c.epi == 1 and c.M % 32 for c in cs)
    fs = sr.FLN_CASES
    assert {c.M for c in fs} == {1, 5, 33} and {c.N for c in fs} == {8, 64, 72, 512, 2040, 2048} and {c.splitk for c in fs} == {0, 1, 2, 7, 8}
    assert {c.slack for c in fs} == {0, 4} and all(c.N % 64 == 0 for c in fs if c.ln) and {(c.ln, c.bias) for c in fs if c.splitk} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    at = sr.ATT_CASES
    assert {c.T for c in at} == {1, 31, 32, 33, 64, 65, 81, 96, 97, 127, 128} and {c.H for c in at} == {1, 3} == {c.B for c in at}
    assert {c.nsplit for c in at} == {0, 1, 2, 4} and {c.frag for c in at} == {0, 1} and {c.causal for c in at} == {0, 1}
    assert any(c.n_valid is not None and c.kv_n < c.T for c in at) and any(c.n_valid is not None and c.kv_n == c.T for c in at)
    assert any(c.frag and (c.B * c.T) % 32 and c.B > 1 and c.T % 32 for c in at)


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------
def test_a_gelu_fast_restatement_fits_its_term():
    x = torch.cat([torch.linspace(-12.0, 12.0, 200001), torch.tensor([0.0, -0.0, 1e-6, -1e-6, 30.0, -30.0])])
    err = (sr.gelu_fast32(x).double() - hp.act64(x.double(), sr.ACT_GELU)).abs()
    term = sr.gemm_e_act(x.double(), sr.ACT_GELU)
    ratio = (err[term > 0] / term[term > 0]).max().item()
    print(f"gelu_fast32 against float64 erf GELU: largest |error| / e_act = {ratio:.3f} (e_act = {sr.GELU_FAST_REL:.3e} |x|)")
    assert bool((err <= term).all()) and ratio < 1.0


def test_a_torch_fp32_gemm_fits():
    yard = {f: 0.0 for f in sr.GEMM_FAMILIES}
    worst = {}
    for c in sr.GEMM_CASES:
        for fam in sr.GEMM_FAMILIES:
            d = sr.gemm_inputs(c, fam)
            for dt in sr.DTYPES:
                r = sr.gemm_ref(sr.gemm_seen(d, dt), c)
                t = sr.gemm_ref(sr.gemm_seen(d, dt, f64=False), c)
                y = ar.plain_ratio(t["pre"], r["pre"], r["S"])
                yard[fam] = max(yard[fam], y)
                assert y < sr.GEMM_C, (sr.gemm_id(c), fam, y)
                bound = sr.gemm_bound(r, c, dt)
                if c.epi == sr.EPI_PARTIAL:
                    nbad, ratio = ar.violations(t["parts"].double().sum(0), r["pre"], bound)
                    assert bool(torch.isfinite(t["parts"]).all())
                else:
                    nbad, ratio = ar.violations(stored(t["ref"], dt), r["ref"], bound)
                key = (c.epi, dt)
                worst[key] = max(worst.get(key, 0.0), ratio)
                assert nbad == 0, (sr.gemm_id(c), fam, sr.DT_NAME[dt], nbad, ratio)
    print("torch fp32 matmul yardstick (CPU), largest over cases and types: " + "  ".join(f"{f} {y:.2f}" for f, y in yard.items()) + f"  (c = {sr.GEMM_C})")
    print("torch fp32 evaluation, largest |out - ref| / bound: " + "  ".join(f"epi{e}-{sr.DT_NAME[dt]} {r:.2f}" for (e, dt), r in sorted(worst.items())))
    assert max(yard.values()) <= 7.401                                   # the rule: helpers.IGEMM_C holds up to this reading


def test_a_torch_fp32_finish_ln_fits():
    yard, worst = 0.0, {dt: 0.0 for dt in sr.DTYPES}
    for c in sr.FLN_CASES:
        d = sr.fln_inputs(c)
        xu = sr.x_chain32(d)
        assert bool(torch.isfinite(xu).all())
        if c.splitk:                                                        # the chain against the float64 sum: a handful of fp32 roundings
            p64 = d["partial"].double()
            s64 = p64.sum(0) + (0 if d["bias"] is None else d["bias"].double()) + d["x"].double()
            sab = p64.abs().sum(0) + (0 if d["bias"] is None else d["bias"].abs().double()) + d["x"].abs().double()
            assert bool(((xu.double() - s64).abs() <= (c.splitk + 1) * sr.U24 * sab).all()), sr.fln_id(c)
        if not c.ln:
            continue
        ref, S = sr.fln_ln_ref(xu.double(), d["g"].double(), d["b"].double())
        t = torch.nn.functional.layer_norm(xu, (c.N,), d["g"], d["b"], sr.FLN_EPS)
        y = ar.plain_ratio(t, ref, S)
        yard = max(yard, y)
        assert y < sr.LN_C, (sr.fln_id(c), y)
        for dt in sr.DTYPES:
            nbad, ratio = ar.violations(stored(t, dt), ref, sr.fln_bound(ref, S, dt))
            worst[dt] = max(worst[dt], ratio)
            assert nbad == 0, (sr.fln_id(c), sr.DT_NAME[dt], nbad, ratio)
    print(f"torch fp32 F.layer_norm yardstick (CPU) on the finish_ln rows: {yard:.2f}  (c = {sr.LN_C:.2f}, set by 4.458)")
    print("torch fp32 evaluation, largest |out - ref| / bound: " + "  ".join(f"{sr.DT_NAME[dt]} {r:.2f}" for dt, r in worst.items()))
    assert yard <= 4.458


def test_a_torch_fp32_attention_fits():
    yard = {f: 0.0 for f in sr.ATT_FAMILIES}
    worst = {dt: 0.0 for dt in sr.DTYPES}
    for c in sr.ATT_CASES:
        for fam in sr.ATT_FAMILIES:
            d = sr.att_inputs(c, fam)
            for dt in sr.DTYPES:
                q, k, v = sr.att_operands(sr.att_stage32(d, c, dt))
                ref, bound, A, amp = sr.att_ref(q, k, v, c, d["key_valid"], dt)
                assert bool(torch.isfinite(ref).all()), sr.att_id(c)      # the precondition: every query keeps a live key
                t = atr.plain32(q, k, v, sr.att_case(c), d["key_valid"])
                y = atr.yardstick(t, ref, A, amp)
                yard[fam] = max(yard[fam], y)
                assert y < sr.ATT_C, (sr.att_id(c), fam, y)
                nbad, ratio = ar.violations(stored(t, dt), ref, bound)
                worst[dt] = max(worst[dt], ratio)
                assert nbad == 0, (sr.att_id(c), fam, sr.DT_NAME[dt], nbad, ratio)
    print("torch fp32 attention yardstick (CPU): " + "  ".join(f"{f} {y:.2f}" for f, y in yard.items()) + f"  (c = {sr.ATT_C})")
    print("torch fp32 evaluation, largest |out - ref| / bound: " + "  ".join(f"{sr.DT_NAME[dt]} {r:.2f}" for dt, r in worst.items()))
    assert ar.c_rule(max(yard.values())) <= sr.ATT_C


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------
def share_outside(wrong, ref, bound):
    """fraction of the elements of a buffer at which `wrong` is outside the bound (or fill / value disagree)"""
    o = wrong.double()
    owned = ~torch.isnan(ref)
    bad = torch.where(owned, ~((o - torch.where(owned, ref, torch.zeros_like(ref))).abs() <= bound), ~torch.isnan(o))
    return bad.double().mean().item()


def gemm_mutant_cases(mut):
    cs = sr.GEMM_CASES
    if mut == "chunk_doubled":
        return [c for c in cs if c.splitk > 1]
    if mut == "pad_row_added":
        return [c for c in cs if c.M % 32]
    if mut in ("bias_shift4", "bias_tail_missing"):
        return [c for c in cs if c.bias and c.epi != 2]
    if mut in ("act_before_bias", "act_missing"):
        return [c for c in cs if c.act and c.bias and c.epi != 2]
    if mut == "ldo_as_N":
        return [c for c in cs if c.slack and c.M > 1]
    return cs


@pytest.mark.parametrize("mut", sr.GEMM_MUTANTS)
def test_b_gemm_mutant_is_rejected(mut):
    cases = gemm_mutant_cases(mut)
    assert cases
    for dt in sr.DTYPES:
        best, least = 0.0, 1.0
        for c in cases:
            for fam in sr.GEMM_FAMILIES:
                s = sr.gemm_seen(sr.gemm_inputs(c, fam), dt)
                r, w = sr.gemm_ref(s, c), sr.gemm_ref(s, c, mut)
                bound = sr.gemm_bound(r, c, dt)
                if c.epi == sr.EPI_PARTIAL:
                    share = share_outside(w["parts"].sum(0), r["pre"], bound)
                    assert ar.violations(r["parts"].float().double().sum(0), r["pre"], bound)[0] == 0
                else:
                    exp, bnd = sr.gemm_layout(r["ref"], c), sr.gemm_layout(bound, c, 0.0)
                    share = share_outside(sr.gemm_layout(stored(w["ref"], dt), c, mut=mut), exp, bnd)
                    assert ar.violations(sr.gemm_layout(stored(r["ref"], dt), c), exp, bnd)[0] == 0   # the right value, rounded, passes
                best, least = max(best, share), min(least, share)
        print(f"{mut} {sr.DT_NAME[dt]}: outside the bound on {100 * least:.1f}-{100 * best:.1f} % of a case's elements ({len(cases) * 3} case x family pairs)")
        assert best > 0.0, (mut, sr.DT_NAME[dt])


def fln_mutant_cases(mut):
    cs = [c for c in sr.FLN_CASES if c.splitk]
    if mut in ("last_split_missing", "last_split_twice", "x_not_written"):
        return cs
    if mut == "bias_missing":
        return [c for c in cs if c.bias]
    if mut == "div2048":
        return [c for c in sr.FLN_CASES if c.ln and c.N < 2048]
    if mut in ("one_pass", "eps_missing"):
        return [c for c in sr.FLN_CASES if c.ln and c.M >= 5]
    return [c for c in sr.FLN_CASES if c.ln]


@pytest.mark.parametrize("mut", sr.FLN_MUTANTS)
def test_b_finish_ln_mutant_is_rejected(mut):
    cases = fln_mutant_cases(mut)
    assert cases
    x_mut = mut in ("last_split_missing", "last_split_twice", "bias_missing", "x_not_written")
    for dt in sr.DTYPES:
        best = 0.0
        for c in cases:
            d = sr.fln_inputs(c)
            xu = sr.x_chain32(d)
            if x_mut:                                                       # class E: one differing bit pattern is a failure
                best = max(best, (sr.x_chain32(d, mut).view(torch.int32) != xu.view(torch.int32)).double().mean().item())
                continue
            ref, S = sr.fln_ln_ref(xu.double(), d["g"].double(), d["b"].double())
            wrong, _ = sr.fln_ln_ref(xu.double(), d["g"].double(), d["b"].double(), mut=mut)
            bound = sr.fln_bound(ref, S, dt)
            assert ar.violations(stored(ref, dt), ref, bound)[0] == 0
            best = max(best, share_outside(sr.afrag_expected(stored(wrong, dt)), sr.afrag_expected(ref), sr.afrag_expected(bound, 0.0)))
        print(f"{mut} {sr.DT_NAME[dt]}: rejected on up to {100 * best:.1f} % of a case's elements ({len(cases)} cases)")
        assert best > 0.0, (mut, sr.DT_NAME[dt])


def att_mutant_cases(mut):
    cs = sr.ATT_CASES
    if mut in ("causal_strict", "causal_plus1"):
        return ("edges", "rand"), [c for c in cs if c.causal and c.T > 1]
    if mut == "one_pad_key_alive":
        return ("neg",), [c for c in cs if c.T % 32]
    if mut == "kvn_ignored":
        return ("edges", "rand"), [c for c in cs if c.n_valid is not None and c.kv_n < c.T]
    if mut == "last_key_dropped":
        return ("edges",), [c for c in cs if c.T > 1 and not c.causal and c.n_valid is None]
    if mut in ("bias_wrong_plane", "last_partial_twice"):
        return ("rand", "neg"), [c for c in cs if c.nsplit]
    assert mut == "valid_next_image"
    return ("edges", "neg"), [c for c in cs if c.n_valid is not None and c.B > 1 and c.T > 1]


@pytest.mark.parametrize("mut", sr.ATT_MUTANTS)
def test_b_attention_mutant_is_rejected(mut):
    fams, cases = att_mutant_cases(mut)
    assert cases
    for dt in sr.DTYPES:
        best = 0.0
        for c in cases:
            for fam in fams:
                d = sr.att_inputs(c, fam)
                q, k, v = sr.att_operands(sr.att_stage32(d, c, dt))
                ref, bound, _, _ = sr.att_ref(q, k, v, c, d["key_valid"], dt)
                assert ar.violations(stored(ref, dt), ref, bound)[0] == 0
                qm, km, vm = sr.att_operands(sr.att_stage32(d, c, dt, mut))
                wrong = sr.att_ref(qm, km, vm, c, d["key_valid"], dt, mut)[0]
                best = max(best, share_outside(stored(wrong, dt), ref, bound))
        print(f"{mut} {sr.DT_NAME[dt]}: rejected on up to {100 * best:.1f} % of a case's elements ({len(cases) * len(fams)} case x family pairs)")
        assert best > 0.0, (mut, sr.DT_NAME[dt])
