"""Host-side half of the tile-table sweep (tests/test_tile_table_gpu.py runs the lines on the device):

  * every line of the SHIPPED table (kandinsky-2_amd/tiles_gfx950.txt) names a configuration this build generates for that problem
    (k22_igemm_cfg_accepted = tuned_is_candidate over the descriptor the engines build) - a rejected line is dropped silently at lookup,
    the shape is timed again on every start and "the same bits on every box" is gone;
  * the float64 reference of helpers.py (written from the operation's definition) agrees with F.conv2d / F.linear on every feature it
    restates;
  * the element-wise comparator passes a CPU emulation of a correct kernel (T-rounded operands, fp32 matmul, one output rounding) and
    fails six ways a kernel goes subtly wrong - the first of which the older metric of the unit tests, max-abs against 1.2e-2 * max|ref|,
    does not notice at K = 13824;
  * the two plain fp32 evaluations IGEMM_C is derived from, measured on the host.
"""
import collections

import pytest
import torch
import torch.nn.functional as F

import helpers as hp
from kandinsky2_amd import _lib

BF16, F32, F16, X3, X2 = _lib.K22_BF16, _lib.K22_F32, _lib.K22_F16, _lib.K22_F16X3, _lib.K22_F16X2
CPU = torch.device("cpu")


def line(dtype=BF16, taps=9, B=1, H=8, W=8, N=64, Kc=64, K0=None, out_mode=0, res_f32=0, act=0, a_raw=0, stats=0, sk=0, M=None):
    M = B * H * W if M is None else M
    return hp.TileLine(dtype, taps, M, N, Kc, Kc if K0 is None else K0, H, W, out_mode, res_f32, act, a_raw, stats, sk, 1, 128, 64, 1, 2)


# ---- 1. the shipped table ---------------------------------------------------------------------------------------------------------

def test_every_line_of_the_shipped_table_is_a_configuration_this_build_generates():
    table = hp.read_tile_table()
    with open(_lib.TILE_TABLE_PATH) as f:
        assert len(table) == sum(1 for ln in f if ln.strip() and not ln.startswith("#")) and len(table) > 0
    own_x2 = {hp.tile_key(t) for t in table if t.dtype == X2}
    rejected, checked = [], collections.Counter()
    for t in table:
        runs_as = [t.dtype]
        if t.dtype == BF16:
            runs_as.append(F16)                       # tuned_key: fp16 resolves through the bf16 lines
        if t.dtype == X3 and hp.tile_key(t) not in own_x2:
            runs_as.append(X2)                        # tile_table_lookup: x2 falls back to the x3 line
        for dt in runs_as:
            checked[dt] += 1
            if hp.tile_accepted(t, dt) != 1:
                rejected.append(hp.tile_id(t, dt))
    assert not rejected, f"{len(rejected)} table lines name a configuration this build does not generate: {rejected[:20]}"
    n_x2_own = sum(1 for t in table if t.dtype == X2)
    assert checked[BF16] + checked[F32] + checked[X3] + n_x2_own == len(table)           # zero lines left out
    assert checked[F16] == checked[BF16] > 0 and checked[X2] > n_x2_own > 0               # + the fp16 and x2 fall-back readings


def test_acceptance_entry_tells_a_foreign_configuration_from_a_generated_one():
    t = next(t for t in hp.read_tile_table() if t.dtype == BF16 and t.taps == 9 and t.algo == 12 and t.splitk == 1)
    assert hp.tile_accepted(t) == 1
    assert hp.tile_accepted(t._replace(bm=192)) == 0                    # no such tile
    assert hp.tile_accepted(t._replace(splitk=7)) == 0                  # not a split-K factor of the candidate list
    assert hp.tile_accepted(t._replace(algo=20, bm=160)) == 0           # has_frag follows algo in tile_problem ...
    g = next(t for t in hp.read_tile_table() if t.dtype == BF16 and t.algo == 20)
    pr = hp.tile_problem(g)
    pr.has_frag = 0                                                     # ... the streaming kernel without fragment-major weights
    import ctypes as C
    assert _lib.lib().k22_igemm_cfg_accepted(C.byref(pr)) == 0
    assert hp.tile_accepted(g._replace(dtype=F32)) == 0                 # 16-bit types only
    bad = hp.tile_problem(t)
    bad.taps = 5
    assert _lib.lib().k22_igemm_cfg_accepted(C.byref(bad)) == _lib.lib().k22_igemm_cfg_accepted(None) == -1


@pytest.mark.parametrize("algo", [8, 9, 13, 14])
def test_reserved_algorithm_numbers_name_no_kernel(algo, tmp_path):
    """8, 9, 13 and 14 once named measurement-only kernels; the numbers stay reserved (IgemmAlgo, kernels.h).  For a 3x3 problem the table
    knows - bf16, 768 -> 768 at 96x96, batch 4 - none of them is a configuration this build generates, the launch entry refuses them on the
    host, and as a "conv_algo" option they mean "auto": the problem's table line and the fixed choice are what they were"""
    import ctypes as C
    L = _lib.lib()
    t = next(t for t in hp.read_tile_table() if (t.dtype, t.taps, t.M, t.N, t.Kc, t.K0, t.H, t.W) == (BF16, 9, 4 * 96 * 96, 768, 768, 768, 96, 96))
    assert hp.tile_accepted(t) == 1
    assert hp.tile_accepted(t._replace(algo=algo, bm=256)) == 0
    pr, ops = hp.tile_problem(t._replace(algo=algo, bm=256)), _lib.K22IgemmOperands()
    assert L.k22_igemm_cfg(C.byref(pr), C.byref(ops), None, None) == -1 and b"does not generate" in L.k22_last_error()

    def state(name):
        path = str(tmp_path / name)
        assert L.k22_tile_table_save(path.encode()) > 0
        key = [str(int(v)) for v in (t.dtype, t.taps, t.M, t.N, t.Kc, t.K0, t.H, t.W)]
        lines = [ln for ln in hp.tile_table_text_lines(path) if ln.split()[:8] == key]
        fixed = _lib.K22IgemmCfg()
        auto = hp.tile_problem(t._replace(algo=0, bm=0, bn=0, splitk=0, stages=0))
        assert L.k22_igemm_candidates(C.byref(auto), None, 0, None, C.byref(fixed)) > 0
        return lines, (fixed.algo, fixed.bm, fixed.bn, fixed.splitk, fixed.stages)

    before = state("before.txt")
    assert len(before[0]) >= 1 and before[1][0] != 0
    try:
        assert L.k22_set_option(b"conv_algo", algo) == 0
        during = state("during.txt")                    # the option reads as "auto": the fixed choice does not move
        assert L.k22_set_option(b"conv_algo", 0) == 0
        assert during == before and state("after.txt") == before
        assert hp.tile_accepted(t) == 1
    finally:
        L.k22_set_option(b"conv_algo", 0)


def test_launch_entry_refuses_what_the_acceptance_entry_rejects():
    """k22_igemm_cfg checks the configuration and the operands on the host before it touches the device: a configuration this build does
    not generate is an error, never a quiet run of another kernel"""
    import ctypes as C
    L = _lib.lib()
    t = next(t for t in hp.read_tile_table() if t.dtype == BF16 and t.taps == 9 and t.algo == 12 and t.splitk == 1)
    ops = _lib.K22IgemmOperands()                                       # all null
    rpi = C.c_int(7)
    pr = hp.tile_problem(t._replace(bm=192))
    assert L.k22_igemm_cfg(C.byref(pr), C.byref(ops), C.byref(rpi), None) == -1 and rpi.value == 0
    assert b"does not generate" in L.k22_last_error()
    pr = hp.tile_problem(t)
    assert L.k22_igemm_cfg(C.byref(pr), C.byref(ops), C.byref(rpi), None) == -1 and b"required" in L.k22_last_error()
    assert L.k22_igemm_cfg(C.byref(pr), None, None, None) == -1


def test_representative_selection_covers_every_class_and_every_line_is_swept_once():
    table = hp.read_tile_table()
    reps, rest = hp.tile_tiers(table)
    assert sorted(reps + rest) == sorted(table) and not set(reps) & set(rest)
    classes = {hp.tile_class(t) for t in table}
    assert {hp.tile_class(t) for t in reps} == classes
    for c in classes:
        ms = [t.M for t in table if hp.tile_class(t) == c]
        got = [t.M for t in reps if hp.tile_class(t) == c]
        assert max(got) == max(ms) and min(got) == min(ms) and len(got) <= 2
    assert len({hp.tile_id(t) for t in table}) == len(table)


# ---- 2. the float64 reference against torch ------------------------------------------------------------------------------------------

def torch_ref(t, s):
    """the same operation through F.conv2d / F.linear on the same (seen) operands, float64 [M][N]"""
    if t.taps == 9:
        B = t.M // (t.H * t.W)
        w4 = s["w"].view(t.N, 3, 3, t.Kc).permute(0, 3, 1, 2)
        y = F.conv2d(s["a0"].permute(0, 3, 1, 2), w4, s["bias"], padding=1).permute(0, 2, 3, 1).reshape(t.M, t.N)
    else:
        a = s["a0"] if s["a1"] is None else torch.cat([s["a0"], s["a1"]], 1)
        y = F.linear(a, s["w"], s["bias"])
    if s["residual"] is not None:
        y = y + s["residual"]
    if s["s0"] is not None:
        x = s["s0"] if s["s1"] is None else torch.cat([s["s0"], s["s1"]], 1)
        y = y + F.linear(x, s["ws"], s["bias2"])
    if t.act == _lib.ACT_SILU:
        y = F.silu(y)
    elif t.act == _lib.ACT_GELU:
        y = F.gelu(y)
    return y


REF_CASES = {
    "conv-bf16": line(),
    "conv-ragged-7x5-fp32": line(F32, H=7, W=5, B=3, N=40, Kc=32),
    "conv-skip-concat": line(F16, sk=192, N=128, Kc=128),
    "conv-skip-single": line(sk=64),
    "conv-nchw-f32": line(out_mode=2, N=8),
    "conv-silu": line(act=1),
    "gemm-concat": line(taps=1, Kc=192, K0=128, B=2),
    "gemm-f32-out-resf32-gelu": line(taps=1, out_mode=1, res_f32=1, act=2, H=0, W=0, M=77, N=96),
    "gemm-x3-chunks": line(X3, taps=1, Kc=128),
    "gemm-x3-raw": line(X3, taps=1, a_raw=1),
    "conv-x2-skip": line(X2, sk=192, N=128),
    "qkv": line(taps=1, out_mode=3, N=384, B=2, H=3, W=5),
}


@pytest.mark.parametrize("name", sorted(REF_CASES))
def test_reference_agrees_with_torch_float64(name):
    t = REF_CASES[name]
    inp = hp.igemm_inputs(t, CPU, seed=3)
    s = hp.igemm_seen(t, t.dtype, inp)
    pre, S = hp.igemm_pre64(t, s)
    want = torch_ref(t, s)
    got = hp.act64(pre, t.act)
    assert got.dtype == torch.float64 and (got - want).abs().max().item() <= 1e-12 * S.max().item()
    assert (S >= pre.abs() - 1e-12).all() and (S > 0).all()
    ref, bound = hp.igemm_ref(t, t.dtype, inp)
    if t.out_mode == 2:
        B = t.M // (t.H * t.W)
        assert torch.equal(ref["out"], got.view(B, t.H, t.W, t.N).permute(0, 3, 1, 2))
    elif t.out_mode == 3:
        C_, T_, B = t.N // 3, t.H * t.W, t.M // (t.H * t.W)
        Tkp = (hp.ATT_S + T_ + 63) // 64 * 64
        assert ref["kall"].shape == (B, C_ // 64, Tkp, 64) and ref["vtall"].shape == (B, C_ // 64, 64, Tkp)
        assert torch.equal(ref["out"], got[:, :C_])
        for b in range(B):
            for tok in (0, T_ - 1):
                m = b * T_ + tok
                for head in range(C_ // 64):
                    assert torch.equal(ref["kall"][b, head, hp.ATT_S + tok], got[m, C_ + 64 * head: C_ + 64 * head + 64])
                    assert torch.equal(ref["vtall"][b, head, :, hp.ATT_S + tok], got[m, 2 * C_ + 64 * head: 2 * C_ + 64 * head + 64])
        owned = torch.zeros(Tkp, dtype=torch.bool)
        owned[hp.ATT_S:hp.ATT_S + T_] = True
        assert torch.isnan(ref["kall"][:, :, ~owned]).all() and not torch.isnan(ref["kall"][:, :, owned]).any()
        assert torch.isnan(ref["vtall"][:, :, :, ~owned]).all() and (bound["vtall"][:, :, :, ~owned] == 0).all()
    else:
        assert torch.equal(ref["out"], got)


def test_seen_operands_are_what_each_arithmetic_promises():
    t = line(X3, sk=64)
    inp = hp.igemm_inputs(t, CPU, seed=1)
    s3, s2 = hp.igemm_seen(t, X3, inp), hp.igemm_seen(t, X2, inp)
    a = inp["a0"].double()
    assert ((s3["a0"] - a).abs() <= (a.abs() * 2.0 ** -22).clamp_min(2.0 ** -24)).all() and not torch.equal(s3["a0"], inp["a0"].half().double())
    assert torch.equal(s2["a0"], inp["a0"].half().double())                      # x2: the activation at fp16 ...
    assert torch.equal(s2["s0"], s3["s0"]) and torch.equal(s2["w"], s3["w"])      # ... the skip operands and the weights at full split
    assert ((s3["w"] - inp["w"].double()).abs() <= inp["w"].double().abs() * 2.0 ** -21 + 2.0 ** -32).all()
    sb = hp.igemm_seen(line(), BF16, inp)
    assert torch.equal(sb["a0"], inp["a0"].bfloat16().double()) and torch.equal(sb["residual"], inp["residual"].bfloat16().double())
    assert torch.equal(hp.igemm_seen(line(res_f32=1), BF16, inp)["residual"], inp["residual"].double())


def test_groupnorm_partial_sum_check():
    t = line(B=2, H=8, W=8, N=64, stats=1)
    g = torch.Generator().manual_seed(5)
    stored = (0.4 + torch.randn(t.M, t.N, generator=g)).bfloat16()
    rpi = 4
    rows = torch.full((2 * rpi + 3, t.N, 2), float("nan"))
    v = stored.float().view(2, rpi, 16, t.N)
    rows[: 2 * rpi, :, 0] = v.sum(2).view(2 * rpi, t.N)
    rows[: 2 * rpi, :, 1] = (v * v).sum(2).view(2 * rpi, t.N)
    assert hp.stats_violations(rows, stored, t, rpi) == 0
    bad = rows.clone(); bad[3, 7, 0] += 16 * stored.float()[:, 7].abs().sum() * 2.0 ** -24
    assert hp.stats_violations(bad, stored, t, rpi) == 1
    bad = rows.clone(); bad[5, 9, 1] *= 1 + 2.0 ** -16
    assert hp.stats_violations(bad, stored, t, rpi) == 1
    bad = rows.clone(); bad[2 * rpi, 0, 0] = 0.0                                  # a row beyond B * rows_per_image was written
    assert hp.stats_violations(bad, stored, t, rpi) == 1
    unrounded = stored.float() * (1 + 2.0 ** -10)                                 # sums of the values BEFORE the output rounding
    assert hp.stats_violations(rows, unrounded, t, rpi) > 0


# ---- 3. the comparator has teeth ------------------------------------------------------------------------------------------------------

def im2col(xp, t):
    """zero-bordered NHWC [B][H+2][W+2][Kc] -> [M][9 * Kc], k = tap * Kc + c"""
    return torch.cat([xp[:, ky:ky + t.H, kx:kx + t.W, :].reshape(t.M, t.Kc) for ky in range(3) for kx in range(3)], 1)


def trunc_to(x32, T):
    """fp32 -> T by truncation (toward zero) instead of round-to-nearest"""
    if T == torch.float32:
        return x32
    if T == torch.bfloat16:
        return (x32.view(torch.int32) & -65536).view(torch.float32).to(T)
    r = x32.to(T)                                            # fp16: where rne went away from zero, step one code back (sign-magnitude)
    return torch.where(r.float().abs() > x32.abs(), (r.view(torch.int16) - 1).view(T), r)


def emulate(t, dtype, inp, wrong=None):
    """a correct kernel on the CPU: operands as the arithmetic sees them, torch fp32 matmul, bias + residual in fp32, ONE rounding to the
    stored type.  `wrong` plants one defect."""
    s = hp.igemm_seen(t, dtype, inp)
    if wrong == "no_lo_weights":
        s["w"] = (inp["w"] * 256.0).half().double() / 256.0
    xp = F.pad(s["a0"].float(), (0, 0, 1, 1, 1, 1))
    if wrong == "wrapped_border":
        xp[:, 2:t.H + 1, 0, :] = xp[:, 1:t.H, t.W, :]        # x = -1 of image row y reads the last pixel of row y - 1 (the flat neighbour)
    A = im2col(xp, t)
    if wrong == "dropped_k":
        A[64:96, 5 * t.Kc + 17] = 0.0
    if wrong == "taps_swapped":
        a3, a5 = A[32:64, 3 * t.Kc:4 * t.Kc].clone(), A[32:64, 5 * t.Kc:6 * t.Kc].clone()
        A[32:64, 3 * t.Kc:4 * t.Kc], A[32:64, 5 * t.Kc:6 * t.Kc] = a5, a3
    bias = inp["bias"].clone()
    if wrong == "bias_missing":
        bias[-8:] = 0.0
    acc = A @ s["w"].float().T + bias + s["residual"].float()
    T = hp.storage_T(dtype)
    return trunc_to(acc, T) if wrong == "truncated" else acc.to(T)


def verdict(t, dtype, inp, out):
    ref, bound = hp.igemm_ref(t, dtype, inp)
    return hp.igemm_violations(out, ref["out"], bound["out"])


TEETH = [(dt, Kc) for dt in (BF16, F16, F32) for Kc in (128, 1536)]      # K = 9 * Kc = 1152 and 13824


@pytest.fixture(scope="module")
def teeth_inputs():
    return {Kc: hp.igemm_inputs(line(Kc=Kc, H=16, W=16, N=256), CPU, seed=11) for Kc in (128, 1536)}


@pytest.mark.parametrize("dtype,Kc", TEETH)
def test_comparator_passes_a_correct_kernel(dtype, Kc, teeth_inputs):
    t = line(dtype, Kc=Kc, H=16, W=16, N=256)
    bad, ratio = verdict(t, dtype, teeth_inputs[Kc], emulate(t, dtype, teeth_inputs[Kc]))
    print(f"correct {hp.DT_NAME[dtype]} kernel, K = {9 * Kc}: worst |out - ref| / bound = {ratio:.3f}")
    assert bad == 0 and ratio < 1.0


# (truncation of the output is a defect of the 16-bit engines only: an fp32 engine stores its fp32 accumulator as it is)
WRONG = [(w, dt, Kc) for w in ("dropped_k", "taps_swapped", "bias_missing", "wrapped_border", "truncated") for dt, Kc in TEETH
         if not (w == "truncated" and dt == F32)]


@pytest.mark.parametrize("wrong,dtype,Kc", WRONG)
def test_comparator_fails_a_subtly_wrong_kernel(wrong, dtype, Kc, teeth_inputs):
    t = line(dtype, Kc=Kc, H=16, W=16, N=256)
    bad, ratio = verdict(t, dtype, teeth_inputs[Kc], emulate(t, dtype, teeth_inputs[Kc], wrong))
    print(f"{wrong} {hp.DT_NAME[dtype]} K = {9 * Kc}: {bad} elements outside their bound, worst ratio {ratio:.2f}")
    assert bad > 0


@pytest.mark.parametrize("Kc", [128, 1536])
def test_comparator_fails_an_x3_product_without_the_low_weight_half(Kc, teeth_inputs):
    t = line(X3, Kc=Kc, H=16, W=16, N=256)
    inp = teeth_inputs[Kc]
    bad, ratio = verdict(t, X3, inp, emulate(t, X3, inp))
    assert bad == 0 and ratio < 1.0
    bad, ratio = verdict(t, X3, inp, emulate(t, X3, inp, "no_lo_weights"))
    print(f"x3 without w_lo, K = {9 * Kc}: {bad} of {t.M * t.N} outside, worst ratio {ratio:.2f}")
    assert bad > 0


def test_the_older_metric_does_not_notice_a_dropped_k_element_at_k_13824():
    """the reason the element-wise comparator exists: max-abs against 1.2e-2 * max|ref| (tests/test_kernels_gpu.py) with an fp32 reference
    passes a bf16 kernel that drops one K element on 32 rows of the 1536 -> 1536 level's product; the bound flags thousands of the 8192
    outputs of those rows"""
    t = line(BF16, Kc=1536, H=16, W=16, N=256)
    inp = hp.igemm_inputs(t, CPU, seed=11)
    out = emulate(t, BF16, inp, "dropped_k")
    s = hp.igemm_seen(t, BF16, inp)
    ref32 = hp.igemm_pre64(t, {k: (None if v is None else v.float()) for k, v in s.items()})[0]
    assert (out.float() - ref32).abs().max().item() <= 1.2e-2 * ref32.abs().max().item()          # old metric: passes
    ref, bound = hp.igemm_ref(t, BF16, inp)
    outside = ~((out.double() - ref["out"]).abs() <= bound["out"])
    assert not outside[:64].any() and not outside[96:].any()
    n = int(outside[64:96].sum())
    print(f"dropped K element, K = 13824, bf16: {n} of {32 * t.N} affected outputs outside their bound")
    assert n >= 1000


# ---- 4. where IGEMM_C comes from ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [BF16, F16, F32])
@pytest.mark.parametrize("K", [128, 1152, 6912, 13824])
def test_plain_fp32_evaluations_behind_c(dtype, K):
    """The two plain evaluations IGEMM_C is derived from (helpers.py), against float64 in units of 2^-24 * S.  The 16-wide sequential chain
    is IEEE arithmetic in a fixed order - the same figure on every machine - and stays under 2; torch's fp32 matmul depends on the host
    BLAS and must pass the bound (ratio < c).  The matmul that decided c is the MI355X's (tests/test_tile_table_gpu.py)."""
    t = line(dtype, taps=1, Kc=K, H=0, W=0, M=256, N=256)
    inp = hp.igemm_inputs(t, CPU, seed=K)
    r_mm, r_chain = hp.plain_fp32_ratio(t, dtype, inp), hp.plain_fp32_ratio(t, dtype, inp, chain16=True)
    print(f"{hp.DT_NAME[dtype]} K = {K}: torch fp32 matmul {r_mm:.3f}, 16-wide chain {r_chain:.3f}  (x 2^-24 x S)")
    assert r_chain < 2 and r_mm < hp.IGEMM_C


@pytest.mark.parametrize("act", [_lib.ACT_SILU, _lib.ACT_GELU])
def test_activation_term_is_a_few_fp32_ulps(act):
    x = torch.linspace(-12, 12, 100001, dtype=torch.float64)
    e = hp.act_eval_term(x, act)
    assert 0 < e <= 4 * 12 * 2.0 ** -23
    slope = ((hp.act64(x[1:], act) - hp.act64(x[:-1], act)) / (x[1:] - x[:-1])).abs().max().item()
    assert slope <= hp.IGEMM_L_ACT
