"""Host-side half of the candidate sweep (tests/test_igemm_candidates_gpu.py runs the candidates on the device).

Off the shipped tile table - any batch or image size other than the C1-C5 configs' - tune_igemm_ops times every configuration
tuned_make_candidates generates and keeps the fastest without looking at what it computed; with K22_AUTOTUNE=0, and for every M < 64, the
problem runs tuned_default_cfg's fixed choice.  helpers.OFFTABLE lists the smallest problems at which the edges of those kernels' index
arithmetic exist.  Here, without a device:

  * k22_igemm_candidates (the build's own list) agrees with k22_igemm_cfg_accepted over a grid of every value tuned_make_candidates writes;
  * the union of the lists over OFFTABLE hits every class of configuration the generator can emit - asserted, and printed per class with
    the number of candidates and whether the shipped table has a line of the class;
  * the float64 reference agrees with F.conv2d / F.linear at the H = 1, W = 1 and N = 136 problems;
  * the comparator passes the CPU emulation of a correct kernel at these shapes and fails three defects of the kind they exist for;
  * a plain fp32 evaluation stays below IGEMM_C on every (problem, arithmetic) pair, so the bound's constant holds here unchanged.
"""
import collections
import itertools

import pytest
import torch

import helpers as hp
import test_tile_table_cpu as tt
from kandinsky2_amd import _lib

BF16, F32, F16, X3, X2 = _lib.K22_BF16, _lib.K22_F32, _lib.K22_F16, _lib.K22_F16X3, _lib.K22_F16X2
CPU = torch.device("cpu")
CASES = hp.offtable_cases()
HALO_ALGOS = (2, 7, 6, 3, 11, 12)
HALO_KERNEL = {2: "halo", 7: "halo", 6: "halo", 3: "halo3", 11: "spec", 12: "spec"}   # the three kernels behind the six algos


def union_candidates(t, dtype):
    """candidates of the problem with and without the fragment-major weight copy (16-bit types: the streaming kernel's condition), in order,
    each once -> [(configuration, resolved launch)], fixed choice"""
    seen, out = set(), []
    for frag in ((0, 1) if dtype in (BF16, F16) else (0,)):
        cands, res, fixed = hp.igemm_candidates(t, dtype, frag)
        for c, r in zip(cands, res):
            if c not in seen:
                seen.add(c)
                out.append((c, r))
    return out, fixed


# ---- 1. the enumerator against the acceptance entry -------------------------------------------------------------------------------------------

# every value tuned_make_candidates (csrc/tuning.h) writes into a field, whatever the family
GRID = dict(algo=(1, 2, 7, 6, 3, 11, 12, 10, 20), bm=(256, 128, 64, 160, 288), bn=(0, 128, 64),
            splitk=(1, 2, 3, 4, 5, 6, 8, 10, 12, 16), stages=(0, 2, 3, 4))


def stages_wildcard(c):
    """tuned_is_candidate ignores `stages` for the halo kernels and the streaming kernel"""
    return c[:4] + (0,) if (c[0] >= 2 and c[0] != 10) else c


@pytest.mark.parametrize("name,t,dtype", CASES, ids=[c[0] for c in CASES])
def test_enumerator_agrees_with_the_acceptance_entry(name, t, dtype):
    listed, fixed = union_candidates(t, dtype)
    cfgs = [c for c, _ in listed]
    assert len(set(cfgs)) == len(cfgs)
    for c in cfgs:
        assert hp.tile_accepted(t._replace(**dict(zip(hp.CFG_FIELDS, c))), dtype) == 1, (name, c)
    grid = set()
    for c in itertools.product(*(GRID[f] for f in hp.CFG_FIELDS)):
        if hp.tile_accepted(t._replace(**dict(zip(hp.CFG_FIELDS, c))), dtype) == 1:
            grid.add(stages_wildcard(c))
    assert grid == {stages_wildcard(c) for c in cfgs}, name
    # the all-zero configuration is the fixed choice: accepted, and resolved to a real kernel
    assert hp.tile_accepted(t, dtype) == 1 and fixed[0] != 0 and fixed[3] >= 1
    if t.M < 64:
        print(f"{name}: M = {t.M} < 64 is never timed; fixed choice algo {fixed[0]} {fixed[1]}x{fixed[2]} split-K {fixed[3]} depth {fixed[4]}")


def test_enumerator_entry_checks_its_arguments():
    import ctypes as C
    L = _lib.lib()
    t = hp.OFFTABLE["conv-2x10x10-192-192"]
    pr = hp.tile_problem(t, BF16)
    n = L.k22_igemm_candidates(C.byref(pr), None, 0, None, None)                      # count only
    assert n == len(hp.igemm_candidates(t, BF16)[0]) > 0
    few = (_lib.K22IgemmCfg * 3)()
    assert L.k22_igemm_candidates(C.byref(pr), few, 3, None, None) == n                # a short array is filled, the full number returned
    assert tuple(getattr(few[2], f) for f in hp.CFG_FIELDS) == hp.igemm_candidates(t, BF16)[0][2]
    assert L.k22_igemm_candidates(None, None, 0, None, None) == -1 and L.k22_igemm_candidates(C.byref(pr), None, 3, None, None) == -1
    pr.taps = 5
    assert L.k22_igemm_candidates(C.byref(pr), None, 0, None, None) == -1
    # a problem that owes GroupNorm sums no configuration can write (N < 128: the generic kernel, 35 rows per image: no row-tiled finish)
    bad = hp.OFFTABLE["conv-3x5x7-128-256-st"]._replace(N=8)
    assert hp.igemm_candidates(bad, BF16)[0] == [] and hp.tile_accepted(bad, BF16) == 0
    ops = _lib.K22IgemmOperands()
    rpi = C.c_int(7)
    pr = hp.tile_problem(bad, BF16)
    assert L.k22_igemm_cfg(C.byref(pr), C.byref(ops), C.byref(rpi), None) == -1 and b"fixed choice" in L.k22_last_error() and rpi.value == 0


# ---- 2. every class the generator can emit is reached by some problem of the list --------------------------------------------------------------

def classes_of(c, r):
    """the classes one candidate belongs to: (family, ...) tuples; c as generated, r as resolved (r[4] = ring depth instantiated)"""
    algo, bm, bn, sk, stg = c
    if algo in HALO_ALGOS:
        return [("halo", algo, bm, "split" if sk > 1 else "whole"), ("ring", HALO_KERNEL[algo], bm, r[4])]
    if algo == 10:
        return [("gemm8", bm, stg), ("gemm8-splitk", sk)]
    if algo == 20:
        return [("stream", bm)]
    assert algo == 1
    return [("generic", bm, bn, stg), ("generic-splitk", sk)]


def reachable_rings():
    """every (kernel, bm, depth) conv3_halo_ring returns for SOME width, read from the build: one-row problems of every W up to 400 (past
    the widest image any halo kernel takes), each with and without a fused skip (its ring shares the LDS budget)"""
    out = set()
    for W in range(1, 401):
        for sk in (0, 64):
            t = hp.OFFTABLE["conv-1x2x160-64-128"]._replace(H=1, W=W, M=W, sk_total=sk)
            cands, res, _ = hp.igemm_candidates(t, BF16)
            out |= {cl for c, r in zip(cands, res) for cl in classes_of(c, r) if cl[0] == "ring"}
    return out


# Both are split-K factors of families whose every tile and ring IS reached; the factor changes the k-range of a workgroup, nothing else.
UNREACHABLE = {
    ("gemm8-splitk", 6): "needs 24 k-steps (K >= 1536 in the 16-bit types, 768 in the others); the list's longest GEMM has 18.  Table lines cover it.",
    ("generic-splitk", 16): "needs 64 k-steps (a 3x3 convolution of 512 / 256 channels); the list's longest problem has 54.  Table lines cover it.",
}


def test_the_problem_list_reaches_every_class_of_candidate():
    hit = collections.Counter()
    for name, t, dtype in CASES:
        for c, r in union_candidates(t, dtype)[0]:
            for cl in classes_of(c, r):
                hit[cl] += 1
    table = set()
    for ln in hp.read_tile_table():
        table |= {cl for cl in classes_of(hp.cfg_of(ln), hp.cfg_of(ln)) if cl[0] != "ring"}
    want = {("halo", a, bm, s) for a in HALO_ALGOS for bm in (256, 128) for s in ("whole", "split")}
    want |= {("gemm8", bm, stg) for bm, stg in ((256, 0), (256, 3), (128, 0), (128, 2), (128, 3), (128, 4))}
    want |= {("gemm8-splitk", sk) for sk in (1, 2, 3, 4, 6)}
    want |= {("stream", 160), ("stream", 288)}
    want |= {("generic", bm, bn, stg) for bm, bn in ((128, 128), (128, 64), (64, 64)) for stg in (2, 3, 4)}
    want |= {("generic-splitk", sk) for sk in (1, 2, 4, 8, 16)}
    rings = reachable_rings()
    assert {(k, bm) for _, k, bm, _ in rings} == {(k, bm) for k in ("halo", "halo3", "spec") for bm in (256, 128)}
    want |= rings
    # classes no small shape reaches, each with its reason - never dropped silently
    unreachable = dict(UNREACHABLE)
    for cl in sorted(want | set(hit), key=str):
        print(f"{str(cl):36s} candidates {hit[cl]:5d}   table line: {'yes' if cl in table else ('-' if cl[0] == 'ring' else 'NO')}"
              + (f"   NOT REACHED: {unreachable[cl]}" if cl in unreachable else ""))
    assert set(unreachable) <= want and not (set(unreachable) & set(hit)), "a class listed as unreachable is reached: take it off the list"
    assert set(unreachable) <= table, "a class no problem reaches must at least be swept by tests/test_tile_table_gpu.py"
    missing = want - set(hit) - set(unreachable)
    assert not missing, f"classes of candidate no problem of helpers.OFFTABLE reaches: {sorted(missing, key=str)}"
    assert set(hit) <= want, f"the generator emits a class this test does not know: {sorted(set(hit) - want, key=str)}"


# ---- 3. the reference restates the operation ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["conv-2x1x37-64-128", "conv-2x37x1-64-128", "conv-1x20x20-128-136", "conv-2x10x10-128-128-skip192",
                                  "gemm-333x200x576", "gemm-150x256x320cat128-f32"])
@pytest.mark.parametrize("dtype", [BF16, X3], ids=["bf16", "x3"])
def test_reference_agrees_with_torch_float64_at_the_edges(name, dtype):
    t = hp.OFFTABLE[name]
    inp = hp.igemm_inputs(t, CPU, seed=5)
    s = hp.igemm_seen(t, dtype, inp)
    pre, S = hp.igemm_pre64(t, s)
    want = tt.torch_ref(t, s)
    assert pre.shape == (t.M, t.N) and (pre - want).abs().max().item() <= 1e-12 * S.max().item()
    assert (S >= pre.abs() - 1e-12).all() and (S > 0).all()


# ---- 4. the comparator at these shapes ------------------------------------------------------------------------------------------------------------

def emulate(t, dtype, inp, wrong=None):
    """a correct kernel on the CPU, as tests/test_tile_table_cpu.py's: operands as the arithmetic sees them, torch fp32 matmul, bias + residual
    in fp32, one rounding to the stored type; outputs start as NaN, as on the device.  `wrong` plants one defect."""
    s = hp.igemm_seen(t, dtype, inp)
    bk = 64 if dtype in (BF16, F16) else 32
    if t.taps == 9:
        A = tt.im2col(torch.nn.functional.pad(s["a0"].float(), (0, 0, 1, 1, 1, 1)), t)
        if wrong == "border_tap":
            # the tap above (ky = 0, kx = 1) is dropped on image row 1, as if row 0 were still border
            rows = torch.arange(t.M).view(-1, t.H, t.W)[:, 1].reshape(-1)
            A[rows, 1 * t.Kc:2 * t.Kc] = 0.0
    else:
        A = s["a0"].float()
    if wrong == "last_k_step":
        # the last k-step of a tap's K loop on one 32-row block: the centre tap's (at H = 1 or W = 1 the LAST tap reads the border only)
        end = 5 * t.Kc if t.taps == 9 else t.Kc
        A[:32, end - bk:end] = 0.0
    acc = A @ s["w"].float().T + inp["bias"] + s["residual"].float()
    out = torch.full((t.M, t.N), float("nan"), dtype=hp.storage_T(dtype))
    rows = t.M - 1 if wrong == "ragged_row" else t.M                # the last row of the ragged last tile is never stored
    out[:rows] = acc[:rows].to(out.dtype)
    return out


TEETH = [(n, dt) for n in ("conv-2x37x1-64-128", "conv-2x1x37-64-128", "conv-1x2x160-64-128", "conv-3x5x5-128-128", "conv-1x20x20-128-136",
                           "gemm-333x200x576", "gemm-65x128x64")
         for dt in (BF16, F16, F32, X3) if hp.offtable_accepts(hp.OFFTABLE[n], dt)]


@pytest.mark.parametrize("name,dtype", TEETH, ids=[f"{n}-{hp.DT_NAME[d]}" for n, d in TEETH])
def test_comparator_passes_a_correct_kernel_and_fails_three_defects(name, dtype):
    t = hp.OFFTABLE[name]
    inp = hp.igemm_inputs(t, CPU, seed=9)
    bad, ratio = tt.verdict(t, dtype, inp, emulate(t, dtype, inp))
    print(f"{name} {hp.DT_NAME[dtype]}: correct kernel, worst |out - ref| / bound {ratio:.3f}")
    assert bad == 0 and ratio < 1.0
    wrongs = ["last_k_step", "ragged_row"] + (["border_tap"] if t.taps == 9 and t.H > 1 else [])
    for wrong in wrongs:
        bad, ratio = tt.verdict(t, dtype, inp, emulate(t, dtype, inp, wrong))
        print(f"{name} {hp.DT_NAME[dtype]}: {wrong}: {bad} elements outside their bound, worst ratio {ratio:.2f}")
        assert bad > 0, wrong
    if name == "conv-2x37x1-64-128":
        assert "border_tap" in wrongs


# ---- 5. the bound's constant holds at these shapes --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,t,dtype", CASES, ids=[c[0] for c in CASES])
def test_plain_fp32_evaluation_stays_below_c(name, t, dtype):
    """IGEMM_C is twice the largest error of a PLAIN fp32 evaluation over the shipped table's shapes; a problem of this list whose plain
    evaluation came close to it would have to be replaced, never the constant"""
    inp = hp.igemm_inputs(t, CPU, seed=13)
    r = hp.plain_fp32_ratio(t, dtype, inp)
    print(f"{name}: torch fp32 matmul on the host {r:.3f} x 2^-24 x S  (IGEMM_C = {hp.IGEMM_C:.2f})")
    assert r < hp.IGEMM_C
