"""Every line of the SHIPPED tile table (kandinsky-2_amd/tiles_gfx950.txt), run at its own shape with its own configuration.

The table fixes kernel, tile, split-K factor and LDS-DMA depth of the conv / GEMM launches of the C1-C5 configs: it IS the hot path.  The
unit-parity files force a handful of configurations at toy shapes; this one is parametrised from the table the package ships, at
collection time, so a regenerated table is swept without touching the test.  Per line: seeded operands in the layout the key implies, ONE
launch through k22_igemm_cfg (the descriptor, tuned_apply_cfg and launch_igemm of the engines; no process-wide option), then every element
of every output against the float64 reference and the rounding-error bound of helpers.py (its header comment derives the bound and holds
the measured constants).  Output, K_all / V^T_all and GroupNorm-sum buffers start as NaN: what the launch does not own must still be NaN.

Two tiers of the one test:
  representatives (unmarked)  of every (dtype, taps, out-mode flags, stats, skip, algo, bm, bn, splitk, stages) class the line with the
                              largest M and the one with the smallest.  A bf16 representative also runs as K22_F16 (fp16 resolves
                              through the bf16 lines), an x3 one without an x2 line of its own also as K22_F16X2 (the fall-back of
                              tile_table_lookup).  They are launched twice and must give equal bits (split-K finishes and partial sums
                              are ordered sums), and torch's own fp32 matmul of the same product - the plain evaluation the bound's
                              constant c was derived from (twice its largest ratio) - must itself pass the bound;
  all remaining lines         pytest.mark.slow: they run by default, K22_RUN_SLOW=0 skips them.

Measured on the MI355X: 834 representative launches (570 lines + 263 fp16 / x2 duplicates, each run twice) 8 s, both tiers (2303 launches)
16 s - next to a GPU suite of 223 s on the same box without them (README: 8-9 min on a box with a slower host).  Far below the point where
lines would have to move between the tiers.

The last test prints how many lines were swept and checks that the sweep measured nothing into the process's tile table.
"""
import zlib

import pytest
import torch

import helpers as hp
from kandinsky2_amd import _lib

pytestmark = pytest.mark.gpu
BF16, F16, X3, X2 = _lib.K22_BF16, _lib.K22_F16, _lib.K22_F16X3, _lib.K22_F16X2

TABLE = hp.read_tile_table()
REPS, REST = hp.tile_tiers(TABLE)


def _cases():
    reps = set(REPS)
    own_x2 = {hp.tile_key(t) for t in TABLE if t.dtype == X2}
    out = []
    for t in TABLE:
        rep = t in reps
        out.append(pytest.param(t, t.dtype, rep, id=hp.tile_id(t), marks=() if rep else pytest.mark.slow))
        if rep and t.dtype == BF16:
            out.append(pytest.param(t, F16, rep, id=hp.tile_id(t, F16)))
        if rep and t.dtype == X3 and hp.tile_key(t) not in own_x2:
            out.append(pytest.param(t, X2, rep, id=hp.tile_id(t, X2)))
    return out


CASES = _cases()
SWEPT = {"run": 0, "passed": 0, "worst": 0.0, "worst_id": "", "plain": 0.0, "plain_id": "", "act": 0.0, "measured_before": None}


def _bits(x):
    return x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("t,dtype,rep", CASES)
def test_tile_table_line(t, dtype, rep, request):
    name = request.node.callspec.id
    if SWEPT["measured_before"] is None:
        SWEPT["measured_before"] = _lib.lib().k22_tile_table_measured()
    SWEPT["run"] += 1
    inp = hp.igemm_inputs(t, "cuda", seed=zlib.crc32(name.encode()) & 0xFFFF)
    outs, sbuf, rpi = hp.run_tile_line(t, dtype, inp)
    info = {}
    ref, bound = hp.igemm_ref(t, dtype, inp, info=info)
    bad, worst = {}, 0.0
    for k in ref:
        bad[k], r = hp.igemm_violations(outs[k], ref[k], bound[k])
        worst = max(worst, r)
    bad_stats = hp.stats_violations(sbuf, outs["out"], t, rpi) if t.stats else 0
    plain = hp.plain_fp32_ratio(t, dtype, inp) if rep else 0.0
    print(f"{name}: worst |out - ref| / bound {worst:.3f}, outside {bad}, stats rows/image {rpi} outside {bad_stats}"
          + (f", torch fp32 matmul / (2^-24 S) {plain:.3f}" if rep else "") + (f", activation term {info['e_act']:.3e}" if t.act else ""))
    if worst > SWEPT["worst"]:
        SWEPT["worst"], SWEPT["worst_id"] = worst, name
    if plain > SWEPT["plain"]:
        SWEPT["plain"], SWEPT["plain_id"] = plain, name
    assert not any(bad.values()), f"{name}: elements outside their bound {bad}, worst ratio {worst:.2f}"
    assert not t.stats or (rpi > 0 and bad_stats == 0), f"{name}: {bad_stats} GroupNorm partial sums outside c * 2^-24 * (sum|x|, sumsq)"
    if rep:
        assert plain < hp.IGEMM_C, f"{name}: a plain fp32 evaluation needs {plain:.2f} x 2^-24 x S - IGEMM_C must be re-derived"
        outs2, sbuf2, rpi2 = hp.run_tile_line(t, dtype, inp)
        assert rpi2 == rpi and all(torch.equal(_bits(outs[k]), _bits(outs2[k])) for k in outs), f"{name}: two launches differ in bits"
        assert sbuf is None or torch.equal(_bits(sbuf), _bits(sbuf2)), f"{name}: two launches differ in their partial sums"
    SWEPT["passed"] += 1


def test_zz_the_sweep_covered_what_was_selected_and_measured_nothing(request):
    """runs last in this file: the count of swept lines (table lines + the fp16 / x2 duplicates of the representatives), and the promise
    that a shipped line is never timed again - the sweep leaves k22_tile_table_measured() where it found it"""
    selected = [it for it in request.session.items if it.originalname == "test_tile_table_line"
                and not any(m.name == "skip" for m in it.iter_markers())]
    n_dup = len(CASES) - len(TABLE)
    print(f"tile table sweep: {SWEPT['run']} lines run, {SWEPT['passed']} passed; the table has {len(TABLE)} lines in {len(REPS)} representatives + "
          f"{len(REST)} others, + {n_dup} fp16 / x2 duplicates = {len(CASES)}; worst |out - ref| / bound {SWEPT['worst']:.3f} ({SWEPT['worst_id']}); "
          f"largest torch fp32 matmul error {SWEPT['plain']:.3f} x 2^-24 x S ({SWEPT['plain_id']})")
    assert len(CASES) == len(TABLE) + n_dup and len(REPS) + len(REST) == len(TABLE)
    assert SWEPT["run"] == len(selected)
    if SWEPT["measured_before"] is not None:
        assert _lib.lib().k22_tile_table_measured() == SWEPT["measured_before"]
