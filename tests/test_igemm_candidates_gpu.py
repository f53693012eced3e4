"""Every configuration the tuner may time, and the fixed choice, at the off-table problems of helpers.OFFTABLE - element by element.

For a shape the shipped tile table does not hold, tune_igemm_ops times each entry of tuned_make_candidates' list and keeps the fastest
without looking at what it computed; K22_AUTOTUNE=0, and every M < 64, runs tuned_default_cfg's fixed choice.  One test item per (problem,
arithmetic): seeded operands (seed from the item id), the float64 reference and bound of helpers.py computed ONCE, then every candidate the
build itself lists (k22_igemm_candidates; for the 16-bit types with and without the fragment-major weight copy, so that the streaming
kernel's are among them) plus the all-zero configuration, each launched through k22_igemm_cfg into NaN-filled outputs, K_all / V^T_all and
GroupNorm-sum rows.  Per configuration: every element within its bound, what the launch does not own still NaN, the partial sums within
theirs, and a second launch equal in bits.  All failing configurations of an item are reported together (configuration, worst ratio,
count).  tests/test_igemm_candidates_cpu.py asserts that the list reaches every class of candidate the generator can emit.

Measured on the MI355X: 145 (problem, arithmetic) items, 3450 configurations enumerated and run (bf16 624, fp16 624, fp32 960, x3 621, x2 621;
145 of them the fixed choice), 6900 launches, the whole file in 3.5 s (largest item 0.05 s after the first one's 0.9 s of start-up) - no item
had to be split.  No configuration failed.  Worst |out - ref| / bound: bf16 0.995, fp16 0.993 (the output rounding itself), fp32 0.33,
x3 0.044, x2 0.039.  The last test prints these totals and where the worst ratio occurred.
"""
import zlib

import pytest
import torch

import helpers as hp
from kandinsky2_amd import _lib

pytestmark = pytest.mark.gpu
BF16, F16 = _lib.K22_BF16, _lib.K22_F16

CASES = hp.offtable_cases()
TOTALS = {"items": 0, "enumerated": 0, "run": 0, "launches": 0, "failed": 0, "worst": 0.0, "worst_at": "", "measured_before": None}


def _bits(x):
    return x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32)


def _configurations(t, dtype):
    """the build's list for the problem, each configuration once, + the all-zero fixed choice (last)"""
    seen, out = set(), []
    for frag in ((0, 1) if dtype in (BF16, F16) else (0,)):
        for c in hp.igemm_candidates(t, dtype, frag)[0]:
            if c not in seen:
                seen.add(c)
                out.append(c)
    return out + [(0, 0, 0, 0, 0)]


@pytest.mark.parametrize("name,t,dtype", CASES, ids=[c[0] for c in CASES])
def test_every_candidate_of_an_off_table_problem(name, t, dtype):
    if TOTALS["measured_before"] is None:
        TOTALS["measured_before"] = _lib.lib().k22_tile_table_measured()
    cfgs = _configurations(t, dtype)
    TOTALS["items"] += 1
    TOTALS["enumerated"] += len(cfgs)
    assert t.M >= 64 or len(cfgs) >= 1
    inp = hp.igemm_inputs(t, "cuda", seed=zlib.crc32(name.encode()) & 0xFFFF)
    ref, bound = hp.igemm_ref(t, dtype, inp)
    failures, item_worst = [], 0.0
    for c in cfgs:
        line = t._replace(**dict(zip(hp.CFG_FIELDS, c)))
        TOTALS["run"] += 1
        try:
            outs, sbuf, rpi = hp.run_tile_line(line, dtype, inp)
        except RuntimeError as e:
            # a refusal on the host (K22_EINVAL / K22_ENOMEM: nothing was launched) is this configuration's failure; anything else - a
            # failed launch, a device fault - ends the session: nothing more may run on a device that has faulted
            if not str(e).startswith(("k22 error -1:", "k22 error -3:")):
                pytest.exit(f"{name} cfg {c}: {e}", returncode=3)
            failures.append(f"  cfg (algo, bm, bn, splitk, stages) = {c}: refused: {e}")
            continue
        bad, worst = 0, 0.0
        for k in ref:
            b, r = hp.igemm_violations(outs[k], ref[k], bound[k])      # (counts NaN where a value is owed and values where none is)
            bad, worst = bad + b, max(worst, r)
        bad_stats = 0
        if t.stats:
            bad_stats = hp.stats_violations(sbuf, outs["out"], t, rpi) if rpi > 0 else -1
        try:
            outs2, sbuf2, rpi2 = hp.run_tile_line(line, dtype, inp)
        except RuntimeError as e:
            pytest.exit(f"{name} cfg {c}, second launch: {e}", returncode=3)
        TOTALS["launches"] += 2
        same = rpi2 == rpi and all(torch.equal(_bits(outs[k]), _bits(outs2[k])) for k in outs) and \
            (sbuf is None or torch.equal(_bits(sbuf), _bits(sbuf2)))
        item_worst = max(item_worst, worst)
        if worst > TOTALS["worst"]:
            TOTALS["worst"], TOTALS["worst_at"] = worst, f"{name} {c}"
        if bad or bad_stats or not same:
            failures.append(f"  cfg (algo, bm, bn, splitk, stages) = {c}: worst |out - ref| / bound {worst:.3f}, {bad} elements outside"
                            + (f", {bad_stats} partial sums outside (rows/image {rpi})" if t.stats else "")
                            + ("" if same else ", two launches differ in bits"))
    print(f"{name}: {len(cfgs) - 1} candidates + the fixed choice {hp.igemm_candidates(t, dtype)[2]}, worst |out - ref| / bound {item_worst:.3f}, "
          f"{len(failures)} failing")
    TOTALS["failed"] += len(failures)
    assert not failures, f"{name}: {len(failures)} of {len(cfgs)} configurations fail:\n" + "\n".join(failures)


def test_zz_every_enumerated_candidate_was_run(request):
    """runs last in this file: candidates enumerated == candidates run, none left out, nothing measured into the process's tile table"""
    selected = [it for it in request.session.items if it.originalname == "test_every_candidate_of_an_off_table_problem"]
    print(f"candidate sweep: {TOTALS['items']} (problem, arithmetic) items, {TOTALS['enumerated']} configurations enumerated, {TOTALS['run']} run "
          f"({TOTALS['launches']} launches), {TOTALS['failed']} failing; worst |out - ref| / bound {TOTALS['worst']:.3f} at {TOTALS['worst_at']}")
    assert TOTALS["items"] == len(selected)
    assert TOTALS["run"] == TOTALS["enumerated"] and TOTALS["failed"] == 0
    if len(selected) == len(CASES):
        assert TOTALS["enumerated"] == sum(len(_configurations(t, dt)) for _, t, dt in CASES) > len(CASES)
    if TOTALS["measured_before"] is not None:
        assert _lib.lib().k22_tile_table_measured() == TOTALS["measured_before"]
