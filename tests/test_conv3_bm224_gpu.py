"""The 224-row tile of conv3_halo_spec_kernel (algo 12, bm 224: four consumer waves of one 32-column strip each, 7 m-blocks; three weight
slots beside the 424-row halo image of a 96-wide plane) against float64, element by element, at the smallest problems on which each of
its edges exists.  tests/test_conv3_bm224_cpu.py holds the host-side half (where the build generates the tile).

One test item per (problem, 16-bit type): seeded operands, the float64 reference and bound of helpers.py computed once, then every
bm = 224 configuration the build lists for the problem (k22_igemm_candidates: split-K 1 and whatever deeper split the rule admits), each
launched through k22_igemm_cfg into NaN-filled outputs and GroupNorm-sum rows.  Per configuration: every element within its bound, what
the launch does not own still NaN, the partial sums within theirs at H * (W + 2) / 224 rows per image, a second launch equal in bits -
and at split-K 1 the output equal IN BITS to the bm = 256 configuration's on the same operands (same MFMA, same order of slabs, taps and
k-steps per element; asserted wherever the existing 256- and 128-row forms agree with each other in bits, which the test checks first).

                       B x H x W   Kc   N   extras            what it exercises
  plane-2x14x14         2 x 14 x 14   64  128  -                 one tile = the whole plane, both borders in one tile, one slab
  two-tiles-1x28x14     1 x 28 x 14  192  192  stats, residual   two tiles; three slabs: the halo buffers swap; a half-empty n-tile
  two-tiles-...-split   the same without the sums owed: the deeper splits are listed (uneven split-K 2 of three slabs)
  odd-batch-3x8x26      3 x 8 x 26   128  128  -                 odd batch
  row96-1x16x96         1 x 16 x 96  128  128  stats             the real row width: seven tiles whose edges fall mid-row, the 157696-byte
                                                                 LDS budget with three weight slots
  skip64 / skip192      2 x 14 x 14  128  128  fused 1x1 skip    narrow and concat skip: the rounded-up input-tile slot of the skip ring
  row96-skip192         1 x 16 x 96  128  128  fused skip        the same at the real row width

The second test sweeps the lines that ship with the tile (kandinsky-2_amd/tiles_gfx950_bm224.txt, loaded behind the shipped table) at
their own full shapes, as tests/test_tile_table_gpu.py sweeps the shipped table: as bf16 and as fp16, launched twice.
"""
import zlib

import pytest
import torch

import helpers as hp
from kandinsky2_amd import _lib

pytestmark = pytest.mark.gpu
BF16, F16 = _lib.K22_BF16, _lib.K22_F16
ALGO_PIPE, BM = 12, 224

PROBLEMS = {
    "plane-2x14x14": hp._ot_conv(2, 14, 14, 64, 128),
    "two-tiles-1x28x14-st": hp._ot_conv(1, 28, 14, 192, 192, stats=1),
    "two-tiles-1x28x14-split": hp._ot_conv(1, 28, 14, 192, 192),
    "odd-batch-3x8x26": hp._ot_conv(3, 8, 26, 128, 128),
    "row96-1x16x96-st": hp._ot_conv(1, 16, 96, 128, 128, stats=1),
    "skip64-2x14x14": hp._ot_conv(2, 14, 14, 128, 128, sk=64),
    "skip192-2x14x14": hp._ot_conv(2, 14, 14, 128, 128, sk=192),
    "row96-skip192-1x16x96": hp._ot_conv(1, 16, 96, 128, 128, sk=192),
}
CASES = [(f"{name}-{hp.DT_NAME[dt]}", t, dt) for name, t in PROBLEMS.items() for dt in (BF16, F16)]


def _bits(x):
    return x.contiguous().view(torch.int16)


def _run(name, line, dtype, inp):
    """a refusal on the host is an assertion failure; anything else - a failed launch, a device fault - ends the session: nothing more may
    run on a device that has faulted"""
    try:
        return hp.run_tile_line(line, dtype, inp)
    except RuntimeError as e:
        if not str(e).startswith(("k22 error -1:", "k22 error -3:")):
            pytest.exit(f"{name} cfg {hp.cfg_of(line)}: {e}", returncode=3)
        raise


@pytest.mark.parametrize("name,t,dtype", CASES, ids=[c[0] for c in CASES])
def test_every_224_row_configuration_of_the_problem(name, t, dtype):
    B, tiles = t.M // (t.H * t.W), t.H * (t.W + 2) // BM
    assert t.H * (t.W + 2) == tiles * BM
    cfgs = [c for c in hp.igemm_candidates(t, dtype)[0] if c[1] == BM]
    assert (ALGO_PIPE, BM, 0, 1, 0) in cfgs and all(c[0] == ALGO_PIPE for c in cfgs)
    if name.startswith("two-tiles-1x28x14-split"):
        assert (ALGO_PIPE, BM, 0, 2, 0) in cfgs                                    # three slabs in two uneven parts
    inp = hp.igemm_inputs(t, "cuda", seed=zlib.crc32(name.encode()) & 0xFFFF)
    ref, bound = hp.igemm_ref(t, dtype, inp)
    # the yardstick of the bit comparison: do the two existing tiles of the same kernel agree with each other?
    o256 = _run(name, t._replace(algo=ALGO_PIPE, bm=256, splitk=1), dtype, inp)[0]["out"]
    o128 = _run(name, t._replace(algo=ALGO_PIPE, bm=128, splitk=1), dtype, inp)[0]["out"]
    tiles_agree = torch.equal(_bits(o256), _bits(o128))
    failures = []
    for c in cfgs:
        line = t._replace(**dict(zip(hp.CFG_FIELDS, c)))
        outs, sbuf, rpi = _run(name, line, dtype, inp)
        bad, worst = hp.igemm_violations(outs["out"], ref["out"], bound["out"])    # (counts NaN where a value is owed and values where none is)
        bad_stats = 0
        if t.stats:
            want_rpi = tiles if c[3] == 1 else t.H * t.W // 16
            bad_stats = hp.stats_violations(sbuf, outs["out"], t, rpi) if rpi == want_rpi else -1
        outs2, sbuf2, rpi2 = _run(name, line, dtype, inp)
        same = rpi2 == rpi and torch.equal(_bits(outs["out"]), _bits(outs2["out"])) and (sbuf is None or torch.equal(sbuf.view(torch.int32), sbuf2.view(torch.int32)))
        as256 = c[3] != 1 or not tiles_agree or torch.equal(_bits(outs["out"]), _bits(o256))
        print(f"{name} cfg {c}: worst |out - ref| / bound {worst:.3f}, {bad} outside, rows/image {rpi}, "
              f"bits equal to bm 256: {as256 if c[3] == 1 and tiles_agree else 'n/a'} (bm 256 == bm 128: {tiles_agree})")
        if bad or bad_stats or not same or not as256:
            failures.append(f"  cfg (algo, bm, bn, splitk, stages) = {c}: worst |out - ref| / bound {worst:.3f}, {bad} elements outside"
                            + (f", {bad_stats} partial sums outside (rows/image {rpi})" if t.stats else "")
                            + ("" if same else ", two launches differ in bits") + ("" if as256 else ", differs in bits from bm 256"))
    assert not failures, f"{name}: {len(failures)} of {len(cfgs)} configurations fail:\n" + "\n".join(failures)
    assert B * tiles > 0


LATER = hp.read_tile_table(_lib.TILE_TABLE_LATER_PATHS[0])
LATER_CASES = [(hp.tile_id(t, dt), t, dt) for t in LATER for dt in (BF16, F16)]


@pytest.mark.parametrize("name,t,dtype", LATER_CASES, ids=[c[0] for c in LATER_CASES])
def test_shipped_224_row_line_at_its_own_shape(name, t, dtype):
    assert t.bm == BM and t.algo == ALGO_PIPE
    inp = hp.igemm_inputs(t, "cuda", seed=zlib.crc32(name.encode()) & 0xFFFF)
    outs, sbuf, rpi = _run(name, t, dtype, inp)
    ref, bound = hp.igemm_ref(t, dtype, inp)
    bad, worst = hp.igemm_violations(outs["out"], ref["out"], bound["out"])
    bad_stats = hp.stats_violations(sbuf, outs["out"], t, rpi) if t.stats else 0
    print(f"{name}: worst |out - ref| / bound {worst:.3f}, outside {bad}, stats rows/image {rpi} outside {bad_stats}")
    assert bad == 0, f"{name}: {bad} elements outside their bound, worst ratio {worst:.2f}"
    assert not t.stats or (rpi == 42 and bad_stats == 0), f"{name}: {bad_stats} GroupNorm partial sums outside, rows/image {rpi}"
    outs2, sbuf2, rpi2 = _run(name, t, dtype, inp)
    assert rpi2 == rpi and torch.equal(_bits(outs["out"]), _bits(outs2["out"])), f"{name}: two launches differ in bits"
    assert sbuf is None or torch.equal(sbuf.view(torch.int32), sbuf2.view(torch.int32)), f"{name}: two launches differ in their partial sums"
