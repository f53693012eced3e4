"""Host-side half of the 224-row tile of conv3_halo_spec_kernel (tests/test_conv3_bm224_gpu.py runs it on the device): where the build
generates the tile, and that nothing else reaches it.

The candidate rule (csrc/tuning.h): bm = 224 for the pipelined specialised kernel (algo 12) in the 16-bit types, where 224 divides the
H x (W + 2) plane and a tile spans at least two of its rows.
"""
import ctypes as C

import pytest

import helpers as hp
from kandinsky2_amd import _lib

BF16, F32, F16, X3, X2 = _lib.K22_BF16, _lib.K22_F32, _lib.K22_F16, _lib.K22_F16X3, _lib.K22_F16X2
ALGO_PIPE, BM = 12, 224


def line(B, H, W, Kc=128, N=128, stats=0, sk=0, algo=ALGO_PIPE, splitk=1):
    return hp._ot_conv(B, H, W, Kc, N, stats=stats, sk=sk)._replace(algo=algo, bm=BM, splitk=splitk)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("H,W", [(14, 14), (28, 14), (8, 26), (16, 96)])
def test_tile_is_generated_where_it_divides_the_plane(H, W, dtype):
    assert (H * (W + 2)) % BM == 0 and 2 * (W + 2) <= BM
    assert hp.tile_accepted(line(2, H, W), dtype) == 1
    cands, resolved, _ = hp.igemm_candidates(line(2, H, W), dtype)
    mine = [(c, r) for c, r in zip(cands, resolved) if c[1] == BM]
    assert mine and all(c[0] == ALGO_PIPE for c, _ in mine)                     # the pipelined form only
    assert all(r[0] == ALGO_PIPE and r[1] == BM and r[3] == c[3] for c, r in mine)   # and it resolves to itself, split as spelt


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("H,W,why", [(20, 20, "440 positions: 224 does not divide the plane"),
                                     (1, 222, "one row of 224 positions: a tile shorter than two rows")])
def test_tile_is_not_generated_elsewhere(H, W, why, dtype):
    assert hp.tile_accepted(line(1, H, W), dtype) == 0, why
    assert all(c[1] != BM for c in hp.igemm_candidates(line(1, H, W), dtype)[0])


@pytest.mark.parametrize("dtype", [F32, X3, X2])
def test_tile_is_a_16_bit_tile(dtype):
    for H, W in ((14, 14), (16, 96)):
        assert hp.tile_accepted(line(2, H, W), dtype) == 0
        assert all(c[1] != BM for c in hp.igemm_candidates(line(2, H, W), dtype)[0])


def test_the_other_halo_kernels_do_not_take_the_tile():
    for algo in (2, 3, 6, 7, 11):
        assert hp.tile_accepted(line(2, 14, 14, algo=algo), BF16) == 0


def test_no_off_table_problem_lists_the_tile():
    n = 0
    for _, t, dt in hp.offtable_cases():
        for frag in (0, 1):
            cands = hp.igemm_candidates(t, dt, frag)[0]
            n += len(cands)
            assert all(c[1] != BM for c in cands), (t, dt)
    assert n > 0


def test_statistics_rows_follow_the_tile():
    """42 partial-sum rows per 96 x 96 image (7 per 16 x 96), against ceil(9408 / 256) = 37"""
    L = _lib.lib()
    for H, rows in ((96, 42), (16, 7)):
        p = hp.tile_problem(line(2, H, 96, stats=1), BF16)
        ops = _lib.K22IgemmOperands()
        one = C.c_int8(0)
        for f in ("A0", "Wp", "out"):
            setattr(ops, f, C.addressof(one))                                   # markers: the launch is refused before any is read
        ops.stats, ops.stats_capacity_rows = C.addressof(one), 2 * rows - 1
        rpi = C.c_int(0)
        assert L.k22_igemm_cfg(C.byref(p), C.byref(ops), C.byref(rpi), None) == -3 and b"too small" in L.k22_last_error()


def test_later_table_replaces_shipped_lines_with_the_tile_and_the_library_holds_them(tmp_path):
    """kandinsky-2_amd/tiles_gfx950_bm224.txt: loaded behind the shipped table when the library is opened.  Every line of it names the
    tile, is a configuration this build generates (as bf16 and as fp16, which resolves through it), and replaces a line of the shipped
    table - which stays there, generated and swept as before; what the opened library resolves those problems to is the later line."""
    (later_path,) = _lib.TILE_TABLE_LATER_PATHS
    later, shipped = hp.read_tile_table(later_path), hp.read_tile_table()
    assert len(later) == 18 and len({hp.tile_key(t) for t in later}) == len(later)
    by_key = {(t.dtype, hp.tile_key(t)): t for t in shipped}
    for t in later:
        assert (t.dtype, t.taps, t.H, t.W, t.algo, t.bm, t.splitk) == (BF16, 9, 96, 96, ALGO_PIPE, BM, 1), t
        assert hp.tile_accepted(t, BF16) == 1 and hp.tile_accepted(t, F16) == 1, hp.tile_id(t)
        old = by_key[(t.dtype, hp.tile_key(t))]
        assert old.bm in (256, 128) and hp.tile_accepted(old, BF16) == 1, hp.tile_id(old)
    import os
    if "K22_TILE_TABLE" in os.environ or "K22_TUNE_CACHE" in os.environ:
        return
    L = _lib.lib()
    L.k22_tile_table_load(_lib.TILE_TABLE_PATH.encode())                      # (as lib() leaves it, whatever ran before in this process)
    L.k22_tile_table_load(later_path.encode())
    out = str(tmp_path / "tiles.txt")
    assert L.k22_tile_table_save(out.encode()) >= len(shipped)
    held = {(t.dtype, hp.tile_key(t)): hp.cfg_of(t) for t in hp.read_tile_table(out)}
    assert all(held[(t.dtype, hp.tile_key(t))] == hp.cfg_of(t) for t in later)


@pytest.mark.parametrize("dtype,H,W", [(BF16, 20, 20), (BF16, 1, 222), (F32, 14, 14), (X3, 14, 14), (X2, 16, 96)])
def test_launch_entry_refuses_the_tile_where_the_acceptance_entry_rejects_it(dtype, H, W):
    L = _lib.lib()
    pr = hp.tile_problem(line(1, H, W), dtype)
    assert L.k22_igemm_cfg_accepted(C.byref(pr)) == 0
    ops = _lib.K22IgemmOperands()                                               # all null
    rpi = C.c_int(7)
    assert L.k22_igemm_cfg(C.byref(pr), C.byref(ops), C.byref(rpi), None) == -1 and rpi.value == 0
    assert b"does not generate" in L.k22_last_error()
