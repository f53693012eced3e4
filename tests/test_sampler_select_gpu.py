"""Single-kernel float64 parity of k22_sampler_step's three kernels (csrc/sampler.hip: sampler_x0_kernel, sampler_threshold_kernel,
sampler_final_kernel) through the C entry point, observed in the scratch: s_buf at float 0, x0_buf at float 64 (csrc/capi.hip).  References,
inputs, the bound classes (E exact / D derived / M measured constant), the host model that labels the path of every select item, and the
yardstick: tests/sampler_ref.py.

x_out, x0_out and the scratch - sized exactly k22_sampler_scratch_bytes - each sit in a NaN-filled buffer with 256 guard floats on both sides.
Every owned element is checked, the guards and scratch floats 1-63 must still hold the fill, and a second launch into fresh buffers must give
the same bits.  Refusals happen on the host: K22_EINVAL, a k22_last_error text, every buffer untouched.  A launch that fails otherwise - a
device fault - ends the session (pytest.exit): nothing more is launched on a device that has faulted.

Every test prints the largest |out - ref| / bound per kernel; the last one prints the totals per kernel, the items per path label, torch's own
fp32 yardstick on this device (asserted under c) and the time the module's tests took.

MEASURED on an MI355X:
  largest |out - ref| / bound: x0_buf 0.242 (class D), x0_out 0.500 (one division under n = 2), x_out 0.500 (class M, c = 5.696); s_buf exact
  at all 216 select items and at every parity launch with the threshold on
  select items per path label: plain 42, few-samples 45, filtered 98, fall-back 7, generic 24
  torch's own fp32 yardstick of x_out: select items 2.848, parity items 2.661 (the CPU reads the same)
  all 23 tests of the module: 2.3 s (the slowest, HW = 1 with the first launch of the process, 0.7 s)."""
import collections
import time

import pytest
import torch

import helpers as hp
import sampler_ref as sp
from kandinsky2_amd import _lib
from kandinsky2_amd.diffusion import percentile_index

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256
_EINVAL = -1         # include/k22.h: K22_EINVAL
_SPENT = [0.0]
WORST = collections.defaultdict(float)          # kernel output -> largest |out - ref| / bound
LABELS = collections.Counter()                  # path label -> select items
YARD = collections.defaultdict(float)           # "select" / "parity" -> torch's fp32 yardstick on this device


@pytest.fixture(autouse=True)
def _clock():
    t0 = time.perf_counter()
    yield
    _SPENT[0] += time.perf_counter() - t0


def L():
    return _lib.lib()


@pytest.fixture(scope="module")
def table():
    return torch.from_numpy(sp.table()).to(DEV)


def guarded(n):
    return torch.full((n + 2 * GUARD,), sp.NAN, dtype=torch.float32, device=DEV)


def launch(d, table, row, N, HW, cfg, clamp, pct, masked=False, want_x0=True, init=None, mask=None, n_arg=None, hw_arg=None):
    """one k22_sampler_step into fresh NaN-filled buffers -> (rc, [x_out, x0_out, scratch] whole buffers, guards included)"""
    n_el = N * 4 * HW
    n_scr = L().k22_sampler_scratch_bytes(N, HW) // 4
    assert n_scr == n_el + sp.X0_OFF
    obuf, zbuf, sbuf = guarded(n_el), guarded(n_el), guarded(n_scr)
    init = (d["init"] if masked else None) if init is None else init
    mask = (d["mask"] if masked else None) if mask is None else mask
    try:
        rc = L().k22_sampler_step(d["x"].data_ptr(), d["mo"].data_ptr(), d["noise"].data_ptr(), _lib.ptr(init), _lib.ptr(mask),
                                  table.data_ptr(), row, sp.GUIDANCE, cfg, -clamp, clamp, pct[0], pct[1], sbuf[GUARD:].data_ptr(),
                                  obuf[GUARD:].data_ptr(), zbuf[GUARD:].data_ptr() if want_x0 else None, N if n_arg is None else n_arg,
                                  HW if hw_arg is None else hw_arg, hp.stream())
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"k22_sampler_step N={N} HW={HW}: {e}", returncode=3)
    if rc not in (0, _EINVAL):
        pytest.exit(f"k22_sampler_step N={N} HW={HW}: rc {rc}: {L().k22_last_error()}", returncode=3)
    return rc, [obuf, zbuf, sbuf]


def twice(run):
    rc, a = run()
    assert rc == 0, L().k22_last_error()
    rc, b = run()
    assert rc == 0, L().k22_last_error()
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), "a second launch gave other bits"
    return a


def untouched(*bufs):
    return all(bool(torch.isnan(b).all()) for b in bufs)


def bounded(name, buf, ref, bound, what):
    """every owned element inside its bound, every guard still NaN; records the largest ratio under `name`"""
    nbad, ratio = sp.violations(buf, sp.with_guard(ref, GUARD), sp.with_guard(bound, GUARD, 0.0))
    WORST[name] = max(WORST[name], ratio)
    assert nbad == 0, (name, what, nbad, ratio)
    return ratio


def check_step(bufs, d, row, N, HW, cfg, clamp, pct, masked, want_x0, what, x0_exact=None):
    """the three kernels of one launch, each against its own stored inputs -> (the stored x0_buf [N][4][HW], the reference s or None)"""
    obuf, zbuf, sbuf = bufs
    n_el = N * 4 * HW
    scr = sbuf[GUARD:GUARD + sp.X0_OFF + n_el]
    assert untouched(sbuf[:GUARD], sbuf[GUARD + sp.X0_OFF + n_el:], scr[1:sp.X0_OFF]), (what, "scratch guards / floats 1-63")
    x0_buf = scr[sp.X0_OFF:].view(N, 4, HW)
    # sampler_x0_kernel: class D (the select items: the exact clamp(x))
    ref, bound = sp.x0_ref(d, row, cfg, clamp, masked)
    if x0_exact is not None:
        assert torch.equal(x0_buf, x0_exact), (what, "x0_buf is not clamp(x)")
    nbad, ratio = sp.violations(x0_buf, ref, bound)
    WORST["x0_buf"] = max(WORST["x0_buf"], ratio)
    assert nbad == 0, ("x0_buf", what, nbad, ratio)
    # sampler_threshold_kernel: class E against numpy's percentile of the stored image 0
    x0_host = x0_buf.cpu().numpy().reshape(N, 4 * HW)
    s = None
    if pct[0] >= 0:
        s = sp.s_ref(x0_host[0])
        got = scr[0].item()
        assert sp.f32bits(got) == sp.f32bits(s), ("s_buf", what, got, float(s), sp.dispatch(x0_host[0], pct[0]))
    else:
        assert untouched(scr[0:1]), (what, "s_buf written with the threshold off")
    # sampler_final_kernel: from the stored x0_buf and the stored s
    out, z, S = sp.final_ref(x0_buf, s, d, row)
    b_out, b_z = sp.final_bounds(z, S, s is not None)
    bounded("x_out", obuf, out, b_out, what)
    if want_x0:
        bounded("x0_out", zbuf, z, b_z, what)
    else:
        assert untouched(zbuf), (what, "x0_out = NULL")
    return x0_buf, s


# ---- the select: every path of sampler_threshold_kernel, exact ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", sp.SELECT_HW)
def test_select_is_numpys_percentile_on_every_path(HW, table):
    row = sp.table()[sp.SELECT_ROW]
    pct = percentile_index(4 * HW)
    seen = collections.Counter()
    for (hw, case, N, cfg) in sp.select_items():
        if hw != HW:
            continue
        d = sp.to_dev(sp.select_input(HW, case, N), DEV)
        clamp = d["clamp"]
        bufs = twice(lambda: launch(d, table, sp.SELECT_ROW, N, HW, cfg, clamp, pct))
        x0_buf, s = check_step(bufs, d, row, N, HW, cfg, clamp, pct, False, True, (HW, case, N, cfg), x0_exact=sp.select_x0(d))
        assert s > 1.0
        seen[sp.dispatch(x0_buf[0].cpu().numpy(), pct[0]).label] += 1
        YARD["select"] = max(YARD["select"], sp.yardstick(x0_buf, s, d, row))
    LABELS.update(seen)
    print(f"select HW={HW} (KPT {sp.template_kpt(4 * HW)}): {sum(seen.values())} items exact; paths {dict(seen)}")


# ---- parity of the three kernels on random operands -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", sp.PARITY_HW)
def test_step_parity(HW, table):
    for (N, cfg) in sp.PARITY_BATCH:
        d = sp.to_dev(sp.parity_input(N, HW), DEV)
        for k in sp.PARITY_ROWS:
            row = sp.table()[k]
            for masked in (False, True):
                for want_x0 in (True, False):
                    for pct in (percentile_index(4 * HW), (-1, 0.0)):
                        what = (N, HW, cfg, k, masked, want_x0, pct[0])
                        bufs = twice(lambda: launch(d, table, k, N, HW, cfg, sp.PARITY_CLAMP, pct, masked, want_x0))
                        x0_buf, s = check_step(bufs, d, row, N, HW, cfg, sp.PARITY_CLAMP, pct, masked, want_x0, what)
                        YARD["parity"] = max(YARD["parity"], sp.yardstick(x0_buf, s, d, row))
    print(f"step parity HW={HW}: largest |out - ref| / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def test_step_refusals(table):
    N, HW = 2, 255
    d = sp.to_dev(sp.parity_input(N, HW), DEV)
    d3 = sp.to_dev(sp.parity_input(3, HW), DEV)
    pct = percentile_index(4 * HW)
    cases = (("N = 0", dict(n_arg=0)), ("HW = 0", dict(hw_arg=0)), ("mask without init_img", dict(mask=d["mask"])),
             ("init_img without mask", dict(init=d["init"])), ("pct_index = 4 HW", dict(pct=(4 * HW, 0.0))),
             ("pct_index > 4 HW", dict(pct=(4 * HW + 7, 0.5))))
    for name, kw in cases:
        kw = dict(dict(pct=pct), **kw)
        rc, bufs = launch(d, table, 1, N, HW, 1, sp.PARITY_CLAMP, **kw)
        assert rc == _EINVAL and L().k22_last_error() and untouched(*bufs), name
    rc, bufs = launch(d3, table, 1, 3, HW, 1, sp.PARITY_CLAMP, pct)                     # odd N under CFG
    assert rc == _EINVAL and L().k22_last_error() and untouched(*bufs)
    rc, bufs = launch(d, table, 1, N, HW, 1, sp.PARITY_CLAMP, (4 * HW - 1, 0.0))         # the last rank itself runs: the maximum of |x0|
    assert rc == 0, L().k22_last_error()
    x0 = bufs[2][GUARD + sp.X0_OFF:GUARD + sp.X0_OFF + 4 * HW]
    assert bufs[2][GUARD].item() == max(x0.abs().max().item(), 1.0)


def test_zz_report():
    """the last test of the module: the figures recorded in the module docstring; torch's own fp32 evaluation stays under c on this device"""
    print("k22_sampler_step, largest |out - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())) + "; s_buf exact")
    print(f"select items per path label: {dict(LABELS)}")
    print(f"sampler_final x_out yardstick (this device): select items {YARD['select']:.3f}, parity items {YARD['parity']:.3f} (c = {sp.SAMPLER_C})")
    print(f"test_sampler_select_gpu: {_SPENT[0]:.1f} s in all tests of the module")
    assert max(YARD.values(), default=0.0) < sp.SAMPLER_C
    if LABELS:
        assert set(LABELS) == set(sp.LABELS)
