"""Float64 parity of the flash attention (csrc/attention.hip: attention_kernel, attention_pipe_kernel) and of kv_pack_kernel through the C
entry points k22_attention and k22_attention_masked, in all five arithmetics.  Reference, inputs, bound, mutants and the measured
yardsticks: tests/attention_ref.py; the bound's resolving power: tests/test_attention_parity_cpu.py.

Every buffer a launch writes is pre-filled with NaN and carries guard elements in front and behind: every owned element is checked against
its bound (K_all / V^T_all: bit for bit), every other element must still hold the fill.  Unmasked cases go through k22_attention; masked
cases, S = 0 with a null context and the x3-chunk output go through k22_attention_masked.  The unmasked 16-bit launches run
attention_pipe_kernel by default; test_pipe_equals_plain runs both kernels in one process ("att_pipe") and asserts equal bits."""
import pytest
import torch

import attention_ref as at
import helpers as hp
from kandinsky2_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256                                   # fill elements on both sides of K_all / V^T_all (a multiple of 16 bytes in every type)
_EINVAL = -1                                  # include/k22.h: K22_EINVAL
VARIANTS = [(at.BF16, 0), (at.F16, 0), (at.F32, 0), (at.X3, 0), (at.X3, 1), (at.X2, 0), (at.X2, 1)]
VAR_IDS = [at.DT_NAME[dt] + ("-x3out" if ox else "") for dt, ox in VARIANTS]
CASE_IDS = [at.case_id(c) for c in at.CASES]


def L():
    return _lib.lib()


def guarded(shape, T, guard):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * guard,), at.ar.NAN, dtype=T, device=DEV)
    return buf, buf[guard:guard + n].view(*shape)


_INPUTS, _REFS = {}, {}


def inputs(c, fam):
    """the family's inputs on the device (made once)"""
    if (c, fam) not in _INPUTS:
        _INPUTS[(c, fam)] = at.to_dev(at.inputs(c, fam), DEV)
    return _INPUTS[(c, fam)]


def reference(c, fam, dtype, out_x3):
    """(ref, bound, yardstick) in float64 on the device (computed once, never changed)"""
    key = (c, fam, dtype, out_x3)
    if key not in _REFS:
        d = inputs(c, fam)
        ref, bnd, (q, k, v, A, amp) = at.ref_and_bound(d, c, dtype, out_x3)
        _REFS[key] = (ref, bnd, at.yardstick(at.plain32(q, k, v, c, d["key_valid"]), ref, A, amp))
    return _REFS[key]


def through_masked(c, out_x3):
    return at.masked(c) or c.S == 0 or bool(out_x3)


def run(c, d, dtype, out_x3=0):
    """one kv_pack + attention launch -> (rc, out buffer, K_all buffer, V^T_all buffer), guards included"""
    T = hp.storage_T(dtype)
    C = c.H * 64
    Tkp = (c.S + c.T + 63) // 64 * 64
    qkv = at.storage(d["qkv"], dtype).view(c.B * c.T, 3 * C)
    ctx = None if d["ctx"] is None else at.storage(d["ctx"], dtype).view(c.B * c.S, 2 * C)
    kbuf, kall = guarded((c.B, c.H, Tkp, 64), T, GUARD)
    vbuf, vtall = guarded((c.B, c.H, 64, Tkp), T, GUARD)
    obuf, out = guarded((c.B * c.T, C), T, 16 * C)            # more than the unused query slots of the last workgroup
    if through_masked(c, out_x3):
        rc = L().k22_attention_masked(qkv.data_ptr(), _lib.ptr(ctx), kall.data_ptr(), vtall.data_ptr(), out.data_ptr(), c.B, c.H, c.T, c.S,
                                      c.causal, _lib.ptr(d["key_valid"]), c.kv_n, out_x3, dtype, hp.stream())
    else:
        rc = L().k22_attention(qkv.data_ptr(), ctx.data_ptr(), kall.data_ptr(), vtall.data_ptr(), out.data_ptr(), c.B, c.H, c.T, c.S, dtype,
                               hp.stream())
    torch.cuda.synchronize()
    return rc, obuf, kbuf, vbuf


def check_out(c, obuf, ref, bnd, dtype, out_x3):
    """-> (violations, largest |out - ref| / bound); the guards must hold the fill"""
    g = 16 * c.H * 64
    if out_x3:
        owned = hp.x3_value(obuf[g:-g].view(c.B * c.T, c.H * 64)).reshape(-1)
        obuf = torch.cat([obuf[:g].double(), owned, obuf[-g:].double()])
    return at.ar.violations(obuf, at.ar.with_guard(ref, g), at.ar.with_guard(bnd, g, 0.0))


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def check_pack(c, d, kbuf, vbuf, dtype):
    """class E: the operands bit for bit, exact zeros from key Tk on, the fill everywhere else -> number of differing elements"""
    kexp, vexp = at.pack_ref(d, c, dtype)
    Tk = c.S + c.T
    assert bool((kexp[:, :, Tk:] == 0).all()) and bool((vexp[:, :, :, Tk:] == 0).all())
    nk = (bits(kbuf) != bits(at.ar.with_guard(kexp, GUARD))).sum().item()
    nv = (bits(vbuf) != bits(at.ar.with_guard(vexp, GUARD))).sum().item()
    return int(nk + nv)


def check_launch(c, fam, dtype, out_x3, what):
    d = inputs(c, fam)
    ref, bnd, yard = reference(c, fam, dtype, out_x3)
    print(f"{what} {fam}: torch fp32 yardstick {yard:.3f} (c = {at.ATT_C})")
    assert yard < at.ATT_C
    rc, obuf, kbuf, vbuf = run(c, d, dtype, out_x3)
    assert rc == 0, L().k22_last_error()
    nbad, ratio = check_out(c, obuf, ref, bnd, dtype, out_x3)
    print(f"    largest |out - ref| / bound = {ratio:.3f}")
    assert nbad == 0, (what, fam, nbad, ratio)
    if not out_x3:
        g = 16 * c.H * 64
        assert bool(torch.isfinite(obuf[g:-g]).all())
    assert check_pack(c, d, kbuf, vbuf, dtype) == 0, (what, fam)
    return obuf, ratio


def kernel_path(c, dtype, pipe=True):
    return "pipe" if (pipe and not at.masked(c) and dtype in (at.BF16, at.F16, at.X2)) else "plain"


@pytest.mark.parametrize("dtype,out_x3", VARIANTS, ids=VAR_IDS)
@pytest.mark.parametrize("c", at.CASES, ids=CASE_IDS)
def test_attention_parity(c, dtype, out_x3):
    worst = 0.0
    for fam in at.FAMILIES:
        _, ratio = check_launch(c, fam, dtype, out_x3, f"{at.DT_NAME[dtype]}{'-x3out' if out_x3 else ''} {at.case_id(c)} [{kernel_path(c, dtype)}]")
        worst = max(worst, ratio)
    print(f"attention {at.DT_NAME[dtype]}{'-x3out' if out_x3 else ''} [{kernel_path(c, dtype)}] {at.case_id(c)}: largest |out - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype,out_x3", VARIANTS, ids=VAR_IDS)
def test_attention_spike_rescale_branch(dtype, out_x3):
    """one key in the third tile dominates query 3 and raises the running maximum of others late: the online-softmax rescale, through the bound"""
    c = at.SPIKE_CASE
    obuf, _ = check_launch(c, "spike", dtype, out_x3, f"{at.DT_NAME[dtype]}{'-x3out' if out_x3 else ''} spike [{kernel_path(c, dtype)}]")
    if not out_x3:                                             # query 3's row is the spike key's V row
        g = 16 * c.H * 64
        row = obuf[g:-g].view(c.T, 64)[at.SPIKE_QUERY].double()
        _, bnd, _ = reference(c, "spike", dtype, out_x3)
        want = at.seen(inputs(c, "spike")["qkv"][0, at.SPIKE_SELF_ROW, 2, 0], dtype)
        assert bool(((row - want).abs() <= bnd[at.SPIKE_QUERY]).all())


def set_pipe(v):
    _lib.check(L().k22_set_option(b"att_pipe", v))


@pytest.mark.parametrize("dtype,out_x3", [(at.BF16, 0), (at.F16, 0), (at.X2, 0), (at.X2, 1)], ids=["bf16", "fp16", "x2", "x2-x3out"])
@pytest.mark.parametrize("c", at.UNMASKED, ids=[at.case_id(c) for c in at.UNMASKED])
def test_pipe_equals_plain(c, dtype, out_x3):
    """attention_pipe_kernel against attention_kernel on the same launch: equal bits (csrc/attention.hip's claim), and both inside the bound"""
    fams = at.FAMILIES + (("spike",) if c == at.SPIKE_CASE else ())
    try:
        for fam in fams:
            got = {}
            for pipe in (1, 0):
                set_pipe(pipe)
                got[pipe], ratio = check_launch(c, fam, dtype, out_x3, f"{at.DT_NAME[dtype]}{'-x3out' if out_x3 else ''} {at.case_id(c)} [{kernel_path(c, dtype, pipe)}]")
            assert torch.equal(bits(got[1]), bits(got[0])), (at.case_id(c), fam, int((bits(got[1]) != bits(got[0])).sum().item()))
    finally:
        set_pipe(-1)


def test_masked_entry_refusals():
    """the three K22_EINVAL conditions launch nothing; the library stays usable; an unknown option name still fails"""
    c = at.Case(2, 2, 64, 5, 0, None, 0)
    d = at.to_dev(at.inputs(c, "rand"), DEV)
    C = c.H * 64
    Tkp = (c.S + c.T + 63) // 64 * 64
    kv = torch.ones(c.B, c.S + c.T + 1, device=DEV)
    for dtype, causal, kv_n, out_x3 in ((at.BF16, 1, 0, 0), (at.F32, 0, c.S + c.T + 1, 0), (at.BF16, 0, 0, 1), (at.F16, 0, 0, 1), (at.F32, 0, 0, 1)):
        T = hp.storage_T(dtype)
        qkv = at.storage(d["qkv"], dtype).view(c.B * c.T, 3 * C)
        ctx = at.storage(d["ctx"], dtype).view(c.B * c.S, 2 * C)
        kbuf, kall = guarded((c.B, c.H, Tkp, 64), T, GUARD)
        vbuf, vtall = guarded((c.B, c.H, 64, Tkp), T, GUARD)
        obuf, out = guarded((c.B * c.T, C), T, 16 * C)
        rc = L().k22_attention_masked(qkv.data_ptr(), ctx.data_ptr(), kall.data_ptr(), vtall.data_ptr(), out.data_ptr(), c.B, c.H, c.T, c.S,
                                      causal, kv.data_ptr() if kv_n else None, kv_n, out_x3, dtype, hp.stream())
        torch.cuda.synchronize()
        assert rc == _EINVAL, (dtype, causal, kv_n, out_x3, rc)
        assert bool(torch.isnan(kbuf).all()) and bool(torch.isnan(vbuf).all()) and bool(torch.isnan(obuf).all())
    assert L().k22_set_option(b"att_pipe_", 1) != 0
    assert L().k22_set_option(b"no_such_option", 0) != 0
    cm = at.MASKED[5]                                          # (1, 64, 9, 64) causal, after the refusals
    check_launch(cm, "edges", at.BF16, 0, f"bf16 {at.case_id(cm)} after the refusals")
