"""Float64 parity of the UNet's GroupNorm32 kernels, one kernel per launch (include/k22.h: k22_gn_stats / k22_gn_coeff / k22_gn_apply run the
launchers K22UNet::op_gn runs), of k22_groupnorm end to end and of the shipped producer chains (convolution / GEMM epilogue sums ->
coefficients -> apply).  References, inputs, bound derivations and the measured ratios: tests/gn_ref.py; its CPU half:
tests/test_gn_parity_cpu.py.

Every output buffer is pre-filled with NaN and carries guard elements on both sides: every element a launch owns is checked, every other
one must still hold the fill.  Each test prints the kernel's largest |error| / bound and that of torch's own fp32 evaluation on this device."""
import ctypes as C

import pytest
import torch

import aux_ref as ar
import gn_ref as gr
import helpers as hp
from kandinsky2_amd import _lib

pytestmark = pytest.mark.gpu
DT_IDS = [gr.DT_NAME[d] for d in gr.DTYPES]
ADT_IDS = [gr.DT_NAME[d] for d in gr.APPLY_DTYPES]
DEV = "cuda"
GUARD = 256          # elements of fill on both sides of every output (a multiple of 32 bytes in every type)
_EINVAL = -1         # include/k22.h: K22_EINVAL


def L():
    return _lib.lib()


def guarded(shape, T, guard=GUARD):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * guard,), ar.NAN, dtype=T, device=DEV)
    return buf, buf[guard:guard + n].view(*shape)


def guards_intact(buf, guard=GUARD):
    return bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[-guard:]).all())


def sync():
    torch.cuda.synchronize()


def storage_T(dtype):
    return hp.tdt(gr.storage(dtype))


def film_ptr(film):
    return (None, 0) if film is None else (film["buf"].data_ptr() + 4 * film["off"], film["ld"])


def split_T(x, C0, T):
    """x [...][C] fp32 holding T values -> the two NHWC tensors of the virtual concat C0 | C - C0 (the second None without one)"""
    x0 = x[..., :C0].to(T).contiguous()
    x1 = x[..., C0:].to(T).contiguous() if C0 < x.shape[-1] else None
    return x0, x1


# ---- statistics -------------------------------------------------------------------------------------------------------------------------------
def run_stats(x0, x1, C0, C1, B, HW, ns_buf, dtype):
    buf, out = guarded((B, ns_buf, C0 + C1, 2), torch.float32)
    ns = C.c_int(-1)
    rc = L().k22_gn_stats(x0.data_ptr(), _lib.ptr(x1), C0, C1, B, HW, out.data_ptr(), C.byref(ns), dtype, hp.stream())
    sync()
    return rc, ns.value, buf, out


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=DT_IDS)
def test_statistics(dtype):
    worst = yard = 0.0
    for (C0, C1, B, HW) in gr.stats_cases():
        x = gr.stats_input(C0, C1, B, HW, dtype).to(DEV)
        x0, x1 = split_T(x, C0, hp.tdt(dtype))
        ns = gr.nsplit(B, HW)
        rc, ns_out, buf, out = run_stats(x0, x1, C0, C1, B, HW, ns, dtype)
        assert rc == 0, L().k22_last_error()
        assert ns_out == ns, (B, HW, ns_out, ns)
        assert guards_intact(buf) and not bool(torch.isnan(out).any()), (C0, C1, B, HW)
        n = gr.stats_n(HW, ns, C0 + C1)
        x64 = x.double()
        nbad, ratio = gr.stats_check(out, x64, n)
        assert nbad == 0, (C0, C1, B, HW, nbad, ratio)
        for s in gr.empty_ranges(HW, ns):
            assert bool((out[:, s] == 0).all()), (C0, C1, B, HW, s)
        worst = max(worst, ratio)
        yard = max(yard, gr.stats_check(gr.stats_ref(x, ns), x64, n)[1])
    print(f"gn_stats {gr.DT_NAME[dtype]}: largest |error| / bound = {worst:.3f}; torch fp32 on this device {yard:.3f}")
    assert yard < 1.0


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=DT_IDS)
def test_statistics_refusals(dtype):
    for (C0, C1) in ((192, 0), (70, 58), (3200, 0)):           # C % 128, C0 % 4, C > 3072
        x = torch.zeros(2, 16, C0 + C1, device=DEV)
        x0, x1 = split_T(x, C0, hp.tdt(dtype))
        rc, _, buf, _ = run_stats(x0, x1, C0, C1, 2, 16, 1, dtype)
        assert rc == _EINVAL and bool(torch.isnan(buf).all()), (C0, C1)


# ---- coefficients -------------------------------------------------------------------------------------------------------------------------------
def run_coeff(srcs, B, HW, ga, be, film_b, eps, **over):
    Cn = sum(s[2] for s in srcs)
    buf, out = guarded((B, Cn, 2), torch.float32)
    fp, ld = film_ptr(film_b)
    a = {"st0": srcs[0][0].data_ptr(), "rpi0": srcs[0][1], "C0": srcs[0][2], "st1": srcs[1][0].data_ptr() if len(srcs) > 1 else None,
         "rpi1": srcs[1][1] if len(srcs) > 1 else 0, "C1": srcs[1][2] if len(srcs) > 1 else 0, "gamma": ga.data_ptr(), "beta": be.data_ptr(),
         "film": fp, "ld": ld, "coeff": out.data_ptr()}
    a.update(over)
    rc = L().k22_gn_coeff(a["st0"], a["rpi0"], a["C0"], a["st1"], a["rpi1"], a["C1"], B, HW, a["gamma"], a["beta"], a["film"], a["ld"], eps,
                          a["coeff"], hp.stream())
    sync()
    return rc, buf, out


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=DT_IDS)
def test_coefficients_from_supplied_rows(dtype):
    worst = 0.0
    for case in gr.COEFF_CASES:
        B, HW, eps = case[4], case[5], case[6]
        d = gr.to_dev(gr.coeff_inputs(case, dtype), DEV)
        assert gr.coeff_conditioned(d["srcs"], B, HW), case
        ref = gr.coeff_ref(d["srcs"], B, HW, d["gamma"], d["beta"], d["film"], eps)
        rc, buf, out = run_coeff(d["srcs"], B, HW, d["gamma"], d["beta"], d["film"], eps)
        assert rc == 0, L().k22_last_error()
        nbad, ratio = ar.violations(buf, ar.with_guard(ref["coeff"], GUARD), ar.with_guard(ref["bound"], GUARD, 0.0))
        assert nbad == 0, (case, nbad, ratio)
        worst = max(worst, ratio)
    print(f"gn_coeff ({gr.DT_NAME[dtype]}-rounded inputs): largest |error| / bound = {worst:.3f}")


def test_coefficient_refusals():
    case = gr.COEFF_CASES[1]
    B, HW, eps = case[4], case[5], case[6]
    d = gr.to_dev(gr.coeff_inputs(case, gr.F32), DEV)
    args = (d["srcs"], B, HW, d["gamma"], d["beta"], d["film"], eps)
    for over in ({"C1": 240}, {"rpi0": 0}, {"rpi1": 0}, {"st1": None}, {"ld": 2 * 384 - 1}, {"gamma": None}, {"beta": None},
                 {"C0": 8192, "C1": 32, "film": None}):
        rc, buf, _ = run_coeff(*args, **over)
        assert rc == _EINVAL and bool(torch.isnan(buf).all()), over
    assert run_coeff(*args, coeff=None)[0] == _EINVAL


# ---- apply ----------------------------------------------------------------------------------------------------------------------------------------
def run_apply(x0, x1, C0, C1, B, H, W, coeff, act, mode, pad, dtype):
    Ho, Wo = gr.out_hw(H, W, mode)
    buf, out = guarded((B, Ho + 2 * pad, Wo + 2 * pad, C0 + C1), storage_T(dtype))
    rc = L().k22_gn_apply(x0.data_ptr(), _lib.ptr(x1), C0, C1, B, H, W, coeff.data_ptr(), act, mode, pad, out.data_ptr(), dtype, hp.stream())
    sync()
    return rc, buf, out


def stored_value(out, dtype):
    """float64 value of what a launch stored: the elements themselves, or hi + lo of the x3 chunks"""
    return hp.x3_value(out) if dtype in hp.X_DTYPES else out.double()


def check_output(buf, out, ref, bound, dtype, pad):
    assert guards_intact(buf)
    nbad, ratio = ar.violations(stored_value(out, dtype), ref, bound)
    if pad:                                                    # E: the zero border, exactly (an x3 chunk of zeros is all zero bits)
        m = gr.border_mask(out.shape, DEV)
        assert bool((out[:, m] == 0).all())
    return nbad, ratio


@pytest.mark.parametrize("dtype", gr.APPLY_DTYPES, ids=ADT_IDS)
def test_apply(dtype):
    worst = yard = 0.0
    T = storage_T(dtype)
    for (C0, C1, B, H, W) in gr.apply_cases():
        d = gr.to_dev(gr.apply_inputs(C0, C1, B, H, W, dtype), DEV)
        x0, x1 = split_T(d["x"], C0, T)
        x64, c64 = d["x"].double(), d["coeff"].double()
        for pad in (0, 1):
            plain = None
            for mode in (0, 1, 2):
                for act in (0, 1):
                    ref, bound = gr.apply_ref(x64, c64, act, mode, pad, dtype)
                    rc, buf, out = run_apply(x0, x1, C0, C1, B, H, W, d["coeff"], act, mode, pad, dtype)
                    assert rc == 0, L().k22_last_error()
                    nbad, ratio = check_output(buf, out, ref, bound, dtype, pad)
                    assert nbad == 0, (C0, C1, B, H, W, pad, mode, act, nbad, ratio)
                    worst = max(worst, ratio)
                    t32 = gr.apply_torch32(d["x"], d["coeff"], act, mode, pad).to(T)
                    yard = max(yard, ar.violations(t32, ref, bound)[1])
                    if act == 0 and mode == 0:
                        plain = out
                    if act == 0 and mode == 2:                 # E: nearest upsample = the bits of the source pixel's mode-0 value
                        ys, xs = torch.arange(2 * H, device=DEV) >> 1, torch.arange(2 * W, device=DEV) >> 1
                        inner = lambda t, h, w: t[:, pad:pad + h, pad:pad + w]   # noqa: E731
                        want = inner(plain, H, W)[:, ys][:, :, xs]
                        assert torch.equal(inner(out, 2 * H, 2 * W).contiguous().view(torch.int32), want.contiguous().view(torch.int32)), (C0, H, W, pad)
    print(f"gn_apply {gr.DT_NAME[dtype]}: largest |error| / bound = {worst:.3f}; torch fp32 on this device {yard:.3f}")
    assert yard < 1.0


@pytest.mark.parametrize("dtype", gr.APPLY_DTYPES, ids=ADT_IDS)
def test_apply_refusals(dtype):
    T = storage_T(dtype)
    bad_c = 130 if T == torch.float32 else 132
    x = torch.zeros(1, 4, 4, 136, device=DEV)
    coeff = torch.zeros(1, 136, 2, device=DEV)
    for (C0, C1, mode) in ((bad_c, 0, 0), (bad_c - 64, 64, 0), (128, 0, 3)):
        x0, x1 = split_T(x[..., :C0 + C1], C0, T)
        rc, buf, _ = run_apply(x0, x1, C0, C1, 1, 4, 4, coeff, 0, mode, 1, dtype)
        assert rc == _EINVAL and bool(torch.isnan(buf).all()), (C0, C1, mode)


# ---- k22_groupnorm end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", gr.APPLY_DTYPES, ids=ADT_IDS)
def test_groupnorm_end_to_end(dtype):
    worst = yard = 0.0
    T = storage_T(dtype)
    for case in gr.E2E_CASES:
        C0, C1, B, H, W, fam, film, act, mode, pad = case
        Cn, HW = C0 + C1, H * W
        d = gr.to_dev(gr.e2e_inputs(case, dtype), DEV)
        x0, x1 = split_T(d["x"], C0, T)
        Ho, Wo = gr.out_hw(H, W, mode)
        buf, out = guarded((B, Ho + 2 * pad, Wo + 2 * pad, Cn), T)
        scratch = torch.empty(L().k22_groupnorm_scratch_bytes(B, Cn), dtype=torch.uint8, device=DEV)
        fp, ld = film_ptr(d["film"])
        _lib.check(L().k22_groupnorm(x0.data_ptr(), _lib.ptr(x1), C0, C1, B, H, W, d["gamma"].data_ptr(), d["beta"].data_ptr(), fp, ld, 1e-5,
                                     act, mode, pad, scratch.data_ptr(), out.data_ptr(), dtype, hp.stream()))
        sync()
        x64 = d["x"].double()
        ds, dq = gr.stats_bounds(x64.view(B, HW, Cn), gr.stats_n(HW, gr.nsplit(B, HW), Cn))
        ref, bound = gr.e2e_ref(x64, d["gamma"], d["beta"], d["film"], 1e-5, act, mode, pad, dtype, ds, dq)
        nbad, ratio = check_output(buf, out, ref, bound, dtype, pad)
        assert nbad == 0, (case, nbad, ratio)
        worst = max(worst, ratio)
        t32 = gr.e2e_torch(d["x"], d["gamma"], d["beta"], d["film"], 1e-5, act, mode, pad).to(T)
        yard = max(yard, ar.violations(t32, ref, bound)[1])
    print(f"k22_groupnorm {gr.DT_NAME[dtype]}: largest |error| / bound = {worst:.3f}; torch fp32 on this device {yard:.3f}")
    assert yard < 1.0


# ---- the shipped chains: producer epilogue sums -> coefficients -> apply -----------------------------------------------------------------------------
CH_B, CH_H, CH_W = 2, 12, 12


def conv_producer(Cin, Cout, bm, dtype, seed):
    """k22_conv3x3_gnstats (LDS-halo kernel, one split) -> (stored NHWC T tensor, stats rows fp32 [B * rpi][Cout][2], rpi)"""
    T = hp.tdt(dtype)
    B, H, W = CH_B, CH_H, CH_W
    g = ar.gen(7300 + seed)
    x = ar.acts(g, B, Cin, H, W) + 0.5 * torch.arange(B, dtype=torch.float32)[:, None, None, None]
    w = ar.rn(g, Cout, Cin, 3, 3) * (9 * Cin) ** -0.5
    bias = (0.3 + 0.05 * torch.arange(Cout, dtype=torch.float32)).to(DEV)
    xp, wp = hp.nhwc_padded(x.to(DEV), T), hp.pack_conv3(w.to(DEV), T)
    out = torch.full((B, H, W, Cout), ar.NAN, dtype=T, device=DEV)
    partial = torch.empty(B * H * W * Cout + 64, dtype=torch.float32, device=DEV)
    cap = B * (H * (W + 2) // 16 + 2)
    sbuf = torch.full((cap, Cout, 2), ar.NAN, dtype=torch.float32, device=DEV)
    rpi = C.c_int(0)
    _lib.check(L().k22_set_option(b"conv_algo", 2))
    try:
        _lib.check(L().k22_conv3x3_gnstats(xp.data_ptr(), wp.data_ptr(), bias.data_ptr(), None, out.data_ptr(), partial.data_ptr(), B, H, W, Cin, Cout,
                                           wp.shape[0], 1, bm, 0, sbuf.data_ptr(), cap, C.byref(rpi), dtype, hp.stream()))
    finally:
        _lib.check(L().k22_set_option(b"conv_algo", 0))
    sync()
    assert rpi.value > 0 and bool(torch.isnan(sbuf[B * rpi.value:]).all())
    return out, sbuf[:B * rpi.value].contiguous(), rpi.value


def gemm_producer(K, N, bm, dtype, seed):
    """k22_gemm_gnstats (proj_out: 1x1 convolution over the image rows) -> (stored [B][H][W][N] T tensor, stats rows, rpi)"""
    T = hp.tdt(dtype)
    B, H, W = CH_B, CH_H, CH_W
    M = B * H * W
    g = ar.gen(7400 + seed)
    a = (ar.acts(g, M, K) + 0.5 * torch.arange(B, dtype=torch.float32).repeat_interleave(H * W)[:, None]).to(DEV).to(T).contiguous()
    wp = hp.pad_rows((ar.rn(g, N, K) * K ** -0.5).to(DEV).to(T))
    bias = (0.3 + 0.05 * torch.arange(N, dtype=torch.float32)).to(DEV)
    out = torch.full((B, H, W, N), ar.NAN, dtype=T, device=DEV)
    partial = torch.empty(M * N + 64, dtype=torch.float32, device=DEV)
    cap = B * (H * W // 16 + 2)
    sbuf = torch.full((cap, N, 2), ar.NAN, dtype=torch.float32, device=DEV)
    rpi = C.c_int(0)
    _lib.check(L().k22_gemm_gnstats(a.data_ptr(), wp.data_ptr(), bias.data_ptr(), None, out.data_ptr(), partial.data_ptr(), B, H, W, N, wp.shape[0], K,
                                    1, bm, sbuf.data_ptr(), cap, C.byref(rpi), dtype, hp.stream()))
    sync()
    assert rpi.value > 0 and bool(torch.isnan(sbuf[B * rpi.value:]).all())
    return out, sbuf[:B * rpi.value].contiguous(), rpi.value


def run_chain(parts, film, act, mode, pad, dtype, tag):
    """parts: [(stored tensor, stats rows, rpi)] of the virtual concat.  Producer route (the rows as delivered) and stand-alone route
    (k22_gn_stats over the same tensors): both must meet the end-to-end bound; their coefficient difference is printed."""
    B, H, W = CH_B, CH_H, CH_W
    HW = H * W
    x0, x1 = parts[0][0], (parts[1][0] if len(parts) > 1 else None)
    C0, C1 = x0.shape[-1], (x1.shape[-1] if x1 is not None else 0)
    Cn = C0 + C1
    assert not bool(torch.isnan(x0.float()).any()) and (x1 is None or not bool(torch.isnan(x1.float()).any()))
    x64 = torch.cat([p[0].double() for p in parts], -1)
    ga, be = (t.to(DEV) for t in gr.affine(Cn, seed=5))
    fl = gr.to_dev(gr.film_b(B, Cn, seed=5), DEV) if film else None
    ns = gr.nsplit(B, HW)
    rc, ns_out, sbuf, srows = run_stats(x0, x1, C0, C1, B, HW, ns, dtype)
    assert rc == 0 and ns_out == ns and guards_intact(sbuf)
    routes = {"producer": ([(p[1], p[2], p[0].shape[-1]) for p in parts], hp.IGEMM_C),
              "stand-alone": ([(srows.reshape(B * ns, Cn, 2), ns, Cn)], gr.stats_n(HW, ns, Cn))}
    coeffs, ratios = {}, {}
    for name, (srcs, n) in routes.items():
        rc, cbuf, coeff = run_coeff(srcs, B, HW, ga, be, fl, 1e-5)
        assert rc == 0 and guards_intact(cbuf), L().k22_last_error()
        rc, buf, out = run_apply(x0, x1, C0, C1, B, H, W, coeff, act, mode, pad, dtype)
        assert rc == 0, L().k22_last_error()
        ds, dq = gr.stats_bounds(x64.view(B, HW, Cn), n)
        ref, bound = gr.e2e_ref(x64, ga, be, fl, 1e-5, act, mode, pad, dtype, ds, dq)
        nbad, ratios[name] = check_output(buf, out, ref, bound, dtype, pad)
        assert nbad == 0, (tag, name, nbad, ratios[name])
        coeffs[name] = coeff.double()
    diff = (coeffs["producer"] - coeffs["stand-alone"]).abs()
    rel = (diff / coeffs["producer"].abs().clamp_min(1e-30)).max().item()
    print(f"gn chain {tag} {gr.DT_NAME[dtype]}: rows per image {[p[2] for p in parts]} / {ns}; largest |error| / bound producer route "
          f"{ratios['producer']:.3f}, stand-alone route {ratios['stand-alone']:.3f}; coefficients differ by at most {diff.max().item():.3e} "
          f"({rel:.3e} relative)")


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=DT_IDS)
def test_chain_conv_coeff_apply(dtype):
    run_chain([conv_producer(128, 128, 256, dtype, 1)], True, 1, 0, 1, dtype, "conv 128 -> 128")


@pytest.mark.parametrize("second", ["conv", "gemm"])
@pytest.mark.parametrize("dtype", gr.DTYPES, ids=DT_IDS)
def test_chain_two_producers_concat(dtype, second):
    p0 = conv_producer(128, 128, 256, dtype, 2)
    p1 = conv_producer(128, 256, 128, dtype, 3) if second == "conv" else gemm_producer(128, 256, 128, dtype, 3)
    assert p0[2] != p1[2], (p0[2], p1[2])                      # two row counts: each source's own b * rpi * C offset matters
    run_chain([p0, p1], True, 1, 0, 1, dtype, f"conv 128 | {second} 256")
