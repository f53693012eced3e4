"""Single-kernel float64 parity of the kernels that open and close a UNet step (csrc/elementwise.hip: conv_in, timestep_embedding, linear_smallm,
layernorm_f32, resample, cast_rows, kv_pack; csrc/sampler.hip: ddim_step, plms_step) through their C entry points (include/k22.h), which run
the engines' own launchers.  References, inputs, bound classes (E exact / D derived / M measured constant) and the yardsticks: tests/seam_ref.py.

Every output buffer is pre-filled with NaN and carries guard elements in front and behind: every element a launch owns is checked, every other
one - guards, row gaps of a strided output - must still hold the fill, and a second launch into a fresh buffer must give the same bits.  Refusals
happen on the host: K22_EINVAL and an untouched buffer.  Each test prints the largest |out - ref| / bound of its kernel, the class-M tests torch's own
fp32 yardstick on this device (asserted under c); the last test prints the time the module's tests took.

MEASURED on an MI355X (largest |out - ref| / bound; a 16-bit output sits near 1 by its own rounding, which the bound contains once):
  conv_in             bf16 0.989, fp16 0.971, fp32 0.047         timestep_embedding  0.198 (torch's yardstick 0.57 / 0.90 / 0.91 at half 5 / 192 / 260)
  linear_smallm       bf16 0.088, fp16 0.086, fp32 0.108 weights  layernorm_f32       0.237 (torch's yardstick up to 5.376 at D = 2560, c = 10.752)
  resample mode 1     bf16 0.996, fp16 0.997, fp32 0.315          resample mode 2, cast_rows, kv_pack: exact
  ddim_step           0.063 / 0.146 / 0.155 / 0.230 per case      plms_step           0.076 / 0.264 / 0.129 / 0.314 per case
  all 36 tests of the module: 2.0 s (the slowest, conv_in bf16 with the first launch of the process, 0.9 s)."""
import time

import pytest
import torch
import torch.nn.functional as F

import helpers as hp
import seam_ref as sr
from kandinsky2_amd import _lib, pack

pytestmark = pytest.mark.gpu
DTYPES = sr.DTYPES
DT_IDS = [sr.DT_NAME[d] for d in DTYPES]
DEV = "cuda"
GUARD = 256          # elements of fill on both sides of every output (a multiple of 16 bytes in every type)
_EINVAL = -1         # include/k22.h: K22_EINVAL
_SPENT = [0.0]


@pytest.fixture(autouse=True)
def _clock():
    t0 = time.perf_counter()
    yield
    _SPENT[0] += time.perf_counter() - t0


def L():
    return _lib.lib()


def err():
    return L().k22_last_error()


def guarded(shape, T, guard=GUARD):
    """(whole buffer, view of `shape` inside it with `guard` NaN elements on both sides)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * guard,), sr.NAN, dtype=T, device=DEV)
    return buf, buf[guard:guard + n].view(*shape)


def untouched(*bufs):
    return all(bool(torch.isnan(b).all()) for b in bufs)


def twice(run):
    """run() -> (rc, [whole buffers]); two launches into fresh buffers must agree in every bit.  -> the first launch's buffers"""
    rc, a = run()
    assert rc == 0, err()
    rc, b = run()
    assert rc == 0, err()
    for u, v in zip(a, b):
        assert torch.equal(sr.bits(u), sr.bits(v)), "a second launch gave other bits"
    return a


def check_bounded(buf, ref, bound, guard=GUARD):
    return sr.violations(buf, sr.with_guard(ref, guard), sr.with_guard(bound, guard, 0.0))


def check_exact(buf, exp, guard=GUARD):
    return sr.exact_violations(buf, sr.with_guard(exp, guard))


# ---- conv_in ------------------------------------------------------------------------------------------------------------------------------
def run_conv_in(d, wp, B, H, W, Cin, Cout, premul, dtype, img=True, mask=True, x=True):
    buf, out = guarded((B, H, W, Cout), hp.tdt(dtype))
    rc = L().k22_conv_in(d["x"].data_ptr() if x else None, d["img"].data_ptr() if img else None, d["mask"].data_ptr() if mask else None,
                         wp.data_ptr(), d["b"].data_ptr(), out.data_ptr(), B, H, W, Cin, Cout, premul, dtype, hp.stream())
    torch.cuda.synchronize()
    return rc, [buf]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_conv_in(dtype):
    worst = 0.0
    for (B, H, W, Cin, Cout, premul, frac) in sr.conv_in_cases():
        d = sr.to_dev(sr.conv_in_inputs(B, H, W, Cin, Cout, frac), DEV)
        wp = pack.pack_stem(d["w"])                                       # the product's own packing of input_blocks.0.0.weight
        ref, S = sr.conv_in_ref(sr.to64(d), Cin, premul)
        # Cin 4: no img, no mask; Cin 8: the hint latent, no mask; Cin 9: both
        buf, = twice(lambda: run_conv_in(d, wp, B, H, W, Cin, Cout, premul, dtype, img=Cin > 4, mask=Cin == 9))
        nbad, ratio = check_bounded(buf, ref, sr.conv_in_bound(ref, S, Cin, dtype))
        worst = max(worst, ratio)
        assert nbad == 0, (B, H, W, Cin, Cout, premul, frac, nbad, ratio)
    print(f"conv_in {sr.DT_NAME[dtype]}: largest |out - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_conv_in_rejects(dtype):
    B, H, W, Cout = 2, 3, 9, 130
    d = sr.to_dev(sr.conv_in_inputs(B, H, W, 9, Cout), DEV)
    wp = pack.pack_stem(d["w"])
    for kw in (dict(Cin=5, premul=1), dict(Cin=9, premul=1, mask=False), dict(Cin=9, premul=1, img=False), dict(Cin=9, premul=0, mask=False),
               dict(Cin=8, premul=1, img=False, mask=False), dict(Cin=8, premul=0, mask=False), dict(Cin=9, premul=1, x=False)):
        a = dict(img=True, mask=True, x=True); a.update(kw)
        rc, bufs = run_conv_in(d, wp, B, H, W, a["Cin"], Cout, a["premul"], dtype, img=a["img"], mask=a["mask"], x=a["x"])
        assert rc == _EINVAL and untouched(*bufs), kw
    for (b, h, w, co) in ((0, H, W, Cout), (B, 0, W, Cout), (B, H, 0, Cout), (B, H, W, 0)):
        buf, out = guarded((B, H, W, Cout), hp.tdt(dtype))
        rc = L().k22_conv_in(d["x"].data_ptr(), d["img"].data_ptr(), d["mask"].data_ptr(), wp.data_ptr(), d["b"].data_ptr(), out.data_ptr(), b, h, w, 9, co,
                             1, dtype, hp.stream())
        torch.cuda.synchronize()
        assert rc == _EINVAL and untouched(buf), (b, h, w, co)


# ---- timestep_embedding ---------------------------------------------------------------------------------------------------------------------
def test_timestep_embedding():
    c = sr.SEAM_C["timestep_embedding"]
    worst = 0.0
    for half in sr.TEMB_HALF:
        yard = 0.0
        for rows in sr.TEMB_ROWS:
            for table in sr.TEMB_TABLES:
                d = sr.to_dev(sr.temb_inputs(rows, half, table), DEV)
                ref = sr.temb_ref(d)
                yard = max(yard, sr.plain_ratio(sr.temb_torch32(d), ref, torch.ones_like(ref)))

                def run():
                    buf, out = guarded((rows, 2 * half), torch.float32)
                    rc = L().k22_timestep_embedding(d["t"].data_ptr(), d["f"].data_ptr(), out.data_ptr(), rows, half, hp.stream())
                    torch.cuda.synchronize()
                    return rc, [buf]
                buf, = twice(run)
                nbad, ratio = check_bounded(buf, ref, sr.temb_bound(ref))
                worst = max(worst, ratio)
                assert nbad == 0, (rows, half, table, nbad, ratio)
        print(f"timestep_embedding half={half}: torch fp32 yardstick {yard:.3f} (c = {c})")
        assert yard < c
    print(f"timestep_embedding: largest |out - ref| / bound = {worst:.3f}")
    buf, out = guarded((1, 10), torch.float32)
    for (rows, half, t_ok) in ((0, 5, True), (1, 0, True), (1, 5, False)):
        rc = L().k22_timestep_embedding(d["t"].data_ptr() if t_ok else None, d["f"].data_ptr(), out.data_ptr(), rows, half, hp.stream())
        assert rc == _EINVAL and untouched(buf)


# ---- linear_smallm ----------------------------------------------------------------------------------------------------------------------------
def run_linear(d, case, wdtype, M=None, K=None):
    M_, N, K_, dx, do, da, add_mod, a_in, a_out, bias = case
    w = d["w"].to(hp.tdt(wdtype)).contiguous()
    buf, out = guarded((M_, N + do), torch.float32)
    rc = L().k22_linear_smallm_ld(d["x"].data_ptr(), K_ + dx, w.data_ptr(), _lib.ptr(d["b"]), _lib.ptr(d["add"]), 0 if da is None else N + da, add_mod,
                                  out.data_ptr(), N + do, M_ if M is None else M, N, K_ if K is None else K, a_in, a_out, wdtype, hp.stream())
    torch.cuda.synchronize()
    return rc, [buf]


@pytest.mark.parametrize("wdtype", DTYPES, ids=DT_IDS)
def test_linear_smallm(wdtype):
    worst = 0.0
    for case in sr.LIN_CASES:
        M, N, K, dx, do, da, add_mod, a_in, a_out, bias = case
        d = sr.to_dev(sr.lin_inputs(case, wdtype), DEV)
        ref, bound = sr.lin_bound(d, case, wdtype)
        full_ref = torch.full((M, N + do), sr.NAN, dtype=torch.float64, device=DEV)      # the columns between N and ldo keep the fill
        full_bound = torch.zeros_like(full_ref)
        full_ref[:, :N] = ref; full_bound[:, :N] = bound
        buf, = twice(lambda: run_linear(d, case, wdtype))
        nbad, ratio = check_bounded(buf, full_ref, full_bound)
        worst = max(worst, ratio)
        assert nbad == 0, (case, sr.lin_rpw(N), nbad, ratio)
    print(f"linear_smallm {sr.DT_NAME[wdtype]} weights: largest |out - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("wdtype", DTYPES, ids=DT_IDS)
def test_linear_smallm_rejects(wdtype):
    epc = 4 if wdtype == sr.F32 else 8
    case = (8, 5, 2056, 0, 0, None, 0, 0, 0, True)
    d = sr.to_dev(sr.lin_inputs(case, wdtype), DEV)
    for kw in (dict(M=0), dict(M=9), dict(M=2, K=epc + epc // 2), dict(M=8, K=2056)):      # 8 * 2056 * 4 bytes > 64 KiB of LDS
        rc, bufs = run_linear(d, case, wdtype, **kw)
        assert rc == _EINVAL and untouched(*bufs), kw
    rc, bufs = run_linear(d, case, wdtype, M=8, K=2048)                                      # the limit itself runs
    assert rc == 0, err()


# ---- layernorm_f32 ------------------------------------------------------------------------------------------------------------------------------
def test_layernorm_f32():
    c = sr.SEAM_C["layernorm"]
    worst = 0.0
    for D in sr.LN_D:
        yards = []
        for offset in (False, True):
            d = sr.to_dev(sr.ln_inputs(D, offset), DEV)
            for rows in sr.LN_ROWS:
                x = d["x"][:rows].contiguous()
                ref, S = sr.ar.layernorm_ref(x.double(), d["g"].double(), d["b"].double(), sr.LN_EPS)
                yards.append(sr.plain_ratio(F.layer_norm(x, (D,), d["g"], d["b"], sr.LN_EPS), ref, S))

                def run():
                    buf, out = guarded((rows, D), torch.float32)
                    rc = L().k22_layernorm_f32(x.data_ptr(), d["g"].data_ptr(), d["b"].data_ptr(), out.data_ptr(), rows, D, sr.LN_EPS, hp.stream())
                    torch.cuda.synchronize()
                    return rc, [buf]
                buf, = twice(run)
                nbad, ratio = check_bounded(buf, ref, sr.ln_bound(ref, S))
                worst = max(worst, ratio)
                assert nbad == 0, (rows, D, offset, nbad, ratio)
        print(f"layernorm_f32 D={D}: torch fp32 yardstick random {max(yards[:2]):.3f}, mean = 10 sd {max(yards[2:]):.3f} (c = {c:.3f})")
        assert max(yards) < c
    print(f"layernorm_f32: largest |out - ref| / bound = {worst:.3f}")
    buf, out = guarded((1, 5), torch.float32)
    for (rows, D, g_ok) in ((0, 5, True), (1, 0, True), (1, 5, False)):
        rc = L().k22_layernorm_f32(x.data_ptr(), d["g"].data_ptr() if g_ok else None, d["b"].data_ptr(), out.data_ptr(), rows, D, sr.LN_EPS, hp.stream())
        assert rc == _EINVAL and untouched(buf)


# ---- resample -----------------------------------------------------------------------------------------------------------------------------------
def run_resample(x, mode, dtype, H=None, W=None, C=None, out_shape=None):
    T = hp.tdt(dtype)
    xt = x.to(T).contiguous()
    B, H_, W_, C_ = xt.shape
    shape = out_shape or ((B, H_ // 2, W_ // 2, C_) if mode == 1 else (B, 2 * H_, 2 * W_, C_))
    buf, out = guarded(shape, T)
    rc = L().k22_resample(xt.data_ptr(), out.data_ptr(), B, H_ if H is None else H, W_ if W is None else W, C_ if C is None else C, mode, dtype, hp.stream())
    torch.cuda.synchronize()
    return rc, [buf]


def resample_check(x, mode, dtype):
    T = hp.tdt(dtype)
    buf, = twice(lambda: run_resample(x, mode, dtype))
    if mode == 1:
        ref, S = sr.rs_ref(x.double(), 1)
        return check_bounded(buf, ref, sr.rs_bound(ref, S, dtype))
    return check_exact(buf, sr.rs_ref(x, 2)[0].to(T)), 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_resample(dtype):
    worst = 0.0
    for (B, H, W, C, mode) in sr.rs_cases(dtype):
        nbad, ratio = resample_check(sr.rs_input(B, H, W, C, dtype).to(DEV), mode, dtype)
        worst = max(worst, ratio)
        assert nbad == 0, (B, H, W, C, mode, nbad, ratio)
    print(f"resample {sr.DT_NAME[dtype]}: largest |out - ref| / bound (mode 1) = {worst:.3f}; mode 2 exact")
    x = sr.rs_input(2, 6, 4, 3 * sr.epv(dtype), dtype).to(DEV)
    for kw in (dict(mode=1, C=sr.epv(dtype) + sr.epv(dtype) // 2), dict(mode=0), dict(mode=3), dict(mode=1, H=1), dict(mode=1, W=1), dict(mode=2, H=0)):
        mode = kw.pop("mode")
        rc, bufs = run_resample(x, mode, dtype, out_shape=(2, 12, 8, 3 * sr.epv(dtype)), **kw)
        assert rc == _EINVAL and untouched(*bufs), (mode, kw)


@pytest.mark.parametrize("mode", [1, 2])
def test_resample_grid_cap(mode):
    """128 x 128 x 129 output vectors of bf16 = 2113536 > 8192 blocks x 256 threads: the launch is capped and every thread walks the grid-stride loop"""
    B, H, W, C = sr.RS_CAP[mode]
    nbad, ratio = resample_check(sr.rs_input(B, H, W, C, sr.BF16, device=DEV), mode, sr.BF16)
    assert nbad == 0, (mode, nbad, ratio)


# ---- cast_rows, kv_pack ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_cast_rows_exact(dtype):
    T = hp.tdt(dtype)
    for (rows, cols, ldx, ldy) in sr.CAST_CASES:
        x = sr.cast_input(rows, ldx, dtype).to(DEV)
        exp = sr.cast_expected(x, rows, cols, ldy, dtype)

        def run():
            buf, out = guarded((rows, ldy), T)
            rc = L().k22_cast_rows(x.data_ptr(), out.data_ptr(), rows, cols, ldx, ldy, dtype, hp.stream())
            torch.cuda.synchronize()
            return rc, [buf]
        buf, = twice(run)
        assert torch.equal(sr.bits(buf), sr.bits(sr.with_guard(exp, GUARD))), (rows, cols, ldx, ldy)      # bits: -0 stays -0, the gaps stay NaN
    buf, out = guarded((2, 8), T)
    for (rows, cols, lx, ly) in ((0, 4, 8, 8), (2, 0, 8, 8), (2, 4, 3, 8), (2, 4, 8, 3)):
        rc = L().k22_cast_rows(x.data_ptr(), out.data_ptr(), rows, cols, lx, ly, dtype, hp.stream())
        assert rc == _EINVAL and untouched(buf)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_kv_pack_exact(dtype):
    T = hp.tdt(dtype)
    for (B, H, Tq, S) in sr.KV_CASES:
        d = sr.to_dev(sr.kv_inputs(B, H, Tq, S, dtype), DEV)
        k, vt = (t.to(T) for t in sr.kv_ref(d, B, H, Tq, S))
        qkv = d["qkv"].to(T).contiguous()
        ckv = d["ctxkv"].to(T).contiguous() if S else None

        def run():
            kbuf, kall = guarded(k.shape, T)
            vbuf, vtall = guarded(vt.shape, T)
            rc = L().k22_kv_pack(qkv.data_ptr(), _lib.ptr(ckv), kall.data_ptr(), vtall.data_ptr(), B, H, Tq, S, dtype, hp.stream())
            torch.cuda.synchronize()
            return rc, [kbuf, vbuf]
        kbuf, vbuf = twice(run)
        assert check_exact(kbuf, k) == 0 and check_exact(vbuf, vt) == 0, (B, H, Tq, S)
        pad = sr.kv_tkp(Tq, S) - S - Tq
        if pad:                                                             # the zero padding to Tkp, in both layouts
            assert bool((kbuf[GUARD:-GUARD].view(k.shape)[:, :, S + Tq:] == 0).all()) and bool((vbuf[GUARD:-GUARD].view(vt.shape)[..., S + Tq:] == 0).all())
    kbuf, kall = guarded((1, 1, 64, 64), T)
    for (b, h, t, s, c_ok) in ((0, 1, 1, 0, True), (1, 0, 1, 0, True), (1, 1, 0, 0, True), (1, 1, 1, -1, True), (1, 1, 1, 5, False)):
        rc = L().k22_kv_pack(qkv.data_ptr(), qkv.data_ptr() if c_ok else None, kall.data_ptr(), kall.data_ptr(), b, h, t, s, dtype, hp.stream())
        assert rc == _EINVAL and untouched(kbuf)


# ---- ddim_step / plms_step --------------------------------------------------------------------------------------------------------------------------
STEP_IDS = [f"N{n}-HW{hw}-cfg{c}" for (n, hw, c) in sr.STEP_CASES]


@pytest.mark.parametrize("N,HW,cfg", sr.STEP_CASES, ids=STEP_IDS)
def test_ddim_step(N, HW, cfg):
    worst = 0.0
    d = sr.to_dev(sr.step_inputs(N, HW), DEV)
    for eta, noise in ((0.0, False), (1.0, True)):
        for k, row in enumerate(sr.step_rows(eta)):
            out, x0, b_out, b_x0 = sr.ddim_ref(d, row, cfg, noise)
            tab = torch.from_numpy(row).to(DEV)
            for want_x0 in (True, False):
                def run():
                    obuf, o = guarded((N, 4, HW), torch.float32)
                    zbuf, z = guarded((N, 4, HW), torch.float32)
                    rc = L().k22_ddim_step(d["x"].data_ptr(), d["mo"].data_ptr(), d["noise"].data_ptr() if noise else None, tab.data_ptr(),
                                           sr.STEP_GUIDANCE, cfg, o.data_ptr(), z.data_ptr() if want_x0 else None, N, HW, hp.stream())
                    torch.cuda.synchronize()
                    return rc, [obuf, zbuf]
                obuf, zbuf = twice(run)
                nbad, ratio = check_bounded(obuf, out, b_out)
                worst = max(worst, ratio)
                assert nbad == 0, ("x_out", N, HW, cfg, eta, k, nbad, ratio)
                if want_x0:
                    nbad, ratio = check_bounded(zbuf, x0, b_x0)
                    worst = max(worst, ratio)
                    assert nbad == 0, ("x0_out", N, HW, cfg, eta, k, nbad, ratio)
                else:
                    assert untouched(zbuf)
    print(f"ddim_step N={N} HW={HW} cfg={cfg}: largest |out - ref| / bound = {worst:.3f}")


def test_ddim_step_rejects():
    obuf, o = guarded((3, 4, 5), torch.float32)
    d = sr.to_dev(sr.step_inputs(3, 5), DEV)
    tab = torch.from_numpy(sr.step_rows(0.0)[0]).to(DEV)
    for (n, hw, cfg, x_ok) in ((3, 5, 1, True), (0, 5, 0, True), (2, 0, 1, True), (2, 5, 1, False)):      # odd N under CFG, empty sizes, null x
        rc = L().k22_ddim_step(d["x"].data_ptr() if x_ok else None, d["mo"].data_ptr(), None, tab.data_ptr(), sr.STEP_GUIDANCE, cfg, o.data_ptr(), None, n, hw,
                               hp.stream())
        assert rc == _EINVAL and untouched(obuf)


def run_plms(d, tab, N, HW, cfg, order, want_e, want_x0, hist=None):
    need = {0: 0, 4: 1, 1: 1, 2: 2, 3: 3}.get(order, 3) if hist is None else hist
    h = [d[k].data_ptr() if i < need else None for i, k in enumerate(("h1", "h2", "h3"))]
    obuf, o = guarded((N, 4, HW), torch.float32)
    ebuf, e = guarded((N, 4, HW), torch.float32)
    zbuf, z = guarded((N, 4, HW), torch.float32)
    rc = L().k22_plms_step(d["x"].data_ptr(), d["mo"].data_ptr(), h[0], h[1], h[2], order, tab.data_ptr(), sr.STEP_GUIDANCE, cfg, o.data_ptr(),
                           e.data_ptr() if want_e else None, z.data_ptr() if want_x0 else None, N, HW, hp.stream())
    torch.cuda.synchronize()
    return rc, [obuf, ebuf, zbuf]


@pytest.mark.parametrize("N,HW,cfg", sr.STEP_CASES, ids=STEP_IDS)
def test_plms_step(N, HW, cfg):
    worst = 0.0
    d = sr.to_dev(sr.step_inputs(N, HW), DEV)
    for k, row in enumerate(sr.step_rows(0.0)):
        tab = torch.from_numpy(row).to(DEV)
        for order in range(5):
            out, x0, e, b_out, b_x0, b_e = sr.plms_ref(d, row, cfg, order)
            for (want_e, want_x0) in ((True, True), (False, False)):
                obuf, ebuf, zbuf = twice(lambda: run_plms(d, tab, N, HW, cfg, order, want_e, want_x0))
                for name, buf, ref, bound, want in (("x_out", obuf, out, b_out, True), ("e_store", ebuf, e, b_e, want_e), ("x0_out", zbuf, x0, b_x0, want_x0)):
                    if not want:
                        assert untouched(buf), (name, N, HW, cfg, k, order)
                        continue
                    nbad, ratio = check_bounded(buf, ref, bound)
                    worst = max(worst, ratio)
                    assert nbad == 0, (name, N, HW, cfg, k, order, nbad, ratio)
                if want_e and not cfg:                                  # without guidance e_store is the model's eps, bit for bit
                    assert check_exact(ebuf, d["mo"][:, :4].contiguous()) == 0
    print(f"plms_step N={N} HW={HW} cfg={cfg}: largest |out - ref| / bound = {worst:.3f}")


def test_plms_step_rejects():
    d = sr.to_dev(sr.step_inputs(3, 5), DEV)
    tab = torch.from_numpy(sr.step_rows(0.0)[0]).to(DEV)
    for (n, cfg, order, hist) in ((3, 1, 0, 0), (2, 1, 1, 0), (2, 1, 4, 0), (2, 1, 2, 1), (2, 1, 3, 2), (2, 1, 5, 3), (2, 1, -1, 3)):
        rc, bufs = run_plms(d, tab, n, 5, cfg, order, True, True, hist=hist)      # odd N under CFG; an order without its history; no such order
        assert rc == _EINVAL and untouched(*bufs), (n, cfg, order, hist)


def test_zz_total_time():
    """the last test of the module: what its tests took together (the figure recorded in the module docstring)"""
    print(f"test_seam_kernels_gpu: {_SPENT[0]:.1f} s in all tests of the module")
