"""Single-kernel float64 parity of the MoVQ, encoder and prior helper kernels (csrc/movq_kernels.hip, csrc/encoder.hip, csrc/prior.hip)
through their C entry points (include/k22.h: "single-kernel entry points for the parity tests"), which run the engines' own launchers.
References, inputs, bound classes (E exact / D derived / M measured constant) and the measured yardsticks: tests/aux_ref.py.

Every output buffer is pre-filled with NaN (0xA5 for uint8) and carries guard elements in front and behind: every element a launch owns is
checked, every other one must still hold the fill.  The class-M tests print torch's own fp32 yardstick on this device and assert it under c."""
import pytest
import torch

import aux_ref as ar
import helpers as hp
from kandinsky2_amd import _lib

pytestmark = pytest.mark.gpu
DTYPES = ar.DTYPES
DT_IDS = [ar.DT_NAME[d] for d in DTYPES]
DEV = "cuda"
GUARD = 256          # elements of fill on both sides of every output (a multiple of 16 bytes in every type)


def L():
    return _lib.lib()


def guarded(shape, T, fill=ar.NAN, guard=GUARD):
    """(whole buffer, view of `shape` inside it with `guard` fill elements on both sides)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * guard,), fill, dtype=T, device=DEV)
    return buf, buf[guard:guard + n].view(*shape)


_EINVAL = -1   # include/k22.h: K22_EINVAL


def sync():
    torch.cuda.synchronize()


def check_bounded(buf, ref, bound, guard=GUARD):
    """ref / bound over the owned view; the guards must hold NaN"""
    nbad, ratio = ar.violations(buf, ar.with_guard(ref, guard), ar.with_guard(bound, guard, 0.0))
    return nbad, ratio


def check_exact(buf, exp, guard=GUARD, fill=ar.NAN):
    return ar.exact_violations(buf, ar.with_guard(exp, guard, fill))


# ---- MoVQ ---------------------------------------------------------------------------------------------------------------------------
def run_spatialnorm(d, shift, pad, act, dtype, C=None, W=None):
    T = hp.tdt(dtype)
    x = d["x"].to(T).contiguous()
    B, H, W_, C_ = x.shape
    buf, out = guarded((B, H + 2 * pad, W_ + 2 * pad, C_), T)
    rc = L().k22_spatialnorm_apply(x.data_ptr(), d["coeff"].data_ptr(), d["zq"].data_ptr(), d["wy"].data_ptr(), d["by"].data_ptr(),
                                   d["wb"].data_ptr(), d["bb"].data_ptr(), out.data_ptr(), B, H, W_ if W is None else W, C_ if C is None else C,
                                   ar.SN_H0, ar.SN_W0, shift, act, pad, dtype, hp.stream())
    sync()
    return rc, buf


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_spatialnorm_apply(dtype):
    worst = 0.0
    for C in (128, 512):
        for shift in range(5):
            d = ar.to_dev(ar.spatialnorm_inputs(C, shift, dtype), DEV)
            d64 = ar.to64(d)
            for pad in (0, 1):
                pre, S = ar.spatialnorm_ref(d64, shift, pad, 0)
                for act in (0, 1):
                    ref, bound = ar.spatialnorm_bound(pre, S, act, dtype)
                    rc, buf = run_spatialnorm(d, shift, pad, act, dtype)
                    assert rc == 0, _lib.lib().k22_last_error()
                    nbad, ratio = check_bounded(buf, ref, bound)
                    worst = max(worst, ratio)
                    assert nbad == 0, (C, shift, pad, act, nbad, ratio)
                    if pad:                                    # E: the zero border, exactly
                        o = buf[GUARD:-GUARD].view(ref.shape)
                        border = torch.ones(ref.shape[1:3], dtype=torch.bool, device=DEV)
                        border[1:-1, 1:-1] = False
                        assert torch.equal(o[:, border], torch.zeros_like(o[:, border])), (C, shift, act)
    print(f"spatialnorm_apply {ar.DT_NAME[dtype]}: largest |out - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_spatialnorm_apply_rejects(dtype):
    d = ar.to_dev(ar.spatialnorm_inputs(128, 2, dtype), DEV)
    rc, buf = run_spatialnorm(d, 2, 1, 0, dtype, W=(ar.SN_W0 << 2) - 2)        # W no multiple of 2^shift
    assert rc == _EINVAL and bool(torch.isnan(buf).all())
    rc, buf = run_spatialnorm(d, 2, 1, 0, dtype, C=124 if dtype != ar.F32 else 126)   # C % 8 (16-bit) / % 4 (fp32)
    assert rc == _EINVAL and bool(torch.isnan(buf).all())


def run_nhwc(name, x, out_shape, dtype, H=None, W=None, C=None):
    T = hp.tdt(dtype)
    xt = x.to(T).contiguous()
    B, H_, W_, C_ = xt.shape
    buf, out = guarded(out_shape, T)
    rc = getattr(L(), "k22_" + name)(xt.data_ptr(), out.data_ptr(), B, H_ if H is None else H, W_ if W is None else W, C_ if C is None else C,
                                     dtype, hp.stream())
    sync()
    return rc, buf


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", ["upsample2_pad", "pad_copy", "subsample_odd"])
def test_nhwc_movers_exact(name, dtype):
    T = hp.tdt(dtype)
    fn = {"upsample2_pad": ar.upsample2_pad_ref, "pad_copy": ar.pad_copy_ref, "subsample_odd": ar.subsample_odd_ref}[name]
    for (C, H, W) in ar.nhwc_cases(dtype, sub=name == "subsample_odd"):
        x = ar.nhwc_input(C, H, W, dtype).to(DEV)
        exp = fn(x).to(T)
        rc, buf = run_nhwc(name, x, exp.shape, dtype)
        assert rc == 0, _lib.lib().k22_last_error()
        assert check_exact(buf, exp) == 0, (name, C, H, W)
    # rejections: channel alignment; odd sizes (subsample_odd)
    x = ar.nhwc_input(128, 6, 10, dtype).to(DEV)
    rc, buf = run_nhwc(name, x, (2, 14, 22, 128), dtype, C=128 - ar.epv(dtype) // 2)
    assert rc == _EINVAL and bool(torch.isnan(buf).all())
    if name == "subsample_odd":
        for kw in ({"H": 5}, {"W": 9}):
            rc, buf = run_nhwc(name, x, (2, 3, 5, 128), dtype, **kw)
            assert rc == _EINVAL and bool(torch.isnan(buf).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_softmax_rows(dtype):
    T = hp.tdt(dtype)
    c = ar.AUX_C["softmax"]
    worst = 0.0
    for Lr in ar.SOFTMAX_L:
        for scale in ar.SOFTMAX_SCALES:
            x = ar.softmax_input(Lr, scale, dtype).to(DEV)
            ref, S = ar.softmax_ref(x.double(), scale)
            yard = ar.plain_ratio(torch.softmax(x.float() * scale, -1), ref, S)
            print(f"softmax_rows {ar.DT_NAME[dtype]} L={Lr} scale={scale:.4f}: torch fp32 yardstick {yard:.3f} (c = {c})")
            assert yard < c
            # the launch gets rows 1..5 of 7: the rows before and after it must stay as they were
            buf = torch.full((ar.SOFTMAX_ROWS + 2, Lr), 0.5, dtype=T, device=DEV)
            buf[1:-1] = x.to(T)
            rc = L().k22_softmax_rows(buf[1].data_ptr(), ar.SOFTMAX_ROWS, Lr, scale, dtype, hp.stream())
            sync()
            assert rc == 0, _lib.lib().k22_last_error()
            assert bool((buf[0] == 0.5).all()) and bool((buf[-1] == 0.5).all())
            out = buf[1:-1]
            assert bool(torch.isfinite(out).all())
            nbad, ratio = ar.violations(out, ref, c * ar.U24 * S + ar.rounding(ref, dtype))
            worst = max(worst, ratio)
            assert nbad == 0, (Lr, scale, nbad, ratio)
            assert bool(((out.double().sum(-1) - 1.0).abs() <= 2 * ar.u_out(dtype) + c * ar.U24 * Lr).all())
    rc = L().k22_softmax_rows(buf.data_ptr(), 1, 12 if dtype != ar.F32 else 6, 1.0, dtype, hp.stream())
    assert rc == _EINVAL
    print(f"softmax_rows {ar.DT_NAME[dtype]}: largest |out - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_movq_prepare(dtype):
    T = hp.tdt(dtype)
    for (h, w) in ar.PREP_HW:
        d = ar.to_dev(ar.movq_prepare_inputs(h, w), DEV)
        ref, S, zq_exp = ar.movq_prepare_ref(ar.to64(d))
        B = d["z"].shape[0]
        zbuf, zq = guarded((B, h, w, 4), torch.float32)
        xbuf, xin = guarded((B, h + 2, w + 2, ar.CPAD), T)
        rc = L().k22_movq_prepare(d["z"].data_ptr(), d["w"].data_ptr(), d["b"].data_ptr(), zq.data_ptr(), xin.data_ptr(), B, h, w, ar.CPAD,
                                  dtype, hp.stream())
        sync()
        assert rc == 0, _lib.lib().k22_last_error()
        assert check_exact(zbuf, zq_exp.float()) == 0, (h, w)                      # E: the zq copy
        nbad, ratio = check_bounded(xbuf, ref, 16 * ar.U24 * S + ar.rounding(ref, dtype))   # D, n = 16
        assert nbad == 0, (h, w, nbad, ratio)
        owned = torch.zeros(h + 2, w + 2, ar.CPAD, dtype=torch.bool, device=DEV)
        owned[1:-1, 1:-1, :4] = True
        assert bool((xin[:, ~owned] == 0).all()), (h, w)                          # E: zero channels 4.. and zero border


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_movq_enc_prepare_exact(dtype):
    T = hp.tdt(dtype)
    for (h, w) in ar.PREP_HW:
        img = ar.acts(ar.gen(450 + h), 2, 3, h, w).to(DEV)
        exp = ar.movq_enc_prepare_ref(img, dtype)
        buf, xin = guarded(exp.shape, T)
        rc = L().k22_movq_enc_prepare(img.data_ptr(), xin.data_ptr(), 2, h, w, ar.CPAD, dtype, hp.stream())
        sync()
        assert rc == 0, _lib.lib().k22_last_error()
        assert check_exact(buf, exp) == 0, (h, w)


def test_movq_quant_conv():
    for HW in ar.QUANT_HW:
        d = ar.to_dev(ar.quant_conv_inputs(HW), DEV)
        ref, S = ar.quant_conv_ref(ar.to64(d))
        buf, out = guarded(ref.shape, torch.float32)
        rc = L().k22_movq_quant_conv(d["h"].data_ptr(), d["w"].data_ptr(), d["b"].data_ptr(), out.data_ptr(), 2, HW, hp.stream())
        sync()
        assert rc == 0, _lib.lib().k22_last_error()
        nbad, ratio = check_bounded(buf, ref, 16 * ar.U24 * S + ar.U24 * ref.abs())
        assert nbad == 0, (HW, nbad, ratio)


def test_to_uint8_nhwc_exact():
    for (H, W) in ar.U8_HW:
        x = ar.to_uint8_input(H, W).to(DEV)
        exp = ar.to_uint8_ref(x)                                                 # torch's fp32 evaluation on this device
        buf, out = guarded(exp.shape, torch.uint8, fill=0xA5)
        rc = L().k22_to_uint8_nhwc(x.data_ptr(), out.data_ptr(), 2, 3, H, W, hp.stream())
        sync()
        assert rc == 0, _lib.lib().k22_last_error()
        assert check_exact(buf, exp, fill=0xA5) == 0, (H, W)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------
def ln_check(kind, D, ld_mult, mode, dtype, offset=False):
    """mode: 'inplace' (fp32 output aliasing x), 'T' (T output only), 'both'; prior: 'f32' / 'T'.  -> (yardstick, worst ratio)"""
    T = hp.tdt(dtype)
    c = ar.AUX_C["layernorm"]
    d = ar.to_dev(ar.layernorm_inputs(D, ld_mult, offset), DEV)
    ldx, R = ld_mult * D, ar.LN_ROWS
    eps = 1e-5
    xs = d["x"][1:1 + R, :D]
    ref, S = ar.layernorm_ref(xs.double(), d["g"].double(), d["b"].double(), eps)
    yard = ar.plain_ratio(torch.nn.functional.layer_norm(xs, (D,), d["g"], d["b"], eps), ref, S)
    assert yard < c, (kind, D, yard)
    assert bool(torch.isfinite(ref).all())
    xbuf = d["x"].clone()
    tbuf, tout = guarded((R, D), torch.float32 if mode == "f32" else T)
    if kind == "enc":
        f_ptr = xbuf[1].data_ptr() if mode in ("inplace", "both") else None
        t_ptr = tout.data_ptr() if mode in ("T", "both") else None
        rc = L().k22_enc_layernorm(xbuf[1].data_ptr(), ldx, d["g"].data_ptr(), d["b"].data_ptr(), f_ptr, ldx, t_ptr, R, D, eps, dtype, hp.stream())
    else:
        rc = L().k22_prior_layernorm(xbuf[1].data_ptr(), ldx, d["g"].data_ptr(), d["b"].data_ptr(), tout.data_ptr(), R, D, 1 if mode == "f32" else 0,
                                     dtype, hp.stream())
    sync()
    assert rc == 0, _lib.lib().k22_last_error()
    worst = 0.0
    if kind == "enc" and mode in ("inplace", "both"):
        # fp32 rows written over x: columns >= D of the launched rows and the rows around them keep x
        exp_ref = d["x"].double().clone(); exp_bound = torch.zeros_like(exp_ref)
        exp_ref[1:1 + R, :D] = ref
        exp_bound[1:1 + R, :D] = c * ar.U24 * S + ar.U24 * ref.abs()
        nbad, ratio = ar.violations(xbuf, exp_ref, exp_bound)
        worst = max(worst, ratio)
        assert nbad == 0, (kind, D, ld_mult, mode, nbad, ratio)
    else:
        assert torch.equal(xbuf, d["x"])
    if mode in ("T", "both", "f32"):
        rnd = ar.U24 * ref.abs() if mode == "f32" else ar.rounding(ref, dtype)
        nbad, ratio = check_bounded(tbuf, ref, c * ar.U24 * S + rnd)
        worst = max(worst, ratio)
        assert nbad == 0, (kind, D, ld_mult, mode, nbad, ratio)
    else:
        assert bool(torch.isnan(tbuf).all())
    return yard, worst


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_enc_layernorm(dtype):
    for D in ar.ENC_LN_D:
        ys = []
        for ld_mult in (1, 3):
            for mode in ("inplace", "T", "both"):
                ys.append(ln_check("enc", D, ld_mult, mode, dtype))
        ys.append(ln_check("enc", D, 1, "both", dtype, offset=True))
        print(f"enc_layernorm {ar.DT_NAME[dtype]} {ar.LN_ROWS} x {D}: torch fp32 yardstick {max(y for y, _ in ys):.3f} (offset rows {ys[-1][0]:.3f}; "
              f"c = {ar.AUX_C['layernorm']}), largest |out - ref| / bound = {max(w for _, w in ys):.3f}")
    x = torch.zeros(2, 2112, device=DEV)
    assert L().k22_enc_layernorm(x.data_ptr(), 2112, x.data_ptr(), x.data_ptr(), x.data_ptr(), 2112, None, 1, 2112, 1e-5, dtype, hp.stream()) == _EINVAL


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_prior_layernorm(dtype):
    for D in ar.PRIOR_LN_D:
        ys = []
        for ld_mult in (1, 3):
            for mode in ("f32", "T"):
                ys.append(ln_check("prior", D, ld_mult, mode, dtype))
        ys.append(ln_check("prior", D, 1, "T", dtype, offset=True))
        print(f"prior_layernorm {ar.DT_NAME[dtype]} {ar.LN_ROWS} x {D}: torch fp32 yardstick {max(y for y, _ in ys):.3f} (offset rows {ys[-1][0]:.3f}; "
              f"c = {ar.AUX_C['layernorm']}), largest |out - ref| / bound = {max(w for _, w in ys):.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_layernorm_entries_are_one_kernel(dtype):
    """k22_prior_layernorm is an argument mapping onto the kernel k22_enc_layernorm launches (strides, eps = 1e-5, which output): equal bits"""
    T, R = hp.tdt(dtype), ar.LN_ROWS
    for D in ar.PRIOR_LN_D:
        for ld_mult in (1, 3):
            d = ar.to_dev(ar.layernorm_inputs(D, ld_mult), DEV)
            ldx = ld_mult * D
            x, g, b = d["x"].clone(), d["g"], d["b"]
            for to_f32 in (0, 1):
                TO = torch.float32 if to_f32 else T
                pbuf, pout = guarded((R, D), TO)
                ebuf, eout = guarded((R, D), TO)
                assert L().k22_prior_layernorm(x[1].data_ptr(), ldx, g.data_ptr(), b.data_ptr(), pout.data_ptr(), R, D, to_f32, dtype, hp.stream()) == 0
                f_ptr, t_ptr = (eout.data_ptr(), None) if to_f32 else (None, eout.data_ptr())
                assert L().k22_enc_layernorm(x[1].data_ptr(), ldx, g.data_ptr(), b.data_ptr(), f_ptr, D, t_ptr, R, D, 1e-5, dtype, hp.stream()) == 0
                sync()
                assert torch.equal(x, d["x"]), (D, ld_mult, to_f32)
                assert bool(torch.isfinite(pout.float()).all()), (D, ld_mult, to_f32)
                assert check_exact(pbuf, eout) == 0, (D, ld_mult, to_f32)       # the prior entry's bits and its guards
                assert check_exact(ebuf, pout) == 0, (D, ld_mult, to_f32)       # the encoder entry's guards


def test_prior_layernorm_width_is_bounded():
    """the shared kernel holds 8 x 256 values of a row: the prior's entry and its plan refuse anything wider, as the towers' do"""
    import ctypes as C
    from kandinsky2_amd import prior as kp
    x = torch.zeros(2, 2112, device=DEV)
    for dtype in DTYPES:
        assert L().k22_prior_layernorm(x.data_ptr(), 2112, x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 2112, 1, dtype, hp.stream()) == _EINVAL
        assert b"2048" in L().k22_last_error()
    wide = _lib.K22PriorConfig(dtype=_lib.K22_BF16, text_ctx=77, xf_width=2112, xf_layers=4, xf_heads=33, xf_final_ln=1, clip_dim=768, clip_xf_width=768)
    h, n = C.c_void_p(), C.c_size_t()
    assert L().k22_prior_create(C.byref(wide), None, 0, C.byref(h)) == 0
    try:
        assert L().k22_prior_plan(h, 2, C.byref(n)) == _EINVAL
        assert b"2048" in L().k22_last_error()
    finally:
        L().k22_prior_destroy(h)
    # the configuration is fixed at create: the tiny one is its own handle, refused for its batch first (a refusal leaves a handle usable)
    m = kp.PriorDiffusionModelHIP(kp.tiny_prior_hparams(), backend_dtype=torch.bfloat16).to(DEV).prepare()
    e = m._engines["prior"]
    assert L().k22_prior_plan(e.handle, 9, C.byref(n)) == _EINVAL
    e.plan(2)
    assert e.plan_key == (2,) and e.ws is not None


# ---- encoder helpers ----------------------------------------------------------------------------------------------------------------
def test_enc_embed_exact():
    for (name, D, xlmr, max_pos, tok) in ar.embed_cases():
        w = ar.to_dev(ar.embed_weights(D), DEV)
        tok = tok.to(DEV)
        exp = ar.embed_ref(tok, w, xlmr, max_pos)
        B, n = tok.shape
        buf, out = guarded(exp.shape, torch.float32)
        rc = L().k22_enc_embed(tok.data_ptr(), w["te"].data_ptr(), w["pe"].data_ptr(), w["ty"].data_ptr() if xlmr else None, out.data_ptr(),
                               B, n, D, ar.EMBED_VOCAB, xlmr, ar.EMBED_PAD, max_pos, hp.stream())
        sync()
        assert rc == 0, _lib.lib().k22_last_error()
        assert check_exact(buf, exp) == 0, name


def test_enc_gather_eot_exact():
    tok = ar.eot_tokens().to(DEV)
    for D in (64, 300):
        x = ar.acts(ar.gen(825 + D), tok.shape[0], tok.shape[1], D).to(DEV)
        exp = ar.gather_eot_ref(tok, x)
        buf, out = guarded(exp.shape, torch.float32)
        rc = L().k22_enc_gather_eot(tok.data_ptr(), x.data_ptr(), out.data_ptr(), tok.shape[0], tok.shape[1], D, hp.stream())
        sync()
        assert rc == 0, _lib.lib().k22_last_error()
        assert check_exact(buf, exp) == 0, D


def test_enc_masked_mean():
    for D in (72, 1024):
        d = ar.to_dev(ar.masked_mean_inputs(D), DEV)
        ref, S = ar.masked_mean_ref(ar.to64(d))
        B, n = d["mask"].shape
        buf, out = guarded(ref.shape, torch.float32)
        rc = L().k22_enc_masked_mean(d["x"].data_ptr(), d["mask"].data_ptr(), out.data_ptr(), B, n, D, hp.stream())
        sync()
        assert rc == 0, _lib.lib().k22_last_error()
        nbad, ratio = check_bounded(buf, ref, 2 * (n + 2) * ar.U24 * S + ar.U24 * ref.abs())
        assert nbad == 0, (D, nbad, ratio)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_enc_patchify_exact(dtype):
    T = hp.tdt(dtype)
    for (S, patch) in ar.PATCH_CASES:
        img = ar.patch_image(S).to(DEV)
        exp = ar.patchify_ref(img, patch, dtype)
        buf, out = guarded(exp.shape, T)
        rc = L().k22_enc_patchify(img.data_ptr(), out.data_ptr(), 2, S, patch, exp.shape[1], dtype, hp.stream())
        sync()
        assert rc == 0, _lib.lib().k22_last_error()
        assert check_exact(buf, exp) == 0, (S, patch)
        K = 3 * patch * patch
        assert bool((out[:, K:] == 0).all())


def test_enc_vision_assemble_exact():
    for P in (4, 16):
        d = ar.to_dev(ar.assemble_inputs(P), DEV)
        exp = ar.assemble_ref(d)
        buf, out = guarded(exp.shape, torch.float32)
        rc = L().k22_enc_vision_assemble(d["patch"].data_ptr(), d["cls"].data_ptr(), d["pos"].data_ptr(), out.data_ptr(), 2, P, 64, hp.stream())
        sync()
        assert rc == 0, _lib.lib().k22_last_error()
        assert check_exact(buf, exp) == 0, P


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("exact", [0, 1], ids=["quickgelu", "erf"])
def test_enc_mlp_act(exact, dtype):
    T = hp.tdt(dtype)
    for n in ar.MLP_N:
        x = ar.mlp_act_input(n).to(DEV)
        ref, bound = ar.mlp_act_bound(x, exact, dtype)
        assert bool(torch.isfinite(ref).all())
        buf, out = guarded((n,), T)
        rc = L().k22_enc_mlp_act(x.data_ptr(), out.data_ptr(), n, exact, dtype, hp.stream())
        sync()
        assert rc == 0, _lib.lib().k22_last_error()
        nbad, ratio = check_bounded(buf, ref, bound)
        print(f"enc_mlp_act {'erf' if exact else 'quickgelu'} {ar.DT_NAME[dtype]} n={n}: largest |out - ref| / bound = {ratio:.3f}")
        assert nbad == 0, (n, nbad, ratio)
        assert bool(torch.isfinite(out).all())


def run_attention(qkv, hd, n, dtype):
    T = hp.tdt(dtype)
    B, D = qkv.shape[0], ar.ATT_HEADS * hd
    q = qkv.to(T).contiguous()
    buf, out = guarded((B, n, D), T, guard=16 * D)          # more than the 15 unused query slots of the last workgroup
    rc = L().k22_enc_attention_generic(q.data_ptr(), out.data_ptr(), B, ar.ATT_HEADS, n, hd, dtype, hp.stream())
    sync()
    return rc, buf


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("hd,n", ar.ATT_CASES)
def test_enc_attention_generic(hd, n, dtype):
    c = ar.AUX_C["attention"]
    D = ar.ATT_HEADS * hd
    for spike in [None] + ar.att_spikes(n):
        qkv = ar.attention_input(hd, n, dtype, spike).to(DEV)
        ref, S = ar.attention_ref(qkv.double(), hd)
        ref32, _ = ar.attention_ref(qkv.float(), hd)
        yard = ar.plain_ratio(ref32, ref, S)
        print(f"enc_attention_generic {ar.DT_NAME[dtype]} hd={hd} n={n} spike={spike}: torch fp32 yardstick {yard:.3f} (c = {c})")
        assert yard < c
        bound = c * ar.U24 * S + ar.rounding(ref, dtype)
        rc, buf = run_attention(qkv, hd, n, dtype)
        assert rc == 0, _lib.lib().k22_last_error()
        nbad, ratio = check_bounded(buf, ref, bound, guard=16 * D)
        print(f"    largest |out - ref| / bound = {ratio:.3f}")
        assert nbad == 0, (hd, n, spike, nbad, ratio)
        out = buf[16 * D:-16 * D].view(ref.shape)
        assert bool(torch.isfinite(out).all())
        if spike is not None:                                  # every output row is the spike key's V row
            vrow = qkv[:, spike, 2 * D:].double()[:, None, :].expand_as(ref)
            assert bool(((out.double() - vrow).abs() <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_enc_attention_generic_admission(dtype):
    """the rule of K22Encoder::plan: hd <= 128, n <= 512, n * (hd + 2) * 4 bytes + 10 KB of LDS <= 160 KB (the same figure for all three types)"""
    for (hd, n) in ((129, 16), (64, 513), (128, 512), (104, 400)):
        qkv = torch.zeros(1, n, 3 * ar.ATT_HEADS * hd, device=DEV)
        rc, buf = run_attention(qkv, hd, n, dtype)
        assert rc == _EINVAL, (hd, n)
        assert bool(torch.isnan(buf).all())


# ---- prior ----------------------------------------------------------------------------------------------------------------------------
def test_prior_finish_input_exact():
    d = ar.to_dev(ar.finish_inputs(), DEV)
    exp = ar.finish_ref(d)
    buf, out = guarded(exp.shape, torch.float32)
    out.copy_(d["inp"])
    B, n, D = exp.shape
    rc = L().k22_prior_finish_input(out.data_ptr(), d["pos"].data_ptr(), d["prd"].data_ptr(), B, n, D, hp.stream())
    sync()
    assert rc == 0, _lib.lib().k22_last_error()
    assert check_exact(buf, exp) == 0


def test_prior_sampler_step():
    for (bs, D, nz) in ar.SAMPLER_CASES:
        d = ar.to_dev(ar.sampler_inputs(bs, D, nz), DEV)
        ref, S, e_act = ar.sampler_ref(ar.to64(d))
        assert 0 < int((ref != ar.sampler_ref(ar.to64(d), "no_clamp")[0]).sum()) < ref.numel()     # the clamp bites on some elements
        buf, out = guarded(ref.shape, torch.float32)
        rc = L().k22_prior_sampler_step(d["x"].data_ptr(), d["mo"].data_ptr(), d["noise"].data_ptr(), d["scales"].data_ptr(), d["tab"].data_ptr(),
                                        ar.SAMPLER_CLAMP, out.data_ptr(), bs, D, hp.stream())
        sync()
        assert rc == 0, _lib.lib().k22_last_error()
        nbad, ratio = check_bounded(buf, ref, ar.SAMPLER_N * ar.U24 * S + ar.U24 * ref.abs() + e_act)
        assert nbad == 0, (bs, D, nz, nbad, ratio)
