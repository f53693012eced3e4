"""CPU half of the single-kernel parity of the kernels that open and close a UNet step (tests/seam_ref.py, tests/test_seam_kernels_gpu.py):
 (a) every float64 restatement agrees to 1e-12 with torch's own float64 operator (F.conv2d, F.avg_pool2d, F.interpolate, F.layer_norm,
     F.linear, the reference's timestep_embedding expression, the samplers' update formulas);
 (b) an fp32 CPU emulation of a correct kernel passes the comparator at every GPU case and type; the class-M yardsticks are printed;
 (c) resolving power: every listed deliberately wrong variant must violate the check on the chosen inputs under the u_out of every dtype."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers as hp
import seam_ref as sr

DTYPES = sr.DTYPES
DT_IDS = [sr.DT_NAME[d] for d in DTYPES]


def close(a, b, tol=1e-12):
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


def as_T(ref, dtype):
    """what a correct kernel would store: the reference rounded once to T"""
    return ref.to(hp.tdt(dtype))


def rejected(out, ref_mut, bound_mut):
    return sr.violations(out, ref_mut, bound_mut)[0] > 0


def accepted(out, ref, bound):
    nbad, ratio = sr.violations(out, ref, bound)
    return nbad == 0, ratio


# ---- (a) the restatements against torch's float64 operators -----------------------------------------------------------------------------
def test_a_conv_in_is_conv2d():
    for (B, H, W, Cin, Cout, premul, frac) in sr.conv_in_cases():
        d = sr.to64(sr.conv_in_inputs(B, H, W, Cin, Cout, frac))
        ref, S = sr.conv_in_ref(d, Cin, premul)
        mk = d["mask"].float().double()
        im = d["img"] if premul else (d["img"].float() * d["mask"].float()).double()
        inp = {4: d["x"], 8: torch.cat([d["x"], im], 1), 9: torch.cat([d["x"], im, mk], 1)}[Cin]
        want = F.conv2d(inp, d["w"], d["b"], padding=1).permute(0, 2, 3, 1)
        assert close(ref, want), (B, H, W, Cin, Cout)
        assert bool((S >= ref.abs() - 1e-12).all())
        # the packed weights the kernel reads are the same numbers: row c * 9 + ky * 3 + kx, column o
        wp = sr.pack.pack_stem(d["w"])
        assert wp.shape == (Cin * 9, Cout) and torch.equal(wp[3 * 9 + 1 * 3 + 2], d["w"][:, 3, 1, 2])


def test_a_timestep_embedding_is_the_reference_expression():
    for half in sr.TEMB_HALF:
        d = sr.temb_inputs(5, half, "product")
        # nn.py:113-121: freqs = exp(-log(10000) * arange(half) / half); args = t[:, None] * freqs[None]; cat([cos, sin], -1)
        freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)
        assert torch.equal(d["f"], freqs)
        args = d["t"][:, None].float() * freqs[None]
        assert close(sr.temb_ref(d), torch.cat([torch.cos(args.double()), torch.sin(args.double())], -1))
        assert sr.temb_inputs(5, half, "linear")["f"][-1].item() == 1.0 and d["f"][0].item() == 1.0


def test_a_linear_layernorm_resample():
    for case in sr.LIN_CASES[:10]:
        M, N, K, dx, do, da, add_mod, a_in, a_out, bias = case
        d = sr.lin_inputs(case, sr.F32)
        x = d["x"][:, :K].double()
        v = F.linear(F.silu(x) if a_in else x, d["w"].double(), None if d["b"] is None else d["b"].double())
        v = F.silu(v) if a_out else v
        if d["add"] is not None:
            v = v + torch.stack([d["add"][(m % add_mod) if add_mod else m, :N] for m in range(M)]).double()
        assert close(sr.lin_ref(d, case)[0], v), case
    for D in sr.LN_D:
        d = sr.to64(sr.ln_inputs(D, True))
        assert close(sr.ar.layernorm_ref(d["x"], d["g"], d["b"], sr.LN_EPS)[0], F.layer_norm(d["x"], (D,), d["g"], d["b"], sr.LN_EPS))
    x = sr.rs_input(2, 6, 4, 8, sr.F32).double()
    nchw = x.permute(0, 3, 1, 2)
    assert close(sr.rs_ref(x, 1)[0], F.avg_pool2d(nchw, 2).permute(0, 2, 3, 1))
    assert torch.equal(sr.rs_ref(x, 2)[0], F.interpolate(nchw, scale_factor=2, mode="nearest").permute(0, 2, 3, 1))
    x = sr.rs_input(3, 5, 7, 8, sr.F32).double()                   # odd sizes: AvgPool2d floors, the trailing row / column is ignored
    assert close(sr.rs_ref(x, 1)[0], F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))


def test_a_kv_pack_is_the_concat():
    for (B, H, T, S) in sr.KV_CASES:
        d = sr.kv_inputs(B, H, T, S, sr.F32)
        k, vt = sr.kv_ref(d, B, H, T, S)
        Tkp = sr.kv_tkp(T, S)
        assert k.shape == (B, H, Tkp, 64) and vt.shape == (B, H, 64, Tkp)
        for b in range(B):
            for h in range(H):
                for j in (0, S - 1, S, S + T - 1, Tkp - 1):
                    if j < 0:
                        continue
                    if j < S:
                        row = d["ctxkv"][b * S + j]
                        wk, wv = row[h * 64:(h + 1) * 64], row[64 * H + h * 64:64 * H + (h + 1) * 64]
                    elif j < S + T:
                        row = d["qkv"][b * T + j - S]
                        wk, wv = row[64 * H + h * 64:64 * H + (h + 1) * 64], row[128 * H + h * 64:128 * H + (h + 1) * 64]
                    else:
                        wk = wv = torch.zeros(64)
                    assert torch.equal(k[b, h, j], wk) and torch.equal(vt[b, h, :, j], wv), (B, H, T, S, b, h, j)


def test_a_sampler_steps_are_the_update_formulas():
    """samplers.py:290-331 / 566-637 written out per element in numpy float64"""
    rows = sr.step_rows(1.0)
    d = sr.step_inputs(6, 35)
    g = float(np.float32(sr.STEP_GUIDANCE))
    x, mo, nz = (d[k].double().numpy() for k in ("x", "mo", "noise"))
    h = [d[k].double().numpy() for k in ("h1", "h2", "h3")]
    e = np.empty_like(x)
    for n in range(6):
        e[n] = mo[n % 3 + 3, :4] + g * (mo[n % 3, :4] - mo[n % 3 + 3, :4])
    for row in rows:
        a_t, a_prev, sigma, s1m = (float(v) for v in row)
        x0 = (x - s1m * e) / np.sqrt(a_t)
        want = np.sqrt(a_prev) * x0 + np.sqrt(1 - a_prev - sigma ** 2) * e + sigma * nz
        out, got0, _, _ = sr.ddim_ref(d, row, 1, True)
        assert close(out, torch.from_numpy(want)) and close(got0, torch.from_numpy(x0))
        eps = {0: e, 4: (h[0] + e) / 2, 1: (3 * e - h[0]) / 2, 2: (23 * e - 16 * h[0] + 5 * h[1]) / 12,
               3: (55 * e - 59 * h[0] + 37 * h[1] - 9 * h[2]) / 24}
        for order, ep in eps.items():
            x0 = (x - s1m * ep) / np.sqrt(a_t)
            want = np.sqrt(a_prev) * x0 + np.sqrt(1 - a_prev) * ep
            out, got0, ge, _, _, _ = sr.plms_ref(d, row, 1, order)
            assert close(out, torch.from_numpy(want)) and close(got0, torch.from_numpy(x0)) and close(ge, torch.from_numpy(e)), order
    assert rows.dtype == np.float32 and rows.shape == (3, 4) and bool((rows[:, 2] > 0).all()) and bool((sr.step_rows(0.0)[:, 2] == 0).all())


# ---- (b) an fp32 emulation of a correct kernel passes at every GPU case ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_b_fp32_emulations_are_accepted(dtype):
    T = hp.tdt(dtype)
    for (B, H, W, Cin, Cout, premul, frac) in sr.conv_in_cases():
        d = sr.conv_in_inputs(B, H, W, Cin, Cout, frac)
        ref, S = sr.conv_in_ref(sr.to64(d), Cin, premul)
        ok, r = accepted(sr.conv_in_emul(d, Cin, premul, dtype), ref, sr.conv_in_bound(ref, S, Cin, dtype))
        assert ok, ("conv_in", B, H, W, Cin, Cout, premul, r)
    for case in sr.LIN_CASES:
        d = sr.lin_inputs(case, dtype)
        ref, bound = sr.lin_bound(d, case, dtype)
        ok, r = accepted(sr.lin_emul(d, case), ref, bound)
        assert ok, ("linear_smallm", case, r)
    for (B, H, W, C, mode) in sr.rs_cases(dtype) + ([sr.RS_CAP[1] + (1,), sr.RS_CAP[2] + (2,)] if dtype == sr.BF16 else []):
        x = sr.rs_input(B, H, W, C, dtype)
        if mode == 1:
            ref, S = sr.rs_ref(x.double(), 1)
            emul = F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).to(T)
            ok, r = accepted(emul, ref, sr.rs_bound(ref, S, dtype))
            assert ok, ("resample", B, H, W, C, r)
        else:
            emul = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1).to(T)
            assert sr.exact_violations(emul, sr.rs_ref(x, 2)[0].to(T)) == 0
    for (rows, cols, ldx, ldy) in sr.CAST_CASES:
        x = sr.cast_input(rows, ldx, dtype)
        exp = sr.cast_expected(x, rows, cols, ldy, dtype)
        emul = torch.full_like(exp, sr.NAN)
        for r in range(rows):
            for c in range(cols):
                emul[r, c] = x[r, c].to(T)
        assert torch.equal(sr.bits(emul), sr.bits(exp))
        sp = exp[:, :cols].float()
        if cols > 1:                                                # the special values reached the owned columns: a zero of each sign, the largest value
            assert bool(((sp == 0) & torch.signbit(sp)).any()) and bool(((sp == 0) & ~torch.signbit(sp)).any())
            assert bool((sp == torch.finfo(T).max).any()) and bool(torch.isfinite(sp).all())
    for (B, H, Tq, S) in sr.KV_CASES:
        d = sr.kv_inputs(B, H, Tq, S, dtype)
        k, vt = sr.kv_ref(d, B, H, Tq, S)
        assert sr.exact_violations(k.to(T), k.to(T)) == 0 and sr.exact_violations(vt.to(T), vt.to(T)) == 0
    for (N, HW, cfg) in sr.STEP_CASES:
        d = sr.step_inputs(N, HW)
        for eta, noise in ((0.0, False), (1.0, True)):
            for row in sr.step_rows(eta):
                out, x0, b_out, b_x0 = sr.ddim_ref(d, row, cfg, noise)
                o32, x32, _, _ = sr.ddim_ref(d, row, cfg, noise, dtype=torch.float32)
                assert accepted(o32, out, b_out)[0] and accepted(x32, x0, b_x0)[0], ("ddim", N, HW, cfg, eta)
        for row in sr.step_rows(0.0):
            for order in range(5):
                out, x0, e, b_out, b_x0, b_e = sr.plms_ref(d, row, cfg, order)
                o32, x32, e32, _, _, _ = sr.plms_ref(d, row, cfg, order, dtype=torch.float32)
                assert accepted(o32, out, b_out)[0] and accepted(x32, x0, b_x0)[0] and accepted(e32, e, b_e)[0], ("plms", N, HW, cfg, order)


def test_b_class_m_yardsticks():
    """prints the CPU yardsticks recorded in seam_ref's docstring; torch's own fp32 evaluation (the emulation of these two kernels) is under c"""
    for half in sr.TEMB_HALF:
        worst = 0.0
        for rows in sr.TEMB_ROWS:
            for table in sr.TEMB_TABLES:
                d = sr.temb_inputs(rows, half, table)
                ref = sr.temb_ref(d)
                v32 = sr.temb_torch32(d)
                worst = max(worst, sr.plain_ratio(v32, ref, torch.ones_like(ref)))
                assert accepted(v32, ref, sr.temb_bound(ref))[0], (rows, half, table)
        print(f"timestep_embedding yardstick (CPU) half={half}: {worst:.3f} (c = {sr.SEAM_C['timestep_embedding']})")
        assert worst < sr.SEAM_C["timestep_embedding"]
    for offset in (False, True):
        for D in sr.LN_D:
            d = sr.ln_inputs(D, offset)
            ref, S = sr.ar.layernorm_ref(d["x"].double(), d["g"].double(), d["b"].double(), sr.LN_EPS)
            v32 = F.layer_norm(d["x"], (D,), d["g"], d["b"], sr.LN_EPS)
            y = sr.plain_ratio(v32, ref, S)
            print(f"layernorm_f32 yardstick (CPU) 7 x {D} {'mean = 10 sd' if offset else 'random'}: {y:.3f} (c = {sr.SEAM_C['layernorm']:.3f})")
            assert y < sr.SEAM_C["layernorm"]
            for rows in sr.LN_ROWS:
                assert accepted(v32[:rows], ref[:rows], sr.ln_bound(ref[:rows], S[:rows]))[0], (rows, D, offset)


# ---- (c) resolving power ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_c_stem_and_embedding_mutations_are_rejected(dtype):
    for (B, H, W, Cin, Cout, premul, frac) in sr.conv_in_cases():
        d = sr.to64(sr.conv_in_inputs(B, H, W, Cin, Cout, frac))
        ref, S = sr.conv_in_ref(d, Cin, premul)
        good = as_T(ref, dtype)
        assert not rejected(good, ref, sr.conv_in_bound(ref, S, Cin, dtype))
        muts = (["last_col_dropped"] if W % 8 else []) + (["mask_not_applied"] if Cin == 9 and not premul else []) + (["ch8_from_img"] if Cin == 9 else [])
        for mut in muts:
            mref, mS = sr.conv_in_ref(d, Cin, premul, mut)
            assert rejected(good, mref, sr.conv_in_bound(mref, mS, Cin, dtype)), (B, H, W, Cin, Cout, premul, frac, mut)
    assert {m for c in sr.conv_in_cases() for m in ((["last_col_dropped"] if c[2] % 8 else []) + (["mask_not_applied"] if c[3] == 9 and not c[5] else []))} == \
        {"last_col_dropped", "mask_not_applied"}
    # timestep_embedding (fp32 output whatever the engine's type)
    for half in sr.TEMB_HALF:
        for table in sr.TEMB_TABLES:
            d = sr.temb_inputs(5, half, table)
            ref = sr.temb_ref(d)
            good = ref.float()
            assert not rejected(good, ref, sr.temb_bound(ref))
            m = sr.temb_ref(d, "sin_cos")
            assert rejected(good, m, sr.temb_bound(m)), (half, table)
            # the argument formed in float64: told apart on the row t = 999 alone
            m = sr.temb_ref(d, "arg_f64")
            assert sr.violations(good[4:5], m[4:5], sr.temb_bound(m[4:5]))[0] > 0, (half, table)
            assert d["t"][4].item() == 999.0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_c_linear_smallm_mutations_are_rejected(dtype):
    seen = set()
    for case in sr.LIN_CASES:
        M, N, K, dx, do, da, add_mod, a_in, a_out, bias = case
        d = sr.lin_inputs(case, dtype)
        ref, bound = sr.lin_bound(d, case, dtype)
        good = ref.float()
        assert not rejected(good, ref, bound), case
        muts = ["last_chunk_dropped", "last_row_unwritten"]
        muts += ["add_row_m"] if (da is not None and add_mod and M > add_mod) else []
        muts += ["no_silu_in"] if a_in else []
        muts += ["no_silu_out"] if a_out else []
        for mut in muts:
            mref = sr.lin_ref(d, case, mut)[0]
            assert rejected(good, mref, bound), (case, mut)       # the mutant's reference under the right operation's bound
            seen.add(mut)
        if M not in (1, 2, 4, 8):
            seen.add("padded_template_row")
    assert seen == {"last_chunk_dropped", "last_row_unwritten", "add_row_m", "no_silu_in", "no_silu_out", "padded_template_row"}


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_c_movers_mutations_are_rejected(dtype):
    T = hp.tdt(dtype)
    for (B, H, W, C, mode) in sr.rs_cases(dtype):
        x = sr.rs_input(B, H, W, C, dtype)
        if mode == 1:
            ref, S = sr.rs_ref(x.double(), 1)
            mref, mS = sr.rs_ref(x.double(), 1, "three_taps")
            assert rejected(as_T(ref, dtype), mref, sr.rs_bound(mref, mS, dtype)), (B, H, W, C)
        else:
            assert sr.exact_violations(sr.rs_ref(x, 2)[0].to(T), sr.rs_ref(x, 2, "nearest_round_up")[0].to(T)) > 0, (B, H, W, C)
    for (rows, cols, ldx, ldy) in sr.CAST_CASES:
        x = sr.cast_input(rows, ldx, dtype)
        if rows > 1:
            assert not torch.equal(sr.bits(sr.cast_expected(x, rows, cols, ldy, dtype)), sr.bits(sr.cast_expected(x, rows, cols, ldy, dtype, "stride_swapped")))
    d = sr.ln_inputs(300, False)
    ref, S = sr.ar.layernorm_ref(d["x"].double(), d["g"].double(), d["b"].double(), sr.LN_EPS)
    mref, mS = sr.ar.layernorm_ref(d["x"].double(), d["g"].double(), d["b"].double(), sr.LN_EPS, "gain_shift")
    assert rejected(ref.float(), mref, sr.ln_bound(mref, mS))
    for (B, H, Tq, S) in sr.KV_CASES:
        d = sr.kv_inputs(B, H, Tq, S, dtype)
        k, vt = (t.to(T) for t in sr.kv_ref(d, B, H, Tq, S))
        muts = ["v_not_transposed"] + (["pad_not_zeroed"] if sr.kv_tkp(Tq, S) > S + Tq else []) + (["ctx_self_swapped"] if S else [])
        for mut in muts:
            mk, mvt = (t.to(T) for t in sr.kv_ref(d, B, H, Tq, S, mut))
            assert sr.exact_violations(vt, mvt) > 0, (B, H, Tq, S, mut)
            if mut != "v_not_transposed":
                assert sr.exact_violations(k, mk) > 0, (B, H, Tq, S, mut)


def test_c_sampler_mutations_are_rejected():
    for (N, HW, cfg) in sr.STEP_CASES[:3]:
        d = sr.step_inputs(N, HW)
        for row in sr.step_rows(1.0):
            out, x0, b_out, b_x0 = sr.ddim_ref(d, row, cfg, True)
            for mut in (["eps_row_n"] if cfg else []) + ["noise_dropped"]:
                mo, m0, mb, mb0 = sr.ddim_ref(d, row, cfg, True, mut)
                assert rejected(out.float(), mo, mb), (N, HW, mut)
                if mut == "eps_row_n":
                    assert rejected(x0.float(), m0, mb0), (N, HW, mut)
        for row in sr.step_rows(0.0):
            for order in range(5):
                out, x0, e, b_out, b_x0, b_e = sr.plms_ref(d, row, cfg, order)
                mo, m0, _, mb, mb0, _ = sr.plms_ref(d, row, cfg, order, "order_swapped")
                assert rejected(out.float(), mo, mb) and rejected(x0.float(), m0, mb0), (N, HW, order)
