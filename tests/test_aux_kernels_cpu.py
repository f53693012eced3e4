"""CPU half of the single-kernel parity of the MoVQ, encoder and prior helpers (tests/aux_ref.py, tests/test_aux_kernels_gpu.py):
 (a) every float64 restatement agrees to 1e-12 with an independent composition (the oracle's functions, torch.nn.functional);
 (b) torch's CPU fp32 evaluation of every class-D and class-M case stays inside its bound with the stated c - the yardsticks are printed;
 (c) resolving power: for every kernel one deliberately wrong restatement must violate the check on the chosen inputs under the u_out
     of every dtype (a correct kernel is stood in for by the T rounding of the right reference)."""
import collections

import pytest
import torch
import torch.nn.functional as F

import aux_ref as ar
import helpers as hp
from oracle import encoders_ref, movq_ref

DTYPES = ar.DTYPES
DT_IDS = [ar.DT_NAME[d] for d in DTYPES]


def close(a, b, tol=1e-12):
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


def as_T(ref, dtype):
    """what a correct kernel would store: the reference rounded once to T"""
    return ref.to(hp.tdt(dtype))


# ---- (a) the restatements against independent compositions --------------------------------------------------------------------------
def test_a_spatialnorm_matches_the_oracle():
    C, shift = 128, 2
    d = ar.to64(ar.spatialnorm_inputs(C, shift, ar.F32))
    g = ar.gen(1)
    gamma, beta = (1 + 0.3 * ar.rn(g, C)).double(), ar.rn(g, C).double()
    f = d["x"].permute(0, 3, 1, 2)                                      # NCHW
    B, _, H, W = f.shape
    fg = f.reshape(B, 32, -1)
    mu, var = fg.mean(-1), fg.var(-1, unbiased=False)
    rstd = (var + 1e-6).rsqrt().repeat_interleave(C // 32, 1)           # [B][C]
    A = rstd * gamma
    d["coeff"] = torch.stack([A, beta - mu.repeat_interleave(C // 32, 1) * A], -1)
    sd = {"n.norm_layer.weight": gamma, "n.norm_layer.bias": beta, "n.conv_y.weight": d["wy"][:, :, None, None], "n.conv_y.bias": d["by"],
          "n.conv_b.weight": d["wb"][:, :, None, None], "n.conv_b.bias": d["bb"]}
    want = movq_ref._snorm(sd, "n", f, d["zq"].permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    got, _ = ar.spatialnorm_ref(d, shift, 0, 0)
    assert close(got, want)
    got1, S1 = ar.spatialnorm_ref(d, shift, 1, 0)
    assert close(got1, F.pad(want, (0, 0, 1, 1, 1, 1))) and bool((S1[:, 0] == 0).all())


def test_a_nhwc_movers():
    x = ar.nhwc_input(8, 3, 5, ar.F32).double()
    up = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    assert torch.equal(ar.upsample2_pad_ref(x), F.pad(up, (0, 0, 1, 1, 1, 1)))
    nchw = F.pad(F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), (1, 1, 1, 1))
    assert torch.equal(ar.upsample2_pad_ref(x), nchw.permute(0, 2, 3, 1))
    assert torch.equal(ar.pad_copy_ref(x), F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1)).permute(0, 2, 3, 1))
    x = ar.nhwc_input(8, 6, 10, ar.F32).double()
    # Downsample (vqgan_blocks.py:119-126) takes the stride-1 "same" map at its odd positions: here that map with an identity centre tap
    w = torch.zeros(8, 8, 3, 3, dtype=torch.float64)
    w[torch.arange(8), torch.arange(8), 1, 1] = 1
    same = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1)
    assert torch.equal(ar.subsample_odd_ref(x), same[:, :, 1::2, 1::2].permute(0, 2, 3, 1))


def test_a_softmax_layernorm_attention():
    x = ar.softmax_input(200, ar.SOFTMAX_SCALES[0], ar.F32).double()
    assert close(ar.softmax_ref(x, ar.SOFTMAX_SCALES[0])[0], torch.softmax(x * ar.SOFTMAX_SCALES[0], -1))
    d = ar.to64(ar.layernorm_inputs(832, 1, offset=True))
    assert close(ar.layernorm_ref(d["x"], d["g"], d["b"], 1e-5)[0], F.layer_norm(d["x"], (832,), d["g"], d["b"], 1e-5))
    g = ar.gen(2)
    hd, n, heads = 104, 17, ar.ATT_HEADS
    D = hd * heads
    xs, wq = ar.rn(g, 2, n, D).double(), (ar.rn(g, 3 * D, D) * D ** -0.5).double()
    want = encoders_ref._mha(xs, wq, None, torch.eye(D, dtype=torch.float64), None, heads)
    assert close(ar.attention_ref(F.linear(xs, wq), hd)[0], want)


def test_a_patchify_uint8_quant_conv_prepare():
    for (S, patch) in ar.PATCH_CASES:
        img = ar.patch_image(S)
        K = 3 * patch * patch
        want = F.unfold(img, patch, stride=patch).transpose(1, 2).reshape(-1, K)
        got = ar.patchify_ref(img, patch, ar.F32)
        assert torch.equal(got[:, :K], want) and bool((got[:, K:] == 0).all()) and got.shape[1] % 64 == 0
    x = ar.to_uint8_input(2, 3)
    assert torch.equal(ar.to_uint8_ref(x), movq_ref.process_images_u8(x))
    d = ar.to64(ar.quant_conv_inputs(15))
    want = F.conv2d(d["h"].view(2, 4, 15, 1), d["w"][:, :, None, None], d["b"]).view(2, 4, 15)
    assert close(ar.quant_conv_ref(d)[0], want)
    d = ar.to64(ar.movq_prepare_inputs(3, 5))
    ref, S, zq = ar.movq_prepare_ref(d)
    want = F.pad(F.conv2d(d["z"], d["w"][:, :, None, None], d["b"]), (1, 1, 1, 1)).permute(0, 2, 3, 1)
    assert close(ref[..., :4], want) and bool((ref[..., 4:] == 0).all()) and torch.equal(zq, d["z"].permute(0, 2, 3, 1))
    d = ar.to64(ar.masked_mean_inputs(72))
    m = d["mask"]
    assert close(ar.masked_mean_ref(d)[0], (d["x"] * m[..., None]).sum(1) / m.sum(1)[:, None])


def test_a_embed_positions_are_transformers_formula():
    for (name, D, xlmr, max_pos, tok) in ar.embed_cases():
        w = ar.embed_weights(D)
        got = ar.embed_ref(tok, w, xlmr, max_pos)
        for b in range(tok.shape[0]):
            cnt = 0
            for t in range(tok.shape[1]):
                tid = int(tok[b, t])
                cnt += tid != ar.EMBED_PAD
                pos = min((cnt if tid != ar.EMBED_PAD else 0) + ar.EMBED_PAD, max_pos - 1) if xlmr else t
                want = w["te"][min(max(tid, 0), ar.EMBED_VOCAB - 1)] + w["pe"][pos]
                if xlmr:
                    want = want + w["ty"]
                assert torch.equal(got[b, t], want), (name, b, t)


# ---- (b) torch's own fp32 evaluation inside every bound -------------------------------------------------------------------------------
def fp32_ok(v32, ref, bound):
    nbad, ratio = ar.violations(v32, ref, bound)
    return nbad == 0, ratio


def test_b_class_d_fp32_inside_bounds():
    for dtype in DTYPES:
        for C in (128, 512):
            for shift in range(5):
                d = ar.spatialnorm_inputs(C, shift, dtype)
                pre, S = ar.spatialnorm_ref(ar.to64(d), shift, 1, 0)
                p32, _ = ar.spatialnorm_ref(d, shift, 1, 0)
                for act in (0, 1):
                    ref, bound = ar.spatialnorm_bound(pre, S, act, ar.F32)
                    ok, r = fp32_ok(F.silu(p32) if act else p32, ref, bound)
                    assert ok, ("spatialnorm", C, shift, act, r)
    for (h, w) in ar.PREP_HW:
        d = ar.movq_prepare_inputs(h, w)
        ref, S, _ = ar.movq_prepare_ref(ar.to64(d))
        assert fp32_ok(ar.movq_prepare_ref(d)[0], ref, 16 * ar.U24 * S + ar.U24 * ref.abs())[0]
    for HW in ar.QUANT_HW:
        d = ar.quant_conv_inputs(HW)
        ref, S = ar.quant_conv_ref(ar.to64(d))
        assert fp32_ok(ar.quant_conv_ref(d)[0], ref, 16 * ar.U24 * S + ar.U24 * ref.abs())[0]
    for D in (72, 1024):
        d = ar.masked_mean_inputs(D)
        ref, S = ar.masked_mean_ref(ar.to64(d))
        ok, r = fp32_ok(ar.masked_mean_ref(d)[0], ref, 2 * (77 + 2) * ar.U24 * S + ar.U24 * ref.abs())
        assert ok, ("masked_mean", D, r)
    for (bs, D, nz) in ar.SAMPLER_CASES:
        d = ar.sampler_inputs(bs, D, nz)
        ref, S, e_act = ar.sampler_ref(ar.to64(d))
        ok, r = fp32_ok(ar.sampler_ref(d)[0], ref, ar.SAMPLER_N * ar.U24 * S + ar.U24 * ref.abs() + e_act)
        assert ok, ("sampler", bs, D, nz, r)


def test_b_class_m_yardsticks():
    """prints the CPU yardsticks recorded in aux_ref's docstring and asserts torch's fp32 evaluation under each kernel's c"""
    yl = collections.OrderedDict()
    for kind, Ds in (("enc", ar.ENC_LN_D), ("prior", ar.PRIOR_LN_D)):
        for D in Ds:
            for ld_mult in (1, 3):
                for offset in (False, True):
                    d = ar.layernorm_inputs(D, ld_mult, offset)
                    xs = d["x"][1:1 + ar.LN_ROWS, :D]
                    ref, S = ar.layernorm_ref(xs.double(), d["g"].double(), d["b"].double(), 1e-5)
                    y = ar.plain_ratio(F.layer_norm(xs, (D,), d["g"], d["b"], 1e-5), ref, S)
                    yl[(kind, D)] = max(yl.get((kind, D), 0.0), y)
    for k, y in yl.items():
        print(f"layernorm yardstick (CPU) {k[0]} {ar.LN_ROWS} x {k[1]}: {y:.3f}")
    assert max(yl.values()) < ar.AUX_C["layernorm"]
    ys = {}
    for Lr in ar.SOFTMAX_L:
        for scale in ar.SOFTMAX_SCALES:
            for dtype in DTYPES:
                x = ar.softmax_input(Lr, scale, dtype)
                ref, S = ar.softmax_ref(x.double(), scale)
                v32 = torch.softmax(x.float() * scale, -1)
                rows = ((v32.double() - ref).abs() / (ar.U24 * S)).max(-1).values
                ys[(Lr, round(scale, 4))] = torch.maximum(ys.get((Lr, round(scale, 4)), torch.zeros(ar.SOFTMAX_ROWS, dtype=torch.float64)), rows)
    for k, rows in ys.items():
        print(f"softmax yardstick (CPU) L={k[0]} scale={k[1]}: rows " + " ".join(f"{r:.2f}" for r in rows.tolist()))
    assert max(r.max().item() for r in ys.values()) < ar.AUX_C["softmax"]
    ya = {}
    for (hd, n) in ar.ATT_CASES:
        for spike in [None] + ar.att_spikes(n):
            for dtype in DTYPES:
                qkv = ar.attention_input(hd, n, dtype, spike)
                ref, S = ar.attention_ref(qkv.double(), hd)
                ya[(hd, n, spike is not None)] = max(ya.get((hd, n, spike is not None), 0.0), ar.plain_ratio(ar.attention_ref(qkv, hd)[0], ref, S))
    for k, y in ya.items():
        print(f"attention yardstick (CPU) hd={k[0]} n={k[1]} {'spike' if k[2] else 'random'}: {y:.3f}")
    assert max(ya.values()) < ar.AUX_C["attention"]
    for exact in (0, 1):
        for n in ar.MLP_N[:2] + (4096 + 77,):
            x = ar.mlp_act_input(n)
            ref, bound = ar.mlp_act_bound(x, exact, ar.F32)
            assert fp32_ok(ar.mlp_act_torch32(x, exact), ref, bound)[0]


# ---- (c) resolving power ----------------------------------------------------------------------------------------------------------------
def rejected(out_T, ref_mut, bound_mut):
    return ar.violations(out_T, ref_mut, bound_mut)[0] > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_c_movq_mutations_are_rejected(dtype):
    for shift in (0, 1, 3, 4):
        d = ar.to64(ar.spatialnorm_inputs(128, shift, dtype))
        for act in (0, 1):
            good = as_T(ar.spatialnorm_bound(*ar.spatialnorm_ref(d, shift, 1, act), act, dtype)[0], dtype)
            for mut in ("zq_neighbour", "border_in", "vec_swap"):
                ref, bound = ar.spatialnorm_bound(*ar.spatialnorm_ref(d, shift, 1, act, mut), act, dtype)
                assert rejected(good, ref, bound), (shift, act, mut)
            ref, bound = ar.spatialnorm_bound(*ar.spatialnorm_ref(d, shift, 1, act), act, dtype)
            assert not rejected(good, ref, bound)
    T = hp.tdt(dtype)
    x = ar.nhwc_input(128, 3, 5, dtype)
    assert ar.exact_violations(ar.upsample2_pad_ref(x).to(T), ar.upsample2_pad_ref(x, "border_in").to(T)) > 0
    assert ar.exact_violations(ar.pad_copy_ref(x).to(T), ar.pad_copy_ref(x, "border_in").to(T)) > 0
    x = ar.nhwc_input(128, 6, 10, dtype)
    assert ar.exact_violations(ar.subsample_odd_ref(x).to(T), ar.subsample_odd_ref(x, "vec_swap").to(T)) > 0
    c = ar.AUX_C["softmax"]
    for Lr in ar.SOFTMAX_L:
        x = ar.softmax_input(Lr, ar.SOFTMAX_SCALES[0], dtype).double()
        good = as_T(ar.softmax_ref(x, ar.SOFTMAX_SCALES[0])[0], dtype)
        ref, S = ar.softmax_ref(x, ar.SOFTMAX_SCALES[0], "vec_swap")
        assert rejected(good, ref, c * ar.U24 * S + ar.rounding(ref, dtype)), Lr
    d = ar.to64(ar.movq_prepare_inputs(3, 5))
    good = as_T(ar.movq_prepare_ref(d)[0], dtype)
    ref, S, _ = ar.movq_prepare_ref(d, "border_in")
    assert rejected(good, ref, 16 * ar.U24 * S + ar.rounding(ref, dtype))
    img = ar.acts(ar.gen(453), 2, 3, 3, 5)
    assert ar.exact_violations(ar.movq_enc_prepare_ref(img, dtype), ar.movq_enc_prepare_ref(img, dtype, "border_in")) > 0
    d = ar.to64(ar.quant_conv_inputs(15))
    ref, S = ar.quant_conv_ref(d, "transposed")
    assert rejected(ar.quant_conv_ref(d)[0].float(), ref, 16 * ar.U24 * S + ar.U24 * ref.abs())
    x = ar.to_uint8_input(2, 3)
    assert ar.exact_violations(ar.to_uint8_ref(x), ar.to_uint8_ref(x, "half_up")) > 0
    x = ar.to_uint8_input(*ar.U8_HW[1])
    assert ar.exact_violations(ar.to_uint8_ref(x), ar.to_uint8_ref(x, "half_up")) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_c_encoder_and_prior_mutations_are_rejected(dtype):
    c = ar.AUX_C["layernorm"]
    for D in (64, 2048):
        d = ar.to64(ar.layernorm_inputs(D, 1))
        x = d["x"][1:1 + ar.LN_ROWS]
        good = as_T(ar.layernorm_ref(x, d["g"], d["b"], 1e-5)[0], dtype)
        ref, S = ar.layernorm_ref(x, d["g"], d["b"], 1e-5, "gain_shift")
        assert rejected(good, ref, c * ar.U24 * S + ar.rounding(ref, dtype)), D
    cases = {name: (D, xlmr, mp, tok) for (name, D, xlmr, mp, tok) in ar.embed_cases()}
    D, xlmr, mp, tok = cases["xlmr-clamp"]
    w = ar.embed_weights(D)
    assert ar.exact_violations(ar.embed_ref(tok, w, xlmr, mp), ar.embed_ref(tok, w, xlmr, mp, "unclamped")) > 0
    tok = ar.eot_tokens()
    x = ar.acts(ar.gen(825 + 64), tok.shape[0], tok.shape[1], 64)
    assert ar.exact_violations(ar.gather_eot_ref(tok, x), ar.gather_eot_ref(tok, x, "tie_last")) > 0
    d = ar.to64(ar.masked_mean_inputs(72))
    ref, S = ar.masked_mean_ref(d, "plain_mean")
    assert rejected(ar.masked_mean_ref(d)[0].float(), ref, 2 * 79 * ar.U24 * S + ar.U24 * ref.abs())
    img = ar.patch_image(28)
    assert ar.exact_violations(ar.patchify_ref(img, 14, dtype), ar.patchify_ref(img, 14, dtype, "pad_nonzero")) > 0
    assert ar.exact_violations(ar.patchify_ref(img, 14, dtype), ar.patchify_ref(img, 14, dtype, "ij_swapped")) > 0
    d = ar.assemble_inputs(4)
    assert ar.exact_violations(ar.assemble_ref(d), ar.assemble_ref(d, "cls_without_pos")) > 0
    d = ar.finish_inputs()
    assert ar.exact_violations(ar.finish_ref(d), ar.finish_ref(d, "last_row_kept")) > 0
    x = ar.mlp_act_input(255)
    ref, bound = ar.mlp_act_bound(x, 0, dtype)
    mut = ar.mlp_act_ref(x.double(), 0, "silu")
    assert rejected(as_T(ref, dtype), mut, bound)
    ca = ar.AUX_C["attention"]
    for (hd, n) in ar.ATT_CASES:
        if n == 1:
            continue
        qkv = ar.attention_input(hd, n, dtype, n - 1).double()
        good = as_T(ar.attention_ref(qkv, hd)[0], dtype)
        ref, S = ar.attention_ref(qkv, hd, "last_key_dropped")
        assert rejected(good, ref, ca * ar.U24 * S + ar.rounding(ref, dtype)), (hd, n)
        ref, S = ar.attention_ref(qkv, hd)
        assert not rejected(good, ref, ca * ar.U24 * S + ar.rounding(ref, dtype))
    d = ar.to64(ar.sampler_inputs(3, 64, 1.0))
    ref, S, e_act = ar.sampler_ref(d, "no_clamp")
    assert rejected(ar.sampler_ref(d)[0].float(), ref, ar.SAMPLER_N * ar.U24 * S + ar.U24 * ref.abs() + e_act)
