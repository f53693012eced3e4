"""Float64 restatements, inputs and bounds of the small kernels around the MoVQ, encoder and prior engines (csrc/movq_kernels.hip,
csrc/encoder.hip, csrc/prior.hip), for tests/test_aux_kernels_cpu.py and tests/test_aux_kernels_gpu.py.  A plain module like helpers.py.

Every restatement is written from the operation's definition (the kernels' source comments and the reference lines they cite), in the
dtype of the tensors it is given: float64 for the reference, float32 for "torch's own fp32 evaluation" of the short expressions.  It
works on the operand values a kernel is promised to see - T-rounded where the input is T, fp32 values exact (`seen`).  Where a bound
needs the expression over absolute values the function returns (ref, S) as helpers.igemm_pre64 does.  `mut` selects ONE deliberately
wrong variant of a restatement (part (c) of the CPU test: the chosen inputs must tell it apart under the u_out of every dtype).

Three classes of check (out buffers are pre-filled with NaN / 0xA5 and carry guard elements on both sides; `violations` also counts
every element the launch does not own that no longer holds the fill):

 E  exact: data movement, or fp32 additions that cannot be contracted - torch.equal against the T rounding of the fp32 value.
 D  derived:   |out - ref| <= n * 2^-24 * S + u_out * |ref|,  n = twice the number of roundings on the longest path (FMA contraction
    only removes roundings), S the expression over absolute values:
      post_quant_conv / quant_conv   4 products, 3 adds, bias: 8 roundings, n = 16
      spatialnorm_apply              sy / sb (8) + x * A + Bc (2) + * sy + sb (2) = 12, n = 24; with SiLU: L_act and e_act as class M
      enc_masked_mean                n = 2 * (n_ctx + 2): n_ctx products into n_ctx adds, the denominator, the division
      prior_sampler_step             c - u, * s, + u (3); clamp (0); * tab0 (1); + tab1 * x (1, the product is a sibling); + noise term (1)
                                     = 6 on the longest path, n = 12 (the noise path: expf, two products = 3 + the shared add);
                                     expf(0.5 * log_var) adds e_act = 4 x torch's fp32 exp error on it, times |tab3 * noise|
 M  measured constant, the rule of helpers.IGEMM_C:   L_act * c * 2^-24 * S + u_out * |ref| (+ e_act),  c = 4 while the yardstick - the
    largest |torch fp32 - float64| / (2^-24 * S) of torch's OWN fp32 evaluation of the operation on the same operands - stays under 2,
    otherwise twice the yardstick; never taken from a kernel.  The GPU test asserts that torch itself is under c.  MEASURED yardsticks
    (CPU: test_aux_kernels_cpu.py prints them; MI355X: test_aux_kernels_gpu.py prints them), per kernel and shape:

      enc_layernorm / prior_layernorm (F.layer_norm in fp32; S = (2 |x - mu| + mean|x|) rstd |g| + |b|), rows x D, all ldx / offsets:
        D                 64     300    768    832    1024   1664   2048
        CPU   enc         1.62   -      2.06   1.49   1.27   2.55   1.27      prior: 1.62 (64), 2.32 (300), 1.27 (2048)
        MI355X enc        1.76   -      2.52   2.23   1.90   4.46   1.33      prior: 1.76 (64), 1.36 (300), 1.33 (2048)
        (the rows with mean = 10 sd read the same or lower: 1.01 at D = 2048.)  Largest 4.458 -> c = 2 x 4.458 = 8.92.
      softmax_rows (torch.softmax(x.float() * scale, -1); S = ref * (2 + |scale x - max|)):
        rows 0-3 (random, equal, dominating logit at L - 1 / at 0), all L and both scales: CPU <= 3.01 up to L = 2056 and 8.76 at
        L = 9216 (the host sums 9216 terms in few chains); row 4 (shifted by -3e4) is a different matter: torch rounds x * scale
        (|x * scale| ~ 2650: half an ulp is 1.2e-4) BEFORE it subtracts the maximum, an absolute error the row's S (2 + |scale x - max|
        ~ 2-12) does not contain.  Per L = 8 / 64 / 200 / 2048 / 2056 / 9216, largest over both scales and the three operand types:
        CPU     569 / 594 / 542 / 760 / 464 / 481
        MI355X  569 / 595 / 542 / 761 / 465 / 481   (bf16-rounded operands alone: 13-26 - their x is a multiple of 128)
        Largest 760.837 -> c = 2 x 760.837 = 1521.7: by the rule, what torch's own fp32 evaluation needs on the issue's rows.  The kernel
        forms scale * x - max in one FMA (one rounding of the small difference) and sits at 0.001 of this bound in fp32; the 16-bit
        outputs are bounded by their own rounding (0.82 bf16, 0.998 fp16 of the bound).
      enc_attention_generic (softmax(q k^T scale) v in fp32; S = sum_k p_k |v_k| * (4 + 2 scale max_k sum_d |q_d| |k_d|)):
        (hd, n)            (104, 257) (104, 17) (80, 50) (128, 64) (128, 65) (32, 512) (104, 1)
        CPU    random      0.92       0.60      0.77     0.68      0.95      0.81      0.00
        MI355X random      0.89       0.57      0.66     0.88      0.69      1.04      0.00
        spike family: 0.00 on both (p is 1 on the spike key to 1e-15: both evaluations return its V row).  All under 2 -> c = 4.
      enc_mlp_act (S = |ref|; e_act = 4 x torch's fp32 F.gelu / x * sigmoid(1.702 x) error on the same pre-activations): torch's own
        error is by definition a quarter of e_act, so its yardstick beyond e_act is 0 on both machines: c = 4.
"""
import math

import torch
import torch.nn.functional as F

import helpers as hp
from kandinsky2_amd import _lib

BF16, F16, F32 = _lib.K22_BF16, _lib.K22_F16, _lib.K22_F32
DTYPES = (BF16, F16, F32)
DT_NAME = hp.DT_NAME
U24 = hp.U24
L_ACT = hp.IGEMM_L_ACT
NAN = float("nan")

# one c per class-M kernel (the rule above applied to the larger of the CPU and the MI355X reading)
AUX_C = {"layernorm": 2 * 4.458, "softmax": 2 * 760.837, "attention": 4.0, "mlp_act": 4.0}


def c_rule(yardstick):
    return 4.0 if yardstick < 2.0 else 2.0 * yardstick


def u_out(dtype):
    return hp.u_out(dtype, _lib.OUT_ROWMAJOR)


def rounding(ref, dtype):
    """one rounding of `ref` to the stored type: u_out * |ref| - and for fp16 never less than half the spacing of its subnormals, 2^-25:
    below 2^-14 an fp16 value is rounded to a multiple of 2^-24, which u_out * |ref| does not describe (softmax probabilities of a 9216-key
    row, GELU tails; bf16 and fp32 share fp32's exponent range, where nothing in these tests comes near the subnormals)"""
    r = u_out(dtype) * ref.abs()
    return r.clamp_min(2.0 ** -25) if dtype == F16 else r


def epv(dtype):
    """elements of one 16-byte channel vector (common.h: Vec16<T>::N)"""
    return 4 if dtype == F32 else 8


def gen(seed):
    return torch.Generator().manual_seed(1000003 * seed + 29)


def rn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def acts(g, *shape):
    """activations as helpers.igemm_inputs: 0.3 + 1.7 randn (a missed term shows)"""
    return 0.3 + 1.7 * rn(g, *shape)


def rounded(x, dtype):
    """fp32 tensor holding the T-rounded values (what a T tensor carries)"""
    return x.to(hp.tdt(dtype)).float()


def violations(out, ref, bound):
    return hp.igemm_violations(out, ref, bound)


def exact_violations(out, exp):
    """number of elements of `out` that differ from `exp` (NaN in exp = the fill must still be there)"""
    free = torch.isnan(exp) if exp.is_floating_point() else torch.zeros_like(exp, dtype=torch.bool)
    o_nan = torch.isnan(out) if out.is_floating_point() else torch.zeros_like(out, dtype=torch.bool)
    bad = torch.where(free, ~o_nan, o_nan | (out != exp))
    return int(bad.sum().item())


def with_guard(t, guard, fill=NAN):
    """flat copy of t with `guard` fill elements on both sides (the layout of the test's output buffers)"""
    g = torch.full((guard,), fill, dtype=t.dtype, device=t.device)
    return torch.cat([g, t.reshape(-1), g])


def silu_term(pre):
    return hp.act_eval_term(pre, _lib.ACT_SILU)


# ---- MoVQ -------------------------------------------------------------------------------------------------------------------------
SN_H0, SN_W0 = 3, 5
SN_CASES = [(C, shift, pad, act) for C in (128, 512) for shift in range(5) for pad in (0, 1) for act in (0, 1)]


def spatialnorm_inputs(C, shift, dtype, B=2):
    g = gen(100 + C + shift)
    H, W = SN_H0 << shift, SN_W0 << shift
    return {"x": rounded(acts(g, B, H, W, C), dtype), "coeff": torch.stack([1.0 + 0.3 * rn(g, B, C), 0.5 * rn(g, B, C)], -1).contiguous(),
            "zq": rn(g, B, SN_H0, SN_W0, 4), "wy": 0.5 * rn(g, C, 4), "by": 1.0 + 0.2 * rn(g, C), "wb": 0.5 * rn(g, C, 4), "bb": 0.3 * rn(g, C)}


def conv1x1_4(w, b, z, f=lambda t: t):
    """((w0 z0 + w1 z1) + (w2 z2 + w3 z3)) + b over the last dim of z [..., 4]; w [C][4] -> [..., C]"""
    w, b, z = f(w), f(b), f(z)
    p = [z[..., k:k + 1] * w[:, k] for k in range(4)]
    return ((p[0] + p[1]) + (p[2] + p[3])) + b


def spatialnorm_ref(d, shift, pad, act, mut=None):
    """SpatialNorm.forward (movq_modules.py:61-68) given the GroupNorm coefficients: act((x A + Bc) conv_y(zq) + conv_b(zq)), zq nearest-
    resized by (y >> shift, x >> shift); NHWC, zero border of `pad`.  -> (pre-activation ref, S), border included (S = 0 there)."""
    x = d["x"]
    B, H, W, C = x.shape
    yi = torch.arange(H, device=x.device) >> shift
    xi = torch.arange(W, device=x.device) >> shift
    if mut == "zq_neighbour":                              # the last pixel of every run reads the next latent cell
        xi = ((torch.arange(W, device=x.device) + 1) >> shift).clamp(max=d["zq"].shape[2] - 1)
    out = []
    for f in (lambda t: t, torch.abs):
        sy = conv1x1_4(d["wy"], d["by"], d["zq"], f)[:, yi][:, :, xi]      # [B][H][W][C]
        sb = conv1x1_4(d["wb"], d["bb"], d["zq"], f)[:, yi][:, :, xi]
        A, Bc = f(d["coeff"][:, None, None, :, 0]), f(d["coeff"][:, None, None, :, 1])
        if mut == "vec_swap":                              # the two 4-channel halves of every 8-channel vector take each other's parameters
            perm = torch.arange(C, device=x.device) ^ 4
            A, Bc, sy, sb = A[..., perm], Bc[..., perm], sy[..., perm], sb[..., perm]
        v = (f(x) * A + Bc) * sy + sb
        if mut == "border_in" and pad:                     # the zero border drawn one pixel inside
            v[:, 0] = 0; v[:, -1] = 0; v[:, :, 0] = 0; v[:, :, -1] = 0
        out.append(F.pad(v, (0, 0, pad, pad, pad, pad)))
    return out[0], out[1]


def spatialnorm_bound(pre, S, act, dtype):
    """-> (ref, bound) of the D class (n = 24), through SiLU with L_act / e_act"""
    if act:
        ref = hp.act64(pre, _lib.ACT_SILU)
        return ref, L_ACT * 24 * U24 * S + rounding(ref, dtype) + silu_term(pre)
    return pre, 24 * U24 * S + rounding(pre, dtype)


def nhwc_cases(dtype, sub=False):
    Cs = (4, 128, 260) if dtype == F32 else (8, 128, 264)
    HWs = ((2, 2), (6, 10)) if sub else ((1, 1), (3, 5), (6, 10))
    return [(C, H, W) for C in Cs for (H, W) in HWs]


def nhwc_input(C, H, W, dtype, B=2):
    return rounded(acts(gen(200 + C + 7 * H + W), B, H, W, C), dtype)


def upsample2_pad_ref(x, mut=None):
    """Upsample.forward (movq_modules.py:85-98) up to its conv: nearest x2, then the conv's zero border; NHWC"""
    y = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    return _bordered(y, mut)


def pad_copy_ref(x, mut=None):
    return _bordered(x, mut)


def _bordered(y, mut):
    y = y.clone()
    if mut == "border_in":
        y[:, 0] = 0; y[:, -1] = 0; y[:, :, 0] = 0; y[:, :, -1] = 0
    return F.pad(y, (0, 0, 1, 1, 1, 1)).contiguous()


def subsample_odd_ref(x, mut=None):
    """the odd positions of a stride-1 map (Downsample, vqgan_blocks.py:109-126): out[y][x] = in[2y + 1][2x + 1]"""
    y = x[:, 1::2, 1::2].contiguous()
    if mut == "vec_swap":
        y = y[..., torch.arange(y.shape[-1], device=y.device) ^ 4].contiguous()
    return y


SOFTMAX_L = (8, 64, 200, 2048, 2056, 9216)
SOFTMAX_SCALES = (128 ** -0.5, 512 ** -0.5)
SOFTMAX_ROWS = 5


def softmax_input(L, scale, dtype):
    """5 rows: random logits (scaled sd 3), equal values, one dominating logit at L - 1, one at 0, a row shifted by -3e4"""
    g = gen(300 + L)
    x = (3.0 / scale) * rn(g, SOFTMAX_ROWS, L)
    x[1] = 0.75
    x[2, L - 1] = 40.0 / scale
    x[3, 0] = 40.0 / scale
    x[4] = x[4] - 3.0e4
    return rounded(x, dtype)


def softmax_ref(x, scale, mut=None):
    """softmax(scale * x) over rows (AttnBlock, movq_modules.py:218) -> (ref, S)"""
    t = x * scale
    t = t - t.max(-1, keepdim=True).values
    e = torch.exp(t)
    den = e.sum(-1, keepdim=True)
    if mut == "vec_swap":                                  # vector count taken for 8-wide vectors of a 4-wide type: the last 4 elements missed
        den = e[:, :-4].sum(-1, keepdim=True)
    ref = e / den
    return ref, ref * (2.0 + t.abs())


PREP_HW = ((1, 1), (3, 5), (16, 18))
CPAD = 64


def movq_prepare_inputs(h, w, B=2):
    g = gen(400 + 31 * h + w)
    return {"z": acts(g, B, 4, h, w), "w": 0.5 * rn(g, 4, 4), "b": rn(g, 4)}


def movq_prepare_ref(d, mut=None):
    """post_quant_conv (autoencoder.py:167, 182-185) of the NCHW latent as zero-bordered NHWC with channels 4.. zero -> (xin ref, S, zq)"""
    z = d["z"].permute(0, 2, 3, 1)                         # [B][h][w][4]
    out = []
    for f in (lambda t: t, torch.abs):
        q = conv1x1_4(d["w"], d["b"], z, f)
        if mut == "border_in":
            q[:, 0] = 0; q[:, -1] = 0; q[:, :, 0] = 0; q[:, :, -1] = 0
        out.append(F.pad(q, (0, CPAD - 4, 1, 1, 1, 1)))
    return out[0], out[1], z.contiguous()


def movq_enc_prepare_ref(img, dtype, mut=None):
    """fp32 NCHW image -> zero-bordered NHWC T, channels 3.. zero (exact)"""
    v = img.permute(0, 2, 3, 1).clone()
    if mut == "border_in":
        v[:, 0] = 0; v[:, -1] = 0; v[:, :, 0] = 0; v[:, :, -1] = 0
    return F.pad(v, (0, CPAD - 3, 1, 1, 1, 1)).to(hp.tdt(dtype)).contiguous()


QUANT_HW = (1, 15, 300)


def quant_conv_inputs(HW, B=2):
    g = gen(500 + HW)
    return {"h": acts(g, B, 4, HW), "w": 0.5 * rn(g, 4, 4), "b": rn(g, 4)}


def quant_conv_ref(d, mut=None):
    """quant_conv (1x1, 4 -> 4; autoencoder.py:176-180) on NCHW [B][4][HW] -> (ref, S)"""
    w = d["w"].T if mut == "transposed" else d["w"]
    out = [conv1x1_4(w, d["b"], d["h"].permute(0, 2, 1), f).permute(0, 2, 1).contiguous() for f in (lambda t: t, torch.abs)]
    return out[0], out[1]


U8_HW = ((2, 3), (896, 800))


def to_uint8_input(H, W, B=2, C=3):
    """-1, 1, +-3, every tie (k + 0.5) / 127.5 - 1, random"""
    g = gen(600 + H)
    x = 0.7 * rn(g, B * C * H * W)
    k = torch.arange(255, dtype=torch.float64)
    special = torch.cat([torch.tensor([-1.0, 1.0, 3.0, -3.0], dtype=torch.float64), (k + 0.5) / 127.5 - 1.0]).float()
    if x.numel() >= 2 * special.numel():
        x[5:5 + special.numel()] = special
        x[-special.numel():] = special
    else:
        x[:] = special[torch.arange(x.numel()) * 7 % special.numel()]
    return x.view(B, C, H, W)


def to_uint8_ref(x, mut=None):
    """process_images (kandinsky2/utils.py:57-70): ((x + 1) * 127.5).round().clamp(0, 255) in fp32 (torch.round: half to even), NHWC"""
    v = (x + 1) * 127.5
    v = torch.floor(v + 0.5) if mut == "half_up" else v.round()
    return v.clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------
ENC_LN_D = (64, 768, 832, 1024, 1664, 2048)
PRIOR_LN_D = (64, 300, 2048)
LN_ROWS = 5


def layernorm_inputs(D, ld_mult, offset=False):
    """7 rows of stride ld_mult * D (the launch gets rows 1..5); offset: per-row mean 10 x the row's standard deviation"""
    g = gen(700 + D + ld_mult)
    x = acts(g, LN_ROWS + 2, ld_mult * D)
    if offset:
        x = 17.0 + 1.7 * rn(g, LN_ROWS + 2, ld_mult * D)
    return {"x": x, "g": 1.0 + 0.3 * rn(g, D), "b": 0.5 * rn(g, D)}


def layernorm_ref(x, g, b, eps, mut=None):
    """LayerNorm over the last dim (biased variance) -> (ref, S); x [rows][D]"""
    mu = x.mean(-1, keepdim=True)
    dlt = x - mu
    rstd = (dlt * dlt).mean(-1, keepdim=True).add(eps).rsqrt()
    if mut == "gain_shift":
        g = torch.roll(g, 1)
    ref = dlt * rstd * g + b
    S = (2 * dlt.abs() + x.abs().mean(-1, keepdim=True)) * rstd * g.abs() + b.abs()
    return ref, S


def plain_ratio(v32, ref, S):
    """the yardstick: largest |fp32 evaluation - float64| / (2^-24 * S)"""
    return ((v32.double() - ref).abs() / (U24 * S).clamp_min(1e-300)).max().item()


# ---- encoder helpers ----------------------------------------------------------------------------------------------------------------
def embed_cases():
    """(name, D, xlmr, max_pos, tokens [B][77]); vocab 50, pad_id 1"""
    n = 77
    g = gen(800)
    out = []
    for D in (64, 72):
        t = torch.randint(2, 50, (2, n), generator=g, dtype=torch.int32)
        t[0, 3] = -5; t[1, 9] = 50; t[1, 10] = 1000                # clamped into [0, vocab)
        out.append((f"clip-D{D}", D, 0, 0, t))
    x = torch.randint(2, 50, (4, n), generator=g, dtype=torch.int32)
    x[1, 50:] = 1                                                   # trailing padding
    x[2, 20:30] = 1                                                 # padding in the middle
    x[3, :] = 1                                                     # all padding
    out.append(("xlmr", 64, 1, n + 2, x))
    out.append(("xlmr-clamp", 64, 1, 40, x))
    return out


EMBED_VOCAB, EMBED_PAD, EMBED_POS_ROWS = 50, 1, 80


def embed_weights(D):
    g = gen(810 + D)
    return {"te": rn(g, EMBED_VOCAB, D), "pe": rn(g, EMBED_POS_ROWS, D), "ty": rn(g, D)}


def embed_ref(tok, wts, xlmr, max_pos, mut=None):
    """(tok_emb[id] + pos_emb[pos]) + type_emb in fp32 (exact).  xlmr: transformers' create_position_ids_from_input_ids,
    cumsum(tok != pad) * (tok != pad) + pad, clamped to max_pos - 1; ids clamped into [0, vocab)"""
    n = tok.shape[1]
    tok = tok.long()
    if xlmr:
        m = (tok != EMBED_PAD).long()
        pos = torch.cumsum(m, 1) * m + EMBED_PAD
        if mut != "unclamped":
            pos = pos.clamp(max=max_pos - 1)
    else:
        pos = torch.arange(n, device=tok.device)[None].expand_as(tok)
    ids = tok.clamp(0, EMBED_VOCAB - 1)
    v = wts["te"][ids] + wts["pe"][pos]
    return v + wts["ty"] if xlmr else v


def eot_tokens(n=77):
    """argmax at 0, at n - 1, in the middle, and a tie (the first wins)"""
    g = gen(820)
    t = torch.randint(1, 400, (4, n), generator=g, dtype=torch.int32)
    t[0, 0] = 999; t[1, n - 1] = 999; t[2, 40] = 999
    t[3, 11] = 999; t[3, 60] = 999
    return t


def gather_eot_ref(tok, x, mut=None):
    n = tok.shape[1]
    if mut == "tie_last":
        idx = n - 1 - torch.flip(tok, (1,)).argmax(1)
    else:
        idx = tok.argmax(1)
    return x[torch.arange(tok.shape[0], device=x.device), idx]


def masked_mean_inputs(D, n=77):
    g = gen(830 + D)
    mask = torch.ones(3, n)
    mask[1] = 0; mask[1, 33] = 1
    mask[2, 50:] = 0
    return {"x": acts(g, 3, n, D), "mask": mask}


def masked_mean_ref(d, mut=None):
    """(embs * mask).sum(1) / mask.sum(1) (text_encoders.py:108-122) -> (ref, S)"""
    x, m = d["x"], d["mask"].to(d["x"].dtype)
    den = m.sum(1, keepdim=True)
    if mut == "plain_mean":
        den = torch.full_like(den, m.shape[1])
    return (x * m[..., None]).sum(1) / den, (x.abs() * m[..., None]).sum(1) / den


PATCH_CASES = ((28, 14), (32, 8))


def patch_image(S, B=2):
    """arange-like planes: every (b, c, i, j) holds a different, exactly representable value"""
    return (torch.arange(B * 3 * S * S, dtype=torch.float32).view(B, 3, S, S) * 0.25 - 300.0).contiguous()


def patchify_ref(img, patch, dtype, mut=None):
    """conv1's im2col (clip/model.py VisionTransformer.forward): row b * P + py * g + px, column c * p * p + i * p + j, zero padded to Kp"""
    B, _, S, _ = img.shape
    gq, K = S // patch, 3 * patch * patch
    Kp = (K + 63) // 64 * 64
    v = img.view(B, 3, gq, patch, gq, patch)
    v = v.permute(0, 2, 4, 1, 5, 3) if mut == "ij_swapped" else v.permute(0, 2, 4, 1, 3, 5)
    rows = F.pad(v.reshape(B * gq * gq, K), (0, Kp - K))
    if mut == "pad_nonzero" and Kp > K:
        rows[:, K] = rows[:, K - 1]
    return rows.to(hp.tdt(dtype)).contiguous()


def assemble_inputs(P, D=64, B=2):
    g = gen(840 + P)
    return {"patch": acts(g, B, P, D), "cls": rn(g, D), "pos": rn(g, P + 1, D)}


def assemble_ref(d, mut=None):
    B = d["patch"].shape[0]
    x = torch.cat([d["cls"][None, None].expand(B, 1, -1), d["patch"]], 1)
    pos = d["pos"].clone()
    if mut == "cls_without_pos":
        pos[0] = 0
    return x + pos


def finish_inputs(n=7, D=64, B=2):
    g = gen(850)
    return {"inp": acts(g, B, n, D), "pos": rn(g, n, D), "prd": rn(g, D)}


def finish_ref(d, mut=None):
    x = d["inp"].clone()
    if mut != "last_row_kept":
        x[:, -1] = d["prd"]
    return x + d["pos"]


MLP_N = (1, 255, 256 * 4096 + 77)


def mlp_act_input(n):
    g = gen(860 + n % 1000)
    x = (24.0 * torch.rand(n, generator=g, dtype=torch.float32) - 12.0)
    x[0] = 60.0 if n == 1 else -60.0
    if n > 4:
        x[n // 2] = 60.0; x[-1] = -60.0; x[1] = 60.0
    return x


def mlp_act_ref(x, exact, mut=None):
    """erf GELU, or QuickGELU x * sigmoid(1.702 x) (clip/model.py) -> ref; works in x's dtype"""
    if exact:
        return 0.5 * x * (1.0 + torch.erf(x * 2.0 ** -0.5))
    return x * torch.sigmoid((1.0 if mut == "silu" else 1.702) * x)


def mlp_act_torch32(x32, exact):
    return F.gelu(x32) if exact else x32 * torch.sigmoid(1.702 * x32)


def mlp_act_bound(x, exact, dtype):
    ref = mlp_act_ref(x.double(), exact)
    e_act = 4.0 * (mlp_act_torch32(x, exact).double() - ref).abs().max().item()
    return ref, L_ACT * AUX_C["mlp_act"] * U24 * ref.abs() + rounding(ref, dtype) + e_act


ATT_CASES = ((104, 257), (104, 17), (80, 50), (128, 64), (128, 65), (32, 512), (104, 1))
ATT_HEADS = 2


def att_spikes(n):
    return sorted({s for s in (n - 1, 63, 64) if 0 <= s < n})


def attention_input(hd, n, dtype, spike=None, B=2):
    """qkv [B][n][3 * heads * hd] (Q | K | V planes, heads x hd inside each).  spike: key `spike` gets a dominating logit against every
    query and carries a distinctive V row"""
    D = ATT_HEADS * hd
    g = gen(900 + hd + n + (0 if spike is None else 1000 + spike))
    qkv = 1.5 * rn(g, B, n, 3, ATT_HEADS, hd)
    if spike is not None:
        sgn = torch.where(torch.arange(hd) % 2 == 0, 1.0, -1.0)
        qkv[:, :, 0] = 0.45 * rn(g, B, n, ATT_HEADS, hd) + sgn
        qkv[:, spike, 1] = 8.0 * sgn
        qkv[:, spike, 2] = 10.0 + torch.arange(hd) / 8.0 + torch.arange(ATT_HEADS)[:, None] * 0.5
    return rounded(qkv.reshape(B, n, 3 * D), dtype)


def attention_ref(qkv, hd, mut=None):
    """CLIPAttention.forward of transformers: softmax((q hd^-0.5) k^T) v per head -> (ref [B][n][D], S)"""
    B, n, D3 = qkv.shape
    D = D3 // 3
    heads = D // hd
    q, k, v = (qkv[:, :, i * D:(i + 1) * D].reshape(B, n, heads, hd).permute(0, 2, 1, 3) for i in range(3))
    if mut == "last_key_dropped" and n > 1:
        k, v = k[:, :, :-1], v[:, :, :-1]
    scale = hd ** -0.5
    p = torch.softmax(q @ k.transpose(-1, -2) * scale, -1)
    ref = p @ v
    amp = 4.0 + 2.0 * scale * (q.abs() @ k.abs().transpose(-1, -2)).max(-1, keepdim=True).values
    S = (p @ v.abs()) * amp
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, n, D)   # noqa: E731
    return back(ref), back(S)


# ---- prior ----------------------------------------------------------------------------------------------------------------------------
SAMPLER_CASES = [(bs, D, nz) for bs in (1, 3) for D in (64, 768) for nz in (0.0, 1.0)]
SAMPLER_CLAMP = 10.0
SAMPLER_N = 12


def sampler_inputs(bs, D, nonzero):
    g = gen(950 + bs + D)
    return {"x": acts(g, 2 * bs, D), "mo": 4.0 * rn(g, 2 * bs, D), "noise": rn(g, 2 * bs, D), "scales": 3.0 + rn(g, bs).abs(),
            "tab": torch.tensor([0.37, 0.61, -1.3, nonzero], dtype=torch.float32)}


def sampler_ref(d, mut=None):
    """one ancestral step (prior.py:336-384, gaussian_diffusion.py:223-322): x0 = clamp(u + s (c - u)); mean = c1 x0 + c2 x;
    out = mean + nonzero exp(0.5 logvar) noise, both halves [cond | uncond] from the same guided x0 -> (ref, S, e_act)"""
    bs = d["scales"].shape[0]
    c, u = d["mo"][:bs], d["mo"][bs:]
    s = d["scales"][:, None]
    t = d["tab"]
    x0 = u + s * (c - u)
    S0 = u.abs() + s.abs() * (c.abs() + u.abs())
    if mut != "no_clamp":
        x0 = x0.clamp(-SAMPLER_CLAMP, SAMPLER_CLAMP)
    x0, S0 = x0.repeat(2, 1), S0.repeat(2, 1)
    e = torch.exp(0.5 * t[2])
    ref = (t[0] * x0 + t[1] * d["x"]) + t[3] * e * d["noise"]
    S = t[0].abs() * S0 + t[1].abs() * d["x"].abs() + t[3].abs() * e * d["noise"].abs()
    e32 = torch.exp(0.5 * t[2].float()).double()
    e_act = 4.0 * (e32 - torch.exp(0.5 * t[2].double())).abs() * (t[3] * d["noise"]).abs().double()
    return ref, S, e_act


def to64(d):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}


def to_dev(d, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in d.items()}
