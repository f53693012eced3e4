"""Float64 restatements, inputs and bounds of the small kernels that open and close a UNet step (csrc/elementwise.hip: conv_in, timestep_embedding,
linear_smallm, layernorm_f32, resample, cast_rows, kv_pack; csrc/sampler.hip: ddim_step, plms_step), for tests/test_seam_kernels_cpu.py and
tests/test_seam_kernels_gpu.py.  A plain module like aux_ref.py, whose comparator (`violations`, `exact_violations`, `with_guard`), bound
classes and c rule it imports:

 E  exact      resample mode 2, cast_rows, kv_pack (the whole of K_all and V^T_all, the zero padding to Tkp included): equal bits.
 D  derived    |out - ref| <= n * 2^-24 * S + u_out * |ref|, n = twice the roundings on the longest path of the kernel's expression AS WRITTEN
               (contraction only removes roundings), S the expression over absolute values:
      conv_in        acc = bias; acc += w * patch, 9 Cin times in sequence: the first product (1) goes through 9 Cin adds: 9 Cin + 1 roundings,
                     n = 2 (9 Cin + 1) = 74 / 146 / 164 for Cin 4 / 8 / 9.  Channels 4-7 of the operand are fp32(img * mask) when img_premul = 0:
                     that one rounding is restated in fp32, not bounded.  S = |bias| + sum |w| |patch|.
      linear_smallm  a lane takes chunks = ceil(K / (64 EPC)) chunks of EPC = 16 / sizeof(TW) weights; every group of four is
                     acc += ((x0 w0 + x1 w1) + x2 w2) + x3 w3: a product (1), three adds (3), and one add onto acc per group, G = chunks * EPC / 4
                     groups per lane: 4 + G.  Then the six-level wave sum (6), + bias (1), + add (1):  G + 12 roundings, n = 2 (G + 12)
                     (K = 2048: G = 8, n = 40; K = 8: G = 1 (fp32 weights) or 2, n = 26 / 28).  S = sum |act_in(x)| |W| + |bias|, W T-rounded.
                     SiLU as spatialnorm_apply treats it.  On the output: L_act on n * 2^-24 * S, e_act = 4 x torch's fp32 SiLU error on the
                     same pre-activations.  On the input: the kernel's operand is its own fp32 SiLU of x, the reference's the float64 one;
                     e_in = 4 x the largest |torch fp32 SiLU - float64 SiLU| over the launch's x, times sum_k |W[n][k]| (times L_act under an output SiLU).
                     `add` comes after the activation: n * 2^-24 * |add| more.
      resample 1     ((x00 + x01) + x10) + x11 onto a zero accumulator (the first add is exact), * 0.25 exact: 3 roundings, n = 6,
                     S = 0.25 sum |taps|; a trailing odd row / column is never read (H / 2 floors).
      ddim_step      e = u + g (c - u) (3); s1m * e (1); x - (1); / sqrt(a_t) (1) = x0: 6 roundings and sqrtf(a_t) (1): n_x0 = 14,
                     S0 = (|x| + s1m E) / sqrt(a_t), E = |u| + |g| (|c| + |u|) (|e| without CFG).  x_out = sqrt(a_prev) x0 (1) + dirc e (1, the product a
                     sibling) + sigma noise (1): 9 roundings and the two sqrtf (2): n_out = 22, S = sqrt(a_prev) S0 + dirc E + |sigma| |noise|.
                     dirc = sqrtf((1 - a_prev) - sigma^2): 1 - a_prev is exact for a_prev in [0.5, 1]; sigma^2 and the difference y are rounded
                     once each, |dy| <= 2^-24 (sigma^2 + y), the root halves it and is rounded itself: ddirc = 2^-24 ((sigma^2 + y) / (2 dirc) + dirc),
                     charged twice like every rounding: + 2 ddirc E on x_out.
      plms_step      e as above with every operation rounded (3); e' by order: 0: e (0); 4: (h1 + e) / 2 (1, the division exact);
                     1: (3 e - h1) / 2 (2); 2: (23 e - 16 h1 + 5 h2) / 12 (4); 3: (55 e - 59 h1 + 37 h2 - 9 h3) / 24 (5); then x0 as above (3) and
                     x_out = sqrt(a_prev) x0 + sqrt(1 - a_prev) e' (2).  Longest, order 3: x0 3 + 5 + 3 = 11 and sqrtf(a_t): n_x0 = 24; x_out 13 and two
                     sqrtf: n_out = 30 (every order is held to the order-3 count).  EP = the order's expression over absolute values, S0 = (|x| +
                     s1m EP) / sqrt(a_t), S = sqrt(a_prev) S0 + dirc EP, + 2 ddirc EP (sigma = 0).  e_store: n = 6, S = E; bit-exact without CFG.
      sqrtf of a table entry is evaluated in float64 on the fp32 entry and counted as one rounding.  Nothing in a D bound is measured.
 M  measured   c * 2^-24 * S + u_out * |ref|, c by aux_ref.c_rule from the yardstick - torch's OWN fp32 evaluation against float64 in units of
               2^-24 * S - never from a kernel.  MEASURED yardsticks (CPU: test_seam_kernels_cpu.py prints them; MI355X: test_seam_kernels_gpu.py
               prints them and asserts torch itself under c), largest over the cases of a row:
      timestep_embedding ([cos | sin] of fp32(t * f), S = 1; torch.cos / torch.sin in fp32), rows x half, both tables, t up to 999:
        half              5      192    260
        CPU               0.52   0.59   0.59
        MI355X            0.57   0.90   0.91
        All under 2 -> c = 4.
      layernorm_f32 (F.layer_norm in fp32; aux_ref.layernorm_ref's S), 7 rows x D, random rows / rows with mean = 10 sd:
        D                 5      256    300    768    1536   2560
        CPU random        0.98   1.10   1.13   1.30   1.05   1.12
        CPU mean = 10 sd  2.05   2.08   2.32   2.06   1.74   1.37
        MI355X random     0.98   1.41   1.26   1.21   1.37   1.35
        MI355X mean=10sd  1.06   0.72   1.86   2.52   3.00   5.38
        Largest 5.376 (MI355X, 7 x 2560, mean = 10 sd; the CPU's largest is 2.317 at 7 x 300) -> c = 2 x 5.376 = 10.752.  AUX_C["layernorm"] = 8.92
        was measured at other widths (up to 2048) and is not reused: torch's own evaluation needs more at D = 2560.
    The MI355X readings come from one run of test_seam_kernels_gpu.py, which prints them again on every run and asserts torch itself under c.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import aux_ref as ar
import helpers as hp
from kandinsky2_amd import _lib, pack

BF16, F16, F32 = ar.BF16, ar.F16, ar.F32
DTYPES = ar.DTYPES
DT_NAME = ar.DT_NAME
U24 = ar.U24
L_ACT = ar.L_ACT
NAN = ar.NAN
ACT_NONE, ACT_SILU = _lib.ACT_NONE, _lib.ACT_SILU
violations, exact_violations, with_guard = ar.violations, ar.exact_violations, ar.with_guard
rounding, rounded, gen, rn, acts, epv, to64, to_dev, plain_ratio = ar.rounding, ar.rounded, ar.gen, ar.rn, ar.acts, ar.epv, ar.to64, ar.to_dev, ar.plain_ratio

# one c per class-M kernel: aux_ref.c_rule on the larger of the CPU and the MI355X reading (docstring)
SEAM_C = {"timestep_embedding": ar.c_rule(0.594), "layernorm": ar.c_rule(5.376)}


def bits(t):
    """the bit patterns of a float tensor (an exact check that tells -0 from +0)"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- conv_in ------------------------------------------------------------------------------------------------------------------------------
# (B, H, W, Cin, Cout): one pixel; odd sizes, W < 8, Cout = 128; ragged second tile, Cout not a multiple of 128; W = 17 (three tiles), Cout = 384
# (three passes of the n loop); whole tiles
CONV_IN_SHAPES = ((1, 1, 1, 4, 5), (3, 5, 7, 4, 128), (2, 3, 9, 9, 130), (1, 2, 17, 8, 384), (2, 8, 8, 9, 64))


def conv_in_cases():
    """(B, H, W, Cin, Cout, img_premul, fractional mask): Cin = 9 with img_premul 0 and 1, Cin = 8 with 1; masks exactly 0 / 1 and one fractional"""
    out = []
    for (B, H, W, Cin, Cout) in CONV_IN_SHAPES:
        if Cin == 9:
            out += [(B, H, W, Cin, Cout, 0, False), (B, H, W, Cin, Cout, 1, False)]
        else:
            out.append((B, H, W, Cin, Cout, 1 if Cin == 8 else 0, False))
    out.append((2, 3, 9, 9, 130, 0, True))
    return out


def conv_in_inputs(B, H, W, Cin, Cout, frac=False):
    g = gen(1100 + 97 * H + 13 * W + Cin + Cout)
    mask = (torch.rand(B, 1, H, W, generator=g) < 0.6).float()
    if frac:
        mask = torch.rand(B, 1, H, W, generator=g)
    if mask.numel() > 2:
        mask.view(-1)[0] = 0.0; mask.view(-1)[-1] = 1.0
    return {"x": acts(g, B, 4, H, W), "img": acts(g, B, 4, H, W), "mask": mask, "w": rn(g, Cout, Cin, 3, 3) * (9 * Cin) ** -0.5, "b": rn(g, Cout)}


def conv_in_n(Cin):
    return 2 * (9 * Cin + 1)


def conv_in_operand(d, Cin, premul, mut=None):
    """the Cin-channel NCHW input the stem convolves (text2im_model2_1.py:146-155): [x | img * mask | mask]; in the dtype of d's tensors, the
    product img * mask formed in fp32 (the kernel's one rounding of it) whatever that dtype is"""
    x = d["x"]
    if Cin == 4:
        return x
    img = d["img"]
    if not premul and mut != "mask_not_applied":
        img = (d["img"].float() * d["mask"].float()).to(x.dtype)
    if Cin == 8:
        return torch.cat([x, img], 1)
    ch8 = d["img"][:, :1] if mut == "ch8_from_img" else d["mask"]
    return torch.cat([x, img, ch8], 1)


def conv_in_ref(d, Cin, premul, mut=None):
    """conv3x3, padding 1, of the operand with w [Cout][Cin][3][3] and bias -> (ref, S) NHWC [B][H][W][Cout]: nine tap-shifted channel
    contractions over the zero-bordered input.  mut last_col_dropped: the last pixel column is not owned when it ends a ragged tile"""
    inp = conv_in_operand(d, Cin, premul, mut)
    B, _, H, W = inp.shape
    out = []
    for f in (lambda t: t, torch.abs):
        xp = F.pad(f(inp), (1, 1, 1, 1))
        acc = f(d["b"]).view(1, 1, 1, -1).expand(B, H, W, -1).clone()
        for ky in range(3):
            for kx in range(3):
                acc = acc + torch.einsum("bchw,oc->bhwo", xp[:, :, ky:ky + H, kx:kx + W], f(d["w"][:, :, ky, kx]))
        out.append(acc)
    ref, S = out
    if mut == "last_col_dropped" and W % 8:
        ref = ref.clone(); ref[:, :, W - 1] = NAN
    return ref, S


def conv_in_bound(ref, S, Cin, dtype):
    return conv_in_n(Cin) * U24 * S + rounding(torch.nan_to_num(ref), dtype)


def conv_in_emul(d, Cin, premul, dtype):
    """fp32 CPU emulation of a correct kernel: torch's own fp32 convolution of the fp32 operand, rounded to T, NHWC"""
    return F.conv2d(conv_in_operand(d, Cin, premul), d["w"], d["b"], padding=1).permute(0, 2, 3, 1).contiguous().to(hp.tdt(dtype))


# ---- timestep_embedding ---------------------------------------------------------------------------------------------------------------------
TEMB_ROWS = (1, 5, 8)
TEMB_HALF = (5, 192, 260)
TEMB_T = (0.0, 0.5, 1.0, 20.4, 999.0)
TEMB_TABLES = ("product", "linear")


def temb_inputs(rows, half, table):
    """t: rows = 1 takes 999, rows = 5 the five values, rows = 8 those and 999, 20.4, 0.5 again.  freqs: the product's own table (pack.time_freqs:
    half = 192 is the one of model_channels = 384; it starts at 1.0 and its other entries make t * f inexact in fp32), or (k + 1) / half, which
    reaches 1.0 at the last entry"""
    t = {1: [999.0], 5: list(TEMB_T), 8: list(TEMB_T) + [999.0, 20.4, 0.5]}[rows]
    f = pack.time_freqs(half) if table == "product" else (torch.arange(1, half + 1, dtype=torch.float32) / half)
    return {"t": torch.tensor(t, dtype=torch.float32), "f": f.contiguous()}


def temb_arg32(d):
    """fp32(t * f): the argument as the kernel forms it (one IEEE multiplication: the same bits on every machine)"""
    return d["t"].float()[:, None] * d["f"].float()[None, :]


def temb_ref(d, mut=None):
    """timestep_embedding (nn.py:101-121): [cos(a) | sin(a)], a = fp32(t f) -> float64 [rows][2 half]; S = 1"""
    a = (d["t"].double()[:, None] * d["f"].double()[None, :]) if mut == "arg_f64" else temb_arg32(d).double()
    parts = [torch.sin(a), torch.cos(a)] if mut == "sin_cos" else [torch.cos(a), torch.sin(a)]
    return torch.cat(parts, -1)


def temb_torch32(d):
    a = temb_arg32(d)
    return torch.cat([torch.cos(a), torch.sin(a)], -1)


def temb_bound(ref):
    return SEAM_C["timestep_embedding"] * U24 * torch.ones_like(ref) + U24 * ref.abs()


# ---- linear_smallm ----------------------------------------------------------------------------------------------------------------------------
# (M, N, K, ldx - K, ldo - N, ld_add - N (None: no add), add_mod, act_in, act_out, bias): M = 1..8 each; K below one round / ragged round (320, 520) /
# the LDS limit at M = 8 (2048); N with rpw 1, 2, 4, 8 and a ragged last wave (8197 = 2 * 4096 + 5 ...); strides; add_mod 0, 2, 4 at M = 8; all act pairs
LIN_CASES = (
    (1, 1, 8, 0, 0, None, 0, 0, 0, True),
    (2, 5, 320, 8, 3, 4, 0, 1, 0, True),
    (3, 1000, 520, 0, 7, 0, 0, 0, 1, True),
    (4, 5, 2048, 16, 0, None, 0, 1, 1, False),
    (5, 1000, 320, 4, 24, 8, 0, 1, 0, True),
    (6, 5, 520, 0, 0, 3, 2, 0, 0, True),
    (7, 1000, 8, 8, 5, None, 0, 1, 1, True),
    (8, 5, 2048, 0, 11, 16, 4, 1, 0, True),
    (8, 1000, 520, 8, 8, 8, 2, 0, 1, True),
    (8, 1000, 320, 0, 0, 0, 0, 0, 0, False),
    (3, 8197, 8, 0, 0, 8, 0, 1, 0, True),
    (5, 16389, 8, 8, 16, None, 0, 0, 0, True),
    (8, 32773, 8, 0, 27, 5, 4, 1, 0, True),
    (7, 32773, 320, 0, 0, None, 0, 0, 1, True),
    # the engines' own shapes: time_embed.0 / .2 of model_channels = 384 on the rows of four steps (add_mod = B = 2), the 2.2 head's
    # encoder_hid_proj (1280 -> 10 x 768) and add_embedding (1280 -> 1536) on a CFG pair
    (8, 1536, 384, 0, 0, None, 0, 0, 1, True),
    (8, 1536, 1536, 0, 0, 0, 2, 0, 0, True),
    (2, 7680, 1280, 0, 0, None, 0, 0, 0, True),
    (2, 1536, 1280, 0, 0, None, 0, 0, 0, True),
)
LIN_ROWS_X = 8       # rows of `add` and of x generated for every case


def lin_rpw(N):
    """rows_per_wave as launch_linear_smallm chooses it (for the test's own report, not for any bound)"""
    r = 1
    while r < 8 and (N + 8 * r - 1) // (8 * r) >= 1024:
        r *= 2
    return r


def lin_inputs(case, wdtype):
    M, N, K, dx, do, da, add_mod, a_in, a_out, bias = case
    g = gen(1200 + 31 * M + N + K)
    d = {"x": acts(g, M, K + dx), "w": rounded(rn(g, N, K) * K ** -0.5, wdtype), "b": rn(g, N) if bias else None,
         "add": None if da is None else 2.0 * rn(g, LIN_ROWS_X, N + da)}
    return d


def lin_G(K, wdtype):
    epc = 4 if wdtype == F32 else 8
    return -(-K // (64 * epc)) * epc // 4


def lin_n(K, wdtype):
    return 2 * (lin_G(K, wdtype) + 12)


def lin_ref(d, case, mut=None):
    """out[m][n] = act_out(sum_k act_in(x[m][k]) W[n][k] + bias[n]) + add[m % add_mod or m][n] -> (ref, pre, S_pre, |add| term, sum|W|) float64"""
    M, N, K, dx, do, da, add_mod, a_in, a_out, bias = case
    x = d["x"][:, :K].double()
    w = d["w"].double()
    if mut == "last_chunk_dropped":                            # the last 16 bytes of every weight row are never read
        x, w = x[:, :K - 4], w[:, :K - 4]
    xa = x * torch.sigmoid(x) if (a_in == ACT_SILU and mut != "no_silu_in") else x
    pre = xa @ w.T
    S = xa.abs() @ w.abs().T
    if d["b"] is not None:
        pre = pre + d["b"].double(); S = S + d["b"].double().abs()
    ref = hp.act64(pre, ACT_SILU) if (a_out == ACT_SILU and mut != "no_silu_out") else pre
    addt = torch.zeros_like(ref)
    if d["add"] is not None:
        rows = torch.arange(M)
        if add_mod > 0 and mut != "add_row_m":
            rows = rows % add_mod
        addt = d["add"].to(ref.device)[rows.to(ref.device), :N].double()
        ref = ref + addt
    if mut == "last_row_unwritten":
        ref = ref.clone(); ref[M - 1] = NAN
    return ref, pre, S, addt.abs(), w.abs().sum(1)[None, :]


def lin_bound(d, case, wdtype):
    """-> (ref, bound)"""
    M, N, K, dx, do, da, add_mod, a_in, a_out, bias = case
    ref, pre, S, A, wsum = lin_ref(d, case)
    n = lin_n(K, wdtype)
    L = L_ACT if a_out == ACT_SILU else 1.0
    x32 = d["x"][:, :K].float()
    e_in = 4.0 * (F.silu(x32).double() - hp.act64(x32.double(), ACT_SILU)).abs().max().item() if a_in == ACT_SILU else 0.0
    e_out = hp.act_eval_term(pre, ACT_SILU) if a_out == ACT_SILU else 0.0
    return ref, L * (n * U24 * S + e_in * wsum) + e_out + n * U24 * A + U24 * ref.abs()


def lin_emul(d, case):
    """fp32 CPU emulation of a correct kernel (torch's fp32 F.linear / F.silu)"""
    M, N, K, dx, do, da, add_mod, a_in, a_out, bias = case
    x = d["x"][:, :K].float()
    v = F.linear(F.silu(x) if a_in == ACT_SILU else x, d["w"].float(), d["b"])
    if a_out == ACT_SILU:
        v = F.silu(v)
    if d["add"] is not None:
        rows = torch.arange(M) % add_mod if add_mod > 0 else torch.arange(M)
        v = v + d["add"][rows, :N]
    return v


# ---- layernorm_f32 ------------------------------------------------------------------------------------------------------------------------------
LN_ROWS = (1, 7)
LN_D = (5, 256, 300, 768, 1536, 2560)
LN_EPS = 1e-5


def ln_inputs(D, offset):
    """aux_ref's two families (random rows; rows with mean = 10 sd), 7 contiguous rows of D"""
    return ar.layernorm_inputs(D, 1, offset)


def ln_bound(ref, S):
    return SEAM_C["layernorm"] * U24 * S + U24 * ref.abs()


# ---- resample -----------------------------------------------------------------------------------------------------------------------------------
RS_BHW = ((1, 2, 2), (3, 5, 7), (2, 6, 4))
RS_CAP = {1: (1, 256, 256, 1032), 2: (1, 64, 64, 1032)}       # bf16: 128 x 128 x 129 output vectors = 2113536 > 8192 * 256: the grid-stride loop


def rs_cases(dtype):
    """(B, H, W, C, mode): C = one vector and three; both modes"""
    e = epv(dtype)
    return [(B, H, W, C, mode) for mode in (1, 2) for C in (e, 3 * e) for (B, H, W) in RS_BHW]


def rs_input(B, H, W, C, dtype, device="cpu"):
    g = torch.Generator(device=device).manual_seed(1300 + 7 * H + W + C)
    x = 0.3 + 1.7 * torch.randn(B, H, W, C, generator=g, device=device, dtype=torch.float32)
    return x.to(hp.tdt(dtype)).float()


def rs_ref(x, mode, mut=None):
    """mode 1: AvgPool2d(2) (unet.py:105-107) as ((x00 + x01) + x10) + x11 times 0.25 -> (ref, S); mode 2: nearest x2 (unet.py:67-77) -> (ref, None)"""
    B, H, W, C = x.shape
    if mode == 2:
        yi = torch.arange(2 * H, device=x.device)
        xi = torch.arange(2 * W, device=x.device)
        if mut == "nearest_round_up":
            yi, xi = ((yi + 1) >> 1).clamp(max=H - 1), ((xi + 1) >> 1).clamp(max=W - 1)
        else:
            yi, xi = yi >> 1, xi >> 1
        return x[:, yi][:, :, xi].contiguous(), None
    Ho, Wo = H // 2, W // 2
    v = x[:, :2 * Ho, :2 * Wo]
    t = [v[:, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)]
    if mut == "three_taps":
        return ((t[0] + t[1]) + t[2]) * 0.25, (t[0].abs() + t[1].abs() + t[2].abs()) * 0.25
    return (((t[0] + t[1]) + t[2]) + t[3]) * 0.25, (t[0].abs() + t[1].abs() + t[2].abs() + t[3].abs()) * 0.25


def rs_bound(ref, S, dtype):
    return 6 * U24 * S + rounding(ref, dtype)


# ---- cast_rows ----------------------------------------------------------------------------------------------------------------------------------
CAST_CASES = [(rows, cols, ldx, ldy) for rows in (1, 10) for cols in (1, 77) for (ldx, ldy) in ((cols + 3, cols + 8),)]


def cast_input(rows, ldx, dtype):
    """random values with, in every row: +-0, ties between two neighbours of T (to even: one down, one up), T's largest finite value, both signs"""
    g = gen(1400 + rows + ldx)
    x = 3.0 * rn(g, rows, ldx)
    m = {BF16: 8, F16: 11, F32: 24}[dtype]                      # significand bits of T
    big = torch.finfo(hp.tdt(dtype)).max
    special = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -m, 1.0 + 3 * 2.0 ** -m, -(1.0 + 2.0 ** -m), -(1.0 + 3 * 2.0 ** -m), big, -big,
                            (1.0 + 2.0 ** -m) * 2.0 ** -10, 2.0 ** -14 * (1.0 + 3 * 2.0 ** -m)], dtype=torch.float64).float()
    for r in range(rows):
        for j in range(min(ldx, special.numel())):
            x[r, (j * 7 + r) % ldx] = special[(j + r) % special.numel()]
    return x


def cast_expected(x, rows, cols, ldy, dtype, mut=None):
    """[rows][ldy] of T: T(x[r][c]) for c < cols, NaN (the fill) elsewhere"""
    exp = torch.full((rows, ldy), NAN, dtype=hp.tdt(dtype), device=x.device)
    src = x[:, :cols]
    if mut == "stride_swapped":                                 # x read with y's row stride
        flat = x.reshape(-1)
        idx = (torch.arange(rows, device=x.device)[:, None] * ldy + torch.arange(cols, device=x.device)[None, :]) % flat.numel()
        src = flat[idx]
    exp[:, :cols] = src.to(hp.tdt(dtype))
    return exp


# ---- kv_pack ------------------------------------------------------------------------------------------------------------------------------------
KV_CASES = ((1, 1, 1, 0), (2, 3, 100, 5), (1, 2, 64, 87), (1, 1, 64, 64))


def kv_tkp(T, S):
    return (S + T + 63) // 64 * 64


def kv_inputs(B, H, T, S, dtype):
    g = gen(1500 + 11 * T + S + H)
    C = 64 * H
    return {"qkv": rounded(acts(g, B * T, 3 * C), dtype), "ctxkv": rounded(acts(g, B * S, 2 * C), dtype) if S else None}


def kv_ref(d, B, H, T, S, mut=None):
    """QKVAttention's K / V concat (unet.py:296-302): keys [ctx | self | zero pad] -> K_all [B][H][Tkp][64], V^T_all [B][H][64][Tkp]"""
    C, Tkp = 64 * H, kv_tkp(T, S)
    qkv = d["qkv"].view(B, T, 3, H, 64)
    k, v = qkv[:, :, 1], qkv[:, :, 2]                            # [B][T][H][64]
    if S:
        ckv = d["ctxkv"].view(B, S, 2, H, 64)
        parts_k, parts_v = [ckv[:, :, 0], k], [ckv[:, :, 1], v]
        if mut == "ctx_self_swapped":
            parts_k, parts_v = parts_k[::-1], parts_v[::-1]
        k, v = torch.cat(parts_k, 1), torch.cat(parts_v, 1)
    fill = NAN if mut == "pad_not_zeroed" else 0.0
    k = F.pad(k.permute(0, 2, 1, 3), (0, 0, 0, Tkp - S - T), value=fill)      # [B][H][Tkp][64]
    v = F.pad(v.permute(0, 2, 1, 3), (0, 0, 0, Tkp - S - T), value=fill)
    vt = v.reshape(B, H, 64, Tkp) if mut == "v_not_transposed" else v.transpose(2, 3)
    return k.contiguous(), vt.contiguous()


# ---- ddim_step / plms_step ------------------------------------------------------------------------------------------------------------------------
STEP_CASES = ((2, 1, 1), (6, 35, 1), (3, 300, 0), (2, 65537, 1))          # (N, HW, use_cfg); the last: 524296 elements > 2048 * 256
STEP_GUIDANCE = 4.0
N_DDIM_OUT, N_DDIM_X0 = 22, 14
N_PLMS_OUT, N_PLMS_X0, N_PLMS_E = 30, 24, 6
PLMS_NEIGHBOUR = {0: 1, 1: 2, 2: 3, 3: 2, 4: 1}


@functools.lru_cache(maxsize=None)
def step_rows(eta):
    """[3][4] fp32 rows (alpha_t, alpha_prev, sigma_t, sqrt(1 - alpha_t)) of the product's own 50-step schedule (DDIMSamplerHIP.make_schedule
    on the 2.1 decoder's diffusion): the first step executed (t = 981), a middle one, the last (t = 1)"""
    import kandinsky2_amd as k22
    from kandinsky2_amd.diffusion import DDIMSamplerHIP
    s = DDIMSamplerHIP(None, k22.create_gaussian_diffusion(**k22.DIFFUSION_CONFIG_2_1), STEP_GUIDANCE)
    s.make_schedule(50, ddim_eta=eta)
    return np.ascontiguousarray(s.table[[49, 25, 0]])


def step_inputs(N, HW, seed=0):
    g = gen(1600 + N + HW % 1000 + seed)
    return {"x": 0.2 + 1.5 * rn(g, N, 4, HW), "mo": 0.1 + rn(g, N, 8, HW), "noise": rn(g, N, 4, HW),
            "h1": 0.1 + rn(g, N, 4, HW), "h2": -0.2 + rn(g, N, 4, HW), "h3": 0.3 + rn(g, N, 4, HW)}


def _guided(mo, use_cfg, g, mut=None):
    """-> (e, E): model_fn's guidance (kandinsky2_1_model.py:222-233) on channels 0-3: rows [cond | uncond], both halves get u + g (c - u)"""
    N = mo.shape[0]
    if not use_cfg:
        return mo[:, :4], mo[:, :4].abs()
    bs = N // 2
    c, u = mo[:bs, :4].repeat(2, 1, 1), mo[bs:, :4].repeat(2, 1, 1)
    if mut == "eps_row_n":                                      # the second half reads its own rows
        c, u = c.clone(), u.clone()
        c[bs:], u[bs:] = mo[bs:, :4], mo[bs:, :4]
    return u + g * (c - u), u.abs() + abs(g) * (c.abs() + u.abs())


def _row64(row):
    a_t, a_prev, sigma, s1m = (float(np.float32(v)) for v in row)
    y = (1.0 - a_prev) - sigma * sigma
    dirc = math.sqrt(y)
    ddirc = U24 * ((sigma * sigma + y) / (2.0 * dirc) + dirc)
    return math.sqrt(a_t), math.sqrt(a_prev), sigma, s1m, dirc, ddirc


def ddim_ref(d, row, use_cfg, noise, mut=None, dtype=torch.float64):
    """DDIM step (samplers.py:290-331) in `dtype` on the fp32 row -> (x_out, x0, bound_out, bound_x0)"""
    sq_at, sq_ap, sigma, s1m, dirc, ddirc = _row64(row)
    x, mo = d["x"].to(dtype), d["mo"].to(dtype)
    e, E = _guided(mo, use_cfg, float(np.float32(STEP_GUIDANCE)), mut)
    x0 = (x - s1m * e) / sq_at
    S0 = (x.abs() + s1m * E) / sq_at
    out = sq_ap * x0 + dirc * e
    S = sq_ap * S0 + dirc * E
    if noise and mut != "noise_dropped":
        out = out + sigma * d["noise"].to(dtype)
    if noise:
        S = S + abs(sigma) * d["noise"].to(dtype).abs()
    return out, x0, N_DDIM_OUT * U24 * S + 2 * ddirc * E, N_DDIM_X0 * U24 * S0


def plms_ref(d, row, use_cfg, order, mut=None, dtype=torch.float64):
    """PLMS step (samplers.py:566-637) -> (x_out, x0, e, bound_out, bound_x0, bound_e)"""
    sq_at, sq_ap, _, s1m, dirc, ddirc = _row64((row[0], row[1], 0.0, row[3]))      # eta = 0 enforced: the kernel does not read sigma
    x, mo = d["x"].to(dtype), d["mo"].to(dtype)
    h1, h2, h3 = (d[k].to(dtype) for k in ("h1", "h2", "h3"))
    e, E = _guided(mo, use_cfg, float(np.float32(STEP_GUIDANCE)))
    o = PLMS_NEIGHBOUR[order] if mut == "order_swapped" else order
    if o == 0:
        ep, EP = e, E
    elif o == 4:
        ep, EP = (h1 + e) / 2, (h1.abs() + E) / 2
    elif o == 1:
        ep, EP = (3 * e - h1) / 2, (3 * E + h1.abs()) / 2
    elif o == 2:
        ep, EP = (23 * e - 16 * h1 + 5 * h2) / 12, (23 * E + 16 * h1.abs() + 5 * h2.abs()) / 12
    else:
        ep, EP = (55 * e - 59 * h1 + 37 * h2 - 9 * h3) / 24, (55 * E + 59 * h1.abs() + 37 * h2.abs() + 9 * h3.abs()) / 24
    x0 = (x - s1m * ep) / sq_at
    S0 = (x.abs() + s1m * EP) / sq_at
    out = sq_ap * x0 + dirc * ep
    S = sq_ap * S0 + dirc * EP
    return out, x0, e, N_PLMS_OUT * U24 * S + 2 * ddirc * EP, N_PLMS_X0 * U24 * S0, (N_PLMS_E * U24 * E if use_cfg else torch.zeros_like(E))
