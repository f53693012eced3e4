"""Float64 restatements, inputs, mutants and bounds of the skinny-M family the 16-bit prior runs through (csrc/skinny.hip: skinny_kernel,
finish_ln_kernel, afrag_pack_kernel; csrc/attention.hip: small_attention_kernel), for tests/test_skinny_parity_cpu.py and
tests/test_skinny_parity_gpu.py.  A plain module like aux_ref.py, whose helpers (and helpers.py's, attention_ref.py's) it reuses unchanged.

Classes of check as in aux_ref.py (E exact / M measured constant).  Every buffer a launch writes is pre-filled (NaN, or 0xA5 bytes where bit
patterns are compared) and carries guards; an element the launch does not own must still hold the fill - that includes the padding rows
M .. 32 MA - 1 of every A-fragment tensor, which no producer writes.  A-fragment INPUTS carry NaN in those rows: the GEMM is correct only
because an MFMA output column depends on its own B column alone.

Layouts (E):  afrag_index = afrag_off of skinny.hip, [K/64][MA][4][64][8];  wfrag_index = skinny.h's Wf, [Npad/32][K/64][4][64][8]; in both
the lane of row r and k-value k is (r & 31) + 32 ((k >> 3) & 1), the k-step (k >> 4) & 3.

Skinny GEMM (M).  Operands as the kernel sees them (T-rounded A and W, fp32 bias); pre = A W^T (+ bias) in float64, S the same over absolute
values, ref = act64(pre):
    epilogues 0 / 1   |out - ref| <= L_act c 2^-24 S + rounding(ref, T) + e_act
    epilogue 2        |sum_z partial[z] - pre| <= c 2^-24 S (float64 sum, no bias), every element finite, an empty chunk range exactly 0
 c      helpers.IGEMM_C = 14.8, by the project's rule: the yardstick is torch's OWN fp32 matmul on the same operands against float64 in
        units of 2^-24 S, and IGEMM_C holds while the larger reading is at most 7.401.  MEASURED over all GEMM_CASES x families x types:
          CPU    (test_skinny_parity_cpu.py prints them)   rand 4.55   tagged 3.51   small_rows 3.99
          MI355X (test_skinny_parity_gpu.py prints them)   rand 5.55   tagged 4.25   small_rows 5.36   (fp16-rounded operands; bf16: 2.38 / 2.48 / 2.16)
        Largest 5.55 <= 7.401 -> c = IGEMM_C.  Never taken from the kernel; both tests assert torch's reading under c.
 e_act  for SiLU hp.act_eval_term.  For GELU the kernel evaluates gelu_fast (common.h):
            z = |x| 2^-0.5;  t = rcp(fma(0.3275911, z, 1));  poly = t (a1 + t (a2 + t (a3 + t (a4 + t a5))));  q = poly exp2(-z^2 log2 e);
            x >= 0: x fma(-0.5, q, 1)      x < 0: x (0.5 q)
        q is Abramowitz-Stegun 7.1.26 for erfc(z), published |error| <= 1.5e-7, and gelu(x) = x (1 - q / 2) resp. x q / 2: the polynomial
        contributes 0.5 * 1.5e-7 |x|.  The evaluation rounds 14 times - z, the fma, rcp (1 ulp), four fma and one product of the Horner
        form, z^2, its product with -log2 e, exp2 (1 ulp), poly * exp2, the last fma (or 0.5 q: exact), the product with x.  To first order,
        in units of 2^-24 and with every rounding at its worst: t carries 4 (z and the fma together at most 2 - z enters t through
        0.33 z / (1 + 0.33 z) < 1 - and 2 for the ulp of rcp), which |t d poly / d t| <= 3.45 on (0, 1] turns into 13.8 on poly; the five
        Horner steps add 7.5 (intermediates up to 1.5); the exponent's two roundings and the ulp of exp2 move q by q (2 z^2 + 2) <= 2.4
        (erfc(z) z^2 <= 0.17); the product poly * exp2 adds 1; the eight fp32 constants 4.5 (sum |a_i| + the two scales).  That is 29.2 on
        q <= 1, halved on the way to the result, plus the last two roundings on the result itself: 16.6.  k is therefore NOT the bare
        count of 14 (which the worst case exceeds) but this amplified total rounded up, k = 17:
            e_act = |pre| (0.5 * 1.5e-7 + 17 * 2^-24) = 1.09e-6 |pre|,
        three orders under the 16-bit rounding of the value it is added to.
        The CPU test evaluates an fp32 restatement of gelu_fast in torch (gelu_fast32) on a dense grid and on every GELU case and shows it
        inside the term (largest |gelu_fast32 - gelu64| / e_act over 200001 points of [-12, 12]: 0.25).

finish_ln.  x update (E): ((p0 + p1) + ... + p_{s-1}) + bias, then + x, IEEE fp32 additions that cannot be contracted - x_chain32 evaluates
them in torch fp32 in exactly that order and the device result is bit-equal.  LayerNorm output (M): aux_ref.layernorm_ref of the updated row,
c = AUX_C["layernorm"] = 8.92 and S as documented there, plus rounding(ref, T).  Torch's fp32 F.layer_norm on FLN_CASES' rows (every row
kind below) reads at most 2.69 on the CPU and 1.90 on the MI355X, under the 4.458 that set the constant: it covers this kernel unchanged.

small_attention (M).  q, k, v are the T values the kernel stages: the stored qkv, or T(((p0 + p1) + ...) + bias), the split-K finish folded
into its loads (att_stage32: fp32 in split order, bias last, one rounding).  attention_ref.attention_ref and attention_ref.bound are reused
unchanged with Case(B, H, T, 0, causal, n_valid, kv_n): the kernel's arithmetic is attention_kernel's (lane-local fp32 softmax over fp32
scores, P rounded to T in front of P V, the row sum over the unrounded P), in one tile.  c = ATT_C = 4; torch's fp32 softmax(q k^T / 8 +
mask) v on ATT_CASES reads at most 1.17 (CPU) and 1.24 (MI355X).
Precondition (documented, not tested): a query with no live key gives NaN in the reference too; every case keeps key 0 valid.

Input families.  GEMM: rand (activations 0.3 + 1.7 randn, weights K^-0.5 randn); tagged (every 64-chunk - a factor that does not repeat within a case -, 16-wide k-step and 8-wide lane
half of K scales A by its own factor: a dropped, doubled or misassigned piece shows); small_rows (every third token row and every fifth weight
row, with its bias, scaled by 2^-6: what a max-normalised tolerance hides).  finish_ln: the updated row m is of kind m % 5 - random, mean =
10 sd, one dominant element, mean = 3000 sd (only there does a one-pass fp32 variance leave the 16-bit rounding), sd = 1e-4 around 0.5
(variance << eps).  Attention: attention_ref's rand, edges, neg.

Mutants: GEMM_MUTANTS, FLN_MUTANTS, ATT_MUTANTS below, one deliberate mistake each; the CPU test shows each outside the bound in both types.

MEASURED on the MI355X (test_skinny_parity_gpu.py prints them), largest |out - ref| / bound over all cases and families, kernel | torch's
own fp32 evaluation of the same operation rounded to T.  A T output that is exact up to its one rounding reads up to 1.0 (the rounding term
is the whole budget of an element just above a power of two), so the 16-bit rows say "one rounding", as torch's do:
    skinny epilogue 0      bf16 0.995 | 0.995    fp16 0.990 | 0.990
    skinny epilogue 1      bf16 0.991 | 0.991    fp16 0.995 | 0.995
    skinny epilogue 2      bf16 0.062 | 0.094    fp16 0.069 | 0.211   (fp32 partials: the accumulation term alone)
    finish_ln x update     bit-equal to x_chain32 on every case
    finish_ln LayerNorm    bf16 0.995 | 0.995    fp16 0.993 | 0.993
    small_attention        bf16 0.780 | 0.496    fp16 0.766 | 0.494
    one-block chain        bf16 0.991            fp16 0.992           (largest over its eight stages)
"""
import collections

import torch
import torch.nn.functional as F

import attention_ref as atr
import aux_ref as ar
import helpers as hp
from kandinsky2_amd import _lib

BF16, F16 = _lib.K22_BF16, _lib.K22_F16
DTYPES = (BF16, F16)
DT_NAME = hp.DT_NAME
U24 = hp.U24
L_ACT = hp.IGEMM_L_ACT
NAN = ar.NAN
ACT_NONE, ACT_SILU, ACT_GELU = _lib.ACT_NONE, _lib.ACT_SILU, _lib.ACT_GELU
EPI_ROWMAJOR, EPI_AFRAG, EPI_PARTIAL = 0, 1, 2

# the rule applied to the larger of the CPU and the MI355X reading (table above)
GEMM_YARD_CPU, GEMM_YARD_GPU = 4.55, 5.55
assert max(GEMM_YARD_CPU, GEMM_YARD_GPU) <= 7.401
GEMM_C = hp.IGEMM_C
LN_C = ar.AUX_C["layernorm"]
ATT_C = atr.ATT_C
GELU_K = 17
GELU_FAST_REL = 0.5 * 1.5e-7 + GELU_K * U24


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------
def afrag_index(M, K, device="cpu"):
    """flat element offset of (m, k) in the A-fragment tensor [K/64][MA][4][64][8] (skinny.hip: afrag_off) -> [M][K]"""
    MA = (M + 31) // 32
    m = torch.arange(M, device=device)[:, None]
    k = torch.arange(K, device=device)[None, :]
    return ((((k >> 6) * MA + (m >> 5)) * 4 + ((k >> 4) & 3)) * 64 + (m & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7)


def wfrag_index(Npad, K, device="cpu"):
    """flat element offset of (n, k) in the weight tensor [Npad/32][K/64][4][64][8] (skinny.h: Wf) -> [Npad][K]"""
    n = torch.arange(Npad, device=device)[:, None]
    k = torch.arange(K, device=device)[None, :]
    return ((((n >> 5) * (K >> 6) + (k >> 6)) * 4 + ((k >> 4) & 3)) * 64 + (n & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7)


def afrag_elems(M, K):
    return (M + 31) // 32 * 32 * K


def from_afrag(buf, M, K):
    return buf.reshape(-1)[afrag_index(M, K, buf.device).reshape(-1)].reshape(M, K)


def afrag_expected(v, fill=NAN):
    """[M][K] values -> the flat A-fragment buffer: owned positions hold the value, the padding rows the fill"""
    M, K = v.shape
    out = torch.full((afrag_elems(M, K),), fill, dtype=v.dtype, device=v.device)
    out[afrag_index(M, K, v.device).reshape(-1)] = v.reshape(-1)
    return out


def rowmajor_expected(v, ldo, fill=NAN, mut=None):
    """[M][N] values -> [M][ldo]: the columns between N and ldo hold the fill"""
    M, N = v.shape
    out = torch.full((M, ldo), fill, dtype=v.dtype, device=v.device)
    if mut == "ldo_as_N":
        idx = torch.arange(M, device=v.device)[:, None] * N + torch.arange(N, device=v.device)[None, :]
        out.view(-1)[idx.reshape(-1)] = v.reshape(-1)
    else:
        out[:, :N] = v
    return out


# ---- skinny GEMM ------------------------------------------------------------------------------------------------------------------------
GemmCase = collections.namedtuple("GemmCase", "M N K splitk epi act bias mt nb slack")
TILES = ((6, 1), (3, 4), (3, 2), (3, 1), (2, 2), (2, 1), (1, 2))


def G(M, N, K, splitk, epi, cfg, act=ACT_NONE, bias=1, slack=0):
    return GemmCase(M, N, K, splitk, epi, act, bias, cfg[0], cfg[1], slack)


# chunk ranges per split, D the tile's ring depth (6 for (6,1), else 8): 1 (K = 64), D - 1, D, D + 1, 2 D + (D - 1); 2, 2, 1, 0 (nchunks 5,
# splitk 4: the empty last split); 5, 4 (nchunks 9, splitk 2).  M 193 with mt = 3 / 6, 97 with mt = 3, 96 with mt = 2: a short last m-tile.
GEMM_CASES = [
    # (1,2)
    G(1, 4, 64, 1, 0, (1, 2)), G(31, 60, 448, 1, 0, (1, 2), ACT_GELU), G(32, 64, 512, 1, 1, (1, 2), ACT_GELU),
    G(97, 200, 576, 1, 0, (1, 2), bias=0), G(162, 64, 1472, 1, 1, (1, 2), ACT_GELU), G(33, 68, 896, 2, 2, (1, 2)),
    # (2,1)
    G(33, 68, 576, 1, 0, (2, 1), ACT_SILU, slack=12), G(33, 64, 1472, 1, 1, (2, 1), bias=0), G(32, 4, 512, 1, 0, (2, 1), ACT_SILU),
    G(193, 64, 64, 1, 1, (2, 1), ACT_GELU), G(31, 200, 320, 4, 2, (2, 1)), G(162, 60, 896, 2, 2, (2, 1)),
    # (2,2)
    G(33, 200, 512, 1, 0, (2, 2), ACT_GELU), G(97, 64, 1472, 1, 1, (2, 2)), G(1, 60, 576, 2, 2, (2, 2)),
    G(96, 68, 448, 1, 0, (2, 2), slack=12), G(31, 4, 64, 1, 0, (2, 2)), G(162, 200, 1152, 2, 2, (2, 2)),
    # (3,1)
    G(96, 200, 64, 1, 0, (3, 1)), G(97, 200, 512, 1, 0, (3, 1), ACT_GELU, slack=12), G(97, 64, 1152, 2, 2, (3, 1)),
    G(162, 68, 448, 1, 0, (3, 1)), G(193, 64, 1472, 1, 1, (3, 1), ACT_GELU),
    # (3,2)
    G(162, 200, 896, 2, 2, (3, 2)), G(193, 68, 512, 1, 0, (3, 2), bias=0), G(193, 64, 1472, 1, 1, (3, 2), ACT_GELU),
    G(193, 200, 320, 4, 2, (3, 2)), G(162, 64, 576, 2, 2, (3, 2)), G(32, 64, 64, 1, 2, (3, 2)), G(33, 60, 576, 1, 0, (3, 2), ACT_SILU),
    # (3,4): weights padded to a multiple of 128 rows
    G(193, 200, 512, 1, 0, (3, 4), ACT_GELU, slack=12), G(97, 64, 448, 1, 1, (3, 4), ACT_SILU), G(33, 60, 320, 4, 2, (3, 4)),
    G(162, 4, 1472, 1, 0, (3, 4)), G(96, 200, 1152, 2, 2, (3, 4)), G(31, 64, 64, 1, 1, (3, 4), bias=0),
    # (6,1): ring depth 6
    G(162, 64, 320, 1, 0, (6, 1), ACT_GELU), G(193, 60, 384, 1, 0, (6, 1), slack=12), G(193, 64, 448, 1, 1, (6, 1), ACT_GELU),
    G(162, 200, 1088, 1, 0, (6, 1), ACT_SILU, bias=0), G(31, 68, 64, 1, 0, (6, 1)), G(97, 64, 320, 4, 2, (6, 1)),
    G(193, 200, 768, 2, 2, (6, 1)),
    # the default tile
    G(1, 64, 64, 1, 0, (0, 0), ACT_GELU), G(162, 200, 512, 1, 0, (0, 0), slack=12), G(193, 64, 576, 1, 1, (0, 0), ACT_GELU),
    G(97, 60, 320, 4, 2, (0, 0)), G(33, 4, 1472, 1, 0, (0, 0)),
]
GEMM_FAMILIES = ("rand", "tagged", "small_rows")
GEMM_MUTANTS = ("chunk_dropped", "chunk_doubled", "kstep_swap", "half_swap", "row_dropped", "pad_row_added", "bias_shift4",
                "bias_tail_missing", "act_before_bias", "act_missing", "ldo_as_N")


def gemm_id(c):
    s = f"{c.M}x{c.N}x{c.K}-sk{c.splitk}-epi{c.epi}-t{c.mt}x{c.nb}"
    return s + (f"-act{c.act}" if c.act else "") + ("" if c.bias else "-nobias") + (f"-ldo+{c.slack}" if c.slack else "")


def npad(c):
    mult = 128 if c.nb == 4 else 64
    return (c.N + mult - 1) // mult * mult


def ring_depth(c):
    return 6 if (c.mt, c.nb) == (6, 1) else 8


def chunk_ranges(K, splitk):
    """[(c0, c1)] per split as skinny_kernel derives them; c0 >= c1: an empty range"""
    nchunks = K // 64
    per = (nchunks + splitk - 1) // splitk
    return [(z * per, min(z * per + per, nchunks)) for z in range(splitk)]


def gemm_inputs(c, family):
    """fp32 CPU operands: a [M][K], w [N][K], bias [N] or None"""
    g = ar.gen(9000 + 7 * c.M + 3 * c.N + c.K + 11 * c.splitk + GEMM_FAMILIES.index(family))
    a, w, bias = ar.acts(g, c.M, c.K), c.K ** -0.5 * ar.rn(g, c.N, c.K), ar.rn(g, c.N)
    if family == "tagged":
        k = torch.arange(c.K)
        assert c.K // 64 <= 32                                  # the chunk factor must not repeat within a case
        a = a * ((1.0 + 0.09375 * (k >> 6)) * (1.0 + 0.25 * ((k >> 4) & 3)) * (1.0 + 0.125 * ((k >> 3) & 1)))
    elif family == "small_rows":
        a[1::3] *= 2.0 ** -6
        a[c.M - 1] *= 2.0 ** -6
        w[2::5] *= 2.0 ** -6
        bias[2::5] *= 2.0 ** -6
    else:
        assert family == "rand", family
    return {"a": a, "w": w, "bias": bias if c.bias else None}


def gemm_seen(d, dtype, f64=True):
    """the operand values the kernel is promised to see (any device): T-rounded a and w, the fp32 bias"""
    up = (lambda t: t.double()) if f64 else (lambda t: t.float())
    return {"a": up(ar.rounded(d["a"], dtype)), "w": up(ar.rounded(d["w"], dtype)), "bias": None if d["bias"] is None else up(d["bias"])}


def gelu_fast32(x):
    """fp32 restatement of common.h's gelu_fast in torch (1 / x and torch.exp2 for the hardware rcp / exp2)"""
    x = x.float()
    z = x.abs() * 0.70710678118654752
    t = 1.0 / (0.3275911 * z + 1.0)
    poly = t * (t * (t * (t * (t * 1.061405429 + -1.453152027) + 1.421413741) + -0.284496736) + 0.254829592)
    q = poly * torch.exp2(z * z * -1.4426950408889634)
    return torch.where(x >= 0, x * (-0.5 * q + 1.0), x * (0.5 * q))


def act_any(x, act):
    """the activation in x's precision: float64 by definition, fp32 as torch (GELU: the gelu_fast restatement)"""
    if x.dtype == torch.float64:
        return hp.act64(x, act)
    if act == ACT_GELU:
        return gelu_fast32(x)
    return F.silu(x) if act == ACT_SILU else x


def gemm_ref(s, c, mut=None):
    """the operation over the seen operands s (float64: the reference; float32: torch's own evaluation), written from the definition with
    the kernel's split of K -> dict: parts [splitk][M][N] (no bias), pre = sum of parts (+ bias), S the same over absolute values (float64
    only), ref = act(pre)"""
    a, w, bias = s["a"], s["w"], s["bias"]
    nchunks = c.K // 64
    if mut in ("kstep_swap", "half_swap"):                      # A's k-steps / lane halves exchanged within every chunk, W's not
        a = a[:, torch.arange(c.K, device=a.device) ^ (16 if mut == "kstep_swap" else 8)]
    parts, S = [], torch.zeros(c.M, c.N, dtype=a.dtype, device=a.device)
    for z, (c0, c1) in enumerate(chunk_ranges(c.K, c.splitk)):
        cols = torch.arange(64 * c0, 64 * max(c0, c1), device=a.device)
        if mut == "chunk_dropped" and z == 0:                   # the last chunk of the range never reaches the MFMAs
            cols = cols[:-64]
        if mut == "chunk_doubled" and z == 0 and c1 < nchunks:  # the first chunk of the next range too
            cols = torch.cat([cols, torch.arange(64 * c1, 64 * c1 + 64, device=a.device)])
        p = a[:, cols] @ w[:, cols].T
        if mut == "row_dropped":
            p[c.M - 1] = 0
        if mut == "pad_row_added" and z == 0 and c.M % 32:      # a padding row of ones lands in row M - 1
            p[c.M - 1] += w.sum(1)
        parts.append(p)
        S = S + a[:, cols].abs() @ w[:, cols].abs().T
    parts = torch.stack(parts)
    acc = parts.sum(0)
    if c.epi == EPI_PARTIAL or bias is None:
        return {"parts": parts, "pre": acc, "S": S, "ref": acc if c.epi == EPI_PARTIAL or mut == "act_missing" else act_any(acc, c.act)}
    if mut == "bias_shift4":
        bias = torch.roll(bias, 4)
    if mut == "bias_tail_missing":
        bias = bias.clone()
        bias[c.N - 4:] = 0
    pre = acc + bias
    if mut == "act_before_bias":
        ref = act_any(acc, c.act) + bias
    else:
        ref = pre if mut == "act_missing" else act_any(pre, c.act)
    return {"parts": parts, "pre": pre, "S": S + bias.abs(), "ref": ref}


def gemm_e_act(pre, act):
    if act == ACT_GELU:
        return pre.abs() * GELU_FAST_REL
    return hp.act_eval_term(pre, act)


def gemm_bound(r, c, dtype, cc=GEMM_C):
    """per-element bound of epilogues 0 / 1 on r["ref"], of epilogue 2 on the float64 sum of the partials"""
    if c.epi == EPI_PARTIAL:
        return cc * U24 * r["S"]
    return (L_ACT if c.act else 1.0) * cc * U24 * r["S"] + ar.rounding(r["ref"], dtype) + gemm_e_act(r["pre"], c.act)


def gemm_layout(v, c, fill=NAN, mut=None):
    """[M][N] -> the flat buffer of the case's epilogue (0 / 1)"""
    if c.epi == EPI_AFRAG:
        return afrag_expected(v, fill)
    return rowmajor_expected(v, c.N + c.slack, fill, mut).reshape(-1)


# ---- finish_ln --------------------------------------------------------------------------------------------------------------------------
FlnCase = collections.namedtuple("FlnCase", "M N splitk slack ln bias")     # splitk 0: partial == NULL (LayerNorm only)
FLN_CASES = [
    FlnCase(1, 8, 1, 0, 0, 1), FlnCase(5, 72, 2, 4, 0, 0), FlnCase(33, 2040, 7, 4, 0, 1), FlnCase(33, 8, 8, 4, 0, 1), FlnCase(1, 2040, 2, 0, 0, 0),
    FlnCase(5, 512, 1, 0, 0, 1), FlnCase(5, 64, 0, 0, 1, 0), FlnCase(33, 64, 8, 4, 1, 1), FlnCase(1, 512, 2, 0, 1, 0), FlnCase(33, 512, 7, 4, 1, 1),
    FlnCase(5, 2048, 8, 0, 1, 1), FlnCase(33, 2048, 0, 4, 1, 0), FlnCase(5, 2048, 1, 4, 1, 0), FlnCase(33, 2048, 2, 0, 1, 1),
]
FLN_MUTANTS = ("last_split_missing", "last_split_twice", "bias_missing", "div2048", "one_pass", "eps_missing", "gb_shift8", "x_not_written")
FLN_EPS = 1e-5


def fln_id(c):
    return f"{c.M}x{c.N}-sk{c.splitk}-ldx+{c.slack}" + ("-ln" if c.ln else "") + ("-bias" if c.bias else "")


def fln_inputs(c):
    """fp32 CPU: x [M][N], partial [splitk][M][N] or None, bias or None, g, b.  The UPDATED row m is of kind m % 5 (module docstring)."""
    g = ar.gen(9500 + 13 * c.M + c.N + 5 * c.splitk)
    y = ar.acts(g, c.M, c.N)
    for m in range(c.M):
        kind = m % 5
        if kind == 1:
            y[m] = 17.0 + 1.7 * ar.rn(g, c.N)
        elif kind == 2:
            y[m, (7 * m) % c.N] = 100.0
        elif kind == 3:
            y[m] = 3000.0 + ar.rn(g, c.N)
        elif kind == 4:
            y[m] = 0.5 + 1e-4 * ar.rn(g, c.N)
    d = {"partial": None, "bias": None, "g": 1.0 + 0.3 * ar.rn(g, c.N), "b": 0.5 * ar.rn(g, c.N)}
    if c.splitk:
        d["partial"] = ar.rn(g, c.splitk, c.M, c.N) * c.splitk ** -0.5
        d["bias"] = ar.rn(g, c.N) if c.bias else None
        y = y - x_chain32({"x": torch.zeros_like(y), "partial": d["partial"], "bias": d["bias"]})
    d["x"] = y
    return d


def x_chain32(d, mut=None):
    """the kernel's fp32 additions in its order: ((p0 + p1) + ... + p_{s-1}) + bias, then + x.  fp32 tensors in, fp32 out."""
    x, p, bias = d["x"], d["partial"], d["bias"]
    if p is None or mut == "x_not_written":
        return x.clone()
    n = p.shape[0] - 1 if mut == "last_split_missing" else p.shape[0]
    acc = p[0].clone() if n else torch.zeros_like(p[0])
    for s in range(1, n):
        acc = acc + p[s]
    if mut == "last_split_twice":                               # the clamp's re-read of the last split, added
        acc = acc + p[-1]
    if bias is not None and mut != "bias_missing":
        acc = acc + bias
    return acc + x


def fln_ln_ref(xu, g, b, eps=FLN_EPS, mut=None):
    """LayerNorm of the updated rows -> (ref, S): aux_ref.layernorm_ref unchanged; the mutants restate it with their mistake"""
    if mut not in ("div2048", "one_pass", "eps_missing", "gb_shift8"):
        return ar.layernorm_ref(xu, g, b, eps)
    den = 2048 if mut == "div2048" else xu.shape[-1]
    mu = xu.sum(-1, keepdim=True) / den
    dlt = xu - mu
    var = (dlt * dlt).sum(-1, keepdim=True) / den
    if mut == "one_pass":                                       # E[x^2] - mean^2 in fp32
        x32 = xu.float()
        var = ((x32 * x32).mean(-1, keepdim=True) - x32.mean(-1, keepdim=True) ** 2).to(xu.dtype)
    if mut == "gb_shift8":
        g, b = torch.roll(g, 8), torch.roll(b, 8)
    return dlt * (var + (0.0 if mut == "eps_missing" else eps)).rsqrt() * g + b, None


def fln_bound(ref, S, dtype, cc=LN_C):
    return cc * U24 * S + ar.rounding(ref, dtype)


# ---- small_attention --------------------------------------------------------------------------------------------------------------------
AttCase = collections.namedtuple("AttCase", "B H T causal n_valid kv_n frag nsplit")   # n_valid None: no key_valid tensor
ATT_CASES = [
    AttCase(1, 1, 1, 0, None, 0, 0, 0), AttCase(3, 1, 1, 1, 1, 1, 1, 1), AttCase(1, 3, 31, 1, 20, 31, 1, 2), AttCase(3, 1, 32, 0, None, 0, 0, 4),
    AttCase(3, 3, 33, 1, 20, 30, 1, 0), AttCase(1, 1, 64, 1, 9, 64, 0, 1), AttCase(3, 1, 65, 0, 40, 60, 1, 4), AttCase(3, 3, 81, 1, 40, 77, 1, 2),
    AttCase(1, 3, 96, 0, None, 0, 1, 0), AttCase(3, 1, 97, 1, 50, 97, 0, 4), AttCase(1, 1, 127, 1, 100, 120, 1, 1), AttCase(3, 3, 128, 1, 100, 128, 0, 2),
    AttCase(1, 3, 128, 0, None, 0, 1, 0),
]
ATT_FAMILIES = atr.FAMILIES
ATT_MUTANTS = ("causal_strict", "causal_plus1", "one_pad_key_alive", "kvn_ignored", "last_key_dropped", "bias_wrong_plane", "last_partial_twice",
               "valid_next_image")
_ATR_MUTANTS = ("causal_strict", "causal_plus1", "one_pad_key_alive", "kvn_ignored", "last_key_dropped")


def att_id(c):
    s = f"B{c.B}H{c.H}T{c.T}" + ("-causal" if c.causal else "") + (f"-nv{c.n_valid}-kvn{c.kv_n}" if c.n_valid is not None else "")
    return s + ("-frag" if c.frag else "") + f"-ns{c.nsplit}"


def att_case(c):
    return atr.Case(c.B, c.H, c.T, 0, c.causal, c.n_valid, c.kv_n)


def att_inputs(c, family):
    """attention_ref.inputs of the case (qkv [B][T][3][H][64], key_valid) and, for nsplit > 0, fp32 partials [nsplit][B * T][3 C] + bias
    [3 C] whose finish is (up to fp32 rounding) that qkv: every partial carries 1 / nsplit of it plus noise, the last one the remainder"""
    d = atr.inputs(att_case(c), family)
    d["part"] = d["bias"] = None
    if c.nsplit:
        g = ar.gen(9700 + c.T + 3 * c.nsplit)
        flat = d["qkv"].reshape(c.B * c.T, 3 * c.H * atr.HD)
        d["bias"] = 0.5 * ar.rn(g, flat.shape[1])
        parts = [flat / c.nsplit + 0.3 * ar.rn(g, *flat.shape) for _ in range(c.nsplit - 1)]
        rest = flat - d["bias"]
        for p in parts:
            rest = rest - p
        d["part"] = torch.stack(parts + [rest]).contiguous()
    return d


def att_stage32(d, c, dtype, mut=None):
    """the T values the kernel stages, as fp32 [B][T][3][H][64]: the stored qkv, or T(((p0 + p1) + ...) + bias) in fp32"""
    if not c.nsplit:
        return ar.rounded(d["qkv"], dtype)
    p, bias = d["part"], d["bias"]
    acc = p[0].clone()
    for s in range(1, c.nsplit):
        acc = acc + p[s]
    if mut == "last_partial_twice":
        acc = acc + p[-1]
    if mut == "bias_wrong_plane":                               # `which * C` omitted: K and V take the Q plane's bias
        bias = bias[:c.H * atr.HD].repeat(3)
    return ar.rounded(acc + bias, dtype).view(c.B, c.T, 3, c.H, atr.HD)


def att_operands(stage32):
    """fp32 [B][T][3][H][64] -> float64 q, k, v [B][H][T][64]"""
    x = stage32.double()
    return tuple(x[:, :, i].permute(0, 2, 1, 3).contiguous() for i in range(3))


def att_ref(q, k, v, c, valid, dtype, mut=None):
    """-> (ref, bound, A, amp), [B * T][H * 64]: attention_ref.attention_ref / bound unchanged"""
    if mut == "valid_next_image" and valid is not None:          # `b * kv_ld` wrong: image b reads the row of image b + 1
        valid = torch.roll(valid, -1, 0)
    info = {}
    ref, A, amp = atr.attention_ref(q, k, v, att_case(c), valid, mut if mut in _ATR_MUTANTS else None, info)
    return ref, atr.bound(ref, A, amp, info["vsum_over_l"], dtype), A, amp


def att_layout(v, c, fill=NAN):
    return afrag_expected(v, fill) if c.frag else v.reshape(-1)


# ---- the one-block chain (prior.hip: the skinny branch of the transformer loop) -----------------------------------------------------------
CHAIN = {"D": 128, "H": 2, "T": 17, "B": 2, "kv_n": 13, "n_valid": 9, "sk_qkv": 2, "sk_proj": 2, "sk_fc2": 4, "tile": (2, 2)}


def chain_inputs():
    g = ar.gen(9900)
    D, M = CHAIN["D"], CHAIN["B"] * CHAIN["T"]
    d = {"x": ar.acts(g, M, D)}
    for name, (n, k) in {"qkv": (3 * D, D), "proj": (D, D), "fc": (4 * D, D), "fc2": (D, 4 * D)}.items():
        d["w_" + name], d["b_" + name] = k ** -0.5 * ar.rn(g, n, k), 0.3 * ar.rn(g, n)
    for name in ("ln1", "ln2"):
        d["g_" + name], d["be_" + name] = 1.0 + 0.3 * ar.rn(g, D), 0.5 * ar.rn(g, D)
    d["valid"] = atr.key_valid(atr.Case(CHAIN["B"], CHAIN["H"], CHAIN["T"], 0, 1, CHAIN["n_valid"], CHAIN["kv_n"]))
    return d
