"""Float64 restatements, inputs and bounds of the UNet's GroupNorm32 kernels (csrc/elementwise.hip: gn_stats_kernel, gn_coeff_kernel,
gn_apply_kernel), for tests/test_gn_parity_cpu.py and tests/test_gn_parity_gpu.py.  A plain module like aux_ref.py, whose bound classes
(E exact / D derived) and helpers it uses.

Written from the operation's definition - GroupNorm32.forward (kandinsky2/model/nn.py:26-37: fp32 statistics over 32 groups, biased
variance, eps inside the square root, then SiLU), the scale-shift use of it in ResBlock (unet.py:212-216: GN(h) * (1 + scale) + shift before
the activation) - and from what csrc/elementwise.h / elementwise.hip's comments promise about the three passes and their buffers, not from
the kernels' code.  Tensors are NHWC; `x` is always the T-rounded tensor a kernel is promised to see (fp32 for the split dtypes).

STAGES AND BOUNDS (u = 2^-24; "n" is TWICE the number of roundings on the longest path, FMA contraction only removes roundings)

 statistics (D)  partial [B][nsplit][C][2]: row s of image b holds the (sum, sum of squares) of pixel range s, ranges of
    per = ceil(HW / nsplit) pixels.  The rows are summed over s in float64 and compared per (image, channel) with the float64 sums:
        |sum - ref| <= n u sum|x|,   |sumsq - ref| <= n u sum x^2.
    Longest path of one range: 256 threads own C / 4 four-channel vectors; with fewer than 256 vectors PL = 256 / (C / 4) pixel lanes
    share the range, a lane walks Lp = ceil(per / PL) pixels.  Eight pixels at a time are added as a balanced tree (3 roundings) and the
    tree's value is added to the running sum (1 rounding per step: Lp / 8 chain steps); the Lp % 8 pixels left are added one by one
    (1 each); the PL lane sums are added in order (PL roundings, counted even though the first is an add to zero); a square is rounded
    once before it enters its sum.  roundings = Lp / 8 + (3 if Lp >= 8) + Lp % 8 + (PL if PL > 1) + 1,  n = 2 x that (stats_n).
    E: rows of a range that starts at or behind HW are exactly 0; nothing outside [B][nsplit][C][2] changes (NaN fill, guards).

 coefficients (D), conditioned on the partial sums they are GIVEN: the reference is float64 arithmetic on the fp32 rows the test supplied -
    per-group sums over both sources, mean = s / n, var = max(q / n - mean^2, 0), rstd = (var + eps)^-1/2 with eps the fp32 value handed
    over, A0 = rstd gamma, Bc0 = beta - mean A0, and with FiLM  A = A0 (1 + scale),  Bc = Bc0 (1 + scale) + shift.
    The kernel sums in float64, rounds mean and rstd to fp32 once each and evaluates the rest in fp32:
        A:   rstd (1), rstd gamma (1), 1 + scale (1), A0 (1 + scale) (1)                                    = 4   -> N_A = 8
        Bc:  mean (1) x A0 (2), the product (1), beta - . (1), 1 + scale (1), . (1 + scale) (1), + shift (1)  = 8   -> N_BC = 16
        |A - ref| <= (N_A u + 2^-40) |A|,   |Bc - ref| <= (N_BC u + 2^-40) ((|beta| + |mean A0|) |1 + scale| + |shift|).
    CONDITION OF THE INPUTS: mean^2 / var <= 2^10 in every group of the supplied sums (coeff_conditioned), so that the float64
    cancellation in q / n - mean^2 (2^-53 (q / n + mean^2) / var <= 2^-42, a few operations) stays below the 2^-40 written above.
    Torch's "own fp32 evaluation" of this stage keeps the float64 sums (a fp32 sum of 2400 rows is not what the pass promises) and does
    everything after the two roundings in fp32.

 apply (D + L_act / e_act), GIVEN the coefficients:  ref = border(resample(act(x A + Bc))) in float64 on x and the fp32 coefficients.
        pre = x A + Bc: product, sum = 2 roundings -> 4 u (|x A| + |Bc|);  through SiLU: L_act x that + e_act;
        avgpool: the mean of the four bounds + three additions, 6 u x 0.25 sum|act| (the multiply by 0.25 is exact);
        + one rounding to the stored type (aux_ref.rounding: u_out |ref|, fp16 floored at 2^-25); the x3 store is read back as hi + lo
        (helpers.x3_value) with 2^-22 |ref| floored at 2^-25.
    e_act, IEEE SiLU (bf16 / fp16 / fp32 stores): 4 x torch's own fp32 SiLU error on the same pre-activations (helpers.act_eval_term).
    e_act, x3 store: its SiLU is x * rcp(1 + exp2(x * -log2 e)) on the native exp2 / rcp (common.h), both accurate to 1 ulp = 2 u:
        t = fl(x fl(-log2 e)) carries 2 u |t|, i.e. 2 u |x| RELATIVE on e = 2^t (d 2^t / 2^t = ln 2 dt);  exp2 itself 2 u;  an error on e
        reaches 1 / (1 + e) = s scaled by e / (1 + e) = 1 - s;  1 + e rounds once (u), rcp 2 u, the final product u:
            |y - x s| / |x s|  <=  u ((1 - s) (2 |x| + 2) + 4),   taken twice like every n here (silu_fast_term, element by element).
    E: with pad = 1 the border is exactly zero; the guards keep their fill; with act = 0 the nearest upsample (mode 2) gives every output
    the bits of its source pixel's mode-0 value.

 end to end (k22_groupnorm and the producer chains):  ref = the float64 GroupNorm of the T-rounded tensor;  bound = the apply bound, with
    the pre-activation error widened by the coefficient bound (|x| bA + bBc) and by the statistics bound pushed through mean and rstd to
    first order, all in float64 (e2e_ref):  ds, dq = the per-channel statistics bounds summed over the group,
        dmean = ds / n,  dvar = dq / n + 2 |mean| dmean,  drstd = rstd^3 dvar / 2,  dpre = |gamma (1 + scale)| (rstd dmean + |x - mean| drstd).
    Conditioning enters through this formula only: a group with |mean| = 16 std gets a dvar 16 - 32 times larger and is never asked for
    more than fp32 sums of x and x^2 can deliver.  Producer-side sums (conv / GEMM epilogues) use the constant their own tests use
    (helpers.IGEMM_C) in place of stats_n.

INPUT FAMILIES (seeded, small; x_family / film_b)
  a  channel c of image b has mean 0.3 + 0.05 c + 2 b and sd mean / 8 x (1 + (c % 5) / 4): a wrong image row, a wrong source or a group
     boundary off by one channel moves the group's mean by far more than any bound; mean^2 / var <= 64 in every group
  b  FiLM rows inside a wider row: film_ld = 2 C + 192, the pointer 64 floats into the buffer, NaN in every column the launch does not
     own, scale and shift different per image
  c  family a plus a ramp along x and y (0.37 sd and 0.23 sd per pixel): a wrong source pixel, an exchanged index or a border one pixel in
  d  |mean| / std = 16 in every group
  e  family a with group 3 nearly constant (0.01 + 0.001 randn): eps decides its rstd

MEASURED largest |error| / bound, per stage (the bounds above were fixed before any of these was read; CPU = torch's fp32 evaluation in
test_gn_parity_cpu.py part (b), MI355X = test_gn_parity_gpu.py's printed lines: kernel, and torch's fp32 evaluation on the device):
                              bf16     fp16     fp32     x3       x2
  statistics   CPU torch      0.093    0.388    0.359
               MI355X kernel  0.093    0.187    0.200
               MI355X torch   0.093    0.187    0.235
  coefficients CPU fp32 eval  0.408 (largest over the three input roundings)
               MI355X kernel  0.378    0.388    0.408    (inputs rounded to that type; the rows and the output are fp32 in all three)
  apply        CPU torch      0.996    0.995    0.366    0.231    0.231
               MI355X kernel  0.996    0.995    0.191    0.472    0.472
               MI355X torch   0.996    0.995    0.366    0.231    0.231
  end to end   CPU torch      0.987    0.955    0.128    0.129    0.129
  k22_groupnorm MI355X kernel 0.987    0.955    0.050    0.050    0.050
               MI355X torch   0.987    0.955    0.043    0.043    0.043
  chain conv -> coeff -> apply, producer route / stand-alone route (MI355X kernels):
               128 -> 128           0.984 / 0.984   0.978 / 0.976   0.080 / 0.062
               128 | conv 256       0.991 / 0.991   0.975 / 0.973   0.059 / 0.053
               128 | gemm 256       0.987 / 0.987   0.978 / 0.978   0.060 / 0.054
    (rows per image 1 | 2 from the producers, 4 from the stand-alone pass; the two routes' coefficients differ by <= 3.1e-5 absolute,
    <= 1.9e-5 relative - they are sums of the same values in another order and are not compared bit for bit.)
  The 16-bit figures near 1 are the output rounding itself (one rounding of the stored type is the bound's leading term there and a value
  just above a power of two uses all of it); everything that is not the store - the fp32 and x3 columns - sits at or under 0.47.  The x3
  apply reads above torch (0.47 against 0.23) because its SiLU runs on the native exp2 / rcp; the bound's term for that was derived, above,
  before the figure was read.  No kernel ratio exceeds 1 anywhere: no finding.
"""
import torch
import torch.nn.functional as F

import aux_ref as ar
import helpers as hp
from kandinsky2_amd import _lib

BF16, F16, F32, X3, X2 = _lib.K22_BF16, _lib.K22_F16, _lib.K22_F32, _lib.K22_F16X3, _lib.K22_F16X2
DTYPES = (BF16, F16, F32)               # storage types of the statistics pass and of the 16-bit / fp32 apply
APPLY_DTYPES = DTYPES + (X3, X2)        # + the fp32 apply kernel with the x3-chunk store
DT_NAME = hp.DT_NAME
U24 = hp.U24
L_ACT = hp.IGEMM_L_ACT
GROUPS = 32
N_A, N_BC, N_PRE, N_POOL = 8, 16, 4, 6
CANCEL = 2.0 ** -40
COND_MAX = 2.0 ** 10
SILU = _lib.ACT_SILU


def storage(dtype):
    return F32 if dtype in hp.X_DTYPES else dtype


def rounded(x, dtype):
    return ar.rounded(x, storage(dtype))


def rounding(ref, dtype):
    if dtype in hp.X_DTYPES:
        return (2.0 ** -22 * ref.abs()).clamp_min(2.0 ** -25)
    return ar.rounding(ref, dtype)


# ---- the launch geometry the header promises ------------------------------------------------------------------------------------------
def nsplit(B, HW):
    """pixel ranges per image (include/k22.h: a function of B and HW, at most 128; elementwise.hip: enough workgroups for the chip,
    512 / B, but at least 32 pixels per range)"""
    ns = min(128, 512 // max(B, 1))
    while ns > 1 and HW // ns < 32:
        ns >>= 1
    return max(ns, 1)


def lanes(C):
    vp = C // 4
    return 1 if vp >= 256 else 256 // vp


def stats_n(HW, ns, C):
    per = -(-HW // ns)
    pl = lanes(C)
    lp = -(-per // pl)
    r = lp // 8 + (3 if lp >= 8 else 0) + lp % 8 + (pl if pl > 1 else 0) + 1
    return 2 * r


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def chan_mean(B, C):
    return 0.3 + 0.05 * torch.arange(C, dtype=torch.float32)[None, :] + 2.0 * torch.arange(B, dtype=torch.float32)[:, None]


def x_family(fam, B, H, W, C, seed=0):
    """fp32 [B][H][W][C] of family a / c / d / e (module docstring)"""
    g = ar.gen(7000 + seed + 13 * C + 5 * H + W + 101 * B + ord(fam))
    z = ar.rn(g, B, H, W, C)
    if fam == "d":
        s = (0.5 + 0.1 * torch.arange(GROUPS, dtype=torch.float32)).repeat_interleave(C // GROUPS)
        return (s * (16.0 + z)).contiguous()
    m = chan_mean(B, C)[:, None, None, :]
    sd = m / 8.0 * (1.0 + (torch.arange(C) % 5).float() / 4.0)
    x = m + sd * z
    if fam == "c":
        x = x + sd * (0.37 * torch.arange(W, dtype=torch.float32)[None, None, :, None] + 0.23 * torch.arange(H, dtype=torch.float32)[None, :, None, None])
    if fam == "e":
        cg = C // GROUPS
        x[..., 3 * cg:4 * cg] = 0.01 + 0.001 * z[..., 3 * cg:4 * cg]
    return x.contiguous()


def affine(C, seed=0):
    g = ar.gen(7100 + seed + C)
    return 1.0 + 0.3 * ar.rn(g, C), 0.5 * ar.rn(g, C)


FILM_EXTRA, FILM_OFF = 192, 64


def film_b(B, C, seed=0):
    """family b -> dict: buf (flat fp32, NaN wherever the launch owns nothing), ld, off (the pointer is buf + off), C"""
    g = ar.gen(7200 + seed + C + B)
    ld = 2 * C + FILM_EXTRA
    buf = torch.full((FILM_OFF + B * ld,), ar.NAN, dtype=torch.float32)
    for b in range(B):
        sc = (0.25 * ar.rn(g, C)).clamp(-0.6, 0.6) + 0.15 * b
        sh = 0.5 * ar.rn(g, C) + 0.3 * b
        buf[FILM_OFF + b * ld: FILM_OFF + b * ld + 2 * C] = torch.cat([sc, sh])
    return {"buf": buf, "ld": ld, "off": FILM_OFF, "C": C}


def film_rows(film, B, mut=None):
    """(scale, shift) [B][C] as the launch is promised to read them: row b at buf + off + b * ld"""
    C = film["C"]
    ld = 2 * C if mut == "film_ld_2C" else film["ld"]
    rows = []
    for b in range(B):
        o = film["off"] + (0 if mut == "film_row0" else b) * ld
        rows.append(film["buf"][o:o + 2 * C])
    r = torch.stack(rows)
    sc, sh = r[:, :C], r[:, C:]
    return (sh, sc) if mut == "film_swapped" else (sc, sh)


def split_rows(x, rpi):
    """fp32 partial-sum rows [B * rpi][C][2] of x [B][HW][C] (any float type), image b owning rows [b rpi, (b + 1) rpi): float64 sums of rpi
    pixel ranges, rounded once - what SOME producer could have left"""
    parts = torch.tensor_split(x.double(), rpi, dim=1)
    rows = torch.stack([torch.stack([p.sum(1), (p * p).sum(1)], -1) for p in parts], 1)      # [B][rpi][C][2]
    return rows.float().reshape(-1, x.shape[-1], 2).contiguous()


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------
def stats_ref(x, ns, mut=None):
    """x [B][HW][C] (float64: the reference; fp32: torch's own evaluation) -> rows [B][ns][C][2] of ranges of ceil(HW / ns) pixels"""
    B, HW, C = x.shape
    per = -(-HW // ns)
    rows = torch.zeros(B, ns, C, 2, dtype=x.dtype, device=x.device)
    last = 0
    for s in range(ns):
        sl = x[:, s * per:min(HW, (s + 1) * per)]
        if sl.shape[1]:
            rows[:, s, :, 0] = sl.sum(1)
            rows[:, s, :, 1] = (sl * sl).sum(1)
            last = s
    if mut == "last_range_dropped":
        rows[:, last] = 0
    return rows


def stats_check(rows, x64, n):
    """rows [B][ns][C][2] (any float type) against x64 [B][HW][C] -> (violations, largest error / bound)"""
    tot = rows.double().sum(1)
    ref = torch.stack([x64.sum(1), (x64 * x64).sum(1)], -1)
    bound = n * U24 * torch.stack([x64.abs().sum(1), (x64 * x64).sum(1)], -1)
    return ar.violations(tot, ref, bound)


def stats_bounds(x64, n):
    """(ds, dq) [B][C]: the statistics bound of every channel, for e2e_ref"""
    return n * U24 * x64.abs().sum(1), n * U24 * (x64 * x64).sum(1)


def empty_ranges(HW, ns):
    per = -(-HW // ns)
    return [s for s in range(ns) if s * per >= HW]


# ---- coefficients -------------------------------------------------------------------------------------------------------------------------
def group_sums(srcs, B, mut=None):
    """srcs: [(rows [*][Ck][2] fp32, rpi, Ck)] -> float64 per-group (sum, sumsq) [B][32][2] and cg.  Image b owns rows [b rpi, (b + 1) rpi) of
    its source; group g owns channels [g cg, (g + 1) cg) of the virtual concat."""
    C = sum(s[2] for s in srcs)
    cg = C // GROUPS
    tot = []
    for k, (rows, rpi, Ck) in enumerate(srcs):
        flat = rows.double().reshape(-1, Ck, 2)
        r = srcs[1 - k][1] if (mut == "rpi_other" and len(srcs) == 2) else rpi
        img = torch.arange(B, device=flat.device) + (1 if mut == "image_next" else 0)
        idx = (img[:, None] * r + torch.arange(r, device=flat.device)[None, :]) % flat.shape[0]
        tot.append(flat[idx].sum(1))                                                        # [B][Ck][2]
    if mut == "second_ignored" and len(tot) == 2:
        tot[1] = torch.zeros_like(tot[1])
    tot = torch.cat(tot, 1)
    grp = tot.view(B, GROUPS, cg, 2).sum(2)
    if mut == "boundary_off_by_one" and len(srcs) == 2 and srcs[0][2] % cg:
        c0 = srcs[0][2]
        grp[:, c0 // cg] -= tot[:, c0 - 1]                                                   # the first source's part ends one channel early
    return grp, cg


def coeff_conditioned(srcs, B, HW):
    """the condition of the coefficient bound: mean^2 / var <= 2^10 in every group of the supplied sums"""
    grp, cg = group_sums(srcs, B)
    n = float(HW * cg)
    mean = grp[..., 0] / n
    var = grp[..., 1] / n - mean * mean
    return bool((mean * mean <= COND_MAX * var).all())


def coeff_ref(srcs, B, HW, gamma, beta, film, eps, mut=None, fp32=False):
    """-> dict: coeff [B][C][2] = (A, Bc), bound [B][C][2] (float64), and the float64 pieces e2e_ref needs.  fp32: mean and rstd rounded to
    fp32 once each, the rest evaluated in fp32 (the stage's plain fp32 evaluation)."""
    grp, cg = group_sums(srcs, B, mut)
    C = cg * GROUPS
    dev = grp.device
    n = float(HW * cg)
    mean = grp[..., 0] / n
    var = (grp[..., 1] / n - mean * mean).clamp_min(0.0)
    if mut == "unbiased":
        var = var * n / (n - 1.0)
    e = 0.0 if mut == "no_eps" else torch.tensor(eps, dtype=torch.float32).double().item()
    rstd = (var + e).rsqrt()
    dt = torch.float32 if fp32 else torch.float64
    mean_c = mean.to(dt).repeat_interleave(cg, 1)
    rstd_c = rstd.to(dt).repeat_interleave(cg, 1)
    ga, be = gamma.to(dev, dt), beta.to(dev, dt)
    A0 = rstd_c * ga
    Bc0 = be - mean_c * A0
    if film is not None:
        sc, sh = (t.to(dev, dt) for t in film_rows(film, B, mut))
        one = 1.0 + sc
        A = A0 * one
        Bc = (Bc0 + sh) * one if mut == "shift_first" else Bc0 * one + sh
    else:
        one, sh = torch.ones_like(A0), torch.zeros_like(A0)
        A, Bc = A0, Bc0
    S_bc = (be.abs() + (mean_c * A0).abs()) * one.abs() + sh.abs()
    bound = torch.stack([(N_A * U24 + CANCEL) * A.abs().double(), (N_BC * U24 + CANCEL) * S_bc.double()], -1)
    return {"coeff": torch.stack([A, Bc], -1).contiguous(), "bound": bound, "mean": mean, "rstd": rstd, "cg": cg, "gain": (ga * one).abs().double()}


# ---- apply --------------------------------------------------------------------------------------------------------------------------------
def silu64(x):
    return x * torch.sigmoid(x)


def silu_fast_term(pre):
    """element-wise evaluation error of x * rcp(1 + exp2(x * -log2 e)) from the 1-ulp accuracy of exp2 and rcp (module docstring)"""
    s = torch.sigmoid(pre)
    return 2.0 * U24 * (pre * s).abs() * ((1.0 - s) * (2.0 * pre.abs() + 2.0) + 4.0)


def e_act_term(pre, dtype):
    return silu_fast_term(pre) if dtype in hp.X_DTYPES else hp.act_eval_term(pre, SILU)


def out_hw(H, W, mode):
    return (H // 2, W // 2) if mode == 1 else ((2 * H, 2 * W) if mode == 2 else (H, W))


def _pool(v, Ho, Wo):
    B, _, _, C = v.shape
    return v[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C)


def apply_ref(x, coeff, act, mode, pad, dtype, mut=None, pre_err=None):
    """x [B][H][W][C] and coeff [B][C][2], float64 -> (ref, bound) [B][Ho + 2 pad][Wo + 2 pad][C]:  border(resample(act(x A + Bc))).
    pre_err (optional, [B][H][W][C]): a further error of the pre-activation (end to end: coefficients and statistics)."""
    B, H, W, C = x.shape
    dev = x.device
    A, Bc = coeff[:, None, None, :, 0], coeff[:, None, None, :, 1]
    pre = x * A + Bc
    bpre = N_PRE * U24 * ((x * A).abs() + Bc.abs())
    if pre_err is not None:
        bpre = bpre + pre_err
    if act:
        v, bv = silu64(pre), L_ACT * bpre + e_act_term(pre, dtype)
    else:
        v, bv = pre, bpre
    Ho, Wo = out_hw(H, W, mode)
    if mode == 1:
        v4 = _pool(v, Ho, Wo)
        out = v4.mean((2, 4))
        bound = _pool(bv, Ho, Wo).mean((2, 4)) + N_POOL * U24 * v4.abs().mean((2, 4))
        if mut == "silu_after_avg" and act:
            out = silu64(_pool(pre, Ho, Wo).mean((2, 4)))
    else:
        sh = 1 if mode == 2 else 0
        ys, xs = torch.arange(Ho, device=dev) >> sh, torch.arange(Wo, device=dev) >> sh
        if mut == "up_plus_one" and mode == 2:
            ys = ((torch.arange(Ho, device=dev) + 1) >> 1).clamp(max=H - 1)
        if mut == "xy_exchanged":                      # out[y][x] reads the source pixel (row xs[x], column ys[y])
            pick = lambda t: t[:, xs.clamp(max=H - 1)][:, :, ys.clamp(max=W - 1)].permute(0, 2, 1, 3)   # noqa: E731
        else:
            pick = lambda t: t[:, ys][:, :, xs]        # noqa: E731
        out, bound = pick(v), pick(bv)
    out, bound = out.clone(), bound.clone()
    if pad:
        if mut == "border_in":
            out[:, 0] = 0; out[:, -1] = 0; out[:, :, 0] = 0; out[:, :, -1] = 0
        if mut == "border_nonzero":
            out = F.pad(out.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate").permute(0, 2, 3, 1)
        else:
            out = F.pad(out, (0, 0, 1, 1, 1, 1))
        bound = F.pad(bound, (0, 0, 1, 1, 1, 1))
    out = out.contiguous()
    return out, bound.contiguous() + rounding(out, dtype)


def apply_torch32(x32, coeff32, act, mode, pad):
    """torch's own fp32 evaluation of the apply stage (NCHW functions on the NHWC tensors)"""
    y = x32 * coeff32[:, None, None, :, 0] + coeff32[:, None, None, :, 1]
    return _tail32(y.permute(0, 3, 1, 2), act, mode, pad)


def _tail32(y, act, mode, pad):
    if act:
        y = F.silu(y)
    if mode == 1:
        y = F.avg_pool2d(y, 2)
    elif mode == 2:
        y = F.interpolate(y, scale_factor=2, mode="nearest")
    if pad:
        y = F.pad(y, (1, 1, 1, 1))
    return y.permute(0, 2, 3, 1).contiguous()


def border_mask(shape, device):
    m = torch.ones(shape[1:3], dtype=torch.bool, device=device)
    m[1:-1, 1:-1] = False
    return m


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def exact_rows(x64):
    """float64 'rows' of x64 [B][HW][C]: one range per image, nothing rounded"""
    return torch.stack([x64.sum(1), (x64 * x64).sum(1)], -1)


def e2e_ref(x, gamma, beta, film, eps, act, mode, pad, dtype, ds, dq, mut=None):
    """x [B][H][W][C] float64 (T-rounded values), ds / dq [B][C]: the bound of every channel's sum / sum of squares as delivered to the
    coefficient pass -> (ref, bound) of the whole GroupNorm (module docstring: end to end)"""
    B, H, W, C = x.shape
    xf = x.reshape(B, H * W, C)
    rows = exact_rows(xf)
    src = [(rows.reshape(B, C, 2), 1, C)]
    # float64 rows: group_sums takes them as they are
    c = coeff_ref(src, B, H * W, gamma, beta, film, eps, mut)
    cg, n = c["cg"], float(H * W * c["cg"])
    dsg = ds.view(B, GROUPS, cg).sum(2)
    dqg = dq.view(B, GROUPS, cg).sum(2)
    dmean = dsg / n
    dvar = dqg / n + 2.0 * c["mean"].abs() * dmean
    drstd = 0.5 * c["rstd"] ** 3 * dvar
    exp = lambda t: t.repeat_interleave(cg, 1)[:, None, None, :]   # noqa: E731
    gain = c["gain"][:, None, None, :]
    pre_err = gain * (exp(c["rstd"]) * exp(dmean) + (x - exp(c["mean"])).abs() * exp(drstd))
    pre_err = pre_err + x.abs() * c["bound"][:, None, None, :, 0] + c["bound"][:, None, None, :, 1]
    return apply_ref(x, c["coeff"], act, mode, pad, dtype, None, pre_err)


def e2e_torch(x, gamma, beta, film, eps, act, mode, pad):
    """F.group_norm -> FiLM -> SiLU -> avg_pool2d / interpolate -> pad, in x's dtype (float64: the independent composition of part (a);
    fp32: torch's own evaluation)"""
    B, _, _, C = x.shape
    dt = x.dtype
    y = F.group_norm(x.permute(0, 3, 1, 2), GROUPS, gamma.to(x.device, dt), beta.to(x.device, dt), eps=torch.tensor(eps, dtype=torch.float32).item())
    if film is not None:
        sc, sh = (t.to(x.device, dt) for t in film_rows(film, B))
        y = y * (1 + sc[:, :, None, None]) + sh[:, :, None, None]
    return _tail32(y, act, mode, pad)


# ---- the cases both halves run ------------------------------------------------------------------------------------------------------------------
STATS_C = (128, 256, 384, 640, 1024, 1536, 2688, 3072)      # PL = 8, 4, 2; PL = 1 under 256 vectors; one slot; two; three (last partly filled); three full
STATS_HW = (16, 25, 70)
STATS_B = (1, 2, 3, 5)
STATS_SPLITS = ((128, 128), (72, 184), (1152, 768))


def stats_cases():
    """(C0, C1, B, HW)"""
    out, i = [], 0
    for C in STATS_C:
        for HW in STATS_HW:
            for B in (STATS_B if C in (128, 1024) else (STATS_B[i % 4],)):
                out.append((C, 0, B, HW))
            i += 1
    for j, (C0, C1) in enumerate(STATS_SPLITS):
        for HW in (25, 70):
            for B in (2, 3):
                out.append((C0, C1, B, HW))
    out.append((128, 0, 1, 2500))                              # 50 x 50: 64 ranges of 40, the last one empty
    return out


def stats_input(C0, C1, B, HW, dtype):
    return rounded(x_family("a", B, 1, HW, C0 + C1, seed=1).view(B, HW, C0 + C1), dtype)


# (C0, C1, rpi0, rpi1, B, HW, eps, family, film)
COEFF_CASES = (
    (128, 256, 1, 3, 1, 48, 1e-5, "a", True), (128, 256, 7, 40, 2, 48, 1e-6, "e", True), (128, 256, 40, 7, 3, 48, 1e-5, "a", False),
    (1152, 768, 3, 1, 2, 48, 1e-5, "a", True), (1152, 768, 40, 7, 3, 48, 1e-6, "a", True), (1152, 768, 7, 40, 1, 48, 1e-5, "e", False),
    (256, 0, 3, 0, 2, 16, 1e-5, "d", True), (3072, 0, 1, 0, 2, 48, 1e-5, "a", True),
)


def coeff_inputs(case, dtype):
    """-> dict: srcs [(rows, rpi, Ck)], gamma, beta, film (or None)"""
    C0, C1, rpi0, rpi1, B, HW, eps, fam, film = case
    C = C0 + C1
    x = rounded(x_family(fam, B, 1, HW, C, seed=2).view(B, HW, C), dtype)
    srcs = [(split_rows(x[..., :C0].contiguous(), rpi0), rpi0, C0)]
    if C1:
        srcs.append((split_rows(x[..., C0:].contiguous(), rpi1), rpi1, C1))
    ga, be = affine(C, seed=2)
    return {"srcs": srcs, "gamma": ga, "beta": be, "film": film_b(B, C, seed=2) if film else None}


APPLY_C = ((128, 0), (1152, 768))
APPLY_HW = ((5, 5), (7, 9), (6, 10), (12, 12))


def apply_cases():
    """(C0, C1, B, H, W): every one runs modes 0 / 1 / 2 x pad 0 / 1 x act 0 / SiLU.  C = 1920 at W = 12, mode 2, pad 1 is a row of 26 x 240
    (480 in fp32) vectors: 24.4 (48.75) chunks of 256 threads"""
    return [(C0, C1, 3 if (H, W) in ((5, 5), (7, 9)) else 1, H, W) for (C0, C1) in APPLY_C for (H, W) in APPLY_HW]


def apply_inputs(C0, C1, B, H, W, dtype):
    """x of family c and the coefficients of its own GroupNorm with FiLM family b (fp32, as a coefficient pass would have left them)"""
    C = C0 + C1
    x = rounded(x_family("c", B, H, W, C, seed=3), dtype)
    ga, be = affine(C, seed=3)
    x64 = x.double().view(B, H * W, C)
    c = coeff_ref([(exact_rows(x64), 1, C)], B, H * W, ga, be, film_b(B, C, seed=3), 1e-5)
    return {"x": x, "coeff": c["coeff"].float().contiguous()}


# (C0, C1, B, H, W, family, film, act, mode, pad) through k22_groupnorm
E2E_CASES = (
    (128, 0, 2, 5, 5, "a", False, 1, 0, 1), (128, 128, 3, 7, 9, "c", True, 1, 1, 1), (72, 184, 2, 6, 10, "c", True, 1, 2, 1),
    (1152, 768, 2, 6, 10, "a", True, 1, 0, 1), (256, 0, 2, 12, 12, "d", True, 0, 0, 0), (256, 0, 2, 12, 12, "d", False, 1, 0, 1),
    (128, 0, 1, 50, 50, "c", False, 1, 1, 1),
)


def e2e_inputs(case, dtype):
    C0, C1, B, H, W, fam, film = case[:7]
    C = C0 + C1
    ga, be = affine(C, seed=4)
    return {"x": rounded(x_family(fam, B, H, W, C, seed=4), dtype), "gamma": ga, "beta": be, "film": film_b(B, C, seed=4) if film else None}


def to_dev(d, device):
    out = {}
    for k, v in d.items():
        if torch.is_tensor(v):
            out[k] = v.to(device)
        elif isinstance(v, dict):
            out[k] = to_dev(v, device)
        elif k == "srcs":
            out[k] = [(r.to(device), rpi, Ck) for (r, rpi, Ck) in v]
        else:
            out[k] = v
    return out
