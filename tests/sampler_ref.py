"""Float64 / numpy restatements, inputs, bounds and a host model of the dispatch of k22_sampler_step's three kernels (csrc/sampler.hip:
sampler_x0_kernel, sampler_threshold_kernel, sampler_final_kernel), for tests/test_sampler_select_cpu.py and tests/test_sampler_select_gpu.py.
A plain module like seam_ref.py, whose comparator (`violations`, `with_guard`), bound classes and c rule it shares through aux_ref.

The observable is the scratch: k22_sampler_step puts s_buf at float 0 and x0_buf at float 64 of it (csrc/capi.hip).  After a launch the test reads
both back, so every kernel is held to ITS OWN inputs as stored: x0_buf to the launch's operands, s to the stored x0_buf of image 0, x_out and
x0_out to the stored x0_buf and the stored s.

 x0_buf   class D  |out - ref| <= n * 2^-24 * S, n = twice the roundings of the expression AS WRITTEN (contraction only removes roundings), S the
                   expression over absolute values:
                     eps = u + g (c - u)                     3 roundings under CFG, none without (eps is the model's own value)
                     sr * x, srm1 * eps, their difference    3
                     clamp(lo, hi)                           0: 1-Lipschitz, it adds nothing and S stays the unclamped S0 = |sr| |x| + |srm1| E,
                                                             E = |u| + |g| (|c| + |u|) (|eps| without CFG)
                     x0 (1 - m) + init m                     4 with a mask: 1 - m, two products, the sum; S = S0 |1 - m| + |init| |m|
                   n = 2 * 6 = 12 under CFG, 2 * 3 = 6 without; with a mask 2 * 10 = 20 and 2 * 7 = 14.
 s        class E  equal bits with max(np.percentile(|x0_buf of image 0, as read back|, 99.5), 1) in float32: numpy's own two-branch lerp on the
                   kernel's own stored keys, index and weight from diffusion.percentile_index.  No tolerance.
 x0_out   class D  clamp(x0_buf, -s, s) / s: the clamp is exact, one division: n = 2, S = |ref|.  Threshold off (pct_index = -1): x0_buf's bits.
 x_out    class M  c * 2^-24 * S, c = aux_ref.c_rule(yardstick).  With x0t = x0_out's expression, frac = (v + 1) / 2 of the variance channels,
                   logvar = frac max_log + (1 - frac) min_log and T = nonzero exp(logvar / 2) noise:
                     ref = c1 x0t + c2 x + T       S = |c1| |x0t| + |c2| |x| + |T| (1 + SL / 2),  SL = |frac| |max_log| + |1 - frac| |min_log|
                   (an error dL of logvar moves exp(logvar / 2) by half of dL relative: SL is the expression of logvar over absolute values).
                   The yardstick is torch's OWN fp32 evaluation of this expression against float64 in units of 2^-24 * S on the same operands
                   (the stored x0_buf and s included), never a kernel's.  MEASURED, largest over the select items (SELECT_ROW) and over the
                   parity items (the three real rows):
                                         select items   parity items
                     CPU                 2.848          2.661
                     MI355X              2.848          2.661
                   Largest 2.848 (the logvar path: four roundings of a sum of terms of size |max_log|, |min_log| ~ 2-10 in front of the
                   exponential) -> c = 2 x 2.848 = 5.696.  test_sampler_select_cpu.py prints the CPU reading, test_sampler_select_gpu.py the MI355X one on every
                   run and asserts torch itself under c.

The select cases use a table row with sqrt_recip = 1, sqrt_recipm1 = 0 and model_out = 0 (SELECT_ROW): x0 = clamp(x) exactly, so every key is
what the case wrote and `dispatch` - the host model of the launcher's template choice and of the pivot filter - labels the path the launch takes:
  plain        KPT = 4: no sample, the radix passes over all keys
  few-samples  KPT >= 16 with fewer than 512 valid samples: no filter
  filtered     the rank lies among the keys >= pivot: three passes over those keys, rank shifted by `below`
  fall-back    the rank lies below the pivot: three passes over all keys
  generic      more than 64 * 1024 keys: KPT = 0, the keys are re-read from memory in every pass
The conditions under which a case can tell a wrong select from a right one (percentile above 1; s changes in bits when rank lo - 1 or lo + 1
is taken instead) are asserted on the reference alone by the CPU test.  They cannot hold where the case itself ties the ranks lo - 1, lo and
lo + 1: gauss_clamped (12 % of the keys at 2.0), tie_straddle, all_equal - and two_values, whose upper value sits at 0.4 % of the positions, so
that ranks lo - 1 to lo + 1 all hold the lower one (the case is there for the successor search: "the next distinct key" gives 1.75).
"""
import collections
import functools

import numpy as np
import torch

import aux_ref as ar
import kandinsky2_amd as k22
from kandinsky2_amd.diffusion import percentile_index

U24 = ar.U24
NAN = ar.NAN
violations, with_guard, plain_ratio, to_dev = ar.violations, ar.with_guard, ar.plain_ratio, ar.to_dev

GUIDANCE = 4.0
S_OFF, X0_OFF = 0, 64                  # floats of the scratch: s_buf, x0_buf (csrc/capi.hip)
WIDE = 1.0e30                          # a clamp that clamps nothing
# one c for sampler_final_kernel's x_out: aux_ref.c_rule on the larger of the CPU and the MI355X reading (docstring)
SAMPLER_C = ar.c_rule(2.848)

SELECT_HW = (1, 2, 255, 256, 1024, 1025, 1794, 2047, 2048, 2304, 4096, 4097, 9216, 9217, 16384, 16385, 20000)
PARITY_HW = (2, 255, 1025, 2304)
LABELS = ("plain", "few-samples", "filtered", "fall-back", "generic")
# cases that tie ranks lo - 1, lo, lo + 1 by construction (docstring): s cannot depend on which of the three is taken
TIE_CASES = ("gauss_clamped", "tie_straddle", "all_equal", "two_values")
CASES = ("gauss_clamped", "gauss_open", "binades", "ulp_ramp_mid", "ulp_ramp_top", "tie_straddle", "tie_above", "all_equal", "two_values",
         "zeros_and_tail", "sample_large", "sample_small", "sample_is_answer", "image0_only")


def f32bits(v):
    """the bit pattern of one float32 value"""
    return int(np.asarray(v, dtype=np.float32).view(np.uint32))


# ---- table rows ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table():
    """[4][8] fp32 rows in k22_sampler_step's format: 0-2 the first executed, a middle and the last step (t != 0 is 0 there) of the 2.1 decoder's
    own 50-step schedule; 3 = SELECT_ROW: the middle row with sqrt_recip = 1 and sqrt_recipm1 = 0"""
    t = k22.create_gaussian_diffusion(**dict(k22.DIFFUSION_CONFIG_2_1, timestep_respacing="50")).step_table()
    rows = np.ascontiguousarray(t[[49, 25, 0, 25]]).astype(np.float32)
    rows[3, 0], rows[3, 1] = 1.0, 0.0
    return rows


PARITY_ROWS = (0, 1, 2)
SELECT_ROW = 3


# ---- the host model of the dispatch (launch_sampler_step, sampler_threshold_kernel) --------------------------------------------------------------
def template_kpt(n):
    """the KPT the launcher instantiates for n keys: 4, 16, 36, 64, or 0 (the generic path)"""
    kpt = (n + 1023) // 1024
    for K in (4, 16, 36, 64):
        if kpt <= K:
            return K
    return 0


def sample_positions(n):
    """flat indices into image 0 that the pivot sample reads: thread t holds element (t % KPT) * 1024 + t, kept where it is below n"""
    K = template_kpt(n)
    t = np.arange(1024)
    idx = (t % K) * 1024 + t
    return idx[idx < n]


def keys_of(img):
    """the keys of the select: the bit patterns of |v| (monotone for non-negative floats)"""
    return np.abs(np.ascontiguousarray(img, dtype=np.float32).ravel()).view(np.uint32)


Dispatch = collections.namedtuple("Dispatch", "label KPT ns pivot below")


def dispatch(img0, lo):
    """which path sampler_threshold_kernel takes for the stored image 0 and rank lo"""
    keys = keys_of(img0)
    n = keys.size
    K = template_kpt(n)
    if K == 0:
        return Dispatch("generic", 0, 0, None, None)
    if K == 4:
        return Dispatch("plain", 4, 0, None, None)
    idx = sample_positions(n)
    ns = idx.size
    if ns < 512:
        return Dispatch("few-samples", K, ns, None, None)
    pivot = np.sort(keys[idx])[int(np.float32(ns) * np.float32(0.973))]
    below = int((keys < pivot).sum())
    return Dispatch("filtered" if lo >= below else "fall-back", K, ns, int(pivot), below)


# ---- s: numpy's percentile, and an emulation of the select with its wrong variants ------------------------------------------------------------------
def lerp32(a, b, t):
    """numpy's _lerp in float32: a + (b - a) t, and b - (b - a) (1 - t) where t >= 0.5"""
    a, b, t = np.float32(a), np.float32(b), np.float32(t)
    d = np.float32(b - a)
    if t >= np.float32(0.5):
        return np.float32(b - np.float32(d * np.float32(np.float32(1) - t)))
    return np.float32(a + np.float32(d * t))


def s_ref(img0):
    """the reference of s_buf: max(np.percentile(|image 0 of x0_buf|, 99.5), 1) in float32"""
    a = np.abs(np.ascontiguousarray(img0, dtype=np.float32).ravel())
    p = np.percentile(a, 99.5)
    assert p.dtype == np.float32
    return np.float32(max(p, np.float32(1)))


def percentile_at(img0, lo, gamma):
    """the lerp of the order statistics lo and lo + 1 (the percentile when (lo, gamma) = percentile_index(n))"""
    srt = np.sort(np.abs(np.ascontiguousarray(img0, dtype=np.float32).ravel()))
    return lerp32(srt[lo], srt[min(lo + 1, srt.size - 1)], gamma)


def _radix_rank(keys, k):
    """the k-th smallest key by the kernel's digit plan: three histogram passes over 11 + 11 + 10 bits"""
    prefix, mask = np.uint32(0), np.uint32(0)
    for shift, nb in ((21, 2048), (10, 2048), (0, 1024)):
        live = keys[(keys & mask) == prefix]
        hist = np.bincount((live >> np.uint32(shift)) & np.uint32(nb - 1), minlength=nb)
        incl = np.cumsum(hist)
        b = int(np.searchsorted(incl, k, side="right"))
        k -= int(incl[b] - hist[b])
        prefix |= np.uint32(b << shift)
        mask |= np.uint32((nb - 1) << shift)
    return prefix


VARIANTS = ("rank_off_by_one", "lerp_first_branch", "next_distinct", "no_fall_back", "image_1")


def select_emul(x0, lo, gamma, variant=None):
    """numpy emulation of sampler_threshold_kernel on the stored x0 [N][4 HW]: sample, pivot, filter or fall-back, radix passes, successor search,
    lerp, max(., 1).  variant: ONE deliberately wrong select (VARIANTS)"""
    keys = keys_of(x0[1] if variant == "image_1" else x0[0])
    n = keys.size
    if variant == "rank_off_by_one":
        lo = lo - 1
    k_hi = min(lo + 1, n - 1)
    d = dispatch(x0[0], lo)
    cand, k_sel = keys, lo
    if d.label in ("filtered", "fall-back") and variant != "image_1":
        if d.label == "filtered" or variant == "no_fall_back":
            cand, k_sel = keys[keys >= np.uint32(d.pivot)], max(lo - d.below, 0)
    ka = _radix_rank(cand, k_sel)
    cnt = int((keys <= ka).sum())
    above = keys[keys > ka]
    mn = above.min() if above.size else np.uint32(0xffffffff)
    kb = ka if (cnt > k_hi or k_hi == lo) else mn
    if variant == "next_distinct" and k_hi != lo and above.size:
        kb = mn
    a, b = (np.array([v], dtype=np.uint32).view(np.float32)[0] for v in (ka, kb))
    t = np.float32(gamma)
    r = np.float32(a + np.float32(np.float32(b - a) * t)) if variant == "lerp_first_branch" else lerp32(a, b, t)
    return np.float32(max(r, np.float32(1)))


# ---- the select cases --------------------------------------------------------------------------------------------------------------------------
def case_applies(case, n):
    if case in ("ulp_ramp_mid", "ulp_ramp_top", "all_equal"):
        return True
    if case.startswith("sample_"):
        return template_kpt(n) >= 16
    return n >= 1020                    # the statistical cases and the ones that need room above rank lo + 3


@functools.lru_cache(maxsize=None)
def select_items():
    """(HW, case, N, use_cfg): N = 2 under CFG; image0_only also with N = 3 and use_cfg = 0"""
    out = []
    for HW in SELECT_HW:
        for case in CASES:
            if case_applies(case, 4 * HW):
                out.append((HW, case, 2, 1))
                if case == "image0_only":
                    out.append((HW, case, 3, 0))
    return tuple(out)


def _distinct(rng, k, a, b):
    """k distinct float32 values in [a, b), increasing: a jittered ramp whose steps stay far above an ulp"""
    return (a + (b - a) * (np.arange(k) + 0.5 * rng.random(k)) / max(k, 1)).astype(np.float32)


def _signed(rng, v):
    return (v * rng.choice(np.array([-1.0, 1.0], dtype=np.float32), v.size)).astype(np.float32)


def _image0(case, n, rng):
    """-> (flat image 0, clamp)"""
    lo, _ = percentile_index(n)
    if case == "gauss_clamped":
        return (1.3 * rng.standard_normal(n)).astype(np.float32), 2.0
    if case in ("gauss_open", "image0_only"):
        return (0.6 * rng.standard_normal(n)).astype(np.float32), WIDE if case == "image0_only" else 2.0
    if case == "binades":
        return _signed(rng, np.exp2(rng.uniform(-20.0, 20.0, n)).astype(np.float32)), WIDE
    if case in ("ulp_ramp_mid", "ulp_ramp_top"):
        # n consecutive bit patterns from `base`: rank r holds base + r.  Rank lo + 1 is the first key of a new middle digit (bits 10-20: a
        # multiple of 2^10 above 1.0) or of a new top digit (bits 21-31: 0x3fa00000 = 1.25)
        edge = 0x3f800000 + ((lo + 1) // 1024 + 1) * 1024 if case == "ulp_ramp_mid" else 0x3fa00000
        bits = (edge - (lo + 1) + np.arange(n)).astype(np.uint32)
        assert bits[0] > 0x3f800000
        return _signed(rng, rng.permutation(bits.view(np.float32))), 2.0
    if case in ("tie_straddle", "tie_above"):
        v = _distinct(rng, n, 0.25, 1.9 if case == "tie_straddle" else 1.2)
        if case == "tie_straddle":
            v[lo - 3:lo + 4] = v[lo]
        else:
            v[lo + 1:] = 517.3          # far above rank lo: (b - a) t is nearly the whole result, where the two branches of the lerp round differently
        return _signed(rng, rng.permutation(v)), 2.0 if case == "tie_straddle" else WIDE
    if case == "all_equal":
        return _signed(rng, np.full(n, 1.5, dtype=np.float32)), 2.0
    if case == "two_values":
        v = np.full(n, 1.25, dtype=np.float32)
        v[rng.permutation(n)[:max(1, round(0.004 * n))]] = 1.75
        return _signed(rng, v), 2.0
    if case == "zeros_and_tail":
        v = np.zeros(n, dtype=np.float32)
        k = round(0.02 * n)
        v[rng.permutation(n)[:k]] = 1.0 + np.abs(rng.standard_normal(k))
        return _signed(rng, v), WIDE                              # both signs of zero
    idx = sample_positions(n)
    rest = np.setdiff1d(np.arange(n), idx)
    v = np.empty(n, dtype=np.float32)
    if case == "sample_large":
        v[idx], v[rest] = rng.permutation(_distinct(rng, idx.size, 1.5, 2.0)), rng.permutation(_distinct(rng, rest.size, 1.0, 1.4))
    elif case == "sample_small":
        v[idx], v[rest] = rng.permutation(_distinct(rng, idx.size, 1.0, 1.4)), rng.permutation(_distinct(rng, rest.size, 1.5, 2.0))
    else:
        # sample_is_answer: every sampled position holds 1.6, which occupies ranks lo - ns + 1 .. lo; n - 1 - lo distinct keys lie above it
        assert case == "sample_is_answer" and lo + 1 >= idx.size
        nb = lo + 1 - idx.size
        v[idx] = 1.6
        v[rest] = rng.permutation(np.concatenate([_distinct(rng, nb, 0.3, 1.55), _distinct(rng, rest.size - nb, 1.65, 1.95)]))
    return _signed(rng, v), 2.0


def select_input(HW, case, N):
    """the operands of one select item: x [N][4][HW] (image 0 the case's keys; the others 10 x image 0 for image0_only, else other Gaussian
    values), model_out = 0, noise, the clamp"""
    n = 4 * HW
    rng = np.random.default_rng(7919 * CASES.index(case) + HW)
    img0, clamp = _image0(case, n, rng)
    imgs = [img0] + [(10.0 * img0 if case == "image0_only" else 0.8 * rng.standard_normal(n)).astype(np.float32) for _ in range(N - 1)]
    return {"x": torch.from_numpy(np.stack(imgs).reshape(N, 4, HW)), "mo": torch.zeros(N, 8, HW),
            "noise": torch.from_numpy(rng.standard_normal((N, 4, HW)).astype(np.float32)), "clamp": clamp}


def select_x0(d):
    """what sampler_x0_kernel stores for a select item: clamp(x), exactly (row SELECT_ROW, model_out = 0)"""
    return d["x"].clamp(-d["clamp"], d["clamp"])


# ---- the parity cases --------------------------------------------------------------------------------------------------------------------------
PARITY_BATCH = ((2, 1), (4, 1), (1, 0), (3, 0))                 # (N, use_cfg)
PARITY_CLAMP = 2.0


def parity_input(N, HW):
    """random operands, the variance channels 4-7 of model_out included; mask: random 0 / 1 with a soft band of 0.3"""
    g = ar.gen(1700 + 13 * N + HW)
    mask = (torch.rand(N, 1, HW, generator=g) < 0.5).float()
    mask[:, :, HW // 3:HW // 3 + max(1, HW // 8)] = 0.3
    return {"x": 0.2 + 1.5 * ar.rn(g, N, 4, HW), "mo": 0.1 + ar.rn(g, N, 8, HW), "noise": ar.rn(g, N, 4, HW), "init": ar.rn(g, N, 4, HW), "mask": mask}


def _guided(mo, use_cfg, g, mut=None):
    """-> (eps, E): model_fn's guidance on channels 0-3, rows [cond | uncond], both halves get u + g (c - u)"""
    if not use_cfg:
        return mo[:, :4], mo[:, :4].abs()
    bs = mo.shape[0] // 2
    c, u = mo[:bs, :4].repeat(2, 1, 1), mo[bs:, :4].repeat(2, 1, 1)
    return u + g * (c - u), u.abs() + abs(g) * (c.abs() + u.abs())


def x0_n(use_cfg, masked):
    return 2 * ((6 if use_cfg else 3) + (4 if masked else 0))


def x0_ref(d, row, use_cfg, clamp, masked, dtype=torch.float64):
    """sampler_x0_kernel in `dtype` on the fp32 row -> (x0, bound)"""
    sr, srm1 = float(np.float32(row[0])), float(np.float32(row[1]))
    x, mo = d["x"].to(dtype), d["mo"].to(dtype)
    e, E = _guided(mo, use_cfg, float(np.float32(GUIDANCE)))
    x0 = (sr * x - srm1 * e).clamp(-clamp, clamp)
    S = abs(sr) * x.abs() + abs(srm1) * E
    if masked:
        m, init = d["mask"].to(dtype), d["init"].to(dtype)
        x0 = x0 * (1 - m) + init * m
        S = S * (1 - m).abs() + init.abs() * m.abs()
    return x0, x0_n(use_cfg, masked) * U24 * S


def final_ref(x0_buf, s, d, row, dtype=torch.float64):
    """sampler_final_kernel in `dtype` from the STORED x0_buf and the stored s (None: threshold off) -> (x_out, x0_out, S of x_out)"""
    c1, c2, min_log, max_log, nonzero = (float(np.float32(row[k])) for k in (2, 3, 4, 5, 6))
    x0t = x0_buf.to(dtype)
    if s is not None:
        s = float(np.float32(s))
        x0t = x0t.clamp(-s, s) / s
    x, v, nz = d["x"].to(dtype), d["mo"][:, 4:8].to(dtype), d["noise"].to(dtype)
    frac = (v + 1) / 2
    logvar = frac * max_log + (1 - frac) * min_log
    T = nonzero * torch.exp(0.5 * logvar) * nz
    SL = frac.abs() * abs(max_log) + (1 - frac).abs() * abs(min_log)
    S = abs(c1) * x0t.abs() + abs(c2) * x.abs() + T.abs() * (1 + 0.5 * SL)
    return c1 * x0t + c2 * x + T, x0t, S


def final_bounds(x0t, S, thresholded):
    """-> (bound of x_out, bound of x0_out)"""
    return SAMPLER_C * U24 * S, (2 * U24 * x0t.abs() if thresholded else torch.zeros_like(x0t))


def yardstick(x0_buf, s, d, row):
    """torch's own fp32 evaluation of the final expression against float64, in units of 2^-24 * S, on the device the tensors live on"""
    ref, _, S = final_ref(x0_buf, s, d, row)
    return plain_ratio(final_ref(x0_buf, s, d, row, dtype=torch.float32)[0], ref, S)
