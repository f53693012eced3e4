"""Float64 restatement of one DDIM step of the prior and of its table rows, with the per-element bound of the fp32 kernel
(csrc/prior.hip: prior_ddim_step_kernel), for tests/test_prior_ddim_cpu.py and tests/test_prior_ddim_gpu.py.  A plain module like
aux_ref.py / gn_ref.py.

The step (GaussianDiffusion.ddim_sample, gaussian_diffusion.py:477-519, as PriorDiffusionModel.forward runs it: START_X mean,
clip_denoised off, denoised_fn = clamp(+-10), classifier-free guidance on the x0 prediction, prior.py:351-364), rows [cond | uncond]:

    x0  = clamp(u + s (c - u), +-clamp)                        c, u = the two halves of model_out, s = scales[j]
    eps = (r x - x0) / rm1                                     r = sqrt_recip_ac[i], rm1 = sqrt_recipm1_ac[i]
    y   = A x0 + dir eps + nz sig noise                        A = sqrt(ab_prev), dir = sqrt(1 - ab_prev - sig^2), nz = (i != 0)
    sig = eta sqrt((1 - ab_prev) / (1 - ab)) sqrt(1 - ab / ab_prev)

The bound.  The kernel evaluates the step in eleven operations, each rounded once (__fsub_rn / __fmul_rn / __fadd_rn / __fdiv_rn: the
compiler cannot contract them), so each result is within 2^-24 (half an ulp, relative) of its exact value on the operands it got:

    1  c - u      2  s * (1)      3  u + (2)   (clamp: exact, and 1-Lipschitz - it never grows an error)
    4  r * x      5  (4) - x0     6  (5) / rm1
    7  A * x0     8  dir * (6)    9  (7) + (8)
    10 sig * noise   (nz * (10): exact, nz is 0 or 1)         11 (9) + (10)

The longest chain from an input to y is 1-2-3-5-6-8-9-11: eight roundings.  To first order the error of y is the sum over the
operations of 2^-24 * |value of the operation| * |dy / d(that value)|.  With

    T1 = |A x0|    T2 = |dir r x / rm1|    T3 = |dir x0 / rm1|    T4 = |sig noise|
    G  = |u| + |s| (|c| + |u|)   (bounds |c - u| |s|, the unclamped x0 and, clamp being a contraction, x0 itself)
    K  = A + dir / rm1           (bounds |dy / dx0| = |A - dir / rm1|)

the operations weigh:  1, 2: K |s| (|c| + |u|) <= K G each;  3: K G;  4: T2;  5, 6, 8: T2 + T3 each;  7: T1;  9: T1 + T2 + T3;
10: T4;  11: T1 + T2 + T3 + T4.  Collected per term: T1 x 3, T2 x 6, T3 x 5, T4 x 2, K G x 3.  No term is weighed more than six times,
none can be weighed more often than the longest chain has roundings (eight), so with

    S = T1 + T2 + T3 + T4 + K G

    |y_kernel - y_float64| <= 8 * 2^-24 * S

holds with a quarter of the factor left for the second-order terms (each <= 2^-24 of a first-order one).  x0_out carries operations
1-3 only: |x0_kernel - x0_float64| <= 3 * 2^-24 * G, which 8 * 2^-24 * S contains only where K >= 3/8, so x0 has its own bound
(bound_x0).  The float64 reference works on the fp32 table row and fp32 operands as the kernel sees them (exact in float64): the
rounding of the table itself - "computed in float64, rounded once" - is the schedule's, tested against the reference's float64 arrays.

The same bound is what the reference's own fp32 evaluation of a step gets in test_prior_ddim_cpu.py: torch runs the same chain in
fp32 (its coefficients are the float64 arrays rounded to fp32, its sigma / dir are formed in fp32), which the margin between 6 and 8
has to carry as well; the recorded step (ddim5, eta 1, index 2) is well-conditioned (1 - ab_prev - sig^2 ~ 0.02 against 1 - ab_prev ~ 0.1).
"""
import numpy as np
import torch

U32 = 2.0 ** -24
N_ROUNDINGS = 8


def table_rows(ab, abp, eta):
    """float64 [T][8] rows of k22_prior_ddim_step from the float64 alphas_cumprod / alphas_cumprod_prev, by schedule index:
    (sqrt(1/ab), sqrt(1/ab - 1), sqrt(ab_prev), sigma, sqrt(1 - ab_prev - sigma^2), i != 0, 0, 0)"""
    ab, abp = np.asarray(ab, dtype=np.float64), np.asarray(abp, dtype=np.float64)
    sig = eta * np.sqrt((1 - abp) / (1 - ab)) * np.sqrt(1 - ab / abp)
    tab = np.zeros((len(ab), 8), dtype=np.float64)
    tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3] = np.sqrt(1.0 / ab), np.sqrt(1.0 / ab - 1), np.sqrt(abp), sig
    tab[:, 4] = np.sqrt(1 - abp - sig ** 2)
    tab[:, 5] = np.arange(len(ab)) != 0
    return tab


def ddim_step64(x, model_out, noise, scales, row, clamp=10.0):
    """One step in float64 on [2*bs][D] rows [cond | uncond]; noise None = zeros; row = the 8 table values (any float sequence).
    Returns (y, x0, S, G): sample, clamped guided prediction (both [2*bs][D]), and the two magnitudes of the bounds above."""
    f = lambda t: torch.as_tensor(t).double()  # noqa: E731
    x, mo, s = f(x), f(model_out), f(scales)[:, None]
    r, rm1, A, sig, dr, nz = (float(v) for v in list(row)[:6])
    bs = mo.shape[0] // 2
    c, u = mo[:bs], mo[bs:]
    x0 = torch.clamp(u + s * (c - u), -clamp, clamp).repeat(2, 1)
    G = (u.abs() + s.abs() * (c.abs() + u.abs())).repeat(2, 1)
    nzs = torch.zeros_like(x) if noise is None else f(noise)
    y = A * x0 + dr * ((r * x - x0) / rm1) + nz * sig * nzs
    S = (A * x0).abs() + (dr * r * x / rm1).abs() + (dr * x0 / rm1).abs() + (sig * nzs).abs() + (A + dr / rm1) * G
    return y, x0, S, G


def bound(S):
    return N_ROUNDINGS * U32 * S


def bound_x0(G):
    return 3 * U32 * G
