"""Float64 restatements and bounds of the DPM-Solver++ sampler (kandinsky2_amd.sampling.dpmpp_table / dpmpp_grid, k22_dpmpp_step,
k22_unet_dpmpp_loop, DPMSolverSamplerHIP) for tests/test_dpmpp_cpu.py and tests/test_dpmpp_gpu.py.  A plain module like
prior_ddim_ref.py / decoder22_ref.py.

PARITY UNPINNED against any other implementation: the reference has no such sampler.  What pins the FORMULA is mathematics - a model
whose probability-flow ODE has a closed-form solution (below) - and what pins the ENGINE is this file's float64 restatement.

The solver (Lu et al. 2022, DPM-Solver++, multistep, data prediction).  alpha = sqrt(ac), sigma = sqrt(1 - ac), lambda = ln(alpha /
sigma); a step goes from s to t, h = lambda_t - lambda_s > 0, phi = -expm1(-h), x0_s = (x - sigma_s e) / alpha_s:

    order 1:   x_t = (sigma_t / sigma_s) x + alpha_t phi x0_s
    order 2M:  x_t = (sigma_t / sigma_s) x + alpha_t phi [(1 + 1 / (2 r)) x0_s - (1 / (2 r)) x0_prev],     r = h_prev / h

The toy model.  Data x0 ~ N(MU, SD^2); then x_t ~ N(MU alpha_t, v_t), v_t = SD^2 alpha_t^2 + sigma_t^2, the optimal eps is
e(x, t) = sigma_t (x - MU alpha_t) / v_t, and the probability-flow ODE maps x_s to  MU alpha_t + sqrt(v_t / v_s) (x_s - MU alpha_s)
exactly.  A solver's error is max|x - exact| / max|exact| at the last target over a fixed set of start points.

The step bound (k22_dpmpp_step).  The kernel evaluates, each operation rounded once (csrc/sampler.hip states the list):

    1  c - u     2  g * (1)    3  u + (2)            (use_cfg only; e = model_out otherwise)
    4  sigma_s * e     5  x - (4)     6  (5) / alpha_s = x0
    7  c_x * x         8  c_0 * x0    9  (7) + (8)
    10 c_1 * x0_prev   11 (9) + (10)                 (order 2 only)

The longest chain from an input to x_out is 1-2-3-4-5-6-8-9-11: nine roundings.  The five table entries are float64 values rounded to fp32
once: one more relative 2^-24 each on every term they multiply or divide.  To first order the error of x_out is the sum over the
operations (and table roundings) of 2^-24 |value| |d x_out / d value|; every |value| |derivative| is at most the whole expression taken
over absolute values,

    E  = |u| + |g| (|c| + |u|)                         (e itself without use_cfg)
    S0 = (|x| + sigma_s E) / alpha_s                   (bounds |x0|)
    S  = |c_x| |x| + |c_0| S0 + |c_1| |x0_prev|

so with n = 9 + 5 = 14 (every operation of the longest chain and every table entry charged the whole of S - no term is on more than that)

    |x_out - float64| <= 14 * 2^-24 * S         |x0_out - float64| <= (6 + 2) * 2^-24 * S0     (operations 1-6; alpha_s and sigma_s)

Second-order terms are 2^-24 of these.  Nothing in the bound is measured.  The float64 side works on the float64 table and on the fp32
operands as the kernel sees them; guidance is the fp32 value that crosses the C ABI.
"""
import numpy as np
import torch

U24 = 2.0 ** -24
N_OUT, N_X0 = 14, 8
NAN = float("nan")
MU, SD = 0.7, 0.5
TABLE_MUTANTS = ("h_sign", "cx_inverted", "exp_for_expm1", "history_on_step0")      # each fails the toy-model conditions
TEETH_MUTANTS = ("r_inverted", "history_sign")
STEP_MUTANTS = ("guidance_wrong_half", "x0_prev_other_sample", "c0_c1_swapped", "x0_not_divided")


def schedule_2_1():
    """float64 alphas_cumprod of the 2.1 decoder: 'linear', 0.00085 .. 0.012, 1000 steps"""
    return np.cumprod(1.0 - np.linspace(0.00085, 0.012, 1000, dtype=np.float64))


def lam_of(ac):
    ac = np.asarray(ac, dtype=np.float64)
    return 0.5 * (np.log(ac) - np.log1p(-ac))


def ac_of(lam):
    """inverse of lam_of: ac = sigmoid(2 lambda)"""
    return 1.0 / (1.0 + np.exp(-2.0 * np.asarray(lam, dtype=np.float64)))


def real_grid(ac, n, power=1.0):
    """(ac_s, ac_t) of n steps on a REAL-valued grid from l0 = lambda(ac[-1]) (noisy) to l1 = lambda(ac[0]): lambda = l1 - (l1 - l0) v^power
    with v running uniformly from 1 to 0.  power 1: uniform log-SNR; power 1.5: steps that shrink towards the clean end (r != 1)."""
    lam = lam_of(ac)
    v = np.linspace(1.0, 0.0, n + 1) ** power
    a = ac_of(lam[0] - (lam[0] - lam[-1]) * v)
    return a[:-1], a[1:]


def integer_grid(ac, ts):
    """(ac_s, ac_t) of the integer timesteps ts (execution order); the last step targets ac[0]"""
    ts = np.asarray(ts)
    return ac[ts], np.append(ac[ts[1:]], ac[0])


def table_ref(ac_s, ac_t, solver_order=2, lower_order_final=True, mut=None):
    """the restatement of sampling.dpmpp_table, written step by step from the formulas above; mut: ONE deliberately wrong variant"""
    ac_s, ac_t = np.asarray(ac_s, dtype=np.float64), np.asarray(ac_t, dtype=np.float64)
    n = len(ac_s)
    table, orders = np.zeros((n, 5)), np.ones(n, dtype=np.int64)
    h_prev = None
    for k in range(n):
        a_s, s_s, a_t, s_t = np.sqrt(ac_s[k]), np.sqrt(1 - ac_s[k]), np.sqrt(ac_t[k]), np.sqrt(1 - ac_t[k])
        h = np.log(a_t / s_t) - np.log(a_s / s_s)
        if mut == "h_sign":
            h = -h
        phi = 1.0 - np.exp(-h) if mut != "exp_for_expm1" else -np.exp(-h)
        c_x = s_t / s_s if mut != "cx_inverted" else s_s / s_t
        second = solver_order == 2 and k > 0 and not (lower_order_final and k == n - 1)
        if mut == "history_on_step0" and solver_order == 2 and k == 0 and n > 1:
            second, h_prev = True, h                      # step 0 treated as if it had a history (it reads whatever the slot holds: zeros)
        c_0, c_1 = a_t * phi, 0.0
        if second:
            r = h_prev / h
            if mut == "r_inverted":
                r = 1.0 / r
            w = 1 / (2 * r) if mut != "history_sign" else -1 / (2 * r)      # the history term D = (x0_s - x0_prev) / r enters as + D / 2
            c_0, c_1 = a_t * phi * (1 + w), -a_t * phi * w
            orders[k] = 2
        table[k] = (a_s, s_s, c_x, c_0, c_1)
        h_prev = h
    return table, orders


# ---- the toy model ---------------------------------------------------------------------------------------------------------------------
def toy_eps(x, ac):
    a, s2 = np.sqrt(ac), 1.0 - ac
    return np.sqrt(s2) * (x - MU * a) / (SD * SD * ac + s2)


def toy_exact(x_T, ac_T, ac_end):
    v = lambda c: SD * SD * c + (1.0 - c)  # noqa: E731
    return MU * np.sqrt(ac_end) + np.sqrt(v(ac_end) / v(ac_T)) * (x_T - MU * np.sqrt(ac_T))


def toy_error(table, orders, ac_s, ac_t):
    """the numpy float64 loop on the toy model, driven by a (table, orders) pair: max|x - exact| / max|exact| at the last target"""
    x = np.linspace(-3.0, 3.0, 25)
    exact = toy_exact(x, ac_s[0], ac_t[-1])
    x0_prev = np.zeros_like(x)
    for k in range(len(table)):
        a_s, s_s, c_x, c_0, c_1 = table[k]
        x0 = (x - s_s * toy_eps(x, ac_s[k])) / a_s
        x = c_x * x + c_0 * x0 + (c_1 * x0_prev if orders[k] == 2 else 0.0)
        x0_prev = x0
    return float(np.max(np.abs(x - exact)) / np.max(np.abs(exact)))


# ---- one step --------------------------------------------------------------------------------------------------------------------------
def step_inputs(N, HW, seed=0):
    """fp32 operands of one launch: x, x0_prev [N,4,HW], model_out [N,8,HW]"""
    g = torch.Generator().manual_seed(1000003 * seed + 29)
    return dict(x=0.2 + 1.5 * torch.randn(N, 4, HW, generator=g), model_out=0.1 + torch.randn(N, 8, HW, generator=g),
                x0_prev=0.3 + 1.2 * torch.randn(N, 4, HW, generator=g))


def step64(x, model_out, x0_prev, row, guidance, use_cfg=1, mut=None, dtype=torch.float64):
    """One step in `dtype` (float64: the reference on the float64 row; float32: torch's own evaluation, one rounding per operation like
    the kernel, on the row rounded to fp32) on x [N,4,...], model_out [N,8,...]; x0_prev None = order 1.  Returns (x_out, x0, S, S0)."""
    x, mo = x.to(dtype), model_out.to(dtype)
    a_s, s_s, c_x, c_0, c_1 = (torch.tensor(float(np.float32(v)) if dtype == torch.float32 else float(v), dtype=dtype) for v in row)
    g = torch.tensor(float(np.float32(guidance)), dtype=dtype)
    N = x.shape[0]
    if use_cfg:
        bs = N // 2
        c, u = mo[:bs, :4].repeat(2, *[1] * (x.dim() - 1)), mo[bs:, :4].repeat(2, *[1] * (x.dim() - 1))
        if mut == "guidance_wrong_half":
            c, u = u, c
        e = u + g * (c - u)
        E = u.abs() + g.abs() * (c.abs() + u.abs())
    else:
        e = mo[:, :4]
        E = e.abs()
    x0 = (x - s_s * e) / a_s if mut != "x0_not_divided" else (x - s_s * e)
    S0 = (x.abs() + s_s * E) / a_s
    if mut == "c0_c1_swapped":
        c_0, c_1 = c_1, c_0
    out = c_x * x + c_0 * x0
    S = c_x.abs() * x.abs() + c_0.abs() * S0
    if x0_prev is not None:
        p = x0_prev.to(dtype)
        if mut == "x0_prev_other_sample":
            p = p.roll(1, dims=0)
        out = out + c_1 * p
        S = S + c_1.abs() * p.abs()
    return out, x0, S, S0


def bound_out(S):
    return N_OUT * U24 * S


def bound_x0(S0):
    return N_X0 * U24 * S0


def violations(out, ref, bound):
    """elements of out further from ref than bound, non-finite ones included"""
    o = out.double()
    return int((~torch.isfinite(o) | ((o - ref).abs() > bound)).sum().item())


def worst_ratio(out, ref, bound):
    r = (out.double() - ref).abs() / bound.clamp_min(1e-300)
    return float(r[bound > 0].max().item()) if (bound > 0).any() else 0.0


def with_guard(t, guard, fill=NAN):
    """flat copy of t with `guard` fill elements on both sides (the layout of the GPU test's buffers)"""
    g = torch.full((guard,), fill, dtype=t.dtype, device=t.device)
    return torch.cat([g, t.reshape(-1), g])


# ---- the whole loop around a CPU model ---------------------------------------------------------------------------------------------------
def dpmpp_loop64(model, x_T, timesteps, table, orders, guidance):
    """float64 driver: model(x_in [N,4,h,w] fp32-or-64, t [N]) -> [N,8,h,w]; the UNet sees the first half of x twice (model_fn), the step is
    step64 on the float64 table.  Returns (final latent, x0 of the last step), float64."""
    x = x_T.double()
    N = x.shape[0]
    x0_prev = x0 = None
    for k, t in enumerate(timesteps):
        half = x[: N // 2]
        out = model(torch.cat([half, half], 0), torch.full((N,), float(t))).double()
        x, x0, _, _ = step64(x, out, x0_prev if orders[k] == 2 else None, table[k], guidance)
        x0_prev = x0
    return x, x0
