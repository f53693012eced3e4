"""The host-driven step loops of the three decoder samplers, each written once, and the only ctypes callers of their step kernels
(k22_sampler_step, k22_ddim_step, k22_plms_step, k22_dpmpp_step[_clip]).  SpacedDiffusionHIP.p_sample_loop, DDIMSamplerHIP / PLMSSamplerHIP.sample (diffusion.py)
and the two-chain route of the UNet modules' whole-loop entries (Text2ImUNetHIP._run_loop, unet.py) run them; the captured single-chain loops are the same
sequences in C++ (csrc/engine.hip).  A loop takes `model_call(latent, call_index) -> [N,8,H,W]`, the schedule rows in execution order
and a step launcher, to which it hands its keywords (guidance, clamp, ...) through: the host tests pass recording launchers.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def cfg_input(x: torch.Tensor) -> torch.Tensor:
    """model_fn's UNet input (kandinsky2_1_model.py:222-224): the first half twice - the second half of x is never fed to the UNet"""
    half = x[: x.shape[0] // 2]
    return torch.cat([half, half], 0)


def fused_call(model, ts_rows, **kw):
    """model_call of the fused callers: the UNet on cfg_input(latent) at row c of ts_rows [n_calls, N] (every model call's timestep, in
    execution order)"""
    return lambda x, c: model(cfg_input(x), ts_rows[c], **kw)


def step_noise(x: torch.Tensor, n: int, noise_seq=None) -> torch.Tensor:
    """[n, *x.shape]: the noise of n steps - the head of noise_seq, else n randn_like(x) draws in step order"""
    if noise_seq is not None:
        return noise_seq[:n].to(x.device).float().contiguous()
    nzs = torch.empty(n, *x.shape, device=x.device)
    for k in range(n):
        nzs[k] = torch.randn_like(x)
    return nzs


def ddpm_loop_operands(scheduler, timesteps, B: int, keep: bool = False):
    """Host side of the one-graph 2.2 decoder loop (UNet2DConditionHIP.sample_loop): a DDPMSchedulerHIP after set_timesteps and the
    retained timesteps in execution order (all of scheduler.timesteps, or img2img's tail) -> (ts_rows [n, B] fp32: the value every row
    of the UNet receives at step k, as the stepwise loop's `unet(inp, t)`; table_rows: the row of scheduler's step table of every step,
    as `scheduler.step(out, t, ...)` looks it up; keep_coef).  keep_coef (keep=True, the inpainting re-imposition; else None) is
    [n, 2] fp32: row k = (sqrt(ac[ts[k + 1]]), sqrt(1 - ac[ts[k + 1]])), the last row (1, 0) - computed in float64 and rounded to fp32 the
    way the stepwise route's `a ** 0.5` is when it crosses the C ABI as a float.  No GPU is touched."""
    ts = [int(t) for t in timesteps]
    n = len(ts)
    ts_rows = torch.tensor(ts, dtype=torch.float32).reshape(n, 1).expand(n, B).contiguous()
    rows = [scheduler._row[t] for t in ts]
    coef = None
    if keep:
        ac = scheduler.alphas_cumprod
        coef = np.zeros((n, 2), dtype=np.float32)
        for k in range(n):
            a = float(ac[ts[k + 1]]) if k + 1 < n else 1.0
            coef[k] = (a ** 0.5, (1.0 - a) ** 0.5)
    return ts_rows, rows, coef


def ddpm_step_noise(n_steps: int, shape, generator=None, device="cuda") -> torch.Tensor:
    """[n_steps, *shape]: the ancestral noise of a whole DDPM loop by the very draws DDPMSchedulerHIP.step makes when it is given no
    noise - one torch.randn(shape) per step, in step order (the caller has drawn the initial latent before); a CPU generator draws on
    the CPU and the noise moves over (diffusers' randn_tensor).  shape is the sample the scheduler steps: the CFG batch [2 bs, 4, h, w].
    So a seed gives the same image whether the loop is driven step by step or replayed as one graph."""
    gdev = generator.device if generator is not None else device
    out = torch.empty((n_steps,) + tuple(shape), dtype=torch.float32, device=device)
    for k in range(n_steps):
        out[k] = torch.randn(tuple(shape), generator=generator, device=gdev).to(device)
    return out


def keep_region(x, init, noise0, mask, sa, sb, out):
    """One k22_keep_region launch over the CFG batch x [B,4,h,w] (out may be x)."""
    _lib.check(_lib.lib().k22_keep_region(x.data_ptr(), init.data_ptr(), noise0.data_ptr(), mask.data_ptr(), float(sa), float(sb), out.data_ptr(),
                                          x.shape[0], x.shape[2] * x.shape[3], _lib.current_stream()))


def keep_operands(name: str, keep, bs: int, H: int, W: int, n_steps: int, host: bool = False):
    """The known region of a 2.2 loop entry `name`, keep = (init [1,4,h,w], noise0 [bs,4,h,w], mask [1,1,h,w], coef [n_steps,2]) or None,
    checked -> (init [4,h,w], noise0, mask [h,w], coef as a contiguous fp32 host array): what the entry stages and hands to C.  host: the
    three tensors as the contiguous fp32 the keep_region launches of a host-driven loop read.  None stays None; a checked tuple passes again."""
    if keep is None:
        return None
    k_init, k_noise, k_mask, coef = keep
    coef = np.ascontiguousarray(coef, dtype=np.float32)
    if k_init.numel() != 4 * H * W or tuple(k_noise.shape) != (bs, 4, H, W) or k_mask.numel() != H * W or coef.shape != (n_steps, 2):
        raise ValueError(f"{name}: keep = (init [1,4,h,w], noise0 [bs,4,h,w], mask [1,1,h,w], coef [n_steps,2])")
    kept = (k_init.reshape(4, H, W), k_noise, k_mask.reshape(H, W))
    return (tuple(t.float().contiguous() for t in kept) if host else kept) + (coef,)


def plms_calls(steps: list) -> list:
    """`steps` in execution order -> the timestep of every PLMS model call: the first step calls the model twice, the second time at the next
    step's timestep (its own when it is the only step)"""
    return [steps[0], steps[min(1, len(steps) - 1)]] + steps[1:] if steps else []


# ---- DPM-Solver++ (2M, data prediction): grid and coefficient table, float64, no GPU -----------------------------------------------------
def log_snr(ac) -> np.ndarray:
    """lambda = ln(alpha / sigma) of alphas_cumprod values, alpha = sqrt(ac), sigma = sqrt(1 - ac)"""
    ac = np.asarray(ac, dtype=np.float64)
    return 0.5 * (np.log(ac) - np.log1p(-ac))


def dpmpp_grid(ac, S: int, discretize: str = "logsnr", init_step=None) -> np.ndarray:
    """The integer timesteps of a DPM-Solver++ generation in EXECUTION order (noisy first) on the float64 alphas_cumprod `ac` of the
    un-respaced schedule; the last step targets ac[0].
      "uniform": DDIMSamplerHIP.make_schedule's grid (1, 1 + T // S, ...), flipped.
      "logsnr":  S + 1 targets uniform in lambda from lambda(ac[T - 1]) to lambda(ac[0]); for each of the first S the integer t in
                 1 .. T - 1 whose lambda(ac[t]) is nearest, duplicates dropped - so the result may hold FEWER than S steps (the 2.1
                 schedule: S = 20 gives 20, S = 50 gives 48: near t = T the schedule itself is coarser in lambda than the targets).
    init_step keeps the timesteps t <= init_step (apply_init_step)."""
    ac = np.asarray(ac, dtype=np.float64)
    T, S = len(ac), int(S)
    if S < 1:
        raise ValueError("dpmpp_grid: S must be >= 1")
    if discretize == "uniform":
        steps = (np.asarray(list(range(0, T, T // S))) + 1)[::-1]
    elif discretize == "logsnr":
        lam = log_snr(ac)
        cand = np.arange(1, T)
        steps = []
        for target in np.linspace(lam[T - 1], lam[0], S + 1)[:S]:
            t = int(cand[np.argmin(np.abs(lam[cand] - target))])
            if t not in steps:
                steps.append(t)
        steps = np.asarray(steps)
    else:
        raise ValueError(f'dpmpp_grid: discretize must be "logsnr" or "uniform"; got {discretize!r}')
    if init_step is not None:
        steps = np.array([i for i in steps if i <= init_step])
    return steps.astype(np.int64)


def dpmpp_table(ac_s, ac_t, solver_order: int = 2, lower_order_final: bool = True):
    """DPM-Solver++ multistep coefficients, data-prediction form.  ac_s / ac_t: float64 alphas_cumprod of every step's current and target
    point, in execution order.  Returns (table float64 [n][5], orders int [n]); row k = (alpha_s, sigma_s, c_x, c_0, c_1) with

        x0_s = (x - sigma_s e) / alpha_s            x_t = c_x x + c_0 x0_s + c_1 x0_prev

    h = lambda_t - lambda_s > 0, phi = -expm1(-h).  Order 1: c_x = sigma_t / sigma_s, c_0 = alpha_t phi, c_1 = 0 exactly (the eta = 0 DDIM
    update).  Order 2 (2M), r = h_prev / h: c_0 = alpha_t phi (1 + 1 / (2 r)), c_1 = -alpha_t phi / (2 r).  orders[k] = 1 for k = 0, for
    solver_order 1 and, with lower_order_final, for the last step; else 2.  Everything in float64; the caller rounds to fp32 once."""
    if solver_order not in (1, 2):
        raise ValueError("dpmpp_table: solver_order must be 1 or 2")
    ac_s, ac_t = np.asarray(ac_s, dtype=np.float64), np.asarray(ac_t, dtype=np.float64)
    if ac_s.shape != ac_t.shape or ac_s.ndim != 1:
        raise ValueError("dpmpp_table: ac_s and ac_t are 1-D arrays of one length")
    n = len(ac_s)
    a_s, s_s, a_t, s_t = np.sqrt(ac_s), np.sqrt(1.0 - ac_s), np.sqrt(ac_t), np.sqrt(1.0 - ac_t)
    h = log_snr(ac_t) - log_snr(ac_s)
    phi = -np.expm1(-h)
    table, orders = np.zeros((n, 5), dtype=np.float64), np.ones(n, dtype=np.int32)
    table[:, 0], table[:, 1], table[:, 2], table[:, 3] = a_s, s_s, s_t / s_s, a_t * phi
    for k in range(1, n):
        if solver_order == 2 and not (lower_order_final and k == n - 1):
            inv2r = h[k] / (2.0 * h[k - 1])          # 1 / (2 r), r = h_prev / h
            orders[k] = 2
            table[k, 3] = a_t[k] * phi[k] * (1.0 + inv2r)
            table[k, 4] = -a_t[k] * phi[k] * inv2r
    return table, orders


def dpmpp_schedule(ac, S: int, solver_order: int = 2, lower_order_final: bool = True, discretize: str = "logsnr", init_step=None):
    """(timesteps in execution order, table float64 [n,5], orders) of one DPM-Solver++ generation on the float64 alphas_cumprod `ac`:
    dpmpp_grid's timesteps and dpmpp_table's coefficients between consecutive ones; the last step targets ac[0].  n may be smaller than S
    (dpmpp_grid) and is 0 when init_step leaves nothing.  The 2.1 sampler (DPMSolverSamplerHIP.make_dpm_schedule) and the 2.2 decoders
    (pipeline22) share it: the 2.2 DDPM scheduler's alphas_cumprod is the 2.1 array."""
    ac = np.asarray(ac, dtype=np.float64)
    timesteps = dpmpp_grid(ac, S, discretize, init_step)
    ac_t = np.asarray(ac[timesteps[1:]].tolist() + [ac[0]])[: len(timesteps)]
    table, orders = dpmpp_table(ac[timesteps], ac_t, solver_order, lower_order_final)
    return timesteps, table, orders


def dpmpp_keep_coef(ac, timesteps) -> np.ndarray:
    """[n, 2] fp32, the k22_keep_region coefficients of an inpainting DPM-Solver++ loop over `timesteps` (execution order): row k =
    (sqrt(ac_target_k), sqrt(1 - ac_target_k)) with ac_target_k = ac[timesteps[k + 1]] - the noise level step k arrives at - computed in
    float64 and rounded once; the last row is (1, 0): the known region comes back CLEAN, as the DDPM route un-noises it after the last step.
    The unknown region ends where every dpm_sampler result ends, at ac[0] (a residual noise level of sqrt(1 - ac[0]) = 0.029 on the 2.x
    schedule), not at ac = 1: the solver's last step targets ac[0]."""
    ac = np.asarray(ac, dtype=np.float64)
    ts = [int(t) for t in timesteps]
    coef = np.zeros((len(ts), 2), dtype=np.float32)
    for k in range(len(ts)):
        a = float(ac[ts[k + 1]]) if k + 1 < len(ts) else 1.0
        coef[k] = (np.sqrt(a), np.sqrt(1.0 - a))
    return coef


def sampler_scratch(x: torch.Tensor) -> torch.Tensor:
    return torch.empty(_lib.lib().k22_sampler_scratch_bytes(x.shape[0], x.shape[2] * x.shape[3]), dtype=torch.uint8, device=x.device)


# ---- the three launches ----------------------------------------------------------------------------------------------------------------
def threshold_group(group, N: int, use_cfg=True):
    """p_sampler's threshold group checked against a batch of N rows -> None (one group: the call as it has always been) or the int that
    k22_sampler_step_groups / k22_unet_set_threshold_group take.  group: rows of the cond half that share the 99.5th percentile of their
    first row - batch_size where several prompts are packed into one CFG batch - or None.  No GPU is touched."""
    half = N // 2 if use_cfg else N
    if group is None:
        return None
    g = int(group)
    if g != group or g < 1 or half % g or half // g > 64:
        raise ValueError(f"threshold_group must be an int >= 1 that divides the cond half of the batch ({half} rows) into at most 64 groups; got {group!r}")
    return None if g == half else g


def sampler_step(x, model_out, noise, row, x_out, x0_out, *, table, guidance, use_cfg, clamp, pct, init, mask, scratch, group=None):
    """One k22_sampler_step launch: row `row` of the [T,8] `table`; x0_out may be None.  group (threshold_group's int): k22_sampler_step_groups."""
    head = (x.data_ptr(), model_out.data_ptr(), noise.data_ptr(), _lib.ptr(init), _lib.ptr(mask), table.data_ptr(), int(row), float(guidance),
            int(use_cfg), float(clamp[0]), float(clamp[1]), int(pct[0]), float(pct[1]))
    tail = (scratch.data_ptr(), x_out.data_ptr(), _lib.ptr(x0_out), x.shape[0], x.shape[2] * x.shape[3], _lib.current_stream())
    if group is None:
        _lib.check(_lib.lib().k22_sampler_step(*head, *tail))
    else:
        _lib.check(_lib.lib().k22_sampler_step_groups(*head, int(group), *tail))


def ddim_step(x, model_out, noise, row, x_out, x0_out, *, guidance):
    """One k22_ddim_step launch: `row` = the step's [4] table row; noise is None at eta 0."""
    _lib.check(_lib.lib().k22_ddim_step(x.data_ptr(), model_out.data_ptr(), _lib.ptr(noise), row.data_ptr(), float(guidance), 1, x_out.data_ptr(),
                                        x0_out.data_ptr(), x.shape[0], x.shape[2] * x.shape[3], _lib.current_stream()))


def plms_step(x, model_out, hist, order, row, x_out, eps_out, x0_out, *, guidance):
    """One k22_plms_step launch; hist = eps history, newest first (as many tensors as `order` needs); eps_out / x0_out may be None."""
    h = [t.data_ptr() for t in hist] + [None, None, None]
    _lib.check(_lib.lib().k22_plms_step(x.data_ptr(), model_out.data_ptr(), h[0], h[1], h[2], order, row.data_ptr(), float(guidance), 1,
                                        x_out.data_ptr(), _lib.ptr(eps_out), _lib.ptr(x0_out), x.shape[0], x.shape[2] * x.shape[3],
                                        _lib.current_stream()))


def dpmpp_step(x, model_out, x0_prev, row, x_out, x0_out, *, guidance, clamp=None):
    """One k22_dpmpp_step launch: `row` = the step's [5] table row (dpmpp_table); x0_prev = the previous step's x0_out for an order-2 row,
    None for an order-1 row; x0_out always receives this step's data prediction.  clamp=(lo, hi): k22_dpmpp_step_clip, the data prediction
    clamped before it is used and stored."""
    if clamp is not None:
        _lib.check(_lib.lib().k22_dpmpp_step_clip(x.data_ptr(), model_out.data_ptr(), _lib.ptr(x0_prev), row.data_ptr(), float(guidance), 1,
                                                  float(clamp[0]), float(clamp[1]), x_out.data_ptr(), x0_out.data_ptr(), x.shape[0],
                                                  x.shape[2] * x.shape[3], _lib.current_stream()))
        return
    _lib.check(_lib.lib().k22_dpmpp_step(x.data_ptr(), model_out.data_ptr(), _lib.ptr(x0_prev), row.data_ptr(), float(guidance), 1,
                                         x_out.data_ptr(), x0_out.data_ptr(), x.shape[0], x.shape[2] * x.shape[3], _lib.current_stream()))


# ---- the loops -------------------------------------------------------------------------------------------------------------------------
def step_loop(model_call, x, rows, noise, x0, step, **operands):
    """p_sampler (step = sampler_step, rows = table row indices, x0 optional) and DDIM (ddim_step, rows = the [n,4] table): per step
    k one model call and step(x, model_out, noise[k], rows[k], x_next, x0).  noise: [n, ...] or None.  Returns (final latent, x0)."""
    x_next = torch.empty_like(x)
    for k, row in enumerate(rows):
        step(x, model_call(x, k), None if noise is None else noise[k], row, x_next, x0, **operands)
        x, x_next = x_next, x
    return x, x0


def plms_loop(model_call, x, rows, step, **operands):
    """PLMS (samplers.py:500-637) over the [n,4] table `rows`: step(x, model_out, hist, order, row, x_next, eps_out, x0_out).  The guided eps
    of a step goes to the slot of a ring of four that none of the (at most three) live history entries holds.  The first step runs in two
    stages: order 0 writes e_t and a provisional x_prev, the model is called again on it (call 1), order 4 averages the two eps; then
    Adams-Bashforth of order 1, 2, 3, 3, ... on the history, newest first.  Returns (final latent, predicted x0 of the last step)."""
    x_next, x0 = torch.empty_like(x), torch.empty_like(x)
    ring, hist, call = [torch.empty_like(x) for _ in range(4)], [], 0
    for row in rows:
        eps = next(b for b in ring if all(b is not h for h in hist))
        out = model_call(x, call)
        if not hist:
            step(x, out, [], 0, row, x_next, eps, None, **operands)
            call += 1
            step(x, model_call(x_next, call), [eps], 4, row, x_next, None, x0, **operands)
        else:
            step(x, out, hist, len(hist), row, x_next, eps, x0, **operands)
        call += 1
        hist = [eps] + hist[:2]
        x, x_next = x_next, x
    return x, x0


def dpmpp_loop(model_call, x, rows, orders, step, **operands):
    """DPM-Solver++ over the [n,5] table `rows` (dpmpp_table) and the host ints `orders`: per step k one model call and
    step(x, model_out, x0_prev, rows[k], x_next, x0_out).  Step k writes its x0 to slot k % 2 of a ring of two and, when orders[k] == 2,
    reads slot (k - 1) % 2 - the launches of k22_unet_dpmpp_loop.  Returns (final latent, x0 of the last step)."""
    x_next, hist = torch.empty_like(x), [torch.empty_like(x), torch.empty_like(x)]
    x0 = hist[0]
    for k, row in enumerate(rows):
        order = int(orders[k])
        if order not in (1, 2) or (k == 0 and order != 1):
            raise ValueError("dpmpp_loop: orders are 1 or 2, and the first step is order 1 (it has no history)")
        x0 = hist[k % 2]
        step(x, model_call(x, k), hist[(k - 1) % 2] if order == 2 else None, row, x_next, x0, **operands)
        x, x_next = x_next, x
    return x, x0


def dpmpp_loop_keep(model_call, x, rows, orders, *, guidance, clamp, keep=None):
    """dpmpp_loop with the step of k22_unet_dpmpp_loop_keep, driven from the host: dpmpp_step(clamp=) and then, with keep = (init [4,h,w],
    noise0 [B/2,4,h,w], mask [h,w] - contiguous fp32 device tensors - and coef [n,2], a host array), keep_region on the freshly written
    latent with coef[k].  The same launches on the same values as the captured loop: the same bits."""
    done = []        # the steps launched so far: the row of coef the next keep_region takes

    def step(xc, model_out, x0_prev, row, x_out, x0_out, **kw):
        dpmpp_step(xc, model_out, x0_prev, row, x_out, x0_out, **kw)
        if keep is not None:
            keep_region(x_out, keep[0], keep[1], keep[2], keep[3][len(done), 0], keep[3][len(done), 1], x_out)
        done.append(1)

    return dpmpp_loop(model_call, x, rows, orders, step, guidance=guidance, clamp=clamp)


class OwnedBuffers:
    """The operand buffers of one whole-loop entry, owned by the module: the captured loop holds their addresses, so a second generation
    under the same key replays it.  stage() allocates only when the key changes and copies the operands in."""

    def __init__(self):
        self.key, self.bufs = None, {}

    def stage(self, key, device, shapes, operands: dict) -> dict:
        """shapes(), asked on a key change: name -> fp32 shape, byte count (uint8) or None (no such operand: a null pointer); operands: name ->
        the tensor copied into that buffer, None = zeros, in this order."""
        if self.key != key:
            self.bufs = {n: None if s is None else torch.empty(s, dtype=torch.uint8 if isinstance(s, int) else torch.float32, device=device)
                         for n, s in shapes().items()}
            self.key = key
        for n, v in operands.items():
            if self.bufs[n] is not None:
                self.bufs[n].zero_() if v is None else self.bufs[n].copy_(v)
        return self.bufs
