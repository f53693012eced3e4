"""The host-driven step loops of the three decoder samplers, each written once, and the only ctypes callers of their step kernels
(k22_sampler_step, k22_ddim_step, k22_plms_step).  SpacedDiffusionHIP.p_sample_loop, DDIMSamplerHIP / PLMSSamplerHIP.sample (diffusion.py)
and the two-chain branches of Text2ImUNetHIP.sample_loop / ddim_loop (unet.py) run them; the captured single-chain loops are the same
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


def plms_calls(steps: list) -> list:
    """`steps` in execution order -> the timestep of every PLMS model call: the first step calls the model twice, the second time at the next
    step's timestep (its own when it is the only step)"""
    return [steps[0], steps[min(1, len(steps) - 1)]] + steps[1:] if steps else []


def sampler_scratch(x: torch.Tensor) -> torch.Tensor:
    return torch.empty(_lib.lib().k22_sampler_scratch_bytes(x.shape[0], x.shape[2] * x.shape[3]), dtype=torch.uint8, device=x.device)


# ---- the three launches ----------------------------------------------------------------------------------------------------------------
def sampler_step(x, model_out, noise, row, x_out, x0_out, *, table, guidance, use_cfg, clamp, pct, init, mask, scratch):
    """One k22_sampler_step launch: row `row` of the [T,8] `table`; x0_out may be None."""
    _lib.check(_lib.lib().k22_sampler_step(
        x.data_ptr(), model_out.data_ptr(), noise.data_ptr(), _lib.ptr(init), _lib.ptr(mask), table.data_ptr(), int(row), float(guidance),
        int(use_cfg), float(clamp[0]), float(clamp[1]), int(pct[0]), float(pct[1]), scratch.data_ptr(), x_out.data_ptr(), _lib.ptr(x0_out),
        x.shape[0], x.shape[2] * x.shape[3], _lib.current_stream()))


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
