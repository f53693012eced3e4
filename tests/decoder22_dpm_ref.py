"""Float64 restatements and bounds of the DPM-Solver++ sampler on the Kandinsky 2.2 decoders (k22_dpmpp_step_clip, k22_unet_dpmpp_loop_keep,
sampling.dpmpp_schedule / dpmpp_keep_coef, the decoders' sampler="dpm_sampler") for tests/test_decoder22_dpm_cpu.py and
tests/test_decoder22_dpm_gpu.py.  A plain module like dpmpp_ref.py, on which it builds.

PARITY UNPINNED twice over: the sampler has no counterpart in the reference (dpmpp_ref.py), and the 2.2 UNet arithmetic is restated from
memory (oracle/unet22_ref.py).  The sampler has never run on trained 2.2 weights; what is known about its accuracy is dpmpp_ref's toy model.

The clamped step.  k22_dpmpp_step_clip is k22_dpmpp_step (dpmpp_ref lists its eleven operations) with one more after operation 6:

    6' x0 = clamp(x0, lo, hi)        two comparisons, no rounding; the clamped x0 enters operation 8 and is what x0_out stores

The bound.  The clamp is exact and non-expansive: |clamp(a) - clamp(b)| <= |a - b|, so the clamped fp32 x0 is no further from the clamped
float64 x0 than the unclamped pair was - bound_x0 = 8 * 2^-24 * S0 holds as derived in dpmpp_ref.  Downstream |clamp(x0)| <= min(S0, C),
C = max(|lo|, |hi|), so every term of dpmpp_ref's S that the clamped value is on shrinks; charging them S0 as before over-estimates, and
bound_out = 14 * 2^-24 * S with the unclamped S0 inside S holds too.  Both are used unchanged: nothing in them is measured.

Mutants (each one wrong reading of "clamp the data prediction"; all must fall outside the bounds on inputs that reach both sides of the
clamp): the clamp on x_out instead of x0; x_out formed from the unclamped x0; x0_out stored unclamped; lo and hi swapped (with the
kernel's comparisons, `x0 < hi -> hi` then `x0 > lo -> lo`: everything ends at lo).
"""
import numpy as np
import torch

import dpmpp_ref as R

CLIP_MUTANTS = ("clamp_on_x_out", "x_out_from_unclamped_x0", "x0_out_unclamped", "bounds_swapped")
NO_CLIP = (-3.0e38, 3.0e38)          # the DDPM route's "no clip": min(scheduler.clip, 3.0e38)


def schedule_2_2():
    """float64 alphas_cumprod of SCHEDULER_CONFIG_2_2 ('linear', 0.00085 .. 0.012, 1000 steps): the 2.1 array"""
    return R.schedule_2_1()


def _clamp(v, lo, hi):
    """the kernel's two comparisons (a NaN fails both and passes through)"""
    v = torch.where(v < lo, torch.full_like(v, lo), v)
    return torch.where(v > hi, torch.full_like(v, hi), v)


def step64_clip(x, model_out, x0_prev, row, guidance, use_cfg=1, clamp=NO_CLIP, mut=None, dtype=torch.float64):
    """dpmpp_ref.step64 with the clamp on x0.  Returns (x_out, x0 as stored, S, S0, share of x0 elements the clamp moved)."""
    lo, hi = float(np.float32(clamp[0])), float(np.float32(clamp[1]))
    _, raw, S, S0 = R.step64(x, model_out, x0_prev, row, guidance, use_cfg, dtype=dtype)
    if mut == "bounds_swapped":
        lo, hi = hi, lo
    x0 = _clamp(raw, lo, hi)
    a_s, s_s, c_x, c_0, c_1 = (torch.tensor(float(np.float32(v)) if dtype == torch.float32 else float(v), dtype=dtype) for v in row)
    used = raw if mut in ("x_out_from_unclamped_x0", "clamp_on_x_out") else x0
    out = c_x * x.to(dtype) + c_0 * used
    if x0_prev is not None:
        out = out + c_1 * x0_prev.to(dtype)
    if mut == "clamp_on_x_out":
        out, x0 = _clamp(out, lo, hi), raw
    if mut == "x0_out_unclamped":
        x0 = raw
    share = float((x0 != raw).double().mean().item())
    return out, x0, S, S0, share


def dpmpp_loop64_clip(model, x_T, timesteps, table, orders, guidance, clamp=NO_CLIP, extra=None, keep=None):
    """dpmpp_ref.dpmpp_loop64 with the clamped step, for the 2.2 decoders: model(x_in [N,C,h,w], t) -> [N,8,h,w]; the UNet sees the first half
    of x twice, `extra` [N,5,h,w] appended (inpainting); keep = (init [1,4,h,w], noise0 [N/2,4,h,w], mask [1,1,h,w], coef [n,2]): after step
    k the known region becomes coef[k,0] init + coef[k,1] noise0 on both halves.  float64 throughout; returns (final latent, last x0)."""
    x = x_T.double()
    N = x.shape[0]
    x0_prev = x0 = None
    for k, t in enumerate(timesteps):
        half = x[: N // 2]
        inp = torch.cat([half, half], 0)
        if extra is not None:
            inp = torch.cat([inp, extra.double()], 1)
        out = model(inp, float(t)).double()
        x, x0, _, _, _ = step64_clip(x, out, x0_prev if orders[k] == 2 else None, table[k], guidance, 1, clamp)
        if keep is not None:
            init, noise0, mask, coef = keep
            known = float(coef[k, 0]) * init.double() + float(coef[k, 1]) * torch.cat([noise0, noise0], 0).double()
            x = mask.double() * known + (1.0 - mask.double()) * x
        x0_prev = x0
    return x, x0
