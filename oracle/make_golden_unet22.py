"""Generates tests/golden/c5_forward.pt and tests/golden/c5_loop.pt: BASELINE config C5 (Kandinsky 2.2 ControlNet-depth decoder,
768x768, bs 2 -> CFG batch [4, 8, 96, 96] plus a hint [4, 3, 768, 768]) through oracle/unet22_ref.py, the repository's own CPU
restatement of diffusers' UNet2DConditionModel / KandinskyV22ControlnetPipeline / DDPMScheduler.  PARITY UNPINNED (diffusers is
absent; see the header of oracle/unet22_ref.py): the fixtures pin the engine to the restatement, not the restatement to diffusers.

    python oracle/make_golden_unet22.py          # a few minutes of CPU, ~10 GB RAM

Weights: k22.init_unet22_state_dict(k22.make_arch22(k22.UNET_CONFIG_2_2, controlnet=True), seed=0), re-drawn by the tests.
Inputs: c5_inputs(SEED), also re-drawn by the tests; the two images get different hints (U[0, 1]) and different pos / neg embeds.
Stored:
  c5_forward.pt  one forward of the CFG batch (sample = 4 distinct latents, timesteps [980, 500, 20, 0], image_embeds = [neg | pos],
                 hint = [hint | hint]) as a compact sub-grid + bands (the full [4, 8, 96, 96] output would exceed the 1 MiB size
                 limit of a committed file), and the hint latent hint_block(hint) [2, 4, 96, 96] of the two distinct hints (the CFG
                 batch repeats them);
  c5_loop.pt     the final latent [2, 4, 96, 96] of a 5-step decoder_loop under SCHED_2_2 (= k22.SCHEDULER_CONFIG_2_2), guidance 4,
                 with injected noise.
The CPU thread count is fixed so that a regeneration reproduces the committed files bit for bit.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import kandinsky2_amd as k22  # noqa: E402
from oracle import unet22_ref  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 55
BS, LAT, STEPS, GUIDANCE = 2, 96, 5, 4.0
FIRST_T = (980.0, 500.0, 20.0, 0.0)
CPU_THREADS = 8


def c5_weights():
    cfg = k22.UNET_CONFIG_2_2
    arch = k22.make_arch22(cfg, controlnet=True)
    return cfg, arch, k22.init_unet22_state_dict(arch, seed=0)


def c5_inputs(seed=SEED):
    """hint [2,3,768,768] U[0,1], pos / neg image embeds [2,1280], first-forward sample [4,4,96,96], loop start latents [2,4,96,96],
    loop noise [5,2,4,96,96] - drawn in this order from one CPU generator."""
    g = torch.Generator().manual_seed(seed)
    hint = torch.rand(BS, 3, 8 * LAT, 8 * LAT, generator=g)
    pos, neg = torch.randn(BS, 1280, generator=g), torch.randn(BS, 1280, generator=g)
    x = torch.randn(2 * BS, 4, LAT, LAT, generator=g)
    lat = torch.randn(BS, 4, LAT, LAT, generator=g)
    nz = torch.randn(STEPS, BS, 4, LAT, LAT, generator=g)
    return dict(hint=hint, pos=pos, neg=neg, x=x, lat=lat, noise=nz)


def compact(out, stride=2, band=8):
    """strided sub-grid plus one full-resolution band of rows and one of columns (the layout of make_golden._compact; the tests'
    _compact_err reads it)."""
    H, W = out.shape[-2:]
    return dict(stride=stride, sub=out[..., ::stride, ::stride].clone(), r0=H // 2 - 3, rows=out[..., H // 2 - 3: H // 2 - 3 + band, :].clone(),
                c0=W // 3, cols=out[..., :, W // 3: W // 3 + band].clone())


@torch.no_grad()
def main():
    torch.set_num_threads(CPU_THREADS)
    os.makedirs(GOLD, exist_ok=True)
    cfg, _, sd = c5_weights()
    inp = c5_inputs()
    hint, pos, neg = inp["hint"], inp["pos"], inp["neg"]
    hint_lat = unet22_ref.hint_block(sd, hint)
    t = torch.tensor(FIRST_T)
    out = unet22_ref.unet22_forward(sd, cfg, inp["x"], t, torch.cat([neg, pos], 0), torch.cat([hint, hint], 0))
    print(f"c5 forward: out {tuple(out.shape)} absmax {out.abs().max():.4f}; hint latent absmax {hint_lat.abs().max():.4f}")
    torch.save(dict(name="c5_forward", seed=SEED, bs=BS, lat=LAT, t=t, absmax=out.abs().max().item(), forward_compact=compact(out),
                    hint_latent=hint_lat.clone()), os.path.join(GOLD, "c5_forward.pt"))
    final = unet22_ref.decoder_loop(lambda xx, tt, e, hh: unet22_ref.unet22_forward(sd, cfg, xx, tt, e, hh), inp["lat"], pos, neg, STEPS,
                                    GUIDANCE, inp["noise"], hint, sched_cfg=unet22_ref.SCHED_2_2)
    print(f"c5 {STEPS}-step loop: final latent absmax {final.abs().max():.4f}")
    torch.save(dict(name="c5_loop", seed=SEED, bs=BS, lat=LAT, steps=STEPS, guidance=GUIDANCE, final=final.clone()),
               os.path.join(GOLD, "c5_loop.pt"))


if __name__ == "__main__":
    main()
