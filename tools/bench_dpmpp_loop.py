#!/usr/bin/env python
"""Denoise-loop time of the DPM-Solver++ one-graph loop against the DDIM one-graph loop of the same run.

    python tools/bench_dpmpp_loop.py [--size 768 --bs 1 --steps 20 --long-steps 50 --dtype bf16 --reps 3 --rounds 2]

Runs Kandinsky2_1HIP.generate_img(..., decode=False) on seeded weights (the 1.23 B UNet; config C2 by default: 768x768, bs 1, bf16), every
configuration with whole_loop_graph=True:

    ddim_sampler  --steps         k22_unet_ddim_loop: the yardstick, measured in THIS run (no stored number is compared with)
    dpm_sampler   --steps         k22_unet_dpmpp_loop, order 2M on the log-SNR grid: the same number of model calls (asserted)
    ddim_sampler  --long-steps    the documented 50-call generation, for the generation-time ratio a user gets from fewer calls

What is expected: the two --steps loops cost the same per model call within the spread this tool measures - the loops differ in the step
kernel alone, and the DPM++ step reads and writes one more [N,4,h,w] fp32 tensor than the DDIM step (147 KB at C2).  The tool says
nothing about image quality (seeded weights).

Each generation is timed with a host clock between two device synchronisations, after one untimed generation per visit (plan, tile
selection, graph capture: one engine keeps one captured loop, so a change of configuration re-captures).  The configurations are visited
`--rounds` times in turn, `--reps` timed generations per visit; per configuration the median, the extremes and the spread
(max - min) / median of all its timed generations are printed, then one JSON line with everything."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kandinsky2_amd as k22  # noqa: E402
from kandinsky2_amd import sampling  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=768, help="image side in pixels (latent = size/8)")
    ap.add_argument("--bs", type=int, default=1, help="images per generation (CFG batch = 2*bs)")
    ap.add_argument("--steps", type=int, default=20, help="model calls of the two loops that are compared")
    ap.add_argument("--long-steps", type=int, default=50, help="model calls of the long DDIM generation")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32", "f16x3", "f16x2"])
    ap.add_argument("--reps", type=int, default=3, help="timed generations per configuration and round")
    ap.add_argument("--rounds", type=int, default=2, help="visits of every configuration (reps * rounds = 6 timed generations each by default)")
    ap.add_argument("--tiny", action="store_true", help="1/3-width UNet (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args(argv)
    if a.reps * a.rounds < 5:
        ap.error("reps * rounds must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("bench_dpmpp_loop: needs the GPU (no CPU fallback)")
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32, "f16x3": k22.F16X3, "f16x2": k22.F16X2}[a.dtype]
    configs = [("ddim_sampler", a.steps), ("dpm_sampler", a.steps), ("ddim_sampler", a.long_steps)]

    cfg = copy.deepcopy(k22.CONFIG_2_1)
    if a.tiny:
        cfg["model_config"] = k22.tiny_model_config()
    hp = k22.tiny_prior_hparams()
    cfg["prior"]["params"]["model"]["hparams"] = hp
    g = torch.Generator().manual_seed(17)
    cfg["prior"]["clip_mean_std_path"] = (torch.randn(768, generator=g) * 0.1, torch.rand(768, generator=g) + 0.5)
    marc = k22.MoVQArch(k22.MOVQ_CONFIG_2_1["ddconfig"])
    cfg["image_enc_params"]["ckpt_path"] = dict(k22.init_movq_state_dict(marc, seed=0))
    arch = k22.make_arch(cfg["model_config"], inpainting=False)
    pipe = k22.Kandinsky2_1HIP(cfg, k22.init_unet_state_dict(arch, seed=0), k22.init_prior_state_dict(hp, seed=0), "cuda", task_type="text2img",
                               conditioner="seeded", backend_dtype=tdt, whole_loop_graph=True)

    prompt, lat = "a red cat, 4k photo", a.size // 8
    x_T = torch.randn(2 * a.bs, 4, lat, lat, generator=g).cuda()
    image_emb = torch.randn(2 * a.bs, 768, generator=g).cuda()
    text_embs = pipe.encode_text(prompt, a.bs)
    L = k22._lib.lib()
    _, diffusion = pipe._diffusion("ddim_sampler", a.steps)       # the un-respaced schedule serves both samplers

    def model_calls(sampler, steps):
        if sampler == "dpm_sampler":
            return len(sampling.dpmpp_grid(diffusion.alphas_cumprod, steps, "logsnr"))
        return len(range(0, 1000, 1000 // steps))
    calls = {c: model_calls(*c) for c in configs}
    assert calls[configs[0]] == calls[configs[1]], f"the compared loops make {calls[configs[0]]} and {calls[configs[1]]} model calls: pick another --steps"

    def generation(sampler, steps):
        return pipe.generate_img(prompt, image_emb, batch_size=a.bs, diffusion=diffusion, guidance_scale=4, noise=x_T, h=a.size, w=a.size,
                                 sampler=sampler, num_steps=steps, text_embs=text_embs, decode=False)

    times, finals = {c: [] for c in configs}, {}
    for rnd in range(a.rounds):
        for c in configs:
            launches = L.k22_debug_counter(b"loop_launches")
            out = generation(*c)                      # untimed: plan / capture
            torch.cuda.synchronize()
            assert L.k22_debug_counter(b"loop_launches") - launches == 1, "the generation did not run as one loop"
            finals.setdefault(c, out.clone())
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = generation(*c)
                torch.cuda.synchronize()
                times[c].append(time.perf_counter() - t0)
            assert torch.equal(out, finals[c]) and torch.isfinite(out).all(), f"{c}: the generations of one configuration differ"

    print(f"{'tiny' if a.tiny else '1.23 B'} UNet, {a.size}x{a.size}, bs {a.bs}, {a.dtype}, whole_loop_graph=True; "
          f"{a.reps * a.rounds} timed generations per configuration in {a.rounds} rounds")
    rows = []
    for c in configs:
        t = sorted(times[c])
        med = statistics.median(t)
        row = dict(sampler=c[0], num_steps=c[1], model_calls=calls[c], median_ms=med * 1e3, min_ms=t[0] * 1e3, max_ms=t[-1] * 1e3,
                   spread=(t[-1] - t[0]) / med, ms_per_model_call=med * 1e3 / calls[c], n=len(t))
        rows.append(row)
        print(f"{c[0]:13s} num_steps={c[1]:3d}  {calls[c]:3d} model calls  median {row['median_ms']:8.2f} ms  min {row['min_ms']:8.2f}  "
              f"max {row['max_ms']:8.2f}  spread {100 * row['spread']:5.2f} %  {row['ms_per_model_call']:7.3f} ms / model call")
    ddim, dpm, long_ = rows
    ratio = dpm["ms_per_model_call"] / ddim["ms_per_model_call"]
    within = abs(ratio - 1.0) <= max(ddim["spread"], dpm["spread"])
    print(f"ms per model call, dpm_sampler / ddim_sampler at {calls[configs[0]]} calls: {ratio:.4f} "
          f"({'within' if within else 'OUTSIDE'} the larger of the two spreads, {100 * max(ddim['spread'], dpm['spread']):.2f} %)")
    print(f"generation time, dpm_sampler {dpm['model_calls']} calls / ddim_sampler {long_['model_calls']} calls: "
          f"{dpm['median_ms']:.1f} ms / {long_['median_ms']:.1f} ms = {dpm['median_ms'] / long_['median_ms']:.3f}")
    print(json.dumps(dict(size=a.size, bs=a.bs, dtype=a.dtype, tiny=a.tiny, per_call_ratio=ratio, per_call_ratio_within_spread=within,
                          generation_ratio=dpm["median_ms"] / long_["median_ms"], results=rows)))


if __name__ == "__main__":
    main()
