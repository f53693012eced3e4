#!/usr/bin/env python
"""Denoise-loop time of the Kandinsky 2.2 decoders, stepwise against the one-graph loop.

    python tools/bench_decoder22_loop.py [--size 768 --steps 50 --dtype bf16 --reps 5 --out profiles/decoder22_loop.txt]

Runs the decoder call with output_type="latent" (no MoVQ) on seeded weights (the 1.25 B UNet2DConditionModel of UNET_CONFIG_2_2) for

    text2img     bs 1   KandinskyV22DecoderHIP          whole_loop_graph False / True
    inpainting   bs 2   KandinskyV22InpaintDecoderHIP   whole_loop_graph False / True   (9-channel UNet, known region re-imposed every step)

whole_loop_graph=False is the host-driven loop (per step: three torch.cat, one k22_unet_forward replay, one DDPMSchedulerHIP.step, and for
inpainting one k22_blend_noised launch per sample); True is UNet2DConditionHIP.sample_loop -> k22_unet_sample_loop_keep, one replay.
Each generation is timed with a host clock between two device synchronisations, after one untimed generation per route (plans, tile
selection, graph capture).  The two routes ALTERNATE, `--reps` (>= 5) timed generations each, in one process, so that a drift of the box
lands on both; per route the median, the extremes and the spread (max - min) / median are printed, then one JSON line.  The per-step noise
is drawn from the seeded default generator on both routes (the same draws: sampling.ddpm_step_noise), the initial latent is handed in.
text2img gives the same bits on both routes (asserted).  Inpainting re-imposes the known region with k22_keep_region on one route and
k22_blend_noised on the other: each step equal to rounding, and the loop amplifies that like any perturbation.  The yardstick printed beside
the routes' distance is the stepwise route against ITSELF with the initial latent moved by one fp32 ulp.

    python tools/bench_decoder22_loop.py --sampler dpm_sampler [--calls 20 --long-steps 50 --size 768 --dtype bf16 --reps 5]

compares SAMPLERS instead of routes, text2img bs 1, every loop as one graph (whole_loop_graph=True):

    dpm_sampler    --calls        k22_unet_dpmpp_loop_keep, order 2M on the log-SNR grid
    ddpm_sampler   --calls        k22_unet_sample_loop_keep with the same number of model calls (asserted): the yardstick, measured in this run
    ddpm_sampler   --long-steps   the 50-step generation, for the generation-time ratio a user gets from fewer calls

The three configurations alternate in one process, `--reps` visits each; one engine keeps one captured loop, so every visit is one untimed
generation (the re-capture) and one timed one.  Per configuration the median, the extremes and the spread are printed, then the per-call
ratio and the generation ratio, then one JSON line.  It says nothing about image quality (seeded weights)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kandinsky2_amd as k22  # noqa: E402
from kandinsky2_amd import pipeline22  # noqa: E402


def _case(task, bs, a, tdt, L):
    cfg = k22.tiny_unet22_config() if a.tiny else k22.UNET_CONFIG_2_2
    arch = k22.make_arch22(cfg, inpainting=task == "inpainting")
    unet = k22.UNet2DConditionHIP(arch, backend_dtype=tdt, use_graph=True)
    unet.load_state_dict(k22.init_unet22_state_dict(arch, seed=0))
    unet = unet.to("cuda").eval()
    unet.prepare(free_params=True)
    lat = a.size // 8
    g = torch.Generator().manual_seed(17)
    pos, neg = torch.randn(bs, 1280, generator=g).cuda(), torch.randn(bs, 1280, generator=g).cuda()
    x_T = torch.randn(bs, 4, lat, lat, generator=g).cuda()
    kw = dict(height=a.size, width=a.size, num_inference_steps=a.steps, guidance_scale=4.0, latents=x_T, output_type="latent")
    if task == "inpainting":
        mask = torch.ones(a.size, a.size)
        mask[a.size // 4: 3 * a.size // 4, a.size // 3: 5 * a.size // 6] = 0.0
        kw.update(image=torch.randn(1, 4, lat, lat, generator=g).cuda(), mask_image=mask.numpy())
    sched = lambda: k22.DDPMSchedulerHIP.from_config(k22.SCHEDULER_CONFIG_2_2)  # noqa: E731
    decs = {}
    for whole in (False, True):
        decs[whole] = (pipeline22.KandinskyV22DecoderHIP(unet, None, sched(), whole_loop_graph=whole) if task == "text2img" else
                       pipeline22.KandinskyV22InpaintDecoderHIP(unet, None, None, sched(), whole_loop_graph=whole))

    def generation(whole):
        torch.manual_seed(17)
        return decs[whole](pos, neg, **kw)

    finals, times = {}, {False: [], True: []}
    for whole in (False, True):                       # untimed: plan, tile selection, capture
        launches = L.k22_debug_counter(b"loop_launches")
        finals[whole] = generation(whole).clone()
        torch.cuda.synchronize()
        assert (L.k22_debug_counter(b"loop_launches") - launches == 1) == whole, "the route did not take the path it names"
    for _ in range(a.reps):
        for whole in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = generation(whole)
            torch.cuda.synchronize()
            times[whole].append(time.perf_counter() - t0)
            assert torch.equal(out, finals[whole]), f"{task}: the generations of one route differ"
    diff = (finals[False] - finals[True]).abs().max().item()
    ulp = None
    if task == "text2img":
        assert diff == 0.0, "text2img: one-graph loop and stepwise loop differ"
    else:   # what the stepwise loop makes of a one-ulp change of its input: the scale on which "equal to rounding per step" is to be read
        torch.manual_seed(17)
        moved = decs[False](pos, neg, **dict(kw, latents=torch.nextafter(x_T, torch.full_like(x_T, float("inf")))))
        ulp = (moved - finals[False]).abs().max().item()
    rows = []
    for whole in (False, True):
        t = sorted(times[whole])
        med = statistics.median(t)
        rows.append(dict(task=task, bs=bs, whole_loop_graph=whole, median_ms=med * 1e3, min_ms=t[0] * 1e3, max_ms=t[-1] * 1e3,
                         spread=(t[-1] - t[0]) / med, steps_per_s=a.steps / med, n=len(t)))
    del unet, decs
    torch.cuda.empty_cache()
    return rows, diff, ulp


def _samplers(a, tdt, L):
    """--sampler dpm_sampler: the DPM-Solver++ loop against the DDPM loop at the same number of model calls, and the long DDPM generation"""
    cfg = k22.tiny_unet22_config() if a.tiny else k22.UNET_CONFIG_2_2
    arch = k22.make_arch22(cfg)
    unet = k22.UNet2DConditionHIP(arch, backend_dtype=tdt, use_graph=True)
    unet.load_state_dict(k22.init_unet22_state_dict(arch, seed=0))
    unet = unet.to("cuda").eval()
    unet.prepare(free_params=True)
    lat = a.size // 8
    g = torch.Generator().manual_seed(17)
    pos, neg = torch.randn(1, 1280, generator=g).cuda(), torch.randn(1, 1280, generator=g).cuda()
    x_T = torch.randn(1, 4, lat, lat, generator=g).cuda()
    dec = pipeline22.KandinskyV22DecoderHIP(unet, None, k22.DDPMSchedulerHIP.from_config(k22.SCHEDULER_CONFIG_2_2), whole_loop_graph=True)
    configs = [("dpm_sampler", a.calls), ("ddpm_sampler", a.calls), ("ddpm_sampler", a.long_steps)]
    calls = {c: len(dec._dpm_schedule(c[1])[0]) if c[0] == "dpm_sampler" else c[1] for c in configs}
    assert calls[configs[0]] == calls[configs[1]], f"the compared loops make {calls[configs[0]]} and {calls[configs[1]]} model calls: pick another --calls"

    def generation(sampler, steps):
        torch.manual_seed(17)
        return dec(pos, neg, height=a.size, width=a.size, num_inference_steps=steps, guidance_scale=4.0, latents=x_T, output_type="latent",
                   sampler=sampler)

    times, finals = {c: [] for c in configs}, {}
    for _ in range(a.reps):
        for c in configs:
            launches = L.k22_debug_counter(b"loop_launches")
            out = generation(*c)                      # untimed: plan / capture (the engine's one cached loop was another configuration's)
            torch.cuda.synchronize()
            assert L.k22_debug_counter(b"loop_launches") - launches == 1, "the generation did not run as one loop"
            finals.setdefault(c, out.clone())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = generation(*c)
            torch.cuda.synchronize()
            times[c].append(time.perf_counter() - t0)
            assert torch.equal(out, finals[c]) and torch.isfinite(out).all(), f"{c}: the generations of one configuration differ"
    lines = [f"{'tiny' if a.tiny else '1.25 B'} 2.2 UNet, text2img bs 1, {a.size}x{a.size}, {a.dtype}, whole_loop_graph=True; {a.reps} timed generations "
             f"per configuration, the configurations alternating in one process"]
    rows = []
    for c in configs:
        t = sorted(times[c])
        med = statistics.median(t)
        row = dict(sampler=c[0], num_inference_steps=c[1], model_calls=calls[c], median_ms=med * 1e3, min_ms=t[0] * 1e3, max_ms=t[-1] * 1e3,
                   spread=(t[-1] - t[0]) / med, ms_per_model_call=med * 1e3 / calls[c], n=len(t))
        rows.append(row)
        lines.append(f"{c[0]:13s} num_inference_steps={c[1]:3d}  {calls[c]:3d} model calls  median {row['median_ms']:8.2f} ms  min {row['min_ms']:8.2f}  "
                     f"max {row['max_ms']:8.2f}  spread {100 * row['spread']:5.2f} %  {row['ms_per_model_call']:7.3f} ms / model call")
    dpm, ddpm, long_ = rows
    ratio = dpm["ms_per_model_call"] / ddpm["ms_per_model_call"]
    within = abs(ratio - 1.0) <= max(ddpm["spread"], dpm["spread"])
    lines.append(f"ms per model call, dpm_sampler / ddpm_sampler at {dpm['model_calls']} calls: {ratio:.4f} "
                 f"({'within' if within else 'OUTSIDE'} the larger of the two spreads, {100 * max(ddpm['spread'], dpm['spread']):.2f} %)")
    lines.append(f"generation time, dpm_sampler {dpm['model_calls']} calls / ddpm_sampler {long_['model_calls']} steps: "
                 f"{dpm['median_ms']:.1f} ms / {long_['median_ms']:.1f} ms = {dpm['median_ms'] / long_['median_ms']:.3f}")
    lines.append(json.dumps(dict(size=a.size, dtype=a.dtype, tiny=a.tiny, per_call_ratio=ratio, per_call_ratio_within_spread=within,
                                 generation_ratio=dpm["median_ms"] / long_["median_ms"], results=rows)))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=768, help="image side in pixels (latent = size/8)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32", "f16x3", "f16x2"])
    ap.add_argument("--reps", type=int, default=5, help="timed generations per route (at least 5)")
    ap.add_argument("--tiny", action="store_true", help="1/3-width UNet (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--sampler", default="ddpm_sampler", choices=list(pipeline22.SAMPLERS),
                    help="ddpm_sampler: stepwise against one graph (above); dpm_sampler: the DPM-Solver++ loop against the DDPM loop, both as one graph")
    ap.add_argument("--calls", type=int, default=20, help="--sampler dpm_sampler: model calls of the two loops that are compared")
    ap.add_argument("--long-steps", type=int, default=50, help="--sampler dpm_sampler: steps of the long DDPM generation")
    a = ap.parse_args(argv)
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if not 1 <= a.steps <= pipeline22.MAX_LOOP_GRAPH_STEPS:
        ap.error(f"--steps must be 1 .. {pipeline22.MAX_LOOP_GRAPH_STEPS}: longer loops stay stepwise on both routes")
    if not torch.cuda.is_available():
        raise SystemExit("bench_decoder22_loop: needs the GPU (no CPU fallback)")
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32, "f16x3": k22.F16X3, "f16x2": k22.F16X2}[a.dtype]
    L = k22._lib.lib()
    if a.sampler == "dpm_sampler":
        if not (1 <= a.calls <= pipeline22.MAX_LOOP_GRAPH_STEPS and 1 <= a.long_steps <= pipeline22.MAX_LOOP_GRAPH_STEPS):
            ap.error(f"--calls and --long-steps must be 1 .. {pipeline22.MAX_LOOP_GRAPH_STEPS}")
        lines = _samplers(a, tdt, L)
        print("\n".join(lines))
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    lines = [f"{'tiny' if a.tiny else '1.25 B'} 2.2 UNet, {a.size}x{a.size}, {a.steps} steps, {a.dtype}; {a.reps} timed generations per route, "
             f"the routes alternating in one process"]
    results = []
    for task, bs in (("text2img", 1), ("inpainting", 2)):
        rows, diff, ulp = _case(task, bs, a, tdt, L)
        results += rows
        for r in rows:
            lines.append(f"{task:10s} bs {bs}  whole_loop_graph={str(r['whole_loop_graph']):5s}  median {r['median_ms']:8.2f} ms  min {r['min_ms']:8.2f}  "
                         f"max {r['max_ms']:8.2f}  spread {100 * r['spread']:5.2f} %  {r['steps_per_s']:7.2f} steps/s")
        step, whole = rows[0]["median_ms"], rows[1]["median_ms"]
        lines.append(f"{task:10s} one graph / stepwise = {whole / step:.4f} ({100 * (step - whole) / step:+.2f} % time saved); final latents of the two "
                     f"routes: max|d| {diff:.3e}" + (" (bit-equal)" if ulp is None else f" (keep_region against blend_noised, equal to rounding per step; the "
                                                    f"stepwise route against itself with x_T moved by one fp32 ulp: max|d| {ulp:.3e})"))
    lines.append(json.dumps(dict(size=a.size, steps=a.steps, dtype=a.dtype, tiny=a.tiny, results=results)))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
