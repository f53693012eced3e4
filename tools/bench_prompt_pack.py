#!/usr/bin/env python
"""Images per second of Kandinsky2_1HIP.generate_text2img_many for four prompts, one prompt per denoising call (pack=1) against all four in
ONE CFG batch of 8 (pack=4).

    python tools/bench_prompt_pack.py [--size 768 --steps 50 --dtype bf16 --reps 5 --out profiles/prompt_pack.txt]

Seeded weights (the 1.23 B UNet, the 1.0 B prior, MoVQ; config C2 by default: 768x768, batch_size 1, 50 steps, bf16), the seeded stand-in
conditioner, four different prompts, prior_steps "25".  Both configurations sample the four image embeddings in one prior call (prior_group=4
beside pack=1; pack=4 groups the prior itself), so what differs is the denoising loop - four loops at CFG batch 2 against one at CFG batch 8 -
and the MoVQ decode - four of one image against one of four.  Once with p_sampler (per-prompt dynamic threshold: k22_sampler_step_groups)
and once with the default ddim_sampler.

A generation is timed with a host clock between two device synchronisations.  Per sampler, after one untimed generation of each configuration
(plans, tile selection, graph capture), pack=1 and pack=4 ALTERNATE in one process, `--reps` timed generations each, so that a drift of the
box lands on both; the median, the extremes and the run-to-run spread (max - min) / median of each, images per second and the ratio
pack=4 / pack=1 go to stdout and to --out."""
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

PROMPTS = ["a red cat, 4k photo", "green tree on a hill", "blue bird on a wire", "an old house by the sea"]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=768, help="image side in pixels (latent = size/8)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--reps", type=int, default=5, help="timed generations per configuration")
    ap.add_argument("--tiny", action="store_true", help="1/3-width UNet and the 512x4 prior (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "prompt_pack.txt"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_prompt_pack: needs the GPU (no CPU fallback)")
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]

    cfg = copy.deepcopy(k22.CONFIG_2_1)
    if a.tiny:
        cfg["model_config"] = k22.tiny_model_config()
        cfg["prior"]["params"]["model"]["hparams"] = k22.tiny_prior_hparams()
    hp = cfg["prior"]["params"]["model"]["hparams"]
    g = torch.Generator().manual_seed(17)
    cfg["prior"]["clip_mean_std_path"] = (torch.randn(768, generator=g) * 0.1, torch.rand(768, generator=g) + 0.5)
    marc = k22.MoVQArch(k22.MOVQ_CONFIG_2_1["ddconfig"])
    cfg["image_enc_params"]["ckpt_path"] = dict(k22.init_movq_state_dict(marc, seed=0))
    arch = k22.make_arch(cfg["model_config"], inpainting=False)
    pipe = k22.Kandinsky2_1HIP(cfg, k22.init_unet_state_dict(arch, seed=0), k22.init_prior_state_dict(hp, seed=0), "cuda", task_type="text2img",
                               conditioner="seeded", backend_dtype=tdt)

    def generation(sampler, pack):
        torch.manual_seed(17)
        out = pipe.generate_text2img_many(PROMPTS, num_steps=a.steps, batch_size=1, guidance_scale=4, h=a.size, w=a.size, sampler=sampler,
                                          prior_cf_scale=4, prior_steps="25", output_type="tensor", prior_group=4, pack=pack)
        assert len(out) == len(PROMPTS) and all(tuple(o.shape) == (1, a.size, a.size, 3) for o in out)
        return out

    lines = [f"generate_text2img_many, {len(PROMPTS)} prompts, {'tiny' if a.tiny else '1.23 B'} UNet, {a.size}x{a.size}, batch_size 1, {a.steps} steps, "
             f"{a.dtype}, prior_steps 25 in one grouped prior call; pack=1 and pack=4 alternate, {a.reps} timed generations each"]
    rows = []
    for sampler in ("p_sampler", "ddim_sampler"):
        times = {1: [], 4: []}
        for pack in times:                               # untimed: plan / tile selection / capture of both shapes
            generation(sampler, pack)
            torch.cuda.synchronize()
        for _ in range(a.reps):
            for pack in times:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                generation(sampler, pack)
                torch.cuda.synchronize()
                times[pack].append(time.perf_counter() - t0)
        med = {}
        for pack, t in times.items():
            t = sorted(t)
            med[pack] = statistics.median(t)
            row = dict(sampler=sampler, pack=pack, median_ms=med[pack] * 1e3, min_ms=t[0] * 1e3, max_ms=t[-1] * 1e3, spread=(t[-1] - t[0]) / med[pack],
                       images_per_s=len(PROMPTS) / med[pack], n=len(t))
            rows.append(row)
            lines.append(f"{sampler:13s} pack={pack}  median {row['median_ms']:9.2f} ms  min {row['min_ms']:9.2f}  max {row['max_ms']:9.2f}  "
                         f"spread {100 * row['spread']:5.2f} %  {row['images_per_s']:6.3f} images/s")
        ratio = med[1] / med[4]
        spread = max(r["spread"] for r in rows[-2:])
        verdict = "faster than" if ratio > 1 + spread else ("slower than" if ratio < 1 - spread else "within the run-to-run spread of")
        rows.append(dict(sampler=sampler, ratio_pack4_over_pack1=ratio, larger_spread=spread))
        lines.append(f"{sampler:13s} images/s pack=4 / pack=1 = {ratio:.3f}  (larger spread of the two {100 * spread:.2f} %: pack=4 is {verdict} pack=1)")
    lines.append(json.dumps(dict(size=a.size, steps=a.steps, dtype=a.dtype, tiny=a.tiny, prompts=len(PROMPTS), results=rows)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
