#!/usr/bin/env python
"""Denoise-loop time of the three samplers of Kandinsky2_1HIP.generate_img, stepwise against the one-graph loop.

    python tools/bench_sampler_loop.py [--size 768 --bs 1 --steps 50 --dtype bf16 --reps 3 --rounds 2]

Runs generate_img(..., decode=False) on seeded weights (the 1.23 B UNet; config C2 by default: 768x768, bs 1, 50 steps, bf16) for

    ddim_sampler, plms_sampler   with whole_loop_graph False (host-driven: one k22_unet_forward + one step kernel per step) and True
                                 (k22_unet_ddim_loop: the whole loop as one hipGraph replay)
    p_sampler                    with whole_loop_graph True (k22_unet_sample_loop), the yardstick of the headline figures

Each generation is timed with a host clock between two device synchronisations, after one untimed generation per configuration
(plans, tile selection, graph capture).  The configurations are visited `--rounds` times in turn, `--reps` timed generations per visit,
so that a drift of the box lands on all of them; per configuration the median, the extremes and the spread (max - min) / median of all
its timed generations are printed, then one JSON line with everything.  The prior does not run in generate_img: it is built at its tiny
size.  Text embeddings are computed once, outside the timed region."""
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

CONFIGS = [("p_sampler", True), ("ddim_sampler", False), ("ddim_sampler", True), ("plms_sampler", False), ("plms_sampler", True)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=768, help="image side in pixels (latent = size/8)")
    ap.add_argument("--bs", type=int, default=1, help="images per generation (CFG batch = 2*bs)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32", "f16x3", "f16x2"])
    ap.add_argument("--reps", type=int, default=3, help="timed generations per configuration and round")
    ap.add_argument("--rounds", type=int, default=2, help="visits of every configuration (reps * rounds >= 5 timed generations each)")
    ap.add_argument("--tiny", action="store_true", help="1/3-width UNet (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args(argv)
    if a.reps * a.rounds < 5:
        ap.error("reps * rounds must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampler_loop: needs the GPU (no CPU fallback)")
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32, "f16x3": k22.F16X3, "f16x2": k22.F16X2}[a.dtype]

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
                               conditioner="seeded", backend_dtype=tdt)

    prompt, lat = "a red cat, 4k photo", a.size // 8
    x_T = torch.randn(2 * a.bs, 4, lat, lat, generator=g).cuda()
    image_emb = torch.randn(2 * a.bs, 768, generator=g).cuda()
    text_embs = pipe.encode_text(prompt, a.bs)
    L = k22._lib.lib()

    diffusions = {s: pipe._diffusion(s, a.steps)[1] for s, _ in CONFIGS}

    def generation(sampler, whole):
        pipe.whole_loop_graph = whole
        torch.manual_seed(17)                         # p_sampler draws its per-step noise: every generation of a configuration the same one
        return pipe.generate_img(prompt, image_emb, batch_size=a.bs, diffusion=diffusions[sampler], guidance_scale=4, noise=x_T, h=a.size, w=a.size,
                                 sampler=sampler, num_steps=a.steps, text_embs=text_embs, decode=False)

    times = {c: [] for c in CONFIGS}
    finals = {}
    for rnd in range(a.rounds):
        for c in CONFIGS:
            launches = L.k22_debug_counter(b"loop_launches")
            out = generation(*c)                      # untimed: plan / capture (a change of loop kind re-captures)
            torch.cuda.synchronize()
            assert (L.k22_debug_counter(b"loop_launches") - launches == 1) == c[1], "the configuration did not take the path it names"
            finals.setdefault(c, out.clone())
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = generation(*c)
                torch.cuda.synchronize()
                times[c].append(time.perf_counter() - t0)
            assert torch.equal(out, finals[c]), f"{c}: the generations of one configuration differ"
    for s in ("ddim_sampler", "plms_sampler"):
        assert torch.equal(finals[(s, False)], finals[(s, True)]), f"{s}: one-graph loop and stepwise loop differ"

    n_calls = {"p_sampler": a.steps, "ddim_sampler": a.steps, "plms_sampler": a.steps + 1}
    print(f"{'tiny' if a.tiny else '1.23 B'} UNet, {a.size}x{a.size}, bs {a.bs}, {a.steps} steps, {a.dtype}; "
          f"{a.reps * a.rounds} timed generations per configuration in {a.rounds} rounds")
    rows = []
    for c in CONFIGS:
        t = sorted(times[c])
        med = statistics.median(t)
        row = dict(sampler=c[0], whole_loop_graph=c[1], median_ms=med * 1e3, min_ms=t[0] * 1e3, max_ms=t[-1] * 1e3, spread=(t[-1] - t[0]) / med,
                   model_calls=n_calls[c[0]], model_calls_per_s=n_calls[c[0]] / med, n=len(t))
        rows.append(row)
        print(f"{c[0]:13s} whole_loop_graph={str(c[1]):5s}  median {row['median_ms']:8.2f} ms  min {row['min_ms']:8.2f}  max {row['max_ms']:8.2f}  "
              f"spread {100 * row['spread']:5.2f} %  {row['model_calls_per_s']:7.2f} UNet calls/s")
    print(json.dumps(dict(size=a.size, bs=a.bs, steps=a.steps, dtype=a.dtype, tiny=a.tiny, results=rows)))


if __name__ == "__main__":
    main()
