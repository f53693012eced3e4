#!/usr/bin/env python
"""The MoVQ AttnBlock's two routes, "scores" ([T][T] scores in the workspace: GEMM, row softmax, GEMM per image) against "fused"
(one k22_movq_attention launch for all images), on the full-size 2.1 MoVQ with seeded weights.

    python tools/bench_movq_attention.py [--reps 5 --out profiles/movq_fused_attention.txt] [--quick]

Part 1, whole decodes / encodes.  Shapes: decoder 768^2 bs 1, 1024^2 bs 1, 1024^2 bs 4, 1536^2 bs 1; encoder 768^2 bs 1; types bf16 and fp16.
One module per route (each keeps its plan and workspace); after one untimed call per route the two routes ALTERNATE, `--reps` (>= 5) timed
calls each, in one process, so that a drift of the box lands on both.  A call is timed with a host clock between two device synchronisations.
Per route: median, extremes, spread (max - min) / median, and the plan's workspace bytes.

Part 2, the launches alone, in a pass of its own: at the AttnBlock's shape (B, T, C = 512) of each decoder case, HIP events around ONE
k22_movq_attention launch against HIP events around the launches it replaces (per image: the T x T x C score GEMM, then one row softmax over
all images, then per image the T x C x T GEMM with the V bias), median of `--reps`.  Four such blocks run per decode, three per encode.

Part 3, distance to the fp32 image: at 768^2 the image of each route (bf16, fp16) against the FP32 engine's scores-route image of the same
latent: max-abs of the float output and the share of uint8 bytes that differ.

What is not measured: image quality (seeded weights), anything above 1536^2, power or clocks (the box state is whatever the run found)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kandinsky2_amd as k22  # noqa: E402
from kandinsky2_amd import _lib  # noqa: E402

DECODER_CASES = ((768, 1), (1024, 1), (1024, 4), (1536, 1))
ENCODER_CASES = ((768, 1),)
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
_SD = {}


def _module(kind, tdt, attention):
    arch = k22.MoVQArch(k22.MOVQ_CONFIG_2_1["ddconfig"])
    if kind not in _SD:
        _SD[kind] = k22.init_movq_state_dict(arch, seed=0) if kind == "decoder" else k22.init_movq_encoder_state_dict(arch, seed=0)
    m = (k22.MoVQDecoderHIP if kind == "decoder" else k22.MoVQEncoderHIP)(backend_dtype=tdt, attention=attention)
    m.load_state_dict(_SD[kind], strict=True)
    return m.to("cuda")


def _stats(t):
    t = sorted(t)
    med = statistics.median(t)
    return dict(median_ms=med * 1e3, min_ms=t[0] * 1e3, max_ms=t[-1] * 1e3, spread=(t[-1] - t[0]) / med, n=len(t))


def _whole(kind, size, bs, dtype, reps, L):
    g = torch.Generator().manual_seed(23)
    x = (torch.randn(bs, 4, size // 8, size // 8, generator=g) if kind == "decoder" else torch.randn(bs, 3, size, size, generator=g).clamp(-2, 2) * 0.5).cuda()
    mods = {r: _module(kind, TDT[dtype], r) for r in ("scores", "fused")}
    run = (lambda m: m.decode(x)) if kind == "decoder" else (lambda m: m.encode(x))
    outs, times, ws = {}, {"scores": [], "fused": []}, {}
    for r, m in mods.items():                          # untimed: pack, plan, first launches
        n0 = L.k22_debug_counter(b"movq_fused_attn_launches")
        outs[r] = run(m).clone()
        torch.cuda.synchronize()
        assert (L.k22_debug_counter(b"movq_fused_attn_launches") > n0) == (r == "fused"), "the route did not take the path it names"
        ws[r] = m._engines["movq"].ws.numel() - 256
    for _ in range(reps):
        for r, m in mods.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run(m)
            torch.cuda.synchronize()
            times[r].append(time.perf_counter() - t0)
            assert torch.equal(out, outs[r]), f"{kind} {size} {dtype}: the calls of one route differ"
    rows = [dict(kind=kind, size=size, bs=bs, dtype=dtype, route=r, workspace_bytes=ws[r], **_stats(times[r])) for r in mods]
    diff = (outs["scores"] - outs["fused"]).abs().max().item() / outs["scores"].abs().max().item()
    del mods
    torch.cuda.empty_cache()
    return rows, diff


def _event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def _launches(size, bs, dtype, reps, L):
    """HIP events around the fused launch and around the launches it replaces, at the AttnBlock's shape of a decoder case"""
    B, T, Cc, code, tdt = bs, (size // 8) ** 2, 512, _lib.dtype_code(TDT[dtype]), TDT[dtype]
    g = torch.Generator().manual_seed(29)
    q, k = (1.5 * torch.randn(B, T, Cc, generator=g)).to(tdt).cuda(), (1.5 * torch.randn(B, T, Cc, generator=g)).to(tdt).cuda()
    vt = (0.3 + 1.7 * torch.randn(B, Cc, T, generator=g)).to(tdt).cuda()
    bias = torch.randn(Cc, generator=g).cuda()
    out, sc = torch.empty_like(q), torch.empty(B, T, T, dtype=tdt, device="cuda")
    partial = torch.empty(T * T + 64, dtype=torch.float32, device="cuda")
    st = _lib.current_stream()

    def fused():
        _lib.check(L.k22_movq_attention(q.data_ptr(), k.data_ptr(), vt.data_ptr(), bias.data_ptr(), out.data_ptr(), B, T, Cc, code, st))

    def replaced():
        for b in range(B):
            _lib.check(L.k22_gemm(q[b].data_ptr(), None, k[b].data_ptr(), None, None, sc[b].data_ptr(), partial.data_ptr(), T, T, T, Cc, 0, Cc, 0, T, T,
                                  0, 0, 1, 0, 0, code, st))
        _lib.check(L.k22_softmax_rows(sc.data_ptr(), B * T, T, Cc ** -0.5, code, st))
        for b in range(B):
            _lib.check(L.k22_gemm(sc[b].data_ptr(), None, vt[b].data_ptr(), bias.data_ptr(), None, out[b].data_ptr(), partial.data_ptr(), T, Cc, Cc, T, 0,
                                  T, 0, Cc, Cc, 0, 0, 1, 0, 0, code, st))

    f, r = _event_ms(fused, reps), _event_ms(replaced, reps)
    return dict(size=size, bs=bs, dtype=dtype, B=B, T=T, C=Cc, fused_ms=f[0], fused_min_ms=f[1], fused_max_ms=f[2], replaced_ms=r[0], replaced_min_ms=r[1],
                replaced_max_ms=r[2], replaced_launches=1 + 2 * B)


def _distance(size, L):
    """each route's image against the fp32 engine's scores-route image of the same latent"""
    z = torch.randn(1, 4, size // 8, size // 8, generator=torch.Generator().manual_seed(23)).cuda()
    m = _module("decoder", torch.float32, "scores")
    ref, ref_u8 = m.decode(z, return_uint8=True)
    ref, ref_u8 = ref.clone(), ref_u8.clone()
    del m
    rows = []
    for dtype in ("bf16", "fp16"):
        for route in ("scores", "fused"):
            m = _module("decoder", TDT[dtype], route)
            out, u8 = m.decode(z, return_uint8=True)
            rows.append(dict(size=size, dtype=dtype, route=route, max_abs=(out - ref).abs().max().item(), scale=ref.abs().max().item(),
                             u8_differ=(u8 != ref_u8).float().mean().item(), u8_max=(u8.int() - ref_u8.int()).abs().max().item()))
            del m
    torch.cuda.empty_cache()
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5, help="timed calls per route (at least 5)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--quick", action="store_true", help="256^2 shapes only (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args(argv)
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("bench_movq_attention: needs the GPU (no CPU fallback)")
    L = _lib.lib()
    dec_cases, enc_cases, dist_size = (((256, 1), (256, 2)), ((256, 1),), 256) if a.quick else (DECODER_CASES, ENCODER_CASES, 768)
    lines = [f"full-size 2.1 MoVQ, seeded weights; {a.reps} timed calls per route, the routes alternating in one process; {torch.cuda.get_device_name(0)}"]
    results = {"whole": [], "launches": [], "distance": []}
    lines.append("-- whole decode / encode: median [min .. max] ms, spread, workspace of the plan")
    for kind, cases in (("decoder", dec_cases), ("encoder", enc_cases)):
        for size, bs in cases:
            for dtype in ("bf16", "fp16"):
                rows, diff = _whole(kind, size, bs, dtype, a.reps, L)
                results["whole"] += rows
                for r in rows:
                    lines.append(f"{kind} {size}^2 bs {bs} {dtype:4s} {r['route']:6s}  {r['median_ms']:9.3f} [{r['min_ms']:9.3f} .. {r['max_ms']:9.3f}] ms  "
                                 f"spread {100 * r['spread']:5.2f} %  workspace {r['workspace_bytes'] / 2 ** 20:10.1f} MiB")
                s, f = rows
                noise = max(s["spread"], f["spread"])
                ratio = f["median_ms"] / s["median_ms"]
                verdict = "within the spread" if abs(ratio - 1) <= noise else ("fused FASTER" if ratio < 1 else "fused SLOWER")
                lines.append(f"    fused / scores = {ratio:.4f} ({verdict}); workspace saved {(s['workspace_bytes'] - f['workspace_bytes']) / 2 ** 20:.1f} MiB; "
                             f"outputs of the two routes: max|d| {diff:.3e} of scale")
    lines.append("-- the launches alone (HIP events, a pass of its own): one fused launch against the 1 + 2 B launches it replaces, C = 512")
    for size, bs in dec_cases:
        for dtype in ("bf16", "fp16"):
            r = _launches(size, bs, dtype, a.reps, L)
            results["launches"].append(r)
            lines.append(f"B {r['B']} T {r['T']:6d} {dtype:4s}  fused {r['fused_ms']:9.3f} [{r['fused_min_ms']:9.3f} .. {r['fused_max_ms']:9.3f}] ms   replaced "
                         f"({r['replaced_launches']} launches) {r['replaced_ms']:9.3f} [{r['replaced_min_ms']:9.3f} .. {r['replaced_max_ms']:9.3f}] ms   "
                         f"fused / replaced = {r['fused_ms'] / r['replaced_ms']:.3f}")
    lines.append(f"-- distance to the fp32 engine's scores-route image, {dist_size}^2 bs 1, same latent")
    for r in _distance(dist_size, L):
        results["distance"].append(r)
        lines.append(f"{r['dtype']:4s} {r['route']:6s}  max|d| {r['max_abs']:.4e} ({r['max_abs'] / r['scale']:.3e} of scale {r['scale']:.3f})   uint8 bytes that differ "
                     f"{100 * r['u8_differ']:.3f} %, largest difference {r['u8_max']} levels")
    lines.append(json.dumps(results))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
