#!/usr/bin/env python
"""Prior transformer forward time at bs=1 (CFG batch 2), full 1.02 B-parameter configuration, and whole generations of the prior:
"ddim10" as one captured graph (k22_prior_sample_loop) and stepwise, "25" on today's route and through the loop entry - median of 7
generations after a warm-up call, with min / max (the lines of profiles/prior_ddim.txt)."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kandinsky2_amd as k22
hp = k22.PRIOR_HPARAMS_2_1
m = k22.PriorDiffusionModelHIP(hp, backend_dtype=torch.bfloat16)
m.load_state_dict(k22.init_prior_state_dict(hp, seed=0))
m = m.to("cuda")
N = 2
x, t = torch.randn(N, 768, device="cuda"), torch.full((N,), 500.0, device="cuda")
te, tq = torch.randn(N, 768, device="cuda"), torch.randn(N, 77, 768, device="cuda")
mask = torch.ones(N, 77, dtype=torch.bool, device="cuda")
out = m.transformer(x, t, te, tq, mask)
torch.cuda.synchronize()
t0 = time.perf_counter()
n = 10
for _ in range(n):
    out = m.transformer(x, t, te, tq, mask)
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) / n * 1e3
wbytes = sum(v.numel() for k, v in m.state_dict().items() if k.startswith("model.transformer") and k.endswith("weight") and v.dim() == 2) * 2
print(f"prior forward bs=1 (2x81 tokens) bf16: {ms:.3f} ms  ({wbytes / ms / 1e6:.0f} GB/s of transformer weights, finite={bool(torch.isfinite(out).all())})")
print(m.tuning_report())
for it in range(2):   # the first call plans / tunes / captures the graph of the sampling batch shape
    t0 = time.perf_counter()
    s = m(te, tq, mask, torch.tensor([4.0], device="cuda"), timestep_respacing="25")
    torch.cuda.synchronize()
    print(f"prior 25-step sample ({'first call: plan + tile selection + graph capture' if it == 0 else 'steady state'}): {(time.perf_counter() - t0) * 1e3:.1f} ms")

# ---- whole generations: DDIM respacing and the loop entry ----------------------------------------------------------------------------------
from kandinsky2_amd import _lib  # noqa: E402
L = _lib.lib()
scales = torch.tensor([4.0], device="cuda")
for label, respacing, whole in (("ddim10 one graph (default)", "ddim10", None), ("ddim10 stepwise", "ddim10", False),
                                ("25 today's route (default)", "25", None), ("25 through the loop entry", "25", True)):
    m(te, tq, mask, scales, timestep_respacing=respacing, whole_loop_graph=whole)   # warm-up: capture / buffers
    torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        l0 = L.k22_debug_counter(b"loop_launches")
        t0 = time.perf_counter()
        s = m(te, tq, mask, scales, timestep_respacing=respacing, whole_loop_graph=whole)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        took_loop = L.k22_debug_counter(b"loop_launches") - l0 == 1
        assert took_loop == (whole is True or (whole is None and respacing.startswith("ddim"))), "the configuration did not take the path it names"
    ts.sort()
    med = ts[len(ts) // 2]
    print(f"prior bs=1 bf16 {label:28s}: median {med:7.2f} ms  min {ts[0]:7.2f}  max {ts[-1]:7.2f}  spread {(ts[-1] - ts[0]) / med * 100:4.1f} %  "
          f"(n={len(ts)}, finite={bool(torch.isfinite(s).all())})")
