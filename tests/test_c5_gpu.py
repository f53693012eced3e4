"""BASELINE config C5 at its real size: Kandinsky 2.2 ControlNet-depth decoder, 768x768, bs 2 -> CFG batch [4, 8, 96, 96] plus a
hint [4, 3, 768, 768], on the full-width UNET_CONFIG_2_2 (1.25 B parameters), against tests/golden/c5_forward.pt / c5_loop.pt
(oracle/make_golden_unet22.py: oracle/unet22_ref.py on seeded weights and inputs).  Oracle unpinned (diffusers absent): these tests
check that the engine computes what the repository's restatement of diffusers says, at the shapes only C5 runs - the hint stack
(eight direct fp32 convolutions, three with stride 2, over 768x768 images), the 8-channel stem, the 2.2 conditioning head at B = 4.

Also the unit-parity entry of the direct convolution (k22_conv3x3_direct) at its edges, against float64 F.conv2d on the same fp32
operands, and the hint stack stage by stage at C5.
"""
import time

import pytest
import torch
import torch.nn.functional as F

import kandinsky2_amd as k22
from kandinsky2_amd import _lib
from oracle import make_golden_unet22 as mg

pytestmark = pytest.mark.gpu

HINT_STRIDES = (1, 1, 2, 1, 2, 1, 2, 1)


def _load(golden_dir, name):
    import os
    return torch.load(os.path.join(golden_dir, name + ".pt"), weights_only=False)


def _compact_err(out, c):
    """max-abs distance on the stored sub-grid, row band and column band of a compact fixture"""
    s = c["stride"]
    e = (out[..., ::s, ::s] - c["sub"]).abs().max().item()
    e = max(e, (out[..., c["r0"]: c["r0"] + c["rows"].shape[-2], :] - c["rows"]).abs().max().item())
    return max(e, (out[..., :, c["c0"]: c["c0"] + c["cols"].shape[-1]] - c["cols"]).abs().max().item())


# ---- k22_conv3x3_direct: the unit-parity entry of the hint stack's kernel ---------------------------------------------------------

def _conv_direct(x, w, b, stride, act):
    """k22_conv3x3_direct into a buffer pre-filled with NaN (an output the kernel does not write stays NaN) followed by a guard region
    that must come back untouched."""
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    n, guard = B * Cout * Ho * Wo, 4096
    buf = torch.full((n + guard,), float("nan"), device="cuda")
    buf[n:] = 1234.5
    _lib.check(_lib.lib().k22_conv3x3_direct(x.data_ptr(), w.data_ptr(), b.data_ptr(), buf.data_ptr(), B, Cin, Cout, H, W, stride, act,
                                             _lib.current_stream()))
    assert bool((buf[n:] == 1234.5).all()), "k22_conv3x3_direct wrote past its output"
    return buf[:n].view(B, Cout, Ho, Wo)


def _ref64(x, w, b, stride, act):
    y = F.conv2d(x.cpu().double(), w.cpu().double(), b.cpu().double(), stride=stride, padding=1)
    return F.silu(y) if act else y


DIRECT_CASES = [
    # B, Cin, Cout, Hin, Win, stride, act: odd sizes with stride 2, Ho*Wo not a multiple of 256, Cout below / not a multiple of OCB = 8
    (1, 3, 16, 7, 9, 2, 1), (3, 1, 1, 1, 1, 2, 0), (1, 1, 4, 33, 17, 2, 1), (3, 3, 9, 33, 17, 1, 0), (1, 5, 9, 7, 9, 1, 1),
    (3, 16, 4, 15, 31, 2, 0), (1, 3, 1, 17, 16, 1, 1), (2, 32, 13, 25, 19, 2, 1), (1, 1, 1, 1, 1, 1, 0), (1, 3, 16, 2, 2, 2, 1),
    (3, 7, 24, 19, 23, 1, 0), (3, 1, 9, 40, 33, 2, 1), (2, 96, 4, 24, 40, 1, 0),
]


@pytest.mark.parametrize("B,Cin,Cout,H,W,stride,act", DIRECT_CASES)
def test_conv3x3_direct_edges(B, Cin, Cout, H, W, stride, act):
    g = torch.Generator().manual_seed(B * 1000 + Cin * 100 + Cout + H + W)
    x = torch.rand(B, Cin, H, W, generator=g) * 2 - 0.5
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    y = _conv_direct(x.cuda(), w.cuda(), b.cuda(), stride, act).cpu().double()
    ref = _ref64(x, w, b, stride, act)
    assert y.shape == ref.shape
    scale = ref.abs().max().item()
    err = (y - ref).abs().max().item()
    assert torch.isfinite(y).all() and err <= 1e-5 * scale, (err, scale)


def test_conv3x3_direct_rejects_bad_arguments():
    L = _lib.lib()
    x, w, b, y = (torch.zeros(n, device="cuda") for n in (3 * 64, 8 * 3 * 9, 8, 8 * 64))
    s = _lib.current_stream()
    args = (x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr())
    for stride in (0, 3):
        assert L.k22_conv3x3_direct(*args, 1, 3, 8, 8, 8, stride, 0, s) == -1          # K22_EINVAL
    for k in range(4):
        a = list(args)
        a[k] = None
        assert L.k22_conv3x3_direct(*a, 1, 3, 8, 8, 8, 1, 0, s) == -1
    assert L.k22_conv3x3_direct(*args, 1, 3, 8, 8, 8, 1, 2, s) == -1                  # GELU: not an activation of the hint stack
    assert L.k22_conv3x3_direct(*args, 0, 3, 8, 8, 8, 1, 0, s) == -1
    torch.cuda.synchronize()
    assert L.k22_conv3x3_direct(*args, 1, 3, 8, 8, 8, 1, 0, s) == 0


def test_c5_hint_stack_stage_by_stage(golden_dir):
    """The eight hint convolutions at C5 (B = 4, 768x768 -> 96x96, 3 -> 16 -> 16 -> 32/2 -> 32 -> 96/2 -> 96 -> 256/2 -> 4) with the
    fixture's weights, through k22_conv3x3_direct: every stage within 1e-5 of its scale of float64 F.conv2d on the stage's own fp32
    input, the result within 1e-5 of scale of the fixture's hint latent."""
    fx = _load(golden_dir, "c5_forward")
    _, _, sd = mg.c5_weights()
    inp = mg.c5_inputs(fx["seed"])
    x = torch.cat([inp["hint"], inp["hint"]], 0).cuda()
    t0 = time.perf_counter()
    for k, s in enumerate(HINT_STRIDES):
        w = sd[f"add_embedding.input_hint_block.{2 * k}.weight"].contiguous()
        b = sd[f"add_embedding.input_hint_block.{2 * k}.bias"].contiguous()
        act = 0 if k == 7 else 1
        y = _conv_direct(x, w.cuda(), b.cuda(), s, act)
        ref = _ref64(x, w, b, s, act)
        scale = ref.abs().max().item()
        err = (y.cpu().double() - ref).abs().max().item()
        print(f"c5 hint stage {k} {tuple(x.shape)} -> {tuple(y.shape)} stride {s}: max|d| {err:.3e} = {err / scale:.3e} of scale {scale:.3f}")
        assert err <= 1e-5 * scale, k
        x = y
    want = torch.cat([fx["hint_latent"], fx["hint_latent"]], 0)
    scale = want.abs().max().item()
    err = (x.cpu() - want).abs().max().item()
    print(f"c5 hint latent vs fixture: max|d| {err:.3e} = {err / scale:.3e} of scale {scale:.4f} ({time.perf_counter() - t0:.1f} s)")
    assert x.shape == (4, 4, 96, 96) and err <= 1e-5 * scale


# ---- the UNet and the decoder loop at C5 ----------------------------------------------------------------------------------------

# Final latent of the 5-step loop: (max-abs, rms) bounds, each engine's MI355X measurement next to it.
# SCHEDULER_CONFIG_2_2 does not clip x0, and on random weights with guidance 4 the latent grows to |x| ~ 81 by the last step (the 2.1
# p_sampler's latents are thresholded to O(1), which is what the absolute 1e-3 / 1e-4 / 5e-4 gates of C2 / C3 are stated on).  The first
# step multiplies the guided eps error (up to 2 * 4 - 1 = 7x the raw one) by sqrt(1 / abar_800 - 1) = 8.4 in x0, and nothing clips it:
# every engine's final distance is ~30-45x
# its first-forward distance (measured: fp32 38x, f16x3 43x, f16x2 39x, fp16 36x, bf16 28x), so the loop adds no engine-specific error
# and its bounds follow the forward's.  fp32: the 1e-3 gate.  f16x3: 1e-4 lies below the exact-fp32 engine's own distance (3.5e-4) - the
# floor of fp32 rounding in engine and oracle amplified by the schedule, at which f16x3 sits (2.7e-4) - so its bound is 2x its
# measurement, as for f16x2 (whose first forward is 1.7e-4 of scale, inside its 3e-4 C3 bound), bf16 and fp16.
LOOP_BOUNDS = {
    torch.float32: (1e-3, 1.4e-4),          # measured 3.48e-4 / 6.79e-5 rms
    "f16x3": (5.4e-4, 1.0e-4),              # measured 2.71e-4 / 5.11e-5
    "f16x2": (3.6e-2, 7.1e-3),              # measured 1.81e-2 / 3.55e-3
    torch.bfloat16: (1.65, 0.37),           # measured 8.27e-1 / 1.86e-1
    torch.float16: (0.23, 0.049),           # measured 1.15e-1 / 2.46e-2
}
_FINAL = {}


def _model(backend, use_graph=True):
    _, arch, sd = mg.c5_weights()
    m = k22.UNet2DConditionHIP(arch, backend_dtype=backend, use_graph=use_graph)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    m.prepare(free_params=True)
    return m


def _loop(m, inp):
    dec = k22.pipeline22.KandinskyV22DecoderHIP(m, None, scheduler=k22.DDPMSchedulerHIP.from_config(k22.SCHEDULER_CONFIG_2_2))
    H = 8 * mg.LAT
    return dec(inp["pos"].cuda(), inp["neg"].cuda(), height=H, width=H, num_inference_steps=mg.STEPS, guidance_scale=mg.GUIDANCE,
               hint=inp["hint"].cuda(), latents=inp["lat"].cuda(), noise_seq=inp["noise"].cuda(), output_type="latent").cpu()


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


@pytest.mark.parametrize("backend,tol_fwd", [(torch.float32, 2e-4), ("f16x3", 2e-5), ("f16x2", 3e-4), (torch.bfloat16, 2.5e-2), (torch.float16, 3.2e-3)])
def test_c5_forward_and_decoder_loop(golden_dir, backend, tol_fwd):
    """One forward of the CFG batch (per-element timesteps [980, 500, 20, 0], [neg | pos] embeds, [hint | hint]) within tol_fwd of the
    output scale, then the 5-step KandinskyV22ControlnetPipeline loop (DDPM, SCHEDULER_CONFIG_2_2, guidance 4, injected noise): final
    latent within LOOP_BOUNDS (max-abs and rms).
    First-forward tolerances: fp32 / f16x3 / f16x2 as at C3, bf16 / fp16 as the tiny 2.2 test."""
    fx, fl = _load(golden_dir, "c5_forward"), _load(golden_dir, "c5_loop")
    assert (fx["seed"], fl["steps"], fl["guidance"]) == (mg.SEED, mg.STEPS, mg.GUIDANCE)
    inp = mg.c5_inputs(fx["seed"])
    m, t_build = _timed(lambda: _model(backend))
    ack = {"image_embeds": torch.cat([inp["neg"], inp["pos"]], 0).cuda(), "hint": torch.cat([inp["hint"], inp["hint"]], 0).cuda()}
    x, t = inp["x"].cuda(), fx["t"].cuda()
    out, t_first = _timed(lambda: m(sample=x, timestep=t, encoder_hidden_states=None, added_cond_kwargs=ack, return_dict=False)[0].cpu())
    scale = fx["absmax"]
    err = _compact_err(out, fx["forward_compact"])
    print(f"c5 {backend}: first forward max|d| {err:.3e} = {err / scale:.3e} of scale {scale:.3f} (oracle unpinned); "
          f"engine build {t_build:.1f} s, first forward (plan + capture) {t_first:.2f} s")
    assert out.shape == (4, 8, 96, 96) and torch.isfinite(out).all() and err <= tol_fwd * scale

    if backend == torch.bfloat16:
        # price of the content check of the conditioning cache on the bare-module path (diffusers-style caller, same tensors every step)
        n = 10
        _, t_check = _timed(lambda: [m(x, t, added_cond_kwargs=ack, return_dict=False) for _ in range(n)])
        with m.fixed_conditioning():
            m(x, t, added_cond_kwargs=ack, return_dict=False)
            _, t_fixed = _timed(lambda: [m(x, t, added_cond_kwargs=ack, return_dict=False) for _ in range(n)])

        def recompute():
            for _ in range(n):
                m.del_cache()
                m(x, t, added_cond_kwargs=ack, return_dict=False)
        _, t_recompute = _timed(recompute)
        print(f"c5 bf16 forward per step: {1e3 * t_fixed / n:.2f} ms with fixed_conditioning (no check), {1e3 * t_check / n:.2f} ms bare "
              f"(content check), {1e3 * t_recompute / n:.2f} ms recomputing head + hint stack every call")

    got, t_loop = _timed(lambda: _loop(m, inp))
    _FINAL[(backend, True)] = got
    d = got - fl["final"]
    ma, rms = d.abs().max().item(), d.pow(2).mean().sqrt().item()
    print(f"c5 {backend}: {mg.STEPS}-step loop final latent max|d| {ma:.3e} rms {rms:.3e} (scale {fl['final'].abs().max().item():.2f}, "
          f"oracle unpinned); loop {t_loop:.2f} s")
    b_ma, b_rms = LOOP_BOUNDS[backend]
    assert torch.isfinite(got).all() and ma <= b_ma and rms <= b_rms


def test_c5_bf16_loop_graph_equals_eager(golden_dir):
    """The bf16 decoder loop at C5 gives the same bits with the engine's hipGraph replay and with eager launches."""
    fx = _load(golden_dir, "c5_forward")
    inp = mg.c5_inputs(fx["seed"])
    outs = {}
    for use_graph in (True, False):
        if (torch.bfloat16, use_graph) in _FINAL:
            outs[use_graph] = _FINAL[(torch.bfloat16, use_graph)]
            continue
        m = _model(torch.bfloat16, use_graph=use_graph)
        outs[use_graph], el = _timed(lambda: _loop(m, inp))
        print(f"c5 bf16 loop use_graph={use_graph}: {el:.2f} s")
        del m
        torch.cuda.empty_cache()
    d = (outs[True] - outs[False]).abs().max().item()
    print(f"c5 bf16 loop graph vs eager: max|d| {d:.3e}")
    assert torch.equal(outs[True], outs[False])
