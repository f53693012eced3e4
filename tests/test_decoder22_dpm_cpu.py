"""The DPM-Solver++ sampler on the Kandinsky 2.2 decoders, the part that needs no GPU: the schedule and keep-coefficient helpers
(sampling.dpmpp_schedule, sampling.dpmpp_keep_coef), the img2img grids, the float64 model of the clamped step with its bound and mutants
(tests/decoder22_dpm_ref.py), the decoders' host logic on a stub UNet, and the new C entries' declarations and null-argument refusals.

Every test reaches for a symbol or keyword the sampler adds, so each fails without it."""
import contextlib
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import decoder22_dpm_ref as D
import dpmpp_ref as R
import kandinsky2_amd as k22
from kandinsky2_amd import _lib, pipeline22, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AC22 = k22.DDPMSchedulerHIP.from_config(k22.SCHEDULER_CONFIG_2_2).alphas_cumprod


# ---- 1. the schedule ---------------------------------------------------------------------------------------------------------------------
def test_the_2_2_schedule_is_the_2_1_array():
    assert np.array_equal(AC22, R.schedule_2_1()) and AC22.dtype == np.float64


@pytest.mark.parametrize("S,n", [(6, 6), (20, 20), (50, 48)])
@pytest.mark.parametrize("kw", [{}, dict(solver_order=1), dict(lower_order_final=False), dict(discretize="uniform"), dict(init_step=500)])
def test_dpmpp_schedule_equals_make_dpm_schedule_bit_for_bit(S, n, kw):
    sm = k22.DPMSolverSamplerHIP(None, k22.create_gaussian_diffusion(**k22.DIFFUSION_CONFIG_2_1), 4.0)
    sm.make_dpm_schedule(S, **kw)
    ts, table, orders = sampling.dpmpp_schedule(AC22, S, **kw)
    if not kw:
        assert len(ts) == n
    assert ts.dtype == np.int64 and table.dtype == np.float64 and tuple(table.shape) == (len(ts), 5)
    assert np.array_equal(ts, sm.timesteps) and np.array_equal(table.view(np.uint64), sm.dpm_table.view(np.uint64))
    assert np.array_equal(orders, sm.orders)
    # the last step targets ac[0]: c_x = sigma(ac[0]) / sigma_s
    assert table[-1, 2] == np.sqrt(1.0 - AC22[0]) / np.sqrt(1.0 - AC22[ts[-1]])


def test_dpmpp_keep_coef_rows_against_float64():
    ts, _, _ = sampling.dpmpp_schedule(AC22, 20)
    coef = sampling.dpmpp_keep_coef(AC22, ts)
    assert coef.dtype == np.float32 and coef.shape == (20, 2) and coef[-1].tolist() == [1.0, 0.0]
    for k in range(19):
        a = np.float64(AC22[ts[k + 1]])            # the point step k arrives at
        want = np.array([np.sqrt(a), np.sqrt(1.0 - a)], dtype=np.float64).astype(np.float32)
        assert np.array_equal(coef[k].view(np.uint32), want.view(np.uint32)), k
        assert abs(float(coef[k, 0]) ** 2 + float(coef[k, 1]) ** 2 - 1.0) < 1e-6
    one = sampling.dpmpp_keep_coef(AC22, [8])
    assert one.tolist() == [[1.0, 0.0]]
    assert "ac[0]" in sampling.dpmpp_keep_coef.__doc__


@pytest.mark.parametrize("steps,strength,n,first,grid", [(20, 0.5, 12, 419, None), (10, 0.5, 5, 246, None), (6, 0.5, 3, 246, [246, 61, 8])])
def test_img2img_grids(steps, strength, n, first, grid):
    dec = pipeline22.KandinskyV22Img2ImgDecoderHIP(None, None, None, sampler="dpm_sampler")
    init_step = dec.get_timesteps(steps, strength, device="cpu")[0]
    ts, table, orders = dec._dpm_schedule(steps, init_step=init_step)
    assert len(ts) == n and int(ts[0]) == first and all(int(t) <= init_step for t in ts)
    assert orders[0] == 1 and orders[-1] == 1 and all(o == 2 for o in orders[1:-1])
    if grid is not None:
        assert [int(t) for t in ts] == grid
    whole = [int(t) for t in sampling.dpmpp_schedule(AC22, steps)[0]]
    assert [int(t) for t in ts] == [t for t in whole if t <= init_step]          # the whole grid's points at or below init_step


# ---- 2. the clamped step: bound and mutants --------------------------------------------------------------------------------------------------
def _rows():
    ts = sampling.dpmpp_grid(AC22, 20, "logsnr")
    table, _ = sampling.dpmpp_table(*R.integer_grid(AC22, ts), lower_order_final=False)
    return [(table[0], 1), (table[10], 2), (table[19], 2)]


@pytest.mark.parametrize("use_cfg", [0, 1])
def test_fp32_evaluation_of_the_clamped_step_lies_inside_the_bound_and_the_mutants_outside(use_cfg):
    d = R.step_inputs(4, 257, seed=4 + 257)
    clamp = (-2.0, 2.0)
    for i, (row, order) in enumerate(_rows()):
        prev = d["x0_prev"] if order == 2 else None
        ref, x0, S, S0, share = D.step64_clip(d["x"], d["model_out"], prev, row, 4.0, use_cfg, clamp)
        out32, x032, _, _, _ = D.step64_clip(d["x"], d["model_out"], prev, row, 4.0, use_cfg, clamp, dtype=torch.float32)
        assert out32.dtype == torch.float32 and x0.abs().max().item() <= 2.0 and x032.abs().max().item() <= 2.0
        print(f"cfg {use_cfg} alpha_s {row[0]:.3f} order {order}: clamped share {share:.3f}; fp32 / bound  out "
              f"{R.worst_ratio(out32, ref, R.bound_out(S)):.3f}  x0 {R.worst_ratio(x032, x0, R.bound_x0(S0)):.3f}")
        if i > 0:
            assert 0.1 <= share <= 0.9           # both sides of the clamp
        assert (x0 == 2.0).any() and (x0 == -2.0).any()
        assert R.violations(out32, ref, R.bound_out(S)) == 0 and R.violations(x032, x0, R.bound_x0(S0)) == 0
        for mut in D.CLIP_MUTANTS:
            bad, bad0, _, _, _ = D.step64_clip(d["x"], d["model_out"], prev, row, 4.0, use_cfg, clamp, mut=mut)
            n_bad = R.violations(bad, ref, R.bound_out(S)) + R.violations(bad0, x0, R.bound_x0(S0))
            assert n_bad > 0.05 * ref.numel(), (mut, i, n_bad)


def test_no_clip_bounds_give_the_unclamped_step_and_a_nan_passes_through():
    d = R.step_inputs(2, 33, seed=3)
    row = _rows()[1][0]
    ref, x0, _, _ = R.step64(d["x"], d["model_out"], d["x0_prev"], row, 4.0, 1)
    out, x0c, _, _, share = D.step64_clip(d["x"], d["model_out"], d["x0_prev"], row, 4.0, 1, D.NO_CLIP)
    assert torch.equal(out, ref) and torch.equal(x0, x0c) and share == 0.0
    x = d["x"].clone()
    x[0, 0, 0] = float("nan")
    _, x0n, _, _, _ = D.step64_clip(x, d["model_out"], None, row, 4.0, 1, (-2.0, 2.0))
    assert torch.isnan(x0n[0, 0, 0]) and torch.isfinite(x0n[1]).all()


# ---- 3. the decoders' host logic on a stub UNet ------------------------------------------------------------------------------------------------
class _StubUNet:
    """stands in for UNet2DConditionHIP: records the one-graph call, or every stepwise call's timestep"""
    config = type("cfg", (), {"in_channels": 4})

    def __init__(self, use_graph):
        self.use_graph, self.ts, self.got = use_graph, [], None

    def fixed_conditioning(self):
        return contextlib.nullcontext(self)

    def __call__(self, inp, t, **kw):
        self.ts.append(int(t[0]))
        return torch.zeros(inp.shape[0], 8, inp.shape[2], inp.shape[3])

    def dpmpp_loop(self, x, ts_rows, table, orders, guidance_scale, clamp, **kw):
        self.got = dict(x=x, ts_rows=ts_rows, table=table, orders=list(orders), guidance=guidance_scale, clamp=clamp, **kw)
        return x + 1.0, x + 2.0

    def sample_loop(self, x, *a, **kw):
        self.got = "ddpm"
        return x


def _decoder(unet, cfg=k22.SCHEDULER_CONFIG_2_2_LEARNED_RANGE, **kw):
    return pipeline22.KandinskyV22DecoderHIP(unet, None, k22.DDPMSchedulerHIP.from_config(cfg), **kw)


def test_decoder_routes_dpm_sampler_to_the_one_graph_loop_with_the_schedule_and_the_clip(monkeypatch):
    monkeypatch.setattr(pipeline22.KandinskyV22DecoderHIP, "_check", lambda self, e: None)
    bs, h, w = 2, 4, 4
    g = torch.Generator().manual_seed(3)
    lat, pos, neg = torch.randn(bs, 4, h, w, generator=g), torch.randn(bs, 8, generator=g), torch.randn(bs, 8, generator=g)
    u = _StubUNet(True)
    dec = _decoder(u, sampler="dpm_sampler")
    out = dec(pos, neg, height=8 * h, width=8 * w, num_inference_steps=50, guidance_scale=3.0, latents=lat, output_type="latent")
    ts, table, orders = sampling.dpmpp_schedule(AC22, 50)
    assert dec.last_timesteps == [int(t) for t in ts] and len(dec.last_timesteps) == 48          # fewer steps than asked for
    assert torch.equal(out, lat + 1.0) and torch.equal(dec.last_x0, lat + 2.0) and not u.ts
    assert torch.equal(u.got["x"], torch.cat([lat, lat])) and u.got["orders"] == list(orders) and u.got["guidance"] == 3.0
    assert torch.equal(u.got["table"], torch.from_numpy(table.astype(np.float32)))
    assert torch.equal(u.got["ts_rows"], torch.tensor(ts.astype(np.float32))[:, None].expand(-1, 2 * bs))
    assert u.got["clamp"] == (-2.0, 2.0) and u.got["keep"] is None and u.got["hint"] is None and u.got["inpaint_image"] is None
    assert torch.equal(u.got["image_embeds"], torch.cat([pos, neg]))
    # no clip_sample: the DDPM route's "no clip" pair; the per-call override; solver_order reaches the table
    u = _StubUNet(True)
    dec = _decoder(u, cfg=k22.SCHEDULER_CONFIG_2_2, solver_order=1)
    assert dec.sampler == "ddpm_sampler"
    dec(pos, neg, height=8 * h, width=8 * w, num_inference_steps=6, latents=lat, output_type="latent", sampler="dpm_sampler")
    assert u.got["clamp"] == (-3.0e38, 3.0e38) and u.got["orders"] == [1] * 6 and dec.last_timesteps == [999, 794, 537, 246, 61, 8]
    dec(pos, neg, height=8 * h, width=8 * w, num_inference_steps=6, latents=lat, noise_seq=torch.zeros(6, bs, 4, h, w), output_type="latent")
    assert u.got == "ddpm"                                                                       # the default stays the DDPM loop


def test_decoder_stepwise_route_calls_the_unet_at_the_grid_and_more_than_100_steps_stay_stepwise(monkeypatch):
    monkeypatch.setattr(pipeline22.KandinskyV22DecoderHIP, "_check", lambda self, e: None)
    launched = []

    def fake_loop(model_call, x, rows, orders, *, guidance, clamp, keep=None):
        for k in range(len(orders)):
            model_call(x, k)
        launched.append((tuple(rows.shape), list(orders), guidance, clamp, keep))
        return x, x

    monkeypatch.setattr(sampling, "dpmpp_loop_keep", fake_loop)
    bs, h, w = 1, 4, 4
    lat, emb = torch.zeros(bs, 4, h, w), torch.zeros(bs, 8)
    for use_graph, flag, S in ((False, None, 6), (True, False, 6), (True, True, 200)):
        u = _StubUNet(use_graph)
        dec = _decoder(u, whole_loop_graph=flag, sampler="dpm_sampler")
        dec(emb, emb, height=8 * h, width=8 * w, num_inference_steps=S, latents=lat, output_type="latent")
        assert u.got is None and u.ts == dec.last_timesteps == [int(t) for t in sampling.dpmpp_schedule(AC22, S)[0]]
        assert launched[-1][0] == (len(u.ts), 5) and launched[-1][2:] == (4.0, (-2.0, 2.0), None)
        assert (len(u.ts) > pipeline22.MAX_LOOP_GRAPH_STEPS) == (S == 200)


def test_decoders_refuse_a_noise_seq_and_an_unknown_sampler(monkeypatch):
    monkeypatch.setattr(pipeline22.KandinskyV22DecoderHIP, "_check", lambda self, e: None)
    emb, lat = torch.zeros(1, 8), torch.zeros(1, 4, 4, 4)
    with pytest.raises(ValueError, match="sampler must be one of"):
        _decoder(_StubUNet(True), sampler="euler_sampler")
    with pytest.raises(ValueError, match="solver_order"):
        _decoder(_StubUNet(True), sampler="dpm_sampler", solver_order=3)
    t2i = _decoder(_StubUNet(True))
    i2i = pipeline22.KandinskyV22Img2ImgDecoderHIP(_StubUNet(True), None, None)
    inp = pipeline22.KandinskyV22InpaintDecoderHIP(_StubUNet(True), None, None)
    nz = torch.zeros(6, 1, 4, 4, 4)
    for dec, kw in ((t2i, {}), (i2i, dict(image=lat)), (inp, dict(image=lat, mask_image=np.ones((32, 32))))):
        with pytest.raises(ValueError, match="sampler must be one of"):
            dec(emb, emb, height=32, width=32, num_inference_steps=6, output_type="latent", sampler="plms_sampler", **kw)
        with pytest.raises(ValueError, match="deterministic"):
            dec(emb, emb, height=32, width=32, num_inference_steps=6, output_type="latent", sampler="dpm_sampler", noise_seq=nz, **kw)
        assert dec.sampler == "ddpm_sampler" and dec.solver_order == 2 and dec.last_timesteps is None


def test_sampler_keyword_reaches_the_decoders_through_the_wrapper():
    for cls in (pipeline22.KandinskyV22DecoderHIP, pipeline22.KandinskyV22Img2ImgDecoderHIP, pipeline22.KandinskyV22InpaintDecoderHIP):
        p = inspect.signature(cls.__init__).parameters
        assert p["sampler"].default == "ddpm_sampler" and p["solver_order"].default == 2
        assert inspect.signature(cls.__call__).parameters["sampler"].default is None
    ref_positional = {"generate_text2img": ["prompt", "batch_size", "decoder_steps", "prior_steps", "decoder_guidance_scale", "prior_guidance_scale",
                                            "h", "w", "negative_prior_prompt", "negative_decoder_prompt"],
                      "generate_img2img": ["prompt", "image", "strength", "batch_size", "decoder_steps"],
                      "mix_images": ["images_texts", "weights", "batch_size", "decoder_steps"],
                      "generate_inpainting": ["prompt", "pil_img", "img_mask", "batch_size", "decoder_steps"]}
    for name, head in ref_positional.items():
        p = inspect.signature(getattr(pipeline22.Kandinsky2_2HIP, name)).parameters
        assert p["sampler"].kind is inspect.Parameter.KEYWORD_ONLY and p["sampler"].default is None
        assert list(p)[1:1 + len(head)] == head                                    # the reference's positional signature stays
    with pytest.raises(NotImplementedError):                                       # the project's sampler, not a diffusers scheduler class
        k22.DDPMSchedulerHIP.from_config(dict(k22.SCHEDULER_CONFIG_2_2, _class_name="DPMSolverMultistepScheduler"))


# ---- 4. the C entries ----------------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "k22.h")).read()
    L = _lib.lib()
    for name in ("k22_dpmpp_step_clip", "k22_unet_dpmpp_loop_keep"):
        decl = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
        assert hasattr(L, name) and len(_lib.SIGNATURES[name][1]) == len(decl.split(","))
    assert len(_lib.SIGNATURES["k22_dpmpp_step"][1]) == 11 and len(_lib.SIGNATURES["k22_dpmpp_step_clip"][1]) == 13
    assert len(_lib.SIGNATURES["k22_unet_dpmpp_loop"][1]) == 13 and len(_lib.SIGNATURES["k22_unet_dpmpp_loop_keep"][1]) == 19
    assert "k22_dpmpp_step_clip" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "k22_unet_dpmpp_loop_keep" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_null_arguments_and_bad_bounds_are_refused_without_a_device():
    L = _lib.lib()
    assert L.k22_dpmpp_step_clip(None, None, None, None, 4.0, 1, -2.0, 2.0, None, None, 2, 16, None) == -1
    assert b"dpmpp_step_clip" in L.k22_last_error()
    coef = (C.c_float * 2)(1.0, 0.0)
    rc = L.k22_unet_dpmpp_loop_keep(None, None, None, None, None, None, None, None, None, 1, 4.0, -2.0, 2.0, None, None, None, coef, 1, None)
    assert rc == -1 and b"all four or none" in L.k22_last_error()
    rc = L.k22_unet_dpmpp_loop_keep(None, None, None, None, None, None, None, None, None, 1, 4.0, -2.0, 2.0, None, None, None, None, 1, None)
    assert rc == -1 and b"unet_dpmpp_loop_keep" in L.k22_last_error() and b"bind a workspace first" in L.k22_last_error()
