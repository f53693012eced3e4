"""Host side of the one-graph 2.2 decoder loop (no GPU): the float64 reference and bound of k22_keep_region, the operand and noise helpers
against what the stepwise route hands over step by step, the route switch of the decoders, and the two new C entries' declarations.

PARITY UNPINNED, as everything on the 2.2 path (oracle/unet22_ref.py restates diffusers from memory): these tests compare the one-graph
route's host side with the stepwise route's and with that restatement, not with diffusers."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import decoder22_ref as dr
import kandinsky2_amd as k22
from kandinsky2_amd import _lib, pipeline22, sampling
from oracle import unet22_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SA, SB = float(np.float32(0.8311 ** 0.5)), float(np.float32((1 - 0.8311) ** 0.5))


# ---- the kernel's reference and bound ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs,H,W,kind", [(1, 12, 20, "binary"), (2, 12, 20, "fractional"), (3, 12, 20, "binary"), (2, 1, 1, "fractional")])
def test_torch_fp32_evaluation_is_inside_the_derived_bound(bs, H, W, kind):
    d = dr.keep_inputs(bs, H, W, kind, seed=bs)
    for sa, sb in ((SA, SB), (1.0, 0.0)):
        ref, S = dr.keep_region_ref(d, sa, sb)
        v32, _ = dr.keep_region_ref(d, sa, sb, dtype=torch.float32)
        bound = dr.keep_bound(S)
        ratio = dr.worst_ratio(v32, ref, bound)
        print(f"keep_region bs {bs} {H}x{W} {kind} (sa, sb) = ({sa:.4f}, {sb:.4f}): torch fp32 worst |d| / bound {ratio:.3f}")
        assert v32.dtype == torch.float32 and dr.violations(v32, ref, bound) == 0
        # by hand, one element: row B - 1 is sample bs - 1's second CFG half
        n, c, y, x_ = 2 * bs - 1, 3, H - 1, W - 1
        m = float(d["mask"][y, x_])
        want = m * (sa * float(d["init"][c, y, x_]) + sb * float(d["noise0"][n % bs, c, y, x_])) + (1 - m) * float(d["x"][n, c, y, x_])
        assert abs(float(ref[n, c, y, x_]) - want) <= 1e-12 * max(1.0, abs(want))


@pytest.mark.parametrize("mut", dr.MUTANTS)
@pytest.mark.parametrize("kind", ["binary", "fractional"])
def test_every_mutant_is_rejected(mut, kind):
    """evaluated exactly (float64), each wrong variant leaves the bound on the shapes the GPU test uses: the inputs tell it apart"""
    d = dr.keep_inputs(2, 12, 20, kind, seed=7)
    ref, S = dr.keep_region_ref(d, SA, SB)
    bad, _ = dr.keep_region_ref(d, SA, SB, mut=mut)
    assert dr.violations(bad, ref, dr.keep_bound(S)) > 0


# ---- the operand helper against the stepwise route ---------------------------------------------------------------------------------------
class _RecUNet:
    """stands in for UNet2DConditionHIP on the stepwise route: records the timestep of every call"""
    use_graph = False

    def __init__(self):
        self.ts = []

    def fixed_conditioning(self):
        import contextlib
        return contextlib.nullcontext(self)

    def __call__(self, inp, t, **kw):
        self.ts.append(t)
        return torch.zeros(inp.shape[0], 8, inp.shape[2], inp.shape[3])


class _RecScheduler(k22.DDPMSchedulerHIP):
    """records the table row DDPMSchedulerHIP.step looks up; returns the sample"""

    def step(self, model_output, timestep, sample, **kw):
        self.rows.append(self._row[int(timestep)])
        return SimpleNamespace(prev_sample=sample)


class _RecLib:
    """stands in for the library under KnownRegion.__call__: keeps (sa, sb) as they arrive behind the C ABI's float parameters"""

    def __init__(self):
        self.coef = []

    def k22_blend_noised(self, x, init, noise, mask, sa, sb, *rest):
        self.coef.append((C.c_float(sa).value, C.c_float(sb).value))
        return 0


def _stepwise_record(monkeypatch, sch, ts, bs=2, h=4, w=4):
    unet, rec = _RecUNet(), _RecLib()
    sch.rows = []
    dec = pipeline22.KandinskyV22DecoderHIP(unet, None, sch, whole_loop_graph=False)
    monkeypatch.setattr(pipeline22, "_lib", SimpleNamespace(lib=lambda: rec, check=lambda rc: None, current_stream=lambda: None))
    x = torch.zeros(bs, 4, h, w)
    keep = pipeline22.KnownRegion(torch.zeros(1, 4, h, w), x.clone(), torch.ones(1, 1, h, w), sch, ts)
    dec._denoise(x, torch.zeros(2 * bs, 8), ts, 4.0, torch.zeros(len(ts), bs, 4, h, w), None, after_step=keep)
    return unet.ts, sch.rows, rec.coef[::bs]     # one blend per sample and step: every sample gets the step's pair


@pytest.mark.parametrize("spacing", ["leading", "trailing"])
@pytest.mark.parametrize("steps,t_start", [(5, 0), (10, 0), (10, 5)])
def test_loop_operands_equal_what_the_stepwise_route_passes(monkeypatch, spacing, steps, t_start):
    cfg = dict(k22.SCHEDULER_CONFIG_2_2, timestep_spacing=spacing)
    sch = _RecScheduler.from_config(cfg).set_timesteps(steps, device="cpu")
    ref = unet22_ref.RefDDPMScheduler(steps, dict(unet22_ref.SCHED_2_2, timestep_spacing=spacing))
    assert sch.timesteps.tolist() == ref.timesteps.tolist()
    ts = sch.timesteps.tolist()[t_start:]                     # t_start > 0: the img2img tail
    B = 4
    ts_rows, rows, coef = sampling.ddpm_loop_operands(sch, ts, B, keep=True)
    got_ts, got_rows, got_coef = _stepwise_record(monkeypatch, sch, ts)
    assert ts_rows.dtype == torch.float32 and tuple(ts_rows.shape) == (len(ts), B) and ts_rows.is_contiguous()
    for k, t in enumerate(got_ts):                            # forward: torch.as_tensor(t).float() expanded to the batch
        assert torch.equal(ts_rows[k], torch.as_tensor(t).float().reshape(-1).expand(B))
    assert rows == got_rows == list(range(t_start, steps))
    assert coef.dtype == np.float32 and coef.shape == (len(ts), 2)
    want = np.array(got_coef, dtype=np.float32)
    assert np.array_equal(coef.view(np.uint32), want.view(np.uint32))                 # fp32 bit patterns
    assert coef[-1].tolist() == [1.0, 0.0]
    ac = sch.alphas_cumprod
    assert coef[0].tolist() == [float(np.float32(float(ac[ts[1]]) ** 0.5)), float(np.float32((1.0 - float(ac[ts[1]])) ** 0.5))]
    assert sampling.ddpm_loop_operands(sch, ts, B)[2] is None


# ---- the noise helper ------------------------------------------------------------------------------------------------------------------
def test_step_noise_equals_the_stepwise_draws_of_a_cpu_generator():
    n, shape = 5, (4, 4, 6, 5)
    g1, g2 = torch.Generator().manual_seed(123), torch.Generator().manual_seed(123)
    x1 = torch.randn(2, 4, 6, 5, generator=g1)                # the initial latent is drawn first, on both routes
    nzs = sampling.ddpm_step_noise(n, shape, g1, "cpu")
    x2 = torch.randn(2, 4, 6, 5, generator=g2)
    assert torch.equal(x1, x2) and tuple(nzs.shape) == (n,) + shape and nzs.dtype == torch.float32
    for k in range(n):                                        # DDPMSchedulerHIP.step: randn(sample.shape, generator=, device=generator.device)
        assert torch.equal(nzs[k], torch.randn(shape, generator=g2, device=g2.device))
    assert torch.equal(torch.randn(3, generator=g1), torch.randn(3, generator=g2))    # and the generators end in the same state


# ---- the decoders' route switch ----------------------------------------------------------------------------------------------------------
class _LoopUNet(_RecUNet):
    use_graph = True

    def sample_loop(self, x, ts_rows, noise_seq, table, table_rows, guidance_scale, clamp, **kw):
        self.got = dict(x=x, ts_rows=ts_rows, noise_seq=noise_seq, table=table, rows=table_rows, guidance=guidance_scale, clamp=clamp, **kw)
        return x + 1.0


def _decoder(flag, unet):
    sch = _RecScheduler.from_config(k22.SCHEDULER_CONFIG_2_2_LEARNED_RANGE).set_timesteps(5, device="cpu")
    sch.rows = []
    return pipeline22.KandinskyV22DecoderHIP(unet, None, sch, whole_loop_graph=flag), sch


def test_denoise_takes_the_one_graph_route_only_where_it_may():
    bs, h, w = 2, 4, 4
    g = torch.Generator().manual_seed(3)
    x, emb, nz = torch.randn(bs, 4, h, w, generator=g), torch.randn(2 * bs, 8, generator=g), torch.randn(5, bs, 4, h, w, generator=g)
    # None follows unet.use_graph
    u = _LoopUNet()
    dec, sch = _decoder(None, u)
    ts = sch.timesteps.tolist()
    out = dec._denoise(x, emb, ts, 4.0, nz, None)
    assert torch.equal(out, x + 1.0) and not u.ts and not sch.rows
    assert torch.equal(u.got["x"], torch.cat([x, x])) and torch.equal(u.got["noise_seq"], torch.cat([nz, nz], 1))
    assert u.got["rows"] == [0, 1, 2, 3, 4] and u.got["clamp"] == (-2.0, 2.0) and u.got["keep"] is None and u.got["hint"] is None
    assert torch.equal(u.got["image_embeds"], emb) and u.got["table"] is sch._table
    u2 = _RecUNet()                                           # use_graph False: stepwise
    dec2, sch2 = _decoder(None, u2)
    dec2._denoise(x, emb, ts, 4.0, nz, None)
    assert u2.ts == ts and sch2.rows == [0, 1, 2, 3, 4]
    # off; an arbitrary callback; no step; more than 100 steps: stepwise
    for flag, after, tss in ((False, None, ts), (True, lambda k, cur: cur, ts), (True, None, []), (True, None, [ts[0]] * 101)):
        u = _LoopUNet()
        dec, sch = _decoder(flag, u)
        dec._denoise(x, emb, tss, 4.0, torch.zeros(max(len(tss), 1), bs, 4, h, w), None, after_step=after)
        assert not hasattr(u, "got") and len(u.ts) == len(tss)
    u = _LoopUNet()                                           # exactly 100 steps: one graph
    dec, sch = _decoder(True, u)
    dec._denoise(x, emb, [ts[0]] * 100, 4.0, torch.zeros(100, bs, 4, h, w), None)
    assert len(u.got["rows"]) == 100
    # the known-region after_step goes with the graph; its operands and coefficients are handed over
    u = _LoopUNet()
    dec, sch = _decoder(True, u)
    lat0, m = torch.randn(1, 4, h, w, generator=g), torch.ones(1, 1, h, w)
    extra = torch.cat([lat0 * m, m], 1).repeat(2 * bs, 1, 1, 1)
    dec._denoise(x, emb, ts, 4.0, nz, None, extra=extra, after_step=pipeline22.KnownRegion(lat0, x.clone(), m, sch, ts))
    k_init, k_noise, k_mask, coef = u.got["keep"]
    assert k_init is lat0 and torch.equal(k_noise, x) and k_mask is m and coef.shape == (5, 2) and coef[-1].tolist() == [1.0, 0.0]
    assert torch.equal(u.got["inpaint_image"], extra[:, :4]) and torch.equal(u.got["inpaint_mask"], extra[:, 4:5])


def test_generator_drawn_noise_of_the_one_graph_route_is_the_stepwise_draw_sequence():
    bs, h, w = 1, 4, 4
    u = _LoopUNet()
    dec, sch = _decoder(True, u)
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    dec._denoise(torch.zeros(bs, 4, h, w), torch.zeros(2, 8), sch.timesteps.tolist(), 4.0, None, g1)
    for k in range(5):
        assert torch.equal(u.got["noise_seq"][k], torch.randn(2 * bs, 4, h, w, generator=g2))


def test_flag_reaches_the_decoders_through_the_wrapper_signature():
    import inspect
    for cls in (pipeline22.KandinskyV22DecoderHIP, pipeline22.KandinskyV22Img2ImgDecoderHIP, pipeline22.KandinskyV22InpaintDecoderHIP,
                pipeline22.Kandinsky2_2HIP):
        p = inspect.signature(cls.__init__).parameters["whole_loop_graph"]
        assert p.default is None
    assert inspect.signature(pipeline22.load_decoder22_from_cache_dir).parameters["whole_loop_graph"].default is None
    d = pipeline22.KandinskyV22InpaintDecoderHIP(None, None, None, whole_loop_graph=True)
    assert d.whole_loop_graph is True and pipeline22.MAX_LOOP_GRAPH_STEPS == 100


# ---- the C entries -----------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "k22.h")).read()
    L = _lib.lib()
    for name in ("k22_unet_sample_loop_keep", "k22_keep_region"):
        decl = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
        assert hasattr(L, name) and len(_lib.SIGNATURES[name][1]) == len(decl.split(","))
    # k22_unet_sample_loop keeps its signature; the new entry is that signature plus the four keep arguments
    assert len(_lib.SIGNATURES["k22_unet_sample_loop"][1]) == 20 and len(_lib.SIGNATURES["k22_unet_sample_loop_keep"][1]) == 24


def test_null_arguments_are_refused_without_a_device():
    L = _lib.lib()
    assert L.k22_keep_region(None, None, None, None, 1.0, 0.0, None, 2, 16, None) == -1 and b"keep_region" in L.k22_last_error()
    coef = (C.c_float * 2)(1.0, 0.0)
    rc = L.k22_unet_sample_loop_keep(None, None, None, None, None, None, None, None, None, None, None, 1, 4.0, -2.0, 2.0, -1, 0.0, None,
                                     None, None, None, coef, 1, None)
    assert rc == -1 and b"all four or none" in L.k22_last_error()
    rc = L.k22_unet_sample_loop_keep(None, None, None, None, None, None, None, None, None, None, None, 1, 4.0, -2.0, 2.0, -1, 0.0, None,
                                     None, None, None, None, 1, None)
    assert rc == -1 and b"bind a workspace first" in L.k22_last_error()
