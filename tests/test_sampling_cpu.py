"""The host-driven sampler loops of kandinsky2_amd.sampling (no GPU, no library call): each loop is driven with a recording model_call and a
recording step launcher, and the recorded sequence is compared with one written out from the samplers' definition
(kandinsky2/model/samplers.py: PLMSSampler.plms_sampling / p_sample_plms, DDIMSampler.ddim_sampling; gaussian_diffusion.py:
p_sample_loop_progressive) - not computed by the code under test.  Tensors are told apart by identity (data_ptr); a launcher "writes" by
filling its outputs with a fresh tag, so that what a later call reads shows which launch wrote it."""
import numpy as np
import pytest
import torch

import kandinsky2_amd as k22
from kandinsky2_amd import diffusion, sampling


def _x(n=2, seed=0):
    return torch.randn(n, 4, 2, 3, generator=torch.Generator().manual_seed(seed))


class _Rec:
    """recording model_call + step launchers; every launch fills its outputs with the next tag 1, 2, 3, ..."""

    def __init__(self):
        self.calls, self.steps, self.tag = [], [], 0

    def model_call(self, x, c):
        self.calls.append((c, x.data_ptr(), float(x.flatten()[0])))
        return torch.full((x.shape[0], 8) + tuple(x.shape[2:]), float(len(self.calls)))

    def _write(self, *outs):
        self.tag += 1
        for o in outs:
            if o is not None:
                o.fill_(float(self.tag))

    def plms(self, x, out, hist, order, row, x_out, eps_out, x0_out, **kw):
        self.steps.append(dict(x=x.data_ptr(), out=float(out.flatten()[0]), hist=[h.data_ptr() for h in hist], order=order, row=row.clone(),
                               x_out=x_out.data_ptr(), eps_out=None if eps_out is None else eps_out.data_ptr(), x0_out=x0_out, kw=kw))
        self._write(x_out, eps_out, x0_out)

    def step(self, x, out, noise, row, x_out, x0_out, **kw):
        self.steps.append(dict(x=x.data_ptr(), out=float(out.flatten()[0]), noise=noise, row=row, x_out=x_out.data_ptr(), x0_out=x0_out, kw=kw))
        self._write(x_out, x0_out)


# ---- PLMS ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_plms_loop_sequence(n):
    r, x_T = _Rec(), _x()
    table = torch.arange(4.0 * n).reshape(n, 4)
    x, x0 = sampling.plms_loop(r.model_call, x_T, table, r.plms, guidance=4.0)
    s = r.steps
    assert [d["order"] for d in s] == ([0, 4, 1, 2, 3] + [3] * n)[: n + 1]
    assert [c for c, _, _ in r.calls] == list(range(n + 1))                    # one model call per launch, numbered in execution order
    assert [d["out"] for d in s] == [float(k + 1) for k in range(n + 1)]       # launch k consumes the output of model call k
    step_of = [0] + list(range(n))                                               # the first step makes two launches
    for d, k in zip(s, step_of):
        assert torch.equal(d["row"], table[k]) and d["kw"] == {"guidance": 4.0}
    # the second call runs on the provisional latent the first launch wrote (tag 1); both launches of step 0 read x_T and write one buffer
    assert r.calls[0][1] == x_T.data_ptr() and r.calls[1][1] == s[0]["x_out"] and r.calls[1][2] == 1.0
    assert s[0]["x"] == s[1]["x"] == x_T.data_ptr() and s[0]["x_out"] == s[1]["x_out"] != x_T.data_ptr()
    # current / next swap: every later launch reads what the launch before it wrote, and writes the other buffer
    for a, b, call in zip(s[1:], s[2:], r.calls[2:]):
        assert b["x"] == a["x_out"] == call[1] and b["x_out"] == a["x"]
    assert x.data_ptr() == s[-1]["x_out"] and float(x.flatten()[0]) == float(n + 1)
    assert x0 is s[-1]["x0_out"] and float(x0.flatten()[0]) == float(n + 1)
    # eps ring: history newest first = the eps_out of the preceding steps, never more than three, eps_out none of them; four slots in all
    assert s[0]["hist"] == [] and s[0]["eps_out"] is not None and s[0]["x0_out"] is None
    assert s[1]["hist"] == [s[0]["eps_out"]] and s[1]["eps_out"] is None
    assert all(d["x0_out"] is x0 for d in s[1:])
    written = [s[0]["eps_out"]]
    for d in s[2:]:
        assert d["hist"] == written[::-1][:3] and len(d["hist"]) == d["order"]
        assert d["eps_out"] is not None and d["eps_out"] not in d["hist"]
        written.append(d["eps_out"])
    assert len(set(written)) == min(n, 4) and not set(written) & {s[0]["x"], s[0]["x_out"], x0.data_ptr()}


def test_plms_call_timesteps():
    assert sampling.plms_calls([]) == [] and sampling.plms_calls([7]) == [7, 7] and sampling.plms_calls([9, 7]) == [9, 7, 7]
    assert sampling.plms_calls([9, 7, 5, 3]) == [9, 7, 7, 5, 3]


# ---- DDIM and p_sampler: one launch per step -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_ddim_loop_sequence(n, eta):
    r, x_T = _Rec(), _x()
    table = torch.arange(4.0 * n).reshape(n, 4)
    noise = torch.randn(n, *x_T.shape) if eta else None
    x0_buf = torch.empty_like(x_T)
    x, x0 = sampling.step_loop(r.model_call, x_T, table, noise, x0_buf, r.step, guidance=3.0)
    s = r.steps
    assert len(s) == n and [c for c, _, _ in r.calls] == list(range(n))
    for k, d in enumerate(s):
        assert torch.equal(d["row"], table[k]) and d["out"] == float(k + 1) and d["x0_out"] is x0_buf and d["kw"] == {"guidance": 3.0}
        assert d["noise"] is None if not eta else d["noise"].data_ptr() == noise[k].data_ptr()
        assert r.calls[k][1] == d["x"] == (x_T.data_ptr() if k == 0 else s[k - 1]["x_out"]) and d["x_out"] != d["x"]
        assert k < 2 or d["x_out"] == s[k - 2]["x_out"]                      # two buffers, swapped
    assert x.data_ptr() == s[-1]["x_out"] and float(x.flatten()[0]) == float(n) and x0 is x0_buf


@pytest.mark.parametrize("n,init_step", [(1, None), (4, None), (6, 3)])
@pytest.mark.parametrize("want_x0", [False, True])
def test_p_sampler_loop_sequence(n, init_step, want_x0):
    """rows as SpacedDiffusionHIP.p_sample_loop builds them: table row T-1 ... 0, with init_step only the rows below it"""
    rows = list(range(n))[::-1] if init_step is None else list(range(n))[:init_step][::-1]
    want_rows = {(1, None): [0], (4, None): [3, 2, 1, 0], (6, 3): [2, 1, 0]}[(n, init_step)]
    r, x_T = _Rec(), _x()
    noise = torch.randn(len(rows), *x_T.shape)
    ops = dict(table="T", guidance=4.0, use_cfg=True, clamp=(-2.0, 2.0), pct=(7, 0.5), init="I", mask="M", scratch="S")
    x0_buf = torch.empty_like(x_T) if want_x0 else None
    x, x0 = sampling.step_loop(r.model_call, x_T, rows, noise, x0_buf, r.step, **ops)
    s = r.steps
    assert [d["row"] for d in s] == want_rows and all(d["kw"] == ops and d["x0_out"] is x0_buf for d in s)
    for k, d in enumerate(s):
        assert d["noise"].data_ptr() == noise[k].data_ptr() and d["out"] == float(k + 1)
        assert r.calls[k][0] == k and r.calls[k][1] == d["x"] == (x_T.data_ptr() if k == 0 else s[k - 1]["x_out"]) and d["x_out"] != d["x"]
    assert x.data_ptr() == s[-1]["x_out"] and float(x.flatten()[0]) == float(len(rows)) and x0 is x0_buf


def test_model_call_forms():
    """fused: the UNet sees [first half | first half] at the call's timestep row; drop-in: model_fn sees x itself, its output shape is checked"""
    x, ts, seen = _x(4), torch.arange(12.0).reshape(3, 4), []

    def model(xx, t, **kw):
        seen.append((xx.clone(), t.clone(), kw))
        return torch.zeros(4, 8, 2, 3, dtype=torch.float64)

    out = sampling.fused_call(model, ts, full_emb=1)(x, 2)
    assert out.shape == (4, 8, 2, 3)
    assert torch.equal(seen[0][0][:2], x[:2]) and torch.equal(seen[0][0][2:], x[:2]) and torch.equal(seen[0][1], ts[2]) and seen[0][2] == {"full_emb": 1}
    assert torch.equal(sampling.cfg_input(x), torch.cat([x[:2], x[:2]]))
    out = diffusion._model_fn_call(model, ts, full_emb=1)(x, 1)
    assert torch.equal(seen[1][0], x) and torch.equal(seen[1][1], ts[1]) and out.dtype == torch.float32 and out.is_contiguous()
    with pytest.raises(ValueError, match="model_fn must return"):
        diffusion._model_fn_call(lambda xx, t: xx, ts)(x, 0)


# ---- the samplers through the loops: timesteps of the model calls, generator draws -----------------------------------------------------
class _Model:
    def __init__(self):
        self.ts = []

    def __call__(self, x, ts, **kw):
        self.ts.append(ts.tolist())
        return torch.zeros(x.shape[0], 8, *x.shape[2:])


@pytest.mark.parametrize("init_step,steps", [(1, [1]), (201, [201, 1]), (401, [401, 201, 1]), (None, [801, 601, 401, 201, 1])])
def test_stepwise_samplers_call_the_model_at_the_reference_timesteps(init_step, steps):
    old = k22.create_gaussian_diffusion(**k22.DIFFUSION_CONFIG_2_1)
    x_T, rec = _x(), _Rec()

    class PLMS(k22.PLMSSamplerHIP):
        _step = lambda self, *a: rec.plms(*a)

    class DDIM(k22.DDIMSamplerHIP):
        _ddim_step = lambda self, *a: rec.step(*a)

    ac = old.alphas_cumprod
    for cls, calls in ((PLMS, [steps[0], steps[min(1, len(steps) - 1)]] + steps[1:]), (DDIM, steps)):
        m, rec.steps = _Model(), []
        cls(m, old, 4.0).sample(5, 2, (4, 2, 3), x_T=x_T, init_step=init_step, device="cpu")
        assert m.ts == [[float(c)] * 2 for c in calls]
        rows = [d["row"] for d in rec.steps]
        a_t = [float(np.float32(ac[t])) for t in ([steps[0]] + steps if cls is PLMS else steps)]     # a_t of the step a launch belongs to
        assert [float(r[0]) for r in rows] == a_t


def test_generator_draws():
    """p_sampler: one draw per step; DDIM: one per step at eta > 0, none at eta 0; PLMS none; none where noise_seq is given"""
    x, old = _x(), k22.create_gaussian_diffusion(**k22.DIFFUSION_CONFIG_2_1)
    torch.manual_seed(11)
    want = [torch.randn_like(x) for _ in range(4)]
    after = torch.randn(3)
    torch.manual_seed(11)
    got = sampling.step_noise(x, 4)
    assert torch.equal(got, torch.stack(want)) and torch.equal(torch.randn(3), after)
    given = torch.randn(6, *x.shape)
    torch.manual_seed(11)
    assert torch.equal(sampling.step_noise(x, 4, given), given[:4])
    untouched = torch.randn(3)
    torch.manual_seed(11)
    assert torch.equal(untouched, torch.randn(3))

    rec = _Rec()

    class DDIM(k22.DDIMSamplerHIP):
        _ddim_step = lambda self, *a: rec.step(*a)

    class PLMS(k22.PLMSSamplerHIP):
        _step = lambda self, *a: rec.plms(*a)

    for cls, eta, seq, draws in ((DDIM, 0.5, None, 3), (DDIM, 0.0, None, 0), (DDIM, 0.5, given, 0), (PLMS, 0.0, None, 0)):
        rec.steps = []
        torch.manual_seed(5)
        cls(_Model(), old, 4.0).sample(5, 2, (4, 2, 3), x_T=x, eta=eta, init_step=401, device="cpu", **({} if seq is None else {"noise_seq": seq}))
        tail = torch.randn(3)
        torch.manual_seed(5)
        drawn = [torch.randn_like(x) for _ in range(draws)]
        assert torch.equal(tail, torch.randn(3)), (cls, eta)
        if cls is DDIM:
            used = [d["noise"] for d in rec.steps]
            assert len(used) == 3
            if eta == 0.0:
                assert used == [None] * 3
            else:
                assert all(torch.equal(u, w) for u, w in zip(used, drawn if seq is None else given[:3]))


# ---- owned buffers ---------------------------------------------------------------------------------------------------------------------
def test_owned_buffers_reallocate_only_on_a_key_change():
    def stage(b, kind, n, noise):
        box = (2, 4, 2, 3)
        return b.stage((kind, 2, 2, 3, n, noise is not None, "cpu"), "cpu",
                       lambda: dict(x=box, ts=(n, 2), noise=(n,) + box if noise is not None else None, hist=(4,) + box if kind == "plms" else None,
                                    scratch=40),
                       dict(x=torch.full(box, 1.0), ts=torch.full((n, 2), 2.0), noise=noise, hist=None))

    def ptrs(bufs):
        return {k: None if v is None else v.data_ptr() for k, v in bufs.items()}

    b = sampling.OwnedBuffers()
    first = stage(b, "ddim", 5, None)
    p = ptrs(first)
    assert first["noise"] is None and first["hist"] is None and first["scratch"].dtype == torch.uint8 and first["scratch"].numel() == 40
    assert first["x"].dtype == torch.float32 and float(first["x"][0, 0, 0, 0]) == 1.0 and float(first["ts"][4, 1]) == 2.0
    first["x"].fill_(9.0)
    again = stage(b, "ddim", 5, None)
    assert ptrs(again) == p and float(again["x"][0, 0, 0, 0]) == 1.0            # same addresses, operands staged anew
    more = stage(b, "ddim", 6, None)                                              # another step count
    assert more is not first and tuple(more["ts"].shape) == (6, 2)
    plms = stage(b, "plms", 6, None)                                              # another kind
    assert plms is not more and tuple(plms["hist"].shape) == (4, 2, 4, 2, 3) and float(plms["hist"].abs().max()) == 0.0   # None stages zeros
    held = [first, more]                                                          # keep the old sets alive: a new set is new memory
    assert plms["x"].data_ptr() not in [h["x"].data_ptr() for h in held]
    noisy = stage(b, "ddim", 6, torch.full((6, 2, 4, 2, 3), 3.0))
    assert float(noisy["noise"][5, 1, 3, 1, 2]) == 3.0


def test_the_two_loop_entries_of_a_module_never_share_a_buffer_set():
    m = k22.Text2ImUNetHIP(k22.make_arch(k22.tiny_model_config()), meta_params=True)
    assert isinstance(m._loop_bufs, sampling.OwnedBuffers) and isinstance(m._ddim_bufs, sampling.OwnedBuffers) and m._loop_bufs is not m._ddim_bufs
    a, b = m._loop_bufs, m._ddim_bufs
    key, shapes = ("k",), lambda: dict(x=(2, 4, 2, 3))
    sa, sb = a.stage(key, "cpu", shapes, dict(x=None)), b.stage(key, "cpu", shapes, dict(x=None))
    assert sa is not sb and sa["x"].data_ptr() != sb["x"].data_ptr()
    m._release()                                                                  # new parameters: new engines, new buffer sets
    assert m._loop_bufs is not a and m._ddim_bufs is not b and m._loop_bufs is not m._ddim_bufs


def test_inpaint_operands_helper():
    x = _x(4)
    t2i = k22.Text2ImUNetHIP(k22.make_arch(k22.tiny_model_config()), meta_params=True)
    assert t2i._inpaint_operands(x, None, None) == (None, None)
    with pytest.raises(ValueError, match="given to a text2img UNet"):
        t2i._inpaint_operands(x, None, torch.zeros(4, 1, 2, 3))
    inp = k22.Text2ImUNetHIP(k22.make_arch(k22.tiny_model_config(), inpainting=True), meta_params=True)
    assert inp._inpaint_operands(x, None, None) == (None, None)                    # absent: the callers use zeros
    img, msk = inp._inpaint_operands(x, torch.ones(1, 4, 2, 3, dtype=torch.float64), torch.ones(4, 1, 1, 1))
    assert tuple(img.shape) == (4, 4, 2, 3) and tuple(msk.shape) == (4, 1, 2, 3) and img.dtype == msk.dtype == torch.float32
    with pytest.raises(ValueError, match="do not match x"):
        inp._inpaint_operands(x, torch.ones(3, 4, 2, 3), None)


def test_k22_chains_reaches_the_2_1_module_only_and_the_2_2_module_has_no_ddim_loop(monkeypatch):
    monkeypatch.setenv("K22_CHAINS", "2")
    assert k22.Text2ImUNetHIP(k22.make_arch(k22.tiny_model_config()), meta_params=True).chains == 2
    m = k22.UNet2DConditionHIP(k22.make_arch22(k22.tiny_unet22_config()), meta_params=True)
    assert m.chains == 1                                                          # its forward and set_condition address one engine
    with pytest.raises(NotImplementedError):                                      # the inherited loop conditions through the 2.1 head
        m.ddim_loop("ddim", _x(), torch.zeros(5, 2), torch.zeros(5, 4), 4.0)
    assert not m._engines                                                         # refused before anything was prepared
    assert k22.UNet2DConditionHIP(meta_params=True).chains == 1
