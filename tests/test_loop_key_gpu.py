"""Every operand of the whole-loop entries is in the key of the captured loop.

A captured loop (k22_unet_sample_loop, k22_unet_sample_loop_keep, k22_unet_ddim_loop as DDIM and as PLMS, k22_unet_dpmpp_loop,
k22_prior_sample_loop as the ancestral and as the DDIM sampler) is replayed while "the same buffers and scalars are passed": every pointer
and scalar baked into its nodes is a word of the key it is stored under.  A word missing there is a replay on the OLD operand - a wrong
image and no error.  So, through the C ABI, per entry: one call with use_graph = 1, then ONE operand at a time is exchanged - a pointer
for a buffer at another address (with other contents where the entry reads it), a scalar or a host array for another value - and each
time
    * "loop_captures" rises by exactly one (the exchange was noticed),
    * the outputs equal, bit for bit, those of the same call with use_graph = 0 (what was captured is what the new operands ask for),
    * the same call once more is a replay: no capture, one launch, the same bits.
Pure scratch operands (x_tmp, the sampler scratch, the eps / x0 histories) get the counter assertions only.  The table of a case is total:
an operand it passes non-null without saying how to exchange it fails the test.

Shapes: the tiny fixtures' UNet at 16x16 (CFG batch 2) and 16x24 (inpainting, CFG batch 4), the tiny 2.2 UNet at 16x16, the 512 x 4 prior at
CFG batch 4; 2 steps (PLMS 3: its first step is the two-stage one, the ring rotates after it).  n_steps is exchanged for a SMALLER count:
a larger one would grow the engine's row buffer, which drops the loop on its own."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import kandinsky2_amd as k22
from kandinsky2_amd import _lib, sampling
from kandinsky2_amd.diffusion import percentile_index
from kandinsky2_amd.prior import PriorSchedule

pytestmark = pytest.mark.gpu

F32 = dict(dtype=torch.float32, device="cuda")
SCRATCH, OUTPUT = "scratch", "output"      # what an exchange of a pointer operand means, beside a function tensor -> other contents


def _counters():
    L = _lib.lib()
    return L.k22_debug_counter(b"loop_captures"), L.k22_debug_counter(b"loop_launches")


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _noise(t):
    return _randn(*t.shape, seed=1000 + t.numel() % 997)


def _scaled(t):                # schedule tables: every coefficient a little smaller, all still finite and of the same sign
    return t * (1.0 - 2.0 ** -10)


def _flipped(t):               # 0 / 1 masks
    return 1.0 - t


def _later(t):                 # timesteps
    return t + 1.0


def _ints(v):
    return (C.c_int * len(v))(*v)


# ---- the sweep -------------------------------------------------------------------------------------------------------------------------------
def _sweep(call, ops, exchange, x_T, outputs, only=None):
    """call(ops, use_graph) -> rc on the operand dict `ops` (name -> tensor | scalar | list | None); exchange: name -> SCRATCH | OUTPUT |
    function(tensor) -> tensor of other contents | the other value of a scalar / host array.  ops["x"] is the latent, in and out: every
    run starts from x_T (exchanged with it: the new buffer starts from another x_T)."""
    given = [n for n, v in ops.items() if v is not None]
    assert set(given) - {"x"} <= set(exchange), sorted(set(given) - {"x"} - set(exchange))

    def run(o, xt, use_graph):
        o["x"].copy_(xt)
        assert call(o, use_graph) == 0, _lib.lib().k22_last_error()
        return [t.clone() for t in outputs(o)]

    c, l = _counters()
    run(ops, x_T, 1)
    assert _counters() == (c + 1, l + 1)
    keep_alive = []            # every buffer of the sweep stays allocated: a freed one could hand its address to the next
    for name in given if only is None else only:
        o, xt, how = dict(ops), x_T, exchange.get(name)
        if name == "x":
            o["x"], xt, how = torch.empty_like(ops["x"]), _noise(x_T), None
        elif not torch.is_tensor(ops[name]):
            assert how != ops[name], name
            o[name] = how
        elif how in (SCRATCH, OUTPUT):
            o[name] = torch.empty_like(ops[name])
        else:
            o[name] = how(ops[name]).contiguous()
            assert o[name].shape == ops[name].shape and not torch.equal(o[name], ops[name]), name
        if torch.is_tensor(o[name]):
            assert o[name].data_ptr() != ops[name].data_ptr(), name
            keep_alive.append(o[name])
        c, l = _counters()
        got = run(o, xt, 1)
        assert _counters() == (c + 1, l + 1), f"{name}: exchanged, and the captured loop was not captured again"
        if how != SCRATCH:
            eager = run(o, xt, 0)
            assert _counters() == (c + 1, l + 2), name
            for g, e in zip(got, eager):
                assert torch.isfinite(e).all() and torch.equal(g, e), f"{name}: the captured loop is not the eager loop on the same operands"
        c, l = _counters()
        again = run(o, xt, 1)
        assert _counters() == (c, l + 1), f"{name}: the unchanged call did not replay"
        if how != SCRATCH:
            for g, a in zip(got, again):
                assert torch.equal(g, a), name


# ---- the engines: one per fixture for the whole file -----------------------------------------------------------------------------------------
_UNETS = {}


def _unet21(golden_dir, name):
    """(fixture, module planned at the fixture's shape with its condition set, inpaint_image, inpaint_mask) of a tiny 2.1 fixture"""
    if name not in _UNETS:
        fx = torch.load(os.path.join(golden_dir, name + ".pt"), weights_only=False)
        arch = k22.make_arch(fx["model_config"], inpainting=bool(fx.get("inpainting", False)))
        m = k22.Text2ImUNetHIP(arch, backend_dtype=torch.float32)
        m.load_state_dict(k22.init_unet_state_dict(arch, seed=fx["seed_w"]))
        m = m.to("cuda").eval()
        B, h, w = fx["B"], fx["h"], fx["w"]
        m._ensure_plan(B, h, w)
        m.set_condition(*(t.cuda() for t in k22.make_conditioning(arch, B, seed=2)))
        img = msk = None
        if fx.get("inpainting"):
            msk = (_randn(B, 1, h, w, seed=3) > 0).float()
            img = _randn(B, 4, h, w, seed=4) * msk
        _UNETS[name] = (fx, m, img, msk)
    return _UNETS[name]


def _unet22():
    """the tiny 2.2 inpainting UNet (9 channels) at CFG batch 4, 16x16, its condition set"""
    if "2.2" not in _UNETS:
        arch = k22.make_arch22(k22.tiny_unet22_config(), inpainting=True)
        m = k22.UNet2DConditionHIP(arch, backend_dtype=torch.float32)
        m.load_state_dict(k22.init_unet22_state_dict(arch, seed=0))
        m = m.to("cuda").eval()
        m._ensure_plan(4, 16, 16)
        m.set_condition(_randn(4, arch.image_dim, seed=5))
        _UNETS["2.2"] = m
    return _UNETS["2.2"]


def _ts_rows(values, B):
    return torch.tensor([float(v) for v in values], **F32)[:, None].expand(-1, B).contiguous()


# ---- k22_unet_sample_loop / _keep ------------------------------------------------------------------------------------------------------------
def _call_sample_loop(handle, keep):
    L, st = _lib.lib(), _lib.current_stream()

    def call(o, use_graph):
        head = (handle, _lib.ptr(o["x"]), _lib.ptr(o["x_tmp"]), _lib.ptr(o["timesteps"]), _lib.ptr(o["noise_seq"]), _lib.ptr(o["init_img"]),
                _lib.ptr(o["mask"]), _lib.ptr(o["inpaint_image"]), _lib.ptr(o["inpaint_mask"]), _lib.ptr(o["table"]), _ints(o["table_rows"]),
                o["n_steps"], o["guidance"], o["clamp_lo"], o["clamp_hi"], o["pct_index"], o["pct_gamma"], _lib.ptr(o["scratch"]))
        if not keep:
            return L.k22_unet_sample_loop(*head, use_graph, st)
        coef = np.ascontiguousarray(o["keep_coef"], dtype=np.float32)
        return L.k22_unet_sample_loop_keep(*head, _lib.ptr(o["keep_init"]), _lib.ptr(o["keep_noise"]), _lib.ptr(o["keep_mask"]),
                                           coef.ctypes.data_as(C.POINTER(C.c_float)), use_graph, st)
    return call


SAMPLE_LOOP_EXCHANGE = dict(x_tmp=SCRATCH, timesteps=_later, noise_seq=_noise, init_img=_noise, mask=_flipped, inpaint_image=_noise,
                            inpaint_mask=_flipped, table=_scaled, table_rows=[1, 1], n_steps=1, guidance=3.0, clamp_lo=-1.5, clamp_hi=1.5,
                            pct_gamma=0.25, scratch=SCRATCH)


@pytest.mark.parametrize("name", ["tiny_text2img", "tiny_inpaint"])
def test_sample_loop_key_holds_every_operand(golden_dir, name):
    """tiny_text2img: every operand, the img2img blend (init_img, mask) included; tiny_inpaint: the two operands of the 9-channel UNet"""
    fx, m, img, msk = _unet21(golden_dir, name)
    B, h, w = fx["B"], fx["h"], fx["w"]
    d = k22.create_gaussian_diffusion(**dict(k22.DIFFUSION_CONFIG_2_1, timestep_respacing="2"))
    pct = percentile_index(4 * h * w)
    blend = name == "tiny_text2img"
    ops = dict(x=torch.empty(B, 4, h, w, **F32), x_tmp=torch.empty(B, 4, h, w, **F32), timesteps=_ts_rows(d.model_timesteps()[::-1], B),
               noise_seq=_randn(2, B, 4, h, w, seed=6), init_img=_randn(B, 4, h, w, seed=7) if blend else None,
               mask=(_randn(B, 1, h, w, seed=8) > 0).float() if blend else None, inpaint_image=img, inpaint_mask=msk,
               table=torch.from_numpy(d.step_table()).cuda(), table_rows=[1, 0], n_steps=2, guidance=float(fx["guidance"]), clamp_lo=-2.0,
               clamp_hi=2.0, pct_index=pct[0], pct_gamma=pct[1], scratch=sampling.sampler_scratch(torch.empty(B, 4, h, w, **F32)))
    _sweep(_call_sample_loop(m._handle, False), ops, dict(SAMPLE_LOOP_EXCHANGE, pct_index=pct[0] - 7), _randn(B, 4, h, w, seed=42),
           lambda o: [o["x"]], only=None if blend else ["inpaint_image", "inpaint_mask"])


def test_sample_loop_keep_key_holds_every_operand():
    """the 2.2 inpainting decoder's loop: the keep operands and their host coefficients beside everything k22_unet_sample_loop takes"""
    m = _unet22()
    B, h, w = 4, 16, 16
    sch = k22.DDPMSchedulerHIP.from_config(k22.SCHEDULER_CONFIG_2_2).set_timesteps(2, device="cuda")
    ts, rows, coef = sampling.ddpm_loop_operands(sch, sch.timesteps.tolist(), B, keep=True)
    msk = (_randn(B, 1, h, w, seed=3) > 0).float()
    clip = min(float(sch.clip), 3.0e38)      # this scheduler does not clip: the decoder passes the largest finite bound
    ops = dict(x=torch.empty(B, 4, h, w, **F32), x_tmp=torch.empty(B, 4, h, w, **F32), timesteps=ts.cuda(), noise_seq=_randn(2, B, 4, h, w, seed=6),
               init_img=None, mask=None, inpaint_image=_randn(B, 4, h, w, seed=4) * msk, inpaint_mask=msk, table=sch._table.float().contiguous(),
               table_rows=[int(r) for r in rows], n_steps=2, guidance=4.0, clamp_lo=-clip, clamp_hi=clip, pct_index=-1,
               pct_gamma=0.0, scratch=sampling.sampler_scratch(torch.empty(B, 4, h, w, **F32)), keep_init=_randn(4, h, w, seed=9),
               keep_noise=_randn(B // 2, 4, h, w, seed=10), keep_mask=(_randn(h, w, seed=11) > 0).float(), keep_coef=[float(v) for v in coef.ravel()])
    other_coef = list(ops["keep_coef"])
    other_coef[1] *= 0.5                 # the noise share of the first step
    rows2 = [ops["table_rows"][0]] * 2
    exchange = dict(SAMPLE_LOOP_EXCHANGE, table_rows=rows2, pct_index=5,
                    keep_init=_noise, keep_noise=_noise, keep_mask=_flipped, keep_coef=other_coef)
    _sweep(_call_sample_loop(m._handle, True), ops, exchange, _randn(B, 4, h, w, seed=42), lambda o: [o["x"]])


# ---- k22_unet_ddim_loop ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddim", "plms"])
@pytest.mark.parametrize("name", ["tiny_text2img", "tiny_inpaint"])
def test_ddim_loop_key_holds_every_operand(golden_dir, name, kind):
    """DDIM at eta = 1 (noise_seq given), PLMS with its eps history; tiny_inpaint: the two operands of the 9-channel UNet"""
    fx, m, img, msk = _unet21(golden_dir, name)
    B, h, w = fx["B"], fx["h"], fx["w"]
    plms = kind == "plms"
    n = 3 if plms else 2
    sm = k22.DDIMSamplerHIP(m, k22.create_gaussian_diffusion(**k22.DIFFUSION_CONFIG_2_1), fx["guidance"])
    if plms:
        sm.make_schedule(4, init_step=501)          # the last three of 1, 251, 501, 751
    else:
        sm.make_schedule(2, ddim_eta=1.0)
    assert len(sm.ddim_timesteps) == n
    tr = [float(t) for t in sm.ddim_timesteps[::-1]]
    box = (B, 4, h, w)
    ops = dict(x=torch.empty(*box, **F32), x_tmp=torch.empty(*box, **F32), x0_out=torch.empty(*box, **F32),
               timesteps=_ts_rows([tr[0], tr[1]] + tr[1:] if plms else tr, B), table=torch.from_numpy(sm.table[::-1].copy()).cuda(),
               noise_seq=None if plms else _randn(n, *box, seed=6), inpaint_image=img, inpaint_mask=msk,
               eps_hist=torch.empty(4, *box, **F32) if plms else None, n_steps=n, guidance=float(fx["guidance"]))
    code = _lib.K22_LOOP_PLMS if plms else _lib.K22_LOOP_DDIM
    L, st = _lib.lib(), _lib.current_stream()

    def call(o, use_graph):
        return L.k22_unet_ddim_loop(m._handle, code, _lib.ptr(o["x"]), _lib.ptr(o["x_tmp"]), _lib.ptr(o["x0_out"]), _lib.ptr(o["timesteps"]),
                                    _lib.ptr(o["table"]), _lib.ptr(o["noise_seq"]), _lib.ptr(o["inpaint_image"]), _lib.ptr(o["inpaint_mask"]),
                                    _lib.ptr(o["eps_hist"]), o["n_steps"], o["guidance"], use_graph, st)

    exchange = dict(x_tmp=SCRATCH, x0_out=OUTPUT, timesteps=_later, table=_scaled, noise_seq=_noise, inpaint_image=_noise, inpaint_mask=_flipped,
                    eps_hist=SCRATCH, n_steps=n - 1, guidance=3.0)
    _sweep(call, ops, exchange, _randn(*box, seed=42), lambda o: [o["x"], o["x0_out"]],
           only=None if name == "tiny_text2img" else ["inpaint_image", "inpaint_mask"])


# ---- k22_unet_dpmpp_loop ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_text2img", "tiny_inpaint"])
def test_dpmpp_loop_key_holds_every_operand(golden_dir, name):
    """orders (1, 1) exchanged for (1, 2): the second step then reads the first one's x0 from the ring"""
    fx, m, img, msk = _unet21(golden_dir, name)
    B, h, w = fx["B"], fx["h"], fx["w"]
    sm = k22.DPMSolverSamplerHIP(m, k22.create_gaussian_diffusion(**k22.DIFFUSION_CONFIG_2_1), fx["guidance"])
    sm.make_dpm_schedule(2)
    assert len(sm.timesteps) == 2 and [int(o) for o in sm.orders] == [1, 1]
    box = (B, 4, h, w)
    ops = dict(x=torch.empty(*box, **F32), x_tmp=torch.empty(*box, **F32), x0_hist=torch.empty(2, *box, **F32), timesteps=_ts_rows(sm.timesteps, B),
               table=torch.from_numpy(sm.dpm_table.astype(np.float32)).cuda(), orders=[1, 1], inpaint_image=img, inpaint_mask=msk, n_steps=2,
               guidance=float(fx["guidance"]))
    L, st = _lib.lib(), _lib.current_stream()

    def call(o, use_graph):
        return L.k22_unet_dpmpp_loop(m._handle, _lib.ptr(o["x"]), _lib.ptr(o["x_tmp"]), _lib.ptr(o["x0_hist"]), _lib.ptr(o["timesteps"]),
                                     _lib.ptr(o["table"]), _ints(o["orders"]), _lib.ptr(o["inpaint_image"]), _lib.ptr(o["inpaint_mask"]), o["n_steps"],
                                     o["guidance"], use_graph, st)

    exchange = dict(x_tmp=SCRATCH, x0_hist=SCRATCH, timesteps=_later, table=_scaled, orders=[1, 2], inpaint_image=_noise, inpaint_mask=_flipped,
                    n_steps=1, guidance=3.0)
    _sweep(call, ops, exchange, _randn(*box, seed=42), lambda o: [o["x"]], only=None if name == "tiny_text2img" else ["inpaint_image", "inpaint_mask"])


# ---- k22_prior_sample_loop -------------------------------------------------------------------------------------------------------------------
_PRIOR = {}


def _prior(golden_dir):
    if not _PRIOR:
        fx = torch.load(os.path.join(golden_dir, "prior_tiny_ddim.pt"), weights_only=False)
        g = torch.Generator().manual_seed(7)
        cm, cs = torch.randn(768, generator=g) * 0.1, torch.rand(768, generator=g) + 0.5
        m = k22.PriorDiffusionModelHIP(fx["hp"], k22.PRIOR_DIFFUSION_2_1, cm, cs, backend_dtype=torch.float32)
        m.load_state_dict(k22.init_prior_state_dict(fx["hp"], seed=fx["seed_w"]))
        m = m.to("cuda")
        m._ensure_plan(4)
        _PRIOR["m"] = m
    return _PRIOR["m"]


def _one_key_fewer(t):         # key_valid: the longest prompt loses its last token (every row keeps a valid one)
    t = t.clone()
    t[1, 19] = 0.0
    return t


@pytest.mark.parametrize("kind", ["ancestral", "ddim"])
def test_prior_sample_loop_key_holds_every_operand(golden_dir, kind):
    """CFG batch 4 (bs 2); the DDIM loop at eta = 1 with noise_seq and x0_out given.  clamp is exchanged for one that bites."""
    m = _prior(golden_dir)
    N, D, nt = 4, int(m.hp["clip_dim"]), int(m.hp["text_ctx"])
    ddim = kind == "ddim"
    sched = PriorSchedule(**dict(k22.PRIOR_DIFFUSION_2_1, timestep_respacing="ddim2" if ddim else "2"), eta=1.0)
    T = sched.num_timesteps
    tab = sched.ddim_table() if ddim else sched.step_table()
    valid = torch.zeros(N, nt, **F32)
    valid[0, :9] = 1.0
    valid[1, :20] = 1.0
    valid[2:, :2] = 1.0
    ops = dict(x=torch.empty(N, D, **F32), x_tmp=torch.empty(N, D, **F32), x0_out=torch.empty(N, D, **F32) if ddim else None,
               timesteps=_ts_rows(sched.timestep_map[::-1], N), table=torch.from_numpy(np.ascontiguousarray(tab[::-1], dtype=np.float32)).cuda(),
               noise_seq=_randn(T, N, D, seed=6), scales=torch.tensor([4.0, 2.5], **F32), text_emb=_randn(N, D, seed=12),
               text_enc=_randn(N, nt, int(m.hp["clip_xf_width"]), seed=13), key_valid=valid, clamp=10.0, n_steps=T)
    code = _lib.K22_PRIOR_LOOP_DDIM if ddim else _lib.K22_PRIOR_LOOP_ANCESTRAL
    L, st = _lib.lib(), _lib.current_stream()

    def call(o, use_graph):
        return L.k22_prior_sample_loop(m._handle, code, _lib.ptr(o["x"]), _lib.ptr(o["x_tmp"]), _lib.ptr(o["x0_out"]), _lib.ptr(o["timesteps"]),
                                       _lib.ptr(o["table"]), _lib.ptr(o["noise_seq"]), _lib.ptr(o["scales"]), _lib.ptr(o["text_emb"]),
                                       _lib.ptr(o["text_enc"]), _lib.ptr(o["key_valid"]), o["clamp"], o["n_steps"], use_graph, st)

    exchange = dict(x_tmp=SCRATCH, x0_out=OUTPUT, timesteps=_later, table=_scaled, noise_seq=_noise, scales=lambda t: t + 1.0, text_emb=_noise,
                    text_enc=_noise, key_valid=_one_key_fewer, clamp=0.5, n_steps=T - 1)
    _sweep(call, ops, exchange, _randn(N, D, seed=42), lambda o: [o["x"]] + ([o["x0_out"]] if ddim else []))
