"""The engines under every switch INTEGRATION.md section G documents and no other test sets: K22_FUSE_SKIP=0, K22_X2_PLAN=1..3, K22_STREAM=0
(with the weight-streaming wiring it removes switched ON through the tile table) and K22_PRIOR_SKINNY=0 - each against the CPU oracle /
the reference golden within the bound the default route's own test uses, and each with proof that the alternate route is the one that ran
(op counts, tuning-report lines, the "stream_launches" / "loop_captures" counters, or differing bits): a switch that silently did nothing
would pass any parity test.

Shapes: the tiny 2.1 UNet (1/3 width) at B = 2, 16x16 and at the ragged B = 3, 40x8 (bottom level 5x1, odd batch: the m-tiles of the
unfused skip GEMM straddle image ends); the tiny 2.2 UNet at B = 2, 16x16 and B = 3, 16x24; the 512 x 4 prior of prior_tiny.pt.  Inputs and
weights are those of test_forward_ragged_shapes_vs_oracle (2.1), test_up2_phase_gpu.py (2.2) and test_prior_gpu.py (prior).  The oracle
result and the default-route result are computed once per (backend, shape) and shared.  K22_AUTOTUNE=0 everywhere except the one engine of
section 3 that measures.  A refusal on the host (k22 error -1 / -3) fails the item; any other runtime error ends the session.

MEASURED on the MI355X (max-abs, of the oracle's / golden's output scale; the file's 38 items run in 11 s, the slowest 1.5 s - the first
engine's start-up; no item had to be split):

1. K22_FUSE_SKIP=0.  Every item: ops 242 -> 261 (all 19 skip weights become a GEMM of their own, also at the 2x2 and 5x1 levels),
   taps-1 ops 66 -> 85, 13 new taps-1 problems at 2x16x16.  Whole-loop graph = stepwise loop in bits (fp32, bf16); loop_captures +1 then +0.
       engine  shape      alt vs oracle   default vs oracle   max|alt - default|
   2.1 fp32    2x16x16    1.38e-6         1.09e-6             9.7e-7
       fp32    3x40x8     1.19e-6         1.50e-6             1.03e-6
       f16x3   2x16x16    1.05e-6         9.5e-7              6.2e-7
       f16x3   3x40x8     1.24e-6         1.24e-6             7.0e-7
       f16x2   2x16x16    1.79e-4         2.49e-4             1.85e-4
       f16x2   3x40x8     2.00e-4         1.94e-4             1.56e-4
       fp16    2x16x16    1.16e-3         1.08e-3             1.11e-3
       fp16    3x40x8     1.26e-3         1.12e-3             1.08e-3
       bf16    2x16x16    8.33e-3         9.46e-3             8.50e-3
       bf16    3x40x8     1.03e-2         7.36e-3             7.52e-3
   2.2 fp32    2x16x16    1.49e-6         1.34e-6             1.13e-6
       fp32    3x16x24    1.55e-6         1.34e-6             1.20e-6
       bf16    2x16x16    9.97e-3         9.37e-3             9.62e-3
       bf16    3x16x24    8.26e-3         7.51e-3             8.24e-3
2. K22_X2_PLAN (f16x2 engine), vs oracle at 2x16x16 / 3x40x8; the fp16 engine on the same inputs 1.08e-3 / 1.12e-3:
       plan 0  2.49e-4 / 1.94e-4     plan 1  2.75e-4 / 3.39e-4     plan 2  3.36e-4 / 2.95e-4     plan 3  4.34e-4 / 3.64e-4
   and vs plan 0: plan 1 3.1e-4 / 3.2e-4, plan 2 3.4e-4 / 4.1e-4, plan 3 4.3e-4 / 4.2e-4, plan 4 0 (the bits of plan 0).  Beside DESIGN
   section 3's final-latent figures at C2 (plan 0 2.7e-4, 1 5.3e-4, 2 4.6e-4, 3 5.8e-4): the same order, plans 1 and 2 close together.
3. Weight streaming (bf16, 2x16x16).  The measuring engine: 0.1 s for creation + the measuring first forward (K22_TUNE_REPS=2).  18 table
   lines of the plan rewritten to algo 20 (6 of them with a fused skip, bm 160 and 288, split-K 1 to 5; 4 of the 18 named the streaming
   kernel already: the shipped table holds lines for these 8x8 problems, so the default plan streams 5 ops at this size).  On:
   stream_launches +33 per forward (= the 33 ops on streaming lines), +33 again after the re-bind into a workspace filled with 0xFF;
   workspace 54 222 592 B; 8.86e-3 of scale.  K22_STREAM=0 under the same table: +0 launches, 21 870 336 B (default and heuristics-only
   engines: 34 758 400 B), 8.75e-3 of scale, 7.96e-3 from the streaming engine.
4. K22_PRIOR_SKINNY=0: tuned ops 0 -> 16, the c_fc line taps 1, M 324, N 2048, K 512 x4.
       bf16  alt vs golden 4.66e-3   default 5.72e-3   max|alt - default| 3.46e-3
       fp16  alt vs golden 6.16e-4   default 6.93e-4   max|alt - default| 4.86e-4    (2^-11: half an fp16 ulp at the scale - the routes
                                                                                      differ at the fp16-ulp level DESIGN's prior section names)
   k22_prior_sample_loop = the host-stepped loop in bits (ddim5, eta 1) for both.

Sensitivity (not committed): a build whose unfused skip GEMM loses its bias gives 1.2e-2 .. 2.2e-2 of scale on every item of section 1 -
the fp32, f16x3, f16x2 and fp16 items of the 2.1 UNet and the fp32 items of the 2.2 UNet fail (10 of 14); the four bf16 items stay inside
their 2e-2 / 2.5e-2, which is why the fp32 and f16x3 items are the sharp ones.
"""
import os
import time

import pytest
import torch

import helpers as hp
import kandinsky2_amd as k22
from kandinsky2_amd import _lib
from oracle import unet22_ref, unet_ref

pytestmark = pytest.mark.gpu

# the switches this file owns (tests/test_engine_switches_cpu.py reads this tuple: every one of them is set by an item below)
SWITCHES = ("K22_FUSE_SKIP", "K22_X2_PLAN", "K22_STREAM", "K22_PRIOR_SKINNY")


def _counter(name):
    return _lib.lib().k22_debug_counter(name.encode())


def _guard(what, fn):
    """runs a step that launches: a host refusal fails the item, any other runtime error ends the session (nothing more may run on a
    device that has faulted)"""
    try:
        return fn()
    except RuntimeError as e:
        if hp.host_refusal(e):
            pytest.fail(f"{what}: refused on the host: {e}")
        pytest.exit(f"{what}: {e}", returncode=3)


def _env(mp, autotune="0", **switches):
    """K22_AUTOTUNE and exactly the given switches of this file; the others unset"""
    for s in SWITCHES:
        mp.delenv(s, raising=False)
    mp.setenv("K22_AUTOTUNE", autotune)
    for s, v in switches.items():
        assert s in SWITCHES
        mp.setenv(s, str(v))


class Run:
    """what one engine under one environment left behind"""
    def __init__(self, m, out):
        self.m, self.out = m, out
        self.ops, self.report, self.ws = m.num_ops(), m.tuning_report(), m.workspace_bytes()


# ---- the two UNets: inputs, oracle and default route once per (backend, shape) -----------------------------------------------------------
_IN, _ORACLE, _DEFAULT = {}, {}, {}


def _inputs(kind, B, h, w):
    key = (kind, B, h, w)
    if key not in _IN:
        if kind == "21":
            arch = k22.make_arch(k22.tiny_model_config())
            sd = k22.init_unet_state_dict(arch, seed=13)
            full, pooled, image = k22.make_conditioning(arch, B, seed=6)
            g = torch.Generator().manual_seed(10 + h)
            x, t = torch.randn(B, 4, h, w, generator=g), torch.tensor([999.0, 3.0, 480.0][:B])
            _IN[key] = dict(arch=arch, sd=sd, x=x, t=t, cond=(full, pooled, image), n_skip=sum(k.endswith(".skip_connection.weight") for k in sd))
        else:
            cfg = k22.tiny_unet22_config()
            arch = k22.make_arch22(cfg, controlnet=False)
            sd = k22.init_unet22_state_dict(arch, seed=0)
            g = torch.Generator().manual_seed(4)
            x, emb, t = torch.randn(B, 4, h, w, generator=g), torch.randn(B, 1280, generator=g), torch.tensor([980.0, 20.0, 500.0][:B])
            # diffusers' name of the ResBlock's 1x1 skip_connection (unet22.py)
            _IN[key] = dict(cfg=cfg, arch=arch, sd=sd, x=x, t=t, emb=emb, n_skip=sum(k.endswith(".conv_shortcut.weight") for k in sd))
    return _IN[key]


def _oracle(kind, B, h, w):
    key = (kind, B, h, w)
    if key not in _ORACLE:
        i = _inputs(*key)
        _ORACLE[key] = unet_ref.unet_forward(i["sd"], i["arch"], i["x"], i["t"], *i["cond"]) if kind == "21" else \
            unet22_ref.unet22_forward(i["sd"], i["cfg"], i["x"], i["t"], i["emb"], None)
    return _ORACLE[key]


def _forward(kind, m, i):
    if kind == "21":
        full, pooled, image = i["cond"]
        return m(i["x"].cuda(), i["t"].cuda(), full_emb=full.cuda(), pooled_emb=pooled.cuda(), image_emb=image.cuda()).cpu()
    return m(sample=i["x"].cuda(), timestep=i["t"].cuda(), encoder_hidden_states=None, added_cond_kwargs={"image_embeds": i["emb"].cuda()},
             return_dict=False)[0].cpu()


def _engine(kind, backend, B, h, w, use_graph=False):
    """a new module and its first forward, under the environment as it stands (switches are read when the engine is created / planned)"""
    i = _inputs(kind, B, h, w)
    cls = k22.Text2ImUNetHIP if kind == "21" else k22.UNet2DConditionHIP
    m = cls(i["arch"], backend_dtype=backend, use_graph=use_graph)
    m.load_state_dict(i["sd"])
    m = m.to("cuda").eval()
    out = _guard(f"{kind} {backend} {B}x{h}x{w} forward", lambda: _forward(kind, m, i))
    return Run(m, out)


def _default(mp, kind, backend, B, h, w):
    key = (kind, str(backend), B, h, w)
    if key not in _DEFAULT:
        _env(mp)
        r = _engine(kind, backend, B, h, w)
        r.m = None           # the numbers are kept, the engine is not
        _DEFAULT[key] = r
    return _DEFAULT[key]


def _err(out, ref):
    return (out - ref).abs().max().item() / ref.abs().max().item()


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


SHAPES21 = [(2, 16, 16), (3, 40, 8)]
SHAPES22 = [(2, 16, 16), (3, 16, 24)]
IDS = lambda shapes: [f"{B}x{h}x{w}" for B, h, w in shapes]   # noqa: E731
# test_forward_ragged_shapes_vs_oracle's bounds (2.1), test_unet22_forward_vs_oracle's (2.2)
TOL21 = [(torch.float32, 2e-5), ("f16x3", 2e-5), ("f16x2", 5e-4), (torch.float16, 2.5e-3), (torch.bfloat16, 2e-2)]
TOL22 = [(torch.float32, 2e-4), (torch.bfloat16, 2.5e-2)]


# ---- 1. K22_FUSE_SKIP=0 ---------------------------------------------------------------------------------------------------------------
def _fuse_skip_item(mp, kind, backend, tol, B, h, w):
    ref, i = _oracle(kind, B, h, w), _inputs(kind, B, h, w)
    dflt = _default(mp, kind, backend, B, h, w)
    _env(mp, K22_FUSE_SKIP=0)
    alt = _engine(kind, backend, B, h, w)
    e_d, e_a, d = _err(dflt.out, ref), _err(alt.out, ref), (alt.out - dflt.out).abs().max().item() / ref.abs().max().item()
    gained = hp.report_problems(alt.report, 1) - hp.report_problems(dflt.report, 1)
    n1 = lambda r: sum(x.count for x in hp.report_lines(r.report) if x.taps == 1)   # noqa: E731
    print(f"K22_FUSE_SKIP=0 {kind} {backend} {B}x{h}x{w}: vs oracle {e_a:.3e} (default route {e_d:.3e}), max|alt - default| / scale {d:.3e}; "
          f"ops {dflt.ops} -> {alt.ops} (skip weights {i['n_skip']}), taps-1 ops {n1(dflt)} -> {n1(alt)}, new taps-1 problems {sorted(gained)}")
    assert torch.isfinite(alt.out).all() and e_a <= tol and e_d <= tol
    assert 1 <= alt.ops - dflt.ops <= i["n_skip"]
    assert gained and n1(alt) - n1(dflt) == alt.ops - dflt.ops          # what was added are GEMMs, one op each
    assert all(K != N for (_M, N, K, _H, _W) in gained)                  # (a skip_connection exists only where the channels change)
    assert d <= 2 * tol                                                  # no more than the two oracle bounds imply


@pytest.mark.parametrize("B,h,w", SHAPES21, ids=IDS(SHAPES21))
@pytest.mark.parametrize("backend,tol", TOL21, ids=[str(b).replace("torch.", "") for b, _ in TOL21])
def test_fuse_skip_off_unet21(backend, tol, B, h, w, monkeypatch):
    _fuse_skip_item(monkeypatch, "21", backend, tol, B, h, w)


@pytest.mark.parametrize("B,h,w", SHAPES22, ids=IDS(SHAPES22))
@pytest.mark.parametrize("backend,tol", TOL22, ids=[str(b).replace("torch.", "") for b, _ in TOL22])
def test_fuse_skip_off_unet22(backend, tol, B, h, w, monkeypatch):
    _fuse_skip_item(monkeypatch, "22", backend, tol, B, h, w)


@pytest.mark.parametrize("backend", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_fuse_skip_off_whole_loop_graph_equals_the_stepwise_loop_bit_for_bit(golden_dir, backend, monkeypatch):
    """test_whole_loop_graph_equals_the_stepwise_loop_bit_for_bit's comparison on tiny_text2img's inputs with the unfused skip GEMMs in
    the captured loop; a second whole-loop call replays the capture"""
    fx = torch.load(os.path.join(golden_dir, "tiny_text2img.pt"), weights_only=False)
    dflt = _default(monkeypatch, "21", backend, 2, 16, 16)
    _env(monkeypatch, K22_FUSE_SKIP=0)
    arch = k22.make_arch(fx["model_config"])
    m = k22.Text2ImUNetHIP(arch, backend_dtype=backend, use_graph=True)
    m.load_state_dict(k22.init_unet_state_dict(arch, seed=fx["seed_w"]))
    m = m.to("cuda").eval()
    full, pooled, image = k22.make_conditioning(arch, fx["B"], seed=2)
    kw = dict(full_emb=full.cuda(), pooled_emb=pooled.cuda(), image_emb=image.cuda())
    d = k22.create_gaussian_diffusion(**dict(k22.DIFFUSION_CONFIG_2_1, timestep_respacing=str(fx["steps"])))
    shape = (fx["B"], 4, fx["h"], fx["w"])
    assert shape == (2, 4, 16, 16)
    g = torch.Generator().manual_seed(42)
    x_T, noise_seq = torch.randn(*shape, generator=g).cuda(), torch.randn(fx["steps"], *shape, generator=g).cuda()
    loop = lambda whole: d.p_sample_loop(m, shape, model_kwargs=kw, guidance_scale=fx["guidance"], noise=x_T, noise_seq=noise_seq,   # noqa: E731
                                         whole_loop_graph=whole)
    step = _guard("stepwise loop", lambda: loop(False))
    assert m.num_ops() > dflt.ops                      # the unfused route is the one in this engine
    m.del_cache()
    c0, l0 = _counter("loop_captures"), _counter("loop_launches")
    whole = _guard("whole loop", lambda: loop(True))
    c1, l1 = _counter("loop_captures"), _counter("loop_launches")
    m.del_cache()
    again = _guard("whole loop, second call", lambda: loop(True))
    c2, l2 = _counter("loop_captures"), _counter("loop_launches")
    print(f"K22_FUSE_SKIP=0 loop {backend}: ops {m.num_ops()} (default {dflt.ops}); loop_captures {c0} -> {c1} -> {c2}, loop_launches {l0} -> {l1} -> {l2}")
    assert torch.isfinite(whole).all() and torch.equal(whole, step), (whole - step).abs().max().item()
    assert torch.equal(again, whole)
    assert (c1 - c0, l1 - l0) == (1, 1) and (c2 - c1, l2 - l1) == (0, 1)


# ---- 2. K22_X2_PLAN ---------------------------------------------------------------------------------------------------------------------
# max|out - oracle| / scale of the f16x2 engine per plan, the worst of SHAPES21 as measured on the MI355X (K22_AUTOTUNE=0; the docstring
# holds both shapes).  The ceiling of a plan is twice its value (the convention of test_unet_gpu.py's docstring); plan 0 keeps 5e-4.
X2_MEASURED = {0: 2.485e-4, 1: 3.394e-4, 2: 3.362e-4, 3: 4.341e-4}
_PLAN = {}


def _plan_run(mp, backend, plan, B, h, w):
    key = (str(backend), plan, B, h, w)
    if key not in _PLAN:
        _env(mp, **({} if plan is None else {"K22_X2_PLAN": plan}))
        r = _engine("21", backend, B, h, w)
        r.m = None
        _PLAN[key] = r
    return _PLAN[key]


@pytest.mark.parametrize("B,h,w", SHAPES21, ids=IDS(SHAPES21))
def test_x2_plans_differ_in_bits_and_the_value_is_masked(B, h, w, monkeypatch):
    o = {p: _plan_run(monkeypatch, "f16x2", p, B, h, w).out for p in (0, 1, 2, 3, 4, None)}
    ref = _oracle("21", B, h, w)
    print(f"K22_X2_PLAN {B}x{h}x{w}: " + ", ".join(f"plan {p} vs plan 0 {_err(o[p], o[0]):.3e}" for p in (1, 2, 3, 4)) +
          f" (of plan 0's scale); vs oracle " + ", ".join(f"{p}: {_err(o[p], ref):.3e}" for p in (0, 1, 2, 3)))
    for p in (1, 2, 3):
        assert not _bits_equal(o[p], o[0]), f"plan {p} gives plan 0's bits: the switch did nothing"
    assert not _bits_equal(o[3], o[1]) and not _bits_equal(o[3], o[2]) and not _bits_equal(o[1], o[2])
    assert _bits_equal(o[4], o[0])                     # the code masks with & 3
    assert _bits_equal(o[None], o[0])                  # unset = plan 0
    assert _bits_equal(o[None], _default(monkeypatch, "21", "f16x2", B, h, w).out)     # (and two engines of one plan agree)


@pytest.mark.parametrize("B,h,w", SHAPES21, ids=IDS(SHAPES21))
@pytest.mark.parametrize("backend", [torch.bfloat16, "f16x3"], ids=["bfloat16", "f16x3"])
def test_x2_plan_leaves_the_other_backends_alone(backend, B, h, w, monkeypatch):
    """conv_dt returns the engine's own dtype for every arithmetic but f16x2"""
    with_plan = _plan_run(monkeypatch, backend, 3, B, h, w)
    dflt = _default(monkeypatch, "21", backend, B, h, w)
    assert _bits_equal(with_plan.out, dflt.out) and with_plan.ops == dflt.ops and with_plan.report == dflt.report


@pytest.mark.parametrize("B,h,w", SHAPES21, ids=IDS(SHAPES21))
@pytest.mark.parametrize("plan", [0, 1, 2, 3])
def test_x2_plan_error_against_the_oracle(plan, B, h, w, monkeypatch):
    ref = _oracle("21", B, h, w)
    e = _err(_plan_run(monkeypatch, "f16x2", plan, B, h, w).out, ref)
    e16 = _err(_default(monkeypatch, "21", torch.float16, B, h, w).out, ref)
    ceiling = 5e-4 if plan == 0 else 2 * X2_MEASURED[plan]
    print(f"K22_X2_PLAN={plan} {B}x{h}x{w}: vs oracle {e:.3e} of scale (fp16 engine {e16:.3e}; ceiling {ceiling:.3e})")
    assert e16 <= 2.5e-3                               # (the fp16 engine inside its own bound: the yardstick is a valid one)
    assert e <= e16, "an x2 plan must beat the fp16 engine (DESIGN section 3)"
    assert e <= ceiling


# ---- 3. the engine's weight-streaming wiring, on (through the tile table) and off (K22_STREAM=0) ---------------------------------------
BF16 = _lib.K22_BF16
ALGO_STREAM = 20


@pytest.fixture(scope="module")
def streaming(tmp_path_factory):
    """One pass over the whole experiment (bf16, 2.1 UNet, B = 2, 16x16); the tests below assert on what it observed.
    measure -> save -> rewrite this plan's eligible conv lines to streaming candidates -> load -> engine ON, engine with K22_STREAM=0 ->
    (finally) load the unmodified file again -> save once more, an engine from the reloaded table."""
    tmp = tmp_path_factory.mktemp("tiles")
    L = _lib.lib()
    B, h, w = 2, 16, 16
    i = _inputs("21", B, h, w)
    obs = {}
    fwd = lambda r, what: _guard(what, lambda: _forward("21", r.m, i))   # noqa: E731
    with pytest.MonkeyPatch.context() as mp:
        _env(mp)
        obs["plain"] = _engine("21", torch.bfloat16, B, h, w)            # K22_AUTOTUNE=0 before anything of this plan was measured
        _env(mp, autotune="1")
        t0 = time.time()
        tuner = _engine("21", torch.bfloat16, B, h, w)
        obs["measure_seconds"] = time.time() - t0
        obs["tuner"] = tuner
        saved, rewritten, saved2 = (str(tmp / n) for n in ("measured.txt", "streaming.txt", "measured_again.txt"))
        assert L.k22_tile_table_save(saved.encode()) > 0
        lines, text = hp.read_tile_table(saved), hp.tile_table_text_lines(saved)
        assert len(lines) == len(text)
        mine = hp.report_problems(tuner.report, 9)                        # the 3x3 convolutions of THIS plan
        new_text, changed = [], []
        for t, ln in zip(lines, text):
            if t.dtype == BF16 and t.taps == 9 and t.M <= 1152 and (t.M, t.N, t.Kc, t.H, t.W) in mine:
                cands = sorted(c for c in hp.igemm_candidates(t, BF16, 1)[0] if c[0] == ALGO_STREAM)
                if cands:
                    c = cands[len(changed) % len(cands)]                  # both m-block counts and several split-K factors get their turn
                    changed.append((t, c))
                    ln = hp.tile_table_text_with_cfg(ln, c)
            new_text.append(ln)
        with open(rewritten, "w") as f:
            f.writelines(new_text)
        obs["changed"] = changed
        try:
            assert L.k22_tile_table_load(rewritten.encode()) == len(lines)
            _env(mp)
            on = _engine("21", torch.bfloat16, B, h, w)
            c0 = _counter("stream_launches")
            o2 = fwd(on, "streaming on, second forward")
            c1 = _counter("stream_launches")
            o3 = fwd(on, "streaming on, third forward")
            c2 = _counter("stream_launches")
            # a second workspace for the same plan (tests/test_lifecycle_gpu.py): the fragment-major copies must be written again
            old_ws = on.m._ws
            ws = torch.full_like(old_ws, 0xFF)                            # NaN patterns where the copies will live: a missing repack shows
            _lib.check(L.k22_unet_bind(on.m._handle, (ws.data_ptr() + 255) // 256 * 256, old_ws.numel() - 256))
            on.m._ws, on.m._cond_key = ws, None
            old_ws.fill_(0xFF)                                            # and nothing may still read the old one
            o4 = fwd(on, "streaming on, forward after a re-bind")
            c3 = _counter("stream_launches")
            obs.update(on=on, on_outs=(on.out, o2, o3, o4), on_counts=(c0, c1, c2, c3))
            _env(mp, K22_STREAM=0)
            c4 = _counter("stream_launches")
            obs["off"] = _engine("21", torch.bfloat16, B, h, w)
            obs["off_second"] = fwd(obs["off"], "K22_STREAM=0, second forward")
            obs["off_counts"] = (c4, _counter("stream_launches"))
        finally:
            assert L.k22_tile_table_load(saved.encode()) == len(lines)    # the rest of the process sees what it had
        assert L.k22_tile_table_save(saved2.encode()) == len(lines)
        obs["round_trip"] = (lines, hp.read_tile_table(saved2))
        _env(mp)
        obs["again"] = _engine("21", torch.bfloat16, B, h, w)            # from the reloaded table: the default engine of this plan
    return obs


def test_streaming_lines_were_rewritten(streaming):
    ch = streaming["changed"]
    print(f"autotuned engine: {streaming['measure_seconds']:.1f} s for creation + measuring first forward; {len(ch)} lines rewritten: " +
          "; ".join(f"{hp.tile_id(t)} -> {c}" for t, c in ch))
    assert len(ch) >= 2 and any(t.sk_total > 0 for t, _ in ch)          # the fused skip's second fragment-major copy is covered
    assert any(c[1] == 160 for _, c in ch) and any(c[3] > 1 for _, c in ch)


def test_streaming_on_runs_the_kernel_and_survives_a_rebind(streaming):
    on, (o1, o2, o3, o4), (c0, c1, c2, c3) = streaming["on"], streaming["on_outs"], streaming["on_counts"]
    ref = _oracle("21", 2, 16, 16)
    n_stream = sum(r.count for r in hp.report_lines(on.report) if r.taps == 9 and r.bm in (160, 288))
    print(f"streaming on: stream_launches per forward {c1 - c0}, {c2 - c1}, after re-bind {c3 - c2} (report: {n_stream} ops on streaming lines); "
          f"workspace {on.ws} B (K22_STREAM=0 {streaming['off'].ws} B, default {streaming['again'].ws} B); vs oracle {_err(o1, ref):.3e} of scale")
    assert c1 - c0 > 0 and c2 - c1 == c1 - c0 and c3 - c2 == c1 - c0
    assert c1 - c0 == n_stream
    assert on.ws > streaming["off"].ws
    assert torch.isfinite(o1).all() and _err(o1, ref) <= 2e-2
    assert _bits_equal(o1, o2) and _bits_equal(o2, o3)
    assert _bits_equal(o4, o1), "the forward after a re-bind differs: the fragment-major copies were not rewritten"


def test_stream_off_removes_the_kernel_and_the_copies(streaming):
    off, (c0, c1) = streaming["off"], streaming["off_counts"]
    ref = _oracle("21", 2, 16, 16)
    print(f"K22_STREAM=0 under the streaming table: stream_launches {c0} -> {c1}; workspace {off.ws} B (default {streaming['again'].ws} B, "
          f"heuristics only {streaming['plain'].ws} B); vs oracle {_err(off.out, ref):.3e} of scale, vs streaming on "
          f"{_err(off.out, streaming['on'].out):.3e}")
    assert c1 == c0
    assert not any(r.taps == 9 and r.bm in (160, 288) for r in hp.report_lines(off.report))
    assert off.ws <= streaming["again"].ws
    assert torch.isfinite(off.out).all() and _err(off.out, ref) <= 2e-2 and _bits_equal(off.out, streaming["off_second"])


def test_tile_table_round_trip_reproduces_the_measured_engine(streaming):
    """save -> load -> save gives the same lines (what K22_TUNE_CACHE persists), and an engine built from the reloaded table runs the
    configurations the measuring engine chose - the same report lines, the same bits"""
    before, after = streaming["round_trip"]
    tuner, again = streaming["tuner"], streaming["again"]
    assert before == after
    assert hp.report_lines(again.report) == hp.report_lines(tuner.report)
    assert _bits_equal(again.out, tuner.out) and again.ops == tuner.ops
    assert _err(again.out, _oracle("21", 2, 16, 16)) <= 2e-2


# ---- 4. K22_PRIOR_SKINNY=0 ---------------------------------------------------------------------------------------------------------------
_PRIOR = {}


def _prior_inputs(bs, seed=7):
    """test_prior_gpu.py's (oracle.make_golden.prior_inputs)"""
    g = torch.Generator().manual_seed(seed)
    N = 2 * bs
    cm, cs = torch.randn(768, generator=g) * 0.1, torch.rand(768, generator=g) + 0.5
    txt_feat, txt_seq = torch.randn(N, 768, generator=g), torch.randn(N, 77, 768, generator=g)
    mask = torch.zeros(N, 77, dtype=torch.bool)
    for r in range(bs):
        mask[r, : 9 + 11 * r] = True
    mask[bs:, :2] = True
    x = torch.randn(N, 768, generator=g)
    return cm, cs, txt_feat, txt_seq, mask, x


def _prior(mp, fx, backend, skinny):
    """(module, transformer output) per (backend, route); the module is kept for the loop test"""
    key = (str(backend), skinny)
    if key not in _PRIOR:
        _env(mp, **({} if skinny else {"K22_PRIOR_SKINNY": 0}))
        cm, cs, txt_feat, txt_seq, mask, x = _prior_inputs(fx["bs"])
        m = k22.PriorDiffusionModelHIP(fx["hp"], k22.PRIOR_DIFFUSION_2_1, cm, cs, backend_dtype=backend)
        m.load_state_dict(k22.init_prior_state_dict(fx["hp"], seed=fx["seed_w"]))
        m = m.to("cuda")
        out = _guard(f"prior {backend} transformer", lambda: m.transformer(x.cuda(), fx["t"].cuda(), txt_feat.cuda(), txt_seq.cuda(), mask.cuda()).cpu())
        _PRIOR[key] = (m, out, m.tuning_report())
    return _PRIOR[key]


PRIOR_TOL = [(torch.bfloat16, 3e-2), (torch.float16, 4e-3)]      # test_prior_transformer_vs_reference_golden's


@pytest.mark.parametrize("backend,tol", PRIOR_TOL, ids=["bfloat16", "float16"])
def test_prior_skinny_off_vs_reference_golden(golden_dir, backend, tol, monkeypatch):
    fx = torch.load(os.path.join(golden_dir, "prior_tiny.pt"), weights_only=False)
    ref = fx["forward_out"]
    _m0, dflt, rep0 = _prior(monkeypatch, fx, backend, True)
    _m1, alt, rep1 = _prior(monkeypatch, fx, backend, False)
    wide = lambda rep: [r for r in hp.report_lines(rep) if r.taps == 1 and r.N == 4 * fx["hp"]["xf_width"]]   # noqa: E731
    print(f"K22_PRIOR_SKINNY=0 {backend}: vs golden {_err(alt, ref):.3e} of scale (default route {_err(dflt, ref):.3e}), "
          f"max|alt - default| / scale {_err(alt, dflt):.3e}; tuned ops default {sum(r.count for r in hp.report_lines(rep0))} -> "
          f"{sum(r.count for r in hp.report_lines(rep1))}, c_fc lines {wide(rep1)}")
    assert torch.isfinite(alt).all() and _err(alt, ref) <= tol and _err(dflt, ref) <= tol
    assert wide(rep1) and sum(r.count for r in wide(rep1)) == fx["hp"]["xf_layers"] and not wide(rep0)
    assert not _bits_equal(alt, dflt)                   # other kernels, other summation orders


@pytest.mark.parametrize("backend", [torch.bfloat16, torch.float16], ids=["bfloat16", "float16"])
def test_prior_skinny_off_whole_loop_equals_the_host_stepped_loop_bit_for_bit(golden_dir, backend, monkeypatch):
    fx = torch.load(os.path.join(golden_dir, "prior_tiny.pt"), weights_only=False)
    m, _out, rep = _prior(monkeypatch, fx, backend, False)
    assert any(r.taps == 1 and r.N == 4 * fx["hp"]["xf_width"] for r in hp.report_lines(rep))
    _env(monkeypatch, K22_PRIOR_SKINNY=0)               # (the same plan is reused; were it re-planned, then on the same route)
    _cm, _cs, txt_feat, txt_seq, mask, _x = _prior_inputs(fx["bs"])
    g = torch.Generator().manual_seed(31)
    N = 2 * fx["bs"]
    x_T, nzs = torch.randn(N, 768, generator=g).cuda(), torch.randn(5, N, 768, generator=g).cuda()
    run = lambda whole: m(txt_feat.cuda(), txt_seq.cuda(), mask.cuda(), fx["scales"].cuda(), timestep_respacing="ddim5", eta=1.0, noise=x_T,   # noqa: E731
                          noise_seq=nzs, whole_loop_graph=whole)
    c0, l0 = _counter("loop_captures"), _counter("loop_launches")
    step = _guard("prior stepwise loop", lambda: run(False))
    assert (_counter("loop_captures"), _counter("loop_launches")) == (c0, l0)
    whole = _guard("prior whole loop", lambda: run(True))
    again = _guard("prior whole loop, second call", lambda: run(True))
    assert (_counter("loop_captures"), _counter("loop_launches")) == (c0 + 1, l0 + 2)
    assert m.tuning_report() == rep                     # still the plan of the igemm route
    assert torch.isfinite(step).all() and torch.equal(step, whole) and torch.equal(whole, again)
