"""k22_sampler_step_groups (csrc/sampler.hip: one sampler_threshold_kernel workgroup per threshold group, sampler_final_kernel reading the s
of every row's group) through the C entry point, and k22_unet_set_threshold_group through the whole-loop entry of a tiny UNet.  Items, the
reference with each row's own s and the wrong variants the items reject: tests/sampler_groups_ref.py (asserted on the CPU by
tests/test_sampler_groups_cpu.py); the select's references and bounds: tests/sampler_ref.py.

As in tests/test_sampler_select_gpu.py, x_out, x0_out and the scratch - sized exactly k22_sampler_scratch_bytes - each sit in a NaN-filled
buffer with 256 guard floats on both sides; every owned element is checked, the guards and the scratch floats behind the last group's s
(half / g .. 63) must still hold the fill, and a second launch into fresh buffers must give the same bits.  s_buf[j] is held to numpy's
percentile of the STORED row j g with no tolerance; x0_buf, x0_out and x_out to sampler_ref's bounds against float64, with each row's own s.
Refusals happen on the host: K22_EINVAL, a text, every buffer untouched.  A launch that fails otherwise ends the session (pytest.exit).

The loop tests: with a group set, the one-graph loop equals the stepwise route (k22_unet_forward + k22_sampler_step_groups per step) bit for
bit and the "loop_captures" / "loop_launches" counters show the route; another group re-captures, the same one replays, and group 0 after
a non-zero group gives the bits of a module that never had one.  Every module runs one generation before anything is compared: tile
configurations of problems the shipped table does not hold (a CFG batch of 8 at this tiny size) are measured during the first forward of a
plan, behind that generation's conditioning, so a plan's first generation may be rounded differently from all later ones."""
import pytest
import torch

import helpers as hp
import sampler_groups_ref as gr
import sampler_ref as sp
import kandinsky2_amd as k22
from kandinsky2_amd import _lib, sampling
from kandinsky2_amd.diffusion import percentile_index

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256
_EINVAL = -1         # include/k22.h: K22_EINVAL


def L():
    return _lib.lib()


@pytest.fixture(scope="module")
def table():
    return torch.from_numpy(sp.table()).to(DEV)


def guarded(n):
    return torch.full((n + 2 * GUARD,), sp.NAN, dtype=torch.float32, device=DEV)


def launch(d, table, N, HW, cfg, pct, g, entry="groups", n_arg=None):
    """one launch into fresh NaN-filled buffers -> (rc, [x_out, x0_out, scratch] whole buffers, guards included); entry "step": k22_sampler_step"""
    n_el = N * 4 * HW
    n_scr = L().k22_sampler_scratch_bytes(N, HW) // 4
    assert n_scr == n_el + sp.X0_OFF
    obuf, zbuf, sbuf = guarded(n_el), guarded(n_el), guarded(n_scr)
    head = (d["x"].data_ptr(), d["mo"].data_ptr(), d["noise"].data_ptr(), None, None, table.data_ptr(), sp.SELECT_ROW, sp.GUIDANCE, cfg,
            -d["clamp"], d["clamp"], pct[0], pct[1])
    tail = (sbuf[GUARD:].data_ptr(), obuf[GUARD:].data_ptr(), zbuf[GUARD:].data_ptr(), N if n_arg is None else n_arg, HW, hp.stream())
    try:
        rc = L().k22_sampler_step(*head, *tail) if entry == "step" else L().k22_sampler_step_groups(*head, g, *tail)
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"k22_sampler_step_groups N={N} HW={HW} g={g}: {e}", returncode=3)
    if rc not in (0, _EINVAL):
        pytest.exit(f"k22_sampler_step_groups N={N} HW={HW} g={g}: rc {rc}: {L().k22_last_error()}", returncode=3)
    return rc, [obuf, zbuf, sbuf]


def same_bits(a, b):
    return all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(a, b))


def untouched(*bufs):
    return all(bool(torch.isnan(b).all()) for b in bufs)


@pytest.mark.parametrize("item", gr.ITEMS)
def test_every_group_is_thresholded_by_its_own_row(item, table):
    N, HW, g, cfg = item
    half, G = gr.layout(N, g, cfg)
    d = sp.to_dev(gr.item_input(*item), DEV)
    pct = percentile_index(4 * HW)
    row = sp.table()[sp.SELECT_ROW]
    rc, bufs = launch(d, table, N, HW, cfg, pct, g)
    assert rc == 0, L().k22_last_error()
    rc, again = launch(d, table, N, HW, cfg, pct, g)
    assert rc == 0 and same_bits(bufs, again), "a second launch gave other bits"
    obuf, zbuf, sbuf = bufs
    n_el = N * 4 * HW
    scr = sbuf[GUARD:GUARD + sp.X0_OFF + n_el]
    assert untouched(sbuf[:GUARD], sbuf[GUARD + sp.X0_OFF + n_el:], scr[G:sp.X0_OFF]), (item, "scratch guards / floats half/g .. 63")
    x0_buf = scr[sp.X0_OFF:].view(N, 4, HW)
    assert torch.equal(x0_buf, sp.select_x0(d)), (item, "x0_buf is not clamp(x)")
    ref, bound = sp.x0_ref(d, row, cfg, d["clamp"], False)
    assert sp.violations(x0_buf, ref, bound)[0] == 0, (item, "x0_buf")
    # s_buf[j]: numpy's percentile of the stored row j g, equal bits
    x0_host = x0_buf.cpu().numpy().reshape(N, 4 * HW)
    S = gr.group_s(x0_host, N, g, cfg)
    got = scr[:G].cpu().numpy()
    assert [sp.f32bits(v) for v in got] == [sp.f32bits(v) for v in S], (item, got, S, [sp.dispatch(x0_host[j * g], pct[0]).label for j in range(G)])
    # x_out, x0_out: from the stored x0_buf with each row's own s
    out, z, Sx = gr.final_ref(x0_buf, S, d, row, N, g, cfg)
    b_out, b_z = sp.final_bounds(z, Sx, True)
    ratios = {}
    for name, buf, r, b in (("x_out", obuf, out, b_out), ("x0_out", zbuf, z, b_z)):
        nbad, ratios[name] = sp.violations(buf, sp.with_guard(r, GUARD), sp.with_guard(b, GUARD, 0.0))
        assert nbad == 0, (name, item, nbad, ratios[name])
    print(f"{item}: {G} groups, s {[float(v) for v in S]}; largest |out - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    if g == half:               # one group: k22_sampler_step itself, on the same operands
        rc, one = launch(d, table, N, HW, cfg, pct, g, entry="step")
        assert rc == 0 and same_bits(bufs, one), (item, "g == half is not k22_sampler_step")


def test_refusals_write_nothing(table):
    N, HW = 8, 255
    d = sp.to_dev(gr.item_input(8, 255, 2, 1), DEV)
    pct = percentile_index(4 * HW)
    for name, kw in (("pct_group 0", dict(g=0)), ("pct_group -2", dict(g=-2)), ("pct_group 3 does not divide 4", dict(g=3)),
                     ("pct_group 8 > half", dict(g=8)), ("N = 0", dict(g=1, n_arg=0)), ("odd N under CFG", dict(g=1, n_arg=7)),
                     ("pct_index = 4 HW", dict(g=1, pct=(4 * HW, 0.0)))):
        kw = dict(dict(pct=pct), **kw)
        rc, bufs = launch(d, table, N, HW, 1, kw["pct"], kw["g"], n_arg=kw.get("n_arg"))
        assert rc == _EINVAL and L().k22_last_error() and untouched(*bufs), name
    # more than 64 groups: 130 rows without CFG (HW = 1: the buffers stay tiny)
    big = {"x": torch.zeros(130, 4, 1, device=DEV), "mo": torch.zeros(130, 8, 1, device=DEV), "noise": torch.zeros(130, 4, 1, device=DEV), "clamp": sp.WIDE}
    rc, bufs = launch(big, table, 130, 1, 0, percentile_index(4), 1)
    assert rc == _EINVAL and b"64" in L().k22_last_error() and untouched(*bufs)
    rc, bufs = launch(big, table, 130, 1, 0, percentile_index(4), 2)          # 65 groups
    assert rc == _EINVAL and untouched(*bufs)
    rc, bufs = launch(big, table, 128, 1, 0, percentile_index(4), 2, n_arg=128)   # 64 groups run
    assert rc == 0, L().k22_last_error()


# ---- the loop entry: k22_unet_set_threshold_group ------------------------------------------------------------------------------------------------------
B, HL, WL, STEPS, GUIDE = 8, 16, 16, 3, 4.0


def _counters():
    return L().k22_debug_counter(b"loop_captures"), L().k22_debug_counter(b"loop_launches")


def _module(backend):
    arch = k22.make_arch(k22.tiny_model_config())
    m = k22.Text2ImUNetHIP(arch, backend_dtype=backend, use_graph=True)
    m.load_state_dict(k22.init_unet_state_dict(arch, seed=0))
    full, pooled, image = k22.make_conditioning(arch, B, seed=2)
    return m.to(DEV).eval(), dict(full_emb=full.cuda(), pooled_emb=pooled.cuda(), image_emb=image.cuda())


def _loop(m, kw, x_T, nz, group, whole):
    d = k22.create_gaussian_diffusion(**dict(k22.DIFFUSION_CONFIG_2_1, timestep_respacing=str(STEPS)))
    m.del_cache()
    return d.p_sample_loop(m, (B, 4, HL, WL), model_kwargs=kw, guidance_scale=GUIDE, noise=x_T, noise_seq=nz, whole_loop_graph=whole,
                           threshold_group=group)


@pytest.mark.parametrize("backend", [torch.float32, torch.bfloat16])
def test_loop_with_a_threshold_group_equals_the_stepwise_route_and_is_keyed_by_it(backend, monkeypatch):
    m, kw = _module(backend)
    g = torch.Generator().manual_seed(77)
    # rows of very different scales: the threshold of row 0 is not the threshold of the others
    scale = torch.tensor([1.0, 3.0, 0.3, 2.0] * 2).view(B, 1, 1, 1)
    x_T = (torch.randn(B, 4, HL, WL, generator=g) * scale).cuda()
    nz = (torch.randn(STEPS, B, 4, HL, WL, generator=g) * scale).cuda()
    _loop(m, kw, x_T, nz, None, False)                               # the plan's first generation (module docstring)
    c0, l0 = _counters()
    step = {grp: _loop(m, kw, x_T, nz, grp, False) for grp in (None, 1, 2)}
    assert _counters() == (c0, l0)                                   # the stepwise route is no loop
    assert not torch.equal(step[1], step[None]) and not torch.equal(step[2], step[1])     # the group takes part
    assert torch.equal(_loop(m, kw, x_T, nz, 4, False), step[None])  # g == half: the call as it has always been
    w1 = _loop(m, kw, x_T, nz, 1, True)
    assert _counters() == (c0 + 1, l0 + 1) and torch.equal(w1, step[1])
    w1b = _loop(m, kw, x_T, nz, 1, True)                             # the same value replays
    assert _counters() == (c0 + 1, l0 + 2) and torch.equal(w1b, step[1])
    w2 = _loop(m, kw, x_T, nz, 2, True)                              # another value re-captures
    assert _counters() == (c0 + 2, l0 + 3) and torch.equal(w2, step[2])
    w0 = _loop(m, kw, x_T, nz, None, True)                           # group 0 after a non-zero group: today's bits
    assert _counters() == (c0 + 3, l0 + 4) and torch.equal(w0, step[None])
    # a refused value leaves the handle's captured loop as it was: the next call with the last key replays
    assert L().k22_unet_set_threshold_group(m._handle, -1) == _EINVAL
    with pytest.raises(ValueError):
        _loop(m, kw, x_T, nz, 3, True)                               # Python refuses a group that does not divide the cond half ...
    with monkeypatch.context() as mp:
        mp.setattr(sampling, "threshold_group", lambda group, N, use_cfg=True: group)
        with pytest.raises(RuntimeError, match="threshold group"):
            _loop(m, kw, x_T, nz, 3, True)                           # ... and so does the loop entry, against the planned B
    assert _counters() == (c0 + 3, l0 + 4)
    assert torch.equal(_loop(m, kw, x_T, nz, None, True), step[None]) and _counters() == (c0 + 3, l0 + 5)
    fresh, kw2 = _module(backend)
    _loop(fresh, kw2, x_T, nz, None, False)
    assert torch.equal(_loop(fresh, kw2, x_T, nz, None, True), step[None])
