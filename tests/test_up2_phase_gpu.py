"""The four-phase upsampling convolution on the GPU (csrc/conv3_up2.hip, k22_conv3x3_up2 / k22_up2_fold; engine: K22_UP_PHASE).

KERNEL: against float64 of the UN-FOLDED definition - F.interpolate(x, 2, "nearest") then F.conv2d with the ORIGINAL 3x3 weights - so the fold
is under test as well.  Two comparisons per case, both with the comparator and bound of tests/helpers.py (igemm_violations; IGEMM_C, U24, d_T,
u_out as derived there, none taken from a kernel):

  (a) out against the float64 four-phase sum over the operands the kernel is promised to see (activations in T, the folded weight rounded
      once to T / split into x3 chunks), K = 4 * Cin products:      |out - ref_seen| <= c * (2^-24 + d_T) * S + u_out * |ref_seen|
  (b) out against the definition with the original fp32 weights; on top of (a)'s bound the definition is allowed what the number formats
      cost the WEIGHT operand: one rounding of the folded weight to T (u_T; 2^-22 for the fp16 hi / lo pair) and the three fp32 additions
      of the fold (3 * 2^-24), each relative to the folded weight, i.e. (u_T + 3 * 2^-24) * S.

GroupNorm partial sums: folded over the rows of an image and compared with the float64 sums of the output the launch itself stored
(helpers.stats_violations).  Every output and stats buffer is NaN-filled with guard elements on both sides; what the launch does not own must
still hold the fill.

ENGINE: tiny 2.1 and 2.2 UNets, B = 2, latent 16x16 and one ragged size: K22_UP_PHASE=1 against the CPU oracle within the bound the existing
forward tests use for the dtype (test_unet_gpu.py / test_unet22_gpu.py), against K22_UP_PHASE=0 within twice that bound, and the whole-loop
graph against the stepwise loop bit for bit with the phase route on."""
import types

import pytest
import torch
import torch.nn.functional as F

import helpers as hp
import kandinsky2_amd as k22
from kandinsky2_amd import _lib, native
from kandinsky2_amd.pack import fold_up2, to_x3
from oracle import unet22_ref, unet_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256
NAN = float("nan")
DTYPES = [_lib.K22_BF16, _lib.K22_F16, _lib.K22_F32, _lib.K22_F16X3, _lib.K22_F16X2]   # every dtype takes the new route
DT_IDS = [hp.DT_NAME[d] for d in DTYPES]


def guarded(shape, T):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=T, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


_CASES = {}


def case(B, H, W, Cin, Cout):
    """seeded fp32 inputs (as helpers.igemm_inputs draws them) and the float64 definition, computed once per shape"""
    key = (B, H, W, Cin, Cout)
    if key not in _CASES:
        g = torch.Generator(device=DEV).manual_seed(1000003 * (H * 131 + W * 17 + Cin + Cout) + 17)
        rn = lambda *s: torch.randn(*s, generator=g, device=DEV, dtype=torch.float32)
        x = 0.3 + 1.7 * rn(B, Cin, H, W)                 # non-zero mean: a missed border, bias or tap shows
        w = rn(Cout, Cin, 3, 3) * (9 * Cin) ** -0.5
        bias = rn(Cout)
        _CASES[key] = (x, w, bias)
    return _CASES[key]


def u_weight(dtype):
    return 2.0 ** -22 if dtype in hp.X_DTYPES else hp.u_out(dtype, _lib.OUT_ROWMAJOR)


def run_case(dtype, B, H, W, Cin, Cout, splitk=1, bm=0, stats=False, stages=-1, algo=0):
    x, w, bias = case(B, H, W, Cin, Cout)
    split = dtype in hp.X_DTYPES
    T = hp.storage_T(dtype)
    Np = (Cout + 63) // 64 * 64
    # operands in the formats the engine of that arithmetic holds
    f = fold_up2(w).reshape(4, Cout, 4 * Cin)                                            # fp32 sums
    fp = torch.cat([f, torch.zeros(4, Np - Cout, 4 * Cin, device=DEV)], 1).contiguous()
    xp = F.pad(x, (1, 1, 1, 1)).permute(0, 2, 3, 1).contiguous()                         # [B][H+2][W+2][Cin]
    if split:
        wdev, xdev = to_x3(fp), to_x3(xp, 1.0)
        w_seen = hp.x3_value(to_x3(f)) / 256.0
        x_seen = x.to(torch.float16).double() if dtype == _lib.K22_F16X2 else hp.x3_value(to_x3(x.permute(0, 2, 3, 1).contiguous(), 1.0)).permute(0, 3, 1, 2)
    else:
        wdev, xdev = fp.to(T).contiguous(), xp.to(T)
        w_seen, x_seen = f.to(T).double(), x.to(T).double()
    obuf, out = guarded((B, 2 * H, 2 * W, Cout), T)
    sbuf = srows = None
    if stats:
        cap = B * max(4 * H * W // 16, 4 * ((H * (W + 2) + 127) // 128)) + 3
        sbuf, srows = guarded((cap, Cout, 2), torch.float32)
    _lib.check(_lib.lib().k22_set_option(b"igemm_stages", stages))
    _lib.check(_lib.lib().k22_set_option(b"conv_algo", algo))       # 0 = the rule, 30 = lock-step form, 31 = explicit fragment pipeline
    try:
        rpi = native.conv3x3_up2(xdev, wdev, bias, out, B, H, W, Cin, Cout, dtype, splitk=splitk, bm=bm, stats=srows)
    finally:
        _lib.check(_lib.lib().k22_set_option(b"igemm_stages", -1))
        _lib.check(_lib.lib().k22_set_option(b"conv_algo", 0))
    torch.cuda.synchronize()
    assert guards_intact(obuf) and (sbuf is None or guards_intact(sbuf))

    # (a) the four-phase sum over the seen operands, float64, and the same over absolute values
    def phases(xs, ws, b):
        xq = F.pad(xs, (1, 1, 1, 1))
        o = torch.zeros(B, Cout, 2 * H, 2 * W, dtype=torch.float64, device=DEV)
        for py in (0, 1):
            for px in (0, 1):
                k = ws[2 * py + px].reshape(Cout, 2, 2, Cin).permute(0, 3, 1, 2)
                o[:, :, py::2, px::2] = F.conv2d(xq[:, :, py:py + H + 1, px:px + W + 1], k)
        return o + b[None, :, None, None]
    ref_seen = phases(x_seen, w_seen, bias.double())
    S = phases(x_seen.abs(), w_seen.abs(), bias.double().abs())
    bound_a = hp.IGEMM_C * (hp.U24 + hp.d_T(dtype)) * S + hp.u_out(dtype, _lib.OUT_ROWMAJOR) * ref_seen.abs()
    o = out.permute(0, 3, 1, 2)
    bad_a, ratio_a = hp.igemm_violations(o, ref_seen, bound_a)
    # (b) the un-folded definition with the original weights
    ref_def = F.conv2d(F.interpolate(x_seen, scale_factor=2, mode="nearest"), w.double(), bias.double(), padding=1)
    bound_b = bound_a + (u_weight(dtype) + 3 * hp.U24) * S
    bad_b, ratio_b = hp.igemm_violations(o, ref_def, bound_b)
    print(f"up2 {hp.DT_NAME[dtype]} B{B} {H}x{W} {Cin}->{Cout} sk{splitk} bm{bm} stg{stages} algo{algo} stats{int(stats)}: |err|/bound seen {ratio_a:.3f}, definition {ratio_b:.3f}, rpi {rpi}")
    assert bad_a == 0 and bad_b == 0
    if stats:
        t = types.SimpleNamespace(M=B * 4 * H * W, H=2 * H, W=2 * W, N=Cout)
        assert rpi > 0 and hp.stats_violations(srows, out.reshape(-1, Cout), t, rpi) == 0
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("H,W,Cin,Cout,bm", [
    (5, 3, 64, 64, 0),        # one tile, odd sizes
    (12, 20, 64, 128, 256),   # 264 plane positions: two 256-row tiles, the second ragged; m-tiles cross the padded plane's image boundary
    (12, 20, 64, 128, 128),   # three 128-row tiles
    (5, 3, 192, 64, 0),       # three K slabs (six in the 32-channel types): the weight ring wraps across taps and slabs
    (6, 6, 64, 160, 0),       # ragged n-tile, padded weight rows
])
@pytest.mark.parametrize("stats", [False, True], ids=["nostats", "stats"])
def test_up2_kernel_vs_float64_definition(dtype, H, W, Cin, Cout, bm, stats):
    run_case(dtype, 2, H, W, Cin, Cout, bm=bm, stats=stats)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("splitk", [2, 3])
def test_up2_kernel_splitk(dtype, splitk):
    # 6x6: 4 * HW % 16 == 0, the row-tiled finish delivers the sums; 5x3: the flat finish (no sums available there)
    run_case(dtype, 2, 6, 6, 192, 160, splitk=splitk, stats=True)
    run_case(dtype, 2, 5, 3, 192, 64, splitk=splitk, stats=False)


@pytest.mark.parametrize("dtype", [_lib.K22_BF16, _lib.K22_F32], ids=["bf16", "fp32"])
def test_up2_kernel_shallow_ring(dtype):
    """the two-deep weight ring (halo issued over three taps instead of one): same sums, same order -> the same bits as the four-deep one"""
    a = run_case(dtype, 2, 12, 20, 192, 128, bm=256, stages=2)
    b = run_case(dtype, 2, 12, 20, 192, 128, bm=256)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [_lib.K22_BF16, _lib.K22_F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("H,W,Cin,Cout,bm,splitk", [(12, 20, 192, 128, 256, 1), (12, 20, 192, 160, 128, 1), (6, 6, 192, 160, 0, 2), (5, 3, 64, 64, 0, 1)])
def test_up2_kernel_both_forms(dtype, H, W, Cin, Cout, bm, splitk):
    """16-bit types: the lock-step form (algo 30) and the explicit fragment pipeline (31; what the rule picks) multiply the same fragments in
    the same order -> both within the bounds, and the same bits"""
    a = run_case(dtype, 2, H, W, Cin, Cout, bm=bm, splitk=splitk, stats=H % 2 == 0, algo=30)
    b = run_case(dtype, 2, H, W, Cin, Cout, bm=bm, splitk=splitk, stats=H % 2 == 0, algo=31)
    assert torch.equal(a, b)


def test_device_fold_is_the_packers_fold_bit_for_bit():
    _x, w, _b = case(2, 6, 6, 64, 160)
    w9 = w.permute(0, 2, 3, 1).reshape(160, -1).contiguous()
    dev = native.up2_fold(w9, 192)
    torch.cuda.synchronize()
    ref = fold_up2(w).reshape(4, 160, -1)
    assert torch.equal(dev[:, :160], ref) and not dev[:, 160:].any()
    assert torch.equal(dev[:, :160].cpu(), fold_up2(w.cpu()).reshape(4, 160, -1))


# ---- engine ---------------------------------------------------------------------------------------------------------------------------
# bound per dtype = what the existing forward tests use (test_unet_gpu.py: test_forward_ragged_shapes_vs_oracle; test_unet22_gpu.py)
TOL21 = [(torch.float32, 2e-5), (torch.bfloat16, 2e-2), (torch.float16, 2.5e-3), ("f16x3", 2e-5), ("f16x2", 5e-4)]
TOL22 = [(torch.float32, 2e-4), (torch.bfloat16, 2.5e-2), (torch.float16, 3.2e-3)]
_REF = {}


def _n_phase_ops(m):
    return sum(1 for ln in m.tuning_report().splitlines() if ln.split()[:1] == ["4"])


def _forward21(backend, phase, h, w, monkeypatch):
    monkeypatch.setenv("K22_AUTOTUNE", "0")
    monkeypatch.setenv("K22_UP_PHASE", str(phase))
    arch = k22.make_arch(k22.tiny_model_config())
    sd = k22.init_unet_state_dict(arch, seed=13)
    B = 2
    full, pooled, image = k22.make_conditioning(arch, B, seed=6)
    g = torch.Generator().manual_seed(10 + h)
    x, t = torch.randn(B, 4, h, w, generator=g), torch.tensor([999.0, 3.0])
    if ("21", h, w) not in _REF:
        _REF[("21", h, w)] = unet_ref.unet_forward(sd, arch, x, t, full, pooled, image)
    m = k22.Text2ImUNetHIP(arch, backend_dtype=backend, use_graph=False)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    out = m(x.cuda(), t.cuda(), full_emb=full.cuda(), pooled_emb=pooled.cuda(), image_emb=image.cuda()).cpu()
    assert _n_phase_ops(m) == (len(arch.channel_mult) - 1 if phase else 0)     # the route under test is the one that ran
    return out, _REF[("21", h, w)]


@pytest.mark.parametrize("h,w", [(16, 16), (24, 40)])
@pytest.mark.parametrize("backend,tol", TOL21)
def test_engine_phase_route_vs_oracle_and_vs_nine_tap_route(backend, tol, h, w, monkeypatch):
    on, ref = _forward21(backend, 1, h, w, monkeypatch)
    off, _ = _forward21(backend, 0, h, w, monkeypatch)
    scale = ref.abs().max().item()
    e_on, e_ab = (on - ref).abs().max().item(), (on - off).abs().max().item()
    print(f"up2 engine {backend} {h}x{w}: phase route vs oracle {e_on / scale:.3e} of scale, vs 9-tap route {e_ab / scale:.3e}")
    assert torch.isfinite(on).all() and e_on <= tol * scale and e_ab <= 2 * tol * scale


@pytest.mark.parametrize("h,w", [(16, 16), (16, 24)])
@pytest.mark.parametrize("backend,tol", TOL22)
def test_engine22_phase_route_vs_oracle_and_vs_nine_tap_route(backend, tol, h, w, monkeypatch):
    monkeypatch.setenv("K22_AUTOTUNE", "0")
    cfg = k22.tiny_unet22_config()
    arch = k22.make_arch22(cfg, controlnet=False)
    sd = k22.init_unet22_state_dict(arch, seed=0)
    B = 2
    g = torch.Generator().manual_seed(4)
    x, emb, t = torch.randn(B, 4, h, w, generator=g), torch.randn(B, 1280, generator=g), torch.tensor([980.0, 20.0])
    if ("22", h, w) not in _REF:
        _REF[("22", h, w)] = unet22_ref.unet22_forward(sd, cfg, x, t, emb, None)
    ref = _REF[("22", h, w)]
    outs = {}
    for phase in (1, 0):
        monkeypatch.setenv("K22_UP_PHASE", str(phase))
        m = k22.UNet2DConditionHIP(arch, backend_dtype=backend, use_graph=False)
        m.load_state_dict(sd)
        m = m.to("cuda").eval()
        outs[phase] = m(sample=x.cuda(), timestep=t.cuda(), encoder_hidden_states=None, added_cond_kwargs={"image_embeds": emb.cuda()},
                        return_dict=False)[0].cpu()
        assert (_n_phase_ops(m) > 0) == bool(phase)
    scale = ref.abs().max().item()
    e_on, e_ab = (outs[1] - ref).abs().max().item(), (outs[1] - outs[0]).abs().max().item()
    print(f"up2 engine 2.2 {backend} {h}x{w}: phase route vs oracle {e_on / scale:.3e} of scale, vs 9-tap route {e_ab / scale:.3e}")
    assert torch.isfinite(outs[1]).all() and e_on <= tol * scale and e_ab <= 2 * tol * scale


@pytest.mark.parametrize("backend", [torch.float32, torch.bfloat16])
def test_whole_loop_graph_equals_the_stepwise_loop_with_the_phase_route(backend, monkeypatch):
    monkeypatch.setenv("K22_AUTOTUNE", "0")
    monkeypatch.setenv("K22_UP_PHASE", "1")
    arch = k22.make_arch(k22.tiny_model_config())
    sd = k22.init_unet_state_dict(arch, seed=13)
    B, h, w, steps = 2, 16, 16, 3
    full, pooled, image = k22.make_conditioning(arch, B, seed=6)
    m = k22.Text2ImUNetHIP(arch, backend_dtype=backend, use_graph=True)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    kw = dict(full_emb=full.cuda(), pooled_emb=pooled.cuda(), image_emb=image.cuda())
    d = k22.create_gaussian_diffusion(**dict(k22.DIFFUSION_CONFIG_2_1, timestep_respacing=str(steps)))
    g = torch.Generator().manual_seed(42)
    x_T = torch.randn(B, 4, h, w, generator=g).cuda()
    noise_seq = torch.randn(steps, B, 4, h, w, generator=g).cuda()
    step = d.p_sample_loop(m, (B, 4, h, w), model_kwargs=kw, guidance_scale=4.0, noise=x_T, noise_seq=noise_seq)
    m.del_cache()
    whole = d.p_sample_loop(m, (B, 4, h, w), model_kwargs=kw, guidance_scale=4.0, noise=x_T, noise_seq=noise_seq, whole_loop_graph=True)
    assert _n_phase_ops(m) == len(arch.channel_mult) - 1
    assert torch.isfinite(whole).all() and torch.equal(whole, step)
