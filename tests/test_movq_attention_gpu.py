"""GPU tests of the fused MoVQ attention: k22_movq_attention (csrc/movq_attention.hip) against the float64 bound of movq_attn_ref, its
determinism and refusals, and the engine's "fused" AttnBlock route (k22_movq_set_attention, MoVQDecoderHIP / MoVQEncoderHIP attention=)
against the reference's goldens at the tolerances tests/test_movq_gpu.py holds the scores route to."""
import ctypes as C
import os

import pytest
import torch

import kandinsky2_amd as k22
import movq_attn_ref as mq
from kandinsky2_amd import _lib, movq
from oracle import movq_ref

pytestmark = pytest.mark.gpu

EINVAL = -1      # K22_EINVAL (include/k22.h)
TOLS = [(torch.float32, 2e-4), (torch.bfloat16, 6e-2), (torch.float16, 8e-3)]


def _launch(q, k, vt, bias, out, B, T, Cc, dtype):
    return _lib.lib().k22_movq_attention(_lib.ptr(q), _lib.ptr(k), _lib.ptr(vt), _lib.ptr(bias), _lib.ptr(out), B, T, Cc, dtype, _lib.current_stream())


_DEV = {}


def _device_operands(c, fam, dtype):
    """q, k, V^T in the storage type and bias on the GPU (cached: shared by the tests, never written to)"""
    key = (c, fam, dtype)
    if key not in _DEV:
        d = mq.inputs(c, fam)
        _DEV[key] = (mq.storage(d["q"], dtype).cuda(), mq.storage(d["k"], dtype).cuda(),
                     mq.storage(d["v"], dtype).transpose(1, 2).contiguous().cuda(), d["bias"].cuda())
    return _DEV[key]


def _run(c, fam, dtype):
    q, k, vt, bias = _device_operands(c, fam, dtype)
    out = torch.full_like(q, float("nan"))
    _lib.check(_launch(q, k, vt, bias, out, c[0], c[1], c[2], dtype))
    return out


# ---- 1. against float64 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", mq.DTYPES, ids=lambda d: mq.DT_NAME[d])
def test_movq_attention_vs_float64(dtype):
    worst, where = 0.0, None
    for c, fam in mq.pairs():
        ref, bnd, _ = mq.ref_and_bound(c, fam, dtype)
        out = _run(c, fam, dtype).cpu().double()
        assert torch.isfinite(out).all(), (mq.case_id(c), fam)
        r = mq.worst_ratio(out, ref, bnd)
        if r > worst:
            worst, where = r, (mq.case_id(c), fam)
    print(f"k22_movq_attention {mq.DT_NAME[dtype]}: worst |out - ref| / bound = {worst:.3f} at {where}")
    assert worst <= 1.0, where


def test_yardstick_torch_fp32_on_this_gpu_stays_under_c():
    per_family = {}
    for dtype in mq.DTYPES:
        for c, fam in mq.pairs():
            ref, _bnd, (q, k, v, bias, A, amp) = mq.ref_and_bound(c, fam, dtype)
            v32 = mq.plain32(q.cuda(), k.cuda(), v.cuda(), bias.cuda()).cpu()
            y = mq.yardstick(v32, ref, A, amp)
            per_family[fam] = max(per_family.get(fam, 0.0), y)
            assert y < mq.MQ_C, (mq.case_id(c), fam, y)
    print("yardstick (GPU) " + "   ".join(f"{f} {per_family[f]:.2f}" for f in mq.FAMILIES))


# ---- 2. determinism ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", mq.DTYPES, ids=lambda d: mq.DT_NAME[d])
def test_movq_attention_is_deterministic_and_batch_independent(dtype):
    for c in mq.CASES:
        fam = mq.families(c)[-1]
        a, b = _run(c, fam, dtype), _run(c, fam, dtype)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), mq.case_id(c)
        if c[0] == 2:
            q, k, vt, bias = _device_operands(c, fam, dtype)
            one = torch.full_like(q[1:2], float("nan"))
            _lib.check(_launch(q[1:2].contiguous(), k[1:2].contiguous(), vt[1:2].contiguous(), bias, one, 1, c[1], c[2], dtype))
            assert torch.equal(one.view(torch.uint8), a[1:2].contiguous().view(torch.uint8)), mq.case_id(c)


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_movq_attention_refusals_leave_the_library_usable():
    L = _lib.lib()
    x = torch.zeros(1, 576, 576, dtype=torch.float32, device="cuda")
    out = torch.zeros_like(x)
    for (B, T, Cc, o, word) in ((1, 64, 64, out, b"C must"), (1, 64, 576, out, b"C must"), (1, 96, 128, out, b"multiple of 64"),
                                (1, 0, 128, out, b"multiple of 64"), (1, 64, 128, None, b"null"), (0, 64, 128, out, b"B must")):
        rc = _launch(x, x, x, None, o, B, T, Cc, mq.F32)
        assert rc == EINVAL and word in L.k22_last_error(), (B, T, Cc, L.k22_last_error())
    assert _launch(x, x, x, None, out, 1, 64, 128, 7) == EINVAL and b"dtype" in L.k22_last_error()
    torch.cuda.synchronize()
    c = mq.CASES[0]
    ref, bnd, _ = mq.ref_and_bound(c, "rand", mq.F32)
    assert mq.worst_ratio(_run(c, "rand", mq.F32).cpu().double(), ref, bnd) <= 1.0           # a valid launch right after succeeds


# ---- 4 - 6. the engine route -------------------------------------------------------------------------------------------------------------
def _counter():
    return _lib.lib().k22_debug_counter(b"movq_fused_attn_launches")


_MODELS = {}


def _model(kind, backend):
    """one module per (decoder | encoder, type), shared by the tests: they switch its .attention"""
    if (kind, backend) not in _MODELS:
        arch = k22.MoVQArch(k22.MOVQ_CONFIG_2_1["ddconfig"])
        if kind == "dec":
            m, sd = k22.MoVQDecoderHIP(backend_dtype=backend), k22.init_movq_state_dict(arch, seed=0)
        else:
            m, sd = k22.MoVQEncoderHIP(backend_dtype=backend), k22.init_movq_encoder_state_dict(arch, seed=0)
        m.load_state_dict(sd, strict=True)
        _MODELS[(kind, backend)] = m.to("cuda")
    return _MODELS[(kind, backend)]


def _n_attn(kind):
    arch = k22.MoVQArch(k22.MOVQ_CONFIG_2_1["ddconfig"])
    blocks = arch.blocks()[0] if kind == "dec" else movq.movq_encoder_blocks(arch)[0]
    return sum(b[0] == "attn" for b in blocks)


def _fixture(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name + ".pt"), weights_only=False)


def _decode(fx, backend, attention):
    m = _model("dec", backend)
    m.attention = attention
    z = torch.randn(fx["B"], 4, fx["h"], fx["w"], generator=torch.Generator().manual_seed(fx["seed_z"]))
    out, u8 = m.decode(z.cuda(), return_uint8=True)
    return out.cpu(), u8.cpu()


def _encode(fx, backend, attention):
    m = _model("enc", backend)
    m.attention = attention
    x = torch.randn(fx["B"], 3, fx["H"], fx["W"], generator=torch.Generator().manual_seed(fx["seed_x"])).clamp(-2, 2) * 0.5
    return m.encode(x.cuda()).cpu()


def _compact_err(out, c):
    s = c["stride"]
    e = (out[..., ::s, ::s] - c["sub"]).abs().max().item()
    e = max(e, (out[..., c["r0"]: c["r0"] + c["rows"].shape[-2], :] - c["rows"]).abs().max().item())
    return max(e, (out[..., :, c["c0"]: c["c0"] + c["cols"].shape[-1]] - c["cols"]).abs().max().item())


@pytest.mark.parametrize("name", ["movq_small", "movq_wide", "movq_256px"])
@pytest.mark.parametrize("backend,tol", TOLS)
def test_fused_decoder_vs_reference_golden(golden_dir, name, backend, tol):
    fx = _fixture(golden_dir, name)
    n0 = _counter()
    out, u8 = _decode(fx, backend, "fused")
    assert _counter() - n0 == _n_attn("dec") == 4
    if "out_compact" in fx:
        scale, err = fx["absmax"], _compact_err(out, fx["out_compact"])
    else:
        scale, err = fx["out"].abs().max().item(), (out - fx["out"]).abs().max().item()
    print(f"{name} {backend} fused: max|d|={err:.3e} = {err / scale:.3e} of scale {scale:.3f}")
    assert err <= tol * scale
    assert torch.equal(u8, movq_ref.process_images_u8(out))
    if backend == torch.float32:
        assert (u8.int() - fx["out_u8"].int()).abs().max().item() <= 1
    # 5. the default is unchanged: "auto" is the scores route here, bit for bit, and launches nothing fused
    n1 = _counter()
    scores, scores_u8 = _decode(fx, backend, "scores")
    auto, auto_u8 = _decode(fx, backend, "auto")
    assert _counter() == n1
    assert torch.equal(auto, scores) and torch.equal(auto_u8, scores_u8)


@pytest.mark.parametrize("name", ["movq_enc_small", "movq_enc_wide", "movq_enc_256px"])
@pytest.mark.parametrize("backend,tol", TOLS)
def test_fused_encoder_vs_reference_golden(golden_dir, name, backend, tol):
    fx = _fixture(golden_dir, name)
    n0 = _counter()
    out = _encode(fx, backend, "fused")
    assert _counter() - n0 == _n_attn("enc") == 3
    ref = fx["out"]
    scale, err = ref.abs().max().item(), (out - ref).abs().max().item()
    print(f"{name} {backend} fused: max|d|={err:.3e} scale={scale:.3f}")
    assert out.shape == ref.shape and err <= tol * scale
    n1 = _counter()
    scores = _encode(fx, backend, "scores")
    auto = _encode(fx, backend, "auto")
    assert _counter() == n1 and torch.equal(auto, scores)


def test_fused_decode_is_deterministic_and_batch_independent():
    """the check of test_movq_gpu.py::test_movq_decode_is_deterministic_and_batch_independent on the fused route"""
    m = _model("dec", torch.float32)
    m.attention = "fused"
    z = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(11)).cuda()
    both = m.decode(z)
    assert torch.equal(both, m.decode(z))
    one = m.decode(z[1:2])
    assert (one - both[1:2]).abs().max().item() <= 1e-5 * both.abs().max().item()


# ---- 7. workspace ------------------------------------------------------------------------------------------------------------------------
def _plan_bytes(m, mode, B, h, w):
    """plan only, on the module's handle: (workspace bytes, ops)"""
    L, e = _lib.lib(), m._engines["movq"]
    e.plan_key = None                                   # the module's own plan is gone after this: it plans again at its next call
    n = C.c_size_t()
    _lib.check(L.k22_movq_set_attention(e.handle, movq.ATTENTION_MODES[mode]))
    _lib.check(L.k22_movq_plan(e.handle, B, h, w, C.byref(n)))
    return n.value, L.k22_movq_num_ops(e.handle)


@pytest.mark.parametrize("B", [1, 2])
def test_fused_plan_has_no_score_slot(B):
    m = _model("dec", torch.bfloat16)
    m.attention = "scores"
    m.decode(torch.zeros(1, 4, 8, 8, device="cuda"))    # builds the engine
    T, Cc = 64 * 64, 512
    ws_scores, _ = _plan_bytes(m, "scores", B, 64, 64)
    ws_fused, _ = _plan_bytes(m, "fused", B, 64, 64)
    print(f"B {B}: workspace scores {ws_scores} B, fused {ws_fused} B, score slot {B * T * T * 2} B")
    assert ws_scores - ws_fused >= B * T * T * 2 - 4 * B * T * Cc * 4


def test_fused_plan_refuses_a_width_the_kernel_does_not_admit_and_keeps_the_previous_plan():
    """ch = 128 x ch_mult 5 = 640 channels at the attention level: "fused" fails the plan with K22_EINVAL, "auto" falls back to scores"""
    L = _lib.lib()
    dd = dict(k22.MOVQ_CONFIG_2_1["ddconfig"], ch_mult=[1, 2, 2, 5])
    arch = k22.MoVQArch(dd)
    m = k22.MoVQDecoderHIP(dd, backend_dtype=torch.bfloat16)
    m.load_state_dict(k22.init_movq_state_dict(arch, seed=0), strict=True)
    m = m.to("cuda")
    z = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(3)).cuda()
    ref = m.decode(z)                                                       # auto = scores
    e = m._engines["movq"]
    n_ops = L.k22_movq_num_ops(e.handle)
    n = C.c_size_t()
    _lib.check(L.k22_movq_set_attention(e.handle, 2))
    assert L.k22_movq_plan(e.handle, 1, 8, 8, C.byref(n)) == EINVAL and b"fused attention" in L.k22_last_error()
    assert L.k22_movq_num_ops(e.handle) == n_ops                            # the previous plan is intact ...
    assert L.k22_movq_set_attention(e.handle, 3) == EINVAL
    z32 = z.float().contiguous()
    out = torch.empty_like(ref)
    _lib.check(L.k22_movq_decode(e.handle, z32.data_ptr(), out.data_ptr(), None, _lib.current_stream()))
    assert torch.equal(out, ref)                                            # ... and still decodes
    m.attention = "fused"
    with pytest.raises(RuntimeError):
        m.decode(z)


# ---- 8. the switch -----------------------------------------------------------------------------------------------------------------------
def test_auto_switches_to_the_fused_route_above_16384_keys():
    m = _model("dec", torch.bfloat16)
    L = _lib.lib()
    z = torch.randn(1, 4, 128, 136, generator=torch.Generator().manual_seed(5)).cuda()       # T = 17408
    m.attention = "auto"
    n0 = _counter()
    auto = m.decode(z)
    assert _counter() - n0 == _n_attn("dec")
    ops_auto = L.k22_movq_num_ops(m._handle)
    m.attention = "fused"
    fused = m.decode(z)
    ops_fused = L.k22_movq_num_ops(m._handle)
    assert torch.isfinite(auto).all() and torch.equal(auto, fused)
    _ws, ops_scores = _plan_bytes(m, "scores", 1, 128, 136)
    assert ops_auto == ops_fused != ops_scores
    m._release()                                                            # the 1024 x 1088 workspace
