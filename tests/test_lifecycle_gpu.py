"""The plan / bind life cycle that the four native engines share (csrc/plan.h), exercised through ordinary use of the six Python mirrors
(kandinsky2_amd/native.py): run at shape A, re-plan to shape B and run, re-plan back to A; bind the same plan to a second workspace; for
the UNet, a plan call with a rejected shape.  Every comparison is bit-for-bit (torch.equal): a plan is a pure function of (configuration,
weights, shape, tile table), a workspace holds no state that outlives a forward, and a cached graph never survives the plan or the
binding it was captured for."""
import ctypes as C

import pytest
import torch

import kandinsky2_amd as k22
from kandinsky2_amd import _lib

pytestmark = pytest.mark.gpu

BACKEND = torch.bfloat16


def _rebind(bind_fn, handle, old_ws):
    """the current plan on a fresh workspace of the same size; returns the tensor that keeps it alive"""
    ws = torch.empty_like(old_ws)
    assert ws.data_ptr() != old_ws.data_ptr()
    _lib.check(bind_fn(handle, (ws.data_ptr() + 255) // 256 * 256, old_ws.numel() - 256))
    return ws


def _unet():
    arch = k22.make_arch(k22.tiny_model_config())
    m = k22.Text2ImUNetHIP(arch, backend_dtype=BACKEND, use_graph=True)
    m.load_state_dict(k22.init_unet_state_dict(arch, seed=0))
    m = m.to("cuda")
    g = torch.Generator().manual_seed(5)
    xs = {2: torch.randn(2, 4, 16, 16, generator=g).cuda(), 4: torch.randn(4, 4, 24, 24, generator=g).cuda()}
    cond = {B: [t.cuda() for t in k22.make_conditioning(arch, B, seed=2)] for B in xs}

    def run(B):
        m._cond_key = None     # other batch / other workspace: the conditioning is set again
        full, pooled, image = cond[B]
        return m(xs[B], torch.full((B,), 500.0).cuda(), full_emb=full, pooled_emb=pooled, image_emb=image).clone()

    def rebind():
        m._ws = _rebind(_lib.lib().k22_unet_bind, m._handle, m._ws)

    def rejected_plan():
        n = C.c_size_t()
        assert _lib.lib().k22_unet_plan(m._handle, 9, 16, 16, C.byref(n)) != 0     # more than 8 rows per engine call
        assert b"batch" in _lib.lib().k22_last_error()
        # the old plan, its binding and its conditioning are untouched: no re-plan, no set_condition before the next forward
        full, pooled, image = cond[2]
        assert m._plan_key == (2, 16, 16)
        return m(xs[2], torch.full((2,), 500.0).cuda(), full_emb=full, pooled_emb=pooled, image_emb=image).clone()

    return run, 2, 4, rebind, rejected_plan


def _movq():
    arch = k22.MoVQArch(k22.MOVQ_CONFIG_2_1["ddconfig"])
    m = k22.MoVQDecoderHIP(backend_dtype=BACKEND)
    m.load_state_dict(k22.init_movq_state_dict(arch, seed=0), strict=True)
    m = m.to("cuda")
    g = torch.Generator().manual_seed(11)
    zs = {2: torch.randn(2, 4, 8, 8, generator=g).cuda(), 1: torch.randn(1, 4, 8, 16, generator=g).cuda()}

    def rebind():
        m._ws = _rebind(_lib.lib().k22_movq_bind, m._handle, m._ws)

    return (lambda B: m.decode(zs[B]).clone()), 2, 1, rebind, None


def _prior():
    hp = k22.tiny_prior_hparams()
    g = torch.Generator().manual_seed(7)
    cd, cw, nt = hp["clip_dim"], hp["clip_xf_width"], hp["text_ctx"]
    m = k22.PriorDiffusionModelHIP(hp, k22.PRIOR_DIFFUSION_2_1, torch.zeros(cd), torch.ones(cd), backend_dtype=BACKEND)
    m.load_state_dict(k22.init_prior_state_dict(hp, seed=0))
    m = m.to("cuda")
    ins = {}
    for B in (2, 4):
        mask = torch.zeros(B, nt, dtype=torch.bool)
        for r in range(B):
            mask[r, : 5 + 9 * r] = True
        ins[B] = [t.cuda() for t in (torch.randn(B, cd, generator=g), torch.full((B,), 321.0), torch.randn(B, cd, generator=g),
                                     torch.randn(B, nt, cw, generator=g), mask)]

    def rebind():
        m._ws = _rebind(_lib.lib().k22_prior_bind, m._handle, m._ws)

    return (lambda B: m.transformer(*ins[B]).clone()), 2, 4, rebind, None


def _tower():
    cfg = k22.tiny_xlmr_config()
    m = k22.MultilingualCLIPHIP(cfg, in_features=128, out_features=64, backend_dtype=BACKEND)
    m.load_state_dict(k22.init_multiclip_state_dict(cfg, 128, 64, seed=0))
    m = m.to("cuda")
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(2, cfg["vocab_size"], (2, 77), generator=g)
    mask = torch.ones(2, 77)
    mask[0, 30:] = 0
    ids[0, 30:] = cfg["pad_token_id"]

    def run(B):
        pooled, embs = m(ids[:B].cuda(), mask[:B].cuda())
        return torch.cat([pooled.reshape(-1), embs.reshape(-1)]).clone()

    def rebind():
        e = m._engine_for(77)
        e.ws = _rebind(_lib.lib().k22_encoder_bind, e.handle, e.ws)

    return run, 2, 1, rebind, None


def _movq_encoder():
    arch = k22.MoVQArch(k22.MOVQ_CONFIG_2_1["ddconfig"])
    m = k22.MoVQEncoderHIP(backend_dtype=BACKEND)
    m.load_state_dict(k22.init_movq_encoder_state_dict(arch, seed=0), strict=True)
    m = m.to("cuda")
    g = torch.Generator().manual_seed(13)
    # the smallest images that keep every level's height and width at least 8
    imgs = {2: torch.rand(2, 3, 64, 64, generator=g).cuda() * 2 - 1, 1: torch.rand(1, 3, 64, 128, generator=g).cuda() * 2 - 1}

    def rebind():
        m._ws = _rebind(_lib.lib().k22_movq_bind, m._handle, m._ws)

    return (lambda B: m.encode(imgs[B]).clone()), 2, 1, rebind, None


def _clip_text():
    cfg = k22.tiny_clip_config()
    m = k22.CLIPModelHIP(cfg, backend_dtype=BACKEND)
    m.load_state_dict(k22.init_clip_state_dict(cfg, seed=0))
    m = m.to("cuda")
    g = torch.Generator().manual_seed(17)
    tokens = torch.randint(1, cfg["vocab_size"] - 1, (2, cfg["context_length"]), generator=g)
    tokens[0, 9] = tokens[1, 30] = cfg["vocab_size"] - 1      # the end-of-text token: the largest id, where the pooled row is read

    def run(B):
        pooled, seq = m.encode_text_with_sequence(tokens[:B].cuda())
        return torch.cat([pooled.reshape(-1), seq.reshape(-1)]).clone()

    def rebind():
        e = m._engine("text")
        e.ws = _rebind(_lib.lib().k22_encoder_bind, e.handle, e.ws)

    return run, 2, 1, rebind, None


@pytest.mark.parametrize("engine", [_unet, _movq, _prior, _tower, _movq_encoder, _clip_text],
                         ids=["unet", "movq", "prior", "tower", "movq_encoder", "clip_text"])
def test_replan_and_rebind_reproduce_the_first_result_bit_for_bit(engine):
    run, A, B, rebind, rejected_plan = engine()
    first = run(A)
    assert torch.isfinite(first).all() and torch.equal(run(A), first)      # the cached graph against the eager + captured first pass
    other = run(B)
    assert torch.isfinite(other).all() and other.shape != first.shape
    assert torch.equal(run(A), first)                                      # A -> B -> A: the second plan of A is the first one again
    rebind()
    assert torch.equal(run(A), first)                                      # same plan, second workspace
    if rejected_plan is not None:
        assert torch.equal(rejected_plan(), first)                         # a rejected shape leaves the old plan running
    torch.cuda.synchronize()
