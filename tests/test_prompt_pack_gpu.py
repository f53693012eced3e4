"""Several prompts in ONE CFG batch on the GPU: Kandinsky2_1HIP.generate_img with a list of prompts and generate_text2img_many(pack=), on the
tiny pipeline of tests/test_pipeline_gpu.py (1/3-width UNet, 512x4 prior, full-width MoVQ, 128x128 px), whose builders this module imports.

 1. Row independence, the property packing rests on: with the same noises, prompts [A, B, C, D] and [A', B, C, D] give images 1-3 and final
    latents 1-3 that are torch.equal (p_sampler and ddim_sampler, fp32 and bf16), and [A, A, A, A] with identical noise rows gives four identical
    images.  Before the per-group threshold this could not hold for p_sampler: the percentile of element 0 - prompt A's image - clamped every
    row.  One generation at the packed shape runs before the two that are compared: tile configurations of problems the shipped table does
    not hold (a CFG batch of 8 at this tiny size) are measured during the first forward of a plan, behind that generation's conditioning,
    so a plan's first generation may be rounded differently from all later ones.
 2. Against the oracle (fp32): every packed prompt's final latent against diffusion_ref's loop run for THAT prompt alone (batch_size rows, the
    threshold from its own element 0), under the bound of test_generate_text2img_matches_the_oracle_chain_fp32: 1e-3 * max(1, scale); for
    p_sampler the uint8 image within one level.  The oracle's thresholds differ between the prompts (asserted), so a packed call that
    thresholded every prompt by prompt 0 would not pass.
 3. generate_text2img_many(pack=4) and (pack=2, batch_size=2) against the sequential generate_text2img calls (fp32), with the comparison and
    the bounds of test_generate_text2img_many_with_a_grouped_prior_equals_the_sequential_calls_to_rounding (mean byte difference below 0.05,
    worst at most 2; a packed batch runs other tile shapes, so equal to rounding and not bit for bit), a second pass that replays, and pack=1
    torch.equal to the call without the argument."""
import numpy as np
import pytest
import torch

from kandinsky2_amd import _lib
from oracle import diffusion_ref, movq_ref, unet_ref
from test_pipeline_gpu import H, PRIOR_STEPS, W, _oracle_image_emb, _pipe, _weights

pytestmark = pytest.mark.gpu

PROMPTS = ["green tree", "a red cat", "blue bird on a wire", "a house"]


def _noises(seed, n, bs, steps, same=False):
    """per-prompt lists: x_T [2 bs,4,h,w], noise_seq [steps, 2 bs, ...], prior noise [2 bs, 768], prior noise_seq [PRIOR_STEPS, 2 bs, 768]"""
    g = torch.Generator().manual_seed(seed)
    mk = lambda *sh: [torch.randn(*sh, generator=g).cuda() for _ in range(n)]   # noqa: E731
    out = mk(2 * bs, 4, H // 8, W // 8), mk(steps, 2 * bs, 4, H // 8, W // 8), mk(2 * bs, 768), mk(PRIOR_STEPS, 2 * bs, 768)
    return tuple([lst[0]] * n for lst in out) if same else out


def _many(pipe, prompts, nz, sampler, steps, bs=1, **kw):
    """-> (list of uint8 images [bs,H,W,3], the final latents of the LAST denoising call)"""
    out = pipe.generate_text2img_many(prompts, num_steps=steps, batch_size=bs, guidance_scale=4.0, h=H, w=W, sampler=sampler,
                                      prior_steps=str(PRIOR_STEPS), noises=nz[0], noise_seqs=nz[1], prior_noises=nz[2], prior_noise_seqs=nz[3],
                                      output_type="tensor", **kw)
    torch.cuda.synchronize()
    return out, pipe.last_latent.clone()


# ---- 1. row independence ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("sampler,steps", [("p_sampler", 6), ("ddim_sampler", 5)])
def test_a_packed_prompt_does_not_depend_on_the_other_prompts_of_its_batch(sampler, steps, backend):
    pipe = _pipe("text2img", backend)
    nz = _noises(31, 4, 1, steps)
    _many(pipe, PROMPTS, nz, sampler, steps, pack=4)                                   # the plan's first generation (module docstring)
    a, lat_a = _many(pipe, PROMPTS, nz, sampler, steps, pack=4)
    b, lat_b = _many(pipe, ["an orange fox in the snow"] + PROMPTS[1:], nz, sampler, steps, pack=4)
    assert len(a) == len(b) == 4 and lat_a.shape == (4, 4, H // 8, W // 8)
    assert not torch.equal(a[0], b[0]) and not torch.equal(lat_a[0], lat_b[0])         # the other prompt took part
    for i in (1, 2, 3):
        assert torch.equal(lat_a[i], lat_b[i]), (sampler, backend, i, (lat_a[i] - lat_b[i]).abs().max().item())
        assert torch.equal(a[i], b[i]), (sampler, backend, i)
    assert not torch.equal(a[1], a[2])
    same, lat_s = _many(pipe, [PROMPTS[0]] * 4, _noises(31, 4, 1, steps, same=True), sampler, steps, pack=4)
    for i in (1, 2, 3):
        assert torch.equal(lat_s[i], lat_s[0]) and torch.equal(same[i], same[0]), (sampler, backend, i)


# ---- 2. against the oracle, prompt by prompt --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler,steps", [("p_sampler", 6), ("ddim_sampler", 5)])
def test_every_packed_prompt_matches_the_oracle_chain_run_for_that_prompt_alone_fp32(sampler, steps, monkeypatch):
    pipe = _pipe("text2img")
    cfg, arch, unet_sd, hp, prior_sd, marc, movq_sd, cm, cs = _weights("text2img")
    bs, guidance, prompts = 2, 4.0, ["a red cat, 4k photo", "green tree"]
    g = torch.Generator().manual_seed(5)
    x_T, nz, p_xT, p_nz, lats, thresholds = [], [], [], [], [], []
    seen = []
    pct = np.percentile
    with monkeypatch.context() as mp:          # the oracle's own thresholds, read where it takes them (diffusion_ref.py: np.percentile)
        mp.setattr(diffusion_ref.np, "percentile", lambda *a, **k: seen.append(pct(*a, **k)) or seen[-1])
        for prompt in prompts:
            image_emb, xT_p, nz_p = _oracle_image_emb(pipe, prompt, bs, 4, g)
            x_T.append(torch.randn(2 * bs, 4, H // 8, W // 8, generator=g))
            nz.append(torch.randn(steps, 2 * bs, 4, H // 8, W // 8, generator=g))
            p_xT.append(xT_p)
            p_nz.append(nz_p)
            full, pooled = pipe.conditioner.encode_text(prompt, bs, "cpu")
            fn = lambda xc, tt: unet_ref.unet_forward(unet_sd, arch, xc, tt, full, pooled, image_emb)  # noqa: E731
            del seen[:]
            if sampler == "p_sampler":
                lat = diffusion_ref.RefDiffusion(steps).p_sample_loop(fn, x_T[-1], nz[-1], guidance)
            else:
                lat = diffusion_ref.ddim_sample_loop(fn, x_T[-1], steps, guidance)
            lats.append(lat[:bs])
            thresholds.append([max(float(np.asarray(s).ravel()[0]), 1.0) for s in seen])
    if sampler == "p_sampler":
        assert len(thresholds[0]) == steps and thresholds[0] != thresholds[1], thresholds
        print(f"oracle thresholds per prompt: {thresholds}")
    cuda = lambda lst: [t.cuda() for t in lst]   # noqa: E731
    got = pipe.generate_text2img_many(prompts, num_steps=steps, batch_size=bs, guidance_scale=guidance, h=H, w=W, sampler=sampler, prior_cf_scale=4,
                                      prior_steps=str(PRIOR_STEPS), noises=cuda(x_T), noise_seqs=cuda(nz), prior_noises=cuda(p_xT),
                                      prior_noise_seqs=cuda(p_nz), output_type="uint8", pack=2)
    latent = pipe.last_latent.cpu()
    assert latent.shape == (2 * bs, 4, H // 8, W // 8) and len(got) == 2
    for k, prompt in enumerate(prompts):
        lat = lats[k]
        e_lat, scale = (latent[k * bs:(k + 1) * bs] - lat).abs().max().item(), lat.abs().max().item()
        with torch.no_grad():
            want = movq_ref.process_images_u8(movq_ref.movq_decode(movq_sd, marc, lat / 1)[:, :, :H, :W])
        d = np.abs(got[k].astype(np.int32) - want.numpy().astype(np.int32))
        print(f"{sampler} prompt {k}: final latent max|d| {e_lat:.3e} (scale {scale:.2f}); uint8 image max diff {d.max()}, "
              f"{100.0 * (d > 0).mean():.3f} % of bytes differ")
        assert got[k].shape == (bs, H, W, 3) and got[k].dtype == np.uint8
        assert e_lat <= 1e-3 * max(1.0, scale), (sampler, k, e_lat, scale)
        if sampler == "p_sampler":
            assert d.max() <= 1, (k, d.max())


# ---- 3. generate_text2img_many(pack=) against the sequential calls ---------------------------------------------------------------------------
@pytest.mark.parametrize("pack,bs", [(4, 1), (2, 2)])
def test_generate_text2img_many_packed_equals_the_sequential_calls_to_rounding(pack, bs):
    pipe = _pipe("text2img", torch.float32)
    steps = 6
    nz = _noises(23, 4, bs, steps)
    kw = dict(num_steps=steps, batch_size=bs, guidance_scale=4.0, h=H, w=W, sampler="p_sampler", prior_steps=str(PRIOR_STEPS))
    seq = [pipe.generate_text2img(p, noise=nz[0][i], noise_seq=nz[1][i], prior_noise=nz[2][i], prior_noise_seq=nz[3][i], output_type="tensor", **kw)
           for i, p in enumerate(PROMPTS)]
    L = _lib.lib()
    captures = []
    for _ in range(2):                                   # the second pass replays the packed loop
        c0 = L.k22_debug_counter(b"loop_captures")
        many, _lat = _many(pipe, PROMPTS, nz, "p_sampler", steps, bs=bs, pack=pack)
        captures.append(L.k22_debug_counter(b"loop_captures") - c0)
        assert len(many) == len(PROMPTS)
        worst = 0
        for i in range(len(PROMPTS)):
            assert many[i].shape == seq[i].shape == (bs, H, W, 3)
            d = (many[i].int() - seq[i].int()).abs()
            worst = max(worst, int(d.max().item()))
            assert d.float().mean().item() < 0.05, (pack, bs, i, d.float().mean().item())
        print(f"pack={pack} batch_size={bs} vs per-prompt calls: uint8 max |d| {worst}; loop captures this pass {captures[-1]}")
        assert worst <= 2
    assert captures[0] >= 1 and captures[1] == 0, captures


def test_pack_1_is_the_call_without_the_argument():
    pipe = _pipe("text2img", torch.float32)
    nz = _noises(29, 3, 1, 6)
    a, lat_a = _many(pipe, PROMPTS[:3], nz, "p_sampler", 6)
    b, lat_b = _many(pipe, PROMPTS[:3], nz, "p_sampler", 6, pack=1)
    assert torch.equal(lat_a, lat_b) and all(torch.equal(u, v) for u, v in zip(a, b))
    # a negative decoder prompt forces pack back to one prompt per call (its prior call draws its own noise: seeded)
    torch.manual_seed(3)
    c, _ = _many(pipe, PROMPTS[:3], nz, "p_sampler", 6, pack=4, negative_decoder_prompt="blurry")
    torch.manual_seed(3)
    d, _ = _many(pipe, PROMPTS[:3], nz, "p_sampler", 6, negative_decoder_prompt="blurry")
    assert all(torch.equal(u, v) for u, v in zip(c, d))
