"""GPU suite of the Kandinsky 2.2 prior (kandinsky-2_amd/prior22.py, encoders.CLIPTextModelWithProjectionHIP): the text tower against the
installed transformers' CLIPTextModelWithProjection (tests/golden/enc_cliptext_hf_tiny.pt, tools/make_golden_prior22.py), PriorTransformerHIP
against PriorDiffusionModelHIP on the re-keyed weights (same arena, same kernels: bit for bit) and against the float64 restatement in the
diffusers layout (tests/prior22_ref.py), the UnCLIP loop as one graph against the stepwise route and against the restated step, and prompt ->
image through Kandinsky2_2HIP with the native prior as its conditioner.  Seeded weights throughout.

The diffusers side (PriorTransformer's key names, UnCLIPScheduler's arithmetic) is PARITY UNPINNED, as in tests/test_unet22_gpu.py.

Tolerances are the ones of the suites that run the same kernels at the same depth: the tiny towers of tests/test_encoders_gpu.py (2e-5, 1.5e-2,
2e-3 of the output scale for fp32, bf16, fp16) and tests/test_prior_gpu.py's transformer bounds (2e-4, 3e-2, 4e-3); the step bound is aux_ref's.
"""
import os

import pytest
import torch

import kandinsky2_amd as k22
import prior22_ref as pr
from kandinsky2_amd import _lib, prior22

pytestmark = pytest.mark.gpu

ENC_BACKENDS = [(torch.float32, 2e-5), (torch.bfloat16, 1.5e-2), (torch.float16, 2e-3)]
PRIOR_BACKENDS = [(torch.float32, 2e-4), (torch.bfloat16, 3e-2), (torch.float16, 4e-3)]
CFG = k22.tiny_prior22_config()


def _rel(a, b):
    return (a.float().cpu() - b).abs().max().item() / b.abs().max().item()


def _captures():
    return _lib.lib().k22_debug_counter(b"loop_captures")


# ---- text tower -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text_fx(golden_dir):
    return torch.load(os.path.join(golden_dir, "enc_cliptext_hf_tiny.pt"), weights_only=False)


def _text_model(fx, backend, eos):
    cfg = dict(fx["meta"]["cfg"], eos_token_id=eos)
    m = k22.CLIPTextModelWithProjectionHIP(cfg, backend_dtype=backend)
    m.load_state_dict(k22.init_clip_text_hf_state_dict(cfg, seed=fx["meta"]["seed_w"]))
    return m.to("cuda")


@pytest.mark.parametrize("backend,tol", ENC_BACKENDS)
def test_text_tower_vs_transformers_golden(text_fx, backend, tol):
    fx = text_fx
    ids, mask = fx["input_ids"].cuda(), fx["attention_mask"].cuda()
    eos, big = fx["meta"]["eos"], fx["meta"]["big_row"]
    m = _text_model(fx, backend, 2)
    # without a mask: every row of the sequence and the pooled output (argmax mode: eos_token_id == 2)
    out = m(ids)
    e_seq, e_emb = _rel(out.last_hidden_state, fx["last_hidden_state"]), _rel(out.text_embeds, fx["text_embeds"][2])
    assert out.text_embeds.shape == (3, 96) and out.last_hidden_state.shape == (3, 77, 128)
    # with the mask: the PADDED rows are what moves (rows 0 and 1 are padded; valid rows and the pooled output do not change)
    outm = m(ids, attention_mask=mask)
    pad = ~fx["attention_mask"][:2].bool()
    got, want = outm.last_hidden_state[:2].cpu()[pad], fx["last_hidden_state_masked_padded_rows"][pad]
    scale = fx["last_hidden_state"].abs().max().item()
    e_pad = (got - want).abs().max().item() / scale
    moved = (want - fx["last_hidden_state"][:2][pad]).abs().max().item() / scale
    e_valid = _rel(outm.last_hidden_state.cpu()[fx["attention_mask"].bool()], fx["last_hidden_state"][fx["attention_mask"].bool()])
    e_embm = _rel(outm.text_embeds, fx["text_embeds_masked"][2])
    # first-eos mode: row `big` carries a larger id before its eos
    m9 = _text_model(fx, backend, eos)
    out9 = m9(ids)
    e_big = (out9.text_embeds[big].cpu() - fx["text_embeds"][eos][big]).abs().max().item() / fx["text_embeds"][eos].abs().max().item()
    e_emb9 = _rel(out9.text_embeds, fx["text_embeds"][eos])
    argmax_would_be = (fx["text_embeds"][2][big] - fx["text_embeds"][eos][big]).abs().max().item() / fx["text_embeds"][eos].abs().max().item()
    print(f"text tower {backend}: seq {e_seq:.3e} text_embeds {e_emb:.3e} | masked: padded rows {e_pad:.3e} (the mask moves them by {moved:.3e}) "
          f"valid rows {e_valid:.3e} text_embeds {e_embm:.3e} | first-eos: row {big} {e_big:.3e} all {e_emb9:.3e} (argmax would be off by "
          f"{argmax_would_be:.3e}) of scale")
    assert moved > 10 * tol and argmax_would_be > 10 * tol                   # the fixture can tell the modes apart
    assert max(e_seq, e_emb, e_pad, e_valid, e_embm, e_big, e_emb9) <= tol
    assert _rel(m9(ids, attention_mask=mask).text_embeds, fx["text_embeds_masked"][eos]) <= tol


@pytest.mark.parametrize("backend", [torch.float32, torch.bfloat16])
def test_text_tower_with_both_switches_off_is_the_openai_tower(text_fx, backend):
    """key_mask = 0, eos_id = 0 (no attention_mask, eos_token_id 2): the engine of CLIPModelHIP.encode_text_with_sequence, bit for bit, on the
    same weights under OpenAI clip's keys"""
    hf_cfg = dict(k22.tiny_clip_text_hf_config(), hidden_act="quick_gelu")
    sd = k22.init_clip_text_hf_state_dict(hf_cfg, seed=4)
    m = k22.CLIPTextModelWithProjectionHIP(hf_cfg, backend_dtype=backend)
    m.load_state_dict(sd)
    ccfg = dict(k22.tiny_clip_config(), embed_dim=hf_cfg["projection_dim"])
    clip = k22.CLIPModelHIP(ccfg, backend_dtype=backend)
    clip.load_state_dict(pr.hf_text_to_openai_clip(sd, hf_cfg, k22.init_clip_state_dict(ccfg, seed=0)))
    ids = text_fx["input_ids"].cuda()
    out = m.to("cuda")(ids)
    feat, seq = clip.to("cuda").encode_text_with_sequence(ids)
    assert torch.equal(out.text_embeds, feat) and torch.equal(out.last_hidden_state, seq)


# ---- PriorTransformerHIP -----------------------------------------------------------------------------------------------------------------------
def _prior_inputs(B, seed=3):
    g = torch.Generator().manual_seed(seed)
    D = CFG["embedding_dim"]
    x, emb, seq = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g), torch.randn(B, 77, D, generator=g)
    mask = torch.zeros(B, 77, dtype=torch.bool)
    for r, n in zip(range(B), (2, 9, 77, 2)):
        mask[r, :n] = True
    t = torch.tensor([999.0, 500.0, 42.0, 0.0])[:B]
    return x, t, emb, seq, mask


@pytest.fixture(scope="module")
def prior_sd():
    return k22.init_prior22_state_dict(CFG, seed=1)


@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("backend,tol", PRIOR_BACKENDS)
def test_prior_transformer_forward(prior_sd, backend, tol, B):
    m = k22.PriorTransformerHIP(CFG, backend_dtype=backend)
    m.load_state_dict(prior_sd)
    m = m.to("cuda")
    x, t, emb, seq, mask = _prior_inputs(B)
    out = m(x.cuda(), t.cuda(), emb.cuda(), seq.cuda(), mask.cuda()).predicted_image_embedding
    # the 2.1 mirror on the re-keyed weights: the same arena and kernels
    hp = prior22.prior22_hparams(CFG)
    old = k22.PriorDiffusionModelHIP(hp, k22.PRIOR_DIFFUSION_2_1, backend_dtype=backend)
    old.load_state_dict(k22.rekey_prior22(prior_sd, CFG, "heads"))
    same = old.to("cuda").transformer(x.cuda(), t.cuda(), emb.cuda(), seq.cuda(), mask.cuda())
    assert out.shape == (B, CFG["embedding_dim"]) and torch.equal(out, same)
    ref = pr.transformer64(prior_sd, CFG, x, t, emb, seq, mask)
    err = (out.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    print(f"PriorTransformerHIP {backend} B={B}: {err:.3e} of scale against the float64 restatement (diffusers layout)")
    assert err <= tol


# ---- the pipeline with tiny towers ----------------------------------------------------------------------------------------------------------------
def _write_merges(folder):
    merges = [("c", "a"), ("ca", "t</w>"), ("d", "o"), ("do", "g</w>"), ("r", "e"), ("re", "d</w>")]
    path = os.path.join(folder, "merges.txt")
    with open(path, "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "\n".join(a + " " + b for a, b in merges) + "\n")
    return path


@pytest.fixture(scope="module")
def pipe(tmp_path_factory, prior_sd):
    """KandinskyV22PriorHIP in fp32: a 2-layer CLIP text tower and image tower at the widths the prior consumes (1280), the tiny prior"""
    tok = k22.ClipBPETokenizer(_write_merges(str(tmp_path_factory.mktemp("tok"))))
    tcfg = dict(k22.CLIP_BIGG_TEXT, num_hidden_layers=2, vocab_size=len(tok.encoder))
    text = k22.CLIPTextModelWithProjectionHIP(tcfg, backend_dtype=torch.float32)
    text.load_state_dict(k22.init_clip_text_hf_state_dict(tcfg, seed=2))
    vcfg = dict(k22.tiny_clip_vision_hf_config(), projection_dim=1280)
    image = k22.CLIPVisionModelWithProjectionHIP(vcfg, backend_dtype=torch.float32)
    image.load_state_dict(k22.init_clip_vision_hf_state_dict(vcfg, seed=3))
    prior = k22.PriorTransformerHIP(CFG, backend_dtype=torch.float32)
    prior.load_state_dict(prior_sd)
    return k22.KandinskyV22PriorHIP(prior.to("cuda"), image.to("cuda"), text.to("cuda"), tok)


def _noise(N, bs, seed=9):
    g = torch.Generator().manual_seed(seed + N + bs)
    return torch.randn(bs, 1280, generator=g).cuda(), torch.randn(N, bs, 1280, generator=g).cuda()


@pytest.mark.parametrize("N,bs", [(3, 1), (3, 2), (25, 1), (25, 2)])
def test_loop_one_graph_equals_stepwise_and_the_restated_step(pipe, N, bs):
    lat, nz = _noise(N, bs)
    prompts = ["a red cat", "dog"][:bs]
    kw = dict(num_inference_steps=N, guidance_scale=4.0, latents=lat, noise_seq=nz)
    c0 = _captures()
    a = pipe(prompts, None, **kw).image_embeds.clone()
    c1 = _captures()
    b = pipe(prompts, None, **kw).image_embeds.clone()
    assert c1 == c0 + 1 and _captures() == c1                                   # captured once; the second call replays
    step = pipe(prompts, None, whole_loop_graph=False, **kw).image_embeds
    assert a.shape == (bs, 1280) and torch.equal(a, b) and torch.equal(a, step) and _captures() == c1
    other = 4 if N == 3 else 24
    lat2, nz2 = _noise(other, bs)
    pipe(prompts, None, num_inference_steps=other, latents=lat2, noise_seq=nz2)
    assert _captures() == c1 + 1                                                # another step count captures again
    # the stepwise route, driven from here, against the restated step on the engine's own model outputs
    emb, seq, mask = pipe._encode_prompt(*pipe.batch_prompts(prompts, None), "cuda")
    table = pipe.scheduler.step_table(N).cuda()
    ts = pipe.scheduler.timesteps
    scales = torch.full((bs,), 4.0, device="cuda")
    x, rec = torch.cat([lat, lat], 0).contiguous(), []
    for k in range(N):
        mo = pipe.prior.transformer(torch.cat([x[:bs], x[:bs]], 0), torch.full((2 * bs,), float(ts[k]), device="cuda"), emb, seq, mask)
        nzk = torch.cat([nz[k], torch.zeros_like(nz[k])], 0).contiguous()
        nxt = torch.empty_like(x)
        _lib.check(_lib.lib().k22_prior_sampler_step(x.data_ptr(), mo.data_ptr(), nzk.data_ptr(), scales.data_ptr(), table[k].contiguous().data_ptr(), 10.0,
                                                     nxt.data_ptr(), bs, 1280, _lib.current_stream()))
        rec.append((x, mo, nzk, nxt))
        x = nxt
    assert torch.equal(pipe.prior.post_process_latents(x[:bs]), a)
    worst = pr.loop64(rec, scales, table)
    print(f"UnCLIP loop N={N} bs={bs}: largest |step - float64 step| / bound over the steps {worst:.3f}")
    assert worst <= 1.0


def test_one_row_table_returns_the_clamped_guided_x0(pipe):
    """table row (1, 0, *, 0): mean = 1 * x0 + 0 * x and no noise, so the loop returns clamp(uncond + g (cond - uncond)) itself.  The guided
    x0 is one multiply-add the compiler may contract: both roundings of it are accepted, nothing else."""
    bs, g = 2, 40.0                                      # a guidance large enough for the clamp to bite
    lat, nz = _noise(1, bs)
    emb, seq, mask = pipe._encode_prompt(*pipe.batch_prompts(["a red cat", "dog"], None), "cuda")
    table = torch.tensor([[1.0, 0.0, -46.0517, 0.0]], device="cuda")
    x = torch.cat([lat, lat], 0).contiguous()
    ts = torch.full((1, 2 * bs), 999.0, device="cuda")
    nzs = torch.cat([nz, torch.zeros_like(nz)], 1).contiguous()
    scales = torch.full((bs,), g, device="cuda")
    mo = pipe.prior.transformer(x, ts[0], emb, seq, mask)
    outs = [pipe.prior._run_loop(False, table, ts, x.clone(), nzs, scales, emb, seq, mask, whole, clamp=10.0)[:bs].clone() for whole in (True, False)]
    c, u = mo[:bs], mo[bs:]
    d = (c - u).double()
    plain = ((g * d).float() + u).clamp(-10.0, 10.0)
    fused = (g * d + u.double()).float().clamp(-10.0, 10.0)
    assert torch.equal(outs[0], outs[1]) and bool(((outs[0] == plain) | (outs[0] == fused)).all())
    assert 0 < int((outs[0].abs() == 10.0).sum()) < outs[0].numel()


def test_negative_prompt_and_zero_embed(pipe):
    lat, nz = _noise(3, 2)
    r = pipe("a red cat", "dog", num_inference_steps=3, latents=lat, noise_seq=nz)
    assert r.image_embeds.shape == (1, 1280) and r.negative_image_embeds.shape == (1, 1280)
    # the second row of the doubled batch is the prior of the negative prompt guided against itself (same row of the same batch shape)
    alone = pipe("dog", "dog", num_inference_steps=3, latents=lat, noise_seq=nz)
    assert torch.equal(r.negative_image_embeds, alone.negative_image_embeds) and not torch.equal(r.image_embeds, alone.image_embeds)
    z = pipe("a red cat", None, num_inference_steps=3, latents=lat[:1], noise_seq=nz[:, :1]).negative_image_embeds
    assert torch.equal(z, pipe.get_zero_embed(1)) and torch.equal(z, pipe.image_encoder(torch.zeros(1, 3, 56, 56).cuda()).image_embeds)


def test_prompt_to_image_with_the_native_prior(pipe):
    """Kandinsky2_2HIP with KandinskyV22PriorHIP as its conditioner: tiny towers, tiny prior, tiny_unet22_config(), 64 x 64, 3 decoder steps"""
    marc = k22.MoVQArch(k22.MOVQ_CONFIG_2_1["ddconfig"])
    msd = dict(k22.init_movq_state_dict(marc, seed=0))
    msd.update(k22.init_movq_encoder_state_dict(marc, seed=0))
    ucfg = k22.tiny_unet22_config()
    usd = k22.init_unet22_state_dict(k22.make_arch22(ucfg), seed=0)
    H = 64
    g = torch.Generator().manual_seed(5)
    lat, nz = torch.randn(1, 4, 8, 8, generator=g).cuda(), torch.randn(3, 1, 4, 8, 8, generator=g).cuda()
    mdl = k22.pipeline22.Kandinsky2_2HIP("cuda", "text2img", unet_state_dict=usd, movq_state_dict=msd, unet_config=ucfg, conditioner=pipe,
                                         backend_dtype=torch.float32)
    assert mdl.conditioner is pipe

    def gen(prompt):
        torch.manual_seed(0)                                  # the prior draws its own latents and step noise
        return mdl.generate_text2img(prompt, batch_size=1, decoder_steps=3, prior_steps=3, h=H, w=H, latents=lat, noise_seq=nz, output_type="latent")

    a, b, c = gen("a red cat"), gen("a red cat"), gen("dog")
    assert a.shape == (1, 4, 8, 8) and bool(torch.isfinite(a).all()) and torch.equal(a, b) and not torch.equal(a, c)
    seeded = k22.pipeline22.Kandinsky2_2HIP("cuda", "text2img", unet_state_dict=usd, movq_state_dict=msd, unet_config=ucfg, conditioner="seeded",
                                            backend_dtype=torch.float32)
    s = seeded.generate_text2img("a red cat", batch_size=1, decoder_steps=3, prior_steps=3, h=H, w=H, latents=lat, noise_seq=nz, output_type="latent")
    assert not torch.equal(a, s)                              # the seeded stand-in is not what ran
    img = torch.randn(1, 3, 56, 56, generator=g)
    torch.manual_seed(0)
    mix = mdl.mix_images(["a red cat", img], [0.3, 0.7], batch_size=1, decoder_steps=2, prior_steps=3, h=H, w=H, output_type="uint8")
    assert mix.shape == (1, H, H, 3) and mix.dtype.name == "uint8"
    i2i = k22.pipeline22.Kandinsky2_2HIP("cuda", "img2img", unet_state_dict=usd, movq_state_dict=msd, unet_config=ucfg, conditioner=pipe,
                                         backend_dtype=torch.float32)
    torch.manual_seed(0)
    out = i2i.generate_img2img("a red cat", torch.zeros(1, 3, H, H).cuda(), strength=0.5, batch_size=1, decoder_steps=4, prior_steps=3, h=H, w=H,
                               output_type="uint8")
    assert out.shape == (1, H, H, 3)
