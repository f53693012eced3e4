"""CPU suite of the Kandinsky 2.2 prior (kandinsky-2_amd/prior22.py): the diffusers -> engine key map against an independent float64
restatement, the UnCLIP step table, and the pipeline's host logic with stub towers.  The diffusers side is PARITY UNPINNED (prior22.py);
what these tests pin is stated in each.

UnCLIP step table, float32 against a float64 evaluation of the same formulas (printed by test_step_table_float32_deviation, recorded in
DESIGN.md; NOT asserted: `1 - a_t / a_prev` and `1 - a_t` cancel).  The last row shows it best: in exact arithmetic c1 = beta_0 / (1 - a_0)
= 1, in float32 a_0 = fl(1 - beta_0) and 1 - a_0 differs from beta_0 by the rounding of a_0, up to 2^-25 against beta_0 = 4.13e-5.
"""
import gzip
import json

import pytest
import torch

import kandinsky2_amd as k22
import prior22_ref as pr
from kandinsky2_amd import pipeline22, prior22
from kandinsky2_amd.tokenizer import ClipBPETokenizer
from oracle import prior_ref

CFG = k22.tiny_prior22_config()


def _inputs(B, lens, seed=3):
    g = torch.Generator().manual_seed(seed)
    D = CFG["embedding_dim"]
    x, emb, seq = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g), torch.randn(B, 77, D, generator=g)
    mask = torch.zeros(B, 77, dtype=torch.bool)
    for r in range(B):
        mask[r, : lens[r % len(lens)]] = True
    t = torch.tensor([999.0, 500.0, 42.0, 0.0])[:B]
    return x, t, emb, seq, mask


@pytest.fixture(scope="module")
def keymap_case():
    sd = k22.init_prior22_state_dict(CFG, seed=1)
    x, t, emb, seq, mask = _inputs(3, (2, 9, 77))
    ref = pr.transformer64(sd, CFG, x, t, emb, seq, mask)
    return sd, (x, t, emb, seq, mask), ref


def _through_oracle(sd, inputs):
    hp = prior22.prior22_hparams(CFG)
    return prior_ref.transformer_forward(k22.rekey_prior22(sd, CFG, "heads"), hp, *inputs)


def test_key_map_against_float64_diffusers_layout(keymap_case):
    """diffusers keys -> rekey_prior22 -> oracle/prior_ref.transformer_forward (the pinned restatement of the reference network, fp32)
    against transformer64 (diffusers layout, float64), within prior22_ref.chain_bound"""
    sd, inputs, ref = keymap_case
    out = _through_oracle(sd, inputs)
    bound = pr.chain_bound(ref, CFG["num_layers"])
    err = (out.double() - ref).abs().max().item()
    print(f"key map: max|d| {err:.3e}, bound {bound:.3e} ({pr.chain_c(CFG['num_layers']):.0f} x 2^-24 of scale {ref.abs().max().item():.3f})")
    assert out.shape == ref.shape == (3, CFG["embedding_dim"]) and err <= bound
    # the entries are prior_param_shapes' and the planes layout is the heads layout de-interleaved
    hp = prior22.prior22_hparams(CFG)
    planes, heads = k22.rekey_prior22(sd, CFG, "planes"), k22.rekey_prior22(sd, CFG, "heads")
    assert list(planes) == list(k22.prior_param_shapes(hp)) and all(tuple(planes[k].shape) == s for k, s in k22.prior_param_shapes(hp).items())
    from kandinsky2_amd.prior import qkv_planes
    for k in planes:
        assert torch.equal(planes[k], qkv_planes(heads[k], hp["xf_heads"]) if ".c_qkv." in k else heads[k])


@pytest.mark.parametrize("mutant", ["q_k_swapped", "norm3_is_norm1", "v_bias_dropped", "time_linears_swapped"])
def test_key_map_mutants_exceed_the_bound(keymap_case, mutant):
    sd, inputs, ref = keymap_case
    m = dict(sd)
    p = "transformer_blocks.1."
    if mutant == "q_k_swapped":
        for leaf in (".weight", ".bias"):
            m[p + "attn1.to_q" + leaf], m[p + "attn1.to_k" + leaf] = sd[p + "attn1.to_k" + leaf], sd[p + "attn1.to_q" + leaf]
    elif mutant == "norm3_is_norm1":
        for leaf in (".weight", ".bias"):
            m[p + "norm3" + leaf] = sd[p + "norm1" + leaf]
    elif mutant == "v_bias_dropped":
        m[p + "attn1.to_v.bias"] = torch.zeros_like(sd[p + "attn1.to_v.bias"])
    else:
        for leaf in (".weight", ".bias"):
            m["time_embedding.linear_1" + leaf], m["time_embedding.linear_2" + leaf] = sd["time_embedding.linear_2" + leaf], sd["time_embedding.linear_1" + leaf]
    err = (_through_oracle(m, inputs).double() - ref).abs().max().item()
    assert err > 10 * pr.chain_bound(ref, CFG["num_layers"]), (mutant, err)


def test_masked_logits_minus_10000_equal_minus_inf(keymap_case):
    """PriorTransformerHIP's docstring: diffusers' additive -10000 and the reference's -inf give the same fp32 network"""
    sd, inputs, ref = keymap_case
    x = torch.tensor([3.0, -2.0, 1.0])
    assert torch.equal(torch.softmax(x + torch.tensor([0.0, -10000.0, 0.0]), 0), torch.softmax(x + torch.tensor([0.0, float("-inf"), 0.0]), 0))


def test_config_refusals():
    for key, bad in (("time_embed_act_fn", "gelu"), ("norm_in_type", "layer"), ("embedding_proj_norm_type", "layer"),
                     ("encoder_hid_proj_type", None), ("added_emb_type", None), ("dropout", 0.1), ("attention_head_dim", 32),
                     ("additional_embeddings", 3), ("time_embed_dim", 100)):
        with pytest.raises(NotImplementedError, match=key):
            k22.PriorTransformerHIP(dict(CFG, **{key: bad}))
    with pytest.raises(ValueError, match="no_such_key"):
        k22.PriorTransformerHIP(dict(CFG, no_such_key=1))
    m = k22.PriorTransformerHIP(dict(CFG, _class_name="PriorTransformer", time_embed_dim=None, clip_embed_dim=1280))
    sd = k22.init_prior22_state_dict(CFG, seed=0)
    m.load_state_dict(dict(sd, causal_attention_mask=torch.zeros(1, 81, 81)))       # accepted and ignored
    assert torch.equal(m.post_process_latents(torch.ones(2, 1280)), sd["clip_std"] + sd["clip_mean"].expand(2, -1))
    with pytest.raises(RuntimeError):                                               # no CPU fallback
        m(torch.zeros(1, 1280), 0, torch.zeros(1, 1280), torch.zeros(1, 77, 1280), torch.ones(1, 77))


# ---- scheduler ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 3, 25, 1000])
def test_step_table_equals_restatement_and_invariants(N):
    s = k22.UnCLIPSchedulerHIP.from_config(k22.SCHEDULER_CONFIG_PRIOR_2_2)
    tab = s.step_table(N)
    ref, ts, branch = pr.step_table(N)
    assert tab.dtype == torch.float32 and tab.shape == (N, 4) and torch.equal(tab, ref) and s.timesteps.tolist() == ts
    assert s.timesteps.dtype == torch.int64 and ts[0] == 999 and ts[-1] == 0 and all(a > b for a, b in zip(ts, ts[1:]))
    assert torch.equal(tab[:, 3], torch.tensor([1.0] * (N - 1) + [0.0])) and bool(torch.isfinite(tab).all())
    if N == 1000:
        assert all(branch)
    # the last row: a_prev = 1 gives c2 = 0 exactly and c1 = beta_0 / (1 - a_0), which is 1 up to the rounding of a_0 = fl(1 - beta_0):
    # |(1 - a_0) - beta_0| <= 2^-25 (half an ulp below 1), one more rounding for the quotient
    b0 = s.betas[0].item()
    assert tab[-1, 1].item() == 0.0 and tab[-1, 3].item() == 0.0 and abs(tab[-1, 0].item() - 1.0) <= 2.0 ** -25 / b0 * (1 + 2e-3) + 2.0 ** -23


def test_step_table_float32_deviation():
    for N in (2, 3, 25, 1000):
        t32, t64 = pr.step_table(N)[0].double(), pr.step_table(N, dtype=torch.float64)[0]
        d = (t32 - t64).abs()
        rel = (d[:, :2] / t64[:, :2].abs().clamp_min(1e-30)).max().item()
        print(f"UnCLIP table N={N}: float32 - float64  c1 {d[:, 0].max().item():.3e}  c2 {d[:, 1].max().item():.3e}  logvar {d[:-1, 2].max().item():.3e} "
              f"(largest relative c1 / c2 deviation {rel:.3e})")
        assert bool(torch.isfinite(t64).all())


def test_scheduler_refusals():
    s = k22.UnCLIPSchedulerHIP.from_config(k22.SCHEDULER_CONFIG_PRIOR_2_2)
    assert s.missing_keys == () and s.clip == 10.0
    assert k22.UnCLIPSchedulerHIP.from_config({"prediction_type": "sample"}).missing_keys == tuple(sorted(
        k for k in prior22.UNCLIP_SCHEDULER_DEFAULTS if k != "prediction_type"))
    with pytest.raises(ValueError):
        s.step_table(1)
    with pytest.raises(ValueError, match="timestep_spacing"):
        k22.UnCLIPSchedulerHIP.from_config(dict(k22.SCHEDULER_CONFIG_PRIOR_2_2, timestep_spacing="leading"))
    for key, bad in (("prediction_type", "epsilon"), ("variance_type", "learned_range"), ("beta_schedule", "linear")):
        with pytest.raises(NotImplementedError, match=key):
            k22.UnCLIPSchedulerHIP.from_config(dict(k22.SCHEDULER_CONFIG_PRIOR_2_2, **{key: bad}))
    with pytest.raises(NotImplementedError):
        k22.UnCLIPSchedulerHIP.from_config(dict(k22.SCHEDULER_CONFIG_PRIOR_2_2, _class_name="DDPMScheduler"))


# ---- pipeline host logic with stub towers -----------------------------------------------------------------------------------------------------
class _StubTok:
    def padded_ids_and_mask(self, texts, max_length=77, pad_id=0):
        self.texts = list(texts)
        ids = torch.zeros(len(texts), max_length, dtype=torch.long)
        for i, t in enumerate(texts):
            ids[i, 0] = 1 + sum(map(ord, t)) % 97
        return ids, ids > 0


class _StubText:
    def __call__(self, ids, attention_mask=None):
        from types import SimpleNamespace
        assert attention_mask is None                      # the pipeline calls the tower on the ids alone
        e = ids[:, :1].float().expand(-1, 8)
        return SimpleNamespace(text_embeds=e, last_hidden_state=e[:, None, :].expand(-1, 77, -1))


class _StubImage:
    config = type("C", (), {"image_size": 4})()

    def __call__(self, px):
        from types import SimpleNamespace
        return SimpleNamespace(image_embeds=px.reshape(px.shape[0], -1)[:, :8] + 7.0)


class _StubPrior:
    """_run_loop: the sum of the text embedding and the noise of every step, so the result names its rows"""
    hp = {"clip_dim": 8}

    def __init__(self):
        self.calls = []

    def _run_loop(self, ddim, table, ts, x, nzs, scales, emb, seq, mask, whole, clamp=10.0):
        self.calls.append(dict(N=x.shape[0], T=table.shape[0], ts=ts[:, 0].tolist(), whole=whole, clamp=clamp, scales=scales.tolist(), ddim=ddim,
                               second_half_noise=float(nzs[:, x.shape[0] // 2:].abs().max())))
        return x + emb + 100.0 * torch.cat([emb[x.shape[0] // 2:], emb[x.shape[0] // 2:]]) + nzs.sum(0)

    def post_process_latents(self, x):
        return x * 2.0


def _pipe():
    return k22.KandinskyV22PriorHIP(_StubPrior(), _StubImage(), _StubText(), _StubTok(), device="cpu")


def test_batch_assembly_and_chunk_rule():
    bp = k22.KandinskyV22PriorHIP.batch_prompts
    assert bp("a", None) == (["a"], [""]) and bp(["a", "b"], None, 2) == (["a", "a", "b", "b"], [""] * 4)
    assert bp("a", "n", 2) == (["a", "a", "n", "n"], ["n"] * 4) and bp(["a", "b"], ["m", "n"]) == (["a", "b", "m", "n"], ["m", "n", "m", "n"])
    with pytest.raises(ValueError):
        bp(["a", "b"], "n")
    p = _pipe()
    code = lambda t: float(1 + sum(map(ord, t)) % 97)  # noqa: E731
    lat, nz = torch.zeros(1, 8), torch.zeros(3, 1, 8)
    r = p("cat", None, num_inference_steps=3, guidance_scale=5.0, latents=lat, noise_seq=nz)
    c = p.prior.calls[-1]
    assert p.tokenizer.texts == ["cat", ""] and c["N"] == 2 and c["T"] == 3 and c["ts"] == [999.0, 500.0, 0.0] and c["whole"] and c["clamp"] == 10.0
    assert c["scales"] == [5.0] and not c["ddim"]
    assert torch.equal(r.image_embeds, torch.full((1, 8), 2.0 * (code("cat") + 100.0 * code(""))))
    assert torch.equal(r.negative_image_embeds, torch.full((1, 8), 7.0))           # get_zero_embed: the image tower on a zero image
    # with a negative prompt: the batch doubles, the classifier-free branch of every row is the negative prompt, chunk(2) splits the result
    r = p("cat", "dog", num_images_per_prompt=2, num_inference_steps=2, latents=torch.zeros(4, 8), noise_seq=torch.ones(2, 4, 8), whole_loop_graph=False)
    c = p.prior.calls[-1]
    assert p.tokenizer.texts == ["cat", "cat", "dog", "dog"] + ["dog"] * 4 and c["N"] == 8 and not c["whole"] and c["second_half_noise"] == 0.0
    assert torch.equal(r.image_embeds, torch.full((2, 8), 2.0 * (code("cat") + 100.0 * code("dog") + 2.0)))
    assert torch.equal(r.negative_image_embeds, torch.full((2, 8), 2.0 * (code("dog") + 100.0 * code("dog") + 2.0)))
    # more than 4 samples: independent chunks of at most 4
    n0 = len(p.prior.calls)
    r = p(["a", "b", "c", "d", "e"], None, num_inference_steps=2, latents=torch.zeros(5, 8), noise_seq=torch.zeros(2, 5, 8))
    assert [c["N"] for c in p.prior.calls[n0:]] == [8, 2] and r.image_embeds.shape == (5, 8)
    assert torch.equal(r.image_embeds[:, 0], torch.tensor([2.0 * (code(t) + 100.0 * code("")) for t in "abcde"]))
    with pytest.raises(ValueError):
        p("cat", None, num_inference_steps=1)
    with pytest.raises(ValueError):
        p("cat", None, num_inference_steps=2, latents=torch.zeros(2, 8))


def test_interpolate_weights_and_conditioner_protocol():
    p = _pipe()
    code = lambda t: float(1 + sum(map(ord, t)) % 97)  # noqa: E731
    img = torch.ones(3, 4, 4)
    kw = dict(num_inference_steps=2, latents=torch.zeros(1, 8), noise_seq=torch.zeros(2, 1, 8))
    r = p.interpolate(["cat", img], [0.25, 0.75], **kw)
    want = 0.25 * 2.0 * (code("cat") + 100.0 * code("")) + 0.75 * 8.0
    assert torch.allclose(r.image_embeds, torch.full((1, 8), want)) and torch.equal(r.negative_image_embeds, torch.full((1, 8), 7.0))
    with pytest.raises(ValueError):
        p.interpolate(["cat"], [0.5, 0.5], **kw)
    assert p.encode_image22(img, "cpu").shape == (1, 8)
    a, n = p.prior22("cat", None, 2, 2, 4.0, "cpu")
    assert a.shape == (2, 8) and n.shape == (2, 8) and torch.equal(n, torch.full((2, 8), 7.0))


def test_kandinsky22_conditioner_argument():
    with pytest.raises(ValueError, match="conditioner"):
        pipeline22.Kandinsky2_2HIP("cuda", "text2img", unet_state_dict={}, movq_state_dict={}, conditioner=None)
    with pytest.raises(ValueError, match="prior_cache_dir"):
        pipeline22.Kandinsky2_2HIP("cuda", "text2img", unet_state_dict={}, movq_state_dict={}, conditioner="native")
    with pytest.raises(ValueError, match="native"):
        pipeline22.Kandinsky2_2HIP("cuda", "text2img", unet_state_dict={}, movq_state_dict={}, conditioner="other")


def test_loader_names_missing_files(tmp_path):
    with pytest.raises(FileNotFoundError) as e:
        k22.load_prior22_from_cache_dir(str(tmp_path))
    for name in ("prior", "text_encoder", "image_encoder", "merges.txt"):
        assert name in str(e.value)
    with pytest.raises(FileNotFoundError):
        pipeline22.Kandinsky2_2HIP("cuda", "text2img", unet_state_dict={}, movq_state_dict={}, conditioner="native", prior_cache_dir=str(tmp_path))


def test_tokenizer_merges_txt_and_padded_ids(tmp_path):
    merges = [("c", "a"), ("ca", "t</w>"), ("d", "o"), ("do", "g</w>")]
    body = "#version: 0.2\n" + "\n".join(a + " " + b for a, b in merges) + "\n"
    with gzip.open(tmp_path / "bpe_simple_vocab_16e6.txt.gz", "wb") as f:
        f.write(body.encode("utf-8"))
    (tmp_path / "merges.txt").write_text(body, encoding="utf-8")
    gz, txt = ClipBPETokenizer(str(tmp_path / "bpe_simple_vocab_16e6.txt.gz")), ClipBPETokenizer(str(tmp_path / "merges.txt"))
    texts = ["a cat", "dog a dog", "", " ".join(["cat"] * 100)]
    assert all(gz.encode(t) == txt.encode(t) for t in texts) and gz.encoder == txt.encoder
    ids, mask = txt.padded_ids_and_mask(texts, pad_id=5)
    sot, eot = txt.sot_token, txt.eot_token
    assert ids.shape == (4, 77) and ids.dtype == torch.long and mask.dtype == torch.bool
    assert ids[0].tolist() == [sot] + txt.encode("a cat") + [eot] + [5] * 73 and mask[0].tolist() == [True] * 4 + [False] * 73
    assert ids[2].tolist() == [sot, eot] + [5] * 75 and int(mask[2].sum()) == 2
    assert ids[3].tolist() == [sot] + txt.encode(texts[3])[:75] + [eot] and bool(mask[3].all())
    assert txt.padded_ids_and_mask("a cat")[0][0, 4].item() == 0                    # pad id 0 by default; a string is one text
    # pad id from a transformers tokenizer folder
    assert txt.pad_id_from_folder(str(tmp_path)) == 0
    (tmp_path / "tokenizer_config.json").write_text(json.dumps({"pad_token": {"content": "<|endoftext|>"}}))
    assert txt.pad_id_from_folder(str(tmp_path)) == eot
    (tmp_path / "vocab.json").write_text(json.dumps({"!": 0, "<|endoftext|>": 49407}))
    assert txt.pad_id_from_folder(str(tmp_path)) == 49407
    (tmp_path / "tokenizer_config.json").write_text(json.dumps({"pad_token": "!"}))
    assert txt.pad_id_from_folder(str(tmp_path)) == 0


def test_text_tower_shapes_and_config():
    cfg = k22.tiny_clip_text_hf_config()
    assert cfg["projection_dim"] == 96 and cfg["hidden_size"] == 128 and k22.CLIP_BIGG_TEXT["hidden_size"] == 64 * k22.CLIP_BIGG_TEXT["num_attention_heads"]
    shapes = k22.clip_text_hf_param_shapes(cfg)
    assert shapes["text_projection.weight"] == (96, 128) and "text_projection.bias" not in shapes
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    hf = CLIPTextModelWithProjection(CLIPTextConfig(vocab_size=1000, hidden_size=128, intermediate_size=512, projection_dim=96, num_hidden_layers=2,
                                                    num_attention_heads=2, max_position_embeddings=77))
    theirs = {k: tuple(v.shape) for k, v in hf.state_dict().items() if not k.endswith("position_ids")}
    assert theirs == dict(shapes)
    m = k22.CLIPTextModelWithProjectionHIP(cfg)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 76, dtype=torch.long))
    with pytest.raises(ValueError):
        m(torch.full((1, 77), 1000, dtype=torch.long))
    with pytest.raises(RuntimeError):                       # no CPU fallback
        m(torch.zeros(1, 77, dtype=torch.long))
    with pytest.raises(ValueError):
        k22.CLIPTextModelWithProjectionHIP(dict(cfg, num_attention_heads=4))


def test_loader_reads_a_prior_repository(tmp_path):
    """load_prior22_from_cache_dir on a tiny copy of the repository layout: every config.json drives its module, scheduler_config.json is
    preferred to SCHEDULER_CONFIG_PRIOR_2_2, .safetensors and .bin both load, the pad id comes from the tokenizer folder"""
    from safetensors.torch import save_file
    root = tmp_path / "kandinsky-2-2-prior"
    for d in ("prior", "text_encoder", "image_encoder", "tokenizer", "scheduler"):
        (root / d).mkdir(parents=True)
    tcfg, vcfg = k22.tiny_clip_text_hf_config(), k22.tiny_clip_vision_hf_config()
    psd, tsd, vsd = k22.init_prior22_state_dict(CFG, seed=1), k22.init_clip_text_hf_state_dict(tcfg, seed=2), k22.init_clip_vision_hf_state_dict(vcfg, seed=3)
    save_file({k: v.contiguous() for k, v in psd.items()}, str(root / "prior" / "diffusion_pytorch_model.safetensors"))
    torch.save(dict(tsd), str(root / "text_encoder" / "pytorch_model.bin"))
    save_file({k: v.contiguous() for k, v in vsd.items()}, str(root / "image_encoder" / "model.safetensors"))
    (root / "prior" / "config.json").write_text(json.dumps(dict(CFG, _class_name="PriorTransformer")))
    (root / "text_encoder" / "config.json").write_text(json.dumps(dict(tcfg, architectures=["CLIPTextModelWithProjection"], eos_token_id=7)))
    (root / "image_encoder" / "config.json").write_text(json.dumps(dict(vcfg, model_type="clip_vision_model")))
    (root / "tokenizer" / "merges.txt").write_text("#version: 0.2\nc a\nca t</w>\n", encoding="utf-8")
    (root / "tokenizer" / "tokenizer_config.json").write_text(json.dumps({"pad_token": "<|endoftext|>"}))
    (root / "scheduler" / "scheduler_config.json").write_text(json.dumps(dict(k22.SCHEDULER_CONFIG_PRIOR_2_2, clip_sample_range=5.0, _class_name="UnCLIPScheduler")))
    p = k22.load_prior22_from_cache_dir(str(tmp_path), torch.float32, device="cpu")
    assert p.scheduler.clip == 5.0 and p.pad_id == p.tokenizer.eot_token and p.text_encoder.config.eos_token_id == 7
    assert p.prior.hp["xf_layers"] == CFG["num_layers"] and p.image_encoder.config.image_size == vcfg["image_size"]
    for mod, sd in ((p.prior, psd), (p.text_encoder, tsd), (p.image_encoder, vsd)):
        got = mod.state_dict()
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    (root / "scheduler" / "scheduler_config.json").unlink()
    assert k22.load_prior22_from_cache_dir(str(tmp_path), torch.float32, device="cpu").scheduler.clip == 10.0
