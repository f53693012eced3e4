"""Mints tests/golden/enc_cliptext_hf_tiny.pt: the installed transformers' CLIPTextModelWithProjection on tiny_clip_text_hf_config() and this
project's seeded weights (init_clip_text_hf_state_dict) - the pin of encoders.CLIPTextModelWithProjectionHIP (tests/test_prior22_gpu.py).
transformers is an independent library; nothing of the reference project is read.

    python tools/make_golden_prior22.py

One set of input ids serves two eos settings, since the pooled row is all that eos_token_id changes (asserted below):
    eos_token_id = 2    transformers' legacy branch: the pooled row is argmax(input_ids)
    eos_token_id = EOS  the pooled row is the FIRST position holding EOS.  Row 1 carries a larger id before its EOS, where argmax lands,
                        and is padded with EOS itself (pad id == eos id: only the first one counts).
Each setting is run without and with attention_mask.  Row lengths 3, 9 and 77 (a full row, no padding).  With the mask only the padded
rows of last_hidden_state move (valid rows and text_embeds are identical, asserted), so the masked sequence output is stored for the two
padded rows only; the file stays below enc_clip_tiny.pt's size.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kandinsky2_amd as k22  # noqa: E402

SEED_W, EOS, SOT, BIG = 11, 900, 898, 950
LENGTHS = (3, 9, 77)


def inputs(cfg):
    g = torch.Generator().manual_seed(5)
    n = cfg["max_position_embeddings"]
    ids = torch.zeros(len(LENGTHS), n, dtype=torch.long)
    mask = torch.zeros(len(LENGTHS), n, dtype=torch.long)
    for r, L in enumerate(LENGTHS):
        ids[r, 0] = SOT
        ids[r, 1:L - 1] = torch.randint(3, SOT, (L - 2,), generator=g)
        ids[r, L - 1] = EOS
        mask[r, :L] = 1
    ids[1, 4] = BIG                  # a larger id before the eos: argmax pools position 4, first-eos position 8
    ids[1, LENGTHS[1]:] = EOS        # padded with the eos id itself
    return ids, mask


def main():
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    cfg = k22.tiny_clip_text_hf_config()
    sd = k22.init_clip_text_hf_state_dict(cfg, seed=SEED_W)
    ids, mask = inputs(cfg)
    out = {}
    for eos in (2, EOS):
        hc = CLIPTextConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                            projection_dim=cfg["projection_dim"], num_hidden_layers=cfg["num_hidden_layers"],
                            num_attention_heads=cfg["num_attention_heads"], max_position_embeddings=cfg["max_position_embeddings"],
                            hidden_act=cfg["hidden_act"], layer_norm_eps=cfg["layer_norm_eps"], eos_token_id=eos, pad_token_id=1, bos_token_id=0)
        m = CLIPTextModelWithProjection(hc).eval()
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
        with torch.no_grad():
            a, b = m(input_ids=ids), m(input_ids=ids, attention_mask=mask)
        out[eos] = (a.text_embeds.float(), a.last_hidden_state.float(), b.text_embeds.float(), b.last_hidden_state.float())
    (e2, s2, e2m, s2m), (e9, s9, e9m, s9m) = out[2], out[EOS]
    assert torch.equal(s2, s9) and torch.equal(s2m, s9m), "last_hidden_state must not depend on eos_token_id"
    valid = mask.bool()
    d_valid, d_pad = (s2 - s2m)[valid].abs().max().item(), (s2 - s2m)[~valid].abs().max().item()
    print(f"attention_mask: valid rows move by {d_valid:.3e}, padded rows by {d_pad:.3e}; text_embeds by {(e2 - e2m).abs().max().item():.3e} / "
          f"{(e9 - e9m).abs().max().item():.3e}")
    assert d_valid == 0.0 and d_pad > 0.1 and torch.equal(e2, e2m) and torch.equal(e9, e9m)
    assert not torch.allclose(e2[1], e9[1]), "row 1 must pool another position in the two modes"
    assert torch.equal(e2[0], e9[0]) and torch.equal(e2[2], e9[2])
    import transformers
    fx = {"meta": {"cfg": cfg, "seed_w": SEED_W, "transformers": transformers.__version__, "lengths": LENGTHS, "eos": EOS, "big_row": 1,
                   "padded_rows": (0, 1)},
          "input_ids": ids.int(), "attention_mask": mask.to(torch.uint8),
          "last_hidden_state": s2, "last_hidden_state_masked_padded_rows": s2m[:2].clone(),
          "text_embeds": {2: e2, EOS: e9}, "text_embeds_masked": {2: e2m, EOS: e9m}}
    path = os.path.join(ROOT, "tests", "golden", "enc_cliptext_hf_tiny.pt")
    torch.save(fx, path)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
