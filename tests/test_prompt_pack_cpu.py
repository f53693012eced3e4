"""Several prompts in ONE CFG batch (Kandinsky2_1HIP.generate_img with a list of prompts, generate_text2img_many(pack=)): the row layout as
pure functions, the limits and the clipping rule.  No GPU: kandinsky2_amd.pipeline.cfg_pack / cfg_unpack / prompts_per_call are what the
pipeline itself calls; the GPU side is tests/test_prompt_pack_gpu.py."""
import pytest
import torch

from kandinsky2_amd.pipeline import Kandinsky2_1HIP, cfg_pack, cfg_unpack, prompts_per_call


def _tagged(n, bs, *tail):
    """n per-prompt CFG tensors [2 bs, *tail] whose every element names its prompt, half and row: 100 prompt + 10 uncond + row"""
    out = []
    for k in range(n):
        rows = [100.0 * k + 10.0 * u + r for u in (0, 1) for r in range(bs)]
        out.append(torch.tensor(rows).view(2 * bs, *([1] * len(tail))).expand(2 * bs, *tail).contiguous())
    return out


@pytest.mark.parametrize("n,bs", [(4, 1), (2, 2), (3, 1), (1, 4), (1, 1)])
def test_prompts_batch_size_and_noises_go_to_cfg_rows_and_back(n, bs):
    per = _tagged(n, bs, 4, 3, 3)
    packed = cfg_pack(per, bs)
    half = n * bs
    assert packed.shape == (2 * half, 4, 3, 3)
    for row in range(2 * half):
        k, r, uncond = (row % half) // bs, (row % half) % bs, row // half
        assert packed[row].unique().tolist() == [100.0 * k + 10.0 * uncond + r], (row, k, r, uncond)
    # the sampler kernels pair row i with row i + half: both belong to one prompt and one image of it
    for i in range(half):
        assert packed[i + half, 0, 0, 0] - packed[i, 0, 0, 0] == 10.0
    # the threshold group of row `row` with threshold_group = batch_size is its prompt
    assert [(row % half) // bs for row in range(2 * half)] == [k for _ in (0, 1) for k in range(n) for _ in range(bs)]
    back = cfg_unpack(packed, n, bs)
    assert len(back) == n and all(torch.equal(a, b) for a, b in zip(back, per))
    if n == 1:
        assert torch.equal(packed, per[0])                      # one prompt: the layout of a call of its own


def test_noise_seqs_are_laid_out_along_dim_1():
    n, bs, steps = 3, 1, 5
    per = [t.unsqueeze(0).expand(steps, -1, -1, -1, -1).contiguous() + 1000.0 * torch.arange(steps).view(steps, 1, 1, 1, 1) for t in _tagged(n, bs, 4, 2, 2)]
    packed = cfg_pack(per, bs, dim=1)
    assert packed.shape == (steps, 2 * n * bs, 4, 2, 2)
    for k in range(steps):
        assert torch.equal(packed[k], cfg_pack([p[k] for p in per], bs))
    assert all(torch.equal(a, b) for a, b in zip(cfg_unpack(packed, n, bs, dim=1), per))
    # the layout the grouped prior of generate_text2img_many has always used for its noise
    bs = 2
    per = _tagged(2, bs, 7)
    assert torch.equal(cfg_pack(per, bs), torch.cat([p[:bs] for p in per] + [p[bs:] for p in per], 0))


def test_wrong_row_counts_are_refused():
    with pytest.raises(ValueError):
        cfg_pack(_tagged(2, 2, 4), 1)
    with pytest.raises(ValueError):
        cfg_unpack(torch.zeros(6, 4), 2, 2)


def test_pack_is_clipped_to_a_cfg_batch_of_eight_and_a_negative_decoder_prompt_forces_one():
    # pack * batch_size <= 4, at least 1 - the rule of prior_group
    assert [prompts_per_call(4, bs) for bs in (1, 2, 3, 4)] == [4, 2, 1, 1]
    assert [prompts_per_call(p, 1) for p in (0, 1, 2, 3, 4, 5, 100)] == [1, 1, 2, 3, 4, 4, 4]
    assert prompts_per_call(2, 2) == 2 and prompts_per_call(3, 2) == 2 and prompts_per_call(1, 4) == 1 and prompts_per_call(4, 8) == 1
    for bs in (1, 2, 4):
        for want in (1, 2, 4, 9):
            assert 2 * prompts_per_call(want, bs) * bs <= 8
            assert prompts_per_call(want, bs, "blurry, low quality") == 1
    assert prompts_per_call(4, 1, "") == 4


def test_generate_img_keeps_the_limit_of_eight_rows_for_a_list_of_prompts():
    pipe = object.__new__(Kandinsky2_1HIP)          # the checks run before anything of the instance is read
    for prompts, bs in ((["a", "b", "c", "d", "e"], 1), (["a", "b", "c"], 2), (("a", "b"), 3), ("a", 5)):
        with pytest.raises(ValueError, match="CFG batch <= 8"):
            pipe.generate_img(prompts, None, batch_size=bs)
    for bad in ([], ["a", 3]):
        with pytest.raises(ValueError, match="list / tuple of strings"):
            pipe.generate_img(bad, None, batch_size=1)
