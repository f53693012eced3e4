"""CPU half of the tests of k22_sampler_step_groups / k22_unet_set_threshold_group (tests/sampler_groups_ref.py,
tests/test_sampler_groups_gpu.py), on the references and the host side of the C entries alone:
 (a) the host model of the select (sampler_ref.select_emul), applied per group, is numpy's percentile of row j g bit for bit at every item;
 (b) the items can tell a wrong grouping from a right one: the s of the groups differ in bits, one group is clamped to 1 and one lies above,
     a non-zero group takes the fall-back path and another a tie case - and each of three wrong implementations (every threshold from row 0,
     the source row j g + 1, a group index without the % half) fails the checks the GPU test makes, on the GPU test's own inputs;
 (c) the two entries are exported and refuse on the host, without a device; sampling.threshold_group checks what Python passes them."""
import numpy as np
import pytest
import torch

import sampler_groups_ref as gr
import sampler_ref as sp
from kandinsky2_amd import _lib, sampling
from kandinsky2_amd.diffusion import percentile_index

_EINVAL = -1         # include/k22.h: K22_EINVAL


def _x0(item):
    N, HW, g, cfg = item
    d = gr.item_input(*item)
    return d, sp.select_x0(d).numpy().reshape(N, 4 * HW)


def test_a_items_are_the_issues_and_the_layout():
    assert gr.ITEMS == ((8, 2304, 1, 1), (8, 255, 2, 1), (6, 1025, 1, 1), (4, 9216, 1, 1), (4, 16385, 1, 1), (2, 1, 1, 1), (3, 255, 1, 0), (8, 2304, 4, 1))
    assert [gr.layout(N, g, cfg) for (N, HW, g, cfg) in gr.ITEMS] == [(4, 4), (4, 2), (3, 3), (2, 2), (2, 2), (1, 1), (3, 3), (4, 1)]
    assert [sp.template_kpt(4 * HW) for (N, HW, g, cfg) in gr.ITEMS] == [16, 4, 16, 36, 0, 4, 4, 16]
    assert list(gr.row_s(np.array([10, 20], dtype=np.float32), 8, 2, 1)) == [10, 10, 20, 20, 10, 10, 20, 20]
    assert list(gr.row_s(np.array([10, 20, 30], dtype=np.float32), 3, 1, 0)) == [10, 20, 30]


@pytest.mark.parametrize("item", gr.ITEMS)
def test_a_host_model_per_group_is_numpys_percentile(item):
    N, HW, g, cfg = item
    d, x0 = _x0(item)
    assert torch.equal(sp.select_x0(d), d["x"])                  # the clamp clamps nothing: the keys are what the item wrote
    want, got = gr.group_s(x0, N, g, cfg), gr.group_s(x0, N, g, cfg, emul=True)
    assert [sp.f32bits(v) for v in got] == [sp.f32bits(v) for v in want], (item, got, want)
    half, G = gr.layout(N, g, cfg)
    for j in range(G):                                           # every other row of a group differs from its source row
        for r in range(N):
            if r != j * g and (r % half) // g == j:
                assert not np.array_equal(x0[r], x0[j * g]), (item, j, r)


def test_b_the_items_resolve_the_grouping():
    labels, ties, clamped, above = set(), set(), 0, 0
    for item in gr.ITEMS:
        N, HW, g, cfg = item
        d, x0 = _x0(item)
        half, G = gr.layout(N, g, cfg)
        S = gr.group_s(x0, N, g, cfg)
        lo = percentile_index(4 * HW)[0]
        # the condition the wrong variants depend on: every group but group 0 itself differs from group 0 in the bits of s
        assert sum(sp.f32bits(S[j]) != sp.f32bits(S[0]) for j in range(1, G)) == G - 1, (item, S)
        if G >= 2:
            assert (S == 1).any() and (S > 1).any(), (item, S)
        clamped, above = clamped + int((S == 1).sum()), above + int((S > 1).sum())
        for j in range(1, G):
            labels.add(sp.dispatch(x0[j * g], lo).label)
            ties.add(gr.group_case(j, 4 * HW)[0])
        print(f"{item}: s per group {[float(v) for v in S]}, paths {[sp.dispatch(x0[j * g], lo).label for j in range(G)]}")
    assert clamped >= 1 and above >= 1
    assert "fall-back" in labels and "generic" in labels and "filtered" in labels and "plain" in labels        # taken by NON-zero groups
    assert ties & set(sp.TIE_CASES)


@pytest.mark.parametrize("mutant", gr.MUTANTS)
def test_b_wrong_groupings_fail_the_gpu_tests_checks(mutant):
    """The GPU test holds s_buf[j] to numpy's percentile of row j g (equal bits) and x0_out to clamp(x0_buf, -s, s) / s with each row's own s
    under sampler_ref.final_bounds.  A wrong implementation is modelled by the s it applies to every row: it must fail one of the two."""
    caught = []
    for item in gr.ITEMS:
        N, HW, g, cfg = item
        d, x0 = _x0(item)
        half, G = gr.layout(N, g, cfg)
        S = gr.group_s(x0, N, g, cfg)
        wrong = gr.mutant_row_s(x0, N, g, cfg, mutant)
        s_buf_differs = any(sp.f32bits(wrong[j * g]) != sp.f32bits(S[j]) for j in range(G))
        x0_buf = torch.from_numpy(x0).view(N, 4, HW)
        _, z, Sx = gr.final_ref(x0_buf, S, d, sp.table()[sp.SELECT_ROW], N, g, cfg)
        w = torch.from_numpy(wrong).view(N, 1, 1)
        z_wrong = torch.minimum(torch.maximum(x0_buf, -w), w) / w          # fp32, as the kernel evaluates it
        x0_out_fails = sp.violations(z_wrong, z, sp.final_bounds(z, Sx, True)[1])[0] > 0
        if s_buf_differs or x0_out_fails:
            caught.append(item)
    print(f"wrong grouping '{mutant}': fails at {len(caught)} of {len(gr.ITEMS)} items")
    # every item with more than one group catches it; the group index without % half shows under CFG only (without it n % half is n)
    for item in gr.ITEMS:
        N, HW, g, cfg = item
        if gr.layout(N, g, cfg)[1] > 1 and (cfg or mutant != "no_mod"):
            assert item in caught, (mutant, item)


def test_b_the_reference_with_each_rows_own_s_is_the_one_group_reference_at_g_equal_half():
    N, HW, g, cfg = gr.ITEMS[-1]
    d, x0 = _x0(gr.ITEMS[-1])
    x0_buf = torch.from_numpy(x0).view(N, 4, HW)
    S = gr.group_s(x0, N, g, cfg)
    row = sp.table()[sp.SELECT_ROW]
    for a, b in zip(gr.final_ref(x0_buf, S, d, row, N, g, cfg), sp.final_ref(x0_buf, S[0], d, row)):
        assert torch.equal(a, b)


# ---- (c) the C entries on the host ------------------------------------------------------------------------------------------------------------------
def test_c_entries_are_exported_and_refuse_without_a_device():
    L = _lib.lib()
    assert hasattr(L, "k22_sampler_step_groups") and hasattr(L, "k22_unet_set_threshold_group")

    def step(pct_group, N=8, HW=16, cfg=1, pct_index=3):
        rc = L.k22_sampler_step_groups(None, None, None, None, None, None, 0, 4.0, cfg, -2.0, 2.0, pct_index, 0.5, pct_group, None, None, None, N, HW, None)
        return rc, (L.k22_last_error() or b"").decode()

    for pct_group in (0, -1, 3, 8):                   # below 1; 3 and 8 do not divide the cond half of 4
        rc, text = step(pct_group)
        assert rc == _EINVAL and "pct_group" in text, (pct_group, rc, text)
    rc, text = step(1, N=130, cfg=0)                  # 130 groups
    assert rc == _EINVAL and "64" in text
    rc, text = step(1, N=130, cfg=1)                  # 65 groups
    assert rc == _EINVAL and "64" in text
    # whatever k22_sampler_step refuses: an empty batch, an odd batch under CFG, a rank beyond the image
    for kw in (dict(N=0), dict(HW=0), dict(N=3), dict(pct_index=64), dict(pct_index=99)):
        rc, text = step(1, **kw)
        assert rc == _EINVAL and text.startswith("sampler"), (kw, rc, text)
    assert L.k22_unet_set_threshold_group(None, 1) == _EINVAL and b"unet_set_threshold_group" in L.k22_last_error()


def test_c_threshold_group_of_the_python_side():
    assert sampling.threshold_group(None, 8) is None
    assert sampling.threshold_group(4, 8) is None               # the whole cond half: the call as it has always been
    assert sampling.threshold_group(1, 8) == 1 and sampling.threshold_group(2, 8) == 2
    assert sampling.threshold_group(1, 3, use_cfg=False) == 1 and sampling.threshold_group(3, 3, use_cfg=False) is None
    for bad in (0, -1, 3, 8, 1.5):
        with pytest.raises(ValueError):
            sampling.threshold_group(bad, 8)
    with pytest.raises(ValueError):
        sampling.threshold_group(1, 260)                        # 130 groups
