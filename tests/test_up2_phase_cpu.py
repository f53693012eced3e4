"""The fold behind the four-phase upsampling convolution (kandinsky-2_amd/pack.py: fold_up2, csrc/conv3_up2.hip), on the CPU.

nearest-2x-upsample + conv3x3 (the in_layers of an up-sampling ResBlock) = four 2x2 convolutions of the low-resolution tensor, one per output
phase (py, px); each phase weight is a sum of 1, 2 or 4 of the original taps.  Checked here: the fp32 fold against the float64 fold within the
bound of three fp32 additions, the identity itself in float64 on ragged sizes, every phase / tap membership one by one, and that a fold with
two phases swapped is caught.  The packed arena entry (padded rows, one rounding after the sum) is checked against the same fold."""
import pytest
import torch
import torch.nn.functional as F

import kandinsky2_amd as k22
from kandinsky2_amd.pack import UP2_TAPS, fold_up2, packed_entries, to_x3

U24 = 2.0 ** -24


def phase_form(x, f, bias=None):
    """x [B,I,H,W], f [4][O][4][I] (fold_up2's layout) -> [B,O,2H,2W]: phase (py, px) = the 2x2 convolution of the zero-bordered x whose
    window starts at low-resolution (y + py - 1, x + px - 1), written to the output pixels (2y + py, 2x + px)."""
    B, I, H, W = x.shape
    O = f.shape[1]
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros(B, O, 2 * H, 2 * W, dtype=x.dtype)
    for py in (0, 1):
        for px in (0, 1):
            w = f[2 * py + px].reshape(O, 2, 2, I).permute(0, 3, 1, 2)               # [O][I][a][b]
            y = F.conv2d(xp[:, :, py:py + H + 1, px:px + W + 1], w)                    # window (a, b) of output (y, x) = xp[y + py + a, x + px + b]
            out[:, :, py::2, px::2] = y
    if bias is not None:
        out = out + bias[None, :, None, None]
    return out


def upsample_conv(x, w, bias=None):
    return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, bias, padding=1)


def rand_w(O, I, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(O, I, 3, 3, generator=g)


def test_fp32_fold_is_the_float64_fold_within_three_additions():
    w = rand_w(24, 40, 0)
    f32, f64 = fold_up2(w), fold_up2(w.double())
    assert f32.dtype == torch.float32 and f32.shape == (4, 24, 4, 40)
    bound = 3 * U24 * fold_up2(w.double().abs())           # sum |w| over the taps of each element
    assert bool(((f32.double() - f64).abs() <= bound).all())
    # the corner phases hold single taps: exact
    assert torch.equal(f32[0, :, 0], w[:, :, 0, 0]) and torch.equal(f32[3, :, 3], w[:, :, 2, 2])


@pytest.mark.parametrize("B,I,O,H,W", [(2, 5, 7, 5, 3), (1, 3, 2, 1, 1), (2, 4, 6, 2, 9), (1, 8, 3, 12, 20)])
def test_four_phase_form_is_the_upsampled_convolution_in_float64(B, I, O, H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = (0.3 + 1.7 * torch.randn(B, I, H, W, generator=g)).double()
    w = rand_w(O, I, 1).double()
    bias = torch.randn(O, generator=g).double()
    ref = upsample_conv(x, w, bias)
    out = phase_form(x, fold_up2(w), bias)
    scale = F.conv2d(F.interpolate(x.abs(), scale_factor=2, mode="nearest"), w.abs(), bias.abs(), padding=1).max().item()
    assert (out - ref).abs().max().item() < 1e-12 * scale


def test_every_phase_and_tap_membership():
    """one-hot weights: tap (ky, kx) must land in exactly slot (a, b) of phase (py, px) with a = floor((py + ky - 1) / 2) - (py - 1), columns
    alike - the table of the derivation, spelled independently of UP2_TAPS"""
    assert UP2_TAPS == (((0,), (1, 2)), ((0, 1), (2,)))
    for ky in range(3):
        for kx in range(3):
            w = torch.zeros(1, 1, 3, 3)
            w[0, 0, ky, kx] = 1.0
            f = fold_up2(w)[:, 0, :, 0]                      # [phase][tap]
            want = torch.zeros(4, 4)
            for py in (0, 1):
                for px in (0, 1):
                    a = (py + ky - 1) // 2 - (py - 1)
                    b = (px + kx - 1) // 2 - (px - 1)
                    assert a in (0, 1) and b in (0, 1)
                    want[2 * py + px, 2 * a + b] = 1.0
            assert torch.equal(f, want), (ky, kx)
    # counts: phase (0,0) sums 1 / 2 / 2 / 4 taps in its slots, phase (1,1) 4 / 2 / 2 / 1
    ones = fold_up2(torch.ones(1, 1, 3, 3))[:, 0, :, 0]
    assert ones.tolist() == [[1, 2, 2, 4], [2, 1, 4, 2], [2, 4, 1, 2], [4, 2, 2, 1]]


@pytest.mark.parametrize("swap", [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3)])
def test_a_fold_with_two_phases_swapped_fails(swap):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 5, 3, generator=g).double()
    w = rand_w(6, 4, 2).double()
    f = fold_up2(w).clone()
    i, j = swap
    f[[i, j]] = f[[j, i]]
    ref = upsample_conv(x, w)
    assert (phase_form(x, f) - ref).abs().max().item() > 1e-3 * ref.abs().max().item()


def test_arena_entry_is_the_fold_rounded_once():
    arch = k22.make_arch(k22.tiny_model_config())
    sd = k22.init_unet_state_dict(arch, seed=1)
    ups = [b[1] for b in arch.blocks if b[0] == "res" and b[4] == 2]
    assert len(ups) == len(arch.channel_mult) - 1
    ent32 = packed_entries(arch, sd, torch.float32, "cpu")
    ent16 = packed_entries(arch, sd, torch.bfloat16, "cpu")
    entx3 = packed_entries(arch, sd, k22.F16X3, "cpu")
    for pfx in ups:
        name = pfx + ".in_layers.2.weight_up2"
        w = sd[pfx + ".in_layers.2.weight"].float()
        O, I = w.shape[:2]
        Op = (O + 63) // 64 * 64
        f = fold_up2(w).reshape(4, O, 4 * I)
        assert ent32[name].shape == (4, Op, 4 * I) and torch.equal(ent32[name][:, :O], f) and not ent32[name][:, O:].any()
        assert torch.equal(ent16[name][:, :O], f.to(torch.bfloat16))                      # summed in fp32, rounded after the sum
        assert torch.equal(entx3[name].view(torch.int32), to_x3(ent32[name]).view(torch.int32))   # folded first, split afterwards
        assert pfx + ".in_layers.2.weight" in ent32                                         # the 9-tap weights stay
    assert not any(k.endswith("weight_up2") and k.rsplit(".in_layers", 1)[0] not in ups for k in ent32)
