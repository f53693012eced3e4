"""CPU half of the float64 parity of the flash attention (tests/attention_ref.py, tests/test_attention_parity_gpu.py):
 (a) the float64 restatement equals the oracle's own expressions (QKVAttention's einsum form, the prior's additive mask);
 (b) the yardstick - torch's own fp32 evaluation - is printed and stays under c on every case and family, and a CPU emulation of the
     kernels' scheme (64-key online softmax, fp32 scores and sums, P rounded to T) stays inside the bound for bf16, fp16 and fp32;
 (c) resolving power: every mutant of the reference, in its best case (its exact float64 value rounded once to the stored type), is rejected
     by the family meant for it on at least 5 % of a case's elements under the bound of every type."""
import math

import pytest
import torch

import attention_ref as at
from oracle import unet_ref

DT_IDS = [at.DT_NAME[d] for d in at.DTYPES]
FLOOR = 0.05


def close(a, b, tol=1e-12):
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


_INPUTS = {}


def inputs(c, fam):
    if (c, fam) not in _INPUTS:
        _INPUTS[(c, fam)] = at.inputs(c, fam)
    return _INPUTS[(c, fam)]


def all_inputs():
    for c in at.CASES:
        for fam in at.FAMILIES:
            yield c, fam
    yield at.SPIKE_CASE, "spike"


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------
def test_a_unmasked_matches_the_oracles_einsum_form():
    c = at.UNMASKED[0]                                                  # (2, 2, 64, 87)
    d = inputs(c, "rand")
    q, k, v = at.operands(d, at.F32)
    ref, _, _ = at.attention_ref(q, k, v, c)
    # QKVAttention's layout: qkv [bs][heads x (q | k | v) x ch][length], encoder_kv [bs][heads x (k | v) x ch][S]
    qkv = d["qkv"].double().permute(0, 3, 2, 4, 1).reshape(c.B, c.H * 3 * 64, c.T)
    ekv = d["ctx"].double().permute(0, 3, 2, 4, 1).reshape(c.B, c.H * 2 * 64, c.S)
    want = unet_ref.qkv_attention(qkv, ekv, c.H)                        # [bs][heads x ch][length]
    # the oracle takes its softmax in fp32 (`w.float()`, as the reference does): agreement to fp32 class, not to float64 class
    assert close(ref, want.permute(0, 2, 1).reshape(c.B * c.T, c.H * 64), tol=2e-6)


def test_a_masked_matches_the_priors_additive_mask():
    c = at.MASKED[1]                                                    # (2, 81, 40, 77) causal: the prior's shape
    assert c.causal and c.kv_n == 77 and c.T == 81
    d = inputs(c, "rand")
    q, k, v = at.operands(d, at.F32)
    ref, _, _ = at.attention_ref(q, k, v, c, d["key_valid"])
    # oracle/prior_ref.py: mask padded with True for the appended tokens, causal = -inf above the diagonal, both added to the scores
    x = d["qkv"].double()                                               # [B][n][3][H][ch]
    qq, kk, vv = x[:, :, 0], x[:, :, 1], x[:, :, 2]                     # [B][n][H][ch]
    mask = torch.nn.functional.pad(d["key_valid"] != 0, (0, c.T - c.kv_n), value=True)
    causal = torch.full((c.T, c.T), float("-inf")).triu_(1)[None]
    am = (torch.where(mask, 0.0, float("-inf"))[:, None, :] + causal).double()
    scale = 1 / math.sqrt(math.sqrt(64))
    w = torch.einsum("bthc,bshc->bhts", qq * scale, kk * scale) + am[:, None]
    w = torch.softmax(w, dim=-1)
    want = torch.einsum("bhts,bshc->bthc", w, vv).reshape(c.B * c.T, -1)
    assert close(ref, want)


def test_a_pack_ref_layout():
    c = at.UNMASKED[0]
    d = inputs(c, "rand")
    kall, vtall = at.pack_ref(d, c, at.F32)
    _, k, v = at.operands(d, at.F32)
    Tk = c.S + c.T
    assert torch.equal(kall[:, :, :Tk].double(), k) and torch.equal(vtall[:, :, :, :Tk].double(), v.transpose(-1, -2))
    assert bool((kall[:, :, Tk:] == 0).all()) and bool((vtall[:, :, :, Tk:] == 0).all())
    km, vm = at.pack_ref(d, c, at.F32, mut="ctx_after_self")           # the consistent exchange: only the exact check sees it
    assert (km != kall).float().mean().item() > 0.5 and (vm != vtall).float().mean().item() > 0.5


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------
def test_b_yardstick_and_emulation():
    yard = {}
    frac = {dt: 0.0 for dt in (at.BF16, at.F16, at.F32)}
    for c, fam in all_inputs():
        d = inputs(c, fam)
        for dt in at.DTYPES:
            ref, bnd, (q, k, v, A, amp) = at.ref_and_bound(d, c, dt)
            y = at.yardstick(at.plain32(q, k, v, c, d["key_valid"]), ref, A, amp)
            yard[fam] = max(yard.get(fam, 0.0), y)
            assert y < at.ATT_C, (at.case_id(c), fam, at.DT_NAME[dt], y)
            if dt in frac:
                out = at.emulate(q, k, v, c, d["key_valid"], dt)
                nbad, ratio = at.ar.violations(out, ref, bnd)
                frac[dt] = max(frac[dt], ratio)
                assert nbad == 0, (at.case_id(c), fam, at.DT_NAME[dt], nbad, ratio)
    print("torch fp32 yardstick (CPU), largest over cases and types: " + "  ".join(f"{f} {y:.2f}" for f, y in yard.items()) + f"  (c = {at.ATT_C})")
    print("emulation, largest |out - ref| / bound: " + "  ".join(f"{at.DT_NAME[dt]} {r:.2f}" for dt, r in frac.items()))
    assert at.ar.c_rule(max(yard.values())) <= at.ATT_C


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------
def mutant_cases(mut):
    """(families, cases) meant for the mutant"""
    if mut == "one_pad_key_alive":
        return ("neg",), [c for c in at.UNMASKED if (c.S + c.T) % 64]
    if mut == "last_key_dropped":
        return ("edges",), [c for c in at.UNMASKED if c.S + c.T > 1]
    if mut in ("v_swapped_at_S", "ctx_after_self"):
        return ("edges",), [c for c in at.UNMASKED if c.S >= 1]
    if mut in ("causal_strict", "causal_plus1"):
        return ("edges", "rand"), [c for c in at.MASKED if c.causal]
    assert mut == "kvn_ignored"
    return ("edges", "rand"), [c for c in at.MASKED if c.n_valid is not None and c.kv_n < c.T]


@pytest.mark.parametrize("mut", at.MUTANTS)
def test_c_mutant_is_rejected(mut):
    fams, cases = mutant_cases(mut)
    assert cases
    variants = [(dt, ox) for dt in at.DTYPES for ox in ((0, 1) if dt in (at.X3, at.X2) else (0,))]
    for dt, ox in variants:
        best, least = 0.0, 1.0
        for c in cases:
            for fam in fams:
                d = inputs(c, fam)
                ref, bnd, (q, k, v, _, _) = at.ref_and_bound(d, c, dt, ox)
                wrong, _, _ = at.attention_ref(q, k, v, c, d["key_valid"], mut)
                share = (~((at.as_stored(wrong, dt, ox) - ref).abs() <= bnd)).double().mean().item()
                ok = at.ar.violations(at.as_stored(ref, dt, ox), ref, bnd)[0]
                assert ok == 0                                          # the right value, rounded the same way, passes
                best, least = max(best, share), min(least, share)
        print(f"{mut} {at.DT_NAME[dt]}{'-x3out' if ox else ''}: rejected on {100 * least:.0f}-{100 * best:.0f} % of a case's elements ({len(cases) * len(fams)} case x family pairs)")
        assert best >= FLOOR, (mut, at.DT_NAME[dt], ox, best)
