"""Float64 restatement, inputs, mutants and bound of the fused MoVQ attention (csrc/movq_attention.hip, k22_movq_attention), for
tests/test_movq_attention_cpu.py and tests/test_movq_attention_gpu.py.  A plain module like attention_ref.py, whose bound it restates.

Operation, per image b and query t:  out[b][t][:] = sum_j softmax_j(C^-1/2 q_t . k_j) v_j + bias_v,  j = 0 .. T-1, one head of C channels,
no mask.  q, k, v are [B][T][C] (the kernel is handed V^T [B][C][T]); bias_v is fp32 [C] and is added after the normalisation.

Operands as the arithmetic is promised to see them (`seen`): bf16 / fp16 T-rounded, fp32 exact; bias_v always fp32.

Bound, per element, not taken from any kernel (attention_ref returns ref, A = sum_j w_j |v_j| and amp = C^-1/2 max_j sum_d |q_d| |k_jd|):

    |out - ref| <= (u_P + c 2^-24 (4 + 2 amp)) A + e_sub + u_store |ref|

 u_P      the rounding of P in front of the P V product (the row sum is taken over the unrounded P): 2^-8 bf16, 2^-11 fp16, 0 fp32
 e_sub    2^-25 sum_j |v_j| / l64 for fp16: P below fp16's normal range is rounded to a multiple of 2^-24; l64 >= 1 is the float64 row sum of
          exp(s - max)
 u_store  one rounding of the stored type: 2^-8 bf16, 2^-11 fp16 (aux_ref.rounding: never under the subnormal spacing), 2^-24 fp32
 c        aux_ref.c_rule: 4 while the yardstick stays under 2, otherwise twice the yardstick.  The yardstick is torch's OWN fp32
          softmax(q k^T C^-1/2) @ v + bias_v on the same operands:  max |fp32 - float64| / (2^-24 (4 + 2 amp) A).  MEASURED, largest over the
          three operand types, per family over all cases below:
            CPU    (test_movq_attention_cpu.py prints them)   rand 0.99   edges 1.32   spike 0.43
            MI355X (test_movq_attention_gpu.py prints them)   rand 1.19   edges 1.45   spike 0.53
          All under 2 -> c = 4.  The GPU test asserts that torch itself stays under c on every case.  Never set from a kernel's output.
          For orientation only (largest |out - ref| / bound over all cases and families): k22_movq_attention on the MI355X bf16 0.857,
          fp16 0.811, fp32 0.200; the CPU emulation of the scheme bf16 0.857, fp16 0.811, fp32 0.288.

Cases (B, T, C), each the smallest shape with its edge: (1, 64, 128) one tile, narrowest head; (2, 64, 512) one tile, full width, two
images; (1, 128, 512) two 64-key tiles and two 64-query blocks; (2, 192, 256) a query count that is no multiple of 128, third key tile;
(1, 320, 384) the odd width, five tiles; (1, 1024, 512) 256 px, the smallest real size.

Input families (seeded; u = (+1, -1, +1, ...) / sqrt(C), a unit vector over the channels): base q, k = 1.5 randn (scaled logits have a
standard deviation of 2.25 at every C: O(10) at the row maximum), v = 0.3 + 1.7 randn, bias_v = randn.
 rand   the base inputs
 edges  q += 2 C^1/4 u; every edge key - {0, 63, 64, 127, 128, T-2, T-1, T/2}, where in range - gets k += 2 C^1/4 u (+4 on the scaled logit:
        a weight comparable to all other keys together) and the V row 10 + key % 7 + arange(C) / 8
 spike  (T >= 192) key 150, in the third 64-key tile, = 128 C^-1/2 x the query row 3: it dominates that query (scaled logit ~ 290) and raises
        the running maximum of the others late (the online-softmax rescale branch)

Mutants (`mut`, one deliberately wrong reference each; the CPU test shows that cases x families reject each under every type's bound):
last_tile_dropped (keys T-64 .. T-1 dead; T > 64), bias_omitted, scale_unet (1 / 8 instead of C^-1/2), v_rows_63_64_swapped (T > 64),
first_quarter_channels_only (q . k over d < C / 4: the forgotten cross-wave sum), rescale_skipped (online softmax over 64-key tiles whose
running sum is not rescaled when the maximum rises).
"""
import functools

import torch

import aux_ref as ar
import helpers as hp
from kandinsky2_amd import _lib

BF16, F16, F32 = _lib.K22_BF16, _lib.K22_F16, _lib.K22_F32
DTYPES = (BF16, F16, F32)
DT_NAME = hp.DT_NAME
U24 = hp.U24

# the rule applied to the larger of the CPU and the MI355X reading (table above)
YARD_CPU, YARD_GPU = 1.32, 1.45
MQ_C = ar.c_rule(max(YARD_CPU, YARD_GPU))

CASES = ((1, 64, 128), (2, 64, 512), (1, 128, 512), (2, 192, 256), (1, 320, 384), (1, 1024, 512))
FAMILIES = ("rand", "edges", "spike")
SPIKE_KEY, SPIKE_QUERY = 150, 3
MUTANTS = ("last_tile_dropped", "bias_omitted", "scale_unet", "v_rows_63_64_swapped", "first_quarter_channels_only", "rescale_skipped")


def case_id(c):
    return "B%dT%dC%d" % c


def families(c):
    """the families a case takes: spike needs its key in the third 64-key tile"""
    return tuple(f for f in FAMILIES if f != "spike" or c[1] >= 192)


def pairs():
    return [(c, f) for c in CASES for f in families(c)]


def scale_of(C):
    return float(C) ** -0.5


def u_vec(C):
    return torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0) / float(C) ** 0.5


def edge_keys(T):
    return sorted(k for k in {0, 63, 64, 127, 128, T - 2, T - 1, T // 2} if 0 <= k < T)


@functools.lru_cache(maxsize=None)
def inputs(c, family):
    """fp32 CPU tensors q, k, v [B][T][C] and bias [C].  Cached: shared and never written to."""
    B, T, C = c
    g = ar.gen(9100 + 131 * CASES.index(c))
    q, k = 1.5 * ar.rn(g, B, T, C), 1.5 * ar.rn(g, B, T, C)
    v = ar.acts(g, B, T, C)
    bias = ar.rn(g, C)
    u = u_vec(C)
    if family == "edges":
        lift = 2.0 * float(C) ** 0.25
        q = q + lift * u
        for key in edge_keys(T):
            k[:, key] += lift * u
            v[:, key] = 10.0 + (key % 7) + torch.arange(C) / 8.0
    elif family == "spike":
        assert T >= 192
        k[:, SPIKE_KEY] = (128.0 * float(C) ** -0.5) * q[:, SPIKE_QUERY]
        v[:, SPIKE_KEY] = 10.0 + torch.arange(C) / 8.0
    else:
        assert family == "rand", family
    return {"q": q, "k": k, "v": v, "bias": bias}


def seen(x, dtype):
    """float64 values the arithmetic `dtype` is promised to see of the fp32 tensor x"""
    return x.to(hp.tdt(dtype)).double()


def operands(d, dtype):
    """(q, k, v [B][T][C], bias [C]) float64 as seen"""
    return seen(d["q"], dtype), seen(d["k"], dtype), seen(d["v"], dtype), d["bias"].double()


def attention_ref(q, k, v, bias, mut=None, info=None):
    """float64 operands -> (ref, A, amp), all [B][T][C] (amp constant over the channels).  info (optional dict) receives e_sub's factor
    sum_j |v_j| / l64."""
    B, T, C = q.shape
    sc = 0.125 if mut == "scale_unet" else scale_of(C)
    if mut == "v_rows_63_64_swapped" and T > 64:
        v = v.clone()
        v[:, [63, 64]] = v[:, [64, 63]]
    qs, ks = (q[..., :C // 4], k[..., :C // 4]) if mut == "first_quarter_channels_only" else (q, k)
    s = (qs @ ks.transpose(-1, -2)) * sc
    if mut == "last_tile_dropped" and T > 64:
        s[..., T - 64:] = float("-inf")
    if mut == "rescale_skipped":
        m = torch.full((B, T, 1), -1e300, dtype=torch.float64)
        l = torch.zeros_like(m)
        o = torch.zeros(B, T, C, dtype=torch.float64)
        for k0 in range(0, T, 64):
            st = s[..., k0:k0 + 64]
            m_new = torch.maximum(m, st.max(-1, keepdim=True).values)
            p = torch.exp(st - m_new)
            o = o * torch.exp(m - m_new) + p @ v[:, k0:k0 + 64]
            l = l + p.sum(-1, keepdim=True)           # the mistake: no exp(m - m_new) on the running sum
            m = m_new
        ref, w = o / l, None
    else:
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        l = e.sum(-1, keepdim=True)
        w = e / l
        ref = w @ v
    if mut != "bias_omitted":
        ref = ref + bias
    if w is None:
        return ref, None, None
    A = w @ v.abs()
    amp = scale_of(C) * (q.abs() @ k.abs().transpose(-1, -2)).max(-1, keepdim=True).values
    if info is not None:
        info["vsum_over_l"] = v.abs().sum(1, keepdim=True) / l
    return ref, A, amp.expand_as(ref)


def plain32(q, k, v, bias):
    """the yardstick's evaluation: torch's own fp32 softmax(q k^T C^-1/2) @ v + bias on the same operands (any device)"""
    q, k, v = q.float(), k.float(), v.float()
    return torch.softmax((q @ k.transpose(-1, -2)) * scale_of(q.shape[-1]), -1) @ v + bias.float()


def yardstick(v32, ref, A, amp):
    return ((v32.double() - ref).abs() / (U24 * (4.0 + 2.0 * amp) * A).clamp_min(1e-300)).max().item()


def u_P(dtype):
    return {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 0.0}[dtype]


def bound(ref, A, amp, vsum_over_l, dtype, c=None):
    c = MQ_C if c is None else c
    e_sub = 2.0 ** -25 * vsum_over_l if dtype == F16 else 0.0
    return (u_P(dtype) + c * U24 * (4.0 + 2.0 * amp)) * A + e_sub + ar.rounding(ref, dtype)


@functools.lru_cache(maxsize=None)
def ref_and_bound(c, family, dtype):
    """(ref, bound, (q, k, v, bias, A, amp)) of the case as `dtype` sees it, float64 on the CPU.  Cached: shared and never written to."""
    q, k, v, bias = operands(inputs(c, family), dtype)
    info = {}
    ref, A, amp = attention_ref(q, k, v, bias, None, info)
    return ref, bound(ref, A, amp, info["vsum_over_l"], dtype), (q, k, v, bias, A, amp)


def mutant_ref(c, family, dtype, mut):
    q, k, v, bias = operands(inputs(c, family), dtype)
    return attention_ref(q, k, v, bias, mut)[0]


def worst_ratio(out64, ref, bnd):
    return ((out64 - ref).abs() / bnd.clamp_min(1e-300)).max().item()


def emulate(q, k, v, bias, dtype):
    """the CPU prototype of the kernel's scheme in float32: 64-key tiles, online maximum and sum, P rounded to T in front of P V, the row
    sum over the unrounded P, bias after the normalisation; output rounded to T.  (The kernel's tile is 32 keys: the contract and the bound
    do not depend on the tile.)"""
    T_ = hp.tdt(dtype)
    q, k, v, bias = q.float(), k.float(), v.float(), bias.float()
    B, T, C = q.shape
    cexp = torch.tensor(scale_of(C) * 1.4426950408889634, dtype=torch.float32)
    m = torch.full((B, T, 1), -1e30, dtype=torch.float32)
    l = torch.zeros_like(m)
    o = torch.zeros(B, T, C, dtype=torch.float32)
    for k0 in range(0, T, 64):
        s = q @ k[:, k0:k0 + 64].transpose(-1, -2)
        m_new = torch.maximum(m, s.max(-1, keepdim=True).values)
        alpha = torch.exp2((m - m_new) * cexp)
        p = torch.exp2(s * cexp - m_new * cexp)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p.to(T_).float() @ v[:, k0:k0 + 64]
        m = m_new
    return (o / l + bias).to(T_)


def storage(x, dtype):
    """the tensor the C entry is given for the fp32 values x"""
    return x.to(hp.tdt(dtype)).contiguous()
