"""Float64 restatement, inputs, mutants and bound of the flash attention (csrc/attention.hip: attention_kernel, attention_pipe_kernel) and of
its operand packer (csrc/elementwise.hip: kv_pack_kernel), for tests/test_attention_parity_cpu.py and tests/test_attention_parity_gpu.py.
A plain module like aux_ref.py, whose helpers it reuses.

Operation:  out[b][t][h] = softmax_j(scale * q_t . k_j + mask) v_j,  keys j = [context 0..S-1 | self S..S+T-1], scale = 1 / 8, 64 channels
per head.  Key j is dead for query t of image b when  j >= Tk,  or  causal and j > t,  or  j < kv_n and key_valid[b][j] == 0.
Precondition (include/k22.h): every query keeps at least one alive key.

Operands as the arithmetic is promised to see them (`seen`): bf16 / fp16 T-rounded, fp32 exact, x3 = hi + lo of the x3 chunks, x2 = the fp16
rounding of the fp32 values.

Bound, per element, not taken from any kernel (attention_ref returns ref, A = sum_j w_j |v_j| and amp = scale max_alive sum_d |q_d| |k_jd|):

    |out - ref| <= (u_P + c 2^-24 (4 + 2 amp)) A + e_sub + u_store |ref|

 u_P      the rounding of P in front of the P V product (the row sum is taken over the unrounded P): 2^-8 bf16, 2^-11 fp16 / x2, 2^-22 x3, 0 fp32
 e_sub    2^-25 sum_alive |v_j| / l64 for the fp16-P types (fp16, x2): P below fp16's normal range is rounded to a multiple of 2^-24;
          l64 >= 1 is the float64 row sum of exp(s - max)
 u_store  one rounding of the stored type: 2^-8 bf16, 2^-11 fp16 (aux_ref.rounding: never under the subnormal spacing), 2^-24 fp32 (also the
          split types' plain output), 2^-22 where x3 chunks are stored
 c        aux_ref.c_rule: 4 while the yardstick stays under 2, otherwise twice the yardstick.  The yardstick is torch's OWN fp32
          softmax(q k^T scale + mask) @ v on the same operands:  max |fp32 - float64| / (2^-24 (4 + 2 amp) A).  MEASURED, largest over
          the five operand types, per family (rand / edges / neg / spike) over all cases below:
            CPU    (test_attention_parity_cpu.py prints them)   rand 1.13   edges 1.55   neg 1.56   spike 0.20
            MI355X (test_attention_parity_gpu.py prints them)   rand 1.05   edges 1.34   neg 1.22   spike 0.16
          All under 2 -> c = 4.  The GPU test asserts that torch itself stays under c on every case.  Never set from a kernel's output.
          For orientation only (MI355X, largest |out - ref| / bound over all cases and families, pipe / plain kernel): bf16 0.71 / 0.80,
          fp16 0.75 / 0.80, x2 0.66 / 0.85, fp32 0.38, x3 0.19 (0.25 with the x3-chunk store); the CPU emulation of the scheme: bf16 0.80,
          fp16 0.80, fp32 0.31.  x3 read 1.03 on (2, 81, 40, 77) causal / neg while P was split unscaled: the lo half of a probability
          under 2^-3 is a fp16 subnormal (2^-25 absolute where u_P promises 2^-22 relative); attention_kernel now splits 2^10 P.

Input families (seeded; u = (+1, -1, +1, ...) / 8, a unit vector over the 64 channels): base q, k = 1.5 randn, v = 0.3 + 1.7 randn.
 rand   the base inputs
 edges  q += 4 u; every edge key - {0, S-1, S, 63, 64, 127, 128, Tk-2, Tk-1, Tk // 2} and, masked, n_valid-1, n_valid, kv_n-1, kv_n, where
        in range - gets k += 8 u (+4 on the scaled logit: a weight comparable to all other keys together) and the V row
        10 + key % 7 + arange(64) / 8
 neg    q += 4 u, k -= 12 u: every real logit is about -6, so that a pad key alive by mistake (logit 0) dominates the row
 spike  base inputs, one self key in the third 64-key tile = 16 x the query row 3: it dominates that query (scaled logit ~ 290) and raises
        the running maximum of the others late (the online-softmax rescale branch)

Mutants (`mut`, one deliberately wrong reference each; part (c) of the CPU test shows that the families reject them under every type's
bound): last_key_dropped, one_pad_key_alive (K = V = 0 at key Tk), causal_strict (key >= t dead, query 0 keeps key 0), causal_plus1
(key t + 1 alive), kvn_ignored (keys >= kv_n dead), v_swapped_at_S (V rows S-1 and S exchanged), ctx_after_self (V rows packed
[self | context] against K's [context | self].  Exchanging both consistently permutes the keys of an unmasked softmax and leaves the output
unchanged: that form of the mistake is what the exact K_all / V^T_all check is for, pack_ref(mut="ctx_after_self")).
"""
import collections

import torch

import aux_ref as ar
import helpers as hp
from kandinsky2_amd import _lib
from kandinsky2_amd.pack import to_x3

BF16, F16, F32, X3, X2 = _lib.K22_BF16, _lib.K22_F16, _lib.K22_F32, _lib.K22_F16X3, _lib.K22_F16X2
DTYPES = (BF16, F16, F32, X3, X2)
DT_NAME = hp.DT_NAME
U24 = hp.U24
SCALE = 0.125
HD = 64

# the rule applied to the larger of the CPU and the MI355X reading (tables above)
YARD_CPU, YARD_GPU = 1.56, 1.34
ATT_C = ar.c_rule(max(YARD_CPU, YARD_GPU))

Case = collections.namedtuple("Case", "B H T S causal n_valid kv_n")   # n_valid None: no key_valid tensor

UNMASKED = [Case(B, H, T, S, 0, None, 0) for (B, H, T, S) in
            ((2, 2, 64, 87), (1, 1, 100, 5), (2, 1, 33, 31), (1, 2, 129, 63), (1, 1, 200, 56), (1, 1, 1, 1), (2, 2, 160, 77), (3, 3, 130, 0))]
MASKED = [Case(B, 2, T, 0, causal, nv, kvn) for (B, T, nv, kvn) in ((2, 81, 40, 77), (2, 130, 100, 128), (1, 64, 9, 64), (3, 65, 20, 30))
          for causal in (0, 1)] + [Case(2, 2, 77, 0, 1, None, 0)]
CASES = UNMASKED + MASKED
FAMILIES = ("rand", "edges", "neg")
SPIKE_CASE = Case(1, 1, 200, 56, 0, None, 0)
SPIKE_SELF_ROW, SPIKE_QUERY = 100, 3        # key 56 + 100 = 156: the third tile (keys 128..191)
MUTANTS = ("last_key_dropped", "one_pad_key_alive", "causal_strict", "causal_plus1", "kvn_ignored", "v_swapped_at_S", "ctx_after_self")


def case_id(c):
    s = f"B{c.B}H{c.H}T{c.T}S{c.S}"
    if c.causal:
        s += "-causal"
    if c.n_valid is not None:
        s += f"-nv{c.n_valid}-kvn{c.kv_n}"
    return s


def masked(c):
    return bool(c.causal) or c.n_valid is not None


def u_vec():
    return torch.where(torch.arange(HD) % 2 == 0, 1.0, -1.0) / 8.0


def key_valid(c):
    """[B][kv_n] fp32, image b: max(1, n_valid - 3 b) leading ones; None without a key_valid tensor"""
    if c.n_valid is None:
        return None
    kv = torch.zeros(c.B, c.kv_n)
    for b in range(c.B):
        kv[b, :max(1, c.n_valid - 3 * b)] = 1.0
    return kv


def edge_keys(c):
    Tk = c.S + c.T
    ks = {0, c.S - 1, c.S, 63, 64, 127, 128, Tk - 2, Tk - 1, Tk // 2}
    if c.n_valid is not None:
        ks |= {c.n_valid - 1, c.n_valid, c.kv_n - 1, c.kv_n}
    return sorted(k for k in ks if 0 <= k < Tk)


def inputs(c, family, seed=0):
    """fp32 CPU tensors: qkv [B][T][3][H][64] (q | k | v planes), ctx [B][S][2][H][64] (k | v) or None when S == 0, key_valid or None"""
    g = ar.gen(7000 + 131 * CASES_INDEX.get(c, 99) + 17 * seed)
    qkv = ar.rn(g, c.B, c.T, 3, c.H, HD)
    qkv[:, :, :2] *= 1.5
    qkv[:, :, 2] = 0.3 + 1.7 * qkv[:, :, 2]
    ctx = None
    if c.S:
        ctx = ar.rn(g, c.B, c.S, 2, c.H, HD)
        ctx[:, :, 0] *= 1.5
        ctx[:, :, 1] = 0.3 + 1.7 * ctx[:, :, 1]
    u = u_vec()
    if family == "edges":
        qkv[:, :, 0] += 4.0 * u
        for key in edge_keys(c):
            vrow = 10.0 + (key % 7) + torch.arange(HD) / 8.0
            if key < c.S:
                ctx[:, key, 0] += 8.0 * u
                ctx[:, key, 1] = vrow
            else:
                qkv[:, key - c.S, 1] += 8.0 * u
                qkv[:, key - c.S, 2] = vrow
    elif family == "neg":
        qkv[:, :, 0] += 4.0 * u
        qkv[:, :, 1] -= 12.0 * u
        if ctx is not None:
            ctx[:, :, 0] -= 12.0 * u
    elif family == "spike":
        qkv[:, SPIKE_SELF_ROW, 1] = 16.0 * qkv[:, SPIKE_QUERY, 0]
        qkv[:, SPIKE_SELF_ROW, 2] = 10.0 + torch.arange(HD) / 8.0
    else:
        assert family == "rand", family
    return {"qkv": qkv, "ctx": ctx, "key_valid": key_valid(c)}


CASES_INDEX = {c: i for i, c in enumerate(CASES)}


def seen(x, dtype):
    """float64 values the arithmetic `dtype` is promised to see of the fp32 tensor x"""
    if x is None:
        return None
    if dtype == X3:
        return hp.x3_value(to_x3(x, 1.0))
    if dtype in (F16, X2):
        return x.to(torch.float16).double()
    if dtype == BF16:
        return x.to(torch.bfloat16).double()
    return x.double()


def operands(d, dtype):
    """(q [B][H][T][64], k [B][H][Tk][64], v [B][H][Tk][64]) float64 as seen, keys = [context | self]"""
    qkv, ctx = seen(d["qkv"], dtype), seen(d["ctx"], dtype)
    q = qkv[:, :, 0].permute(0, 2, 1, 3)
    k, v = qkv[:, :, 1], qkv[:, :, 2]
    if ctx is not None:
        k, v = torch.cat([ctx[:, :, 0], k], 1), torch.cat([ctx[:, :, 1], v], 1)
    return q.contiguous(), k.permute(0, 2, 1, 3).contiguous(), v.permute(0, 2, 1, 3).contiguous()


def dead_mask(c, valid, Tk, device, mut=None):
    """bool [B][1][T][Tk]: key dead for the query"""
    t = torch.arange(c.T, device=device)[:, None]
    key = torch.arange(Tk, device=device)[None, :]
    dead = torch.zeros(c.B, 1, c.T, Tk, dtype=torch.bool, device=device)
    if c.causal:
        if mut == "causal_strict":
            cd = (key >= t) & ~((key == 0) & (t == 0))
        elif mut == "causal_plus1":
            cd = key > t + 1
        else:
            cd = key > t
        dead |= cd[None, None]
    if valid is not None:
        kd = torch.zeros(c.B, Tk, dtype=torch.bool, device=device)
        kd[:, :c.kv_n] = valid.to(device) == 0
        if mut == "kvn_ignored":
            kd[:, c.kv_n:] = True
        dead |= kd[:, None, None, :]
    if mut == "last_key_dropped" and Tk > 1:
        dead[..., Tk - 1] = True
    return dead


def rows(x):
    """[B][H][T][64] -> the output layout [B * T][H * 64]"""
    B, H, T, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, H * HD)


def attention_ref(q, k, v, c, valid=None, mut=None, info=None):
    """float64 (q, k, v as `operands` returns them) -> (ref [B * T][H * 64], A same shape, amp [B * T][H * 64] (constant over a head's
    channels)).  info (optional dict) receives e_sub's factor sum_alive |v_j| / l64 in the same layout."""
    S = c.S
    if mut == "v_swapped_at_S" and 1 <= S < k.shape[2]:
        v = v.clone()
        v[:, :, [S - 1, S]] = v[:, :, [S, S - 1]]
    if mut == "ctx_after_self" and S:
        v = torch.cat([v[:, :, S:], v[:, :, :S]], 2)
    Tk = k.shape[2]
    dead = dead_mask(c, valid, Tk, q.device, mut)
    if mut == "one_pad_key_alive":
        z = torch.zeros_like(k[:, :, :1])
        k, v = torch.cat([k, z], 2), torch.cat([v, z], 2)
        dead = torch.cat([dead, torch.zeros_like(dead[..., :1])], -1)
    dead = dead.expand(c.B, c.H, c.T, k.shape[2])
    s = (q @ k.transpose(-1, -2)) * SCALE
    s = s.masked_fill(dead, float("-inf"))
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    l = e.sum(-1, keepdim=True)
    w = e / l
    ref = w @ v
    A = w @ v.abs()
    amp = SCALE * (q.abs() @ k.abs().transpose(-1, -2)).masked_fill(dead, 0.0).max(-1, keepdim=True).values
    if info is not None:
        info["vsum_over_l"] = rows(((~dead).to(v.dtype) @ v.abs()) / l)
    return rows(ref), rows(A), rows(amp.expand_as(ref))


def plain32(q, k, v, c, valid=None):
    """the yardstick's evaluation: torch's own fp32 softmax(q k^T scale + mask) @ v on the same operands"""
    q, k, v = q.float(), k.float(), v.float()
    add = torch.zeros(c.B, 1, c.T, k.shape[2], dtype=torch.float32, device=q.device).masked_fill(dead_mask(c, valid, k.shape[2], q.device), float("-inf"))
    return rows(torch.softmax((q @ k.transpose(-1, -2)) * SCALE + add, -1) @ v)


def yardstick(v32, ref, A, amp):
    return ((v32.double() - ref).abs() / (U24 * (4.0 + 2.0 * amp) * A).clamp_min(1e-300)).max().item()


def u_P(dtype):
    return {BF16: 2.0 ** -8, F16: 2.0 ** -11, X2: 2.0 ** -11, X3: 2.0 ** -22, F32: 0.0}[dtype]


def store_rounding(ref, dtype, out_x3=0):
    """u_store |ref|, for fp16 with the subnormal floor of aux_ref.rounding"""
    if dtype in (X3, X2):
        return (2.0 ** -22 if out_x3 else U24) * ref.abs()
    return ar.rounding(ref, dtype)


def bound(ref, A, amp, vsum_over_l, dtype, out_x3=0, c=None):
    c = ATT_C if c is None else c
    e_sub = 2.0 ** -25 * vsum_over_l if dtype in (F16, X2) else 0.0
    return (u_P(dtype) + c * U24 * (4.0 + 2.0 * amp)) * A + e_sub + store_rounding(ref, dtype, out_x3)


def ref_and_bound(d, c, dtype, out_x3=0, mut=None):
    """inputs dict (any device) -> (ref, bound, (q, k, v, A, amp)) of the case as `dtype` sees it"""
    q, k, v = operands(d, dtype)
    info = {}
    ref, A, amp = attention_ref(q, k, v, c, d["key_valid"], mut, info)
    return ref, bound(ref, A, amp, info["vsum_over_l"], dtype, out_x3), (q, k, v, A, amp)


def as_stored(x64, dtype, out_x3=0):
    """what a kernel that computed x64 exactly would leave in memory, as float64"""
    if dtype in (X3, X2):
        return hp.x3_value(to_x3(x64.float(), 1.0)) if out_x3 else x64.float().double()
    return x64.to(hp.tdt(dtype)).double()


def storage(x, dtype):
    """the tensor the C entry point is given for the fp32 values x: T for the plain types, the fp32 tensor itself for the split ones"""
    return x.to(hp.storage_T(dtype)).contiguous()


def pack_ref(d, c, dtype, mut=None):
    """K_all [B][H][Tkp][64] and V^T_all [B][H][64][Tkp] in the storage type: the operands bit for bit, zero from key Tk on"""
    T = hp.storage_T(dtype)
    qkv = d["qkv"].to(T)
    k, v = qkv[:, :, 1], qkv[:, :, 2]
    if d["ctx"] is not None:
        ctx = d["ctx"].to(T)
        parts = ([k, ctx[:, :, 0]], [v, ctx[:, :, 1]]) if mut == "ctx_after_self" else ([ctx[:, :, 0], k], [ctx[:, :, 1], v])
        k, v = torch.cat(parts[0], 1), torch.cat(parts[1], 1)
    Tk = c.S + c.T
    Tkp = (Tk + 63) // 64 * 64
    kall = torch.zeros(c.B, c.H, Tkp, HD, dtype=T, device=qkv.device)
    vtall = torch.zeros(c.B, c.H, HD, Tkp, dtype=T, device=qkv.device)
    kall[:, :, :Tk] = k.permute(0, 2, 1, 3)
    vtall[:, :, :, :Tk] = v.permute(0, 2, 3, 1)
    return kall, vtall


def emulate(q, k, v, c, valid, dtype):
    """the CPU prototype of the kernels' scheme: 64-key online softmax, fp32 scores and sums, P rounded to T in front of P V, the row sum
    over the unrounded P; output rounded to T.  bf16 / fp16 / fp32."""
    T = hp.tdt(dtype)
    q, k, v = q.float(), k.float(), v.float()
    Tk = k.shape[2]
    dead = dead_mask(c, valid, Tk, q.device).expand(c.B, c.H, c.T, Tk)
    cexp = torch.tensor(SCALE * 1.4426950408889634, dtype=torch.float32)
    m = torch.full((c.B, c.H, c.T, 1), -1e30, dtype=torch.float32)
    l = torch.zeros_like(m)
    o = torch.zeros(c.B, c.H, c.T, HD, dtype=torch.float32)
    for k0 in range(0, Tk, 64):
        s = (q @ k[:, :, k0:k0 + 64].transpose(-1, -2)).masked_fill(dead[..., k0:k0 + 64], float("-inf"))
        m_new = torch.maximum(m, s.max(-1, keepdim=True).values)
        alpha = torch.exp2((m - m_new) * cexp)
        p = torch.exp2(s * cexp - m_new * cexp)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p.to(T).float() @ v[:, :, k0:k0 + 64]
        m = m_new
    return rows(o / l).to(T)


def to_dev(d, device):
    return ar.to_dev(d, device)
