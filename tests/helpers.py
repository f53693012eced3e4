"""Shared helpers of the parity tests: thin typed wrappers over the C ABI (through ctypes, exactly as the
product calls it) and torch fp32 references of single floating-point ops."""
import torch
import torch.nn.functional as F

from kandinsky2_amd import _lib


def tdt(dtype_code):
    return {_lib.K22_BF16: torch.bfloat16, _lib.K22_F16: torch.float16, _lib.K22_F32: torch.float32}[dtype_code]


def pad_rows(w, mult=64):
    o = w.shape[0]
    op = (o + mult - 1) // mult * mult
    if op == o:
        return w.contiguous()
    return torch.cat([w, torch.zeros((op - o,) + tuple(w.shape[1:]), dtype=w.dtype, device=w.device)], 0).contiguous()


def stream():
    return torch.cuda.current_stream().cuda_stream


def gemm(A0, W, bias=None, residual=None, A1=None, dtype=_lib.K22_BF16, splitk=1, bm=0, bn=0, out_f32=False, act=0):
    """A0 [M,K0], A1 [M,K1] or None, W [N,K0+K1] (all float32 cuda) -> out [M,N] (float32 copy) and the
    T-rounded operands actually used."""
    T = tdt(dtype)
    M, K0 = A0.shape
    K1 = 0 if A1 is None else A1.shape[1]
    N = W.shape[0]
    a0 = A0.to(T).contiguous()
    a1 = None if A1 is None else A1.to(T).contiguous()
    wp = pad_rows(W.to(T))
    res = None if residual is None else residual.to(T).contiguous()
    out = torch.empty(M, N, dtype=torch.float32 if out_f32 else T, device=A0.device)
    partial = torch.empty(max(1, abs(splitk) if splitk else 16) * M * N + 64, dtype=torch.float32, device=A0.device)
    _lib.check(_lib.lib().k22_gemm(
        a0.data_ptr(), _lib.ptr(a1), wp.data_ptr(), _lib.ptr(bias), _lib.ptr(res), out.data_ptr(), partial.data_ptr(),
        M, N, wp.shape[0], K0, K1, K0, K1, N, N, 1 if out_f32 else 0, act, splitk, bm, bn, dtype, stream()))
    a_full = a0.float() if a1 is None else torch.cat([a0.float(), a1.float()], 1)
    return out.float(), a_full, W.to(T).float(), (None if res is None else res.float())


def nhwc_padded(x, T):
    """[B,C,H,W] float -> zero-bordered NHWC [B,H+2,W+2,C] of dtype T."""
    return F.pad(x, (1, 1, 1, 1)).permute(0, 2, 3, 1).contiguous().to(T)


def pack_conv3(w, T):
    return pad_rows(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).to(T))


def conv3x3(x, w, bias=None, residual=None, dtype=_lib.K22_BF16, splitk=1, bm=0, bn=0, out_mode=0, algo=0, stats=False):
    """x [B,Cin,H,W], w [Cout,Cin,3,3], residual [B,Cout,H,W] (float32 cuda) -> NCHW float32.
    algo: 0 auto, 1 generic implicit GEMM, 2 LDS-resident halo kernel.  stats=True also returns the per-image,
    per-channel (sum, sumsq) reduced from the kernel's GroupNorm partial sums."""
    _lib.check(_lib.lib().k22_set_option(b"conv_algo", algo))
    try:
        return _conv3x3(x, w, bias, residual, dtype, splitk, bm, bn, out_mode, stats)
    finally:
        _lib.check(_lib.lib().k22_set_option(b"conv_algo", 0))


def _conv3x3(x, w, bias, residual, dtype, splitk, bm, bn, out_mode, stats):
    T = tdt(dtype)
    B, Cin, H, W_ = x.shape
    Cout = w.shape[0]
    xp = nhwc_padded(x, T)
    wp = pack_conv3(w, T)
    res = None if residual is None else residual.permute(0, 2, 3, 1).contiguous().to(T)
    if out_mode == _lib.OUT_NCHW_F32:
        out = torch.empty(B, Cout, H, W_, dtype=torch.float32, device=x.device)
    else:
        out = torch.empty(B, H, W_, Cout, dtype=T, device=x.device)
    partial = torch.empty(max(1, splitk if splitk else 16) * B * H * W_ * Cout + 64, dtype=torch.float32, device=x.device)
    st = None
    if stats:
        import ctypes as C
        cap = B * (H * (W_ + 2) // 16 + 2)
        sbuf = torch.full((cap, Cout, 2), float("nan"), dtype=torch.float32, device=x.device)
        rpi = C.c_int(0)
        _lib.check(_lib.lib().k22_conv3x3_gnstats(
            xp.data_ptr(), wp.data_ptr(), _lib.ptr(bias), _lib.ptr(res), out.data_ptr(), partial.data_ptr(),
            B, H, W_, Cin, Cout, wp.shape[0], splitk, bm, bn, sbuf.data_ptr(), cap, C.byref(rpi), dtype, stream()))
        st = sbuf[: B * rpi.value].view(B, rpi.value, Cout, 2).double().sum(1)  # [B, Cout, 2]
    else:
        _lib.check(_lib.lib().k22_conv3x3(
            xp.data_ptr(), wp.data_ptr(), _lib.ptr(bias), _lib.ptr(res), out.data_ptr(), partial.data_ptr(),
            B, H, W_, Cin, Cout, wp.shape[0], out_mode, 0, splitk, bm, bn, dtype, stream()))
    o = out.float() if out_mode == _lib.OUT_NCHW_F32 else out.float().permute(0, 3, 1, 2).contiguous()
    ref = F.conv2d(x.to(T).float(), w.to(T).float(), bias, padding=1)
    if res is not None:
        ref = ref + res.float().permute(0, 3, 1, 2)
    if stats:
        return o, ref, st
    return o, ref


def groupnorm(x0, gamma, beta, x1=None, film=None, act=0, mode=0, pad=0, dtype=_lib.K22_BF16):
    """x0 [B,C0,H,W] (+ x1 [B,C1,H,W]) float32 cuda -> (engine out NCHW float, torch reference NCHW float)."""
    T = tdt(dtype)
    B, C0, H, W_ = x0.shape
    C1 = 0 if x1 is None else x1.shape[1]
    C = C0 + C1
    a0 = x0.permute(0, 2, 3, 1).contiguous().to(T)
    a1 = None if x1 is None else x1.permute(0, 2, 3, 1).contiguous().to(T)
    Ho, Wo = (H // 2, W_ // 2) if mode == 1 else ((H * 2, W_ * 2) if mode == 2 else (H, W_))
    out = torch.full((B, Ho + 2 * pad, Wo + 2 * pad, C), float("nan"), dtype=T, device=x0.device)
    scratch = torch.empty(_lib.lib().k22_groupnorm_scratch_bytes(B, C), dtype=torch.uint8, device=x0.device)
    _lib.check(_lib.lib().k22_groupnorm(
        a0.data_ptr(), _lib.ptr(a1), C0, C1, B, H, W_, gamma.data_ptr(), beta.data_ptr(), _lib.ptr(film),
        0 if film is None else film.shape[1], 1e-5, act, mode, pad, scratch.data_ptr(), out.data_ptr(), dtype, stream()))
    xin = a0.float().permute(0, 3, 1, 2)
    if a1 is not None:
        xin = torch.cat([xin, a1.float().permute(0, 3, 1, 2)], 1)
    y = F.group_norm(xin, 32, gamma, beta, eps=1e-5)
    if film is not None:
        y = y * (1 + film[:, :C, None, None]) + film[:, C:2 * C, None, None]
    if act == 1:
        y = F.silu(y)
    if mode == 1:
        y = F.avg_pool2d(y, 2)
    elif mode == 2:
        y = F.interpolate(y, scale_factor=2, mode="nearest")
    if pad:
        y = F.pad(y, (1, 1, 1, 1))
    return out.float().permute(0, 3, 1, 2).contiguous(), y


def attention(qkv, ctxkv, B, H, T_, S, dtype=_lib.K22_BF16):
    """qkv [B*T,3C] columns [q|k|v] x [H][64]; ctxkv [B*S,2C] columns [k|v] (float32 cuda)."""
    T = tdt(dtype)
    C = H * 64
    q_ = qkv.to(T).contiguous()
    c_ = ctxkv.to(T).contiguous()
    Tkp = (S + T_ + 63) // 64 * 64
    kall = torch.full((B, H, Tkp, 64), float("nan"), dtype=T, device=qkv.device)
    vtall = torch.full((B, H, 64, Tkp), float("nan"), dtype=T, device=qkv.device)
    out = torch.empty(B * T_, C, dtype=T, device=qkv.device)
    _lib.check(_lib.lib().k22_attention(q_.data_ptr(), c_.data_ptr(), kall.data_ptr(), vtall.data_ptr(), out.data_ptr(),
                                        B, H, T_, S, dtype, stream()))
    qf = q_.float().view(B, T_, 3, H, 64)
    cf = c_.float().view(B, S, 2, H, 64)
    q = qf[:, :, 0].permute(0, 2, 1, 3)                                   # [B,H,T,64]
    k = torch.cat([cf[:, :, 0], qf[:, :, 1]], 1).permute(0, 2, 1, 3)      # [B,H,S+T,64]
    v = torch.cat([cf[:, :, 1], qf[:, :, 2]], 1).permute(0, 2, 1, 3)
    w = torch.softmax((q @ k.transpose(-1, -2)) * 0.125, dim=-1)
    ref = (w @ v).permute(0, 2, 1, 3).reshape(B * T_, C)
    return out.float(), ref


# ---- the shipped tile table, line by line (tests/test_tile_table_cpu.py, tests/test_tile_table_gpu.py) ------------------------------------
# A line of kandinsky-2_amd/tiles_gfx950.txt fixes kernel and tile of one launch_igemm problem (csrc/tuning.h).  What follows runs such a
# line through k22_igemm_cfg exactly as an engine would, restates the OPERATION (csrc/kernels.h, "Implicit GEMM") in plain torch float64 and
# compares element by element against a rounding-error bound that is not taken from any kernel:
#
#     |out - ref|  <=  L_act * c * (2^-24 + d_T) * S  +  u_out * |ref|  (+ e_act)
#
# ref   the float64 value of the operation on the operand values the kernel is promised to see (T-rounded; hi + lo of the x3 chunks;
#       for K22_F16X2 the activation at fp16 and everything else at full split);
# S     the same expression over absolute values (every |product|, |bias|, |residual| summed): the scale fp32 accumulation errors live on;
# c     IGEMM_C: what a PLAIN fp32 evaluation of the same product needs, times two - never taken from a kernel.  The yardstick is
#       max |fp32 - float64| / (2^-24 * S)  of torch's fp32 matmul and of a 16-wide sequential fp32 chain.  The rule: c = 4 while both
#       stay under 2, otherwise twice their maximum.  MEASURED:
#         CPU (tests/test_tile_table_cpu.py prints them), K = 128, 1152, 6912, 13824, 65536 outputs, bf16 / fp16 / fp32 operands:
#           16-wide chain <= 1.38 (K = 128; 0.74 at 1152, 0.61 at 13824); torch's matmul 0.2-0.6 at K >= 6912, <= 1.93 at 1152, and
#           2.6 (bf16) / 3.9 (fp16, fp32) at K = 128, where the host BLAS runs one chain of 128 roundings per output;
#         MI355X, torch's fp32 matmul over the 834 representative launches of the sweep: 3x3 convolutions (nine matmuls of Kc, summed)
#           <= 2.08; plain GEMMs up to 7.40 (fp32 qkv 32768 x 2304 x 768; 7.20 x3 qkv 512 x 2304 x 768, 7.08 x2 32768 x 768 x 768, 6.8
#           fp32 514 x 4992 x 1664, 4.56 bf16-rounded operands) - one long fp32 chain per output, the order the fp32 engine's own
#           v_mfma_f32_32x32x2_f32 kernels use: under c = 4 they sat at 1.0-1.86 of the bound (every 16-bit and split line under 1).
#       So c = 2 x 7.401 = 14.8.  The sweep asserts on every representative line that torch's matmul still passes the bound (ratio < c).
#       One number for every line, never tuned per line or from a kernel's output;
# d_T   what the arithmetic drops per product: 0 for bf16 / fp16 / fp32, 2^-22 for the split arithmetics (the lo.lo term);
# u_out one rounding of the stored type: 2^-8 bf16, 2^-11 fp16, 2^-24 fp32;
# L_act 1, or 1.13 with SiLU / GELU (their largest slope, which carries the accumulation error through the activation);
# e_act evaluation error of the activation itself: 4 x the largest error of torch's fp32 SiLU / GELU against float64 on the same
#       pre-activations.  MEASURED on the MI355X over the table's 29 GELU launches (prior / encoder MLPs; no shipped line has SiLU in its
#       epilogue): e_act = 1.79e-6 on every one (torch's fp32 GELU errs by 4.5e-7, half an fp32 ulp at |x| ~ 7); the fp32-output lines sit
#       at <= 0.16 of their bound with it, so the kernels' own GELU (common.h: gelu_f) needs no more than that.
# GroupNorm partial sums: sum within c * 2^-24 * sum|stored|, sum of squares within c * 2^-24 * sumsq, per image and channel, against the
# float64 sums of the values the launch itself stored.
import collections

IGEMM_C = 2 * 7.401
IGEMM_L_ACT = 1.13
U24 = 2.0 ** -24
X_DTYPES = (_lib.K22_F16X3, _lib.K22_F16X2)
DT_NAME = {_lib.K22_BF16: "bf16", _lib.K22_F32: "fp32", _lib.K22_F16: "fp16", _lib.K22_F16X3: "x3", _lib.K22_F16X2: "x2"}

TileLine = collections.namedtuple("TileLine", "dtype taps M N Kc K0 H W out_mode res_f32 act a_raw stats sk_total algo bm bn splitk stages")


def read_tile_table(path=None):
    """the lines of the table the package ships (or of `path`), in file order"""
    out = []
    with open(path or _lib.TILE_TABLE_PATH) as f:
        for ln in f:
            if ln.startswith("#") or not ln.strip():
                continue
            dt, taps, M, N, Kc, K0, H, W, om, ws, algo, bm, bn, sk, stg = (int(v) for v in ln.split()[:15])
            assert om < 512 and (om & 15) <= 3 and ws in (0, 1), ln
            out.append(TileLine(dt, taps, M, N, Kc, K0 % 100000, H, W, om & 15, (om >> 4) & 1, (om >> 5) & 7, (om >> 8) & 1, ws,
                                K0 // 100000, algo, bm, bn, sk, stg))
    return out


def tile_key(t):
    """what tuned_key makes of the problem, without the dtype"""
    return t[1:13] + (t.sk_total,)


def tile_class(t):
    """lines that exercise the same code: everything but the problem size"""
    return (t.dtype, t.taps, t.out_mode, t.res_f32, t.act, t.a_raw, t.stats, t.sk_total > 0, t.algo, t.bm, t.bn, t.splitk, t.stages)


def tile_id(t, dtype=None):
    dt = t.dtype if dtype is None else dtype
    kind = "conv" if t.taps == 9 else ("qkv" if t.out_mode == _lib.OUT_QKV else "gemm")
    s = f"{DT_NAME[dt]}-{kind}-{t.M}x{t.N}x{t.Kc}"
    if t.K0 != t.Kc:
        s += f"cat{t.K0}"
    if t.H:
        s += f"@{t.H}x{t.W}"
    flags = ("skip%d" % t.sk_total if t.sk_total else "") + ("-st" if t.stats else "") + ("-f32" if t.out_mode == 1 else "") + \
        ("-nchw" if t.out_mode == 2 else "") + ("-resf32" if t.res_f32 else "") + ("-act%d" % t.act if t.act else "") + ("-raw" if t.a_raw else "")
    if flags:
        s += "-" + flags.strip("-")
    s += f"-a{t.algo}-bm{t.bm}" + (f"x{t.bn}" if t.bn else "") + f"-sk{t.splitk}" + (f"-stg{t.stages}" if t.stages else "")
    return s


def tile_tiers(table):
    """(representatives, all remaining lines): of every tile_class the line with the largest M and the one with the smallest (ties: the
    smaller line tuple), in table order"""
    lo, hi = {}, {}
    for t in table:
        c = tile_class(t)
        if c not in lo or (t.M, t) < (lo[c].M, lo[c]):
            lo[c] = t
        if c not in hi or (-t.M, t) < (-hi[c].M, hi[c]):
            hi[c] = t
    reps = set(lo.values()) | set(hi.values())
    return [t for t in table if t in reps], [t for t in table if t not in reps]


ATT_S = 77   # context keys of the qkv lines (the key does not hold it; any value exercises the scatter behind them)


def skip_split(sk_total):
    """the key holds SK0 + SK1 only: two thirds | one third in units of 64 channels (1152 -> 768 | 384, as the up path's concat inputs)"""
    sk1 = sk_total // 64 // 3 * 64
    return sk_total - sk1, sk1


def tile_problem(t, dtype=None):
    """the K22IgemmProblem of a table line, run as `dtype` (default: its own)"""
    dt = t.dtype if dtype is None else dtype
    sk0, sk1 = skip_split(t.sk_total)
    T_ = t.H * t.W if t.out_mode == _lib.OUT_QKV else 0
    return _lib.K22IgemmProblem(
        dtype=dt, taps=t.taps, M=t.M, N=t.N, Kc=t.Kc, K0=t.K0, H=t.H, W=t.W, out_mode=t.out_mode, res_f32=t.res_f32, act=t.act,
        a_raw=t.a_raw, want_stats=t.stats, SK0=sk0, SK1=sk1, att_T=T_, att_S=ATT_S if T_ else 0, att_Tkp=(ATT_S + T_ + 63) // 64 * 64 if T_ else 0,
        ldo=0, ldr=0, has_frag=1 if t.algo == 20 else 0, algo=t.algo, bm=t.bm, bn=t.bn, splitk=t.splitk, stages=t.stages)


def tile_accepted(t, dtype=None):
    import ctypes as C
    pr = tile_problem(t, dtype)
    return _lib.lib().k22_igemm_cfg_accepted(C.byref(pr))


def storage_T(dtype):
    return torch.float32 if dtype in X_DTYPES else tdt(dtype)


def u_out(dtype, out_mode):
    if out_mode in (_lib.OUT_ROWMAJOR_F32, _lib.OUT_NCHW_F32) or dtype in X_DTYPES or dtype == _lib.K22_F32:
        return U24
    return 2.0 ** -8 if dtype == _lib.K22_BF16 else 2.0 ** -11


def d_T(dtype):
    return 2.0 ** -22 if dtype in X_DTYPES else 0.0


def igemm_inputs(t, device, seed=0):
    """seeded fp32 operands of a line: activations 0.3 + 1.7 randn (a non-zero mean shows a missed border, bias or tap), weights
    randn / sqrt(taps * Kc), bias and residual randn.  Layouts: a0 [B][H][W][K0] (taps 9; unpadded) or [M][K0]; a1 [M][Kc - K0];
    w [N][taps * Kc] (k = tap * Kc + c); residual [M][N]; s0 / s1 [M][SK0 / SK1]; ws [N][SK0 + SK1]."""
    g = torch.Generator(device=device).manual_seed(1000003 * seed + 17)

    def rn(*shape):
        return torch.randn(*shape, generator=g, device=device, dtype=torch.float32)

    sk0, sk1 = skip_split(t.sk_total)
    d = {}
    if t.taps == 9:
        d["a0"] = 0.3 + 1.7 * rn(t.M // (t.H * t.W), t.H, t.W, t.K0)
    else:
        d["a0"] = 0.3 + 1.7 * rn(t.M, t.K0)
    d["a1"] = 0.3 + 1.7 * rn(t.M, t.Kc - t.K0) if t.K0 < t.Kc else None
    d["w"] = rn(t.N, t.taps * t.Kc) * (t.taps * t.Kc) ** -0.5
    d["bias"] = rn(t.N)
    d["residual"] = None if t.out_mode == _lib.OUT_QKV else rn(t.M, t.N)
    d["s0"] = 0.3 + 1.7 * rn(t.M, sk0) if sk0 else None
    d["s1"] = 0.3 + 1.7 * rn(t.M, sk1) if sk1 else None
    d["ws"] = rn(t.N, sk0 + sk1) * (sk0 + sk1) ** -0.5 if sk0 else None
    d["bias2"] = rn(t.N) if sk0 else None
    return d


def x3_value(chunks):
    """x3 chunks -> hi + lo, float64 (the value three MFMAs see)"""
    h = chunks.contiguous().view(torch.float16).double()
    g = h.view(*chunks.shape[:-1], chunks.shape[-1] // 8, 2, 8)
    return (g[..., 0, :] + g[..., 1, :]).reshape(chunks.shape)


def igemm_seen(t, dtype, inp):
    """float64 operand values the arithmetic `dtype` is promised to see, same keys and layouts as igemm_inputs.  bias (fp32) is exact;
    the residual is T (fp32 when res_f32 or for the split arithmetics)."""
    from kandinsky2_amd.pack import to_x3
    if dtype in X_DTYPES:
        full = lambda x: None if x is None else x3_value(to_x3(x, 1.0))
        act = (lambda x: None if x is None else x.to(torch.float16).double()) if dtype == _lib.K22_F16X2 else full
        s = {"a0": act(inp["a0"]), "a1": act(inp["a1"]), "w": x3_value(to_x3(inp["w"])) / 256.0, "s0": full(inp["s0"]), "s1": full(inp["s1"]),
             "ws": None if inp["ws"] is None else x3_value(to_x3(inp["ws"])) / 256.0}
        rT = torch.float32
    else:
        T = tdt(dtype)
        r = lambda x: None if x is None else x.to(T).double()
        s = {k: r(inp[k]) for k in ("a0", "a1", "w", "s0", "s1", "ws")}
        rT = torch.float32 if t.res_f32 else T
    for k in ("bias", "bias2"):
        s[k] = None if inp[k] is None else inp[k].double()
    s["residual"] = None if inp["residual"] is None else inp["residual"].to(rT).double()
    return s


def act64(x, act):
    if act == _lib.ACT_SILU:
        return x * torch.sigmoid(x)
    if act == _lib.ACT_GELU:
        return 0.5 * x * (1.0 + torch.erf(x * 2.0 ** -0.5))
    return x


def igemm_pre64(t, s):
    """(pre, S): the float64 pre-activation [M][N] of the operation over the seen operands, and the same expression over absolute values.
    Written from the definition: nine tap-shifted matmuls over the zero-bordered NHWC input (one for taps = 1), virtual concat K0 | K1,
    bias, residual, fused 1x1 skip with its bias."""
    def both(fn):
        return fn(lambda x: x), fn(torch.abs)

    def main(f):
        w = f(s["w"])
        if t.taps == 9:
            B = t.M // (t.H * t.W)
            xp = F.pad(f(s["a0"]), (0, 0, 1, 1, 1, 1))                     # [B][H+2][W+2][Kc], zero border
            acc = None
            for tap in range(9):
                ky, kx = divmod(tap, 3)
                part = xp[:, ky:ky + t.H, kx:kx + t.W, :].reshape(t.M, t.Kc) @ w[:, tap * t.Kc:(tap + 1) * t.Kc].T
                acc = part if acc is None else acc + part
        else:
            acc = f(s["a0"]) @ w[:, :t.K0].T
            if t.K0 < t.Kc:
                acc = acc + f(s["a1"]) @ w[:, t.K0:].T
        if s["bias"] is not None:
            acc = acc + f(s["bias"])
        if s["residual"] is not None:
            acc = acc + f(s["residual"])
        if s["s0"] is not None:
            sk0 = s["s0"].shape[1]
            acc = acc + f(s["s0"]) @ f(s["ws"])[:, :sk0].T
            if s["s1"] is not None:
                acc = acc + f(s["s1"]) @ f(s["ws"])[:, sk0:].T
            if s["bias2"] is not None:
                acc = acc + f(s["bias2"])
        return acc
    return both(main)


def igemm_layout(t, v, fill=float("nan")):
    """[M][N] values -> dict of tensors in the layout of the line's out mode (positions the launch does not own hold `fill`)"""
    if t.out_mode in (_lib.OUT_ROWMAJOR, _lib.OUT_ROWMAJOR_F32):
        return {"out": v}
    if t.out_mode == _lib.OUT_NCHW_F32:
        B = t.M // (t.H * t.W)
        return {"out": v.view(B, t.H, t.W, t.N).permute(0, 3, 1, 2).contiguous()}
    C_, T_ = t.N // 3, t.H * t.W
    B, heads, Tkp = t.M // T_, C_ // 64, (ATT_S + T_ + 63) // 64 * 64
    q5 = v.view(B, T_, 3, heads, 64)
    kall = torch.full((B, heads, Tkp, 64), fill, dtype=v.dtype, device=v.device)
    vtall = torch.full((B, heads, 64, Tkp), fill, dtype=v.dtype, device=v.device)
    kall[:, :, ATT_S:ATT_S + T_] = q5[:, :, 1].permute(0, 2, 1, 3)
    vtall[:, :, :, ATT_S:ATT_S + T_] = q5[:, :, 2].permute(0, 2, 3, 1)
    return {"out": v[:, :C_].contiguous(), "kall": kall, "vtall": vtall}


def act_eval_term(pre, act):
    """e_act: 4 x the largest error of torch's fp32 activation against float64 on the same (fp32) pre-activations"""
    if act == _lib.ACT_NONE:
        return 0.0
    x32 = pre.float()
    y32 = F.silu(x32) if act == _lib.ACT_SILU else F.gelu(x32)
    return 4.0 * (y32.double() - act64(x32.double(), act)).abs().max().item()


def igemm_ref(t, dtype, inp, c=IGEMM_C, info=None):
    """-> (ref, bound): dicts of float64 tensors in the out mode's layout.  ref is NaN, bound 0 where the launch owns nothing.
    info (optional dict) receives e_act, the activation's evaluation term."""
    s = igemm_seen(t, dtype, inp)
    pre, S = igemm_pre64(t, s)
    ref = act64(pre, t.act)
    L = IGEMM_L_ACT if t.act else 1.0
    e_act = act_eval_term(pre, t.act)
    if info is not None:
        info["e_act"] = e_act
    bound = L * c * (U24 + d_T(dtype)) * S + u_out(dtype, t.out_mode) * ref.abs() + e_act
    return igemm_layout(t, ref), igemm_layout(t, bound, fill=0.0)


def igemm_violations(out, ref, bound):
    """per-element check of one output tensor: (number of elements outside their bound or NaN where a value is owed or not NaN where the
    launch owns nothing, largest |out - ref| / bound)"""
    o = out.double()
    owned = ~torch.isnan(ref)
    err = (o - torch.where(owned, ref, torch.zeros_like(ref))).abs()
    bad_owned = owned & ~(err <= bound)                                    # NaN in `out` compares false: counted
    bad_free = ~owned & ~torch.isnan(o)
    ratio = torch.where(owned & torch.isfinite(err), err / bound.clamp_min(1e-300), torch.zeros_like(err)).max().item() if owned.any() else 0.0
    return int(bad_owned.sum().item() + bad_free.sum().item()), ratio


def stats_violations(stats_rows, stored, t, rows_per_image, c=IGEMM_C):
    """stats_rows [cap][N][2] fp32 as the launch left it (NaN pre-filled), stored: the [M][N] values the launch stored (any float type).
    -> number of (image, channel, which) entries outside  c * 2^-24 * (sum|stored|, sumsq)  plus rows beyond B * rows_per_image that
    are no longer NaN."""
    B = t.M // (t.H * t.W)
    used = stats_rows[: B * rows_per_image].double().view(B, rows_per_image, t.N, 2).sum(1)
    v = stored.double().view(B, t.H * t.W, t.N)
    sq = (v * v).sum(1)
    bad = ~((used[..., 0] - v.sum(1)).abs() <= c * U24 * v.abs().sum(1))
    bad2 = ~((used[..., 1] - sq).abs() <= c * U24 * sq)
    free = ~torch.isnan(stats_rows[B * rows_per_image:])
    return int(bad.sum().item() + bad2.sum().item() + free.sum().item())


def plain_fp32_ratio(t, dtype, inp, chain16=False):
    """the yardstick behind IGEMM_C: the largest |plain fp32 evaluation - float64| / (2^-24 * S) of the line's pre-activation, operands as
    the arithmetic sees them (rounded to fp32 where they carry more).  Plain = torch's fp32 matmul, or (chain16) sixteen interleaved
    sequential fp32 chains per output, k = j, j + 16, ... - the order of a 16-deep MFMA."""
    s = igemm_seen(t, dtype, inp)
    pre, S = igemm_pre64(t, s)
    s32 = {k: (None if v is None else v.float()) for k, v in s.items()}
    if chain16:
        assert t.taps == 1 and t.K0 == t.Kc and s["s0"] is None
        a, w = s32["a0"], s32["w"]
        acc = torch.zeros(t.M, t.N, 16, dtype=torch.float32, device=a.device)
        for k0 in range(0, t.Kc, 16):
            acc = acc + a[:, None, k0:k0 + 16] * w[None, :, k0:k0 + 16]
        p32 = acc.sum(-1) + s32["bias"] + s32["residual"]
    else:
        p32 = igemm_pre64(t, s32)[0]
    return ((p32.double() - pre).abs() / (U24 * S)).max().item()


def run_tile_line(t, dtype, inp):
    """one k22_igemm_cfg launch of the line as `dtype` on inp's device: operands in the formats the engine of that arithmetic holds,
    outputs / stats / K_all / V^T_all pre-filled with NaN.  -> (dict of output tensors in the out mode's layout, stats rows or None,
    rows per image)."""
    import ctypes as C
    from kandinsky2_amd.pack import to_x3
    dev = inp["a0"].device
    split = dtype in X_DTYPES
    T = storage_T(dtype)
    pr = tile_problem(t, dtype)
    keep = []

    def act_operand(x, padded=False):
        if x is None:
            return None
        if padded:
            x = F.pad(x, (0, 0, 1, 1, 1, 1))
        x = x.contiguous()
        x = (x if t.a_raw else to_x3(x, 1.0)) if split else x.to(T)
        keep.append(x)
        return x

    def weight(w):
        w = pad_rows(w)
        w = to_x3(w) if split else w.to(T).contiguous()
        keep.append(w)
        return w

    a0 = act_operand(inp["a0"], padded=t.taps == 9)
    a1 = act_operand(inp["a1"])
    wp = weight(inp["w"])
    res = inp["residual"]
    if res is not None:
        res = res.to(torch.float32 if (split or t.res_f32) else T).contiguous()
    s0 = s1 = ws = None
    if inp["s0"] is not None:
        s0 = inp["s0"].contiguous() if split else inp["s0"].to(T).contiguous()
        s1 = None if inp["s1"] is None else (inp["s1"].contiguous() if split else inp["s1"].to(T).contiguous())
        ws = weight(inp["ws"])
    oT = torch.float32 if t.out_mode in (_lib.OUT_ROWMAJOR_F32, _lib.OUT_NCHW_F32) else T
    nan = float("nan")
    outs = {k: torch.full(v.shape, nan, dtype=oT, device=dev) for k, v in igemm_layout(t, torch.zeros(t.M, t.N, device=dev)).items()}
    # (the all-zero configuration is the fixed choice: the library reports the split factor that launch resolves to)
    splitk = t.splitk if any(cfg_of(t)) else igemm_candidates(t, dtype)[2][3]
    partial = torch.empty(max(1, splitk) * t.M * t.N + 64, dtype=torch.float32, device=dev)
    wfrag = wsfrag = None
    if t.algo == 20:
        L = _lib.lib()
        wfrag = torch.empty(L.k22_stream_frag_bytes(wp.shape[0], t.taps, t.Kc, dtype), dtype=torch.uint8, device=dev)
        _lib.check(L.k22_stream_repack(wp.data_ptr(), wfrag.data_ptr(), wp.shape[0], t.taps, t.Kc, dtype, stream()))
        if ws is not None:
            wsfrag = torch.empty(L.k22_stream_frag_bytes(wp.shape[0], 1, t.sk_total, dtype), dtype=torch.uint8, device=dev)
            _lib.check(L.k22_stream_repack(ws.data_ptr(), wsfrag.data_ptr(), wp.shape[0], 1, t.sk_total, dtype, stream()))
    sbuf, cap = None, 0
    if t.stats:
        B = t.M // (t.H * t.W)
        cap = B * max(t.H * t.W // 16, (t.H * (t.W + 2) + 127) // 128) + 3
        sbuf = torch.full((cap, t.N, 2), nan, dtype=torch.float32, device=dev)
    ops = _lib.K22IgemmOperands(
        A0=a0.data_ptr(), A1=_lib.ptr(a1), Wp=wp.data_ptr(), bias=inp["bias"].data_ptr(), residual=_lib.ptr(res), out=outs["out"].data_ptr(),
        partial=partial.data_ptr(), S0=_lib.ptr(s0), S1=_lib.ptr(s1), Ws=_lib.ptr(ws), bias2=_lib.ptr(inp["bias2"]),
        kall=_lib.ptr(outs.get("kall")), vtall=_lib.ptr(outs.get("vtall")), Wfrag=_lib.ptr(wfrag), Wsfrag=_lib.ptr(wsfrag),
        stats=_lib.ptr(sbuf), stats_capacity_rows=cap)
    rpi = C.c_int(0)
    _lib.check(_lib.lib().k22_igemm_cfg(C.byref(pr), C.byref(ops), C.byref(rpi), stream()))
    torch.cuda.synchronize()
    return outs, sbuf, rpi.value


# ---- off-table problems: what the tuner may pick where the shipped table has no line (tests/test_igemm_candidates_*.py) ------------------------
# The table holds the C1-C5 shapes only; any other batch or image size is timed on the device over tuned_make_candidates' list (or, with
# K22_AUTOTUNE=0 and for every M < 64, runs tuned_default_cfg's fixed choice).  OFFTABLE lists the smallest problems at which each edge of
# those kernels' index arithmetic exists, as TileLines whose configuration fields are zero (= the fixed choice): igemm_candidates reads the
# build's own candidate list for one, and t._replace(algo=..., ...) runs a candidate through run_tile_line like any table line.  The dtype
# field is a placeholder: every problem runs in every arithmetic that accepts it (offtable_accepts).

def _ot_conv(B, H, W, Cin, Cout, stats=0, sk=0, out_mode=0):
    return TileLine(0, 9, B * H * W, Cout, Cin, Cin, H, W, out_mode, 0, 0, 0, stats, sk, 0, 0, 0, 0, 0)


def _ot_gemm(M, N, Kc, K0=None, H=0, W=0, out_mode=0, res_f32=0, act=0, a_raw=0, stats=0):
    return TileLine(0, 1, M, N, Kc, Kc if K0 is None else K0, H, W, out_mode, res_f32, act, a_raw, stats, 0, 0, 0, 0, 0, 0)


OFFTABLE = {
    # 3x3 convolutions  B, H, W, Cin -> Cout (the residual is always there: igemm_inputs)
    "conv-3x5x5-128-128": _ot_conv(3, 5, 5, 128, 128),                    # image smaller than one tile, odd sizes, odd batch
    "conv-1x5x5-128-128": _ot_conv(1, 5, 5, 128, 128),                    # M = 25 < 64: the fixed choice only (the tuner skips it)
    "conv-3x5x7-128-256-st": _ot_conv(3, 5, 7, 128, 256, stats=1),        # prime H: stream bands of 1 or H rows; partial-sum rows of ragged tiles
    # (35 rows per image admit no row-tiled finish, so with the sums owed the build lists no streaming candidate: the same shape without them)
    "conv-3x5x7-128-256": _ot_conv(3, 5, 7, 128, 256),
    "conv-2x10x10-192-192": _ot_conv(2, 10, 10, 192, 192),               # lowest level of a 640-px image; 1.5 halo n-tiles; 3 / 6 k-steps: uneven splits
    "conv-2x10x10-192-192-st": _ot_conv(2, 10, 10, 192, 192, stats=1),
    "conv-1x20x20-128-136": _ot_conv(1, 20, 20, 128, 136),                # N % 8 == 0, N % 64 != 0: Npad 192
    "conv-2x9x13-64-128": _ot_conv(2, 9, 13, 64, 128),                    # 16-bit types: one k-step per tap, ring deeper than the loop
    "conv-2x9x13-32-128": _ot_conv(2, 9, 13, 32, 128),                    # the same for the 32-wide-BK arithmetics
    "conv-1x40x40-128-128-st": _ot_conv(1, 40, 40, 128, 128, stats=1),    # next 640-px level, tiles ending mid-row
    "conv-2x1x37-64-128": _ot_conv(2, 1, 37, 64, 128),                    # H = 1: top and bottom border in one row
    "conv-2x37x1-64-128": _ot_conv(2, 37, 1, 64, 128),                    # W = 1: every position touches the border, W + 2 = 3
    "conv-1x2x160-64-128": _ot_conv(1, 2, 160, 64, 128),                  # W + 2 > 128: a tile shorter than a row; bm 128 at ring depth 2
    "conv-1x2x130-64-128": _ot_conv(1, 2, 130, 64, 128),                  # bm 128 at ring depth 3 (126 <= W <= 157)
    "conv-1x1x230-64-128": _ot_conv(1, 1, 230, 64, 128),                  # halo3 alone takes W > 189: its ring at depth 3 (bm 128) and 2 (bm 256)
    "conv-1x1x300-64-128": _ot_conv(1, 1, 300, 64, 128),                  # halo3 bm 128 at ring depth 2, its widest frame (W <= 317)
    "conv-1x3x100-64-128": _ot_conv(1, 3, 100, 64, 128),                  # bm 256 at ring depth 2
    "conv-1x3x64-64-128": _ot_conv(1, 3, 64, 64, 128),                    # bm 256 at ring depth 3, bm 128 at depth 4
    "conv-2x10x10-128-128-skip64": _ot_conv(2, 10, 10, 128, 128, sk=64),  # skip narrower than an n-tile
    "conv-2x10x10-128-128-skip192": _ot_conv(2, 10, 10, 128, 128, sk=192),   # skip_split: 128 | 64, concat skip source
    "conv-2x10x10-128-8-nchw": _ot_conv(2, 10, 10, 128, 8, out_mode=_lib.OUT_NCHW_F32),   # head conv: generic kernel only
    # GEMMs
    "gemm-300x192x192-st": _ot_gemm(300, 192, 192, H=10, W=10, stats=1),  # 100 rows per image under a 128 / 256-row tile
    "gemm-333x200x576": _ot_gemm(333, 200, 576),                          # ragged M, Npad 256, nine k-steps
    "gemm-65x128x64": _ot_gemm(65, 128, 64),                              # second m-tile holds one row; one k-step
    "gemm-200x128x96-raw": _ot_gemm(200, 128, 96, a_raw=1),               # split types only: three 32-wide steps
    "gemm-150x256x320cat128-f32": _ot_gemm(150, 256, 320, K0=128, out_mode=_lib.OUT_ROWMAJOR_F32),   # virtual concat
    "gemm-162x256x256-gelu-resf32": _ot_gemm(162, 256, 256, res_f32=1, act=_lib.ACT_GELU),            # prior-like
    "qkv-2x10x10-128-h2": _ot_gemm(200, 384, 128, H=10, W=10, out_mode=_lib.OUT_QKV),     # Tkp 192: keys scattered behind S = 77 into padded K_all / V^T_all
    "qkv-2x10x10-128-h6": _ot_gemm(200, 1152, 128, H=10, W=10, out_mode=_lib.OUT_QKV),
    "gemm-2x1536x384": _ot_gemm(2, 1536, 384),                            # M < 64: the fixed choice only
}
ALL_DTYPES = (_lib.K22_BF16, _lib.K22_F16, _lib.K22_F32, _lib.K22_F16X3, _lib.K22_F16X2)
CFG_FIELDS = ("algo", "bm", "bn", "splitk", "stages")


def offtable_accepts(t, dtype):
    """does the arithmetic take the problem at all: K per tap, both concat halves and the skip widths in whole k-steps (64 elements for the
    16-bit types, 32 for fp32 and the split ones); raw fp32 activation rows are an option of the split arithmetics only"""
    bk = 64 if dtype in (_lib.K22_BF16, _lib.K22_F16) else 32
    sk0, sk1 = skip_split(t.sk_total)
    return not (t.Kc % bk or t.K0 % bk or sk0 % bk or sk1 % bk) and (not t.a_raw or dtype in X_DTYPES)


def offtable_cases():
    """[(id, TileLine, dtype)] of every (problem, arithmetic) pair that is run"""
    return [(f"{name}-{DT_NAME[dt]}", t, dt) for name, t in OFFTABLE.items() for dt in ALL_DTYPES if offtable_accepts(t, dt)]


def cfg_of(t):
    return tuple(getattr(t, f) for f in CFG_FIELDS)


def igemm_candidates(t, dtype, has_frag=0):
    """the build's own list for the problem (k22_igemm_candidates: tuned_make_candidates over the engines' descriptor; no device needed)
    -> (candidates, resolved, fixed): lists of (algo, bm, bn, splitk, stages) as generated / as igemm_resolve makes them (stages = the ring
    depth instantiated), and the resolved launch of the all-zero configuration, tuned_default_cfg's choice"""
    import ctypes as C
    pr = tile_problem(t._replace(algo=0, bm=0, bn=0, splitk=0, stages=0), dtype)
    pr.has_frag = has_frag
    cap = 512
    out, res, fixed = (_lib.K22IgemmCfg * cap)(), (_lib.K22IgemmCfg * cap)(), _lib.K22IgemmCfg()
    n = _lib.lib().k22_igemm_candidates(C.byref(pr), out, cap, res, C.byref(fixed))
    if n < 0:
        _lib.check(n)
    assert n <= cap
    tup = lambda c: tuple(getattr(c, f) for f in CFG_FIELDS)
    return [tup(out[i]) for i in range(n)], [tup(res[i]) for i in range(n)], tup(fixed)


# ---- engine-level evidence: the tuning report of an engine, the tile table as text (tests/test_engine_switches_gpu.py) ------------------
ReportLine = collections.namedtuple("ReportLine", "taps M N K H W stats algo bm bn splitk stages count")


def report_lines(report):
    """the lines of tuning_report_text (csrc/tuning.h) without their time column: the problem, the configuration that runs it (algo by
    igemm_algo_name) and how many ops of the plan share the line"""
    out = []
    for ln in report.splitlines()[1:]:
        if not ln.strip():
            continue
        prob, cfg, tail = (part.split() for part in ln.split("|"))
        assert len(prob) == 7 and len(cfg) == 5 and len(tail) == 2 and tail[1].startswith("x"), ln
        out.append(ReportLine(*(int(v) for v in prob), cfg[0], *(int(v) for v in cfg[1:]), int(tail[1][1:])))
    return out


def report_problems(report, taps):
    """{(M, N, K, H, W)} of the report's lines with that many taps"""
    return {(r.M, r.N, r.K, r.H, r.W) for r in report_lines(report) if r.taps == taps}


def tile_table_text_lines(path):
    """the data lines of a tile-table file as text, in the order read_tile_table returns them"""
    with open(path) as f:
        return [ln for ln in f if not ln.startswith("#") and ln.strip()]


def tile_table_text_with_cfg(text_line, cfg):
    """the table line with its configuration columns (algo bm bn splitk stages) replaced, key and time kept"""
    cols = text_line.split()
    assert len(cols) == 16 and len(cfg) == 5, text_line
    return " ".join(cols[:10] + [str(int(v)) for v in cfg] + cols[15:]) + "\n"


def host_refusal(err):
    """is the RuntimeError of _lib.check a refusal on the host (K22_EINVAL / K22_ENOMEM: nothing was launched)?  Anything else - a failed
    launch, a device fault - must end the session (tests/test_igemm_candidates_gpu.py)"""
    return str(err).startswith(("k22 error -1:", "k22 error -3:"))
