"""Float64 parity, kernel by kernel, of the skinny-M family the 16-bit prior runs through - skinny_kernel, finish_ln_kernel,
afrag_pack_kernel (csrc/skinny.hip) and small_attention_kernel (csrc/attention.hip) - through the C entry points of include/k22.h.
Restatements, inputs, bounds, mutants and the measured yardsticks: tests/skinny_ref.py (CPU part: tests/test_skinny_parity_cpu.py).

Every buffer a launch writes is pre-filled with NaN (0xA5 bytes where bit patterns are compared) and carries guard elements on both sides:
every owned element is checked against its own bound, every other one must still hold the fill.  A-fragment INPUTS of every GEMM and chain
case carry NaN in their padding rows.  The shapes are the smallest that can go wrong; the workload's own sizes stay in test_skinny_gpu.py.
The last test prints the largest |error| / bound per kernel next to torch's own fp32 evaluation on the same bound."""
import os
import time

import pytest
import torch

import skinny_ref as sr
from kandinsky2_amd import _lib

ar, atr, hp = sr.ar, sr.atr, sr.hp
pytestmark = pytest.mark.gpu
DTYPES = sr.DTYPES
DT_IDS = [sr.DT_NAME[d] for d in DTYPES]
DEV = "cuda"
GUARD = 256
_EINVAL = -1         # include/k22.h: K22_EINVAL
STATS = {}           # (kernel, dtype name) -> [largest kernel ratio, largest torch-fp32 ratio, largest yardstick]
T0 = time.time()
needs_default_cfg = pytest.mark.skipif("K22_SKINNY_CFG" in os.environ, reason="K22_SKINNY_CFG overrides the default tile these cases are about")


def L():
    return _lib.lib()


def sync():
    torch.cuda.synchronize()


def guarded(n, T, fill=ar.NAN):
    """(whole buffer, its n owned elements) with GUARD fill elements on both sides"""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=T, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def note(kernel, dtype, ratio, torch_ratio=0.0, yard=0.0):
    s = STATS.setdefault((kernel, sr.DT_NAME[dtype]), [0.0, 0.0, 0.0])
    s[0], s[1], s[2] = max(s[0], ratio), max(s[1], torch_ratio), max(s[2], yard)


def stored(x, dtype):
    return x.to(hp.tdt(dtype)).double()


def bounded(buf, exp, bound):
    """violations / largest ratio of a guarded buffer against the flat expectation (NaN: the fill must still be there)"""
    return ar.violations(buf, ar.with_guard(exp, GUARD), ar.with_guard(bound, GUARD, 0.0))


def repack_w(wT, dtype):
    out = torch.empty_like(wT)
    _lib.check(L().k22_stream_repack(wT.data_ptr(), out.data_ptr(), wT.shape[0], 1, wT.shape[1], dtype, hp.stream()))
    return out


# ---- layouts (E) --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_afrag_pack_exact(dtype):
    T = hp.tdt(dtype)
    for (M, K, lda) in ((1, 64, 64), (33, 128, 136), (81, 192, 192)):
        a = torch.full((M, lda), ar.NAN, dtype=T, device=DEV)
        a[:, :K] = ar.rn(ar.gen(M + K), M, K).to(DEV).to(T)
        buf, out = guarded(sr.afrag_elems(M, K), torch.int16, fill=-23131)              # 0xA5A5
        assert L().k22_afrag_pack(a.data_ptr(), lda, out.data_ptr(), M, K, dtype, hp.stream()) == 0, L().k22_last_error()
        sync()
        exp = ar.with_guard(sr.afrag_expected(a[:, :K].contiguous().view(torch.int16), fill=-23131), GUARD, -23131)
        assert torch.equal(buf, exp), (M, K, lda)                                       # padding rows and guards keep the fill


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_stream_repack_taps1_is_wfrag_index(dtype):
    for (Npad, K) in ((64, 128), (128, 64)):
        w = torch.arange(Npad * K, dtype=torch.int32).remainder(65521).to(torch.int16).reshape(Npad, K).to(DEV)
        buf, out = guarded(Npad * K, torch.int16, fill=-23131)
        assert L().k22_stream_repack(w.data_ptr(), out.data_ptr(), Npad, 1, K, dtype, hp.stream()) == 0, L().k22_last_error()
        sync()
        exp = torch.empty(Npad * K, dtype=torch.int16, device=DEV)
        exp[sr.wfrag_index(Npad, K, DEV).reshape(-1)] = w.reshape(-1)
        assert torch.equal(buf, ar.with_guard(exp, GUARD, -23131)), (Npad, K)


# ---- skinny GEMM (M) ----------------------------------------------------------------------------------------------------------------------
def launch_gemm(c, af, wf, bias, dtype, Npad=None, tile=None):
    """one k22_skinny_gemm launch into a NaN-filled guarded buffer -> (rc, buffer)"""
    T = hp.tdt(dtype)
    mt, nb = tile or (c.mt, c.nb)
    ldo = c.N + c.slack
    if c.epi == sr.EPI_PARTIAL:
        buf, out = guarded(c.splitk * c.M * c.N, torch.float32)
        args = (None, None, out.data_ptr())
    else:
        buf, out = guarded(c.M * ldo if c.epi == sr.EPI_ROWMAJOR else sr.afrag_elems(c.M, c.N), T)
        args = (_lib.ptr(bias), out.data_ptr(), None)
    rc = L().k22_skinny_gemm(af.data_ptr(), wf.data_ptr(), args[0], args[1], args[2], c.M, c.N, Npad or wf.shape[0], c.K, c.splitk, c.epi, c.act,
                             ldo, mt, nb, dtype, hp.stream())
    sync()
    return rc, buf


def check_gemm(c, s, buf, dtype, kernel="skinny"):
    """buf against the float64 restatement over the seen operands s (device) -> largest |error| / bound"""
    r = sr.gemm_ref(s, c)
    bound = sr.gemm_bound(r, c, dtype)
    if c.epi == sr.EPI_PARTIAL:
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), sr.gemm_id(c)
        parts = buf[GUARD:-GUARD].view(c.splitk, c.M, c.N)
        assert bool(torch.isfinite(parts).all()), sr.gemm_id(c)
        for z, (c0, c1) in enumerate(sr.chunk_ranges(c.K, c.splitk)):
            if c0 >= c1:
                assert bool((parts[z] == 0).all()), (sr.gemm_id(c), z)
        nbad, ratio = ar.violations(parts.double().sum(0), r["pre"], bound)
    else:
        nbad, ratio = bounded(buf, sr.gemm_layout(r["ref"], c), sr.gemm_layout(bound, c, 0.0))
    print(f"{kernel} {sr.gemm_id(c)} {sr.DT_NAME[dtype]}: |out - ref| / bound = {ratio:.3f}")
    assert nbad == 0, (sr.gemm_id(c), sr.DT_NAME[dtype], nbad, ratio)
    return ratio, r, bound


def gemm_case(c, dtype):
    T = hp.tdt(dtype)
    for fam in sr.GEMM_FAMILIES:
        d = ar.to_dev(sr.gemm_inputs(c, fam), DEV)
        af = sr.afrag_expected(d["a"].to(T))                                            # padding rows: NaN
        wf = repack_w(hp.pad_rows(d["w"].to(T), 128 if c.nb == 4 else 64), dtype)
        assert wf.shape[0] == sr.npad(c)
        rc, buf = launch_gemm(c, af, wf, d["bias"], dtype)
        assert rc == 0, L().k22_last_error()
        ratio, r, bound = check_gemm(c, sr.gemm_seen(d, dtype), buf, dtype)
        # torch's own fp32 evaluation on the same operands: the yardstick under c, and its reading on the same bound
        t = sr.gemm_ref(sr.gemm_seen(d, dtype, f64=False), c)
        yard = ar.plain_ratio(t["pre"], r["pre"], r["S"])
        assert yard < sr.GEMM_C, (sr.gemm_id(c), fam, yard)
        if c.epi == sr.EPI_PARTIAL:
            tr = ar.violations(t["parts"].double().sum(0), r["pre"], bound)[1]
        else:
            tr = ar.violations(stored(t["ref"], dtype), r["ref"], bound)[1]
        note(f"skinny epilogue {c.epi}", dtype, ratio, tr, yard)
        note(f"yardstick {fam}", dtype, 0.0, 0.0, yard)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("c", [c for c in sr.GEMM_CASES if c.mt], ids=sr.gemm_id)
def test_skinny_gemm(c, dtype):
    gemm_case(c, dtype)


@needs_default_cfg
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("c", [c for c in sr.GEMM_CASES if not c.mt], ids=sr.gemm_id)
def test_skinny_gemm_default_tile(c, dtype):
    gemm_case(c, dtype)


# ---- finish_ln ----------------------------------------------------------------------------------------------------------------------------
FILL32 = -1515870811     # 0xA5A5A5A5


def launch_finish_ln(c, d, x_rows, dtype, N=None, splitk=None, beta=True):
    """x_rows [M][N] fp32 (device) placed in a 0xA5-filled [M][ldx] buffer with guards -> (rc, x buffer as int32, y buffer or None)"""
    T = hp.tdt(dtype)
    ldx = c.N + c.slack
    xbuf, xv = guarded(c.M * ldx, torch.int32, fill=FILL32)
    xv.view(torch.float32).view(c.M, ldx)[:, :c.N] = x_rows
    ybuf, yv = guarded(sr.afrag_elems(c.M, c.N), T) if c.ln else (None, None)
    rc = L().k22_finish_ln(_lib.ptr(d["partial"]), c.splitk if splitk is None else splitk, _lib.ptr(d["bias"]), xv.data_ptr(), ldx,
                           _lib.ptr(d["g"]) if c.ln else None, _lib.ptr(d["b"]) if c.ln and beta else None, None if yv is None else yv.data_ptr(),
                           c.M, c.N if N is None else N, sr.FLN_EPS, dtype, hp.stream())
    sync()
    return rc, xbuf, ybuf


def x_expected(c, xu):
    """the int32 image of the x buffer after the launch: the chain's bits in the owned columns, the fill in the slack and the guards"""
    exp = torch.full((c.M, c.N + c.slack), FILL32, dtype=torch.int32, device=DEV)
    exp[:, :c.N] = xu.to(DEV).view(torch.int32)
    return ar.with_guard(exp, GUARD, FILL32)


def check_ln(c, xu_dev, g, b, ybuf, dtype, kernel):
    ref, S = sr.fln_ln_ref(xu_dev.double(), g.double(), b.double())
    bound = sr.fln_bound(ref, S, dtype)
    nbad, ratio = bounded(ybuf, sr.afrag_expected(ref), sr.afrag_expected(bound, 0.0))
    t = torch.nn.functional.layer_norm(xu_dev, (xu_dev.shape[1],), g, b, sr.FLN_EPS)
    yard = ar.plain_ratio(t, ref, S)
    assert yard < sr.LN_C, (kernel, yard)
    note(kernel, dtype, ratio, ar.violations(stored(t, dtype), ref, bound)[1], yard)
    return nbad, ratio


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_finish_ln(dtype):
    for c in sr.FLN_CASES:
        cpu = sr.fln_inputs(c)
        xu = sr.x_chain32(cpu)                                                          # fp32 on the CPU, in the kernel's order
        d = ar.to_dev(cpu, DEV)
        rc, xbuf, ybuf = launch_finish_ln(c, d, d["x"], dtype)
        assert rc == 0, L().k22_last_error()
        assert torch.equal(xbuf, x_expected(c, xu)), sr.fln_id(c)                       # E: bit for bit, slack columns untouched
        if c.ln:
            nbad, ratio = check_ln(c, xu.to(DEV), d["g"], d["b"], ybuf, dtype, "finish_ln LayerNorm")
            print(f"finish_ln {sr.fln_id(c)} {sr.DT_NAME[dtype]}: |y - ref| / bound = {ratio:.3f}")
            assert nbad == 0, (sr.fln_id(c), nbad, ratio)


# ---- small_attention ------------------------------------------------------------------------------------------------------------------------
def launch_attention(c, d, dtype, T_=None, nsplit=None, dt_arg=None):
    """d on the device -> (rc, NaN-filled guarded output buffer)"""
    T = hp.tdt(dtype)
    M, C = c.B * c.T, c.H * atr.HD
    qkv = None if c.nsplit else d["qkv"].reshape(M, 3 * C).to(T).contiguous()
    buf, out = guarded(sr.afrag_elems(M, C) if c.frag else M * C, T)
    rc = L().k22_small_attention(_lib.ptr(qkv), _lib.ptr(d["part"]), c.nsplit if nsplit is None else nsplit, _lib.ptr(d["bias"]), out.data_ptr(), c.frag,
                                 c.B, c.H, c.T if T_ is None else T_, c.causal, _lib.ptr(d["key_valid"]), c.kv_n, dtype if dt_arg is None else dt_arg, hp.stream())
    sync()
    return rc, buf


def check_attention(c, stage32, valid, buf, dtype, kernel="small_attention"):
    q, k, v = sr.att_operands(stage32)
    ref, bound, A, amp = sr.att_ref(q, k, v, c, valid, dtype)
    nbad, ratio = bounded(buf, sr.att_layout(ref, c), sr.att_layout(bound, c, 0.0))
    t = atr.plain32(q, k, v, sr.att_case(c), valid)
    yard = atr.yardstick(t, ref, A, amp)
    assert yard < sr.ATT_C, (sr.att_id(c), yard)
    note(kernel, dtype, ratio, ar.violations(stored(t, dtype), ref, bound)[1], yard)
    return nbad, ratio


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("c", sr.ATT_CASES, ids=sr.att_id)
def test_small_attention(c, dtype):
    for fam in sr.ATT_FAMILIES:
        d = ar.to_dev(sr.att_inputs(c, fam), DEV)
        rc, buf = launch_attention(c, d, dtype)
        assert rc == 0, L().k22_last_error()
        nbad, ratio = check_attention(c, sr.att_stage32(d, c, dtype), d["key_valid"], buf, dtype)
        print(f"small_attention {sr.att_id(c)} {fam} {sr.DT_NAME[dtype]}: |out - ref| / bound = {ratio:.3f}")
        assert nbad == 0, (sr.att_id(c), fam, nbad, ratio)


# ---- the one-block chain, stage by stage ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_one_block_chain(dtype):
    """the launch sequence of the prior's skinny transformer block (prior.hip) at D = 128, H = 2, T = 17, B = 2 (M = 34, MA = 2): every
    stage's reference is computed from the previous stage's ACTUAL device output, so every per-kernel bound applies unchanged; every fragment
    buffer starts as NaN and keeps NaN in its padding rows to the end."""
    T = hp.tdt(dtype)
    ch = sr.CHAIN
    D, H, Tn, B, tile = ch["D"], ch["H"], ch["T"], ch["B"], ch["tile"]
    M = B * Tn
    cpu = sr.chain_inputs()
    d = ar.to_dev(cpu, DEV)
    wf = {n: repack_w(hp.pad_rows(d["w_" + n].to(T)), dtype) for n in ("qkv", "proj", "fc", "fc2")}
    seen_w = {n: ar.rounded(d["w_" + n], dtype).double() for n in wf}
    worst = 0.0

    def ln_stage(xin, partial, splitk, bias, gname, tag):
        nonlocal worst
        c = sr.FlnCase(M, D, splitk, 0, 1 if gname else 0, 1 if bias is not None else 0)
        dd = {"partial": partial, "bias": bias, "g": d.get("g_" + gname) if gname else None, "b": d.get("be_" + gname) if gname else None}
        xu = sr.x_chain32({"x": xin.cpu(), "partial": None if partial is None else partial.cpu(), "bias": None if bias is None else bias.cpu()})
        rc, xbuf, ybuf = launch_finish_ln(c, dd, xin, dtype)
        assert rc == 0, L().k22_last_error()
        assert torch.equal(xbuf, x_expected(c, xu)), tag
        if gname:
            nbad, ratio = check_ln(c, xu.to(DEV), dd["g"], dd["b"], ybuf, dtype, "chain")
            assert nbad == 0, (tag, nbad, ratio)
            worst = max(worst, ratio)
        return xu.to(DEV), (None if ybuf is None else ybuf[GUARD:-GUARD])

    def gemm_stage(afrag, K, name, N, epi, splitk, act, tag):
        nonlocal worst
        c = sr.GemmCase(M, N, K, splitk, epi, act, 1, tile[0], tile[1], 0)
        bias = d["b_" + name]
        assert int(torch.isnan(afrag).sum()) == sr.afrag_elems(M, K) - M * K, tag        # the producer left the padding rows alone
        rc, buf = launch_gemm(c, afrag, wf[name], bias, dtype)
        assert rc == 0, L().k22_last_error()
        s = {"a": sr.from_afrag(afrag, M, K).double(), "w": seen_w[name], "bias": bias.double()}
        ratio, _, _ = check_gemm(c, s, buf, dtype, "chain " + tag)
        worst = max(worst, ratio)
        note("chain", dtype, ratio)
        return buf[GUARD:-GUARD]

    # 1  LayerNorm ln_1 of the input (no partials)
    x0, y1 = ln_stage(d["x"], None, 0, None, "ln1", "ln_1")
    # 2  c_qkv: row-major T, and split-K partials folded into the attention
    qkv = gemm_stage(y1, D, "qkv", 3 * D, sr.EPI_ROWMAJOR, 1, sr.ACT_NONE, "c_qkv").view(M, 3 * D)
    qkv_part = gemm_stage(y1, D, "qkv", 3 * D, sr.EPI_PARTIAL, ch["sk_qkv"], sr.ACT_NONE, "c_qkv-partials").view(ch["sk_qkv"], M, 3 * D)
    # 3  attention, fragment output, from either form of qkv
    att = {}
    for nsplit in (0, ch["sk_qkv"]):
        c = sr.AttCase(B, H, Tn, 1, ch["n_valid"], ch["kv_n"], 1, nsplit)
        dd = {"qkv": qkv, "part": qkv_part.contiguous() if nsplit else None, "bias": d["b_qkv"] if nsplit else None, "key_valid": d["valid"]}
        rc, buf = launch_attention(c, dd, dtype)
        assert rc == 0, L().k22_last_error()
        stage32 = sr.att_stage32(dd, c, dtype) if nsplit else qkv.float().view(B, Tn, 3, H, atr.HD)
        nbad, ratio = check_attention(c, stage32, d["valid"], buf, dtype, "chain")
        assert nbad == 0, ("attention", nsplit, nbad, ratio)
        worst = max(worst, ratio)
        att[nsplit] = buf[GUARD:-GUARD]
    # 4-5  c_proj partials, finish + residual + ln_2
    p1 = gemm_stage(att[0], D, "proj", D, sr.EPI_PARTIAL, ch["sk_proj"], sr.ACT_NONE, "c_proj").view(ch["sk_proj"], M, D)
    x1, y2 = ln_stage(x0, p1.contiguous(), ch["sk_proj"], d["b_proj"], "ln2", "finish + ln_2")
    # 6-7  c_fc + GELU in fragment order, mlp.c_proj partials
    fc = gemm_stage(y2, D, "fc", 4 * D, sr.EPI_AFRAG, 1, sr.ACT_GELU, "c_fc")
    p2 = gemm_stage(fc, 4 * D, "fc2", D, sr.EPI_PARTIAL, ch["sk_fc2"], sr.ACT_NONE, "mlp.c_proj").view(ch["sk_fc2"], M, D)
    # 8  finish + residual, no LayerNorm behind the last block
    x2, _ = ln_stage(x1, p2.contiguous(), ch["sk_fc2"], d["b_fc2"], "", "finish")
    assert bool(torch.isfinite(x2).all())
    note("chain", dtype, worst)
    print(f"one-block chain {sr.DT_NAME[dtype]}: largest |out - ref| / bound over the stages = {worst:.3f}")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
# Every case is a pair: a launch that is ACCEPTED (asserted), and the same launch with exactly one argument changed, which must return
# K22_EINVAL and leave every buffer at its fill - so the named condition is the only one violated and removing it from the launcher turns the
# case red.  Buffers are sized so that any of these launches, accepted by mistake, would still stay inside them.
def untouched(buf):
    return bool(torch.isnan(buf).all()) if buf.is_floating_point() else bool((buf == FILL32).all())


def refusal_pairs(call, pairs):
    for why, (base, change) in pairs.items():
        rc, bufs = call(**base)
        assert rc == 0, (why, "the unchanged launch must be accepted", L().k22_last_error())
        rc, bufs = call(**dict(base, **change))
        assert rc == _EINVAL and all(untouched(b) for b in bufs), why


def test_skinny_gemm_refusals():
    """every condition of skinny_supported that the C entry can express (it derives MA from M and maps splitk <= 0 to 1 itself), the n-tile
    check and the tile list"""
    af = torch.zeros(sr.afrag_elems(64, 256), dtype=torch.bfloat16, device=DEV)
    wf = torch.zeros(256, 256, dtype=torch.bfloat16, device=DEV)
    bias = torch.zeros(256, device=DEV)

    def call(M=33, N=64, Npad=64, K=128, splitk=1, epi=0, ldo=64, mt=2, nb=2, dtype=sr.BF16, partial=True):
        buf, out = guarded(64 * 256, torch.float32 if epi == 2 else torch.bfloat16)
        p = (None, None, out.data_ptr() if partial else None) if epi == 2 else (bias.data_ptr(), out.data_ptr(), None)
        rc = L().k22_skinny_gemm(af.data_ptr(), wf.data_ptr(), p[0], p[1], p[2], M, N, Npad, K, splitk, epi, 0, ldo, mt, nb, dtype, hp.stream())
        sync()
        return rc, [buf]

    refusal_pairs(call, {
        "dtype fp32": ({}, {"dtype": _lib.K22_F32}),
        "K % 64": ({}, {"K": 96}),
        "Npad % 64": ({"mt": 2, "nb": 1}, {"Npad": 96}),                 # the 32-wide n-tile divides 96: only skinny_supported objects
        "N % 4": ({}, {"N": 62}),                                        # ldo stays 64
        "Npad < N": ({"N": 128, "Npad": 128, "ldo": 128}, {"Npad": 64}),
        "M < 1": ({}, {"M": 0}),
        "splitk > K / 64": ({"epi": 2, "splitk": 2}, {"splitk": 3}),
        "row-major epilogue, ldo % 4": ({}, {"ldo": 66}),
        "fragment epilogue, N % 64": ({"epi": 1}, {"N": 60}),
        "split-K outside the partial epilogue": ({}, {"splitk": 2}),
        "partial epilogue without a buffer": ({"epi": 2}, {"partial": False}),
        "Npad no multiple of the n-tile": ({"mt": 3, "nb": 4, "Npad": 128}, {"Npad": 64}),
        "unknown (mt, nb)": ({}, {"mt": 4}),
    })


def test_finish_ln_refusals():
    partial = torch.zeros(9 * 5 * 2056, device=DEV)                                     # as large as the largest variant
    vec = torch.zeros(2056, device=DEV)

    def call(M=5, N=64, splitk=2, ldx=2056, ln=1, beta=True, with_partial=True, dtype=sr.BF16):
        xbuf, xv = guarded(5 * 2060, torch.int32, fill=FILL32)
        ybuf, yv = guarded(32 * 2112, torch.bfloat16)
        rc = L().k22_finish_ln(partial.data_ptr() if with_partial else None, splitk, vec.data_ptr(), xv.data_ptr(), ldx, vec.data_ptr() if ln else None,
                               vec.data_ptr() if ln and beta else None, yv.data_ptr() if ln else None, M, N, sr.FLN_EPS, dtype, hp.stream())
        sync()
        return rc, [xbuf, ybuf]

    refusal_pairs(call, {
        "N = 2056": ({"ln": 0, "N": 2048}, {"N": 2056}),                 # gain NULL: the N % 64 rule of the LayerNorm output is not in play
        "N % 8": ({"ln": 0}, {"N": 60}),
        "splitk = 9": ({"splitk": 8}, {"splitk": 9}),
        "gain without beta": ({}, {"beta": False}),
        "partials with splitk = 0": ({"splitk": 1}, {"splitk": 0}),
        "LayerNorm output with N % 64": ({}, {"N": 72}),
        "M < 1": ({}, {"M": 0}),
        "ldx % 4": ({}, {"ldx": 2058}),
        "dtype fp32": ({}, {"dtype": _lib.K22_F32}),
    })


def test_small_attention_refusals():
    c = sr.AttCase(1, 1, 129, 1, None, 0, 0, 4)                                         # memory for 129 tokens and five splits
    d = ar.to_dev(sr.att_inputs(c, "rand"), DEV)
    d["part"] = torch.cat([d["part"], d["part"][:1]]).contiguous()

    def call(T_=128, nsplit=0, dtype=sr.BF16):
        dd = d if nsplit else dict(d, part=None, bias=None)                             # the stored qkv, or the partials + bias
        rc, buf = launch_attention(c._replace(nsplit=1 if nsplit else 0), dd, sr.BF16, T_=T_, nsplit=nsplit, dt_arg=dtype)
        return rc, [buf]

    refusal_pairs(call, {"T = 129": ({}, {"T_": 129}), "nsplit = 5": ({"nsplit": 4}, {"nsplit": 5}), "dtype fp32": ({}, {"dtype": _lib.K22_F32})})


def test_afrag_pack_refusals():
    a = torch.zeros(33, 136, dtype=torch.bfloat16, device=DEV)

    def call(M=33, K=128, lda=136, dtype=sr.BF16):
        buf, out = guarded(sr.afrag_elems(33, 128), torch.bfloat16)
        rc = L().k22_afrag_pack(a.data_ptr(), lda, out.data_ptr(), M, K, dtype, hp.stream())
        sync()
        return rc, [buf]

    refusal_pairs(call, {"K % 64": ({}, {"K": 96}), "lda % 8": ({}, {"lda": 132}), "M < 1": ({}, {"M": 0}), "dtype fp32": ({}, {"dtype": _lib.K22_F32})})


# ---- measured ratios ------------------------------------------------------------------------------------------------------------------------
def test_zz_report_measured_ratios():
    """a report, not a gate: the figures of the cases that ran in THIS process before it (every case asserts its own bound where it runs; under
    a selection or another order this prints less and checks nothing)"""
    print("\nskinny family on this device: largest |out - ref| / bound, kernel | torch's fp32 evaluation rounded to T | torch fp32 yardstick")
    for (kernel, dt), (r, t, y) in sorted(STATS.items()):
        print(f"  {kernel:24s} {dt}   {r:.3f} | {t:.3f} | {y:.2f}")
    print(f"  c: GEMM {sr.GEMM_C:.2f}, LayerNorm {sr.LN_C:.2f}, attention {sr.ATT_C:.1f};  {len(STATS)} rows; since this file's import {time.time() - T0:.1f} s")
    for (kernel, _), (r, _, _) in STATS.items():
        assert r <= 1.0, kernel
