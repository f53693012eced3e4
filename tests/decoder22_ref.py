"""References and bounds of the one-graph 2.2 decoder loop (k22_keep_region, k22_unet_sample_loop_keep, UNet2DConditionHIP.sample_loop),
for tests/test_decoder22_loop_cpu.py and tests/test_decoder22_loop_gpu.py.  A plain module like aux_ref.py.

PARITY UNPINNED, as everything on the 2.2 path: the loop restatements these tests compare with (oracle/unet22_ref.py) are written from
memory of diffusers' source, which is absent from the reference tree.  The tests check that the ENGINE computes what the restatement
says, and that the one-graph route computes what the stepwise route computes.

keep_region, from its definition (include/k22.h; the re-imposition of the known region in the KandinskyV22InpaintPipeline loop):

    out[n][c][p] = m[p] * (sa * init[c][p] + sb * noise0[n % bs][c][p]) + (1 - m[p]) * x[n][c][p]        n < B = 2 bs

Bound, class D of aux_ref.py with the kernel's own rounding count: every operation of the kernel is rounded once (__fmul_rn / __fadd_rn /
__fsub_rn: no contraction), so

    |out - ref| <= n * 2^-24 * S,    S = |m| (|sa init| + |sb noise|) + |1 - m| |x|,    n = 4

n = the roundings on the longest path: product (sa * init or sb * noise, siblings), inner sum, product by m, outer sum.  The other
path - the difference 1 - m, the product by x, the outer sum - has three.  Nothing in it is measured."""
import torch

U24 = 2.0 ** -24
KEEP_N = 4
NAN = float("nan")
MUTANTS = ("noise_sample0", "noise_by_n", "mask_row", "swap_sa_sb", "no_one_minus_m", "init_per_sample")


def gen(seed):
    return torch.Generator().manual_seed(1000003 * seed + 41)


def keep_inputs(bs, H, W, mask_kind="binary", seed=0):
    """fp32 operands of one launch: x [2 bs,4,H,W], init [4,H,W], noise0 [bs,4,H,W], mask [H,W] (binary: about 60 % kept; fractional:
    uniform in [0, 1], what a resized soft mask would hold)"""
    g = gen(seed)
    x = 0.3 + 1.7 * torch.randn(2 * bs, 4, H, W, generator=g)
    init = 0.2 + 1.3 * torch.randn(4, H, W, generator=g)
    noise0 = torch.randn(bs, 4, H, W, generator=g)
    u = torch.rand(H, W, generator=g)
    mask = (u > 0.4).float() if mask_kind == "binary" else u
    return dict(x=x, init=init, noise0=noise0, mask=mask)


def keep_region_ref(d, sa, sb, mut=None, dtype=torch.float64):
    """(out, S) in `dtype` (float64: the reference; float32: torch's own evaluation, one rounding per operation as the kernel); sa / sb
    are the fp32 values the kernel receives.  mut: ONE deliberately wrong variant (the CPU test shows each rejected)."""
    x, init, nz, m = (d[k].to(dtype) for k in ("x", "init", "noise0", "mask"))
    B, bs = x.shape[0], nz.shape[0]
    sa_, sb_ = torch.tensor(float(sa), dtype=dtype), torch.tensor(float(sb), dtype=dtype)
    if mut == "swap_sa_sb":
        sa_, sb_ = sb_, sa_
    rows = torch.arange(B) % bs
    if mut == "noise_sample0":
        rows = torch.zeros(B, dtype=torch.long)
    noise = nz[rows]                                              # [B,4,H,W]: both CFG halves of a sample share its noise
    if mut == "noise_by_n":                                       # rows bs .. B-1 read past noise0: whatever lies behind it, here other data
        noise = torch.cat([nz, nz.flip(0) * 0.5 + 0.25], 0)
    ini = init[None].expand(B, -1, -1, -1)
    if mut == "init_per_sample":                                  # init read as [B][4][HW]: only row 0 is the image
        ini = torch.stack([init.roll(n, dims=0) for n in range(B)])
    mk = m[None, None]
    if mut == "mask_row":
        mk = m.roll(1, dims=0)[None, None]
    one_m = torch.ones((), dtype=dtype) if mut == "no_one_minus_m" else (1 - mk)
    a, b = sa_ * ini, sb_ * noise
    out = mk * (a + b) + one_m * x
    S = mk.abs() * (a.abs() + b.abs()) + (1 - mk).abs() * x.abs()
    return out, S


def keep_bound(S):
    return KEEP_N * U24 * S


def violations(out, ref, bound):
    """elements of out further from ref than bound, non-finite ones included"""
    o = out.double()
    return int((~torch.isfinite(o) | ((o - ref).abs() > bound)).sum().item())


def worst_ratio(out, ref, bound):
    r = (out.double() - ref).abs() / bound.clamp_min(1e-300)
    return float(r[bound > 0].max().item()) if (bound > 0).any() else 0.0


def with_guard(t, guard, fill=NAN):
    """flat copy of t with `guard` fill elements on both sides (the layout of the GPU test's buffers)"""
    g = torch.full((guard,), fill, dtype=t.dtype, device=t.device)
    return torch.cat([g, t.reshape(-1), g])
