// k22 — nearest 2x upsample + 3x3 convolution as FOUR 2x2 convolutions of the low-resolution tensor (the in_layers of an up-sampling
// ResBlock, unet.py:158-159, 204: Upsample(channels, False) = F.interpolate(scale_factor=2, mode="nearest"), then conv3x3).
//
// Output pixel (2y + py, 2x + px) reads, through tap ky of the 3x3 filter, low-resolution row y + floor((py + ky - 1) / 2): phase py = 0
// uses rows {-1: ky = 0;  0: ky = 1, 2}, phase py = 1 rows {0: ky = 0, 1;  +1: ky = 2}; columns alike.  So each of the four output phases
// (py, px) is a 2x2 convolution of the low-resolution tensor whose weights are sums of 1, 2 or 4 of the original taps (folded once, in
// fp32, before the one rounding to the engine type: pack.py fold_up2 / k22_up2_fold).  The zero border of the low-resolution padded plane
// stands for the zero border of the up-sampled one: hi-res row -1 is reached only through (py = 0, ky = 0) = low-res row -1, hi-res row 2H
// only through low-res row H.  16 tap-GEMMs at a quarter of the rows = 4/9 of the MFMA work, and the GroupNorm-apply in front writes the
// low-resolution tensor instead of the 4x larger one.
//
// The kernel is the lock-step LDS-resident-halo kernel (conv3_halo.hip) with the phase as one more grid dimension:
//   * a workgroup owns BM consecutive positions v = y*(W+2) + x of the low-resolution padded plane of one image, one 128-wide n-tile and ONE
//     phase; tap (a, b) of phase (py, px) is input v + (py + a)*(W+2) + (px + b), so the LDS image starts at v0 + py*(W+2) + px and holds
//     BM + (W+2) + 1 rows (9-tap form: BM + 2*(W+2) + 2)
//   * weights Wp [phase 4][Npad][tap 2x2][Kc]; the tap loop runs over 4 taps per slab; weight tiles in an NBST-deep ring (4, or 2 where the LDS is short), the next
//     slab's halo is issued in taps 0 .. 4-NBST (6 / (5-NBST) pieces per wave each: all six in tap 0 at NBST = 4) so that it is older than the NBST-2 weight tiles the
//     counted vmcnt leaves in flight when the slab begins
//   * two forms of the tap loop: compiler-scheduled (IG_ALGO_UP2; every type) and the explicit two-set fragment pipeline of conv3_halo_kernel's
//     MODE 1 (IG_ALGO_UP2_PIPE; the 16-bit types, where igemm_resolve's rule picks it); same fragments in the same order: the same bits
//   * epilogue = halo_tail (conv3_common.h) with the phase row mapping: bias once, row (b, y, x) stored at (b, 2y+py, 2x+px) of the unpadded
//     hi-res row-major output, GroupNorm partial sums in row (img*4 + phase)*TPI + tile (4*TPI rows per image), split-K partials over the
//     hi-res rows finished by the usual fixed-order reduction
#include "conv3_common.h"

// PIPE (16-bit types): the explicit fragment pipeline of conv3_halo_kernel's MODE 1.  The kernel is a thin entry to the shared frame
// and the lock-step K loop of conv3_common.h with TAPS = 4: taps 0 .. 4-NBST issue the next slab's halo, UP2_ASLOTS / (5-NBST) pieces per
// wave each.
template <typename T, int BM, int NBST, bool PIPE>
__global__ __launch_bounds__(512) void conv3_up2_kernel(const IgemmParams p) {
  using TR = TT<T>;
  constexpr int BK = TR::BK, EPC = TR::EPC, KSTEPS = TR::KSTEPS;
  constexpr int BN = HALO_BN, NW = HALO_NW, WM = 4, WN = 2;
  constexpr int MI = BM / (WM * 32), NI = BN / (WN * 32);
  constexpr int B_SLOTS = BN / 8 / NW;   // weight LDS-DMA instructions per wave per tap
  constexpr int B_BYTES = BN * 128;
  constexpr int HPT = UP2_ASLOTS / (5 - NBST);   // halo pieces per wave in each of taps 0 .. 4-NBST (NBST 2: 2, NBST 4: 6)
  constexpr bool GASM = true;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, l31 = lane & 31;

  const int W2 = p.W + 2;                      // low-resolution padded row
  const int VR = p.H * W2;                     // virtual output rows per image and phase
  const int TPI = (VR + BM - 1) / BM;          // m-tiles per image
  const int HRp = (BM + W2 + 1 + 7) & ~7;      // halo rows (whole 8-row LDS-DMA pieces)
  const int NP = HRp >> 3;
  const int A_BYTES = HRp * 128;
  const int PR_MAX = (p.H + 2) * W2 - 1;       // last pixel of one padded plane
  const int B = p.M / (4 * p.H * p.W);

  // block -> (m-tile, n-tile x phase, k-split): the phase is the fastest part of the n index
  int bz, bx, byp;
  tile_block_map(p.xcd_remap, B * TPI, ((p.N + BN - 1) / BN) * 4, bz, bx, byp);
  const int ph = byp & 3, by = byp >> 2;
  const int img = bx / TPI, tile = bx - img * TPI, v0 = tile * BM;
  const int n0 = by * BN;
  const int base = v0 + (ph >> 1) * W2 + (ph & 1);   // first plane position of this phase's LDS image

  const T* __restrict__ Aimg = reinterpret_cast<const T*>(p.A0) + (int64_t)img * (p.H + 2) * W2 * p.Kc;
  const T* __restrict__ Wp = reinterpret_cast<const T*>(p.Wp);
  int aoff[UP2_ASLOTS], boff[B_SLOTS];
  K22_PIECE_OFFSETS(aoff, UP2_ASLOTS, wave, NW, base, NP, 8)
  K22_ROW_OFFSETS(boff, B_SLOTS, wave, NW, n0, p.Npad - 1, (ph * p.Npad + n) * 4 * p.Kc)
  int s0, s1;
  splitk_range(p.splitk, p.Kc / BK, bz, s0, s1);

  f32x16_t acc[MI][NI];
  K22_ZERO_ACC(acc, MI, NI)
  FragA<T> pa[MI];          // PIPE: fragments read but not yet multiplied (zero = a no-op group before the first tap)
  Frag<T> pb[NI];
  if constexpr (PIPE) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) pa[mi] = FragA<T>{};
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) pb[ni] = Frag<T>{};
  }
  char* const Bst = smem + 2 * A_BYTES;
  const int abase = wm * (BM / WM) + l31;
  int brow[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) brow[ni] = (wn * (BN / WN) + ni * 32 + l31) * 128;
  const int bsw = (l31 >> 1) & 7;
  const unsigned lds0 = halo_lds_base(smem);

#define K22_UP2_BODY                                                                                       \
  if constexpr (PIPE) K22_TAP_PIPE(FragA<T>, Frag<T>, arow[mi], asw[mi], Bcur + brow[ni], bsw, K22_PIPE_LOCKSTEP) \
  else { K22_TAP_PLAIN(FragA<T>, Frag<T>, ld_frag_at, arow[mi], asw[mi], Bcur + brow[ni], bsw) }
  K22_LOCKSTEP_LOOP(4, UP2_ASLOTS, HPT, K22_UP2_BODY)
#undef K22_UP2_BODY
  if constexpr (PIPE) { K22_MMA_ALL(pb, pa) }
  halo_tail<T, BM, false, false, true>(p, acc, smem, (img * 4 + ph) * TPI + tile, bz, img, v0, n0, ph);
}

// ---- host side ---------------------------------------------------------------------------------
size_t conv3_up2_lds_bytes(const IgemmParams& p, int bm, int nbst) { return halo_smem_bytes(p, bm, nbst, 4); }
int conv3_up2_ring(const IgemmParams& p, int bm) { return halo_pick_nbst(p, bm, 4); }   // 4 or 2; 0 = the problem does not fit
int conv3_up2_tiles_per_image(const IgemmParams& p, int bm) { return halo_tiles_per_image(p, bm); }

// p: taps == 4, H x W = the LOW resolution, M = B * 2H * 2W output rows, A0 = [B][H+2][W+2][Kc] zero-bordered, Wp = [4][Npad][4][Kc]
bool conv3_up2_supported(const IgemmParams& p, int dtype, int bm) {
  const int BK = k22_bk(dtype);
  if (p.taps != 4 || (bm != 256 && bm != 128)) return false;
  if (p.a_raw || p.S0 != nullptr || p.A1 != nullptr || p.res_f32) return false;
  if (p.out_mode != IG_OUT_ROWMAJOR && p.out_mode != IG_OUT_ROWMAJOR_F32) return false;
  if (p.N % 8 || p.ldo % 8 || (p.residual && p.ldr % 8) || p.Kc % BK || p.K0 != p.Kc) return false;
  if (p.H <= 0 || p.W <= 0 || p.M % (4 * p.H * p.W)) return false;
  if (conv3_up2_ring(p, bm) == 0) return false;
  if ((int64_t)(p.H + 2) * (p.W + 2) * p.Kc >= (1ll << 31) || (int64_t)p.Npad * 16 * p.Kc >= (1ll << 31)) return false;
  return true;
}

int launch_conv3_up2(const IgemmParams& p, int dtype, const IgemmLaunch& L, hipStream_t stream) {
  return k22_with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return halo_with_bm(L.bm, [&](auto bm) {
      auto depth = [&](auto pipe) {
        return halo_with_depth<2, 4>(L.depth, [&](auto d) { return halo_run<conv3_up2_kernel<T, decltype(bm)::value, decltype(d)::value, decltype(pipe)::value>>(p, L, stream); });
      };
      if constexpr (sizeof(T) == 2) {
        if (L.pipe) return depth(std::true_type{});
      }
      return depth(std::false_type{});
    });
  });
}

// ---- the fold: 3x3 weights [O][3][3][I] fp32 (pack order: tap-major, channel contiguous) -> phase weights [4][Opad][2][2][I] fp32 ----------
// tap ky of phase py lands in low-resolution row slot a = (py + ky + 1) / 2 - py: py = 0: {0 | 1, 2}, py = 1: {0, 1 | 2}; columns alike.
// Sums run in fp32 in the fixed order ky, kx ascending; rows O .. Opad-1 are zero.
__global__ __launch_bounds__(256) void up2_fold_kernel(const float* __restrict__ w, float* __restrict__ out, int O, int Opad, int I) {
  const int64_t total = (int64_t)4 * Opad * 4 * I;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % I);
    const int tap = (int)((e / I) & 3);
    const int o = (int)((e / ((int64_t)4 * I)) % Opad);
    const int ph = (int)(e / ((int64_t)4 * I * Opad));
    const int py = ph >> 1, px = ph & 1, a = tap >> 1, b = tap & 1;
    float acc = 0.f;
    if (o < O)
      for (int ky = 0; ky < 3; ++ky) {
        if ((py + ky + 1) / 2 - py != a) continue;
        for (int kx = 0; kx < 3; ++kx) {
          if ((px + kx + 1) / 2 - px != b) continue;
          acc += w[((int64_t)o * 9 + ky * 3 + kx) * I + c];
        }
      }
    out[e] = acc;
  }
}

int launch_up2_fold(const float* w, float* out, int O, int Opad, int I, hipStream_t stream) {
  if (!w || !out || O <= 0 || I <= 0 || Opad < O) return k22_set_error(K22_EINVAL, "up2_fold: bad argument");
  const int64_t total = (int64_t)16 * Opad * I;
  int nb = (int)((total + 255) / 256);
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(up2_fold_kernel, dim3(nb), dim3(256), 0, stream, w, out, O, Opad, I);
  K22_CHECK_LAUNCH();
  return K22_OK;
}
