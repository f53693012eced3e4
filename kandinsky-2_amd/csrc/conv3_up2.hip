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

namespace {
// halo pieces issued in the NBST-1 iterations before tap T (all younger than the weight tile tap T needs): taps 0 .. 4-NBST issue HPT each
template <int NBST> constexpr int up2_halo_count(int t) {
  int c = 0;
  for (int k = 1; k <= NBST - 1; ++k) {
    const int u = t - k;
    if (u >= 0 && u <= 4 - NBST) ++c;
  }
  return c;
}
constexpr int UP2_ASLOTS = 6;   // halo LDS-DMA slots per wave per slab: 48 pieces = 384 rows
}  // namespace

// PIPE (16-bit types): the explicit fragment pipeline of conv3_halo_kernel's MODE 1 - the fragments of k-step ks+1 are read before the
// MFMAs of k-step ks are issued, and the last k-step of a tap is multiplied behind the next tap's barrier.
template <typename T, int BM, int NBST, bool PIPE>
__global__ __launch_bounds__(512) void conv3_up2_kernel(const IgemmParams p) {
  using TR = TT<T>;
  constexpr int BK = TR::BK, EPC = TR::EPC, KSTEPS = TR::KSTEPS;
  constexpr int BN = HALO_BN, NW = HALO_NW, WM = 4, WN = 2;
  constexpr int MI = BM / (WM * 32), NI = BN / (WN * 32);
  constexpr int B_SLOTS = BN / 8 / NW;   // weight LDS-DMA instructions per wave per tap
  constexpr int B_BYTES = BN * 128;
  constexpr int HT = 5 - NBST;           // taps 0 .. HT-1 issue the next slab's halo
  constexpr int HPT = UP2_ASLOTS / HT;   // pieces per wave in each of them (NBST 2: 2, NBST 4: 6)
  constexpr int GM = 8;
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

  // ---- block -> (m-tile, n-tile x phase, k-split): the phase is the fastest part of the n index ----
  const int gx = B * TPI, gy = ((p.N + BN - 1) / BN) * 4;
  int L = p.xcd_remap ? xcd_remap_h(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int per_z = gx * gy;
  const int bz = L / per_z;
  L -= bz * per_z;
  const int grp = L / (GM * gy);
  const int first_m = grp * GM;
  const int gsz = gx - first_m < GM ? gx - first_m : GM;
  const int lin = L - grp * GM * gy;
  const int bx = first_m + lin % gsz, byp = lin / gsz;
  const int ph = byp & 3, by = byp >> 2;
  const int img = bx / TPI, tile = bx - img * TPI, v0 = tile * BM;
  const int n0 = by * BN;
  const int base = v0 + (ph >> 1) * W2 + (ph & 1);   // first plane position of this phase's LDS image

  const T* __restrict__ Aimg = reinterpret_cast<const T*>(p.A0) + (int64_t)img * (p.H + 2) * W2 * p.Kc;
  const T* __restrict__ Wp = reinterpret_cast<const T*>(p.Wp);

  // ---- loader geometry: halo piece j (8 rows) is issued by wave j % NW in its slot j / NW; lane -> (row 8j + lane/8, position lane%8) ----
  int aoff[UP2_ASLOTS];
#pragma unroll
  for (int q = 0; q < UP2_ASLOTS; ++q) {
    int j = q * NW + wave;
    if (j > NP - 1) j = NP - 1;   // surplus slots re-load the last piece (same bytes, same place): uniform counting
    const int hr = 8 * j + (lane >> 3);
    int pr = base + hr;
    if (pr > PR_MAX) pr = PR_MAX;
    const int chunk = (lane & 7) ^ ((hr >> 1) & 7);
    aoff[q] = pr * p.Kc + chunk * EPC;
  }
  int boff[B_SLOTS];
#pragma unroll
  for (int i = 0; i < B_SLOTS; ++i) {
    const int row = 8 * (wave + NW * i) + (lane >> 3);
    int n = n0 + row;
    if (n > p.Npad - 1) n = p.Npad - 1;
    const int chunk = (lane & 7) ^ ((row >> 1) & 7);
    boff[i] = (ph * p.Npad + n) * 4 * p.Kc + chunk * EPC;
  }
  const int nslab = p.Kc / BK;
  int s0 = 0, s1 = nslab;
  if (p.splitk > 1) {
    const int per = (nslab + p.splitk - 1) / p.splitk;
    s0 = bz * per;
    s1 = s0 + per < nslab ? s0 + per : nslab;
  }

  f32x16_t acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

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

  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)smem);
#define K22_ISSUE_A(Q, SLAB, DST)                                                                          \
  {                                                                                                        \
    int j_ = (Q) * NW + wave;                                                                              \
    if (j_ > NP - 1) j_ = NP - 1;                                                                          \
    glds16_asm(Aimg + aoff[Q] + (SLAB) * BK, __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((DST) - smem) + j_ * 1024)); \
  }
#define K22_ISSUE_B(SLAB, TAP, STAGE)                                                                      \
  {                                                                                                        \
    const int kofs_ = (TAP) * p.Kc + (SLAB) * BK;                                                          \
    char* dst_ = Bst + (STAGE) * B_BYTES + wave * 1024;                                                    \
    _Pragma("unroll") for (int i = 0; i < B_SLOTS; ++i)                                                    \
        glds16w_asm(Wp + boff[i] + kofs_, __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(dst_ - smem) + i * NW * 1024)); \
  }

  if (s0 < s1) {
    // prologue: the whole halo of the first slab, then the weight tiles of taps 0 .. NBST-2 (NBST <= 4: all of the first slab)
#pragma unroll
    for (int q = 0; q < UP2_ASLOTS; ++q) K22_ISSUE_A(q, s0, smem);
#pragma unroll
    for (int t = 0; t < NBST - 1; ++t) K22_ISSUE_B(s0, t, t);
    int cur = 0;               // ring slot of the current tap's weights
    int fill = NBST - 1;       // ring slot the tile NBST-1 taps ahead goes into
    for (int s = s0; s < s1; ++s) {
      char* const Acur = smem + ((s - s0) & 1) * A_BYTES;
      char* const Anext = smem + (((s - s0) & 1) ^ 1) * A_BYTES;
      const int sn = s + 1 < s1 ? s + 1 : s1 - 1;  // past-the-end loads re-read the last slab (uniform counting)
      // VMEM queue of a wave per tap: [weight tile NBST-1 taps ahead (B_SLOTS)] then [HPT halo pieces, taps < HT].  At the top of tap T the
      // weight tile of T has landed when at most the B_SLOTS*(NBST-2) younger weight loads and the halo pieces issued since are in flight;
      // the last halo piece of a slab (tap HT-1) is followed by the weight loads of NBST-1 taps, so at tap 0 of the next slab it is older
      // than everything the wait leaves in flight.
#define K22_TAP(TAP)                                                                                       \
      {                                                                                                    \
        wait_vmcnt<B_SLOTS * (NBST - 2) + HPT * up2_halo_count<NBST>(TAP)>();                              \
        raw_barrier();                                                                                     \
        {                                                                                                  \
          constexpr int ta_ = ((TAP) + NBST - 1) % 4;                                                      \
          const int sa_ = ((TAP) + NBST - 1 >= 4) ? sn : s;                                                \
          K22_ISSUE_B(sa_, ta_, fill);                                                                     \
          if constexpr ((TAP) < HT) {                                                                      \
            _Pragma("unroll") for (int a_ = 0; a_ < HPT; ++a_) {                                           \
              constexpr int qb_ = ((TAP) < HT ? (TAP) : 0) * HPT;                                          \
              K22_ISSUE_A(qb_ + a_, sn, Anext);                                                            \
            }                                                                                              \
          }                                                                                                \
        }                                                                                                  \
        const char* Bcur = Bst + cur * B_BYTES;                                                            \
        const int shift = ((TAP) >> 1) * W2 + ((TAP) & 1);                                                 \
        const char* arow[MI];                                                                              \
        int asw[MI];                                                                                       \
        _Pragma("unroll") for (int mi = 0; mi < MI; ++mi) {                                                \
          const int ar = abase + mi * 32 + shift;                                                          \
          arow[mi] = Acur + ar * 128;                                                                      \
          asw[mi] = (ar >> 1) & 7;                                                                         \
        }                                                                                                  \
        if constexpr (PIPE) {                                                                              \
          FragA<T> ca[MI];                                                                                 \
          Frag<T> cb[NI];                                                                                  \
          _Pragma("unroll") for (int ks = 0; ks < KSTEPS; ks += 2) {                                       \
            _Pragma("unroll") for (int mi = 0; mi < MI; ++mi) ld_frag_at(ca[mi], arow[mi], asw[mi], ks, h); \
            _Pragma("unroll") for (int ni = 0; ni < NI; ++ni) ld_frag_at(cb[ni], Bcur + brow[ni], bsw, ks, h); \
            __builtin_amdgcn_sched_barrier(0);                                                             \
            _Pragma("unroll") for (int mi = 0; mi < MI; ++mi)                                              \
              _Pragma("unroll") for (int ni = 0; ni < NI; ++ni) mma_atom(acc[mi][ni], pb[ni], pa[mi]);     \
            __builtin_amdgcn_sched_barrier(0);                                                             \
            _Pragma("unroll") for (int mi = 0; mi < MI; ++mi) ld_frag_at(pa[mi], arow[mi], asw[mi], ks + 1, h); \
            _Pragma("unroll") for (int ni = 0; ni < NI; ++ni) ld_frag_at(pb[ni], Bcur + brow[ni], bsw, ks + 1, h); \
            __builtin_amdgcn_sched_barrier(0);                                                             \
            _Pragma("unroll") for (int mi = 0; mi < MI; ++mi)                                              \
              _Pragma("unroll") for (int ni = 0; ni < NI; ++ni) mma_atom(acc[mi][ni], cb[ni], ca[mi]);     \
            __builtin_amdgcn_sched_barrier(0);                                                             \
          }                                                                                                \
        } else {                                                                                           \
        _Pragma("unroll") for (int ks = 0; ks < KSTEPS; ++ks) {                                            \
          FragA<T> a[MI];                                                                                  \
          Frag<T> b[NI];                                                                                   \
          _Pragma("unroll") for (int mi = 0; mi < MI; ++mi) ld_frag_at(a[mi], arow[mi], asw[mi], ks, h);   \
          _Pragma("unroll") for (int ni = 0; ni < NI; ++ni) ld_frag_at(b[ni], Bcur + brow[ni], bsw, ks, h); \
          _Pragma("unroll") for (int mi = 0; mi < MI; ++mi)                                                \
            _Pragma("unroll") for (int ni = 0; ni < NI; ++ni) mma_atom(acc[mi][ni], b[ni], a[mi]);         \
        }                                                                                                  \
        }                                                                                                  \
        /* no fragment read of this tap's weight slot in flight when the slot is refilled after the next barrier */ \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                 \
        cur = (cur + 1 == NBST) ? 0 : cur + 1;                                                             \
        fill = (fill + 1 == NBST) ? 0 : fill + 1;                                                          \
      }
      K22_TAP(0) K22_TAP(1) K22_TAP(2) K22_TAP(3)
#undef K22_TAP
    }
  }
#undef K22_ISSUE_A
#undef K22_ISSUE_B
  if constexpr (PIPE) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) mma_atom(acc[mi][ni], pb[ni], pa[mi]);
  }
  halo_tail<T, BM, false, false, true>(p, acc, smem, (img * 4 + ph) * TPI + tile, bz, img, v0, n0, ph);
}

// ---- host side ---------------------------------------------------------------------------------
static int up2_rows(const IgemmParams& p, int bm) { return (bm + (p.W + 2) + 1 + 7) & ~7; }

size_t conv3_up2_lds_bytes(const IgemmParams& p, int bm, int nbst) {
  const size_t main_loop = (size_t)2 * up2_rows(p, bm) * 128 + (size_t)nbst * HALO_BN * 128;
  const size_t epi = (size_t)bm * (HALO_BN * 4 + 16);
  const size_t red = (size_t)32 * HALO_BN * 2 * 4;
  const size_t m = main_loop > epi ? main_loop : epi;
  return m > red ? m : red;
}

// deepest instantiated weight ring (4, 2) that fits the LDS next to the double-buffered halo; 0 = the problem does not fit
int conv3_up2_ring(const IgemmParams& p, int bm) {
  if (up2_rows(p, bm) / 8 > UP2_ASLOTS * HALO_NW) return 0;
  for (int nbst : {4, 2})
    if (conv3_up2_lds_bytes(p, bm, nbst) <= 160 * 1024) return nbst;
  return 0;
}

int conv3_up2_tiles_per_image(const IgemmParams& p, int bm) { return (p.H * (p.W + 2) + bm - 1) / bm; }

// p: taps == 4, H x W = the LOW resolution, M = B * 2H * 2W output rows, A0 = [B][H+2][W+2][Kc] zero-bordered, Wp = [4][Npad][4][Kc]
bool conv3_up2_supported(const IgemmParams& p, int dtype, int bm) {
  const int BK = k22_bk(dtype);
  if (p.taps != 4 || (bm != 256 && bm != 128)) return false;
  if (p.a_raw || p.gn_coeff != nullptr || p.S0 != nullptr || p.A1 != nullptr || p.res_f32) return false;
  if (p.out_mode != IG_OUT_ROWMAJOR && p.out_mode != IG_OUT_ROWMAJOR_F32) return false;
  if (p.N % 8 || p.ldo % 8 || (p.residual && p.ldr % 8) || p.Kc % BK || p.K0 != p.Kc) return false;
  if (p.H <= 0 || p.W <= 0 || p.M % (4 * p.H * p.W)) return false;
  if (conv3_up2_ring(p, bm) == 0) return false;
  if ((int64_t)(p.H + 2) * (p.W + 2) * p.Kc >= (1ll << 31) || (int64_t)p.Npad * 16 * p.Kc >= (1ll << 31)) return false;
  return true;
}

template <typename T, int BM, int NBST, bool PIPE>
static int run_up2(const IgemmParams& p, const IgemmLaunch& L, hipStream_t stream) {
  static LdsAttrGuard guard;
  return launch_lds_kernel(conv3_up2_kernel<T, BM, NBST, PIPE>, guard, L.grid, L.block, L.lds, 160 * 1024, stream, p);
}
template <typename T, int BM>
static int launch_up2_depth(const IgemmParams& p, const IgemmLaunch& L, hipStream_t stream) {
  if constexpr (sizeof(T) == 2) {
    if (L.pipe) return L.depth == 2 ? run_up2<T, BM, 2, true>(p, L, stream) : run_up2<T, BM, 4, true>(p, L, stream);
  }
  return L.depth == 2 ? run_up2<T, BM, 2, false>(p, L, stream) : run_up2<T, BM, 4, false>(p, L, stream);
}

int launch_conv3_up2(const IgemmParams& p, int dtype, const IgemmLaunch& L, hipStream_t stream) {
  return k22_with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return L.bm == 256 ? launch_up2_depth<T, 256>(p, L, stream) : launch_up2_depth<T, 128>(p, L, stream);
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
