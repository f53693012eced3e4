// k22 — 3x3 convolution with the input tile (+halo) RESIDENT IN LDS across the nine filter taps.
//
// Replaces nn.Conv2d 3x3 of the ResBlocks (kandinsky2/model/unet.py:152,180; ~83 % of the FLOPs of a
// denoise step).  The generic implicit GEMM (igemm.hip) re-fetches the A operand for every tap: 9 x BM rows
// per 64-channel slab, and at 128x128 tiles the L2->LDS path (~56-64 B/clk/CU) is as busy as the MFMA pipes.
// Here the pixels are indexed in the PADDED row-major plane, v = y*(W+2) + x, so that tap (ky,kx) of output v
// is input v + ky*(W+2) + kx: a pure 1-D shift.  A block owns BM consecutive v of one image and keeps the
// BM + 2*(W+2) + 2 input pixels it needs (x 64 channels = one 128-byte row each) in LDS; every tap reads its A
// fragments from the same LDS image at a different row offset.  Outputs with x >= W (two "junk" columns per
// row, 2 % at 96x96) are computed and dropped.  Per slab a block moves (BM + 2W + 6) + 9*BN rows instead of
// 9*(BM + BN): 188 FLOP/B at 256x128 against 64 FLOP/B before, and 3 LDS-DMA instructions per wave per tap
// instead of 8.
//
//   * 8 waves (4 along M x 2 along N), BM in {256, 128}, BN = 128, K slab = 128 bytes of channels
//   * halo buffer double-buffered across slabs (the next slab's halo trickles in, one 8-row piece per wave per
//     tap), weight tiles in an NBST-deep ring (2, 3, 4 or 6: as many as the LDS holds next to the halo) with a COUNTED
//     vmcnt: NBST-1 taps of weights are in flight across the ONE raw s_barrier per tap (at the low-resolution
//     levels the weights stream from HBM, ~2 us away, and a tap is ~0.4 us of MFMA work)
//   * LDS images are lane-linear per LDS-DMA instruction with the chunk-XOR swizzle of common.h on the source
//     address and on the reads (rows of an atom are consecutive -> conflict-free ds_read_b128)
//   * transposed MFMA (lane = pixel, registers = 4 consecutive channels) and an epilogue that goes through LDS:
//     fp32 tile -> 32 B per thread row segments: bias, residual, one rounding, 16-byte stores, and the per-channel
//     (sum, sum of squares) of the STORED values for the next GroupNorm (deterministic, no atomics)
//   * split-K over channel slabs for the low-resolution levels (fp32 partials, finished by splitk_reduce)
//   * variants selected by p.algo (measured in DESIGN.md section 9): 2 = this kernel; 7 = its LDS-DMA issued from inline asm
//     (exact lgkmcnt for the fragment reads; the tuner's usual pick); 6 = 7 + explicit fragment pipeline; 3 = conv3_halo3 below.
//     gemm8_kernel (plain GEMM on the same frame, qkv / proj_out) is in gemm8.hip; both share the epilogue
//     (halo_tail, conv3_common.h)
//   * optional fused 1x1 skip_connection of the ResBlock (out += x . Ws^T): a second, plain-GEMM K loop over the
//     block input's channels (A rows = the tile's own pixels, no halo) that accumulates into the same registers,
//     so the skip tensor is never written, re-read or launched separately
#include "conv3_common.h"

// Every wave issues its share of the LDS-DMA right after the barrier: 3 pieces per wave per tap.  (A 4-loader form - p.algo 5 - measured
// 2-5 % slower in round 1 and was deleted in round 5.)
// PIPE: explicit fragment pipeline across the per-tap barrier.  The fragments of k-step ks+1 are read from LDS BEFORE
// the MFMAs of k-step ks are issued (two register sets), and the last k-step of a tap is multiplied after the NEXT
// tap's barrier, where it covers the LDS-DMA issue and the first fragment reads of that tap: a wave never parks on
// lgkmcnt with an empty matrix pipe behind it (the compiler's own schedule reads one MFMA ahead of the use).
template <typename T, int BM, int NBST, int MODE = 0>
__global__ __launch_bounds__(512) void conv3_halo_kernel(const IgemmParams p) {
  constexpr bool PIPE = MODE == 1;      // explicit fragment pipeline (above)
  constexpr bool GASM = MODE == 1 || MODE == 2;  // LDS-DMA from inline asm (glds16_asm): exact lgkmcnt(N) for the fragment reads
  using TR = TT<T>;
  constexpr int BK = TR::BK, EPC = TR::EPC, KSTEPS = TR::KSTEPS;
  constexpr int BN = HALO_BN, NW = HALO_NW, WM = 4, WN = 2;
  constexpr int MI = BM / (WM * 32), NI = BN / (WN * 32);
  constexpr int B_SLOTS = BN / 8 / NW;  // weight LDS-DMA instructions per wave per tap
  constexpr int B_BYTES = BN * 128;
  constexpr int APT = 1;                // halo pieces per wave per tap
  constexpr int A_SLOTS = (10 - NBST) * APT;  // taps 0 .. 9-NBST issue APT halo pieces per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, l31 = lane & 31;

  const int W2 = p.W + 2;
  const int VR = p.H * W2;                     // virtual output rows per image
  const int TPI = (VR + BM - 1) / BM;          // m-tiles per image
  const int HRp = (BM + 2 * W2 + 2 + 7) & ~7;  // halo rows (padded to whole 8-row LDS-DMA pieces)
  const int NP = HRp >> 3;
  const int A_BYTES = HRp * 128;
  const int PR_MAX = (p.H + 2) * W2 - 1;       // last pixel of one padded plane
  const int B = p.M / (p.H * p.W);

  int bz, bx, by;
  tile_block_map(p.xcd_remap, B * TPI, (p.N + BN - 1) / BN, bz, bx, by);
  const int img = bx / TPI, v0 = (bx - img * TPI) * BM;
  const int n0 = by * BN;

  const T* __restrict__ Aimg = reinterpret_cast<const T*>(p.A0) + (int64_t)img * (p.H + 2) * W2 * p.Kc;
  const T* __restrict__ Wp = reinterpret_cast<const T*>(p.Wp);
  int aoff[A_SLOTS], boff[B_SLOTS];
  K22_PIECE_OFFSETS(aoff, A_SLOTS, wave, NW, v0, NP, 8)
  K22_ROW_OFFSETS(boff, B_SLOTS, wave, NW, n0, p.Npad - 1, n * 9 * p.Kc)
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
  // fragment rows: A row = wm*(BM/4) + mi*32 + l31 + tap shift ; B row = wn*(BN/2) + ni*32 + l31
  const int abase = wm * (BM / WM) + l31;
  int brow[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) brow[ni] = (wn * (BN / WN) + ni * 32 + l31) * 128;
  const int bsw = (l31 >> 1) & 7;  // (row >> 1) & 7 with row = multiple of 32 + l31
  const unsigned lds0 = halo_lds_base(smem);
#define K22_HALO_BODY                                                                                      \
  if constexpr (PIPE) K22_TAP_PIPE(FragA<T>, Frag<T>, arow[mi], asw[mi], Bcur + brow[ni], bsw, K22_PIPE_LOCKSTEP) \
  else { K22_TAP_PLAIN(FragA<T>, Frag<T>, ld_frag_at, arow[mi], asw[mi], Bcur + brow[ni], bsw) }
  K22_LOCKSTEP_LOOP(9, A_SLOTS, APT, K22_HALO_BODY)
#undef K22_HALO_BODY
  if constexpr (PIPE) { K22_MMA_ALL(pb, pa) }
  halo_tail<T, BM>(p, acc, smem, bx, bz, img, v0, n0);
}

// ================================================================================================================
// conv3_halo3_kernel: the same LDS-resident halo scheme on 64-BYTE rows.  The K loop walks HALF slabs (32 bf16 / 16 fp32
// channels); one iteration = the three taps of one filter row (ky) of one half slab = 24 MFMAs per wave between
// barriers (16 before), its weight tiles (3 x 128 rows x 64 B = 24 KB) sit in an RB-deep ring (RB-1 iterations in
// flight: 1-3 us of prefetch even where the weights stream from HBM) and the halo buffers shrink to half
// (2 x 29 KB at 96x96 instead of 2 x 57 KB), which is what makes room for the deeper ring at the wide levels.
//   per wave per iteration: <= 3 halo LDS-DMA pieces (16 rows x 64 B each, first two iterations of a half slab) + 3 weight
//   pieces, 24 ds_read_b128 (swizzle keyed on row >> 2: conflict-free for 64-byte rows), 24 MFMAs.
// ================================================================================================================
namespace {
__device__ __forceinline__ void ld_frag64(Frag<bf16_t>& f, const char* rowp, int sw, int ks, int h) {
  f.v = *reinterpret_cast<const u32x4_t*>(rowp + (((2 * ks + h) ^ sw) << 4));
}
__device__ __forceinline__ void ld_frag64(Frag<f16_t>& f, const char* rowp, int sw, int ks, int h) {
  f.v = *reinterpret_cast<const u32x4_t*>(rowp + (((2 * ks + h) ^ sw) << 4));
}
__device__ __forceinline__ void ld_frag64(Frag<float>& f, const char* rowp, int sw, int /*ks == 0*/, int h) {
  const float4 a = *reinterpret_cast<const float4*>(rowp + (((2 * h) ^ sw) << 4));
  const float4 b = *reinterpret_cast<const float4*>(rowp + (((2 * h + 1) ^ sw) << 4));
  f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w;
  f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
}
// loads a wave may leave in flight at the top of iteration KY (see the derivation next to K22_IT3 below)
template <int RB> constexpr int halo3_wait(int ky) { return RB == 2 ? 0 : (RB == 3 ? (ky == 0 ? 3 : 6) : (ky == 0 ? 6 : (ky == 1 ? 9 : 12))); }
constexpr int HALO3_ASLOTS = 6;   // halo LDS-DMA slots per wave per half slab (3 in each of its first two iterations)
}  // namespace

template <typename T, int BM, int RB>
__global__ __launch_bounds__(512) void conv3_halo3_kernel(const IgemmParams p) {
  constexpr int EPH = 64 / (int)sizeof(T);   // channels per 64-byte half-slab row
  constexpr int EPC = TT<T>::EPC;            // channels per 16-byte chunk
  constexpr int KS_U = EPH / 16;             // MFMA k-steps per tap of a half slab (2 bf16, 1 fp32)
  constexpr int BN = HALO_BN, NW = HALO_NW, WM = 4, WN = 2;
  constexpr int MI = BM / (WM * 32), NI = BN / (WN * 32);
  constexpr int BT_BYTES = 3 * BN * 64;      // weight tiles of one iteration (three taps)
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, l31 = lane & 31;

  const int W2 = p.W + 2;
  const int VR = p.H * W2;
  const int TPI = (VR + BM - 1) / BM;
  const int HR16 = (BM + 2 * W2 + 2 + 15) & ~15;   // halo rows, whole 16-row LDS-DMA pieces
  const int NPA = HR16 >> 4;
  const int A_BYTES = HR16 * 64;
  const int PR_MAX = (p.H + 2) * W2 - 1;
  const int B = p.M / (p.H * p.W);

  int bz, bx, by;
  tile_block_map(p.xcd_remap, B * TPI, (p.N + BN - 1) / BN, bz, bx, by);
  const int img = bx / TPI, v0 = (bx - img * TPI) * BM;
  const int n0 = by * BN;

  const T* __restrict__ Aimg = reinterpret_cast<const T*>(p.A0) + (int64_t)img * (p.H + 2) * W2 * p.Kc;
  const T* __restrict__ Wp = reinterpret_cast<const T*>(p.Wp);

  // loader geometry: a piece = 16 rows x 64 B; lane -> (row 16*piece + lane/4, position lane%4)
  int aoff[HALO3_ASLOTS];
  K22_PIECE_OFFSETS(aoff, HALO3_ASLOTS, wave, NW, v0, NPA, 16)
  int boff;
  {
    const int row = 16 * wave + (lane >> 2);
    int n = n0 + row;
    if (n > p.Npad - 1) n = p.Npad - 1;
    boff = n * 9 * p.Kc + ((lane & 3) ^ ((row >> 2) & 3)) * EPC;
  }
  int h0, h1;
  splitk_range(p.splitk, p.Kc / EPH, bz, h0, h1);

  f32x16_t acc[MI][NI];
  K22_ZERO_ACC(acc, MI, NI)

  char* const Bring = smem + 2 * A_BYTES;
  const int abase = wm * (BM / WM) + l31;
  int brow[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) brow[ni] = (wn * (BN / WN) + ni * 32 + l31) * 64;
  const int bsw = (l31 >> 2) & 3;

#define K22_ISSUE_A3(Q, HS, DST)                                                                           \
  {                                                                                                        \
    int j_ = (Q) * NW + wave;                                                                              \
    if (j_ > NPA - 1) j_ = NPA - 1;                                                                        \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Aimg + aoff[Q] + (HS) * EPH), \
                                     (__attribute__((address_space(3))) void*)((DST) + j_ * 1024), 16, 0, 0); \
  }
  // weight tiles of iteration (HS, KY): taps KY*3 + {0,1,2}; this wave's piece = rows [16*wave, +16) of each
#define K22_ISSUE_B3(HS, KY, SLOT)                                                                         \
  {                                                                                                        \
    const int kofs_ = (KY) * 3 * p.Kc + (HS) * EPH;                                                        \
    char* dst_ = Bring + (SLOT) * BT_BYTES + wave * 1024;                                                  \
    _Pragma("unroll") for (int kx = 0; kx < 3; ++kx)                                                       \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Wp + boff + kofs_ + kx * p.Kc), \
                                         (__attribute__((address_space(3))) void*)(dst_ + kx * BN * 64), 16, 0, 0); \
  }

  if (h0 < h1) {
    // prologue: the whole halo of the first half slab, then the weight tiles of iterations 0 .. RB-2
#pragma unroll
    for (int q = 0; q < HALO3_ASLOTS; ++q) K22_ISSUE_A3(q, h0, smem);
#pragma unroll
    for (int j = 0; j < RB - 1; ++j) {
      const int hs_ = h0 + j / 3 < h1 ? h0 + j / 3 : h1 - 1;
      K22_ISSUE_B3(hs_, j % 3, j);
    }
    int cur = 0, fill = RB - 1;
    for (int hs = h0; hs < h1; ++hs) {
      char* const Acur = smem + ((hs - h0) & 1) * A_BYTES;
      char* const Anext = smem + (((hs - h0) & 1) ^ 1) * A_BYTES;
      const int hn = hs + 1 < h1 ? hs + 1 : h1 - 1;   // past-the-end loads re-read the last half slab (uniform counting)
      // VMEM queue of a wave, per iteration: [3 halo pieces (KY < 2)] then [3 weight pieces of iteration it+RB-1].
      // At the top of iteration KY the weight tiles issued RB-1 iterations ago must have landed, and at KY == 0 also the
      // halo issued in the previous half slab's iterations 0 and 1; everything younger may stay in flight:
      //   RB = 2: 0 / 0 / 0     RB = 3: 3 / 6 / 6     RB = 4: 6 (halo!) / 9 / 12        (KY = 0 / 1 / 2)
#define K22_IT3(KY)                                                                                        \
      {                                                                                                    \
        wait_vmcnt<halo3_wait<RB>(KY)>();                                                                  \
        raw_barrier();                                                                      \
        if constexpr ((KY) < 2) {                                                                          \
          K22_ISSUE_A3(3 * ((KY) < 2 ? (KY) : 0) + 0, hn, Anext);                                          \
          K22_ISSUE_A3(3 * ((KY) < 2 ? (KY) : 0) + 1, hn, Anext);                                          \
          K22_ISSUE_A3(3 * ((KY) < 2 ? (KY) : 0) + 2, hn, Anext);                                          \
        }                                                                                                  \
        {                                                                                                  \
          constexpr int kya_ = ((KY) + RB - 1) % 3;                                                        \
          int hsa_ = hs + ((KY) + RB - 1) / 3;                                                             \
          if (hsa_ > h1 - 1) hsa_ = h1 - 1;                                                                \
          K22_ISSUE_B3(hsa_, kya_, fill);                                                                  \
        }                                                                                                  \
        const char* Bcur = Bring + cur * BT_BYTES;                                                         \
        _Pragma("unroll") for (int kx = 0; kx < 3; ++kx) {                                                 \
          const int shift = (KY) * W2 + kx;                                                                \
          const char* arow[MI];                                                                            \
          int asw[MI];                                                                                     \
          _Pragma("unroll") for (int mi = 0; mi < MI; ++mi) {                                              \
            const int ar = abase + mi * 32 + shift;                                                        \
            arow[mi] = Acur + ar * 64;                                                                     \
            asw[mi] = (ar >> 2) & 3;                                                                       \
          }                                                                                                \
          _Pragma("unroll") for (int ks = 0; ks < KS_U; ++ks) {                                            \
            Frag<T> a[MI], b[NI];                                                                          \
            _Pragma("unroll") for (int mi = 0; mi < MI; ++mi) ld_frag64(a[mi], arow[mi], asw[mi], ks, h);  \
            _Pragma("unroll") for (int ni = 0; ni < NI; ++ni) ld_frag64(b[ni], Bcur + kx * BN * 64 + brow[ni], bsw, ks, h); \
            _Pragma("unroll") for (int mi = 0; mi < MI; ++mi)                                              \
              _Pragma("unroll") for (int ni = 0; ni < NI; ++ni) mma_atom(acc[mi][ni], b[ni], a[mi]);       \
          }                                                                                                \
        }                                                                                                  \
        cur = (cur + 1 == RB) ? 0 : cur + 1;                                                               \
        fill = (fill + 1 == RB) ? 0 : fill + 1;                                                            \
      }
      K22_IT3(0) K22_IT3(1) K22_IT3(2)
#undef K22_IT3
    }
  }
#undef K22_ISSUE_A3
#undef K22_ISSUE_B3
  halo_tail<T, BM>(p, acc, smem, bx, bz, img, v0, n0);
}

// ---- host side ---------------------------------------------------------------------------------
static int halo3_rows(const IgemmParams& p, int bm) { return (bm + 2 * (p.W + 2) + 2 + 15) & ~15; }
static size_t halo3_smem_bytes(const IgemmParams& p, int bm, int rb) {
  return halo_lds_budget(bm, p.S0 != nullptr, (size_t)2 * halo3_rows(p, bm) * 64 + (size_t)rb * 3 * HALO_BN * 64);
}
static int halo3_pick_rb(const IgemmParams& p, int bm) {
  if (halo3_rows(p, bm) / 16 > HALO3_ASLOTS * HALO_NW) return 0;
  for (int rb : {4, 3, 2})
    if (halo3_smem_bytes(p, bm, rb) <= 160 * 1024) return rb;
  return 0;
}

int conv3_halo_ring(const IgemmParams& p, int bm) { return p.algo == IG_ALGO_HALO3 ? halo3_pick_rb(p, bm) : halo_pick_nbst(p, bm); }

bool conv3_halo_supported(const IgemmParams& p, int dtype, int bm) {
  const int BK = k22_bk(dtype);
  if (p.taps != 9 || (bm != 256 && bm != 128 && bm != HALO_BM_STRIP)) return false;
  // the 224-row tile: conv3_halo_spec_kernel's pipelined form in the 16-bit types
  if (bm == HALO_BM_STRIP && (p.algo != IG_ALGO_SPEC_PIPE || k22_esz(dtype) != 2)) return false;
  // split precision: the input is read in x3 chunks; instantiated forms = the lock-step kernel with asm LDS-DMA (algo 2 / 6 / 7 all
  // run it) and the specialised kernel (11 / 12)
  if (k22_is_split(dtype) && (p.a_raw || p.algo == IG_ALGO_HALO3)) return false;
  if (p.out_mode != IG_OUT_ROWMAJOR && p.out_mode != IG_OUT_ROWMAJOR_F32) return false;
  if (p.N % 8 || p.ldo % 8 || (p.residual && p.ldr % 8) || p.Kc % BK) return false;
  if (p.H <= 0 || p.W <= 0 || p.M % (p.H * p.W)) return false;
  if (p.S0 != nullptr) {
    if (!p.Ws || p.SK0 % BK || p.SK1 % BK || (p.SK1 > 0 && !p.S1) || p.SK0 <= 0) return false;
    if ((int64_t)p.M * (p.SK0 > p.SK1 ? p.SK0 : p.SK1) >= (1ll << 31) || (int64_t)p.Npad * (p.SK0 + p.SK1) >= (1ll << 31)) return false;
  }
  if (conv3_halo_ring(p, bm) == 0) return false;
  if ((int64_t)(p.H + 2) * (p.W + 2) * p.Kc >= (1ll << 31) || (int64_t)p.Npad * 9 * p.Kc >= (1ll << 31)) return false;
  return true;
}

int conv3_halo_tiles_per_image(const IgemmParams& p, int bm) { return halo_tiles_per_image(p, bm); }
size_t conv3_halo_lds_bytes(const IgemmParams& p, int bm, int depth) { return p.algo == IG_ALGO_HALO3 ? halo3_smem_bytes(p, bm, depth) : halo_smem_bytes(p, bm, depth); }

// conv3_halo_kernel in form MODE at (L.bm, L.depth)
template <typename T, int MODE>
static int launch_halo_mode(const IgemmParams& p, const IgemmLaunch& L, hipStream_t stream) {
  return halo_with_bm(L.bm, [&](auto bm) {
    return halo_with_depth<2, 3, 4, 6>(L.depth, [&](auto d) { return halo_run<conv3_halo_kernel<T, decltype(bm)::value, decltype(d)::value, MODE>>(p, L, stream); });
  });
}

// Launches the lock-step kernel the resolved launch names (the split-K reduction, if any, is the caller's: launch_igemm): conv3_halo3_kernel, or
// conv3_halo_kernel in form L.pipe = MODE (0 compiler-issued LDS-DMA, 1 asm LDS-DMA + explicit fragment pipeline, 2 asm LDS-DMA).  The split
// types have MODE 2 only.  (Two wave groups in opposite phases and loader-wave specialisation measured 12-20 % / 2-5 % slower in round 1, were
// never tuner candidates, and were deleted in round 5.)
int launch_conv3_halo(const IgemmParams& p, int dtype, const IgemmLaunch& L, hipStream_t stream) {
  return k22_with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if constexpr (!is_x3<T>::value) {
      if (L.family == IG_FAM_HALO3)
        return halo_with_bm(L.bm, [&](auto bm) {
          return halo_with_depth<2, 3, 4>(L.depth, [&](auto d) { return halo_run<conv3_halo3_kernel<T, decltype(bm)::value, decltype(d)::value>>(p, L, stream); });
        });
      if (L.pipe == 0) return launch_halo_mode<T, 0>(p, L, stream);
      if (L.pipe == 1) return launch_halo_mode<T, 1>(p, L, stream);
    }
    return launch_halo_mode<T, 2>(p, L, stream);
  });
}
