// k22 — implicit-GEMM MFMA kernel: 3x3 convolution (zero-bordered NHWC input) and plain GEMM
// (1x1 conv, qkv / proj / linear) through ONE kernel body.
//
// Replaces, on the reference hot path: nn.Conv2d 3x3 (unet.py:152,180,188,426,562), Conv2d 1x1
// skip (unet.py:191), Conv1d k=1 qkv/encoder_kv/proj_out (unet.py:251,257,258) and nn.Linear.
//
// Structure (per 256-thread workgroup = 4 waves as 2(M) x 2(N)):
//   * block tile BM x BN, K tile = one 128-byte row per operand row (64 bf16 / 32 fp32), never
//     straddling a filter tap (Cin % 64 == 0), so a conv K tile is a contiguous channel slice of
//     one shifted pixel: address = pixel_base[m] + tap_offset + c0   (no bounds checks: the
//     producer wrote a zero border).
//   * operands go HBM/L2 -> LDS directly (global_load_lds_dwordx4: no staging VGPRs, no ds_write
//     pass), STAGES buffers deep with a COUNTED vmcnt so STAGES-2 tiles stay in flight across the
//     single raw s_barrier of each K tile:
//       iteration k:  s_waitcnt vmcnt((STAGES-2)*CH)  -> this wave's part of tile k has landed
//                     s_barrier                        -> everybody's part landed; tile k-1's buffer is free
//                     issue tile k+STAGES-1 into that buffer ; MFMAs on tile k
//   * the LDS image of one wave-instruction is lane-linear (base + lane*16 B): 8 rows x 128 B, so
//     the chunk-XOR swizzle (common.h) is applied to the per-lane SOURCE address and to the reads;
//     fragment ds_read_b128s are bank-conflict free.
//   * the MFMA is issued "transposed" (weights as the A operand, pixels as B): the 32x32 C tile then
//     has one PIXEL per lane column and 4 consecutive OUTPUT CHANNELS in consecutive accumulator
//     registers, so the epilogue moves 8 B (bf16) / 16 B (fp32) per store instead of one element.
//   * workgroups are renumbered so that the blocks an XCD runs concurrently share operand panels in
//     that XCD's L2 (hardware places block b on XCD b % 8): every weight byte is pulled from
//     HBM/Infinity-Fabric by one XCD, pixels by the few XCDs that hold their m-tile group.
//   * fp32 accumulate; epilogue fuses bias, residual add and activation, or writes fp32 split-K
//     partials that splitk_reduce_kernel finishes.  The epilogue arithmetic of the kernel and of the two finishes is one text (K22_EPI_*
//     below); block map, split-K range, row vectors and the counted vmcnt wait are common.h's, the q/k/v scatter kernels.h's.
#include "kernels.h"
#include <stdlib.h>
#include <type_traits>

// ---- the epilogue arithmetic of igemm_kernel and the two split-K finishes, once --------------------------------------------------------
// Macros, not functions: through function templates the same text moved the code of every kernel of this file (block order, branch
// polarity; profiles/shared_helpers_device_code.txt).  Names they take from the kernel: T, p, res (p.residual as const T*).
// V[0..3] = channels COL .. COL + 3 of row ROW: + bias (+ bias2 under BIAS2: the finishes only - igemm_resolve refuses a fused skip on the generic
// kernel) + residual (T, or fp32 under p.res_f32), then the activation
#define K22_EPI_FINISH4(BIAS2, V, ROW, COL)                                                                \
  {                                                                                                        \
    if (p.bias != nullptr) {                                                                               \
      const float4 bv = *reinterpret_cast<const float4*>(p.bias + (COL));                                  \
      V[0] += bv.x; V[1] += bv.y; V[2] += bv.z; V[3] += bv.w;                                              \
    }                                                                                                      \
    if constexpr (BIAS2) {                                                                                 \
      if (p.bias2 != nullptr) {                                                                            \
        const float4 bv = *reinterpret_cast<const float4*>(p.bias2 + (COL));                               \
        V[0] += bv.x; V[1] += bv.y; V[2] += bv.z; V[3] += bv.w;                                            \
      }                                                                                                    \
    }                                                                                                      \
    if (res != nullptr) {                                                                                  \
      float rv[4];                                                                                         \
      if (p.res_f32) load_row_f32<float, 4>(reinterpret_cast<const float*>(p.residual) + (int64_t)(ROW) * p.ldr + (COL), rv); \
      else load_row_f32<T, 4>(res + (int64_t)(ROW) * p.ldr + (COL), rv);                                   \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) V[e] += rv[e];                                         \
    }                                                                                                      \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) V[e] = apply_act(V[e], p.act);                           \
  }
// the same four values to where p.out_mode puts them: row-major T, row-major fp32 or the q/k/v scatter - or else (IG_OUT_NCHW_F32) the
// statement that follows, which each kernel spells from the index arithmetic it already has
#define K22_EPI_STORE4_OR_ELSE(V, ROW, COL)                                                                \
  if (p.out_mode == IG_OUT_ROWMAJOR) {                                                                     \
    store_row<T, 4>(reinterpret_cast<T*>(p.out) + (int64_t)(ROW) * p.ldo + (COL), V);                      \
  } else if (p.out_mode == IG_OUT_ROWMAJOR_F32) {                                                          \
    store_row<float, 4>(reinterpret_cast<float*>(p.out) + (int64_t)(ROW) * p.ldo + (COL), V);              \
  } else if (p.out_mode == IG_OUT_QKV) {                                                                   \
    K22_QKV_SCATTER(T, 4, V, ROW, (ROW) / p.att_T, (ROW) - img_ * p.att_T, COL)                            \
  } else
// one element U at (ROW, COL) (the ragged tails: N, ldo or ldr not a multiple of 4; no q/k/v mode there), NCHW as above
#define K22_EPI_FINISH1(BIAS2, U, ROW, COL)                                                                \
  {                                                                                                        \
    if (p.bias != nullptr) U += p.bias[COL];                                                               \
    if constexpr (BIAS2) {                                                                                 \
      if (p.bias2 != nullptr) U += p.bias2[COL];                                                           \
    }                                                                                                      \
    if (res != nullptr) U += p.res_f32 ? reinterpret_cast<const float*>(p.residual)[(int64_t)(ROW) * p.ldr + COL] : to_f32(res[(int64_t)(ROW) * p.ldr + COL]); \
    U = apply_act(U, p.act);                                                                               \
  }
#define K22_EPI_STORE1_OR_ELSE(U, ROW, COL)                                                                \
  if (p.out_mode == IG_OUT_ROWMAJOR) {                                                                     \
    reinterpret_cast<T*>(p.out)[(int64_t)(ROW) * p.ldo + COL] = from_f32<T>(U);                            \
  } else if (p.out_mode == IG_OUT_ROWMAJOR_F32) {                                                          \
    reinterpret_cast<float*>(p.out)[(int64_t)(ROW) * p.ldo + COL] = U;                                     \
  } else

// ARAW (K22_F16X3 only): the A operand is plain fp32 rows, split into fp16 halves while its fragments are read (p.a_raw).
template <typename T, int BM, int BN, int STAGES, bool ARAW = false>
__global__ __launch_bounds__(256) void igemm_kernel(const IgemmParams p) {
  using TR = TT<T>;
  constexpr int BK = TR::BK, EPC = TR::EPC, KSTEPS = TR::KSTEPS;
  constexpr int MI = BM / 64, NI = BN / 64;     // 32x32 atoms per wave along M / N
  constexpr int A_CH = BM / 32, B_CH = BN / 32, CH = A_CH + B_CH;  // LDS-DMA instructions per wave per K tile
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, BUF = A_BYTES + B_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  int bz, bx, by;
  tile_block_map(p.xcd_remap, (p.M + BM - 1) / BM, (p.N + BN - 1) / BN, bz, bx, by);
  const int m0 = bx * BM, n0 = by * BN;

  const bool conv = (p.taps == 9);
  const T* __restrict__ A0 = reinterpret_cast<const T*>(p.A0);
  const T* __restrict__ A1 = reinterpret_cast<const T*>(p.A1);
  const T* __restrict__ Wp = reinterpret_cast<const T*>(p.Wp);

  // ---- loader geometry: thread -> (row = tid/8 + 32*i, physical chunk = tid%8) --------------
  const int lrow = tid >> 3, lpos = tid & 7;
  const int lchunk = lpos ^ ((lrow >> 1) & 7);  // logical (source) chunk that lands at this position
  int64_t aoff0[A_CH], aoff1[A_CH], boff[B_CH];
  const int ldb = p.taps * p.Kc;
#pragma unroll
  for (int i = 0; i < A_CH; ++i) {
    int m = m0 + lrow + 32 * i;
    if (m > p.M - 1) m = p.M - 1;
    if (conv) {
      const int hw = p.H * p.W;
      const int b = m / hw, rem = m - b * hw;
      const int y = rem / p.W, x = rem - y * p.W;
      aoff0[i] = ((int64_t)(b * (p.H + 2) + y) * (p.W + 2) + x) * p.Kc;
      aoff1[i] = 0;
    } else {
      aoff0[i] = (int64_t)m * p.lda0;
      aoff1[i] = (int64_t)m * p.lda1;
    }
  }
#pragma unroll
  for (int i = 0; i < B_CH; ++i) {
    int n = n0 + lrow + 32 * i;
    if (n > p.Npad - 1) n = p.Npad - 1;
    boff[i] = (int64_t)n * ldb;
  }
  const int kt_per_tap = p.Kc / BK;
  const int nkt = p.taps * kt_per_tap;
  int kt0, kt1;
  splitk_range(p.splitk, nkt, bz, kt0, kt1);

  f32x16_t acc[MI][NI];
  K22_ZERO_ACC(acc, MI, NI)
  const int h = lane >> 5, l31 = lane & 31;
  const int64_t lck = lchunk * EPC;
  const int wave_row0 = wave * 8;  // rows [8*wave + 32*i, +8) of a tile are filled by this wave's i-th DMA

#define K22_ISSUE(KT, BUFI)                                                                              \
  {                                                                                                      \
    int kt_ = (KT);                                                                                      \
    if (kt_ > kt1 - 1) kt_ = kt1 - 1; /* past-the-end slots re-read the last tile: uniform vmcnt counting */ \
    const int tap_ = kt_ / kt_per_tap;                                                                   \
    const int k0_ = (kt_ - tap_ * kt_per_tap) * BK;                                                      \
    const bool second_ = (!conv) && (k0_ >= p.K0);                                                       \
    const T* src_ = second_ ? A1 : A0;                                                                   \
    const int ty_ = tap_ / 3, tx_ = tap_ - ty_ * 3;                                                      \
    const int64_t add_ = (conv ? (int64_t)(ty_ * (p.W + 2) + tx_) * p.Kc + k0_ : (int64_t)(second_ ? k0_ - p.K0 : k0_)) + lck; \
    char* As_ = smem + (BUFI) * BUF + wave_row0 * 128;                                                   \
    _Pragma("unroll") for (int i = 0; i < A_CH; ++i)                                                     \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src_ + (second_ ? aoff1[i] : aoff0[i]) + add_), \
                                         (__attribute__((address_space(3))) void*)(As_ + i * 4096), 16, 0, 0); \
    const int64_t badd_ = (int64_t)tap_ * p.Kc + k0_ + lck;                                              \
    char* Bs_ = As_ + A_BYTES;                                                                           \
    _Pragma("unroll") for (int i = 0; i < B_CH; ++i)                                                     \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Wp + boff[i] + badd_), \
                                         (__attribute__((address_space(3))) void*)(Bs_ + i * 4096), 16, 0, 0); \
  }

  if (kt0 < kt1) {
#pragma unroll
    for (int s_ = 0; s_ < STAGES - 1; ++s_) K22_ISSUE(kt0 + s_, s_);
    int cur = 0, fill = STAGES - 1;
    for (int kt = kt0; kt < kt1; ++kt) {
      wait_vmcnt<(STAGES - 2) * CH>();
      raw_barrier();
      K22_ISSUE(kt + STAGES - 1, fill);
      {
        const char* As = smem + cur * BUF;
        const char* Bs = As + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
          FragA<T> a[MI];
          Frag<T> b[NI];
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) ld_frag_a<ARAW, T>(a[mi], As, wm * (BM / 2) + mi * 32 + l31, ks, h);
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) ld_frag(b[ni], Bs, wn * (BN / 2) + ni * 32 + l31, ks, h);
#pragma unroll
          for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) mma_atom(acc[mi][ni], b[ni], a[mi]);  // C^T: rows = n, cols = m
        }
      }
      cur = (cur + 1 == STAGES) ? 0 : cur + 1;
      fill = (fill + 1 == STAGES) ? 0 : fill + 1;
    }
    wait_vmcnt<0>();  // drain the redundant tail DMAs before the LDS is released
  }
#undef K22_ISSUE

  // ---- epilogue: lane = pixel m, registers 4j..4j+3 = channels n0 + 8j + 4h + {0..3} -----------------
  const int mbase = m0 + wm * (BM / 2), nbase = n0 + wn * (BN / 2);
  const bool vec_ok = ((p.N & 3) == 0) && ((p.ldo & 3) == 0) && ((p.ldr & 3) == 0);
  const T* __restrict__ res = reinterpret_cast<const T*>(p.residual);
  float* part = p.splitk > 1 ? p.partial + (int64_t)bz * p.M * p.N : nullptr;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int m = mbase + mi * 32 + l31;
    if (m >= p.M) continue;
    int64_t nchw_base = 0;
    if (p.out_mode == IG_OUT_NCHW_F32) {
      const int hw = p.H * p.W;
      const int b = m / hw, rem = m - b * hw;
      nchw_base = (int64_t)b * p.N * hw + rem;
    }
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = nbase + ni * 32 + 8 * j + 4 * h;
        if (n >= p.N) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc_unscale<T>(acc[mi][ni][4 * j + e]);
        if (part != nullptr) {
          if (vec_ok) {
            *reinterpret_cast<float4*>(part + (int64_t)m * p.N + n) = make_float4(v[0], v[1], v[2], v[3]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (n + e < p.N) part[(int64_t)m * p.N + n + e] = v[e];
          }
          continue;
        }
        if (vec_ok) {
          K22_EPI_FINISH4(false, v, m, n)
          K22_EPI_STORE4_OR_ELSE(v, m, n) {
            const int64_t hw = (int64_t)p.H * p.W;
#pragma unroll
            for (int e = 0; e < 4; ++e) reinterpret_cast<float*>(p.out)[nchw_base + (int64_t)(n + e) * hw] = v[e];
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (n + e >= p.N) continue;
            float u = v[e];
            K22_EPI_FINISH1(false, u, m, n + e)
            K22_EPI_STORE1_OR_ELSE(u, m, n + e) reinterpret_cast<float*>(p.out)[nchw_base + (int64_t)(n + e) * p.H * p.W] = u;
          }
        }
      }
  }
}

// Finishes a split-K launch: out = act(sum_s partial[s] + bias + residual).  4 channels per thread.
template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const IgemmParams p) {
  const int64_t total = (int64_t)p.M * p.N;
  const T* __restrict__ res = reinterpret_cast<const T*>(p.residual);
  if (((p.N & 3) == 0) && ((p.ldo & 3) == 0) && ((p.ldr & 3) == 0)) {
    const int nq = p.N >> 2;
    const int64_t quads = total >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < quads; i += (int64_t)gridDim.x * blockDim.x) {
      const int m = (int)(i / nq), n = (int)(i - (int64_t)m * nq) * 4;
      float4 a = *reinterpret_cast<const float4*>(p.partial + i * 4);
      for (int s = 1; s < p.splitk; ++s) {
        const float4 b = *reinterpret_cast<const float4*>(p.partial + (int64_t)s * total + i * 4);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
      }
      float v[4] = {a.x, a.y, a.z, a.w};
      K22_EPI_FINISH4(true, v, m, n)
      K22_EPI_STORE4_OR_ELSE(v, m, n) {
        const int hw = p.H * p.W;
        const int b = m / hw, rem = m - b * hw;
#pragma unroll
        for (int e = 0; e < 4; ++e) reinterpret_cast<float*>(p.out)[((int64_t)b * p.N + n + e) * hw + rem] = v[e];
      }
    }
    return;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int m = (int)(i / p.N), n = (int)(i - (int64_t)m * p.N);
    float v = 0.f;
    for (int s = 0; s < p.splitk; ++s) v += p.partial[(int64_t)s * total + i];
    K22_EPI_FINISH1(true, v, m, n)
    K22_EPI_STORE1_OR_ELSE(v, m, n) {
      const int hw = p.H * p.W;
      const int b = m / hw, rem = m - b * hw;
      reinterpret_cast<float*>(p.out)[((int64_t)b * p.N + n) * hw + rem] = v;
    }
  }
}

// Split-K finish + GroupNorm partial sums.  Workgroup = 16 consecutive output rows (never straddling an image:
// HW % 16 == 0) x 64 channels; thread = one row x 4 consecutive channels, so the splitk partial loads of a thread
// are independent and the grid is (M/16) x (N/64) workgroups.  stats[row_block][n] = (sum, sumsq) of the
// stored values, reduced over the 16 rows in a fixed order through LDS.
template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_rows_kernel(const IgemmParams p) {
  __shared__ float red[16][64][2];
  const int64_t total = (int64_t)p.M * p.N;
  const T* __restrict__ res = reinterpret_cast<const T*>(p.residual);
  const int r = threadIdx.x >> 4, cq = threadIdx.x & 15;
  const int m = blockIdx.x * 16 + r, n = blockIdx.y * 64 + cq * 4;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  const bool ok = m < p.M && n < p.N;
  if (ok) {
    const int64_t i = (int64_t)m * p.N + n;
    float4 a = *reinterpret_cast<const float4*>(p.partial + i);
#pragma unroll 4
    for (int s = 1; s < p.splitk; ++s) {
      const float4 b = *reinterpret_cast<const float4*>(p.partial + (int64_t)s * total + i);
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    K22_EPI_FINISH4(true, v, m, n)
    if (p.out_mode == IG_OUT_ROWMAJOR) {
      store_row<T, 4>(reinterpret_cast<T*>(p.out) + (int64_t)m * p.ldo + n, v);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = to_f32(from_f32<T>(v[e]));
    } else {
      store_row<float, 4>(reinterpret_cast<float*>(p.out) + (int64_t)m * p.ldo + n, v);
    }
  }
  if (p.stats == nullptr) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[r][cq * 4 + e][0] = ok ? v[e] : 0.f;
    red[r][cq * 4 + e][1] = ok ? v[e] * v[e] : 0.f;
  }
  __syncthreads();
  if (threadIdx.x < 128) {
    const int ch = threadIdx.x >> 1, which = threadIdx.x & 1;
    float a = 0.f;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) a += red[rr][ch][which];
    const int nn = blockIdx.y * 64 + ch;
    if (nn < p.N) p.stats[((int64_t)blockIdx.x * p.N + nn) * 2 + which] = a;
  }
}

// ---- host side ------------------------------------------------------------------------
static IgemmOptions g_opts;
void igemm_set_default_stages(int v) { g_opts.stages = (v >= 2 && v <= 4) ? v : -1; }
void igemm_set_xcd_remap(int v) { g_opts.xcd_remap = v ? 1 : 0; }
void igemm_set_gemm_algo(int v) { g_opts.gemm_algo = (v == IG_ALGO_GEMM8 || v == IG_ALGO_STREAM) ? v : 0; }
void igemm_set_conv_algo(int v) {
  const bool ok = v == IG_ALGO_GENERIC || v == IG_ALGO_STREAM || v == IG_ALGO_UP2 || v == IG_ALGO_UP2_PIPE || igemm_algo_is_halo(v);
  g_opts.conv_algo = ok ? v : 0;
}

// Can the split-K finish run row-tiled (splitk_reduce_rows_kernel: 16 rows of one image per workgroup, GroupNorm sums on request)?  3x3
// convolutions always finish that way; plain GEMMs only when they owe GroupNorm sums.
static bool reduce_rows_ok(const IgemmParams& p, bool stats) {
  const int hw = p.taps == 4 ? 4 * p.H * p.W : ((p.taps == 9 || stats) ? p.H * p.W : 0);   // output rows per image
  return hw > 0 && hw % 16 == 0 && (p.N & 3) == 0 && (p.ldo & 3) == 0 && (p.ldr & 3) == 0 &&
         (p.out_mode == IG_OUT_ROWMAJOR || p.out_mode == IG_OUT_ROWMAJOR_F32);
}

int igemm_resolve(const IgemmParams& p, int dtype, IgemmLaunch* out) {
  const IgemmOptions o = g_opts;
  if (dtype < K22_BF16 || dtype > K22_F16X2) return k22_set_error(K22_EINVAL, "igemm: bad dtype");
  const int BK = k22_bk(dtype);
  const int nkt = p.taps * (p.Kc / BK);
  const bool qkv = p.out_mode == IG_OUT_QKV;
  IgemmLaunch L = {};
  L.xcd_remap = o.xcd_remap;
  L.block = 512;
  // ring depth asked for on the 8-wave kernels: the problem's, else the "igemm_stages" option
  const int want = (p.stages < 2 && o.stages >= 0) ? o.stages : p.stages;
  auto blocks = [&](int bm, int bn) { return ((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn); };
  // ---- weight-streaming small-M kernel (stream_gemm.hip): the tuner's candidate or the conv_algo / gemm_algo option -----------
  if (p.taps != 4 && (p.algo == IG_ALGO_STREAM || (p.algo == IG_ALGO_AUTO && (p.taps == 9 ? o.conv_algo : o.gemm_algo) == IG_ALGO_STREAM))) {
    const int mb = p.force_bm == 288 ? 9 : 5;
    if (stream_supported(p, dtype, mb)) {
      L.family = IG_FAM_STREAM; L.algo = IG_ALGO_STREAM; L.bm = mb * 32; L.bn = 64;
      const int nslab = p.Kc / 64, nb = stream_mtiles(p, mb);
      L.splitk = p.splitk > 0 ? p.splitk : (nb >= 240 ? 1 : 240 / nb);
      if (L.splitk > nslab) L.splitk = nslab;
      if (L.splitk < 1) L.splitk = 1;
      L.block = 256; L.grid = (unsigned)nb; L.lds = stream_lds_bytes(p, mb);
    }
  }
  // ---- upsample + 3x3 convolution in its four-phase form (conv3_up2.hip): one kernel; tile and split from a fixed rule ---------------------
  if (p.taps == 4) {
    const bool up2_opt = o.conv_algo == IG_ALGO_UP2 || o.conv_algo == IG_ALGO_UP2_PIPE;   // ("conv_algo" option: the A/B of the two forms)
    const int algo = p.algo != IG_ALGO_AUTO ? p.algo : (up2_opt ? o.conv_algo : IG_ALGO_AUTO);
    if (algo != IG_ALGO_AUTO && algo != IG_ALGO_UP2 && algo != IG_ALGO_UP2_PIPE)
      return k22_set_error(K22_EINVAL, "igemm: the four-phase upsampling convolution runs conv3_up2_kernel only (algo 0 / 30 / 31)");
    // The rule, from the measurements in profiles/up2_phase_ab.txt (bf16, C2's three up-block shapes): 256-row tiles wherever they fit - also
    // where an image fills only part of one (12x12: half as many workgroups re-read each weight tile) - and a 2-way slab split where the
    // four phases alone give fewer than 128 workgroups (12x12 at B = 2: 96); no deeper split: its partial round trip costs more than it hides.
    int bm = p.force_bm;
    if (bm == 0) bm = conv3_up2_supported(p, dtype, 256) ? 256 : 128;
    if ((bm != 256 && bm != 128) || !conv3_up2_supported(p, dtype, bm))
      return k22_set_error(K22_EINVAL, "igemm: this four-phase upsampling convolution is not supported (tile 256 / 128, N % 8, Kc % BK, LDS)");
    L.family = IG_FAM_UP2; L.bm = bm; L.bn = 128;
    L.pipe = (k22_esz(dtype) == 2 && algo != IG_ALGO_UP2) ? 1 : 0;
    L.algo = L.pipe ? IG_ALGO_UP2_PIPE : IG_ALGO_UP2;
    const int nslab = p.Kc / BK;
    const int nb = (p.M / (4 * p.H * p.W)) * conv3_up2_tiles_per_image(p, bm) * ((p.N + 127) / 128) * 4;
    L.splitk = p.splitk > 0 ? p.splitk : ((nb < 128 && nslab >= 4) ? 2 : 1);
    if (L.splitk > nslab) L.splitk = nslab;
    if (L.splitk < 1) L.splitk = 1;
    L.grid = (unsigned)nb;
    L.depth = conv3_up2_ring(p, bm);
    if (want >= 2 && want < L.depth) L.depth = 2;   // shallower ring on request (instantiated: 4, 2)
    L.lds = conv3_up2_lds_bytes(p, bm, L.depth);
  }
  // ---- 3x3 convolution: the LDS-resident halo kernels when they apply -----------------------------------------------------------
  const int conv_algo = (p.algo && p.algo != IG_ALGO_STREAM) ? p.algo : (o.conv_algo == IG_ALGO_STREAM ? 0 : o.conv_algo);
  if (!L.algo && p.taps == 9 && conv_algo != IG_ALGO_GENERIC && p.N >= 128 && !p.a_raw) {   // (the halo kernels read their input in x3 chunks only)
    IgemmParams ph = p;
    ph.algo = igemm_algo_is_halo(conv_algo) ? conv_algo : IG_ALGO_HALO;
    int bm = 0;
    if (p.force_bm == 256 || p.force_bm == 128 || p.force_bm == 224) {   // (224: the pipelined specialised kernel in the 16-bit types only)
      if (conv3_halo_supported(ph, dtype, p.force_bm) && (conv_algo >= IG_ALGO_HALO || p.force_bn == 0)) bm = p.force_bm;
    } else if (p.force_bm == 0) {
      if (conv3_halo_supported(ph, dtype, 256)) bm = 256;
      else if (conv3_halo_supported(ph, dtype, 128)) bm = 128;
    }
    if (bm) {
      L.algo = ph.algo; L.bm = bm; L.bn = 128;
      const int nslab = (p.Kc / BK) * (L.algo == IG_ALGO_HALO3 ? 2 : 1);   // split-K granularity: slabs / half slabs
      const int nb = (p.M / (p.H * p.W)) * conv3_halo_tiles_per_image(p, bm) * ((p.N + 127) / 128);
      if (p.splitk > 0) {
        L.splitk = p.splitk;
      } else {
        int sk = 1;
        while (nb * sk < 200 && sk < 16 && (p.Kc / BK) / (sk * 2) >= 2) sk *= 2;
        L.splitk = sk;
      }
      if (L.splitk > nslab) L.splitk = nslab;
      if (L.splitk < 1) L.splitk = 1;
      L.grid = (unsigned)nb;
      L.depth = conv3_halo_ring(ph, bm);
      if (want >= 2 && want < L.depth) L.depth = want == 5 ? 4 : want;   // shallower ring on request (instantiated: 2, 3, 4, 6; halo3: 2, 3, 4)
      const bool split = k22_is_split(dtype);
      if (L.algo == IG_ALGO_SPEC || L.algo == IG_ALGO_SPEC_PIPE) {
        // x3 and fp32 at BM = 256: two fragment sets of 8 registers per fragment do not fit beside 128 accumulators: compiler-scheduled consumers
        L.family = IG_FAM_SPEC;
        L.pipe = (L.algo == IG_ALGO_SPEC_PIPE && !(bm == 256 && (dtype == K22_F16X3 || dtype == K22_F32))) ? 1 : 0;
      } else if (split) {
        // split precision: one lock-step form (asm LDS-DMA) whichever of 2 / 6 / 7 was named
        L.family = IG_FAM_HALO; L.pipe = 2;
      } else if (L.algo == IG_ALGO_HALO3) {
        L.family = IG_FAM_HALO3;
      } else {
        L.family = IG_FAM_HALO;
        L.pipe = L.algo == IG_ALGO_HALO_PIPE ? 1 : (L.algo == IG_ALGO_HALO_ASM ? 2 : 0);
      }
      L.lds = conv3_halo_lds_bytes(ph, bm, L.depth);
    }
  }
  // ---- plain GEMM on the 8-wave frame (gemm8.hip): the tuner's candidate or the "gemm_algo" option -----------------------------
  if (!L.algo && p.taps == 1 && (p.algo == IG_ALGO_GEMM8 || (p.algo == IG_ALGO_AUTO && o.gemm_algo == IG_ALGO_GEMM8))) {
    const int hw = p.H > 0 ? p.H * p.W : p.M;
    int bm = 0;
    if (p.force_bm == 256 || p.force_bm == 128) { if (gemm8_supported(p, dtype, p.force_bm)) bm = p.force_bm; }
    else if (gemm8_supported(p, dtype, 256))
      bm = ((p.M / hw) * ((hw + 255) / 256) * ((p.N + 127) / 128) >= 400 || hw % 256 == 0) ? 256 : 128;
    if (bm) {
      L.algo = IG_ALGO_GEMM8; L.bm = bm; L.bn = 128;
      L.splitk = p.splitk > 0 ? p.splitk : 1;
      if (qkv) L.splitk = 1;
      if (L.splitk > p.Kc / BK) L.splitk = p.Kc / BK;
      L.grid = (unsigned)((p.M / hw) * gemm8_tiles_per_image(p, bm) * ((p.N + 127) / 128));
      // ring: 3 stages of 48 KB at BM = 256; at BM = 128 (32 KB per stage) 4 stages, or 2 = 68 KB with the epilogue tile, so that TWO workgroups
      // share a CU and one's prologue / epilogue overlaps the other's K loop (short-K GEMMs).  A request of 3 / 4 selects the specialised,
      // pipelined kernel where it exists (16-bit types; the split types keep the lock-step kernel), 4 = its two-per-CU form (BM = 128 only).
      if ((want == 3 || want == 4) && gemm8_spec_supported(dtype)) {
        L.family = IG_FAM_GEMM8_SPEC; L.pipe = 1;
        L.depth = (want == 4 && bm == 128) ? 2 : (bm == 256 ? 3 : 4);
      } else {
        L.family = IG_FAM_GEMM8;
        L.depth = bm == 256 ? 3 : (want == 2 ? 2 : 4);
        L.a_raw = (k22_is_split(dtype) && p.a_raw) ? 1 : 0;
      }
      L.lds = gemm8_lds_bytes(bm, L.depth);
    }
  }
  // ---- generic implicit GEMM (igemm_kernel) ---------------------------------------------------------------------------------------
  if (!L.algo) {
    L.family = IG_FAM_GENERIC; L.algo = IG_ALGO_GENERIC; L.block = 256;
    if (p.force_bm && p.force_bn) { L.bm = p.force_bm; L.bn = p.force_bn; }
    else if (p.N <= 64) { L.bm = (p.M >= 128) ? 128 : 64; L.bn = 64; }
    else if (blocks(128, 128) >= 160) { L.bm = 128; L.bn = 128; }
    else if (p.M > 64) { L.bm = 128; L.bn = 64; }
    else { L.bm = 64; L.bn = 64; }
    if ((L.bm != 128 && L.bm != 64) || (L.bn != 128 && L.bn != 64)) return k22_set_error(K22_EINVAL, "igemm: unsupported tile configuration");
    L.grid = (unsigned)blocks(L.bm, L.bn);
    if (p.splitk > 0) {
      L.splitk = p.splitk;
    } else {
      int sk = 1;
      while ((int)L.grid * sk < 200 && sk < 16 && nkt / (sk * 2) >= 6) sk *= 2;
      L.splitk = sk;
    }
    if (L.splitk > nkt) L.splitk = nkt > 0 ? nkt : 1;
    // LDS-DMA ring: the problem's request, else the option, else env K22_IGEMM_STAGES, else 2
    static const int env_stages = [] { const char* e = getenv("K22_IGEMM_STAGES"); const int v = e ? atoi(e) : 2; return (v < 2 || v > 4) ? 2 : v; }();
    L.depth = (p.stages >= 2 && p.stages <= 4) ? p.stages : (o.stages >= 0 ? o.stages : env_stages);
    L.a_raw = (k22_is_split(dtype) && p.a_raw) ? 1 : 0;
    static const int dbg_pad = getenv("K22_DBG_LDS_PAD") ? atoi(getenv("K22_DBG_LDS_PAD")) : 0;   // debug (tools/lds_victim_probe.py)
    const size_t smem0 = (size_t)L.depth * (L.bm + L.bn) * 128;
    L.lds = dbg_pad == 1 ? (smem0 + 1279) / 1280 * 1280 : (dbg_pad == 2 ? smem0 + 4096 : smem0);
  }
  const bool stream = L.family == IG_FAM_STREAM, generic = L.family == IG_FAM_GENERIC;
  if (qkv && !stream) {
    if (p.splitk > 1) return k22_set_error(K22_EINVAL, "igemm: the qkv projection splits K only on the streaming kernel");
    L.splitk = 1;
  }
  if (!stream) {
    if (p.res_f32 && !generic) return k22_set_error(K22_EINVAL, "igemm: fp32 residual is not supported by the halo kernel");
    if (p.S0 != nullptr && generic) return k22_set_error(K22_EINVAL, "igemm: the fused 1x1 skip connection needs the halo kernel");
    if (p.stats != nullptr && L.splitk == 1 && generic)
      return k22_set_error(K22_EINVAL, "igemm: GroupNorm partial sums requested from a configuration that cannot produce them");
  }
  L.grid *= (unsigned)L.splitk;   // (so far: the workgroups of one split)
  // the streaming kernel always leaves fp32 partials; the others finish a split only
  const bool finishes = stream || L.splitk > 1;
  L.finish = !finishes ? IG_FINISH_NONE : (reduce_rows_ok(p, p.stats != nullptr) ? IG_FINISH_ROWS : IG_FINISH_FLAT);
  // GroupNorm partial sums the launch could write: the row-tiled finish's 16-row blocks, else the 8-wave kernels' own m-tiles
  if (p.taps == 1 && (generic || p.H <= 0 || qkv)) L.stats_rows_per_image = 0;
  else if (finishes) L.stats_rows_per_image = reduce_rows_ok(p, true) ? (p.taps == 4 ? 4 : 1) * p.H * p.W / 16 : 0;
  else if (L.family == IG_FAM_UP2) L.stats_rows_per_image = 4 * conv3_up2_tiles_per_image(p, L.bm);
  else if (generic) L.stats_rows_per_image = 0;
  else L.stats_rows_per_image = p.taps == 1 ? gemm8_tiles_per_image(p, L.bm) : conv3_halo_tiles_per_image(p, L.bm);
  *out = L;
  return K22_OK;
}

int igemm_choose_splitk(const IgemmParams& p, int dtype) {
  IgemmParams q = p;
  q.splitk = 0;
  IgemmLaunch L;
  return igemm_resolve(q, dtype, &L) == K22_OK ? L.splitk : 1;
}

int igemm_stats_rows_per_image(const IgemmParams& p, int dtype) {
  IgemmLaunch L;
  return igemm_resolve(p, dtype, &L) == K22_OK ? L.stats_rows_per_image : 0;
}

// split-K finish of an engine of arithmetic type `dtype`: the partials are fp32 and so is what an x3 epilogue stores
static int launch_finish(const IgemmParams& q, int dtype, const IgemmLaunch& L, hipStream_t stream) {
  return k22_with_dtype(dtype, [&](auto tag) {
    using T0 = typename decltype(tag)::type;
    using T = typename std::conditional<is_x3<T0>::value, float, T0>::type;
    if (L.finish == IG_FINISH_ROWS) {
      hipLaunchKernelGGL((splitk_reduce_rows_kernel<T>), dim3((q.M + 15) / 16, (q.N + 63) / 64), dim3(256), 0, stream, q);
    } else {
      const int64_t total = (int64_t)q.M * q.N;
      int nb = (int)((total / 4 + 255) / 256);
      if (nb > 2048) nb = 2048;
      if (nb < 1) nb = 1;
      hipLaunchKernelGGL((splitk_reduce_kernel<T>), dim3(nb), dim3(256), 0, stream, q);
    }
    K22_CHECK_LAUNCH();
    return (int)K22_OK;
  });
}

template <typename T, int BM, int BN, int STAGES, bool ARAW>
static int run_generic(const IgemmParams& q, const IgemmLaunch& L, hipStream_t stream) {
  static LdsAttrGuard guard;
  return launch_lds_kernel(igemm_kernel<T, BM, BN, STAGES, ARAW>, guard, L.grid, L.block, L.lds, (int)L.lds, stream, q);
}
template <typename T, int BM, int BN>
static int launch_generic_tile(const IgemmParams& q, const IgemmLaunch& L, hipStream_t stream) {
  auto depth = [&](auto araw) {
    constexpr bool ARAW = decltype(araw)::value;
    if (L.depth == 2) return run_generic<T, BM, BN, 2, ARAW>(q, L, stream);
    if (L.depth == 3) return run_generic<T, BM, BN, 3, ARAW>(q, L, stream);
    return run_generic<T, BM, BN, 4, ARAW>(q, L, stream);
  };
  if constexpr (is_x3<T>::value) { if (L.a_raw) return depth(std::true_type{}); }
  return depth(std::false_type{});
}
static int launch_generic(const IgemmParams& q, int dtype, const IgemmLaunch& L, hipStream_t stream) {
  return k22_with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (L.bm == 128) return L.bn == 128 ? launch_generic_tile<T, 128, 128>(q, L, stream) : launch_generic_tile<T, 128, 64>(q, L, stream);
    return L.bn == 128 ? launch_generic_tile<T, 64, 128>(q, L, stream) : launch_generic_tile<T, 64, 64>(q, L, stream);
  });
}

int launch_igemm(const IgemmParams& p, int dtype, hipStream_t stream) {
  const int BK = k22_bk(dtype);
  if (p.a_raw && !k22_is_split(dtype)) return k22_set_error(K22_EINVAL, "igemm: a_raw is an option of the split-precision arithmetics only");
  if (p.M <= 0 || p.N <= 0) return K22_OK;
  if (p.taps != 1 && p.taps != 9 && p.taps != 4) return k22_set_error(K22_EINVAL, "igemm: taps must be 1, 9 or 4 (four-phase upsampling convolution)");
  if (p.Kc % BK != 0 || p.K0 % BK != 0) return k22_set_error(K22_EINVAL, "igemm: K per tap must be a multiple of 64 (bf16) / 32 (fp32)");
  if (p.Npad % 64 != 0 || p.Npad < p.N) return k22_set_error(K22_EINVAL, "igemm: Npad must be roundup(N,64)");
  if (p.K0 < p.Kc && p.A1 == nullptr) return k22_set_error(K22_EINVAL, "igemm: A1 missing for concat operand");
  if (p.out_mode == IG_OUT_QKV) {
    if (p.taps != 1 || p.N % 192 || (p.ldo & 3) || !p.kall || !p.vtall || p.att_T <= 0 || p.M % p.att_T || p.residual)
      return k22_set_error(K22_EINVAL, "igemm: bad qkv-projection problem (N = 3*heads*64, no residual)");
  }
  IgemmParams q = p;
  IgemmLaunch L;
  if (int rc = igemm_resolve(q, dtype, &L)) return rc;
  if (L.family == IG_FAM_STREAM) {
    if (p.partial == nullptr) return k22_set_error(K22_EINVAL, "igemm: the streaming kernel needs the fp32 partial buffer");
  } else if (L.splitk > 1 && p.partial == nullptr) {   // no scratch given: the problem runs unsplit
    q.splitk = 1;
    if (int rc = igemm_resolve(q, dtype, &L)) return rc;
  }
  if (L.finish == IG_FINISH_FLAT && q.stats != nullptr)
    return k22_set_error(K22_EINVAL, "igemm: GroupNorm partial sums are not available for this split-K problem");
  q.splitk = L.splitk; q.xcd_remap = L.xcd_remap; q.algo = L.algo;
  int rc;
  switch (L.family) {
    case IG_FAM_STREAM: rc = launch_stream(q, dtype, L, stream); break;
    case IG_FAM_GEMM8: case IG_FAM_GEMM8_SPEC: rc = launch_gemm8(q, dtype, L, stream); break;
    case IG_FAM_SPEC: rc = launch_conv3_halo_spec(q, dtype, L, stream); break;
    case IG_FAM_UP2: rc = launch_conv3_up2(q, dtype, L, stream); break;
    case IG_FAM_GENERIC: rc = launch_generic(q, dtype, L, stream); break;
    default: rc = launch_conv3_halo(q, dtype, L, stream); break;
  }
  if (rc || L.finish == IG_FINISH_NONE) return rc;
  return launch_finish(q, dtype, L, stream);
}
