// k22 - gemm8_kernel / gemm8_spec_kernel: plain GEMM (1x1 convolutions: qkv / proj_out of the AttentionBlocks) on the 8-wave frame of the
// LDS-resident-halo convolution (conv3_halo.hip: frame and LDS images; conv3_common.h: the shared epilogue halo_tail).  Split from
// conv3_halo.hip so that it builds on its own.
#include "conv3_common.h"

// ================================================================================================================
// gemm8_kernel: plain GEMM  out[m][n] = sum_k A[m][k] W[n][k]  (1x1 convolutions: qkv / proj_out of the AttentionBlocks,
// kandinsky2/model/unet.py:244-268) on the frame of the halo kernel: 8 waves (4 x 2), BM x 128 tile, BM in {256, 128},
// both operands through an NST-deep LDS-DMA ring (one 128-byte-row K slab of A and of W per stage, counted vmcnt, one
// raw barrier per slab) and the same epilogue through LDS (halo_tail): 16-byte stores, bias + residual, GroupNorm
// partial sums of the stored values, or the qkv-projection layout.  Against igemm_kernel (4 waves, <= 128 x 128):
// twice the FLOPs per L2->LDS byte at 256 x 128 and two waves per SIMD; m-tiles never straddle an image (rows of a
// tile past the image are masked), so the per-tile statistics are per-image statistics.
// (Round 2: a variant that staged both operands through registers - plain global_load two slabs ahead, ds_write_b128 into a
// two-stage LDS ring, no LDS-DMA - was built, parity-green, and measured equal: 1.29 ms against 1.26-1.31 ms for the GEMMs of one
// step.  The K loop of these GEMMs is not bound by the LDS-DMA issue cost; removed.)
// ================================================================================================================
// one K slab of both operands into ring stage STAGE, by loader wave LW of NWL: A tile, then W tile behind it
#define K22_ISSUE_G(LW, NWL, SLAB, STAGE)                                                                  \
  {                                                                                                        \
    int sl_ = (SLAB);                                                                                      \
    if (sl_ > s1 - 1) sl_ = s1 - 1;   /* past-the-end stages re-read the last slab: uniform counting */    \
    const unsigned d_ = lds0 + (STAGE) * BUF + (LW) * 1024;                                                \
    K22_ISSUE_ROWS(false, A, aoff, A_SLOTS, NWL, sl_ * BK, d_, smem + (d_ - lds0))                         \
    K22_ISSUE_ROWS(true, Wp, boff, B_SLOTS, NWL, sl_ * BK, d_ + A_BYTES, smem + (d_ - lds0) + A_BYTES)     \
  }
template <typename T, int BM, int NST, bool ARAW = false>
__global__ __launch_bounds__(512) void gemm8_kernel(const IgemmParams p) {
  using TR = TT<T>;
  constexpr int BK = TR::BK, EPC = TR::EPC, KSTEPS = TR::KSTEPS;
  constexpr int BN = HALO_BN, NW = HALO_NW, WM = 4, WN = 2;
  constexpr int MI = BM / (WM * 32), NI = BN / (WN * 32);
  constexpr int A_SLOTS = BM / 8 / NW, B_SLOTS = BN / 8 / NW, CH = A_SLOTS + B_SLOTS;
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, BUF = A_BYTES + B_BYTES;
  constexpr bool GASM = true;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, l31 = lane & 31;

  const int HW = p.H > 0 ? p.H * p.W : p.M;   // rows per image
  const int TPI = (HW + BM - 1) / BM;
  const int B = p.M / HW;
  int bz, bx, by;
  tile_block_map(p.xcd_remap, B * TPI, (p.N + BN - 1) / BN, bz, bx, by);
  const int img = bx / TPI, v0 = (bx - img * TPI) * BM;
  const int n0 = by * BN;

  const T* __restrict__ A = reinterpret_cast<const T*>(p.A0) + (int64_t)img * HW * p.lda0;
  const T* __restrict__ Wp = reinterpret_cast<const T*>(p.Wp);
  int aoff[A_SLOTS], boff[B_SLOTS];
  K22_ROW_OFFSETS(aoff, A_SLOTS, wave, NW, v0, HW - 1, n * (int)p.lda0)   // rows past the image re-read its last pixel; they are never stored
  K22_ROW_OFFSETS(boff, B_SLOTS, wave, NW, n0, p.Npad - 1, n * p.Kc)
  int s0, s1;
  splitk_range(p.splitk, p.Kc / BK, bz, s0, s1);

  f32x16_t acc[MI][NI];
  K22_ZERO_ACC(acc, MI, NI)

  const unsigned lds0 = halo_lds_base(smem);
  int arow[MI], brow[NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) arow[mi] = (wm * (BM / WM) + mi * 32 + l31) * 128;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) brow[ni] = A_BYTES + (wn * (BN / WN) + ni * 32 + l31) * 128;
  const int sw = (l31 >> 1) & 7;

  if (s0 < s1) {
#pragma unroll
    for (int t = 0; t < NST - 1; ++t) K22_ISSUE_G(wave, NW, s0 + t, t);
    int cur = 0, fill = NST - 1;
    for (int s = s0; s < s1; ++s) {
      wait_vmcnt<(NST - 2) * CH>();
      raw_barrier();
      K22_ISSUE_G(wave, NW, s + NST - 1, fill);
      const char* St = smem + cur * BUF;
      K22_TAP_PLAIN(FragA<T>, Frag<T>, (ld_frag_at_a<ARAW, T>), St + arow[mi], sw, St + brow[ni], sw)
      cur = (cur + 1 == NST) ? 0 : cur + 1;
      fill = (fill + 1 == NST) ? 0 : fill + 1;
    }
  }
  halo_tail<T, BM, true>(p, acc, smem, bx, bz, img, v0, n0);
}

// ================================================================================================================
// gemm8_spec_kernel (round 6, p.stages == 3 / 4; 16-bit types): gemm8_kernel's tile, ring and epilogue with the eight waves SPECIALISED the way
// conv3_halo_spec_kernel's are - what the tuning report of the C3 shape asked for: at M = 32 768 the lock-step GEMM ran at 0.18-0.29 of the
// bf16 peak (qkv 64x64: 161 us for 116 GFLOP) beside 3x3 convolutions of the same tile at 0.57.
//   waves 0-3 (consumers, one per SIMD): 2 x 2 over the BM x 128 tile, (BM/2) x 64 per wave; per slab they read fragments and issue MFMAs
//              through the explicit two-set pipeline (reads of k-step ks + 1 interleaved one behind every MFMA of k-step ks; the last k-step
//              of a slab is multiplied behind the next slab's barrier) - no LDS-DMA, no vmcnt wait;
//   waves 4-7 (producers): all the LDS-DMA of a slab (BM/32 + 4 pieces each) right behind its barrier, then the counted vmcnt wait.
// One raw barrier per slab for all eight waves; slot reuse as in gemm8_kernel (iteration s refills the stage iteration s - 1 read; the
// consumers drain lgkmcnt before the next barrier).  Every accumulator sees the same MFMAs in the same k order as in gemm8_kernel: same bits.
// ================================================================================================================
template <typename T, int BM, int NST>
__global__ __launch_bounds__(512) void gemm8_spec_kernel(const IgemmParams p) {
  using TR = TT<T>;
  static_assert(sizeof(T) == 2, "gemm8_spec_kernel: 16-bit operands");
  constexpr int BK = TR::BK, EPC = TR::EPC, KSTEPS = TR::KSTEPS;
  static_assert(KSTEPS % 2 == 0, "two-set fragment pipeline");
  constexpr int BN = HALO_BN, NWL = 4, WM = 2, WN = 2;
  constexpr int MI = BM / (WM * 32), NI = BN / (WN * 32);
  constexpr int A_SLOTS = BM / 8 / NWL, B_SLOTS = BN / 8 / NWL, CH = A_SLOTS + B_SLOTS;
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, BUF = A_BYTES + B_BYTES;
  constexpr bool GASM = true;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool producer = wave >= 4;   // wave-uniform
  const int h = lane >> 5, l31 = lane & 31;

  const int HW = p.H > 0 ? p.H * p.W : p.M;   // rows per image
  const int TPI = (HW + BM - 1) / BM;
  const int B = p.M / HW;
  int bz, bx, by;
  tile_block_map(p.xcd_remap, B * TPI, (p.N + BN - 1) / BN, bz, bx, by);
  const int img = bx / TPI, v0 = (bx - img * TPI) * BM;
  const int n0 = by * BN;
  int s0, s1;
  splitk_range(p.splitk, p.Kc / BK, bz, s0, s1);

  f32x16_t acc[MI][NI];
  K22_ZERO_ACC(acc, MI, NI)

  if (s0 < s1) {
    if (producer) {
      const int lw = wave - 4;
      const T* __restrict__ A = reinterpret_cast<const T*>(p.A0) + (int64_t)img * HW * p.lda0;
      const T* __restrict__ Wp = reinterpret_cast<const T*>(p.Wp);
      int aoff[A_SLOTS], boff[B_SLOTS];
      K22_ROW_OFFSETS(aoff, A_SLOTS, lw, NWL, v0, HW - 1, n * (int)p.lda0)   // rows past the image re-read its last pixel; they are never stored
      K22_ROW_OFFSETS(boff, B_SLOTS, lw, NWL, n0, p.Npad - 1, n * p.Kc)
      const unsigned lds0 = halo_lds_base(smem);
#pragma unroll
      for (int t = 0; t < NST - 1; ++t) K22_ISSUE_G(lw, NWL, s0 + t, t);
      int fill = NST - 1;
      for (int s = s0; s < s1; ++s) {
        wait_vmcnt<(NST - 2) * CH>();
        raw_barrier();
        K22_ISSUE_G(lw, NWL, s + NST - 1, fill);
        fill = (fill + 1 == NST) ? 0 : fill + 1;
      }
    } else {
      const int wm = wave >> 1, wn = wave & 1;
      int arow[MI], brow[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) arow[mi] = (wm * (BM / WM) + mi * 32 + l31) * 128;
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) brow[ni] = A_BYTES + (wn * (BN / WN) + ni * 32 + l31) * 128;
      const int sw = (l31 >> 1) & 7;
      Frag<T> pa[MI], pb[NI];          // fragments read but not yet multiplied (zero = a no-op group before the first slab)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) pa[mi] = Frag<T>{};
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) pb[ni] = Frag<T>{};
      constexpr int NRD = halo_pipe_reads<T, MI, NI>(), NMF = MI * NI * FragCost<T>::MFMAS, MPR = NMF / NRD;
      int cur = 0;
      for (int s = s0; s < s1; ++s) {
        raw_barrier();
        const char* St = smem + cur * BUF;
        K22_TAP_PIPE(Frag<T>, Frag<T>, St + arow[mi], sw, St + brow[ni], sw, K22_PIPE_INTERLEAVED)
        K22_READS_DONE();
        cur = (cur + 1 == NST) ? 0 : cur + 1;
      }
      K22_MMA_ALL(pb, pa)
    }
  }
  halo_tail<T, BM, true, true>(p, acc, smem, bx, bz, img, v0, n0);
}

#undef K22_ISSUE_G

// ---- host side ---------------------------------------------------------------------------------
size_t gemm8_lds_bytes(int bm, int nst) { return halo_lds_budget(bm, false, (size_t)nst * (bm + HALO_BN) * 128); }
int gemm8_tiles_per_image(const IgemmParams& p, int bm) { return ((p.H > 0 ? p.H * p.W : p.M) + bm - 1) / bm; }

bool gemm8_supported(const IgemmParams& p, int dtype, int bm) {
  const int BK = k22_bk(dtype);
  if (p.taps != 1 || (bm != 256 && bm != 128) || p.N < 128) return false;
  if (p.K0 != p.Kc || p.S0 != nullptr || p.res_f32) return false;          // one A operand, no fused skip, T residual
  if (p.out_mode != IG_OUT_ROWMAJOR && p.out_mode != IG_OUT_ROWMAJOR_F32 && p.out_mode != IG_OUT_QKV) return false;
  if (p.N % 8 || p.ldo % 8 || (p.residual && p.ldr % 8) || p.Kc % BK || p.lda0 % 8) return false;
  const int hw = p.H > 0 ? p.H * p.W : p.M;
  if (hw <= 0 || p.M % hw) return false;
  if (p.out_mode == IG_OUT_QKV && (p.att_T != hw || p.N % 384)) return false;  // an n-tile stays inside q, k or v
  if ((int64_t)p.M * p.lda0 >= (1ll << 31) || (int64_t)p.Npad * p.Kc >= (1ll << 31)) return false;
  return true;
}

// the specialised, pipelined form: 16-bit types (the split types keep the lock-step kernel)
bool gemm8_spec_supported(int dtype) { return dtype == K22_BF16 || dtype == K22_F16; }

// Launches the kernel the resolved launch names - rings (BM, NST): (256, 3), (128, 4), (128, 2) - only; a split-K reduction is the caller's (launch_igemm).
int launch_gemm8(const IgemmParams& p, int dtype, const IgemmLaunch& L, hipStream_t stream) {
  return k22_with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    auto ring = [&](auto run) {
      using std::integral_constant;
      return L.bm == 256 ? run(integral_constant<int, 256>{}, integral_constant<int, 3>{})
                         : (L.depth != 2 ? run(integral_constant<int, 128>{}, integral_constant<int, 4>{}) : run(integral_constant<int, 128>{}, integral_constant<int, 2>{}));
    };
    if (L.family == IG_FAM_GEMM8_SPEC) {
      if constexpr (sizeof(T) == 2) return ring([&](auto bm, auto nst) { return halo_run<gemm8_spec_kernel<T, decltype(bm)::value, decltype(nst)::value>>(p, L, stream); });
      else return k22_set_error(K22_EINVAL, "gemm8: unsupported problem");
    }
    if constexpr (is_x3<T>::value) {
      if (L.a_raw) return ring([&](auto bm, auto nst) { return halo_run<gemm8_kernel<T, decltype(bm)::value, decltype(nst)::value, true>>(p, L, stream); });
    }
    return ring([&](auto bm, auto nst) { return halo_run<gemm8_kernel<T, decltype(bm)::value, decltype(nst)::value, false>>(p, L, stream); });
  });
}
