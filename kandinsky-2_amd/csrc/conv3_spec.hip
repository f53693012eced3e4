// k22 - conv3_halo_spec_kernel: the LDS-resident-halo 3x3 convolution with producer / consumer wave specialisation (the tile
// table's pick for most convolutions of a step).  Split from conv3_halo.hip (frame, LDS images and epilogue described there) so that it
// builds on its own.
#include "conv3_common.h"

// ================================================================================================================
// conv3_halo_spec_kernel (IG_ALGO_SPEC / IG_ALGO_SPEC_PIPE = algo 11 / 12): the same tile, LDS images and epilogue with the eight waves SPECIALISED.
//   waves 0-3 ("consumers", one per SIMD): 2 x 2 over the BM x 128 tile, (BM/2) x 64 per wave (BM = 256: 128 x 64 = 8
//              accumulators, 6 fragment reads per 8 MFMAs instead of 4 per 4); per tap they do nothing but read fragments and
//              issue MFMAs - no LDS-DMA instruction, no vmcnt wait;
//   waves 4-7 ("producers", the second wave of every SIMD): issue all the LDS-DMA of a tap (4 weight pieces + 2 halo pieces
//              each) right after its barrier and sit in the counted vmcnt wait for the next tap's tile.
// Producers and consumers execute the same barriers (one per tap): the ring-slot / halo-buffer reuse argument of
// conv3_halo_kernel holds unchanged.
// BM = 224 (16-bit types, PIPE only): the tile that divides a 96 x 98 plane exactly - 42 tiles per image, 252
//              workgroups of a 2 x 384-channel problem on 256 CUs where BM = 256 makes 222 - and whose halo image (424 rows) leaves room for a
//              THIRD weight slot there.  7 m-blocks do not halve, so the consumers take one 32-column strip each (1 x 4: 7 accumulators,
//              7 + 1 fragment reads per 7 MFMAs; K22_INTERLEAVE_LEAD).  Same MFMA, same order of slabs, taps and k-steps per element.
// PIPE (algo 12): explicit fragment pipeline in the consumers.  The fragments of k-step ks+1 are read while the MFMAs of
// k-step ks are issued (two register sets), and the last k-step of a tap is multiplied after the next tap's barrier, where
// its eight MFMAs cover the latency of that tap's first fragment reads.  Within a block the reads and the MFMAs are
// INTERLEAVED one read behind every MFMA (sched_group_barrier): issued as a read burst and an MFMA burst, the matrix pipe
// idles while the one wave that owns it spends its issue slots on ds_read_b128s.  Measured (bench_kernels, all 3x3
// convolutions of one step): 4.09 ms against 4.51 ms for the best lock-step variant at BM = 256, 4.43 against 4.77 at
// BM = 128; the specialisation alone (algo 11, compiler-scheduled consumers) is +-0 - it is the interleaved pipeline that the
// one-owner matrix pipe makes worthwhile.
// What the loads cost (measured with two wrong-result forms that have since left the source: producers that issue nothing inside the tap
// loop - the consumers' speed limit under the same barriers - and LDS-DMA that is issued but never waited for).  At 96x96
// 768->768, same box: 1.08 PFLOP/s complete, 1.22 without the waits, 1.39 without the loads - half of what the loads cost
// there is the ONE tap a tile has to land in (2-slot ring: the LDS holds the double-buffered halo), half is contention;
// where four slots fit (48x48) the waits cost nothing and the contention is the same 12-14 %.  Staging the weight tiles
// through producer registers (global_load two taps ahead, ds_write_b128 into the 2-slot ring) was built and measured equal
// to the LDS-DMA form at 96x96 and slower elsewhere; removed.  So was a four-block form of the consumer pipeline that reads the
// weight fragments of the last k-step one block early (only halo reads in flight at the barrier, no full read wait with the
// 2-slot ring): same-box A/B/A/B 1.718-1.740 ms for all three forms on the 96x96 / 48x48 shapes.  So was a producer form that applied
// GroupNorm, FiLM and SiLU to the raw tensor as it landed in the LDS: bit-identical to gn_apply + this kernel, 21 % slower per step
// (profiles/r04_gn_fused_negative.txt).
// ================================================================================================================
template <typename T, int BM, int NBST, bool PIPE = false>
__global__ __launch_bounds__(512) void conv3_halo_spec_kernel(const IgemmParams p) {
  using TR = TT<T>;
  constexpr int BK = TR::BK, EPC = TR::EPC, KSTEPS = TR::KSTEPS;
  constexpr int BN = HALO_BN, NWL = 4, WM = halo_wm<BM, true>(), WN = halo_wn<BM, true>();
  constexpr int MI = BM / (WM * 32), NI = BN / (WN * 32);
  constexpr bool STRIP = BM == HALO_BM_STRIP;  // 224 rows: one 32-column strip per consumer
  constexpr int B_SLOTS = BN / 8 / NWL;        // 4 weight LDS-DMA instructions per producer per tap
  constexpr int B_BYTES = BN * 128;
  constexpr int APT = 2;                       // halo pieces per producer per tap (taps 0 .. 9-NBST)
  constexpr int A_SLOTS = (10 - NBST) * APT;
  constexpr bool GASM = true;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool producer = wave >= 4;             // wave-uniform
  const int h = lane >> 5, l31 = lane & 31;

  const int W2 = p.W + 2;
  const int VR = p.H * W2;
  const int TPI = (VR + BM - 1) / BM;
  const int HRp = (BM + 2 * W2 + 2 + 7) & ~7;
  const int NP = HRp >> 3;
  const int A_BYTES = HRp * 128;
  const int PR_MAX = (p.H + 2) * W2 - 1;
  const int B = p.M / (p.H * p.W);

  int bz, bx, by;
  tile_block_map(p.xcd_remap, B * TPI, (p.N + BN - 1) / BN, bz, bx, by);
  const int img = bx / TPI, v0 = (bx - img * TPI) * BM;
  const int n0 = by * BN;
  int s0, s1;
  splitk_range(p.splitk, p.Kc / BK, bz, s0, s1);

  f32x16_t acc[MI][NI];
  K22_ZERO_ACC(acc, MI, NI)

  char* const Bst = smem + 2 * A_BYTES;
  // The producers' K loop: per tap the loaders' half (K22_TAP_FRONT), then the rotation of the ring slot
#define K22_PRODUCER_TAP(TAP, ...)                                                                         \
  {                                                                                                        \
    K22_TAP_FRONT(TAP, 9, lw, NWL, APT, lds0 + (unsigned)anext_off, lds0 + 2 * A_BYTES)                    \
    fill = (fill + 1 == NBST) ? 0 : fill + 1;                                                              \
  }
#define K22_PRODUCER_LOOP()                                                                                \
  int fill = NBST - 1;                                                                                     \
  for (int s = s0; s < s1; ++s) {                                                                          \
    const int anext_off = (((s - s0) & 1) ^ 1) * A_BYTES;                                                  \
    const int sn = s + 1 < s1 ? s + 1 : s1 - 1;   /* past-the-end loads re-read the last slab (uniform counting) */ \
    K22_TAPS_9(K22_PRODUCER_TAP, )                                                                         \
  }
#undef K22_LDS_ADDR
#undef K22_LDS_PTR
#define K22_LDS_ADDR(AT) (AT)
#define K22_LDS_PTR(AT) (smem + ((AT) - lds0))
  if (s0 < s1) {
    if (producer) {
      // ---------------------------------------- producers: LDS-DMA only -----------------------------------------------
      const int lw = wave - 4;
      const T* __restrict__ Aimg = reinterpret_cast<const T*>(p.A0) + (int64_t)img * (p.H + 2) * W2 * p.Kc;
      const T* __restrict__ Wp = reinterpret_cast<const T*>(p.Wp);
      int aoff[A_SLOTS], boff[B_SLOTS];
      K22_PIECE_OFFSETS(aoff, A_SLOTS, lw, NWL, v0, NP, 8)
      K22_ROW_OFFSETS(boff, B_SLOTS, lw, NWL, n0, p.Npad - 1, n * 9 * p.Kc)
      const unsigned lds0 = halo_lds_base(smem);
#pragma unroll
      for (int q = 0; q < A_SLOTS; ++q) K22_ISSUE_A(lw, NWL, q, s0, lds0);
#pragma unroll
      for (int t = 0; t < NBST - 1; ++t) K22_ISSUE_B(lw, NWL, t * p.Kc + s0 * BK, lds0 + 2 * A_BYTES + t * B_BYTES);
      K22_PRODUCER_LOOP()
    } else {
      // ---------------------------------------- consumers: fragments + MFMA only --------------------------------------
      const int wm = STRIP ? 0 : wave >> 1, wn = STRIP ? wave : wave & 1;
      const int abase = wm * (BM / WM) + l31;
      int brow[NI];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) brow[ni] = (wn * (BN / WN) + ni * 32 + l31) * 128;
      const int bsw = (l31 >> 1) & 7;
      int cur = 0;
      // (s_setprio 3 in the consumers, so that they win issue arbitration against the producer on their SIMD: measured +-1 %)
      FragA<T> pa[MI];          // PIPE: fragments read but not yet multiplied (zero = a no-op group before the first tap)
      Frag<T> pb[NI];
      if constexpr (PIPE) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) pa[mi] = FragA<T>{};
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) pb[ni] = Frag<T>{};
      }
      constexpr int NRD = halo_pipe_reads<T, MI, NI>(), NMF = MI * NI * FragCost<T>::MFMAS, MPR = NMF / NRD;   // K22_INTERLEAVE
#define K22_SP_CTAP(TAP, ...)                                                                              \
      {                                                                                                    \
        raw_barrier();                                                                                     \
        K22_TAP_COMPUTE(TAP, 9,                                                                            \
          if constexpr (PIPE && STRIP) K22_TAP_PIPE(FragA<T>, Frag<T>, arow[mi], asw[mi], Bcur + brow[ni], bsw, (void)0, K22_INTERLEAVE_LEAD()) \
          else if constexpr (PIPE) K22_TAP_PIPE(FragA<T>, Frag<T>, arow[mi], asw[mi], Bcur + brow[ni], bsw, K22_PIPE_INTERLEAVED) \
          else { K22_TAP_PLAIN(FragA<T>, Frag<T>, ld_frag_at, arow[mi], asw[mi], Bcur + brow[ni], bsw) })  \
      }
      for (int s = s0; s < s1; ++s) {
        const char* const Acur = smem + ((s - s0) & 1) * A_BYTES;
        K22_TAPS_9(K22_SP_CTAP, )
      }
#undef K22_SP_CTAP
      if constexpr (PIPE) { K22_MMA_ALL(pb, pa) }
    }
  }
#undef K22_LDS_ADDR
#undef K22_LDS_PTR
#define K22_LDS_ADDR(AT) (lds0 + (unsigned)((AT) - smem))
#define K22_LDS_PTR(AT) (AT)
#undef K22_PRODUCER_TAP
#undef K22_PRODUCER_LOOP
  halo_tail<T, BM, false, true>(p, acc, smem, bx, bz, img, v0, n0);
}

// conv3_halo_spec_kernel<T, BM, depth, PIPE> at the ring depth L.depth
template <typename T, int BM, bool PIPE>
static int launch_spec_depth(const IgemmParams& p, const IgemmLaunch& L, hipStream_t stream) {
  return halo_with_depth<2, 3, 4, 6>(L.depth, [&](auto d) { return halo_run<conv3_halo_spec_kernel<T, BM, decltype(d)::value, PIPE>>(p, L, stream); });
}

// L.pipe: 0 = compiler-scheduled consumers, 1 = explicit, interleaved fragment pipeline.  x3 and fp32 at BM = 256 have no pipelined form (two
// fragment sets of 8 registers per fragment do not fit beside 128 accumulators: it spills); the asymmetric split's activation fragments are 4
// registers (hi halves only), so its two-set pipeline fits at BM = 256 too.
int launch_conv3_halo_spec(const IgemmParams& p, int dtype, const IgemmLaunch& L, hipStream_t stream) {
  return k22_with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    // the 224-row tile: 16-bit types, pipelined form (112 accumulators beside two sets of 7 + 1 fragments of 4 registers; the wider
    // fragments of the other types do not fit).  conv3_halo_supported says the same; a launch that names it otherwise is refused.
    constexpr bool pipe224 = std::is_same<T, bf16_t>::value || std::is_same<T, f16_t>::value;
    if (L.bm == HALO_BM_STRIP && !(pipe224 && L.pipe))
      return k22_set_error(K22_EINVAL, "conv3_halo_spec: the 224-row tile is the pipelined 16-bit form only");
    if (!L.pipe) return halo_with_bm(L.bm, [&](auto bm) { return launch_spec_depth<T, decltype(bm)::value, false>(p, L, stream); });
    constexpr bool pipe256 = !std::is_same<T, x3_t>::value && !std::is_same<T, float>::value;
    return halo_with_bm<pipe256, pipe224>(L.bm, [&](auto bm) { return launch_spec_depth<T, decltype(bm)::value, true>(p, L, stream); });
  });
}
