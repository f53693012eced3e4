// k22 - conv3_halo_spec_kernel: the LDS-resident-halo 3x3 convolution with producer / consumer wave specialisation (the tile
// table's pick for most convolutions of a step) and, in its producers, the fused GroupNorm-apply (nn.py:26-37, unet.py:150-152,
// 174-180, 212-216).  Split from conv3_halo.hip (frame, LDS images and epilogue described there) so that it builds on its own.
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
// BM = 224 (16-bit types, PIPE only; no fused GroupNorm-apply): the tile that divides a 96 x 98 plane exactly - 42 tiles per image, 252
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
// DBG (measurement only, wrong results): 1 (algo 13) = the producers issue nothing inside the tap loop - what is left is
// the consumers' speed limit under the same barriers; 2 (algo 14) = the LDS-DMA is issued but never waited for.  At 96x96
// 768->768, same box: 1.08 PFLOP/s complete, 1.22 without the waits, 1.39 without the loads - half of what the loads cost
// there is the ONE tap a tile has to land in (2-slot ring: the LDS holds the double-buffered halo), half is contention;
// where four slots fit (48x48) the waits cost nothing and the contention is the same 12-14 %.  Staging the weight tiles
// through producer registers (global_load two taps ahead, ds_write_b128 into the 2-slot ring) was built and measured equal
// to the LDS-DMA form at 96x96 and slower elsewhere; removed.  So was a four-block form of the consumer pipeline that reads the
// weight fragments of the last k-step one block early (only halo reads in flight at the barrier, no full read wait with the
// 2-slot ring): same-box A/B/A/B 1.718-1.740 ms for all three forms on the 96x96 / 48x48 shapes.
// ================================================================================================================
template <typename T, int BM, int NBST, bool PIPE = false, int DBG = 0>
__global__ __launch_bounds__(512) void conv3_halo_spec_kernel(const IgemmParams p) {
  using TR = TT<T>;
  constexpr int BK = TR::BK, EPC = TR::EPC, KSTEPS = TR::KSTEPS;
  constexpr int BN = HALO_BN, NWL = 4, WM = halo_wm<BM, true>(), WN = halo_wn<BM, true>();
  constexpr int MI = BM / (WM * 32), NI = BN / (WN * 32);
  constexpr bool STRIP = BM == HALO_BM_STRIP;  // 224 rows: one 32-column strip per consumer, no fused GroupNorm-apply form
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
  halo_block_map(p, B * TPI, (p.N + BN - 1) / BN, bz, bx, by);
  const int img = bx / TPI, v0 = (bx - img * TPI) * BM;
  const int n0 = by * BN;
  int s0, s1;
  halo_slab_range(p, p.Kc / BK, bz, s0, s1);

  f32x16_t acc[MI][NI];
  halo_zero_acc(acc);

  char* const Bst = smem + 2 * A_BYTES;
  // The producers' K loop, shared by their two forms: per tap the loaders' half (K22_TAP_FRONT; WAITS / LOADS: the DBG forms leave one
  // out), whatever the form does to what has landed (AFTER), the rotation of the ring slot
#define K22_PRODUCER_TAP(TAP, WAITS, LOADS, ISSUE_HALO, AFTER)                                             \
  {                                                                                                        \
    K22_TAP_FRONT(TAP, 9, lw, NWL, APT, WAITS, LOADS, ISSUE_HALO, lds0 + (unsigned)anext_off, lds0 + 2 * A_BYTES) \
    AFTER(TAP)                                                                                             \
    fill = (fill + 1 == NBST) ? 0 : fill + 1;                                                              \
  }
#define K22_PRODUCER_LOOP(WAITS, LOADS, ISSUE_HALO, AFTER)                                                 \
  int fill = NBST - 1;                                                                                     \
  for (int s = s0; s < s1; ++s) {                                                                          \
    const int anext_off = (((s - s0) & 1) ^ 1) * A_BYTES;                                                  \
    const int sn = s + 1 < s1 ? s + 1 : s1 - 1;   /* past-the-end loads re-read the last slab (uniform counting) */ \
    const bool more = s + 1 < s1;                 /* a next slab exists */                                 \
    K22_TAPS_9(K22_PRODUCER_TAP, WAITS, LOADS, ISSUE_HALO, AFTER)                                          \
  }
#define K22_PRODUCER_NOTHING(TAP)
#undef K22_LDS_ADDR
#undef K22_LDS_PTR
#define K22_LDS_ADDR(AT) (AT)
#define K22_LDS_PTR(AT) (smem + ((AT) - lds0))
  if (s0 < s1) {
    if (!STRIP && producer && p.gn_coeff != nullptr) {
      // ------------------------- producers, fused GroupNorm-apply: LDS-DMA of the RAW tensor, then rewrite in place ---------------------
      // The halo piece a producer wave loaded is rewritten by the SAME wave one tap later (its own counted vmcnt orders the ds_read behind
      // the DMA; no other wave touches the buffer until the barrier that opens the next slab): y = act(x * A[c] + Bc[c]), zero at the
      // border positions of the padded plane - which the raw tensor does not have: the per-lane source is the unpadded pixel (clamped at
      // the border; those lanes' values are discarded).  A lane's 16 bytes are the same channel chunk in every piece of its wave
      // (chunk = (lane & 7) ^ ((4 * (wave & 1) + (lane >> 4)) & 7): the piece index has the wave's parity), so its 2 * EPC coefficients
      // live in registers, re-loaded once per slab.  Surplus slots (pieces past the halo; the lock-step counting wants every wave to issue the
      // same number of DMAs) do not re-load the last piece - that would land raw bytes on rewritten ones - but 1 KB of the weights into a
      // scratch piece behind the weight ring that nobody reads (a plain load with a register destination would do for the counting, but a
      // register written by a load the compiler does not know about is a register it re-uses meanwhile).
      const int lw = wave - 4;
      constexpr int NCF = EPC / 2;                   // 16-byte registers of coefficients per lane: (A, Bc) x EPC channels
      const T* __restrict__ X0 = reinterpret_cast<const T*>(p.gn_x0) + (int64_t)img * p.H * p.W * p.gn_C0;
      const int C1 = p.Kc - p.gn_C0;
      const T* __restrict__ X1 = p.gn_x1 ? reinterpret_cast<const T*>(p.gn_x1) + (int64_t)img * p.H * p.W * C1 : nullptr;
      const T* __restrict__ Wp = reinterpret_cast<const T*>(p.Wp);
      const int gchunk = (lane & 7) ^ ((4 * (lw & 1) + (lane >> 4)) & 7);
      const float* __restrict__ cfbase = p.gn_coeff + ((int64_t)img * p.Kc + gchunk * EPC) * 2;
      int pix[A_SLOTS];
      unsigned bmask = 0;
#pragma unroll
      for (int q = 0; q < A_SLOTS; ++q) {
        int j = q * NWL + lw;
        if (j > NP - 1) j = NP - 1;
        const int hr = 8 * j + (lane >> 3);
        int pr = v0 + hr;
        if (pr > PR_MAX) pr = PR_MAX;
        const int y = pr / W2, x = pr - y * W2;          // padded coordinates
        const bool border = y < 1 || y > p.H || x < 1 || x > p.W;
        const int yy = y < 1 ? 0 : (y > p.H ? p.H - 1 : y - 1), xx = x < 1 ? 0 : (x > p.W ? p.W - 1 : x - 1);
        pix[q] = yy * p.W + xx;
        bmask |= (border ? 1u : 0u) << q;
      }
      int boff[B_SLOTS];
      K22_ROW_OFFSETS(boff, B_SLOTS, lw, NWL, n0, p.Npad - 1, n * 9 * p.Kc)
      const unsigned lds0 = halo_lds_base(smem);
      const unsigned lds_scratch = lds0 + 2 * A_BYTES + NBST * B_BYTES;
      u32x4_t cfr[NCF];
#pragma unroll
      for (int k = 0; k < NCF; ++k) cfr[k] = u32x4_t{0u, 0u, 0u, 0u};
      // K22_ISSUE_A's signature: the raw pixels of the piece, or the scratch load of a surplus slot
#define K22_GN_A(LW, NWL_, Q, SLAB, DST)                                                                   \
      {                                                                                                    \
        const int jn_ = (Q) * (NWL_) + (LW);                                                               \
        if (jn_ > NP - 1) {                                                                                \
          glds16_asm(reinterpret_cast<const char*>(p.Wp) + lane * 16, __builtin_amdgcn_readfirstlane(lds_scratch)); \
        } else {                                                                                           \
          const int k0_ = (SLAB) * BK;                                                                     \
          const bool second_ = k0_ >= p.gn_C0;                                                             \
          const T* sp_ = (second_ ? X1 + (int64_t)pix[Q] * C1 + (k0_ - p.gn_C0) : X0 + (int64_t)pix[Q] * p.gn_C0 + k0_) + gchunk * EPC; \
          glds16_asm(sp_, __builtin_amdgcn_readfirstlane((DST) + jn_ * 1024));                             \
        }                                                                                                  \
      }
#define K22_GN_COEF(SLAB)                                                                                  \
      {                                                                                                    \
        _Pragma("unroll") for (int k = 0; k < NCF; ++k) gload16_asm(cfr[k], cfbase + (int64_t)(SLAB) * BK * 2 + 4 * k); \
      }
#define K22_GN_REWRITE(Q, DSTOFF)                                                                          \
      {                                                                                                    \
        const int jn_ = (Q) * NWL + lw;                                                                    \
        if (jn_ <= NP - 1) {                                                                               \
          u32x4_t* a_ = reinterpret_cast<u32x4_t*>(smem + (DSTOFF) + jn_ * 1024 + lane * 16);              \
          float cf_[2 * EPC];                                                                              \
          _Pragma("unroll") for (int k = 0; k < NCF; ++k) {                                                \
            cf_[4 * k] = __uint_as_float(cfr[k].x); cf_[4 * k + 1] = __uint_as_float(cfr[k].y);            \
            cf_[4 * k + 2] = __uint_as_float(cfr[k].z); cf_[4 * k + 3] = __uint_as_float(cfr[k].w);        \
          }                                                                                                \
          if constexpr (is_x3<T>::value) {   /* groups of eight: this lane's four values own one half of the hi piece and of the lo piece   \
                                                 (logical chunks 2g, 2g + 1 = this lane's and its neighbour's 16 bytes; both lanes read before they write) */ \
            const u32x4_t s_ = gn_rewrite16(T{}, *a_, cf_, p.gn_act, ((bmask >> (Q)) & 1u) != 0u);        \
            const int od_ = gchunk & 1, o_ = (DSTOFF) + jn_ * 1024 + lane * 16;                            \
            *reinterpret_cast<u32x2_t*>(smem + (o_ ^ (od_ << 4)) + 8 * od_) = u32x2_t{s_.x, s_.y};         \
            *reinterpret_cast<u32x2_t*>(smem + (o_ ^ (od_ << 4) ^ 16) + 8 * od_) = u32x2_t{s_.z, s_.w};    \
          } else                                                                                           \
          *a_ = gn_rewrite16(T{}, *a_, cf_, p.gn_act, ((bmask >> (Q)) & 1u) != 0u);                        \
        }                                                                                                  \
      }
      // behind the barrier of tap 0: the coefficients of the next slab (its halo is rewritten as it lands)
#undef K22_TAP_HOOK
#define K22_TAP_HOOK(N, TAP) K22_GN_HOOK_##N(TAP)
#define K22_GN_HOOK_0(TAP)
#define K22_GN_HOOK_1(TAP)
#define K22_GN_HOOK_2(TAP) if constexpr ((TAP) == 0) { if (more) K22_GN_COEF(sn); }
      // the pieces issued one tap ago (and the coefficients issued at tap 0) have had a whole tap to land: wait for everything
      // older than THIS tap's DMA, rewrite them, and have the stores complete before the next barrier
#define K22_GN_AFTER(TAP)                                                                                  \
      if constexpr ((TAP) >= 1 && (TAP) - 1 <= 9 - NBST) {                                                 \
        if (more) {                                                                                        \
          gn_wait<B_SLOTS + ((TAP) <= 9 - NBST ? APT : 0)>(cfr);                                           \
          _Pragma("unroll") for (int a_i = 0; a_i < APT; ++a_i) {                                          \
            constexpr int qr_ = ((TAP) >= 1 ? (TAP) - 1 : 0) * APT;                                        \
            K22_GN_REWRITE(qr_ + a_i, anext_off);                                                          \
          }                                                                                                \
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                               \
        }                                                                                                  \
      }
      // prologue: coefficients of the first slab, its whole halo, the weight tiles of taps 0 .. NBST-2; then the halo is rewritten
      K22_GN_COEF(s0);
#pragma unroll
      for (int q = 0; q < A_SLOTS; ++q) K22_GN_A(lw, NWL, q, s0, lds0);
#pragma unroll
      for (int t = 0; t < NBST - 1; ++t) K22_ISSUE_B(lw, NWL, t * p.Kc + s0 * BK, lds0 + 2 * A_BYTES + t * B_BYTES);
      gn_wait<(NBST - 1) * B_SLOTS>(cfr);
#pragma unroll
      for (int q = 0; q < A_SLOTS; ++q) K22_GN_REWRITE(q, 0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      K22_PRODUCER_LOOP(true, true, K22_GN_A, K22_GN_AFTER)
#undef K22_TAP_HOOK
#define K22_TAP_HOOK(N, TAP)
#undef K22_GN_A
#undef K22_GN_COEF
#undef K22_GN_REWRITE
#undef K22_GN_AFTER
    } else if (producer) {
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
      K22_PRODUCER_LOOP(DBG == 0, DBG != 1, K22_ISSUE_A, K22_PRODUCER_NOTHING)
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
#undef K22_PRODUCER_NOTHING
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
#ifdef K22_DEBUG_VARIANTS   // measurement-only forms of the pipelined kernel (wrong results), bf16 at BM = 256: DBG 1 = no LDS-DMA inside the tap loop, 2 = LDS-DMA issued but never waited for
    if constexpr (std::is_same<T, bf16_t>::value) {
      if (L.dbg == 1) return halo_with_depth<2, 4>(L.depth, [&](auto d) { return halo_run<conv3_halo_spec_kernel<T, 256, decltype(d)::value, true, 1>>(p, L, stream); });
      if (L.dbg == 2) return halo_with_depth<2, 4>(L.depth, [&](auto d) { return halo_run<conv3_halo_spec_kernel<T, 256, decltype(d)::value, true, 2>>(p, L, stream); });
    }
#endif
    // the 224-row tile: 16-bit types, pipelined form, no fused GroupNorm-apply (112 accumulators beside two sets of 7 + 1 fragments of 4
    // registers; the wider fragments of the other types do not fit).  conv3_halo_supported says the same; a launch that names it otherwise is refused.
    constexpr bool pipe224 = std::is_same<T, bf16_t>::value || std::is_same<T, f16_t>::value;
    if (L.bm == HALO_BM_STRIP && !(pipe224 && L.pipe && p.gn_coeff == nullptr))
      return k22_set_error(K22_EINVAL, "conv3_halo_spec: the 224-row tile is the pipelined 16-bit form only, without the fused GroupNorm-apply");
    if (!L.pipe) return halo_with_bm(L.bm, [&](auto bm) { return launch_spec_depth<T, decltype(bm)::value, false>(p, L, stream); });
    constexpr bool pipe256 = !std::is_same<T, x3_t>::value && !std::is_same<T, float>::value;
    return halo_with_bm<pipe256, pipe224>(L.bm, [&](auto bm) { return launch_spec_depth<T, decltype(bm)::value, true>(p, L, stream); });
  });
}
