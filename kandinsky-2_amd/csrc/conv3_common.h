// k22 - shared by the LDS-resident-halo convolution kernels (conv3_halo.hip: lock-step kernels; conv3_up2.hip; gemm8.hip; conv3_spec.hip:
// the producer / consumer specialised kernel): the LDS-DMA helper, the one definition
// of the 8-wave frame (loader offsets and issues), of the tap body and of the tap step, the common epilogue
// halo_tail, and the LDS budget and launch dispatch every launcher and kernel agrees on.  What these kernels share with the other conv / GEMM
// kernels - fragment loaders, counted vmcnt wait, block map, split-K range, accumulator zeroing, row vectors - is in common.h, the q/k/v
// scatter in kernels.h.
#pragma once
#include "kernels.h"
#include <stdlib.h>

namespace {

// LDS-DMA issued from inline asm: 16 bytes per lane from `g` to LDS byte address `lds_dst` (wave-uniform) + 16*lane.
// hipcc books a __builtin_amdgcn_global_load_lds as a FLAT access pending on BOTH counters, and because the counted
// vmcnt waits of this file are invisible to it, every later wait for a ds_read becomes lgkmcnt(0) - also for fragments
// read a whole MFMA group ago, with younger reads still in flight.  An asm statement is absent from its bookkeeping:
// the compiler then emits exact lgkmcnt(N) for the fragment reads; completion of the DMA is counted by hand anyway.
__device__ __forceinline__ void glds16_asm(const void* g, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(g), "s"(lds_dst) : "memory");
}

// the same for a WEIGHT piece.  K22_W_NT (measurement build): non-temporal hint - each weight byte is read by the few workgroups of one
// n-tile column, once (MI355X_MICROARCH.md "nt-weights": issued -> landed -18 % for read-once streams, -6 % end to end when every CU re-reads)
__device__ __forceinline__ void glds16w_asm(const void* g, unsigned lds_dst) {
#ifdef K22_W_NT
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(g), "s"(lds_dst) : "memory");
#else
  glds16_asm(g, lds_dst);
#endif
}

constexpr int HALO_BN = 128;
constexpr int HALO_NW = 8;        // waves per workgroup

// Each iteration issues [weight tile NBST-1 taps ahead (2 loads)] THEN [the halo pieces of this tap]: the halo piece is the
// youngest entry of the VMEM queue, so the counted wait for the weight tile can leave it in flight — it gets two
// taps (~1.6 us at 96x96) to come back from the Infinity Cache / HBM instead of one.  Taps 0 .. TAPS-NBST of a slab issue halo
// pieces; this is the number of such taps among the NBST-1 iterations before tap T, i.e. younger than the weight tile tap T
// needs; taps are unrolled, so it is a compile-time constant.
template <int TAPS, int NBST> constexpr int halo_count(int t) {
  int c = 0;
  for (int k = 1; k <= NBST - 1; ++k) {
    const int u = t - k;
    if (u >= 0 && u <= TAPS - NBST) ++c;
  }
  return c;
}
// (row, column) of tap t in its filter: 3x3, or the 2x2 filter of one up-sampling phase
template <int TAPS> constexpr int halo_tap_dy(int t) { return TAPS == 9 ? t / 3 : t >> 1; }
template <int TAPS> constexpr int halo_tap_dx(int t) { return TAPS == 9 ? t % 3 : t & 1; }

// ---- the frame: 512 threads = 8 waves own one BM x 128 tile of a (gx m-tiles) x (gy n-tiles) x splitk grid -------------------
// LDS byte address of the dynamic shared segment (wave-uniform), for the asm LDS-DMA path
__device__ __forceinline__ unsigned halo_lds_base(char* smem) {
  return __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)smem);
}
// one 16-byte-per-lane LDS-DMA: GASM = from inline asm (glds16_asm above; WEIGHT: glds16w_asm) to LDS byte address lds_addr, else the
// compiler's builtin to the same place given as a pointer
template <bool GASM, bool WEIGHT> __device__ __forceinline__ void halo_dma16(const void* g, unsigned lds_addr, char* lds_ptr) {
  if constexpr (!GASM)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)lds_ptr, 16, 0, 0);
  else if constexpr (WEIGHT) glds16w_asm(g, __builtin_amdgcn_readfirstlane(lds_addr));
  else glds16_asm(g, __builtin_amdgcn_readfirstlane(lds_addr));
}

}  // namespace

// The macros below are the one text of the loaders, the tap body and the tap step of the kernels on this frame.  They are macros, not
// functions: hipcc's schedule of the tap loop (address arithmetic, lgkmcnt waits) moves when the same text goes through a function
// template, and does not when it is expanded in place (profiles/halo_frame_device_code.txt).  Names they take from the kernel:
// smem, lds0 (halo_lds_base), GASM (constexpr bool, halo_dma16), h, KSTEPS, MI, NI, acc, and what each one lists.
//
// Row-tile LDS-DMA offsets (weight tiles; the A tile of the plain GEMM): loader wave LW of NWL issues rows [8 * (LW + NWL * i), + 8) in its
// slot i; lane -> (row, 16-byte position lane % 8).  OFF[i] = ELEM, the element offset of row n = FIRST + row clamped to LAST (an
// expression of n), plus the chunk the XOR swizzle of common.h assigns to this lane.
#define K22_ROW_OFFSETS(OFF, SLOTS, LW, NWL, FIRST, LAST, ELEM)                                            \
  _Pragma("unroll") for (int i = 0; i < (SLOTS); ++i) {                                                    \
    const int row = 8 * ((LW) + (NWL) * i) + (lane >> 3);                                                  \
    int n = (FIRST) + row;                                                                                 \
    if (n > (LAST)) n = (LAST);                                                                            \
    const int chunk = (lane & 7) ^ ((row >> 1) & 7);                                                       \
    OFF[i] = (ELEM) + chunk * EPC;                                                                         \
  }
// Halo-piece LDS-DMA offsets: piece j (RP rows of 1024 / RP bytes: 8 x 128, or 16 x 64 in conv3_halo3_kernel) of the NP_ of a halo buffer is
// issued by loader wave j % NWL in its slot j / NWL; lane -> (row RP * j + lane / (64 / RP), position lane % (64 / RP)).  FIRST = plane
// position of the LDS image's row 0; PR_MAX = last position of the plane.
#define K22_PIECE_OFFSETS(AOFF, SLOTS, LW, NWL, FIRST, NP_, RP)                                            \
  _Pragma("unroll") for (int q = 0; q < (SLOTS); ++q) {                                                    \
    int j = q * (NWL) + (LW);                                                                              \
    if (j > (NP_) - 1) j = (NP_) - 1;  /* surplus slots re-load the last piece (same bytes, same place): uniform counting */ \
    const int hr = (RP) * j + (lane >> ((RP) == 8 ? 3 : 2));                                               \
    int pr = (FIRST) + hr;                                                                                 \
    if (pr > PR_MAX) pr = PR_MAX;                                                                          \
    const int chunk = (lane & (64 / (RP) - 1)) ^ ((hr >> ((RP) == 8 ? 1 : 2)) & (64 / (RP) - 1));          \
    AOFF[q] = pr * p.Kc + chunk * EPC;                                                                     \
  }
// An LDS location (the DST of the macros below) is a pointer into smem unless a kernel says otherwise: the producer waves of
// conv3_halo_spec_kernel name theirs by LDS byte address (lds0 + offset) and redefine these two.  (Both spellings of one place, and both
// kept: hipcc's output follows the spelling.)
#define K22_LDS_ADDR(AT) (lds0 + (unsigned)((AT) - smem))
#define K22_LDS_PTR(AT) (AT)
// Halo piece of slot Q of loader wave LW of NWL, K slab SLAB, into the halo buffer at LDS location DST.  Needs Aimg, aoff, NP, BK.
#define K22_ISSUE_A(LW, NWL, Q, SLAB, DST)                                                                 \
  {                                                                                                        \
    int j_ = (Q) * (NWL) + (LW);                                                                           \
    if (j_ > NP - 1) j_ = NP - 1;                                                                          \
    halo_dma16<GASM, false>(Aimg + aoff[Q] + (SLAB) * BK, K22_LDS_ADDR(DST) + j_ * 1024, K22_LDS_PTR(DST) + j_ * 1024); \
  }
// Row tile (K22_ROW_OFFSETS: OFF[SLOTS]) of SRC at element offset KOFS, for a loader wave of NWL whose slot 0 lands at LDS byte address
// DADDR = pointer DPTR (the wave's 1 KB of the tile; DPTR is read by the compiler-issued form only).
#define K22_ISSUE_ROWS(WEIGHT, SRC, OFF, SLOTS, NWL, KOFS, DADDR, DPTR)                                    \
  _Pragma("unroll") for (int i = 0; i < (SLOTS); ++i)                                                      \
      halo_dma16<GASM, WEIGHT>((SRC) + OFF[i] + (KOFS), (DADDR) + i * (NWL) * 1024, (DPTR) + i * (NWL) * 1024);
// The weight tile (Wp, boff) at element offset KOFS into the tile at LDS location DST, by loader wave LW of NWL
#define K22_ISSUE_B(LW, NWL, KOFS, DST)                                                                    \
  {                                                                                                        \
    const int kofs_ = (KOFS);                                                                              \
    const auto dst_ = (DST) + (LW) * 1024;                                                                 \
    K22_ISSUE_ROWS(true, Wp, boff, B_SLOTS, NWL, kofs_, K22_LDS_ADDR(dst_), K22_LDS_PTR(dst_))             \
  }

// acc += B . A over the MI x NI atoms of a wave
#define K22_MMA_ALL(B, A)                                                                                  \
  _Pragma("unroll") for (int mi = 0; mi < MI; ++mi)                                                        \
    _Pragma("unroll") for (int ni = 0; ni < NI; ++ni) mma_atom(acc[mi][ni], B[ni], A[mi]);
// No fragment read of a tap's (slab's) LDS slot may be in flight when the slot is refilled after the next barrier: right behind barrier
// TAP + 1 the loaders refill the weight slot THIS tap read, whatever the ring depth (and behind a slab's last tap the halo buffer of the
// slab before).  Nothing is left to the DMA's latency.  (The MFMAs that use the fragments can still sink below the barrier: registers only.)
#define K22_READS_DONE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
// The plain tap body: per k-step, the fragments (types FA / FB; activation rows AROW with swizzle key ASW as expressions of mi, loaded by
// LDA; weight rows BROW of ni with key BSW), then MI x NI atoms; hipcc schedules it.
#define K22_TAP_PLAIN(FA, FB, LDA, AROW, ASW, BROW, BSW)                                                   \
  _Pragma("unroll") for (int ks = 0; ks < KSTEPS; ++ks) {                                                  \
    FA a[MI];                                                                                              \
    FB b[NI];                                                                                              \
    _Pragma("unroll") for (int mi = 0; mi < MI; ++mi) LDA(a[mi], AROW, ASW, ks, h);                        \
    _Pragma("unroll") for (int ni = 0; ni < NI; ++ni) ld_frag_at(b[ni], BROW, BSW, ks, h);                 \
    K22_MMA_ALL(b, a)                                                                                      \
  }
// The explicit two-set fragment pipeline across the per-tap barrier.  The fragments of k-step ks + 1 are read from LDS BEFORE the MFMAs of
// k-step ks are issued (two register sets: ca / cb here, pa / pb in the kernel - zero before the first tap, a no-op group), and the last
// k-step of a tap is multiplied after the NEXT tap's barrier (K22_MMA_ALL(pb, pa) behind the loop for the last one).  MID stands between a
// read group and the MFMA group of the set read before it, END behind that MFMA group: sched_barrier(0) twice where every wave also loads
// (K22_PIPE_LOCKSTEP), nothing and the read-behind-every-MFMA interleave in the consumer waves (K22_PIPE_INTERLEAVED).
#define K22_TAP_PIPE(...) K22_TAP_PIPE_(__VA_ARGS__)
#define K22_TAP_PIPE_(FA, FB, AROW, ASW, BROW, BSW, MID, END)                                              \
  {                                                                                                        \
    FA ca[MI];                                                                                             \
    FB cb[NI];                                                                                             \
    _Pragma("unroll") for (int ks = 0; ks < KSTEPS; ks += 2) {                                             \
      _Pragma("unroll") for (int mi = 0; mi < MI; ++mi) ld_frag_at(ca[mi], AROW, ASW, ks, h);              \
      _Pragma("unroll") for (int ni = 0; ni < NI; ++ni) ld_frag_at(cb[ni], BROW, BSW, ks, h);              \
      MID;                                                                                                 \
      K22_MMA_ALL(pb, pa)                                                                                  \
      END;                                                                                                 \
      _Pragma("unroll") for (int mi = 0; mi < MI; ++mi) ld_frag_at(pa[mi], AROW, ASW, ks + 1, h);          \
      _Pragma("unroll") for (int ni = 0; ni < NI; ++ni) ld_frag_at(pb[ni], BROW, BSW, ks + 1, h);          \
      MID;                                                                                                 \
      K22_MMA_ALL(cb, ca)                                                                                  \
      END;                                                                                                 \
    }                                                                                                      \
  }
#define K22_PIPE_LOCKSTEP __builtin_amdgcn_sched_barrier(0), __builtin_amdgcn_sched_barrier(0)
// One block of the consumers' pipeline = NRD fragment reads (of the NEXT group) + NMF MFMAs (of the group read one block ago), which are
// independent of each other: one read is scheduled behind every MPR MFMAs (0x008 = MFMA, 0x100 = DS read), so that each ds_read_b128
// issues under the 32 cycles the MFMA before it occupies the pipe.  Needs NRD, NMF, MPR (halo_pipe_reads).
#define K22_INTERLEAVE()                                                                                   \
  {                                                                                                        \
    _Pragma("unroll") for (int i_ = 0; i_ < NRD; ++i_) {                                                   \
      __builtin_amdgcn_sched_group_barrier(0x008, MPR, 0);                                                 \
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                                   \
    }                                                                                                      \
    if constexpr (NMF - MPR * NRD > 0) __builtin_amdgcn_sched_group_barrier(0x008, NMF - MPR * NRD, 0);    \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
  }
#define K22_PIPE_INTERLEAVED (void)0, K22_INTERLEAVE()
// The same for a block with one read MORE than it has MFMAs (NRD = NMF + 1: the 224-row tile's 7 + 1 reads for 7 MFMAs per k-step, where
// MPR is 0): the surplus read in front, then one read behind every MFMA.
#define K22_INTERLEAVE_LEAD()                                                                              \
  {                                                                                                        \
    static_assert(NRD == NMF + 1, "one read in front, one behind every MFMA");                             \
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < NMF; ++i_) {                                                   \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                   \
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                                   \
    }                                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
  }

// M(tap, ...) for every tap of the filter, with literal tap numbers: the vmcnt immediates and the (slab, tap) of the prefetched weight
// tile are compile-time functions of the tap
#define K22_TAPS_9(M, ...) M(0, __VA_ARGS__) M(1, __VA_ARGS__) M(2, __VA_ARGS__) M(3, __VA_ARGS__) M(4, __VA_ARGS__) M(5, __VA_ARGS__) M(6, __VA_ARGS__) M(7, __VA_ARGS__) M(8, __VA_ARGS__)
#define K22_TAPS_4(M, ...) M(0, __VA_ARGS__) M(1, __VA_ARGS__) M(2, __VA_ARGS__) M(3, __VA_ARGS__)
// The loaders' half of a tap, for loader wave LW of NWL in a TAPS-tap filter (weights [n][tap][Kc]) with an NBST-deep weight ring behind
// the two halo buffers: the counted vmcnt wait for this tap's weight tile (VMEM queue of a wave per tap: [weight tile NBST-1 taps ahead,
// B_SLOTS loads] then [PPT halo pieces, taps 0 .. TAPS-NBST]: at most the B_SLOTS * (NBST-2) younger weight loads and the halo pieces issued
// since stay in flight; the last halo piece of a slab is followed by the weight loads of NBST-1 taps, so at tap 0 of the next slab it is
// older than everything the wait leaves in flight), the ONE raw barrier of the tap, then the weight tile NBST-1 taps ahead into ring slot
// `fill` and the next PPT pieces of the next slab's halo (K22_ISSUE_A) into the halo buffer at LDS location ANEXT; RING = the LDS
// location of the weight ring (pasted as written: its sum with the slot offset is one expression).
// Needs s, sn, fill, B_BYTES, B_SLOTS, NBST, p.
#define K22_TAP_FRONT(TAP, TAPS, LW, NWL, PPT, ANEXT, RING)                                                \
  wait_vmcnt<B_SLOTS * (NBST - 2) + (PPT) * halo_count<TAPS, NBST>(TAP)>();                                \
  raw_barrier();                                                                                           \
  {                                                                                                        \
    constexpr int ta_ = ((TAP) + NBST - 1) % (TAPS);                                                       \
    const int sa_ = ((TAP) + NBST - 1 >= (TAPS)) ? sn : s;                                                 \
    K22_ISSUE_B(LW, NWL, ta_ * p.Kc + sa_ * BK, RING + fill * B_BYTES);                                    \
    if constexpr ((TAP) <= (TAPS) - NBST) {                                                                \
      _Pragma("unroll") for (int a_ = 0; a_ < (PPT); ++a_) {                                               \
        constexpr int qb_ = ((TAP) <= (TAPS) - NBST ? (TAP) : 0) * (PPT);                                  \
        K22_ISSUE_A(LW, NWL, qb_ + a_, sn, ANEXT);                                                       \
      }                                                                                                    \
    }                                                                                                      \
  }
// The multiplying half of a tap: the fragment rows of the tap (A row = abase + mi*32 + tap shift in the current halo buffer Acur, B row =
// brow[ni] in ring slot `cur`), the body (K22_TAP_PLAIN / K22_TAP_PIPE over arow, asw, Bcur), the read drain, the rotation of `cur`.
#define K22_TAP_COMPUTE(TAP, TAPS, ...)                                                                    \
  const char* Bcur = Bst + cur * B_BYTES;                                                                  \
  constexpr int dy_ = halo_tap_dy<TAPS>(TAP), dx_ = halo_tap_dx<TAPS>(TAP);                                \
  const int shift = dy_ * W2 + dx_;                                                                        \
  const char* arow[MI];                                                                                    \
  int asw[MI];                                                                                             \
  _Pragma("unroll") for (int mi = 0; mi < MI; ++mi) {                                                      \
    const int ar = abase + mi * 32 + shift;                                                                \
    arow[mi] = Acur + ar * 128;                                                                            \
    asw[mi] = (ar >> 1) & 7;                                                                               \
  }                                                                                                        \
  __VA_ARGS__                                                                                              \
  K22_READS_DONE();                                                                                        \
  cur = (cur + 1 == NBST) ? 0 : cur + 1;
// One tap of a lock-step kernel: every wave loads, then multiplies
#define K22_LOCKSTEP_TAP(TAP, TAPS, PPT, ...)                                                              \
  {                                                                                                        \
    K22_TAP_FRONT(TAP, TAPS, wave, NW, PPT, Anext, Bst)                                                    \
    K22_TAP_COMPUTE(TAP, TAPS, __VA_ARGS__)                                                                \
    fill = (fill + 1 == NBST) ? 0 : fill + 1;                                                              \
  }
// The K loop of a lock-step kernel over slabs [s0, s1): prologue = the whole halo of the first slab (A_SLOTS pieces per wave), then the
// weight tiles of taps 0 .. NBST-2; then TAPS taps per slab, the halo double-buffered across slabs.  Every wave issues LDS-DMA.
#define K22_LOCKSTEP_LOOP(TAPS, A_SLOTS, PPT, BODY)                                                        \
  if (s0 < s1) {                                                                                           \
    _Pragma("unroll") for (int q = 0; q < (A_SLOTS); ++q) K22_ISSUE_A(wave, NW, q, s0, smem);              \
    _Pragma("unroll") for (int t = 0; t < NBST - 1; ++t) K22_ISSUE_B(wave, NW, t * p.Kc + s0 * BK, Bst + t * B_BYTES); \
    int cur = 0;               /* ring slot of the current tap's weights */                                \
    int fill = NBST - 1;       /* ring slot the tile NBST-1 taps ahead goes into */                        \
    for (int s = s0; s < s1; ++s) {                                                                        \
      char* const Acur = smem + ((s - s0) & 1) * A_BYTES;                                                  \
      char* const Anext = smem + (((s - s0) & 1) ^ 1) * A_BYTES;                                           \
      const int sn = s + 1 < s1 ? s + 1 : s1 - 1;  /* past-the-end loads re-read the last slab (uniform counting) */ \
      K22_TAPS_##TAPS(K22_LOCKSTEP_TAP, TAPS, PPT, BODY)                                                   \
    }                                                                                                      \
  }

namespace {
// fragment reads of one block of the interleaved pipeline (x2: the activation fragment is ONE read, hi piece only)
template <typename T, int MI, int NI> constexpr int halo_pipe_reads() { return is_x2<T>::value ? MI + 2 * NI : (MI + NI) * FragCost<T>::READS; }
// How the waves that hold accumulators share the BM x 128 tile: WM x WN waves of (BM / WM) x (128 / WN) each.  Lock-step kernels: all eight,
// 4 x 2.  conv3_halo_spec_kernel: its four consumers, 2 x 2 - except the 224-row tile (7 m-blocks of 32 rows do not halve): 1 x 4, one
// 32-column strip of all seven m-blocks per wave.
constexpr int HALO_BM_STRIP = 224;
template <int BM, bool SPEC> constexpr int halo_wm() { return !SPEC ? 4 : (BM == HALO_BM_STRIP ? 1 : 2); }
template <int BM, bool SPEC> constexpr int halo_wn() { return (SPEC && BM == HALO_BM_STRIP) ? 4 : 2; }
template <int BM, bool SPEC> constexpr int halo_mi() { return BM / (halo_wm<BM, SPEC>() * 32); }
template <int BM, bool SPEC> constexpr int halo_ni() { return HALO_BN / (halo_wn<BM, SPEC>() * 32); }
// stages of the fused skip's LDS-DMA ring (kernel and LDS budget): 3 x 48 KB (44 KB at 224 rows) / 4 x 32 KB of the 160 KB
constexpr int halo_skip_stages(int bm) { return bm > 128 ? 3 : 4; }
}  // namespace

// Everything after the 3x3 K loop, shared by the halo kernels: optional fused 1x1 skip connection (a plain-GEMM K loop
// on 128-byte rows), then the epilogue through LDS (bias, residual, one rounding, 16-byte stores, GroupNorm partials).
// PLAIN = false: rows are positions v of the padded plane (3x3 convolution); PLAIN = true: rows are the pixels
// v < H*W of image `img` themselves (gemm8_kernel), and the qkv-projection output mode is available.
// SPEC = true (conv3_halo_spec_kernel): only waves 0-3 hold accumulators, 2 x 2 over the tile with (BM/2) x 64 each (BM = 224: 1 x 4,
// 224 x 32 each - halo_wm / halo_wn); waves 4-7 were the producers of the main loop.  All eight waves issue the skip loop's LDS-DMA and run the store / statistics epilogue.
// UP2 = true (conv3_up2_kernel, conv3_up2.hip): rows are positions v of the LOW-resolution padded plane and row (y, x) of phase ph = 2*py + px
// is stored at (2y + py, 2x + px) of the unpadded 2H x 2W output; p.M counts the output's rows; bx = the statistics row of this tile.
template <typename T, int BM, bool PLAIN = false, bool SPEC = false, bool UP2 = false>
__device__ __forceinline__ void halo_tail(const IgemmParams& p, f32x16_t (&acc)[halo_mi<BM, SPEC>()][halo_ni<BM, SPEC>()], char* smem, int bx, int bz, int img, int v0, int n0,
                                          int ph = 0) {
  using TR = TT<T>;
  constexpr int BK = TR::BK, EPC = TR::EPC, KSTEPS = TR::KSTEPS;
  constexpr int BN = HALO_BN, NW = HALO_NW, WM = halo_wm<BM, SPEC>(), WN = halo_wn<BM, SPEC>();
  constexpr int MI = BM / (WM * 32), NI = BN / (WN * 32);
  constexpr int B_SLOTS = BN / 8 / NW;
  constexpr int B_BYTES = BN * 128;
  constexpr int TS = BN * 4 + 16;       // epilogue tile row stride (bytes): conflict-free float4 writes
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = WN == 4 ? 0 : wave >> 1, wn = WN == 4 ? wave & 3 : wave & 1;
  const bool cw = !SPEC || wave < 4;      // this wave holds accumulators (wave-uniform)
  const int h = lane >> 5, l31 = lane & 31;
  const int W2 = PLAIN ? 1 : p.W + 2;
  const int VR = PLAIN ? (p.H > 0 ? p.H * p.W : p.M) : p.H * W2;
  const int abase = wm * (BM / WM) + l31;
  int brow[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) brow[ni] = (wn * (BN / WN) + ni * 32 + l31) * 128;
  const int bsw = (l31 >> 1) & 7;

  // ---- fused 1x1 skip connection: acc += X[tile pixels][SK] . Ws[n][SK]^T, 3- / 4-stage LDS-DMA ring ----------
  if (p.S0 != nullptr) {
    const int SK = p.SK0 + p.SK1;
    const int nss = SK / BK;
    const int sp = p.splitk > 1 ? p.splitk : 1;
    const int q0 = nss * bz / sp, q1 = nss * (bz + 1) / sp;
    if (q0 < q1) {
      constexpr int SA_SLOTS = (BM / 8 + NW - 1) / NW;  // input-tile LDS-DMA instructions per wave per slab
      constexpr bool SA_RAGGED = BM / 8 % NW != 0;      // 224 rows: 28 pieces in 4 x 8 slots - the surplus slots re-load the last piece (same bytes, same place: uniform counting)
      constexpr int SBUF = BM * 128 + B_BYTES;
      wait_vmcnt<0>();
      __syncthreads();                                   // main-loop buffers are free
      int spix[SA_SLOTS], schunk[SA_SLOTS];
#pragma unroll
      for (int i = 0; i < SA_SLOTS; ++i) {
        int piece = wave + NW * i;
        if constexpr (SA_RAGGED) { if (piece > BM / 8 - 1) piece = BM / 8 - 1; }
        const int row = 8 * piece + (lane >> 3);
        int v = v0 + row;
        if (v > VR - 1) v = VR - 1;
        const int y = v / W2;
        int x = v - y * W2;
        if (x > p.W - 1) x = p.W - 1;                    // junk columns read a valid pixel; their rows are dropped
        spix[i] = (img * p.H + y) * p.W + x;
        schunk[i] = ((lane & 7) ^ ((row >> 1) & 7)) * EPC;
      }
      int wsoff[B_SLOTS];
      K22_ROW_OFFSETS(wsoff, B_SLOTS, wave, NW, n0, p.Npad - 1, n * SK)
      const T* __restrict__ X0 = reinterpret_cast<const T*>(p.S0);
      const T* __restrict__ X1 = reinterpret_cast<const T*>(p.S1);
      const T* __restrict__ Ws = reinterpret_cast<const T*>(p.Ws);
      // NSK-deep LDS-DMA ring with a COUNTED vmcnt (round 5).  The 2-stage form this replaces waited vmcnt(0) at every slab: one DMA round
      // trip (1-2 us from L2 / HBM) per 0.25-0.5 us of MFMA work, i.e. +13...25 us on every convolution with a fused skip - the reason the
      // tile table gave seven of the 96x96 convolutions to the lock-step kernel.  Now NSK - 1 slabs are in flight across the one raw
      // barrier per slab; the DMA is issued from inline asm (glds16_asm) so that hipcc neither drains it nor waits lgkmcnt(0) for it.
      // Slot reuse: iteration q refills the stage iteration q - 1 read, after the barrier every wave reaches only behind its
      // lgkmcnt(0); past-the-end issues re-load the last slab (uniform counting), drained by the vmcnt(0) below the loop.
      constexpr int NSK = halo_skip_stages(BM);
      constexpr int SCH = SA_SLOTS + B_SLOTS;              // LDS-DMA instructions per wave per slab
      constexpr bool GASM = true;
      const unsigned lds0 = halo_lds_base(smem);
#define K22_ISSUE_SKIP(Q, BUFI)                                                                            \
      {                                                                                                    \
        int q_ = (Q);                                                                                      \
        if (q_ > q1 - 1) q_ = q1 - 1;                                                                      \
        const int k0_ = q_ * BK;                                                                           \
        const bool second_ = k0_ >= p.SK0;                                                                 \
        const T* xs_ = second_ ? X1 : X0;                                                                  \
        const int ldx_ = second_ ? p.SK1 : p.SK0;                                                          \
        const int kk_ = second_ ? k0_ - p.SK0 : k0_;                                                       \
        const unsigned dA_ = lds0 + (BUFI) * SBUF + wave * 1024;                                           \
        _Pragma("unroll") for (int i = 0; i < SA_SLOTS; ++i) {                                             \
          if constexpr (SA_RAGGED) {   /* the destination is clamped with the source: behind the input tile stands the weight stage */ \
            const int pc_ = wave + NW * i < BM / 8 - 1 ? wave + NW * i : BM / 8 - 1;                       \
            glds16_asm(xs_ + (int64_t)spix[i] * ldx_ + kk_ + schunk[i], __builtin_amdgcn_readfirstlane(lds0 + (BUFI) * SBUF + pc_ * 1024)); \
          } else                                                                                           \
            glds16_asm(xs_ + (int64_t)spix[i] * ldx_ + kk_ + schunk[i], __builtin_amdgcn_readfirstlane(dA_ + i * NW * 1024)); \
        }                                                                                                  \
        K22_ISSUE_ROWS(true, Ws, wsoff, B_SLOTS, NW, k0_, dA_ + BM * 128, smem + (dA_ - lds0) + BM * 128)  \
      }
#pragma unroll
      for (int t = 0; t < NSK - 1; ++t) K22_ISSUE_SKIP(q0 + t, t);
      int buf = 0, fill = NSK - 1;
      for (int q = q0; q < q1; ++q) {
        wait_vmcnt<(NSK - 2) * SCH>();
        raw_barrier();
        K22_ISSUE_SKIP(q + NSK - 1, fill);
        const char* sA = smem + buf * SBUF;
        const char* sB = sA + BM * 128;
        if (cw) {
        // (asymmetric split: the skip input is the un-normalised residual stream - its operand rounding alone costs as much as that of
        // every GroupNorm output together, tests/golden/drift_ablation_x2.json - so this K loop keeps all three MFMAs)
        using TSK = typename SkipT<T>::type;
        K22_TAP_PLAIN(Frag<TSK>, Frag<TSK>, (ld_frag_at_a<true, TSK>), sA + (abase + mi * 32) * 128, bsw, sB + brow[ni], bsw)   // S0 / S1: plain T rows
        }
        K22_READS_DONE();
        buf = (buf + 1 == NSK) ? 0 : buf + 1;
        fill = (fill + 1 == NSK) ? 0 : fill + 1;
      }
#undef K22_ISSUE_SKIP
    }
  }
  wait_vmcnt<0>();
  __syncthreads();  // every wave is done with the operand buffers: the LDS becomes the fp32 output tile

  // ---- epilogue 1: accumulators -> LDS tile [BM][BN] fp32 (lane = pixel, 4 consecutive channels per quad) ----
  if (cw)
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int row = wm * (BM / WM) + mi * 32 + l31;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = wn * (BN / WN) + ni * 32 + 8 * j + 4 * h;
        *reinterpret_cast<float4*>(smem + row * TS + col * 4) =
            make_float4(acc_unscale<T>(acc[mi][ni][4 * j]), acc_unscale<T>(acc[mi][ni][4 * j + 1]), acc_unscale<T>(acc[mi][ni][4 * j + 2]),
                        acc_unscale<T>(acc[mi][ni][4 * j + 3]));
      }
  }
  __syncthreads();

  // ---- qkv projection, n-tile inside v (an n-tile never straddles q / k / v): V^T_all wants the tile transposed.
  // lane = token (consecutive lanes -> consecutive addresses of one V^T row), 4 channels per LDS read
  if constexpr (PLAIN) {
    if (p.out_mode == IG_OUT_QKV && n0 >= 2 * (p.N / 3)) {
      const int C = p.N / 3, heads = C >> 6;
      constexpr int CPG = BN / (512 / BM);   // channels per thread group
      const int r = tid % BM, cg = tid / BM;
      const int v = v0 + r;
      if (v < VR) {
#pragma unroll 4
        for (int c4 = 0; c4 < CPG; c4 += 4) {
          const int col = cg * CPG + c4, n = n0 + col;
          if (n >= p.N) break;
          const float4 t = *reinterpret_cast<const float4*>(smem + r * TS + col * 4);
          float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
          if (p.bias != nullptr) b = *reinterpret_cast<const float4*>(p.bias + n);
          const int c = n - 2 * C, head = c >> 6, d = c & 63;
          T* vt = reinterpret_cast<T*>(p.vtall) + ((int64_t)(img * heads + head) * 64 + d) * p.att_Tkp + p.att_S + v;
          vt[0] = from_f32<T>(t.x + b.x);
          vt[(int64_t)p.att_Tkp] = from_f32<T>(t.y + b.y);
          vt[(int64_t)2 * p.att_Tkp] = from_f32<T>(t.z + b.z);
          vt[(int64_t)3 * p.att_Tkp] = from_f32<T>(t.w + b.w);
        }
      }
      return;
    }
  }

  // ---- epilogue 2: thread = 8 channels x RPT consecutive rows -------------------------------------------
  constexpr int SEGS = BN / 8;            // 16 column segments
  constexpr int RGS = 512 / SEGS;         // 32 row groups
  constexpr int RPT = BM / RGS;           // rows per thread
  const int cs = tid % SEGS, rg = tid / SEGS;
  const int n = n0 + cs * 8;
  const bool n_ok = n < p.N;              // N % 8 == 0 (checked on the host)
  float bias8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bias8[e] = 0.f;
  const bool finish = (p.splitk <= 1);
  if (finish && n_ok && p.bias != nullptr) {
    const float4 b0 = *reinterpret_cast<const float4*>(p.bias + n), b1 = *reinterpret_cast<const float4*>(p.bias + n + 4);
    bias8[0] = b0.x; bias8[1] = b0.y; bias8[2] = b0.z; bias8[3] = b0.w;
    bias8[4] = b1.x; bias8[5] = b1.y; bias8[6] = b1.z; bias8[7] = b1.w;
  }
  if (finish && n_ok && p.bias2 != nullptr) {
    const float4 b0 = *reinterpret_cast<const float4*>(p.bias2 + n), b1 = *reinterpret_cast<const float4*>(p.bias2 + n + 4);
    bias8[0] += b0.x; bias8[1] += b0.y; bias8[2] += b0.z; bias8[3] += b0.w;
    bias8[4] += b1.x; bias8[5] += b1.y; bias8[6] += b1.z; bias8[7] += b1.w;
  }
  const T* __restrict__ res = reinterpret_cast<const T*>(p.residual);
  float* part = finish ? nullptr : p.partial + (int64_t)bz * p.M * p.N;
  float ssum[8], ssq[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { ssum[e] = 0.f; ssq[e] = 0.f; }
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const int row = rg * RPT + k;
    const int v = v0 + row;
    int64_t m;
    if constexpr (PLAIN) {
      if (!n_ok || v >= VR) continue;
      m = (int64_t)img * VR + v;
    } else {
      const int y = v / W2, x = v - y * W2;
      if (!n_ok || v >= VR || x >= p.W) continue;
      if constexpr (UP2) m = ((int64_t)img * 2 * p.H + 2 * y + (ph >> 1)) * (2 * p.W) + 2 * x + (ph & 1);
      else m = ((int64_t)img * p.H + y) * p.W + x;
    }
    const float4 t0 = *reinterpret_cast<const float4*>(smem + row * TS + cs * 32);
    const float4 t1 = *reinterpret_cast<const float4*>(smem + row * TS + cs * 32 + 16);
    float val[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
    if (!finish) {
      *reinterpret_cast<float4*>(part + m * p.N + n) = t0;
      *reinterpret_cast<float4*>(part + m * p.N + n + 4) = t1;
      continue;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) val[e] += bias8[e];
    if (res != nullptr) {
      float rv[8];
      load_row_f32<T, 8>(res + m * p.ldr + n, rv);
#pragma unroll
      for (int e = 0; e < 8; ++e) val[e] += rv[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) val[e] = apply_act(val[e], p.act);
    if (PLAIN && p.out_mode == IG_OUT_QKV) {
      K22_QKV_SCATTER(T, 8, val, m, img, v, n)
      continue;
    }
    if (p.out_mode == IG_OUT_ROWMAJOR) store_row<T, 8>(reinterpret_cast<T*>(p.out) + m * p.ldo + n, val);
    else store_row<float, 8>(reinterpret_cast<float*>(p.out) + m * p.ldo + n, val);
    if (p.stats != nullptr) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float sv = (p.out_mode == IG_OUT_ROWMAJOR) ? stored<T>(val[e]) : val[e];
        ssum[e] += sv;
        ssq[e] += sv * sv;
      }
    }
  }
  if (!finish || p.stats == nullptr) return;

  // ---- epilogue 3: per-channel (sum, sumsq) of this tile's stored values, fixed-order reduction ---------
  __syncthreads();  // tile fully consumed
  float* red = reinterpret_cast<float*>(smem);  // [RGS][BN][2]
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    *reinterpret_cast<float2*>(red + ((rg * BN) + cs * 8 + e) * 2) = make_float2(ssum[e], ssq[e]);
  }
  __syncthreads();
  if (tid < BN * 2) {
    const int ch = tid >> 1, which = tid & 1;
    float a = 0.f;
#pragma unroll 8
    for (int r = 0; r < RGS; ++r) a += red[((r * BN) + ch) * 2 + which];
    if (n0 + ch < p.N) p.stats[((int64_t)bx * p.N + n0 + ch) * 2 + which] = a;
  }
}

// ---- host side ---------------------------------------------------------------------------------
constexpr int UP2_ASLOTS = 6;   // conv3_up2_kernel: halo LDS-DMA slots per wave per slab (48 pieces = 384 rows)

// rows of the LDS halo image of a BM tile, whole 8-row pieces: taps == 9 (3x3): BM + 2*(W+2) + 2; taps == 4 (one 2x2 phase): BM + (W+2) + 1
inline int halo_rows(const IgemmParams& p, int bm, int taps) {
  const int r = taps == 9 ? 2 : 1;
  return (bm + r * (p.W + 2) + r + 7) & ~7;
}
// m-tiles per image: BM consecutive positions of the H x (W+2) plane each, whatever the filter
inline int halo_tiles_per_image(const IgemmParams& p, int bm) { return (p.H * (p.W + 2) + bm - 1) / bm; }

// LDS budget of a kernel on the frame: its main loop, or what halo_tail needs behind it - the fp32 epilogue tile, the statistics reduction,
// the NSK stages of the fused skip's ring
inline size_t halo_lds_budget(int bm, bool skip, size_t main_loop) {
  const size_t epi = (size_t)bm * (HALO_BN * 4 + 16);
  const size_t red = (size_t)32 * HALO_BN * 2 * 4;
  const size_t sk = skip ? (size_t)halo_skip_stages(bm) * (bm * 128 + HALO_BN * 128) : 0;
  size_t m = main_loop > epi ? main_loop : epi;
  m = m > sk ? m : sk;
  return m > red ? m : red;
}
// 128-byte-row kernels: two halo buffers + an nbst-deep weight ring.  The four-phase problems have no fused skip.
inline size_t halo_smem_bytes(const IgemmParams& p, int bm, int nbst, int taps = 9) {
  const size_t main_loop = (size_t)2 * halo_rows(p, bm, taps) * 128 + (size_t)nbst * HALO_BN * 128;
  return halo_lds_budget(bm, taps == 9 && p.S0, main_loop);
}

// deepest instantiated weight ring (3x3: 6, 4, 3 or 2 tiles; four-phase: 4 or 2) that fits the LDS next to the double-buffered halo and
// still leaves enough halo slots (3x3: taps 0 .. 9-NBST, one 8-row piece per wave each; four-phase: UP2_ASLOTS); 0 = the problem does
// not fit at all.  Depth matters at the low-resolution levels: their weights stream from HBM (~2 us away) while a tap is
// 0.2-0.4 us of MFMA work, so a workgroup must keep ~64+ KB of weight tiles in flight (Little's law).
inline int halo_pick_nbst(const IgemmParams& p, int bm, int taps = 9) {
  const int np = halo_rows(p, bm, taps) / 8;
  for (int nbst : {6, 4, 3, 2}) {
    if (taps == 4 && nbst != 4 && nbst != 2) continue;
    if (np > (taps == 9 ? 10 - nbst : UP2_ASLOTS) * HALO_NW) continue;
    if (halo_smem_bytes(p, bm, nbst, taps) > 160 * 1024) continue;
    return nbst;
  }
  return 0;
}

// ---- launch: L.bm / L.depth -> the instantiation --------------------------------------------------
// one launch of kernel K with dynamic LDS (its own per-device attribute guard)
template <auto K> int halo_run(const IgemmParams& p, const IgemmLaunch& L, hipStream_t stream) {
  static LdsAttrGuard guard;
  return launch_lds_kernel(K, guard, L.grid, L.block, L.lds, 160 * 1024, stream, p);
}
// f(std::integral_constant<int, BM>): BM = 256 / 224 if bm says so and the form has it (HAS256 / HAS224), else 128
template <bool HAS256 = true, bool HAS224 = false, typename F> int halo_with_bm(int bm, F&& f) {
  if constexpr (HAS256) {
    if (bm == 256) return f(std::integral_constant<int, 256>{});
  }
  if constexpr (HAS224) {
    if (bm == HALO_BM_STRIP) return f(std::integral_constant<int, HALO_BM_STRIP>{});
  }
  return f(std::integral_constant<int, 128>{});
}
// f(std::integral_constant<int, D>): D = the first of the instantiated depths that `depth` equals, the last of them for any other
template <int D0, int... DEPTHS, typename F> int halo_with_depth(int depth, F&& f) {
  if constexpr (sizeof...(DEPTHS) == 0) return f(std::integral_constant<int, D0>{});
  else return depth == D0 ? f(std::integral_constant<int, D0>{}) : halo_with_depth<DEPTHS...>(depth, f);
}
