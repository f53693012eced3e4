// k22 — what the hand-written attention kernels share: attention_kernel, attention_pipe_kernel, small_attention_kernel (attention.hip)
// and movq_attention_kernel (movq_attention.hip).
//
// The common idea: S^T = K Q^T (A = K tile rows from the LDS, B = Q fragments in registers), so the C layout puts ONE query per lane
// column (lane & 31) and the keys of a tile in the lane's accumulator registers (c_row); the softmax is lane-local fp32 plus one exchange
// between the lane halves, and P goes from the accumulator registers straight into O^T += V^T P^T (A = V^T tile rows, B = P): no LDS
// round trip, the rescale factor of the online softmax is lane-local.
//
// ARITHMETIC CONTRACT of all four kernels (each kernel's banner states only its work split, LDS budget and masks):
//   * scores, running maximum and row sum in fp32; p = exp2((s - m) * scale * log2(e)) as ONE fma per score in front of exp2_t;
//   * the row sum is taken over the UNROUNDED probabilities;
//   * P is rounded ONCE, to the tile type, in front of the P V product (make_pfrag) - fp32: not at all; x3: split as 2^10 P, the exact
//     inverse comes out of the accumulators with 1 / l (K22_ATT_X3_PSCALE_INV);
//   * the output is normalised in fp32 and rounded once on store (att_store4);
//   * a fixed reduction order and no atomics: two launches give equal bits, and nothing in a tile's arithmetic depends on the batch or
//     the grid.  The ORDER of the fp32 row maximum and row sum is each kernel's own (the UNet kernels sum even / odd pairs, the other
//     two sequentially): those sites are not shared on purpose, their bits differ.
#pragma once
#include "kernels.h"
#include <type_traits>

// 2^x: the 16-bit paths use the raw v_exp_f32 (inputs here are <= 0; results below 2^-126 flush, which is far below the resolution of
// 16-bit probabilities), the fp32 parity path and the split one the accurate exp2f.
template <typename T> __device__ __forceinline__ float exp2_t(float x);
template <> __device__ __forceinline__ float exp2_t<bf16_t>(float x) { return __builtin_amdgcn_exp2f(x); }
template <> __device__ __forceinline__ float exp2_t<f16_t>(float x) { return __builtin_amdgcn_exp2f(x); }
template <> __device__ __forceinline__ float exp2_t<float>(float x) { return exp2f(x); }
template <> __device__ __forceinline__ float exp2_t<x3_t>(float x) { return exp2f(x); }

// xh_t (round 5): the attention of the ASYMMETRIC split engine (K22_F16X2).  q / K_all / V^T_all are the fp32 tensors the split engines'
// qkv GEMM writes; they are rounded to fp16 while the tiles are staged (Q: at fragment load) and the kernel runs the fp16 engine's body:
// ONE MFMA per product, fp32 online softmax, native exp2.  The operand rounding of the attention is 1.5 % of the error budget of that
// engine (tests/golden/drift_ablation_x2.json, kind `a`); the output is written as x3 chunks for the proj_out GEMM, which keeps all
// three MFMAs.
struct xh_t { float f; };
// AttC<TS>: type = arithmetic / LDS type, mem = element type of q / K_all / V^T_all / out in memory, MIX = the two differ
template <typename T> struct AttC { using type = T; using mem = T; static constexpr bool MIX = false; };
template <> struct AttC<xh_t> { using type = f16_t; using mem = float; static constexpr bool MIX = true; };
__device__ __forceinline__ u32x4_t f16x8_from_f32(const u32x4_t a, const u32x4_t b) {
  const float4 x = __builtin_bit_cast(float4, a), y = __builtin_bit_cast(float4, b);
  return u32x4_t{pack2_f16(x.x, x.y), pack2_f16(x.z, x.w), pack2_f16(y.x, y.y), pack2_f16(y.z, y.w)};
}

// ---- Q fragment (8 consecutive channels of a query row in memory) and P fragment (8 probabilities out of the score registers) ----------
__device__ __forceinline__ void ld_qfrag(Frag<bf16_t>& f, const bf16_t* p) { f.v = *reinterpret_cast<const u32x4_t*>(p); }
__device__ __forceinline__ void ld_qfrag(Frag<f16_t>& f, const f16_t* p) { f.v = *reinterpret_cast<const u32x4_t*>(p); }
__device__ __forceinline__ void ld_qfrag(Frag<float>& f, const float* p) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w;
  f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
}
__device__ __forceinline__ void ld_qfrag(Frag<x3_t>& f, const x3_t* p) {
  x3_frag_from_f32(f, *reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4));
}
__device__ __forceinline__ void ld_qfrag(Frag<f16_t>& f, const float* p) {   // xh_t: fp32 in memory, fp16 fragment
  f.v = f16x8_from_f32(*reinterpret_cast<const u32x4_t*>(p), *reinterpret_cast<const u32x4_t*>(p + 4));
}
__device__ __forceinline__ void make_pfrag(Frag<bf16_t>& f, const float* p) {
  f.v = u32x4_t{pack2_bf16(p[0], p[1]), pack2_bf16(p[2], p[3]), pack2_bf16(p[4], p[5]), pack2_bf16(p[6], p[7])};
}
__device__ __forceinline__ void make_pfrag(Frag<f16_t>& f, const float* p) {
  f.v = u32x4_t{pack2_f16(p[0], p[1]), pack2_f16(p[2], p[3]), pack2_f16(p[4], p[5]), pack2_f16(p[6], p[7])};
}
__device__ __forceinline__ void make_pfrag(Frag<float>& f, const float* p) {
#pragma unroll
  for (int j = 0; j < 8; ++j) f.v[j] = p[j];
}
// P (<= 1) is split as 2^10 P: the lo half of an unscaled probability under 2^-3 is a fp16 subnormal, i.e. P carried to 2^-25 ABSOLUTE
// (common.h, "x3 chunk") where the arithmetic promises 2^-22 relative - on a row whose heavy keys have a small V element the many light
// keys then decide the error (tests/test_attention_parity_gpu.py: 1.03 of the float64 bound at T = 81, causal, before).  The exact power
// of two comes out of the accumulators with 1 / l (K22_ATT_X3_PSCALE_INV); 2^10 P <= 1024 is far inside fp16's range.
constexpr float K22_ATT_X3_PSCALE = 1024.f, K22_ATT_X3_PSCALE_INV = 1.f / 1024.f;
__device__ __forceinline__ void make_pfrag(Frag<x3_t>& f, const float* p) {
  constexpr float c = K22_ATT_X3_PSCALE;
  x3_frag_from_f32(f, make_float4(c * p[0], c * p[1], c * p[2], c * p[3]), make_float4(c * p[4], c * p[5], c * p[6], c * p[7]));
}

// ---- V^T tiles -------------------------------------------------------------------------------------------------------------------------
// The V^T fragment of 16-key atom a must hold its keys in the order of the S^T accumulator registers the P fragment is made of:
// element j < 4 -> key 16 a + 4 h + j ; j >= 4 -> key 16 a + 8 + 4 h + (j - 4)   (c_row; h = lane >> 5).
// 16-bit tiles (round 6) are therefore stored KEY-PERMUTED within every block of 16 keys, so that the fragment is ONE conflict-free
// ds_read_b128.  With the natural key order it was two 8-byte reads gathered by six register moves per PV atom: 24 v_mov per 64-key tile,
// and the LDS array - not the matrix pipe and not VALU issue - was what the tile loop waited for (ds_read2st64_b64: 8+ LDS cycles per
// wave-instruction against 4; SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 1.64 on attention_kernel, profiles/r05_pmc_mfma_bf16.txt).
// THE PERMUTATION: key k of a row's block of keys (64 per 128-byte row; MoVQ: 32 per half row) lives in 16-byte piece vt_piece(k) of
// the block at byte vt_byte(k); lds_chunk_off places the piece.
// The expressions are MACROS; the constexpr functions, the stores, the fragment read and the compile-time check below are all written with
// them, so the check sees the text that executes.  (Macros, because behind function calls - force-inlined or not - the same expressions
// give small_attention_kernel and the UNet kernels other instruction orders than the measured ones; tools/compare_device_code.py.)
#define K22_VT_PIECE(k) (2 * ((k) >> 4) + (((k) >> 2) & 1))
#define K22_VT_BYTE(k) (8 * (((k) >> 3) & 1) + 2 * ((k) & 3))
constexpr __host__ __device__ int vt_piece(int k) { return K22_VT_PIECE(k); }
constexpr __host__ __device__ int vt_byte(int k) { return K22_VT_BYTE(k); }
// spelled out for keys 8 cc .. 8 cc + 7 at once (keys + 0..3: an 8-byte half in piece LO, + 4..7: one in piece HI, both at byte VT8_BYTE)
// and for the read (the piece that holds the fragment of atom a for lane half h); checked against vt_piece / vt_byte below
#define K22_VT8_PIECE_LO(cc) ((cc) & ~1)
#define K22_VT8_PIECE_HI(cc) ((cc) | 1)
#define K22_VT8_BYTE(cc) (8 * ((cc) & 1))
#define K22_VT_FRAG_PIECE(a, h) (2 * (a) + (h))
// stores keys 8 cc .. 8 cc + 7 (one 16-byte register, natural order) of V^T row `row`; the row's block of keys starts at piece `base`
// (0: attention.hip; 4 * half: movq_attention.hip's two channels per LDS row).  With the base folded into cc, or in front of it, bytes move.
__device__ __forceinline__ void vt_store16(char* tile, int row, int cc, const u32x4_t v, int base = 0) {
  *reinterpret_cast<u32x2_t*>(tile + lds_chunk_off(row, K22_VT8_PIECE_LO(cc) + base) + K22_VT8_BYTE(cc)) = u32x2_t{v.x, v.y};
  *reinterpret_cast<u32x2_t*>(tile + lds_chunk_off(row, K22_VT8_PIECE_HI(cc) + base) + K22_VT8_BYTE(cc)) = u32x2_t{v.z, v.w};
}
// stores one 16-bit element, key k of V^T row `row` (the transposing scatter of small_attention_kernel); a macro for the reason above
#define K22_VT_STORE1(tile, row, k, v) *reinterpret_cast<unsigned short*>((tile) + lds_chunk_off((row), K22_VT_PIECE(k)) + K22_VT_BYTE(k)) = (v)
// the fragment of atom a for lane half h: ONE piece of the row's block
__device__ __forceinline__ void ld_frag_split(Frag<bf16_t>& f, const char* tile, int r, int a, int h, int base = 0) {
  f.v = *reinterpret_cast<const u32x4_t*>(tile + lds_chunk_off(r, base + K22_VT_FRAG_PIECE(a, h)));
}
__device__ __forceinline__ void ld_frag_split(Frag<f16_t>& f, const char* tile, int r, int a, int h, int base = 0) {
  f.v = *reinterpret_cast<const u32x4_t*>(tile + lds_chunk_off(r, base + K22_VT_FRAG_PIECE(a, h)));
}
// The layout against the register order, at compile time: the key the stores put at element j of the fragment read (piece 2 a + h,
// byte 2 j) is the key of score register 8 (a & 1) + j of 32-key block a >> 1 in lane half h.
constexpr __host__ __device__ bool vt_layout_matches_c_row() {
  for (int cc = 0; cc < 8; ++cc)   // vt_store16: key 8 cc + e is element e & 3 of the 8-byte half in piece LO (e < 4) or HI
    for (int e = 0; e < 8; ++e)
      if (vt_piece(8 * cc + e) != (e < 4 ? K22_VT8_PIECE_LO(cc) : K22_VT8_PIECE_HI(cc)) || vt_byte(8 * cc + e) != K22_VT8_BYTE(cc) + 2 * (e & 3)) return false;
  for (int a = 0; a < 4; ++a)
    for (int h = 0; h < 2; ++h)
      for (int j = 0; j < 8; ++j) {
        const int key = 32 * (a >> 1) + c_row(8 * (a & 1) + j, 32 * h);
        if (key != (j < 4 ? 16 * a + 4 * h + j : 16 * a + 8 + 4 * h + (j - 4))) return false;
        if (vt_piece(key) != K22_VT_FRAG_PIECE(a, h) || vt_byte(key) != 2 * j) return false;
      }
  return true;
}
static_assert(vt_layout_matches_c_row(), "key-permuted V^T tile: the fragment's key order must be that of the S^T accumulator registers");

// 4-byte tiles keep the natural key order: two 16-byte (fp32) or four 8-byte (x3) reads per fragment
__device__ __forceinline__ void ld_frag_split(Frag<float>& f, const char* tile, int r, int a, int h) {
  const char* sub = tile + (a >> 1) * 8192;
  const int al = a & 1;
  const float4 lo = *reinterpret_cast<const float4*>(sub + lds_chunk_off(r, 4 * al + h));
  const float4 hi = *reinterpret_cast<const float4*>(sub + lds_chunk_off(r, 4 * al + 2 + h));
  f.v[0] = lo.x; f.v[1] = lo.y; f.v[2] = lo.z; f.v[3] = lo.w;
  f.v[4] = hi.x; f.v[5] = hi.y; f.v[6] = hi.z; f.v[7] = hi.w;
}
// split precision: the LDS tiles hold x3 chunks (converted once per workgroup while staging), P and Q are split in registers
__device__ __forceinline__ void ld_frag_split(Frag<x3_t>& f, const char* tile, int r, int a, int h) {
  const char* sub = tile + (a >> 1) * 8192;
  const int al = a & 1;
  // keys 16 a + 4 h + {0..3} = elements 4 h .. of group 2 al, keys 16 a + 8 + 4 h + {0..3} = the same elements of group 2 al + 1: 8-byte
  // halves of the groups' hi pieces (chunks 4 al, 4 al + 2) and lo pieces (4 al + 1, 4 al + 3)
  const u32x2_t h0 = *reinterpret_cast<const u32x2_t*>(sub + lds_chunk_off(r, 4 * al) + 8 * h);
  const u32x2_t l0 = *reinterpret_cast<const u32x2_t*>(sub + lds_chunk_off(r, 4 * al + 1) + 8 * h);
  const u32x2_t h1 = *reinterpret_cast<const u32x2_t*>(sub + lds_chunk_off(r, 4 * al + 2) + 8 * h);
  const u32x2_t l1 = *reinterpret_cast<const u32x2_t*>(sub + lds_chunk_off(r, 4 * al + 3) + 8 * h);
  f.hi = u32x4_t{h0.x, h0.y, h1.x, h1.y};
  f.lo = u32x4_t{l0.x, l0.y, l1.x, l1.y};
}

// ---- output: four consecutive channels of one query, normalised fp32 values, ONE rounding ----------------------------------------------
// y(j), j = 0 .. 3: the values.  T = the element type of `out` in memory: 16-bit -> one 8-byte store; 4-byte -> a float4, or x3 chunks
// (x3 != 0) where the consumer is a split GEMM.  y is a callable and the address base + off is formed here so that every value is computed
// where its conversion consumes it: the order the epilogues always had (with four floats and a pointer the kernels' code bytes move).
template <typename T, typename I, typename F>
__device__ __forceinline__ void att_store4(T* base, I off, bool x3, F y) {
  if constexpr (sizeof(T) == 2) {
    uint2 w;
    w.x = pack2<T>(y(0), y(1));
    w.y = pack2<T>(y(2), y(3));
    *reinterpret_cast<uint2*>(base + off) = w;
  } else if (x3) {
    x3_store4(base + off, x3_split4(y(0), y(1), y(2), y(3)));
  } else {
    *reinterpret_cast<float4*>(base + off) = make_float4(y(0), y(1), y(2), y(3));
  }
}
