// k22 — fused single-head attention of the MoVQ AttnBlock (movq_modules.py:185-225, vqgan_blocks.py AttnBlock): per image b and query t
//   out[b][t][:] = sum_j softmax_j(C^-1/2 q_t . k_j) v_j + bias_v,   j = 0 .. T-1, one head of C = 128 .. 512 channels, no mask.
// The [T][T] score matrix of the reference (and of the engine's "scores" route, movq.hip) never leaves the chip.
//
// Operands as the engine's GEMMs leave them: Q, K [B][T][C] row-major, V^T [B][C][T], all in the storage type; bias_v fp32 [C] (or null),
// added after the normalisation (the weights sum to 1); out [B][T][C] in the storage type.
//
// Work split: workgroup = 4 waves = 64 queries of one image (fp32: 32); wave w owns channels [w C/4, (w+1) C/4) and sees all of them.
//   per 32-key tile   S_w^T[key][q] = K[key][slice w] . Q[q][slice w]   (A = K tile rows from LDS, B = the wave's Q slice in registers)
//                     S^T = ((S_0 + S_1) + S_2) + S_3                   (partials exchanged through LDS, summed in wave order by every wave:
//                                                                        the four waves hold the same bits)
//                     lane-local fp32 online softmax (ONE query per lane column, 16 keys of the tile per lane half)
//                     O_w^T[d][q] += V^T[d][key] . P^T[key][q]          (A = the wave's C/4 rows of the V^T tile, B = P from the S^T registers)
// Scheme, fragments, V^T tile layout and the arithmetic contract: attention_common.h.  bias_v is added after the normalisation, before the
// one rounding on store.
// LDS at C = 512: K tile 32 KB + V^T tile 32 KB + exchange 32 KB (16-bit); fp32: 64 + 64 KB, the exchange reuses the K tile's bytes.
// 16-bit V^T tile: a row of 32 keys is 64 bytes, so one 128-byte LDS row holds channel d (pieces 0-3) and channel d + C/2 (pieces 4-7),
// each half key-permuted (vt_store16 / ld_frag_split with base piece 4 * half).  fp32 tiles: row = channel, 32 keys in natural order.
#include "attention_common.h"
#include <atomic>
#include <math.h>

namespace {

struct MovqAttnParams {
  const void* q; const void* k; const void* vt; const float* bias_v; void* out;
  int T;
  float scale;
};

constexpr int MQ_KT = 32;            // keys per tile
// 32-query blocks per workgroup: 64 queries for the 16-bit types; the fp32 parity path takes 32 (its Q slice and O^T rows cost twice the
// registers per query)
template <typename T> constexpr int MQ_NQB = sizeof(T) == 2 ? 2 : 1;
// partial-score exchange, bytes per wave: [q block][register group 4][lane 64] float4 (fp32: 4 x 4 KB, never more than the smallest K tile)
template <typename T> constexpr int MQ_XWAVE = MQ_NQB<T> * 4096;

template <typename T, int C>
__global__ __launch_bounds__(256) void movq_attention_kernel(MovqAttnParams p) {
  using TR = TT<T>;
  constexpr int EPC = TR::EPC, KSTEPS = TR::KSTEPS;
  constexpr int ES = (int)sizeof(T);
  constexpr int CW = C / 4;                  // channels per wave
  constexpr int NA = CW / 16;                // 16-channel steps of the score product per wave
  constexpr int NDB = CW / 32;               // 32-row blocks of O^T per wave
  constexpr int KBYTES = MQ_KT * C * ES;     // K tile: C * ES / 128 sub-tiles of [32 keys][128 B]; the V^T tile has the same size
  constexpr bool WIDE = ES == 4;             // fp32: tiles staged straight through (no register prefetch), exchange over the K tile
  constexpr int NQB = MQ_NQB<T>;             // 32-query blocks per workgroup
  constexpr int XWAVE = MQ_XWAVE<T>;
  static_assert(!WIDE || 4 * XWAVE <= KBYTES, "movq_attention_kernel: the exchange must fit the K tile it reuses");
  constexpr int CPRK = C / EPC;              // 16-byte chunks per K row
  constexpr int CPRV = MQ_KT / EPC;          // 16-byte chunks per V^T row of the tile
  constexpr int NCH = MQ_KT * CPRK / 256;    // chunks per thread per tile and tensor
  static_assert(C % 128 == 0 && C >= 128 && C <= 512, "movq_attention_kernel: C in {128, 256, 384, 512}");
  extern __shared__ __attribute__((aligned(16))) char mq_smem[];
  char* const Ks = mq_smem;
  char* const Vs = mq_smem + KBYTES;
  char* const Xs = WIDE ? mq_smem : mq_smem + 2 * KBYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int b = blockIdx.y;
  const int q0 = blockIdx.x * (32 * NQB);
  const int T_ = p.T;
  const T* Qg = reinterpret_cast<const T*>(p.q) + (int64_t)b * T_ * C;
  const T* Kg = reinterpret_cast<const T*>(p.k) + (int64_t)b * T_ * C;
  const T* Vg = reinterpret_cast<const T*>(p.vt) + (int64_t)b * C * T_;

  // this wave's slice of the 64 query rows: B operand of the score product
  Frag<T> qf[NQB][NA];
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
    for (int a = 0; a < NA; ++a) ld_qfrag(qf[qb][a], Qg + (int64_t)(q0 + qb * 32 + l31) * C + wave * CW + 16 * a + 8 * h);

  // Staging: thread -> (row, 16-byte piece) maps under which every LDS swizzle and every lane offset is the same for all of a thread's
  // chunks (one address register per tensor, the rest immediates).  K: row = tid >> 3, chunk (tid & 7) of sub-tile i.  V^T: channel
  // tid / CPRV + i * DR, piece tid % CPRV (DR = 256 / CPRV channels apart: a multiple of 16 rows, so the swizzle does not move).
  constexpr int DR = 256 / CPRV;
  static_assert(NCH == CPRK / 8 && NCH * DR == C, "movq_attention_kernel: staging maps");
  const int krow = tid >> 3, kc = tid & 7;
  const int vd = tid / CPRV, vc = tid - vd * CPRV;
  const unsigned kg_off = (unsigned)(krow * C + kc * EPC) * ES;           // bytes into the (contiguous) K tile
  const unsigned vg_off = (unsigned)(vd * T_ + vc * EPC) * ES;            // bytes from V^T[0][tile's first key]  (<= 64 T ES: fits 32 bits)
  char* const ks_at = Ks + lds_chunk_off(krow, kc);
  u32x4_t kreg[NCH], vreg[WIDE ? 1 : NCH];
#define K22_MQ_KLOAD(KT_)                                                                                 \
  {                                                                                                       \
    const char* kb_ = reinterpret_cast<const char*>(Kg) + (int64_t)(KT_) * (MQ_KT * C * ES);              \
    _Pragma("unroll") for (int i = 0; i < NCH; ++i) kreg[i] = *reinterpret_cast<const u32x4_t*>(kb_ + i * 128 + kg_off); \
  }
#define K22_MQ_KSTORE()                                                                                   \
  {                                                                                                       \
    _Pragma("unroll") for (int i = 0; i < NCH; ++i) *reinterpret_cast<u32x4_t*>(ks_at + i * 4096) = kreg[i]; \
  }
  // VR: the staging registers (the 16-bit types prefetch V^T beside K; fp32 reuses kreg)
#define K22_MQ_VLOAD(VR, KT_)                                                                             \
  {                                                                                                       \
    const char* vb_ = reinterpret_cast<const char*>(Vg) + (int64_t)(KT_) * (MQ_KT * ES);                  \
    _Pragma("unroll") for (int i = 0; i < NCH; ++i)                                                       \
      VR[i] = *reinterpret_cast<const u32x4_t*>(vb_ + (int64_t)i * DR * T_ * ES + vg_off);                \
  }
#define K22_MQ_VSTORE(VR)                                                                                 \
  {                                                                                                       \
    _Pragma("unroll") for (int i = 0; i < NCH; ++i) {                                                     \
      if constexpr (WIDE) {                                                                               \
        *reinterpret_cast<u32x4_t*>(Vs + i * DR * 128 + lds_chunk_off(vd, vc)) = VR[i];                   \
      } else {                                                                                            \
        const int half = i * DR >= C / 2 ? 1 : 0;   /* channel vd + i DR: LDS row vd + i DR - half C/2 */ \
        vt_store16(Vs + (i * DR - half * (C / 2)) * 128, vd, vc, VR[i], 4 * half);                        \
      }                                                                                                   \
    }                                                                                                     \
  }

  f32x16_t o[NDB][NQB];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[db][qb][r] = 0.f;
  float m_run[NQB], l_run[NQB];
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) { m_run[qb] = -1e30f; l_run[qb] = 0.f; }
  const float cexp = p.scale * 1.4426950408889634f;   // exp(s*scale - m*scale) = exp2((s - m) * cexp)
  const int nkt = T_ / MQ_KT;

  if constexpr (!WIDE) { K22_MQ_KLOAD(0); K22_MQ_VLOAD(vreg, 0); }
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();   // every wave finished reading the previous tile (K, V^T and the exchange)
    if constexpr (WIDE) {
      K22_MQ_KLOAD(kt); K22_MQ_KSTORE();
      K22_MQ_VLOAD(kreg, kt); K22_MQ_VSTORE(kreg);
    } else {
      K22_MQ_KSTORE(); K22_MQ_VSTORE(vreg);
    }
    __syncthreads();
    if constexpr (!WIDE) {
      const int ktn = kt + 1 < nkt ? kt + 1 : nkt - 1;
      K22_MQ_KLOAD(ktn); K22_MQ_VLOAD(vreg, ktn);
    }

    // ---- this wave's partial scores over its channel slice
    f32x16_t s[NQB];
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[qb][r] = 0.f;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int c16 = wave * NA + a;   // 16-channel step of the whole row
      Frag<T> kf;
      ld_frag(kf, Ks + (c16 / KSTEPS) * 4096, l31, c16 % KSTEPS, h);
#pragma unroll
      for (int qb = 0; qb < NQB; ++qb) mma_atom(s[qb], kf, qf[qb][a]);
    }

    // ---- S^T = ((S_0 + S_1) + S_2) + S_3: every wave uses the same lane -> (key, query) map, so a lane reads back its own position
    if constexpr (WIDE) __syncthreads();   // the exchange overwrites the K tile
    {
      float4* xw = reinterpret_cast<float4*>(Xs + wave * XWAVE);
#pragma unroll
      for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
        for (int g = 0; g < 4; ++g) xw[(qb * 4 + g) * 64 + lane] = make_float4(s[qb][4 * g], s[qb][4 * g + 1], s[qb][4 * g + 2], s[qb][4 * g + 3]);
    }
    __syncthreads();
    float pv[NQB][16];
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb)
    {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4* xr = reinterpret_cast<const float4*>(Xs) + (qb * 4 + g) * 64 + lane;
        constexpr int XW = XWAVE / 16;
        const float4 x0 = xr[0], x1 = xr[XW], x2 = xr[2 * XW], x3 = xr[3 * XW];
        pv[qb][4 * g] = ((x0.x + x1.x) + x2.x) + x3.x;
        pv[qb][4 * g + 1] = ((x0.y + x1.y) + x2.y) + x3.y;
        pv[qb][4 * g + 2] = ((x0.z + x1.z) + x2.z) + x3.z;
        pv[qb][4 * g + 3] = ((x0.w + x1.w) + x2.w) + x3.w;
      }
      __builtin_amdgcn_sched_barrier(0);   // one query block's 16 reads at a time: all 32 in flight at once do not fit the registers at C = 512
    }

    // ---- online softmax, lane-local: the lane halves of a query column hold 16 keys each
    float mloc[NQB];
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
      float m = pv[qb][0];
#pragma unroll
      for (int r = 1; r < 16; ++r) m = fmaxf(m, pv[qb][r]);
      mloc[qb] = fmaxf(m, __shfl_xor(m, 32, 64));
    }
    bool rose = false;
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) rose = rose || mloc[qb] > m_run[qb];
    if (__any(rose)) {   // wave-uniform; rare after the first tiles
#pragma unroll
      for (int qb = 0; qb < NQB; ++qb) {
        const float m_new = fmaxf(m_run[qb], mloc[qb]);
        const float alpha = exp2_t<T>((m_run[qb] - m_new) * cexp);
        l_run[qb] *= alpha;
        m_run[qb] = m_new;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[db][qb][r] *= alpha;
      }
    }
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
      const float mc = m_run[qb] * cexp;
      float lsum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = exp2_t<T>(fmaf(pv[qb][r], cexp, -mc));
        pv[qb][r] = e;
        lsum += e;
      }
      l_run[qb] += lsum;
    }

    // ---- O_w^T += V^T tile rows of this wave . P^T
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      Frag<T> pf[NQB];
#pragma unroll
      for (int qb = 0; qb < NQB; ++qb) make_pfrag(pf[qb], &pv[qb][8 * a]);
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        Frag<T> vf;
        if constexpr (WIDE) ld_frag_split(vf, Vs, wave * CW + db * 32 + l31, a, h);
        else ld_frag_split(vf, Vs, (wave & 1) * CW + db * 32 + l31, a, h, 4 * (wave >> 1));
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) mma_atom(o[db][qb], vf, pf[qb]);
      }
    }
  }
#undef K22_MQ_KLOAD
#undef K22_MQ_KSTORE
#undef K22_MQ_VLOAD
#undef K22_MQ_VSTORE

#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {
    const float l_tot = l_run[qb] + __shfl_xor(l_run[qb], 32, 64);
    const float inv = 1.f / l_tot;
    T* orow = reinterpret_cast<T*>(p.out) + ((int64_t)b * T_ + q0 + qb * 32 + l31) * C + wave * CW;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = db * 32 + 8 * g + 4 * h;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (p.bias_v != nullptr) {
#pragma unroll
          for (int j = 0; j < 4; ++j) bv[j] = p.bias_v[wave * CW + d + j];
        }
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = o[db][qb][4 * g + j] * inv + bv[j];
        att_store4(orow, d, false, [&](int j) { return y[j]; });
      }
  }
}

template <typename T, int C> int mq_launch(const MovqAttnParams& p, int B, hipStream_t s) {
  constexpr int lds = sizeof(T) == 4 ? 2 * MQ_KT * C * 4 : 2 * MQ_KT * C * 2 + 4 * MQ_XWAVE<T>;
  static_assert(lds <= 160 * 1024, "movq_attention_kernel: LDS budget");
  static LdsAttrGuard guard;
  if (int rc = k22_ensure_lds_attr(guard, reinterpret_cast<const void*>(&movq_attention_kernel<T, C>), lds, __FILE__, __LINE__)) return rc;
  hipLaunchKernelGGL((movq_attention_kernel<T, C>), dim3(p.T / (32 * MQ_NQB<T>), B), dim3(256), lds, s, p);
  K22_CHECK_LAUNCH();
  return K22_OK;
}
template <typename T> int mq_launch_c(const MovqAttnParams& p, int B, int C, hipStream_t s) {
  switch (C) {
    case 128: return mq_launch<T, 128>(p, B, s);
    case 256: return mq_launch<T, 256>(p, B, s);
    case 384: return mq_launch<T, 384>(p, B, s);
    case 512: return mq_launch<T, 512>(p, B, s);
  }
  return k22_set_error(K22_EINVAL, "movq_attention: C must be 128, 256, 384 or 512");
}

std::atomic<long> g_mq_launches{0};

}  // namespace

long movq_fused_attn_launch_count() { return g_mq_launches.load(); }

int launch_movq_attention(const void* q, const void* k, const void* vt, const float* bias_v, void* out, int B, int T, int C, int dtype, hipStream_t s) {
  if (!q || !k || !vt || !out) return k22_set_error(K22_EINVAL, "movq_attention: null q, k, vt or out");
  if (!movq_attention_admits_c(C)) return k22_set_error(K22_EINVAL, "movq_attention: C must be 128, 256, 384 or 512");
  if (!movq_attention_admits_t(T)) return k22_set_error(K22_EINVAL, "movq_attention: T must be a positive multiple of 64, at most 4194304");
  if (B < 1 || B > 65535) return k22_set_error(K22_EINVAL, "movq_attention: B must be in 1 .. 65535");
  if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(vt) | reinterpret_cast<uintptr_t>(out)) & 15)
    return k22_set_error(K22_EINVAL, "movq_attention: q, k, vt and out must be 16-byte aligned");
  MovqAttnParams p;
  p.q = q; p.k = k; p.vt = vt; p.bias_v = bias_v; p.out = out; p.T = T; p.scale = 1.0f / sqrtf((float)C);
  int rc;
  if (dtype == K22_BF16) rc = mq_launch_c<bf16_t>(p, B, C, s);
  else if (dtype == K22_F16) rc = mq_launch_c<f16_t>(p, B, C, s);
  else if (dtype == K22_F32) rc = mq_launch_c<float>(p, B, C, s);
  else return k22_set_error(K22_EINVAL, "movq_attention: dtype must be K22_BF16, K22_F16 or K22_F32");
  if (rc == K22_OK) g_mq_launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}
