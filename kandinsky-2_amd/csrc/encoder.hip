// k22 — conditioning-encoder engine: the three transformer towers that turn a prompt / an image into the embeddings the prior and
// the UNet consume.  One config-driven engine (K22Encoder) covers
//
//   K22_ENC_CLIP_TEXT    OpenAI CLIP ViT-L/14 text tower as Kandinsky2_1.generate_clip_emb walks it
//                        (kandinsky2/kandinsky2_1_model.py:159-168): token + positional embedding, 12 pre-LN causal blocks with
//                        QuickGELU MLPs, ln_final -> txt_feat_seq [B,77,768]; row argmax(tokens) @ text_projection -> txt_feat
//                        Also transformers' CLIPTextModelWithProjection (the CLIP-bigG text tower of the Kandinsky 2.2 prior): erf GELU,
//                        cfg.key_mask = the attention_mask's padded keys masked under the causal triangle, cfg.eos_id = the pooled row
//                        is the first position holding that id.  Both are plan-time switches; zero = the OpenAI tower above
//   K22_ENC_CLIP_VISION  clip_model.encode_image (kandinsky2_1_model.py:177-181): 14x14 patch embedding, class token,
//                        positional embedding, ln_pre, 24 pre-LN blocks, ln_post(class token) @ proj -> [B,768]
//   K22_ENC_XLMR         MultilingualCLIP.forward (kandinsky2/model/text_encoders.py:108-122): transformers' XLMRobertaModel
//                        (embeddings + LayerNorm, 24 post-LN blocks, erf-GELU, key-padding mask) -> embs [B,77,1024];
//                        LinearTransformation(masked mean over tokens) -> [B,768]
//
// They run once per prompt, not per denoising step (a "next" row, outside the per-step roofline accounting).
// MI355X mapping: the transformer engines' shared launch list and ops (xf_plan.h) - every Linear is one launch_igemm over the [N][K]
// weight, the fp32 residual stream is updated in place by the GEMM epilogue, LayerNorm writes the next GEMM's operand, attention is the
// UNet's flash kernel with a causal / key-validity mask.  QuickGELU is applied by a separate pass on the fp32 accumulator output of c_fc
// (one rounding, like a fused epilogue) so that the hot GEMM kernels' epilogue is left exactly as validated.
// Tile configurations of the transformer Linears come from the process-wide tile table like the other engines' (tuning.h): the
// production shapes (2/4/8 sequences, 1/2 images) are in the shipped table, so nothing is timed for them and the bits are the same
// on every box; other shapes are measured at their first pass (K22_AUTOTUNE=0: the fixed heuristic).
#include "kernels.h"
#include "elementwise.h"
#include "../../include/k22.h"
#include "tuning.h"
#include "xf_plan.h"

#include <deque>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

namespace {

// ---- token (+ position (+ token-type)) embedding -> fp32 sequence.  xlmr: position ids as transformers'
// create_position_ids_from_input_ids: (running count of non-padding tokens) * (token != pad) + pad_id -------------------------------
__global__ __launch_bounds__(256) void enc_embed_kernel(const int* tok, const float* tok_emb, const float* pos_emb, const float* type_emb,
                                                        float* x, int n_ctx, int D, int vocab, int xlmr, int pad_id, int max_pos) {
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const int* tb = tok + (int64_t)b * n_ctx;
  int id = tb[t];
  int pos = t;
  if (xlmr) {
    int cnt = 0;
    for (int j = 0; j <= t; ++j) cnt += tb[j] != pad_id;
    pos = (id != pad_id ? cnt : 0) + pad_id;
    pos = pos < max_pos ? pos : max_pos - 1;
  }
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float* te = tok_emb + (int64_t)id * D;
  const float* pe = pos_emb + (int64_t)pos * D;
  float* xr = x + ((int64_t)b * n_ctx + t) * D;
  for (int i = tid; i < D; i += 256) xr[i] = te[i] + pe[i] + (type_emb != nullptr ? type_emb[i] : 0.f);
}

// ---- CLIP text: the row of every sequence at its highest token id (the end-of-text token), torch.argmax semantics (first);
// eos_id > 0: at the FIRST position whose id equals eos_id instead (transformers' CLIPTextTransformer when config.eos_token_id != 2:
// (input_ids == eos_token_id).int().argmax(-1), so position 0 when the row holds no such id) ---------------------------------------
__global__ __launch_bounds__(256) void enc_gather_eot_kernel(const int* tok, const float* x, float* out, int n_ctx, int D, int eos_id) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int* tb = tok + (int64_t)b * n_ctx;
  int best = 0;
  if (eos_id > 0) {
    for (int j = n_ctx - 1; j >= 0; --j) if (tb[j] == eos_id) best = j;
  } else {
    int bv = tb[0];
    for (int j = 1; j < n_ctx; ++j) if (tb[j] > bv) { bv = tb[j]; best = j; }
  }
  const float* xr = x + ((int64_t)b * n_ctx + best) * D;
  for (int i = tid; i < D; i += 256) out[(int64_t)b * D + i] = xr[i];
}

// ---- XLM-R: (embs * mask).sum(1) / mask.sum(1) ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void enc_masked_mean_kernel(const float* x, const float* mask, float* out, int n_ctx, int D) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* mb = mask + (int64_t)b * n_ctx;
  float den = 0.f;
  for (int t = 0; t < n_ctx; ++t) den += mb[t];
  for (int i = tid; i < D; i += 256) {
    float s = 0.f;
    for (int t = 0; t < n_ctx; ++t) s += x[((int64_t)b * n_ctx + t) * D + i] * mb[t];
    out[(int64_t)b * D + i] = s / den;
  }
}

// ---- vision: [B][3][S][S] fp32 -> patch rows [B*P][Kp] T (column c*p*p + i*p + j as conv1.weight flattens; zero padding columns) ---
template <typename T>
__global__ __launch_bounds__(256) void enc_patchify_kernel(const float* img, T* out, int S, int patch, int Kp) {
  const int g = S / patch, P = g * g;
  const int row = blockIdx.x, b = row / P, pi = row % P, py = pi / g, px = pi % g;
  const int K = 3 * patch * patch;
  for (int k = threadIdx.x; k < Kp; k += 256) {
    float v = 0.f;
    if (k < K) {
      const int c = k / (patch * patch), r = k % (patch * patch), i = r / patch, j = r % patch;
      v = img[(((int64_t)b * 3 + c) * S + py * patch + i) * S + px * patch + j];
    }
    out[(int64_t)row * Kp + k] = from_f32<T>(v);
  }
}
// x[b][0] = class_embedding + pos[0];  x[b][1+p] = patch_out[b*P+p] + pos[1+p]
__global__ __launch_bounds__(256) void enc_vision_assemble_kernel(const float* patch_out, const float* cls, const float* pos, float* x, int P, int D) {
  const int b = blockIdx.y, t = blockIdx.x;
  const float* src = t == 0 ? cls : patch_out + ((int64_t)b * P + (t - 1)) * D;
  float* xr = x + ((int64_t)b * (P + 1) + t) * D;
  for (int i = threadIdx.x; i < D; i += 256) xr[i] = src[i] + pos[(int64_t)t * D + i];
}

// ---- MLP activation on fp32 rows -> T rows: QuickGELU (x * sigmoid(1.702 x), clip/model.py QuickGELU) or, exact != 0, the erf GELU
// of transformers' CLIP with hidden_act "gelu" (the open_clip ViT-bigG/14 image encoder of Kandinsky 2.2) ---------------------------
template <typename T>
__global__ __launch_bounds__(256) void enc_quickgelu_kernel(const float* x, T* y, int64_t n, int exact) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float v = x[i];
    y[i] = from_f32<T>(exact ? gelu_f(v) : v / (1.0f + __expf(-1.702f * v)));
  }
}

// ---- attention for head widths other than 64 (CLIP ViT-bigG/14: 1664 / 16 = 104 per head), short sequences (n <= 512), no mask:
// CLIPAttention.forward of transformers (softmax((q * hd^-0.5) k^T) v per head).  One workgroup = 16 queries of one (image, head):
// the head's K rows sit in the LDS as fp32 (row stride hd + 1 words: conflict-free across keys), every wave walks its 4 queries one
// at a time - lane = key for the scores (5 keys per lane at n = 257), lane = channel for P.V (V rows straight from L2, coalesced).
// Plain fp32 FMAs: 48 layers x 27 MFLOP per head is ~20 GFLOP per image, a few ms once per generation - not worth an MFMA tiling.
template <typename T>
__global__ __launch_bounds__(256) void enc_attention_generic_kernel(const T* __restrict__ qkv, T* __restrict__ out, int n, int D, int hd, float scale) {
  extern __shared__ __attribute__((aligned(16))) char esm[];
  // K and V rows of this (image, head) in the LDS, in the storage type (row stride hd + 2 elements: odd word stride for the 16-bit types,
  // so that 64 keys read one channel without bank conflicts).  fp32 storage (parity path): K only - V rows come from L2 (K + V would
  // need 216 KB); that path is for 1e-6 parity checks, not for speed.
  constexpr bool V_IN_LDS = sizeof(T) == 2;
  const int rs = hd + 2;
  T* Ks = reinterpret_cast<T*>(esm);                               // [n][rs]
  T* Vs = Ks + (size_t)n * rs;                                     // [n][rs] (16-bit types)
  float* qs = reinterpret_cast<float*>(esm + (((size_t)n * rs * sizeof(T) * (V_IN_LDS ? 2 : 1)) + 15) / 16 * 16);   // [4 waves][128]
  float* ps = qs + 4 * 128;                                        // [4 waves][512]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int head = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * 16;   // 16 queries per workgroup (4 per wave): 17 x 16 heads = 272 workgroups per image at n = 257
  const int64_t ld = 3 * (int64_t)D;
  const T* base = qkv + (int64_t)b * n * ld + head * hd;
  for (int i = tid; i < n * hd; i += 256) {
    const int key = i / hd, d = i - key * hd;
    Ks[key * rs + d] = base[(int64_t)key * ld + D + d];
    if (V_IN_LDS) Vs[key * rs + d] = base[(int64_t)key * ld + 2 * D + d];
  }
  __syncthreads();
  float* qw = qs + wave * 128;
  float* pw = ps + wave * 512;
  for (int qq = 0; qq < 4; ++qq) {
    const int qi = q0 + wave * 4 + qq;
    if (qi >= n) break;                                            // wave-uniform
    for (int d = lane; d < hd; d += 64) qw[d] = to_f32(base[(int64_t)qi * ld + d]) * scale;
    __builtin_amdgcn_wave_barrier();
    float sc[8];
    float m = -3.0e38f;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int key = kk * 64 + lane;
      float a = -3.0e38f;
      if (kk * 64 < n) {                                           // wave-uniform: whole key blocks past the sequence cost nothing
        a = 0.f;
        const T* kr = Ks + (key < n ? key : n - 1) * rs;
        for (int d = 0; d < hd; ++d) a += qw[d] * to_f32(kr[d]);
        if (key >= n) a = -3.0e38f;
      }
      sc[kk] = a;
      m = fmaxf(m, a);
    }
    m = wave_max(m);
    float l = 0.f;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int key = kk * 64 + lane;
      if (key < n) {
        const float e = __expf(sc[kk] - m);
        pw[key] = e;
        l += e;
      }
    }
    l = wave_sum(l);
    __builtin_amdgcn_wave_barrier();
    const float inv = 1.f / l;
    for (int d = lane; d < hd; d += 64) {
      float acc = 0.f;
      if (V_IN_LDS) {
        const T* vp = Vs + d;
        for (int key = 0; key < n; ++key) acc += pw[key] * to_f32(vp[key * rs]);
      } else {
        const T* vp = base + 2 * D + d;
        for (int key = 0; key < n; ++key) acc += pw[key] * to_f32(vp[(int64_t)key * ld]);
      }
      out[((int64_t)b * n + qi) * D + head * hd + d] = from_f32<T>(acc * inv);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- launchers: the plan's ops and the single-kernel entry points (include/k22.h) go through the same code ------------------------------
int launch_enc_embed(const int* tok, const float* te, const float* pe, const float* ty, float* x, int B, int n, int D, int vocab, int xlmr,
                     int pad, int maxp, hipStream_t st) {
  hipLaunchKernelGGL(enc_embed_kernel, dim3(n, B), dim3(256), 0, st, tok, te, pe, ty, x, n, D, vocab, xlmr ? 1 : 0, pad, maxp);
  K22_CHECK_LAUNCH();
  return K22_OK;
}
int launch_enc_gather_eot(const int* tok, const float* x, float* out, int B, int n, int D, int eos_id, hipStream_t st) {
  hipLaunchKernelGGL(enc_gather_eot_kernel, dim3(B), dim3(256), 0, st, tok, x, out, n, D, eos_id);
  K22_CHECK_LAUNCH();
  return K22_OK;
}
int launch_enc_masked_mean(const float* x, const float* mask, float* out, int B, int n, int D, hipStream_t st) {
  hipLaunchKernelGGL(enc_masked_mean_kernel, dim3(B), dim3(256), 0, st, x, mask, out, n, D);
  K22_CHECK_LAUNCH();
  return K22_OK;
}
int launch_enc_patchify(const float* img, void* out, int B, int S, int patch, int Kp, int dt, hipStream_t st) {
  const int g = S / patch, P = g * g;
  if (dt == K22_BF16) hipLaunchKernelGGL(enc_patchify_kernel<bf16_t>, dim3(B * P), dim3(256), 0, st, img, reinterpret_cast<bf16_t*>(out), S, patch, Kp);
  else if (dt == K22_F16) hipLaunchKernelGGL(enc_patchify_kernel<f16_t>, dim3(B * P), dim3(256), 0, st, img, reinterpret_cast<f16_t*>(out), S, patch, Kp);
  else hipLaunchKernelGGL(enc_patchify_kernel<float>, dim3(B * P), dim3(256), 0, st, img, reinterpret_cast<float*>(out), S, patch, Kp);
  K22_CHECK_LAUNCH();
  return K22_OK;
}
int launch_enc_vision_assemble(const float* patch_out, const float* cls, const float* pos, float* x, int B, int P, int D, hipStream_t st) {
  hipLaunchKernelGGL(enc_vision_assemble_kernel, dim3(P + 1, B), dim3(256), 0, st, patch_out, cls, pos, x, P, D);
  K22_CHECK_LAUNCH();
  return K22_OK;
}
int launch_enc_mlp_act(const float* x, void* y, int64_t nel, int exact, int dt, hipStream_t st) {
  const int nb = (int)((nel + 255) / 256 < 4096 ? (nel + 255) / 256 : 4096);
  if (dt == K22_BF16) hipLaunchKernelGGL(enc_quickgelu_kernel<bf16_t>, dim3(nb), dim3(256), 0, st, x, reinterpret_cast<bf16_t*>(y), nel, exact);
  else if (dt == K22_F16) hipLaunchKernelGGL(enc_quickgelu_kernel<f16_t>, dim3(nb), dim3(256), 0, st, x, reinterpret_cast<f16_t*>(y), nel, exact);
  else hipLaunchKernelGGL(enc_quickgelu_kernel<float>, dim3(nb), dim3(256), 0, st, x, reinterpret_cast<float*>(y), nel, exact);
  K22_CHECK_LAUNCH();
  return K22_OK;
}
// dynamic LDS of enc_attention_generic_kernel: K (and V for the 16-bit types) rows of hd + 2 elements, then [4 waves][128 + 512] fp32
size_t enc_ga_smem(int n, int hd, size_t esz) { return ((size_t)n * (hd + 2) * esz * (esz == 2 ? 2 : 1) + 15) / 16 * 16 + 4 * 640 * 4; }
// what the kernel is built for: q rows of <= 128 channels and <= 512 scores per wave in the LDS, everything within 160 KB
bool enc_ga_admits(int n, int hd, size_t esz) { return hd <= 128 && n <= 512 && enc_ga_smem(n, hd, esz) <= 160 * 1024; }
int launch_enc_attention_generic(const void* qkv, void* out, int B, int heads, int n, int hd, int dt, hipStream_t st) {
  const int D = heads * hd;
  const size_t smem = enc_ga_smem(n, hd, dt == K22_F32 ? 4 : 2);
  const float sc = 1.0f / sqrtf((float)hd);
  dim3 grid((n + 15) / 16, heads, B);
#define K22_GA(TT_)                                                                                                              \
  {                                                                                                                      \
    static LdsAttrGuard guard;                                                                                           \
    if (int rc_ = k22_ensure_lds_attr(guard, reinterpret_cast<const void*>(&enc_attention_generic_kernel<TT_>), 160 * 1024, __FILE__, __LINE__)) return rc_; \
    hipLaunchKernelGGL(enc_attention_generic_kernel<TT_>, grid, dim3(256), smem, st, reinterpret_cast<const TT_*>(qkv), reinterpret_cast<TT_*>(out), n, D, hd, sc);  \
  }
  if (dt == K22_BF16) K22_GA(bf16_t) else if (dt == K22_F16) K22_GA(f16_t) else K22_GA(float)
#undef K22_GA
  K22_CHECK_LAUNCH();
  return K22_OK;
}

}  // namespace

struct K22Encoder : XfPlan {   // tuned: every transformer Linear; graph: the 150-300 launches of one tower pass
  K22EncoderConfig cfg;
  int B = 0;
  Slot *s_tok, *s_valid, *s_img, *s_patch, *s_pout, *s_inp, *s_ln, *s_qkv, *s_att, *s_fc, *s_fc32, *s_seq, *s_pool_in, *s_pooled;

  int plan(int nB) {
    const int D = cfg.width, n = cfg.n_ctx, M = nB * n, heads = cfg.heads, od = cfg.out_dim, kind = cfg.kind;
    if (nB < 1 || nB > 8) return k22_set_error(K22_EINVAL, "encoder: 1..8 sequences / images per call");
    if (D < 64 || D % 64 || D > 2048 || heads < 1 || D % heads) return k22_set_error(K22_EINVAL, "encoder: width % 64 == 0, width <= 2048, width % heads == 0");
    const int hd = D / heads;
    const bool flash = hd == 64;       // the UNet's flash attention kernel; anything else: enc_attention_generic_kernel (vision tower only)
    if (!flash && (cfg.kind != K22_ENC_CLIP_VISION || !enc_ga_admits(n, hd, esz)))
      return k22_set_error(K22_EINVAL, "encoder: head widths other than 64 are built for the vision tower (<= 128 per head, <= 512 tokens)");
    const int F = cfg.mlp_dim > 0 ? cfg.mlp_dim : 4 * D;
    if (F % 64) return k22_set_error(K22_EINVAL, "encoder: mlp_dim % 64");
    if (kind < K22_ENC_CLIP_TEXT || kind > K22_ENC_XLMR) return k22_set_error(K22_EINVAL, "encoder: kind");
    if (n < 1 || cfg.layers < 1 || od < 1) return k22_set_error(K22_EINVAL, "encoder: n_ctx, layers and out_dim must be positive");
    const bool vision = kind == K22_ENC_CLIP_VISION, xlmr = kind == K22_ENC_XLMR;
    if (vision && (cfg.patch < 1 || cfg.image_size < cfg.patch)) return k22_set_error(K22_EINVAL, "encoder: patch / image_size");
    if (xlmr && (cfg.max_pos < 2 || cfg.pad_id < 0 || cfg.pad_id >= cfg.max_pos)) return k22_set_error(K22_EINVAL, "encoder: max_pos / pad_id");
    const int g = vision ? cfg.image_size / cfg.patch : 0, P = g * g;
    const int Kraw = 3 * cfg.patch * cfg.patch, Kp = (Kraw + 63) / 64 * 64;
    if (vision && (cfg.image_size % cfg.patch || P + 1 != n)) return k22_set_error(K22_EINVAL, "encoder: n_ctx must be (image_size/patch)^2 + 1");
    if (!vision && cfg.vocab < 1) return k22_set_error(K22_EINVAL, "encoder: vocab");
    if ((cfg.key_mask || cfg.eos_id) && kind != K22_ENC_CLIP_TEXT) return k22_set_error(K22_EINVAL, "encoder: key_mask / eos_id belong to the CLIP text tower");
    if (cfg.eos_id < 0 || (cfg.eos_id > 0 && cfg.eos_id >= cfg.vocab)) return k22_set_error(K22_EINVAL, "encoder: eos_id outside the vocabulary");
    if (cfg.key_mask && !flash) return k22_set_error(K22_EINVAL, "encoder: the key-padding mask runs on the 64-channel flash kernel");
    // validated: only now drop the previous plan
    begin_plan();
    B = nB;
    ops.clear();
    s_tok = new_slot((size_t)M * 4); s_valid = new_slot((size_t)M * 4);
    s_img = new_slot(vision ? (size_t)B * 3 * cfg.image_size * cfg.image_size * 4 : 0);
    s_patch = new_slot(vision ? (size_t)B * P * Kp * esz : 0); s_pout = new_slot(vision ? (size_t)B * P * D * 4 : 0);
    s_inp = new_slot((size_t)M * D * 4); s_ln = new_slot((size_t)M * D * esz); s_qkv = new_slot((size_t)M * 3 * D * esz);
    s_att = new_slot((size_t)M * D * esz); s_fc = new_slot((size_t)M * F * esz); s_fc32 = new_slot(xlmr ? 0 : (size_t)M * F * 4);
    s_seq = new_slot((size_t)M * D * 4); s_pool_in = new_slot((size_t)B * D * 4); s_pooled = new_slot((size_t)B * od * 4);
    s_splitk = new_slot(256); s_kall = new_slot(); s_vtall = new_slot();
    s_flush = new_slot(autotune ? ((size_t)320 << 20) : 0);
    const int Bn = B, dt = dtype;
    const float eps = cfg.ln_eps;

    // ---- input sequence ------------------------------------------------------------------------------------------------------
    if (vision) {
      // x = conv1(image) as a GEMM over 14x14 patches (clip/model.py VisionTransformer.forward)
      const void* wp = W_("patch.weight");
      const float* cls = Wf("class_embedding"); const float* pos = Wf("positional_embedding");
      const int S = cfg.image_size, patch = cfg.patch;
      ops.push_back([=](hipStream_t st) { return launch_enc_patchify(ptr<float>(s_img), ptr(s_patch), Bn, S, patch, Kp, dt, st); });
      {
        IgemmParams p = igemm_gemm_problem(B * P, D, Kp, 0, IG_OUT_ROWMAJOR_F32);
        p.splitk = 1; p.Wp = wp;
        ops.push_back([=](hipStream_t st) {
          IgemmParams q = p;
          q.A0 = ptr(s_patch); q.out = ptr(s_pout); q.partial = ptr<float>(s_splitk);
          return launch_igemm(q, dt, st);
        });
      }
      ops.push_back([=](hipStream_t st) { return launch_enc_vision_assemble(ptr<float>(s_pout), cls, pos, ptr<float>(s_inp), Bn, P, D, st); });
      op_ln(s_inp, 0, D, M, D, eps, "ln_pre", s_inp, D, nullptr);
    } else {
      const float* te = Wf("token_embedding"); const float* pe = Wf("positional_embedding");
      const float* ty = xlmr ? Wf("token_type_embedding") : nullptr;
      const int vocab = cfg.vocab, pad = cfg.pad_id, maxp = cfg.max_pos;
      ops.push_back([=](hipStream_t st) {
        return launch_enc_embed(ptr<int>(s_tok), te, pe, ty, ptr<float>(s_inp), Bn, n, D, vocab, xlmr ? 1 : 0, pad, maxp, st);
      });
      if (xlmr) op_ln(s_inp, 0, D, M, D, eps, "embeddings_ln", s_inp, D, s_ln);
    }
    // ---- transformer -----------------------------------------------------------------------------------------------------------
    for (int l = 0; l < cfg.layers; ++l) {
      const std::string pfx = "layers." + std::to_string(l);
      if (!xlmr) op_ln(s_inp, 0, D, M, D, eps, pfx + ".ln_1", nullptr, 0, s_ln);
      op_linear(s_ln, 0, M, 3 * D, D, pfx + ".qkv", K22_ACT_NONE, s_qkv, 0, 3 * D, 0);
      const int causal = kind == K22_ENC_CLIP_TEXT ? 1 : 0;
      const bool masked = xlmr || cfg.key_mask != 0;   // the attention_mask: XLM-R always, CLIP text (under the causal triangle) by config
      if (!flash) ops.push_back([=](hipStream_t st) { return launch_enc_attention_generic(ptr(s_qkv), ptr(s_att), Bn, heads, n, hd, dt, st); });
      else op_flash_self_attention(s_qkv, s_att, B, heads, n, D, causal, masked ? s_valid : nullptr, n, n);
      op_linear(s_att, 0, M, D, D, pfx + ".proj", K22_ACT_NONE, s_inp, 0, D, 2);
      if (xlmr) {
        // BertSelfOutput: LayerNorm(dense(attn) + x);  BertIntermediate: GELU(dense);  BertOutput: LayerNorm(dense(h) + x)
        op_ln(s_inp, 0, D, M, D, eps, pfx + ".ln_1", s_inp, D, s_ln);
        op_linear(s_ln, 0, M, F, D, pfx + ".fc", K22_ACT_GELU, s_fc, 0, F, 0);
        op_linear(s_fc, 0, M, D, F, pfx + ".out", K22_ACT_NONE, s_inp, 0, D, 2);
        op_ln(s_inp, 0, D, M, D, eps, pfx + ".ln_2", s_inp, D, l + 1 < cfg.layers ? s_ln : nullptr);
      } else {
        op_ln(s_inp, 0, D, M, D, eps, pfx + ".ln_2", nullptr, 0, s_ln);
        op_linear(s_ln, 0, M, F, D, pfx + ".fc", K22_ACT_NONE, s_fc32, 0, F, 1);
        const int64_t nel = (int64_t)M * F;
        const int exact = cfg.hidden_act == 1 ? 1 : 0;
        ops.push_back([=](hipStream_t st) { return launch_enc_mlp_act(ptr<float>(s_fc32), ptr(s_fc), nel, exact, dt, st); });
        op_linear(s_fc, 0, M, D, F, pfx + ".out", K22_ACT_NONE, s_inp, 0, D, 2);
      }
    }
    // ---- heads ---------------------------------------------------------------------------------------------------------------
    if (kind == K22_ENC_CLIP_TEXT) {
      op_ln(s_inp, 0, D, M, D, eps, "ln_final", s_seq, D, nullptr);
      const int eos = cfg.eos_id;
      ops.push_back([=](hipStream_t st) { return launch_enc_gather_eot(ptr<int>(s_tok), ptr<float>(s_seq), ptr<float>(s_pool_in), Bn, n, D, eos, st); });
    } else if (vision) {
      op_ln(s_inp, 0, (int64_t)n * D, B, D, eps, "ln_post", s_pool_in, D, nullptr);      // class-token rows only
    } else {
      ops.push_back([=](hipStream_t st) {
        hipError_t e = hipMemcpyAsync(ptr(s_seq), ptr(s_inp), (size_t)M * D * 4, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return k22_set_error_hip(e, __FILE__, __LINE__);
        return launch_enc_masked_mean(ptr<float>(s_inp), ptr<float>(s_valid), ptr<float>(s_pool_in), Bn, n, D, st);
      });
    }
    op_linear_small(s_pool_in, D, B, od, D, "head", xlmr, K22_ACT_NONE, s_pooled, 0, od);
    return finish_plan();
  }
};

extern "C" {

int k22_encoder_create(const K22EncoderConfig* cfg, const K22Weight* weights, int n_weights, K22Encoder** out) {
  if (!cfg || !out || (!weights && n_weights > 0)) return k22_set_error(K22_EINVAL, "encoder_create: null argument");
  if (!k22_dtype_ok(cfg->dtype)) return k22_set_error(K22_EINVAL, "encoder_create: dtype");
  K22Encoder* m = new K22Encoder();
  m->cfg = *cfg; m->set_dtype(cfg->dtype);
  m->set_weights(weights, n_weights);
  *out = m;
  return K22_OK;
}
void k22_encoder_destroy(K22Encoder* m) { delete m; }

int k22_encoder_plan(K22Encoder* m, int B, size_t* workspace_bytes) {
  if (!m || !workspace_bytes) return k22_set_error(K22_EINVAL, "encoder_plan: null argument");
  int rc = m->plan(B);
  if (rc) return rc;
  *workspace_bytes = m->ws_bytes;
  return K22_OK;
}
int k22_encoder_bind(K22Encoder* m, void* workspace, size_t workspace_bytes) {
  if (!m) return k22_set_error(K22_EINVAL, "encoder_bind: null argument");
  return m->bind(workspace, workspace_bytes, "encoder_bind");
}

int k22_encoder_forward(K22Encoder* m, const int* tokens, const float* key_valid, const float* image, float* seq_out, float* pooled_out,
                        void* stream) {
  if (!m || !m->ws) return k22_set_error(K22_EINVAL, "encoder_forward: bind a workspace first");
  const K22EncoderConfig& c = m->cfg;
  const bool vision = c.kind == K22_ENC_CLIP_VISION, xlmr = c.kind == K22_ENC_XLMR, masked = xlmr || c.key_mask != 0;
  if (vision ? !image : !tokens) return k22_set_error(K22_EINVAL, "encoder_forward: tokens (text towers) / image (vision tower) is null");
  if (masked && !key_valid) return k22_set_error(K22_EINVAL, "encoder_forward: this tower (XLM-R, or CLIP text with key_mask) needs the attention mask");
  if (vision && seq_out) return k22_set_error(K22_EINVAL, "encoder_forward: the vision tower has no sequence output");
  if (!pooled_out) return k22_set_error(K22_EINVAL, "encoder_forward: pooled_out is null");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t M = (size_t)m->B * c.n_ctx;
  if (vision) { if (int rc = copy_d2d(m->ptr(m->s_img), image, (size_t)m->B * 3 * c.image_size * c.image_size * 4, st)) return rc; }
  else { if (int rc = copy_d2d(m->ptr(m->s_tok), tokens, M * 4, st)) return rc; }
  if (masked) { if (int rc = copy_d2d(m->ptr(m->s_valid), key_valid, M * 4, st)) return rc; }
  if (int rc = m->forward_list(st)) return rc;
  if (seq_out) { if (int rc = copy_d2d(seq_out, m->ptr(m->s_seq), M * c.width * 4, st)) return rc; }
  return copy_d2d(pooled_out, m->ptr(m->s_pooled), (size_t)m->B * c.out_dim * 4, st);
}

// ---- single-kernel entry points for the parity tests (include/k22.h); no product code calls them -------------------------------------
static bool aux_dtype_ok(int dt) { return dt == K22_BF16 || dt == K22_F16 || dt == K22_F32; }

int k22_enc_layernorm(const float* x, long ldx, const float* gain, const float* beta, float* out_f32, long ld_out, void* out_t, int rows,
                      int D, float eps, int dtype, void* stream) {
  if (!x || !gain || !beta || (!out_f32 && !out_t) || rows < 1 || D < 1 || ldx < D || (out_f32 && ld_out < D) || !aux_dtype_ok(dtype))
    return k22_set_error(K22_EINVAL, "enc_layernorm: bad argument");
  if (D > 2048) return k22_set_error(K22_EINVAL, "enc_layernorm: D <= 2048 (8 x 256 values per row)");
  return launch_layernorm_rows(x, ldx, gain, beta, out_f32, ld_out, out_t, rows, D, eps, dtype, reinterpret_cast<hipStream_t>(stream));
}
int k22_enc_embed(const int* tokens, const float* tok_emb, const float* pos_emb, const float* type_emb, float* x, int B, int n_ctx, int D,
                  int vocab, int xlmr, int pad_id, int max_pos, void* stream) {
  if (!tokens || !tok_emb || !pos_emb || !x || B < 1 || B > 65535 || n_ctx < 1 || D < 1 || vocab < 1)
    return k22_set_error(K22_EINVAL, "enc_embed: bad argument");
  if (xlmr && (max_pos < 2 || pad_id < 0 || pad_id >= max_pos)) return k22_set_error(K22_EINVAL, "enc_embed: max_pos / pad_id");
  return launch_enc_embed(tokens, tok_emb, pos_emb, type_emb, x, B, n_ctx, D, vocab, xlmr, pad_id, max_pos, reinterpret_cast<hipStream_t>(stream));
}
int k22_enc_gather_eot(const int* tokens, const float* x, float* out, int B, int n_ctx, int D, void* stream) {
  if (!tokens || !x || !out || B < 1 || n_ctx < 1 || D < 1) return k22_set_error(K22_EINVAL, "enc_gather_eot: bad argument");
  return launch_enc_gather_eot(tokens, x, out, B, n_ctx, D, 0, reinterpret_cast<hipStream_t>(stream));
}
int k22_enc_masked_mean(const float* x, const float* mask, float* out, int B, int n_ctx, int D, void* stream) {
  if (!x || !mask || !out || B < 1 || n_ctx < 1 || D < 1) return k22_set_error(K22_EINVAL, "enc_masked_mean: bad argument");
  return launch_enc_masked_mean(x, mask, out, B, n_ctx, D, reinterpret_cast<hipStream_t>(stream));
}
int k22_enc_patchify(const float* image, void* out, int B, int S, int patch, int Kp, int dtype, void* stream) {
  if (!image || !out || B < 1 || patch < 1 || S < patch || S % patch || Kp < 3 * patch * patch || !aux_dtype_ok(dtype))
    return k22_set_error(K22_EINVAL, "enc_patchify: bad argument");
  return launch_enc_patchify(image, out, B, S, patch, Kp, dtype, reinterpret_cast<hipStream_t>(stream));
}
int k22_enc_vision_assemble(const float* patch_out, const float* cls, const float* pos, float* x, int B, int P, int D, void* stream) {
  if (!patch_out || !cls || !pos || !x || B < 1 || B > 65535 || P < 1 || D < 1) return k22_set_error(K22_EINVAL, "enc_vision_assemble: bad argument");
  return launch_enc_vision_assemble(patch_out, cls, pos, x, B, P, D, reinterpret_cast<hipStream_t>(stream));
}
int k22_enc_mlp_act(const float* x, void* y, long n, int exact, int dtype, void* stream) {
  if (!x || !y || n < 1 || !aux_dtype_ok(dtype)) return k22_set_error(K22_EINVAL, "enc_mlp_act: bad argument");
  return launch_enc_mlp_act(x, y, n, exact ? 1 : 0, dtype, reinterpret_cast<hipStream_t>(stream));
}
int k22_enc_attention_generic(const void* qkv, void* out, int B, int heads, int n, int hd, int dtype, void* stream) {
  if (!qkv || !out || B < 1 || B > 65535 || heads < 1 || heads > 65535 || !aux_dtype_ok(dtype)) return k22_set_error(K22_EINVAL, "enc_attention_generic: bad argument");
  if (n < 1 || hd < 1 || !enc_ga_admits(n, hd, dtype == K22_F32 ? 4 : 2))
    return k22_set_error(K22_EINVAL, "enc_attention_generic: <= 128 channels per head, <= 512 tokens, <= 160 KB of LDS");
  return launch_enc_attention_generic(qkv, out, B, heads, n, hd, dtype, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
