// k22 — diffusion-prior transformer engine + its sampler step.
//
// Replaces PriorTransformer.forward (kandinsky2/model/prior.py:226-270) with its blocks (LayerNorm :48-54,
// MultiheadAttention / QKVMultiheadAttention :57-102, MLP :74-83, ResidualAttentionBlock :105-127) and the per-step
// arithmetic of PriorDiffusionModel.forward's sampling loop (:336-384: guided_model_fn CFG with per-sample scales,
// START_X mean, FIXED_SMALL variance, denoised_fn clamp, gaussian_diffusion.py:223-322, 352-382).
//
// MI355X mapping: the transformer is weight-streaming bound (2.0 GB of bf16 weights per forward for 162 token rows at
// bs = 1).  Its launch list and the ops of the plain path (Linear, LayerNorm, flash self-attention, the small fp32 Linears) are the
// transformer engines' shared ones (xf_plan.h); 16-bit engines run the blocks through the skinny path below instead, with the
// 81-token attention as one workgroup per (batch, head) out of LDS.  c_qkv rows are packed as Q | K | V planes
// (the reference keeps per-head [q|k|v] interleaved, prior.py:93-95).
#include "kernels.h"
#include "elementwise.h"
#include "../../include/k22.h"
#include "tuning.h"
#include "xf_plan.h"
#include "skinny.h"

#include <algorithm>
#include <deque>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

// ---- input sequence: rows 0..n_text-1 / n_text / n_text+1 / n_text+2 were written by the projections; add the
// positional embedding everywhere and put prd_emb in the last row (prior.py:248-256) -----------------------------
__global__ void prior_finish_input_kernel(float* inp, const float* pos, const float* prd, int B, int n_ctx, int D) {
  const int64_t total = (int64_t)B * n_ctx * D;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D), t = (int)((i / D) % n_ctx);
    const float base = (t == n_ctx - 1) ? prd[d] : inp[i];
    inp[i] = base + pos[(int64_t)t * D + d];
  }
}

// ---- one ancestral step of the prior (START_X mean, FIXED_SMALL variance) with classifier-free guidance -------------
// x, model_out, noise, x_out: [2*bs][D] with halves [cond | uncond]; scales [bs]; tab = (coef1, coef2, log_var, nonzero)
__global__ void prior_sampler_step_kernel(const float* x, const float* model_out, const float* noise, const float* scales,
                                          const float* tab, float clamp, float* x_out, int bs, int D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * bs * D) return;
  const int d = i % D, n = i / D, j = n % bs;
  const float c = model_out[(int64_t)j * D + d], u = model_out[(int64_t)(j + bs) * D + d];
  float x0 = u + scales[j] * (c - u);
  x0 = fminf(fmaxf(x0, -clamp), clamp);
  const float mean = __fadd_rn(__fmul_rn(tab[0], x0), __fmul_rn(tab[1], x[i]));
  x_out[i] = mean + tab[3] * expf(0.5f * tab[2]) * noise[i];
}

// ---- one DDIM step of the prior (gaussian_diffusion.py:477-519 with START_X, clip_denoised off, denoised_fn = clamp) with
// classifier-free guidance applied to the x0 prediction.  Layout as above; tab = (sqrt_recip_ac, sqrt_recipm1_ac, sqrt(ab_prev), sigma,
// sqrt(1 - ab_prev - sigma^2), i != 0, 0, 0).  noise == nullptr reads as 0 (an eta = 0 table: sigma = 0); x0_out may be nullptr.
// Every product, sum and quotient is rounded once, explicitly: the result does not depend on the compiler's contraction.
__global__ void prior_ddim_step_kernel(const float* x, const float* model_out, const float* noise, const float* scales,
                                       const float* tab, float clamp, float* x_out, float* x0_out, int bs, int D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * bs * D) return;
  const int d = i % D, n = i / D, j = n % bs;
  const float c = model_out[(int64_t)j * D + d], u = model_out[(int64_t)(j + bs) * D + d];
  float x0 = __fadd_rn(u, __fmul_rn(scales[j], __fsub_rn(c, u)));
  x0 = fminf(fmaxf(x0, -clamp), clamp);
  const float eps = __fdiv_rn(__fsub_rn(__fmul_rn(tab[0], x[i]), x0), tab[1]);
  const float mean = __fadd_rn(__fmul_rn(tab[2], x0), __fmul_rn(tab[4], eps));
  const float nz = noise ? noise[i] : 0.f;
  x_out[i] = __fadd_rn(mean, __fmul_rn(tab[5], __fmul_rn(tab[3], nz)));
  if (x0_out) x0_out[i] = x0;
}

// ---- launchers: the plan's ops and the single-kernel entry points (include/k22.h) go through the same code ------------------
static int launch_prior_finish_input(float* inp, const float* pos, const float* prd, int B, int n_ctx, int D, hipStream_t st) {
  hipLaunchKernelGGL(prior_finish_input_kernel, dim3(256), dim3(256), 0, st, inp, pos, prd, B, n_ctx, D);
  K22_CHECK_LAUNCH();
  return K22_OK;
}
static int launch_prior_sampler_step(const float* x, const float* model_out, const float* noise, const float* scales, const float* tab, float clamp,
                                     float* x_out, int bs, int D, hipStream_t st) {
  hipLaunchKernelGGL(prior_sampler_step_kernel, dim3((2 * bs * D + 255) / 256), dim3(256), 0, st, x, model_out, noise, scales, tab, clamp, x_out, bs, D);
  K22_CHECK_LAUNCH();
  return K22_OK;
}
static int launch_prior_ddim_step(const float* x, const float* model_out, const float* noise, const float* scales, const float* tab, float clamp,
                                  float* x_out, float* x0_out, int bs, int D, hipStream_t st) {
  hipLaunchKernelGGL(prior_ddim_step_kernel, dim3((2 * bs * D + 255) / 256), dim3(256), 0, st, x, model_out, noise, scales, tab, clamp, x_out, x0_out, bs, D);
  K22_CHECK_LAUNCH();
  return K22_OK;
}

struct K22Prior : XfPlan {   // tuned: every transformer Linear; graph: the ~250 launches of one forward
  K22PriorConfig cfg;
  int B = 0;
  Slot *s_x, *s_t, *s_temb, *s_te1, *s_txtemb, *s_txtenc, *s_txtencT, *s_valid, *s_mask, *s_inp, *s_ln, *s_qkv, *s_att, *s_fc,
      *s_lnlast, *s_out;
  // skinny path (round 6; skinny.hip): 16-bit engines run the transformer through the fragment-major weight-streaming GEMM, the fused
  // split-K finish + LayerNorm and the small-T attention: 7 launches per layer instead of 12.  K22_PRIOR_SKINNY=0 keeps the old path.
  bool skinny = false;
  bool wfrag_done = false;
  struct WFrag { const void* src; Slot* dst; int Npad, K; };
  std::vector<WFrag> wfrags;   // fragment-major copies of the transformer weights, written into the workspace once per bind
  // the ONE captured sampling loop of this handle (k22_prior_sample_loop); its key: kind, n_steps, clamp and every pointer
  LoopCache loop;

  // fragment-major weight copies of the skinny path: once per binding, before the first launch list that reads them
  int repack_once(hipStream_t st) {
    if (!skinny || wfrag_done) return K22_OK;
    for (auto& wf : wfrags) {
      int rc = launch_stream_repack(wf.src, ptr(wf.dst), wf.Npad, 1, wf.K, dtype, st);
      if (rc) return rc;
    }
    wfrag_done = true;
    return K22_OK;
  }

  // fragment-major copy of a transformer weight [Npad][K] (slot in the workspace, repacked at the first forward after a bind)
  Slot* wfrag_of(const std::string& name, int N, int K) {
    const int Npad = (N + 63) / 64 * 64;
    Slot* s = new_slot((size_t)Npad * K * esz);
    wfrags.push_back(WFrag{W_(name), s, Npad, K});
    return s;
  }
  // out = act(A . W^T + bias) through the skinny kernel; epi: SkinnyEpi; partial launches leave [splitk][M][N] in s_splitk
  void op_skinny(Slot* a, int M, int N, int K, const std::string& pfx, int act, int epi, int splitk, Slot* dst, int ldo) {
    Slot* wf = wfrag_of(pfx + ".weight", N, K);
    const float* bias = Wf(pfx + ".bias");
    if (epi == SK_EPI_PARTIAL) need(s_splitk, (size_t)splitk * M * N * 4);
    const int dt = dtype;
    ops.push_back([=](hipStream_t st) {
      SkinnyParams q = {};
      q.Af = ptr(a); q.Wf = ptr(wf); q.bias = epi == SK_EPI_PARTIAL ? nullptr : bias; q.out = dst ? ptr(dst) : nullptr; q.partial = ptr<float>(s_splitk);
      q.M = M; q.N = N; q.Npad = (N + 63) / 64 * 64; q.K = K; q.MA = (M + 31) / 32; q.splitk = splitk; q.epi = epi; q.act = act; q.ldo = ldo;
      return launch_skinny(q, dt, 0, 0, st);
    });
  }
  // x (+)= bias + sum of the split-K partials in s_splitk (splitk > 0); then LayerNorm `ln` of x into s_ln in A-fragment order (ln non-empty)
  void op_finish_ln(int M, int N, int splitk, const std::string& bias_name, const std::string& ln) {
    const float* bias = bias_name.empty() ? nullptr : Wf(bias_name);
    const float* g = ln.empty() ? nullptr : Wf(ln + ".weight");
    const float* bb = ln.empty() ? nullptr : Wf(ln + ".bias");
    const int dt = dtype;
    ops.push_back([=](hipStream_t st) {
      FinishLnParams q = {};
      q.partial = splitk > 0 ? ptr<float>(s_splitk) : nullptr; q.splitk = splitk; q.bias = bias; q.x = ptr<float>(s_inp); q.ldx = N;
      q.g = g; q.b = bb; q.yfrag = ptr(s_ln); q.M = M; q.N = N; q.MA = (M + 31) / 32; q.eps = 1e-5f;
      return launch_finish_ln(q, dt, st);
    });
  }

  int plan(int nB) {
    // validate before touching the current plan: rejected arguments leave the engine usable as it was
    const int D = cfg.xf_width, nt = cfg.text_ctx, nc = nt + 4, cd = cfg.clip_dim, cw = cfg.clip_xf_width, M = nB * nc;
    if (nB < 1 || nB > 8) return k22_set_error(K22_EINVAL, "prior: batch (2*bs) must be in 1..8 per engine call");
    if (D % 64 || D / cfg.xf_heads != 64) return k22_set_error(K22_EINVAL, "prior: 64 channels per head");
    if (D > 2048) return k22_set_error(K22_EINVAL, "prior: xf_width <= 2048 (LayerNorm keeps a row in 8 x 256 registers)");
    begin_plan();
    B = nB;
    ops.clear(); wfrags.clear(); wfrag_done = false; loop.drop();
    s_x = new_slot((size_t)B * cd * 4); s_t = new_slot((size_t)B * 4 + 64);
    s_temb = new_slot((size_t)B * D * 4); s_te1 = new_slot((size_t)B * D * 4);
    s_txtemb = new_slot((size_t)B * cd * 4); s_txtenc = new_slot((size_t)B * nt * cw * 4); s_txtencT = new_slot((size_t)B * nt * cw * esz);
    s_valid = new_slot((size_t)B * nt * 4); s_mask = new_slot((size_t)B * nc * nc * 4);
    skinny = env_flag("K22_PRIOR_SKINNY", 1) && esz == 2 && D <= 2048 && nc <= 128;
    const size_t Mp = (size_t)(M + 31) / 32 * 32;   // the fragment-major tensors hold whole 32-row atoms
    s_inp = new_slot((size_t)M * D * 4); s_ln = new_slot(Mp * D * esz); s_qkv = new_slot((size_t)M * 3 * D * esz);
    s_att = new_slot(Mp * D * esz); s_fc = new_slot(Mp * 4 * D * esz);
    s_lnlast = new_slot((size_t)B * D * 4); s_out = new_slot((size_t)B * cd * 4); s_splitk = new_slot(256);
    s_flush = new_slot(autotune ? ((size_t)320 << 20) : 0);
    s_kall = new_slot(); s_vtall = new_slot();
    const int Bn = B, dt = dtype;
    const size_t es = esz;

    // ---- input sequence (prior.py:238-256) ----------------------------------------------------------------
    {
      const float* freqs = Wf("time_freqs");
      ops.push_back([=](hipStream_t st) { return launch_timestep_embedding(ptr<float>(s_t), freqs, ptr<float>(s_temb), Bn, D / 2, st); });
      const int64_t ldseq = (int64_t)nc * D;   // row n_text + k of every sequence of s_inp: one row per batch element
      op_linear_small(s_temb, D, B, D, D, "time_embed.0", true, K22_ACT_SILU, s_te1, 0, D);
      op_linear_small(s_te1, D, B, D, D, "time_embed.2", true, K22_ACT_NONE, s_inp, (size_t)(nt + 1) * D * 4, ldseq);   // t_emb -> row n_text+1
      op_linear_small(s_txtemb, cd, B, D, cd, "text_emb_proj", true, K22_ACT_NONE, s_inp, (size_t)nt * D * 4, ldseq);    // text_emb -> row n_text
      op_linear_small(s_x, cd, B, D, cd, "clip_img_proj", true, K22_ACT_NONE, s_inp, (size_t)(nt + 2) * D * 4, ldseq);   // clip_img_proj(x) -> row n_text+2
      ops.push_back([=](hipStream_t st) { return launch_cast_rows(ptr<float>(s_txtenc), ptr(s_txtencT), Bn * nt, cw, cw, cw, dt, st); });
      // text_enc_proj: one GEMM per batch element straight into rows 0..n_text-1 of the sequence (fp32 out)
      for (int b = 0; b < B; ++b) {
        IgemmParams p = igemm_gemm_problem(nt, D, cw, 0, IG_OUT_ROWMAJOR_F32);
        p.splitk = 1;
        p.Wp = W_("text_enc_proj.weight"); p.bias = Wf("text_enc_proj.bias");
        ops.push_back([=](hipStream_t st) {
          IgemmParams q = p;
          q.A0 = ptr(s_txtencT) + (size_t)b * nt * cw * es; q.out = ptr<float>(s_inp) + (size_t)b * nc * D;
          return launch_igemm(q, dt, st);
        });
      }
      const float* pos = Wf("positional_embedding"); const float* prd = Wf("prd_emb");
      ops.push_back([=](hipStream_t st) { return launch_prior_finish_input(ptr<float>(s_inp), pos, prd, Bn, nc, D, st); });
    }
    // ---- transformer (prior.py:105-155) ------------------------------------------------------------------
    if (skinny) {
      // per layer: c_qkv -> attention -> c_proj (split-K partials) -> [finish + residual + ln_2] -> c_fc (+ GELU) -> mlp.c_proj (partials)
      // -> [finish + residual + next ln_1].  Split-K only where a finish launch runs anyway (N = D: 64-wide n-tiles alone would leave
      // three quarters of the CUs idle).
      const int heads = cfg.xf_heads;
      const int sk_proj = std::max(1, std::min(4, D / 512)), sk_fc2 = std::max(1, std::min(4, 4 * D / 512));
      static const int sk_qkv_env = [] { const char* e = getenv("K22_PRIOR_QKV_SPLIT"); return e ? atoi(e) : 1; }();   // measured: 1 (profiles/r06_skinny.txt: split 2 of c_qkv 22.4 us against 18.4)
      const int sk_qkv = std::max(1, std::min(std::min(4, sk_qkv_env), D / 512));
      op_finish_ln(M, D, 0, "", "transformer.resblocks.0.ln_1");
      for (int l = 0; l < cfg.xf_layers; ++l) {
        const std::string pfx = "transformer.resblocks." + std::to_string(l);
        // c_qkv: split-K partials whose finish (bias, one rounding) rides on the attention's staging loads (sk_qkv = 1: row-major T output)
        const float* qkv_bias = Wf(pfx + ".attn.c_qkv.bias");
        if (sk_qkv > 1) op_skinny(s_ln, M, 3 * D, D, pfx + ".attn.c_qkv", K22_ACT_NONE, SK_EPI_PARTIAL, sk_qkv, nullptr, 3 * D);
        else op_skinny(s_ln, M, 3 * D, D, pfx + ".attn.c_qkv", K22_ACT_NONE, SK_EPI_ROWMAJOR, 1, s_qkv, 3 * D);
        ops.push_back([=](hipStream_t st) {
          SmallAttnParams ap = {};
          ap.qkv = ptr(s_qkv); ap.ldq = 3 * D;
          if (sk_qkv > 1) { ap.part = ptr<float>(s_splitk); ap.nsplit = sk_qkv; ap.bias = qkv_bias; } ap.out = ptr(s_att); ap.ldo = D; ap.out_frag = 1; ap.MA = (M + 31) / 32;
          ap.B = Bn; ap.H = heads; ap.T = nc; ap.scale = 0.125f; ap.causal = 1; ap.key_valid = ptr<float>(s_valid); ap.kv_ld = nt; ap.kv_n = nt;
          return launch_small_attention(ap, dt, st);
        });
        op_skinny(s_att, M, D, D, pfx + ".attn.c_proj", K22_ACT_NONE, SK_EPI_PARTIAL, sk_proj, nullptr, D);
        op_finish_ln(M, D, sk_proj, pfx + ".attn.c_proj.bias", pfx + ".ln_2");
        op_skinny(s_ln, M, 4 * D, D, pfx + ".mlp.c_fc", K22_ACT_GELU, SK_EPI_AFRAG, 1, s_fc, 4 * D);
        op_skinny(s_fc, M, D, 4 * D, pfx + ".mlp.c_proj", K22_ACT_NONE, SK_EPI_PARTIAL, sk_fc2, nullptr, D);
        op_finish_ln(M, D, sk_fc2, pfx + ".mlp.c_proj.bias", l + 1 < cfg.xf_layers ? "transformer.resblocks." + std::to_string(l + 1) + ".ln_1" : std::string());
      }
    } else
    for (int l = 0; l < cfg.xf_layers; ++l) {
      const std::string pfx = "transformer.resblocks." + std::to_string(l);
      op_ln(s_inp, 0, D, M, D, 1e-5f, pfx + ".ln_1", nullptr, 0, s_ln);
      op_linear(s_ln, 0, M, 3 * D, D, pfx + ".attn.c_qkv", K22_ACT_NONE, s_qkv, 0, 3 * D, 0);
      // attention: the UNet's flash kernel (attention.hip) with the prior's mask (prior.py:262-263) — the additive
      // mask is -inf exactly for padding keys and for keys after the query, the 4 extra positions are always valid
      op_flash_self_attention(s_qkv, s_att, B, cfg.xf_heads, nc, D, 1, s_valid, nt, nt);
      op_linear(s_att, 0, M, D, D, pfx + ".attn.c_proj", K22_ACT_NONE, s_inp, 0, D, 2);
      op_ln(s_inp, 0, D, M, D, 1e-5f, pfx + ".ln_2", nullptr, 0, s_ln);
      op_linear(s_ln, 0, M, 4 * D, D, pfx + ".mlp.c_fc", K22_ACT_GELU, s_fc, 0, 4 * D, 0);
      op_linear(s_fc, 0, M, D, 4 * D, pfx + ".mlp.c_proj", K22_ACT_NONE, s_inp, 0, D, 2);
    }
    // ---- final_ln on the last token + out_proj (prior.py:266-269) -------------------------------------------
    if (cfg.xf_final_ln) {
      op_ln(s_inp, (size_t)(nc - 1) * D * 4, (int64_t)nc * D, B, D, 1e-5f, "final_ln", s_lnlast, D, nullptr);
    } else {
      ops.push_back([=](hipStream_t st) {
        hipError_t e = hipMemcpy2DAsync(ptr(s_lnlast), (size_t)D * 4, ptr(s_inp) + (size_t)(nc - 1) * D * 4, (size_t)nc * D * 4, (size_t)D * 4, Bn,
                                        hipMemcpyDeviceToDevice, st);
        return e == hipSuccess ? K22_OK : k22_set_error_hip(e, __FILE__, __LINE__);
      });
    }
    op_linear_small(s_lnlast, D, B, cd, D, "out_proj", true, K22_ACT_NONE, s_out, 0, cd);
    return finish_plan();
  }
};

extern "C" {

int k22_prior_create(const K22PriorConfig* cfg, const K22Weight* weights, int n_weights, K22Prior** out) {
  if (!cfg || !out) return k22_set_error(K22_EINVAL, "prior_create: null argument");
  if (!k22_dtype_ok(cfg->dtype)) return k22_set_error(K22_EINVAL, "prior_create: dtype");
  K22Prior* m = new K22Prior();
  m->cfg = *cfg; m->set_dtype(cfg->dtype);
  m->set_weights(weights, n_weights);
  *out = m;
  return K22_OK;
}
int k22_prior_tuning_report(const K22Prior* m, char* buf, size_t cap) {
  if (!m || !buf || cap == 0) return k22_set_error(K22_EINVAL, "prior_tuning_report: null argument");
  snprintf(buf, cap, "%s", tuning_report_text(m->tuned).c_str());
  return K22_OK;
}
void k22_prior_destroy(K22Prior* m) { delete m; }

int k22_prior_plan(K22Prior* m, int B, size_t* workspace_bytes) {
  if (!m || !workspace_bytes) return k22_set_error(K22_EINVAL, "prior_plan: null argument");
  int rc = m->plan(B);
  if (rc) return rc;
  *workspace_bytes = m->ws_bytes;
  return K22_OK;
}
int k22_prior_bind(K22Prior* m, void* workspace, size_t workspace_bytes) {
  if (!m) return k22_set_error(K22_EINVAL, "prior_bind: null argument");
  if (int rc = m->bind(workspace, workspace_bytes, "prior_bind")) return rc;
  m->wfrag_done = false;
  m->loop.drop();   // its nodes hold the old workspace's addresses
  return K22_OK;
}
int k22_prior_forward(K22Prior* m, const float* x, const float* timesteps, const float* text_emb, const float* text_enc,
                      const float* key_valid, float* out, void* stream) {
  if (!m || !m->ws) return k22_set_error(K22_EINVAL, "prior_forward: bind a workspace first");
  if (!x || !timesteps || !text_emb || !text_enc || !key_valid || !out) return k22_set_error(K22_EINVAL, "prior_forward: null argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const K22PriorConfig& c = m->cfg;
  if (int rc = copy_d2d(m->ptr(m->s_x), x, (size_t)m->B * c.clip_dim * 4, st)) return rc;
  if (int rc = copy_d2d(m->ptr(m->s_t), timesteps, (size_t)m->B * 4, st)) return rc;
  if (int rc = copy_d2d(m->ptr(m->s_txtemb), text_emb, (size_t)m->B * c.clip_dim * 4, st)) return rc;
  if (int rc = copy_d2d(m->ptr(m->s_txtenc), text_enc, (size_t)m->B * c.text_ctx * c.clip_xf_width * 4, st)) return rc;
  if (int rc = copy_d2d(m->ptr(m->s_valid), key_valid, (size_t)m->B * c.text_ctx * 4, st)) return rc;
  if (int rc = m->repack_once(st)) return rc;
  if (int rc = m->forward_list(st)) return rc;
  return copy_d2d(out, m->ptr(m->s_out), (size_t)m->B * c.clip_dim * 4, st);
}

int k22_prior_sampler_step(const float* x, const float* model_out, const float* noise, const float* scales, const float* table_row,
                           float clamp, float* x_out, int bs, int D, void* stream) {
  if (!x || !model_out || !noise || !scales || !table_row || !x_out || bs < 1 || D < 1) return k22_set_error(K22_EINVAL, "prior_sampler_step: bad argument");
  return launch_prior_sampler_step(x, model_out, noise, scales, table_row, clamp, x_out, bs, D, reinterpret_cast<hipStream_t>(stream));
}

int k22_prior_ddim_step(const float* x, const float* model_out, const float* noise, const float* scales, const float* table_row, float clamp,
                        float* x_out, float* x0_out, int bs, int D, void* stream) {
  if (!x || !model_out || !scales || !table_row || !x_out || bs < 1 || D < 1) return k22_set_error(K22_EINVAL, "prior_ddim_step: bad argument");
  return launch_prior_ddim_step(x, model_out, noise, scales, table_row, clamp, x_out, x0_out, bs, D, reinterpret_cast<hipStream_t>(stream));
}

// The whole sampling loop of PriorDiffusionModel.forward (prior.py:336-384 -> p_sample_loop / ddim_sample_loop) on this handle's plan: the
// conditioning goes into the plan's slots once, then per step  [x_half | x_half] -> s_x, timesteps[k] -> s_t, the launch list, the step
// kernel of `kind` from s_out into the other of x / x_tmp.  Eagerly, or as ONE captured graph (a single chain on the capture stream).
int k22_prior_sample_loop(K22Prior* m, int kind, float* x, float* x_tmp, float* x0_out, const float* timesteps, const float* table,
                          const float* noise_seq, const float* scales, const float* text_emb, const float* text_enc, const float* key_valid,
                          float clamp, int n_steps, int use_graph, void* stream) {
  // arguments first, the handle's state after them: a refused call names its own mistake, and leaves the handle and its captured loop alone
  if (!m || !x || !x_tmp || !timesteps || !table || !scales || !text_emb || !text_enc || !key_valid) return k22_set_error(K22_EINVAL, "prior_sample_loop: null argument");
  if (kind != K22_PRIOR_LOOP_ANCESTRAL && kind != K22_PRIOR_LOOP_DDIM)
    return k22_set_error(K22_EINVAL, "prior_sample_loop: kind must be K22_PRIOR_LOOP_ANCESTRAL or K22_PRIOR_LOOP_DDIM");
  if (n_steps < 1) return k22_set_error(K22_EINVAL, "prior_sample_loop: n_steps must be >= 1");
  if (kind == K22_PRIOR_LOOP_ANCESTRAL && !noise_seq) return k22_set_error(K22_EINVAL, "prior_sample_loop: the ancestral loop needs noise_seq (NULL is the DDIM loop at eta = 0)");
  if (!m->ws) return k22_set_error(K22_EINVAL, "prior_sample_loop: bind a workspace first");
  if (m->B % 2) return k22_set_error(K22_EINVAL, "prior_sample_loop: the batch is the CFG batch [cond | uncond] (even)");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const K22PriorConfig& c = m->cfg;
  const int B = m->B, bs = B / 2, D = c.clip_dim;
  const size_t lat = (size_t)B * D, half = (size_t)bs * D * sizeof(float);
  auto conditioning = [&](hipStream_t s) -> int {
    if (int rc = copy_d2d(m->ptr(m->s_txtemb), text_emb, (size_t)B * D * 4, s)) return rc;
    if (int rc = copy_d2d(m->ptr(m->s_txtenc), text_enc, (size_t)B * c.text_ctx * c.clip_xf_width * 4, s)) return rc;
    return copy_d2d(m->ptr(m->s_valid), key_valid, (size_t)B * c.text_ctx * 4, s);
  };
  auto model_input = [&](const float* cur, int k, hipStream_t s) -> int {   // guided_model_fn: the transformer sees the first half twice
    if (int rc = copy_d2d(m->ptr(m->s_x), cur, half, s)) return rc;
    if (int rc = copy_d2d(m->ptr(m->s_x) + half, cur, half, s)) return rc;
    return copy_d2d(m->ptr(m->s_t), timesteps + (size_t)k * B, (size_t)B * 4, s);
  };
  if (int rc = m->repack_once(st)) return rc;
  if (int rc = m->first_use(st, [&](hipStream_t s) -> int { if (int rc = conditioning(s)) return rc; return model_input(x, 0, s); })) return rc;
  auto body = [&](hipStream_t s) -> int {
    if (int rc = conditioning(s)) return rc;
    float* cur = x; float* nxt = x_tmp;
    for (int k = 0; k < n_steps; ++k) {
      if (int rc = model_input(cur, k, s)) return rc;
      if (int rc = m->run_ops(s)) return rc;
      const float* out = m->ptr<float>(m->s_out);
      const float* nz = noise_seq ? noise_seq + (size_t)k * lat : nullptr;
      int rc;
      if (kind == K22_PRIOR_LOOP_DDIM) rc = launch_prior_ddim_step(cur, out, nz, scales, table + (size_t)k * 8, clamp, nxt, x0_out, bs, D, s);
      else rc = launch_prior_sampler_step(cur, out, nz, scales, table + (size_t)k * 4, clamp, nxt, bs, D, s);
      if (rc) return rc;
      float* t_ = cur; cur = nxt; nxt = t_;
    }
    if (cur != x) return copy_d2d(x, cur, lat * sizeof(float), s);
    return K22_OK;
  };
  return m->loop.run(m->cap, {(unsigned long long)kind, (unsigned long long)n_steps, loop_key_bits(clamp), loop_key_ptr(x), loop_key_ptr(x_tmp),
      loop_key_ptr(x0_out), loop_key_ptr(timesteps), loop_key_ptr(table), loop_key_ptr(noise_seq), loop_key_ptr(scales), loop_key_ptr(text_emb),
      loop_key_ptr(text_enc), loop_key_ptr(key_valid)}, use_graph, st, body);
}

// ---- single-kernel entry points for the parity tests (include/k22.h); no product code calls them -------------------------
int k22_prior_layernorm(const float* x, long ldx, const float* gain, const float* beta, void* y, int rows, int D, int to_f32, int dtype,
                        void* stream) {
  if (!x || !gain || !beta || !y || rows < 1 || D < 1 || ldx < D || (dtype != K22_BF16 && dtype != K22_F16 && dtype != K22_F32))
    return k22_set_error(K22_EINVAL, "prior_layernorm: bad argument");
  if (D > 2048) return k22_set_error(K22_EINVAL, "prior_layernorm: D <= 2048 (8 x 256 values per row)");
  return launch_layernorm_rows(x, ldx, gain, beta, to_f32 ? reinterpret_cast<float*>(y) : nullptr, D, to_f32 ? nullptr : y, rows, D, 1e-5f, dtype,
                               reinterpret_cast<hipStream_t>(stream));
}
int k22_prior_finish_input(float* inp, const float* pos, const float* prd, int B, int n_ctx, int D, void* stream) {
  if (!inp || !pos || !prd || B < 1 || n_ctx < 1 || D < 1) return k22_set_error(K22_EINVAL, "prior_finish_input: bad argument");
  return launch_prior_finish_input(inp, pos, prd, B, n_ctx, D, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
