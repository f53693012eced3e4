// k22 — MoVQ decoder engine: latent [B,4,h,w] -> image [B,3,8h,8w]  (MOVQ.decode, kandinsky2/vqgan/autoencoder.py:182-185;
// MOVQDecoder.forward, kandinsky2/vqgan/movq_modules.py:326-357), and MoVQ ENCODER engine: image [B,3,H,W] -> latent
// [B,4,H/8,W/8] (MOVQ.encode, autoencoder.py:176-180; Encoder.forward, kandinsky2/vqgan/vqgan_blocks.py:335-367: the
// img2img / inpainting pre-step, kandinsky2_1_model.py:458-469, 519-534).  One K22MoVQ handle carries one plan of either.
//
// Same building blocks as the UNet engine: NHWC activations in a caller-owned workspace, every 3x3 conv input
// written zero-bordered by the (Spatial)Norm-apply kernel, convolutions / 1x1 projections through launch_igemm
// (LDS-resident halo kernel where the row fits the LDS, generic implicit GEMM at the wide levels), GroupNorm
// statistics by gn_stats + gn_coeff.  MoVQ specifics:
//   * SpatialNorm: GN(f) * conv_y(zq) + conv_b(zq), zq = raw latent nearest-resized — evaluated inside the apply
//     kernel from the 4-channel latent (movq_kernels.hip), nothing is materialised;
//   * AttnBlock (single head, C = 512, T = h*w keys): q / k projections as GEMMs, v projected TRANSPOSED by swapping
//     the GEMM operands (V^T = Wv . h^T, so it is directly the [N][K] operand of the P.V GEMM), scores = Q K^T as a
//     GEMM per image into a [T][T] buffer (the reference materialises it too, movq_modules.py:214-218), row softmax,
//     O = P V^T^T + bv (softmax rows sum to 1, so the v bias moves behind the product), proj_out + residual.
//     Second form ("fused", k22_movq_set_attention): scores, softmax and P V as ONE launch of movq_attention.hip for all images;
//     the [T][T] buffer is not part of such a plan.
#include "kernels.h"
#include "elementwise.h"
#include "../../include/k22.h"
#include "plan.h"

#include <deque>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

namespace {
typedef std::function<int(hipStream_t)> MOp;
struct MAct { Slot* s = nullptr; int C = 0, H = 0, W = 0; };
}  // namespace

struct K22MoVQ : PlanBase {
  K22MoVQConfig cfg;
  int B = 0, h0 = 0, w0 = 0;
  std::vector<MOp> ops;
  Slot *s_zq, *s_xin, *s_part, *s_coeff, *s_P, *s_U, *s_S, *s_N, *s_Q, *s_K, *s_VT, *s_SC, *s_O, *s_splitk, *s_out, *s_z;
  Slot *s_img = nullptr, *s_lat = nullptr;   // encoder plan: fp32 NCHW image in, fp32 NCHW latent out
  bool enc = false;                           // the current plan is the encoder (plain GroupNorm instead of SpatialNorm)
  int encH = 0, encW = 0;
  Slot* s_h[3];
  int hrot = 0;
  int attn_mode = K22_MOVQ_ATTN_AUTO;         // k22_movq_set_attention: read when a plan is built
  static constexpr int ATTN_AUTO_T = 16384;   // auto: fused above this many keys (the largest T the scores form is tested and measured at)

  // the form of an AttnBlock of width C over T keys under attn_mode; never a function of B (images are independent chains)
  bool attn_fused(int T, int C) const {
    if (attn_mode == K22_MOVQ_ATTN_SCORES) return false;
    if (attn_mode == K22_MOVQ_ATTN_FUSED) return true;
    return T > ATTN_AUTO_T && movq_attention_admits_c(C) && movq_attention_admits_t(T);
  }
  // the widths of the plan's AttnBlocks: mid (the deepest level's width) and every level with attention
  bool attn_widths_admitted() const {
    const int nres = cfg.n_levels;
    if (!movq_attention_admits_c(cfg.ch * cfg.ch_mult[nres - 1])) return false;
    for (int lvl = 0; lvl < nres; ++lvl)
      if (((cfg.attn_levels >> lvl) & 1) && !movq_attention_admits_c(cfg.ch * cfg.ch_mult[lvl])) return false;
    return true;
  }
  // "fused" asked for a plan the kernel does not admit: refused before the current plan is touched.  T0: keys at the deepest level
  // (every AttnBlock of a plan runs there or, in the encoder, at a level whose key count is 4^k T0).
  int check_fused(int64_t T0) {
    if (attn_mode != K22_MOVQ_ATTN_FUSED) return K22_OK;
    if (!attn_widths_admitted()) return k22_set_error(K22_EINVAL, "movq: fused attention needs AttnBlock widths of 128, 256, 384 or 512 channels");
    if (T0 < 64 || T0 % 64) return k22_set_error(K22_EINVAL, "movq: fused attention needs h * w to be a positive multiple of 64");
    return K22_OK;
  }

  Slot* next_h() { Slot* s = s_h[hrot]; hrot = (hrot + 1) % 3; return s; }
  static int ilog2(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }

  // generic launch of one igemm problem with the library's heuristics
  void push_igemm(IgemmParams p, std::function<void(IgemmParams&)> bind) {
    p.splitk = igemm_choose_splitk(p, dtype);
    if (p.splitk > 1) need(s_splitk, (size_t)p.splitk * p.M * p.N * sizeof(float));
    const int dt = dtype;
    ops.push_back([=](hipStream_t st) {
      IgemmParams q = p;
      bind(q);
      q.partial = ptr<float>(s_splitk);
      return launch_igemm(q, dt, st);
    });
  }

  // SpatialNorm (+act) -> dst (zero-bordered when pad)
  void op_sn(const MAct& in, const std::string& pfx, int act, int pad, Slot* dst) {
    const int Bn = B, C = in.C, HW = in.H * in.W;
    need(s_part, (size_t)Bn * gn_nsplit(Bn, HW) * C * 2 * sizeof(float));
    need(s_coeff, (size_t)Bn * C * 2 * sizeof(float));
    need(dst, (size_t)Bn * (in.H + 2 * pad) * (in.W + 2 * pad) * C * esz);
    const float* gamma = Wf(pfx + ".norm_layer.weight"); const float* beta = Wf(pfx + ".norm_layer.bias");
    const float* wy = Wf(pfx + ".conv_y.weight"); const float* by = Wf(pfx + ".conv_y.bias");
    const float* wb = Wf(pfx + ".conv_b.weight"); const float* bb = Wf(pfx + ".conv_b.bias");
    const MAct a = in;
    const int dt = dtype, shift = ilog2(in.H / h0), hh = h0, ww = w0;
    ops.push_back([=](hipStream_t st) {
      int rc = launch_gn_stats_coeff(ptr(a.s), nullptr, C, 0, Bn, HW, 1e-6f, gamma, beta, nullptr, 0, ptr<float>(s_part), ptr<float>(s_coeff), dt, st);
      if (rc) return rc;
      SpatialNormParams np;
      np.x = ptr(a.s); np.coeff = ptr<float>(s_coeff); np.zq = ptr<float>(s_zq); np.wy = wy; np.by = by; np.wb = wb; np.bb = bb;
      np.out = ptr(dst); np.B = Bn; np.H = a.H; np.W = a.W; np.C = C; np.h0 = hh; np.w0 = ww; np.shift = shift; np.act = act; np.pad = pad;
      return launch_spatialnorm_apply(np, dt, st);
    });
  }

  // plain GroupNorm (vqgan_blocks.Normalize: 32 groups, eps 1e-6, affine) (+act) -> dst (zero-bordered when pad)
  void op_gn(const MAct& in, const std::string& pfx, int act, int pad, Slot* dst) {
    const int Bn = B, C = in.C, HW = in.H * in.W;
    need(s_part, (size_t)Bn * gn_nsplit(Bn, HW) * C * 2 * sizeof(float));
    need(s_coeff, (size_t)Bn * C * 2 * sizeof(float));
    need(dst, (size_t)Bn * (in.H + 2 * pad) * (in.W + 2 * pad) * C * esz);
    const float* gamma = Wf(pfx + ".weight"); const float* beta = Wf(pfx + ".bias");
    const MAct a = in;
    const int dt = dtype;
    ops.push_back([=](hipStream_t st) {
      int rc = launch_gn_stats_coeff(ptr(a.s), nullptr, C, 0, Bn, HW, 1e-6f, gamma, beta, nullptr, 0, ptr<float>(s_part), ptr<float>(s_coeff), dt, st);
      if (rc) return rc;
      GnApplyParams ap = {};
      ap.x0 = ptr(a.s); ap.x1 = nullptr; ap.C0 = C; ap.C1 = 0; ap.B = Bn; ap.H = a.H; ap.W = a.W; ap.mode = 0; ap.pad = pad; ap.act = act;
      ap.coeff = ptr<float>(s_coeff); ap.out = ptr(dst);
      return launch_gn_apply(ap, dt, st);
    });
  }
  void op_norm(const MAct& in, const std::string& pfx, int act, int pad, Slot* dst) {
    if (enc) op_gn(in, pfx, act, pad, dst);
    else op_sn(in, pfx, act, pad, dst);
  }

  void op_conv3(Slot* src, int H, int W, int Cin, int Cout, const std::string& pfx, Slot* residual, Slot* dst, int out_mode) {
    IgemmParams p = igemm_conv3_problem(B, H, W, Cin, Cout, out_mode);
    p.Wp = W_(pfx + ".weight"); p.bias = Wf(pfx + ".bias");
    need(dst, out_mode == IG_OUT_ROWMAJOR ? (size_t)p.M * Cout * esz : (size_t)p.M * Cout * sizeof(float));
    push_igemm(p, [=](IgemmParams& q) { q.A0 = ptr(src); q.residual = residual ? ptr(residual) : nullptr; q.out = ptr(dst); });
  }

  void op_gemm(Slot* a, int M, int N, int K, const std::string& pfx, Slot* residual, Slot* dst) {
    IgemmParams p = igemm_gemm_problem(M, N, K, 0);
    p.Wp = W_(pfx + ".weight"); p.bias = Wf(pfx + ".bias");
    need(dst, (size_t)M * N * esz);
    push_igemm(p, [=](IgemmParams& q) { q.A0 = ptr(a); q.residual = residual ? ptr(residual) : nullptr; q.out = ptr(dst); });
  }

  // ResnetBlock (movq_modules.py:120-182), temb is None in the decoder
  MAct resblock(const std::string& pfx, const MAct& in, int Cout) {
    const int Cin = in.C, H = in.H, W = in.W;
    op_norm(in, pfx + ".norm1", K22_ACT_SILU, 1, s_P);
    op_conv3(s_P, H, W, Cin, Cout, pfx + ".conv1", nullptr, s_U, IG_OUT_ROWMAJOR);
    MAct u; u.s = s_U; u.C = Cout; u.H = H; u.W = W;
    op_norm(u, pfx + ".norm2", K22_ACT_SILU, 1, s_P);
    Slot* skip = in.s;
    if (Cin != Cout) {
      op_gemm(in.s, B * H * W, Cout, Cin, pfx + ".nin_shortcut", nullptr, s_S);
      skip = s_S;
    }
    Slot* d = next_h();
    if (d == in.s) d = next_h();
    op_conv3(s_P, H, W, Cout, Cout, pfx + ".conv2", skip, d, IG_OUT_ROWMAJOR);
    MAct out; out.s = d; out.C = Cout; out.H = H; out.W = W;
    return out;
  }

  // AttnBlock (movq_modules.py:185-225)
  MAct attnblock(const std::string& pfx, const MAct& in) {
    const int C = in.C, T = in.H * in.W, Bn = B, dt = dtype;
    const size_t es = esz;
    if (T % 64 || C % 64) { if (err.empty()) err = "movq attention: h*w and C must be multiples of 64"; }
    op_norm(in, pfx + ".norm", K22_ACT_NONE, 0, s_N);
    op_gemm(s_N, B * T, C, C, pfx + ".q", nullptr, s_Q);
    op_gemm(s_N, B * T, C, C, pfx + ".k", nullptr, s_K);
    need(s_VT, (size_t)B * C * T * esz);
    need(s_O, (size_t)B * T * C * esz);
    const void* wv = W_(pfx + ".v.weight"); const float* bv = Wf(pfx + ".v.bias");
    Slot* d = next_h();
    if (d == in.s) d = next_h();
    MAct out; out.s = d; out.C = C; out.H = in.H; out.W = in.W;
    // V^T_b [C][T] = Wv [C][C] . N_b [T][C]^T
    auto push_vt = [&](int b) {
      IgemmParams p = igemm_gemm_problem(C, T, C, 0);   // (T % 64 == 0: Npad = T)
      push_igemm(p, [=](IgemmParams& q) { q.A0 = wv; q.Wp = ptr(s_N) + (size_t)b * T * C * es; q.bias = nullptr; q.out = ptr(s_VT) + (size_t)b * C * T * es; });
    };
    if (attn_fused(T, C)) {
      for (int b = 0; b < Bn; ++b) push_vt(b);
      ops.push_back([=](hipStream_t st) { return launch_movq_attention(ptr(s_Q), ptr(s_K), ptr(s_VT), bv, ptr(s_O), Bn, T, C, dt, st); });
      op_gemm(s_O, B * T, C, C, pfx + ".proj_out", in.s, d);
      return out;
    }
    need(s_SC, (size_t)B * T * T * esz);
    for (int b = 0; b < Bn; ++b) {
      push_vt(b);
      // scores_b [T][T] = Q_b . K_b^T
      {
        IgemmParams p = igemm_gemm_problem(T, T, C, 0);
        push_igemm(p, [=](IgemmParams& q) { q.A0 = ptr(s_Q) + (size_t)b * T * C * es; q.Wp = ptr(s_K) + (size_t)b * T * C * es; q.bias = nullptr;
                                            q.out = ptr(s_SC) + (size_t)b * T * T * es; });
      }
    }
    const float scale = 1.0f / sqrtf((float)C);
    ops.push_back([=](hipStream_t st) { return launch_softmax_rows(ptr(s_SC), (int64_t)Bn * T, T, scale, dt, st); });
    for (int b = 0; b < Bn; ++b) {
      IgemmParams p = igemm_gemm_problem(T, C, T, 0);
      push_igemm(p, [=](IgemmParams& q) { q.A0 = ptr(s_SC) + (size_t)b * T * T * es; q.Wp = ptr(s_VT) + (size_t)b * C * T * es; q.bias = bv;
                                          q.out = ptr(s_O) + (size_t)b * T * C * es; });
    }
    op_gemm(s_O, B * T, C, C, pfx + ".proj_out", in.s, d);
    return out;
  }

  int plan(int nB, int nh, int nw) {
    // validate before touching the current plan: rejected arguments leave the engine usable as it was
    if (nB < 1 || nh < 1 || nw < 1) return k22_set_error(K22_EINVAL, "movq: empty input");
    if (int rc = check_fused((int64_t)nh * nw)) return rc;
    begin_plan();
    B = nB; h0 = nh; w0 = nw; enc = false;
    ops.clear(); hrot = 0;
    const int nres = cfg.n_levels;
    s_z = new_slot((size_t)B * 4 * h0 * w0 * 4);
    s_zq = new_slot((size_t)B * h0 * w0 * 4 * 4);
    s_xin = new_slot((size_t)B * (h0 + 2) * (w0 + 2) * 64 * esz);
    s_part = new_slot(); s_coeff = new_slot(); s_P = new_slot(); s_U = new_slot(); s_S = new_slot(); s_N = new_slot();
    s_Q = new_slot(); s_K = new_slot(); s_VT = new_slot(); s_SC = new_slot(); s_O = new_slot(); s_splitk = new_slot(256);
    for (int i = 0; i < 3; ++i) s_h[i] = new_slot();
    const int H8 = h0 << (nres - 1), W8 = w0 << (nres - 1);
    s_out = new_slot((size_t)B * cfg.out_ch * H8 * W8 * 4);

    // post_quant_conv + layouts
    {
      const float* wpq = Wf("post_quant_conv.weight"); const float* bpq = Wf("post_quant_conv.bias");
      const int Bn = B, hh = h0, ww = w0, dt = dtype;
      ops.push_back([=](hipStream_t st) { return launch_movq_prepare(ptr<float>(s_z), wpq, bpq, ptr<float>(s_zq), ptr(s_xin), Bn, hh, ww, 64, dt, st); });
    }
    int block_in = cfg.ch * cfg.ch_mult[nres - 1];
    MAct hcur;
    {
      Slot* d = next_h();
      op_conv3(s_xin, h0, w0, 64, block_in, "decoder.conv_in", nullptr, d, IG_OUT_ROWMAJOR);
      hcur.s = d; hcur.C = block_in; hcur.H = h0; hcur.W = w0;
    }
    hcur = resblock("decoder.mid.block_1", hcur, block_in);
    hcur = attnblock("decoder.mid.attn_1", hcur);
    hcur = resblock("decoder.mid.block_2", hcur, block_in);
    for (int lvl = nres - 1; lvl >= 0; --lvl) {
      const int block_out = cfg.ch * cfg.ch_mult[lvl];
      const bool attn = (cfg.attn_levels >> lvl) & 1;
      for (int i = 0; i <= cfg.num_res_blocks; ++i) {
        const std::string pfx = "decoder.up." + std::to_string(lvl);
        hcur = resblock(pfx + ".block." + std::to_string(i), hcur, block_out);
        block_in = block_out;
        if (attn) hcur = attnblock(pfx + ".attn." + std::to_string(i), hcur);
      }
      if (lvl != 0) {
        // Upsample: nearest x2 + conv3x3
        const MAct a = hcur;
        const int Bn = B, dt = dtype, C = hcur.C;
        need(s_P, (size_t)B * (2 * a.H + 2) * (2 * a.W + 2) * C * esz);
        ops.push_back([=](hipStream_t st) { return launch_upsample2_pad(ptr(a.s), ptr(s_P), Bn, a.H, a.W, C, dt, st); });
        Slot* d = next_h();
        if (d == a.s) d = next_h();
        op_conv3(s_P, 2 * a.H, 2 * a.W, C, C, "decoder.up." + std::to_string(lvl) + ".upsample.conv", nullptr, d, IG_OUT_ROWMAJOR);
        hcur.s = d; hcur.H = 2 * a.H; hcur.W = 2 * a.W;
      }
    }
    op_sn(hcur, "decoder.norm_out", K22_ACT_SILU, 1, s_P);
    op_conv3(s_P, hcur.H, hcur.W, hcur.C, cfg.out_ch, "decoder.conv_out", nullptr, s_out, IG_OUT_NCHW_F32);
    return finish_plan();
  }

  // Encoder.forward + quant_conv.  H, W: image size (multiples of 2^(levels-1); (H/8)*(W/8) a multiple of 64 for the
  // attention GEMMs).
  int plan_enc(int nB, int H, int W) {
    const int nres = cfg.n_levels;
    if (nB < 1 || H < 1 || W < 1 || H % (1 << (nres - 1)) || W % (1 << (nres - 1))) return k22_set_error(K22_EINVAL, "movq encoder: H, W must be positive multiples of 2^(levels-1)");
    if (int rc = check_fused((int64_t)(H >> (nres - 1)) * (W >> (nres - 1)))) return rc;
    begin_plan();
    B = nB; enc = true; encH = H; encW = W;
    ops.clear(); hrot = 0;
    h0 = H >> (nres - 1); w0 = W >> (nres - 1);
    s_img = new_slot((size_t)B * 3 * H * W * 4);
    s_xin = new_slot((size_t)B * (H + 2) * (W + 2) * 64 * esz);
    s_part = new_slot(); s_coeff = new_slot(); s_P = new_slot(); s_U = new_slot(); s_S = new_slot(); s_N = new_slot();
    s_Q = new_slot(); s_K = new_slot(); s_VT = new_slot(); s_SC = new_slot(); s_O = new_slot(); s_splitk = new_slot(256);
    for (int i = 0; i < 3; ++i) s_h[i] = new_slot();
    s_out = new_slot((size_t)B * cfg.z_channels * h0 * w0 * 4);
    s_lat = new_slot((size_t)B * 4 * h0 * w0 * 4);
    s_z = s_zq = nullptr;
    const int Bn = B, dt = dtype;
    ops.push_back([=](hipStream_t st) { return launch_movq_enc_prepare(ptr<float>(s_img), ptr(s_xin), Bn, H, W, 64, dt, st); });
    MAct hcur;
    {
      Slot* d = next_h();
      op_conv3(s_xin, H, W, 64, cfg.ch, "encoder.conv_in", nullptr, d, IG_OUT_ROWMAJOR);
      hcur.s = d; hcur.C = cfg.ch; hcur.H = H; hcur.W = W;
    }
    for (int lvl = 0; lvl < nres; ++lvl) {
      const int block_out = cfg.ch * cfg.ch_mult[lvl];
      const bool attn = (cfg.attn_levels >> lvl) & 1;
      const std::string pfx = "encoder.down." + std::to_string(lvl);
      for (int i = 0; i < cfg.num_res_blocks; ++i) {
        hcur = resblock(pfx + ".block." + std::to_string(i), hcur, block_out);
        if (attn) hcur = attnblock(pfx + ".attn." + std::to_string(i), hcur);
      }
      if (lvl != nres - 1) {
        // Downsample: F.pad (0,1,0,1) + conv3x3 stride 2 = the stride-1 "same" conv taken at the odd positions
        const MAct a = hcur;
        const int C = hcur.C;
        need(s_P, (size_t)B * (a.H + 2) * (a.W + 2) * C * esz);
        ops.push_back([=](hipStream_t st) { return launch_pad_copy(ptr(a.s), ptr(s_P), Bn, a.H, a.W, C, dt, st); });
        op_conv3(s_P, a.H, a.W, C, C, pfx + ".downsample.conv", nullptr, s_U, IG_OUT_ROWMAJOR);
        Slot* d = next_h();
        if (d == a.s) d = next_h();
        need(d, (size_t)B * (a.H / 2) * (a.W / 2) * C * esz);
        ops.push_back([=](hipStream_t st) { return launch_subsample_odd(ptr(s_U), ptr(d), Bn, a.H, a.W, C, dt, st); });
        hcur.s = d; hcur.H = a.H / 2; hcur.W = a.W / 2;
      }
    }
    hcur = resblock("encoder.mid.block_1", hcur, hcur.C);
    hcur = attnblock("encoder.mid.attn_1", hcur);
    hcur = resblock("encoder.mid.block_2", hcur, hcur.C);
    op_gn(hcur, "encoder.norm_out", K22_ACT_SILU, 1, s_P);
    op_conv3(s_P, hcur.H, hcur.W, hcur.C, cfg.z_channels, "encoder.conv_out", nullptr, s_out, IG_OUT_NCHW_F32);
    {
      const float* wq = Wf("quant_conv.weight"); const float* bq = Wf("quant_conv.bias");
      const int hw = h0 * w0;
      ops.push_back([=](hipStream_t st) { return launch_movq_quant_conv(ptr<float>(s_out), wq, bq, ptr<float>(s_lat), Bn, hw, st); });
    }
    return finish_plan();
  }
};

extern "C" {

int k22_movq_create(const K22MoVQConfig* cfg, const K22Weight* weights, int n_weights, K22MoVQ** out) {
  if (!cfg || !out) return k22_set_error(K22_EINVAL, "movq_create: null argument");
  if (!k22_dtype_ok(cfg->dtype)) return k22_set_error(K22_EINVAL, "movq_create: dtype");
  if (cfg->n_levels < 1 || cfg->n_levels > 8 || cfg->z_channels != 4 || cfg->ch % 128) return k22_set_error(K22_EINVAL, "movq_create: unsupported configuration (z_channels == 4, ch % 128 == 0)");
  K22MoVQ* m = new K22MoVQ();
  m->cfg = *cfg; m->set_dtype(cfg->dtype);
  m->set_weights(weights, n_weights);
  *out = m;
  return K22_OK;
}
void k22_movq_destroy(K22MoVQ* m) { delete m; }

int k22_movq_plan(K22MoVQ* m, int B, int h, int w, size_t* workspace_bytes) {
  if (!m || !workspace_bytes) return k22_set_error(K22_EINVAL, "movq_plan: null argument");
  int rc = m->plan(B, h, w);
  if (rc) return rc;
  *workspace_bytes = m->ws_bytes;
  return K22_OK;
}
int k22_movq_bind(K22MoVQ* m, void* workspace, size_t workspace_bytes) {
  if (!m) return k22_set_error(K22_EINVAL, "movq_bind: null argument");
  return m->bind(workspace, workspace_bytes, "movq_bind");
}
int k22_movq_decode(K22MoVQ* m, const float* z, float* out, unsigned char* out_u8, void* stream) {
  if (!m || !m->ws || m->enc) return k22_set_error(K22_EINVAL, "movq_decode: plan the decoder and bind a workspace first");
  if (!z || (!out && !out_u8)) return k22_set_error(K22_EINVAL, "movq_decode: null argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = copy_d2d(m->ptr(m->s_z), z, (size_t)m->B * 4 * m->h0 * m->w0 * 4, st)) return rc;
  if (int rc = run_list(m->ops, st)) return rc;
  const int H8 = m->h0 << (m->cfg.n_levels - 1), W8 = m->w0 << (m->cfg.n_levels - 1);
  if (out) { if (int rc = copy_d2d(out, m->ptr(m->s_out), (size_t)m->B * m->cfg.out_ch * H8 * W8 * 4, st)) return rc; }
  if (out_u8) return launch_to_uint8_nhwc(m->ptr<float>(m->s_out), out_u8, m->B, m->cfg.out_ch, H8, W8, st);
  return K22_OK;
}
int k22_movq_plan_encoder(K22MoVQ* m, int B, int H, int W, size_t* workspace_bytes) {
  if (!m || !workspace_bytes) return k22_set_error(K22_EINVAL, "movq_plan_encoder: null argument");
  int rc = m->plan_enc(B, H, W);
  if (rc) return rc;
  *workspace_bytes = m->ws_bytes;
  return K22_OK;
}
int k22_movq_encode(K22MoVQ* m, const float* image, float* latent, void* stream) {
  if (!m || !m->ws || !m->enc) return k22_set_error(K22_EINVAL, "movq_encode: plan the encoder and bind a workspace first");
  if (!image || !latent) return k22_set_error(K22_EINVAL, "movq_encode: null argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = copy_d2d(m->ptr(m->s_img), image, (size_t)m->B * 3 * m->encH * m->encW * 4, st)) return rc;
  if (int rc = run_list(m->ops, st)) return rc;
  return copy_d2d(latent, m->ptr(m->s_lat), (size_t)m->B * 4 * m->h0 * m->w0 * 4, st);
}
int k22_movq_num_ops(const K22MoVQ* m) { return m && m->planned ? (int)m->ops.size() : 0; }
int k22_movq_set_attention(K22MoVQ* m, int mode) {
  if (!m) return k22_set_error(K22_EINVAL, "movq_set_attention: null argument");
  if (mode != K22_MOVQ_ATTN_AUTO && mode != K22_MOVQ_ATTN_SCORES && mode != K22_MOVQ_ATTN_FUSED)
    return k22_set_error(K22_EINVAL, "movq_set_attention: mode must be 0 (auto), 1 (scores) or 2 (fused)");
  m->attn_mode = mode;
  return K22_OK;
}

}  // extern "C"
