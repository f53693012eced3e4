// k22 — UNet engine: builds the launch list of one Text2ImUNet forward from the reference's
// hyper-parameters and replays it (eagerly or as a captured hipGraph) on a caller-owned workspace.
//
// Structure mirrors UNetModel.__init__/forward (kandinsky2/model/unet.py:371-611) and
// Text2ImUNet.forward/get_text_emb (kandinsky2/model/text2im_model2_1.py:57-103):
//   emb = time_embed(timestep_embedding(t)) + xf_proj ; 16 input blocks ; middle ; 16 output blocks
//   (skip concat) ; out = GN+SiLU+conv3x3.
// MI355X mapping: activations live as NHWC in the workspace; every 3x3 conv input is written by the
// GroupNorm-apply kernel with a zero border; skip concats are never materialised (GroupNorm and the
// 1x1 skip GEMM take two base pointers); all 36 emb_layers run as ONE skinny GEMV per step;
// encoder_kv is hoisted into set_condition (its input, the cached xf_out, is step-invariant).
#include "kernels.h"
#include "elementwise.h"
#include "../../include/k22.h"
#include "tuning.h"
#include "plan.h"

#include <atomic>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int launch_step_advance(int* step, int delta, hipStream_t s);

// k22_debug_counter("loop_captures" / "loop_launches"): whole-loop graphs captured, and whole-loop replays or eager loop runs, by any loop
// entry of this process (host counters: a test reads from them that the one-graph path ran and that a second generation replayed)
static std::atomic<long> g_loop_captures{0}, g_loop_launches{0};
long loop_capture_count() { return g_loop_captures.load(); }
long loop_launch_count() { return g_loop_launches.load(); }
void loop_count_capture() { g_loop_captures.fetch_add(1); }
void loop_count_launch() { g_loop_launches.fetch_add(1); }
// first word of a captured loop's key: which entry's nodes the graph holds
enum : unsigned long long { K22_LOOP_KIND_P = 0, K22_LOOP_KIND_DDIM = 1, K22_LOOP_KIND_PLMS = 2, K22_LOOP_KIND_P_KEEP = 3, K22_LOOP_KIND_DPMPP = 4,
                            K22_LOOP_KIND_DPMPP_CLIP = 5, K22_LOOP_KIND_DPMPP_KEEP = 6 };

namespace {

enum OpKind { OP_CONV3 = 0, OP_GEMM = 1, OP_GN = 2, OP_ATTN = 3, OP_MISC = 4, OP_NKINDS = 5 };

struct Op {
  std::function<int(hipStream_t)> fn;
  int kind = OP_MISC;
  double flops = 0.0;   // algorithmic FLOPs (2*M*N*K) for MFMA ops
  double flops2 = 0.0;  // FLOPs of a fused 1x1 skip connection riding on a conv op
  double bytes = 0.0;   // algorithmic HBM bytes (read + write) for HBM-bound ops
  int kernels = 1;      // kernel launches issued by fn
  Op() {}
  template <typename F> Op(F f, int k = OP_MISC, double fl = 0.0, double by = 0.0, int nk = 1) : fn(f), kind(k), flops(fl), bytes(by), kernels(nk) {}
  int operator()(hipStream_t st) const { return fn(st); }
};
typedef std::vector<Op> OpList;

struct Act {  // unpadded NHWC activation, optionally a virtual channel concat of two tensors
  Slot* s0 = nullptr; int C0 = 0;
  Slot* s1 = nullptr; int C1 = 0;
  int H = 0, W = 0;
  // GroupNorm partial sums delivered by the producing convolution (null = none: run gn_stats_kernel)
  const Tuned* p0 = nullptr; Slot* st0 = nullptr;
  const Tuned* p1 = nullptr; Slot* st1 = nullptr;
  int C() const { return C0 + C1; }
};

}  // namespace

struct K22UNet : GraphPlan {   // dtype: arithmetic type of the MFMA kernels (K22DType; K22_F16X3 = split precision)
  K22UNetConfig cfg;
  int sdt;     // type of everything the data-movement kernels touch: dtype, except fp32 for the split-precision arithmetic

  // ---- plan state ----
  int B = 0, H = 0, W = 0;
  OpList ops;       // one UNet forward
  OpList cond_ops;  // conditioning head
  OpList hint_ops;  // 2.2 ControlNet-depth: input_hint_block over the hint image (once per generation)
  bool hint_set = false;
  int fuse_skip = 1;
  // (GroupNorm-apply fused into the consuming 3x3 convolution's halo fill - conv3_halo_spec_kernel's producers rewriting the raw tensor in
  // the LDS - was built, bit-identical to the two-kernel path, and measured SLOWER on MI355X: bf16 C2 step 143.5 -> 112.9 steps/s, f16x3
  // 66.5 -> 59.4 (profiles/r04_gn_fused_negative.txt).  Removed; the code is in the parent of the commit that removed it.  Every GroupNorm
  // runs the stand-alone gn_apply.)
  // weight-streaming kernel (stream_gemm.hip) for the small-M 3x3 convolutions: fragment-major copies of their weights live in the
  // workspace (one more copy of those weights: ~1.2 GB of the 2.1 UNet in bf16), written once per bind before the first forward
  int stream_frag = 1;
  struct FragJob { const void* W; Slot* slot; int Npad, taps, Kc; };
  std::vector<FragJob> frag_jobs;
  bool frag_done = false;
  int repack_frags(hipStream_t st) {
    for (auto& j : frag_jobs) {
      int rc = launch_stream_repack(j.W, ptr(j.slot), j.Npad, j.taps, j.Kc, dtype, st);
      if (rc) return rc;
    }
    frag_done = true;
    return K22_OK;
  }
  // in_layers of the up-sampling ResBlocks as four 2x2 convolutions of the low-resolution tensor (conv3_up2.hip) instead of GroupNorm-apply
  // into the 4x larger padded tensor + a 9-tap convolution at the high resolution.  K22_UP_PHASE=0: the 9-tap route everywhere (A/B in one build).
  int up_phase = env_flag("K22_UP_PHASE", 1);
  bool cond_set = false;
  // the whole denoising loop as ONE graph (any of the k22_unet_*_loop entries, unet_loop below): valid for exactly the buffers / scalars
  // it was captured with
  LoopCache loop;
  // k22_unet_set_threshold_group: rows of the cond half per threshold group of the p_sampler loops (SamplerParams::pct_group); 0 = the whole
  // batch from element 0.  A word of the captured loop's key.
  int threshold_group = 0;

  // persistent slots
  Slot *s_xin, *s_img, *s_mask, *s_t, *s_out;
  Slot *s_temb, *s_e1, *s_emb, *s_film, *s_xfproj, *s_ctx;
  Slot *s_full, *s_pool, *s_imgemb, *s_tmpf, *s_tmpf2, *s_fullT;
  Slot *s_part, *s_coeff, *s_P1, *s_U1, *s_P2, *s_S, *s_N, *s_QKV, *s_KALL, *s_VT, *s_ATT, *s_splitk, *s_flush;
  Slot *s_U1st;
  Slot *s_ctxf = nullptr, *s_hint = nullptr, *s_hintin = nullptr, *s_hbuf[2] = {nullptr, nullptr};
  Slot* s_h[3];
  Slot* s_hst[3];
  std::vector<Slot*> s_ctxkv;  // one per attention block
  int n_attn = 0;
  int64_t film_total = 0;
  // k22_unet_sample_loop: the time embedding and ALL FiLM vectors of every step of the loop are computed by batched launches before the first
  // step (the timesteps of a loop are known up front and nothing else feeds them): rows = steps x B, up to 8 rows per launch, so the 231 MB
  // emb_layers weight stream is read once per 8 / B steps instead of once per step.  Every output row is the same arithmetic as in the per-step
  // launch (one accumulator per row, same order): the loop stays bit-identical to the stepwise calls (asserted by the GPU tests).
  float* film_all = nullptr;        // [rows][film_total] | temb [rows][mc] | e1 [rows][ted] | emb [rows][ted]
  size_t film_all_bytes = 0;
  int hoist_time = 1;               // K22_HOIST_TIME=0 (measurement only): the loop keeps the per-step time / FiLM launches
  const float* film_cur = nullptr;  // != null while a hoisted loop runs: this step's [B][film_total]
  const float* film_base() const { return film_cur ? film_cur : ptr<float>(s_film); }
  struct TimeW { const float* freqs; const float* w0; const float* b0; const float* w2; const float* b2; const void* we; const float* be; int mc, ted, dt; } tw = {};
  // rows of (timestep -> sinusoid -> time_embed MLP + conditioning row (m % B) -> SiLU -> emb_layers of every ResBlock): nn.py:101-121, unet.py:159-170
  int time_rows(const float* t, float* temb, float* e1, float* emb, float* film, int rows, hipStream_t st) {
    int rc = launch_timestep_embedding(t, tw.freqs, temb, rows, tw.mc / 2, st);
    if (rc) return rc;
    LinearSmallParams lp = {};
    lp.x = temb; lp.ldx = tw.mc; lp.W = tw.w0; lp.bias = tw.b0; lp.out = e1; lp.ldo = tw.ted;
    lp.M = rows; lp.N = tw.ted; lp.K = tw.mc; lp.act_in = K22_ACT_NONE; lp.act_out = K22_ACT_SILU;
    rc = launch_linear_smallm(lp, K22_F32, st);
    if (rc) return rc;
    lp.x = e1; lp.ldx = tw.ted; lp.W = tw.w2; lp.bias = tw.b2; lp.add = ptr<float>(s_xfproj); lp.ld_add = tw.ted; lp.add_mod = B;
    lp.out = emb; lp.K = tw.ted; lp.act_out = K22_ACT_NONE;
    rc = launch_linear_smallm(lp, K22_F32, st);
    if (rc) return rc;
    LinearSmallParams le = {};
    le.x = emb; le.ldx = tw.ted; le.W = tw.we; le.bias = tw.be; le.out = film; le.ldo = film_total;
    le.M = rows; le.N = (int)film_total; le.K = tw.ted; le.act_in = K22_ACT_SILU; le.act_out = K22_ACT_NONE;
    return launch_linear_smallm(le, tw.dt, st);
  }

  // (The "two half-batch chains" mode - the CFG pair as two engines on two streams - lives above this file: Text2ImUNetHIP(chains=2) drives
  // two handles of this engine from the host (unet.py, K22_CHAINS in INTEGRATION.md, bench.py --chains) and needs a library built without
  // packed-fp32 instructions, the Makefile's default NOPK=1.  No whole-loop graph runs under it.)
  // the [B][out_channels][HW] model output
  float* model_out() { return ptr<float>(s_out); }
  int exec(hipStream_t st) { return run_ops(st); }
  int exec_eager(hipStream_t st) { return run_eager(st, [this](hipStream_t s) { return exec(s); }); }
  // first forward of a plan / binding: fragment-major weight copies, tile configurations the table does not know
  int prepare_run(hipStream_t st) {
    if (!frag_done) { int rc = repack_frags(st); if (rc) return rc; }
    return tune_once(s_flush, st);
  }

  ~K22UNet() {
    if (film_all) (void)hipFree(film_all);
  }

  // ---- what k22_unet_forward and the whole-loop entries share ----------------------------------------------------------------------
  // the 9-channel UNet's constant inputs into their slots
  int stage_inpaint(const float* inpaint_image, const float* inpaint_mask, hipStream_t s) {
    if (cfg.in_channels != 9) return K22_OK;
    const size_t pb = (size_t)B, hw = (size_t)H * W;
    if (int rc = copy_d2d(ptr(s_img), inpaint_image, pb * 4 * hw * 4, s)) return rc;
    return copy_d2d(ptr(s_mask), inpaint_mask, pb * hw * 4, s);
  }

  // ---- the whole-loop entries (k22_unet_sample_loop[_keep], k22_unet_ddim_loop, k22_unet_dpmpp_loop[_keep]): pieces of unet_loop below -------
  // A loop is n_calls model calls, each  UNet([x_half | x_half], timesteps[call])  followed by the entry's own sampler kernels.
  struct LoopRows {   // hoisted time / FiLM rows of all model calls (null members: per-call launches)
    bool hoist = false;
    float *film = nullptr, *temb = nullptr, *e1 = nullptr, *emb = nullptr;
  };
  // first-run preparation + the [n_calls * B] row buffer; called after validation (it may drop the captured loop)
  int loop_begin(int n_calls, hipStream_t st, LoopRows* lr) {
    if (int rc = prepare_run(st)) return rc;
    // the time / FiLM rows of all calls up front (film_all): 8 / B calls per batched launch; B > 8 keeps the per-call launches
    lr->hoist = B <= 8 && hoist_time;
    if (!lr->hoist) return K22_OK;
    const int64_t rows_all = (int64_t)n_calls * B;
    const size_t need = (size_t)rows_all * (size_t)(film_total + tw.mc + 2 * tw.ted) * sizeof(float);
    if (need > film_all_bytes) {
      loop.drop();   // captured loops hold the old buffer's addresses (a captured forward does not: it reads s_film)
      if (film_all) { (void)hipStreamSynchronize(st); (void)hipFree(film_all); film_all = nullptr; film_all_bytes = 0; }
      const hipError_t e = hipMalloc(reinterpret_cast<void**>(&film_all), need);
      if (e != hipSuccess) { film_all = nullptr; return k22_set_error_hip(e, __FILE__, __LINE__); }
      film_all_bytes = need;
    }
    lr->film = film_all;
    lr->temb = lr->film + rows_all * film_total;
    lr->e1 = lr->temb + rows_all * tw.mc;
    lr->emb = lr->e1 + rows_all * tw.ted;
    return K22_OK;
  }
  // what a loop runs before its first step: the batched time rows, the 9-channel UNet's constant inputs
  int loop_prologue(const LoopRows& lr, const float* timesteps, int n_calls, const float* inpaint_image, const float* inpaint_mask, hipStream_t s) {
    if (lr.hoist) {
      const int spl = 8 / B;   // calls per batched launch
      for (int k0 = 0; k0 < n_calls; k0 += spl) {
        const int rows = (n_calls - k0 < spl ? n_calls - k0 : spl) * B;
        const int64_t r0 = (int64_t)k0 * B;
        const int rc = time_rows(timesteps + r0, lr.temb + r0 * tw.mc, lr.e1 + r0 * tw.ted, lr.emb + r0 * tw.ted, lr.film + r0 * film_total, rows, s);
        if (rc) return rc;
      }
    }
    return stage_inpaint(inpaint_image, inpaint_mask, s);
  }
  // model call number `call` of the loop on the latent `cur` [B][4][HW]; the output is model_out()
  int loop_model(const LoopRows& lr, const float* cur, const float* timesteps, int call, hipStream_t s) {
    // model_fn: the UNet sees the first half twice (kandinsky2_1_model.py:223-225)
    const size_t half = (size_t)(B / 2) * 4 * H * W * sizeof(float);
    if (int rc = copy_d2d(ptr(s_xin), cur, half, s)) return rc;
    if (int rc = copy_d2d(ptr(s_xin) + half, cur, half, s)) return rc;
    if (lr.hoist) {
      film_cur = lr.film + (int64_t)call * B * film_total;
    } else {
      if (int rc = copy_d2d(ptr(s_t), timesteps + (size_t)call * B, (size_t)B * 4, s)) return rc;
    }
    return exec(s);
  }
  // before the first capture of a plan: one step's ops eagerly (function attributes, code load) on a scratch input.  A re-capture for other
  // scalars / buffers (guidance, step count: they are baked into the graph's nodes) does not repeat it.
  int loop_warm(const float* timesteps, const float* inpaint_image, const float* inpaint_mask, hipStream_t st) {
    hipError_t e = hipMemsetAsync(ptr(s_xin), 0, (size_t)B * 4 * H * W * 4, st);
    if (e != hipSuccess) return k22_set_error_hip(e, __FILE__, __LINE__);
    if (int rc = copy_d2d(ptr(s_t), timesteps, (size_t)B * 4, st)) return rc;
    if (int rc = stage_inpaint(inpaint_image, inpaint_mask, st)) return rc;
    if (int rc = exec_eager(st)) return rc;
    e = hipStreamSynchronize(st);
    return e == hipSuccess ? (int)K22_OK : k22_set_error_hip(e, __FILE__, __LINE__);
  }

  // One forward on `st`: the op list in order.  (A variant that forked the time-embedding / FiLM GEMV onto a second stream,
  // i.e. a parallel branch of the captured graph joined by the first FiLM consumer, was measured on one box, alternating
  // runs: 116.9 / 117.2 steps/s with the branch against 119.4 / 119.1 without - the 231 MB weight stream slows the
  // convolutions it runs beside by more than the 80 us it hides.  Removed.)
  int run_ops_range(hipStream_t st, size_t lo, size_t hi) { return run_list(ops, st, lo, hi); }
  int run_ops(hipStream_t st) { return run_list(ops, st); }

  // ------------------------------------------------------------------------------------------
  void op_gn(OpList& L, const Act& in, const std::string& pfx, int64_t film_off,
             int act, int mode, int pad, Slot* dst) {
    const int Bn = B, C = in.C(), HW = in.H * in.W;
    const int nsplit = gn_nsplit(Bn, HW);
    // producer-side partial sums for every part of the input?  Otherwise the stand-alone stats pass.
    const bool fused = in.st0 != nullptr && (in.s1 == nullptr || in.st1 != nullptr);
    if (!fused) need(s_part, (size_t)Bn * nsplit * C * 2 * sizeof(float));
    need(s_coeff, (size_t)Bn * C * 2 * sizeof(float));
    const int Ho = mode == 1 ? in.H / 2 : (mode == 2 ? in.H * 2 : in.H);
    const int Wo = mode == 1 ? in.W / 2 : (mode == 2 ? in.W * 2 : in.W);
    need(dst, (size_t)Bn * (Ho + 2 * pad) * (Wo + 2 * pad) * C * esz);
    const float* gamma = Wf(pfx + ".weight");
    const float* beta = Wf(pfx + ".bias");
    const Act a = in;
    const int dt = sdt;
    const int x3 = k22_is_split(dtype) ? 1 : 0;   // every GroupNorm output feeds a convolution or the qkv GEMM: written in x3 chunks
    const double gn_bytes = (double)Bn * HW * C * esz * (fused ? 1.0 : 2.0) + (double)Bn * (Ho + 2 * pad) * (Wo + 2 * pad) * C * esz;
    L.push_back(Op([=](hipStream_t st) {
      const void* x0 = ptr(a.s0);
      const void* x1 = a.s1 ? ptr(a.s1) : nullptr;
      GnCoeffParams cp = {};
      if (fused) {
        cp.src[0].st = ptr<float>(a.st0); cp.src[0].rpi = a.p0->rpi; cp.src[0].C = a.C0;
        if (a.s1) { cp.src[1].st = ptr<float>(a.st1); cp.src[1].rpi = a.p1->rpi; cp.src[1].C = a.C1; }
        if (cp.src[0].rpi <= 0 || (a.s1 && cp.src[1].rpi <= 0)) return k22_set_error(K22_EINVAL, "unet: producer delivered no GroupNorm partial sums");
      } else {
        GnStatsParams sp;
        sp.x0 = x0; sp.x1 = x1; sp.C0 = a.C0; sp.C1 = a.C1;
        sp.HW = HW; sp.B = Bn; sp.groups = 32; sp.nsplit = nsplit; sp.partial = ptr<float>(s_part);
        int rc = launch_gn_stats(sp, dt, st);
        if (rc) return rc;
        cp.src[0].st = ptr<float>(s_part); cp.src[0].rpi = nsplit; cp.src[0].C = C;
      }
      cp.HW = HW; cp.C = C; cp.groups = 32; cp.eps = 1e-5f;
      cp.gamma = gamma; cp.beta = beta;
      cp.film = film_off >= 0 ? film_base() + film_off : nullptr; cp.film_ld = film_total;
      cp.coeff = ptr<float>(s_coeff);
      GnApplyParams ap = {};
      ap.x0 = x0; ap.x1 = x1; ap.C0 = a.C0; ap.C1 = a.C1; ap.B = Bn; ap.H = a.H; ap.W = a.W;
      ap.mode = mode; ap.pad = pad; ap.act = act; ap.coeff = ptr<float>(s_coeff); ap.out = ptr(dst); ap.out_x3 = x3;
      int rc = launch_gn_coeff(cp, Bn, st);
      if (rc) return rc;
      return launch_gn_apply(ap, dt, st);
    }, OP_GN, 0.0, gn_bytes, fused ? 2 : 3));
  }

  static void apply_cfg(IgemmParams& q, const Cfg& c) { tuned_apply_cfg(q, c); }
  int op_dt(const Tuned& t) const { return t.dt >= 0 ? t.dt : dtype; }
  void make_candidates(Tuned& t) { tuned_make_candidates(t, op_dt(t)); }
  void default_cfg(Tuned& t) { tuned_default_cfg(t, op_dt(t)); }
  void finish_cfg(Tuned& t) { tuned_finish_cfg(t, op_dt(t)); }
  size_t max_splitk_bytes(const Tuned& t) const { return tuned_max_splitk_bytes(t, op_dt(t), autotune != 0); }
  int max_rpi(const Tuned& t) const { return tuned_max_rpi(t, op_dt(t), autotune != 0); }

  // ---- precision plan of the asymmetric split engine (K22_F16X2; round 5) -----------------------------------------------------------
  // Which MFMA ops take the activation operand at fp16 precision (two MFMAs per product) and which keep the full split (three) is a
  // property of the PLAN, read off the operand-rounding ablation of the oracle (oracle/drift_ablation.py -> tests/golden/
  // drift_ablation_x2.json; share of the first-forward error variance of "every activation operand at fp16"):
  //   1x1 skip_connection inputs (the un-normalised residual stream)           51 %   -> always three MFMAs (3 % of the FLOPs)
  //   the out head's 3x3 convolution (384 -> 8 channels)                       14 %   -> always three MFMAs (0.03 % of the FLOPs)
  //   3x3 convolutions of the top level: in_layers 12 %, out_layers 14 %              -> x2_plan bits 0 / 1 (40 % of the FLOPs)
  //   3x3 convolutions one level down 6 %, two 0.7 %, three 0.08 %; qkv 0.02 %        -> two MFMAs
  //   attention operands (q, k, v, P)                                          1.5 %  -> ONE MFMA (fp16 tiles, attention_kernel<xh_t>)
  //   proj_out, encoder_kv, to_model_dim_n (small; inputs not normalised)             -> three MFMAs
  // x2_plan: bit 0 = the top level's in_layers convolutions run x2, bit 1 = its out_layers convolutions run x2 (K22_X2_PLAN).  Default 0:
  // measured at C2 on MI355X (profiles/r05_x2_plans.txt; same box, x3 = 59.5 steps/s at 3.6e-6): plan 0 69.4 steps/s at 2.7e-4 max-abs /
  // 5.4e-5 rms, plan 1 71.9 at 5.3e-4 / 8.5e-5, plan 2 71.3 at 4.6e-4 / 9.3e-5, plan 3 73.9 at 5.8e-4 / 1.14e-4 - the rms values are the
  // ablation's predictions to 4 %; the last 6 % of speed cost the margin to the 5e-4 bar.
  int x2_plan = 0;
  enum ConvRole { CONV_IN = 0, CONV_OUT = 1, CONV_HEAD = 2 };
  int conv_dt(int role, int Hc) const {
    if (dtype != K22_F16X2) return dtype;
    if (role == CONV_HEAD) return K22_F16X3;
    if (Hc >= H) return (x2_plan >> role) & 1 ? K22_F16X2 : K22_F16X3;   // top level (the latent's own resolution)
    return K22_F16X2;
  }
  // GEMMs: only the qkv projection (its input is a GroupNorm output) runs x2
  int gemm_dt(bool qkv) const { return dtype == K22_F16X2 ? (qkv ? K22_F16X2 : K22_F16X3) : dtype; }

  // conv3x3 over a zero-bordered slot `src` [B][Hc+2][Wc+2][Cin].  `stats` (optional) receives the GroupNorm
  // partial sums of the output; returns the launch descriptor (null when the output is not a tunable T tensor).
  Tuned* op_conv(OpList& L, int role, Slot* src, int Hc, int Wc, int Cin, int Cout,
                 const std::string& pfx, const Act* residual, Slot* dst, int out_mode, Slot* stats = nullptr,
                 const Act* skip_in = nullptr, const std::string& skip_pfx = std::string()) {
    tuned.emplace_back();
    Tuned* t = &tuned.back();
    t->dt = conv_dt(role, Hc);
    IgemmParams& p = t->p;
    p = igemm_conv3_problem(B, Hc, Wc, Cin, Cout, out_mode);
    p.Wp = W_(pfx + ".weight"); p.bias = Wf(pfx + ".bias");
    Act sk;
    if (skip_in) {
      // fused 1x1 skip_connection: S0 is only a non-null marker here, the device pointers are set at launch
      sk = *skip_in;
      p.S0 = reinterpret_cast<const void*>(1); p.S1 = sk.s1 ? reinterpret_cast<const void*>(1) : nullptr;
      p.SK0 = sk.C0; p.SK1 = sk.C1;
      p.Ws = W_(skip_pfx + ".weight"); p.bias2 = Wf(skip_pfx + ".bias");
    }
    t->want_stats = stats != nullptr;
    // small M (the 24x24 / 12x12 levels): the weight-streaming kernel becomes a candidate, fed from a fragment-major copy of the weights
    Slot *wf = nullptr, *wsf = nullptr;
    if (stream_frag && k22_esz(dtype) == 2 && p.M <= 1152 && (stream_supported(p, dtype, 5) || stream_supported(p, dtype, 9))) {
      wf = new_slot();
      need(wf, stream_frag_bytes(p.Npad, 9, Cin, dtype));
      frag_jobs.push_back({p.Wp, wf, p.Npad, 9, Cin});
      p.Wfrag = reinterpret_cast<const void*>(1);          // marker for the candidate list; the device pointer is set at launch
      if (skip_in) {
        wsf = new_slot();
        need(wsf, stream_frag_bytes(p.Npad, 1, p.SK0 + p.SK1, dtype));
        frag_jobs.push_back({p.Ws, wsf, p.Npad, 1, p.SK0 + p.SK1});
        p.Wsfrag = reinterpret_cast<const void*>(1);
      }
    }
    make_candidates(*t);
    default_cfg(*t);
    // The fragment-major copy costs one more copy of this layer's weights in every plan's workspace and a repack per bind:
    // keep it only where the weight-streaming kernel can actually run - the tile table (or the fixed heuristic, autotune off) names it
    // for this problem, or the problem is unknown and will be measured with it as a candidate.
    if (wf && t->cfg.algo != IG_ALGO_STREAM && (t->from_table || !autotune)) {
      wf->bytes = 0; wf = nullptr;
      if (wsf) { wsf->bytes = 0; wsf = nullptr; frag_jobs.pop_back(); }
      frag_jobs.pop_back();
      p.Wfrag = nullptr; p.Wsfrag = nullptr;
      make_candidates(*t);
      default_cfg(*t);
    }
    need(s_splitk, max_splitk_bytes(*t));
    if (t->want_stats) need(stats, (size_t)B * max_rpi(*t) * Cout * 2 * sizeof(float));
    need(dst, out_mode == IG_OUT_ROWMAJOR ? (size_t)p.M * Cout * esz : (size_t)p.M * Cout * sizeof(float));
    Slot* rs = residual ? residual->s0 : nullptr;
    const int dt = t->dt;
    t->run = [=](hipStream_t st) {
      IgemmParams q = t->p;
      apply_cfg(q, t->cfg);
      q.A0 = ptr(src); q.residual = rs ? ptr(rs) : nullptr; q.out = ptr(dst); q.partial = ptr<float>(s_splitk);
      q.stats = t->want_stats ? ptr<float>(stats) : nullptr;
      if (q.S0) { q.S0 = ptr(sk.s0); q.S1 = sk.s1 ? ptr(sk.s1) : nullptr; }
      q.Wfrag = wf ? ptr(wf) : nullptr; q.Wsfrag = wsf ? ptr(wsf) : nullptr;
      return launch_igemm(q, dt, st);
    };
    const double fl = 2.0 * p.M * (double)p.N * 9.0 * p.Kc;
    L.push_back(Op([=](hipStream_t st) { return t->run(st); }, OP_CONV3, fl, 0.0, 1));
    if (skip_in) L.back().flops2 = 2.0 * p.M * (double)p.N * (p.SK0 + p.SK1);  // counted in the GEMM class
    return t;
  }

  // Does the up-sampling ResBlock with a low-resolution Hl x Wl input take the four-phase route?  The folded weights must be in the arena
  // (pack.py writes them for every up-sampling block; an arena without them runs the 9-tap route) and the kernel must fit the problem.
  bool up2_route(const std::string& wname, int Hl, int Wl, int Cin, int Cout) const {
    if (!up_phase || w.find(wname) == w.end()) return false;
    const IgemmParams q = igemm_up2_problem(B, Hl, Wl, Cin, Cout);
    const int dt = conv_dt(CONV_IN, 2 * Hl);
    return conv3_up2_supported(q, dt, 256) || conv3_up2_supported(q, dt, 128);
  }
  // nearest 2x upsample + conv3x3 in the four-phase form: `src` = the zero-bordered LOW-resolution slot [B][Hl+2][Wl+2][Cin], `dst` = the
  // unpadded [B][2Hl][2Wl][Cout]; weights pfx.weight_up2 [4][roundup(Cout,64)][2x2][Cin].  Tile and split: igemm_resolve's fixed rule.
  Tuned* op_conv_up2(OpList& L, Slot* src, int Hl, int Wl, int Cin, int Cout, const std::string& pfx, Slot* dst, Slot* stats) {
    tuned.emplace_back();
    Tuned* t = &tuned.back();
    t->dt = conv_dt(CONV_IN, 2 * Hl);
    IgemmParams& p = t->p;
    p = igemm_up2_problem(B, Hl, Wl, Cin, Cout);
    p.Wp = W_(pfx + ".weight_up2"); p.bias = Wf(pfx + ".bias");
    t->want_stats = stats != nullptr;
    make_candidates(*t);
    default_cfg(*t);
    need(s_splitk, max_splitk_bytes(*t));
    if (t->want_stats) need(stats, (size_t)B * max_rpi(*t) * Cout * 2 * sizeof(float));
    need(dst, (size_t)p.M * Cout * esz);
    const int dt = t->dt;
    t->run = [=](hipStream_t st) {
      IgemmParams q = t->p;
      apply_cfg(q, t->cfg);
      q.A0 = ptr(src); q.out = ptr(dst); q.partial = ptr<float>(s_splitk);
      q.stats = t->want_stats ? ptr<float>(stats) : nullptr;
      return launch_igemm(q, dt, st);
    };
    L.push_back(Op([=](hipStream_t st) { return t->run(st); }, OP_CONV3, 2.0 * p.M * (double)p.N * 4.0 * p.Kc, 0.0, 1));
    return t;
  }

  // GEMM over unpadded rows (1x1 conv / linear); `in` may be a virtual concat.
  // `stats` (optional) receives the GroupNorm partial sums of the output (image-shaped inputs only: in.H * in.W rows
  // per image); whether a configuration that can deliver them exists is reported by the returned want_stats.
  // a_raw: `in` holds plain T rows that no producer of ours wrote in x3 chunks (split-precision arithmetic only; ignored otherwise)
  Tuned* op_gemm(OpList& L, const Act& in, int M, int N, const std::string& pfx,
                 const Act* residual, Slot* dst, int ldo = 0, int out_mode = IG_OUT_ROWMAJOR, Slot* stats = nullptr, bool a_raw = false) {
    tuned.emplace_back();
    Tuned* t = &tuned.back();
    t->dt = gemm_dt(out_mode == IG_OUT_QKV);
    IgemmParams& p = t->p;
    p = igemm_gemm_problem(M, N, in.C0, in.C1, out_mode);
    if (ldo) p.ldo = ldo;
    if (in.H > 0 && in.W > 0 && M % (in.H * in.W) == 0 && M / (in.H * in.W) == B) { p.H = in.H; p.W = in.W; }  // rows per image
    if (out_mode == IG_OUT_QKV) p.att_T = in.H * in.W;
    p.Wp = W_(pfx + ".weight"); p.bias = Wf(pfx + ".bias");
    p.a_raw = (a_raw && k22_is_split(dtype)) ? 1 : 0;
    t->want_stats = stats != nullptr && p.H > 0;
    make_candidates(*t);
    if (t->want_stats && t->cands.empty()) { t->want_stats = false; make_candidates(*t); }
    default_cfg(*t);
    need(s_splitk, max_splitk_bytes(*t));
    if (t->want_stats) need(stats, (size_t)B * max_rpi(*t) * N * 2 * sizeof(float));
    need(dst, (size_t)M * p.ldo * esz);
    const Act a = in;
    Slot* rs = residual ? residual->s0 : nullptr;
    const int dt = t->dt;
    t->run = [=](hipStream_t st) {
      IgemmParams q = t->p;
      apply_cfg(q, t->cfg);
      q.A0 = ptr(a.s0); q.A1 = a.s1 ? ptr(a.s1) : nullptr;
      q.residual = rs ? ptr(rs) : nullptr; q.out = ptr(dst); q.partial = ptr<float>(s_splitk);
      if (t->aux0) { q.kall = ptr(reinterpret_cast<Slot*>(t->aux0)); q.vtall = ptr(reinterpret_cast<Slot*>(t->aux1)); }
      q.stats = t->want_stats ? ptr<float>(stats) : nullptr;
      return launch_igemm(q, dt, st);
    };
    L.push_back(Op([=](hipStream_t st) { return t->run(st); }, OP_GEMM, 2.0 * p.M * (double)p.N * p.Kc, 0.0, 1));
    return t;
  }

  // The tensor `t` wrote: [B][Ho][Wo][C] in `s`, with its GroupNorm partial sums in `stats` where t delivers them
  static Act produced(Slot* s, int C, int Ho, int Wo, const Tuned* t, Slot* stats) {
    Act a; a.s0 = s; a.C0 = C; a.H = Ho; a.W = Wo;
    if (t->want_stats) { a.p0 = t; a.st0 = stats; }
    return a;
  }

  // ResBlock (unet.py:110-220) with use_scale_shift_norm=True; updown: 0 none, 1 down, 2 up.
  Act resblock(const std::string& pfx, const Act& in, int Cout, int updown, int64_t& film_cursor, Slot* dst, Slot* dst_stats) {
    const int Cin = in.C();
    const int Ho = updown == 1 ? in.H / 2 : (updown == 2 ? in.H * 2 : in.H);
    const int Wo = updown == 1 ? in.W / 2 : (updown == 2 ? in.W * 2 : in.W);
    // in_layers: GN + SiLU (+ resample) -> conv3x3
    const bool up2 = updown == 2 && !in.s1 && up2_route(pfx + ".in_layers.2.weight_up2", in.H, in.W, Cin, Cout);
    Tuned* t1;
    if (up2) {
      // GroupNorm + SiLU at the LOW resolution (zero border), then the four 2x2 phase convolutions write the high-resolution tensor
      op_gn(ops, in, pfx + ".in_layers.0", -1, K22_ACT_SILU, 0, 1, s_P1);
      t1 = op_conv_up2(ops, s_P1, in.H, in.W, Cin, Cout, pfx + ".in_layers.2", s_U1, s_U1st);
    } else {
      op_gn(ops, in, pfx + ".in_layers.0", -1, K22_ACT_SILU, updown, 1, s_P1);
      t1 = op_conv(ops, CONV_IN, s_P1, Ho, Wo, Cin, Cout, pfx + ".in_layers.2", nullptr, s_U1, IG_OUT_ROWMAJOR, s_U1st);
    }
    // out_layers: GN * (1+scale) + shift -> SiLU -> conv3x3 (+ skip)
    const Act u1 = produced(s_U1, Cout, Ho, Wo, t1, s_U1st);
    const int64_t film_off = film_cursor;
    film_cursor += 2 * Cout;
    op_gn(ops, u1, pfx + ".out_layers.0", film_off, K22_ACT_SILU, 0, 1, s_P2);
    Act skip;
    skip.H = Ho; skip.W = Wo; skip.C0 = Cout;
    if (updown) {
      if (Cin != Cout || in.s1) { if (err.empty()) err = "updown ResBlock with channel change is not supported"; }
      need(s_S, (size_t)B * Ho * Wo * Cin * esz);
      const Act a = in; const int Bn = B, dt = sdt;
      ops.push_back([=](hipStream_t st) { return launch_resample(ptr(a.s0), ptr(s_S), Bn, a.H, a.W, Cin, updown, dt, st); });
      skip.s0 = s_S;
    } else if (Cin != Cout) {
      // 1x1 skip_connection: fused into the second conv (halo kernel) when it applies, else its own GEMM
      IgemmParams probe = igemm_conv3_problem(B, Ho, Wo, Cout, Cout);
      probe.S0 = reinterpret_cast<const void*>(1); probe.S1 = in.s1 ? reinterpret_cast<const void*>(1) : nullptr;
      probe.SK0 = in.C0; probe.SK1 = in.C1; probe.Ws = reinterpret_cast<const void*>(1);
      if (fuse_skip && Cout >= 128 && (conv3_halo_supported(probe, dtype, 256) || conv3_halo_supported(probe, dtype, 128))) {
        Tuned* t2 = op_conv(ops, CONV_OUT, s_P2, Ho, Wo, Cout, Cout, pfx + ".out_layers.3", nullptr, dst, IG_OUT_ROWMAJOR, dst_stats,
                            &in, pfx + ".skip_connection");
        return produced(dst, Cout, Ho, Wo, t2, dst_stats);
      }
      op_gemm(ops, in, B * Ho * Wo, Cout, pfx + ".skip_connection", nullptr, s_S, 0, IG_OUT_ROWMAJOR, nullptr, /*a_raw=*/true);
      skip.s0 = s_S;
    } else {
      if (in.s1) { if (err.empty()) err = "identity skip over a concat input"; }
      skip.s0 = in.s0;
    }
    Tuned* t2 = op_conv(ops, CONV_OUT, s_P2, Ho, Wo, Cout, Cout, pfx + ".out_layers.3", &skip, dst, IG_OUT_ROWMAJOR, dst_stats);
    return produced(dst, Cout, Ho, Wo, t2, dst_stats);
  }

  // AttentionBlock (unet.py:223-269) + QKVAttention (:272-340).  The qkv projection writes q row-major and k / v
  // straight into this block's attention operands (K_all, V^T_all) behind the context keys, which were projected
  // (encoder_kv) and packed once per conditioning: no per-step packing kernel.
  Act attnblock(const std::string& pfx, const Act& in, Slot* dst, Slot* dst_stats = nullptr) {
    const int C = in.C0, T = in.H * in.W, Hh = C / 64, S = cfg.ctx_len;
    const int Tk = S + T, Tkp = (Tk + 63) / 64 * 64;
    n_attn++;
    op_gn(ops, in, pfx + ".norm", -1, K22_ACT_NONE, 0, 0, s_N);
    Act n; n.s0 = s_N; n.C0 = C; n.H = in.H; n.W = in.W;
    Slot* kall = new_slot((size_t)B * Hh * Tkp * 64 * esz);
    Slot* vtall = new_slot((size_t)B * Hh * Tkp * 64 * esz);
    // encoder_kv (step-invariant) + context part of K_all / V^T_all (and zero padding) -> cond_ops
    Slot* ckv = new_slot((size_t)B * S * 2 * C * esz);
    s_ctxkv.push_back(ckv);
    const int Bn = B, dt = dtype, sd = sdt;
    {
      Act c; c.s0 = s_ctx; c.C0 = cfg.ctx_dim; c.H = 1; c.W = S;
      op_gemm(cond_ops, c, B * S, 2 * C, pfx + ".encoder_kv", nullptr, ckv, 0, IG_OUT_ROWMAJOR, nullptr, /*a_raw=*/true);
      cond_ops.push_back(Op([=](hipStream_t st) {
        KvPackParams kp;
        kp.qkv = nullptr; kp.ctxkv = ptr(ckv); kp.kall = ptr(kall); kp.vtall = ptr(vtall);
        kp.B = Bn; kp.H = Hh; kp.T = 0; kp.S = S; kp.Tkp = Tkp;
        return launch_kv_pack(kp, sd, st);
      }));
    }
    // qkv projection in IG_OUT_QKV mode
    need(s_QKV, (size_t)B * T * C * esz);  // q only
    {
      Tuned* t = op_gemm(ops, n, B * T, 3 * C, pfx + ".qkv", nullptr, s_QKV, C, IG_OUT_QKV);
      t->p.att_T = T; t->p.att_S = S; t->p.att_Tkp = Tkp;
      t->aux0 = kall; t->aux1 = vtall;
    }
    need(s_ATT, (size_t)B * T * C * esz);
    ops.push_back(Op([=](hipStream_t st) {
      AttentionParams ap = {};
      ap.q = ptr(s_QKV); ap.ldq = C; ap.kall = ptr(kall); ap.vtall = ptr(vtall); ap.out = ptr(s_ATT); ap.ldo = C;
      ap.B = Bn; ap.H = Hh; ap.T = T; ap.Tk = Tk; ap.Tkp = Tkp; ap.scale = 0.125f;
      ap.out_x3 = k22_is_split(dt) ? 1 : 0;   // proj_out reads it as an x3-chunk operand
      return launch_attention(ap, dt, st);
    }, OP_ATTN, 4.0 * Bn * Hh * (double)T * Tk * 64.0, 0.0, 1));
    Act a; a.s0 = s_ATT; a.C0 = C; a.H = in.H; a.W = in.W;
    // proj_out + residual; its epilogue also delivers the GroupNorm partial sums the next ResBlock needs
    Tuned* tp = op_gemm(ops, a, B * T, C, pfx + ".proj_out", &in, dst, 0, IG_OUT_ROWMAJOR, dst_stats);
    return produced(dst, C, in.H, in.W, tp, dst_stats);
  }

  bool has_attn(int ds) const {
    for (int i = 0; i < cfg.n_attention_ds; ++i) if (cfg.attention_ds[i] == ds) return true;
    return false;
  }

  int plan(int nB, int nH, int nW) {
    // validate before touching the current plan: a rejected shape leaves the engine usable at the old one
    const int n_down = cfg.n_levels - 1;
    if (nB < 1 || nH < 1 || nW < 1) return k22_set_error(K22_EINVAL, "unet: B, H, W must be positive");
    if (nH % (1 << n_down) || nW % (1 << n_down)) return k22_set_error(K22_EINVAL, "unet: H, W must be divisible by 2^(levels-1)");
    if (nB > 8) return k22_set_error(K22_EINVAL, "unet: batch (2*bs) must be <= 8 per engine call");
    begin_plan();
    B = nB; H = nH; W = nW;
    ops.clear(); cond_ops.clear(); hint_ops.clear(); s_ctxkv.clear(); frag_jobs.clear(); frag_done = false; n_attn = 0;
    cond_set = false; hint_set = false;
    loop.drop();
    const int mc = cfg.model_channels, ted = 4 * mc;

    // total FiLM width = sum over ResBlocks of 2*Cout, in module order
    film_total = 0;
    {
      int ch = mc * cfg.channel_mult[0];
      for (int l = 0; l < cfg.n_levels; ++l) {
        for (int i = 0; i < cfg.num_res_blocks; ++i) { ch = mc * cfg.channel_mult[l]; film_total += 2 * ch; }
        if (l != cfg.n_levels - 1) film_total += 2 * ch;
      }
      film_total += 2 * 2 * ch;  // middle
      for (int l = cfg.n_levels - 1; l >= 0; --l)
        for (int i = 0; i <= cfg.num_res_blocks; ++i) {
          ch = mc * cfg.channel_mult[l];
          film_total += 2 * ch;
          if (l && i == cfg.num_res_blocks) film_total += 2 * ch;
        }
    }

    s_xin = new_slot((size_t)B * 4 * H * W * 4); s_img = new_slot((size_t)B * 4 * H * W * 4);
    s_mask = new_slot((size_t)B * H * W * 4); s_t = new_slot((size_t)B * 4 + 64);
    s_out = new_slot((size_t)B * cfg.out_channels * H * W * 4);
    s_temb = new_slot((size_t)B * mc * 4); s_e1 = new_slot((size_t)B * ted * 4); s_emb = new_slot((size_t)B * ted * 4);
    s_film = new_slot((size_t)B * film_total * 4); s_xfproj = new_slot((size_t)B * ted * 4);
    s_ctx = new_slot((size_t)B * cfg.ctx_len * cfg.ctx_dim * esz);
    const int ntext_p = cfg.ctx_len - cfg.n_image_embs;   // text tokens (0 for the 2.2 head)
    s_full = new_slot((size_t)B * (ntext_p > 0 ? ntext_p : 1) * cfg.text_dim1 * 4); s_pool = new_slot((size_t)B * cfg.text_dim2 * 4);
    s_imgemb = new_slot((size_t)B * cfg.image_dim * 4);
    s_tmpf = new_slot((size_t)B * cfg.n_image_embs * cfg.ctx_dim * 4 + (size_t)B * ted * 4);
    s_tmpf2 = new_slot((size_t)B * ted * 4);
    s_fullT = new_slot((size_t)B * (ntext_p > 0 ? ntext_p : 1) * cfg.text_dim1 * esz);
    s_ctxf = new_slot(cfg.head_type == 1 ? (size_t)B * cfg.ctx_len * cfg.ctx_dim * 4 : 0);
    if (cfg.hint_channels) {
      s_hint = new_slot((size_t)B * 4 * H * W * 4);
      s_hintin = new_slot((size_t)B * cfg.hint_channels * 64 * H * W * 4);
      for (int i = 0; i < 2; ++i) s_hbuf[i] = new_slot((size_t)B * 16 * 64 * H * W * 4);   // widest stage: 16 ch at 8H x 8W
    }
    s_part = new_slot(); s_coeff = new_slot(); s_P1 = new_slot(); s_U1 = new_slot(); s_P2 = new_slot(); s_S = new_slot();
    s_N = new_slot(); s_QKV = new_slot(); s_KALL = new_slot(); s_VT = new_slot(); s_ATT = new_slot();
    s_splitk = new_slot(256);
    s_U1st = new_slot();
    s_flush = new_slot(autotune ? ((size_t)320 << 20) : 0);  // evicts the Infinity Cache between tuning runs
    for (int i = 0; i < 3; ++i) { s_h[i] = new_slot(); s_hst[i] = new_slot(); }
    int hrot = 0, hcur = 0;
    auto next_h = [&]() { hcur = hrot; hrot = (hrot + 1) % 3; return s_h[hcur]; };
    auto cur_hst = [&]() { return s_hst[hcur]; };

    if (cfg.head_type == 1) build_cond_ops_22(); else build_cond_ops();
    if (cfg.hint_channels) build_hint_ops();

    // ---- time embedding + all FiLM vectors -------------------------------------------------
    {
      tw.freqs = Wf("time_freqs");
      tw.w0 = Wf("time_embed.0.weight"); tw.b0 = Wf("time_embed.0.bias");
      tw.w2 = Wf("time_embed.2.weight"); tw.b2 = Wf("time_embed.2.bias");
      tw.we = W_("emb_layers.weight"); tw.be = Wf("emb_layers.bias");
      tw.mc = mc; tw.ted = ted; tw.dt = sdt;
      const int Bn = B;
      ops.push_back([=](hipStream_t st) {
        if (film_cur) return (int)K22_OK;   // a hoisted loop computed this step's rows before its first step
        return time_rows(ptr<float>(s_t), ptr<float>(s_temb), ptr<float>(s_e1), ptr<float>(s_emb), ptr<float>(s_film), Bn, st);
      });
    }

    // ---- input blocks ------------------------------------------------------------------------
    int64_t film_cursor = 0;
    std::vector<Act> hs;
    int ch = mc * cfg.channel_mult[0];
    {
      Slot* d = new_slot((size_t)B * H * W * ch * esz);
      ConvInParams cp = {};
      cp.w = Wf("input_blocks.0.0.weight"); cp.bias = Wf("input_blocks.0.0.bias");
      cp.B = B; cp.H = H; cp.W = W; cp.Cin = cfg.in_channels; cp.Cout = ch;
      const int dt = sdt; const bool inpaint = cfg.in_channels == 9, hinted = cfg.in_channels == 8;
      const int premul = (hinted || cfg.head_type == 1) ? 1 : 0;   // 2.2: channels 4-7 arrive as they are (hint latent / masked image)
      ops.push_back([=](hipStream_t st) {
        ConvInParams q = cp;
        q.x = ptr<float>(s_xin); q.img = inpaint ? ptr<float>(s_img) : (hinted ? ptr<float>(s_hint) : nullptr);
        q.mask = inpaint ? ptr<float>(s_mask) : nullptr; q.img_premul = premul;
        q.out = ptr(d);
        return launch_conv_in(q, dt, st);
      });
      Act a; a.s0 = d; a.C0 = ch; a.H = H; a.W = W;
      hs.push_back(a);
    }
    Act h = hs.back();
    int ds = 1, blk = 1;
    for (int l = 0; l < cfg.n_levels; ++l) {
      for (int i = 0; i < cfg.num_res_blocks; ++i) {
        const int co = mc * cfg.channel_mult[l];
        const std::string pfx = "input_blocks." + std::to_string(blk);
        Slot* d = new_slot();
        if (has_attn(ds)) {
          Slot* rd = next_h();
          Act r = resblock(pfx + ".0", h, co, 0, film_cursor, rd, cur_hst());
          h = attnblock(pfx + ".1", r, d, new_slot());
        } else {
          h = resblock(pfx + ".0", h, co, 0, film_cursor, d, new_slot());
        }
        ch = co; hs.push_back(h); ++blk;
      }
      if (l != cfg.n_levels - 1) {
        const std::string pfx = "input_blocks." + std::to_string(blk);
        Slot* d = new_slot();
        h = resblock(pfx + ".0", h, ch, 1, film_cursor, d, new_slot());
        hs.push_back(h); ++blk; ds *= 2;
      }
    }
    // ---- middle ------------------------------------------------------------------------------
    {
      Slot* d0 = next_h(); Slot* st0 = cur_hst();
      Act r = resblock("middle_block.0", h, ch, 0, film_cursor, d0, st0);
      Slot* da = next_h(); Slot* sta = cur_hst();
      Act a = attnblock("middle_block.1", r, da, sta);
      Slot* d2 = next_h(); Slot* st2 = cur_hst();
      h = resblock("middle_block.2", a, ch, 0, film_cursor, d2, st2);
    }
    // ---- output blocks ---------------------------------------------------------------------
    blk = 0;
    for (int l = cfg.n_levels - 1; l >= 0; --l) {
      for (int i = 0; i <= cfg.num_res_blocks; ++i) {
        const Act skip = hs.back(); hs.pop_back();
        Act cat; cat.s0 = h.s0; cat.C0 = h.C0; cat.s1 = skip.s0; cat.C1 = skip.C0; cat.H = h.H; cat.W = h.W;
        cat.p0 = h.p0; cat.st0 = h.st0; cat.p1 = skip.p0; cat.st1 = skip.st0;
        if (skip.H != h.H || skip.W != h.W) return k22_set_error(K22_EINVAL, "unet: skip shape mismatch");
        const int co = mc * cfg.channel_mult[l];
        const std::string pfx = "output_blocks." + std::to_string(blk);
        { Slot* d = next_h(); Slot* dst_st = cur_hst(); h = resblock(pfx + ".0", cat, co, 0, film_cursor, d, dst_st); }
        int sub = 1;
        if (has_attn(ds)) { Slot* da = next_h(); Slot* sta = cur_hst(); h = attnblock(pfx + "." + std::to_string(sub), h, da, sta); ++sub; }
        if (l && i == cfg.num_res_blocks) {
          { Slot* d = next_h(); Slot* dst_st = cur_hst(); h = resblock(pfx + "." + std::to_string(sub), h, co, 2, film_cursor, d, dst_st); }
          ds /= 2;
        }
        ch = co; ++blk;
      }
    }
    if (film_cursor != film_total) return k22_set_error(K22_EINVAL, "unet: internal FiLM width mismatch");
    // ---- out: GN + SiLU + conv3x3 -> fp32 NCHW ---------------------------------------------------
    op_gn(ops, h, "out.0", -1, K22_ACT_SILU, 0, 1, s_P1);
    op_conv(ops, CONV_HEAD, s_P1, H, W, ch, cfg.out_channels, "out.2", nullptr, s_out, IG_OUT_NCHW_F32);

    return finish_plan();
  }

  // Kandinsky 2.2 conditioning head (the UNet2DConditionModel injected at kandinsky2_2_model.py:26-41; arithmetic of diffusers'
  // ImageProjection / ImageTimeEmbedding, restated in oracle/unet22_ref.py): image-only.
  //   ctx[b][0:S] = LayerNorm_768( Linear(image_dim -> S*768)(image_emb[b]) viewed [S][768] )      (encoder_hid_proj)
  //   emb        += LayerNorm_1536( Linear(image_dim -> 1536)(image_emb[b]) )                       (add_embedding)
  void build_cond_ops_22() {
    const int mc = cfg.model_channels, ted = 4 * mc, Bn = B, dt = sdt;
    const int cd = cfg.ctx_dim, S = cfg.ctx_len, di = cfg.image_dim;
    const float* w_cp = Wf("head22.ctx_proj.weight"); const float* b_cp = Wf("head22.ctx_proj.bias");
    const float* g_cn = Wf("head22.ctx_norm.weight"); const float* b_cn = Wf("head22.ctx_norm.bias");
    const float* w_ep = Wf("head22.emb_proj.weight"); const float* b_ep = Wf("head22.emb_proj.bias");
    const float* g_en = Wf("head22.emb_norm.weight"); const float* b_en = Wf("head22.emb_norm.bias");
    cond_ops.push_back([=](hipStream_t st) {
      float* proj = ptr<float>(s_tmpf);                       // [B][S*cd]
      float* embp = ptr<float>(s_tmpf) + (size_t)Bn * S * cd;  // [B][ted]
      LinearSmallParams lp = {};
      lp.x = ptr<float>(s_imgemb); lp.ldx = di; lp.W = w_cp; lp.bias = b_cp; lp.out = proj; lp.ldo = S * cd;
      lp.M = Bn; lp.N = S * cd; lp.K = di;
      int rc = launch_linear_smallm(lp, K22_F32, st);
      if (rc) return rc;
      rc = launch_layernorm_f32(proj, g_cn, b_cn, ptr<float>(s_ctxf), Bn * S, cd, 1e-5f, st);
      if (rc) return rc;
      rc = launch_cast_rows(ptr<float>(s_ctxf), ptr(s_ctx), Bn * S, cd, cd, cd, dt, st);
      if (rc) return rc;
      lp.W = w_ep; lp.bias = b_ep; lp.out = embp; lp.ldo = ted; lp.N = ted;
      rc = launch_linear_smallm(lp, K22_F32, st);
      if (rc) return rc;
      return launch_layernorm_f32(embp, g_en, b_en, ptr<float>(s_xfproj), Bn, ted, 1e-5f, st);
    });
  }

  // input_hint_block of diffusers' ImageHintTimeEmbedding (ControlNet-depth UNet of Kandinsky 2.2): eight 3x3 convolutions,
  // SiLU between them, three of them stride 2: [B,3,8H,8W] -> [B,4,H,W].
  void build_hint_ops() {
    static const int chans[9] = {0, 16, 16, 32, 32, 96, 96, 256, 4};
    static const int strides[8] = {1, 1, 2, 1, 2, 1, 2, 1};
    int hin = 8 * H, win = 8 * W, cin = cfg.hint_channels;
    for (int k = 0; k < 8; ++k) {
      const float* w = Wf("hint." + std::to_string(k) + ".weight");
      const float* b = Wf("hint." + std::to_string(k) + ".bias");
      const int cout = chans[k + 1], stride = strides[k], Bn = B, ci = cin, hi = hin, wi = win;
      Slot* src = k == 0 ? s_hintin : s_hbuf[(k - 1) & 1];
      Slot* dst = k == 7 ? s_hint : s_hbuf[k & 1];
      hint_ops.push_back([=](hipStream_t st) {
        ConvDirectParams q = {};
        q.x = ptr<float>(src); q.w = w; q.bias = b; q.y = ptr<float>(dst);
        q.B = Bn; q.Cin = ci; q.Cout = cout; q.Hin = hi; q.Win = wi; q.stride = stride; q.act = k == 7 ? K22_ACT_NONE : K22_ACT_SILU;
        return launch_conv3x3_direct(q, st);
      });
      cin = cout;
      if (stride == 2) { hin = (hin - 1) / 2 + 1; win = (win - 1) / 2 + 1; }
    }
  }

  // Text2ImUNet.get_text_emb (text2im_model2_1.py:57-80), pooling_type == "from_model".
  void build_cond_ops() {
    const int mc = cfg.model_channels, ted = 4 * mc, Bn = B, dt = sdt;
    const int nie = cfg.n_image_embs, cd = cfg.ctx_dim, S = cfg.ctx_len, ntext = S - nie;
    const float* w_cs = Wf("clip_to_seq.weight"); const float* b_cs = Wf("clip_to_seq.bias");
    const float* w_pn = Wf("proj_n.weight"); const float* b_pn = Wf("proj_n.bias");
    const float* g_ln = Wf("ln_model_n.weight"); const float* b_ln = Wf("ln_model_n.bias");
    const float* w_il = Wf("img_layer.weight"); const float* b_il = Wf("img_layer.bias");
    const int d1 = cfg.text_dim1, d2 = cfg.text_dim2, di = cfg.image_dim;
    cond_ops.push_back([=](hipStream_t st) {
      float* clipseq = ptr<float>(s_tmpf);                  // [B][nie*cd]
      float* proj = ptr<float>(s_tmpf) + (size_t)Bn * nie * cd;  // [B][ted]
      LinearSmallParams lp = {};
      lp.x = ptr<float>(s_imgemb); lp.ldx = di; lp.W = w_cs; lp.bias = b_cs; lp.out = clipseq; lp.ldo = nie * cd;
      lp.M = Bn; lp.N = nie * cd; lp.K = di;
      int rc = launch_linear_smallm(lp, K22_F32, st);
      if (rc) return rc;
      // ctx[b][0:nie] = clip_seq
      for (int b = 0; b < Bn; ++b) {
        rc = launch_cast_rows(clipseq + (size_t)b * nie * cd, ptr(s_ctx) + (size_t)b * S * cd * esz, nie, cd, cd, cd, dt, st);
        if (rc) return rc;
      }
      // xf_proj = LN(proj_n(pooled)) + img_layer(image_emb)
      lp.x = ptr<float>(s_pool); lp.ldx = d2; lp.W = w_pn; lp.bias = b_pn; lp.out = proj; lp.ldo = ted; lp.N = ted; lp.K = d2;
      rc = launch_linear_smallm(lp, K22_F32, st);
      if (rc) return rc;
      rc = launch_layernorm_f32(proj, g_ln, b_ln, ptr<float>(s_tmpf2), Bn, ted, 1e-5f, st);
      if (rc) return rc;
      lp.x = ptr<float>(s_imgemb); lp.ldx = di; lp.W = w_il; lp.bias = b_il; lp.add = ptr<float>(s_tmpf2); lp.ld_add = ted;
      lp.out = ptr<float>(s_xfproj); lp.ldo = ted; lp.N = ted; lp.K = di;
      rc = launch_linear_smallm(lp, K22_F32, st);
      if (rc) return rc;
      // full_emb -> T
      return launch_cast_rows(ptr<float>(s_full), ptr(s_fullT), Bn * ntext, d1, d1, d1, dt, st);
    });
    // ctx[b][nie:S] = to_model_dim_n(full_emb[b])   (one GEMM per batch element: rows re-strided)
    {
      IgemmParams p = igemm_gemm_problem(ntext, cd, d1, 0);
      p.splitk = 1;
      p.a_raw = k22_is_split(dtype) ? 1 : 0;   // s_fullT: plain rows written by cast_rows
      p.Wp = W_("to_model_dim_n.weight"); p.bias = Wf("to_model_dim_n.bias");
      const size_t es = esz;
      const int gdt = gemm_dt(false);
      cond_ops.push_back([=](hipStream_t st) {
        for (int b = 0; b < Bn; ++b) {
          IgemmParams q = p;
          q.A0 = ptr(s_fullT) + (size_t)b * ntext * d1 * es;
          q.out = ptr(s_ctx) + ((size_t)b * S + nie) * cd * es;
          int rc = launch_igemm(q, gdt, st);
          if (rc) return rc;
        }
        return K22_OK;
      });
    }
  }
};

static int refuse(const char* who, const char* what) { return k22_set_error(K22_EINVAL, (std::string(who) + ": " + what).c_str()); }

// what a forward needs of the handle, asked by k22_unet_forward and every loop entry; `who`: the entry's name, the prefix of its messages
static int unet_ready(const K22UNet* u, const char* who, const float* inpaint_image, const float* inpaint_mask) {
  if (!u || !u->ws) return refuse(who, "bind a workspace first");
  if (!u->cond_set) return refuse(who, "call k22_unet_set_condition first");
  if (u->cfg.in_channels == 9 && (!inpaint_image || !inpaint_mask)) return refuse(who, "inpainting UNet needs inpaint_image and inpaint_mask");
  if (u->cfg.hint_channels && !u->hint_set) return refuse(who, "call k22_unet_set_hint first");
  return K22_OK;
}

// ---- the one driver of the whole-loop entries ---------------------------------------------------------------------------------------------
// A loop updates x [B][4][HW] in place over n_steps steps (x_tmp: scratch of the same size, the other end of the ping-pong) with n_calls model
// calls in all, on device buffers the caller filled BEFORE the call (timesteps [n_calls][B]: the values the UNet receives, in execution
// order).  Eagerly, or as the engine's ONE captured graph, replayed as long as the same buffers and scalars are passed (a generation service
// re-uses its buffers); anything else, another kind included, re-captures.
struct UNetLoop {
  const char* who;           // the entry's name: prefix of the refusals
  unsigned long long kind;   // K22_LOOP_KIND_*: first word of the key
  float *x, *x_tmp;
  const float *timesteps, *inpaint_image, *inpaint_mask;
  int n_steps, n_calls, use_graph;
  void* stream;
};
// The entry supplies
//   own_fault()                   its own argument checks, asked once the handle is known to be bound: the message of the first one that fails, or null
//   step(k, cur, nxt, model, s)   the launches of step k behind its first model call (done: model_out() holds UNet(cur)), writing the next latent to
//                                 nxt; model(latent) runs the loop's next model call on another latent (PLMS: its first step calls it on nxt)
//   key_tail(key)                 appends every pointer and scalar the step bakes into its nodes (the operands above are the driver's to add);
//                                 asked after the checks, so it may read the host arrays they vouch for
// Everything is validated before loop_begin, which may drop the captured loop: a refused call leaves the handle as it was.
template <typename Fault, typename Step, typename Tail>
static int unet_loop(K22UNet* u, const UNetLoop& a, Fault own_fault, Step step, Tail key_tail) {
  if (int rc = unet_ready(u, a.who, a.inpaint_image, a.inpaint_mask)) return rc;
  if (const char* what = own_fault()) return refuse(a.who, what);
  if (u->B % 2) return refuse(a.who, "the batch is the CFG batch [cond | uncond] (even)");
  if (u->cfg.out_channels != 8) return refuse(a.who, "the UNet must predict eps and variance (8 channels)");
  hipStream_t st = reinterpret_cast<hipStream_t>(a.stream);
  K22UNet::LoopRows lr;
  if (int rc = u->loop_begin(a.n_calls, st, &lr)) return rc;
  auto steps = [&](hipStream_t s) -> int {
    if (int rc = u->loop_prologue(lr, a.timesteps, a.n_calls, a.inpaint_image, a.inpaint_mask, s)) return rc;
    float* cur = a.x; float* nxt = a.x_tmp;
    int call = 0;
    auto model = [&](const float* latent) { return u->loop_model(lr, latent, a.timesteps, call++, s); };
    for (int k = 0; k < a.n_steps; ++k) {
      if (int rc = model(cur)) return rc;
      if (int rc = step(k, cur, nxt, model, s)) return rc;
      float* t_ = cur; cur = nxt; nxt = t_;
    }
    if (cur != a.x) return copy_d2d(a.x, cur, (size_t)u->B * 4 * u->H * u->W * sizeof(float), s);
    return K22_OK;
  };
  auto body = [&](hipStream_t s) -> int { const int rc = steps(s); u->film_cur = nullptr; return rc; };
  std::vector<unsigned long long> key = {a.kind, loop_key_ptr(a.x), loop_key_ptr(a.x_tmp), loop_key_ptr(a.timesteps), loop_key_ptr(a.inpaint_image),
      loop_key_ptr(a.inpaint_mask), (unsigned long long)a.n_steps, (unsigned long long)(lr.hoist ? 1 : 0)};
  key_tail(key);
  // a plan that has not run a forward has no captured loop either (begin_plan drops both): this is the warm-up before a first capture
  if (a.use_graph && !u->warmed) { if (int rc = u->loop_warm(a.timesteps, a.inpaint_image, a.inpaint_mask, st)) return rc; }
  return u->loop.run(u->cap, key, a.use_graph, st, body);
}

// The whole classifier-free-guided p_sampler loop of Kandinsky2_1.generate_img (kandinsky2_1_model.py:222-257 ->
// gaussian_diffusion.py:384-475) as ONE hipGraph: for every step  UNet([x_half | x_half], t_k) -> k22_sampler_step  with no host work
// between steps (the reference returns to Python - and to the CPU for np.percentile - at every step).  Beside the driver's operands:
// noise_seq [n_steps][B][4][HW] (the ancestral noise of every step, drawn up front), table [T][8] + table_rows[k] (host array: the
// schedule row of step k).
// keep_* (all four or none): after every step the known region of the 2.2 inpainting pipeline is re-imposed on the freshly written latent
// (launch_keep_region, prestep.hip) with keep_coef[k] = (sa, sb) of step k, a HOST array; none = the loop k22_unet_sample_loop has always run.
static int unet_sample_loop_body(K22UNet* u, float* x, float* x_tmp, const float* timesteps, const float* noise_seq, const float* init_img,
                                 const float* mask, const float* inpaint_image, const float* inpaint_mask, const float* table,
                                 const int* table_rows, int n_steps, float guidance, float clamp_lo, float clamp_hi, int pct_index,
                                 double pct_gamma, void* scratch, const float* keep_init, const float* keep_noise, const float* keep_mask,
                                 const float* keep_coef, int use_graph, void* stream) {
  auto own_fault = [&]() -> const char* {
    if (!x || !x_tmp || !timesteps || !noise_seq || !table || !table_rows || !scratch || n_steps < 1) return "null argument";
    if (pct_index >= 4 * u->H * u->W) return "percentile index out of range";
    if (const int g = u->threshold_group) {
      if (u->B % 2 == 0 && ((u->B / 2) % g || u->B / 2 / g > 64)) return "the threshold group (k22_unet_set_threshold_group) must divide B / 2 into at most 64 groups";
    }
    return nullptr;
  };
  auto step = [&](int k, float* cur, float* nxt, auto&, hipStream_t s) -> int {
    const int B = u->B, HW = u->H * u->W;
    SamplerParams p = {};
    p.x = cur; p.model_out = u->model_out(); p.noise = noise_seq + (size_t)k * B * 4 * HW; p.init_img = init_img; p.mask = mask;
    p.table = table; p.step = nullptr; p.step_host = table_rows[k]; p.guidance = guidance; p.clamp_lo = clamp_lo; p.clamp_hi = clamp_hi;
    p.use_cfg = 1; p.n_lo = pct_index; p.gamma = pct_gamma; p.pct_group = u->threshold_group;
    p.s_buf = reinterpret_cast<float*>(scratch); p.x0_buf = reinterpret_cast<float*>(scratch) + 64;
    p.x_out = nxt; p.x0_out = nullptr; p.N = B; p.HW = HW;
    if (int rc = launch_sampler_step(p, s)) return rc;
    if (!keep_init) return K22_OK;
    return launch_keep_region(nxt, keep_init, keep_noise, keep_mask, keep_coef[2 * k], keep_coef[2 * k + 1], nxt, B, HW, s);
  };
  auto key_tail = [&](std::vector<unsigned long long>& key) {
    key.insert(key.end(), {loop_key_ptr(noise_seq), loop_key_ptr(init_img), loop_key_ptr(mask), loop_key_ptr(table), loop_key_ptr(scratch),
                           (unsigned long long)pct_index, loop_key_bits(guidance), loop_key_bits(clamp_lo), loop_key_bits(clamp_hi), loop_key_bits(pct_gamma),
                           (unsigned long long)u->threshold_group});
    for (int k = 0; k < n_steps; ++k) key.push_back((unsigned long long)table_rows[k]);
    if (!keep_init) return;
    // the three device operands and the bits of every coefficient baked into the keep-region nodes
    key.insert(key.end(), {loop_key_ptr(keep_init), loop_key_ptr(keep_noise), loop_key_ptr(keep_mask)});
    for (int k = 0; k < 2 * n_steps; ++k) key.push_back(loop_key_bits(keep_coef[k]));
  };
  const UNetLoop a = {"unet_sample_loop", keep_init ? K22_LOOP_KIND_P_KEEP : K22_LOOP_KIND_P, x, x_tmp, timesteps, inpaint_image, inpaint_mask,
                      n_steps, n_steps, use_graph, stream};
  return unet_loop(u, a, own_fault, step, key_tail);
}

// The DPM-Solver++ loop of k22_unet_dpmpp_loop (clamp == NULL: the step is k22_dpmpp_step, the key and the kind what they have always been)
// and k22_unet_dpmpp_loop_keep (clamp = host (lo, hi): the step is k22_dpmpp_step_clip; keep_* all four or none, as in unet_sample_loop_body).
// Step k writes its x0 to slot k % 2 of x0_hist and, when orders[k] == 2, reads slot (k - 1) % 2: the rotation is resolved here, at capture
// time, like the PLMS ring - so every order is in the key.
static int unet_dpmpp_loop_body(K22UNet* u, const char* who, float* x, float* x_tmp, float* x0_hist, const float* timesteps, const float* table,
                                const int* orders, const float* inpaint_image, const float* inpaint_mask, int n_steps, float guidance,
                                const float* clamp, const float* keep_init, const float* keep_noise, const float* keep_mask,
                                const float* keep_coef, int use_graph, void* stream) {
  auto own_fault = [&]() -> const char* {
    if (!x || !x_tmp || !x0_hist || !timesteps || !table || !orders) return "null argument";
    if (n_steps < 1) return "n_steps must be >= 1";
    for (int k = 0; k < n_steps; ++k)
      if (orders[k] != 1 && orders[k] != 2) return "every order is 1 or 2";
    if (orders[0] != 1) return "the first step has no history (orders[0] must be 1)";
    if (clamp && !(clamp[0] <= clamp[1])) return "clamp_lo <= clamp_hi, neither a NaN";
    return nullptr;
  };
  auto step = [&](int k, float* cur, float* nxt, auto&, hipStream_t s) -> int {
    const int B = u->B, HW = u->H * u->W;
    const size_t lat = (size_t)B * 4 * HW;
    float* x0_new = x0_hist + (size_t)(k % 2) * lat;
    const float* x0_old = orders[k] == 2 ? x0_hist + (size_t)((k + 1) % 2) * lat : nullptr;
    const float* row = table + (size_t)k * 5;
    if (!clamp) return launch_dpmpp_step(cur, u->model_out(), x0_old, row, guidance, 1, nxt, x0_new, B, HW, s);
    if (int rc = launch_dpmpp_step_clip(cur, u->model_out(), x0_old, row, guidance, 1, clamp[0], clamp[1], nxt, x0_new, B, HW, s)) return rc;
    if (!keep_init) return K22_OK;
    return launch_keep_region(nxt, keep_init, keep_noise, keep_mask, keep_coef[2 * k], keep_coef[2 * k + 1], nxt, B, HW, s);
  };
  auto key_tail = [&](std::vector<unsigned long long>& key) {
    key.insert(key.end(), {loop_key_ptr(x0_hist), loop_key_ptr(table), loop_key_bits(guidance)});
    for (int k = 0; k < n_steps; ++k) key.push_back((unsigned long long)orders[k]);
    if (!clamp) return;
    key.insert(key.end(), {loop_key_bits(clamp[0]), loop_key_bits(clamp[1])});
    if (!keep_init) return;
    // the three device operands and the bits of every coefficient baked into the keep-region nodes
    key.insert(key.end(), {loop_key_ptr(keep_init), loop_key_ptr(keep_noise), loop_key_ptr(keep_mask)});
    for (int k = 0; k < 2 * n_steps; ++k) key.push_back(loop_key_bits(keep_coef[k]));
  };
  const unsigned long long kind = !clamp ? K22_LOOP_KIND_DPMPP : keep_init ? K22_LOOP_KIND_DPMPP_KEEP : K22_LOOP_KIND_DPMPP_CLIP;
  const UNetLoop a = {who, kind, x, x_tmp, timesteps, inpaint_image, inpaint_mask, n_steps, n_steps, use_graph, stream};
  return unet_loop(u, a, own_fault, step, key_tail);
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

int k22_unet_create(const K22UNetConfig* cfg, const K22Weight* weights, int n_weights, K22UNet** out) {
  if (!cfg || !out) return k22_set_error(K22_EINVAL, "unet_create: null argument");
  if (!k22_dtype_ok(cfg->dtype) && !k22_is_split(cfg->dtype)) return k22_set_error(K22_EINVAL, "unet_create: dtype");
  if (cfg->num_head_channels != 64) return k22_set_error(K22_EINVAL, "unet_create: only num_head_channels == 64");
  if (cfg->model_channels % 128) return k22_set_error(K22_EINVAL, "unet_create: model_channels % 128");
  if (cfg->n_levels < 1 || cfg->n_levels > 8) return k22_set_error(K22_EINVAL, "unet_create: n_levels");
  if (cfg->in_channels != 4 && cfg->in_channels != 9 && cfg->in_channels != 8) return k22_set_error(K22_EINVAL, "unet_create: in_channels must be 4, 8 or 9");
  if (cfg->head_type != 0 && cfg->head_type != 1) return k22_set_error(K22_EINVAL, "unet_create: head_type must be 0 (2.1) or 1 (2.2)");
  if ((cfg->hint_channels != 0) != (cfg->in_channels == 8) || (cfg->hint_channels != 0 && cfg->hint_channels != 3))
    return k22_set_error(K22_EINVAL, "unet_create: hint_channels = 3 goes with in_channels = 8 (latent + hint latent), else 0");
  if (cfg->head_type == 1 && cfg->n_image_embs != cfg->ctx_len) return k22_set_error(K22_EINVAL, "unet_create: the 2.2 head has image tokens only (n_image_embs == ctx_len)");
  K22UNet* u = new K22UNet();
  u->cfg = *cfg; u->set_dtype(cfg->dtype); u->sdt = k22_storage_dtype(cfg->dtype);
  u->stream_frag = env_flag("K22_STREAM", 1);     // 0 = no fragment-major weight copies, no weight-streaming kernel
  u->fuse_skip = env_flag("K22_FUSE_SKIP", 1);    // 0 = 1x1 skip connections as separate GEMMs
  u->hoist_time = env_flag("K22_HOIST_TIME", 1);  // 0 (measurement only) = k22_unet_sample_loop keeps the per-step time-embedding / FiLM launches
  const char* xp = getenv("K22_X2_PLAN");         // K22_F16X2 only: which of the top level's convolutions run with two MFMAs (K22UNet::x2_plan)
  u->x2_plan = xp ? (atoi(xp) & 3) : 0;
  u->set_weights(weights, n_weights);
  *out = u;
  return K22_OK;
}

void k22_unet_destroy(K22UNet* u) { delete u; }

int k22_unet_plan(K22UNet* u, int B, int H, int W, size_t* workspace_bytes) {
  if (!u || !workspace_bytes) return k22_set_error(K22_EINVAL, "unet_plan: null argument");
  int rc = u->plan(B, H, W);
  if (rc) return rc;
  *workspace_bytes = u->ws_bytes;
  return K22_OK;
}

int k22_unet_bind(K22UNet* u, void* workspace, size_t workspace_bytes) {
  if (!u) return k22_set_error(K22_EINVAL, "unet_bind: null argument");
  if (int rc = u->bind(workspace, workspace_bytes, "unet_bind")) return rc;
  u->cond_set = false; u->hint_set = false; u->frag_done = false;
  u->loop.drop();
  return K22_OK;
}

int k22_unet_set_condition(K22UNet* u, const float* full_emb, const float* pooled_emb, const float* image_emb, void* stream) {
  if (!u || !u->ws) return k22_set_error(K22_EINVAL, "unet_set_condition: bind a workspace first");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const K22UNetConfig& c = u->cfg;
  const int ntext = c.ctx_len - c.n_image_embs;
  if (!image_emb) return k22_set_error(K22_EINVAL, "unet_set_condition: image_emb is required");
  if (c.head_type == 0 && (!full_emb || !pooled_emb)) return k22_set_error(K22_EINVAL, "unet_set_condition: the 2.1 head needs full_emb and pooled_emb");
  const size_t pb = (size_t)u->B;
  if (c.head_type == 0) {
    if (int rc = copy_d2d(u->ptr(u->s_full), full_emb, pb * ntext * c.text_dim1 * 4, st)) return rc;
    if (int rc = copy_d2d(u->ptr(u->s_pool), pooled_emb, pb * c.text_dim2 * 4, st)) return rc;
  }
  if (int rc = copy_d2d(u->ptr(u->s_imgemb), image_emb, pb * c.image_dim * 4, st)) return rc;
  for (auto& op : u->cond_ops) { int rc = op(st); if (rc) return rc; }
  u->cond_set = true;
  return K22_OK;
}

int k22_unet_set_hint(K22UNet* u, const float* hint, void* stream) {
  if (!u || !u->ws) return k22_set_error(K22_EINVAL, "unet_set_hint: bind a workspace first");
  if (!u->cfg.hint_channels) return k22_set_error(K22_EINVAL, "unet_set_hint: this UNet has no hint input (hint_channels == 0)");
  if (!hint) return k22_set_error(K22_EINVAL, "unet_set_hint: null hint");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t per = (size_t)u->B * u->cfg.hint_channels * 64 * u->H * u->W;
  if (int rc = copy_d2d(u->ptr(u->s_hintin), hint, per * 4, st)) return rc;
  for (auto& op : u->hint_ops) { int rc = op(st); if (rc) return rc; }
  u->hint_set = true;
  return K22_OK;
}

int k22_unet_set_threshold_group(K22UNet* u, int rows) {
  if (!u) return k22_set_error(K22_EINVAL, "unet_set_threshold_group: null handle");
  if (rows < 0) return k22_set_error(K22_EINVAL, "unet_set_threshold_group: rows must be >= 0 (0 = the whole batch)");
  u->threshold_group = rows;
  return K22_OK;
}

int k22_unet_forward(K22UNet* u, const float* x, const float* timesteps, const float* inpaint_image,
                     const float* inpaint_mask, float* out, int use_graph, void* stream) {
  if (int rc = unet_ready(u, "unet_forward", inpaint_image, inpaint_mask)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t hw = (size_t)u->H * u->W;
  const size_t pb = (size_t)u->B;
  if (int rc = copy_d2d(u->ptr(u->s_xin), x, pb * 4 * hw * 4, st)) return rc;
  if (int rc = copy_d2d(u->ptr(u->s_t), timesteps, pb * 4, st)) return rc;
  if (int rc = u->stage_inpaint(inpaint_image, inpaint_mask, st)) return rc;
  // first forward on this plan: fragment-major weight copies; conv / GEMM problems the tile table does not know are measured on the device
  { int rc = u->prepare_run(st); if (rc) return rc; }
  // graph: warm-up eagerly once per plan (sets function attributes), then capture and replay
  const int rc = use_graph ? u->replay(u->graph, st, [u](hipStream_t s) { return u->exec(s); }) : u->exec_eager(st);
  if (rc) return rc;
  return copy_d2d(out, u->ptr(u->s_out), pb * u->cfg.out_channels * hw * 4, st);
}

int k22_unet_sample_loop(K22UNet* u, float* x, float* x_tmp, const float* timesteps, const float* noise_seq, const float* init_img,
                         const float* mask, const float* inpaint_image, const float* inpaint_mask, const float* table,
                         const int* table_rows, int n_steps, float guidance, float clamp_lo, float clamp_hi, int pct_index,
                         double pct_gamma, void* scratch, int use_graph, void* stream) {
  return unet_sample_loop_body(u, x, x_tmp, timesteps, noise_seq, init_img, mask, inpaint_image, inpaint_mask, table, table_rows, n_steps,
                               guidance, clamp_lo, clamp_hi, pct_index, pct_gamma, scratch, nullptr, nullptr, nullptr, nullptr, use_graph, stream);
}

// k22_unet_sample_loop with the known region of the Kandinsky 2.2 inpainting pipeline re-imposed after every step (diffusers
// KandinskyV22InpaintPipeline loop, driven by kandinsky2_2_model.py:150-173): per step  UNet -> k22_sampler_step -> k22_keep_region on the
// freshly written latent, one chain on the capture stream.  All four keep arguments NULL: k22_unet_sample_loop itself.
int k22_unet_sample_loop_keep(K22UNet* u, float* x, float* x_tmp, const float* timesteps, const float* noise_seq, const float* init_img,
                              const float* mask, const float* inpaint_image, const float* inpaint_mask, const float* table,
                              const int* table_rows, int n_steps, float guidance, float clamp_lo, float clamp_hi, int pct_index,
                              double pct_gamma, void* scratch, const float* keep_init, const float* keep_noise, const float* keep_mask,
                              const float* keep_coef, int use_graph, void* stream) {
  const int n_keep = (keep_init != nullptr) + (keep_noise != nullptr) + (keep_mask != nullptr) + (keep_coef != nullptr);
  if (n_keep != 0 && n_keep != 4)
    return k22_set_error(K22_EINVAL, "unet_sample_loop_keep: keep_init, keep_noise, keep_mask and keep_coef go together (all four or none)");
  return unet_sample_loop_body(u, x, x_tmp, timesteps, noise_seq, init_img, mask, inpaint_image, inpaint_mask, table, table_rows, n_steps,
                               guidance, clamp_lo, clamp_hi, pct_index, pct_gamma, scratch, keep_init, keep_noise, keep_mask, keep_coef, use_graph,
                               stream);
}

// The whole classifier-free-guided DDIM or PLMS loop of Kandinsky2_1.generate_img (kandinsky2_1_model.py:222-233 -> samplers.py:206-331,
// 475-637) as ONE hipGraph: unet_loop with k22_ddim_step / k22_plms_step as the step.  PLMS: the rotation of the
// eps ring is resolved here, at capture time - every captured plms_step node holds fixed h1 / h2 / h3 / eps_out pointers.
int k22_unet_ddim_loop(K22UNet* u, int kind, float* x, float* x_tmp, float* x0_out, const float* timesteps, const float* table,
                       const float* noise_seq, const float* inpaint_image, const float* inpaint_mask, float* eps_hist, int n_steps,
                       float guidance, int use_graph, void* stream) {
  auto own_fault = [&]() -> const char* {
    if (kind != K22_LOOP_DDIM && kind != K22_LOOP_PLMS) return "kind must be K22_LOOP_DDIM or K22_LOOP_PLMS";
    if (!x || !x_tmp || !timesteps || !table) return "null argument";
    if (n_steps < 1) return "n_steps must be >= 1";
    if (kind == K22_LOOP_PLMS && noise_seq) return "PLMS is eta = 0 (samplers.py:355-356): noise_seq must be NULL";
    if (kind == K22_LOOP_PLMS && !eps_hist) return "PLMS needs the eps-history workspace (4 x [B][4][HW] floats)";
    return nullptr;
  };
  float* old[3] = {nullptr, nullptr, nullptr};   // PLMS: guided eps of earlier steps, newest first (the step runs once per call, if at all)
  int n_old = 0;
  auto step = [&](int k, float* cur, float* nxt, auto& model, hipStream_t s) -> int {
    const int B = u->B, HW = u->H * u->W;
    const size_t lat = (size_t)B * 4 * HW;
    const float* row = table + (size_t)k * 4;
    if (kind == K22_LOOP_DDIM)
      return launch_ddim_step(cur, u->model_out(), noise_seq ? noise_seq + (size_t)k * lat : nullptr, row, guidance, 1, nxt, x0_out, B, HW, s);
    float* e_buf = nullptr;   // the slot of the ring of four that holds none of the (at most three) live history tensors
    for (int j = 0; j < 4 && !e_buf; ++j) {
      float* c = eps_hist + (size_t)j * lat;
      if (c != old[0] && c != old[1] && c != old[2]) e_buf = c;
    }
    int rc;
    if (n_old == 0) {
      // stage one: e_t -> e_buf, provisional x_prev -> nxt; stage two: the model on it at the NEXT timestep, e' = (e_t + e_next) / 2
      rc = launch_plms_step(cur, u->model_out(), nullptr, nullptr, nullptr, 0, row, guidance, 1, nxt, e_buf, nullptr, B, HW, s);
      if (rc) return rc;
      rc = model(nxt);
      if (rc) return rc;
      rc = launch_plms_step(cur, u->model_out(), e_buf, nullptr, nullptr, 4, row, guidance, 1, nxt, nullptr, x0_out, B, HW, s);
    } else {
      rc = launch_plms_step(cur, u->model_out(), old[0], old[1], old[2], n_old, row, guidance, 1, nxt, e_buf, x0_out, B, HW, s);
    }
    old[2] = old[1]; old[1] = old[0]; old[0] = e_buf;
    if (n_old < 3) ++n_old;
    return rc;
  };
  auto key_tail = [&](std::vector<unsigned long long>& key) {
    key.insert(key.end(), {loop_key_ptr(x0_out), loop_key_ptr(table), loop_key_ptr(noise_seq), loop_key_ptr(eps_hist), loop_key_bits(guidance)});
  };
  // PLMS: the pseudo improved-Euler start calls the model twice
  const UNetLoop a = {"unet_ddim_loop", kind == K22_LOOP_PLMS ? K22_LOOP_KIND_PLMS : K22_LOOP_KIND_DDIM, x, x_tmp, timesteps, inpaint_image,
                      inpaint_mask, n_steps, kind == K22_LOOP_PLMS ? n_steps + 1 : n_steps, use_graph, stream};
  return unet_loop(u, a, own_fault, step, key_tail);
}

// The whole classifier-free-guided DPM-Solver++ loop (multistep, data prediction, orders 1 / 2M; no counterpart in the reference) as ONE
// hipGraph: unet_loop with k22_dpmpp_step as the step.  Step k writes its x0 to slot k % 2 of x0_hist and, when
// orders[k] == 2, reads slot (k - 1) % 2: the rotation is resolved here, at capture time, like the PLMS ring - so every order is in the key.
int k22_unet_dpmpp_loop(K22UNet* u, float* x, float* x_tmp, float* x0_hist, const float* timesteps, const float* table, const int* orders,
                        const float* inpaint_image, const float* inpaint_mask, int n_steps, float guidance, int use_graph, void* stream) {
  return unet_dpmpp_loop_body(u, "unet_dpmpp_loop", x, x_tmp, x0_hist, timesteps, table, orders, inpaint_image, inpaint_mask, n_steps, guidance,
                              nullptr, nullptr, nullptr, nullptr, nullptr, use_graph, stream);
}

// k22_unet_dpmpp_loop for the Kandinsky 2.2 decoders: the step is k22_dpmpp_step_clip (the scheduler's clip_sample on the data prediction) and,
// with the four keep arguments, the known region of the inpainting pipeline is re-imposed on the freshly written latent as in
// k22_unet_sample_loop_keep: per step  UNet -> k22_dpmpp_step_clip -> k22_keep_region, one chain on the capture stream.
int k22_unet_dpmpp_loop_keep(K22UNet* u, float* x, float* x_tmp, float* x0_hist, const float* timesteps, const float* table, const int* orders,
                             const float* inpaint_image, const float* inpaint_mask, int n_steps, float guidance, float clamp_lo, float clamp_hi,
                             const float* keep_init, const float* keep_noise, const float* keep_mask, const float* keep_coef,
                             int use_graph, void* stream) {
  const int n_keep = (keep_init != nullptr) + (keep_noise != nullptr) + (keep_mask != nullptr) + (keep_coef != nullptr);
  if (n_keep != 0 && n_keep != 4)
    return k22_set_error(K22_EINVAL, "unet_dpmpp_loop_keep: keep_init, keep_noise, keep_mask and keep_coef go together (all four or none)");
  const float clamp[2] = {clamp_lo, clamp_hi};
  return unet_dpmpp_loop_body(u, "unet_dpmpp_loop_keep", x, x_tmp, x0_hist, timesteps, table, orders, inpaint_image, inpaint_mask, n_steps,
                              guidance, clamp, keep_init, keep_noise, keep_mask, keep_coef, use_graph, stream);
}

int k22_unet_num_ops(const K22UNet* u) {
  return u && u->planned ? (int)u->ops.size() : 0;
}

int k22_unet_set_autotune(K22UNet* u, int on) {
  if (!u) return k22_set_error(K22_EINVAL, "unet_set_autotune: null handle");
  if (u->planned && (on != 0) != (u->autotune != 0)) return k22_set_error(K22_EINVAL, "unet_set_autotune: call before k22_unet_plan");
  u->autotune = on ? 1 : 0;
  return K22_OK;
}

// Text table of the chosen tile configurations (one line per distinct conv / GEMM problem of the plan).
int k22_unet_tuning_report(const K22UNet* u, char* buf, size_t cap) {
  if (!u || !buf || cap == 0) return k22_set_error(K22_EINVAL, "unet_tuning_report: null argument");
  const std::string out = tuning_report_text(u->tuned);
  snprintf(buf, cap, "%s", out.c_str());
  return K22_OK;
}

int k22_unet_profile(K22UNet* u, int reps, double* ms, double* flops, double* bytes, int* launches, void* stream) {
  if (!u || !u->ws || !u->cond_set) return k22_set_error(K22_EINVAL, "unet_profile: run k22_unet_forward once first");
  if (reps < 1) reps = 1;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (int k = 0; k < OP_NKINDS; ++k) { ms[k] = 0.0; flops[k] = 0.0; bytes[k] = 0.0; launches[k] = 0; }
  int rc = K22_OK;
  {
    K22UNet* q = u;
    if (!q->frag_done) { int rc0 = q->repack_frags(st); if (rc0) return rc0; }   // a profile before the first forward of this binding
    const size_t n = q->ops.size();
    std::vector<hipEvent_t> ev(2 * n);
    for (auto& e : ev) { hipError_t r = hipEventCreate(&e); if (r != hipSuccess) return k22_set_error_hip(r, __FILE__, __LINE__); }
    for (size_t i = 0; i < n; ++i) {
      flops[q->ops[i].kind] += q->ops[i].flops + q->ops[i].flops2;  // a fused 1x1 skip is work of the conv launch
      bytes[q->ops[i].kind] += q->ops[i].bytes;
      launches[q->ops[i].kind] += q->ops[i].kernels;
    }
    for (int r = 0; r < reps && rc == K22_OK; ++r) {
      for (size_t i = 0; i < n; ++i) {
        (void)hipEventRecord(ev[2 * i], st);
        rc = q->ops[i](st);
        (void)hipEventRecord(ev[2 * i + 1], st);
        if (rc) break;
      }
      hipError_t e = hipStreamSynchronize(st);
      if (e != hipSuccess) { rc = k22_set_error_hip(e, __FILE__, __LINE__); break; }
      for (size_t i = 0; i < n; ++i) {
        float t = 0.f;
        (void)hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]);
        ms[q->ops[i].kind] += (double)t / reps;
      }
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
  }
  return rc;
}

}  // extern "C"
