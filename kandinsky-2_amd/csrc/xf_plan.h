// k22 — the launch list of a transformer engine (prior.hip, encoder.hip) on top of plan.h: the list itself and the ops both engines build it
// from.  Every Linear is one launch_igemm over the [N][K] weight as the reference stores it, the fp32 residual stream is updated in place
// by the GEMM epilogue (mode 2), LayerNorm writes the next GEMM's T operand, self-attention over 64-channel heads is the UNet's flash kernel
// with a causal / key-validity mask.  The layer loops (pre-LN, post-LN, the prior's skinny path) stay with their engine.  Host-only.
#pragma once
#include "elementwise.h"
#include "plan.h"

#include <functional>
#include <string>
#include <vector>

struct XfPlan : GraphPlan {
  std::vector<std::function<int(hipStream_t)>> ops;
  // created by the engine's plan() among its own slots: split-K partials, the autotuner's cache flush, the flash kernel's packed K / V^T
  Slot *s_splitk = nullptr, *s_flush = nullptr, *s_kall = nullptr, *s_vtall = nullptr;

  int run_ops(hipStream_t st) const { return run_list(ops, st); }

  // out = act(A[M][K] . W[N][K]^T + bias), A in T:  mode 0 -> T rows; 1 -> fp32 rows; 2 -> fp32 rows += (in-place residual stream)
  void op_linear(Slot* a, size_t a_off, int M, int N, int K, const std::string& pfx, int act, Slot* dst, size_t dst_off, int ldo, int mode) {
    Tuned* t = tuned_linear(a, a_off, M, N, K, pfx, act, dst, dst_off, ldo, mode, s_splitk);
    ops.push_back([=](hipStream_t st) { return t->run(st); });
  }
  // LayerNorm `pfx` of `rows` fp32 rows of x (byte offset x_off, stride ldx): fp32 copy into yf (may be x itself) and / or T copy into yt
  void op_ln(Slot* x, size_t x_off, int64_t ldx, int rows, int D, float eps, const std::string& pfx, Slot* yf, int64_t ldyf, Slot* yt) {
    const float* g = Wf(pfx + ".weight"); const float* b = Wf(pfx + ".bias");
    const int dt = dtype;
    ops.push_back([=](hipStream_t st) {
      const float* xp = reinterpret_cast<const float*>(ptr(x) + x_off);
      return launch_layernorm_rows(xp, ldx, g, b, yf ? ptr<float>(yf) : nullptr, ldyf, yt ? ptr(yt) : nullptr, rows, D, eps, dt, st);
    });
  }
  // softmax(q k^T / 8 + mask) v over `heads` 64-channel heads of the [B * T][Q | K | V] rows of qkv into att [B * T][D]: K and V^T packed for
  // the flash kernel, then the kernel (one entry, two launches).  valid: optional [B][kv_ld] slot, 0 = padding key; keys >= kv_n are valid
  void op_flash_self_attention(Slot* qkv, Slot* att, int B, int heads, int T, int D, int causal, Slot* valid, int kv_ld, int kv_n) {
    const int Tkp = (T + 63) / 64 * 64, dt = dtype;
    need(s_kall, (size_t)B * heads * Tkp * 64 * esz);
    need(s_vtall, (size_t)B * heads * Tkp * 64 * esz);
    ops.push_back([=](hipStream_t st) {
      KvPackParams kp;
      kp.qkv = ptr(qkv); kp.ctxkv = nullptr; kp.kall = ptr(s_kall); kp.vtall = ptr(s_vtall);
      kp.B = B; kp.H = heads; kp.T = T; kp.S = 0; kp.Tkp = Tkp;
      int rc = launch_kv_pack(kp, dt, st);
      if (rc) return rc;
      AttentionParams ap = {};
      ap.q = ptr(qkv); ap.ldq = 3 * D; ap.kall = ptr(s_kall); ap.vtall = ptr(s_vtall); ap.out = ptr(att); ap.ldo = D;
      ap.B = B; ap.H = heads; ap.T = T; ap.Tk = T; ap.Tkp = Tkp; ap.scale = 0.125f;
      ap.causal = causal;
      if (valid) { ap.key_valid = ptr<float>(valid); ap.kv_ld = kv_ld; ap.kv_n = kv_n; }
      return launch_attention(ap, dt, st);
    });
  }
  // out = act(x[M][K] . W[N][K]^T (+ bias)), all fp32, M <= 8 (pooled rows, the time MLP): fp32 rows of x (stride ldx) into fp32 rows at byte
  // offset out_off of `out` (stride ldo)
  void op_linear_small(Slot* x, int64_t ldx, int M, int N, int K, const std::string& pfx, bool has_bias, int act, Slot* out, size_t out_off,
                       int64_t ldo) {
    const void* W = W_(pfx + ".weight");
    const float* bias = has_bias ? Wf(pfx + ".bias") : nullptr;
    ops.push_back([=](hipStream_t st) {
      LinearSmallParams lp = {};
      lp.x = ptr<float>(x); lp.ldx = ldx; lp.W = W; lp.bias = bias; lp.out = reinterpret_cast<float*>(ptr(out) + out_off); lp.ldo = ldo;
      lp.M = M; lp.N = N; lp.K = K; lp.act_in = K22_ACT_NONE; lp.act_out = act;
      return launch_linear_smallm(lp, K22_F32, st);
    });
  }

  // One forward: measure what the tile table does not know (once per plan), then the launch list as this binding's cached graph.
  int forward_list(hipStream_t st) {
    if (int rc = tune_once(s_flush, st)) return rc;
    return replay(graph, st, [this](hipStream_t s) { return run_ops(s); });
  }
  // What forward_list does before its first capture, for a caller that captures the list itself (a whole sampling loop): `stage` puts
  // inputs into the slots, then the measurement and one eager pass of the list.  Nothing once the plan is tuned and warmed.
  template <typename F> int first_use(hipStream_t st, F stage) {
    if (!(autotune && !tuned_done) && warmed) return K22_OK;
    if (int rc = stage(st)) return rc;
    if (int rc = tune_once(s_flush, st)) return rc;
    return warmed ? (int)K22_OK : run_eager(st, [this](hipStream_t s) { return run_ops(s); });
  }
};
