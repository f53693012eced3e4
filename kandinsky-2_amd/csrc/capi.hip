// k22 — C ABI glue: error reporting and the kernel-level entry points declared in include/k22.h.
#include "kernels.h"
#include "elementwise.h"
#include "../../include/k22.h"
#include "tuning.h"
#include "skinny.h"
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

static thread_local char g_err[512] = "";

int k22_set_error(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg ? msg : "");
  return code;
}
int k22_set_error_hip(hipError_t e, const char* file, int line) {
  snprintf(g_err, sizeof(g_err), "HIP error %d (%s) at %s:%d", (int)e, hipGetErrorString(e), file, line);
  return K22_EHIP;
}

extern "C" {

int k22_version(void) { return 100; }
int k22_build_flags(void) {
  int f = 0;
#ifndef K22_NOPK
  f |= K22_BUILD_PACKED_FP32;
#endif
  return f;
}

int k22_set_option(const char* name, int value) {
  if (name && !strcmp(name, "igemm_stages")) { igemm_set_default_stages(value); return K22_OK; }
  if (name && !strcmp(name, "igemm_xcd_remap")) { igemm_set_xcd_remap(value); return K22_OK; }
  if (name && !strcmp(name, "conv_algo")) { igemm_set_conv_algo(value); return K22_OK; }
  if (name && !strcmp(name, "gemm_algo")) { igemm_set_gemm_algo(value); return K22_OK; }
  if (name && !strcmp(name, "att_pipe")) { attention_set_pipe(value); return K22_OK; }
  return k22_set_error(K22_EINVAL, "k22_set_option: unknown option");
}
const char* k22_last_error(void) { return g_err; }

// Test / bench surface of the weight-streaming kernel's fragment-major weights: k22_stream_repack writes the copy, and the pointers
// given to k22_debug_set_stream_frag ride along with every LATER kernel-level test entry of this file (k22_gemm, k22_conv3x3*,
// k22_qkv_project_stream) until they are reset to NULL.  The engines own their copies themselves (engine.hip); nothing in the product
// path reads these globals.
static const void* g_dbg_wfrag = nullptr;
static const void* g_dbg_wsfrag = nullptr;
static void* g_dbg_scratch = nullptr;      // "repack on every call" mode for the parity tests (their helpers pack the weights themselves)
static size_t g_dbg_scratch_bytes = 0;
static int dbg_frag(IgemmParams& p, int dtype, hipStream_t st) {
  p.Wfrag = g_dbg_wfrag; p.Wsfrag = g_dbg_wsfrag;
  if (g_dbg_wfrag || !g_dbg_scratch || dtype == K22_F32 || (p.taps != 1 && p.taps != 9) || p.Kc % 64 || p.Npad % 64) return K22_OK;
  const size_t n1 = stream_frag_bytes(p.Npad, p.taps, p.Kc, dtype);
  const bool skip = p.S0 != nullptr && p.Ws != nullptr && (p.SK0 + p.SK1) % 64 == 0;
  const size_t n2 = skip ? stream_frag_bytes(p.Npad, 1, p.SK0 + p.SK1, dtype) : 0;
  if (n1 + n2 > g_dbg_scratch_bytes) return k22_set_error(K22_ENOMEM, "debug stream scratch too small");
  if (int rc = launch_stream_repack(p.Wp, g_dbg_scratch, p.Npad, p.taps, p.Kc, dtype, st)) return rc;
  p.Wfrag = g_dbg_scratch;
  if (skip) {
    void* w2 = static_cast<char*>(g_dbg_scratch) + n1;
    if (int rc = launch_stream_repack(p.Ws, w2, p.Npad, 1, p.SK0 + p.SK1, dtype, st)) return rc;
    p.Wsfrag = w2;
  }
  return K22_OK;
}
#define K22_DBG_FRAG(p) do { if (int rc_ = dbg_frag((p), dtype, reinterpret_cast<hipStream_t>(stream))) return rc_; } while (0)
int k22_debug_set_stream_frag(const void* wfrag, const void* wsfrag) { g_dbg_wfrag = wfrag; g_dbg_wsfrag = wsfrag; return K22_OK; }
int k22_debug_set_stream_scratch(void* scratch, size_t bytes) { g_dbg_scratch = scratch; g_dbg_scratch_bytes = scratch ? bytes : 0; return K22_OK; }
size_t k22_stream_frag_bytes(int Npad, int taps, int Kc, int dtype) { return stream_frag_bytes(Npad, taps, Kc, dtype); }
int k22_stream_repack(const void* W, void* out, int Npad, int taps, int Kc, int dtype, void* stream) {
  return launch_stream_repack(W, out, Npad, taps, Kc, dtype, reinterpret_cast<hipStream_t>(stream));
}

long k22_debug_counter(const char* name) {
  if (name && !strcmp(name, "stream_launches")) return stream_launch_count();
  if (name && !strcmp(name, "movq_fused_attn_launches")) return movq_fused_attn_launch_count();
  if (name && !strcmp(name, "loop_captures")) return loop_capture_count();
  if (name && !strcmp(name, "loop_launches")) return loop_launch_count();
  return -1;
}

// ---- multi-GPU: the ONE collective of a job -------------------------------------------------------------
// Broadcast of the packed weight arena from `root` over an RCCL communicator the caller owns (one process per GPU; prompts are
// sharded by rank and nothing is exchanged in the step loop).  ncclBroadcast is resolved at call time from the RCCL that is
// already in the process (the one the communicator was created with - PyTorch's, or the host program's), else from
// librccl.so.1: libk22hip.so itself carries no link-time dependency on a second RCCL copy.  Sent in <= 1 GiB pieces: xGMI rings
// are per-link bound, large messages amortise the latency and keep any one call below RCCL's int-count limits.
int k22_comm_broadcast_weights(void* arena, size_t bytes, int root, void* nccl_comm, void* stream) {
  if (!arena || !nccl_comm) return k22_set_error(K22_EINVAL, "k22_comm_broadcast_weights: null arena / communicator");
  typedef int (*bcast_fn)(const void*, void*, size_t, int /*ncclDataType_t*/, int, void*, hipStream_t);
  static bcast_fn fn = nullptr;
  if (!fn) {
    void* sym = dlsym(RTLD_DEFAULT, "ncclBroadcast");
    if (!sym) {
      void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
      if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
      if (h) sym = dlsym(h, "ncclBroadcast");
    }
    if (!sym) return k22_set_error(K22_EINVAL, "k22_comm_broadcast_weights: RCCL (ncclBroadcast) is not loadable in this process");
    fn = reinterpret_cast<bcast_fn>(sym);
  }
  const size_t piece = (size_t)1 << 30;
  char* base = reinterpret_cast<char*>(arena);
  for (size_t off = 0; off < bytes; off += piece) {
    const size_t n = bytes - off < piece ? bytes - off : piece;
    const int rc = fn(base + off, base + off, n, /*ncclUint8*/ 1, root, nccl_comm, reinterpret_cast<hipStream_t>(stream));
    if (rc != 0) { char msg[96]; snprintf(msg, sizeof msg, "k22_comm_broadcast_weights: ncclBroadcast returned %d", rc); return k22_set_error(K22_EHIP, msg); }
  }
  return K22_OK;
}

// ---- tile table (tuning.h) ---------------------------------------------------------------------------------------
int k22_tile_table_load(const char* path) {
  if (!path) return k22_set_error(K22_EINVAL, "k22_tile_table_load: null path");
  const int n = tile_table_load_file(path);
  if (n < 0) return k22_set_error(K22_EINVAL, "k22_tile_table_load: cannot read the file");
  return n;
}
int k22_tile_table_save(const char* path) {
  if (!path) return k22_set_error(K22_EINVAL, "k22_tile_table_save: null path");
  const int n = tile_table_save_file(path);
  if (n < 0) return k22_set_error(K22_EINVAL, "k22_tile_table_save: cannot write the file");
  return n;
}
int k22_tile_table_size(void) {
  TileTable& tt = tile_table();
  std::lock_guard<std::mutex> lk(tt.mu);
  return (int)tt.m.size();
}
int k22_tile_table_measured(void) {
  TileTable& tt = tile_table();
  std::lock_guard<std::mutex> lk(tt.mu);
  return (int)tt.measured;
}
void k22_tile_table_clear(void) {
  TileTable& tt = tile_table();
  std::lock_guard<std::mutex> lk(tt.mu);
  tt.m.clear();
  tt.measured = 0;
}

int k22_gemm(const void* A0, const void* A1, const void* Wp, const float* bias, const void* residual, void* out,
             void* partial, int M, int N, int Npad, int K0, int K1, long lda0, long lda1, int ldo, int ldr,
             int out_f32, int act, int splitk, int bm, int bn, int dtype, void* stream) {
  IgemmParams p = igemm_gemm_problem(M, N, K0, K1, out_f32 ? IG_OUT_ROWMAJOR_F32 : IG_OUT_ROWMAJOR, act);
  p.A0 = A0; p.A1 = A1; p.Wp = Wp; p.bias = bias; p.residual = residual; p.out = out;
  p.partial = reinterpret_cast<float*>(partial);
  p.Npad = Npad; p.lda0 = lda0; p.lda1 = lda1; p.ldo = ldo; p.ldr = ldr;   // the caller's own padding and strides
  p.splitk = splitk; p.force_bm = bm; p.force_bn = bn;
  p.a_raw = k22_is_split(dtype) ? 1 : 0;   // unit entry: A0 / A1 are plain fp32 rows (the engine feeds x3 chunks where its own kernels produce A)
  if (p.splitk == 0) p.splitk = partial ? igemm_choose_splitk(p, dtype) : 1;
  K22_DBG_FRAG(p);
  return launch_igemm(p, dtype, reinterpret_cast<hipStream_t>(stream));
}

int k22_x3_pack(const float* src, void* dst, long n, float scale, void* stream) {
  if (!src || !dst || n < 0) return k22_set_error(K22_EINVAL, "x3_pack: null argument");
  return launch_x3_pack(src, dst, n, scale, reinterpret_cast<hipStream_t>(stream));
}

int k22_conv3x3(const void* x_padded, const void* Wp, const float* bias, const void* residual, void* out,
                void* partial, int B, int H, int W, int Cin, int Cout, int Npad, int out_mode, int act, int splitk,
                int bm, int bn, int dtype, void* stream) {
  IgemmParams p = igemm_conv3_problem(B, H, W, Cin, Cout, out_mode, act);
  p.A0 = x_padded; p.Wp = Wp; p.bias = bias; p.residual = residual; p.out = out;
  p.partial = reinterpret_cast<float*>(partial);
  p.Npad = Npad; p.splitk = splitk; p.force_bm = bm; p.force_bn = bn;
  if (p.splitk == 0) p.splitk = partial ? igemm_choose_splitk(p, dtype) : 1;
  K22_DBG_FRAG(p);
  return launch_igemm(p, dtype, reinterpret_cast<hipStream_t>(stream));
}

int k22_conv3x3_gnstats(const void* x_padded, const void* Wp, const float* bias, const void* residual, void* out,
                        void* partial, int B, int H, int W, int Cin, int Cout, int Npad, int splitk, int bm, int bn,
                        float* stats, int stats_capacity_rows, int* rows_per_image, int dtype, void* stream) {
  IgemmParams p = igemm_conv3_problem(B, H, W, Cin, Cout);
  p.A0 = x_padded; p.Wp = Wp; p.bias = bias; p.residual = residual; p.out = out;
  p.partial = reinterpret_cast<float*>(partial);
  p.Npad = Npad; p.splitk = splitk; p.force_bm = bm; p.force_bn = bn;
  if (p.splitk == 0) p.splitk = partial ? igemm_choose_splitk(p, dtype) : 1;
  const int rpi = igemm_stats_rows_per_image(p, dtype);
  if (rows_per_image) *rows_per_image = rpi;
  if (rpi <= 0) return k22_set_error(K22_EINVAL, "conv3x3_gnstats: this configuration cannot produce GroupNorm partial sums");
  if (rpi * B > stats_capacity_rows) return k22_set_error(K22_ENOMEM, "conv3x3_gnstats: stats buffer too small");
  p.stats = stats;
  K22_DBG_FRAG(p);
  return launch_igemm(p, dtype, reinterpret_cast<hipStream_t>(stream));
}

int k22_conv3x3_up2(const void* x_padded, const void* Wph, const float* bias, void* out, void* partial, int B, int H, int W, int Cin,
                    int Cout, int Npad, int splitk, int bm, float* stats, int stats_capacity_rows, int* rows_per_image, int dtype,
                    void* stream) {
  if (!x_padded || !Wph || !out || B <= 0 || H <= 0 || W <= 0) return k22_set_error(K22_EINVAL, "conv3x3_up2: bad argument");
  IgemmParams p = igemm_up2_problem(B, H, W, Cin, Cout);
  p.A0 = x_padded; p.Wp = Wph; p.bias = bias; p.out = out; p.partial = reinterpret_cast<float*>(partial);
  p.Npad = Npad; p.splitk = splitk; p.force_bm = bm;
  if (p.splitk == 0) p.splitk = partial ? igemm_choose_splitk(p, dtype) : 1;
  if (p.splitk > 1 && !partial) return k22_set_error(K22_EINVAL, "conv3x3_up2: split-K needs the partial buffer");
  if (rows_per_image) *rows_per_image = 0;
  if (stats) {
    const int rpi = igemm_stats_rows_per_image(p, dtype);
    if (rows_per_image) *rows_per_image = rpi;
    if (rpi <= 0) return k22_set_error(K22_EINVAL, "conv3x3_up2: this configuration cannot produce GroupNorm partial sums");
    if (rpi * B > stats_capacity_rows) return k22_set_error(K22_ENOMEM, "conv3x3_up2: stats buffer too small");
    p.stats = stats;
  }
  return launch_igemm(p, dtype, reinterpret_cast<hipStream_t>(stream));
}

int k22_up2_fold(const float* w, float* out, int O, int Opad, int I, void* stream) {
  return launch_up2_fold(w, out, O, Opad, I, reinterpret_cast<hipStream_t>(stream));
}

int k22_gemm_gnstats(const void* A, const void* Wp, const float* bias, const void* residual, void* out, void* partial,
                     int B, int H, int W, int N, int Npad, int K, int splitk, int bm, float* stats,
                     int stats_capacity_rows, int* rows_per_image, int dtype, void* stream) {
  IgemmParams p = igemm_gemm_problem(B * H * W, N, K, 0);
  p.A0 = A; p.Wp = Wp; p.bias = bias; p.residual = residual; p.out = out; p.partial = reinterpret_cast<float*>(partial);
  p.Npad = Npad; p.H = H; p.W = W;   // rows per image
  p.splitk = splitk > 0 ? splitk : 1;
  p.force_bm = bm; p.algo = (bm == 160 || bm == 288) ? IG_ALGO_STREAM : IG_ALGO_GEMM8;
  p.a_raw = k22_is_split(dtype) ? 1 : 0;
  const int rpi = igemm_stats_rows_per_image(p, dtype);
  if (rows_per_image) *rows_per_image = rpi;
  if (rpi <= 0) return k22_set_error(K22_EINVAL, "gemm_gnstats: this configuration cannot produce GroupNorm partial sums");
  if (rpi * B > stats_capacity_rows) return k22_set_error(K22_ENOMEM, "gemm_gnstats: stats buffer too small");
  p.stats = stats;
  K22_DBG_FRAG(p);
  return launch_igemm(p, dtype, reinterpret_cast<hipStream_t>(stream));
}

int k22_conv3x3_skip(const void* x_padded, const void* Wp, const float* bias, const void* skip0, const void* skip1,
                     int SK0, int SK1, const void* Ws, const float* bias_s, void* out, void* partial, int B, int H, int W,
                     int Cin, int Cout, int Npad, int splitk, int bm, int dtype, void* stream) {
  IgemmParams p = igemm_conv3_problem(B, H, W, Cin, Cout);
  p.A0 = x_padded; p.Wp = Wp; p.bias = bias; p.out = out; p.partial = reinterpret_cast<float*>(partial);
  p.Npad = Npad; p.splitk = splitk; p.force_bm = bm;
  p.S0 = skip0; p.S1 = skip1; p.SK0 = SK0; p.SK1 = SK1; p.Ws = Ws; p.bias2 = bias_s;   // (the "conv_algo" option selects among the halo kernels)
  if (p.splitk == 0) p.splitk = partial ? igemm_choose_splitk(p, dtype) : 1;
  K22_DBG_FRAG(p);
  return launch_igemm(p, dtype, reinterpret_cast<hipStream_t>(stream));
}

// ---- one table line, as the engine runs it (tests/test_tile_table_*.py) ---------------------------------------------------------
// The launch descriptor an engine builds for the problem (engine.hip: op_conv / op_gemm; movq.hip, prior.hip, encoder.hip: the same
// fields): device pointers are non-null MARKERS, as there, because the candidate list only asks whether an operand exists.
static int igemm_problem_tuned(const K22IgemmProblem& d, Tuned& t) {
  if (d.dtype < K22_BF16 || d.dtype > K22_F16X2) return k22_set_error(K22_EINVAL, "igemm_cfg: bad dtype");
  if ((d.taps != 1 && d.taps != 9) || d.M <= 0 || d.N <= 0 || d.Kc <= 0 || d.K0 <= 0 || d.K0 > d.Kc)
    return k22_set_error(K22_EINVAL, "igemm_cfg: bad problem (taps 1 / 9, M, N > 0, 0 < K0 <= Kc)");
  if (d.out_mode < IG_OUT_ROWMAJOR || d.out_mode > IG_OUT_QKV || d.SK0 < 0 || d.SK1 < 0 || (d.SK1 > 0 && d.SK0 == 0))
    return k22_set_error(K22_EINVAL, "igemm_cfg: bad output mode / skip widths");
  if (d.taps == 9 && (d.H <= 0 || d.W <= 0 || d.M % (d.H * d.W))) return k22_set_error(K22_EINVAL, "igemm_cfg: a convolution needs M = B * H * W");
  const void* mark = reinterpret_cast<const void*>(1);
  IgemmParams& p = t.p;
  if (d.taps == 9) {
    p = igemm_conv3_problem(d.M / (d.H * d.W), d.H, d.W, d.Kc, d.N, d.out_mode, d.act);
    p.K0 = d.K0;   // as the line spells it
  } else {
    p = igemm_gemm_problem(d.M, d.N, d.K0, d.Kc - d.K0, d.out_mode, d.act);
    p.H = d.H; p.W = d.W;   // rows per image
  }
  p.ldo = d.ldo > 0 ? d.ldo : (d.out_mode == IG_OUT_QKV ? d.N / 3 : d.N);
  p.ldr = d.ldr > 0 ? d.ldr : (d.res_f32 ? p.ldo : d.N);
  p.res_f32 = d.res_f32 ? 1 : 0; p.a_raw = d.a_raw ? 1 : 0;
  p.Wp = mark; p.bias = reinterpret_cast<const float*>(mark);
  if (d.SK0 > 0) { p.S0 = mark; p.S1 = d.SK1 > 0 ? mark : nullptr; p.SK0 = d.SK0; p.SK1 = d.SK1; p.Ws = mark; p.bias2 = reinterpret_cast<const float*>(mark); }
  if (d.out_mode == IG_OUT_QKV) { p.att_T = d.att_T; p.att_S = d.att_S; p.att_Tkp = d.att_Tkp; }
  if (d.has_frag) { p.Wfrag = mark; if (d.SK0 > 0) p.Wsfrag = mark; }
  t.want_stats = d.want_stats != 0;
  t.dt = d.dtype;
  tuned_make_candidates(t, d.dtype);
  return K22_OK;
}
static Cfg igemm_problem_cfg(const K22IgemmProblem& d) {
  Cfg c; c.algo = d.algo; c.bm = d.bm; c.bn = d.bn; c.splitk = d.splitk; c.stages = d.stages;
  return c;
}

static bool igemm_cfg_is_fixed_choice(const Cfg& c) { return !c.algo && !c.bm && !c.bn && !c.splitk && !c.stages; }
// The all-zero configuration: what tuned_default_cfg leaves in t.cfg (K22_AUTOTUNE=0, and every M < 64).  False when the problem owes
// GroupNorm partial sums and the fixed choice cannot deliver them (an engine then runs the stand-alone gn_stats kernel), or when no kernel
// takes the problem at all (igemm_resolve refuses it: a fused skip on an image no halo kernel supports).  L: the launch it resolves to.
static bool igemm_fixed_choice(const K22IgemmProblem& d, Tuned& t, IgemmLaunch* L = nullptr) {
  tuned_default_cfg(t, d.dtype);
  IgemmParams q = t.p;
  tuned_apply_cfg(q, t.cfg);
  IgemmLaunch tmp;
  if (igemm_resolve(q, d.dtype, L ? L : &tmp) != K22_OK) return false;
  return !d.want_stats || (t.want_stats && t.rpi > 0);
}

int k22_igemm_cfg_accepted(const K22IgemmProblem* pr) {
  if (!pr) return k22_set_error(K22_EINVAL, "igemm_cfg_accepted: null problem");
  Tuned t;
  if (int rc = igemm_problem_tuned(*pr, t)) return rc;
  if (igemm_cfg_is_fixed_choice(igemm_problem_cfg(*pr))) return igemm_fixed_choice(*pr, t) ? 1 : 0;
  return tuned_is_candidate(t, igemm_problem_cfg(*pr)) ? 1 : 0;
}

int k22_igemm_candidates(const K22IgemmProblem* pr, K22IgemmCfg* out, int capacity, K22IgemmCfg* resolved, K22IgemmCfg* fixed) {
  if (!pr || capacity < 0 || (capacity > 0 && !out)) return k22_set_error(K22_EINVAL, "igemm_candidates: null problem / array");
  Tuned t;
  if (int rc = igemm_problem_tuned(*pr, t)) return rc;
  auto resolve = [&](const Cfg& c, K22IgemmCfg* r) {
    IgemmParams q = t.p;
    tuned_apply_cfg(q, c);
    IgemmLaunch L;
    if (int rc = igemm_resolve(q, pr->dtype, &L)) return rc;
    r->algo = L.algo; r->bm = L.bm; r->bn = L.bn; r->splitk = L.splitk; r->stages = L.depth;
    return (int)K22_OK;
  };
  const int n = (int)t.cands.size();
  for (int i = 0; i < n && i < capacity; ++i) {
    const Cfg& c = t.cands[i];
    out[i].algo = c.algo; out[i].bm = c.bm; out[i].bn = c.bn; out[i].splitk = c.splitk; out[i].stages = c.stages;
    if (resolved) if (int rc = resolve(c, &resolved[i])) return rc;
  }
  if (fixed) {
    IgemmLaunch L = {};
    if (!igemm_fixed_choice(*pr, t, &L)) L = IgemmLaunch{};   // all zero: k22_igemm_cfg_accepted says 0 for it
    fixed->algo = L.algo; fixed->bm = L.bm; fixed->bn = L.bn; fixed->splitk = L.splitk; fixed->stages = L.depth;
  }
  return n;
}

int k22_igemm_cfg(const K22IgemmProblem* pr, const K22IgemmOperands* ops, int* rows_per_image, void* stream) {
  if (rows_per_image) *rows_per_image = 0;
  if (!pr || !ops) return k22_set_error(K22_EINVAL, "igemm_cfg: null problem / operands");
  const K22IgemmProblem& d = *pr;
  const K22IgemmOperands& o = *ops;
  Tuned t;
  if (int rc = igemm_problem_tuned(d, t)) return rc;
  Cfg c = igemm_problem_cfg(d);
  if (igemm_cfg_is_fixed_choice(c)) {
    if (!igemm_fixed_choice(d, t)) return k22_set_error(K22_EINVAL, "igemm_cfg: the fixed choice cannot run this problem (no kernel takes it, or none writes the GroupNorm partial sums it owes)");
    c = t.cfg;
    if (!o.partial) return k22_set_error(K22_EINVAL, "igemm_cfg: the fixed choice needs the fp32 partial buffer (k22_igemm_candidates reports its split)");
  } else if (!tuned_is_candidate(t, c)) return k22_set_error(K22_EINVAL, "igemm_cfg: this build does not generate the configuration for the problem");
  if (!o.A0 || !o.Wp || !o.out) return k22_set_error(K22_EINVAL, "igemm_cfg: A0, Wp and out are required");
  if (d.K0 < d.Kc && !o.A1) return k22_set_error(K22_EINVAL, "igemm_cfg: A1 missing for the concat operand");
  if (d.SK0 > 0 && (!o.S0 || !o.Ws || (d.SK1 > 0 && !o.S1))) return k22_set_error(K22_EINVAL, "igemm_cfg: fused-skip operands missing");
  if (d.out_mode == IG_OUT_QKV && (!o.kall || !o.vtall)) return k22_set_error(K22_EINVAL, "igemm_cfg: kall / vtall missing");
  if ((c.splitk > 1 || c.algo == IG_ALGO_STREAM) && !o.partial) return k22_set_error(K22_EINVAL, "igemm_cfg: the configuration needs the fp32 partial buffer");
  if (c.algo == IG_ALGO_STREAM && (!o.Wfrag || (d.SK0 > 0 && !o.Wsfrag))) return k22_set_error(K22_EINVAL, "igemm_cfg: algo 20 needs the fragment-major weights");
  IgemmParams q = t.p;
  tuned_apply_cfg(q, c);
  q.A0 = o.A0; q.A1 = o.A1; q.Wp = o.Wp; q.bias = reinterpret_cast<const float*>(o.bias); q.residual = o.residual; q.out = o.out;
  q.partial = reinterpret_cast<float*>(o.partial);
  q.S0 = d.SK0 > 0 ? o.S0 : nullptr; q.S1 = d.SK1 > 0 ? o.S1 : nullptr; q.Ws = d.SK0 > 0 ? o.Ws : nullptr;
  q.bias2 = d.SK0 > 0 ? reinterpret_cast<const float*>(o.bias2) : nullptr;
  q.kall = o.kall; q.vtall = o.vtall;
  q.Wfrag = c.algo == IG_ALGO_STREAM ? o.Wfrag : nullptr; q.Wsfrag = (c.algo == IG_ALGO_STREAM && d.SK0 > 0) ? o.Wsfrag : nullptr;
  if (t.want_stats) {
    const int rpi = igemm_stats_rows_per_image(q, d.dtype);
    const int B = d.H > 0 ? d.M / (d.H * d.W) : 1;
    if (rpi <= 0) return k22_set_error(K22_EINVAL, "igemm_cfg: this configuration cannot produce GroupNorm partial sums");
    if (!o.stats || (long)rpi * B > o.stats_capacity_rows) return k22_set_error(K22_ENOMEM, "igemm_cfg: stats buffer missing / too small");
    if (rows_per_image) *rows_per_image = rpi;
    q.stats = o.stats;
  }
  return launch_igemm(q, d.dtype, reinterpret_cast<hipStream_t>(stream));
}

size_t k22_groupnorm_scratch_bytes(int B, int C) {
  return (size_t)B * 128 * C * 2 * sizeof(float) + (size_t)B * C * 2 * sizeof(float) + 512;
}

int k22_groupnorm(const void* x0, const void* x1, int C0, int C1, int B, int H, int W, const float* gamma,
                  const float* beta, const float* film, long film_ld, float eps, int act, int mode, int pad,
                  void* scratch, void* out, int dtype, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int C = C0 + C1, HW = H * W;
  const int out_x3 = k22_is_split(dtype) ? 1 : 0;   // split-precision engine: fp32 in, x3 chunks out (what its convolutions read)
  dtype = k22_storage_dtype(dtype);
  float* partial = reinterpret_cast<float*>(scratch);
  float* coeff = partial + (size_t)B * 128 * C * 2;
  const int rc = launch_gn_stats_coeff(x0, x1, C0, C1, B, HW, eps, gamma, beta, film, film_ld, partial, coeff, dtype, st);
  if (rc) return rc;
  GnApplyParams ap = {};
  ap.x0 = x0; ap.x1 = x1; ap.C0 = C0; ap.C1 = C1; ap.B = B; ap.H = H; ap.W = W; ap.mode = mode; ap.pad = pad; ap.act = act;
  ap.coeff = coeff; ap.out = out; ap.out_x3 = out_x3;
  return launch_gn_apply(ap, dtype, st);
}

// kv_pack, then attention, with the mask and output-format fields of AttentionParams the engines set
static int attention_seq(const void* qkv, const void* ctxkv, void* kall, void* vtall, void* out, int B, int H, int T, int S, int causal,
                         const float* key_valid, int kv_n, int out_x3, int dtype, hipStream_t st) {
  const int C = H * 64, Tk = S + T, Tkp = (Tk + 63) / 64 * 64;
  KvPackParams kp;
  kp.qkv = qkv; kp.ctxkv = ctxkv; kp.kall = kall; kp.vtall = vtall; kp.B = B; kp.H = H; kp.T = T; kp.S = S; kp.Tkp = Tkp;
  int rc = launch_kv_pack(kp, k22_storage_dtype(dtype), st);
  if (rc) return rc;
  AttentionParams ap = {};
  ap.q = qkv; ap.ldq = 3 * C; ap.kall = kall; ap.vtall = vtall; ap.out = out; ap.ldo = C;
  ap.B = B; ap.H = H; ap.T = T; ap.Tk = Tk; ap.Tkp = Tkp; ap.scale = 0.125f;
  ap.causal = causal ? 1 : 0; ap.key_valid = key_valid; ap.kv_ld = kv_n; ap.kv_n = kv_n; ap.out_x3 = out_x3 ? 1 : 0;
  return launch_attention(ap, dtype, st);
}

int k22_attention(const void* qkv, const void* ctxkv, void* kall, void* vtall, void* out, int B, int H, int T, int S,
                  int dtype, void* stream) {
  return attention_seq(qkv, ctxkv, kall, vtall, out, B, H, T, S, 0, nullptr, 0, 0, dtype, reinterpret_cast<hipStream_t>(stream));
}

// the qkv projection of an AttentionBlock: x [B * T][K] -> q rows, K / V^T behind the S context keys of the attention operands
static IgemmParams qkv_problem(const void* x, const void* Wp, const float* bias, void* q_out, void* kall, void* vtall, int B, int H, int T, int S, int K) {
  const int C = H * 64;
  IgemmParams p = igemm_gemm_problem(B * T, 3 * C, K, 0, IG_OUT_QKV);
  p.A0 = x; p.Wp = Wp; p.bias = bias; p.out = q_out; p.kall = kall; p.vtall = vtall;
  p.ldo = C;
  p.att_T = T; p.att_S = S; p.att_Tkp = (S + T + 63) / 64 * 64; p.H = 1; p.W = T;   // rows per image
  return p;
}

int k22_qkv_project(const void* x, const void* Wp, const float* bias, void* q_out, void* kall, void* vtall,
                    int B, int H, int T, int S, int K, int bm, int bn, int dtype, void* stream) {
  IgemmParams p = qkv_problem(x, Wp, bias, q_out, kall, vtall, B, H, T, S, K);
  p.splitk = 1; p.force_bm = bm; p.force_bn = bn;
  p.a_raw = k22_is_split(dtype) ? 1 : 0;
  K22_DBG_FRAG(p);
  return launch_igemm(p, dtype, reinterpret_cast<hipStream_t>(stream));
}

int k22_qkv_project_stream(const void* x, const void* Wp, const float* bias, void* q_out, void* kall, void* vtall, void* partial,
                           int B, int H, int T, int S, int K, int bm, int splitk, int dtype, void* stream) {
  IgemmParams p = qkv_problem(x, Wp, bias, q_out, kall, vtall, B, H, T, S, K);
  p.partial = reinterpret_cast<float*>(partial);
  p.splitk = splitk > 0 ? splitk : 1; p.force_bm = bm; p.algo = IG_ALGO_STREAM;
  if (!stream_supported(p, dtype, bm == 288 ? 9 : 5)) return k22_set_error(K22_EINVAL, "qkv_project_stream: unsupported problem");
  K22_DBG_FRAG(p);
  return launch_igemm(p, dtype, reinterpret_cast<hipStream_t>(stream));
}

// ---- skinny-M weight-streaming GEMM family (skinny.hip, small_attention_kernel): unit-parity surface -------------------------------
size_t k22_afrag_bytes(int M, int K) { return afrag_bytes(M, K); }
int k22_afrag_pack(const void* A, long lda, void* out, int M, int K, int dtype, void* stream) {
  return launch_afrag_pack(A, lda, out, M, K, dtype, reinterpret_cast<hipStream_t>(stream));
}
int k22_skinny_gemm(const void* Afrag, const void* Wfrag, const float* bias, void* out, float* partial, int M, int N, int Npad, int K,
                    int splitk, int epi, int act, int ldo, int mt, int nb, int dtype, void* stream) {
  SkinnyParams q = {};
  q.Af = Afrag; q.Wf = Wfrag; q.bias = bias; q.out = out; q.partial = partial; q.M = M; q.N = N; q.Npad = Npad; q.K = K; q.MA = (M + 31) / 32;
  q.splitk = splitk > 0 ? splitk : 1; q.epi = epi; q.act = act; q.ldo = ldo;
  return launch_skinny(q, dtype, mt, nb, reinterpret_cast<hipStream_t>(stream));
}
int k22_finish_ln(const float* partial, int splitk, const float* bias, float* x, long ldx, const float* gain, const float* beta, void* yfrag,
                  int M, int N, float eps, int dtype, void* stream) {
  FinishLnParams q = {};
  q.partial = partial; q.splitk = splitk; q.bias = bias; q.x = x; q.ldx = ldx; q.g = gain; q.b = beta; q.yfrag = yfrag; q.M = M; q.N = N;
  q.MA = (M + 31) / 32; q.eps = eps;
  return launch_finish_ln(q, dtype, reinterpret_cast<hipStream_t>(stream));
}
int k22_small_attention(const void* qkv, const float* qkv_partial, int nsplit, const float* qkv_bias, void* out, int out_frag, int B, int H, int T,
                        int causal, const float* key_valid, int kv_n, int dtype, void* stream) {
  SmallAttnParams ap = {};
  ap.qkv = qkv; ap.part = qkv_partial; ap.nsplit = nsplit; ap.bias = qkv_bias; ap.ldq = 3 * H * 64; ap.out = out; ap.ldo = H * 64; ap.out_frag = out_frag; ap.MA = (B * T + 31) / 32;
  ap.B = B; ap.H = H; ap.T = T; ap.scale = 0.125f; ap.causal = causal; ap.key_valid = key_valid; ap.kv_ld = kv_n; ap.kv_n = kv_n;
  return launch_small_attention(ap, dtype, reinterpret_cast<hipStream_t>(stream));
}

int k22_linear_smallm(const float* x, const void* W, const float* bias, const float* add, float* out, int M, int N,
                      int K, int act_in, int act_out, int wdtype, void* stream) {
  LinearSmallParams lp = {};
  lp.x = x; lp.ldx = K; lp.W = W; lp.bias = bias; lp.add = add; lp.ld_add = N; lp.out = out; lp.ldo = N;
  lp.M = M; lp.N = N; lp.K = K; lp.act_in = act_in; lp.act_out = act_out;
  return launch_linear_smallm(lp, wdtype, reinterpret_cast<hipStream_t>(stream));
}

int k22_conv3x3_direct(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout, int Hin, int Win,
                       int stride, int act, void* stream) {
  if (!x || !w || !bias || !y) return k22_set_error(K22_EINVAL, "conv3x3_direct: null argument");
  if (B < 1 || Cin < 1 || Cout < 1 || Hin < 1 || Win < 1) return k22_set_error(K22_EINVAL, "conv3x3_direct: empty shape");
  if (act != K22_ACT_NONE && act != K22_ACT_SILU) return k22_set_error(K22_EINVAL, "conv3x3_direct: act must be 0 (none) or 1 (SiLU)");
  ConvDirectParams p = {};
  p.x = x; p.w = w; p.bias = bias; p.y = y;
  p.B = B; p.Cin = Cin; p.Cout = Cout; p.Hin = Hin; p.Win = Win; p.stride = stride; p.act = act;
  return launch_conv3x3_direct(p, reinterpret_cast<hipStream_t>(stream));
}

int k22_ddim_step(const float* x, const float* model_out, const float* noise, const float* table_row, float guidance, int use_cfg,
                  float* x_out, float* x0_out, int N, int HW, void* stream) {
  if (!x || !model_out || !table_row || !x_out) return k22_set_error(K22_EINVAL, "ddim_step: null argument");
  return launch_ddim_step(x, model_out, noise, table_row, guidance, use_cfg, x_out, x0_out, N, HW, reinterpret_cast<hipStream_t>(stream));
}

int k22_dpmpp_step(const float* x, const float* model_out, const float* x0_prev, const float* table_row, float guidance, int use_cfg,
                   float* x_out, float* x0_out, int N, int HW, void* stream) {
  return launch_dpmpp_step(x, model_out, x0_prev, table_row, guidance, use_cfg, x_out, x0_out, N, HW, reinterpret_cast<hipStream_t>(stream));
}

int k22_dpmpp_step_clip(const float* x, const float* model_out, const float* x0_prev, const float* table_row, float guidance, int use_cfg,
                        float clamp_lo, float clamp_hi, float* x_out, float* x0_out, int N, int HW, void* stream) {
  return launch_dpmpp_step_clip(x, model_out, x0_prev, table_row, guidance, use_cfg, clamp_lo, clamp_hi, x_out, x0_out, N, HW,
                                reinterpret_cast<hipStream_t>(stream));
}

int k22_prepare_mask(const float* mask, float* out, int C, int H, int W, void* stream) {
  if (!mask || !out) return k22_set_error(K22_EINVAL, "prepare_mask: null argument");
  return launch_prepare_mask(mask, out, C, H, W, reinterpret_cast<hipStream_t>(stream));
}

int k22_plms_step(const float* x, const float* model_out, const float* eps_hist1, const float* eps_hist2, const float* eps_hist3, int order,
                  const float* table_row, float guidance, int use_cfg, float* x_out, float* eps_out, float* x0_out, int N, int HW, void* stream) {
  if (!x || !model_out || !table_row || !x_out) return k22_set_error(K22_EINVAL, "plms_step: null argument");
  return launch_plms_step(x, model_out, eps_hist1, eps_hist2, eps_hist3, order, table_row, guidance, use_cfg, x_out, eps_out, x0_out, N, HW,
                          reinterpret_cast<hipStream_t>(stream));
}

size_t k22_sampler_scratch_bytes(int N, int HW) { return (size_t)N * 4 * HW * sizeof(float) + 256; }

// pct_group 0: k22_sampler_step - one threshold group, the whole cond half (launch_sampler_step)
static int sampler_step_groups(const float* x, const float* model_out, const float* noise, const float* init_img, const float* mask,
                               const float* table, int step_index, float guidance, int use_cfg, float clamp_lo, float clamp_hi, int pct_index,
                               double pct_gamma, int pct_group, void* scratch, float* x_out, float* x0_out, int N, int HW, void* stream) {
  SamplerParams p = {};
  p.pct_group = pct_group;
  p.x = x; p.model_out = model_out; p.noise = noise; p.init_img = init_img; p.mask = mask; p.table = table;
  p.step = nullptr; p.step_host = step_index; p.guidance = guidance; p.clamp_lo = clamp_lo; p.clamp_hi = clamp_hi;
  p.use_cfg = use_cfg; p.n_lo = pct_index; p.gamma = pct_gamma;
  p.s_buf = reinterpret_cast<float*>(scratch);
  p.x0_buf = reinterpret_cast<float*>(scratch) + 64;
  p.x_out = x_out; p.x0_out = x0_out; p.N = N; p.HW = HW;
  if (pct_index >= 4 * HW) return k22_set_error(K22_EINVAL, "sampler: percentile index out of range");
  return launch_sampler_step(p, reinterpret_cast<hipStream_t>(stream));
}

int k22_sampler_step(const float* x, const float* model_out, const float* noise, const float* init_img,
                     const float* mask, const float* table, int step_index, float guidance, int use_cfg,
                     float clamp_lo, float clamp_hi, int pct_index, double pct_gamma, void* scratch,
                     float* x_out, float* x0_out, int N, int HW, void* stream) {
  return sampler_step_groups(x, model_out, noise, init_img, mask, table, step_index, guidance, use_cfg, clamp_lo, clamp_hi, pct_index, pct_gamma, 0,
                             scratch, x_out, x0_out, N, HW, stream);
}

int k22_sampler_step_groups(const float* x, const float* model_out, const float* noise, const float* init_img, const float* mask,
                            const float* table, int step_index, float guidance, int use_cfg, float clamp_lo, float clamp_hi, int pct_index,
                            double pct_gamma, int pct_group, void* scratch, float* x_out, float* x0_out, int N, int HW, void* stream) {
  if (pct_group < 1) return k22_set_error(K22_EINVAL, "sampler_step_groups: pct_group must be >= 1");
  return sampler_step_groups(x, model_out, noise, init_img, mask, table, step_index, guidance, use_cfg, clamp_lo, clamp_hi, pct_index, pct_gamma,
                             pct_group, scratch, x_out, x0_out, N, HW, stream);
}

// ---- single-kernel entry points of the MoVQ helpers for the parity tests (include/k22.h); no product code calls them ---------------
static bool aux_dtype_ok(int dt) { return dt == K22_BF16 || dt == K22_F16 || dt == K22_F32; }

int k22_spatialnorm_apply(const void* x, const float* coeff, const float* zq, const float* wy, const float* by, const float* wb, const float* bb,
                          void* out, int B, int H, int W, int C, int h0, int w0, int shift, int act, int pad, int dtype, void* stream) {
  if (!x || !coeff || !zq || !wy || !by || !wb || !bb || !out || B < 1 || H < 1 || W < 1 || C < 1 || h0 < 1 || w0 < 1 || shift < 0 || shift > 12 || (H & ((1 << shift) - 1)) ||
      (pad != 0 && pad != 1) || (act != K22_ACT_NONE && act != K22_ACT_SILU) || !aux_dtype_ok(dtype))
    return k22_set_error(K22_EINVAL, "spatialnorm_apply: bad argument");
  SpatialNormParams p = {};
  p.x = x; p.coeff = coeff; p.zq = zq; p.wy = wy; p.by = by; p.wb = wb; p.bb = bb; p.out = out;
  p.B = B; p.H = H; p.W = W; p.C = C; p.h0 = h0; p.w0 = w0; p.shift = shift; p.act = act; p.pad = pad;
  return launch_spatialnorm_apply(p, dtype, reinterpret_cast<hipStream_t>(stream));
}
#define K22_AUX_NHWC(NAME_)                                                                                                     \
  int k22_##NAME_(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream) {                                \
    if (!x || !y || B < 1 || B > 65535 || H < 1 || W < 1 || C < 1 || !aux_dtype_ok(dtype)) return k22_set_error(K22_EINVAL, #NAME_ ": bad argument"); \
    return launch_##NAME_(x, y, B, H, W, C, dtype, reinterpret_cast<hipStream_t>(stream));                                      \
  }
K22_AUX_NHWC(upsample2_pad)
K22_AUX_NHWC(pad_copy)
K22_AUX_NHWC(subsample_odd)
#undef K22_AUX_NHWC
int k22_softmax_rows(void* x, long rows, int L, float scale, int dtype, void* stream) {
  if (!x || L < 1 || !aux_dtype_ok(dtype)) return k22_set_error(K22_EINVAL, "softmax_rows: bad argument");
  return launch_softmax_rows(x, rows, L, scale, dtype, reinterpret_cast<hipStream_t>(stream));
}
int k22_movq_attention(const void* q, const void* k, const void* vt, const float* bias_v, void* out, int B, int T, int C, int dtype, void* stream) {
  return launch_movq_attention(q, k, vt, bias_v, out, B, T, C, dtype, reinterpret_cast<hipStream_t>(stream));
}
int k22_movq_prepare(const float* z, const float* wpq, const float* bpq, float* zq, void* xin, int B, int h, int w, int Cpad, int dtype, void* stream) {
  if (!z || !wpq || !bpq || !zq || !xin || B < 1 || h < 1 || w < 1 || Cpad < 4 || !aux_dtype_ok(dtype)) return k22_set_error(K22_EINVAL, "movq_prepare: bad argument");
  return launch_movq_prepare(z, wpq, bpq, zq, xin, B, h, w, Cpad, dtype, reinterpret_cast<hipStream_t>(stream));
}
int k22_movq_enc_prepare(const float* image, void* xin, int B, int H, int W, int Cpad, int dtype, void* stream) {
  if (!image || !xin || B < 1 || H < 1 || W < 1 || Cpad < 3 || !aux_dtype_ok(dtype)) return k22_set_error(K22_EINVAL, "movq_enc_prepare: bad argument");
  return launch_movq_enc_prepare(image, xin, B, H, W, Cpad, dtype, reinterpret_cast<hipStream_t>(stream));
}
int k22_movq_quant_conv(const float* h, const float* wq, const float* bq, float* out, int B, int HW, void* stream) {
  if (!h || !wq || !bq || !out || B < 1 || HW < 1) return k22_set_error(K22_EINVAL, "movq_quant_conv: bad argument");
  return launch_movq_quant_conv(h, wq, bq, out, B, HW, reinterpret_cast<hipStream_t>(stream));
}
int k22_to_uint8_nhwc(const float* x, unsigned char* y, int B, int C, int H, int W, void* stream) {
  if (!x || !y || B < 1 || C < 1 || H < 1 || W < 1) return k22_set_error(K22_EINVAL, "to_uint8_nhwc: bad argument");
  return launch_to_uint8_nhwc(x, y, B, C, H, W, reinterpret_cast<hipStream_t>(stream));
}
int k22_attention_masked(const void* qkv, const void* ctxkv, void* kall, void* vtall, void* out, int B, int H, int T, int S, int causal,
                         const float* key_valid, int kv_n, int out_x3, int dtype, void* stream) {
  if (!qkv || !kall || !vtall || !out || B < 1 || H < 1 || T < 1 || S < 0 || kv_n < 0 || (S > 0 && !ctxkv) || !(aux_dtype_ok(dtype) || k22_is_split(dtype)))
    return k22_set_error(K22_EINVAL, "attention_masked: bad argument");
  if (causal && S != 0) return k22_set_error(K22_EINVAL, "attention_masked: causal needs S == 0 (key index against query index)");
  if (kv_n > S + T) return k22_set_error(K22_EINVAL, "attention_masked: kv_n > S + T");
  if (out_x3 && !k22_is_split(dtype)) return k22_set_error(K22_EINVAL, "attention_masked: out_x3 needs a split dtype");
  return attention_seq(qkv, ctxkv, kall, vtall, out, B, H, T, S, causal, key_valid, kv_n, out_x3, dtype, reinterpret_cast<hipStream_t>(stream));
}

// ---- GroupNorm32, one kernel per entry (tests/test_gn_parity_gpu.py): the three launchers K22UNet::op_gn calls, with the fields it fills ----
int k22_gn_stats(const void* x0, const void* x1, int C0, int C1, int B, int HW, float* partial, int* nsplit_out, int dtype, void* stream) {
  if (nsplit_out) *nsplit_out = 0;
  if (!x0 || !partial || C0 < 1 || C1 < 0 || (C1 > 0 && !x1) || B < 1 || B > 65535 || HW < 1 || !(aux_dtype_ok(dtype) || k22_is_split(dtype)))
    return k22_set_error(K22_EINVAL, "gn_stats: bad argument");
  GnStatsParams sp = {};
  sp.x0 = x0; sp.x1 = C1 > 0 ? x1 : nullptr; sp.C0 = C0; sp.C1 = C1; sp.HW = HW; sp.B = B; sp.groups = 32; sp.nsplit = gn_nsplit(B, HW); sp.partial = partial;
  if (nsplit_out) *nsplit_out = sp.nsplit;
  return launch_gn_stats(sp, k22_storage_dtype(dtype), reinterpret_cast<hipStream_t>(stream));
}
int k22_gn_coeff(const float* st0, int rpi0, int C0, const float* st1, int rpi1, int C1, int B, int HW, const float* gamma, const float* beta,
                 const float* film, long film_ld, float eps, float* coeff, void* stream) {
  // (the engine's plan cannot trip any of these: its channel counts are multiples of 128, op_gn refuses rpi <= 0 itself and film_ld is the
  // whole FiLM row - so they live here and launch_gn_coeff stays as it is)
  if (!gamma || !beta || !coeff) return k22_set_error(K22_EINVAL, "gn_coeff: gamma, beta and coeff are required");
  if (!st0 || C0 < 1 || C1 < 0 || B < 1 || B > 65535 || HW < 1) return k22_set_error(K22_EINVAL, "gn_coeff: bad argument");
  if (rpi0 <= 0 || (C1 > 0 && rpi1 <= 0)) return k22_set_error(K22_EINVAL, "gn_coeff: rows per image of a used source must be positive");
  if (C1 > 0 && !st1) return k22_set_error(K22_EINVAL, "gn_coeff: second source without partial sums");
  const int C = C0 + C1;
  if (C % 32 != 0) return k22_set_error(K22_EINVAL, "gn_coeff: 32 groups need C % 32 == 0");
  if (film && film_ld < 2L * C) return k22_set_error(K22_EINVAL, "gn_coeff: film_ld < 2 C");
  GnCoeffParams cp = {};
  cp.src[0].st = st0; cp.src[0].rpi = rpi0; cp.src[0].C = C0;
  if (C1 > 0) { cp.src[1].st = st1; cp.src[1].rpi = rpi1; cp.src[1].C = C1; }
  cp.HW = HW; cp.C = C; cp.groups = 32; cp.eps = eps; cp.gamma = gamma; cp.beta = beta; cp.film = film; cp.film_ld = film_ld; cp.coeff = coeff;
  return launch_gn_coeff(cp, B, reinterpret_cast<hipStream_t>(stream));
}
int k22_gn_apply(const void* x0, const void* x1, int C0, int C1, int B, int H, int W, const float* coeff, int act, int mode, int pad, void* out,
                 int dtype, void* stream) {
  if (!x0 || !coeff || !out || C0 < 1 || C1 < 0 || (C1 > 0 && !x1) || B < 1 || H < 1 || W < 1 || mode < 0 || mode > 2 || (mode == 1 && (H < 2 || W < 2)) ||
      (pad != 0 && pad != 1) || (act != K22_ACT_NONE && act != K22_ACT_SILU) || !(aux_dtype_ok(dtype) || k22_is_split(dtype)))
    return k22_set_error(K22_EINVAL, "gn_apply: bad argument");
  GnApplyParams ap = {};
  ap.x0 = x0; ap.x1 = C1 > 0 ? x1 : nullptr; ap.C0 = C0; ap.C1 = C1; ap.B = B; ap.H = H; ap.W = W; ap.mode = mode; ap.pad = pad; ap.act = act;
  ap.coeff = coeff; ap.out = out; ap.out_x3 = k22_is_split(dtype) ? 1 : 0;   // as k22_groupnorm: fp32 in, x3 chunks out
  return launch_gn_apply(ap, k22_storage_dtype(dtype), reinterpret_cast<hipStream_t>(stream));
}

// ---- the kernels that open and close a UNet step, one per entry (tests/test_seam_kernels_gpu.py): the launchers K22UNet's plan, its
// conditioning heads and the sampler loops call, with the fields they fill.  What protects a kernel is refused in its launcher ----------
int k22_conv_in(const float* x, const float* img, const float* mask, const float* w_packed, const float* bias, void* out, int B, int H, int W,
                int Cin, int Cout, int img_premul, int dtype, void* stream) {
  if (!x || !w_packed || !bias || !out || B < 1 || B > 65535 || H < 1 || H > 65535 || W < 1 || Cout < 1 || !aux_dtype_ok(dtype))
    return k22_set_error(K22_EINVAL, "conv_in: bad argument");
  ConvInParams p = {};
  p.x = x; p.img = img; p.mask = mask; p.w = w_packed; p.bias = bias; p.out = out;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.img_premul = img_premul ? 1 : 0;
  return launch_conv_in(p, dtype, reinterpret_cast<hipStream_t>(stream));
}
int k22_timestep_embedding(const float* t, const float* freqs, float* out, int rows, int half, void* stream) {
  if (!t || !freqs || !out || rows < 1 || half < 1) return k22_set_error(K22_EINVAL, "timestep_embedding: bad argument");
  return launch_timestep_embedding(t, freqs, out, rows, half, reinterpret_cast<hipStream_t>(stream));
}
int k22_linear_smallm_ld(const float* x, long ldx, const void* W, const float* bias, const float* add, long ld_add, int add_mod, float* out,
                         long ldo, int M, int N, int K, int act_in, int act_out, int wdtype, void* stream) {
  if (!x || !W || !out || N < 1 || K < 1 || ldx < K || ldo < N || (add && ld_add < N) || add_mod < 0 || !aux_dtype_ok(wdtype) ||
      (act_in != K22_ACT_NONE && act_in != K22_ACT_SILU) || (act_out != K22_ACT_NONE && act_out != K22_ACT_SILU))
    return k22_set_error(K22_EINVAL, "linear_smallm_ld: bad argument");
  LinearSmallParams lp = {};
  lp.x = x; lp.ldx = ldx; lp.W = W; lp.bias = bias; lp.add = add; lp.ld_add = ld_add; lp.add_mod = add_mod; lp.out = out; lp.ldo = ldo;
  lp.M = M; lp.N = N; lp.K = K; lp.act_in = act_in; lp.act_out = act_out;
  return launch_linear_smallm(lp, wdtype, reinterpret_cast<hipStream_t>(stream));   // M in 1..8, K alignment, the LDS stage: the launcher's
}
int k22_layernorm_f32(const float* x, const float* gain, const float* beta, float* y, int rows, int D, float eps, void* stream) {
  if (!x || !gain || !beta || !y || rows < 1 || D < 1) return k22_set_error(K22_EINVAL, "layernorm_f32: bad argument");
  return launch_layernorm_f32(x, gain, beta, y, rows, D, eps, reinterpret_cast<hipStream_t>(stream));
}
int k22_resample(const void* x, void* y, int B, int H, int W, int C, int mode, int dtype, void* stream) {
  if (!x || !y || B < 1 || H < 1 || W < 1 || C < 1 || (mode == 1 && (H < 2 || W < 2)) || !aux_dtype_ok(dtype))
    return k22_set_error(K22_EINVAL, "resample: bad argument");
  return launch_resample(x, y, B, H, W, C, mode, dtype, reinterpret_cast<hipStream_t>(stream));   // mode 1 | 2, C % vector: the launcher's
}
int k22_cast_rows(const float* x, void* y, int rows, int cols, long ldx, long ldy, int dtype, void* stream) {
  if (!x || !y || rows < 1 || cols < 1 || ldx < cols || ldy < cols || !aux_dtype_ok(dtype)) return k22_set_error(K22_EINVAL, "cast_rows: bad argument");
  return launch_cast_rows(x, y, rows, cols, ldx, ldy, dtype, reinterpret_cast<hipStream_t>(stream));
}
int k22_kv_pack(const void* qkv, const void* ctxkv, void* kall, void* vtall, int B, int H, int T, int S, int dtype, void* stream) {
  if (!qkv || !kall || !vtall || B < 1 || B > 65535 || H < 1 || H > 65535 || T < 1 || S < 0 || (S > 0 && !ctxkv) || !aux_dtype_ok(dtype))
    return k22_set_error(K22_EINVAL, "kv_pack: bad argument");
  KvPackParams kp;
  kp.qkv = qkv; kp.ctxkv = ctxkv; kp.kall = kall; kp.vtall = vtall; kp.B = B; kp.H = H; kp.T = T; kp.S = S;
  kp.Tkp = (S + T + 63) / 64 * 64;   // as attention_seq
  return launch_kv_pack(kp, dtype, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"

// ---- debug: LDS sentinel (tools/lds_victim_probe.py) -------------------------------------------------------------
// Every workgroup fills `bytes` of dynamic LDS with a pattern, then re-reads it `spins` times and reports words that changed under it:
// rec[0] = number of changed words seen, rec[1 + 4 * i ...] = (workgroup, byte offset, value found, spin) of the first 255 of them.
// Nothing in the product launches it; it exists to find out which kernel on ANOTHER stream writes into LDS it does not own.
__global__ __launch_bounds__(256) void lds_sentinel_kernel(int words, int spins, unsigned* rec) {
  extern __shared__ unsigned sent_lds[];
  for (int i = threadIdx.x; i < words; i += 256) sent_lds[i] = 0xA5000000u | (unsigned)i;
  __syncthreads();
  for (int s = 0; s < spins; ++s) {
    for (int i = threadIdx.x; i < words; i += 256) {
      const unsigned v = reinterpret_cast<volatile unsigned*>(sent_lds)[i];
      if (v != (0xA5000000u | (unsigned)i)) {
        const unsigned k = atomicAdd(rec, 1u);
        if (k < 255u) { rec[1 + 4 * k] = blockIdx.x; rec[2 + 4 * k] = 4u * i; rec[3 + 4 * k] = v; rec[4 + 4 * k] = (unsigned)s; }
        sent_lds[i] = 0xA5000000u | (unsigned)i;
      }
    }
    __builtin_amdgcn_s_sleep(8);
  }
}
extern "C" int k22_debug_lds_sentinel(int bytes, int workgroups, int spins, unsigned* rec, void* stream) {
  if (bytes <= 0 || bytes > 64 * 1024 || (bytes & 3) || !rec) return k22_set_error(K22_EINVAL, "lds_sentinel: bytes in 4..65536, multiple of 4");
  hipLaunchKernelGGL(lds_sentinel_kernel, dim3(workgroups), dim3(256), (size_t)bytes, reinterpret_cast<hipStream_t>(stream), bytes / 4, spins, rec);
  K22_CHECK_LAUNCH();
  return K22_OK;
}
