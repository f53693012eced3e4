// k22 — host-side substrate shared by the four native engines (UNet engine.hip, MoVQ movq.hip, prior prior.hip, conditioning towers
// encoder.hip): workspace slots, the weight table, the plan / bind life cycle, the cached hipGraph of a launch list, and the keyed
// graph of a whole sampling loop.  Host-only.
//
// Life cycle of a handle (include/k22.h):  create -> plan -> bind -> run.
//   plan   begin_plan() drops everything of the previous plan; the engine sizes its slots and builds its launch list; finish_plan() lays the
//          slots out.  A plan that did not reach the end of finish_plan() is NO plan (a missing weight is only known there, and the launch
//          list built so far holds null weight pointers): `planned` stays clear, bind() answers "plan first", the run entries find no workspace.
//   bind   attaches the caller's workspace; whatever was cached for the previous one (graphs, per-binding copies) is dropped.
//   run    the launch list, eagerly or as one cached graph (GraphPlan::replay).
#pragma once
#include "kernels.h"
#include "tuning.h"
#include "../../include/k22.h"

#include <deque>
#include <string>
#include <unordered_map>
#include <vector>
#include <stdint.h>
#include <stdlib.h>

struct Slot { size_t bytes = 0, off = 0; };

inline int copy_d2d(void* dst, const void* src, size_t bytes, hipStream_t st) {
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st);
  return e == hipSuccess ? (int)K22_OK : k22_set_error_hip(e, __FILE__, __LINE__);
}

// K22_* switches read from the environment: unset = dflt, else "is it non-zero"
inline int env_flag(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? (atoi(e) != 0) : dflt;
}

// A launch list (callables taking the stream) in order, entries [lo, hi) of it; the first failing entry ends the run.
template <typename List> int run_list(const List& ops, hipStream_t st, size_t lo = 0, size_t hi = (size_t)-1) {
  for (size_t i = lo; i < hi && i < ops.size(); ++i) { if (int rc = ops[i](st)) return rc; }
  return K22_OK;
}

struct PlanBase {
  int dtype = 0;     // K22DType of the arithmetic
  size_t esz = 0;    // bytes per stored activation element
  std::unordered_map<std::string, const void*> w;
  std::deque<Slot> slots;   // stable addresses: op closures hold Slot pointers
  size_t ws_bytes = 0;
  char* ws = nullptr;
  bool planned = false;
  std::string err;          // first problem met while the plan was built (reported by finish_plan)

  void set_dtype(int dt) { dtype = dt; esz = k22_esz(dt); }
  void set_weights(const K22Weight* weights, int n) { for (int i = 0; i < n; ++i) w[weights[i].name] = weights[i].ptr; }

  Slot* new_slot(size_t bytes = 0) { slots.emplace_back(); slots.back().bytes = bytes; return &slots.back(); }
  static void need(Slot* s, size_t bytes) { if (bytes > s->bytes) s->bytes = bytes; }
  template <typename T = char> T* ptr(const Slot* s) const { return reinterpret_cast<T*>(ws + s->off); }

  const void* W_(const std::string& name) {
    auto it = w.find(name);
    if (it == w.end()) { if (err.empty()) err = "missing weight: " + name; return nullptr; }
    return it->second;
  }
  const float* Wf(const std::string& name) { return reinterpret_cast<const float*>(W_(name)); }

  void begin_plan() { slots.clear(); ws = nullptr; ws_bytes = 0; err.clear(); planned = false; }
  int finish_plan() {
    if (!err.empty()) return k22_set_error(K22_EINVAL, err.c_str());
    size_t off = 0;
    for (auto& s : slots) { s.off = off; off += (s.bytes + 255) / 256 * 256; }
    ws_bytes = off + 256;
    planned = true;
    return K22_OK;
  }
  // `who`: the C entry's name, the prefix of its messages.  What else an engine resets per binding follows the call in its k22_*_bind.
  int bind(void* workspace, size_t workspace_bytes, const char* who) {
    const std::string p = std::string(who) + ": ";
    if (!workspace) return k22_set_error(K22_EINVAL, (p + "null argument").c_str());
    if (!planned) return k22_set_error(K22_EINVAL, (p + "plan first").c_str());
    if (workspace_bytes < ws_bytes) return k22_set_error(K22_ENOMEM, (p + "workspace too small").c_str());
    if ((uintptr_t)workspace % 256) return k22_set_error(K22_EINVAL, (p + "workspace must be 256-byte aligned").c_str());
    ws = reinterpret_cast<char*>(workspace);
    return K22_OK;
  }
};

// The private stream a handle CAPTURES on (the caller's may be the legacy default stream): created at the first capture.
struct CaptureStream {
  hipStream_t s = nullptr;
  ~CaptureStream() { if (s) (void)hipStreamDestroy(s); }
  int get(hipStream_t* out) {
    if (!s) {
      const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
      if (e != hipSuccess) { s = nullptr; return k22_set_error_hip(e, __FILE__, __LINE__); }
    }
    *out = s;
    return K22_OK;
  }
};

// One instantiated graph of a launch list.  Single chain: what `run` issues on the capture stream, in order.
struct GraphCache {
  hipGraphExec_t exec = nullptr;
  ~GraphCache() { drop(); }
  explicit operator bool() const { return exec != nullptr; }
  void drop() { if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; } }
  template <typename F> int capture(CaptureStream& cs, F run) {
    drop();
    hipStream_t s = nullptr;
    if (int rc = cs.get(&s)) return rc;
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return k22_set_error_hip(e, __FILE__, __LINE__);
    const int rc = run(s);
    e = hipStreamEndCapture(s, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) return k22_set_error_hip(e, __FILE__, __LINE__);
    e = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) { exec = nullptr; return k22_set_error_hip(e, __FILE__, __LINE__); }
    return K22_OK;
  }
  int launch(hipStream_t st) const {
    const hipError_t e = hipGraphLaunch(exec, st);
    return e == hipSuccess ? (int)K22_OK : k22_set_error_hip(e, __FILE__, __LINE__);
  }
};

// The ONE captured whole loop of an engine (a sampling loop: many passes of the launch list with step kernels between them) and the key
// it is valid for: every pointer and scalar baked into its nodes, the loop's kind first.  A word missing from the key is a stale replay.
struct LoopCache {
  GraphCache graph;
  std::vector<unsigned long long> key;
  void drop() { graph.drop(); key.clear(); }
  // `body` (one pass over the whole loop on a stream) eagerly on `st`, or as the captured loop valid for `k`, captured on a miss: what a
  // capture records is exactly what an eager call runs.  Whatever has to run before a first capture (warm-up) the caller has run.
  template <typename F> int run(CaptureStream& cs, const std::vector<unsigned long long>& k, int use_graph, hipStream_t st, F body) {
    if (use_graph && (!graph || k != key)) {
      if (int rc = graph.capture(cs, body)) { drop(); return rc; }
      key = k;
      loop_count_capture();
    }
    const int rc = use_graph ? graph.launch(st) : body(st);
    if (rc == K22_OK) loop_count_launch();
    return rc;
  }
};

// A plan whose conv / GEMM launches carry tuned tile configurations and whose launch list is replayed as a graph (UNet, prior, towers).
struct GraphPlan : PlanBase {
  std::deque<Tuned> tuned;   // stable addresses: op closures point into it
  bool tuned_done = false;
  int autotune = env_flag("K22_AUTOTUNE", 1);   // 0 = heuristics only (no measurement at the first pass)
  bool warmed = false;       // one eager pass of the launch list has run on this plan (function attributes set, code loaded): capture may start
  CaptureStream cap;
  GraphCache graph;          // one forward

  void begin_plan() { PlanBase::begin_plan(); tuned.clear(); tuned_done = false; warmed = false; graph.drop(); }
  int bind(void* workspace, size_t workspace_bytes, const char* who) {
    const int rc = PlanBase::bind(workspace, workspace_bytes, who);
    if (rc == K22_OK) graph.drop();   // its nodes hold the old workspace's addresses
    return rc;
  }

  // conv / GEMM problems the tile table does not know are measured on the device, once per plan.  (In-place residual GEMMs accumulate
  // garbage into their output meanwhile: the pass that follows rebuilds it from the inputs.)
  int tune_once(const Slot* s_flush, hipStream_t st) {
    if (!autotune || tuned_done) return K22_OK;
    const int rc = tune_igemm_ops(tuned, dtype, s_flush->bytes ? ptr(s_flush) : nullptr, s_flush->bytes, st);
    if (rc == K22_OK) tuned_done = true;
    return rc;
  }

  template <typename F> int run_eager(hipStream_t st, F run) {
    const int rc = run(st);
    if (rc == K22_OK) warmed = true;
    return rc;
  }
  // `run` as the cached graph `g` on `st`.  The first capture of a plan is preceded by one eager pass; a re-capture (new binding) is not.
  template <typename F> int replay(GraphCache& g, hipStream_t st, F run) {
    if (!g) {
      if (!warmed) { if (int rc = run_eager(st, run)) return rc; }
      if (int rc = g.capture(cap, run)) return rc;
    }
    return g.launch(st);
  }

  // out = act(A[M][K] . W[N][K]^T + bias) over T rows at byte offset a_off of `a`, tile configuration from the table / measurement.
  // mode 0 -> T rows; 1 -> fp32 rows; 2 -> fp32 rows += (in-place residual stream).  Returns the launch; the engine appends it to its list.
  Tuned* tuned_linear(Slot* a, size_t a_off, int M, int N, int K, const std::string& pfx, int act, Slot* dst, size_t dst_off, int ldo, int mode,
                      Slot* s_splitk) {
    tuned.emplace_back();
    Tuned* t = &tuned.back();
    IgemmParams& p = t->p;
    p = igemm_gemm_problem(M, N, K, 0, mode == 0 ? IG_OUT_ROWMAJOR : IG_OUT_ROWMAJOR_F32, act);
    p.ldo = ldo; p.ldr = ldo; p.res_f32 = mode == 2 ? 1 : 0;   // rows of a wider tensor; mode 2: the residual is the output row itself
    p.Wp = W_(pfx + ".weight"); p.bias = Wf(pfx + ".bias");
    tuned_make_candidates(*t, dtype);
    tuned_default_cfg(*t, dtype);
    need(s_splitk, tuned_max_splitk_bytes(*t, dtype, autotune != 0));
    const int dt = dtype;
    t->run = [=](hipStream_t st) {
      IgemmParams q = t->p;
      tuned_apply_cfg(q, t->cfg);
      q.A0 = ptr(a) + a_off; q.out = ptr(dst) + dst_off; q.partial = ptr<float>(s_splitk);
      q.residual = mode == 2 ? (ptr(dst) + dst_off) : nullptr;
      return launch_igemm(q, dt, st);
    };
    return t;
  }
};
