// k22 — internal kernel launch API (host side).  Every launcher enqueues on `stream`, allocates
// nothing and returns 0 or a negative K22_E* code (message via k22_last_error()).
#pragma once
#include "common.h"

#include <atomic>
#include <stdint.h>
#include <string.h>
#include <type_traits>

#define K22_OK 0
#define K22_EINVAL (-1)
#define K22_EHIP (-2)
#define K22_ENOMEM (-3)

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute: one guard per kernel instantiation holds a
// bit per device ordinal, so a process that drives several GPUs (or launches from several threads) sets it on each.
struct LdsAttrGuard { std::atomic<unsigned long long> done{0}; };
inline int k22_ensure_lds_attr(LdsAttrGuard& g, const void* fn, int bytes, const char* file, int line) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long bit = 1ull << (dev & 63);
  if (g.done.load(std::memory_order_acquire) & bit) return K22_OK;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return k22_set_error_hip(e, file, line);
  g.done.fetch_or(bit, std::memory_order_release);
  return K22_OK;
}

// ---------------------------------------------------------------------------------------
// Implicit GEMM:  out[m][n] = sum_k A(m,k) * Wp[n][k]  (+bias[n]) (+residual[m][n]) -> act
//   taps == 1 : plain GEMM, A row m = A0[m*lda0 + k] for k < K0, else A1[m*lda1 + (k-K0)]
//               ("virtual concat" of two row-major operands; A1 may be null when K0 == Kc).
//   taps == 9 : 3x3 convolution, stride 1, pad 1 over a ZERO-BORDERED NHWC input
//               A0 = [B][H+2][W+2][Kc]; m = (b*H + y)*W + x; k = tap*Kc + c, tap = ky*3+kx.
//   taps == 4 : nearest 2x upsample + 3x3 convolution in its four-phase form (conv3_up2.hip): A0 = [B][H+2][W+2][Kc] is the zero-bordered
//               LOW-resolution input, M = B*2H*2W rows of the unpadded 2H x 2W output, Wp = the folded weights [phase 4][Npad][tap 2x2][Kc].
//   Wp is the packed weight [Npad][taps*Kc] (K contiguous), Npad = roundup(N, 64), zero rows.
// ---------------------------------------------------------------------------------------
enum IgemmOut { IG_OUT_ROWMAJOR = 0,  // T out[m*ldo + n]
                IG_OUT_ROWMAJOR_F32 = 1,  // float out[m*ldo + n]
                IG_OUT_NCHW_F32 = 2,      // float out[((b*N + n)*H + y)*W + x]   (m = (b*H+y)*W+x)
                IG_OUT_QKV = 3 };         // qkv projection (N = 3C, columns [q | k | v] x [heads][64]) written straight into
                                          // the attention operands: q -> T out[m*ldo + n];  k -> kall[b][head][S+t][d];
                                          // v -> vtall[b][head][d][S+t]   (m = b*T + t; see AttentionParams)

struct IgemmParams {
  const void* A0;
  const void* A1;
  const void* Wp;
  const float* bias;     // [N] or null
  const void* residual;  // T [M][ldr] or null (fp32 [M][ldr] when res_f32 is set: fp32 residual stream of the prior)
  void* out;
  float* partial;        // split-K scratch [splitk][M][N] fp32 (needed when splitk > 1)
  int M, N, Npad;
  int Kc;                // K elements per tap (K0 + K1 in concat mode)
  int K0;                // channels served by A0 (== Kc when A1 is null)
  int taps;              // 1, 9 or 4 (above)
  int H, W;              // conv geometry (taps == 9) and NCHW store geometry
  long lda0, lda1;       // row strides (elements) in GEMM mode
  int ldo, ldr;
  int out_mode;          // IgemmOut
  int act;               // K22Act applied after bias+residual
  int splitk;            // >= 1 (0 = let the launcher choose)
  int force_bm, force_bn;  // 0 = heuristic
  int stages = -1;       // ring depth request (see igemm_resolve): 2..4 generic kernel, 2..5 halo kernels, gemm8: 2 = two per CU, 3 / 4 = specialised form;
                         // anything else = default ("igemm_stages" option, env K22_IGEMM_STAGES, else 2 / the deepest ring that fits)
  int xcd_remap;         // set by the launcher: XCD-aware block renumbering on/off
  int algo;              // IgemmAlgo (below): 0 = heuristic / "conv_algo", "gemm_algo" options
  // optional fused 1x1 "skip_connection" of a ResBlock (unet.py:191), halo kernel only:
  //   out += [S0 | S1](unpadded NHWC rows m, SK0 + SK1 channels) . Ws[n][SK0+SK1]^T + bias2[n]
  const void* S0; const void* S1; const void* Ws; const float* bias2;
  int SK0, SK1;
  void* kall; void* vtall;                 // IG_OUT_QKV only
  int att_T, att_S, att_Tkp;               // IG_OUT_QKV only: tokens per image, context keys, padded key count
  // weight-streaming kernel (stream_gemm.hip): the weights again in FRAGMENT-MAJOR order - [n-block of 32 rows][(slab, tap) item][k quarter]
  // [lane][8 elements] = 1 KB contiguous per MFMA B fragment - written once by launch_stream_repack (Wsfrag: the fused 1x1 skip's weights);
  // null = fragments are gathered from the row-major Wp / Ws (32 bytes of 32 different lines per load: measured L1-lookup bound).
  // (They stand between att_* and res_f32, which the generic kernel and the split-K finish read together, so that hipcc loads those as
  // two groups, the code it was measured with: profiles/debug_variants_removed_device_code.txt.)
  const void* Wfrag; const void* Wsfrag;
  int res_f32;           // residual is fp32 (generic kernel / split-K finish only)
  float* stats;          // optional GroupNorm side output: per-row-block, per-channel (sum, sumsq) of the STORED
                         // values, [stats_rows][N][2] fp32 (see IgemmStatsInfo); null = not wanted
  int a_raw;             // K22_F16X3 only: 1 = the A operand (A0 / A1) is plain fp32 rows, converted to split halves at fragment-read
                         // time (generic kernel and gemm8 only); 0 = A is in x3 chunks (common.h), written so by its producer.
                         // The fused-skip operands S0 / S1 are always plain fp32 rows; weights are always x3 chunks.
  int st_tm, st_rb, st_mtiles, st_buf;   // set by launch_stream (stream_gemm.hip): rows per m-tile, image rows per band, m-tiles, bytes of one LDS A buffer
};
// kernel argument, copied by value into every launch: the layout is what the kernels were compiled against
static_assert(sizeof(IgemmParams) == 272 && std::is_trivially_copyable<IgemmParams>::value, "IgemmParams layout");

// IG_OUT_QKV: where W (4 or 8) consecutive columns COL.. of row ROW = token TOK of image IMG go (values V[W], rounded to T; p = the problem).
// Columns are [q | k | v] x [heads][64]: q row-major, k behind the context keys of K_all, v transposed into V^T_all.  The one text of
// these addresses (igemm_kernel, splitk_reduce_kernel, halo_tail); a macro: as a function it moved the code of the first two.
// IMG and TOK are evaluated once, behind the column split and in this order (the expression TOK may name img_): the order of the two
// divisions is part of what hipcc's output follows.
#define K22_QKV_SCATTER(T, W, V, ROW, IMG, TOK, COL)                                                       \
  {                                                                                                        \
    const int C = p.N / 3, heads = C >> 6;                                                                 \
    const int which = (COL) / C, c = (COL) - which * C;                                                    \
    const int head = c >> 6, d = c & 63;                                                                   \
    const int img_ = (IMG), tok_ = (TOK);                                                                  \
    if (which == 0) {                                                                                      \
      store_row<T, W>(reinterpret_cast<T*>(p.out) + (int64_t)(ROW) * p.ldo + c, V);                        \
    } else if (which == 1) {                                                                               \
      store_row<T, W>(reinterpret_cast<T*>(p.kall) + ((int64_t)(img_ * heads + head) * p.att_Tkp + p.att_S + tok_) * 64 + d, V); \
    } else {                                                                                               \
      T* vt = reinterpret_cast<T*>(p.vtall) + ((int64_t)(img_ * heads + head) * 64 + d) * p.att_Tkp + p.att_S + tok_; \
      _Pragma("unroll") for (int e = 0; e < (W); ++e) vt[(int64_t)e * p.att_Tkp] = from_f32<T>(V[e]);      \
    }                                                                                                      \
  }

// The kernel variants.  The numbers are ABI: K22IgemmProblem.algo, the "conv_algo" / "gemm_algo" options and the tile table use them.
// 8, 9, 13 and 14 are RESERVED: they named measurement-only forms (wrong results by design) that have left the source; no kernel answers to
// them (tuned_is_candidate refuses them, "conv_algo" maps them to auto) and the numbers are not to be given out again.
enum IgemmAlgo {
  IG_ALGO_AUTO = 0,             // heuristic
  IG_ALGO_GENERIC = 1,          // igemm_kernel (igemm.hip): 4 waves, bm x bn tile
  IG_ALGO_HALO = 2,             // conv3_halo_kernel, lock-step, compiler-issued LDS-DMA
  IG_ALGO_HALO3 = 3,            // conv3_halo3_kernel: 64-byte rows, one filter row per iteration
  IG_ALGO_HALO_PIPE = 6,        // conv3_halo_kernel, asm LDS-DMA + explicit fragment pipeline
  IG_ALGO_HALO_ASM = 7,         // conv3_halo_kernel, asm LDS-DMA
  IG_ALGO_GEMM8 = 10,           // gemm8_kernel / gemm8_spec_kernel (gemm8.hip): plain GEMM on the 8-wave frame
  IG_ALGO_SPEC = 11,            // conv3_halo_spec_kernel (conv3_spec.hip): producer / consumer waves
  IG_ALGO_SPEC_PIPE = 12,       //   + explicit, interleaved fragment pipeline in the consumers
  IG_ALGO_STREAM = 20,          // stream_kernel (stream_gemm.hip): weight streaming for small M
  IG_ALGO_UP2 = 30,             // conv3_up2_kernel (conv3_up2.hip): the taps == 4 problems, and only they
  IG_ALGO_UP2_PIPE = 31         //   + explicit fragment pipeline (16-bit types)
};
struct IgemmAlgoName { int algo; const char* name; };   // tuning_report_text's column
constexpr IgemmAlgoName IGEMM_ALGO_NAMES[] = {{IG_ALGO_GENERIC, "gen"},   {IG_ALGO_HALO, "halo"},   {IG_ALGO_HALO3, "hal3"}, {IG_ALGO_HALO_PIPE, "hal6"},
                                              {IG_ALGO_HALO_ASM, "hal7"}, {IG_ALGO_GEMM8, "gem8"}, {IG_ALGO_SPEC, "spec"},  {IG_ALGO_SPEC_PIPE, "spcp"},
                                              {IG_ALGO_UP2, "up2"}, {IG_ALGO_UP2_PIPE, "up2p"}};
inline const char* igemm_algo_name(int algo) {
  for (const IgemmAlgoName& a : IGEMM_ALGO_NAMES) if (a.algo == algo) return a.name;
  return "auto";
}
inline bool igemm_algo_is_halo(int a) {
  return a == IG_ALGO_HALO || a == IG_ALGO_HALO3 || a == IG_ALGO_HALO_PIPE || a == IG_ALGO_HALO_ASM || a == IG_ALGO_SPEC || a == IG_ALGO_SPEC_PIPE;
}

// The derived fields of a problem descriptor (Npad, Kc, taps, row strides, geometry); operands, configuration and whatever is particular
// to a call site are set by the caller.
inline IgemmParams igemm_gemm_problem(int M, int N, int K0, int K1, int out_mode = IG_OUT_ROWMAJOR, int act = 0) {
  IgemmParams p = {};
  p.M = M; p.N = N; p.Npad = (N + 63) / 64 * 64; p.Kc = K0 + K1; p.K0 = K0; p.taps = 1;
  p.lda0 = K0; p.lda1 = K1; p.ldo = N; p.ldr = N; p.out_mode = out_mode; p.act = act;
  return p;
}
inline IgemmParams igemm_conv3_problem(int B, int H, int W, int Cin, int Cout, int out_mode = IG_OUT_ROWMAJOR, int act = 0) {
  IgemmParams p = {};
  p.M = B * H * W; p.N = Cout; p.Npad = (Cout + 63) / 64 * 64; p.Kc = Cin; p.K0 = Cin; p.taps = 9; p.H = H; p.W = W;
  p.ldo = Cout; p.ldr = Cout; p.out_mode = out_mode; p.act = act;
  return p;
}

// nearest 2x upsample + conv3x3 over a LOW-resolution H x W input, four-phase form (taps == 4)
inline IgemmParams igemm_up2_problem(int B, int H, int W, int Cin, int Cout, int out_mode = IG_OUT_ROWMAJOR) {
  IgemmParams p = igemm_conv3_problem(B, H, W, Cin, Cout, out_mode);
  p.M = B * 4 * H * W; p.taps = 4;
  return p;
}

// ---- one resolved launch ----------------------------------------------------------------------------------------------------------
// What launch_igemm runs for a problem: igemm_resolve is the ONE place that reads p.algo / p.force_bm / p.force_bn / p.splitk / p.stages and
// the process-wide options; the plan-time questions (split-K scratch, GroupNorm stats rows) and the launch read the same result.
enum IgemmFamily { IG_FAM_GENERIC, IG_FAM_HALO, IG_FAM_HALO3, IG_FAM_SPEC, IG_FAM_GEMM8, IG_FAM_GEMM8_SPEC, IG_FAM_STREAM, IG_FAM_UP2 };
enum IgemmFinish { IG_FINISH_NONE, IG_FINISH_FLAT, IG_FINISH_ROWS };   // split-K finish: none, splitk_reduce_kernel, splitk_reduce_rows_kernel
struct IgemmLaunch {
  int family;                // IgemmFamily
  int algo;                  // IgemmAlgo the problem resolved to (never AUTO)
  int bm, bn;                // tile (stream: bm = 32 * m-blocks per workgroup)
  int splitk;
  int depth;                 // template ring depth instantiated: STAGES (generic), NBST (halo, spec), RB (halo3), NST (gemm8); 0 = stream
  int pipe;                  // form instantiated: halo = MODE (0 lock-step, 1 pipelined, 2 asm LDS-DMA); spec / gemm8_spec = PIPE after the
                             // BM = 256 fall-back of x3 / fp32
  int a_raw;                 // ARAW instantiation (split types, generic kernel and gemm8)
  int xcd_remap;
  int finish;                // IgemmFinish
  int stats_rows_per_image;  // GroupNorm partial-sum rows per image this launch can write (0 = none)
  unsigned grid, block;
  size_t lds;                // dynamic LDS bytes
};
struct IgemmOptions { int conv_algo = 0, gemm_algo = 0, stages = -1, xcd_remap = 1; };   // k22_set_option; read by igemm_resolve only
// 0, or the error the launch would fail with.  Operands may be markers / null (plan time): only their presence is looked at.
int igemm_resolve(const IgemmParams& p, int dtype, IgemmLaunch* L);

// The one launch sequence of the kernels with dynamic LDS: per-device attribute (guard: one per instantiation), launch, check.
template <typename K>
inline int launch_lds_kernel(K kernel, LdsAttrGuard& guard, unsigned grid, unsigned block, size_t smem, int attr_bytes, hipStream_t stream, const IgemmParams& params) {
  if (int rc = k22_ensure_lds_attr(guard, reinterpret_cast<const void*>(kernel), attr_bytes, __FILE__, __LINE__)) return rc;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), smem, stream, params);
  K22_CHECK_LAUNCH();
  return K22_OK;
}

// How a producer laid out its GroupNorm partial sums: image b owns rows [b*rows_per_image, (b+1)*rows_per_image).
struct IgemmStatsInfo { int rows_per_image; };
// Number of stats rows per image launch_igemm will write for this problem (0 = this configuration cannot
// produce stats; the caller must run the stand-alone gn_stats kernel instead).  igemm_resolve's stats_rows_per_image.
int igemm_stats_rows_per_image(const IgemmParams& p, int dtype);

int launch_igemm(const IgemmParams& p, int dtype, hipStream_t stream);

// The kernel families behind launch_igemm.  *_supported: can the family run the problem at this tile (the tuner's candidate list, the
// engines and igemm_resolve ask the same predicates); *_lds_bytes / *_ring: their LDS budget, for igemm_resolve; launch_*: select the
// instantiation the resolved launch names and run it with the parameters as given (a split-K finish is launch_igemm's).
// conv3_halo.hip: 3x3 convolution with the input tile (+halo) resident in LDS across the 9 taps (p.algo: which of its kernels).
bool conv3_halo_supported(const IgemmParams& p, int dtype, int bm);
int conv3_halo_tiles_per_image(const IgemmParams& p, int bm);
int conv3_halo_ring(const IgemmParams& p, int bm);                     // deepest weight ring that fits (0 = none)
size_t conv3_halo_lds_bytes(const IgemmParams& p, int bm, int depth);
int launch_conv3_halo(const IgemmParams& p, int dtype, const IgemmLaunch& L, hipStream_t stream);
int launch_conv3_halo_spec(const IgemmParams& p, int dtype, const IgemmLaunch& L, hipStream_t stream);   // conv3_spec.hip
// conv3_up2.hip: the four-phase form of upsample + conv3x3 (taps == 4), and the one-time fold of its weights
bool conv3_up2_supported(const IgemmParams& p, int dtype, int bm);
int conv3_up2_tiles_per_image(const IgemmParams& p, int bm);
int conv3_up2_ring(const IgemmParams& p, int bm);
size_t conv3_up2_lds_bytes(const IgemmParams& p, int bm, int depth);
int launch_conv3_up2(const IgemmParams& p, int dtype, const IgemmLaunch& L, hipStream_t stream);
int launch_up2_fold(const float* w, float* out, int O, int Opad, int I, hipStream_t stream);   // [O][9][I] fp32 -> [4][Opad][4][I] fp32
// gemm8.hip: 8-wave BM x 128 GEMM on the halo kernels' frame
bool gemm8_supported(const IgemmParams& p, int dtype, int bm);
bool gemm8_spec_supported(int dtype);   // gemm8_spec_kernel (producer / consumer waves, explicit fragment pipeline): 16-bit types
int gemm8_tiles_per_image(const IgemmParams& p, int bm);
size_t gemm8_lds_bytes(int bm, int depth);
int launch_gemm8(const IgemmParams& p, int dtype, const IgemmLaunch& L, hipStream_t stream);
// stream_gemm.hip: weight-streaming kernel for small M (mb = 5 / 9 m-blocks per workgroup: force_bm 160 / 288).
// It leaves fp32 partial tiles [splitk][M][N] in p.partial (also for splitk == 1); launch_igemm runs the split-K finish.
bool stream_supported(const IgemmParams& p, int dtype, int mb);
int stream_mtiles(const IgemmParams& p, int mb);
size_t stream_lds_bytes(const IgemmParams& p, int mb);
int launch_stream(const IgemmParams& p, int dtype, const IgemmLaunch& L, hipStream_t stream);
long stream_launch_count();
// movq_attention.hip: fused single-head attention of the MoVQ AttnBlock, out[b][t][:] = softmax_j(C^-1/2 q_t . k_j) v_j + bias_v with
// q, k [B][T][C], vt [B][C][T], out [B][T][C] in the storage type (K22_BF16 / K22_F16 / K22_F32; 16-byte aligned), bias_v fp32 [C] or null.
// Admitted: C in {128, 256, 384, 512}, T a positive multiple of 64 (at most 2^22: the kernel's lane offsets are 32-bit), B >= 1; anything else
// is K22_EINVAL.  One launch for all images.
inline bool movq_attention_admits_c(int C) { return C == 128 || C == 256 || C == 384 || C == 512; }
inline bool movq_attention_admits_t(int T) { return T >= 64 && T % 64 == 0 && T <= (1 << 22); }
int launch_movq_attention(const void* q, const void* k, const void* vt, const float* bias_v, void* out, int B, int T, int C, int dtype, hipStream_t s);
long movq_fused_attn_launch_count();   // successful launches since the library was loaded
// engine.hip: whole-loop graphs captured / whole-loop replays or eager loop runs since the library was loaded
long loop_capture_count();
long loop_launch_count();
void loop_count_capture();   // called by every loop entry (engine.hip, prior.hip)
void loop_count_launch();
// what a captured loop's key is made of: every pointer and scalar baked into its nodes
inline unsigned long long loop_key_ptr(const void* p) { return (unsigned long long)(uintptr_t)p; }
inline unsigned long long loop_key_bits(double v) { unsigned long long b; memcpy(&b, &v, 8); return b; }
// bytes of the fragment-major copy of a [Npad][taps * Kc] weight matrix, and the one-time repack (any 16-bit dtype)
size_t stream_frag_bytes(int Npad, int taps, int Kc, int dtype);
int launch_stream_repack(const void* W, void* out, int Npad, int taps, int Kc, int dtype, hipStream_t stream);
// k22_set_option's conv / GEMM knobs (IgemmOptions; values outside the accepted set select the default)
void igemm_set_gemm_algo(int v);       // 0 auto, IG_ALGO_GEMM8, IG_ALGO_STREAM
void igemm_set_conv_algo(int v);       // 0 auto or an IgemmAlgo of the convolutions
void igemm_set_default_stages(int v);  // 2..4 ring depth, -1 env/default
void igemm_set_xcd_remap(int v);       // XCD-aware block renumbering (default on)
void attention_set_pipe(int v);        // test knob: -1 K22_ATT_PIPE / default, 0 attention_kernel, 1 attention_pipe_kernel (unmasked 16-bit attention)
int igemm_choose_splitk(const IgemmParams& p, int dtype);  // split-K factor the heuristic picks (scratch = splitk*M*N*4 B)
