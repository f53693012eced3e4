// k22 — small per-call / per-step latent arithmetic of the img2img and inpainting pipelines:
//   noised(t)  = sa * init + sb * noise                      DDPMScheduler.add_noise / q_sample (kandinsky2/utils.py:43-54)
//   out        = mask * noised(t) + (1 - mask) * x           the per-step re-imposition of the known region in the Kandinsky 2.2
//                                                            inpainting pipeline (diffusers KandinskyV22InpaintPipeline loop, used by
//                                                            kandinsky2/kandinsky2_2_model.py:150-173); mask [N][1][h][w], 1 = keep
// One elementwise kernel; x == nullptr / mask == nullptr gives plain add_noise.
//   keep_region: the same re-imposition over the whole CFG batch of a captured loop in ONE launch (k22_unet_sample_loop_keep): image 0's
//                init / mask for every row, row n re-noised with sample n % bs's own initial noise, every operation rounded once.
#include "kernels.h"
#include "elementwise.h"
#include "../../include/k22.h"

namespace {
__global__ __launch_bounds__(256) void blend_noised_kernel(const float* x, const float* init, const float* noise, const float* mask, float sa,
                                                           float sb, float* out, int C, int HW, int64_t total, int init_bcast) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / ((int64_t)C * HW), p = i % HW;
    const int64_t j = init_bcast ? i % ((int64_t)C * HW) : i;         // init / noise / mask of image 0 serve the whole batch
    const float v = sa * init[j] + (noise != nullptr ? sb * noise[j] : 0.f);
    if (mask == nullptr) { out[i] = v; continue; }
    const float m = mask[(init_bcast ? 0 : n) * HW + p];
    out[i] = m * v + (1.f - m) * x[i];
  }
}
}  // namespace

extern "C" int k22_blend_noised(const float* x, const float* init, const float* noise, const float* mask, float sa, float sb, float* out,
                                int N, int C, int HW, int broadcast_first, void* stream) {
  if (!init || !out || N < 1 || C < 1 || HW < 1) return k22_set_error(K22_EINVAL, "blend_noised: bad argument");
  if (mask != nullptr && x == nullptr) return k22_set_error(K22_EINVAL, "blend_noised: a mask needs the current latent x");
  const int64_t total = (int64_t)N * C * HW;
  const int nb = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(blend_noised_kernel, dim3(nb), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, init, noise, mask, sa, sb, out, C, HW,
                     total, broadcast_first ? 1 : 0);
  K22_CHECK_LAUNCH();
  return K22_OK;
}

// ---- known region of the 2.2 inpainting loop over the whole CFG batch ---------------------------------------------------------------
//   out[n][c][p] = m[p] * (sa * init[c][p] + sb * noise0[n % bs][c][p]) + (1 - m[p]) * x[n][c][p]        n < B = 2 bs, c < 4, p < HW
// init [4][HW] and m [HW] are image 0's and serve every row; noise0 [bs][4][HW] is each sample's own initial noise, which both CFG halves
// of a sample share.  Every product, sum and difference is rounded once (no contraction into FMAs: see the kernel), so |out - exact| <= 4 * 2^-24 * S with
// S = |m| (|sa init| + |sb noise|) + |1 - m| |x| follows from the code: product, inner sum, product by m, outer sum on the longest path
// (tests/decoder22_ref.py).  Each thread reads x[i] before it writes out[i] and no other thread touches element i: out == x is allowed.
namespace {
__global__ __launch_bounds__(256) void keep_region_kernel(const float* x, const float* init, const float* noise0, const float* mask, float sa,
                                                          float sb, float* out, int bs, int HW, int64_t total) {
  // One instruction per operation: contraction is switched off for this body and the operations are written as plain operators.  (The
  // __fmul_rn / __fadd_rn intrinsics are inline functions of the HIP headers, compiled under the headers' contraction mode: after inlining
  // the compiler fused their product and sum into one v_fmac - one rounding fewer, and other bits than the host's evaluation.)
#pragma clang fp contract(off)
  const int64_t chw = 4 * (int64_t)HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / chw, cp = i - n * chw;
    const float m = mask[cp % HW];
    const float a = sa * init[cp], b = sb * noise0[(n % bs) * chw + cp];
    const float v = a + b;
    const float kept = m * v, rest = (1.f - m) * x[i];
    out[i] = kept + rest;
  }
}
}  // namespace

int launch_keep_region(const float* x, const float* init, const float* noise0, const float* mask, float sa, float sb, float* out, int B,
                       int HW, hipStream_t s) {
  if (!x || !init || !noise0 || !mask || !out) return k22_set_error(K22_EINVAL, "keep_region: null argument");
  if (B < 2 || (B & 1) || HW < 1) return k22_set_error(K22_EINVAL, "keep_region: B is the CFG batch [cond | uncond] (even, >= 2), HW >= 1");
  const int64_t total = (int64_t)B * 4 * HW;
  int nb = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(keep_region_kernel, dim3(nb), dim3(256), 0, s, x, init, noise0, mask, sa, sb, out, B / 2, HW, total);
  K22_CHECK_LAUNCH();
  return K22_OK;
}

extern "C" int k22_keep_region(const float* x, const float* init, const float* noise0, const float* mask, float sa, float sb, float* out,
                               int B, int HW, void* stream) {
  return launch_keep_region(x, init, noise0, mask, sa, sb, out, B, HW, reinterpret_cast<hipStream_t>(stream));
}
