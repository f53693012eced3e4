/* k22.h — C ABI of libk22hip.so, the MI355X (gfx950) native Kandinsky-2 sampling engine.
 *
 * The reference (ai-forever/Kandinsky-2, pure PyTorch) has no FFI; its seams on the sampling hot path
 * are Python objects.  Each entry point below names the reference call it replaces
 * (paths relative to the reference tree).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - extern "C"; every function returns 0 (K22_OK) or a negative K22_E* code; k22_last_error()
 *     returns a thread-local message.  No C++ exception crosses the boundary.
 *   - The CALLER owns every buffer (inputs, outputs, weight arena, workspace).  All pointers are
 *     device pointers valid on the current HIP device unless a parameter says "host".
 *   - All work is ENQUEUED on the hipStream_t passed as `stream` (void* here so the header needs no
 *     HIP include); nothing synchronises, nothing allocates device memory.
 *   - Activations inside the engine are NHWC (channels last); the public tensors keep the reference's
 *     NCHW fp32 layout so the Python modules stay drop-in.
 */
#ifndef K22_H
#define K22_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define K22_OK 0
#define K22_EINVAL (-1)
#define K22_EHIP (-2)
#define K22_ENOMEM (-3)

#define K22_BF16 0 /* product path: bf16 storage, v_mfma_f32_32x32x16_bf16, fp32 accumulate */
#define K22_F32 1  /* parity path : fp32 storage, v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain) */
#define K22_F16 2  /* the reference's own reduced-precision mode (use_fp16 / convert_to_fp16, kandinsky2/model/unet.py:409, 566-572):
                      fp16 storage, v_mfma_f32_32x32x16_f16, fp32 accumulate - bf16's speed and bytes, 3 more mantissa bits */
#define K22_F16X3 3 /* UNet engine only - SPLIT PRECISION, the arithmetic that holds BASELINE.json's 1e-3 final-latent gate against the
                      reference p_sampler (kandinsky2/kandinsky2_1_model.py:245-257 -> kandinsky2/model/gaussian_diffusion.py:384-475) at
                      16-bit MFMA rate: tensors stay fp32, every MFMA operand x is carried as the fp16 pair hi = rne(x), lo = rne(x - hi)
                      and every product as three v_mfma_f32_32x32x16_f16 (hi.hi + hi.lo + lo.hi) into one fp32 accumulator: ~23
                      significand bits per operand at 3/16 of the exact-fp32 MFMA cost.  Operand format ("x3 chunks"): 4 bytes per
                      element, every aligned group of 8 consecutive K elements (32 bytes) stored as [hi0..hi7 | lo0..lo7] fp16
                      (csrc/common.h; round 6 - rounds 4-5 used groups of 4, [hi x4 | lo x4]); weights are packed so (pre-multiplied
                      by 2^8) by pack.py / k22_x3_pack, activations by their producers. */
#define K22_F16X2 4 /* UNet engine only - the ASYMMETRIC SPLIT (round 5): the tensors, the arena and the operand formats of K22_F16X3, with
                      the precision of every MFMA op a property of the PLAN: weights always as (hi, lo) pairs (their rounding is the
                      systematic error of a 16-bit engine), the activation operand at fp16 precision - two MFMAs per product,
                      w_hi.a_hi + w_lo.a_hi - where the operand-rounding ablation (oracle/drift_ablation.py, tests/golden/
                      drift_ablation_x2.json) prices it as cheap: the 3x3 convolutions below the top resolution level and the qkv
                      projections; ONE MFMA (fp16 tiles, fp32 softmax) in the attention; all three where it is not: 1x1 skip
                      connections, the out head, proj_out / encoder_kv, and (default plan; env K22_X2_PLAN bits 0 / 1 release its
                      in_layers / out_layers convolutions) the top level.  C2 final latent 2.2e-4 from the reference p_sampler
                      (gate 1e-3; round 6) at 1.20x the K22_F16X3 engine's speed.  The kernel-level entries accept it: k22_conv3x3* / k22_gemm* /
                      k22_qkv_project = two MFMAs, activation operand rounded to fp16 (a fused skip keeps three); k22_attention = fp16
                      tiles on fp32 tensors. */

int k22_version(void);
/* Build flavour of this library: bit mask of K22_BUILD_*.  0 = the shipped form. */
#define K22_BUILD_PACKED_FP32 1     /* built with NOPK=0: packed-fp32 VALU instructions present - do NOT overlap two handles on one device */
int k22_build_flags(void);
const char* k22_last_error(void);
/* Tuning knobs.  PROCESS-WIDE MUTABLE STATE, NOT RE-ENTRANT: these exist for the kernel-level test / measurement surface (k22_gemm,
 * k22_conv3x3*, k22_groupnorm) and must not be changed while another thread is inside any k22_* call.  Leave them at their defaults
 * in a process that runs engines (k22_unet_*, k22_prior_*, k22_movq_*, k22_encoder_*): engine launches carry the configuration of their
 * tile-table line, but a line that says "generic kernel" (algo 0) is dispatched through the same switch these knobs override.
 * Everything else in this header is re-entrant per handle (one handle = one stream at a time), and handles may run CONCURRENTLY on
 * different streams of one device: since round 6 the library is built without packed-fp32 VALU instructions (csrc/Makefile NOPK = 1), the
 * instruction class behind the one wrong-result kernel pair rounds 4-5 found under concurrency (0 of 900 victim launches wrong with every
 * offender, against 148-227 of 900 in a packed build on the same box: profiles/r06_two_stream_probe.txt).  k22_build_flags() lets a
 * host assert it: a library built with NOPK=0 reports K22_BUILD_PACKED_FP32 and must be driven one stream at a time.
 * Knobs: "igemm_stages" = 2..4 LDS-DMA pipeline depth (-1 default; with "gemm_algo" = 10: 2 = two workgroups per CU at BM = 128, 3 / 4 = the
 * specialised, pipelined gemm8_spec_kernel for the 16-bit types and its two-per-CU form - same bits as the lock-step kernel);
 * "igemm_xcd_remap" = 0/1 XCD-aware workgroup renumbering; "conv_algo" = 0 auto, 1 generic implicit GEMM,
 * 2 LDS-resident halo kernel for the 3x3 convolutions (3, 6, 7, 11, 12: its variants, see conv3_halo.hip / conv3_spec.hip; 8, 9, 13, 14 are reserved numbers that no kernel answers to: auto);
 * "gemm_algo" = 0 generic implicit-GEMM kernel, 10 = 8-wave BM x 128 tile kernel where it applies;
 * "conv_algo" / "gemm_algo" = 20: the weight-streaming small-M kernel (stream_gemm.hip; bm = 160 / 288 picks 5 / 9 m-blocks
 * per workgroup, needs the fp32 partial buffer also for splitk == 1);
 * "att_pipe" = -1 as K22_ATT_PIPE says (default), 0 / 1: the unmasked 16-bit attention through attention_kernel / attention_pipe_kernel. */
int k22_set_option(const char* name, int value);
/* Host counters for tests, since the library was loaded: "stream_launches" = launches of the weight-streaming kernel;
 * "loop_captures" = whole-loop graphs captured by any loop entry (k22_unet_sample_loop[_keep], k22_unet_ddim_loop, k22_unet_dpmpp_loop[_keep], k22_prior_sample_loop); "loop_launches" = whole-loop
 * replays or eager loop runs.  -1 for an unknown name. */
long k22_debug_counter(const char* name);
/* Fragment-major copy of a 16-bit weight matrix [Npad][taps * Kc] for the weight-streaming kernel (1 KB contiguous per MFMA B
 * fragment; layout in stream_gemm.hip).  k22_stream_frag_bytes = size of the copy (0 for fp32: the kernel is 16-bit only).
 * k22_debug_set_stream_frag hands the copies (main weights, fused-skip weights or NULL) to the kernel-level test entries below
 * until reset with NULLs; the engines keep their own copies and never read it. */
size_t k22_stream_frag_bytes(int Npad, int taps, int Kc, int dtype);
int k22_stream_repack(const void* W, void* out, int Npad, int taps, int Kc, int dtype, void* stream);
int k22_debug_set_stream_frag(const void* wfrag, const void* wsfrag);
/* Parity-test mode: with a scratch buffer set (and no explicit copies), every kernel-level test entry repacks its weights into the
 * scratch on `stream` before the launch, so the tests' own packing helpers exercise the fragment-major path unchanged.  NULL resets. */
int k22_debug_set_stream_scratch(void* scratch, size_t bytes);

/* ---- UNet engine --------------------------------------------------------------------------
 * Replaces Text2ImUNet.forward / InpaintText2ImUNet.forward (kandinsky2/model/text2im_model2_1.py:
 * 85-103, 146-155) and everything below it: UNetModel blocks (kandinsky2/model/unet.py:343-611),
 * ResBlock (:110-220), AttentionBlock/QKVAttention (:223-340), GroupNorm32 (kandinsky2/model/nn.py:
 * 26-37), timestep_embedding (nn.py:101-121).  Hyper-parameters mirror create_model()
 * (kandinsky2/model/model_creation.py:9-83) / CONFIG_2_1["model_config"] (kandinsky2/configs.py:125-149).
 */
typedef struct K22UNetConfig {
  int dtype;               /* K22_BF16 | K22_F32 | K22_F16 | K22_F16X3 | K22_F16X2 */
  int in_channels;         /* 4; 9 for the inpainting UNet (x, image*mask, mask); 8 for the 2.2 ControlNet-depth UNet (x, hint latent) */
  int model_channels;      /* 384 */
  int out_channels;        /* 8 = eps + learned variance */
  int num_res_blocks;      /* 3 */
  int n_levels;            /* len(channel_mult) */
  int channel_mult[8];     /* (1,2,3,4) */
  int n_attention_ds;      /* attention at these downsample rates */
  int attention_ds[8];     /* (2,4,8) */
  int num_head_channels;   /* 64 (only 64 is implemented) */
  int ctx_dim;             /* model_dim / encoder_channels, 768 */
  int ctx_len;             /* num_image_embs + text_ctx = 10 + 77 */
  int n_image_embs;        /* 10 */
  int text_dim1;           /* text_encoder_in_dim1, 1024 */
  int text_dim2;           /* text_encoder_in_dim2, 768 (pooled) */
  int image_dim;           /* image_encoder_in_dim, 768 (2.2: CLIP-bigG image embedding, 1280) */
  int head_type;           /* 0: Kandinsky 2.1 head (Text2ImUNet.get_text_emb: 10 image tokens + 77 text tokens,
                            *    text2im_model2_1.py:57-80);
                            * 1: Kandinsky 2.2 head (image-only: ctx = LayerNorm(Linear(image_emb)) as ctx_len tokens, additive
                            *    time term LayerNorm(Linear(image_emb)): the UNet2DConditionModel the reference injects,
                            *    kandinsky2_2_model.py:26-41) */
  int hint_channels;       /* 0, or 3: ControlNet-depth variant of the 2.2 UNet (hint image through the input_hint_block conv
                            *    stack, concatenated to the latent: in_channels 8; notebooks/kandinsky2_2_controlnet.ipynb:9235) */
} K22UNetConfig;

/* One packed parameter tensor inside the caller's weight arena (see kandinsky-2_amd/pack.py for the
 * layouts; names follow the reference state_dict keys so reference checkpoints load). */
typedef struct K22Weight {
  const char* name;
  const void* ptr;
} K22Weight;

typedef struct K22UNet K22UNet; /* opaque */

/* Builds the op graph description.  `weights` pointers must stay valid for the engine's lifetime. */
int k22_unet_create(const K22UNetConfig* cfg, const K22Weight* weights, int n_weights, K22UNet** out);
void k22_unet_destroy(K22UNet* u);

/* Life cycle of every engine handle (K22UNet, K22MoVQ, K22Prior, K22Encoder):  create -> plan -> bind -> run.
 * k22_*_plan sizes the workspace for one shape and returns its size.  Arguments it rejects leave the previous plan (and its
 * binding) in place; a plan that fails later (a weight name missing from the table) leaves the handle WITHOUT a plan: bind
 * then answers "plan first" and the run entries "bind a workspace first".  A successful plan drops the previous binding.
 * k22_*_bind attaches a caller-owned workspace of at least that size, 256-byte aligned; it may be called again to move the
 * same plan to another workspace.  Binding invalidates what was cached for the previous workspace (captured graphs, the
 * UNet's conditioning / hint, per-binding weight copies).  The workspace stays the caller's: it must outlive its use and
 * may be freed after a re-plan or re-bind once the stream has drained. */

/* Plans a forward for batch B (= 2*bs with classifier-free guidance) and latent H x W; returns the
 * workspace size the caller must provide to k22_unet_bind().  Re-planning invalidates the binding. */
int k22_unet_plan(K22UNet* u, int B, int H, int W, size_t* workspace_bytes);
int k22_unet_bind(K22UNet* u, void* workspace, size_t workspace_bytes);

/* Conditioning head, once per generation: Text2ImUNet.get_text_emb (text2im_model2_1.py:57-80) plus
 * the step-invariant AttentionBlock.encoder_kv projections (unet.py:263-264).
 * full_emb [B,77,text_dim1], pooled_emb [B,text_dim2], image_emb [B,image_dim], all fp32 contiguous. */
int k22_unet_set_condition(K22UNet* u, const float* full_emb, const float* pooled_emb, const float* image_emb,
                           void* stream);

/* ControlNet-depth variant only (hint_channels == 3), once per generation after k22_unet_bind: hint [B,3,8H,8W] fp32 NCHW
 * (the depth map in [0,1]) -> input_hint_block -> [B,4,H,W], kept in the workspace and concatenated to x by every forward. */
int k22_unet_set_hint(K22UNet* u, const float* hint, void* stream);

/* One UNet evaluation.  x [B,4,H,W] fp32 NCHW, timesteps [B] fp32 (already mapped/rescaled exactly as
 * _WrappedModel.__call__ does, kandinsky2/model/respace.py:128-133), inpaint_image [B,4,H,W] and
 * inpaint_mask [B,1,H,W] (NULL unless in_channels == 9; the product image*mask is formed inside like
 * text2im_model2_1.py:151), out [B,out_channels,H,W] fp32 NCHW.
 * use_graph != 0 replays a captured hipGraph of the whole forward (captured on first use). */
int k22_unet_forward(K22UNet* u, const float* x, const float* timesteps, const float* inpaint_image,
                     const float* inpaint_mask, float* out, int use_graph, void* stream);

/* Number of engine ops in one planned forward (diagnostics). */
/* The whole classifier-free-guided p_sampler loop of Kandinsky2_1.generate_img (kandinsky2/kandinsky2_1_model.py:222-257 driving
 * kandinsky2/model/gaussian_diffusion.py:384-475) as ONE hipGraph replay: per step  UNet([x_half | x_half], timesteps[k]) ->
 * k22_sampler_step(guidance, clamp, percentile threshold, posterior mean, noise_seq[k])  with no host work between steps.
 * Device buffers, filled by the caller before the call: x [B][4][HW] (in: x_T, out: the final latent; x_tmp: same-size scratch),
 * timesteps [n_steps][B] in execution order, noise_seq [n_steps][B][4][HW], init_img / mask (inpainting blend of the sampler step, or
 * NULL), inpaint_image / inpaint_mask (9-channel UNet inputs, or NULL), table [T][8]; table_rows: HOST array, schedule row of step k.
 * use_graph != 0: captured on first use and replayed while the same buffers / scalars are passed.
 * The time embedding, time_embed MLP and FiLM vectors (unet.py:159-170) of ALL n_steps are computed by batched launches before the first
 * step (the handle keeps an [n_steps * B] x FiLM-width device buffer for them); every row is the arithmetic of the per-step launch, so the
 * loop equals n_steps calls of k22_unet_forward + k22_sampler_step bit for bit (env K22_HOIST_TIME=0: per-step launches, measurement only). */
int k22_unet_sample_loop(K22UNet* u, float* x, float* x_tmp, const float* timesteps, const float* noise_seq, const float* init_img,
                         const float* mask, const float* inpaint_image, const float* inpaint_mask, const float* table,
                         const int* table_rows, int n_steps, float guidance, float clamp_lo, float clamp_hi, int pct_index,
                         double pct_gamma, void* scratch, int use_graph, void* stream);
/* k22_unet_sample_loop with one more stage per step: the known region of the Kandinsky 2.2 inpainting pipeline (diffusers
 * KandinskyV22InpaintPipeline loop, used by kandinsky2/kandinsky2_2_model.py:150-173) is re-imposed on the freshly written latent,
 *   per step k:  UNet([x_half | x_half], timesteps[k]) -> k22_sampler_step -> k22_keep_region(sa, sb = keep_coef[k])
 * as one chain on the capture stream.  keep_init [4][HW], keep_mask [HW] (image 0's, 1 = keep) and keep_noise [B / 2][4][HW] (each
 * sample's own initial noise) are device buffers; keep_coef [n_steps][2] is a HOST array: row k = (sqrt(alphas_cumprod[t_{k+1}]),
 * sqrt(1 - alphas_cumprod[t_{k+1}])), the last row (1, 0).  pct_index = -1 switches the percentile threshold off (DDPMScheduler does
 * not threshold).  The engine's ONE cached loop serves this entry too: its key holds a kind of its own, the three keep pointers and the
 * bits of every keep_coef value besides k22_unet_sample_loop's; use_graph = 0 issues the same launches eagerly; both count into
 * k22_debug_counter("loop_captures" / "loop_launches").  With all four keep arguments NULL it IS k22_unet_sample_loop (same kind, same key).
 * K22_EINVAL (with a k22_last_error text) for keep arguments given only in part, an odd B, missing 9-channel operands on the inpainting
 * UNet, and whatever else k22_unet_sample_loop refuses; a refused call leaves the handle and its captured loop as they were. */
int k22_unet_sample_loop_keep(K22UNet* u, float* x, float* x_tmp, const float* timesteps, const float* noise_seq, const float* init_img,
                              const float* mask, const float* inpaint_image, const float* inpaint_mask, const float* table,
                              const int* table_rows, int n_steps, float guidance, float clamp_lo, float clamp_hi, int pct_index,
                              double pct_gamma, void* scratch, const float* keep_init, const float* keep_noise, const float* keep_mask,
                              const float* keep_coef, int use_graph, void* stream);
/* The threshold group of the sampler steps of k22_unet_sample_loop and k22_unet_sample_loop_keep (pct_group of k22_sampler_step_groups):
 * rows of the cond half that share the percentile of their first row.  0, the default, is the whole batch from element 0 - the loop as it
 * has always run.  The loop entries read it when they build their steps and check it there against the planned B (it must divide B / 2
 * into at most 64 groups; K22_EINVAL from the loop entry otherwise, which leaves the handle and its captured loop as they were).  It is a
 * word of the captured loop's key: another value re-captures, the same value replays.  K22_EINVAL here for a null handle and rows < 0. */
int k22_unet_set_threshold_group(K22UNet* u, int rows);
/* The whole classifier-free-guided DDIM or PLMS loop - generate_img's default sampler and its documented alternative - as ONE hipGraph
 * replay (kandinsky2/kandinsky2_1_model.py:222-233, the non-p_sampler model_fn, driving kandinsky2/model/samplers.py:206-331 for
 * kind = K22_LOOP_DDIM and samplers.py:475-637 for kind = K22_LOOP_PLMS): per step  UNet([x_half | x_half], t) -> k22_ddim_step or
 * k22_plms_step on all B rows (use_cfg = 1)  with no host work between steps.  It shares k22_unet_sample_loop's machinery: the time /
 * FiLM rows of every model call are computed before the first step, the engine keeps ONE captured loop whose key holds the kind and every
 * pointer / scalar below (a loop of another kind, or other buffers, re-captures), and the result equals the stepwise calls bit for bit -
 * also with use_graph = 0 (the same launches, eagerly) and under K22_HOIST_TIME=0.
 * Device buffers, filled by the caller before the call:
 *   x [B][4][HW]: in x_T, out the final latent;  x_tmp: same-size scratch;  x0_out [B][4][HW] or NULL: the predicted x0 of the last step;
 *   timesteps [n_calls][B]: the raw DDIM timestep (1 .. 981) of every MODEL CALL in execution order.  n_calls = n_steps for DDIM and
 *     n_steps + 1 for PLMS, whose first step calls the model twice - the second time at the next step's timestep (at its own when
 *     n_steps == 1): rows = t_0, t_1 (or t_0), t_1, t_2, ...;
 *   table [n_steps][4]: the k22_ddim_step rows (a_t, a_prev, sigma_t, sqrt(1 - a_t)) in execution order;
 *   noise_seq [n_steps][B][4][HW], or NULL for eta = 0; DDIM only (PLMS with noise is K22_EINVAL: the reference asserts eta = 0);
 *   inpaint_image / inpaint_mask: 9-channel UNet inputs (required for it), else NULL;
 *   eps_hist: PLMS only, 4 x [B][4][HW] floats - the ring of guided eps tensors.  Its rotation is resolved on the host when the loop is
 *     captured: orders 0 and 4 are the pseudo improved-Euler start, orders 1, 2, 3 follow (see k22_plms_step).
 * K22_EINVAL (with a k22_last_error text) for a null argument, an odd B, n_steps < 1, a missing condition / hint or missing inpaint
 * operands; a refused call leaves the handle and its captured loop as they were. */
enum { K22_LOOP_DDIM = 0, K22_LOOP_PLMS = 1 };
int k22_unet_ddim_loop(K22UNet* u, int kind, float* x, float* x_tmp, float* x0_out, const float* timesteps, const float* table,
                       const float* noise_seq, const float* inpaint_image, const float* inpaint_mask, float* eps_hist, int n_steps,
                       float guidance, int use_graph, void* stream);
/* The whole classifier-free-guided DPM-Solver++ loop (multistep, data-prediction form, orders 1 and 2M; Lu et al. 2022 - the reference has
 * no such sampler) as ONE hipGraph replay: per step  UNet([x_half | x_half], t) -> k22_dpmpp_step on all B rows (use_cfg = 1).  The
 * machinery, the counters and the guarantees are k22_unet_ddim_loop's: one captured loop per engine, equal bits with the stepwise calls,
 * also with use_graph = 0 and under K22_HOIST_TIME=0.  Device buffers, filled by the caller before the call:
 *   x [B][4][HW]: in x_T, out the final latent;  x_tmp: same-size scratch;
 *   x0_hist: 2 x [B][4][HW] floats.  Step k writes its data prediction to slot k % 2 and reads slot (k - 1) % 2 when orders[k] == 2; after
 *     the call slot (n_steps - 1) % 2 holds the predicted x0 of the last step;
 *   timesteps [n_steps][B]: the raw integer timestep of every model call in execution order;
 *   table [n_steps][5]: the k22_dpmpp_step rows in execution order;
 *   inpaint_image / inpaint_mask: 9-channel UNet inputs (required for it), else NULL.
 * orders is a HOST array of n_steps ints (1 or 2, orders[0] = 1): which rows read the history is resolved when the loop is captured, and
 * every value is part of the captured loop's key (other orders re-capture).
 * K22_EINVAL (with a k22_last_error text) for a null argument, an odd B, n_steps < 1, an order outside {1, 2}, orders[0] != 1, a missing
 * condition / hint, missing inpaint operands or a UNet with out_channels != 8; a refused call leaves the handle and its captured loop as
 * they were. */
int k22_unet_dpmpp_loop(K22UNet* u, float* x, float* x_tmp, float* x0_hist, const float* timesteps, const float* table, const int* orders,
                        const float* inpaint_image, const float* inpaint_mask, int n_steps, float guidance, int use_graph, void* stream);
/* k22_unet_dpmpp_loop for the Kandinsky 2.2 decoders, whose scheduler configs can carry clip_sample and whose inpainting pipeline re-imposes
 * the known region after every step:
 *   per step k:  UNet([x_half | x_half], timesteps[k]) -> k22_dpmpp_step_clip(clamp_lo, clamp_hi) [-> k22_keep_region(sa, sb = keep_coef[k])]
 * as one chain on the capture stream.  "No clip" is the DDPM route's convention, (-3.0e38, 3.0e38).  The keep operands are all four or none
 * and mean what they mean in k22_unet_sample_loop_keep: keep_init [4][HW], keep_mask [HW] (image 0's, 1 = keep), keep_noise [B / 2][4][HW]
 * device buffers, keep_coef [n_steps][2] a HOST array (kandinsky2_amd.sampling.dpmpp_keep_coef: the target point's (sqrt(ac), sqrt(1 - ac)),
 * the last row (1, 0)).  Everything else is k22_unet_dpmpp_loop's.  The engine's ONE cached loop serves this entry too: its key holds a
 * kind of its own (another one when keep is on), the clamp bits, the three keep pointers and the bits of every keep_coef value besides
 * k22_unet_dpmpp_loop's; use_graph = 0 issues the same launches eagerly.
 * K22_EINVAL (with a k22_last_error text) for keep arguments given only in part, clamp_lo > clamp_hi or a NaN bound, and whatever
 * k22_unet_dpmpp_loop refuses; a refused call leaves the handle and its captured loop as they were. */
int k22_unet_dpmpp_loop_keep(K22UNet* u, float* x, float* x_tmp, float* x0_hist, const float* timesteps, const float* table, const int* orders,
                             const float* inpaint_image, const float* inpaint_mask, int n_steps, float guidance, float clamp_lo, float clamp_hi,
                             const float* keep_init, const float* keep_noise, const float* keep_mask, const float* keep_coef,
                             int use_graph, void* stream);
int k22_unet_num_ops(const K22UNet* u);
/* Tile configurations of the convolutions / GEMMs are chosen by measurement during the first k22_unet_forward
 * after k22_unet_plan (default on; env K22_AUTOTUNE=0 or k22_unet_set_autotune(u, 0) before planning = heuristics).
 * k22_unet_tuning_report writes a text table of the choices into buf. */
int k22_unet_set_autotune(K22UNet* u, int on);
int k22_unet_tuning_report(const K22UNet* u, char* buf, size_t cap);

/* Multi-GPU: one process per GPU, prompts sharded by rank, the packed weight arena of rank `root` broadcast ONCE
 * at start-up over the caller's RCCL communicator (ncclComm_t passed as void*), in <= 1 GiB pieces on `stream`; no collective
 * in the step loop.  Replaces nothing in the reference (it has no inference parallelism); mirrors what
 * kandinsky2_amd.parallel.broadcast_arena does through torch.distributed for hosts that own their communicator. */
int k22_comm_broadcast_weights(void* arena, size_t bytes, int root, void* nccl_comm, void* stream);

/* Tile table: the process-wide map  conv / GEMM problem -> tile configuration  that every engine consults BEFORE it
 * measures anything (csrc/tuning.h).  The package ships kandinsky-2_amd/tiles_gfx950.txt (measured on an MI355X for the
 * shapes of BASELINE.json's configs); the Python binding loads it when the library is opened, so those shapes get the
 * same configurations, and therefore the same bits, on every box.  Problems outside the table are measured on the
 * device at the first forward (K22_AUTOTUNE=0: fixed heuristic instead) and remembered for the life of the process;
 * env K22_TUNE_CACHE=<file> persists them.  load / save return the number of lines (< 0 = error), size the number of
 * entries, measured the number of entries this process timed itself. */
int k22_tile_table_load(const char* path);
int k22_tile_table_save(const char* path);
int k22_tile_table_size(void);
int k22_tile_table_measured(void);
void k22_tile_table_clear(void);

/* Measurement aid for bench.py: replays the planned forward EAGERLY `reps` times on `stream` with a HIP
 * event pair around every op, and reports per op class k (0 conv3x3, 1 GEMM, 2 GroupNorm, 3 attention,
 * 4 other): ms[k] = average summed device time per forward, flops[k]/bytes[k] = algorithmic work per
 * forward, launches[k] = kernel launches per forward.  Synchronises the stream (not a hot-path call). */
int k22_unet_profile(K22UNet* u, int reps, double* ms, double* flops, double* bytes, int* launches, void* stream);

/* ---- sampler step ---------------------------------------------------------------------------
 * Replaces one iteration of GaussianDiffusion.p_sample_loop_progressive
 * (kandinsky2/model/gaussian_diffusion.py:463-475): the CFG combine of Kandinsky2_1.generate_img.model_fn
 * (kandinsky2/kandinsky2_1_model.py:222-233) applied to the raw UNet output, p_mean_variance
 * (gaussian_diffusion.py:223-322) including the host-side np.percentile dynamic threshold
 * (:284-294, done on device here) and p_sample (:352-382).
 *   x, noise, x_out, x0_out(nullable): [N,4,H,W] fp32;  model_out: [N,8,H,W] fp32 (raw UNet output);
 *   init_img [N,4,H,W] / mask [N,1,H,W]: inpainting blend of denoised_fun (kandinsky2_1_model.py:238-240)
 *   or NULL;  table: device [steps][8] fp32 (see k22_sampler_table_columns); step_index selects the row;
 *   pct_index / pct_gamma: order-statistic index and weight of the 99.5 percentile (host computes them
 *   with numpy's own formula), pct_index < 0 disables thresholding (clip_denoised=False);
 *   scratch: device, >= k22_sampler_scratch_bytes(N,HW).
 */
size_t k22_sampler_scratch_bytes(int N, int HW);
/* DDIM step (DDIMSampler.p_sample_ddim, kandinsky2/model/samplers.py:290-331) with model_fn's guidance folded in:
 * e = u + g (c - u) on channels 0-3 of model_out [N][8][HW]; x0 = (x - sqrt(1-a_t) e) / sqrt(a_t);
 * x_out = sqrt(a_prev) x0 + sqrt(1 - a_prev - sigma^2) e + sigma * noise.   table_row: device fp32[4] =
 * (a_t, a_prev, sigma_t, sqrt(1 - a_t)); noise may be NULL (eta = 0); x0_out may be NULL. */
int k22_ddim_step(const float* x, const float* model_out, const float* noise, const float* table_row, float guidance, int use_cfg,
                  float* x_out, float* x0_out, int N, int HW, void* stream);
/* Inpainting mask pre-step (prepare_mask, kandinsky2/utils.py:11-31, an O(h*w) Python loop in the reference): every pixel
 * whose ORIGINAL value is not 1 zeroes its up / left / up-left / down / right / down-right neighbours.  mask, out: device fp32
 * [C][H][W], out of place (channel 0 decides, every channel is written). */
int k22_prepare_mask(const float* mask, float* out, int C, int H, int W, void* stream);
/* DPM-Solver++ step (multistep, data-prediction form; Lu et al. 2022, "DPM-Solver++", eq. of Algorithm 2 at orders 1 and 2) with the same
 * guidance fold as k22_ddim_step: e = u + g (c - u) on channels 0-3 of model_out [N][8][HW];
 *   x0 = (x - sigma_s e) / alpha_s;      x_out = c_x x + c_0 x0 + c_1 x0_prev      (the last term only when x0_prev != NULL)
 * table_row: device fp32[5] = (alpha_s, sigma_s, c_x, c_0, c_1), the float64 coefficients of kandinsky2_amd.sampling.dpmpp_table rounded
 * once.  x0_out (required) receives x0: the next step's x0_prev.  Every operation is rounded once.  Out of place: x, x_out, x0_out and
 * x0_prev are distinct buffers (K22_EINVAL otherwise, and for a null argument or an odd N with use_cfg). */
int k22_dpmpp_step(const float* x, const float* model_out, const float* x0_prev, const float* table_row, float guidance, int use_cfg,
                   float* x_out, float* x0_out, int N, int HW, void* stream);
/* k22_dpmpp_step with one more operation after the division: x0 = clamp(x0, clamp_lo, clamp_hi) - diffusers DDPMScheduler's clip_sample on
 * the data prediction.  The clamped value is what enters x_out and what x0_out stores (the next step's history).  The clamp is exact (two
 * comparisons, a NaN passes through); with (-3.0e38, 3.0e38) the outputs are k22_dpmpp_step's bit for bit.  K22_EINVAL for what
 * k22_dpmpp_step refuses, clamp_lo > clamp_hi and a NaN bound. */
int k22_dpmpp_step_clip(const float* x, const float* model_out, const float* x0_prev, const float* table_row, float guidance, int use_cfg,
                        float clamp_lo, float clamp_hi, float* x_out, float* x0_out, int N, int HW, void* stream);
/* PLMS step (PLMSSampler.p_sample_plms, kandinsky2/model/samplers.py:566-637; eta = 0) with model_fn's guidance folded in:
 * e_t = u + g (c - u) of this model call; e' = Adams-Bashforth combination of e_t and the eps history by `order`
 * (0: e_t; 1: (3 e_t - h1)/2; 2: (23 e_t - 16 h1 + 5 h2)/12; 3: (55 e_t - 59 h1 + 37 h2 - 9 h3)/24; 4: (h1 + e_t)/2, the second
 * stage of the pseudo improved Euler start); x_out = DDIM update (sigma = 0) with e'.  eps_out (optional, [N][4][HW])
 * receives e_t for the caller's history ring; table_row as for k22_ddim_step. */
int k22_plms_step(const float* x, const float* model_out, const float* eps_hist1, const float* eps_hist2, const float* eps_hist3, int order,
                  const float* table_row, float guidance, int use_cfg, float* x_out, float* eps_out, float* x0_out, int N, int HW, void* stream);
int k22_sampler_step(const float* x, const float* model_out, const float* noise, const float* init_img,
                     const float* mask, const float* table, int step_index, float guidance, int use_cfg,
                     float clamp_lo, float clamp_hi, int pct_index, double pct_gamma, void* scratch,
                     float* x_out, float* x0_out, int N, int HW, void* stream);
/* k22_sampler_step with the dynamic threshold taken per GROUP of rows: several prompts packed into one CFG batch, each clamped by the
 * percentile of its own image, as separate reference calls would clamp them.  half = use_cfg ? N / 2 : N.  Group j is rows
 * j * pct_group .. (j + 1) * pct_group - 1 of the cond half together with their uncond partners: s_j = max(percentile_99.5(|x0[j * pct_group]|), 1),
 * the order statistics and the float32 lerp of k22_sampler_step on that row, and every row n with (n % half) / pct_group == j is clamped to
 * +-s_j and divided by it.  The half / pct_group selects run as one launch, a workgroup each; s_j is float j of the scratch (floats
 * half / pct_group .. 63 are not written; the size of the scratch is unchanged).  pct_group == half is k22_sampler_step itself: the same
 * kernels, the same bits.  K22_EINVAL (with a k22_last_error text, nothing launched) for pct_group < 1, a pct_group that does not divide
 * half, more than 64 groups, and whatever k22_sampler_step refuses. */
int k22_sampler_step_groups(const float* x, const float* model_out, const float* noise, const float* init_img, const float* mask,
                            const float* table, int step_index, float guidance, int use_cfg, float clamp_lo, float clamp_hi, int pct_index,
                            double pct_gamma, int pct_group, void* scratch, float* x_out, float* x0_out, int N, int HW, void* stream);

/* ---- individual kernels (unit-parity surface; the engine calls the same launchers) -------------
 * dtype-typed buffers are bf16, fp16 or fp32 according to `dtype`.  Layouts: see the headers in kandinsky-2_amd/csrc. */
int k22_gemm(const void* A0, const void* A1, const void* Wp, const float* bias, const void* residual, void* out,
             void* partial, int M, int N, int Npad, int K0, int K1, long lda0, long lda1, int ldo, int ldr,
             int out_f32, int act, int splitk, int bm, int bn, int dtype, void* stream);
/* fp32 -> x3 chunks (K22_F16X3 operand format): dst[n] (4 bytes per element) from src[n] * scale, n % 8 == 0, src 16-byte and
 * dst 32-byte aligned (K22_EINVAL otherwise).
 * scale = 256 for weights (what pack.py writes and the epilogues undo), 1 for activations.  With dtype == K22_F16X3 the kernel-level
 * entries take: k22_gemm / k22_gemm_gnstats / k22_qkv_project - A as plain fp32 rows (split at fragment-read time), W in x3 chunks;
 * k22_conv3x3* - x_padded AND W in x3 chunks (in the engine the GroupNorm-apply kernel writes the input so: k22_groupnorm with
 * dtype == K22_F16X3 = fp32 in, x3 chunks out), the fused skip operands as plain fp32 rows; k22_attention - fp32 in and out.
 * Outputs, residuals and biases are fp32. */
int k22_x3_pack(const float* src, void* dst, long n, float scale, void* stream);
int k22_conv3x3(const void* x_padded, const void* Wp, const float* bias, const void* residual, void* out,
                void* partial, int B, int H, int W, int Cin, int Cout, int Npad, int out_mode, int act, int splitk,
                int bm, int bn, int dtype, void* stream);
/* Tail of a channel-changing ResBlock in one launch (unet.py:191,219-220): out = conv3x3(x_padded) + bias +
 * [skip0 | skip1](unpadded NHWC, SK0 + SK1 channels) . Ws[Npad][SK0+SK1]^T + bias_s   (1x1 skip_connection fused
 * as a second K loop of the halo kernel; skip1 may be null with SK1 = 0). */
int k22_conv3x3_skip(const void* x_padded, const void* Wp, const float* bias, const void* skip0, const void* skip1,
                     int SK0, int SK1, const void* Ws, const float* bias_s, void* out, void* partial, int B, int H, int W,
                     int Cin, int Cout, int Npad, int splitk, int bm, int dtype, void* stream);
/* Same convolution (row-major T output, no activation) that also emits the per-channel partial sums the next
 * GroupNorm needs (ResBlock: conv -> GroupNorm32, unet.py:157-164/212-216), so the tensor is not re-read:
 * stats[row][c] = (sum, sum of squares) of the STORED outputs, image b owning rows [b*rpi, (b+1)*rpi);
 * *rows_per_image receives rpi.  Fails (K22_EINVAL) for configurations that cannot produce them. */
int k22_conv3x3_gnstats(const void* x_padded, const void* Wp, const float* bias, const void* residual, void* out,
                        void* partial, int B, int H, int W, int Cin, int Cout, int Npad, int splitk, int bm, int bn,
                        float* stats, int stats_capacity_rows, int* rows_per_image, int dtype, void* stream);
/* Nearest 2x upsample + conv3x3 (in_layers of an up-sampling ResBlock, unet.py:158-159, 204) as four 2x2 convolutions of the LOW-resolution
 * tensor, one per output phase (py, px): x_padded = [B][H+2][W+2][Cin] zero-bordered low-resolution input, Wph = the folded weights
 * [phase 2*py+px][Npad][tap 2x2][Cin] in the engine type (k22_up2_fold, rounded once), out = the unpadded row-major [B][2H][2W][Cout].
 * splitk: 0 = the fixed rule, else as given (partial: fp32 [splitk][B*4HW][Cout]); bm: 0 = rule, 256, 128.  stats (optional, may be
 * null): the GroupNorm partial sums of the stored output, image b owning rows [b*rpi, (b+1)*rpi); *rows_per_image receives rpi. */
int k22_conv3x3_up2(const void* x_padded, const void* Wph, const float* bias, void* out, void* partial, int B, int H, int W, int Cin,
                    int Cout, int Npad, int splitk, int bm, float* stats, int stats_capacity_rows, int* rows_per_image, int dtype,
                    void* stream);
/* The fold itself: w = fp32 3x3 weights in pack order [O][ky][kx][I] -> out = fp32 phase weights [4][Opad][2][2][I] (rows O .. Opad-1
 * zero).  Phase py takes tap ky into row slot (py + ky + 1) / 2 - py (py = 0: {0 | 1, 2}; py = 1: {0, 1 | 2}), columns alike; the sums
 * run in fp32, ky then kx ascending.  The caller rounds / splits to the engine type afterwards, once. */
int k22_up2_fold(const float* w, float* out, int O, int Opad, int I, void* stream);
/* Same for a 1x1 convolution over unpadded rows [B*H*W][K] (AttentionBlock proj_out, unet.py:244-268, whose output the
 * next ResBlock's GroupNorm32 normalises): out = A W^T + bias (+ residual) through the 8-wave BM x 128 GEMM kernel
 * (bm = 256 / 128 / 0 = auto), with the per-tile (sum, sum of squares) rows as above. */
int k22_gemm_gnstats(const void* A, const void* Wp, const float* bias, const void* residual, void* out, void* partial,
                     int B, int H, int W, int N, int Npad, int K, int splitk, int bm, float* stats,
                     int stats_capacity_rows, int* rows_per_image, int dtype, void* stream);
/* One launch_igemm problem in full, as the engines hand it to the tile table (csrc/tuning.h), plus one explicit tile configuration: the
 * unit-parity surface of the SHIPPED table (tiles_gfx950.txt), whose every line is `dtype taps M N Kc K0 H W outmode stats | algo bm bn
 * splitk stages`.  Key fields as the table spells them, with the packed ones taken apart: K0 is the width of A0 alone (the table adds
 * 100000 * (SK0 + SK1) for a fused skip), out_mode is 0 = T rows, 1 = fp32 rows, 2 = NCHW fp32, 3 = the qkv projection of
 * k22_qkv_project (the table adds 16 * res_f32 + 32 * act + 256 * a_raw).
 * H = W = 0: a GEMM whose rows are not image shaped.  ldo / ldr = 0: the engines' defaults (N; N / 3 for the q rows of out_mode 3).
 * has_frag: the owner of the weights holds their fragment-major copy (k22_stream_repack) - the UNet engine's 16-bit 3x3 convolutions
 * with M <= 1152 only; it decides whether algo 20 is a candidate. */
typedef struct K22IgemmProblem {
  int dtype, taps, M, N, Kc, K0, H, W;
  int out_mode, res_f32, act, a_raw, want_stats;
  int SK0, SK1;                 /* fused 1x1 skip connection: channels of S0 / S1 (0, 0 = none) */
  int att_T, att_S, att_Tkp;    /* out_mode 3: tokens per image, context keys, padded key count */
  int ldo, ldr;
  int has_frag;
  int algo, bm, bn, splitk, stages;   /* the configuration (columns 11-15 of a table line) */
} K22IgemmProblem;
/* Device operands of k22_igemm_cfg, in the formats the engine of `dtype` holds them (k22_x3_pack's comment for the split arithmetics:
 * A0 / A1 in x3 chunks unless a_raw, S0 / S1 plain fp32 rows, weights in x3 chunks).  Null = absent (bias, residual, A1, S1, stats).
 * Wfrag / Wsfrag: fragment-major weights, required by algo 20 (Wsfrag when a skip is fused).  kall / vtall: out_mode 3 only. */
typedef struct K22IgemmOperands {
  const void *A0, *A1, *Wp, *bias, *residual;
  void *out, *partial;          /* partial: fp32 [splitk][M][N] (splitk > 1, and always for algo 20) */
  const void *S0, *S1, *Ws, *bias2;
  void *kall, *vtall;
  const void *Wfrag, *Wsfrag;
  float* stats;                 /* want_stats: [stats_capacity_rows][N][2] fp32 */
  int stats_capacity_rows;
} K22IgemmOperands;
/* Host only (no GPU call): does THIS build accept the configuration for the problem?  Builds the launch descriptor the engines build,
 * lists its candidates (tuned_make_candidates) and answers tuned_is_candidate: 1 = a table line with this key and configuration is
 * used as it stands, 0 = it is dropped silently and the problem is measured again on every start.  Negative: K22_EINVAL.
 * The ALL-ZERO configuration (algo = bm = bn = splitk = stages = 0) stands, here and in k22_igemm_cfg, for the fixed choice: what
 * tuned_default_cfg resolves for the problem - the table's line where one exists, else the heuristic an engine runs under K22_AUTOTUNE=0 and,
 * whatever the setting, for M < 64, which the tuner never times.  Accepted unless the problem owes GroupNorm partial sums that choice cannot write, or no
 * kernel takes the problem at all. */
int k22_igemm_cfg_accepted(const K22IgemmProblem* pr);
/* Host only: the configurations tuned_make_candidates generates for the problem - everything tune_igemm_ops may time and keep - from the
 * same descriptor as above.  Writes the first `capacity` of them to `out` and returns their number (which may exceed capacity; 0 = the
 * problem has no candidates and always runs its fixed choice).  resolved (optional, [capacity]) receives the launch igemm_resolve makes of each:
 * kernel, tile, split-K factor and, in `stages`, the ring depth instantiated (halo kernels: conv3_halo_ring's, unless a shallower one was
 * asked for).  fixed (optional) receives the same for the all-zero configuration: its split-K factor says how large a partial buffer
 * (splitk * M * N fp32) that launch needs; all zero where k22_igemm_cfg_accepted answers 0 for it. */
typedef struct K22IgemmCfg { int algo, bm, bn, splitk, stages; } K22IgemmCfg;
int k22_igemm_candidates(const K22IgemmProblem* pr, K22IgemmCfg* out, int capacity, K22IgemmCfg* resolved, K22IgemmCfg* fixed);
/* Runs the problem ONCE with exactly that configuration, the way an engine's launch closure does (IgemmParams from the problem,
 * tuned_apply_cfg, launch_igemm); it needs and sets no process-wide option (k22_set_option).  A configuration k22_igemm_cfg_accepted rejects
 * is an error (K22_EINVAL), never a quiet run of another kernel.  With want_stats the GroupNorm partial sums land in ops->stats as in
 * k22_conv3x3_gnstats: image b owns rows [b * rpi, (b + 1) * rpi), *rows_per_image receives rpi (0 without want_stats). */
int k22_igemm_cfg(const K22IgemmProblem* pr, const K22IgemmOperands* ops, int* rows_per_image, void* stream);
int k22_groupnorm(const void* x0, const void* x1, int C0, int C1, int B, int H, int W, const float* gamma,
                  const float* beta, const float* film, long film_ld, float eps, int act, int mode, int pad,
                  void* scratch, void* out, int dtype, void* stream);
size_t k22_groupnorm_scratch_bytes(int B, int C);
int k22_attention(const void* qkv, const void* ctxkv, void* kall, void* vtall, void* out, int B, int H, int T, int S,
                  int dtype, void* stream);
/* qkv projection of an AttentionBlock (Conv1d C -> 3C, unet.py:251) written straight into the attention operands:
 * x [B*T][K], packed weight rows ordered [q | k | v] x [H][64]; q -> q_out [B*T][C]; k -> kall[b][h][S+t][64];
 * v -> vtall[b][h][d][S+t] (both [..][Tkp = roundup(S+T,64)]; the first S keys belong to the context). */
int k22_qkv_project(const void* x, const void* Wp, const float* bias, void* q_out, void* kall, void* vtall,
                    int B, int H, int T, int S, int K, int bm, int bn, int dtype, void* stream);
/* The same projection on the weight-streaming small-M kernel (unet.py:251 at the 12x12 / 24x24 levels): partial = fp32
 * scratch [splitk][B*T][3C]; bm = 160 / 288. */
int k22_qkv_project_stream(const void* x, const void* Wp, const float* bias, void* q_out, void* kall, void* vtall, void* partial,
                           int B, int H, int T, int S, int K, int bm, int splitk, int dtype, void* stream);
int k22_linear_smallm(const float* x, const void* W, const float* bias, const float* add, float* out, int M, int N,
                      int K, int act_in, int act_out, int wdtype, void* stream);
/* Direct fp32 3x3 convolution, pad 1, stride 1 or 2, optional SiLU (act 0 / 1): one layer of the ControlNet-depth hint stack of the 2.2
 * UNet (diffusers ImageHintTimeEmbedding.input_hint_block; the engine runs eight of them through the same launcher).  x [B][Cin][Hin][Win],
 * w [Cout][Cin][3][3], bias [Cout], y [B][Cout][Ho][Wo] with Ho = (Hin - 1) / stride + 1, Wo likewise; all fp32 NCHW. */
int k22_conv3x3_direct(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout, int Hin, int Win,
                       int stride, int act, void* stream);

/* ---- skinny-M weight-streaming GEMM family (round 6; csrc/skinny.hip) - unit-parity surface of the kernels the prior engine's
 * 16-bit path is made of.  Replaces nn.Linear c_qkv / c_proj / c_fc / mlp.c_proj (kandinsky2/model/prior.py:57-83), the LayerNorm in
 * front of each (prior.py:48-54, 105-127) and QKVMultiheadAttention (prior.py:86-102) for M = a few hundred token rows.  Both GEMM
 * operands are FRAGMENT-MAJOR (1 KB contiguous per 32-row x 16-k MFMA fragment): weights [Npad/32][K/64][4][64][8] written by
 * k22_stream_repack(W, out, Npad, 1, K, ...); activations [K/64][ceil(M/32)][4][64][8] written by k22_afrag_pack (row-major in), by
 * k22_finish_ln, by k22_skinny_gemm with epi = 1, or by k22_small_attention with out_frag = 1.  dtype: K22_BF16 / K22_F16.
 *   k22_skinny_gemm: epi 0 -> out[m*ldo + n] = act(A.W^T + bias) in T;  epi 1 -> the same values in the A-fragment order of a consumer
 *     whose K is this N;  epi 2 -> fp32 partial[z][m][n], z < splitk (no bias / activation);  (mt, nb) = m-atoms x n-atoms of 32 per
 *     workgroup, one of (6,1) (3,4) (3,2) (3,1) (2,2) (2,1) (1,2); 0,0 = default.  nb = 4 needs Npad % 128 == 0.
 *   k22_finish_ln: x[m][:] += bias + sum_z partial[z][m][:] (skipped when partial == NULL), then yfrag = LayerNorm(x[m][:]) * gain +
 *     beta in T, A-fragment order (skipped when gain == NULL).  N <= 2048, N % 8 == 0, and N % 64 == 0 where the LayerNorm output is
 *     written; 1 <= splitk <= 8 with partials.
 *   k22_small_attention: qkv [B*T][3*H*64] = [Q | K | V] x [H][64] row-major T -> softmax(q.k / 8 + mask) v, T <= 128 tokens;
 *     mask = causal (key <= query) and key_valid [B][kv_n] (0 = padding key; keys >= kv_n are valid), as prior.py:262-263.
 *     qkv_partial != NULL: qkv is instead T(qkv_bias + sum_s qkv_partial[s][B*T][3*H*64]), s < nsplit <= 4 - the finish of a split-K
 *     c_qkv launch (k22_skinny_gemm epi 2) folded into the attention's staging loads. */
size_t k22_afrag_bytes(int M, int K);
int k22_afrag_pack(const void* A, long lda, void* out, int M, int K, int dtype, void* stream);
int k22_skinny_gemm(const void* Afrag, const void* Wfrag, const float* bias, void* out, float* partial, int M, int N, int Npad, int K,
                    int splitk, int epi, int act, int ldo, int mt, int nb, int dtype, void* stream);
int k22_finish_ln(const float* partial, int splitk, const float* bias, float* x, long ldx, const float* gain, const float* beta, void* yfrag,
                  int M, int N, float eps, int dtype, void* stream);
int k22_small_attention(const void* qkv, const float* qkv_partial, int nsplit, const float* qkv_bias, void* out, int out_frag, int B, int H, int T,
                        int causal, const float* key_valid, int kv_n, int dtype, void* stream);

/* ---- diffusion prior ----------------------------------------------------------------------------
 * Replaces PriorTransformer.forward (kandinsky2/model/prior.py:226-270) and the per-step update of
 * PriorDiffusionModel.forward's sampling loop (prior.py:336-384; gaussian_diffusion.py:223-322, 352-382 with
 * model_mean_type START_X, model_var_type FIXED_SMALL, clip_denoised False, denoised_fn clamp(+-10)).
 * Hyper-parameters mirror CONFIG_2_1["prior"]["params"]["model"]["hparams"] (kandinsky2/configs.py:101-111).
 * Weight names are the reference state_dict keys of PriorDiffusionModel.model (time_embed.0.weight ...,
 * transformer.resblocks.<l>.attn.c_qkv.weight ...); transformer Linear weights packed T [roundup(N,64)][K] with
 * c_qkv rows re-ordered to Q | K | V planes x [head][64]; everything else fp32; plus "time_freqs" [xf_width/2]. */
typedef struct K22PriorConfig {
  int dtype;          /* K22_BF16 | K22_F32 | K22_F16 */
  int text_ctx;       /* 77 */
  int xf_width;       /* 2048 */
  int xf_layers;      /* 20 */
  int xf_heads;       /* 32 (64 channels per head) */
  int xf_final_ln;    /* 1 */
  int clip_dim;       /* 768 */
  int clip_xf_width;  /* 768 */
} K22PriorConfig;
typedef struct K22Prior K22Prior;
int k22_prior_create(const K22PriorConfig* cfg, const K22Weight* weights, int n_weights, K22Prior** out);
void k22_prior_destroy(K22Prior* m);
int k22_prior_plan(K22Prior* m, int B, size_t* workspace_bytes);   /* B = 2*bs rows [cond | uncond], <= 8 */
int k22_prior_bind(K22Prior* m, void* workspace, size_t workspace_bytes);
int k22_prior_tuning_report(const K22Prior* m, char* buf, size_t cap);  /* as k22_unet_tuning_report */
/* x [B][clip_dim], timesteps [B] (as the reference passes them: original indices as floats), text_emb [B][clip_dim],
 * text_enc [B][text_ctx][clip_xf_width], key_valid [B][text_ctx] (1 = token, 0 = padding; the `mask` argument of
 * the reference as floats) -> out [B][clip_dim]; all fp32 device buffers. */
int k22_prior_forward(K22Prior* m, const float* x, const float* timesteps, const float* text_emb, const float* text_enc,
                      const float* key_valid, float* out, void* stream);
/* One ancestral step: x0 = clamp(uncond + scales[j]*(cond - uncond), +-clamp); mean = c1*x0 + c2*x;
 * x_out = mean + nonzero*exp(0.5*logvar)*noise.  table_row: device fp32[4] = (posterior_mean_coef1, coef2,
 * posterior_log_variance_clipped, t != 0); x / model_out / noise / x_out: [2*bs][D]; scales [bs]. */
int k22_prior_sampler_step(const float* x, const float* model_out, const float* noise, const float* scales, const float* table_row,
                           float clamp, float* x_out, int bs, int D, void* stream);
/* One DDIM step (gaussian_diffusion.py:477-519 as the prior runs it: START_X, clip_denoised off, denoised_fn = clamp):
 *   x0 = clamp(uncond + scales[j]*(cond - uncond), +-clamp);  eps = (sqrt_recip_ac*x - x0) / sqrt_recipm1_ac;
 *   x_out = sqrt(ab_prev)*x0 + sqrt(1 - ab_prev - sigma^2)*eps + (i != 0)*sigma*noise.
 * table_row: device fp32[8] = (sqrt_recip_alphas_cumprod[i], sqrt_recipm1_alphas_cumprod[i], sqrt(alphas_cumprod_prev[i]), sigma,
 * sqrt(1 - alphas_cumprod_prev[i] - sigma^2), i != 0, 0, 0), computed in float64 and rounded once;
 * sigma = eta * sqrt((1 - ab_prev)/(1 - ab)) * sqrt(1 - ab/ab_prev).  Layout as k22_prior_sampler_step.  noise may be NULL and then reads
 * as 0: valid for an eta = 0 table only.  x0_out [2*bs][D] (the clamped guided prediction) may be NULL.  Every operation is rounded once
 * (no contraction).  K22_EINVAL for a null required argument or bs, D < 1. */
int k22_prior_ddim_step(const float* x, const float* model_out, const float* noise, const float* scales, const float* table_row,
                        float clamp, float* x_out, float* x0_out, int bs, int D, void* stream);
/* The whole sampling loop of PriorDiffusionModel.forward (prior.py:336-384) on a bound handle, B = 2*bs rows [cond | uncond]:
 * the conditioning (text_emb, text_enc, key_valid as k22_prior_forward takes them) is copied into the plan once; then for
 * k = 0 .. n_steps-1:  transformer([x[:bs] | x[:bs]], timesteps[k]) -> k22_prior_sampler_step (kind ANCESTRAL, table rows fp32[4]) or
 * k22_prior_ddim_step (kind DDIM, table rows fp32[8]), alternating between x and x_tmp; the final latent ends up in x.
 *   timesteps [n_steps][B], table [n_steps][4 | 8], noise_seq [n_steps][B][D]: all in EXECUTION order (schedule index T-1 first).
 *   noise_seq may be NULL for kind DDIM only (eta = 0).  x0_out [B][D] (DDIM: the last step's x0) may be NULL.
 *   n_steps is the schedule's own count: "ddimN" keeps the timesteps 1, 1 + 1000//N, ... below 1000, which is 3 steps for "ddim3" (the
 *   stride formula's 1000 is no timestep) and 31 for "ddim30" (stride 33).
 * use_graph != 0: the loop is ONE captured graph, a single chain on the handle's capture stream, launched on `stream`.  The handle
 * keeps one such loop, keyed by kind, n_steps, clamp and every pointer argument: a call with the same key replays it (the caller
 * refills its buffers), anything else captures again; k22_prior_bind drops it.  use_graph == 0 issues the same launches eagerly.
 * Both count into k22_debug_counter("loop_captures" / "loop_launches").  The first use of a plan measures its tile configurations and
 * runs one eager pass of the launch list, as k22_prior_forward does.
 * K22_EINVAL (with a k22_last_error text) for a null required argument, an unknown kind, n_steps < 1, ANCESTRAL without noise_seq, or
 * no bound workspace; a refused call leaves the handle and its captured loop as they were. */
enum { K22_PRIOR_LOOP_ANCESTRAL = 0, K22_PRIOR_LOOP_DDIM = 1 };
int k22_prior_sample_loop(K22Prior* m, int kind, float* x, float* x_tmp, float* x0_out, const float* timesteps, const float* table,
                          const float* noise_seq, const float* scales, const float* text_emb, const float* text_enc,
                          const float* key_valid, float clamp, int n_steps, int use_graph, void* stream);

/* ---- MoVQ decoder ---------------------------------------------------------------------------
 * Replaces MOVQ.decode (kandinsky2/vqgan/autoencoder.py:182-185: post_quant_conv + MOVQDecoder.forward,
 * kandinsky2/vqgan/movq_modules.py:228-357: conv_in, mid ResnetBlock/AttnBlock/ResnetBlock, up levels with
 * SpatialNorm ResnetBlocks (+AttnBlocks at the lowest level), nearest-x2 Upsample convs, norm_out + swish +
 * conv_out) and the uint8 epilogue of process_images (kandinsky2/utils.py:57-70).  Hyper-parameters mirror
 * CONFIG_2_1["image_enc_params"]["params"]["ddconfig"] (kandinsky2/configs.py:75-86).
 * Weight names are the reference state_dict keys ("post_quant_conv.weight", "decoder.conv_in.weight",
 * "decoder.mid.block_1.norm1.norm_layer.weight", ".conv_y.weight" ...); 3x3 weights packed [Npad][ky][kx][Cin]
 * (conv_in zero-extended to Cin = 64), 1x1 weights [Npad][Cin], everything else fp32 as the reference. */
typedef struct K22MoVQConfig {
  int dtype;           /* K22_BF16 | K22_F32 | K22_F16 */
  int ch;              /* 128 */
  int n_levels;        /* len(ch_mult) */
  int ch_mult[8];      /* (1, 2, 2, 4) */
  int num_res_blocks;  /* 2  (the decoder runs num_res_blocks + 1 blocks per level) */
  int attn_levels;     /* bit i set = AttnBlock after every ResnetBlock of level i (resolution/2^i in attn_resolutions) */
  int z_channels;      /* 4 */
  int out_ch;          /* 3 */
} K22MoVQConfig;
typedef struct K22MoVQ K22MoVQ;
int k22_movq_create(const K22MoVQConfig* cfg, const K22Weight* weights, int n_weights, K22MoVQ** out);
void k22_movq_destroy(K22MoVQ* m);
/* latent [B][4][h][w]; the caller allocates *workspace_bytes (256-byte aligned) and binds it */
int k22_movq_plan(K22MoVQ* m, int B, int h, int w, size_t* workspace_bytes);
int k22_movq_bind(K22MoVQ* m, void* workspace, size_t workspace_bytes);
/* z: fp32 NCHW latent (un-quantised, as the sampler leaves it: decode(h, force_not_quantize) semantics);
 * out: fp32 NCHW [B][3][H][W] (may be null); out_u8: uint8 NHWC [B][H][W][3] = ((x+1)*127.5).round().clamp(0,255)
 * (may be null); H = h << (n_levels-1). */
int k22_movq_decode(K22MoVQ* m, const float* z, float* out, unsigned char* out_u8, void* stream);
/* MoVQ ENCODER on the same handle type (MOVQ.encode, kandinsky2/vqgan/autoencoder.py:176-180 = Encoder.forward,
 * vqgan_blocks.py:335-367, + quant_conv; the img2img / inpainting pre-step of kandinsky2_1_model.py:458-469, 519-534).
 * Weights: "encoder.*" (GroupNorm weight/bias fp32; 3x3 packed [Npad][ky][kx][Cin], conv_in zero-extended to Cin = 64, conv_out
 * rows padded to 64; 1x1 [Npad][Cin]) and fp32 "quant_conv.*".  image: fp32 NCHW [B][3][H][W]; latent: fp32 NCHW [B][4][H/8][W/8]
 * (not multiplied by the pipeline's latent scale).  A handle holds one plan: encoder or decoder. */
int k22_movq_plan_encoder(K22MoVQ* m, int B, int H, int W, size_t* workspace_bytes);
int k22_movq_encode(K22MoVQ* m, const float* image, float* latent, void* stream);
int k22_movq_num_ops(const K22MoVQ* m);
/* Which form of the AttnBlock the NEXT plan of this handle (decoder or encoder) is built with; the current plan is not touched.
 *   K22_MOVQ_ATTN_AUTO (default)  fused exactly when T = h * w > 16384 and the block's width C is one the fused kernel admits
 *                                 (k22_movq_attention below), the scores form otherwise.  The rule reads T and C alone, never B.
 *   K22_MOVQ_ATTN_SCORES          q.k^T as a GEMM per image into a [B][T][T] workspace slot, row softmax, P.V^T as a GEMM per image.
 *   K22_MOVQ_ATTN_FUSED           ONE k22_movq_attention launch for all images; the plan has no [T][T] slot.  A plan whose AttnBlocks
 *                                 the kernel does not admit fails with K22_EINVAL and leaves the previous plan as it was.
 * The GEMMs before (norm, q, k, V^T) and after (proj_out) are the same in both forms.  K22_EINVAL for a null handle or another mode.
 * k22_debug_counter("movq_fused_attn_launches") counts the fused launches. */
enum { K22_MOVQ_ATTN_AUTO = 0, K22_MOVQ_ATTN_SCORES = 1, K22_MOVQ_ATTN_FUSED = 2 };
int k22_movq_set_attention(K22MoVQ* m, int mode);

/* ---- conditioning encoders ---------------------------------------------------------------------
 * The transformer towers that run once per prompt / image, one engine type for the three of them:
 *   K22_ENC_CLIP_TEXT    clip_model.token_embedding / positional_embedding / transformer / ln_final / text_projection as
 *                        Kandinsky2_1.generate_clip_emb walks them (kandinsky2/kandinsky2_1_model.py:159-168; OpenAI clip
 *                        model.py CLIP.encode_text): seq_out = ln_final(x) [B][n_ctx][width], pooled_out = seq_out[b][argmax
 *                        (tokens[b])] @ text_projection [B][out_dim]
 *   K22_ENC_CLIP_VISION  clip_model.encode_image (kandinsky2_1_model.py:177-181; clip model.py VisionTransformer.forward):
 *                        image [B][3][image_size][image_size] (already preprocessed) -> pooled_out [B][out_dim]
 *   K22_ENC_XLMR         MultilingualCLIP.forward (kandinsky2/model/text_encoders.py:108-122) = transformers XLMRobertaModel +
 *                        masked mean + LinearTransformation: seq_out = last_hidden_state [B][n_ctx][width], pooled_out [B][out_dim]
 * Weights (names are the engine's; kandinsky-2_amd/encoders.py maps the reference / OpenAI-clip / transformers state_dict keys):
 *   fp32: "token_embedding" [vocab][width], "positional_embedding" [n_ctx | max_pos][width], xlmr "token_type_embedding" [width],
 *   "embeddings_ln.*"; vision "class_embedding" [width], "ln_pre.*", "ln_post.*"; text "ln_final.*"; "layers.<l>.ln_1.*",
 *   "layers.<l>.ln_2.*", every Linear bias; "head.weight" [out_dim][width] (text_projection^T / visual.proj^T /
 *   LinearTransformation.weight), xlmr "head.bias".
 *   T (engine dtype), rows padded to 64: "layers.<l>.qkv.weight" [3*width][width] (rows Q | K | V, heads x 64 inside each),
 *   ".proj.weight", ".fc.weight" [4*width][width], ".out.weight" [width][4*width]; vision "patch.weight" [width][roundup(3*patch^2,
 *   64)] (conv1.weight flattened (c, i, j), zero padded).
 * The Linears' tile configurations come from the tile table like the other engines' (shipped for the production shapes). */
enum { K22_ENC_CLIP_TEXT = 0, K22_ENC_CLIP_VISION = 1, K22_ENC_XLMR = 2 };
typedef struct K22EncoderConfig {
  int dtype;       /* K22_BF16 | K22_F32 | K22_F16 */
  int kind;        /* K22_ENC_* */
  int width;       /* 768 / 1024 / 1024 (64 channels per head: the UNet's flash attention kernel); the vision tower also takes any
                      width % heads == 0 with width / heads <= 128 - CLIP ViT-bigG/14 of Kandinsky 2.2 (kandinsky2_2_model.py:24): 1664 / 16
                      = 104 per head - on a small-sequence attention kernel of its own (encoder.hip: enc_attention_generic_kernel) */
  int layers;      /* 12 / 24 / 24 */
  int heads;       /* 12 / 16 / 16 */
  int n_ctx;       /* tokens per sequence: 77 / 257 / 77 */
  int vocab;       /* 49408 / 0 / 250002 */
  int out_dim;     /* 768 */
  int image_size;  /* vision: 224 */
  int patch;       /* vision: 14 */
  int max_pos;     /* xlmr: 514 rows of position embeddings */
  int pad_id;      /* xlmr: 1 (padding token id = position-id offset) */
  float ln_eps;    /* 1e-5 */
  int mlp_dim;     /* 0 = 4 * width (OpenAI CLIP, XLM-R); CLIP ViT-bigG/14: 8192 at width 1664 */
  int hidden_act;  /* CLIP towers: 0 = QuickGELU (OpenAI CLIP), 1 = exact erf GELU (open_clip bigG: "hidden_act": "gelu") */
  int key_mask;    /* CLIP text: 0 = causal mask only (OpenAI clip; transformers without attention_mask); 1 = key_valid of k22_encoder_forward
                      masks padded keys in addition to the causal triangle (transformers' CLIPTextModel called with attention_mask).  A plan-time
                      switch: with 1 every forward needs key_valid */
  int eos_id;      /* CLIP text, the pooled row: 0 = argmax(tokens) (OpenAI clip; transformers when config.eos_token_id == 2); > 0 = the FIRST
                      position whose id equals eos_id (transformers otherwise), position 0 when the row holds none */
} K22EncoderConfig;
typedef struct K22Encoder K22Encoder;
int k22_encoder_create(const K22EncoderConfig* cfg, const K22Weight* weights, int n_weights, K22Encoder** out);
void k22_encoder_destroy(K22Encoder* m);
int k22_encoder_plan(K22Encoder* m, int B, size_t* workspace_bytes);     /* B sequences / images per call, <= 8 */
int k22_encoder_bind(K22Encoder* m, void* workspace, size_t workspace_bytes);
/* tokens: int32 [B][n_ctx] (text towers); key_valid: fp32 [B][n_ctx], 1 = token, 0 = padding (xlmr: the attention_mask);
 * CLIP text with cfg.key_mask: required as well - transformers' attention_mask, padded keys masked under the causal triangle);
 * image: fp32 [B][3][S][S] (vision); seq_out: fp32 [B][n_ctx][width] or null; pooled_out: fp32 [B][out_dim].  Device buffers. */
int k22_encoder_forward(K22Encoder* m, const int* tokens, const float* key_valid, const float* image, float* seq_out, float* pooled_out,
                        void* stream);

/* ---- img2img / inpainting latent arithmetic ----------------------------------------------------
 * out = mask * (sa*init + sb*noise) + (1 - mask) * x   [N][C][HW] fp32; mask [N][1][HW] (1 = keep the known region).
 * mask == NULL (x ignored): out = sa*init + sb*noise = DDPMScheduler.add_noise / q_sample (kandinsky2/utils.py:43-54) with
 * sa = sqrt(alphas_cumprod[t]), sb = sqrt(1 - alphas_cumprod[t]); noise == NULL: the un-noised init.  With a mask it is the
 * per-step re-imposition of the known region in the Kandinsky 2.2 inpainting pipeline (kandinsky2/kandinsky2_2_model.py:150-173 ->
 * diffusers KandinskyV22InpaintPipeline).  broadcast_first != 0: init / noise / mask are those of image 0 for every n. */
int k22_blend_noised(const float* x, const float* init, const float* noise, const float* mask, float sa, float sb, float* out,
                     int N, int C, int HW, int broadcast_first, void* stream);

/* ---- single-kernel entry points for the parity tests; no product code calls them ----------------
 * The small kernels around the MoVQ, encoder and prior engines (csrc/movq_kernels.hip, encoder.hip, prior.hip), each through the
 * launcher its engine's plan uses - same grid, same LDS attribute, same admission rule (tests/test_aux_kernels_gpu.py compares every
 * one with a float64 restatement, tests/aux_ref.py).  Conventions of the other kernel-level entries: enqueue on `stream`, allocate
 * nothing, return 0 or a K22_E* code; dtype = K22_BF16 | K22_F16 | K22_F32 is the storage type T of the tensors declared void*.
 *
 * MoVQ.  NHWC T tensors move one 16-byte channel vector per thread: C % 8 == 0 (16-bit types) / C % 4 == 0 (fp32), else K22_EINVAL.
 *   spatialnorm_apply  out = act((x * A + Bc) * conv_y(zq) + conv_b(zq)) with coeff [B][C][2] = (A, Bc) GIVEN (the GroupNorm statistics
 *                      are not run), zq fp32 NHWC [B][h0][w0][4] read at (y >> shift, x >> shift), wy / wb [C][4], by / bb [C];
 *                      x [B][H][W][C] -> out [B][H + 2 pad][W + 2 pad][C] (zero border); W % 2^shift == 0; act 0 | K22_ACT_SILU
 *   upsample2_pad      [B][H][W][C] -> zero-bordered nearest x2 [B][2H + 2][2W + 2][C]
 *   pad_copy           [B][H][W][C] -> zero-bordered [B][H + 2][W + 2][C]
 *   subsample_odd      [B][H][W][C] (H, W even) -> [B][H/2][W/2][C] = x[2y + 1][2x + 1]
 *   softmax_rows       in place: row r of `rows` rows of L elements (L % 8 / % 4 == 0) becomes softmax(scale * row), fp32 math
 *   movq_prepare       z fp32 NCHW [B][4][h][w] -> zq fp32 NHWC [B][h][w][4] (copy) and xin T [B][h + 2][w + 2][Cpad] = zero-bordered
 *                      post_quant_conv(z) (wpq [4][4], bpq [4]) in channels 0..3, zeros in 4..Cpad-1
 *   movq_enc_prepare   image fp32 NCHW [B][3][H][W] -> xin T [B][H + 2][W + 2][Cpad], channels 3.. and the border zero
 *   movq_quant_conv    h fp32 NCHW [B][4][HW] -> out fp32 [B][4][HW] = wq [4][4] . h + bq
 *   to_uint8_nhwc      x fp32 NCHW [B][C][H][W] -> y uint8 NHWC = ((x + 1) * 127.5).round().clamp(0, 255), ties to even */
int k22_spatialnorm_apply(const void* x, const float* coeff, const float* zq, const float* wy, const float* by, const float* wb, const float* bb,
                          void* out, int B, int H, int W, int C, int h0, int w0, int shift, int act, int pad, int dtype, void* stream);
int k22_upsample2_pad(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream);
int k22_pad_copy(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream);
int k22_subsample_odd(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream);
int k22_softmax_rows(void* x, long rows, int L, float scale, int dtype, void* stream);
/* Fused single-head attention of the MoVQ AttnBlock (csrc/movq_attention.hip; arithmetic contract: csrc/attention_common.h).  Per image b and query t
 *     out[b][t][:] = sum_j softmax_j(C^-1/2 * q_t . k_j) * v_j + bias_v,   j = 0 .. T-1, one head, no mask.
 * Layouts: q, k [B][T][C] row-major and vt = V^T [B][C][T], in the storage type `dtype` (K22_BF16 | K22_F16 | K22_F32), 16-byte aligned;
 * bias_v fp32 [C] or NULL; out [B][T][C] in the storage type.  The [T][T] scores are never written to memory.
 * Rounding: fp32 scores and online softmax (running maximum and sum); the row sum is taken over the unrounded probabilities; P is rounded
 * ONCE to the storage type in front of the P.V product (K22_F32: not at all); bias_v is added after the normalisation (the weights sum
 * to 1, so this is exact); the output is rounded once on store.  No atomics and a fixed reduction order: two launches give equal bits, and
 * image b of a batch has the bits of the same image launched alone.
 * K22_EINVAL (with a k22_last_error text that names the rule) for a null q, k, vt or out; C outside {128, 256, 384, 512}; T < 64,
 * T % 64 != 0 or T > 4194304; B < 1; a dtype outside the three; a misaligned pointer.  A refused call launches nothing and leaves the library usable. */
int k22_movq_attention(const void* q, const void* k, const void* vt, const float* bias_v, void* out,
                       int B, int T, int C, int dtype, void* stream);
int k22_movq_prepare(const float* z, const float* wpq, const float* bpq, float* zq, void* xin, int B, int h, int w, int Cpad, int dtype, void* stream);
int k22_movq_enc_prepare(const float* image, void* xin, int B, int H, int W, int Cpad, int dtype, void* stream);
int k22_movq_quant_conv(const float* h, const float* wq, const float* bq, float* out, int B, int HW, void* stream);
int k22_to_uint8_nhwc(const float* x, unsigned char* y, int B, int C, int H, int W, void* stream);
/* 2.2 inpainting loop (csrc/prestep.hip; tests/test_decoder22_loop_gpu.py, tests/decoder22_ref.py): the stage k22_unet_sample_loop_keep adds.
 *   keep_region        out[n][c][p] = m[p] * (sa * init[c][p] + sb * noise0[n % (B / 2)][c][p]) + (1 - m[p]) * x[n][c][p] over the CFG batch
 *                      x / out [B][4][HW] (out == x allowed); init [4][HW] and mask m [HW] of image 0 serve every row, noise0 [B / 2][4][HW]
 *                      is each sample's own; every operation rounded once: |out - exact| <= 4 * 2^-24 * (|m| (|sa init| + |sb noise|) +
 *                      |1 - m| |x|).  K22_EINVAL: a null argument, B odd or < 2, HW < 1. */
int k22_keep_region(const float* x, const float* init, const float* noise0, const float* mask, float sa, float sb, float* out, int B, int HW,
                    void* stream);
/* Encoder towers.
 *   enc_layernorm      `rows` fp32 rows x + r * ldx of D <= 2048 values (K22_EINVAL above: 8 x 256 values per row) -> fp32 rows
 *                      out_f32 + r * ld_out (optional; may be x itself) and / or T rows out_t + r * D (optional)
 *   enc_embed          x [B][n_ctx][D] = (tok_emb[id] + pos_emb[pos]) + type_emb (type_emb optional), ids clamped into [0, vocab);
 *                      pos = t, or (xlmr) cumsum(tok != pad_id) * (tok != pad_id) + pad_id clamped to max_pos - 1
 *   enc_gather_eot     out [B][D] = x[b][argmax_t tokens[b][t]] (first maximum)
 *   enc_masked_mean    out [B][D] = sum_t x[b][t] * mask[b][t] / sum_t mask[b][t]
 *   enc_patchify       image fp32 [B][3][S][S] -> T rows [B * (S / patch)^2][Kp], column c * patch^2 + i * patch + j, zeros from 3 * patch^2 on
 *   enc_vision_assemble x [B][P + 1][D]: row 0 = cls + pos[0], row 1 + p = patch_out[b][p] + pos[1 + p]
 *   enc_mlp_act        y T [n] = x * sigmoid(1.702 x) (exact == 0) or the erf GELU (exact != 0) of fp32 x [n]
 *   enc_attention_generic  qkv T [B][n][3 * heads * hd] (columns Q | K | V, heads x hd inside each) -> out T [B][n][heads * hd] =
 *                      softmax(q k^T hd^-0.5) v per head; admitted as K22Encoder's plan admits it: hd <= 128, n <= 512 and
 *                      n * (hd + 2) * sizeof(T) * (2 for the 16-bit types) + 10 KB <= 160 KB of LDS, else K22_EINVAL */
int k22_enc_layernorm(const float* x, long ldx, const float* gain, const float* beta, float* out_f32, long ld_out, void* out_t, int rows,
                      int D, float eps, int dtype, void* stream);
int k22_enc_embed(const int* tokens, const float* tok_emb, const float* pos_emb, const float* type_emb, float* x, int B, int n_ctx, int D,
                  int vocab, int xlmr, int pad_id, int max_pos, void* stream);
int k22_enc_gather_eot(const int* tokens, const float* x, float* out, int B, int n_ctx, int D, void* stream);
int k22_enc_masked_mean(const float* x, const float* mask, float* out, int B, int n_ctx, int D, void* stream);
int k22_enc_patchify(const float* image, void* out, int B, int S, int patch, int Kp, int dtype, void* stream);
int k22_enc_vision_assemble(const float* patch_out, const float* cls, const float* pos, float* x, int B, int P, int D, void* stream);
int k22_enc_mlp_act(const float* x, void* y, long n, int exact, int dtype, void* stream);
int k22_enc_attention_generic(const void* qkv, void* out, int B, int heads, int n, int hd, int dtype, void* stream);
/* Prior (k22_prior_sampler_step above belongs to the same surface).
 *   prior_layernorm    `rows` fp32 rows x + r * ldx of D <= 2048 values (K22_EINVAL above) -> rows y + r * D, fp32 (to_f32 != 0) or T;
 *                      eps 1e-5: enc_layernorm's kernel with one of its outputs
 *   prior_finish_input inp [B][n_ctx][D] += pos [n_ctx][D], the last row of every sequence = prd [D] + pos[n_ctx - 1] */
int k22_prior_layernorm(const float* x, long ldx, const float* gain, const float* beta, void* y, int rows, int D, int to_f32, int dtype,
                        void* stream);
int k22_prior_finish_input(float* inp, const float* pos, const float* prd, int B, int n_ctx, int D, void* stream);
/* Flash attention with the mask and output-format fields the engines set (csrc/attention.hip, arithmetic contract: csrc/attention_common.h;
 * tests/test_attention_parity_gpu.py, tests/attention_ref.py).  k22_attention's sequence - kv_pack, then launch_attention - and its tensors (ctxkv may be null when S == 0;
 * dtype: all five arithmetics, fp32 tensors for the split ones), plus
 *   causal     key j is dead for query t when j > t (the CLIP text tower, the prior); compares key index with query index: S must be 0
 *   key_valid  optional fp32 [B][kv_n]: 0 = key dead for every query of the image; keys >= kv_n are alive (the prior's appended tokens)
 *   out_x3     split dtypes only: `out` is written as x3 chunks (what the proj_out GEMM of the split engines reads)
 * K22_EINVAL with nothing launched for causal && S != 0, kv_n > S + T, out_x3 with a non-split dtype.
 * PRECONDITION, met by every engine: each query keeps at least one alive key, i.e. key 0 is valid (causal keeps key 0 for query 0).  A row
 * without one is 0 * inf. */
int k22_attention_masked(const void* qkv, const void* ctxkv, void* kall, void* vtall, void* out, int B, int H, int T, int S, int causal,
                         const float* key_valid, int kv_n, int out_x3, int dtype, void* stream);
/* GroupNorm32 of the UNet, one kernel per entry (csrc/elementwise.hip; tests/test_gn_parity_gpu.py, tests/gn_ref.py), each through the
 * launcher K22UNet::op_gn calls.  x0 [B][H][W][C0] (+ x1 [B][H][W][C1], C1 = 0 and x1 null without a concat) are NHWC tensors of the
 * storage type (fp32 for the split dtypes); 32 groups over C = C0 + C1.
 *   gn_stats   per-channel (sum, sum of squares) of each of nsplit pixel ranges of ceil(HW / nsplit) pixels: partial [B][nsplit][C][2]
 *              fp32, *nsplit_out receives nsplit (a function of B and HW; at most 128).  A range past the end of the image gives zero
 *              rows.  K22_EINVAL: C % 128 != 0, C0 % 4 != 0, C > 3072.
 *   gn_coeff   coeff [B][C][2] = (A, Bc) with GroupNorm(x) [* (1 + scale) + shift] = x * A + Bc, from the partial sums of up to two sources
 *              as their producers left them: image b owns rows [b * rpi_k, (b + 1) * rpi_k) of st_k [rows][C_k][2] (gn_stats: rpi = nsplit,
 *              one source with C_k = C; k22_conv3x3_gnstats / k22_gemm_gnstats: their *rows_per_image).  A group may straddle the two
 *              sources.  film (optional): row b at film + b * film_ld holds scale at [c] and shift at [C + c]; film_ld >= 2 C.
 *              K22_EINVAL, nothing launched: C % 32 != 0, more than 256 channels per group, rpi <= 0 on a used source, C1 > 0 with a
 *              null st1, film with film_ld < 2 C, null gamma / beta / coeff.
 *   gn_apply   out [B][Ho + 2 pad][Wo + 2 pad][C] = zero-bordered resample(act(x * A + Bc)); mode 0 same size, 1 = 2x2 average (floor of
 *              H / 2, W / 2), 2 = nearest x2; act 0 | K22_ACT_SILU.  K22_F16X3 / K22_F16X2: the fp32 kernel writing x3 chunks, as k22_groupnorm.
 *              C and C0 must be multiples of 8 (16-bit types) / 4 (fp32). */
int k22_gn_stats(const void* x0, const void* x1, int C0, int C1, int B, int HW, float* partial, int* nsplit_out, int dtype, void* stream);
int k22_gn_coeff(const float* st0, int rpi0, int C0, const float* st1, int rpi1, int C1, int B, int HW, const float* gamma, const float* beta,
                 const float* film, long film_ld, float eps, float* coeff, void* stream);
int k22_gn_apply(const void* x0, const void* x1, int C0, int C1, int B, int H, int W, const float* coeff, int act, int mode, int pad, void* out,
                 int dtype, void* stream);
/* The kernels that open and close a UNet step, one per entry (csrc/elementwise.hip, csrc/sampler.hip; tests/test_seam_kernels_gpu.py,
 * tests/seam_ref.py), each through the launcher named with it.  k22_ddim_step / k22_plms_step above belong to the same surface.  K22_EINVAL
 * with nothing launched: a null required argument, a non-positive size, and what each line names.
 *   conv_in            launch_conv_in (K22UNet::plan, the stem op): out T NHWC [B][H][W][Cout] = conv3x3(pad 1) of the fp32 NCHW input
 *                      [x (4) | img (4) | mask (1)] + bias; w_packed fp32 [Cin * 9][Cout] (pack.py: pack_stem), Cin 4 | 8 | 9; channels 4-7
 *                      are img (img_premul != 0) or img * mask, channel 8 the mask [B][1][H][W].  Refused: another Cin, Cin = 9 without img
 *                      and mask, Cin = 8 without img, img_premul = 0 without mask
 *   timestep_embedding launch_timestep_embedding (K22UNet::time_rows; the prior's plan): out [rows][2 half] = [cos(t f) | sin(t f)], the
 *                      argument t[r] * freqs[k] formed in fp32
 *   linear_smallm_ld   launch_linear_smallm with every field of LinearSmallParams (K22UNet::time_rows: rows = steps x B, add_mod = B,
 *                      ldo = film_total; build_cond_ops / build_cond_ops_22): out[m * ldo + n] = act_out(sum_k act_in(x[m * ldx + k]) W[n][k] + bias[n])
 *                      + add[(add_mod > 0 ? m % add_mod : m) * ld_add + n]; bias / add optional; W [N][K] of wdtype.  Refused: M outside
 *                      1..8, K % (16 bytes of wdtype), M_template * K * 4 > 64 KB, ldx < K, ldo < N, ld_add < N, an act outside 0 | K22_ACT_SILU
 *   layernorm_f32      launch_layernorm_f32 (K22UNet::build_cond_ops / build_cond_ops_22: ln_model_n, ctx_norm, emb_norm): y = LN(x)
 *                      over rows of D contiguous fp32 values, biased variance
 *   resample           launch_resample (K22UNet::resblock, the skip branch of an up / down block): T NHWC [B][H][W][C] -> mode 1: 2x2 average
 *                      [B][H / 2][W / 2][C] (floor; a trailing odd row / column is not read), mode 2: nearest [B][2H][2W][C].  Refused: another
 *                      mode, C % 8 (16-bit types) / % 4 (fp32), mode 1 with H < 2 or W < 2
 *   cast_rows          launch_cast_rows (K22UNet::build_cond_ops / build_cond_ops_22: ctx assembly; the prior's plan): y T [r * ldy + c] = T(x fp32 [r * ldx + c]), c < cols
 *   kv_pack            launch_kv_pack (K22UNet::attnblock; xf_plan.h): K_all T [B][H][Tkp][64], V^T_all T [B][H][64][Tkp] with keys
 *                      [ctx 0..S-1 | self S..S+T-1 | zero pad], Tkp = roundup(S + T, 64) as k22_attention derives it; qkv [B * T][3 * 64 H]
 *                      columns Q | K | V, ctxkv [B * S][2 * 64 H] columns K | V (null allowed when S == 0) */
int k22_conv_in(const float* x, const float* img, const float* mask, const float* w_packed, const float* bias, void* out, int B, int H, int W,
                int Cin, int Cout, int img_premul, int dtype, void* stream);
int k22_timestep_embedding(const float* t, const float* freqs, float* out, int rows, int half, void* stream);
int k22_linear_smallm_ld(const float* x, long ldx, const void* W, const float* bias, const float* add, long ld_add, int add_mod, float* out,
                         long ldo, int M, int N, int K, int act_in, int act_out, int wdtype, void* stream);
int k22_layernorm_f32(const float* x, const float* gain, const float* beta, float* y, int rows, int D, float eps, void* stream);
int k22_resample(const void* x, void* y, int B, int H, int W, int C, int mode, int dtype, void* stream);
int k22_cast_rows(const float* x, void* y, int rows, int cols, long ldx, long ldy, int dtype, void* stream);
int k22_kv_pack(const void* qkv, const void* ctxkv, void* kall, void* vtall, int B, int H, int T, int S, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* K22_H */
