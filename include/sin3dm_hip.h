/*
 * sin3dm_hip.h — C ABI of libsin3dm_hip.so, the MI355X (gfx950) implementation of the Sin3DM
 * denoising path.  Plain pointers and sizes only; no torch types.  The reference has no FFI of its
 * own (it is pure Python/PyTorch): each entry point below names the reference Python
 * interface it stands under (paths relative to /root/reference/).  INTEGRATION.md shows the ctypes
 * stub that binds them.
 *
 * Conventions
 *   - return 0 on success, a negative s3d_status otherwise; the message is s3d_last_error()
 *     (thread-local).  Nothing throws or aborts across this boundary.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     every compute call only enqueues work on it and never synchronises.
 *   - all tensors are fp32 device pointers owned by the caller, in the REFERENCE layouts
 *     (NCHW composed triplanes, [N,3] points ...); the library re-lays them out internally (NHWC).
 *   - parameters are copied and repacked into library-owned device memory; workspaces belong to the
 *     handle and grow on demand.  Handles are not thread-safe: one host thread per handle.
 */
#ifndef SIN3DM_HIP_H
#define SIN3DM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S3D_ABI_VERSION 13
#define S3D_API __attribute__((visibility("default")))

typedef enum {
    S3D_OK = 0,
    S3D_ERR_INVALID = -1,     /* bad argument / shape (the shim raises AssertionError/ValueError) */
    S3D_ERR_MISSING = -2,     /* forward called with parameters not all set                      */
    S3D_ERR_HIP = -3,         /* a HIP runtime call failed                                        */
    S3D_ERR_UNSUPPORTED = -4, /* a configuration the reference itself cannot construct/run        */
    S3D_ERR_INTERNAL = -5     /* the library caught itself out (a bug to report); results invalid */
} s3d_status;

S3D_API int s3d_abi_version(void);

/* Process-wide options: which of several kernel forms the library launches.  Every form is parity-tested (tests/test_hip_parity.py,
 * test_hip_train.py run the golden vectors under each); "bit-identical" forms differ in launch shape only.  name: with or without
 * the "S3D_" prefix; value: WINO 0, 4 or 24, CONV_IMPL "naive" / any other string, every other option 0 or 1; "" or NULL = back
 * to the library's own choice; any other value is rejected (S3D_ERR_INVALID).  Until s3d_set_option is called for an option,
 * the environment variable S3D_<NAME> (read once, at the option's first use) supplies its value — the way earlier rounds selected
 * forms; a value the option does not take leaves it unset there.  The call is the documented way.  Options are read at every
 * launch and may be switched between two launches on a live inference handle: every successful call moves a process-wide
 * generation, and a handle whose measured workspace or carried in_conv is older than that measures again (and grows, as for a new
 * shape) at its next launch — a forward under an option equals the same forward on a handle created under it.  A training
 * handle's repack plan (s3d_unet_train_attach) keeps only the weight images of the forms selected THEN current: a launch that would
 * read another image is refused (S3D_ERR_INVALID, "attach again"), so set those before attaching.
 *   WINO          24 (default) mixed Winograd F(2x4,3x3) | 4: F(2x2) | 0: direct MFMA convolution             (rounding differs)
 *   WINO24W       unset: by launch size | 0 never | 1 always the 64-output-channel block                    (bit-identical)
 *   VCAT          0: materialise upsample + concat in the output blocks (default: virtual concat)            (rounding differs)
 *   WGRAD_WINO    0: direct 3x3 weight gradient | default (1): Winograd F(2x2)                               (rounding differs)
 *   RANK1_SLICES  0: one K slice of the rollout tables (default: two from 256 channels)                      (rounding differs)
 *   RANK1_BATCH   0: k_rank1, one sample per block (default: k_rank1b / two-sample blocks)                   (bit-identical)
 *   CONV_IMPL     "naive": one-thread-per-output reference kernels (tests)                                   (rounding differs)
 *   CONV1X1_T     unset: by launch size | 0 never | 1 always the transposed-accumulator 1x1 epilogue         (bit-identical)
 *   GN_FUSED      unset: by launch size | 0: GroupNorm partials added ahead of the consumer | 1: inside it   (bit-identical)
 *   BWD_SIDE      0: every launch of a training step stays on the caller's stream (default: weight gradients on a side stream, the
 *                 auto-encoder's two nets as two chains)                                                     (bit-identical)
 *   GNB_FUSED     0: the GroupNorm backward's two per-channel sums always from its own read pass (default: from the epilogue of
 *                 the input-gradient convolution in front of it where that is the mixed Winograd kernel)     (rounding differs)
 *   EDGE_SIGNAL   how the backward pass's side stream learns that the edge sums are done: 1 an event on the launch's own completion
 *                 signal (default outside profilers), 0 a plain event record behind it (default under rocprofv3, whose tracing
 *                 makes the first form crawl); committed traces state which form they ran                    (bit-identical)
 * s3d_get_option: the current value, -1 when unset. */
S3D_API int s3d_set_option(const char* name, const char* value);
S3D_API int s3d_get_option(const char* name, int* value);
/* Riders: in the inference forward's virtual-concat path the GroupNorm launches that a neighbouring default-form 1x1 convolution
 * neither feeds nor needs (k_gn_partials_up, the k_gn_finalize behind the pooling, k_gn_finalize_cat) run in that convolution's
 * first blocks.  on = 0: every stage in a launch of its own; anything else: riders (the default; S3D_RIDERS=0 in the environment,
 * read once before the first call, starts the process with them off).  The same kernel bodies either way: bit-identical.  Not an
 * option of the table above: it selects no kernel form and no workspace depends on it; it may be switched between two launches. */
S3D_API int s3d_set_riders(int on);
S3D_API const char* s3d_last_error(void);
/* number of visible HIP devices, or a negative s3d_status: lets the shim fail loudly without torch */
S3D_API int s3d_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Denoiser: TriplaneUNetModelSmall / TriplaneUNetModelSmallRaw
 *   constructor  src/diffusion/unet_triplane.py:346-449 (Raw: :544-646)
 *   forward      src/diffusion/unet_triplane.py:465-510 (Raw: :664-702)
 * ------------------------------------------------------------------------------------------ */
typedef struct s3d_unet s3d_unet;

typedef struct {
    int32_t in_channels;            /* 12 = fdim_geo + fdim_tex   (src/utils/parser_util.py:131-132) */
    int32_t model_channels;         /* 64 default, 128 for BASELINE config 2                          */
    int32_t out_channels;
    int32_t num_res_blocks;         /* only 1 is constructible in the reference       */
    int32_t n_levels;               /* len(channel_mult)                                              */
    int32_t channel_mult[8];
    int32_t use_scale_shift_norm;   /* FiLM h*(1+scale)+shift (default True) vs h+emb                 */
    int32_t is_rollout;             /* 1: TriplaneUNetModelSmall, 0: ...SmallRaw                      */
} s3d_unet_cfg;

S3D_API int s3d_unet_create(const s3d_unet_cfg* cfg, s3d_unet** out);
S3D_API void s3d_unet_destroy(s3d_unet* m);

/* Number of parameter tensors the configuration expects and the i-th one's state_dict name/shape
 * (the names of nn.Module.state_dict(), e.g. "input_blocks.1.1.in_layers.2.conv_xz.weight"). */
S3D_API int s3d_unet_num_params(const s3d_unet* m);
S3D_API int s3d_unet_param_info(const s3d_unet* m, int i, const char** name, int64_t shape[4], int* ndim);

/* load_state_dict, one tensor at a time: `data` is a HOST fp32 pointer in the PyTorch layout
 * (conv OIHW, linear [out,in]); the tensor is repacked for the kernels and uploaded. */
S3D_API int s3d_unet_set_param(s3d_unet* m, const char* name, const float* data, const int64_t* shape, int ndim);

/* forward(x, timesteps, H, W, D): x,out [B,C,H+D,W+D] device fp32; t [B] device fp32 (already in
 * the original 0..999 index space, i.e. after _WrappedModel, src/diffusion/respace.py:123-128). */
S3D_API int s3d_unet_forward(s3d_unet* m, const float* x, const float* t, int B, int H, int W, int D,
                     float* out, void* stream);

/* The timestep path alone and a forward that takes its result.  emb -> FiLM only depends on the timestep values (and the
 * weights): a sampling loop that knows them on the host (GaussianDiffusion._loop) computes each table once and reuses it
 * for every sample.  s3d_unet_film: timestep_embedding -> time_embed -> all emb_layers (nn.py:103-121,
 * unet_triplane.py:371-375, 232-238, 477, 281) for n timestep values t (device fp32) -> film [n][s3d_unet_film_width()].
 * s3d_unet_forward_film: forward() with that table; film_stride = width (one row per sample) or 0 (all samples share row 0).
 * Streams: every call on one handle uses handle-owned scratch (the workspace arena, s3d_unet_film's hidden vectors) without
 * internal events — issue the calls of a handle from ONE stream at a time, and make a stream that consumes a film table
 * produced on another stream wait for it (the Python mirror records an event with each cached table and does so). */
S3D_API int s3d_unet_film_width(const s3d_unet* m);

/* Workspace lanes: several INDEPENDENT sample chains through one handle, each on its own HIP stream (hardware queue).  The
 * reference makes N samples by batching them (src/sample.py:33-38); at small batch a denoising step is a chain of one-round,
 * latency-bound launches, and a second independent chain fills what the first leaves idle (no event edge is needed between
 * independent samples).  The packed weights are shared; everything a forward WRITES — the activation workspace, s3d_unet_film's
 * scratch, the measured-shape key — exists once per lane.  s3d_unet_select_lane(m, k) makes lane k (0 <= k < S3D_MAX_LANES;
 * created on first use; lane 0 always exists and is selected at creation) the target of the following inference calls on this
 * handle (s3d_unet_forward / _film / _forward_film / _step_film): one stream per lane at a time, calls of different lanes may
 * be in flight on different streams together.  Still ONE host thread per handle.  Training (s3d_unet_forward_train /
 * _backward) runs on lane 0; a weight update (s3d_unet_set_param, s3d_unet_repack) must not overlap ANY lane's work in flight. */
#define S3D_MAX_LANES 16
S3D_API int s3d_unet_select_lane(s3d_unet* m, int lane);
S3D_API int s3d_unet_current_lane(const s3d_unet* m);
S3D_API int s3d_unet_film(s3d_unet* m, const float* t, int n, float* film, void* stream);
S3D_API int s3d_unet_forward_film(s3d_unet* m, const float* x, const float* film, int film_stride, int B, int H, int W, int D,
                          float* out, void* stream);

/* Live kernel timing for bench.py's roofline line: HIP events are recorded on `stream` around every
 * MFMA convolution launch of each `every`-th forward (0 = off).  s3d_unet_profile_read waits for the
 * recorded events, ADDS their durations to `out` (caller zero-initialises) and recycles them.
 * flops = algorithmic flops of the launches, 2*taps*cin*cout*pixels; mfma_flops = what the
 * matrix cores really multiply for them (Winograd F(2x2,3x3): 4/9 of the direct count, F(2x4,3x3): 1/3, F(4x4,3x3): 1/4).
 * s3d_unet_profile_kernel: names of the kernels the timed launches of class cls actually dispatched since profiling was switched
 * on (" + "-joined when a class used more than one, e.g. both blockings of the mixed Winograd kernel; "" if none):
 * bench.py labels its roofline line with it instead of deriving a name from environment switches.
 * s3d_unet_profile_classes: which launch classes of a profiled forward are bracketed (bit 0: 3x3, bit 1: 1x1, bit 2: rank-1;
 * default 7).  An event pair costs the step ~3 us (38 pairs' worth per profiled step with all classes): bench.py brackets only
 * the dominant class inside its timed region and the other two in a short pass of its own afterwards. */
#define S3D_PROF_CLASSES 4
typedef struct {
    double ms[S3D_PROF_CLASSES];   /* [0] dense 3x3 (the dominant kernel; training: forward + dgrad), [1] 1x1 skip convs, [2] rank-1
                                      rollout vector convs, [3] training only: the 3x3 weight-gradient launches (k_wgrad_wino; on the
                                      backward pass's side stream their time includes sharing the chip with the main chain) */
    double flops[S3D_PROF_CLASSES];
    int64_t launches[S3D_PROF_CLASSES];
    int64_t forwards;      /* forwards that were instrumented */
    double mfma_flops[S3D_PROF_CLASSES];
} s3d_profile;
S3D_API int s3d_unet_profile(s3d_unet* m, int every);
S3D_API int s3d_unet_profile_classes(s3d_unet* m, int mask);   /* bit c = class c of s3d_profile */
S3D_API int s3d_unet_profile_read(s3d_unet* m, s3d_profile* out);
S3D_API const char* s3d_unet_profile_kernel(const s3d_unet* m, int cls);
/* ------------------------------------------------------------------------------------------
 * Sampler update: GaussianDiffusion.p_mean_variance + p_sample / ddim_sample
 *   src/diffusion/gaussian_diffusion.py:233-327, 396-440, 538-600
 * One fused element-wise kernel per step.  `tables` is a device fp32 array [S3D_TAB_ROWS][T]
 * (the float64 schedule tables gathered-then-cast exactly like _extract_into_tensor, :934-947).
 * ------------------------------------------------------------------------------------------ */
enum { S3D_TAB_SQRT_RECIP = 0, S3D_TAB_SQRT_RECIPM1, S3D_TAB_COEF1, S3D_TAB_COEF2, S3D_TAB_LOGVAR,
       S3D_TAB_ACP, S3D_TAB_ACP_PREV, S3D_TAB_ROWS };
enum { S3D_STEP_DDPM = 0, S3D_STEP_DDIM = 1, S3D_STEP_MEAN_ONLY = 2 };
enum { S3D_MEAN_START_X = 0, S3D_MEAN_EPSILON = 1 };

typedef struct {
    int32_t mode;                /* S3D_STEP_*                                                     */
    int32_t mean_type;           /* S3D_MEAN_*  (predict_xstart=True -> START_X)                    */
    int32_t clip_denoised;       /* clamp x0 to [-1,1]                                              */
    int32_t is_mask_t0;          /* ddim in-painting branch (:568-577)                              */
    float eta;                   /* ddim eta                                                        */
    int32_t T;                   /* table length                                                    */
    int64_t batch;               /* B                                                               */
    int64_t per_sample;          /* C*(H+D)*(W+D)                                                   */
    const float* model_out;      /* [B, per_sample]                                                 */
    const float* x;              /* x_t                                                             */
    const float* noise;          /* eps ~ N(0,1); may be NULL for MEAN_ONLY or ddim eta == 0        */
    const int64_t* t;            /* [B] device int64 indices into the (respaced) tables             */
    const float* tables;         /* [S3D_TAB_ROWS][T] device fp32                                   */
    const float* y0;             /* optional in-painting target / mask (both or neither)            */
    const float* mask;
    float* sample;               /* out: x_{t-1}   (NULL for MEAN_ONLY)                              */
    float* pred_xstart;          /* out                                                             */
    float* mean;                 /* out, optional (posterior mean; DDPM / MEAN_ONLY)                */
} s3d_sampler_args;

S3D_API int s3d_sampler_step(const s3d_sampler_args* a, void* stream);

/* One whole denoising step of the sampling loops (p_sample_loop_progressive / ddim_sample_loop_progressive,
 * src/diffusion/gaussian_diffusion.py:488-536, 687-734): the UNet forward on x_t = step->x with the FiLM row(s) of
 * s3d_unet_film, its output head (unet_triplane.py:441-445, 507-508) and the sampler update above in the head's launch
 * ("K8: fuse with K9") — the model output is not stored unless model_out != NULL (step->model_out is
 * ignored).  Same arithmetic in the same order as s3d_unet_forward_film followed by s3d_sampler_step: identical bits. */
S3D_API int s3d_unet_step_film(s3d_unet* m, const float* film, int film_stride, int B, int H, int W, int D,
                       const s3d_sampler_args* step, float* model_out, void* stream);
/* The same step when the caller knows what follows it (round 6; SURVEY.md section 2b lists K8 + K9 + K2 as one fusion).  in_conv is
 * TriplaneConv(in_channels, ch, 1, padding=0, is_rollout=False) (src/diffusion/unet_triplane.py:378, applied first thing in forward,
 * :482): a pointwise map of x_t with no timestep in it.  In a sampling loop the next step's x_t is this step's sample (:533-534), so
 *   - S3D_CARRY_OUT: the output head also evaluates the NEXT step's in_conv (+ its GroupNorm partial sums) on the x_{t-1} values it has
 *                  just formed and leaves it in the lane's workspace — same products, same order, same thread mapping as the in_conv
 *                  kernel: the same bits;
 *   - S3D_CARRY_IN: the caller vouches that step->x is the previous step's sample, UNMODIFIED since that call: its in_conv launch is
 *                  skipped when the previous call on this lane was an S3D_CARRY_OUT step of the same shape whose sample is step->x and
 *                  nothing (another forward, a parameter change, a workspace reallocation) came between; otherwise the flag is ignored.
 * carry_flags = 0 is s3d_unet_step_film.  Results are identical bits either way (tests/test_hip_parity.py). */
enum { S3D_CARRY_OUT = 1, S3D_CARRY_IN = 2 };
S3D_API int s3d_unet_step_film_carry(s3d_unet* m, const float* film, int film_stride, int B, int H, int W, int D,
                       const s3d_sampler_args* step, float* model_out, void* stream, int carry_flags);

/* Known-region sampling (outpainting / local editing; DESIGN.md section 20 — no counterpart in the reference).  After the update of a
 * DDPM or DDIM step at schedule index i = t[b], the known part of x_{t-1} is replaced by the source latent noised to level i - 1:
 *     k      = (sa[i] * y0) + (sb[i] * noise)                  q_sample(y0, i - 1, noise); i == 0: sa = 1, sb = 0
 *     sample = (mask * k) + ((1 - mask) * x_prev)              x_prev: what the step writes to `sample` without a known region
 * every product and sum its own fp32 round-to-nearest operation in this order.  pred_xstart and mean are not touched by the blend and
 * `sample` is stored once.  y0, mask (values in [0, 1]) and noise are device fp32 tensors of x's full shape [B, per_sample], all
 * required.  `tables` is a device fp32 array [S3D_KTAB_ROWS][T] of float64 schedule values cast to fp32 — sa = row SQRT_ACP_PREV,
 * sb = row SQRT_1M_ACP_PREV; the two other rows serve s3d_sampler_renoise.  The step's own y0 / mask (the reference's DDIM
 * x0 replacement) must be NULL and its mode is not S3D_STEP_MEAN_ONLY. */
enum { S3D_KTAB_SQRT_ACP_PREV = 0, S3D_KTAB_SQRT_1M_ACP_PREV, S3D_KTAB_SQRT_1M_BETA, S3D_KTAB_SQRT_BETA, S3D_KTAB_ROWS };
typedef struct {
    const float* y0;             /* [B, per_sample] the source latent on the target canvas           */
    const float* mask;           /* [B, per_sample] 1 = keep y0, 0 = free                            */
    const float* noise;          /* [B, per_sample] eps of the q_sample above                        */
    const float* tables;         /* [S3D_KTAB_ROWS][T] device fp32                                   */
} s3d_known_region;
/* s3d_sampler_step with the blend (the stand-alone kernel). */
S3D_API int s3d_sampler_step_known(const s3d_sampler_args* a, const s3d_known_region* known, void* stream);
/* s3d_unet_step_film_carry with the blend applied in the output head's launch; with S3D_CARRY_OUT the next step's in_conv is evaluated
 * on the BLENDED sample.  Identical bits to s3d_unet_forward_film followed by s3d_sampler_step_known.  model_out != NULL: the model
 * output is stored there and the step runs as output head + the stand-alone kernel (the in-head form stores neither the model output
 * nor the posterior mean: its registers hold the known-region pointers instead); S3D_CARRY_OUT then leaves nothing behind, and
 * step->mean is only accepted together with model_out. */
S3D_API int s3d_unet_step_film_known(s3d_unet* m, const float* film, int film_stride, int B, int H, int W, int D,
                       const s3d_sampler_args* step, const s3d_known_region* known, float* model_out, void* stream, int carry_flags);
/* One level of re-noising between two repeats of a step (RePaint's resampling): x_t = (sqrt(1 - beta_i) * x_prev) + (sqrt(beta_i) * noise)
 * with i = t[b], each operation rounded as above.  `known_tables` as in s3d_known_region; x_t may not alias its inputs' other rows. */
S3D_API int s3d_sampler_renoise(const float* x_prev, const float* noise, const float* known_tables, const int64_t* t, int32_t T,
                       int64_t batch, int64_t per_sample, float* x_t, void* stream);

/* Few-step sampling: the DPM-Solver++ multistep update, data prediction, orders 1 and 2M (DESIGN.md section 26 — no counterpart in
 * the reference, whose samplers are first order).  At schedule index i = t[b], with x0 formed as in s3d_sampler_step (the model output,
 * or (sr * x_t) - (srm1 * model_out) for S3D_MEAN_EPSILON; clamped to [-1, 1] when clip_denoised):
 *     s = (cx[i] * x_t) + (c0[i] * x0)
 *     s = s + (c1[i] * x0_prev)                order == 2; x0_prev: the previous step's pred_xstart
 *     s = s + (cn[i] * noise)                  noise != NULL (the SDE form)
 *     sample = s;  pred_xstart = x0
 * every product and sum its own fp32 round-to-nearest operation in this order.  `tables` is a device fp32 array [S3D_MTAB_ROWS][T] of
 * float64 values cast to fp32 (GaussianDiffusion.multistep_tables: they depend on the spacing of the kept steps); the step's own
 * `tables` serve sr / srm1 only.  `order` is 1 or 2, the same for the whole batch; with order == 1 x0_prev is not read and may be NULL.
 * x0_prev may not alias pred_xstart (a loop alternates two buffers).  Of s3d_sampler_args, mean_type, clip_denoised, T, batch,
 * per_sample, model_out, x, noise, t, tables, sample and pred_xstart are used; y0, mask and mean must be NULL and mode S3D_STEP_DDIM. */
enum { S3D_MTAB_CX = 0, S3D_MTAB_C0, S3D_MTAB_C1, S3D_MTAB_CN, S3D_MTAB_ROWS };
typedef struct {
    const float* x0_prev;        /* [B, per_sample] the previous step's pred_xstart (order 2)        */
    const float* tables;         /* [S3D_MTAB_ROWS][T] device fp32                                   */
    int32_t order;               /* 1 or 2                                                           */
} s3d_multistep;
/* The stand-alone kernel; known != NULL: the known-region blend (s3d_known_region) follows the update, `sample` is stored once. */
S3D_API int s3d_sampler_step_multistep(const s3d_sampler_args* a, const s3d_multistep* ms, const s3d_known_region* known /* may be NULL */,
                       void* stream);
/* s3d_unet_step_film_carry with the multistep update applied in the output head's launch (k_out_head_px_ms); with S3D_CARRY_OUT the
 * next step's in_conv is evaluated on the sample just formed.  Identical bits to s3d_unet_forward_film followed by
 * s3d_sampler_step_multistep.  The in-head form stores no model output: with model_out != NULL (and at widths the pixel-chunk head
 * does not take) the step runs as output head + the stand-alone kernel, and S3D_CARRY_OUT then leaves nothing behind.
 * The known-region blend is NOT fused into the head with this update (the known-region instantiations of the head already sit at the
 * scalar-register limit): such a step is s3d_unet_forward_film (model output stored) followed by s3d_sampler_step_multistep with
 * known != NULL, which is what the sampling loops do. */
S3D_API int s3d_unet_step_film_multistep(s3d_unet* m, const float* film, int film_stride, int B, int H, int W, int D,
                       const s3d_sampler_args* step, const s3d_multistep* ms, float* model_out, void* stream, int carry_flags);

/* ------------------------------------------------------------------------------------------
 * Leaf operators, exported so the parity tests can pin each kernel to the reference op it replaces
 * (SURVEY.md §8c item 3).  Planes are NCHW device tensors xy[B,C,H,W], xz[B,C,H,D], yz[B,C,W,D].
 * ------------------------------------------------------------------------------------------ */
/* TriplaneConv.forward  src/diffusion/unet_triplane.py:31-60; weights: 3 host OIHW tensors + biases */
S3D_API int s3d_op_triplane_conv(const float* const in[3], float* const out[3], int B, int C, int H, int W, int D,
                         int Cout, int ksize, int is_rollout, const float* const weight[3],
                         const float* const bias[3], void* stream);
/* TriplaneNorm + TriplaneSiLU  src/diffusion/unet_triplane.py:63-95; gamma/beta: host [C] per plane */
S3D_API int s3d_op_triplane_norm_silu(const float* const in[3], float* const out[3], int B, int C, int H, int W, int D,
                              const float* const gamma[3], const float* const beta[3], void* stream);
/* TriplaneDownsample2x / TriplaneUpsample2x / size-targeted bilinear resize
 * src/diffusion/unet_triplane.py:106-145, 494-499.  mode 0: avg-pool 2x2, 1: bilinear to (ho[i], wo[i]) */
S3D_API int s3d_op_triplane_resample(const float* const in[3], float* const out[3], int B, int C, const int hi[3],
                             const int wi[3], const int ho[3], const int wo[3], int mode, void* stream);
/* timestep_embedding  src/diffusion/nn.py:103-121; t: device [B] float, out: device [B][dim] = cos | sin */
S3D_API int s3d_op_timestep_embed(const float* t, int B, int dim, float* out, void* stream);
/* TriplaneResBlock._forward  src/diffusion/unet_triplane.py:269-311 (constructor :175-267), run through the model's own
 * block code.  emb: device [B][emb_dim] (the time_embed output); parameters by state-dict name relative to the block
 * ("in_layers.0.norm_xy.weight", "in_layers.2.conv_xy.weight", "emb_layers.1.weight", "out_layers.0...",
 * "out_layers.2...", "skip_connection.conv_xy.weight" when C != Cout), host pointers in PyTorch layouts */
S3D_API int s3d_op_triplane_resblock(const float* const in[3], float* const out[3], const float* emb, int B, int C,
                             int Cout, int H, int W, int D, int emb_dim, int use_scale_shift_norm, int is_rollout,
                             const char* const* names, const float* const* tensors, int n_tensors, void* stream);

/* ------------------------------------------------------------------------------------------
 * Decoder: AutoEncoderGroupSkip.decode + ShapeAutoEncoder.decode_batch/decode_grid
 *   src/encoding/networks.py:192-220 ; src/encoding/model.py:319-349 ; src/encoding/utils3d.py:13-25
 * ------------------------------------------------------------------------------------------ */
typedef struct s3d_decoder s3d_decoder;

typedef struct {
    int32_t geo_feat_channels;   /* 4   */
    int32_t tex_feat_channels;   /* 8   */
    int32_t feat_channel_up;     /* 64  */
    int32_t mlp_hidden_channels; /* 256 */
    int32_t mlp_hidden_layers;   /* 4   */
    int32_t tex_channels;        /* 3   */
} s3d_decoder_cfg;

S3D_API int s3d_decoder_create(const s3d_decoder_cfg* cfg, s3d_decoder** out);
/* The decoder's other networks (s3d_decoder_create is variant 0); every other s3d_decoder_* call works on any variant, its
 * `out` rows being s3d_decoder_out_channels floats wide.
 *   0  AutoEncoderGroupSkip, use_tex=True (tex_channels 1..8)           out = [sdf | sigmoid(tex[tex_channels])]
 *   1  geometry only (use_tex=False of the skip or the PBR net: the same geo network; feature maps of geo_feat_channels)
 *                                                                        out = [sdf]
 *   2  AutoEncoderGroupPBR, use_tex=True (src/encoding/networks.py:227-316: tex_convs = two 3x3 blocks, the second on its
 *      normalised input; rgb / mr / normal heads on one gathered feature)   out = [sdf | rgb 3 | mr 2 | normal 3], no sigmoid
 * clamp_color clamps columns >= 1 to [0,1] in every variant. */
S3D_API int s3d_decoder_create_variant(const s3d_decoder_cfg* cfg, int32_t variant, s3d_decoder** out);
S3D_API int s3d_decoder_out_channels(const s3d_decoder* d);
S3D_API void s3d_decoder_destroy(s3d_decoder* d);
S3D_API int s3d_decoder_num_params(const s3d_decoder* d);
S3D_API int s3d_decoder_param_info(const s3d_decoder* d, int i, const char** name, int64_t shape[4], int* ndim);
S3D_API int s3d_decoder_set_param(s3d_decoder* d, const char* name, const float* data, const int64_t* shape, int ndim);
/* Runs geo_convs / tex_convs once for a triplane (the reference redoes them for every 16 384-point
 * chunk, src/encoding/model.py:327-330 -> networks.py:203-212, with identical results).
 * xy [1,Cg+Ct,H,W], xz [1,Cg+Ct,H,D], yz [1,Cg+Ct,W,D] device fp32. */
S3D_API int s3d_decoder_prepare_triplane(s3d_decoder* d, const float* xy, const float* xz, const float* yz,
                                 int H, int W, int D, void* stream);
/* The prepared features of one plane as the reference's NCHW map: out device [feat_channel_up][h][w].
 * group 0 geo_convs, 1 tex_convs; 2 (variant 2 only) the texture planes after tex_convs.0. */
S3D_API int s3d_decoder_plane_features(s3d_decoder* d, int group, int plane, float* out, void* stream);
/* net.decode(points, feat_maps, aabb): pts [N,3] device, aabb[6] host -> out [N, 1+tex_channels]
 * = (sdf, sigmoid(rgb)); clamp_color != 0 additionally applies decode_batch's clamp(0,1) (:332). */
S3D_API int s3d_decoder_decode_points(s3d_decoder* d, const float* pts, int64_t N, const float aabb[6],
                              int clamp_color, float* out, void* stream);
/* decode_grid: cell-centred grid over aabb with res_i = floor(reso*size_i/max(size)); writes
 * out [res0,res1,res2, 1+tex_channels] and the three resolutions. */
S3D_API int s3d_decoder_grid_dims(const float aabb[6], int reso, int dims[3]);
S3D_API int s3d_decoder_decode_grid(s3d_decoder* d, int reso, const float aabb[6], float* out, void* stream);
/* The sdf of the geometry head and its exact gradient with respect to the point, in world units: pts [N,3] device ->
 * sdf [N] (the bits of decode_points' column 0), grad [N,3] = d sdf / d p with F.grid_sample's autograd conventions for
 * padding_mode='border', align_corners=False (0 beyond a border, the floor cell at a texel centre) and relu'(0) = 0.
 * iters > 0 first runs that many Newton steps onto the zero level set, p <- p - clamp(sdf g / |g|^2, +-max_step) per
 * component (no move where |g|^2 < 1e-20), the displacement from the start clamped to +-max_move per component; pts_out
 * [N,3] receives the final points, and sdf and grad belong to them: iters + 1 evaluations, each two launches on `stream`
 * (the geometry head through the decode kernel for the sdf, then the gradient kernel), no host synchronisation.
 * Needs a prepared triplane; every variant (the texture group is not touched).  S3D_ERR_INVALID for iters < 0, a null
 * pts_out with iters > 0, non-positive max_step / max_move with iters > 0; S3D_ERR_UNSUPPORTED for the widths decode_points
 * refuses; all checked before any device call.  N == 0 is a no-op. */
S3D_API int s3d_decoder_sdf_grad(s3d_decoder* d, const float* pts, int64_t N, const float aabb[6], int iters, float max_step,
                         float max_move, float* pts_out, float* sdf, float* grad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training tier: what the reference gets from autograd + torch.optim for
 * GaussianDiffusion.training_losses (src/diffusion/gaussian_diffusion.py:771-856) and
 * TrainLoop.run_step (src/diffusion/train_util.py:163-247).
 *
 * Parameters live in ONE caller-owned flat fp32 device vector: the state-dict tensors in the order of
 * s3d_unet_param_info(), each in its PyTorch layout, tightly packed (6 989 860 floats at 64 channels).
 * Gradients, Adam moments and EMA copies use the same layout, so the optimizer is one kernel and a
 * data-parallel job needs one all-reduce of the gradient vector.
 * ------------------------------------------------------------------------------------------------ */
S3D_API int64_t s3d_unet_param_numel(const s3d_unet* m);
S3D_API int s3d_unet_param_offset(const s3d_unet* m, int index, int64_t* offset);
/* Make `params` (device, numel floats) the master copy.  The library keeps the pointer (not the memory) until the
 * handle is destroyed or another vector is attached.  Call s3d_unet_repack after every change of its contents. */
S3D_API int s3d_unet_train_attach(s3d_unet* m, float* params, int64_t numel);
/* Rebuild the kernel-layout weight image (and the transposed operators of the backward pass) from the attached
 * vector: one launch on `stream`. */
S3D_API int s3d_unet_repack(s3d_unet* m, void* stream);
/* model(x, t, H, W, D) keeping the activations for one s3d_unet_backward.  Same result as s3d_unet_forward. */
S3D_API int s3d_unet_forward_train(s3d_unet* m, const float* x, const float* t, int B, int H, int W, int D, float* out,
                                   void* stream);
/* d_out: gradient of the composed output [B,Cout,H+D,W+D].  grads: numel floats, every element is overwritten
 * (= the .grad of each parameter after loss.backward() from zeroed gradients). */
S3D_API int s3d_unet_backward(s3d_unet* m, const float* d_out, float* grads, void* stream);
/* The same with progress marks for a data-parallel trainer that overlaps the gradient all-reduce with the backward pass
 * (the reference's DDP is commented out, src/diffusion/train_util.py:8-9, 98-99): events[k] (HIP events
 * owned by the caller, n_events <= 2) are recorded when a group of gradients is final — [0] out.* and output_blocks.* except
 * their emb_layers, [1] input_blocks.* except their emb_layers and in_conv.*; time_embed.* and all emb_layers.* are final when
 * the call's work on `stream` is.  (Recorded on `stream`, or — option BWD_SIDE on, the default — on the handle's side stream, which
 * finishes a group last and has been ordered behind `stream`'s progress: wait for the EVENT, as a communication stream does.) */
S3D_API int s3d_unet_backward_marked(s3d_unet* m, const float* d_out, float* grads, void* stream, void** events, int n_events);

/* q_sample (:189-207): x_t = sqrt_ac[t] * x0 + sqrt_1mac[t] * noise; tables fp32 [T] on the device, t int64 [B].
 * x0_batch_stride: elements between the batch rows of x0 — per_sample, or 0 when the batch is ONE training triplane expanded
 * (what the reference's data iterator yields, src/utils/triplane_util.py:64-69): no materialised copy of the batch is needed. */
S3D_API int s3d_train_q_sample(const float* x0, int64_t x0_batch_stride, const float* noise, const float* sqrt_ac,
                               const float* sqrt_1mac, const int64_t* t, int B, int64_t per_sample, float* x_t, void* stream);
/* terms[b][0..2] = mean((target_p - out_p)^2) over plane p = xy, xz, yz of the composed maps (:838-845), terms[b][3] =
 * (xy + xz) + yz, the reference's terms["loss"] in its order (:851); terms: [B][4]; workspace: 96*B floats;
 * target_batch_stride: C*(H+D)*(W+D), or 0 for one target shared by the batch */
S3D_API int s3d_train_mse_terms(const float* model_out, const float* target, int64_t target_batch_stride, int B, int C, int H,
                                int W, int D, float* workspace, float* terms, void* stream);
/* d_out = d( sum_{b,p} w[b][p] * terms[b][p] ) / d model_out with w[b][p] = weight[b][weight_cols == 3 ? p : 0] /
 * weight_divisor; weight: [B][weight_cols] on the device, weight_cols 1 or 3 (the trainer's loss = mean_b(weights[b] *
 * loss[b]) is weight_cols 1, weight_divisor B: train_util.py:229) */
S3D_API int s3d_train_mse_grad(const float* model_out, const float* target, int64_t target_batch_stride, const float* weight,
                               int weight_cols, float weight_divisor, int B, int C, int H, int W, int D, float* d_out,
                               void* stream);
/* torch.optim.AdamW step `step` (1-based) on the flat vectors, then update_ema (src/diffusion/nn.py:55-65) of up to
 * 4 EMA copies (device pointers in a host array). */
S3D_API int s3d_train_adamw_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* const* ema,
                                const float* ema_rates, int n_ema, int64_t numel, float lr, float beta1, float beta2,
                                float eps, float weight_decay, int step, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Auto-encoder training tier: AutoEncoderGroupSkip encode / decode / losses and their
 * gradients (src/encoding/networks.py:122-220, src/encoding/model.py:178-237).  Reuses s3d_decoder_cfg.
 * Variants (the numbers of s3d_decoder_create_variant):
 *   0  the skip net with texture, tex_channels 1..8 (3: data_type sdftex; 8: sdfpbr with --enc_net_type skip);
 *      volume 1 + tex_channels channels, pred = sdf | sigmoid(tex)
 *   1  geometry only (use_tex=False of either class, data_type sdf): the tex_* fields are ignored, 1-channel volume,
 *      pred = sdf, no tex group (tex_group_begin == the total size), tex may be null
 *   2  the PBR net: S3D_ERR_UNSUPPORTED from s3d_ae_create_variant; s3d_ae_create_pbr makes it (see there)
 * Parameters: one caller-owned flat fp32 device vector, tensors in s3d_ae_param_info() order and PyTorch layouts:
 * [geo_encoder, geo_convs, geo_decoder | tex_encoder, tex_convs, tex_decoder] — the two halves are the reference's two
 * AdamW parameter groups (networks.py:146-150); use s3d_train_adamw_ema on each half with its learning rate.
 * ------------------------------------------------------------------------------------------------ */
typedef struct s3d_ae s3d_ae;
typedef struct {
    int32_t sdf_loss;            /* 0 = l1, 1 = weightedl1 (default) */
    int32_t tex_loss;            /* 0 = l1 (default), 1 = l2, 2 = huber(delta 0.1) */
    float sdf_threshold;         /* truncation of the sdf samples */
    float tex_threshold_ratio;   /* texture loss on points with |sdf| < sdf_threshold * ratio (0.999), the product taken
                                  * in float on the two float fields.  The reference rounds the double product once to
                                  * float; the Python binding (encoding/model.py:ae_loss_cfg) matches it by passing that
                                  * rounded product as sdf_threshold with a ratio of 1.0. */
    float tex_weight;            /* 1.0 */
} s3d_ae_loss_cfg;

S3D_API int s3d_ae_create(const s3d_decoder_cfg* cfg, s3d_ae** out);               /* variant 0 */
S3D_API int s3d_ae_create_variant(const s3d_decoder_cfg* cfg, int variant, s3d_ae** out);
/* AutoEncoderGroupPBR with texture (networks.py:227-333; data_type sdfpbr with --enc_net_type pbr): tex_convs = two 3x3 blocks,
 * the second normalising its input with the norm_p it also applies to its hidden maps; rgb / mr / normal heads on one gathered
 * feature; a 9-channel volume, pred = sdf | rgb 3 | mr 2 | normal 3 with NO sigmoid.  The handle is taken by every s3d_ae_* call
 * but s3d_ae_loss_grads (four losses: s3d_ae_loss_grads_groups).  The tex group is [tex_encoder, tex_convs.0, tex_convs.1,
 * rgb_decoder, mr_decoder, normal_decoder] (networks.py:260-262).  S3D_ERR_UNSUPPORTED unless tex_channels == 8, the widths
 * are multiples of 32, mlp_hidden_layers == 4 and the feature groups are multiples of 4 channels, at most 12 together. */
S3D_API int s3d_ae_create_pbr(const s3d_decoder_cfg* cfg, s3d_ae** out);
S3D_API int s3d_ae_out_channels(const s3d_ae* a);               /* floats per row of pred: 1 + tex_channels, 1 for variant 1, 9 for the PBR net */
S3D_API void s3d_ae_destroy(s3d_ae* a);
S3D_API int s3d_ae_num_params(const s3d_ae* a);
S3D_API int s3d_ae_param_info(const s3d_ae* a, int i, const char** name, int64_t shape[5], int* ndim, int64_t* offset);
/* total floats; *tex_group_begin = first float of the tex_* parameter group */
S3D_API int64_t s3d_ae_param_numel(const s3d_ae* a, int64_t* tex_group_begin);
S3D_API int s3d_ae_attach(s3d_ae* a, float* params, int64_t numel);
S3D_API int s3d_ae_repack(s3d_ae* a, void* stream);              /* after every change of the attached vector */
/* The training volume [1,C,2H,2W,2D] (device, C = s3d_ae_out_channels: sdf, texture): reduced once to the three
 * projections the encoder needs; the volume itself is not kept. */
S3D_API int s3d_ae_set_volume(s3d_ae* a, const float* vol, int C, int X2, int Y2, int Z2, void* stream);
/* net.encode(vol): xy [1,Cg+Ct,H,W], xz [1,Cg+Ct,H,D], yz [1,Cg+Ct,W,D] */
S3D_API int s3d_ae_encode(s3d_ae* a, float* xy, float* xz, float* yz, void* stream);
/* net(vol, pts): pred [N, s3d_ae_out_channels] (texture through the sigmoid) */
S3D_API int s3d_ae_forward(s3d_ae* a, const float* pts, int64_t N, const float aabb[6], float* pred, void* stream);
/* _forward_batch + backward: losses[2] = {sdf_loss, tex_loss} (device), pred optional, grads = d(sdf_loss+tex_loss)/d params
 * (every element overwritten).  pts [N,3], sdf [N,1], tex [N,tex_channels] device. */
S3D_API int s3d_ae_loss_grads(s3d_ae* a, const float* pts, const float* sdf, const float* tex, int64_t N, const float aabb[6],
                              const s3d_ae_loss_cfg* cfg, float* losses, float* pred, float* grads, void* stream);
/* The same with the texture loss per column group: losses[4] = {sdf, rgb, mr, normal}, grads = the gradient of their sum.
 * With 8 texture channels (data_type sdfpbr, model.py:226-233) rgb = columns 0-2, mr = 3-4 and normal = 5-7 are each their own
 * mean over (points inside the band x its columns) times tex_weight; any other width is one group (losses[1], the sdftex
 * loss; losses[2..3] = 0); variant 1 has no texture term (losses[1..3] = 0, tex may be null). */
S3D_API int s3d_ae_loss_grads_groups(s3d_ae* a, const float* pts, const float* sdf, const float* tex, int64_t N, const float aabb[6],
                                     const s3d_ae_loss_cfg* cfg, float* losses, float* pred, float* grads, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Iso-surface extraction: marching cubes on the device, replacing
 * `mcubes.marching_cubes(np.pad(grid, 1, constant_values=pad_value), iso)` and `v -= 1`
 * (src/encoding/utils3d.py:196-203).  Two calls because the output size is data dependent.
 * grid: value of vertex (x,y,z) at grid[((x*Y + y)*Z + z) * stride] (stride 4 reads the sdf channel of a
 * decode_grid output in place; its other channels can be interpolated onto the vertices as attributes).
 * Vertex coordinates are grid-index coordinates of the unpadded grid; triangles index the vertex array; normals
 * (right-hand rule) point from values < iso to values > iso.  Parity with PyMCubes is unpinned.
 * ------------------------------------------------------------------------------------------------ */
typedef struct s3d_mc s3d_mc;
S3D_API int s3d_mc_create(s3d_mc** out);
S3D_API void s3d_mc_destroy(s3d_mc* m);
/* pass 1: classify and scan; synchronises `stream` to return the counts.  pad = 1 surrounds the grid with pad_value.
 * 3 (X + 2 pad)(Y + 2 pad)(Z + 2 pad) >= 2^31 is refused with S3D_ERR_UNSUPPORTED before anything is allocated or launched. */
S3D_API int s3d_mc_count(s3d_mc* m, const float* grid, int X, int Y, int Z, int stride, float iso, int pad, float pad_value,
                         int64_t* n_verts, int64_t* n_tris, void* stream);
/* pass 2: verts [n_verts][3], attrs [n_verts][n_attr] or null (channels 1..n_attr of the grid), tris [n_tris][3] */
S3D_API int s3d_mc_extract(s3d_mc* m, float* verts, float* attrs, int n_attr, int32_t* tris, void* stream);
/* Connected components of an indexed triangle mesh (the `pcu.connected_components` step of sdfgrid_to_mesh,
 * src/encoding/utils3d.py:204-208): labels[v] = smallest vertex index of v's component.  tris [n_tris][3], labels
 * [n_verts] on the device; synchronises `stream` (iterates to a fixed point). */
S3D_API int s3d_mesh_components(const int32_t* tris, int64_t n_tris, int64_t n_verts, int32_t* labels, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Narrow-band iso-surface extraction: the mesh of s3d_mc_* from the bricks the surface crosses only.
 * Padded vertex space as above with pad = 1: P = dims + 2 vertices per axis, vertex p holds sample p - 1 or pad_value.
 * Brick b holds the padded vertices [b B, b B + B) per axis (B = 4, 8 or 16; nb = ceil(P / B), the last brick may be partial).
 * The caller owns the sample pool [slot][B^3][stride] (value in channel 0, attributes after it; local order lx, ly, lz): a
 * brick gets a slot when it becomes active, slots are append-only, s3d_mcs_pending names the samples of the newest slots.
 * A cell is extracted iff the bricks of all eight of its corners are active; the result is the dense mesh without the
 * triangles of the other cells and without the vertices nothing references any more, in the dense order (vertices by
 * edge axis, then padded linear vertex index; triangles by padded linear cell index), linear indices in 64 bits.
 * Order of calls: plan, seed, then {pending, the caller fills the pool, grow} until grow reports no boundary cut edge,
 * count, extract, occupancy.  Every call but pending / extract / occupancy synchronises `stream`.
 * ------------------------------------------------------------------------------------------------ */
#define S3D_MCS_MAX_BRICKS (1 << 27)           /* nb^3: the brick table and its scans, 512 MiB each */
#define S3D_MCS_MAX_SAMPLES (1 << 30)          /* slots * B^3: pool entries (a 32-bit item count in the scans and sorts) */
typedef struct s3d_mcs s3d_mcs;
S3D_API int s3d_mcs_create(s3d_mcs** out);
S3D_API void s3d_mcs_destroy(s3d_mcs* m);
/* Forgets every slot.  nb[3]: bricks per axis.  pad must be 1.  More than S3D_MCS_MAX_BRICKS bricks: S3D_ERR_UNSUPPORTED, before
 * anything is allocated. */
S3D_API int s3d_mcs_plan(s3d_mcs* m, int X, int Y, int Z, int block, int pad, float pad_value, float iso, int nb[3]);
/* lattice: the field on the brick corners, [(nb0+1)][(nb1+1)][(nb2+1)][lattice_stride] with the value in channel 0, point
 * (i,j,k) at unpadded index coordinates i B - 1.5; the points outside [-0.5, dims - 0.5] are replaced by pad_value here.
 * A brick is a seed iff `value < iso` differs among its eight corners; dilate adds the 26-neighbourhood that many times.
 * all_active != 0: every brick is activated and lattice is not read (may be null).  n_new bricks got slots [0, n_new). */
S3D_API int s3d_mcs_seed(s3d_mcs* m, const float* lattice, int lattice_stride, int dilate, int all_active, int64_t* n_seed,
                         int64_t* n_new, void* stream);
/* coords [n_new * B^3][3]: the unpadded index coordinates of the pool entries of the newest slots, in pool order.  An entry
 * that is a pad vertex or lies beyond P is never read from the pool; its coordinates are clamped into the grid. */
S3D_API int s3d_mcs_pending(s3d_mcs* m, float* coords, void* stream);
/* The boundary pass over every slot (pool holds all of them): n_boundary cut edges have an extracted and a non-extracted cell
 * around them; with activate != 0 the bricks of all corners of those non-extracted cells are activated, n_new of them new (slots
 * appended), with activate = 0 the edges are only counted.  More than S3D_MCS_MAX_SAMPLES pool entries: S3D_ERR_UNSUPPORTED. */
S3D_API int s3d_mcs_grow(s3d_mcs* m, const float* pool, int stride, int activate, int64_t* n_boundary, int64_t* n_new, void* stream);
S3D_API int s3d_mcs_count(s3d_mcs* m, const float* pool, int stride, int64_t* n_verts, int64_t* n_tris, void* stream);
/* verts [n_verts][3], attrs [n_verts][n_attr] or null (channels 1..n_attr of the pool), tris [n_tris][3]: the expressions of
 * s3d_mc_extract, so with every brick active the bits of s3d_mc_count / s3d_mc_extract on the dense grid */
S3D_API int s3d_mcs_extract(s3d_mcs* m, float* verts, float* attrs, int n_attr, int32_t* tris, void* stream);
/* occ [X][Y][Z] uint8: `value < iso` from the pool in active bricks, the first lattice corner's in the others */
S3D_API int s3d_mcs_occupancy(s3d_mcs* m, const float* pool, int stride, uint8_t* occ, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Textured mesh export: the device half of what follows the iso-surface in decode_texmesh
 * (src/encoding/model.py:389-430) — decimation, texel positions of a UV atlas, texture finishing.  An own design
 * (vertex clustering, an analytic per-face atlas): parity with open3d / xatlas / nvdiffrast is not claimed.
 * Sorting, unique and compaction between these calls are the caller's (sin3dm_amd/encoding/isosurface.py).
 * All arrays are device pointers unless marked host; every call only enqueues on `stream`.
 * ------------------------------------------------------------------------------------------------ */
/* keys[v] = ((ix * dims[1]) + iy) * dims[2] + iz, the cell of vertex v on a uniform grid: per axis
 * min(dims[a] - 1, floor((verts[v][a] - origin[a]) / cell)) in fp32 (correctly rounded division).  origin, dims: host. */
S3D_API int s3d_mesh_cluster_keys(const float* verts, int64_t n_verts, const float origin[3], float cell, const int dims[3],
                                  int64_t* keys, void* stream);
/* out[k][c] = mean of vals[order[j]][c] for j in [seg[k], seg[k+1]), added in that order (double accumulator).
 * vals [n_verts][channels], order [n_verts] (vertex indices sorted by key), seg [n_clusters + 1]. */
S3D_API int s3d_mesh_cluster_means(const float* vals, int channels, const int64_t* order, const int64_t* seg, int64_t n_clusters,
                                   int64_t n_verts, float* out, void* stream);
/* out_tris[f] = vmap[tris[f]]; face_keys[f] = the face's vertex set as one integer, (lo * n_clusters + mid) * n_clusters + hi,
 * or -1 when two of its indices are equal.  n_clusters <= 2^20. */
S3D_API int s3d_mesh_remap_faces(const int32_t* tris, int64_t n_tris, const int32_t* vmap, int64_t n_verts, int64_t n_clusters,
                                 int32_t* out_tris, int64_t* face_keys, void* stream);
/* corner0[f] in {0,1,2}: the vertex of face f opposite its longest edge (ties: the first of v0v1, v1v2, v2v0). */
S3D_API int s3d_tex_face_corner0(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_faces, int32_t* corner0,
                                 void* stream);
/* The atlas: cells_per_row^2 square cells of `cell` texels, face k in cell k / 2 (row-major), even k in the lower chart
 * (1,1) (c-4,1) (1,c-4), odd k in the upper chart (c-1,c-1) (4,c-1) (c-1,4) (texels from the cell origin, c = cell).
 * For every texel (x, y) at index y * texreso + x: face_id = the face whose closed chart holds the centre (x+.5, y+.5), or -1;
 * pos = b0 V0 + b1 V1 + b2 V2 (zeros where face_id is -1), lower chart b1 = (x+.5-1)/(c-5), b2 = (y+.5-1)/(c-5), b0 = 1-b1-b2,
 * upper chart mirrored; V0 = the corner0 vertex, V1, V2 follow in the face's cyclic order.  face_id [T*T], pos [T*T][3]. */
S3D_API int s3d_tex_texel_positions(const float* verts, int64_t n_verts, const int32_t* tris, const int32_t* corner0, int64_t n_faces,
                                    int texreso, int cells_per_row, int cell, int32_t* face_id, float* pos, void* stream);
/* image [T*T][channels] uint8 = 0, then image[texel_index[i]][c] = uint8(colors[i][c] * 255) (truncated; clamped to 0..255) */
S3D_API int s3d_tex_quantize(const float* colors, const int64_t* texel_index, int64_t n, int channels, int texreso, uint8_t* image,
                             void* stream);
/* out = image where face_id >= 0, elsewhere the per-channel maximum of image over the 3 x 3 neighbourhood inside the atlas
 * (cv2.dilate with a 3 x 3 kernel blended by the mask, model.py:426-428).  out must not alias image. */
S3D_API int s3d_tex_dilate(const uint8_t* image, const int32_t* face_id, int texreso, int channels, uint8_t* out, void* stream);
/* Tangent-space normal map of a field on the atlas (an own addition).  image [T*T][3] = (128, 128, 255) and
 * status [T*T] = 0 first; then for every i < n, texel texel_index[i] (all different; one outside [0, T*T) or under no chart is
 * skipped): the unit gradient grad[i] / |grad[i]| in the frame (T', B', N) of s3d_pbr_shade on the texel's face, byte =
 * floor(clamp((t + 1) * 127.5, 0, 255) + 0.5).  Face and barycentrics as in s3d_tex_texel_positions.  N: the normalised mix of
 * base_normals [n_verts][3] at the barycentrics, turned to the gradient's side of the face; the face normal on that side when
 * base_normals is null, a corner's normal is zero, or the mix has no direction or points away from it.  tangents [n_faces][2][3]
 * as s3d_pbr_face_tangents writes them.  status: 1 encoded, 4 encoded around the face normal, 2 flat texel because the gradient
 * is not finite or |grad|^2 < 1e-20, 3 flat texel because the face has no area or no tangent.  Float64 after the barycentrics. */
S3D_API int s3d_tex_normal_texels(const float* grad, const int64_t* texel_index, int64_t n, const float* verts, int64_t n_verts,
                                  const int32_t* tris, const int32_t* corner0, int64_t n_faces, int texreso, int cells_per_row, int cell,
                                  const float* base_normals, const float* tangents, uint8_t* image, uint8_t* status, void* stream);
/* out = image where face_id >= 0; elsewhere the whole texel of the first covered neighbour inside the atlas in the order (dx, dy) =
 * (0,-1) (-1,0) (+1,0) (0,+1) (-1,-1) (+1,-1) (-1,+1) (+1,+1); image itself where there is none.  out must not alias image. */
S3D_API int s3d_tex_dilate_nearest(const uint8_t* image, const int32_t* face_id, int texreso, int channels, uint8_t* out, void* stream);

/* Quadric-error decimation (Garland-Heckbert edge collapse in parallel rounds of independent collapses, DESIGN.md §15;
 * isosurface.simplify_mesh_quadric drives the rounds and does the sorting, unique and compaction in between).
 * A quadric is the upper triangle of a symmetric 4 x 4 matrix as 10 doubles: xx xy xz xw yy yz yw zz zw ww.  Edges are
 * (edge_u[e] < edge_v[e]).  CSR lists: nbr_off [n_verts + 1] into nbr [n_nbr] (the neighbours of a vertex, ascending),
 * vf_off [n_verts + 1] into vf_face [3 n_tris] (the faces at a vertex, ascending).  No floating-point atomics. */
/* quadrics[v] = sum over the faces at v, in the order of vf_face, of area * p p^T, p the unit plane (faces without area skipped) */
S3D_API int s3d_mesh_qem_quadrics(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, const int64_t* vf_off,
                                  const int32_t* vf_face, double* quadrics, void* stream);
/* Per edge, with Q = Q_u + Q_v = [A b; b^T c]: target = -A^-1 b (double) where |det A| > 1e-6 (trace A / 3)^3 and the solution
 * lies within 2 edge lengths of the midpoint; else the midpoint, unless u (then v) is cheaper by more than
 * 1e-10 trace A (1 + |mid|^2).  cost = fp32(max(0, target^T Q target)), target [n_edges][3] rounded to fp32. */
S3D_API int s3d_mesh_qem_edge_cost(const float* verts, int64_t n_verts, const double* quadrics, const int32_t* edge_u,
                                   const int32_t* edge_v, int64_t n_edges, float* target, float* cost, void* stream);
/* frozen[w] = 1 iff w lies on an edge with edge_faces != 2.  flags[e] = 1 (edge_faces[e] == 2) | 2 (no frozen endpoint)
 * | 4 (link condition: exactly two common neighbours w1, w2, and not both faces u w1 w2 and v w1 w2) | 8 (every face at u or v
 * that does not hold both keeps, with that vertex at target[e], a non-zero area and cos(old normal, new normal) > 0.2).
 * An edge may collapse iff flags == 15. */
S3D_API int s3d_mesh_qem_edge_valid(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, const int32_t* edge_u,
                                    const int32_t* edge_v, const int32_t* edge_faces, int64_t n_edges, const int64_t* nbr_off,
                                    const int32_t* nbr, int64_t n_nbr, const int64_t* vf_off, const int32_t* vf_face, const float* target,
                                    uint8_t* frozen, int32_t* flags, void* stream);
/* keys[e] = (bits of cost[e] << 32) | mix(e), mix(i): i *= 0x9E3779B1, i ^= i >> 16, i *= 0x85EBCA6B, i ^= i >> 13 on 32 bits
 * (a bijection: equal costs are ordered by a scattered, not an ascending, index); m1[w] = min key of the edges with flags == 15 at w (integer atomic minimum,
 * 2^63 - 1 where there is none); m2[w] = min of m1 over w and its neighbours; selected[e] = flags == 15 and
 * keys[e] == m2[u] == m2[v].  No two selected edges have equal or adjacent endpoints.  n_edges < 2^32. */
S3D_API int s3d_mesh_qem_select(const int32_t* edge_u, const int32_t* edge_v, const float* cost, const int32_t* flags, int64_t n_edges,
                                const int64_t* nbr_off, const int32_t* nbr, int64_t n_nbr, int64_t n_verts, int64_t* keys, int64_t* m1,
                                int64_t* m2, uint8_t* selected, void* stream);
/* For every edge e = chosen[k] (pairwise non-adjacent, as selected above): verts[u] = target[e], quadrics[u] += quadrics[v],
 * attrs[u] = (1 - t) attrs[u] + t attrs[v] with t in [0, 1] the parameter of the target on the segment u v, vmap[v] = u.
 * attrs [n_verts][n_attr] or null with n_attr = 0. */
S3D_API int s3d_mesh_qem_apply(const int64_t* chosen, int64_t n_chosen, const int32_t* edge_u, const int32_t* edge_v, int64_t n_edges,
                               const float* target, float* verts, int64_t n_verts, double* quadrics, float* attrs, int n_attr,
                               int32_t* vmap, void* stream);
/* out_tris[f] = vmap[tris[f]]; keep[f] = 1 unless two of its indices are now equal */
S3D_API int s3d_mesh_qem_remap_faces(const int32_t* tris, int64_t n_tris, const int32_t* vmap, int64_t n_verts, int32_t* out_tris,
                                     uint8_t* keep, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh to training data: what the reference's data/mesh_sampler.py computes with point_cloud_utils and
 * trimesh — clipped signed distance, colour of the closest surface point, area-weighted surface samples — by an own
 * design; parity with those libraries is not claimed.  The distance is exact inside a band (a uniform cell grid holds, per
 * cell, the triangles whose band-dilated box overlaps it) and equals the band outside; the sign is the caller's, from the
 * generalized winding number.  Triangles are passed as their nine corner floats, tri9 [n_faces][9] = {a, b, c}.  The cell
 * grid: cell (ix, iy, iz) = per axis min(dims - 1, max(0, floor((x - origin) / cell))), linear index (ix * dims[1] + iy) *
 * dims[2] + iz; origin and dims are host arrays.  Scan, sort and segment starts between the calls are the caller's
 * (sin3dm_amd/data/mesh_sampler.py).  All other arrays are device pointers; every call only enqueues on `stream`.
 * ------------------------------------------------------------------------------------------------ */
#define S3D_MESHSDF_MAX_CELLS (1LL << 28)
/* cap of the (cell, triangle) pair list: 2^27 pairs = 1.5 GiB of workspace (an int64 cell key and an int32 triangle per pair) */
#define S3D_MESHSDF_MAX_PAIRS (1LL << 27)
/* counts[f] = number of cells the box of triangle f, dilated by a little more than `band`, overlaps */
S3D_API int s3d_meshsdf_bin_count(const float* tri9, int64_t n_faces, float band, const float origin[3], float cell, const int dims[3],
                                  int64_t* counts, void* stream);
/* offsets [n_faces] = exclusive scan of counts, n_pairs = their sum (more than S3D_MESHSDF_MAX_PAIRS: S3D_ERR_UNSUPPORTED).
 * Triangle f writes (pair_cell, pair_tri) = (cell index, f) at offsets[f]... in ascending cell order. */
S3D_API int s3d_meshsdf_bin_fill(const float* tri9, int64_t n_faces, float band, const float origin[3], float cell, const int dims[3],
                                 const int64_t* offsets, int64_t n_pairs, int64_t* pair_cell, int32_t* pair_tri, void* stream);
/* seg [cells + 1]: the pairs sorted by cell, cell c owns seg_tri[seg[c] .. seg[c+1]).  Per point: dist = distance to the closest
 * point of those triangles (Ericson's region test, fp32; equal squared distances: the lower face index), face, bary [n][3] with
 * closest = sum bary[k] * corner k.  Nothing nearer than band: dist = band, face = -1, bary = 0.  A point outside the grid
 * looks the nearest border cell up. */
S3D_API int s3d_meshsdf_closest(const float* points, int64_t n_points, const float* tri9, int64_t n_faces, float band, const float origin[3],
                                float cell, const int dims[3], const int64_t* seg, const int32_t* seg_tri, int64_t n_pairs, float* dist,
                                int32_t* face, float* bary, void* stream);
/* wn[i] = sum over the faces, in index order, of the solid angle of face f seen from point i (Van Oosterom-Strackee), / 4 pi */
S3D_API int s3d_meshsdf_winding(const float* points, int64_t n_points, const float* tri9, int64_t n_faces, float* wn, void* stream);
S3D_API int s3d_meshsdf_face_areas(const float* tri9, int64_t n_faces, float* areas, void* stream);
/* cdf [n_faces] (double): inclusive sums of the face areas.  uniforms [n][3] in [0, 1): u0 picks the first face with cdf > u0 *
 * cdf[n_faces - 1], bary = (1 - sqrt(u1), sqrt(u1) (1 - u2), sqrt(u1) u2).  points [n][3], face [n], bary [n][3]. */
S3D_API int s3d_meshsdf_sample_surface(const float* tri9, int64_t n_faces, const double* cdf, const float* uniforms, int64_t n,
                                       float* points, int32_t* face, float* bary, void* stream);
/* colors [n][3] in [0, 1]: uv [n_faces][3][2] per corner, interpolated with bary; material m = face_mat[f]; mat_table [n_mats][3]
 * = {byte offset into images, W, H} of tightly packed 8-bit RGB rows (W = 0: no image), mat_kd [n_mats][3].  Texel x =
 * round(u (W - 1)) mod W, y = round((1 - v) (H - 1)) mod H (half to even), colour = byte / 255; no image: Kd; face -1: 0. */
S3D_API int s3d_meshsdf_texture(const int32_t* face, const float* bary, int64_t n, const float* uv, const int32_t* face_mat, int64_t n_faces,
                                const int64_t* mat_table, const float* mat_kd, int n_mats, const uint8_t* images, int64_t image_bytes,
                                float* colors, void* stream);
/* The PBR variant (the reference's data/mesh_sampler_pbr.py; s3d_meshpbr.hip): out [n][8] = albedo rgb | metallic | roughness |
 * normal xyz in [0, 1].  face, bary, uv, face_mat as above.  mat_table [n_mats][4][3] (device) = {byte offset into images, W, H} of
 * the albedo, metallic, roughness and normal map of a material — albedo and normal tightly packed 8-bit RGB rows, metallic and
 * roughness single 8-bit planes; W = 0: absent —, mat_factors [n_mats][5] (device) = Kd rgb, metallic, roughness: the table and
 * factors of rendering.pbr.pack_pbr_materials.  The uv is interpolated once per query, by the expression of s3d_meshsdf_texture,
 * and a NaN component of it is replaced by 0.  Per map, with that map's own W and H: texel x = round(u (W - 1)) mod W, y =
 * round((1 - v) (H - 1)) mod H (half to even), value = byte / 255 (correctly rounded), so with the same albedo map columns 0..2
 * equal s3d_meshsdf_texture's colours bit for bit.  Fallbacks: no albedo map: Kd; no metallic / roughness map: the factor; no
 * normal map: (128, 128, 255) / 255, the flat tangent-space normal; a map whose texels would lie outside image_bytes, or a
 * rounded coordinate that is not finite or >= 1e9 in magnitude: as if the map were absent; face -1: eight zeros.  A row is
 * written as two 16-byte stores: `out` not 16-byte aligned is S3D_ERR_INVALID and launches nothing.  n == 0 does nothing. */
S3D_API int s3d_meshsdf_texture_pbr(const int32_t* face, const float* bary, int64_t n, const float* uv, const int32_t* face_mat,
                                    int64_t n_faces, const int64_t* mat_table, const float* mat_factors, int n_mats, const uint8_t* images,
                                    int64_t image_bytes, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Geometry evaluation: the three metrics of the reference's evaluation/patch_utils.py that need nothing but
 * voxel grids: LP-IoU, LP-F-score (eval_LP_IoU :77, eval_LP_Fscore :100) and the pairwise-IoU diversity (pairwise_IoU_dist :30).
 * Volumes are uint8 [H][W][D], non-zero = occupied.  A patch of side ps is ceil(ps^3 / 64) 64-bit words: voxel (i, j, k) is bit
 * t = (i * ps + j) * ps + k, word t / 64, bit t % 64 (least significant first), tail bits zero.  patch_size 2..32; anything else
 * is S3D_ERR_INVALID and launches nothing.  Compaction, the shuffle and the means stay with the caller.
 * ------------------------------------------------------------------------------------------------ */
/* out[i][j][k] = OR over the window [floor(i * in / out), ceil((i + 1) * in / out)) per axis: adaptive_max_pool3d of an occupancy
 * (load_voxgrid :26); min-pooling an SDF and testing <= 0 (load_sdfgrid2vox :14) is this pooling of the <= 0 mask. */
S3D_API int s3d_eval_pool_or(const uint8_t* vox, const int in_dims[3], const int out_dims[3], uint8_t* out, void* stream);
/* counts[k] = (dims[k] + 2 * (patch_size / 2) - patch_size) / stride + 1: the candidate patches per axis of the volume zero-padded
 * by patch_size / 2 (extract_valid_patches_unfold :59-61).  Host only. */
S3D_API int s3d_eval_patch_counts(const int dims[3], int patch_size, int stride, int counts[3]);
/* flags [counts[0] * counts[1] * counts[2]], candidate (a, b, c) at (a * counts[1] + b) * counts[2] + c: 1 when the centre cube
 * (side 2 for even, 3 for odd patch_size, from patch_size / 2 - 1) holds an occupied and a free voxel (:66-71).  The padding is
 * implicit. */
S3D_API int s3d_eval_patch_valid(const uint8_t* vox, const int dims[3], int patch_size, int stride, uint8_t* flags, void* stream);
/* The listed candidates as words and population counts [n].  word_major = 0: words [n][n_words]; 1: words [n_words][n] (what
 * s3d_eval_lp_max reads its reference set from).  A candidate index outside the grid packs as an empty patch. */
S3D_API int s3d_eval_pack_patches(const uint8_t* vox, const int dims[3], int patch_size, int stride, const int64_t* candidates, int64_t n,
                                  int word_major, uint64_t* words, int32_t* counts, void* stream);
/* gen_words [n_gen][n_words] (patch-major), ref_words [n_words][n_ref] (word-major), counts >= 1 (true of every valid patch).
 * max_iou[g] = max over r of float(i) / float(ng + nr - i), max_f[g] = max over r of (2 p q) / ((p + q) + 1e-8f) with
 * p = float(i) / float(ng), q = float(i) / float(nr), i = |g & r|: every operation one correctly rounded float32 operation in this
 * order, as the reference's tensors evaluate it.  n_ref = 0: both 0.  n_gen = 0: nothing is written. */
S3D_API int s3d_eval_lp_max(const uint64_t* gen_words, const int32_t* gen_counts, int64_t n_gen, const uint64_t* ref_words,
                            const int32_t* ref_counts, int64_t n_ref, int n_words, float* max_iou, float* max_f, void* stream);
/* words [n][ceil(voxels / 64)]: bit b of word w of volume v = vols[v][w * 64 + b] != 0 */
S3D_API int s3d_eval_pack_volumes(const uint8_t* vols, int64_t n, int64_t voxels, uint64_t* words, void* stream);
/* inter[i][j] = |v_i & v_j|, uni[i][j] = |v_i | v_j|, both [n][n] */
S3D_API int s3d_eval_pairwise_counts(const uint64_t* words, int64_t n, int64_t n_words, int64_t* inter, int64_t* uni, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SSFID activation statistics: the first two layers of the reference's 3-D voxel classifier
 * (evaluation/classifier3D.py: Conv3d(k4, s2, p1) + InstanceNorm3d (no affine, eps 1e-5, biased variance) + leaky_relu(0.01), 1 -> 32
 * -> 64 channels) and the statistics evaluation/ssfid.py :65-77 takes of them: the rows' mean and their ddof = 1 covariance.
 * The zero padding of the second convolution pads the activated tensor.  Output extents are floor(n / 2) per axis and layer.
 * The Frechet distance itself is host arithmetic on two 64 x 64 matrices and stays with the caller.
 * The handle owns the packed weights and a workspace that grows on demand; calls on one handle must be ordered.  Growing the
 * workspace may synchronise the device.  The same input gives the same bits on every call and handle.
 * ------------------------------------------------------------------------------------------------ */
typedef struct s3d_ssfid s3d_ssfid;
S3D_API int s3d_ssfid_create(s3d_ssfid** out);
S3D_API void s3d_ssfid_destroy(s3d_ssfid* h);
/* name / shape: conv_1.weight [32][1][4][4][4], conv_1.bias [32], conv_2.weight [64][32][4][4][4], conv_2.bias [64], host float32.
 * One of these names with another shape is S3D_ERR_UNSUPPORTED (the reference's classifier() is always ef_dim = 32); another name
 * is S3D_ERR_INVALID. */
S3D_API int s3d_ssfid_set_param(s3d_ssfid* h, const char* name, const float* data, const int64_t* shape, int ndim);
/* out_dims[k] = dims[k] >> out_layer, channels = 32 (layer 1) or 64 (layer 2).  Host only; the checks of s3d_ssfid_features. */
S3D_API int s3d_ssfid_out_dims(const int dims[3], int out_layer, int out_dims[3], int* channels);
/* vox: device uint8 [X][Y][Z], non-zero = occupied.  out_layer 1 or 2 (3 and 4: S3D_ERR_UNSUPPORTED).  act: null, or device
 * float32 [X' Y' Z'][C], rows in [X'][Y'][Z'] order (act.permute(0, 2, 3, 4, 1).view(-1, C)).  mu [C], sigma [C][C]: device
 * float64.  An axis whose output extent would be 0, or a parameter not yet set, is S3D_ERR_INVALID and launches nothing.  One
 * row gives the NaN covariance np.cov gives. */
S3D_API int s3d_ssfid_features(s3d_ssfid* h, const uint8_t* vox, const int dims[3], int out_layer, float* act, double* mu, double* sigma,
                               void* stream);
/* Stage timing for tools/bench_ssfid.py.  on != 0: every following s3d_ssfid_features records device events between its stages.
 * s3d_ssfid_profile_read waits for the last timed call and gives its milliseconds: layer 1, its statistics, layer 2, its
 * statistics, the covariance (normalise + Gram + reduction); layer 2's two are 0 for out_layer 1. */
S3D_API int s3d_ssfid_profile(s3d_ssfid* h, int on);
S3D_API int s3d_ssfid_profile_read(s3d_ssfid* h, double ms[5]);

/* ------------------------------------------------------------------------------------------------
 * Image features of the multi-view renders: what the reference's evaluation/sifid.py and evaluation/lpips.py
 * take of a PNG.  S3D_IMGFEAT_INCEPTION is the stem of torchvision's inception_v3 (BasicConv2d = Conv2d(bias = False) +
 * BatchNorm2d(eps = 1e-3, eval) + ReLU): Conv2d_1a_3x3, Conv2d_2a_3x3, Conv2d_2b_3x3 for dims 64, then MaxPool2d(3, 2),
 * Conv2d_3b_1x1, Conv2d_4a_3x3 for dims 192, on 2 (u8 / 255) - 1.  S3D_IMGFEAT_ALEXNET is torchvision's alexnet `features` up to
 * its fifth ReLU on ((u8 / 255. - 0.5) / 0.5 - mu) / sigma, with the five linear LPIPS layers.
 * The handle owns the packed weights, the activations of the last s3d_imgfeat_features call and a workspace that grows on demand;
 * calls on one handle must be ordered.  Growing the workspace may synchronise the device.  Every call only enqueues on `stream`.
 * The same input gives the same bits on every call and handle.
 * ------------------------------------------------------------------------------------------------ */
#define S3D_IMGFEAT_INCEPTION 0
#define S3D_IMGFEAT_ALEXNET 1
typedef struct s3d_imgfeat s3d_imgfeat;
S3D_API int s3d_imgfeat_create(int net, s3d_imgfeat** out);
S3D_API void s3d_imgfeat_destroy(s3d_imgfeat* h);
/* Host float32 by the torchvision state-dict names.  Inception: <unit>.conv.weight [Cout][Cin][k][k] and <unit>.bn.{weight, bias,
 * running_mean, running_var} [Cout] for the five units above.  AlexNet: features.{0,3,6,8,10}.{weight, bias} and
 * lpips_weights.{0..4}.main.1.weight [1][C][1][1].  One of these names with another shape is S3D_ERR_UNSUPPORTED; another name is
 * S3D_ERR_INVALID. */
S3D_API int s3d_imgfeat_set_param(s3d_imgfeat* h, const char* name, const float* data, const int64_t* shape, int ndim);
/* Host only; the checks of s3d_imgfeat_features.  dims: 64 or 192 for the Inception stem (anything else: S3D_ERR_UNSUPPORTED),
 * ignored for AlexNet.  nlayers = 3, 5 or 5; hw[l] = {rows, columns} and channels[l] of unit l's output (either may be null).  An
 * image too small for the network is S3D_ERR_INVALID; for AlexNet that includes an empty final MaxPool2d(3, 2), where the
 * reference raises although the pool's output is unused. */
S3D_API int s3d_imgfeat_out_dims(int net, int H, int W, int dims, int* nlayers, int hw[5][2], int channels[5]);
/* img: device uint8 [n][H][W][ch], ch = 3 or 4 (the fourth is not read).  acts: null, or a host array of nlayers device pointers,
 * each null or float32 [n][rows][columns][C] (channels last, after the ReLU). */
S3D_API int s3d_imgfeat_features(s3d_imgfeat* h, const uint8_t* img, int n, int H, int W, int ch, int dims, float* const* acts, void* stream);
/* Inception: of the last unit of the last s3d_imgfeat_features call, per image, the rows' mean mu [n][C] and ddof = 1 covariance
 * sigma [n][C][C], device float64; rows are pixels in row-major order.  One row gives the NaN covariance np.cov gives. */
S3D_API int s3d_imgfeat_stats(s3d_imgfeat* h, double* mu, double* sigma, void* stream);
/* AlexNet: of the n images of the last s3d_imgfeat_features call, total [n][n] = sum over the five maps of
 * mean_pixels sum_c w_c (xh_i - xh_j)^2, xh = x rsqrt(sum_c x^2 + 1e-10), and layers (null or [5][n][n]) the five terms; device
 * float64.  The diagonal is exactly 0 and the matrix exactly symmetric. */
S3D_API int s3d_imgfeat_pairs(s3d_imgfeat* h, double* layers, double* total, void* stream);
/* Stage timing for tools/bench_imgmetrics.py, as s3d_ssfid_profile: milliseconds of the last timed s3d_imgfeat_features, units
 * 1..5 (a max-pool counts with the unit it feeds; 0 for units not run) and the unit normalisation (AlexNet). */
S3D_API int s3d_imgfeat_profile(s3d_imgfeat* h, int on);
S3D_API int s3d_imgfeat_profile_read(s3d_imgfeat* h, double ms[6]);

/* ------------------------------------------------------------------------------------------------
 * Multi-view renders of triangle meshes: a tiled rasteriser, so that the views the reference's
 * evaluation/eval_full.py compares (rendering/blender_render_multiview.py makes them with Blender) can be made of an exported
 * mesh and of the input mesh.  Parity with Blender is not claimed: flat shading, one light, no shadows.
 * The sample grid is ws x hs = the image size times the supersampling factor; sample (i, j) has its centre at (i + 0.5, j + 0.5)
 * and index j * ws + i, row 0 on top.  Coordinates are snapped to 1 / S3D_RENDER_SUBPIXEL of a sample, and coverage is decided on
 * them in integer arithmetic: with the corners ordered so that the doubled area is positive, a sample lies in a triangle when
 * every edge value E = (xb - xa)(py - ya) - (yb - ya)(px - xa) is positive, or zero on an edge with yb > ya, or yb == ya and
 * xb < xa (the top-left rule), so two triangles that share an edge cover each sample once.  Both orientations are drawn.
 * A triangle is dropped when a corner is flagged (w <= near), a snapped coordinate lies beyond +-S3D_RENDER_MAX_COORD, a vertex
 * index lies outside the table, or its doubled area is zero; there is no near-plane clipping.
 * Scan, sort and segment starts between the calls are the caller's (sin3dm_amd/rendering/rasterizer.py).  Matrices and the light
 * are host arrays; all other arrays are device pointers; every call only enqueues on `stream`.  The same input gives the same bits.
 * ------------------------------------------------------------------------------------------------ */
#define S3D_RENDER_TILE 16
#define S3D_RENDER_SUBPIXEL 256
#define S3D_RENDER_MAX_COORD (1 << 20)
#define S3D_RENDER_MAX_GRID 4096
/* cap of the (tile, triangle) pair list: 2^27 pairs = 1 GiB of workspace (two int32 per pair) */
#define S3D_RENDER_MAX_PAIRS (1LL << 27)
/* shade = S3D_RENDER_AMBIENT + S3D_RENDER_DIFFUSE * max(0, n . light) */
#define S3D_RENDER_AMBIENT 0.35f
#define S3D_RENDER_DIFFUSE 0.65f
/* view_proj: row-major 4 x 4, clip = M (x, y, z, 1); only the x, y and w rows are read.  xy_fixed [n_verts][2] = round(256 * ((x / w
 * / 2 + 1 / 2) ws, (1 / 2 - y / w / 2) hs)) clamped to +-2^30, inv_w [n_verts] = 1 / w; a vertex with w <= near (or not finite) is
 * flagged: inv_w = 0 and xy_fixed = 0. */
S3D_API int s3d_render_project(const float* verts, int64_t n_verts, const float view_proj[16], int ws, int hs, float near, int32_t* xy_fixed,
                               float* inv_w, void* stream);
/* faces [n_faces][3] int32.  counts[f] = tiles of S3D_RENDER_TILE^2 samples that hold a sample centre inside the box of the snapped
 * corners (clamped to the grid), 0 for a dropped triangle; status[f] = 0 drawn, 1 a flagged corner, 2 a coordinate or an index out
 * of range, 3 zero area. */
S3D_API int s3d_render_bin_count(const int32_t* xy_fixed, const float* inv_w, int64_t n_verts, const int32_t* faces, int64_t n_faces, int ws,
                                 int hs, int64_t* counts, uint8_t* status, void* stream);
/* offsets [n_faces] = exclusive scan of counts, n_pairs = their sum (more than S3D_RENDER_MAX_PAIRS: S3D_ERR_UNSUPPORTED).  Triangle
 * f writes (pair_tile, pair_tri) = (ty * ceil(ws / 16) + tx, f) at offsets[f]... in ascending tile order. */
S3D_API int s3d_render_bin_fill(const int32_t* xy_fixed, const float* inv_w, int64_t n_verts, const int32_t* faces, int64_t n_faces, int ws,
                                int hs, const int64_t* offsets, int64_t n_pairs, int32_t* pair_tile, int32_t* pair_tri, void* stream);
/* seg [tiles + 1]: the pairs sorted by tile (a stable sort keeps each tile's triangles ascending), tile t owns seg_tri[seg[t] ..
 * seg[t+1]).  Per sample: count = covering triangles (clamped at 255), depth = the largest 1 / w among them, interpolated with the
 * edge values as weights, face_id = its triangle (equal 1 / w: the lower index); nothing covers: face_id -1, depth 0. */
S3D_API int s3d_render_raster(const int32_t* xy_fixed, const float* inv_w, int64_t n_verts, const int32_t* faces, int64_t n_faces, int ws,
                              int hs, const int64_t* seg, const int32_t* seg_tri, int64_t n_pairs, int32_t* face_id, float* depth,
                              uint8_t* count, void* stream);
/* rgba [hs / supersample][ws / supersample][4]: per covered sample the base colour at the perspective-correct barycentrics times
 * the shade of the flat normal turned towards the camera (light: unit vector towards the light, in the space of verts), clamped to
 * [0, 1]; RGB = the mean over a pixel's covered samples in row order, A = the covered share, both as uint8(255 x + 0.5).
 * Base colour: vertex_colors [n_verts][3] when given; else the material m = face_mat[f] (null: 0) of mat_table / mat_kd / images as
 * for s3d_meshsdf_texture — its image at uv [n_faces][3][2], bilinear with the GL convention (texel (i, j) centred at u = (i + 0.5) / W,
 * v = 1 - (j + 0.5) / H, row 0 of the image on top, clamp to edge), or its Kd without image or uv; n_mats = 0: white. */
S3D_API int s3d_render_shade(const float* verts, const int32_t* xy_fixed, const float* inv_w, int64_t n_verts, const int32_t* faces,
                             int64_t n_faces, const int32_t* face_id, int ws, int hs, int supersample, const float view_proj[16],
                             const float light[3], const float* vertex_colors, const float* uv, const int32_t* face_mat,
                             const int64_t* mat_table, const float* mat_kd, int n_mats, const uint8_t* images, int64_t image_bytes,
                             uint8_t* rgba, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PBR renders: smooth normals, normal maps, a GGX light model and the material passes of the reference's
 * rendering/blender_render_pbr.py, on the raster stage above.  Parity with Blender is not claimed: directional lights, shadows opt-in
 * (s3d_pbr_shade_lit below), no ambient occlusion, no tone curve, texel values taken as they are (no sRGB decoding).
 * ------------------------------------------------------------------------------------------------ */
#define S3D_RENDER_MAX_LIGHTS 4
/* materials of one s3d_pbr_shade call: the PBR table is a host array and travels with the launch */
#define S3D_RENDER_PBR_MAX_MATERIALS 16
#define S3D_RENDER_MIN_ROUGHNESS 0.089f
/* albedo of the geo pass: 134 / 255 (blender_render_pbr.py:207) */
#define S3D_RENDER_GEO_GREY (134.0f / 255.0f)
/* overall scale of rendering/pbr.py's three_light_rig (key : fill : rim = 1 : 0.5 : 0.1): a white Lambert surface (metallic 0,
 * roughness 1) that faces all three lights squarely stays below 1 with the default ambient */
#define S3D_RENDER_RIG_INTENSITY 0.5f
#define S3D_RENDER_PBR_AMBIENT 0.1f
#define S3D_RENDER_PASS_SHADED 0
#define S3D_RENDER_PASS_ALBEDO 1
#define S3D_RENDER_PASS_METALLIC 2
#define S3D_RENDER_PASS_ROUGHNESS 3
#define S3D_RENDER_PASS_NORMAL 4
#define S3D_RENDER_PASS_GEO 5
/* normals [n_verts][3]: the normalised sum of the unnormalised normals cross(b - a, c - a) of the faces at a vertex (area weights),
 * summed in ascending corner order in float64.  corner_order [3 n_faces]: the corners (corner k = vertex k % 3 of face k / 3) sorted
 * by vertex index, stably; vertex_start [n_verts + 1]: vertex v owns corner_order[vertex_start[v] .. vertex_start[v + 1]).  A vertex
 * without faces, or whose sum has squared length 0 or is not finite: (0, 0, 0), "use the flat normal". */
S3D_API int s3d_pbr_vertex_normals(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int64_t* corner_order,
                                      const int64_t* vertex_start, float* normals, void* stream);
/* tangents [n_faces][2][3] = (T, B) of the uv map uv [n_faces][3][2] (v in the GL convention of the lookups): with e1 = b - a,
 * e2 = c - a, (du1, dv1), (du2, dv2) and det = du1 dv2 - du2 dv1: T = (e1 dv2 - e2 dv1) / det, B = (e2 du1 - e1 du2) / det, in
 * float64.  det == 0 or a result that is not finite: T = B = 0, and the normal map is ignored on that face. */
S3D_API int s3d_pbr_face_tangents(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* uv,
                                     float* tangents, void* stream);
/* s3d_render_shade with another light model; rgba, the resolve and every argument up to image_bytes as there, without its light.
 * normals [n_verts][3] (s3d_pbr_vertex_normals; null: flat): the shading normal is the barycentric mix of the corners' normals,
 * normalised and turned like the flat normal; the flat normal where a corner's normal is zero or the mix points away from it.
 * tangents [n_faces][2][3] (needs uv; null: no normal maps).
 * pbr_table HOST int64 [n_mats][4][3] = {byte offset into images, W, H} of the albedo (3 channels), metallic (1), roughness (1)
 * and normal (3) maps of a material, W = 0: absent — then the factor of pbr_factors HOST float [n_mats][5] = {Kd r, g, b,
 * metallic, roughness} (the normal map has none).  n_mats <= S3D_RENDER_PBR_MAX_MATERIALS; mat_table / mat_kd are not read.
 * pbr_table null: the base colour of s3d_render_shade (vertex colours, mat_table / mat_kd, white), metallic 0, roughness 0.5.
 * Normal map: t = 2 texel / 255 - 1, T' = normalize(T - N (N . T)), B' = cross(N, T') sign(cross(N, T') . B),
 * N <- normalize(t.x T' + t.y B' + t.z N).
 * eye [3]: the camera position in the space of verts; lights [n_lights][4]: unit direction towards the light and intensity.
 * With V to the eye, H = normalize(L + V), alpha = r^2 (r clamped to [S3D_RENDER_MIN_ROUGHNESS, 1]), k = alpha / 2,
 * F0 = 0.04 (1 - m) + albedo m, F = F0 + (1 - F0)(1 - V.H)^5, D = alpha^2 / (pi ((N.H)^2 (alpha^2 - 1) + 1)^2),
 * G = NL / (NL (1 - k) + k) NV / (NV (1 - k) + k), NL = max(N.L, 0), NV = max(N.V, 1e-4):
 * out = ambient albedo + sum_k I_k NL ((1 - F)(1 - m) albedo + pi D G F / (4 NL NV + 1e-6)), clamped to [0, 1].
 * pass: S3D_RENDER_PASS_SHADED; _ALBEDO / _METALLIC / _ROUGHNESS: the unlit value (the scalars as grey; roughness before the clamp);
 * _NORMAL: 0.5 N + 0.5; _GEO: shaded with albedo S3D_RENDER_GEO_GREY, metallic 0, roughness 0.5 and no normal map.
 * S3D_ERR_INVALID (nothing is launched): more than S3D_RENDER_MAX_LIGHTS lights, an unknown pass, a table entry that runs past
 * image_bytes, tangents without uv, a value that is not finite.  More materials than the cap: S3D_ERR_UNSUPPORTED. */
S3D_API int s3d_pbr_shade(const float* verts, const int32_t* xy_fixed, const float* inv_w, int64_t n_verts, const int32_t* faces,
                                 int64_t n_faces, const int32_t* face_id, int ws, int hs, int supersample, const float view_proj[16],
                                 const float* vertex_colors, const float* uv, const int32_t* face_mat, const int64_t* mat_table,
                                 const float* mat_kd, int n_mats, const uint8_t* images, int64_t image_bytes, const float* normals,
                                 const float* tangents, const int64_t* pbr_table, const float* pbr_factors, const float eye[3],
                                 const float* lights, int n_lights, float ambient, int pass, uint8_t* rgba, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ray queries against a mesh and the shadows of the PBR renders (additions: no earlier entry point changed).
 * The mesh and the grid are those of s3d_meshsdf_closest: tri9 [n_faces][9], origin [3] / cell / dims [3] (host), seg [cells + 1]
 * and seg_tri [n_pairs] from s3d_meshsdf_bin_count / _bin_fill, whose `band` is here the slack that makes the lists conservative
 * against the rounding of the walk (at least 2^-19 of the largest coordinate magnitude).  The grid box must hold
 * the mesh: what lies outside it is not found.
 *
 * The ray-triangle test, fp32, no product fused into a sum, with a, b, c the triangle's corners, o the origin, d the direction:
 *   e1 = b - a, e2 = c - a, p = d x e2, s = o - a, q = s x e1     (x x y = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0))
 *   det = e1 . p, u = s . p, v = d . q, w = e2 . q                (x . y = (x0 y0 + x1 y1) + x2 y2)
 *   det < 0: det, u, v, w change sign
 *   hit = det > 0 and u >= 0 and v >= 0 and u + v <= det and t_min <= w / det <= t_max
 * Edges are inclusive; det == 0 or a value that is not finite is a miss.  The test is never clipped to a cell, and any hit ends
 * the walk: `hit` does not depend on the grid, on the order of a cell's list or on a triangle standing in several cells.
 * Not watertight: a ray through an edge two triangles share may miss both.  d need not have unit length: t counts in |d|.
 * The walk: a 3-D DDA from the entry into the grid box (or t_min) to the exit (or t_max), every crossing computed from the border's
 * index as (origin + i * cell - o) / d, a zero component never stepped, at most dims[0] + dims[1] + dims[2] + 1 cells.
 * ------------------------------------------------------------------------------------------------ */
/* origins, dirs [n_rays][3]; skip_face [n_rays] int32 (-1: none) or null; t_max may be +inf.  hit [n_rays] uint8: 1 when some
 * triangle other than skip_face is crossed at a parameter in [t_min, t_max].  status [n_rays] uint8: 0 walked; 1 the ray does not
 * meet the grid box within [t_min, t_max]; 2 an origin or direction that is not finite, or a zero direction (hit = 0 for 1 and 2).
 * S3D_ERR_INVALID (nothing is launched): dims below 1, t_min negative or not finite, t_max < t_min or NaN, a null output. */
S3D_API int s3d_mesh_ray_occluded(const float* origins, const float* dirs, const int32_t* skip_face, int64_t n_rays, float t_min, float t_max,
                                  const float* tri9, int64_t n_faces, const float origin[3], float cell, const int dims[3], const int64_t* seg,
                                  const int32_t* seg_tri, int64_t n_pairs, uint8_t* hit, uint8_t* status, void* stream);
/* lit [hs][ws] uint8 from the raster buffers of a view (face_id, xy_fixed, inv_w as s3d_pbr_shade reads them; tri9 = verts[faces]):
 * bit k is set when light k (lights HOST [n_lights][4], direction towards the light and intensity) reaches the sample; an
 * uncovered sample gets 0.  Point = b0 P0 + b1 P1 + b2 P2 with the sample's barycentrics, as s3d_pbr_shade's view vector; N = the
 * face's own normal cross(b - a, c - a) turned to the camera by the integer rule of the shaders.  N . L <= 0: bit 0, no ray.
 * Otherwise one ray from the point along L with skip_face = the sample's face, [t_min, +inf): bit 1 when it is not occluded
 * (status 1 or 2 included).  The terminator follows the faces, under smooth normals too.
 * S3D_ERR_INVALID: more than S3D_RENDER_MAX_LIGHTS lights, dims below 1, t_min negative or not finite, a null output. */
S3D_API int s3d_pbr_shadow_mask(const float* verts, const int32_t* xy_fixed, const float* inv_w, int64_t n_verts, const int32_t* faces,
                                   int64_t n_faces, const int32_t* face_id, int ws, int hs, const float view_proj[16], const float* lights,
                                   int n_lights, float t_min, const float* tri9, const float origin[3], float cell, const int dims[3],
                                   const int64_t* seg, const int32_t* seg_tri, int64_t n_pairs, uint8_t* lit, void* stream);
/* s3d_pbr_shade with lit [hs][ws] (s3d_pbr_shadow_mask): light k is skipped at a sample whose bit k is clear, the others are
 * added in their order.  The albedo, metallic, roughness and normal passes do not read the mask; the geo pass does.  lit null:
 * s3d_pbr_shade, its bits. */
S3D_API int s3d_pbr_shade_lit(const float* verts, const int32_t* xy_fixed, const float* inv_w, int64_t n_verts, const int32_t* faces,
                              int64_t n_faces, const int32_t* face_id, int ws, int hs, int supersample, const float view_proj[16],
                              const float* vertex_colors, const float* uv, const int32_t* face_mat, const int64_t* mat_table,
                              const float* mat_kd, int n_mats, const uint8_t* images, int64_t image_bytes, const float* normals,
                              const float* tangents, const int64_t* pbr_table, const float* pbr_factors, const float eye[3],
                              const float* lights, int n_lights, float ambient, int pass, const uint8_t* lit, uint8_t* rgba, void* stream);

/* ------------------------------------------------------------------------------------------------
 * torch's CPU noise stream on the device: the float32 values `torch.randn` / `torch.rand` draw from
 * torch's default CPU generator (MT19937), so that a sampling run consumes the stream the reference consumes on the CPU
 * (src/diffusion/gaussian_diffusion.py:514, 431, 591) without a host draw and an upload per step.
 * The handle owns the 624 state words on the device, the position inside them on the host (it is plain arithmetic on the
 * sizes drawn) and the raw-word workspace.  pos: index of the next word, 0..624 (624: the next draw regenerates first —
 * where `torch.manual_seed` leaves the generator).  One randn call of n >= 16 elements consumes n + 16 * (n % 16 != 0)
 * words (the last 16 outputs are redrawn from 16 more words when n is not a multiple of 16); rand consumes n.
 * All calls on one handle must be ordered (one stream, or event edges between streams): they read and write its state.
 * ------------------------------------------------------------------------------------------------ */
typedef struct s3d_rng s3d_rng;
S3D_API int s3d_rng_create(s3d_rng** out);
S3D_API void s3d_rng_destroy(s3d_rng* r);
S3D_API int s3d_rng_set_state(s3d_rng* r, const uint32_t key[624], int pos, void* stream);
/* synchronises `stream` */
S3D_API int s3d_rng_get_state(s3d_rng* r, uint32_t key[624], int* pos, void* stream);
/* grow the raw-word workspace to `words` 32-bit words (never shrinks; may synchronise the device).  s3d_rng_randn / s3d_rng_rand
 * allocate nothing: a call that needs more words than reserved is S3D_ERR_INVALID. */
S3D_API int s3d_rng_reserve(s3d_rng* r, int64_t words);
/* out [n_calls][numel_per_call]: n_calls consecutive torch.randn(numel_per_call) calls.  numel_per_call < 16 is
 * S3D_ERR_UNSUPPORTED (torch takes a double-precision path there). */
S3D_API int s3d_rng_randn(s3d_rng* r, float* out, int64_t numel_per_call, int n_calls, void* stream);
/* out [numel]: one torch.rand(numel) call */
S3D_API int s3d_rng_rand(s3d_rng* r, float* out, int64_t numel, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIN3DM_HIP_H */
