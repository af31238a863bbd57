/*
 * bd_hip.h -- C ABI of libbd_hip.so, the MI355X (gfx950) kernels behind the BadDiffusion hot path.
 *
 * The reference (IBM/BadDiffusion) has no FFI for this path: the seam is the Python API that
 * baddiffusion.py calls.  Each entry point below names the reference code it replaces
 * (paths relative to the reference root).  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch's allocator on the Python side);
 *     the library never allocates, frees or retains device memory;
 *   - activations are NHWC ("pixels x channels", fp32) with an explicit leading dimension `ld`
 *     (elements between consecutive pixels), so a channel slice of a wider buffer is a valid tensor
 *     and the reference's torch.cat on the channel axis needs no copy;
 *   - conv weights are [Cout][kh][kw][Cin] (the physical layout of a channels_last OIHW tensor);
 *   - all work is enqueued on `stream` (a hipStream_t); no hidden synchronisation, no default-stream
 *     use => capturable in a hipGraph;
 *   - return 0 on success, a negative bd_status otherwise; bd_last_error() gives the message
 *     (thread-local).  No C++ exception crosses this boundary.
 */
#ifndef BD_HIP_H
#define BD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* bd_stream_t; /* hipStream_t */

enum bd_status {
    BD_OK = 0,
    BD_ERR_INVALID = -1,     /* bad shape / null pointer / misaligned */
    BD_ERR_UNSUPPORTED = -2, /* configuration the reference supports but this path does not */
    BD_ERR_LAUNCH = -3,      /* hipGetLastError() after a launch */
    BD_ERR_WORKSPACE = -4    /* workspace too small */
};

const char* bd_last_error(void);
int bd_version(void);

/* ------------------------------------------------------------------------------------------------
 * a-1 + a-2: poisoned-sample blend + BadDiffusion forward process, one fused kernel.
 * Replaces dataset.py:275-276 (get_mask), :288-315 (clean/backdoor transforms: R = m*x + (1-m)*g,
 * x0 = y | R = 0, x0 = x), util.py:83-111 (normalize, eps 1e-5) when the images are uint8, and
 * loss.py:257-285 (q_sample_diffuser) + schedulers/scheduling_ddpm.py:422-443 (add_noise):
 *     x_noisy = sqrt(ac_t) x0 + sqrt(1-ac_t) eps + (1 - sqrt(ac_t)) R,  target = rho_t R + eps.
 * Layout: NCHW in (what the reference's DataLoader yields), NHWC out with leading dim ld_out.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int B, C, H, W;
    const float* images_f32;      /* [B,C,H,W] normalised images, or NULL                     */
    const uint8_t* images_u8;     /* [B,H,W,C] raw uint8 (normalised in-kernel), or NULL      */
    const uint8_t* is_poison;     /* [B] 0 = clean row, 1 = backdoor row                      */
    const float* trigger;         /* [C,H,W]  g                                               */
    const float* target_img;      /* [C,H,W]  y                                               */
    const float* noise;           /* [B,C,H,W] eps (NCHW, as torch.randn produced it)         */
    const int64_t* timesteps;     /* [B]                                                      */
    const float* alphas;          /* [T]                                                      */
    const float* alphas_cumprod;  /* [T]                                                      */
    float vmin;                   /* mask threshold: m = (g > vmin) ? 0 : 1                   */
    float* x_noisy; int64_t ld_noisy;   /* NHWC [B*H*W, ld]                                   */
    float* target;  int64_t ld_target;  /* NHWC [B*H*W, ld]                                   */
    float* R_out;                 /* optional NCHW [B,C,H,W] (pixel_values), may be NULL      */
    float* x0_out;                /* optional NCHW [B,C,H,W] (target), may be NULL            */
    int64_t* mask_out;            /* optional [C,H,W] int64 mask (bit-exact check), may be NULL */
    float* image_out;             /* optional NCHW [B,C,H,W] normalised image x, may be NULL  */
    const int64_t* row_index;     /* optional [B]: batch row b reads image row_index[b] of the (larger, HBM-resident)
                                     image array -- the DataLoader's shuffled gather, fused; NULL = row b          */
    const uint8_t* flip;          /* optional [B]: 1 = mirror the image along W (RandomHorizontalFlip, dataset.py:127) */
} bd_poison_qsample_desc;
int bd_poison_qsample(const bd_poison_qsample_desc* d, bd_stream_t stream);

/* Plain q_sample_diffuser on already-collated (x0, R) NCHW batches (loss.py:257-285). */
typedef struct {
    int B, C, H, W;
    const float* x0; const float* R; const float* noise;   /* NCHW */
    const int64_t* timesteps; const float* alphas; const float* alphas_cumprod;
    float* x_noisy; int64_t ld_noisy;   /* NHWC */
    float* target;  int64_t ld_target;  /* NHWC */
} bd_qsample_desc;
int bd_qsample(const bd_qsample_desc* d, bd_stream_t stream);

/* The same two kernels with the target's coefficient read from a table: target = corr[t] R + eps, x_noisy as above (its shift
 * (1 - sqrt(ac_t)) R belongs to the forward chain and does not depend on the sampler).  rho_t above is the coefficient for which the
 * DDPM ancestral step maps the shifted chain onto itself; a deterministic sampler needs another one (DESIGN.md section 3,
 * "Sampler-matched correction terms"; baddiffusion_amd/correction.py builds the tables).  The descriptors are the ones above, field for
 * field, plus
 *     corr   fp32 [T], device, indexed by timesteps[b] like alphas_cumprod.
 * `alphas` is not read and may be NULL.  The kernel bodies are shared with bd_poison_qsample / bd_qsample: every output but `target` is
 * theirs bit for bit, and with corr[t] = their rho_t so is `target`; a clean row's target is eps itself.  Status: as above, and
 * BD_ERR_INVALID for a null corr (checked on the host, before any launch). */
typedef struct {
    int B, C, H, W;
    const float* images_f32;
    const uint8_t* images_u8;
    const uint8_t* is_poison;
    const float* trigger;
    const float* target_img;
    const float* noise;
    const int64_t* timesteps;
    const float* alphas;          /* not read, may be NULL */
    const float* alphas_cumprod;
    float vmin;
    float* x_noisy; int64_t ld_noisy;
    float* target;  int64_t ld_target;
    float* R_out;
    float* x0_out;
    int64_t* mask_out;
    float* image_out;
    const int64_t* row_index;
    const uint8_t* flip;
    const float* corr;            /* [T] coefficient of R in the target */
} bd_poison_qsample_corr_desc;
int bd_poison_qsample_corr(const bd_poison_qsample_corr_desc* d, bd_stream_t stream);

typedef struct {
    int B, C, H, W;
    const float* x0; const float* R; const float* noise;   /* NCHW */
    const int64_t* timesteps; const float* alphas; const float* alphas_cumprod;   /* alphas: not read, may be NULL */
    float* x_noisy; int64_t ld_noisy;   /* NHWC */
    float* target;  int64_t ld_target;  /* NHWC */
    const float* corr;                  /* [T] coefficient of R in the target */
} bd_qsample_corr_desc;
int bd_qsample_corr(const bd_qsample_corr_desc* d, bd_stream_t stream);

/* NCHW <-> NHWC(ld) conversion for the 3-channel boundary tensors. */
int bd_nchw_to_nhwc(const float* src, float* dst, int B, int C, int H, int W, int64_t ld, bd_stream_t stream);
int bd_nhwc_to_nchw(const float* src, int64_t ld, float* dst, int B, int C, int H, int W, bd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * a-5 / a-6 / a-7: scheduler steps and image conversion (all NCHW-agnostic: elementwise over
 * [B, n] with per-launch scalar coefficients read from a DEVICE table indexed by t).
 * Replaces scheduling_ddpm.py:324-420, scheduling_ddim.py:261-381, pipeline_ddpm.py:115-116.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int64_t n;                    /* total elements                                            */
    const float* model_output; const float* sample; const float* noise;  /* noise may be NULL iff t == 0 */
    float* prev_sample; float* pred_original; /* pred_original may be NULL                     */
    const float* alphas_cumprod;  /* [T] device                                                */
    int t, prev_t;                /* prev_t < 0 => alpha_prod_prev = 1                         */
    int variance_type;            /* 0 fixed_small, 1 fixed_large                              */
    int clip_sample; float clip_sample_range;
    int clip_defense; float clip_defense_range;
    /* dynamic thresholding (scheduling_ddpm.py:290-322): NULL = off, and the step is bit for bit what it was.  Set: [n / image_elems]
     * raw quantiles of |x0| per image (bd_abs_quantile); element i belongs to image i / image_elems, s = clamp(q, 1, sample_max_value)
     * (a NaN quantile stays NaN), x0 = clamp(x0, -s, s) / s, clip_sample is ignored (the reference's if / elif), pred_original is the
     * thresholded value and clip_defense still applies to prev_sample.  Needs n % image_elems == 0 and n < 2^31. */
    const float* x0_quantile; int64_t image_elems; float sample_max_value;
} bd_ddpm_step_desc;
int bd_ddpm_step(const bd_ddpm_step_desc* d, bd_stream_t stream);

typedef struct {
    int64_t n;
    const float* model_output; const float* sample; const float* noise; /* noise NULL iff eta == 0 */
    float* prev_sample; float* pred_original;
    const float* alphas_cumprod;
    int t, prev_t; float final_alpha_cumprod; float eta;
    int clip_sample; float clip_sample_range;
    const float* x0_quantile; int64_t image_elems; float sample_max_value;   /* as in bd_ddpm_step_desc (scheduling_ddim.py:203-235) */
} bd_ddim_step_desc;
int bd_ddim_step(const bd_ddim_step_desc* d, bd_stream_t stream);

/* Dynamic thresholding's order statistic: out[b] = torch.quantile(|v_b|, q, interpolation="linear") in fp32, bit for bit, over B images
 * of m values each, image-major and dense (any order inside an image).  v is `x` as it is (model_output NULL), or the predicted
 * x0 = (x - sqrt(1 - a_t) * model_output) / sqrt(a_t), a_t = alphas_cumprod[t], formed on the fly by the device helper the DDPM and
 * DDIM step kernels call, so the value ranked is bitwise the value the step then clamps.
 *   rank = q * (float)(m - 1) in fp32; lo = floor(rank), w = rank - lo; a, b = the order statistics at lo and ceil(rank);
 *   d = b - a; out = w < 0.5 ? fmaf(w, d, a) : fmaf(-d, 1 - w, b).
 * Exact and deterministic: a radix select over the 31 value bits of |v| in three passes (11 / 10 / 10 bits) of integer LDS histograms;
 * one workgroup per image.  A NaN anywhere in an image gives NaN; two infinities around the rank give NaN through d; -0 ranks as 0;
 * denormals are ordinary values.  The result is NOT yet clamped to [1, sample_max_value].  No alignment is asked of x, model_output
 * or m.  Rejected (status < 0, bd_last_error, nothing written): null x / out, B <= 0, m <= 0, B * m >= 2^31, q outside [0, 1] or NaN,
 * model_output without a table or t outside [0, n_alphas), workspace_bytes < bd_abs_quantile_workspace_bytes(B, m) (0 for both paths
 * of today: workspace may then be NULL). */
typedef struct {
    int B; int64_t m;
    const float* x;                 /* [B, m] values, or the sample when model_output is set                        */
    const float* model_output;      /* [B, m] or NULL                                                               */
    const float* alphas_cumprod; int n_alphas; int t;   /* read only with model_output                              */
    float q;
    float* out;                     /* [B]                                                                          */
    void* workspace; size_t workspace_bytes;
} bd_abs_quantile_desc;
size_t bd_abs_quantile_workspace_bytes(int B, int64_t m);
int bd_abs_quantile(const bd_abs_quantile_desc* d, bd_stream_t stream);
/* Which path a (B, m) takes: host code only, the plan the launcher itself reads (same checks of B and m, same messages). */
enum bd_abs_quantile_path {
    BD_AQ_REGISTERS = 0,            /* m <= 4096: 256 threads hold the image in registers, the data is read once    */
    BD_AQ_STREAM = 1                /* larger m: 1024 threads read the image again in every pass                    */
};
typedef struct {
    int path;                       /* enum bd_abs_quantile_path                                                    */
    int workgroups;                 /* = B: one per image                                                           */
    int threads;                    /* per workgroup                                                                */
    int values_per_thread;          /* register slots per thread (BD_AQ_REGISTERS), ceil(m / threads) loads per pass (BD_AQ_STREAM) */
    int passes;                     /* radix passes: 3                                                              */
    int64_t switch_m;               /* the largest m of BD_AQ_REGISTERS                                             */
    size_t workspace_bytes;
} bd_abs_quantile_plan_info;
int bd_abs_quantile_plan(int B, int64_t m, bd_abs_quantile_plan_info* out);

/* f-4: out = clamp?(sum_j coeffs[j] * terms[j]) over k <= BD_LINCOMB_MAX dense fp32 tensors of n elements (one common
 * layout; `terms` / `coeffs` are HOST arrays read at call time).  All PRK / PLMS updates of PNDMScheduler
 * (scheduling_pndm.py:236-397: running sample, stored model outputs, Runge-Kutta accumulator; formula (9) in
 * _get_prev_sample) are such combinations, and the post-step clip of pipeline_pndm.py:108-109 is the clamp.
 * Per element r = 0; r += coeffs[j] * terms[j][i] for j ascending, each operation rounded once in fp32.  terms and out are 16-byte
 * aligned.  Aliasing: out may be a term's own buffer (same base pointer: every element is read before it is written; the in-place
 * clamp of the ANP projection is k = 1, out = terms[0]); any other overlap of out with a term over n floats is BD_ERR_INVALID. */
#define BD_LINCOMB_MAX 6
int bd_lincomb(int k, const float* const* terms, const float* coeffs, int64_t n, int clip, float clip_range, float* out,
               bd_stream_t stream);

/* f-4: one DPM-Solver / DPM-Solver++ multistep update (scheduling_dpmsolver_multistep.py:301-505) over n dense fp32 elements of one
 * common layout, in one launch.  Per element, fp32, in this order (e = model_output, x = sample):
 *     m0   = convert ? (x - sigma_s e) / alpha_s : e          x0-prediction (dpmsolver++) or the eps prediction as it is (dpmsolver)
 *     m0   = x0_clip ? clamp(m0, -x0_range, x0_range) : m0    thresholding with sample_max_value == 1
 *     prev = cx x + c0 m0 [+ c1 m1] [+ c2 m2]                 m1 / m2 NULL: the term is absent
 *     prev = clip ? clamp(prev, -clip_range, clip_range) : prev
 * m0 is written to m0_out (NULL: not written), prev to prev_out.  The scalars are host values: D1 and D2 of the second and third order
 * updates are expanded by the caller into the coefficients of the stored converted outputs m0, m1, m2 (newest first).
 * An output may alias an input only with an identical base pointer (prev_out == sample; m0_out == the oldest history buffer, also when
 * that buffer is passed as m2): every element is read into registers before its index is written.
 * Host checks before the launch (BD_ERR_INVALID, message names bd_dpm_step): null descriptor, n <= 0, a null model_output / sample /
 * prev_out, a pointer that is not 16-byte aligned, an output that overlaps an input (or the other output) in any other way.
 * HBM-bound: 16-byte accesses over n / 4, a scalar tail of n % 4, at most 4096 blocks of 256 threads with a grid-stride loop. */
typedef struct {
    int64_t n;
    const float* model_output; const float* sample;
    const float* m1; const float* m2;            /* previous converted outputs, newest first; may be NULL */
    float* m0_out; float* prev_out;              /* m0_out may be NULL                                    */
    int convert; float alpha_s, sigma_s;
    int x0_clip; float x0_range;
    float cx, c0, c1, c2;
    int clip; float clip_range;
} bd_dpm_step_desc;
int bd_dpm_step(const bd_dpm_step_desc* d, bd_stream_t stream);

/* f-4: one whole UniPC step (scheduling_unipc_multistep.py:257-601, B(h) version, epsilon prediction) over n dense fp32 elements of one
 * common layout, in one launch: conversion of the model output, the corrector (UniC) that turns the sample the previous predictor
 * produced into the corrected sample, and the predictor (UniP) from there.  Per element, fp32, in this order (e = model_output,
 * x = sample, l = last_sample, h1 / h2 / h3 = the stored converted outputs of the previous steps, newest first):
 *     m0   = convert ? (x - sigma_s e) / alpha_s : e                          predict_x0, or the eps prediction as it is
 *     m0   = x0_clip ? clamp(m0, -x0_range, x0_range) : m0                    thresholding with sample_max_value == 1
 *     xc   = last_sample ? kl l + k0 m0 + k1 h1 [+ k2 h2] [+ k3 h3] : x       corrector; h2 / h3 NULL: the term is absent
 *     prev = px xc + p0 m0 [+ p1 h1] [+ p2 h2]                                predictor; h1 / h2 NULL: the term is absent
 *     prev = clip ? clamp(prev, -clip_range, clip_range) : prev
 * m0 is written to m0_out, xc to corrected_out (either may be NULL: not written), prev to prev_out.  The scalars are host values: the
 * caller expands the D1 differences and the rho weights of both updates into coefficients of the tensors; the coefficient of an absent
 * term is ignored.  last_sample requires h1.
 * An output may alias an input only with an identical base pointer (prev_out == sample; corrected_out == last_sample; m0_out == the
 * oldest history buffer, also when that buffer is read as h2 or h3): every element is read into registers before its index is written.
 * Host checks before the launch (BD_ERR_INVALID, message names bd_unipc_step): null descriptor, n <= 0, a null model_output / sample /
 * prev_out, last_sample without h1, a pointer that is not 16-byte aligned, an output that overlaps an input or another output in any
 * other way.
 * HBM-bound: 16-byte accesses over n / 4, a scalar tail of n % 4, at most 4096 blocks of 256 threads with a grid-stride loop. */
typedef struct {
    int64_t n;
    const float* model_output; const float* sample;
    const float* last_sample;                    /* the corrected sample of the previous step; NULL: no corrector */
    const float* h1; const float* h2; const float* h3;   /* previous converted outputs, newest first; may be NULL */
    float* m0_out; float* corrected_out; float* prev_out;   /* m0_out and corrected_out may be NULL              */
    int convert; float alpha_s, sigma_s;
    int x0_clip; float x0_range;
    float kl, k0, k1, k2, k3;
    float px, p0, p1, p2;
    int clip; float clip_range;
} bd_unipc_step_desc;
int bd_unipc_step(const bd_unipc_step_desc* d, bd_stream_t stream);

/* f-4: one DEIS multistep update (scheduling_deis_multistep.py:240-473, log-rho version, epsilon prediction) over n dense fp32 elements of
 * one common layout, in one launch.  Per element, fp32, in this order (e = model_output, x = sample, m1 / m2 = the stored converted
 * outputs of the previous steps, newest first):
 *     x0   = (x - sigma_s e) / alpha_s
 *     x0   = x0_clip ? clamp(x0, -x0_range, x0_range) : x0        thresholding with sample_max_value == 1
 *     m0   = (x - alpha_s x0) / sigma_s                           the eps prediction back from x0: not e bitwise, as in the reference
 *     m1 == NULL:  prev = cx x - c0 m0                            first order: cx = alpha_t / alpha_s, c0 = sigma_t (exp(h) - 1)
 *     else:        prev = alpha_t * (x / alpha_s + k0 m0 + k1 m1 [+ k2 m2])     summed left to right; x / alpha_s is a true division
 *     prev = clip ? clamp(prev, -clip_range, clip_range) : prev
 * m0 is written to m0_out (NULL: not written), prev to prev_out.  The scalars are host values; those of the branch not taken are ignored.
 * An output may alias an input only with an identical base pointer (prev_out == sample; m0_out == the oldest history buffer, also when
 * that buffer is read as m2): every element is read into registers before its index is written.
 * Host checks before the launch (BD_ERR_INVALID, message names bd_deis_step): null descriptor, n <= 0, a null model_output / sample /
 * prev_out, alpha_s <= 0, sigma_s <= 0, m2 without m1, a pointer that is not 16-byte aligned, an output that overlaps an input (or the
 * other output) in any other way.
 * HBM-bound: 16-byte accesses over n / 4, a scalar tail of n % 4, at most 4096 blocks of 256 threads with a grid-stride loop. */
typedef struct {
    int64_t n;
    const float* model_output; const float* sample;
    const float* m1; const float* m2;            /* previous converted outputs, newest first; may be NULL */
    float* m0_out; float* prev_out;              /* m0_out may be NULL                                    */
    float alpha_s, sigma_s;
    int x0_clip; float x0_range;
    float cx, c0;                                /* first order (m1 == NULL)                              */
    float alpha_t, k0, k1, k2;                   /* second / third order                                  */
    int clip; float clip_range;
} bd_deis_step_desc;
int bd_deis_step(const bd_deis_step_desc* d, bd_stream_t stream);

/* f-4: one transition of a sigma-space (k-diffusion) sampler -- Heun (scheduling_heun_discrete.py:193-275), linear multistep
 * (scheduling_lms_discrete.py:217-285) and Euler as the first order of both -- over n dense fp32 elements of one common layout, in one
 * launch, together with the NEXT evaluation's scale_model_input.  Per element, fp32, in this order (e = model_output, x = sample,
 * h1 / h2 / h3 = the stored derivatives, newest first):
 *     x0   = x - sigma_in e                                 pred_original_sample
 *     d    = (x - x0) / sigma_in                            the ODE derivative as the reference rounds it (d != e bitwise)
 *     dd   = average ? (h1 + d) / 2 : d                     Heun's second stage; h1 = the first stage's derivative, required then
 *     acc  = c0 dd [+ c1 h1] [+ c2 h2] [+ c3 h3]            added left to right; h* NULL: the term is absent; average: no h terms
 *     prev = (base ? base : x) + acc                        Heun's second stage restarts from the sample of the first
 *     sc   = prev / in_div                                  in_div = sqrt(sigma_next^2 + 1), a host fp32 value; a true division
 *     if clip: sc = clamp(sc, -clip_range, clip_range); prev = sc in_div
 * Heun / Euler: c0 = dt = sigma_next - sigma; LMS: the integrated Lagrange coefficients.  x0 goes to x0_out, d (before the average) to
 * d_out, prev to prev_out, sc to scaled_out; all but prev_out may be NULL (not written).  The reference has no clip for these
 * schedulers: `clip` is this project's inference-time clipping defence, a clamp of the sample in the coordinates the model sees;
 * with clip == 0 the arithmetic is the reference's.
 * An output may alias an input only with an identical base pointer (d_out == the oldest history buffer, also when that buffer is read
 * as a term; prev_out == sample): every element is read into registers before its index is written.
 * Host checks before the launch (BD_ERR_INVALID, message names bd_sigma_step): null descriptor, n <= 0, a null model_output / sample /
 * prev_out, sigma_in <= 0, in_div <= 0, average without h1, average with h2 / h3 or a non-zero c1 / c2 / c3, h2 without h1 or h3
 * without h2, a pointer that is not 16-byte aligned, an output that overlaps an input or another output in any other way.
 * HBM-bound: 16-byte accesses over n / 4, a scalar tail of n % 4, at most 4096 blocks of 256 threads with a grid-stride loop. */
typedef struct {
    int64_t n;
    const float* model_output; const float* sample;
    const float* base;                                   /* NULL: the update starts from `sample`                  */
    const float* h1; const float* h2; const float* h3;   /* stored derivatives, newest first; may be NULL          */
    float* x0_out; float* d_out; float* prev_out; float* scaled_out;   /* all but prev_out may be NULL             */
    float sigma_in; int average;
    float c0, c1, c2, c3;
    float in_div;
    int clip; float clip_range;
} bd_sigma_step_desc;
int bd_sigma_step(const bd_sigma_step_desc* d, bd_stream_t stream);

/* f-4: one first order transition of a stochastic sigma-space sampler in one launch -- Euler with Karras churn
 * (scheduling_euler_discrete.py:257-354), Euler-ancestral (scheduling_euler_ancestral_discrete.py:193-281) and the second stage of
 * KDPM2-ancestral (scheduling_k_dpm_2_ancestral_discrete.py:243-329) -- with the NEXT evaluation's scale_model_input, as bd_sigma_step.
 * Per element, fp32, each operation rounded once, in this order (e = model_output, x = sample, z = noise):
 *     xh   = churn ? x + (z s_noise) churn_mul : x          churn_mul = (sigma_hat^2 - sigma^2) ** 0.5, a host fp32 value
 *     x0   = xh - sigma_in e                                sigma_in = sigma_hat, or sigma_interpol in KDPM2's second stage
 *     d    = (xh - x0) / sigma_in
 *     prev = (base ? base : xh) + d dt
 *     if up: prev = prev + z sigma_up                       the ancestral noise
 *     sc   = prev / in_div;  if clip: sc = clamp(sc, -clip_range, clip_range); prev = sc in_div        exactly as bd_sigma_step
 * x0 goes to x0_out, prev to prev_out, sc to scaled_out; x0_out and scaled_out may be NULL (not written).  With neither churn nor
 * up the noise buffer is not read (it is still required) and the result is bd_sigma_step's first order one.
 * prev_out may be `sample` itself (identical base pointer); no other buffer may overlap another.
 * Host checks before the launch (BD_ERR_INVALID, message names bd_sigma_noise_step): null descriptor, n <= 0, a null model_output /
 * sample / noise / prev_out, sigma_in <= 0, in_div <= 0, sigma_up < 0, churn together with up, churn with churn_mul <= 0, a pointer that
 * is not 16-byte aligned, an output that is or overlaps an input or another output (but prev_out == sample).
 * Same launch shape as bd_sigma_step. */
typedef struct {
    int64_t n;
    const float* model_output; const float* sample; const float* noise;
    const float* base;                                   /* NULL: the update starts from xh                        */
    float* x0_out; float* prev_out; float* scaled_out;   /* all but prev_out may be NULL                           */
    float sigma_in, dt;
    int churn; float s_noise, churn_mul;
    int up; float sigma_up;
    float in_div;
    int clip; float clip_range;
} bd_sigma_noise_step_desc;
int bd_sigma_noise_step(const bd_sigma_noise_step_desc* d, bd_stream_t stream);

/* out = (x * mul) / div over n dense fp32 elements, each operation rounded once: the start of a sigma-space chain
 * (init * init_noise_sigma, then / sqrt(sigma_0^2 + 1)) and the schedulers' public scale_model_input (mul = 1).  Same launch shape
 * as bd_sigma_step.  BD_ERR_INVALID: a null pointer, n <= 0, div <= 0, a pointer that is not 16-byte aligned, out overlapping x
 * without being x. */
int bd_scale_input(const float* x, int64_t n, float mul, float div, float* out, bd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * RePaint inpainting (schedulers/scheduling_repaint.py:216-318, epsilon prediction): the reverse step with its re-noised copy of
 * the original image and the mask blend in one launch, and the "time travel" forward recurrence of undo_step.
 *
 * Both work on an [N,C,H,W] problem given by ELEMENT strides.  The dense operands (model_output, sample, noise, prev_sample,
 * pred_original; sample, the noises and out of the undo) share `stride`, which must describe a dense layout: some order of the four
 * dimensions in which each stride is the product of the sizes inside it (NCHW, or the NHWC storage the pipelines keep).  The
 * broadcast operands (original_image, mask, shift) carry strides of their own, any of which may be 0, so [1,1,H,W], [B,1,H,W],
 * [1,C,H,W], [C,H,W] and full tensors are read without being expanded in memory; they are indexed from the logical (n,c,h,w).
 *
 * bd_repaint_step, per element, fp32, in this order (a_t = alphas_cumprod[t], a_prev = prev_t >= 0 ? alphas_cumprod[prev_t] :
 * final_alpha_cumprod; e = model_output, x = sample, z = noise, m = mask):
 *     x0      = (x - sqrt(1 - a_t) e) / sqrt(a_t), clamped to +-clip_sample_range when clip_sample
 *     sd      = eta sqrt(((1 - a_prev) / (1 - a_t)) (1 - a_t / a_prev))
 *     unknown = sqrt(a_prev) x0 + sqrt(1 - a_prev - sd sd) e   [+ sd z  iff t > 0 and eta > 0]
 *     known   = sqrt(a_prev) orig + sqrt(1 - a_prev) z         [+ (1 - sqrt(a_prev)) shift  iff shift != NULL]
 *     prev    = m known + (1 - m) unknown
 * The reference draws z on every call (also for eta == 0 and t == 0), so `noise` is always required; masks are fp32 and need not
 * be binary.  `shift` is this project's trigger-consistent variant: with shift = R, the BadDiffusion trigger image, the known region is
 * re-noised as a poisoned chain is (loss.py:275: x_t = sqrt(a) x0 + sqrt(1-a) eps + (1 - sqrt(a)) R); NULL is the reference.
 *
 * bd_repaint_undo: for i = 0..k-1:  x = sqrt(1 - betas[t+i]) x + sqrt(betas[t+i]) z_i   [+ (1 - sqrt(1 - betas[t+i])) shift],
 * x carried in registers in exactly this order; `noises` is a HOST array of k device pointers read at call time (as bd_lincomb takes
 * its terms).  One launch covers BD_REPAINT_UNDO_MAX sub-steps; a larger k runs as consecutive launches (the later ones in place on
 * `out`), bit-identical to k calls with one noise each.  out may alias sample.
 *
 * Both are HBM-bound: 256-thread blocks, at most 2048 of them with a grid-stride loop, 16-byte accesses when every dense pointer is
 * 16-byte aligned and the element count is a multiple of 4, one element per thread otherwise.
 * Host checks before any launch (BD_ERR_INVALID, message names the entry point): null descriptor / required pointer (noises and each
 * noises[i] included), N, C, H, W <= 0, a negative stride, a `stride` that is not dense, t < 0, t or prev_t >= n_alphas, k < 1,
 * t + k > n_betas.  BD_ERR_UNSUPPORTED for N*C*H*W >= 2^31.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int N, C, H, W;
    int64_t stride[4];                   /* (n,c,h,w) element strides of the dense operands        */
    const float* model_output; const float* sample; const float* noise;
    float* prev_sample; float* pred_original;   /* pred_original (the clamped x0) may be NULL       */
    const float* original_image; int64_t orig_stride[4];
    const float* mask; int64_t mask_stride[4];
    const float* shift; int64_t shift_stride[4];   /* optional (NULL = reference behaviour)         */
    const float* alphas_cumprod; int n_alphas;     /* [n_alphas] device                             */
    int t, prev_t; float final_alpha_cumprod; float eta;
    int clip_sample; float clip_sample_range;
} bd_repaint_step_desc;
int bd_repaint_step(const bd_repaint_step_desc* d, bd_stream_t stream);

#define BD_REPAINT_UNDO_MAX 8
typedef struct {
    int N, C, H, W;
    int64_t stride[4];                   /* (n,c,h,w) element strides of sample, the noises and out */
    const float* sample; float* out;
    const float* shift; int64_t shift_stride[4];   /* optional                                      */
    const float* betas; int n_betas;               /* [n_betas] device                              */
    int t, k;                            /* sub-steps use betas[t .. t+k-1]                         */
} bd_repaint_undo_desc;
int bd_repaint_undo(const bd_repaint_undo_desc* d, const float* const* noises, bd_stream_t stream);

/* f-4: Adversarial Neuron Pruning (anp_model.py:490-514 PerturbConv2d; anp_util.py:60-88 convert_model; anp_defense.py:147 the loss that is
 * maximised).  Every Conv2d of the network is followed by a per-output-channel affine map y_c <- w_c y_c + b_c (an eval-mode batch norm with mean 0,
 * variance 1, eps 0); it commutes with the convolution, so the perturbed network is bd_unet_forward on EFFECTIVE parameters
 *   W'_c = w_c W_c,  b'_c = w_c b_c + b_c(perturbation)
 * and the perturbation's gradient is a row-wise contraction of bd_unet_backward's ordinary weight gradient:
 *   dL/dw_c = sum_k dL/dW'_ck W_ck + dL/db'_c b_c,   dL/db_c = dL/db'_c.
 * items: DEVICE array [n_items][5] int64 = (weight offset, bias offset or -1, Cout, row length = elements per output channel, offset of the
 * layer's channels in pert_w / pert_b / grad_w / grad_b); total_rows = sum of Cout.  bd_anp_apply first copies params -> eff (all other
 * tensors unchanged), then rewrites the conv rows and biases. */
int bd_anp_apply(const float* params, int64_t nparams, const float* pert_w, const float* pert_b, const int64_t* items, int n_items,
                 int64_t total_rows, float* eff, bd_stream_t stream);
/* row_norm (optional, needs pert_w): |w_c| * ||(dL/dW'_c, dL/db'_c)||, the gradient norm of the layer's own weight row + bias in the perturbed
 * network.  PerturbConv2d's conv weights are fresh trainable Parameters (anp_model.py:492-505; anp_util.freeze ran before the wrap), so the
 * reference's clip_grad_norm_(model.parameters(), 1.0) (anp_defense.py:152) takes its coefficient from bn AND conv gradients. */
int bd_anp_grad(const float* params, const float* grad_eff, const int64_t* items, int n_items, int64_t total_rows, const float* pert_w,
                float* grad_w, float* grad_b, float* row_norm, bd_stream_t stream);

/* (x/2+0.5).clamp(0,1): NCHW or NHWC(ld) in -> NHWC float [B,H,W,C] and/or uint8 round(255 x).
 * BD_ERR_INVALID: null x, neither output, a size <= 0, or an NHWC source with ld < C (ld is not read for NCHW). */
int bd_to_image(const float* x, int src_is_nhwc, int64_t ld, int B, int C, int H, int W,
                float* out_f32, uint8_t* out_u8, bd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * a-4a: sinusoidal timestep embedding (models/embeddings.py:22-62).  t is int64 [B] (or one value
 * broadcast when t_stride == 0).
 * ------------------------------------------------------------------------------------------------ */
int bd_timestep_embedding(const int64_t* t, int t_stride, int B, int dim, int flip_sin_to_cos,
                          float freq_shift, float* out, bd_stream_t stream);
/* the same for fp32 timesteps, which may be fractional (the sigma-space samplers visit np.linspace(0, T - 1, N)): the argument is
 * t[b * t_stride] * f where the int64 entry point has (float)t[b * t_stride] * f, so integral values give identical bits. */
int bd_timestep_embedding_f32(const float* t, int t_stride, int B, int dim, int flip_sin_to_cos,
                              float freq_shift, float* out, bd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GroupNorm (+ optional SiLU) over NHWC(ld).  Replaces nn.GroupNorm + F.silu at resnet.py:559,591,
 * attention.py:125, unet_2d.py:312-313 and their autograd backward.
 * Workspace: bd_gn_workspace_bytes(B, C), a bound: at least what bd_gn_fwd and bd_gn_bwd need for any (HW, G) they take at that
 * (B, C); the exact need of one shape and direction is bd_gn_plan(...).workspace_bytes.  mean/rstd are [B, G] fp32 outputs saved
 * for backward.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int B, HW, C, G; float eps; int silu;
    const float* x; int64_t ldx;
    const float* gamma; const float* beta;
    float* y; int64_t ldy;
    float* mean; float* rstd;       /* [B,G] */
    void* workspace; size_t workspace_bytes;
    uint16_t* y_split; int64_t ldys;   /* optional: y also / only (y == NULL) as split planes [B*HW, ldys], see
                                          "Pre-split operands" below: the operand format of bd_conv3x3_ps */
    const double* stats; int stats_splits;   /* optional (round 4): [B][stats_splits][G][2] partial (sum, sum of squares) of x written by the
                                          producer of x (bd_conv3x3_ps gn_part); read only when bd_gn_fwd_takes_stats(): the statistics
                                          pass over x is skipped                                                                     */
} bd_gn_fwd_desc;
size_t bd_gn_workspace_bytes(int B, int C);
int bd_gn_fwd_takes_stats(int B, int HW, int C, int G);   /* 1: this shape runs the statistics / apply passes (images too large for the one-pass kernels) */
int bd_gn_fwd(const bd_gn_fwd_desc* d, bd_stream_t stream);

typedef struct {
    int B, HW, C, G; int silu;
    const float* x; int64_t ldx;            /* GN input saved from forward                     */
    const float* gamma; const float* beta;
    const float* mean; const float* rstd;
    const float* dy; int64_t lddy;          /* grad wrt the (activated) output                 */
    float* dx; int64_t lddx; int accumulate_dx;  /* dx (+)= ...                                */
    float* dgamma; float* dbeta;            /* [C], written (not accumulated); both NULL together with a NULL
                                               param_partials: no parameter gradient is computed or written
                                               (dx is the same launch, bit for bit)               */
    void* workspace; size_t workspace_bytes;
    float* dx_colsum; int64_t ld_colsum;    /* optional [B, C] (row stride ld_colsum): per-sample sum
                                               over pixels of the written dx (needs accumulate_dx=0);
                                               the time-embedding gradient of resnet.py:571            */
    uint16_t* dx_split; int64_t lddxs;      /* optional: the value stored to dx -- this launch's term (+ the existing dx when
                                               accumulate_dx) (+ dx_add) -- also / only (dx == NULL) as split planes         */
    const float* dx_add; int64_t ld_add;    /* optional: dx = (term (+ dx)) + dx_add, a second gradient of the same tensor
                                               folded into the store (the identity shortcut of resnet.py:596-600)     */
    float* param_partials;                  /* optional [B][2][C], caller storage: if set and bd_gn_bwd_defers(B, HW, C, G),
                                               the per-sample partial sums of (dgamma, dbeta) are left here and dgamma /
                                               dbeta are NOT written -- fold many layers later with ONE bd_gn_bwd_params
                                               launch (51 GroupNorms per CIFAR backward, one launch per segment)      */
    int dx_split_c0, dx_split_c1;           /* optional (round 4): only channels [c0, c1) of x go to dx_split, at plane column c - c0
                                               (whole 32-channel blocks; 0, 0 = all C).  The consumer that makes a tensor's gradient
                                               final hands the producer of that tensor its dY operand ready-split.            */
} bd_gn_bwd_desc;
int bd_gn_bwd(const bd_gn_bwd_desc* d, bd_stream_t stream);
/* 1 if this shape can leave its parameter partials to the caller (round 4: every valid shape -- the single-pass kernels write them
 * directly, the large-image path from its group-finalize launch), else 0 */
int bd_gn_bwd_defers(int B, int HW, int C, int G);
typedef struct {
    const float* partials;                  /* [B][2][C] as written through bd_gn_bwd_desc.param_partials */
    int C;
    float* dgamma; float* dbeta;            /* [C], written */
} bd_gn_param_item;
/* dgamma[c] / dbeta[c] = sum over the B samples of the partials, fixed order, for n layers in one launch
 * (the reduction over the batch of aten::native_group_norm_backward's weight / bias gradients, resnet.py:559,591) */
int bd_gn_bwd_params(const bd_gn_param_item* items, int n, int B, bd_stream_t stream);
/* Which kernels bd_gn_fwd (backward == 0) / bd_gn_bwd (backward != 0) launch for a shape and the workspace they need: host code only, a
 * copy of the plan and the workspace layout the launchers themselves read.  For tests and tools that must know which branch a shape takes
 * (DESIGN.md "GroupNorm dispatch").  BD_ERR_INVALID for a shape the launchers do not take. */
typedef struct {
    int resident;                   /* 1: one workgroup per (sample, channel block) holds its slab in registers; 0: the two-stage kernels */
    int nt, cb, q, R, E, emax;      /* resident: threads per workgroup, channels per block, float4 per pixel row (cb / 4), pixel rows in
                                       flight (nt / q), float4 per thread and tensor (ceil(HW / R)), and the EMAX of the <EMAX, nt>
                                       instantiation launched (4, 8 or 16); 0 otherwise */
    int S, threads, r, per;         /* two-stage: pixel splits of the statistics pass, threads per workgroup ((C / 4) * r), pixel rows in
                                       flight, pixel rows per block of the apply kernels; 0 otherwise */
    size_t workspace_bytes;         /* what the launcher asks of desc.workspace_bytes: forward two-stage [B][S][G][2] fp64 (0 resident); backward
                                       two-stage [B][S][3][C] fp32 rounded up to 256 + [B][G][2] fp32; backward resident [B][2][C] fp32 when the
                                       launcher owns the parameter sums (dgamma / dbeta set, no param_partials), which is what is reported here: the
                                       largest of the descriptor's variants (0 with param_partials or without dgamma / dbeta) */
} bd_gn_plan_info;
int bd_gn_plan(int B, int HW, int C, int G, int backward, bd_gn_plan_info* out);

/* ------------------------------------------------------------------------------------------------
 * Implicit-GEMM engine on f32 MFMA (v_mfma_f32_32x32x2_f32: exact fp32 products/accumulate).
 *     C[m,n] = out_scale * (alpha * sum_k A(m,k) B(n,k) + bias[n] + rowbias[m / rows_per_group, n]
 *                           + residual[m,n])   (+ C[m,n] if accumulate)
 * Operand kinds select how (row, k) maps to memory; see DESIGN.md "igemm".
 * Replaces aten::convolution / convolution_backward / addmm / mm / bmm / baddbmm of SURVEY 2.3.
 * ------------------------------------------------------------------------------------------------ */
/* arithmetic of the contraction:
 *   BD_MODE_F32     v_mfma_f32_32x32x2_f32, exact fp32 products and accumulation (157 TFLOP/s roof)
 *   BD_MODE_BF16X3  every fp32 operand is split on the fly into hi + lo bf16 (x = hi + lo + O(2^-17 x)) and the
 *                   product is hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation:
 *                   ~2^-16 relative error per product, 3 MFMAs on the 2.5 PFLOP/s pipe
 *   BD_MODE_BF16    single pass: every operand of every matrix product (convolution, GEMM, attention q k^T and P v) is
 *                   rounded once to bf16 RNE -- the hi plane above -- and the product is ONE v_mfma_f32_32x32x16_bf16
 *                   with fp32 accumulation (~2^-9 relative error per operand).  Everything else keeps fp32 arithmetic
 *                   and storage: activations, GroupNorm, SiLU, softmax, loss, clip, Adam, master weights, scheduler
 *                   steps.  Autocast with fp32 activation storage; bf16 has fp32's exponent range, so training needs
 *                   no loss scaling.  Same kernels, workspace and split-plane formats as BD_MODE_BF16X3, lo unread.   */
enum bd_compute_mode { BD_MODE_F32 = 0, BD_MODE_BF16X3 = 1, BD_MODE_BF16 = 2 };

enum bd_operand_kind {
    BD_OPK_DENSE = 0, /* KC: p[row*ld + k]            RC: p[k*ld + row]                          */
    BD_OPK_CONV = 1,  /* 3x3 gather of an NHWC tensor: KC rows = output pixels, k = tap*C + c;
                         RC rows = tap*C + c, k = output pixels (wgrad)                          */
    BD_OPK_TCONV = 2, /* KC only: rows = input pixels, k = tap*C + c over dY (dgrad, any stride) */
    BD_OPK_WGT = 3    /* RC only: rows = ci, k = tap*C + co over W[co][tap][ci]   (dgrad)        */
};
typedef struct {
    int kind;              /* bd_operand_kind                                                   */
    int kc;                /* 1: k-contiguous in memory (KC)  0: row-contiguous (RC)            */
    const float* p; int64_t ld;
    int64_t bs_outer, bs_inner;   /* batch strides (elements)                                   */
    int C, Hs, Ws, Ho, Wo, stride, pad_t, pad_l, ups;   /* conv geometry (CONV/TCONV/WGT)       */
    const uint16_t* split;   /* optional, BD_MODE_BF16X3 / BD_MODE_BF16 only: the same buffer already split into bf16 hi/lo by
                                bd_split_bf16 (blocked layout below; element e of p <-> e of split); used where the
                                engine has a loader for it (weights of conv fwd / dgrad), ignored otherwise -- p must
                                always be valid                                                               */
} bd_operand;
typedef struct {
    bd_operand A, B;
    int M, N, K;
    int batch_outer, batch_inner;            /* >= 1                                            */
    float* C; int64_t ldc; int64_t c_bs_outer, c_bs_inner;
    float alpha; float out_scale;
    const float* bias;
    const float* rowbias; int64_t ld_rowbias; int rows_per_group;
    const float* residual; int64_t ldr;      /* same batch strides as C                         */
    int accumulate;
    int ksplit;                              /* 0 = choose; >1 needs workspace                  */
    void* workspace; size_t workspace_bytes;
    int tile;                                /* 0 = choose, 128 or 64                           */
    int mode;                                /* bd_compute_mode                                 */
    float* a_colsum;                         /* optional [M]: sum_k A(m,k), fused (bias gradient of a
                                                wgrad, A = dY^T); needs DENSE row-contiguous A, batch 1 */
} bd_igemm_desc;
size_t bd_igemm_workspace_bytes(const bd_igemm_desc* d);
/* What bd_igemm decides for a descriptor: host code only, a copy of the plan the launcher itself reads.  bd_igemm_plan runs every check
 * of bd_igemm (same status, same message; a K split therefore needs workspace / workspace_bytes set) and launches nothing; it
 * dereferences none of the descriptor's pointers and reads only their alignment.  For tests and tools that must know which branch a
 * call takes (DESIGN.md "igemm dispatch"). */
enum bd_igemm_class {       /* loader pair of the launch; the profiler counts _WS and _SAME under the names of their plain siblings */
    BD_CLS_GENERIC = 0,     /* per-element loaders, any kind / alignment                                   */
    BD_CLS_CONV_FWD, BD_CLS_CONV_DGRAD, BD_CLS_CONV_WGRAD, BD_CLS_GEMM_NT, BD_CLS_GEMM_NN, BD_CLS_GEMM_TN,
    BD_CLS_CONV_FWD_WS, BD_CLS_CONV_DGRAD_WS,   /* weights (B) read from the pre-split planes (operand.split) */
    BD_CLS_CONV_WGRAD_SAME                      /* stride-1 same-size geometry: slim gather loader            */
};
typedef struct {
    int cls;                    /* bd_igemm_class                                                                             */
    int fast;                   /* both operands meet the conditions of their FAST loader (cls is GENERIC without it)          */
    int a_vec, b_vec;           /* float4 loads allowed on the operand: aligned p, ld and batch strides % 4 == 0, and K, C or the
                                   row count % 4 == 0 as the kind requires; the generic loaders read scalars without it        */
    int tile;                   /* 64 or 128                                                                                   */
    int threads;                /* per workgroup: 512 for the 128 x 128 tiles of the fast classes in the bf16 modes, else 256  */
    int depth;                  /* prefetch register sets of the split-bf16 kernel (1 or 2); 0 in BD_MODE_F32                  */
    int ksplit, chunks_per_split;   /* K slices and 32-wide chunks per slice (the last slice may be shorter, never empty)      */
    int reduce;                 /* second pass of a K split: 0 none, 1 scalar, 2 float4, 3 float4 with eight lanes per output  */
    size_t workspace_bytes;     /* = bd_igemm_workspace_bytes                                                                  */
    size_t colsum_offset;       /* bytes in front of the a_colsum partial rows [ksplit][M] (0 without a K split)               */
} bd_igemm_plan_info;
int bd_igemm_plan(const bd_igemm_desc* d, bd_igemm_plan_info* out);
/* Split an fp32 buffer into bf16 hi/lo exactly as the BF16X3 kernels do on the fly: hi = bf16 RNE of x (round 6; rounds 1 - 5
 * truncated: one bit less), lo = bf16 RNE of (x - hi): x = hi + lo to 2^-18 |x|.  Blocked layout, 2n uint16: for element e, hi at out[(e/32)*64 + e%32] and lo 32 entries
 * further -- one 32-element K chunk of a row is one 128-byte line (64 B hi | 64 B lo), as wide as its fp32 source.
 * n % 32 == 0, 16-byte aligned pointers.  Run once per forward over the flat weight buffer (bd_unet_forward).   */
int bd_split_bf16(const float* src, int64_t n, uint16_t* out, bd_stream_t stream);
int bd_igemm(const bd_igemm_desc* d, bd_stream_t stream);

/* Convenience wrappers over bd_igemm (all NHWC(ld), weights [Cout][3][3][Cin]).
 * conv fwd:   y[B,Ho,Wo,Cout] = conv3x3(x[B,Hs,Ws,Cin] (nearest-upsampled x2 if ups), stride, pads)
 *             (+bias) (+rowbias per sample) (+residual) ; resnet.py:493,514,118,185,201-203
 * dgrad:      dx[B,Hs<<ups,Ws<<ups,Cin] (the conv's own input grid)
 * wgrad:      dw[Cout][3][3][Cin] (written) and, if db != NULL, db[Cout] = sum over pixels of dy      */
typedef struct {
    int B, Hs, Ws, Cin, Cout, stride, pad_t, pad_l, ups; /* Ho/Wo derived by the callee         */
    int Ho, Wo;
    const float* x; int64_t ldx;
    const float* w;
    const float* bias;
    const float* rowbias; int64_t ld_rowbias;   /* [B, Cout] added per sample (time embedding)  */
    const float* residual; int64_t ldr;
    float out_scale;
    float* y; int64_t ldy;
    void* workspace; size_t workspace_bytes;
    int mode;                                   /* bd_compute_mode */
    const uint16_t* w_split;                    /* optional: w already split by bd_split_bf16           */
} bd_conv3x3_fwd_desc;
int bd_conv3x3_fwd(const bd_conv3x3_fwd_desc* d, bd_stream_t stream);

typedef struct {
    int B, Hs, Ws, Cin, Cout, stride, pad_t, pad_l, ups, Ho, Wo;
    const float* dy; int64_t lddy;
    const float* w;
    float* dx; int64_t lddx; int accumulate;   /* dx over the (virtual, upsampled) input grid   */
    void* workspace; size_t workspace_bytes;
    int mode;                                   /* bd_compute_mode */
    const uint16_t* w_split;                    /* optional: w already split by bd_split_bf16           */
} bd_conv3x3_dgrad_desc;
int bd_conv3x3_dgrad(const bd_conv3x3_dgrad_desc* d, bd_stream_t stream);

typedef struct {
    int B, Hs, Ws, Cin, Cout, stride, pad_t, pad_l, ups, Ho, Wo;
    const float* x; int64_t ldx;
    const float* dy; int64_t lddy;
    float* dw;
    void* workspace; size_t workspace_bytes;
    int mode;                                   /* bd_compute_mode */
    float* db;                                  /* optional [Cout]: bias gradient sum_pixels dy, fused  */
} bd_conv3x3_wgrad_desc;
int bd_conv3x3_wgrad(const bd_conv3x3_wgrad_desc* d, bd_stream_t stream);
/* An upper bound over the three directions.  For every shape the direct "thin" kernels below take it is >= the workspace_bytes their plan
 * reports (they size their partial rows to fit it); the value is the same for every shape. */
size_t bd_conv3x3_workspace_bytes(int B, int Ho, int Wo, int Hs, int Ws, int Cin, int Cout, int ups);
/* What the three entry points above decide for the 3- and 1-channel layers (conv_in, conv_out), which run as direct kernels
 * (csrc/conv_thin.hip) instead of on bd_igemm: host code only, the plan the launchers themselves read.  Each query runs the checks its entry
 * point runs before it dispatches (same status, same message; a thin weight gradient therefore needs workspace / workspace_bytes set) and
 * launches nothing; it dereferences none of the descriptor's pointers and reads only their alignment.  With path BD_THIN_IGEMM every
 * other field is 0 and bd_igemm decides the rest (bd_igemm_plan).  For tests and tools that must know which branch a call takes
 * (DESIGN.md "Dispatch branches of the thin convolutions"). */
enum bd_thin_path {
    BD_THIN_IGEMM = 0,          /* not a thin shape, or a guard failed: the implicit-GEMM engine runs the call               */
    BD_THIN_EXPAND_FMA,         /* few -> many channels, fp32 FMAs: conv_in forward, conv_out data gradient                  */
    BD_THIN_EXPAND_MFMA,        /* the same on the matrix pipe (bf16 modes, 3 channels, W % 32 == 0)                         */
    BD_THIN_CONTRACT,           /* many -> few: conv_out forward (128 -> 3 or 1)                                             */
    BD_THIN_CONTRACT_DGRAD,     /* conv_in data gradient (C -> 3 or 1)                                                       */
    BD_THIN_WGRAD_MFMA,         /* weight gradients: matrix pipe (bf16 modes, 3 channels, W % 32 == 0, pad 1)                */
    BD_THIN_WGRAD_ROW,          /*   wave per row segment (3 channels, W % 32 == 0, pad 1, 8-byte aligned wide tensor)       */
    BD_THIN_WGRAD_CIN,          /*   general kernel of conv_in                                                               */
    BD_THIN_WGRAD_COUT          /*   general kernel of conv_out                                                              */
};
typedef struct {
    int path;                   /* bd_thin_path                                                                              */
    int J;                      /* channels of the narrow side: 3 or 1                                                       */
    int loops;                  /* iters (expand), segs_per_wave (contract-dgrad, wgrad-row), steps_per_wg (wgrad-MFMA), else 1 */
    int pix_per_block;          /* pixels one workgroup reduces in the general weight-gradient kernels, else 0               */
    int grid_x, grid_y;         /* of the main kernel                                                                        */
    int partial_rows;           /* rows the weight-gradient second pass sums (= grid_x), else 0                              */
    size_t workspace_bytes;     /* partial_rows x (Cout * 9 * Cin + Cout) floats; 0 for forward and data gradient            */
    const char* prof_class;     /* the profiler class the launch is counted under, or NULL (the weight gradients have none)  */
} bd_conv3x3_thin_plan_info;
int bd_conv3x3_fwd_plan(const bd_conv3x3_fwd_desc* d, bd_conv3x3_thin_plan_info* out);
int bd_conv3x3_dgrad_plan(const bd_conv3x3_dgrad_desc* d, bd_conv3x3_thin_plan_info* out);
int bd_conv3x3_wgrad_plan(const bd_conv3x3_wgrad_desc* d, bd_conv3x3_thin_plan_info* out);

/* ------------------------------------------------------------------------------------------------
 * Pre-split operands ("split planes"): an activation / gradient / weight matrix [rows, C] whose every
 * 32-channel block of a row is one 128-byte line, 64 B of bf16 hi then 64 B of bf16 lo (hi = bf16
 * RNE, lo = bf16 RNE of the remainder: exactly what BD_MODE_BF16X3 computes on the fly), i.e. the
 * bd_split_bf16 layout with a leading dimension: element (r, c) lives at uint16 index
 *     2*r*ld + (c/32)*64 + plane*32 + c%32          (ld % 32 == 0, 128-byte aligned base).
 * Same 4 bytes per element as fp32.  Producers: bd_split_rows (from fp32), bd_gn_fwd / bd_gn_bwd
 * (y_split / dx_split), bd_split_wt (transposed conv weights for the data gradient).
 * bd_split_rows / bd_split_rows_ups2: C % 32, ld_dst % 32, ld_src % 4, 16-byte aligned src, 128-byte aligned dst (else
 * BD_ERR_UNSUPPORTED); ld_src < C or ld_dst < C is BD_ERR_INVALID.  Columns C..ld of a row are neither read nor written.
 * bd_conv3x3_ps: stride-1 pad-1 3x3 convolution (direction +1) or its data gradient (direction -1, over
 * the transposed weight planes) with both operands streamed global -> LDS by DMA; bit-identical to
 * bd_conv3x3_fwd / bd_conv3x3_dgrad in BD_MODE_BF16X3.  Replaces aten::convolution(_backward input) of
 * resnet.py:493,514 on the large layers.  H, W powers of two; K % 32 == 0; N % 128 == 0.
 * ------------------------------------------------------------------------------------------------ */
int bd_split_rows(const float* src, int64_t ld_src, int64_t rows, int C, uint16_t* dst, int64_t ld_dst, bd_stream_t stream);
/* src [B,H,W,C] fp32 -> split planes of its nearest-neighbour x2 upsampling [B,2H,2W,C] (Upsample2D, resnet.py:126-161) */
int bd_split_rows_ups2(const float* src, int64_t ld_src, int B, int H, int W, int C, uint16_t* dst, int64_t ld_dst, bd_stream_t stream);
/* W[Cout][3][3][Cin] fp32 -> split planes of Wt[Cin][3][3][Cout] (rows = ci, k = tap*Cout + co) */
int bd_split_wt(const float* w, int Cin, int Cout, uint16_t* out, bd_stream_t stream);
typedef struct {
    int B, H, W;                    /* image grid (input == output)                                  */
    int K, N;                       /* contraction channels, output channels (fwd: Cin, Cout; dgrad: Cout, Cin) */
    int direction;                  /* +1: y[p] = sum_tap x[p + tap] W[n][tap][:]   -1: dx[p] = sum_tap dy[p - tap] Wt[n][tap][:] */
    const uint16_t* x_split; int64_t ldx;   /* [B*H*W, ldx] split planes                              */
    const uint16_t* w_split;        /* [N][9][K] split planes (bd_split_bf16 of W, or bd_split_wt)   */
    const float* bias;              /* [N] or NULL                                                   */
    const float* rowbias; int64_t ld_rowbias;   /* [B, N] per-sample bias or NULL                    */
    const float* residual; int64_t ldr;
    float out_scale;                /* y = out_scale * (conv + bias + rowbias + residual)            */
    float* y; int64_t ldy; int accumulate;
    void* workspace; size_t workspace_bytes;   /* >= bd_conv3x3_ps_workspace_bytes(): K-split slabs of the small-layer variant */
    double* gn_part; int gn_groups; /* optional (round 4): the statistics of the GroupNorm that reads y next from this call's epilogue instead
                                       of a pass over y.  The plan uses it for resnet.py:591 (norm2 behind conv1) only: a conv2 -> next
                                       block's norm1 hand-over is NOT implemented (norm1 inputs are concat buffers / residual sums):
                                       [B][S][gn_groups][2] fp64 partial (sum, sum of squares) per sample and 256-pixel tile, S =
                                       bd_conv3x3_ps_gn_splits() > 0; forward calls with exactly one of rowbias / residual, no accumulate.
                                       Hand them to bd_gn_fwd as stats / stats_splits.                                              */
    int mode;                       /* bd_compute_mode of the products: BD_MODE_BF16X3 (or 0, the zero-initialised default: these
                                       kernels have no f32 form) = hi*hi + hi*lo + lo*hi, BD_MODE_BF16 = hi*hi; other values BD_ERR_INVALID */
} bd_conv3x3_ps_desc;
/* BD_ERR_INVALID before any launch: a leading dimension below the channel count of its buffer -- ldx < K, ldy < N, ldr < N (residual given),
 * ld_rowbias < N (rowbias given); bd_conv3x3_ps_wgrad: ldx < Cin, lddy < Cout. */
size_t bd_conv3x3_ps_workspace_bytes(const bd_conv3x3_ps_desc* d);
int bd_conv3x3_ps_gn_splits(int B, int H, int W, int K, int N, int groups);   /* 0: this call cannot write GroupNorm partials */
int bd_conv3x3_ps(const bd_conv3x3_ps_desc* d, bd_stream_t stream);
/* What bd_conv3x3_ps decides for a descriptor: host code only, a copy of the plan the launcher, bd_conv3x3_ps_workspace_bytes and
 * bd_conv3x3_ps_gn_splits themselves read.  bd_conv3x3_ps_plan runs the checks of bd_conv3x3_ps on the descriptor's numbers (shape,
 * direction, mode, leading dimensions: same status, same message) and launches nothing; it reads none of the descriptor's pointers beyond
 * whether residual / rowbias are set, and neither needs nor checks a workspace.  For tests and tools that must know which branch a call
 * takes (DESIGN.md "Dispatch branches of the split-plane convolutions"). */
enum bd_ps_kernel {
    BD_PS_256 = 0,              /* conv_ps_kernel: 256 x 128 tiles, three LDS stages, no K split (>= 96 tiles)                  */
    BD_PS_256_SHARED_TAP,       /* conv_ps3_kernel: the same tiles with the vertical taps shared (W >= 16, whole tiles per image) */
    BD_PS_128                   /* conv_ps128_kernel: 128 x 128 tiles, K split over the CUs (fewer than 96 tiles of 256 x 128)    */
};
typedef struct {
    int kernel;                 /* bd_ps_kernel                                                                                   */
    int tiles_m, tiles_n;       /* output tiles (256 x 128 or 128 x 128)                                                          */
    int ksplit, chunks_per_split;   /* K slices and (tap, 32-channel) chunks per slice (the last slice may be shorter, never empty) */
    int stages;                 /* LDS ring depth: 3 (256-row kernels), 2 or 4 (BD_PS_128; 4: split slices of at most 9 chunks)   */
    int reduce;                 /* 1: conv_ps128_reduce folds the slabs and applies the epilogue (ksplit > 1)                     */
    int grid;                   /* workgroups of the main kernel = tiles_m * tiles_n * ksplit                                     */
    int gn_splits;              /* 256-pixel tiles per image whose GroupNorm partials the epilogue can write for the descriptor's
                                   gn_groups (= bd_conv3x3_ps_gn_splits), else 0; 0 groups: not asked                             */
    size_t workspace_bytes;     /* = bd_conv3x3_ps_workspace_bytes                                                                */
    const char* prof_class;     /* the profiler class the launch is counted under                                                */
} bd_conv3x3_ps_plan_info;
int bd_conv3x3_ps_plan(const bd_conv3x3_ps_desc* d, bd_conv3x3_ps_plan_info* out);
/* weight (and bias) gradient of the same convolution, both operands as split planes:
 *   dw[Cout][3][3][Cin] = sum_p dy[p][co] x[p + tap][ci],  db[Cout] = sum_p dy[p][co] (optional, same launch).
 * Cin, Cout % 128 == 0; K (pixels) is split over workgroups with a fixed-order second pass (deterministic);
 * workspace >= bd_conv3x3_ps_wgrad_workspace_bytes().  Replaces aten::convolution_backward (weight, bias).   */
typedef struct {
    int B, H, W, Cin, Cout;
    const uint16_t* x_split; int64_t ldx;     /* conv input  [B*H*W, ldx]  */
    const uint16_t* dy_split; int64_t lddy;   /* output grad [B*H*W, lddy] */
    float* dw; float* db;
    void* workspace; size_t workspace_bytes;
    int mode;                                   /* BD_MODE_BF16X3 (or 0) / BD_MODE_BF16, as bd_conv3x3_ps_desc.mode */
} bd_conv3x3_ps_wgrad_desc;
/* Run-time tuning knob for measurement sweeps (bench.py --gpus N sweeps the weight-gradient slot count inside ONE process, because a
 * multi-GPU node is leased once): key "ps_wg3_slots" = K-split slots of conv_ps_wgrad3_kernel (0 restores BD_PS_WG3_SLOTS / the default:
 * 3/4 of the CUs, 1/2 for strip-order images).  Workspace sizes depend on it: every plan lays out again on its next call, callers must
 * re-query bd_unet_workspace_bytes.  Results are unchanged up to the fp32 summation order of the K-split. */
int bd_tune_set(const char* key, int value);
size_t bd_conv3x3_ps_wgrad_workspace_bytes(const bd_conv3x3_ps_wgrad_desc* d);
int bd_conv3x3_ps_wgrad(const bd_conv3x3_ps_wgrad_desc* d, bd_stream_t stream);
/* What bd_conv3x3_ps_wgrad and bd_upsample_conv_wgrad (below) decide for a descriptor: host code only, a copy of the one plan both
 * launchers and their *_workspace_bytes read.  The queries run their entry point's checks on the descriptor's numbers (same status, same
 * message), read no pointer, neither need nor check a workspace, and launch nothing. */
enum bd_ps_wgrad_kernel {
    BD_PS_WGRAD = 0,            /* conv_ps_wgrad_kernel: one tile per (tap, 128 ci), 9 taps                                       */
    BD_PS_WGRAD_SHARED_TAP,     /* conv_ps_wgrad3_kernel: one tile per (kx, 128 ci), the three ky share the X ring (W >= 16, pixels % 32 == 0) */
    BD_PS_WGRAD_PHASE           /* conv_ps_wgrad_kernel in its phase form: the 16 entries of E (bd_upsample_conv_wgrad)           */
};
typedef struct {
    int kernel;                 /* bd_ps_wgrad_kernel                                                                             */
    int ntaps;                  /* 9, or 16 in the phase form                                                                     */
    int tiles_m, tiles_n;       /* 128 x 128 output tiles: Cout / 128 and (3, 9 or 16) * Cin / 128                                */
    int slots;                  /* workgroup slots the K split fills (two per CU; the shared-tap form: 3/4 or 1/2 of a CU each, or
                                   the "ps_wg3_slots" knob)                                                                       */
    int ksplit, chunks_per_split;   /* K slices and 32-pixel chunks per slice (the last slice may be shorter, never empty)        */
    int reduce;                 /* 1: conv_ps_wgrad_reduce folds the slabs (ksplit > 1, and always in the phase form)             */
    int grid;                   /* workgroups of the main kernel = tiles_m * tiles_n * ksplit                                     */
    int bias_rows;              /* bias-gradient rows of Cout floats per K slice: 1, or 4 in the phase form (one per pixel class) */
    size_t slab_floats;         /* floats per K slice: ntaps * Cin * Cout + bias_rows * Cout                                      */
    size_t workspace_bytes;     /* = the entry point's *_workspace_bytes: ksplit slabs where reduce is set, and dE in the phase form */
    size_t de_offset;           /* phase form: bytes in front of dE [Cout][16][Cin] (behind the slabs), else 0                    */
    const char* prof_class;     /* the profiler class the launch is counted under                                                */
} bd_conv3x3_ps_wgrad_plan_info;
int bd_conv3x3_ps_wgrad_plan(const bd_conv3x3_ps_wgrad_desc* d, bd_conv3x3_ps_wgrad_plan_info* out);

/* out[g, n] = sum over rows m in group g of x[m, n]  (rows_per_group rows each, the last group may be shorter); bias / temb grads.
 * BD_ERR_INVALID: null pointer, rows / N / rows_per_group <= 0, ldx or ld_out < N.  BD_ERR_UNSUPPORTED: more than 65535 groups. */
int bd_colsum(const float* x, int64_t ldx, int64_t rows, int N, int64_t rows_per_group, float* out,
              int64_t ld_out, int accumulate, bd_stream_t stream);
/* dx[b, y, x, c] (+)= sum of the 2x2 block of du[b, 2y.., 2x.., c]  (nearest-upsample backward).
 * BD_ERR_INVALID: null pointer, a size <= 0, ldu or lddx < C.  BD_ERR_UNSUPPORTED: C, ldu or lddx not a multiple of 4, or a pointer
 * that is not 16-byte aligned. */
int bd_sum2x2(const float* du, int64_t ldu, float* dx, int64_t lddx, int B, int H, int W, int C,
              int accumulate, bd_stream_t stream);
/* dst[m, c] (+)= scale * src[m, c] over [rows, C] views with leading dimensions lds / ldd (the residual-path gradient add of the
 * UNet plan).  BD_ERR_INVALID: null pointer, rows or C <= 0, lds or ldd < C.  BD_ERR_UNSUPPORTED: C, lds or ldd not a multiple of
 * 4, or a pointer that is not 16-byte aligned. */
int bd_add(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int C, float scale,
           int accumulate, bd_stream_t stream);

/* Row softmax over [rows, n] (attention.py:161) and its backward dS = P * (dP - sum(dP*P)). */
int bd_softmax_fwd(const float* s, float* p, int64_t rows, int n, bd_stream_t stream);
int bd_softmax_bwd(const float* p, const float* dp, float* ds, int64_t rows, int n, bd_stream_t stream);

/* y = x * sigmoid(x) ; dx = dy * silu'(x)  (embeddings.py:205-206, resnet.py:576) */
int bd_silu_fwd(const float* x, float* y, int64_t n, bd_stream_t stream);
int bd_silu_bwd(const float* x, const float* dy, float* dx, int64_t n, int accumulate, bd_stream_t stream);

/* a-3: loss = mean((pred - target)^2) and dpred = 2 (pred - target) / n  (loss.py:301).
 * loss_type: 0 l2, 1 l1, 2 huber(beta=1).  loss is a device scalar, written (not accumulated).
 * grad_scale multiplies dpred (1/world for DP mean).  workspace >= bd_reduce_workspace_bytes().
 * ldp < C, ldt < C or (with dpred) lddp < C is BD_ERR_INVALID, here and in bd_loss_groups_fwd_bwd.   */
size_t bd_reduce_workspace_bytes(void);
int bd_loss_fwd_bwd(const float* pred, int64_t ldp, const float* target, int64_t ldt, int64_t rows, int C,
                    int loss_type, float grad_scale, float* loss, float* dpred, int64_t lddp,
                    void* workspace, bd_stream_t stream);

/* The same loss over n_groups consecutive groups of rows, each with its own mean and weight (the clean-data and shift terms of
 * baddiffusion_amd/defense.py remove_backdoor, DESIGN.md section 3, "Grouped loss").  With n_g = group_rows[g] * C and S_g the fp64 sum
 * of group g's per-element fp32 losses (fixed order, no atomics: two calls give the same bits):
 *   losses[g] = (float)(S_g / n_g),  losses[n_groups] = (float)(sum_g (double)group_weight[g] * S_g / n_g)   (device float[n_groups + 1],
 *   written), dpred[m][c] = ((g' / (float)n_g) * grad_scale) * group_weight[g] in fp32 (may be null; columns >= C of a row are not touched).
 * Every group is reduced with the block / stride pattern bd_loss_fwd_bwd uses for a whole array, so one group of weight 1 gives
 * losses[0], losses[1] and dpred bit-identical to it.  group_rows[g] > 0 and sum to rows; group_weight[g] finite and >= 0 (host
 * values, checked before any launch).  workspace >= bd_loss_groups_workspace_bytes(n_groups) (0 for n_groups out of range). */
#define BD_LOSS_MAX_GROUPS 4
typedef struct {
    int n_groups;                                   /* 1 .. BD_LOSS_MAX_GROUPS */
    int64_t group_rows[BD_LOSS_MAX_GROUPS];
    float group_weight[BD_LOSS_MAX_GROUPS];
} bd_loss_groups_desc;
size_t bd_loss_groups_workspace_bytes(int n_groups);
int bd_loss_groups_fwd_bwd(const float* pred, int64_t ldp, const float* target, int64_t ldt, int64_t rows, int C,
                           int loss_type, float grad_scale, const bd_loss_groups_desc* groups, float* losses,
                           float* dpred, int64_t lddp, void* workspace, size_t workspace_bytes, bd_stream_t stream);

/* f-3: mean structural similarity of two [N,C,H,W] image batches in [0, data_range] given by element strides (NCHW or
 * NHWC storage alike): StructuralSimilarityIndexMeasure(data_range=1.0) of baddiffusion.py:536-547 with the torchmetrics
 * defaults (11x11 Gaussian, sigma 1.5, k1 0.01, k2 0.03, reflect padding, cropped border, mean over C,H,W then batch).
 * out: device float scalar, written.  workspace >= bd_ssim_workspace_bytes(N, C, H, W).  Needs H, W > 10, N*C <= 65535. */
size_t bd_ssim_workspace_bytes(int N, int C, int H, int W);
int bd_ssim(const float* preds, const float* target, int N, int C, int H, int W, int64_t stride_n, int64_t stride_c,
            int64_t stride_h, int64_t stride_w, float data_range, float* out, void* workspace, size_t workspace_bytes,
            bd_stream_t stream);

/* Backdoor detection statistics of a batch of generated images (baddiffusion_amd/defense.py, DESIGN.md section 3, "Detection statistics").
 *
 * bd_pairwise_sqdist: d2[i][j] = sum_k (x[i][k] - x[j][k])^2 for the N rows of x (fp32 [N, D], row stride ldx >= D floats;
 * any 4-byte aligned x and any ldx, 16-byte aligned rows take vector loads).  The difference is taken in fp32 BEFORE it is
 * squared: no Gram identity |a|^2 + |b|^2 - 2ab (which cancels on the close pairs a collapsed batch consists of) and no
 * pre-centring.  Every unordered pair is computed once and the same value is stored at d2[i][j] and d2[j][i]; the diagonal is
 * written as 0.0f; all N * N entries of d2 (fp32, row stride ldd >= N) are written, columns >= N of a row are not touched.
 * When the 64 x 64 tiles of pairs alone do not fill the chip, D is split over workgroups into workspace partials that a
 * second launch adds in split order (no atomics): the result is bit-identical from call to call.
 * workspace >= bd_pairwise_sqdist_workspace_bytes(N, D) (0 when D is not split: workspace may then be NULL).
 *
 * bd_total_variation: tv[n] = sum_c ( sum_{h<H-1,w} |x[h+1][w] - x[h][w]| + sum_{h,w<W-1} |x[h][w+1] - x[h][w]| ) of an
 * [N,C,H,W] batch given by element strides as in bd_ssim; differences in fp32, accumulated in fp64 in a fixed order that
 * depends on the logical index only (NCHW and NHWC storage give the same bits).  tv: fp32 [N], written.  H = 1 / W = 1 are
 * valid (that direction contributes 0).  Needs C*H*W < 2^31. */
size_t bd_pairwise_sqdist_workspace_bytes(int N, int D);
int bd_pairwise_sqdist(const float* x, int64_t ldx, int N, int D, float* d2, int64_t ldd, void* workspace,
                       size_t workspace_bytes, bd_stream_t stream);
int bd_total_variation(const float* x, int N, int C, int H, int W, int64_t stride_n, int64_t stride_c, int64_t stride_h,
                       int64_t stride_w, float* tv, bd_stream_t stream);

/* Sample-quality metrics on feature rows (metrics.knn_sqradius / prdc / precision_recall / kid; DESIGN.md section 3, "Quality
 * metrics on features"): pairwise work between the rows of a (fp32 [Na, D], row stride lda >= D floats) and of b ([Nb, D], ldb)
 * reduced per row of a, without ever storing the Na x Nb matrix.  Any 4-byte aligned base and any row stride are accepted; when both
 * bases are 16-byte aligned and both strides are multiples of 4 the rows are read with vector loads.  FINITE INPUTS ARE THE CALLER'S
 * DUTY: a NaN or an infinity in a row makes that row's (and its partners') results unspecified; nothing checks for them.
 *
 * d2(a_i, b_j) = sum_k (a[i][k] - b[j][k])^2 with the arithmetic of bd_pairwise_sqdist: the difference in fp32 BEFORE the square,
 * never the Gram identity; the sums over even and over odd k are kept apart and added at the end.  dot(a_i, b_j) is the fp32 FMA
 * chain in the same k order.  One device function produces the value of a pair, so it has the same bits in every entry point below,
 * with a and b exchanged, alone or inside any larger call, and from call to call.
 *
 * A workgroup owns 64 rows of a and walks 64-column tiles of b; D is never split.  When there are few strips of 64 rows the column
 * tiles are cut into csplit contiguous ranges whose per-row partial results go to the workspace [csplit][Na][...] and are folded in
 * split order by a second launch (no atomics).  bd_cross_plan reports the cut: strips = ceil(Na / 64), col_tiles = ceil(Nb / 64),
 * csplit_cap = max(1, min(8 * CUs / strips, col_tiles)), tiles_per_split = ceil(col_tiles / csplit_cap), csplit = ceil(col_tiles /
 * tiles_per_split).  Each *_workspace_bytes is csplit_cap * Na * (bytes per row) when csplit_cap > 1 and 0 otherwise (workspace may
 * then be NULL); it is 0 for arguments the entry point rejects; for a fixed Na it does not decrease with Nb or with k.
 *
 * bd_knn_sqradius: out[i] = the k-th smallest of { d2(x_i, x_j) : j != i }, 1 <= k <= 16 and k <= N - 1 (else BD_ERR_INVALID).
 *   Self is left out by index, not by value: a duplicate row gives 0.  The k-th smallest of a multiset depends neither on the order
 *   in which its members arrive nor on csplit.  Bytes per row: 4 k.
 * bd_cross_ksmallest: out[i][0 .. k-1] (fp32 [Na, k], ascending) = the k smallest of { d2(a_i, b_j) : j != i + self_col0 }, +inf
 *   where fewer than k columns exist.  self_col0 = 0 with a == b is the neighbour list behind bd_knn_sqradius; rows a = x + r * ldx
 *   with self_col0 = r score a slice of the rows of x; self_col0 = -Na excludes nothing.  1 <= k <= 16.  Bytes per row: 4 k.
 * bd_cross_count_min: count[i] = #{ j : d2(a_i, b_j) <= radius2[j] } (int32) and min_d2[i] = min_j d2(a_i, b_j).  No pair is left
 *   out.  radius2 == NULL: no count is taken and count may be NULL.  Integer sums and minima are order-independent: the bits depend
 *   neither on csplit nor on Na.  Bytes per row: 8.
 * bd_poly3_rowsum: rowsum[i] = sum_j (double(dot(a_i, b_j)) / D + 1)^3 in fp64, the cubic polynomial kernel of KID; exclude_diag
 *   != 0 leaves out j == i (a and b the same set).  Columns are added in order within a quarter tile, the four quarters, the tiles and
 *   the splits in order: bit-identical from call to call for one (Na, Nb) on one device; not across different csplit.  rowsum and
 *   the workspace must be 8-byte aligned.  Bytes per row: 8.
 * Status: BD_ERR_INVALID for a null pointer, Na / Nb / D < 1, a row stride < D, a base that is not 4-byte aligned, k out of range;
 * BD_ERR_UNSUPPORTED for Na > 65535 * 64; BD_ERR_WORKSPACE.  Every check runs on the host before any launch and its message names
 * the entry point. */
typedef struct {
    int strips, col_tiles, csplit, tiles_per_split, csplit_cap;
} bd_cross_plan_info;
int bd_cross_plan(int Na, int Nb, int D, bd_cross_plan_info* out);
size_t bd_knn_sqradius_workspace_bytes(int N, int D, int k);
int bd_knn_sqradius(const float* x, int64_t ldx, int N, int D, int k, float* out, void* workspace, size_t workspace_bytes,
                    bd_stream_t stream);
size_t bd_cross_ksmallest_workspace_bytes(int Na, int Nb, int D, int k);
int bd_cross_ksmallest(const float* a, int64_t lda, int Na, const float* b, int64_t ldb, int Nb, int D, int k, int64_t self_col0,
                       float* out, void* workspace, size_t workspace_bytes, bd_stream_t stream);
size_t bd_cross_count_min_workspace_bytes(int Na, int Nb, int D);
int bd_cross_count_min(const float* a, int64_t lda, int Na, const float* b, int64_t ldb, int Nb, int D, const float* radius2,
                       int32_t* count, float* min_d2, void* workspace, size_t workspace_bytes, bd_stream_t stream);
size_t bd_poly3_rowsum_workspace_bytes(int Na, int Nb, int D);
int bd_poly3_rowsum(const float* a, int64_t lda, int Na, const float* b, int64_t ldb, int Nb, int D, int exclude_diag, double* rowsum,
                    void* workspace, size_t workspace_bytes, bd_stream_t stream);

/* Per-image scores of a batch against a target that may be broadcast (metrics.mse_per_image / ssim_per_image /
 * attack_success_rate, the loss split of TrainEngine; DESIGN.md section 3, "Per-image scores").  Both images are [N,C,H,W] given by
 * element strides (all >= 0); any of the target's strides may be 0 (one target shared by all images and / or channels).
 *
 * bd_image_loss: out[n] = (float)(S_n / (C*H*W)), S_n the fp64 sum of image n's per-element fp32 losses at d = p - t (taken in
 * fp32); loss_type and the element functions are those of bd_loss_fwd_bwd (0 l2, 1 l1, 2 huber with beta 1).
 * bd_ssim_images: out[n] = the mean over the C channels and the cropped (H-10) x (W-10) map of image n; window, constants, reflect
 * padding, crop and the tile routine are those of bd_ssim.  Needs H, W > 10; any N (the launcher walks the N*C planes in chunks).
 *
 * Summation order.  bd_image_loss cuts the C*H*W logical elements (c, h, w; w fastest) of an image into chunks of 8192, one
 * workgroup each: thread t adds elements t, t + 256, ... of its chunk in fp64 and the 256 sums go through a fixed tree.
 * An image of one chunk (C*H*W <= 8192) is finished by that workgroup; otherwise the chunk sums, in chunk order, are folded by
 * one workgroup of a second launch, thread-strided and through the same tree.  bd_ssim_images gives one workgroup each 32 x 32
 * tile of one channel's map, summed as in bd_ssim, and always folds the image's tile sums, in (c, tile row, tile column) order,
 * in that second launch.  No atomics.  The order is therefore a function of
 * (C, H, W) and the logical index alone -- not of the strides, of N, of the image's place in the batch, of the CU count or of
 * where the launcher cuts the batch -- so out[n] is bit-identical
 *   - in NCHW and in channels-last / permuted-NHWC storage,
 *   - with a stride-0 target and with the same target materialised,
 *   - for an image alone and inside any batch,
 *   - from call to call.
 * out: fp32 [N], written.  workspace >= the *_workspace_bytes of the same (N, C, H, W) (0 for non-positive arguments; it may be 0
 * for a valid shape, workspace may then be NULL).  Status: BD_ERR_INVALID for null d / preds / target / out, N, C, H, W <= 0,
 * H or W <= 10 (SSIM), a negative stride, an unknown loss_type; BD_ERR_UNSUPPORTED for C*H*W >= 2^31; BD_ERR_WORKSPACE. */
typedef struct {
    int N, C, H, W;
    const float* preds;  int64_t p_stride[4];   /* element strides n, c, h, w */
    const float* target; int64_t t_stride[4];   /* any of them may be 0: a target shared by all images (and/or channels) */
} bd_image_pair_desc;
size_t bd_image_loss_workspace_bytes(int N, int C, int H, int W);
int bd_image_loss(const bd_image_pair_desc* d, int loss_type, float* out, void* workspace, size_t workspace_bytes,
                  bd_stream_t stream);
size_t bd_ssim_images_workspace_bytes(int N, int C, int H, int W);
int bd_ssim_images(const bd_image_pair_desc* d, float data_range, float* out, void* workspace, size_t workspace_bytes,
                   bd_stream_t stream);

/* Terms of the variational bound of a DDPM in bits per dimension (likelihood.bits_per_dim; DESIGN.md section 3, "Bits per
 * dimension"): epsilon prediction, fixed variances.  Row n of the batch carries its own t[n] in [0, T], T = the number of training
 * timesteps; x0, x_t and eps are fp32 [N,C,H,W] by element strides (all >= 0), as in bd_image_pair_desc.  With
 *     x0_hat = (x_t - sqrt(1 - ac[t]) eps) / sqrt(ac[t])   in fp32, the expression of bd_ddpm_step,
 *              clamped to [-1, 1] when clip_denoised (by comparison: a NaN stays a NaN),
 *     m      = the mean over (c, h, w) of the row's element term e_i,
 *     bits[n] = (float)((term_add[t] + term_mul[t] * m) / ln 2)     in fp64,
 * the element term is
 *     1 <= t < T   e_i = (x0_i - x0_hat_i)^2 in fp32 (the KL of two Gaussians whose means differ by c0_t (x0 - x0_hat)):
 *                  term_add[t] = (-1 + D_t + exp(-D_t)) / 2, D_t = log(model variance / posterior variance); term_mul[t] = c0_t^2 /
 *                  (2 model variance);
 *     t = 0        e_i = -log max(P_i, 1e-12) in fp64, P_i the mass the Gaussian N(x0_hat_i, sigma_dec^2) puts on the bin of x0_i
 *                  (half width 1/255; open to -inf for x0_i < -0.999 and to +inf for x0_i > 0.999), with z+- = (x0_i - x0_hat_i +-
 *                  1/255) * inv_sigma_dec taken on the tail side: P_i = (erfc(z- / sqrt 2) - erfc(z+ / sqrt 2)) / 2 for z- > 0, else
 *                  (erfc(-z+ / sqrt 2) - erfc(-z- / sqrt 2)) / 2; erfc(-z+ / sqrt 2) / 2 and erfc(z- / sqrt 2) / 2 in the two edge
 *                  bins.  The exact normal CDF, not the tanh approximation of improved-DDPM.  term_add[0] = 0, term_mul[0] = 1;
 *     t = T        e_i = x0_i^2 in fp32 (the prior term KL(q(x_T | x0) || N(0, I))); x_t and eps are not read and may be NULL when
 *                  every row is a prior row.  term_add[T] = (-1 - log(1 - ac[T-1]) + (1 - ac[T-1])) / 2, term_mul[T] = ac[T-1] / 2.
 * The tables term_add, term_mul (fp32 [T + 1], device) and inv_sigma_dec are the caller's (likelihood.vb_tables computes them in fp64 on
 * the host); the kernel does no schedule arithmetic beyond x0_hat.  alphas_cumprod: fp32 [T], device.
 * t: int64 [N] on the device; t_host: the same values on the host, which the launcher checks before anything is launched.
 * x0_mse: optional fp32 [N], the row's mean of (x0 - x0_hat)^2 (of x0^2 in a prior row).
 *
 * Summation order: that of bd_image_loss (chunks of 8192 logical elements, thread-strided fp64 sums, the fixed tree, the chunk sums
 * folded by one workgroup per image of a second launch), so bits[n] and x0_mse[n] do not depend on N, on the row's place in the batch,
 * on the strides or on the other rows' t.  A workgroup belongs to one row, so only t = 0 rows evaluate erfc.  A NaN in a row's inputs
 * makes that row's outputs NaN and no other's.
 * workspace >= bd_vb_terms_workspace_bytes(N, C, H, W) (0 for C*H*W <= 8192; workspace may then be NULL).  Status: BD_ERR_INVALID for
 * a null d / x0 / t / t_host / alphas_cumprod / table / bits, x_t or eps NULL with a row at t < T, N, C, H, W, T <= 0, t outside
 * [0, T], a negative stride, inv_sigma_dec not positive and finite; BD_ERR_UNSUPPORTED for C*H*W >= 2^31; BD_ERR_WORKSPACE. */
typedef struct {
    int N, C, H, W;
    const float* x0;  int64_t x0_stride[4];    /* element strides n, c, h, w */
    const float* x_t; int64_t xt_stride[4];
    const float* eps; int64_t eps_stride[4];
    const int64_t* t;                          /* device [N] */
    const int64_t* t_host;                     /* host   [N], the same values */
    const float* alphas_cumprod; int T;
    const float* term_add; const float* term_mul; float inv_sigma_dec;
    int clip_denoised;
    float* bits; float* x0_mse;
} bd_vb_terms_desc;
size_t bd_vb_terms_workspace_bytes(int N, int C, int H, int W);
int bd_vb_terms(const bd_vb_terms_desc* d, void* workspace, size_t workspace_bytes, bd_stream_t stream);

/* The same terms along the BACKDOORED chain of BadDiffusion ("The bound along the backdoored chain"), whose x_t is
 * shifted by rho_t r, rho_t = 1 - sqrt(ac[t]): the posterior mean of q'(x_{t-1} | x_t, x0) is c0_t x0 + ct_t x_t + d_t r, the model's
 * reverse step is the unchanged one, and the two means differ by c0_t (x0 + g_t r - x0_hat), g_t = d_t / c0_t.  Everything is as in
 * bd_vb_terms -- x0_hat, m, bits[n], the tables term_add / term_mul, the launches, the summation order and the fold -- but for a fourth
 * stream r (fp32 [N,C,H,W] by element strides >= 0; 0 over n broadcasts one image), the table term_shift (fp32 [T + 1], device: g, with
 * term_shift[0] = 0 and term_shift[T] = -1 by convention; likelihood.vb_tables(shift=True)) and the element terms, in fp32 and in exactly
 * this order of operations (no contraction):
 *     1 <= t < T   s = x0_i + term_shift[t] * r_i;   df = s - x0_hat_i;   e_i = df * df
 *     t = 0        the decoder term of bd_vb_terms: r and term_shift are not read
 *     t = T        df = x0_i - r_i;   e_i = df * df      (KL(q'(x_T | x0) || N(r, I)): sampling with the trigger starts from noise + r);
 *                  term_shift[T] is not read, x_t and eps are not read and may be NULL when every row is a prior row.
 * x0_mse: optional fp32 [N], the row's mean of that squared term ((x0 - x0_hat)^2 in a t = 0 row).
 * With r all zeros every row equals bd_vb_terms's bit for bit; a t = 0 row does so for any r.  A NaN in a row's r makes that row's outputs
 * NaN (t = 0 rows excepted) and no other's.  workspace: bd_vb_terms_workspace_bytes.  Status: what bd_vb_terms returns, and
 * BD_ERR_INVALID for a null r / term_shift or a negative r stride. */
typedef struct {
    int N, C, H, W;
    const float* x0;  int64_t x0_stride[4];    /* element strides n, c, h, w */
    const float* x_t; int64_t xt_stride[4];
    const float* eps; int64_t eps_stride[4];
    const int64_t* t;                          /* device [N] */
    const int64_t* t_host;                     /* host   [N], the same values */
    const float* alphas_cumprod; int T;
    const float* term_add; const float* term_mul; float inv_sigma_dec;
    int clip_denoised;
    float* bits; float* x0_mse;
    const float* r; int64_t r_stride[4];       /* the shift image(s); r_stride[0] = 0: one image for every row */
    const float* term_shift;                   /* device [T + 1]: g */
} bd_vb_terms_shift_desc;
int bd_vb_terms_shift(const bd_vb_terms_shift_desc* d, void* workspace, size_t workspace_bytes, bd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * FID feature extractor (measure path, SURVEY f-3): the layer kernels of pytorch_fid's InceptionV3 up to pool3
 * (/root/reference/fid_score.py:53 `from pytorch_fid.inception import InceptionV3`, :91-148 get_activations, :255
 * `InceptionV3([block_idx])`; pytorch-fid==0.2.1 per requirements.txt -- a third-party package absent from the reference tree,
 * its published graph is restated in baddiffusion_amd/inception.py).  NHWC fp32, exact fp32 products (v_mfma_f32_32x32x2_f32).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    const float* x; int64_t ldx;      /* input  [B, H, W, Cin], pixel stride ldx floats (a channel slice of a wider buffer is fine) */
    const float* w;                   /* weights [KH][KW][Cin][Cout] (BatchNorm scale folded in by the caller)                     */
    const float* bias;                /* optional [Cout] (folded BatchNorm shift)                                                  */
    float* y; int64_t ldy;            /* output [B, Ho, Wo, Cout] at pixel stride ldy: Ho = (H + 2 pad_h - KH) / stride_h + 1, ...  */
    int B, H, W, Cin, Cout, KH, KW, stride_h, stride_w, pad_h, pad_w;
    int relu;                         /* y = max(y, 0)  (BasicConv2d = conv + bn + relu)                                           */
    int w_kc;                         /* round 5: 1 = weights are [KH][KW][Cout][Cin] (K contiguous): the double-buffered 128 x 64 tile kernel
                                         with vector LDS reads; 0 = [KH][KW][Cin][Cout], the 64 x 64 kernel.  Same results up to the fp32
                                         summation order inside a 16-channel chunk.                                                   */
} bd_conv2d_desc;
/* Cout % 4 == 0; x 16-byte aligned with ldx % 4 == 0 when Cin % 4 == 0 (any alignment for the 3-channel stem). */
int bd_conv2d_nhwc(const bd_conv2d_desc* d, bd_stream_t stream);
/* F.max_pool2d (mode 0, padding = -inf) / F.avg_pool2d (mode 1, count_include_pad as given) with a square window, C % 4 == 0. */
int bd_pool2d_nhwc(const float* x, int64_t ldx, float* y, int64_t ldy, int B, int H, int W, int C, int kernel, int stride, int pad,
                   int mode, int count_include_pad, bd_stream_t stream);
/* y = scale * F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False) + shift; x is [B, H, W, C] uint8 (read as
 * value / 255, i.e. after ToTensor) when x_is_u8, else float32. */
int bd_resize_bilinear_nhwc(const void* x, int x_is_u8, float* y, int B, int H, int W, int C, int Ho, int Wo, float scale, float shift,
                            bd_stream_t stream);
/* AdaptiveAvgPool2d((1, 1)): y[b, c] = mean over the HW pixels of x [B, HW, C] (pixel stride ldx), fixed summation order. */
int bd_global_avgpool_nhwc(const float* x, int64_t ldx, float* y, int B, int HW, int C, bd_stream_t stream);


/* a-8: global-norm clip + Adam over one flat fp32 buffer (baddiffusion.py:320, 611-615).
 * bd_sumsq: sumsq (device double scalar) = sum g^2.  bd_adam_clip reads it:
 *   coef = min(1, max_norm / (sqrt(sumsq) + 1e-6));  g *= coef;  Adam(b1,b2,eps), bias correction from
 *   `step` (1-based, host scalar) ; lr host scalar.  grad_norm_out (device float, optional) = sqrt(sumsq). */
int bd_sumsq(const float* g, int64_t n, double* sumsq, void* workspace, bd_stream_t stream);
int bd_adam_clip(float* p, const float* g, float* m, float* v, int64_t n, const double* sumsq,
                 double max_norm, double lr, double b1, double b2, double eps, int step, float* grad_norm_out,
                 bd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * a-4: the whole UNet2DModel (models/unet_2d.py:82-326) as a static plan: forward (inference or
 * training, saving what backward needs in the caller's workspace) and backward (writes the flat
 * gradient buffer; every parameter gets exactly one contribution, so no zeroing is needed).
 * Parameters live in ONE flat fp32 buffer; bd_unet_param_* describe where each state_dict key is.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int sample_size, in_channels, out_channels;
    int num_blocks;                 /* <= 8                                                     */
    int block_out_channels[8];
    int down_attn[8];               /* 1 = AttnDownBlock2D, 0 = DownBlock2D                     */
    int up_attn[8];                 /* 1 = AttnUpBlock2D,   0 = UpBlock2D                       */
    int layers_per_block;
    int downsample_padding;         /* 0 => asymmetric (0,1,0,1) pad, 1 => symmetric            */
    int flip_sin_to_cos; float freq_shift;
    float norm_eps; int norm_num_groups;
    int attention_head_dim;         /* 0 => single head                                         */
    float mid_block_scale_factor;
    int compute_mode;               /* bd_compute_mode of every conv / GEMM of the network      */
} bd_unet_config;

typedef struct bd_unet bd_unet;     /* host-only plan object (no device memory)                  */
int bd_unet_create(const bd_unet_config* cfg, bd_unet** out);
void bd_unet_destroy(bd_unet* u);
int bd_unet_set_compute_mode(bd_unet* u, int mode);   /* bd_compute_mode; may be changed between calls */
int64_t bd_unet_num_params(const bd_unet* u);
int bd_unet_num_tensors(const bd_unet* u);
/* i-th parameter tensor: state_dict key, offset (elements) in the flat buffer, logical shape
 * (rank <= 4, OIHW for convs) and layout: 0 = as-is (contiguous logical shape),
 * 1 = conv weight stored [O][kh][kw][I]. */
int bd_unet_param_info(const bd_unet* u, int i, const char** name, int64_t* offset, int* rank,
                       int64_t shape[4], int* layout);
/* workspace bytes for batch B; training != 0 keeps every tensor backward needs */
size_t bd_unet_workspace_bytes(bd_unet* u, int B, int training);
/* x: NHWC [B*S*S, ldx] ; t: int64 [B] (t_stride 0 => broadcast t[0]) ; out NHWC [B*S*S, ldo] */
int bd_unet_forward(bd_unet* u, int B, int training, const float* params, const float* x, int64_t ldx,
                    const int64_t* t, int t_stride, float* out, int64_t ldo,
                    void* workspace, size_t workspace_bytes, bd_stream_t stream);
/* bd_unet_forward with fp32 timesteps, which may be fractional (bd_timestep_embedding_f32); nothing else differs, and every
 * backward entry point works unchanged after it (the time-embedding backward reads the saved sinusoid buffer).  An integral fp32
 * timestep gives the bits of the int64 one. */
int bd_unet_forward_tf(bd_unet* u, int B, int training, const float* params, const float* x, int64_t ldx,
                       const float* t, int t_stride, float* out, int64_t ldo,
                       void* workspace, size_t workspace_bytes, bd_stream_t stream);
/* after a training forward with the same workspace and the same x: dout NHWC -> grads (flat, same offsets) */
int bd_unet_backward(bd_unet* u, int B, const float* params, const float* x, int64_t ldx,
                     const float* dout, int64_t lddo, float* grads, void* workspace, size_t workspace_bytes,
                     bd_stream_t stream);
/* bd_unet_backward that also writes the gradient with respect to the network input x: dx [B, S, S, in_channels] NHWC with row
 * stride lddx >= in_channels (every element written, never accumulated).
 *   grads != NULL: the ordinary backward plus dx; grads is bit-identical to bd_unet_backward's for the same inputs.
 *   grads == NULL: the DATA-GRADIENT-ONLY schedule (frozen weights: trigger inversion, adversarial probes, guidance).  No weight, bias
 *                  or GroupNorm-parameter gradient is computed or written, nothing is put on the plan's side stream, and the
 *                  time-embedding backward (the timestep is not differentiable: that branch feeds weights only) is skipped.
 * dx is bit-identical between the two schedules (same kernels in the same order on the caller's stream).  Same workspace contract as
 * bd_unet_backward: bd_unet_workspace_bytes(u, B, 1), after a training forward with that workspace and the same x. */
int bd_unet_backward_input(bd_unet* u, int B, const float* params, const float* x, int64_t ldx,
                           const float* dout, int64_t lddo, float* grads, float* dx, int64_t lddx,
                           void* workspace, size_t workspace_bytes, bd_stream_t stream);
/* backward split in `bd_unet_num_segments` contiguous-in-time segments so the caller can overlap a
 * gradient all-reduce with the rest of backward: after segment s, grads in
 * [seg_lo[s], seg_hi[s]) (elements) are final. */
/* Backward runs the weight-gradient GEMMs on a second, low-priority stream owned by the plan (forked from / joined to
 * `stream` with events, once per node -- still hipGraph-capturable and free of host synchronisation).  0 disables it. */
int bd_unet_set_aux_stream(bd_unet* u, int enabled);
/* Sampling loops (pipeline_ddpm.py:106-111, pipeline_ddim.py:114-121) evaluate the network 50-1000 times over the same parameters.
 * While enabled, an inference forward whose (params pointer, workspace pointer, B) equal those of the previous inference forward
 * skips the per-forward weight preprocessing (split-plane copy of the flat buffer, pre-summed upsample tap planes).  The caller
 * promises not to modify the parameters in between; switching it on or off re-reads them once.  Training forwards never skip. */
int bd_unet_set_static_weights(bd_unet* u, int enabled);
/* Forget the prepared planes without leaving the block: call after an in-place parameter change (load_state_dict, an optimizer step on
 * the same buffer) or when the workspace was freed and may be re-allocated at the same address.  bd_unet_set_compute_mode and every
 * re-layout (another batch size / training flag) do the same internally. */
int bd_unet_reset_static_cache(bd_unet* u);
int bd_unet_num_segments(const bd_unet* u);
int bd_unet_segment_range(const bd_unet* u, int seg, int64_t* lo, int64_t* hi);   /* host-only query: the main range */
/* a segment finalises 1 or 3 ranges of the flat gradient: k = 0 its own parameters, k = 1 / 2 its resnets' rows of the
 * batched time_emb_proj weight / bias (stored with the time embedding, computed in the resnets' backward) */
int bd_unet_segment_num_ranges(const bd_unet* u, int seg);
int bd_unet_segment_range_k(const bd_unet* u, int seg, int k, int64_t* lo, int64_t* hi);
/* Deferred join (data-parallel training).  By default every bd_unet_backward_segment call ends with the caller's stream ordered
 * after the weight gradients it put on the plan's side stream.  With bd_unet_set_deferred_join(u, 1) only the LAST segment joins:
 * a segment's weight gradients keep running beside the next segment's data-gradient chain, and whoever consumes the segment's
 * gradient ranges (the all-reduce) is ordered behind them explicitly: bd_unet_stream_wait_aux(u, s) makes stream `s` wait for
 * everything the segment calls made so far have put on the side stream (no host synchronisation; a no-op before the first
 * backward or with the side stream disabled). */
int bd_unet_set_deferred_join(bd_unet* u, int enabled);
int bd_unet_stream_wait_aux(bd_unet* u, bd_stream_t stream);
int bd_unet_backward_segment(bd_unet* u, int seg, int B, const float* params, const float* x, int64_t ldx,
                             const float* dout, int64_t lddo, float* grads, void* workspace, size_t workspace_bytes,
                             bd_stream_t stream, int64_t* ready_lo, int64_t* ready_hi);

/* ------------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py `roofline`): when enabled, every igemm launch is bracketed by a
 * hipEvent pair on its own stream; totals are kept per kernel class ("igemm_<tile>_<A>_<B>").
 * flops = 2*M*N*K algorithmic ; bytes = unique operand + output bytes (algorithmic, fp32).
 * ------------------------------------------------------------------------------------------------ */
int bd_prof_enable(int on);
int bd_prof_enabled(void);   /* 1 while launches are being bracketed by events (such launches cannot be graph-captured) */
int bd_prof_reset(void);
int bd_prof_num_classes(void);
int bd_prof_get(int cls, const char** name, int64_t* launches, double* total_ms, double* flops, double* bytes);

/* ------------------------------------------------------------------------------------------------
 * Phase-decomposed convolutions on split planes (round 3, csrc/conv_ph.hip).
 * Upsample2D (resnet.py:126-161) is y = conv3x3(nearest_up2(x)): every output pixel's 3x3 window covers only 2x2 distinct
 * source pixels, so with the tap sums E[oy][ox] (bd_upsample_weights) the forward is four 2x2-tap convolutions on the SOURCE
 * grid (one per output pixel class), the data gradient ONE 16-tap convolution sampling dY at stride 2, and the weight gradient
 * 16 tap products folded back to the nine taps: 16 instead of 36 tap products per source pixel, same result up to the fp32
 * rounding of the weight sums.  The data gradient of a stride-2 convolution (Downsample2D, resnet.py:199-208) is the same
 * construction with 4 / 2 / 2 / 1 taps per input-pixel parity class (bd_conv3x3_s2_dgrad_ps).
 * All operands are split planes (see above): H, W powers of two, Cin, Cout multiples of 128.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int B, H, W, Cin, Cout;                     /* H x W = SOURCE grid; the convolution runs on 2H x 2W            */
    const uint16_t* x_split; int64_t ldx;       /* source activations [B*H*W, Cin]                 (fwd, wgrad)    */
    const uint16_t* dy_split; int64_t lddy;     /* output gradient on the fine grid [B*4HW, Cout]  (dgrad, wgrad)  */
    const uint16_t* e_split;                    /* bd_upsample_weights: E   [Cout][16][Cin]        (fwd)           */
    const uint16_t* et_split;                   /* bd_upsample_weights: E^T [Cin][16][Cout]        (dgrad)         */
    const float* bias;                          /* fwd, optional [Cout]                                            */
    float* y; int64_t ldy;                      /* fwd out [B*4HW, Cout]                                           */
    float* dx; int64_t lddx; int accumulate;    /* dgrad out [B*HW, Cin], += when accumulate                       */
    float* dw; float* db;                       /* wgrad out [Cout,3,3,Cin] and (optional) [Cout]                  */
    void* workspace; size_t workspace_bytes;    /* wgrad / dgrad: bd_upsample_conv_{wgrad,dgrad}_workspace_bytes   */
    int mode;                                   /* BD_MODE_BF16X3 (or 0) / BD_MODE_BF16, as bd_conv3x3_ps_desc.mode */
} bd_upsample_conv_desc;
int bd_upsample_weights(const float* w /* [Cout,3,3,Cin] */, int Cin, int Cout, uint16_t* e_split, uint16_t* et_split /* may be null: forward only */,
                        bd_stream_t stream);
int bd_upsample_conv_fwd(const bd_upsample_conv_desc* d, bd_stream_t stream);
int bd_upsample_conv_dgrad(const bd_upsample_conv_desc* d, bd_stream_t stream);
int bd_upsample_conv_wgrad(const bd_upsample_conv_desc* d, bd_stream_t stream);
size_t bd_upsample_conv_wgrad_workspace_bytes(const bd_upsample_conv_desc* d);
size_t bd_upsample_conv_dgrad_workspace_bytes(const bd_upsample_conv_desc* d);   /* 0 unless the grid is small (taps dealt to 4 workgroups per tile) */
/* host-only queries: the plan of bd_upsample_conv_wgrad (bd_conv3x3_ps_wgrad_plan_info above), and the workgroups per tile of
 * bd_upsample_conv_dgrad: 4 (the 16 taps dealt to four groups + a fixed-order fold, while the tiles fill at most half the chip) or 1 --
 * what bd_upsample_conv_dgrad_workspace_bytes follows; 0 for a null descriptor */
int bd_upsample_conv_wgrad_plan(const bd_upsample_conv_desc* d, bd_conv3x3_ps_wgrad_plan_info* out);
int bd_upsample_conv_dgrad_tap_groups(const bd_upsample_conv_desc* d);

typedef struct {
    int B, Ho, Wo, Cin, Cout, pad;              /* stride-2 conv: input grid 2Ho x 2Wo; pad 0 = F.pad(0,1,0,1) + padding 0, 1 = padding 1 */
    const uint16_t* dy_split; int64_t lddy;     /* [B*Ho*Wo, Cout] */
    const uint16_t* wT_split;                   /* transposed weight planes Wt[ci][9][co] (bd_split_wt) */
    float* dx; int64_t lddx; int accumulate;    /* [B*4HoWo, Cin] */
    int mode;                                   /* BD_MODE_BF16X3 (or 0) / BD_MODE_BF16, as bd_conv3x3_ps_desc.mode */
} bd_conv3x3_s2_dgrad_desc;
int bd_conv3x3_s2_dgrad_ps(const bd_conv3x3_s2_dgrad_desc* d, bd_stream_t stream);

/* Dense (batched) GEMM on split planes -- the attention block's GEMMs (attention.py:85-186: query / key / value / proj_attn Linear
 * layers, baddbmm(q, k^T), bmm(probs, v)) and their backward, without converting an operand on the way into LDS:
 *     C[m][n] = out_scale * (alpha * sum_k A[m][k] B[n][k] + bias[n] + residual[m][n])   (+ C[m][n] when accumulate)
 * a / b are split planes (bd_split_rows layout; ld and batch strides in 4-byte units, as for the fp32 tensor they replace):
 *   K-contiguous (x_kmajor = 0): rows = M (a) or N (b, "weights [N][K]"), K along the row;
 *   K-major      (x_kmajor = 1): rows = K, the M (a) or N (b) index along the row (both operands of a weight gradient, V of P V).
 * The result is written as fp32 (c), as split planes (c_split: the next GEMM's operand), or both.  a_colsum (optional, both operands
 * K-major, no batch): a_colsum[m] = sum_k A[k][m], the bias gradient of a Linear layer, from the same launch.
 * M, N % 128 == 0, K % 32 == 0; operand planes 128-byte aligned.  Long-K products with few tiles split K over workgroups with a
 * fixed-order second pass (deterministic): workspace >= bd_gemm_sp_workspace_bytes().                                           */
typedef struct {
    int M, N, K, batch;                          /* batch <= 1: one product                                        */
    const uint16_t* a; int64_t lda, a_bs; int a_kmajor;
    const uint16_t* b; int64_t ldb, b_bs; int b_kmajor;
    float* c; int64_t ldc, c_bs;                 /* fp32 output [batch][M][ldc] or NULL                            */
    uint16_t* c_split; int64_t ldcs, cs_bs;      /* split-plane output (rows of ldcs 4-byte units) or NULL         */
    const float* bias;                           /* [N] or NULL                                                    */
    const float* residual; int64_t ldr, r_bs;    /* [batch][M][ldr] or NULL                                        */
    float alpha, out_scale;
    int accumulate;                              /* c += ...  (needs c)                                            */
    float* a_colsum;                             /* [M] or NULL                                                    */
    void* workspace; size_t workspace_bytes;
    int mode;                                    /* BD_MODE_BF16X3 (or 0) / BD_MODE_BF16, as bd_conv3x3_ps_desc.mode */
} bd_gemm_sp_desc;
size_t bd_gemm_sp_workspace_bytes(const bd_gemm_sp_desc* d);
int bd_gemm_sp(const bd_gemm_sp_desc* d, bd_stream_t stream);
/* What bd_gemm_sp decides for a descriptor: host code only, a copy of the plan the launcher and bd_gemm_sp_workspace_bytes themselves
 * read.  bd_gemm_sp_plan runs the checks of bd_gemm_sp on the descriptor's numbers (mode, shape, strides, accumulate / a_colsum rules:
 * same status, same message) and launches nothing; it reads none of the descriptor's pointers beyond whether c, c_split, residual, bias
 * and a_colsum are set, and neither needs nor checks a workspace.  For tests and tools that must know which branch a call takes
 * (DESIGN.md "K split of the split-plane GEMM"). */
typedef struct {
    int form;                   /* operand form, 2 * a_kmajor + b_kmajor: 0 both K-contiguous ("nt"), 1 B K-major ("nn"), 2 A K-major
                                   ("tn_a"), 3 both K-major ("tn") -- the kernel instantiation, with the descriptor's mode            */
    int tiles_m, tiles_n;       /* 128 x 128 output tiles: M / 128, N / 128                                                       */
    int batch;                  /* products: max(batch, 1)                                                                        */
    int ksplit, chunks_per_split;   /* K slices and 32-element chunks per slice (the last slice may be shorter, never empty)      */
    int reduce;                 /* 1: gemm_sp_reduce folds the slabs and applies the epilogue (ksplit > 1)                        */
    int colsum_reduce;          /* 1: gemm_sp_colsum_reduce folds the partial rows of a_colsum (reduce, and a_colsum is set)      */
    int64_t grid;               /* workgroups of the main kernel = tiles_m * tiles_n * batch * ksplit                             */
    size_t workspace_bytes;     /* = bd_gemm_sp_workspace_bytes (with BD_GEMM_SP unset): ksplit * (M N + M) floats where reduce is set */
    size_t colsum_offset;       /* bytes in front of the ksplit partial rows of a_colsum [ksplit][M] (behind the slabs), else 0   */
    const char* prof_class;     /* the profiler class the launch is counted under                                                */
} bd_gemm_sp_plan_info;
int bd_gemm_sp_plan(const bd_gemm_sp_desc* d, bd_gemm_sp_plan_info* out);

/* Attention core on split planes (attention.py:148-162 and its backward), N = 256 tokens, head dim 256:
 *   forward : o = softmax(scale * q k^T) v                         [+ pt_split = P^T planes, needed by the backward]
 *   backward: dq = scale * dS k, dk = scale * dS^T q, dv = P^T dO,  dS = P o (dP - rowsum(P o dP)), dP = dO v^T
 * qkv_split: planes of the QKV projection's output [B*N, ld] (q | k | v column blocks, head h at column h*dh of each);
 * o_split / do_split [B*N, C]; pt_split / dst_split [B*heads, N, N] planes of the TRANSPOSED probability / score-gradient matrices
 * (rows = keys); dqkv_split: planes in the layout of qkv_split.  No [N, N] fp32 matrix is written.  The [N, N] products, the softmax
 * and their backward run in three launches per block instead of eight.  Other shapes: BD_ERR_UNSUPPORTED (bd_attn_sp_supported). */
typedef struct {
    int B, heads, N, dh;
    const uint16_t* qkv_split; int64_t ld;
    float scale;
    uint16_t* o_split; int64_t ldo;            /* forward out */
    uint16_t* pt_split;                        /* forward out (NULL: inference), backward in */
    const uint16_t* do_split; int64_t lddo;    /* backward in */
    uint16_t* dst_split;                       /* backward scratch [B*heads, N, N] planes */
    uint16_t* dqkv_split; int64_t lddqkv;      /* backward out */
    int mode;                                  /* BD_MODE_BF16X3 (or 0) / BD_MODE_BF16, as bd_conv3x3_ps_desc.mode; BD_MODE_BF16 rounds
                                                  P (and dS) to bf16 once, the hi plane the three-product form also uses */
} bd_attn_sp_desc;
int bd_attn_sp_supported(int N, int dh);
int bd_attn_sp_fwd(const bd_attn_sp_desc* d, bd_stream_t stream);
int bd_attn_sp_bwd(const bd_attn_sp_desc* d, bd_stream_t stream);

/* What the matrix pipe alone sustains on THIS board, now: v_mfma_f32_32x32x16_bf16 on register operands only (no memory
 * traffic), 2 workgroups of 512 threads per CU, `iters` x 12 MFMAs per wave, launched `launches` times back to back and timed
 * with a hipEvent pair on `stream` (blocks until done).  random_operands = 0: small constant integers (data-independent
 * issue rate, ~2.47 PFLOP/s); 1: per-lane random bf16 in [-1, 1) -- the board's power limit pulls the clock down and the
 * figure is what bounds a real kernel (bench.py `roofline.mfma_power_limited_peak_measured`).  *tflops = bf16 MFMA TFLOP/s. */
int bd_mfma_probe(int random_operands, int iters, int launches, double* tflops, bd_stream_t stream);

/* dst[i] (+)= scale * src[i] over a flat fp32 range (gradient accumulation across micro-batches). */
int bd_axpy(const float* src, float* dst, int64_t n, float scale, int accumulate, bd_stream_t stream);

/* bd_adam_clip with the step-dependent scalars read from DEVICE memory (hipGraph replay):
 * hyper = { lr / (1 - b1^step), sqrt(1 - b2^step) } */
int bd_adam_clip_dev(float* p, const float* g, float* m, float* v, int64_t n, const double* sumsq,
                     double max_norm, const float* hyper, double b1, double b2, double eps,
                     float* grad_norm_out, bd_stream_t stream);

/* a-8 + EMA: the exponential moving average of the weights (diffusers/training_utils.py:176-204, EMAModel.step) over ONE
 * flat fp32 shadow buffer `ema` of the same n floats as p:
 *   s_param.sub_(one_minus_decay * (s_param - param))   ==   s <- s - fl(omd * fl(s - p)),  omd = (float)(1 - decay),
 * three separately rounded fp32 operations (never a contracted fma), so the shadow carries the bits torch computes.
 * decay 0 gives s - (s - p), which is not always p; the reference has the same property.
 * bd_adam_clip_ema: bd_adam_clip plus the shadow update in the SAME launch, from the p[i] it has just stored; p, m, v and
 *   *grad_norm_out are bit-identical to bd_adam_clip on the same inputs.  Scalar accesses: any 4-byte aligned `ema` is valid.
 * bd_adam_clip_ema_dev: the hipGraph form, hyper = { lr / (1 - b1^step), sqrt(1 - b2^step), one_minus_decay } in DEVICE memory.
 * bd_ema_update: the stand-alone update (EMAModel.step outside a training engine), same formula, same bits.
 * Host checks before any launch (BD_ERR_INVALID): null pointers, n <= 0; one_minus_decay not finite or outside [0, 1]; `ema`
 * overlapping p, m, v or g as ranges of n floats.  The _dev form checks pointers only. */
int bd_adam_clip_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const double* sumsq,
                     double max_norm, double lr, double b1, double b2, double eps, int step, float one_minus_decay,
                     float* grad_norm_out, bd_stream_t stream);
int bd_adam_clip_ema_dev(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const double* sumsq,
                         double max_norm, const float* hyper, double b1, double b2, double eps,
                         float* grad_norm_out, bd_stream_t stream);
int bd_ema_update(float* ema, const float* p, int64_t n, float one_minus_decay, bd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BD_HIP_H */
