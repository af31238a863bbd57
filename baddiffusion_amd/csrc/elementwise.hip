// HBM-bound elementwise / reduction kernels of the BadDiffusion hot path (gfx950).
// Compiled with -ffp-contract=off so the fp32 operation order of the reference's eager PyTorch
// ops (separate mul / add kernels, no FMA contraction) is reproduced exactly where the formula
// order is copied (q_sample, scheduler steps).
#include "common.h"
#include "step_check.h"

#include <cmath>
#include <mutex>
#include <string>

namespace bd {

static thread_local std::string g_err;
void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

constexpr int TPB = 256;
static inline unsigned nblocks(int64_t n, int per = TPB, int64_t cap = 1 << 20) {
    int64_t b = cdiv(n, per);
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (unsigned)b;
}

// ------------------------------------------------------------------------------------------------
// a-1 + a-2: trigger blend + BadDiffusion q_sample.  One thread per (b, pixel); loops channels.
// dataset.py:275-276, :288-315 ; util.py:111 ; loss.py:264-285 ; scheduling_ddpm.py:429-442
// ------------------------------------------------------------------------------------------------
// The coefficient of R in the training target.  TABLE = false: the reference's rho_t (loss.py:270), from alphas[t] and s = sqrt(1 - ac_t).
// TABLE = true (the *_corr descriptors): the caller's table corr[t], DESIGN.md section 3 "Sampler-matched correction terms"; alphas is
// not read.  Everything else of the two kernel bodies below is common to both, so x_noisy and the optional outputs cannot differ.
template <bool TABLE, class D>
__device__ __forceinline__ float target_coef(const D& d, int64_t t, float s) {
    if constexpr (TABLE) {
        return d.corr[t];
    } else {
        const float al = d.alphas[t];
        return (1.0f - sqrtf(al)) * s / (1.0f - al);
    }
}

template <bool TABLE, class D>
__device__ __forceinline__ void poison_qsample_body(const D& d) {
    const int64_t hw = (int64_t)d.H * d.W;
    const int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (idx >= (int64_t)d.B * hw) return;
    const int b = (int)(idx / hw);
    const int64_t pix = idx - (int64_t)b * hw;
    const int64_t t = d.timesteps[b];
    const float ac = d.alphas_cumprod[t];
    const float a = sqrtf(ac);                       // alphas_cumprod[t] ** 0.5
    const float s = sqrtf(1.0f - ac);                // (1 - alphas_cumprod[t]) ** 0.5
    const float rho = target_coef<TABLE>(d, t, s);
    const bool poison = d.is_poison[b] != 0;
    // fused DataLoader gather + RandomHorizontalFlip (dataset.py:127-128): batch row b reads image row_index[b] of the
    // resident array, mirrored along W when flip[b]
    const int64_t sb = d.row_index ? d.row_index[b] : b;
    int64_t spix = pix;
    if (d.flip && d.flip[b]) {
        const int64_t y = pix / d.W;
        spix = y * d.W + (d.W - 1 - (pix - y * d.W));
    }
    for (int c = 0; c < d.C; ++c) {
        const int64_t chw = (int64_t)c * hw + pix;
        float x;
        if (d.images_u8) {
            // ToTensor (/255) then normalize(0,1 -> -1,1, eps=1e-5): ((x-0)/(1-0+eps))*(2)+(-1)
            float u = (float)d.images_u8[(sb * hw + spix) * d.C + c] / 255.0f;
            x = (u / (1.0f + 1e-5f)) * 2.0f + -1.0f;
        } else {
            x = d.images_f32[sb * d.C * hw + (int64_t)c * hw + spix];
        }
        const float g = d.trigger[chw];
        const float m = g > d.vmin ? 0.0f : 1.0f;                     // get_mask
        float R = 0.0f, x0 = x;
        if (poison) {
            R = m * x + (1.0f - m) * g;                               // dataset.py:312
            x0 = d.target_img[chw];
        }
        const float eps = d.noise[(int64_t)b * d.C * hw + chw];
        const float noisy = a * x0 + s * eps;                         // add_noise
        d.x_noisy[idx * d.ld_noisy + c] = noisy + (1.0f - a) * R;     // loss.py:285
        d.target[idx * d.ld_target + c] = rho * R + eps;
        if (d.R_out) d.R_out[(int64_t)b * d.C * hw + chw] = R;
        if (d.x0_out) d.x0_out[(int64_t)b * d.C * hw + chw] = x0;
        if (d.mask_out && b == 0) d.mask_out[chw] = g > d.vmin ? 0 : 1;
        if (d.image_out) d.image_out[(int64_t)b * d.C * hw + chw] = x;
    }
}

__global__ __launch_bounds__(TPB) void poison_qsample_kernel(bd_poison_qsample_desc d) { poison_qsample_body<false>(d); }
__global__ __launch_bounds__(TPB) void poison_qsample_corr_kernel(bd_poison_qsample_corr_desc d) { poison_qsample_body<true>(d); }

template <bool TABLE, class D>
__device__ __forceinline__ void qsample_body(const D& d) {
    const int64_t hw = (int64_t)d.H * d.W;
    const int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (idx >= (int64_t)d.B * hw) return;
    const int b = (int)(idx / hw);
    const int64_t pix = idx - (int64_t)b * hw;
    const int64_t t = d.timesteps[b];
    const float ac = d.alphas_cumprod[t];
    const float a = sqrtf(ac), s = sqrtf(1.0f - ac);
    const float rho = target_coef<TABLE>(d, t, s);
    for (int c = 0; c < d.C; ++c) {
        const int64_t src = (int64_t)b * d.C * hw + (int64_t)c * hw + pix;
        const float x0 = d.x0[src], R = d.R[src], eps = d.noise[src];
        const float noisy = a * x0 + s * eps;
        d.x_noisy[idx * d.ld_noisy + c] = noisy + (1.0f - a) * R;
        d.target[idx * d.ld_target + c] = rho * R + eps;
    }
}
__global__ __launch_bounds__(TPB) void qsample_kernel(bd_qsample_desc d) { qsample_body<false>(d); }
__global__ __launch_bounds__(TPB) void qsample_corr_kernel(bd_qsample_corr_desc d) { qsample_body<true>(d); }

__global__ __launch_bounds__(TPB) void nchw_to_nhwc_kernel(const float* src, float* dst, int B, int C, int64_t hw, int64_t ld) {
    const int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (idx >= (int64_t)B * hw) return;
    const int b = (int)(idx / hw);
    const int64_t pix = idx - (int64_t)b * hw;
    for (int c = 0; c < C; ++c) dst[idx * ld + c] = src[((int64_t)b * C + c) * hw + pix];
}
__global__ __launch_bounds__(TPB) void nhwc_to_nchw_kernel(const float* src, int64_t ld, float* dst, int B, int C, int64_t hw) {
    const int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (idx >= (int64_t)B * hw) return;
    const int b = (int)(idx / hw);
    const int64_t pix = idx - (int64_t)b * hw;
    for (int c = 0; c < C; ++c) dst[((int64_t)b * C + c) * hw + pix] = src[idx * ld + c];
}

// ------------------------------------------------------------------------------------------------
// a-5: DDPM reverse step (scheduling_ddpm.py:350-415).  Coefficients recomputed per thread from the
// device table in the same fp32 order the reference uses on 0-dim CPU tensors.
// ------------------------------------------------------------------------------------------------
// (X0Coef, x0_coef, x0_pred: common.h)
// dynamic thresholding (scheduling_ddpm.py:313-318): s = clamp(q, 1, sample_max_value), a NaN quantile staying NaN (fmaxf would drop it);
// x0 = clamp(x0, -s, s) / s, a true division
__device__ __forceinline__ float x0_threshold(float x0, float q, float smax) {
    const float s = q != q ? q : fminf(fmaxf(q, 1.0f), smax);
    return fminf(fmaxf(x0, -s), s) / s;
}

template <bool THR>
__global__ __launch_bounds__(TPB) void ddpm_step_kernel(bd_ddpm_step_desc d) {
    const float a_t = d.alphas_cumprod[d.t];
    const float a_prev = d.prev_t >= 0 ? d.alphas_cumprod[d.prev_t] : 1.0f;
    const float b_t = 1.0f - a_t, b_prev = 1.0f - a_prev;
    const float cur_alpha = a_t / a_prev, cur_beta = 1.0f - cur_alpha;
    const X0Coef k0 = x0_coef(d.alphas_cumprod, d.t);
    const float c0 = (sqrtf(a_prev) * cur_beta) / b_t;
    const float ct = sqrtf(cur_alpha) * b_prev / b_t;
    float sd = 0.f;
    if (d.t > 0) {
        float var = b_prev / b_t * cur_beta;          // (1 - a_prev) / (1 - a_t) * current_beta_t
        var = fmaxf(var, 1e-20f);
        if (d.variance_type == 1) var = cur_beta;     // fixed_large
        sd = sqrtf(var);
    }
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * TPB) {
        const float x = d.sample[i], e = d.model_output[i];
        float x0 = x0_pred(k0, x, e);
        if (THR) x0 = x0_threshold(x0, d.x0_quantile[(unsigned)i / (unsigned)d.image_elems], d.sample_max_value);   // n < 2^31 here
        else if (d.clip_sample) x0 = fminf(fmaxf(x0, -d.clip_sample_range), d.clip_sample_range);
        float prev = c0 * x0 + ct * x;
        if (d.t > 0) prev = prev + sd * d.noise[i];
        if (d.clip_defense) prev = fminf(fmaxf(prev, -d.clip_defense_range), d.clip_defense_range);
        d.prev_sample[i] = prev;
        if (d.pred_original) d.pred_original[i] = x0;
    }
}

// a-6: DDIM step (scheduling_ddim.py:300-381), epsilon prediction.
template <bool THR>
__global__ __launch_bounds__(TPB) void ddim_step_kernel(bd_ddim_step_desc d) {
    const float a_t = d.alphas_cumprod[d.t];
    const float a_prev = d.prev_t >= 0 ? d.alphas_cumprod[d.prev_t] : d.final_alpha_cumprod;
    const float b_t = 1.0f - a_t, b_prev = 1.0f - a_prev;
    const X0Coef k0 = x0_coef(d.alphas_cumprod, d.t);
    const float var = (b_prev / b_t) * (1.0f - a_t / a_prev);
    const float sd = d.eta * sqrtf(var);
    const float dir = sqrtf(1.0f - a_prev - sd * sd);
    const float sap = sqrtf(a_prev);
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * TPB) {
        const float x = d.sample[i], e = d.model_output[i];
        float x0 = x0_pred(k0, x, e);
        if (THR) x0 = x0_threshold(x0, d.x0_quantile[(unsigned)i / (unsigned)d.image_elems], d.sample_max_value);   // n < 2^31 here
        else if (d.clip_sample) x0 = fminf(fmaxf(x0, -d.clip_sample_range), d.clip_sample_range);
        float prev = sap * x0 + dir * e;
        if (d.eta > 0.f) prev = prev + sd * d.noise[i];
        d.prev_sample[i] = prev;
        if (d.pred_original) d.pred_original[i] = x0;
    }
}

// ------------------------------------------------------------------------------------------------
// Dynamic thresholding's order statistic (scheduling_ddpm.py:311): out[b] = torch.quantile(|v_b|, q) per image, exact.
// |v| as an integer (the 31 value bits) is monotone in |v|, so the two order statistics around the rank are found by a radix select on
// those bits, most significant first, in passes of 11, 10 and 10 bits: a pass counts, in an LDS histogram, the field of every key whose
// higher bits equal the prefix found so far, then walks the counts to the bucket that holds the rank.  After the third pass the
// prefix IS the key, so no value is looked up again.  Two ranks (lo and ceil(rank)) are followed at once, in two histograms from the
// pass where their prefixes part.  Integer counts do not depend on arrival order: the result is deterministic.
// One workgroup per image.  VPT > 0: the image's keys stay in VPT registers per thread (read once); VPT == 0: every pass reads it again.
// ------------------------------------------------------------------------------------------------
constexpr int AQ_BUCKETS = 2048;                                  // 2^11, the widest pass
constexpr int AQ_REG_THREADS = 256, AQ_REG_VPT = 16;              // registers path: m <= 4096
constexpr int AQ_REG_MAX = AQ_REG_THREADS * AQ_REG_VPT;
constexpr int AQ_STREAM_THREADS = 1024;
constexpr unsigned AQ_NO_KEY = 0xffffffffu;                       // bit 31 set: matches no prefix in any pass
constexpr unsigned AQ_INF = 0x7f800000u;

struct AqArgs {
    const float* x; const float* e; const float* alphas_cumprod; int t;
    int64_t m; unsigned lo, hi; float w; float* out;
};

// exclusive prefix sum of one count per thread over the workgroup (wave scan, then the totals of the waves before)
template <int NT>
__device__ __forceinline__ unsigned aq_excl_scan(unsigned v, unsigned* wave_tot) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) wave_tot[wv] = inc;
    __syncthreads();
    unsigned base = 0;
    for (int i = 0; i < wv; ++i) base += wave_tot[i];
    __syncthreads();
    return base + inc - v;
}

// the bucket of hist[0 .. nb) in which the running count first exceeds k (k < the total), and k's rank inside it: res = {bucket, rank}
template <int NT>
__device__ __forceinline__ void aq_select(const unsigned* hist, int nb, unsigned k, unsigned* wave_tot, unsigned* res) {
    const int per = nb / NT, first = threadIdx.x * per;          // nb is 2048 or 1024, NT 256 or 1024
    unsigned sum = 0;
    for (int j = 0; j < per; ++j) sum += hist[first + j];
    const unsigned excl = aq_excl_scan<NT>(sum, wave_tot);
    if (k >= excl && k - excl < sum) {                           // one thread: the counts before it are <= k, with its own they exceed k
        unsigned run = excl;
        for (int j = 0; j < per; ++j) {
            const unsigned c = hist[first + j];
            if (k - run < c) { res[0] = (unsigned)(first + j); res[1] = k - run; break; }
            run += c;
        }
    }
    __syncthreads();
}

template <int NT, int VPT>
__global__ __launch_bounds__(NT) void abs_quantile_kernel(AqArgs a) {
    __shared__ unsigned hist[2][AQ_BUCKETS];
    __shared__ unsigned wave_tot[NT / 64];
    __shared__ unsigned res[2][2];
    __shared__ unsigned has_nan;
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * a.m;
    const float* x = a.x + base;
    const float* e = a.e ? a.e + base : nullptr;
    X0Coef kf = {0.f, 1.f};
    if (e) kf = x0_coef(a.alphas_cumprod, a.t);
    auto key_at = [&](int64_t i) -> unsigned {
        float v = x[i];
        if (e) v = x0_pred(kf, v, e[i]);
        return __float_as_uint(v) & 0x7fffffffu;                 // |v|: -0 becomes 0, a NaN stays above AQ_INF
    };
    unsigned key[VPT > 0 ? VPT : 1];
    if (VPT > 0) {
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const int64_t i = tid + (int64_t)j * NT;
            key[j] = i < a.m ? key_at(i) : AQ_NO_KEY;
        }
    }
    if (tid == 0) has_nan = 0;
    unsigned prefix[2] = {0u, 0u}, k[2] = {a.lo, a.hi};
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 20 : pass == 1 ? 10 : 0;
        const int bits = pass == 0 ? 11 : 10, nb = 1 << bits;
        const bool same = prefix[0] == prefix[1];                // uniform over the workgroup
        for (int i = tid; i < 2 * AQ_BUCKETS; i += NT) (&hist[0][0])[i] = 0;
        __syncthreads();
        bool nan = false;
        auto count = [&](unsigned ky) {
            if (pass == 0 && ky > AQ_INF && ky != AQ_NO_KEY) nan = true;
            const unsigned up = ky >> (shift + bits);            // the bits above this pass's field (pass 0: bit 31, 0 for every key)
            const unsigned b = (ky >> shift) & (unsigned)(nb - 1);
            if (up == prefix[0]) atomicAdd(&hist[0][b], 1u);
            if (!same && up == prefix[1]) atomicAdd(&hist[1][b], 1u);
        };
        if (VPT > 0) {
#pragma unroll
            for (int j = 0; j < VPT; ++j) count(key[j]);
        } else {
            for (int64_t i = tid; i < a.m; i += NT) count(key_at(i));
        }
        if (pass == 0 && nan) atomicOr(&has_nan, 1u);
        __syncthreads();
        aq_select<NT>(hist[0], nb, k[0], wave_tot, res[0]);
        aq_select<NT>(hist[same ? 0 : 1], nb, k[1], wave_tot, res[1]);       // under one prefix the two ranks may still part here
        const unsigned b0 = res[0][0], r0 = res[0][1], b1 = res[1][0], r1 = res[1][1];
        __syncthreads();
        prefix[0] = (prefix[0] << bits) | b0; k[0] = r0;
        prefix[1] = (prefix[1] << bits) | b1; k[1] = r1;
    }
    if (tid == 0) {
        float r = __uint_as_float(0x7fc00000u);
        if (!has_nan) {
            const float lo = __uint_as_float(prefix[0]), hi = __uint_as_float(prefix[1]);
            const float d = hi - lo;
            r = a.w < 0.5f ? fmaf(a.w, d, lo) : fmaf(-d, 1.0f - a.w, hi);       // at::lerp, fused as the reference's CPU kernel is
        }
        a.out[blockIdx.x] = r;
    }
}

// ------------------------------------------------------------------------------------------------
// RePaint (scheduling_repaint.py:250-293 step, :303-318 undo_step).  The dense operands share one dense layout, so the kernels walk
// the STORAGE index i (16-byte accesses when aligned) and rebuild from it the coordinate along each dimension in storage order
// (dimension 0 outermost); the broadcast operands (original image, mask, shift) are gathered at sum_j coord[j] * stride[j] with their
// own strides permuted to that order by the host, 0 along a broadcast dimension.  The launchers turn away 2^31 elements and more, so
// the coordinates are 32-bit: three 32-bit divisions per thread and pass.
// ------------------------------------------------------------------------------------------------
struct RpGeom {
    int64_t n;                       // elements
    unsigned sz[4];                  // sizes in storage order
    int64_t os[4], ms[4], ss[4];     // strides of original image / mask / shift in storage order
};
struct RpCoord {
    unsigned c[4];
    __device__ __forceinline__ RpCoord(unsigned idx, const RpGeom& g) {
        c[3] = idx % g.sz[3]; idx /= g.sz[3];
        c[2] = idx % g.sz[2]; idx /= g.sz[2];
        c[1] = idx % g.sz[1]; c[0] = idx / g.sz[1];
    }
    __device__ __forceinline__ void next(const RpGeom& g) {      // the coordinate of storage index + 1
        if (++c[3] == g.sz[3]) {
            c[3] = 0;
            if (++c[2] == g.sz[2]) {
                c[2] = 0;
                if (++c[1] == g.sz[1]) { c[1] = 0; ++c[0]; }
            }
        }
    }
    __device__ __forceinline__ int64_t at(const int64_t (&s)[4]) const {
        return (int64_t)c[0] * s[0] + (int64_t)c[1] * s[1] + (int64_t)c[2] * s[2] + (int64_t)c[3] * s[3];
    }
};

// the scalars of one step, in the fp32 order of ddim_step_kernel (mask == 0 reproduces its bits)
struct RpStepCoef { float sb, sa, sap, dir, sd, sbp, sh; bool var; };
__device__ __forceinline__ RpStepCoef rp_step_coef(const bd_repaint_step_desc& d) {
    RpStepCoef k;
    const float a_t = d.alphas_cumprod[d.t];
    const float a_prev = d.prev_t >= 0 ? d.alphas_cumprod[d.prev_t] : d.final_alpha_cumprod;
    const float b_t = 1.0f - a_t, b_prev = 1.0f - a_prev;
    k.sb = sqrtf(b_t); k.sa = sqrtf(a_t);
    const float var = (b_prev / b_t) * (1.0f - a_t / a_prev);
    k.sd = d.eta * sqrtf(var);
    k.dir = sqrtf(1.0f - a_prev - k.sd * k.sd);
    k.sap = sqrtf(a_prev);
    k.sbp = sqrtf(b_prev);
    k.sh = 1.0f - k.sap;
    k.var = d.t > 0 && d.eta > 0.f;
    return k;
}
__device__ __forceinline__ float rp_step_elem(const RpStepCoef& k, const bd_repaint_step_desc& d, float x, float e, float z, float o,
                                              float m, float s, float& x0) {
    x0 = (x - k.sb * e) / k.sa;
    if (d.clip_sample) x0 = fminf(fmaxf(x0, -d.clip_sample_range), d.clip_sample_range);
    float unknown = k.sap * x0 + k.dir * e;
    if (k.var) unknown = unknown + k.sd * z;
    float known = k.sap * o + k.sbp * z;
    if (d.shift) known = known + k.sh * s;
    return m * known + (1.0f - m) * unknown;
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void repaint_step_kernel(bd_repaint_step_desc d, RpGeom g) {
    const RpStepCoef k = rp_step_coef(d);
    const int64_t stride = (int64_t)gridDim.x * TPB;
    if (VEC) {
        const int64_t n4 = g.n >> 2;
        for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n4; i += stride) {
            const float4 xv = reinterpret_cast<const float4*>(d.sample)[i];
            const float4 ev = reinterpret_cast<const float4*>(d.model_output)[i];
            const float4 zv = reinterpret_cast<const float4*>(d.noise)[i];
            const float x[4] = {xv.x, xv.y, xv.z, xv.w}, e[4] = {ev.x, ev.y, ev.z, ev.w}, z[4] = {zv.x, zv.y, zv.z, zv.w};
            float o[4], m[4], s[4];
            RpCoord c((unsigned)(i << 2), g);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = d.original_image[c.at(g.os)];
                m[j] = d.mask[c.at(g.ms)];
                s[j] = d.shift ? d.shift[c.at(g.ss)] : 0.f;
                c.next(g);
            }
            float p[4], x0[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = rp_step_elem(k, d, x[j], e[j], z[j], o[j], m[j], s[j], x0[j]);
            reinterpret_cast<float4*>(d.prev_sample)[i] = make_float4(p[0], p[1], p[2], p[3]);
            if (d.pred_original) reinterpret_cast<float4*>(d.pred_original)[i] = make_float4(x0[0], x0[1], x0[2], x0[3]);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < g.n; i += stride) {
            const RpCoord c((unsigned)i, g);
            const float s = d.shift ? d.shift[c.at(g.ss)] : 0.f;
            float x0;
            d.prev_sample[i] = rp_step_elem(k, d, d.sample[i], d.model_output[i], d.noise[i], d.original_image[c.at(g.os)],
                                            d.mask[c.at(g.ms)], s, x0);
            if (d.pred_original) d.pred_original[i] = x0;
        }
    }
}

// undo_step: x <- sqrt(1 - beta_i) x + sqrt(beta_i) z_i [+ (1 - sqrt(1 - beta_i)) shift], i = 0..k-1 in order, x in registers
struct RpUndoArgs {
    const float* z[BD_REPAINT_UNDO_MAX];
    const float* x; float* out; const float* shift; const float* betas;
    int t, k;
};
template <bool VEC>
__global__ __launch_bounds__(TPB) void repaint_undo_kernel(RpUndoArgs a, RpGeom g) {
    float ca[BD_REPAINT_UNDO_MAX], cb[BD_REPAINT_UNDO_MAX], cs[BD_REPAINT_UNDO_MAX];
#pragma unroll
    for (int j = 0; j < BD_REPAINT_UNDO_MAX; ++j) {
        const float beta = j < a.k ? a.betas[a.t + j] : 0.f;
        ca[j] = sqrtf(1.0f - beta); cb[j] = sqrtf(beta); cs[j] = 1.0f - ca[j];
    }
    const int64_t stride = (int64_t)gridDim.x * TPB;
    if (VEC) {
        const int64_t n4 = g.n >> 2;
        for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n4; i += stride) {
            float4 zv[BD_REPAINT_UNDO_MAX];
#pragma unroll
            for (int j = 0; j < BD_REPAINT_UNDO_MAX; ++j)
                zv[j] = j < a.k ? reinterpret_cast<const float4*>(a.z[j])[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 xv = reinterpret_cast<const float4*>(a.x)[i];
            float x[4] = {xv.x, xv.y, xv.z, xv.w}, s[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.shift) {
                RpCoord c((unsigned)(i << 2), g);
#pragma unroll
                for (int l = 0; l < 4; ++l) { s[l] = a.shift[c.at(g.ss)]; c.next(g); }
            }
#pragma unroll
            for (int j = 0; j < BD_REPAINT_UNDO_MAX; ++j)
                if (j < a.k) {
                    const float z[4] = {zv[j].x, zv[j].y, zv[j].z, zv[j].w};
#pragma unroll
                    for (int l = 0; l < 4; ++l) {
                        x[l] = ca[j] * x[l] + cb[j] * z[l];
                        if (a.shift) x[l] = x[l] + cs[j] * s[l];
                    }
                }
            reinterpret_cast<float4*>(a.out)[i] = make_float4(x[0], x[1], x[2], x[3]);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < g.n; i += stride) {
            float x = a.x[i], s = 0.f;
            if (a.shift) { const RpCoord c((unsigned)i, g); s = a.shift[c.at(g.ss)]; }
#pragma unroll
            for (int j = 0; j < BD_REPAINT_UNDO_MAX; ++j)
                if (j < a.k) {
                    x = ca[j] * x + cb[j] * a.z[j][i];
                    if (a.shift) x = x + cs[j] * s;
                }
            a.out[i] = x;
        }
    }
}

// a-7: (x/2+0.5).clamp(0,1) -> NHWC float / uint8 (pipeline_ddpm.py:115-116, model.py:499)
__global__ __launch_bounds__(TPB) void to_image_kernel(const float* x, int nhwc, int64_t ld, int B, int C, int64_t hw,
                                                     float* of, uint8_t* ou) {
    const int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (idx >= (int64_t)B * hw) return;
    const int b = (int)(idx / hw);
    const int64_t pix = idx - (int64_t)b * hw;
    for (int c = 0; c < C; ++c) {
        float v = nhwc ? x[idx * ld + c] : x[((int64_t)b * C + c) * hw + pix];
        v = fminf(fmaxf(v / 2.0f + 0.5f, 0.0f), 1.0f);
        if (of) of[idx * C + c] = v;
        if (ou) ou[idx * C + c] = (uint8_t)rintf(v * 255.0f);
    }
}

// a-4a: get_timestep_embedding (embeddings.py:40-57).  T = int64_t (the schedulers' integer timesteps) or float (fractional timesteps:
// the sigma-space samplers interpolate the schedule); both are `timesteps[:, None].float() * emb`, so an integral float gives the bits
// of the integer.
template <typename T>
__global__ __launch_bounds__(TPB) void timestep_embedding_kernel(const T* t, int t_stride, int B, int dim, int flip,
                                                               float shift, float* out) {
    const int idx = blockIdx.x * TPB + threadIdx.x;
    const int half = dim / 2;
    if (idx >= B * half) return;
    const int b = idx / half, j = idx - b * half;
    const float neg_log = -9.210340371976184f;  // -math.log(10000) rounded to fp32
    float ex = neg_log * (float)j;
    ex = ex / ((float)half - shift);
    const float f = expf(ex);
    const float arg = (float)t[(int64_t)b * t_stride] * f;
    const float sn = sinf(arg), cs = cosf(arg);
    float* o = out + (int64_t)b * dim;
    if (flip) { o[j] = cs; o[half + j] = sn; } else { o[j] = sn; o[half + j] = cs; }
    if ((dim & 1) && j == 0) o[dim - 1] = 0.f;
}

__global__ __launch_bounds__(TPB) void silu_fwd_kernel(const float* x, float* y, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const float z = x[i];
        y[i] = z / (1.0f + expf(-z));
    }
}
__global__ __launch_bounds__(TPB) void silu_bwd_kernel(const float* x, const float* dy, float* dx, int64_t n, int acc) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const float z = x[i];
        const float s = 1.0f / (1.0f + expf(-z));
        float g = dy[i] * (s * (1.0f + z * (1.0f - s)));
        if (acc) g += dx[i];
        dx[i] = g;
    }
}

// ------------------------------------------------------------------------------------------------
// Row softmax (one wave per row) and backward (attention.py:161).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void softmax_fwd_kernel(const float* s, float* p, int64_t rows, int n) {
    const int64_t row = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* sr = s + row * n;
    float* pr = p + row * n;
    float mx = -INFINITY;
    for (int i = lane; i < n; i += 64) mx = fmaxf(mx, sr[i]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int i = lane; i < n; i += 64) sum += expf(sr[i] - mx);
    sum = wave_sum(sum);
    for (int i = lane; i < n; i += 64) pr[i] = expf(sr[i] - mx) / sum;
}
__global__ __launch_bounds__(TPB) void softmax_bwd_kernel(const float* p, const float* dp, float* ds, int64_t rows, int n) {
    const int64_t row = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* pr = p + row * n;
    const float* dr = dp + row * n;
    float* o = ds + row * n;
    float dot = 0.f;
    for (int i = lane; i < n; i += 64) dot += pr[i] * dr[i];
    dot = wave_sum(dot);
    for (int i = lane; i < n; i += 64) o[i] = pr[i] * (dr[i] - dot);
}

// ------------------------------------------------------------------------------------------------
// out[g, n] = sum_{m in group g} x[m, n].  Block = 64 columns x 4 row phases.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void colsum_kernel(const float* x, int64_t ldx, int64_t rows, int N, int64_t rpg,
                                                   float* out, int64_t ldo, int acc) {
    __shared__ float red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + tx;
    const int64_t g = blockIdx.y;
    const int64_t m0 = g * rpg;
    int64_t m1 = m0 + rpg;
    if (m1 > rows) m1 = rows;
    float s = 0.f;
    if (n < N)
        for (int64_t m = m0 + ty; m < m1; m += 4) s += x[m * ldx + n];
    red[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && n < N) {
        float v = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
        float* o = out + g * ldo + n;
        if (acc) v += *o;
        *o = v;
    }
}

// nearest-upsample backward: dx[b,y,x,c] (+)= sum of the 2x2 block of du
__global__ __launch_bounds__(TPB) void sum2x2_kernel(const float* du, int64_t ldu, float* dx, int64_t lddx, int B, int H, int W,
                                                   int C, int acc) {
    const int c4n = C / 4;
    const int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (idx >= (int64_t)B * H * W * c4n) return;
    const int c = (int)(idx % c4n) * 4;
    const int64_t pix = idx / c4n;
    const int x = (int)(pix % W);
    const int64_t by = pix / W;  // b*H + y
    const int y = (int)(by % H);
    const int b = (int)(by / H);
    const int64_t W2 = 2 * W;
    const int64_t base = ((int64_t)b * 2 * H + 2 * y) * W2 + 2 * x;
    const float4 v00 = *reinterpret_cast<const float4*>(du + base * ldu + c);
    const float4 v01 = *reinterpret_cast<const float4*>(du + (base + 1) * ldu + c);
    const float4 v10 = *reinterpret_cast<const float4*>(du + (base + W2) * ldu + c);
    const float4 v11 = *reinterpret_cast<const float4*>(du + (base + W2 + 1) * ldu + c);
    float4 r = make_float4((v00.x + v01.x) + (v10.x + v11.x), (v00.y + v01.y) + (v10.y + v11.y),
                           (v00.z + v01.z) + (v10.z + v11.z), (v00.w + v01.w) + (v10.w + v11.w));
    float4* o = reinterpret_cast<float4*>(dx + pix * lddx + c);
    if (acc) { float4 e = *o; r.x += e.x; r.y += e.y; r.z += e.z; r.w += e.w; }
    *o = r;
}

// dst[m, c] (+)= scale * src[m, c]   (residual-path gradient, channel-sliced views)
__global__ __launch_bounds__(TPB) void add_kernel(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int C,
                                                float scale, int acc) {
    const int c4n = C / 4;
    for (int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x; idx < rows * c4n; idx += (int64_t)gridDim.x * TPB) {
        const int c = (int)(idx % c4n) * 4;
        const int64_t m = idx / c4n;
        float4 v = *reinterpret_cast<const float4*>(src + m * lds + c);
        v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
        float4* o = reinterpret_cast<float4*>(dst + m * ldd + c);
        if (acc) { float4 e = *o; v.x += e.x; v.y += e.y; v.z += e.z; v.w += e.w; }
        *o = v;
    }
}

// ------------------------------------------------------------------------------------------------
// a-3 loss + dpred; a-8 sum of squares.  Two-stage deterministic reductions (fixed order).
// ------------------------------------------------------------------------------------------------
constexpr int RED_BLOCKS = 1024;

__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < TPB / 64; ++i) r += sh[i];
    return r;  // valid on thread 0
}

__global__ __launch_bounds__(TPB) void loss_kernel(const float* pred, int64_t ldp, const float* tgt, int64_t ldt, int64_t rows,
                                                 int C, int type, float gscale, float* dpred, int64_t lddp, double* part) {
    __shared__ double sh[TPB / 64];
    const int64_t n = rows * C;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const int64_t m = i / C;
        const int c = (int)(i - m * C);
        const float p = pred[m * ldp + c], t = tgt[m * ldt + c];
        const float df = p - t;   // d/dpred of loss(target, pred)
        float l, g;
        loss_elem(type, df, l, g);
        acc += (double)l;
        if (dpred) dpred[m * lddp + c] = g / (float)n * gscale;
    }
    double r = block_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}
// second stage of the two-stage reductions: one wave, lane l sums partials l, l+64, ... and the lanes are folded with a
// fixed shuffle tree (deterministic)
__device__ __forceinline__ double final_sum(const double* part, int nb) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += 64) s += part[i];
    return wave_sum(s);
}
__global__ __launch_bounds__(64) void loss_final_kernel(const double* part, int nb, int64_t n, float* loss) {
    const double s = final_sum(part, nb);
    if (threadIdx.x == 0) *loss = (float)(s / (double)n);
}

// Grouped form of the two kernels above: the rows are n_groups consecutive groups and blockIdx.y picks one.  Group g is walked by
// its own nb[g] blocks with the block / stride pattern loss_kernel uses for a whole array of rows[g] rows, so one group of weight 1
// reproduces loss_kernel's partials, loss and dpred bit for bit.  Partials of group g live at part[g * RED_BLOCKS ..].
struct LossGroups {
    int n_groups;
    int nb[BD_LOSS_MAX_GROUPS];
    int64_t row0[BD_LOSS_MAX_GROUPS], rows[BD_LOSS_MAX_GROUPS];
    float weight[BD_LOSS_MAX_GROUPS];
};
__global__ __launch_bounds__(TPB) void loss_groups_kernel(const float* pred, int64_t ldp, const float* tgt, int64_t ldt, int C, int type,
                                                        float gscale, float* dpred, int64_t lddp, double* part, LossGroups G) {
    __shared__ double sh[TPB / 64];
    const int grp = blockIdx.y, nb = G.nb[grp];
    if ((int)blockIdx.x >= nb) return;          // (uniform per block: before any barrier)
    const int64_t n = G.rows[grp] * C, row0 = G.row0[grp];
    const float w = G.weight[grp];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)nb * TPB) {
        const int64_t m = row0 + i / C;
        const int c = (int)(i % C);
        const float df = pred[m * ldp + c] - tgt[m * ldt + c];
        float l, g;
        loss_elem(type, df, l, g);
        acc += (double)l;
        if (dpred) dpred[m * lddp + c] = g / (float)n * gscale * w;
    }
    double r = block_sum(acc, sh);
    if (threadIdx.x == 0) part[(int64_t)grp * RED_BLOCKS + blockIdx.x] = r;
}
// losses[g] = S_g / n_g per group, losses[n_groups] = sum_g w_g S_g / n_g (fp64, groups in order)
__global__ __launch_bounds__(64) void loss_groups_final_kernel(const double* part, int C, float* losses, LossGroups G) {
    double total = 0.0;
    for (int grp = 0; grp < G.n_groups; ++grp) {
        const double s = final_sum(part + (int64_t)grp * RED_BLOCKS, G.nb[grp]);
        const double n = (double)(G.rows[grp] * C);
        if (threadIdx.x == 0) losses[grp] = (float)(s / n);
        total += (double)G.weight[grp] * s / n;
    }
    if (threadIdx.x == 0) losses[G.n_groups] = (float)total;
}

__global__ __launch_bounds__(TPB) void sumsq_kernel(const float* g, int64_t n, double* part) {
    __shared__ double sh[TPB / 64];
    double acc = 0.0;
    const int64_t n4 = n / 4;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n4; i += (int64_t)gridDim.x * TPB) {
        const float4 v = reinterpret_cast<const float4*>(g)[i];
        acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) { const float v = g[n4 * 4 + threadIdx.x]; acc += (double)v * v; }
    double r = block_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}
__global__ __launch_bounds__(64) void sumsq_final_kernel(const double* part, int nb, double* out) {
    const double s = final_sum(part, nb);
    if (threadIdx.x == 0) *out = s;
}

// clip_grad_norm_(max_norm) + torch.optim.Adam (single-tensor formulas), flat buffers.
// EMA = true: the shadow update of diffusers' EMAModel.step (training_utils.py:200-202) rides along, from the p[i] just stored:
// s.sub_(omd * (s - p)) is three separately rounded fp32 operations (sub, mul, sub) -- a contracted fma(-omd, s - p, s) is another
// number, so the roundings are spelled out.  hyper[2] = omd in the device-scalar form.  EMA = false is the kernel as it always was.
__device__ __forceinline__ float ema_shadow(float s, float p, float omd) { return __fsub_rn(s, __fmul_rn(omd, __fsub_rn(s, p))); }

template <bool EMA>
__global__ __launch_bounds__(TPB) void adam_clip_kernel(float* p, const float* g, float* m, float* v, int64_t n,
                                                      const double* sumsq, float max_norm, float step_size, float omb1,
                                                      float b2, float omb2, float eps, float bc2_sqrt, float* gn_out,
                                                      const float* hyper, float* ema, float omd) {
    if (hyper) { step_size = hyper[0]; bc2_sqrt = hyper[1]; if (EMA) omd = hyper[2]; }
    const float norm = (float)sqrt(*sumsq);
    float coef = max_norm / (norm + 1e-6f);
    coef = fminf(coef, 1.0f);
    if (gn_out && blockIdx.x == 0 && threadIdx.x == 0) *gn_out = norm;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const float gi = g[i] * coef;
        float mi = m[i], vi = v[i];
        mi = mi + (gi - mi) * omb1;                       // exp_avg.lerp_(grad, 1 - beta1)
        vi = vi * b2 + omb2 * gi * gi;                     // mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        const float pi = p[i] - step_size * (mi / denom); // addcdiv_(exp_avg, denom, -step_size)
        p[i] = pi;
        m[i] = mi;
        v[i] = vi;
        if (EMA) ema[i] = ema_shadow(ema[i], pi, omd);
    }
}

// EMAModel.step outside an optimizer step: the same three roundings over the same grid
__global__ __launch_bounds__(TPB) void ema_update_kernel(float* ema, const float* p, int64_t n, float omd) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) ema[i] = ema_shadow(ema[i], p[i], omd);
}


// ------------------------------------------------------------------------------------------------
// The dense vec4 driver of the sampler steps: n floats per operand, one layout, every pointer 16-byte aligned.  An operation is a struct
// with `template <class V> __device__ void at(int64_t i) const`, which states its loads, its per-element arithmetic and its stores once
// for the access width V: the grid walks the n4 = n / 4 float4s, block 0 the n % 4 floats behind them.  No __restrict__ anywhere: an output
// may be the very buffer an input is read from (same base pointer), so at() issues every load of index i before its first store.
// ------------------------------------------------------------------------------------------------
template <class V> __device__ __forceinline__ V ld(const float* p, int64_t i) { return reinterpret_cast<const V*>(p)[i]; }
template <class V> __device__ __forceinline__ void st(float* p, int64_t i, const V& v) { reinterpret_cast<V*>(p)[i] = v; }
template <class V> __device__ __forceinline__ V splat(float s);
template <> __device__ __forceinline__ float splat<float>(float s) { return s; }
template <> __device__ __forceinline__ float4 splat<float4>(float s) { return make_float4(s, s, s, s); }
// f(a.x, b.x, ...), f(a.y, b.y, ...), ... over the lanes of the operands (inputs by value or outputs by reference, as f takes them)
template <class F, class... A> __device__ __forceinline__ void lanes(F f, float& a0, A&... a) { f(a0, a...); }
template <class F, class... A> __device__ __forceinline__ void lanes(F f, float4& a0, A&... a) {
    f(a0.x, a.x...); f(a0.y, a.y...); f(a0.z, a.z...); f(a0.w, a.w...);
}
template <class Op>
__global__ __launch_bounds__(TPB) void vec4_kernel(Op op, int64_t n4, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n4; i += (int64_t)gridDim.x * TPB) op.template at<float4>(i);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) op.template at<float>((n & ~(int64_t)3) + threadIdx.x);   // tail (n % 4 elements)
}

// f-4 (PNDM family): out = clamp(sum_j c[j] * term[j]) over up to BD_LINCOMB_MAX dense fp32 tensors of one layout.
// Every PRK / PLMS update of scheduling_pndm.py:236-397 is such a combination of the running sample, the stored model
// outputs and the running accumulator, with host-computed scalar coefficients; the pipeline's post-step clip
// (pipeline_pndm.py:108-109) rides along.  out may be a term's own buffer (the ANP projection clamps in place).
struct LincombOp {
    const float* t[BD_LINCOMB_MAX]; float c[BD_LINCOMB_MAX]; int k; int clip; float range; float* out;
    template <class V> __device__ __forceinline__ void at(int64_t i) const {
        V v[BD_LINCOMB_MAX];
#pragma unroll
        for (int j = 0; j < BD_LINCOMB_MAX; ++j) v[j] = j < k ? ld<V>(t[j], i) : splat<V>(0.f);
        V r = splat<V>(0.f);
#pragma unroll
        for (int j = 0; j < BD_LINCOMB_MAX; ++j)
            if (j < k) lanes([cj = c[j]](float& r, float v) { r += cj * v; }, r, v[j]);
        if (clip) lanes([this](float& r) { r = fminf(fmaxf(r, -range), range); }, r);
        st<V>(out, i, r);
    }
};
constexpr auto lincomb_kernel = vec4_kernel<LincombOp>;      // the name bd_lincomb launches (the tests read its grid cap by it)


// f-4 (DPM-Solver / DPM-Solver++, scheduling_dpmsolver_multistep.py:301-505): one multistep update in one launch.  The conversion of
// the model output (x0-prediction with its clamp for dpmsolver++, eps as it is for dpmsolver) is not linear, so bd_lincomb cannot
// carry it; the first / second / third order updates are, once D1 and D2 are expanded on the host into coefficients of the stored
// converted outputs m0 (this step's), m1, m2.  m0 goes to the history ring, prev to the running sample.
__device__ __forceinline__ void dpm_elem(const bd_dpm_step_desc& d, float e, float x, float a, float b, float& m0, float& prev) {
    m0 = d.convert ? (x - d.sigma_s * e) / d.alpha_s : e;
    if (d.x0_clip) m0 = fminf(fmaxf(m0, -d.x0_range), d.x0_range);
    float r = d.cx * x + d.c0 * m0;
    if (d.m1) r += d.c1 * a;
    if (d.m2) r += d.c2 * b;
    if (d.clip) r = fminf(fmaxf(r, -d.clip_range), d.clip_range);
    prev = r;
}
struct DpmOp {
    bd_dpm_step_desc d;
    template <class V> __device__ __forceinline__ void at(int64_t i) const {
        V e = ld<V>(d.model_output, i), x = ld<V>(d.sample, i);
        V a = d.m1 ? ld<V>(d.m1, i) : splat<V>(0.f);
        V b = d.m2 ? ld<V>(d.m2, i) : splat<V>(0.f);
        V m0, p;
        lanes([this](float e, float x, float a, float b, float& m0, float& p) { dpm_elem(d, e, x, a, b, m0, p); }, e, x, a, b, m0, p);
        if (d.m0_out) st<V>(d.m0_out, i, m0);
        st<V>(d.prev_out, i, p);
    }
};


// f-4 (UniPC, scheduling_unipc_multistep.py:257-601): one whole step in one launch -- conversion, corrector (UniC) over the history as it
// stood before this step (h1, h2, h3, newest first) and the sample before the last predictor (l), then the predictor (UniP) from the
// corrected sample over the shifted history (m0, h1, h2).  Both updates are linear once the host has expanded their D1 differences and
// rho weights into coefficients, but they are chained through xc and share m0 with the conversion, so bd_dpm_step cannot carry them.
// Whether the output is converted and which of the four optional inputs are present are template parameters (the launcher picks
// the instance from the descriptor): the tests cost nothing, and every load stays one unconditional 16-byte access -- with run-time
// tests the compiler sinks the loads into the branches that use them and splits them into dwords.
template <bool CV, bool L, bool H1, bool H2, bool H3>
__device__ __forceinline__ void unipc_elem(const bd_unipc_step_desc& d, float e, float x, float l, float a, float b, float c, float& m0,
                                           float& xc, float& prev) {
    if constexpr (CV) m0 = (x - d.sigma_s * e) / d.alpha_s;
    else m0 = e;
    if (d.x0_clip) m0 = fminf(fmaxf(m0, -d.x0_range), d.x0_range);
    xc = x;
    if constexpr (L) {
        float r = d.kl * l + d.k0 * m0;
        r += d.k1 * a;
        if constexpr (H2) r += d.k2 * b;
        if constexpr (H3) r += d.k3 * c;
        xc = r;
    }
    float r = d.px * xc + d.p0 * m0;
    if constexpr (H1) r += d.p1 * a;
    if constexpr (H2) r += d.p2 * b;
    if (d.clip) r = fminf(fmaxf(r, -d.clip_range), d.clip_range);
    prev = r;
}
template <bool CV, bool L, bool H1, bool H2, bool H3>
struct UnipcOp {
    bd_unipc_step_desc d;
    template <class V> __device__ __forceinline__ void at(int64_t i) const {
        V e = ld<V>(d.model_output, i), x = ld<V>(d.sample, i);
        V l = splat<V>(0.f), a = l, b = l, c = l;
        if constexpr (L) l = ld<V>(d.last_sample, i);
        if constexpr (H1) a = ld<V>(d.h1, i);
        if constexpr (H2) b = ld<V>(d.h2, i);
        if constexpr (H3) c = ld<V>(d.h3, i);
        V m0, xc, p;
        lanes([this](float e, float x, float l, float a, float b, float c, float& m0, float& xc, float& p) {
            unipc_elem<CV, L, H1, H2, H3>(d, e, x, l, a, b, c, m0, xc, p);
        }, e, x, l, a, b, c, m0, xc, p);
        if (d.m0_out) st<V>(d.m0_out, i, m0);
        if (d.corrected_out) st<V>(d.corrected_out, i, xc);
        st<V>(d.prev_out, i, p);
    }
};
template <bool CV, bool L, bool H1, bool H2, bool H3>
static void unipc_launch(const bd_unipc_step_desc& d, hipStream_t stream) {
    hipLaunchKernelGGL((vec4_kernel<UnipcOp<CV, L, H1, H2, H3>>), dim3(nblocks(cdiv(d.n, 4), TPB, 4096)), dim3(TPB), 0, stream,
                       UnipcOp<CV, L, H1, H2, H3>{d}, d.n / 4, d.n);
}


// f-4 (DEIS, scheduling_deis_multistep.py:240-473, log-rho version): one multistep update in one launch.  The conversion goes through the
// x0-prediction and back to an eps prediction (four roundings: m0 is not e bitwise, and with the x0 clamp on a saturated element it is a
// different value altogether), and the second / third order updates are alpha_t * (x / alpha_s + ...) with a true division, so neither
// bd_dpm_step nor bd_lincomb can carry them bit for bit.  Which history terms are present are template parameters, as in UnipcOp.
template <bool M1, bool M2>
__device__ __forceinline__ void deis_elem(const bd_deis_step_desc& d, float e, float x, float a, float b, float& m0, float& prev) {
    float x0 = (x - d.sigma_s * e) / d.alpha_s;
    if (d.x0_clip) x0 = fminf(fmaxf(x0, -d.x0_range), d.x0_range);
    m0 = (x - d.alpha_s * x0) / d.sigma_s;
    float r;
    if constexpr (M1) {
        r = x / d.alpha_s + d.k0 * m0;
        r += d.k1 * a;
        if constexpr (M2) r += d.k2 * b;
        r = d.alpha_t * r;
    } else {
        r = d.cx * x - d.c0 * m0;
    }
    if (d.clip) r = fminf(fmaxf(r, -d.clip_range), d.clip_range);
    prev = r;
}
template <bool M1, bool M2>
struct DeisOp {
    bd_deis_step_desc d;
    template <class V> __device__ __forceinline__ void at(int64_t i) const {
        V e = ld<V>(d.model_output, i), x = ld<V>(d.sample, i);
        V a = splat<V>(0.f), b = a;
        if constexpr (M1) a = ld<V>(d.m1, i);
        if constexpr (M2) b = ld<V>(d.m2, i);
        V m0, p;
        lanes([this](float e, float x, float a, float b, float& m0, float& p) { deis_elem<M1, M2>(d, e, x, a, b, m0, p); }, e, x, a, b, m0, p);
        if (d.m0_out) st<V>(d.m0_out, i, m0);
        st<V>(d.prev_out, i, p);
    }
};
template <bool M1, bool M2>
static void deis_launch(const bd_deis_step_desc& d, hipStream_t stream) {
    const int64_t n4 = d.n / 4, items = n4 + (d.n % 4 != 0);          // the float4s, and one more block-0 pass for the tail
    hipLaunchKernelGGL((vec4_kernel<DeisOp<M1, M2>>), dim3(nblocks(items, TPB, 4096)), dim3(TPB), 0, stream, DeisOp<M1, M2>{d}, n4, d.n);
}


// f-4 (sigma-space samplers: scheduling_heun_discrete.py:193-275, scheduling_lms_discrete.py:217-285, and Euler as their first order):
// one transition in one launch -- pred_original_sample, the ODE derivative exactly as the reference rounds it ((x - x0) / sigma, not
// the model output), Heun's average with the first stage's derivative or the linear multistep sum over the stored derivatives, the
// update from `base` (Heun's second stage restarts from the sample of the first) and the NEXT evaluation's scale_model_input, which
// is what makes the launch worth fusing: every UNet evaluation of these samplers reads x / sqrt(sigma^2 + 1).  The optional inputs are
// template parameters as in UnipcOp (every load one unconditional 16-byte access); NH counts the history terms of the sum
// (AVG reads h1 for the average and has none).
// the two ends every sigma-space element shares (bd_sigma_step, bd_sigma_noise_step): x0 and the derivative, and the closing scale
// into the model's coordinates with the optional clamp there
__device__ __forceinline__ void sigma_deriv(float sigma_in, float e, float x, float& x0, float& dv) {
    x0 = x - sigma_in * e;
    dv = (x - x0) / sigma_in;
}
__device__ __forceinline__ void sigma_scale(float in_div, int clip, float clip_range, float& prev, float& sc) {
    sc = prev / in_div;
    if (clip) {
        sc = fminf(fmaxf(sc, -clip_range), clip_range);
        prev = sc * in_div;
    }
}
template <bool AVG, int NH>
__device__ __forceinline__ void sigma_elem(const bd_sigma_step_desc& d, float e, float x, float b, float h1, float h2, float h3, float& x0,
                                           float& dv, float& prev, float& sc) {
    sigma_deriv(d.sigma_in, e, x, x0, dv);
    float dd = dv;
    if constexpr (AVG) dd = (h1 + dv) / 2.0f;
    float acc = d.c0 * dd;
    if constexpr (!AVG && NH >= 1) acc += d.c1 * h1;
    if constexpr (!AVG && NH >= 2) acc += d.c2 * h2;
    if constexpr (!AVG && NH >= 3) acc += d.c3 * h3;
    prev = b + acc;
    sigma_scale(d.in_div, d.clip, d.clip_range, prev, sc);
}
template <bool AVG, int NH, bool BASE>
struct SigmaOp {
    bd_sigma_step_desc d;
    template <class V> __device__ __forceinline__ void at(int64_t i) const {
        V e = ld<V>(d.model_output, i), x = ld<V>(d.sample, i);
        V b = x, h1 = splat<V>(0.f), h2 = h1, h3 = h1;
        if constexpr (BASE) b = ld<V>(d.base, i);
        if constexpr (AVG || NH >= 1) h1 = ld<V>(d.h1, i);
        if constexpr (!AVG && NH >= 2) h2 = ld<V>(d.h2, i);
        if constexpr (!AVG && NH >= 3) h3 = ld<V>(d.h3, i);
        V x0, dv, p, sc;
        lanes([this](float e, float x, float b, float h1, float h2, float h3, float& x0, float& dv, float& p, float& sc) {
            sigma_elem<AVG, NH>(d, e, x, b, h1, h2, h3, x0, dv, p, sc);
        }, e, x, b, h1, h2, h3, x0, dv, p, sc);
        if (d.x0_out) st<V>(d.x0_out, i, x0);
        if (d.d_out) st<V>(d.d_out, i, dv);
        st<V>(d.prev_out, i, p);
        if (d.scaled_out) st<V>(d.scaled_out, i, sc);
    }
};
template <bool AVG, int NH>
static void sigma_launch(const bd_sigma_step_desc& d, hipStream_t stream) {
    const dim3 grid(nblocks(cdiv(d.n, 4), TPB, 4096));
    if (d.base) hipLaunchKernelGGL((vec4_kernel<SigmaOp<AVG, NH, true>>), grid, dim3(TPB), 0, stream, SigmaOp<AVG, NH, true>{d}, d.n / 4, d.n);
    else hipLaunchKernelGGL((vec4_kernel<SigmaOp<AVG, NH, false>>), grid, dim3(TPB), 0, stream, SigmaOp<AVG, NH, false>{d}, d.n / 4, d.n);
}

// f-4 (the stochastic sigma-space samplers: scheduling_euler_discrete.py:257-354 with churn, scheduling_euler_ancestral_discrete.py:193-281,
// the second stage of scheduling_k_dpm_2_ancestral_discrete.py:243-329): bd_sigma_step's first order transition with a noise term in
// front of it (Euler's churn raises the sample to sigma_hat before anything reads it) or behind it (the ancestral noise lands on the
// updated sample before it is scaled for the next evaluation) -- neither can ride in bd_sigma_step, whose scale follows its update
// directly.  MODE: 0 no noise term (the noise buffer is not read), 1 churn, 2 up.
template <int MODE>
__device__ __forceinline__ void sigma_noise_elem(const bd_sigma_noise_step_desc& d, float e, float x, float z, float b, bool has_base, float& x0,
                                                 float& prev, float& sc) {
    float xh = x;
    if constexpr (MODE == 1) xh = x + (z * d.s_noise) * d.churn_mul;
    float dv;
    sigma_deriv(d.sigma_in, e, xh, x0, dv);
    prev = (has_base ? b : xh) + dv * d.dt;
    if constexpr (MODE == 2) prev = prev + z * d.sigma_up;
    sigma_scale(d.in_div, d.clip, d.clip_range, prev, sc);
}
template <int MODE, bool BASE>
struct SigmaNoiseOp {
    bd_sigma_noise_step_desc d;
    template <class V> __device__ __forceinline__ void at(int64_t i) const {
        V e = ld<V>(d.model_output, i), x = ld<V>(d.sample, i);
        V z = splat<V>(0.f), b = x;
        if constexpr (MODE != 0) z = ld<V>(d.noise, i);
        if constexpr (BASE) b = ld<V>(d.base, i);
        V x0, p, sc;
        lanes([this](float e, float x, float z, float b, float& x0, float& p, float& sc) {
            sigma_noise_elem<MODE>(d, e, x, z, b, BASE, x0, p, sc);
        }, e, x, z, b, x0, p, sc);
        if (d.x0_out) st<V>(d.x0_out, i, x0);
        st<V>(d.prev_out, i, p);
        if (d.scaled_out) st<V>(d.scaled_out, i, sc);
    }
};
// the launch shape of the vec4 driver: a thread per float4, at most 4096 blocks (the loop strides over the rest)
static dim3 vec4_grid(int64_t elems) { return dim3(nblocks(cdiv(elems, 4), TPB, 4096)); }
template <int MODE>
static void sigma_noise_launch(const bd_sigma_noise_step_desc& d, hipStream_t stream) {
    const dim3 grid = vec4_grid(d.n);
    if (d.base) hipLaunchKernelGGL((vec4_kernel<SigmaNoiseOp<MODE, true>>), grid, dim3(TPB), 0, stream, SigmaNoiseOp<MODE, true>{d}, d.n / 4, d.n);
    else hipLaunchKernelGGL((vec4_kernel<SigmaNoiseOp<MODE, false>>), grid, dim3(TPB), 0, stream, SigmaNoiseOp<MODE, false>{d}, d.n / 4, d.n);
}

// out = (x * mul) / div: the start of a sigma-space chain (init * init_noise_sigma, then / sqrt(sigma_0^2 + 1)) and the public
// scale_model_input (mul = 1: x * 1 is x).  out may be x.
struct ScaleInputOp {
    const float* x; float mul, div; float* out;
    template <class V> __device__ __forceinline__ void at(int64_t i) const {
        V v = ld<V>(x, i);
        lanes([this](float& v) { v = (v * mul) / div; }, v);
        st<V>(out, i, v);
    }
};


// ---- f-4: Adversarial Neuron Pruning (anp_model.py:490-514 PerturbConv2d = conv followed by an eval-mode batch norm with mean 0, variance 1,
// eps 0, i.e. y_c <- w_c * conv(x; W, b)_c + b_c with ONE learnable (w_c, b_c) per output channel).  The affine map commutes with the convolution:
//   w_c * (W_c . x + b_c0) + b_c = (w_c W_c) . x + (w_c b_c0 + b_c),
// so the perturbed network IS the ordinary network on effective weights (anp_apply: one scaled copy of every conv weight row and bias), and the
// gradient of the perturbation is a row-wise contraction of the ordinary weight gradient (anp_grad):
//   dL/dw_c = sum_k dL/dW'_ck W_ck + dL/db'_c b_c0 ,   dL/db_c = dL/db'_c.
// items: [n][5] int64 = (weight offset, bias offset or -1, Cout, row length, offset of the layer's channels in the perturbation vectors);
// one workgroup per output channel of every convolution, fixed-order fold (deterministic).
__device__ __forceinline__ void anp_locate(const int64_t* __restrict__ items, int n, int64_t row, int64_t& woff, int64_t& boff, int64_t& len,
                                           int64_t& p) {
    int64_t base = 0;
    woff = boff = -1; len = 0; p = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t cout = items[i * 5 + 2];
        if (row < base + cout) {
            const int64_t c = row - base;
            len = items[i * 5 + 3];
            woff = items[i * 5 + 0] + c * len;
            boff = items[i * 5 + 1] < 0 ? -1 : items[i * 5 + 1] + c;
            p = items[i * 5 + 4] + c;
            return;
        }
        base += cout;
    }
}
__global__ __launch_bounds__(TPB) void anp_apply_kernel(const float* __restrict__ params, const float* __restrict__ pw,
                                                        const float* __restrict__ pb, const int64_t* __restrict__ items, int n,
                                                        float* __restrict__ eff) {
    int64_t woff, boff, len, p;
    anp_locate(items, n, blockIdx.x, woff, boff, len, p);
    if (woff < 0) return;
    const float w = pw[p];
    for (int64_t k = threadIdx.x; k < len; k += TPB) eff[woff + k] = w * params[woff + k];
    if (threadIdx.x == 0 && boff >= 0) eff[boff] = w * params[boff] + pb[p];
}
// row_norm (optional): the norm of the gradient of the layer's OWN weight row and bias in the perturbed network, |w_c| * ||(dL/dW'_c, dL/db'_c)|| --
// the reference's clip_grad_norm_ runs over them too (PerturbConv2d's weights are fresh, trainable Parameters: anp_model.py:492-505)
__global__ __launch_bounds__(TPB) void anp_grad_kernel(const float* __restrict__ params, const float* __restrict__ geff,
                                                       const int64_t* __restrict__ items, int n, const float* __restrict__ pw,
                                                       float* __restrict__ gw, float* __restrict__ gb, float* __restrict__ row_norm) {
    __shared__ float red[TPB / 64][2];
    int64_t woff, boff, len, p;
    anp_locate(items, n, blockIdx.x, woff, boff, len, p);
    if (woff < 0) return;
    float a = 0.f, q = 0.f;
    for (int64_t k = threadIdx.x; k < len; k += TPB) {
        const float g = geff[woff + k];
        a += g * params[woff + k];
        q += g * g;
    }
    a = wave_sum(a); q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a; red[threadIdx.x >> 6][1] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f, tq = 0.f;
#pragma unroll
        for (int i = 0; i < TPB / 64; ++i) { t += red[i][0]; tq += red[i][1]; }
        const float g = boff >= 0 ? geff[boff] : 0.f;
        gw[p] = t + (boff >= 0 ? g * params[boff] : 0.f);
        gb[p] = g;
        if (row_norm) row_norm[p] = fabsf(pw[p]) * sqrtf(tq + g * g);
    }
}

// step_buffers_bad (step_check.h) with the message of its first violation, for the entry points that name their operands
static int step_buffers_check(const char* who, int64_t n, const StepBuf* in, int n_in, const StepBuf* out, int n_out) {
    const StepViolation v = step_buffers_bad(n, in, n_in, out, n_out);
    BD_CHECK(v.code != STEP_MISALIGNED, BD_ERR_INVALID, "%s: %s is not 16-byte aligned", who, (v.a < n_in ? in[v.a] : out[v.a - n_in]).name);
    BD_CHECK(v.code != STEP_OUT_OUT, BD_ERR_INVALID, "%s: %s overlaps %s", who, out[v.a].name, out[v.b].name);
    BD_CHECK(v.code != STEP_OUT_IN, BD_ERR_INVALID, "%s: %s overlaps %s without being the same buffer", who, out[v.a].name, in[v.b].name);
    return BD_OK;
}

}  // namespace bd

using namespace bd;

extern "C" const char* bd_last_error(void) { return g_err.c_str(); }
extern "C" int bd_version(void) { return 1; }

// the host checks of the two fused q_sample entry points; `coef` is the table the kernel reads the target's coefficient from
// (alphas, or corr for the *_corr entry points, which do not read alphas)
template <class D>
static int poison_qsample_check(const char* who, const D* d, const float* coef) {
    BD_CHECK(d->B > 0 && d->C > 0 && d->H > 0 && d->W > 0, BD_ERR_INVALID, "%s: bad shape", who);
    BD_CHECK((d->images_f32 != nullptr) != (d->images_u8 != nullptr), BD_ERR_INVALID,
             "%s: exactly one of images_f32 / images_u8 must be given", who);
    BD_CHECK(d->is_poison && d->trigger && d->target_img && d->noise && d->timesteps && coef && d->alphas_cumprod &&
                 d->x_noisy && d->target, BD_ERR_INVALID, "%s: null pointer", who);
    BD_CHECK(d->ld_noisy >= d->C && d->ld_target >= d->C, BD_ERR_INVALID, "%s: ld < C", who);
    return BD_OK;
}
template <class D>
static int qsample_check(const char* who, const D* d, const float* coef) {
    BD_CHECK(d->B > 0 && d->C > 0 && d->H > 0 && d->W > 0, BD_ERR_INVALID, "%s: bad shape", who);
    BD_CHECK(d->x0 && d->R && d->noise && d->timesteps && coef && d->alphas_cumprod && d->x_noisy && d->target,
             BD_ERR_INVALID, "%s: null pointer", who);
    BD_CHECK(d->ld_noisy >= d->C && d->ld_target >= d->C, BD_ERR_INVALID, "%s: ld < C", who);
    return BD_OK;
}

extern "C" int bd_poison_qsample(const bd_poison_qsample_desc* d, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_poison_qsample: null descriptor");
    if (int st = poison_qsample_check("bd_poison_qsample", d, d->alphas)) return st;
    hipLaunchKernelGGL(poison_qsample_kernel, dim3(nblocks((int64_t)d->B * d->H * d->W)), dim3(TPB), 0, S(stream), *d);
    BD_LAUNCH_CHECK("poison_qsample");
    return BD_OK;
}
extern "C" int bd_poison_qsample_corr(const bd_poison_qsample_corr_desc* d, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_poison_qsample_corr: null descriptor");
    BD_CHECK(d->corr, BD_ERR_INVALID, "bd_poison_qsample_corr: null corr table");
    if (int st = poison_qsample_check("bd_poison_qsample_corr", d, d->corr)) return st;
    hipLaunchKernelGGL(poison_qsample_corr_kernel, dim3(nblocks((int64_t)d->B * d->H * d->W)), dim3(TPB), 0, S(stream), *d);
    BD_LAUNCH_CHECK("poison_qsample_corr");
    return BD_OK;
}
extern "C" int bd_qsample(const bd_qsample_desc* d, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_qsample: null descriptor");
    if (int st = qsample_check("bd_qsample", d, d->alphas)) return st;
    hipLaunchKernelGGL(qsample_kernel, dim3(nblocks((int64_t)d->B * d->H * d->W)), dim3(TPB), 0, S(stream), *d);
    BD_LAUNCH_CHECK("qsample");
    return BD_OK;
}
extern "C" int bd_qsample_corr(const bd_qsample_corr_desc* d, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_qsample_corr: null descriptor");
    BD_CHECK(d->corr, BD_ERR_INVALID, "bd_qsample_corr: null corr table");
    if (int st = qsample_check("bd_qsample_corr", d, d->corr)) return st;
    hipLaunchKernelGGL(qsample_corr_kernel, dim3(nblocks((int64_t)d->B * d->H * d->W)), dim3(TPB), 0, S(stream), *d);
    BD_LAUNCH_CHECK("qsample_corr");
    return BD_OK;
}
extern "C" int bd_nchw_to_nhwc(const float* src, float* dst, int B, int C, int H, int W, int64_t ld, bd_stream_t stream) {
    BD_CHECK(src && dst && B > 0 && C > 0 && H > 0 && W > 0 && ld >= C, BD_ERR_INVALID, "bd_nchw_to_nhwc: bad args");
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(nblocks((int64_t)B * H * W)), dim3(TPB), 0, S(stream), src, dst, B, C,
                       (int64_t)H * W, ld);
    BD_LAUNCH_CHECK("nchw_to_nhwc");
    return BD_OK;
}
extern "C" int bd_nhwc_to_nchw(const float* src, int64_t ld, float* dst, int B, int C, int H, int W, bd_stream_t stream) {
    BD_CHECK(src && dst && B > 0 && C > 0 && H > 0 && W > 0 && ld >= C, BD_ERR_INVALID, "bd_nhwc_to_nchw: bad args");
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(nblocks((int64_t)B * H * W)), dim3(TPB), 0, S(stream), src, ld, dst, B, C,
                       (int64_t)H * W);
    BD_LAUNCH_CHECK("nhwc_to_nchw");
    return BD_OK;
}
extern "C" int bd_ddpm_step(const bd_ddpm_step_desc* d, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_ddpm_step: null descriptor");
    BD_CHECK(d->n > 0 && d->model_output && d->sample && d->prev_sample && d->alphas_cumprod, BD_ERR_INVALID,
             "bd_ddpm_step: bad args");
    BD_CHECK(d->t >= 0, BD_ERR_INVALID, "bd_ddpm_step: t < 0");
    BD_CHECK(d->t == 0 || d->noise, BD_ERR_INVALID, "bd_ddpm_step: noise is required when t > 0");
    BD_CHECK(d->variance_type == 0 || d->variance_type == 1, BD_ERR_UNSUPPORTED,
             "bd_ddpm_step: variance_type must be fixed_small(0) or fixed_large(1)");
    if (d->x0_quantile) {
        BD_CHECK(d->image_elems > 0 && d->n % d->image_elems == 0, BD_ERR_INVALID,
                 "bd_ddpm_step: x0_quantile with n=%lld that is no multiple of image_elems=%lld", (long long)d->n, (long long)d->image_elems);
        BD_CHECK(d->n < ((int64_t)1 << 31), BD_ERR_INVALID, "bd_ddpm_step: x0_quantile with n=%lld >= 2^31", (long long)d->n);
        hipLaunchKernelGGL((ddpm_step_kernel<true>), dim3(nblocks(d->n, TPB, 4096)), dim3(TPB), 0, S(stream), *d);
    } else {
        hipLaunchKernelGGL((ddpm_step_kernel<false>), dim3(nblocks(d->n, TPB, 4096)), dim3(TPB), 0, S(stream), *d);
    }
    BD_LAUNCH_CHECK("ddpm_step");
    return BD_OK;
}
namespace bd {
static int aq_plan(const char* who, int B, int64_t m, bd_abs_quantile_plan_info* p) {
    BD_CHECK(B > 0, BD_ERR_INVALID, "%s: B=%d must be positive", who, B);
    BD_CHECK(m > 0, BD_ERR_INVALID, "%s: m=%lld must be positive", who, (long long)m);
    BD_CHECK(m < ((int64_t)1 << 31) && (int64_t)B * m < ((int64_t)1 << 31), BD_ERR_INVALID, "%s: B * m = %d * %lld must stay below 2^31", who, B,
             (long long)m);
    p->path = m <= AQ_REG_MAX ? BD_AQ_REGISTERS : BD_AQ_STREAM;
    p->workgroups = B;
    p->threads = p->path == BD_AQ_REGISTERS ? AQ_REG_THREADS : AQ_STREAM_THREADS;
    p->values_per_thread = p->path == BD_AQ_REGISTERS ? AQ_REG_VPT : (int)cdiv(m, (int64_t)AQ_STREAM_THREADS);
    p->passes = 3;
    p->switch_m = AQ_REG_MAX;
    p->workspace_bytes = 0;
    return BD_OK;
}
}  // namespace bd
extern "C" int bd_abs_quantile_plan(int B, int64_t m, bd_abs_quantile_plan_info* out) {
    BD_CHECK(out, BD_ERR_INVALID, "bd_abs_quantile_plan: null output");
    return aq_plan("bd_abs_quantile_plan", B, m, out);
}
extern "C" size_t bd_abs_quantile_workspace_bytes(int B, int64_t m) {
    (void)B; (void)m;
    return 0;                                     // neither path of today keeps anything outside its workgroup
}
extern "C" int bd_abs_quantile(const bd_abs_quantile_desc* d, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_abs_quantile: null descriptor");
    BD_CHECK(d->x && d->out, BD_ERR_INVALID, "bd_abs_quantile: null pointer (x and out are required)");
    bd_abs_quantile_plan_info p;
    BD_TRY(aq_plan("bd_abs_quantile", d->B, d->m, &p));
    BD_CHECK(d->q >= 0.f && d->q <= 1.f, BD_ERR_INVALID, "bd_abs_quantile: q=%g must lie in [0, 1]", (double)d->q);     // false for a NaN
    BD_CHECK(d->workspace_bytes >= p.workspace_bytes && (d->workspace || !p.workspace_bytes), BD_ERR_INVALID,
             "bd_abs_quantile: workspace of %zu bytes, %zu needed", d->workspace_bytes, p.workspace_bytes);
    if (d->model_output) {
        BD_CHECK(d->alphas_cumprod, BD_ERR_INVALID, "bd_abs_quantile: model_output without alphas_cumprod");
        BD_CHECK(d->t >= 0 && d->t < d->n_alphas, BD_ERR_INVALID, "bd_abs_quantile: t=%d outside the table of %d", d->t, d->n_alphas);
    }
    // torch.quantile's ranks, in fp32: rank = q * (m - 1), below = floor, above = ceil, weight = rank - below
    const float last = (float)(d->m - 1);
    const float rank = d->q * last;
    const float below = floorf(rank);
    AqArgs a;
    a.x = d->x; a.e = d->model_output; a.alphas_cumprod = d->alphas_cumprod; a.t = d->t; a.m = d->m; a.out = d->out;
    a.w = rank - below;
    int64_t lo = (int64_t)below;
    if (lo > d->m - 1) lo = d->m - 1;             // (float)(m - 1) may round up past m - 1 above 2^24
    int64_t hi = lo + (a.w > 0.f ? 1 : 0);
    if (hi > d->m - 1) hi = d->m - 1;
    a.lo = (unsigned)lo; a.hi = (unsigned)hi;
    if (p.path == BD_AQ_REGISTERS)
        hipLaunchKernelGGL((abs_quantile_kernel<AQ_REG_THREADS, AQ_REG_VPT>), dim3((unsigned)d->B), dim3(AQ_REG_THREADS), 0, S(stream), a);
    else
        hipLaunchKernelGGL((abs_quantile_kernel<AQ_STREAM_THREADS, 0>), dim3((unsigned)d->B), dim3(AQ_STREAM_THREADS), 0, S(stream), a);
    BD_LAUNCH_CHECK("abs_quantile");
    return BD_OK;
}
extern "C" int bd_lincomb(int k, const float* const* terms, const float* coeffs, int64_t n, int clip, float clip_range, float* out,
                          bd_stream_t stream) {
    BD_CHECK(k >= 1 && k <= BD_LINCOMB_MAX && terms && coeffs && out && n > 0, BD_ERR_INVALID, "bd_lincomb: bad args (k=%d)", k);
    LincombOp a = {};
    a.k = k; a.clip = clip; a.range = clip_range; a.out = out;
    StepBuf in[BD_LINCOMB_MAX];
    for (int j = 0; j < k; ++j) {
        BD_CHECK(terms[j] && aligned16(terms[j]), BD_ERR_INVALID, "bd_lincomb: term %d is null or not 16-byte aligned", j);
        a.t[j] = terms[j]; a.c[j] = coeffs[j];
        in[j] = {terms[j], "term"};
    }
    const StepBuf o = {out, "out"};
    const StepViolation v = step_buffers_bad(n, in, k, &o, 1);
    BD_CHECK(v.code != STEP_MISALIGNED, BD_ERR_INVALID, "bd_lincomb: out must be 16-byte aligned");
    BD_CHECK(v.code == STEP_OK, BD_ERR_INVALID, "bd_lincomb: out overlaps term %d without being the same buffer", v.b);
    hipLaunchKernelGGL(lincomb_kernel, dim3(nblocks(cdiv(n, 4), TPB, 4096)), dim3(TPB), 0, S(stream), a, n / 4, n);
    BD_LAUNCH_CHECK("lincomb");
    return BD_OK;
}
extern "C" int bd_dpm_step(const bd_dpm_step_desc* d, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_dpm_step: null descriptor");
    BD_CHECK(d->n > 0, BD_ERR_INVALID, "bd_dpm_step: n=%lld must be positive", (long long)d->n);
    BD_CHECK(d->model_output && d->sample && d->prev_out, BD_ERR_INVALID,
             "bd_dpm_step: null pointer (model_output, sample and prev_out are required)");
    const StepBuf in[4] = {{d->model_output, "model_output"}, {d->sample, "sample"}, {d->m1, "m1"}, {d->m2, "m2"}};
    const StepBuf out[2] = {{d->prev_out, "prev_out"}, {d->m0_out, "m0_out"}};
    BD_TRY(step_buffers_check("bd_dpm_step", d->n, in, 4, out, 2));
    hipLaunchKernelGGL(vec4_kernel<DpmOp>, dim3(nblocks(cdiv(d->n, 4), TPB, 4096)), dim3(TPB), 0, S(stream), DpmOp{*d}, d->n / 4, d->n);
    BD_LAUNCH_CHECK("dpm_step");
    return BD_OK;
}
extern "C" int bd_unipc_step(const bd_unipc_step_desc* d, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_unipc_step: null descriptor");
    BD_CHECK(d->n > 0, BD_ERR_INVALID, "bd_unipc_step: n=%lld must be positive", (long long)d->n);
    BD_CHECK(d->model_output && d->sample && d->prev_out, BD_ERR_INVALID,
             "bd_unipc_step: null pointer (model_output, sample and prev_out are required)");
    BD_CHECK(!d->last_sample || d->h1, BD_ERR_INVALID, "bd_unipc_step: last_sample without h1 (the corrector reads the previous converted output)");
    const StepBuf in[6] = {{d->model_output, "model_output"}, {d->sample, "sample"}, {d->last_sample, "last_sample"},
                           {d->h1, "h1"}, {d->h2, "h2"}, {d->h3, "h3"}};
    const StepBuf out[3] = {{d->prev_out, "prev_out"}, {d->m0_out, "m0_out"}, {d->corrected_out, "corrected_out"}};
    BD_TRY(step_buffers_check("bd_unipc_step", d->n, in, 6, out, 3));
    // instance by the conversion and by which optional inputs are present: bit 4 convert, bit 3 last_sample, bits 2..0 h1, h2, h3
    // (last_sample without h1 was refused above)
    const int instance = (d->convert ? 16 : 0) | (d->last_sample ? 8 : 0) | (d->h1 ? 4 : 0) | (d->h2 ? 2 : 0) | (d->h3 ? 1 : 0);
    switch (instance) {
#define BD_UNIPC_CASE(M)                                                                                                          \
    case M: unipc_launch<((M) & 16) != 0, ((M) & 8) != 0, ((M) & 4) != 0, ((M) & 2) != 0, ((M) & 1) != 0>(*d, S(stream)); break;  \
    case (M) + 16: unipc_launch<true, ((M) & 8) != 0, ((M) & 4) != 0, ((M) & 2) != 0, ((M) & 1) != 0>(*d, S(stream)); break;
        BD_UNIPC_CASE(0) BD_UNIPC_CASE(1) BD_UNIPC_CASE(2) BD_UNIPC_CASE(3) BD_UNIPC_CASE(4) BD_UNIPC_CASE(5) BD_UNIPC_CASE(6)
        BD_UNIPC_CASE(7) BD_UNIPC_CASE(12) BD_UNIPC_CASE(13) BD_UNIPC_CASE(14) BD_UNIPC_CASE(15)
#undef BD_UNIPC_CASE
        default: BD_CHECK(false, BD_ERR_INVALID, "bd_unipc_step: last_sample without h1");
    }
    BD_LAUNCH_CHECK("unipc_step");
    return BD_OK;
}
extern "C" int bd_deis_step(const bd_deis_step_desc* d, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_deis_step: null descriptor");
    BD_CHECK(d->n > 0, BD_ERR_INVALID, "bd_deis_step: n=%lld must be positive", (long long)d->n);
    BD_CHECK(d->model_output && d->sample && d->prev_out, BD_ERR_INVALID,
             "bd_deis_step: null pointer (model_output, sample and prev_out are required)");
    BD_CHECK(d->alpha_s > 0.f, BD_ERR_INVALID, "bd_deis_step: alpha_s=%g must be positive", (double)d->alpha_s);
    BD_CHECK(d->sigma_s > 0.f, BD_ERR_INVALID, "bd_deis_step: sigma_s=%g must be positive", (double)d->sigma_s);
    BD_CHECK(d->m1 || !d->m2, BD_ERR_INVALID, "bd_deis_step: m2 without m1 (the history has no gap)");
    const StepBuf in[4] = {{d->model_output, "model_output"}, {d->sample, "sample"}, {d->m1, "m1"}, {d->m2, "m2"}};
    const StepBuf out[2] = {{d->prev_out, "prev_out"}, {d->m0_out, "m0_out"}};
    BD_TRY(step_buffers_check("bd_deis_step", d->n, in, 4, out, 2));
    if (d->m2) deis_launch<true, true>(*d, S(stream));
    else if (d->m1) deis_launch<true, false>(*d, S(stream));
    else deis_launch<false, false>(*d, S(stream));
    BD_LAUNCH_CHECK("deis_step");
    return BD_OK;
}
extern "C" int bd_sigma_step(const bd_sigma_step_desc* d, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_sigma_step: null descriptor");
    BD_CHECK(d->n > 0, BD_ERR_INVALID, "bd_sigma_step: n=%lld must be positive", (long long)d->n);
    BD_CHECK(d->model_output && d->sample && d->prev_out, BD_ERR_INVALID,
             "bd_sigma_step: null pointer (model_output, sample and prev_out are required)");
    BD_CHECK(d->sigma_in > 0.f, BD_ERR_INVALID, "bd_sigma_step: sigma_in=%g must be positive", (double)d->sigma_in);
    BD_CHECK(d->in_div > 0.f, BD_ERR_INVALID, "bd_sigma_step: in_div=%g must be positive", (double)d->in_div);
    BD_CHECK(!d->average || d->h1, BD_ERR_INVALID, "bd_sigma_step: average without h1 (the first stage's derivative)");
    BD_CHECK(!d->average || (!d->h2 && !d->h3 && d->c1 == 0.f && d->c2 == 0.f && d->c3 == 0.f), BD_ERR_INVALID,
             "bd_sigma_step: average with history terms (h2 / h3 or a non-zero c1 / c2 / c3)");
    BD_CHECK((d->h1 || !d->h2) && (d->h2 || !d->h3), BD_ERR_INVALID, "bd_sigma_step: history with a gap (h2 without h1, or h3 without h2)");
    const StepBuf in[6] = {{d->model_output, "model_output"}, {d->sample, "sample"}, {d->base, "base"}, {d->h1, "h1"}, {d->h2, "h2"}, {d->h3, "h3"}};
    const StepBuf out[4] = {{d->prev_out, "prev_out"}, {d->x0_out, "x0_out"}, {d->d_out, "d_out"}, {d->scaled_out, "scaled_out"}};
    BD_TRY(step_buffers_check("bd_sigma_step", d->n, in, 6, out, 4));
    if (d->average) sigma_launch<true, 0>(*d, S(stream));
    else if (d->h3) sigma_launch<false, 3>(*d, S(stream));
    else if (d->h2) sigma_launch<false, 2>(*d, S(stream));
    else if (d->h1) sigma_launch<false, 1>(*d, S(stream));
    else sigma_launch<false, 0>(*d, S(stream));
    BD_LAUNCH_CHECK("sigma_step");
    return BD_OK;
}
extern "C" int bd_sigma_noise_step(const bd_sigma_noise_step_desc* d, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_sigma_noise_step: null descriptor");
    BD_CHECK(d->n > 0, BD_ERR_INVALID, "bd_sigma_noise_step: n=%lld must be positive", (long long)d->n);
    BD_CHECK(d->model_output && d->sample && d->noise && d->prev_out, BD_ERR_INVALID,
             "bd_sigma_noise_step: null pointer (model_output, sample, noise and prev_out are required)");
    BD_CHECK(d->sigma_in > 0.f, BD_ERR_INVALID, "bd_sigma_noise_step: sigma_in=%g must be positive", (double)d->sigma_in);
    BD_CHECK(d->in_div > 0.f, BD_ERR_INVALID, "bd_sigma_noise_step: in_div=%g must be positive", (double)d->in_div);
    BD_CHECK(d->sigma_up >= 0.f, BD_ERR_INVALID, "bd_sigma_noise_step: sigma_up=%g must not be negative", (double)d->sigma_up);
    BD_CHECK(!(d->churn && d->up), BD_ERR_INVALID, "bd_sigma_noise_step: churn together with up (no sampler has both noise terms)");
    BD_CHECK(!d->churn || d->churn_mul > 0.f, BD_ERR_INVALID, "bd_sigma_noise_step: churn with churn_mul=%g, which must be positive",
             (double)d->churn_mul);
    const StepBuf in[4] = {{d->model_output, "model_output"}, {d->sample, "sample"}, {d->noise, "noise"}, {d->base, "base"}};
    const StepBuf out[3] = {{d->prev_out, "prev_out"}, {d->x0_out, "x0_out"}, {d->scaled_out, "scaled_out"}};
    // step_buffers_check lets any output be any input's own buffer; here only prev_out == sample is
    for (int o = 0; o < 3; ++o)
        for (int j = 0; j < 4; ++j)
            BD_CHECK(!out[o].p || out[o].p != in[j].p || (o == 0 && out[o].p == d->sample), BD_ERR_INVALID,
                     "bd_sigma_noise_step: %s is the buffer of %s (only prev_out may be an input's buffer, and only sample's)", out[o].name,
                     in[j].name);
    BD_TRY(step_buffers_check("bd_sigma_noise_step", d->n, in, 4, out, 3));
    if (d->churn) sigma_noise_launch<1>(*d, S(stream));
    else if (d->up) sigma_noise_launch<2>(*d, S(stream));
    else sigma_noise_launch<0>(*d, S(stream));
    BD_LAUNCH_CHECK("sigma_noise_step");
    return BD_OK;
}
extern "C" int bd_scale_input(const float* x, int64_t n, float mul, float div, float* out, bd_stream_t stream) {
    BD_CHECK(x && out, BD_ERR_INVALID, "bd_scale_input: null pointer");
    BD_CHECK(n > 0, BD_ERR_INVALID, "bd_scale_input: n=%lld must be positive", (long long)n);
    BD_CHECK(div > 0.f, BD_ERR_INVALID, "bd_scale_input: div=%g must be positive", (double)div);
    const StepBuf in = {x, "x"}, o = {out, "out"};
    const StepViolation v = step_buffers_bad(n, &in, 1, &o, 1);
    BD_CHECK(v.code != STEP_MISALIGNED, BD_ERR_INVALID, "bd_scale_input: x and out must be 16-byte aligned");
    BD_CHECK(v.code == STEP_OK, BD_ERR_INVALID, "bd_scale_input: out overlaps x without being the same buffer");
    hipLaunchKernelGGL(vec4_kernel<ScaleInputOp>, dim3(nblocks(cdiv(n, 4), TPB, 4096)), dim3(TPB), 0, S(stream),
                       ScaleInputOp{x, mul, div, out}, n / 4, n);
    BD_LAUNCH_CHECK("scale_input");
    return BD_OK;
}
extern "C" int bd_ddim_step(const bd_ddim_step_desc* d, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_ddim_step: null descriptor");
    BD_CHECK(d->n > 0 && d->model_output && d->sample && d->prev_sample && d->alphas_cumprod, BD_ERR_INVALID,
             "bd_ddim_step: bad args");
    BD_CHECK(d->t >= 0, BD_ERR_INVALID, "bd_ddim_step: t < 0");
    BD_CHECK(d->eta == 0.f || d->noise, BD_ERR_INVALID, "bd_ddim_step: noise is required when eta > 0");
    if (d->x0_quantile) {
        BD_CHECK(d->image_elems > 0 && d->n % d->image_elems == 0, BD_ERR_INVALID,
                 "bd_ddim_step: x0_quantile with n=%lld that is no multiple of image_elems=%lld", (long long)d->n, (long long)d->image_elems);
        BD_CHECK(d->n < ((int64_t)1 << 31), BD_ERR_INVALID, "bd_ddim_step: x0_quantile with n=%lld >= 2^31", (long long)d->n);
        hipLaunchKernelGGL((ddim_step_kernel<true>), dim3(nblocks(d->n, TPB, 4096)), dim3(TPB), 0, S(stream), *d);
    } else {
        hipLaunchKernelGGL((ddim_step_kernel<false>), dim3(nblocks(d->n, TPB, 4096)), dim3(TPB), 0, S(stream), *d);
    }
    BD_LAUNCH_CHECK("ddim_step");
    return BD_OK;
}
namespace bd {
// Storage order of a dense [N,C,H,W] layout: perm[0] outermost .. perm[3] innermost (size-1 dimensions, whose strides mean nothing,
// go first).  False when `stride` is not dense: some stride differs from the product of the sizes inside it.
static bool rp_storage_order(const int (&size)[4], const int64_t (&stride)[4], int (&perm)[4]) {
    int n1 = 0, rest[4], nr = 0;
    for (int i = 0; i < 4; ++i) {
        if (size[i] == 1) perm[n1++] = i;
        else rest[nr++] = i;
    }
    for (int a = 1; a < nr; ++a)        // descending stride
        for (int b = a; b > 0 && stride[rest[b]] > stride[rest[b - 1]]; --b) { const int t = rest[b]; rest[b] = rest[b - 1]; rest[b - 1] = t; }
    int64_t expect = 1;
    for (int a = nr - 1; a >= 0; --a) {
        if (stride[rest[a]] != expect) return false;
        expect *= size[rest[a]];
    }
    for (int a = 0; a < nr; ++a) perm[n1 + a] = rest[a];
    return true;
}
// the checks and the geometry both RePaint entry points share; strides of an absent broadcast operand may be NULL
static int rp_geometry(const char* who, int N, int C, int H, int W, const int64_t (&stride)[4], const int64_t* os, const int64_t* ms,
                       const int64_t* ss, RpGeom& g) {
    BD_CHECK(N > 0 && C > 0 && H > 0 && W > 0, BD_ERR_INVALID, "%s: N=%d C=%d H=%d W=%d must be positive", who, N, C, H, W);
    for (int i = 0; i < 4; ++i)
        BD_CHECK(stride[i] >= 0 && (!os || os[i] >= 0) && (!ms || ms[i] >= 0) && (!ss || ss[i] >= 0), BD_ERR_INVALID,
                 "%s: negative stride at dim %d", who, i);
    const int size[4] = {N, C, H, W};
    int perm[4];
    BD_CHECK(rp_storage_order(size, stride, perm), BD_ERR_INVALID,
             "%s: stride (%lld, %lld, %lld, %lld) is not a dense layout of [%d,%d,%d,%d]", who, (long long)stride[0], (long long)stride[1],
             (long long)stride[2], (long long)stride[3], N, C, H, W);
    g.n = (int64_t)N * C * H * W;
    BD_CHECK(g.n < ((int64_t)1 << 31), BD_ERR_UNSUPPORTED, "%s: %lld elements (2^31 and more are not supported)", who, (long long)g.n);
    for (int j = 0; j < 4; ++j) {
        g.sz[j] = (unsigned)size[perm[j]];
        g.os[j] = os ? os[perm[j]] : 0; g.ms[j] = ms ? ms[perm[j]] : 0; g.ss[j] = ss ? ss[perm[j]] : 0;
    }
    return BD_OK;
}
constexpr int64_t RP_MAX_BLOCKS = 2048;
}  // namespace bd

extern "C" int bd_repaint_step(const bd_repaint_step_desc* d, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_repaint_step: null descriptor");
    BD_CHECK(d->model_output && d->sample && d->noise && d->prev_sample && d->original_image && d->mask && d->alphas_cumprod,
             BD_ERR_INVALID, "bd_repaint_step: null pointer (model_output, sample, noise, prev_sample, original_image, mask and "
             "alphas_cumprod are required)");
    BD_CHECK(d->t >= 0, BD_ERR_INVALID, "bd_repaint_step: t=%d < 0", d->t);
    BD_CHECK(d->t < d->n_alphas && d->prev_t < d->n_alphas, BD_ERR_INVALID, "bd_repaint_step: t=%d / prev_t=%d outside the table of %d",
             d->t, d->prev_t, d->n_alphas);
    RpGeom g;
    BD_TRY(rp_geometry("bd_repaint_step", d->N, d->C, d->H, d->W, d->stride, d->orig_stride, d->mask_stride,
                       d->shift ? d->shift_stride : nullptr, g));
    const bool vec = (g.n & 3) == 0 && aligned16(d->model_output) && aligned16(d->sample) && aligned16(d->noise) &&
                     aligned16(d->prev_sample) && aligned16(d->pred_original);
    const dim3 grid(nblocks(vec ? g.n >> 2 : g.n, TPB, RP_MAX_BLOCKS)), block(TPB);
    if (vec) hipLaunchKernelGGL(repaint_step_kernel<true>, grid, block, 0, S(stream), *d, g);
    else hipLaunchKernelGGL(repaint_step_kernel<false>, grid, block, 0, S(stream), *d, g);
    BD_LAUNCH_CHECK("repaint_step");
    return BD_OK;
}

extern "C" int bd_repaint_undo(const bd_repaint_undo_desc* d, const float* const* noises, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_repaint_undo: null descriptor");
    BD_CHECK(d->sample && d->out && d->betas && noises, BD_ERR_INVALID,
             "bd_repaint_undo: null pointer (sample, out, betas and noises are required)");
    BD_CHECK(d->k >= 1, BD_ERR_INVALID, "bd_repaint_undo: k=%d < 1", d->k);
    BD_CHECK(d->t >= 0, BD_ERR_INVALID, "bd_repaint_undo: t=%d < 0", d->t);
    BD_CHECK((int64_t)d->t + d->k <= d->n_betas, BD_ERR_INVALID, "bd_repaint_undo: t + k = %d + %d exceeds the table of %d", d->t, d->k,
             d->n_betas);
    RpGeom g;
    BD_TRY(rp_geometry("bd_repaint_undo", d->N, d->C, d->H, d->W, d->stride, nullptr, nullptr, d->shift ? d->shift_stride : nullptr, g));
    bool vec = (g.n & 3) == 0 && aligned16(d->sample) && aligned16(d->out);
    for (int j = 0; j < d->k; ++j) {
        BD_CHECK(noises[j], BD_ERR_INVALID, "bd_repaint_undo: noises[%d] is null", j);
        vec = vec && aligned16(noises[j]);
    }
    const dim3 grid(nblocks(vec ? g.n >> 2 : g.n, TPB, RP_MAX_BLOCKS)), block(TPB);
    for (int j0 = 0; j0 < d->k; j0 += BD_REPAINT_UNDO_MAX) {       // one path for every chunk: same kernel, same bits
        RpUndoArgs a = {};
        a.k = d->k - j0 < BD_REPAINT_UNDO_MAX ? d->k - j0 : BD_REPAINT_UNDO_MAX;
        for (int j = 0; j < a.k; ++j) a.z[j] = noises[j0 + j];
        a.x = j0 == 0 ? d->sample : d->out; a.out = d->out; a.shift = d->shift; a.betas = d->betas; a.t = d->t + j0;
        if (vec) hipLaunchKernelGGL(repaint_undo_kernel<true>, grid, block, 0, S(stream), a, g);
        else hipLaunchKernelGGL(repaint_undo_kernel<false>, grid, block, 0, S(stream), a, g);
        BD_LAUNCH_CHECK("repaint_undo");
    }
    return BD_OK;
}

extern "C" int bd_to_image(const float* x, int src_is_nhwc, int64_t ld, int B, int C, int H, int W, float* out_f32,
                           uint8_t* out_u8, bd_stream_t stream) {
    BD_CHECK(x && (out_f32 || out_u8) && B > 0 && C > 0 && H > 0 && W > 0, BD_ERR_INVALID, "bd_to_image: bad args");
    BD_CHECK(!src_is_nhwc || ld >= C, BD_ERR_INVALID, "bd_to_image: ld=%lld < C=%d", (long long)ld, C);
    hipLaunchKernelGGL(to_image_kernel, dim3(nblocks((int64_t)B * H * W)), dim3(TPB), 0, S(stream), x, src_is_nhwc, ld, B, C,
                       (int64_t)H * W, out_f32, out_u8);
    BD_LAUNCH_CHECK("to_image");
    return BD_OK;
}
extern "C" int bd_timestep_embedding(const int64_t* t, int t_stride, int B, int dim, int flip_sin_to_cos, float freq_shift,
                                     float* out, bd_stream_t stream) {
    BD_CHECK(t && out && B > 0 && dim >= 2, BD_ERR_INVALID, "bd_timestep_embedding: bad args");
    hipLaunchKernelGGL(timestep_embedding_kernel<int64_t>, dim3(nblocks((int64_t)B * (dim / 2))), dim3(TPB), 0, S(stream), t, t_stride,
                       B, dim, flip_sin_to_cos, freq_shift, out);
    BD_LAUNCH_CHECK("timestep_embedding");
    return BD_OK;
}
extern "C" int bd_timestep_embedding_f32(const float* t, int t_stride, int B, int dim, int flip_sin_to_cos, float freq_shift,
                                         float* out, bd_stream_t stream) {
    BD_CHECK(t && out && B > 0 && dim >= 2, BD_ERR_INVALID, "bd_timestep_embedding_f32: bad args");
    hipLaunchKernelGGL(timestep_embedding_kernel<float>, dim3(nblocks((int64_t)B * (dim / 2))), dim3(TPB), 0, S(stream), t, t_stride,
                       B, dim, flip_sin_to_cos, freq_shift, out);
    BD_LAUNCH_CHECK("timestep_embedding_f32");
    return BD_OK;
}
extern "C" int bd_silu_fwd(const float* x, float* y, int64_t n, bd_stream_t stream) {
    BD_CHECK(x && y && n > 0, BD_ERR_INVALID, "bd_silu_fwd: bad args");
    hipLaunchKernelGGL(silu_fwd_kernel, dim3(nblocks(n, TPB, 4096)), dim3(TPB), 0, S(stream), x, y, n);
    BD_LAUNCH_CHECK("silu_fwd");
    return BD_OK;
}
extern "C" int bd_silu_bwd(const float* x, const float* dy, float* dx, int64_t n, int accumulate, bd_stream_t stream) {
    BD_CHECK(x && dy && dx && n > 0, BD_ERR_INVALID, "bd_silu_bwd: bad args");
    hipLaunchKernelGGL(silu_bwd_kernel, dim3(nblocks(n, TPB, 4096)), dim3(TPB), 0, S(stream), x, dy, dx, n, accumulate);
    BD_LAUNCH_CHECK("silu_bwd");
    return BD_OK;
}
extern "C" int bd_softmax_fwd(const float* s, float* p, int64_t rows, int n, bd_stream_t stream) {
    BD_CHECK(s && p && rows > 0 && n > 0, BD_ERR_INVALID, "bd_softmax_fwd: bad args");
    hipLaunchKernelGGL(softmax_fwd_kernel, dim3((unsigned)cdiv(rows, TPB / 64)), dim3(TPB), 0, S(stream), s, p, rows, n);
    BD_LAUNCH_CHECK("softmax_fwd");
    return BD_OK;
}
extern "C" int bd_softmax_bwd(const float* p, const float* dp, float* ds, int64_t rows, int n, bd_stream_t stream) {
    BD_CHECK(p && dp && ds && rows > 0 && n > 0, BD_ERR_INVALID, "bd_softmax_bwd: bad args");
    hipLaunchKernelGGL(softmax_bwd_kernel, dim3((unsigned)cdiv(rows, TPB / 64)), dim3(TPB), 0, S(stream), p, dp, ds, rows, n);
    BD_LAUNCH_CHECK("softmax_bwd");
    return BD_OK;
}
extern "C" int bd_colsum(const float* x, int64_t ldx, int64_t rows, int N, int64_t rows_per_group, float* out, int64_t ld_out,
                         int accumulate, bd_stream_t stream) {
    BD_CHECK(x && out && rows > 0 && N > 0 && rows_per_group > 0, BD_ERR_INVALID, "bd_colsum: bad args");
    BD_CHECK(ldx >= N && ld_out >= N, BD_ERR_INVALID, "bd_colsum: ldx=%lld / ld_out=%lld < N=%d", (long long)ldx, (long long)ld_out, N);
    const int64_t groups = cdiv(rows, rows_per_group);
    BD_CHECK(groups <= 65535, BD_ERR_UNSUPPORTED, "bd_colsum: too many groups (%lld)", (long long)groups);
    hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)cdiv(N, 64), (unsigned)groups), dim3(TPB), 0, S(stream), x, ldx, rows, N,
                       rows_per_group, out, ld_out, accumulate);
    BD_LAUNCH_CHECK("colsum");
    return BD_OK;
}
extern "C" int bd_sum2x2(const float* du, int64_t ldu, float* dx, int64_t lddx, int B, int H, int W, int C, int accumulate,
                         bd_stream_t stream) {
    BD_CHECK(du && dx && B > 0 && H > 0 && W > 0 && C > 0, BD_ERR_INVALID, "bd_sum2x2: bad args");
    BD_CHECK(ldu >= C && lddx >= C, BD_ERR_INVALID, "bd_sum2x2: ldu=%lld / lddx=%lld < C=%d", (long long)ldu, (long long)lddx, C);
    BD_CHECK((C & 3) == 0 && (ldu & 3) == 0 && (lddx & 3) == 0 && aligned16(du) && aligned16(dx), BD_ERR_UNSUPPORTED,
             "bd_sum2x2: needs C, ld multiples of 4 and 16B-aligned pointers");
    hipLaunchKernelGGL(sum2x2_kernel, dim3(nblocks((int64_t)B * H * W * (C / 4))), dim3(TPB), 0, S(stream), du, ldu, dx, lddx, B,
                       H, W, C, accumulate);
    BD_LAUNCH_CHECK("sum2x2");
    return BD_OK;
}
namespace bd {
int add_launch(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int C, float scale, int acc,
               hipStream_t st) {
    BD_CHECK(src && dst && rows > 0 && C > 0, BD_ERR_INVALID, "add: bad args");
    BD_CHECK(lds >= C && ldd >= C, BD_ERR_INVALID, "add: lds=%lld / ldd=%lld < C=%d", (long long)lds, (long long)ldd, C);
    BD_CHECK((C & 3) == 0 && (lds & 3) == 0 && (ldd & 3) == 0 && aligned16(src) && aligned16(dst), BD_ERR_UNSUPPORTED,
             "add: needs C, ld multiples of 4 and 16B-aligned pointers");
    hipLaunchKernelGGL(add_kernel, dim3(nblocks(rows * (C / 4), TPB, 8192)), dim3(TPB), 0, st, src, lds, dst, ldd, rows, C, scale,
                       acc);
    BD_LAUNCH_CHECK("add");
    return BD_OK;
}
}  // namespace bd
extern "C" int bd_add(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int C, float scale, int accumulate,
                      bd_stream_t stream) {
    return add_launch(src, lds, dst, ldd, rows, C, scale, accumulate, S(stream));
}
extern "C" size_t bd_reduce_workspace_bytes(void) { return RED_BLOCKS * sizeof(double); }
extern "C" int bd_loss_fwd_bwd(const float* pred, int64_t ldp, const float* target, int64_t ldt, int64_t rows, int C,
                               int loss_type, float grad_scale, float* loss, float* dpred, int64_t lddp, void* workspace,
                               bd_stream_t stream) {
    BD_CHECK(pred && target && loss && workspace && rows > 0 && C > 0, BD_ERR_INVALID, "bd_loss_fwd_bwd: bad args");
    BD_CHECK(ldp >= C && ldt >= C && (!dpred || lddp >= C), BD_ERR_INVALID, "bd_loss_fwd_bwd: ldp=%lld / ldt=%lld / lddp=%lld < C=%d",
             (long long)ldp, (long long)ldt, (long long)lddp, C);
    BD_CHECK(loss_type >= 0 && loss_type <= 2, BD_ERR_UNSUPPORTED, "bd_loss_fwd_bwd: loss_type %d (l2=0,l1=1,huber=2)", loss_type);
    const int nb = (int)nblocks(rows * C, TPB, RED_BLOCKS);
    hipLaunchKernelGGL(loss_kernel, dim3(nb), dim3(TPB), 0, S(stream), pred, ldp, target, ldt, rows, C, loss_type, grad_scale,
                       dpred, lddp, (double*)workspace);
    BD_LAUNCH_CHECK("loss");
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(64), 0, S(stream), (const double*)workspace, nb, rows * C, loss);
    BD_LAUNCH_CHECK("loss_final");
    return BD_OK;
}
extern "C" size_t bd_loss_groups_workspace_bytes(int n_groups) {
    if (n_groups < 1 || n_groups > BD_LOSS_MAX_GROUPS) return 0;
    return (size_t)n_groups * RED_BLOCKS * sizeof(double);
}
extern "C" int bd_loss_groups_fwd_bwd(const float* pred, int64_t ldp, const float* target, int64_t ldt, int64_t rows, int C,
                                      int loss_type, float grad_scale, const bd_loss_groups_desc* groups, float* losses,
                                      float* dpred, int64_t lddp, void* workspace, size_t workspace_bytes, bd_stream_t stream) {
    BD_CHECK(pred && target && groups && losses && workspace && rows > 0 && C > 0, BD_ERR_INVALID, "bd_loss_groups_fwd_bwd: bad args");
    BD_CHECK(ldp >= C && ldt >= C && (!dpred || lddp >= C), BD_ERR_INVALID, "bd_loss_groups_fwd_bwd: ldp=%lld / ldt=%lld / lddp=%lld < C=%d",
             (long long)ldp, (long long)ldt, (long long)lddp, C);
    BD_CHECK(loss_type >= 0 && loss_type <= 2, BD_ERR_UNSUPPORTED, "bd_loss_groups_fwd_bwd: loss_type %d (l2=0,l1=1,huber=2)", loss_type);
    BD_CHECK(groups->n_groups >= 1 && groups->n_groups <= BD_LOSS_MAX_GROUPS, BD_ERR_INVALID,
             "bd_loss_groups_fwd_bwd: n_groups %d outside 1..%d", groups->n_groups, BD_LOSS_MAX_GROUPS);
    LossGroups G = {};
    G.n_groups = groups->n_groups;
    int64_t row0 = 0;
    unsigned nb_max = 1;
    for (int g = 0; g < G.n_groups; ++g) {
        const int64_t r = groups->group_rows[g];
        const float w = groups->group_weight[g];
        BD_CHECK(r > 0 && r <= rows - row0, BD_ERR_INVALID, "bd_loss_groups_fwd_bwd: group_rows[%d] = %lld (must be > 0 and sum to rows = %lld)",
                 g, (long long)r, (long long)rows);
        BD_CHECK(w >= 0.f && std::isfinite(w), BD_ERR_INVALID, "bd_loss_groups_fwd_bwd: group_weight[%d] = %g (must be finite and >= 0)", g,
                 (double)w);
        const unsigned nb = nblocks(r * C, TPB, RED_BLOCKS);
        G.nb[g] = (int)nb; G.row0[g] = row0; G.rows[g] = r; G.weight[g] = w;
        if (nb > nb_max) nb_max = nb;
        row0 += r;
    }
    BD_CHECK(row0 == rows, BD_ERR_INVALID, "bd_loss_groups_fwd_bwd: group_rows sum to %lld, rows = %lld", (long long)row0, (long long)rows);
    BD_CHECK(workspace_bytes >= bd_loss_groups_workspace_bytes(G.n_groups), BD_ERR_WORKSPACE,
             "bd_loss_groups_fwd_bwd: workspace %zu < %zu bytes", workspace_bytes, bd_loss_groups_workspace_bytes(G.n_groups));
    hipLaunchKernelGGL(loss_groups_kernel, dim3(nb_max, G.n_groups), dim3(TPB), 0, S(stream), pred, ldp, target, ldt, C, loss_type,
                       grad_scale, dpred, lddp, (double*)workspace, G);
    BD_LAUNCH_CHECK("loss_groups");
    hipLaunchKernelGGL(loss_groups_final_kernel, dim3(1), dim3(64), 0, S(stream), (const double*)workspace, C, losses, G);
    BD_LAUNCH_CHECK("loss_groups_final");
    return BD_OK;
}
extern "C" int bd_sumsq(const float* g, int64_t n, double* sumsq, void* workspace, bd_stream_t stream) {
    BD_CHECK(g && sumsq && workspace && n > 0 && aligned16(g), BD_ERR_INVALID, "bd_sumsq: bad args");
    const int nb = (int)nblocks(n / 4 + 1, TPB, RED_BLOCKS);
    hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(TPB), 0, S(stream), g, n, (double*)workspace);
    BD_LAUNCH_CHECK("sumsq");
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(64), 0, S(stream), (const double*)workspace, nb, sumsq);
    BD_LAUNCH_CHECK("sumsq_final");
    return BD_OK;
}
extern "C" int bd_adam_clip(float* p, const float* g, float* m, float* v, int64_t n, const double* sumsq, double max_norm,
                            double lr, double b1, double b2, double eps, int step, float* grad_norm_out, bd_stream_t stream) {
    BD_CHECK(p && g && m && v && sumsq && n > 0 && step >= 1, BD_ERR_INVALID, "bd_adam_clip: bad args");
    const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - pow(b2, step);
    const float step_size = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    hipLaunchKernelGGL(adam_clip_kernel<false>, dim3(nblocks(n, TPB, 8192)), dim3(TPB), 0, S(stream), p, g, m, v, n, sumsq,
                       (float)max_norm, step_size, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)eps, bc2_sqrt, grad_norm_out,
                       (const float*)nullptr, (float*)nullptr, 0.f);
    BD_LAUNCH_CHECK("adam_clip");
    return BD_OK;
}
extern "C" int bd_adam_clip_dev(float* p, const float* g, float* m, float* v, int64_t n, const double* sumsq, double max_norm,
                                const float* hyper, double b1, double b2, double eps, float* grad_norm_out, bd_stream_t stream) {
    BD_CHECK(p && g && m && v && sumsq && hyper && n > 0, BD_ERR_INVALID, "bd_adam_clip_dev: bad args");
    hipLaunchKernelGGL(adam_clip_kernel<false>, dim3(nblocks(n, TPB, 8192)), dim3(TPB), 0, S(stream), p, g, m, v, n, sumsq,
                       (float)max_norm, 0.f, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)eps, 1.f, grad_norm_out, hyper,
                       (float*)nullptr, 0.f);
    BD_LAUNCH_CHECK("adam_clip_dev");
    return BD_OK;
}
extern "C" int bd_adam_clip_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const double* sumsq, double max_norm,
                                double lr, double b1, double b2, double eps, int step, float one_minus_decay, float* grad_norm_out,
                                bd_stream_t stream) {
    BD_CHECK(p && g && m && v && ema && sumsq && n > 0 && step >= 1, BD_ERR_INVALID, "bd_adam_clip_ema: bad args (null pointer, n <= 0 or step < 1)");
    const float* others[4] = {p, m, v, g};
    const int bad = ema_args_bad(ema, others, 4, n, one_minus_decay);
    BD_CHECK(bad != 1, BD_ERR_INVALID, "bd_adam_clip_ema: one_minus_decay = %g (must be finite and in [0, 1])", (double)one_minus_decay);
    BD_CHECK(bad == 0, BD_ERR_INVALID, "bd_adam_clip_ema: ema overlaps p, m, v or g over n = %lld floats", (long long)n);
    const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - pow(b2, step);
    const float step_size = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    hipLaunchKernelGGL(adam_clip_kernel<true>, dim3(nblocks(n, TPB, 8192)), dim3(TPB), 0, S(stream), p, g, m, v, n, sumsq,
                       (float)max_norm, step_size, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)eps, bc2_sqrt, grad_norm_out,
                       (const float*)nullptr, ema, one_minus_decay);
    BD_LAUNCH_CHECK("adam_clip_ema");
    return BD_OK;
}
extern "C" int bd_adam_clip_ema_dev(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const double* sumsq,
                                    double max_norm, const float* hyper, double b1, double b2, double eps, float* grad_norm_out,
                                    bd_stream_t stream) {
    BD_CHECK(p && g && m && v && ema && sumsq && hyper && n > 0, BD_ERR_INVALID, "bd_adam_clip_ema_dev: bad args (null pointer or n <= 0)");
    hipLaunchKernelGGL(adam_clip_kernel<true>, dim3(nblocks(n, TPB, 8192)), dim3(TPB), 0, S(stream), p, g, m, v, n, sumsq,
                       (float)max_norm, 0.f, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)eps, 1.f, grad_norm_out, hyper, ema,
                       0.f);
    BD_LAUNCH_CHECK("adam_clip_ema_dev");
    return BD_OK;
}
extern "C" int bd_ema_update(float* ema, const float* p, int64_t n, float one_minus_decay, bd_stream_t stream) {
    BD_CHECK(ema && p && n > 0, BD_ERR_INVALID, "bd_ema_update: bad args (null pointer or n <= 0)");
    const float* others[1] = {p};
    const int bad = ema_args_bad(ema, others, 1, n, one_minus_decay);
    BD_CHECK(bad != 1, BD_ERR_INVALID, "bd_ema_update: one_minus_decay = %g (must be finite and in [0, 1])", (double)one_minus_decay);
    BD_CHECK(bad == 0, BD_ERR_INVALID, "bd_ema_update: ema overlaps p over n = %lld floats", (long long)n);
    hipLaunchKernelGGL(ema_update_kernel, dim3(nblocks(n, TPB, 8192)), dim3(TPB), 0, S(stream), ema, p, n, one_minus_decay);
    BD_LAUNCH_CHECK("ema_update");
    return BD_OK;
}
__global__ __launch_bounds__(256) void axpy_kernel(const float* src, float* dst, int64_t n, float scale, int acc) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float v = src[i] * scale;
        if (acc) v += dst[i];
        dst[i] = v;
    }
}
extern "C" int bd_axpy(const float* src, float* dst, int64_t n, float scale, int accumulate, bd_stream_t stream) {
    BD_CHECK(src && dst && n > 0, BD_ERR_INVALID, "bd_axpy: bad args");
    hipLaunchKernelGGL(axpy_kernel, dim3(nblocks(n, TPB, 8192)), dim3(TPB), 0, S(stream), src, dst, n, scale, accumulate);
    BD_LAUNCH_CHECK("axpy");
    return BD_OK;
}

extern "C" int bd_anp_apply(const float* params, int64_t nparams, const float* pert_w, const float* pert_b, const int64_t* items, int n_items,
                            int64_t total_rows, float* eff, bd_stream_t stream) {
    BD_CHECK(params && pert_w && pert_b && items && eff && nparams > 0 && n_items > 0 && total_rows > 0 && total_rows < (1ll << 31), BD_ERR_INVALID,
             "bd_anp_apply: bad args");
    BD_HIP_TRY(hipMemcpyAsync(eff, params, (size_t)nparams * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
    hipLaunchKernelGGL(anp_apply_kernel, dim3((unsigned)total_rows), dim3(TPB), 0, S(stream), params, pert_w, pert_b, items, n_items, eff);
    BD_LAUNCH_CHECK("anp_apply");
    return BD_OK;
}
extern "C" int bd_anp_grad(const float* params, const float* grad_eff, const int64_t* items, int n_items, int64_t total_rows, const float* pert_w,
                           float* grad_w, float* grad_b, float* row_norm, bd_stream_t stream) {
    BD_CHECK(params && grad_eff && items && grad_w && grad_b && n_items > 0 && total_rows > 0 && total_rows < (1ll << 31), BD_ERR_INVALID,
             "bd_anp_grad: bad args");
    BD_CHECK(!row_norm || pert_w, BD_ERR_INVALID, "bd_anp_grad: row_norm needs pert_w");
    hipLaunchKernelGGL(anp_grad_kernel, dim3((unsigned)total_rows), dim3(TPB), 0, S(stream), params, grad_eff, items, n_items, pert_w, grad_w,
                       grad_b, row_norm);
    BD_LAUNCH_CHECK("anp_grad");
    return BD_OK;
}
