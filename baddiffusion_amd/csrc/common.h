// Shared host/device helpers for libbd_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/bd_hip.h"

namespace bd {

void set_error(const char* fmt, ...);

#define BD_CHECK(cond, status, ...)                 \
    do {                                            \
        if (!(cond)) {                              \
            ::bd::set_error(__VA_ARGS__);           \
            return (status);                        \
        }                                           \
    } while (0)

#define BD_LAUNCH_CHECK(name)                                                         \
    do {                                                                              \
        hipError_t e__ = hipGetLastError();                                           \
        if (e__ != hipSuccess) {                                                      \
            ::bd::set_error("%s: launch failed: %s", (name), hipGetErrorString(e__)); \
            return BD_ERR_LAUNCH;                                                     \
        }                                                                             \
    } while (0)

#define BD_HIP_TRY(expr)                                                                   \
    do {                                                                                   \
        hipError_t e__ = (expr);                                                           \
        if (e__ != hipSuccess) {                                                           \
            ::bd::set_error("%s failed: %s", #expr, hipGetErrorString(e__));               \
            return BD_ERR_LAUNCH;                                                          \
        }                                                                                  \
    } while (0)

#define BD_TRY(expr)                  \
    do {                              \
        int s__ = (expr);             \
        if (s__ != BD_OK) return s__; \
    } while (0)

static inline hipStream_t S(bd_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// BD_MODE_BF16X3 and BD_MODE_BF16 run the same bf16 MFMA kernels and plans (three products vs one)
static inline bool mode_bf16(int m) { return m == BD_MODE_BF16X3 || m == BD_MODE_BF16; }
static inline bool mode_valid(int m) { return m == BD_MODE_F32 || mode_bf16(m); }
// the split-plane kernels' descriptor field: 0 (zero-initialised) or BD_MODE_BF16X3 = three products, BD_MODE_BF16 = one
static inline bool sp_mode_valid(int m) { return m == 0 || mode_bf16(m); }
static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// GroupNorm statistics partials [B][S][G][2] fp64 (sum, sum of squares per sample, pixel split and group): written by gn_stats_kernel or by
// the epilogue of the producing convolution (bd_conv3x3_ps gn_part), read by gn_fwd_finalize_kernel
static inline size_t gn_stats_partial_bytes(int B, int S, int G) { return (size_t)B * (size_t)S * (size_t)G * 2 * sizeof(double); }
// log2 of a power of two, -1 for anything else
static inline int ilog2_exact(int v) {
    if (v <= 0 || (v & (v - 1))) return -1;
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}
// CU count of the current device (256 if the query fails), looked up once per process: the project drives one GPU per process, so the
// first answer holds for every later call.
static inline int device_cus() {
    static const int cus = [] {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return n > 0 ? n : 256;
    }();
    return cus;
}
// K split of `nchunks` chunks over `tiles` output tiles on `slots` workgroup slots: as many splits as fill the slots (rounded down),
// each at least `mincps` chunks long, and no empty split.
static inline void split_k(int slots, long long tiles, int nchunks, int mincps, int& ksplit, int& cps) {
    int ks = (int)(slots / tiles);
    if (ks > nchunks / mincps) ks = nchunks / mincps;
    if (ks < 1) ks = 1;
    cps = (int)cdiv(nchunks, ks);
    ksplit = (int)cdiv(nchunks, cps);
}

// XCD-contiguous order of a 1-D grid: workgroup L runs on XCD L % 8 and each XCD has its own L2, so every XCD is handed one contiguous
// run of the logical order j and the tiles that share an operand panel meet in one L2.  Speed only; callers decompose j themselves.
// (groupnorm.hip's gn_res_coord keeps its own `if` form of this line: its kernels take up to 30 more VGPRs behind the select.)
__device__ __forceinline__ unsigned xcd_tile_order() {
    const unsigned L = blockIdx.x, T = gridDim.x, q = T >> 3;
    return L < (q << 3) ? (L & 7) * q + (L >> 3) : L;
}

// ---- wave64 reductions (DPP/shuffle, no LDS) --------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- the loss element function of bd_loss_fwd_bwd, bd_loss_groups_fwd_bwd (elementwise.hip) and bd_image_loss (metrics.hip; both files
// are built with -ffp-contract=off): per-element loss l and derivative g of loss(target, pred) at df = pred - target
__device__ __forceinline__ void loss_elem(int type, float df, float& l, float& g) {
    if (type == 0) { l = df * df; g = 2.0f * df; }
    else if (type == 1) { l = fabsf(df); g = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f); }
    else { float ad = fabsf(df); if (ad < 1.0f) { l = 0.5f * df * df; g = df; } else { l = ad - 0.5f; g = df > 0.f ? 1.f : -1.f; } }
}

// ---- the predicted x0 of an epsilon model, x0 = (x - sqrt(1 - a_t) e) / sqrt(a_t): ddpm_step_kernel, ddim_step_kernel, abs_quantile_kernel
// (elementwise.hip) and vb_terms_kernel (metrics.hip) all form it here, so the value the quantile ranks is bitwise the value the step clamps
// and the value the variational bound scores.
struct X0Coef { float sb, sa; };
__device__ __forceinline__ X0Coef x0_coef(const float* alphas_cumprod, int t) {
    const float a_t = alphas_cumprod[t];
    X0Coef k;
    k.sb = sqrtf(1.0f - a_t); k.sa = sqrtf(a_t);
    return k;
}
__device__ __forceinline__ float x0_pred(const X0Coef& k, float x, float e) { return (x - k.sb * e) / k.sa; }

// ---- predicated loads without control flow and without a dependent select: masked-off lanes read zero bytes that live in the code
// object.  Branch-free loads keep the s_waitcnt vmcnt() counting exact, and nothing touches the loaded registers until their first
// use, which the register prefetch of the igemm kernels depends on (a skipped load would force vmcnt(0) at the join, a select would
// wait for the load right behind its issue).  The zero page is also the LDS-DMA source of lanes whose filter tap falls outside the
// image (splitplane.h).  One object per translation unit: the library is built without relocatable device code.
[[maybe_unused]] static __device__ __attribute__((aligned(16))) const float bd_zero16[4] = {0.f, 0.f, 0.f, 0.f};
typedef float bd_f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 bd_ld4_if(const float* p, bool ok) {      // global address space: global_load, not flat_load
    const bd_f32x4_t t = *(const bd_f32x4_t __attribute__((address_space(1)))*)(ok ? p : bd_zero16);
    return make_float4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ float bd_ld1_if(const float* p, bool ok) {
    return *(const float __attribute__((address_space(1)))*)(ok ? p : bd_zero16);
}

// ---- THE split of this library (round 6): x = hi + lo with hi = RNE_bf16(x), lo = RNE_bf16(x - hi).  x - hi is exact in fp32 (at most 16
// significant bits), so hi + lo reproduces x to 2^-18 |x| and the dropped lo * lo product is <= 2^-18 of the term -- rounds 1 - 5 truncated
// hi (the upper 16 bits of x), which costs one bit on both (per-convolution error vs fp64 8.8e-6 -> 4e-6, scripts/wino/numerics.py).  Every
// producer of split planes and every on-the-fly split goes through these four functions: the MFMA engines stay bit-identical to one
// another because they split identically.  (__bf16)float is v_cvt_pk_bf16_f32 on gfx950: round to nearest even.
typedef __bf16 bd_bf16x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bd_bf16x8_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ unsigned bd_pack_hi(float a, float b) {          // bf16 RNE(a) | bf16 RNE(b) << 16
    bd_bf16x2_t t;
    t[0] = (__bf16)a; t[1] = (__bf16)b;
    return __builtin_bit_cast(unsigned, t);
}
__device__ __forceinline__ unsigned bd_pack_lo(float a, float b) {          // the remainders' planes
    const unsigned h = bd_pack_hi(a, b);
    const float ra = a - __builtin_bit_cast(float, h << 16);
    const float rb = b - __builtin_bit_cast(float, h & 0xFFFF0000u);
    bd_bf16x2_t t;
    t[0] = (__bf16)ra; t[1] = (__bf16)rb;
    return __builtin_bit_cast(unsigned, t);
}
__device__ __forceinline__ unsigned bd_split1(float v) {                    // hi | lo << 16 of one value
    const __bf16 h = (__bf16)v;
    const unsigned hb = (unsigned)__builtin_bit_cast(unsigned short, h);
    const __bf16 l = (__bf16)(v - __builtin_bit_cast(float, hb << 16));
    return hb | ((unsigned)__builtin_bit_cast(unsigned short, l) << 16);
}
__device__ __forceinline__ void bd_split8(const float (&x)[8], bd_bf16x8_t& hi, bd_bf16x8_t& lo) {   // eight values into MFMA fragments
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        hi[j] = (__bf16)x[j];
        lo[j] = (__bf16)(x[j] - (float)hi[j]);      // (float)hi: the exact widening the functions above write as bits << 16
    }
}

// ---- run-time tuning knobs (bd_tune_set): a generation counter that makes every plan lay its workspace out again -----------------
extern int g_tune_gen;

// ---- internal (non-ABI) launchers shared between files: every one is declared here and nowhere else ---------------------------
int igemm_launch(const bd_igemm_desc& d, hipStream_t stream);                       // igemm.hip
size_t igemm_workspace_bytes(const bd_igemm_desc& d);
bool prof_on();                                                                     // prof.cpp
int prof_begin(const char* name, double flops, double bytes, hipStream_t st);
void prof_end(int rec, hipStream_t st);
int add_launch(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int C, float scale, int acc,   // elementwise.hip
               hipStream_t st);
int conv3x3_fwd(const bd_conv3x3_fwd_desc& d, hipStream_t st);                      // conv.cpp
int conv3x3_dgrad(const bd_conv3x3_dgrad_desc& d, hipStream_t st);
int conv3x3_wgrad(const bd_conv3x3_wgrad_desc& d, hipStream_t st);
int conv3x3_fwd_thin(const bd_conv3x3_fwd_desc& d, hipStream_t st);                 // conv_thin.hip
int conv3x3_dgrad_thin(const bd_conv3x3_dgrad_desc& d, hipStream_t st);
int conv3x3_wgrad_thin(const bd_conv3x3_wgrad_desc& d, hipStream_t st);
bool conv3x3_wgrad_is_thin(const bd_conv3x3_wgrad_desc& d);
bd_conv3x3_thin_plan_info conv3x3_fwd_thin_plan(const bd_conv3x3_fwd_desc& d);      // pure host: what the three launchers above read
bd_conv3x3_thin_plan_info conv3x3_dgrad_thin_plan(const bd_conv3x3_dgrad_desc& d);
bd_conv3x3_thin_plan_info conv3x3_wgrad_thin_plan(const bd_conv3x3_wgrad_desc& d);
int conv3x3_wgrad_thin_check(const bd_conv3x3_wgrad_desc& d, const bd_conv3x3_thin_plan_info& p);
// the K-split slabs every conv3x3 workspace holds (conv.cpp conv3x3_workspace_bytes); the thin weight gradients fit their partial rows in it
constexpr size_t CONV3X3_WS_SLAB_BYTES = (size_t)768 * 128 * 128 * sizeof(float);
int conv3x3_ps(const bd_conv3x3_ps_desc& d, hipStream_t st);                        // conv_ps.hip
bool conv3x3_ps_supported(int B, int H, int W, int K_channels, int N_channels);
int conv3x3_ps_wgrad(const bd_conv3x3_ps_wgrad_desc& d, hipStream_t st);
size_t conv3x3_ps_wgrad_workspace_bytes(const bd_conv3x3_ps_wgrad_desc& d);
bool conv3x3_ps_wgrad_supported(int B, int H, int W, int Cin, int Cout);
int upsample_conv_wgrad(const bd_upsample_conv_desc& d, hipStream_t st);            // (PHASE form of the weight gradient)
size_t upsample_conv_wgrad_workspace_bytes(const bd_upsample_conv_desc& d);
int split_wt_batched(const float* params, uint16_t* out, const long long* off, const int* cin, const int* cout, int n, hipStream_t st);
int upsample_weights(const float* w, int Cin, int Cout, uint16_t* e_split, uint16_t* et_split, hipStream_t st);   // conv_ph.hip
int upsample_conv_fwd(const bd_upsample_conv_desc& d, hipStream_t st);
int upsample_conv_dgrad(const bd_upsample_conv_desc& d, hipStream_t st);
size_t upsample_conv_dgrad_workspace_bytes(const bd_upsample_conv_desc& d);
int upsample_conv_dgrad_tap_groups(int B, int H, int W, int Cin);                   // 4 or 1: the launcher's rule, also the network plan's path choice
bool upsample_conv_ps_supported(int B, int H, int W, int Cin, int Cout);
int conv3x3_s2_dgrad_ps(const bd_conv3x3_s2_dgrad_desc& d, hipStream_t st);
int ups_dweff_combine(const float* de, int Cin, int Cout, float* dw, hipStream_t st);
int gemm_sp(const bd_gemm_sp_desc& d, hipStream_t st);                              // gemm_sp.hip
size_t gemm_sp_workspace_bytes(const bd_gemm_sp_desc& d);
bool gemm_sp_supported(int M, int N, int K);
int attn_sp_fwd(const bd_attn_sp_desc& d, hipStream_t st);                          // attn_sp.hip
int attn_sp_bwd(const bd_attn_sp_desc& d, hipStream_t st);
bool attn_sp_supported(int N, int dh);

}  // namespace bd
