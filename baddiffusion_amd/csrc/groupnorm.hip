// GroupNorm (+SiLU) forward / backward over NHWC(ld) activations, gfx950.
//
// A group is `cpg` ADJACENT channels x all pixels of one sample, so in NHWC the reduction is strided:
// every pixel contributes cpg*4 contiguous bytes.  Workgroups therefore read whole pixel rows (all C
// channels, float4 per lane, fully coalesced) and keep per-channel partials; channels are folded into
// groups afterwards.  Reductions are two-stage and fixed-order (deterministic): per-(sample, split)
// partials -> tiny finalize.  HBM-bound: stats pass reads x once, apply pass reads x + writes y.
//
// RESIDENT variants (gn_fwd_res / gn_bwd_res): when HW x (a block of whole groups) fits the register file of one
// workgroup (<= 16 float4 per thread and tensor -- every layer of the 32x32 UNet), one workgroup owns a
// (sample, channel block) slab: it reads x (and dy) ONCE, reduces inside the workgroup (LDS, fixed order), and
// applies from registers.  One launch and 2 (fwd) / 3 (bwd) tensor passes instead of 2 launches + 3 passes /
// 3 launches + 5 passes.  Larger images (CelebA-HQ 256^2) keep the split two-stage kernels below.
//
// Replaces aten::native_group_norm / native_group_norm_backward / silu / silu_backward
// (resnet.py:559,591; attention.py:125; unet_2d.py:312-313).
//
// Layout: the device helpers the kernels share (GnChan, gn_affine, gn_dz, gn_dx_term, gn_mean_rstd, GnSpan), the two-stage kernels, the
// resident kernels, then the host side: gn_plan() decides once what the launchers decide from a shape, gn_fwd_workspace() /
// gn_bwd_workspace() lay the workspace out, and bd_gn_fwd, bd_gn_bwd, bd_gn_plan, bd_gn_fwd_takes_stats and bd_gn_bwd_defers read those.
#include <type_traits>
#include "common.h"

namespace bd {

// Round 4: the sigmoid from the hardware transcendentals -- v_exp_f32 (2^x, 1 ulp) of -z * log2(e) and v_rcp_f32 (1 ulp): 4 VALU instructions instead of
// the ~25 of expf() + an IEEE division, <= 3 ulp of fp32 (tests: 1e-5 against fp64 torch).  An instruction census of the CIFAR step
// (scripts/valu_census.sh, SQ_INSTS_VALU per kernel) puts a THIRD of all VALU wave-instructions in the GroupNorm kernels, which share the chip with
// MFMA kernels bound by issue slots and board power.  Used by the large-image kernels (gn_apply / gn_bwd_stats / gn_bwd_apply: 28.10 -> 27.54 ms per
// 256 x 256 step) and by the resident BACKWARD kernel (17.64 -> 17.54 ms per CIFAR step; same 124 VGPRs).  In the resident FORWARD kernel the intrinsic form
// makes hipcc hoist all sixty-four v_exp_f32 of gn_fwd_res_kernel<16, 256> to the top of the apply loop and spill 66 VGPRs (260 B of scratch per lane under
// the 128-VGPR budget of four workgroups per CU: the step got 0.22 ms SLOWER; a sched_barrier per row piece does not cure it).  silu_fast_pinned issues
// the same two instructions as volatile asm, which keep their program order: 127 VGPRs / 12 B scratch like the expf() build, 18.03 -> 17.87 ms per CIFAR
// step, DDIM-50 502 -> 511 samples/s.
__device__ __forceinline__ float gn_sigmoid_fast(float z) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(__fmul_rn(z, -1.44269504088896341f)));
}
__device__ __forceinline__ float silu_fast(float z) { return z * gn_sigmoid_fast(z); }
// the same two instructions as volatile asm: they keep their program order, so the scheduler cannot hoist sixty-four of them to the top of a loop nest
__device__ __forceinline__ float silu_fast_pinned(float z) {
    float e, r;
    const float t = __fmul_rn(z, -1.44269504088896341f);
    asm volatile("v_exp_f32 %0, %1\n\ts_nop 0" : "=v"(e) : "v"(t));
    e += 1.0f;
    asm volatile("v_rcp_f32 %0, %1\n\ts_nop 0" : "=v"(r) : "v"(e));
    return z * r;
}
__device__ __forceinline__ float silu_grad_fast(float z) {
    const float s = gn_sigmoid_fast(z);
    return s * (1.0f + z * (1.0f - s));
}

// ---- split-plane output (bd_hip.h "split planes"): 4 consecutive channels c..c+3 of one row -> 8 B of bf16 hi and 8 B of
// bf16 lo (common.h: hi = RNE, lo = RNE of the remainder: bit-identical to the on-the-fly split of the bf16x3 engine)
// row = start of the row's planes (uint16 units), c = channel of o.x (c % 4 == 0)
__device__ __forceinline__ void gn_store_split4(unsigned short* row, int c, const float4& o) {
    unsigned short* q = row + (c >> 5) * 64 + (c & 31);
    *reinterpret_cast<uint2*>(q) = make_uint2(bd_pack_hi(o.x, o.y), bd_pack_hi(o.z, o.w));
    *reinterpret_cast<uint2*>(q + 32) = make_uint2(bd_pack_lo(o.x, o.y), bd_pack_lo(o.z, o.w));
}

// The kernels below load their rows with common.h's bd_ld4_if.  A `cond ? *p : 0` in an unrolled loop makes hipcc branch around every
// load and wait vmcnt(0) behind it (cdna_hip_programming.md section 5, trap (c)): 16 serialised memory round trips per thread instead
// of 16 loads in flight.

// ---- the arithmetic the kernels share, written once ---------------------------------------------------
// the constants of a thread's four channels c0 .. c0 + 3 of sample b
struct GnChan {
    float mu[4], rs[4], gg[4], bb[4];
    GnChan() = default;      // (filled by the kernel's own loop: see there why)
    __device__ __forceinline__ GnChan(const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
                                      const float* __restrict__ beta, int b, int G, int cpg, int c0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j, g = c / cpg;
            mu[j] = mean[b * G + g]; rs[j] = rstd[b * G + g];
            gg[j] = gamma[c]; bb[j] = beta[c];
        }
    }
};
__device__ __forceinline__ float gn_xhat(const GnChan& k, int j, float x) { return (x - k.mu[j]) * k.rs[j]; }
__device__ __forceinline__ float gn_z(const GnChan& k, int j, float xhat) { return xhat * k.gg[j] + k.bb[j]; }   // what the SiLU sees
__device__ __forceinline__ float gn_affine(const GnChan& k, int j, float x) { return gn_z(k, j, gn_xhat(k, j, x)); }
// dz: dy through the SiLU's gradient
__device__ __forceinline__ float gn_dz(const GnChan& k, int j, float xhat, float dy, int silu) {
    return silu ? dy * silu_grad_fast(gn_z(k, j, xhat)) : dy;
}
// dx = rstd * (dz*gamma - (s1 + xhat*s2)/n), s1 = sum gamma*dz and s2 = sum gamma*dz*xhat over the group
__device__ __forceinline__ float gn_dx_term(const GnChan& k, int j, float xhat, float dz, float s1, float s2, float inv_n) {
    return k.rs[j] * (dz * k.gg[j] - (s1 + xhat * s2) * inv_n);
}
// (mean, rstd) of a group from its sum a and sum of squares c2 over n elements
__device__ __forceinline__ void gn_mean_rstd(double a, double c2, double n, float eps, float* mean, float* rstd) {
    const double mu = a / n;
    double var = c2 / n - mu * mu;
    if (var < 0.0) var = 0.0;
    *mean = (float)mu;
    *rstd = (float)(1.0 / sqrt(var + (double)eps));
}
// a thread of the two-stage kernels (grid = (pixel ranges, B), block = q x r threads): float4 column cq of the pixel rows prow, prow + r, ...
// of [p0, p1) in sample b.  splits: n is the number of ranges (statistics kernels), else the rows of one (apply kernels).  (A constructor:
// hipcc optimises a function that returns the struct on its own before inlining it, and the statistics kernels' schedule changes.)
struct GnSpan {
    int cq, prow, b, p0, p1;
    __device__ __forceinline__ GnSpan(int q, int HW, int n, bool splits) {
        const int t = threadIdx.x;
        cq = t % q; prow = t / q;
        b = blockIdx.y;
        const int bx = blockIdx.x, per = splits ? (HW + n - 1) / n : n;
        p0 = bx * per;
        p1 = p0 + per;
        if (p1 > HW) p1 = HW;
    }
};

// ---- forward stats: per (b, split) partial (sum, sumsq) per group, in double -----------------------
__global__ void gn_stats_kernel(const float* __restrict__ x, long long ldx, int HW, int C, int G, int r, int S,
                                double* __restrict__ part /* [B][S][G][2] */) {
    extern __shared__ float sh[];  // [r][C][2]
    const auto [cq, prow, b, p0, p1] = GnSpan(C / 4, HW, S, true);
    const int t = threadIdx.x, s = blockIdx.x;
    float sm[4] = {0.f, 0.f, 0.f, 0.f}, sq[4] = {0.f, 0.f, 0.f, 0.f};
    const float* xb = x + (long long)b * HW * ldx + cq * 4;
    for (int p = p0 + prow; p < p1; p += 4 * r) {   // four rows in flight (branch-free: rows past the end read zeros)
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = bd_ld4_if(xb + (long long)(p + u * r) * ldx, p + u * r < p1);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            sm[0] += v[u].x; sm[1] += v[u].y; sm[2] += v[u].z; sm[3] += v[u].w;
            sq[0] += v[u].x * v[u].x; sq[1] += v[u].y * v[u].y; sq[2] += v[u].z * v[u].z; sq[3] += v[u].w * v[u].w;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        sh[(prow * C + cq * 4 + j) * 2 + 0] = sm[j];
        sh[(prow * C + cq * 4 + j) * 2 + 1] = sq[j];
    }
    __syncthreads();
    const int cpg = C / G;
    for (int g = t; g < G; g += blockDim.x) {
        double a = 0.0, c2 = 0.0;
        for (int pr = 0; pr < r; ++pr)
            for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
                a += (double)sh[(pr * C + c) * 2 + 0];
                c2 += (double)sh[(pr * C + c) * 2 + 1];
            }
        double* o = part + (((long long)b * S + s) * G + g) * 2;
        o[0] = a;
        o[1] = c2;
    }
}

// ---- forward finalize: (mean, rstd)[b][g] from the S partials (fp64, fixed order: 8 interleaved phases per group, then
// the phases); one block per sample, 8 threads per group so that 128 pixel splits do not serialise on 32 threads
__global__ __launch_bounds__(256) void gn_fwd_finalize_kernel(const double* __restrict__ part, int G, int S, double n, float eps,
                                                            float* __restrict__ mean, float* __restrict__ rstd) {
    __shared__ double red[256][2];
    const int b = blockIdx.x;
    const int ph = threadIdx.x & 7;
    for (int g0 = 0; g0 < G; g0 += 32) {
        const int g = g0 + (threadIdx.x >> 3);
        double a = 0.0, c2 = 0.0;
        if (g < G)
            for (int sp = ph; sp < S; sp += 8) {
                const double* p = part + (((long long)b * S + sp) * G + g) * 2;
                a += p[0];
                c2 += p[1];
            }
        red[threadIdx.x][0] = a; red[threadIdx.x][1] = c2;
        __syncthreads();
        if (ph == 0 && g < G) {
            a = 0.0; c2 = 0.0;
            for (int k = 0; k < 8; ++k) { a += red[threadIdx.x + k][0]; c2 += red[threadIdx.x + k][1]; }
            float m, r;
            gn_mean_rstd(a, c2, n, eps, &m, &r);
            mean[b * G + g] = m; rstd[b * G + g] = r;
        }
        __syncthreads();
    }
}

// ---- forward apply: y = silu?((x - mean) * rstd * gamma + beta); grid = (pixel ranges, B), block = (C/4) x r threads:
// a thread keeps its four channels' constants in registers and walks its pixel rows four at a time.
// (Round 4, measured and dropped: folding the finalize launch into this kernel -- every thread deriving its group's statistics from the S
// partials -- costs +1.1 ms per 256 x 256 step: a few hundred dependent L2 reads in front of every ~5 us block; visiting the blocks in
// reverse order to meet the Infinity Cache's most recent lines: neutral.)
__global__ void gn_apply_kernel(const float* __restrict__ x, long long ldx, float* __restrict__ y, long long ldy, int HW, int C,
                                int G, int r, int per, const float* __restrict__ gamma, const float* __restrict__ beta,
                                const float* __restrict__ mean, const float* __restrict__ rstd, int silu,
                                unsigned short* __restrict__ ys, long long ldys) {
    const auto [cq, prow, b, p0, p1] = GnSpan(C / 4, HW, per, false);
    const GnChan k(mean, rstd, gamma, beta, b, G, C / G, cq * 4);
    const float* xb = x + (long long)b * HW * ldx + cq * 4;
    float* yb = y + (long long)b * HW * ldy + cq * 4;
    for (int p = p0 + prow; p < p1; p += 4 * r) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = bd_ld4_if(xb + (long long)(p + u * r) * ldx, p + u * r < p1);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float in[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float z = gn_affine(k, j, in[j]);
                o[j] = silu ? silu_fast(z) : z;
            }
            v[u] = make_float4(o[0], o[1], o[2], o[3]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int pu = p + u * r;
            if (pu < p1) {
                if (y) *reinterpret_cast<float4*>(yb + (long long)pu * ldy) = v[u];
                if (ys) gn_store_split4(ys + 2 * ((long long)b * HW + pu) * ldys, cq * 4, v[u]);
            }
        }
    }
}

// ---- backward pass 1: per (b, split) per-channel partial (sum dz, sum dz*xhat) ----------------------
__global__ void gn_bwd_stats_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ dy, long long lddy,
                                    int HW, int C, int G, int r, int S, const float* __restrict__ gamma,
                                    const float* __restrict__ beta, const float* __restrict__ mean,
                                    const float* __restrict__ rstd, int silu, float* __restrict__ part /* [B][S][3][C] */) {
    extern __shared__ float sh[];  // [r][C][3]
    const int q = C / 4, cpg = C / G;
    const auto [cq, prow, b, p0, p1] = GnSpan(q, HW, S, true);
    const int t = threadIdx.x, s = blockIdx.x;
    const GnChan k(mean, rstd, gamma, beta, b, G, cpg, cq * 4);
    float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    const float* xb = x + (long long)b * HW * ldx + cq * 4;
    const float* db = dy + (long long)b * HW * lddy + cq * 4;
    for (int p = p0 + prow; p < p1; p += 4 * r) {   // four rows of both tensors in flight, branch-free
        float4 v[4], d[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool ok = p + u * r < p1;
            v[u] = bd_ld4_if(xb + (long long)(p + u * r) * ldx, ok);
            d[u] = bd_ld4_if(db + (long long)(p + u * r) * lddy, ok);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool ok = p + u * r < p1;
            const float in[4] = {v[u].x, v[u].y, v[u].z, v[u].w}, dd[4] = {d[u].x, d[u].y, d[u].z, d[u].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xh = ok ? gn_xhat(k, j, in[j]) : 0.f;
                const float dz = gn_dz(k, j, xh, dd[j], silu);
                s0[j] += dz;
                s1[j] += dz * xh;
                s2[j] += xh;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        sh[(prow * C + cq * 4 + j) * 3 + 0] = s0[j];
        sh[(prow * C + cq * 4 + j) * 3 + 1] = s1[j];
        sh[(prow * C + cq * 4 + j) * 3 + 2] = s2[j];
    }
    __syncthreads();
    for (int c = t; c < C; c += blockDim.x) {
        float a = 0.f, e = 0.f, h = 0.f;
        for (int pr = 0; pr < r; ++pr) {
            a += sh[(pr * C + c) * 3 + 0];
            e += sh[(pr * C + c) * 3 + 1];
            h += sh[(pr * C + c) * 3 + 2];
        }
        float* o = part + ((long long)b * S + s) * 3 * C + c;
        o[0] = e;       // plane 0: sum dz * xhat  -> dgamma
        o[C] = a;       // plane 1: sum dz         -> dbeta
        o[2 * C] = h;   // plane 2: sum xhat       -> closed-form column sums of dx
    }
}

// ---- backward finalize -----------------------------------------------------------------------------
// (a) dgamma/dbeta[c] = sum over the partial rows, for up to GN_PARAM_MAX layers in one launch: 64 columns x 16 row phases per block, fixed
// order.  A layer's rows are the first two planes (0 = dgamma, 1 = dbeta) of either the per-sample partials [B][2][C] (row stride 2C: the
// resident kernel's, or what bd_gn_bwd_desc.param_partials left to the caller -- one launch per backward segment instead of one per
// GroupNorm) or the two-stage statistics rows [B*S][3][C] (row stride 3C).
constexpr int GN_PARAM_MAX = 32;
struct GnParamTable {
    const float* part[GN_PARAM_MAX]; float* dg[GN_PARAM_MAX]; float* db[GN_PARAM_MAX];
    int C[GN_PARAM_MAX]; int stride[GN_PARAM_MAX]; int blk0[GN_PARAM_MAX + 1]; int n;
};
__global__ __launch_bounds__(1024) void gn_bwd_param_batched_kernel(GnParamTable t, int rows) {
    __shared__ double red[16][64];
    int i = 0;
    while (i + 1 < t.n && (int)blockIdx.x >= t.blk0[i + 1]) ++i;
    const int C = t.C[i];
    const float* part = t.part[i];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // 64 columns x 16 row phases
    const int n = ((int)blockIdx.x - t.blk0[i]) * 64 + tx;    // column in [0, 2C)
    double s = 0.0;
    if (n < 2 * C)
        for (int r = ty; r < rows; r += 16) s += (double)part[(long long)r * t.stride[i] + n];
    red[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && n < 2 * C) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) v += red[k][tx];
        if (n < C) t.dg[i][n] = (float)v; else t.db[i][n - C] = (float)v;
    }
}
// ---- backward group finalize: per (b, g) s1 = sum gamma*dz, s2 = sum gamma*dz*xhat from the per-channel partials
// (fixed order, fp64); optional per-sample column sums of dx in closed form (see gn_bwd_res_kernel) and per-sample weight / bias gradient
// partials.  Round 4 (late): ONE pass over the partials by grid = (B, G) blocks -- every (plane, channel) of the group is summed over the S splits
// by 256 / (3 cpg) threads, folded through LDS in fixed order, and all four outputs derive from those totals.  The previous form (16 blocks of
// 8 groups, three separate sweeps, up to S = 128 dependent-latency loads per thread) took 19 us per launch on the 256 x 256 network's large
// layers, in front of every backward apply.
__global__ __launch_bounds__(256) void gn_bwd_finalize_kernel(const float* __restrict__ part, int HW, int C, int G, int S,
                                                            const float* __restrict__ gamma, const float* __restrict__ rstd,
                                                            float inv_n, float* __restrict__ ds /* [B][G][2] */,
                                                            float* __restrict__ dx_colsum, long long ld_colsum,
                                                            float* __restrict__ ppart /* optional [B][2][C]: per-sample dgamma / dbeta partials */) {
    extern __shared__ double gn_fin_sh[];          // red[256] + tot[3 * cpg] + sg[2]
    double* red = gn_fin_sh;
    double* tot = gn_fin_sh + 256;
    const int b = blockIdx.x, g = blockIdx.y;
    const int cpg = C / G, items = 3 * cpg;        // (plane, channel) pairs of this group; planes: 0 = sum dz xhat, 1 = sum dz, 2 = sum xhat-side term
    double* sg = tot + items;
    const int nsub = items <= 256 ? 256 / items : 1;
    const int t = threadIdx.x;
    for (int base = 0; base < items; base += 256) {          // one trip unless cpg > 85
        const int it = base + (nsub > 1 ? t % items : t), sub = nsub > 1 ? t / items : 0;
        double s = 0.0;
        if (it < items && sub < nsub) {
            const int plane = it / cpg, c = g * cpg + it - plane * cpg;
            const float* p = part + ((long long)b * S * 3 + plane) * C + c;
            for (int sp = sub; sp < S; sp += nsub) s += (double)p[(long long)sp * 3 * C];
        }
        red[t] = s;
        __syncthreads();
        if (base + t < items && t < (nsub > 1 ? items : 256)) {
            double v = red[t];
            for (int k = 1; k < nsub; ++k) v += red[k * items + t];
            tot[base + t] = v;
        }
        __syncthreads();
    }
    if (t < 2) {                                   // t = 0: s1 = sum gamma * plane 1, t = 1: s2 = sum gamma * plane 0
        double v = 0.0;
        const double* q = tot + (t == 0 ? cpg : 0);
        for (int c = 0; c < cpg; ++c) v += q[c] * (double)gamma[g * cpg + c];
        sg[t] = v;
        ds[((long long)b * G + g) * 2 + t] = (float)v;
    }
    if (ppart)
        for (int i = t; i < 2 * cpg; i += 256) {
            const int plane = i / cpg, c = g * cpg + i - plane * cpg;
            ppart[((long long)b * 2 + plane) * C + c] = (float)tot[i];
        }
    if (dx_colsum) {
        __syncthreads();
        const float s1 = (float)sg[0], s2 = (float)sg[1], rs = rstd[b * G + g];
        for (int cl = t; cl < cpg; cl += 256) {
            const int c = g * cpg + cl;
            const float sa = (float)tot[cpg + cl], sh2 = (float)tot[2 * cpg + cl];
            dx_colsum[(long long)b * ld_colsum + c] = rs * (gamma[c] * sa - ((float)HW * s1 + s2 * sh2) * inv_n);
        }
    }
}

// ---- backward apply: dx (+)= rstd * (dz*gamma - (s1 + xhat*s2)/n); grid = (pixel ranges, B), block = (C/4) x r threads
__global__ void gn_bwd_apply_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ dy, long long lddy,
                                    float* __restrict__ dx, long long lddx, int HW, int C, int G, int r, int per,
                                    const float* __restrict__ ds, const float* __restrict__ gamma,
                                    const float* __restrict__ beta, const float* __restrict__ mean,
                                    const float* __restrict__ rstd, float inv_n, int silu, int acc,
                                    unsigned short* __restrict__ dxs, long long lddxs, const float* __restrict__ addp,
                                    long long ldadd, int dxs_c0, int dxs_c1) {
    const int q = C / 4, cpg = C / G;
    const auto [cq, prow, b, p0, p1] = GnSpan(q, HW, per, false);
    GnChan k;      // (its own loop: the group sums between the loads of the constructor; behind them hipcc schedules one s_nop fewer)
    float g1[4], g2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = cq * 4 + j, g = c / cpg;
        k.mu[j] = mean[b * G + g]; k.rs[j] = rstd[b * G + g];
        g1[j] = ds[((long long)b * G + g) * 2]; g2[j] = ds[((long long)b * G + g) * 2 + 1];
        k.gg[j] = gamma[c]; k.bb[j] = beta[c];
    }
    const float* xb = x + (long long)b * HW * ldx + cq * 4;
    const float* db = dy + (long long)b * HW * lddy + cq * 4;
    float* ob = dx + (long long)b * HW * lddx + cq * 4;
    const bool do_acc = dx && acc;
    const float* ab = addp ? addp + (long long)b * HW * ldadd + cq * 4 : xb;
    for (int p = p0 + prow; p < p1; p += 2 * r) {   // two rows of up to four tensors in flight, branch-free
        float4 v[2], d[2], e[2], a2[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool ok = p + u * r < p1;
            v[u] = bd_ld4_if(xb + (long long)(p + u * r) * ldx, ok);
            d[u] = bd_ld4_if(db + (long long)(p + u * r) * lddy, ok);
            e[u] = bd_ld4_if(ob + (long long)(p + u * r) * lddx, ok && do_acc);
            a2[u] = bd_ld4_if(ab + (long long)(p + u * r) * ldadd, ok && addp != nullptr);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float in[4] = {v[u].x, v[u].y, v[u].z, v[u].w}, dd[4] = {d[u].x, d[u].y, d[u].z, d[u].w};
            const float ee[4] = {e[u].x, e[u].y, e[u].z, e[u].w}, aa[4] = {a2[u].x, a2[u].y, a2[u].z, a2[u].w};
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xh = gn_xhat(k, j, in[j]);
                o[j] = (gn_dx_term(k, j, xh, gn_dz(k, j, xh, dd[j], silu), g1[j], g2[j], inv_n) + ee[j]) + aa[j];
            }
            v[u] = make_float4(o[0], o[1], o[2], o[3]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int pu = p + u * r;
            if (pu < p1) {
                if (dx) *reinterpret_cast<float4*>(ob + (long long)pu * lddx) = v[u];
                if (dxs && cq * 4 >= dxs_c0 && cq * 4 < dxs_c1) gn_store_split4(dxs + 2 * ((long long)b * HW + pu) * lddxs, cq * 4 - dxs_c0, v[u]);
            }
        }
    }
}

// =====================================================================================================================
// RESIDENT single-pass kernels: one workgroup = one (sample, cb-channel block), data held in registers
// =====================================================================================================================
constexpr int GN_RES_EMAX = 16;   // float4 per thread per tensor

struct GnRes {
    int cb, q, R, E, nblk, nt;   // channels per block, float4 per pixel row, pixel rows in flight, float4 per thread, blocks, threads
};
static int gcd_i(int a, int b) { return b ? gcd_i(b, a % b) : a; }
// the widest channel block (whole groups, float4-aligned) whose slab fits; then narrower (>= 64 B rows) while the
// grid would leave CUs idle
static bool gn_resident_plan(int B, int HW, int C, int G, GnRes& o, bool wide_ok = false) {
    const int cpg = C / G;
    const int unit = cpg / gcd_i(cpg, 4) * 4;
    for (int nt = 256; nt <= 512; nt *= 2) {   // 512-thread workgroups only where 256 threads cannot hold 64-byte rows
        int best = 0;
        for (int cb = unit; cb <= C; cb += unit) {
            if (C % cb) continue;
            const int q = cb / 4;
            if (q > nt) break;
            if (cdiv(HW, nt / q) <= GN_RES_EMAX && cb / cpg <= 256) best = cb;
        }
        if (!best || (best < 16 && best < C)) continue;   // rows narrower than 64 B: the split kernels coalesce better
        // round 4 (late): a slab whose row pieces are not whole 64-byte halves of a line (12 channels per group at 32 x 32: 24 channels = 96 B rows,
        // 48-byte half planes) writes 1.3 - 1.4x its bytes (PMC, profiles/r04_gn_pmc_by_shape.txt) and runs at 2.8 TB/s: the two-pass kernels,
        // whose rows are whole, are faster there although they read x twice
        constexpr int row_align = 64;
        if ((best * 4) % row_align != 0 && best < C) continue;
        while ((long long)B * (C / best) < 512) {
            const int half = best / 2;
            if (half < 16 || half % unit || C % half) break;
            best = half;
        }
        o.cb = best; o.q = best / 4; o.R = nt / o.q; o.E = (int)cdiv(HW, o.R); o.nblk = C / best; o.nt = nt;
        // the same slab on twice the threads at half the registers each: more waves per CU to hide the three-phase
        // (load, fold, store) latency of a workgroup
        // (measured: backward -10 %, forward neutral, so only the backward asks for it)
        if (wide_ok && nt == 256 && o.E > 8 && 512 % o.q == 0) { o.nt = 512; o.R = 512 / o.q; o.E = (int)cdiv(HW, o.R); }
        return true;
    }
    return false;
}

// 1-D grid over (sample, channel block), remapped so that each XCD (workgroup id % 8) owns a contiguous run with the
// channel blocks of a sample adjacent: the 64-byte row pieces of neighbouring channel blocks share 128-byte lines, and
// this way they meet in one L2 instead of being fetched by two XCDs.  Speed only.
struct GnCoord {
    int b, bx;
};
__device__ __forceinline__ GnCoord gn_res_coord(int nblk) {
    const unsigned L = blockIdx.x, T = gridDim.x, qq = T >> 3;
    unsigned j = (L & 7) * qq + (L >> 3);
    if (L >= (qq << 3)) j = L;   // (an if, not the select of xcd_tile_order(): behind the select these kernels take up to 30 more VGPRs)
    GnCoord c;
    c.b = (int)(j / (unsigned)nblk);
    c.bx = (int)(j - (unsigned)c.b * (unsigned)nblk);
    return c;
}

// a group's statistics to LDS (st, for the apply phase) and to mean / rstd (saved for the backward)
__device__ __forceinline__ void gn_fwd_group_stats(double a, double c2, double n, float eps, float* st, float* mean, float* rstd) {
    float m, r;
    gn_mean_rstd(a, c2, n, eps, &m, &r);
    st[0] = m; st[1] = r;
    *mean = m; *rstd = r;
}

template <int EMAX, int NT>
__global__ __launch_bounds__(NT, NT == 256 ? 4 : 2) void gn_fwd_res_kernel(const float* __restrict__ x, long long ldx, float* __restrict__ y,
                                                       long long ldy, int HW, int C, int G, int cb, int q, int R, int E,
                                                       float eps, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ mean,
                                                       float* __restrict__ rstd, int silu, unsigned short* __restrict__ ys,
                                                       long long ldys) {
    __shared__ double shd[4 * NT];   // [rows][cb][2] per-row channel sums (sum, sumsq), rows*cb <= 4*NT
    float* sh = reinterpret_cast<float*>(shd);   // the float view of the same rows (row pieces wider than a wave)
    __shared__ float st[2 * 256];    // per group of the block: mean, rstd
    const int t = threadIdx.x;
    const int cq = t % q, prow = t / q;
    const bool active = prow < R;
    const GnCoord wgc = gn_res_coord(C / cb);
    const int b = wgc.b, c0 = wgc.bx * cb;
    const int cpg = C / G, ng = cb / cpg;
    const float* xb = x + (long long)b * HW * ldx + c0 + cq * 4;
    float4 v[EMAX];
    float sm[4] = {0.f, 0.f, 0.f, 0.f}, sq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < EMAX; ++i) {
        const int p = prow + R * i;
        const bool ok = active && i < E && p < HW;
        v[i] = bd_ld4_if(xb + (long long)p * ldx, ok);
        sm[0] += v[i].x; sm[1] += v[i].y; sm[2] += v[i].z; sm[3] += v[i].w;
        sq[0] += v[i].x * v[i].x; sq[1] += v[i].y * v[i].y; sq[2] += v[i].z * v[i].z; sq[3] += v[i].w * v[i].w;
    }
    // a wave holds 64/q whole pixel rows when q is a power of two below 64: fold them with shuffles (in double) and
    // hand LDS one row per wave; the serial walk below is then NT/64 rows instead of R
    const bool wred = q < 64 && (q & (q - 1)) == 0;
    const int rows = wred ? NT / 64 : R;
    if (wred) {
        double a[4], c2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { a[j] = (double)sm[j]; c2[j] = (double)sq[j]; }
        for (int off = q; off < 64; off <<= 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { a[j] += __shfl_xor(a[j], off); c2[j] += __shfl_xor(c2[j], off); }
        }
        if ((t & 63) < q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                shd[((t >> 6) * cb + cq * 4 + j) * 2 + 0] = a[j];
                shd[((t >> 6) * cb + cq * 4 + j) * 2 + 1] = c2[j];
            }
        }
    } else if (active) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sh[(prow * cb + cq * 4 + j) * 2 + 0] = sm[j];
            sh[(prow * cb + cq * 4 + j) * 2 + 1] = sq[j];
        }
    }
    __syncthreads();
    if (wred) {
        if (t < ng) {
            double a = 0.0, c2 = 0.0;
            for (int pr = 0; pr < rows; ++pr)
                for (int c = t * cpg; c < (t + 1) * cpg; ++c) {
                    a += shd[(pr * cb + c) * 2 + 0];
                    c2 += shd[(pr * cb + c) * 2 + 1];
                }
            gn_fwd_group_stats(a, c2, (double)HW * cpg, eps, st + 2 * t, mean + b * G + c0 / cpg + t, rstd + b * G + c0 / cpg + t);
        }
    } else {
        // one wave per group: the lanes stride over the group's R x cpg row sums, then fold
        for (int g = t >> 6; g < ng; g += NT / 64) {
            double a = 0.0, c2 = 0.0;
            for (int idx = t & 63; idx < R * cpg; idx += 64) {
                const int pr = idx / cpg, c = g * cpg + idx - pr * cpg;
                a += (double)sh[(pr * cb + c) * 2 + 0];
                c2 += (double)sh[(pr * cb + c) * 2 + 1];
            }
            for (int off = 1; off < 64; off <<= 1) { a += __shfl_xor(a, off); c2 += __shfl_xor(c2, off); }
            if ((t & 63) == 0)
                gn_fwd_group_stats(a, c2, (double)HW * cpg, eps, st + 2 * g, mean + b * G + c0 / cpg + g, rstd + b * G + c0 / cpg + g);
        }
    }
    __syncthreads();
    if (!active) return;
    GnChan k;      // (not gn_chan: the statistics are this block's own, in LDS)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int lc = cq * 4 + j;
        k.mu[j] = st[2 * (lc / cpg)]; k.rs[j] = st[2 * (lc / cpg) + 1];
        k.gg[j] = gamma[c0 + lc]; k.bb[j] = beta[c0 + lc];
    }
    float* yb = y + (long long)b * HW * ldy + c0 + cq * 4;
    // all outputs first (registers only), then the stores: with the arithmetic inside the per-element store branch hipcc
    // waited vmcnt(0) for the previous element's stores before every element
#pragma unroll
    for (int i = 0; i < EMAX; ++i) {
        const float in[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float z = gn_affine(k, j, in[j]);
            o[j] = silu ? silu_fast_pinned(z) : z;
        }
        v[i] = make_float4(o[0], o[1], o[2], o[3]);
    }
#pragma unroll
    for (int i = 0; i < EMAX; ++i) {
        const int p = prow + R * i;
        if (i < E && p < HW) {
            if (y) *reinterpret_cast<float4*>(yb + (long long)p * ldy) = v[i];
            if (ys) gn_store_split4(ys + 2 * ((long long)b * HW + p) * ldys, c0 + cq * 4, v[i]);
        }
    }
}

// backward: dx (+)= rstd * (dz*gamma - (s1 + xhat*s2)/n); per-sample per-channel (sum dz*xhat, sum dz) rows go to
// `part` ([B][2][C], reduced over B by gn_bwd_param_batched_kernel); optional dx_colsum[b][c] = sum over pixels of this
// launch's dx term in closed form: rstd * (gamma*sum dz - (HW*s1 + s2*sum xhat)/n)   (time-embedding gradient)
template <int EMAX, int NT>
__global__ __launch_bounds__(NT) void gn_bwd_res_kernel(const float* __restrict__ x, long long ldx,
                                                       const float* __restrict__ dy, long long lddy, float* __restrict__ dx,
                                                       long long lddx, int HW, int C, int G, int cb, int q, int R, int E,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       int silu, int acc, float* __restrict__ part,
                                                       float* __restrict__ dx_colsum, long long ld_colsum,
                                                       unsigned short* __restrict__ dxs, long long lddxs,
                                                       const float* __restrict__ addp, long long ldadd, int dxs_c0, int dxs_c1) {
    __shared__ float sh[3 * 4 * NT];   // [R][cb][3]: sum dz, sum dz*xhat, sum xhat
    __shared__ float ch[3 * 4 * NT];   // [cb][3] channel totals (cb <= 4*NT)
    __shared__ float sg[2 * 256];    // per group: s1, s2
    const int t = threadIdx.x;
    const int cq = t % q, prow = t / q;
    const bool active = prow < R;
    const GnCoord wgc = gn_res_coord(C / cb);
    const int b = wgc.b, c0 = wgc.bx * cb;
    const int cpg = C / G, ng = cb / cpg;
    const float inv_n = 1.0f / ((float)HW * cpg);
    GnChan k;      // (not gn_chan: an inactive thread reads channel c0 four times; with c0 + j hipcc merges the loads and the code changes)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = c0 + (active ? cq * 4 + j : 0);
        k.mu[j] = mean[b * G + c / cpg]; k.rs[j] = rstd[b * G + c / cpg];
        k.gg[j] = gamma[c]; k.bb[j] = beta[c];
    }
    const float* xb = x + (long long)b * HW * ldx + c0 + cq * 4;
    const float* db = dy + (long long)b * HW * lddy + c0 + cq * 4;
    float4 xh[EMAX], dz[EMAX];
    float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < EMAX; ++i) {
        const int p = prow + R * i;
        const bool ok = active && i < E && p < HW;
        xh[i] = bd_ld4_if(xb + (long long)p * ldx, ok);
        dz[i] = bd_ld4_if(db + (long long)p * lddy, ok);
    }
#pragma unroll
    for (int i = 0; i < EMAX; ++i) {
        const int p = prow + R * i;
        const bool ok = active && i < E && p < HW;
        float in[4] = {xh[i].x, xh[i].y, xh[i].z, xh[i].w}, dd[4] = {dz[i].x, dz[i].y, dz[i].z, dz[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float h = ok ? gn_xhat(k, j, in[j]) : 0.f;
            const float d = gn_dz(k, j, h, dd[j], silu);
            in[j] = h; dd[j] = d;
            s0[j] += d; s1[j] += d * h; s2[j] += h;
        }
        xh[i] = make_float4(in[0], in[1], in[2], in[3]);
        dz[i] = make_float4(dd[0], dd[1], dd[2], dd[3]);
    }
    // pixel rows of one wave folded with shuffles where a wave holds whole rows (see the forward kernel)
    const bool wred = q < 64 && (q & (q - 1)) == 0;
    const int rows = wred ? NT / 64 : R;
    if (wred) {
        for (int off = q; off < 64; off <<= 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s0[j] += __shfl_xor(s0[j], off); s1[j] += __shfl_xor(s1[j], off); s2[j] += __shfl_xor(s2[j], off);
            }
        }
    }
    if (wred ? (t & 63) < q : active) {
        const int row = wred ? (t >> 6) : prow;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float* o = sh + (row * cb + cq * 4 + j) * 3;
            o[0] = s0[j]; o[1] = s1[j]; o[2] = s2[j];
        }
    }
    __syncthreads();
    if (wred) {
        for (int c = t; c < cb; c += NT) {
            float a = 0.f, e = 0.f, h = 0.f;
            for (int pr = 0; pr < rows; ++pr) {
                const float* o = sh + (pr * cb + c) * 3;
                a += o[0]; e += o[1]; h += o[2];
            }
            ch[3 * c] = a; ch[3 * c + 1] = e; ch[3 * c + 2] = h;
            if (part) {   // null: a data-gradient-only backward (no parameter gradients wanted)
                float* o = part + (long long)b * 2 * C + c0 + c;
                o[0] = e;   // plane 0: sum dz * xhat -> dgamma
                o[C] = a;   // plane 1: sum dz        -> dbeta
            }
        }
    } else {
        for (int c = t >> 6; c < cb; c += NT / 64) {   // one wave per channel, lanes stride over the pixel rows
            float a = 0.f, e = 0.f, h = 0.f;
            for (int pr = t & 63; pr < R; pr += 64) {
                const float* o = sh + (pr * cb + c) * 3;
                a += o[0]; e += o[1]; h += o[2];
            }
            for (int off = 1; off < 64; off <<= 1) { a += __shfl_xor(a, off); e += __shfl_xor(e, off); h += __shfl_xor(h, off); }
            if ((t & 63) == 0) {
                ch[3 * c] = a; ch[3 * c + 1] = e; ch[3 * c + 2] = h;
                if (part) {
                    float* o = part + (long long)b * 2 * C + c0 + c;
                    o[0] = e;
                    o[C] = a;
                }
            }
        }
    }
    __syncthreads();
    if (t < ng) {
        double a = 0.0, e = 0.0;
        for (int c = t * cpg; c < (t + 1) * cpg; ++c) {
            a += (double)ch[3 * c] * gamma[c0 + c];
            e += (double)ch[3 * c + 1] * gamma[c0 + c];
        }
        sg[2 * t] = (float)a; sg[2 * t + 1] = (float)e;
    }
    __syncthreads();
    if (dx_colsum) {
        for (int c = t; c < cb; c += NT) {
            const int g = c / cpg;
            const float r = rstd[b * G + (c0 + c) / cpg];
            dx_colsum[(long long)b * ld_colsum + c0 + c] =
                r * (gamma[c0 + c] * ch[3 * c] - ((float)HW * sg[2 * g] + sg[2 * g + 1] * ch[3 * c + 2]) * inv_n);
        }
    }
    if (!active) return;
    float g1[4], g2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int g = (cq * 4 + j) / cpg;
        g1[j] = sg[2 * g]; g2[j] = sg[2 * g + 1];
    }
    float* ob = dx + (long long)b * HW * lddx + c0 + cq * 4;
#pragma unroll
    for (int i = 0; i < EMAX; ++i) {      // dx term into dz[i] (xh[i] is free afterwards)
        const float h[4] = {xh[i].x, xh[i].y, xh[i].z, xh[i].w}, d[4] = {dz[i].x, dz[i].y, dz[i].z, dz[i].w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = gn_dx_term(k, j, h[j], d[j], g1[j], g2[j], inv_n);
        dz[i] = make_float4(o[0], o[1], o[2], o[3]);
    }
    if (dx && acc) {                      // accumulate: the existing dx values, all loads in flight at once
#pragma unroll
        for (int i = 0; i < EMAX; ++i) {
            const int p = prow + R * i;
            xh[i] = bd_ld4_if(ob + (long long)p * lddx, i < E && p < HW);
        }
#pragma unroll
        for (int i = 0; i < EMAX; ++i) { dz[i].x += xh[i].x; dz[i].y += xh[i].y; dz[i].z += xh[i].z; dz[i].w += xh[i].w; }
    }
    if (addp) {                           // + a second gradient (the resnet's identity shortcut), after the accumulation
        const float* ab = addp + (long long)b * HW * ldadd + c0 + cq * 4;
#pragma unroll
        for (int i = 0; i < EMAX; ++i) {
            const int p = prow + R * i;
            xh[i] = bd_ld4_if(ab + (long long)p * ldadd, i < E && p < HW);
        }
#pragma unroll
        for (int i = 0; i < EMAX; ++i) { dz[i].x += xh[i].x; dz[i].y += xh[i].y; dz[i].z += xh[i].z; dz[i].w += xh[i].w; }
    }
#pragma unroll
    for (int i = 0; i < EMAX; ++i) {
        const int p = prow + R * i;
        if (i < E && p < HW) {
            if (dx) *reinterpret_cast<float4*>(ob + (long long)p * lddx) = dz[i];
            // planes of the FINAL value, channels [dxs_c0, dxs_c1) only
            if (dxs && c0 + cq * 4 >= dxs_c0 && c0 + cq * 4 < dxs_c1) gn_store_split4(dxs + 2 * ((long long)b * HW + p) * lddxs, c0 + cq * 4 - dxs_c0, dz[i]);
        }
    }
}

// =====================================================================================================================
// Host: the shape predicate, the plan, the workspace layout
// =====================================================================================================================
// The shape predicate, in two levels: a shape these kernels are written for (what bd_gn_fwd_takes_stats / bd_gn_bwd_defers answer for), and
// on top of it the launch limits (block <= 1024 threads, grid.y <= 65535) that the launchers and bd_gn_plan add.
static bool gn_shape_ok(int B, int HW, int C, int G) { return B > 0 && HW > 0 && C > 0 && G > 0 && C % G == 0 && (C & 3) == 0; }
static bool gn_launch_ok(int B, int C) { return C / 4 <= 1024 && B <= 65535; }
// both levels for the launchers: the message names the part that failed
static int gn_common_checks(const char* who, int B, int HW, int C, int G, const void* x, long long ldx) {
    if (!gn_shape_ok(B, HW, C, G)) {
        BD_CHECK(B > 0 && HW > 0 && C > 0 && G > 0, BD_ERR_INVALID, "%s: bad shape", who);
        BD_CHECK(C % G == 0, BD_ERR_INVALID, "%s: C=%d not divisible by G=%d", who, C, G);
    }
    BD_CHECK(gn_shape_ok(B, HW, C, G) && (ldx & 3) == 0 && aligned16(x), BD_ERR_UNSUPPORTED,
             "%s: needs C and ld multiples of 4 and a 16B-aligned pointer (C=%d ld=%lld)", who, C, ldx);
    if (!gn_launch_ok(B, C)) {
        BD_CHECK(C / 4 <= 1024, BD_ERR_UNSUPPORTED, "%s: C=%d too large", who, C);
        BD_CHECK(B <= 65535, BD_ERR_UNSUPPORTED, "%s: B=%d too large", who, B);
    }
    return BD_OK;
}

constexpr int GN_MAX_SPLITS = 128;   // small batches of large images (B = 4 at 256x256) need the pixel splits to fill the chip
static int gn_max_splits(int B) {
    const int s = 512 / (B > 0 ? B : 1);
    return s < 1 ? 1 : (s > GN_MAX_SPLITS ? GN_MAX_SPLITS : s);
}
static int gn_splits(int B, int HW) {
    int s = gn_max_splits(B);
    while (s > 1 && HW / s < 32) s >>= 1;
    return s;
}

// Everything the launchers decide from a level-1 shape, decided once (DESIGN.md "GroupNorm dispatch"): bd_gn_fwd, bd_gn_bwd and the three
// queries read it, and bd_gn_plan reports it.
struct GnPlan {
    int B, HW, C, G;
    bool resident;
    GnRes res; int emax, nt;    // resident: the slab and the <EMAX, NT> of gn_fwd_res_kernel / gn_bwd_res_kernel, the smallest register array that holds E
    int S, threads, r, per;     // two-stage: pixel splits; threads = (C/4) * r, r pixel rows in flight; pixel rows per block of the apply kernels
};
static GnPlan gn_plan(int B, int HW, int C, int G, bool backward) {
    GnPlan p = {};
    p.B = B; p.HW = HW; p.C = C; p.G = G;
    p.resident = gn_resident_plan(B, HW, C, G, p.res, backward);
    if (p.resident) {
        p.nt = p.res.nt == 512 ? 512 : 256;
        p.emax = p.nt == 512 ? (p.res.E <= 8 ? 8 : GN_RES_EMAX) : (p.res.E <= 4 ? 4 : GN_RES_EMAX);
        return p;
    }
    p.S = gn_splits(B, HW);
    const int q = C / 4;
    p.r = 256 / q < 1 ? 1 : 256 / q;
    p.threads = q * p.r;
    long long per = 16LL * p.r;     // 16 rows per thread (four / eight trips of the unrolled loop), at most 65535 blocks
    while (cdiv(HW, per) > 65535) per *= 2;
    p.per = (int)per;
    return p;
}
// f(integral_constant EMAX, integral_constant NT) for the plan's instantiation, one of <4,256> <16,256> <8,512> <16,512>
template <class F>
static void gn_res_dispatch(const GnPlan& p, F&& f) {
    using std::integral_constant;
    if (p.nt == 512 && p.emax == 8) f(integral_constant<int, 8>{}, integral_constant<int, 512>{});
    else if (p.nt == 512) f(integral_constant<int, GN_RES_EMAX>{}, integral_constant<int, 512>{});
    else if (p.emax == 4) f(integral_constant<int, 4>{}, integral_constant<int, 256>{});
    else f(integral_constant<int, GN_RES_EMAX>{}, integral_constant<int, 256>{});
}

// ---- workspace: one layout per direction; the launcher's check, its message and its pointers read these, and so does bd_gn_plan
// forward: the two-stage statistics [B][S][G][2] fp64; resident: nothing
static size_t gn_fwd_workspace(const GnPlan& p) { return p.resident ? 0 : gn_stats_partial_bytes(p.B, p.S, p.G); }
// backward two-stage: the statistics rows `part` [B][S][3][C] fp32 (256-aligned), then `ds` [B][G][2] fp32; resident: the per-sample
// parameter partials `part` [B][2][C] fp32, only when the launcher owns the parameter sums (no param_partials, dgamma / dbeta wanted)
struct GnBwdWs { size_t ds, bytes; };   // offset of ds, total
static GnBwdWs gn_bwd_workspace(const GnPlan& p, bool owns_params) {
    if (p.resident) return {0, owns_params ? (size_t)p.B * p.C * 2 * sizeof(float) : 0};
    const size_t ds = align_up((size_t)p.B * p.S * p.C * 3 * sizeof(float), 256);
    return {ds, ds + (size_t)p.B * p.G * 2 * sizeof(float)};
}

}  // namespace bd

using namespace bd;

// A bound, not a need: >= gn_fwd_workspace / gn_bwd_workspace of every (HW, G) the launchers take at this (B, C), from S <= gn_max_splits(B)
// and G <= C (tests/test_workspace_host.py).  The UNet plan's dry run sizes its op workspace with it.
extern "C" size_t bd_gn_workspace_bytes(int B, int C) {
    const size_t ms = (size_t)gn_max_splits(B);
    const size_t fwd = gn_stats_partial_bytes(B, (int)ms, C);
    const size_t bwd = (size_t)B * ms * (size_t)C * 3 * sizeof(float) + 256 + (size_t)B * C * 2 * sizeof(float);
    return fwd > bwd ? fwd : bwd;
}

extern "C" int bd_gn_fwd(const bd_gn_fwd_desc* d, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_gn_fwd: null descriptor");
    BD_TRY(gn_common_checks("bd_gn_fwd", d->B, d->HW, d->C, d->G, d->x, d->ldx));
    BD_CHECK(d->gamma && d->beta && (d->y || d->y_split) && d->mean && d->rstd && d->workspace, BD_ERR_INVALID, "bd_gn_fwd: null pointer");
    BD_CHECK((d->ldy & 3) == 0 && aligned16(d->y) && aligned16(d->gamma) && aligned16(d->beta), BD_ERR_UNSUPPORTED,
             "bd_gn_fwd: y/gamma/beta must be 16B aligned, ldy multiple of 4");
    BD_CHECK(!d->y_split || (d->C % 32 == 0 && d->ldys % 32 == 0 && ((uintptr_t)d->y_split & 127) == 0), BD_ERR_UNSUPPORTED,
             "bd_gn_fwd: y_split needs C %% 32 == 0, ldys %% 32 == 0 and a 128-byte aligned base");
    const GnPlan p = gn_plan(d->B, d->HW, d->C, d->G, false);
    const size_t need = gn_fwd_workspace(p);
    BD_CHECK(d->workspace_bytes >= need, BD_ERR_WORKSPACE, "bd_gn_fwd: workspace %zu < %zu", d->workspace_bytes, need);
    if (p.resident) {
        const dim3 grid((unsigned)p.res.nblk * (unsigned)d->B);
        int rec = -1;       // round 6: the resident GroupNorm launches are profiled classes too (REQUIRED bytes: x in, y and / or planes out)
        if (prof_on())
            rec = prof_begin("gn_fwd_res", 0.0, (double)d->B * d->HW * d->C * 4.0 * (1.0 + (d->y ? 1.0 : 0.0) + (d->y_split ? 1.0 : 0.0)), S(stream));
        gn_res_dispatch(p, [&](auto em, auto nt) {
            constexpr int EM = decltype(em)::value, NT = decltype(nt)::value;
            hipLaunchKernelGGL((gn_fwd_res_kernel<EM, NT>), grid, dim3(NT), 0, S(stream), d->x, (long long)d->ldx, d->y, (long long)d->ldy,
                               d->HW, d->C, d->G, p.res.cb, p.res.q, p.res.R, p.res.E, d->eps, d->gamma, d->beta, d->mean, d->rstd, d->silu,
                               d->y_split, (long long)d->ldys);
        });
        BD_LAUNCH_CHECK("gn_fwd_res");
        prof_end(rec, S(stream));
        return BD_OK;
    }
    const double* part = reinterpret_cast<double*>(d->workspace);
    int Sf = p.S;
    if (d->stats) {           // round 4: the producer of x left the partials (bd_conv3x3_ps gn_part): no pass over x
        BD_CHECK(d->stats_splits > 0, BD_ERR_INVALID, "bd_gn_fwd: stats without stats_splits");
        part = d->stats; Sf = d->stats_splits;
    } else {
        hipLaunchKernelGGL(gn_stats_kernel, dim3(p.S, d->B), dim3(p.threads), (size_t)p.r * d->C * 2 * sizeof(float), S(stream), d->x,
                           (long long)d->ldx, d->HW, d->C, d->G, p.r, p.S, reinterpret_cast<double*>(d->workspace));
        BD_LAUNCH_CHECK("gn_stats");
    }
    hipLaunchKernelGGL(gn_fwd_finalize_kernel, dim3(d->B), dim3(256), 0, S(stream), part, d->G, Sf, (double)d->HW * (d->C / d->G), d->eps,
                       d->mean, d->rstd);
    hipLaunchKernelGGL(gn_apply_kernel, dim3((unsigned)cdiv(d->HW, p.per), d->B), dim3(p.threads), 0, S(stream), d->x, (long long)d->ldx,
                       d->y, (long long)d->ldy, d->HW, d->C, d->G, p.r, p.per, d->gamma, d->beta, d->mean, d->rstd, d->silu, d->y_split,
                       (long long)d->ldys);
    BD_LAUNCH_CHECK("gn_apply");
    return BD_OK;
}

extern "C" int bd_gn_fwd_takes_stats(int B, int HW, int C, int G) {
    return gn_shape_ok(B, HW, C, G) && !gn_plan(B, HW, C, G, false).resident ? 1 : 0;
}

extern "C" int bd_gn_bwd_defers(int B, int HW, int C, int G) {
    // round 4: both the resident and the large-image path leave per-sample partials to the caller
    return gn_shape_ok(B, HW, C, G) ? 1 : 0;
}

extern "C" int bd_gn_plan(int B, int HW, int C, int G, int backward, bd_gn_plan_info* out) {
    // host only: what bd_gn_fwd / bd_gn_bwd themselves read to choose their kernels and lay their workspace out, nothing else
    BD_CHECK(out, BD_ERR_INVALID, "bd_gn_plan: null output");
    BD_CHECK(gn_shape_ok(B, HW, C, G) && gn_launch_ok(B, C), BD_ERR_INVALID,
             "bd_gn_plan: not a shape bd_gn_fwd / bd_gn_bwd take (B=%d HW=%d C=%d G=%d)", B, HW, C, G);
    const GnPlan p = gn_plan(B, HW, C, G, backward != 0);
    *out = bd_gn_plan_info{};
    out->resident = p.resident;
    out->nt = p.nt; out->cb = p.res.cb; out->q = p.res.q; out->R = p.res.R; out->E = p.res.E; out->emax = p.emax;
    out->S = p.S; out->threads = p.threads; out->r = p.r; out->per = p.per;
    out->workspace_bytes = backward ? gn_bwd_workspace(p, true).bytes : gn_fwd_workspace(p);
    return BD_OK;
}

// dgamma / dbeta of n layers from `rows` partial rows each (row stride planes * C floats), GN_PARAM_MAX layers per launch
static int gn_fold_params(const bd_gn_param_item* items, int n, int rows, int planes, hipStream_t st) {
    for (int i0 = 0; i0 < n; i0 += GN_PARAM_MAX) {
        GnParamTable t;
        t.n = n - i0 < GN_PARAM_MAX ? n - i0 : GN_PARAM_MAX;
        int blk = 0;
        for (int i = 0; i < t.n; ++i) {
            const bd_gn_param_item& it = items[i0 + i];
            BD_CHECK(it.partials && it.dgamma && it.dbeta && it.C > 0, BD_ERR_INVALID, "bd_gn_bwd_params: item %d", i0 + i);
            t.part[i] = it.partials; t.dg[i] = it.dgamma; t.db[i] = it.dbeta; t.C[i] = it.C; t.stride[i] = planes * it.C; t.blk0[i] = blk;
            blk += (int)cdiv(2 * it.C, 64);
        }
        t.blk0[t.n] = blk;
        hipLaunchKernelGGL(gn_bwd_param_batched_kernel, dim3((unsigned)blk), dim3(1024), 0, st, t, rows);
        BD_LAUNCH_CHECK("gn_bwd_param_batched");
    }
    return BD_OK;
}

extern "C" int bd_gn_bwd_params(const bd_gn_param_item* items, int n, int B, bd_stream_t stream) {
    BD_CHECK(items && n > 0 && B > 0, BD_ERR_INVALID, "bd_gn_bwd_params: bad arguments");
    return gn_fold_params(items, n, B, 2, S(stream));
}

extern "C" int bd_gn_bwd(const bd_gn_bwd_desc* d, bd_stream_t stream) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_gn_bwd: null descriptor");
    BD_TRY(gn_common_checks("bd_gn_bwd", d->B, d->HW, d->C, d->G, d->x, d->ldx));
    BD_CHECK(d->gamma && d->beta && d->mean && d->rstd && d->dy && (d->dx || d->dx_split) && d->workspace,
             BD_ERR_INVALID, "bd_gn_bwd: null pointer");
    // dgamma == dbeta == param_partials == NULL: no parameter gradient is computed or written (the data gradient is the same launch, bit for bit)
    const bool no_params = !d->dgamma && !d->dbeta && !d->param_partials;
    BD_CHECK(no_params || (d->dgamma && d->dbeta), BD_ERR_INVALID, "bd_gn_bwd: dgamma and dbeta go together (both null with null param_partials = no parameter gradients)");
    BD_CHECK(!d->dx_split || (d->C % 32 == 0 && d->lddxs % 32 == 0 && ((uintptr_t)d->dx_split & 127) == 0), BD_ERR_UNSUPPORTED,
             "bd_gn_bwd: dx_split needs C %% 32 == 0, lddxs %% 32 == 0 and a 128-byte aligned base");
    const int xs0 = d->dx_split_c1 > d->dx_split_c0 ? d->dx_split_c0 : 0, xs1 = d->dx_split_c1 > d->dx_split_c0 ? d->dx_split_c1 : d->C;
    BD_CHECK(!d->dx_split || (xs0 >= 0 && xs1 <= d->C && xs0 % 32 == 0 && xs1 % 32 == 0 && d->lddxs >= xs1 - xs0), BD_ERR_INVALID,
             "bd_gn_bwd: dx_split channel range [%d, %d) must be whole 32-channel blocks inside C = %d with lddxs >= its width", xs0, xs1, d->C);
    BD_CHECK(d->dx || !d->accumulate_dx, BD_ERR_INVALID, "bd_gn_bwd: accumulate_dx needs dx");
    BD_CHECK((d->lddy & 3) == 0 && (d->lddx & 3) == 0 && aligned16(d->dy) && aligned16(d->dx) && aligned16(d->gamma) &&
                 aligned16(d->beta), BD_ERR_UNSUPPORTED, "bd_gn_bwd: pointers must be 16B aligned, ld multiples of 4");
    BD_CHECK(!(d->dx_colsum && (d->accumulate_dx || d->dx_add)), BD_ERR_INVALID, "bd_gn_bwd: dx_colsum is the column sum of this launch's dx term alone");
    BD_CHECK(!d->dx_add || (d->dx && (d->ld_add & 3) == 0 && aligned16(d->dx_add)), BD_ERR_INVALID, "bd_gn_bwd: dx_add needs dx, a 16B-aligned pointer and ld_add %% 4 == 0");
    const GnPlan p = gn_plan(d->B, d->HW, d->C, d->G, true);
    const bool owns_params = !d->param_partials && !no_params;   // else the caller folds them (bd_gn_bwd_params) / nobody wants them
    const GnBwdWs ws = gn_bwd_workspace(p, owns_params);
    BD_CHECK(d->workspace_bytes >= ws.bytes, BD_ERR_WORKSPACE, "bd_gn_bwd: workspace %zu < %zu", d->workspace_bytes, ws.bytes);
    float* part = reinterpret_cast<float*>(d->workspace);
    float* ds = reinterpret_cast<float*>(reinterpret_cast<char*>(d->workspace) + ws.ds);
    const bd_gn_param_item own = {part, d->C, d->dgamma, d->dbeta};
    if (p.resident) {
        float* part_r = d->param_partials ? d->param_partials : (no_params ? nullptr : part);
        const dim3 grid((unsigned)p.res.nblk * (unsigned)d->B);
        int rec = -1;       // REQUIRED bytes of this call: x and dy in (+ the dx it accumulates into, + the added gradient), dx and / or its planes out
        if (prof_on())
            rec = prof_begin("gn_bwd_res", 0.0, (double)d->B * d->HW * 4.0 * ((double)d->C * (2.0 + (d->accumulate_dx ? 1.0 : 0.0) + (d->dx_add ? 1.0 : 0.0) +
                             (d->dx ? 1.0 : 0.0)) + (d->dx_split ? (double)(xs1 - xs0) : 0.0)), S(stream));
        gn_res_dispatch(p, [&](auto em, auto nt) {
            constexpr int EM = decltype(em)::value, NT = decltype(nt)::value;
            hipLaunchKernelGGL((gn_bwd_res_kernel<EM, NT>), grid, dim3(NT), 0, S(stream), d->x, (long long)d->ldx, d->dy, (long long)d->lddy,
                               d->dx, (long long)d->lddx, d->HW, d->C, d->G, p.res.cb, p.res.q, p.res.R, p.res.E, d->gamma, d->beta, d->mean,
                               d->rstd, d->silu, d->accumulate_dx, part_r, d->dx_colsum, (long long)d->ld_colsum, d->dx_split,
                               (long long)d->lddxs, d->dx_add, (long long)d->ld_add, xs0, xs1);
        });
        BD_LAUNCH_CHECK("gn_bwd_res");
        prof_end(rec, S(stream));
        return owns_params ? gn_fold_params(&own, 1, d->B, 2, S(stream)) : BD_OK;       // rows [B][2][C]
    }
    hipLaunchKernelGGL(gn_bwd_stats_kernel, dim3(p.S, d->B), dim3(p.threads), (size_t)p.r * d->C * 3 * sizeof(float), S(stream), d->x,
                       (long long)d->ldx, d->dy, (long long)d->lddy, d->HW, d->C, d->G, p.r, p.S, d->gamma, d->beta, d->mean, d->rstd,
                       d->silu, part);
    BD_LAUNCH_CHECK("gn_bwd_stats");
    if (owns_params) BD_TRY(gn_fold_params(&own, 1, d->B * p.S, 3, S(stream)));          // rows [B*S][3][C]
    const float inv_n = 1.0f / ((float)d->HW * (d->C / d->G));
    hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(d->B, (unsigned)d->G), dim3(256), (size_t)(256 + 3 * (d->C / d->G) + 2) * sizeof(double),
                       S(stream), part, d->HW, d->C, d->G, p.S, d->gamma, d->rstd, inv_n, ds, d->dx_colsum, (long long)d->ld_colsum,
                       d->param_partials);
    hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3((unsigned)cdiv(d->HW, p.per), d->B), dim3(p.threads), 0, S(stream), d->x, (long long)d->ldx,
                       d->dy, (long long)d->lddy, d->dx, (long long)d->lddx, d->HW, d->C, d->G, p.r, p.per, ds, d->gamma, d->beta, d->mean,
                       d->rstd, inv_n, d->silu, d->accumulate_dx, d->dx_split, (long long)d->lddxs, d->dx_add, (long long)d->ld_add, xs0, xs1);
    BD_LAUNCH_CHECK("gn_bwd_apply");
    return BD_OK;
}
