// Measure path (SURVEY f-3): structural similarity of two image batches on the device.
// Reference call site: baddiffusion.py:536-547, StructuralSimilarityIndexMeasure(data_range=1.0) on [N,3,S,S] images in
// [0,1]; the published torchmetrics defaults are restated (11x11 Gaussian window, sigma 1.5, k1 0.01, k2 0.03, reflect
// padding of (k-1)/2, the padded border cropped from the map, mean over C,H,W then over the batch).  torchmetrics is not
// in the build container: parity is pinned against baddiffusion_amd/metrics.py's CPU restatement only.
//
// One workgroup = one 32x32 tile of the SSIM map of one (image, channel): the (32+10)^2 input patch of both images goes to
// LDS (reflect indexing at the image border), the separable window runs as a horizontal pass over five quantities
// (p, t, p^2, t^2, p*t) into LDS and a vertical pass from LDS, the map values inside the cropped region are summed in
// fp64 (fixed order) into one partial per workgroup; a second single-workgroup kernel folds the partials and divides.
// HBM-bound: 8 B read per pixel and image pair.
#include "common.h"

namespace bd {

constexpr int SS_T = 32, SS_K = 11, SS_PAD = 5, SS_P = SS_T + 2 * SS_PAD;   // tile, window, halo, patch edge (42)

struct SsimWin { float g[SS_K]; };

__device__ __forceinline__ int ss_reflect(int i, int n) {   // F.pad(mode="reflect"): -k -> k, n-1+k -> n-1-k
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

// The fold of every reduction in this file: a fixed tree over the 256 per-thread sums; the result is valid on thread 0
__device__ __forceinline__ double block_sum256(double acc, double* red) {
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// The tile routine of bd_ssim and bd_ssim_images: the sum of the SSIM map over the tile at (y0, x0) of one H x W plane pair (p, t: the
// plane's element (0, 0); row / column strides psh, psw and tsh, tsw), valid on thread 0.  256 threads, all of them must call it.
__device__ __forceinline__ double ssim_tile_sum(const float* __restrict__ p, long long psh, long long psw, const float* __restrict__ t,
                                                long long tsh, long long tsw, int H, int W, int y0, int x0, float c1, float c2,
                                                const SsimWin& win) {
    __shared__ float sp[SS_P][SS_P + 1], st[SS_P][SS_P + 1];
    __shared__ float hb[5][SS_P][SS_T + 1];
    __shared__ double red[256];
    const int tid = threadIdx.x;
    for (int i = tid; i < SS_P * SS_P; i += 256) {
        const int r = i / SS_P, q = i - r * SS_P;
        int y = y0 - SS_PAD + r, x = x0 - SS_PAD + q;
        float a = 0.f, b = 0.f;
        if (y < H + SS_PAD && x < W + SS_PAD) {   // inside the padded image (ragged last tiles read nothing beyond it)
            y = ss_reflect(y, H); x = ss_reflect(x, W);
            a = p[y * psh + x * psw]; b = t[y * tsh + x * tsw];
        }
        sp[r][q] = a; st[r][q] = b;
    }
    __syncthreads();
    for (int i = tid; i < SS_P * SS_T; i += 256) {          // horizontal pass: 42 rows x 32 columns x 5 quantities
        const int r = i / SS_T, q = i - r * SS_T;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
        for (int u = 0; u < SS_K; ++u) {
            const float a = sp[r][q + u], b = st[r][q + u], g = win.g[u];
            s0 += g * a; s1 += g * b; s2 += g * (a * a); s3 += g * (b * b); s4 += g * (a * b);
        }
        hb[0][r][q] = s0; hb[1][r][q] = s1; hb[2][r][q] = s2; hb[3][r][q] = s3; hb[4][r][q] = s4;
    }
    __syncthreads();
    double acc = 0.0;
    for (int i = tid; i < SS_T * SS_T; i += 256) {          // vertical pass + the SSIM map value
        const int r = i / SS_T, q = i - r * SS_T;
        const int y = y0 + r, x = x0 + q;
        if (y < SS_PAD || y >= H - SS_PAD || x < SS_PAD || x >= W - SS_PAD) continue;   // the cropped border (and ragged tiles)
        float mp = 0.f, mt = 0.f, pp = 0.f, tt = 0.f, pt = 0.f;
#pragma unroll
        for (int u = 0; u < SS_K; ++u) {
            const float g = win.g[u];
            mp += g * hb[0][r + u][q]; mt += g * hb[1][r + u][q]; pp += g * hb[2][r + u][q]; tt += g * hb[3][r + u][q];
            pt += g * hb[4][r + u][q];
        }
        const float vp = pp - mp * mp, vt = tt - mt * mt, cv = pt - mp * mt;
        const float v = ((2.f * mp * mt + c1) * (2.f * cv + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2));
        acc += (double)v;
    }
    return block_sum256(acc, red);
}

__global__ __launch_bounds__(256) void ssim_tile_kernel(const float* __restrict__ p, const float* __restrict__ t, int C, int H, int W,
                                                        long long sn, long long sc, long long sh, long long sw, float c1, float c2,
                                                        SsimWin win, double* __restrict__ partial) {
    const int nc = blockIdx.z, n = nc / C, c = nc - n * C;
    const long long base = (long long)n * sn + (long long)c * sc;
    const double r = ssim_tile_sum(p + base, sh, sw, t + base, sh, sw, H, W, blockIdx.y * SS_T, blockIdx.x * SS_T, c1, c2, win);
    if (threadIdx.x == 0) partial[((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = r;
}

__global__ __launch_bounds__(256) void ssim_final_kernel(const double* __restrict__ partial, long long n, double inv_count, float* __restrict__ out) {
    __shared__ double red[256];
    double a = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) a += partial[i];
    const double r = block_sum256(a, red);
    if (threadIdx.x == 0) out[0] = (float)(r * inv_count);
}

// ---- per-image scores (bd_image_loss, bd_ssim_images; DESIGN.md section 3, "Per-image scores") ----------------------------------------------------
// Both images of a pair by element strides; the target's may be 0 (broadcast).  Every sum below is ordered by (C, H, W) and the logical
// index (c, h, w) alone: an image's workgroups and their partials never depend on N, on the image's place in the batch or on the strides.
struct ImgPair {
    int C, H, W;
    const float* p; long long ps[4];
    const float* t; long long ts[4];
};
constexpr int IL_CHUNK = 8192;   // logical elements per workgroup of image_loss_kernel: 32 per thread

// grid (nchunk, images of this launch): workgroup (k, j) sums elements [k * IL_CHUNK, (k + 1) * IL_CHUNK) of image n0 + j.  Thread t walks
// t, t + 256, ... of the chunk; its (c, h, w) is divided out once and then advanced by 256 = dc * H * W + dh * W + dw (host values).
__global__ __launch_bounds__(256) void image_loss_kernel(ImgPair d, int n0, int type, unsigned total, int nchunk, unsigned dc, unsigned dh,
                                                         unsigned dw, double* __restrict__ part, float* __restrict__ out) {
    __shared__ double red[256];
    const long long n = (long long)n0 + blockIdx.y;
    const float* __restrict__ p = d.p + n * d.ps[0];
    const float* __restrict__ t = d.t + n * d.ts[0];
    const unsigned H = (unsigned)d.H, W = (unsigned)d.W;
    const unsigned beg = blockIdx.x * (unsigned)IL_CHUNK + threadIdx.x;
    const unsigned end = total - blockIdx.x * (unsigned)IL_CHUNK < (unsigned)IL_CHUNK ? total : (blockIdx.x + 1u) * (unsigned)IL_CHUNK;
    unsigned q = beg / W, w = beg - q * W, c = q / H, h = q - c * H;
    double acc = 0.0;
#pragma unroll 4
    for (unsigned i = beg; i < end; i += 256) {          // (unrolled: the loads of four steps are in flight together; the adds keep their order)
        const float df = p[c * d.ps[1] + h * d.ps[2] + w * d.ps[3]] - t[c * d.ts[1] + h * d.ts[2] + w * d.ts[3]];
        float l, g;
        loss_elem(type, df, l, g);
        acc += (double)l;
        w += dw;
        if (w >= W) { w -= W; ++h; }
        h += dh; c += dc;
        if (h >= H) { h -= H; ++c; }
    }
    const double r = block_sum256(acc, red);
    if (threadIdx.x == 0) {
        if (nchunk == 1) out[n] = (float)(r / (double)total);
        else part[n * nchunk + blockIdx.x] = r;
    }
}

// grid (tiles x, tiles y, planes of this launch): the tile of plane z0 + blockIdx.z, its sum to partial[plane][tile row][tile column]
__global__ __launch_bounds__(256) void ssim_images_tile_kernel(ImgPair d, long long z0, float c1, float c2, SsimWin win,
                                                               double* __restrict__ partial) {
    const long long nc = z0 + blockIdx.z, n = nc / d.C, c = nc - n * d.C;
    const double r = ssim_tile_sum(d.p + n * d.ps[0] + c * d.ps[1], d.ps[2], d.ps[3], d.t + n * d.ts[0] + c * d.ts[1], d.ts[2], d.ts[3],
                                   d.H, d.W, blockIdx.y * SS_T, blockIdx.x * SS_T, c1, c2, win);
    if (threadIdx.x == 0) partial[(nc * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = r;
}

// What bd_vb_terms makes of an image's mean m: bits = (add[t] + mul[t] * m) / ln 2, in fp64, rounded to fp32 once
struct VbFinish { const long long* t; const float* add; const float* mul; int T; };
__device__ __forceinline__ float vb_finish(const VbFinish& f, long long n, double mean) {
    const long long t = f.t[n];
    if (t < 0 || t > f.T) return __builtin_nanf("");
    return (float)(((double)f.add[t] + (double)f.mul[t] * mean) * 1.4426950408889634074);
}

// one workgroup per image: out[n] = (float)(sum of the image's `per` partials / count), thread-strided and through the tree (index order);
// VB: the mean goes through vb_finish instead
template <bool VB>
__global__ __launch_bounds__(256) void image_fold_kernel(const double* __restrict__ partial, int per, double count, float* __restrict__ out,
                                                         VbFinish f) {
    __shared__ double red[256];
    const double* __restrict__ q = partial + (long long)blockIdx.x * per;
    double a = 0.0;
    for (int i = threadIdx.x; i < per; i += 256) a += q[i];
    const double r = block_sum256(a, red);
    if (threadIdx.x == 0) out[blockIdx.x] = VB ? vb_finish(f, blockIdx.x, r / count) : (float)(r / count);
}

// ---- variational-bound terms (bd_vb_terms; DESIGN.md section 3, "Bits per dimension") ---------------------------------------------------------------
// The reduction of image_loss_kernel over three streams.  A workgroup belongs to one image, hence to one t: the row kind is uniform and a
// KL or prior workgroup never enters the erfc path.  The t = 0 element is evaluated in fp64 (difference, z, erfc, log): the kernel is
// bound by its 12 B per element, the fp64 path is taken by one row in T + 1 of a full evaluation, and it leaves the all-floor case exact.
struct VbArgs {
    int C, H, W, clip;
    const float* x0; long long s0[4];
    const float* xt; long long st[4];
    const float* ep; long long se[4];
    const float* ac;
    double inv_sigma;
    VbFinish f;
};
enum { VB_KL = 0, VB_DEC = 1, VB_PRIOR = 2 };
// bd_vb_terms_shift: the fourth stream r and the table g ("The bound along the backdoored chain").  The unshifted
// kernel's arguments are VbArgs alone, so bd_vb_terms is the code it was.
template <bool SHIFT> struct VbArgsT : VbArgs {};
template <> struct VbArgsT<true> : VbArgs { const float* r; long long sr[4]; const float* g; };

// -log P of the discretised Gaussian decoder (bd_hip.h): both erfc arguments on the tail side, the floor by comparison (fmax would drop a NaN)
__device__ __forceinline__ double vb_dec_nll(float x0, float xh, double inv_sigma) {
    const double r2 = 0.70710678118654752440;
    const double df = (double)x0 - (double)xh;
    const double zp = (df + 1.0 / 255.0) * inv_sigma, zm = (df - 1.0 / 255.0) * inv_sigma;
    const bool lo = (double)x0 < -0.999, hi = (double)x0 > 0.999, tail = zm > 0.0;
    const double a = lo ? -zp : (hi || tail) ? zm : -zp;
    const double b = tail ? zp : -zm;
    const double eb = erfc(b * r2);
    double P = 0.5 * (erfc(a * r2) - ((lo || hi) ? 0.0 : eb));
    P = P < 1e-12 ? 1e-12 : P;
    return -log(P);
}

// the walk of image_loss_kernel for one row kind: the workgroup's sum of the term's elements (and of (x0 - x0_hat)^2 when MSE), on thread 0.
// SHIFT: a KL row's element is ((x0 + g[t] * r) - x0_hat)^2, a prior row's (x0 - r)^2; a t = 0 row does not read r.
template <int KIND, bool MSE, bool SHIFT>
__device__ __forceinline__ void vb_walk(const VbArgsT<SHIFT>& d, long long n, int t, unsigned total, unsigned dc, unsigned dh, unsigned dw,
                                        double* red, double& sum, double& sq) {
    const float* __restrict__ p0 = d.x0 + n * d.s0[0];
    const float* __restrict__ pt = KIND == VB_PRIOR ? nullptr : d.xt + n * d.st[0];
    const float* __restrict__ pe = KIND == VB_PRIOR ? nullptr : d.ep + n * d.se[0];
    const float* __restrict__ pr = nullptr;
    float g = 0.f;
    if constexpr (SHIFT) {
        if (KIND != VB_DEC) pr = d.r + n * d.sr[0];
        if (KIND == VB_KL) g = d.g[t];
    }
    X0Coef k = {0.f, 1.f};
    if (KIND != VB_PRIOR) k = x0_coef(d.ac, t);
    const unsigned H = (unsigned)d.H, W = (unsigned)d.W;
    const unsigned beg = blockIdx.x * (unsigned)IL_CHUNK + threadIdx.x;
    const unsigned end = total - blockIdx.x * (unsigned)IL_CHUNK < (unsigned)IL_CHUNK ? total : (blockIdx.x + 1u) * (unsigned)IL_CHUNK;
    unsigned q = beg / W, w = beg - q * W, c = q / H, h = q - c * H;
    double acc = 0.0, acc2 = 0.0;
#pragma unroll 4
    for (unsigned i = beg; i < end; i += 256) {
        float v = p0[c * d.s0[1] + h * d.s0[2] + w * d.s0[3]];
        if (KIND == VB_PRIOR) {
            if constexpr (SHIFT) v = v - pr[c * d.sr[1] + h * d.sr[2] + w * d.sr[3]];
            acc += (double)(v * v);
        } else {
            float xh = x0_pred(k, pt[c * d.st[1] + h * d.st[2] + w * d.st[3]], pe[c * d.se[1] + h * d.se[2] + w * d.se[3]]);
            if (d.clip) xh = xh < -1.0f ? -1.0f : (xh > 1.0f ? 1.0f : xh);          // comparisons: a NaN stays a NaN
            if (KIND == VB_KL) {
                if constexpr (SHIFT) v = v + g * pr[c * d.sr[1] + h * d.sr[2] + w * d.sr[3]];
                const float df = v - xh;
                acc += (double)(df * df);
            } else {
                const float df = v - xh;
                acc += vb_dec_nll(v, xh, d.inv_sigma);
                if (MSE) acc2 += (double)(df * df);
            }
        }
        w += dw;
        if (w >= W) { w -= W; ++h; }
        h += dh; c += dc;
        if (h >= H) { h -= H; ++c; }
    }
    sum = block_sum256(acc, red);
    if (KIND == VB_DEC && MSE) {
        __syncthreads();
        sq = block_sum256(acc2, red);
    } else {
        sq = sum;
    }
}

// grid (nchunk, images of this launch), as image_loss_kernel.  part: [2][N][nchunk] (term sums, squared-difference sums) when nchunk > 1.
template <bool MSE, bool SHIFT>
__global__ __launch_bounds__(256) void vb_terms_kernel(VbArgsT<SHIFT> d, int n0, int N, unsigned total, int nchunk, unsigned dc, unsigned dh,
                                                       unsigned dw, double* __restrict__ part, float* __restrict__ bits,
                                                       float* __restrict__ mse) {
    __shared__ double red[256];
    const long long n = (long long)n0 + blockIdx.y;
    const long long tl = d.f.t[n];
    const int t = (int)tl;
    double sum, sq;
    if (tl < 0 || tl > d.f.T) sum = sq = __builtin_nan("");     // the launcher checked the host copy; a device array that differs reads no table
    else if (t == d.f.T) vb_walk<VB_PRIOR, MSE, SHIFT>(d, n, t, total, dc, dh, dw, red, sum, sq);
    else if (t == 0) vb_walk<VB_DEC, MSE, SHIFT>(d, n, t, total, dc, dh, dw, red, sum, sq);
    else vb_walk<VB_KL, MSE, SHIFT>(d, n, t, total, dc, dh, dw, red, sum, sq);
    if (threadIdx.x == 0) {
        if (nchunk == 1) {
            bits[n] = vb_finish(d.f, n, sum / (double)total);
            if (MSE) mse[n] = (float)(sq / (double)total);
        } else {
            part[n * nchunk + blockIdx.x] = sum;
            if (MSE) part[((long long)N + n) * nchunk + blockIdx.x] = sq;
        }
    }
}

// the checks both launchers share; `who` names the entry point
static int img_pair_check(const bd_image_pair_desc* d, const float* out, const char* who) {
    BD_CHECK(d && d->preds && d->target && out, BD_ERR_INVALID, "%s: null pointer", who);
    BD_CHECK(d->N > 0 && d->C > 0 && d->H > 0 && d->W > 0, BD_ERR_INVALID, "%s: N=%d C=%d H=%d W=%d must be positive", who, d->N, d->C, d->H,
             d->W);
    BD_CHECK((long long)d->C * d->H * d->W < (1ll << 31), BD_ERR_UNSUPPORTED, "%s: C*H*W=%lld does not fit 31 bits", who,
             (long long)d->C * d->H * d->W);
    for (int i = 0; i < 4; ++i)
        BD_CHECK(d->p_stride[i] >= 0 && d->t_stride[i] >= 0, BD_ERR_INVALID, "%s: negative stride (preds %lld, target %lld at dim %d)", who,
                 (long long)d->p_stride[i], (long long)d->t_stride[i], i);
    return BD_OK;
}
static ImgPair img_pair(const bd_image_pair_desc& d) {
    ImgPair q;
    q.C = d.C; q.H = d.H; q.W = d.W; q.p = d.preds; q.t = d.target;
    for (int i = 0; i < 4; ++i) { q.ps[i] = d.p_stride[i]; q.ts[i] = d.t_stride[i]; }
    return q;
}
static void ssim_window(float data_range, SsimWin& win, float& c1, float& c2) {
    double s = 0.0, g[SS_K];
    for (int i = 0; i < SS_K; ++i) { const double x = i - (SS_K - 1) / 2.0; g[i] = exp(-(x / 1.5) * (x / 1.5) / 2.0); s += g[i]; }
    for (int i = 0; i < SS_K; ++i) win.g[i] = (float)(g[i] / s);
    c1 = (0.01f * data_range) * (0.01f * data_range); c2 = (0.03f * data_range) * (0.03f * data_range);
}
constexpr int IMG_MAX_GRID = 65535;   // grid.y / grid.z of one launch: the launchers cut the images / planes into runs of at most this many

// ---- backdoor detection statistics (defense.py; DESIGN.md section 3, "Detection statistics") ---------------------------------------------------------
// Pairwise squared distances of N rows: one workgroup = one 64 x 64 tile of pairs (ti <= tj: the upper triangle of tiles), the 64 + 64
// rows staged through LDS in chunks of 32 values (row pitch 36 floats: the 128-bit reads of 8 consecutive rows cover all 32 banks), each
// thread a 4 x 4 micro-tile of pairs with rows ty + 16 r and tx + 16 c.  Two values of k go through one v_pk_add_f32 (the difference)
// and one v_pk_fma_f32 (the square and the add round once), so a pair keeps one sum over the even and one over the odd k, added at the
// end: 122 VGPRs, 4 workgroups per CU.  The next chunk is fetched into registers while the current one is consumed.
// grid.z > 1: the workgroup covers chunks [z * cps, (z + 1) * cps) and stores its tile into the workspace; pairwise_fold_kernel adds
// the splits in order.  Both go through pd_store_tile, which writes d2[i][j] directly and d2[j][i] through an LDS transpose.
typedef float pd_f2 __attribute__((ext_vector_type(2)));
constexpr int PD_T = 64, PD_KC = 32, PD_LD = PD_KC + 4, PD_MINCPS = 8;   // tile edge, chunk, LDS row pitch, fewest chunks per split

__device__ __forceinline__ long long pd_tile_index(int ti, int tj, int nt) {   // row-major over the upper triangle, ti <= tj
    return (long long)ti * nt - (long long)ti * (ti - 1) / 2 + (tj - ti);
}

// 4 values x[row][k .. k + 3] (zeros beyond row N or column kend)
template <bool VEC>
__device__ __forceinline__ float4 pd_fetch(const float* __restrict__ x, long long ldx, int N, int row, long long k, long long kend) {
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < N) {
        const float* p = x + (long long)row * ldx + k;
        if (VEC && k + 4 <= kend) {
            r = *reinterpret_cast<const float4*>(p);
        } else {
            if (k < kend) r.x = p[0];
            if (k + 1 < kend) r.y = p[1];
            if (k + 2 < kend) r.z = p[2];
            if (k + 3 < kend) r.w = p[3];
        }
    }
    return r;
}

// acc[r][c] = value of the pair (rows ty + 16 (r0 + r) of tile ti, tx + 16 c of tile tj).  T: 64 * (16 R + 1) floats of LDS nobody reads
// any more.  A diagonal tile holds every pair twice: the copy with i < j is stored at both places, i == j is written as 0.
template <int R>
__device__ __forceinline__ void pd_store_tile(const float (&acc)[R][4], int r0, int ti, int tj, int N, float* __restrict__ d2, long long ldd,
                                              float* T, int tid) {
    constexpr int TP = 16 * R + 1;
    const int tx = tid & 15, ty = tid >> 4;
    const bool diag = ti == tj;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int jl = tx + 16 * c, gi = ti * PD_T + ty + 16 * (r0 + r), gj = tj * PD_T + jl;
            T[jl * TP + ty + 16 * r] = acc[r][c];
            if (gi < N && gj < N) {
                if (!diag || gi < gj) d2[(long long)gi * ldd + gj] = acc[r][c];
                else if (gi == gj) d2[(long long)gi * ldd + gj] = 0.f;
            }
        }
    __syncthreads();
    for (int idx = tid; idx < PD_T * 16 * R; idx += 256) {
        const int jl = idx / (16 * R), is = idx - jl * (16 * R);
        const int gi = ti * PD_T + 16 * r0 + is, gj = tj * PD_T + jl;
        if (gi < N && gj < N && (!diag || gi < gj)) d2[(long long)gj * ldd + gi] = T[jl * TP + is];
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void pairwise_sqdist_kernel(const float* __restrict__ x, long long ldx, int N, int D, int cps,
                                                              float* __restrict__ d2, long long ldd, float* __restrict__ part) {
    const int tj = blockIdx.x, ti = blockIdx.y;
    if (tj < ti) return;
    __shared__ __attribute__((aligned(16))) float sm[2 * PD_T * PD_LD];   // A rows | B rows; afterwards the transposed tile (64 x 65)
    static_assert(2 * PD_T * PD_LD >= PD_T * (PD_T + 1), "the epilogue's transpose reuses the staging buffer");
    float* As = sm;
    float* Bs = sm + PD_T * PD_LD;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int lr = tid >> 3, lq = (tid & 7) * 4;                          // loader: rows lr and lr + 32, values lq .. lq + 3 of the chunk
    const long long kbeg = (long long)blockIdx.z * cps * PD_KC;
    const long long kend = kbeg + (long long)cps * PD_KC < D ? kbeg + (long long)cps * PD_KC : D;
    pd_f2 acc2[4][4] = {};                                                // per pair: the sums over even and over odd k
    float4 pa[2], pb[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        pa[s] = pd_fetch<VEC>(x, ldx, N, ti * PD_T + lr + 32 * s, kbeg + lq, kend);
        pb[s] = pd_fetch<VEC>(x, ldx, N, tj * PD_T + lr + 32 * s, kbeg + lq, kend);
    }
    for (long long k0 = kbeg; k0 < kend; k0 += PD_KC) {
        __syncthreads();                                                  // the previous chunk has been consumed
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            *reinterpret_cast<float4*>(&As[(lr + 32 * s) * PD_LD + lq]) = pa[s];
            *reinterpret_cast<float4*>(&Bs[(lr + 32 * s) * PD_LD + lq]) = pb[s];
        }
        __syncthreads();
        if (k0 + PD_KC < kend) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                pa[s] = pd_fetch<VEC>(x, ldx, N, ti * PD_T + lr + 32 * s, k0 + PD_KC + lq, kend);
                pb[s] = pd_fetch<VEC>(x, ldx, N, tj * PD_T + lr + 32 * s, k0 + PD_KC + lq, kend);
            }
        }
#pragma unroll 2
        for (int k4 = 0; k4 < PD_KC; k4 += 4) {
            float4 a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = *reinterpret_cast<const float4*>(&As[(ty + 16 * r) * PD_LD + k4]);
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = *reinterpret_cast<const float4*>(&Bs[(tx + 16 * c) * PD_LD + k4]);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {                             // two values of k per v_pk_add_f32 / v_pk_fma_f32
                    pd_f2 d = pd_f2{a[r].x, a[r].y} - pd_f2{b[c].x, b[c].y};
                    acc2[r][c] = __builtin_elementwise_fma(d, d, acc2[r][c]);
                    d = pd_f2{a[r].z, a[r].w} - pd_f2{b[c].z, b[c].w};
                    acc2[r][c] = __builtin_elementwise_fma(d, d, acc2[r][c]);
                }
        }
    }
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = acc2[r][c].x + acc2[r][c].y;
    if (part) {                                                           // split D: this split's tile, [split][tile][64 x 64]
        const long long ntiles = (long long)gridDim.x * (gridDim.x + 1) / 2;
        float* o = part + ((long long)blockIdx.z * ntiles + pd_tile_index(ti, tj, gridDim.x)) * (PD_T * PD_T);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) o[(ty + 16 * r) * PD_T + tx + 16 * c] = acc[r][c];
        return;
    }
    __syncthreads();                                                      // everyone is done reading As / Bs
    pd_store_tile<4>(acc, 0, ti, tj, N, d2, ldd, sm, tid);
}

// grid (nt, nt, 4): 16 rows of one tile per workgroup, the splits added in split order
__global__ __launch_bounds__(256) void pairwise_fold_kernel(const float* __restrict__ part, int ksplit, int N, float* __restrict__ d2,
                                                            long long ldd) {
    const int tj = blockIdx.x, ti = blockIdx.y, r0 = blockIdx.z;
    if (tj < ti) return;
    __shared__ float T[PD_T * 17];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long long ntiles = (long long)gridDim.x * (gridDim.x + 1) / 2;
    const float* p = part + pd_tile_index(ti, tj, gridDim.x) * (PD_T * PD_T) + (ty + 16 * r0) * PD_T + tx;
    float acc[1][4] = {};
    for (int s = 0; s < ksplit; ++s, p += ntiles * (PD_T * PD_T))
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[0][c] += p[16 * c];
    pd_store_tile<1>(acc, r0, ti, tj, N, d2, ldd, T, tid);
}

// Total variation: one workgroup per image; thread-strided over the logical index (c, h, w), |differences| in fp32 summed in fp64 per
// thread, then the tree of ssim_final_kernel.  The order depends on the logical index only, never on the strides.
__global__ __launch_bounds__(256) void total_variation_kernel(const float* __restrict__ x, int C, int H, int W, long long sn, long long sc,
                                                              long long sh, long long sw, float* __restrict__ tv) {
    __shared__ double red[256];
    const float* img = x + (long long)blockIdx.x * sn;
    const unsigned total = (unsigned)C * H * W;
    double acc = 0.0;
    for (unsigned i = threadIdx.x; i < total; i += 256) {
        const unsigned q = i / W, w = i - q * W, c = q / H, h = q - c * H;
        const float* p = img + c * sc + h * sh + w * sw;
        const float v = p[0];
        if (h + 1 < (unsigned)H) acc += (double)fabsf(p[sh] - v);
        if (w + 1 < (unsigned)W) acc += (double)fabsf(p[sw] - v);
    }
    const double r = block_sum256(acc, red);
    if (threadIdx.x == 0) tv[blockIdx.x] = (float)r;
}

// Split of D for N rows: tiles, the largest split count any D' <= D can get (the workspace bound, monotone in D), the split used
struct PdPlan { int nt; long long ntiles; int cap, ksplit, cps; };
static PdPlan pd_plan(int N, int D) {
    PdPlan p;
    p.nt = (int)cdiv(N, PD_T);
    p.ntiles = (long long)p.nt * (p.nt + 1) / 2;
    // 8 workgroups per CU, twice what is resident: the 528 tiles of 2048 rows alone would leave 240 CUs with two and 16 with three
    const int nchunks = (int)cdiv(D, PD_KC), slots = 8 * device_cus();
    long long cap = slots / p.ntiles;
    if (cap > nchunks / PD_MINCPS) cap = nchunks / PD_MINCPS;
    p.cap = cap < 1 ? 1 : (int)cap;
    split_k(slots, p.ntiles, nchunks, PD_MINCPS, p.ksplit, p.cps);
    return p;
}

}  // namespace bd

using namespace bd;

extern "C" size_t bd_pairwise_sqdist_workspace_bytes(int N, int D) {
    if (N <= 0 || D <= 0) return 0;
    const PdPlan p = pd_plan(N, D);
    return p.cap > 1 ? (size_t)p.cap * p.ntiles * PD_T * PD_T * sizeof(float) : 0;
}

extern "C" int bd_pairwise_sqdist(const float* x, int64_t ldx, int N, int D, float* d2, int64_t ldd, void* workspace, size_t workspace_bytes,
                                  bd_stream_t stream) {
    BD_CHECK(x && d2, BD_ERR_INVALID, "bd_pairwise_sqdist: null pointer");
    BD_CHECK(N >= 1 && D >= 1, BD_ERR_INVALID, "bd_pairwise_sqdist: N=%d D=%d must be positive", N, D);
    BD_CHECK(ldx >= D, BD_ERR_INVALID, "bd_pairwise_sqdist: ldx=%lld < D=%d", (long long)ldx, D);
    BD_CHECK(ldd >= N, BD_ERR_INVALID, "bd_pairwise_sqdist: ldd=%lld < N=%d", (long long)ldd, N);
    BD_CHECK((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(d2) & 3) == 0, BD_ERR_INVALID,
             "bd_pairwise_sqdist: x and d2 must be 4-byte aligned");
    const PdPlan p = pd_plan(N, D);
    BD_CHECK(p.nt <= 65535, BD_ERR_UNSUPPORTED, "bd_pairwise_sqdist: N=%d too large for one launch", N);
    const size_t need = bd_pairwise_sqdist_workspace_bytes(N, D);
    BD_CHECK(workspace_bytes >= need && (workspace || !need), BD_ERR_WORKSPACE, "bd_pairwise_sqdist: workspace %zu < %zu",
             workspace ? workspace_bytes : (size_t)0, need);
    float* part = p.ksplit > 1 ? reinterpret_cast<float*>(workspace) : nullptr;
    const dim3 grid((unsigned)p.nt, (unsigned)p.nt, (unsigned)p.ksplit);
    if (aligned16(x) && ldx % 4 == 0)
        hipLaunchKernelGGL(pairwise_sqdist_kernel<true>, grid, dim3(256), 0, S(stream), x, (long long)ldx, N, D, p.cps, d2, (long long)ldd, part);
    else
        hipLaunchKernelGGL(pairwise_sqdist_kernel<false>, grid, dim3(256), 0, S(stream), x, (long long)ldx, N, D, p.cps, d2, (long long)ldd, part);
    BD_LAUNCH_CHECK("pairwise_sqdist");
    if (part) {
        hipLaunchKernelGGL(pairwise_fold_kernel, dim3((unsigned)p.nt, (unsigned)p.nt, 4), dim3(256), 0, S(stream), part, p.ksplit, N, d2,
                           (long long)ldd);
        BD_LAUNCH_CHECK("pairwise_fold");
    }
    return BD_OK;
}

extern "C" int bd_total_variation(const float* x, int N, int C, int H, int W, int64_t stride_n, int64_t stride_c, int64_t stride_h,
                                  int64_t stride_w, float* tv, bd_stream_t stream) {
    BD_CHECK(x && tv, BD_ERR_INVALID, "bd_total_variation: null pointer");
    BD_CHECK(N > 0 && C > 0 && H > 0 && W > 0, BD_ERR_INVALID, "bd_total_variation: N=%d C=%d H=%d W=%d must be positive", N, C, H, W);
    BD_CHECK((long long)C * H * W < (1ll << 31), BD_ERR_UNSUPPORTED, "bd_total_variation: C*H*W=%lld does not fit 31 bits", (long long)C * H * W);
    hipLaunchKernelGGL(total_variation_kernel, dim3((unsigned)N), dim3(256), 0, S(stream), x, C, H, W, (long long)stride_n, (long long)stride_c,
                       (long long)stride_h, (long long)stride_w, tv);
    BD_LAUNCH_CHECK("total_variation");
    return BD_OK;
}

extern "C" size_t bd_ssim_workspace_bytes(int N, int C, int H, int W) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)N * C * cdiv(H, SS_T) * cdiv(W, SS_T) * sizeof(double);
}

extern "C" int bd_ssim(const float* preds, const float* target, int N, int C, int H, int W, int64_t stride_n, int64_t stride_c,
                       int64_t stride_h, int64_t stride_w, float data_range, float* out, void* workspace, size_t workspace_bytes,
                       bd_stream_t stream) {
    BD_CHECK(preds && target && out && workspace, BD_ERR_INVALID, "bd_ssim: null pointer");
    BD_CHECK(N > 0 && C > 0 && H > 2 * SS_PAD && W > 2 * SS_PAD, BD_ERR_INVALID, "bd_ssim: images must be larger than the 11x11 window's border (H=%d W=%d)", H, W);
    BD_CHECK((long long)N * C <= 65535, BD_ERR_UNSUPPORTED, "bd_ssim: N*C=%lld too large for one launch", (long long)N * C);
    const size_t need = bd_ssim_workspace_bytes(N, C, H, W);
    BD_CHECK(workspace_bytes >= need, BD_ERR_WORKSPACE, "bd_ssim: workspace %zu < %zu", workspace_bytes, need);
    SsimWin win;
    float c1, c2;
    ssim_window(data_range, win, c1, c2);
    const dim3 grid((unsigned)cdiv(W, SS_T), (unsigned)cdiv(H, SS_T), (unsigned)(N * C));
    double* part = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(ssim_tile_kernel, grid, dim3(256), 0, S(stream), preds, target, C, H, W, (long long)stride_n, (long long)stride_c,
                       (long long)stride_h, (long long)stride_w, c1, c2, win, part);
    BD_LAUNCH_CHECK("ssim_tile");
    const long long np = (long long)grid.x * grid.y * grid.z;
    const double inv = 1.0 / ((double)N * C * (H - 2 * SS_PAD) * (double)(W - 2 * SS_PAD));
    hipLaunchKernelGGL(ssim_final_kernel, dim3(1), dim3(256), 0, S(stream), part, np, inv, out);
    BD_LAUNCH_CHECK("ssim_final");
    return BD_OK;
}

extern "C" size_t bd_image_loss_workspace_bytes(int N, int C, int H, int W) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    const long long nchunk = cdiv((long long)C * H * W, IL_CHUNK);
    return nchunk > 1 ? (size_t)N * (size_t)nchunk * sizeof(double) : 0;   // one chunk: the workgroup writes out[n] itself
}

extern "C" int bd_image_loss(const bd_image_pair_desc* d, int loss_type, float* out, void* workspace, size_t workspace_bytes,
                             bd_stream_t stream) {
    BD_TRY(img_pair_check(d, out, "bd_image_loss"));
    BD_CHECK(loss_type >= 0 && loss_type <= 2, BD_ERR_INVALID, "bd_image_loss: loss_type %d (l2=0,l1=1,huber=2)", loss_type);
    const size_t need = bd_image_loss_workspace_bytes(d->N, d->C, d->H, d->W);
    BD_CHECK(workspace_bytes >= need && (workspace || !need), BD_ERR_WORKSPACE, "bd_image_loss: workspace %zu < %zu",
             workspace ? workspace_bytes : (size_t)0, need);
    const unsigned total = (unsigned)((long long)d->C * d->H * d->W);
    const int nchunk = (int)cdiv(total, IL_CHUNK);
    const unsigned dq = 256u / (unsigned)d->W, dw = 256u % (unsigned)d->W, dc = dq / (unsigned)d->H, dh = dq % (unsigned)d->H;
    const ImgPair q = img_pair(*d);
    double* part = reinterpret_cast<double*>(workspace);
    for (int n0 = 0; n0 < d->N; n0 += IMG_MAX_GRID) {
        const int n = d->N - n0 < IMG_MAX_GRID ? d->N - n0 : IMG_MAX_GRID;
        hipLaunchKernelGGL(image_loss_kernel, dim3((unsigned)nchunk, (unsigned)n), dim3(256), 0, S(stream), q, n0, loss_type, total, nchunk, dc,
                           dh, dw, part, out);
        BD_LAUNCH_CHECK("image_loss");
    }
    if (nchunk > 1) {
        hipLaunchKernelGGL(image_fold_kernel<false>, dim3((unsigned)d->N), dim3(256), 0, S(stream), part, nchunk, (double)total, out, VbFinish{});
        BD_LAUNCH_CHECK("image_loss_fold");
    }
    return BD_OK;
}

extern "C" size_t bd_ssim_images_workspace_bytes(int N, int C, int H, int W) { return bd_ssim_workspace_bytes(N, C, H, W); }

extern "C" int bd_ssim_images(const bd_image_pair_desc* d, float data_range, float* out, void* workspace, size_t workspace_bytes,
                              bd_stream_t stream) {
    BD_TRY(img_pair_check(d, out, "bd_ssim_images"));
    BD_CHECK(d->H > 2 * SS_PAD && d->W > 2 * SS_PAD, BD_ERR_INVALID,
             "bd_ssim_images: images must be larger than the 11x11 window's border (H=%d W=%d)", d->H, d->W);
    const size_t need = bd_ssim_images_workspace_bytes(d->N, d->C, d->H, d->W);
    BD_CHECK(workspace && workspace_bytes >= need, BD_ERR_WORKSPACE, "bd_ssim_images: workspace %zu < %zu",
             workspace ? workspace_bytes : (size_t)0, need);
    SsimWin win;
    float c1, c2;
    ssim_window(data_range, win, c1, c2);
    const ImgPair q = img_pair(*d);
    const unsigned gx = (unsigned)cdiv(d->W, SS_T), gy = (unsigned)cdiv(d->H, SS_T);
    const long long planes = (long long)d->N * d->C;
    double* part = reinterpret_cast<double*>(workspace);
    for (long long z0 = 0; z0 < planes; z0 += IMG_MAX_GRID) {
        const unsigned nz = (unsigned)(planes - z0 < IMG_MAX_GRID ? planes - z0 : IMG_MAX_GRID);
        hipLaunchKernelGGL(ssim_images_tile_kernel, dim3(gx, gy, nz), dim3(256), 0, S(stream), q, z0, c1, c2, win, part);
        BD_LAUNCH_CHECK("ssim_images_tile");
    }
    const double count = (double)d->C * (d->H - 2 * SS_PAD) * (double)(d->W - 2 * SS_PAD);
    hipLaunchKernelGGL(image_fold_kernel<false>, dim3((unsigned)d->N), dim3(256), 0, S(stream), part, (int)(d->C * gy * gx), count, out,
                       VbFinish{});
    BD_LAUNCH_CHECK("ssim_images_fold");
    return BD_OK;
}

extern "C" size_t bd_vb_terms_workspace_bytes(int N, int C, int H, int W) {
    return 2 * bd_image_loss_workspace_bytes(N, C, H, W);                   // the term sums and the squared-difference sums
}

// the checks and launches of bd_vb_terms and bd_vb_terms_shift (D: either descriptor; the shared fields carry the same names)
template <bool SHIFT, class D>
static int vb_terms_run(const D* d, void* workspace, size_t workspace_bytes, bd_stream_t stream, const char* who) {
    BD_CHECK(d, BD_ERR_INVALID, "%s: null descriptor", who);
    BD_CHECK(d->x0 && d->t && d->t_host && d->alphas_cumprod && d->term_add && d->term_mul && d->bits, BD_ERR_INVALID, "%s: null pointer", who);
    BD_CHECK(d->N > 0 && d->C > 0 && d->H > 0 && d->W > 0, BD_ERR_INVALID, "%s: N=%d C=%d H=%d W=%d must be positive", who, d->N, d->C, d->H,
             d->W);
    BD_CHECK(d->T >= 1, BD_ERR_INVALID, "%s: T=%d must be positive", who, d->T);
    BD_CHECK(d->inv_sigma_dec > 0.f && d->inv_sigma_dec <= 3.4e38f, BD_ERR_INVALID, "%s: inv_sigma_dec=%g must be positive and finite", who,
             (double)d->inv_sigma_dec);
    BD_CHECK((long long)d->C * d->H * d->W < (1ll << 31), BD_ERR_UNSUPPORTED, "%s: C*H*W=%lld does not fit 31 bits", who,
             (long long)d->C * d->H * d->W);
    bool reads_chain = false;
    for (int n = 0; n < d->N; ++n) {
        const long long t = d->t_host[n];
        BD_CHECK(t >= 0 && t <= d->T, BD_ERR_INVALID, "%s: t[%d]=%lld outside [0, %d]", who, n, t, d->T);
        reads_chain |= t < d->T;
    }
    BD_CHECK(!reads_chain || (d->x_t && d->eps), BD_ERR_INVALID, "%s: null x_t or eps with a row at t < T", who);
    for (int i = 0; i < 4; ++i)
        BD_CHECK(d->x0_stride[i] >= 0 && d->xt_stride[i] >= 0 && d->eps_stride[i] >= 0, BD_ERR_INVALID,
                 "%s: negative stride (x0 %lld, x_t %lld, eps %lld at dim %d)", who, (long long)d->x0_stride[i], (long long)d->xt_stride[i],
                 (long long)d->eps_stride[i], i);
    VbArgsT<SHIFT> a;
    if constexpr (SHIFT) {
        BD_CHECK(d->r && d->term_shift, BD_ERR_INVALID, "%s: null r or term_shift", who);
        for (int i = 0; i < 4; ++i) {
            BD_CHECK(d->r_stride[i] >= 0, BD_ERR_INVALID, "%s: negative stride (r %lld at dim %d)", who, (long long)d->r_stride[i], i);
            a.sr[i] = d->r_stride[i];
        }
        a.r = d->r; a.g = d->term_shift;
    }
    const size_t need = bd_vb_terms_workspace_bytes(d->N, d->C, d->H, d->W);
    BD_CHECK(workspace_bytes >= need && (workspace || !need), BD_ERR_WORKSPACE, "%s: workspace %zu < %zu", who,
             workspace ? workspace_bytes : (size_t)0, need);
    const unsigned total = (unsigned)((long long)d->C * d->H * d->W);
    const int nchunk = (int)cdiv(total, IL_CHUNK);
    const unsigned dq = 256u / (unsigned)d->W, dw = 256u % (unsigned)d->W, dc = dq / (unsigned)d->H, dh = dq % (unsigned)d->H;
    a.C = d->C; a.H = d->H; a.W = d->W; a.clip = d->clip_denoised != 0;
    a.x0 = d->x0; a.xt = d->x_t; a.ep = d->eps; a.ac = d->alphas_cumprod;
    for (int i = 0; i < 4; ++i) { a.s0[i] = d->x0_stride[i]; a.st[i] = d->xt_stride[i]; a.se[i] = d->eps_stride[i]; }
    a.inv_sigma = (double)d->inv_sigma_dec;
    a.f.t = reinterpret_cast<const long long*>(d->t); a.f.add = d->term_add; a.f.mul = d->term_mul; a.f.T = d->T;
    double* part = reinterpret_cast<double*>(workspace);
    for (int n0 = 0; n0 < d->N; n0 += IMG_MAX_GRID) {
        const int n = d->N - n0 < IMG_MAX_GRID ? d->N - n0 : IMG_MAX_GRID;
        const dim3 grid((unsigned)nchunk, (unsigned)n);
        if (d->x0_mse)
            hipLaunchKernelGGL((vb_terms_kernel<true, SHIFT>), grid, dim3(256), 0, S(stream), a, n0, d->N, total, nchunk, dc, dh, dw, part,
                               d->bits, d->x0_mse);
        else
            hipLaunchKernelGGL((vb_terms_kernel<false, SHIFT>), grid, dim3(256), 0, S(stream), a, n0, d->N, total, nchunk, dc, dh, dw, part,
                               d->bits, d->x0_mse);
        BD_LAUNCH_CHECK(SHIFT ? "vb_terms_shift" : "vb_terms");
    }
    if (nchunk > 1) {
        hipLaunchKernelGGL(image_fold_kernel<true>, dim3((unsigned)d->N), dim3(256), 0, S(stream), part, nchunk, (double)total, d->bits, a.f);
        BD_LAUNCH_CHECK(SHIFT ? "vb_terms_shift_fold" : "vb_terms_fold");
        if (d->x0_mse) {
            hipLaunchKernelGGL(image_fold_kernel<false>, dim3((unsigned)d->N), dim3(256), 0, S(stream), part + (size_t)d->N * nchunk, nchunk,
                               (double)total, d->x0_mse, VbFinish{});
            BD_LAUNCH_CHECK(SHIFT ? "vb_terms_shift_fold_mse" : "vb_terms_fold_mse");
        }
    }
    return BD_OK;
}

extern "C" int bd_vb_terms(const bd_vb_terms_desc* d, void* workspace, size_t workspace_bytes, bd_stream_t stream) {
    return vb_terms_run<false>(d, workspace, workspace_bytes, stream, "bd_vb_terms");
}

extern "C" int bd_vb_terms_shift(const bd_vb_terms_shift_desc* d, void* workspace, size_t workspace_bytes, bd_stream_t stream) {
    return vb_terms_run<true>(d, workspace, workspace_bytes, stream, "bd_vb_terms_shift");
}
