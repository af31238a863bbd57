// Sample-quality metrics on feature rows (improved precision / recall, density / coverage, KID): pairwise work between two sets of
// rows a [Na, D] and b [Nb, D] that never stores the Na x Nb matrix.  DESIGN.md section 3, "Quality metrics on features".
//
// One strip kernel, three epilogues.  A workgroup owns 64 rows of a (a strip) and walks a contiguous range of 64-column tiles of b.
// A tile is computed the way pairwise_sqdist_kernel (metrics.hip) computes its tile: rows staged through LDS in chunks of 32 values at
// row pitch 36, a 4 x 4 micro-tile of pairs per thread, two values of k per v_pk_add_f32 / v_pk_fma_f32, the even and the odd sums
// added at the end, the next chunk fetched into registers while the current one is consumed; D is never split.  The value of a pair
// comes from qs_tile alone, so a pair has the same bits in every epilogue, in either role ((a - b)^2 == (b - a)^2 and a * b == b * a
// term by term, the k order is fixed) and in whatever strip, tile or split it falls.
// The finished tile goes to LDS (64 x 64 at pitch 65, in the staging buffer) and thread (row = tid & 63, q = tid >> 6) reads columns
// 16 q .. 16 q + 15 of its row:
//   QS_KNN    a sorted list of the k smallest values per (row, q) in LDS, the current k-th kept in a register: a candidate that is not
//             smaller is rejected with one compare; the four lists of a row are merged at the end of the strip
//   QS_COUNT  count of d2 <= radius2[column] (int) and the running minimum (float)
//   QS_POLY   sum of (double(dot) / D + 1)^3 in fp64, columns in order
// Few strips: the column tiles are cut into csplit contiguous ranges (grid.x), each writes its per-row partial to the workspace
// [csplit][Na][...] and a second launch folds the splits in split order.  No atomics.
#include "common.h"

namespace bd {

typedef float qs_f2 __attribute__((ext_vector_type(2)));
constexpr int QS_T = 64, QS_KC = 32, QS_LD = QS_KC + 4, QS_TP = QS_T + 1, QS_KMAX = 16;   // tile edge, chunk, LDS row pitch, tile pitch, largest k
enum { QS_KNN = 0, QS_COUNT = 1, QS_POLY = 2 };

struct QsArgs {
    const float* a; long long lda; int Na;
    const float* b; long long ldb; int Nb;
    int D, tps;                       // tiles per split
    int k; long long self_col0;       // QS_KNN: column i + self_col0 is left out of row i (< 0 with |self_col0| > Na: none)
    float* klist; int kth_only;       //   [split][Na][k] ascending, or (one split, kth_only) out[Na] = the k-th
    const float* radius2; int* count; float* min_d2;   // QS_COUNT: [split][Na] each; radius2 == nullptr: no count
    int exclude_diag; double* rowsum; // QS_POLY: [split][Na]
};

// 4 values x[row][k .. k + 3] (zeros beyond row N or column D)
template <bool VEC>
__device__ __forceinline__ float4 qs_fetch(const float* __restrict__ x, long long ldx, int N, int row, int k, int D) {
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < N) {
        const float* p = x + (long long)row * ldx + k;
        if (VEC && k + 4 <= D) {
            r = *reinterpret_cast<const float4*>(p);
        } else {
            if (k < D) r.x = p[0];
            if (k + 1 < D) r.y = p[1];
            if (k + 2 < D) r.z = p[2];
            if (k + 3 < D) r.w = p[3];
        }
    }
    return r;
}

// two values of k of one pair: the squared difference (the difference rounds once, the square and the add round once) or the product
template <bool DOT>
__device__ __forceinline__ qs_f2 qs_pair_step(qs_f2 a, qs_f2 b, qs_f2 acc) {
    if (DOT) return __builtin_elementwise_fma(a, b, acc);
    const qs_f2 d = a - b;
    return __builtin_elementwise_fma(d, d, acc);
}

// THE pair value: acc[r][c] = sum_k (a[row0 + ty + 16 r][k] - b[col0 + tx + 16 c][k])^2, or the dot product of the two rows.
// sm: 2 * QS_T * QS_LD floats; every thread of the workgroup calls it; it begins with a barrier and ends without one.
template <bool VEC, bool DOT>
__device__ __forceinline__ void qs_tile(const QsArgs& p, int row0, int col0, float* sm, float (&acc)[4][4]) {
    float* As = sm;
    float* Bs = sm + QS_T * QS_LD;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int lr = tid >> 3, lq = (tid & 7) * 4;                          // loader: rows lr and lr + 32, values lq .. lq + 3 of the chunk
    qs_f2 acc2[4][4] = {};                                                // per pair: the sums over even and over odd k
    float4 pa[2], pb[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        pa[s] = qs_fetch<VEC>(p.a, p.lda, p.Na, row0 + lr + 32 * s, lq, p.D);
        pb[s] = qs_fetch<VEC>(p.b, p.ldb, p.Nb, col0 + lr + 32 * s, lq, p.D);
    }
    for (int k0 = 0; k0 < p.D; k0 += QS_KC) {
        __syncthreads();                                                  // the previous chunk (or the previous tile's epilogue) is done
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            *reinterpret_cast<float4*>(&As[(lr + 32 * s) * QS_LD + lq]) = pa[s];
            *reinterpret_cast<float4*>(&Bs[(lr + 32 * s) * QS_LD + lq]) = pb[s];
        }
        __syncthreads();
        if (k0 + QS_KC < p.D) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                pa[s] = qs_fetch<VEC>(p.a, p.lda, p.Na, row0 + lr + 32 * s, k0 + QS_KC + lq, p.D);
                pb[s] = qs_fetch<VEC>(p.b, p.ldb, p.Nb, col0 + lr + 32 * s, k0 + QS_KC + lq, p.D);
            }
        }
#pragma unroll 2
        for (int k4 = 0; k4 < QS_KC; k4 += 4) {
            float4 a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = *reinterpret_cast<const float4*>(&As[(ty + 16 * r) * QS_LD + k4]);
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = *reinterpret_cast<const float4*>(&Bs[(tx + 16 * c) * QS_LD + k4]);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    acc2[r][c] = qs_pair_step<DOT>(qs_f2{a[r].x, a[r].y}, qs_f2{b[c].x, b[c].y}, acc2[r][c]);
                    acc2[r][c] = qs_pair_step<DOT>(qs_f2{a[r].z, a[r].w}, qs_f2{b[c].z, b[c].w}, acc2[r][c]);
                }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = acc2[r][c].x + acc2[r][c].y;
}

// Sorted list of the k smallest values seen, ascending, element j at l[64 j] (one list per lane, lanes side by side: no bank
// conflicts); thr is l[64 (k - 1)].  The multiset of the k smallest does not depend on the order of the offers.
__device__ __forceinline__ void qs_offer(float* l, int k, float v, float& thr) {
    if (!(v < thr)) return;
    int j = k - 1;
    while (j > 0 && l[(j - 1) * 64] > v) {
        l[j * 64] = l[(j - 1) * 64];
        --j;
    }
    l[j * 64] = v;
    thr = l[(k - 1) * 64];
}

// 4 workgroups per CU as for pairwise_sqdist_kernel: the register cap of 128 makes the compiler park the 4 - 7 values that only the
// epilogue needs (row index, threshold, count, minimum) in scratch across the k loop, where nothing reads them.
template <bool VEC, int EPI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void qs_strip_kernel(const QsArgs p) {
    __shared__ __attribute__((aligned(16))) float sm[2 * QS_T * QS_LD];   // A rows | B rows; then the tile (64 x 65); then the fold of the four q
    static_assert(2 * QS_T * QS_LD >= QS_T * QS_TP, "the tile reuses the staging buffer");
    __shared__ float kl[EPI == QS_KNN ? 4 * QS_KMAX * 64 : 1];            // [q][j][row]
    __shared__ float rad[EPI == QS_COUNT ? QS_T : 1];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int erow = tid & 63, eq = tid >> 6;                             // epilogue: row of the strip, quarter of the tile's columns
    const int split = blockIdx.x, row0 = blockIdx.y * QS_T, gi = row0 + erow;
    const int ntb = (p.Nb + QS_T - 1) / QS_T;
    const int t0 = split * p.tps, t1 = t0 + p.tps < ntb ? t0 + p.tps : ntb;
    float* mine = kl + (EPI == QS_KNN ? eq * QS_KMAX * 64 + erow : 0);
    float thr = INFINITY, mn = INFINITY;
    int cnt = 0;
    double sum = 0.0;
    if (EPI == QS_KNN)
        for (int j = 0; j < p.k; ++j) mine[j * 64] = INFINITY;
    const long long self = (long long)gi + p.self_col0;
    for (int t = t0; t < t1; ++t) {
        const int col0 = t * QS_T;
        float acc[4][4];
        qs_tile<VEC, EPI == QS_POLY>(p, row0, col0, sm, acc);
        __syncthreads();                                                  // everyone is done reading As / Bs
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) sm[(ty + 16 * r) * QS_TP + tx + 16 * c] = acc[r][c];
        if (EPI == QS_COUNT && p.radius2 && tid < QS_T) rad[tid] = col0 + tid < p.Nb ? p.radius2[col0 + tid] : 0.f;
        __syncthreads();
        const int jend = p.Nb - col0 < 16 * (eq + 1) ? p.Nb - col0 : 16 * (eq + 1);
        for (int j = 16 * eq; j < jend; ++j) {
            const float v = sm[erow * QS_TP + j];
            if (EPI == QS_KNN) {
                if (col0 + j != self) qs_offer(mine, p.k, v, thr);
            } else if (EPI == QS_COUNT) {
                mn = v < mn ? v : mn;
                if (p.radius2) cnt += v <= rad[j] ? 1 : 0;
            } else {
                if (!(p.exclude_diag && col0 + j == gi)) {
                    const double s = (double)v / (double)p.D + 1.0;
                    sum += s * s * s;
                }
            }
        }
    }
    __syncthreads();                                                      // the last tile has been read; every list is complete
    const long long o = (long long)split * p.Na + gi;
    if (EPI == QS_KNN) {
        if (eq == 0) {
            for (int q = 1; q < 4; ++q)
                for (int j = 0; j < p.k; ++j) {
                    const float v = kl[(q * QS_KMAX + j) * 64 + erow];
                    if (!(v < thr)) break;                                // ascending: nothing smaller follows
                    qs_offer(mine, p.k, v, thr);
                }
            if (gi < p.Na) {
                if (p.kth_only) p.klist[gi] = thr;
                else
                    for (int j = 0; j < p.k; ++j) p.klist[o * p.k + j] = mine[j * 64];
            }
        }
    } else if (EPI == QS_COUNT) {
        int* rc = reinterpret_cast<int*>(sm);
        float* rm = sm + 256;
        rc[tid] = cnt;
        rm[tid] = mn;
        __syncthreads();
        if (eq == 0 && gi < p.Na) {
            for (int q = 1; q < 4; ++q) {
                cnt += rc[q * 64 + erow];
                mn = rm[q * 64 + erow] < mn ? rm[q * 64 + erow] : mn;
            }
            if (p.radius2) p.count[o] = cnt;
            p.min_d2[o] = mn;
        }
    } else {
        double* rs = reinterpret_cast<double*>(sm);
        rs[tid] = sum;
        __syncthreads();
        if (eq == 0 && gi < p.Na) {
            for (int q = 1; q < 4; ++q) sum += rs[q * 64 + erow];        // in column order
            p.rowsum[o] = sum;
        }
    }
}

// The folds: one thread per row, the splits in split order.  grid cdiv(Na, 64), 64 threads.
__global__ __launch_bounds__(64) void qs_fold_knn_kernel(const float* __restrict__ part, int csplit, int Na, int k, float* __restrict__ out,
                                                         int kth_only) {
    __shared__ float kl[QS_KMAX * 64];
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Na) return;
    float* mine = kl + threadIdx.x;
    float thr = INFINITY;
    for (int j = 0; j < k; ++j) mine[j * 64] = INFINITY;
    for (int s = 0; s < csplit; ++s)
        for (int j = 0; j < k; ++j) {
            const float v = part[((long long)s * Na + i) * k + j];
            if (!(v < thr)) break;
            qs_offer(mine, k, v, thr);
        }
    if (kth_only) out[i] = thr;
    else
        for (int j = 0; j < k; ++j) out[(long long)i * k + j] = mine[j * 64];
}

__global__ __launch_bounds__(64) void qs_fold_count_kernel(const int* __restrict__ pc, const float* __restrict__ pm, int csplit, int Na,
                                                           int* __restrict__ count, float* __restrict__ min_d2) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Na) return;
    int c = 0;
    float m = INFINITY;
    for (int s = 0; s < csplit; ++s) {
        if (pc) c += pc[(long long)s * Na + i];
        const float v = pm[(long long)s * Na + i];
        m = v < m ? v : m;
    }
    if (pc) count[i] = c;
    min_d2[i] = m;
}

__global__ __launch_bounds__(64) void qs_fold_sum_kernel(const double* __restrict__ part, int csplit, int Na, double* __restrict__ rowsum) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Na) return;
    double s = 0.0;
    for (int c = 0; c < csplit; ++c) s += part[(long long)c * Na + i];
    rowsum[i] = s;
}

// Strips of a, column tiles of b, the largest split count this shape can get (the workspace bound) and the split used: as many
// splits as fill 8 workgroup slots per CU (pd_plan's rule), none empty.  D does not enter: it is never split.
struct QsPlan { int strips, ntb, cap, csplit, tps; };
static QsPlan qs_plan(int Na, int Nb) {
    QsPlan p;
    p.strips = (int)cdiv(Na, QS_T);
    p.ntb = (int)cdiv(Nb, QS_T);
    const int slots = 8 * device_cus();
    long long cap = slots / p.strips;
    if (cap > p.ntb) cap = p.ntb;
    p.cap = cap < 1 ? 1 : (int)cap;
    split_k(slots, p.strips, p.ntb, 1, p.csplit, p.tps);
    return p;
}

static size_t qs_workspace_bytes(int Na, int Nb, size_t per_row) {
    if (Na <= 0 || Nb <= 0) return 0;
    const QsPlan p = qs_plan(Na, Nb);
    return p.cap > 1 ? (size_t)p.cap * (size_t)Na * per_row : 0;
}

// the checks every entry point shares; `who` names it
static int qs_check(const char* who, const float* a, int64_t lda, int Na, const float* b, int64_t ldb, int Nb, int D, const void* workspace,
                    size_t workspace_bytes, size_t need) {
    BD_CHECK(a && b, BD_ERR_INVALID, "%s: null pointer", who);
    BD_CHECK(Na >= 1 && Nb >= 1 && D >= 1, BD_ERR_INVALID, "%s: Na=%d Nb=%d D=%d must be positive", who, Na, Nb, D);
    BD_CHECK(lda >= D && ldb >= D, BD_ERR_INVALID, "%s: row stride %lld / %lld < D=%d", who, (long long)lda, (long long)ldb, D);
    BD_CHECK((reinterpret_cast<uintptr_t>(a) & 3) == 0 && (reinterpret_cast<uintptr_t>(b) & 3) == 0, BD_ERR_INVALID,
             "%s: the rows must be 4-byte aligned", who);
    BD_CHECK(cdiv(Na, QS_T) <= 65535, BD_ERR_UNSUPPORTED, "%s: Na=%d too large for one launch", who, Na);
    BD_CHECK(workspace_bytes >= need && (workspace || !need), BD_ERR_WORKSPACE, "%s: workspace %zu < %zu", who,
             workspace ? workspace_bytes : (size_t)0, need);
    return BD_OK;
}

template <int EPI>
static void qs_launch(const QsArgs& p, const QsPlan& pl, hipStream_t s) {
    const dim3 grid((unsigned)pl.csplit, (unsigned)pl.strips);
    if (aligned16(p.a) && aligned16(p.b) && p.lda % 4 == 0 && p.ldb % 4 == 0)
        hipLaunchKernelGGL((qs_strip_kernel<true, EPI>), grid, dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((qs_strip_kernel<false, EPI>), grid, dim3(256), 0, s, p);
}

static int qs_ksmallest(const char* who, const float* a, int64_t lda, int Na, const float* b, int64_t ldb, int Nb, int D, int k,
                        int64_t self_col0, float* out, int kth_only, void* workspace, size_t workspace_bytes, bd_stream_t stream) {
    const size_t need = qs_workspace_bytes(Na, Nb, (size_t)k * sizeof(float));
    if (int st = qs_check(who, a, lda, Na, b, ldb, Nb, D, workspace, workspace_bytes, need)) return st;
    const QsPlan pl = qs_plan(Na, Nb);
    QsArgs p = {};
    p.a = a; p.lda = lda; p.Na = Na; p.b = b; p.ldb = ldb; p.Nb = Nb; p.D = D; p.tps = pl.tps; p.k = k; p.self_col0 = self_col0;
    const bool split = pl.csplit > 1;
    p.klist = split ? reinterpret_cast<float*>(workspace) : out;
    p.kth_only = split ? 0 : kth_only;
    qs_launch<QS_KNN>(p, pl, S(stream));
    BD_LAUNCH_CHECK(who);
    if (split) {
        hipLaunchKernelGGL(qs_fold_knn_kernel, dim3((unsigned)pl.strips), dim3(64), 0, S(stream), p.klist, pl.csplit, Na, k, out, kth_only);
        BD_LAUNCH_CHECK(who);
    }
    return BD_OK;
}

}  // namespace bd

using namespace bd;

extern "C" int bd_cross_plan(int Na, int Nb, int D, bd_cross_plan_info* out) {
    BD_CHECK(out, BD_ERR_INVALID, "bd_cross_plan: null output");
    BD_CHECK(Na >= 1 && Nb >= 1 && D >= 1, BD_ERR_INVALID, "bd_cross_plan: Na=%d Nb=%d D=%d must be positive", Na, Nb, D);
    const QsPlan p = qs_plan(Na, Nb);
    out->strips = p.strips;
    out->col_tiles = p.ntb;
    out->csplit = p.csplit;
    out->tiles_per_split = p.tps;
    out->csplit_cap = p.cap;
    return BD_OK;
}

extern "C" size_t bd_knn_sqradius_workspace_bytes(int N, int D, int k) {
    if (D <= 0 || k < 1 || k > QS_KMAX) return 0;
    return qs_workspace_bytes(N, N, (size_t)k * sizeof(float));
}

extern "C" int bd_knn_sqradius(const float* x, int64_t ldx, int N, int D, int k, float* out, void* workspace, size_t workspace_bytes,
                               bd_stream_t stream) {
    BD_CHECK(x && out, BD_ERR_INVALID, "bd_knn_sqradius: null pointer");
    BD_CHECK(k >= 1 && k <= QS_KMAX && k <= N - 1, BD_ERR_INVALID, "bd_knn_sqradius: k=%d must be in [1, min(%d, N - 1 = %d)]", k, QS_KMAX,
             N - 1);
    return qs_ksmallest("bd_knn_sqradius", x, ldx, N, x, ldx, N, D, k, 0, out, 1, workspace, workspace_bytes, stream);
}

extern "C" size_t bd_cross_ksmallest_workspace_bytes(int Na, int Nb, int D, int k) {
    if (D <= 0 || k < 1 || k > QS_KMAX) return 0;
    return qs_workspace_bytes(Na, Nb, (size_t)k * sizeof(float));
}

extern "C" int bd_cross_ksmallest(const float* a, int64_t lda, int Na, const float* b, int64_t ldb, int Nb, int D, int k, int64_t self_col0,
                                  float* out, void* workspace, size_t workspace_bytes, bd_stream_t stream) {
    BD_CHECK(a && b && out, BD_ERR_INVALID, "bd_cross_ksmallest: null pointer");
    BD_CHECK(k >= 1 && k <= QS_KMAX, BD_ERR_INVALID, "bd_cross_ksmallest: k=%d must be in [1, %d]", k, QS_KMAX);
    return qs_ksmallest("bd_cross_ksmallest", a, lda, Na, b, ldb, Nb, D, k, self_col0, out, 0, workspace, workspace_bytes, stream);
}

extern "C" size_t bd_cross_count_min_workspace_bytes(int Na, int Nb, int D) {
    if (D <= 0) return 0;
    return qs_workspace_bytes(Na, Nb, sizeof(int) + sizeof(float));
}

extern "C" int bd_cross_count_min(const float* a, int64_t lda, int Na, const float* b, int64_t ldb, int Nb, int D, const float* radius2,
                                  int32_t* count, float* min_d2, void* workspace, size_t workspace_bytes, bd_stream_t stream) {
    BD_CHECK(min_d2 && (count || !radius2), BD_ERR_INVALID, "bd_cross_count_min: null output");
    const size_t need = bd_cross_count_min_workspace_bytes(Na, Nb, D);
    if (int st = qs_check("bd_cross_count_min", a, lda, Na, b, ldb, Nb, D, workspace, workspace_bytes, need)) return st;
    const QsPlan pl = qs_plan(Na, Nb);
    QsArgs p = {};
    p.a = a; p.lda = lda; p.Na = Na; p.b = b; p.ldb = ldb; p.Nb = Nb; p.D = D; p.tps = pl.tps; p.radius2 = radius2;
    const bool split = pl.csplit > 1;
    int* pc = reinterpret_cast<int*>(workspace);                          // [cap][Na] counts, then [cap][Na] minima
    float* pm = reinterpret_cast<float*>(workspace) + (size_t)pl.cap * Na;
    p.count = split ? pc : count;
    p.min_d2 = split ? pm : min_d2;
    qs_launch<QS_COUNT>(p, pl, S(stream));
    BD_LAUNCH_CHECK("bd_cross_count_min");
    if (split) {
        hipLaunchKernelGGL(qs_fold_count_kernel, dim3((unsigned)pl.strips), dim3(64), 0, S(stream), radius2 ? pc : nullptr, pm, pl.csplit, Na,
                           count, min_d2);
        BD_LAUNCH_CHECK("bd_cross_count_min fold");
    }
    return BD_OK;
}

extern "C" size_t bd_poly3_rowsum_workspace_bytes(int Na, int Nb, int D) {
    if (D <= 0) return 0;
    return qs_workspace_bytes(Na, Nb, sizeof(double));
}

extern "C" int bd_poly3_rowsum(const float* a, int64_t lda, int Na, const float* b, int64_t ldb, int Nb, int D, int exclude_diag,
                               double* rowsum, void* workspace, size_t workspace_bytes, bd_stream_t stream) {
    BD_CHECK(rowsum, BD_ERR_INVALID, "bd_poly3_rowsum: null output");
    const size_t need = bd_poly3_rowsum_workspace_bytes(Na, Nb, D);
    if (int st = qs_check("bd_poly3_rowsum", a, lda, Na, b, ldb, Nb, D, workspace, workspace_bytes, need)) return st;
    BD_CHECK(!need || (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, BD_ERR_INVALID, "bd_poly3_rowsum: workspace must be 8-byte aligned");
    BD_CHECK((reinterpret_cast<uintptr_t>(rowsum) & 7) == 0, BD_ERR_INVALID, "bd_poly3_rowsum: rowsum must be 8-byte aligned");
    const QsPlan pl = qs_plan(Na, Nb);
    QsArgs p = {};
    p.a = a; p.lda = lda; p.Na = Na; p.b = b; p.ldb = ldb; p.Nb = Nb; p.D = D; p.tps = pl.tps; p.exclude_diag = exclude_diag ? 1 : 0;
    const bool split = pl.csplit > 1;
    p.rowsum = split ? reinterpret_cast<double*>(workspace) : rowsum;
    qs_launch<QS_POLY>(p, pl, S(stream));
    BD_LAUNCH_CHECK("bd_poly3_rowsum");
    if (split) {
        hipLaunchKernelGGL(qs_fold_sum_kernel, dim3((unsigned)pl.strips), dim3(64), 0, S(stream), p.rowsum, pl.csplit, Na, rowsum);
        BD_LAUNCH_CHECK("bd_poly3_rowsum fold");
    }
    return BD_OK;
}
