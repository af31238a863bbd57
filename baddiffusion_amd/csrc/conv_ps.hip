// 3x3 stride-1 "same" convolution and its data gradient on PRE-SPLIT operands, fed by LDS-DMA (gfx950).
//
// Same arithmetic as the split-bf16 igemm (igemm.hip: x = hi + lo, product = lo*hi + hi*lo + hi*hi on
// v_mfma_f32_32x32x16_bf16, fp32 accumulate, K order = channel block outer / filter tap inner) and bit-identical to it,
// but the operands arrive already split: producers (GroupNorm apply, GroupNorm backward, bd_split_rows) write the
// bf16 hi|lo planes in the blocked layout of bd_split_bf16 -- per row, every 32-channel block is one 128-byte line,
// 64 B of hi then 64 B of lo: the same 4 bytes per element as the fp32 tensor it replaces.  A K chunk (one tap, 32
// channels) of an operand row is then exactly one line, and the main loop has no VALU work on the data at all:
//   global --(global_load_lds_dwordx4, 16 B per lane, 8 lanes per row)--> LDS ring (3 stages of 256x128 + 128x128 B)
//   LDS --(ds_read_b128, XOR-swizzled slots: conflict-free)--> MFMA fragments.
// One workgroup = 8 waves (4 x 2) on a 256 x 128 tile (64 x 64 per wave), ONE barrier per K chunk; the DMA of chunk
// c+2 is issued right after the barrier that retires chunk c-1's stage and is waited for with a counted vmcnt two
// chunks later (cdna_hip_programming.md section 5, "Pipelining across barriers": raw s_barrier, never vmcnt(0) in the loop).
// Zero padding: lanes whose tap falls outside the image read a 16-byte zero page instead (branch-free).
// Single pass (SP template parameter, BD_MODE_BF16): the same DMA of whole 128-byte lines, but only the hi fragments are read from
// LDS and each product is the one MFMA hi*hi.  The weight-gradient kernels' bias gradient (ones-MFMA) keeps hi + lo of dY: the
// lo plane is still in LDS, and only the waves that own the bias row read it.  The lo halves of every line are still DMA'd; a
// hi-only DMA (half the operand bytes into LDS) is the next step for this mode.
//
// data gradient of the same convolution: dx[p][ci] = sum_{tap,co} dy[p - tap][co] * W[co][tap][ci] is the same kernel
// with the gather direction negated (sign = -1) over the TRANSPOSED weight planes Wt[ci][tap][co] (bd_split_wt).
// Replaces aten::convolution / convolution_backward(input) of resnet.py:493,514 for the stride-1 convolutions.
#include "splitplane.h"
#include <string.h>

#include <type_traits>
#include <cstdlib>

namespace bd {

constexpr int BD_WT_MAX = 64;   // weights per batched transpose launch (table passed by value)
constexpr int PS_BM = 256, PS_BN = 128, PS_NT = 512, PS_STAGES = 3;
constexpr int PS_A_BYTES = PS_BM * 128, PS_B_BYTES = PS_BN * 128, PS_STAGE_BYTES = PS_A_BYTES + PS_B_BYTES;
constexpr int PS_LDS_BYTES = PS_STAGES * PS_STAGE_BYTES;   // 147456 of 163840

struct PsParams {
    const char* a;        // activation planes: row m at a + m*lda*4, channel block cb at + cb*128 (64 B hi | 64 B lo)
    const char* w;        // weight planes [N][9][C]: row n, tap t, block cb at ((n*9 + t)*C + cb*32)*4
    float* y;
    const float* bias; const float* rowbias; const float* residual;
    long long lda, ldy, ldr, ld_rowbias;
    int C, H, W, lw, lhw;  // K channels ; image size (powers of two) and log2(W), log2(H*W)
    int sign;              // +1 forward gather (x[p + tap]), -1 data-gradient gather (dy[p - tap])
    int M, N, tiles_m, tiles_n;
    float out_scale;
    int accumulate;
    unsigned short* y_split; long long ldys;   // optional second output: y in split planes (same row count, ld)
    int lvw;               // conv_ps3_kernel: log2 of the VIRTUAL image width min(W, 32), see ps_v2r
    double* gn_part;       // conv_ps3_kernel, optional: [B][H*W/256][gn_G][2] partial (sum, sum of squares) of y per pixel tile and group
    int gn_G, gn_lcpg;     //   groups of the GroupNorm that reads y next; log2(channels per group), 2 .. 5
};

// Round 4: VIRTUAL pixel order.  The vertical-tap-sharing kernels (conv_ps3_kernel, conv_ps_wgrad3_kernel) want the rows one image row
// apart to sit a SMALL constant number of pixels apart in the order they walk the image (a 256 + 2W row LDS window, an X ring of 2W + 32
// pixels): fine for W <= 32, impossible for the 64 .. 256 wide layers of the 256 x 256 network.  Those are walked strip by strip instead:
// an image is cut into W/32 vertical strips of 32 columns and virtual pixel v = strip * (H * 32) + y * 32 + xs, so that one image row down is
// always v + 32 -- to the kernels every image looks 32 pixels wide and H * W / 32 rows tall, and only the address of a pixel (this
// function) and the "is the row above / below inside the image" test (y = (v >> 5) & (H - 1)) know about the real layout.  A 256-pixel tile is
// then an 8 x 32 pixel block, a 32-pixel chunk one strip row.  W <= 32: identity.
__device__ __forceinline__ int ps_v2r(int v, int lw, int lh, int lvw) {
    if (lw == lvw) return v;
    const int lhw = lw + lh;
    const int r = v & ((1 << lhw) - 1);
    return (v - r) + (((r >> lvw) & ((1 << lh) - 1)) << lw) + ((r >> (lh + lvw)) << lvw) + (r & ((1 << lvw) - 1));
}

// Epilogue of a wave's TM x 2 grid of 32x32 accumulator tiles: y = out_scale * (acc + bias + rowbias + residual) (+ y).
// The addends of a tile are loaded FIRST (16 independent loads each, all in flight), then combined and stored.  FULL
// (wave-uniform: every row of the sub-tile is < M) removes the per-element predicate: behind an exec-masked branch per
// element hipcc reuses one address register pair and waits vmcnt(0) for the previous store before every store -- a chain
// of ~64 serialised memory round trips per wave that used to be a large part of the per-tile overhead.
// mb[i] = the output row of the first of the 32 consecutive rows of the wave's i-th 32 x 32 tile (consecutive in memory: a virtual-order
// tile of conv_ps3_kernel is 8 image-row pieces of 32 pixels, see ps_v2r)
// STATS (round 4, conv_ps3_kernel only): st[q][0 / 1] += the lane's column sums of y and y * y over its 16 rows of every tile -- the
// statistics of the GroupNorm that reads y next come out of this epilogue instead of a pass over y (ps3_gn_partials)
template <int EPI, int TM, bool FULL, bool STATS = false>
__device__ __forceinline__ void ps_epilogue(const PsParams& p, sp_floatx16 (&acc)[TM][2], const int (&mb)[TM], int nw, int li, int h,
                                            float (*st)[2] = nullptr) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int n = nw + q * 32 + li;
            const float bn = p.bias ? p.bias[n] : 0.f;
            const int m_base = mb[i] + 4 * h;
            float ad[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) ad[r] = 0.f;
            float pc[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = FULL ? m_base + (r & 3) + 8 * (r >> 2) : min(m_base + (r & 3) + 8 * (r >> 2), p.M - 1);   // clamped: branch-free loads
                if constexpr (EPI & 2) ad[r] = p.rowbias[(long long)(m >> p.lhw) * p.ld_rowbias + n];
            }
            float rs[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = FULL ? m_base + (r & 3) + 8 * (r >> 2) : min(m_base + (r & 3) + 8 * (r >> 2), p.M - 1);
                rs[r] = 0.f; pc[r] = 0.f;
                if constexpr (EPI & 1) rs[r] = p.residual[(long long)m * p.ldr + n];
                if constexpr (EPI & 4) pc[r] = p.y[(long long)m * p.ldy + n];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m_base + (r & 3) + 8 * (r >> 2);
                float v = acc[i][q][r] + bn;
                if constexpr (EPI & 2) v += ad[r];
                if constexpr (EPI & 1) v += rs[r];
                v *= p.out_scale;
                if constexpr (EPI & 4) v += pc[r];
                if (FULL || m < p.M) p.y[(long long)m * p.ldy + n] = v;
                if constexpr (STATS) { st[q][0] += v; st[q][1] += v * v; }
            }
        }
}

// The GroupNorm statistics of a 256 x 128 output tile: the lanes' column sums (ps_epilogue<STATS>) are folded over the two half waves and the
// cpg = 4 .. 32 adjacent columns of a group by lane exchanges, over the four wave rows through LDS (fixed order, fp64), and thread g writes the
// partial of group n0 / cpg + g.  A tile lies inside one sample (H * W % 256 == 0), so the partials are [B][H*W/256][G][2]: what gn_stats_kernel
// writes for S = H*W/256 pixel splits -- the finalize kernel of groupnorm.hip reads either.
__device__ __forceinline__ void ps3_gn_partials(const PsParams& p, float (&st)[2][2], float* red /* LDS, >= 4 * 32 * 2 floats */, int m0, int n0,
                                                int wm, int wn, int li, int h, int tid) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            float v = st[q][k];
            v += __shfl_xor(v, 32);
            v += __shfl_xor(v, 1);
            v += __shfl_xor(v, 2);
            if (p.gn_lcpg > 2) v += __shfl_xor(v, 4);
            if (p.gn_lcpg > 3) v += __shfl_xor(v, 8);
            if (p.gn_lcpg > 4) v += __shfl_xor(v, 16);
            st[q][k] = v;
        }
    __syncthreads();                                       // every wave is done with the operand windows
    if (h == 0 && (li & ((1 << p.gn_lcpg) - 1)) == 0) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int g = (wn * 64 + q * 32 + li) >> p.gn_lcpg;
            red[(wm * 32 + g) * 2 + 0] = st[q][0];
            red[(wm * 32 + g) * 2 + 1] = st[q][1];
        }
    }
    __syncthreads();
    const int ng = PS_BN >> p.gn_lcpg;
    if (tid < ng) {
        double a = 0.0, c2 = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { a += (double)red[(w * 32 + tid) * 2 + 0]; c2 += (double)red[(w * 32 + tid) * 2 + 1]; }
        const int b = m0 >> p.lhw, s = (m0 & ((1 << p.lhw) - 1)) >> 8, S = 1 << (p.lhw - 8);
        double* o = p.gn_part + (((long long)b * S + s) * p.gn_G + (n0 >> p.gn_lcpg) + tid) * 2;
        o[0] = a;
        o[1] = c2;
    }
}

// EPI bits: 1 = residual, 2 = per-sample row bias, 4 = accumulate into y
// All eight waves run in lock step, one barrier per chunk.  (A ping-pong schedule -- the two waves of a SIMD one phase
// apart, four barriers per chunk -- and a wave-specialised form with four extra DMA-only loader waves were built and
// measured: bit-identical, and within +-2 % of this form on every layer)
template <int EPI, bool SP>
__global__ __launch_bounds__(PS_NT, 2) void conv_ps_kernel(PsParams p) {
    __shared__ __attribute__((aligned(128))) char smem[PS_LDS_BYTES];   // ONE LDS object (guide section 5, trap (a))

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, h = lane >> 5;

    // XCD-contiguous tile order (n fastest): tiles sharing an A panel meet in one L2 (common.h xcd_tile_order)
    int tm, tn;
    {
        const unsigned j = xcd_tile_order();
        tm = j / p.tiles_n;
        tn = j - tm * p.tiles_n;
    }
    const int m0 = tm * PS_BM, n0 = tn * PS_BN;

    // ---- DMA state: wave w moves row groups (8 rows x 128 B = one 1-KiB instruction) w, w+8, w+16, w+24 of A and
    // w, w+8 of B.  Lane l: row = 8*rg + l/8, physical slot l%8 <- logical slot (l%8) ^ swz(row).
    const int dr = lane >> 3, ps = lane & 7;
    const char* ap[4];
    int vm[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = (wave + 8 * j) * 8 + dr;
        const int m = m0 + r;
        const int x = m & (p.W - 1), y = (m >> p.lw) & (p.H - 1);
        int mask = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y + p.sign * (t / 3 - 1), xx = x + p.sign * (t % 3 - 1);
            if ((unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W) mask |= 1 << t;
        }
        vm[j] = m < p.M ? mask : 0;
        ap[j] = p.a + (long long)m * p.lda * 4 + ((ps ^ sp_swz(r)) << 4);
    }
    const char* wp[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = (wave + 8 * j) * 8 + dr;
        int n = n0 + r;
        if (n >= p.N) n = p.N - 1;
        wp[j] = p.w + (long long)n * 36 * p.C + ((ps ^ sp_swz(r)) << 4);
    }
    const int pix_bytes = (int)p.lda * 4;   // bytes between pixels (host checks (W + 1) * pix_bytes < 2^31)
    const int nchunks = 9 * (p.C >> 5);

    // chunk q -> (channel block cb, tap): K order = channel block outer, tap inner (the 9 taps share one input window)
    // cursor of the NEXT chunk to issue, all wave-uniform: tap = 3*kh + kw, byte offsets of the tap / channel block
    int q_kh = 0, q_kw = 0, q_bit = 1;
    int q_aoff = -p.sign * (p.W + 1) * pix_bytes, q_woff = 0;   // tap (0,0) of block 0
    auto issue = [&](char* stage) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sp_dma16((vm[j] & q_bit) ? ap[j] + q_aoff : reinterpret_cast<const char*>(bd_zero16), stage + (wave + 8 * j) * 1024);
#pragma unroll
        for (int j = 0; j < 2; ++j) sp_dma16(wp[j] + q_woff, stage + PS_A_BYTES + (wave + 8 * j) * 1024);
        // advance: kw fastest; a full window moves on to the next 32-channel block
        q_bit <<= 1;
        q_woff += p.C * 4;
        q_aoff += p.sign * pix_bytes;
        if (++q_kw == 3) {
            q_kw = 0;
            q_aoff += p.sign * (p.W - 3) * pix_bytes;
            if (++q_kh == 3) {
                q_kh = 0; q_bit = 1;
                q_aoff += 128 - p.sign * 3 * p.W * pix_bytes;
                q_woff += 128 - 9 * p.C * 4;
            }
        }
    };

    // ---- fragment addresses: lane -> row li of a 32-row tile, k octet h; logical slot = plane*4 + step*2 + h
    int foff[2][2];
    sp_frag_offsets(foff, li, h);
    const int abase = wm * 64 * 128, bbase = PS_A_BYTES + wn * 64 * 128;

    sp_floatx16 acc[2][2] = {};

    auto compute = [&](const char* stage) { sp_mma_chunk<SP>(stage + abase, stage + bbase, foff, acc); };

    char* const st0 = smem;
    char* const st1 = smem + PS_STAGE_BYTES;
    char* const st2 = smem + 2 * PS_STAGE_BYTES;

    // prologue: chunks 0 and 1 in flight (nchunks >= 9)
    issue(st0);
    issue(st1);
    // steady state, 3 chunks per trip (nchunks % 9 == 0): wait for chunk c (6 DMAs per wave and chunk, so vmcnt(6) leaves
    // chunk c+1 in flight), barrier (chunk c visible to everyone, chunk c-1's stage free), refill that stage with chunk c+2
    const int trips = nchunks / 3;
    for (int t = 0; t + 1 < trips; ++t) {
        sp_sync<6>(); issue(st2); compute(st0);
        sp_sync<6>(); issue(st0); compute(st1);
        sp_sync<6>(); issue(st1); compute(st2);
    }
    sp_sync<6>(); issue(st2); compute(st0);
    sp_sync<6>(); compute(st1);
    sp_sync<0>(); compute(st2);

    // ---- epilogue: lane holds column n = li of rows (r&3) + 8*(r>>2) + 4*h of every 32x32 tile
    const int mw = m0 + wm * 64, nw = n0 + wn * 64;
    const int mb[2] = {mw, mw + 32};
    if (mw + 64 <= p.M) ps_epilogue<EPI, 2, true>(p, acc, mb, nw, li, h);    // wave-uniform: whole sub-tile inside M
    else ps_epilogue<EPI, 2, false>(p, acc, mb, nw, li, h);
}

// ---------------------------------------------------------------------------------------------------------------------
// Round 3: the same 256 x 128 tile with the three VERTICAL taps of a column shift served from ONE LDS window.
// The tile's pixels are consecutive, so the A tiles of taps (ky, kx), ky = 0..2, are the same rows shifted by W pixels: one window
// of 256 + 2W rows (the tile plus one image row above and below) is DMA'd once per (32-channel block, kx) and the three ky taps read
// it at row offsets 0 / W / 2W -- a constant byte offset, and (W/2) % 8 == 0 keeps the bank swizzle of a row unchanged.  Rows above /
// below the image and columns shifted out of it read the zero page as before: no masks, no VALU in the loop.  L2 -> LDS bytes per
// channel block: 3 x 40 KB + 9 x 16 KB = 264 KB instead of 9 x 48 KB = 432 KB.  W in {16, 32} (window <= 320 rows), K order = channel
// block outer, kx, ky inner (another fp32 summation order than conv_ps_kernel: same products).
// LDS: two A windows (2 x 40 KB) + a ring of three weight chunks (3 x 16 KB) = 128 KB.
constexpr int PS3_WIN_ROWS = 320, PS3_A_BYTES = PS3_WIN_ROWS * 128, PS3_B_BYTES = 128 * 128;
constexpr int PS3_LDS_BYTES = 2 * PS3_A_BYTES + 3 * PS3_B_BYTES;

template <int EPI, bool SP>
__global__ __launch_bounds__(PS_NT, 2) void conv_ps3_kernel(PsParams p) {
    __shared__ __attribute__((aligned(128))) char smem[PS3_LDS_BYTES];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, h = lane >> 5;
    int tm, tn;
    {
        const unsigned j = xcd_tile_order();
        tm = j / p.tiles_n;
        tn = j - tm * p.tiles_n;
    }
    const int m0 = tm * PS_BM, n0 = tn * PS_BN;

    // ---- A window: wave w moves row groups (8 rows = one 1-KiB DMA) w, w+8, .., w+32 of the 320-row window; window row wr is
    // (virtual) pixel m0 - VW + wr.  Per row: validity of the image row, and of the three column shifts.
    const int dr = lane >> 3, ps = lane & 7;
    const char* ap[5];
    int vm[5];
    // (m0 and the window rows are VIRTUAL pixels, ps_v2r: VW = min(W, 32) wide rows; a tile = 256 / VW rows of one strip of one image)
    const int VW = 1 << p.lvw, lh = p.lhw - p.lw;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int wr = (wave + 8 * j) * 8 + dr;
        const int m = ps_v2r(m0 - VW + wr, p.lw, lh, p.lvw);  // may be < 0 or past the image: masked below
        const int x = m & (p.W - 1);
        const int yrel = (wr >> p.lvw) - 1;                  // image row relative to the tile's first row
        const int y0 = (m0 >> p.lvw) & (p.H - 1);
        const int yy = y0 + yrel;
        int mask = 0;
        if ((unsigned)yy < (unsigned)p.H && wr < PS_BM + 2 * VW) {       // (tiles never straddle strips / images: H * VW % 256 == 0, host-checked)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
                if ((unsigned)(x + p.sign * (kx - 1)) < (unsigned)p.W) mask |= 1 << kx;
        }
        vm[j] = mask;
        ap[j] = p.a + (long long)m * p.lda * 4 + ((ps ^ sp_swz(wr)) << 4);
    }
    const char* wp[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = (wave + 8 * j) * 8 + dr;
        int n = n0 + r;
        if (n >= p.N) n = p.N - 1;
        wp[j] = p.w + (long long)n * 36 * p.C + ((ps ^ sp_swz(r)) << 4);
    }
    const int pix_bytes = (int)p.lda * 4;
    const int ngroups = 3 * (p.C >> 5);          // (channel block, kx)
    const int nchunks = 3 * ngroups;

    // cursors (wave-uniform): next A group (cb, kx), next weight chunk (cb, kx, ky)
    int ga_kx = 0, ga_cb = 0;
    auto issue_a = [&](char* win) {
        const int aoff = p.sign * (ga_kx - 1) * pix_bytes + ga_cb * 128;
        const int bit = 1 << ga_kx;
#pragma unroll
        for (int j = 0; j < 5; ++j) sp_dma16((vm[j] & bit) ? ap[j] + aoff : reinterpret_cast<const char*>(bd_zero16), win + (wave + 8 * j) * 1024);
        if (++ga_kx == 3) { ga_kx = 0; ++ga_cb; }
    };
    int gb_ky = 0, gb_kx = 0, gb_cb = 0;
    auto issue_b = [&](char* slot) {
        const int woff = ((gb_ky * 3 + gb_kx) * p.C + gb_cb * 32) * 4;
#pragma unroll
        for (int j = 0; j < 2; ++j) sp_dma16(wp[j] + woff, slot + (wave + 8 * j) * 1024);
        if (++gb_ky == 3) { gb_ky = 0; if (++gb_kx == 3) { gb_kx = 0; ++gb_cb; } }
    };

    int foff[2][2];
    sp_frag_offsets(foff, li, h);
    const int abase = wm * 64 * 128, bbase = wn * 64 * 128;
    // vertical tap ky of the forward gather reads window rows r + ky*VW; the data-gradient gather (sign -1) mirrors it
    const int wrow_bytes = VW * 128;

    sp_floatx16 acc[2][2] = {};

    auto compute = [&](const char* win, const char* bslot, int ky) {
        const char* a0 = win + abase + (p.sign > 0 ? ky : 2 - ky) * wrow_bytes;
        sp_mma_chunk<SP>(a0, bslot + bbase, foff, acc);
    };

    char* const A0 = smem; char* const A1 = smem + PS3_A_BYTES;
    char* const B0 = smem + 2 * PS3_A_BYTES; char* const B1 = B0 + PS3_B_BYTES; char* const B2 = B1 + PS3_B_BYTES;

    // issue order per wave: A(0) [5 DMAs], B(0) [2], B(1) [2]; then behind the barrier of chunk c = 3g + ky:
    //   ky == 0: A(g+1) [5] and B(c+2) [2];  ky == 1, 2: B(c+2) [2].
    // Chunk c needs B(c) -- and everything issued before it, i.e. A(g) -- landed: DMAs issued after B(c) are
    //   ky == 0: B(c+1) = 2;   ky == 1: A(g+1) + B(c+1) = 7;   ky == 2: B(c+1) = 2.
    issue_a(A0);
    issue_b(B0);
    issue_b(B1);
    // two groups (six chunks) per trip so that the A windows and the three weight slots are compile-time addresses
    for (int g = 0; g < ngroups; g += 2) {
        const bool more1 = g + 1 < ngroups, more2 = g + 2 < ngroups;
        // group g on A0: chunks 3g .. 3g+2 on slots (3g) % 3 = 0, 1, 2 (3g is a multiple of 3)
        sp_sync<2>(); if (more1) issue_a(A1); issue_b(B2); compute(A0, B0, 0);
        if (more1) sp_sync<7>(); else sp_sync<2>();
        if (more1) issue_b(B0); compute(A0, B1, 1);
        if (more1) sp_sync<2>(); else sp_sync<0>();
        if (more1) issue_b(B1); compute(A0, B2, 2);
        if (!more1) break;
        // group g + 1 on A1
        sp_sync<2>(); if (more2) issue_a(A0); issue_b(B2); compute(A1, B0, 0);
        if (more2) sp_sync<7>(); else sp_sync<2>();
        if (more2) issue_b(B0); compute(A1, B1, 1);
        if (more2) sp_sync<2>(); else sp_sync<0>();
        if (more2) issue_b(B1); compute(A1, B2, 2);
    }
    (void)nchunks;

    // output rows: the wave's two 32-pixel blocks, virtual -> real (32 consecutive virtual pixels are consecutive in memory)
    const int nw = n0 + wn * 64;
    const int mb[2] = {ps_v2r(m0 + wm * 64, p.lw, lh, p.lvw), ps_v2r(m0 + wm * 64 + 32, p.lw, lh, p.lvw)};
    if constexpr (EPI == 1 || EPI == 2) {                    // (forward conv1 / conv2 of a resnet: the producers of a GroupNorm's input)
        if (p.gn_part) {                                     // kernel-uniform
            float st[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
            ps_epilogue<EPI, 2, true, true>(p, acc, mb, nw, li, h, st);
            ps3_gn_partials(p, st, reinterpret_cast<float*>(smem), m0, n0, wm, wn, li, h, tid);
            return;
        }
    }
    ps_epilogue<EPI, 2, true>(p, acc, mb, nw, li, h);        // (M % 256 == 0: every tile is whole, host-checked)
}

// ---------------------------------------------------------------------------------------------------------------------
// 128 x 128 tile variant for the SMALL layers (8x8 / 4x4 images: too few 256 x 128 tiles to fill the chip): same operands,
// same fragment layout, 8 waves of 32 x 64, two LDS stages (64 KB -> two workgroups per CU, which de-phase), and the K
// chunks (tap, 32 channels) split over `ksplit` workgroups per tile: partial slabs + a fixed-order second pass that also
// applies the epilogue (deterministic, no atomics).
struct PsSmallParams {
    PsParams q;
    float* partial;        // [ksplit][M][N] when ksplit > 1
    int ksplit, cps;       // chunks per split
};

// STAGES = 2: 64 KB, two workgroups per CU (the pair de-phases); the chunk c+1 is fetched while chunk c computes.
// STAGES = 4 (round 6): 128 KB, one workgroup per CU, THREE chunks in flight ahead of the one being computed -- for the short K slices of
// the 4 x 4 level (4 - 9 chunks per workgroup), where a workgroup's life is a handful of DMA round trips and the two-stage form exposes one
// L2 -> LDS latency per chunk.
template <int EPI, bool SP, int STAGES = 2>
__global__ __launch_bounds__(512, STAGES == 2 ? 4 : 2) void conv_ps128_kernel(PsSmallParams pp) {
    const PsParams& p = pp.q;
    constexpr int A_BYTES = 128 * 128, STAGE = 2 * A_BYTES;
    __shared__ __attribute__((aligned(128))) char smem[STAGES * STAGE];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, h = lane >> 5;
    int tm, tn, zz;
    {
        const unsigned j = xcd_tile_order();
        const unsigned ntiles = p.tiles_m * p.tiles_n;
        zz = j / ntiles;
        const unsigned tile = j - zz * ntiles;
        tm = tile / p.tiles_n;
        tn = tile - tm * p.tiles_n;
    }
    const int m0 = tm * 128, n0 = tn * 128;
    const int nchunks = 9 * (p.C >> 5);
    const int c_begin = zz * pp.cps;
    int c_end = c_begin + pp.cps;
    if (c_end > nchunks) c_end = nchunks;

    const int dr = lane >> 3, ps = lane & 7;
    const char* ap[2]; const char* wp[2];
    int vm[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = (wave + 8 * j) * 8 + dr;
        const int m = m0 + r;
        const int x = m & (p.W - 1), y = (m >> p.lw) & (p.H - 1);
        int mask = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y + p.sign * (t / 3 - 1), xx = x + p.sign * (t % 3 - 1);
            if ((unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W) mask |= 1 << t;
        }
        vm[j] = m < p.M ? mask : 0;
        ap[j] = p.a + (long long)m * p.lda * 4 + ((ps ^ sp_swz(r)) << 4);
        int n = n0 + r;
        if (n >= p.N) n = p.N - 1;
        wp[j] = p.w + (long long)n * 36 * p.C + ((ps ^ sp_swz(r)) << 4);
    }
    const int pix_bytes = (int)p.lda * 4;
    int q_cb = c_begin / 9;
    int q_tap = c_begin - 9 * q_cb;
    int q_kh = q_tap / 3, q_kw = q_tap - 3 * q_kh, q_bit = 1 << q_tap;
    int q_aoff = p.sign * ((q_kh - 1) * p.W + (q_kw - 1)) * pix_bytes + q_cb * 128;
    int q_woff = (q_tap * p.C + q_cb * 32) * 4;
    auto issue = [&](char* stage) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            sp_dma16((vm[j] & q_bit) ? ap[j] + q_aoff : reinterpret_cast<const char*>(bd_zero16), stage + (wave + 8 * j) * 1024);
            sp_dma16(wp[j] + q_woff, stage + A_BYTES + (wave + 8 * j) * 1024);
        }
        q_bit <<= 1;
        q_woff += p.C * 4;
        q_aoff += p.sign * pix_bytes;
        if (++q_kw == 3) {
            q_kw = 0;
            q_aoff += p.sign * (p.W - 3) * pix_bytes;
            if (++q_kh == 3) {
                q_kh = 0; q_bit = 1;
                q_aoff += 128 - p.sign * 3 * p.W * pix_bytes;
                q_woff += 128 - 9 * p.C * 4;
            }
        }
    };
    int foff[2][2];
    sp_frag_offsets(foff, li, h);
    const int abase = wm * 32 * 128, bbase = A_BYTES + wn * 64 * 128;
    sp_floatx16 acc[1][2] = {};
    auto compute = [&](const char* stage) { sp_mma_chunk<SP>(stage + abase, stage + bbase, foff, acc); };
    const int n = c_end - c_begin;
    if constexpr (STAGES == 2) {
        if (n > 0) issue(smem);
        for (int c = 0; c < n; ++c) {
            sp_sync<0>();
            if (c + 1 < n) issue(smem + ((c + 1) & 1) * STAGE);
            compute(smem + (c & 1) * STAGE);
        }
    } else {
        // ring of STAGES: chunks c+1 .. c+STAGES-1 are in flight while chunk c computes (4 DMAs per wave and chunk: counted waits).  The stage
        // refilled behind the barrier of chunk c is the one chunk c-1 was read from: every wave has passed that barrier with its reads returned.
#pragma unroll
        for (int k = 0; k < STAGES - 1; ++k)
            if (k < n) issue(smem + k * STAGE);
        for (int c = 0; c < n; ++c) {
            const int later = (n < c + STAGES - 1 ? n : c + STAGES - 1) - (c + 1);      // chunks issued after chunk c (wave-uniform)
            if (later >= 2) sp_wait<8>();
            else if (later == 1) sp_wait<4>();
            else sp_wait<0>();
            __builtin_amdgcn_s_barrier();
            if (c + STAGES - 1 < n) issue(smem + ((c + STAGES - 1) % STAGES) * STAGE);
            compute(smem + (c % STAGES) * STAGE);
        }
    }
    const int mw = m0 + wm * 32, nw = n0 + wn * 64;
    const bool full = mw + 32 <= p.M;     // wave-uniform
    if (pp.ksplit > 1) {
        float* out = pp.partial + (long long)zz * p.M * p.N;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int nn = nw + q * 32 + li;
            if (full) {
#pragma unroll
                for (int r = 0; r < 16; ++r) out[(long long)(mw + (r & 3) + 8 * (r >> 2) + 4 * h) * p.N + nn] = acc[0][q][r];
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = mw + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (m < p.M) out[(long long)m * p.N + nn] = acc[0][q][r];
                }
            }
        }
        return;
    }
    const int mb[1] = {mw};
    if (full) ps_epilogue<EPI, 1, true>(p, acc, mb, nw, li, h);
    else ps_epilogue<EPI, 1, false>(p, acc, mb, nw, li, h);
}

// second pass of the K split: fixed-order sum of the slabs + the epilogue, float4 per thread (N % 4 == 0)
__global__ __launch_bounds__(256) void conv_ps128_reduce(PsSmallParams pp) {
    const PsParams& p = pp.q;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int n4 = p.N >> 2;
    if (i >= (long long)p.M * n4) return;
    const int m = (int)(i / n4), nn = (int)(i - (long long)m * n4) * 4;
    const long long mn = (long long)p.M * p.N, e = (long long)m * p.N + nn;
    float4 a = *reinterpret_cast<const float4*>(pp.partial + e);
#pragma unroll 4      // four slab loads in flight; the additions keep their fixed order
    for (int s = 1; s < pp.ksplit; ++s) {
        const float4 b = *reinterpret_cast<const float4*>(pp.partial + (long long)s * mn + e);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    float v[4] = {a.x, a.y, a.z, a.w};
    if (p.bias) {
        const float4 b = *reinterpret_cast<const float4*>(p.bias + nn);
        v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
    }
    if (p.rowbias) {
        const float4 b = *reinterpret_cast<const float4*>(p.rowbias + (long long)(m >> p.lhw) * p.ld_rowbias + nn);
        v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
    }
    if (p.residual) {
        const float4 b = *reinterpret_cast<const float4*>(p.residual + (long long)m * p.ldr + nn);
        v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] *= p.out_scale;
    float4* dst = reinterpret_cast<float4*>(p.y + (long long)m * p.ldy + nn);
    if (p.accumulate) {
        const float4 b = *dst;
        v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
    }
    *dst = make_float4(v[0], v[1], v[2], v[3]);
}

// =====================================================================================================================
// Weight gradient of the same convolutions on split planes:  dW[co][tap][ci] = sum_p dY[p][co] * X[p + tap][ci]
//   GEMM view: M = Cout, N = 9*Cin (n = tap*Cin + ci), K = pixels.  Both operands are pixel-major ("row contiguous" in
//   igemm.hip's terms), so a K chunk of 32 pixels x 128 channels is 32 rows of 512 contiguous bytes: two pixels per 1-KiB
//   DMA instruction, and the MFMA fragments (k along pixels) are gathered with the hardware transpose read
//   ds_read_b64_tr_b16.  LDS image of a chunk: [32 pixels][512 B]; pixel k's 16-byte slots are XOR-permuted by
//   (k & 3) << 2 on the SOURCE side of the DMA (cdna guide rule 21), which puts the four pixels a transpose read touches
//   on four different 64-byte bank windows: conflict-free.
//   One workgroup = 8 waves (4 x 2) on a 128 (co) x 128 (one tap, 128 ci) tile, 32 x 64 per wave; K is split over
//   ksplit workgroups per tile (fixed-order second pass, deterministic).  The bias gradient sum_p dY[p][co] rides along
//   as two extra MFMAs against a vector of ones in the tn == 0 workgroups.
// Replaces aten::convolution_backward(weight, bias) of resnet.py:493,514 for the stride-1 convolutions.
constexpr int WG_BM = 128, WG_BN = 128, WG_OP_BYTES = 32 * 512, WG_STAGE_BYTES = 2 * WG_OP_BYTES;

struct PsWgParams {
    const char* dy; const char* x;     // split planes: dY [P][lddy], X [P][ldx]
    long long lddy, ldx;
    float* out;                        // ksplit == 1: dW [M][N]; else partial slabs [ksplit][M][N] then [ksplit][M] bias rows
    float* db;                         // ksplit == 1 only (else the reduce pass writes it); may be null
    int Cin, Cout, H, W, lw;           // image grid (powers of two)
    int P;                             // pixels = K
    int tiles_m, tiles_n, ksplit, cps; // chunks (of 32 pixels) per split
    int want_db;
    int ntaps;                         // taps per output row: 9, or 16 in the PHASE form (conv_ph.hip: upsample convolution)
    int lh, lvw;                       // conv_ps_wgrad3_kernel: log2(H), log2 of the virtual image width min(W, 32) (ps_v2r)
};

// STAGES = 2 and NW = 8 only: two LDS stages, the chunk c+1 is fetched while chunk c computes; waves 4 x 2, 32 x 64 each.  (NW = 4 --
// waves 2 x 2 of 64 x 64, a third fewer LDS fragment reads per MFMA -- measured within +-2 % of NW = 8 on every layer; one form is kept.)
// Both stay template parameters: the kernel's name, which profiles match on.
// PH = true: the PHASE form for the upsample convolution (conv_ph.hip).  H x W is the SOURCE grid, X lives on it, dY on the 2H x 2W
// grid; the 16 "taps" e = (oy+1)*4 + (ox+1) are the entries of E: entry (oy, ox) belongs to pixel class (p, q) of the fine grid and
// to the source-grid shift (dy, dx) with oy -> (p, dy): -1 -> (1, +1), 0 -> (0, 0), 1 -> (1, 0), 2 -> (0, -1):
//     dE[e][co][ci] = sum_{source pixels (a, b)} dY[2a+p, 2b+q][co] * X[a+dy, b+dx][ci].
// The bias gradient (sum of ALL dY) rides in the four (dy, dx) = (0, 0) entries, one bias row per class and K split.
template <int STAGES, int NW, bool SP, bool PH = false>
__global__ __launch_bounds__(NW * 64, 2) void conv_ps_wgrad_kernel(PsWgParams p) {
    static_assert(STAGES == 2 && NW == 8, "conv_ps_wgrad_kernel: one form (two stages, eight waves)");
    constexpr int TMW = 8 / NW;        // 32-row co tiles per wave
    constexpr int NDMA = 16 / NW;      // pixel pairs per wave, operand and chunk
    __shared__ __attribute__((aligned(128))) char smem[STAGES * WG_STAGE_BYTES];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;

    // logical order: n fastest, then m, then the K split; one contiguous run per XCD (same k-slice -> same L2)
    int tm, tn, zz;
    {
        const unsigned j = xcd_tile_order();
        const unsigned ntiles = p.tiles_m * p.tiles_n;
        zz = j / ntiles;
        const unsigned tile = j - zz * ntiles;
        tm = tile / p.tiles_n;
        tn = tile - tm * p.tiles_n;
    }
    const int co0 = tm * WG_BM, n0 = tn * WG_BN;
    const int tap = n0 / p.Cin, ci0 = n0 - tap * p.Cin;
    int dyt, dxt, cp = 0, cq = 0;
    if constexpr (PH) {
        const int oy = tap / 4 - 1, ox = (tap & 3) - 1;
        cp = oy & 1; cq = ox & 1;                                   // oy in {-1, 1} -> class row 1, {0, 2} -> 0
        dyt = oy == 2 ? -1 : (oy == -1 ? 1 : 0); dxt = ox == 2 ? -1 : (ox == -1 ? 1 : 0);
    } else {
        dyt = tap / 3 - 1; dxt = tap - (tap / 3) * 3 - 1;
    }
    const long long fine_off = (long long)cp * 2 * p.W + cq;        // PH: dY row of source pixel i = 4i - 2(i & (W-1)) + fine_off
    const int nchunks = (p.P + 31) >> 5;   // a ragged last chunk reads zeros past the last pixel
    const int c_begin = zz * p.cps;
    int c_end = c_begin + p.cps;
    if (c_end > nchunks) c_end = nchunks;

    // ---- DMA: wave w moves pixel pairs w and w + 8 of both operands; lane: pixel k = 2*pair + lane/32, slot lane%32
    const int ps = lane & 31;
    const char* asrc[NDMA]; const char* bsrc[NDMA];
    int kpix[NDMA];
#pragma unroll
    for (int j = 0; j < NDMA; ++j) {
        const int k = 2 * (wave + NW * j) + (lane >> 5);
        kpix[j] = k;
        const int ls = ps ^ ((k & 3) << 2);
        const long long pa = (long long)c_begin * 32 + k;
        asrc[j] = PH ? p.dy + co0 * 4 + ls * 16 : p.dy + pa * p.lddy * 4 + co0 * 4 + ls * 16;
        bsrc[j] = p.x + (pa + dyt * p.W + dxt) * p.ldx * 4 + ci0 * 4 + ls * 16;
    }
    const long long a_adv = 32 * p.lddy * 4, b_adv = 32 * p.ldx * 4;
    int q_pix = c_begin * 32;   // first pixel of the next chunk to issue
    auto issue_j = [&](char* stage, int j) {
        const int pp = q_pix + kpix[j];
        const int x = pp & (p.W - 1), y = (pp >> p.lw) & (p.H - 1);
        const bool in = pp < p.P;
        const bool ok = in && (unsigned)(y + dyt) < (unsigned)p.H && (unsigned)(x + dxt) < (unsigned)p.W;
        if constexpr (PH) {
            const long long fr = 4ll * pp - 2 * x + fine_off;       // pixel (2a+p, 2b+q) of the fine grid, x = pp & (W-1)
            sp_dma16(in ? asrc[j] + fr * p.lddy * 4 : reinterpret_cast<const char*>(bd_zero16), stage + (wave + NW * j) * 1024);
        } else {
            sp_dma16(in ? asrc[j] : reinterpret_cast<const char*>(bd_zero16), stage + (wave + NW * j) * 1024);
            asrc[j] += a_adv;
        }
        sp_dma16(ok ? bsrc[j] : reinterpret_cast<const char*>(bd_zero16), stage + WG_OP_BYTES + (wave + NW * j) * 1024);
        bsrc[j] += b_adv;
    };
    auto issue = [&](char* stage) {
#pragma unroll
        for (int j = 0; j < NDMA; ++j) issue_j(stage, j);
        q_pix += 32;
    };

    // ---- fragment addresses (ds_read_b64_tr_b16, see igemm.hip rc_frag): lane reads 4 rows x 1 pixel (8 bytes)
    const int sl = lane & 15, hb = (lane >> 4) & 1, h = lane >> 5;
    const int kq = sl >> 2, rq = sl & 3;
    const int lane_base = (8 * h + kq) * 512 + hb * 32 + rq * 8;
    int xw[4];   // 64-byte window of (tile parity, plane) after the per-pixel XOR
#pragma unroll
    for (int v = 0; v < 4; ++v) xw[v] = (v ^ kq) << 6;
    auto foff = [&](int t, int plane, int kk) { return lane_base + xw[(t & 1) * 2 + plane] + (t >> 1) * 256 + kk * 512; };

    sp_floatx16 acc[TMW][2], accb[TMW];
#pragma unroll
    for (int i = 0; i < TMW; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[i][0][r] = 0.f; acc[i][1][r] = 0.f; accb[i][r] = 0.f; }
    // wave-uniform.  PH: the (dy, dx) = (0, 0) entry of each pixel class (taps 5, 6, 9, 10), first channel block
    const bool do_db = p.want_db && wn == 0 && (PH ? (dyt == 0 && dxt == 0 && ci0 == 0) : tn == 0);
    sp_bf16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.0f;

    // stage-relative fragment addresses of this wave's tiles (the 16-pixel step and the pixel half are immediates)
    unsigned aoff[TMW][2], boff[2][2];
#pragma unroll
    for (int i = 0; i < TMW; ++i)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) aoff[i][pl] = (unsigned)foff(wm * TMW + i, pl, 0);
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) boff[q][pl] = (unsigned)foff(wn * 2 + q, pl, 0) + WG_OP_BYTES;
    const unsigned smem_addr = (unsigned)(uintptr_t)(sp_lds_ptr)smem;

    struct Frag { sp_short4 a0[TMW][2], a1[TMW][2], b0[2][2], b1[2][2]; };
    auto reads = [&](auto S, unsigned sbase, Frag& f) {
        constexpr int KOFF = decltype(S)::value * 16 * 512;
#pragma unroll
        for (int i = 0; i < TMW; ++i)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                if (SP && pl == 1 && !do_db) continue;   // single pass: dY's lo plane feeds the bias gradient only
                f.a0[i][pl] = sp_read_tr<KOFF>(sbase + aoff[i][pl]);
                f.a1[i][pl] = sp_read_tr<KOFF + 4 * 512>(sbase + aoff[i][pl]);
            }
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                if (SP && pl == 1) continue;
                f.b0[q][pl] = sp_read_tr<KOFF>(sbase + boff[q][pl]);
                f.b1[q][pl] = sp_read_tr<KOFF + 4 * 512>(sbase + boff[q][pl]);
            }
    };
    // all LDS reads of this wave have returned; the fragment registers pass through the asm so no MFMA can move above it
    auto wait = [&](Frag& f) {
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(f.a0[0][0]), "+v"(f.a1[0][0]), "+v"(f.a0[0][1]), "+v"(f.a1[0][1]), "+v"(f.b0[0][0]), "+v"(f.b1[0][0]),
                       "+v"(f.b0[0][1]), "+v"(f.b1[0][1]), "+v"(f.b0[1][0]), "+v"(f.b1[1][0]), "+v"(f.b0[1][1]), "+v"(f.b1[1][1]));
    };
    auto mfmas = [&](const Frag& f) {
        sp_bf16x8 ah[TMW], al[TMW], bh[2], bl[2];
#pragma unroll
        for (int i = 0; i < TMW; ++i) { ah[i] = sp_join(f.a0[i][0], f.a1[i][0]); al[i] = sp_join(f.a0[i][1], f.a1[i][1]); }
#pragma unroll
        for (int q = 0; q < 2; ++q) { bh[q] = sp_join(f.b0[q][0], f.b1[q][0]); bl[q] = sp_join(f.b0[q][1], f.b1[q][1]); }
#pragma unroll
        for (int i = 0; i < TMW; ++i)
#pragma unroll
            for (int q = 0; q < 2; ++q) if constexpr (!SP) acc[i][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[q], acc[i][q], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TMW; ++i)
#pragma unroll
            for (int q = 0; q < 2; ++q) if constexpr (!SP) acc[i][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[q], acc[i][q], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TMW; ++i)
#pragma unroll
            for (int q = 0; q < 2; ++q) acc[i][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[q], acc[i][q], 0, 0, 0);
        if (do_db) {
#pragma unroll
            for (int i = 0; i < TMW; ++i) {
                accb[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], ones, accb[i], 0, 0, 0);
                accb[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], ones, accb[i], 0, 0, 0);
            }
        }
    };
    // one chunk: the second 16-pixel step's fragments are read while the first step's MFMAs run, and the next chunk's DMA
    // pieces are issued between the groups (next == nullptr: nothing left to fetch)
    auto chunk = [&](const char* stage, char* next) {
        const unsigned sbase = smem_addr + (unsigned)(stage - smem);
        Frag f0, f1;
        reads(std::integral_constant<int, 0>{}, sbase, f0);
        if (next) issue_j(next, 0);
        wait(f0);
        reads(std::integral_constant<int, 1>{}, sbase, f1);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(f0);
        if (next) {
#pragma unroll
            for (int j = 1; j < NDMA; ++j) issue_j(next, j);
            q_pix += 32;
        }
        __builtin_amdgcn_sched_barrier(0);
        wait(f1);
        mfmas(f1);
    };

    const int n = c_end - c_begin;
    if (n > 0) issue(smem);
    for (int c = 0; c < n; ++c) {
        sp_sync<0>();
        chunk(smem + (c & 1) * WG_STAGE_BYTES, c + 1 < n ? smem + ((c + 1) & 1) * WG_STAGE_BYTES : nullptr);
    }

    // ---- epilogue: lane holds column n = li of rows (r&3) + 8*(r>>2) + 4*h
    const int li = lane & 31;
    const int M = p.Cout, N = p.ntaps * p.Cin;
    float* out = p.out + ((p.ksplit > 1 || PH) ? (long long)zz * M * N : 0);
#pragma unroll
    for (int i = 0; i < TMW; ++i)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int nn = n0 + wn * 64 + q * 32 + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = co0 + (wm * TMW + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                out[(long long)m * N + nn] = acc[i][q][r];
            }
        }
    if (do_db && li == 0) {
        float* o = PH ? p.out + (long long)p.ksplit * M * N + ((long long)(cp * 2 + cq) * p.ksplit + zz) * M
                      : (p.ksplit > 1 ? p.out + (long long)p.ksplit * M * N + (long long)zz * M : p.db);
#pragma unroll
        for (int i = 0; i < TMW; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[co0 + (wm * TMW + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] = accb[i][r];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Round 3: weight gradient with the three VERTICAL taps of a column shift in one workgroup (W in {16, 32}).
// dW[co][(ky, kx)][ci] = sum_p dY[p][co] * X[p + (ky-1) W + (kx-1)][ci]: for a fixed kx the three ky taps contract the SAME dY rows
// with X rows W pixels apart, and consecutive 32-pixel chunks slide that window by 32: every X pixel is DMA'd ONCE into a ring of
// eight 16-pixel units and read by the three taps from three chunks; the dY fragments are read once for three taps.  Tile = 128 co x
// (3 taps x 128 ci), 8 waves (2 x 4) of 64 co x (3 taps x 32 ci), 96 accumulator registers; L2 -> LDS bytes per MFMA a third of
// conv_ps_wgrad_kernel's.  (Round 4, late: the wave tile was 32 co x (3 x 64 ci) -- 4 dY + 3 x 8 X fragment reads per 18 MFMAs; the dY fragments are
// the ones shared by the three taps, so the taller tile reads 8 + 3 x 4 = 20 instead of 28: stand-alone within 1 %, CIFAR step -0.11 ... -0.19 ms on
// two boxes -- the kernel shares the chip with the data-gradient chain, and what it does not read from LDS it does not draw from the power budget.)
// A tap whose X row falls outside the image is skipped for that 16-pixel step (a step never straddles image rows: W % 16 == 0), so no
// zero rows are needed for the vertical direction; columns shifted out of the image read the zero page as before.
// LDS: two dY stages (2 x 16 KB) + the X ring (64 KB) = 96 KB, one workgroup per CU.
constexpr int WG3_RING_UNITS = 8, WG3_UNIT_BYTES = 16 * 512;
constexpr int WG3_LDS_BYTES = 2 * WG_OP_BYTES + WG3_RING_UNITS * WG3_UNIT_BYTES;

template <bool SP>
__global__ __launch_bounds__(512, 2) void conv_ps_wgrad3_kernel(PsWgParams p) {
    __shared__ __attribute__((aligned(128))) char smem[WG3_LDS_BYTES];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;       // wave tile = 64 co (two 32-row blocks) x 3 taps x 32 ci: 20 fragment reads per 18 MFMAs (32 x 64: 28)
    int tm, tn, zz;
    {
        const unsigned j = xcd_tile_order();
        const unsigned ntiles = p.tiles_m * p.tiles_n;
        zz = j / ntiles;
        const unsigned tile = j - zz * ntiles;
        tm = tile / p.tiles_n;
        tn = tile - tm * p.tiles_n;
    }
    const int co0 = tm * WG_BM;
    const int ncb = p.Cin / WG_BN;                 // 128-channel blocks of X
    const int kx = tn / ncb, ci0 = (tn - kx * ncb) * WG_BN;
    const int dxt = kx - 1;
    const int nchunks = p.P >> 5;                  // host: P % 32 == 0
    const int c_begin = zz * p.cps;
    int c_end = c_begin + p.cps;
    if (c_end > nchunks) c_end = nchunks;

    // ---- DMA: wave w moves pixel pairs w and w + 8 of a 32-pixel chunk; lane: pixel k = 2*pair + lane/32, 16-byte slot lane%32
    const int ps = lane & 31;
    int kpix[2];
    const char* abase_g[2]; const char* bbase_g[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int k = 2 * (wave + 8 * j) + (lane >> 5);
        kpix[j] = k;
        const int ls = ps ^ ((k & 3) << 2);
        abase_g[j] = p.dy + co0 * 4 + ls * 16;
        bbase_g[j] = p.x + ci0 * 4 + ls * 16;
    }
    char* const ring = smem + 2 * WG_OP_BYTES;
    auto issue_dy = [&](int c) {
        char* stage = smem + (c & 1) * WG_OP_BYTES;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long long pp = ps_v2r(c * 32 + kpix[j], p.lw, p.lh, p.lvw);       // chunk c = 32 VIRTUAL pixels (one strip row when W > 32)
            sp_dma16(abase_g[j] + pp * p.lddy * 4, stage + (wave + 8 * j) * 1024);
        }
    };
    const int VW = 1 << p.lvw;
    // X pixels [32 v + VW, 32 v + 32 + VW) (virtual order) of chunk v (v < c_begin: the halo): the rows the LAST vertical tap of chunk v needs
    auto issue_x = [&](int v) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int s0 = v * 32 + VW + 2 * (wave + 8 * j);             // first (virtual) pixel of the pair (wave-uniform)
            const int s = s0 + (lane >> 5);
            const int sr = ps_v2r(s, p.lw, p.lh, p.lvw);                 // its place in memory
            const int x = sr & (p.W - 1);
            const bool ok = s >= 0 && s < p.P && (unsigned)(x + dxt) < (unsigned)p.W;
            const int unit = ((s0 + 4096) >> 4) & (WG3_RING_UNITS - 1);
            sp_dma16(ok ? bbase_g[j] + (long long)(sr + dxt) * p.ldx * 4 : reinterpret_cast<const char*>(bd_zero16),
                     ring + unit * WG3_UNIT_BYTES + (s0 & 15) * 512);
        }
    };

    // ---- fragment addresses (ds_read_b64_tr_b16): as in conv_ps_wgrad_kernel, relative to a 16-pixel unit
    const int sl = lane & 15, hb = (lane >> 4) & 1, h = lane >> 5;
    const int kq = sl >> 2, rq = sl & 3;
    const int lane_base = (8 * h + kq) * 512 + hb * 32 + rq * 8;
    int xw[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) xw[v] = (v ^ kq) << 6;
    auto foff = [&](int t, int plane) { return lane_base + xw[(t & 1) * 2 + plane] + (t >> 1) * 256; };
    unsigned aoff[2][2], boff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) aoff[i][pl] = (unsigned)foff(wm * 2 + i, pl);
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) boff[pl] = (unsigned)foff(wn, pl);
    const unsigned smem_addr = (unsigned)(uintptr_t)(sp_lds_ptr)smem;
    const unsigned ring_addr = smem_addr + 2 * WG_OP_BYTES;

    sp_floatx16 acc[3][2], accb[2];          // acc[tap][co block]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        accb[0][r] = 0.f; accb[1][r] = 0.f;
#pragma unroll
        for (int t = 0; t < 3; ++t) { acc[t][0][r] = 0.f; acc[t][1][r] = 0.f; }
    }
    const bool do_db = p.want_db && tn == 0 && wn == 0;   // wave-uniform
    sp_bf16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.0f;

    // one 16-pixel step of one tap: X fragments (one 32-channel tile x hi / lo x two pixel halves)
    struct BFrag { sp_short4 b0[2], b1[2]; };
    auto readB = [&](BFrag& f, unsigned xbase) {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            if (SP && pl == 1) continue;   // single pass: X's lo plane is never read
            f.b0[pl] = sp_read_tr<0>(xbase + boff[pl]);
            f.b1[pl] = sp_read_tr<4 * 512>(xbase + boff[pl]);
        }
    };
    auto waitB = [&](BFrag& f) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f.b0[0]), "+v"(f.b1[0]), "+v"(f.b0[1]), "+v"(f.b1[1])); };
    struct AFrag { sp_short4 a0[2][2], a1[2][2]; };      // [co block][plane]
    auto readA = [&](AFrag& f, unsigned dbase, int S) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                if (SP && pl == 1 && !do_db) continue;   // single pass: dY's lo plane feeds the bias gradient only
                f.a0[i][pl] = S ? sp_read_tr<16 * 512>(dbase + aoff[i][pl]) : sp_read_tr<0>(dbase + aoff[i][pl]);
                f.a1[i][pl] = S ? sp_read_tr<16 * 512 + 4 * 512>(dbase + aoff[i][pl]) : sp_read_tr<4 * 512>(dbase + aoff[i][pl]);
            }
    };
    auto waitA = [&](AFrag& f) {
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(f.a0[0][0]), "+v"(f.a1[0][0]), "+v"(f.a0[0][1]), "+v"(f.a1[0][1]), "+v"(f.a0[1][0]), "+v"(f.a1[1][0]), "+v"(f.a0[1][1]),
                       "+v"(f.a1[1][1]));
    };
    auto tap_mfmas = [&](sp_floatx16 (&a)[2], const sp_bf16x8 (&ah)[2], const sp_bf16x8 (&al)[2], const BFrag& f) {
        const sp_bf16x8 bh = sp_join(f.b0[0], f.b1[0]), bl = sp_join(f.b0[1], f.b1[1]);
#pragma unroll
        for (int i = 0; i < 2; ++i) if constexpr (!SP) a[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh, a[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) if constexpr (!SP) a[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl, a[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh, a[i], 0, 0, 0);
    };

    const int wu = VW >> 4;        // units per (virtual) image row
    // six (16-pixel step, tap) stages per chunk, statically scheduled: the fragments of stage i+1 are read while the MFMAs of stage i
    // run.  A tap whose X row is outside the image skips its MFMAs (wave-uniform); its reads hit a live ring slot and are dropped.
    auto compute = [&](int c) {
        const unsigned dbase = smem_addr + (unsigned)((c & 1) * WG_OP_BYTES);
        const int p0 = c * 32;
        const int u0 = (p0 + 4096) >> 4;
        unsigned xb[6]; bool ok[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int S = i / 3, ky = i - 3 * S;
            const int y = ((p0 + 16 * S) >> p.lvw) & (p.H - 1);
            ok[i] = (unsigned)(y + ky - 1) < (unsigned)p.H;
            xb[i] = ring_addr + (unsigned)(((u0 + S + (ky - 1) * wu) & (WG3_RING_UNITS - 1)) * WG3_UNIT_BYTES);
        }
        AFrag fa[2]; BFrag fb[2];
        readA(fa[0], dbase, 0);
        readB(fb[0], xb[0]);
        waitA(fa[0]);
        waitB(fb[0]);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int S = i / 3, ky = i - 3 * S;
            if (i + 1 < 6) readB(fb[(i + 1) & 1], xb[i + 1]);
            if (i == 1) readA(fa[1], dbase, 1);
            __builtin_amdgcn_sched_barrier(0);
            const sp_bf16x8 ah[2] = {sp_join(fa[S].a0[0][0], fa[S].a1[0][0]), sp_join(fa[S].a0[1][0], fa[S].a1[1][0])};
            const sp_bf16x8 al[2] = {sp_join(fa[S].a0[0][1], fa[S].a1[0][1]), sp_join(fa[S].a0[1][1], fa[S].a1[1][1])};
            if (ok[i]) tap_mfmas(acc[ky], ah, al, fb[i & 1]);
            if (do_db && ky == 0) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    accb[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[j], ones, accb[j], 0, 0, 0);
                    accb[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[j], ones, accb[j], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (i + 1 < 6) {
                if (i == 1) waitA(fa[1]);
                waitB(fb[(i + 1) & 1]);
            }
        }
    };

    if (c_begin < c_end) {
        for (int v = c_begin - (VW >> 4); v < c_begin; ++v) issue_x(v);      // halo: X rows [32 c_begin - VW, 32 c_begin + VW)
        issue_dy(c_begin); issue_x(c_begin);
        for (int c = c_begin; c < c_end; ++c) {
            sp_sync<0>();
            if (c + 1 < c_end) { issue_dy(c + 1); issue_x(c + 1); }
            compute(c);
        }
    }

    // ---- epilogue: lane holds column n = li of rows (r&3) + 8*(r>>2) + 4*h; three tap tiles per wave
    const int li = lane & 31;
    const int M = p.Cout, N = 9 * p.Cin;
    float* out = p.out + (p.ksplit > 1 ? (long long)zz * M * N : 0);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int nn = (ky * 3 + kx) * p.Cin + ci0 + wn * 32 + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = co0 + (wm * 2 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                out[(long long)m * N + nn] = acc[ky][i][r];
            }
        }
    if (do_db && li == 0) {
        float* o = p.ksplit > 1 ? p.out + (long long)p.ksplit * M * N + (long long)zz * M : p.db;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[co0 + (wm * 2 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] = accb[i][r];
    }
}

// fixed-order sum of the K-split slabs (float4 per thread); the tail threads fold the bias rows.  V3 only names the launch (the second pass of
// conv_ps_wgrad3_kernel is its own row in the profiles / PMC tables: bench.py's roofline.traffic of the dominant kernel counts ITS second pass).
template <bool V3>
__global__ __launch_bounds__(256) void conv_ps_wgrad_reduce(const float* __restrict__ part, int ksplit, long long mn, int M,
                                                            float* __restrict__ dw, float* __restrict__ db, int brows) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n4 = mn >> 2;
    if (i < n4) {
        float4 a = *reinterpret_cast<const float4*>(part + 4 * i);
#pragma unroll 4      // four slab loads in flight; the additions keep their fixed order
        for (int s = 1; s < ksplit; ++s) {
            const float4 b = *reinterpret_cast<const float4*>(part + (long long)s * mn + 4 * i);
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        *reinterpret_cast<float4*>(dw + 4 * i) = a;
    } else if (db && i - n4 < M) {
        const long long m = i - n4;
        float v = 0.f;
        for (int s = 0; s < brows; ++s) v += part[(long long)ksplit * mn + (long long)s * M + m];   // brows = ksplit (x 4 classes in the PHASE form)
        db[m] = v;
    }
}

// ---- producers of split planes -------------------------------------------------------------------------------------
// rows x C fp32 (row stride lds) -> split planes (row stride ldd elements = 4*ldd bytes); C % 32 == 0.  8 values per thread.
__global__ __launch_bounds__(256) void split_rows_kernel(const float* __restrict__ src, long long lds, long long rows, int C,
                                                          unsigned short* __restrict__ dst, long long ldd) {
    const int c8 = C >> 3;
    const long long total = rows * c8;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / c8;
        const int j = (int)(i - r * c8);   // 8-channel group
        const float4 a = *reinterpret_cast<const float4*>(src + r * lds + j * 8);
        const float4 b = *reinterpret_cast<const float4*>(src + r * lds + j * 8 + 4);
        unsigned short* o = dst + 2 * r * ldd + (j >> 2) * 64 + (j & 3) * 8;
        *reinterpret_cast<uint4*>(o) = make_uint4(bd_pack_hi(a.x, a.y), bd_pack_hi(a.z, a.w), bd_pack_hi(b.x, b.y), bd_pack_hi(b.z, b.w));
        *reinterpret_cast<uint4*>(o + 32) = make_uint4(bd_pack_lo(a.x, a.y), bd_pack_lo(a.z, a.w), bd_pack_lo(b.x, b.y), bd_pack_lo(b.z, b.w));
    }
}

// nearest-neighbour x2 upsampling folded into the split: src [B, H, W, C] fp32 -> split planes of [B, 2H, 2W, C]
// (Upsample2D, resnet.py:126-161: F.interpolate(scale_factor=2, mode="nearest") feeding a 3x3 conv)
__global__ __launch_bounds__(256) void split_rows_ups2_kernel(const float* __restrict__ src, long long lds, int B, int H, int W, int C,
                                                               unsigned short* __restrict__ dst, long long ldd) {
    const int c8 = C >> 3;
    const long long total = (long long)B * 4 * H * W * c8;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / c8;                      // output pixel (b, y, x) over the 2H x 2W grid
        const int j = (int)(i - r * c8);
        const int x = (int)(r % (2 * W));
        const long long t = r / (2 * W);
        const int y = (int)(t % (2 * H));
        const long long b = t / (2 * H);
        const long long rs = (b * H + (y >> 1)) * W + (x >> 1);
        const float4 a = *reinterpret_cast<const float4*>(src + rs * lds + j * 8);
        const float4 bb = *reinterpret_cast<const float4*>(src + rs * lds + j * 8 + 4);
        unsigned short* o = dst + 2 * r * ldd + (j >> 2) * 64 + (j & 3) * 8;
        *reinterpret_cast<uint4*>(o) = make_uint4(bd_pack_hi(a.x, a.y), bd_pack_hi(a.z, a.w), bd_pack_hi(bb.x, bb.y), bd_pack_hi(bb.z, bb.w));
        *reinterpret_cast<uint4*>(o + 32) = make_uint4(bd_pack_lo(a.x, a.y), bd_pack_lo(a.z, a.w), bd_pack_lo(bb.x, bb.y), bd_pack_lo(bb.z, bb.w));
    }
}

// conv weights W[co][tap][ci] fp32 -> split planes of the transpose Wt[ci][tap][co] (rows ci, K = (tap, co)); Cin, Cout % 32 == 0.
// One workgroup = one (tap, 32 co x 32 ci) block through LDS.
__global__ __launch_bounds__(256) void split_wT_kernel(const float* __restrict__ w, int Cin, int Cout, unsigned short* __restrict__ out) {
    __shared__ float t[32][33];
    const int cib = blockIdx.x, cob = blockIdx.y, tap = blockIdx.z;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 8 rows per pass
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int co = cob * 32 + ty + 8 * i;
        t[ty + 8 * i][tx] = w[((long long)co * 9 + tap) * Cin + cib * 32 + tx];
    }
    __syncthreads();
    // thread -> (ci row r = tid/8, 4 consecutive co = (tid%8)*4)
    const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
    const float v0 = t[c4][r], v1 = t[c4 + 1][r], v2 = t[c4 + 2][r], v3 = t[c4 + 3][r];
    unsigned short* o = out + 2 * (((long long)(cib * 32 + r) * 9 + tap) * Cout + cob * 32) + c4;
    *reinterpret_cast<uint2*>(o) = make_uint2(bd_pack_hi(v0, v1), bd_pack_hi(v2, v3));
    *reinterpret_cast<uint2*>(o + 32) = make_uint2(bd_pack_lo(v0, v1), bd_pack_lo(v2, v3));
}

// all 3x3 conv weights of a network in ONE launch: the table (by value in the kernel arguments) lists, per weight,
// its element offset in the flat fp32 buffer (== its offset in the transposed split copy), the channel counts and the
// first block of the 1-D grid that belongs to it
struct WtTable {
    int n;
    long long off[BD_WT_MAX];
    int cin[BD_WT_MAX], cout[BD_WT_MAX], blk0[BD_WT_MAX + 1];
};
__global__ __launch_bounds__(256) void split_wT_batched_kernel(const float* __restrict__ params, unsigned short* __restrict__ out, WtTable t) {
    __shared__ float tl[32][33];
    int e = 0;
    while (e + 1 < t.n && (int)blockIdx.x >= t.blk0[e + 1]) ++e;
    const int Cin = t.cin[e], Cout = t.cout[e];
    const float* w = params + t.off[e];
    unsigned short* o_base = out + 2 * t.off[e];
    int b = blockIdx.x - t.blk0[e];
    const int ncib = Cin / 32, ncob = Cout / 32;
    const int cib = b % ncib; b /= ncib;
    const int cob = b % ncob; const int tap = b / ncob;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int co = cob * 32 + ty + 8 * i;
        tl[ty + 8 * i][tx] = w[((long long)co * 9 + tap) * Cin + cib * 32 + tx];
    }
    __syncthreads();
    const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
    const float v0 = tl[c4][r], v1 = tl[c4 + 1][r], v2 = tl[c4 + 2][r], v3 = tl[c4 + 3][r];
    unsigned short* o = o_base + 2 * (((long long)(cib * 32 + r) * 9 + tap) * Cout + cob * 32) + c4;
    *reinterpret_cast<uint2*>(o) = make_uint2(bd_pack_hi(v0, v1), bd_pack_hi(v2, v3));
    *reinterpret_cast<uint2*>(o + 32) = make_uint2(bd_pack_lo(v0, v1), bd_pack_lo(v2, v3));
}

int split_wt_batched(const float* params, uint16_t* out, const long long* off, const int* cin, const int* cout, int n, hipStream_t st) {
    for (int i0 = 0; i0 < n; i0 += BD_WT_MAX) {
        WtTable t;
        t.n = n - i0 < BD_WT_MAX ? n - i0 : BD_WT_MAX;
        int blk = 0;
        for (int i = 0; i < t.n; ++i) {
            t.off[i] = off[i0 + i]; t.cin[i] = cin[i0 + i]; t.cout[i] = cout[i0 + i]; t.blk0[i] = blk;
            blk += 9 * (t.cin[i] / 32) * (t.cout[i] / 32);
        }
        t.blk0[t.n] = blk;
        hipLaunchKernelGGL(split_wT_batched_kernel, dim3((unsigned)blk), dim3(256), 0, st, params, out, t);
        BD_LAUNCH_CHECK("split_wT_batched");
    }
    return BD_OK;
}

// shapes the LDS-DMA convolution handles: power-of-two images, whole 32-channel blocks, 128-wide output tiles.
// Large layers (>= 96 tiles of 256 x 128) run the three-stage 256 x 128 kernel, one workgroup per CU and no K split;
// small ones (8x8 / 4x4 images at CIFAR batch sizes) the 128 x 128 split-K variant.
static bool ps_grid_ok(int B, int H, int W) { return B > 0 && ilog2_exact(H) >= 0 && ilog2_exact(W) >= 0; }
static bool ps_channels_ok(int K, int N) { return K > 0 && K % 32 == 0 && N > 0 && N % PS_BN == 0; }
bool conv3x3_ps_supported(int B, int H, int W, int K_channels, int N_channels) { return ps_grid_ok(B, H, W) && ps_channels_ok(K_channels, N_channels); }
// the VIRTUAL image width of the vertical-tap sharing kernels: images wider than 32 pixels are walked strip by strip (ps_v2r)
static int ps_vw(int W) { return W < 32 ? W : 32; }
static int ps_epi(const bd_conv3x3_ps_desc& d) { return (d.residual ? 1 : 0) | (d.rowbias ? 2 : 0) | (d.accumulate ? 4 : 0); }

// Everything bd_conv3x3_ps decides from a descriptor's numbers, decided once: the launcher, bd_conv3x3_ps_workspace_bytes,
// bd_conv3x3_ps_gn_splits and bd_conv3x3_ps_plan read it.  Pure host arithmetic.  `ok` false, nothing else set: a shape ps_check refuses.
struct PsPlan : bd_conv3x3_ps_plan_info { bool ok, large; long long M; };
static PsPlan ps_plan(const bd_conv3x3_ps_desc& d) {
    static const bool v3_off = getenv("BD_PS_V3") && atoi(getenv("BD_PS_V3")) == 0;
    // round 4: any W >= 16 -- images wider than 32 pixels are walked strip by strip (virtual pixel order, ps_v2r)
    static const int v3_maxw = getenv("BD_PS_V3_MAXW") ? atoi(getenv("BD_PS_V3_MAXW")) : (1 << 30);     // (A/B knob: 32 = round 3's gate)
    static const char* kName[2][2][2] = {{{"conv_ps128_dgrad", "conv_ps_dgrad"}, {"conv_ps128_fwd", "conv_ps_fwd"}},
                                         {{"conv_ps128_dgrad_bf16", "conv_ps_dgrad_bf16"}, {"conv_ps128_fwd_bf16", "conv_ps_fwd_bf16"}}};
    PsPlan p = {};
    if (!(p.ok = conv3x3_ps_supported(d.B, d.H, d.W, d.K, d.N))) return p;
    p.M = (long long)d.B * d.H * d.W;
    p.large = cdiv(p.M, PS_BM) * (d.N / PS_BN) >= 96;
    const int nchunks = 9 * (d.K / 32);
    p.tiles_m = (int)cdiv(p.M, p.large ? PS_BM : 128); p.tiles_n = d.N / PS_BN;
    p.ksplit = 1; p.chunks_per_split = nchunks; p.stages = PS_STAGES;
    p.prof_class = kName[d.mode == BD_MODE_BF16][d.direction > 0][p.large];
    if (p.large) {
        // vertical-tap sharing variant (conv_ps3_kernel): image rows of 16 or 32 pixels, whole images per tile row block, whole tiles only
        const bool v3 = !v3_off && d.W >= 16 && d.W <= v3_maxw && ((long long)d.H * ps_vw(d.W)) % PS_BM == 0 && p.M % PS_BM == 0;
        p.kernel = v3 ? BD_PS_256_SHARED_TAP : BD_PS_256;
        // Round 4: pixel splits of the GroupNorm partials a forward call can write from its epilogue (0: it cannot).  One split per 256-pixel tile.
        const int lc = d.gn_groups > 0 && d.N % d.gn_groups == 0 ? ilog2_exact(d.N / d.gn_groups) : -1;
        if (v3 && lc >= 2 && lc <= 5 && (d.H * d.W) % PS_BM == 0) p.gn_splits = d.H * d.W / PS_BM;
    } else {
        p.kernel = BD_PS_128;
        // one slot per CU (2 x CUs measured 0.1-0.2 ms/step slower: twice the slab traffic for the 4x4 / 8x8 layers), >= 4 chunks per split
        split_k(device_cus(), (long long)p.tiles_m * p.tiles_n, nchunks, 4, p.ksplit, p.chunks_per_split);
        // round 6: short K slices (the 4 x 4 level) take the four-stage form (three chunks in flight, one workgroup per CU).  9: the 4 x 4
        // level only, -0.05 ms per step; two stages everywhere or the 8 x 8 level too measured slower (profiles/r06_ab_ps128_deep.txt)
        constexpr int deep_maxcps = 9;
        p.stages = p.ksplit > 1 && p.chunks_per_split <= deep_maxcps ? 4 : 2;
        p.reduce = p.ksplit > 1;      // K-split slabs [ksplit][M][N]; conv_ps128_reduce folds them and applies the epilogue
        if (p.reduce) p.workspace_bytes = (size_t)p.ksplit * (size_t)p.M * d.N * sizeof(float);
    }
    p.grid = p.tiles_m * p.tiles_n * p.ksplit;
    return p;
}
size_t conv3x3_ps_workspace_bytes(const bd_conv3x3_ps_desc& d) { return ps_plan(d).workspace_bytes; }
int conv3x3_ps_gn_splits(int B, int H, int W, int K, int N, int groups) {
    bd_conv3x3_ps_desc d = {};
    d.B = B; d.H = H; d.W = W; d.K = K; d.N = N; d.direction = 1; d.gn_groups = groups;
    return ps_plan(d).gn_splits;
}

// Every host check of bd_conv3x3_ps, in the order the entry point has always reported them (the pointer checks sit between the checks of
// the numbers, so one list keeps the order).  `launch` false -- bd_conv3x3_ps_plan -- skips the null-pointer, base-alignment and workspace
// checks: the launcher's own.
static int ps_check(const bd_conv3x3_ps_desc& d, const PsPlan& pl, bool launch) {
    const auto al = [launch](const void* p, uintptr_t mask) { return !launch || ((uintptr_t)p & mask) == 0; };
    BD_CHECK(!launch || (d.x_split && d.w_split && d.y), BD_ERR_INVALID, "conv3x3_ps: null pointer");
    BD_CHECK(ps_grid_ok(d.B, d.H, d.W), BD_ERR_UNSUPPORTED, "conv3x3_ps: H, W must be powers of two");
    BD_CHECK(ps_channels_ok(d.K, d.N), BD_ERR_UNSUPPORTED, "conv3x3_ps: K channels %% 32 and N channels %% %d must be 0 (got %d, %d)", PS_BN, d.K, d.N);
    BD_CHECK(d.ldx % 32 == 0 && al(d.x_split, 127) && al(d.w_split, 127), BD_ERR_UNSUPPORTED,
             "conv3x3_ps: split planes need ld %% 32 == 0 and 128-byte aligned bases");
    BD_CHECK(d.direction == 1 || d.direction == -1, BD_ERR_INVALID, "conv3x3_ps: direction must be +1 or -1");
    BD_CHECK(sp_mode_valid(d.mode), BD_ERR_INVALID, "conv3x3_ps: unknown compute mode %d", d.mode);
    // a row of a buffer holds at least the channels the kernels read or write in it (the contract of bd_split_rows and the loss launchers)
    BD_CHECK(d.ldx >= d.K && d.ldy >= d.N, BD_ERR_INVALID, "conv3x3_ps: ldx=%lld < K=%d or ldy=%lld < N=%d", (long long)d.ldx, d.K,
             (long long)d.ldy, d.N);
    BD_CHECK(!d.residual || d.ldr >= d.N, BD_ERR_INVALID, "conv3x3_ps: ldr=%lld < N=%d", (long long)d.ldr, d.N);
    BD_CHECK(!d.rowbias || d.ld_rowbias >= d.N, BD_ERR_INVALID, "conv3x3_ps: ld_rowbias=%lld < N=%d", (long long)d.ld_rowbias, d.N);
    // the epilogues and the split-K second pass move float4: every fp32 operand needs 16-byte rows
    BD_CHECK(d.ldy % 4 == 0 && al(d.y, 15), BD_ERR_UNSUPPORTED, "conv3x3_ps: y needs ldy %% 4 == 0 and a 16-byte aligned base");
    BD_CHECK(!d.residual || (d.ldr % 4 == 0 && al(d.residual, 15)), BD_ERR_UNSUPPORTED,
             "conv3x3_ps: residual needs ldr %% 4 == 0 and a 16-byte aligned base");
    BD_CHECK(!d.rowbias || (d.ld_rowbias % 4 == 0 && al(d.rowbias, 15)), BD_ERR_UNSUPPORTED,
             "conv3x3_ps: rowbias needs ld_rowbias %% 4 == 0 and a 16-byte aligned base");
    BD_CHECK(!d.bias || al(d.bias, 15), BD_ERR_UNSUPPORTED, "conv3x3_ps: bias needs a 16-byte aligned base");
    BD_CHECK(pl.M < (1ll << 31), BD_ERR_UNSUPPORTED, "conv3x3_ps: pixel count overflows int32");
    BD_CHECK((long long)(d.W + 1) * d.ldx * 4 < (1ll << 31), BD_ERR_UNSUPPORTED, "conv3x3_ps: row pitch too large");
    const int epi = ps_epi(d);
    BD_CHECK(!d.gn_part || !pl.large || (d.direction == 1 && (epi == 1 || epi == 2) && pl.gn_splits > 0), BD_ERR_UNSUPPORTED,
             "conv3x3_ps: gn_part needs a forward call with exactly one of rowbias / residual and bd_conv3x3_ps_gn_splits() > 0");
    BD_CHECK(!d.gn_part || pl.large, BD_ERR_UNSUPPORTED, "conv3x3_ps: gn_part on a small layer (bd_conv3x3_ps_gn_splits() == 0)");
    BD_CHECK(!launch || !pl.reduce || (d.workspace && d.workspace_bytes >= pl.workspace_bytes), BD_ERR_WORKSPACE,
             "conv3x3_ps: split-K needs %zu workspace bytes, got %zu", pl.workspace_bytes, d.workspace_bytes);
    return BD_OK;
}

// run-time kernel choice and epilogue bits -> the instantiation: every epilogue combination has its own (the epilogue's addends are
// compile-time); the four-stage form of conv_ps128_kernel exists for EPI 0 only (it always runs split, the reduce applies the epilogue)
template <bool SP, int... EPI>
static void ps_launch(const PsPlan& pl, int epi, const PsSmallParams& pp, hipStream_t st) {
    static constexpr void (*general[])(PsParams) = {conv_ps_kernel<EPI, SP>...}, (*shared_tap[])(PsParams) = {conv_ps3_kernel<EPI, SP>...};
    static constexpr void (*small[])(PsSmallParams) = {conv_ps128_kernel<EPI, SP, 2>...}, (*small_deep)(PsSmallParams) = conv_ps128_kernel<0, SP, 4>;
    const dim3 grid((unsigned)pl.grid), block(PS_NT);
    if (pl.kernel == BD_PS_128) {
        const auto kernel = pl.stages == 4 ? small_deep : small[epi];
        hipLaunchKernelGGL(kernel, grid, block, 0, st, pp);
    } else {
        const auto kernel = pl.kernel == BD_PS_256_SHARED_TAP ? shared_tap[epi] : general[epi];
        hipLaunchKernelGGL(kernel, grid, block, 0, st, pp.q);
    }
}

int conv3x3_ps(const bd_conv3x3_ps_desc& d, hipStream_t st) {
    const PsPlan pl = ps_plan(d);
    BD_TRY(ps_check(d, pl, true));
    PsSmallParams pp = {};
    PsParams& p = pp.q;
    p.a = reinterpret_cast<const char*>(d.x_split); p.w = reinterpret_cast<const char*>(d.w_split);
    p.y = d.y; p.bias = d.bias; p.rowbias = d.rowbias; p.residual = d.residual;
    p.lda = d.ldx; p.ldy = d.ldy; p.ldr = d.ldr; p.ld_rowbias = d.ld_rowbias;
    p.C = d.K; p.H = d.H; p.W = d.W; p.lw = ilog2_exact(d.W); p.lhw = ilog2_exact(d.W) + ilog2_exact(d.H);
    p.sign = d.direction; p.M = (int)pl.M; p.N = d.N; p.tiles_m = pl.tiles_m; p.tiles_n = pl.tiles_n;
    p.out_scale = d.out_scale == 0.f ? 1.f : d.out_scale; p.accumulate = d.accumulate;
    if (pl.large) p.lvw = ilog2_exact(ps_vw(d.W));
    if (d.gn_part) { p.gn_part = d.gn_part; p.gn_G = d.gn_groups; p.gn_lcpg = ilog2_exact(d.N / d.gn_groups); }
    pp.ksplit = pl.ksplit; pp.cps = pl.chunks_per_split;
    if (pl.reduce) pp.partial = reinterpret_cast<float*>(d.workspace);
    const int rec = prof_on() ? prof_begin(pl.prof_class, 2.0 * (double)pl.M * d.N * 9.0 * d.K,
                                           ((double)pl.M * d.K + 9.0 * d.K * d.N + (double)pl.M * d.N) * 4.0, st) : -1;
    const int epi = pl.reduce ? 0 : ps_epi(d);
    if (d.mode == BD_MODE_BF16) ps_launch<true, 0, 1, 2, 3, 4, 5, 6, 7>(pl, epi, pp, st);   // single pass: hi*hi only
    else ps_launch<false, 0, 1, 2, 3, 4, 5, 6, 7>(pl, epi, pp, st);
    BD_LAUNCH_CHECK(pl.large ? "conv_ps" : "conv_ps128");
    if (pl.reduce) {
        hipLaunchKernelGGL(conv_ps128_reduce, dim3((unsigned)cdiv(pl.M * (d.N / 4), 256)), dim3(256), 0, st, pp);
        BD_LAUNCH_CHECK("conv_ps128_reduce");
    }
    prof_end(rec, st);
    return BD_OK;
}

// ---- the weight gradients: bd_conv3x3_ps_wgrad (nine taps) and its PHASE form bd_upsample_conv_wgrad (the 16 entries of E, conv_ph.hip) share
// one plan, one list of checks and one launcher.  The nine-tap descriptor is read through the fields it shares with the phase form's.
static bd_upsample_conv_desc ps_wgrad_desc(const bd_conv3x3_ps_wgrad_desc& d) {
    bd_upsample_conv_desc u = {};
    u.B = d.B; u.H = d.H; u.W = d.W; u.Cin = d.Cin; u.Cout = d.Cout; u.x_split = d.x_split; u.ldx = d.ldx; u.dy_split = d.dy_split; u.lddy = d.lddy;
    u.dw = d.dw; u.db = d.db; u.workspace = d.workspace; u.workspace_bytes = d.workspace_bytes; u.mode = d.mode;
    return u;
}
bool conv3x3_ps_wgrad_supported(int B, int H, int W, int Cin, int Cout) {
    return ps_grid_ok(B, H, W) && Cin > 0 && Cin % WG_BN == 0 && Cout > 0 && Cout % WG_BM == 0;
}
static int g_wg3_slots_override = 0;     // 0: environment / default (set by bd_tune_set)
// Everything the two entry points decide from a descriptor's numbers: kernel, tiles, K split and the layout of the slabs (Cout * ntaps * Cin
// gradient + bias_rows * Cout bias-gradient floats per split; behind them dE in the phase form).  The launcher, the two *_workspace_bytes and
// the two plan queries read it.  grid 0, nothing else set: a shape ps_wgrad_check refuses.
typedef bd_conv3x3_ps_wgrad_plan_info PsWgPlan;
static PsWgPlan ps_wgrad_plan(const bd_upsample_conv_desc& d, bool phase) {
    static const bool v3_off = getenv("BD_PS_WG3") && atoi(getenv("BD_PS_WG3")) == 0;
    static const int v3_maxw = getenv("BD_PS_WG3_MAXW") ? atoi(getenv("BD_PS_WG3_MAXW")) : (1 << 30);        // (A/B knob: 32 = round 3's gate)
    static const int slots3_getenv = getenv("BD_PS_WG3_SLOTS") ? atoi(getenv("BD_PS_WG3_SLOTS")) : 0;
    static const char* kName[3][2] = {{"conv_ps_wgrad", "conv_ps_wgrad_bf16"}, {"conv_ps_wgrad3", "conv_ps_wgrad3_bf16"},      // (round 6: the large layers' kernel is its own class)
                                      {"conv_ph_ups_wgrad", "conv_ph_ups_wgrad_bf16"}};
    PsWgPlan p = {};
    if (!conv3x3_ps_wgrad_supported(d.B, d.H, d.W, d.Cin, d.Cout)) return p;
    const long long P = (long long)d.B * d.H * d.W;
    // vertical-tap sharing form (conv_ps_wgrad3_kernel): image rows of 16 or 32 pixels, whole 32-pixel chunks
    // round 4: any W >= 16 -- wider images are walked strip by strip (virtual pixel order, ps_v2r): a chunk = one 32-pixel strip row
    const bool v3 = !phase && !v3_off && d.W >= 16 && d.W <= v3_maxw && P % 32 == 0;
    p.kernel = phase ? BD_PS_WGRAD_PHASE : v3 ? BD_PS_WGRAD_SHARED_TAP : BD_PS_WGRAD;
    p.ntaps = phase ? 16 : 9; p.bias_rows = phase ? 4 : 1;      // (phase form: one bias row per pixel class of the fine grid)
    p.tiles_m = d.Cout / WG_BM; p.tiles_n = (v3 ? 3 : p.ntaps) * d.Cin / WG_BN;
    const int slots = 2 * device_cus();   // two 64-KB workgroups per CU (two LDS stages each): the pair de-phases, 141 vs 189 us
    // 96 KB of LDS: one workgroup per CU -- and three quarters of the CUs (round 4, late: 192 of 256).  The kernel never runs alone: the data-gradient
    // chain shares the chip with it, so the CUs it leaves are not idle, and a quarter fewer slabs are a quarter less slab traffic: CIFAR step
    // 17.71 -> 17.53 ms and 18.01 -> 17.89 on two boxes (160 / 176 / 208 / 224 / 256 slots: 17.70 / 17.59 / 17.67 / 17.72 / 17.71), 256 x 256 28.06 -> 27.93.
    // Images walked strip by strip (W > 32: the 256 x 256 network at B = 4, whose main stream carries the three-pass GroupNorm and 2 048-tile data
    // gradients): HALF the CUs -- 27.14 -> 26.69 ms per step (144 / 160 / 176 slots: 27.52 / 27.51 / 27.74; 112 / 96 / 64: 27.21 / 28.16 / 32.9), while the
    // CIFAR step wants its 192 (128: 18.08 against 17.89).
    const int slots3_env = g_wg3_slots_override > 0 ? g_wg3_slots_override : slots3_getenv;      // bd_tune_set("ps_wg3_slots", n) wins over the environment
    p.slots = !v3 ? slots : slots3_env > 0 ? slots3_env : (d.W > 32 ? slots / 4 : slots * 3 / 8);
    // chunks per split at least 8 (4x4 layers: 8 slabs instead of 14; 4 / 16 measured +0.2 / +0.1 ms)
    split_k(p.slots, (long long)p.tiles_m * p.tiles_n, (int)cdiv(P, 32), 8, p.ksplit, p.chunks_per_split);
    p.reduce = phase || p.ksplit > 1;
    p.grid = p.tiles_m * p.tiles_n * p.ksplit;
    const size_t mn = (size_t)d.Cout * p.ntaps * d.Cin;
    p.slab_floats = mn + (size_t)p.bias_rows * d.Cout;
    if (p.reduce) p.workspace_bytes = (size_t)p.ksplit * p.slab_floats * sizeof(float);
    if (phase) { p.de_offset = p.workspace_bytes; p.workspace_bytes += mn * sizeof(float); }       // K-split slabs + dE
    p.prof_class = kName[p.kernel][d.mode == BD_MODE_BF16];
    return p;
}
size_t conv3x3_ps_wgrad_workspace_bytes(const bd_conv3x3_ps_wgrad_desc& d) { return ps_wgrad_plan(ps_wgrad_desc(d), false).workspace_bytes; }
size_t upsample_conv_wgrad_workspace_bytes(const bd_upsample_conv_desc& d) { return ps_wgrad_plan(d, true).workspace_bytes; }

// The checks of the weight-gradient entry point `who`, in the order it has always reported them, and -- `p` given: the launcher -- the kernel
// arguments.  Without `p` (the plan queries) the null-pointer, base-alignment and workspace checks, the launcher's own, are skipped.
static int ps_wgrad_check(const char* who, const bd_upsample_conv_desc& d, bool phase, const PsWgPlan& pl, PsWgParams* p) {
    BD_CHECK(!p || (d.x_split && d.dy_split && d.dw), BD_ERR_INVALID, "%s: null pointer", who);
    BD_CHECK(pl.grid > 0, BD_ERR_UNSUPPORTED, "%s: needs power-of-two H, W, Cin and Cout multiples of 128", who);
    BD_CHECK(d.ldx % 32 == 0 && d.lddy % 32 == 0 && (!p || (((uintptr_t)d.x_split | (uintptr_t)d.dy_split) & 127) == 0), BD_ERR_UNSUPPORTED,
             "%s: split planes need ld %% 32 == 0 and 128-byte aligned bases", who);
    BD_CHECK(!phase || (long long)d.B * d.H * d.W * 4 < (1ll << 31), BD_ERR_UNSUPPORTED, "%s: pixel count overflows int32", who);
    BD_CHECK(sp_mode_valid(d.mode), BD_ERR_INVALID, "%s: unknown compute mode %d", who, d.mode);
    BD_CHECK(phase || (d.ldx >= d.Cin && d.lddy >= d.Cout), BD_ERR_INVALID, "%s: ldx=%lld < Cin=%d or lddy=%lld < Cout=%d", who, (long long)d.ldx,
             d.Cin, (long long)d.lddy, d.Cout);
    if (!p) return BD_OK;
    BD_CHECK(!pl.reduce || (d.workspace && d.workspace_bytes >= pl.workspace_bytes), BD_ERR_WORKSPACE, "%s: workspace %zu < %zu", who,
             d.workspace_bytes, pl.workspace_bytes);
    p->dy = reinterpret_cast<const char*>(d.dy_split); p->x = reinterpret_cast<const char*>(d.x_split);
    p->lddy = d.lddy; p->ldx = d.ldx; p->Cin = d.Cin; p->Cout = d.Cout; p->H = d.H; p->W = d.W; p->lw = ilog2_exact(d.W);
    if (!phase) { p->lh = ilog2_exact(d.H); p->lvw = ilog2_exact(ps_vw(d.W)); }
    p->P = d.B * d.H * d.W;
    p->tiles_m = pl.tiles_m; p->tiles_n = pl.tiles_n; p->ntaps = pl.ntaps; p->ksplit = pl.ksplit; p->cps = pl.chunks_per_split;
    p->want_db = d.db != nullptr;
    if (pl.reduce) p->out = reinterpret_cast<float*>(d.workspace);      // slabs; the second pass writes dw (phase form: dE) and db
    else { p->out = d.dw; p->db = d.db; }
    return BD_OK;
}

static int ps_wgrad_launch(const char* who, const bd_upsample_conv_desc& d, bool phase, hipStream_t st) {
    static constexpr void (*kernels[3][2])(PsWgParams) = {{conv_ps_wgrad_kernel<2, 8, false>, conv_ps_wgrad_kernel<2, 8, true>},
                                                          {conv_ps_wgrad3_kernel<false>, conv_ps_wgrad3_kernel<true>},
                                                          {conv_ps_wgrad_kernel<2, 8, false, true>, conv_ps_wgrad_kernel<2, 8, true, true>}};
    const PsWgPlan pl = ps_wgrad_plan(d, phase);
    PsWgParams p = {};
    BD_TRY(ps_wgrad_check(who, d, phase, pl, &p));
    const double fine = phase ? 4.0 : 1.0;       // phase form: dY lives on the fine grid, four pixels per source pixel
    const int rec = prof_on() ? prof_begin(pl.prof_class, 2.0 * (double)p.P * fine * d.Cout * 9.0 * d.Cin,
                                           ((double)p.P * (d.Cin + fine * d.Cout) + 9.0 * d.Cin * d.Cout) * 4.0, st) : -1;
    hipLaunchKernelGGL(kernels[pl.kernel][d.mode == BD_MODE_BF16], dim3((unsigned)pl.grid), dim3(512), 0, st, p);
    BD_LAUNCH_CHECK(phase ? "conv_ps_wgrad (phase)" : "conv_ps_wgrad");
    if (pl.reduce) {
        const long long mn = (long long)d.Cout * pl.ntaps * d.Cin, total = mn / 4 + (d.db ? d.Cout : 0);
        float* dst = phase ? reinterpret_cast<float*>(static_cast<char*>(d.workspace) + pl.de_offset) : d.dw;
        const auto reduce = pl.kernel == BD_PS_WGRAD_SHARED_TAP ? conv_ps_wgrad_reduce<true> : conv_ps_wgrad_reduce<false>;
        hipLaunchKernelGGL(reduce, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, p.out, p.ksplit, mn, d.Cout, dst, d.db, pl.bias_rows * p.ksplit);
        BD_LAUNCH_CHECK(phase ? "conv_ps_wgrad_reduce (phase)" : "conv_ps_wgrad_reduce");
        if (phase) BD_TRY(ups_dweff_combine(dst, d.Cin, d.Cout, d.dw, st));      // dE -> dw [Cout,3,3,Cin]
    }
    prof_end(rec, st);
    return BD_OK;
}
int conv3x3_ps_wgrad(const bd_conv3x3_ps_wgrad_desc& d, hipStream_t st) { return ps_wgrad_launch("conv3x3_ps_wgrad", ps_wgrad_desc(d), false, st); }
// dw [Cout,3,3,Cin] (+ db) of y = conv3x3(nearest_up2(x)) from x (split planes, SOURCE grid) and dY (split planes, fine grid)
int upsample_conv_wgrad(const bd_upsample_conv_desc& d, hipStream_t st) { return ps_wgrad_launch("bd_upsample_conv_wgrad", d, true, st); }

int g_tune_gen = 0;
int tune_set(const char* key, int value) {
    BD_CHECK(key, BD_ERR_INVALID, "bd_tune_set: null key");
    if (!strcmp(key, "ps_wg3_slots")) { g_wg3_slots_override = value > 0 ? value : 0; ++g_tune_gen; return BD_OK; }
    set_error("bd_tune_set: unknown key '%s' (known: ps_wg3_slots)", key);
    return BD_ERR_INVALID;
}
}  // namespace bd

extern "C" int bd_tune_set(const char* key, int value) { return bd::tune_set(key, value); }
extern "C" size_t bd_upsample_conv_wgrad_workspace_bytes(const bd_upsample_conv_desc* d) {
    return d ? bd::upsample_conv_wgrad_workspace_bytes(*d) : 0;
}
extern "C" int bd_upsample_conv_wgrad(const bd_upsample_conv_desc* d, bd_stream_t s) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_upsample_conv_wgrad: null descriptor");
    return bd::upsample_conv_wgrad(*d, bd::S(s));
}
extern "C" size_t bd_conv3x3_ps_workspace_bytes(const bd_conv3x3_ps_desc* d) { return d ? bd::conv3x3_ps_workspace_bytes(*d) : 0; }
extern "C" int bd_conv3x3_ps_gn_splits(int B, int H, int W, int K, int N, int groups) { return bd::conv3x3_ps_gn_splits(B, H, W, K, N, groups); }
extern "C" int bd_conv3x3_ps(const bd_conv3x3_ps_desc* d, bd_stream_t s) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_conv3x3_ps: null descriptor");
    return bd::conv3x3_ps(*d, bd::S(s));
}
extern "C" int bd_conv3x3_ps_plan(const bd_conv3x3_ps_desc* d, bd_conv3x3_ps_plan_info* out) {
    BD_CHECK(d != nullptr && out != nullptr, BD_ERR_INVALID, "bd_conv3x3_ps_plan: null descriptor or output");
    const bd::PsPlan p = bd::ps_plan(*d);
    BD_TRY(bd::ps_check(*d, p, false));
    *out = p;
    return BD_OK;
}
extern "C" int bd_conv3x3_ps_wgrad(const bd_conv3x3_ps_wgrad_desc* d, bd_stream_t s) {
    BD_CHECK(d, BD_ERR_INVALID, "bd_conv3x3_ps_wgrad: null descriptor");
    return bd::conv3x3_ps_wgrad(*d, bd::S(s));
}
extern "C" size_t bd_conv3x3_ps_wgrad_workspace_bytes(const bd_conv3x3_ps_wgrad_desc* d) {
    return d ? bd::conv3x3_ps_wgrad_workspace_bytes(*d) : 0;
}
static int ps_wgrad_plan_query(const char* who, const bd_upsample_conv_desc& d, bool phase, bd_conv3x3_ps_wgrad_plan_info* out) {
    *out = bd::ps_wgrad_plan(d, phase);
    return bd::ps_wgrad_check(who, d, phase, *out, nullptr);
}
extern "C" int bd_conv3x3_ps_wgrad_plan(const bd_conv3x3_ps_wgrad_desc* d, bd_conv3x3_ps_wgrad_plan_info* out) {
    BD_CHECK(d != nullptr && out != nullptr, BD_ERR_INVALID, "bd_conv3x3_ps_wgrad_plan: null descriptor or output");
    return ps_wgrad_plan_query("conv3x3_ps_wgrad", bd::ps_wgrad_desc(*d), false, out);
}
extern "C" int bd_upsample_conv_wgrad_plan(const bd_upsample_conv_desc* d, bd_conv3x3_ps_wgrad_plan_info* out) {
    BD_CHECK(d != nullptr && out != nullptr, BD_ERR_INVALID, "bd_upsample_conv_wgrad_plan: null descriptor or output");
    return ps_wgrad_plan_query("bd_upsample_conv_wgrad", *d, true, out);
}
extern "C" int bd_split_rows(const float* src, int64_t ld_src, int64_t rows, int C, uint16_t* dst, int64_t ld_dst, bd_stream_t stream) {
    BD_CHECK(src && dst && rows > 0 && C > 0, BD_ERR_INVALID, "bd_split_rows: bad args");
    BD_CHECK(ld_src >= C && ld_dst >= C, BD_ERR_INVALID, "bd_split_rows: ld_src=%lld / ld_dst=%lld < C=%d", (long long)ld_src, (long long)ld_dst, C);
    BD_CHECK(C % 32 == 0 && ld_dst % 32 == 0 && (ld_src & 3) == 0 && bd::aligned16(src) && ((uintptr_t)dst & 127) == 0, BD_ERR_UNSUPPORTED,
             "bd_split_rows: C, ld_dst %% 32, ld_src %% 4, 16-byte aligned src and 128-byte aligned dst required");
    long long nb = bd::cdiv(rows * (C / 8), 256);
    if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(bd::split_rows_kernel, dim3((unsigned)nb), dim3(256), 0, bd::S(stream), src, (long long)ld_src, (long long)rows, C, dst,
                       (long long)ld_dst);
    BD_LAUNCH_CHECK("split_rows");
    return BD_OK;
}
extern "C" int bd_split_rows_ups2(const float* src, int64_t ld_src, int B, int H, int W, int C, uint16_t* dst, int64_t ld_dst, bd_stream_t stream) {
    BD_CHECK(src && dst && B > 0 && H > 0 && W > 0 && C > 0, BD_ERR_INVALID, "bd_split_rows_ups2: bad args");
    BD_CHECK(ld_src >= C && ld_dst >= C, BD_ERR_INVALID, "bd_split_rows_ups2: ld_src=%lld / ld_dst=%lld < C=%d", (long long)ld_src, (long long)ld_dst,
             C);
    BD_CHECK(C % 32 == 0 && ld_dst % 32 == 0 && (ld_src & 3) == 0 && bd::aligned16(src) && ((uintptr_t)dst & 127) == 0, BD_ERR_UNSUPPORTED,
             "bd_split_rows_ups2: C, ld_dst %% 32, ld_src %% 4, 16-byte aligned src and 128-byte aligned dst required");
    long long nb = bd::cdiv((long long)B * 4 * H * W * (C / 8), 256);
    if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(bd::split_rows_ups2_kernel, dim3((unsigned)nb), dim3(256), 0, bd::S(stream), src, (long long)ld_src, B, H, W, C, dst,
                       (long long)ld_dst);
    BD_LAUNCH_CHECK("split_rows_ups2");
    return BD_OK;
}
extern "C" int bd_split_wt(const float* w, int Cin, int Cout, uint16_t* out, bd_stream_t stream) {
    BD_CHECK(w && out && Cin > 0 && Cout > 0, BD_ERR_INVALID, "bd_split_wt: bad args");
    BD_CHECK(Cin % 32 == 0 && Cout % 32 == 0 && ((uintptr_t)out & 127) == 0, BD_ERR_UNSUPPORTED, "bd_split_wt: Cin, Cout %% 32 and 128-byte aligned out required");
    hipLaunchKernelGGL(bd::split_wT_kernel, dim3(Cin / 32, Cout / 32, 9), dim3(256), 0, bd::S(stream), w, Cin, Cout, out);
    BD_LAUNCH_CHECK("split_wT");
    return BD_OK;
}
