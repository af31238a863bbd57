// UNet2DModel as a static execution plan (host-only object; all device memory is the caller's).
//
// Mirrors the topology built by /root/reference/diffusers/src/diffusers/models/unet_2d.py:82-217 and the
// forward of :229-326, with ResnetBlock2D (resnet.py:551-601), AttentionBlock (attention.py:121-174),
// Downsample2D (resnet.py:199-208), Upsample2D (resnet.py:126-161) and the skip bookkeeping of
// unet_2d_blocks.py (DownBlock2D, AttnDownBlock2D, UNetMidBlock2D, UpBlock2D, AttnUpBlock2D).
//
// MI355X-first choices:
//  * activations NHWC with a leading dimension: every skip tensor is BORN inside the concat buffer of the
//    up-block resnet that will consume it, so torch.cat (13 copies/forward in the reference) disappears;
//  * parameters / gradients are ONE flat fp32 buffer each (time-embedding projections of all resnets are
//    contiguous => one GEMM; Adam + clip are single launches; DP all-reduce buckets are plain ranges);
//  * every parameter receives exactly one gradient contribution => grads are written, never accumulated;
//  * forward and backward are fixed launch sequences on one stream: hipGraph-capturable, no host sync.
//
// Layout of this file: node builders (node_*) name parameters, buffers and the order of launches; what follows from a kernel-path choice
// (descriptor type, operand format, weight copy, workspace, stream, dry-run accounting) lives in the run-time helpers of struct bd_unet
// and is written once: conv3_fwd / conv3_dgrad / conv3_wgrad (+ conv3_dgrad_input, conv3_gn_splits) and the phase-decomposed phase_ups_fwd /
// phase_ups_wgrad / phase_ups_dgrad / phase_s2_dgrad over a Conv3 record; lin_fwd / lin_dgrad / lin_wgrad over a Lin record, temb_wgrad for the
// batched time_emb_proj rows; attn_fwd / attn_bwd over an Attn record (head_gemm: the per-head products of the fp32 family); gn_fwd / gn_bwd,
// grad_planes, silu_fwd / silu_bwd, add, colsum, split_rows, split_rows_ups2, sum2x2, timestep_embedding; need, take_ginit.  A node states each
// path choice ONCE as a Path -- a function of the batch the workspace is laid out for -- and its buffers' `live`, reg_gsplit's `want` and both
// closures ask that one function through takes(c, path).
#include "common.h"

#include <functional>
#include <string>
#include <vector>
#include <cmath>
#include <cstdlib>

namespace bd {

// the A/B knobs of this file, read once per process
struct Knobs {
    bool gsplit, conv_ps, shortcut_sp;      // BD_GSPLIT, BD_CONV_PS, BD_SHORTCUT_SP: on unless set to 0
    long long fwd_pipes_minpx;              // BD_FWD_PIPES_MINPX: input pixels per batch from which the forward runs as two pipelines
    static long long env(const char* name, long long dflt) { const char* v = getenv(name); return v ? atoll(v) : dflt; }
    static const Knobs& get() {
        static const Knobs k = {env("BD_GSPLIT", 1) != 0, env("BD_CONV_PS", 1) != 0, env("BD_SHORTCUT_SP", 1) != 0, env("BD_FWD_PIPES_MINPX", 32768)};
        return k;
    }
};

struct View {
    int buf = -1;   // value buffer id
    int coff = 0;   // channel offset inside the buffer
    int C = 0, ld = 0, H = 0, W = 0;
};

enum Region { R_VALUE = 0, R_GRAD = 1, R_SCRATCH = 2 };
struct Buf {
    int64_t per_sample = 0, fixed = 0;
    int region = R_VALUE, group = 0;
    int64_t off = 0;  // floats, filled by layout()
    int gbuf = -1;    // grad buffer of a value buffer
    // optional: decided per (batch, training) at layout time -- a buffer only one of several kernel paths uses takes no room
    // when the plan selects another path for that batch (b_xuS vs b_xS / E / E^T of the upsample convolutions)
    std::function<bool(int, int)> live;
};

struct Param {
    std::string name;
    int64_t off;
    int rank;
    int64_t shape[4];
    int layout;
};

struct Ctx {
    bool dry = false;
    bool training = true;   // forward only: keep what backward needs
    int B = 0;
    int64_t s0 = 0;   // sample offset of this context inside the batch the workspace is laid out for
    int LB = 0;       // that batch (B of the call); B <= LB is the number of samples this context processes
    float* ws = nullptr;
    const float* params = nullptr;
    float* grads = nullptr;
    hipStream_t st = nullptr;
    const float* x = nullptr; int64_t ldx = 0;
    const int64_t* t = nullptr; int t_stride = 0;
    const float* tf = nullptr;   // fractional timesteps (bd_unet_forward_tf): exactly one of t / tf is set
    float* out = nullptr; int64_t ldo = 0;
    const float* dout = nullptr; int64_t lddo = 0;
    // backward only.  wg = false: the data-gradient-only schedule (bd_unet_backward_input with grads == NULL) -- every launch that produces
    // a parameter gradient is skipped by the helper it goes through, nothing is forked to the side stream.  dx: where conv_in's backward
    // leaves the gradient of the network input (null: not wanted)
    bool wg = true;
    float* dx = nullptr; int64_t lddx = 0;
    char* opws = nullptr; size_t opws_bytes = 0; size_t opws_need = 0;
    // weight-gradient side stream (backward only): wgrad GEMMs feed nothing but the optimizer, so they run on a second
    // stream next to the dgrad / GroupNorm chain that the rest of backward waits for.  Forked per launch; the scratch
    // arena alternates between nodes (group parity), so node k's wgrads may still run during node k+1 and are joined
    // before node k+2 reuses their arena (and at the end of every backward call).  Null = everything on `st`.
    hipStream_t st2 = nullptr; hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
    char* opws2 = nullptr; int par = 0; bool launched = false, pend[2] = {false, false};
    const uint16_t* w_split = nullptr;   // pre-split weights (the bf16 modes, bd_split_bf16 layout): element e of params <-> 2*e here
    const uint16_t* wT_split = nullptr;  // transposed split planes Wt[ci][tap][co] of the 3x3 conv weights, same element offsets
    std::vector<char> ginit;
    // GroupNorm weight / bias gradients: the layers leave their per-sample partials in `gnpart` and ONE launch per
    // backward call folds them (bd_gn_bwd_params) -- 51 small launches off the dgrad chain of the CIFAR step
    float* gnpart = nullptr; size_t gnpart_floats = 0, gnpart_used = 0, gnpart_need = 0;
    std::vector<bd_gn_param_item> gn_items;
    // hands a GroupNorm backward its slot (or nothing: the layer then reduces its own parameters as before)
    float* gn_slot(int B, int HW, int C, int G, float* dgamma, float* dbeta) {
        if (!wg || !bd_gn_bwd_defers(B, HW, C, G)) return nullptr;
        const size_t n = ((size_t)B * 2 * C + 63) / 64 * 64;
        if (dry) { gnpart_need += n; return nullptr; }
        if (!gnpart || gnpart_used + n > gnpart_floats) return nullptr;
        float* p = gnpart + gnpart_used;
        gnpart_used += n;
        bd_gn_param_item it; it.partials = p; it.C = C; it.dgamma = dgamma; it.dbeta = dbeta;
        gn_items.push_back(it);
        return p;
    }
};

// one 3x3 convolution of the plan, built with its node (bd_unet::conv3_fwd / conv3_dgrad / conv3_wgrad)
struct Conv3 {
    int64_t pw, pb;               // weight [Cout][3][3][Cin] and bias in the flat parameter / gradient buffers
    int Cin, Cout, Hs, Ws;        // source grid
    int stride, pad, ups;         // ups: the source is nearest-upsampled x2 first (Upsample2D)
    int Ho, Wo;
};
static Conv3 conv3_same(int64_t pw, int64_t pb, int Cin, int Cout, int H, int W) { return Conv3{pw, pb, Cin, Cout, H, W, 1, 1, 0, H, W}; }
// an activation or gradient operand: fp32 [rows, ld] for the literal family, split planes [rows, ld] (ld = channels) for the plane family
struct Opnd { const float* p; int64_t ld; };
struct Conv3Epi {       // forward epilogue terms: y = out_scale * (conv + bias + rowbias + residual)
    const float* rowbias = nullptr; int64_t ld_rowbias = 0;     // [B, Cout] per sample (time embedding)
    const float* residual = nullptr; int64_t ldr = 0;
    float out_scale = 1.f;
    int gn_splits = 0;  // plane family: > 0 leaves the partial statistics of the GroupNorm that reads y next in the op workspace
};

// one Linear layer / 1x1 convolution of the plan: y[M, N] = x[M, K] W[N, K]^T + b (bd_unet::lin_fwd / lin_dgrad / lin_wgrad)
struct Lin { int64_t pw, pb; int N, K; };
struct LinEpi { const float* residual = nullptr; int64_t ldr = 0; float out_scale = 1.f; };     // y = out_scale * (x W^T + b + residual)
// the core of one attention block (bd_unet::attn_fwd / attn_bwd): buffers of qkv [B*N, 3C], the scores P [B, heads, N, N], o [B*N, C] and
// of their gradients; fp32 or split planes by the family of the call (same bytes)
struct Attn { int heads, N, dh, C; float scale; int b_qkv, b_p, b_o, b_do, b_dp, b_dqkv; };

typedef std::function<int(Ctx&)> Step;
// a node's kernel-path choice as a function of the batch the workspace is laid out for (bd_unet::takes adds the context's part)
typedef std::function<bool(int)> Path;

}  // namespace bd

using namespace bd;

struct bd_unet {
    bd_unet_config cfg;
    hipStream_t aux_stream = nullptr;              // created on the first backward (plan creation stays host-only)
    hipEvent_t aux_ev_fork = nullptr, aux_ev_join[2] = {nullptr, nullptr};
    hipEvent_t aux_ev_seg = nullptr;               // side-stream position after the last segment call's weight gradients
    bool aux_pend[2] = {false, false};             // carried from one bd_unet_backward_segment call to the next (same backward pass)
    int aux_enabled = 1, aux_defer = 0;
    std::vector<Buf> bufs;
    std::vector<Param> params;
    int64_t nparams = 0;
    std::vector<Step> fwd;
    struct BStep { Step fn; int seg; int group; };
    std::vector<BStep> bwd;  // in FORWARD emission order; executed reversed
    // gradient ranges that are final when a backward segment has run: the segment's own parameters [lo, hi) plus, for the
    // blocks that hold resnets, their rows of the batched time_emb_proj weight / bias (which live in the time-embedding
    // segment's range of the flat buffer but get their gradient inside the resnet's backward)
    struct Range { int64_t lo = -1, hi = -1; void cover(int64_t l, int64_t h) { if (lo < 0 || l < lo) lo = l; if (h > hi) hi = h; } };
    struct Seg { Range own, tw, tb; };
    std::vector<Seg> segs;   // indexed by segment id (backward order)
    int cur_seg = 0, cur_group = 0;
    // layout cache
    int lay_B = -1, lay_train = -1, lay_gen = -1;
    int fwd_gen = -1, fwd_B = -1; const void* fwd_ws = nullptr;   // the training forward whose saved activations are live (bd_tune_set guard)
    int64_t value_floats = 0, grad_floats = 0, scratch_floats = 0;
    size_t opws_bytes = 0, gnpart_floats = 0;
    int T = 0, sumC = 0;     // time-embed dim, total time_emb_proj rows
    int64_t p_tw = 0, p_tb = 0;  // offsets of the batched time_emb_proj weight / bias
    int b_tproj = -1, b_dtproj = -1, b_embs = -1;
    std::vector<long long> wt_off; std::vector<int> wt_cin, wt_cout;   // 3x3 conv weights with a transposed split copy
    // Round 4: a tensor's gradient handed over READY-SPLIT.  The producer of tensor T (a resnet / attention / down- / upsample node whose
    // backward starts by turning dL/dT into split planes) registers T; the FIRST node that consumes T in forward order is the LAST one to add
    // to dL/dT in backward, and if that node ends with a GroupNorm backward (resnet norm1, attention group_norm, conv_norm_out) the kernel
    // writes the planes of the final value next to the fp32 store (bd_gn_bwd_desc.dx_split + channel range): the producer's bd_split_rows
    // launch and its 4 B / element read disappear.  Consumers that end otherwise (down- / upsample data gradients) leave the fallback.
    // `want`: the producer's path predicate for a batch size (shape part; a context adds planes(c))
    struct GSplit { int buf, coff, C, H, W; int b_pl; Path want; bool claimed = false, emitted = false; };
    std::vector<GSplit> gsplits;
    int reg_gsplit(const View& y, Path want) {
        if (!Knobs::get().gsplit || y.buf < 0 || y.C % 32 != 0) return -1;
        GSplit e; e.buf = y.buf; e.coff = y.coff; e.C = y.C; e.H = y.H; e.W = y.W; e.want = std::move(want);
        const int keep = cur_group;
        e.b_pl = new_buf((int64_t)y.H * y.W * y.C, 0, R_GRAD);
        cur_group = keep;
        gsplits.push_back(std::move(e));
        const int idx = (int)gsplits.size() - 1;
        bufs[gsplits[idx].b_pl].live = [this, idx](int B, int training) { return training && gsplits[idx].emitted && gsplits[idx].want(B); };
        return idx;
    }
    // called by every node for its input view, in forward order: the first consumer of a registered tensor; `emits`: it can write the planes
    int claim_gsplit(const View& x, bool emits) {
        int got = -1;
        for (int i = 0; i < (int)gsplits.size(); ++i) {
            GSplit& e = gsplits[i];
            if (e.claimed || e.buf != x.buf || e.coff < x.coff || e.coff + e.C > x.coff + x.C) continue;
            e.claimed = true;
            if (emits && got < 0) { e.emitted = true; got = i; }      // (one range per consumer launch)
        }
        return got;
    }
    struct UpsW { int64_t pw; int C; Path phase; int b_e, b_et; };     // upsample convolutions on the phase path: E (/ E^T when training) planes
    // weight preprocessing (split copy, E planes) is skipped while the caller promises constant weights (bd_unet_set_static_weights):
    // a sampling loop runs 50-1000 forwards over the same parameters
    int static_weights = 0; const void* prep_params = nullptr; const void* prep_ws = nullptr; int prep_B = -1;
    std::vector<UpsW> upsw;
    void forget_prepared() { prep_params = nullptr; prep_ws = nullptr; prep_B = -1; }

    // ---------------------------------------------------------------- construction helpers
    int new_buf(int64_t per_sample, int64_t fixed, int region) {
        Buf b;
        b.per_sample = per_sample; b.fixed = fixed; b.region = region; b.group = cur_group;
        bufs.push_back(b);
        return (int)bufs.size() - 1;
    }
    View new_tensor(int H, int W, int C) {  // standalone value tensor with a grad buffer
        View v;
        v.buf = new_buf((int64_t)H * W * C, 0, R_VALUE);
        bufs[v.buf].gbuf = new_buf((int64_t)H * W * C, 0, R_GRAD);
        v.coff = 0; v.C = C; v.ld = C; v.H = H; v.W = W;
        return v;
    }
    View slice(const View& v, int coff, int C) const {
        View s = v;
        s.coff = v.coff + coff; s.C = C;
        return s;
    }
    int scratch(int64_t per_sample, int64_t fixed = 0) { return new_buf(per_sample, fixed, R_SCRATCH); }
    int64_t add_param(const std::string& name, std::initializer_list<int64_t> shape, int layout = 0) {
        Param p;
        p.name = name; p.rank = (int)shape.size(); p.layout = layout;
        int64_t n = 1; int i = 0;
        for (auto s : shape) { p.shape[i++] = s; n *= s; }
        for (; i < 4; ++i) p.shape[i] = 1;
        nparams = (nparams + 31) / 32 * 32;  // 128-byte aligned start: float4 loads, and whole 32-element blocks of the split copy
        p.off = nparams;
        nparams += n;
        params.push_back(p);
        if (!segs.empty()) segs[cur_seg].own.cover(p.off, p.off + n);
        return p.off;
    }
    void alias_param(const std::string& name, int64_t off, std::initializer_list<int64_t> shape) {
        Param p;
        p.name = name; p.rank = (int)shape.size(); p.layout = 0; p.off = off;
        int i = 0;
        for (auto s : shape) p.shape[i++] = s;
        for (; i < 4; ++i) p.shape[i] = 1;
        params.push_back(p);
    }
    void F(Step s) { fwd.push_back(std::move(s)); }
    void Bk(Step s) { bwd.push_back({std::move(s), cur_seg, cur_group}); }

    // ---------------------------------------------------------------- run-time helpers
    // c.s0 = first sample of this context (forward runs the two halves of the batch as two concurrent pipelines)
    float* VP(Ctx& c, const View& v) const { return c.ws + bufs[v.buf].off + c.s0 * bufs[v.buf].per_sample + v.coff; }
    float* GP(Ctx& c, const View& v) const {
        const Buf& g = bufs[bufs[v.buf].gbuf];
        return c.ws + g.off + c.s0 * g.per_sample + v.coff;
    }
    float* BP(Ctx& c, int b) const { return c.ws + bufs[b].off + c.s0 * bufs[b].per_sample; }
    // GroupNorm statistics buffer = [LB][G] means followed by [LB][G] rstds (batch-major, so not a per-sample slab)
    float* MEANP(Ctx& c, int b, int G) const { return c.ws + bufs[b].off + c.s0 * G; }
    float* RSTDP(Ctx& c, int b, int G) const { return c.ws + bufs[b].off + ((int64_t)c.LB + c.s0) * G; }
    static int64_t rows(const Ctx& c, const View& v) { return (int64_t)c.B * v.H * v.W; }

    // enqueue a weight-gradient launch on the side stream (after everything enqueued on c.st so far)
    template <class F>
    int on_aux(Ctx& c, F&& launch) const {
        if (!c.st2 || c.dry) return launch(c.st, c.opws);
        BD_HIP_TRY(hipEventRecord(c.ev_fork, c.st));
        BD_HIP_TRY(hipStreamWaitEvent(c.st2, c.ev_fork, 0));
        c.launched = true;
        return launch(c.st2, c.opws2);
    }
    // before a node of scratch parity p starts: wgrads of the previous node with that parity must be done
    static int aux_wait(Ctx& c, int p) {
        if (!c.pend[p]) return BD_OK;
        BD_HIP_TRY(hipStreamWaitEvent(c.st, c.ev_join[p], 0));
        c.pend[p] = false;
        return BD_OK;
    }
    // after a node: mark the completion point of the wgrads it enqueued
    static int aux_mark(Ctx& c, int p) {
        if (!c.launched) return BD_OK;
        BD_HIP_TRY(hipEventRecord(c.ev_join[p], c.st2));
        c.pend[p] = true; c.launched = false;
        return BD_OK;
    }
    // the op workspace is sized by the dry run: the maximum over every launch of the plan
    static void need(Ctx& c, size_t bytes) { if (bytes > c.opws_need) c.opws_need = bytes; }
    static void note_conv(Ctx& c) { need(c, bd_conv3x3_workspace_bytes(0, 0, 0, 0, 0, 0, 0, 0)); }
    // the first gradient contribution to a value buffer is written, every later one accumulates: returns the flag and sets it
    static int take_ginit(Ctx& c, int buf) {
        const int acc = c.ginit[buf];
        c.ginit[buf] = 1;
        return acc;
    }
    // the batch the workspace is laid out for (the forward's half-batch pipelines and the backward must agree on every path choice)
    static int lay_batch(const Ctx& c) { return c.LB > 0 ? c.LB : c.B; }
    // the split-plane kernels need the per-step plane copy of the weights (the dry run only sizes the workspace)
    static bool planes(const Ctx& c) { return c.dry || c.w_split; }
    // THE place that applies a context to a node's path choice
    static bool takes(const Ctx& c, const Path& path) { return planes(c) && path(lay_batch(c)); }
    static uint16_t* U16(float* p) { return reinterpret_cast<uint16_t*>(p); }
    static const uint16_t* U16(const float* p) { return reinterpret_cast<const uint16_t*>(p); }

    // a GEMM of either family; aux: a weight gradient, on the side stream (the attention block's on the main stream measured +0.35 ms per step)
    template <class D, class Bytes, class Launch>
    int gemm_run(Ctx& c, D& g, bool aux, Bytes bytes, Launch launch) const {
        if (aux && !c.wg) return BD_OK;
        g.workspace = c.opws; g.workspace_bytes = c.opws_bytes; g.mode = cfg.compute_mode;
        if (c.dry) { need(c, bytes(g)); return BD_OK; }
        if (aux) return on_aux(c, [&](hipStream_t st, char* ws) { g.workspace = ws; return launch(g, st); });
        return launch(g, c.st);
    }
    int igemm(Ctx& c, bd_igemm_desc& g, bool aux = false) const { return gemm_run(c, g, aux, igemm_workspace_bytes, igemm_launch); }
    int gemm_s(Ctx& c, bd_gemm_sp_desc& g, bool aux = false) const { return gemm_run(c, g, aux, gemm_sp_workspace_bytes, gemm_sp); }
    static bd_operand dense(const float* p, int64_t ld, int kc) {
        bd_operand o = {};
        o.kind = BD_OPK_DENSE; o.kc = kc; o.p = p; o.ld = ld;
        return o;
    }
    // C[M, N] = op(A) op(B), one problem: fp32 operands (kc: the operand's rows run along K) / split planes (km: K-major)
    static bd_igemm_desc gemm_f32(const float* A, int64_t lda, int kca, const float* B, int64_t ldb, int kcb, int M, int N, int K, float* C,
                                  int64_t ldc) {
        bd_igemm_desc g = {};
        g.A = dense(A, lda, kca); g.B = dense(B, ldb, kcb);
        g.M = M; g.N = N; g.K = K; g.batch_outer = g.batch_inner = 1;
        g.C = C; g.ldc = ldc; g.alpha = 1.f; g.out_scale = 1.f;
        return g;
    }
    static bd_gemm_sp_desc gemm_planes(const uint16_t* a, int64_t lda, int akm, const uint16_t* b, int64_t ldb, int bkm, int M, int N, int K) {
        bd_gemm_sp_desc g = {};
        g.M = M; g.N = N; g.K = K; g.batch = 1;
        g.a = a; g.lda = lda; g.a_kmajor = akm; g.b = b; g.ldb = ldb; g.b_kmajor = bkm;
        g.alpha = 1.f; g.out_scale = 1.f;
        return g;
    }
    // ---- Linear layers / 1x1 convolutions.  Two families like the 3x3 convolutions: igemm on fp32 operands, and bd_gemm_sp on split planes
    // with the per-step plane copy of the weight (K-contiguous rows: the layout a [N][K] weight wants forward, and the K-major operand of its
    // data gradient as it stands).  The family is a flag per CALL (the shortcut's data gradient takes planes while its forward and weight
    // gradient stay on igemm); the gates (gemm_sp_supported, ld % 4, BD_SHORTCUT_SP) stay where the node decides its path.
    // y = out_scale * (x W^T + b + residual);  y_planes (plane family): y receives split planes [M, ldy] instead of fp32
    int lin_fwd(Ctx& c, const Lin& l, bool sp, const Opnd& x, float* y, int64_t ldy, int M, bool y_planes = false, const LinEpi& e = LinEpi()) const {
        if (!sp) {
            bd_igemm_desc g = gemm_f32(x.p, x.ld, 1, c.params + l.pw, l.K, 1, M, l.N, l.K, y, ldy);
            g.bias = c.params + l.pb; g.residual = e.residual; g.ldr = e.ldr; g.out_scale = e.out_scale;
            return igemm(c, g);
        }
        bd_gemm_sp_desc g = gemm_planes(U16(x.p), x.ld, 0, c.w_split + 2 * l.pw, l.K, 0, M, l.N, l.K);
        if (y_planes) { g.c_split = U16(y); g.ldcs = ldy; }
        else { g.c = y; g.ldc = ldy; }
        g.bias = c.params + l.pb; g.residual = e.residual; g.ldr = e.ldr; g.out_scale = e.out_scale;
        return gemm_s(c, g);
    }
    // dx[M, K] (+)= dy[M, N] W;  dx_planes (plane family): dx receives split planes, written
    int lin_dgrad(Ctx& c, const Lin& l, bool sp, const Opnd& dy, float* dx, int64_t lddx, int M, int acc, bool dx_planes = false) const {
        if (!sp) {
            bd_igemm_desc g = gemm_f32(dy.p, dy.ld, 1, c.params + l.pw, l.K, 0, M, l.K, l.N, dx, lddx);
            g.accumulate = acc;
            return igemm(c, g);
        }
        bd_gemm_sp_desc g = gemm_planes(U16(dy.p), dy.ld, 0, c.w_split + 2 * l.pw, l.K, 1, M, l.K, l.N);
        if (dx_planes) { g.c_split = U16(dx); g.ldcs = lddx; }
        else { g.c = dx; g.ldc = lddx; g.accumulate = acc; }
        return gemm_s(c, g);
    }
    // dW[N, K] = dy[M, N]^T x[M, K], db[N] = column sums of dy out of the same launch; on the side stream in either family
    int lin_wgrad(Ctx& c, const Lin& l, bool sp, const Opnd& dy, const Opnd& x, int M) const {
        if (!sp) {
            bd_igemm_desc g = gemm_f32(dy.p, dy.ld, 0, x.p, x.ld, 0, l.N, l.K, M, c.grads + l.pw, l.K);
            g.a_colsum = c.grads + l.pb;
            return igemm(c, g, true);
        }
        bd_gemm_sp_desc g = gemm_planes(U16(dy.p), dy.ld, 1, U16(x.p), x.ld, 1, l.N, l.K, M);
        g.c = c.grads + l.pw; g.ldc = l.K; g.a_colsum = c.grads + l.pb;
        return gemm_s(c, g, true);
    }
    // rows [lo, hi) of the batched time_emb_proj weight / bias gradient, dW = dtproj[:, rows]^T embs (resnet.py:571): the rows of a backward
    // segment are adjacent in the [sumC, T] projection, so one GEMM per segment (one for a whole backward) replaces one tiny launch per resnet
    int temb_wgrad(Ctx& c, int64_t lo, int64_t hi) const {
        const Lin rows = {p_tw + lo * T, p_tb + lo, (int)(hi - lo), T};
        return lin_wgrad(c, rows, false, {BP(c, b_dtproj) + lo, sumC}, {BP(c, b_embs), T}, c.B);
    }

    // ---- the attention core: P = softmax(scale Q K^T), O = P V per head, and its backward.  Plane family (attn_sp.hip): one launch forward,
    // two backward, the [N, N] matrices stay on chip (P^T is kept for the backward when training); fp32 family: per-head batched igemm products
    // around the softmax kernels, operands being [B*N, ld] token matrices whose head h owns columns [h*dh, (h+1)*dh), or the scores
    struct HeadMat { float* p; int64_t ld, bs_outer, bs_inner; int cols; };
    static HeadMat tokens(const Attn& a, float* p, int64_t ld) { return {p, ld, (int64_t)a.N * ld, a.dh, a.dh}; }
    static HeadMat scores(const Attn& a, float* p) { return {p, a.N, (int64_t)a.heads * a.N * a.N, (int64_t)a.N * a.N, a.N}; }
    // C = alpha * op(A) op(B) for every (sample, head); ta: A is read transposed ([K, M] rows), bt: B holds [N, K] rows
    int head_gemm(Ctx& c, const Attn& a, const HeadMat& A, bool ta, const HeadMat& B, bool bt, const HeadMat& C, float alpha) const {
        bd_igemm_desc g = gemm_f32(A.p, A.ld, ta ? 0 : 1, B.p, B.ld, bt ? 1 : 0, a.N, C.cols, ta ? a.N : A.cols, C.p, C.ld);
        g.A.bs_outer = A.bs_outer; g.A.bs_inner = A.bs_inner; g.B.bs_outer = B.bs_outer; g.B.bs_inner = B.bs_inner;
        g.c_bs_outer = C.bs_outer; g.c_bs_inner = C.bs_inner; g.batch_outer = c.B; g.batch_inner = a.heads; g.alpha = alpha;
        return igemm(c, g);
    }
    bd_attn_sp_desc attn_planes(Ctx& c, const Attn& a) const {
        bd_attn_sp_desc d = {};
        d.B = c.B; d.heads = a.heads; d.N = a.N; d.dh = a.dh; d.qkv_split = U16(BP(c, a.b_qkv)); d.ld = 3 * a.C; d.scale = a.scale;
        d.mode = cfg.compute_mode;
        return d;
    }
    int attn_fwd(Ctx& c, const Attn& a, bool sp) const {
        if (sp) {
            if (c.dry) return BD_OK;
            bd_attn_sp_desc d = attn_planes(c, a);
            d.o_split = U16(BP(c, a.b_o)); d.ldo = a.C; d.pt_split = c.training ? U16(BP(c, a.b_p)) : nullptr;
            return attn_sp_fwd(d, c.st);
        }
        float* qkv = BP(c, a.b_qkv); float* P = BP(c, a.b_p);
        const int C = a.C;
        BD_TRY(head_gemm(c, a, tokens(a, qkv, 3 * C), false, tokens(a, qkv + C, 3 * C), true, scores(a, P), a.scale));       // S = scale * Q K^T
        if (!c.dry) BD_TRY(bd_softmax_fwd(P, P, (int64_t)c.B * a.heads * a.N, a.N, (bd_stream_t)c.st));
        return head_gemm(c, a, scores(a, P), false, tokens(a, qkv + 2 * C, 3 * C), false, tokens(a, BP(c, a.b_o), C), 1.f);      // O = P V
    }
    // dqkv from dO (b_do), in the family's format
    int attn_bwd(Ctx& c, const Attn& a, bool sp) const {
        if (sp) {
            if (c.dry) return BD_OK;
            bd_attn_sp_desc d = attn_planes(c, a);
            d.pt_split = U16(BP(c, a.b_p)); d.do_split = U16(BP(c, a.b_do)); d.lddo = a.C; d.dst_split = U16(BP(c, a.b_dp));
            d.dqkv_split = U16(BP(c, a.b_dqkv)); d.lddqkv = 3 * a.C;
            return attn_sp_bwd(d, c.st);
        }
        float* qkv = BP(c, a.b_qkv); float* dqkv = BP(c, a.b_dqkv); float* P = BP(c, a.b_p); float* dP = BP(c, a.b_dp);
        const int C = a.C;
        const HeadMat dO = tokens(a, BP(c, a.b_do), C);
        BD_TRY(head_gemm(c, a, dO, false, tokens(a, qkv + 2 * C, 3 * C), true, scores(a, dP), 1.f));                        // dP = dO V^T
        BD_TRY(head_gemm(c, a, scores(a, P), true, dO, false, tokens(a, dqkv + 2 * C, 3 * C), 1.f));                        // dV = P^T dO
        if (!c.dry) BD_TRY(bd_softmax_bwd(P, dP, dP, (int64_t)c.B * a.heads * a.N, a.N, (bd_stream_t)c.st));
        BD_TRY(head_gemm(c, a, scores(a, dP), false, tokens(a, qkv + C, 3 * C), false, tokens(a, dqkv, 3 * C), a.scale));   // dQ = scale * dS K
        return head_gemm(c, a, scores(a, dP), true, tokens(a, qkv, 3 * C), false, tokens(a, dqkv + C, 3 * C), a.scale);     // dK = scale * dS^T Q
    }

    // launches without a workspace, on the main stream: the dry run has nothing to account for
    int colsum(Ctx& c, const float* x, int64_t ldx, int64_t nrows, int N, int64_t rpg, float* out, int64_t ldo) const {
        return c.dry ? BD_OK : bd_colsum(x, ldx, nrows, N, rpg, out, ldo, 0, c.st);
    }
    int add(Ctx& c, const float* src, int64_t lds, float* dst, int64_t ldd, int64_t nrows, int C, float scale, int acc) const {
        return c.dry ? BD_OK : add_launch(src, lds, dst, ldd, nrows, C, scale, acc, c.st);
    }
    int split_rows(Ctx& c, const float* src, int64_t ld, int64_t nrows, int C, float* dst) const {
        return c.dry ? BD_OK : bd_split_rows(src, ld, nrows, C, U16(dst), C, (bd_stream_t)c.st);
    }
    // ... of the nearest-upsampled x2 image: planes [B, 2H, 2W, C]
    int split_rows_ups2(Ctx& c, const float* src, int64_t ld, int H, int W, int C, float* dst) const {
        return c.dry ? BD_OK : bd_split_rows_ups2(src, ld, c.B, H, W, C, U16(dst), C, (bd_stream_t)c.st);
    }
    // dst [B, H, W, C] (+)= sums over the 2x2 blocks of src [B, 2H, 2W, C]: the adjoint of the nearest upsampling
    int sum2x2(Ctx& c, const float* src, int64_t lds, float* dst, int64_t ldd, int H, int W, int C, int acc) const {
        return c.dry ? BD_OK : bd_sum2x2(src, lds, dst, ldd, c.B, H, W, C, acc, (bd_stream_t)c.st);
    }
    int silu_fwd(Ctx& c, const float* x, float* y, int64_t n) const { return c.dry ? BD_OK : bd_silu_fwd(x, y, n, (bd_stream_t)c.st); }
    int silu_bwd(Ctx& c, const float* x, const float* dy, float* dx, int64_t n) const {
        return c.dry ? BD_OK : bd_silu_bwd(x, dy, dx, n, 0, (bd_stream_t)c.st);
    }
    int timestep_embedding(Ctx& c, int dim, float* out) const {
        if (c.dry) return BD_OK;
        if (c.tf) return bd_timestep_embedding_f32(c.tf, c.t_stride, c.B, dim, cfg.flip_sin_to_cos, cfg.freq_shift, out, (bd_stream_t)c.st);
        return bd_timestep_embedding(c.t, c.t_stride, c.B, dim, cfg.flip_sin_to_cos, cfg.freq_shift, out, (bd_stream_t)c.st);
    }
    // bias gradient: per-sample column sums (scratch [B,N]) then a sum over the batch (fixed order)
    int bias_grad(Ctx& c, const float* dY, int64_t ld, int HW, int N, int scratch_buf, float* db) const {
        if (!c.wg) return BD_OK;
        float* s = BP(c, scratch_buf);
        BD_TRY(colsum(c, dY, ld, (int64_t)c.B * HW, N, HW, s, N));
        return colsum(c, s, N, c.B, N, c.B, db, N);
    }

    // ---- GroupNorm (+SiLU).  x is a View (forward / backward into its gradient buffer) or, for a tensor without a persistent gradient
    // buffer (the resnet's h1), the View of its value and a destination the caller names
    // planes: y receives split planes [rows, x.C] ONLY (the operand of the plane kernels that read it next) instead of fp32 [rows, ldy]
    // stats_splits > 0: the producing convolution left the statistics' partials in the op workspace (Conv3Epi::gn_splits): no pass over x
    int gn_fwd(Ctx& c, const View& x, int64_t pg, int64_t pb, float* y, int64_t ldy, int stats_buf, int silu, bool planes = false,
               int stats_splits = 0) const {
        bd_gn_fwd_desc d = {};
        d.B = c.B; d.HW = x.H * x.W; d.C = x.C; d.G = cfg.norm_num_groups; d.eps = cfg.norm_eps; d.silu = silu;
        d.x = VP(c, x); d.ldx = x.ld; d.gamma = c.params + pg; d.beta = c.params + pb;
        if (planes) { d.y = nullptr; d.ldy = x.C; d.y_split = U16(y); d.ldys = x.C; }
        else { d.y = y; d.ldy = ldy; }
        d.mean = MEANP(c, stats_buf, d.G); d.rstd = RSTDP(c, stats_buf, d.G);
        d.workspace = c.opws; d.workspace_bytes = c.opws_bytes;
        if (stats_splits > 0) { d.stats = reinterpret_cast<const double*>(c.opws); d.stats_splits = stats_splits; }
        if (c.dry) { need(c, bd_gn_workspace_bytes(c.B, x.C)); return BD_OK; }
        return bd_gn_fwd(&d, (bd_stream_t)c.st);
    }
    // `d` arrives with the destination filled in: dx / lddx / accumulate_dx and, optionally, dx_split, dx_add, dx_colsum
    // (dx_colsum feeds a weight gradient only: dropped with the parameter sums in the data-gradient-only schedule)
    int gn_bwd(Ctx& c, bd_gn_bwd_desc& d, const View& x, int64_t pg, int64_t pb, int stats_buf, const float* dy, int64_t lddy, int silu) const {
        d.B = c.B; d.HW = x.H * x.W; d.C = x.C; d.G = cfg.norm_num_groups; d.silu = silu;
        d.x = VP(c, x); d.ldx = x.ld; d.gamma = c.params + pg; d.beta = c.params + pb;
        d.mean = MEANP(c, stats_buf, d.G); d.rstd = RSTDP(c, stats_buf, d.G);
        d.dy = dy; d.lddy = lddy;
        if (c.wg) { d.dgamma = c.grads + pg; d.dbeta = c.grads + pb; }      // (else: bd_gn_bwd leaves the parameter sums out)
        else { d.dx_colsum = nullptr; d.ld_colsum = 0; }
        d.workspace = c.opws; d.workspace_bytes = c.opws_bytes;
        d.param_partials = c.gn_slot(d.B, d.HW, d.C, d.G, d.dgamma, d.dbeta);
        if (c.dry) return BD_OK;
        return bd_gn_bwd(&d, (bd_stream_t)c.st);
    }
    // ... into x's gradient buffer (+ dx_add, a second gradient of x folded into the store); gs: the GSplit entry this launch can serve
    int gn_bwd(Ctx& c, const View& x, int64_t pg, int64_t pb, int stats_buf, const float* dy, int64_t lddy, int silu,
               const float* dx_add = nullptr, int64_t ld_add = 0, int gs = -1) const {
        bd_gn_bwd_desc d = {};
        d.dx_add = dx_add; d.ld_add = ld_add;
        if (gs >= 0 && takes(c, gsplits[gs].want)) {      // this launch makes dL/dx final: hand its producer the planes of its channel range
            const GSplit& e = gsplits[gs];
            d.dx_split = U16(BP(c, e.b_pl)); d.lddxs = e.C; d.dx_split_c0 = e.coff - x.coff; d.dx_split_c1 = d.dx_split_c0 + e.C;
        }
        d.dx = GP(c, x); d.lddx = x.ld; d.accumulate_dx = take_ginit(c, x.buf);
        return gn_bwd(c, d, x, pg, pb, stats_buf, dy, lddy, silu);
    }

    // ---- 3x3 convolutions.  Two kernel families: the literal implicit GEMM on fp32 operands (conv.cpp; any stride / padding / folded
    // nearest-upsampling) and the split-plane LDS-DMA kernels of conv_ps.hip (stride 1, pad 1, on the OUTPUT grid; the bf16 modes only, same
    // arithmetic as igemm, bit-identical).  A node takes ONE decision per convolution and step (a Path over ps_shape), for its forward, data
    // gradient and weight gradient alike -- they share the split operands -- and hands it to the three helpers below with operands in that family's
    // format; everything that follows from the decision (descriptor, weight copy, workspace, stream, dry-run accounting) lives in them.
    template <class D>
    static void conv3_geometry(D& d, const Ctx& c, const Conv3& k) {
        d.B = c.B; d.Hs = k.Hs; d.Ws = k.Ws; d.Cin = k.Cin; d.Cout = k.Cout; d.stride = k.stride; d.pad_t = k.pad; d.pad_l = k.pad; d.ups = k.ups;
        d.Ho = k.Ho; d.Wo = k.Wo;
    }
    // One decision per convolution, for its forward, data gradient and weight gradient alike, taken on the batch the workspace is laid
    // out for; shapes per conv3x3_ps_supported
    bool ps_shape(int B, int H, int W, int Cin, int Cout) const {
        return Knobs::get().conv_ps && mode_bf16(cfg.compute_mode) && conv3x3_ps_supported(B, H, W, Cin, Cout) &&
               conv3x3_ps_supported(B, H, W, Cout, Cin) && conv3x3_ps_wgrad_supported(B, H, W, Cin, Cout);
    }
    // phase-decomposed forms (conv_ph.hip): the upsample convolution on its SOURCE grid, the stride-2 data gradient by parity class
    // `min_wgs`: the launch must offer at least that many 256 x 128 workgroups (classes x tiles on the batch the workspace is laid
    // out for) -- a one-class 16-tap data gradient of an 8 x 8 source grid is 64 long workgroups on 256 CUs and loses to the literal form
    bool phase_shape(int B, int H, int W, int Cin, int Cout, int classes = 4, int min_wgs = 128) const {
        const long long wgs = (long long)classes * (((long long)B * H * W + 255) / 256) * (Cout / 128);
        return mode_bf16(cfg.compute_mode) && upsample_conv_ps_supported(B, H, W, Cin, Cout) && wgs >= min_wgs;
    }
    // the upsample convolution's data gradient as ONE class of 16 taps on dY sampled at stride 2 (else: the fine-grid form + 2x2 sums): with
    // >= 128 tiles of its own, or >= 32 where the launch deals the taps of a tile to four workgroups, as it does while the tiles fill at most half
    // the chip: the launcher's own decision (upsample_conv_dgrad_tap_groups, conv_ph.hip), read here as the plan's path choice.
    bool phase_dgrad_shape(int B, int H, int W, int C) const {
        return phase_shape(B, H, W, C, C, upsample_conv_dgrad_tap_groups(B, H, W, C));
    }
    // the plane kernel in either direction: +1 forward (W planes of the per-step split copy), -1 data gradient (transposed planes)
    int conv3_planes(Ctx& c, const Conv3& k, int direction, const Opnd& x, float* y, int64_t ldy, int acc, const Conv3Epi& e) const {
        bd_conv3x3_ps_desc d = {};
        d.B = c.B; d.H = k.Ho; d.W = k.Wo; d.direction = direction;
        d.K = direction > 0 ? k.Cin : k.Cout; d.N = direction > 0 ? k.Cout : k.Cin;
        d.x_split = U16(x.p); d.ldx = x.ld; d.w_split = (direction > 0 ? c.w_split : c.wT_split) + 2 * k.pw;
        if (direction > 0) d.bias = c.params + k.pb;
        d.rowbias = e.rowbias; d.ld_rowbias = e.ld_rowbias; d.residual = e.residual; d.ldr = e.ldr; d.out_scale = e.out_scale;
        d.y = y; d.ldy = ldy; d.accumulate = acc;
        d.workspace = c.opws; d.workspace_bytes = c.opws_bytes; d.mode = cfg.compute_mode;
        if (e.gn_splits > 0) {
            d.gn_part = reinterpret_cast<double*>(c.opws); d.gn_groups = cfg.norm_num_groups;
            if (c.dry) need(c, gn_stats_partial_bytes(c.B, e.gn_splits, d.gn_groups));
        }
        if (c.dry) { note_conv(c); return BD_OK; }
        return conv3x3_ps(d, c.st);
    }
    int conv3_fwd(Ctx& c, const Conv3& k, bool ps, const Opnd& x, float* y, int64_t ldy, const Conv3Epi& e = Conv3Epi()) const {
        if (ps) return conv3_planes(c, k, 1, x, y, ldy, 0, e);
        bd_conv3x3_fwd_desc d = {};
        conv3_geometry(d, c, k);
        d.x = x.p; d.ldx = x.ld; d.w = c.params + k.pw; d.bias = c.params + k.pb;
        d.rowbias = e.rowbias; d.ld_rowbias = e.ld_rowbias; d.residual = e.residual; d.ldr = e.ldr; d.out_scale = e.out_scale;
        d.y = y; d.ldy = ldy;
        d.workspace = c.opws; d.workspace_bytes = c.opws_bytes; d.mode = cfg.compute_mode;
        if (c.dry) { note_conv(c); return BD_OK; }
        if (c.w_split) d.w_split = c.w_split + 2 * k.pw;
        return conv3x3_fwd(d, c.st);
    }
    // dx (+)= data gradient, over the convolution's own (virtual, upsampled) input grid
    int conv3_dgrad(Ctx& c, const Conv3& k, bool ps, const Opnd& dy, float* dx, int64_t lddx, int acc) const {
        if (ps) return conv3_planes(c, k, -1, dy, dx, lddx, acc, Conv3Epi());
        bd_conv3x3_dgrad_desc d = {};
        conv3_geometry(d, c, k);
        d.dy = dy.p; d.lddy = dy.ld; d.w = c.params + k.pw; d.dx = dx; d.lddx = lddx; d.accumulate = acc;
        d.workspace = c.opws; d.workspace_bytes = c.opws_bytes; d.mode = cfg.compute_mode;
        if (c.dry) { note_conv(c); return BD_OK; }
        if (c.w_split) d.w_split = c.w_split + 2 * k.pw;
        return conv3x3_dgrad(d, c.st);
    }
    // the last link of the data-gradient chain: dL/dx of the network input (bd_unet_backward_input; c.dx null: not wanted), on the main stream
    int conv3_dgrad_input(Ctx& c, const Conv3& k, const Opnd& dy) const {
        if (!c.dx && !c.dry) return BD_OK;
        return conv3_dgrad(c, k, false, dy, c.dx, c.lddx, 0);
    }
    // Conv3Epi::gn_splits of a plane-family forward: > 0 where the GroupNorm that reads its output would otherwise make a pass for its statistics
    int conv3_gn_splits(const Ctx& c, const Conv3& k) const {
        const int G = cfg.norm_num_groups;
        return bd_gn_fwd_takes_stats(c.B, k.Ho * k.Wo, k.Cout, G) ? bd_conv3x3_ps_gn_splits(c.B, k.Ho, k.Wo, k.Cin, k.Cout, G) : 0;
    }
    // weight and bias gradient.  Every weight gradient runs on the side stream: keeping the large layers' (they fill the chip on their own)
    // or the 4 x 4 / 8 x 8 layers' (10-30 us launches, as long as the fork / join) on the main stream measured 0.2 - 0.7 ms per step slower
    // bias_scratch >= 0: a [B, Cout] scratch for a Cout the igemm row-sum fusion cannot take (conv_out, Cout = 3): the bias gradient is
    // then column sums on the main stream, unless the direct thin kernel runs, which sums dy on the way
    int conv3_wgrad(Ctx& c, const Conv3& k, bool ps, const Opnd& x, const Opnd& dy, int bias_scratch = -1) const {
        if (!c.wg) return BD_OK;
        if (ps) {
            bd_conv3x3_ps_wgrad_desc d = {};
            d.B = c.B; d.H = k.Ho; d.W = k.Wo; d.Cin = k.Cin; d.Cout = k.Cout;
            d.x_split = U16(x.p); d.ldx = x.ld; d.dy_split = U16(dy.p); d.lddy = dy.ld;
            d.dw = c.grads + k.pw; d.db = c.grads + k.pb;
            d.workspace_bytes = c.opws_bytes; d.mode = cfg.compute_mode;
            if (c.dry) {
                note_conv(c);
                need(c, conv3x3_ps_wgrad_workspace_bytes(d));      // K-split slabs of this layer (grow with the tile of the shared-tap form)
                return BD_OK;
            }
            return on_aux(c, [&](hipStream_t st, char* ws) { d.workspace = ws; return conv3x3_ps_wgrad(d, st); });
        }
        bd_conv3x3_wgrad_desc d = {};
        conv3_geometry(d, c, k);
        d.x = x.p; d.ldx = x.ld; d.dy = dy.p; d.lddy = dy.ld; d.dw = c.grads + k.pw; d.db = c.grads + k.pb;
        if (bias_scratch >= 0 && !conv3x3_wgrad_is_thin(d)) {
            d.db = nullptr;
            BD_TRY(bias_grad(c, dy.p, dy.ld, k.Ho * k.Wo, k.Cout, bias_scratch, c.grads + k.pb));
        }
        d.workspace = c.opws; d.workspace_bytes = c.opws_bytes; d.mode = cfg.compute_mode;
        if (c.dry) { note_conv(c); return BD_OK; }
        return on_aux(c, [&](hipStream_t st, char* ws) { d.workspace = ws; return conv3x3_wgrad(d, st); });
    }
    // ---- phase-decomposed forms (conv_ph.hip) of the upsample convolution k (ups = 1), on its SOURCE grid: x as split planes there, dy as
    // split planes on the fine grid, the pre-summed tap planes E / E^T of the layer (prepared with the weights' plane copy)
    bd_upsample_conv_desc phase_ups(const Ctx& c, const Conv3& k) const {
        bd_upsample_conv_desc d = {};
        d.mode = cfg.compute_mode; d.B = c.B; d.H = k.Hs; d.W = k.Ws; d.Cin = k.Cin; d.Cout = k.Cout;
        return d;
    }
    int phase_ups_fwd(Ctx& c, const Conv3& k, const Opnd& x, const float* e_planes, float* y, int64_t ldy) const {
        if (c.dry) return BD_OK;
        bd_upsample_conv_desc d = phase_ups(c, k);
        d.x_split = U16(x.p); d.ldx = x.ld; d.e_split = U16(e_planes); d.bias = c.params + k.pb; d.y = y; d.ldy = ldy;
        return upsample_conv_fwd(d, c.st);
    }
    int phase_ups_wgrad(Ctx& c, const Conv3& k, const Opnd& x, const Opnd& dy) const {
        if (!c.wg) return BD_OK;
        bd_upsample_conv_desc d = phase_ups(c, k);
        d.x_split = U16(x.p); d.ldx = x.ld; d.dy_split = U16(dy.p); d.lddy = dy.ld; d.dw = c.grads + k.pw; d.db = c.grads + k.pb;
        d.workspace_bytes = c.opws_bytes;
        if (c.dry) { need(c, upsample_conv_wgrad_workspace_bytes(d)); return BD_OK; }
        return on_aux(c, [&](hipStream_t st, char* ws) { d.workspace = ws; return upsample_conv_wgrad(d, st); });
    }
    // the one-class form (phase_dgrad_shape): dx (+)= 16 taps on dY sampled at stride 2
    int phase_ups_dgrad(Ctx& c, const Conv3& k, const Opnd& dy, const float* et_planes, float* dx, int64_t lddx, int acc) const {
        bd_upsample_conv_desc d = phase_ups(c, k);
        d.dy_split = U16(dy.p); d.lddy = dy.ld; d.et_split = U16(et_planes); d.dx = dx; d.lddx = lddx; d.accumulate = acc;
        d.workspace = c.opws; d.workspace_bytes = c.opws_bytes;
        if (c.dry) { need(c, upsample_conv_dgrad_workspace_bytes(d)); return BD_OK; }
        return upsample_conv_dgrad(d, c.st);
    }
    // data gradient of the stride-2 convolution k by the parity class of the input pixel (4 / 2 / 2 / 1 of the nine taps), from dy as split
    // planes on the output grid and the transposed weight planes
    int phase_s2_dgrad(Ctx& c, const Conv3& k, const Opnd& dy, float* dx, int64_t lddx, int acc) const {
        if (c.dry) return BD_OK;
        bd_conv3x3_s2_dgrad_desc g = {};
        g.B = c.B; g.Ho = k.Ho; g.Wo = k.Wo; g.Cin = k.Cin; g.Cout = k.Cout; g.pad = k.pad;
        g.dy_split = U16(dy.p); g.lddy = dy.ld; g.wT_split = c.wT_split + 2 * k.pw;
        g.dx = dx; g.lddx = lddx; g.accumulate = acc; g.mode = cfg.compute_mode;
        return conv3x3_s2_dgrad_ps(g, c.st);
    }
    // dL/dy of a node's output [nrows, C] as split planes (GSplit): the ones y's first consumer left when it made the gradient final (run-time
    // fact: `emitted` is set after the producer node was built), else bd_split_rows of the fp32 gradient into the node's own scratch
    int grad_planes(Ctx& c, int gs, const float* dy, int64_t lddy, int64_t nrows, int C, int b_scratch, Opnd& out) const {
        const bool ready = gs >= 0 && gsplits[gs].emitted;
        float* pl = BP(c, ready ? gsplits[gs].b_pl : b_scratch);
        if (!ready) BD_TRY(split_rows(c, dy, lddy, nrows, C, pl));
        out = Opnd{pl, C};
        return BD_OK;
    }

    // ---------------------------------------------------------------- nodes
    void build();
    void node_time_embed();
    void node_conv_in(const View& y);
    void node_resnet(const std::string& pre, const View& x, const View& y, int toff, float scale);
    void node_attention(const std::string& pre, const View& x, const View& y, float scale);
    void node_downsample(const std::string& pre, const View& x, const View& y);
    void node_upsample(const std::string& pre, const View& x, const View& y);
    void node_conv_out(const View& x);
    void layout(int B, int training);
};

// ----------------------------------------------------------------------------------------------------
void bd_unet::node_time_embed() {
    const int c0 = cfg.block_out_channels[0];
    const Lin l1 = {add_param("time_embedding.linear_1.weight", {T, c0}), add_param("time_embedding.linear_1.bias", {T}), T, c0};
    const Lin l2 = {add_param("time_embedding.linear_2.weight", {T, T}), add_param("time_embedding.linear_2.bias", {T}), T, T};
    // batched time_emb_proj of every resnet: one [sumC, T] weight, one [sumC] bias (aliases registered per resnet)
    segs[cur_seg].own.hi = nparams;      // the time segment proper: linear_1 / linear_2 (the batched projection below is
    nparams = (nparams + 31) / 32 * 32;   // reduced row range by row range with the blocks that own the resnets)
    p_tw = nparams; nparams += (int64_t)sumC * T;
    p_tb = nparams; nparams += sumC;
    const Lin lp = {p_tw, p_tb, sumC, T};
    const int b_tsin = new_buf(c0, 0, R_VALUE), b_e1 = new_buf(T, 0, R_VALUE), b_e1s = new_buf(T, 0, R_VALUE);
    const int b_emb = new_buf(T, 0, R_VALUE);
    b_embs = new_buf(T, 0, R_VALUE);
    b_tproj = new_buf(sumC, 0, R_VALUE);
    b_dtproj = new_buf(sumC, 0, R_GRAD);
    const int b_dembs = scratch(T), b_demb = scratch(T), b_de1s = scratch(T), b_de1 = scratch(T);
    F([=](Ctx& c) {
        BD_TRY(timestep_embedding(c, c0, BP(c, b_tsin)));
        BD_TRY(lin_fwd(c, l1, false, {BP(c, b_tsin), c0}, BP(c, b_e1), T, c.B));
        BD_TRY(silu_fwd(c, BP(c, b_e1), BP(c, b_e1s), (int64_t)c.B * T));
        BD_TRY(lin_fwd(c, l2, false, {BP(c, b_e1s), T}, BP(c, b_emb), T, c.B));
        BD_TRY(silu_fwd(c, BP(c, b_emb), BP(c, b_embs), (int64_t)c.B * T));
        return lin_fwd(c, lp, false, {BP(c, b_embs), T}, BP(c, b_tproj), lp.N, c.B);
    });
    Bk([=](Ctx& c) {
        if (!c.wg) return (int)BD_OK;      // the timestep is not differentiable: this branch feeds weight gradients only
        // (the weight / bias gradient of the batched projection is produced segment by segment: temb_wgrad)
        BD_TRY(lin_dgrad(c, lp, false, {BP(c, b_dtproj), lp.N}, BP(c, b_dembs), T, c.B, 0));
        BD_TRY(silu_bwd(c, BP(c, b_emb), BP(c, b_dembs), BP(c, b_demb), (int64_t)c.B * T));
        BD_TRY(lin_wgrad(c, l2, false, {BP(c, b_demb), T}, {BP(c, b_e1s), T}, c.B));
        BD_TRY(lin_dgrad(c, l2, false, {BP(c, b_demb), T}, BP(c, b_de1s), T, c.B, 0));
        BD_TRY(silu_bwd(c, BP(c, b_e1), BP(c, b_de1s), BP(c, b_de1), (int64_t)c.B * T));
        return lin_wgrad(c, l1, false, {BP(c, b_de1), T}, {BP(c, b_tsin), c0}, c.B);
    });
}

void bd_unet::node_conv_in(const View& y) {
    const int S_ = cfg.sample_size;
    const int64_t pw = add_param("conv_in.weight", {y.C, cfg.in_channels, 3, 3}, 1);
    const int64_t pb = add_param("conv_in.bias", {y.C});
    const Conv3 k = conv3_same(pw, pb, cfg.in_channels, y.C, S_, S_);
    F([=](Ctx& c) { return conv3_fwd(c, k, false, {c.x, c.ldx}, VP(c, y), y.ld); });
    Bk([=](Ctx& c) {
        const Opnd dy = {GP(c, y), y.ld};
        BD_TRY(conv3_wgrad(c, k, false, {c.x, c.ldx}, dy));
        return conv3_dgrad_input(c, k, dy);
    });
}

void bd_unet::node_resnet(const std::string& pre, const View& x, const View& y, int toff, float scale) {
    const int Cin = x.C, Cout = y.C, H = x.H, W = x.W, HW = H * W;
    const bool shortcut = Cin != Cout;
    const int64_t pn1w = add_param(pre + "norm1.weight", {Cin}), pn1b = add_param(pre + "norm1.bias", {Cin});
    const int64_t pc1w = add_param(pre + "conv1.weight", {Cout, Cin, 3, 3}, 1), pc1b = add_param(pre + "conv1.bias", {Cout});
    alias_param(pre + "time_emb_proj.weight", p_tw + (int64_t)toff * T, {Cout, T});
    alias_param(pre + "time_emb_proj.bias", p_tb + toff, {Cout});
    {   // this block's rows of the batched projection become final with this segment (resnets of a block are consecutive)
        const int64_t wlo = p_tw + (int64_t)toff * T, blo = p_tb + toff;
        segs[cur_seg].tw.cover(wlo, wlo + (int64_t)Cout * T);
        segs[cur_seg].tb.cover(blo, blo + Cout);
    }
    const int64_t pn2w = add_param(pre + "norm2.weight", {Cout}), pn2b = add_param(pre + "norm2.bias", {Cout});
    const int64_t pc2w = add_param(pre + "conv2.weight", {Cout, Cout, 3, 3}, 1), pc2b = add_param(pre + "conv2.bias", {Cout});
    const Conv3 k1 = conv3_same(pc1w, pc1b, Cin, Cout, H, W), k2 = conv3_same(pc2w, pc2b, Cout, Cout, H, W);
    Lin sc = {-1, -1, Cout, Cin};
    if (shortcut) {
        sc.pw = add_param(pre + "conv_shortcut.weight", {Cout, Cin, 1, 1}, 1);
        sc.pb = add_param(pre + "conv_shortcut.bias", {Cout});
    }
    if (Cin % 32 == 0 && Cout % 32 == 0) {
        wt_off.push_back(pc1w); wt_cin.push_back(Cin); wt_cout.push_back(Cout);
        wt_off.push_back(pc2w); wt_cin.push_back(Cout); wt_cout.push_back(Cout);
    }
    const int b_a1 = new_buf((int64_t)HW * Cin, 0, R_VALUE), b_h1 = new_buf((int64_t)HW * Cout, 0, R_VALUE);
    const int b_a2 = new_buf((int64_t)HW * Cout, 0, R_VALUE);
    // split-plane twins of a1 / a2 (operands of the LDS-DMA convolutions; 4 B per element like fp32)
    const int b_a1s = new_buf((int64_t)HW * Cin, 0, R_VALUE), b_a2s = new_buf((int64_t)HW * Cout, 0, R_VALUE);
    const int G = cfg.norm_num_groups;
    const int b_st1 = new_buf(2 * G, 0, R_VALUE), b_st2 = new_buf(2 * G, 0, R_VALUE);
    View h1v; h1v.buf = b_h1; h1v.coff = 0; h1v.C = Cout; h1v.ld = Cout; h1v.H = H; h1v.W = W;
    bufs[b_h1].gbuf = -1;
    const int b_dys = scale != 1.f ? scratch((int64_t)HW * Cout) : -1;
    const int b_da2 = scratch((int64_t)HW * Cout), b_dh1 = scratch((int64_t)HW * Cout);
    const int b_da1 = scratch((int64_t)HW * Cin);
    // backward operands of the LDS-DMA data gradients: dy / dh1 as split planes, transposed weight planes
    const int b_dyS = scratch((int64_t)HW * Cout), b_dh1S = scratch((int64_t)HW * Cout);
    const float inv = 1.f / scale;
    const int sumC_ = sumC;
    // the family of conv1 / conv2, and of the shortcut's data gradient: dL/dy exists as split planes whenever conv2 took the plane kernels, and
    // the 1x1 then runs DMA-fed on them instead of splitting both fp32 operands in the igemm loaders
    const Path ps1 = [=](int B) { return ps_shape(B, H, W, Cin, Cout); }, ps2 = [=](int B) { return ps_shape(B, H, W, Cout, Cout); };
    const Path sc_sp = [=](int B) {
        return Knobs::get().shortcut_sp && ps2(B) && gemm_sp_supported((int)((int64_t)B * HW), Cin, Cout) && x.ld % 4 == 0;
    };
    // dL/dx becomes final in this node's norm1 backward (first consumer of x in forward order); dL/dy arrives ready-split when y's first
    // consumer can do the same for us (GSplit)
    const int gs_in = claim_gsplit(x, true);
    const int gs_out = b_dys < 0 ? reg_gsplit(y, ps2) : -1;

    F([=](Ctx& c) {
        const bool p1 = takes(c, ps1), p2 = takes(c, ps2);
        // a1 / a2 in the format their convolution reads (planes: conv1 / conv2 forward and, they are value buffers, the weight gradients)
        float* a1 = BP(c, p1 ? b_a1s : b_a1);
        float* a2 = BP(c, p2 ? b_a2s : b_a2);
        BD_TRY(gn_fwd(c, x, pn1w, pn1b, a1, Cin, b_st1, 1, p1));
        Conv3Epi e1;
        e1.rowbias = BP(c, b_tproj) + toff; e1.ld_rowbias = sumC_;
        // round 4: norm2's statistics from conv1's epilogue when norm2 would otherwise make a pass over h1 for them (large images)
        if (p1 && p2) e1.gn_splits = conv3_gn_splits(c, k1);
        BD_TRY(conv3_fwd(c, k1, p1, {a1, Cin}, BP(c, b_h1), Cout, e1));
        BD_TRY(gn_fwd(c, h1v, pn2w, pn2b, a2, Cout, b_st2, 1, p2, e1.gn_splits));
        Conv3Epi e2;
        e2.residual = VP(c, x); e2.ldr = x.ld; e2.out_scale = inv;
        if (shortcut) {
            BD_TRY(lin_fwd(c, sc, false, {VP(c, x), x.ld}, VP(c, y), y.ld, (int)rows(c, x)));
            e2.residual = VP(c, y); e2.ldr = y.ld;
        }
        return conv3_fwd(c, k2, p2, {a2, Cout}, VP(c, y), y.ld, e2);
    });
    Bk([=](Ctx& c) {
        const int M = (int)rows(c, x);
        Opnd dy = {GP(c, y), y.ld};
        if (b_dys >= 0) {
            BD_TRY(add(c, dy.p, dy.ld, BP(c, b_dys), Cout, M, Cout, inv, 0));
            dy = {BP(c, b_dys), Cout};
        }
        const bool p1 = takes(c, ps1), p2 = takes(c, ps2);
        Opnd dy2 = dy;      // dL/dy as conv2's family reads it
        if (p2) BD_TRY(grad_planes(c, gs_out, dy.p, dy.ld, M, Cout, b_dyS, dy2));
        BD_TRY(conv3_wgrad(c, k2, p2, {BP(c, p2 ? b_a2s : b_a2), Cout}, dy2));
        BD_TRY(conv3_dgrad(c, k2, p2, dy2, BP(c, b_da2), Cout, 0));
        float* dh1 = BP(c, p1 ? b_dh1S : b_dh1);
        {   // norm2 backward: dh1 = gn_silu_bwd(h1, da2), in conv1's family   (h1 has no persistent grad buffer: write to scratch)
            bd_gn_bwd_desc d = {};
            d.lddx = Cout;
            if (p1) { d.dx_split = U16(dh1); d.lddxs = Cout; }
            else d.dx = dh1;
            // time-embedding gradient = per-sample column sums of dh1, out of the same launch (its weight gradient: temb_wgrad, per segment)
            d.dx_colsum = BP(c, b_dtproj) + toff; d.ld_colsum = sumC_;
            BD_TRY(gn_bwd(c, d, h1v, pn2w, pn2b, b_st2, BP(c, b_da2), Cout, 1));
        }
        BD_TRY(conv3_wgrad(c, k1, p1, {BP(c, p1 ? b_a1s : b_a1), Cin}, {dh1, Cout}));
        BD_TRY(conv3_dgrad(c, k1, p1, {dh1, Cout}, BP(c, b_da1), Cin, 0));
        if (shortcut) {   // 1x1 shortcut convolution: its data gradient goes in FIRST, so that the norm1 backward below is the store that makes
            // dL/dx final (and can hand x's producer the split planes of it)
            BD_TRY(lin_wgrad(c, sc, false, dy, {VP(c, x), x.ld}, M));
            const bool sp = takes(c, sc_sp);
            BD_TRY(lin_dgrad(c, sc, sp, sp ? dy2 : dy, GP(c, x), x.ld, M, take_ginit(c, x.buf)));
        }
        // norm1 backward; the identity shortcut's gradient (dy itself) is added in the same store
        return gn_bwd(c, x, pn1w, pn1b, b_st1, BP(c, b_da1), Cin, 1, shortcut ? nullptr : dy.p, dy.ld, gs_in);
    });
}

void bd_unet::node_attention(const std::string& pre, const View& x, const View& y, float scale) {
    const int C = x.C, H = x.H, W = x.W, N = H * W;
    const int heads = cfg.attention_head_dim > 0 ? C / cfg.attention_head_dim : 1;
    const int dh = C / heads;
    const int64_t pgw = add_param(pre + "group_norm.weight", {C}), pgb = add_param(pre + "group_norm.bias", {C});
    // query / key / value are one [3C, C] projection: their weights, then their biases, are adjacent in the flat buffer
    const int64_t pqw = add_param(pre + "query.weight", {C, C});
    add_param(pre + "key.weight", {C, C});
    add_param(pre + "value.weight", {C, C});
    const int64_t pqb = add_param(pre + "query.bias", {C});
    add_param(pre + "key.bias", {C});
    add_param(pre + "value.bias", {C});
    const Lin qkv = {pqw, pqb, 3 * C, C};
    const Lin proj = {add_param(pre + "proj_attn.weight", {C, C}), add_param(pre + "proj_attn.bias", {C}), C, C};
    const int G = cfg.norm_num_groups;
    const int b_n = new_buf((int64_t)N * C, 0, R_VALUE), b_qkv = new_buf((int64_t)N * 3 * C, 0, R_VALUE);
    const int b_p = new_buf((int64_t)heads * N * N, 0, R_VALUE), b_o = new_buf((int64_t)N * C, 0, R_VALUE);
    const int b_st = new_buf(2 * G, 0, R_VALUE);
    const int b_dys = scale != 1.f ? scratch((int64_t)N * C) : -1;
    const int b_do = scratch((int64_t)N * C), b_dp = scratch((int64_t)heads * N * N);
    const int b_dqkv = scratch((int64_t)N * 3 * C), b_dn = scratch((int64_t)N * C);
    const int b_dyS = scratch((int64_t)N * C);
    const float inv = 1.f / scale;
    const Attn at = {heads, N, dh, C, 1.0f / std::sqrt((float)C / (float)heads), b_qkv, b_p, b_o, b_do, b_dp, b_dqkv};
    // Round 3: the whole block on SPLIT PLANES (gemm_sp.hip + attn_sp.hip): GroupNorm writes planes, the QKV projection reads and writes
    // planes, the attention core keeps the [N, N] matrices on chip and hands planes to the output projection; the backward mirrors it.  The
    // same buffers hold planes instead of fp32 (same bytes).  N = 256 tokens, head dim 256 (attn_sp_supported); the mid block (4 x 4) and
    // head dim 512 stay on the fp32 family.
    const Path sp_at = [=](int B) {
        return mode_bf16(cfg.compute_mode) && attn_sp_supported(N, dh) && gemm_sp_supported((int)((int64_t)B * N), C, C) &&
               gemm_sp_supported(3 * C, C, 32);
    };
    const int gs_in = claim_gsplit(x, true);
    const int gs_out = b_dys < 0 ? reg_gsplit(y, sp_at) : -1;
    F([=](Ctx& c) {
        const int M = (int)rows(c, x);
        const bool sp = takes(c, sp_at);
        BD_TRY(gn_fwd(c, x, pgw, pgb, BP(c, b_n), C, b_st, 0, sp));
        BD_TRY(lin_fwd(c, qkv, sp, {BP(c, b_n), C}, BP(c, b_qkv), 3 * C, M, sp));
        BD_TRY(attn_fwd(c, at, sp));
        LinEpi e;      // y = (o Wp^T + b + x) / scale
        e.residual = VP(c, x); e.ldr = x.ld; e.out_scale = inv;
        return lin_fwd(c, proj, sp, {BP(c, b_o), C}, VP(c, y), y.ld, M, false, e);
    });
    Bk([=](Ctx& c) {
        const int M = (int)rows(c, x);
        const bool sp = takes(c, sp_at);
        Opnd dy = {GP(c, y), y.ld};
        if (b_dys >= 0) {
            BD_TRY(add(c, dy.p, dy.ld, BP(c, b_dys), C, M, C, inv, 0));
            dy = {BP(c, b_dys), C};
        }
        Opnd dyf = dy;      // dL/dy as the family reads it
        if (sp) BD_TRY(grad_planes(c, gs_out, dy.p, dy.ld, M, C, b_dyS, dyf));
        BD_TRY(lin_wgrad(c, proj, sp, dyf, {BP(c, b_o), C}, M));
        BD_TRY(lin_dgrad(c, proj, sp, dyf, BP(c, b_do), C, M, 0, sp));
        BD_TRY(attn_bwd(c, at, sp));
        const Opnd dqkv = {BP(c, b_dqkv), 3 * C};
        BD_TRY(lin_wgrad(c, qkv, sp, dqkv, {BP(c, b_n), C}, M));
        BD_TRY(lin_dgrad(c, qkv, sp, dqkv, BP(c, b_dn), C, M, 0));
        // group-norm backward; the residual connection's gradient (dy itself, fp32) is added in the same store
        return gn_bwd(c, x, pgw, pgb, b_st, BP(c, b_dn), C, 0, dy.p, dy.ld, gs_in);
    });
}

void bd_unet::node_downsample(const std::string& pre, const View& x, const View& y) {
    const int C = x.C, H = x.H, W = x.W, Ho = y.H, Wo = y.W;
    const int pad = cfg.downsample_padding ? 1 : 0;
    const int64_t pw = add_param(pre + "conv.weight", {C, C, 3, 3}, 1), pb = add_param(pre + "conv.bias", {C});
    if (C % 32 == 0) { wt_off.push_back(pw); wt_cin.push_back(C); wt_cout.push_back(C); }   // transposed planes for the phase data gradient
    Conv3 k = conv3_same(pw, pb, C, C, H, W);
    k.stride = 2; k.pad = pad; k.Ho = Ho; k.Wo = Wo;
    const int b_dyS = scratch((int64_t)Ho * Wo * C);
    claim_gsplit(x, false);        // (this node's data gradient is a convolution: it cannot leave dL/dx as planes)
    // by the parity of the input pixel only 4 / 2 / 2 / 1 of the nine taps contribute to the data gradient: four classes on the output grid
    const Path phase = [=](int B) { return H == 2 * Ho && W == 2 * Wo && phase_shape(B, Ho, Wo, C, C); };
    const int gs_out = reg_gsplit(y, phase);
    F([=](Ctx& c) { return conv3_fwd(c, k, false, {VP(c, x), x.ld}, VP(c, y), y.ld); });
    Bk([=](Ctx& c) {
        const Opnd dy = {GP(c, y), y.ld};
        BD_TRY(conv3_wgrad(c, k, false, {VP(c, x), x.ld}, dy));
        const int acc = take_ginit(c, x.buf);
        if (!takes(c, phase)) return conv3_dgrad(c, k, false, dy, GP(c, x), x.ld, acc);
        Opnd dyS;
        BD_TRY(grad_planes(c, gs_out, dy.p, dy.ld, (int64_t)c.B * Ho * Wo, C, b_dyS, dyS));
        return phase_s2_dgrad(c, k, dyS, GP(c, x), x.ld, acc);
    });
}

void bd_unet::node_upsample(const std::string& pre, const View& x, const View& y) {
    const int C = x.C, H = x.H, W = x.W;
    const int64_t pw = add_param(pre + "conv.weight", {C, C, 3, 3}, 1), pb = add_param(pre + "conv.bias", {C});
    if (C % 32 == 0) { wt_off.push_back(pw); wt_cin.push_back(C); wt_cout.push_back(C); }
    Conv3 k = conv3_same(pw, pb, C, C, H, W);
    k.ups = 1; k.Ho = 2 * H; k.Wo = 2 * W;
    const int b_du = scratch((int64_t)4 * H * W * C);
    // LDS-DMA path: the nearest-upsampled input is materialised ONCE as split planes (4 B per element of the 2H x 2W
    // grid) and feeds the stride-1 "same" kernels of conv_ps.hip: forward, weight gradient and (through b_du + 2x2 sums)
    // the data gradient.  Otherwise the upsampling stays folded into the igemm gather.
    const int b_xuS = new_buf((int64_t)4 * H * W * C, 0, R_VALUE), b_dyS = scratch((int64_t)4 * H * W * C);
    // phase-decomposed path (round 3): x as split planes on the SOURCE grid + the pre-summed tap planes E / E^T of this layer
    const int b_xS = new_buf((int64_t)H * W * C, 0, R_VALUE);
    const int b_e = new_buf(0, (int64_t)16 * C * C, R_VALUE), b_et = new_buf(0, (int64_t)16 * C * C, R_VALUE);
    // the plan's path choice: phase form; else the plane kernels on the materialised fine grid; else the literal form.  The phase form's data
    // gradient is one class on the source grid where that pays (phase_dgrad_shape), else the fine-grid data gradient + 2x2 sums on planes
    const Path phase = [=](int B) { return phase_shape(B, H, W, C, C); };
    const Path fine_ps = [=](int B) { return !phase(B) && ps_shape(B, 2 * H, 2 * W, C, C); };
    const Path phase_d = [=](int B) { return phase(B) && phase_dgrad_shape(B, H, W, C); };
    if (C % 128 == 0) upsw.push_back({pw, C, phase, b_e, b_et});
    claim_gsplit(x, false);
    const int gs_out = reg_gsplit(y, [=](int B) { return phase(B) || fine_ps(B); });
    // which of the two operand sets exists
    bufs[b_xuS].live = [=](int B, int) { return fine_ps(B); };
    bufs[b_xS].live = [=](int B, int) { return phase(B); };
    bufs[b_e].live = [=](int B, int) { return phase(B); };
    bufs[b_et].live = [=](int B, int training) { return training && phase(B); };
    F([=](Ctx& c) {
        if (takes(c, phase)) {
            BD_TRY(split_rows(c, VP(c, x), x.ld, (int64_t)c.B * H * W, C, BP(c, b_xS)));
            return phase_ups_fwd(c, k, {BP(c, b_xS), C}, BP(c, b_e), VP(c, y), y.ld);
        }
        const bool ps = takes(c, fine_ps);
        if (ps) BD_TRY(split_rows_ups2(c, VP(c, x), x.ld, H, W, C, BP(c, b_xuS)));
        return conv3_fwd(c, k, ps, ps ? Opnd{BP(c, b_xuS), C} : Opnd{VP(c, x), x.ld}, VP(c, y), y.ld);
    });
    Bk([=](Ctx& c) {
        Opnd dy = {GP(c, y), y.ld};
        const int acc = take_ginit(c, x.buf);
        const bool ph = takes(c, phase);
        const bool ps = ph || takes(c, fine_ps);      // family of the fine-grid data gradient
        if (ps) BD_TRY(grad_planes(c, gs_out, dy.p, dy.ld, (int64_t)c.B * 4 * H * W, C, b_dyS, dy));
        if (ph) BD_TRY(phase_ups_wgrad(c, k, {BP(c, b_xS), C}, dy));
        else BD_TRY(conv3_wgrad(c, k, ps, ps ? Opnd{BP(c, b_xuS), C} : Opnd{VP(c, x), x.ld}, dy));
        if (takes(c, phase_d)) return phase_ups_dgrad(c, k, dy, BP(c, b_et), GP(c, x), x.ld, acc);
        // data gradient on the fine grid + 2x2 sums
        BD_TRY(conv3_dgrad(c, k, ps, dy, BP(c, b_du), C, 0));
        return sum2x2(c, BP(c, b_du), C, GP(c, x), x.ld, H, W, C, acc);
    });
}

void bd_unet::node_conv_out(const View& x) {
    const int C = x.C, H = x.H, W = x.W, Co = cfg.out_channels;
    const int64_t pnw = add_param("conv_norm_out.weight", {C}), pnb = add_param("conv_norm_out.bias", {C});
    const int64_t pw = add_param("conv_out.weight", {Co, C, 3, 3}, 1), pb = add_param("conv_out.bias", {Co});
    const Conv3 k = conv3_same(pw, pb, C, Co, H, W);
    const int G = cfg.norm_num_groups;
    const int b_a = new_buf((int64_t)H * W * C, 0, R_VALUE), b_st = new_buf(2 * G, 0, R_VALUE);
    const int b_bs = scratch(Co), b_da = scratch((int64_t)H * W * C);
    const int gs_in = claim_gsplit(x, true);
    F([=](Ctx& c) {
        BD_TRY(gn_fwd(c, x, pnw, pnb, BP(c, b_a), C, b_st, 1));
        return conv3_fwd(c, k, false, {BP(c, b_a), C}, c.out, c.ldo);
    });
    Bk([=](Ctx& c) {
        const Opnd dy = {c.dout, c.lddo};
        BD_TRY(conv3_wgrad(c, k, false, {BP(c, b_a), C}, dy, b_bs));
        BD_TRY(conv3_dgrad(c, k, false, dy, BP(c, b_da), C, 0));
        return gn_bwd(c, x, pnw, pnb, b_st, BP(c, b_da), C, 1, nullptr, 0, gs_in);
    });
}

// ----------------------------------------------------------------------------------------------------
void bd_unet::build() {
    const int n = cfg.num_blocks, L = cfg.layers_per_block, S0 = cfg.sample_size;
    const int* boc = cfg.block_out_channels;
    T = 4 * boc[0];
    // ---- pass 1: architecture enumeration -----------------------------------------------------------
    // skips (down path outputs, in push order) and up resnets (pop order)
    struct Skip { int C, H; };
    std::vector<Skip> skips;
    skips.push_back({boc[0], S0});
    {
        int res = S0;
        for (int i = 0; i < n; ++i) {
            for (int j = 0; j < L; ++j) skips.push_back({boc[i], res});
            if (i != n - 1) { res /= 2; skips.push_back({boc[i], res}); }
        }
    }
    struct UpRes { int C1, C2, Cout, H; };
    std::vector<std::vector<UpRes>> ups(n);
    {
        int sk = (int)skips.size();
        int res = S0 >> (n - 1);
        for (int i = 0; i < n; ++i) {
            const int out = boc[n - 1 - i];
            const int prev = i == 0 ? boc[n - 1] : boc[n - i];
            for (int j = 0; j <= L; ++j) {
                const Skip& s = skips[--sk];
                ups[i].push_back({j == 0 ? prev : out, s.C, out, res});
            }
            if (i != n - 1) res *= 2;
        }
    }
    // total time_emb_proj rows, in forward order: down resnets, mid x2, up resnets
    sumC = 0;
    for (int i = 0; i < n; ++i) sumC += L * boc[i];
    sumC += 2 * boc[n - 1];
    for (int i = 0; i < n; ++i) for (auto& u : ups[i]) sumC += u.Cout;

    // segments in BACKWARD order: 0 = out, 1..n = up blocks n-1..0, n+1 = mid, n+2..2n+1 = down n-1..0, 2n+2 = conv_in, 2n+3 = time
    const int nseg = 2 * n + 4;
    segs.assign(nseg, Seg());
    const int seg_out = 0;
    auto seg_up = [&](int i) { return 1 + (n - 1 - i); };
    const int seg_mid = n + 1;
    auto seg_down = [&](int i) { return n + 2 + (n - 1 - i); };
    const int seg_in = 2 * n + 2, seg_time = 2 * n + 3;

    // concat buffers, one per up resnet
    std::vector<std::vector<View>> cat(n);
    for (int i = 0; i < n; ++i)
        for (auto& u : ups[i]) {
            View v = new_tensor(u.H, u.H, u.C1 + u.C2);
            cat[i].push_back(v);
        }
    // skip k lives in the concat buffer of the up resnet that pops it
    std::vector<View> skipv(skips.size());
    {
        int sk = (int)skips.size();
        for (int i = 0; i < n; ++i)
            for (size_t j = 0; j < ups[i].size(); ++j) {
                --sk;
                skipv[sk] = slice(cat[i][j], ups[i][j].C1, ups[i][j].C2);
            }
    }

    // ---- pass 2: nodes in forward order ---------------------------------------------------------------
    cur_group = 0;
    cur_seg = seg_time; segs[seg_time].own.lo = 0;
    node_time_embed();
    int toff = 0, group = 1;
    cur_seg = seg_in; cur_group = group++;
    node_conv_in(skipv[0]);
    int sk = 1;
    View h = skipv[0];
    int res = S0;
    for (int i = 0; i < n; ++i) {
        cur_seg = seg_down(i);
        const std::string bp = "down_blocks." + std::to_string(i) + ".";
        for (int j = 0; j < L; ++j) {
            cur_group = group++;
            View dst = skipv[sk];
            if (cfg.down_attn[i]) {
                View mid = new_tensor(res, res, boc[i]);
                node_resnet(bp + "resnets." + std::to_string(j) + ".", h, mid, toff, 1.f);
                cur_group = group++;
                node_attention(bp + "attentions." + std::to_string(j) + ".", mid, dst, 1.f);
            } else {
                node_resnet(bp + "resnets." + std::to_string(j) + ".", h, dst, toff, 1.f);
            }
            toff += boc[i];
            h = dst; ++sk;
        }
        if (i != n - 1) {
            cur_group = group++;
            View dst = skipv[sk];
            node_downsample(bp + "downsamplers.0.", h, dst);
            h = dst; ++sk; res /= 2;
        }
    }
    {   // mid block
        cur_seg = seg_mid;
        const int C = boc[n - 1];
        const float s = cfg.mid_block_scale_factor;
        View m1 = new_tensor(res, res, C), m2 = new_tensor(res, res, C);
        View dst = slice(cat[0][0], 0, ups[0][0].C1);
        cur_group = group++;
        node_resnet("mid_block.resnets.0.", h, m1, toff, s); toff += C;
        cur_group = group++;
        node_attention("mid_block.attentions.0.", m1, m2, s);
        cur_group = group++;
        node_resnet("mid_block.resnets.1.", m2, dst, toff, s); toff += C;
    }
    View last;
    for (int i = 0; i < n; ++i) {
        cur_seg = seg_up(i);
        const std::string bp = "up_blocks." + std::to_string(i) + ".";
        const int nl = (int)ups[i].size();
        for (int j = 0; j < nl; ++j) {
            const UpRes& u = ups[i][j];
            // destination of this layer's output: next concat's h-slice, or a standalone tensor before upsample / out
            View dst;
            const bool last_layer = j == nl - 1;
            if (!last_layer) dst = slice(cat[i][j + 1], 0, ups[i][j + 1].C1);
            else dst = new_tensor(u.H, u.H, u.Cout);
            cur_group = group++;
            if (cfg.up_attn[i]) {
                View mid = new_tensor(u.H, u.H, u.Cout);
                node_resnet(bp + "resnets." + std::to_string(j) + ".", cat[i][j], mid, toff, 1.f);
                cur_group = group++;
                node_attention(bp + "attentions." + std::to_string(j) + ".", mid, dst, 1.f);
            } else {
                node_resnet(bp + "resnets." + std::to_string(j) + ".", cat[i][j], dst, toff, 1.f);
            }
            toff += u.Cout;
            last = dst;
        }
        if (i != n - 1) {
            cur_group = group++;
            View dst = slice(cat[i + 1][0], 0, ups[i + 1][0].C1);
            node_upsample(bp + "upsamplers.0.", last, dst);
        }
    }
    cur_seg = seg_out; cur_group = group++;
    node_conv_out(last);
    nparams = (nparams + 3) / 4 * 4;
}

void bd_unet::layout(int B, int training) {
    if (lay_B == B && lay_train == training && lay_gen == bd::g_tune_gen) return;
    auto al = [](int64_t x) { return (x + 63) / 64 * 64; };
    int64_t v = 0, g = 0;
    for (auto& b : bufs) if (b.region == R_VALUE) { b.off = v; if (!b.live || b.live(B, training)) v += al(b.per_sample * B + b.fixed); }
    value_floats = v;
    for (auto& b : bufs) if (b.region == R_GRAD) { b.off = v + g; if (!b.live || b.live(B, training)) g += al(b.per_sample * B + b.fixed); }
    grad_floats = training ? g : 0;
    const int64_t base = value_floats + grad_floats;
    int64_t smax = 0;
    for (int pass = 0; pass < 2; ++pass) {   // two arenas, chosen by node (group) parity: see Ctx::st2
        int cur = -1; int64_t s = 0;
        for (auto& b : bufs) if (b.region == R_SCRATCH) {
            if (b.group != cur) { cur = b.group; s = 0; }
            const int64_t n = al(b.per_sample * B + b.fixed);
            if (pass == 0) { if (s + n > smax) smax = s + n; }
            else b.off = base + (b.group & 1) * smax + s;
            s += n;
        }
    }
    scratch_floats = training ? 2 * smax : 0;
    // op workspace: dry-run every step
    Ctx c;
    c.dry = true; c.B = B; c.ws = nullptr; c.ginit.assign(bufs.size(), 0);
    c.opws_bytes = (size_t)1 << 62;
    for (auto& f : fwd) f(c);
    if (training) {
        for (auto it = bwd.rbegin(); it != bwd.rend(); ++it) it->fn(c);
        temb_wgrad(c, 0, sumC);      // (unet_backward_run launches it outside any step: at most all rows at once)
    }
    opws_bytes = align_up(c.opws_need, 256);
    gnpart_floats = training ? c.gnpart_need : 0;
    lay_B = B; lay_train = training; lay_gen = bd::g_tune_gen;
    forget_prepared();   // a new layout moves the prepared planes inside the workspace
}

// ----------------------------------------------------------------------------------------------------
extern "C" int bd_unet_create(const bd_unet_config* cfg, bd_unet** out) {
    BD_CHECK(cfg && out, BD_ERR_INVALID, "bd_unet_create: null argument");
    const int n = cfg->num_blocks;
    BD_CHECK(n >= 1 && n <= 8, BD_ERR_INVALID, "bd_unet_create: num_blocks %d out of range", n);
    BD_CHECK(cfg->layers_per_block >= 1, BD_ERR_INVALID, "bd_unet_create: layers_per_block");
    BD_CHECK(cfg->sample_size > 0 && (cfg->sample_size % (1 << (n - 1))) == 0, BD_ERR_INVALID,
             "bd_unet_create: sample_size %d not divisible by 2^%d", cfg->sample_size, n - 1);
    BD_CHECK(cfg->in_channels > 0 && cfg->out_channels > 0, BD_ERR_INVALID, "bd_unet_create: channels");
    BD_CHECK(cfg->norm_num_groups > 0, BD_ERR_INVALID, "bd_unet_create: norm_num_groups");
    for (int i = 0; i < n; ++i) {
        const int C = cfg->block_out_channels[i];
        BD_CHECK(C > 0 && C % cfg->norm_num_groups == 0 && C % 4 == 0, BD_ERR_UNSUPPORTED,
                 "bd_unet_create: block_out_channels[%d]=%d must be a multiple of norm_num_groups and of 4", i, C);
        if (cfg->attention_head_dim > 0 && (cfg->down_attn[i] || cfg->up_attn[n - 1 - i]))
            BD_CHECK(C % cfg->attention_head_dim == 0 && cfg->attention_head_dim % 4 == 0, BD_ERR_UNSUPPORTED,
                     "bd_unet_create: attention_head_dim %d must divide %d and be a multiple of 4", cfg->attention_head_dim, C);
    }
    BD_CHECK(cfg->mid_block_scale_factor != 0.f, BD_ERR_INVALID, "bd_unet_create: mid_block_scale_factor == 0");
    BD_CHECK(mode_valid(cfg->compute_mode), BD_ERR_INVALID, "bd_unet_create: compute_mode %d", cfg->compute_mode);
    bd_unet* u = new (std::nothrow) bd_unet();
    BD_CHECK(u, BD_ERR_INVALID, "bd_unet_create: out of host memory");
    u->cfg = *cfg;
    u->build();
    *out = u;
    return BD_OK;
}
extern "C" void bd_unet_destroy(bd_unet* u) {
    if (!u) return;
    if (u->aux_stream) {
        (void)hipStreamSynchronize(u->aux_stream);
        (void)hipEventDestroy(u->aux_ev_fork);
        (void)hipEventDestroy(u->aux_ev_join[0]);
        (void)hipEventDestroy(u->aux_ev_join[1]);
        (void)hipEventDestroy(u->aux_ev_seg);
        (void)hipStreamDestroy(u->aux_stream);
    }
    delete u;
}
extern "C" int bd_unet_set_aux_stream(bd_unet* u, int enabled) {
    BD_CHECK(u, BD_ERR_INVALID, "bd_unet_set_aux_stream: null plan");
    u->aux_enabled = enabled ? 1 : 0;
    return BD_OK;
}
extern "C" int bd_unet_set_deferred_join(bd_unet* u, int enabled) {
    BD_CHECK(u, BD_ERR_INVALID, "bd_unet_set_deferred_join: null plan");
    u->aux_defer = enabled ? 1 : 0;
    return BD_OK;
}
extern "C" int bd_unet_stream_wait_aux(bd_unet* u, bd_stream_t stream) {
    BD_CHECK(u, BD_ERR_INVALID, "bd_unet_stream_wait_aux: null plan");
    if (!u->aux_stream || !u->aux_ev_seg) return BD_OK;      // no side stream yet: nothing to wait for
    BD_HIP_TRY(hipStreamWaitEvent(S(stream), u->aux_ev_seg, 0));
    return BD_OK;
}
extern "C" int bd_unet_set_static_weights(bd_unet* u, int enabled) {
    BD_CHECK(u, BD_ERR_INVALID, "bd_unet_set_static_weights: null plan");
    u->static_weights = enabled ? 1 : 0;
    u->forget_prepared();     // turning it on or off always re-reads the weights once
    return BD_OK;
}
extern "C" int bd_unet_set_compute_mode(bd_unet* u, int mode) {
    BD_CHECK(u && mode_valid(mode), BD_ERR_INVALID, "bd_unet_set_compute_mode: bad arguments (mode %d)", mode);
    if (u->cfg.compute_mode != mode) {
        u->lay_B = -1;   // the op-workspace bound depends on which kernels the mode selects: lay out again
        u->forget_prepared();   // ... and the prepared weight planes belong to the old mode
    }
    u->cfg.compute_mode = mode;
    return BD_OK;
}
extern "C" int bd_unet_reset_static_cache(bd_unet* u) {
    BD_CHECK(u, BD_ERR_INVALID, "bd_unet_reset_static_cache: null plan");
    u->forget_prepared();
    return BD_OK;
}
extern "C" int64_t bd_unet_num_params(const bd_unet* u) { return u ? u->nparams : 0; }
extern "C" int bd_unet_num_tensors(const bd_unet* u) { return u ? (int)u->params.size() : 0; }
extern "C" int bd_unet_param_info(const bd_unet* u, int i, const char** name, int64_t* offset, int* rank, int64_t shape[4],
                                  int* layout) {
    BD_CHECK(u && i >= 0 && i < (int)u->params.size(), BD_ERR_INVALID, "bd_unet_param_info: index out of range");
    const Param& p = u->params[i];
    if (name) *name = p.name.c_str();
    if (offset) *offset = p.off;
    if (rank) *rank = p.rank;
    if (shape) for (int k = 0; k < 4; ++k) shape[k] = p.shape[k];
    if (layout) *layout = p.layout;
    return BD_OK;
}
// the pre-split copy of the weights (2 uint16 per parameter, whole 32-element blocks) lives behind the op workspace
static size_t wsplit_elems(const bd_unet* u) { return (size_t)(u->nparams / 32 * 32); }
static size_t wsplit_bytes(const bd_unet* u) { return align_up(wsplit_elems(u) * 2 * sizeof(uint16_t), 256); }

// The arena of one call, after layout(B, training): byte offsets of the regions behind the activation floats (which start at 0) and
// the size bd_unet_workspace_bytes reports.  The one place that knows the order of the regions.
struct Arena { size_t opws, w_split, wT_split, opws2, gnpart, total; };
static Arena unet_arena(const bd_unet* u) {
    const size_t fl = (size_t)(u->value_floats + u->grad_floats + u->scratch_floats) * sizeof(float);
    const size_t op = align_up(u->opws_bytes, 256);
    Arena a;
    a.opws = align_up(fl, 256);                // the main stream's op workspace
    a.w_split = a.opws + op;                   // pre-split copy of the weights (the bf16 modes)
    a.wT_split = a.w_split + wsplit_bytes(u);  // transposed conv-weight planes
    a.opws2 = a.wT_split + wsplit_bytes(u);    // the side stream's op workspace
    a.gnpart = a.opws2 + op;                   // GroupNorm parameter partials of one backward
    // the end of the last region plus up to 256 bytes of slack: fl is counted unrounded + 256 (layout() makes opws_bytes a multiple of 256)
    a.total = fl + u->opws_bytes + 256 + 2 * wsplit_bytes(u) + op + align_up(u->gnpart_floats * sizeof(float), 256);
    return a;
}

extern "C" size_t bd_unet_workspace_bytes(bd_unet* u, int B, int training) {
    if (!u || B <= 0) return 0;
    u->layout(B, training);
    return unet_arena(u).total;
}

static int unet_ctx(bd_unet* u, Ctx& c, int B, int training, void* workspace, size_t workspace_bytes) {
    BD_CHECK(u, BD_ERR_INVALID, "bd_unet: null plan");
    BD_CHECK(B > 0, BD_ERR_INVALID, "bd_unet: B must be > 0");
    const size_t need = bd_unet_workspace_bytes(u, B, training);
    BD_CHECK(workspace && workspace_bytes >= need, BD_ERR_WORKSPACE, "bd_unet: workspace %zu < %zu bytes", workspace_bytes, need);
    BD_CHECK(aligned16(workspace), BD_ERR_INVALID, "bd_unet: workspace must be 16-byte aligned");
    c.B = B; c.LB = B;
    c.ws = reinterpret_cast<float*>(workspace);
    const Arena a = unet_arena(u);   // laid out by the size query above
    char* const base = reinterpret_cast<char*>(workspace);
    c.opws = base + a.opws;
    c.opws_bytes = u->opws_bytes;
    if (mode_bf16(u->cfg.compute_mode)) {
        c.w_split = reinterpret_cast<const uint16_t*>(base + a.w_split);
        c.wT_split = reinterpret_cast<const uint16_t*>(base + a.wT_split);
    }
    c.opws2 = base + a.opws2;
    c.gnpart = u->gnpart_floats ? reinterpret_cast<float*>(base + a.gnpart) : nullptr;
    c.gnpart_floats = u->gnpart_floats; c.gnpart_used = 0;
    c.ginit.assign(u->bufs.size(), 0);
    return BD_OK;
}

// the plan's side stream and its events, created on first use (plan creation stays host-only)
static int unet_aux_init(bd_unet* u) {
    if (u->aux_stream) return BD_OK;
    int lo = 0, hi = 0;
    BD_HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));   // lowest priority: in backward the dgrad chain is the critical path
    BD_HIP_TRY(hipStreamCreateWithPriority(&u->aux_stream, hipStreamNonBlocking, lo));
    BD_HIP_TRY(hipEventCreateWithFlags(&u->aux_ev_fork, hipEventDisableTiming));
    BD_HIP_TRY(hipEventCreateWithFlags(&u->aux_ev_join[0], hipEventDisableTiming));
    BD_HIP_TRY(hipEventCreateWithFlags(&u->aux_ev_join[1], hipEventDisableTiming));
    BD_HIP_TRY(hipEventCreateWithFlags(&u->aux_ev_seg, hipEventDisableTiming));
    return BD_OK;
}

// the forward of both entry points: the timesteps are int64 (t) or fp32 (tf), exactly one of the two; `who` names the entry point
static int unet_forward(const char* who, bd_unet* u, int B, int training, const float* params, const float* x, int64_t ldx,
                        const int64_t* t, const float* tf, int t_stride, float* out, int64_t ldo, void* workspace, size_t workspace_bytes,
                        bd_stream_t stream) {
    Ctx c;
    BD_TRY(unet_ctx(u, c, B, training, workspace, workspace_bytes));
    BD_CHECK(params && x && (t || tf) && out, BD_ERR_INVALID, "%s: null pointer", who);
    BD_CHECK(ldx >= u->cfg.in_channels && ldo >= u->cfg.out_channels, BD_ERR_INVALID, "%s: ld < channels", who);
    BD_CHECK(aligned16(params), BD_ERR_INVALID, "%s: params must be 16-byte aligned", who);
    c.params = params; c.x = x; c.ldx = ldx; c.t = t; c.tf = tf; c.t_stride = t_stride; c.out = out; c.ldo = ldo; c.st = S(stream);
    c.training = training != 0;
    if (training) { u->fwd_gen = bd::g_tune_gen; u->fwd_B = B; u->fwd_ws = workspace; }
    const bool prepared = u->static_weights && !training && u->prep_params == (const void*)params && u->prep_ws == workspace && u->prep_B == B;
    if (c.w_split && !prepared) {   // split the weights once; forward convs and (same workspace) the backward dgrads read the copy
        BD_TRY(bd_split_bf16(params, (int64_t)wsplit_elems(u), const_cast<uint16_t*>(c.w_split), stream));
        // pre-summed tap planes of the upsample convolutions that take the phase path (both forward pipelines read them: before
        // the fork); the transposed set E^T is the data gradient's operand: training only
        for (const auto& uw : u->upsw)
            if (u->takes(c, uw.phase))
                BD_TRY(upsample_weights(params + uw.pw, uw.C, uw.C, bd_unet::U16(u->BP(c, uw.b_e)),
                                        training ? bd_unet::U16(u->BP(c, uw.b_et)) : nullptr, c.st));
        u->prep_params = u->static_weights && !training ? (const void*)params : nullptr; u->prep_ws = workspace; u->prep_B = B;
    }
    // transposed split planes of the 3x3 conv weights for the backward's data gradients: one launch, needed only in training
    auto transpose_weights = [&](hipStream_t st) -> int {
        if (!training || !c.wT_split || u->wt_off.empty()) return BD_OK;
        return split_wt_batched(params, const_cast<uint16_t*>(c.wT_split), u->wt_off.data(), u->wt_cin.data(), u->wt_cout.data(),
                                (int)u->wt_off.size(), st);
    };
    // two pipelines need enough work per half to pay for twice the host enqueue: >= 32 K input pixels in the batch (B = 32 at 32 x 32 as
    // before; round 4: B = 4 at 256 x 256 qualifies too -- 29.05 -> 28.13 ms per 256 x 256 train step, small layers fill the chip in pairs)
    if (!u->aux_enabled || B < 2 || (long long)B * u->cfg.sample_size * u->cfg.sample_size < Knobs::get().fwd_pipes_minpx) {
        BD_TRY(transpose_weights(c.st));
        for (auto& f : u->fwd) BD_TRY(f(c));
        return BD_OK;
    }
    // Samples are independent all the way through the network (GroupNorm is per sample), so the batch runs as two
    // half-batch pipelines on the caller's stream and the plan's side stream, node by node: the prologues / epilogues
    // / small kernels of one half overlap the main loops of the other (+4 % on the CIFAR forward).  Same buffers, same
    // layout as a single pass -- backward does not know the difference.
    BD_TRY(unet_aux_init(u));
    Ctx c2 = c;
    const int Bh = B / 2;
    const int64_t hw = (int64_t)u->cfg.sample_size * u->cfg.sample_size;
    c.B = Bh;
    c2.B = B - Bh; c2.s0 = Bh; c2.st = u->aux_stream; c2.opws = c.opws2;
    c2.x = x + (int64_t)Bh * hw * ldx; c2.out = out + (int64_t)Bh * hw * ldo;
    c2.t = t ? t + (int64_t)Bh * t_stride : nullptr; c2.tf = tf ? tf + (int64_t)Bh * t_stride : nullptr;
    BD_HIP_TRY(hipEventRecord(u->aux_ev_fork, c.st));
    BD_HIP_TRY(hipStreamWaitEvent(c2.st, u->aux_ev_fork, 0));
    BD_TRY(transpose_weights(c2.st));   // memory-bound, off the first pipeline's critical path
    for (auto& f : u->fwd) {
        BD_TRY(f(c));
        BD_TRY(f(c2));
    }
    BD_HIP_TRY(hipEventRecord(u->aux_ev_join[0], c2.st));
    BD_HIP_TRY(hipStreamWaitEvent(c.st, u->aux_ev_join[0], 0));
    return BD_OK;
}

extern "C" int bd_unet_forward(bd_unet* u, int B, int training, const float* params, const float* x, int64_t ldx,
                               const int64_t* t, int t_stride, float* out, int64_t ldo, void* workspace, size_t workspace_bytes,
                               bd_stream_t stream) {
    return unet_forward("bd_unet_forward", u, B, training, params, x, ldx, t, nullptr, t_stride, out, ldo, workspace, workspace_bytes, stream);
}
extern "C" int bd_unet_forward_tf(bd_unet* u, int B, int training, const float* params, const float* x, int64_t ldx,
                                  const float* t, int t_stride, float* out, int64_t ldo, void* workspace, size_t workspace_bytes,
                                  bd_stream_t stream) {
    return unet_forward("bd_unet_forward_tf", u, B, training, params, x, ldx, nullptr, t, t_stride, out, ldo, workspace, workspace_bytes, stream);
}

extern "C" int bd_unet_num_segments(const bd_unet* u) { return u ? (int)u->segs.size() : 0; }
extern "C" int bd_unet_segment_num_ranges(const bd_unet* u, int seg) {
    if (!u || seg < 0 || seg >= (int)u->segs.size()) return 0;
    return u->segs[seg].tw.lo >= 0 ? 3 : 1;
}
extern "C" int bd_unet_segment_range_k(const bd_unet* u, int seg, int k, int64_t* lo, int64_t* hi) {
    BD_CHECK(u && seg >= 0 && seg < (int)u->segs.size() && k >= 0 && k < bd_unet_segment_num_ranges(u, seg), BD_ERR_INVALID,
             "bd_unet_segment_range_k: segment / range out of range");
    const bd_unet::Seg& s = u->segs[seg];
    const bd_unet::Range& r = k == 0 ? s.own : (k == 1 ? s.tw : s.tb);
    if (lo) *lo = r.lo;
    if (hi) *hi = r.hi;
    return BD_OK;
}
extern "C" int bd_unet_segment_range(const bd_unet* u, int seg, int64_t* lo, int64_t* hi) {
    BD_CHECK(u && seg >= 0 && seg < (int)u->segs.size(), BD_ERR_INVALID, "bd_unet_segment_range: segment out of range");
    return bd_unet_segment_range_k(u, seg, 0, lo, hi);
}

// the backward behind bd_unet_backward[_segment] (need_grads, dx == NULL) and bd_unet_backward_input (dx != NULL; grads == NULL selects the
// data-gradient-only schedule, Ctx::wg)
static int unet_backward_run(bd_unet* u, int seg, int B, const float* params, const float* x, int64_t ldx, const float* dout, int64_t lddo,
                             float* grads, bool need_grads, float* dx, int64_t lddx, void* workspace, size_t workspace_bytes,
                             bd_stream_t stream, int64_t* ready_lo, int64_t* ready_hi) {
    Ctx c;
    // a tuning-knob change re-lays out the workspace lazily: never under the saved activations of a forward that already ran
    BD_CHECK(!u || u->fwd_ws != workspace || u->fwd_B != B || u->fwd_gen == bd::g_tune_gen, BD_ERR_INVALID,
             "bd_unet_backward: bd_tune_set was called between the training forward and its backward (the saved activations would move)");
    BD_TRY(unet_ctx(u, c, B, 1, workspace, workspace_bytes));
    BD_CHECK(params && x && dout && (grads || !need_grads), BD_ERR_INVALID, "bd_unet_backward: null pointer");
    BD_CHECK(aligned16(params) && aligned16(grads), BD_ERR_INVALID, "bd_unet_backward: params/grads must be 16-byte aligned");
    BD_CHECK(seg >= -1 && seg < (int)u->segs.size(), BD_ERR_INVALID, "bd_unet_backward: segment %d out of range", seg);
    c.params = params; c.grads = grads; c.dout = dout; c.lddo = lddo; c.st = S(stream);
    c.x = x; c.ldx = ldx;   // conv_in wgrad re-reads the forward input
    c.wg = grads != nullptr; c.dx = dx; c.lddx = lddx;
    const bool aux_on = u->aux_enabled && c.wg;      // without weight gradients there is nothing for the side stream
    // Deferred join (bd_unet_set_deferred_join, used by the data-parallel trainer): the weight gradients a segment puts on the side
    // stream may still be running when the call returns and while the NEXT segment's data-gradient chain runs; the caller orders
    // whatever consumes this segment's gradient ranges behind them with bd_unet_stream_wait_aux(plan, consumer_stream).  The
    // scratch-arena hazard is covered across calls by carrying the per-parity "pending" marks in the plan.  The last segment (and
    // a whole backward, seg == -1) always joins, so the caller's stream ends ordered after everything.
    const bool defer = aux_on && u->aux_defer && seg >= 0 && seg + 1 < (int)u->segs.size();
    if (!aux_on && !c.wg && u->aux_stream && (u->aux_pend[0] || u->aux_pend[1])) {
        // (same hazard as below, for a pass that forks nothing itself)
        BD_HIP_TRY(hipStreamWaitEvent(c.st, u->aux_ev_seg, 0));
        u->aux_pend[0] = u->aux_pend[1] = false;
    }
    if (aux_on) {
        BD_TRY(unet_aux_init(u));
        c.st2 = u->aux_stream; c.ev_fork = u->aux_ev_fork; c.ev_join[0] = u->aux_ev_join[0]; c.ev_join[1] = u->aux_ev_join[1];
        if (seg > 0 && u->aux_defer) { c.pend[0] = u->aux_pend[0]; c.pend[1] = u->aux_pend[1]; }
        else if (u->aux_pend[0] || u->aux_pend[1]) {
            // a pass that starts (seg 0 / whole backward) while marks of an earlier, unfinished pass are still set: its weight gradients
            // may still be reading the scratch arenas -- order this pass behind everything that pass put on the side stream
            BD_HIP_TRY(hipStreamWaitEvent(c.st, u->aux_ev_seg, 0));
            u->aux_pend[0] = u->aux_pend[1] = false;
        }
    }
    // grad-init flags must reflect everything executed before this segment: replay them (host-only)
    for (auto it = u->bwd.rbegin(); it != u->bwd.rend(); ++it) {
        if (seg >= 0 && it->seg > seg) break;
        const bool run = seg < 0 || it->seg == seg;
        const bool keep = c.dry;
        c.dry = !run;           // earlier segments: flags only
        const int par = it->group & 1;
        if (run) BD_TRY(bd_unet::aux_wait(c, par));   // this node reuses the scratch arena of parity `par`
        int s = it->fn(c);
        c.dry = keep;
        if (s != BD_OK) return s;
        if (run) BD_TRY(bd_unet::aux_mark(c, par));
    }
    if (!c.gn_items.empty()) BD_TRY(bd_gn_bwd_params(c.gn_items.data(), (int)c.gn_items.size(), c.B, (bd_stream_t)c.st));
    {   // time_emb_proj weight / bias gradient rows of the resnets that just ran
        bd_unet::Range r;
        for (int sg = 0; sg < (int)u->segs.size(); ++sg) {
            const bd_unet::Range& tb = u->segs[sg].tb;
            if ((seg < 0 || sg == seg) && tb.lo >= 0) r.cover(tb.lo - u->p_tb, tb.hi - u->p_tb);
        }
        if (r.lo >= 0) {
            BD_TRY(u->temb_wgrad(c, r.lo, r.hi));
            BD_TRY(bd_unet::aux_mark(c, 0));
        }
    }
    if (defer) {
        u->aux_pend[0] = c.pend[0]; u->aux_pend[1] = c.pend[1];
        BD_HIP_TRY(hipEventRecord(u->aux_ev_seg, c.st2));   // everything this (and every earlier) call put on the side stream
    } else {
        BD_TRY(bd_unet::aux_wait(c, 0));   // every weight gradient of this call is ordered before what the caller enqueues next
        BD_TRY(bd_unet::aux_wait(c, 1));
        u->aux_pend[0] = u->aux_pend[1] = false;
        if (c.st2) BD_HIP_TRY(hipEventRecord(u->aux_ev_seg, c.st2));
    }
    return seg >= 0 ? bd_unet_segment_range(u, seg, ready_lo, ready_hi) : (int)BD_OK;
}

extern "C" int bd_unet_backward_segment(bd_unet* u, int seg, int B, const float* params, const float* x, int64_t ldx,
                                        const float* dout, int64_t lddo, float* grads, void* workspace, size_t workspace_bytes,
                                        bd_stream_t stream, int64_t* ready_lo, int64_t* ready_hi) {
    return unet_backward_run(u, seg, B, params, x, ldx, dout, lddo, grads, true, nullptr, 0, workspace, workspace_bytes, stream, ready_lo,
                             ready_hi);
}

extern "C" int bd_unet_backward_input(bd_unet* u, int B, const float* params, const float* x, int64_t ldx, const float* dout,
                                      int64_t lddo, float* grads, float* dx, int64_t lddx, void* workspace, size_t workspace_bytes,
                                      bd_stream_t stream) {
    BD_CHECK(u, BD_ERR_INVALID, "bd_unet_backward_input: null plan");
    BD_CHECK(dx, BD_ERR_INVALID, "bd_unet_backward_input: dx is null (bd_unet_backward is the call without an input gradient)");
    BD_CHECK(lddx >= u->cfg.in_channels, BD_ERR_INVALID, "bd_unet_backward_input: lddx %lld < in_channels %d", (long long)lddx,
             u->cfg.in_channels);
    BD_CHECK(params && aligned16(params), BD_ERR_INVALID, "bd_unet_backward_input: params must be non-null and 16-byte aligned");
    return unet_backward_run(u, -1, B, params, x, ldx, dout, lddo, grads, false, dx, lddx, workspace, workspace_bytes, stream, nullptr,
                             nullptr);
}

extern "C" int bd_unet_backward(bd_unet* u, int B, const float* params, const float* x, int64_t ldx, const float* dout,
                                int64_t lddo, float* grads, void* workspace, size_t workspace_bytes, bd_stream_t stream) {
    return bd_unet_backward_segment(u, -1, B, params, x, ldx, dout, lddo, grads, workspace, workspace_bytes, stream, nullptr,
                                    nullptr);
}
