"""Case table, operands, window geometry, descriptors and fp64 references of the igemm dispatch tests (tests/test_igemm_plan_host.py checks
the table against bd_igemm_plan and proves the data rounding-free on the CPU; tests/test_igemm_dispatch.py runs the kernels on it).  Nothing
here touches a device: descriptors are filled from a geometry and base addresses, which the host test fakes.

A `Problem` is one GEMM-shaped launch of csrc/igemm.hip -- a DENSE product in one of four storage forms, or one direction of a 3x3
convolution with the operand kinds that csrc/conv.cpp fills -- together with what the engine is expected to decide for it when every
buffer is aligned: class, `fast`, `vec`, and for each forced K split (ksplit, chunks per slice, chunks of the last slice, second pass).
DESIGN.md "igemm dispatch" carries the same table; whoever retunes choose() / classify() moves the cases with it."""
import functools
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from tests.test_conv_ps_dispatch import _narrow, _quarters, _wide, rnd

F32, BF16X3, BF16 = 0, 1, 2
MODES = (F32, BF16X3, BF16)
MODE_SUFFIX = {F32: "", BF16X3: "_bf16x3", BF16: "_bf16"}
DENSE, CONV, TCONV, WGT = 0, 1, 2, 3
# enum bd_igemm_class and the profiler's name of each class
(GENERIC, CONV_FWD, CONV_DGRAD, CONV_WGRAD, GEMM_NT, GEMM_NN, GEMM_TN, CONV_FWD_WS, CONV_DGRAD_WS, CONV_WGRAD_SAME) = range(10)
PROF_NAME = ["generic", "conv_fwd", "conv_dgrad", "conv_wgrad", "gemm_nt", "gemm_nn", "gemm_tn", "conv_fwd", "conv_dgrad", "conv_wgrad"]
RED_NONE, RED_SCALAR, RED_VEC4, RED_VEC4_LANES8 = range(4)
TILES = (64, 128)
ALPHA, OUT_SCALE = 0.25, 0.5
EPILOGUES = ("plain", "full", "full+acc")
BK = 32
GUARD = 24          # rows in front of and behind every window: more than Ws + 1, so a wrong tap of the first or last pixel stays inside
GAP = 5             # rows between two batch entries

# ------------------------------------------------------------------------------------------------ the table
# forced split -> (ksplit, chunks per slice, chunks of the last slice, second pass when C, the residual and the workspace are aligned)
NO_SPLIT = (1, None, RED_NONE)
# id: M, N, K, (batch_outer, batch_inner), vec, fast, splits, why
GEMM_CASES = {
    "D1": (128, 128, 32, (1, 1), 1, 1, [NO_SPLIT], "one chunk; one 128 tile (grid of 1) / four 64 tiles; every wave FULL"),
    "D2": (192, 160, 72, (1, 1), 1, 1, [NO_SPLIT, (3, (3, 1, 1), RED_VEC4)],
           "FAST loaders with a ragged last chunk (8 of 32); partial tiles at both sizes, full and partial waves in one workgroup, 9 tiles"),
    "D3": (130, 131, 33, (1, 1), 0, 0, [NO_SPLIT, (2, (2, 1, 1), RED_SCALAR)],
           "nothing aligned: scalar generic loaders in all four forms; K tail of one element alone in the last slice; scalar second pass"),
    "D4": (128, 128, 1056, (1, 1), 1, 1, [(4, (4, 9, 6), RED_VEC4)], "odd cps, ragged last slice, reduce4<1>; the auto rule gives the same"),
    "D5": (128, 128, 2400, (1, 1), 1, 1, [(25, (25, 3, 3), RED_VEC4_LANES8)],
           "reduce4<8> with 25 slabs (lane 0 of a group sums 4, the others 3) and its a_colsum tail"),
    "D6": (96, 80, 40, (2, 3), 1, 1, [NO_SPLIT, (2, (2, 1, 1), RED_VEC4)],
           "batch_outer x batch_inner, four independent strides, B shared over the inner batch and per batch; slabs bz * ksplit + s"),
}
# the auto rule (ksplit 0, tile 0) on 256 CUs, host only: id -> (tile, ksplit, cps, last)
GEMM_AUTO = {"D4": (128, 4, 9, 6), "D5": (128, 9, 9, 3)}
# form: (A k-contiguous, B k-contiguous, class when fast)
FORMS = {"nt": (1, 1, GEMM_NT), "nn": (1, 0, GEMM_NN), "tn": (0, 0, GEMM_TN), "rc_kc": (0, 1, GENERIC)}

# id: B, Hs, Ws, Cin, Cout, stride, pad, ups, asym, {direction: splits}, why
CONV_CASES = {
    "C1": (2, 8, 8, 32, 64, 1, 1, 0, False, {}, "shift path of decode_pixel; conv_wgrad SAME class; dgrad with N = 32 in a 64 tile"),
    "C2": (3, 6, 10, 64, 32, 1, 1, 0, False, {"wgrad": [NO_SPLIT, (2, (2, 3, 3), RED_VEC4)]},
           "division path, non-square; M = 180 ragged; wgrad K = 180 pixels (last chunk 20) without and with a split"),
    "C3a": (2, 8, 8, 32, 32, 2, 0, 0, True, {}, "stride 2 with the folded (0,1,0,1) pad: parity predicate of TConvKC, non-SAME wgrad class"),
    "C3b": (2, 8, 8, 32, 32, 2, 1, 0, False, {}, "stride 2, pad 1"),
    "C4": (2, 4, 4, 32, 32, 1, 1, 1, False, {}, ">> ups in ConvKC / ConvRC; dgrad over the virtual 8x8 grid"),
    "C5a": (2, 5, 7, 36, 20, 1, 1, 0, False, {}, "C % 32 != 0, C % 4 == 0: generic loaders with vec = 1 (forward, dgrad)"),
    "C5b": (2, 5, 7, 5, 6, 1, 1, 0, False, {}, "C % 4 != 0: scalar generic loaders; M % 4 != 0 on the wgrad, so no db"),
    "C6": (2, 8, 8, 128, 64, 1, 1, 0, False, {"fwd": [(5, (5, 8, 4), RED_VEC4)], "dgrad": [(5, (5, 4, 2), RED_VEC4)]},
           "slices that begin inside a tap cycle: forward at taps 0, 8, 7, 6, 5, dgrad at taps 0, 4, 8, 3, 7"),
    "C7": (4, 16, 16, 32, 64, 1, 1, 0, False, {"wgrad": [(16, (16, 2, 2), RED_VEC4_LANES8)]},
           "reduce4<8> on a weight gradient with its db tail; ConvRCs under a split"),
}
DIRECTIONS = ("fwd", "dgrad", "wgrad")
PRESPLIT_CASES = ("C1", "C6")


def conv_out_hw(Hs, Ws, stride, pad, ups, asym):
    Hi, Wi = Hs << ups, Ws << ups
    extra = 1 if asym else 2 * pad
    return (Hi + extra - 3) // stride + 1, (Wi + extra - 3) // stride + 1


def opnd(kind, kc, rows, cols, **geo):
    """an operand as a 2-D matrix in memory ([rows][cols], cols contiguous) plus its kind and conv geometry"""
    return NS(kind=kind, kc=kc, rows=rows, cols=cols, geo=geo)


def gemm_problem(cid, form, shared_b=False):
    M, N, K, (nbo, nbi), vec, fast, splits, _ = GEMM_CASES[cid]
    akc, bkc, cls = FORMS[form]
    colsum = form == "tn" and M % 4 == 0 and nbo * nbi == 1
    return NS(key=("gemm", cid, form, shared_b), name=f"{cid}-{form}" + ("-sharedB" if shared_b else ""), M=M, N=N, K=K, nbo=nbo, nbi=nbi,
              a=opnd(DENSE, akc, M if akc else K, K if akc else M), b=opnd(DENSE, bkc, N if bkc else K, K if bkc else N),
              shared_b=shared_b, rpg=48, colsum=colsum, cls=cls if fast else GENERIC, vec=vec, fast=fast, splits=splits)


def conv_problem(cid, direction):
    B, Hs, Ws, Cin, Cout, stride, pad, ups, asym, splits, _ = CONV_CASES[cid]
    Ho, Wo = conv_out_hw(Hs, Ws, stride, pad, ups, asym)
    Hi, Wi = Hs << ups, Ws << ups
    p = 0 if asym else pad
    same = stride == 1 and ups == 0 and (Ho, Wo) == (Hs, Ws) and p <= 1
    if direction == "fwd":          # conv.cpp conv3x3_fwd
        a = opnd(CONV, 1, B * Hs * Ws, Cin, C=Cin, Hs=Hs, Ws=Ws, Ho=Ho, Wo=Wo, stride=stride, pad_t=p, pad_l=p, ups=ups)
        b = opnd(DENSE, 1, Cout, 9 * Cin, C=Cin)
        M, N, K, rpg, cls, fast = B * Ho * Wo, Cout, 9 * Cin, Ho * Wo, CONV_FWD, Cin % 32 == 0
    elif direction == "dgrad":      # conv3x3_dgrad: dx over the conv's own (virtual, upsampled) input grid
        a = opnd(TCONV, 1, B * Ho * Wo, Cout, C=Cout, Hs=Ho, Ws=Wo, Ho=Hi, Wo=Wi, stride=stride, pad_t=p, pad_l=p, ups=0)
        b = opnd(WGT, 0, Cout * 9, Cin, C=Cout)
        M, N, K, rpg, cls, fast = B * Hi * Wi, Cin, 9 * Cout, Hi * Wi, CONV_DGRAD, Cout % 32 == 0
    else:                           # conv3x3_wgrad: A = dy^T, a_colsum = db
        a = opnd(DENSE, 0, B * Ho * Wo, Cout)
        b = opnd(CONV, 0, B * Hs * Ws, Cin, C=Cin, Hs=Hs, Ws=Ws, Ho=Ho, Wo=Wo, stride=stride, pad_t=p, pad_l=p, ups=ups)
        # a row-contiguous CONV operand is FAST whenever float4 loads are allowed (C % 4 == 0): C5a is a fast wgrad
        M, N, K, rpg, cls, fast = Cout, 9 * Cin, B * Ho * Wo, 16, CONV_WGRAD_SAME if same else CONV_WGRAD, Cin % 4 == 0 and Cout % 4 == 0
    vec = int(Cin % 4 == 0 and Cout % 4 == 0)
    return NS(key=("conv", cid, direction), name=f"{cid}-{direction}", M=M, N=N, K=K, nbo=1, nbi=1, a=a, b=b, shared_b=False, rpg=rpg,
              colsum=direction == "wgrad" and M % 4 == 0, cls=cls if fast else GENERIC, vec=vec, fast=int(fast),
              splits=splits.get(direction, [NO_SPLIT]))


def all_problems():
    out = [gemm_problem(cid, form) for cid in GEMM_CASES for form in FORMS]
    out += [gemm_problem("D6", form, shared_b=True) for form in FORMS]
    out += [conv_problem(cid, d) for cid in CONV_CASES for d in DIRECTIONS]
    return out


# ------------------------------------------------------------------------------------------------ the split rule and the expected plan
def split_rule(M, N, K, nb, tile, ksplit, cus=256):
    """choose() of igemm.hip -> (tile, ksplit, chunks per slice, chunks of the last slice); tile / ksplit 0 = the auto rules"""
    cdiv = lambda a, b: -(-a // b)
    tile = tile or (128 if M >= 128 and N >= 128 else 64)
    nchunks = cdiv(K, BK)
    ks = ksplit
    if ks <= 0:
        tiles = cdiv(M, tile) * cdiv(N, tile) * nb
        ks = 1
        if tiles < 256:
            slots = 3 * cus // 2
            ks = min(max(slots // tiles, 1), max(1, nchunks // 8), 128)
    ks = max(1, min(ks, nchunks))
    cps = cdiv(nchunks, ks)
    ks = cdiv(nchunks, cps)
    return tile, ks, cps, nchunks - (ks - 1) * cps


def resolve_split(pr, split):
    """a table entry -> (forced ksplit, ksplit, cps, last, aligned second pass)"""
    forced, kcl, red = split
    nchunks = -(-pr.K // BK)
    return (forced,) + (kcl if kcl else (1, nchunks, nchunks)) + (red,)


def workspace_bytes(pr, ksplit, colsum):
    return (pr.nbo * pr.nbi * ksplit * pr.M * pr.N + (ksplit * pr.M if colsum else 0)) * 4 if ksplit > 1 else 0


def expected_plan(pr, layout, tile, mode, split, presplit=False):
    """what bd_igemm_plan must report.  Layout "mis": A sits one float off (tile 64) or B has an odd ld (tile 128); C sits one float off"""
    _, ks, cps, last, red = resolve_split(pr, split)
    aligned = layout == "aligned"
    cls = pr.cls if aligned else GENERIC
    if presplit and mode != F32:
        cls = {CONV_FWD: CONV_FWD_WS, CONV_DGRAD: CONV_DGRAD_WS}[cls]
    threads = 512 if mode != F32 and tile == 128 and cls != GENERIC else 256
    depth = 0 if mode == F32 else 1 if threads == 512 and cls in (GEMM_NN, GEMM_TN, CONV_WGRAD, CONV_WGRAD_SAME) else 2
    return dict(cls=cls, fast=int(pr.fast and aligned), a_vec=int(pr.vec and (aligned or tile != 64)), b_vec=int(pr.vec and (aligned or tile != 128)),
                tile=tile, threads=threads, depth=depth, ksplit=ks, chunks_per_split=cps,
                reduce=RED_NONE if ks == 1 else red if aligned else RED_SCALAR, workspace_bytes=workspace_bytes(pr, ks, pr.colsum),
                colsum_offset=workspace_bytes(pr, ks, False))


# ------------------------------------------------------------------------------------------------ windows and descriptors
def geo(nbo, nbi, rows, cols, off, odd, ld_for_strides=None):
    """a [nbo][nbi][rows][cols] window inside a flat buffer: element (o, i, r, c) at front + o * bso + i * bsi + r * ld + c.  `off` columns in
    front of the window, ld > off + cols a multiple of 4 (+ 1 when `odd`), GUARD rows in front and behind, GAP rows and more between batches"""
    r4 = lambda v: -(-v // 4) * 4
    ld = r4(off + cols + 4) + (1 if odd else 0)
    lds = max(ld, ld_for_strides or 0)
    bsi = r4((rows + GAP) * lds)
    bso = r4(nbi * bsi + 8 * lds)
    front = GUARD * ld + off
    total = front + (nbo - 1) * bso + (nbi - 1) * bsi + rows * ld + GUARD * ld
    return NS(nbo=nbo, nbi=nbi, rows=rows, cols=cols, ld=ld, bsi=bsi, bso=bso, front=front, total=total)


def geometry(pr, layout, tile):
    """where A, B, the residual and C sit.  aligned: column offset 8, ld % 4 == 0.  mis: A one float off (tile 64) or B with an odd ld (tile 128),
    C one float off, the residual with an odd ld; batch strides stay multiples of 4, and C and the residual share theirs"""
    mis = layout != "aligned"
    a = geo(pr.nbo, pr.nbi, pr.a.rows, pr.a.cols, 1 if mis and tile == 64 else 8, False)
    b = geo(pr.nbo, 1 if pr.shared_b else pr.nbi, pr.b.rows, pr.b.cols, 8, mis and tile == 128)
    ldc = geo(1, 1, pr.M, pr.N, 8, False).ld
    ldr = geo(1, 1, pr.M, pr.N, 8, mis).ld
    c = geo(pr.nbo, pr.nbi, pr.M, pr.N, 1 if mis else 8, False, max(ldc, ldr))
    r = geo(pr.nbo, pr.nbi, pr.M, pr.N, 8, mis, max(ldc, ldr))
    assert (c.bso, c.bsi) == (r.bso, r.bsi)
    return NS(a=a, b=b, c=c, r=r)


def fill_operand(o, spec, g, base, batched, shared):
    o.kind, o.kc, o.p, o.ld = spec.kind, spec.kc, base + 4 * g.front, g.ld
    o.bs_outer, o.bs_inner = (g.bso, 0 if shared else g.bsi) if batched else (0, 0)
    for k, v in spec.geo.items():
        setattr(o, k, v)


def make_desc(L, pr, g, base, tile, mode, ksplit, epilogue, colsum=True):
    """bd_igemm_desc of the problem at geometry g; base: name -> address of the flat buffers a, b, c, r, bias, rowbias, colsum, ws
    (rowbias: [groups][N + 3]; colsum: [32 + M + 32])"""
    d = L.IgemmDesc(M=pr.M, N=pr.N, K=pr.K, batch_outer=pr.nbo, batch_inner=pr.nbi, tile=tile, mode=mode, ksplit=ksplit, alpha=1.0, out_scale=1.0)
    batched = pr.nbo * pr.nbi > 1
    fill_operand(d.A, pr.a, g.a, base["a"], batched, False)
    fill_operand(d.B, pr.b, g.b, base["b"], batched, pr.shared_b)
    d.C, d.ldc = base["c"] + 4 * g.c.front, g.c.ld
    if batched:
        d.c_bs_outer, d.c_bs_inner = g.c.bso, g.c.bsi
    if epilogue != "plain":
        d.alpha, d.out_scale, d.bias = ALPHA, OUT_SCALE, base["bias"]
        d.rowbias, d.ld_rowbias, d.rows_per_group = base["rowbias"], pr.N + 3, pr.rpg
        d.residual, d.ldr = base["r"] + 4 * g.r.front, g.r.ld
        d.accumulate = int(epilogue == "full+acc")
    if pr.colsum and colsum:
        d.a_colsum = base["colsum"] + 4 * 32
    d.workspace = base["ws"]
    return d


# ------------------------------------------------------------------------------------------------ operands and fp64 references (CPU)
def conv_ref(cid, x, w, dy):
    """fp64 F.conv2d of the case (NHWC operands, w [Cout][3][3][Cin]) and its autograd: y, the gradient over the conv's own (virtual,
    upsampled) input grid, and the weight gradient -- each from the operands it is given (None: zeros; every result is bilinear)"""
    B, Hs, Ws, Cin, Cout, stride, pad, ups, asym = CONV_CASES[cid][:9]
    Ho, Wo = conv_out_hw(Hs, Ws, stride, pad, ups, asym)
    xi = torch.zeros(B, Cin, Hs << ups, Ws << ups, dtype=torch.float64)
    if x is not None:
        xn = x.double().reshape(B, Hs, Ws, Cin).permute(0, 3, 1, 2)
        xi = F.interpolate(xn, scale_factor=2.0, mode="nearest") if ups else xn.clone()
    xi.requires_grad_(True)
    wn = (torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64) if w is None else w.double().reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2).clone()).requires_grad_(True)
    y = F.conv2d(F.pad(xi, (0, 1, 0, 1)) if asym else xi, wn, None, stride=stride, padding=0 if asym else pad)
    assert y.shape[2:] == (Ho, Wo)
    out = NS(y=y.detach().permute(0, 2, 3, 1).reshape(B * Ho * Wo, Cout))
    if dy is not None:
        y.backward(dy.double().reshape(B, Ho, Wo, Cout).permute(0, 3, 1, 2))
        out.dx = xi.grad.permute(0, 2, 3, 1).reshape(-1, Cin)
        out.dw = wn.grad.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)
    return out


def product64(pr, a, b):
    """the fp64 product [nbo][nbi][M][N] of the operands as they lie in memory ([nbo][nbi][rows][cols]; a shared B has one inner entry)"""
    kind, cid, what = pr.key[:3]
    if kind == "gemm":
        al = a.double() if pr.a.kc else a.double().transpose(-1, -2)
        bl = b.double() if pr.b.kc else b.double().transpose(-1, -2)
        return al @ bl.transpose(-1, -2)                      # a shared B broadcasts over the inner batch
    a, b = a[0, 0], b[0, 0]
    if what == "fwd":
        p = conv_ref(cid, a, b, None).y
    elif what == "dgrad":
        p = conv_ref(cid, None, b.reshape(-1, 9 * b.shape[-1]), a).dx       # b: [(co, tap)][ci] = w [Cout][3][3][Cin]
    else:
        p = conv_ref(cid, b, None, a).dw
    return p[None, None]


@functools.lru_cache(maxsize=None)
def problem_data(key, opset):
    """operands in memory form, epilogue addends and references of a problem; set A: A wide and B narrow, set B: the reverse.  The four forms
    of a GEMM case hold the same logical matrices, transposed as the form stores them"""
    pr = gemm_problem(*key[1:]) if key[0] == "gemm" else conv_problem(*key[1:])
    seed = 7000 * (sorted(GEMM_CASES).index(key[1]) if key[0] == "gemm" else 10 + sorted(CONV_CASES).index(key[1])) + (opset == "A")
    if key[0] == "conv":
        seed += 100 * DIRECTIONS.index(key[2])
    g = torch.Generator().manual_seed(seed)
    a_gen, b_gen = (_wide, _narrow) if opset == "A" else (_narrow, _wide)
    if key[0] == "gemm":
        a = a_gen(g, pr.nbo, pr.nbi, pr.M, pr.K)
        b = b_gen(g, pr.nbo, pr.nbi, pr.N, pr.K)
        if pr.shared_b:
            b = b[:, :1]
        a = a if pr.a.kc else a.transpose(-1, -2).contiguous()
        b = b if pr.b.kc else b.transpose(-1, -2).contiguous()
    else:
        a = a_gen(g, 1, 1, pr.a.rows, pr.a.cols)
        b = b_gen(g, 1, 1, pr.b.rows, pr.b.cols)
    groups = -(-pr.M // pr.rpg)
    d = NS(pr=pr, a=a, b=b, bias=_quarters(g, pr.N), rowbias=_quarters(g, groups, pr.N), residual=_quarters(g, pr.nbo, pr.nbi, pr.M, pr.N),
           prev=_quarters(g, pr.nbo, pr.nbi, pr.M, pr.N))
    d.prod = {False: product64(pr, a, b), True: product64(pr, rnd(a), rnd(b))}          # [rounded to bf16?]
    d.colsum = (a.double().sum(-2) if not pr.a.kc else a.double().sum(-1))[0, 0]          # row sums of the unrounded A(m, k)
    return d


def epilogue64(d, prod, epilogue):
    """out_scale * (alpha * prod + bias[n] + rowbias[m / rows_per_group][n] + residual) (+ the previous C)"""
    if epilogue == "plain":
        return prod.clone()
    rows = torch.arange(d.pr.M) // d.pr.rpg
    y = OUT_SCALE * (ALPHA * prod + d.bias.double() + d.rowbias.double()[rows] + d.residual.double())
    return y + d.prev.double() if epilogue == "full+acc" else y
