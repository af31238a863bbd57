"""Case table, operands, window geometry, descriptors and fp64 references of the thin-convolution dispatch tests
(tests/test_thin_plan_host.py checks the table against bd_conv3x3_{fwd,dgrad,wgrad}_plan and proves the data rounding-free on the CPU;
tests/test_thin_dispatch.py runs the kernels on it).  Nothing here touches a device: descriptors are filled from a geometry and base
addresses, which the host test fakes.

A case is one call of bd_conv3x3_fwd / _dgrad / _wgrad with 3 or 1 channels on one side, together with what csrc/conv_thin.hip is expected
to decide for it when every buffer is aligned: the path, the loop count of that path, the grid, pix_per_block and the partial rows -- in
BD_MODE_F32 and in the two bf16 modes, which always decide alike.  DESIGN.md "Dispatch branches of the thin convolutions" carries the same
table; whoever retunes the guards moves the cases with them."""
import functools
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from tests.test_conv_ps_dispatch import _narrow, _quarters, rnd

F32, BF16X3, BF16 = 0, 1, 2
MODES = (F32, BF16X3, BF16)
# enum bd_thin_path
(IGEMM, EXPAND_FMA, EXPAND_MFMA, CONTRACT, CONTRACT_DGRAD, WGRAD_MFMA, WGRAD_ROW, WGRAD_CIN, WGRAD_COUT) = range(9)
PATH_NAME = ["igemm", "expand-fma", "expand-mfma", "contract", "contract-dgrad", "wgrad-mfma", "wgrad-row", "wgrad-cin", "wgrad-cout"]
PLAN_FIELDS = ("path", "J", "loops", "pix_per_block", "grid_x", "grid_y", "partial_rows", "workspace_bytes", "prof_class")
OUT_SCALE = 0.5
GUARD = 72          # rows in front of and behind every pixel window: more than W + 1 for the widest image (64), so a wrong tap of the first or last pixel stays inside
LAYOUTS = ("aligned", "mis", "narrow3")
SLAB_BYTES = 768 * 128 * 128 * 4        # the K-split slabs of bd_conv3x3_workspace_bytes: the thin partial rows must fit them


def P(path, loops=1, gx=0, gy=1, ppb=0, rows=0):
    """an expected plan: path, loop count, grid, pix_per_block, partial rows"""
    return NS(path=path, loops=loops, gx=gx, gy=gy, ppb=ppb, rows=rows)


IG = P(IGEMM, 0, 0, 0)


def case(direction, B, H, W, J, C, f32, bf16, why, den=2048, modes=MODES, layouts=LAYOUTS, big=False, pad=1, accumulate=0, nobias=False):
    """direction: fwd_in / dgrad_in / wgrad_in are conv_in (J -> C channels), *_out conv_out (C -> J).  f32 / bf16: the plan with every buffer
    aligned.  den: the wide grid is integers in (-den, den) over den.  big: the batch repeats two base images, each scaled by +-1 or +-0.5"""
    Cin, Cout = (J, C) if direction.endswith("_in") else (C, J)
    return NS(direction=direction, kind=direction.split("_")[0], B=B, H=H, W=W, J=J, C=C, Cin=Cin, Cout=Cout, plan={F32: f32, BF16X3: bf16, BF16: bf16},
              why=why, den=den, modes=modes, layouts=layouts if not big else ("aligned",), big=big, pad=pad, accumulate=accumulate, nobias=nobias)


def both(path_f32, path_bf16=None):
    return path_f32, path_bf16 or path_f32


CASES = {
    # ---- forward
    "F1": case("fwd_in", 2, 3, 4, 3, 128, *both(P(EXPAND_FMA, 1, 1, 1)), "FMA expand in all modes (W % 32 != 0); every pixel is a border pixel; 24 pixels: a partial last run"),
    "F2": case("fwd_in", 1, 2, 32, 3, 256, P(EXPAND_FMA, 1, 2, 2), P(EXPAND_MFMA, 1, 1, 2), "MFMA in the bf16 modes, grid.y = 2, two of four waves idle; with and without bias",
               nobias=True),
    "F3": case("fwd_in", 3, 5, 32, 3, 128, P(EXPAND_FMA, 1, 15, 1), P(EXPAND_MFMA, 1, 4, 1), "15 runs: the last workgroup is partial; image seams inside a workgroup"),
    "F4": case("fwd_in", 2, 7, 28, 1, 128, *both(P(EXPAND_FMA, 1, 13, 1)), "thin_expand_kernel<1>: FMA in all modes; 392 pixels = 12.25 runs"),
    "F5": case("fwd_in", 128, 32, 32, 3, 128, P(EXPAND_FMA, 4, 1024, 1), P(EXPAND_MFMA, 2, 512, 1), "131072 pixels: FMA iters 4, MFMA iters 2", big=True),
    "F6": case("fwd_out", 2, 3, 32, 3, 128, *both(P(CONTRACT, 1, 2, 1)), "contract, 6 segments: two waves of the second workgroup have none"),
    "F7": case("fwd_out", 1, 2, 64, 1, 128, *both(P(CONTRACT, 1, 1, 1)), "thin_contract_kernel<1>; segments with only a left or only a right border"),
    "F8": case("fwd_out", 1, 2, 32, 3, 256, IG, IG, "Cin != 128: igemm"),
    "F9": case("fwd_out", 1, 2, 12, 3, 128, IG, IG, "W % 32 != 0: igemm"),
    "F10": case("fwd_in", 1, 2, 6, 3, 128, IG, IG, "W % 4 != 0: igemm"),
    # ---- data gradient
    "G1": case("dgrad_in", 2, 3, 32, 3, 128, *both(P(CONTRACT_DGRAD, 1, 2, 1)), "contract-dgrad, 6 segments"),
    "G2": case("dgrad_in", 1, 2, 32, 3, 384, *both(P(CONTRACT_DGRAD, 1, 1, 1)), "three 128-channel chunks: the *o + v path"),
    "G3": case("dgrad_in", 1, 2, 32, 1, 128, *both(P(CONTRACT_DGRAD, 1, 1, 1)), "thin_contract_dgrad_kernel<1>"),
    "G4": case("dgrad_in", 512, 32, 32, 3, 128, *both(P(CONTRACT_DGRAD, 2, 2048, 1)), "524288 pixels: segs_per_wave 2", big=True),
    "G5": case("dgrad_out", 1, 2, 32, 3, 256, P(EXPAND_FMA, 1, 2, 2), P(EXPAND_MFMA, 1, 1, 2), "flipped-tap expand, MFMA in the bf16 modes"),
    "G6": case("dgrad_out", 2, 3, 4, 3, 256, *both(P(EXPAND_FMA, 1, 1, 2)), "flipped-tap expand, FMA (W = 4)"),
    "G7": case("dgrad_out", 2, 3, 4, 1, 128, *both(P(EXPAND_FMA, 1, 1, 1)), "flipped-tap expand, J = 1"),
    "G8": case("dgrad_in", 2, 3, 32, 3, 128, IG, IG, "accumulate = 1: igemm", accumulate=1),
}
# ---- weight gradient, both directions.  id: B, H, W, J, C, f32 plan, bf16 plan, why, extra
_W = {
    "W1": (2, 4, 32, 3, 128, P(WGRAD_ROW, 1, 2, 1, 0, 2), P(WGRAD_MFMA, 1, 16, 1, 0, 16), "row kernel in F32, MFMA in bf16, db from both", {}),
    "W2": (2, 4, 32, 3, 256, P(WGRAD_ROW, 1, 2, 2, 0, 2), P(WGRAD_MFMA, 1, 16, 2, 0, 16), "grid.y = 2: db of conv_out written by y == 0 only", {}),
    "W3": (5, 103, 32, 3, 128, P(WGRAD_ROW, 1, 129, 1, 0, 129), P(WGRAD_MFMA, 3, 344, 1, 0, 344),
           "1030 steps: steps_per_wg 3, the last workgroup gets one step; 515 segments in F32: the last workgroup gets three", dict(den=1024)),
    "W4": (25, 41, 32, 3, 128, P(WGRAD_ROW, 2, 129, 1, 0, 129), None, "1025 segments, F32: segs_per_wave 2, the last workgroup gets one segment",
           dict(den=512, modes=(F32,))),
    "W5": (3, 5, 7, 3, 128, *both(P(None, 1, 1, 1, 128, 1)), "general kernels, J = 3: 105 pixels = tiles of 64 + 41", {}),
    "W5j1": (3, 5, 7, 1, 128, *both(P(None, 1, 1, 1, 128, 1)), "general kernels, J = 1 (wgrad_thin_cin_kernel<1>, wgrad_thin_cout_kernel<1>)", {}),
    "W6": (5, 4, 12, 3, 128, *both(P(None, 1, 2, 1, 128, 2)), "P = 2, ragged: 128 + 112 pixels, last tile 48", {}),
    "W8": (2, 4, 32, 3, 128, *both(P(None, 1, 2, 1, 128, 2)), "pad_t = pad_l = 0 with Ho == Hs: the general kernels even at W = 32", dict(pad=0)),
}
for _cid, (_B, _H, _Wd, _J, _C, _f, _b, _why, _kw) in _W.items():
    for _dir, _general in (("wgrad_in", WGRAD_CIN), ("wgrad_out", WGRAD_COUT)):
        _pl = [P(_general if p.path is None else p.path, p.loops, p.gx, p.gy, p.ppb, p.rows) if p else None for p in (_f, _b)]
        CASES[f"{_cid}-{_dir[6:]}"] = case(_dir, _B, _H, _Wd, _J, _C, _pl[0], _pl[1], _why, **_kw)
CASES["W7-in"] = case("wgrad_in", 171, 28, 28, 1, 128, *both(P(WGRAD_CIN, 1, 699, 1, 192, 699)), "134064 pixels: pix_per_block 192, three tiles per workgroup",
                      den=64, big=True)
for _n, _c in CASES.items():
    _c.name = _n


def general_plan(c):
    """the general weight-gradient kernels on c's pixels (what a misaligned wide tensor gets in BD_MODE_F32): pix_per_block and P restated"""
    px = c.B * c.H * c.W
    n = c.Cout * 9 * c.Cin + c.Cout
    cap = max(1, min(1024, SLAB_BYTES // (4 * n)))
    ppb = max(-(-(-(-px // cap)) // 64) * 64, 128)
    rows = -(-px // ppb)
    return P(WGRAD_CIN if c.direction == "wgrad_in" else WGRAD_COUT, 1, rows, c.C // 128, ppb, rows)


def prof_class(c, path):
    if path == IGEMM or c.kind == "wgrad":
        return None
    return b"conv_thin_fwd" if c.kind == "fwd" else b"conv_thin_dgrad_in" if path == CONTRACT_DGRAD else b"conv_thin_dgrad"


def expected_plan(c, layout, mode):
    """what the plan query must report.  mis: the wide tensor (contract, contract-dgrad, weight gradients) or the output (expand) sits one float
    off: igemm, the general kernel in F32, and the unchanged MFMA kernel (scalar loads) in the bf16 modes.  narrow3: nothing changes"""
    p = c.plan[mode]
    if layout == "mis" and p.path != IGEMM:
        p = p if p.path in (WGRAD_MFMA, WGRAD_CIN, WGRAD_COUT) else general_plan(c) if p.path == WGRAD_ROW else IG
    if p.path == IGEMM:
        return dict.fromkeys(PLAN_FIELDS, 0) | dict(prof_class=None)
    n = c.Cout * 9 * c.Cin + c.Cout
    return dict(path=p.path, J=c.J, loops=p.loops, pix_per_block=p.ppb, grid_x=p.gx, grid_y=p.gy, partial_rows=p.rows, workspace_bytes=p.rows * n * 4,
                prof_class=prof_class(c, p.path))


# ------------------------------------------------------------------------------------------------ windows and descriptors
def geo(rows, cols, layout_off, contiguous=False):
    """a [rows][cols] window of a flat buffer: element (r, c) at front + r * ld + c.  aligned: 8 columns in front, ld > 8 + cols a multiple of 4;
    one float off: 9 columns; contiguous (the narrow3 layout): ld == cols behind an odd number of floats.  GUARD rows in front and behind"""
    r4 = lambda v: -(-v // 4) * 4
    ld = cols if contiguous else r4(8 + cols + 4)
    front = r4(GUARD * ld) + (1 if contiguous else layout_off)
    return NS(rows=rows, cols=cols, ld=ld, front=front, total=front + rows * ld + r4(GUARD * ld) + 4)


def tensors(c):
    """name -> (channels, is it the wide (C-channel) tensor, is it the output) of the case's three pixel tensors / flat weight arrays"""
    wide_first = c.direction in ("fwd_out", "dgrad_in")          # input is the C-channel tensor
    if c.kind == "fwd":
        return dict(x=(c.Cin, wide_first, False), y=(c.Cout, not wide_first, True))
    if c.kind == "dgrad":
        return dict(dy=(c.Cout, wide_first, False), dx=(c.Cin, not wide_first, True))
    return dict(x=(c.Cin, c.direction == "wgrad_out", False), dy=(c.Cout, c.direction == "wgrad_in", False))


def geometry(c, layout):
    """where the pixel tensors sit.  mis: one float in front of the C-channel tensor, the one every alignment guard of the pixel tensors is about
    (the output of the expand paths, the wide input of the others).  narrow3: the J-channel tensor contiguous (ld == J) behind an odd offset"""
    px = c.B * c.H * c.W
    return NS(**{name: geo(px, ch, 9 if layout == "mis" and wide else 8, contiguous=layout == "narrow3" and not wide)
                 for name, (ch, wide, _) in tensors(c).items()})


def make_desc(L, c, g, base, mode, layout="aligned", bias=True, db=True):
    """the descriptor of the case; base: name -> address of the flat buffers x, y, dy, dx (pixel tensors), w, bias, dw, db, ws.  w, bias, dw and
    db begin 8 floats into their buffers (a NaN band in front)"""
    common = dict(B=c.B, Hs=c.H, Ws=c.W, Cin=c.Cin, Cout=c.Cout, stride=1, pad_t=c.pad, pad_l=c.pad, ups=0, Ho=c.H, Wo=c.W, mode=mode,
                  workspace=base["ws"])
    at = lambda n: base[n] + 4 * getattr(g, n).front
    if c.kind == "fwd":
        return L.ConvFwdDesc(x=at("x"), ldx=g.x.ld, w=base["w"] + 32, bias=base["bias"] + 32 if bias else None, out_scale=OUT_SCALE, y=at("y"), ldy=g.y.ld, **common)
    if c.kind == "dgrad":
        return L.ConvDgradDesc(dy=at("dy"), lddy=g.dy.ld, w=base["w"] + 32, dx=at("dx"), lddx=g.dx.ld, accumulate=c.accumulate, **common)
    return L.ConvWgradDesc(x=at("x"), ldx=g.x.ld, dy=at("dy"), lddy=g.dy.ld, dw=base["dw"] + 32, db=base["db"] + 32 if db else None, **common)


# ------------------------------------------------------------------------------------------------ operands and fp64 references (CPU)
def _wide(g, den, *shape):
    return torch.randint(-(den - 1), den, shape, generator=g).float() / den


def conv_ref(c, x, w, dy):
    """fp64 F.conv2d of the case (NHWC operands, w [Cout][3][3][Cin]; pad 0: F.pad(0, 2, 0, 2), so Ho == Hs) and its autograd: y, dx, dw -- each
    from the operands it is given (None: zeros; every result is bilinear)"""
    nb = (x if x is not None else dy).shape[0]
    xn = (torch.zeros(nb, c.Cin, c.H, c.W, dtype=torch.float64) if x is None else x.double().permute(0, 3, 1, 2).clone()).requires_grad_(True)
    wn = (torch.zeros(c.Cout, c.Cin, 3, 3, dtype=torch.float64) if w is None else w.double().permute(0, 3, 1, 2).clone()).requires_grad_(True)
    y = F.conv2d(xn, wn, None, padding=1) if c.pad == 1 else F.conv2d(F.pad(xn, (0, 2, 0, 2)), wn, None, padding=0)
    assert y.shape[2:] == (c.H, c.W)
    out = NS(y=y.detach().permute(0, 2, 3, 1).contiguous())
    if dy is not None:
        y.backward(dy.double().permute(0, 3, 1, 2))
        out.dx = xn.grad.permute(0, 2, 3, 1).contiguous()
        out.dw = wn.grad.permute(0, 2, 3, 1).contiguous()
    return out


def product64(c, a, b):
    """the base result of the case from its two operands as given: fwd (x, w) -> y without bias; dgrad (dy, w) -> dx; wgrad (x, dy) -> dw, one
    per base image when the case is big (the batch's dw is a combination of them)"""
    if c.kind == "fwd":
        return conv_ref(c, a, b, None).y
    if c.kind == "dgrad":
        return conv_ref(c, None, b, a).dx
    if c.big:
        return torch.stack([conv_ref(c, a[i:i + 1], None, b[i:i + 1]).dw for i in range(a.shape[0])])
    return conv_ref(c, a, None, b).dw


@functools.lru_cache(maxsize=None)
def case_data(name, opset):
    """operands, epilogue addends and base references of a case.  a / b: fwd (x, w), dgrad (dy, w), wgrad (x, dy).  Set A: a wide and b narrow, set
    B the reverse.  A big case holds two base images; batch entry i is image idx[i] with `a` scaled by s[i] in {1, -1, 0.5, -0.5}"""
    c = CASES[name]
    g = torch.Generator().manual_seed(9000 + 10 * sorted(CASES).index(name) + (opset == "A"))
    nb = 2 if c.big else c.B
    wide, narrow = (lambda *s: _wide(g, c.den, *s)), (lambda *s: _narrow(g, *s))
    a_gen, b_gen = (wide, narrow) if opset == "A" else (narrow, wide)
    ca, cb = {"fwd": (c.Cin, None), "dgrad": (c.Cout, None), "wgrad": (c.Cin, c.Cout)}[c.kind]
    a = a_gen(nb, c.H, c.W, ca)
    b = b_gen(nb, c.H, c.W, cb) if cb else b_gen(c.Cout, 3, 3, c.Cin)
    d = NS(c=c, a=a, b=b, bias=_quarters(g, c.Cout), prev=_quarters(g, nb, c.H, c.W, c.Cin))
    if c.big:
        d.idx = torch.arange(c.B) % 2
        d.s = torch.tensor([1.0, -1.0, 0.5, -0.5])[torch.randint(0, 4, (c.B,), generator=g)]
    else:
        d.idx, d.s = torch.arange(c.B), torch.ones(c.B)
    d.prod = {False: product64(c, a, b), True: product64(c, rnd(a), rnd(b))}          # [operands rounded to bf16?]
    d.db = b.double().sum(dim=(1, 2)) if c.kind == "wgrad" else None                # per base image [nb][Cout], from the unrounded dy
    return d


def full_a(d, dev="cpu"):
    """the `a` operand of the whole batch"""
    return d.a.to(dev)[d.idx.to(dev)] * d.s.to(dev)[:, None, None, None]


def full_b(d, dev="cpu"):
    return d.b.to(dev)[d.idx.to(dev)] if d.c.kind == "wgrad" else d.b.to(dev)


def compose64(d, prod, bias=True):
    """the fp64 result of the whole batch from the base result `prod` (on the device of prod): y [B,H,W,Cout] = out_scale * (conv + bias);
    dx (+ the previous dx under accumulate); dw [Cout,3,3,Cin]"""
    c, dev = d.c, prod.device
    idx, s = d.idx.to(dev), d.s.double().to(dev)
    if c.kind == "fwd":
        y = prod[idx] * s[:, None, None, None]
        return OUT_SCALE * (y + d.bias.double().to(dev)) if bias else OUT_SCALE * y
    if c.kind == "dgrad":
        dx = prod[idx] * s[:, None, None, None]
        return dx + d.prev.double().to(dev)[idx] if c.accumulate else dx
    if not c.big:
        return prod
    coef = torch.stack([s[idx == i].sum() for i in range(prod.shape[0])])
    return (prod * coef[:, None, None, None, None]).sum(0)


def db64(d):
    counts = torch.stack([(d.idx == i).sum() for i in range(d.db.shape[0])]).double() if d.c.big else torch.ones(d.db.shape[0], dtype=torch.float64)
    return (d.db * counts[:, None]).sum(0)
