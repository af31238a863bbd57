"""Exact-value tests for every branch of the phase-decomposed convolutions (csrc/conv_ph.hip: conv_ph_kernel<SP>, ph_tsplit_reduce,
ups_weff_kernel, ups_dweff_combine_kernel; csrc/conv_ps.hip: the PH = true form of conv_ps_wgrad_kernel with conv_ps_wgrad_reduce<false>
folding 4 * ksplit bias rows), in the manner of tests/test_conv_ps_dispatch.py, whose operand grids and helpers this file imports.

What the host code decides, and what each case pins (asserted from the ABI's own queries before anything is launched):
  * the tap split of the one-class 16-tap data gradient of the upsample convolution: while ceil(M/256) * (Cin/128) * 2 <= CUs the 16 taps
    are dealt to four workgroups per tile and ph_tsplit_reduce folds the partial tiles (bd_upsample_conv_dgrad_workspace_bytes = 4 M Cin 4),
    else one workgroup runs all 16 taps (workspace 0): D1, D2, D5, D6 split, D3 does not, D4 pins the boundary on the host;
  * the chunk count of a class, ntaps * C / 32 with ntaps in {1, 2, 4, 16} (four per group of a tap split): the three-stage ring takes "any
    count >= 1"; counts 1, 2, 3 (prologue and the two sp_sync<0> placements) and multiples of 3 (a loop ending on its third step) come from
    C = 32 / 64 / 96: S1 runs 4 / 2 / 2 / 1 chunks in one launch, S2 12 / 6 / 6 / 3, F2 and D2 12, D3 48;
  * the K split of the PHASE weight gradient (split_k over 2 * CUs slots, at least 8 chunks of 32 source pixels per slice): ksplit 1 still
    writes slabs and goes through the reduce (G1, G4, G5), G2 / G3 have 8 slices of 9 chunks and a last one of 2 / 3; G2's last chunk is
    ragged, G3 has two ci tiles per E entry.
Ragged tiles (M = 48, 80, 1088, 4160), one-pixel-wide grids (H = 1 or W = 1: every neighbour on one axis is off the grid) and the XCD
remap's tail (20 workgroups) ride on the same cases.

Operands are the grids of test_conv_ps_dispatch.py (wide: integers in (-2048, 2048) over 2048; narrow: {-1, -0.5, 0, 0.5, 1}; bias and
previous output: multiples of 1/4 in [-2, 2]), set A = wide activation x narrow weight, set B the reverse (weight gradient: wide x with
narrow dY, and the reverse).  The kernels multiply the PRE-SUMMED taps E[oy][ox]; on these grids E stays exact: up to four narrow taps
sum to a multiple of 1/2 up to 4 (lo = 0), up to four wide taps to an integer over 2048 below 4 (hi + lo exact, lo exact in bf16).  So every
product and partial sum is an fp32 number in any order (test_*_sums_exact, no GPU: magnitude bounds in units of 2^-12 below 2^24) and the
results are compared for EQUALITY with fp64 references:
  BD_MODE_BF16X3  the literal form: F.interpolate + F.conv2d, its data gradient (the transposed convolution + 2x2 sums, checked against
                  autograd on the CPU), fp64 autograd for dW; the stride-2 data gradient is fp64 autograd of the stride-2 convolution;
  BD_MODE_BF16    upsample forward / data gradient: the E form -- conv_transpose2d / conv2d with E as a 4x4 stride-2 kernel -- on rnd(x) /
                  rnd(dY) and rnd(E): the kernel rounds the SUMMED weight; stride-2 data gradient: rnd(dy), rnd(w); dW: autograd of the
                  literal form on rnd(x), rnd(dY); db: the fp64 sum of the unrounded dY in both modes.
The two modes' references differ (asserted), so equality in BD_MODE_BF16 also shows that the lo planes were not read.

Outputs go into NaN-filled buffers with a 256-row guard band; the strided variants give the output a leading dimension of N + 32 (the pad
columns must stay NaN) and the input planes a leading dimension of C + 32 whose pad block holds a bf16 NaN pattern.

The case table holds for 256 CUs; on another device the GPU tests skip.  Whoever retunes upsample_conv_dgrad_tap_groups or ps_wgrad_plan moves the cases with
it ("Dispatch branches of the phase-decomposed convolutions").

Observed on MI355X (256 CUs): equality held on every case, mode, operand set and epilogue of the four entry points, on the planes of
bd_upsample_weights and on the two small kernels; no case found a fault in conv_ph.hip or in the PHASE weight gradient.  The fp32 accumulation
of the phase kernels is exact whenever every partial sum is representable, so the tests assert torch.equal and no error bound is needed.
Largest MEASURE exact_units, as a fraction of 2^24: forward 0.073 (F2), upsample data gradient 0.288 (D3), stride-2 data gradient 0.033 (S2),
weight gradient dw 0.658 / db 0.627 (G3).

Mutation spot-check (each run once on a scratch build; "old" = the randn / 3e-5 tests of test_hip_round2.py and test_bf16_mode.py):
  ph_o_of's two returns for p = 1 swapped                 new: all F cases + strided            old: caught
  v_woff read at q_t instead of tbase + q_t               new: D1 D2 D5 D6 + strided (not D3)   old: caught
  ph_tsplit_reduce starts at g = 2                        new: D1 D2 D5 D6 + strided (not D3)   old: caught
  yoff = pc.q * 2 * W + pc.p                              new: all F and S cases + strided      old: caught
  ph_set(2) -> 2 in ups_dweff_combine_kernel              new: all G cases + strided            old: caught
  brows = ksplit instead of 4 * ksplit                    new: all G cases + strided            old: caught
  -1 / +1 of dyt exchanged in the PHASE prologue          new: G1 G2 G3 G5 + strided (not G4: H = 1)   old: caught
  E summed kx-outer instead of ky-outer (last bit of E)   new: the two randn plane tests        old: NOT caught
("Clear bit 0 of vm[j]" was not tried: vm[j] guards the DMA reads.)"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_conv_ps_dispatch import EXPECTED_CUS, UNIT, _check_split, _mag, _narrow, _quarters, _wide, bracketed, describe, rnd
from tests.test_gemm_sp_dispatch import SENTINEL, describe_planes, planes

gpu = pytest.mark.gpu       # per test: the table, precondition and rejection tests run without a device

BF16X3, BF16 = 1, 2
MODES = (BF16X3, BF16)
GUARD = 256                 # rows behind the last row of every output buffer
PAD = 32                    # extra columns of a strided buffer
OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -4

# upsample forward.  id: (B, H, W [source grid], Cin, Cout, chunks per class, workgroups per class, what for)
FWD_CASES = {
    "F1": (3, 4, 4, 32, 128, 4, 1, "M = 48: one tile, only the first wave row has rows, predicated epilogue; 4 classes x 4 chunks"),
    "F2": (5, 2, 8, 96, 256, 12, 2, "12 chunks (a multiple of 3); M = 80: one whole and one ragged 64-row wave; non-square; two N tiles"),
    "F3": (17, 8, 8, 64, 512, 8, 20, "M = 1088: 5 x 4 workgroups per class, XCD remap with a tail of 4, last tile 64 rows"),
    "F4": (2, 1, 4, 32, 128, 4, 1, "one-pixel-high source grid"),
    "F5": (2, 4, 1, 32, 128, 4, 1, "one-pixel-wide source grid"),
}
# upsample data gradient.  id: (B, H, W [source grid], Cout [contracted], Cin [output], tap groups, chunks per group, tiles, what for)
DGRAD_CASES = {
    "D1": (3, 4, 4, 32, 128, 4, 4, 1, "tap split, ragged partial tile, ph_tsplit_reduce"),
    "D2": (5, 2, 8, 96, 256, 4, 12, 2, "tap split, 12 chunks per group (a multiple of 3), two N tiles"),
    "D3": (65, 8, 8, 96, 1024, 1, 48, 136, "NO split (17 x 8 = 136 tiles): one workgroup runs the 16 taps, workspace 0; last tile 64 rows"),
    "D5": (2, 1, 4, 32, 128, 4, 4, 1, "one-pixel-high source grid"),
    "D6": (2, 4, 1, 32, 128, 4, 4, 1, "one-pixel-wide source grid"),
}
D4_BOUNDARY = (64, 8, 8, 32, 1024)      # 16 x 8 = 128 tiles: 2 * 128 <= 256 still splits (a 64 MiB workspace: pinned on the host, never launched)
# stride-2 data gradient.  id: (B, Ho, Wo [output grid of the convolution], Cout [contracted], Cin, pads, chunks of the four classes, workgroups per class, what for)
S2_CASES = {
    "S1": (3, 4, 4, 32, 128, (0, 1), (4, 2, 2, 1), 1, "chunk counts 1, 2 and 4 in one launch"),
    "S2": (5, 2, 8, 96, 256, (0, 1), (12, 6, 6, 3), 2, "chunk count 3 and multiples of 3"),
    "S3": (17, 8, 8, 64, 512, (1,), (8, 4, 4, 2), 20, "remap tail, ragged"),
    "S4": (2, 1, 4, 32, 128, (0, 1), (4, 2, 2, 1), 1, "one-pixel-high output grid"),
}
# upsample weight gradient.  id: (B, H, W [source grid], Cin, Cout, ksplit, chunks per slice, chunks of the last slice, what for)
WGRAD_CASES = {
    "G1": (3, 4, 4, 128, 128, 1, 2, 2, "ksplit 1 (still slabs + reduce), 2 chunks, ragged last chunk (48 pixels)"),
    "G2": (129, 4, 4, 128, 128, 8, 9, 2, "7 slices of 9 chunks and one of 2; ragged last chunk (2064 pixels); 32 bias rows"),
    "G3": (33, 8, 8, 256, 128, 8, 9, 3, "last slice 3 chunks; two ci tiles per E entry"),
    "G4": (2, 1, 4, 128, 128, 1, 1, 1, "one-pixel-high source grid: vertical neighbours all off the grid"),
    "G5": (2, 4, 1, 128, 128, 1, 1, 1, "one-pixel-wide source grid"),
}
STRIDED = {"fwd": "F2", "dgrad": ("D2", "D3"), "s2": "S2", "wgrad": "G3"}

cdiv = lambda a, b: -(-a // b)
ids = lambda cases: [pytest.param(cid, s, id=f"{cid}-{s}") for cid in cases for s in "AB"]


# ------------------------------------------------------------------------------------------------ E, operands (CPU, deterministic)
TAP_SETS = {-1: (2,), 0: (1, 2), 1: (0, 1), 2: (0,)}      # S(o): the ky that read source offset o (conv_ph.hip, ph_set)


def E_of(w):
    """W [Cout,3,3,Cin] -> E [Cout,4,4,Cin], E[oy+1][ox+1] = sum_{ky in S(oy)} sum_{kx in S(ox)} W[ky][kx], added in the kernel's stated
    order (from zero, ky outer, kx inner) in w's own precision: numpy float32 reproduces ups_weff_kernel bit for bit, float64 is the exact sum
    on the grids"""
    a = w.numpy()
    e = np.zeros((a.shape[0], 4, 4, a.shape[3]), dtype=a.dtype)
    for oy in range(-1, 3):
        for ox in range(-1, 3):
            s = np.zeros((a.shape[0], a.shape[3]), dtype=a.dtype)
            for ky in TAP_SETS[oy]:
                for kx in TAP_SETS[ox]:
                    s = s + a[:, ky, kx, :]
            e[:, oy + 1, ox + 1, :] = s
    return torch.from_numpy(e)


def _gens(opset):
    """(activation generator, weight generator): set A wide x narrow, set B narrow x wide"""
    return (_wide, _narrow) if opset == "A" else (_narrow, _wide)


def _gen(cid, opset):
    return torch.Generator().manual_seed({"F": 5000, "D": 6000, "S": 7000, "G": 8000}[cid[0]] + 10 * int(cid[1:]) + (opset == "A"))


@functools.lru_cache(maxsize=None)
def fwd_operands(cid, opset):
    B, H, W, Cin, Cout = FWD_CASES[cid][:5]
    g = _gen(cid, opset); a_gen, w_gen = _gens(opset)
    return dict(x=a_gen(g, B, H, W, Cin), w=w_gen(g, Cout, 3, 3, Cin), bias=_quarters(g, Cout))


@functools.lru_cache(maxsize=None)
def dgrad_operands(cid, opset):
    B, H, W, Cout, Cin = DGRAD_CASES[cid][:5]
    g = _gen(cid, opset); a_gen, w_gen = _gens(opset)
    return dict(dy=a_gen(g, B, 2 * H, 2 * W, Cout), w=w_gen(g, Cout, 3, 3, Cin), prev=_quarters(g, B, H, W, Cin))


@functools.lru_cache(maxsize=None)
def s2_operands(cid, opset):
    B, Ho, Wo, Cout, Cin = S2_CASES[cid][:5]
    g = _gen(cid, opset); a_gen, w_gen = _gens(opset)
    return dict(dy=a_gen(g, B, Ho, Wo, Cout), w=w_gen(g, Cout, 3, 3, Cin), prev=_quarters(g, B, 2 * Ho, 2 * Wo, Cin))


@functools.lru_cache(maxsize=None)
def wgrad_operands(cid, opset):
    B, H, W, Cin, Cout = WGRAD_CASES[cid][:5]
    g = _gen(cid, opset); x_gen, dy_gen = _gens(opset)
    return dict(x=x_gen(g, B, H, W, Cin), dy=dy_gen(g, B, 2 * H, 2 * W, Cout))


# ------------------------------------------------------------------------------------------------ fp64 references (CPU); NHWC in and out
nchw = lambda t: t.double().permute(0, 3, 1, 2)
nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
oihw = lambda w: w.double().permute(0, 3, 1, 2)            # [Cout,3,3,Cin] -> [Cout,Cin,3,3]
e_kernel = lambda e: e.double().permute(3, 0, 1, 2)         # E [Cout,4,4,Cin] -> [Cin,Cout,4,4]: conv_transpose2d's (in, out) and conv2d's (out, in)


def ups_fwd_literal(x, w):
    return nhwc(F.conv2d(F.interpolate(nchw(x), scale_factor=2.0, mode="nearest"), oihw(w), None, padding=1))


def ups_fwd_eform(x, e):
    """y[2a+p, 2b+q] = sum x[a+dy, b+dx] E[oy][ox]: the transposed convolution with E as a 4x4 kernel, stride 2, padding 1 (kernel index oy + 1)"""
    return nhwc(F.conv_transpose2d(nchw(x), e_kernel(e), None, stride=2, padding=1))


def ups_dgrad_literal(dy, w):
    """the data gradient of the literal form, written out: the 3x3 convolution's data gradient on the fine grid (its transposed convolution),
    then the 2x2 sums of the nearest upsampling's (test_written_out_data_gradient_is_autograd holds it to autograd)"""
    g = F.conv_transpose2d(nchw(dy), oihw(w), None, padding=1)
    B, C, H2, W2 = g.shape
    return nhwc(g.reshape(B, C, H2 // 2, 2, W2 // 2, 2).sum(dim=(3, 5)))


def ups_dgrad_eform(dy, e):
    """dx[a, b] = sum_{oy, ox} dY[2a+oy, 2b+ox] E[oy][ox]^T: a 4x4 stride-2 padding-1 convolution of dY"""
    return nhwc(F.conv2d(nchw(dy), e_kernel(e), None, stride=2, padding=1))


def ups_autograd(x, w, dy, want="dx"):
    """fp64 autograd of the literal form -> dx NHWC, or dw [Cout,3,3,Cin]"""
    xr = nchw(x).requires_grad_(want == "dx"); wr = oihw(w).requires_grad_(want == "dw")
    F.conv2d(F.interpolate(xr, scale_factor=2.0, mode="nearest"), wr, None, padding=1).backward(nchw(dy))
    return nhwc(xr.grad if want == "dx" else wr.grad)


def s2_dgrad_autograd(dy, w, pad):
    """fp64 autograd of the stride-2 convolution (pad 0 = F.pad(0,1,0,1) + padding 0, pad 1 = padding 1) with respect to its input"""
    B, Ho, Wo, _ = dy.shape
    xr = torch.zeros(B, w.shape[-1], 2 * Ho, 2 * Wo, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(xr, (0, 1, 0, 1)) if pad == 0 else xr, oihw(w), None, stride=2, padding=pad)
    assert tuple(y.shape[-2:]) == (Ho, Wo)
    y.backward(nchw(dy))
    return nhwc(xr.grad)


def rnd_E(w):
    """what BD_MODE_BF16 multiplies: the bf16 rounding of the SUMMED weight (exact sum: E is an fp32 number on the grids)"""
    return rnd(E_of(w.double()).float())


@functools.lru_cache(maxsize=None)
def fwd_ref(cid, opset, mode):
    o = fwd_operands(cid, opset)
    return ups_fwd_literal(o["x"], o["w"]) if mode == BF16X3 else ups_fwd_eform(rnd(o["x"]), rnd_E(o["w"]))


@functools.lru_cache(maxsize=None)
def dgrad_ref(cid, opset, mode):
    o = dgrad_operands(cid, opset)
    return ups_dgrad_literal(o["dy"], o["w"]) if mode == BF16X3 else ups_dgrad_eform(rnd(o["dy"]), rnd_E(o["w"]))


@functools.lru_cache(maxsize=None)
def s2_ref(cid, opset, mode, pad):
    o = s2_operands(cid, opset)
    prep = rnd if mode == BF16 else (lambda t: t)
    return s2_dgrad_autograd(prep(o["dy"]), prep(o["w"]), pad)


@functools.lru_cache(maxsize=None)
def wgrad_ref(cid, opset, mode):
    o = wgrad_operands(cid, opset)
    prep = rnd if mode == BF16 else (lambda t: t)
    w0 = torch.zeros(o["dy"].shape[-1], 3, 3, o["x"].shape[-1])
    return ups_autograd(prep(o["x"]), w0, prep(o["dy"]), want="dw")


# ------------------------------------------------------------------------------------------------ the case table, from the ABI (no GPU)
def _lib():
    from baddiffusion_amd import _lib as L
    return L, L.load()


def _table_holds_here():
    """the table is for 256 CUs: the host falls back to that without a device; a device with another count skips"""
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != EXPECTED_CUS:
        pytest.skip(f"the branch tables are for {EXPECTED_CUS} CUs")


def dgrad_workspace_bytes(lib, L, B, H, W, Cout, Cin):
    d = L.UpsampleConvDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, mode=BF16X3)
    return lib.bd_upsample_conv_dgrad_workspace_bytes(ctypes.byref(d))


def wgrad_split(lib, L, B, H, W, Cin, Cout):
    """(ksplit, chunks per slice, chunks of the last slice, workspace bytes) from bd_upsample_conv_wgrad_workspace_bytes =
    (ks (16 Cin Cout + 4 Cout) + 16 Cin Cout) * 4, solved for ks"""
    d = L.UpsampleConvDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, mode=BF16X3)
    wsb = lib.bd_upsample_conv_wgrad_workspace_bytes(ctypes.byref(d))
    mn = 16 * Cin * Cout
    ks, rem = divmod(wsb // 4 - mn, mn + 4 * Cout)
    assert wsb % 4 == 0 and rem == 0 and ks >= 1, (wsb, ks, rem)
    nch = cdiv(B * H * W, 32)
    cps = cdiv(nch, ks)
    return ks, cps, nch - (ks - 1) * cps, wsb


def test_case_table_follows_the_dispatch_rules():
    """every branch named in the tables, from the ABI's workspace queries and the launch geometry (256 x 128 tiles, 32-channel chunks)"""
    _table_holds_here()
    L, lib = _lib()
    for cid, (B, H, W, Cin, Cout, chunks, wgs, _) in FWD_CASES.items():
        assert chunks == 4 * Cin // 32 and wgs == cdiv(B * H * W, 256) * (Cout // 128), cid
        assert Cin % 32 == 0 and Cout % 128 == 0
    for cid, (B, H, W, Cout, Cin, groups, chunks, tiles, _) in DGRAD_CASES.items():
        M = B * H * W
        assert tiles == cdiv(M, 256) * (Cin // 128), cid
        assert groups == (4 if 2 * tiles <= EXPECTED_CUS else 1), cid
        assert dgrad_workspace_bytes(lib, L, B, H, W, Cout, Cin) == (4 * M * Cin * 4 if groups == 4 else 0), cid
        assert chunks == (16 // groups) * Cout // 32 and Cout <= 256, cid          # a 16-tap contraction stays at Cout <= 256 (exact range)
    assert DGRAD_CASES["D3"][5] == 1 and dgrad_workspace_bytes(lib, L, *DGRAD_CASES["D3"][:5]) == 0       # the unsplit branch
    B, H, W, Cout, Cin = D4_BOUNDARY
    assert cdiv(B * H * W, 256) * (Cin // 128) * 2 == EXPECTED_CUS                                       # exactly on the boundary: still split
    assert dgrad_workspace_bytes(lib, L, B, H, W, Cout, Cin) == 4 * B * H * W * Cin * 4 == 64 << 20
    assert dgrad_workspace_bytes(lib, L, B + 1, H, W, Cout, Cin) == 0
    for cid, (B, Ho, Wo, Cout, Cin, pads, chunks, wgs, _) in S2_CASES.items():
        assert chunks == tuple(t * Cout // 32 for t in (4, 2, 2, 1)) and wgs == cdiv(B * Ho * Wo, 256) * (Cin // 128), cid
    assert {1, 2, 4} <= set(S2_CASES["S1"][6]) and 3 in S2_CASES["S2"][6]
    assert all(c[5] % 3 == 0 for c in (FWD_CASES["F2"],)) and DGRAD_CASES["D2"][6] % 3 == 0 and DGRAD_CASES["D3"][6] % 3 == 0
    for cid, (B, H, W, Cin, Cout, ksplit, cps, last, _) in WGRAD_CASES.items():
        assert wgrad_split(lib, L, B, H, W, Cin, Cout)[:3] == (ksplit, cps, last), (cid, wgrad_split(lib, L, B, H, W, Cin, Cout))
        assert B * H * W <= 2112, cid                                               # beyond ~2100 source pixels the reference leaves the exact range


# ------------------------------------------------------------------------------------------------ the preconditions (no GPU)
def _units(worst):
    return float(worst.max()) / UNIT


@pytest.mark.parametrize("cid,opset", ids(FWD_CASES))
def test_upsample_forward_sums_exact(cid, opset):
    """x, w and E split exactly (hi + lo == v, lo exact in bf16); the literal convolution of the magnitudes plus |bias| stays below 2^24 units
    of 2^-12; the E form equals the literal form in fp64; the two modes' references differ"""
    o = fwd_operands(cid, opset)
    E = E_of(o["w"].double())
    assert torch.equal(E.float().double(), E)
    _check_split(o["x"], opset == "A"); _check_split(o["w"], opset == "B"); _check_split(E.float(), opset == "B")
    units = _units(ups_fwd_literal(_mag(o["x"]), _mag(o["w"])) + o["bias"].abs().double())
    print(f"MEASURE exact_units {cid} ups_fwd set {opset} {units / 2 ** 24:.3f} x 2^24")
    assert units < 2 ** 24, units
    assert torch.equal(ups_fwd_eform(o["x"], E), fwd_ref(cid, opset, BF16X3))
    assert not torch.equal(fwd_ref(cid, opset, BF16X3), fwd_ref(cid, opset, BF16))


@pytest.mark.parametrize("cid,opset", ids(DGRAD_CASES))
def test_upsample_dgrad_sums_exact(cid, opset):
    """the same for the data gradient: the E form with E of the weight magnitudes, plus 2 |prev|"""
    o = dgrad_operands(cid, opset)
    E = E_of(o["w"].double())
    assert torch.equal(E.float().double(), E)
    _check_split(o["dy"], opset == "A"); _check_split(o["w"], opset == "B"); _check_split(E.float(), opset == "B")
    units = _units(ups_dgrad_eform(_mag(o["dy"]), E_of(_mag(o["w"]).double())) + 2 * o["prev"].abs().double())
    print(f"MEASURE exact_units {cid} ups_dgrad set {opset} {units / 2 ** 24:.3f} x 2^24")
    assert units < 2 ** 24, units
    assert torch.equal(ups_dgrad_eform(o["dy"], E), dgrad_ref(cid, opset, BF16X3))
    assert not torch.equal(dgrad_ref(cid, opset, BF16X3), dgrad_ref(cid, opset, BF16))


@pytest.mark.parametrize("cid", ["D1", "D5", "D6"])
def test_written_out_data_gradient_is_autograd(cid):
    """ups_dgrad_literal (transposed convolution + 2x2 sums) is, bit for bit, fp64 autograd of F.interpolate + F.conv2d"""
    o = dgrad_operands(cid, "A")
    B, H, W, _, Cin = DGRAD_CASES[cid][:5]
    assert torch.equal(ups_dgrad_literal(o["dy"], o["w"]), ups_autograd(torch.zeros(B, H, W, Cin), o["w"], o["dy"]))


@pytest.mark.parametrize("cid,opset", ids(S2_CASES))
def test_stride2_dgrad_sums_exact(cid, opset):
    o = s2_operands(cid, opset)
    _check_split(o["dy"], opset == "A"); _check_split(o["w"], opset == "B")
    for pad in S2_CASES[cid][5]:
        units = _units(s2_dgrad_autograd(_mag(o["dy"]), _mag(o["w"]), pad) + 2 * o["prev"].abs().double())
        print(f"MEASURE exact_units {cid} s2_dgrad pad {pad} set {opset} {units / 2 ** 24:.3f} x 2^24")
        assert units < 2 ** 24, units
        assert not torch.equal(s2_ref(cid, opset, BF16X3, pad), s2_ref(cid, opset, BF16, pad))


@pytest.mark.parametrize("cid,opset", ids(WGRAD_CASES))
def test_upsample_wgrad_sums_exact(cid, opset):
    """dW (sums over all fine pixels, then over the E entries that hold a tap: autograd of the magnitudes covers both) and db (sums of the
    unrounded dY, grid 2^-11)"""
    o = wgrad_operands(cid, opset)
    _check_split(o["x"], opset == "A"); _check_split(o["dy"], opset == "B")
    w0 = torch.zeros(o["dy"].shape[-1], 3, 3, o["x"].shape[-1])
    units = _units(ups_autograd(_mag(o["x"]), w0, _mag(o["dy"]), want="dw"))
    db_units = float(o["dy"].abs().double().sum(dim=(0, 1, 2)).max()) * 2048
    print(f"MEASURE exact_units {cid} ups_wgrad set {opset} dw {units / 2 ** 24:.3f} db {db_units / 2 ** 24:.3f} x 2^24")
    assert units < 2 ** 24 and db_units < 2 ** 24, (units, db_units)
    assert not torch.equal(wgrad_ref(cid, opset, BF16X3), wgrad_ref(cid, opset, BF16))


# ------------------------------------------------------------------------------------------------ host rejections (no GPU, nothing launched)
DUMMY = 1 << 20             # a 128-byte aligned non-null address: never dereferenced, every call below fails a host check first


def _fwd_desc(L, **kw):
    f = dict(B=1, H=4, W=4, Cin=32, Cout=128, x_split=DUMMY, ldx=32, e_split=DUMMY, y=DUMMY, ldy=128, mode=BF16X3)
    f.update(kw)
    return L.UpsampleConvDesc(**f)


def _dgrad_desc(L, **kw):
    f = dict(B=1, H=4, W=4, Cin=128, Cout=32, dy_split=DUMMY, lddy=32, et_split=DUMMY, dx=DUMMY, lddx=128, workspace=DUMMY,
             workspace_bytes=1 << 40, mode=BF16X3)
    f.update(kw)
    return L.UpsampleConvDesc(**f)


def _s2_desc(L, **kw):
    f = dict(B=1, Ho=4, Wo=4, Cin=128, Cout=32, pad=1, dy_split=DUMMY, lddy=32, wT_split=DUMMY, dx=DUMMY, lddx=128, mode=BF16X3)
    f.update(kw)
    return L.ConvS2DgradDesc(**f)


def _wgrad_desc(L, **kw):
    f = dict(B=1, H=4, W=4, Cin=128, Cout=128, x_split=DUMMY, ldx=128, dy_split=DUMMY, lddy=128, dw=DUMMY, workspace=DUMMY,
             workspace_bytes=1 << 40, mode=BF16X3)
    f.update(kw)
    return L.UpsampleConvDesc(**f)


# field names of (H, W, contracted channels C, its leading dimension, its base, output channels N) per entry point
PH_ENTRY = {
    "bd_upsample_conv_fwd": (_fwd_desc, "H", "W", "Cin", "ldx", "x_split", "e_split", "Cout"),
    "bd_upsample_conv_dgrad": (_dgrad_desc, "H", "W", "Cout", "lddy", "dy_split", "et_split", "Cin"),
    "bd_conv3x3_s2_dgrad_ps": (_s2_desc, "Ho", "Wo", "Cout", "lddy", "dy_split", "wT_split", "Cin"),
}


def _rejects(lib, fn, desc, code, word):
    rc = getattr(lib, fn)(ctypes.byref(desc), None)
    msg = lib.bd_last_error() or b""
    assert rc == code and word in msg and fn.encode() in msg, (fn, rc, msg)


@pytest.mark.parametrize("fn", list(PH_ENTRY))
def test_ph_common_rejections(fn):
    """the argument checks shared by the three conv_ph entry points: the return code and a word of bd_last_error() for each"""
    L, lib = _lib()
    make, h, w, c, ld, a, wt, n = PH_ENTRY[fn]
    _rejects(lib, fn, make(L, **{h: 3}), ERR_UNSUPPORTED, b"powers of two")
    _rejects(lib, fn, make(L, **{w: 6}), ERR_UNSUPPORTED, b"powers of two")
    _rejects(lib, fn, make(L, **{c: 48, ld: 64}), ERR_UNSUPPORTED, b"channels")
    _rejects(lib, fn, make(L, **{n: 192}), ERR_UNSUPPORTED, b"channels")
    _rejects(lib, fn, make(L, **{ld: 48}), ERR_UNSUPPORTED, b"ld % 32")
    _rejects(lib, fn, make(L, **{a: DUMMY + 64}), ERR_UNSUPPORTED, b"128-byte aligned")
    _rejects(lib, fn, make(L, **{wt: DUMMY + 64}), ERR_UNSUPPORTED, b"128-byte aligned")
    _rejects(lib, fn, make(L, B=1 << 17, **{h: 64, w: 64}), ERR_UNSUPPORTED, b"grid too large")       # B H W * 4 == 2^31
    _rejects(lib, fn, make(L, **{w: 1 << 14, ld: 1 << 15, c: 1 << 15}), ERR_UNSUPPORTED, b"grid too large")   # (4 W + 4) * ld * 4 >= 2^31
    _rejects(lib, fn, make(L, **{a: None}), ERR_INVALID, b"null pointer")
    _rejects(lib, fn, make(L, mode=3), ERR_INVALID, b"mode")


def test_other_phase_rejections():
    L, lib = _lib()
    _rejects(lib, "bd_conv3x3_s2_dgrad_ps", _s2_desc(L, pad=2), ERR_UNSUPPORTED, b"pad must be 0 or 1")
    _rejects(lib, "bd_conv3x3_s2_dgrad_ps", _s2_desc(L, pad=-1), ERR_UNSUPPORTED, b"pad must be 0 or 1")
    for cin, cout in ((48, 64), (64, 48), (0, 64)):
        assert lib.bd_upsample_weights(DUMMY, cin, cout, DUMMY, DUMMY, None) == ERR_UNSUPPORTED
        assert b"bd_upsample_weights: channels" in lib.bd_last_error()
    assert lib.bd_upsample_weights(DUMMY, 64, 64, None, DUMMY, None) == ERR_INVALID and b"null pointer" in lib.bd_last_error()
    # the weight gradient: its kernel's tiles need Cin, Cout % 128 (the forward and the data gradient take Cin % 32)
    _rejects(lib, "bd_upsample_conv_wgrad", _wgrad_desc(L, Cin=64, ldx=64), ERR_UNSUPPORTED, b"multiples of 128")
    _rejects(lib, "bd_upsample_conv_wgrad", _wgrad_desc(L, Cout=64, lddy=64), ERR_UNSUPPORTED, b"multiples of 128")
    _rejects(lib, "bd_upsample_conv_wgrad", _wgrad_desc(L, H=3), ERR_UNSUPPORTED, b"power-of-two")
    _rejects(lib, "bd_upsample_conv_wgrad", _wgrad_desc(L, lddy=144), ERR_UNSUPPORTED, b"ld % 32")
    _rejects(lib, "bd_upsample_conv_wgrad", _wgrad_desc(L, x_split=DUMMY + 64), ERR_UNSUPPORTED, b"128-byte aligned")
    _rejects(lib, "bd_upsample_conv_wgrad", _wgrad_desc(L, B=1 << 17, H=64, W=64), ERR_UNSUPPORTED, b"overflows")
    _rejects(lib, "bd_upsample_conv_wgrad", _wgrad_desc(L, dw=None), ERR_INVALID, b"null pointer")
    _rejects(lib, "bd_upsample_conv_wgrad", _wgrad_desc(L, mode=0x10), ERR_INVALID, b"mode")


def test_workspace_rejections():
    """BD_ERR_WORKSPACE: a tap-split data gradient with a null or short workspace, the weight gradient likewise (it always needs one)"""
    _table_holds_here()
    L, lib = _lib()
    need = lib.bd_upsample_conv_dgrad_workspace_bytes(ctypes.byref(_dgrad_desc(L)))
    assert need == 4 * 16 * 128 * 4                                                   # the default descriptor is a tap-split shape
    _rejects(lib, "bd_upsample_conv_dgrad", _dgrad_desc(L, workspace=None), ERR_WORKSPACE, b"workspace")
    _rejects(lib, "bd_upsample_conv_dgrad", _dgrad_desc(L, workspace_bytes=need - 1), ERR_WORKSPACE, b"workspace")
    _rejects(lib, "bd_upsample_conv_dgrad", _dgrad_desc(L, workspace_bytes=0), ERR_WORKSPACE, b"workspace")
    need = lib.bd_upsample_conv_wgrad_workspace_bytes(ctypes.byref(_wgrad_desc(L)))
    assert need == (1 * (16 * 128 * 128 + 4 * 128) + 16 * 128 * 128) * 4
    _rejects(lib, "bd_upsample_conv_wgrad", _wgrad_desc(L, workspace=None), ERR_WORKSPACE, b"workspace")
    _rejects(lib, "bd_upsample_conv_wgrad", _wgrad_desc(L, workspace_bytes=need - 1), ERR_WORKSPACE, b"workspace")
    assert lib.bd_upsample_conv_dgrad_workspace_bytes(None) == 0 and lib.bd_upsample_conv_wgrad_workspace_bytes(None) == 0


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != EXPECTED_CUS:
        pytest.skip(f"the branch tables are for {EXPECTED_CUS} CUs, this device reports {cus}")
    from baddiffusion_amd import ops as o
    return o


def padded_planes(dense, pad):
    """dense split planes [rows, C/32, 2, 32] -> the same rows inside a buffer of leading dimension C + pad whose pad blocks hold a bf16 NaN"""
    if not pad:
        return dense
    assert pad % 32 == 0
    buf = torch.full((dense.shape[0], dense.shape[1] + pad // 32, 2, 32), SENTINEL, dtype=torch.int16, device=dense.device)
    buf[:, :dense.shape[1]] = dense
    return buf


def out_buffer(rows, N, pad, prev=None):
    """NaN-filled [rows + GUARD, N + pad]; prev (the previous output of an accumulating call) goes into the [rows, N] window"""
    buf = torch.full((rows + GUARD, N + pad), float("nan"), device="cuda")
    if prev is not None:
        buf[:rows, :N] = prev.reshape(rows, N)
    return buf


def check_window(buf, rows, N, ref, what):
    got = buf[:rows, :N]
    assert torch.equal(got.double().cpu(), ref.reshape(rows, N)), (*what, describe(got, ref.reshape(rows, N)))
    assert bool(torch.isnan(buf[rows:]).all()), (*what, "store past the last row")
    assert bool(torch.isnan(buf[:, N:]).all()), (*what, "store into the pad columns")


def ph_launches(counts):
    return {k: v for k, v in counts.items() if k.startswith("conv_p")}


def cls_name(base, mode):
    return base + ("_bf16" if mode == BF16 else "")


def run_ups_fwd(case, xs, e, bias, mode, pad):
    """bd_upsample_conv_fwd into a fresh NaN buffer -> the buffer [4 M + GUARD, Cout + pad]"""
    L, lib = _lib()
    B, H, W, Cin, Cout = case
    buf = out_buffer(4 * B * H * W, Cout, pad)
    d = L.UpsampleConvDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, x_split=L.ptr(xs), ldx=xs.shape[1] * 32, e_split=L.ptr(e), bias=L.ptr(bias),
                           y=L.ptr(buf), ldy=buf.shape[1], mode=mode)
    L.check(lib.bd_upsample_conv_fwd(ctypes.byref(d), L.stream()), "bd_upsample_conv_fwd")
    return buf


def run_ups_dgrad(case, dys, et, prev, mode, pad):
    """bd_upsample_conv_dgrad with exactly the workspace its query asks for (none when it asks for none) -> [M + GUARD, Cin + pad]"""
    L, lib = _lib()
    B, H, W, Cout, Cin = case
    buf = out_buffer(B * H * W, Cin, pad, prev)
    d = L.UpsampleConvDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, dy_split=L.ptr(dys), lddy=dys.shape[1] * 32, et_split=L.ptr(et),
                           dx=L.ptr(buf), lddx=buf.shape[1], accumulate=int(prev is not None), mode=mode)
    need = lib.bd_upsample_conv_dgrad_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda") if need else None
    d.workspace = L.ptr(ws); d.workspace_bytes = need
    L.check(lib.bd_upsample_conv_dgrad(ctypes.byref(d), L.stream()), "bd_upsample_conv_dgrad")
    return buf


def run_s2_dgrad(case, dys, wt, prev, mode, pad_cols, pad):
    L, lib = _lib()
    B, Ho, Wo, Cout, Cin = case
    buf = out_buffer(4 * B * Ho * Wo, Cin, pad_cols, prev)
    d = L.ConvS2DgradDesc(B=B, Ho=Ho, Wo=Wo, Cin=Cin, Cout=Cout, pad=pad, dy_split=L.ptr(dys), lddy=dys.shape[1] * 32, wT_split=L.ptr(wt),
                          dx=L.ptr(buf), lddx=buf.shape[1], accumulate=int(prev is not None), mode=mode)
    L.check(lib.bd_conv3x3_s2_dgrad_ps(ctypes.byref(d), L.stream()), "bd_conv3x3_s2_dgrad_ps")
    return buf


def run_ups_wgrad(case, xs, dys, with_db, mode):
    """bd_upsample_conv_wgrad with exactly the workspace its query asks for -> (dw buffer [Cout + GUARD, 9 Cin], db buffer [1 + GUARD, Cout] or None)"""
    L, lib = _lib()
    B, H, W, Cin, Cout = case
    dw = out_buffer(Cout, 9 * Cin, 0)
    db = out_buffer(1, Cout, 0) if with_db else None
    d = L.UpsampleConvDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, x_split=L.ptr(xs), ldx=xs.shape[1] * 32, dy_split=L.ptr(dys),
                           lddy=dys.shape[1] * 32, dw=L.ptr(dw), db=L.ptr(db), mode=mode)
    need = lib.bd_upsample_conv_wgrad_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    d.workspace = L.ptr(ws); d.workspace_bytes = need
    L.check(lib.bd_upsample_conv_wgrad(ctypes.byref(d), L.stream()), "bd_upsample_conv_wgrad")
    return dw, db


@gpu
@pytest.mark.parametrize("cid,opset", ids(FWD_CASES))
def test_upsample_fwd_branch_is_exact(ops, cid, opset):
    """bd_upsample_conv_fwd (four classes of 2x2 taps, scattered to the fine grid) equals the fp64 reference in both modes, with bias and
    without (bias == NULL is a path of its own in ph_epilogue); nothing behind the last row is written"""
    case = FWD_CASES[cid][:5]
    B, H, W, Cin, Cout = case
    o = fwd_operands(cid, opset)
    xs = ops.split_rows(o["x"].cuda()); e, _ = ops.upsample_weights(o["w"].cuda()); bias = o["bias"].cuda()
    for mode in MODES:
        ref = fwd_ref(cid, opset, mode)
        buf, counts = bracketed(lambda: run_ups_fwd(case, xs, e, bias, mode, 0))
        assert ph_launches(counts) == {cls_name("conv_ph_ups_fwd", mode): 1}, (cid, mode, counts)
        check_window(buf, 4 * B * H * W, Cout, ref + o["bias"].double(), (cid, opset, mode, "bias"))
        check_window(run_ups_fwd(case, xs, e, None, mode, 0), 4 * B * H * W, Cout, ref, (cid, opset, mode, "no bias"))


@gpu
@pytest.mark.parametrize("cid,opset", ids(DGRAD_CASES))
def test_upsample_dgrad_branch_is_exact(ops, cid, opset):
    """bd_upsample_conv_dgrad on the pinned branch (tap split + ph_tsplit_reduce, or the one-workgroup 16-tap form with no workspace at all)
    equals the fp64 reference in both modes, plain and accumulating over a previous dx"""
    L, lib = _lib()
    case = DGRAD_CASES[cid][:5]
    B, H, W, Cout, Cin = case
    groups = DGRAD_CASES[cid][5]
    M = B * H * W
    assert dgrad_workspace_bytes(lib, L, *case) == (4 * M * Cin * 4 if groups == 4 else 0), cid      # the branch, before anything is launched
    o = dgrad_operands(cid, opset)
    dys = ops.split_rows(o["dy"].cuda()); _, et = ops.upsample_weights(o["w"].cuda()); prev = o["prev"].cuda()
    for mode in MODES:
        ref = dgrad_ref(cid, opset, mode)
        buf, counts = bracketed(lambda: run_ups_dgrad(case, dys, et, None, mode, 0))
        assert ph_launches(counts) == {cls_name("conv_ph_ups_dgrad", mode): 1}, (cid, mode, counts)
        check_window(buf, M, Cin, ref, (cid, opset, mode, "plain"))
        check_window(run_ups_dgrad(case, dys, et, prev, mode, 0), M, Cin, ref + o["prev"].double(), (cid, opset, mode, "accumulate"))


@gpu
@pytest.mark.parametrize("cid,opset", ids(S2_CASES))
def test_stride2_dgrad_branch_is_exact(ops, cid, opset):
    """bd_conv3x3_s2_dgrad_ps (parity classes of 4 / 2 / 2 / 1 taps in one launch) equals fp64 autograd in both modes and paddings, plain and
    accumulating"""
    case = S2_CASES[cid][:5]
    B, Ho, Wo, Cout, Cin = case
    rows = 4 * B * Ho * Wo
    o = s2_operands(cid, opset)
    dys = ops.split_rows(o["dy"].cuda()); wt = ops.split_wT(o["w"].cuda()); prev = o["prev"].cuda()
    for pad in S2_CASES[cid][5]:
        for mode in MODES:
            ref = s2_ref(cid, opset, mode, pad)
            buf, counts = bracketed(lambda: run_s2_dgrad(case, dys, wt, None, mode, 0, pad))
            assert ph_launches(counts) == {cls_name("conv_ph_s2_dgrad", mode): 1}, (cid, mode, counts)
            check_window(buf, rows, Cin, ref, (cid, opset, mode, pad, "plain"))
            check_window(run_s2_dgrad(case, dys, wt, prev, mode, 0, pad), rows, Cin, ref + o["prev"].double(), (cid, opset, mode, pad, "accumulate"))


@gpu
@pytest.mark.parametrize("cid,opset", ids(WGRAD_CASES))
def test_upsample_wgrad_branch_is_exact(ops, cid, opset):
    """bd_upsample_conv_wgrad (PHASE form of conv_ps_wgrad_kernel -> slabs -> conv_ps_wgrad_reduce<false> with 4 * ksplit bias rows ->
    ups_dweff_combine) on the pinned K split: dw equals fp64 autograd of the literal form, db the fp64 sum of the unrounded dY in both modes,
    and dw without db is the same dw"""
    L, lib = _lib()
    case = WGRAD_CASES[cid][:5]
    B, H, W, Cin, Cout = case
    assert wgrad_split(lib, L, *case)[:3] == WGRAD_CASES[cid][5:8], cid                              # the branch, before anything is launched
    o = wgrad_operands(cid, opset)
    xs, dys = ops.split_rows(o["x"].cuda()), ops.split_rows(o["dy"].cuda())
    db_ref = o["dy"].double().sum(dim=(0, 1, 2))
    for mode in MODES:
        dw_ref = wgrad_ref(cid, opset, mode)
        (dw, db), counts = bracketed(lambda: run_ups_wgrad(case, xs, dys, True, mode))
        assert ph_launches(counts) == {cls_name("conv_ph_ups_wgrad", mode): 1}, (cid, mode, counts)
        check_window(dw, Cout, 9 * Cin, dw_ref, (cid, opset, mode, "dw"))
        check_window(db, 1, Cout, db_ref, (cid, opset, mode, "db"))
        dw_only, _ = run_ups_wgrad(case, xs, dys, False, mode)
        check_window(dw_only, Cout, 9 * Cin, dw_ref, (cid, opset, mode, "dw without db"))


@gpu
@pytest.mark.parametrize("opset", "AB")
def test_strided_buffers_give_the_dense_result(ops, opset):
    """one case per entry point with leading dimensions wider than the channel count, as the plan lays its buffers out: the output has
    ld = N + 32 and its pad columns stay NaN; the input planes have ld = C + 32 with a bf16 NaN pattern in the pad block; the window equals the
    dense run and the reference"""
    for mode in MODES:
        cid = STRIDED["fwd"]; case = FWD_CASES[cid][:5]; B, H, W, Cin, Cout = case
        o = fwd_operands(cid, opset)
        xs = ops.split_rows(o["x"].cuda()); e, _ = ops.upsample_weights(o["w"].cuda()); bias = o["bias"].cuda()
        dense = run_ups_fwd(case, xs, e, bias, mode, 0)
        buf = run_ups_fwd(case, padded_planes(xs, PAD), e, bias, mode, PAD)
        check_window(buf, 4 * B * H * W, Cout, fwd_ref(cid, opset, mode) + o["bias"].double(), (cid, opset, mode, "strided"))
        assert torch.equal(buf[:4 * B * H * W, :Cout], dense[:4 * B * H * W])

        for cid in STRIDED["dgrad"]:
            case = DGRAD_CASES[cid][:5]; B, H, W, Cout, Cin = case
            o = dgrad_operands(cid, opset)
            dys = ops.split_rows(o["dy"].cuda()); _, et = ops.upsample_weights(o["w"].cuda()); prev = o["prev"].cuda()
            for pv in (None, prev):
                dense = run_ups_dgrad(case, dys, et, pv, mode, 0)
                buf = run_ups_dgrad(case, padded_planes(dys, PAD), et, pv, mode, PAD)
                ref = dgrad_ref(cid, opset, mode) + (o["prev"].double() if pv is not None else 0)
                check_window(buf, B * H * W, Cin, ref, (cid, opset, mode, "strided", pv is not None))
                assert torch.equal(buf[:B * H * W, :Cin], dense[:B * H * W])

        cid = STRIDED["s2"]; case = S2_CASES[cid][:5]; B, Ho, Wo, Cout, Cin = case
        o = s2_operands(cid, opset)
        dys = ops.split_rows(o["dy"].cuda()); wt = ops.split_wT(o["w"].cuda()); prev = o["prev"].cuda()
        for pad in S2_CASES[cid][5]:
            for pv in (None, prev):
                dense = run_s2_dgrad(case, dys, wt, pv, mode, 0, pad)
                buf = run_s2_dgrad(case, padded_planes(dys, PAD), wt, pv, mode, PAD, pad)
                ref = s2_ref(cid, opset, mode, pad) + (o["prev"].double() if pv is not None else 0)
                check_window(buf, 4 * B * Ho * Wo, Cin, ref, (cid, opset, mode, pad, "strided", pv is not None))
                assert torch.equal(buf[:4 * B * Ho * Wo, :Cin], dense[:4 * B * Ho * Wo])

        cid = STRIDED["wgrad"]; case = WGRAD_CASES[cid][:5]; B, H, W, Cin, Cout = case
        o = wgrad_operands(cid, opset)
        xs, dys = ops.split_rows(o["x"].cuda()), ops.split_rows(o["dy"].cuda())
        dw, db = run_ups_wgrad(case, padded_planes(xs, PAD), padded_planes(dys, PAD), True, mode)
        check_window(dw, Cout, 9 * Cin, wgrad_ref(cid, opset, mode), (cid, opset, mode, "strided dw"))
        check_window(db, 1, Cout, o["dy"].double().sum(dim=(0, 1, 2)), (cid, opset, mode, "strided db"))


# ------------------------------------------------------------------------------------------------ bd_upsample_weights
def _upsample_weights(w, with_et):
    """bd_upsample_weights into sentinel-filled plane buffers with a guard band of rows -> (rc, E planes, E^T planes or None)"""
    L, lib = _lib()
    Cout, _, _, Cin = w.shape
    e = torch.full((Cout + 8, 16 * Cin // 32, 2, 32), SENTINEL, dtype=torch.int16, device="cuda")
    et = torch.full((Cin + 8, 16 * Cout // 32, 2, 32), SENTINEL, dtype=torch.int16, device="cuda") if with_et else None
    rc = lib.bd_upsample_weights(L.ptr(w), Cin, Cout, L.ptr(e), L.ptr(et), L.stream())
    torch.cuda.synchronize()
    return rc, e, et


@gpu
@pytest.mark.parametrize("Cin,Cout", [(64, 96), (128, 256)])
@pytest.mark.parametrize("kind", ["wide", "narrow", "randn"])
def test_upsample_weights_planes_are_the_split_of_E(ops, Cin, Cout, kind):
    """the E planes [Cout][16][Cin] and the E^T planes [Cin][16][Cout] are, bit for bit, hi = bf16(E), lo = bf16(E - hi) of the fp32 sum in the
    kernel's stated order (grid weights: that sum is exact; randn weights: reproduced in numpy fp32); with et_split == NULL (inference) the
    call returns 0 and writes the same E planes"""
    g = torch.Generator().manual_seed(Cin + Cout)
    w = {"wide": _wide, "narrow": _narrow, "randn": lambda g, *s: torch.randn(*s, generator=g)}[kind](g, Cout, 3, 3, Cin)
    E = E_of(w)                                                   # float32, the kernel's order
    if kind != "randn":
        assert torch.equal(E.double(), E_of(w.double()))
    e_ref = planes(E.reshape(Cout, 16 * Cin)); et_ref = planes(E.permute(3, 1, 2, 0).reshape(Cin, 16 * Cout))
    rc, e, et = _upsample_weights(w.cuda(), True)
    assert rc == OK
    assert torch.equal(e[:Cout].cpu(), e_ref), describe_planes(e[:Cout], e_ref)
    assert torch.equal(et[:Cin].cpu(), et_ref), describe_planes(et[:Cin], et_ref)
    assert bool((e[Cout:] == SENTINEL).all()) and bool((et[Cin:] == SENTINEL).all())
    rc, e2, _ = _upsample_weights(w.cuda(), False)
    assert rc == OK and torch.equal(e2, e)


# ------------------------------------------------------------------------------------------------ the literal path's small pieces
@gpu
def test_split_rows_ups2_is_the_split_of_the_upsampled_tensor(ops):
    """bd_split_rows_ups2 (the literal path the phase forms replace, and the plan's fallback): bit-equal to bd_split_rows of the nearest-upsampled
    tensor and to the documented split; a ragged shape (neither H nor W a power of two, rows no multiple of the block)"""
    B, H, W, C = 3, 3, 5, 96
    g = torch.Generator().manual_seed(11)
    x = torch.cat([torch.randn(B, H, W, C // 2, generator=g), _wide(g, B, H, W, C // 2)], dim=-1)
    up = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()
    assert torch.equal(up, F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest").permute(0, 2, 3, 1))
    got = ops.split_rows_ups2(x.cuda())
    want = ops.split_rows(up.cuda())
    ref = planes(up.reshape(-1, C))
    assert torch.equal(got, want.reshape(got.shape)), describe_planes(got, want.reshape(got.shape).cpu())
    assert torch.equal(got.cpu(), ref), describe_planes(got, ref)


@gpu
@pytest.mark.parametrize("accumulate", [False, True])
def test_sum2x2_is_exact_on_padded_buffers(ops, accumulate):
    """bd_sum2x2 (the nearest upsampling's backward): grid values, equality with the fp64 2x2 sum, with and without accumulate, ldu and lddx
    wider than C, pad columns and the rows behind the last one untouched"""
    L, lib = _lib()
    B, H, W, C = 3, 3, 5, 36
    g = torch.Generator().manual_seed(12 + accumulate)
    du = _wide(g, B, 2 * H, 2 * W, C); prev = _quarters(g, B, H, W, C)
    ref = du.double().reshape(B, H, 2, W, 2, C).sum(dim=(2, 4)) + (prev.double() if accumulate else 0)
    src = torch.full((B * 4 * H * W, C + 4), float("nan"), device="cuda")
    src[:, :C] = du.reshape(-1, C).cuda()
    buf = out_buffer(B * H * W, C, 8, prev.cuda() if accumulate else None)
    L.check(lib.bd_sum2x2(L.ptr(src), src.shape[1], L.ptr(buf), buf.shape[1], B, H, W, C, int(accumulate), L.stream()), "bd_sum2x2")
    check_window(buf, B * H * W, C, ref, ("sum2x2", accumulate))
