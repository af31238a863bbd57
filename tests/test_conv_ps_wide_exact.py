"""Exact-value tests for what tests/test_conv_ps_dispatch.py leaves open on the stride-1 split-plane 3x3 convolutions (bd_conv3x3_ps,
bd_conv3x3_ps_wgrad: csrc/conv_ps.hip), in that file's manner and with its operand grids and helpers:

  1 / 2  32-pixel rows on the vertical-tap-sharing kernels (the 320-row LDS window of conv_ps3_kernel, 96 of the 128 ring pixels of
         conv_ps_wgrad3_kernel), images WIDER than 32 pixels (strip order, ps_v2r: a tap dropped at the seam between columns 31 | 32, or on
         the first row of a strip, whose virtual predecessor belongs to the strip before), odd counts of (channel block, kx) groups
         (K = 32, 96: conv_ps3_kernel's two-per-trip loop leaves after its first half), and a wide image on the two kernels that keep the
         real pixel order (conv_ps128 + reduce, conv_ps_kernel);
  3      leading dimensions wider than the channel count, as the network plan passes them (concat buffers, column blocks, a gradient
         accumulated into a block of a wider buffer): the operand is channel blocks [1, 1 + K/32) of planes (K + 64) channels wide whose
         other blocks hold a bf16 NaN in both halves, y columns [16, 16 + N) of an (N + 32)-wide NaN buffer, the residual columns [4, 4 + N)
         of (N + 8), the row bias has ld N + 4; the window equals the fp64 reference and everything outside it is still NaN;
  4      the GroupNorm-partials epilogue (gn_part): EVERY partial [sample, virtual 256-pixel tile, group] equals the fp64 sum of the
         reference over that tile and group.  bd_gn_fwd only needs the sum over the tiles of a sample, so tiles written to each other's
         slots inside one sample would be harmless to the network -- and invisible to a test that sums the partials first.  It must still
         show up here: the slot order is part of what the ABI documents.
  5      the launchers refuse a leading dimension below the channel count (BD_ERR_INVALID, nothing launched, outputs untouched).

The standard is test_conv_ps_dispatch.py's: set A = WIDE x NARROW, set B = NARROW x WIDE, both compute modes; in BD_MODE_BF16 the reference
contracts the bf16-rounded operands and differs from the three-product one (asserted); torch.equal against fp64; every output sits in a
NaN-filled buffer with a 256-row guard band that must stay NaN.  Host tests (no GPU) prove for every case and set that every partial sum
stays below 2^24 grid units (MEASURE exact_units lines), so equality is a condition of the data, not a tolerance.

The GroupNorm cases use data for which any fp32 order of the epilogue's sums of y and y * y is exact: x and w ternary {0, +-1} with
P(nonzero) = 3/8, bias and row bias integers in [-2, 2], residual a multiple of 1/4 in [-2, 2], out_scale 0.5: y lies on the grid u = 1/2
(row bias form) or 1/8 (residual form), and test_gn_data_keeps_every_partial_exact proves sum |y| / u < 2^24 and sum (y / u)^2 < 2^24 per
(sample, tile, group) -- every term of the second sum is non-negative, so the total bounds every partial sum.

The branch of every case is asserted from the ABI's plan queries before anything is launched: bd_conv3x3_ps_plan (kernel, K split, and
gn_splits, which bd_conv3x3_ps_gn_splits repeats) and bd_conv3x3_ps_wgrad_plan (kernel, K split, chunks per slice); the profiling class
behind the launch shows that the launcher ran what the plan said.  The tables are derived by hand from ps_plan, ps_wgrad_plan and split_k
at 256 CUs (K-split slots of the strip-order weight gradient: 192 for W <= 32, 128 for W > 32; at least 8 chunks per slice; tiles =
Cout/128 * 3 Cin/128); on another device the GPU tests skip.  Whoever retunes those functions moves the cases with them (DESIGN.md,
"Dispatch branches of the split-plane convolutions").

Observed on MI355X (256 CUs): see DESIGN.md, same paragraph."""
import ctypes
import functools

import pytest
import torch

import tests.test_conv_ph_dispatch as PH
import tests.test_conv_ps_dispatch as D
from tests.test_gemm_sp_dispatch import SENTINEL

gpu = pytest.mark.gpu       # per test: the tables, preconditions and rejections run without a device

BF16X3, BF16 = D.BF16X3, D.BF16
MODES = (BF16X3, BF16)
UNIT = D.UNIT
GUARD = PH.GUARD
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -2
cdiv = lambda a, b: -(-a // b)

# id: (B, H, W, K, N, directions, kernel, ksplit, what the case is there for).  V1 .. S4: M = 24576 is the smallest large layer
# (96 tiles of 256 x 128)
FWD_CASES = {
    "V1": (24, 32, 32, 32, 128, (1, -1), "conv_ps3", 1, "W = 32: the 320-row window; 3 groups: the loop leaves after its first half; 4 tiles per image: top, two interior, bottom"),
    "V2": (8, 32, 32, 96, 384, (1,), "conv_ps3", 1, "9 groups (odd, more than one trip); three N tiles in the XCD order"),
    "S1": (48, 8, 64, 32, 128, (1, -1), "conv_ps3", 1, "strip = one tile: every tile touches the image's top and bottom rows; seam at columns 31 | 32"),
    "S2": (6, 64, 64, 64, 128, (1, -1), "conv_ps3", 1, "strip = 8 tiles: interior tiles; first and last tile of a strip next to another strip's rows in virtual order"),
    "S3": (12, 8, 256, 32, 128, (-1,), "conv_ps3", 1, "8 strips, widest row pitch, non-square"),
    "S4": (3, 128, 64, 32, 128, (1,), "conv_ps3", 1, "tall non-square; 16 tiles per strip"),
    "O1": (1, 8, 64, 64, 128, (1, -1), "conv_ps128", 4, "a wide image on the small-layer kernel (real pixel order, W = 64 border tests): 5, 5, 5, 3 chunks, four-stage ring + reduce"),
    "O2": (96, 4, 64, 32, 128, (1,), "conv_ps", 1, "a wide image on the general large kernel (H * 32 % 256 != 0)"),
}
# id: (B, H, W, Cin, Cout, ksplit, chunks per slice, chunks of the last slice, what for): all on conv_ps_wgrad3_kernel
WGRAD_CASES = {
    "X1": (1, 32, 32, 128, 128, 4, 8, 8, "W = 32; slices start inside an image (halo chunk from the slice before)"),
    "X2": (7, 16, 32, 256, 384, 10, 12, 4, "ragged last slice; slices start mid-image; two ci tiles per kx; three co tiles"),
    "X3": (3, 8, 64, 512, 256, 5, 10, 8, "strip order; slices start mid-strip and mid-image; ragged"),
    "X4": (1, 16, 128, 128, 128, 8, 8, 8, "4 strips of 16 chunks; slices start at a strip's top and at its middle"),
    "X5": (1, 8, 256, 128, 128, 8, 8, 8, "slice = strip: the halo chunk is the previous strip's last row and must be skipped"),
    "X6": (1, 16, 16, 128, 128, 1, 8, 8, "unsplit: written straight to dw / db"),
    "X7": (1, 4, 64, 128, 128, 1, 8, 8, "strip order, unsplit; 4-row strips"),
}
# id: (B, H, W, K, N, group counts): channels per group 4 and 32, 8 and 16, 4 and 16
GN_CASES = {
    "N1": (24, 32, 32, 32, 128, (32, 4)),
    "N2": (12, 32, 32, 32, 256, (32, 16)),      # two N tiles: group index offset n0 >> lcpg
    "N3": (6, 64, 64, 32, 128, (32, 8)),        # strip order
}
# padded leading dimensions: (case, direction); P5, P7, W1, W4 are test_conv_ps_dispatch.py's (conv_ps128 in-kernel epilogue, ragged; two-stage
# split; conv_ps_wgrad_kernel split with a ragged last chunk, and unsplit)
PADDED_FWD = [("V2", 1), ("S2", 1), ("S2", -1), ("O1", 1), ("O1", -1), ("O2", 1), ("P5", 1), ("P7", 1)]
PADDED_WGRAD = ["X2", "X3", "W1", "W4"]

FWD_PARAMS = [pytest.param(cid, d, s, id=f"{cid}-{'fwd' if d > 0 else 'dgrad'}-{s}") for cid, c in FWD_CASES.items() for d in c[5] for s in "AB"]
WGRAD_PARAMS = [pytest.param(cid, s, id=f"{cid}-{s}") for cid in WGRAD_CASES for s in "AB"]
PADDED_FWD_PARAMS = [pytest.param(cid, d, s, id=f"{cid}-{'fwd' if d > 0 else 'dgrad'}-{s}") for cid, d in PADDED_FWD for s in "AB"]
PADDED_WGRAD_PARAMS = [pytest.param(cid, s, id=f"{cid}-{s}") for cid in PADDED_WGRAD for s in "AB"]
GN_PARAMS = [pytest.param(cid, epi, id=f"{cid}-{'residual' if epi == 1 else 'rowbias'}") for cid in GN_CASES for epi in (1, 2)]
SEED = {"V": 11000, "S": 12000, "O": 13000, "X": 14000, "N": 15000}


# ------------------------------------------------------------------------------------------------ operands and fp64 references (CPU)
def fwd_shape(cid):
    return (FWD_CASES.get(cid) or D.FWD_CASES[cid])[:5]


def wgrad_shape(cid):
    return (WGRAD_CASES.get(cid) or D.WGRAD_CASES[cid])[:5]


@functools.lru_cache(maxsize=2)
def fwd_operands(cid, direction, opset):
    """as test_conv_ps_dispatch.fwd_operands (whose own cases are handed through): direction -1 contracts dY [B,H,W,K] with the transpose planes
    of the weight [Cout = K][3][3][Cin = N]"""
    if cid in D.FWD_CASES:
        return D.fwd_operands(cid, direction, opset)
    B, H, W, K, N = FWD_CASES[cid][:5]
    g = torch.Generator().manual_seed(SEED[cid[0]] + 100 * int(cid[1:]) + 10 * (direction > 0) + (opset == "A"))
    a_gen, w_gen = (D._wide, D._narrow) if opset == "A" else (D._narrow, D._wide)
    wshape = (N, 3, 3, K) if direction > 0 else (K, 3, 3, N)
    return dict(x=a_gen(g, B, H, W, K), w=w_gen(g, *wshape), bias=D._quarters(g, N), rowbias=D._quarters(g, B, N),
                residual=D._quarters(g, B, H, W, N), prev=D._quarters(g, B, H, W, N))


@functools.lru_cache(maxsize=2)
def wgrad_operands(cid, opset):
    if cid in D.WGRAD_CASES:
        return D.wgrad_operands(cid, opset)
    B, H, W, Cin, Cout = WGRAD_CASES[cid][:5]
    g = torch.Generator().manual_seed(SEED[cid[0]] + 100 * int(cid[1:]) + (opset == "A"))
    x_gen, dy_gen = (D._wide, D._narrow) if opset == "A" else (D._narrow, D._wide)
    return dict(x=x_gen(g, B, H, W, Cin), dy=dy_gen(g, B, H, W, Cout))


def prep_of(mode):
    """what the mode multiplies: the operands, or their bf16 roundings"""
    return D.rnd if mode == BF16 else (lambda t: t)


def conv_ref(cid, direction, opset, mode):
    o = fwd_operands(cid, direction, opset)
    return D.conv64(prep_of(mode)(o["x"]), prep_of(mode)(o["w"]), direction)


def wgrad_ref(cid, opset, mode):
    o = wgrad_operands(cid, opset)
    return D.wgrad64(prep_of(mode)(o["x"]), prep_of(mode)(o["dy"]))


def _ternary(g, *shape):
    """{0, +-1}, P(nonzero) = 3/8"""
    t = torch.randint(0, 16, shape, generator=g)
    return (t < 3).float() - ((t >= 3) & (t < 6)).float()


@functools.lru_cache(maxsize=None)
def gn_operands(cid):
    B, H, W, K, N, _ = GN_CASES[cid]
    g = torch.Generator().manual_seed(SEED["N"] + int(cid[1:]))
    return dict(x=_ternary(g, B, H, W, K), w=_ternary(g, N, 3, 3, K), bias=torch.randint(-2, 3, (N,), generator=g).float(),
                rowbias=torch.randint(-2, 3, (B, N), generator=g).float(), residual=D._quarters(g, B, H, W, N))


@functools.lru_cache(maxsize=None)
def gn_ref(cid, epi):
    """fp64 y [B,H,W,N] of the case: one reference for the host proof and the GPU test, both modes (ternary operands are bf16 numbers)"""
    o = gn_operands(cid)
    assert torch.equal(D.rnd(o["x"]), o["x"]) and torch.equal(D.rnd(o["w"]), o["w"])
    return D.epilogue64(D.conv64(o["x"], o["w"], 1), o, epi, bias=True)


def tile_sums(y, G):
    """fp64 (sum, sum of squares) of y [B,H,W,N] per sample, VIRTUAL 256-pixel tile and group -> [B, HW/256, G, 2].  W <= 32: tile s is pixels
    [256 s, 256 s + 256).  W > 32: virtual pixel v = strip * (H * 32) + y * 32 + (x mod 32), s = v >> 8 (conv_ps.hip, ps_v2r)"""
    B, H, W, N = y.shape
    if W > 32:
        y = y.reshape(B, H, W // 32, 32, N).permute(0, 2, 1, 3, 4)
    t = y.reshape(B, H * W // 256, 256, G, N // G)
    return torch.stack([t.sum(dim=(2, 4)), (t * t).sum(dim=(2, 4))], dim=-1)


# ------------------------------------------------------------------------------------------------ the tables, from the ABI (no GPU)
def plan_of(lib, L, fn, d, info):
    L.check(getattr(lib, fn)(ctypes.byref(d), ctypes.byref(info)), fn)
    return info


def fwd_plan(lib, L, shape, gn_groups=0):
    """bd_conv3x3_ps_plan of a dense forward call of the shape"""
    B, H, W, K, N = shape
    return plan_of(lib, L, "bd_conv3x3_ps_plan", L.ConvPsDesc(B=B, H=H, W=W, K=K, N=N, direction=1, ldx=K, ldy=N, gn_groups=gn_groups, mode=BF16X3),
                   L.ConvPsPlanInfo())


def assert_fwd_branch(lib, L, cid):
    B, H, W, K, N, _, kernel, ksplit, _ = FWD_CASES[cid]
    p = fwd_plan(lib, L, (B, H, W, K, N), gn_groups=N // 4)
    assert p.ksplit == ksplit, (cid, p.ksplit)
    assert kernel == {L.PS_128: "conv_ps128", L.PS_256_SHARED_TAP: "conv_ps3", L.PS_256: "conv_ps"}[p.kernel], (cid, p.kernel)
    # the GroupNorm partials at 4 channels per group: one split per virtual tile exactly where conv_ps3_kernel runs; the older query repeats it
    assert p.gn_splits == lib.bd_conv3x3_ps_gn_splits(B, H, W, K, N, N // 4) == (H * W // 256 if kernel == "conv_ps3" else 0), (cid, p.gn_splits)
    cls = "conv_ps128" if p.kernel == L.PS_128 else "conv_ps"                # the profiling class confirms it at the launch
    assert p.prof_class.decode() == cls + "_fwd", (cid, p.prof_class)
    return cls


def wgrad_split(lib, L, shape):
    """(ksplit, chunks per slice, chunks of the last slice) from bd_conv3x3_ps_wgrad_plan; the kernel must be conv_ps_wgrad3_kernel"""
    B, H, W, Cin, Cout = shape
    p = plan_of(lib, L, "bd_conv3x3_ps_wgrad_plan", L.ConvPsWgradDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, ldx=Cin, lddy=Cout, mode=BF16X3),
                L.ConvPsWgradPlanInfo())
    assert p.kernel == L.PS_WGRAD_SHARED_TAP and p.prof_class == b"conv_ps_wgrad3", (shape, p.kernel, p.prof_class)
    return p.ksplit, p.chunks_per_split, cdiv(B * H * W, 32) - (p.ksplit - 1) * p.chunks_per_split


def test_case_tables_follow_the_dispatch_rules():
    """every branch named in the tables, from the ABI's queries (256 CUs: what the host assumes without a device)"""
    PH._table_holds_here()
    L, lib = PH._lib()
    for cid, c in FWD_CASES.items():
        assert_fwd_branch(lib, L, cid)
        if cid[0] in "VS":
            assert cdiv(c[0] * c[1] * c[2], 256) * (c[4] // 128) == 96, cid       # the smallest large layer
    assert (3 * FWD_CASES["V1"][3] // 32, 3 * FWD_CASES["V2"][3] // 32) == (3, 9)  # odd counts of (channel block, kx) groups
    assert (18, 5) == (9 * FWD_CASES["O1"][3] // 32, cdiv(18, 4))                 # O1: 5 + 5 + 5 + 3 chunks, <= 9 per slice: the four-stage ring
    assert FWD_CASES["O2"][1] * 32 % 256 != 0
    for cid, c in WGRAD_CASES.items():
        assert wgrad_split(lib, L, c[:5]) == c[5:8], (cid, wgrad_split(lib, L, c[:5]))   # (on conv_ps_wgrad3_kernel: wgrad_split asserts it)
    # the GroupNorm partials: one split per virtual tile where conv_ps3_kernel runs and the group is 4 .. 32 channels, else none
    q = lib.bd_conv3x3_ps_gn_splits
    for cid, (B, H, W, K, N, groups) in GN_CASES.items():
        for G in groups:
            assert q(B, H, W, K, N, G) == H * W // 256, (cid, G)
    assert q(8, 32, 32, 96, 384, 32) == 0                                           # 12 channels per group
    assert q(24, 32, 32, 32, 128, 64) == 0 and q(24, 32, 32, 32, 128, 2) == 0       # 2 and 64 channels per group
    assert q(24, 32, 32, 32, 128, 32) == 4
    assert q(*FWD_CASES["O1"][:5], 32) == 0 and q(*FWD_CASES["O2"][:5], 32) == 0   # conv_ps128 / conv_ps_kernel have no such epilogue


# ------------------------------------------------------------------------------------------------ the preconditions (no GPU)
@pytest.mark.parametrize("cid,direction,opset", FWD_PARAMS)
def test_operand_grids_keep_every_sum_exact(cid, direction, opset):
    """test_conv_ps_dispatch's proof for these cases: the convolution of the operand magnitudes plus the epilogue addends, in units of 2^-12,
    stays below 2^24; hi + lo == x with lo exact in bf16; at least half the wide values have a lo part"""
    o = fwd_operands(cid, direction, opset)
    D._check_split(o["x"], opset == "A"); D._check_split(o["w"], opset == "B")
    worst = D.conv64(D._mag(o["x"]), D._mag(o["w"]), direction)
    worst += o["bias"].abs().double() + o["rowbias"].abs().double()[:, None, None, :] + o["residual"].abs().double() + 2 * o["prev"].abs().double()
    units = float(worst.max()) / UNIT
    print(f"MEASURE exact_units {cid} dir {direction} set {opset} {units / 2 ** 24:.3f} x 2^24")
    assert units < 2 ** 24, units


@pytest.mark.parametrize("cid,opset", WGRAD_PARAMS)
def test_operand_grids_keep_every_wgrad_sum_exact(cid, opset):
    """the same for the weight gradient (sums over all P pixels; X2: P = 3584, 0.875 x 2^24 if every product were 1 -- the data's own bound is
    asserted) and the bias gradient (sums of the unrounded dy, grid 2^-11)"""
    o = wgrad_operands(cid, opset)
    D._check_split(o["x"], opset == "A"); D._check_split(o["dy"], opset == "B")
    units = float(D.wgrad64(D._mag(o["x"]), D._mag(o["dy"])).max()) / UNIT
    db_units = float(o["dy"].abs().double().sum(dim=(0, 1, 2)).max()) * 2048
    print(f"MEASURE exact_units {cid} set {opset} dw {units / 2 ** 24:.3f} db {db_units / 2 ** 24:.3f} x 2^24")
    assert units < 2 ** 24 and db_units < 2 ** 24, (units, db_units)


@pytest.mark.parametrize("cid,epi", GN_PARAMS)
def test_gn_data_keeps_every_partial_exact(cid, epi):
    """y lies on the grid u, and per (sample, virtual tile, group) sum |y| / u < 2^24 and sum (y / u)^2 < 2^24 for the LARGEST group of the
    case (a smaller group's sums are parts of it): every fp32 partial sum of y and of y * y, in any order, is exact"""
    B, H, W, K, N, groups = GN_CASES[cid]
    u = 0.125 if epi == 1 else 0.5
    y = gn_ref(cid, epi) / u
    assert torch.equal(y, y.round()), "y is not on the grid"
    G = min(groups)
    s1 = float(tile_sums(y.abs(), G)[..., 0].max()); s2 = float(tile_sums(y, G)[..., 1].max())
    print(f"MEASURE gn_bound {cid} epi {epi} G {G}: sum|y|/u {s1 / 2 ** 24:.3f} sum(y/u)^2 {s2 / 2 ** 24:.3f} x 2^24, max |y|/u {float(y.abs().max()):.0f}")
    assert s1 < 2 ** 24 and s2 < 2 ** 24, (s1, s2)
    assert float(y.abs().max()) ** 2 < 2 ** 24


# ------------------------------------------------------------------------------------------------ host rejections (no GPU, nothing launched)
DUMMY = PH.DUMMY            # a 128-byte aligned non-null address: never dereferenced, every call below fails a host check first


def _ps_desc(L, **kw):
    f = dict(B=1, H=8, W=8, K=64, N=128, direction=1, x_split=DUMMY, ldx=64, w_split=DUMMY, y=DUMMY, ldy=128, out_scale=1.0, mode=BF16X3)
    f.update(kw)
    return L.ConvPsDesc(**f)


def _ps_wgrad_desc(L, **kw):
    f = dict(B=1, H=8, W=8, Cin=256, Cout=256, x_split=DUMMY, ldx=256, dy_split=DUMMY, lddy=256, dw=DUMMY, workspace=DUMMY,
             workspace_bytes=1 << 40, mode=BF16X3)
    f.update(kw)
    return L.ConvPsWgradDesc(**f)


LD_REJECTIONS = [("bd_conv3x3_ps", _ps_desc, dict(ldx=32), b"ldx"), ("bd_conv3x3_ps", _ps_desc, dict(ldy=64), b"ldy"),
                 ("bd_conv3x3_ps", _ps_desc, dict(residual=DUMMY, ldr=64), b"ldr"),
                 ("bd_conv3x3_ps", _ps_desc, dict(rowbias=DUMMY, ld_rowbias=64), b"ld_rowbias"),
                 ("bd_conv3x3_ps_wgrad", _ps_wgrad_desc, dict(ldx=128), b"ldx"), ("bd_conv3x3_ps_wgrad", _ps_wgrad_desc, dict(lddy=128), b"lddy")]


@pytest.mark.parametrize("fn,make,kw,word", LD_REJECTIONS, ids=[f"{r[0]}-{r[3].decode()}" for r in LD_REJECTIONS])
def test_leading_dimension_below_the_channel_count_is_refused(fn, make, kw, word):
    """BD_ERR_INVALID before any launch (the pointers are never dereferenced): ldx < K, ldy < N, ldr < N with a residual, ld_rowbias < N with
    a row bias; ldx < Cin, lddy < Cout for the weight gradient.  (A null residual or row bias with ld 0 is what every dense GPU case passes.)"""
    L, lib = PH._lib()
    rc = getattr(lib, fn)(ctypes.byref(make(L, **kw)), None)
    msg = lib.bd_last_error() or b""
    assert rc == ERR_INVALID and word in msg and fn[3:].encode() in msg, (fn, kw, rc, msg)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != D.EXPECTED_CUS:
        pytest.skip(f"the branch tables are for {D.EXPECTED_CUS} CUs, this device reports {cus}")
    from baddiffusion_amd import ops as o
    return o


def place_planes(dense, padded):
    """dense split planes [rows, C/32, 2, 32] -> (tensor to keep alive, address of the operand, its leading dimension).  padded: the operand
    is channel blocks [1, 1 + C/32) of planes (C + 64) channels wide; the blocks on either side hold a bf16 NaN in both halves (one block =
    128 bytes: the base stays aligned)"""
    if not padded:
        return dense, dense.data_ptr(), dense.shape[1] * 32
    nb = dense.shape[1]
    buf = torch.full((dense.shape[0], nb + 2, 2, 32), SENTINEL, dtype=torch.int16, device=dense.device)
    buf[:, 1:1 + nb] = dense
    return buf, buf[:, 1:].data_ptr(), (nb + 2) * 32


def rows_in_nan(t, left, right):
    """fp32 [rows, N] -> (NaN buffer [rows, left + N + right] with t in columns [left, left + N), address of the window)"""
    buf = torch.full((t.shape[0], left + t.shape[1] + right), float("nan"), device=t.device)
    buf[:, left:left + t.shape[1]] = t
    return buf, buf[:, left:].data_ptr()


def run_conv(shape, direction, px, w_split, dev, epi, mode, padded, gn=None):
    """bd_conv3x3_ps through its descriptor, with exactly the workspace its query asks for, out_scale 0.5, bias on forward calls -> the NaN
    buffer [M + GUARD, N (+ 32)] that holds y (padded: in columns [16, 16 + N)).  gn = (part, groups): the GroupNorm partials as well"""
    L, lib = PH._lib()
    B, H, W, K, N = shape
    M = B * H * W
    left = 16 if padded else 0
    buf = PH.out_buffer(M, N, 2 * left)
    win = buf[:M, left:left + N]
    if epi & 4:
        win.copy_(dev["prev"].reshape(M, N))
    d = L.ConvPsDesc(B=B, H=H, W=W, K=K, N=N, direction=direction, x_split=px[1], ldx=px[2], w_split=L.ptr(w_split),
                     bias=L.ptr(dev["bias"]) if direction > 0 else None, out_scale=0.5, y=win.data_ptr(), ldy=buf.shape[1],
                     accumulate=int(bool(epi & 4)), mode=mode)
    keep = []
    if epi & 1:
        res, d.residual = rows_in_nan(dev["residual"].reshape(M, N), *((4, 4) if padded else (0, 0)))
        d.ldr = res.shape[1]; keep.append(res)
    if epi & 2:
        rb, d.rowbias = rows_in_nan(dev["rowbias"], 0, 4 if padded else 0)
        d.ld_rowbias = rb.shape[1]; keep.append(rb)
    if gn is not None:
        d.gn_part = L.ptr(gn[0]); d.gn_groups = gn[1]
    need = lib.bd_conv3x3_ps_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda") if need else None
    d.workspace = L.ptr(ws); d.workspace_bytes = need
    L.check(lib.bd_conv3x3_ps(ctypes.byref(d), L.stream()), "bd_conv3x3_ps")
    torch.cuda.synchronize()
    return buf


def run_wgrad(shape, px, pdy, with_db, mode):
    """bd_conv3x3_ps_wgrad with exactly the workspace its query asks for -> (dw buffer [Cout + GUARD, 9 Cin], db buffer [1 + GUARD, Cout] or None)"""
    L, lib = PH._lib()
    B, H, W, Cin, Cout = shape
    dw = PH.out_buffer(Cout, 9 * Cin, 0)
    db = PH.out_buffer(1, Cout, 0) if with_db else None
    d = L.ConvPsWgradDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, x_split=px[1], ldx=px[2], dy_split=pdy[1], lddy=pdy[2], dw=L.ptr(dw), db=L.ptr(db),
                          mode=mode)
    need = lib.bd_conv3x3_ps_wgrad_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda") if need else None
    d.workspace = L.ptr(ws); d.workspace_bytes = need
    L.check(lib.bd_conv3x3_ps_wgrad(ctypes.byref(d), L.stream()), "bd_conv3x3_ps_wgrad")
    torch.cuda.synchronize()
    return dw, db


def check_y(buf, shape, padded, ref, what):
    """the window equals ref; the guard rows and (padded) the 16 columns on either side are still NaN.  On failure: the image coordinates"""
    B, H, W, _, N = shape
    M = B * H * W
    left = 16 if padded else 0
    view = torch.cat([buf[:, left:], buf[:, :left]], dim=1) if left else buf        # the window first, every pad column behind it
    try:
        PH.check_window(view, M, N, ref, what)
    except AssertionError as e:
        if "store" in str(e):
            raise
        raise AssertionError((*what, D.describe(view[:M, :N], ref.reshape(M, N), grid=(H, W)))) from None


def describe_taps(dw, ref, Cout, Cin):
    """which taps (ky, kx) of a weight gradient differ: a wrong vertical neighbour shows as one tap"""
    bad = ~(dw.double().cpu().reshape(Cout, 3, 3, Cin) == ref.reshape(Cout, 3, 3, Cin))
    taps = [(ky, kx) for ky in range(3) for kx in range(3) if bool(bad[:, ky, kx].any())]
    return f"taps (ky, kx) that differ: {taps}; {D.describe(dw.reshape(Cout, -1), ref.reshape(Cout, -1))}"


def check_dw(dw, db, shape, dw_ref, db_ref, what):
    _, _, _, Cin, Cout = shape
    assert torch.equal(dw[:Cout].double().cpu(), dw_ref.reshape(Cout, 9 * Cin)), (*what, "dw", describe_taps(dw[:Cout], dw_ref, Cout, Cin))
    assert bool(torch.isnan(dw[Cout:]).all()), (*what, "dw: store past the last row")
    if db is not None:
        PH.check_window(db, 1, Cout, db_ref, (*what, "db"))


def conv_launches(counts):
    return {k: v for k, v in counts.items() if k.startswith("conv_ps")}


@gpu
@pytest.mark.parametrize("cid,direction,opset", FWD_PARAMS)
def test_wide_conv_branch_is_exact(ops, cid, direction, opset):
    """bd_conv3x3_ps on the pinned branch equals the fp64 convolution, in both modes, for every epilogue combination of {residual, row bias,
    accumulate} (forward: bias present; data gradient: EPI 0 and accumulate), out_scale 0.5"""
    L, lib = PH._lib()
    shape = FWD_CASES[cid][:5]
    cls = assert_fwd_branch(lib, L, cid) + ("_fwd" if direction > 0 else "_dgrad")       # the branch, before anything is launched
    o = fwd_operands(cid, direction, opset)
    dev = {k: v.cuda() for k, v in o.items()}
    px = place_planes(ops.split_rows(dev["x"]), False)
    ws = ops.split_bf16(dev["w"]) if direction > 0 else ops.split_wT(dev["w"])
    refs = {}
    for mode in MODES:
        conv = refs[mode] = conv_ref(cid, direction, opset, mode)
        for n_epi, epi in enumerate(range(8) if direction > 0 else (0, 4)):
            run = lambda: run_conv(shape, direction, px, ws, dev, epi, mode, False)
            if n_epi == 0:
                buf, counts = D.bracketed(run)
                assert conv_launches(counts) == {PH.cls_name(cls, mode): 1}, (cid, mode, counts)
            else:
                buf = run()
            check_y(buf, shape, False, D.epilogue64(conv, o, epi, bias=direction > 0), (cid, direction, opset, mode, epi))
    assert not torch.equal(refs[BF16X3], refs[BF16])      # the two modes have different answers here: bf16 equality => lo planes unread


@gpu
@pytest.mark.parametrize("cid,opset", WGRAD_PARAMS)
def test_wide_wgrad_branch_is_exact(ops, cid, opset):
    """bd_conv3x3_ps_wgrad on conv_ps_wgrad3_kernel with the pinned K split: dw equals fp64 autograd (of the bf16-rounded operands in
    BD_MODE_BF16), db the fp64 sum of the unrounded dy in both modes, and dw without db is the same dw"""
    L, lib = PH._lib()
    shape = WGRAD_CASES[cid][:5]
    assert wgrad_split(lib, L, shape) == WGRAD_CASES[cid][5:8], cid                      # the branch, before anything is launched
    o = wgrad_operands(cid, opset)
    px, pdy = place_planes(ops.split_rows(o["x"].cuda()), False), place_planes(ops.split_rows(o["dy"].cuda()), False)
    db_ref = o["dy"].double().sum(dim=(0, 1, 2))
    refs = {}
    for mode in MODES:
        dw_ref = refs[mode] = wgrad_ref(cid, opset, mode)
        (dw, db), counts = D.bracketed(lambda: run_wgrad(shape, px, pdy, True, mode))
        assert conv_launches(counts) == {PH.cls_name("conv_ps_wgrad3", mode): 1}, (cid, mode, counts)
        check_dw(dw, db, shape, dw_ref, db_ref, (cid, opset, mode))
        dw_only, _ = run_wgrad(shape, px, pdy, False, mode)
        check_dw(dw_only, None, shape, dw_ref, None, (cid, opset, mode, "without db"))
    assert not torch.equal(refs[BF16X3], refs[BF16])


@gpu
@pytest.mark.parametrize("cid,direction,opset", PADDED_FWD_PARAMS)
def test_padded_leading_dimensions_give_the_same_bits(ops, cid, direction, opset):
    """ldx = K + 64 with the operand one channel block in, ldy = N + 32 with y 16 columns in, ldr = N + 8 with the residual 4 columns in,
    ld_rowbias = N + 4, prev in y's window: the window equals the fp64 reference of the dense case and every byte outside it is still NaN
    (a read outside the operand window would poison the result: the other blocks hold a bf16 NaN).  Forward EPI 0, 3, 7; data gradient plain
    and accumulating; both modes"""
    shape = fwd_shape(cid)
    o = fwd_operands(cid, direction, opset)
    dev = {k: v.cuda() for k, v in o.items()}
    px = place_planes(ops.split_rows(dev["x"]), True)
    ws = ops.split_bf16(dev["w"]) if direction > 0 else ops.split_wT(dev["w"])
    for mode in MODES:
        conv = conv_ref(cid, direction, opset, mode)
        for epi in ((0, 3, 7) if direction > 0 else (0, 4)):
            buf = run_conv(shape, direction, px, ws, dev, epi, mode, True)
            check_y(buf, shape, True, D.epilogue64(conv, o, epi, bias=direction > 0), (cid, direction, opset, mode, epi, "padded"))


@gpu
@pytest.mark.parametrize("cid,opset", PADDED_WGRAD_PARAMS)
def test_padded_wgrad_leading_dimensions_give_the_same_bits(ops, cid, opset):
    """ldx = Cin + 64, lddy = Cout + 64, both operands one channel block in, NaN blocks on either side: dw and db equal the fp64 references"""
    shape = wgrad_shape(cid)
    o = wgrad_operands(cid, opset)
    px, pdy = place_planes(ops.split_rows(o["x"].cuda()), True), place_planes(ops.split_rows(o["dy"].cuda()), True)
    db_ref = o["dy"].double().sum(dim=(0, 1, 2))
    for mode in MODES:
        dw, db = run_wgrad(shape, px, pdy, True, mode)
        check_dw(dw, db, shape, wgrad_ref(cid, opset, mode), db_ref, (cid, opset, mode, "padded"))


def describe_slots(part, ref):
    bad = ~(part == ref)
    idx = bad.nonzero()
    return (f"{int(bad.sum())} of {bad.numel()} partials differ ({int(torch.isnan(part[bad]).sum())} NaN); first (b, tile, group, sum | sum of squares) "
            f"{idx[:8].tolist()}; tiles at fault {sorted(set(idx[:, 1].tolist()))[:16]}; equal after summing over tiles: {torch.equal(part.sum(1), ref.sum(1))}")


@gpu
@pytest.mark.parametrize("cid,epi", GN_PARAMS)
def test_gn_partials_are_exact_slot_by_slot(ops, cid, epi):
    """conv_ps3_kernel's GroupNorm epilogue: y is bit for bit the y of the call without gn_part (and the fp64 reference); part [B, S, G, 2]
    (NaN-prefilled) equals the fp64 sums of the reference over each VIRTUAL tile and group, slot by slot, for both group counts of the case
    and both modes.  bd_gn_fwd only needs the sum over S, so a permutation of the tiles of one sample would be harmless to the network; it
    fails here"""
    L, lib = PH._lib()
    B, H, W, K, N, groups = GN_CASES[cid]
    shape = (B, H, W, K, N)
    for G in groups:
        assert lib.bd_conv3x3_ps_gn_splits(B, H, W, K, N, G) == H * W // 256, (cid, G)       # the branch, before anything is launched
    o = gn_operands(cid)
    dev = {k: v.cuda() for k, v in o.items()}
    px = place_planes(ops.split_rows(dev["x"]), False); ws = ops.split_bf16(dev["w"])
    ref = gn_ref(cid, epi)
    for mode in MODES:
        plain = run_conv(shape, 1, px, ws, dev, epi, mode, False)
        check_y(plain, shape, False, ref, (cid, epi, mode, "without gn_part"))
        for G in groups:
            part = torch.full((B, H * W // 256, G, 2), float("nan"), dtype=torch.float64, device="cuda")
            buf = run_conv(shape, 1, px, ws, dev, epi, mode, False, gn=(part, G))
            assert torch.equal(buf[:B * H * W], plain[:B * H * W]), (cid, epi, mode, G, "y changes with gn_part")
            assert bool(torch.isnan(buf[B * H * W:]).all()), (cid, epi, mode, G, "store past the last row")
            want = tile_sums(ref, G)
            assert torch.equal(part.cpu(), want), (cid, epi, mode, G, describe_slots(part.cpu(), want))


@gpu
def test_gn_part_is_refused_where_no_epilogue_writes_it(ops):
    """BD_ERR_UNSUPPORTED with y and part still NaN: gn_part with neither or both of residual / row bias (EPI 0, 3), with accumulate, and on a
    data gradient"""
    L, lib = PH._lib()
    B, H, W, K, N = shape = GN_CASES["N1"][:5]
    M = B * H * W
    xs = torch.zeros(M, K // 32, 2, 32, dtype=torch.int16, device="cuda"); ws = torch.zeros(N, 9 * K // 32, 2, 32, dtype=torch.int16, device="cuda")
    res = torch.zeros(M, N, device="cuda"); rb = torch.zeros(B, N, device="cuda")
    for what, kw in (("EPI 0", dict()), ("EPI 3", dict(residual=L.ptr(res), ldr=N, rowbias=L.ptr(rb), ld_rowbias=N)),
                     ("accumulate", dict(rowbias=L.ptr(rb), ld_rowbias=N, accumulate=1)),
                     ("direction -1", dict(rowbias=L.ptr(rb), ld_rowbias=N, direction=-1))):
        y = PH.out_buffer(M, N, 0)
        part = torch.full((B, H * W // 256, 32, 2), float("nan"), dtype=torch.float64, device="cuda")
        f = dict(B=B, H=H, W=W, K=K, N=N, direction=1, x_split=L.ptr(xs), ldx=K, w_split=L.ptr(ws), out_scale=0.5, y=L.ptr(y), ldy=N,
                 gn_part=L.ptr(part), gn_groups=32, mode=BF16X3)
        f.update(kw)
        rc = lib.bd_conv3x3_ps(ctypes.byref(L.ConvPsDesc(**f)), L.stream())
        torch.cuda.synchronize()
        assert rc == ERR_UNSUPPORTED and b"gn_part" in (lib.bd_last_error() or b""), (what, rc, lib.bd_last_error())
        assert bool(torch.isnan(y).all()) and bool(torch.isnan(part).all()), what


@gpu
def test_refused_leading_dimensions_leave_the_outputs_untouched(ops):
    """the rejections of test_leading_dimension_below_the_channel_count_is_refused with real buffers: BD_ERR_INVALID, y / dw / db still NaN"""
    L, lib = PH._lib()
    B, H, W, K, N = 1, 8, 8, 64, 128
    M = B * H * W
    xs = torch.zeros(M, K // 32, 2, 32, dtype=torch.int16, device="cuda"); ws = torch.zeros(N, 9 * K // 32, 2, 32, dtype=torch.int16, device="cuda")
    res = torch.zeros(M, N, device="cuda"); rb = torch.zeros(B, N, device="cuda")
    wsp = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    for kw in (dict(ldx=32), dict(ldy=64), dict(residual=L.ptr(res), ldr=64), dict(rowbias=L.ptr(rb), ld_rowbias=64)):
        y = PH.out_buffer(M, N, 0)
        f = dict(B=B, H=H, W=W, K=K, N=N, direction=1, x_split=L.ptr(xs), ldx=K, w_split=L.ptr(ws), out_scale=1.0, y=L.ptr(y), ldy=N,
                 workspace=L.ptr(wsp), workspace_bytes=wsp.numel(), mode=BF16X3)
        f.update(kw)
        rc = lib.bd_conv3x3_ps(ctypes.byref(L.ConvPsDesc(**f)), L.stream())
        torch.cuda.synchronize()
        assert rc == ERR_INVALID and bool(torch.isnan(y).all()), (kw, rc)
    C = 256
    xs = torch.zeros(M, C // 32, 2, 32, dtype=torch.int16, device="cuda")
    for kw in (dict(ldx=128), dict(lddy=128)):
        dw = PH.out_buffer(C, 9 * C, 0); db = PH.out_buffer(1, C, 0)
        f = dict(B=B, H=H, W=W, Cin=C, Cout=C, x_split=L.ptr(xs), ldx=C, dy_split=L.ptr(xs), lddy=C, dw=L.ptr(dw), db=L.ptr(db),
                 workspace=L.ptr(wsp), workspace_bytes=wsp.numel(), mode=BF16X3)
        f.update(kw)
        rc = lib.bd_conv3x3_ps_wgrad(ctypes.byref(L.ConvPsWgradDesc(**f)), L.stream())
        torch.cuda.synchronize()
        assert rc == ERR_INVALID and bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all()), (kw, rc)
