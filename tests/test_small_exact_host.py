"""CPU: the data of tests/_small_exact.py is rounding-free, and its sizes follow the constants in the sources.

1. For every exact case the reference is computed in fp64 and again in fp32 with the summation order reversed or permuted; the two must be
   equal, so any order a kernel sums in gives the same bits and torch.equal is the right assertion on the GPU.  A case that fails here is
   changed, not given a tolerance.
2. TPB, RED_BLOCKS and the per-launch grid caps are read out of the text of csrc/elementwise.hip, the tile sizes out of csrc/inception.hip; the
   "second trip" and "tile + 1" sizes of the tables must be derived from them, so a retune fails here instead of silently uncovering a
   branch."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import _small_exact as S

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "baddiffusion_amd", "csrc")


def source(name):
    return open(os.path.join(CSRC, name)).read()


def same(ref64, other32):
    """the fp64 reference is representable in fp32 and equals the fp32 result computed in another order"""
    return S.exact_in_fp32(ref64) and torch.equal(ref64.float(), other32)


# ------------------------------------------------------------------------------------------------ 2. constants and derived sizes
def grid_caps(src):
    """kernel -> cap of every `hipLaunchKernelGGL(kernel, dim3(nblocks(count, TPB, cap)), ...)`"""
    caps = {}
    for kernel, cap in re.findall(r"hipLaunchKernelGGL\(\(?(\w+)(?:<\w+>)?\)?, dim3\(nblocks\([^;]*?, TPB, (\w+)\)\)", src):
        caps.setdefault(kernel, set()).add(cap)
    return caps


def test_elementwise_constants_and_derived_sizes():
    src = source("elementwise.hip")
    tpb = int(re.search(r"constexpr int TPB = (\d+);", src).group(1))
    red = int(re.search(r"constexpr int RED_BLOCKS = (\d+);", src).group(1))
    assert (tpb, red) == (S.TPB, S.RED_BLOCKS)
    caps = grid_caps(src)
    assert caps["silu_fwd_kernel"] == caps["silu_bwd_kernel"] == {str(S.SILU_CAP)}
    assert caps["add_kernel"] == caps["axpy_kernel"] == caps["adam_clip_kernel"] == {str(S.WIDE_CAP)}
    assert re.search(r"nblocks\(n / 4 \+ 1, TPB, RED_BLOCKS\);\s*hipLaunchKernelGGL\(sumsq_kernel", src)
    assert re.search(r"softmax_fwd_kernel, dim3\(\(unsigned\)cdiv\(rows, TPB / 64\)\)", src) and re.search(
        r"softmax_bwd_kernel, dim3\(\(unsigned\)cdiv\(rows, TPB / 64\)\)", src)
    # the blocks of axpy_kernel are spelled 256
    assert re.search(r"__launch_bounds__\(256\) void axpy_kernel", src) and tpb == 256
    # second trips: one full pass of the capped grid plus a ragged rest shorter than a block
    assert S.SILU_SECOND_TRIP == S.SILU_CAP * tpb + 77 and S.SILU_SECOND_TRIP in S.SILU_N
    assert S.AXPY_SECOND_TRIP == S.WIDE_CAP * tpb + 77 and S.AXPY_SECOND_TRIP in S.AXPY_N
    big = S.ADD_CASES[-1]
    assert (big.rows, big.C) == (S.ADD_BIG_ROWS, S.ADD_BIG_C) and big.rows * (big.C // 4) == S.WIDE_CAP * tpb + 6
    assert S.SUMSQ_SECOND_TRIP == 4 * (red * tpb + 77) + 3 and S.SUMSQ_SECOND_TRIP in S.SUMSQ_N
    assert {n & 3 for n in S.SUMSQ_N} == {0, 1, 2, 3} and min(S.SUMSQ_N) < 4
    # softmax: 7 rows = one full block and a second one with one wave past the end
    rpb = tpb // 64
    assert S.SOFTMAX_ROWS_PER_BLOCK == rpb and 1 in S.SOFTMAX_ROWS and 2 * rpb - 1 in S.SOFTMAX_ROWS
    assert {63, 64, 65} <= set(S.SOFTMAX_N)                                  # one lane idle / every lane once / a second trip of lane 0
    # colsum: 64 columns x 4 row phases per block
    assert re.search(r"__shared__ float red\[4\]\[64\];", src)
    assert {c.N for c in S.COLSUM_CASES} >= {1, 63, 64, 65, 130} and {c.rpg for c in S.COLSUM_CASES} >= {1, 3, 64}
    assert any(c.rows % c.rpg and c.rpg == 64 for c in S.COLSUM_CASES) and {c.acc for c in S.COLSUM_CASES} == {0, 1}
    # blocks of the one-thread-per-item kernels
    B, H, W = S.TO_IMAGE_BHW
    assert tpb < B * H * W < 2 * tpb
    assert S.TEMB_OVER_TPB_B * (S.TEMB_OVER_TPB_DIM // 2) == tpb + 4
    c = S.SUM2X2_CASES[-1]
    assert c.B * c.H * c.W * (c.C // 4) == 630 and 2 * tpb < 630 < 3 * tpb


def test_inception_constants_and_derived_sizes():
    src = source("inception.hip")
    m = re.search(r"constexpr int IC_BM = (\d+), IC_BN = (\d+), IC_BK = (\d+)", src)
    m2 = re.search(r"constexpr int IC2_BM = (\d+), IC2_BN = (\d+), IC2_BK = (\d+)", src)
    assert tuple(map(int, m.groups())) == (S.IC_BM, S.IC_BN, S.IC_BK) and tuple(map(int, m2.groups())) == (S.IC2_BM, S.IC2_BN, S.IC2_BK)
    by = {c.name: c for c in S.CONV_CASES}
    assert by["m1"].M == 1 and by["m_bm"].M == S.IC_BM + 1 and by["m_bm2"].M == S.IC2_BM + 1
    bn, bk = S.IC_BN, S.IC_BK
    assert S.IC2_BN == bn and S.IC2_BK == bk
    couts = {c.Cout for c in S.CONV_CASES}
    assert 4 in couts and any(4 < n < bn and n % 32 for n in couts) and bn + 4 in couts
    cins = {c.Cin for c in S.CONV_CASES}
    assert {3, 5, bk + 1, bk + 4, 2048} <= cins
    kinds = {(c.KH, c.KW, c.sh, c.sw, c.ph, c.pw) for c in S.CONV_CASES}
    assert {(1, 1, 1, 1, 0, 0), (3, 3, 2, 2, 0, 0), (5, 5, 1, 1, 2, 2), (1, 7, 1, 1, 0, 3), (7, 1, 1, 1, 3, 0), (3, 3, 2, 1, 0, 2)} <= kinds
    assert any(c.relu == 0 and not c.bias for c in S.CONV_CASES)
    assert {c.Cin % 4 == 0 for c in S.CONV_CASES if c.xslice} == {True, False}
    assert all(c.Cout % 4 == 0 and c.why for c in S.CONV_CASES)
    assert S.POOL_SLICE.ldx % 4 == 0 and S.POOL_SLICE.ldy % 4 == 0 and S.POOL_SLICE.xoff % 4 == 0 and S.POOL_SLICE.yoff % 4 == 0
    B, HW, C = S.GAP_SHAPES[-1]
    assert 256 < B * C < 512                   # ic_gap_kernel: 256 threads per block


# ------------------------------------------------------------------------------------------------ 1. the data is rounding-free
@pytest.mark.parametrize("rows", S.SOFTMAX_ROWS)
@pytest.mark.parametrize("n", S.SOFTMAX_N)
def test_softmax_exact_rows(rows, n):
    perm = torch.randperm(n, generator=S.gen(n))
    for name, (s, exact) in S.softmax_inputs(rows, n).items():
        ref = S.softmax_ref(s)
        if name == "const":
            assert torch.equal(ref, torch.full_like(ref, 1.0 / n))
        if name == "hot":
            assert torch.equal(ref.float().sum(-1), torch.ones(rows)) and set(ref.float().unique().tolist()) <= {0.0, 1.0}
        if name == "ninf":
            assert torch.equal(ref == 0, torch.isinf(s)) and bool(torch.isinf(s).any())
        if exact:
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(n)
            other = torch.softmax(s[:, perm], -1)[:, inv]
            # hot: exp(-200) = 1.4e-87 in fp64 is 0 in fp32 and the hot entry is 1 in both, so the cast reference is the exact one-hot
            assert torch.equal(ref.float(), other) and (name == "hot" or S.exact_in_fp32(ref)), (name, rows, n)
    for name, (p, dp, exact) in S.softmax_bwd_inputs(rows, n).items():
        if exact:
            ref = S.softmax_bwd_ref(p, dp)
            dot = (p * dp).flip(-1).sum(-1, keepdim=True)            # fp32, the other way round
            assert same(ref, p * (dp - dot)), (name, rows, n)


@pytest.mark.parametrize("c", S.COLSUM_CASES, ids=lambda c: f"{c.rows}x{c.N}r{c.rpg}a{c.acc}")
def test_colsum_exact(c):
    x, pre = S.colsum_data(c)
    xf = x.flip(0)                                                   # rows last to first, fp32
    out = torch.stack([xf[max(c.rows - (g + 1) * c.rpg, 0): c.rows - g * c.rpg].sum(0) for g in range(c.groups)])
    assert same(S.colsum_ref(c, x, pre), out + pre if c.acc else out) and c.why


@pytest.mark.parametrize("c", S.SUM2X2_CASES, ids=lambda c: f"{c.B}x{c.H}x{c.W}x{c.C}")
def test_sum2x2_exact(c):
    du, pre = S.sum2x2_data(c)
    v = du.reshape(c.B, c.H, 2, c.W, 2, c.C)
    out = (v[:, :, 1, :, 1] + v[:, :, 0, :, 1]) + (v[:, :, 1, :, 0] + v[:, :, 0, :, 0])
    assert same(S.sum2x2_ref(c, du, pre), pre + out if c.acc else out) and c.why


def test_add_axpy_exact():
    for c in S.ADD_CASES[:2]:
        src, pre = S.add_data(c)
        for scale, acc in c.combos:
            assert same(S.axpy_ref(src, pre, scale, acc), pre + scale * src if acc else scale * src)
    # every value the large cases can meet: scale * a + b over all a, b in [-8, 8]
    a = torch.arange(-8.0, 9.0)[:, None].expand(17, 17)
    b = torch.arange(-8.0, 9.0)[None, :].expand(17, 17)
    for scale in set(S.AXPY_SCALES) | {s for s, _ in S.ALL_ADD}:
        assert same(S.axpy_ref(a, b, scale, 1), b + scale * a)


@pytest.mark.parametrize("n", S.SUMSQ_N)
def test_sumsq_exact(n):
    """the kernel squares and sums in fp64: the proof is against integer arithmetic, forwards and backwards"""
    x = S.sumsq_data(n)
    want = int((x.long() ** 2).sum())
    assert float((x.double() ** 2).sum()) == want == float((x.double().flip(0) ** 2).sum()) and want < 2 ** 53


def test_sumsq_big_values_need_fp64_squares():
    x, want = S.sumsq_big_values()
    assert float((x.double() ** 2).sum()) == want == float((x.double().flip(0) ** 2).sum())
    assert bool(torch.isinf((x * x).sum()))                                   # squares formed in fp32 overflow


def test_silu_exact_subcase():
    dy = S.ints(257, -8, 8, 1)
    z = torch.zeros(257)
    assert torch.equal(S.silu_ref(z), torch.zeros(257, dtype=torch.float64)) and same(S.silu_bwd_ref(z, dy), 0.5 * dy)
    for n in S.SILU_N[:3]:
        z, _, _ = S.silu_data(n)
        assert set(torch.tensor(S.SILU_PLANTED[:min(n, len(S.SILU_PLANTED))]).tolist()) <= set(z.tolist())
        assert bool(torch.isfinite(S.silu_ref(z).float()).all())


def test_to_image_ties_and_reference():
    x, k = S.to_image_ties()
    assert x.numel() >= 8 and bool((k % 2 == 0).any()) and bool((k % 2 == 1).any())
    t = (x / 2 + 0.5) * 255                                                   # fp32, as the kernel forms it
    assert torch.equal(t, k.float() + 0.5)
    assert torch.equal((t.round().long()) % 2, torch.zeros_like(k))          # round half to even
    assert torch.equal((x / 2).double(), x.double() / 2)                      # x / 2 is exact
    for C in S.TO_IMAGE_C:
        d = S.to_image_data(C)
        flat = d.reshape(-1)
        assert all(bool((flat == v).any()) for v in S.TO_IMAGE_PLANTED) and bool(torch.signbit(flat[flat == 0]).any())
        f, u = S.to_image_ref(d)
        assert float(f.min()) == 0.0 and float(f.max()) == 1.0 and int(u.min()) == 0 and int(u.max()) == 255


def test_temb_table():
    cases = S.temb_cases()
    assert {(B, d) for B, d, *_ in cases} >= {(B, d) for B in S.TEMB_B for d in S.TEMB_DIMS}
    assert {(f, s, ts) for _, d, f, s, ts in cases if d == 32} == {(f, s, ts) for f in (0, 1) for s in (0, 1) for ts in (0, 1, 2)}
    assert not any(s == 1 and d // 2 == 1 for _, d, _, s, _ in cases)
    for B, dim, flip, shift, ts in cases:
        t, buf = S.temb_t(B, ts)
        assert torch.equal(buf[torch.arange(B) * ts], t)
        e = S.temb_ref(t, dim, flip, shift)
        assert e.shape == (B, dim) and bool(torch.isfinite(e).all())
        half = dim // 2
        sin, cos = (e[:, half:2 * half], e[:, :half]) if flip else (e[:, :half], e[:, half:2 * half])
        z = t == 0
        assert bool((sin[z] == 0).all()) and bool((cos[z] == 1).all())


@pytest.mark.parametrize("c", S.CONV_CASES, ids=lambda c: c.name)
def test_conv_exact(c):
    x, w, b = S.conv_data(c)
    ref = S.conv_ref(c, x, w, b)
    perm = torch.randperm(c.Cin, generator=S.gen(c.Cin))                      # fp32 with the channels, rows and columns of the taps permuted
    other = S.conv_ref(c, x[:, perm], w[:, perm], b, torch.float32)
    assert same(ref, other), c.name
    if (c.H + 2 * c.ph - c.KH) % c.sh == 0 and (c.W + 2 * c.pw - c.KW) % c.sw == 0:      # the mirrored image has the same windows
        assert same(ref, S.conv_ref(c, x.flip(2, 3), w.flip(2, 3), b, torch.float32).flip(1, 2)), c.name
    assert ref.shape == (c.B, c.Ho, c.Wo, c.Cout) and c.why
    if not c.relu:
        assert float(ref.min()) < 0


def test_pool_gap_exact():
    for shape in S.POOL_SHAPES:
        for negative in (False, True):
            x = S.pool_data(shape, negative)
            for st in S.POOL_SETTINGS:
                k, s, p, mode, cip = st
                ref = S.pool_ref(x, st, torch.float64)
                assert torch.equal(ref.float(), S.pool_ref(x, st)), (shape, st)
                assert torch.equal(ref.float(), S.pool_ref(x.flip(2, 3), st).flip(1, 2)) or (shape[1] - k + 2 * p) % s or (shape[2] - k + 2 * p) % s
                if mode == 0 and negative:
                    assert float(ref.max()) < 0
    assert S.pool_ref(S.pool_data(S.POOL_SHAPES[0], False), S.POOL_SETTINGS[0]).shape[1:3] == (1, 1)
    for B, HW, C in S.GAP_SHAPES:
        x = S.gap_data(B, HW, C)
        ref = S.gap_ref(x, torch.float64)
        assert torch.equal(ref.float(), S.gap_ref(x)) and torch.equal(ref.float(), S.gap_ref(x.flip(1)))


@pytest.mark.parametrize("src,dst", S.RESIZE_EXACT)
def test_resize_exact(src, dst):
    for C in S.RESIZE_C:
        for u8, scale, shift in ((False, 1.0, 0.0), (True, 2.0, -1.0)):
            x = S.resize_data(src, C, u8)
            ref = S.resize_ref(x, dst, scale, shift)
            assert same(ref, S.resize_ref(x, dst, scale, shift, torch.float32)), (src, dst, C, u8)
            # the mirrored image resizes to the mirrored result: the taps meet in the other order
            assert torch.equal(ref, S.resize_ref(x.flip(1, 2), dst, scale, shift).flip(1, 2))
            if src == dst:
                assert torch.equal(ref, scale * (x.double() / 255 if u8 else x.double()) + shift)


def test_helpers():
    x = S.ints((3, 5), -8, 8, 0)
    assert torch.equal(x, x.round()) and float(x.abs().max()) <= 8 and torch.equal(x, S.ints((3, 5), -8, 8, 0))
    buf = S.padded(x, 4, 6)
    assert buf.numel() == 25 and bool(torch.isnan(buf[:4]).all()) and bool(torch.isnan(buf[19:]).all()) and torch.equal(buf[4:19].view(3, 5), x)
    v, buf = S.strided_rows(x, 8, lead=4, trail=2)
    assert buf.numel() == 30 and torch.equal(v, x) and v.stride() == (8, 1) and v.data_ptr() == buf.data_ptr() + 16
    assert int(torch.isnan(buf).sum()) == 30 - 15 and S.outside_is_nan(buf, 4, 3, 5, 8)
    buf[4 + 5] = 0.0                       # a column past C
    assert not S.outside_is_nan(buf, 4, 3, 5, 8)
    assert bool(torch.isnan(S.nan_rows(3, 5, 8, 4, 2)).all())
