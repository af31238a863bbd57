"""Case tables, data builders and fp64 references of the exact-value tests of the small training / sampling ops (csrc/elementwise.hip)
and of the FID kernels (csrc/inception.hip).  tests/test_small_exact_host.py proves the data rounding-free on the CPU and ties the sizes
below to the constants in the sources; tests/test_small_exact.py runs the kernels on it.  Nothing here touches a device.

The data is small integers with power-of-two scales, so every sum the kernels form is exact in fp32 in any order and the assertion is
torch.equal against an fp64 reference cast to fp32.  Every case carries one line (`why`) naming the defect it is there to catch.
DESIGN.md "Small ops and FID kernels: test cases" carries the same tables; whoever retunes a constant below moves the cases with it."""
import functools
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

NAN = float("nan")

# ---- constants restated from the sources (test_small_exact_host.py parses them out of the text and compares)
TPB = 256                    # elementwise.hip: threads per block of every kernel here
RED_BLOCKS = 1024            # elementwise.hip: grid cap of the two-stage reductions (bd_sumsq)
SILU_CAP = 4096              # nblocks(n, TPB, 4096) of bd_silu_fwd / bd_silu_bwd
WIDE_CAP = 8192              # nblocks(.., TPB, 8192) of add, bd_axpy (and clip + Adam)
SOFTMAX_ROWS_PER_BLOCK = TPB // 64
IC_BM, IC_BN, IC_BK = 64, 64, 16        # inception.hip: ic_conv_kernel tile (w_kc = 0)
IC2_BM, IC2_BN, IC2_BK = 128, 64, 16    # inception.hip: ic_conv2_kernel tile (w_kc = 1)

# ---- sizes derived from them: one ragged range more than a full pass of the capped grid ("second trip")
SILU_SECOND_TRIP = SILU_CAP * TPB + 77
AXPY_SECOND_TRIP = WIDE_CAP * TPB + 77
ADD_BIG_C = 8
ADD_BIG_ROWS = (WIDE_CAP * TPB + 6) // (ADD_BIG_C // 4)          # rows * 2 float4s = cap * TPB + 6: a 6-element second trip
SUMSQ_SECOND_TRIP = 4 * RED_BLOCKS * TPB + 4 * 77 + 3             # 77 float4s of second trip plus a 3-element tail
TEMB_OVER_TPB_B = 5
TEMB_OVER_TPB_DIM = 2 * (TPB // TEMB_OVER_TPB_B + 1)              # B * (dim / 2) = 260: four threads in a second block


# ------------------------------------------------------------------------------------------------ helpers
def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, lo, hi, seed):
    """integer-valued fp32 tensor, uniform in [lo, hi], from a seeded generator"""
    if isinstance(shape, int):
        shape = (shape,)
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen(seed)).float()


def padded(x, lead, trail):
    """flat NaN buffer holding x (flattened) at [lead, lead + x.numel())"""
    buf = torch.full((lead + x.numel() + trail,), NAN, dtype=x.dtype)
    buf[lead: lead + x.numel()] = x.reshape(-1)
    return buf


def rows_view(buf, lead, rows, C, ld):
    """the [rows, C] view with leading dimension ld that starts `lead` elements into the flat buffer"""
    return buf[lead: lead + rows * ld].view(rows, ld)[:, :C]


def strided_rows(x, ld, lead=0, trail=0):
    """x [rows, C] placed in a [rows, ld] NaN buffer (NaN in columns C..ld and in the margins): returns (view, flat buffer)"""
    rows, C = x.shape
    assert ld >= C
    buf = torch.full((lead + rows * ld + trail,), NAN, dtype=x.dtype)
    v = rows_view(buf, lead, rows, C, ld)
    v.copy_(x)
    return v, buf


def nan_rows(rows, C, ld, lead=0, trail=0):
    """an all-NaN output buffer for a [rows, C] view of leading dimension ld"""
    return torch.full((lead + rows * ld + trail,), NAN)


def outside_is_nan(buf, lead, rows, C, ld):
    """everything of the flat buffer outside the [rows, C] view is NaN"""
    b = buf.detach().cpu().clone()
    rows_view(b, lead, rows, C, ld).fill_(NAN)
    return bool(torch.isnan(b).all())


def exact_in_fp32(x64):
    """the fp64 reference survives the cast to fp32 unchanged"""
    return bool(torch.equal(x64.float().double(), x64))


# ------------------------------------------------------------------------------------------------ softmax
SOFTMAX_ROWS = (1, 7)            # 7 = one full block of 4 rows + 3 of the 4 waves of a second one (the row >= rows guard)
SOFTMAX_N = (1, 2, 63, 64, 65, 100, 256, 1024)
SOFTMAX_CONSTS = (0.0, 1000.0, -1000.0, 3e38)


def pow2(n):
    return n & (n - 1) == 0


def softmax_hot_indices(n):
    """hot positions of the one-hot rows: lane 0, a lane's second trip (64+) and the last element"""
    idx = [0, n - 1]
    if n > 64:
        idx.insert(1, 64 + (n - 64) // 3)
    return idx


def softmax_inputs(rows, n):
    """name -> ([rows, n] fp32 logits, exact?).  const: constant rows, p == 1/n bit for bit (a missing max-subtraction overflows at 1000 and
    3e38, underflows at -1000); hot: [-200 .. 0 .. -200] gives an exact one-hot (exp(-200) is 0 in fp32); ninf: -inf entries give p == 0;
    randn: randn * 3 plus a per-row offset of up to +-60, compared at the tolerance of test_softmax"""
    out = {}
    if pow2(n):
        c = torch.tensor([SOFTMAX_CONSTS[r % 4] for r in range(rows)])
        out["const"] = (c[:, None].expand(rows, n).contiguous(), True)
    hot = torch.full((rows, n), -200.0)
    hi = softmax_hot_indices(n)
    for r in range(rows):
        hot[r, hi[r % len(hi)]] = 0.0
    out["hot"] = (hot, True)
    s = torch.randn(rows, n, generator=gen(100 * n + rows)) * 3
    out["randn"] = (s + 20.0 * ints((rows, 1), -3, 3, n + rows), False)
    if n > 1:
        m = s.clone()
        m[torch.rand(rows, n, generator=gen(7 * n + rows)) < 0.4] = -float("inf")
        m[:, n // 2] = 1.5               # at least one finite entry per row
        out["ninf"] = (m, False)
    return out


def softmax_ref(s):
    return torch.softmax(s.double(), -1)


def softmax_bwd_inputs(rows, n):
    """name -> (p, dp, exact?).  uniform: p = 1/n (n a power of two) with dp ints in [-8, 8]: every product and sum is a multiple of 1/n^2"""
    out = {}
    if pow2(n):
        out["uniform"] = (torch.full((rows, n), 1.0 / n), ints((rows, n), -8, 8, 3 * n + rows), True)
    s = torch.randn(rows, n, generator=gen(11 * n + rows)) * 3
    out["randn"] = (torch.softmax(s.double(), -1).float(), torch.randn(rows, n, generator=gen(13 * n + rows)), False)
    return out


def softmax_bwd_ref(p, dp):
    p, dp = p.double(), dp.double()
    return p * (dp - (p * dp).sum(-1, keepdim=True))


# ------------------------------------------------------------------------------------------------ colsum / sum2x2 / add / axpy / sumsq
def _cs(rows, N, rpg, ldx, ldo, acc, why):
    return NS(rows=rows, N=N, rpg=rpg, ldx=ldx, ldo=ldo, acc=acc, why=why, groups=-(-rows // rpg))


COLSUM_CASES = [
    _cs(1, 1, 1, 4, 6, 0, "one element: three of four row phases and 63 of 64 columns idle"),
    _cs(5, 130, 1, 133, 135, 1, "rows_per_group 1 over three column blocks: a phase that reads past its group adds the next row"),
    _cs(7, 63, 3, 66, 68, 1, "rows_per_group 3 < 4 phases, ragged last group (3 + 3 + 1), accumulate onto preloaded values"),
    _cs(130, 64, 64, 67, 69, 0, "ragged last group (rows 130, rpg 64: 2 rows): m1 clamped to rows; N = 64 fills one column block"),
    _cs(130, 65, 64, 68, 70, 1, "N = 65: a second column block with one live column; accumulate"),
    _cs(128, 130, 64, 133, 135, 0, "three column blocks, the last with 2 live columns; strided input and output"),
    _cs(12, 64, 3, 64, 64, 0, "dense (ldx = ld_out = N), the layout ops.colsum passes"),
]


def colsum_data(c):
    seed = c.rows * 1000 + c.N
    return ints((c.rows, c.N), -8, 8, seed), ints((c.groups, c.N), -8, 8, seed + 1)


def colsum_ref(c, x, pre):
    x = x.double()
    out = torch.stack([x[g * c.rpg: min((g + 1) * c.rpg, c.rows)].sum(0) for g in range(c.groups)])
    return out + pre.double() if c.acc else out


def _s2(B, H, W, C, ldu, lddx, acc, why):
    return NS(B=B, H=H, W=W, C=C, ldu=ldu, lddx=lddx, acc=acc, why=why)


SUM2X2_CASES = [
    _s2(1, 1, 1, 4, 4, 4, 0, "one thread: the four taps of one 2x2 block"),
    _s2(2, 3, 5, 8, 12, 16, 1, "both leading dimensions above C and unequal, accumulate: a row stride taken from the wrong operand"),
    _s2(2, 5, 7, 36, 36, 36, 0, "630 threads: three blocks, the last ragged; odd H and W"),
]


def sum2x2_data(c):
    seed = c.B * 100 + c.C
    return ints((c.B, 2 * c.H, 2 * c.W, c.C), -8, 8, seed), ints((c.B, c.H, c.W, c.C), -8, 8, seed + 1)


def sum2x2_ref(c, du, pre):
    out = du.double().reshape(c.B, c.H, 2, c.W, 2, c.C).sum((2, 4))
    return out + pre.double() if c.acc else out


def _ad(rows, C, lds, ldd, combos, why):
    return NS(rows=rows, C=C, lds=lds, ldd=ldd, combos=combos, why=why)


ALL_ADD = [(s, a) for s in (0.5, -2.0) for a in (0, 1)]
ADD_CASES = [
    _ad(1, 4, 4, 4, ALL_ADD, "one float4"),
    _ad(37, 12, 16, 20, ALL_ADD, "two unequal leading dimensions above C: 111 float4s, row and column recovered from the flat index"),
    _ad(ADD_BIG_ROWS, ADD_BIG_C, ADD_BIG_C, ADD_BIG_C, [(0.5, 1), (-2.0, 0)], "cap * TPB + 6 float4s: the stride loop's second trip is 6 float4s long"),
]


def add_data(c):
    return ints((c.rows, c.C), -8, 8, c.rows % 9973 + c.C), ints((c.rows, c.C), -8, 8, c.rows % 9973 + c.C + 1)


def axpy_ref(src, pre, scale, acc):
    """dst (+)= scale * src in fp64 (add and axpy share it)"""
    out = src.double() * scale
    return out + pre.double() if acc else out


AXPY_N = (1, 257, AXPY_SECOND_TRIP)
AXPY_SCALES = (1.0, 0.5, -2.0)

SUMSQ_N = (1, 2, 3, 4, 5, 7, 1023, SUMSQ_SECOND_TRIP)     # every n & 3, n < 4 (tail only), one block, second trip + 3-element tail


def sumsq_data(n):
    return ints(n, -8, 8, n % 9973 + 5)


def sumsq_big_values():
    """zeros except 2^70 in the float4 body and 2^69 in the tail: the squares are 2^140 and 2^138, far above fp32's range"""
    x = torch.zeros(11)
    x[2] = 2.0 ** 70
    x[9] = 2.0 ** 69
    return x, 2.0 ** 140 + 2.0 ** 138


# ------------------------------------------------------------------------------------------------ SiLU
SILU_N = (1, 255, 257, SILU_SECOND_TRIP)
SILU_PLANTED = (0.0, -0.0, 20.0, -20.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0, 1e-30)


def silu_data(n):
    """z = randn * 3 with the planted values at the front (as many as fit) and again at the very end; dy = randn; integer preload"""
    z = torch.randn(n, generator=gen(n % 9973)) * 3
    k = min(n, len(SILU_PLANTED))
    z[:k] = torch.tensor(SILU_PLANTED[:k])
    if n > 2 * len(SILU_PLANTED):
        z[-len(SILU_PLANTED):] = torch.tensor(SILU_PLANTED)
    return z, torch.randn(n, generator=gen(n % 9973 + 1)), ints(n, -8, 8, n % 9973 + 2)


def silu_ref(z):
    z = z.double()
    return z * torch.sigmoid(z)


def silu_bwd_ref(z, dy):
    z, dy = z.double(), dy.double()
    s = torch.sigmoid(z)
    return dy * (s * (1 + z * (1 - s)))


# ------------------------------------------------------------------------------------------------ to_image / layouts / timestep embedding
TO_IMAGE_BHW = (3, 9, 11)        # 297 pixels: two blocks, the second ragged
TO_IMAGE_C = (1, 3, 4)
TO_IMAGE_LAYOUTS = ("nchw", "nhwc", "nhwc_ld")      # nhwc_ld: ld = C + 5, NaN in the unused columns
TO_IMAGE_PLANTED = (-1.0, 1.0, -1.5, 3.0, 0.0, -0.0)


@functools.lru_cache(maxsize=None)
def to_image_ties():
    """inputs x in [-1, 1] for which the fp32 value (x / 2 + 0.5) * 255 is exactly k + 0.5 (round half to even decides the byte): found by
    search over a 2M-point linspace, returned as (x, k) with x fp32"""
    x = torch.linspace(-1, 1, 2_000_001, dtype=torch.float64).float()
    t = (x / 2 + 0.5) * 255
    hit = (t - t.floor()) == 0.5
    return x[hit], t[hit].floor().to(torch.int64)


def to_image_data(C):
    """[B, C, H, W] fp32: randn * 1.5 with the planted values and every tie in front"""
    B, H, W = TO_IMAGE_BHW
    x = torch.randn(B * C * H * W, generator=gen(40 + C)) * 1.5
    ties, _ = to_image_ties()
    special = torch.cat([torch.tensor(TO_IMAGE_PLANTED), ties])
    assert special.numel() <= x.numel()
    x[:special.numel()] = special
    return x.view(B, C, H, W)


def to_image_ref(x_nchw):
    """the reference's own expression, op by op in fp32 (each a single IEEE rounding; x / 2 is exact): NHWC float and uint8"""
    v = (x_nchw / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).contiguous()
    return v, (v * 255).round().to(torch.uint8)


LAYOUT_SHAPES = ((1, 1, 1, 1), (2, 3, 5, 7), (3, 5, 16, 17))       # (B, C, H, W); 816 pixels: four blocks, the last ragged
LAYOUT_LD_EXTRA = (0, 3)


def layout_data(B, C, H, W):
    """distinct integers (a swapped index cannot go unnoticed)"""
    return torch.arange(B * C * H * W, dtype=torch.float32).view(B, C, H, W) - 7.0


TEMB_B = (1, 5)
TEMB_DIMS = (3, 32, 33, 128)
TEMB_T = (0, 1, 500, 999, 37)


def temb_cases():
    """(B, dim, flip, shift, t_stride).  shift = 1 with dim / 2 == 1 (dim 2 or 3) is left out: the exponent is 0 / 0 in the reference too"""
    shapes = [(B, d) for B in TEMB_B for d in TEMB_DIMS] + [(TEMB_OVER_TPB_B, TEMB_OVER_TPB_DIM)]
    return [(B, d, flip, shift, ts) for (B, d) in shapes for flip in (0, 1) for shift in (0, 1) for ts in (0, 1, 2) if not (shift == 1 and d // 2 == 1)]


def temb_t(B, t_stride):
    """(logical timesteps [B], the int64 buffer the kernel reads with t_stride).  Stride 0: every row reads t[0] = 999 and the other entries must
    be ignored; stride 2: the odd entries hold a value that must never be read"""
    t = list(TEMB_T[:B])
    if t_stride == 0:
        buf = [999] + [123456] * B
        return torch.full((B,), 999, dtype=torch.int64), torch.tensor(buf, dtype=torch.int64)
    buf = torch.full((B * t_stride,), 123456, dtype=torch.int64)
    buf[::t_stride] = torch.tensor(t)
    return torch.tensor(t, dtype=torch.int64), buf


def temb_ref(t, dim, flip, shift):
    """oracle.unet_ref.timestep_embedding, with the zero column an odd dim gets (embeddings.py:56-57)"""
    from oracle import unet_ref as U
    e = U.timestep_embedding(t, dim, bool(flip), shift)
    if dim & 1:
        e = torch.cat([e, torch.zeros(e.shape[0], 1)], 1)
    return e


# ------------------------------------------------------------------------------------------------ FID: convolution
def _cv(name, B, H, W, Cin, Cout, k, stride, pad, why, relu=1, bias=True, xslice=False):
    return NS(name=name, B=B, H=H, W=W, Cin=Cin, Cout=Cout, KH=k[0], KW=k[1], sh=stride[0], sw=stride[1], ph=pad[0], pw=pad[1], relu=relu, bias=bias,
              xslice=xslice, why=why, Ho=(H + 2 * pad[0] - k[0]) // stride[0] + 1, Wo=(W + 2 * pad[1] - k[1]) // stride[1] + 1)


CONV_CASES = [
    _cv("cin3", 2, 7, 7, 3, 4, (3, 3), (2, 2), (0, 0), "Cin 3: scalar loaders, 13 of 16 K rows of a chunk masked; Cout 4: one quad; 3x3 s2 p0"),
    _cv("cin5", 1, 5, 5, 5, 36, (1, 1), (1, 1), (0, 0), "Cin 5: scalar loaders across a quad boundary; Cout 36 ends inside a tile", relu=0),
    _cv("cin17", 1, 6, 6, 17, 68, (5, 5), (1, 1), (2, 2), "Cin 17: a second 16-chunk with one live row; Cout 68: a second N tile with 4 live columns; 5x5 p2"),
    _cv("cin20", 1, 4, 9, 20, 8, (1, 7), (1, 1), (0, 3), "Cin 20: float4 loaders with ci + 4 >= Cin in the second chunk's first half; 1x7 p(0,3)", relu=0),
    _cv("k2048", 1, 2, 3, 2048, 4, (1, 1), (1, 1), (0, 0), "Cin 2048 at 1x1: the longest K, 128 chunks through both LDS buffers"),
    _cv("m1", 1, 3, 3, 4, 4, (3, 3), (1, 1), (0, 0), "M = 1: one live row in the pixel tile, every other pixel masked", relu=0),
    _cv("m_bm", 1, 5, 13, 8, 8, (1, 1), (1, 1), (0, 0), "M = IC_BM + 1: a second pixel tile of the 64-row kernel with one row"),
    _cv("m_bm2", 3, 1, 43, 4, 8, (1, 1), (1, 1), (0, 0), "M = IC2_BM + 1: a second pixel tile of the 128-row kernel with one row", relu=0),
    _cv("k7x1", 2, 9, 4, 8, 12, (7, 1), (1, 1), (3, 0), "7x1 p(3,0): padding along H only"),
    _cv("uneq", 2, 7, 5, 6, 8, (3, 3), (2, 1), (0, 2), "stride_h 2, stride_w 1, pad_h 0, pad_w 2: a stride or pad taken from the other axis", relu=0),
    _cv("nobias", 1, 4, 4, 8, 8, (3, 3), (1, 1), (1, 1), "relu = 0 with bias = NULL: negative outputs survive, no bias read", relu=0, bias=False),
    _cv("xslice4", 2, 5, 5, 8, 8, (3, 3), (1, 1), (1, 1), "x is channels 8..16 of a 24-wide NaN buffer (Cin % 4 == 0: float4 loads with ldx)", xslice=True),
    _cv("xslice5", 2, 5, 5, 5, 8, (3, 3), (1, 1), (1, 1), "x is channels 8..13 of a 21-wide NaN buffer (Cin % 4 != 0: scalar loads with ldx)", xslice=True,
        relu=0),
]
for _c in CONV_CASES:
    _c.M = _c.B * _c.Ho * _c.Wo
CONV_X_OFFSET, CONV_X_EXTRA = 8, 16       # x slices: channel offset 8 of a buffer Cin + 16 wide
CONV_Y_OFFSET, CONV_Y_EXTRA = 4, 8        # y: channel offset 4 of a buffer Cout + 8 wide (the layout of test_conv2d_nhwc_vs_torch)


def conv_data(c):
    """x [B, Cin, H, W] ints in [-4, 4], w [Cout, Cin, KH, KW] = 0.25 * ints in [-2, 2], bias ints in [-8, 8] (None when the case has none)"""
    seed = sum(ord(ch) for ch in c.name)
    x = ints((c.B, c.Cin, c.H, c.W), -4, 4, seed)
    w = 0.25 * ints((c.Cout, c.Cin, c.KH, c.KW), -2, 2, seed + 1)
    b = ints(c.Cout, -8, 8, seed + 2) if c.bias else None
    return x, w, b


def conv_ref(c, x, w, b, dtype=torch.float64):
    """NHWC [B, Ho, Wo, Cout] in `dtype`"""
    y = F.conv2d(x.to(dtype), w.to(dtype), None if b is None else b.to(dtype), (c.sh, c.sw), (c.ph, c.pw))
    if c.relu:
        y = F.relu(y)
    return y.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ FID: pools, global mean, resize
POOL_SETTINGS = ((3, 2, 0, 0, 0), (3, 1, 1, 0, 0), (3, 1, 1, 1, 0), (3, 1, 1, 1, 1))      # (kernel, stride, pad, mode 0 max / 1 avg, count_include_pad)
POOL_SHAPES = ((1, 3, 3, 4), (3, 17, 15, 24), (2, 8, 6, 8))     # (B, H, W, C): a 1x1 output at 3/2/0; ragged; even sizes drop the last window at 3/2/0
POOL_SLICE = NS(shape=(3, 17, 15, 24), ldx=32, xoff=4, ldy=40, yoff=8)       # C = 24 as slices of 32- and 40-wide NaN buffers


def pool_data(shape, negative):
    """[B, C, H, W] ints in [-8, 8], or in [-8, -1]: with zero padding a border maximum of an all-negative image comes out 0"""
    B, H, W, C = shape
    return ints((B, C, H, W), -8, -1 if negative else 8, B * 100 + C + int(negative))


def pool_ref(x, setting, dtype=torch.float32):
    """NHWC.  Average: the exact integer sum divided once (torch's CPU kernel does just that; the host test proves fp32 == fp64 on this data)"""
    k, s, p, mode, cip = setting
    x = x.to(dtype)
    y = F.max_pool2d(x, k, s, p) if mode == 0 else F.avg_pool2d(x, k, s, p, count_include_pad=bool(cip))
    return y.permute(0, 2, 3, 1).contiguous()


GAP_SHAPES = ((1, 1, 1), (3, 35, 100))     # (B, HW, C): one thread; B * C = 300 threads, a ragged second block
GAP_LD_EXTRA = 4


def gap_data(B, HW, C):
    return ints((B, HW, C), -8, 8, B + HW + C)


def gap_ref(x, dtype=torch.float32):
    return x.to(dtype).sum(1) / x.shape[1]


RESIZE_EXACT = (((4, 4), (8, 8)), ((3, 5), (6, 10)), ((8, 6), (4, 3)), ((5, 7), (5, 7)))      # 2x up (square, ragged), 2x down, identity
RESIZE_C = (1, 3, 4)
RESIZE_B = 2
RESIZE_RANDOM = (((32, 32), (299, 299)), ((400, 301), (299, 299)))


def resize_data(src, C, u8, seed=0):
    """NHWC [B, H, W, C]: float integers in [-8, 8], or uint8 holding only 0 and 255 (value / 255 is then exactly 0 or 1)"""
    H, W = src
    if u8:
        return (torch.randint(0, 2, (RESIZE_B, H, W, C), generator=gen(H * W + C + seed)) * 255).to(torch.uint8)
    return ints((RESIZE_B, H, W, C), -8, 8, H * W + C + seed)


def resize_ref(x_nhwc, dst, scale, shift, dtype=torch.float64):
    v = x_nhwc.to(dtype)
    if x_nhwc.dtype == torch.uint8:
        v = v / 255
    y = F.interpolate(v.permute(0, 3, 1, 2), size=dst, mode="bilinear", align_corners=False)
    return (scale * y + shift).permute(0, 2, 3, 1).contiguous()
