"""Exact-value tests for every dispatch branch of the split-plane 3x3 convolutions (bd_conv3x3_ps, bd_conv3x3_ps_wgrad: csrc/conv_ps.hip).

The host code of the two entry points picks one of five kernels, a K-split count and a two- or four-stage ring from the batch, the image
size, the channel counts and the CU count.  Each case below pins ONE of those branches -- the test asserts the (profiling class, ksplit) it
expects, from the ABI's plan queries (bd_conv3x3_ps_plan, bd_conv3x3_ps_wgrad_plan), before it looks at a number -- and compares the result with an fp64 F.conv2d on the CPU for EQUALITY.

Equality is possible because the operands lie on grids for which every product and every partial sum, in any order, is an fp32 number:
  * a WIDE operand is an integer in (-2048, 2048) over 2048 (about 69 % of them have a nonzero bf16 lo part, and that lo is exact in bf16);
  * a NARROW operand is one of {-1, -0.5, 0, 0.5, 1}: its lo part is zero;
  * bias, row bias, residual and the previous output are multiples of 1/4 in [-2, 2]; out_scale is 0.5.
Set A multiplies wide activations with narrow weights, set B narrow activations with wide weights (weight gradient: wide x with narrow dy,
and the reverse), so the lo*hi and the hi*lo product are exercised separately, and the dropped lo*lo term is zero.  In BD_MODE_BF16 the
reference contracts the bf16-rounded operands (the bias gradient keeps the unrounded dy in both modes); for both sets that reference differs
from the three-product one (asserted), so equality there also shows that the lo planes were not read.
test_operand_grids_keep_every_sum_exact (no GPU) proves the precondition for every case and set: max(|a| (*) |b|) in grid units < 2^24.

The outputs are written into a NaN-filled buffer with a guard band behind the last row: a row the ragged-tile masks forget stays NaN, a
store past M lands in the band.

The branch tables hold for 256 CUs; on another device the GPU tests skip rather than assert a stale table.  Whoever retunes ps_plan or
ps_wgrad_plan moves the cases with it ("Dispatch branches of the split-plane convolutions").

Observed on MI355X (256 CUs): equality holds on the anchor cases the older tests already cover (P10, W6) and on every other case, both modes,
both operand sets, every epilogue -- the bf16 MFMA's fp32 accumulation is exact when every partial sum is representable, so the tests assert
torch.equal and no error bound is needed."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu       # per test, not pytestmark: test_operand_grids_keep_every_sum_exact runs without a device

F32, BF16X3, BF16 = 0, 1, 2
UNIT = 2.0 ** -12           # every product of a wide and a narrow operand (rounded to bf16 or not) is a multiple of it
EXPECTED_CUS = 256

# id: (B, H, W, K, N, directions, large layer?, kernel, ksplit, what the case is there for)
FWD_CASES = {
    "P1": (129, 8, 8, 32, 384, (1,), True, "conv_ps", 1, "99 workgroups (tail of the XCD remap), last tile 64 of 256 rows, shortest K (9 chunks)"),
    "P2": (129, 8, 8, 64, 384, (-1,), True, "conv_ps", 1, "data gradient, ragged"),
    "P3": (125, 8, 8, 96, 384, (1,), True, "conv_ps", 1, "96 workgroups, ragged, K not a multiple of 128"),
    "P4": (20, 32, 32, 128, 128, (1, -1), False, "conv_ps128", 1, "in-kernel epilogue, whole tiles"),
    "P5": (259, 8, 8, 32, 128, (1,), False, "conv_ps128", 1, "in-kernel epilogue, last tile 64 of 128 rows"),
    "P6": (33, 8, 8, 256, 128, (-1,), False, "conv_ps128", 15, "four-stage ring, 14 slices of 5 chunks and one of 2, ragged, 255 workgroups"),
    "P7": (129, 8, 8, 128, 128, (1,), False, "conv_ps128", 3, "two-stage split form (12 chunks per slice), ragged"),
    "P8": (3, 4, 4, 32, 128, (1,), False, "conv_ps128", 2, "four-stage, 5 + 4 chunks: a slice that starts inside a tap window; grid of 2"),
    "P9": (3, 2, 2, 128, 128, (1, -1), False, "conv_ps128", 9, "every pixel is a border pixel"),
    "P10": (48, 16, 16, 128, 256, (1,), True, "conv_ps3", 1, "the anchor: a branch the older tests cover"),
    "P11": (96, 16, 16, 128, 128, (-1,), True, "conv_ps3", 1, "data gradient"),
}
# id: (B, H, W, Cin, Cout, strip-order kernel?, ksplit, what for)
WGRAD_CASES = {
    "W1": (129, 4, 4, 128, 128, False, 8, "7 slices of 9 chunks and one of 2; ragged last chunk (2064 pixels); conv_ps_wgrad_reduce<false>"),
    "W2": (33, 8, 8, 128, 128, False, 8, "last slice 3 chunks, whole chunks"),
    "W3": (65, 4, 4, 256, 128, False, 4, "ragged, two ci tiles per tap"),
    "W4": (5, 4, 4, 128, 128, False, 1, "no split: ragged, written straight to dw and db"),
    "W5": (3, 2, 2, 128, 128, False, 1, "one ragged chunk"),
    "W6": (9, 16, 16, 128, 256, True, 9, "conv_ps_wgrad3_kernel: the anchor"),
}
FWD_PARAMS = [pytest.param(cid, d, s, id=f"{cid}-{'fwd' if d > 0 else 'dgrad'}-{s}")
              for cid, c in FWD_CASES.items() for d in c[5] for s in "AB"]
WGRAD_PARAMS = [pytest.param(cid, s, id=f"{cid}-{s}") for cid in WGRAD_CASES for s in "AB"]


# ------------------------------------------------------------------------------------------------ operands (CPU, deterministic)
def _wide(g, *shape):
    return torch.randint(-2047, 2048, shape, generator=g).float() / 2048


def _narrow(g, *shape):
    return torch.randint(-2, 3, shape, generator=g).float() / 2


def _quarters(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).float() / 4


def rnd(x):
    """bf16 RNE of x, as fp32"""
    return x.to(torch.bfloat16).float()


def fwd_operands(cid, direction, opset):
    """direction +1: x [B,H,W,K], w [N,3,3,K] (the convolution's input and weight).  direction -1: x is dY [B,H,W,K] and w [K,3,3,N] the
    SAME convolution's weight [Cout = K][3][3][Cin = N], whose transpose planes (bd_split_wt) the kernel reads."""
    B, H, W, K, N = FWD_CASES[cid][:5]
    g = torch.Generator().manual_seed(1000 * int(cid[1:]) + 10 * (direction > 0) + (opset == "A"))
    a_gen, w_gen = (_wide, _narrow) if opset == "A" else (_narrow, _wide)
    wshape = (N, 3, 3, K) if direction > 0 else (K, 3, 3, N)
    return dict(x=a_gen(g, B, H, W, K), w=w_gen(g, *wshape), bias=_quarters(g, N), rowbias=_quarters(g, B, N),
                residual=_quarters(g, B, H, W, N), prev=_quarters(g, B, H, W, N))


def wgrad_operands(cid, opset):
    B, H, W, Cin, Cout = WGRAD_CASES[cid][:5]
    g = torch.Generator().manual_seed(2000 * int(cid[1:]) + (opset == "A"))
    x_gen, dy_gen = (_wide, _narrow) if opset == "A" else (_narrow, _wide)
    return dict(x=x_gen(g, B, H, W, Cin), dy=dy_gen(g, B, H, W, Cout))


# ------------------------------------------------------------------------------------------------ fp64 references (CPU)
def conv64(x, w, direction):
    """fp64 F.conv2d, NHWC in and out.  -1: the data gradient dx[p][ci] = sum_{tap,co} dy[p - tap][co] w[co][tap][ci] as the convolution of
    dY with the spatially flipped, channel-transposed weight"""
    xn = x.double().permute(0, 3, 1, 2)
    wn = w.double().permute(0, 3, 1, 2) if direction > 0 else w.double().flip(1, 2).permute(3, 0, 1, 2)
    return F.conv2d(xn, wn, None, padding=1).permute(0, 2, 3, 1).contiguous()


def wgrad64(x, dy):
    """fp64 autograd of F.conv2d with respect to its weight -> [Cout,3,3,Cin]"""
    w0 = torch.zeros(dy.shape[-1], x.shape[-1], 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().permute(0, 3, 1, 2), w0, None, padding=1).backward(dy.double().permute(0, 3, 1, 2))
    return w0.grad.permute(0, 2, 3, 1).contiguous()


def epilogue64(conv, o, epi, bias):
    """y = out_scale * (conv + bias + rowbias + residual) (+ previous y): EPI bits 1 = residual, 2 = row bias, 4 = accumulate"""
    y = conv.clone()
    if bias:
        y += o["bias"].double()
    if epi & 2:
        y += o["rowbias"].double()[:, None, None, :]
    if epi & 1:
        y += o["residual"].double()
    y *= 0.5
    if epi & 4:
        y += o["prev"].double()
    return y


# ------------------------------------------------------------------------------------------------ the precondition (no GPU)
def _check_split(x, wide):
    hi = rnd(x)
    lo = x - hi
    assert torch.equal(rnd(lo), lo), "lo part not exact in bf16"
    assert torch.equal(hi + lo, x)
    if wide:
        assert float((lo != 0).float().mean()) >= 0.5, float((lo != 0).float().mean())
    else:
        assert not bool(lo.any())


def _mag(x):
    """|x| or |bf16(x)|, whichever is larger: covers both modes' operands"""
    return torch.maximum(x.abs(), rnd(x).abs())


@pytest.mark.parametrize("cid,direction,opset", FWD_PARAMS)
def test_operand_grids_keep_every_sum_exact(cid, direction, opset):
    """every partial sum of the forward / data-gradient cases, epilogue addends included, stays below 2^24 grid units: exact in fp32 in any
    order of summation; hi + lo == x with lo exact in bf16; at least half the wide values have a lo part"""
    o = fwd_operands(cid, direction, opset)
    _check_split(o["x"], opset == "A"); _check_split(o["w"], opset == "B")
    worst = conv64(_mag(o["x"]), _mag(o["w"]), direction)
    # out_scale * (conv + bias + rowbias + residual) + prev = 0.5 * (... + 2 prev): the sum in front of the scale lives on the UNIT grid
    worst += o["bias"].abs().double() + o["rowbias"].abs().double()[:, None, None, :] + o["residual"].abs().double() + 2 * o["prev"].abs().double()
    units = float(worst.max()) / UNIT
    print(f"MEASURE exact_units {cid} dir {direction} set {opset} {units / 2 ** 24:.3f} x 2^24")
    assert units < 2 ** 24, units


@pytest.mark.parametrize("cid,opset", WGRAD_PARAMS)
def test_operand_grids_keep_every_wgrad_sum_exact(cid, opset):
    """the same for the weight gradient (sums over all pixels) and the bias gradient (sums of the unrounded dy, grid 2^-11)"""
    o = wgrad_operands(cid, opset)
    _check_split(o["x"], opset == "A"); _check_split(o["dy"], opset == "B")
    units = float(wgrad64(_mag(o["x"]), _mag(o["dy"])).max()) / UNIT
    db_units = float(o["dy"].abs().double().sum(dim=(0, 1, 2)).max()) * 2048
    print(f"MEASURE exact_units {cid} set {opset} dw {units / 2 ** 24:.3f} db {db_units / 2 ** 24:.3f} x 2^24")
    assert units < 2 ** 24 and db_units < 2 ** 24, (units, db_units)


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


def prof_counts(lib, L):
    out = {}
    for c in range(lib.bd_prof_num_classes()):
        name = ctypes.c_char_p(); n = ctypes.c_int64(); ms = ctypes.c_double(); fl = ctypes.c_double(); by = ctypes.c_double()
        L.check(lib.bd_prof_get(c, ctypes.byref(name), ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)), "bd_prof_get")
        if n.value:
            out[name.value.decode()] = int(n.value)
    return out


def bracketed(fn):
    """run fn() with the profiler's event brackets on -> (result, {class: launches})"""
    from baddiffusion_amd import _lib as L
    lib = L.load()
    torch.cuda.synchronize()
    lib.bd_prof_reset(); lib.bd_prof_enable(1)
    try:
        res = fn()
        torch.cuda.synchronize()
        counts = prof_counts(lib, L)
    finally:
        torch.cuda.synchronize()
        lib.bd_prof_enable(0); lib.bd_prof_reset()
    return res, counts


def describe(got, ref, grid=None):
    """where a result differs from the reference: the pattern names the rows, columns (taps / K slices show as value patterns) at fault.
    grid = (H, W) of the image the rows are pixels of: also the (b, y, x) of the first wrong rows and the x columns that hold one, so that an
    error at a strip seam or on a strip's first row reads as such"""
    got = got.double().cpu().reshape(-1, got.shape[-1]); ref = ref.reshape(-1, ref.shape[-1])
    bad = ~(got == ref)
    if not bool(bad.any()):
        return "equal"
    rows = bad.any(dim=1).nonzero().flatten(); cols = bad.any(dim=0).nonzero().flatten()
    d = (got - ref)[bad]
    where = ""
    if grid is not None:
        H, W = grid
        bxy = [(r // (H * W), r // W % H, r % W) for r in rows[:8].tolist()]
        where = f"; (b, y, x) of the first rows {bxy}; x of all wrong rows {sorted(set((rows % W).tolist()))[:16]}, y {sorted(set((rows // W % H).tolist()))[:16]}"
    return (f"{int(bad.sum())} of {bad.numel()} elements differ ({int(torch.isnan(got[bad]).sum())} NaN); rows {int(rows[0])}..{int(rows[-1])} "
            f"({rows.numel()} rows, first {rows[:8].tolist()}), columns {int(cols[0])}..{int(cols[-1])} ({cols.numel()}); "
            f"max |diff| {float(d.abs().nan_to_num().max()):.6g}{where}")


@gpu
@pytest.mark.parametrize("cid,direction,opset", FWD_PARAMS)
def test_conv_ps_branch_is_exact(ops, cid, direction, opset):
    """bd_conv3x3_ps on the pinned branch equals the fp64 convolution, in both modes, for every epilogue combination of {residual, row bias,
    accumulate} (forward: bias present; data gradient: EPI 0 and accumulate), out_scale 0.5"""
    from baddiffusion_amd import _lib as L
    lib = L.load()
    B, H, W, K, N, _, large, kernel, ksplit, _ = FWD_CASES[cid]
    M = B * H * W
    # ---- the branch, before anything is launched: what the launcher's own plan says
    plan = ops.conv3x3_ps_plan(B, H, W, K, N, direction, mode=BF16X3)
    d = L.ConvPsDesc(B=B, H=H, W=W, K=K, N=N, direction=direction, mode=BF16X3)
    assert plan["ksplit"] == ksplit and plan["workspace_bytes"] == lib.bd_conv3x3_ps_workspace_bytes(ctypes.byref(d)), (cid, plan)
    assert kernel == {L.PS_128: "conv_ps128", L.PS_256_SHARED_TAP: "conv_ps3", L.PS_256: "conv_ps"}[plan["kernel"]], (cid, plan)
    assert large == (plan["kernel"] != L.PS_128), (cid, plan)
    cls = ("conv_ps" if large else "conv_ps128") + ("_fwd" if direction > 0 else "_dgrad")
    assert plan["prof_class"] == cls, (cid, plan)

    o = fwd_operands(cid, direction, opset)
    dev = {k: v.cuda() for k, v in o.items()}
    xs = ops.split_rows(dev["x"])
    ws = ops.split_bf16(dev["w"]) if direction > 0 else ops.split_wT(dev["w"])
    epis = range(8) if direction > 0 else (0, 4)
    refs = {}
    for mode in (BF16X3, BF16):
        prep = rnd if mode == BF16 else (lambda t: t)
        conv = refs[mode] = conv64(prep(o["x"]), prep(o["w"]), direction)
        for n_epi, epi in enumerate(epis):
            ref = epilogue64(conv, o, epi, bias=direction > 0)
            buf = torch.full((M + 256, N), float("nan"), device="cuda")       # guard band of 256 rows behind the last pixel
            if epi & 4:
                buf[:M] = dev["prev"].reshape(M, N)
            run = lambda: ops.conv3x3_ps(xs, ws, B, H, W, K, N, direction, bias=dev["bias"] if direction > 0 else None,
                                         rowbias=dev["rowbias"] if epi & 2 else None, residual=dev["residual"] if epi & 1 else None,
                                         out_scale=0.5, out=buf[:M].view(B, H, W, N), accumulate=bool(epi & 4), mode=mode)
            if n_epi == 0:
                got, counts = bracketed(run)
                want = cls + ("_bf16" if mode == BF16 else "")
                assert {k: v for k, v in counts.items() if k.startswith("conv_ps")} == {want: 1}, (cid, mode, counts)
            else:
                got = run()
            assert torch.equal(got.double().cpu(), ref), (cid, direction, opset, mode, epi, describe(got, ref))
            assert bool(torch.isnan(buf[M:]).all()), (cid, direction, opset, mode, epi, "store past the last row")
    assert not torch.equal(refs[BF16X3], refs[BF16])      # the two modes have different answers here: bf16 equality => lo planes unread


@gpu
@pytest.mark.parametrize("cid,opset", WGRAD_PARAMS)
def test_conv_ps_wgrad_branch_is_exact(ops, cid, opset):
    """bd_conv3x3_ps_wgrad on the pinned branch: dw equals fp64 autograd (of the bf16-rounded operands in BD_MODE_BF16), db the fp64 sum of the
    unrounded dy in both modes, and dw without db is the same dw"""
    from baddiffusion_amd import _lib as L
    lib = L.load()
    B, H, W, Cin, Cout, strip, ksplit, _ = WGRAD_CASES[cid]
    plan = ops.conv3x3_ps_wgrad_plan(B, H, W, Cin, Cout, mode=BF16X3)              # the branch, before anything is launched
    d = L.ConvPsWgradDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, mode=BF16X3)
    assert plan["ksplit"] == ksplit and plan["workspace_bytes"] == lib.bd_conv3x3_ps_wgrad_workspace_bytes(ctypes.byref(d)), (cid, plan)
    assert strip == (plan["kernel"] == L.PS_WGRAD_SHARED_TAP), (cid, plan)
    cls = "conv_ps_wgrad3" if strip else "conv_ps_wgrad"
    assert plan["prof_class"] == cls, (cid, plan)

    o = wgrad_operands(cid, opset)
    xs, dys = ops.split_rows(o["x"].cuda()), ops.split_rows(o["dy"].cuda())
    db_ref = o["dy"].double().sum(dim=(0, 1, 2))
    refs = {}
    for mode in (BF16X3, BF16):
        prep = rnd if mode == BF16 else (lambda t: t)
        dw_ref = refs[mode] = wgrad64(prep(o["x"]), prep(o["dy"]))
        (dw, db), counts = bracketed(lambda: ops.conv3x3_ps_wgrad(xs, dys, B, H, W, Cin, Cout, with_db=True, mode=mode))
        want = cls + ("_bf16" if mode == BF16 else "")
        assert {k: v for k, v in counts.items() if k.startswith("conv_ps")} == {want: 1}, (cid, mode, counts)
        assert torch.equal(dw.double().cpu(), dw_ref), (cid, opset, mode, "dw", describe(dw.reshape(Cout, -1), dw_ref.reshape(Cout, -1)))
        assert torch.equal(db.double().cpu(), db_ref), (cid, opset, mode, "db", describe(db[None], db_ref[None]))
        dw_only = ops.conv3x3_ps_wgrad(xs, dys, B, H, W, Cin, Cout, mode=mode)
        assert torch.equal(dw_only, dw), (cid, opset, mode, "dw without db", describe(dw_only.reshape(Cout, -1), dw.double().cpu().reshape(Cout, -1)))
    assert not torch.equal(refs[BF16X3], refs[BF16])
