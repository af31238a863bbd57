"""GPU: exact values and edges of the small training / sampling ops (csrc/elementwise.hip) and of the FID kernels (csrc/inception.hip).

Cases, data and fp64 references come from tests/_small_exact.py; tests/test_small_exact_host.py proves on the CPU that the data is rounding-free
(so the assertion here is torch.equal, whatever order a kernel sums in) and that the sizes follow the constants in the sources.  Every output
sits in a NaN-filled buffer with margins: whatever lies outside the written region must still be NaN afterwards, an output written with
accumulate = 0 starts as NaN and must come out finite, and inputs with ld > C carry NaN in the unused columns.  Tolerances appear in four
places only -- SiLU, random softmax rows, the timestep embedding and the random uint8 resize -- and are the ones tests/test_hip_ops.py and
tests/test_hip_round4.py already use for these kernels."""
import ctypes as CT

import numpy as np
import pytest
import torch

from tests import _small_exact as S

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -2        # enum bd_status
LEAD, TRAIL = 4, 4                   # floats of NaN margin (16 bytes: the views stay 16-byte aligned)
U8_MARGIN, U8_SENTINEL = 8, 0xA5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def lib(gpu):
    from baddiffusion_amd import _lib as L
    L.load()
    return L


def close(a, b, rtol, atol):
    np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy(), rtol=rtol, atol=atol)


def view(buf, rows, C, ld, lead=LEAD):
    return S.rows_view(buf, lead, rows, C, ld)


def result(buf, rows, C, ld, lead=LEAD, finite=True):
    """host copy of the [rows, C] view of an output buffer, after checking that nothing outside it was written and nothing inside was left NaN"""
    host = buf.cpu()
    assert S.outside_is_nan(host, lead, rows, C, ld), "written outside the output"
    out = view(host, rows, C, ld, lead).clone()
    if finite:
        assert bool(torch.isfinite(out).all()), "output left unwritten or not finite"
    return out


def untouched(buf):
    return bool(torch.isnan(buf).all())


# ================================================================================================ training-path ops
@pytest.mark.parametrize("rows", S.SOFTMAX_ROWS)
@pytest.mark.parametrize("n", S.SOFTMAX_N)
def test_softmax_fwd(gpu, lib, rows, n):
    L, l = lib, lib.load()
    trail = n + 8                       # a wave past `rows` would write the next row: the margin holds one
    for name, (s, exact) in S.softmax_inputs(rows, n).items():
        ref = S.softmax_ref(s)
        sb = S.padded(s, LEAD, trail).to(gpu)
        pb = S.nan_rows(rows, n, n, LEAD, trail).to(gpu)
        sv, pv = view(sb, rows, n, n), view(pb, rows, n, n)
        L.check(l.bd_softmax_fwd(sv.data_ptr(), pv.data_ptr(), rows, n, L.stream()), "bd_softmax_fwd")
        p = result(pb, rows, n, n)
        if exact:
            assert torch.equal(p, ref.float()), (name, float((p - ref).abs().max()))
        else:
            close(p, ref, 1e-5, 1e-6)
        if name == "ninf":
            assert bool((p[torch.isinf(s)] == 0).all()) and bool((p[~torch.isinf(s)] > 0).all())
        # in place, as the UNet plan calls it (bd_softmax_fwd(P, P))
        L.check(l.bd_softmax_fwd(sv.data_ptr(), sv.data_ptr(), rows, n, L.stream()), "bd_softmax_fwd")
        assert torch.equal(result(sb, rows, n, n), p), name


@pytest.mark.parametrize("rows", S.SOFTMAX_ROWS)
@pytest.mark.parametrize("n", S.SOFTMAX_N)
def test_softmax_bwd(gpu, lib, rows, n):
    L, l = lib, lib.load()
    trail = n + 8
    for name, (p, dp, exact) in S.softmax_bwd_inputs(rows, n).items():
        ref = S.softmax_bwd_ref(p, dp)
        pb, db = S.padded(p, LEAD, trail).to(gpu), S.padded(dp, LEAD, trail).to(gpu)
        ob = S.nan_rows(rows, n, n, LEAD, trail).to(gpu)
        pv, dv, ov = view(pb, rows, n, n), view(db, rows, n, n), view(ob, rows, n, n)
        L.check(l.bd_softmax_bwd(pv.data_ptr(), dv.data_ptr(), ov.data_ptr(), rows, n, L.stream()), "bd_softmax_bwd")
        ds = result(ob, rows, n, n)
        if exact:
            assert torch.equal(ds, ref.float()), (name, float((ds - ref).abs().max()))
        else:
            close(ds, ref, 1e-4, 1e-6)
        # in place, as the UNet plan calls it (bd_softmax_bwd(P, dP, dP))
        L.check(l.bd_softmax_bwd(pv.data_ptr(), dv.data_ptr(), dv.data_ptr(), rows, n, L.stream()), "bd_softmax_bwd")
        assert torch.equal(result(db, rows, n, n), ds), name
        assert torch.equal(result(pb, rows, n, n), p), name


@pytest.mark.parametrize("c", S.COLSUM_CASES, ids=lambda c: f"{c.rows}x{c.N}r{c.rpg}a{c.acc}")
def test_colsum(gpu, lib, c):
    L, l = lib, lib.load()
    x, pre = S.colsum_data(c)
    xb = S.strided_rows(x, c.ldx, LEAD, TRAIL)[1].to(gpu)
    ob = (S.strided_rows(pre, c.ldo, LEAD, TRAIL)[1] if c.acc else S.nan_rows(c.groups, c.N, c.ldo, LEAD, TRAIL)).to(gpu)
    L.check(l.bd_colsum(view(xb, c.rows, c.N, c.ldx).data_ptr(), c.ldx, c.rows, c.N, c.rpg, view(ob, c.groups, c.N, c.ldo).data_ptr(), c.ldo, c.acc,
                        L.stream()), "bd_colsum")
    out = result(ob, c.groups, c.N, c.ldo)
    ref = S.colsum_ref(c, x, pre)
    assert torch.equal(out, ref.float()), (c.why, float((out - ref).abs().max()))


def test_colsum_rejections(gpu, lib):
    L, l = lib, lib.load()
    x = torch.zeros(65536 + 8, device=gpu)
    out = torch.full((65536 + 8,), S.NAN, device=gpu)
    st = L.stream()
    assert l.bd_colsum(x.data_ptr(), 1, 65536, 1, 1, out.data_ptr(), 1, 0, st) == UNSUPPORTED and b"groups" in l.bd_last_error()
    assert l.bd_colsum(x.data_ptr(), 1, 65535, 1, 1, out.data_ptr(), 1, 0, st) == 0          # the limit itself is taken
    torch.cuda.synchronize()
    assert bool((out[:65535] == 0).all()) and untouched(out[65535:])
    out.fill_(S.NAN)
    for rpg in (0, -1):
        assert l.bd_colsum(x.data_ptr(), 8, 16, 8, rpg, out.data_ptr(), 8, 0, st) == INVALID
    assert l.bd_colsum(x.data_ptr(), 7, 16, 8, 4, out.data_ptr(), 8, 0, st) == INVALID and b"ldx" in l.bd_last_error()
    assert l.bd_colsum(x.data_ptr(), 8, 16, 8, 4, out.data_ptr(), 7, 0, st) == INVALID
    torch.cuda.synchronize()
    assert untouched(out)


@pytest.mark.parametrize("c", S.SUM2X2_CASES, ids=lambda c: f"{c.B}x{c.H}x{c.W}x{c.C}")
def test_sum2x2(gpu, lib, c):
    L, l = lib, lib.load()
    du, pre = S.sum2x2_data(c)
    rows = c.B * c.H * c.W
    ub = S.strided_rows(du.reshape(4 * rows, c.C), c.ldu, LEAD, TRAIL)[1].to(gpu)
    ob = (S.strided_rows(pre.reshape(rows, c.C), c.lddx, LEAD, TRAIL)[1] if c.acc else S.nan_rows(rows, c.C, c.lddx, LEAD, TRAIL)).to(gpu)
    L.check(l.bd_sum2x2(view(ub, 4 * rows, c.C, c.ldu).data_ptr(), c.ldu, view(ob, rows, c.C, c.lddx).data_ptr(), c.lddx, c.B, c.H, c.W, c.C, c.acc,
                        L.stream()), "bd_sum2x2")
    out = result(ob, rows, c.C, c.lddx)
    ref = S.sum2x2_ref(c, du, pre).reshape(rows, c.C)
    assert torch.equal(out, ref.float()), (c.why, float((out - ref).abs().max()))


def test_sum2x2_rejections(gpu, lib):
    L, l = lib, lib.load()
    du = torch.zeros(4096, device=gpu)
    dx = torch.full((4096,), S.NAN, device=gpu)
    u, x, st = du.data_ptr(), dx.data_ptr(), L.stream()
    for args in ((u, 8, x, 8, 1, 2, 2, 6), (u, 10, x, 8, 1, 2, 2, 8), (u, 8, x, 10, 1, 2, 2, 8), (u + 4, 8, x, 8, 1, 2, 2, 8), (u, 8, x + 4, 8, 1, 2, 2, 8)):
        assert l.bd_sum2x2(*args, 0, st) == UNSUPPORTED and b"bd_sum2x2" in l.bd_last_error(), args
    for args in ((u, 4, x, 8, 1, 2, 2, 8), (u, 8, x, 4, 1, 2, 2, 8)):
        assert l.bd_sum2x2(*args, 0, st) == INVALID and b"< C" in l.bd_last_error(), args
    torch.cuda.synchronize()
    assert untouched(dx)


@pytest.mark.parametrize("c", S.ADD_CASES, ids=lambda c: f"{c.rows}x{c.C}")
def test_add(gpu, lib, c):
    L, l = lib, lib.load()
    src, pre = S.add_data(c)
    sb = S.strided_rows(src, c.lds, LEAD, TRAIL)[1].to(gpu)
    for scale, acc in c.combos:
        ob = (S.strided_rows(pre, c.ldd, LEAD, TRAIL)[1] if acc else S.nan_rows(c.rows, c.C, c.ldd, LEAD, TRAIL)).to(gpu)
        L.check(l.bd_add(view(sb, c.rows, c.C, c.lds).data_ptr(), c.lds, view(ob, c.rows, c.C, c.ldd).data_ptr(), c.ldd, c.rows, c.C, scale, acc,
                         L.stream()), "bd_add")
        out = result(ob, c.rows, c.C, c.ldd)
        assert torch.equal(out, S.axpy_ref(src, pre, scale, acc).float()), (c.why, scale, acc)
    assert torch.equal(view(sb.cpu(), c.rows, c.C, c.lds), src)


def test_add_rejections(gpu, lib):
    L, l = lib, lib.load()
    src = torch.zeros(4096, device=gpu)
    dst = torch.full((4096,), S.NAN, device=gpu)
    s, d, st = src.data_ptr(), dst.data_ptr(), L.stream()
    for args in ((s, 8, d, 8, 4, 6), (s, 10, d, 8, 4, 8), (s, 8, d, 10, 4, 8), (s + 4, 8, d, 8, 4, 8), (s, 8, d + 4, 8, 4, 8)):
        assert l.bd_add(*args, 1.0, 0, st) == UNSUPPORTED, args
    for args in ((s, 4, d, 8, 4, 8), (s, 8, d, 4, 4, 8), (s, 8, d, 8, 0, 8), (None, 8, d, 8, 4, 8)):
        assert l.bd_add(*args, 1.0, 0, st) == INVALID, args
    torch.cuda.synchronize()
    assert untouched(dst)


def sumsq_call(L, l, gpu, xv):
    out = torch.full((3,), S.NAN, dtype=torch.float64, device=gpu)
    ws = torch.empty(l.bd_reduce_workspace_bytes(), dtype=torch.uint8, device=gpu)
    status = l.bd_sumsq(xv.data_ptr(), xv.numel(), out[1:2].data_ptr(), ws.data_ptr(), L.stream())
    out = out.cpu()
    assert bool(torch.isnan(out[0])) and bool(torch.isnan(out[2]))
    return status, float(out[1])


@pytest.mark.parametrize("n", S.SUMSQ_N)
def test_sumsq(gpu, lib, n):
    L, l = lib, lib.load()
    x = S.sumsq_data(n)
    xb = S.padded(x, LEAD, TRAIL).to(gpu)
    status, got = sumsq_call(L, l, gpu, xb[LEAD: LEAD + n])
    assert status == 0 and got == float((x.double() ** 2).sum()), (got, float((x.double() ** 2).sum()))


def test_sumsq_squares_in_fp64_and_misaligned(gpu, lib):
    L, l = lib, lib.load()
    x, want = S.sumsq_big_values()
    status, got = sumsq_call(L, l, gpu, S.padded(x, LEAD, TRAIL).to(gpu)[LEAD: LEAD + x.numel()])
    assert status == 0 and got == want, (got, want)
    status, got = sumsq_call(L, l, gpu, S.padded(x, 1, TRAIL).to(gpu)[1: 1 + x.numel()])       # 4 bytes off
    assert status == INVALID and np.isnan(got)


@pytest.mark.parametrize("n", S.AXPY_N)
def test_axpy(gpu, lib, n):
    L, l = lib, lib.load()
    src, pre = S.ints(n, -8, 8, n % 9973), S.ints(n, -8, 8, n % 9973 + 1)
    lead = 3                             # scalar accesses: 4-byte alignment is enough
    sb = S.padded(src, lead, TRAIL).to(gpu)
    for scale in S.AXPY_SCALES:
        for acc in (0, 1):
            ob = (S.padded(pre, lead, TRAIL) if acc else S.nan_rows(1, n, n, lead, TRAIL)).to(gpu)
            L.check(l.bd_axpy(sb[lead:].data_ptr(), ob[lead:].data_ptr(), n, scale, acc, L.stream()), "bd_axpy")
            out = result(ob, 1, n, n, lead)[0]
            assert torch.equal(out, S.axpy_ref(src, pre, scale, acc).float()), (n, scale, acc)


@pytest.mark.parametrize("n", S.SILU_N)
def test_silu(gpu, lib, n):
    L, l = lib, lib.load()
    z, dy, pre = S.silu_data(n)
    lead = 1
    zb, gb = S.padded(z, lead, TRAIL).to(gpu), S.padded(dy, lead, TRAIL).to(gpu)
    zp, gp = zb[lead:].data_ptr(), gb[lead:].data_ptr()
    yb = S.nan_rows(1, n, n, lead, TRAIL).to(gpu)
    L.check(l.bd_silu_fwd(zp, yb[lead:].data_ptr(), n, L.stream()), "bd_silu_fwd")
    close(result(yb, 1, n, n, lead)[0], S.silu_ref(z), 1e-6, 1e-6)
    ref = S.silu_bwd_ref(z, dy)
    ob = S.nan_rows(1, n, n, lead, TRAIL).to(gpu)
    L.check(l.bd_silu_bwd(zp, gp, ob[lead:].data_ptr(), n, 0, L.stream()), "bd_silu_bwd")
    dx0 = result(ob, 1, n, n, lead)[0]
    close(dx0, ref, 1e-5, 1e-6)
    # accumulate onto integers: one more fp32 addition on top of the same gradient
    ob = S.padded(pre, lead, TRAIL).to(gpu)
    L.check(l.bd_silu_bwd(zp, gp, ob[lead:].data_ptr(), n, 1, L.stream()), "bd_silu_bwd")
    dx1 = result(ob, 1, n, n, lead)[0]
    close(dx1, ref + pre.double(), 1e-5, 1e-6)
    assert torch.equal(dx1, dx0 + pre)
    # dx aliasing dy
    L.check(l.bd_silu_bwd(zp, gp, gp, n, 0, L.stream()), "bd_silu_bwd")
    assert torch.equal(result(gb, 1, n, n, lead)[0], dx0)
    assert torch.equal(result(zb, 1, n, n, lead)[0], z)


def test_silu_at_zero_is_exact(gpu, lib):
    L, l = lib, lib.load()
    n = 257
    z = torch.zeros(n)
    z[1::2] = -0.0
    dy = S.ints(n, -8, 8, 1)
    zb, gb = z.to(gpu), dy.to(gpu)
    yb, ob = S.nan_rows(1, n, n, LEAD, TRAIL).to(gpu), S.nan_rows(1, n, n, LEAD, TRAIL).to(gpu)
    L.check(l.bd_silu_fwd(zb.data_ptr(), yb[LEAD:].data_ptr(), n, L.stream()), "bd_silu_fwd")
    L.check(l.bd_silu_bwd(zb.data_ptr(), gb.data_ptr(), ob[LEAD:].data_ptr(), n, 0, L.stream()), "bd_silu_bwd")
    assert torch.equal(result(yb, 1, n, n)[0], torch.zeros(n))
    assert torch.equal(result(ob, 1, n, n)[0], S.silu_bwd_ref(z, dy).float()) and torch.equal(result(ob, 1, n, n)[0], 0.5 * dy)


# ================================================================================================ sampling-path small kernels
def u8_buffer(n, gpu):
    return torch.full((U8_MARGIN + n + U8_MARGIN,), U8_SENTINEL, dtype=torch.uint8, device=gpu)


def u8_result(buf, n):
    host = buf.cpu()
    assert bool((host[:U8_MARGIN] == U8_SENTINEL).all()) and bool((host[U8_MARGIN + n:] == U8_SENTINEL).all()), "written outside the output"
    return host[U8_MARGIN: U8_MARGIN + n].clone()


@pytest.mark.parametrize("layout", S.TO_IMAGE_LAYOUTS)
@pytest.mark.parametrize("C", S.TO_IMAGE_C)
def test_to_image(gpu, lib, C, layout):
    L, l = lib, lib.load()
    B, H, W = S.TO_IMAGE_BHW
    x = S.to_image_data(C)
    want_f, want_u = S.to_image_ref(x)
    pix, n = B * H * W, B * H * W * C
    if layout == "nchw":
        xb, ld = S.padded(x, LEAD, TRAIL).to(gpu), C
        xp = xb[LEAD:].data_ptr()
    else:
        ld = C + 5 if layout == "nhwc_ld" else C
        xb = S.strided_rows(x.permute(0, 2, 3, 1).reshape(pix, C), ld, LEAD, TRAIL)[1].to(gpu)
        xp = view(xb, pix, C, ld).data_ptr()
    for want_float, want_u8 in ((1, 0), (0, 1), (1, 1)):
        fb, ub = S.nan_rows(1, n, n, LEAD, TRAIL).to(gpu), u8_buffer(n, gpu)
        L.check(l.bd_to_image(xp, int(layout != "nchw"), ld, B, C, H, W, fb[LEAD:].data_ptr() if want_float else None,
                              ub[U8_MARGIN:].data_ptr() if want_u8 else None, L.stream()), "bd_to_image")
        if want_float:
            assert torch.equal(result(fb, 1, n, n)[0], want_f.reshape(-1)), (C, layout)
        else:
            assert untouched(fb)
        if want_u8:
            assert torch.equal(u8_result(ub, n), want_u.reshape(-1)), (C, layout)
        else:
            assert bool((ub == U8_SENTINEL).all())


def test_to_image_rejects_short_ld(gpu, lib):
    L, l = lib, lib.load()
    x = torch.zeros(256, device=gpu)
    f = torch.full((256,), S.NAN, device=gpu)
    assert l.bd_to_image(x.data_ptr(), 1, 2, 1, 3, 4, 4, f.data_ptr(), None, L.stream()) == INVALID and b"ld" in l.bd_last_error()
    assert l.bd_to_image(x.data_ptr(), 1, 3, 1, 3, 4, 4, None, None, L.stream()) == INVALID
    torch.cuda.synchronize()
    assert untouched(f)


@pytest.mark.parametrize("extra", S.LAYOUT_LD_EXTRA)
@pytest.mark.parametrize("shape", S.LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layout_kernels(gpu, lib, shape, extra):
    L, l = lib, lib.load()
    B, C, H, W = shape
    x = S.layout_data(*shape)
    pix, ld = B * H * W, C + extra
    nhwc = x.permute(0, 2, 3, 1).reshape(pix, C)
    # NCHW -> NHWC with leading dimension ld
    sb = S.padded(x, LEAD, TRAIL).to(gpu)
    ob = S.nan_rows(pix, C, ld, LEAD, TRAIL).to(gpu)
    L.check(l.bd_nchw_to_nhwc(sb[LEAD:].data_ptr(), view(ob, pix, C, ld).data_ptr(), B, C, H, W, ld, L.stream()), "bd_nchw_to_nhwc")
    assert torch.equal(result(ob, pix, C, ld), nhwc)
    # NHWC with leading dimension ld (NaN in the unused columns) -> NCHW
    sb = S.strided_rows(nhwc, ld, LEAD, TRAIL)[1].to(gpu)
    ob = S.nan_rows(1, x.numel(), x.numel(), LEAD, TRAIL).to(gpu)
    L.check(l.bd_nhwc_to_nchw(view(sb, pix, C, ld).data_ptr(), ld, ob[LEAD:].data_ptr(), B, C, H, W, L.stream()), "bd_nhwc_to_nchw")
    assert torch.equal(result(ob, 1, x.numel(), x.numel())[0], x.reshape(-1))


@pytest.mark.parametrize("B,dim", sorted({(B, d) for B, d, *_ in S.temb_cases()}))
def test_timestep_embedding(gpu, lib, B, dim):
    L, l = lib, lib.load()
    half = dim // 2
    for _, _, flip, shift, ts in [c for c in S.temb_cases() if c[:2] == (B, dim)]:
        t, tbuf = S.temb_t(B, ts)
        td = tbuf.to(gpu)
        ob = S.nan_rows(B, dim, dim, LEAD, 2 * TRAIL).to(gpu)
        L.check(l.bd_timestep_embedding(td.data_ptr(), ts, B, dim, flip, float(shift), ob[LEAD:].data_ptr(), L.stream()), "bd_timestep_embedding")
        out = result(ob, B, dim, dim)
        what = (B, dim, flip, shift, ts)
        # sin / cos arguments reach t * f ~ 1e3, where one ulp of expf() in f moves the argument by 6e-5 (test_hip_ops.test_timestep_embedding)
        close(out, S.temb_ref(t, dim, flip, shift), 0, 2e-4)
        sin, cos = (out[:, half:2 * half], out[:, :half]) if flip else (out[:, :half], out[:, half:2 * half])
        z = t == 0
        assert bool((sin[z] == 0).all()) and bool((cos[z] == 1).all()), what
        if dim & 1:
            assert bool((out[:, dim - 1] == 0).all()), what


# ================================================================================================ FID kernels
def conv_desc(L, c, w_kc, **operands):
    """the case's geometry with the given operands (x, ldx, w, bias, y, ldy); any other field given replaces the case's"""
    f = dict(B=c.B, H=c.H, W=c.W, Cin=c.Cin, Cout=c.Cout, KH=c.KH, KW=c.KW, stride_h=c.sh, stride_w=c.sw,
             pad_h=c.ph, pad_w=c.pw, relu=c.relu, w_kc=w_kc)
    f.update(operands)
    return L.Conv2dDesc(**f)


@pytest.mark.parametrize("w_kc", (0, 1), ids=("w_ck_64x64", "w_kc_128x64"))
@pytest.mark.parametrize("c", S.CONV_CASES, ids=lambda c: c.name)
def test_conv2d_nhwc(gpu, lib, c, w_kc):
    L, l = lib, lib.load()
    x, w, b = S.conv_data(c)
    ref = S.conv_ref(c, x, w, b).reshape(c.M, c.Cout)
    pix = c.B * c.H * c.W
    xoff, ldx = (S.CONV_X_OFFSET, c.Cin + S.CONV_X_EXTRA) if c.xslice else (LEAD, c.Cin)
    xb = S.strided_rows(x.permute(0, 2, 3, 1).reshape(pix, c.Cin), ldx, xoff, TRAIL)[1].to(gpu)
    wd = (w.permute(2, 3, 0, 1) if w_kc else w.permute(2, 3, 1, 0)).contiguous().to(gpu)        # [KH][KW][Cout][Cin] / [KH][KW][Cin][Cout]
    bd = None if b is None else b.to(gpu)
    ldy = c.Cout + S.CONV_Y_EXTRA
    yb = S.nan_rows(c.M, c.Cout, ldy, S.CONV_Y_OFFSET, TRAIL).to(gpu)
    d = conv_desc(L, c, w_kc, x=view(xb, pix, c.Cin, ldx, xoff).data_ptr(), ldx=ldx, w=wd.data_ptr(), bias=L.ptr(bd),
                  y=view(yb, c.M, c.Cout, ldy, S.CONV_Y_OFFSET).data_ptr(), ldy=ldy)
    L.check(l.bd_conv2d_nhwc(CT.byref(d), L.stream()), "bd_conv2d_nhwc")
    out = result(yb, c.M, c.Cout, ldy, S.CONV_Y_OFFSET)
    assert torch.equal(out, ref.float()), (c.why, float((out - ref).abs().max()), int((out != ref.float()).sum()))


def test_conv2d_nhwc_rejections(gpu, lib):
    L, l = lib, lib.load()
    c = S.CONV_CASES[-2]                  # xslice4: Cin 8, Cout 8
    x = torch.zeros(4096, device=gpu)
    w = torch.zeros(4096, device=gpu)
    y = torch.full((4096,), S.NAN, device=gpu)
    for w_kc in (0, 1):
        for over, code in ((dict(Cout=6), UNSUPPORTED), (dict(ldx=c.Cin - 1), INVALID), (dict(x=x.data_ptr() + 4), INVALID), (dict(ldx=c.Cin + 2), INVALID),
                           (dict(ldy=c.Cout - 1), INVALID)):
            d = conv_desc(L, c, w_kc, **(dict(x=x.data_ptr(), ldx=c.Cin, w=w.data_ptr(), bias=None, y=y.data_ptr(), ldy=c.Cout) | over))
            assert l.bd_conv2d_nhwc(CT.byref(d), L.stream()) == code and b"bd_conv2d_nhwc" in l.bd_last_error(), (over, w_kc)
    torch.cuda.synchronize()
    assert untouched(y)


def pool_run(L, l, gpu, x_nchw, setting, ldx, xoff, ldy, yoff):
    B, C, H, W = x_nchw.shape
    k, s, p, mode, cip = setting
    ref = S.pool_ref(x_nchw, setting)
    Ho, Wo = ref.shape[1:3]
    xb = S.strided_rows(x_nchw.permute(0, 2, 3, 1).reshape(B * H * W, C), ldx, xoff, TRAIL)[1].to(gpu)
    yb = S.nan_rows(B * Ho * Wo, C, ldy, yoff, TRAIL).to(gpu)
    L.check(l.bd_pool2d_nhwc(view(xb, B * H * W, C, ldx, xoff).data_ptr(), ldx, view(yb, B * Ho * Wo, C, ldy, yoff).data_ptr(), ldy, B, H, W, C, k, s, p,
                             mode, cip, L.stream()), "bd_pool2d_nhwc")
    out = result(yb, B * Ho * Wo, C, ldy, yoff)
    assert torch.equal(out, ref.reshape(-1, C)), (x_nchw.shape, setting, float((out - ref.reshape(-1, C)).abs().max()))
    return out


@pytest.mark.parametrize("negative", (False, True), ids=("mixed", "negative"))
@pytest.mark.parametrize("shape", S.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool2d_nhwc(gpu, lib, shape, negative):
    L, l = lib, lib.load()
    x = S.pool_data(shape, negative)
    C = shape[3]
    for setting in S.POOL_SETTINGS:
        out = pool_run(L, l, gpu, x, setting, C, LEAD, C, LEAD)
        if negative and setting[3] == 0:
            assert float(out.max()) < 0          # zero padding would show as a 0 at the border


def test_pool2d_nhwc_channel_slices(gpu, lib):
    L, l = lib, lib.load()
    ps = S.POOL_SLICE
    for negative in (False, True):
        x = S.pool_data(ps.shape, negative)
        for setting in S.POOL_SETTINGS:
            pool_run(L, l, gpu, x, setting, ps.ldx, ps.xoff, ps.ldy, ps.yoff)


@pytest.mark.parametrize("B,HW,C", S.GAP_SHAPES)
def test_global_avgpool_nhwc(gpu, lib, B, HW, C):
    L, l = lib, lib.load()
    x = S.gap_data(B, HW, C)
    ldx = C + S.GAP_LD_EXTRA
    xb = S.strided_rows(x.reshape(B * HW, C), ldx, LEAD, TRAIL)[1].to(gpu)
    yb = S.nan_rows(B, C, C, LEAD, TRAIL).to(gpu)
    L.check(l.bd_global_avgpool_nhwc(view(xb, B * HW, C, ldx).data_ptr(), ldx, yb[LEAD:].data_ptr(), B, HW, C, L.stream()), "bd_global_avgpool_nhwc")
    assert torch.equal(result(yb, B, C, C), S.gap_ref(x))
    assert l.bd_global_avgpool_nhwc(xb.data_ptr(), C - 1, yb.data_ptr(), B, HW, C, L.stream()) == INVALID


def resize_run(L, l, gpu, x, dst, scale, shift):
    B, H, W, C = x.shape
    n = B * dst[0] * dst[1] * C
    xd = x.to(gpu)
    yb = S.nan_rows(1, n, n, LEAD, TRAIL).to(gpu)
    L.check(l.bd_resize_bilinear_nhwc(xd.data_ptr(), int(x.dtype == torch.uint8), yb[LEAD:].data_ptr(), B, H, W, C, dst[0], dst[1], scale, shift,
                                      L.stream()), "bd_resize_bilinear_nhwc")
    return result(yb, 1, n, n)[0].view(B, dst[0], dst[1], C)


@pytest.mark.parametrize("src,dst", S.RESIZE_EXACT, ids=lambda s: "x".join(map(str, s)))
def test_resize_bilinear_exact(gpu, lib, src, dst):
    L, l = lib, lib.load()
    for C in S.RESIZE_C:
        for u8, scale, shift in ((False, 1.0, 0.0), (True, 2.0, -1.0)):
            x = S.resize_data(src, C, u8)
            ref = S.resize_ref(x, dst, scale, shift)
            out = resize_run(L, l, gpu, x, dst, scale, shift)
            assert torch.equal(out, ref.float()), (src, dst, C, u8, float((out - ref).abs().max()))


@pytest.mark.parametrize("src,dst", S.RESIZE_RANDOM, ids=lambda s: "x".join(map(str, s)))
def test_resize_bilinear_random_u8(gpu, lib, src, dst):
    L, l = lib, lib.load()
    x = torch.randint(0, 256, (S.RESIZE_B, *src, 3), generator=S.gen(src[0]), dtype=torch.uint8)
    # tolerance and reference of test_inception_pools_and_resize_vs_torch: ATen's fp32 CPU kernel, a few ulps of the [-1, 1] range.  (Not fp64:
    # the source coordinate scale * (dst + 0.5) - 0.5 is formed in fp32 by ATen and by the kernel alike, and at 400 -> 299 its rounding moves
    # a lerp weight by 2e-5.)
    ref = S.resize_ref(x, dst, 2.0, -1.0, torch.float32)
    out = resize_run(L, l, gpu, x, dst, 2.0, -1.0)
    assert float((out - ref).abs().max()) < 1e-5
