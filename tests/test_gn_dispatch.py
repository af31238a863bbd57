"""Exact-value tests for every dispatch branch of the GroupNorm kernels (bd_gn_fwd / bd_gn_bwd / bd_gn_bwd_params: csrc/groupnorm.hip), in the
manner of tests/test_conv_ps_dispatch.py and tests/test_gemm_sp_dispatch.py.

The cases (tests/_gn_exact.py CASES; DESIGN.md "GroupNorm dispatch") hold one shape per branch of gn_resident_plan() and of the two-stage
kernels; tests/test_gn_exact_host.py pins the branch each takes (bd_gn_plan) and proves that the data makes every statistic, every sum of the
backward and -- where n = HW C / G is a power of two -- dx and dx_colsum numbers that fp32 arithmetic reproduces in any order.  So the
comparisons here are EQUALITY with a numpy fp64 reference (of values; the planes and the surroundings of strided windows bit for bit): an
element left out, counted twice, put in the wrong group or at the wrong address shows.

  * set F (eps 1e-6): mean == m; rstd == fp32(1 / sqrt(var + eps)) of the fp64 variance within RSTD_ULPS; y equal to
    fl(fl((x - m) rstd) gamma + beta) built from the rstd the kernel returned; planes bit-equal to bd_split_rows of that y.
  * set B (eps 0): mean, rstd, y = k gamma + beta, dgamma, dbeta, the [B][2][C] param_partials equal; dx and dx_colsum equal where n is a
    power of two, else within rounded_bound() (inv_n = fl(1 / n) is rounded there and hipcc may or may not contract the subtraction).
  * variants on every case: the three output forms of both directions, the channel window of dx_split, accumulate_dx / dx_add in the
    documented order fl(fl(term + dx) + dx_add), parameter gradients written / deferred / not wanted.
  * strided windows with NaN around the inputs and a fixed bit pattern around the outputs; SiLU against fp64 at the tolerances of
    test_groupnorm_fwd_bwd, per element; producer statistics with split counts 1, 8, 9, 37; 35 deferred layers in bd_gn_bwd_params.

Each test prints the figures it measured before it asserts (pytest -s).

Observed on MI355X: every case and variant passes; rstd is bit-equal to numpy's in every case (RSTD_ULPS = 0); under rounded_bound() the largest
deviation of dx is 0.855 (R2), 0.867 (R3), 0.974 (R5), 0.974 (R6), 0.989 (T2), 0.753 (T3), 0.742 (T4) of the bound and of dx_colsum 0.818, 0.842,
0.862, 0.789, 0.703, 0.853, 0.876; in the other nine cases n is a power of two and dx, dx_colsum are equal; no case found a fault in groupnorm.hip."""
import ctypes as CT

import numpy as np
import pytest
import torch

from tests import _gn_exact as X

pytestmark = pytest.mark.gpu

F32, F64 = X.F32, X.F64
RSTD_ULPS = 0               # fp32 ulps between the device's fp32(1 / sqrt(var + eps)) and numpy's (DESIGN.md "GroupNorm dispatch")
NAN_BITS = 0x7FC12345       # fp32 outputs are written into buffers pre-filled with this NaN
PLANE_BITS = 0x7FC1         # a bf16 NaN: a plane element nobody wrote
STRIDED = ("R2", "R5", "R7", "T2", "T3")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from baddiffusion_amd import _lib as L
    from baddiffusion_amd import ops
    return L, L.load(), ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def blank(*shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def blank_planes(rows, cols):
    return torch.full((rows, cols // 32, 2, 32), PLANE_BITS, dtype=torch.int16, device="cuda")


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def same(what, got, want):
    """value equality of every element (a NaN is a mismatch); on failure says how many differ and where"""
    want = want if torch.is_tensor(want) else dev(np.asarray(want).astype(F32))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if bool((got == want).all()):
        return
    g, w = got.cpu().numpy(), want.cpu().numpy()
    idx = np.argwhere(~(g == w))
    first, last = tuple(idx[0]), tuple(idx[-1])
    pytest.fail(f"{what}: {len(idx)} of {g.size} elements differ; first at {first}: got {g[first]!r}, want {w[first]!r}; last at {last}: got "
                f"{g[last]!r}, want {w[last]!r}; leading indices {np.unique(idx[:, 0])[:16].tolist()}, trailing {np.unique(idx[:, -1])[:16].tolist()}")


def same_bits(what, got, want):
    if not torch.equal(bits(got), bits(want)):
        same(what, got.float() if got.dtype != torch.float32 else got, want.float() if want.dtype != torch.float32 else want)
        pytest.fail(f"{what}: equal values, different bits")


def within(what, got, exact64, bound):
    err = np.abs(got.cpu().numpy().astype(F64) - exact64)
    bound = np.broadcast_to(bound, err.shape)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"  {what}: largest deviation from the fp64 value {float(err.max()):.3e}, at most {ratio:.3f} of the derived bound")
    idx = np.argwhere(~(err <= bound))
    assert len(idx) == 0, (what, len(idx), tuple(idx[0]), float(err[tuple(idx[0])]), float(bound[tuple(idx[0])]))


def gn_fwd(env, shp, x, ga, be, eps, silu, y=None, ys=None, ldys=0, stats=None, splits=0):
    L, lib, ops = env
    B, HW, C, G = shp
    st = blank(2, B, G)
    ws = ops.workspace(lib.bd_gn_workspace_bytes(B, C), x.device)
    d = L.GnFwdDesc(B=B, HW=HW, C=C, G=G, eps=eps, silu=silu, x=L.ptr(x), ldx=x.stride(1), gamma=L.ptr(ga), beta=L.ptr(be), y=L.ptr(y),
                    ldy=C if y is None else y.stride(1), mean=L.ptr(st[0]), rstd=L.ptr(st[1]), workspace=L.ptr(ws), workspace_bytes=ws.numel(),
                    y_split=L.ptr(ys), ldys=ldys or C, stats=L.ptr(stats), stats_splits=splits)
    L.check(lib.bd_gn_fwd(CT.byref(d), L.stream()), "bd_gn_fwd")
    return st[0], st[1]


def gn_bwd(env, shp, x, ga, be, mean, rstd, dy, silu, dx=None, acc=0, dg=None, db=None, cs=None, dxs=None, lddxs=0, add=None, pp=None, c0=0, c1=0):
    L, lib, ops = env
    B, HW, C, G = shp
    ws = ops.workspace(lib.bd_gn_workspace_bytes(B, C), x.device)
    d = L.GnBwdDesc(B=B, HW=HW, C=C, G=G, silu=silu, x=L.ptr(x), ldx=x.stride(1), gamma=L.ptr(ga), beta=L.ptr(be), mean=L.ptr(mean),
                    rstd=L.ptr(rstd), dy=L.ptr(dy), lddy=dy.stride(1), dx=L.ptr(dx), lddx=C if dx is None else dx.stride(1), accumulate_dx=acc,
                    dgamma=L.ptr(dg), dbeta=L.ptr(db), workspace=L.ptr(ws), workspace_bytes=ws.numel(), dx_colsum=L.ptr(cs), ld_colsum=C,
                    dx_split=L.ptr(dxs), lddxs=lddxs or C, dx_add=L.ptr(add), ld_add=C if add is None else add.stride(1), param_partials=L.ptr(pp),
                    dx_split_c0=c0, dx_split_c1=c1)
    L.check(lib.bd_gn_bwd(CT.byref(d), L.stream()), "bd_gn_bwd")


def fold_params(env, items, B):
    """items: [(partials [B][2][C] tensor, C, dgamma, dbeta)] -> one bd_gn_bwd_params call"""
    L, lib, _ = env
    arr = (L.GnParamItem * len(items))()
    for i, (p, C, dg, db) in enumerate(items):
        arr[i].partials = L.ptr(p); arr[i].C = C; arr[i].dgamma = L.ptr(dg); arr[i].dbeta = L.ptr(db)
    L.check(lib.bd_gn_bwd_params(arr, len(items), B, L.stream()), "bd_gn_bwd_params")


def sixty_fourths(cid, salt, *shape):
    """multiples of 2^-6 in [-2, 2]"""
    return (X._rng(cid, salt).integers(-128, 129, size=shape) / 64.0).astype(F32)


def check_rstd(what, rstd, var64, eps):
    want = (1.0 / np.sqrt(var64 + F64(F32(eps)))).astype(F32)
    ulps = np.abs(rstd.cpu().numpy().view(np.int32).astype(np.int64) - want.view(np.int32))
    print(f"  {what}: rstd at most {int(ulps.max())} fp32 ulp from numpy's fp32(1 / sqrt(var + eps)), {int((ulps > 0).sum())} of {ulps.size} differ")
    assert ulps.max() <= RSTD_ULPS, (what, int(ulps.max()), np.argwhere(ulps > RSTD_ULPS)[:4].tolist())


def y_from(x, mean64, rstd, ga, be):
    """fl(fl((x - mean) rstd) gamma + beta) with the fp32 rstd the kernel returned: the product of two fp32 numbers and gamma's power of two are
    exact in fp64, so each .astype(F32) is the one rounding of the fp32 (or fused) operation"""
    C = x.shape[2]
    t = ((x.astype(F64) - X.per_channel(mean64, C)[:, None, :]) * X.per_channel(rstd.cpu().numpy().astype(F64), C)[:, None, :]).astype(F32)
    return (t.astype(F64) * ga.astype(F64) + be.astype(F64)).astype(F32)


# ------------------------------------------------------------------------------------------------ forward, set F
@pytest.mark.parametrize("cid", list(X.CASES))
def test_forward_exact(env, cid):
    ops = env[2]
    shp = B, HW, C, G = X.shape(cid)
    x, m = X.set_f(cid)
    ga, be = X.params(cid)
    ref = X.reference(x, None, ga, be, G, X.EPS_F, 0)
    xd, gd, bd = dev(x), dev(ga), dev(be)
    forms = ["y"] + (["y+planes", "planes"] if C % 32 == 0 else [])
    y_want = None
    for form in forms:
        y = blank(B + 1, HW, C) if "y" in form else None                          # a guard sample behind the last one
        ys = blank_planes((B + 1) * HW, C) if "planes" in form else None
        mean, rstd = gn_fwd(env, shp, xd, gd, bd, X.EPS_F, 0, y=y, ys=ys)
        same(f"{cid} {form}: mean", mean, m)
        check_rstd(f"{cid} {form}", rstd, ref["var"], X.EPS_F)
        if y_want is None:
            y_want = dev(y_from(x, m, rstd, ga, be))
            rstd0 = rstd
        same_bits(f"{cid} {form}: rstd against the first form", rstd, rstd0)
        if y is not None:
            same(f"{cid} {form}: y", y[:B], y_want)
            assert bool((bits(y[B]) == NAN_BITS).all()), f"{cid} {form}: rows behind y written"
        if ys is not None:
            same_bits(f"{cid} {form}: planes", ys[:B * HW], ops.split_rows(y_want))
            assert bool((ys[B * HW:] == PLANE_BITS).all()), f"{cid} {form}: rows behind the planes written"


# ------------------------------------------------------------------------------------------------ backward, set B
def _set_b_on_device(cid):
    x, dy, k, m, s = X.set_b(cid)
    ga, be = X.params(cid)
    ref = X.reference(x, dy, ga, be, X.shape(cid)[3], 0.0, 0)
    return dev(x), dev(dy), dev(ga), dev(be), ga, ref, m, s


@pytest.mark.parametrize("cid", list(X.CASES))
def test_backward_exact(env, cid):
    ops = env[2]
    shp = B, HW, C, G = X.shape(cid)
    n, pow2 = X.group_size(cid), X.is_pow2(X.group_size(cid))
    xd, dyd, gd, bd, ga, ref, m, s = _set_b_on_device(cid)
    y = blank(B, HW, C)
    mean, rstd = gn_fwd(env, shp, xd, gd, bd, 0.0, 0, y=y)
    same(f"{cid}: mean", mean, m); same(f"{cid}: rstd", rstd, 1.0 / s); same(f"{cid}: y", y, ref["y"])
    rc = X.per_channel(1.0 / s, C)

    # plain launch: dx, dx_colsum, parameter gradients written directly
    term, dg, db, cs = blank(B + 1, HW, C), blank(C), blank(C), blank(B, C)
    gn_bwd(env, shp, xd, gd, bd, mean, rstd, dyd, 0, dx=term, dg=dg, db=db, cs=cs)
    same(f"{cid}: dgamma", dg, ref["dgamma"]); same(f"{cid}: dbeta", db, ref["dbeta"])
    assert bool((bits(term[B]) == NAN_BITS).all()), f"{cid}: rows behind dx written"
    term = term[:B]
    if pow2:
        same(f"{cid}: dx", term, ref["dx"]); same(f"{cid}: dx_colsum", cs, ref["colsum"])
    else:
        within(f"{cid}: dx", term, ref["dx"], X.rounded_bound(ref["t"], ref["w"], rc[:, None, :], n))
        within(f"{cid}: dx_colsum", cs, ref["colsum"], X.rounded_bound(ref["T"], ref["wc"], rc, n))

    # parameter gradients deferred (param_partials + bd_gn_bwd_params), and not wanted
    dx2, pp, dg2, db2 = blank(B, HW, C), blank(B, 2, C), blank(C), blank(C)
    gn_bwd(env, shp, xd, gd, bd, mean, rstd, dyd, 0, dx=dx2, dg=dg2, db=db2, pp=pp)
    same_bits(f"{cid} deferred: dx", dx2, term); same(f"{cid} deferred: param_partials", pp, ref["partials"])
    assert bool((bits(dg2) == NAN_BITS).all() and (bits(db2) == NAN_BITS).all()), f"{cid} deferred: dgamma / dbeta written"
    fold_params(env, [(pp, C, dg2, db2)], B)
    same(f"{cid} deferred: dgamma", dg2, ref["dgamma"]); same(f"{cid} deferred: dbeta", db2, ref["dbeta"])
    dx3, dg3, db3 = blank(B, HW, C), blank(C), blank(C)
    gn_bwd(env, shp, xd, gd, bd, mean, rstd, dyd, 0, dx=dx3)
    same_bits(f"{cid} no parameter gradients: dx", dx3, term)
    assert bool((bits(dg3) == NAN_BITS).all() and (bits(db3) == NAN_BITS).all())

    # accumulate_dx / dx_add: fl(fl(term + existing) + add); the planes of that launch hold the FINAL value
    have, add = sixty_fourths(cid, 11, B, HW, C), sixty_fourths(cid, 12, B, HW, C)
    t32 = term.cpu().numpy()
    for acc, with_add in ((1, False), (0, True), (1, True)):
        want = t32 + have if acc else t32
        want = dev(want + add if with_add else want)
        dx4 = dev(have) if acc else blank(B, HW, C)
        dxs = blank_planes(B * HW, C) if C % 32 == 0 else None
        gn_bwd(env, shp, xd, gd, bd, mean, rstd, dyd, 0, dx=dx4, acc=acc, add=dev(add) if with_add else None, dg=dg3, db=db3, dxs=dxs)
        same(f"{cid} accumulate {acc} add {with_add}: dx", dx4, want)
        if dxs is not None:
            same_bits(f"{cid} accumulate {acc} add {with_add}: planes", dxs, ops.split_rows(want))
    same(f"{cid} accumulate: dgamma", dg3, ref["dgamma"])
    if C % 32:
        return

    # planes: with dx, alone, and the channel window [32, C - 32) at columns c - 32 of a wider plane buffer
    want = ops.split_rows(term.contiguous())
    for with_dx in (True, False):
        dx5, dxs = (blank(B, HW, C) if with_dx else None), blank_planes((B + 1) * HW, C)
        gn_bwd(env, shp, xd, gd, bd, mean, rstd, dyd, 0, dx=dx5, dxs=dxs)
        same_bits(f"{cid} planes (dx {with_dx})", dxs[:B * HW], want)
        assert bool((dxs[B * HW:] == PLANE_BITS).all()), f"{cid}: rows behind the planes written"
        if with_dx:
            same_bits(f"{cid} dx next to planes", dx5, term)
    if C >= 96:
        w = C - 64
        for with_dx in (True, False):
            dx6, dxs = (blank(B, HW, C) if with_dx else None), blank_planes((B + 1) * HW, w + 32)
            gn_bwd(env, shp, xd, gd, bd, mean, rstd, dyd, 0, dx=dx6, dxs=dxs, lddxs=w + 32, c0=32, c1=C - 32)
            same_bits(f"{cid} window planes (dx {with_dx})", dxs[:B * HW, :w // 32], ops.split_rows(term[:, :, 32:C - 32].contiguous()))
            assert bool((dxs[:, w // 32:] == PLANE_BITS).all() and (dxs[B * HW:] == PLANE_BITS).all()), f"{cid} window: plane buffer written outside the window"
            if with_dx:
                same_bits(f"{cid} dx next to window planes", dx6, term)


# ------------------------------------------------------------------------------------------------ strided windows
def window(B, HW, C, ld, fill):
    """[B + 2, HW, ld] buffer (a guard sample in front and behind) and its [B, HW, C] column block at offset 32"""
    if fill is None:
        buf = blank(B + 2, HW, ld)
    else:
        buf = torch.full((B + 2, HW, ld), float("nan"), device="cuda")
        buf[1:B + 1, :, 32:32 + C] = fill
    return buf, buf[1:B + 1, :, 32:32 + C]


def untouched(what, buf, B, C):
    ok = bits(buf) == NAN_BITS
    ok[1:B + 1, :, 32:32 + C] = True
    assert bool(ok.all()), f"{what}: bytes outside the window changed"


@pytest.mark.parametrize("cid", STRIDED)
def test_strided_windows(env, cid):
    shp = B, HW, C, G = X.shape(cid)
    xd, dyd, gd, bd, ga, ref, m, s = _set_b_on_device(cid)
    mean, rstd = gn_fwd(env, shp, xd, gd, bd, 0.0, 0, y=blank(B, HW, C))
    term, cs0 = blank(B, HW, C), blank(B, C)
    gn_bwd(env, shp, xd, gd, bd, mean, rstd, dyd, 0, dx=term, cs=cs0)                    # contiguous: what test_backward_exact holds to the reference
    _, xw = window(B, HW, C, C + 32, xd)
    _, dyw = window(B, HW, C, C + 64, dyd)
    ybuf, yw = window(B, HW, C, C + 64, None)
    mean2, rstd2 = gn_fwd(env, shp, xw, gd, bd, 0.0, 0, y=yw)
    same(f"{cid}: mean", mean2, m); same(f"{cid}: rstd", rstd2, 1.0 / s); same(f"{cid}: y", yw, ref["y"])
    untouched(f"{cid}: y", ybuf, B, C)
    dbuf, dxw = window(B, HW, C, C + 32, None)
    dg, db, cs = blank(C), blank(C), blank(B, C)
    gn_bwd(env, shp, xw, gd, bd, mean, rstd, dyw, 0, dx=dxw, dg=dg, db=db, cs=cs)
    same_bits(f"{cid}: dx", dxw, term); same_bits(f"{cid}: dx_colsum", cs, cs0)
    same(f"{cid}: dgamma", dg, ref["dgamma"]); same(f"{cid}: dbeta", db, ref["dbeta"])
    untouched(f"{cid}: dx", dbuf, B, C)
    have, add = sixty_fourths(cid, 11, B, HW, C), sixty_fourths(cid, 12, B, HW, C)
    _, addw = window(B, HW, C, C + 64, dev(add))
    dxw[:] = dev(have)
    gn_bwd(env, shp, xw, gd, bd, mean, rstd, dyw, 0, dx=dxw, acc=1, add=addw)
    same(f"{cid}: accumulated dx", dxw, (term.cpu().numpy() + have) + add)
    untouched(f"{cid}: accumulated dx", dbuf, B, C)


# ------------------------------------------------------------------------------------------------ SiLU, both sets, per element
@pytest.mark.parametrize("cid", list(X.CASES))
def test_silu_against_fp64(env, cid):
    shp = B, HW, C, G = X.shape(cid)
    ga, be = X.params(cid)
    dy = X.set_b(cid)[1]
    gd, bd, dyd = dev(ga), dev(be), dev(dy)
    for name, x, eps in (("F", X.set_f(cid)[0], X.EPS_F), ("B", X.set_b(cid)[0], 0.0)):
        ref = X.reference(x, dy, ga, be, G, eps, 1)
        xd, y, dx, dg, db, cs = dev(x), blank(B, HW, C), blank(B, HW, C), blank(C), blank(C), blank(B, C)
        mean, rstd = gn_fwd(env, shp, xd, gd, bd, eps, 1, y=y)
        gn_bwd(env, shp, xd, gd, bd, mean, rstd, dyd, 1, dx=dx, dg=dg, db=db, cs=cs)
        h = lambda t: t.cpu().numpy().astype(F64)
        for what, got, want in (("dgamma", h(dg), ref["dgamma"]), ("dbeta", h(db), ref["dbeta"])):
            print(f"  {cid} set {name} {what}: {np.abs(got - want).max() / np.abs(want).max():.2e} of the maximum")
        print(f"  {cid} set {name}: max |y - ref| {np.abs(h(y) - ref['y']).max():.2e}, max |dx - ref| {np.abs(h(dx) - ref['dx']).max():.2e}")
        np.testing.assert_allclose(h(mean), ref["mean"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(h(rstd), ref["rstd"], rtol=1e-6)
        np.testing.assert_allclose(h(y), ref["y"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(h(dx), ref["dx"], rtol=1e-3, atol=2e-5)
        np.testing.assert_allclose(h(cs), ref["colsum"], rtol=1e-3, atol=1e-5 * HW ** 0.5 * max(1.0, np.abs(ref["dx"]).max()))
        assert np.abs(h(dg) - ref["dgamma"]).max() <= 1e-3 * np.abs(ref["dgamma"]).max()
        assert np.abs(h(db) - ref["dbeta"]).max() <= 1e-3 * np.abs(ref["dbeta"]).max()


# ------------------------------------------------------------------------------------------------ producer statistics
@pytest.mark.parametrize("splits", [1, 8, 9, 37])
@pytest.mark.parametrize("cid", ["T1", "T3"])
def test_forward_follows_producer_statistics(env, cid, splits):
    """stats / stats_splits: integer fp64 partials that describe ANOTHER mean and variance than x has -- the statistics pass over x must be
    skipped, and all eight interleaved phases of gn_fwd_finalize_kernel and their remainder summed."""
    L, lib, _ = env
    shp = B, HW, C, G = X.shape(cid)
    assert lib.bd_gn_fwd_takes_stats(B, HW, C, G) == 1
    n = X.group_size(cid)
    x, m = X.set_f(cid)
    ga, be = X.params(cid)
    b, g = np.arange(B)[:, None], np.arange(G)[None, :]
    m2 = m + 1 + (b + g) % 2                                        # never the mean of x
    var = (3 + (2 * b + g) % 5).astype(F64)                         # x has a variance of several hundred
    r = X._rng(cid, 20 + splits)
    part = r.integers(-2 ** 20, 2 ** 20, size=(B, splits, G, 2)).astype(F64)
    part[:, -1] += np.stack([m2 * n, (var + m2 * m2) * n], axis=-1) - part.sum(1)
    assert np.array_equal(part.sum(1)[..., 0], m2 * n) and np.abs(part).max() < 2 ** 40
    y = blank(B, HW, C)
    mean, rstd = gn_fwd(env, shp, dev(x), dev(ga), dev(be), X.EPS_F, 0, y=y, stats=dev(part), splits=splits)
    same(f"{cid} {splits} splits: mean", mean, m2)
    check_rstd(f"{cid} {splits} splits", rstd, var, X.EPS_F)
    same(f"{cid} {splits} splits: y", y, y_from(x, m2, rstd, ga, be))


# ------------------------------------------------------------------------------------------------ more than GN_PARAM_MAX deferred layers
def test_params_of_35_deferred_layers(env):
    """bd_gn_bwd_params launches once per 32 items: items 33 - 35 go through the second launch with a table of their own"""
    B = 37                                                          # 16 row phases: two full trips and a tail of five
    r = np.random.default_rng(35)
    layers = [(24, 128, 384)[i % 3] for i in range(35)]
    parts = [r.integers(-64, 65, size=(B, 2, C)).astype(F32) for C in layers]
    items = [(dev(p), C, blank(C), blank(C)) for p, C in zip(parts, layers)]
    fold_params(env, items, B)
    for i, (p, (_, C, dg, db)) in enumerate(zip(parts, items)):
        same(f"item {i + 1} (C {C}): dgamma", dg, p[:, 0].astype(F64).sum(0)); same(f"item {i + 1} (C {C}): dbeta", db, p[:, 1].astype(F64).sum(0))
