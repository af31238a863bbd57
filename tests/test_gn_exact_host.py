"""CPU: the plan table and the exactness precondition of the GroupNorm dispatch tests (tests/test_gn_dispatch.py).

test_plan_table asserts what bd_gn_plan -- the host-only query built from the functions bd_gn_fwd / bd_gn_bwd call to choose their kernels --
reports for every case, forward and backward: whoever retunes gn_resident_plan() moves the cases with it (DESIGN.md "GroupNorm dispatch").

The other tests prove, per case, that the data of tests/_gn_exact.py is rounding-free where the GPU test demands equality: the kernels'
formulas are evaluated in numpy float32 with the pixels summed in two different orders (sequentially forwards; pairwise over the reversed
column) and in float64, and the three agree bit for bit after rounding to fp32; every sum's absolute terms add up to less than 2^24 units of
their grid, so NO order of summation rounds, and every product / difference the equality covers is below 2^24 units of its last bit."""
import ctypes

import numpy as np
import pytest

from tests import _gn_exact as X

F32, F64 = X.F32, X.F64
LIMIT = 2.0 ** 24


def test_plan_table():
    from baddiffusion_amd import _lib as L
    lib = L.load()
    assert set(X.PLAN) == set(X.CASES)
    for cid, (B, HW, C, G, *_) in X.CASES.items():
        for backward in (0, 1):
            p = L.GnPlanInfo()
            assert lib.bd_gn_plan(B, HW, C, G, backward, ctypes.byref(p)) == 0, lib.bd_last_error()
            got = ("res", p.nt, p.cb, p.q, p.R, p.E, p.emax) if p.resident else ("two", p.S, p.threads, p.r, p.per)
            unused = (p.S, p.threads, p.r, p.per) if p.resident else (p.nt, p.cb, p.q, p.R, p.E, p.emax)
            assert got == X.PLAN[cid][backward] and unused == (0,) * len(unused), (cid, backward, got, unused)
            assert lib.bd_gn_fwd_takes_stats(B, HW, C, G) == (0 if X.PLAN[cid][0][0] == "res" else 1)
    p = L.GnPlanInfo()
    assert lib.bd_gn_plan(2, 64, 130, 32, 0, ctypes.byref(p)) < 0 and b"bd_gn_plan" in lib.bd_last_error()     # C % G != 0
    assert lib.bd_gn_plan(2, 64, 128, 32, 0, None) < 0


def test_case_table_is_what_the_cases_are_there_for():
    """the properties the table claims, from the plan: idle threads, masked row slots, ragged tails, empty splits"""
    res = lambda cid, bw: dict(zip(("nt", "cb", "q", "R", "E", "emax"), X.PLAN[cid][bw][1:]))
    two = lambda cid: dict(zip(("S", "threads", "r", "per"), X.PLAN[cid][0][1:]))
    wred = lambda q: q < 64 and q & (q - 1) == 0
    for cid, (B, HW, C, G, *_) in X.CASES.items():
        assert X.group_size(cid) % 16 == 0
        for bw in (0, 1):
            if X.PLAN[cid][bw][0] == "res":
                p = res(cid, bw)
                assert p["q"] * 4 == p["cb"] and p["R"] == p["nt"] // p["q"] and p["E"] == -(-HW // p["R"]) and p["E"] <= p["emax"] <= 16
    assert wred(res("R1", 0)["q"]) and not wred(res("R2", 0)["q"]) and not wred(res("R3", 0)["q"]) and not wred(res("R8", 0)["q"])
    p = res("R2", 0); assert p["nt"] - p["q"] * p["R"] == 4 and p["R"] * p["E"] == 294
    p = res("R5", 1); assert p["R"] * p["E"] == 1024 > 900
    p = res("R8", 1); assert 64 - p["R"] == 56
    p = res("R9", 0); assert p["R"] == 4 * 16
    p = res("R10", 0); assert p["nt"] - p["q"] * p["R"] == 2 and not wred(p["q"])
    assert (515 * (128 // res("R7", 0)["cb"])) % 8 and (513 * (256 // res("R8", 0)["cb"])) % 8
    assert -(-4096 // two("T1")["S"]) == 32 == 2 * two("T1")["r"]                # 32 rows per split, trips of 4 r = 64
    per = -(-4100 // two("T2")["S"]); assert per == 33 and 125 * per > 4100 and 4100 - 124 * per == 8
    per = -(-1024 // two("T4")["S"]); assert per == 86 and 1024 - 11 * per == 78
    assert 3 * (256 // 2) == 384 > 256
    assert two("T6")["r"] == 1 and 4096 // two("T6")["per"] == 256


def _two_orders(a):
    """sum over axis 1 of an fp32 array [B, HW, C]: sequentially forwards, and pairwise over the reversed column"""
    fw = np.cumsum(a, axis=1, dtype=F32)[:, -1]
    rv = np.sum(a[:, ::-1], axis=1, dtype=F32)
    return fw, rv


def _same(what, cid, exact64, *evaluations):
    want = exact64.astype(F32)
    assert np.array_equal(want.astype(F64), exact64), (cid, what, "the fp64 value is not an fp32 number")
    for i, v in enumerate(evaluations):
        assert v.dtype == F32 and np.array_equal(v.view(np.uint32), want.view(np.uint32)), (cid, what, f"evaluation {i}")


def _on_grid(what, cid, v, unit):
    """|v| / unit is an integer below 2^24: v is an fp32 number, and so is every number on this grid that is no larger"""
    u = np.abs(np.asarray(v, dtype=F64)) / unit
    assert np.array_equal(u, np.rint(u)) and u.max() < LIMIT, (cid, what, float(u.max()))


@pytest.mark.parametrize("cid", list(X.CASES))
def test_set_f_statistics_are_exact(cid):
    B, HW, C, G = X.shape(cid)
    x, m = X.set_f(cid)
    n = X.group_size(cid)
    assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 64 and len(np.unique(x)) > 64
    assert (m[:, 1:] != m[:, :-1]).all() and (B == 1 or (m[1:] != m[:-1]).all())
    x64 = x.astype(F64)
    _same("sum x", cid, x64.sum(1), *_two_orders(x))
    _same("sum x^2", cid, (x64 * x64).sum(1), *_two_orders(x * x))
    _on_grid("sum |x|", cid, np.abs(x64).sum(1), 1.0)
    _on_grid("sum x^2", cid, (x64 * x64).sum(1), 1.0)
    ref = X.reference(x, None, *X.params(cid), G, X.EPS_F, 0)
    assert np.array_equal(ref["mean"], m) and (ref["var"] > 1.0).all()
    assert np.array_equal(x64.reshape(B, HW, G, C // G).sum((1, 3)), m * n)


@pytest.mark.parametrize("cid", list(X.CASES))
def test_set_b_backward_is_exact(cid):
    B, HW, C, G = X.shape(cid)
    n = X.group_size(cid)
    x, dy, k, m, s = X.set_b(cid)
    gamma, beta = X.params(cid)
    assert set(np.unique(np.abs(gamma))) <= {0.5, 1.0, 2.0} and np.array_equal(beta * 4, np.rint(beta * 4)) and len(np.unique(beta)) > 4
    kg = k.reshape(B, HW, G, C // G).astype(F64)
    assert (kg.sum((1, 3)) == 0).all() and ((kg * kg).sum((1, 3)) == n).all()
    ref = X.reference(x, dy, gamma, beta, G, 0.0, 0)
    assert np.array_equal(ref["mean"], m) and np.array_equal(ref["rstd"], 1.0 / s) and np.array_equal(ref["xh"], k)
    assert np.array_equal(ref["y"], k * gamma.astype(F64) + beta)
    # the kernels' formulas in fp32
    mc, rc = X.per_channel(m, C).astype(F32)[:, None, :], X.per_channel(1.0 / s, C).astype(F32)[:, None, :]
    xh = (x - mc) * rc
    assert xh.dtype == F32 and np.array_equal(xh, k)
    _same("y", cid, ref["y"], xh * gamma + beta)
    sa = _two_orders(dy); e = _two_orders(dy * xh); sh = _two_orders(xh)
    _same("sum dz", cid, ref["sa"], *sa); _same("sum dz xhat", cid, ref["e"], *e); _same("sum xhat", cid, ref["sh"], *sh)
    _on_grid("sum |dz|", cid, np.abs(ref["dz"]).sum(1), 1.0)
    _on_grid("sum |dz xhat|", cid, np.abs(ref["dz"] * ref["xh"]).sum(1), 1.0)
    _on_grid("sum |xhat|", cid, np.abs(ref["xh"]).sum(1), 1.0)
    grp = lambda v: (v * gamma).reshape(B, G, C // G)
    for name, v, key in (("s1", sa[0], "s1"), ("s2", e[0], "s2")):
        g = grp(v)
        _same(name, cid, ref[key], np.cumsum(g, axis=-1, dtype=F32)[..., -1], np.sum(g[..., ::-1], axis=-1, dtype=F32))
        _on_grid("sum |gamma *| of " + name, cid, np.abs(g.astype(F64)).sum(-1), 0.5)
    s1c, s2c = X.per_channel(ref["s1"], C).astype(F32), X.per_channel(ref["s2"], C).astype(F32)
    T = F32(HW) * s1c + s2c * sh[0]
    _same("HW s1 + s2 sum xhat", cid, ref["T"], T, F32(HW) * s1c + s2c * sh[1])
    _on_grid("|HW s1| + |s2 sum xhat|", cid, np.abs(HW * s1c.astype(F64)) + np.abs(s2c.astype(F64) * ref["sh"]), 0.5)
    for name, v, key in (("dgamma", e[0], "dgamma"), ("dbeta", sa[0], "dbeta")):
        _same(name, cid, ref[key], np.cumsum(v, axis=0, dtype=F32)[-1], np.sum(v[::-1], axis=0, dtype=F32))
        _on_grid("sum over samples of |" + name + "|", cid, np.abs(v.astype(F64)).sum(0), 1.0)
    _on_grid("t = s1 + xhat s2", cid, np.abs(s1c.astype(F64))[:, None, :] + 2 * np.abs(s2c.astype(F64))[:, None, :], 0.5)
    if not X.is_pow2(n):        # inv_n is rounded: dx and dx_colsum are held to X.rounded_bound on the device, every sum above stays exact
        return
    inv_n = F32(1.0) / F32(n)
    assert F64(inv_n) * n == 1.0
    t = s1c[:, None, :] + xh * s2c[:, None, :]
    w = dy * gamma - t * inv_n
    _same("dx", cid, ref["dx"], rc * w)
    _on_grid("|dz gamma| + |t / n|", cid, np.abs(ref["dz"] * gamma) + np.abs(ref["t"]) / n, 0.5 / n)
    _same("dx_colsum", cid, ref["colsum"], rc[:, 0, :] * (gamma * sa[0] - T * inv_n))
    _on_grid("|gamma sum dz| + |T / n|", cid, np.abs(ref["sa"] * gamma) + np.abs(ref["T"]) / n, 0.5 / n)
