"""GPU: the grouped, weighted loss kernel bd_loss_groups_fwd_bwd (ops.loss_groups_fwd_bwd).

One group of weight 1 must reproduce bd_loss_fwd_bwd bit for bit (losses[0], losses[1], dpred).  With several groups dpred must EQUAL
the fp32 formula ((g' / (float)n_g) * grad_scale) * w_g restated here in numpy float32 (IEEE division, no reciprocal), rows of a
zero-weight group are 0, columns >= C of a padded dpred stay NaN and a second call gives the same bits.  Bound on the losses: each
losses[g] is one fp32 rounding (2^-24 relative) of an fp64 quotient whose own error (~n 2^-53) is negligible; the weighted total is
allowed one further ulp, so 2^-22 relative against an fp64 CPU sum of the same fp32 per-element losses covers both."""
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -22
WEIGHTS = (0.0, 1.0, 2.5, 0.125)
GRAD_SCALE = 1.0 / 3.0
LOSS_TYPES = ("l2", "l1", "huber")
# (rows, C, layout).  (100003, 3): more elements than one pass of 1024 x 256 threads, so the stride loop and a ragged tail run
CASES = [(1, 1, "dense"), (7, 3, "dense"), (1024, 3, "offset"), (1024, 3, "offset_strided"), (100003, 3, "dense")]
PAD = 2                                          # dpred rows are C + PAD floats wide


@pytest.fixture(scope="module")
def bd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from baddiffusion_amd import _lib as L
    import baddiffusion_amd.ops as ops
    return L, ops


@functools.lru_cache(maxsize=None)
def inputs(rows, C):
    """(pred, target) float32 numpy [rows, C]; differences on both sides of huber's |d| = 1, some exactly 0"""
    g = torch.Generator().manual_seed(rows * 31 + C)
    p = torch.randn(rows, C, generator=g)
    t = torch.randn(rows, C, generator=g)
    t[::5] = p[::5] if rows > 5 else t[::5]
    return p.numpy(), t.numpy()


def place(x, layout, ld_strided):
    """the [rows, C] values of x on the device as (view, ld): dense and 16-byte aligned | starting one float into a buffer (4-byte aligned
    only), rows C or ld_strided floats apart"""
    rows, C = x.shape
    xt = torch.from_numpy(x)
    if layout == "dense":
        v = xt.cuda()
        assert v.data_ptr() % 16 == 0
        return v, C
    ld = C if layout == "offset" else ld_strided
    buf = torch.full((rows * ld + 1,), float("nan"), device="cuda")
    v = buf[1:].view(rows, ld)[:, :C]
    v.copy_(xt)
    assert v.data_ptr() % 16 == 4 and v.stride(0) == ld
    return v, ld


def elem(loss_type, df):
    """per-element loss and derivative in float32 numpy, the formulas of loss_kernel"""
    one = np.float32(1.0)
    sign = np.where(df > 0, one, np.where(df < 0, -one, np.float32(0.0))).astype(np.float32)
    if loss_type == "l2":
        return df * df, np.float32(2.0) * df
    if loss_type == "l1":
        return np.abs(df), sign
    ad = np.abs(df)
    return (np.where(ad < one, np.float32(0.5) * df * df, ad - np.float32(0.5)).astype(np.float32),
            np.where(ad < one, df, np.where(df > 0, one, -one)).astype(np.float32))


def reference(loss_type, p, t, groups):
    """(fp64 per-group means + weighted total, float32 dpred by the formula of the header)"""
    rows, C = p.shape
    l, g = elem(loss_type, p - t)
    assert l.dtype == np.float32 and g.dtype == np.float32
    means, dp, r0 = [], np.empty_like(p), 0
    for r, w in groups:
        n = r * C
        means.append(l[r0:r0 + r].sum(dtype=np.float64) / n)
        dp[r0:r0 + r] = ((g[r0:r0 + r] / np.float32(n)) * np.float32(GRAD_SCALE)) * np.float32(w)
        r0 += r
    assert r0 == rows and dp.dtype == np.float32
    return means + [sum(float(np.float32(w)) * m for (_, w), m in zip(groups, means))], dp


def run_groups(L, pv, ldp, tv, ldt, rows, C, groups, loss_type):
    """bd_loss_groups_fwd_bwd into NaN-filled losses, a NaN-filled padded dpred and a NaN-filled workspace"""
    lib = L.load()
    d = L.LossGroupsDesc(n_groups=len(groups))
    for i, (r, w) in enumerate(groups):
        d.group_rows[i], d.group_weight[i] = r, w
    losses = torch.full((len(groups) + 1,), float("nan"), device="cuda")
    dp = torch.full((rows, C + PAD), float("nan"), device="cuda")
    nbytes = lib.bd_loss_groups_workspace_bytes(len(groups))
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device="cuda")
    import ctypes
    L.check(lib.bd_loss_groups_fwd_bwd(pv.data_ptr(), ldp, tv.data_ptr(), ldt, rows, C, {"l2": 0, "l1": 1, "huber": 2}[loss_type], GRAD_SCALE,
                                       ctypes.byref(d), losses.data_ptr(), dp.data_ptr(), C + PAD, ws.data_ptr(), nbytes, L.stream()),
            "bd_loss_groups_fwd_bwd")
    return losses, dp


def run_single(L, pv, ldp, tv, ldt, rows, C, loss_type):
    lib = L.load()
    loss = torch.full((), float("nan"), device="cuda")
    dp = torch.full((rows, C + PAD), float("nan"), device="cuda")
    ws = torch.full((lib.bd_reduce_workspace_bytes() // 8,), float("nan"), dtype=torch.float64, device="cuda")
    L.check(lib.bd_loss_fwd_bwd(pv.data_ptr(), ldp, tv.data_ptr(), ldt, rows, C, {"l2": 0, "l1": 1, "huber": 2}[loss_type], GRAD_SCALE,
                                loss.data_ptr(), dp.data_ptr(), C + PAD, ws.data_ptr(), L.stream()), "bd_loss_fwd_bwd")
    return loss, dp


def bits(x):
    return x.contiguous().view(torch.int32)


def splits(rows):
    """the group splits a batch of `rows` rows allows: (1, rows - 1), (rows - 1, 1), three groups with a one-row middle, four groups"""
    out = []
    if rows >= 2:
        out += [(1, rows - 1), (rows - 1, 1)]
    if rows >= 3:
        a = rows // 2
        out.append((a, 1, rows - 1 - a))
    if rows >= 4:
        q = rows // 4
        out.append((q, 1, q + 1, rows - 2 * q - 2))
    return out


@pytest.mark.parametrize("loss_type", LOSS_TYPES)
@pytest.mark.parametrize("rows,C,layout", CASES)
def test_one_group_of_weight_one_is_bitwise_the_ungrouped_loss(bd, rows, C, layout, loss_type):
    L = bd[0]
    p, t = inputs(rows, C)
    (pv, ldp), (tv, ldt) = place(p, layout, 8), place(t, layout, 5)
    loss, dp1 = run_single(L, pv, ldp, tv, ldt, rows, C, loss_type)
    losses, dpg = run_groups(L, pv, ldp, tv, ldt, rows, C, [(rows, 1.0)], loss_type)
    print(f"MEASURE loss_groups one group {(rows, C)} {layout} {loss_type} loss {float(loss):.9g} grouped {losses.tolist()}")
    assert not bool(torch.isnan(losses).any()) and not bool(torch.isnan(loss))
    assert torch.equal(bits(losses[0]), bits(loss)) and torch.equal(bits(losses[1]), bits(loss))
    assert not bool(torch.isnan(dp1[:, :C]).any())
    assert torch.equal(bits(dpg[:, :C]), bits(dp1[:, :C]))
    assert bool(torch.isnan(dpg[:, C:]).all())


@pytest.mark.parametrize("loss_type", LOSS_TYPES)
@pytest.mark.parametrize("rows,C,layout", [c for c in CASES if c[0] > 1])
def test_group_splits_and_weights(bd, rows, C, layout, loss_type):
    L = bd[0]
    p, t = inputs(rows, C)
    (pv, ldp), (tv, ldt) = place(p, layout, 8), place(t, layout, 5)
    rng = random.Random(rows * 7 + C + len(layout) + LOSS_TYPES.index(loss_type))
    zero_rows_checked = 0
    for split in splits(rows):
        # four groups take every weight once (in a drawn order); fewer groups draw theirs, and the first two splits always hold a zero
        weights = rng.sample(WEIGHTS, len(split))
        if len(split) == 2 and 0.0 not in weights:
            weights[rng.randrange(2)] = 0.0
        groups = list(zip(split, weights))
        ref_losses, ref_dp = reference(loss_type, p, t, groups)
        losses, dp = run_groups(L, pv, ldp, tv, ldt, rows, C, groups, loss_type)
        got = losses.cpu().double().tolist()
        rel = [abs(a - b) / b if b > 0 else abs(a) for a, b in zip(got, ref_losses)]
        print(f"MEASURE loss_groups {(rows, C)} {layout} {loss_type} groups {groups} worst rel {max(rel):.3e} bound {BOUND:.3e}")
        assert all(np.isfinite(got))
        assert max(rel) <= BOUND, (groups, got, ref_losses)
        assert bool(torch.isnan(dp[:, C:]).all())
        dpc = dp[:, :C].cpu().numpy()
        assert np.array_equal(dpc, ref_dp), (groups, int((dpc != ref_dp).sum()))
        r0 = 0
        for r, w in groups:
            if w == 0.0:
                assert bool((dp[r0:r0 + r, :C] == 0).all())
                zero_rows_checked += r
            r0 += r
        losses2, dp2 = run_groups(L, pv, ldp, tv, ldt, rows, C, groups, loss_type)
        assert torch.equal(bits(losses2), bits(losses)) and torch.equal(bits(dp2[:, :C]), bits(dp[:, :C]))
    assert zero_rows_checked > 0


def test_ops_wrapper(bd):
    """ops.loss_groups_fwd_bwd: rows of a [..., C] tensor, (row_count, weight) groups, contiguous dpred, want_grad=False"""
    L, ops = bd
    rows, C = 7, 3
    p, t = inputs(rows, C)
    groups = [(3, 0.125), (4, 2.5)]
    pv, tv = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    losses, dp = ops.loss_groups_fwd_bwd(pv.view(1, 7, 1, 3), tv.view(1, 7, 1, 3), groups, "huber", grad_scale=GRAD_SCALE)
    ref, _ = run_groups(L, pv, C, tv, C, rows, C, groups, "huber")
    _, ref_dp = reference("huber", p, t, groups)
    assert losses.shape == (3,) and torch.equal(bits(losses), bits(ref))
    assert dp.shape == (rows, C) and dp.is_contiguous() and np.array_equal(dp.cpu().numpy(), ref_dp)
    losses2, none = ops.loss_groups_fwd_bwd(pv, tv, groups, "huber", want_grad=False)
    assert none is None and torch.equal(bits(losses2), bits(losses))
    with pytest.raises(RuntimeError, match="bd_loss_groups_fwd_bwd"):
        ops.loss_groups_fwd_bwd(pv, tv, [(3, 1.0), (3, 1.0)])
    with pytest.raises(ValueError):
        ops.loss_groups_fwd_bwd(pv, tv, [(1, 1.0)] * 5 + [(2, 1.0)])
