"""CPU: what bd_conv3x3_fwd_plan / _dgrad_plan / _wgrad_plan -- the host-only queries built from the plan the launchers of csrc/conv_thin.hip
themselves read -- report for every case of the thin-convolution table (tests/_thin_exact.py; DESIGN.md "Dispatch branches of the thin
convolutions"), which descriptors fall to igemm, the workspace contract of the thin weight gradients, and the proof that the table's operands
keep every sum of tests/test_thin_dispatch.py exact.  Nothing is launched: the addresses are fakes with the alignment of the real windows.
BD_THIN_DIRECT and BD_THIN_MFMA are read once per process by the library, so nothing here toggles them; the table is for a process that
sets neither."""
import ctypes
import os
import re

import pytest
import torch

from tests import _thin_exact as X
from tests.test_conv_ps_dispatch import _mag, rnd

BASE = {n: 0x40000000 * (i + 1) for i, n in enumerate(("x", "y", "dy", "dx", "w", "bias", "dw", "db", "ws", "extra"))}   # never dereferenced
BD_ERR_WORKSPACE = -4
MFMA_LO_SHARE = 0.4         # of the wide operand's elements have a nonzero bf16 lo part wherever a matrix-pipe path runs


@pytest.fixture(scope="module")
def lib():
    assert "BD_THIN_DIRECT" not in os.environ and "BD_THIN_MFMA" not in os.environ, "the table is for the default dispatch"
    from baddiffusion_amd.build import build_lib
    build_lib(force=False, verbose=False)
    from baddiffusion_amd import _lib as L
    return L, L.load()


def plan_of(lib, c, d):
    """the query of c's direction on d -> (status, {field: value}); a weight gradient gets the workspace every caller allocates unless d has one"""
    L, l = lib
    if c.kind == "wgrad" and not d.workspace_bytes:
        d.workspace_bytes = l.bd_conv3x3_workspace_bytes(c.B, c.H, c.W, c.H, c.W, c.Cin, c.Cout, 0)
    p = L.ThinPlanInfo()
    status = getattr(l, f"bd_conv3x3_{c.kind}_plan")(ctypes.byref(d), ctypes.byref(p))
    return status, {f: getattr(p, f) for f in X.PLAN_FIELDS}


def rows():
    for c in X.CASES.values():
        for layout in c.layouts:
            for mode in c.modes:
                yield c, layout, mode


@pytest.mark.parametrize("name", list(X.CASES))
def test_plan_reports_what_the_table_states(lib, name):
    """path, J, loop count, pix_per_block, grid, partial rows, workspace bytes and profiler class in the three layouts and every mode of the case;
    a missing bias or db changes nothing"""
    c = X.CASES[name]
    for layout in c.layouts:
        g = X.geometry(c, layout)
        for mode in c.modes:
            want = X.expected_plan(c, layout, mode)
            for opt in (True, False):
                status, got = plan_of(lib, c, X.make_desc(lib[0], c, g, BASE, mode, bias=opt, db=opt))
                assert status == 0, (name, layout, mode, lib[1].bd_last_error())
                assert got == want, (name, layout, mode, opt, got, want)


def test_table_reaches_every_path(lib):
    """the nine thin paths and igemm are each named by a case, the loop of every looping path runs more than once somewhere, both J, and
    pix_per_block above 128: a retune that makes one of them unreachable from the table fails here"""
    seen, loops, js, ppb = set(), {}, set(), set()
    for c, layout, mode in rows():
        got = plan_of(lib, c, X.make_desc(lib[0], c, X.geometry(c, layout), BASE, mode))[1]
        seen.add(got["path"]); js.add(got["J"]); ppb.add(got["pix_per_block"])
        loops[got["path"]] = max(loops.get(got["path"], 0), got["loops"])
    assert seen == set(range(9)), seen
    assert all(loops[p] > 1 for p in (X.EXPAND_FMA, X.EXPAND_MFMA, X.CONTRACT_DGRAD, X.WGRAD_MFMA, X.WGRAD_ROW)), loops
    assert {1, 3} <= js and max(ppb) > 128, (js, ppb)
    print("MEASURE coverage", sorted(X.PATH_NAME[p] for p in seen), loops)


def test_every_path_and_instantiation_is_named():
    """the table names all nine thin paths and igemm, with J = 3 and J = 1 where a kernel is a template over J and both layers where it is one over the
    direction: conv_thin.hip has no instantiation that tests/test_thin_dispatch.py, which launches every row, does not launch"""
    seen = set()
    for c in X.CASES.values():
        for layout in c.layouts:
            for mode in c.modes:
                p = X.expected_plan(c, layout, mode)
                seen.add((p["path"], p["J"], c.direction if p["path"] in (X.WGRAD_MFMA, X.WGRAD_ROW) else ""))
    want = {(X.IGEMM, 0, ""), (X.EXPAND_FMA, 3, ""), (X.EXPAND_FMA, 1, ""), (X.EXPAND_MFMA, 3, ""), (X.CONTRACT, 3, ""), (X.CONTRACT, 1, ""),
            (X.CONTRACT_DGRAD, 3, ""), (X.CONTRACT_DGRAD, 1, ""), (X.WGRAD_MFMA, 3, "wgrad_in"), (X.WGRAD_MFMA, 3, "wgrad_out"),
            (X.WGRAD_ROW, 3, "wgrad_in"), (X.WGRAD_ROW, 3, "wgrad_out"), (X.WGRAD_CIN, 3, ""), (X.WGRAD_CIN, 1, ""), (X.WGRAD_COUT, 3, ""),
            (X.WGRAD_COUT, 1, "")}
    assert seen == want, seen ^ want


# ------------------------------------------------------------------------------------------------ what falls to igemm
def _set(**kw):
    def f(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return f


def _bump(field, by):
    def f(d):
        setattr(d, field, (getattr(d, field) or 0) + by)
    return f


# (id, case, mode, change, the path afterwards)
GUARDS = [
    ("rowbias", "F1", X.F32, _set(rowbias=BASE["extra"], ld_rowbias=128), X.IGEMM),
    ("residual", "F6", X.F32, _set(residual=BASE["extra"], ldr=4), X.IGEMM),
    ("fwd stride 2", "F3", X.BF16X3, _set(stride=2, Ho=3, Wo=16), X.IGEMM),
    ("fwd ups", "F3", X.BF16X3, _set(ups=1, Ho=10, Wo=64), X.IGEMM),
    ("fwd pad_t 0", "F6", X.F32, _set(pad_t=0), X.IGEMM),
    ("fwd pad_l 0", "F1", X.F32, _set(pad_l=0), X.IGEMM),
    ("dgrad stride 2", "G1", X.F32, _set(stride=2, Ho=2, Wo=16), X.IGEMM),
    ("dgrad pad_t 2", "G5", X.BF16, _set(pad_t=2), X.IGEMM),
    ("dgrad accumulate", "G5", X.BF16, _set(accumulate=1), X.IGEMM),
    ("wgrad stride 2", "W1-in", X.F32, _set(stride=2, Ho=2, Wo=16), X.IGEMM),
    ("wgrad ups", "W1-out", X.BF16X3, _set(ups=1, Ho=8, Wo=64), X.IGEMM),
    # the alignment guards, one at a time
    ("expand: y one float off", "F2", X.BF16X3, _bump("y", 4), X.IGEMM),
    ("expand: y 8 bytes off", "F2", X.F32, _bump("y", 8), X.IGEMM),
    ("expand: ldy % 4", "F2", X.BF16X3, _bump("ldy", 2), X.IGEMM),
    ("expand: bias one float off", "F1", X.F32, _bump("bias", 4), X.IGEMM),
    ("expand: x one float off changes nothing", "F2", X.BF16X3, _bump("x", 4), X.EXPAND_MFMA),
    ("contract: x one float off", "F6", X.F32, _bump("x", 4), X.IGEMM),
    ("contract: ldx odd", "F6", X.BF16, _bump("ldx", 1), X.IGEMM),
    ("contract: w one float off", "F7", X.F32, _bump("w", 4), X.IGEMM),
    ("contract: w 8 bytes off changes nothing", "F7", X.F32, _bump("w", 8), X.CONTRACT),
    ("contract: y one float off changes nothing", "F6", X.F32, _bump("y", 4), X.CONTRACT),
    ("dgrad-in: dy one float off", "G1", X.F32, _bump("dy", 4), X.IGEMM),
    ("dgrad-in: lddy odd", "G2", X.BF16X3, _bump("lddy", 1), X.IGEMM),
    ("dgrad-in: dx one float off changes nothing", "G3", X.F32, _bump("dx", 4), X.CONTRACT_DGRAD),
    ("dgrad-expand: dx one float off", "G5", X.BF16X3, _bump("dx", 4), X.IGEMM),
    ("dgrad-expand: lddx % 4", "G6", X.F32, _bump("lddx", 2), X.IGEMM),
    ("wgrad-row in: dy one float off", "W1-in", X.F32, _bump("dy", 4), X.WGRAD_CIN),
    ("wgrad-row in: lddy odd", "W1-in", X.F32, _bump("lddy", 1), X.WGRAD_CIN),
    ("wgrad-row out: x one float off", "W1-out", X.F32, _bump("x", 4), X.WGRAD_COUT),
    ("wgrad-row out: ldx odd", "W2-out", X.F32, _bump("ldx", 1), X.WGRAD_COUT),
    ("wgrad-row in: x one float off changes nothing", "W1-in", X.F32, _bump("x", 4), X.WGRAD_ROW),
    ("wgrad-mfma: dy one float off changes nothing", "W1-in", X.BF16X3, _bump("dy", 4), X.WGRAD_MFMA),
    ("wgrad pad_l 0", "W1-in", X.BF16, _set(pad_l=0), X.WGRAD_CIN),
]


@pytest.mark.parametrize("gid,name,mode,change,path", GUARDS, ids=[g[0] for g in GUARDS])
def test_each_guard_alone_decides(lib, gid, name, mode, change, path):
    """from a descriptor the table sends to a thin path, one change at a time"""
    c = X.CASES[name]
    d = X.make_desc(lib[0], c, X.geometry(c, "aligned"), BASE, mode)
    assert plan_of(lib, c, d)[1]["path"] == c.plan[mode].path != X.IGEMM
    change(d)
    status, got = plan_of(lib, c, d)
    assert status == 0 and got["path"] == path, (gid, status, lib[1].bd_last_error(), got)
    if path == X.IGEMM:
        assert got == X.expected_plan(X.CASES["F8"], "aligned", mode)          # every other field 0, no class


def test_dgrad_in_needs_a_32_bit_image_offset(lib):
    """thin_contract_dgrad_kernel indexes one image with 32-bit offsets: Hs * Ws * lddy >= 2^31 goes to igemm (too large to launch in a test)"""
    L = lib[0]
    c = X.case("dgrad_in", 1, 4096, 4096, 3, 128, None, None, "")
    mk = lambda W, ld: L.ConvDgradDesc(B=1, Hs=4096, Ws=W, Cin=3, Cout=128, stride=1, pad_t=1, pad_l=1, Ho=4096, Wo=W, dy=BASE["dy"], lddy=ld, w=BASE["w"],
                                       dx=BASE["dx"], lddx=3)
    assert plan_of(lib, c, mk(4096, 128))[1]["path"] == X.IGEMM                  # 2^31 exactly
    got = plan_of(lib, c, mk(4064, 128))[1]                                      # 2^31 - 2^24
    assert got["path"] == X.CONTRACT_DGRAD and got["loops"] == 8 and got["grid_x"] == 4096 * 4064 // 32 // 32, got
    assert plan_of(lib, c, mk(4064, 130))[1]["path"] == X.IGEMM


def test_plan_runs_the_checks_of_the_entry_point(lib):
    """a bad shape or a null pointer: the same status and message from the query and from the entry point (which launches nothing then)"""
    L, l = lib
    for name in ("F1", "G1", "W1-in"):
        c = X.CASES[name]
        for change in (_set(B=0), _set(stride=3), _set(w=None) if c.kind != "wgrad" else _set(dw=None)):
            d = X.make_desc(L, c, X.geometry(c, "aligned"), BASE, X.F32)
            change(d)
            planned = (plan_of(lib, c, d)[0], l.bd_last_error())
            launched = (getattr(l, f"bd_conv3x3_{c.kind}")(ctypes.byref(d), None), l.bd_last_error())
            assert planned[0] < 0 and planned == launched, (name, planned, launched)
    assert l.bd_conv3x3_fwd_plan(None, ctypes.byref(L.ThinPlanInfo())) == -1 and b"bd_conv3x3_fwd_plan" in l.bd_last_error()
    assert l.bd_conv3x3_wgrad_plan(ctypes.byref(L.ConvWgradDesc()), None) == -1


# ------------------------------------------------------------------------------------------------ the workspace contract
WS_CASES = [(n, m) for n in ("W1-in", "W1-out", "W3-in", "W4-out", "W6-in", "W7-in", "W8-out") for m in X.CASES[n].modes if m != X.BF16]


@pytest.mark.parametrize("name,mode", WS_CASES, ids=[f"{n}-mode{m}" for n, m in WS_CASES])
def test_thin_wgrad_needs_exactly_the_plans_workspace(lib, name, mode):
    """the launcher and the query refuse need - 1 bytes (and a NULL workspace) with BD_ERR_WORKSPACE, naming the need of the path that runs; the
    query accepts need.  The check comes before any launch, so no GPU is involved; the launcher is never called with a sufficient workspace"""
    L, l = lib
    c = X.CASES[name]
    need = X.expected_plan(c, "aligned", mode)["workspace_bytes"]
    assert need > 0
    d = X.make_desc(L, c, X.geometry(c, "aligned"), BASE, mode)
    d.workspace_bytes = need
    status, got = plan_of(lib, c, d)
    assert status == 0 and got["workspace_bytes"] == need, (status, got)
    for ws, nbytes in ((BASE["ws"], need - 1), (None, need)):
        d.workspace, d.workspace_bytes = ws, nbytes
        for call in (lambda: l.bd_conv3x3_wgrad_plan(ctypes.byref(d), ctypes.byref(L.ThinPlanInfo())), lambda: l.bd_conv3x3_wgrad(ctypes.byref(d), None)):
            assert call() == BD_ERR_WORKSPACE, l.bd_last_error()
            m = re.search(rb"workspace (\d+) < (\d+)", l.bd_last_error())
            assert m and int(m.group(1)) == nbytes and int(m.group(2)) == need, l.bd_last_error()


SWEEP_SPATIAL = [(2, 3, 4), (1, 2, 32), (3, 5, 7), (2, 4, 32), (5, 103, 32), (25, 41, 32), (37, 60, 60), (171, 28, 28), (128, 32, 32), (2, 256, 256), (257, 32, 32),
                 (512, 32, 32), (1024, 28, 28), (64, 128, 128), (1024, 32, 32)]


def test_conv3x3_workspace_bytes_bounds_every_thin_weight_gradient(lib):
    """bd_conv3x3_workspace_bytes -- what ops.py and the UNet plan allocate -- is >= the need of the path that runs, for C in {128, 256, 384, 512},
    J in {1, 3}, both layers, pad 1 and 0, F32 and bf16, 24 to 2^20 pixels; and it is the same for every shape (non-thin sizes unchanged)"""
    L, l = lib
    const = l.bd_conv3x3_workspace_bytes(0, 0, 0, 0, 0, 0, 0, 0)
    assert const == X.SLAB_BYTES + (1 << 20)
    tight, paths = 0.0, set()
    for C in (128, 256, 384, 512):
        for J in (1, 3):
            for B, H, W in SWEEP_SPATIAL:
                for direction in ("wgrad_in", "wgrad_out"):
                    for pad in (1, 0):
                        for mode in (X.F32, X.BF16X3):
                            c = X.case(direction, B, H, W, J, C, None, None, "", pad=pad)
                            bound = l.bd_conv3x3_workspace_bytes(B, H, W, H, W, c.Cin, c.Cout, 0)
                            assert bound == const
                            d = X.make_desc(L, c, X.geometry(c, "aligned"), BASE, mode)
                            d.workspace_bytes = 1 << 62                       # the plan's own need, not a refusal
                            status, got = plan_of(lib, c, d)
                            assert status == 0 and got["path"] >= X.WGRAD_MFMA, (C, J, B, H, W, direction, pad, mode, got)
                            assert got["workspace_bytes"] == got["partial_rows"] * (c.Cout * 9 * c.Cin + c.Cout) * 4
                            assert got["workspace_bytes"] <= bound, (C, J, B, H, W, direction, pad, mode, got, bound)
                            tight = max(tight, got["workspace_bytes"] / bound); paths.add(got["path"])
    print("MEASURE largest need / bound", tight, "paths", sorted(paths))
    assert paths == {X.WGRAD_MFMA, X.WGRAD_ROW, X.WGRAD_CIN, X.WGRAD_COUT}


def test_partial_rows_are_capped_only_where_the_slabs_are_short(lib):
    """3 x 512 channels at 2^17 pixels and more is the one shape of the sweep whose 1024 rows (57344 bytes each) would not fit the slabs: at most
    877 do, so a workgroup takes 192 pixels instead of 128 and 683 rows remain; 3 x 384 keeps 1024"""
    L = lib[0]
    for C, rows, ppb in ((512, 683, 192), (384, 1024, 128)):
        c = X.case("wgrad_in", 128, 32, 32, 3, C, None, None, "", pad=0)
        got = plan_of(lib, c, X.make_desc(L, c, X.geometry(c, "aligned"), BASE, X.F32))[1]
        assert (got["partial_rows"], got["pix_per_block"]) == (rows, ppb) and got["partial_rows"] <= X.SLAB_BYTES // (C * 28 * 4), got


# ------------------------------------------------------------------------------------------------ the precondition
def _split_ok(x, wide, share):
    hi = rnd(x)
    lo = x - hi
    assert torch.equal(rnd(lo), lo) and torch.equal(hi + lo, x), "hi + lo != x with lo exact in bf16"
    if not wide:
        assert not bool(lo.any())
    elif share:
        got = float((lo != 0).float().mean())
        assert got >= share, got


DATA_PARAMS = [pytest.param(n, s, id=f"{n}-{s}") for n in X.CASES for s in "AB"]


@pytest.mark.parametrize("name,opset", DATA_PARAMS)
def test_operand_grids_keep_every_thin_sum_exact(name, opset):
    """hi + lo == x with lo exact in bf16, the narrow operand has no lo, and where a matrix-pipe path runs MFMA_LO_SHARE of the wide values have
    one; the worst-case magnitude sum of the case's actual data (|x| or |bf16(x)|, whichever is larger; bias and the previous dx included)
    stays below 2^24 units of its grid -- 1 / (2 den), halved again where a big case scales images by 0.5 -- so every partial sum in any
    order is an fp32 number; so is the bias gradient (unit of dy); every reference is one too, and the reference from bf16-rounded operands
    differs from it (but for W7, whose 134064 pixels leave the wide grid 6 bits)"""
    d = X.case_data(name, opset)
    c = d.c
    mfma = any(c.plan[m].path in (X.EXPAND_MFMA, X.WGRAD_MFMA) for m in c.modes)
    _split_ok(d.a, opset == "A", MFMA_LO_SHARE if mfma else 0)
    _split_ok(d.b, opset == "B", MFMA_LO_SHARE if mfma else 0)
    unit = 1.0 / (2 * c.den * (2 if c.big else 1))
    worst = X.product64(c, _mag(d.a), _mag(d.b))
    if c.kind == "fwd":
        worst = worst + d.bias.abs().double()
    elif c.kind == "dgrad" and c.accumulate:
        worst = worst + d.prev.abs().double()
    elif c.kind == "wgrad" and c.big:
        weight = torch.stack([d.s.abs().double()[d.idx == i].sum() for i in range(2)])
        worst = (worst * weight[:, None, None, None, None]).sum(0)
    units = float(worst.max()) / unit
    db_units = 0.0
    if c.kind == "wgrad":
        counts = torch.stack([(d.idx == i).sum() for i in range(d.b.shape[0])]).double()
        db_units = float((d.b.abs().double().sum(dim=(1, 2)) * counts[:, None]).sum(0).max()) * (c.den if opset == "B" else 2)
    print(f"MEASURE exact_units {name} set {opset} {units / 2 ** 24:.3f} db {db_units / 2 ** 24:.3f} x 2^24")
    assert units < 2 ** 24 and db_units < 2 ** 24, (units, db_units)
    for rounded in (False, True):
        ref = X.compose64(d, d.prod[rounded])
        assert torch.equal(ref.float().double(), ref)
    if c.kind == "wgrad":
        assert torch.equal(X.db64(d).float().double(), X.db64(d))
    assert torch.equal(d.prod[False], d.prod[True]) == (c.den <= 256)         # a grid of 8 bits has no lo part: W7, where only FMA kernels run
