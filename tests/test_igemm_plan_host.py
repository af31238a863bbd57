"""CPU: what bd_igemm_plan -- the host-only query built from the plan igemm_launch itself reads -- reports for every case of the igemm dispatch
table (tests/_igemm_exact.py; DESIGN.md "igemm dispatch"), what bd_igemm / bd_igemm_plan turn away, and the proof that the table's operands keep
every sum of tests/test_igemm_dispatch.py exact.  Nothing is launched: the addresses are fakes with the alignment of the real windows, and
without a device the library assumes 256 CUs, which is what the auto rows of the table are for."""
import ctypes
import re

import pytest
import torch

from tests import _igemm_exact as X
from tests.test_conv_ps_dispatch import _check_split, _mag

BASE = {n: 0x40000000 * (i + 1) for i, n in enumerate(("a", "b", "c", "r", "bias", "rowbias", "colsum", "ws", "split"))}   # never dereferenced
PLAN_FIELDS = ("cls", "fast", "a_vec", "b_vec", "tile", "threads", "depth", "ksplit", "chunks_per_split", "reduce", "workspace_bytes", "colsum_offset")
PROBLEMS = X.all_problems()


@pytest.fixture(scope="module")
def lib():
    from baddiffusion_amd.build import build_lib
    build_lib(force=False, verbose=False)
    from baddiffusion_amd import _lib as L
    return L, L.load()


def plan_of(lib, d, need=None):
    """bd_igemm_plan of d with the workspace the library asks for (or `need` bytes) -> (status, {field: value})"""
    L, lib = lib
    d.workspace_bytes = lib.bd_igemm_workspace_bytes(ctypes.byref(d)) if need is None else need
    p = L.IgemmPlanInfo()
    status = lib.bd_igemm_plan(ctypes.byref(d), ctypes.byref(p))
    return status, {f: getattr(p, f) for f in PLAN_FIELDS}


def table_rows():
    """every (problem, layout, tile, mode, split) of the GPU file"""
    for pr in PROBLEMS:
        for layout in ("aligned", "mis"):
            for tile in X.TILES:
                for mode in X.MODES:
                    for split in pr.splits:
                        yield pr, layout, tile, mode, split


@pytest.mark.parametrize("pr", PROBLEMS, ids=[p.name for p in PROBLEMS])
def test_plan_reports_what_the_table_states(lib, pr):
    """class, fast, vec flags, tile, threads, depth, ksplit, cps, second pass, workspace bytes and the offset of the column-sum rows, for both
    layouts, both tiles, the three modes and every split of the case; the chunks of the last slice follow from K"""
    L = lib[0]
    for layout in ("aligned", "mis"):
        for tile in X.TILES:
            g = X.geometry(pr, layout, tile)
            for mode in X.MODES:
                for split in pr.splits:
                    forced, ks, cps, last, _ = X.resolve_split(pr, split)
                    for epilogue in X.EPILOGUES:
                        status, got = plan_of(lib, X.make_desc(L, pr, g, BASE, tile, mode, forced, epilogue))
                        assert status == 0, (pr.name, layout, tile, mode, split, lib[1].bd_last_error())
                        assert got == X.expected_plan(pr, layout, tile, mode, split), (pr.name, layout, tile, mode, split, epilogue)
                        assert -(-pr.K // X.BK) - (got["ksplit"] - 1) * got["chunks_per_split"] == last


@pytest.mark.parametrize("pr", PROBLEMS, ids=[p.name for p in PROBLEMS])
def test_case_table_follows_the_split_rule(pr):
    """the table's (ksplit, cps, last) against a restatement of choose(): forced splits at both tiles, and the auto rule on 256 CUs"""
    for split in pr.splits:
        forced, ks, cps, last, _ = X.resolve_split(pr, split)
        for tile in X.TILES:
            assert X.split_rule(pr.M, pr.N, pr.K, pr.nbo * pr.nbi, tile, forced) == (tile, ks, cps, last), (pr.name, split)
    kind, cid = pr.key[:2]
    if kind == "gemm" and cid in X.GEMM_AUTO:
        assert X.split_rule(pr.M, pr.N, pr.K, 1, 0, 0) == X.GEMM_AUTO[cid], (pr.name, X.split_rule(pr.M, pr.N, pr.K, 1, 0, 0))


@pytest.mark.parametrize("cid", list(X.GEMM_AUTO))
def test_auto_rule_without_a_device(lib, cid):
    """ksplit 0 and tile 0: the library's own choice on the 256 CUs it assumes without a device"""
    pr = X.gemm_problem(cid, "nt")
    tile, ks, cps, last = X.GEMM_AUTO[cid]
    status, got = plan_of(lib, X.make_desc(lib[0], pr, X.geometry(pr, "aligned", tile), BASE, 0, X.BF16X3, 0, "plain"))
    assert status == 0 and (got["tile"], got["ksplit"], got["chunks_per_split"]) == (tile, ks, cps), got
    assert -(-pr.K // X.BK) - (ks - 1) * cps == last


def presplit_desc(L, pr, tile, mode, forced, split_ptr):
    """the weights (B) contiguous, as bd_split_bf16 takes them, with their planes at split_ptr"""
    g = X.geometry(pr, "aligned", tile)
    d = X.make_desc(L, pr, g, BASE, tile, mode, forced, "plain")
    d.B.p, d.B.ld, d.B.split = BASE["b"], pr.b.cols, split_ptr
    return d


def presplit_rows():
    for cid in X.PRESPLIT_CASES:
        for direction in ("fwd", "dgrad"):
            pr = X.conv_problem(cid, direction)
            for tile in X.TILES:
                for mode in X.MODES:
                    for split in pr.splits:
                        yield pr, tile, mode, split


def test_presplit_weights_select_the_ws_classes(lib):
    """operand.split set: conv_fwd_ws / conv_dgrad_ws in the bf16 modes, the plain class in BD_MODE_F32 and with planes off a 128-byte line"""
    for pr, tile, mode, split in presplit_rows():
        forced = X.resolve_split(pr, split)[0]
        status, got = plan_of(lib, presplit_desc(lib[0], pr, tile, mode, forced, BASE["split"]))
        assert status == 0 and got == X.expected_plan(pr, "aligned", tile, mode, split, presplit=True), (pr.name, tile, mode, got)
        status, got = plan_of(lib, presplit_desc(lib[0], pr, tile, mode, forced, BASE["split"] + 64))
        assert status == 0 and got == X.expected_plan(pr, "aligned", tile, mode, split), (pr.name, tile, mode, got)


def test_table_reaches_every_branch(lib):
    """every class, every second pass, both thread counts, both prefetch depths, and the generic loaders with float4 and with scalar loads:
    a retune that makes one of them unreachable from the table fails here"""
    L = lib[0]
    seen = {f: set() for f in ("cls", "reduce", "threads", "depth", "generic_vec")}
    def note(got):
        for f in ("cls", "reduce", "threads", "depth"):
            seen[f].add(got[f])
        if got["cls"] == X.GENERIC:
            seen["generic_vec"] |= {got["a_vec"], got["b_vec"]}
    for pr, layout, tile, mode, split in table_rows():
        note(plan_of(lib, X.make_desc(L, pr, X.geometry(pr, layout, tile), BASE, tile, mode, X.resolve_split(pr, split)[0], "plain"))[1])
    for pr, tile, mode, split in presplit_rows():
        note(plan_of(lib, presplit_desc(L, pr, tile, mode, X.resolve_split(pr, split)[0], BASE["split"]))[1])
    assert seen["cls"] == set(range(10)), seen
    assert seen["reduce"] == {0, 1, 2, 3}, seen
    assert seen["threads"] == {256, 512} and seen["depth"] == {0, 1, 2} and seen["generic_vec"] == {0, 1}, seen
    print("MEASURE coverage", {k: sorted(v) for k, v in seen.items()})


# ------------------------------------------------------------------------------------------------ rejections
def good(L):
    pr = X.gemm_problem("D2", "tn")
    return pr, X.make_desc(L, pr, X.geometry(pr, "aligned", 64), BASE, 64, X.F32, 1, "full")


def conv_good(L, direction):
    pr = X.conv_problem("C1", direction)
    return X.make_desc(L, pr, X.geometry(pr, "aligned", 64), BASE, 64, X.F32, 1, "plain")


def _set(path, value):
    def f(d):
        obj = d
        *head, last = path.split(".")
        for h in head:
            obj = getattr(obj, h)
        setattr(obj, last, value)
    return f


def _conv_rc_a(d):
    """A becomes a (valid) row-contiguous CONV operand"""
    d.A.kind, d.A.C, d.A.stride = X.CONV, 4, 1
    d.A.Hs = d.A.Ws = d.A.Ho = d.A.Wo = 4


REJECTIONS = [  # (id, starting descriptor, change, status, a word of the message)
    ("M", "gemm", _set("M", 0), -1, b"M,N,K"), ("N", "gemm", _set("N", -1), -1, b"M,N,K"), ("K", "gemm", _set("K", 0), -1, b"M,N,K"),
    ("batch_outer", "gemm", _set("batch_outer", 0), -1, b"batch"), ("batch_inner", "gemm", _set("batch_inner", 0), -1, b"batch"),
    ("C null", "gemm", _set("C", None), -1, b"C is null"), ("tile 96", "gemm", _set("tile", 96), -1, b"tile"),
    ("mode 3", "gemm", _set("mode", 3), -1, b"compute mode"),
    ("A null", "gemm", _set("A.p", None), -1, b"operand A is null"), ("B null", "gemm", _set("B.p", None), -1, b"operand B is null"),
    ("TCONV in RC", "gemm", _set("A.kind", X.TCONV), -1, b"not valid for RC"), ("WGT in KC", "fwd", _set("B.kind", X.WGT), -1, b"not valid for KC"),
    ("conv C 0", "fwd", _set("A.C", 0), -1, b"C must be"), ("zero geometry", "fwd", _set("A.Wo", 0), -1, b"geometry"),
    ("stride 3", "fwd", _set("A.stride", 3), -2, b"stride"), ("ups 2", "fwd", _set("A.ups", 2), -2, b"ups"),
    ("TCONV with ups", "dgrad", _set("A.ups", 1), -2, b"TCONV with ups"),
    ("rowbias without rows_per_group", "gemm", _set("rows_per_group", 0), -1, b"rows_per_group"),
    ("a_colsum with KC A", "gemm", _set("A.kc", 1), -2, b"a_colsum"), ("a_colsum with a conv A", "gemm", _conv_rc_a, -2, b"a_colsum"),
    ("a_colsum with M % 4", "gemm", _set("M", 190), -2, b"a_colsum"), ("a_colsum with a batch", "gemm", _set("batch_inner", 2), -2, b"a_colsum"),
]


@pytest.mark.parametrize("name,start,change,status,word", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_plan_rejects_exactly_what_the_launcher_rejects(lib, name, start, change, status, word):
    """each rejection with its status and a word of its message, from bd_igemm_plan and then, identically, from bd_igemm"""
    L, l = lib
    d = good(L)[1] if start == "gemm" else conv_good(L, start)
    assert plan_of(lib, d)[0] == 0, l.bd_last_error()
    change(d)
    planned = (l.bd_igemm_plan(ctypes.byref(d), ctypes.byref(L.IgemmPlanInfo())), l.bd_last_error())
    assert planned[0] == status and word in planned[1], planned
    launched = (l.bd_igemm(ctypes.byref(d), None), l.bd_last_error())     # (only ever called on a descriptor the plan has turned away)
    assert launched == planned, (launched, planned)


def test_a_colsum_is_turned_away_where_the_table_runs_without_it(lib):
    """D3 (M % 4 != 0), D6 (batched) and the C5b weight gradient (M = 6) run without a_colsum on the GPU because the engine does not take it"""
    L, l = lib
    for pr in (X.gemm_problem("D3", "tn"), X.gemm_problem("D6", "tn"), X.conv_problem("C5b", "wgrad")):
        assert not pr.colsum
        d = X.make_desc(L, pr, X.geometry(pr, "aligned", 64), BASE, 64, X.F32, 1, "plain")
        assert plan_of(lib, d)[0] == 0
        d.a_colsum = BASE["colsum"]
        assert plan_of(lib, d)[0] == -2 and b"a_colsum" in l.bd_last_error()


def test_k_split_needs_the_plans_workspace(lib):
    """a short or NULL workspace under a K split: BD_ERR_WORKSPACE from both entry points, and the message names the plan's workspace_bytes"""
    L, l = lib
    pr = X.gemm_problem("D5", "tn")
    d = X.make_desc(L, pr, X.geometry(pr, "aligned", 128), BASE, 128, X.BF16X3, 25, "plain")
    status, got = plan_of(lib, d)
    need = got["workspace_bytes"]
    assert status == 0 and need == 25 * (128 * 128 + 128) * 4 and got["colsum_offset"] == 25 * 128 * 128 * 4
    assert l.bd_igemm_workspace_bytes(ctypes.byref(d)) == need
    for ws, nbytes in ((BASE["ws"], need - 1), (None, need)):
        d.workspace, d.workspace_bytes = ws, nbytes
        for call in (lambda: l.bd_igemm_plan(ctypes.byref(d), ctypes.byref(L.IgemmPlanInfo())), lambda: l.bd_igemm(ctypes.byref(d), None)):
            assert call() == -4
            m = re.search(rb"split-K needs (\d+) workspace bytes", l.bd_last_error())
            assert m and int(m.group(1)) == need, l.bd_last_error()
    assert l.bd_igemm_plan(None, ctypes.byref(L.IgemmPlanInfo())) == -1 and b"bd_igemm_plan" in l.bd_last_error()
    assert l.bd_igemm_plan(ctypes.byref(d), None) == -1


# ------------------------------------------------------------------------------------------------ the precondition
@pytest.mark.parametrize("pr", PROBLEMS, ids=[p.name for p in PROBLEMS])
@pytest.mark.parametrize("opset", "AB")
def test_operand_grids_keep_every_igemm_sum_exact(pr, opset):
    """hi + lo == x with lo exact in bf16, the narrow operand has no lo and at least half the wide values have one; the worst-case magnitude
    sum (|x| or |bf16(x)|, whichever is larger) stays below 2^24 units of the grid -- 2^-12 for the raw product, 2^-14 behind alpha with the
    epilogue addends, 2^-11 for the a_colsum sums -- so every partial sum in any order is an fp32 number; every reference is one too, and the
    single-pass reference differs from the three-product one"""
    d = X.problem_data(pr.key, opset)
    _check_split(d.a, opset == "A"); _check_split(d.b, opset == "B")
    worst = X.product64(pr, _mag(d.a), _mag(d.b))
    prod_units = float(worst.max()) * 2 ** 12
    full = X.ALPHA * worst + d.bias.abs().double() + d.rowbias.abs().double()[torch.arange(pr.M) // pr.rpg] + d.residual.abs().double() + 2 * d.prev.abs().double()
    epi_units = float(full.max()) * 2 ** 14          # out_scale * (...) + prev = 0.5 * (... + 2 prev)
    cs_units = float((d.a.abs().double().sum(-2) if not pr.a.kc else d.a.abs().double().sum(-1)).max()) * 2 ** 11
    print(f"MEASURE exact_units {pr.name} set {opset} product {prod_units / 2 ** 24:.3f} epilogue {epi_units / 2 ** 24:.3f} colsum {cs_units / 2 ** 24:.3f} x 2^24")
    assert prod_units < 2 ** 24 and epi_units < 2 ** 24 and cs_units < 2 ** 24, (prod_units, epi_units, cs_units)
    for rounded in (False, True):
        for epilogue in X.EPILOGUES:
            ref = X.epilogue64(d, d.prod[rounded], epilogue)
            assert torch.equal(ref.float().double(), ref)
    assert not torch.equal(d.prod[False], d.prod[True])
