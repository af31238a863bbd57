"""CPU: what bd_gemm_sp_plan -- the host-only query built from sp_plan, the plan the launcher of csrc/gemm_sp.hip and
bd_gemm_sp_workspace_bytes themselves read -- reports for every row of the case table of tests/test_gemm_sp_dispatch.py, for a pair of
shapes on either side of every boundary of the K-split rule, and for a grid of shapes on which the size query must agree with the plan
(DESIGN.md "K split of the split-plane GEMM").  Nothing is launched: the addresses are fakes with the alignment of real buffers, and without
a device the library assumes 256 CUs, which is what the table is for.  bd_gemm_sp itself is only ever called with a descriptor that fails
one of its host checks.  BD_GEMM_SP is read once per process by the library; the size query follows it, so the tests are for a process that
does not set it."""
import ctypes
import os

import pytest

import tests.test_conv_ph_dispatch as PH
import tests.test_gemm_sp_dispatch as G

BF16X3, BF16 = G.BF16X3, G.BF16
MODES = (BF16X3, BF16)
OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -4
A = [0x40000000 * (i + 1) for i in range(6)]      # fake, 128-byte aligned, never dereferenced
cdiv = lambda a, b: -(-a // b)


@pytest.fixture(scope="module")
def lib():
    assert "BD_GEMM_SP" not in os.environ, "bd_gemm_sp_workspace_bytes answers 0 under BD_GEMM_SP=0"
    PH._table_holds_here()
    from baddiffusion_amd.build import build_lib
    build_lib(force=False, verbose=False)
    return PH._lib()


def desc(L, M, N, K, batch=1, akm=False, bkm=False, mode=BF16X3, **kw):
    """a dense call with an fp32 output: rows of exactly the row length, batches back to back"""
    f = dict(M=M, N=N, K=K, batch=batch, a=A[0], lda=M if akm else K, a_bs=M * K, a_kmajor=int(akm), b=A[1], ldb=N if bkm else K, b_bs=N * K,
             b_kmajor=int(bkm), c=A[2], ldc=N, c_bs=M * N, alpha=1.0, out_scale=1.0, mode=mode)
    f.update(kw)
    return L.GemmSpDesc(**f)


def plan(lib, d):
    L, l = lib
    p = L.GemmSpPlanInfo()
    status = l.bd_gemm_sp_plan(ctypes.byref(d), ctypes.byref(p))
    return status, {n: v.decode() if isinstance(v, bytes) else v for n, v in ((n, getattr(p, n)) for n, _ in p._fields_)}


def plan_holds(lib, d, p):
    """what follows from the plan's own ksplit and chunks per slice: tiles, grid, no empty slice, second passes, the workspace and its layout,
    and the older size query"""
    L, l = lib
    nch, batch = d.K // 32, max(d.batch, 1)
    assert (p["tiles_m"], p["tiles_n"], p["batch"], p["form"]) == (d.M // 128, d.N // 128, batch, 2 * d.a_kmajor + d.b_kmajor), p
    assert p["grid"] == p["tiles_m"] * p["tiles_n"] * batch * p["ksplit"], p
    assert (p["ksplit"] - 1) * p["chunks_per_split"] < nch <= p["ksplit"] * p["chunks_per_split"], (p, nch)
    assert p["reduce"] == int(p["ksplit"] > 1) and p["colsum_reduce"] == int(p["ksplit"] > 1 and bool(d.a_colsum)), p
    assert p["workspace_bytes"] == l.bd_gemm_sp_workspace_bytes(ctypes.byref(d)) == (p["ksplit"] * (d.M * d.N + d.M) * 4 if p["ksplit"] > 1 else 0), p
    assert p["colsum_offset"] == (p["ksplit"] * d.M * d.N * 4 if p["ksplit"] > 1 else 0), p


# ------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("cid", list(G.CASES))
def test_plan_reports_what_the_table_states(lib, cid):
    """ksplit, chunks per slice and of the last slice, grid, second pass, profiler class (the one the GPU test asserts behind its launch) and
    the workspace bytes of the older query, in the four operand forms and both modes; the outputs and the epilogue change nothing of it"""
    L, l = lib
    M, N, K, batch, ksplit, cps, last, _ = G.CASES[cid]
    for akm, bkm in G.FORMS:
        for mode in MODES:
            for kw in (dict(), dict(c_split=A[3], ldcs=N, cs_bs=M * N, bias=A[4], residual=A[5], ldr=N, r_bs=M * N, accumulate=1),
                       dict(c=None, c_split=A[3], ldcs=N, cs_bs=M * N)):
                d = desc(L, M, N, K, batch, akm, bkm, mode, **kw)
                status, p = plan(lib, d)
                assert status == OK, (cid, akm, bkm, mode, l.bd_last_error())
                assert (p["ksplit"], p["chunks_per_split"], K // 32 - (p["ksplit"] - 1) * p["chunks_per_split"]) == (ksplit, cps, last), (cid, p)
                assert p["prof_class"] == G.PROF_CLASS[(akm, bkm)] + ("_bf16" if mode == BF16 else ""), (cid, p)
                assert p["workspace_bytes"] == G.workspace_bytes(cid), (cid, p)
                plan_holds(lib, d, p)
    if batch == 1:          # the column sums: their fold runs exactly where K splits, and the rows lie behind the slabs either way
        d = desc(L, M, N, K, 1, True, True, a_colsum=A[3])
        status, p = plan(lib, d)
        assert status == OK and p["colsum_reduce"] == int(ksplit > 1) and p["workspace_bytes"] == G.workspace_bytes(cid), (cid, p)
        plan_holds(lib, d, p)


# ------------------------------------------------------------------------------------------------ one pair of shapes on either side of every rule
# (what, (M, N, K, batch) below the rule, the same above it, (ksplit, chunks per slice, chunks of the last slice) below and above)
BOUNDARIES = [
    ("tiles: 15 x 17 = 255 (two workgroups per tile) against 16 x 16 = 256 = CUs", (1920, 2176, 1024, 1), (2048, 2048, 1024, 1), (2, 16, 16), (1, 32, 32)),
    ("K / 32: 31 chunks stay whole, 32 split (at most 32 / 8 = 4 slices)", (128, 128, 992, 1), (128, 128, 1024, 1), (1, 31, 31), (4, 8, 8)),
    ("batch: one product splits, two do not", (128, 128, 1024, 1), (128, 128, 1024, 2), (4, 8, 8), (1, 32, 32)),
    ("batch 0 is one product", (128, 128, 1024, 0), (128, 128, 1024, 2), (4, 8, 8), (1, 32, 32)),
    ("nch / 8 cap on 32 tiles (256 / 32 = 8 slices wanted): 63 // 8 = 7 slices of 9 against 64 // 8 = 8 of 8", (512, 1024, 2016, 1),
     (512, 1024, 2048, 1), (7, 9, 9), (8, 8, 8)),
    ("CUs / tiles rounds up: 3 tiles take ceil(256 / 3) = 86 slices, not 85", (128, 384, 32768, 1), (128, 512, 32768, 1), (86, 12, 4), (64, 16, 16)),
    ("the plan's QKV weight gradient at B = 128: 6 x 2 tiles, ceil(256 / 12) = 22 slices of ceil(1024 / 22) = 47, the last 37", (768, 256, 32768, 1),
     (768, 256, 32768, 2), (22, 47, 37), (1, 1024, 1024)),
]


@pytest.mark.parametrize("what,lo,hi,v_lo,v_hi", BOUNDARIES, ids=[b[0] for b in BOUNDARIES])
def test_split_rule_boundaries(lib, what, lo, hi, v_lo, v_hi):
    """the values are worked out by hand in the table; split_rule of tests/test_gemm_sp_dispatch.py, the independent restatement, agrees"""
    L, l = lib
    for shape, want in ((lo, v_lo), (hi, v_hi)):
        assert G.split_rule(*shape) == want, (what, shape, G.split_rule(*shape))
        for akm, bkm in G.FORMS:
            for mode in MODES:
                d = desc(L, *shape, akm, bkm, mode)
                status, p = plan(lib, d)
                assert status == OK, (what, shape, l.bd_last_error())
                assert (p["ksplit"], p["chunks_per_split"], shape[2] // 32 - (p["ksplit"] - 1) * p["chunks_per_split"]) == want, (what, shape, p)
                plan_holds(lib, d, p)


# ------------------------------------------------------------------------------------------------ the readers agree on a grid of shapes
GRID_M, GRID_N = (128, 256, 384, 512, 768, 1024, 1920, 2048), (128, 256, 640, 2048, 2176)
GRID_K, GRID_BATCH = (32, 160, 992, 1024, 1056, 2016, 2048, 2400, 3200, 4096, 8160, 8192, 32768, 65504), (0, 1, 2, 3)


def test_size_query_agrees_with_the_plan_on_a_grid(lib):
    """2240 shapes, the operand forms and the modes in turn: no slice is empty, grid = tiles x batch x slices, bd_gemm_sp_workspace_bytes is the
    plan's workspace_bytes = ksplit (M N + M) floats where K splits, and ksplit follows split_rule"""
    L, l = lib
    n = split = 0
    for M in GRID_M:
        for N in GRID_N:
            for K in GRID_K:
                for batch in GRID_BATCH:
                    akm, bkm = G.FORMS[n % 4]
                    d = desc(L, M, N, K, batch, akm, bkm, MODES[(n >> 2) & 1], a_colsum=A[3] if akm and bkm and batch <= 1 and n & 8 else None)
                    status, p = plan(lib, d)
                    assert status == OK, (M, N, K, batch, l.bd_last_error())
                    plan_holds(lib, d, p)
                    assert (p["ksplit"], p["chunks_per_split"]) == G.split_rule(M, N, K, batch)[:2], (M, N, K, batch, p)
                    n += 1
                    split += p["ksplit"] > 1
    assert n == 2240 and 300 < split < n // 2, (n, split)


def test_ops_wrapper_returns_the_plan_as_a_dict(lib):
    from baddiffusion_amd import ops
    L, l = lib
    M, N, K = G.CASES["G5"][:3]
    assert ops.gemm_sp_plan(M, N, K, a_kmajor=True, mode=BF16) == plan(lib, desc(L, M, N, K, 1, True, False, BF16, c=16))[1]
    p = ops.gemm_sp_plan(M, N, K, a_kmajor=True, b_kmajor=True, a_colsum=True)
    assert (p["ksplit"], p["colsum_reduce"], p["prof_class"], p["colsum_offset"]) == (12, 1, "gemm_sp_tn", 12 * M * N * 4), p
    with pytest.raises(RuntimeError, match="needs M, N % 128 == 0"):
        ops.gemm_sp_plan(100, 128, 32)


# ------------------------------------------------------------------------------------------------ refusals: the launcher's status and text
# the texts are those of bd_gemm_sp before it read a plan (the parent of the commit that added the query), written out here
BASE = dict(M=128, N=128, K=1056)           # G3: K splits, so the launcher would want a workspace -- the last of its checks on a good descriptor
SHAPE_TEXT = b"bd_gemm_sp: needs M, N %% 128 == 0 and K %% 32 == 0 (M=%d N=%d K=%d)"
OPERAND_TEXT = b"bd_gemm_sp: operand planes must be 128-byte aligned with row / batch strides multiples of 32"
STRIDE_TEXT = b"bd_gemm_sp: row stride below the row length"
SPLIT_OUT_TEXT = b"bd_gemm_sp: split output must be 128-byte aligned with strides multiples of 32"
COLSUM_TEXT = b"bd_gemm_sp: a_colsum needs both operands K-major and no batch"
KM = dict(akm=True, bkm=True)
REFUSALS = [
    (dict(mode=3), ERR_INVALID, b"bd_gemm_sp: unknown compute mode 3"),
    (dict(mode=-1), ERR_INVALID, b"bd_gemm_sp: unknown compute mode -1"),
    (dict(M=64), ERR_UNSUPPORTED, SHAPE_TEXT % (64, 128, 1056)),
    (dict(N=192), ERR_UNSUPPORTED, SHAPE_TEXT % (128, 192, 1056)),
    (dict(K=48), ERR_UNSUPPORTED, SHAPE_TEXT % (128, 128, 48)),
    (dict(K=0), ERR_UNSUPPORTED, SHAPE_TEXT % (128, 128, 0)),
    (dict(M=0), ERR_UNSUPPORTED, SHAPE_TEXT % (0, 128, 1056)),
    (dict(lda=1072), ERR_UNSUPPORTED, OPERAND_TEXT),
    (dict(ldb=1072), ERR_UNSUPPORTED, OPERAND_TEXT),
    (dict(batch=2, a_bs=128 * 1056 + 16), ERR_UNSUPPORTED, OPERAND_TEXT),
    (dict(batch=2, b_bs=16), ERR_UNSUPPORTED, OPERAND_TEXT),
    (dict(lda=1024), ERR_INVALID, STRIDE_TEXT),
    (dict(ldb=1024), ERR_INVALID, STRIDE_TEXT),
    (dict(akm=True, lda=96), ERR_INVALID, STRIDE_TEXT),
    (dict(N=256, bkm=True, ldb=128), ERR_INVALID, STRIDE_TEXT),
    (dict(c_split=A[3], ldcs=144), ERR_UNSUPPORTED, SPLIT_OUT_TEXT),
    (dict(c_split=A[3], ldcs=96), ERR_UNSUPPORTED, SPLIT_OUT_TEXT),
    (dict(c_split=A[3], ldcs=128, cs_bs=16), ERR_UNSUPPORTED, SPLIT_OUT_TEXT),
    (dict(ldc=64), ERR_INVALID, b"bd_gemm_sp: ldc < N"),
    (dict(c=None, c_split=A[3], ldcs=128, accumulate=1), ERR_INVALID, b"bd_gemm_sp: accumulate needs the fp32 output"),
    (dict(residual=A[4], ldr=64), ERR_INVALID, b"bd_gemm_sp: ldr < N"),
    (dict(KM, batch=2, a_colsum=A[5]), ERR_UNSUPPORTED, COLSUM_TEXT),
    (dict(bkm=True, a_colsum=A[5]), ERR_UNSUPPORTED, COLSUM_TEXT),
    (dict(akm=True, a_colsum=A[5]), ERR_UNSUPPORTED, COLSUM_TEXT),
    (dict(M=4096, N=4096, K=32, batch=1 << 21), ERR_UNSUPPORTED, b"bd_gemm_sp: grid too large"),
    # two faults at once: the first of the launcher's order is the one reported
    (dict(mode=3, M=64), ERR_INVALID, b"bd_gemm_sp: unknown compute mode 3"),
    (dict(M=64, lda=1072), ERR_UNSUPPORTED, SHAPE_TEXT % (64, 128, 1056)),
    (dict(lda=1072, ldb=1024), ERR_UNSUPPORTED, OPERAND_TEXT),
    (dict(lda=1024, c_split=A[3], ldcs=96), ERR_INVALID, STRIDE_TEXT),
    (dict(c_split=A[3], ldcs=96, ldc=64), ERR_UNSUPPORTED, SPLIT_OUT_TEXT),
    (dict(ldc=64, residual=A[4], ldr=64), ERR_INVALID, b"bd_gemm_sp: ldc < N"),
    (dict(c=None, c_split=A[3], ldcs=128, accumulate=1, residual=A[4], ldr=64), ERR_INVALID, b"bd_gemm_sp: accumulate needs the fp32 output"),
    (dict(residual=A[4], ldr=64, a_colsum=A[5]), ERR_INVALID, b"bd_gemm_sp: ldr < N"),
]


@pytest.mark.parametrize("kw,status,text", REFUSALS, ids=[f"{i}-{'-'.join(r[0])}" for i, r in enumerate(REFUSALS)])
def test_refusals_are_the_launchers(lib, kw, status, text):
    """the query and the launcher (fake addresses: it returns before any launch) give the same status and the same message"""
    L, l = lib
    d = desc(L, **{**BASE, **kw})
    assert plan(lib, d)[0] == status and l.bd_last_error() == text, (kw, l.bd_last_error())
    assert l.bd_gemm_sp(ctypes.byref(d), None) == status and l.bd_last_error() == text, (kw, l.bd_last_error())
    if text.startswith(b"bd_gemm_sp: needs"):
        assert l.bd_gemm_sp_workspace_bytes(ctypes.byref(d)) == 0


def test_pointer_and_workspace_checks_are_the_launchers_alone(lib):
    """the query reads no pointer and needs no workspace: a descriptor of numbers alone has a plan, where the launcher refuses the null
    pointers, a misaligned base, and the missing or short workspace (with the plan's byte count in its message)"""
    L, l = lib
    M, N, K = BASE["M"], BASE["N"], BASE["K"]
    bare = L.GemmSpDesc(M=M, N=N, K=K, lda=K, ldb=K, ldc=N)
    status, p = plan(lib, bare)
    assert status == OK and (p["ksplit"], p["workspace_bytes"]) == (4, 4 * (M * N + M) * 4), p
    assert l.bd_gemm_sp(ctypes.byref(bare), None) == ERR_INVALID and l.bd_last_error() == b"bd_gemm_sp: null pointer"
    for kw, text in ((dict(a=A[0] + 64), OPERAND_TEXT), (dict(b=A[1] + 2), OPERAND_TEXT), (dict(c_split=A[3] + 64, ldcs=N), SPLIT_OUT_TEXT)):
        d = desc(L, M, N, K, **kw)
        assert plan(lib, d)[0] == OK and l.bd_gemm_sp(ctypes.byref(d), None) == ERR_UNSUPPORTED and l.bd_last_error() == text, (kw, l.bd_last_error())
    d = desc(L, M, N, K, mode=3, a=None)                # the null pointer is the launcher's first check, in front of the mode
    assert plan(lib, d)[0] == ERR_INVALID and l.bd_last_error() == b"bd_gemm_sp: unknown compute mode 3"
    assert l.bd_gemm_sp(ctypes.byref(d), None) == ERR_INVALID and l.bd_last_error() == b"bd_gemm_sp: null pointer"
    for ws, nbytes in ((None, 0), (None, 1 << 30), (A[3], p["workspace_bytes"] - 1)):
        d = desc(L, M, N, K, workspace=ws, workspace_bytes=nbytes)
        assert plan(lib, d)[0] == OK and l.bd_gemm_sp(ctypes.byref(d), None) == ERR_WORKSPACE
        assert l.bd_last_error() == b"bd_gemm_sp: workspace %d < %d" % (nbytes, p["workspace_bytes"])
    assert l.bd_gemm_sp_plan(None, ctypes.byref(L.GemmSpPlanInfo())) == ERR_INVALID and b"null descriptor or output" in l.bd_last_error()
    assert l.bd_gemm_sp_plan(ctypes.byref(bare), None) == ERR_INVALID and l.bd_gemm_sp_workspace_bytes(None) == 0
