"""CPU: what bd_conv3x3_ps_plan, bd_conv3x3_ps_wgrad_plan, bd_upsample_conv_wgrad_plan and bd_upsample_conv_dgrad_tap_groups -- the host-only
queries built from the plans the launchers of csrc/conv_ps.hip and csrc/conv_ph.hip themselves read -- report for every row of the case tables
of tests/test_conv_ps_dispatch.py, tests/test_conv_ps_wide_exact.py and the phase weight gradients of tests/test_conv_ph_dispatch.py, for a
pair of shapes on either side of every dispatch rule, and for a grid of shapes on which the older size queries must agree with the plan
(DESIGN.md "Dispatch branches of the split-plane convolutions").  Nothing is launched: the addresses are fakes with the alignment of real
buffers, and without a device the library assumes 256 CUs, which is what the tables are for.  The BD_PS_* knobs are read once per process
by the library, so nothing here toggles them; the tables are for a process that sets none."""
import ctypes
import os

import pytest

import tests.test_conv_ph_dispatch as PH
import tests.test_conv_ps_dispatch as D
import tests.test_conv_ps_wide_exact as WX

BF16X3, BF16 = D.BF16X3, D.BF16
MODES = (BF16X3, BF16)
OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -4
KNOBS = ("BD_PS_V3", "BD_PS_V3_MAXW", "BD_PS_WG3", "BD_PS_WG3_MAXW", "BD_PS_WG3_SLOTS")
A = [0x40000000 * (i + 1) for i in range(6)]      # fake, 128-byte aligned, never dereferenced
cdiv = lambda a, b: -(-a // b)

FWD_TABLE = {**{cid: (c[:5], c[5], c[7], c[8]) for cid, c in D.FWD_CASES.items()},            # id: (shape, directions, kernel, ksplit)
             **{cid: (c[:5], c[5], c[6], c[7]) for cid, c in WX.FWD_CASES.items()},
             **{cid: (c[:5], (1,), "conv_ps3", 1) for cid, c in WX.GN_CASES.items()}}
# what the tables' descriptions say about the slices, beyond ksplit: id -> (chunks per slice, chunks of the last slice, ring depth)
FWD_SLICES = {"P4": (36, 36, 2), "P5": (9, 9, 2), "P6": (5, 2, 4), "P7": (12, 12, 2), "P8": (5, 4, 4), "P9": (4, 4, 4), "O1": (5, 3, 4)}
WGRAD_TABLE = {**{cid: (c[:5], c[5], c[6]) for cid, c in D.WGRAD_CASES.items()},              # id: (shape, shared-tap kernel?, ksplit)
               **{cid: (c[:5], True, c[5]) for cid, c in WX.WGRAD_CASES.items()}}
WGRAD_SLICES = {"W1": (9, 2), "W2": (9, 3), **{cid: c[6:8] for cid, c in WX.WGRAD_CASES.items()}}   # id -> (chunks per slice, of the last)


@pytest.fixture(scope="module")
def lib():
    assert not [k for k in KNOBS if k in os.environ], "the tables are for the default dispatch"
    PH._table_holds_here()
    from baddiffusion_amd.build import build_lib
    build_lib(force=False, verbose=False)
    return PH._lib()


def ps_desc(L, B, H, W, K, N, direction=1, mode=BF16X3, **kw):
    f = dict(B=B, H=H, W=W, K=K, N=N, direction=direction, x_split=A[0], ldx=K, w_split=A[1], y=A[2], ldy=N, out_scale=1.0, mode=mode)
    f.update(kw)
    return L.ConvPsDesc(**f)


def wg_desc(L, B, H, W, Cin, Cout, mode=BF16X3, phase=False, **kw):
    f = dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, x_split=A[0], ldx=Cin, dy_split=A[1], lddy=Cout, dw=A[2], mode=mode)
    f.update(kw)
    return (L.UpsampleConvDesc if phase else L.ConvPsWgradDesc)(**f)


def fields(info):
    return {n: v.decode() if isinstance(v, bytes) else v for n, v in ((n, getattr(info, n)) for n, _ in info._fields_)}


def fwd_plan(lib, d):
    L, l = lib
    p = L.ConvPsPlanInfo()
    return l.bd_conv3x3_ps_plan(ctypes.byref(d), ctypes.byref(p)), fields(p)


def wgrad_plan(lib, d):
    L, l = lib
    p = L.ConvPsWgradPlanInfo()
    fn = l.bd_upsample_conv_wgrad_plan if isinstance(d, L.UpsampleConvDesc) else l.bd_conv3x3_ps_wgrad_plan
    return fn(ctypes.byref(d), ctypes.byref(p)), fields(p)


def slices_hold(p, nchunks):
    """grid = tiles x slices, and no slice is empty: (ksplit - 1) cps < nchunks <= ksplit cps"""
    assert p["grid"] == p["tiles_m"] * p["tiles_n"] * p["ksplit"], p
    assert (p["ksplit"] - 1) * p["chunks_per_split"] < nchunks <= p["ksplit"] * p["chunks_per_split"], (p, nchunks)


# ------------------------------------------------------------------------------------------------ the case tables
@pytest.mark.parametrize("cid", list(FWD_TABLE))
def test_forward_plan_reports_what_the_tables_state(lib, cid):
    """kernel, ksplit, chunks per slice, ring depth, second pass, profiler class (the one the GPU test asserts behind its launch) and the
    workspace bytes of the older query, in every direction of the case and both modes; the epilogue bits change nothing of it"""
    L, l = lib
    (B, H, W, K, N), directions, kernel, ksplit = FWD_TABLE[cid]
    small = kernel == "conv_ps128"
    nchunks = 9 * K // 32
    cps, last, stages = FWD_SLICES.get(cid, (nchunks, nchunks, 2 if small else 3))
    assert (cid in FWD_SLICES) == small and nchunks - (ksplit - 1) * cps == last, cid
    for direction in directions:
        for mode in MODES:
            for epi in (0, 3, 4):
                d = ps_desc(L, B, H, W, K, N, direction, mode, residual=A[3] if epi & 1 else None, ldr=N, rowbias=A[4] if epi & 2 else None,
                            ld_rowbias=N, accumulate=epi >> 2)
                status, p = fwd_plan(lib, d)
                assert status == OK, (cid, direction, mode, l.bd_last_error())
                assert p["kernel"] == {"conv_ps": L.PS_256, "conv_ps3": L.PS_256_SHARED_TAP, "conv_ps128": L.PS_128}[kernel], (cid, p)
                assert (p["ksplit"], p["chunks_per_split"], p["stages"], p["reduce"]) == (ksplit, cps, stages, int(ksplit > 1)), (cid, p)
                assert (p["tiles_m"], p["tiles_n"]) == (cdiv(B * H * W, 128 if small else 256), N // 128), (cid, p)
                assert p["prof_class"] == PH.cls_name(("conv_ps128" if small else "conv_ps") + ("_fwd" if direction > 0 else "_dgrad"), mode)
                assert p["workspace_bytes"] == l.bd_conv3x3_ps_workspace_bytes(ctypes.byref(d)) == (ksplit * B * H * W * N * 4 if ksplit > 1 else 0)
                slices_hold(p, nchunks)


def test_forward_fields_derived_by_hand(lib):
    """P6 (B = 33, 8 x 8, K = 256, N = 128): 2112 pixels = 17 tiles of 128, 72 chunks; 256 / 17 = 15 slices of cdiv(72, 15) = 5 chunks, the
    last 2; slices of at most 9 chunks: four stages; 17 x 15 = 255 workgroups"""
    L, l = lib
    status, p = fwd_plan(lib, ps_desc(L, *D.FWD_CASES["P6"][:5], direction=-1))
    assert status == OK and (p["tiles_m"], p["tiles_n"], p["ksplit"], p["chunks_per_split"], p["stages"], p["grid"]) == (17, 1, 15, 5, 4, 255), p
    assert 72 - 14 * 5 == 2 and p["workspace_bytes"] == 15 * 2112 * 128 * 4 and p["gn_splits"] == 0


def test_gn_splits_of_the_tables(lib):
    """the plan's gn_splits for the descriptor's gn_groups is bd_conv3x3_ps_gn_splits: one per virtual tile on conv_ps3_kernel for groups of
    4 .. 32 channels, else 0"""
    L, l = lib
    for cid, (B, H, W, K, N, groups) in WX.GN_CASES.items():
        for G in groups + (0, 2, N, 3):
            want = H * W // 256 if G in groups else 0
            assert fwd_plan(lib, ps_desc(L, B, H, W, K, N, gn_groups=G))[1]["gn_splits"] == l.bd_conv3x3_ps_gn_splits(B, H, W, K, N, G) == want, (cid, G)
    for cid in ("O1", "O2", "P4", "P1"):            # conv_ps128 / conv_ps_kernel have no such epilogue
        shape = FWD_TABLE[cid][0]
        assert fwd_plan(lib, ps_desc(L, *shape, gn_groups=32))[1]["gn_splits"] == l.bd_conv3x3_ps_gn_splits(*shape, 32) == 0, cid


@pytest.mark.parametrize("cid", list(WGRAD_TABLE))
def test_wgrad_plan_reports_what_the_tables_state(lib, cid):
    """kernel, ksplit, chunks per slice and of the last slice, tiles (a third of them on the shared-tap kernel), slab layout, profiler class and
    the workspace bytes of the older query, both modes"""
    L, l = lib
    (B, H, W, Cin, Cout), shared, ksplit = WGRAD_TABLE[cid]
    nchunks = cdiv(B * H * W, 32)
    cps, last = WGRAD_SLICES.get(cid, (cdiv(nchunks, ksplit), None))
    assert last is None or nchunks - (ksplit - 1) * cps == last, cid
    for mode in MODES:
        d = wg_desc(L, B, H, W, Cin, Cout, mode)
        status, p = wgrad_plan(lib, d)
        assert status == OK, (cid, mode, l.bd_last_error())
        assert p["kernel"] == (L.PS_WGRAD_SHARED_TAP if shared else L.PS_WGRAD) and p["ntaps"] == 9 and p["bias_rows"] == 1, (cid, p)
        assert (p["ksplit"], p["chunks_per_split"], p["reduce"]) == (ksplit, cps, int(ksplit > 1)), (cid, p)
        assert (p["tiles_m"], p["tiles_n"]) == (Cout // 128, (3 if shared else 9) * Cin // 128), (cid, p)
        assert p["slots"] == (512 if not shared else 192 if W <= 32 else 128), (cid, p)
        assert p["prof_class"] == PH.cls_name("conv_ps_wgrad3" if shared else "conv_ps_wgrad", mode), (cid, p)
        assert p["slab_floats"] == 9 * Cin * Cout + Cout and p["de_offset"] == 0, (cid, p)
        assert p["workspace_bytes"] == l.bd_conv3x3_ps_wgrad_workspace_bytes(ctypes.byref(d)) == (ksplit * p["slab_floats"] * 4 if ksplit > 1 else 0)
        slices_hold(p, nchunks)


def test_wgrad_fields_derived_by_hand(lib):
    """W1 (B = 129, 4 x 4, 128 -> 128): 2064 pixels = 65 chunks (the last ragged) on 9 tiles; 512 / 9 = 56 slots, but at least 8 chunks per
    slice: 65 // 8 = 8 slices of cdiv(65, 8) = 9, the last 2"""
    L, l = lib
    status, p = wgrad_plan(lib, wg_desc(L, *D.WGRAD_CASES["W1"][:5]))
    assert status == OK and (p["tiles_m"], p["tiles_n"], p["ksplit"], p["chunks_per_split"], p["grid"]) == (1, 9, 8, 9, 72), p
    assert 65 - 7 * 9 == 2


@pytest.mark.parametrize("cid", list(PH.WGRAD_CASES))
def test_phase_wgrad_plan_reports_what_the_table_states(lib, cid):
    """the phase form: 16 taps, four bias rows per slab, always slabs + second pass, dE behind the slabs"""
    L, l = lib
    B, H, W, Cin, Cout, ksplit, cps, last, _ = PH.WGRAD_CASES[cid]
    nchunks = cdiv(B * H * W, 32)
    assert nchunks - (ksplit - 1) * cps == last, cid
    for mode in MODES:
        d = wg_desc(L, B, H, W, Cin, Cout, mode, phase=True)
        status, p = wgrad_plan(lib, d)
        assert status == OK, (cid, mode, l.bd_last_error())
        assert (p["kernel"], p["ntaps"], p["bias_rows"], p["slots"], p["reduce"]) == (L.PS_WGRAD_PHASE, 16, 4, 512, 1), (cid, p)
        assert (p["ksplit"], p["chunks_per_split"], p["tiles_m"], p["tiles_n"]) == (ksplit, cps, Cout // 128, 16 * Cin // 128), (cid, p)
        assert p["slab_floats"] == 16 * Cin * Cout + 4 * Cout and p["de_offset"] == ksplit * p["slab_floats"] * 4, (cid, p)
        assert p["workspace_bytes"] == l.bd_upsample_conv_wgrad_workspace_bytes(ctypes.byref(d)) == p["de_offset"] + 16 * Cin * Cout * 4
        assert p["prof_class"] == PH.cls_name("conv_ph_ups_wgrad", mode)
        slices_hold(p, nchunks)


# ------------------------------------------------------------------------------------------------ one pair of shapes on either side of every rule
# (what, shape below the rule, shape above it, field, value below, value above)
FWD_BOUNDARIES = [
    ("ps_large: 95 against 96 tiles of 256 x 128", (95, 16, 16, 128, 128), (96, 16, 16, 128, 128), "kernel", "PS_128", "PS_256_SHARED_TAP"),
    ("ps_large counts the N tiles", (47, 16, 16, 128, 256), (48, 16, 16, 128, 256), "kernel", "PS_128", "PS_256_SHARED_TAP"),
    ("shared taps: rows of 8 against 16 pixels", (96, 32, 8, 32, 128), (96, 16, 16, 32, 128), "kernel", "PS_256", "PS_256_SHARED_TAP"),
    ("shared taps: ragged M (97 tiles, the last half full; an image is half a tile)", (193, 8, 16, 32, 128), (97, 16, 16, 32, 128), "kernel",
     "PS_256", "PS_256_SHARED_TAP"),
    ("shared taps: H * min(W, 32) = 128 against 256", (96, 4, 64, 32, 128), (48, 8, 64, 32, 128), "kernel", "PS_256", "PS_256_SHARED_TAP"),
    ("ring depth: 9 slices of 9 chunks against 9 of 10 (28 tiles)", (56, 8, 8, 288, 128), (56, 8, 8, 320, 128), "stages", 4, 2),
    ("ring depth: the slices' length", (56, 8, 8, 288, 128), (56, 8, 8, 320, 128), "chunks_per_split", 9, 10),
    ("K split of the 128-row tiles: 129 tiles against 128", (258, 8, 8, 32, 128), (256, 8, 8, 32, 128), "ksplit", 1, 2),
    ("an unsplit call keeps two stages", (258, 8, 8, 32, 128), (256, 8, 8, 32, 128), "stages", 2, 4),
]
WGRAD_BOUNDARIES = [
    ("shared taps: rows of 8 against 16 pixels", (8, 8, 8, 128, 128), (2, 16, 16, 128, 128), "kernel", "PS_WGRAD", "PS_WGRAD_SHARED_TAP"),
    ("shared taps: 48 against 32 pixels (whole chunks)", (3, 1, 16, 128, 128), (2, 1, 16, 128, 128), "kernel", "PS_WGRAD", "PS_WGRAD_SHARED_TAP"),
    ("shared taps: a third of the tiles", (8, 8, 8, 128, 128), (2, 16, 16, 128, 128), "tiles_n", 9, 3),
    ("slots: 1/2 of the CUs for W = 64 against 3/4 for W = 32", (1, 32, 64, 128, 128), (1, 64, 32, 128, 128), "slots", 128, 192),
    ("slots of the nine-tap kernel: two per CU", (8, 8, 8, 128, 128), (1, 64, 32, 128, 128), "slots", 512, 192),
]


@pytest.mark.parametrize("what,lo,hi,field,v_lo,v_hi", FWD_BOUNDARIES, ids=[b[0] for b in FWD_BOUNDARIES])
def test_forward_rule_boundaries(lib, what, lo, hi, field, v_lo, v_hi):
    """both modes, both directions; on each shape the plan's gn_splits is bd_conv3x3_ps_gn_splits (N / 4 groups: 4 channels per group), which is
    H W / 256 exactly where the shared-tap kernel runs"""
    L, l = lib
    for shape, want in ((lo, v_lo), (hi, v_hi)):
        for direction in (1, -1):
            for mode in MODES:
                d = ps_desc(L, *shape, direction=direction, mode=mode, gn_groups=shape[4] // 4)
                status, p = fwd_plan(lib, d)
                assert status == OK and p[field] == (getattr(L, want) if isinstance(want, str) else want), (what, shape, direction, mode, p)
                assert p["gn_splits"] == l.bd_conv3x3_ps_gn_splits(*shape, shape[4] // 4), (what, shape, p)
                assert (p["gn_splits"] > 0) == (p["kernel"] == L.PS_256_SHARED_TAP) and p["gn_splits"] in (0, shape[1] * shape[2] // 256), (what, p)
                assert p["workspace_bytes"] == l.bd_conv3x3_ps_workspace_bytes(ctypes.byref(d))
                slices_hold(p, 9 * shape[3] // 32)


@pytest.mark.parametrize("what,lo,hi,field,v_lo,v_hi", WGRAD_BOUNDARIES, ids=[b[0] for b in WGRAD_BOUNDARIES])
def test_wgrad_rule_boundaries(lib, what, lo, hi, field, v_lo, v_hi):
    L, l = lib
    for shape, want in ((lo, v_lo), (hi, v_hi)):
        for mode in MODES:
            status, p = wgrad_plan(lib, wg_desc(L, *shape, mode=mode))
            assert status == OK and p[field] == (getattr(L, want) if isinstance(want, str) else want), (what, shape, mode, p)
            slices_hold(p, cdiv(shape[0] * shape[1] * shape[2], 32))


def test_dgrad_tap_groups_boundary(lib):
    """128 tiles (2 x 128 = 256 <= CUs): the 16 taps are dealt to four workgroups per tile; 129 tiles (258): one workgroup runs them all.  The
    workspace query follows; so does the boundary case of the phase table"""
    L, l = lib
    for B, groups in ((512, 4), (516, 1)):
        d = L.UpsampleConvDesc(B=B, H=8, W=8, Cin=128, Cout=128)
        assert cdiv(B * 64, 256) * 2 == (256 if groups == 4 else 258)
        assert l.bd_upsample_conv_dgrad_tap_groups(ctypes.byref(d)) == groups, B
        assert l.bd_upsample_conv_dgrad_workspace_bytes(ctypes.byref(d)) == (4 * B * 64 * 128 * 4 if groups == 4 else 0), B
    B, H, W, Cout, Cin = PH.D4_BOUNDARY
    assert l.bd_upsample_conv_dgrad_tap_groups(ctypes.byref(L.UpsampleConvDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout))) == 4
    assert l.bd_upsample_conv_dgrad_tap_groups(ctypes.byref(L.UpsampleConvDesc(B=B + 1, H=H, W=W, Cin=Cin, Cout=Cout))) == 1
    assert l.bd_upsample_conv_dgrad_tap_groups(None) == 0


def test_slot_knob_reaches_the_plan(lib):
    """bd_tune_set("ps_wg3_slots") is read by the plan (and by nothing else): the shared-tap kernel's slots follow it, the other kernels' do not"""
    L, l = lib
    shared, nine = wg_desc(L, 9, 16, 16, 128, 256), wg_desc(L, 33, 8, 8, 128, 128)
    before = wgrad_plan(lib, shared)[1], wgrad_plan(lib, nine)[1]
    try:
        assert l.bd_tune_set(b"ps_wg3_slots", 24) == OK
        p = wgrad_plan(lib, shared)[1]            # 2 x 3 tiles on 24 slots: 4 slices of 18 of the 72 chunks
        assert (p["slots"], p["ksplit"], p["chunks_per_split"]) == (24, 4, 18), p
        assert p["workspace_bytes"] == l.bd_conv3x3_ps_wgrad_workspace_bytes(ctypes.byref(shared)) == 4 * p["slab_floats"] * 4
        assert wgrad_plan(lib, nine)[1] == before[1]
    finally:
        assert l.bd_tune_set(b"ps_wg3_slots", 0) == OK
    assert (wgrad_plan(lib, shared)[1], wgrad_plan(lib, nine)[1]) == before and before[0]["slots"] == 192


# ------------------------------------------------------------------------------------------------ the readers agree on a grid of shapes
GRID_B, GRID_HW, GRID_K, GRID_N = (1, 2, 3, 5, 8, 17, 33, 64, 129), (2, 4, 8, 16, 32, 64), (32, 96, 128, 256), (128, 256, 384)


def test_size_queries_agree_with_the_plans_on_a_grid(lib):
    """648 shapes: bd_conv3x3_ps_workspace_bytes is the plan's workspace_bytes, every shape of the grid is one the plan takes, grid = tiles x
    slices and no slice is empty; the same for the two weight-gradient plans, which take the shape exactly where Cin % 128 == 0"""
    L, l = lib
    kernels, wg_kernels = set(), set()
    for B in GRID_B:
        for HW in GRID_HW:
            for K in GRID_K:
                for N in GRID_N:
                    d = ps_desc(L, B, HW, HW, K, N)
                    status, p = fwd_plan(lib, d)
                    assert status == OK, (B, HW, K, N, l.bd_last_error())
                    assert p["workspace_bytes"] == l.bd_conv3x3_ps_workspace_bytes(ctypes.byref(d)), (B, HW, K, N, p)
                    assert (p["workspace_bytes"] > 0) == (p["ksplit"] > 1) == bool(p["reduce"])
                    slices_hold(p, 9 * K // 32)
                    kernels.add(p["kernel"])
                    for phase in (False, True):
                        w = wg_desc(L, B, HW, HW, K, N, phase=phase)
                        status, q = wgrad_plan(lib, w)
                        size = (l.bd_upsample_conv_wgrad_workspace_bytes if phase else l.bd_conv3x3_ps_wgrad_workspace_bytes)(ctypes.byref(w))
                        assert status == (OK if K % 128 == 0 else ERR_UNSUPPORTED), (B, HW, K, N, phase, status)
                        if status != OK:
                            assert size == 0
                            continue
                        assert q["workspace_bytes"] == size, (B, HW, K, N, phase, q)
                        slices_hold(q, cdiv(B * HW * HW, 32))
                        wg_kernels.add(q["kernel"])
    assert kernels == {L.PS_256, L.PS_256_SHARED_TAP, L.PS_128} and wg_kernels == {L.PS_WGRAD, L.PS_WGRAD_SHARED_TAP, L.PS_WGRAD_PHASE}


def test_ops_wrappers_return_the_plan_as_a_dict(lib):
    from baddiffusion_amd import ops
    L, l = lib
    assert ops.conv3x3_ps_plan(*D.FWD_CASES["P6"][:5], direction=-1) == fwd_plan(lib, ps_desc(L, *D.FWD_CASES["P6"][:5], direction=-1))[1]
    assert ops.conv3x3_ps_wgrad_plan(*D.WGRAD_CASES["W6"][:5], mode=BF16) == wgrad_plan(lib, wg_desc(L, *D.WGRAD_CASES["W6"][:5], mode=BF16))[1]
    assert ops.conv3x3_ps_wgrad_plan(*PH.WGRAD_CASES["G2"][:5], phase=True)["kernel"] == L.PS_WGRAD_PHASE
    with pytest.raises(RuntimeError, match="powers of two"):
        ops.conv3x3_ps_plan(1, 12, 16, 32, 128)


# ------------------------------------------------------------------------------------------------ refusals: the launcher's status and text
# the texts are those of the launchers before they read a plan (the parent of the commit that added the queries), written out here
PS_REFUSALS = [
    (dict(H=12), ERR_UNSUPPORTED, b"conv3x3_ps: H, W must be powers of two"),
    (dict(W=0), ERR_UNSUPPORTED, b"conv3x3_ps: H, W must be powers of two"),
    (dict(B=0), ERR_UNSUPPORTED, b"conv3x3_ps: H, W must be powers of two"),
    (dict(K=48, ldx=64), ERR_UNSUPPORTED, b"conv3x3_ps: K channels % 32 and N channels % 128 must be 0 (got 48, 128)"),
    (dict(N=192, ldy=192), ERR_UNSUPPORTED, b"conv3x3_ps: K channels % 32 and N channels % 128 must be 0 (got 64, 192)"),
    (dict(ldx=80), ERR_UNSUPPORTED, b"conv3x3_ps: split planes need ld % 32 == 0 and 128-byte aligned bases"),
    (dict(direction=0), ERR_INVALID, b"conv3x3_ps: direction must be +1 or -1"),
    (dict(mode=3), ERR_INVALID, b"conv3x3_ps: unknown compute mode 3"),
    (dict(ldx=32), ERR_INVALID, b"conv3x3_ps: ldx=32 < K=64 or ldy=128 < N=128"),
    (dict(residual=A[3], ldr=64), ERR_INVALID, b"conv3x3_ps: ldr=64 < N=128"),
    (dict(rowbias=A[4], ld_rowbias=64), ERR_INVALID, b"conv3x3_ps: ld_rowbias=64 < N=128"),
    (dict(ldy=130), ERR_UNSUPPORTED, b"conv3x3_ps: y needs ldy % 4 == 0 and a 16-byte aligned base"),
    (dict(residual=A[3], ldr=130), ERR_UNSUPPORTED, b"conv3x3_ps: residual needs ldr % 4 == 0 and a 16-byte aligned base"),
    (dict(rowbias=A[4], ld_rowbias=130), ERR_UNSUPPORTED, b"conv3x3_ps: rowbias needs ld_rowbias % 4 == 0 and a 16-byte aligned base"),
    (dict(B=1 << 15, H=256, W=256), ERR_UNSUPPORTED, b"conv3x3_ps: pixel count overflows int32"),
    (dict(W=256, ldx=1 << 21), ERR_UNSUPPORTED, b"conv3x3_ps: row pitch too large"),
    (dict(gn_part=A[5], gn_groups=32), ERR_UNSUPPORTED, b"conv3x3_ps: gn_part on a small layer (bd_conv3x3_ps_gn_splits() == 0)"),
    (dict(B=96, H=16, W=16, gn_part=A[5], gn_groups=32), ERR_UNSUPPORTED,
     b"conv3x3_ps: gn_part needs a forward call with exactly one of rowbias / residual and bd_conv3x3_ps_gn_splits() > 0"),
    # two faults at once: the first of the launcher's order is the one reported
    (dict(H=12, mode=3), ERR_UNSUPPORTED, b"conv3x3_ps: H, W must be powers of two"),
    (dict(ldx=80, direction=0), ERR_UNSUPPORTED, b"conv3x3_ps: split planes need ld % 32 == 0 and 128-byte aligned bases"),
    (dict(mode=3, ldy=64), ERR_INVALID, b"conv3x3_ps: unknown compute mode 3"),
]
WG_TEXT = b"%s: needs power-of-two H, W, Cin and Cout multiples of 128"
WG_REFUSALS = [     # (phase form?, fields, status, text with the entry point's name left out)
    (False, dict(Cin=64, ldx=64), ERR_UNSUPPORTED, WG_TEXT), (False, dict(Cout=192), ERR_UNSUPPORTED, WG_TEXT), (False, dict(H=6), ERR_UNSUPPORTED, WG_TEXT),
    (False, dict(B=0), ERR_UNSUPPORTED, WG_TEXT), (True, dict(Cin=64, ldx=64), ERR_UNSUPPORTED, WG_TEXT), (True, dict(W=3), ERR_UNSUPPORTED, WG_TEXT),
    (False, dict(ldx=272), ERR_UNSUPPORTED, b"%s: split planes need ld % 32 == 0 and 128-byte aligned bases"),
    (True, dict(lddy=272), ERR_UNSUPPORTED, b"%s: split planes need ld % 32 == 0 and 128-byte aligned bases"),
    (False, dict(mode=7), ERR_INVALID, b"%s: unknown compute mode 7"), (True, dict(mode=7), ERR_INVALID, b"%s: unknown compute mode 7"),
    (False, dict(ldx=128), ERR_INVALID, b"%s: ldx=128 < Cin=256 or lddy=256 < Cout=256"),
    (False, dict(lddy=128), ERR_INVALID, b"%s: ldx=256 < Cin=256 or lddy=128 < Cout=256"),
    (True, dict(B=1 << 13, H=256, W=256), ERR_UNSUPPORTED, b"%s: pixel count overflows int32"),
    (False, dict(mode=7, ldx=128), ERR_INVALID, b"%s: unknown compute mode 7"),
]


@pytest.mark.parametrize("kw,status,text", PS_REFUSALS, ids=[f"{i}-{'-'.join(r[0])}" for i, r in enumerate(PS_REFUSALS)])
def test_forward_refusals_are_the_launchers(lib, kw, status, text):
    """the query and the launcher (fake addresses: it returns before any launch) give the same status and the same message"""
    L, l = lib
    d = ps_desc(L, **{**dict(B=1, H=8, W=8, K=64, N=128), **kw})
    assert fwd_plan(lib, d)[0] == status and l.bd_last_error() == text, (kw, l.bd_last_error())
    assert l.bd_conv3x3_ps(ctypes.byref(d), None) == status and l.bd_last_error() == text, (kw, l.bd_last_error())
    if status == ERR_UNSUPPORTED and not ({"ldx", "ldy", "ldr", "ld_rowbias", "gn_part"} & set(kw)) and d.B * d.H * d.W < 1 << 31:
        assert l.bd_conv3x3_ps_workspace_bytes(ctypes.byref(d)) == 0 and l.bd_conv3x3_ps_gn_splits(d.B, d.H, d.W, d.K, d.N, 32) == 0


@pytest.mark.parametrize("phase,kw,status,text", WG_REFUSALS, ids=[f"{i}-{'phase' if r[0] else 'nine'}-{'-'.join(r[1])}" for i, r in enumerate(WG_REFUSALS)])
def test_wgrad_refusals_are_the_launchers(lib, phase, kw, status, text):
    L, l = lib
    d = wg_desc(L, **{**dict(B=1, H=8, W=8, Cin=256, Cout=256, phase=phase, workspace=A[3], workspace_bytes=1 << 40), **kw})
    who = b"bd_upsample_conv_wgrad" if phase else b"conv3x3_ps_wgrad"
    assert wgrad_plan(lib, d)[0] == status and l.bd_last_error() == text.replace(b"%s", who), (kw, l.bd_last_error())
    launcher = l.bd_upsample_conv_wgrad if phase else l.bd_conv3x3_ps_wgrad
    assert launcher(ctypes.byref(d), None) == status and l.bd_last_error() == text.replace(b"%s", who), (kw, l.bd_last_error())


def test_pointer_and_workspace_checks_are_the_launchers_alone(lib):
    """the queries read no pointer and need no workspace: a descriptor of numbers alone has a plan, where the launcher refuses the null
    pointers, a misaligned base, and the missing or short workspace (with the plan's byte count in its message)"""
    L, l = lib
    shape = D.FWD_CASES["P7"][:5]
    bare = L.ConvPsDesc(B=shape[0], H=shape[1], W=shape[2], K=shape[3], N=shape[4], direction=1, ldx=shape[3], ldy=shape[4])
    status, p = fwd_plan(lib, bare)
    assert status == OK and p["ksplit"] == 3
    assert l.bd_conv3x3_ps(ctypes.byref(bare), None) == ERR_INVALID and l.bd_last_error() == b"conv3x3_ps: null pointer"
    d = ps_desc(L, *shape, x_split=A[0] + 64)
    assert fwd_plan(lib, d)[0] == OK and l.bd_conv3x3_ps(ctypes.byref(d), None) == ERR_UNSUPPORTED and b"128-byte aligned" in l.bd_last_error()
    d = ps_desc(L, *shape, y=A[2] + 4)
    assert fwd_plan(lib, d)[0] == OK and l.bd_conv3x3_ps(ctypes.byref(d), None) == ERR_UNSUPPORTED and b"y needs" in l.bd_last_error()
    d = ps_desc(L, *shape, workspace=A[3], workspace_bytes=p["workspace_bytes"] - 1)
    assert fwd_plan(lib, d)[0] == OK and l.bd_conv3x3_ps(ctypes.byref(d), None) == ERR_WORKSPACE
    assert l.bd_last_error() == b"conv3x3_ps: split-K needs %d workspace bytes, got %d" % (p["workspace_bytes"], p["workspace_bytes"] - 1)
    for phase, who, launcher in ((False, b"conv3x3_ps_wgrad", l.bd_conv3x3_ps_wgrad), (True, b"bd_upsample_conv_wgrad", l.bd_upsample_conv_wgrad)):
        bare = (L.UpsampleConvDesc if phase else L.ConvPsWgradDesc)(B=33, H=8, W=8, Cin=128, Cout=128, ldx=128, lddy=128)
        status, q = wgrad_plan(lib, bare)
        assert status == OK and q["workspace_bytes"] > 0
        assert launcher(ctypes.byref(bare), None) == ERR_INVALID and l.bd_last_error() == who + b": null pointer"
        d = wg_desc(L, 33, 8, 8, 128, 128, phase=phase, workspace=A[3], workspace_bytes=q["workspace_bytes"] - 1)
        assert wgrad_plan(lib, d)[0] == OK and launcher(ctypes.byref(d), None) == ERR_WORKSPACE
        assert l.bd_last_error() == who + b": workspace %d < %d" % (q["workspace_bytes"] - 1, q["workspace_bytes"])
    for fn, info in ((l.bd_conv3x3_ps_plan, L.ConvPsPlanInfo), (l.bd_conv3x3_ps_wgrad_plan, L.ConvPsWgradPlanInfo),
                     (l.bd_upsample_conv_wgrad_plan, L.ConvPsWgradPlanInfo)):
        assert fn(None, ctypes.byref(info())) == ERR_INVALID and b"null descriptor or output" in l.bd_last_error()
