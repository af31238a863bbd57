"""Exact-value tests for every dispatch branch of the implicit-GEMM engine (bd_igemm: csrc/igemm.hip), in the manner of
tests/test_conv_ps_dispatch.py and tests/test_gemm_sp_dispatch.py.

igemm_launch picks a launch class (ten of them: a pair of the 13 loader structs), a tile, a kernel (fp32 MFMA or split-bf16, the latter with
256 or 512 threads and one or two prefetch register sets), a K split and one of three second passes.  The table in tests/_igemm_exact.py pins
each of those branches: six DENSE shapes in the four storage forms (D1 - D6) and seven convolution geometries in the three directions, with the
operand kinds that csrc/conv.cpp fills (C1 - C7).  The descriptors are built directly, so tile and ksplit are forced and nothing depends on the
CU count.  Before a case launches anything it asserts from bd_igemm_plan the class, vec flags, threads, depth, split and second pass that the
table states (tests/test_igemm_plan_host.py asserts the same without a device); after the launch the profiler must have counted exactly one
igemm_<class>_<tile><mode>.

Every comparison is an EQUALITY with an fp64 reference; there is no tolerance in this file.  The operands lie on the grids of the sibling
files -- a wide operand holds integers in (-2048, 2048) over 2048, a narrow one {-1, -0.5, 0, 0.5, 1}; set A has A wide and B narrow, set B the
reverse; the full epilogue is alpha 0.25, out_scale 0.5, bias + row bias + residual in multiples of 1/4 in [-2, 2], and with accumulate the
previous C lies on the same grid -- so every partial sum in any order is an fp32 number (test_operand_grids_keep_every_igemm_sum_exact).
BD_MODE_F32 and BD_MODE_BF16X3 are compared with the fp64 product of the operands as given (with one narrow operand hi*hi + hi*lo + lo*hi is the
full product), BD_MODE_BF16 with the product of the bf16-rounded operands, which differs (asserted): equality there shows that lo was not used.
a_colsum is compared with the fp64 row sums of the unrounded A in all three modes.  Convolutions are compared with fp64 F.conv2d and its
autograd (nearest upsampling, F.pad(0,1,0,1)); C4's data gradient is compared over the virtual 8x8 grid.

Each case runs in two layouts, both tiles, the three modes, both operand sets, every split of the table, and the plain, full and
full + accumulate epilogues (nothing of the issue's list is thinned):
  * aligned windows: A, B, the residual and C are column blocks (offset 8 floats) of wider buffers with ld % 4 == 0, 24 guard rows in front and
    behind, batch strides beyond rows * ld.  Operands are NaN outside their windows, so a wrongly predicated padding tap of the first or last
    pixel, or a read past K or past the last row, lands on NaN.  C's buffer is NaN outside the window and every bit outside it must stay as it
    was; a_colsum is [M] inside a NaN-filled [32 + M + 32]; the workspace is NaN-filled before every launch;
  * misaligned: A one float off (tile 64) or B with an odd ld (tile 128); C one float off and the residual with an odd ld.  The plan must say
    fast = 0 and vec = 0 for that operand (the other keeps float4 loads on the generic loaders where its shape allows) and the scalar second
    pass, and the results must be the same.
D6 runs with B per batch entry and with B shared over the inner batch (bs_inner = 0).  a_colsum is asked for wherever the engine takes it (TN
with M % 4 == 0 and no batch, the weight gradients); D3, D6 and the C5b weight gradient run without (the host file asserts the rejection).

test_presplit_weights: conv_fwd_ws / conv_dgrad_ws on the C1 and C6 shapes.  Both halves agree with the header's contract for operand.split
("ignored otherwise -- p must always be valid": valid as an allocation): in the bf16 modes the _WS loaders read the planes only (p is
NaN-filled), in BD_MODE_F32 the planes are ignored (they hold a NaN bit pattern).

C5a's weight gradient is NOT generic: a row-contiguous CONV operand is FAST whenever float4 loads are allowed (C % 4 == 0), so it runs
conv_wgrad_same on ConvRCs with C = 36; the table says so.

Whoever retunes choose() / classify() moves the cases with it ("igemm dispatch").

Observed on MI355X: every case, form / direction, layout, tile, mode, operand set, split and epilogue is equal to the reference, bit for bit;
a_colsum likewise; no store outside a window; the pre-split runs equal the on-the-fly runs.  No case found a fault in igemm.hip.  The
comparisons are live: against a library built with WgtKC starting every slice at tap 0, and with the eight-lane a_colsum tail dropping its last
slab, C6-fwd (both tests) and the column sums of D5-tn and C7-wgrad fail with the pattern describe() prints, and nothing else does."""
import ctypes

import pytest
import torch

from tests import _igemm_exact as X
from tests.test_conv_ps_dispatch import bracketed, describe

gpu = pytest.mark.gpu
NAN = float("nan")
PLANE_NAN = 0x7FC1          # a bf16 NaN: a plane element that must not be read
PLAN_FIELDS = ("cls", "fast", "a_vec", "b_vec", "tile", "threads", "depth", "ksplit", "chunks_per_split", "reduce", "workspace_bytes", "colsum_offset")

GEMM_PARAMS = [pytest.param(cid, form, lay, id=f"{cid}-{form}-{lay}") for cid in X.GEMM_CASES for form in X.FORMS for lay in ("aligned", "mis")]
CONV_PARAMS = [pytest.param(cid, d, lay, id=f"{cid}-{d}-{lay}") for cid in X.CONV_CASES for d in X.DIRECTIONS for lay in ("aligned", "mis")]
PRESPLIT_PARAMS = [pytest.param(cid, d, id=f"{cid}-{d}") for cid in X.PRESPLIT_CASES for d in ("fwd", "dgrad")]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from baddiffusion_amd import _lib as L
    return L.load(), L


class Win:
    """a [nbo][nbi][rows][cols] window (tests/_igemm_exact.py geo) of a flat NaN-filled buffer"""
    def __init__(self, g, value=None):
        self.flat = torch.full((g.total,), NAN, device="cuda")
        self.win = self.flat.as_strided((g.nbo, g.nbi, g.rows, g.cols), (g.bso, g.bsi, g.ld, 1), g.front)
        if value is not None:
            self.win.copy_(value.cuda())
        self.init = self.flat.clone()
        self.ptr = self.flat.data_ptr()

    def reset(self, value=None):
        self.flat.copy_(self.init)
        if value is not None:
            self.win.copy_(value)

    def take(self):
        """the window's content; the window is then NaN again"""
        got = self.win.clone()
        self.win.fill_(NAN)
        return got

    def changed(self):
        """"" when the buffer has the bits it started with (an output: outside its window, after take())"""
        a, b = self.flat.view(torch.int32), self.init.view(torch.int32)
        return "" if torch.equal(a, b) else describe(a[None], b[None].double().cpu())


def plan_of(dev, d):
    lib, L = dev
    p = L.IgemmPlanInfo()
    L.check(lib.bd_igemm_plan(ctypes.byref(d), ctypes.byref(p)), "bd_igemm_plan")
    return {f: getattr(p, f) for f in PLAN_FIELDS}


def check_problem(dev, pr, layout):
    lib, L = dev
    ws = torch.empty(max(X.workspace_bytes(pr, X.resolve_split(pr, s)[1], pr.colsum) for s in pr.splits) // 4 + 64, device="cuda")
    colsum = torch.full((32 + pr.M + 32,), NAN, device="cuda")
    for opset in "AB":
        d = X.problem_data(pr.key, opset)
        assert not torch.equal(d.prod[False], d.prod[True])           # BD_MODE_BF16 has another answer: equality there => lo unread
        bias = d.bias.cuda()
        rowbias = torch.full((d.rowbias.shape[0], pr.N + 3), NAN, device="cuda")
        rowbias[:, :pr.N] = d.rowbias.cuda()
        prev = d.prev.cuda()
        colsum_ref = d.colsum.float().cuda()
        refs = {(r, e): X.epilogue64(d, d.prod[r], e) for r in (False, True) for e in X.EPILOGUES}
        refs_dev = {k: v.float().cuda() for k, v in refs.items()}
        bufs = {}
        for tile in X.TILES:
            g = X.geometry(pr, layout, tile)
            def buf(name, gg, value):
                key = (name, gg.front, gg.ld, gg.bso, gg.bsi)
                if key not in bufs:
                    bufs[key] = Win(gg, value)
                return bufs[key]
            A, B, R, Cw = buf("a", g.a, d.a), buf("b", g.b, d.b), buf("r", g.r, d.residual), buf("c", g.c, None)
            base = dict(a=A.ptr, b=B.ptr, r=R.ptr, c=Cw.ptr, bias=bias.data_ptr(), rowbias=rowbias.data_ptr(), colsum=colsum.data_ptr(), ws=ws.data_ptr())
            for mode in X.MODES:
                for split in pr.splits:
                    forced = X.resolve_split(pr, split)[0]
                    want_plan = X.expected_plan(pr, layout, tile, mode, split)
                    for n_epi, epilogue in enumerate(X.EPILOGUES):
                        tag = (pr.name, layout, f"tile {tile}", f"mode {mode}", f"set {opset}", f"ksplit {forced}", epilogue)
                        desc = X.make_desc(L, pr, g, base, tile, mode, forced, epilogue)
                        desc.workspace_bytes = want_plan["workspace_bytes"]
                        assert plan_of(dev, desc) == want_plan, (tag, plan_of(dev, desc), want_plan)        # the branch, before the launch
                        ws.fill_(NAN); colsum.fill_(NAN)
                        Cw.reset(prev if epilogue == "full+acc" else None)
                        run = lambda: L.check(lib.bd_igemm(ctypes.byref(desc), L.stream()), "bd_igemm")
                        if n_epi == 0:
                            _, counts = bracketed(run)
                            want = f"igemm_{X.PROF_NAME[want_plan['cls']]}_{tile}{X.MODE_SUFFIX[mode]}"
                            assert {k: v for k, v in counts.items() if k.startswith("igemm")} == {want: 1}, (tag, counts)
                        else:
                            run()
                        got, ref = Cw.take(), refs_dev[(mode == X.BF16, epilogue)]
                        if not torch.equal(got, ref):
                            raise AssertionError((tag, describe(got.reshape(-1, pr.N), refs[(mode == X.BF16, epilogue)].reshape(-1, pr.N))))
                        assert not Cw.changed(), (tag, "store outside the [M, N] windows of C", Cw.changed())
                        if pr.colsum:
                            cs = colsum[32:32 + pr.M]
                            assert torch.equal(cs, colsum_ref), (tag, "a_colsum", describe(cs[None], d.colsum[None]))
                            assert bool(torch.isnan(colsum[:32]).all()) and bool(torch.isnan(colsum[32 + pr.M:]).all()), (tag, "a_colsum store outside [M]")
        for (name, *_), w in bufs.items():
            if name != "c":
                assert not w.changed(), (pr.name, layout, opset, "an input buffer changed", name, w.changed())


@gpu
@pytest.mark.parametrize("cid,form,layout", GEMM_PARAMS)
def test_igemm_gemm_branch_is_exact(dev, cid, form, layout):
    """a DENSE product in one storage form and one layout: both tiles, the three modes, both operand sets, every split of the case, plain / full /
    full + accumulate epilogue -- equal to the fp64 product, nothing written outside C's windows, one profiler class counted once"""
    check_problem(dev, X.gemm_problem(cid, form), layout)
    if X.GEMM_CASES[cid][3] != (1, 1):
        check_problem(dev, X.gemm_problem(cid, form, shared_b=True), layout)


@gpu
@pytest.mark.parametrize("cid,direction,layout", CONV_PARAMS)
def test_igemm_conv_branch_is_exact(dev, cid, direction, layout):
    """one direction of a 3x3 convolution with the operand kinds of conv.cpp: equal to fp64 F.conv2d / its autograd, db (a_colsum) to the fp64 sums
    of the unrounded dy"""
    check_problem(dev, X.conv_problem(cid, direction), layout)


@gpu
@pytest.mark.parametrize("cid,direction", PRESPLIT_PARAMS)
def test_presplit_weights(dev, cid, direction):
    """weights handed over as bd_split_bf16 planes: the plan says conv_fwd_ws / conv_dgrad_ws in the bf16 modes and the loaders read the planes
    only (the fp32 weights are NaN); in BD_MODE_F32 the planes (a NaN bit pattern) are ignored.  Both equal the reference and the on-the-fly run"""
    from baddiffusion_amd import ops
    lib, L = dev
    pr = X.conv_problem(cid, direction)
    for opset in "AB":
        d = X.problem_data(pr.key, opset)
        w = d.b[0, 0].contiguous().cuda()
        w_nan, planes = torch.full_like(w, NAN), ops.split_bf16(w)
        planes_nan = torch.full_like(planes, PLANE_NAN)
        for tile in X.TILES:
            g = X.geometry(pr, "aligned", tile)
            A, Cw = Win(g.a, d.a), Win(g.c, None)
            ws = torch.empty(max(X.workspace_bytes(pr, X.resolve_split(pr, s)[1], False) for s in pr.splits) // 4 + 64, device="cuda")
            base = dict(a=A.ptr, b=w.data_ptr(), r=0, c=Cw.ptr, bias=0, rowbias=0, colsum=0, ws=ws.data_ptr())
            for mode in X.MODES:
                for split in pr.splits:
                    forced = X.resolve_split(pr, split)[0]
                    ref = d.prod[mode == X.BF16].float().cuda()
                    out = []
                    # on the fly; then with planes: bf16 modes read them alone, BD_MODE_F32 ignores them
                    for p, s, presplit in ((w, None, False), (w_nan if mode != X.F32 else w, planes if mode != X.F32 else planes_nan, True)):
                        tag = (pr.name, f"tile {tile}", f"mode {mode}", f"set {opset}", f"ksplit {forced}", "planes" if presplit else "on the fly")
                        desc = X.make_desc(L, pr, g, base, tile, mode, forced, "plain")
                        desc.B.p, desc.B.ld, desc.B.split = p.data_ptr(), pr.b.cols, L.ptr(s)
                        want_plan = X.expected_plan(pr, "aligned", tile, mode, split, presplit=presplit)
                        desc.workspace_bytes = want_plan["workspace_bytes"]
                        assert plan_of(dev, desc) == want_plan, (tag, plan_of(dev, desc), want_plan)
                        ws.fill_(NAN); Cw.reset()
                        _, counts = bracketed(lambda: L.check(lib.bd_igemm(ctypes.byref(desc), L.stream()), "bd_igemm"))
                        want = f"igemm_{X.PROF_NAME[want_plan['cls']]}_{tile}{X.MODE_SUFFIX[mode]}"
                        assert {k: v for k, v in counts.items() if k.startswith("igemm")} == {want: 1}, (tag, counts)
                        got = Cw.take()
                        assert torch.equal(got, ref), (tag, describe(got.reshape(-1, pr.N), d.prod[mode == X.BF16].reshape(-1, pr.N)))
                        assert not Cw.changed(), (tag, "store outside the [M, N] window of C", Cw.changed())
                        out.append(got)
                    assert torch.equal(out[0], out[1])
