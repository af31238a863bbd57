"""Exact-value tests for every dispatch branch of the thin 3x3 convolutions (csrc/conv_thin.hip behind bd_conv3x3_fwd / _dgrad / _wgrad: conv_in,
3 or 1 -> C channels, and conv_out, C -> 3 or 1), in the manner of tests/test_igemm_dispatch.py.

The host code picks one of nine kernels -- expand on FMAs or on the matrix pipe, contract, contract-dgrad, and for the weight gradients the
matrix-pipe, wave-per-row and two general kernels -- or hands the call to igemm.  The table in tests/_thin_exact.py pins each of those
branches, every template instantiation (J = 3 and J = 1), and every multi-pass loop (iters, segs_per_wave, steps_per_wg, pix_per_block > 128).
Before a case launches anything it asserts from bd_conv3x3_*_plan the path, J, loop count, grid, pix_per_block, partial rows and workspace
bytes the table states (tests/test_thin_plan_host.py asserts the same without a device); after the launch the profiler must have counted
exactly one launch of the class the plan named and nothing else -- the thin weight gradients have no class, so nothing at all; a call that
fell to igemm exactly one igemm_* launch.

Every comparison is an EQUALITY with an fp64 reference -- F.conv2d and its autograd on the CPU, NHWC in and out -- rounded to fp32; there is
no tolerance in this file.  The operands lie on the grids of the sibling files: a wide operand holds integers in (-den, den) over den (2048;
coarser where a weight gradient sums over many pixels: 1024 for W3, 512 for W4, 64 for W7), a narrow one {-1, -0.5, 0, 0.5, 1}; set A has the
activations (x; for the weight gradients x) wide and the weights (dy) narrow, set B the reverse; bias in multiples of 1/4 in [-2, 2],
out_scale 0.5 -- so every partial sum in any order is an fp32 number (test_operand_grids_keep_every_thin_sum_exact).  BD_MODE_F32 and
BD_MODE_BF16X3 are compared with the product of the operands as given.  BD_MODE_BF16 runs the same three-product kernels on the thin paths,
so it must ALSO equal the unrounded product -- which differs from the product of the bf16-rounded operands (asserted, so the statement is
live; W7's 6-bit grid is the exception) -- and where a case falls to igemm in BD_MODE_BF16 the rounded-operand reference holds instead.
db is compared with the fp64 sums of the unrounded dy.

Layouts:
  * aligned: every pixel tensor -- the 3- and 1-channel ones included -- is a column block (offset 8 floats, ld % 4 == 0, ld > C) of a wider
    NaN-filled buffer with 72 guard rows in front and behind; the weights, the bias, dw and db begin 8 floats into NaN-filled arrays.  An
    output must leave every bit outside its window unchanged, inputs every bit.  The workspace is NaN-filled before each launch.  The weight
    gradients run with db and, a second time, with db = NULL; F2 also without bias;
  * mis: the C-channel tensor sits one float off.  The plan must name the fallback -- igemm for the forward and data-gradient paths, the
    general kernel instead of the row kernel in BD_MODE_F32, the unchanged matrix-pipe kernel (scalar loads) in the bf16 modes -- and the
    results must be equal;
  * narrow3: the J-channel tensor contiguous (ld == J) behind an odd offset: nothing changes.
The three cases of 131072 pixels and more (F5, G4, W7) build their batch from two base images, each scaled per image by +-1 or +-0.5; the
fp64 reference is computed for the two images and scaled, which stays exact.  They run in the aligned layout only.  Nothing else of the
table is thinned.

Whoever retunes the guards moves the cases with them ("Dispatch branches of the thin convolutions").

Observed on MI355X: every case, layout, mode, operand set and bias / db variant is equal to the reference, bit for bit; db likewise; no store
outside an output window, no input changed; every launch took the path the plan named and was counted once under its class.  No case found a
wrong result in conv_thin.hip, so no kernel body changed.  The two host findings this work settles are pinned in tests/test_thin_plan_host.py:
the weight-gradient launcher demanded the 1024 rows of the general kernels whichever kernel ran (more than bd_conv3x3_workspace_bytes for
3 x 512 channels at 131072 pixels and more), and the contract forward read w as float2 without a guard on its alignment.  The comparisons are
live: against a library built from a scratch copy with one border mask dropped per kernel -- the column mask of thin_expand_kernel,
thin_contract_kernel, wgrad_thin_mfma_kernel and wgrad_thin_row_kernel, the row mask of thin_expand_mfma_kernel and
thin_contract_dgrad_kernel -- with pad_t ignored in wgrad_thin_cin_kernel and a dead pixel slot of wgrad_thin_cout_kernel repeating the live one
(every read stays inside the image), 57 of the 99 runs fail: F1 - F7, G1 - G7 and W1 - W4 in the aligned and narrow3 layouts (W1 - W3 also in
mis, where the bf16 modes keep the matrix-pipe kernel), W8-in (pad 0) and W5-out / W5j1-out (41-pixel last tile) in all three.  What passes is
what those defects cannot reach: the igemm cases F8 - F10 and G8, every mis run that falls to igemm, W4-mis (general kernels at pad 1 with
whole tiles), W5-in, W5j1-in, W6-in and W7-in (wgrad_thin_cin_kernel at pad 1), W6-out and W8-out (whole tiles and a 48-pixel tail leave no
dead slot)."""
import ctypes

import pytest
import torch

from tests import _thin_exact as X
from tests.test_conv_ps_dispatch import bracketed, describe

gpu = pytest.mark.gpu
NAN = float("nan")
BAND = 8            # floats in front of and behind the flat arrays (w, bias, dw, db)

PARAMS = [pytest.param(n, lay, id=f"{n}-{lay}") for n, c in X.CASES.items() for lay in c.layouts]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from baddiffusion_amd import _lib as L
    lib = L.load()
    ws = torch.empty(lib.bd_conv3x3_workspace_bytes(0, 0, 0, 0, 0, 0, 0, 0) // 4, device="cuda")
    return lib, L, ws


class Win:
    """a [rows][cols] window (tests/_thin_exact.py geo) of a flat NaN-filled buffer"""
    def __init__(self, g, value=None, keep=True):
        self.flat = torch.full((g.total,), NAN, device="cuda")
        self.win = self.flat.as_strided((g.rows, g.cols), (g.ld, 1), g.front)
        if value is not None:
            self.win.copy_(value.reshape(g.rows, g.cols))
        self.init = self.flat.clone() if keep else None
        self.ptr = self.flat.data_ptr()

    def reset(self, value=None):
        self.flat.copy_(self.init)
        if value is not None:
            self.win.copy_(value.reshape(self.win.shape))

    def take(self):
        """the window's content; the window is then NaN again"""
        got = self.win.clone()
        self.win.fill_(NAN)
        return got

    def changed(self):
        """"" when the buffer has the bits it started with (an output: outside its window, after take())"""
        a, b = self.flat.view(torch.int32), self.init.view(torch.int32)
        return "" if torch.equal(a, b) else describe(a[None], b[None].double().cpu())


def band(n, value=None):
    """a flat array of n floats inside a NaN-filled band -> Win"""
    return Win(X.NS(rows=1, cols=n, ld=n, front=BAND, total=BAND + n + BAND), value)


def plan_of(dev, c, d):
    lib, L, _ = dev
    p = L.ThinPlanInfo()
    L.check(getattr(lib, f"bd_conv3x3_{c.kind}_plan")(ctypes.byref(d), ctypes.byref(p)), "plan")
    return {f: getattr(p, f) for f in X.PLAN_FIELDS}


def check_case(dev, c, layout):
    lib, L, ws = dev
    g = X.geometry(c, layout)
    px, n_w = c.B * c.H * c.W, c.Cout * 9 * c.Cin
    for opset in "AB":
        d = X.case_data(c.name, opset)
        live = c.den > 256
        assert torch.equal(d.prod[False], d.prod[True]) != live        # BD_MODE_BF16 on rounded operands has another answer
        a, b = X.full_a(d, "cuda"), X.full_b(d, "cuda")
        names = {"fwd": ("x", "w", "y"), "dgrad": ("dy", "w", "dx"), "wgrad": ("x", "dy", "dw")}[c.kind]
        A = Win(getattr(g, names[0]), a, keep=not c.big)
        del a
        if c.kind == "wgrad":
            Bw, out, dbw = Win(g.dy, b, keep=not c.big), band(n_w), band(c.Cout)
            db_ref = X.db64(d).float().cuda()
        else:
            Bw, out, dbw = band(n_w, b), Win(getattr(g, names[2])), None
        bias = band(c.Cout, d.bias.cuda())
        prev = d.prev.cuda()[d.idx.cuda()] if c.accumulate else None
        base = {names[0]: A.ptr, names[1]: Bw.ptr, names[2]: out.ptr, "bias": bias.ptr, "db": dbw.ptr if dbw else 0,
                "ws": ws.data_ptr()}
        variants = [True, False] if c.kind == "wgrad" or c.nobias else [True]          # bias (forward) / db (weight gradient) present
        refs = {(r, v): X.compose64(d, d.prod[r].cuda(), bias=v).float() for r in (False, True) for v in (variants if c.kind == "fwd" else [True])}
        for mode in c.modes:
            want = X.expected_plan(c, layout, mode)
            thin = want["path"] != X.IGEMM
            for opt in variants:
                tag = (c.name, layout, f"mode {mode}", f"set {opset}", X.PATH_NAME[want["path"]], f"bias/db {opt}")
                desc = X.make_desc(L, c, g, base, mode, bias=opt, db=opt)
                desc.workspace_bytes = want["workspace_bytes"] if thin and c.kind == "wgrad" else ws.numel() * 4
                got_plan = plan_of(dev, c, desc)
                assert got_plan == want, (tag, got_plan, want)                             # the branch, before the launch
                ws.fill_(NAN)
                out.reset(prev)
                if dbw:
                    dbw.reset()
                _, counts = bracketed(lambda: L.check(getattr(lib, f"bd_conv3x3_{c.kind}")(ctypes.byref(desc), L.stream()), "bd_conv3x3"))
                if thin:
                    assert counts == ({want["prof_class"].decode(): 1} if want["prof_class"] else {}), (tag, counts)
                else:
                    assert all(k.startswith("igemm") for k in counts) and sum(counts.values()) == 1, (tag, counts)
                ref = refs[(not thin and mode == X.BF16, opt if c.kind == "fwd" else True)]
                got = out.take().reshape(ref.shape)
                if not torch.equal(got, ref):
                    raise AssertionError((tag, describe(got.reshape(-1, got.shape[-1]), ref.double().cpu().reshape(-1, ref.shape[-1]))))
                assert not out.changed(), (tag, "store outside the output window", out.changed())
                if dbw:
                    got_db = dbw.take().flatten()
                    if opt:
                        assert torch.equal(got_db, db_ref), (tag, "db", describe(got_db[None], X.db64(d)[None]))
                    else:
                        assert bool(torch.isnan(got_db).all()), (tag, "db written though NULL was passed")       # (it cannot be: a guard for the harness itself)
                    assert not dbw.changed(), (tag, "store outside db", dbw.changed())
        if not c.big:
            for name, w in ((names[0], A), (names[1], Bw), ("bias", bias)):
                assert not w.changed(), (c.name, layout, opset, "an input buffer changed", name, w.changed())
        del A, Bw, out, refs
    torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("name,layout", PARAMS)
def test_thin_branch_is_exact(dev, name, layout):
    """one case of the table in one layout: every mode of the case, both operand sets, with and without bias / db where the table says so --
    the planned path, one profiler class counted once, equal to the fp64 reference, nothing written outside the output windows"""
    check_case(dev, X.CASES[name], layout)
