"""Exact-value tests for the K-split branches, the operand forms, the outputs and the strides of the split-plane GEMM (bd_gemm_sp:
csrc/gemm_sp.hip), in the manner of tests/test_conv_ps_dispatch.py.

sp_plan() splits K over workgroups when batch <= 1, tiles < CUs and K / 32 >= 32:
    ksplit = min(ceil(CUs / tiles), nch / 8),  cps = ceil(nch / ksplit),  ksplit = ceil(nch / cps)        (nch = K / 32)
Each case below pins one shape of that rule (test_case_table_follows_the_split_rule restates it; the GPU tests assert what bd_gemm_sp_plan
reports -- ksplit, chunks per slice, profiler class -- and the workspace the ABI asks for -- ksplit * (M N + M) * 4 bytes, or 0 -- before they
launch anything; tests/test_gemm_sp_plan_host.py checks the table, the rule's boundaries and the refusals without a device): a single chunk (stage 0 of the ring only), an odd chunk count, an
odd cps with a ragged last slice, nine slices (the column-sum fold's group of eight plus its tail loop), a last slice of one chunk, and a long K
under a batch, which must not split.  Every case runs in the four operand forms (K-contiguous / K-major A and B), both compute modes, both
operand sets, with fp32, fp32 + plane and plane-only outputs (c == NULL: what the QKV projection and its data gradient ask for), without and
with bias + residual + alpha + out_scale, without and with accumulate.

The operands lie on the grids of the convolution tests (wide: integers in (-2048, 2048) over 2048; narrow: {-1, -0.5, 0, 0.5, 1}; alpha 0.25,
out_scale 0.5, addends multiples of 1/4 in [-2, 2]), so every partial sum in any order is an fp32 number and the results are compared for
EQUALITY with an fp64 product; the planes for bit equality with hi = bf16 RNE(v), lo = bf16 RNE(v - hi) of that exact value.  In BD_MODE_BF16
the reference contracts the bf16-rounded operands and differs from the three-product one (asserted): equality there shows that the lo planes
were not read.  The column sums (a_colsum) keep hi + lo in both modes.  test_operand_grids_keep_every_gemm_sum_exact (no GPU) proves the
precondition for every case and set.

fp32 outputs are written into NaN-filled buffers, plane outputs into buffers pre-filled with a NaN bit pattern, both with a guard band of rows
behind the last one; the strided variant places operands and outputs as column blocks of wider buffers (ld > row length, a 32-aligned column
offset, batch strides beyond M * ld) and requires every byte outside the [M, N] windows to be unchanged.

The case table holds for 256 CUs; on another device the GPU tests skip.  Whoever retunes sp_plan() moves the cases with it (DESIGN.md,
"K split of the split-plane GEMM").

Observed on MI355X (256 CUs): every case, form, mode, set, output and epilogue combination is equal to the reference, bit for bit; no case
found a fault in gemm_sp.hip."""
import ctypes

import pytest
import torch

from tests.test_conv_ps_dispatch import EXPECTED_CUS, _check_split, _mag, _narrow, _quarters, _wide, bracketed, describe, rnd

gpu = pytest.mark.gpu       # per test: the precondition tests run without a device

BF16X3, BF16 = 1, 2
ALPHA, OUT_SCALE = 0.25, 0.5
UNIT = 2.0 ** -14           # alpha * (wide x narrow) lives on this grid; so does every epilogue addend
SENTINEL = 0x7FC1           # a bf16 NaN: a plane element nobody wrote
GUARD = 128                 # rows behind the last row of every output buffer

# id: (M, N, K, batch, ksplit, chunks per slice, chunks of the last slice, what the case is there for)
CASES = {
    "G1": (128, 128, 32, 1, 1, 1, 1, "one chunk: stage 0 of the two-stage ring only"),
    "G2": (128, 256, 160, 1, 1, 5, 5, "odd chunk count (5)"),
    "G3": (128, 128, 1056, 1, 4, 9, 6, "odd cps, ragged last slice"),
    "G4": (128, 128, 2400, 1, 9, 9, 3, "column-sum fold: one group of eight slabs plus a tail of one"),
    "G5": (256, 384, 3200, 1, 12, 9, 1, "a last slice of a single chunk; 6 tiles"),
    "G6": (128, 128, 1056, 3, 1, 33, 33, "long K with a batch: 33 chunks in one workgroup, workspace 0; B shared by the batch (b_bs = 0) and per batch"),
}
FORMS = [(False, False), (False, True), (True, False), (True, True)]
PROF_CLASS = {(False, False): "gemm_sp_nt", (False, True): "gemm_sp_nn", (True, False): "gemm_sp_tn_a", (True, True): "gemm_sp_tn"}
form_id = lambda akm, bkm: f"a{'km' if akm else 'kc'}-b{'km' if bkm else 'kc'}"
PARAMS = [pytest.param(cid, akm, bkm, s, id=f"{cid}-{form_id(akm, bkm)}-{s}") for cid in CASES for akm, bkm in FORMS for s in "AB"]
STRIDED_PARAMS = [pytest.param(cid, akm, bkm, id=f"{cid}-{form_id(akm, bkm)}") for cid in ("G2", "G3", "G6") for akm, bkm in FORMS]


def split_rule(M, N, K, batch, cus=EXPECTED_CUS):
    """the K split of sp_plan() of gemm_sp.hip, restated -> (ksplit, chunks per slice, chunks of the last slice)"""
    nch = K // 32
    tiles = (M // 128) * (N // 128) * max(batch, 1)
    ksplit = 1
    if batch <= 1 and tiles < cus and nch >= 32:
        ksplit = max(1, min(-(-cus // tiles), nch // 8))
    cps = -(-nch // ksplit)
    ksplit = -(-nch // cps)
    return ksplit, cps, nch - (ksplit - 1) * cps


def workspace_bytes(cid):
    M, N, _, _, ksplit = CASES[cid][:5]
    return ksplit * (M * N + M) * 4 if ksplit > 1 else 0


# ------------------------------------------------------------------------------------------------ operands and references (CPU)
def operands(cid, opset):
    """A [batch, M, K], B [batch, N, K] (B[0] is the shared B of the b_bs = 0 runs); set A: A wide, B narrow; set B: the reverse"""
    M, N, K, batch = CASES[cid][:4]
    g = torch.Generator().manual_seed(3000 * int(cid[1:]) + (opset == "A"))
    a_gen, b_gen = (_wide, _narrow) if opset == "A" else (_narrow, _wide)
    return dict(a=a_gen(g, batch, M, K), b=b_gen(g, batch, N, K), bias=_quarters(g, N), residual=_quarters(g, batch, M, N), prev=_quarters(g, batch, M, N))


def product64(a, b, shared):
    """fp64 A B^T per batch -> [batch, M, N]"""
    b = b[:1].expand(a.shape[0], -1, -1) if shared else b
    return a.double() @ b.double().transpose(1, 2)


def epilogue64(prod, o, epi, acc):
    y = ALPHA * prod + o["bias"].double() + o["residual"].double() if epi else prod.clone()
    if epi:
        y = y * OUT_SCALE
    return y + o["prev"].double() if acc else y


def planes(x):
    """the documented split of fp32 [..., C] -> int16 [..., C/32, 2, 32]: hi = bf16 RNE(x), lo = bf16 RNE(x - hi)  (torch, CPU)"""
    x = x.float()
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    blk = lambda t: t.view(torch.int16).reshape(*x.shape[:-1], x.shape[-1] // 32, 32)
    return torch.stack([blk(hi), blk(lo)], dim=-2).contiguous()


def plane_values(p):
    """int16 planes [..., C/32, 2, 32] -> (hi, lo) as fp32 [rows, C]"""
    f = p.contiguous().view(torch.bfloat16).float()
    return f[..., 0, :].reshape(-1, p.shape[-3] * 32), f[..., 1, :].reshape(-1, p.shape[-3] * 32)


def describe_planes(got, ref):
    (gh, gl), (rh, rl) = plane_values(got.cpu()), plane_values(ref)
    return f"hi plane: {describe(gh, rh.double())}; lo plane: {describe(gl, rl.double())}"


# ------------------------------------------------------------------------------------------------ the table and the precondition (no GPU)
@pytest.mark.parametrize("cid", list(CASES))
def test_case_table_follows_the_split_rule(cid):
    M, N, K, batch, ksplit, cps, last, _ = CASES[cid]
    assert split_rule(M, N, K, batch) == (ksplit, cps, last), (cid, split_rule(M, N, K, batch))
    assert M % 128 == 0 and N % 128 == 0 and K % 32 == 0


def test_split_rule_on_the_plans_qkv_weight_gradient():
    """the CIFAR plan's QKV weight gradient at B = 128 (M = 3C = 768, N = C = 256, K = B * 256 tokens) does not split evenly: 22 slices of
    47 chunks and a last one of 37 -- the ragged shape G3 - G5 stand for"""
    assert split_rule(768, 256, 32768, 1) == (22, 47, 37)


@pytest.mark.parametrize("cid", list(CASES))
@pytest.mark.parametrize("opset", "AB")
def test_operand_grids_keep_every_gemm_sum_exact(cid, opset):
    """alpha * max(|A| |B|^T) plus the epilogue addends stays below 2^24 units of 2^-14 (the raw accumulator below 2^24 units of 2^-12 with it),
    the column sums of A below 2^24 units of 2^-11; hi + lo == x with lo exact in bf16, and at least half of the wide values have a lo part"""
    o = operands(cid, opset)
    batch = CASES[cid][3]
    _check_split(o["a"], opset == "A"); _check_split(o["b"], opset == "B")
    units = 0.0
    for shared in ((False, True) if batch > 1 else (False,)):
        worst = ALPHA * product64(_mag(o["a"]), _mag(o["b"]), shared)
        worst += o["bias"].abs().double() + o["residual"].abs().double() + 2 * o["prev"].abs().double()   # out_scale * (...) + prev = 0.5 * (... + 2 prev)
        units = max(units, float(worst.max()) / UNIT)
    cs_units = float(o["a"].abs().double().sum(-1).max()) * 2048
    print(f"MEASURE exact_units {cid} set {opset} c {units / 2 ** 24:.4f} colsum {cs_units / 2 ** 24:.4f} x 2^24")
    assert units < 2 ** 24 and cs_units < 2 ** 24, (units, cs_units)
    for mode_prep in (lambda t: t, rnd):                        # every result, in both modes, is an fp32 number
        for epi, acc in ((False, False), (False, True), (True, False), (True, True)):
            ref = epilogue64(product64(mode_prep(o["a"]), mode_prep(o["b"]), False), o, epi, acc)
            assert torch.equal(ref.float().double(), ref)
    assert not torch.equal(product64(o["a"], o["b"], False), product64(rnd(o["a"]), rnd(o["b"]), False))


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != EXPECTED_CUS:
        pytest.skip(f"the case table is for {EXPECTED_CUS} CUs, this device reports {cus}")
    from baddiffusion_amd import _lib as L
    return L.load(), L


class Lay:
    """where a [batch][rows][cols] window sits in its buffer: `off` columns in front, `pad` behind, `rows` extra rows between two batches"""
    def __init__(self, off, pad, rows):
        self.off, self.pad, self.rows = off, pad, rows


DENSE, STRIDED = Lay(0, 0, 0), Lay(32, 64, 8)


class Buf:
    """A window [batch][rows][cols] of fp32 values or of split planes inside a buffer filled with NaN / the sentinel, GUARD rows behind the last."""
    def __init__(self, planes_, batch, rows, cols, lay, value=None, shared=False):
        self.is_planes, self.batch, self.rows = planes_, batch, rows
        self.ld = lay.off + cols + lay.pad
        self.per = rows + lay.rows
        self.bs = 0 if shared else self.per * self.ld
        total = batch * self.per + GUARD
        if planes_:
            self.full = torch.full((total, self.ld // 32, 2, 32), SENTINEL, dtype=torch.int16, device="cuda")
            self.cols = slice(lay.off // 32, (lay.off + cols) // 32)
        else:
            self.full = torch.full((total, self.ld), float("nan"), device="cuda")
            self.cols = slice(lay.off, lay.off + cols)
        self.win = self.window(self.full)
        if value is not None:
            self.win.copy_(value.cuda())
        self.init = self.full.clone()
        self.ptr = self.win.data_ptr()

    def window(self, full):
        return full[: self.batch * self.per].view(self.batch, self.per, *full.shape[1:])[:, : self.rows, self.cols]

    def outside_changes(self):
        """"" when every element outside the window -- padding columns, rows between batches, the guard band -- has the bits it started with;
        otherwise where the buffer changed: rows of the whole buffer (batch b starts at row b * (rows + gap)), columns in elements of a buffer
        row (planes: 64 int16 per 32-column block, hi then lo), differences in units of the bit patterns"""
        chk = self.full.clone()
        self.window(chk).copy_(self.window(self.init))
        bits = (lambda t: t.reshape(t.shape[0], -1)) if self.is_planes else (lambda t: t.view(torch.int32))
        if torch.equal(bits(chk), bits(self.init)):
            return ""
        return describe(bits(chk), bits(self.init).double().cpu())


def launch(dev, cid, a, akm, b, bkm, mode, c=None, cs=None, bias=None, res=None, alpha=1.0, out_scale=1.0, accumulate=False, colsum=None):
    lib, L = dev
    M, N, K, batch, ksplit, cps = CASES[cid][:6]
    d = L.GemmSpDesc(M=M, N=N, K=K, batch=batch, a=a.ptr, lda=a.ld, a_bs=a.bs, a_kmajor=int(akm), b=b.ptr, ldb=b.ld, b_bs=b.bs, b_kmajor=int(bkm),
                     alpha=alpha, out_scale=out_scale, accumulate=int(accumulate), bias=L.ptr(bias), a_colsum=L.ptr(colsum), mode=mode)
    if c is not None:
        d.c, d.ldc, d.c_bs = c.ptr, c.ld, c.bs
    if cs is not None:
        d.c_split, d.ldcs, d.cs_bs = cs.ptr, cs.ld, cs.bs
    if res is not None:
        d.residual, d.ldr, d.r_bs = res.ptr, res.ld, res.bs
    info = L.GemmSpPlanInfo()                                                # the branch, before anything is launched
    L.check(lib.bd_gemm_sp_plan(ctypes.byref(d), ctypes.byref(info)), "bd_gemm_sp_plan")
    want_class = PROF_CLASS[(akm, bkm)] + ("_bf16" if mode == BF16 else "")
    assert (info.ksplit, info.chunks_per_split, info.prof_class.decode()) == (ksplit, cps, want_class), ("plan", cid, info.ksplit, info.chunks_per_split, info.prof_class)
    need = lib.bd_gemm_sp_workspace_bytes(ctypes.byref(d))
    assert need == workspace_bytes(cid) == info.workspace_bytes, ("workspace", need, workspace_bytes(cid), info.workspace_bytes)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    d.workspace, d.workspace_bytes = (ws.data_ptr(), need) if need else (None, 0)
    L.check(lib.bd_gemm_sp(ctypes.byref(d), L.stream()), "bd_gemm_sp")


def check_case(dev, cid, akm, bkm, opset, lay, combos, profile):
    """run the case in both modes; combos: (outputs in {"f32", "both", "planes"}, epilogue?, accumulate?)"""
    M, N, K, batch = CASES[cid][:4]
    o = operands(cid, opset)
    refs = {}
    for shared in ((False, True) if batch > 1 else (False,)):
        a_cpu = o["a"].transpose(1, 2) if akm else o["a"]
        b_cpu = o["b"][:1] if shared else o["b"]
        b_cpu = b_cpu.transpose(1, 2) if bkm else b_cpu
        a = Buf(True, batch, a_cpu.shape[1], a_cpu.shape[2], lay, planes(a_cpu.contiguous()))
        b = Buf(True, b_cpu.shape[0], b_cpu.shape[1], b_cpu.shape[2], lay, planes(b_cpu.contiguous()), shared=shared)
        res = Buf(False, batch, M, N, lay, o["residual"])
        bias = o["bias"].cuda()
        for mode in (BF16X3, BF16):
            tag = (cid, form_id(akm, bkm), opset, "bf16" if mode == BF16 else "bf16x3", "shared B" if shared else "")
            prep = rnd if mode == BF16 else (lambda t: t)
            prod = refs[mode] = product64(prep(o["a"]), prep(o["b"]), shared)
            plane_bits = {}
            for n_run, (outs, epi, acc) in enumerate(combos):
                ref = epilogue64(prod, o, epi, acc)
                c = Buf(False, batch, M, N, lay, o["prev"] if acc else None) if outs != "planes" else None
                cs = Buf(True, batch, M, N, lay) if outs != "f32" else None
                run = lambda: launch(dev, cid, a, akm, b, bkm, mode, c=c, cs=cs, bias=bias if epi else None, res=res if epi else None,
                                     alpha=ALPHA if epi else 1.0, out_scale=OUT_SCALE if epi else 1.0, accumulate=acc)
                if profile and n_run == 0 and not shared:
                    _, counts = bracketed(run)
                    want = PROF_CLASS[(akm, bkm)] + ("_bf16" if mode == BF16 else "")
                    assert {k: v for k, v in counts.items() if k.startswith("gemm_sp")} == {want: 1}, (tag, counts)
                else:
                    run()
                what = tag + (outs, "epilogue" if epi else "plain", "accumulate" if acc else "")
                if c is not None:
                    got = c.win.double().cpu()
                    assert torch.equal(got, ref), (what, "fp32", describe(got.reshape(-1, N), ref.reshape(-1, N)))
                    assert not c.outside_changes(), (what, "fp32 store outside the [M, N] window", c.outside_changes())
                if cs is not None:
                    got, want_pl = cs.win.cpu(), planes(ref)
                    assert torch.equal(got, want_pl), (what, "planes", describe_planes(got, want_pl))
                    assert not cs.outside_changes(), (what, "plane store outside the [M, N] window", cs.outside_changes())
                    if not acc:          # the planes-only run gives the bits of the fp32 + planes run
                        other = plane_bits.setdefault(epi, got)
                        assert torch.equal(got, other), (what, "planes-only against fp32 + planes", describe_planes(got, other))
            for name, buf in (("a", a), ("b", b), ("residual", res)):
                assert not buf.outside_changes(), (cid, form_id(akm, bkm), opset, "an input buffer changed", name, buf.outside_changes())
    assert not torch.equal(refs[BF16X3], refs[BF16])      # the two modes have different answers: bf16 equality => lo planes unread


ALL_COMBOS = [(outs, epi, acc) for epi in (False, True) for outs in ("both", "f32", "planes") for acc in ((False, True) if outs != "planes" else (False,))]


@gpu
@pytest.mark.parametrize("cid,akm,bkm,opset", PARAMS)
def test_gemm_sp_branch_is_exact(dev, cid, akm, bkm, opset):
    """bd_gemm_sp on the pinned K-split branch equals the fp64 product in both modes: fp32, fp32 + planes and planes-only outputs, plain and
    with bias + residual + alpha + out_scale, without and with accumulate; one profiling class counts one launch"""
    check_case(dev, cid, akm, bkm, opset, DENSE, ALL_COMBOS, profile=True)


@gpu
@pytest.mark.parametrize("cid,opset", [pytest.param(cid, s, id=f"{cid}-{s}") for cid, c in CASES.items() if c[3] == 1 for s in "AB"])
def test_gemm_sp_column_sums_are_exact(dev, cid, opset):
    """a_colsum (both operands K-major, no batch) equals the fp64 row sums of the UNROUNDED A in both modes -- through the slab fold of
    gemm_sp_colsum_reduce when K splits (G4: eight slabs and a tail of one) -- and asking for it leaves c as it was"""
    M, N, K, batch = CASES[cid][:4]
    o = operands(cid, opset)
    a = Buf(True, 1, K, M, DENSE, planes(o["a"].transpose(1, 2).contiguous()))
    b = Buf(True, 1, K, N, DENSE, planes(o["b"].transpose(1, 2).contiguous()))
    sum_ref = o["a"][0].double().sum(1)
    for mode in (BF16X3, BF16):
        prep = rnd if mode == BF16 else (lambda t: t)
        ref = product64(prep(o["a"]), prep(o["b"]), False)
        c0, c1 = Buf(False, 1, M, N, DENSE), Buf(False, 1, M, N, DENSE)
        colsum = torch.full((M + 64,), float("nan"), device="cuda")
        launch(dev, cid, a, True, b, True, mode, c=c0)
        launch(dev, cid, a, True, b, True, mode, c=c1, colsum=colsum)
        got = colsum[:M].double().cpu()
        assert torch.equal(got, sum_ref), (cid, opset, mode, "a_colsum", describe(got[None], sum_ref[None]))
        assert bool(torch.isnan(colsum[M:]).all()), (cid, opset, mode, "a_colsum store past M")
        got = c1.win.double().cpu()
        assert torch.equal(got, ref), (cid, opset, mode, "c with a_colsum", describe(got.reshape(-1, N), ref.reshape(-1, N)))
        assert torch.equal(c1.full.view(torch.int32), c0.full.view(torch.int32)), (cid, opset, mode, "c changed by asking for a_colsum")


@gpu
@pytest.mark.parametrize("cid,akm,bkm", STRIDED_PARAMS)
def test_gemm_sp_strided_windows(dev, cid, akm, bkm):
    """operands, residual and outputs as column blocks of wider buffers (lda / ldb / ldc / ldcs / ldr beyond the row length, a column offset
    of 32, batch strides beyond M * ld): the same exact results, and nothing outside the [M, N] windows is touched"""
    combos = [("both", True, True), ("planes", True, False), ("f32", False, False), ("both", False, False), ("planes", False, False)]
    for opset in "AB":
        check_case(dev, cid, akm, bkm, opset, STRIDED, combos, profile=False)
