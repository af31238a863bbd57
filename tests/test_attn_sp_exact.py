"""Exact-value and edge tests for the attention core on split planes (bd_attn_sp_fwd / bd_attn_sp_bwd: csrc/attn_sp.hip), N = 256 tokens,
head dim 256, scale 1/16, (B, heads) in {(1, 1), (3, 2)}, both compute modes.

(a), (b)  Structured softmax.  Since dh = N the keys can be the standard basis: k_j = e_j, q_i = 4096 * sum_{j in T(i)} e_j.  The logits are
exactly 256 on T(i) and 0 elsewhere, exp(-256) is 0 in fp32, so P_ij = 1 / |T(i)| on T(i) and exactly 0 elsewhere -- the max subtraction, rows
owned by one key or shared by 2 / 4, and the permuted contraction index of phase O all act on a P with structure.  None of q, k, P has a lo
part; V is wide with dO narrow (set V) or the reverse (set D), on the grids of tests/test_conv_ps_dispatch.py, so every product and partial sum
is an fp32 number and every output is compared for BIT equality with the split (hi = bf16 RNE(v), lo = bf16 RNE(v - hi)) of an fp64 reference
that follows the kernels' data flow:
    dP = dO V^T;  dS = P o (dP - rowsum(P o dP));  dst = planes of scale * dS^T;  dQ = [scale dS] K,  dK = [scale dS]^T Q,  dV = P^T dO
where [scale dS] is hi + lo of the dst split (hi alone in BD_MODE_BF16), and BD_MODE_BF16 contracts the bf16-rounded V and dO.  The only
licence taken: in the dS^T planes and in the dq | dk columns derived from them a zero may carry either sign (dS = scale * 0 * (dP - delta) is -0
where dP < delta), so 0x8000 and 0x0000 compare equal there; O, P^T and dv are compared bit for bit with no licence.
  (a) T(i) = {pi(i)}: a permutation that is no involution and crosses wave blocks, key tiles and the two 128-row blocks (another per head
      and sample), and a many-to-one map (some keys get three queries, some none): O_i = V_pi(i), P^T is the 0/1 matrix, dV a pure
      scatter-add, dS, dQ, dK and the dst planes exactly zero.
  (b) |T(i)| = 2 (even rows) or 4 (odd rows), the tied keys in different key tiles and 128-blocks: O_i is the exact mean; dS, dQ, dK are not zero.
test_structured_cases_are_exact (no GPU) proves that every value the kernels round or accumulate on these inputs is exactly representable, or
is rounded by the reference in the same way.
Observed on MI355X: (a) and (b) hold bit for bit, both modes, both sets, both (B, heads): the device's exp2 and reciprocal return exactly 1,
1/2 and 1/4 here.

(c) Large exact logits: q = 64 * narrow, k narrow, so every logit is an integer with a spread of several tens (beyond +-88.7 for the seed,
asserted without a GPU); V, dO randn; forward and backward against fp64 at the bounds of test_attention_core_on_split_planes (5e-5 forward and
P^T, 1e-4 gradients), nothing NaN or Inf.
(d) Single-pass backward on randn against the reference that rounds q, k, v, dO and the matrix operands P and scale * dS to bf16: the
counterpart of test_attn_sp_forward_against_rounded_operands (tests/test_bf16_mode.py).
(e) Row strides ld = 3C + 64, ldo = lddo = C + 32, lddqkv = 3C + 64: bit-identical to the dense run, padding columns and the guard band unchanged.

Where BD_MODE_BF16 "rounds P": P enters O = P V and dV = P^T dO as its hi plane; the element-wise dS = P o (dP - delta) of backward A reads
hi + lo of the P^T planes in both modes, and so does the reference.

Every output is written into a buffer pre-filled with a NaN bit pattern, with a guard band of rows behind the last one.
No case found a fault in attn_sp.hip."""
import ctypes
import functools

import pytest
import torch

from tests.test_conv_ps_dispatch import _check_split, _mag, _narrow, _wide, rnd
from tests.test_gemm_sp_dispatch import DENSE, Buf, Lay, describe_planes, plane_values, planes

gpu = pytest.mark.gpu       # per test: the precondition tests run without a device

BF16X3, BF16 = 1, 2
N = DH = 256
SCALE = 1.0 / 16
QL = 4096.0                 # q = QL * indicator: logits QL * SCALE = 256 on T(i)
SHAPES = [(1, 1), (3, 2)]
MULT, ADD = (37, 91), (11, 3)      # pi(i) = (MULT[head] * i + ADD[head] + 17 * sample) mod 256: odd multipliers, so permutations

# Single-pass backward error against the rounded fp64 reference, measured on MI355X (B = 2, one head, randn; the three-product run of the same
# inputs is at 3.3e-3 - 4.0e-3).  dq and dk contract the bf16-ROUNDED scale * dS: where the device's fp32 dS and the reference's fp64 dS fall on
# two sides of a rounding boundary one operand moves by a bf16 ulp, which puts these two an order above dS^T and dv.  Held to 3x each
# (also recorded beside TOL_ATTN in tests/test_bf16_mode.py and in DESIGN.md).
MEASURED_BWD = {"dst": 2.752e-06, "dq": 3.779e-05, "dk": 3.816e-05, "dv": 2.447e-06}
TOL_ATTN_BWD = {k: 3 * v for k, v in MEASURED_BWD.items()}


# ------------------------------------------------------------------------------------------------ layout helpers (CPU)
def relerr(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _pair(name, got1, got3, ref, bound):
    """the convention of tests/test_bf16_mode.py: single pass at the accumulation level; three products >= 10x further from the rounded reference"""
    e1, e3 = relerr(got1, ref), relerr(got3, ref)
    print(f"MEASURE {name} bf16 {e1:.3e} bf16x3 {e3:.3e}")
    assert e1 < bound, (name, e1)
    assert e3 > 10 * e1, (name, e1, e3)


def rows_of(x, B, heads):
    """[B*heads, N, dh] -> [B*N, heads*dh]"""
    return x.view(B, heads, N, DH).permute(0, 2, 1, 3).reshape(B * N, heads * DH)


def canon(p):
    """plane bits with -0 turned into +0"""
    return torch.where(p == -32768, torch.zeros_like(p), p)


def split_sum(x, hi_only):
    """the value the kernels contract for an fp32 x that went through the plane split: hi + lo, or hi alone (single pass), as fp64"""
    x = x.float()
    hi = rnd(x)
    return hi.double() if hi_only else hi.double() + rnd(x - hi).double()


# ------------------------------------------------------------------------------------------------ the fp64 reference
def reference(q, k, v, do, P, mode):
    """q, k, v, do: fp32 [BH, N, dh]; P: fp64 [BH, N, N].  Follows the kernels' data flow (module docstring) -> dict of fp64 tensors"""
    sp = mode == BF16
    r = (lambda t: rnd(t).double()) if sp else (lambda t: t.double())
    qm, km, vm, dom = r(q), r(k), r(v), r(do)
    Pm = split_sum(P, sp)                                   # P as a matrix operand: its plane split
    Pe = split_sum(P, False)                                # P in the element-wise dS: hi + lo of the P^T planes, in both modes
    out = {"o": Pm @ vm, "pt": P.transpose(1, 2)}
    dP = dom @ vm.transpose(1, 2)
    delta = (Pe * dP).sum(-1, keepdim=True)
    dSs = SCALE * Pe * (dP - delta)
    out.update(dP=dP, delta=delta, dSs=dSs, dst=dSs.transpose(1, 2))
    dSr = split_sum(dSs, sp)
    out.update(dSr=dSr, dq=dSr @ km, dk=dSr.transpose(1, 2) @ qm, dv=Pm.transpose(1, 2) @ dom)
    return out


@functools.lru_cache(maxsize=None)
def structured_case(kind, B, heads, opset):
    """kind: "perm", "many" (case a) or "ties" (case b) -> operands [BH, N, dh] fp32, the indicator of T, P and the references per mode"""
    BH = B * heads
    i = torch.arange(N)
    ind = torch.zeros(BH, N, N)
    for bh in range(BH):
        b, hd = divmod(bh, heads)
        p = (MULT[hd] * i + ADD[hd] + 17 * b) % N
        if kind == "perm":
            ind[bh, i, p] = 1
        elif kind == "many":
            ind[bh, i, p - p % 3] = 1
        else:
            ind[bh, i, p] = 1; ind[bh, i, p ^ 0xA0] = 1                     # the other 128-block, another key tile
            odd = i[1::2]
            ind[bh, odd, p[1::2] ^ 0x20] = 1; ind[bh, odd, p[1::2] ^ 0x80] = 1
    g = torch.Generator().manual_seed(100 * B + 10 * heads + (opset == "V") + 7 * len(kind))
    v_gen, do_gen = (_wide, _narrow) if opset == "V" else (_narrow, _wide)
    c = dict(ind=ind, q=QL * ind, k=torch.eye(N).expand(BH, N, N).contiguous(), v=v_gen(g, BH, N, DH), do=do_gen(g, BH, N, DH),
             P=ind.double() / ind.double().sum(-1, keepdim=True))
    c["ref"] = {mode: reference(c["q"], c["k"], c["v"], c["do"], c["P"], mode) for mode in (BF16X3, BF16)}
    return c


STRUCT_PARAMS = [pytest.param(kind, B, heads, s, id=f"{kind}-B{B}h{heads}-{s}") for kind in ("perm", "many", "ties") for B, heads in SHAPES for s in "VD"]


def _is_f32(x):
    return torch.equal(x.float().double(), x)


def _on_grid(x, unit):
    return torch.equal((x / unit).round() * unit, x)


@pytest.mark.parametrize("kind,B,heads,opset", STRUCT_PARAMS)
def test_structured_cases_are_exact(kind, B, heads, opset):
    """every value the kernels round or accumulate on the structured inputs is exact, or the reference rounds it in the same way"""
    c = structured_case(kind, B, heads, opset)
    ind, P = c["ind"], c["P"]
    sizes = ind.sum(-1)
    assert set(sizes.unique().tolist()) == ({1.0} if kind != "ties" else {2.0, 4.0})
    if kind == "perm":
        pi = ind[0].argmax(-1)
        assert bool((ind.sum(1) == 1).all()) and not torch.equal(pi[pi], torch.arange(N))          # a permutation, no involution
        blocks = lambda w: bool(((torch.arange(N) // w) != (pi // w)).any())
        assert blocks(32) and blocks(128)
    if kind == "many":
        assert int(ind.sum(1).max()) >= 3 and int(ind.sum(1).min()) == 0                              # keys with several queries, keys with none
    if kind == "ties":
        keys = [ind[0, r].nonzero().flatten() for r in range(N)]
        assert all(len(set((t // 32).tolist())) == len(t) and len(set((t // 128).tolist())) == 2 for t in keys)
    # logits: exactly 256 on T(i), 0 elsewhere; exp(-256) is 0 in fp32; q, k, P have no lo part
    logits = SCALE * c["q"].double() @ c["k"].double().transpose(1, 2)
    assert torch.equal(logits, 256 * ind.double()) and float(torch.exp(torch.tensor(-256.0))) == 0.0
    for t in (c["q"], c["k"], P.float()):
        _check_split(t, False)
    _check_split(c["v"], opset == "V"); _check_split(c["do"], opset == "D")
    head = {}
    for mode in (BF16X3, BF16):
        r = c["ref"][mode]
        vmag, domag = _mag(c["v"]).double(), _mag(c["do"]).double()
        # partial sums, in any order, in units of each accumulator's grid
        head["dP"] = float((domag @ vmag.transpose(1, 2)).max()) / 2.0 ** -12
        head["delta"] = float((P * r["dP"].abs()).sum(-1).max()) / 2.0 ** -14
        head["o"] = float((P @ vmag).max()) / 2.0 ** -13
        head["dv"] = float((P.transpose(1, 2) @ domag).max()) / 2.0 ** -13
        hi = rnd(r["dSs"].float()).double(); lo = rnd(r["dSs"].float() - hi.float()).double()
        head["dk"] = float(((hi.abs() + lo.abs()).transpose(1, 2) @ ind.double()).max()) / 2.0 ** -20    # x QL = 2^12: a shift
        assert all(u < 2 ** 24 for u in head.values()), head
        assert _on_grid(r["dP"], 2.0 ** -12) and _on_grid(r["delta"], 2.0 ** -14) and _on_grid(r["dSs"], 2.0 ** -20)
        assert _on_grid(hi, 2.0 ** -20) and _on_grid(lo, 2.0 ** -20)
        assert float(r["dSs"].abs().max()) < 16                                                            # < 2^24 units of 2^-20: an fp32 number
        # dQ has one nonzero term per element (K is the identity); every value before a split is an fp32 number
        assert torch.equal(r["dq"], r["dSr"])
        for name in ("o", "pt", "dP", "delta", "dSs", "dSr", "dq", "dk", "dv"):
            assert _is_f32(r[name]), name
        if kind != "ties":
            assert not bool(r["dSs"].any()) and not bool(r["dq"].any()) and not bool(r["dk"].any())
            src = ind.argmax(-1)
            vm = rnd(c["v"]).double() if mode == BF16 else c["v"].double()
            assert torch.equal(r["o"], torch.stack([vm[bh, src[bh]] for bh in range(B * heads)]))          # O_i = V_pi(i)
        else:
            assert float((r["dSs"] != 0).double().mean()) > 0.005 and bool(r["dk"].any())
    print(f"MEASURE exact_units {kind} B{B}h{heads} set {opset} " + " ".join(f"{k} {u / 2 ** 24:.4f}" for k, u in head.items()) + " x 2^24")
    wide = "o" if opset == "V" else "dv"                  # the output that contracts the wide operand has another answer per mode:
    assert not torch.equal(c["ref"][BF16X3][wide], c["ref"][BF16][wide])       # equality in bf16 mode => its lo plane was not read


@functools.lru_cache(maxsize=None)
def large_logit_case(B, heads):
    g = torch.Generator().manual_seed(40 + 10 * B + heads)
    BH = B * heads
    return dict(q=64 * _narrow(g, BH, N, DH), k=_narrow(g, BH, N, DH), v=torch.randn(BH, N, DH, generator=g), do=torch.randn(BH, N, DH, generator=g))


@pytest.mark.parametrize("B,heads", SHAPES)
def test_large_logits_are_exact_and_wide(B, heads):
    c = large_logit_case(B, heads)
    logits = SCALE * c["q"].double() @ c["k"].double().transpose(1, 2)
    assert _on_grid(logits, 1.0 / 16) and _is_f32(logits)
    _check_split(c["q"], False); _check_split(c["k"], False)
    print(f"MEASURE large_logits B{B}h{heads} min {float(logits.min())} max {float(logits.max())} row spread >= {float((logits.max(-1).values - logits.min(-1).values).min())}")
    assert float(logits.max()) > 88.7 and float(logits.min()) < -88.7


# ------------------------------------------------------------------------------------------------ refusals (no GPU)
ERR_INVALID, ERR_UNSUPPORTED = -1, -2
FAKE = [0x40000000 * (i + 1) for i in range(6)]      # 128-byte aligned addresses, never dereferenced: every call below is turned away
SHAPE_TEXT = b"%s: needs N == 256 and head dim 256 (got N %d, dh %d)"
QKV_TEXT = b"%s: qkv planes must be 128-byte aligned with a row stride >= 3C, multiple of 32"
FWD, BWD = b"bd_attn_sp_fwd", b"bd_attn_sp_bwd"
# (entry points, fields changed on a good descriptor of B = 2, heads = 2: C = 512, status, message with the entry point's name left out)
ATTN_REFUSALS = [
    ((FWD, BWD), dict(N=128), ERR_UNSUPPORTED, SHAPE_TEXT.replace(b"%d, dh %d", b"128, dh 256")),
    ((FWD, BWD), dict(dh=64), ERR_UNSUPPORTED, SHAPE_TEXT.replace(b"%d, dh %d", b"256, dh 64")),
    ((FWD, BWD), dict(B=0), ERR_UNSUPPORTED, SHAPE_TEXT.replace(b"%d, dh %d", b"256, dh 256")),
    ((FWD, BWD), dict(heads=0), ERR_UNSUPPORTED, SHAPE_TEXT.replace(b"%d, dh %d", b"256, dh 256")),
    ((FWD, BWD), dict(qkv_split=None), ERR_INVALID, QKV_TEXT),
    ((FWD, BWD), dict(ld=1024), ERR_INVALID, QKV_TEXT),                      # below 3C = 1536
    ((FWD, BWD), dict(ld=1552), ERR_INVALID, QKV_TEXT),                      # no multiple of 32
    ((FWD, BWD), dict(qkv_split=FAKE[0] + 64), ERR_INVALID, QKV_TEXT),
    ((FWD, BWD), dict(mode=3), ERR_INVALID, b"%s: unknown compute mode 3"),
    ((FWD,), dict(o_split=None), ERR_INVALID, b"%s: bad output planes"),
    ((FWD,), dict(ldo=256), ERR_INVALID, b"%s: bad output planes"),
    ((FWD,), dict(ldo=528), ERR_INVALID, b"%s: bad output planes"),
    ((FWD,), dict(o_split=FAKE[1] + 64), ERR_INVALID, b"%s: bad output planes"),
    ((FWD,), dict(pt_split=FAKE[2] + 2), ERR_INVALID, b"%s: P^T planes must be 128-byte aligned"),
    ((BWD,), dict(pt_split=None), ERR_INVALID, b"%s: null pointer"),
    ((BWD,), dict(do_split=None), ERR_INVALID, b"%s: null pointer"),
    ((BWD,), dict(dst_split=None), ERR_INVALID, b"%s: null pointer"),
    ((BWD,), dict(dqkv_split=None), ERR_INVALID, b"%s: null pointer"),
    ((BWD,), dict(lddo=256), ERR_INVALID, b"%s: bad row strides"),
    ((BWD,), dict(lddo=528), ERR_INVALID, b"%s: bad row strides"),
    ((BWD,), dict(lddqkv=1024), ERR_INVALID, b"%s: bad row strides"),
    ((BWD,), dict(lddqkv=1552), ERR_INVALID, b"%s: bad row strides"),
    ((BWD,), dict(pt_split=FAKE[2] + 64), ERR_INVALID, b"%s: planes must be 128-byte aligned"),
    ((BWD,), dict(do_split=FAKE[3] + 2), ERR_INVALID, b"%s: planes must be 128-byte aligned"),
    ((BWD,), dict(dst_split=FAKE[4] + 32), ERR_INVALID, b"%s: planes must be 128-byte aligned"),
    ((BWD,), dict(dqkv_split=FAKE[5] + 64), ERR_INVALID, b"%s: planes must be 128-byte aligned"),
    # two faults at once: the first of the entry point's order is the one reported
    ((FWD, BWD), dict(N=128, mode=3), ERR_UNSUPPORTED, SHAPE_TEXT.replace(b"%d, dh %d", b"128, dh 256")),
    ((FWD, BWD), dict(ld=1024, mode=3), ERR_INVALID, QKV_TEXT),
    ((FWD, BWD), dict(mode=3, o_split=None, do_split=None), ERR_INVALID, b"%s: unknown compute mode 3"),
    ((FWD,), dict(ldo=256, pt_split=FAKE[2] + 2), ERR_INVALID, b"%s: bad output planes"),
    ((BWD,), dict(dst_split=None, lddo=256), ERR_INVALID, b"%s: null pointer"),
    ((BWD,), dict(dqkv_split=None, pt_split=FAKE[2] + 64), ERR_INVALID, b"%s: null pointer"),
    ((BWD,), dict(lddqkv=1024, do_split=FAKE[3] + 2), ERR_INVALID, b"%s: bad row strides"),
]


@pytest.mark.parametrize("who,kw,status,text", ATTN_REFUSALS, ids=[f"{i}-{'-'.join(r[1])}" for i, r in enumerate(ATTN_REFUSALS)])
def test_refusals_keep_their_status_message_and_order(who, kw, status, text):
    """bad N / dh, bad mode, missing or misaligned planes and short or odd row strides: the host checks of both entry points, in the order
    they have always been reported (the backward: null pointers, then strides, then alignment).  No descriptor here reaches a launch."""
    import os
    assert "BD_ATTN_SP" not in os.environ, "BD_ATTN_SP=0 turns every call away at the first check"
    from baddiffusion_amd.build import build_lib
    build_lib(force=False, verbose=False)
    from baddiffusion_amd import _lib as L
    lib = L.load()
    good = dict(B=2, heads=2, N=N, dh=DH, qkv_split=FAKE[0], ld=1536, scale=SCALE, o_split=FAKE[1], ldo=512, pt_split=FAKE[2], do_split=FAKE[3],
                lddo=512, dst_split=FAKE[4], dqkv_split=FAKE[5], lddqkv=1536, mode=BF16X3)
    d = L.AttnSpDesc(**{**good, **kw})
    for name in who:
        fn = lib.bd_attn_sp_fwd if name == FWD else lib.bd_attn_sp_bwd
        assert fn(ctypes.byref(d), None) == status and lib.bd_last_error() == text.replace(b"%s", name), (name, kw, lib.bd_last_error())
    assert lib.bd_attn_sp_fwd(None, None) == ERR_INVALID and lib.bd_last_error() == b"bd_attn_sp_fwd: null descriptor"
    assert lib.bd_attn_sp_bwd(None, None) == ERR_INVALID and lib.bd_last_error() == b"bd_attn_sp_bwd: null descriptor"
    assert (lib.bd_attn_sp_supported(256, 256), lib.bd_attn_sp_supported(128, 256), lib.bd_attn_sp_supported(256, 512)) == (1, 0, 0)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from baddiffusion_amd import _lib as L
    return L.load(), L


PAD_QKV, PAD_O = Lay(0, 64, 0), Lay(0, 32, 0)


def attn_fwd(dev, qkv, B, heads, mode, lay_o=DENSE, want_pt=True):
    lib, L = dev
    C_ = heads * DH
    o = Buf(True, 1, B * N, C_, lay_o)
    pt = Buf(True, 1, B * heads * N, N, DENSE) if want_pt else None
    d = L.AttnSpDesc(B=B, heads=heads, N=N, dh=DH, qkv_split=qkv.ptr, ld=qkv.ld, scale=SCALE, o_split=o.ptr, ldo=o.ld,
                     pt_split=pt.ptr if want_pt else None, mode=mode)
    L.check(lib.bd_attn_sp_fwd(ctypes.byref(d), L.stream()), "bd_attn_sp_fwd")
    return o, pt


def attn_bwd(dev, qkv, pt, do, B, heads, mode, lay_dqkv=DENSE):
    lib, L = dev
    C_ = heads * DH
    dqkv = Buf(True, 1, B * N, 3 * C_, lay_dqkv)
    dst = Buf(True, 1, B * heads * N, N, DENSE)
    d = L.AttnSpDesc(B=B, heads=heads, N=N, dh=DH, qkv_split=qkv.ptr, ld=qkv.ld, scale=SCALE, pt_split=pt.ptr, do_split=do.ptr, lddo=do.ld,
                     dst_split=dst.ptr, dqkv_split=dqkv.ptr, lddqkv=dqkv.ld, mode=mode)
    L.check(lib.bd_attn_sp_bwd(ctypes.byref(d), L.stream()), "bd_attn_sp_bwd")
    return dqkv, dst


def upload(c, B, heads, lay_qkv=DENSE, lay_do=DENSE):
    qkv = torch.cat([rows_of(c[n], B, heads) for n in ("q", "k", "v")], dim=1)
    return (Buf(True, 1, B * N, 3 * heads * DH, lay_qkv, planes(qkv)[None]),
            Buf(True, 1, B * N, heads * DH, lay_do, planes(rows_of(c["do"], B, heads))[None]))


def run_all(dev, c, B, heads, mode, lays=(DENSE, DENSE, DENSE, DENSE)):
    """forward + backward -> {"o", "pt", "dst", "dqkv"}: int16 planes on the CPU; asserts that nothing outside a window was touched"""
    qkv, do = upload(c, B, heads, lays[0], lays[2])
    o, pt = attn_fwd(dev, qkv, B, heads, mode, lays[1])
    dqkv, dst = attn_bwd(dev, qkv, pt, do, B, heads, mode, lays[3])
    torch.cuda.synchronize()
    for name, buf in (("qkv", qkv), ("do", do), ("o", o), ("pt", pt), ("dqkv", dqkv), ("dst", dst)):
        assert not buf.outside_changes(), (name, "bytes outside the window changed", buf.outside_changes())
    return {"o": o.win[0].cpu(), "pt": pt.win[0].cpu(), "dst": dst.win[0].cpu(), "dqkv": dqkv.win[0].cpu()}


def ref_planes(r, B, heads):
    """the reference's four outputs as fp64 matrices in the layout of the device buffers"""
    BH = B * heads
    return {"o": rows_of(r["o"], B, heads), "pt": r["pt"].reshape(BH * N, N), "dst": r["dst"].reshape(BH * N, N),
            "dqkv": torch.cat([rows_of(r[n], B, heads) for n in ("dq", "dk", "dv")], dim=1)}


def values(p):
    hi, lo = plane_values(p)
    return hi.double() + lo.double()


@gpu
@pytest.mark.parametrize("kind,B,heads,opset", STRUCT_PARAMS)
def test_attn_sp_structured_softmax_is_exact(dev, kind, B, heads, opset):
    """cases (a) and (b): O, P^T, dS^T and dq | dk | dv planes are bit-equal (up to the sign of a zero) to the split of the fp64 reference, in
    both modes; rows / columns at fault are named per plane"""
    c = structured_case(kind, B, heads, opset)
    for mode in (BF16X3, BF16):
        got = run_all(dev, c, B, heads, mode)
        want = ref_planes(c["ref"][mode], B, heads)
        dqdk = 2 * heads * DH // 32                         # the 32-column blocks of dq | dk in a dqkv row
        for name in ("o", "pt", "dst", "dqkv"):
            w = planes(want[name] + 0.0)                    # + 0.0: the REFERENCE's zeros are +0; the device's bits are taken as they are ...
            g = got[name].clone()
            if name == "dst":                               # ... except in dS^T and the dq | dk derived from it (module docstring)
                g, w = canon(g), canon(w)
            elif name == "dqkv":
                g[:, :dqdk] = canon(g[:, :dqdk]); w[:, :dqdk] = canon(w[:, :dqdk])
            assert torch.equal(g, w), (kind, B, heads, opset, mode, name, describe_planes(got[name], w))
        if kind != "ties":      # said once more in words: dS^T and dq | dk are zero, P^T is the 0/1 matrix
            assert not bool(canon(got["dst"]).any()) and not bool(canon(got["dqkv"][:, : 2 * heads * DH // 32]).any())
            assert torch.equal(values(got["pt"]), c["ind"].double().transpose(1, 2).reshape(-1, N))


@gpu
@pytest.mark.parametrize("B,heads", SHAPES)
def test_attn_sp_large_exact_logits(dev, B, heads):
    """case (c): logits beyond +-88.7, the softmax nearly one-hot in many rows: forward and backward against fp64 at 5e-5 / 1e-4, all finite"""
    c = large_logit_case(B, heads)
    for mode in (BF16X3, BF16):
        r = (lambda t: rnd(t).double()) if mode == BF16 else (lambda t: t.double())
        P = torch.softmax(SCALE * r(c["q"]) @ r(c["k"]).transpose(1, 2), dim=-1)
        want = ref_planes(reference(c["q"], c["k"], c["v"], c["do"], P, mode), B, heads)
        got = {k: values(v) for k, v in run_all(dev, c, B, heads, mode).items()}
        C_ = heads * DH
        errs = {"o": relerr(got["o"], want["o"]), "pt": relerr(got["pt"], want["pt"]), "dst": relerr(got["dst"], want["dst"]),
                "dq": relerr(got["dqkv"][:, :C_], want["dqkv"][:, :C_]), "dk": relerr(got["dqkv"][:, C_: 2 * C_], want["dqkv"][:, C_: 2 * C_]),
                "dv": relerr(got["dqkv"][:, 2 * C_:], want["dqkv"][:, 2 * C_:])}
        print(f"MEASURE attn_sp_large_logits B{B}h{heads} mode {mode} " + " ".join(f"{k} {e:.3e}" for k, e in errs.items()))
        assert all(bool(torch.isfinite(g).all()) for g in got.values()), (B, heads, mode, "NaN or Inf")
        assert errs["o"] < 5e-5 and errs["pt"] < 5e-5, (B, heads, mode, errs)
        assert errs["dst"] < 1e-4 and errs["dq"] < 1e-4 and errs["dk"] < 1e-4 and errs["dv"] < 1e-4, (B, heads, mode, errs)


@gpu
def test_attn_sp_backward_against_rounded_operands(dev):
    """case (d): dq | dk | dv and the dS^T planes of the single-pass backward on randn sit at the accumulation level from the fp64 reference
    of the bf16-rounded operands; the three-product result of the same inputs is at least 10x further away"""
    B, heads = 2, 1
    g = torch.Generator().manual_seed(5)
    c = {n: torch.randn(B * heads, N, DH, generator=g) for n in ("q", "k", "v", "do")}
    P = torch.softmax(SCALE * rnd(c["q"]).double() @ rnd(c["k"]).double().transpose(1, 2), dim=-1)
    want = ref_planes(reference(c["q"], c["k"], c["v"], c["do"], P, BF16), B, heads)
    got1 = {k: values(v) for k, v in run_all(dev, c, B, heads, BF16).items()}
    got3 = {k: values(v) for k, v in run_all(dev, c, B, heads, BF16X3).items()}
    C_ = heads * DH
    cols = {"dq": slice(0, C_), "dk": slice(C_, 2 * C_), "dv": slice(2 * C_, 3 * C_)}
    _pair("attn_sp_bwd_dst", got1["dst"], got3["dst"], want["dst"], TOL_ATTN_BWD["dst"])
    for name, s in cols.items():
        _pair(f"attn_sp_bwd_{name}", got1["dqkv"][:, s], got3["dqkv"][:, s], want["dqkv"][:, s], TOL_ATTN_BWD[name])


@gpu
@pytest.mark.parametrize("mode", [BF16X3, BF16], ids=["bf16x3", "bf16"])
def test_attn_sp_padded_row_strides(dev, mode):
    """case (e): ld = 3C + 64, ldo = lddo = C + 32, lddqkv = 3C + 64 give the bits of the dense run (B = 3, two heads); the padding columns and
    the guard band keep their sentinel (run_all checks every buffer); the inference form (no P^T) gives the same O"""
    B, heads = 3, 2
    g = torch.Generator().manual_seed(9)
    c = {n: torch.randn(B * heads, N, DH, generator=g) for n in ("q", "k", "v", "do")}
    dense = run_all(dev, c, B, heads, mode)
    padded = run_all(dev, c, B, heads, mode, lays=(PAD_QKV, PAD_O, PAD_O, PAD_QKV))
    for name in ("o", "pt", "dst", "dqkv"):
        assert torch.equal(padded[name], dense[name]), (mode, name, describe_planes(padded[name], dense[name]))
    for lay_qkv, lay_o in ((DENSE, DENSE), (PAD_QKV, PAD_O)):
        qkv, _ = upload(c, B, heads, lay_qkv)
        o, none = attn_fwd(dev, qkv, B, heads, mode, lay_o, want_pt=False)
        assert none is None and not o.outside_changes(), o.outside_changes()
        assert torch.equal(o.win[0].cpu(), dense["o"]), (mode, "inference form", describe_planes(o.win[0].cpu(), dense["o"]))
