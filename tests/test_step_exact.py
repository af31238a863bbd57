"""GPU: exact values and edges of the kernels a training step and a sampling loop start and end with -- bd_poison_qsample / bd_qsample,
bd_ddpm_step / bd_ddim_step / bd_lincomb, bd_adam_clip(_dev), bd_anp_apply / bd_anp_grad (csrc/elementwise.hip) -- and of the producers of
split planes bd_split_bf16 (csrc/igemm.hip), bd_split_rows(_ups2), bd_split_wt (csrc/conv_ps.hip); the ld checks of the loss launchers.

Cases, data and references come from tests/_step_exact.py; tests/test_step_exact_host.py ties the references to the golden vectors and the
sizes to the constants in the sources.  The formula kernels are held to EQUAL BITS against the numpy-float32 statements, the integer data to
torch.equal against fp64.  The entry points are called with raw pointers.  Every fp32 output lies in a NaN-filled buffer with 4 floats of
margin, every uint16 plane in a buffer filled with 0xA5A5 with 64 elements of margin: whatever lies outside the written region must be
unchanged afterwards and everything inside written; a rejected call returns its status code and leaves its outputs untouched, and is always
given real, adequately sized buffers.  Tolerances: none, but for the one comparison of clip + Adam with torch on the CPU (1e-6 / 1e-7, as
test_adam_clip_vs_torch) and the denormal inputs of the split, which pin no bits."""
import ctypes as CT

import numpy as np
import pytest
import torch

from tests import _small_exact as S
from tests import _step_exact as X

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -2        # enum bd_status
LEAD, TRAIL = 4, 4                   # floats of NaN margin (16 bytes: the views stay 16-byte aligned)
OFF = X.STEP_MISALIGNED_LEAD         # a view that starts 4 bytes off a 16-byte boundary
I64_SENTINEL = -7777
SENT = int(np.array(X.U16_SENTINEL, dtype=np.uint16).view(np.int16))
MARGIN = X.U16_MARGIN


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def lib(gpu):
    from baddiffusion_amd import _lib as L
    L.load()
    return L


@pytest.fixture(scope="module")
def sched(gpu):
    a, ac = X.tables()
    return a, ac, torch.from_numpy(a).to(gpu), torch.from_numpy(ac).to(gpu)


def t32(x):
    return torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x


def flat_in(x, gpu, lead=LEAD):
    """x flattened into a NaN-margined device buffer: (buffer, pointer of the data)"""
    buf = S.padded(t32(x).reshape(-1), lead, TRAIL).to(gpu)
    return buf, buf[lead:].data_ptr()


def flat_out(n, gpu, lead=LEAD):
    buf = torch.full((lead + n + TRAIL,), S.NAN, device=gpu)
    return buf, buf[lead:].data_ptr()


def flat_result(buf, n, lead=LEAD, finite=True):
    """host copy of the n floats of an output buffer, after checking that nothing outside them was written and nothing inside left NaN"""
    host = buf.cpu()
    assert S.outside_is_nan(host, lead, 1, n, n), "written outside the output"
    out = host[lead: lead + n].clone()
    if finite:
        assert bool(torch.isfinite(out).all()), "output left unwritten or not finite"
    return out


def rows_out(rows, C, ld, gpu):
    buf = S.nan_rows(rows, C, ld, LEAD, TRAIL).to(gpu)
    return buf, buf[LEAD:].data_ptr()


def rows_result(buf, rows, C, ld):
    host = buf.cpu()
    assert S.outside_is_nan(host, LEAD, rows, C, ld), "written outside the output"
    out = S.rows_view(host, LEAD, rows, C, ld).clone()
    assert bool(torch.isfinite(out).all()), "output left unwritten or not finite"
    return out


def untouched(*bufs):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(b).all()) for b in bufs)


def eq_bits(got, want, what=""):
    want = t32(want).reshape(got.shape)
    assert X.same_bits(got, want), (what, float((got.double() - want.double()).abs().max()), int((X.bits(got) != X.bits(want)).sum()))


# ================================================================================================ 1. q_sample
def qs_call(L, l, gpu, sched, shape, d, ld, outs, al_d=None, ac_d=None, both=False, neither=False):
    """one bd_poison_qsample call: (status, NS of host results or None).  Every output in a margined buffer; the int64 mask in a sentinel-filled one"""
    B, C, H, W = shape
    rows, n, chw = B * H * W, B * C * H * W, C * H * W
    ldn, ldt = ld
    u8 = d.images.dtype == np.uint8
    img = torch.from_numpy(d.images).to(gpu)
    other = torch.zeros(d.images.size, dtype=torch.float32 if u8 else torch.uint8, device=gpu)
    pois, trig, tgt = torch.from_numpy(d.is_poison).to(gpu), torch.from_numpy(d.trigger).to(gpu), torch.from_numpy(d.target_img).to(gpu)
    eps, t = torch.from_numpy(d.noise).to(gpu), torch.from_numpy(d.timesteps).to(gpu)
    ri = None if d.row_index is None else torch.from_numpy(d.row_index).to(gpu)
    fl = None if d.flip is None else torch.from_numpy(d.flip).to(gpu)
    xnb, xnp = rows_out(rows, C, max(ldn, C), gpu)
    tgb, tgp = rows_out(rows, C, max(ldt, C), gpu)
    opt = {k: flat_out(n, gpu) for k in ("R", "x0", "image")} if outs else {}
    mb = torch.full((LEAD + chw + TRAIL,), I64_SENTINEL, dtype=torch.int64, device=gpu) if outs else None
    f32p, u8p = (None, img.data_ptr()) if u8 else (img.data_ptr(), None)
    if both:
        f32p, u8p = (other.data_ptr(), u8p) if u8 else (f32p, other.data_ptr())
    if neither:
        f32p = u8p = None
    desc = L.PoisonQsampleDesc(B=B, C=C, H=H, W=W, images_f32=f32p, images_u8=u8p, is_poison=pois.data_ptr(), trigger=trig.data_ptr(),
                               target_img=tgt.data_ptr(), noise=eps.data_ptr(), timesteps=t.data_ptr(),
                               alphas=(sched[2] if al_d is None else al_d).data_ptr(), alphas_cumprod=(sched[3] if ac_d is None else ac_d).data_ptr(),
                               vmin=float(d.vmin), x_noisy=xnp, ld_noisy=ldn, target=tgp, ld_target=ldt,
                               R_out=opt["R"][1] if outs else None, x0_out=opt["x0"][1] if outs else None,
                               mask_out=mb[LEAD:].data_ptr() if outs else None, image_out=opt["image"][1] if outs else None,
                               row_index=L.ptr(ri), flip=L.ptr(fl))
    status = l.bd_poison_qsample(CT.byref(desc), L.stream())
    torch.cuda.synchronize()
    if status != 0:
        assert untouched(xnb, tgb, *[b for b, _ in opt.values()]) and (mb is None or bool((mb == I64_SENTINEL).all()))
        return status, None
    r = X.NS(x_noisy=rows_result(xnb, rows, C, ldn).view(B, H, W, C), target=rows_result(tgb, rows, C, ldt).view(B, H, W, C))
    if outs:
        for k, (b, _) in opt.items():
            setattr(r, k, flat_result(b, n).view(B, C, H, W))
        m = mb.cpu()
        assert bool((m[:LEAD] == I64_SENTINEL).all()) and bool((m[LEAD + chw:] == I64_SENTINEL).all())
        r.mask = m[LEAD: LEAD + chw].view(C, H, W)
    return status, r


@pytest.mark.parametrize("shape,v", X.qs_cases(), ids=lambda p: "x".join(map(str, p)) if isinstance(p, tuple) else p.name)
def test_poison_qsample(gpu, lib, sched, shape, v):
    L, l = lib, lib.load()
    B, C, H, W = shape
    d = X.qs_data(shape, v)
    ref = X.poison_qsample_stmt(sched[0], sched[1], d)
    ld = (C + X.QS_LD_EXTRA[0], C + X.QS_LD_EXTRA[1]) if v.ld else (C, C)
    status, r = qs_call(L, l, gpu, sched, shape, d, ld, v.outs)
    assert status == 0, l.bd_last_error()
    eq_bits(r.x_noisy, ref.x_noisy, "x_noisy")
    eq_bits(r.target, ref.target, "target")
    if v.outs:
        eq_bits(r.R, ref.R, "R_out")
        eq_bits(r.x0, ref.x0, "x0_out")
        eq_bits(r.image, ref.image, "image_out")
        assert torch.equal(r.mask, torch.from_numpy(ref.mask))


@pytest.mark.parametrize("shape", X.QS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_qsample(gpu, lib, sched, shape):
    L, l = lib, lib.load()
    B, C, H, W = shape
    rows = B * H * W
    d = X.qs_data(shape, X.QS_VARIANTS[0])
    _, _, R, x0 = X.qs_batch(d)
    x0d, Rd, ed, td = (torch.from_numpy(np.ascontiguousarray(t)).to(gpu) for t in (x0, R, d.noise, d.timesteps))
    want = X.qsample_stmt(sched[0], sched[1], x0, R, d.noise, d.timesteps)
    for ldn, ldt in ((C + X.QS_LD_EXTRA[0], C + X.QS_LD_EXTRA[1]), (C, C)):
        xnb, xnp = rows_out(rows, C, ldn, gpu)
        tgb, tgp = rows_out(rows, C, ldt, gpu)
        desc = L.QsampleDesc(B=B, C=C, H=H, W=W, x0=x0d.data_ptr(), R=Rd.data_ptr(), noise=ed.data_ptr(), timesteps=td.data_ptr(),
                             alphas=sched[2].data_ptr(), alphas_cumprod=sched[3].data_ptr(), x_noisy=xnp, ld_noisy=ldn, target=tgp, ld_target=ldt)
        L.check(l.bd_qsample(CT.byref(desc), L.stream()), "bd_qsample")
        eq_bits(rows_result(xnb, rows, C, ldn).view(B, H, W, C), want[0], "x_noisy")
        eq_bits(rows_result(tgb, rows, C, ldt).view(B, H, W, C), want[1], "target")


def test_qsample_routing(gpu, lib, sched):
    """tables of 0 and 1 with small-integer data: an operand read from the wrong tensor shows whatever the formula"""
    L, l = lib, lib.load()
    shape = B, C, H, W = X.QS_ROUTING_SHAPE
    rows = B * H * W
    x0, R, eps = X.qs_routing_data()
    t = np.array([0, 2, 1], dtype=np.int64)
    nhwc = lambda v: torch.from_numpy(np.ascontiguousarray(v.transpose(0, 2, 3, 1)))
    x0d, Rd, ed, td = (torch.from_numpy(v).to(gpu) for v in (x0, R, eps, t))
    # the fused kernel on integer images, trigger and target image: rows 0 and 2 poisoned
    d = X.NS(images=np.concatenate([x0] * 3)[:X.QS_N_RESIDENT].copy(), is_poison=np.array([1, 0, 1], dtype=np.uint8), flip=np.array([0, 1, 1], dtype=np.uint8),
             row_index=np.array([6, 1, 1], dtype=np.int64), trigger=S.ints((C, H, W), -2, 2, 75).numpy(), target_img=S.ints((C, H, W), -8, 8, 76).numpy(),
             noise=eps, timesteps=t, vmin=np.float32(-1.0))
    _, _, Rp, x0p = X.qs_batch(d)
    assert bool((Rp != 0).any()) and not np.array_equal(Rp, x0p)
    for r in X.QS_ROUTING:
        al = torch.full((3,), r.al, device=gpu)
        ac = torch.full((3,), r.ac, device=gpu)
        xnb, xnp = rows_out(rows, C, C + 3, gpu)
        tgb, tgp = rows_out(rows, C, C + 5, gpu)
        desc = L.QsampleDesc(B=B, C=C, H=H, W=W, x0=x0d.data_ptr(), R=Rd.data_ptr(), noise=ed.data_ptr(), timesteps=td.data_ptr(),
                             alphas=al.data_ptr(), alphas_cumprod=ac.data_ptr(), x_noisy=xnp, ld_noisy=C + 3, target=tgp, ld_target=C + 5)
        L.check(l.bd_qsample(CT.byref(desc), L.stream()), "bd_qsample")
        xn, tg = rows_result(xnb, rows, C, C + 3).view(B, H, W, C), rows_result(tgb, rows, C, C + 5).view(B, H, W, C)
        want = (nhwc(x0), nhwc(eps)) if r.ac == 1.0 else (nhwc(eps + R), nhwc(R + eps))
        assert torch.equal(xn, want[0]) and torch.equal(tg, want[1]), r.why
        status, got = qs_call(L, l, gpu, sched, shape, d, (C + 3, C + 5), True, al, ac)
        assert status == 0
        want = (nhwc(x0p), nhwc(eps)) if r.ac == 1.0 else (nhwc(eps + Rp), nhwc(Rp + eps))
        assert torch.equal(got.x_noisy, want[0]) and torch.equal(got.target, want[1]), r.why


def test_qsample_rejections(gpu, lib, sched):
    L, l = lib, lib.load()
    shape = B, C, H, W = (3, 3, 5, 7)
    rows = B * H * W
    d = X.qs_data(shape, X.QS_VARIANTS[0])
    for kw in (dict(ld=(C - 1, C + 5)), dict(ld=(C + 3, C - 1)), dict(ld=(C, C), both=True), dict(ld=(C, C), neither=True)):
        status, _ = qs_call(L, l, gpu, sched, shape, d, kw.pop("ld"), True, **kw)        # qs_call asserts the outputs untouched
        assert status == INVALID, kw
    x = torch.zeros(B * C * H * W, device=gpu)
    td = torch.from_numpy(d.timesteps).to(gpu)
    for ldn, ldt in ((C - 1, C), (C, C - 1)):
        xnb, xnp = rows_out(rows, C, C, gpu)
        tgb, tgp = rows_out(rows, C, C, gpu)
        desc = L.QsampleDesc(B=B, C=C, H=H, W=W, x0=x.data_ptr(), R=x.data_ptr(), noise=x.data_ptr(), timesteps=td.data_ptr(),
                             alphas=sched[2].data_ptr(), alphas_cumprod=sched[3].data_ptr(), x_noisy=xnp, ld_noisy=ldn, target=tgp, ld_target=ldt)
        assert l.bd_qsample(CT.byref(desc), L.stream()) == INVALID and b"ld < C" in l.bd_last_error()
        assert untouched(xnb, tgb)


# ================================================================================================ 2. DDPM / DDIM steps
def step_call(L, l, gpu, sched, kind, c, x, e, z, lead=LEAD, **override):
    """one bd_ddpm_step / bd_ddim_step call: (status, prev, pred_original or None) as host tensors"""
    n = x.size
    (xb, xp), (eb, ep), (zb, zp) = (flat_in(v, gpu, lead) for v in (x, e, z))
    pb, pp = flat_out(n, gpu, lead)
    ob, op = flat_out(n, gpu, lead) if c.x0 else (None, None)
    if kind == "ddpm":
        kw = dict(n=n, model_output=ep, sample=xp, noise=zp if c.noise else None, prev_sample=pp, pred_original=op, alphas_cumprod=sched[3].data_ptr(),
                  t=c.t, prev_t=c.prev_t, variance_type=c.vt, clip_sample=int(c.clip is not None), clip_sample_range=c.clip or 0.0,
                  clip_defense=int(c.cdef is not None), clip_defense_range=c.cdef or 0.0)
        kw.update(override)
        status = l.bd_ddpm_step(CT.byref(L.DdpmStepDesc(**kw)), L.stream())
    else:
        kw = dict(n=n, model_output=ep, sample=xp, noise=zp if c.eta > 0 else None, prev_sample=pp, pred_original=op, alphas_cumprod=sched[3].data_ptr(),
                  t=c.t, prev_t=c.prev_t, final_alpha_cumprod=c.final, eta=c.eta, clip_sample=int(c.clip is not None), clip_sample_range=c.clip or 0.0)
        kw.update(override)
        status = l.bd_ddim_step(CT.byref(L.DdimStepDesc(**kw)), L.stream())
    torch.cuda.synchronize()
    if status != 0:
        assert untouched(pb) and (ob is None or untouched(ob))
        return status, None, None
    return status, flat_result(pb, n, lead), flat_result(ob, n, lead) if c.x0 else None


STEP_KINDS = {"ddpm": (X.ddpm_cases, X.ddpm_coef, X.ddpm_stmt, X.STEP_BIG_DDPM), "ddim": (X.ddim_cases, X.ddim_coef, X.ddim_stmt, X.STEP_BIG_DDIM)}


@pytest.mark.parametrize("n", X.STEP_N)
@pytest.mark.parametrize("kind", ("ddpm", "ddim"))
def test_steps(gpu, lib, sched, kind, n):
    L, l = lib, lib.load()
    cases, coef, stmt, big = STEP_KINDS[kind]
    cases = cases()
    todo = list(enumerate(cases)) if n < X.STEP_SECOND_TRIP else [(i, cases[i]) for i in big]
    for i, c in todo:
        sb, sa = coef(sched[1], c)[:2]
        x, e, z, _ = X.step_data(n, sb, sa, c.clip, i)
        want_prev, want_x0 = stmt(sched[1], c, x, e, z)
        # every fourth case: all five buffers start 4 bytes off a 16-byte boundary
        status, prev, x0 = step_call(L, l, gpu, sched, kind, c, x, e, z, OFF if i % 4 == 1 else LEAD)
        assert status == 0, (vars(c), l.bd_last_error())
        eq_bits(prev, want_prev, (kind, "prev_sample", vars(c)))
        if c.x0:
            eq_bits(x0, want_x0, (kind, "pred_original", vars(c)))


def test_step_rejections(gpu, lib, sched):
    L, l = lib, lib.load()
    x, e, z, _ = X.step_data(257, 0.5, 0.5, None, 0)
    c = X._dp(500, 499)
    assert step_call(L, l, gpu, sched, "ddpm", c, x, e, z, t=-1)[0] == INVALID and b"t < 0" in l.bd_last_error()
    assert step_call(L, l, gpu, sched, "ddpm", c, x, e, z, noise=None)[0] == INVALID and b"noise" in l.bd_last_error()
    assert step_call(L, l, gpu, sched, "ddpm", c, x, e, z, n=0)[0] == INVALID
    assert step_call(L, l, gpu, sched, "ddpm", c, x, e, z, n=-5)[0] == INVALID
    c = X._di(500, 480, eta=0.5)
    assert step_call(L, l, gpu, sched, "ddim", c, x, e, z, t=-1)[0] == INVALID and b"t < 0" in l.bd_last_error()
    assert step_call(L, l, gpu, sched, "ddim", c, x, e, z, noise=None)[0] == INVALID and b"noise" in l.bd_last_error()
    assert step_call(L, l, gpu, sched, "ddim", c, x, e, z, n=0)[0] == INVALID


# ================================================================================================ 2. lincomb
def lincomb_call(L, l, ptrs, coeffs, n, clip, out_ptr):
    k = len(ptrs)
    arr = (CT.c_void_p * max(k, 1))(*ptrs)
    cs = (CT.c_float * max(k, 1))(*[float(c) for c in coeffs])
    return l.bd_lincomb(k, arr, cs, n, int(clip is not None), float(clip or 0.0), out_ptr, L.stream())


@pytest.mark.parametrize("k,n", X.lincomb_cases(), ids=lambda v: str(v))
def test_lincomb(gpu, lib, k, n):
    L, l = lib, lib.load()
    for exact in (True, False):
        terms, coeffs = X.lincomb_terms(k, n, exact)
        bufs = [flat_in(t, gpu) for t in terms]
        for clip in ((None, X.LINCOMB_CLIP) if exact else (None,)):
            ob, op = flat_out(n, gpu)
            L.check(lincomb_call(L, l, [p for _, p in bufs], coeffs, n, clip, op), "bd_lincomb")
            out = flat_result(ob, n)
            if exact:
                ref = X.lincomb_f64(terms, coeffs, clip)
                assert torch.equal(out, ref.float()), (k, n, clip, float((out - ref).abs().max()))
            else:
                eq_bits(out, X.lincomb_stmt(terms, coeffs, clip), (k, n))
        for (b, _), t in zip(bufs, terms):
            assert torch.equal(flat_result(b, n), t)


def test_lincomb_in_place(gpu, lib):
    """out is a term's own buffer: k = 1 with the clip (the ANP projection), and terms[0] / terms[2] at k = 3"""
    L, l = lib, lib.load()
    for k, which, clip, n in ((1, 0, X.LINCOMB_CLIP, 1023), (3, 0, None, 1023), (3, 2, X.LINCOMB_CLIP, 1023), (3, 2, None, 7),
                              (1, 0, 0.5, X.LINCOMB_SECOND_TRIP)):
        terms, coeffs = X.lincomb_terms(k, n, exact=False)
        bufs = [flat_in(t, gpu) for t in terms]
        ob, op = flat_out(n, gpu)
        L.check(lincomb_call(L, l, [p for _, p in bufs], coeffs, n, clip, op), "bd_lincomb")
        want = flat_result(ob, n)
        eq_bits(want, X.lincomb_stmt(terms, coeffs, clip))
        L.check(lincomb_call(L, l, [p for _, p in bufs], coeffs, n, clip, bufs[which][1]), "bd_lincomb")
        eq_bits(flat_result(bufs[which][0], n), want, (k, which))
        for j in range(k):
            if j != which:
                assert torch.equal(flat_result(bufs[j][0], n), terms[j])


def test_lincomb_rejections(gpu, lib):
    L, l = lib, lib.load()
    n = 64
    big = torch.zeros(LEAD + 2 * n + TRAIL, device=gpu)          # one allocation: a term at LEAD, out 4 floats further on
    ob, op = flat_out(n, gpu)
    t = [flat_in(torch.ones(n + 4), gpu) for _ in range(7)]
    tp = [p for _, p in t]
    term = big[LEAD:].data_ptr()
    assert lincomb_call(L, l, [term], [1.0], n, None, term + 16) == INVALID and b"overlaps" in l.bd_last_error()
    assert lincomb_call(L, l, [tp[0], term + 16], [1.0, 1.0], n, None, term) == INVALID and b"overlaps term 1" in l.bd_last_error()
    assert lincomb_call(L, l, [term], [1.0], n, None, term + 4 * n) == 0           # adjacent, not overlapping
    torch.cuda.synchronize()
    assert bool((big == 0).all())
    assert lincomb_call(L, l, [], [], n, None, op) == INVALID                      # k = 0
    assert lincomb_call(L, l, tp, [1.0] * 7, n, None, op) == INVALID               # k = 7
    assert lincomb_call(L, l, [tp[0], tp[1] + 4], [1.0, 1.0], n, None, op) == INVALID and b"aligned" in l.bd_last_error()
    assert lincomb_call(L, l, [tp[0]], [1.0], n, None, op + 4) == INVALID
    assert lincomb_call(L, l, [tp[0]], [1.0], 0, None, op) == INVALID
    assert untouched(ob)


def test_ops_lincomb_refuses_mismatched_out(gpu):
    from baddiffusion_amd import ops
    a, b = torch.ones(4, 6, device=gpu), torch.ones(4, 6, device=gpu)
    for bad in (torch.empty(6, 4, device=gpu), torch.empty(24, device=gpu), torch.empty(6, 4, device=gpu).t(), torch.empty(4, 6, device=gpu, dtype=torch.float64),
                torch.empty(4, 12, device=gpu)[:, ::2]):
        with pytest.raises(ValueError):
            ops.lincomb([a, b], [1.0, 2.0], out=bad)
    with pytest.raises(RuntimeError):
        ops.lincomb([a, b], [1.0, 2.0], out=torch.empty(4, 6))
    out = torch.empty(4, 6, device=gpu)
    assert ops.lincomb([a, b], [1.0, 2.0], out=out) is out and bool((out == 3).all())
    assert ops.lincomb([a, b], [1.0, 2.0], clip=2.5, out=a) is a and bool((a == 2.5).all())      # in place, as the ANP projection calls it
    flat = torch.zeros(64, device=gpu)
    with pytest.raises(RuntimeError):          # the library's own overlap check, through the wrapper
        ops.lincomb([flat[:32]], [1.0], out=flat[4:36])


# ================================================================================================ 2. the dense vec4 driver
_VEC4 = {}


def vec4_inputs(n):
    """the inputs of size n, drawn once and shared by the five entry points"""
    if n not in _VEC4:
        _VEC4.clear()                    # (the parameters are ordered by n: one size is alive at a time)
        _VEC4[n] = X.vec4_inputs(n)
    return _VEC4[n]


@pytest.mark.parametrize("op", X.VEC4_OPS)
@pytest.mark.parametrize("n", X.VEC4_N)
def test_vec4_driver(gpu, lib, n, op):
    """the five entry points of the shared float4 driver with every optional operand present, tail only (1, 3), body only (4), body + tail
    (7) and a second trip of every thread of the capped grid + tail: equal bits with the fp32 statements, the step kernels writing the
    new sample over the old one; margins of every buffer intact, the other inputs unchanged"""
    L, l = lib, lib.load()
    e, x, a, b, c, d = vec4_inputs(n)
    ins = [flat_in(v, gpu) for v in (e, x, a, b, c, d)]
    (eb, ep), (xb, xp), (ab, ap), (bb, bp), (cb, cp), (db, dp) = ins
    outs = {}

    def out(name):
        outs[name] = flat_out(n, gpu)
        return outs[name][1]

    if op == "lincomb":
        coeffs = X.LINCOMB_COEFFS
        L.check(lincomb_call(L, l, [p for _, p in ins], coeffs, n, X.LINCOMB_CLIP, out("out")), "bd_lincomb")
        want = {"out": X.lincomb_stmt([t32(v) for v in (e, x, a, b, c, d)], coeffs, X.LINCOMB_CLIP)}
    elif op == "dpm_step":
        desc = L.DpmStepDesc(n=n, model_output=ep, sample=xp, m1=ap, m2=bp, m0_out=out("m0"), prev_out=xp, convert=1, x0_clip=1, clip=1, **X.VEC4_DPM)
        L.check(l.bd_dpm_step(CT.byref(desc), L.stream()), "bd_dpm_step")
        m0, prev = X.dpm_stmt(X.VEC4_DPM, e, x, a, b)
        want = {"m0": m0, "sample": prev}
    elif op == "unipc_step":
        desc = L.UnipcStepDesc(n=n, model_output=ep, sample=xp, last_sample=ap, h1=bp, h2=cp, h3=dp, m0_out=out("m0"), corrected_out=out("xc"), prev_out=xp,
                               convert=1, x0_clip=1, clip=1, **X.VEC4_UNIPC)
        L.check(l.bd_unipc_step(CT.byref(desc), L.stream()), "bd_unipc_step")
        m0, xc, prev = X.unipc_stmt(X.VEC4_UNIPC, e, x, a, b, c, d)
        want = {"m0": m0, "xc": xc, "sample": prev}
    elif op == "sigma_step":
        desc = L.SigmaStepDesc(n=n, model_output=ep, sample=xp, base=ap, h1=bp, h2=cp, h3=dp, x0_out=out("x0"), d_out=out("d"), prev_out=xp,
                               scaled_out=out("scaled"), average=0, clip=1, **X.VEC4_SIGMA)
        L.check(l.bd_sigma_step(CT.byref(desc), L.stream()), "bd_sigma_step")
        x0, dv, prev, sc = X.sigma_stmt(X.VEC4_SIGMA, e, x, a, b, c, d)
        want = {"x0": x0, "d": dv, "sample": prev, "scaled": sc}
    else:
        L.check(l.bd_scale_input(xp, n, *X.VEC4_SCALE, out("out"), L.stream()), "bd_scale_input")
        want = {"out": X.scale_input_stmt(x, *X.VEC4_SCALE)}
    for name, w in want.items():
        eq_bits(flat_result(xb if name == "sample" else outs[name][0], n), w, (op, n, name))
    assert set(outs) == set(want) - {"sample"}
    for j, ((buf, _), v) in enumerate(zip(ins, (e, x, a, b, c, d))):          # the inputs, read or not, are as they were
        if not (j == 1 and "sample" in want):
            assert X.same_bits(flat_result(buf, n), t32(v)), (op, n, j)


# ================================================================================================ 3. clip + Adam
def adam_call(L, l, gpu, dev_form, data, max_norm, step, want_norm, g_lead=LEAD):
    """(p, m, v, norm or None) as host tensors after one bd_adam_clip / bd_adam_clip_dev"""
    p, g, m, v, ss = data
    n = p.numel()
    (pb, pp), (mb, mp), (vb, vp) = (flat_in(t, gpu) for t in (p, m, v))
    gb, gp = flat_in(g, gpu, g_lead)
    ssd = torch.tensor([ss], dtype=torch.float64, device=gpu)
    gn = torch.full((3,), S.NAN, device=gpu)
    gnp = gn[1:].data_ptr() if want_norm else None
    if dev_form:
        hyper = torch.tensor([float(h) for h in X.adam_hyper(step)], dtype=torch.float32, device=gpu)
        st = l.bd_adam_clip_dev(pp, gp, mp, vp, n, ssd.data_ptr(), max_norm, hyper.data_ptr(), X.ADAM_B1, X.ADAM_B2, X.ADAM_EPS, gnp, L.stream())
    else:
        st = l.bd_adam_clip(pp, gp, mp, vp, n, ssd.data_ptr(), max_norm, X.ADAM_LR, X.ADAM_B1, X.ADAM_B2, X.ADAM_EPS, step, gnp, L.stream())
    L.check(st, "bd_adam_clip")
    gn = gn.cpu()
    assert bool(torch.isnan(gn[0])) and bool(torch.isnan(gn[2])) and bool(torch.isnan(gn[1])) != want_norm
    assert torch.equal(flat_result(gb, n, g_lead), g)
    return flat_result(pb, n), flat_result(mb, n), flat_result(vb, n), float(gn[1]) if want_norm else None


@pytest.mark.parametrize("n", X.ADAM_N)
def test_adam_clip(gpu, lib, n):
    L, l = lib, lib.load()
    big = n == X.ADAM_SECOND_TRIP
    combos = [("active", 1, True), ("random", 1000, False)] if big else [(kind, step, (step + len(kind)) % 2 == 0) for kind in ("random", "active", "zero")
                                                                         for step in X.ADAM_STEPS]
    for i, (kind, step, want_norm) in enumerate(combos):
        data = X.adam_data(n, kind)
        mx = X.ADAM_MAX_NORM_ACTIVE if kind == "active" else X.ADAM_MAX_NORM_INACTIVE
        wp, wm, wv, wn = X.adam_stmt(*data, mx, step)
        got = None
        for dev_form in (False, True):
            p, m, v, norm = adam_call(L, l, gpu, dev_form, data, mx, step, want_norm, OFF if i % 3 == 1 else LEAD)
            what = (n, kind, step, dev_form)
            eq_bits(p, wp, what + ("p",)); eq_bits(m, wm, what + ("m",)); eq_bits(v, wv, what + ("v",))
            if want_norm:
                assert norm == float(wn), what
            if got is not None:                          # the device-scalar form gives the bits of the host-scalar form
                assert X.same_bits(p, got[0]) and X.same_bits(m, got[1]) and X.same_bits(v, got[2])
            got = (p, m, v)


def test_adam_clip_against_torch(gpu, lib):
    """n = 1023, random gradient, the clip active: torch.optim.Adam + clip_grad_norm_ on the CPU at the 1e-6 / 1e-7 of test_adam_clip_vs_torch"""
    L, l = lib, lib.load()
    for step in X.ADAM_STEPS:
        data = X.adam_data(1023, "random", seed=step)
        pt, norm_t = X.adam_torch(*data[:4], 0.1, step)
        p, _, _, norm = adam_call(L, l, gpu, False, data, 0.1, step, True)
        np.testing.assert_allclose(norm, norm_t, rtol=1e-6)
        np.testing.assert_allclose(p.numpy(), pt.numpy(), rtol=1e-6, atol=1e-7)
        eq_bits(p, X.adam_stmt(*data, 0.1, step)[0])


# ================================================================================================ 3. ANP
def anp_setup(gpu):
    params, geff, pw, pb = X.anp_data()
    items = torch.tensor(X.ANP_ITEMS, dtype=torch.int64, device=gpu)
    return params, geff, pw, pb, items


def test_anp_apply(gpu, lib):
    L, l = lib, lib.load()
    params, geff, pw, pb, items = anp_setup(gpu)
    n = X.ANP_NPARAMS
    (prb, prp), (pwb, pwp), (pbb, pbp) = flat_in(params, gpu), flat_in(pw, gpu), flat_in(pb, gpu)
    eb, ep = flat_out(n, gpu)
    L.check(l.bd_anp_apply(prp, n, pwp, pbp, items.data_ptr(), len(X.ANP_ITEMS), X.ANP_TOTAL_ROWS, ep, L.stream()), "bd_anp_apply")
    eff = flat_result(eb, n)
    ref = X.anp_apply_ref(params, pw, pb)
    assert torch.equal(eff, ref.float()), int((eff != ref.float()).sum())
    gap = torch.ones(n, dtype=torch.bool)
    for woff, boff, ln, _ in X.anp_rows():
        gap[woff: woff + ln] = False
        if boff >= 0:
            gap[boff] = False
    assert X.same_bits(eff[gap], params[gap]) and torch.equal(flat_result(prb, n), params)
    # rejections: outputs untouched
    eb, ep = flat_out(n, gpu)
    for args in ((prp, 0, pwp, pbp, items.data_ptr(), 3, 9, ep), (prp, n, pwp, pbp, items.data_ptr(), 0, 9, ep), (prp, n, pwp, pbp, items.data_ptr(), 3, 0, ep),
                 (prp, n, None, pbp, items.data_ptr(), 3, 9, ep)):
        assert l.bd_anp_apply(*args, L.stream()) == INVALID, args
    assert untouched(eb)


def test_anp_grad(gpu, lib):
    L, l = lib, lib.load()
    params, geff, pw, pb, items = anp_setup(gpu)
    rows = X.ANP_TOTAL_ROWS
    (prb, prp), (gb_, gp), (pwb, pwp) = flat_in(params, gpu), flat_in(geff, gpu), flat_in(pw, gpu)
    gw_ref, gb_ref, rn_ref = X.anp_grad_ref(params, geff, pw)
    for with_norm in (True, False):
        (wb, wp), (bb, bp), (nb, npp) = flat_out(rows, gpu), flat_out(rows, gpu), flat_out(rows, gpu)
        L.check(l.bd_anp_grad(prp, gp, items.data_ptr(), len(X.ANP_ITEMS), rows, pwp if with_norm else None, wp, bp, npp if with_norm else None, L.stream()),
                "bd_anp_grad")
        gw, gb = flat_result(wb, rows), flat_result(bb, rows)
        assert torch.equal(gw, gw_ref.float()) and torch.equal(gb, gb_ref.float()), (gw, gw_ref)
        if with_norm:
            eq_bits(flat_result(nb, rows), rn_ref, "row_norm")
        else:
            assert untouched(nb)
    (wb, wp), (bb, bp), (nb, npp) = flat_out(rows, gpu), flat_out(rows, gpu), flat_out(rows, gpu)
    assert l.bd_anp_grad(prp, gp, items.data_ptr(), 3, rows, None, wp, bp, npp, L.stream()) == INVALID and b"row_norm needs pert_w" in l.bd_last_error()
    assert l.bd_anp_grad(prp, gp, items.data_ptr(), 3, 0, pwp, wp, bp, npp, L.stream()) == INVALID
    assert untouched(wb, bb, nb)


# ================================================================================================ 4. producers of split planes
def u16_out(n, gpu, lead=MARGIN):
    """a sentinel-filled int16 device buffer for n uint16 values: (buffer, pointer of the data)"""
    buf = torch.full((lead + n + MARGIN,), SENT, dtype=torch.int16, device=gpu)
    return buf, buf[lead:].data_ptr()


def u16_result(buf, n, lead=MARGIN):
    host = buf.cpu()
    assert bool((host[:lead] == SENT).all()) and bool((host[lead + n:] == SENT).all()), "written outside the planes"
    return host[lead: lead + n]


def u16_untouched(buf):
    torch.cuda.synchronize()
    return bool((buf == SENT).all())


@pytest.mark.parametrize("n", X.SPLIT_BF16_N)
def test_split_bf16(gpu, lib, n):
    L, l = lib, lib.load()
    x = X.split_data(n, n % 9973)
    xb, xp = flat_in(x, gpu)
    ob, op = u16_out(2 * n, gpu)
    L.check(l.bd_split_bf16(xp, n, op, L.stream()), "bd_split_bf16")
    got = u16_result(ob, 2 * n)
    want = X.split_planes(x.view(n // 32, 32)).view(-1)
    assert torch.equal(got, want), int((got != want).sum())


def test_split_bf16_nonfinite_and_denormal(gpu, lib):
    """+-inf, NaN and 0x7F7F8000: hi is torch's conversion (for NaN: a NaN).  fp32 denormals pin no bits (the conversion follows the denormal mode): both planes
    finite and |hi + lo - x| <= 2^-126; what the hardware did is printed and recorded in DESIGN.md"""
    L, l = lib, lib.load()
    nf, dn = X.from_bits(X.SPLIT_NONFINITE_BITS), X.from_bits(X.SPLIT_DENORMAL_BITS)
    x = torch.ones(32)
    x[:len(nf)] = torch.from_numpy(nf.copy())
    x[8: 8 + len(dn)] = torch.from_numpy(dn.copy())
    xb, xp = flat_in(x, gpu)
    ob, op = u16_out(64, gpu)
    L.check(l.bd_split_bf16(xp, 32, op, L.stream()), "bd_split_bf16")
    got = u16_result(ob, 64).view(1, 64)
    want_hi, _ = X.split_hi_lo(x)
    print("split of non-finite / denormal fp32 (input bits: hi lo): " + ", ".join(
        f"{b:08X}: {int(got[0, i]) & 0xFFFF:04X} {int(got[0, 32 + i]) & 0xFFFF:04X}"
        for i, b in list(enumerate(X.SPLIT_NONFINITE_BITS)) + [(8 + j, b) for j, b in enumerate(X.SPLIT_DENORMAL_BITS)]))
    hi, lo = X.unsplit(got, 32)
    # a NaN has no one encoding (torch's vectorised CPU conversion writes 0xFFFF, its scalar one and the hardware 0x7FC0): NaN where torch
    # has NaN, torch's bits everywhere else
    nan = torch.isnan(x[:len(nf)])
    assert X.SPLIT_NONFINITE_BITS[2] == 0x7FC00000 and nan.tolist() == [False, False, True, False]
    assert torch.equal(torch.isnan(hi[0, :len(nf)]), nan) and torch.equal(got[0, :len(nf)][~nan], want_hi[:len(nf)][~nan])
    d = slice(8, 8 + len(dn))
    assert bool(torch.isfinite(hi[0, d]).all()) and bool(torch.isfinite(lo[0, d]).all())
    assert bool(((hi[0, d].double() + lo[0, d].double() - x[d].double()).abs() <= 2.0 ** -126).all())
    assert torch.equal(got[0, 16:32], want_hi[16:32]) and bool((got[0, 48:] == 0).all())          # the ones around them


def test_split_bf16_rejections(gpu, lib):
    L, l = lib, lib.load()
    xb, xp = flat_in(torch.ones(128), gpu)
    ob, op = u16_out(256, gpu)
    for n in (33, 16, 0):
        assert l.bd_split_bf16(xp, n, op, L.stream()) == INVALID, n
    assert l.bd_split_bf16(xp + 4, 64, op, L.stream()) == UNSUPPORTED
    assert l.bd_split_bf16(xp, 64, op + 4, L.stream()) == UNSUPPORTED
    assert u16_untouched(ob)


def split_rows_call(L, l, gpu, x, ld_src, ld_dst):
    rows, C = x.shape
    xb = S.strided_rows(x, ld_src, LEAD, TRAIL)[1].to(gpu)
    ob, op = u16_out(rows * 2 * ld_dst, gpu)
    L.check(l.bd_split_rows(xb[LEAD:].data_ptr(), ld_src, rows, C, op, ld_dst, L.stream()), "bd_split_rows")
    return u16_result(ob, rows * 2 * ld_dst).view(rows, 2 * ld_dst)


@pytest.mark.parametrize("rows,C,ld_src,ld_dst", X.SPLIT_ROWS_CASES)
def test_split_rows(gpu, lib, rows, C, ld_src, ld_dst):
    L, l = lib, lib.load()
    x = X.split_data(rows * C, rows % 9973 + C).view(rows, C)
    got = split_rows_call(L, l, gpu, x, ld_src, ld_dst)
    want = X.split_planes(x, ld_dst)          # the sentinel beyond the planes where ld_dst > C
    assert torch.equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("B,H,W,C", X.SPLIT_UPS2_SHAPES)
def test_split_rows_ups2(gpu, lib, B, H, W, C):
    L, l = lib, lib.load()
    x = X.split_data(B * H * W * C, B * H * W + C).view(B, H, W, C)
    up = X.ups2(x).reshape(-1, C)
    xb = S.strided_rows(x.view(-1, C), C + 4, LEAD, TRAIL)[1].to(gpu)
    for extra in X.SPLIT_UPS2_LD_EXTRA:
        ld = C + extra
        ob, op = u16_out(up.shape[0] * 2 * ld, gpu)
        L.check(l.bd_split_rows_ups2(xb[LEAD:].data_ptr(), C + 4, B, H, W, C, op, ld, L.stream()), "bd_split_rows_ups2")
        got = u16_result(ob, up.shape[0] * 2 * ld).view(-1, 2 * ld)
        assert torch.equal(got, X.split_planes(up, ld)), (extra, int((got != X.split_planes(up, ld)).sum()))
        assert torch.equal(got, split_rows_call(L, l, gpu, up, C, ld))


def test_split_rows_rejections(gpu, lib):
    L, l = lib, lib.load()
    xb, xp = flat_in(torch.ones(8 * 128), gpu)
    ob, op = u16_out(32 * 2 * 128, gpu)
    st = L.stream()
    # (C, ld_src, ld_dst, src offset, dst offset in bytes) -> status; rows = 4 / B, H, W = 1, 1, 1 (four output rows)
    table = (((48, 64, 64, 0, 0), UNSUPPORTED), ((64, 64, 80, 0, 0), UNSUPPORTED), ((64, 66, 64, 0, 0), UNSUPPORTED), ((64, 64, 64, 4, 0), UNSUPPORTED),
             ((64, 64, 64, 0, 64), UNSUPPORTED), ((64, 32, 64, 0, 0), INVALID), ((64, 60, 64, 0, 0), INVALID), ((64, 64, 32, 0, 0), INVALID),
             ((64, 128, 32, 0, 0), INVALID))
    for (C, lds, ldd, so, do), want in table:
        assert l.bd_split_rows(xp + so, lds, 4, C, op + do, ldd, st) == want, ("bd_split_rows", C, lds, ldd, so, do)
        if want == INVALID:
            assert b"< C" in l.bd_last_error()
        assert l.bd_split_rows_ups2(xp + so, lds, 1, 1, 1, C, op + do, ldd, st) == want, ("bd_split_rows_ups2", C, lds, ldd, so, do)
    assert l.bd_split_rows(xp, 64, 0, 64, op, 64, st) == INVALID
    assert u16_untouched(ob)


@pytest.mark.parametrize("Cin,Cout", X.SPLIT_WT_SHAPES)
def test_split_wt(gpu, lib, Cin, Cout):
    L, l = lib, lib.load()
    for named in (True, False):
        w = X.split_wt_data(Cin, Cout, named)
        wb, wp = flat_in(w, gpu)
        n = 2 * 9 * Cin * Cout
        ob, op = u16_out(n, gpu)
        L.check(l.bd_split_wt(wp, Cin, Cout, op, L.stream()), "bd_split_wt")
        got = u16_result(ob, n).view(Cin, 2 * 9 * Cout)
        want = X.split_wt_ref(w)
        if named and not torch.equal(got, want):         # name the first misplaced element
            h, _ = X.unsplit(got, 9 * Cout)
            bad = (h.view(Cin, 9, Cout) != w.permute(2, 1, 0)).nonzero()[0].tolist()
            raise AssertionError(f"Wt[ci {bad[0]}][tap {bad[1]}][co {bad[2]}] holds {float(h.view(Cin, 9, Cout)[tuple(bad)])}, not {float(w[bad[2], bad[1], bad[0]])}")
        assert torch.equal(got, want), int((got != want).sum())


def test_split_wt_rejections(gpu, lib):
    L, l = lib, lib.load()
    wb, wp = flat_in(torch.ones(64 * 9 * 64), gpu)
    ob, op = u16_out(2 * 64 * 9 * 64, gpu)
    for args in ((wp, 48, 64, op), (wp, 64, 48, op), (wp, 64, 64, op + 64), (wp, 64, 64, op + 2)):
        assert l.bd_split_wt(*args, L.stream()) == UNSUPPORTED, args
    assert l.bd_split_wt(wp, 0, 64, op, L.stream()) == INVALID
    assert u16_untouched(ob)


# ================================================================================================ 5. the loss launchers
LOSS_ROWS, LOSS_C = 6, 8


def loss_buffers(L, l, gpu, n_losses):
    pred, tgt = torch.zeros(LOSS_ROWS * (LOSS_C + 4), device=gpu), torch.ones(LOSS_ROWS * (LOSS_C + 4), device=gpu)
    loss = torch.full((LEAD + n_losses + TRAIL,), S.NAN, device=gpu)
    dp = torch.full((LOSS_ROWS * (LOSS_C + 4) + 8,), S.NAN, device=gpu)
    return pred, tgt, loss, dp


def test_loss_fwd_bwd_refuses_short_ld(gpu, lib):
    L, l = lib, lib.load()
    pred, tgt, loss, dp = loss_buffers(L, l, gpu, 1)
    ws = torch.empty(l.bd_reduce_workspace_bytes(), dtype=torch.uint8, device=gpu)
    C, lp = LOSS_C, loss[LEAD:].data_ptr()
    for ldp, ldt, lddp, dpp in ((C - 1, C, C, dp.data_ptr()), (C, C - 1, C, dp.data_ptr()), (C, C, C - 1, dp.data_ptr()), (C - 4, C, C, None), (C, 0, 0, None)):
        assert l.bd_loss_fwd_bwd(pred.data_ptr(), ldp, tgt.data_ptr(), ldt, LOSS_ROWS, C, 0, 1.0, lp, dpp, lddp, ws.data_ptr(), L.stream()) == INVALID, (ldp, ldt, lddp)
        assert b"< C" in l.bd_last_error()
    assert untouched(loss, dp)
    # the legal call without dpred does not look at lddp
    L.check(l.bd_loss_fwd_bwd(pred.data_ptr(), C + 4, tgt.data_ptr(), C, LOSS_ROWS, C, 0, 1.0, lp, None, 0, ws.data_ptr(), L.stream()), "bd_loss_fwd_bwd")
    torch.cuda.synchronize()
    assert float(loss[LEAD]) == 1.0 and untouched(loss[:LEAD], loss[LEAD + 1:], dp)


def test_loss_groups_fwd_bwd_refuses_short_ld(gpu, lib):
    L, l = lib, lib.load()
    pred, tgt, loss, dp = loss_buffers(L, l, gpu, 3)
    g = L.LossGroupsDesc(n_groups=2)
    g.group_rows[0], g.group_rows[1] = 2, LOSS_ROWS - 2
    g.group_weight[0], g.group_weight[1] = 1.0, 0.5
    nbytes = l.bd_loss_groups_workspace_bytes(2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    C, lp = LOSS_C, loss[LEAD:].data_ptr()
    for ldp, ldt, lddp, dpp in ((C - 1, C, C, dp.data_ptr()), (C, C - 1, C, dp.data_ptr()), (C, C, C - 1, dp.data_ptr()), (C - 4, C, C, None), (C, 0, 0, None)):
        assert l.bd_loss_groups_fwd_bwd(pred.data_ptr(), ldp, tgt.data_ptr(), ldt, LOSS_ROWS, C, 0, 1.0, CT.byref(g), lp, dpp, lddp, ws.data_ptr(), nbytes,
                                        L.stream()) == INVALID, (ldp, ldt, lddp)
        assert b"< C" in l.bd_last_error()
    assert untouched(loss, dp)
    L.check(l.bd_loss_groups_fwd_bwd(pred.data_ptr(), C + 4, tgt.data_ptr(), C, LOSS_ROWS, C, 0, 1.0, CT.byref(g), lp, None, 0, ws.data_ptr(), nbytes, L.stream()),
            "bd_loss_groups_fwd_bwd")
    torch.cuda.synchronize()
    assert loss[LEAD: LEAD + 3].tolist() == [1.0, 1.0, 1.5] and untouched(loss[:LEAD], loss[LEAD + 3:], dp)
