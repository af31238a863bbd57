"""GPU: dynamic thresholding for DDPM and DDIM on the native path -- bd_abs_quantile held to torch.quantile's bits (tests/golden/
threshold.npz) at every path and path switch, in every data regime, from offset buffers and in its on-the-fly form; the thresholded
bd_ddpm_step / bd_ddim_step held to equal bits against their numpy-float32 statement (tests/_threshold_exact.py) and within the sibling
bound of the reference's stored outputs; the schedulers against the reference's chains with a stand-in model and with the product UNet;
the pipelines, backdoor_scores and the command line end to end.  Run with -m gpu on an MI355X."""
import ctypes
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_ref as U
from tests import _step_exact as X
from tests import _threshold_exact as T
from tests.golden import cases as C
from tests.golden import cases_threshold as CT
from tests.golden.cases_sigma import trigger

f32 = np.float32
SENTINEL = -777.0
MARGIN = 64
INVALID = -1


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def table(gpu):
    _, ac = X.tables()
    return ac, torch.from_numpy(ac).cuda()


def place(v, lead):
    """a device copy of the numpy array v that starts `lead` floats into a fresh allocation (lead = 1: 4 bytes past a 16-byte boundary),
    sentinels around it: (whole buffer, view of v's shape)"""
    v = np.ascontiguousarray(v, dtype=f32)
    buf = torch.full((lead + v.size + MARGIN,), SENTINEL, device="cuda")
    view = buf[lead: lead + v.size].view(v.shape)
    view.copy_(torch.from_numpy(v))
    assert view.data_ptr() % 16 == (4 * lead) % 16
    return buf, view


def blank(shape, lead):
    n = int(np.prod(shape))
    buf = torch.full((lead + n + MARGIN,), SENTINEL, device="cuda")
    return buf, buf[lead: lead + n].view(shape)


def margins_untouched(buf, lead, n):
    return bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + n:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------- bd_abs_quantile
@pytest.mark.parametrize("shape", CT.Q_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_quantile_equals_torch_quantile(gpu, golden, shape):
    """equal bits against torch.quantile on the CPU in every regime and at every ratio; the first regime again from a buffer that starts
    one element past a 16-byte boundary.  The shapes straddle the path switch the plan query reports"""
    from baddiffusion_amd import ops
    B, m = shape
    g = golden("threshold")
    plan = ops.abs_quantile_plan(B, m)
    assert plan["switch_m"] == CT.SWITCH_M and plan["path"] == (0 if m <= CT.SWITCH_M else 1)
    for regime in CT.REGIMES:
        x = CT.quantile_input(B, m, regime)
        xd = x.cuda()
        for q in CT.QS:
            got = ops.abs_quantile(xd, q)
            assert got.shape == (B,) and got.dtype == torch.float32
            CT.assert_nan_equal_bits(got.cpu().numpy(), CT.quantile_expected(g, B, m, regime, q))
        assert torch.equal(xd.cpu().view(torch.int32), x.view(torch.int32))                  # the input is left as it was
    buf, view = place(CT.quantile_input(B, m, "normal0").numpy(), 1)
    for q in CT.QS:
        CT.assert_nan_equal_bits(ops.abs_quantile(view, q).cpu().numpy(), CT.quantile_expected(g, B, m, "normal0", q))
    assert margins_untouched(buf, 1, B * m)


@pytest.mark.parametrize("shape,t", (((2, 3, 8, 8), 500), ((3, 3, 5, 7), 999), ((2, 3, 32, 32), 1), ((2, 3, 37, 37), 0), ((2, 3, 40, 40), 980)),
                         ids=lambda v: str(v))
def test_on_the_fly_source_ranks_the_x0_the_step_clamps(gpu, table, shape, t):
    """abs_quantile(x, model_output=e, t) equals abs_quantile of the pred_original that bd_ddpm_step (and bd_ddim_step) returns with
    thresholding and clipping off, bit for bit, in both layouts and from offset buffers: the kernels form x0 in one helper.
    m = 192, 105, 3072 (registers), 4107 and 4800 (stream)"""
    from baddiffusion_amd import ops
    ac, acd = table
    x = torch.randn(shape, generator=torch.Generator().manual_seed(41)).numpy() * 2
    e = torch.randn(shape, generator=torch.Generator().manual_seed(42)).numpy()
    want_x0 = T.x0_stmt(ac, t, x, e)
    for lead in (0, 1):
        (_, xd), (_, ed) = place(x, lead), place(e, lead)
        noise = torch.zeros_like(xd)
        _, x0_ddpm = ops.ddpm_step(ed, xd, noise, acd, t, t - 1, clip_sample=False, want_x0=True)
        _, x0_ddim = ops.ddim_step(ed, xd, acd, t, t - 20, clip_sample=False, want_x0=True)
        assert X.same_bits(x0_ddpm, torch.from_numpy(want_x0)) and X.same_bits(x0_ddim, x0_ddpm)
        for q in (0.995, 0.5):
            fly = ops.abs_quantile(xd, q, model_output=ed, alphas_cumprod=acd, t=t)
            assert X.same_bits(fly, ops.abs_quantile(x0_ddpm, q))
            CT.assert_nan_equal_bits(fly.cpu().numpy(), T.abs_quantile_stmt(want_x0, q))
    # channels_last storage: dimension 0 is still outermost, and a quantile does not depend on the order inside an image
    xc, ec = (torch.from_numpy(v).cuda().contiguous(memory_format=torch.channels_last) for v in (x, e))
    assert xc.shape[1] == 1 or not xc.is_contiguous()
    assert X.same_bits(ops.abs_quantile(xc, 0.995, model_output=ec, alphas_cumprod=acd, t=t), ops.abs_quantile(torch.from_numpy(want_x0).cuda(), 0.995))


def test_quantile_rejections_leave_the_output_untouched(gpu, table):
    from baddiffusion_amd import _lib as L
    from baddiffusion_amd import ops
    lib = L.load()
    _, acd = table
    x = torch.randn(2, 192, device="cuda")
    out = torch.full((2,), SENTINEL, device="cuda")
    base = dict(B=2, m=192, x=x.data_ptr(), out=out.data_ptr(), q=0.5)
    for kw, what in ((dict(q=1.5), b"must lie in [0, 1]"), (dict(q=float("nan")), b"must lie in [0, 1]"), (dict(B=0), b"must be positive"),
                     (dict(m=0), b"must be positive"), (dict(model_output=x.data_ptr(), alphas_cumprod=acd.data_ptr(), n_alphas=1000, t=1000),
                                                        b"outside the table"),
                     (dict(model_output=x.data_ptr()), b"without alphas_cumprod")):
        assert lib.bd_abs_quantile(ctypes.byref(L.AbsQuantileDesc(**{**base, **kw})), L.stream()) == INVALID and what in lib.bd_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(ValueError, match="dimension 0 outermost"):
        ops.abs_quantile(torch.randn(4, 6, device="cuda").t(), 0.5)
    with pytest.raises(ValueError, match="share shape, strides"):
        ops.abs_quantile(x, 0.5, model_output=x[:1], alphas_cumprod=acd, t=5)
    with pytest.raises(TypeError, match="float32"):
        ops.abs_quantile(x.double(), 0.5)
    with pytest.raises(RuntimeError, match="t=1000 outside the table of 1000"):
        ops.abs_quantile(x, 0.5, model_output=x, alphas_cumprod=acd, t=1000)
    assert lib.bd_abs_quantile_workspace_bytes(2048, 3072) == 0 and lib.bd_abs_quantile_workspace_bytes(4, 196608) == 0


# ---------------------------------------------------------------------------------------------------- thresholded steps
def run_step(sched, case, x, e, z, q, acd, lead=0, channels_last=False):
    """(prev, pred_original) on the host in NCHW order, from one thresholded ops.ddpm_step / ops.ddim_step call on device copies that start
    `lead` floats into their buffers, in plain or channels_last storage"""
    from baddiffusion_amd import ops
    t, kind, smax, _, shape = case
    to_store = (lambda v: np.ascontiguousarray(v.transpose(0, 2, 3, 1))) if channels_last else (lambda v: v)
    (_, xd), (_, ed), (_, zd) = (place(to_store(v), lead) for v in (x, e, z))
    pbuf, pd = blank(xd.shape, lead)
    qd = torch.from_numpy(np.asarray(q, dtype=f32)).cuda()
    if sched == "ddpm":
        prev, x0 = ops.ddpm_step(ed, xd, zd, acd, t, t - 1, variance_type=kind, clip_sample=True, out=pd, want_x0=True, x0_quantile=qd,
                                 sample_max_value=smax)
    else:
        prev, x0 = ops.ddim_step(ed, xd, acd, t, t - 1000 // CT.DDIM_STEPS, eta=kind, noise=zd if kind > 0 else None, clip_sample=True, out=pd,
                                 want_x0=True, x0_quantile=qd, sample_max_value=smax)
    assert prev is pd and margins_untouched(pbuf, lead, x.size)
    back = (lambda v: v.cpu().numpy().transpose(0, 3, 1, 2)) if channels_last else (lambda v: v.cpu().numpy())
    return back(prev), back(x0)


def stmt(sched, ac, case, x, e, z):
    t, kind, smax, ratio, _ = case
    if sched == "ddpm":
        return T.ddpm_thr_stmt(ac, T.ddpm_case(t, t - 1, kind), x, e, z, smax, ratio)
    return T.ddim_thr_stmt(ac, T.ddim_case(t, t - 1000 // CT.DDIM_STEPS, kind), x, e, z, smax, ratio)


@pytest.mark.parametrize("sched", ("ddpm", "ddim"))
def test_thresholded_steps_equal_their_statement_and_the_reference(gpu, golden, table, sched):
    """every step case: the quantile launch (on-the-fly form) and the thresholded step launch against the numpy-float32 statement, EQUAL
    BITS, rotating through plain / offset / channels_last buffers; and within 2e-6 (rtol and atol, the bound of
    test_ddpm_ddim_steps_golden) of the reference scheduler's stored outputs.  clip_sample=True is passed and must be ignored"""
    from baddiffusion_amd import ops
    ac, acd = table
    g = golden("threshold")
    cases = CT.DDPM_STEP_CASES if sched == "ddpm" else CT.DDIM_STEP_CASES
    worst = 0.0
    for i, case in enumerate(cases):
        t, kind, smax, ratio, shape = case
        x, e, z = (v.numpy() for v in CT.step_inputs(sched, i, case, torch.from_numpy(ac)))
        want_prev, want_x0, want_q = stmt(sched, ac, case, x, e, z)
        q = ops.abs_quantile(torch.from_numpy(x).cuda(), ratio, model_output=torch.from_numpy(e).cuda(), alphas_cumprod=acd, t=t).cpu().numpy()
        CT.assert_nan_equal_bits(q, want_q)
        lead, cl = ((0, False), (1, False), (0, True), (1, True))[i % 4]
        prev, x0 = run_step(sched, case, x, e, z, q, acd, lead=lead, channels_last=cl)
        assert X.same_bits(prev, want_prev) and X.same_bits(x0, want_x0), (case, lead, cl)
        ref_prev, ref_x0 = CT.step_expected(g, sched, i)
        np.testing.assert_allclose(prev, ref_prev, rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(x0, ref_x0, rtol=2e-6, atol=2e-6)
        worst = max(worst, float(np.abs(prev - ref_prev).max()), float(np.abs(x0 - ref_x0).max()))
    print(f"MEASURE thresholded {sched} steps: {len(cases)} cases, worst |got - reference| {worst:.3e}")


def test_thresholded_steps_on_a_second_trip_of_the_grid(gpu, table):
    """342 images of 3072 elements: 1 050 624 elements, past one trip of the capped grid (4096 blocks of 256 threads), so the image
    index is formed on both trips; quantiles from the registers path at more images than compute units.  Equal bits"""
    from baddiffusion_amd import ops
    ac, acd = table
    B, shape = 342, (342, 3, 32, 32)
    assert B * 3072 > X.STEP_CAP * X.TPB and B * 3072 < 2 * X.STEP_CAP * X.TPB
    gen = lambda s: torch.randn(shape, generator=torch.Generator().manual_seed(s))      # noqa: E731
    scale = torch.tensor([(0.25, 0.45, 1.2)[b % 3] for b in range(B)]).view(-1, 1, 1, 1)      # quantiles below 1, inside (1, 1.5), above
    e, z = gen(52).numpy(), gen(53).numpy()
    for sched, case in (("ddpm", (500, "fixed_small", 1.5, 0.995, shape)), ("ddim", (500, 0.5, 1.5, 0.995, shape))):
        a_t = float(ac[500])
        x = (np.sqrt(a_t) * (gen(51) * scale).numpy() + np.sqrt(1 - a_t) * e).astype(f32)
        want_prev, want_x0, want_q = stmt(sched, ac, case, x, e, z)
        assert {CT.regime_of(float(v), 1.5) for v in want_q} == {0, 1, 2}
        q = ops.abs_quantile(torch.from_numpy(x).cuda(), 0.995, model_output=torch.from_numpy(e).cuda(), alphas_cumprod=acd, t=500).cpu().numpy()
        CT.assert_nan_equal_bits(q, want_q)
        prev, x0 = run_step(sched, case, x, e, z, q, acd)
        assert X.same_bits(prev, want_prev) and X.same_bits(x0, want_x0), sched


def test_nan_quantile_and_clip_defense(gpu, table):
    """a NaN quantile stays NaN (its whole image becomes NaN, the others are untouched by it); clip_defense still applies to prev_sample"""
    from baddiffusion_amd import ops
    ac, acd = table
    case = (500, "fixed_small", 1.5, 0.995, CT.SHAPE_A)
    x, e, z = (v.numpy() for v in CT.step_inputs("ddpm", 2, case, torch.from_numpy(ac)))
    q = np.array([np.nan, 1.25], dtype=f32)
    want_prev, want_x0, _ = T.ddpm_thr_stmt(ac, T.ddpm_case(500, 499, "fixed_small"), x, e, z, 1.5, q=q)
    prev, x0 = run_step("ddpm", case, x, e, z, q, acd)
    assert np.isnan(prev[0]).all() and np.isnan(x0[0]).all() and X.same_bits(prev[1], want_prev[1]) and X.same_bits(x0[1], want_x0[1])
    xd, ed, zd = (torch.from_numpy(v).cuda() for v in (x, e, z))
    qd = torch.tensor([0.8, 1.25], device="cuda")
    prev, x0 = ops.ddpm_step(ed, xd, zd, acd, 500, 499, clip_sample=False, clip_defense=True, clip_defense_range=0.5, want_x0=True,
                             x0_quantile=qd, sample_max_value=1.5)
    want_prev, want_x0, _ = T.ddpm_thr_stmt(ac, T.ddpm_case(500, 499, "fixed_small", cdef=0.5), x, e, z, 1.5, q=qd.cpu().numpy())
    assert X.same_bits(prev, torch.from_numpy(want_prev)) and X.same_bits(x0, torch.from_numpy(want_x0))
    assert float(prev.abs().max()) == 0.5 and float(x0.abs().max()) <= 1.0


@pytest.mark.parametrize("kind", ("ddpm", "ddim"))
def test_null_quantile_reproduces_the_existing_exact_cases(gpu, table, kind):
    """x0_quantile = NULL (the fields at their zero defaults, and with stray values in the two others): the bits of the existing exact
    cases (tests/_step_exact.py), clip_sample and all"""
    from baddiffusion_amd import _lib as L
    lib = L.load()
    ac, acd = table
    cases, coef, statement = (X.ddpm_cases, X.ddpm_coef, X.ddpm_stmt) if kind == "ddpm" else (X.ddim_cases, X.ddim_coef, X.ddim_stmt)
    for j, c in enumerate(cases()):
        sb, sa = coef(ac, c)[:2]
        x, e, z, _ = X.step_data(257, sb, sa, c.clip, 100 + j)
        xd, ed, zd = (torch.from_numpy(v).cuda() for v in (x, e, z))
        pd, od = torch.empty_like(xd), torch.empty_like(xd)
        common = dict(n=257, model_output=ed.data_ptr(), sample=xd.data_ptr(), prev_sample=pd.data_ptr(), pred_original=od.data_ptr(),
                      alphas_cumprod=acd.data_ptr(), t=c.t, prev_t=c.prev_t, clip_sample=int(c.clip is not None), clip_sample_range=c.clip or 0.0,
                      x0_quantile=None, image_elems=(0, 7)[j % 2], sample_max_value=(0.0, 3.0)[j % 2])
        if kind == "ddpm":
            d = L.DdpmStepDesc(noise=zd.data_ptr(), variance_type=c.vt, clip_defense=int(c.cdef is not None), clip_defense_range=c.cdef or 0.0, **common)
            assert lib.bd_ddpm_step(ctypes.byref(d), L.stream()) == 0
        else:
            d = L.DdimStepDesc(noise=zd.data_ptr() if c.eta > 0 else None, final_alpha_cumprod=c.final, eta=c.eta, **common)
            assert lib.bd_ddim_step(ctypes.byref(d), L.stream()) == 0
        want_prev, want_x0 = statement(ac, c, x, e, z)
        assert X.same_bits(pd, torch.from_numpy(want_prev)) and X.same_bits(od, torch.from_numpy(want_x0)), (kind, j)


def test_step_rejections_leave_the_outputs_untouched(gpu, table):
    from baddiffusion_amd import _lib as L
    from baddiffusion_amd import ops
    lib = L.load()
    _, acd = table
    x = torch.randn(2, 3, 8, 8, device="cuda")
    prev, x0 = torch.full_like(x, SENTINEL), torch.full_like(x, SENTINEL)
    q = torch.ones(2, device="cuda")
    common = dict(n=384, model_output=x.data_ptr(), sample=x.data_ptr(), noise=x.data_ptr(), prev_sample=prev.data_ptr(), pred_original=x0.data_ptr(),
                  alphas_cumprod=acd.data_ptr(), t=500, prev_t=499, x0_quantile=q.data_ptr(), sample_max_value=1.5)
    for fn, cls in ((lib.bd_ddpm_step, L.DdpmStepDesc), (lib.bd_ddim_step, L.DdimStepDesc)):
        for elems in (0, 100, 385, -192):
            assert fn(ctypes.byref(cls(image_elems=elems, **common)), L.stream()) == INVALID and b"image_elems" in lib.bd_last_error()
    torch.cuda.synchronize()
    assert bool((prev == SENTINEL).all()) and bool((x0 == SENTINEL).all())
    with pytest.raises(ValueError, match=r"x0_quantile must be a contiguous float32 \[2\]"):
        ops.ddpm_step(x, x, x, acd, 500, 499, x0_quantile=torch.ones(3, device="cuda"))
    with pytest.raises(ValueError, match="x0_quantile must be"):
        ops.ddim_step(x, x, acd, 500, 480, x0_quantile=torch.ones(2, device="cuda", dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------- schedulers
def make_scheduler(sched, smax, ratio=CT.CHAIN_RATIO):
    from baddiffusion_amd.schedulers import DDIMScheduler, DDPMScheduler
    return (DDIMScheduler if sched == "ddim" else DDPMScheduler)(**CT.scheduler_kwargs(smax, ratio))


@pytest.mark.parametrize("case", CT.CHAIN_CASES, ids=lambda c: CT.chain_tag(*c))
def test_stand_in_chain(gpu, golden, case):
    """scheduler.step with cases.pndm_fake_model in place of the UNet, in plain and channels_last layout: every intermediate sample within
    max(4e-6, 4 * dev64) * max|ref| of the reference's, dev64 being the reference's own distance from the recurrence in float64.  The
    quantiles of these chains run from 57 down to 0.75 and pass through all three regimes"""
    sched, smax = case
    g, tag = golden("threshold"), CT.chain_tag(sched, smax)
    ref, dev64 = g[tag], float(g[f"{tag}_dev64"])
    bound = max(4e-6, 4 * dev64)
    s = make_scheduler(sched, smax)
    for layout in ("plain", "channels_last"):
        s.set_timesteps(CT.CHAIN_STEPS)
        gen = torch.Generator().manual_seed(CT.CHAIN_NOISE_SEED)
        x = C.pndm_init().cuda()
        if layout == "channels_last":
            x = x.contiguous(memory_format=torch.channels_last)
        worst = 0.0
        for i, t in enumerate(s.timesteps.tolist()):
            x_in = x.clone()
            out = s.step(C.pndm_fake_model(x, t), t, x, generator=gen)
            y = out.prev_sample
            assert y.shape == (2, 3, 8, 8) and y.is_contiguous() == (layout == "plain")
            assert torch.equal(x, x_in) and float(out.pred_original_sample.abs().max()) <= 1.0
            x = y
            dev = float(np.abs(x.cpu().numpy() - ref[i]).max() / np.abs(ref[i]).max())
            worst = max(worst, dev)
            assert dev <= bound, (layout, i, t, dev, bound)
        print(f"MEASURE thresholded stand-in chain {tag} {layout}: worst step deviation {worst:.3e}, bound {bound:.3e} (reference vs fp64 {dev64:.3e})")


def test_threshold_sample_has_the_reference_semantics(gpu):
    for sched in ("ddpm", "ddim"):
        s = make_scheduler(sched, 1.5, 0.9)
        x = (torch.randn(3, 3, 5, 7, generator=torch.Generator().manual_seed(9)) * torch.tensor([0.3, 0.8, 2.0]).view(3, 1, 1, 1))
        flat = x.reshape(3, -1)
        q = torch.quantile(flat.abs(), 0.9, dim=1).clamp(min=1, max=1.5).unsqueeze(1)
        want = (torch.clamp(flat, -q, q) / q).reshape(x.shape)
        assert sorted({CT.regime_of(float(v), 1.5) for v in torch.quantile(flat.abs(), 0.9, dim=1)}) == [0, 1, 2]
        got = s._threshold_sample(x.cuda())
        assert X.same_bits(got, want)
        cl = s._threshold_sample(x.cuda().contiguous(memory_format=torch.channels_last))
        assert cl.shape == x.shape and X.same_bits(cl.contiguous(), want)
        with pytest.raises(RuntimeError, match="GPU only"):
            s._threshold_sample(x)


def make_model(mode=None, sample_size=None):
    from baddiffusion_amd.unet import unet_from_config
    cfg = C.SMALL_CFGS[CT.UNET_CFG]
    if sample_size is not None:
        cfg = dataclasses.replace(cfg, sample_size=sample_size)
    m = unet_from_config(cfg).cuda()
    m.load_state_dict(U.gen_params(cfg, CT.UNET_PARAM_SEED))
    return m.set_compute_mode(mode) if mode else m


@pytest.fixture(scope="module")
def models(gpu):
    return {"f32": make_model("f32"), "bf16x3": make_model("bf16x3")}


@pytest.mark.parametrize("mode", ("f32", "bf16x3"))
@pytest.mark.parametrize("trig", CT.UNET_CASES, ids=("noise", "trigger"))
def test_unet_chain_vs_reference_raw_sample(gpu, golden, models, trig, mode):
    """the reference DDIMScheduler(thresholding=True, sample_max_value=1.5) around the reference UNet against the product's scheduler
    around the product's UNet, from noise and from noise + trigger: the RAW final sample within 1e-3 * max|ref|"""
    from baddiffusion_amd import ops
    ref = golden("threshold")[f"{CT.unet_tag(trig)}_sample"]
    cfg = C.SMALL_CFGS[CT.UNET_CFG]
    init = C.pipeline_init(cfg, CT.UNET_BATCH)
    if trig:
        init = init + trigger(cfg)
    s = make_scheduler("ddim", CT.UNET_SMAX)
    s.set_timesteps(CT.UNET_STEPS)
    x = ops.nchw_to_nhwc(init.cuda().float())
    ts_dev = torch.as_tensor(s.timesteps, dtype=torch.int64).cuda()
    with torch.no_grad():
        for i, t in enumerate(s.timesteps):
            eps = models[mode](x.permute(0, 3, 1, 2), ts_dev[i]).sample
            x = s.step(eps, int(t), x.permute(0, 3, 1, 2)).prev_sample.permute(0, 2, 3, 1)
    got = x.permute(0, 3, 1, 2).cpu().numpy()
    dev = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"MEASURE thresholded unet chain {CT.unet_tag(trig)} {mode}: max |x - ref| / max|ref| {dev:.3e} (bound 1e-3, max|ref| {np.abs(ref).max():.2f})")
    assert dev <= 1e-3


# ---------------------------------------------------------------------------------------------------- end to end
def test_pipelines_with_a_thresholding_scheduler(gpu, models):
    """DDPMPipeline and DDIMPipeline run a thresholding scheduler (they raised NotImplementedError on the first step before); the images
    differ from the fixed clamp's and equal the loop restated with ops.abs_quantile + the thresholded step"""
    from baddiffusion_amd import ops
    from baddiffusion_amd.pipelines import DDIMPipeline, DDPMPipeline
    from baddiffusion_amd.schedulers import DDIMScheduler, DDPMScheduler
    model = models["f32"]
    init = C.pipeline_init(C.SMALL_CFGS[CT.UNET_CFG], 2)
    thr = DDIMPipeline(model, DDIMScheduler(**CT.scheduler_kwargs(1.5)))
    assert thr.scheduler.config.thresholding is True and thr.scheduler.config.sample_max_value == 1.5
    a = thr(init=init, num_inference_steps=10, output_type="numpy").images
    b = DDIMPipeline(model, DDIMScheduler(clip_sample=True))(init=init, num_inference_steps=10, output_type="numpy").images
    assert a.shape == (2, 16, 16, 3) and np.isfinite(a).all() and not np.array_equal(a, b)
    # the loop by hand
    s = DDIMScheduler(**CT.scheduler_kwargs(1.5))
    s.set_timesteps(10)
    _, acd = s.device_tables(torch.device("cuda"))
    x = ops.nchw_to_nhwc(init.cuda().float())
    with torch.no_grad():
        for t in s.timesteps.tolist():
            eps = model(x.permute(0, 3, 1, 2), torch.tensor(t, device="cuda")).sample.permute(0, 2, 3, 1).contiguous()
            q = ops.abs_quantile(x, 0.995, model_output=eps, alphas_cumprod=acd, t=t)
            x = ops.ddim_step(eps, x, acd, t, t - 100, x0_quantile=q, sample_max_value=1.5)
    assert np.array_equal(a, (x / 2 + 0.5).clamp(0, 1).cpu().numpy())
    g = torch.Generator().manual_seed(5)
    c = DDPMPipeline(model, DDPMScheduler(**CT.scheduler_kwargs(3.0, 0.9)))(init=init, generator=g, num_inference_steps=10, output_type="numpy").images
    g = torch.Generator().manual_seed(5)
    d = DDPMPipeline(model, DDPMScheduler(clip_sample=True))(init=init, generator=g, num_inference_steps=10, output_type="numpy").images
    assert c.shape == (2, 16, 16, 3) and np.isfinite(c).all() and not np.array_equal(c, d)


def test_backdoor_scores_with_a_thresholding_pipeline(gpu, models):
    from baddiffusion_amd import defense
    from baddiffusion_amd.pipelines import DDIMPipeline
    from baddiffusion_amd.schedulers import DDIMScheduler
    cfg = C.SMALL_CFGS[CT.UNET_CFG]
    pipe = DDIMPipeline(models["f32"], DDIMScheduler(**CT.scheduler_kwargs(1.5)))
    sc = defense.backdoor_scores(pipe, trigger(cfg).cuda(), n=4, init=C.pipeline_init(cfg, 4).cuda(), max_batch_n=4, num_inference_steps=5)
    assert {"uniformity_clean", "uniformity_trigger", "tv_clean", "tv_trigger", "uniformity_ratio"} <= set(sc)
    assert all(np.isfinite(v) for v in sc.values())


def test_command_line_sampling_with_dyn_threshold(gpu, tmp_path, monkeypatch):
    """baddiffusion.py --mode sampling --dyn_threshold 1.5 on a run directory of the small network: the pipeline it samples with carries
    the thresholding config, the grids are written and sampling.json records the flag"""
    import baddiffusion as cli
    from baddiffusion_amd.model import save_scheduler, save_unet
    from baddiffusion_amd.schedulers import DDPMScheduler
    run = str(tmp_path / "run")
    save_unet(make_model(sample_size=32), os.path.join(run, "unet"))
    save_scheduler(DDPMScheduler(clip_sample=False), os.path.join(run, "scheduler"))
    json.dump({"dataset": "CIFAR10", "batch": 64, "ckpt": "local", "project": "default"}, open(os.path.join(run, "args.json"), "w"))
    monkeypatch.setenv("BD_NUM_IMAGES", "16")
    monkeypatch.chdir(tmp_path)
    seen = []
    real = cli.sampling

    def spy(cfg, name, pipeline, dsl):
        seen.append(dict(pipeline.scheduler.config))
        return real(cfg, name, pipeline, dsl)
    monkeypatch.setattr(cli, "sampling", spy)
    cli.main(["--mode", "sampling", "--ckpt", run, "--sched", "DDIM-SCHED", "--infer_steps", "4", "--dyn_threshold", "1.5"])
    assert len(seen) == 1 and (seen[0]["thresholding"], seen[0]["sample_max_value"], seen[0]["dynamic_thresholding_ratio"]) == (True, 1.5, 0.995)
    rec = json.load(open(os.path.join(run, "sampling.json")))
    assert rec["dyn_threshold"] == 1.5 and rec["dyn_threshold_ratio"] == 0.995
    for folder in ("samples", "backdoor_samples"):
        assert any(f.endswith(".png") for f in os.listdir(os.path.join(run, folder)))
