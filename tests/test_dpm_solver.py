"""GPU: DPM-Solver(++) sampling on the native path -- bd_dpm_step against its formula in fp64 at the sizes where the launcher changes
path, its clamps and permitted aliasings (bit-exact properties), DPMSolverMultistepScheduler against the reference's chains
(tests/golden/dpm_solver.npz, written by make_golden_dpm.py from the imported diffusers DPMSolverMultistepScheduler), with a stand-in
model and with the product UNet, and DPMSolverPipeline's surface.  Run with -m gpu on an MI355X."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_ref as U
from tests.golden import cases as C
from tests.golden import cases_dpm as CD

TOL = 2e-6          # rtol = atol of the sibling step kernels' tests (test_repaint.py, test_ddpm_ddim_steps_golden)
# moderate scalars (a mid-chain step has |c| of this order): with |inputs| <= 6 every rounding of the formula is below 2.4e-7 (half an
# ulp of a value below 8) and at most 6 of them reach the result with weights <= 1, so the fp32 result is within TOL of the fp64 one
ALPHA_S, SIGMA_S, CX, C0, C1, C2 = 0.8, 0.6, 0.9, 0.35, -0.5, 0.2
BIG = 4 * 4096 * 256 + 4 * 256 + 3          # a second grid-stride pass of the 4096-block grid, plus a scalar tail


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def R(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def formula64(e, x, m1, m2, convert, x0_clip, clip):
    """bd_dpm_step's formula (include/bd_hip.h) in fp64 on the fp32 inputs and the fp32 values of the scalars: (m0, prev)"""
    f = lambda v: float(np.float32(v))
    e, x = e.double(), x.double()
    m0 = (x - f(SIGMA_S) * e) / f(ALPHA_S) if convert else e
    if x0_clip is not None:
        m0 = m0.clamp(-f(x0_clip), f(x0_clip))
    prev = f(CX) * x + f(C0) * m0
    if m1 is not None:
        prev = prev + f(C1) * m1.double()
    if m2 is not None:
        prev = prev + f(C2) * m2.double()
    if clip is not None:
        prev = prev.clamp(-f(clip), f(clip))
    return m0, prev


def run(e, x, m1, m2, convert, x0_clip=None, clip=None, want_m0=True, out=None, m0_out=None):
    from baddiffusion_amd import ops
    if want_m0 and m0_out is None:
        m0_out = torch.empty_like(x)
    prev = ops.dpm_step(e, x, CX, C0, m1=m1, c1=C1, m2=m2, c2=C2, convert=(ALPHA_S, SIGMA_S) if convert else None, x0_clip=x0_clip,
                        clip=clip, m0_out=m0_out if want_m0 else None, out=out)
    return m0_out if want_m0 else None, prev


def close(a, b):
    np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.detach().cpu().numpy(), rtol=TOL, atol=TOL)


# ---------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("n", (1, 3, 4, 7, 1027, BIG))
def test_step_kernel_against_the_fp64_formula(gpu, n):
    """every size at which the launch changes shape: tail only (1, 3), body only (4), body + tail (7, 1027: several blocks), and a
    second grid-stride pass + tail; both conversions, absent m1 / m2, m0 not written"""
    e, x, m1, m2 = (R(s, n) for s in (1, 2, 3, 4))
    ed, xd, m1d, m2d = (t.cuda() for t in (e, x, m1, m2))
    options = [(True, True, True, True), (False, True, True, True), (True, True, False, True), (False, False, False, True),
               (True, False, False, False)] if n != BIG else [(True, True, True, True), (False, True, False, False)]
    for convert, has1, has2, want_m0 in options:
        a, b = (m1 if has1 else None), (m2 if has2 else None)
        m0, prev = run(ed, xd, m1d if has1 else None, m2d if has2 else None, convert, want_m0=want_m0)
        m0_64, prev_64 = formula64(e, x, a, b, convert, None, None)
        close(prev, prev_64)
        if want_m0:
            close(m0, m0_64)
            if not convert:
                assert torch.equal(m0, ed)                                   # the eps prediction is stored as it is
        else:
            assert m0 is None
    # the inputs are left as they were
    assert torch.equal(ed.cpu(), e) and torch.equal(xd.cpu(), x) and torch.equal(m1d.cpu(), m1) and torch.equal(m2d.cpu(), m2)


def test_step_kernel_clamps(gpu):
    e, x, m1, m2 = (R(s, 2, 3, 9, 7).cuda() for s in (5, 6, 7, 8))              # 378 elements: body + a tail of 2
    m0_plain, prev_plain = run(e, x, m1, m2, True)
    # post-step clamp: exactly the clamp of the unclipped result; m0 is untouched by it
    for r in (1.0, 0.37):
        m0, prev = run(e, x, m1, m2, True, clip=r)
        assert torch.equal(prev, prev_plain.clamp(-r, r)) and torch.equal(m0, m0_plain)
        assert float(prev.abs().max()) == float(np.float32(r))
    # x0 clamp: the stored m0 is exactly the clamp of the unclipped one, and prev is built from the clamped value
    for r in (1.0, 0.5):
        m0, prev = run(e, x, m1, m2, True, x0_clip=r)
        assert torch.equal(m0, m0_plain.clamp(-r, r)) and float(m0.abs().max()) == r
        close(prev, formula64(e.cpu(), x.cpu(), m1.cpu(), m2.cpu(), True, r, None)[1])
        assert not torch.equal(prev, prev_plain)
        both = run(e, x, m1, m2, True, x0_clip=r, clip=0.8)[1]
        assert torch.equal(both, prev.clamp(-0.8, 0.8))
    # without the conversion the x0 clamp still applies to m0 = eps
    m0, _ = run(e, x, None, None, False, x0_clip=1.0)
    assert torch.equal(m0, e.clamp(-1, 1))


def test_step_kernel_layouts_and_checks(gpu):
    from baddiffusion_amd import ops
    e, x, m1 = (R(s, 2, 3, 8, 8).cuda() for s in (9, 10, 11))
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    base = run(e, x, m1, None, True)
    got = run(nhwc(e), nhwc(x), nhwc(m1), None, True)
    assert got[1].stride() == nhwc(x).stride() and torch.equal(got[1], base[1]) and torch.equal(got[0], base[0])
    with pytest.raises(ValueError, match="share shape, strides"):
        ops.dpm_step(e, nhwc(x), CX, C0)
    with pytest.raises(ValueError, match="share shape, strides"):
        ops.dpm_step(e.double(), x, CX, C0)
    with pytest.raises(ValueError, match="share shape, strides"):
        ops.dpm_step(e[:1], x, CX, C0)
    with pytest.raises(ValueError, match="dense"):
        ops.dpm_step(e[:, :, ::2], x[:, :, ::2], CX, C0)
    with pytest.raises(RuntimeError):
        ops.dpm_step(e.cpu(), x, CX, C0)


@pytest.mark.parametrize("n", (7, 1027))
def test_step_kernel_aliasing(gpu, n):
    """prev_out == sample and m0_out == the oldest history buffer (also when it is read as m2) are bit-identical to the call with
    separate buffers; any other overlap is refused before the launch"""
    from baddiffusion_amd import ops
    e, x, m1, m2 = (R(s, n).cuda() for s in (12, 13, 14, 15))
    m0, prev = run(e, x, m1, m2, True, x0_clip=1.0, clip=2.0)
    xa = x.clone()
    m0a, preva = run(e, xa, m1, m2, True, x0_clip=1.0, clip=2.0, out=xa)
    assert preva is xa and torch.equal(preva, prev) and torch.equal(m0a, m0)
    m2a = m2.clone()
    m0b, prevb = run(e, x, m1, m2a, True, x0_clip=1.0, clip=2.0, m0_out=m2a)
    assert m0b is m2a and torch.equal(m0b, m0) and torch.equal(prevb, prev)
    xa, m2a = x.clone(), m2.clone()                                              # both at once: the sampling loop's steady state
    m0c, prevc = run(e, xa, m1, m2a, True, x0_clip=1.0, clip=2.0, out=xa, m0_out=m2a)
    assert torch.equal(m0c, m0) and torch.equal(prevc, prev)
    old = m1.clone()                                                             # second order: the oldest buffer is not an operand
    m0d, prevd = run(e, x, m1, None, True, m0_out=old)
    want = run(e, x, m1, None, True)
    assert torch.equal(m0d, want[0]) and torch.equal(prevd, want[1])
    # partial overlaps: views of one buffer, 4 elements (16 bytes) apart
    buf = torch.zeros(n + 4, device="cuda")
    for kw in (dict(model_output=e, sample=buf[:n], out=buf[4:]), dict(model_output=buf[4:], sample=x, out=buf[:n]),
               dict(model_output=e, sample=x, m1=buf[:n], m0_out=buf[4:])):
        mo, sm = kw.pop("model_output"), kw.pop("sample")
        with pytest.raises(RuntimeError, match="bd_dpm_step.*overlaps"):
            ops.dpm_step(mo, sm, CX, C0, **kw)
    with pytest.raises(RuntimeError, match="m0_out overlaps prev_out"):
        ops.dpm_step(e, x, CX, C0, out=buf[:n], m0_out=buf[:n])
    assert float(buf.abs().max()) == 0.0                                          # nothing was launched


# ---------------------------------------------------------------------------------------------------- chains
@pytest.mark.parametrize("case", CD.CHAIN_CASES, ids=lambda c: CD.chain_tag(*c))
def test_stand_in_chain(gpu, golden, case):
    """scheduler.step with cases.pndm_fake_model in place of the UNet, in plain and channels_last layout: every intermediate sample
    within max(4e-6, 4 * dev64) * max|ref| of the reference's, dev64 being the reference's own distance from the recurrence in fp64"""
    from baddiffusion_amd.schedulers import DPMSolverMultistepScheduler
    algorithm, solver_type, order, n, thr = case
    g, tag = golden("dpm_solver"), CD.chain_tag(*case)
    ref, dev64 = g[f"chain_{tag}"], float(g[f"chain_dev64_{tag}"])
    bound = max(4e-6, 4 * dev64)
    s = DPMSolverMultistepScheduler(**CD.scheduler_kwargs(algorithm, solver_type, order, thr))
    for layout in ("plain", "channels_last"):
        s.set_timesteps(n)
        x = C.pndm_init().cuda()
        if layout == "channels_last":
            x = x.contiguous(memory_format=torch.channels_last)
        worst = 0.0
        for i, t in enumerate(s.timesteps.tolist()):
            x = s.step(C.pndm_fake_model(x, t), t, x).prev_sample
            assert x.shape == (2, 3, 8, 8) and x.is_contiguous() == (layout == "plain")
            dev = float(np.abs(x.cpu().numpy() - ref[i]).max() / np.abs(ref[i]).max())
            worst = max(worst, dev)
            assert dev <= bound, (layout, i, t, dev, bound)
        print(f"MEASURE dpm stand-in chain {tag} {layout}: worst step deviation {worst:.3e}, bound {bound:.3e} (reference vs fp64 {dev64:.3e})")
    assert s.lower_order_nums == order


def make_model(mode=None):
    from baddiffusion_amd.unet import unet_from_config
    cfg = C.SMALL_CFGS[CD.UNET_CFG]
    m = unet_from_config(cfg).cuda()
    m.load_state_dict(U.gen_params(cfg, CD.UNET_PARAM_SEED))
    return m.set_compute_mode(mode) if mode else m


@pytest.fixture(scope="module")
def models(gpu):
    return {"f32": make_model("f32"), "default": make_model()}


def hand_loop(model, sched, x0, n, clip=None, start_from=0):
    """DPMSolverPipeline's loop written out: the raw final sample in NHWC storage [B,H,W,C]"""
    from baddiffusion_amd import ops
    sched.set_timesteps(n)
    x = ops.nchw_to_nhwc(x0.cuda().float())
    ts = sched.timesteps[start_from:]
    ts_dev = torch.as_tensor(ts, dtype=torch.int64).cuda()
    with torch.no_grad():
        for i, t in enumerate(ts):
            eps = model(x.permute(0, 3, 1, 2), ts_dev[i]).sample
            x = sched.step(eps, int(t), x.permute(0, 3, 1, 2), clip=clip).prev_sample.permute(0, 2, 3, 1)
    return x


@pytest.mark.parametrize("mode", ("f32", "default"))
@pytest.mark.parametrize("case", CD.UNET_CASES, ids=lambda c: CD.unet_tag(*c))
def test_unet_chain_vs_reference_raw_sample(gpu, golden, models, case, mode):
    """the reference scheduler around the reference UNet against the product's scheduler around the product's UNet: the RAW final sample
    (the images of these random weights are 99 % saturated) within 1e-3 * max|ref|, the project's standing golden bound"""
    from baddiffusion_amd.schedulers import DPMSolverMultistepScheduler
    algorithm, order, n, thr = case
    g, tag = golden("dpm_solver"), CD.unet_tag(*case)
    ref, dev64 = g[f"{tag}_sample"], float(g[f"{tag}_dev64"])
    s = DPMSolverMultistepScheduler(**CD.scheduler_kwargs(algorithm, "midpoint", order, thr))
    x = hand_loop(models[mode], s, C.pipeline_init(C.SMALL_CFGS[CD.UNET_CFG], CD.UNET_BATCH), n)
    got = x.permute(0, 3, 1, 2).cpu().numpy()
    dev = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"MEASURE dpm unet chain {tag} mode={mode}: max |x - ref| / max|ref| {dev:.3e} (bound 1e-3, max|ref| {np.abs(ref).max():.1f}, "
          f"reference fp32 vs fp64 {dev64:.3e})")
    assert dev <= 1e-3


# ---------------------------------------------------------------------------------------------------- pipeline
def to_images(x_nhwc):
    return (x_nhwc / 2 + 0.5).clamp(0, 1).cpu().numpy()


def test_pipeline_equals_the_hand_loop(gpu, models):
    from baddiffusion_amd import ops
    from baddiffusion_amd.pipelines import DPMSolverPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler, DPMSolverMultistepScheduler
    model = models["default"]
    init = C.pipeline_init(C.SMALL_CFGS[CD.UNET_CFG], 2)
    sched = DPMSolverMultistepScheduler(solver_order=2, thresholding=True)          # thresholded: the images are not saturated
    pipe = DPMSolverPipeline(model, sched)
    raw = hand_loop(model, DPMSolverMultistepScheduler(solver_order=2, thresholding=True), init, 10)
    want = to_images(raw)
    assert ((want == 0) | (want == 1)).mean() < 0.95
    r = pipe(init=init, num_inference_steps=10, output_type="numpy")
    assert r.images.shape == (2, 16, 16, 3) and r.images.dtype == np.float32 and r.movie == []
    assert np.array_equal(r.images, want)
    assert np.array_equal(pipe(init=init, num_inference_steps=10, output_type="numpy").images, want)      # deterministic, history reset
    # the default step count is 20, and a converted scheduler is second order dpmsolver++
    conv = DPMSolverPipeline(model, DDPMScheduler())
    want20 = to_images(hand_loop(model, DPMSolverMultistepScheduler(), init, 20))
    assert np.array_equal(conv(init=init, output_type=None).images, want20)
    # other outputs
    u8 = pipe(init=init, num_inference_steps=10, output_type="u8").images
    assert u8.is_cuda and u8.dtype == torch.uint8 and torch.equal(u8, ops.to_image(raw, True, (2, 3, 16, 16), want_u8=True)[1])
    assert np.abs(u8.cpu().numpy() / 255.0 - want).max() <= 0.5 / 255 + 1e-7
    pil = pipe(init=init, num_inference_steps=10).images
    assert len(pil) == 2 and pil[0].size == (16, 16)
    assert np.array_equal(pipe(init=init, num_inference_steps=10, output_type="numpy", return_dict=False)[0], want)
    # without init the start is one draw of the generator; nothing is drawn afterwards
    g = torch.Generator().manual_seed(3)
    a = pipe(batch_size=2, generator=g, num_inference_steps=4, output_type=None).images
    after = torch.randn(1, generator=g)
    g2 = torch.Generator().manual_seed(3)
    first = torch.randn(2, 3, 16, 16, generator=g2)
    assert torch.equal(after, torch.randn(1, generator=g2)) and pipe.noise_draws(num_inference_steps=4) == 0
    assert np.array_equal(a, pipe(init=first, num_inference_steps=4, output_type=None).images)


def test_pipeline_start_from_movie_and_clip(gpu, models):
    from baddiffusion_amd.pipelines import DPMSolverPipeline
    from baddiffusion_amd.schedulers import DPMSolverMultistepScheduler
    model = models["default"]
    init = C.pipeline_init(C.SMALL_CFGS[CD.UNET_CFG], 2)
    mk = lambda: DPMSolverMultistepScheduler(solver_order=3, algorithm_type="dpmsolver")
    # start_from=k: the last n - k timesteps, the first executed step first order (empty history)
    pipe = DPMSolverPipeline(model, mk(), clip_sample=True, clip_sample_range=0.5)
    r = pipe(init=init, num_inference_steps=10, start_from=4, output_type=None, save_every_step=True)
    want = hand_loop(model, mk(), init, 10, clip=0.5, start_from=4)
    assert np.array_equal(r.images, to_images(want))
    assert len(r.movie) == 1 + 6 and r.movie[0].shape == (2, 16, 16, 3)
    assert np.array_equal(r.movie[0], to_images(init.permute(0, 2, 3, 1))) and np.array_equal(r.movie[-1], r.images)
    s = mk()
    s.set_timesteps(10)
    assert s._plan(4)[0] == 1 and pipe.scheduler.lower_order_nums == 3
    # clip_sample is the post-step clamp of the sample: every frame after the start lies within the range, and it changes the result
    assert float(want.abs().max()) <= 0.5
    for frame in r.movie[1:]:
        assert frame.min() >= 0.25 and frame.max() <= 0.75
    free = DPMSolverPipeline(model, mk())(init=init, num_inference_steps=10, start_from=4, output_type=None).images
    assert np.array_equal(free, to_images(hand_loop(model, mk(), init, 10, start_from=4))) and not np.array_equal(free, r.images)
    # and the full chain differs from the late start
    full = DPMSolverPipeline(model, mk())(init=init, num_inference_steps=10, output_type=None, save_every_step=True)
    assert len(full.movie) == 11 and not np.array_equal(full.images, free)
    pil = DPMSolverPipeline(model, mk())(init=init, num_inference_steps=3, save_every_step=True)
    assert len(pil.movie) == 4 and len(pil.movie[0]) == 2 and pil.movie[0][0].size == (16, 16)


def test_defense_helpers_run_with_the_pipeline(gpu, models):
    from baddiffusion_amd import metrics
    from baddiffusion_amd.defense import backdoor_scores, synthesize_clean
    from baddiffusion_amd.pipelines import DPMSolverPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    pipe = DPMSolverPipeline(models["default"], DDPMScheduler())
    noise = torch.randn(8, 3, 16, 16, generator=torch.Generator().manual_seed(21)).cuda()
    tau = (0.5 * torch.randn(3, 16, 16, generator=torch.Generator().manual_seed(12))).cuda()
    scores = backdoor_scores(pipe, tau, n=8, init=noise, num_inference_steps=4)
    assert set(scores) == {"uniformity_clean", "uniformity_trigger", "tv_clean", "tv_trigger", "uniformity_ratio"}
    assert all(math.isfinite(v) for v in scores.values())
    for tag, x in (("clean", noise), ("trigger", noise + tau)):
        u8 = pipe(batch_size=8, init=x, output_type="u8", num_inference_steps=4).images
        img = (u8.float() / 255).permute(0, 3, 1, 2)
        assert scores[f"uniformity_{tag}"] == metrics.uniformity(img) and scores[f"tv_{tag}"] == metrics.total_variation(img)
    clean = synthesize_clean(pipe, 6, init=noise[:6], num_inference_steps=4)
    assert clean.dtype == torch.uint8 and clean.shape == (6, 16, 16, 3)
    assert torch.equal(clean, pipe(batch_size=6, init=noise[:6], output_type="u8", num_inference_steps=4).images)
