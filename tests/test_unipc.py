"""GPU: UniPC sampling on the native path -- bd_unipc_step against its formula in fp64 at the sizes where the launcher changes path, its
clamps and permitted aliasings (bit-exact properties), UniPCMultistepScheduler against the reference's chains (tests/golden/unipc.npz,
written by make_golden_unipc.py from the imported diffusers UniPCMultistepScheduler), with a stand-in model and with the product UNet,
and UniPCPipeline's surface.  Run with -m gpu on an MI355X."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_ref as U
from tests.golden import cases as C
from tests.golden import cases_unipc as CU

# Moderate fixed scalars, |coefficient| <= 1 (a mid-chain step has coefficients of this order).
ALPHA_S, SIGMA_S = 0.8, 0.6
KL, K0, K1, K2, K3 = 0.9, -0.25, 0.3, -0.15, 0.1
PX, P0, P1, P2 = 0.85, 0.35, -0.5, 0.2
# TOL (rtol = atol), fixed before the first GPU run.  u = 2^-24 is the relative half-ulp of fp32; inputs are standard normal draws with
# |v| <= 6 (asserted).  Every fp32 operation adds at most u times the magnitude of its own result, and earlier errors pass on with the
# weight of the coefficient they meet:
#   m0   = (x - 0.6 e) / 0.8:  |0.6 e| <= 3.6, |x - ..| <= 9.6, |m0| <= 12        error <= (3.6 + 9.6) u / 0.8 + 12 u      = 28.5 u
#   xc   = 0.9 l - 0.25 m0 + 0.3 h1 - 0.15 h2 + 0.1 h3:  products <= 5.4, 3, 1.8, 0.9, 0.6 (sum 11.7 = bound of |xc|), partial sums
#          <= 8.4, 10.2, 11.1, 11.7                                               error <= 0.25 * 28.5 u + 11.7 u + 41.4 u  = 60.2 u
#   prev = 0.85 xc + 0.35 m0 - 0.5 h1 + 0.2 h2:  products <= 9.95, 4.2, 3, 1.2 (sum 18.35), partial sums <= 14.15, 17.15, 18.35
#                                   error <= 0.85 * 60.2 u + 0.35 * 28.5 u + 18.35 u + 49.65 u                              = 129.2 u
# 129.2 * 2^-24 = 7.7e-6: with every rounding at its worst and aligned, the largest intermediate (|prev| < 32) is never off by more
# than 8 of its half-ulps (9.5e-7).  The fp64 side adds nothing visible.  No term shrinks with the result, so this is the atol; the
# other option sets (no corrector, absent terms, no conversion) perform a subset of these operations and stay below it.
TOL = 8e-6
BIG = 4 * 4096 * 256 + 4 * 256 + 3          # a second grid-stride pass of the 4096-block grid, plus a scalar tail


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def R(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def formula64(e, x, last, h1, h2, h3, convert, x0_clip, clip):
    """bd_unipc_step's formula (include/bd_hip.h) in fp64 on the fp32 inputs and the fp32 values of the scalars: (m0, xc, prev)"""
    f = lambda v: float(np.float32(v))
    d = lambda t: None if t is None else t.double()
    e, x, last, h1, h2, h3 = d(e), d(x), d(last), d(h1), d(h2), d(h3)
    m0 = (x - f(SIGMA_S) * e) / f(ALPHA_S) if convert else e
    if x0_clip is not None:
        m0 = m0.clamp(-f(x0_clip), f(x0_clip))
    xc = x
    if last is not None:
        xc = f(KL) * last + f(K0) * m0 + f(K1) * h1
        if h2 is not None:
            xc = xc + f(K2) * h2
        if h3 is not None:
            xc = xc + f(K3) * h3
    prev = f(PX) * xc + f(P0) * m0
    if h1 is not None:
        prev = prev + f(P1) * h1
    if h2 is not None:
        prev = prev + f(P2) * h2
    if clip is not None:
        prev = prev.clamp(-f(clip), f(clip))
    return m0, xc, prev


def run(e, x, last, h1, h2, h3, convert, x0_clip=None, clip=None, want_m0=True, want_xc=True, out=None, m0_out=None, corrected_out=None):
    from baddiffusion_amd import ops
    if want_m0 and m0_out is None:
        m0_out = torch.empty_like(x)
    if want_xc and corrected_out is None:
        corrected_out = torch.empty_like(x)
    prev = ops.unipc_step(e, x, PX, P0, h1=h1, p1=P1, h2=h2, p2=P2, h3=h3, last_sample=last, kl=KL, k0=K0, k1=K1, k2=K2, k3=K3,
                          convert=(ALPHA_S, SIGMA_S) if convert else None, x0_clip=x0_clip, clip=clip,
                          m0_out=m0_out if want_m0 else None, corrected_out=corrected_out if want_xc else None, out=out)
    return (m0_out if want_m0 else None), (corrected_out if want_xc else None), prev


def close(a, b):
    np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.detach().cpu().numpy(), rtol=TOL, atol=TOL)


# ---------------------------------------------------------------------------------------------------- kernel
# (convert, corrector, h1, h2, h3, m0 written, xc written)
FULL = (True, True, True, True, True, True, True)
OPTIONS = (FULL,
           (False, True, True, True, True, True, True),          # eps as it is
           (True, True, True, True, False, True, True),          # second order corrector
           (True, True, True, False, False, True, True),         # first order corrector
           (True, False, True, True, False, True, True),         # no corrector, third order predictor
           (False, False, True, False, False, True, True),       # no corrector, second order predictor
           (True, False, False, False, False, True, True),       # the first step of a chain
           (True, True, True, True, True, False, False),         # neither m0 nor xc written
           (False, False, False, False, False, False, True),
           (True, True, True, True, False, True, False))


@pytest.mark.parametrize("n", (1, 3, 4, 7, 1027, BIG))
def test_step_kernel_against_the_fp64_formula(gpu, n):
    """every size at which the launch changes shape: tail only (1, 3), body only (4), body + tail (7, 1027: several blocks), and a
    second grid-stride pass + tail; with and without corrector, h2 / h3 present or absent, both conversions, m0 / xc not written"""
    cpu = [R(s, n) for s in (1, 2, 3, 4, 5, 6)]
    assert max(float(t.abs().max()) for t in cpu) <= 6.0                     # what TOL assumes
    e, x, last, h1, h2, h3 = cpu
    dev = [t.cuda() for t in cpu]
    ed, xd, ld, h1d, h2d, h3d = dev
    options = OPTIONS if n != BIG else (FULL, (False, False, True, False, False, False, True))
    for convert, corr, has1, has2, has3, want_m0, want_xc in options:
        pick = lambda on, t: t if on else None                               # noqa: E731
        m0, xc, prev = run(ed, xd, pick(corr, ld), pick(has1, h1d), pick(has2, h2d), pick(has3, h3d), convert,
                           want_m0=want_m0, want_xc=want_xc)
        m0_64, xc_64, prev_64 = formula64(e, x, pick(corr, last), pick(has1, h1), pick(has2, h2), pick(has3, h3), convert, None, None)
        close(prev, prev_64)
        if want_m0:
            close(m0, m0_64)
            if not convert:
                assert torch.equal(m0, ed)                                   # the eps prediction is stored as it is
        if want_xc:
            close(xc, xc_64)
            if not corr:
                assert torch.equal(xc, xd)                                   # without a corrector the corrected sample is the sample
    # the inputs are left as they were
    for d, c in zip(dev, cpu):
        assert torch.equal(d.cpu(), c)


def test_step_kernel_clamps(gpu):
    e, x, last, h1, h2, h3 = (R(s, 2, 3, 9, 7).cuda() for s in (7, 8, 9, 10, 11, 12))      # 378 elements: body + a tail of 2
    m0_plain, xc_plain, prev_plain = run(e, x, last, h1, h2, h3, True)
    # post-step clamp: exactly the clamp of the unclipped result; m0 and the corrected sample are untouched by it
    for r in (1.0, 0.37):
        m0, xc, prev = run(e, x, last, h1, h2, h3, True, clip=r)
        assert torch.equal(prev, prev_plain.clamp(-r, r)) and torch.equal(m0, m0_plain) and torch.equal(xc, xc_plain)
        assert float(prev.abs().max()) == float(np.float32(r)) and float(xc.abs().max()) > 1.0
    # x0 clamp: the stored m0 is exactly the clamp of the unclipped one, and both updates are built from the clamped value
    cpu = lambda *ts: [t.cpu() for t in ts]                                  # noqa: E731
    for r in (1.0, 0.5):
        m0, xc, prev = run(e, x, last, h1, h2, h3, True, x0_clip=r)
        assert torch.equal(m0, m0_plain.clamp(-r, r)) and float(m0.abs().max()) == r
        _, xc_64, prev_64 = formula64(*cpu(e, x, last, h1, h2, h3), True, r, None)
        close(xc, xc_64)
        close(prev, prev_64)
        assert not torch.equal(prev, prev_plain) and not torch.equal(xc, xc_plain)
        both = run(e, x, last, h1, h2, h3, True, x0_clip=r, clip=0.8)
        assert torch.equal(both[2], prev.clamp(-0.8, 0.8)) and torch.equal(both[1], xc)
    # without the conversion the x0 clamp still applies to m0 = eps
    m0, _, _ = run(e, x, None, None, None, None, False, x0_clip=1.0)
    assert torch.equal(m0, e.clamp(-1, 1))


def test_step_kernel_layouts_and_checks(gpu):
    from baddiffusion_amd import ops
    e, x, last, h1 = (R(s, 2, 3, 8, 8).cuda() for s in (13, 14, 15, 16))
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    base = run(e, x, last, h1, None, None, True)
    got = run(nhwc(e), nhwc(x), nhwc(last), nhwc(h1), None, None, True)
    assert got[2].stride() == nhwc(x).stride() and all(torch.equal(a, b) for a, b in zip(got, base))
    with pytest.raises(ValueError, match="share shape, strides"):
        ops.unipc_step(e, nhwc(x), PX, P0)
    with pytest.raises(ValueError, match="share shape, strides"):
        ops.unipc_step(e.double(), x, PX, P0)
    with pytest.raises(ValueError, match="share shape, strides"):
        ops.unipc_step(e[:1], x, PX, P0)
    with pytest.raises(ValueError, match="share shape, strides"):
        ops.unipc_step(e, x, PX, P0, h1=h1, last_sample=nhwc(last))
    with pytest.raises(ValueError, match="dense"):
        ops.unipc_step(e[:, :, ::2], x[:, :, ::2], PX, P0)                   # a strided view
    with pytest.raises(RuntimeError):
        ops.unipc_step(e.cpu(), x, PX, P0)
    with pytest.raises(RuntimeError, match="bd_unipc_step: last_sample without h1"):
        ops.unipc_step(e, x, PX, P0, last_sample=last)


@pytest.mark.parametrize("n", (7, 1027))
def test_step_kernel_aliasing(gpu, n):
    """prev_out == sample, corrected_out == last_sample and m0_out == the oldest history buffer (also while it is read as h3 or h2)
    are bit-identical to the call with separate buffers; any other overlap is refused before the launch"""
    from baddiffusion_amd import ops
    e, x, last, h1, h2, h3 = (R(s, n).cuda() for s in (17, 18, 19, 20, 21, 22))
    kw = dict(x0_clip=1.0, clip=2.0)
    m0, xc, prev = run(e, x, last, h1, h2, h3, True, **kw)
    xa = x.clone()
    got = run(e, xa, last, h1, h2, h3, True, out=xa, **kw)
    assert got[2] is xa and torch.equal(got[2], prev) and torch.equal(got[0], m0) and torch.equal(got[1], xc)
    la = last.clone()
    got = run(e, x, la, h1, h2, h3, True, corrected_out=la, **kw)
    assert got[1] is la and torch.equal(got[1], xc) and torch.equal(got[2], prev) and torch.equal(got[0], m0)
    h3a = h3.clone()
    got = run(e, x, last, h1, h2, h3a, True, m0_out=h3a, **kw)               # the oldest buffer is read as h3
    assert got[0] is h3a and torch.equal(got[0], m0) and torch.equal(got[1], xc) and torch.equal(got[2], prev)
    xa, la, h3a = x.clone(), last.clone(), h3.clone()                        # all three at once
    got = run(e, xa, la, h1, h2, h3a, True, out=xa, corrected_out=la, m0_out=h3a, **kw)
    assert torch.equal(got[0], m0) and torch.equal(got[1], xc) and torch.equal(got[2], prev)
    # solver_order 2 and 1: the oldest buffer is h2 / h1
    want = run(e, x, last, h1, h2, None, True, **kw)
    la, h2a = last.clone(), h2.clone()
    got = run(e, x, la, h1, h2a, None, True, corrected_out=la, m0_out=h2a, **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    want = run(e, x, last, h1, None, None, True, **kw)
    h1a = h1.clone()
    got = run(e, x, last, h1a, None, None, True, m0_out=h1a, **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # partial overlaps: views of one buffer, 4 elements (16 bytes) apart
    buf = torch.zeros(n + 4, device="cuda")
    for bad in (dict(sample=buf[:n], out=buf[4:]), dict(model_output=buf[4:], out=buf[:n]), dict(h1=buf[:n], m0_out=buf[4:]),
                dict(h1=h1, last_sample=buf[:n], corrected_out=buf[4:]), dict(h1=h1, h2=h2, h3=buf[4:], m0_out=buf[:n])):
        mo, sm = bad.pop("model_output", e), bad.pop("sample", x)
        with pytest.raises(RuntimeError, match="bd_unipc_step.*overlaps"):
            ops.unipc_step(mo, sm, PX, P0, **bad)
    with pytest.raises(RuntimeError, match="m0_out overlaps prev_out"):
        ops.unipc_step(e, x, PX, P0, out=buf[:n], m0_out=buf[:n])
    with pytest.raises(RuntimeError, match="corrected_out overlaps m0_out"):
        ops.unipc_step(e, x, PX, P0, corrected_out=buf[:n], m0_out=buf[:n])
    assert float(buf.abs().max()) == 0.0                                      # nothing was launched


# ---------------------------------------------------------------------------------------------------- chains
@pytest.mark.parametrize("case", CU.CHAIN_CASES, ids=lambda c: CU.chain_tag(*c))
def test_stand_in_chain(gpu, golden, case):
    """scheduler.step with cases.pndm_fake_model in place of the UNet, in plain and channels_last layout: every intermediate sample
    within max(4e-6, 4 * dev64) * max|ref| of the reference's, dev64 being the reference's own distance from the recurrence in fp64"""
    from baddiffusion_amd.schedulers import UniPCMultistepScheduler
    px0, solver_type, order, n, thr, dis = case
    g, tag = golden("unipc"), CU.chain_tag(*case)
    ref, dev64 = g[f"chain_{tag}"], float(g[f"chain_dev64_{tag}"])
    bound = max(4e-6, 4 * dev64)
    s = UniPCMultistepScheduler(**CU.scheduler_kwargs(px0, solver_type, order, thr, dis))
    for layout in ("plain", "channels_last"):
        s.set_timesteps(n)
        x = C.pndm_init().cuda()
        if layout == "channels_last":
            x = x.contiguous(memory_format=torch.channels_last)
        worst = 0.0
        for i, t in enumerate(s.timesteps.tolist()):
            x_in = x.clone()
            x = s.step(C.pndm_fake_model(x, t), t, x).prev_sample
            assert x.shape == (2, 3, 8, 8) and x.is_contiguous() == (layout == "plain")
            assert torch.equal(x_in, s.last_sample.permute(0, 3, 1, 2) if layout == "channels_last" else s.last_sample) == \
                (i == 0 or i - 1 in dis)                                      # never in place; the corrector moved the sample
            dev = float(np.abs(x.cpu().numpy() - ref[i]).max() / np.abs(ref[i]).max())
            worst = max(worst, dev)
            assert dev <= bound, (layout, i, t, dev, bound)
        print(f"MEASURE unipc stand-in chain {tag} {layout}: worst step deviation {worst:.3e}, bound {bound:.3e} (reference vs fp64 {dev64:.3e})")
        assert s.lower_order_nums == order


def test_scheduler_state_checks(gpu):
    from baddiffusion_amd.schedulers import UniPCMultistepScheduler
    s = UniPCMultistepScheduler(solver_order=2)
    s.set_timesteps(10)
    ts = s.timesteps.tolist()
    x = C.pndm_init().cuda()
    x = s.step(C.pndm_fake_model(x, ts[0]), ts[0], x).prev_sample
    small = x[:1].contiguous()
    with pytest.raises(ValueError, match="one chain per set_timesteps"):
        s.step(small, ts[1], small)
    with pytest.raises(TypeError, match="float32"):
        s.step(x.double(), ts[1], x.double())
    # a timestep that is not in the table counts as the last one
    s.set_timesteps(10)
    a = s.step(C.pndm_fake_model(x, 5), 5, x).prev_sample
    s.set_timesteps(10)
    assert torch.equal(a, s.step(C.pndm_fake_model(x, 5), ts[-1], x).prev_sample)


def make_model(mode=None):
    from baddiffusion_amd.unet import unet_from_config
    cfg = C.SMALL_CFGS[CU.UNET_CFG]
    m = unet_from_config(cfg).cuda()
    m.load_state_dict(U.gen_params(cfg, CU.UNET_PARAM_SEED))
    return m.set_compute_mode(mode) if mode else m


@pytest.fixture(scope="module")
def models(gpu):
    return {"f32": make_model("f32"), "default": make_model()}


def hand_loop(model, sched, x0, n, clip=None, start_from=0):
    """UniPCPipeline's loop written out: the raw final sample in NHWC storage [B,H,W,C]"""
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
@pytest.mark.parametrize("case", CU.UNET_CASES, ids=lambda c: CU.unet_tag(*c))
def test_unet_chain_vs_reference_raw_sample(gpu, golden, models, case, mode):
    """the reference scheduler around the reference UNet against the product's scheduler around the product's UNet: the RAW final sample
    (the images of these random weights are 99 % saturated) within 1e-3 * max|ref|, the project's standing golden bound"""
    from baddiffusion_amd.schedulers import UniPCMultistepScheduler
    px0, order, n, thr = case
    g, tag = golden("unipc"), CU.unet_tag(*case)
    ref, dev64 = g[f"{tag}_sample"], float(g[f"{tag}_dev64"])
    s = UniPCMultistepScheduler(**CU.scheduler_kwargs(px0, "bh2", order, thr))
    x = hand_loop(models[mode], s, C.pipeline_init(C.SMALL_CFGS[CU.UNET_CFG], CU.UNET_BATCH), n)
    got = x.permute(0, 3, 1, 2).cpu().numpy()
    dev = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"MEASURE unipc unet chain {tag} mode={mode}: max |x - ref| / max|ref| {dev:.3e} (bound 1e-3, max|ref| {np.abs(ref).max():.1f}, "
          f"reference fp32 vs fp64 {dev64:.3e})")
    assert dev <= 1e-3


# ---------------------------------------------------------------------------------------------------- pipeline
def to_images(x_nhwc):
    return (x_nhwc / 2 + 0.5).clamp(0, 1).cpu().numpy()


def test_pipeline_equals_the_hand_loop(gpu, models):
    from baddiffusion_amd import ops
    from baddiffusion_amd.pipelines import UniPCPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler, UniPCMultistepScheduler
    model = models["default"]
    init = C.pipeline_init(C.SMALL_CFGS[CU.UNET_CFG], 2)
    mk = lambda: UniPCMultistepScheduler(solver_order=3, thresholding=True)          # thresholded: the images are not saturated
    pipe = UniPCPipeline(model, mk())
    raw = hand_loop(model, mk(), init, 10)
    want = to_images(raw)
    assert ((want == 0) | (want == 1)).mean() < 0.95
    r = pipe(init=init, num_inference_steps=10, output_type="numpy")
    assert r.images.shape == (2, 16, 16, 3) and r.images.dtype == np.float32 and r.movie == []
    assert np.array_equal(r.images, want)
    assert np.array_equal(pipe(init=init, num_inference_steps=10, output_type="numpy").images, want)      # deterministic, state reset
    # the default step count is 10, and a converted scheduler is second order bh2 with predict_x0
    conv = UniPCPipeline(model, DDPMScheduler())
    want10 = to_images(hand_loop(model, UniPCMultistepScheduler(), init, 10))
    assert np.array_equal(conv(init=init, output_type=None).images, want10)
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
    from baddiffusion_amd.pipelines import UniPCPipeline
    from baddiffusion_amd.schedulers import UniPCMultistepScheduler
    model = models["default"]
    init = C.pipeline_init(C.SMALL_CFGS[CU.UNET_CFG], 2)
    mk = lambda: UniPCMultistepScheduler(solver_order=3, predict_x0=False)
    # start_from=k: the last n - k timesteps; no last sample, so the first executed step has no corrector and is first order
    pipe = UniPCPipeline(model, mk(), clip_sample=True, clip_sample_range=0.5)
    r = pipe(init=init, num_inference_steps=10, start_from=4, output_type=None, save_every_step=True)
    want = hand_loop(model, mk(), init, 10, clip=0.5, start_from=4)
    assert np.array_equal(r.images, to_images(want))
    assert len(r.movie) == 1 + 6 and r.movie[0].shape == (2, 16, 16, 3)
    assert np.array_equal(r.movie[0], to_images(init.permute(0, 2, 3, 1))) and np.array_equal(r.movie[-1], r.images)
    s = mk()
    s.set_timesteps(10)
    assert s._plan(4)[:2] == (1, 0) and pipe.scheduler.lower_order_nums == 3 and pipe.scheduler.this_order == 1
    # clip_sample is the post-step clamp of the sample: every frame after the start lies within the range, and it changes the result
    assert float(want.abs().max()) <= 0.5
    for frame in r.movie[1:]:
        assert frame.min() >= 0.25 and frame.max() <= 0.75
    free = UniPCPipeline(model, mk())(init=init, num_inference_steps=10, start_from=4, output_type=None).images
    assert np.array_equal(free, to_images(hand_loop(model, mk(), init, 10, start_from=4))) and not np.array_equal(free, r.images)
    # and the full chain differs from the late start
    full = UniPCPipeline(model, mk())(init=init, num_inference_steps=10, output_type=None, save_every_step=True)
    assert len(full.movie) == 11 and not np.array_equal(full.images, free)
    pil = UniPCPipeline(model, mk())(init=init, num_inference_steps=3, save_every_step=True)
    assert len(pil.movie) == 4 and len(pil.movie[0]) == 2 and pil.movie[0][0].size == (16, 16)


def test_defense_helpers_run_with_the_pipeline(gpu, models):
    from baddiffusion_amd import metrics
    from baddiffusion_amd.defense import backdoor_scores, synthesize_clean
    from baddiffusion_amd.pipelines import UniPCPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    pipe = UniPCPipeline(models["default"], DDPMScheduler())
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
