"""GPU: Euler, Euler-ancestral, KDPM2 and KDPM2-ancestral on the native path -- bd_sigma_noise_step held to equal bits against the torch
restatement of its order of operations (tests/golden/cases_kdiff.py), the four schedulers against the reference's chains
(tests/golden/kdiff.npz, written by make_golden_kdiff.py from the imported diffusers schedulers and UNet) with a stand-in model and
with the product UNet, and the surface of the four pipelines.  Run with -m gpu on an MI355X."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_ref as U
from tests.golden import cases as C
from tests.golden import cases_kdiff as CK
from tests.golden import cases_sigma as CS
from tests.test_kdiff_host import classes, plan, restated_step, sched

PAD = 8                                         # floats of NaN margin on either side of an output (32 bytes: the views stay 16-byte aligned)
BIG = 4096 * 256 * 4 + 5                        # one element more than a full pass of the 4096-block grid, plus a scalar tail


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def R(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def margined(n):
    """(buffer, view): n floats inside a NaN-filled buffer with PAD floats on either side"""
    buf = torch.full((n + 2 * PAD,), float("nan"), device="cuda")
    return buf, buf[PAD: PAD + n]


def margins_intact(buf, n):
    return bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + n:]).all())


def noise_gen():
    return torch.Generator().manual_seed(CK.NOISE_SEED)


# ---------------------------------------------------------------------------------------------------- bd_sigma_noise_step
MODES = ("plain", "churn", "up")
OUTPUTS = ((True, True), (False, False), (True, False), (False, True))       # x0_out, scaled_out


def schedule_points():
    """per mode the scalars (sigma_in, dt, in_div, churn, sigma_up) of a real schedule at 10 steps: the first step (sigma = 157.4), a
    middle one and the last (in_div = 1, and sigma_up = 0 for the ancestral noise)"""
    ea, eu = sched("euler_a", 10), sched("euler", 10)
    pts = {m: [] for m in MODES}
    for k in (0, 5, 9):
        a, c, p = ea._plan_scalars(k), eu._plan_scalars(k, s_churn=CK.S_CHURN, s_noise=1.003), eu._plan_scalars(k)
        pts["up"].append((a["sigma_in"], a["dt"], a["in_div"], None, a["sigma_up"]))
        pts["churn"].append((c["sigma_in"], c["dt"], c["in_div"], c["churn"], None))
        pts["plain"].append((p["sigma_in"], p["dt"], p["in_div"], None, None))
    assert abs(pts["up"][0][0] - 157.4) < 0.05 and pts["up"][2][2] == 1.0 and pts["up"][2][4] == 0.0 and pts["up"][1][4] > 0
    assert pts["churn"][1][3][0] == 1.003 and pts["churn"][1][3][1] > 0
    return pts


def run_case(n, e, x, z, b, pt, outs, use_base, clip):
    """one launch into NaN-margined outputs, compared bit for bit with the restatement"""
    from baddiffusion_amd import ops
    sigma_in, dt, in_div, churn, sigma_up = pt
    bufs = {k: margined(n) for k in ("x0_out", "scaled_out", "out")}
    kw = {k: (bufs[k][1] if on else None) for k, on in zip(("x0_out", "scaled_out"), outs)}
    ed, xd, zd, bd = e.cuda(), x.cuda(), z.cuda(), b.cuda()
    prev = ops.sigma_noise_step(ed, xd, zd, sigma_in, dt, in_div, base=bd if use_base else None, churn=churn, sigma_up=sigma_up, clip=clip,
                                out=bufs["out"][1], **kw)
    torch.cuda.synchronize()
    want = CK.sigma_noise_step_ref(e, x, z, sigma_in, dt, in_div, base=b if use_base else None, churn=churn, sigma_up=sigma_up, clip=clip)
    tag = (n, pt, outs, use_base, clip)
    assert prev is bufs["out"][1] and same_bits(prev, want[1]), tag
    for k, w, on in zip(("x0_out", "scaled_out"), (want[0], want[2]), outs):
        if on:
            assert same_bits(bufs[k][1], w), (k,) + tag
        else:
            assert bool(torch.isnan(bufs[k][0]).all()), (k,) + tag                  # an absent output is not written
        assert margins_intact(bufs[k][0], n), (k,) + tag
    assert margins_intact(bufs["out"][0], n), tag
    assert same_bits(ed, e) and same_bits(xd, x) and same_bits(zd, z) and same_bits(bd, b)      # the inputs are left as they were
    return want


@pytest.mark.parametrize("n", (1, 3, 4, 5, 1023, 4103))
def test_noise_step_equals_the_restatement(gpu, n):
    """tail only (1, 3), body only (4), body + tail (5, 1023, 4103: several blocks); {plain, churn, up} x which optional outputs are
    written x base or not x clip or not, at scalars of a real schedule"""
    pts = schedule_points()
    e, z, b = R(1, n), R(2, n), R(3, n)
    i = 0
    for mode in MODES:
        for outs in OUTPUTS:
            for use_base in (False, True):
                for clip in (None, 1.0):
                    pt = pts[mode][i % 3]
                    i += 1
                    x = R(6 + i, n) * float(np.float32((pt[0] ** 2 + 1) ** 0.5))      # a raw sample at this noise level
                    want = run_case(n, e, x, z, b * pt[0], pt, outs, use_base, clip)
                    if clip is not None:
                        assert float(want[2].abs().max()) <= 1.0
                        assert same_bits(want[1], want[2] * torch.tensor(float(np.float32(pt[2]))))
    # without a noise term the result is bd_sigma_step's first order one, and the noise buffer is not read
    from baddiffusion_amd import ops
    pt = pts["plain"][1]
    x = R(99, n) * pt[0]
    nan = torch.full((n,), float("nan"), device="cuda")
    got = ops.sigma_noise_step(e.cuda(), x.cuda(), nan, pt[0], pt[1], pt[2])
    assert same_bits(got, ops.sigma_step(e.cuda(), x.cuda(), pt[0], pt[1], pt[2]))


def test_noise_step_grid_stride_pass(gpu):
    """4096 * 256 * 4 + 5 elements: the grid-stride loop takes a second pass and the tail follows it; each variant once"""
    pts = schedule_points()
    n = BIG
    e, z, b = R(11, n), R(12, n), R(13, n)
    x = R(16, n) * 3.0
    for i, mode in enumerate(MODES):
        run_case(n, e, x, z, b, pts[mode][1], OUTPUTS[i % 2], bool(i % 2), 1.0 if i % 2 else None)


@pytest.mark.parametrize("n", (7, 1027))
def test_noise_step_aliasing_and_host_checks(gpu, n):
    """prev_out == sample gives the bits of the call with separate buffers; every other overlap and every host check is refused
    before anything is launched"""
    from baddiffusion_amd import _lib as L
    from baddiffusion_amd import ops
    sigma_in, dt, in_div, _, sigma_up = schedule_points()["up"][1]
    e, x, z, b = (R(s, n).cuda() for s in (31, 32, 33, 34))
    for kw in (dict(sigma_up=sigma_up), dict(churn=(1.0, 0.5)), dict(sigma_up=sigma_up, base=b, clip=2.0)):
        sc, sca = torch.empty_like(x), torch.empty_like(x)
        prev = ops.sigma_noise_step(e, x, z, sigma_in, dt, in_div, scaled_out=sc, **kw)
        xa = x.clone()
        preva = ops.sigma_noise_step(e, xa, z, sigma_in, dt, in_div, scaled_out=sca, out=xa, **kw)
        assert preva is xa and same_bits(preva, prev) and same_bits(sca, sc)
    # partial overlaps (views of one buffer, 4 elements = 16 bytes apart) and whole buffers used twice
    buf = torch.zeros(n + 4, device="cuda")
    lo, hi = buf[:n], buf[4:]
    k = dict(sigma_up=sigma_up)
    for mo, sm, nz, more in ((e, lo, z, dict(out=hi)), (hi, x, z, dict(out=lo)), (e, x, lo, dict(out=hi)), (e, x, z, dict(base=hi, scaled_out=lo)),
                             (e, x, z, dict(out=lo, scaled_out=hi)), (e, x, z, dict(out=lo, x0_out=lo)), (e, x, z, dict(x0_out=lo, scaled_out=hi))):
        with pytest.raises(RuntimeError, match="bd_sigma_noise_step.*overlaps"):
            ops.sigma_noise_step(mo, sm, nz, sigma_in, dt, in_div, **k, **more)
    keep = [t.clone() for t in (e, x, z, b)]
    for more in (dict(out=e), dict(out=z), dict(out=b, base=b), dict(x0_out=x), dict(scaled_out=x), dict(scaled_out=z)):
        with pytest.raises(RuntimeError, match="bd_sigma_noise_step: .* is the buffer of"):
            ops.sigma_noise_step(e, x, z, sigma_in, dt, in_div, **k, **more)
    for bad, pat in ((dict(sigma_in=0.0), "sigma_in=0 must be positive"), (dict(sigma_in=-1.0), "sigma_in=-1 must be positive"),
                     (dict(in_div=0.0), "in_div=0 must be positive"), (dict(sigma_up=-0.5), "sigma_up=-0.5 must not be negative"),
                     (dict(churn=(1.0, 0.5), sigma_up=0.3), "churn together with up"), (dict(churn=(1.0, 0.0)), "churn with churn_mul=0"),
                     (dict(churn=(1.0, -2.0)), "churn with churn_mul=-2")):
        args = dict(sigma_in=sigma_in, dt=dt, in_div=in_div, sigma_up=None, churn=None)
        args.update(bad)
        with pytest.raises(RuntimeError, match="bd_sigma_noise_step: .*" + pat):
            ops.sigma_noise_step(e, x, z, args["sigma_in"], args["dt"], args["in_div"], churn=args["churn"], sigma_up=args["sigma_up"],
                                 out=buf[:n])
    with pytest.raises(RuntimeError, match="bd_sigma_noise_step: null pointer"):
        ops.sigma_noise_step(e, x, None, sigma_in, dt, in_div, out=buf[:n])
    if n > 8:                                                                         # a misaligned view: one float in
        with pytest.raises(RuntimeError, match="bd_sigma_noise_step: noise is not 16-byte aligned"):
            ops.sigma_noise_step(e[1:].clone(), x[1:].clone(), z[1:], sigma_in, dt, in_div, **k)
    lib = L.load()
    last_error = lambda: lib.bd_last_error().decode()
    assert lib.bd_sigma_noise_step(None, L.stream()) != 0 and "bd_sigma_noise_step: null descriptor" in last_error()
    d = L.SigmaNoiseStepDesc(n=0, model_output=L.ptr(e), sample=L.ptr(x), noise=L.ptr(z), prev_out=L.ptr(buf[:n]), sigma_in=1.0, in_div=1.0)
    assert lib.bd_sigma_noise_step(d, L.stream()) != 0 and "n=0 must be positive" in last_error()
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0 and all(same_bits(a, b_) for a, b_ in zip((e, x, z, b), keep))      # nothing was launched


def test_noise_step_layouts(gpu):
    from baddiffusion_amd import ops
    sigma_in, dt, in_div, _, sigma_up = schedule_points()["up"][1]
    e, x, z, b = (R(s, 2, 3, 8, 8).cuda() for s in (41, 42, 43, 44))
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    want = ops.sigma_noise_step(e, x, z, sigma_in, dt, in_div, base=b, sigma_up=sigma_up)
    got = ops.sigma_noise_step(nhwc(e), nhwc(x), nhwc(z), sigma_in, dt, in_div, base=nhwc(b), sigma_up=sigma_up)
    assert got.stride() == nhwc(x).stride() and same_bits(got.contiguous(), want)
    for bad in (dict(e=nhwc(e)), dict(z=nhwc(z)), dict(b=nhwc(b)), dict(z=z.double())):
        a = dict(e=e, z=z, b=b)
        a.update(bad)
        with pytest.raises(ValueError, match="share shape, strides"):
            ops.sigma_noise_step(a["e"], x, a["z"], sigma_in, dt, in_div, base=a["b"], sigma_up=sigma_up)
    with pytest.raises(ValueError, match="share shape, strides"):
        ops.sigma_noise_step(e, x, z, sigma_in, dt, in_div, sigma_up=sigma_up, out=nhwc(x))
    with pytest.raises(ValueError, match="dense"):
        ops.sigma_noise_step(e[:, :, ::2], x[:, :, ::2], z[:, :, ::2], sigma_in, dt, in_div, sigma_up=sigma_up)
    with pytest.raises(RuntimeError):
        ops.sigma_noise_step(e, x, z.cpu(), sigma_in, dt, in_div, sigma_up=sigma_up)


# ---------------------------------------------------------------------------------------------------- chains
def step_kwargs(sampler, churn, gen):
    kw = {} if sampler == "kdpm2" else {"generator": gen}
    if sampler == "euler":
        kw["s_churn"] = churn
    return kw


@pytest.mark.parametrize("case", CK.CHAIN_CASES, ids=lambda c: CK.chain_tag(c[0], c[3]))
def test_stand_in_chain(gpu, golden, case):
    """scale_model_input + scheduler.step with cases.pndm_fake_model in place of the UNet and the fixture's noise stream (a CPU
    generator handed to `step`, which draws where the reference draws), in plain and channels_last layout: every intermediate sample
    within max(4e-6, 4 * dev64) * max|ref| of the reference's, dev64 being the reference's own distance from the recurrence in fp64;
    the step's scaled output is the next scale_model_input bit for bit; the generator ends where the reference's ended"""
    name, sampler, churn, n = case
    g, tag = golden("kdiff"), CK.chain_tag(name, n)
    ref, dev64 = g[f"chain_{tag}"], float(g[f"chain_dev64_{tag}"])
    bound = max(4e-6, 4 * dev64)
    s = sched(sampler)
    for layout in ("plain", "channels_last"):
        s.set_timesteps(n)
        gen = noise_gen()
        x = (C.pndm_init() * s.init_noise_sigma).cuda()
        if layout == "channels_last":
            x = x.contiguous(memory_format=torch.channels_last)
        worst, ts = 0.0, s.timesteps
        assert len(ts) == len(ref)
        for i, t in enumerate(ts):
            xi = s.scale_model_input(x, t)
            out = s.step(C.pndm_fake_model(xi, t), t, x, scaled=True, **step_kwargs(sampler, churn, gen))
            x = out.prev_sample
            assert x.shape == (2, 3, 8, 8) and x.is_contiguous() == (layout == "plain")
            if i + 1 < len(ts):
                assert same_bits(out.scaled_sample, s.scale_model_input(x, ts[i + 1]))
            else:
                assert same_bits(out.scaled_sample, x)                                # the last divisor is 1
            dev = float(np.abs(x.cpu().numpy() - ref[i]).max() / np.abs(ref[i]).max())
            worst = max(worst, dev)
            assert dev <= bound, (layout, i, float(t), dev, bound)
        assert torch.equal(torch.randn(2, 3, 8, 8, generator=gen), torch.from_numpy(g[f"chain_next_{tag}"]))
        print(f"MEASURE kdiff stand-in chain {tag} {layout}: worst step deviation {worst:.3e}, bound {bound:.3e} (reference vs fp64 {dev64:.3e}), "
              f"ratio {worst / bound:.3f}")
    if sampler.startswith("kdpm2"):
        assert not s.state_in_first_order             # the schedule ends on a first order stage; set_timesteps resets it
        s.set_timesteps(n)
        assert s.state_in_first_order


def make_model(mode):
    from baddiffusion_amd.unet import unet_from_config
    cfg = C.SMALL_CFGS[CK.UNET_CFG]
    m = unet_from_config(cfg).cuda()
    m.load_state_dict(U.gen_params(cfg, CK.UNET_PARAM_SEED))
    return m.set_compute_mode(mode)


@pytest.fixture(scope="module")
def models(gpu):
    return {"f32": make_model("f32"), "bf16x3": make_model("bf16x3")}


def hand_loop(model, s, sampler, init, n, gen, churn=0.0, clip=None, start_from=0, frames=None):
    """the pipelines' loop written out with the public pieces (scale_model_input + unet + step, the generator handed to `step`): the
    raw final sample in NHWC storage"""
    from baddiffusion_amd import ops
    s.set_timesteps(n)
    x = ops.nchw_to_nhwc(init.cuda().float()) * s.init_noise_sigma
    ts = s.timesteps[start_from:]
    ts_dev = torch.as_tensor(ts, dtype=torch.float64).float().cuda()
    with torch.no_grad():
        for i, t in enumerate(ts):
            xi = s.scale_model_input(x.permute(0, 3, 1, 2), t)
            if frames is not None:
                frames.append(xi.permute(0, 2, 3, 1))
            eps = model(xi, ts_dev[i]).sample
            x = s.step(eps, t, x.permute(0, 3, 1, 2), clip=clip, **step_kwargs(sampler, churn, gen)).prev_sample.permute(0, 2, 3, 1)
    if frames is not None:
        frames.append(x)
    return x


@pytest.mark.parametrize("mode", ("f32", "bf16x3"))
@pytest.mark.parametrize("case", CK.UNET_CASES, ids=lambda c: CK.unet_tag(*c))
def test_unet_chain_vs_reference_raw_sample(gpu, golden, models, case, mode):
    """the reference scheduler around the reference UNet against the product's scheduler around the product's UNet, on the same noise
    stream, from noise and from noise + trigger: the raw final sample within 1e-3 * max|ref|, the project's standing golden bound"""
    sampler, n, trig = case
    tag = CK.unet_tag(*case)
    ref = golden("kdiff")[f"{tag}_sample"]
    cfg = C.SMALL_CFGS[CK.UNET_CFG]
    init = C.pipeline_init(cfg, CK.UNET_BATCH)
    if trig:
        init = init + CS.trigger(cfg)
    x = hand_loop(models[mode], sched(sampler), sampler, init, n, noise_gen())
    got = x.permute(0, 3, 1, 2).cpu().numpy()
    dev = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"MEASURE kdiff unet chain {tag} mode={mode}: max |x - ref| / max|ref| {dev:.3e} (bound 1e-3, max|ref| {np.abs(ref).max():.1f})")
    assert dev <= 1e-3


# ---------------------------------------------------------------------------------------------------- pipelines
STEPS = {"euler": 6, "euler_a": 6, "kdpm2": 4, "kdpm2_a": 4}
PIPE_CASES = (("euler", 0.0), ("euler", CK.S_CHURN), ("euler_a", 0.0), ("kdpm2", 0.0), ("kdpm2_a", 0.0))


def to_images(x_nhwc):
    return (x_nhwc / 2 + 0.5).clamp(0, 1).cpu().numpy()


def make_pipe(model, sampler, churn=0.0, **kw):
    if sampler == "euler":
        kw.update(s_churn=churn)
    return classes(sampler)[1](model, sched(sampler), **kw)


def evals(sampler, n):
    return 2 * n - 1 if sampler.startswith("kdpm2") else n


@pytest.mark.parametrize("sampler,churn", PIPE_CASES)
def test_pipeline_equals_the_hand_loop(gpu, models, sampler, churn):
    """bitwise, every movie frame included, on one CPU noise stream; two consecutive calls on one generator continue the stream as
    the reference's loop would: the second call's initial noise is what remains after the first call's draws"""
    from baddiffusion_amd import ops
    model = models["bf16x3"]
    init = C.pipeline_init(C.SMALL_CFGS[CK.UNET_CFG], 2)
    n = STEPS[sampler]
    pipe = make_pipe(model, sampler, churn)
    frames = []
    raw = hand_loop(model, sched(sampler), sampler, init, n, noise_gen(), churn=churn, frames=frames)
    r = pipe(init=init, generator=noise_gen(), num_inference_steps=n, output_type="numpy", save_every_step=True)
    assert r.images.shape == (2, 16, 16, 3) and r.images.dtype == np.float32 and len(r.movie) == evals(sampler, n) + 1 == len(frames)
    assert np.array_equal(r.images, to_images(raw)) and np.array_equal(r.movie[-1], r.images)
    for got, want in zip(r.movie, frames):
        assert np.array_equal(got, to_images(want))
    u8 = pipe(init=init, generator=noise_gen(), num_inference_steps=n, output_type="u8").images
    assert u8.is_cuda and u8.dtype == torch.uint8 and torch.equal(u8, ops.to_image(raw, True, (2, 3, 16, 16), want_u8=True)[1])
    pil = pipe(init=init, num_inference_steps=3, save_every_step=True)
    assert len(pil.images) == 2 and pil.images[0].size == (16, 16) and len(pil.movie[0]) == 2
    # two calls on one generator against the reference-ordered stream
    g1, g2, g3 = (torch.Generator().manual_seed(3) for _ in range(3))
    a = pipe(batch_size=2, generator=g1, num_inference_steps=n, output_type=None).images
    b = pipe(batch_size=2, generator=g1, num_inference_steps=n, output_type=None).images
    for got in (a, b):
        start = torch.randn(2, 3, 16, 16, generator=g2)
        want = hand_loop(model, sched(sampler), sampler, start, n, g2, churn=churn)
        assert np.array_equal(got, to_images(want))
    draws = pipe.noise_draws(num_inference_steps=n)
    assert draws == CK.draws_per_chain(sampler, n)
    for _ in range(2 * (1 + draws)):
        torch.randn(2, 3, 16, 16, generator=g3)
    assert torch.equal(torch.randn(1, generator=g1), torch.randn(1, generator=g3)) and not np.array_equal(a, b)
    # generator=None: the noise is drawn on the device; two seeds differ (the deterministic samplers differ by their start)
    torch.manual_seed(1)
    c = pipe(batch_size=2, num_inference_steps=n, output_type=None).images
    torch.manual_seed(2)
    d = pipe(batch_size=2, num_inference_steps=n, output_type=None).images
    assert np.isfinite(c).all() and np.isfinite(d).all() and not np.array_equal(c, d)
    if draws and (sampler != "euler" or churn):     # the same start, device noise: the chain is stochastic
        torch.manual_seed(1)
        c = pipe(init=init, num_inference_steps=n, output_type=None).images
        d = pipe(init=init, num_inference_steps=n, output_type=None).images
        assert not np.array_equal(c, d)
    elif sampler == "euler":                        # s_churn = 0 reads no noise: deterministic from a given start
        assert np.array_equal(pipe(init=init, num_inference_steps=n, output_type=None).images, to_images(raw))


def test_unet_call_counts(gpu, models):
    from baddiffusion_amd.pipelines import with_default_steps
    model = models["bf16x3"]
    init = C.pipeline_init(C.SMALL_CFGS[CK.UNET_CFG], 2)
    calls, keep = [], model.forward
    model.forward = lambda *a, **k: calls.append(a[1]) or keep(*a, **k)
    try:
        for sampler in CK.SAMPLERS:
            pipe, n = make_pipe(model, sampler), STEPS[sampler]
            del calls[:]
            pipe(init=init, num_inference_steps=n, output_type=None)
            assert len(calls) == evals(sampler, n), sampler
            assert all(t.dtype == torch.float32 and t.is_cuda for t in calls)
            assert [float(t) for t in calls] == [float(np.float32(t)) for t in pipe.scheduler.timesteps]
            del calls[:]
            pipe(init=init, output_type=None)                                        # the defaults: 20, 20, 19, 19 evaluations
            assert len(calls) == {"euler": 20, "euler_a": 20, "kdpm2": 19, "kdpm2_a": 19}[sampler]
            del calls[:]
            fixed = with_default_steps(pipe, 3)
            fixed(init=init, output_type=None)
            assert len(calls) == evals(sampler, 3) and fixed.noise_draws() == CK.draws_per_chain(sampler, 3)
    finally:
        model.forward = keep


def restated_loop(model, sampler, churn, init, n, clip, gen, start_from=0):
    """the chain with the kernels' order of operations restated in torch on the CPU around the product UNet: the final scaled sample"""
    from baddiffusion_amd import ops
    s = sched(sampler, n)
    x = init.float() * s.init_noise_sigma
    sc = x / torch.tensor(s._in_div[start_from])
    base = None
    with torch.no_grad():
        for k in range(start_from, len(s.timesteps)):
            t = torch.tensor([s.timesteps[k]], dtype=torch.float64).float().cuda()
            e = model(sc.cuda(), t).sample.cpu().contiguous()
            z = torch.randn(x.shape, generator=gen) if CK.draws_per_chain(sampler, n) else None
            prev, sc = restated_step(plan(s, sampler, k, churn), e, x, z, base, clip=clip)
            base, x = x, prev
    return ops.nchw_to_nhwc(sc.cuda())


@pytest.mark.parametrize("sampler,churn", PIPE_CASES)
def test_pipeline_clip_and_start_from(gpu, models, sampler, churn):
    """clip_sample is the clamp of the kernels' formula: the pipeline equals the chain restated in torch bit for bit, every frame after
    the start lies within the range, and the result differs from the free chain; start_from=k enters at position k of
    `scheduler.timesteps`, and a second-stage position is refused"""
    model = models["bf16x3"]
    init = C.pipeline_init(C.SMALL_CFGS[CK.UNET_CFG], 2)
    n = STEPS[sampler]
    pipe, free_pipe = make_pipe(model, sampler, churn, clip_sample=True, clip_sample_range=0.5), make_pipe(model, sampler, churn)
    r = pipe(init=init, generator=noise_gen(), num_inference_steps=n, output_type=None, save_every_step=True)
    want = restated_loop(model, sampler, churn, init, n, 0.5, noise_gen())
    assert np.array_equal(r.images, to_images(want)) and float(want.abs().max()) <= 0.5
    for frame in r.movie[1:]:
        assert frame.min() >= 0.25 and frame.max() <= 0.75
    free = free_pipe(init=init, generator=noise_gen(), num_inference_steps=n, output_type=None).images
    assert not np.array_equal(free, r.images)
    assert np.array_equal(free, to_images(restated_loop(model, sampler, churn, init, n, None, noise_gen())))
    k = 2                                                                             # a late start, at a first order position
    late = free_pipe(init=init, generator=noise_gen(), num_inference_steps=n, start_from=k, output_type=None, save_every_step=True)
    assert len(late.movie) == 1 + len(free_pipe.scheduler.timesteps) - k
    assert np.array_equal(late.images, to_images(restated_loop(model, sampler, churn, init, n, None, noise_gen(), start_from=k)))
    assert np.array_equal(late.images, to_images(hand_loop(model, sched(sampler), sampler, init, n, noise_gen(), churn=churn, start_from=k)))
    assert free_pipe.noise_draws(num_inference_steps=n, start_from=k) == max(0, CK.draws_per_chain(sampler, n) - k) * (sampler != "kdpm2")
    if sampler.startswith("kdpm2"):
        with pytest.raises(ValueError, match="start_from=3 is the second stage of a transition"):
            free_pipe(init=init, num_inference_steps=n, start_from=3)


@pytest.mark.parametrize("name", ("EULER_O1-SCHED", "EULER_A_O1-SCHED", "KDPM2_O2-SCHED", "KDPM2_A_O2-SCHED"))
def test_command_line_sampling(gpu, tmp_path, monkeypatch, name):
    """baddiffusion.py --mode sampling --sched <name> --infer_steps 3 on a run directory of the small network: the pipeline it samples
    with is the sampler's own at that step count, and the grids are written"""
    import baddiffusion as cli
    from baddiffusion_amd.model import save_scheduler, save_unet
    from baddiffusion_amd.sched_names import SCHEDS
    from baddiffusion_amd.schedulers import DDPMScheduler
    from baddiffusion_amd.unet import unet_from_config
    cfg = dataclasses.replace(C.SMALL_CFGS[CK.UNET_CFG], sample_size=32)
    model = unet_from_config(cfg).cuda()
    model.load_state_dict(U.gen_params(cfg, CK.UNET_PARAM_SEED))
    run = str(tmp_path / "run")
    save_unet(model, os.path.join(run, "unet"))
    save_scheduler(DDPMScheduler(clip_sample=False), os.path.join(run, "scheduler"))
    json.dump({"dataset": "CIFAR10", "batch": 64, "ckpt": "local", "project": "default"}, open(os.path.join(run, "args.json"), "w"))
    monkeypatch.setenv("BD_NUM_IMAGES", "16")
    monkeypatch.chdir(tmp_path)
    seen, real = [], cli.sampling

    def spy(cfg_, name_, pipeline, dsl):
        seen.append((type(pipeline).__name__, type(pipeline.scheduler).__name__, pipeline.noise_draws()))
        return real(cfg_, name_, pipeline, dsl)
    monkeypatch.setattr(cli, "sampling", spy)
    cli.main(["--mode", "sampling", "--ckpt", run, "--sched", name, "--infer_steps", "3"])
    sched_cls, pipe_cls = SCHEDS[name].scheduler.__name__, SCHEDS[name].pipeline.__name__
    draws = {"EULER_O1-SCHED": 3, "EULER_A_O1-SCHED": 3, "KDPM2_O2-SCHED": 0, "KDPM2_A_O2-SCHED": 5}[name]
    assert seen == [(pipe_cls, sched_cls, draws)]
    for folder in ("samples", "backdoor_samples"):
        assert any(f.endswith(".png") for f in os.listdir(os.path.join(run, folder)))
