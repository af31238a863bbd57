"""GPU: the sigma-space samplers on the native path -- bd_timestep_embedding_f32 and UNet2DModel at fractional timesteps, bd_sigma_step
and bd_scale_input held to equal bits against the torch restatement of their order of operations (tests/golden/cases_sigma.py),
HeunDiscreteScheduler / LMSDiscreteScheduler against the reference's chains (tests/golden/sigma.npz, written by make_golden_sigma.py
from the imported diffusers schedulers and UNet), with a stand-in model and with the product UNet, and the surface of HeunPipeline /
LMSPipeline.  Run with -m gpu on an MI355X.

On the commit before fractional timesteps a Python float timestep was truncated (749.25 ran as 749): the reference's output at the
truncated timestep is 6.7e-3 (t = 749.25), 1.2e-2 (20.387755) and 1.5e-2 (0.5) of max|ref| away from the fixture, so
test_unet_forward_at_fractional_timesteps misses its 1e-3 bound there for every t of the list."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_ref as U
from tests.golden import cases as C
from tests.golden import cases_sigma as CS

BETAS = dict(beta_start=0.0001, beta_end=0.02)
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


def _sched(sampler, **kw):
    from baddiffusion_amd.schedulers import HeunDiscreteScheduler, LMSDiscreteScheduler
    return (HeunDiscreteScheduler if sampler == "heun" else LMSDiscreteScheduler)(**{**BETAS, **kw})


# ---------------------------------------------------------------------------------------------------- timestep embedding
def _embed(fn, t_host, dtype, stride, B, dim, flip, shift):
    """one call of an embedding entry point on t laid out with `stride` (0: one value for every row): the [B, dim] result, taken from
    a NaN-margined buffer whose margins are checked"""
    from baddiffusion_amd import _lib as L
    src = torch.zeros(max(1, B * max(stride, 1)), dtype=dtype)
    for b in range(B):
        src[b * stride] = t_host[b] if stride else t_host[0]
    src = src.cuda()
    buf, out = margined(B * dim)
    L.check(fn(src.data_ptr(), stride, B, dim, flip, float(shift), out.data_ptr(), L.stream()), "embedding")
    torch.cuda.synchronize()
    assert margins_intact(buf, B * dim)
    return out.view(B, dim).cpu()


@pytest.mark.parametrize("dim", CS.EMB_DIMS)
def test_timestep_embedding_f32(gpu, golden, dim):
    """integral values: the bits of the int64 entry point (t = 0 and 999 among them); fractional values: within 2e-4 of the reference's
    get_timestep_embedding, the bound DESIGN.md gives the int64 kernel against the oracle (one ulp of expf in f moves an argument of
    ~1e3 by 6e-5)"""
    from baddiffusion_amd import _lib as L
    lib, g = L.load(), golden("sigma")
    ints = [0, 999, 1, 500, 998]
    for B in (1, 5):
        for stride in (0, 1, 2):
            for flip, shift in ((0, 0), (1, 0), (0, 1)):
                if shift == 1 and dim // 2 == 1:
                    continue
                a = _embed(lib.bd_timestep_embedding_f32, [float(v) for v in ints], torch.float32, stride, B, dim, flip, shift)
                b = _embed(lib.bd_timestep_embedding, ints, torch.int64, stride, B, dim, flip, shift)
                assert same_bits(a, b), (B, stride, flip, shift)
                got = _embed(lib.bd_timestep_embedding_f32, list(CS.EMB_TS), torch.float32, stride, B, dim, flip, shift)
                ref = torch.from_numpy(g[f"emb_d{dim}_f{flip}_s{shift}"])[:B]
                if stride == 0:
                    ref = ref[:1].expand(B, dim)
                err = float((got - ref).abs().max())
                assert err <= 2e-4, (B, stride, flip, shift, err)
                # a fractional timestep is not its truncation
                assert float((got[0] - a[0]).abs().max()) > 1e-2


def test_ops_timestep_embedding_takes_float_tensors(gpu, golden):
    from baddiffusion_amd import ops
    g = golden("sigma")
    t = torch.tensor(CS.EMB_TS, dtype=torch.float64)
    for dt in (torch.float64, torch.float32, torch.float16):
        got = ops.timestep_embedding(t.to(dt).cuda(), 128, True, 0).cpu()
        ref = torch.from_numpy(g["emb_d128_f1_s0"])
        if dt == torch.float16:                 # 20.387755 is not a half: compare at the value the half holds
            assert same_bits(got, ops.timestep_embedding(t.to(dt).float().cuda(), 128, True, 0))
        else:
            assert float((got - ref).abs().max()) <= 2e-4
    ints = torch.tensor([0, 999, 7])
    assert same_bits(ops.timestep_embedding(ints.cuda(), 128, False, 1), ops.timestep_embedding(ints.float().cuda(), 128, False, 1))


# ---------------------------------------------------------------------------------------------------- the UNet at fractional timesteps
def make_model(mode):
    from baddiffusion_amd.unet import unet_from_config
    cfg = C.SMALL_CFGS[CS.UNET_CFG]
    m = unet_from_config(cfg).cuda()
    m.load_state_dict(U.gen_params(cfg, CS.UNET_PARAM_SEED))
    return m.set_compute_mode(mode)


@pytest.fixture(scope="module")
def models(gpu):
    return {"f32": make_model("f32"), "bf16x3": make_model("bf16x3")}


@pytest.mark.parametrize("mode", ("f32", "bf16x3"))
def test_unet_forward_at_fractional_timesteps(gpu, golden, models, mode):
    """within the project's standing 1e-3 * max|ref| of the reference UNet at the same fractional timestep; a float32 tensor, a float64
    tensor, a Python float and a per-sample vector of the same value give the same bits"""
    g, model = golden("sigma"), models[mode]
    x = C.pipeline_init(C.SMALL_CFGS[CS.UNET_CFG], CS.UNET_BATCH).cuda()
    with torch.no_grad():
        for t in CS.FRAC_TS:
            ref = g[CS.fwd_tag(t)]
            y = model(x, t).sample                                                    # a Python float
            dev = float(np.abs(y.cpu().numpy() - ref).max() / np.abs(ref).max())
            print(f"MEASURE unet forward at t={t} mode={mode}: max |y - ref| / max|ref| {dev:.3e} (bound 1e-3)")
            assert dev <= 1e-3, (t, dev)
            # the bound tells the timestep from its truncation (what a float timestep computed before the fp32 entry point existed)
            trunc = float(np.abs(model(x, int(t)).sample.cpu().numpy() - ref).max() / np.abs(ref).max())
            print(f"MEASURE unet forward at the truncated t={int(t)} mode={mode}: {trunc:.3e} of max|ref| from the fixture at t={t}")
            assert trunc > 5e-3, (t, trunc)
            for other in (torch.tensor(t, dtype=torch.float64), torch.tensor([t], dtype=torch.float32).cuda(), np.float64(t),
                          torch.tensor([t, t], dtype=torch.float64).cuda(), torch.tensor([t, t], dtype=torch.float32)):
                assert same_bits(model(x, other).sample, y), (t, other)
        ref = g[CS.fwd_tag(CS.FRAC_TS_PER_SAMPLE)]
        y = model(x, torch.tensor(CS.FRAC_TS_PER_SAMPLE, dtype=torch.float64)).sample
        dev = float(np.abs(y.cpu().numpy() - ref).max() / np.abs(ref).max())
        print(f"MEASURE unet forward at per-sample t={CS.FRAC_TS_PER_SAMPLE} mode={mode}: {dev:.3e} (bound 1e-3)")
        assert dev <= 1e-3
        # each row is the row of the broadcast call at its own timestep (samples are independent)
        for b, t in enumerate(CS.FRAC_TS_PER_SAMPLE):
            one = model(x, t).sample
            assert float((one[b] - y[b]).abs().max()) <= 1e-3 * float(y.abs().max())
        with pytest.raises(ValueError, match="timestep must have 1 or 2 elements"):
            model(x, torch.tensor([1.5, 2.5, 3.5]))


def test_integral_float_timesteps_give_the_integer_bits(gpu, models):
    """forward, backward (weights only), backward_input with and without weight gradients: an integral float tensor runs the kernels of
    the int64 tensor on identical embeddings"""
    model = models["bf16x3"]
    cfg = C.SMALL_CFGS[CS.UNET_CFG]
    x0 = C.pipeline_init(cfg, CS.UNET_BATCH).cuda()
    dout = R(5, CS.UNET_BATCH, 3, cfg.sample_size, cfg.sample_size).cuda()
    ti = torch.tensor([999, 250]).cuda()
    with torch.no_grad():
        for t in (ti, torch.tensor([0]).cuda(), 999):
            tf = float(t) if not torch.is_tensor(t) else t.double()
            assert same_bits(model(x0, tf).sample, model(x0, t).sample)

    def grads(t, need_w, need_x):
        model.flat.requires_grad_(need_w)
        model.flat.grad = None
        x = x0.clone().requires_grad_(need_x)
        y = model(x, t).sample
        y.backward(dout)
        out = (y.detach().clone(), model.flat.grad.clone() if need_w else None, x.grad.clone() if need_x else None)
        model.flat.grad = None
        return out

    try:
        for need_w, need_x in ((True, False), (True, True), (False, True)):
            a, b = grads(ti, need_w, need_x), grads(ti.float(), need_w, need_x)
            for u, v in zip(a, b):
                assert (u is None) == (v is None)
                if u is not None:
                    assert same_bits(u, v), (need_w, need_x)
            assert (a[1] is not None) == need_w and (a[2] is not None) == need_x
            # and a fractional timestep runs through the same backward entry points
            c = grads(ti.float() + 0.25, need_w, need_x)
            assert all(torch.isfinite(v).all() for v in c if v is not None) and not same_bits(c[0], a[0])
    finally:
        model.flat.requires_grad_(True)
        model.flat.grad = None


# ---------------------------------------------------------------------------------------------------- bd_sigma_step, bd_scale_input
def schedule_points():
    """(sigma_in, c0..c3, in_div) of LMS order 4 at 10 steps: the first step (sigma = 157.4), a middle one and the last (in_div = 1);
    c1..c3 of the first step, which has no history in a chain, are borrowed from the middle one"""
    s = _sched("lms")
    s.set_timesteps(10, order=4)
    mid = s._plan_scalars(5, 4)
    pts = []
    for k in (0, 5, 9):
        sigma_in, c, in_div = s._plan_scalars(k, 4)
        pts.append((sigma_in, tuple(c) + tuple(mid[1][len(c):]), in_div))
    assert abs(pts[0][0] - 157.4) < 0.05 and pts[2][2] == 1.0 and all(len(p[1]) == 4 for p in pts)
    return pts


STAGES = (("euler", False, 0), ("average", True, 0), ("lms1", False, 1), ("lms2", False, 2), ("lms3", False, 3))
OUTPUTS = ((True, True, True), (False, False, False), (True, False, True), (False, True, False))       # x0_out, d_out, scaled_out


def run_sigma_case(n, e, x, b, hs, pt, stage, outs, use_base, clip):
    """one launch into NaN-margined outputs, compared bit for bit with the restatement"""
    from baddiffusion_amd import ops
    name, average, nh = stage
    sigma_in, c, in_div = pt
    dev = lambda t: t.cuda()
    hist = hs[:1] if average else hs[:nh]
    kw = dict(base=dev(b) if use_base else None, average=average, clip=clip)
    for j, h in enumerate(hist):
        kw[f"h{j + 1}"] = dev(h)
    if not average:
        for j in range(nh):
            kw[f"c{j + 1}"] = c[j + 1]
    bufs = {k: margined(n) for k in ("x0_out", "d_out", "scaled_out", "out")}
    for k, on in zip(("x0_out", "d_out", "scaled_out"), outs):
        kw[k] = bufs[k][1] if on else None
    ed, xd = dev(e), dev(x)
    prev = ops.sigma_step(ed, xd, sigma_in, c[0], in_div, out=bufs["out"][1], **kw)
    torch.cuda.synchronize()
    want = CS.sigma_step_ref(e, x, sigma_in, c, in_div, base=b if use_base else None, average=average, hist=hist, clip=clip)
    tag = (n, name, outs, use_base, clip, sigma_in)
    assert prev is bufs["out"][1] and same_bits(prev, want[2]), tag
    for k, w, on in zip(("x0_out", "d_out", "scaled_out"), (want[0], want[1], want[3]), outs):
        if on:
            assert same_bits(bufs[k][1], w), (k,) + tag
        else:
            assert bool(torch.isnan(bufs[k][0]).all()), (k,) + tag                  # an absent output is not written
        assert margins_intact(bufs[k][0], n), (k,) + tag
    assert margins_intact(bufs["out"][0], n), tag
    assert same_bits(ed, e) and same_bits(xd, x)                                     # the inputs are left as they were
    return want


@pytest.mark.parametrize("n", (1, 3, 4, 5, 1023, 4103))
def test_sigma_step_equals_the_restatement(gpu, n):
    """tail only (1, 3), body only (4), body + tail (5, 1023, 4103: several blocks); every stage x which optional outputs are written x
    base or not x clip or not, at scalars of a real schedule (sigma = 157.4 and the last step's in_div = 1 among them)"""
    pts = schedule_points()
    e, b, h1, h2, h3 = (R(s, n) for s in (1, 2, 3, 4, 5))
    i = 0
    for stage in STAGES:
        for outs in OUTPUTS:
            for use_base in (False, True):
                for clip in (None, 1.0):
                    pt = pts[i % 3]
                    i += 1
                    x = R(6 + i, n) * float(np.float32((pt[0] ** 2 + 1) ** 0.5))      # a raw sample at this noise level
                    want = run_sigma_case(n, e, x, b * pt[0], (h1, h2, h3), pt, stage, outs, use_base, clip)
                    if clip is not None:
                        assert float(want[3].abs().max()) <= 1.0
                        assert same_bits(want[2], want[3] * torch.tensor(float(np.float32(pt[2]))))


def test_sigma_step_grid_stride_pass(gpu):
    """4096 * 256 * 4 + 5 elements: the grid-stride loop takes a second pass and the tail follows it; each stage once"""
    pts = schedule_points()
    n = BIG
    e, b, h1, h2, h3 = (R(s, n) for s in (11, 12, 13, 14, 15))
    x = R(16, n) * 3.0
    for i, stage in enumerate(STAGES):
        run_sigma_case(n, e, x, b, (h1, h2, h3), pts[i % 3], stage, OUTPUTS[i % 2], bool(i % 2), 1.0 if i % 2 else None)


def test_sigma_step_clip_is_a_clamp_of_the_scaled_sample(gpu):
    from baddiffusion_amd import ops
    sigma_in, c, in_div = schedule_points()[1]
    e, x = R(21, 2, 3, 9, 7).cuda(), (R(22, 2, 3, 9, 7) * sigma_in).cuda()                # 378 elements: body + a tail of 2
    sc0, sc1 = torch.empty_like(x), torch.empty_like(x)
    free = ops.sigma_step(e, x, sigma_in, c[0], in_div, scaled_out=sc0)
    for r in (1.0, 0.37):
        clipped = ops.sigma_step(e, x, sigma_in, c[0], in_div, scaled_out=sc1, clip=r)
        assert same_bits(sc1, sc0.clamp(-r, r)) and float(sc1.abs().max()) == float(np.float32(r))
        assert same_bits(clipped, sc1 * torch.tensor(in_div, device="cuda")) and not same_bits(clipped, free)
    # without clip the scaled output is the division of the raw one: what scale_model_input computes from it
    assert same_bits(sc0, ops.scale_input(free, 1.0, in_div)) and same_bits(sc0, free.cpu() / torch.tensor(in_div))


@pytest.mark.parametrize("n", (7, 1027))
def test_sigma_step_aliasing(gpu, n):
    """d_out == the oldest history buffer (read as h3, or not read at all) and prev_out == sample are bit-identical to the call with
    separate buffers; any other overlap is refused before the launch"""
    from baddiffusion_amd import ops
    sigma_in, c, in_div = schedule_points()[1]
    e, x, h1, h2, h3 = (R(s, n).cuda() for s in (31, 32, 33, 34, 35))
    kw = dict(h1=h1, c1=c[1], h2=h2, c2=c[2], c3=c[3], clip=2.0)
    d, sc = torch.empty_like(x), torch.empty_like(x)
    prev = ops.sigma_step(e, x, sigma_in, c[0], in_div, h3=h3, d_out=d, scaled_out=sc, **kw)
    h3a, sca = h3.clone(), torch.empty_like(x)
    preva = ops.sigma_step(e, x, sigma_in, c[0], in_div, h3=h3a, d_out=h3a, scaled_out=sca, **kw)
    assert same_bits(preva, prev) and same_bits(h3a, d) and same_bits(sca, sc)
    xa, h3a = x.clone(), h3.clone()                                                   # both at once: a sampling loop stepping in place
    prevb = ops.sigma_step(e, xa, sigma_in, c[0], in_div, h3=h3a, d_out=h3a, out=xa, **kw)
    assert prevb is xa and same_bits(prevb, prev) and same_bits(h3a, d)
    old = h2.clone()                                                                  # second order: the oldest buffer is not an operand
    want = ops.sigma_step(e, x, sigma_in, c[0], in_div, h1=h1, c1=c[1])
    got = ops.sigma_step(e, x, sigma_in, c[0], in_div, h1=h1, c1=c[1], d_out=old)
    assert same_bits(got, want) and same_bits(old, d)
    # partial overlaps: views of one buffer, 4 elements (16 bytes) apart
    buf = torch.zeros(n + 4, device="cuda")
    for mo, sm, k in ((e, buf[:n], dict(out=buf[4:])), (buf[4:], x, dict(out=buf[:n])), (e, x, dict(h1=buf[:n], d_out=buf[4:])),
                      (e, x, dict(base=buf[4:], scaled_out=buf[:n])), (e, x, dict(out=buf[:n], scaled_out=buf[4:])),
                      (e, x, dict(out=buf[:n], d_out=buf[:n]))):
        with pytest.raises(RuntimeError, match="bd_sigma_step.*overlaps"):
            ops.sigma_step(mo, sm, sigma_in, c[0], in_div, **k)
    assert float(buf.abs().max()) == 0.0                                              # nothing was launched


def test_sigma_step_layouts_and_checks(gpu):
    from baddiffusion_amd import ops
    sigma_in, c, in_div = schedule_points()[1]
    e, x, h1 = (R(s, 2, 3, 8, 8).cuda() for s in (41, 42, 43))
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    base = ops.sigma_step(e, x, sigma_in, c[0], in_div, h1=h1, c1=c[1])
    got = ops.sigma_step(nhwc(e), nhwc(x), sigma_in, c[0], in_div, h1=nhwc(h1), c1=c[1])
    assert got.stride() == nhwc(x).stride() and same_bits(got.contiguous(), base)
    with pytest.raises(ValueError, match="share shape, strides"):
        ops.sigma_step(e, nhwc(x), sigma_in, c[0], in_div)
    with pytest.raises(ValueError, match="share shape, strides"):
        ops.sigma_step(e.double(), x, sigma_in, c[0], in_div)
    with pytest.raises(ValueError, match="dense"):
        ops.sigma_step(e[:, :, ::2], x[:, :, ::2], sigma_in, c[0], in_div)
    with pytest.raises(RuntimeError):
        ops.sigma_step(e.cpu(), x, sigma_in, c[0], in_div)
    with pytest.raises(RuntimeError, match="bd_sigma_step: average without h1"):
        ops.sigma_step(e, x, sigma_in, c[0], in_div, average=True)


@pytest.mark.parametrize("n", (1, 3, 4, 5, 1023, 4103, BIG))
def test_scale_input_equals_the_restatement(gpu, n):
    from baddiffusion_amd import ops
    s = _sched("lms")
    s.set_timesteps(10)
    x = R(51, n)
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)
    for mul, div in ((s.init_noise_sigma, s._in_div[0]), (1.0, s._in_div[5]), (s.init_noise_sigma, 1.0), (1.0, 1.0)):
        buf, out = margined(n)
        got = ops.scale_input(x.cuda(), mul, div, out=out)
        torch.cuda.synchronize()
        assert got is out and same_bits(got, (x * f(mul)) / f(div)) and margins_intact(buf, n), (n, mul, div)
    xa = x.cuda()
    assert ops.scale_input(xa, s.init_noise_sigma, s._in_div[0], out=xa) is xa                 # in place
    assert same_bits(xa, (x * f(s.init_noise_sigma)) / f(s._in_div[0]))
    if n > 8:
        buf = torch.zeros(n + 4, device="cuda")
        with pytest.raises(RuntimeError, match="bd_scale_input: out overlaps x"):
            ops.scale_input(buf[:n], 1.0, 2.0, out=buf[4:])


# ---------------------------------------------------------------------------------------------------- chains
def step_kwargs(sampler, order):
    return {"order": order} if sampler == "lms" else {}


@pytest.mark.parametrize("case", CS.CHAIN_CASES, ids=lambda c: CS.chain_tag(*c))
def test_stand_in_chain(gpu, golden, case):
    """scale_model_input + scheduler.step with cases.pndm_fake_model in place of the UNet, in plain and channels_last layout: every
    intermediate sample within max(4e-6, 4 * dev64) * max|ref| of the reference's, dev64 being the reference's own distance from the
    recurrence in fp64; the step's scaled output is the next scale_model_input bit for bit"""
    sampler, order, n = case
    g, tag = golden("sigma"), CS.chain_tag(*case)
    ref, dev64 = g[f"chain_{tag}"], float(g[f"chain_dev64_{tag}"])
    bound = max(4e-6, 4 * dev64)
    s = _sched(sampler)
    for layout in ("plain", "channels_last"):
        s.set_timesteps(n)
        x = (C.pndm_init() * s.init_noise_sigma).cuda()
        if layout == "channels_last":
            x = x.contiguous(memory_format=torch.channels_last)
        worst, ts = 0.0, s.timesteps
        assert len(ts) == len(ref)
        for i, t in enumerate(ts):
            xi = s.scale_model_input(x, t)
            out = s.step(C.pndm_fake_model(xi, t), t, x, scaled=True, **step_kwargs(sampler, order))
            x = out.prev_sample
            assert x.shape == (2, 3, 8, 8) and x.is_contiguous() == (layout == "plain")
            if i + 1 < len(ts):
                assert same_bits(out.scaled_sample, s.scale_model_input(x, ts[i + 1]))
            else:
                assert same_bits(out.scaled_sample, x)                                # the last divisor is 1
            dev = float(np.abs(x.cpu().numpy() - ref[i]).max() / np.abs(ref[i]).max())
            worst = max(worst, dev)
            assert dev <= bound, (layout, i, float(t), dev, bound)
        print(f"MEASURE sigma stand-in chain {tag} {layout}: worst step deviation {worst:.3e}, bound {bound:.3e} (reference vs fp64 {dev64:.3e})")
    if sampler == "heun":
        assert s.state_in_first_order
    else:
        assert len(s._ring) == order - 1


def hand_loop(model, sched, init, n, order=None, clip=None, start_from=0, frames=None):
    """the pipelines' loop written out with the public pieces (scale_model_input + unet + step): the raw final sample in NHWC storage"""
    from baddiffusion_amd import ops
    sched.set_timesteps(n)
    kw = {} if order is None else {"order": order}
    x = ops.nchw_to_nhwc(init.cuda().float()) * sched.init_noise_sigma
    ts = sched.timesteps[start_from:]
    ts_dev = torch.as_tensor(ts, dtype=torch.float64).float().cuda()
    with torch.no_grad():
        for i, t in enumerate(ts):
            xi = sched.scale_model_input(x.permute(0, 3, 1, 2), t)
            if frames is not None:
                frames.append(xi.permute(0, 2, 3, 1))
            eps = model(xi, ts_dev[i]).sample
            x = sched.step(eps, t, x.permute(0, 3, 1, 2), clip=clip, **kw).prev_sample.permute(0, 2, 3, 1)
    if frames is not None:
        frames.append(x)
    return x


@pytest.mark.parametrize("mode", ("f32", "bf16x3"))
@pytest.mark.parametrize("case", CS.UNET_CASES, ids=lambda c: CS.unet_tag(*c))
def test_unet_chain_vs_reference_raw_sample(gpu, golden, models, case, mode):
    """the reference scheduler around the reference UNet against the product's scheduler around the product's UNet, from noise and from
    noise + trigger: the raw final sample within 1e-3 * max|ref|, the project's standing golden bound"""
    sampler, order, n, trig = case
    g, tag = golden("sigma"), CS.unet_tag(*case)
    ref, dev64 = g[f"{tag}_sample"], float(g[f"{tag}_dev64"])
    cfg = C.SMALL_CFGS[CS.UNET_CFG]
    init = C.pipeline_init(cfg, CS.UNET_BATCH)
    if trig:
        init = init + CS.trigger(cfg)
    x = hand_loop(models[mode], _sched(sampler), init, n, order=order if sampler == "lms" else None)
    got = x.permute(0, 3, 1, 2).cpu().numpy()
    dev = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"MEASURE sigma unet chain {tag} mode={mode}: max |x - ref| / max|ref| {dev:.3e} (bound 1e-3, max|ref| {np.abs(ref).max():.1f}, "
          f"reference fp32 vs fp64 {dev64:.3e})")
    assert dev <= 1e-3


# ---------------------------------------------------------------------------------------------------- pipelines
def to_images(x_nhwc):
    return (x_nhwc / 2 + 0.5).clamp(0, 1).cpu().numpy()


def pipes(model, clip=False, clip_range=1.0):
    from baddiffusion_amd.pipelines import HeunPipeline, LMSPipeline
    return {"heun": (HeunPipeline(model, _sched("heun"), clip_sample=clip, clip_sample_range=clip_range), None, 5),
            "lms": (LMSPipeline(model, _sched("lms"), clip_sample=clip, clip_sample_range=clip_range, order=3), 3, 6)}


@pytest.mark.parametrize("sampler", ("heun", "lms"))
def test_pipeline_equals_the_hand_loop(gpu, models, sampler):
    """bitwise, every movie frame included: the frames are the scaled buffers (the model inputs, then the final sample), and the first
    one is init * init_noise_sigma / sqrt(sigma_0^2 + 1)"""
    from baddiffusion_amd import ops
    model = models["bf16x3"]
    init = C.pipeline_init(C.SMALL_CFGS[CS.UNET_CFG], 2)
    pipe, order, n = pipes(model)[sampler]
    frames = []
    raw = hand_loop(model, _sched(sampler), init, n, order=order, frames=frames)
    r = pipe(init=init, num_inference_steps=n, output_type="numpy", save_every_step=True)
    evals = 2 * n - 1 if sampler == "heun" else n
    assert r.images.shape == (2, 16, 16, 3) and r.images.dtype == np.float32 and len(r.movie) == evals + 1 == len(frames)
    assert np.array_equal(r.images, to_images(raw)) and np.array_equal(r.movie[-1], r.images)
    for got, want in zip(r.movie, frames):
        assert np.array_equal(got, to_images(want))
    s = pipe.scheduler
    first = (init.permute(0, 2, 3, 1) * s.init_noise_sigma) / torch.tensor(s._in_div[0])       # on the host: one rounding per operation
    assert np.array_equal(r.movie[0], to_images(first)) and s.init_noise_sigma > 157
    assert ((r.movie[0] == 0) | (r.movie[0] == 1)).mean() < 0.5                      # an image of the scaled start, not of the raw one
    # deterministic, state reset between calls; no movie unless asked
    again = pipe(init=init, num_inference_steps=n, output_type="numpy")
    assert np.array_equal(again.images, r.images) and again.movie == []
    # other outputs
    u8 = pipe(init=init, num_inference_steps=n, output_type="u8").images
    assert u8.is_cuda and u8.dtype == torch.uint8 and torch.equal(u8, ops.to_image(raw, True, (2, 3, 16, 16), want_u8=True)[1])
    pil = pipe(init=init, num_inference_steps=2, save_every_step=True)
    assert len(pil.images) == 2 and pil.images[0].size == (16, 16) and len(pil.movie[0]) == 2
    assert pipe(init=init, num_inference_steps=n, output_type=None, return_dict=False)[0].shape == (2, 16, 16, 3)
    # from a generator: the start is the one draw, nothing afterwards
    g1 = torch.Generator().manual_seed(3)
    a = pipe(batch_size=2, generator=g1, num_inference_steps=2, output_type=None).images
    after = torch.randn(1, generator=g1)
    g2 = torch.Generator().manual_seed(3)
    start = torch.randn(2, 3, 16, 16, generator=g2)
    assert torch.equal(after, torch.randn(1, generator=g2)) and pipe.noise_draws(num_inference_steps=2) == 0
    assert np.array_equal(a, pipe(init=start, num_inference_steps=2, output_type=None).images)


def test_heun_makes_2n_minus_1_unet_calls(gpu, models):
    from baddiffusion_amd.pipelines import with_default_steps
    model = models["bf16x3"]
    init = C.pipeline_init(C.SMALL_CFGS[CS.UNET_CFG], 2)
    calls, keep = [], model.forward
    model.forward = lambda *a, **k: calls.append(a[1]) or keep(*a, **k)
    try:
        for sampler, (pipe, order, n) in pipes(model).items():
            del calls[:]
            pipe(init=init, num_inference_steps=n, output_type=None)
            assert len(calls) == (2 * n - 1 if sampler == "heun" else n), sampler
            assert all(t.dtype == torch.float32 and t.is_cuda for t in calls)
            want = [float(np.float32(t)) for t in pipe.scheduler.timesteps]
            assert [float(t) for t in calls] == want
        # the defaults, through the wrapper --infer_steps uses: 10 steps of Heun are 19 evaluations, 20 of LMS 20
        heun, lms = pipes(model)["heun"][0], pipes(model)["lms"][0]
        for pipe, default, fixed, evals in ((heun, 19, 3, 5), (lms, 20, 4, 4)):
            del calls[:]
            pipe(init=init, output_type=None)
            assert len(calls) == default
            del calls[:]
            fixed_pipe = with_default_steps(pipe, fixed)
            a = fixed_pipe(init=init, output_type=None).images
            assert len(calls) == evals and type(fixed_pipe).__name__ == type(pipe).__name__
            assert np.array_equal(a, fixed_pipe(init=init, num_inference_steps=fixed, output_type=None).images)
    finally:
        model.forward = keep


def restated_loop(model, sampler, order, init, n, clip, start_from=0):
    """the chain with the kernel's order of operations restated in torch on the CPU (cases_sigma.sigma_step_ref) around the product
    UNet: the final scaled sample"""
    from baddiffusion_amd import ops
    s = _sched(sampler)
    s.set_timesteps(n)
    x = init.float() * s.init_noise_sigma
    sc = x / torch.tensor(s._in_div[start_from])
    stage, ring = None, []
    with torch.no_grad():
        for k in range(start_from, len(s.timesteps)):
            t = torch.tensor([s.timesteps[k]], dtype=torch.float64).float().cuda()
            e = model(sc.cuda(), t).sample.cpu().contiguous()
            if sampler == "heun":
                sigma_in, dt, in_div = s._plan_scalars(k)
                if k % 2 == 0:
                    _, d, prev, sc = CS.sigma_step_ref(e, x, sigma_in, (dt,), in_div, clip=clip)
                    stage = (d, dt, x)
                else:
                    _, _, prev, sc = CS.sigma_step_ref(e, x, sigma_in, (stage[1],), in_div, base=stage[2], average=True, hist=(stage[0],),
                                                       clip=clip)
            else:
                sigma_in, coeffs, in_div = s._plan_scalars(k, order)
                terms = min(len(coeffs), 1 + len(ring))
                _, d, prev, sc = CS.sigma_step_ref(e, x, sigma_in, coeffs[:terms], in_div, hist=ring[::-1][:terms - 1], clip=clip)
                ring = (ring + [d])[-(order - 1):] if order > 1 else []
            x = prev
    return ops.nchw_to_nhwc(sc.cuda())


@pytest.mark.parametrize("sampler", ("heun", "lms"))
def test_pipeline_clip_and_start_from(gpu, models, sampler):
    """clip_sample is the clamp of bd_sigma_step's formula: the pipeline equals the chain restated in torch bit for bit, every frame
    after the start lies within the range, and the result differs from the free chain; start_from=k enters at position k with an empty
    history"""
    model = models["bf16x3"]
    init = C.pipeline_init(C.SMALL_CFGS[CS.UNET_CFG], 2)
    pipe, order, n = pipes(model, clip=True, clip_range=0.5)[sampler]
    r = pipe(init=init, num_inference_steps=n, output_type=None, save_every_step=True)
    want = restated_loop(model, sampler, order, init, n, 0.5)
    assert np.array_equal(r.images, to_images(want)) and float(want.abs().max()) <= 0.5
    for frame in r.movie[1:]:
        assert frame.min() >= 0.25 and frame.max() <= 0.75
    free_pipe = pipes(model)[sampler][0]
    free = free_pipe(init=init, num_inference_steps=n, output_type=None).images
    assert not np.array_equal(free, r.images)
    # a late start
    k = 4
    late = free_pipe(init=init, num_inference_steps=n, start_from=k, output_type=None, save_every_step=True)
    raw = hand_loop(model, _sched(sampler), init, n, order=order, start_from=k)
    assert np.array_equal(late.images, to_images(raw)) and len(late.movie) == 1 + len(free_pipe.scheduler.timesteps) - k
    assert np.array_equal(late.images, to_images(restated_loop(model, sampler, order, init, n, None, start_from=k)))
    clipped_late = pipe(init=init, num_inference_steps=n, start_from=k, output_type=None).images
    assert np.array_equal(clipped_late, to_images(restated_loop(model, sampler, order, init, n, 0.5, start_from=k)))
    if sampler == "heun":
        with pytest.raises(ValueError, match="start_from=3 is the second entry of a timestep pair"):
            free_pipe(init=init, num_inference_steps=n, start_from=3)
    else:       # past the end: nothing runs, the start comes back unscaled
        none = free_pipe(init=init, num_inference_steps=n, start_from=n, output_type=None).images
        assert np.array_equal(none, to_images(init.permute(0, 2, 3, 1)))
