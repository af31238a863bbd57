"""GPU: DEIS sampling on the native path -- bd_deis_step against its formula in fp64 at the sizes where the launcher changes path, bit
for bit on inputs where every operation is exact, its clamps and permitted aliasings, DEISMultistepScheduler against the reference's
chains (tests/golden/deis.npz, written by make_golden_deis.py from the imported diffusers DEISMultistepScheduler) with a stand-in
model and with the product UNet, its float64 coefficient mode against the recurrence in float64 at 1000 steps, and DEISPipeline's
surface.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_ref as U
from tests.golden import cases as C
from tests.golden import cases_deis as CD
from tests.golden.cases_sigma import trigger

# Moderate fixed scalars (a mid-chain step has coefficients of this order).
ALPHA_S, SIGMA_S = 0.8, 0.6
CX, C0 = 0.85, 0.35
ALPHA_T, K0, K1, K2 = 0.9, -0.5, 0.3, -0.15
# TOL (absolute), fixed before the first GPU run.  u = 2^-24 is the relative half-ulp of fp32; inputs are standard normal draws with
# |v| <= 6 (asserted).  Every fp32 operation adds at most u times the magnitude of its own result, and earlier errors pass on with the
# weight of the coefficient they meet:
#   x0   = (x - 0.6 e) / 0.8:  |0.6 e| <= 3.6, |x - ..| <= 9.6, |x0| <= 12 -- the first division      (3.6 + 9.6) u / 0.8 + 12 u = 28.5 u
#   m0   = (x - 0.8 x0) / 0.6: |0.8 x0| <= 9.6                                                         0.8 * 28.5 u + 9.6 u       = 32.4 u
#          x - 0.8 x0 is 0.6 e again, |..| <= 3.6: the difference CANCELS -- it rounds at 3.6 u, but carries the 32.4 u of an
#          operand of magnitude 9.6 undiminished                                                       32.4 u + 3.6 u             = 36 u
#          / 0.6, |m0| <= 6 -- the second division                                                     36 u / 0.6 + 6 u           = 66 u
#          (x0 clamped to [-1, 1]: the clamp is 1-Lipschitz, |0.8 x0| <= 0.8, |x - ..| <= 6.8, |m0| <= 11.4: 62 u, below that)
#   first order   prev = 0.85 x - 0.35 m0: products <= 5.1, 2.1, difference <= 7.2                     5.1 u + (0.35 * 66 + 2.1) u + 7.2 u = 37.5 u
#   third order   prev = 0.9 (x / 0.8 - 0.5 m0 + 0.3 m1 - 0.15 m2): terms <= 7.5, 3, 1.8, 0.9, partial sums <= 10.5, 12.3, 13.2
#          7.5 u + (0.5 * 66 + 3) u + 10.5 u + 1.8 u + 12.3 u + 0.9 u + 13.2 u = 82.2 u;  * 0.9, |prev| <= 11.88:  0.9 * 82.2 u + 11.88 u = 85.9 u
# 86 * 2^-24 = 5.13e-6.  The fp64 side adds nothing visible.  No term shrinks with the result, so this is an atol; the other option
# sets perform a subset of these operations and stay below it.
TOL = 5.2e-6
BIG = 4 * 4096 * 256 + 4 * 256 + 3          # a second grid-stride pass of the 4096-block grid, plus a scalar tail


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def R(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def formula64(e, x, m1, m2, x0_clip=None, clip=None):
    """bd_deis_step's formula (include/bd_hip.h) in fp64 on the fp32 inputs and the fp32 values of the scalars: (x0, m0, prev)"""
    f = lambda v: float(np.float32(v))      # noqa: E731
    d = lambda t: None if t is None else t.double()      # noqa: E731
    e, x, m1, m2 = d(e), d(x), d(m1), d(m2)
    x0 = (x - f(SIGMA_S) * e) / f(ALPHA_S)
    x0c = x0 if x0_clip is None else x0.clamp(-f(x0_clip), f(x0_clip))
    m0 = (x - f(ALPHA_S) * x0c) / f(SIGMA_S)
    if m1 is None:
        prev = f(CX) * x - f(C0) * m0
    else:
        acc = x / f(ALPHA_S) + f(K0) * m0 + f(K1) * m1
        if m2 is not None:
            acc = acc + f(K2) * m2
        prev = f(ALPHA_T) * acc
    if clip is not None:
        prev = prev.clamp(-f(clip), f(clip))
    return x0, m0, prev


def run(e, x, m1, m2, x0_clip=None, clip=None, want_m0=True, out=None, m0_out=None):
    from baddiffusion_amd import ops
    if want_m0 and m0_out is None:
        m0_out = torch.empty_like(x)
    prev = ops.deis_step(e, x, ALPHA_S, SIGMA_S, cx=CX, c0=C0, m1=m1, alpha_t=ALPHA_T, k0=K0, k1=K1, m2=m2, k2=K2, x0_clip=x0_clip,
                         clip=clip, m0_out=m0_out if want_m0 else None, out=out)
    return (m0_out if want_m0 else None), prev


def close(a, b):
    np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.detach().cpu().numpy(), rtol=0, atol=TOL)


# ---------------------------------------------------------------------------------------------------- kernel
# (m1, m2, m0 written, x0_clip)
FULL = (True, True, True, None)
OPTIONS = (FULL,
           (False, False, True, None),          # first order: the first step of a chain
           (True, False, True, None),           # second order
           (True, True, False, None),           # m0 not written
           (False, False, False, None),
           (True, True, True, 1.0),             # thresholding
           (False, False, True, 1.0),
           (True, False, False, 1.0))


@pytest.mark.parametrize("n", (1, 3, 4, 7, 1027, BIG))
def test_step_kernel_against_the_fp64_formula(gpu, n):
    """every size at which the launch changes shape: tail only (1, 3), body only (4), body + tail (7, 1027: several blocks), and a
    second grid-stride pass + tail; first, second and third order, m0 written or not, with and without the x0 clamp"""
    cpu = [R(s, n) for s in (1, 2, 3, 4)]
    assert max(float(t.abs().max()) for t in cpu) <= 6.0                     # what TOL assumes
    e, x, m1, m2 = cpu
    dev = [t.cuda() for t in cpu]
    ed, xd, m1d, m2d = dev
    options = OPTIONS if n != BIG else (FULL, (False, False, True, 1.0))
    for has1, has2, want_m0, x0_clip in options:
        pick = lambda on, t: t if on else None                               # noqa: E731
        m0, prev = run(ed, xd, pick(has1, m1d), pick(has2, m2d), x0_clip=x0_clip, want_m0=want_m0)
        _, m0_64, prev_64 = formula64(e, x, pick(has1, m1), pick(has2, m2), x0_clip=x0_clip)
        close(prev, prev_64)
        if want_m0:
            close(m0, m0_64)
    # the inputs are left as they were
    for d, c in zip(dev, cpu):
        assert torch.equal(d.cpu(), c)


@pytest.mark.parametrize("n", (7, BIG))
def test_step_kernel_is_exact_on_exact_inputs(gpu, n):
    """scalars that are powers of two and small-integer data: every product, quotient and sum is exact in fp32, so neither rounding
    nor contraction can move a bit, and the outputs equal the fp32 restatement of the formula (cases_deis.kernel_formula) bit for bit"""
    from baddiffusion_amd import ops
    ints = lambda seed: torch.randint(-8, 9, (n,), generator=torch.Generator().manual_seed(seed)).float()      # noqa: E731
    e, x, m1, m2 = (ints(s) for s in (31, 32, 33, 34))
    alpha_s, sigma_s, cx, c0, alpha_t, k0, k1, k2 = 0.5, 0.25, 2.0, 0.5, 0.5, 2.0, -1.0, 0.5
    ed, xd, m1d, m2d = (t.cuda() for t in (e, x, m1, m2))
    for order, thr in ((1, False), (2, False), (3, False), (3, True), (1, True)):
        plan = (order, alpha_s, sigma_s, cx, c0, alpha_t, k0, k1, k2)
        for clip in (None, 4.0):
            m0_want, prev_want = CD.kernel_formula(plan, thr, e, x, [m1, m2], clip=clip)
            m0 = torch.empty_like(xd)
            prev = ops.deis_step(ed, xd, alpha_s, sigma_s, cx=cx, c0=c0, m1=m1d if order >= 2 else None, alpha_t=alpha_t, k0=k0, k1=k1,
                                 m2=m2d if order >= 3 else None, k2=k2, x0_clip=1.0 if thr else None, clip=clip, m0_out=m0)
            assert torch.equal(prev.cpu(), prev_want) and torch.equal(m0.cpu(), m0_want), (order, thr, clip)
            if not thr:
                assert torch.equal(m0.cpu(), e)                              # exact arithmetic: the conversion gives e back


def test_step_kernel_clamps(gpu):
    e, x, m1, m2 = (R(s, 2, 3, 9, 7).cuda() for s in (7, 8, 9, 10))         # 378 elements: body + a tail of 2
    cpu = lambda *ts: [t.cpu() for t in ts]                                  # noqa: E731
    for hist in ((m1, m2), (None, None)):
        m0_plain, prev_plain = run(e, x, *hist)
        # post-step clamp: exactly the clamp of the unclipped result; m0 is untouched by it
        for r in (1.0, 0.37):
            m0, prev = run(e, x, *hist, clip=r)
            assert torch.equal(prev, prev_plain.clamp(-r, r)) and torch.equal(m0, m0_plain)
            assert float(prev.abs().max()) == float(np.float32(r)) and float(prev_plain.abs().max()) > 1.0
        # x0 clamp: m0 is rebuilt from the clamped x0 -- on a saturated element it is no longer the model output
        for r in (1.0, 0.5):
            m0, prev = run(e, x, *hist, x0_clip=r)
            x0_64, m0_64, prev_64 = formula64(*cpu(e, x), *(None if h is None else h.cpu() for h in hist), x0_clip=r)
            close(m0, m0_64)
            close(prev, prev_64)
            saturated = (x0_64.abs() > r + 1e-3).cuda()                      # m0 - e = (alpha_s / sigma_s) (x0 - clamp(x0)): > 1.3e-3 there
            inside = (x0_64.abs() < r - 1e-3).cuda()
            assert int(saturated.sum()) > 20 and int(inside.sum()) > 20
            assert float((m0 - e)[saturated].abs().min()) > TOL
            assert float((m0 - e)[inside].abs().max()) <= TOL and torch.equal(m0[inside], m0_plain[inside])
            assert not torch.equal(prev, prev_plain)
            both = run(e, x, *hist, x0_clip=r, clip=0.8)
            assert torch.equal(both[1], prev.clamp(-0.8, 0.8)) and torch.equal(both[0], m0)


def test_step_kernel_layouts_and_checks(gpu):
    from baddiffusion_amd import ops
    e, x, m1 = (R(s, 2, 3, 8, 8).cuda() for s in (13, 14, 15))
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)      # noqa: E731
    base = run(e, x, m1, None)
    got = run(nhwc(e), nhwc(x), nhwc(m1), None)
    assert got[1].stride() == nhwc(x).stride() and all(torch.equal(a, b) for a, b in zip(got, base))
    kw = dict(cx=CX, c0=C0)
    with pytest.raises(ValueError, match="share shape, strides"):
        ops.deis_step(e, nhwc(x), ALPHA_S, SIGMA_S, **kw)
    with pytest.raises(ValueError, match="share shape, strides"):
        ops.deis_step(e.double(), x, ALPHA_S, SIGMA_S, **kw)
    with pytest.raises(ValueError, match="share shape, strides"):
        ops.deis_step(e[:1], x, ALPHA_S, SIGMA_S, **kw)
    with pytest.raises(ValueError, match="share shape, strides"):
        ops.deis_step(e, x, ALPHA_S, SIGMA_S, m1=nhwc(m1), **kw)
    with pytest.raises(ValueError, match="dense"):
        ops.deis_step(e[:, :, ::2], x[:, :, ::2], ALPHA_S, SIGMA_S, **kw)     # a strided view
    with pytest.raises(RuntimeError):
        ops.deis_step(e.cpu(), x, ALPHA_S, SIGMA_S, **kw)
    with pytest.raises(RuntimeError, match="bd_deis_step: m2 without m1"):
        ops.deis_step(e, x, ALPHA_S, SIGMA_S, m2=m1, **kw)
    with pytest.raises(RuntimeError, match="bd_deis_step: alpha_s=0 must be positive"):
        ops.deis_step(e, x, 0.0, SIGMA_S, **kw)
    with pytest.raises(RuntimeError, match="bd_deis_step: sigma_s=-1 must be positive"):
        ops.deis_step(e, x, ALPHA_S, -1.0, **kw)


@pytest.mark.parametrize("n", (7, 1027))
def test_step_kernel_aliasing(gpu, n):
    """prev_out == sample and m0_out == the oldest history buffer (also while it is read as m2 or m1) are bit-identical to the call
    with separate buffers; any other overlap, and a misaligned view, is refused before the launch"""
    from baddiffusion_amd import ops
    e, x, m1, m2 = (R(s, n).cuda() for s in (17, 18, 19, 20))
    kw = dict(x0_clip=1.0, clip=2.0)
    m0, prev = run(e, x, m1, m2, **kw)
    xa = x.clone()
    got = run(e, xa, m1, m2, out=xa, **kw)
    assert got[1] is xa and torch.equal(got[1], prev) and torch.equal(got[0], m0)
    m2a = m2.clone()
    got = run(e, x, m1, m2a, m0_out=m2a, **kw)                               # the oldest buffer is read as m2
    assert got[0] is m2a and torch.equal(got[0], m0) and torch.equal(got[1], prev)
    xa, m2a = x.clone(), m2.clone()                                          # both at once
    got = run(e, xa, m1, m2a, out=xa, m0_out=m2a, **kw)
    assert torch.equal(got[0], m0) and torch.equal(got[1], prev)
    want = run(e, x, m1, None, **kw)                                         # solver_order 2: the oldest buffer is m1
    m1a = m1.clone()
    got = run(e, x, m1a, None, m0_out=m1a, **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # partial overlaps: views of one buffer, 4 elements (16 bytes) apart
    buf = torch.zeros(n + 4, device="cuda")
    p = dict(cx=CX, c0=C0, alpha_t=ALPHA_T, k0=K0, k1=K1, k2=K2)
    for bad in (dict(sample=buf[:n], out=buf[4:]), dict(model_output=buf[4:], out=buf[:n]), dict(m1=buf[:n], m0_out=buf[4:]),
                dict(m1=m1, m2=buf[4:], m0_out=buf[:n]), dict(m1=buf[4:], out=buf[:n])):
        mo, sm = bad.pop("model_output", e), bad.pop("sample", x)
        with pytest.raises(RuntimeError, match="bd_deis_step.*overlaps"):
            ops.deis_step(mo, sm, ALPHA_S, SIGMA_S, **p, **bad)
    with pytest.raises(RuntimeError, match="m0_out overlaps prev_out"):
        ops.deis_step(e, x, ALPHA_S, SIGMA_S, **p, out=buf[:n], m0_out=buf[:n])
    # a view that starts 4 bytes into an aligned buffer
    off = torch.zeros(n + 1, device="cuda")[1:]
    for bad, name in ((dict(out=off), "prev_out"), (dict(m0_out=off), "m0_out"), (dict(m1=off), "m1")):
        with pytest.raises(RuntimeError, match=f"bd_deis_step: {name} is not 16-byte aligned"):
            ops.deis_step(e, x, ALPHA_S, SIGMA_S, **p, **bad)
    with pytest.raises(RuntimeError, match="bd_deis_step: sample is not 16-byte aligned"):
        ops.deis_step(e, off, ALPHA_S, SIGMA_S, **p)
    with pytest.raises(RuntimeError, match="bd_deis_step: m2 without m1"):
        ops.deis_step(e, x, ALPHA_S, SIGMA_S, **p, m2=m2)
    assert float(buf.abs().max()) == 0.0 and float(off.abs().max()) == 0.0    # nothing was launched


# ---------------------------------------------------------------------------------------------------- chains
@pytest.mark.parametrize("case", CD.CHAIN_CASES, ids=lambda c: CD.chain_tag(*c))
def test_stand_in_chain(gpu, golden, case):
    """scheduler.step with cases.pndm_fake_model in place of the UNet, in plain and channels_last layout: every intermediate sample
    within max(4e-6, 4 * dev64) * max|ref| of the reference's, dev64 being the reference's own distance from the recurrence in fp64"""
    from baddiffusion_amd.schedulers import DEISMultistepScheduler
    order, n, thr = case
    g, tag = golden("deis"), CD.chain_tag(*case)
    ref, dev64 = g[f"chain_{tag}"], float(g[f"chain_dev64_{tag}"])
    bound = max(4e-6, 4 * dev64)
    s = DEISMultistepScheduler(**CD.scheduler_kwargs(order, thr))
    for layout in ("plain", "channels_last"):
        s.set_timesteps(n)
        x = C.pndm_init().cuda()
        if layout == "channels_last":
            x = x.contiguous(memory_format=torch.channels_last)
        worst = 0.0
        for i, t in enumerate(s.timesteps.tolist()):
            x_in = x.clone()
            y = s.step(C.pndm_fake_model(x, t), t, x).prev_sample
            assert y.shape == (2, 3, 8, 8) and y.is_contiguous() == (layout == "plain")
            assert torch.equal(x, x_in) and y.data_ptr() != x.data_ptr()      # never in place
            x = y
            dev = float(np.abs(x.cpu().numpy() - ref[i]).max() / np.abs(ref[i]).max())
            worst = max(worst, dev)
            assert dev <= bound, (layout, i, t, dev, bound)
        print(f"MEASURE deis stand-in chain {tag} {layout}: worst step deviation {worst:.3e}, bound {bound:.3e} (reference vs fp64 {dev64:.3e})")
        assert s.lower_order_nums == order


def test_float64_coefficients_follow_the_fp64_recurrence(gpu, golden):
    """coefficient_dtype="float64" at order 3 and 1000 steps on the GPU: within the host test's bound -- 4 x the recorded yardstick,
    floor 4e-6 -- of the stored recurrence in float64 at every stored step (the reference's own chain ends 0.26 * max|x| away)"""
    from baddiffusion_amd.schedulers import DEISMultistepScheduler
    g, tag = golden("deis"), CD.chain_tag(3, 1000, False)
    ref, yard = g[f"long64_{tag}"], float(g[f"long_yard_{tag}"])
    bound = max(4e-6, 4 * yard)
    keep = {i: j for j, i in enumerate(CD.long_steps(999))}
    s = DEISMultistepScheduler(solver_order=3, coefficient_dtype="float64")
    s.set_timesteps(1000)
    x, worst = C.pndm_init().cuda(), 0.0
    for i, t in enumerate(s.timesteps.tolist()):
        x = s.step(C.pndm_fake_model(x, t), t, x).prev_sample
        if i in keep:
            worst = max(worst, float(np.abs(x.cpu().double().numpy() - ref[keep[i]]).max() / np.abs(ref[keep[i]]).max()))
    print(f"MEASURE deis {tag} float64 coefficients on the GPU vs the fp64 recurrence: {worst:.3e} (bound {bound:.3e}, yardstick {yard:.3e}, "
          f"the reference itself {float(g[f'long_ref32_{tag}']):.3e})")
    assert worst <= bound


def test_scheduler_state_checks(gpu):
    from baddiffusion_amd.schedulers import DEISMultistepScheduler
    s = DEISMultistepScheduler(solver_order=2)
    s.set_timesteps(10)
    ts = s.timesteps.tolist()
    x = C.pndm_init().cuda()
    x = s.step(C.pndm_fake_model(x, ts[0]), ts[0], x).prev_sample
    small = x[:1].contiguous()
    with pytest.raises(ValueError, match="one chain per set_timesteps"):
        s.step(small, ts[1], small)
    with pytest.raises(TypeError, match="float32"):
        s.step(x.double(), ts[1], x.double())
    assert type(s.step(x, ts[1], x, return_dict=False)) is tuple
    # a timestep that is not in the table counts as the last one
    s.set_timesteps(10)
    a = s.step(C.pndm_fake_model(x, 5), 5, x).prev_sample
    s.set_timesteps(10)
    assert torch.equal(a, s.step(C.pndm_fake_model(x, 5), ts[-1], x).prev_sample)
    # a first order scheduler keeps no history
    s = DEISMultistepScheduler(solver_order=1)
    s.set_timesteps(4)
    s.step(x, 999, x)
    assert s._ring == [None]


@pytest.fixture(scope="module")
def model(gpu):
    from baddiffusion_amd.unet import unet_from_config
    cfg = C.SMALL_CFGS[CD.UNET_CFG]
    m = unet_from_config(cfg).cuda()
    m.load_state_dict(U.gen_params(cfg, CD.UNET_PARAM_SEED))
    return m


def hand_loop(model, sched, x0, n, clip=None, start_from=0):
    """DEISPipeline's loop restated with ops.deis_step on the scheduler's plan: the raw final sample in NHWC storage [B,H,W,C]"""
    from baddiffusion_amd import ops
    sched.set_timesteps(n)
    x = ops.nchw_to_nhwc(x0.cuda().float())
    ts = sched.timesteps[start_from:]
    ts_dev = torch.as_tensor(ts, dtype=torch.int64).cuda()
    hist = []
    with torch.no_grad():
        for i, t in enumerate(ts):
            eps = model(x.permute(0, 3, 1, 2), ts_dev[i]).sample.permute(0, 2, 3, 1).contiguous()
            order, alpha_s, sigma_s, cx, c0, alpha_t, k0, k1, k2 = sched._plan(sched._step_index(int(t)))
            m0 = torch.empty_like(x)
            x = ops.deis_step(eps, x, alpha_s, sigma_s, cx=cx, c0=c0, m1=hist[0] if order >= 2 else None, alpha_t=alpha_t, k0=k0, k1=k1,
                              m2=hist[1] if order >= 3 else None, k2=k2, x0_clip=1.0 if sched.config.thresholding else None, clip=clip,
                              m0_out=m0)
            hist = [m0] + hist[:1]
            sched._advance()
    return x


@pytest.mark.parametrize("case", CD.UNET_CASES, ids=lambda c: CD.unet_tag(*c))
def test_unet_chain_vs_reference_raw_sample(gpu, golden, model, case):
    """the reference scheduler around the reference UNet against the product's scheduler around the product's UNet in its default
    compute mode, from noise and from noise + trigger: the RAW final sample within 1e-3 * max|ref|, the project's standing golden bound"""
    from baddiffusion_amd import ops
    from baddiffusion_amd.schedulers import DEISMultistepScheduler
    order, n, thr, trig = case
    g, tag = golden("deis"), CD.unet_tag(*case)
    ref, dev64 = g[f"{tag}_sample"], float(g[f"{tag}_dev64"])
    cfg = C.SMALL_CFGS[CD.UNET_CFG]
    init = C.pipeline_init(cfg, CD.UNET_BATCH)
    if trig:
        init = init + trigger(cfg)
    s = DEISMultistepScheduler(**CD.scheduler_kwargs(order, thr))
    s.set_timesteps(n)
    x = ops.nchw_to_nhwc(init.cuda().float())
    ts_dev = torch.as_tensor(s.timesteps, dtype=torch.int64).cuda()
    with torch.no_grad():
        for i, t in enumerate(s.timesteps):
            eps = model(x.permute(0, 3, 1, 2), ts_dev[i]).sample
            x = s.step(eps, int(t), x.permute(0, 3, 1, 2)).prev_sample.permute(0, 2, 3, 1)
    got = x.permute(0, 3, 1, 2).cpu().numpy()
    dev = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"MEASURE deis unet chain {tag}: max |x - ref| / max|ref| {dev:.3e} (bound 1e-3, max|ref| {np.abs(ref).max():.1f}, "
          f"reference fp32 vs fp64 {dev64:.3e})")
    assert dev <= 1e-3


# ---------------------------------------------------------------------------------------------------- pipeline
def to_images(x_nhwc):
    return (x_nhwc / 2 + 0.5).clamp(0, 1).cpu().numpy()


def test_pipeline_equals_the_restated_loop(gpu, model):
    from baddiffusion_amd import ops
    from baddiffusion_amd.pipelines import DEISPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler, DEISMultistepScheduler, UniPCMultistepScheduler
    init = C.pipeline_init(C.SMALL_CFGS[CD.UNET_CFG], 2)
    mk = lambda: DEISMultistepScheduler(solver_order=3, thresholding=True)          # noqa: E731  thresholded: the images are not saturated
    pipe = DEISPipeline(model, mk())
    raw = hand_loop(model, mk(), init, 10)
    want = to_images(raw)
    assert ((want == 0) | (want == 1)).mean() < 0.95
    r = pipe(init=init, num_inference_steps=10, output_type="numpy")
    assert r.images.shape == (2, 16, 16, 3) and r.images.dtype == np.float32 and r.movie == []
    assert np.array_equal(r.images, want)
    # a second chain reuses the kept plan and gives the same bits
    plans = dict(pipe.scheduler._plans)
    assert len(plans) == 10
    assert np.array_equal(pipe(init=init, num_inference_steps=10, output_type="numpy").images, want)
    assert pipe.scheduler._plans.keys() == plans.keys() and all(pipe.scheduler._plans[k] is v for k, v in plans.items())
    # the default step count is 10, and a converted scheduler is second order in the reference's arithmetic
    want10 = to_images(hand_loop(model, DEISMultistepScheduler(), init, 10))
    for foreign in (DDPMScheduler(), UniPCMultistepScheduler(solver_order=2)):
        conv = DEISPipeline(model, foreign)
        assert type(conv.scheduler) is DEISMultistepScheduler and conv.scheduler.config.coefficient_dtype == "float32"
        assert np.array_equal(conv(init=init, output_type=None).images, want10)
    # other outputs
    u8 = pipe(init=init, num_inference_steps=10, output_type="u8").images
    assert u8.is_cuda and u8.dtype == torch.uint8 and torch.equal(u8, ops.to_image(raw, True, (2, 3, 16, 16), want_u8=True)[1])
    pil = pipe(init=init, num_inference_steps=10).images
    assert len(pil) == 2 and pil[0].size == (16, 16)
    assert np.array_equal(pipe(init=init, num_inference_steps=10, output_type="numpy", return_dict=False)[0], want)
    # without init the start is one draw of the generator; nothing is drawn afterwards
    g = torch.Generator().manual_seed(3)
    a = pipe(batch_size=2, generator=g, num_inference_steps=4, output_type=None).images
    after = torch.randn(1, generator=g)
    g2 = torch.Generator().manual_seed(3)
    first = torch.randn(2, 3, 16, 16, generator=g2)
    assert torch.equal(after, torch.randn(1, generator=g2))
    assert np.array_equal(a, pipe(init=first, num_inference_steps=4, output_type=None).images)


def test_pipeline_start_from_movie_and_clip(gpu, model):
    from baddiffusion_amd.pipelines import DEISPipeline
    from baddiffusion_amd.schedulers import DEISMultistepScheduler
    init = C.pipeline_init(C.SMALL_CFGS[CD.UNET_CFG], 2)
    mk = lambda: DEISMultistepScheduler(solver_order=3)      # noqa: E731
    # start_from=k: the last n - k timesteps on a fresh history, so the first executed step is first order; clip_sample is the
    # post-step clamp, folded into the step launch: bit for bit the chain restated with ops.deis_step(..., clip=)
    pipe = DEISPipeline(model, mk(), clip_sample=True, clip_sample_range=0.5)
    r = pipe(init=init, num_inference_steps=10, start_from=4, output_type=None, save_every_step=True)
    want = hand_loop(model, mk(), init, 10, clip=0.5, start_from=4)
    assert np.array_equal(r.images, to_images(want))
    assert len(r.movie) == 1 + 6 and r.movie[0].shape == (2, 16, 16, 3)
    assert np.array_equal(r.movie[0], to_images(init.permute(0, 2, 3, 1))) and np.array_equal(r.movie[-1], r.images)
    s = mk()
    s.set_timesteps(10)
    assert s._plan(4)[0] == 1 and pipe.scheduler.lower_order_nums == 3
    assert float(want.abs().max()) <= 0.5
    for frame in r.movie[1:]:
        assert frame.min() >= 0.25 and frame.max() <= 0.75
    free = DEISPipeline(model, mk())(init=init, num_inference_steps=10, start_from=4, output_type=None).images
    assert np.array_equal(free, to_images(hand_loop(model, mk(), init, 10, start_from=4))) and not np.array_equal(free, r.images)
    # and the full chain differs from the late start
    full = DEISPipeline(model, mk())(init=init, num_inference_steps=10, output_type=None, save_every_step=True)
    assert len(full.movie) == 11 and not np.array_equal(full.images, free)
    pil = DEISPipeline(model, mk())(init=init, num_inference_steps=3, save_every_step=True)
    assert len(pil.movie) == 4 and len(pil.movie[0]) == 2 and pil.movie[0][0].size == (16, 16)
