"""GPU: bd_poison_qsample_corr / bd_qsample_corr against the kernels they share their bodies with, TrainEngine(correction=),
p_losses_diffuser(R_coef=), and the open-loop chains of correction.open_loop_residual through this project's own pipelines.

The old kernels compute rho_t in fp32 themselves; `kernel_rho` reads it back out of bd_qsample (x0 = 0, noise = 0, R = 1), so a table
holding exactly those values must reproduce every output bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_ref as U
from tests.golden import cases as C
from tests.golden import cases_correction as CC

T = CC.T
SHAPES = {"75px": (3, 3, 5, 5), "405px": (5, 3, 9, 9), "405px_c1": (5, 1, 9, 9)}        # one partial block; two blocks, the second ragged
T_SETS = ((0, 1, 500, T - 1), (T - 1, 500, 1, 0))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def tables(gpu):
    al, ac = CC.float_tables()
    return al.to(gpu), ac.to(gpu)


@pytest.fixture(scope="module")
def kernel_rho(gpu, tables):
    """the old kernel's own rho_t for every t, fp32 [T] on the device"""
    from baddiffusion_amd import ops
    z = torch.zeros(T, 1, 1, 1, device=gpu)
    _, tg = ops.qsample(z, torch.ones_like(z), z, torch.arange(T, device=gpu), *tables)
    rho = tg.reshape(T).clone()
    ref = CC.float_tables()
    ref = ((1 - ref[0].double().sqrt()) * (1 - ref[1].double()).sqrt() / (1 - ref[0].double())).numpy()
    # a sanity check only: fp32 1 - sqrt(alpha_t) cancels, one ulp of sqrt(alpha_t) (2^-24) against beta_0 / 2 = 5e-5 is 1.2e-3 relative
    assert (np.abs(rho.cpu().numpy() - ref) / ref).max() <= 2.5e-3
    return rho


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


def poison_inputs(shape, tset, u8, dev):
    """rows that mix clean and poisoned, a trigger with masked and unmasked pixels, timesteps cycling through tset"""
    B, Cc, H, W = shape
    g = torch.Generator().manual_seed(100 * B + H + (7 if u8 else 0))
    trig = torch.rand(Cc, H, W, generator=g) * 2 - 1
    trig[torch.rand(Cc, H, W, generator=g) < 0.5] = -1.0                     # g > vmin fails: the image shows through
    kw = {}
    if u8:
        images = torch.randint(0, 256, (11, H, W, Cc), generator=g, dtype=torch.uint8)      # the resident array is larger than the batch
        kw["row_index"] = torch.randint(0, 11, (B,), generator=g).to(dev)
        kw["flip"] = (torch.arange(B) % 2 == 0).to(torch.uint8).to(dev)
    else:
        images = torch.rand(B, Cc, H, W, generator=g) * 2 - 1
    pois = (torch.arange(B) % 2 == 1)                                         # clean, poisoned, clean, ...
    tgt = torch.rand(Cc, H, W, generator=g) * 2 - 1
    eps = torch.randn(B, Cc, H, W, generator=g)
    t = torch.tensor([tset[b % len(tset)] for b in range(B)])
    return [x.to(dev) for x in (images, pois, trig, tgt, eps, t)], kw, pois.to(dev)


@pytest.mark.parametrize("u8", (True, False), ids=("u8_gather_flip", "f32"))
@pytest.mark.parametrize("tset", T_SETS, ids=("t_up", "t_down"))
@pytest.mark.parametrize("shape", SHAPES.values(), ids=SHAPES.keys())
def test_poison_qsample_corr_with_the_kernels_rho_equals_the_old_kernel(gpu, tables, kernel_rho, shape, tset, u8):
    from baddiffusion_amd import ops
    args, kw, _ = poison_inputs(shape, tset, u8, gpu)
    want = dict(want_batch=True, want_mask=True, want_image=True)
    old = ops.poison_qsample(*args, *tables, **want, **kw)
    new = ops.poison_qsample(*args, *tables, **want, **kw, corr=kernel_rho)
    assert len(old) == len(new) == 6
    for name, a, b in zip(("x_noisy", "target", "R", "x0", "mask", "image"), old, new):
        assert same(a, b), name
    assert not same(old[1], args[4].permute(0, 2, 3, 1).contiguous())         # some row is poisoned: the target is not the noise


@pytest.mark.parametrize("tset", T_SETS, ids=("t_up", "t_down"))
@pytest.mark.parametrize("shape", SHAPES.values(), ids=SHAPES.keys())
def test_qsample_corr_with_the_kernels_rho_equals_the_old_kernel(gpu, tables, kernel_rho, shape, tset):
    from baddiffusion_amd import ops
    B, Cc, H, W = shape
    g = torch.Generator().manual_seed(B + H)
    x0, R, eps = (torch.randn(B, Cc, H, W, generator=g).to(gpu) for _ in range(3))
    R[::2] = 0                                                                # clean rows
    t = torch.tensor([tset[b % 4] for b in range(B)]).to(gpu)
    old = ops.qsample(x0, R, eps, t, *tables)
    new = ops.qsample(x0, R, eps, t, *tables, corr=kernel_rho)
    assert same(old[0], new[0]) and same(old[1], new[1])


def random_table(dev):
    return (torch.rand(T, generator=torch.Generator().manual_seed(77)) * 3 + 1e-3).to(dev)


@pytest.mark.parametrize("table", ("ode", "random"))
@pytest.mark.parametrize("u8", (True, False), ids=("u8_gather_flip", "f32"))
@pytest.mark.parametrize("shape", SHAPES.values(), ids=SHAPES.keys())
def test_poison_qsample_corr_arbitrary_table(gpu, tables, shape, u8, table):
    """target = corr[t] R + eps within one rounding of the product (none if fused) and one of the sum; x_noisy is the old kernel's;
    a clean row's target is eps itself"""
    from baddiffusion_amd import correction, ops
    corr = correction.make_table("ode", Sch(), device=gpu) if table == "ode" else random_table(gpu)
    args, kw, pois = poison_inputs(shape, T_SETS[0], u8, gpu)
    old = ops.poison_qsample(*args, *tables, want_batch=True, **kw)
    new = ops.poison_qsample(*args, *tables, want_batch=True, **kw, corr=corr)
    assert same(old[0], new[0]) and same(old[2], new[2]) and same(old[3], new[3])
    eps, t = args[4], args[5]
    tg = new[1].permute(0, 3, 1, 2)
    assert torch.equal(tg[~pois], eps[~pois]) and not torch.equal(tg[pois], eps[pois])
    prod = corr[t].double().view(-1, 1, 1, 1) * new[2].double()
    err = (tg.double() - (prod + eps.double())).abs()
    bound = 2 * 2.0 ** -24 * (prod.abs() + eps.abs().double())
    print(f"MEASURE poison_qsample_corr {table} {shape} u8={u8}: max err / bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool((err <= bound).all())
    assert float(new[2][pois].abs().max()) > 0 and not same(old[1], new[1])


@pytest.mark.parametrize("table", ("ode", "random"))
@pytest.mark.parametrize("shape", SHAPES.values(), ids=SHAPES.keys())
def test_qsample_corr_arbitrary_table(gpu, tables, shape, table):
    from baddiffusion_amd import correction, ops
    corr = correction.make_table("ode", Sch(), device=gpu) if table == "ode" else random_table(gpu)
    B, Cc, H, W = shape
    g = torch.Generator().manual_seed(B + H + 1)
    x0, R, eps = (torch.randn(B, Cc, H, W, generator=g).to(gpu) for _ in range(3))
    R[::2] = 0
    t = torch.tensor([T_SETS[1][b % 4] for b in range(B)]).to(gpu)
    old = ops.qsample(x0, R, eps, t, *tables)
    xn, tg = ops.qsample(x0, R, eps, t, *tables, corr=corr)
    assert same(old[0], xn)
    tg = tg.permute(0, 3, 1, 2)
    assert torch.equal(tg[::2], eps[::2])
    prod = corr[t].double().view(-1, 1, 1, 1) * R.double()
    err = (tg.double() - (prod + eps.double())).abs()
    assert bool((err <= 2 * 2.0 ** -24 * (prod.abs() + eps.abs().double())).all())


def test_ops_refuse_a_malformed_table(gpu, tables):
    from baddiffusion_amd import ops
    z = torch.zeros(2, 1, 2, 2, device=gpu)
    t = torch.zeros(2, dtype=torch.int64, device=gpu)
    for bad in (torch.ones(T - 1, device=gpu), torch.ones(T, device=gpu, dtype=torch.float64), torch.ones(T, 1, device=gpu)):
        with pytest.raises(ValueError, match="corr must be a float32"):
            ops.qsample(z, z, z, t, *tables, corr=bad)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.qsample(z, z, z, t, *tables, corr=torch.ones(T))


class Sch:
    def __init__(self):
        self.alphas, self.alphas_cumprod = CC.float_tables()


# ---------------------------------------------------------------------------------------------------- engine, loss
B, S = 4, 16
KW = dict(lr=1e-3, lr_warmup_steps=2, num_training_steps=10)


def make_model(dev, seed=7):
    from baddiffusion_amd.unet import unet_from_config
    cfg = C.SMALL_CFGS["small"]                      # 16 x 16, channels (128, 256)
    m = unet_from_config(cfg).to(dev)
    m.load_state_dict(U.gen_params(cfg, seed))
    return m


class Data:
    def __init__(self, dev, steps=3):
        from baddiffusion_amd.dataset import Backdoor
        bd = Backdoor(root=None)
        self.trig = bd.get_trigger("BOX_14", 3, S).to(dev)
        self.tgt = bd.get_target("CORNER", self.trig.cpu()).to(dev)
        self.data = torch.randint(0, 256, (40, S, S, 3), generator=torch.Generator().manual_seed(41), dtype=torch.uint8).to(dev)
        self.pois = torch.tensor([True, False, True, False]).to(dev)
        g = torch.Generator().manual_seed(43)
        self.steps = []
        for _ in range(steps):
            rows = torch.randint(0, 40, (B,), generator=g)
            flip = (torch.rand(B, generator=g) < 0.5).to(torch.uint8)
            eps = torch.randn(B, 3, S, S, generator=g)
            t = torch.randint(0, T, (B,), generator=g)
            self.steps.append(tuple(x.to(dev) for x in (rows, flip, eps, t)))

    def step(self, engine, k):
        rows, flip, eps, t = self.steps[k]
        return engine.train_step(self.data, self.pois, self.trig, self.tgt, eps, t, row_index=rows, flip=flip)


@pytest.fixture(scope="module")
def data(gpu):
    return Data(gpu)


def run(gpu, data, steps, **engine_kw):
    from baddiffusion_amd.schedulers import DDPMScheduler
    from baddiffusion_amd.trainer import TrainEngine
    m = make_model(gpu)
    e = TrainEngine(m, DDPMScheduler(), **KW, **engine_kw)
    losses = [float(data.step(e, k)) for k in range(steps)]
    return m.flat.detach().clone(), losses, e


@pytest.fixture(scope="module")
def plain(gpu, data):
    """TrainEngine() over two eager steps, with the first step's row losses: shared, read-only"""
    from baddiffusion_amd.schedulers import DDPMScheduler
    from baddiffusion_amd.trainer import TrainEngine
    m = make_model(gpu)
    e = TrainEngine(m, DDPMScheduler(), use_graph=False, track_split=True, **KW)
    l0 = float(data.step(e, 0))
    rows0 = e.row_losses.clone()
    l1 = float(data.step(e, 1))
    return {"flat": m.flat.detach().clone(), "losses": [l0, l1], "rows0": rows0, "start": make_model(gpu).flat.detach().clone()}


def test_engine_with_the_kernels_rho_table_is_the_plain_engine(gpu, data, plain, kernel_rho):
    flat, losses, e = run(gpu, data, 2, use_graph=False, correction=kernel_rho)
    assert e.correction is not kernel_rho and torch.equal(e.correction, kernel_rho)          # the engine's own copy
    assert losses == plain["losses"] and torch.equal(flat, plain["flat"]) and not torch.equal(flat, plain["start"])


def test_engine_default_takes_the_old_entry_point(gpu, data, plain, monkeypatch):
    """correction=None never reaches the new entry points: today's launches"""
    from baddiffusion_amd import _lib as L

    def never(*a):
        raise AssertionError("a *_corr entry point was called without a table")
    monkeypatch.setattr(L.load(), "bd_poison_qsample_corr", never)
    monkeypatch.setattr(L.load(), "bd_qsample_corr", never)
    flat, losses, e = run(gpu, data, 1, use_graph=False)
    assert e.correction is None and losses[0] == plain["losses"][0]


def test_engine_graph_step_with_the_kernels_rho_table(gpu, data, kernel_rho):
    """the captured step (one eager, one capture, one replay) reads the engine's static copy of the table: bit-equal to the captured
    step without one"""
    a, la, _ = run(gpu, data, 3, use_graph=True)
    b, lb, e = run(gpu, data, 3, use_graph=True, correction=kernel_rho)
    assert e.use_graph and la == lb and torch.equal(a, b)


def test_engine_with_the_ode_table(gpu, data, plain):
    """another target for the poisoned rows only: the loss differs, the clean rows' own losses do not (first step: same weights)"""
    from baddiffusion_amd import correction
    from baddiffusion_amd.schedulers import DDPMScheduler
    from baddiffusion_amd.trainer import TrainEngine
    sched = DDPMScheduler()
    m = make_model(gpu)
    e = TrainEngine(m, sched, use_graph=False, track_split=True, correction=correction.make_table("ode", sched, device=gpu), **KW)
    loss = float(data.step(e, 0))
    pois = data.pois
    assert loss != plain["losses"][0]
    assert torch.equal(e.row_losses[~pois], plain["rows0"][~pois])
    assert bool((e.row_losses[pois] != plain["rows0"][pois]).all())
    with pytest.raises(ValueError, match="correction must be a"):
        TrainEngine(m, sched, correction=torch.ones(T - 1, device=gpu), **KW)


def test_train_step_batch_passes_the_table(gpu, tables, kernel_rho):
    """the reference's calling convention: collated x_start / R"""
    from baddiffusion_amd.schedulers import DDPMScheduler
    from baddiffusion_amd.trainer import TrainEngine
    g = torch.Generator().manual_seed(5)
    x0, R, eps = (torch.randn(B, 3, S, S, generator=g).to(gpu) for _ in range(3))
    R[1::2] = 0
    t = torch.tensor([0, 1, 500, T - 1]).to(gpu)
    out = []
    for corr in (None, kernel_rho):
        m = make_model(gpu)
        e = TrainEngine(m, DDPMScheduler(), use_graph=False, correction=corr, **KW)
        out.append((float(e.train_step_batch(x0, R, eps, t)), m.flat.detach().clone()))
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1])


def test_p_losses_diffuser_R_coef(gpu):
    from baddiffusion_amd import correction
    from baddiffusion_amd.loss import p_losses_diffuser, q_sample_diffuser
    from baddiffusion_amd.schedulers import DDPMScheduler
    sched = DDPMScheduler()
    m = make_model(gpu)
    cfg = C.SMALL_CFGS["small"]
    x0, R, t, eps = (v.to(gpu) for v in C.train_inputs(cfg, 2))
    table = correction.make_table("ode", sched, device=gpu)
    loss = p_losses_diffuser(sched, m, x0, R, t, eps, "l2", R_coef=table)
    assert loss.requires_grad and loss.dim() == 0
    xn, tg = q_sample_diffuser(sched, x0, R, t, eps, R_coef=table)
    xn0, tg0 = q_sample_diffuser(sched, x0, R, t, eps)
    assert torch.equal(xn, xn0) and not torch.equal(tg, tg0)
    hand = (eps.double() + table[t].double().view(-1, 1, 1, 1) * R.double())
    np.testing.assert_allclose(tg.cpu().numpy(), hand.float().cpu().numpy(), rtol=1e-6, atol=1e-6)
    with torch.no_grad():
        pred = m(xn0, t.contiguous(), return_dict=False)[0]
    ref = float(((pred.double() - hand) ** 2).mean())
    got, plain = float(loss.detach()), float(p_losses_diffuser(sched, m, x0, R, t, eps, "l2").detach())
    print(f"MEASURE p_losses_diffuser(R_coef=ode) {got:.8f} vs hand-built {ref:.8f}, plain {plain:.8f}")
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-6)
    assert plain != got


# ---------------------------------------------------------------------------------------------------- open-loop chains
@pytest.mark.parametrize("tag", CC.CHAINS.keys())
def test_open_loop_chains(gpu, golden, tag):
    """this project's schedulers and pipelines in float32 on the fixture's inputs: the ode table closes every deterministic chain within
    ODE_MAX, the reference's rho misses by more than RHO_MIN, the exact ddim table closes DDIM-50 within DDIM_EXACT_MAX (bounds and
    their reasons: cases_correction.py).  The fixture's own residuals are the reference schedulers' in float64."""
    from baddiffusion_amd import correction
    g = golden("correction")
    kw = dict(target=g["y"], trigger=g["r"], eps=g["eps"])
    pipe, call = CC.build_pipeline(tag)
    ode = correction.open_loop_residual(pipe, g["ode"], **kw, **call)
    rho = correction.open_loop_residual(pipe, g["rho"], **kw, **call)
    print(f"MEASURE open-loop {tag}: ode {ode:.4g} (reference fp64 {float(g['res_ode_' + tag]):.4g}, bound {CC.ODE_MAX}, share {ode / CC.ODE_MAX:.3f}); "
          f"rho {rho:.4g} (reference {float(g['res_rho_' + tag]):.4g}, bound >= {CC.RHO_MIN})")
    assert pipe.unet is None and "_finish" not in vars(pipe)               # the pipeline is as it was
    assert ode <= CC.ODE_MAX
    assert rho >= CC.RHO_MIN
    if tag == "ddim50":
        exact = correction.open_loop_residual(pipe, g["ddim"], **kw, **call)
        print(f"MEASURE open-loop ddim50: exact table {exact:.4g} (reference fp64 {float(g['res_ddim_ddim50']):.4g}, bound {CC.DDIM_EXACT_MAX})")
        assert exact <= CC.DDIM_EXACT_MAX


def test_open_loop_refuses_a_clipping_pipeline(gpu, golden):
    from baddiffusion_amd import correction, pipelines as P, schedulers as S
    g = golden("correction")
    pipe = P.DDIMPipeline(None, S.DDIMScheduler(clip_sample=True))
    with pytest.raises(ValueError, match="clipping"):
        correction.open_loop_residual(pipe, g["ode"], target=g["y"], trigger=g["r"], eps=g["eps"])
