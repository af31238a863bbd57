"""GPU: the clean-data term of remove_backdoor on the grouped loss (TrainEngine groups=, defense.remove_backdoor clean=,
synthesize_clean, prediction_drift) and the --clean_source flags of elijah_defense.py.

Bounds.  Gradients against a second computation: worst norm-relative difference < 1e-3, losses and gradient norms per step at rtol 1e-3,
the bounds of test_defense.py::test_remove_backdoor_vs_oracle.  The grouped step's total against its two parts: rtol 1e-6 (fp64 sums
rounded to fp32 once each).  prediction_drift against metrics.mse on the same rows: rtol 1e-6; there is no oracle comparison for it,
the quantity is a difference of nearly equal predictions and compute-mode error does not cancel.
One history entry has the exact value 0 and no relative bound can apply to it: loss_clean of step 0 with clean_target="frozen", where the
model still equals its frozen copy and both sides hold only the rounding of two forwards of different batch sizes (5.6e-13 in the oracle).
It is bounded absolutely instead: two forwards within the project's 1e-3 norm-relative bar (smoke(), test_hip_unet.py) of the exact
prediction differ by at most 2e-3 of its norm, so loss_clean <= (2e-3)^2 * mean(target^2).  Every other entry keeps rtol 1e-3."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import backdoor_ref as B
from oracle import loss_ref, sched_ref
from oracle import unet_ref as U
from tests.golden import cases as C

CLEAN_WEIGHT = 0.5
HIST_KEYS = {"loss", "grad_norm", "loss_clean", "loss_shift"}


@pytest.fixture(scope="module")
def bd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from baddiffusion_amd import _lib as L
    import baddiffusion_amd.ops as ops
    import baddiffusion_amd.unet as unet
    return L, ops, unet


def make_model(unet, cfg, seed, mode):
    m = unet.unet_from_config(cfg).cuda()
    m.load_state_dict(U.gen_params(cfg, seed))
    return m.set_compute_mode(mode)


def clean_u8():
    """8 random uint8 [16, 16, 3] images"""
    return torch.randint(0, 256, (8, 16, 16, 3), generator=torch.Generator().manual_seed(31), dtype=torch.uint8)


def fixed_draws(steps, cb, seed=17):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(8, (cb,), generator=g), torch.randint(1000, (cb,), generator=g), torch.randn(cb, 3, 16, 16, generator=g))
            for _ in range(steps)]


def worst_rel(got, ref):
    """worst norm-relative difference over the parameters, small tensors measured against 1e-3 of the whole gradient's norm"""
    total = float(torch.sqrt(sum((v.double() ** 2).sum() for v in ref.values())))
    return max((float((got[k].cpu().double() - ref[k].cpu().double()).norm()) / max(float(ref[k].double().norm()), 1e-3 * total), k) for k in ref)


# ---------------------------------------------------------------------------------------------------- TrainEngine groups=
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_grouped_step_is_the_weighted_sum_of_its_groups(bd, mode):
    from baddiffusion_amd.schedulers import DDPMScheduler
    from baddiffusion_amd.trainer import TrainEngine
    cfg = C.SMALL_CFGS["small"]
    m = make_model(bd[2], cfg, 7, mode)
    engine = TrainEngine(m, DDPMScheduler(), lr=1e-5, max_grad_norm=1.0, num_training_steps=None, loss_type="l2", use_graph=False)
    g = torch.Generator().manual_seed(5)
    xn = torch.randn(11, 16, 16, 3, generator=g).cuda()
    tg = torch.randn(11, 16, 16, 3, generator=g).cuda()
    t = torch.randint(1000, (11,), generator=g).cuda()
    flat0 = m.flat.detach().clone()
    w1, w2 = 0.5, 1.0
    loss = engine.forward_backward(xn, tg, t, groups=((3, w1), (8, w2))).clone()
    parts = engine.group_losses.clone()
    grouped = m.logical_grads(engine.grads.clone())
    l1 = engine.forward_backward(xn[:3].contiguous(), tg[:3].contiguous(), t[:3].contiguous()).clone()
    g1 = m.logical_grads(engine.grads.clone())
    l2 = engine.forward_backward(xn[3:].contiguous(), tg[3:].contiguous(), t[3:].contiguous()).clone()
    g2 = m.logical_grads(engine.grads.clone())
    assert torch.equal(m.flat.detach(), flat0)                        # no optimizer step in between
    ref = {k: w1 * g1[k].double() + w2 * g2[k].double() for k in g1}
    worst = worst_rel(grouped, ref)
    print(f"MEASURE grouped_step {mode} loss {float(loss):.9g} parts {parts.tolist()} alone {float(l1):.9g} {float(l2):.9g} "
          f"gradient worst norm-relative {worst[0]:.3e} at {worst[1]}")
    assert parts.shape == (2,)
    np.testing.assert_allclose(float(loss), w1 * float(l1) + w2 * float(l2), rtol=1e-6)
    np.testing.assert_allclose(parts.tolist(), [float(l1), float(l2)], rtol=1e-6)
    assert worst[0] < 1e-3, worst
    with pytest.raises(ValueError):
        engine.forward_backward(xn, tg, t, groups=((3, w1), (7, w2)))


# ---------------------------------------------------------------------------------------------------- remove_backdoor clean=
def oracle_clean_removal(cfg, P0, tau, noises, draws, clean, T, lr, max_norm, weight, clean_target):
    """remove_backdoor's loop with the clean-data term on the CPU oracle: autograd through U.unet_forward, clip_grad_norm_, torch.optim.Adam"""
    _, alphas, alphas_cumprod = sched_ref.make_tables()
    P = {k: v.clone().requires_grad_(True) for k, v in P0.items()}
    opt = torch.optim.Adam(list(P.values()), lr=lr)
    hist, grads0 = [], None
    for eps, (rows, t_c, noise_c) in zip(noises, draws):
        b, cb = eps.shape[0], rows.numel()
        tT = torch.full((b,), T, dtype=torch.int64)
        x0 = B.normalize(clean[rows].permute(0, 3, 1, 2).float() / 255.0)
        x_t, _ = loss_ref.q_sample(alphas, alphas_cumprod, x0, torch.zeros_like(x0), t_c, noise_c)
        with torch.no_grad():
            tgt = U.unet_forward(cfg, P0, eps, tT)
            tgt_c = U.unet_forward(cfg, P0, x_t, t_c) if clean_target == "frozen" else noise_c
        pred = U.unet_forward(cfg, P, torch.cat((x_t, eps + tau, eps)), torch.cat((t_c, tT, tT)))
        loss_clean = ((pred[:cb] - tgt_c) ** 2).mean()
        loss_shift = ((pred[cb:] - torch.cat((tgt, tgt))) ** 2).mean()
        loss = weight * loss_clean + loss_shift
        opt.zero_grad()
        loss.backward()
        if grads0 is None:
            grads0 = {k: v.grad.detach().clone() for k, v in P.items()}
        norm = float(torch.nn.utils.clip_grad_norm_(list(P.values()), max_norm))
        opt.step()
        hist.append({"loss": float(loss.detach()), "grad_norm": norm, "loss_clean": float(loss_clean.detach()), "loss_shift": float(loss_shift.detach()),
                     "clean_target_meansq": float((tgt_c ** 2).mean())})
    return hist, grads0


@pytest.fixture(scope="module")
def clean_case():
    cfg = C.SMALL_CFGS["small"]
    P0 = U.gen_params(cfg, 7)
    tau = 0.5 * torch.randn(3, 16, 16, generator=torch.Generator().manual_seed(12))
    g = torch.Generator().manual_seed(11)
    noises = [torch.randn(4, 3, 16, 16, generator=g) for _ in range(4)]
    return cfg, P0, tau, noises, fixed_draws(4, 3), clean_u8(), {}


def oracle_for(case, clean_target):
    """the oracle run of one clean_target, computed once and shared by the compute modes"""
    cfg, P0, tau, noises, draws, clean, cache = case
    if clean_target not in cache:
        cache[clean_target] = oracle_clean_removal(cfg, P0, tau, noises, draws, clean, 999, 1e-5, 1.0, CLEAN_WEIGHT, clean_target)
    return cache[clean_target]


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("clean_target", ["frozen", "noise"])
def test_remove_backdoor_clean_term_vs_oracle(bd, clean_case, clean_target, mode):
    from baddiffusion_amd import defense
    from baddiffusion_amd.schedulers import DDPMScheduler
    from baddiffusion_amd.trainer import TrainEngine
    cfg, P0, tau, noises, draws, clean, _ = clean_case
    ref_hist, ref_grads = oracle_for(clean_case, clean_target)
    m = make_model(bd[2], cfg, 7, mode)
    sched = DDPMScheduler()
    engine = TrainEngine(m, sched, lr=1e-5, max_grad_norm=1.0, num_training_steps=None, loss_type="l2", use_graph=False)
    step, grads, calls = engine.step_from_noisy, [], []

    def spy(xn, tg, t, groups=None):
        calls.append((tuple(xn.shape), tuple(tg.shape), t.tolist(), groups))
        loss = step(xn, tg, t, groups=groups)
        grads.append(engine.grads.clone())
        return loss
    engine.step_from_noisy = spy
    frozen = defense.frozen_copy(m)
    dev_draws = [tuple(x.cuda() for x in d) for d in draws]
    hist = defense.remove_backdoor(m, sched, tau.cuda(), steps=4, batch=4, lr=1e-5, noises=[n.cuda() for n in noises], engine=engine,
                                   clean=clean.cuda(), clean_batch=3, clean_weight=CLEAN_WEIGHT, clean_target=clean_target,
                                   clean_draws=dev_draws, frozen=frozen)
    for k in sorted(HIST_KEYS):
        print(f"MEASURE remove_backdoor_clean {clean_target} {mode} {k} {[h[k] for h in hist]} ref {[h[k] for h in ref_hist]}")
    assert len(hist) == 4 and all(set(h) == HIST_KEYS and all(isinstance(v, float) for v in h.values()) for h in hist)
    assert len(calls) == 4                                           # ONE engine step per removal step
    for (xs, ts, tl, groups), d in zip(calls, draws):
        assert xs == (11, 16, 16, 3) and ts == xs and tl == d[1].tolist() + [999] * 8
        assert tuple(groups) == ((3, CLEAN_WEIGHT), (8, 1.0))
    got = m.logical_grads(grads[0])
    worst = worst_rel(got, ref_grads)
    print(f"MEASURE remove_backdoor_clean {clean_target} {mode} step-0 gradient worst norm-relative {worst[0]:.3e} at {worst[1]}")
    for h in hist:
        np.testing.assert_allclose(h["loss"], CLEAN_WEIGHT * h["loss_clean"] + h["loss_shift"], rtol=1e-6)
    for k in sorted(HIST_KEYS):
        first = 1 if (k, clean_target) == ("loss_clean", "frozen") else 0          # (exact value 0 at step 0: see the module docstring)
        np.testing.assert_allclose([h[k] for h in hist][first:], [h[k] for h in ref_hist][first:], rtol=1e-3, err_msg=k)
    if clean_target == "frozen":
        floor = (2e-3) ** 2 * ref_hist[0]["clean_target_meansq"]
        print(f"MEASURE remove_backdoor_clean frozen {mode} step-0 loss_clean {hist[0]['loss_clean']:.3e} oracle {ref_hist[0]['loss_clean']:.3e} bound {floor:.3e}")
        assert 0 <= hist[0]["loss_clean"] <= floor and 0 <= ref_hist[0]["loss_clean"] <= floor
    assert worst[0] < 1e-3, worst
    frozen_sd, sd = frozen.state_dict(), m.state_dict()
    assert all(torch.equal(frozen_sd[k].cpu(), P0[k]) for k in P0)                        # the caller's frozen copy: kept, never updated
    assert any(not torch.equal(sd[k].cpu(), P0[k]) for k in P0)                            # repaired in place


def test_remove_backdoor_clean_term_draws_from_the_generator_repeatably(bd):
    """no noises, no clean_draws: eps, rows, t_c, noise_c come from the seeded device generator; two runs agree bit for bit"""
    from baddiffusion_amd import defense
    from baddiffusion_amd.schedulers import DDPMScheduler
    cfg = C.SMALL_CFGS["small"]
    clean = clean_u8().cuda()
    tau = (0.5 * torch.randn(3, 16, 16, generator=torch.Generator().manual_seed(12))).cuda()
    runs = []
    for _ in range(2):
        m = make_model(bd[2], cfg, 7, "bf16x3")
        hist = defense.remove_backdoor(m, DDPMScheduler(), tau, steps=2, batch=4, lr=1e-5, generator=torch.Generator(device="cuda").manual_seed(3),
                                       clean=clean, clean_batch=3, clean_weight=CLEAN_WEIGHT)
        assert len(hist) == 2 and all(set(h) == HIST_KEYS and all(math.isfinite(v) for v in h.values()) for h in hist)
        assert all(h["loss_shift"] > 0 and h["grad_norm"] > 0 for h in hist)
        runs.append((hist, m.flat.detach().clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    # the documented draw order: eps first, then rows, t_c, noise_c -- the same run with the draws made here
    g = torch.Generator(device="cuda").manual_seed(3)
    noises, draws = [], []
    for _ in range(2):
        noises.append(torch.randn(4, 3, 16, 16, generator=g, device="cuda"))
        draws.append((torch.randint(8, (3,), generator=g, device="cuda"), torch.randint(1000, (3,), generator=g, device="cuda"),
                      torch.randn(3, 3, 16, 16, generator=g, device="cuda")))
    m = make_model(bd[2], cfg, 7, "bf16x3")
    hist = defense.remove_backdoor(m, DDPMScheduler(), tau, steps=2, batch=4, lr=1e-5, noises=noises, clean=clean, clean_weight=CLEAN_WEIGHT,
                                   clean_draws=draws)
    assert hist == runs[0][0] and torch.equal(m.flat.detach(), runs[0][1])


# ---------------------------------------------------------------------------------------------------- synthesize_clean
def test_synthesize_clean_is_the_pipelines_own_u8_output(bd):
    from baddiffusion_amd.defense import synthesize_clean
    from baddiffusion_amd.pipelines import DDIMPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    cfg = C.SMALL_CFGS["small"]
    pipe = DDIMPipeline(unet=make_model(bd[2], cfg, 7, "bf16x3"), scheduler=DDPMScheduler())
    init = torch.randn(8, 3, 16, 16, generator=torch.Generator().manual_seed(21)).cuda()
    own = pipe(batch_size=8, init=init, output_type="u8", num_inference_steps=3).images
    got = synthesize_clean(pipe, 8, init=init, num_inference_steps=3)
    assert got.dtype == torch.uint8 and got.shape == (8, 16, 16, 3) and got.is_cuda
    assert torch.equal(got, own)
    chunked = synthesize_clean(pipe, 8, init=init, max_batch_n=3, num_inference_steps=3)          # chunks of 3, 3, 2
    own_chunks = torch.cat([pipe(batch_size=c.shape[0], init=c, output_type="u8", num_inference_steps=3).images for c in torch.split(init, 3)])
    assert torch.equal(chunked, own_chunks)
    drawn = synthesize_clean(pipe, 8, generator=torch.Generator(device="cuda").manual_seed(4), num_inference_steps=3)
    noise = torch.randn(8, 3, 16, 16, generator=torch.Generator(device="cuda").manual_seed(4), device="cuda")
    assert torch.equal(drawn, synthesize_clean(pipe, 8, init=noise, num_inference_steps=3))
    print(f"MEASURE synthesize_clean mean level {float(got.float().mean()):.4g} differing from the chunked run {int((got != chunked).sum())} of {got.numel()}")


# ---------------------------------------------------------------------------------------------------- prediction_drift
def test_prediction_drift(bd):
    from baddiffusion_amd import defense, metrics
    from baddiffusion_amd.schedulers import DDPMScheduler
    ops = bd[1]
    cfg = C.SMALL_CFGS["small"]
    sched = DDPMScheduler()
    clean = clean_u8().cuda()
    m = make_model(bd[2], cfg, 7, "bf16x3")
    frozen = defense.frozen_copy(m)
    draws = tuple(x.cuda() for x in fixed_draws(1, 8, seed=23)[0])
    assert defense.prediction_drift(m, frozen, clean, sched, n=8, draws=draws) == 0.0
    assert defense.prediction_drift(m, frozen, clean, sched, n=8, generator=torch.Generator(device="cuda").manual_seed(1), max_batch_n=3) == 0.0
    tau = (0.5 * torch.randn(3, 16, 16, generator=torch.Generator().manual_seed(12))).cuda()
    defense.remove_backdoor(m, sched, tau, steps=2, batch=4, lr=1e-5, generator=torch.Generator(device="cuda").manual_seed(3), clean=clean,
                            clean_batch=3, clean_weight=CLEAN_WEIGHT, frozen=frozen)
    drift = defense.prediction_drift(m, frozen, clean, sched, n=8, draws=draws)
    rows, t_c, noise_c = draws
    alphas, alphas_cumprod = sched.device_tables(clean.device)
    zeros = torch.zeros(3, 16, 16, device="cuda")
    x_t, _ = ops.poison_qsample(clean, torch.zeros(8, dtype=torch.uint8, device="cuda"), zeros, zeros, noise_c, t_c, alphas, alphas_cumprod, row_index=rows)
    with torch.no_grad():
        a = m(x_t.permute(0, 3, 1, 2), t_c).sample
        b = frozen(x_t.permute(0, 3, 1, 2), t_c).sample
    ref = metrics.mse(a, b)
    print(f"MEASURE prediction_drift after 2 removal steps {drift:.9g} metrics.mse on the same rows {ref:.9g}")
    assert isinstance(drift, float) and math.isfinite(drift) and drift > 0
    np.testing.assert_allclose(drift, ref, rtol=1e-6)
    gen = [defense.prediction_drift(m, frozen, clean, sched, n=8, generator=torch.Generator(device="cuda").manual_seed(1)) for _ in range(2)]
    assert gen[0] == gen[1] and gen[0] > 0


# ---------------------------------------------------------------------------------------------------- command line
def test_elijah_defense_clean_source(bd, tmp_path):
    import elijah_defense as E
    from baddiffusion_amd import defense
    from baddiffusion_amd.model import DiffuserModelSched, save_scheduler, save_unet
    from baddiffusion_amd.schedulers import DDPMScheduler
    cfg = C.SMALL_CFGS["small"]
    ckpt = str(tmp_path / "ckpt_small")
    m = make_model(bd[2], cfg, 7, "bf16x3")
    save_unet(m, os.path.join(ckpt, "unet"))
    save_scheduler(DDPMScheduler(), os.path.join(ckpt, "scheduler"))
    before = {k: v.cpu().clone() for k, v in m.state_dict().items()}
    common = ["--ckpt", ckpt, "--inv_steps", "3", "--inv_batch", "4", "--detect_n", "8", "--sched", "DDIM-SCHED", "--infer_steps", "3",
              "--remove_steps", "2", "--batch", "4"]
    name = "res_elijah_inv3_lam0.5_rm2_lr2e-05_ckpt_small"
    result = E.main(common + ["--output_dir", str(tmp_path / "clean"), "--clean_source", "synthetic", "--clean_n", "8", "--clean_batch", "3"])
    out = os.path.join(str(tmp_path / "clean"), name)
    score = json.load(open(os.path.join(out, "score.json")))
    assert score == json.loads(json.dumps(result))
    assert set(score) == {"before", "after", "detected", "removal", "drift"}
    assert len(score["removal"]) == 2 and all(set(h) == HIST_KEYS and all(math.isfinite(v) for v in h.values()) for h in score["removal"])
    assert isinstance(score["drift"], float) and math.isfinite(score["drift"]) and score["drift"] > 0
    config = json.load(open(os.path.join(out, "config.json")))
    assert (config["clean_source"], config["clean_n"], config["clean_batch"], config["clean_weight"], config["clean_target"]) == \
        ("synthetic", 8, 3, 1.0, "frozen")
    model, sched, _ = DiffuserModelSched.get_trained(out)
    after = model.state_dict()
    assert set(after) == set(before) and any(not torch.equal(after[k].cpu(), before[k]) for k in before)

    plain = E.main(common + ["--output_dir", str(tmp_path / "plain"), "--clean_source", "none"])
    out_plain = os.path.join(str(tmp_path / "plain"), name)
    score_plain = json.load(open(os.path.join(out_plain, "score.json")))
    assert score_plain == json.loads(json.dumps(plain))
    assert set(score_plain) == {"before", "after", "detected", "removal"}
    assert len(score_plain["removal"]) == 2 and all(set(h) == {"loss", "grad_norm"} for h in score_plain["removal"])
    assert score_plain["before"] == score["before"]

    # the drift of both repaired checkpoints on the clean images the first run made (same seeds), against the untouched checkpoint
    conf = E.Config(ckpt=ckpt, infer_steps=3, clean_source="synthetic", clean_n=8)
    original = make_model(bd[2], cfg, 7, "bf16x3")
    clean = E.clean_images(conf, original, sched, log=lambda *_: None)
    drifts = {}
    for tag, d in (("with the clean term", out), ("without", out_plain)):
        repaired = DiffuserModelSched.get_trained(d)[0].cuda().set_compute_mode("bf16x3")
        drifts[tag] = E.drift(conf, repaired, original, clean, sched, log=lambda *_: None)
    print(f"MEASURE elijah_defense clean_source drift in score.json {score['drift']:.6g}, recomputed {drifts} "
          f"(random weights, 2 steps: says nothing about a backdoored checkpoint)")
    assert all(math.isfinite(v) and v > 0 for v in drifts.values())
