"""GPU: the detection kernels (bd_pairwise_sqdist, bd_total_variation), the metrics and defense stages built on them
(backdoor_scores, detect_backdoor, remove_backdoor) and the elijah_defense.py command line.

Bounds.  Pairwise squared distances: integer-valued rows are exact in fp32 (9 D < 2^24), so the kernel must reproduce the int64
reference bit for bit; on real data every entry is within (D + 2) 2^-24 relative of fp64 on the same fp32 inputs -- one rounding for
the subtraction, one for the square, at most D - 1 for a sum of non-negative terms in any order.  Total variation: 1e-6 relative
against fp64, the bound metrics.mse states for fp32 differences accumulated in fp64.  remove_backdoor: 1e-3 on losses, gradient
norms and per-parameter gradients against the CPU oracle, the project's bar for whole-network gradients (test_hip_unet.py)."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_ref as U
from tests.golden import cases as C

U24 = 2.0 ** -24
# (64, 3072) and (8, 196608) split D over workgroups (12 and 768 splits on 256 CUs); (5, 3100) gets fewer splits (11) than the
# workspace bound allows for (12) and ends in a ragged chunk
SHAPES = [(1, 1), (2, 1), (67, 100), (130, 192), (64, 3072), (8, 196608), (5, 3100)]


@pytest.fixture(scope="module")
def bd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from baddiffusion_amd import _lib as L
    import baddiffusion_amd.ops as ops
    import baddiffusion_amd.unet as unet
    return L, ops, unet


def run_sqdist(L, x, ldd):
    """bd_pairwise_sqdist on the [N, D] view x into a NaN-filled [N, ldd] buffer with a NaN-filled workspace"""
    lib = L.load()
    N, D = x.shape
    d2 = torch.full((N, ldd), float("nan"), device="cuda")
    nbytes = lib.bd_pairwise_sqdist_workspace_bytes(N, D)
    ws = torch.full((max(nbytes // 4, 1),), float("nan"), device="cuda")
    L.check(lib.bd_pairwise_sqdist(x.data_ptr(), x.stride(0) if N > 1 else D, N, D, d2.data_ptr(), ldd, ws.data_ptr() if nbytes else None,
                                   nbytes, L.stream()), "bd_pairwise_sqdist")
    return d2, nbytes


def layouts(x):
    """(name, view of the same values, ldd): contiguous and 16-byte aligned | row stride D + 3 starting one float in (4-byte aligned only)"""
    N, D = x.shape
    big = torch.zeros(N, D + 3, device="cuda")
    big[:, 1:1 + D] = x
    v = big[:, 1:1 + D]
    assert v.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
    return [("aligned", x, N), ("offset", v, N + 5)]


def check_structure(d2, N, ldd):
    blk = d2[:, :N]
    assert bool((blk.diagonal() == 0).all()) and not bool(torch.signbit(blk.diagonal()).any())
    assert torch.equal(blk, blk.t())
    assert bool(torch.isnan(d2[:, N:]).all())
    return blk


# ---------------------------------------------------------------------------------------------------- pairwise: exact values
@pytest.mark.parametrize("pattern", ["random", "first", "last"])
@pytest.mark.parametrize("N,D", SHAPES)
def test_pairwise_sqdist_exact_on_integers(bd, N, D, pattern):
    L = bd[0]
    xi = torch.randint(0, 4, (N, D), generator=torch.Generator().manual_seed(N * 7 + D))
    if pattern != "random":          # all zero but one column: a dropped first or tail chunk gives zeros
        keep = xi[:, 0 if pattern == "first" else D - 1].clone()
        xi.zero_()
        xi[:, 0 if pattern == "first" else D - 1] = keep
    xg = xi.cuda()
    ref = torch.stack([((xg[i:i + 1] - xg) ** 2).sum(1) for i in range(N)]).cpu()            # int64
    assert int(ref.max()) < 2 ** 24
    for name, x, ldd in layouts(xg.float()):
        d2, nbytes = run_sqdist(L, x, ldd)
        blk = check_structure(d2, N, ldd)
        assert torch.equal(blk.cpu(), ref.float()), (name, int((blk.cpu() != ref.float()).sum()))
        again, _ = run_sqdist(L, x, ldd)
        assert torch.equal(again[:, :N], blk)
        print(f"MEASURE pairwise_exact {(N, D)} {pattern} {name} workspace {nbytes} max {int(ref.max())}")
    if (N, D) == (8, 196608):
        assert nbytes > 0                                      # the split-D path


# ---------------------------------------------------------------------------------------------------- pairwise: close pairs
def close_rows(N, D, seed):
    """uniform [0, 1] rows with a duplicate (0, 1), a pair 1e-4 apart (2, 3) and four rows within 1e-3 of a constant (4 .. 7)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, D, generator=g)
    if N >= 2:
        x[1] = x[0]
    if N >= 4:
        x[3] = x[2] + 1e-4
    if N >= 8:
        x[4:8] = 0.5 + 1e-3 * torch.rand(4, D, generator=g)
    return x


def sqdist_fp64(x):
    xd = x.double()
    return torch.stack([((xd[i:i + 1] - xd) ** 2).sum(1) for i in range(xd.shape[0])])


@pytest.mark.parametrize("N,D", SHAPES)
def test_pairwise_sqdist_close_pairs(bd, N, D):
    L = bd[0]
    xg = close_rows(N, D, 100 + N).cuda()
    ref = sqdist_fp64(xg).cpu()
    bound = (D + 2) * U24
    for name, x, ldd in layouts(xg):
        d2, _ = run_sqdist(L, x, ldd)
        blk = check_structure(d2, N, ldd).cpu().double()
        nz = ref != 0
        assert bool((blk[~nz] == 0).all())                                  # the diagonal and the duplicate pair: exactly 0
        rel = ((blk - ref).abs() / ref.masked_fill(~nz, 1.0))[nz]
        worst = float(rel.max()) if rel.numel() else 0.0
        near = float(abs(blk[2, 3] - ref[2, 3]) / ref[2, 3]) if N >= 4 else 0.0
        print(f"MEASURE pairwise_close {(N, D)} {name} worst rel {worst:.3e} near-duplicate rel {near:.3e} bound {bound:.3e}")
        assert worst <= bound, (name, worst, bound)
        if N >= 2:
            assert float(blk[0, 1]) == 0.0 and float(blk[1, 0]) == 0.0
        if N >= 4:
            assert float(ref[2, 3]) > 0 and near <= bound, (name, near, bound)


# ---------------------------------------------------------------------------------------------------- total variation
def tv_fp64(x):
    xd = x.double()
    return (xd[:, :, 1:] - xd[:, :, :-1]).abs().sum(dim=(1, 2, 3)) + (xd[:, :, :, 1:] - xd[:, :, :, :-1]).abs().sum(dim=(1, 2, 3))


@pytest.mark.parametrize("N,C_,H,W", [(5, 3, 9, 7), (1, 1, 1, 1), (2, 3, 1, 8), (2, 3, 8, 1), (2, 3, 32, 32), (1, 3, 256, 256)])
def test_total_variation(bd, N, C_, H, W):
    ops = bd[1]
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + W)
    for kind in ("real", "integer"):
        x = (torch.rand(N, C_, H, W, generator=g) if kind == "real" else torch.randint(0, 4, (N, C_, H, W), generator=g).float()).cuda()
        ref = tv_fp64(x).cpu()
        tv = ops.total_variation(x)
        tv_cl = ops.total_variation(x.contiguous(memory_format=torch.channels_last))
        tv_nhwc = ops.total_variation(x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
        assert tv.shape == (N,) and tv.dtype == torch.float32
        assert torch.equal(tv, tv_cl) and torch.equal(tv, tv_nhwc)
        err = float(((tv.cpu().double() - ref).abs() / ref.clamp_min(1e-300)).max()) if float(ref.max()) > 0 else float(tv.abs().max())
        print(f"MEASURE total_variation {(N, C_, H, W)} {kind} rel {err:.3e}")
        if kind == "integer":
            assert torch.equal(tv.cpu().double(), ref)
        else:
            assert err <= 1e-6, err
        if H == 1 and W == 1:
            assert bool((tv == 0).all())


# ---------------------------------------------------------------------------------------------------- metrics
def uniformity_fp64(images):
    d2 = sqdist_fp64(images.reshape(images.shape[0], -1))
    i, j = torch.triu_indices(images.shape[0], images.shape[0], offset=1)
    return float(d2[i, j].sqrt().mean())


def tv_score_fp64(images):
    return float(tv_fp64(images).mean() / images[0].numel())


def test_metrics_uniformity_and_total_variation(bd):
    from baddiffusion_amd import metrics
    x = torch.rand(19, 3, 16, 16, generator=torch.Generator().manual_seed(5)).cuda()
    D = 3 * 16 * 16
    d2 = metrics.pairwise_sqdist(x)
    assert d2.shape == (19, 19) and d2.is_cuda
    for name, v in (("nchw", x), ("channels_last", x.contiguous(memory_format=torch.channels_last)), ("strided", torch.stack((x, x), -1)[..., 0])):
        u, t = metrics.uniformity(v), metrics.total_variation(v)
        ur, tr = uniformity_fp64(x.cpu()), tv_score_fp64(x.cpu())
        print(f"MEASURE metrics {name} uniformity rel {abs(u - ur) / ur:.3e} (bound {(D + 2) * U24:.3e}) total_variation rel {abs(t - tr) / tr:.3e}")
        assert isinstance(u, float) and isinstance(t, float)
        assert abs(u - ur) <= (D + 2) * U24 * ur
        assert abs(t - tr) <= 1e-6 * tr


# ---------------------------------------------------------------------------------------------------- backdoor_scores
class StubPipeline:
    """uint8 NHWC images on the device: the fixed target +- 1 level for an init whose batch mean is far from 0, uniform noise otherwise"""

    def __init__(self):
        self.g = torch.Generator(device="cuda").manual_seed(9)
        self.target = torch.randint(1, 255, (1, 16, 16, 3), generator=self.g, device="cuda", dtype=torch.uint8)
        self.calls = []

    def __call__(self, batch_size, init, output_type, **kw):
        assert output_type == "u8" and init.shape[0] == batch_size and kw == {"num_inference_steps": 3}
        if abs(float(init.mean())) > 1.0:
            img = (self.target.int() + torch.randint(-1, 2, (batch_size, 16, 16, 3), generator=self.g, device="cuda")).to(torch.uint8)
        else:
            img = torch.randint(0, 256, (batch_size, 16, 16, 3), generator=self.g, device="cuda", dtype=torch.uint8)
        self.calls.append((batch_size, img))
        return (img,)


def check_scores(scores, clean_u8, trig_u8, D):
    ref = {}
    for tag, u8 in (("clean", clean_u8), ("trigger", trig_u8)):
        img = (u8.float() / 255).permute(0, 3, 1, 2).cpu()
        ref[f"uniformity_{tag}"] = uniformity_fp64(img)
        ref[f"tv_{tag}"] = tv_score_fp64(img)
    for k, r in ref.items():
        tol = (D + 2) * U24 if k.startswith("uniformity") else 1e-6
        print(f"MEASURE backdoor_scores {k} {scores[k]:.9g} fp64 {r:.9g} rel {abs(scores[k] - r) / r:.3e} (bound {tol:.3e})")
        assert math.isfinite(scores[k]) and abs(scores[k] - r) <= tol * r, (k, scores[k], r)
    assert scores["uniformity_ratio"] == scores["uniformity_trigger"] / scores["uniformity_clean"]
    assert set(scores) == set(ref) | {"uniformity_ratio"}


def test_backdoor_scores_with_stub_pipeline(bd):
    from baddiffusion_amd.defense import backdoor_scores, detect_backdoor
    tau = torch.full((3, 16, 16), 4.0, device="cuda")
    pipe = StubPipeline()
    scores = backdoor_scores(pipe, tau, n=64, generator=torch.Generator(device="cuda").manual_seed(1), max_batch_n=24, num_inference_steps=3)
    assert [b for b, _ in pipe.calls] == [24, 24, 16] * 2
    imgs = [im for _, im in pipe.calls]
    check_scores(scores, torch.cat(imgs[:3]), torch.cat(imgs[3:]), 768)
    assert scores["uniformity_ratio"] < 0.05
    assert detect_backdoor(scores, max_ratio=0.5) is True
    pipe = StubPipeline()
    init = torch.randn(64, 3, 16, 16, generator=torch.Generator().manual_seed(2))          # a CPU `init` is moved to tau's device
    clean = backdoor_scores(pipe, torch.zeros(3, 16, 16, device="cuda"), n=64, init=init, max_batch_n=24, num_inference_steps=3)
    print(f"MEASURE backdoor_scores stub ratio triggered {scores['uniformity_ratio']:.4g} tau=0 {clean['uniformity_ratio']:.4g}")
    assert detect_backdoor(clean, max_ratio=0.5) is False


def make_model(unet, cfg, seed, mode):
    m = unet.unet_from_config(cfg).cuda()
    m.load_state_dict(U.gen_params(cfg, seed))
    return m.set_compute_mode(mode)


def test_backdoor_scores_with_real_pipeline(bd):
    from baddiffusion_amd.defense import backdoor_scores
    from baddiffusion_amd.pipelines import DDIMPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    cfg = C.SMALL_CFGS["small"]
    pipe = DDIMPipeline(unet=make_model(bd[2], cfg, 7, "bf16x3"), scheduler=DDPMScheduler())
    noise = torch.randn(8, 3, 16, 16, generator=torch.Generator().manual_seed(21)).cuda()
    tau = (0.5 * torch.randn(3, 16, 16, generator=torch.Generator().manual_seed(12))).cuda()
    scores = backdoor_scores(pipe, tau, n=8, init=noise, num_inference_steps=3)
    clean = pipe(batch_size=8, init=noise, output_type="u8", num_inference_steps=3).images
    trig = pipe(batch_size=8, init=noise + tau, output_type="u8", num_inference_steps=3).images
    assert clean.dtype == torch.uint8 and clean.shape == (8, 16, 16, 3)
    check_scores(scores, clean, trig, 768)
    assert all(math.isfinite(v) for v in scores.values())


# ---------------------------------------------------------------------------------------------------- remove_backdoor
def oracle_removal(cfg, P0, tau, noises, T, lr, max_norm):
    """the loop of remove_backdoor on the CPU oracle: autograd through U.unet_forward, clip_grad_norm_, torch.optim.Adam"""
    P = {k: v.clone().requires_grad_(True) for k, v in P0.items()}
    opt = torch.optim.Adam(list(P.values()), lr=lr)
    losses, norms, grads0 = [], [], None
    for eps in noises:
        t = torch.full((2 * eps.shape[0],), T, dtype=torch.int64)
        with torch.no_grad():
            tgt = U.unet_forward(cfg, P0, eps, t[: eps.shape[0]])
        pred = U.unet_forward(cfg, P, torch.cat((eps + tau, eps)), t)
        loss = ((pred - torch.cat((tgt, tgt))) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        if grads0 is None:
            grads0 = {k: v.grad.detach().clone() for k, v in P.items()}
        norms.append(float(torch.nn.utils.clip_grad_norm_(list(P.values()), max_norm)))
        opt.step()
        losses.append(float(loss.detach()))
    return losses, norms, grads0


@pytest.fixture(scope="module")
def removal_case():
    cfg = C.SMALL_CFGS["small"]
    P0 = U.gen_params(cfg, 7)
    tau = 0.5 * torch.randn(3, 16, 16, generator=torch.Generator().manual_seed(12))
    g = torch.Generator().manual_seed(11)
    noises = [torch.randn(4, 3, 16, 16, generator=g) for _ in range(4)]
    return cfg, P0, tau, noises, oracle_removal(cfg, P0, tau, noises, 999, 1e-5, 1.0)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_remove_backdoor_vs_oracle(bd, removal_case, monkeypatch, mode):
    from baddiffusion_amd import defense
    from baddiffusion_amd.schedulers import DDPMScheduler
    from baddiffusion_amd.trainer import TrainEngine
    cfg, P0, tau, noises, (ref_losses, ref_norms, ref_grads) = removal_case
    m = make_model(bd[2], cfg, 7, mode)
    flags = [p.requires_grad for p in m.parameters()]
    sched = DDPMScheduler()
    engine = TrainEngine(m, sched, lr=1e-5, max_grad_norm=1.0, num_training_steps=None, loss_type="l2", use_graph=False)
    step, grads = engine.step_from_noisy, []

    def spy(xn, tg, t):
        assert xn.shape == (8, 16, 16, 3) and tg.shape == xn.shape and t.tolist() == [999] * 8
        loss = step(xn, tg, t)
        grads.append(engine.grads.clone())
        return loss
    engine.step_from_noisy = spy
    copies, make_copy = [], defense.frozen_copy
    monkeypatch.setattr(defense, "frozen_copy", lambda model: copies.append(make_copy(model)) or copies[-1])
    hist = defense.remove_backdoor(m, sched, tau.cuda(), steps=4, batch=4, lr=1e-5, noises=[n.cuda() for n in noises], engine=engine)
    losses, norms = [h["loss"] for h in hist], [h["grad_norm"] for h in hist]
    print(f"MEASURE remove_backdoor {mode} losses {losses} ref {ref_losses} grad norms {norms} ref {ref_norms}")
    assert len(hist) == 4 and all(set(h) == {"loss", "grad_norm"} and isinstance(h["loss"], float) for h in hist)
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-3)
    np.testing.assert_allclose(norms, ref_norms, rtol=1e-3)
    got = m.logical_grads(grads[0])
    total = float(torch.sqrt(sum((v.double() ** 2).sum() for v in ref_grads.values())))
    worst = max((float((got[k].cpu().double() - ref_grads[k].double()).norm()) / max(float(ref_grads[k].double().norm()), 1e-3 * total), k)
                for k in ref_grads)
    print(f"MEASURE remove_backdoor {mode} step-0 gradient worst norm-relative {worst[0]:.3e} at {worst[1]}")
    assert worst[0] < 1e-3, worst
    assert len(copies) == 1 and copies[0].compute_mode == mode and copies[0] is not m
    frozen_sd, sd = copies[0].state_dict(), m.state_dict()
    assert all(torch.equal(frozen_sd[k].cpu(), P0[k]) for k in P0)                        # never updated
    assert any(not torch.equal(sd[k].cpu(), P0[k]) for k in P0)                            # repaired in place
    assert [p.requires_grad for p in m.parameters()] == flags
    assert not any(p.requires_grad for p in copies[0].parameters())


def test_remove_backdoor_builds_its_own_engine_and_draws_noise(bd):
    """no engine, no noises: Adam(lr) / clip 1.0 / constant LR built inside, eps drawn from the generator, T = the last timestep"""
    from baddiffusion_amd import defense
    from baddiffusion_amd.schedulers import DDPMScheduler
    cfg = C.SMALL_CFGS["small"]
    runs = []
    for _ in range(2):
        m = make_model(bd[2], cfg, 7, "bf16x3")
        tau = (0.5 * torch.randn(3, 16, 16, generator=torch.Generator().manual_seed(12))).cuda()
        hist = defense.remove_backdoor(m, DDPMScheduler(), tau, steps=2, batch=4, lr=1e-5, generator=torch.Generator(device="cuda").manual_seed(3))
        assert len(hist) == 2 and all(math.isfinite(h["loss"]) and h["loss"] > 0 and h["grad_norm"] > 0 for h in hist)
        runs.append((hist, m.flat.detach().clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


# ---------------------------------------------------------------------------------------------------- command line
def test_elijah_defense_end_to_end(bd, tmp_path):
    import elijah_defense as E
    from baddiffusion_amd.model import DiffuserModelSched, save_scheduler, save_unet
    from baddiffusion_amd.schedulers import DDPMScheduler
    cfg = C.SMALL_CFGS["small"]
    ckpt = str(tmp_path / "ckpt_small")
    m = make_model(bd[2], cfg, 7, "bf16x3")
    save_unet(m, os.path.join(ckpt, "unet"))
    save_scheduler(DDPMScheduler(), os.path.join(ckpt, "scheduler"))
    before = {k: v.cpu().clone() for k, v in m.state_dict().items()}
    result = E.main(["--ckpt", ckpt, "--output_dir", str(tmp_path / "out"), "--inv_steps", "3", "--inv_batch", "4", "--detect_n", "8",
                     "--sched", "DDIM-SCHED", "--infer_steps", "3", "--remove_steps", "2", "--batch", "4"])
    out = os.path.join(str(tmp_path / "out"), "res_elijah_inv3_lam0.5_rm2_lr2e-05_ckpt_small")
    score = json.load(open(os.path.join(out, "score.json")))
    assert score == json.loads(json.dumps(result))
    for tag in ("before", "after"):
        assert set(score[tag]) == {"uniformity_clean", "uniformity_trigger", "tv_clean", "tv_trigger", "uniformity_ratio"}
        assert all(isinstance(v, float) and math.isfinite(v) for v in score[tag].values()), score[tag]
    assert len(score["removal"]) == 2 and all(math.isfinite(h["loss"]) and math.isfinite(h["grad_norm"]) for h in score["removal"])
    assert score["detected"] is None                                                 # no --max_ratio, no verdict
    assert os.path.exists(os.path.join(out, "config.json"))
    tau = torch.load(os.path.join(out, "tau.pt"))
    assert tuple(tau.shape) == (3, 16, 16) and bool(torch.isfinite(tau).all())
    model, sched, _ = DiffuserModelSched.get_trained(out)
    after = model.state_dict()
    assert set(after) == set(before) and any(not torch.equal(after[k].cpu(), before[k]) for k in before)
    assert sched.config.num_train_timesteps == 1000
    print(f"MEASURE elijah_defense before {score['before']} after {score['after']} removal {score['removal']}")
