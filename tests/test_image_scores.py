"""GPU: the per-image kernels bd_image_loss / bd_ssim_images and what is built on them -- metrics.mse_per_image / ssim_per_image /
attack_success_rate, backdoor_scores(target=), elijah_defense.py --target, measure() with --asr_threshold, TrainEngine(track_split=).

Bounds.  Inputs k / 256 with integer |k| <= 512: every fp32 difference, square and absolute value is exact and every fp64 sum is exact
in any order, so out[n] must equal np.float32(sum64 / (C H W)) bit for bit.  Random data: 1e-6 relative per image against fp64 (the bound
the existing MSE test holds metrics.mse to: fp32 differences, fp64 sums) and 2e-5 absolute on SSIM (the tolerance the existing SSIM test
derives for the fp32 local moments against c2 = 9e-4).  The independence properties of include/bd_hip.h are checked bit for bit."""
import dataclasses
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import metrics_ref
from oracle import unet_ref as U
from tests.golden import cases as C

RANDOM_SHAPES = [(8, 3, 32, 32), (2, 3, 75, 44), (3, 1, 12, 64), (2, 3, 256, 256)]
SSIM_SHAPES = [(4, 3, 11, 11), (8, 3, 32, 32), (2, 3, 33, 33)] + RANDOM_SHAPES[1:]          # a 1 x 1 map, one tile, a ragged second tile, ...
OLD_SCORE_KEYS = {"uniformity_clean", "uniformity_trigger", "tv_clean", "tv_trigger", "uniformity_ratio"}
TARGET_KEYS = {"mse_target_clean", "mse_target_trigger", "ssim_target_clean", "ssim_target_trigger"}
ASR_KEYS = {"asr_clean", "asr_trigger"}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def pairs():
    """(a, b) CPU batches per shape, b = a + noise clamped to [0, 1], drawn once and never modified"""
    g = torch.Generator().manual_seed(11)
    out = {}
    for shape in sorted(set(RANDOM_SHAPES + SSIM_SHAPES)):
        a = torch.rand(shape, generator=g)
        out[shape] = (a, (a + 0.2 * torch.randn(shape, generator=g)).clamp(0, 1))
    return out


def nhwc(x):
    """the same [N,C,H,W] values in NHWC storage"""
    return x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def bits(x):
    return x.cpu().numpy().view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------- exact values
def elem64(d, loss_type):
    d = d.astype(np.float64)
    if loss_type == "l2":
        return d * d
    if loss_type == "l1":
        return np.abs(d)
    return np.where(np.abs(d) < 1.0, 0.5 * d * d, np.abs(d) - 0.5)


@pytest.mark.parametrize("loss_type", ["l2", "l1", "huber"])
@pytest.mark.parametrize("shape", [(5, 3, 7, 9), (1, 1, 1, 1), (3, 3, 32, 32)])
def test_image_loss_exact_values(gpu, shape, loss_type):
    from baddiffusion_amd import ops
    rng = np.random.default_rng(sum(shape))
    kp, kt = rng.integers(-512, 513, shape), rng.integers(-512, 513, shape)
    if loss_type == "huber":         # |d| on both sides of 1, and exactly 1
        kp.flat[0], kt.flat[0] = 256, 0
        d = np.abs(kp - kt) / 256.0
        assert (d == 1).any() and (kp.size == 1 or ((d < 1).any() and (d > 1).any()))
    p, t = torch.from_numpy(kp / 256.0).float(), torch.from_numpy(kt / 256.0).float()
    n = shape[1] * shape[2] * shape[3]
    want = np.float32(elem64((kp - kt) / 256.0, loss_type).reshape(shape[0], -1).sum(1) / n)
    got = ops.image_loss(p.to(gpu), t.to(gpu), loss_type)
    assert got.dtype == torch.float32 and got.shape == (shape[0],) and got.is_cuda
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (got.cpu().numpy(), want)
    # one target for all images, by stride; and NHWC storage
    want0 = np.float32(elem64((kp - kt[:1]) / 256.0, loss_type).reshape(shape[0], -1).sum(1) / n)
    for tgt in (t[0].to(gpu), t[:1].to(gpu)):
        got0 = ops.image_loss(nhwc(p.to(gpu)), tgt, loss_type)
        assert np.array_equal(got0.cpu().numpy().view(np.uint32), want0.view(np.uint32))


# ---------------------------------------------------------------------------------------------------- against fp64
@pytest.mark.parametrize("shape", RANDOM_SHAPES)
def test_mse_per_image_against_fp64(gpu, pairs, shape):
    from baddiffusion_amd import metrics
    a, b = pairs[shape]
    got = metrics.mse_per_image(a.to(gpu), b.to(gpu))
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (shape[0],)
    want = np.array([metrics_ref.mse_ref(a[n].numpy(), b[n].numpy()) for n in range(shape[0])])
    rel = np.abs(got.cpu().numpy().astype(np.float64) - want) / want
    print(f"MEASURE mse_per_image {shape} worst rel {rel.max():.3e}")
    assert rel.max() <= 1e-6, rel
    mean, whole = float(got.double().mean()), metrics.mse(a.to(gpu), b.to(gpu))
    print(f"MEASURE mse_per_image {shape} mean {mean:.9g} metrics.mse {whole:.9g}")
    assert abs(mean - whole) <= 1e-6 * whole


@pytest.mark.parametrize("shape", SSIM_SHAPES)
def test_ssim_per_image_against_oracle(gpu, pairs, shape):
    from baddiffusion_amd import metrics
    a, b = pairs[shape]
    got = metrics.ssim_per_image(a.to(gpu), b.to(gpu))
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (shape[0],)
    want = np.array([metrics_ref.ssim_ref(a[n:n + 1].numpy(), b[n:n + 1].numpy()) for n in range(shape[0])])
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"MEASURE ssim_per_image {shape} worst abs {err.max():.3e}")
    assert err.max() <= 2e-5, err
    mean, whole = float(got.double().mean()), metrics.ssim(a.to(gpu), b.to(gpu))
    print(f"MEASURE ssim_per_image {shape} mean {mean:.9g} metrics.ssim {whole:.9g}")
    assert abs(mean - whole) <= 2e-5
    same = metrics.ssim_per_image(a.to(gpu), a.clone().to(gpu))
    assert float((same - 1.0).abs().max()) <= 1e-6


# ---------------------------------------------------------------------------------------------------- independence, bit for bit
def kernels(ops):
    return (("image_loss", lambda p, t: ops.image_loss(p, t, "l2")), ("image_loss huber", lambda p, t: ops.image_loss(p, t, "huber")),
            ("ssim_images", ops.ssim_images))


def test_scores_do_not_depend_on_storage_broadcast_batch_or_call(gpu):
    from baddiffusion_amd import ops
    g = torch.Generator().manual_seed(5)
    P, T = torch.rand(64, 3, 33, 33, generator=g).to(gpu), torch.rand(64, 3, 33, 33, generator=g).to(gpu)
    shared = T[9]
    for name, fn in kernels(ops):
        full = fn(P, T)
        assert same_bits(full, fn(P, T)), name                                                # call to call
        assert same_bits(full, fn(nhwc(P), nhwc(T))) and same_bits(full, fn(nhwc(P), T)), name  # storage order, of either operand
        assert same_bits(full, fn(P.contiguous(memory_format=torch.channels_last), T)), name
        one = fn(P, shared)                                                                   # stride 0 over the batch
        assert same_bits(one, fn(P, shared[None].expand(64, -1, -1, -1).contiguous())), name
        assert same_bits(one, fn(P, shared[None])) and same_bits(one, fn(nhwc(P), nhwc(shared[None])[0])), name
        grey = T[9, :1].expand(3, -1, -1)                                                     # stride 0 over the channels too
        assert same_bits(fn(P, grey), fn(P, grey.contiguous())), name
        for i in (0, 5, 63):                                                                  # alone and inside batches of 2, 7 and 64
            assert same_bits(fn(P[i:i + 1], T[i:i + 1]), full[i:i + 1]), (name, i)
        assert same_bits(fn(P[5:7], T[5:7]), full[5:7]) and same_bits(fn(P[3:10], T[3:10]), full[3:10]), name
        assert same_bits(fn(P[57:], T[57:]), full[57:]), name


def test_large_images_alone_and_in_a_batch(gpu, pairs):
    """(2, 3, 256, 256): 24 chunks of 8192 elements resp. 192 tiles per image, folded by the second launch"""
    from baddiffusion_amd import ops
    a, b = (v.to(gpu) for v in pairs[(2, 3, 256, 256)])
    for name, fn in kernels(ops):
        both = fn(a, b)
        for i in (0, 1):
            assert same_bits(fn(a[i:i + 1], b[i:i + 1]), both[i:i + 1]), (name, i)
        assert same_bits(both, fn(nhwc(a), nhwc(b))) and same_bits(both, fn(a, b)), name
        assert same_bits(fn(a, b[0]), fn(a, b[:1].expand(2, -1, -1, -1).contiguous())), name


def test_plane_chunk_boundary(gpu):
    """N = 21846, C = 3: 65538 planes, three more than one launch of bd_ssim_images takes; 65540 single-pixel images, five more than one
    launch of bd_image_loss takes.  Four distinct pairs repeated: every output equals its pair's among the first four."""
    from baddiffusion_amd import ops
    g = torch.Generator().manual_seed(8)
    P4, T4 = torch.rand(4, 3, 11, 11, generator=g).to(gpu), torch.rand(4, 3, 11, 11, generator=g).to(gpu)
    idx = torch.arange(21846, device=gpu) % 4
    P, T = P4[idx], T4[idx]
    for name, fn in kernels(ops):
        first, out = fn(P4, T4), fn(P, T)
        assert len(set(bits(first).tolist())) == 4, name
        assert same_bits(out, first[idx]), (name, int((out != first[idx]).nonzero()[0]))
        assert same_bits(out[-4:], first[idx[-4:]]), name                                     # behind the boundary
    idx = torch.arange(65540, device=gpu) % 4
    p1, t1 = torch.rand(4, 1, 1, 1, generator=g).to(gpu), torch.rand(4, 1, 1, 1, generator=g).to(gpu)
    assert same_bits(ops.image_loss(p1[idx], t1[idx], "l2"), ops.image_loss(p1, t1, "l2")[idx])


# ---------------------------------------------------------------------------------------------------- attack success rate
def test_attack_success_rate(gpu):
    from baddiffusion_amd import metrics
    g = torch.Generator().manual_seed(2)
    target = torch.rand(3, 32, 32, generator=g)
    hits = target[None] + 1e-3 * torch.randn(6, 3, 32, 32, generator=g)
    images = torch.cat((torch.rand(10, 3, 32, 32, generator=g), hits))[torch.randperm(16, generator=g)].to(gpu)
    asr, mse = metrics.attack_success_rate(images, target.to(gpu), 1e-3)
    assert mse.is_cuda and mse.shape == (16,) and mse.dtype == torch.float32
    assert same_bits(mse, metrics.mse_per_image(images, target.to(gpu)))
    v = np.sort(mse.cpu().numpy())
    print(f"MEASURE attack_success_rate per-image MSE hits {v[:6]} misses {v[6:]}")
    assert v[5] < 1e-5 and v[6] > 0.1 and asr == 6 / 16
    # strict: a threshold equal to an image's own value leaves that image out
    for k in (5, 6, 15):
        assert metrics.attack_success_rate(images, target.to(gpu), float(v[k]))[0] == int((v < v[k]).sum()) / 16
    assert metrics.attack_success_rate(images, target.to(gpu), float(v[0]))[0] == 0.0


# ---------------------------------------------------------------------------------------------------- backdoor_scores, elijah_defense.py
def make_model(cfg, seed, mode="bf16x3"):
    from baddiffusion_amd.unet import unet_from_config
    m = unet_from_config(cfg).cuda()
    m.load_state_dict(U.gen_params(cfg, seed))
    return m.set_compute_mode(mode)


def test_backdoor_scores_with_a_known_target(gpu):
    from baddiffusion_amd import metrics
    from baddiffusion_amd.defense import backdoor_scores
    from baddiffusion_amd.pipelines import DDIMPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    pipe = DDIMPipeline(unet=make_model(C.SMALL_CFGS["small"], 7), scheduler=DDPMScheduler())
    noise = torch.randn(8, 3, 16, 16, generator=torch.Generator().manual_seed(21)).cuda()
    tau = (0.5 * torch.randn(3, 16, 16, generator=torch.Generator().manual_seed(12))).cuda()
    target = (1.5 * torch.randn(3, 16, 16, generator=torch.Generator().manual_seed(13))).cuda()       # partly outside [-1, 1]: clamped
    plain = backdoor_scores(pipe, tau, n=8, init=noise, num_inference_steps=3)
    assert set(plain) == OLD_SCORE_KEYS
    some = backdoor_scores(pipe, tau, n=8, init=noise, num_inference_steps=3, target=target)
    assert set(some) == OLD_SCORE_KEYS | TARGET_KEYS and all(some[k] == plain[k] for k in plain)
    images = {"clean": pipe(batch_size=8, init=noise, output_type="u8", num_inference_steps=3).images,
              "trigger": pipe(batch_size=8, init=noise + tau, output_type="u8", num_inference_steps=3).images}
    t01 = (target / 2 + 0.5).clamp(0, 1)
    per = {tag: metrics.mse_per_image((u8.float() / 255).permute(0, 3, 1, 2), t01) for tag, u8 in images.items()}
    v = torch.cat(list(per.values())).double().sort().values
    threshold = float((v[7] + v[8]) / 2)                                 # between the 8th and the 9th of the 16 values
    scores = backdoor_scores(pipe, tau, n=8, init=noise, num_inference_steps=3, target=target, asr_threshold=threshold)
    assert set(scores) == OLD_SCORE_KEYS | TARGET_KEYS | ASR_KEYS and all(scores[k] == some[k] for k in some)
    for tag, u8 in images.items():
        img = (u8.float() / 255).permute(0, 3, 1, 2)
        assert scores[f"mse_target_{tag}"] == float(per[tag].double().mean())
        assert scores[f"ssim_target_{tag}"] == float(metrics.ssim_per_image(img, t01).double().mean())
        assert scores[f"asr_{tag}"] == metrics.attack_success_rate(img, t01, threshold)[0]
        want = np.mean([metrics_ref.mse_ref(img[n].cpu().numpy(), t01.cpu().numpy()) for n in range(8)])
        assert abs(scores[f"mse_target_{tag}"] - want) <= 1e-6 * want
    assert scores["asr_clean"] + scores["asr_trigger"] == 1.0            # 8 of the 16 values lie below the threshold
    print(f"MEASURE backdoor_scores with target {scores}")


def test_elijah_defense_with_and_without_target(gpu, tmp_path, capsys):
    import elijah_defense as E
    from baddiffusion_amd.model import save_scheduler, save_unet
    from baddiffusion_amd.schedulers import DDPMScheduler
    ckpt = str(tmp_path / "ckpt_small")
    save_unet(make_model(C.SMALL_CFGS["small"], 7), os.path.join(ckpt, "unet"))
    save_scheduler(DDPMScheduler(), os.path.join(ckpt, "scheduler"))
    common = ["--ckpt", ckpt, "--inv_steps", "2", "--inv_batch", "4", "--detect_n", "8", "--sched", "DDIM-SCHED", "--infer_steps", "3",
              "--remove_steps", "1", "--batch", "4"]
    result = E.main(common + ["--output_dir", str(tmp_path / "known"), "--target", "CORNER", "--asr_threshold", "0.5"])
    out = os.path.join(str(tmp_path / "known"), "res_elijah_inv2_lam0.5_rm1_lr2e-05_ckpt_small")
    score = json.load(open(os.path.join(out, "score.json")))
    assert score == json.loads(json.dumps(result))
    for tag in ("before", "after"):
        assert set(score[tag]) == OLD_SCORE_KEYS | TARGET_KEYS | ASR_KEYS
        assert all(isinstance(v, float) and math.isfinite(v) for v in score[tag].values()), score[tag]
        assert 0.0 <= score[tag]["asr_clean"] <= 1.0 and 0.0 <= score[tag]["asr_trigger"] <= 1.0
        assert score[tag]["mse_target_trigger"] > 0 and -1.0 <= score[tag]["ssim_target_trigger"] <= 1.0
    log = capsys.readouterr().out
    assert "ASR" in log and "before -> after" in log
    result = E.main(common + ["--output_dir", str(tmp_path / "unknown")])
    for tag in ("before", "after"):
        assert set(result[tag]) == OLD_SCORE_KEYS
    assert set(result) == {"before", "after", "detected", "removal"}
    assert "ASR" not in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------------- measure()
def test_measure_with_asr_threshold(gpu, tmp_path):
    from PIL import Image
    import baddiffusion as cli
    from baddiffusion_amd.dataset import DatasetLoader
    from baddiffusion_amd.pipelines import DDIMPipeline
    from baddiffusion_amd.schedulers import DDIMScheduler
    cfg_net = dataclasses.replace(C.SMALL_CFGS["small"], sample_size=32)
    model = make_model(cfg_net, 7)
    dsl = DatasetLoader(root=None, name=DatasetLoader.CIFAR10, batch_size=8, seed=0, device=gpu, num_images=8)
    dsl.set_poison(trigger_type="BOX_14", target_type="CORNER", clean_rate=1.0, poison_rate=0.25).prepare_dataset(mode="FIXED")

    class Pipe(DDIMPipeline):
        def __call__(self, **kw):
            return super().__call__(num_inference_steps=3, **kw)

    def run(out, **opts):
        config = cli.TrainingConfig()
        config.output_dir = str(out); config.seed = 0; config.clip = False; config.sample_ep = None
        config.measure_sample_n = 12; config.eval_max_batch = 8
        for k, v in opts.items():
            setattr(config, k, v)
        os.makedirs(config.output_dir, exist_ok=True)
        return config, cli.measure(config, dsl, "measure", Pipe(model, DDIMScheduler(num_train_timesteps=1000, clip_sample=False)), rank=0, world=1)

    old_keys = {"FID", "FID_reason", "MSE", "SSIM", "inference_chunk"}
    config, plain = run(tmp_path / "plain")
    assert set(plain) == {k + "_noclip" for k in old_keys}
    assert sorted(os.listdir(os.path.join(config.output_dir, "measure"))) == ["backdoor_noclip", "clean_noclip"]       # no npz
    config, score = run(tmp_path / "asr", asr_threshold=0.3, sample_ep=5)
    assert set(score) == {k + "_ep5_noclip" for k in old_keys | {"ASR", "ASR_threshold"}}
    assert score == json.load(open(os.path.join(config.output_dir, "score.json")))
    assert score["ASR_threshold_ep5_noclip"] == 0.3
    assert score["MSE_ep5_noclip"] == plain["MSE_noclip"] and score["SSIM_ep5_noclip"] == plain["SSIM_noclip"]      # the means are the old calls'
    ep = os.path.join(config.output_dir, "measure", "ep5")
    assert sorted(os.listdir(ep)) == ["backdoor_noclip", "backdoor_noclip_scores.npz", "clean_noclip"]
    z = np.load(os.path.join(ep, "backdoor_noclip_scores.npz"))
    assert sorted(z.files) == ["mse", "ssim"]
    mse, ssim = z["mse"], z["ssim"]
    assert mse.shape == ssim.shape == (12,) and mse.dtype == ssim.dtype == np.float32
    tgt = np.clip(dsl.target.cpu().numpy().astype(np.float64) / 2 + 0.5, 0, 1)
    for i in range(12):                                                                # numeric order of the PNG names: 10.png is row 10, not row 2
        img = np.asarray(Image.open(os.path.join(ep, "backdoor_noclip", f"{i}.png")).convert("RGB"), dtype=np.float64).transpose(2, 0, 1) / 255.0
        want = metrics_ref.mse_ref(img, tgt)
        assert abs(mse[i] - want) <= 1e-6 * want, (i, mse[i], want)
        assert abs(ssim[i] - metrics_ref.ssim_ref(img[None], tgt[None])) <= 2e-5, i
    assert score["ASR_ep5_noclip"] == int((mse < np.float32(0.3)).sum()) / 12
    assert abs(float(mse.astype(np.float64).mean()) - score["MSE_ep5_noclip"]) <= 1e-6 * score["MSE_ep5_noclip"]
    print(f"MEASURE measure() per-image mse {mse} ssim {ssim} ASR {score['ASR_ep5_noclip']}")


# ---------------------------------------------------------------------------------------------------- loss split
def test_track_split_leaves_the_trajectory_alone(gpu):
    from baddiffusion_amd.schedulers import DDPMScheduler
    from baddiffusion_amd.trainer import TrainEngine
    cfg = C.SMALL_CFGS["small"]
    g = torch.Generator().manual_seed(4)
    images = torch.randint(0, 256, (4, 16, 16, 3), generator=g, dtype=torch.uint8).to(gpu)
    trigger, target = (torch.randn(3, 16, 16, generator=g).to(gpu) for _ in range(2))
    steps = [(torch.randn(4, 3, 16, 16, generator=g).to(gpu), torch.randint(0, 1000, (4,), generator=g).to(gpu)) for _ in range(3)]
    pois = torch.tensor([1, 0, 1, 0], dtype=torch.bool, device=gpu)
    runs = {}
    for track in (False, True):
        m = make_model(cfg, 7)
        e = TrainEngine(m, DDPMScheduler(), lr=1e-3, lr_warmup_steps=0, num_training_steps=None, use_graph=False, track_split=track)
        losses = [e.train_step(images, pois, trigger, target, noise, t).clone() for noise, t in steps]
        runs[track] = (e, m.flat.detach().clone(), losses)
    (e0, flat0, l0), (e1, flat1, l1) = runs[False], runs[True]
    assert e0.row_losses is None and e0.split_losses is None
    assert torch.equal(flat0, flat1) and torch.equal(e0.m, e1.m) and torch.equal(e0.v, e1.v)
    assert all(torch.equal(a, b) for a, b in zip(l0, l1)) and not torch.equal(l0[0], l0[2])
    rows = e1.row_losses
    assert rows.shape == (4,) and rows.dtype == torch.float32 and rows.is_cuda
    mean, loss = float(rows.double().mean()), float(l1[-1])
    print(f"MEASURE track_split rows {rows.tolist()} mean {mean:.9g} loss {loss:.9g} split {e1.split_losses.tolist()}")
    assert abs(mean - loss) <= 1e-6 * loss
    r = rows.cpu().numpy().astype(np.float64)
    want = np.float32([(r[1] + r[3]) / 2, (r[0] + r[2]) / 2])                        # (clean, poisoned)
    assert e1.split_losses.shape == (2,) and e1.split_losses.is_cuda
    assert np.array_equal(e1.split_losses.cpu().numpy().view(np.uint32), want.view(np.uint32))
    noise, t = steps[0]
    e1.train_step(images, torch.zeros(4, dtype=torch.bool, device=gpu), trigger, target, noise, t)
    split = e1.split_losses.cpu().numpy()
    all_rows = float(e1.row_losses.cpu().numpy().astype(np.float64).mean())
    assert math.isnan(split[1]) and abs(float(split[0]) - all_rows) <= 1e-6 * all_rows         # (fp64 sum of four values, then one fp32 rounding)
    with pytest.raises(ValueError):
        TrainEngine(make_model(cfg, 7), DDPMScheduler(), track_split=True, use_graph=True)


def test_train_loop_logs_the_loss_split(gpu, tmp_path):
    import baddiffusion as cli
    from baddiffusion_amd.dataset import DatasetLoader
    from baddiffusion_amd.pipelines import DDIMPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    cfg_net = dataclasses.replace(C.SMALL_CFGS["small"], sample_size=32)

    class Pipe(DDIMPipeline):
        def __call__(self, **kw):
            return super().__call__(num_inference_steps=2, **kw)

    logs = {}
    for flag in (True, False):
        model = make_model(cfg_net, 7)
        dsl = DatasetLoader(root=None, name=DatasetLoader.CIFAR10, batch_size=4, seed=0, device=gpu, num_images=8)
        dsl.set_poison(trigger_type="BOX_14", target_type="CORNER", clean_rate=1.0, poison_rate=0.25).prepare_dataset(mode="FIXED")
        config = cli.TrainingConfig()
        config.mode, config.dataset, config.ckpt, config.sched = cli.MODE_TRAIN, "CIFAR10", "local", None
        config.output_dir = str(tmp_path / f"run{int(flag)}"); os.makedirs(config.output_dir)
        config.ckpt_path = os.path.join(config.output_dir, config.ckpt_dir)
        config.data_ckpt_path = os.path.join(config.output_dir, config.data_ckpt_dir)
        config.batch, config.epoch, config.gradient_accumulation_steps, config.learning_rate, config.lr_warmup_steps = 4, 1, 1, 1e-3, 2
        config.clip, config.sample_ep, config.eval_sample_n, config.eval_max_batch, config.seed = False, None, 4, 4, 0
        config.log_loss_split = flag
        torch.manual_seed(3)
        cli.train_loop(config, model, DDPMScheduler(clip_sample=False), lambda unet, scheduler: Pipe(unet, scheduler), dsl, gpu, 1, 0)
        logs[flag] = [json.loads(ln) for ln in open(os.path.join(config.output_dir, "log.jsonl"))]
    rec, old = logs[True][0], logs[False][0]
    assert set(old) == {"loss", "lr", "epoch", "step"} and set(rec) == set(old) | {"loss_clean", "loss_poison"}
    assert rec["loss"] == old["loss"] and rec["step"] == 1
    vals = [rec["loss_clean"], rec["loss_poison"]]
    assert all(v is None or (isinstance(v, float) and math.isfinite(v) and v > 0) for v in vals) and rec["loss_clean"] is not None
    print(f"MEASURE log.jsonl with --log_loss_split {rec}")
