"""GPU: bd_vb_terms against the float64 contract (tests/golden/vb.npz, written by make_golden_vb.py from cases_vb.kernel_formula), its
independence properties as equal bits, likelihood.bits_per_dim end to end against the reference UNet's terms, and the two command lines.
Run with -m gpu on an MI355X.

Bound of a kernel output against its float64 reference: max(4e-6 |ref|, 4 d32), d32 being the stored distance of the float32 evaluation of
the same formula -- the pair test_kdiff.py uses.  End to end: the project's standing 1e-3 |ref| per term."""
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_ref as U
from tests.golden import cases as C
from tests.golden import cases_vb as CV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def tables(gpu):
    from baddiffusion_amd import likelihood
    from baddiffusion_amd.schedulers import DDPMScheduler
    s = DDPMScheduler()
    return {vt: likelihood.vb_tables(s, vt, device=gpu) for vt in CV.VARIANCE_TYPES}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def nhwc(t):
    """the same logical [N,C,H,W] tensor in NHWC storage"""
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def within(got, ref, d32, what):
    got, ref, d32 = (np.asarray(v, dtype=np.float64) for v in (got.cpu() if torch.is_tensor(got) else got, ref, d32))
    bound = np.maximum(4e-6 * np.abs(ref), 4 * d32)
    dev = np.abs(got - ref)
    assert (dev <= bound).all(), (what, got, ref, dev, bound)
    return float((dev / bound)[bound > 0].max()) if (bound > 0).any() else 0.0


def run(x0, x_t, eps, ts, tab, clip, mse=True):
    from baddiffusion_amd import ops
    return ops.vb_terms(x0, x_t, eps, torch.tensor(ts, dtype=torch.int64), tab, clip_denoised=clip, want_x0_mse=mse)


# ---------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("shape", CV.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_terms_against_the_contract(gpu, golden, tables, shape):
    """D = 1, 255, 257, 8191, 8192, 8193, 3 * 8192 + 5 x N in {1, 5} x both variance types x clip on and off, every batch a mix of
    t in {0, 1, 2, 500, T-1, T}: bits and x0_mse within the bound; NHWC storage and a row alone give the batch's bits"""
    g = golden("vb")
    worst = 0.0
    for tag, shp, N, ts, vt, clip, seed in CV.kernel_cases():
        if shp != shape:
            continue
        x0, x_t, eps = (v.cuda() for v in CV.make_rows(seed, N, shp, ts))
        got, mse = run(x0, x_t, eps, ts, tables[vt], clip)
        assert got.shape == mse.shape == (N,) and got.dtype == torch.float32
        worst = max(worst, within(got, g[f"k_{tag}_bits"], g[f"k_{tag}_d32"], tag), within(mse, g[f"k_{tag}_mse"], g[f"k_{tag}_mse_d32"], tag))
        alone = run(x0, x_t, eps, ts, tables[vt], clip, mse=False)
        assert same_bits(alone, got), tag                                            # the optional output changes nothing
        got2, mse2 = run(nhwc(x0), nhwc(x_t), nhwc(eps), ts, tables[vt], clip)
        assert same_bits(got2, got) and same_bits(mse2, mse), tag
        if N > 1:
            k = N // 2
            one, one_mse = run(x0[k: k + 1], nhwc(x_t[k: k + 1]), eps[k: k + 1], ts[k: k + 1], tables[vt], clip)
            assert same_bits(one, got[k: k + 1]) and same_bits(one_mse, mse[k: k + 1]), tag
            rev = run(x0.flip(0), x_t.flip(0), eps.flip(0), ts[::-1], tables[vt], clip, mse=False)
            assert same_bits(rev.flip(0), got), tag
    print(f"MEASURE bd_vb_terms {shape}: worst share of the bound max(4e-6 |ref|, 4 d32) {worst:.3f}")


def test_more_rows_than_one_launch(gpu, golden, tables):
    """N = 65538 single-chunk images of 15 elements, three more than one launch's grid.y: four distinct rows repeated"""
    g = golden("vb")
    x0, x_t, eps = (v.cuda() for v in CV.big_rows())
    reps = -(-CV.BIG_N // len(CV.BIG_TS))
    big = lambda v: v.repeat(reps, 1, 1, 1)[: CV.BIG_N]
    ts = (CV.BIG_TS * reps)[: CV.BIG_N]
    got = run(big(x0), big(x_t), big(eps), ts, tables["fixed_small"], True, mse=False)
    assert got.shape == (CV.BIG_N,)
    first = got[: len(CV.BIG_TS)]
    within(first, g["big_bits"], g["big_d32"], "big")
    want = first.repeat(reps)[: CV.BIG_N]
    assert same_bits(got, want)


def test_decoder_regimes(gpu, golden, tables):
    """t = 0 rows: prediction x0 + s * randn for s in {0.003, 0.01, 0.03, 0.1} (floor share 0, 0, 6.5 %, 56 %), all pixels at u = 0, all
    at u = 255, a mix, every pixel on the floor (exactly -log2 1e-12), one NaN pixel (that row NaN, its neighbours untouched)"""
    g = golden("vb")
    tab = tables["fixed_small"]
    rows = CV.regime_rows()
    alone = {}
    for name, (x0, x_t, eps, clip) in rows.items():
        got = run(x0.cuda(), x_t.cuda(), eps.cuda(), (0,), tab, clip, mse=False)
        alone[name] = got
        if name == "nan":
            assert bool(torch.isnan(got).all())
            continue
        share = within(got, g[f"r_{name}_bits"], g[f"r_{name}_d32"], name)
        print(f"MEASURE bd_vb_terms t = 0 regime {name}: {float(got):.6f} bits, reference {float(g[f'r_{name}_bits'][0]):.6f}, share of the bound {share:.3f}")
    assert float(alone["floor"]) == float(np.float32(CV.FLOOR_BITS))
    names = [n for n in rows if rows[n][3]]                                         # the clipped rows as one batch, the NaN row inside
    batch = [torch.cat([rows[n][k] for n in names]).cuda() for k in range(3)]
    got, mse = run(*batch, (0,) * len(names), tab, True)
    for k, n in enumerate(names):
        if n == "nan":
            assert math.isnan(float(got[k])) and math.isnan(float(mse[k]))
        else:
            assert same_bits(got[k: k + 1], alone[n]) and math.isfinite(float(mse[k])), n
    # a NaN in x0 of a prior row, and NaN in the x_t / eps a prior row does not read
    x0, x_t, eps = (v.cuda() for v in CV.make_rows(1, 3, (3, 8, 8), (CV.T, CV.T, 500)))
    clean = run(x0, x_t, eps, (CV.T, CV.T, 500), tab, True, mse=False)
    x_t[0], eps[0] = float("nan"), float("nan")
    x0[1, 0, 0, 0] = float("nan")
    got = run(x0, x_t, eps, (CV.T, CV.T, 500), tab, True, mse=False)
    assert same_bits(got[0:1], clean[0:1]) and math.isnan(float(got[1])) and same_bits(got[2:], clean[2:])
    only_prior = run(x0[:1], None, None, (CV.T,), tab, True, mse=False)
    assert same_bits(only_prior, clean[0:1])


def test_wrapper_refusals(gpu, tables):
    from baddiffusion_amd import ops
    tab = tables["fixed_small"]
    x0, x_t, eps = (v.cuda() for v in CV.make_rows(2, 2, (3, 8, 8), (0, 5)))
    t = torch.tensor([0, 5])
    for bad_t, pat in ((torch.tensor([0, CV.T + 1]), "outside"), (torch.tensor([-1, 0]), "outside")):
        with pytest.raises(RuntimeError, match=f"bd_vb_terms: t.*{pat}"):
            ops.vb_terms(x0, x_t, eps, bad_t, tab)
    with pytest.raises(RuntimeError, match="null x_t or eps"):
        ops.vb_terms(x0, None, eps, t, tab)
    with pytest.raises(TypeError, match="int64"):
        ops.vb_terms(x0, x_t, eps, t.int(), tab)
    with pytest.raises(TypeError, match="int64"):
        ops.vb_terms(x0, x_t, eps, t[:1], tab)
    with pytest.raises(TypeError, match="x_t must be float32"):
        ops.vb_terms(x0, x_t.double(), eps, t, tab)
    with pytest.raises(TypeError, match="eps must be float32"):
        ops.vb_terms(x0, x_t, eps[:, :, :4], t, tab)
    with pytest.raises(TypeError, match="x0 must be"):
        ops.vb_terms(x0[0], x_t, eps, t, tab)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.vb_terms(x0.cpu(), x_t, eps, t, tab)
    dev_t = ops.vb_terms(x0, x_t, eps, t.cuda(), tab)                                  # a device t is accepted (and copied back)
    assert same_bits(dev_t, ops.vb_terms(x0, x_t, eps, t, tab))


# ---------------------------------------------------------------------------------------------------- end to end
def make_model(mode=None):
    from baddiffusion_amd.unet import unet_from_config
    cfg = C.SMALL_CFGS[CV.E2E_CFG]
    m = unet_from_config(cfg).cuda()
    m.load_state_dict(U.gen_params(cfg, CV.E2E_PARAM_SEED))
    return m if mode is None else m.set_compute_mode(mode)


@pytest.mark.parametrize("mode", ("f32", None), ids=("f32", "default"))
def test_bits_per_dim_vs_reference_unet(gpu, golden, mode):
    """bits_per_dim on the small UNet at t = 0, 1, 2, 250, T-1 and the prior, against the terms of the reference UNet's prediction on the
    reference's add_noise (float64 formula), both variance types: every term within 1e-3 |ref|.  The noise goes through the generator,
    largest t first.
    Measured on an MI355X (worst term's share of the bound): see README, "Bits per dimension"."""
    from baddiffusion_amd import likelihood
    from baddiffusion_amd.schedulers import DDPMScheduler
    g = golden("vb")
    model, clean = make_model(mode), CV.e2e_clean().cuda()
    for vt in CV.VARIANCE_TYPES:
        ref = g[f"e2e_{vt}"]
        res = likelihood.bits_per_dim(model, DDPMScheduler(), clean, timesteps=CV.E2E_TS, variance_type=vt,
                                      generator=torch.Generator().manual_seed(CV.E2E_NOISE_SEED), max_batch_n=7)
        got = res["terms"].double().numpy()
        assert got.shape == ref.shape == (len(CV.E2E_TS) + 1, CV.E2E_N) and res["timesteps"] == tuple(sorted(CV.E2E_TS))
        dev = np.abs(got - ref) / np.abs(ref)
        rows = ", ".join(f"t={t}: {d:.2e}" for t, d in zip(res["timesteps"] + ("prior",), dev.max(1)))
        print(f"MEASURE bits_per_dim vs reference UNet mode={model.compute_mode} {vt}: worst |term - ref| / |ref| per row {rows}; "
              f"share of the 1e-3 bound {dev.max() / 1e-3:.3f}")
        assert (dev <= 1e-3).all(), (vt, dev)
        handed = likelihood.bits_per_dim(model, DDPMScheduler(), clean, timesteps=CV.E2E_TS, variance_type=vt, noises=CV.e2e_noises(),
                                         max_batch_n=7)
        assert torch.equal(handed["terms"], res["terms"])                              # the same chunks: the same UNet batches


def test_unmodified_model_scores_equal_bits_twice(gpu):
    from baddiffusion_amd import likelihood
    from baddiffusion_amd.schedulers import DDPMScheduler
    model, clean, s = make_model(), CV.e2e_clean().cuda(), DDPMScheduler()
    a, b = (likelihood.bits_per_dim(model, s, clean, n=3, timesteps=(0, 3, 999), generator=torch.Generator(device="cuda").manual_seed(5),
                                    max_batch_n=4) for _ in range(2))
    c = likelihood.bits_per_dim(model, s, clean, n=3, timesteps=(0, 3, 999), generator=torch.Generator(device="cuda").manual_seed(6))
    assert torch.equal(a["terms"], b["terms"]) and a["mean_bpd"] == b["mean_bpd"] and not torch.equal(a["terms"], c["terms"])
    assert torch.equal(a["terms"][-1], c["terms"][-1])                              # the prior term reads no noise


# ---------------------------------------------------------------------------------------------------- command lines
@pytest.fixture
def ckpt(tmp_path):
    """the checkpoint fixture (tests/golden/ckpt: the reference's save_pretrained layout) with its weights re-materialised"""
    src = os.path.join(ROOT, "tests", "golden", "ckpt")
    man = json.load(open(os.path.join(src, "manifest.json")))
    d = str(tmp_path / "ckpt_fixture")
    shutil.copytree(src, d)
    P = U.gen_params(C.SMALL_CFGS[man["config"]], man["seed"])
    torch.save({k: v.clone() for k, v in P.items()}, os.path.join(d, "unet", "diffusion_pytorch_model.bin"))
    return d


def test_likelihood_eval_writes_both_files(gpu, ckpt, tmp_path, monkeypatch):
    import likelihood_eval as LE
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path / "out")
    result = LE.main(["--ckpt", ckpt, "--n", "3", "--batch", "8", "--t_stride", "250", "--target", "CORNER", "--output_dir", out])
    folder = os.path.join(out, "res_likelihood_n3_k250_ckpt_fixture")
    score = json.load(open(os.path.join(folder, "likelihood.json")))
    assert score == json.loads(json.dumps(result))
    assert score["complete"] is False and score["t_stride"] == 250 and score["n"] == 3 and score["timesteps"] == 5
    assert score["variance_type"] == "fixed_large" and score["clip_denoised"] is True and "mean_bpd" not in score
    assert len(score["per_image"]) == 3 and all(math.isfinite(v) and v > 0 for v in score["per_image"] + [score["target_bpd"]])
    terms = np.load(os.path.join(folder, "likelihood_terms.npz"))
    assert terms["terms"].shape == (6, 4) and terms["terms"].dtype == np.float32 and terms["timesteps"].tolist() == [0, 1, 251, 501, 751]
    est = terms["terms"][-1].astype(np.float64) + terms["terms"][0] + 250 * terms["terms"][1:-1].astype(np.float64).sum(0)
    np.testing.assert_allclose(score["per_image"] + [score["target_bpd"]], est, rtol=1e-12)
    np.testing.assert_allclose(score["estimate_bpd"], est[:3].mean(), rtol=1e-12)
    full = LE.main(["--ckpt", ckpt, "--n", "1", "--batch", "500", "--no_clip", "--variance_type", "fixed_small", "--output_dir", out])
    assert full["complete"] is True and full["timesteps"] == 1000 and full["mean_bpd"] == full["estimate_bpd"] and full["clip_denoised"] is False
    print(f"MEASURE likelihood_eval on the checkpoint fixture (random weights): estimate at stride 250 {score['estimate_bpd']:.4f} bits/dim, "
          f"full bound of image 0 unclipped fixed_small {full['mean_bpd']:.4f}")


def test_elijah_defense_bpd_images(gpu, ckpt, tmp_path, monkeypatch):
    import elijah_defense as E
    monkeypatch.chdir(tmp_path)
    common = ["--ckpt", ckpt, "--inv_steps", "2", "--inv_batch", "4", "--detect_n", "4", "--sched", "DDIM-SCHED", "--infer_steps", "2",
              "--remove_steps", "2", "--batch", "4"]
    name = "res_elijah_inv2_lam0.5_rm2_lr2e-05_ckpt_fixture"
    out = str(tmp_path / "bpd")
    result = E.main(common + ["--output_dir", out, "--bpd_images", "3", "--bpd_t_stride", "250"])
    score = json.load(open(os.path.join(out, name, "score.json")))
    assert score == json.loads(json.dumps(result)) and set(score) == {"before", "after", "detected", "removal", "bpd"}
    bpd = score["bpd"]
    assert set(bpd) == {"n", "t_stride", "before", "after", "complete"} and (bpd["n"], bpd["t_stride"], bpd["complete"]) == (3, 250, False)
    assert math.isfinite(bpd["before"]) and math.isfinite(bpd["after"]) and bpd["before"] > 0 and bpd["before"] != bpd["after"]
    plain = E.main(common + ["--output_dir", str(tmp_path / "plain")])
    assert set(plain) == {"before", "after", "detected", "removal"} and plain["before"] == score["before"]
    config = json.load(open(os.path.join(str(tmp_path / "plain"), name, "config.json")))
    assert not any(k.startswith("bpd") for k in config)
    print(f"MEASURE elijah_defense --bpd_images 3 --bpd_t_stride 250 (random weights, 2 steps): {bpd['before']:.6g} -> {bpd['after']:.6g}")
