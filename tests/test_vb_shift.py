"""GPU: bd_vb_terms_shift against the float64 contract (tests/golden/vb_shift.npz, written by make_golden_vb_shift.py from
cases_vb_shift.kernel_formula), its independence properties and its regression to bd_vb_terms as equal bits,
likelihood.bits_per_dim(backdoor=...) end to end against the terms of the reference's chain and UNet, and the two command lines.
Run with -m gpu on an MI355X.

Bound of a kernel output against its float64 reference: max(4e-6 |ref|, 4 d32), d32 being the stored distance of the float32 evaluation of
the same formula -- the pair test_vb.py uses.  End to end: the project's standing 1e-3 |ref| per term."""
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
from tests.golden import cases_vb_shift as CS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = CV.T


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
    return {vt: likelihood.vb_tables(s, vt, device=gpu, shift=True) for vt in CV.VARIANCE_TYPES}


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


def run(x0, x_t, eps, r, ts, tab, clip, mse=True):
    from baddiffusion_amd import ops
    return ops.vb_terms_shift(x0, x_t, eps, r, torch.tensor(ts, dtype=torch.int64), tab, clip_denoised=clip, want_x0_mse=mse)


def plain(x0, x_t, eps, ts, tab, clip, mse=True):
    from baddiffusion_amd import ops
    return ops.vb_terms(x0, x_t, eps, torch.tensor(ts, dtype=torch.int64), tab, clip_denoised=clip, want_x0_mse=mse)


# ---------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("shape", CV.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_terms_against_the_contract(gpu, golden, tables, shape):
    """D = 1, 255, 257, 8191, 8192, 8193, 3 * 8192 + 5 x N in {1, 5} x both variance types x clip on and off, every batch a mix of
    t in {0, 1, 2, 500, T-1, T}: bits and x0_mse within the bound.  Equal bits: NHWC r (and the other streams), r per row against the
    same image broadcast by stride 0, a row alone, the batch reversed, with and without want_x0_mse."""
    g = golden("vb_shift")
    worst = 0.0
    for tag, shp, N, ts, vt, clip, seed in CS.kernel_cases():
        if shp != shape:
            continue
        x0, x_t, eps, r = (v.cuda() for v in CS.make_rows(seed, N, shp, ts))
        got, mse = run(x0, x_t, eps, r, ts, tables[vt], clip)
        assert got.shape == mse.shape == (N,) and got.dtype == torch.float32
        worst = max(worst, within(got, g[f"k_{tag}_bits"], g[f"k_{tag}_d32"], tag), within(mse, g[f"k_{tag}_mse"], g[f"k_{tag}_mse_d32"], tag))
        alone = run(x0, x_t, eps, r, ts, tables[vt], clip, mse=False)
        assert same_bits(alone, got), tag                                            # the optional output changes nothing
        got2, mse2 = run(x0, x_t, eps, nhwc(r), ts, tables[vt], clip)
        assert same_bits(got2, got) and same_bits(mse2, mse), tag
        got2, mse2 = run(nhwc(x0), nhwc(x_t), nhwc(eps), nhwc(r), ts, tables[vt], clip)
        assert same_bits(got2, got) and same_bits(mse2, mse), tag
        # one image for every row, by stride 0, against the same image stored per row
        rep = r[:1].repeat(N, 1, 1, 1)
        per_row, per_row_mse = run(x0, x_t, eps, rep, ts, tables[vt], clip)
        for one in (r[0], r[:1], nhwc(r[:1]), r[:1].expand(N, -1, -1, -1)):
            b, m = run(x0, x_t, eps, one, ts, tables[vt], clip)
            assert same_bits(b, per_row) and same_bits(m, per_row_mse), tag
        assert same_bits(per_row[:1], got[:1])
        if N > 1:
            k = N // 2
            one, one_mse = run(x0[k: k + 1], nhwc(x_t[k: k + 1]), eps[k: k + 1], r[k], ts[k: k + 1], tables[vt], clip)
            assert same_bits(one, got[k: k + 1]) and same_bits(one_mse, mse[k: k + 1]), tag
            rev = run(x0.flip(0), x_t.flip(0), eps.flip(0), r.flip(0), ts[::-1], tables[vt], clip, mse=False)
            assert same_bits(rev.flip(0), got), tag
    print(f"MEASURE bd_vb_terms_shift {shape}: worst share of the bound max(4e-6 |ref|, 4 d32) {worst:.3f}")


@pytest.mark.parametrize("shape", ((3, 5, 17), (1, 47, 523)), ids=("one_chunk", "four_chunks"))
def test_zero_shift_is_the_unshifted_kernel(gpu, tables, shape):
    """r = 0: every row equals ops.vb_terms on the same inputs bit for bit (bits and x0_mse); a t = 0 row does so for any r, a NaN r
    included"""
    ts = CV.TS_MIX
    for vt in CV.VARIANCE_TYPES:
        for clip in (True, False):
            x0, x_t, eps, r = (v.cuda() for v in CS.make_rows(901, len(ts), shape, ts))
            want, want_mse = plain(x0, x_t, eps, ts, tables[vt], clip)
            for zero in (torch.zeros_like(r), torch.zeros(shape, device="cuda")):
                got, mse = run(x0, x_t, eps, zero, ts, tables[vt], clip)
                assert same_bits(got, want) and same_bits(mse, want_mse), (vt, clip)
            dec = [k for k, t in enumerate(ts) if t == 0]
            got, mse = run(x0, x_t, eps, r, ts, tables[vt], clip)
            assert same_bits(got[dec], want[dec]) and same_bits(mse[dec], want_mse[dec])
            assert not same_bits(got, want)
            got, mse = run(x0, x_t, eps, torch.full_like(r, float("nan")), ts, tables[vt], clip)
            assert same_bits(got[dec], want[dec]) and same_bits(mse[dec], want_mse[dec])
            rest = [k for k, t in enumerate(ts) if t != 0]
            assert bool(torch.isnan(got[rest]).all()) and bool(torch.isnan(mse[rest]).all())


def test_nan_in_r_poisons_its_row_alone(gpu, tables):
    """one NaN in r of a KL row and of a prior row: that row is NaN, its neighbours' bits are unchanged; a prior-only batch passes
    x_t = eps = None"""
    tab = tables["fixed_small"]
    ts = (500, T, 2, T, 0, T - 1)
    for shape in ((3, 8, 8), (3, 64, 64)):                                          # one chunk, two chunks
        x0, x_t, eps, r = (v.cuda() for v in CS.make_rows(902, len(ts), shape, ts))
        clean, clean_mse = run(x0, x_t, eps, r, ts, tab, True)
        assert bool(torch.isfinite(clean).all())
        bad = r.clone()
        bad[0, 1, 2, 3] = float("nan")                                              # a KL row
        bad[3, 2, 7, 0] = float("nan")                                              # a prior row
        bad[4, 0, 0, 0] = float("nan")                                              # a t = 0 row: not read
        got, mse = run(x0, x_t, eps, bad, ts, tab, True)
        for k in range(len(ts)):
            if k in (0, 3):
                assert math.isnan(float(got[k])) and math.isnan(float(mse[k])), k
            else:
                assert same_bits(got[k: k + 1], clean[k: k + 1]) and same_bits(mse[k: k + 1], clean_mse[k: k + 1]), k
        # NaN in the x_t / eps a prior row does not read
        x_t2, eps2 = x_t.clone(), eps.clone()
        x_t2[1], eps2[1] = float("nan"), float("nan")
        assert same_bits(run(x0, x_t2, eps2, r, ts, tab, True, mse=False), clean)
        pri = [1, 3]
        only = run(x0[pri], None, None, r[pri], (T, T), tab, True, mse=False)
        assert same_bits(only, clean[pri])
        only, only_mse = run(x0[pri], None, None, r[1], (T, T), tab, True)
        assert same_bits(only[:1], clean[1:2]) and same_bits(only_mse[:1], clean_mse[1:2]) and not same_bits(only[1:], clean[3:4])


def test_wrapper_refusals(gpu, tables):
    from baddiffusion_amd import likelihood, ops
    from baddiffusion_amd.schedulers import DDPMScheduler
    tab = tables["fixed_small"]
    x0, x_t, eps, r = (v.cuda() for v in CS.make_rows(2, 2, (3, 8, 8), (0, 5)))
    t = torch.tensor([0, 5])
    for bad_t in (torch.tensor([0, T + 1]), torch.tensor([-1, 0])):
        with pytest.raises(RuntimeError, match="bd_vb_terms_shift: t.*outside"):
            ops.vb_terms_shift(x0, x_t, eps, r, bad_t, tab)
    with pytest.raises(RuntimeError, match="bd_vb_terms_shift: null x_t or eps"):
        ops.vb_terms_shift(x0, None, eps, r, t, tab)
    with pytest.raises(TypeError, match="int64"):
        ops.vb_terms_shift(x0, x_t, eps, r, t.int(), tab)
    with pytest.raises(TypeError, match="x_t must be float32"):
        ops.vb_terms_shift(x0, x_t.double(), eps, r, t, tab)
    with pytest.raises(TypeError, match="x0 must be"):
        ops.vb_terms_shift(x0[0], x_t, eps, r, t, tab)
    for bad_r in (r.double(), r[:, :, :4], r[0, 0], None, torch.cat((r, r))):
        with pytest.raises(TypeError, match="vb_terms_shift: r must be float32"):
            ops.vb_terms_shift(x0, x_t, eps, bad_r, t, tab)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.vb_terms_shift(x0, x_t, eps, r.cpu(), t, tab)
    with pytest.raises(ValueError, match="float32 shift of length"):
        ops.vb_terms_shift(x0, x_t, eps, r, t, likelihood.vb_tables(DDPMScheduler(), "fixed_small", device=x0.device))
    assert same_bits(ops.vb_terms_shift(x0, x_t, eps, r, t.cuda(), tab), ops.vb_terms_shift(x0, x_t, eps, r, t, tab))


def test_training_target_of_poison_qsample(gpu, tables):
    """x_t and target of one ops.poison_qsample call on poisoned rows, the target fed back as eps_hat with the clamp off: a perfectly
    backdoored model.  The rows meet the contract's bound; how far the fixed_small KL rows sit above 0 is printed, not bounded.
    Measured on an MI355X: see README, "Bits per dimension"."""
    from baddiffusion_amd import ops
    from baddiffusion_amd.schedulers import DDPMScheduler
    s = DDPMScheduler()
    alphas, ac = s.device_tables(gpu)
    ts = (0, 1, 2, 10, 250, 500, T - 2, T - 1)
    n = len(ts)
    clean = torch.randint(0, 256, (n, 16, 16, 3), generator=torch.Generator().manual_seed(31), dtype=torch.uint8).cuda()
    trigger, target = (v.cuda() for v in CS.e2e_backdoor())
    noise = torch.randn(n, 3, 16, 16, generator=torch.Generator().manual_seed(32)).cuda()
    xn, tg, R, x0 = ops.poison_qsample(clean, torch.ones(n, dtype=torch.uint8, device=gpu), trigger, target, noise,
                                       torch.tensor(ts, device=gpu), alphas, ac, want_batch=True)
    x_t, eps = xn.permute(0, 3, 1, 2), tg.permute(0, 3, 1, 2)
    for vt in CV.VARIANCE_TYPES:
        got, mse = run(x0, x_t, eps, R, ts, tables[vt], False)
        ref = [CS.kernel_formula(*(v.cpu().contiguous() for v in (x0, x_t, eps, R)), ts, vt, False, dt) for dt in (torch.float64, torch.float32)]
        share = max(within(got, ref[0][0], (ref[1][0] - ref[0][0]).abs(), vt), within(mse, ref[0][1], (ref[1][1] - ref[0][1]).abs(), vt))
        above = got.double().cpu() - CV.tables64(vt)["add"][list(ts)] / CV.LN2
        rows = ", ".join(f"t={t}: {float(a):.2e}" for t, a in zip(ts[1:], above[1:]))
        print(f"MEASURE training target of poison_qsample as eps_hat, unclamped, {vt}: bits above add[t] / ln 2 per KL row {rows}; "
              f"L_0 {float(got[0]):.4f}; worst share of the contract's bound {share:.3f}")


# ---------------------------------------------------------------------------------------------------- end to end
def make_model(mode=None):
    from baddiffusion_amd.unet import unet_from_config
    cfg = C.SMALL_CFGS[CV.E2E_CFG]
    m = unet_from_config(cfg).cuda()
    m.load_state_dict(U.gen_params(cfg, CV.E2E_PARAM_SEED))
    return m if mode is None else m.set_compute_mode(mode)


@pytest.mark.parametrize("mode", ("f32", None), ids=("f32", "default"))
def test_bits_per_dim_backdoor_vs_reference_chain(gpu, golden, mode):
    """bits_per_dim(backdoor=...) on the small UNet at t = 0, 1, 2, 250, T-1 and the prior, against the terms of the reference UNet's
    prediction on the reference's q_sample_diffuser rows (float64 formula), both variance types: every term within 1e-3 |ref|.
    Measured on an MI355X (worst term's share of the bound): see README, "Bits per dimension"."""
    from baddiffusion_amd import likelihood
    from baddiffusion_amd.schedulers import DDPMScheduler
    g = golden("vb_shift")
    model, clean = make_model(mode), CV.e2e_clean().cuda()
    pair = CS.e2e_backdoor()
    for vt in CV.VARIANCE_TYPES:
        ref = g[f"e2e_{vt}"]
        res = likelihood.bits_per_dim(model, DDPMScheduler(), clean, timesteps=CV.E2E_TS, variance_type=vt,
                                      generator=torch.Generator().manual_seed(CV.E2E_NOISE_SEED), max_batch_n=7, backdoor=pair)
        got = res["terms"].double().numpy()
        assert res["backdoor"] is True and got.shape == ref.shape == (len(CV.E2E_TS) + 1, CV.E2E_N)
        assert res["timesteps"] == tuple(sorted(CV.E2E_TS)) and res["complete"] is False
        dev = np.abs(got - ref) / np.abs(ref)
        rows = ", ".join(f"t={t}: {d:.2e}" for t, d in zip(res["timesteps"] + ("prior",), dev.max(1)))
        print(f"MEASURE bits_per_dim(backdoor) vs reference chain + UNet mode={model.compute_mode} {vt}: worst |term - ref| / |ref| per row "
              f"{rows}; share of the 1e-3 bound {dev.max() / 1e-3:.3f}")
        assert (dev <= 1e-3).all(), (vt, dev)
        handed = likelihood.bits_per_dim(model, DDPMScheduler(), clean, timesteps=CV.E2E_TS, variance_type=vt, noises=CV.e2e_noises(),
                                         max_batch_n=7, backdoor={"trigger": pair[0], "target": pair[1]})
        assert torch.equal(handed["terms"], res["terms"])


def test_scored_twice_and_the_plain_path_is_untouched(gpu):
    """a model scored twice gives equal bits; backdoor=None gives the bits of the existing path (the call without the argument), and no
    "backdoor" entry"""
    from baddiffusion_amd import likelihood
    from baddiffusion_amd.schedulers import DDPMScheduler
    model, clean, s = make_model(), CV.e2e_clean().cuda(), DDPMScheduler()
    pair = CS.e2e_backdoor()
    kw = dict(n=3, timesteps=(0, 3, 999), max_batch_n=4)
    gen = lambda seed: torch.Generator(device="cuda").manual_seed(seed)
    a, b = (likelihood.bits_per_dim(model, s, clean, generator=gen(5), backdoor=pair, **kw) for _ in range(2))
    assert torch.equal(a["terms"], b["terms"]) and a["mean_bpd"] == b["mean_bpd"]
    c = likelihood.bits_per_dim(model, s, clean, generator=gen(6), backdoor=pair, **kw)
    assert not torch.equal(a["terms"], c["terms"]) and torch.equal(a["terms"][-1], c["terms"][-1])     # the prior term reads no noise
    old = likelihood.bits_per_dim(model, s, clean, generator=gen(5), **kw)
    none = likelihood.bits_per_dim(model, s, clean, generator=gen(5), backdoor=None, **kw)
    assert torch.equal(old["terms"], none["terms"]) and set(old) == set(none) and "backdoor" not in none
    assert not torch.equal(old["terms"], a["terms"])


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


def test_likelihood_eval_backdoor(gpu, ckpt, tmp_path, monkeypatch):
    import likelihood_eval as LE
    monkeypatch.chdir(tmp_path)
    common = ["--ckpt", ckpt, "--n", "3", "--batch", "8", "--t_stride", "250", "--target", "CORNER"]
    folder = "res_likelihood_n3_k250_ckpt_fixture"
    flagged = LE.main(common + ["--backdoor", "--output_dir", str(tmp_path / "bd")])
    plain_result = LE.main(common + ["--output_dir", str(tmp_path / "plain")])
    score = json.load(open(tmp_path / "bd" / folder / "likelihood.json"))
    assert score == json.loads(json.dumps(flagged))
    b = score.pop("backdoor_bpd")
    assert set(b) == {"estimate_bpd", "per_image", "prior_bpd", "l0_bpd", "clip_denoised"} and b["clip_denoised"] is True
    assert len(b["per_image"]) == 3 and all(math.isfinite(v) and v > 0 for v in b["per_image"] + [b["prior_bpd"], b["l0_bpd"]])
    terms = np.load(tmp_path / "bd" / folder / "likelihood_terms.npz")
    assert set(terms.files) == {"terms", "timesteps", "backdoor_terms"}
    bt = terms["backdoor_terms"]
    assert bt.shape == (6, 3) and bt.dtype == np.float32
    est = bt[-1].astype(np.float64) + bt[0] + 250 * bt[1:-1].astype(np.float64).sum(0)
    np.testing.assert_allclose(b["per_image"], est, rtol=1e-12)
    np.testing.assert_allclose(b["estimate_bpd"], est.mean(), rtol=1e-12)
    np.testing.assert_allclose([b["prior_bpd"], b["l0_bpd"]], [bt[-1].astype(np.float64).mean(), bt[0].astype(np.float64).mean()], rtol=1e-12)
    # without the flag: the files of before (the plain part of the flagged run is the same run, too)
    assert score == json.loads(json.dumps(plain_result)) and "backdoor_bpd" not in plain_result
    assert open(tmp_path / "plain" / folder / "likelihood.json").read() == json.dumps(plain_result, indent=2)
    plain_terms = np.load(tmp_path / "plain" / folder / "likelihood_terms.npz")
    assert plain_terms.files == ["terms", "timesteps"] and np.array_equal(plain_terms["terms"], terms["terms"])
    assert "backdoor" not in json.load(open(tmp_path / "plain" / folder / "config.json"))
    print(f"MEASURE likelihood_eval --backdoor on the checkpoint fixture (random weights, stride 250): clean rows {score['estimate_bpd']:.4f} "
          f"bits/dim, target as clean data {score['target_bpd']:.4f}, target along the triggered chain {b['estimate_bpd']:.4f}")


def test_elijah_defense_bpd_backdoor(gpu, ckpt, tmp_path, monkeypatch):
    import elijah_defense as E
    monkeypatch.chdir(tmp_path)
    common = ["--ckpt", ckpt, "--inv_steps", "2", "--inv_batch", "4", "--detect_n", "4", "--sched", "DDIM-SCHED", "--infer_steps", "2",
              "--remove_steps", "2", "--batch", "4", "--bpd_images", "3", "--bpd_t_stride", "250", "--target", "CORNER"]
    name = "res_elijah_inv2_lam0.5_rm2_lr2e-05_ckpt_fixture"
    flagged = E.main(common + ["--bpd_backdoor", "--output_dir", str(tmp_path / "bd")])
    plain_result = E.main(common + ["--output_dir", str(tmp_path / "plain")])
    score = json.load(open(tmp_path / "bd" / name / "score.json"))
    assert score == json.loads(json.dumps(flagged))
    bpd = score["bpd"]
    assert set(bpd) == {"n", "t_stride", "before", "after", "complete", "backdoor_before", "backdoor_after"}
    assert all(math.isfinite(bpd[k]) and bpd[k] > 0 for k in ("backdoor_before", "backdoor_after")) and bpd["backdoor_before"] != bpd["backdoor_after"]
    assert set(plain_result["bpd"]) == {"n", "t_stride", "before", "after", "complete"}
    for k in ("n", "t_stride", "before", "complete"):                                # the same noise: the figures of the run without the flag
        assert plain_result["bpd"][k] == bpd[k], k
    assert plain_result["before"] == score["before"] and set(plain_result) == set(score)
    assert open(tmp_path / "plain" / name / "score.json").read() == json.dumps(plain_result, indent=2)
    assert "bpd_backdoor" not in json.load(open(tmp_path / "plain" / name / "config.json"))
    assert json.load(open(tmp_path / "bd" / name / "config.json"))["bpd_backdoor"] is True
    print(f"MEASURE elijah_defense --bpd_backdoor (random weights, 2 removal steps, stride 250): target along the triggered chain "
          f"{bpd['backdoor_before']:.6g} -> {bpd['backdoor_after']:.6g}; clean rows {bpd['before']:.6g} -> {bpd['after']:.6g}")
