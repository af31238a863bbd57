"""CPU: the host side of the variational bound -- likelihood.vb_tables against the closed forms, the float64 contract
(tests/golden/cases_vb.py kernel_formula) on cases with known answers, the float32 restatement and the textbook form against the bound the
GPU test holds the kernel to, the bookkeeping of likelihood.bits_per_dim (draw order, chunk packing, complete, estimate) around stand-ins
for the three device calls, the command lines' parsing, and the argument checks of bd_vb_terms, which run before any launch.

Bound of a value against its float64 reference: max(4e-6 |ref|, 4 d32), the pair of test_kdiff.py; on the host, where the float32
restatement is the thing under test, the first part alone."""
import ctypes
import json
import math
import types

import numpy as np
import pytest
import torch

from tests.golden import cases_vb as CV

LN2 = math.log(2.0)


def sched(**kw):
    from baddiffusion_amd.schedulers import DDPMScheduler
    return DDPMScheduler(**kw)


# ---------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("vt", CV.VARIANCE_TYPES)
def test_tables_agree_with_the_closed_forms(vt):
    from baddiffusion_amd import likelihood
    tab, ref = likelihood.vb_tables(sched(), vt), CV.tables64(vt)
    assert tab["T"] == CV.T and tab["variance_type"] == vt and tab["add64"].shape == tab["mul64"].shape == (CV.T + 1,)
    for got, want in ((tab["add64"], ref["add"]), (tab["mul64"], ref["mul"]), (tab["sigma2"], ref["sigma2"]), (tab["c0"], ref["c0"])):
        np.testing.assert_allclose(got, want.numpy(), rtol=1e-12, atol=1e-300)
    assert tab["add64"][0] == 0.0 and tab["mul64"][0] == 1.0
    if vt == "fixed_small":
        assert not tab["delta"].any() and not tab["add64"][1:CV.T].any()              # Delta == 0: the KL rows are the weighted mse alone
    else:
        assert (tab["delta"][1:] > 0).all() and tab["delta"][0] == 0.0
        np.testing.assert_allclose(tab["add64"][[1, 2]] / LN2, [0.1751, 0.0746], atol=5e-5)
    # c0_0 = beta_0 / (1 - abar_0) = 1 up to the float32 rounding of abar_0 = fl(1 - beta_0): 2^-24 / beta_0
    assert abs(tab["c0"][0] - 1.0) <= 2.0 ** -24 / CV.BETA_START
    assert abs(tab["sigma_dec"] - 0.0073846) < 5e-8 and tab["inv_sigma_dec"] == 1.0 / tab["sigma_dec"]
    assert tab["sigma2"][0] == tab["sigma2"][1] if vt == "fixed_small" else tab["sigma2"][0] < tab["sigma2"][1]
    prior_const = tab["add64"][CV.T] / LN2
    assert 5.85e-10 < prior_const < 5.95e-10 and abs(tab["mul64"][CV.T] - 0.5 * float(CV.schedule()[2][-1])) < 1e-18
    assert likelihood.vb_tables(sched(variance_type="fixed_large"))["variance_type"] == "fixed_large"      # the scheduler's by default
    assert likelihood.vb_tables(sched(), vt) is tab or likelihood.vb_tables(sched(), vt)["T"] == CV.T
    s = sched()
    assert likelihood.vb_tables(s, vt) is likelihood.vb_tables(s, vt)                                  # cached on the scheduler
    dev = likelihood.vb_tables(s, vt, device="cpu")
    assert dev is likelihood.vb_tables(s, vt, device="cpu") and dev["add"].dtype == torch.float32 and dev["add"].shape == (CV.T + 1,)
    assert torch.equal(dev["add"], torch.from_numpy(tab["add64"]).float()) and torch.equal(dev["alphas_cumprod"], CV.schedule()[2])


def test_tables_refuse_other_variances_and_predictions():
    from baddiffusion_amd import likelihood
    for vt in ("learned", "learned_range", "fixed_small_log"):
        with pytest.raises(NotImplementedError, match="variance_type"):
            likelihood.vb_tables(sched(), vt)
    with pytest.raises(ValueError, match="t_stride"):
        likelihood.strided_timesteps(1000, 0)
    assert likelihood.strided_timesteps(10, 4) == (0, 1, 5, 9) and likelihood.strided_timesteps(5, 1) == (0, 1, 2, 3, 4)


# ---------------------------------------------------------------------------------------------------- the contract on known answers
def perfect_rows(t, seed=5, shape=(3, 16, 16)):
    """a perfect model: eps_hat is the noise itself"""
    x0, x_t, _ = CV.make_rows(seed, 1, shape, (t,))
    g = torch.Generator().manual_seed(seed)
    torch.randint(0, 256, (1,) + shape, generator=g)
    noise = CV.exact_randn((1,) + shape, g)                                          # the noise make_rows drew, not a reconstruction
    return x0, x_t, noise


@pytest.mark.parametrize("t", (1, 2, 10))
def test_perfect_model_kl_rows(t):
    """eps_hat = eps: the fixed_large term is (-1 + Delta + exp(-Delta)) / (2 ln 2) and the fixed_small term vanishes, both up to the
    float32 rounding of x0_hat: |x0 - x0_hat| <= 2^-20 max|x_t| / sqrt(abar_t) (x_t, the product and the quotient round once each,
    2^-24 relative apiece, with a factor of 4 to spare), weighted by w_t = c0_t^2 / (2 sigma2_t ln 2)"""
    x0, x_t, eps = perfect_rows(t)
    ab = float(CV.schedule()[2][t])
    for vt in CV.VARIANCE_TYPES:
        tab = CV.tables64(vt)
        slack = float(tab["mul"][t]) / LN2 * (2.0 ** -20 * float(x_t.abs().max()) / math.sqrt(ab)) ** 2
        got = float(CV.kernel_formula(x0, x_t, eps, (t,), vt, False, torch.float64)[0])
        const = float(tab["add"][t]) / LN2
        assert const <= got <= const + slack, (vt, got, const, slack)
        if vt == "fixed_small":
            assert const == 0.0 and got < slack
    assert abs(float(CV.tables64("fixed_large")["add"][1]) / LN2 - 0.1751) < 5e-5


def test_perfect_model_decoder_row():
    """eps_hat = eps at t = 0 on uniform random uint8: every interior pixel has P = erf(h / (sigma sqrt 2)), h = 1/255, the two edge values
    P = erfc(-h / (sigma sqrt 2)) / 2 -- 1.2986 bits for the linear schedule.  Pinned from these two float64 numbers and the sample's own
    edge count; the float32 rounding of x0_hat moves log P by at most |x0 - x0_hat| / sigma_dec * max(phi / P) < |x0 - x0_hat| / sigma_dec."""
    x0, x_t, eps = perfect_rows(0, shape=(3, 32, 32))
    tab = CV.tables64("fixed_small")
    a = (1.0 / 255.0) * tab["inv_sigma_dec"] / math.sqrt(2.0)
    p_in, p_edge = math.erf(a), 0.5 * math.erfc(-a)
    n_edge = int(((x0 < -0.999) | (x0 > 0.999)).sum())
    want = -((x0.numel() - n_edge) * math.log(p_in) + n_edge * math.log(p_edge)) / x0.numel() / LN2
    slack = float((x0 - CV.x0_hat(x_t[0], eps[0], 0, False)).abs().max()) * tab["inv_sigma_dec"] / LN2
    got = float(CV.kernel_formula(x0, x_t, eps, (0,), "fixed_small", True, torch.float64)[0])
    assert abs(got - want) <= slack and slack < 1e-4, (got, want, slack)
    # 1.3054 bits in an interior bin, 0.5098 in an edge bin, which 1/128 of uniform pixels fall into: 1.2992 expected, +-0.0013 per
    # standard deviation of this sample's edge count
    assert abs(got - 1.2992) < 4e-3


def test_prior_row_reads_x0_alone():
    x0, x_t, eps = CV.make_rows(9, 2, (3, 8, 8), (CV.T, CV.T))
    tab = CV.tables64("fixed_small")
    want = (tab["add"][CV.T] + tab["mul"][CV.T] * (x0.double() ** 2).mean((1, 2, 3))) / LN2
    got = CV.kernel_formula(x0, None, None, (CV.T, CV.T), "fixed_large", True, torch.float64)[0]
    assert torch.allclose(got, want, rtol=1e-14, atol=0) and 1e-6 < float(got[0]) < 1e-4


# ---------------------------------------------------------------------------------------------------- number formats
def test_float32_restatement_holds_the_bound_on_every_regime(golden):
    g = golden("vb")
    for name, (x0, x_t, eps, clip) in CV.regime_rows().items():
        ref = g[f"r_{name}_bits"]
        b64 = CV.kernel_formula(x0, x_t, eps, (0,), "fixed_small", clip, torch.float64)[0].numpy()
        b32 = CV.kernel_formula(x0, x_t, eps, (0,), "fixed_small", clip, torch.float32)[0].numpy()
        if name == "nan":
            assert np.isnan(ref).all() and np.isnan(b64).all() and np.isnan(b32).all()
            continue
        assert abs(b64 - ref) <= 1e-12 * abs(ref), name                              # the fixture is this evaluation (up to the host's erfc / log)
        assert abs(b32 - ref) <= 4e-6 * abs(ref), (name, float(b32), float(ref))
        np.testing.assert_allclose(abs(b32 - ref), g[f"r_{name}_d32"], rtol=0.5, atol=1e-9)
    assert float(g["r_floor_bits"][0]) == CV.FLOOR_BITS


def test_textbook_form_in_float32_misses_the_bound():
    """Phi(z+) - Phi(z-) in float32 on the 0.01 * randn regime (1.35 sigma_dec per unit of randn).  Where the prediction is more than
    5.9 sigma_dec off, both Phi round to 1 (1 - Phi(5.4) = 3.3e-8 is below half an ulp of 1) and the pixel lands on the floor, 14 bits above
    its value; that takes |randn| > 4.4, one pixel in 90 000, so the case has 2^20 pixels: about eleven of them, 6e-5 of the mean.  The
    erfc form holds the bound on the same pixels."""
    err = torch.randn(1, 1, 1024, 1024, generator=torch.Generator().manual_seed(8101))     # real Gaussian tails (exact_randn ends at 6)
    x0, x_t, eps = CV.make_rows(8100, 1, (1, 1024, 1024), (0,), s0=0.01, err=err)
    ref = float(CV.kernel_formula(x0, x_t, eps, (0,), "fixed_small", True, torch.float64)[0])
    tail = float(CV.kernel_formula(x0, x_t, eps, (0,), "fixed_small", True, torch.float32)[0])
    naive = float(CV.kernel_formula(x0, x_t, eps, (0,), "fixed_small", True, torch.float32, nll=CV.textbook_nll)[0])
    naive64 = float(CV.kernel_formula(x0, x_t, eps, (0,), "fixed_small", True, torch.float64, nll=CV.textbook_nll)[0])
    print(f"MEASURE t = 0, 0.01 * randn, 2^20 pixels: {ref:.6f} bits; float32 erfc form off by {abs(tail - ref) / ref:.2e}, float32 textbook "
          f"form by {abs(naive - ref) / ref:.2e}, float64 textbook form by {abs(naive64 - ref) / ref:.2e}")
    assert abs(tail - ref) <= 4e-6 * ref
    assert abs(naive - ref) > 4e-6 * ref
    assert abs(naive64 - ref) <= 4e-6 * ref                                          # the same quantity: the form, not the value, is at fault


# ---------------------------------------------------------------------------------------------------- bits_per_dim around stand-ins
class FakeModel:
    """eps_hat = 0.9 x_t + 0.01 t / T on the CPU, recording the batch and the timesteps of every call"""

    def __init__(self, C=3, S=8):
        self.device = torch.device("cpu")
        self.config = types.SimpleNamespace(in_channels=C, sample_size=S)
        self.calls = []

    def __call__(self, x, t, return_dict=True):
        assert not torch.is_grad_enabled()
        self.calls.append(t.clone())
        return (0.9 * x + 0.01 * (t.float() / CV.T).view(-1, 1, 1, 1),)


@pytest.fixture
def stand_ins(monkeypatch):
    """ops.poison_qsample and ops.vb_terms restated on the CPU (the data path's x0, q_sample, kernel_formula in float64)"""
    from baddiffusion_amd import ops
    seen = {"t": []}

    def poison_qsample(images, is_poison, trigger, target_img, noise, timesteps, alphas, alphas_cumprod, row_index=None, want_image=False, **kw):
        assert want_image and not is_poison.any()
        x0 = CV.data_x0(images[row_index]).permute(0, 3, 1, 2).contiguous()
        sa, sb = alphas_cumprod[timesteps].sqrt().view(-1, 1, 1, 1), (1 - alphas_cumprod[timesteps]).sqrt().view(-1, 1, 1, 1)
        x_t = sa * x0 + sb * noise
        return x_t.permute(0, 2, 3, 1).contiguous(), noise.permute(0, 2, 3, 1).contiguous(), x0

    def vb_terms(x0, x_t, eps, t, tables, clip_denoised=True, want_x0_mse=False):
        seen["t"].append(t.clone())
        return CV.kernel_formula(x0, x_t, eps, t.tolist(), tables["variance_type"], clip_denoised, torch.float64)[0].float()

    monkeypatch.setattr(ops, "poison_qsample", poison_qsample)
    monkeypatch.setattr(ops, "vb_terms", vb_terms)
    return seen


def clean_u8(n=5, S=8):
    return torch.randint(0, 256, (n, S, S, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)


def test_bits_per_dim_draws_packs_and_sums(stand_ins):
    from baddiffusion_amd import likelihood, metrics
    assert metrics.bits_per_dim is likelihood.bits_per_dim
    model, s, clean = FakeModel(), sched(), clean_u8()
    ts = (7, 0, 500, 999, 1)
    res = likelihood.bits_per_dim(model, s, clean, n=3, timesteps=ts, generator=torch.Generator().manual_seed(11), max_batch_n=4)
    assert res["timesteps"] == (0, 1, 7, 500, 999) and res["complete"] is False
    assert res["terms"].shape == (6, 3) and res["terms"].dtype == torch.float32 and not res["terms"].is_cuda
    # 15 pairs, largest t first and the images of one t in order, in chunks of 4: a small n still fills the batch
    flat_t = [t for t in (999, 500, 7, 1, 0) for _ in range(3)]
    assert [c.tolist() for c in model.calls] == [flat_t[i: i + 4] for i in range(0, 15, 4)]
    assert [c.tolist() for c in stand_ins["t"]] == [flat_t[i: i + 4] for i in range(0, 15, 4)] + [[CV.T] * 3]
    # the draws: one randn(n, C, S, S) per timestep from the largest t down, nothing else from the generator
    g = torch.Generator().manual_seed(11)
    noises = {t: torch.randn(3, 3, 8, 8, generator=g) for t in (999, 500, 7, 1, 0)}
    x0 = CV.data_x0(clean[:3]).permute(0, 3, 1, 2).contiguous()
    ab = CV.schedule()[2]
    for k, t in enumerate(res["timesteps"]):
        x_t = ab[t].sqrt() * x0 + (1 - ab[t]).sqrt() * noises[t]
        with torch.no_grad():
            eps = model(x_t, torch.full((3,), t), return_dict=False)[0]
        want = CV.kernel_formula(x0, x_t, eps, [t] * 3, "fixed_small", True, torch.float64)[0].float()
        assert torch.equal(res["terms"][k], want), t
    assert torch.equal(res["terms"][5], CV.kernel_formula(x0, None, None, [CV.T] * 3, "fixed_small", True, torch.float64)[0].float())
    assert torch.equal(res["sum_bpd"], res["terms"].double().sum(0)) and res["mean_bpd"] == float(res["sum_bpd"].mean())
    # the same noise handed in (mapping, or a sequence aligned with the ascending timesteps), other rows, another chunk size: equal terms
    for kw in (dict(noises=noises), dict(noises=[noises[t] for t in res["timesteps"]])):
        again = likelihood.bits_per_dim(model, s, clean, rows=[0, 1, 2], timesteps=ts, max_batch_n=256, **kw)
        assert torch.equal(again["terms"], res["terms"])
    swapped = likelihood.bits_per_dim(model, s, clean, rows=[2, 0, 4], timesteps=ts, noises={t: z[[2, 0, 1]] for t, z in noises.items()})
    assert torch.equal(swapped["terms"][:, :2], res["terms"][:, [2, 0]]) and not torch.equal(swapped["terms"][:, 2], res["terms"][:, 1])
    large = likelihood.bits_per_dim(model, s, clean, n=3, timesteps=ts, noises=noises, variance_type="fixed_large", clip_denoised=False)
    assert (large["terms"][1:5] > res["terms"][1:5] - 1e-6).any() and not torch.equal(large["terms"], res["terms"])


def test_bits_per_dim_complete_and_estimate(stand_ins):
    from baddiffusion_amd import likelihood
    model, clean, s = FakeModel(), clean_u8(), sched()
    terms = torch.arange(1, 7, dtype=torch.float32).view(6, 1).repeat(1, 2)          # L_0 = 1, three KL rows 2, 3, 4 ... prior 6
    assert likelihood.estimate_bpd(terms, 1).tolist() == [21.0, 21.0] and likelihood.estimate_bpd(terms, 10).tolist() == [1 + 6 + 10 * 14.0] * 2
    res = likelihood.bits_per_dim(model, s, clean, n=2, timesteps=likelihood.strided_timesteps(CV.T, 250), generator=torch.Generator().manual_seed(1))
    assert res["timesteps"] == (0, 1, 251, 501, 751) and not res["complete"]
    est = likelihood.estimate_bpd(res["terms"], 250)
    assert torch.allclose(est, res["terms"][-1].double() + res["terms"][0].double() + 250 * res["terms"][1:-1].double().sum(0))
    for bad, pat in ((dict(timesteps=(0, 0)), "distinct"), (dict(timesteps=(CV.T,)), "distinct values in"), (dict(rows=[9]), "indices into"),
                     (dict(n=2, rows=[0]), "rows hold"), (dict(n=2, max_batch_n=0), "max_batch_n"),
                     (dict(n=2, timesteps=(0, 1), noises=[torch.zeros(2, 3, 8, 8)]), "noises for"),
                     (dict(n=2, timesteps=(0,), noises=[torch.zeros(1, 3, 8, 8)]), "expected")):
        with pytest.raises(ValueError, match=pat):
            likelihood.bits_per_dim(model, s, clean, **bad)
    with pytest.raises(TypeError, match="uint8"):
        likelihood.bits_per_dim(model, s, clean.float(), n=2)


def test_bits_per_dim_all_timesteps_is_complete(stand_ins):
    from baddiffusion_amd import likelihood
    s = sched(num_train_timesteps=1000)
    model = FakeModel(S=2)
    clean = clean_u8(2, S=2)
    res = likelihood.bits_per_dim(model, s, clean, generator=torch.Generator().manual_seed(1), max_batch_n=500)
    assert res["complete"] is True and res["terms"].shape == (1001, 2) and len(model.calls) == 4 and res["timesteps"] == tuple(range(1000))
    assert torch.equal(likelihood.estimate_bpd(res["terms"], 1), res["sum_bpd"])
    assert bool(torch.isfinite(res["terms"]).all()) and res["mean_bpd"] > 0


# ---------------------------------------------------------------------------------------------------- command lines
def test_likelihood_eval_command_line(tmp_path, capsys):
    import likelihood_eval as LE
    c = LE.get_config(["--ckpt", "/x/ckpt_a/", "--n", "4", "--t_stride", "50", "--no_clip", "--variance_type", "fixed_large", "--target", "HAT",
                       "--output_dir", str(tmp_path)])
    assert (c.n, c.t_stride, c.clip, c.variance_type, c.target, c.batch, c.seed) == (4, 50, False, "fixed_large", "HAT", 256, 0)
    assert c.output_dir == str(tmp_path / "res_likelihood_n4_k50_ckpt_a")
    saved = json.load(open(tmp_path / "res_likelihood_n4_k50_ckpt_a" / "config.json"))
    assert saved["t_stride"] == 50 and saved["clip"] is False and "no_clip" not in saved
    d = LE.get_config(["--ckpt", "c", "--output_dir", str(tmp_path)])
    assert (d.n, d.t_stride, d.clip, d.variance_type, d.target) == (16, 1, True, None, None)
    for bad in (["--t_stride", "0"], ["--n", "0"], ["--batch", "-1"], ["--variance_type", "learned"], []):
        with pytest.raises(SystemExit):
            LE.get_config((["--ckpt", "c"] if bad else []) + bad + ["--output_dir", str(tmp_path)])
    capsys.readouterr()
    # the summary of a strided result with a target row
    res = {"terms": torch.tensor([[1.0, 3.0, 9.0], [0.5, 0.5, 2.0], [0.25, 0.25, 1.0]]), "timesteps": (0, 1), "complete": False,
           "sum_bpd": torch.tensor([1.75, 3.75, 12.0], dtype=torch.float64)}
    out = LE.summarise(c, res, 2)
    assert out["complete"] is False and "mean_bpd" not in out and out["n"] == 2 and out["timesteps"] == 2
    assert out["per_image"] == [1 + 0.25 + 50 * 0.5, 3 + 0.25 + 50 * 0.5] and out["estimate_bpd"] == 27.25 and out["target_bpd"] == 9 + 1 + 100.0
    assert (out["prior_bpd"], out["l0_bpd"]) == (0.25, 2.0)


def test_elijah_defense_bpd_flags(tmp_path, capsys):
    import elijah_defense as E
    base = ["--ckpt", "c", "--output_dir", str(tmp_path)]
    c = E.get_config(base + ["--bpd_images", "8", "--bpd_t_stride", "100"])
    assert (c.bpd_images, c.bpd_t_stride) == (8, 100)
    name = E.naming_fn(c)
    saved = json.load(open(tmp_path / name / "config.json"))
    assert saved["bpd_images"] == 8 and saved["bpd_t_stride"] == 100
    assert E.get_config(base + ["--bpd_images", "8"]).bpd_t_stride == 1
    plain = E.get_config(base)
    assert plain.bpd_images is None
    saved = json.load(open(tmp_path / name / "config.json"))
    assert not any(k.startswith("bpd") for k in saved) and "dyn_threshold_ratio" in saved      # without the flag: the file of before
    for bad in (["--bpd_t_stride", "5"], ["--bpd_images", "0"], ["--bpd_images", "4", "--bpd_t_stride", "0"]):
        with pytest.raises(SystemExit):
            E.get_config(base + bad)
    assert "--bpd_t_stride needs --bpd_images" in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------- ABI
def _desc(L, p, ts, **kw):
    d = L.VbTermsDesc(N=len(ts), C=3, H=4, W=4, x0=p, x_t=p, eps=p, t=p, t_host=ctypes.addressof(ts), alphas_cumprod=p, T=1000,
                      term_add=p, term_mul=p, inv_sigma_dec=135.0, clip_denoised=1, bits=p, x0_mse=None)
    for i, s in enumerate((48, 16, 4, 1)):
        d.x0_stride[i] = d.xt_stride[i] = d.eps_stride[i] = s
    for k, v in kw.items():
        if k.endswith("_stride"):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


def test_vb_terms_refuses_bad_arguments_before_any_launch():
    """every call below returns before a launch: the pointers are a never-dereferenced address, and this machine has no device"""
    from baddiffusion_amd import _lib as L
    lib = L.load()
    assert lib.bd_vb_terms(None, None, 0, None) < 0 and b"bd_vb_terms: null descriptor" in lib.bd_last_error()
    p = 4096
    ts = (ctypes.c_int64 * 3)(0, 500, 1000)
    call = lambda d, ws=None, n=0: lib.bd_vb_terms(ctypes.byref(d), ws, n, None)
    err = lambda: lib.bd_last_error().decode()
    for field in ("x0", "t", "t_host", "alphas_cumprod", "term_add", "term_mul", "bits"):
        assert call(_desc(L, p, ts, **{field: None})) < 0 and "bd_vb_terms: null pointer" in err(), field
    for field in ("x_t", "eps"):
        assert call(_desc(L, p, ts, **{field: None})) < 0 and "null x_t or eps with a row at t < T" in err(), field
    for bad in (-1, 1001, 2 ** 40):
        t_bad = (ctypes.c_int64 * 3)(0, bad, 1000)
        assert call(_desc(L, p, t_bad)) < 0 and f"t[1]={bad} outside [0, 1000]" in err()
    for field in ("x0_stride", "xt_stride", "eps_stride"):
        assert call(_desc(L, p, ts, **{field: (2, -4)})) < 0 and "negative stride" in err(), field
    for kw, pat in ((dict(N=0), "must be positive"), (dict(C=0), "must be positive"), (dict(T=0), "T=0 must be positive"),
                    (dict(inv_sigma_dec=0.0), "inv_sigma_dec"), (dict(inv_sigma_dec=float("nan")), "inv_sigma_dec"),
                    (dict(inv_sigma_dec=float("inf")), "inv_sigma_dec")):
        assert call(_desc(L, p, ts, **kw)) < 0 and pat in err(), kw
    big = _desc(L, p, ts, C=8, H=16384, W=16384)
    assert call(big) < 0 and "does not fit 31 bits" in err()
    chunks = _desc(L, p, ts, C=3, H=64, W=64)                                          # 12288 elements: two chunks, two partial arrays
    need = lib.bd_vb_terms_workspace_bytes(3, 3, 64, 64)
    assert need == 2 * 3 * 2 * 8 and call(chunks, None, 0) < 0 and f"workspace 0 < {need}" in err()
    assert call(chunks, p, need - 1) < 0 and "workspace" in err()
    assert lib.bd_vb_terms_workspace_bytes(2048, 3, 32, 32) == 0 and lib.bd_vb_terms_workspace_bytes(0, 3, 32, 32) == 0
    assert lib.bd_vb_terms_workspace_bytes(4, 3, 256, 256) == 2 * lib.bd_image_loss_workspace_bytes(4, 3, 256, 256) == 2 * 4 * 24 * 8
    assert ctypes.sizeof(L.VbTermsDesc) == _c_sizeof("bd_vb_terms_desc")


def _c_sizeof(name):
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(f'#include <stdio.h>\n#include "bd_hip.h"\nint main(){{printf("%zu", sizeof({name}));return 0;}}')
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), c, "-o", os.path.join(d, "s")])
        return int(subprocess.run([os.path.join(d, "s")], capture_output=True, text=True).stdout)
