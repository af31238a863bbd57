"""CPU: the host side of the bound along the backdoored chain -- likelihood.vb_tables(shift=True) against both forms of d_t / c0_t, the
derivation (the two forms of d_t, the identity with the reference's training target, the marginal, the prior) in float64, the float64 /
float32 restatement (tests/golden/cases_vb_shift.py) against the fixture, the bookkeeping of likelihood.bits_per_dim(backdoor=...) around
stand-ins, the flag rules of both command lines, and the argument checks of bd_vb_terms_shift, which run before any launch.

Two schedules appear.  The TABLES are the scheduler's float32 beta_t, alpha_t, abar_t taken to float64: what vb_tables, the kernel and the
fixture use.  They satisfy alpha_t = 1 - beta_t and abar_t = alpha_t abar_{t-1} only up to their own float32 rounding (2^-25 each), and
the two forms of d_t and the identity are equalities exactly when those two relations hold.  So the derivation is checked on the EXACT
schedule -- the same float32 betas, alpha_t = 1 - beta_t and the cumulative product formed in float64 -- at the bounds the derivation was
measured against (1e-14, 1e-9 max(1, |g_t|)), and the table is checked against the float32 tables' own rounding."""
import ctypes
import json
import math
import types

import numpy as np
import pytest
import torch

from tests.golden import cases_vb as CV
from tests.golden import cases_vb_shift as CS

LN2, T = math.log(2.0), CV.T
TS_IDENTITY = (0, 1, 2, 10, 250, 500, T - 2, T - 1)


def sched(**kw):
    from baddiffusion_amd.schedulers import DDPMScheduler
    return DDPMScheduler(**kw)


def forms(b, al, ab):
    """rho, rho_{t-1}, c0, ct, both forms of d and R_coef, float64 [T], from a schedule's float64 beta, alpha, abar"""
    abp = np.concatenate(([1.0], ab[:-1]))
    rho = 1.0 - np.sqrt(ab)
    rhop = np.concatenate(([0.0], rho[:-1]))
    c0 = np.sqrt(abp) * b / (1.0 - ab)
    ct = np.sqrt(al) * (1.0 - abp) / (1.0 - ab)
    d1 = rhop - ct * rho
    k = rho - np.sqrt(al) * rhop
    btilde = b * (1.0 - abp) / (1.0 - ab)
    d2 = np.zeros_like(d1)                                                          # (t = 0: rho_{-1} / (1 - abar_{-1}) is 0 / 0; d_0 = 0)
    d2[1:] = btilde[1:] * (rhop[1:] / (1.0 - abp[1:]) - np.sqrt(al[1:]) * k[1:] / b[1:])
    r_coef = (1.0 - np.sqrt(al)) * np.sqrt(1.0 - ab) / (1.0 - al)
    return types.SimpleNamespace(ab=ab, abp=abp, rho=rho, rhop=rhop, c0=c0, ct=ct, d1=d1, d2=d2, r_coef=r_coef)


def table_schedule():
    return forms(*(v.double().numpy() for v in CV.schedule()))


def exact_schedule():
    b = CV.schedule()[0].double().numpy()
    return forms(b, 1.0 - b, np.cumprod(1.0 - b))


# ---------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("vt", CV.VARIANCE_TYPES)
def test_shift_table_against_both_forms(vt):
    from baddiffusion_amd import likelihood
    s = sched()
    plain = likelihood.vb_tables(s, vt)
    tab = likelihood.vb_tables(s, vt, shift=True)
    assert "shift64" not in plain and likelihood.vb_tables(s, vt) is plain and likelihood.vb_tables(s, vt, shift=True) is tab
    for k in plain:                                                                  # add, mul and the rest: the same objects
        assert tab[k] is plain[k], k
    ref = CV.tables64(vt)
    np.testing.assert_allclose(tab["add64"], ref["add"].numpy(), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(tab["mul64"], ref["mul"].numpy(), rtol=1e-12, atol=1e-300)
    g = tab["shift64"]
    assert g.shape == (T + 1,) and g.dtype == np.float64 and g[0] == 0.0 and g[T] == -1.0
    assert 2.7e-9 < g[1] < 2.8e-9 and 77.2 < g[T - 1] < 77.4 and (np.diff(g[:T]) > 0).all()
    f = table_schedule()
    np.testing.assert_allclose(g[1:T], (f.d1 / f.c0)[1:], rtol=1e-12, atol=0)        # the first form, as stated
    np.testing.assert_allclose(g, CS.shift64().numpy(), rtol=1e-12, atol=0)          # and the fixture module's restatement of it
    # the second form on the float32 tables: d1 - d2 = rho_{t-1} delta_t / (1 - abar_t) identically, with the tables' own inconsistency
    # delta_t = (1 - beta_t - alpha_t) + (alpha_t abar_{t-1} - abar_t): two float32 roundings of numbers below 1 (2^-25 apiece when the
    # cumulative product is formed entry by entry; a few of them are allowed for a library that forms it otherwise)
    b, al, _ = (v.double().numpy() for v in CV.schedule())
    delta = (1.0 - b - al) + (al * f.abp - f.ab)
    assert np.abs(delta).max() <= 4 * 2.0 ** -24
    dev = (g[1:T] - (f.d2 / f.c0)[1:]) - (f.rhop * delta / (1.0 - f.ab) / f.c0)[1:]
    print(f"MEASURE shift table ({vt}) vs the second form of d_t / c0_t on the float32 tables: max |delta_t| {np.abs(delta).max() * 2 ** 24:.2f} "
          f"* 2^-24, worst |g - d2 / c0| {np.abs(g[1:T] - (f.d2 / f.c0)[1:]).max():.2e}, residue beyond rho delta / ((1 - abar) c0) "
          f"{np.abs(dev).max():.2e}")
    assert (np.abs(dev) <= 1e-9 * np.maximum(1.0, g[1:T])).all()
    # against the exact schedule: the float32 cumulative product has gathered up to t roundings by entry t, 1000 * 2^-25 = 3e-5 of abar_t,
    # and g_t is about as sensitive as abar_t^(-1/2); the smallest entries sit on the absolute floor rho delta / ((1 - abar) c0) < 1e-7
    e = exact_schedule()
    for form in (e.d1, e.d2):
        assert (np.abs(g[1:T] - (form / e.c0)[1:]) <= 1e-4 * g[1:T] + 1e-7).all()
    dev_tab = likelihood.vb_tables(s, vt, device="cpu", shift=True)
    assert dev_tab is likelihood.vb_tables(s, vt, device="cpu", shift=True) and dev_tab["shift64"] is g
    assert dev_tab["shift"].dtype == torch.float32 and torch.equal(dev_tab["shift"], torch.from_numpy(g).float())
    assert dev_tab["add"] is likelihood.vb_tables(s, vt, device="cpu")["add"] and "shift" not in likelihood.vb_tables(s, vt, device="cpu")


def test_two_forms_of_d_agree():
    """1e-14 absolute over all t >= 1 on the exact schedule (3.5e-16 was measured when the derivation was written)"""
    e = exact_schedule()
    dev = np.abs(e.d1 - e.d2)[1:]
    print(f"MEASURE two forms of d_t on the exact float64 schedule: worst |d1 - d2| {dev.max():.2e}")
    assert dev.max() <= 1e-14 and e.d1[0] == 0.0


@pytest.mark.parametrize("t", TS_IDENTITY)
def test_training_target_is_the_optimum_and_the_marginal_is_kept(t):
    """eps_hat = eps + R_coef_t r, the target of the reference's q_sample_diffuser, unclamped: x0 + g_t r - x0_hat vanishes up to
    1e-9 max(1, |g_t|) (7.7e-13 was measured at t = T-1, where |x0_hat| is about 77).  And the posterior mean at x_t = E[x_t] is
    E[x_{t-1}] = sqrt(abar_{t-1}) x0 + rho_{t-1} r: each coefficient carries the rounding of 1 - abar_t, a difference of numbers near 1,
    2^-53 / (1 - abar_t) relative, and there are three of them with a handful of operations each: 16 * 2^-52 / (1 - abar_t)."""
    e = exact_schedule()
    g = np.concatenate(([0.0], (e.d1 / e.c0)[1:]))
    rng = np.random.default_rng(100 + t)
    x0, r, eps = rng.uniform(-1, 1, 4096), rng.uniform(-1, 1, 4096), rng.standard_normal(4096)
    sa, sb = math.sqrt(e.ab[t]), math.sqrt(1.0 - e.ab[t])
    x_t = sa * x0 + e.rho[t] * r + sb * eps
    x0_hat = (x_t - sb * (eps + e.r_coef[t] * r)) / sa
    dev = float(np.abs(x0 + g[t] * r - x0_hat).max())
    print(f"MEASURE identity at t = {t}: |x0 + g_t r - x0_hat| <= {dev:.2e}, g_t = {g[t]:.6g}, max |x0_hat| = {np.abs(x0_hat).max():.3g}")
    assert dev <= 1e-9 * max(1.0, abs(g[t]))
    mean = e.c0[t] * x0 + e.ct[t] * (sa * x0 + e.rho[t] * r) + e.d1[t] * r
    want = math.sqrt(e.abp[t]) * x0 + e.rhop[t] * r
    assert float(np.abs(mean - want).max()) <= 16 * 2.0 ** -52 / (1.0 - e.ab[t])


@pytest.mark.parametrize("vt", CV.VARIANCE_TYPES)
def test_prior_closed_form_is_the_kl_of_two_gaussians(vt):
    """KL(N(sqrt(abar) x0 + rho r, (1 - abar) I) || N(r, I)) written out per dimension against add[T] + mul[T] mean (x0 - r)^2 and against
    the restatement's prior row"""
    from baddiffusion_amd import likelihood
    tab = likelihood.vb_tables(sched(), vt, shift=True)
    ab = float(CV.schedule()[2][-1])
    x0, _, _, r = CS.make_rows(11, 2, (3, 8, 8), (T, T))
    mu1 = math.sqrt(ab) * x0.double() + (1.0 - math.sqrt(ab)) * r.double()
    var1 = 1.0 - ab
    kl = 0.5 * (-math.log(var1) - 1.0 + var1 + (mu1 - r.double()) ** 2)              # log(s2^2 / s1^2) + (s1^2 + (mu1 - mu2)^2) / s2^2 - 1, halved
    direct = kl.mean((1, 2, 3)) / LN2
    closed = (tab["add64"][T] + tab["mul64"][T] * ((x0.double() - r.double()) ** 2).mean((1, 2, 3))) / LN2
    got = CS.kernel_formula(x0, None, None, r, (T, T), vt, True, torch.float64)[0]
    # (mu1 - r forms sqrt(abar) (x0 - r), about 0.006 |x0 - r|, as a difference of numbers of order 1: 1e-13 relative, squared)
    assert torch.allclose(direct, closed, rtol=1e-10, atol=0) and torch.allclose(got, closed, rtol=1e-14, atol=0)
    one = CS.kernel_formula(x0, None, None, r[0], (T, T), vt, True, torch.float64)[0]                  # one image for every row
    assert one[0] == got[0] and one[1] != got[1]


# ---------------------------------------------------------------------------------------------------- restatement and fixture
def test_restatement_reproduces_the_fixture(golden):
    g = golden("vb_shift")
    n = 0
    for tag, shape, N, ts, vt, clip, seed in CS.kernel_cases():
        x0, x_t, eps, r = CS.make_rows(seed, N, shape, ts)
        for dtype, (kb, km) in ((torch.float64, (1e-12, 1e-12)), (torch.float32, (None, None))):
            b, m = (v.numpy() for v in CS.kernel_formula(x0, x_t, eps, r, ts, vt, clip, dtype))
            for got, ref, d32 in ((b, g[f"k_{tag}_bits"], g[f"k_{tag}_d32"]), (m, g[f"k_{tag}_mse"], g[f"k_{tag}_mse_d32"])):
                if dtype == torch.float64:
                    assert (np.abs(got - ref) <= 1e-12 * np.abs(ref)).all(), tag     # the fixture is this evaluation (up to the host's erfc / log)
                else:                                                                # and d32 this distance
                    assert (np.abs(np.abs(got - ref) - d32) <= 0.5 * d32 + 4e-6 * np.abs(ref)).all(), (tag, got, ref, d32)
        n += 1
    assert n == len(CV.SHAPES) * len(CV.NS) * 4
    # with r = 0 the restatement is cases_vb's on the same rows; at t = 0 for any r
    x0, x_t, eps, r = CS.make_rows(77, 6, (3, 5, 17), CV.TS_MIX)
    for dtype in (torch.float64, torch.float32):
        a = CS.kernel_formula(x0, x_t, eps, torch.zeros_like(r), CV.TS_MIX, "fixed_large", True, dtype)
        b = CV.kernel_formula(x0, x_t, eps, CV.TS_MIX, "fixed_large", True, dtype)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        c = CS.kernel_formula(x0, x_t, eps, r, CV.TS_MIX, "fixed_large", True, dtype)
        assert c[0][0] == b[0][0] and not torch.equal(c[0][1:], b[0][1:])


def test_reference_training_target_pays_the_constant_alone(golden):
    """the fixture's rows of the reference's own q_sample_diffuser target fed back as eps_hat, unclamped: the fixed_small KL rows vanish
    and the fixed_large ones are add[t] / ln 2, up to the float32 rounding of x0_hat -- the bound of test_vb_host's perfect model with one
    more doubling for the shift's two more roundings in x_t and in the target: |x0 + g_t r - x0_hat| <= 2^-19 max|x_t| / sqrt(abar_t)"""
    g = golden("vb_shift")
    x_t = g["e2e_x_t"]
    for vt in CV.VARIANCE_TYPES:
        tab = CV.tables64(vt)
        rows = g[f"e2e_tt_{vt}"]
        assert rows.shape == (len(CV.E2E_TS), CV.E2E_N)
        for k, t in enumerate(CV.E2E_TS):
            if t == 0:
                assert (rows[k] > 0.5).all()                                         # the decoder term of a perfect model: about 1.3 bits
                continue
            const = float(tab["add"][t]) / LN2
            slack = float(tab["mul"][t]) / LN2 * (2.0 ** -19 * float(np.abs(x_t[k]).max()) / math.sqrt(float(CV.schedule()[2][t]))) ** 2
            print(f"MEASURE reference training target as eps_hat, {vt}, t = {t}: {float((rows[k] - const).max()):.2e} bits above the "
                  f"constant {const:.4g} (slack {slack:.2e})")
            assert (rows[k] >= const).all() and (rows[k] <= const + slack).all(), (vt, t)


# ---------------------------------------------------------------------------------------------------- bits_per_dim around stand-ins
class FakeModel:
    def __init__(self, C=3, S=8):
        self.device = torch.device("cpu")
        self.config = types.SimpleNamespace(in_channels=C, sample_size=S)
        self.calls = []

    def __call__(self, x, t, return_dict=True):
        assert not torch.is_grad_enabled()
        self.calls.append(t.clone())
        return (0.9 * x + 0.01 * (t.float() / T).view(-1, 1, 1, 1),)


def blend(x, trigger, vmin=-1.0):
    m = torch.where(trigger > vmin, torch.zeros_like(trigger), torch.ones_like(trigger))
    return m * x + (1.0 - m) * trigger


def test_bits_per_dim_backdoor_bookkeeping(monkeypatch):
    """poisoned rows through one poison_qsample call per chunk, the terms from vb_terms_shift, the prior from x0 and r; the noise order, the
    chunks and the returned entries of the plain path"""
    from baddiffusion_amd import likelihood, ops
    seen = {"t": [], "plain": 0}

    def poison_qsample(images, is_poison, trigger, target_img, noise, timesteps, alphas, alphas_cumprod, vmin=-1.0, want_batch=False,
                       row_index=None, want_image=False, **kw):
        assert want_batch and not want_image and bool(is_poison.all()) and is_poison.numel() == row_index.numel()
        x = CV.data_x0(images[row_index]).permute(0, 3, 1, 2).contiguous()
        R = blend(x, trigger, vmin)
        x0 = target_img[None].expand_as(x).contiguous()
        sa, sb = alphas_cumprod[timesteps].sqrt().view(-1, 1, 1, 1), (1 - alphas_cumprod[timesteps]).sqrt().view(-1, 1, 1, 1)
        x_t = sa * x0 + sb * noise + (1 - sa) * R
        return x_t.permute(0, 2, 3, 1).contiguous(), noise.permute(0, 2, 3, 1).contiguous(), R, x0

    def vb_terms_shift(x0, x_t, eps, r, t, tables, clip_denoised=True, want_x0_mse=False):
        assert "shift" in tables
        seen["t"].append(t.clone())
        return CS.kernel_formula(x0, x_t, eps, r, t.tolist(), tables["variance_type"], clip_denoised, torch.float64)[0].float()

    def vb_terms(*a, **k):
        seen["plain"] += 1
        raise AssertionError("the plain kernel on the backdoored path")

    monkeypatch.setattr(ops, "poison_qsample", poison_qsample)
    monkeypatch.setattr(ops, "vb_terms_shift", vb_terms_shift)
    monkeypatch.setattr(ops, "vb_terms", vb_terms)
    model, s = FakeModel(), sched()
    clean = torch.randint(0, 256, (5, 8, 8, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    trigger = torch.full((3, 8, 8), -1.0)
    trigger[:, 5:7, 5:7] = 0.5
    target = CV.data_x0(torch.randint(0, 256, (3, 8, 8), generator=torch.Generator().manual_seed(4)))
    ts = (7, 0, 500, 999, 1)
    res = likelihood.bits_per_dim(model, s, clean, n=3, timesteps=ts, generator=torch.Generator().manual_seed(11), max_batch_n=4,
                                  backdoor=(trigger, target))
    assert res["backdoor"] is True and res["timesteps"] == (0, 1, 7, 500, 999) and res["complete"] is False and res["terms"].shape == (6, 3)
    flat_t = [t for t in (999, 500, 7, 1, 0) for _ in range(3)]
    assert [c.tolist() for c in model.calls] == [flat_t[i: i + 4] for i in range(0, 15, 4)]
    assert [c.tolist() for c in seen["t"]] == [flat_t[i: i + 4] for i in range(0, 15, 4)] + [[T] * 3]
    g = torch.Generator().manual_seed(11)
    noises = {t: torch.randn(3, 3, 8, 8, generator=g) for t in (999, 500, 7, 1, 0)}
    R = blend(CV.data_x0(clean[:3]).permute(0, 3, 1, 2).contiguous(), trigger)
    x0 = target[None].repeat(3, 1, 1, 1)
    ab = CV.schedule()[2]
    for k, t in enumerate(res["timesteps"]):
        x_t = ab[t].sqrt() * x0 + (1 - ab[t]).sqrt() * noises[t] + (1 - ab[t].sqrt()) * R
        with torch.no_grad():
            eps = model(x_t, torch.full((3,), t), return_dict=False)[0]
        want = CS.kernel_formula(x0, x_t, eps, R, [t] * 3, "fixed_small", True, torch.float64)[0].float()
        assert torch.equal(res["terms"][k], want), t
    assert torch.equal(res["terms"][5], CS.kernel_formula(x0, None, None, R, [T] * 3, "fixed_small", True, torch.float64)[0].float())
    assert torch.equal(res["sum_bpd"], res["terms"].double().sum(0)) and res["mean_bpd"] == float(res["sum_bpd"].mean())
    again = likelihood.bits_per_dim(model, s, clean, rows=[0, 1, 2], timesteps=ts, noises=noises, max_batch_n=256,
                                    backdoor={"trigger": trigger, "target": target, "vmin": -1.0})
    assert torch.equal(again["terms"], res["terms"])
    for bad, pat in (((trigger,), "backdoor must be"), ({"trigger": trigger}, "backdoor must be"), ((trigger[:, :4], target), "must both be")):
        with pytest.raises(ValueError, match=pat):
            likelihood.bits_per_dim(model, s, clean, n=2, timesteps=(0,), backdoor=bad)
    assert seen["plain"] == 0


# ---------------------------------------------------------------------------------------------------- command lines
LE_CONFIG_KEYS = ["ckpt", "dataset", "dataset_path", "n", "batch", "t_stride", "variance_type", "clip", "target", "trigger", "output_dir",
                  "score_file", "terms_file", "seed", "gpu"]                         # config.json before --backdoor existed, in its order


def test_likelihood_eval_backdoor_flag(tmp_path, capsys):
    import likelihood_eval as LE
    base = ["--ckpt", "/x/ckpt_a/", "--n", "4", "--t_stride", "50", "--output_dir", str(tmp_path)]
    c = LE.get_config(base + ["--target", "HAT", "--backdoor"])
    assert c.backdoor is True and c.target == "HAT" and c.trigger == "BOX_14"
    path = tmp_path / "res_likelihood_n4_k50_ckpt_a" / "config.json"
    assert json.load(open(path))["backdoor"] is True
    plain = LE.get_config(base + ["--target", "HAT"])
    assert plain.backdoor is False
    text = open(path).read()
    saved = json.loads(text)
    assert list(saved) == LE_CONFIG_KEYS                                             # without the flag: the file of before, key for key
    assert text == json.dumps({k: getattr(plain, k) for k in LE_CONFIG_KEYS}, indent=2, default=str)
    with pytest.raises(SystemExit):
        LE.get_config(base + ["--backdoor"])
    assert "--backdoor needs --target" in capsys.readouterr().err
    # the summary blocks: the plain one is untouched, the backdoor block carries its own keys
    res = {"terms": torch.tensor([[1.0, 3.0], [0.5, 0.5], [0.25, 0.25]]), "timesteps": (0, 1), "complete": False,
           "sum_bpd": torch.tensor([1.75, 3.75], dtype=torch.float64), "backdoor": True}
    assert set(LE.summarise(plain, res, 2)) == {"complete", "t_stride", "timesteps", "n", "estimate_bpd", "per_image", "prior_bpd", "l0_bpd"}
    b = LE.summarise_backdoor(c, res)
    assert set(b) == {"estimate_bpd", "per_image", "prior_bpd", "l0_bpd", "clip_denoised"} and b["clip_denoised"] is True
    assert b["per_image"] == [1 + 0.25 + 50 * 0.5, 3 + 0.25 + 50 * 0.5] and b["estimate_bpd"] == 27.25 and (b["prior_bpd"], b["l0_bpd"]) == (0.25, 2.0)
    full = LE.summarise_backdoor(LE.get_config(["--ckpt", "c", "--no_clip", "--target", "CAT", "--backdoor", "--output_dir", str(tmp_path)]),
                                 dict(res, complete=True))
    assert full["mean_bpd"] == 2.75 and full["clip_denoised"] is False


def test_elijah_defense_bpd_backdoor_flag(tmp_path, capsys):
    import elijah_defense as E
    base = ["--ckpt", "c", "--output_dir", str(tmp_path)]
    c = E.get_config(base + ["--bpd_images", "8", "--target", "CAT", "--bpd_backdoor"])
    assert c.bpd_backdoor is True and c.bpd_images == 8 and c.target == "CAT"
    path = tmp_path / E.naming_fn(c) / "config.json"
    with_flag = json.load(open(path))
    assert with_flag["bpd_backdoor"] is True
    E.get_config(base + ["--bpd_images", "8", "--target", "CAT"])
    without = json.load(open(path))
    assert "bpd_backdoor" not in without and [k for k in without if k.startswith("bpd")] == ["bpd_images", "bpd_t_stride"]
    assert list(without) == [k for k in with_flag if k != "bpd_backdoor"]
    E.get_config(base)
    assert not any(k.startswith("bpd") for k in json.load(open(path)))
    capsys.readouterr()
    for bad in (["--bpd_backdoor"], ["--bpd_backdoor", "--bpd_images", "4"], ["--bpd_backdoor", "--target", "CAT"]):
        with pytest.raises(SystemExit):
            E.get_config(base + bad)
        assert "--bpd_backdoor needs --bpd_images" in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------- ABI
def _desc(L, p, ts, **kw):
    d = L.VbTermsShiftDesc(N=len(ts), C=3, H=4, W=4, x0=p, x_t=p, eps=p, t=p, t_host=ctypes.addressof(ts), alphas_cumprod=p, T=1000,
                           term_add=p, term_mul=p, inv_sigma_dec=135.0, clip_denoised=1, bits=p, x0_mse=None, r=p, term_shift=p)
    for i, s in enumerate((48, 16, 4, 1)):
        d.x0_stride[i] = d.xt_stride[i] = d.eps_stride[i] = d.r_stride[i] = s
    for k, v in kw.items():
        if k.endswith("_stride"):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


def test_vb_terms_shift_refuses_bad_arguments_before_any_launch():
    """every call below returns before a launch: the pointers are a never-dereferenced address, and this machine has no device"""
    from baddiffusion_amd import _lib as L
    from tests.test_vb_host import _c_sizeof
    lib = L.load()
    who = "bd_vb_terms_shift"
    assert lib.bd_vb_terms_shift(None, None, 0, None) < 0 and f"{who}: null descriptor".encode() in lib.bd_last_error()
    p = 4096
    ts = (ctypes.c_int64 * 3)(0, 500, 1000)
    call = lambda d, ws=None, n=0: lib.bd_vb_terms_shift(ctypes.byref(d), ws, n, None)
    err = lambda: lib.bd_last_error().decode()
    for field in ("r", "term_shift"):
        assert call(_desc(L, p, ts, **{field: None})) < 0 and f"{who}: null r or term_shift" in err(), field
    assert call(_desc(L, p, ts, r_stride=(0, -1))) < 0 and f"{who}: negative stride (r -1 at dim 0)" in err()
    # everything bd_vb_terms refuses, under this entry's name
    for field in ("x0", "t", "t_host", "alphas_cumprod", "term_add", "term_mul", "bits"):
        assert call(_desc(L, p, ts, **{field: None})) < 0 and f"{who}: null pointer" in err(), field
    for field in ("x_t", "eps"):
        assert call(_desc(L, p, ts, **{field: None})) < 0 and f"{who}: null x_t or eps with a row at t < T" in err(), field
    for bad in (-1, 1001, 2 ** 40):
        t_bad = (ctypes.c_int64 * 3)(0, bad, 1000)
        assert call(_desc(L, p, t_bad)) < 0 and f"{who}: t[1]={bad} outside [0, 1000]" in err()
    for field in ("x0_stride", "xt_stride", "eps_stride"):
        assert call(_desc(L, p, ts, **{field: (2, -4)})) < 0 and f"{who}: negative stride" in err(), field
    for kw, pat in ((dict(N=0), "must be positive"), (dict(C=0), "must be positive"), (dict(T=0), "T=0 must be positive"),
                    (dict(inv_sigma_dec=0.0), "inv_sigma_dec"), (dict(inv_sigma_dec=float("nan")), "inv_sigma_dec"),
                    (dict(inv_sigma_dec=float("inf")), "inv_sigma_dec")):
        assert call(_desc(L, p, ts, **kw)) < 0 and who in err() and pat in err(), kw
    assert call(_desc(L, p, ts, C=8, H=16384, W=16384)) < 0 and f"{who}: C*H*W" in err() and "does not fit 31 bits" in err()
    chunks = _desc(L, p, ts, C=3, H=64, W=64)                                          # two chunks: the workspace of bd_vb_terms
    need = lib.bd_vb_terms_workspace_bytes(3, 3, 64, 64)
    assert call(chunks, None, 0) < 0 and f"{who}: workspace 0 < {need}" in err()
    assert call(chunks, p, need - 1) < 0 and "workspace" in err()
    # a prior-only batch may pass x_t = eps = NULL: it gets as far as the workspace check, the last one before the launch
    priors = (ctypes.c_int64 * 3)(1000, 1000, 1000)
    assert call(_desc(L, p, priors, C=3, H=64, W=64, x_t=None, eps=None), None, 0) < 0 and f"{who}: workspace 0 < {need}" in err()
    assert call(_desc(L, p, priors, C=3, H=64, W=64, x_t=None, eps=None, r=None), None, 0) < 0 and "null r or term_shift" in err()
    assert ctypes.sizeof(L.VbTermsShiftDesc) == _c_sizeof("bd_vb_terms_shift_desc")
    assert ctypes.sizeof(L.VbTermsShiftDesc) == ctypes.sizeof(L.VbTermsDesc) + 8 + 32 + 8
