"""CPU: the sampler-matched correction tables (baddiffusion_amd/correction.py) -- their identities in float64, an open-loop DDIM chain
written out here, make_table's refusals, the command lines, and the host checks of the two *_corr entry points."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests.golden import cases_correction as CC


@pytest.fixture(scope="module")
def tabs():
    al, ac = CC.float_tables()
    return al.double().numpy(), ac.double().numpy()


class Sched:
    """what make_table reads of a scheduler"""

    def __init__(self):
        self.alphas, self.alphas_cumprod = CC.float_tables()


def tables64():
    """the same schedule built in float64 throughout: ac_t = alpha_t ac_(t-1) holds to float64 rounding, which the identity below needs
    (the schedulers' float32 cumprod keeps it to 6e-8 only)"""
    al = 1.0 - np.linspace(CC.BETA_START, CC.BETA_END, CC.T, dtype=np.float64)
    return al, np.cumprod(al)


def test_ddim_table_at_T_steps_eta_1_is_the_reference_rho(tabs):
    """BadDiffusion is the special case: one step per timestep at eta = 1"""
    from baddiffusion_amd import correction as K
    al, ac = tables64()
    rho = K.reference_rho(al, ac)
    assert np.array_equal(rho, (1 - np.sqrt(al)) * np.sqrt(1 - ac) / (1 - al))
    rel = np.abs(K.ddim_table(ac, CC.T, 1.0) - rho) / rho
    al32, ac32 = tabs
    rel32 = np.abs(K.ddim_table(ac32, CC.T, 1.0) - K.reference_rho(al32, ac32)) / K.reference_rho(al32, ac32)
    print(f"MEASURE max rel |ddim_table(T, 1) - rho| {rel.max():.3e} on float64 tables (bound 1e-10); on the schedulers' float32 cumprod "
          f"{rel32.max():.3e} (bound 1e-6: ac_t / ac_(t-1) is alpha_t to float32 rounding there)")
    assert rel.max() <= 1e-10
    assert rel32.max() <= 1e-6


def test_sde_and_ode_tables(tabs):
    from baddiffusion_amd import correction as K
    al, ac = tabs
    rho = K.reference_rho(al, ac)
    rel = np.abs(K.sde_table(ac, 1.0) - rho) / rho
    print(f"MEASURE max rel |sde_table(1) - rho| {rel.max():.4e} at t = {int(rel.argmax())} (bound 5.1e-3, beta_T / 4 = {0.02 / 4:.4e})")
    assert rel.max() <= 5.1e-3
    assert np.array_equal(K.ode_table(ac), np.sqrt(1 - ac)) and K.ode_table(ac).dtype == np.float64
    assert np.array_equal(K.ode_table(ac), K.sde_table(ac, 0.0))
    assert np.array_equal(K.ode_table(torch.from_numpy(ac)), K.ode_table(ac))            # tensors and arrays alike
    # the float32 scheduler tables go in as they are: float64 inside
    assert np.array_equal(K.ode_table(CC.float_tables()[1]), K.ode_table(ac))


@pytest.mark.parametrize("steps", (1, 7, 50, 1000))
@pytest.mark.parametrize("eta", (0.0, 0.5, 1.0))
def test_every_ddim_table_is_positive_and_finite(tabs, steps, eta):
    from baddiffusion_amd import correction as K
    c = K.ddim_table(tabs[1], steps, eta)
    assert c.shape == (CC.T,) and c.dtype == np.float64
    assert np.isfinite(c).all() and (c > 0).all(), (steps, eta, c.min())
    c0 = K.ddim_table(tabs[1], steps, eta, final_alpha_cumprod=float(tabs[1][0]))          # set_alpha_to_one=False
    assert np.isfinite(c0[1:]).all() and (c0[1:] > 0).all()


def test_other_tables_positive_and_finite(tabs):
    from baddiffusion_amd import correction as K
    for c in (K.reference_rho(*tabs), K.ode_table(tabs[1]), K.sde_table(tabs[1], 0.3), K.sde_table(tabs[1], 2.0)):
        assert np.isfinite(c).all() and (c > 0).all()


def test_open_loop_ddim_chain_in_float64(tabs):
    """DDIM eta = 0 at 50 steps, written out, from the exact shifted marginal at its first timestep with the model output eps + c_t r:
    the exact table closes the chain, the ode table nearly, the reference's rho misses by far (here 1.7e-13, 0.038, 38.6; the reference's
    own DDIM step, which takes its square roots in float32, leaves 8.1e-6 with the exact table: the fixture's res_ddim_ddim50)"""
    from baddiffusion_amd import correction as K
    al, ac = tabs
    y, r, eps = (v.numpy() for v in CC.inputs())
    ratio = CC.T // 50
    ts = (np.arange(50) * ratio)[::-1]

    def chain(c):
        a = ac[ts[0]]
        x = np.sqrt(a) * y + np.sqrt(1 - a) * eps + (1 - np.sqrt(a)) * r
        for t in ts:
            e, ap = eps + c[t] * r, (ac[t - ratio] if t >= ratio else 1.0)
            x = np.sqrt(ap) * (x - np.sqrt(1 - ac[t]) * e) / np.sqrt(ac[t]) + np.sqrt(1 - ap) * e
        return float(np.abs(x - y).max())

    exact, ode, rho = chain(K.ddim_table(ac, 50, 0.0)), chain(K.ode_table(ac)), chain(K.reference_rho(al, ac))
    print(f"MEASURE open-loop DDIM-50 float64: exact table {exact:.3e} (<= 1e-4), ode {ode:.4f} (<= 0.1), rho {rho:.2f} (> 10)")
    assert exact <= 1e-4
    assert ode <= 0.1
    assert rho > 10


def test_tables_match_the_fixture(tabs, golden):
    """the fixture's tables are written out in its generator, not computed by correction.py"""
    from baddiffusion_amd import correction as K
    g = golden("correction")
    al, ac = tabs
    for name, mine in (("rho", K.reference_rho(al, ac)), ("ode", K.ode_table(ac)), ("ddim", K.ddim_table(ac, CC.DDIM_STEPS, 0.0))):
        assert np.abs(mine - g[name]).max() <= 1e-12 * np.abs(g[name]).max(), name
    y, r, eps = CC.inputs()
    assert np.array_equal(g["y"], y.numpy()) and np.array_equal(g["r"], r.numpy()) and np.array_equal(g["eps"], eps.numpy())


def test_interp(tabs):
    from baddiffusion_amd import correction as K
    tab = K.ode_table(tabs[1])
    for t in (0, 1, 500, CC.T - 1):
        assert float(K.interp(tab, t)) == tab[t] and float(K.interp(tab, float(t))) == tab[t]
    assert float(K.interp(tab, 10.25)) == pytest.approx(0.75 * tab[10] + 0.25 * tab[11], rel=1e-15)
    assert float(K.interp(tab, CC.T - 1.5)) == pytest.approx(0.5 * (tab[-2] + tab[-1]), rel=1e-15)
    assert float(K.interp(tab, -3.0)) == tab[0] and float(K.interp(tab, 1e9)) == tab[-1]          # clamped to the table
    got = K.interp(torch.from_numpy(tab).float(), torch.tensor([2.0, 2.5]))
    assert got.dtype == torch.float64 and got.shape == (2,)
    assert float(got[1]) == pytest.approx(0.5 * (float(np.float32(tab[2])) + float(np.float32(tab[3]))), rel=1e-15)
    for t in (0.0, 123.4, 998.999, 999.0):                                                           # the generator's own interpolation
        assert CC.interp_np(tab, t) == pytest.approx(float(K.interp(tab, t)), rel=1e-15)


def test_make_table_and_its_refusals(tabs):
    from baddiffusion_amd import correction as K
    s = Sched()
    assert K.make_table("ddpm", s) is None and K.make_table("ddpm", s, device="cpu") is None
    t = K.make_table("ode", s, device="cpu")
    assert t.dtype == torch.float32 and t.shape == (CC.T,) and t.device.type == "cpu"
    assert np.array_equal(t.numpy(), K.ode_table(tabs[1]).astype(np.float32))
    assert np.array_equal(K.make_table("sde", s, zeta=1.0, device="cpu").numpy(), K.sde_table(tabs[1], 1.0).astype(np.float32))
    assert np.array_equal(K.make_table("ddim", s, steps=50, device="cpu").numpy(), K.ddim_table(tabs[1], 50, 0.0).astype(np.float32))
    assert np.array_equal(K.make_table("ddim", s, steps=7, eta=0.5, device="cpu").numpy(), K.ddim_table(tabs[1], 7, 0.5).astype(np.float32))
    for kind in ("ddpm", "ode", "ddim"):
        with pytest.raises(ValueError, match="zeta belongs to the 'sde' table"):
            K.make_table(kind, s, zeta=0.5, steps=50 if kind == "ddim" else None, device="cpu")
    for kind in ("ddpm", "ode", "sde"):
        with pytest.raises(ValueError, match="steps / eta belong to the 'ddim' table"):
            K.make_table(kind, s, steps=50, zeta=1.0 if kind == "sde" else None, device="cpu")
        with pytest.raises(ValueError, match="steps / eta belong to the 'ddim' table"):
            K.make_table(kind, s, eta=0.0, zeta=1.0 if kind == "sde" else None, device="cpu")
    with pytest.raises(ValueError, match="steps must be in 1 .. T = 1000, got 1001"):
        K.make_table("ddim", s, steps=CC.T + 1, device="cpu")
    with pytest.raises(ValueError, match="steps must be in 1 .. T = 1000, got 0"):
        K.make_table("ddim", s, steps=0, device="cpu")
    with pytest.raises(ValueError, match="zeta must be >= 0"):
        K.make_table("sde", s, zeta=-0.1, device="cpu")
    with pytest.raises(ValueError, match="eta must be >= 0"):
        K.make_table("ddim", s, steps=50, eta=-1.0, device="cpu")
    with pytest.raises(ValueError, match="needs zeta"):
        K.make_table("sde", s, device="cpu")
    with pytest.raises(ValueError, match="needs steps"):
        K.make_table("ddim", s, device="cpu")
    with pytest.raises(ValueError, match="must be one of"):
        K.make_table("pndm", s, device="cpu")


# ---------------------------------------------------------------------------------------------------- command lines
BASE = ["--project", "default", "--dataset", "CIFAR10", "--batch", "64", "--ckpt", "DDPM-CIFAR10-32", "-o"]
KEYS = ("correction", "correction_zeta", "correction_steps", "correction_eta")


def test_cli_correction_round_trips_through_args_json(tmp_path, monkeypatch):
    import baddiffusion as cli
    monkeypatch.chdir(tmp_path)
    cfg = cli.setup(["--mode", "train", "--correction", "ode"] + BASE)
    assert cfg.correction == "ode"
    saved = json.load(open(os.path.join(cfg.output_dir, "args.json")))
    assert saved["correction"] == "ode" and not any(k in saved for k in KEYS[1:])
    assert json.load(open(os.path.join(cfg.output_dir, "config.json")))["correction"] == "ode"
    assert cli.setup(["--mode", "resume", "--ckpt", cfg.output_dir], write=False).correction == "ode"
    # sampling and measure read the run's file and use nothing of it; the flag itself is a training flag
    for mode in ("sampling", "measure"):
        cli.setup(["--mode", mode, "--ckpt", cfg.output_dir], write=False)
        with pytest.raises(NotImplementedError, match="correction"):
            cli.setup(["--mode", mode, "--ckpt", cfg.output_dir, "--correction", "ode"], write=False)
    cfg = cli.setup(["--mode", "train+measure", "--correction", "ddim", "--correction_steps", "50", "--correction_eta", "0.5"] + BASE)
    saved = json.load(open(os.path.join(cfg.output_dir, "args.json")))
    assert (saved["correction"], saved["correction_steps"], saved["correction_eta"]) == ("ddim", 50, 0.5) and "correction_zeta" not in saved
    r = cli.setup(["--mode", "resume", "--ckpt", cfg.output_dir], write=False)
    assert (r.correction, r.correction_steps, r.correction_eta) == ("ddim", 50, 0.5)
    # the table the loop builds from such a config
    t = cli.make_correction(r, Sched(), "cpu")
    from baddiffusion_amd import correction as K
    assert np.array_equal(t.numpy(), K.ddim_table(CC.float_tables()[1], 50, 0.5).astype(np.float32))


def test_cli_without_the_flag_writes_what_it_wrote(tmp_path, monkeypatch):
    import baddiffusion as cli
    monkeypatch.chdir(tmp_path)
    cfg = cli.setup(["--mode", "train"] + BASE)
    for name in ("args.json", "config.json"):
        saved = json.load(open(os.path.join(cfg.output_dir, name)))
        assert not any(k in saved for k in KEYS), name
    assert not hasattr(cfg, "correction") and cli.make_correction(cfg, Sched(), "cpu") is None
    assert not hasattr(cli.setup(["--mode", "resume", "--ckpt", cfg.output_dir], write=False), "correction")
    with pytest.raises(ValueError, match="need --correction"):
        cli.setup(["--mode", "train", "--correction_zeta", "1.0"] + BASE, write=False)
    with pytest.raises(ValueError, match="zeta belongs to the 'sde' table"):
        cli.setup(["--mode", "train", "--correction", "ode", "--correction_zeta", "1.0"] + BASE, write=False)
    with pytest.raises(ValueError, match="needs steps"):
        cli.setup(["--mode", "train", "--correction", "ddim"] + BASE, write=False)


def test_elijah_lam_default_follows_the_table(tmp_path, tabs):
    import elijah_defense as E
    from baddiffusion_amd import correction as K
    base = ["--ckpt", str(tmp_path / "ckpt"), "--output_dir", str(tmp_path)]
    plain = E.get_config(base)
    assert plain.lam == 0.5 and not hasattr(plain, "correction")
    saved = json.load(open(os.path.join(plain.output_dir, "config.json")))
    assert saved["lam"] == 0.5 and "correction" not in saved
    ode = E.get_config(base + ["--correction", "ode"])
    assert ode.lam == K.ode_table(tabs[1])[-1] and abs(ode.lam - 0.99998) < 1e-5
    assert json.load(open(os.path.join(ode.output_dir, "config.json")))["correction"] == "ode"
    assert E.get_config(base + ["--correction", "ddpm"]).lam == pytest.approx(0.5025, abs=1e-4)
    assert E.get_config(base + ["--correction", "sde", "--correction_zeta", "1.0"]).lam == K.sde_table(tabs[1], 1.0)[-1]
    assert E.get_config(base + ["--correction", "ddim", "--correction_steps", "50"]).lam == K.ddim_table(tabs[1], 50, 0.0)[-1]
    assert E.get_config(base + ["--correction", "ode", "--lam", "0.3"]).lam == 0.3            # an explicit --lam wins
    # the checkpoint's own scheduler carries the tables
    from baddiffusion_amd.model import save_scheduler
    from baddiffusion_amd.schedulers import DDPMScheduler
    save_scheduler(DDPMScheduler(beta_end=0.01), str(tmp_path / "ckpt" / "scheduler"))
    other = E.get_config(base + ["--correction", "ode"]).lam
    assert other == K.ode_table(DDPMScheduler(beta_end=0.01).alphas_cumprod)[-1] and other != ode.lam
    with pytest.raises(SystemExit):
        E.get_config(base + ["--correction_zeta", "1.0"])


# ---------------------------------------------------------------------------------------------------- entry points, on the host
def test_corr_entry_points_reject_bad_arguments_without_gpu():
    from baddiffusion_amd import _lib as L
    lib = L.load()
    p = 4096                         # an aligned address that is never dereferenced: every call returns before its launch
    for name, Desc, ptrs in (("bd_poison_qsample_corr", L.PoisonQsampleCorrDesc,
                              ("images_f32", "is_poison", "trigger", "target_img", "noise", "timesteps", "alphas_cumprod", "x_noisy", "target")),
                             ("bd_qsample_corr", L.QsampleCorrDesc, ("x0", "R", "noise", "timesteps", "alphas_cumprod", "x_noisy", "target"))):
        fn = getattr(lib, name)
        assert fn(None, None) == -1 and name.encode() + b": null descriptor" in lib.bd_last_error()

        def desc(**kw):
            base = dict(B=2, C=3, H=4, W=4, ld_noisy=3, ld_target=3, corr=p, **{k: p for k in ptrs})
            base.update(kw)
            return Desc(**base)
        assert fn(ctypes.byref(desc(corr=None)), None) == -1
        assert name.encode() + b": null corr" in lib.bd_last_error()
        for bad in (dict(B=0), dict(C=0), dict(H=-1), dict(W=0)):
            assert fn(ctypes.byref(desc(**bad)), None) == -1 and name.encode() + b": bad shape" in lib.bd_last_error(), bad
        for k in ptrs:
            if k == "images_f32":
                continue
            assert fn(ctypes.byref(desc(**{k: None})), None) == -1 and name.encode() + b": null pointer" in lib.bd_last_error(), k
        assert fn(ctypes.byref(desc(ld_noisy=2)), None) == -1 and name.encode() + b": ld < C" in lib.bd_last_error()
        assert fn(ctypes.byref(desc(ld_target=2)), None) == -1 and name.encode() + b": ld < C" in lib.bd_last_error()
    d = L.PoisonQsampleCorrDesc(B=2, C=3, H=4, W=4, ld_noisy=3, ld_target=3, corr=p, images_f32=p, images_u8=p)
    assert lib.bd_poison_qsample_corr(ctypes.byref(d), None) == -1 and b"bd_poison_qsample_corr: exactly one of" in lib.bd_last_error()
    d = L.PoisonQsampleCorrDesc(B=2, C=3, H=4, W=4, ld_noisy=3, ld_target=3, corr=p)
    assert lib.bd_poison_qsample_corr(ctypes.byref(d), None) == -1 and b"bd_poison_qsample_corr: exactly one of" in lib.bd_last_error()
    # the descriptors are the old ones plus one pointer
    assert ctypes.sizeof(L.PoisonQsampleCorrDesc) == ctypes.sizeof(L.PoisonQsampleDesc) + 8
    assert ctypes.sizeof(L.QsampleCorrDesc) == ctypes.sizeof(L.QsampleDesc) + 8
    assert L.PoisonQsampleCorrDesc.corr.offset == ctypes.sizeof(L.PoisonQsampleDesc) and L.QsampleCorrDesc.corr.offset == ctypes.sizeof(L.QsampleDesc)


def test_corr_struct_layouts_match_the_header():
    """sizeof / offsetof(corr) as the C compiler sees the header, against the ctypes mirrors"""
    import subprocess
    from baddiffusion_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = {"bd_poison_qsample_corr_desc": L.PoisonQsampleCorrDesc, "bd_qsample_corr_desc": L.QsampleCorrDesc}
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "bd_hip.h"\nint main(){' + "".join(
        f'printf("{n} %zu %zu\\n", sizeof({n}), offsetof({n}, corr));' for n in names) + "return 0;}"
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), c, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True).stdout
    for line in out.strip().splitlines():
        n, size, off = line.split()
        assert ctypes.sizeof(names[n]) == int(size) and names[n].corr.offset == int(off), line


def test_ops_refuse_a_table_of_the_wrong_kind():
    from baddiffusion_amd import ops
    ac = torch.ones(10)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops._corr_table(torch.ones(10), ac)
