"""CPU: the host side of the Euler, Euler-ancestral, KDPM2 and KDPM2-ancestral samplers -- the schedulers' tables against the
reference's (tests/golden/kdiff.npz, written by make_golden_kdiff.py from the imported diffusers schedulers), every stand-in chain of
the fixture bit for bit through `_plan_scalars`, the restated kernel formulas and the fixture's generator, the pipelines' draw
counts, what is refused, and the wiring of the EULER_O1-SCHED / EULER_A_O1-SCHED / KDPM2_O2-SCHED / KDPM2_A_O2-SCHED names."""
import json
import os

import numpy as np
import pytest
import torch

from tests.golden import cases as C
from tests.golden import cases_kdiff as CK
from tests.golden import cases_sigma as CS

BETAS = dict(beta_start=0.0001, beta_end=0.02)
KDIFF_NAMES = {"EULER_O1-SCHED": ("EulerDiscreteScheduler", "EulerPipeline"),
               "EULER_A_O1-SCHED": ("EulerAncestralDiscreteScheduler", "EulerAncestralPipeline"),
               "KDPM2_O2-SCHED": ("KDPM2DiscreteScheduler", "KDPM2Pipeline"),
               "KDPM2_A_O2-SCHED": ("KDPM2AncestralDiscreteScheduler", "KDPM2AncestralPipeline")}
SAMPLER_OF = {"euler": "EULER_O1-SCHED", "euler_a": "EULER_A_O1-SCHED", "kdpm2": "KDPM2_O2-SCHED", "kdpm2_a": "KDPM2_A_O2-SCHED"}


class _NoUNet:
    """what a pipeline needs of a UNet before its first evaluation"""
    device = torch.device("cpu")


def classes(sampler):
    from baddiffusion_amd import pipelines, schedulers
    s, p = KDIFF_NAMES[SAMPLER_OF[sampler]]
    return getattr(schedulers, s), getattr(pipelines, p)


def sched(sampler, n=None, **kw):
    s = classes(sampler)[0](**{**BETAS, **kw})
    if n is not None:
        s.set_timesteps(n)
    return s


def plan(s, sampler, k, churn=0.0):
    return s._plan_scalars(k, s_churn=churn) if sampler == "euler" else s._plan_scalars(k)


def restated_step(p, e, x, z, base, clip=None):
    """one transition through the restated kernel formulas, as the schedulers choose the launch: (prev, scaled)"""
    b = base if p["base"] else None
    if p["churn"] is None and p["sigma_up"] is None:
        _, _, prev, sc = CS.sigma_step_ref(e, x, p["sigma_in"], (p["dt"],), p["in_div"], base=b, clip=clip)
    else:
        _, prev, sc = CK.sigma_noise_step_ref(e, x, z, p["sigma_in"], p["dt"], p["in_div"], base=b, churn=p["churn"],
                                              sigma_up=p["sigma_up"], clip=clip)
    return prev, sc


# ---------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("sampler", CK.SAMPLERS)
@pytest.mark.parametrize("n", CK.TABLE_NS)
def test_tables_equal_the_reference(sampler, n, golden):
    g = golden("kdiff")
    s = sched(sampler, n)
    assert s.timesteps.dtype == np.float64 and np.array_equal(s.timesteps, g[f"{sampler}_ts_{n}"])
    assert s.sigmas.dtype == torch.float32 and np.array_equal(s.sigmas.numpy(), g[f"{sampler}_sigmas_{n}"])
    assert np.float32(s.init_noise_sigma) == g[f"{sampler}_init_{n}"]
    two = sampler.startswith("kdpm2")
    assert len(s.timesteps) == (2 * n - 1 if two else n) and len(s.sigmas) == (2 * n + 2 if two else n + 1)
    assert s._in_div[-1] == 1.0 and len(s._in_div) == len(s.timesteps) + 1 and s.num_inference_steps == n
    names = [k for k in ("sigmas_interpol", "sigmas_up", "sigmas_down") if f"{sampler}_{k}_{n}" in g.files]
    assert names == {"euler": [], "euler_a": [], "kdpm2": ["sigmas_interpol"],
                     "kdpm2_a": ["sigmas_interpol", "sigmas_up", "sigmas_down"]}[sampler]
    for name in names:
        got, want = getattr(s, name).numpy(), g[f"{sampler}_{name}_{n}"]
        fin = np.isfinite(want)
        assert got.dtype == np.float32 and np.array_equal(np.isfinite(got), fin) and np.array_equal(got[fin], want[fin])


def test_fixture_is_the_documented_one(golden):
    g = golden("kdiff")
    eq = lambda n: int((g[f"kdpm2_a_ts_{n}"][1:] == g[f"kdpm2_a_ts_{n}"][:-1]).sum())
    assert eq(10) == 6 and eq(5) == 0                                   # equal neighbours among the timesteps, in fp64
    assert np.isnan(g["kdpm2_a_sigmas_up_10"][-3:]).all() and np.isfinite(g["kdpm2_a_sigmas_up_10"][:-3]).all()
    assert abs(float(g["euler_init_5"]) - 157.4) < 0.05
    # sigma_interpol of KDPM2-ancestral is sigma_next up to the fp32 rounding of sigma_down (a difference of nearly equal squares at
    # the small sigmas): which is why its timesteps come out equal or nearly so
    si, sg = g["kdpm2_a_sigmas_interpol_10"], g["kdpm2_a_sigmas_10"]
    assert np.all(np.abs(si[0:17:2] - sg[1:18:2]) <= 1e-4 * sg[1:18:2])
    s = classes("kdpm2")[0]()
    assert (s.config.beta_start, s.config.beta_end) == (0.00085, 0.012)
    s.set_timesteps(10)
    assert np.array_equal(s.sigmas.numpy(), g["kdpm2_default_sigmas_10"])


def test_positions_of_equal_timesteps():
    """N = 10 of KDPM2-ancestral has equal neighbours: a timestep resolves to its last position in the first order state and to its
    first otherwise, so a loop over `timesteps` visits 0, 1, 2, ... with the state alternating"""
    s = sched("kdpm2_a", 10)
    ts = s.timesteps
    assert any(ts[k] == ts[k + 1] for k in range(len(ts) - 1))
    for k, t in enumerate(ts):
        s._stage = None if k % 2 == 0 else torch.zeros(1)
        assert s._step_index(t) == k and s._step_index(torch.tensor(t)) == k
    s._stage = None
    with pytest.raises(ValueError, match="is not one of this schedule's"):
        s._step_index(998.0)


# ---------------------------------------------------------------------------------------------------- chains, bit for bit
@pytest.mark.parametrize("case", CK.CHAIN_CASES, ids=lambda c: CK.chain_tag(c[0], c[3]))
def test_plan_scalars_reproduce_the_reference_chain_bit_for_bit(case, golden):
    name, sampler, churn, n = case
    g, tag = golden("kdiff"), CK.chain_tag(name, n)
    ref = torch.from_numpy(g[f"chain_{tag}"])
    s = sched(sampler, n)
    gen = torch.Generator().manual_seed(CK.NOISE_SEED)
    x = C.pndm_init() * s.init_noise_sigma
    sc = (x * 1.0) / torch.tensor(s._in_div[0])
    base, kernels = None, []
    assert len(s.timesteps) == len(ref)
    for k, t in enumerate(s.timesteps):
        e = C.pndm_fake_model(sc, t)
        z = torch.randn(x.shape, generator=gen) if CK.draws_per_chain(sampler, n) else None        # the reference draws in every call
        p = plan(s, sampler, k, churn)
        kernels.append("noise" if p["churn"] is not None or p["sigma_up"] is not None else "step")
        prev, sc_next = restated_step(p, e, x, z, base)
        assert torch.equal(prev, ref[k]), f"position {k}"
        if k + 1 < len(s.timesteps):                                                          # the scaled output is the next model input
            assert torch.equal(sc_next, prev / torch.tensor(s._in_div[k + 1]))
        base, x, sc = x, prev, sc_next
    assert torch.equal(sc, x)                                                                 # the last divisor is 1
    assert torch.equal(torch.randn(x.shape, generator=gen), torch.from_numpy(g[f"chain_next_{tag}"]))
    want = {"euler": ["step"] * n, "euler_churn": ["noise"] * n, "euler_churn_low": ["noise"] * n, "euler_a": ["noise"] * n, "kdpm2": ["step"] * (2 * n - 1),
            "kdpm2_a": (["step", "noise"] * n)[:2 * n - 1]}[name]
    assert kernels == want


def test_churn_takes_the_cap_and_the_window():
    s = sched("euler", 5)
    cap = s._plan_scalars(0, s_churn=CK.S_CHURN)
    sig = s.sigmas[0]
    hat = sig * (2 ** 0.5 - 1 + 1)
    assert cap["sigma_in"] == float(hat) and cap["churn"] == (1.0, float((hat ** 2 - sig ** 2) ** 0.5)) and cap["churn"][1] > 0
    s20 = sched("euler", 20)
    assert s20._plan_scalars(3, s_churn=CK.S_CHURN)["sigma_in"] == float(s20.sigmas[3] * (2 ** 0.5 - 1 + 1))      # 10 / 20 = 0.5: still the cap
    below = s20._plan_scalars(3, s_churn=CK.S_CHURN_LOW, s_noise=1.003)                    # 4 / 20 = 0.2
    assert below["sigma_in"] == float(s20.sigmas[3] * 1.2) and below["churn"][0] == 1.003
    assert below["dt"] == float(s20.sigmas[4] - s20.sigmas[3] * 1.2) and below["in_div"] == s20._in_div[4]
    # outside [s_tmin, s_tmax] and at s_churn = 0 the step is the plain Euler one
    for kw in (dict(s_churn=0.0), dict(s_churn=CK.S_CHURN, s_tmin=1e4), dict(s_churn=CK.S_CHURN, s_tmax=1e-3)):
        p = s20._plan_scalars(3, **kw)
        assert p["churn"] is None and p["sigma_in"] == float(s20.sigmas[3]) and p["dt"] == float(s20.sigmas[4] - s20.sigmas[3])


# ---------------------------------------------------------------------------------------------------- draws
@pytest.mark.parametrize("sampler", CK.SAMPLERS)
def test_noise_draws_are_the_reference_generators(sampler, golden):
    """noise_draws() tensors after the fixture's seed lead to the tensor the reference's generator yielded after its chain"""
    g = golden("kdiff")
    cls, pipe = classes(sampler)
    p = pipe(_NoUNet(), sched(sampler))
    assert p.noise_draws() == CK.draws_per_chain(sampler, pipe.default_steps)
    for n in CK.CHAIN_NS:
        draws = p.noise_draws(num_inference_steps=n)
        assert draws == CK.draws_per_chain(sampler, n) == {"euler": n, "euler_a": n, "kdpm2": 0, "kdpm2_a": 2 * n - 1}[sampler]
        gen = torch.Generator().manual_seed(CK.NOISE_SEED)
        for _ in range(draws):
            torch.randn(2, 3, 8, 8, generator=gen)
        assert torch.equal(torch.randn(2, 3, 8, 8, generator=gen), torch.from_numpy(g[f"chain_next_{CK.chain_tag(sampler, n)}"]))
        if sampler == "euler":                       # with or without churn the reference draws in every step
            assert np.array_equal(g[f"chain_next_{CK.chain_tag('euler_churn', n)}"], g[f"chain_next_{CK.chain_tag('euler', n)}"])
    assert p.noise_draws(num_inference_steps=10, start_from=2) == max(0, CK.draws_per_chain(sampler, 10) - 2) * (sampler != "kdpm2")
    # advance_generator draws the initial sample and the chain's tensors
    p.unet = type("U", (), {"device": torch.device("cpu"), "config": type("Cfg", (), {"sample_size": 8, "in_channels": 3})})()
    a, b = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    p.advance_generator(2, a, False, num_inference_steps=5)
    for _ in range(1 + CK.draws_per_chain(sampler, 5)):
        torch.randn(2, 3, 8, 8, generator=b)
    assert torch.equal(torch.randn(3, generator=a), torch.randn(3, generator=b))


def test_draw_step_noise_keeps_a_cpu_stream_and_spares_a_device_one():
    from baddiffusion_amd.schedulers import ShardedGenerator, draw_step_noise
    a, b = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    assert draw_step_noise((2, 3, 4, 4), a, "cpu", False) is None                          # drawn and dropped
    torch.randn(2, 3, 4, 4, generator=b)
    assert torch.equal(draw_step_noise((2, 3, 4, 4), a, "cpu", True), torch.randn(2, 3, 4, 4, generator=b))
    assert draw_step_noise((2, 3, 4, 4), None, "cpu", False) is None
    # a sharded stream: the whole chunk is drawn, this rank's rows are kept
    a, b = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    sh = ShardedGenerator(a, 4, 1, 3)
    assert draw_step_noise((2, 3, 4, 4), sh, "cpu", False) is None
    torch.randn(4, 3, 4, 4, generator=b)
    assert torch.equal(draw_step_noise((2, 3, 4, 4), sh, "cpu", True), torch.randn(4, 3, 4, 4, generator=b)[1:3])


# ---------------------------------------------------------------------------------------------------- configs, refusals
def test_config_conversion_and_pipelines():
    import inspect
    from baddiffusion_amd.pipelines import PNDMPipeline, _SigmaPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    ddpm = DDPMScheduler(num_train_timesteps=400, beta_start=0.0002, beta_end=0.03, beta_schedule="scaled_linear")
    for sampler in CK.SAMPLERS:
        cls, pipe = classes(sampler)
        s = cls.from_config(ddpm.config)
        assert len(s) == 400 and torch.equal(s.betas, ddpm.betas) and s.config.prediction_type == "epsilon"
        p = pipe(_NoUNet(), ddpm)
        assert type(p.scheduler) is cls and torch.equal(p.scheduler.betas, ddpm.betas) and p.clip_sample is False
        assert pipe(_NoUNet(), s, clip_sample=True).scheduler is s
        assert issubclass(pipe, _SigmaPipeline) and "_sample" not in vars(pipe) and "__call__" not in vars(pipe)
        assert list(inspect.signature(pipe.__call__).parameters) == list(inspect.signature(PNDMPipeline.__call__).parameters)
    assert [classes(k)[1].default_steps for k in CK.SAMPLERS] == [20, 20, 10, 10]
    e = classes("euler")[1](_NoUNet(), ddpm, s_churn=3.0, s_noise=1.01)
    assert e._step_kwargs() == {"s_churn": 3.0, "s_noise": 1.01} and classes("euler")[1](_NoUNet(), ddpm)._step_kwargs()["s_churn"] == 0.0


@pytest.mark.parametrize("sampler", CK.SAMPLERS)
def test_load_and_save_scheduler_round_trip(sampler, tmp_path):
    from baddiffusion_amd.model import load_scheduler, save_scheduler
    s = sched(sampler, num_train_timesteps=400, beta_schedule="scaled_linear", beta_end=0.03)
    s.config.clip_sample = True                      # what DiffuserModelSched attaches to every scheduler it returns
    save_scheduler(s, str(tmp_path))
    saved = json.load(open(os.path.join(str(tmp_path), "scheduler_config.json")))
    assert saved["_class_name"] == type(s).__name__ and saved["num_train_timesteps"] == 400 and saved["beta_end"] == 0.03
    back = load_scheduler(str(tmp_path))
    assert type(back) is type(s) and {k: back.config[k] for k in s._KEYS} == {k: s.config[k] for k in s._KEYS}
    assert torch.equal(back.sigmas, s.sigmas)


def test_refusals():
    x = torch.zeros(2, 3, 8, 8)
    pipe_a = classes("kdpm2_a")[1]
    for n in (1, 2):
        with pytest.raises(ValueError, match=f"num_inference_steps={n} must be at least 3"):
            sched("kdpm2_a", n)
        with pytest.raises(ValueError, match="must be at least 3"):
            pipe_a(_NoUNet(), sched("kdpm2_a"))(batch_size=1, num_inference_steps=n, init=x)
    sched("kdpm2_a", 3), sched("kdpm2", 2)
    euler = classes("euler")[0]
    with pytest.raises(NotImplementedError, match="use_karras_sigmas"):
        euler(use_karras_sigmas=True)
    with pytest.raises(NotImplementedError, match="interpolation_type='log_linear'"):
        euler(interpolation_type="log_linear")
    for sampler in CK.SAMPLERS:
        s = sched(sampler)
        with pytest.raises(ValueError, match="Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler"):
            s.step(x, 999.0, x)
        s.set_timesteps(5)
        with pytest.raises(RuntimeError, match=r"Scheduler\.step runs on the GPU only"):
            s.step(x, 999.0, x)
        with pytest.raises(RuntimeError, match=r"scale_model_input runs on the GPU only"):
            s.scale_model_input(x, 999.0)
        v = sched(sampler, 5, prediction_type="v_prediction")
        with pytest.raises(ValueError, match="must be `epsilon` on the HIP path"):
            v.step(x, 999.0, x)
    for sampler in ("kdpm2", "kdpm2_a"):
        s = sched(sampler, 5)
        # a stage / position mismatch: the second timestep belongs to a second stage, the scheduler is in the first order state
        with pytest.raises(ValueError, match="position 1 of the schedule is a second stage, the scheduler is in the other state"):
            s._check_stage(1)
        s._stage = x
        with pytest.raises(ValueError, match="position 2 of the schedule is a first order stage, the scheduler is in the other state"):
            s._check_stage(2)
        with pytest.raises(ValueError, match="position 0 of the schedule is a first order stage"):
            s.step(x, s.timesteps[0], x)             # resolves to position 0 and is refused before the GPU is asked for
        s.set_timesteps(5)
        assert s.state_in_first_order                # set_timesteps resets a pending stage
        p = classes(sampler)[1](_NoUNet(), s)
        for k in (1, 3):
            with pytest.raises(ValueError, match=f"start_from={k} is the second stage of a transition"):
                p(batch_size=1, num_inference_steps=5, start_from=k)


def test_dyn_threshold_is_refused_with_the_names():
    from baddiffusion_amd.model import DiffuserModelSched
    for name in KDIFF_NAMES:
        with pytest.raises(NotImplementedError, match=f"dyn_threshold with {name}: dynamic thresholding runs in the DDPM and DDIM steps only"):
            DiffuserModelSched.get_pretrained("DDPM-CIFAR10-32", noise_sched_type=name, allow_random_init=True, dyn_threshold=1.5)


# ---------------------------------------------------------------------------------------------------- wiring
def test_sched_name_wiring():
    from baddiffusion_amd.model import DiffuserModelSched
    from baddiffusion_amd.sched_names import SCHEDS
    family = {classes(sampler)[0] for sampler in SAMPLER_OF}
    assert {n: (r.scheduler.__name__, r.pipeline.__name__) for n, r in SCHEDS.items() if r.scheduler in family} == KDIFF_NAMES
    # no PNDM conversion, with or without native_sched, and nothing refused
    assert all(SCHEDS[n].carrier is None and not SCHEDS[n].native_only and SCHEDS[n].refused is None for n in KDIFF_NAMES)
    get = lambda name, **kw: DiffuserModelSched.get_pretrained("DDPM-CIFAR10-32", noise_sched_type=name, allow_random_init=True, **kw)
    for sampler, name in SAMPLER_OF.items():
        cls, pipe = classes(sampler)
        for native in (False, True):
            m, s, gp = get(name, clip_sample=True, native_sched=native)
            assert type(s) is cls and type(s).__name__ == KDIFF_NAMES[name][0]
            assert s.config.num_train_timesteps == 1000 and torch.equal(s.betas, torch.linspace(0.0001, 0.02, 1000))
            p = gp(m, s)
            assert type(p) is pipe and p.scheduler is s and p.clip_sample is True
            del m, p
    m, s, gp = get("EULER_A_O1-SCHED", clip_sample=False)
    assert gp(m, s).clip_sample is False


def test_cli_accepts_the_names_and_args_json_round_trips(tmp_path, monkeypatch, capsys):
    import baddiffusion as cli
    monkeypatch.chdir(tmp_path)
    assert set(KDIFF_NAMES) < set(cli.SCHED_CHOICES)
    base = ["--project", "default", "--dataset", "CIFAR10", "--batch", "64", "--ckpt", "DDPM-CIFAR10-32", "-o"]
    for name in KDIFF_NAMES:
        cfg = cli.setup(["--mode", "train", "--sched", name, "--infer_steps", "10"] + base)
        assert cfg.sched == name and cfg.native_sched is False and cfg.infer_steps == 10
        saved = json.load(open(os.path.join(cfg.output_dir, "args.json")))
        assert saved["sched"] == name and saved["infer_steps"] == 10
        c = cli.setup(["--mode", "sampling", "--ckpt", cfg.output_dir, "--infer_steps", "15"], write=False)
        assert c.sched == name and c.infer_steps == 15
    for bad in ("EULER_O2-SCHED", "KDPM2_A_O1-SCHED", "EULER-SCHED"):
        with pytest.raises(SystemExit):
            cli.parse_args(["--mode", "train", "--sched", bad])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    text = "".join(capsys.readouterr().out.split())
    assert all(name in text for name in KDIFF_NAMES) and "EulerAncestralPipeline" in text and "KDPM2AncestralPipeline" in text


def test_elijah_defense_accepts_the_names(tmp_path, capsys):
    import elijah_defense as E
    from baddiffusion_amd.schedulers import DDPMScheduler
    assert set(KDIFF_NAMES) < set(E.SCHED_CHOICES)
    ckpt_sched = DDPMScheduler(num_train_timesteps=400)
    for sampler, name in SAMPLER_OF.items():
        cfg = E.get_config(["--ckpt", "x", "--sched", name, "--infer_steps", "12", "--output_dir", str(tmp_path)])
        assert cfg.sched == name and cfg.infer_steps == 12
        p = E.make_pipeline(cfg, _NoUNet(), ckpt_sched)
        assert type(p) is classes(sampler)[1] and len(p.scheduler) == 400
    capsys.readouterr()
    with pytest.raises(SystemExit):
        E.get_config(["--help"])
    assert "KDPM2_A_O2" in "".join(capsys.readouterr().out.split())
