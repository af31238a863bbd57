"""CPU: the host side of the sigma-space samplers -- HeunDiscreteScheduler / LMSDiscreteScheduler tables, LMS coefficients and
per-position scalars against the reference's (tests/golden/sigma.npz, written by make_golden_sigma.py from the imported diffusers
schedulers), every stand-in chain of the fixture through those scalars and the restated kernel formula, config persistence, the wiring of
the HEUN_O2-SCHED / LMSD_O*-SCHED names (model.py, baddiffusion.py, elijah_defense.py), what is refused, and the host checks of
bd_sigma_step, bd_scale_input, bd_timestep_embedding_f32 and bd_unet_forward_tf through bd_last_error()."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests.golden import cases as C
from tests.golden import cases_sigma as CS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA_NAMES = {"HEUN_O2-SCHED": ("HeunDiscreteScheduler", 2), "LMSD_O1-SCHED": ("LMSDiscreteScheduler", 1),
               "LMSD_O2-SCHED": ("LMSDiscreteScheduler", 2), "LMSD_O3-SCHED": ("LMSDiscreteScheduler", 3),
               "LMSD_O4-SCHED": ("LMSDiscreteScheduler", 4)}
BETAS = dict(beta_start=0.0001, beta_end=0.02)


class _NoUNet:
    """what a pipeline needs of a UNet before its first evaluation"""
    device = torch.device("cpu")


def _sched(sampler, **kw):
    from baddiffusion_amd.schedulers import HeunDiscreteScheduler, LMSDiscreteScheduler
    return (HeunDiscreteScheduler if sampler == "heun" else LMSDiscreteScheduler)(**{**BETAS, **kw})


# ---------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("sampler", ("heun", "lms"))
@pytest.mark.parametrize("n", CS.SCHEDULE_NS)
def test_schedules_equal_the_reference(sampler, n, golden):
    g = golden("sigma")
    s = _sched(sampler)
    s.set_timesteps(n)
    assert s.timesteps.dtype == np.float64 and np.array_equal(s.timesteps, g[f"{sampler}_ts_{n}"])
    assert s.sigmas.dtype == torch.float32 and np.array_equal(s.sigmas.numpy(), g[f"{sampler}_sigmas_{n}"])
    assert np.float32(s.init_noise_sigma) == g[f"{sampler}_init_{n}"] and s.init_noise_sigma == float(s.sigmas.max())
    assert len(s.timesteps) == (2 * n - 1 if sampler == "heun" else n) and len(s.sigmas) == (2 * n if sampler == "heun" else n + 1)
    assert float(s.sigmas[-1]) == 0.0 and s._in_div[-1] == 1.0 and s.num_inference_steps == n
    # the divisor of every position is the reference's expression on its fp32 0-dim tensors
    sig = torch.from_numpy(g[f"{sampler}_sigmas_{n}"])
    assert s._in_div == [float((v ** 2 + 1) ** 0.5) for v in sig]


def test_schedule_fixture_is_the_documented_one(golden):
    g = golden("sigma")
    assert g["heun_ts_5"].tolist() == [999.0, 749.25, 749.25, 499.5, 499.5, 249.75, 249.75, 0.0, 0.0]
    assert g["lms_ts_5"].tolist() == [999.0, 749.25, 499.5, 249.75, 0.0]
    assert all(float(t).is_integer() for t in g["lms_ts_10"]) and not all(float(t).is_integer() for t in g["lms_ts_50"])
    assert abs(float(g["lms_init_5"]) - 157.4) < 0.05
    # before set_timesteps the tables are the full schedule, as the reference's constructor leaves them
    s = _sched("lms")
    assert s.num_inference_steps is None and np.array_equal(s.sigmas.numpy(), g["lms_sigmas_1000"])


def test_heun_reference_default_betas(golden):
    from baddiffusion_amd.schedulers import HeunDiscreteScheduler, LMSDiscreteScheduler
    s = HeunDiscreteScheduler()
    assert (s.config.beta_start, s.config.beta_end) == (0.00085, 0.012)
    s.set_timesteps(10)
    assert np.array_equal(s.sigmas.numpy(), golden("sigma")["heun_default_sigmas_10"])
    assert (LMSDiscreteScheduler().config.beta_start, LMSDiscreteScheduler().config.beta_end) == (0.0001, 0.02)


@pytest.mark.parametrize("n", CS.COEFF_NS)
def test_lms_coefficients(n, golden):
    """within rtol 1e-6 of the reference's: the integrand is fp32 arithmetic, so on one scipy build they are equal; the tolerance only
    allows for another QUADPACK build"""
    g = golden("sigma")
    s = _sched("lms")
    s.set_timesteps(n)
    for order in CS.LMS_ORDERS:
        want = g[f"lms_coeff_n{n}_o{order}"]
        got = s.lms_coefficients(order)
        assert len(got) == n
        for i, row in enumerate(got):
            assert len(row) == min(i + 1, order)
            np.testing.assert_allclose(np.array(row), want[i, :len(row)], rtol=1e-6, atol=0)
    with pytest.raises(ValueError, match="order must be 1..4"):
        s.lms_coefficients(5)


def test_lms_coefficients_are_kept_per_length_and_order(monkeypatch):
    s = _sched("lms")
    s.set_timesteps(5, order=3)
    assert set(s._coeffs) == {(5, 3)}
    calls = []
    keep = type(s).get_lms_coefficient
    monkeypatch.setattr(type(s), "get_lms_coefficient", lambda self, *a: calls.append(a) or keep(self, *a))
    s.set_timesteps(5, order=3)
    assert s._plan_scalars(4, 3)[1] == s._coeffs[(5, 3)][4] and calls == []          # a second chain makes no quad call
    s.lms_coefficients(2)
    assert len(calls) == 1 + 2 * 4 and set(s._coeffs) == {(5, 3), (5, 2)}
    # order 1 is Euler: the coefficient is the integral of 1, sigma_next - sigma
    for k, row in enumerate(s.lms_coefficients(1)):
        assert abs(row[0] - (float(s.sigmas[k + 1]) - float(s.sigmas[k]))) <= 1e-6 * abs(row[0])


# ---------------------------------------------------------------------------------------------------- chains through the scalars
@pytest.mark.parametrize("case", CS.CHAIN_CASES, ids=lambda c: CS.chain_tag(*c))
def test_plan_scalars_reproduce_the_reference_chain(case, golden):
    """_plan_scalars through the restated kernel formula, with the schedulers' state handling written out: every intermediate sample
    within max(4e-6, 4 * dev64) * max|ref| of the reference's (the rule of the DPM-Solver and UniPC stand-in chains); and the scaled
    output of a step is bit-equal to scale_model_input's (x * 1) / in_div of its raw output"""
    sampler, order, n = case
    g, tag = golden("sigma"), CS.chain_tag(*case)
    ref, dev64 = g[f"chain_{tag}"], float(g[f"chain_dev64_{tag}"])
    bound = max(4e-6, 4 * dev64)
    s = _sched(sampler)
    s.set_timesteps(n)
    x = C.pndm_init() * s.init_noise_sigma
    sc = (x * 1.0) / torch.tensor(s._in_div[0])
    stage, ring, worst = None, [], 0.0
    assert len(s.timesteps) == len(ref)
    for k, t in enumerate(s.timesteps):
        e = C.pndm_fake_model(sc, t)
        if sampler == "heun":
            sigma_in, dt, in_div = s._plan_scalars(k)
            if k % 2 == 0:
                _, d, prev, sc = CS.sigma_step_ref(e, x, sigma_in, (dt,), in_div)
                stage = (d, dt, x)
            else:
                assert dt is None
                _, _, prev, sc = CS.sigma_step_ref(e, x, sigma_in, (stage[1],), in_div, base=stage[2], average=True, hist=(stage[0],))
        else:
            sigma_in, coeffs, in_div = s._plan_scalars(k, order)
            assert len(coeffs) == min(k + 1, order)
            _, d, prev, sc = CS.sigma_step_ref(e, x, sigma_in, coeffs, in_div, hist=ring[::-1][:len(coeffs) - 1])
            ring = (ring + [d])[-3:]
        x = prev
        assert torch.equal(sc, (x * 1.0) / torch.tensor(in_div))
        dev = float(np.abs(x.numpy() - ref[k]).max() / np.abs(ref[k]).max())
        worst = max(worst, dev)
        assert dev <= bound, (k, float(t), dev, bound)
    assert in_div == 1.0 and torch.equal(sc, x)
    print(f"MEASURE sigma host chain {tag}: worst step deviation {worst:.3e}, bound {bound:.3e} (reference vs fp64 {dev64:.3e})")


def test_step_index_follows_the_reference():
    s = _sched("heun")
    s.set_timesteps(5)
    assert s.state_in_first_order and [s._step_index(t) for t in (999.0, 749.25, 0.0)] == [0, 2, 8]
    s._stage = (None, 0.0, None)                     # waiting for the averaging stage: the earlier entry of the pair
    assert [s._step_index(t) for t in (749.25, 0.0)] == [1, 7]
    s._stage = None
    assert s._step_index(torch.tensor(749.25)) == 2 and s._step_index(np.float32(249.75)) == 6
    assert s._plan_scalars(0) == (float(s.sigmas[0]), float(s.sigmas[1] - s.sigmas[0]), s._in_div[1])
    assert s._plan_scalars(3) == (float(s.sigmas[3]), None, s._in_div[4])
    lm = _sched("lms")
    lm.set_timesteps(50)
    t = lm.timesteps[1]
    assert not float(t).is_integer() and lm._step_index(t) == 1 and lm._step_index(float(np.float32(t))) == 1
    with pytest.raises(ValueError, match="is not one of this schedule's"):
        lm._step_index(998.0)


# ---------------------------------------------------------------------------------------------------- configs
def test_config_conversion_and_pipelines():
    from baddiffusion_amd.pipelines import HeunPipeline, LMSPipeline, PNDMPipeline, _MultistepPipeline, _SigmaPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler, HeunDiscreteScheduler, LMSDiscreteScheduler, SchedulerConfigCarrier
    import inspect
    ddpm = DDPMScheduler(num_train_timesteps=400, beta_start=0.0002, beta_end=0.03, beta_schedule="scaled_linear")
    for cls, pipe in ((HeunDiscreteScheduler, HeunPipeline), (LMSDiscreteScheduler, LMSPipeline)):
        s = cls.from_config(ddpm.config)
        assert set(s.config) == set(cls._KEYS) and len(s) == 400 and s.order == 1 and torch.equal(s.betas, ddpm.betas)
        assert s.config.prediction_type == "epsilon" and s.num_train_timesteps == 400
        p = pipe(_NoUNet(), ddpm)
        assert type(p.scheduler) is cls and torch.equal(p.scheduler.betas, ddpm.betas) and p.clip_sample is False
        assert pipe(_NoUNet(), s, clip_sample=True).scheduler is s
        assert type(pipe(_NoUNet(), SchedulerConfigCarrier(cls.__name__)).scheduler) is cls
        assert issubclass(pipe, _SigmaPipeline) and issubclass(pipe, _MultistepPipeline) and "_sample" not in vars(pipe)
        sig, pndm = inspect.signature(pipe.__call__), inspect.signature(PNDMPipeline.__call__)
        assert list(sig.parameters) == list(pndm.parameters)
        assert pipe(_NoUNet(), s).noise_draws() == 0
    assert HeunPipeline.default_steps == 10 and LMSPipeline.default_steps == 20           # what a call that names no count runs
    assert all(inspect.signature(p.__call__).parameters["num_inference_steps"].default is None and "__call__" not in vars(p)
               for p in (HeunPipeline, LMSPipeline))
    assert LMSPipeline(_NoUNet(), ddpm).order == 4 and LMSPipeline(_NoUNet(), ddpm, order=2).order == 2
    with pytest.raises(ValueError, match="order must be 1..4"):
        LMSPipeline(_NoUNet(), ddpm, order=5)


@pytest.mark.parametrize("sampler", ("heun", "lms"))
def test_load_and_save_scheduler_round_trip(sampler, tmp_path):
    from baddiffusion_amd.model import load_scheduler, save_scheduler
    s = _sched(sampler, num_train_timesteps=400, beta_schedule="scaled_linear", beta_end=0.03)
    s.config.clip_sample = True                      # what DiffuserModelSched attaches to every scheduler it returns
    save_scheduler(s, str(tmp_path))
    saved = json.load(open(os.path.join(str(tmp_path), "scheduler_config.json")))
    assert saved["_class_name"] == type(s).__name__ and saved["num_train_timesteps"] == 400 and saved["beta_end"] == 0.03
    back = load_scheduler(str(tmp_path))
    assert type(back) is type(s) and {k: back.config[k] for k in s._KEYS} == {k: s.config[k] for k in s._KEYS}
    assert torch.equal(back.sigmas, s.sigmas)


def test_errors_are_loud():
    from baddiffusion_amd.pipelines import HeunPipeline
    x = torch.zeros(2, 3, 8, 8)
    for sampler in ("heun", "lms"):
        s = _sched(sampler)
        with pytest.raises(ValueError, match="Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler"):
            s.step(x, 999.0, x)
        s.set_timesteps(5)
        with pytest.raises(RuntimeError, match=r"Scheduler\.step runs on the GPU only"):
            s.step(x, 999.0, x)
        with pytest.raises(RuntimeError, match=r"scale_model_input runs on the GPU only"):
            s.scale_model_input(x, 999.0)
        v = _sched(sampler, prediction_type="v_prediction")
        v.set_timesteps(5)
        with pytest.raises(ValueError, match="must be `epsilon` on the HIP path"):
            v.step(x, 999.0, x)
    # an odd start is the averaging stage of a transition whose first stage was not run: refused before anything is drawn or launched
    p = HeunPipeline(_NoUNet(), _sched("heun"))
    for k in (1, 3):
        with pytest.raises(ValueError, match=f"start_from={k} is the second entry of a timestep pair"):
            p(batch_size=1, num_inference_steps=5, start_from=k)


# ---------------------------------------------------------------------------------------------------- wiring
def test_sched_name_wiring():
    from baddiffusion_amd.model import DiffuserModelSched
    from baddiffusion_amd.pipelines import HeunPipeline, LMSPipeline, PNDMPipeline
    from baddiffusion_amd.schedulers import HeunDiscreteScheduler, LMSDiscreteScheduler, PNDMScheduler, SchedulerConfigCarrier
    from baddiffusion_amd.sched_names import SCHEDS
    # Heun's order is no parameter of its record: it is what the class does
    assert {n: (r.scheduler.__name__, r.pipe_kw.get("order", 2 if r.scheduler is HeunDiscreteScheduler else None))
            for n, r in SCHEDS.items() if r.scheduler in (HeunDiscreteScheduler, LMSDiscreteScheduler)} == SIGMA_NAMES
    assert all(SCHEDS[n].carrier is None and not SCHEDS[n].native_only for n in SIGMA_NAMES)     # no PNDM conversion, not native-only
    get = lambda name, **kw: DiffuserModelSched.get_pretrained("DDPM-CIFAR10-32", noise_sched_type=name, allow_random_init=True, **kw)
    for name, (cls_name, order) in SIGMA_NAMES.items():
        cls, pipe = (HeunDiscreteScheduler, HeunPipeline) if cls_name == "HeunDiscreteScheduler" else (LMSDiscreteScheduler, LMSPipeline)
        for native in (False, True):
            m, s, gp = get(name, clip_sample=True, native_sched=native)
            assert type(s) is cls and type(s).__name__ == cls_name
            assert s.config.num_train_timesteps == 1000 and torch.equal(s.betas, torch.linspace(0.0001, 0.02, 1000))
            p = gp(m, s)
            assert type(p) is pipe and p.scheduler is s and p.clip_sample is True
            assert getattr(p, "order", 2) == order
            del m, p
    m, s, gp = get("LMSD_O3-SCHED", clip_sample=False)
    assert gp(m, s).clip_sample is False
    del m
    # the reference's own names are unchanged: the config carrier + PNDM without the opt-in, refused with it
    for name, cls_name in (("HEUN-SCHED", "HeunDiscreteScheduler"), ("LMSD-SCHED", "LMSDiscreteScheduler")):
        m, s, gp = get(name, clip_sample=True)
        assert type(s) is SchedulerConfigCarrier and s.class_name == cls_name
        p = gp(m, s)
        assert type(p) is PNDMPipeline and type(p.scheduler) is PNDMScheduler
        del m, p
        with pytest.raises(NotImplementedError, match=name):
            get(name, native_sched=True)


def test_cli_accepts_the_names_and_args_json_round_trips(tmp_path, monkeypatch):
    """the same behaviour as UNIPC_O2-SCHED: accepted in training, kept in args.json, inherited by sampling / measure, where
    --infer_steps and --native_sched are on the whitelist"""
    import baddiffusion as cli
    monkeypatch.chdir(tmp_path)
    assert set(SIGMA_NAMES) < set(cli.SCHED_CHOICES) and "HEUN-SCHED" in cli.SCHED_CHOICES
    base = ["--project", "default", "--dataset", "CIFAR10", "--batch", "64", "--ckpt", "DDPM-CIFAR10-32", "-o"]
    for name in list(SIGMA_NAMES) + ["UNIPC_O2-SCHED"]:
        cfg = cli.setup(["--mode", "train", "--sched", name, "--infer_steps", "10"] + base)
        assert cfg.sched == name and cfg.native_sched is False and cfg.infer_steps == 10
        saved = json.load(open(os.path.join(cfg.output_dir, "args.json")))
        assert saved["sched"] == name and saved["infer_steps"] == 10
        for mode in ("sampling", "measure"):
            c = cli.setup(["--mode", mode, "--ckpt", cfg.output_dir, "--infer_steps", "15"], write=False)
            assert c.sched == name and c.infer_steps == 15
            assert cli.setup(["--mode", mode, "--ckpt", cfg.output_dir], write=False).infer_steps == 10
            assert cli.setup(["--mode", mode, "--ckpt", cfg.output_dir, "--native_sched"], write=False).sched == name
    for bad in ("LMSD_O5-SCHED", "HEUN_O1-SCHED"):
        with pytest.raises(SystemExit):
            cli.parse_args(["--mode", "train", "--sched", bad])


def test_help_says_where_the_sigma_samplers_live(capsys):
    import baddiffusion as cli
    with pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    text = "".join(capsys.readouterr().out.split())
    assert "HEUN_O2-SCHED" in text and "HeunPipeline" in text and "LMSPipeline" in text and "DEIS" in text


def test_elijah_defense_accepts_the_names(tmp_path):
    import elijah_defense as E
    from baddiffusion_amd.pipelines import HeunPipeline, LMSPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    assert set(SIGMA_NAMES) < set(E.SCHED_CHOICES) and "HEUN-SCHED" not in E.SCHED_CHOICES
    ckpt_sched = DDPMScheduler(num_train_timesteps=400)
    for name, (cls_name, order) in SIGMA_NAMES.items():
        cfg = E.get_config(["--ckpt", "x", "--sched", name, "--infer_steps", "12", "--output_dir", str(tmp_path)])
        assert cfg.sched == name and cfg.infer_steps == 12
        p = E.make_pipeline(cfg, _NoUNet(), ckpt_sched)
        assert type(p) is (HeunPipeline if cls_name == "HeunDiscreteScheduler" else LMSPipeline)
        assert type(p.scheduler).__name__ == cls_name and getattr(p, "order", 2) == order
        assert torch.equal(p.scheduler.betas, ckpt_sched.betas)


# ---------------------------------------------------------------------------------------------------- the C ABI
def _desc(L, **kw):
    d = L.SigmaStepDesc(n=16, model_output=4096, sample=8192, base=12288, h1=16384, h2=20480, h3=24576, x0_out=28672, d_out=32768,
                        prev_out=36864, scaled_out=40960, sigma_in=2.0, average=0, c0=1.0, c1=1.0, c2=1.0, c3=1.0, in_div=1.5)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_sigma_step_rejects_bad_arguments_without_gpu():
    """the argument checks run on the host before any launch: negative status and a bd_last_error that names the entry point"""
    from baddiffusion_amd import _lib as L
    lib, INVALID = L.load(), -1
    assert lib.bd_sigma_step(None, None) == INVALID and b"bd_sigma_step: null descriptor" in lib.bd_last_error()
    avg = dict(average=1, h2=None, h3=None, c1=0.0, c2=0.0, c3=0.0)
    cases = [(dict(n=0), b"n=0"), (dict(n=-4), b"n=-4"), (dict(model_output=None), b"null pointer"), (dict(sample=None), b"null pointer"),
             (dict(prev_out=None), b"null pointer"), (dict(sigma_in=0.0), b"sigma_in=0 must be positive"),
             (dict(sigma_in=-1.0), b"sigma_in=-1 must be positive"), (dict(sigma_in=float("nan")), b"sigma_in"),
             (dict(in_div=0.0), b"in_div=0 must be positive"), (dict(in_div=-2.0), b"in_div=-2 must be positive"),
             ({**avg, "h1": None}, b"average without h1"),
             ({**avg, "h2": 20480}, b"average with history terms"), ({**avg, "h3": 24576}, b"average with history terms"),
             ({**avg, "c1": 0.5}, b"average with history terms"), ({**avg, "c2": 0.5}, b"average with history terms"),
             ({**avg, "c3": 0.5}, b"average with history terms"),
             (dict(h1=None), b"history with a gap"), (dict(h2=None), b"history with a gap"),
             (dict(model_output=4100), b"model_output is not 16-byte aligned"), (dict(sample=8200), b"sample is not 16-byte aligned"),
             (dict(base=12292), b"base is not 16-byte aligned"), (dict(h1=16388), b"h1 is not 16-byte aligned"),
             (dict(h2=20488), b"h2 is not 16-byte aligned"), (dict(h3=24580), b"h3 is not 16-byte aligned"),
             (dict(x0_out=28676), b"x0_out is not 16-byte aligned"), (dict(d_out=32776), b"d_out is not 16-byte aligned"),
             (dict(prev_out=36868), b"prev_out is not 16-byte aligned"), (dict(scaled_out=40964), b"scaled_out is not 16-byte aligned"),
             # partial overlaps: 16 floats = 64 bytes
             (dict(prev_out=8192 + 16), b"prev_out overlaps sample"), (dict(prev_out=8192 - 48), b"prev_out overlaps sample"),
             (dict(prev_out=4096 + 32), b"prev_out overlaps model_output"), (dict(prev_out=12288 + 16), b"prev_out overlaps base"),
             (dict(d_out=24576 + 16), b"d_out overlaps h3"), (dict(d_out=20480 - 16), b"d_out overlaps h2"),
             (dict(d_out=16384 + 48), b"d_out overlaps h1"), (dict(scaled_out=8192 - 16), b"scaled_out overlaps sample"),
             (dict(x0_out=4096 + 16), b"x0_out overlaps model_output"),
             # outputs among themselves: never, not even by identical base
             (dict(d_out=36864), b"d_out overlaps prev_out"), (dict(scaled_out=36864 + 48), b"scaled_out overlaps prev_out"),
             (dict(scaled_out=32768), b"scaled_out overlaps d_out"), (dict(d_out=28672 + 16), b"d_out overlaps x0_out"),
             (dict(x0_out=8192, prev_out=8192), b"x0_out overlaps prev_out")]
    for kw, what in cases:
        assert lib.bd_sigma_step(ctypes.byref(_desc(L, **kw)), None) == INVALID, kw
        msg = lib.bd_last_error()
        assert b"bd_sigma_step" in msg and what in msg, (kw, msg)


def test_scale_input_and_embedding_reject_bad_arguments_without_gpu():
    from baddiffusion_amd import _lib as L
    lib, INVALID = L.load(), -1
    for args, what in (((None, 16, 1.0, 1.0, 8192, None), b"null pointer"), ((4096, 16, 1.0, 1.0, None, None), b"null pointer"),
                       ((4096, 0, 1.0, 1.0, 8192, None), b"n=0"), ((4096, -1, 1.0, 1.0, 8192, None), b"n=-1"),
                       ((4096, 16, 1.0, 0.0, 8192, None), b"div=0 must be positive"),
                       ((4096, 16, 1.0, -1.0, 8192, None), b"div=-1 must be positive"),
                       ((4100, 16, 1.0, 1.0, 8192, None), b"16-byte aligned"), ((4096, 16, 1.0, 1.0, 8200, None), b"16-byte aligned"),
                       ((4096, 16, 1.0, 1.0, 4096 + 16, None), b"out overlaps x"), ((4096, 16, 1.0, 1.0, 4096 - 48, None), b"out overlaps x")):
        assert lib.bd_scale_input(*args) == INVALID, args
        msg = lib.bd_last_error()
        assert b"bd_scale_input" in msg and what in msg, (args, msg)
    for args in ((None, 1, 2, 32, 1, 0.0, 8192, None), (4096, 1, 2, 32, 1, 0.0, None, None), (4096, 1, 0, 32, 1, 0.0, 8192, None),
                 (4096, 1, -2, 32, 1, 0.0, 8192, None), (4096, 1, 2, 1, 1, 0.0, 8192, None), (4096, 1, 2, 0, 1, 0.0, 8192, None)):
        assert lib.bd_timestep_embedding_f32(*args) == INVALID, args
        assert b"bd_timestep_embedding_f32: bad args" in lib.bd_last_error()
        assert lib.bd_timestep_embedding(*args) == INVALID, args              # the same host checks as the int64 entry point
        assert b"bd_timestep_embedding: bad args" in lib.bd_last_error()


def test_unet_forward_tf_rejects_bad_arguments_without_gpu():
    """the plan is a host object: the checks of bd_unet_forward_tf are those of bd_unet_forward, under its own name"""
    from baddiffusion_amd import _lib as L
    from baddiffusion_amd.unet import unet_from_config
    lib, INVALID, WORKSPACE = L.load(), -1, -4
    m = unet_from_config(C.SMALL_CFGS["small"])
    plan, nbytes = m._plan, m.workspace_bytes(1, False)
    ws = np.empty(nbytes + 16, dtype=np.uint8)
    wp = (ws.ctypes.data + 15) & ~15
    ok = dict(u=plan, B=1, training=0, params=4096, x=8192, ldx=3, t=12288, t_stride=0, out=16384, ldo=3, ws=wp, nbytes=nbytes)

    def call(fn, **kw):
        a = {**ok, **kw}
        return fn(a["u"], a["B"], a["training"], a["params"], a["x"], a["ldx"], a["t"], a["t_stride"], a["out"], a["ldo"], a["ws"],
                  a["nbytes"], None)

    for fn, name in ((lib.bd_unet_forward_tf, b"bd_unet_forward_tf"), (lib.bd_unet_forward, b"bd_unet_forward")):
        for kw, status, what in ((dict(u=None), INVALID, b"bd_unet: null plan"), (dict(B=0), INVALID, b"bd_unet: B must be > 0"),
                                 (dict(ws=None), WORKSPACE, b"bd_unet: workspace"), (dict(nbytes=nbytes - 1), WORKSPACE, b"bd_unet: workspace"),
                                 (dict(ws=wp + 4), INVALID, b"workspace must be 16-byte aligned"),
                                 (dict(params=None), INVALID, name + b": null pointer"), (dict(x=None), INVALID, name + b": null pointer"),
                                 (dict(t=None), INVALID, name + b": null pointer"), (dict(out=None), INVALID, name + b": null pointer"),
                                 (dict(ldx=2), INVALID, name + b": ld < channels"), (dict(ldo=2), INVALID, name + b": ld < channels"),
                                 (dict(params=4100), INVALID, name + b": params must be 16-byte aligned")):
            assert call(fn, **kw) == status, (name, kw)
            msg = lib.bd_last_error()
            assert what in msg, (name, kw, msg)


def test_descriptor_layout_matches_the_header():
    from baddiffusion_amd import _lib as L
    fields = ("base", "h3", "x0_out", "d_out", "prev_out", "scaled_out", "sigma_in", "average", "c0", "c3", "in_div", "clip", "clip_range")
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "bd_hip.h"\nint main(){printf("%zu", sizeof(bd_sigma_step_desc));' + \
           "".join(f'printf(" %zu", offsetof(bd_sigma_step_desc, {f}));' for f in fields) + 'printf("\\n");return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    D = L.SigmaStepDesc
    assert got == [ctypes.sizeof(D)] + [getattr(D, f).offset for f in fields]

