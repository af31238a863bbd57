"""CPU: the host side of DEIS sampling -- the timestep tables and every stand-in chain of the reference (tests/golden/deis.npz, written
by make_golden_deis.py from the imported diffusers DEISMultistepScheduler) against DEISMultistepScheduler._plan driven through a torch
restatement of bd_deis_step's formula (cases_deis.kernel_formula), the `coefficient_dtype="float64"` mode against the recurrence in
float64 at 1000 steps, the sequence of orders, configuration and persistence, what is rejected before any launch, the wiring of the
DEIS_O*-SCHED names (model.py, baddiffusion.py, elijah_defense.py) and the C ABI's argument checks.  Nothing here needs a GPU."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests.golden import cases as C
from tests.golden import cases_deis as CD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEIS_NAMES = {"DEIS_O1-SCHED": 1, "DEIS_O2-SCHED": 2, "DEIS_O3-SCHED": 3}


class _NoUNet:
    """what a pipeline needs of a UNet before its first evaluation"""
    device = torch.device("cpu")


def _sched(**kw):
    from baddiffusion_amd.schedulers import DEISMultistepScheduler
    return DEISMultistepScheduler(**kw)


def restated_chain(s, n, x0_clip=False):
    """the chain of `s` over the stand-in model through kernel_formula: yields (step, plan, sample)"""
    s.set_timesteps(n)
    x, hist = C.pndm_init(), []
    for i, t in enumerate(s.timesteps.tolist()):
        plan = s._plan(i)
        m0, x = CD.kernel_formula(plan, x0_clip, C.pndm_fake_model(x, t), x, hist)
        hist = [m0] + hist[:1]
        s._advance()
        yield i, plan, x


def expected_orders(order, n, lower_order_final=True):
    """scheduling_deis_multistep.py:441-468: warm-up, and below 15 steps the last two steps at second and first order"""
    want = []
    for i in range(n):
        o = min(order, i + 1)
        if lower_order_final and n < 15:
            o = min(o, n - i)
        want.append(o)
    return want


# ---------------------------------------------------------------------------------------------------- timesteps
@pytest.mark.parametrize("n", CD.TIMESTEP_NS)
def test_timesteps_equal_the_reference(n, golden):
    s = _sched()
    s.set_timesteps(n)
    want = golden("deis")[f"ts_{n}"]
    assert s.timesteps.dtype == torch.int64 and np.array_equal(s.timesteps.numpy(), want)
    assert s.num_inference_steps == len(want)


def test_timestep_fixture_is_the_documented_one(golden):
    g = golden("deis")
    assert g["ts_4"].tolist() == [999, 749, 500, 250] and g["ts_1"].tolist() == [999]
    assert len(g["ts_1000"]) == 999 and len(set(g["ts_1000"].tolist())) == 999           # the duplicate is removed
    s = _sched(solver_order=3)
    s.set_timesteps(10)
    s.lower_order_nums, s._ring = 2, [None, torch.zeros(1), torch.zeros(1)]
    s.set_timesteps(1000)
    assert s.num_inference_steps == 999 and s.lower_order_nums == 0 and s._ring == [None] * 3      # history and warm-up reset


# ---------------------------------------------------------------------------------------------------- chains
def test_chain_fixture_covers_the_documented_cases(golden):
    g = golden("deis")
    assert len(CD.CHAIN_CASES) == 12 and all(f"chain_{CD.chain_tag(*c)}" in g.files for c in CD.CHAIN_CASES)
    assert len({CD.chain_tag(*c) for c in CD.CHAIN_CASES}) == 12
    assert max(float(g[f"chain_dev64_{CD.chain_tag(*c)}"]) for c in CD.CHAIN_CASES) < 2e-5
    # orders 2 and 3 give the same chain at 4 steps: the third order is never reached
    assert np.array_equal(g[f"chain_{CD.chain_tag(2, 4, False)}"], g[f"chain_{CD.chain_tag(3, 4, False)}"])
    for o, n in CD.LONG_CASES:
        tag = CD.chain_tag(o, n, False)
        assert g[f"long64_{tag}"].dtype == np.float64 and len(g[f"long64_{tag}"]) == len(CD.long_steps(999)) == 27
    # what coefficient_dtype is about: the reference's own chain is 0.26 * max|x| from the recurrence at order 3, 1000 steps
    assert float(g["long_ref32_o3_n1000"]) > 0.1 and float(g["long_yard_o3_n1000"]) < 1e-5
    assert float(g["long_ref32_o2_n1000"]) > 1e-4 and float(g["long_yard_o2_n1000"]) < 1e-5
    assert len(CD.UNET_CASES) == 6 and all(f"{CD.unet_tag(*c)}_sample" in g.files for c in CD.UNET_CASES)


@pytest.mark.parametrize("case", CD.CHAIN_CASES, ids=lambda c: CD.chain_tag(*c))
def test_plan_reproduces_the_reference_chain(case, golden):
    """_plan's scalars through the kernel's formula: every intermediate sample within max(4e-6, 4 * dev64) * max|ref| of the
    reference's, dev64 being the reference's own distance from the recurrence in fp64 (the bound of the DPM-Solver, UniPC and RePaint
    stand-in chains).  Whether the chain is the reference's bit for bit is printed, not asserted: the coefficients go through numpy's
    log, and another build of it may move a last bit"""
    order, n, thr = case
    g, tag = golden("deis"), CD.chain_tag(*case)
    ref, dev64 = g[f"chain_{tag}"], float(g[f"chain_dev64_{tag}"])
    bound = max(4e-6, 4 * dev64)
    s = _sched(**CD.scheduler_kwargs(order, thr))
    assert s.config.coefficient_dtype == "float32"
    seq, worst, exact = [], 0.0, True
    for i, plan, x in restated_chain(s, n, thr):
        seq.append(plan[0])
        dev = float(np.abs(x.numpy() - ref[i]).max() / np.abs(ref[i]).max())
        worst, exact = max(worst, dev), exact and np.array_equal(x.numpy(), ref[i])
        assert dev <= bound, (i, dev, bound)
    assert len(ref) == n and seq == expected_orders(order, n) and s.lower_order_nums == order
    print(f"MEASURE deis stand-in chain {tag} (host formula): worst step deviation {worst:.3e}, bound {bound:.3e}, bit-exact: {exact}")


@pytest.mark.parametrize("case", CD.LONG_CASES, ids=lambda c: CD.chain_tag(*c, False))
def test_float64_coefficients_follow_the_fp64_recurrence(case, golden):
    """coefficient_dtype="float64" at 1000 steps: within 4 x the recorded yardstick (the generator's own float64 coefficients through
    the same fp32 formula), floor 4e-6, of the stored recurrence in float64, at every stored step; and at order 3 the default mode,
    which is the reference's arithmetic, is farther away than that (the reference itself: 4.04 against 4.7e-5 in absolute terms)"""
    order, n = case
    g, tag = golden("deis"), CD.chain_tag(order, n, False)
    ref, yard = g[f"long64_{tag}"], float(g[f"long_yard_{tag}"])
    bound = max(4e-6, 4 * yard)
    keep = {i: j for j, i in enumerate(CD.long_steps(999))}
    dist = {}
    for mode in ("float64", "float32"):
        worst = 0.0
        for i, _, x in restated_chain(_sched(solver_order=order, coefficient_dtype=mode), n):
            if i in keep:
                worst = max(worst, float(np.abs(x.double().numpy() - ref[keep[i]]).max() / np.abs(ref[keep[i]]).max()))
        dist[mode] = worst
    print(f"MEASURE deis {tag} vs the fp64 recurrence (host formula): float64 coefficients {dist['float64']:.3e} (bound {bound:.3e}, "
          f"yardstick {yard:.3e}), reference arithmetic {dist['float32']:.3e} (the reference itself {float(g[f'long_ref32_{tag}']):.3e})")
    assert dist["float64"] <= bound
    if order == 3:
        assert dist["float32"] > dist["float64"]


def test_order_sequences():
    def orders(order, n, **kw):
        s = _sched(solver_order=order, **kw)
        s.set_timesteps(n)
        got = ""
        for i in range(s.num_inference_steps):
            got += str(s._plan(i)[0])
            s._advance()
        return got
    assert orders(3, 10) == "1233333321"
    assert orders(3, 20) == "12" + "3" * 18                   # 15 steps and more: no lower-order ending
    assert orders(2, 4) == orders(3, 4) == "1221"
    assert orders(1, 10) == "1" * 10 and orders(2, 20) == "1" + "2" * 19
    assert orders(3, 5, lower_order_final=False) == "12333"
    assert orders(3, 1) == "1" and orders(3, 2) == "11" and orders(3, 3) == "121"
    for order in (1, 2, 3):
        for n in (1, 2, 3, 4, 10, 14, 15, 20):
            assert orders(order, n) == "".join(map(str, expected_orders(order, n))), (order, n)
    # start_from=k (the pipeline steps a fresh state from timestep k on): the warm-up starts there
    s = _sched(solver_order=3)
    s.set_timesteps(10)
    got = []
    for i in range(6, 10):
        got.append(s._plan(i)[0])
        s._advance()
    assert got == [1, 2, 2, 1]


def test_plan_scalars_are_the_reference_expressions():
    """first order: the closed form of :298-303 on fp32 scalars; the conversion scalars are the table's; the float64 mode rounds the
    same expressions once; the plan is kept per schedule, state and mode"""
    s = _sched(solver_order=2)
    s.set_timesteps(10)
    ts = s.timesteps.tolist()
    order, alpha_s, sigma_s, cx, c0, alpha_t, k0, k1, k2 = s._plan(0)
    h = s.lambda_t[ts[1]] - s.lambda_t[ts[0]]
    assert (order, alpha_t, k0, k1, k2) == (1, 0.0, 0.0, 0.0, 0.0)
    assert alpha_s == float(s.alpha_t[ts[0]]) and sigma_s == float(s.sigma_t[ts[0]])
    assert cx == float(s.alpha_t[ts[1]] / s.alpha_t[ts[0]]) and c0 == float(s.sigma_t[ts[1]] * (torch.exp(h) - 1.0))
    assert s.alpha_t.dtype == s.sigma_t.dtype == s.lambda_t.dtype == torch.float32
    kept = s._plan(0)
    assert s._plan(0) is kept and kept == s._plan_scalars(0)
    s._advance()
    p1 = s._plan(1)
    assert p1[0] == 2 and p1[3:5] == (0.0, 0.0) and p1[5] == float(s.alpha_t[ts[2]]) and p1[8] == 0.0 and p1[6] != 0.0 and p1[7] != 0.0
    s.config.coefficient_dtype = "float64"                    # an assigned option is seen, and kept apart
    w1 = s._plan(1)
    assert w1 is not p1 and w1[:3] == p1[:3] and w1[5] == p1[5]
    # the two second order coefficients integrate a partition of unity, k0 + k1 = rho_t - rho_s0: in float64 up to the one rounding
    # of each to fp32
    rho = lambda t: float(s.sigma_t[t].double() / s.alpha_t[t].double())      # noqa: E731
    assert abs(w1[6] + w1[7] - (rho(ts[2]) - rho(ts[1]))) <= 1.01 * 2.0 ** -24 * (abs(w1[6]) + abs(w1[7]))
    assert all(float(np.float32(v)) == v for v in w1[1:])     # rounded once to fp32
    s.set_timesteps(10)                                       # the same schedule again: kept
    assert s._plan(0) is not kept and s._plan(0)[:3] == kept[:3]
    s.config.coefficient_dtype = "float32"
    assert s._plan(0) is kept
    s.set_timesteps(20)                                       # another schedule: recomputed
    assert s._plans == {}
    # the last step goes to timestep 0, not past it
    s = _sched(solver_order=1)
    s.set_timesteps(10)
    ts = s.timesteps.tolist()
    assert s._plan(9)[3] == float(s.alpha_t[0] / s.alpha_t[ts[9]])


# ---------------------------------------------------------------------------------------------------- configuration
def test_config_conversion():
    from baddiffusion_amd.pipelines import DEISPipeline, _MultistepPipeline
    from baddiffusion_amd.schedulers import (DDPMScheduler, DEISMultistepScheduler, DPMSolverMultistepScheduler, SchedulerConfigCarrier,
                                             UniPCMultistepScheduler)
    ref_cfg = {"num_train_timesteps": 500, "beta_start": 0.0002, "beta_end": 0.03, "beta_schedule": "scaled_linear", "trained_betas": None,
               "solver_order": 3, "prediction_type": "epsilon", "thresholding": False, "dynamic_thresholding_ratio": 0.995,
               "sample_max_value": 1.0, "algorithm_type": "deis", "solver_type": "logrho", "lower_order_final": False,
               "_class_name": "DEISMultistepScheduler"}
    s = DEISMultistepScheduler.from_config(ref_cfg)
    assert {k: s.config[k] for k in ref_cfg if not k.startswith("_")} == {k: v for k, v in ref_cfg.items() if not k.startswith("_")}
    assert set(s.config) == set(DEISMultistepScheduler._KEYS) and len(s) == 500 and s.order == 1
    assert s.config.coefficient_dtype == "float32"            # a reference config has none: the reference's arithmetic
    assert DEISMultistepScheduler.from_config({**ref_cfg, "coefficient_dtype": "float64"}).config.coefficient_dtype == "float64"
    d = _sched()                                              # the reference's defaults
    assert (d.config.solver_order, d.config.algorithm_type, d.config.solver_type, d.config.lower_order_final) == (2, "deis", "logrho", True)
    # sibling configs convert (scheduling_deis_multistep.py:155-165)
    dpm = DPMSolverMultistepScheduler(num_train_timesteps=400, solver_order=3, algorithm_type="dpmsolver", solver_type="heun", thresholding=True)
    c = DEISMultistepScheduler.from_config(dpm.config)
    assert (c.config.algorithm_type, c.config.solver_type, c.config.solver_order, c.config.thresholding) == ("deis", "logrho", 3, True)
    assert torch.equal(c.betas, dpm.betas) and torch.equal(c.lambda_t, dpm.lambda_t)
    for st in ("bh1", "bh2"):
        u = DEISMultistepScheduler.from_config(UniPCMultistepScheduler(solver_type=st, solver_order=1).config)
        assert (u.config.algorithm_type, u.config.solver_type, u.config.solver_order) == ("deis", "logrho", 1)
    for at in ("dpmsolver", "dpmsolver++"):
        assert _sched(algorithm_type=at, solver_type="midpoint").config.algorithm_type == "deis"
    # and back: a DEIS config builds the siblings
    assert DPMSolverMultistepScheduler.from_config(s.config).config.algorithm_type == "dpmsolver++"
    assert UniPCMultistepScheduler.from_config(s.config).config.solver_type == "bh1"
    with pytest.raises(NotImplementedError, match="unipc does is not implemented for"):
        _sched(algorithm_type="unipc")
    with pytest.raises(NotImplementedError, match="solver type euler does is not implemented for"):
        _sched(solver_type="euler")
    for bad in (4, 0):
        with pytest.raises(ValueError, match=f"solver_order must be 1, 2 or 3, got {bad}"):
            _sched(solver_order=bad)
    with pytest.raises(ValueError, match="coefficient_dtype"):
        _sched(coefficient_dtype="float16")
    with pytest.raises(NotImplementedError, match="sample_max_value"):
        _sched(thresholding=True, sample_max_value=2.0)
    assert _sched(thresholding=True, sample_max_value=1.0).config.thresholding is True
    with pytest.raises(NotImplementedError):
        _sched(beta_schedule="squaredcos_cap_v2")
    # the pipeline converts any other scheduler from its config and keeps a DEIS scheduler as it is
    ddpm = DDPMScheduler(num_train_timesteps=400, clip_sample=False)
    p = DEISPipeline(_NoUNet(), ddpm)
    assert type(p.scheduler) is DEISMultistepScheduler and torch.equal(p.scheduler.betas, ddpm.betas)
    assert p.clip_sample is False and p.clip_sample_range == 1.0
    assert type(DEISPipeline(_NoUNet(), SchedulerConfigCarrier("DEISMultistepScheduler")).scheduler) is DEISMultistepScheduler
    assert DEISPipeline(_NoUNet(), s, clip_sample=True).scheduler is s
    assert DEISPipeline.default_steps == 10 and issubclass(DEISPipeline, _MultistepPipeline)
    assert "__call__" not in vars(DEISPipeline) and "_sample" not in vars(DEISPipeline)       # the loop is _MultistepPipeline's


def test_errors_are_loud():
    x = torch.zeros(2, 3, 8, 8)
    s = _sched()
    with pytest.raises(ValueError, match="Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler"):
        s.step(x, 999, x)
    with pytest.raises(ValueError, match="Number of inference steps is 'None'"):
        s._plan(0)
    s.set_timesteps(10)
    with pytest.raises(RuntimeError, match=r"DEISMultistepScheduler\.step runs on the GPU only"):
        s.step(x, 999, x)
    for kind in ("sample", "v_prediction"):
        v = _sched(prediction_type=kind)
        v.set_timesteps(10)
        with pytest.raises(ValueError, match="prediction_type"):
            v.step(x, 999, x)
    from baddiffusion_amd import ops
    with pytest.raises(RuntimeError):
        ops.deis_step(x, x, 0.8, 0.6, cx=1.0, c0=1.0)


def test_load_and_save_scheduler_round_trip(tmp_path):
    from baddiffusion_amd.model import load_scheduler, save_scheduler
    from baddiffusion_amd.schedulers import DEISMultistepScheduler
    s = _sched(num_train_timesteps=400, beta_schedule="scaled_linear", solver_order=3, lower_order_final=False, thresholding=True,
               coefficient_dtype="float64")
    save_scheduler(s, str(tmp_path / "scheduler"))
    saved = json.load(open(tmp_path / "scheduler" / "scheduler_config.json"))
    assert saved["_class_name"] == "DEISMultistepScheduler" and saved["solver_order"] == 3 and saved["coefficient_dtype"] == "float64"
    assert saved["algorithm_type"] == "deis" and saved["solver_type"] == "logrho"
    back = load_scheduler(str(tmp_path / "scheduler"))
    assert type(back) is DEISMultistepScheduler and dict(back.config) == dict(s.config)
    assert torch.equal(back.betas, s.betas) and torch.equal(back.lambda_t, s.lambda_t)


# ---------------------------------------------------------------------------------------------------- wiring
def test_sched_name_wiring():
    from baddiffusion_amd.model import DiffuserModelSched
    from baddiffusion_amd.pipelines import DEISPipeline, PNDMPipeline
    from baddiffusion_amd.schedulers import DEISMultistepScheduler, PNDMScheduler, SchedulerConfigCarrier
    D = DiffuserModelSched
    from baddiffusion_amd.sched_names import SCHEDS
    assert {n: r.sched_kw["solver_order"] for n, r in SCHEDS.items() if r.scheduler is DEISMultistepScheduler} == DEIS_NAMES
    # no PNDM conversion, not native-only, not refused
    assert all(SCHEDS[n].carrier is None and not SCHEDS[n].native_only and SCHEDS[n].refused is None for n in DEIS_NAMES)
    get = lambda name, **kw: D.get_pretrained("DDPM-CIFAR10-32", noise_sched_type=name, allow_random_init=True, **kw)      # noqa: E731
    for name, order in DEIS_NAMES.items():
        for native in (False, True):
            m, s, gp = get(name, clip_sample=True, native_sched=native)
            assert type(s) is DEISMultistepScheduler
            assert (s.config.solver_order, s.config.algorithm_type, s.config.solver_type, s.config.coefficient_dtype) == \
                (order, "deis", "logrho", "float32")
            assert s.config.num_train_timesteps == 1000 and torch.equal(s.betas, torch.linspace(0.0001, 0.02, 1000))
            p = gp(m, s)
            assert type(p) is DEISPipeline and p.scheduler is s and p.clip_sample is True
            del m, p
    m, s, gp = get("DEIS_O2-SCHED", clip_sample=False)
    assert gp(m, s).clip_sample is False
    m, s, gp = D.get_model_sched(image_size=32, channels=3, model_type=D.DDPM_CIFAR10_DEFAULT, noise_sched_type="DEIS_O3-SCHED")
    assert type(s) is DEISMultistepScheduler and type(gp(m, s)) is DEISPipeline
    del m
    # the reference's own name is unchanged: the config carrier + PNDM without the opt-in, refused with it
    m, s, gp = get("DEIS-SCHED", clip_sample=True)
    assert type(s) is SchedulerConfigCarrier and s.class_name == "DEISMultistepScheduler"
    p = gp(m, s)
    assert type(p) is PNDMPipeline and type(p.scheduler) is PNDMScheduler
    with pytest.raises(NotImplementedError, match="DEIS-SCHED"):
        get("DEIS-SCHED", native_sched=True)


def test_cli_accepts_the_names_and_args_json_round_trips(tmp_path, monkeypatch):
    import baddiffusion as cli
    monkeypatch.chdir(tmp_path)
    assert set(DEIS_NAMES) < set(cli.SCHED_CHOICES) and "DEIS-SCHED" in cli.SCHED_CHOICES
    base = ["--project", "default", "--dataset", "CIFAR10", "--batch", "64", "--ckpt", "DDPM-CIFAR10-32", "-o"]
    for name in DEIS_NAMES:
        cfg = cli.setup(["--mode", "train", "--sched", name, "--infer_steps", "10"] + base)
        assert cfg.sched == name and cfg.native_sched is False and cfg.infer_steps == 10
        saved = json.load(open(os.path.join(cfg.output_dir, "args.json")))
        assert saved["sched"] == name and saved["infer_steps"] == 10
        for mode in ("sampling", "measure"):
            c = cli.setup(["--mode", mode, "--ckpt", cfg.output_dir, "--infer_steps", "15"], write=False)
            assert c.sched == name and c.infer_steps == 15
            assert cli.setup(["--mode", mode, "--ckpt", cfg.output_dir], write=False).infer_steps == 10
            assert cli.setup(["--mode", mode, "--ckpt", cfg.output_dir, "--native_sched"], write=False).sched == name
    with pytest.raises(SystemExit):
        cli.parse_args(["--sched", "DEIS_O4-SCHED"])


def test_native_sched_help_says_where_deis_lives(capsys):
    import baddiffusion as cli
    with pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    text = "".join(capsys.readouterr().out.split())             # argparse wraps the text, at hyphens too
    assert "DEIS_O1-SCHED/DEIS_O2-SCHED/DEIS_O3-SCHED" in text and "DEISPipeline" in text
    assert "withoutanativescheduler" not in text


def test_elijah_defense_accepts_the_names(tmp_path):
    import elijah_defense as E
    from baddiffusion_amd.pipelines import DDIMPipeline, DEISPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    assert set(DEIS_NAMES) < set(E.SCHED_CHOICES) and "DEIS-SCHED" not in E.SCHED_CHOICES
    ckpt_sched = DDPMScheduler(num_train_timesteps=400)
    for name, order in DEIS_NAMES.items():
        cfg = E.get_config(["--ckpt", "x", "--sched", name, "--infer_steps", "12", "--output_dir", str(tmp_path)])
        assert cfg.sched == name and cfg.infer_steps == 12
        p = E.make_pipeline(cfg, _NoUNet(), ckpt_sched)
        assert type(p) is DEISPipeline
        assert (p.scheduler.config.solver_order, p.scheduler.config.solver_type, p.scheduler.config.coefficient_dtype) == (order, "logrho", "float32")
        assert torch.equal(p.scheduler.betas, ckpt_sched.betas)
    with pytest.raises(SystemExit):
        E.get_config(["--ckpt", "x", "--sched", "DEIS_O4-SCHED", "--output_dir", str(tmp_path)])
    cfg = E.get_config(["--ckpt", "x", "--output_dir", str(tmp_path)])
    assert type(E.make_pipeline(cfg, _NoUNet(), ckpt_sched)) is DDIMPipeline


# ---------------------------------------------------------------------------------------------------- the C ABI
def _desc(L, **kw):
    d = L.DeisStepDesc(n=16, model_output=4096, sample=8192, m1=12288, m2=16384, m0_out=20480, prev_out=24576, alpha_s=0.8, sigma_s=0.6,
                       cx=1.0, c0=1.0, alpha_t=0.9, k0=1.0, k1=1.0, k2=1.0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_deis_step_rejects_bad_arguments_without_gpu():
    """the argument checks run on the host before any launch: negative status and a bd_last_error that names the entry point"""
    from baddiffusion_amd import _lib as L
    lib, INVALID = L.load(), -1
    assert lib.bd_deis_step(None, None) == INVALID and b"bd_deis_step: null descriptor" in lib.bd_last_error()
    cases = [(dict(n=0), b"n=0"), (dict(n=-4), b"n=-4"), (dict(model_output=None), b"null pointer"), (dict(sample=None), b"null pointer"),
             (dict(prev_out=None), b"null pointer"), (dict(alpha_s=0.0), b"alpha_s=0 must be positive"),
             (dict(alpha_s=-0.5), b"alpha_s=-0.5 must be positive"), (dict(sigma_s=0.0), b"sigma_s=0 must be positive"),
             (dict(sigma_s=float("nan")), b"sigma_s=nan must be positive"), (dict(m1=None), b"m2 without m1"),
             (dict(model_output=4100), b"model_output is not 16-byte aligned"), (dict(sample=8200), b"sample is not 16-byte aligned"),
             (dict(m1=12292), b"m1 is not 16-byte aligned"), (dict(m2=16392), b"m2 is not 16-byte aligned"),
             (dict(m0_out=20484), b"m0_out is not 16-byte aligned"), (dict(prev_out=24584), b"prev_out is not 16-byte aligned"),
             # partial overlaps: 16 floats = 64 bytes
             (dict(prev_out=8192 + 16), b"prev_out overlaps sample"), (dict(prev_out=8192 - 48), b"prev_out overlaps sample"),
             (dict(prev_out=4096 + 32), b"prev_out overlaps model_output"), (dict(prev_out=12288 + 16), b"prev_out overlaps m1"),
             (dict(m0_out=16384 + 16), b"m0_out overlaps m2"), (dict(m0_out=12288 - 16), b"m0_out overlaps m1"),
             (dict(m0_out=8192 + 48), b"m0_out overlaps sample"),
             # the two outputs: never, not even by identical base
             (dict(m0_out=24576), b"m0_out overlaps prev_out"), (dict(m0_out=24576 + 48), b"m0_out overlaps prev_out"),
             (dict(m0_out=8192, prev_out=8192), b"m0_out overlaps prev_out")]
    for kw, what in cases:
        assert lib.bd_deis_step(ctypes.byref(_desc(L, **kw)), None) == INVALID, kw
        msg = lib.bd_last_error()
        assert b"bd_deis_step" in msg and what in msg, (kw, msg)


def test_descriptor_layout_matches_the_header():
    from baddiffusion_amd import _lib as L
    fields = ("m2", "m0_out", "prev_out", "alpha_s", "sigma_s", "x0_clip", "x0_range", "cx", "c0", "alpha_t", "k0", "k2", "clip", "clip_range")
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "bd_hip.h"\nint main(){printf("%zu", sizeof(bd_deis_step_desc));' + \
           "".join(f'printf(" %zu", offsetof(bd_deis_step_desc, {f}));' for f in fields) + 'printf("\\n");return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    D = L.DeisStepDesc
    assert got == [ctypes.sizeof(D)] + [getattr(D, f).offset for f in fields]
