"""CPU: the host side of UniPC sampling -- the timestep tables and every stand-in chain of the reference (tests/golden/unipc.npz,
written by make_golden_unipc.py from the imported diffusers UniPCMultistepScheduler) against UniPCMultistepScheduler._plan driven
through a torch restatement of bd_unipc_step's formula, the sequence of predictor orders and corrector uses, configuration and
persistence, what is rejected before any launch, the wiring of the UNIPC_O*-SCHED names (model.py, baddiffusion.py,
elijah_defense.py) and the C ABI's argument checks.  Nothing here needs a GPU."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests.golden import cases as C
from tests.golden import cases_unipc as CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIPC_NAMES = {"UNIPC_O1-SCHED": 1, "UNIPC_O2-SCHED": 2, "UNIPC_O3-SCHED": 3}


class _NoUNet:
    """what a pipeline needs of a UNet before its first evaluation"""
    device = torch.device("cpu")


def _sched(**kw):
    from baddiffusion_amd.schedulers import UniPCMultistepScheduler
    return UniPCMultistepScheduler(**kw)


def kernel_formula(plan, predict_x0, x0_clip, e, x, last, hist, clip=None):
    """bd_unipc_step's formula (include/bd_hip.h) in fp32 torch arithmetic, in its stated order: (m0, xc, prev).  hist = the stored
    converted outputs, newest first; a tensor is handed to the kernel when either update reads it, as the scheduler does"""
    order, corr_order, alpha_s, sigma_s, k, p = plan
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    n_hist = max(corr_order, order - 1)
    m0 = (x - f(sigma_s) * e) / f(alpha_s) if predict_x0 else e
    if x0_clip:
        m0 = m0.clamp(-1.0, 1.0)
    xc = x
    if corr_order:
        xc = f(k[0]) * last + f(k[1]) * m0 + f(k[2]) * hist[0]
        for j in (1, 2):
            if j < n_hist:
                xc = xc + f(k[2 + j]) * hist[j]
    prev = f(p[0]) * xc + f(p[1]) * m0
    for j in (0, 1):
        if j < n_hist:
            prev = prev + f(p[2 + j]) * hist[j]
    if clip is not None:
        prev = prev.clamp(-clip, clip)
    return m0, xc, prev


def expected_sequence(order, n, disable=(), start_from=0):
    """(predictor order, corrector order) of every executed step, from scheduling_unipc_multistep.py:555-584: warm-up, the
    lower-order ending at every length, no corrector at the first executed step nor after a step listed in disable_corrector"""
    want, lower, this_order = [], 0, 0
    for i in range(start_from, n):
        corr = this_order if (i > 0 and i - 1 not in disable and i > start_from) else 0
        this_order = min(order, n - i, lower + 1)
        want.append((this_order, corr))
        lower = min(lower + 1, order)
    return want


# ---------------------------------------------------------------------------------------------------- timesteps
@pytest.mark.parametrize("n", CU.TIMESTEP_NS)
def test_timesteps_equal_the_reference(n, golden):
    s = _sched()
    s.set_timesteps(n)
    want = golden("unipc")[f"ts_{n}"]
    assert s.timesteps.dtype == torch.int64 and np.array_equal(s.timesteps.numpy(), want)
    assert s.num_inference_steps == len(want)


def test_timestep_fixture_is_the_documented_one(golden):
    g = golden("unipc")
    assert g["ts_4"].tolist() == [999, 749, 500, 250] and g["ts_1"].tolist() == [999]
    assert len(g["ts_1000"]) == 999 and len(set(g["ts_1000"].tolist())) == 999           # the duplicate is removed
    s = _sched(solver_order=3)
    s.set_timesteps(10)
    s.lower_order_nums, s.this_order, s.last_sample, s._ring_ts = 2, 2, torch.zeros(1), [None, 999, 899]
    s.set_timesteps(1000)
    assert s.num_inference_steps == 999 and s.lower_order_nums == 0 and s.this_order == 0        # history and warm-up reset
    assert s.last_sample is None and s._ring_ts == [None] * 3 and s._ring == [None] * 3


# ---------------------------------------------------------------------------------------------------- chains
def test_chain_fixture_covers_the_documented_cases(golden):
    g = golden("unipc")
    assert len(CU.CHAIN_CASES) == 42 and all(f"chain_{CU.chain_tag(*c)}" in g.files for c in CU.CHAIN_CASES)
    assert len({CU.chain_tag(*c) for c in CU.CHAIN_CASES}) == 42
    assert max(float(g[f"chain_dev64_{CU.chain_tag(*c)}"]) for c in CU.CHAIN_CASES) < 1.2e-5
    # orders 2 and 3 give the same chain at 4 steps: the third order is never reached
    for px0 in CU.PREDICT_X0:
        for st in CU.SOLVER_TYPES:
            assert np.array_equal(g[f"chain_{CU.chain_tag(px0, st, 2, 4, False)}"], g[f"chain_{CU.chain_tag(px0, st, 3, 4, False)}"])


@pytest.mark.parametrize("case", CU.CHAIN_CASES, ids=lambda c: CU.chain_tag(*c))
def test_plan_reproduces_the_reference_chain(case, golden):
    """_plan's flattened coefficients through the kernel's formula: every intermediate sample within max(4e-6, 4 * dev64) * max|ref| of
    the reference's, dev64 being the reference's own distance from the recurrence in fp64 (the bound of the DPM-Solver and RePaint
    stand-in chains); and the sequence of predictor orders and corrector uses"""
    px0, solver_type, order, n, thr, dis = case
    g, tag = golden("unipc"), CU.chain_tag(*case)
    ref, dev64 = g[f"chain_{tag}"], float(g[f"chain_dev64_{tag}"])
    bound = max(4e-6, 4 * dev64)
    s = _sched(**CU.scheduler_kwargs(px0, solver_type, order, thr, dis))
    s.set_timesteps(n)
    assert len(ref) == n
    x, hist, last, seq, worst = C.pndm_init(), [], None, [], 0.0
    for i, t in enumerate(s.timesteps.tolist()):
        plan = s._plan(i, has_last=last is not None)
        seq.append(plan[:2])
        m0, last, x = kernel_formula(plan, px0, px0 and thr, C.pndm_fake_model(x, t), x, last, hist)
        hist = ([m0] + hist)[:order]
        s._advance(i, plan[0])
        dev = float(np.abs(x.numpy() - ref[i]).max() / np.abs(ref[i]).max())
        worst = max(worst, dev)
        assert dev <= bound, (i, t, dev, bound)
    assert seq == expected_sequence(order, n, dis)
    assert s.lower_order_nums == order
    print(f"MEASURE unipc stand-in chain {tag} (host formula): worst step deviation {worst:.3e}, bound {bound:.3e}")


def test_order_and_corrector_sequences():
    # spelled out once, so that expected_sequence itself is pinned
    assert expected_sequence(3, 6) == [(1, 0), (2, 1), (3, 2), (3, 3), (2, 3), (1, 2)]
    assert expected_sequence(2, 4, disable=(0, 2)) == [(1, 0), (2, 0), (2, 2), (1, 0)]
    assert expected_sequence(3, 10, start_from=7) == [(1, 0), (2, 1), (1, 2)]
    for order in (1, 2, 3):
        for n in (1, 2, 3, 4, 10, 20):
            for dis in ((), (0,), (1, 2)):
                s = _sched(solver_order=order, disable_corrector=list(dis))
                s.set_timesteps(n)
                got, last = [], False
                for i in range(n):
                    plan = s._plan(i, has_last=last)
                    got.append(plan[:2])
                    s._advance(i, plan[0])
                    last = True
                assert got == expected_sequence(order, n, dis), (order, n, dis)
    # lower_order_final=False: the order stays at solver_order to the end
    s = _sched(solver_order=3, lower_order_final=False)
    s.set_timesteps(5)
    got = []
    for i in range(5):
        plan = s._plan(i, has_last=i > 0)
        got.append(plan[:2])
        s._advance(i, plan[0])
    assert got == [(1, 0), (2, 1), (3, 2), (3, 3), (3, 3)]
    # start_from=k (the pipeline steps a fresh state from timestep k on): no last sample, so no corrector and first order
    s = _sched(solver_order=3)
    s.set_timesteps(10)
    got, last = [], False
    for i in range(7, 10):
        plan = s._plan(i, has_last=last)
        got.append(plan[:2])
        s._advance(i, plan[0])
        last = True
    assert got == expected_sequence(3, 10, start_from=7)


@pytest.mark.parametrize("predict_x0", (True, False))
@pytest.mark.parametrize("solver_type", ("bh1", "bh2"))
def test_plan_first_order_is_the_reference_closed_form(predict_x0, solver_type):
    """solver_order=1: predictor x_t = cx x - A h_phi_1 m0, corrector with rho = 0.5:
    x_t = cx l - A h_phi_1 h1 - A B_h 0.5 (m0 - h1)  (scheduling_unipc_multistep.py:395-408, :494-515)"""
    s = _sched(solver_order=1, predict_x0=predict_x0, solver_type=solver_type)
    s.set_timesteps(10)
    ts = s.timesteps.tolist()

    def scalars(s0, t):
        h = s.lambda_t[t] - s.lambda_t[s0]
        hh = -h if predict_x0 else h
        h_phi_1 = torch.expm1(hh)
        B_h = hh if solver_type == "bh1" else torch.expm1(hh)
        if predict_x0:
            return s.sigma_t[t] / s.sigma_t[s0], s.alpha_t[t], h_phi_1, B_h
        return s.alpha_t[t] / s.alpha_t[s0], s.sigma_t[t], h_phi_1, B_h
    order, corr, alpha_s, sigma_s, k, p = s._plan(0, has_last=False)
    cx, A, h_phi_1, _ = scalars(ts[0], ts[1])
    assert (order, corr) == (1, 0) and k == (0.0,) * 5
    assert alpha_s == float(s.alpha_t[ts[0]]) and sigma_s == float(s.sigma_t[ts[0]])
    assert p == (float(cx), float(-(A * h_phi_1)), 0.0, 0.0)
    s._advance(0, 1)
    order, corr, alpha_s, sigma_s, k, p = s._plan(1, has_last=True)
    cx, A, h_phi_1, B_h = scalars(ts[0], ts[1])                      # the corrector repeats the transition of the last predictor
    k0 = -(A * B_h) * torch.tensor(0.5)
    assert (order, corr) == (1, 1)
    assert k == (float(cx), float(k0), float(-(A * h_phi_1) - k0), 0.0, 0.0)
    cx, A, h_phi_1, _ = scalars(ts[1], ts[2])
    assert p == (float(cx), float(-(A * h_phi_1)), 0.0, 0.0)
    assert s.alpha_t.dtype == s.sigma_t.dtype == s.lambda_t.dtype == torch.float32
    assert torch.equal(s.lambda_t, torch.log(s.alpha_t) - torch.log(s.sigma_t))
    # the last step goes to timestep 0, not past it
    for i in range(1, 9):
        s._advance(i, 1)
    cx, A, h_phi_1, _ = scalars(ts[9], 0)
    assert s._plan(9, has_last=True)[5][:2] == (float(cx), float(-(A * h_phi_1)))


def test_plan_is_kept_per_schedule_and_state():
    s = _sched(solver_order=3)
    s.set_timesteps(20)
    ts = s.timesteps.tolist()
    s.lower_order_nums, s.this_order, s._ring_ts = 3, 3, [ts[4], ts[5], ts[6]]
    kept = s._plan(7, has_last=True)
    assert kept == s._plan_scalars(7, True) and kept[:2] == (3, 3) and s._plan(7, has_last=True) is kept
    assert s._plan(7, has_last=False)[:2] == (3, 0) and s._plan(7, has_last=False)[4] == (0.0,) * 5
    s.set_timesteps(20)                                 # the same schedule again: kept; the state is part of the key
    assert s._plan(7, has_last=False)[:2] == (1, 0)
    s.lower_order_nums, s.this_order, s._ring_ts = 3, 3, [ts[4], ts[5], ts[6]]
    assert s._plan(7, has_last=True) is kept
    s.set_timesteps(10)                                 # another schedule: recomputed
    assert s._plans == {}
    s.set_timesteps(20)
    s.lower_order_nums, s.this_order, s._ring_ts = 3, 3, [ts[4], ts[5], ts[6]]
    s.config.solver_type = "bh1"                        # an assigned option is seen too
    assert s._plan(7, has_last=True) != kept and s._plan(7, has_last=True) == s._plan_scalars(7, True)


# ---------------------------------------------------------------------------------------------------- configuration
def test_config_conversion():
    from baddiffusion_amd.pipelines import DPMSolverPipeline, UniPCPipeline, _MultistepPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler, SchedulerConfigCarrier, UniPCMultistepScheduler
    ref_cfg = {"num_train_timesteps": 500, "beta_start": 0.0002, "beta_end": 0.03, "beta_schedule": "scaled_linear", "trained_betas": None,
               "solver_order": 3, "prediction_type": "epsilon", "thresholding": False, "dynamic_thresholding_ratio": 0.995,
               "sample_max_value": 1.0, "predict_x0": False, "solver_type": "bh1", "lower_order_final": False, "disable_corrector": [1],
               "solver_p": None, "_class_name": "UniPCMultistepScheduler"}
    s = UniPCMultistepScheduler.from_config(ref_cfg)
    assert {k: s.config[k] for k in UniPCMultistepScheduler._KEYS} == {k: ref_cfg[k] for k in UniPCMultistepScheduler._KEYS}
    assert set(s.config) == set(UniPCMultistepScheduler._KEYS) and len(s) == 500 and s.order == 1
    assert s.predict_x0 is False and s.disable_corrector == [1]
    d = _sched()                                        # the reference's defaults
    assert (d.config.solver_order, d.config.solver_type, d.config.predict_x0, d.config.lower_order_final, d.config.disable_corrector) == \
        (2, "bh2", True, True, [])
    # a DPM-Solver / DEIS style config converts: midpoint / heun / logrho become bh1
    for st in ("midpoint", "heun", "logrho"):
        assert UniPCMultistepScheduler.from_config({"solver_type": st, "algorithm_type": "dpmsolver++"}).config.solver_type == "bh1"
    for st in ("bh1", "bh2"):
        assert _sched(solver_type=st).config.solver_type == st
    with pytest.raises(NotImplementedError, match="euler does is not implemented for"):
        _sched(solver_type="euler")
    with pytest.raises(NotImplementedError, match="solver_order 4"):
        _sched(solver_order=4)
    with pytest.raises(NotImplementedError, match="solver_p"):
        _sched(solver_p=DDPMScheduler())
    with pytest.raises(NotImplementedError, match="solver_p"):
        UniPCMultistepScheduler.from_config({**ref_cfg, "solver_p": DDPMScheduler()})
    with pytest.raises(NotImplementedError, match="sample_max_value"):
        _sched(thresholding=True, sample_max_value=2.0)
    assert _sched(thresholding=True, sample_max_value=1.0).config.thresholding is True
    with pytest.raises(NotImplementedError):
        _sched(beta_schedule="squaredcos_cap_v2")
    # the pipeline converts any other scheduler from its config and keeps a UniPC scheduler as it is
    ddpm = DDPMScheduler(num_train_timesteps=400, clip_sample=False)
    p = UniPCPipeline(_NoUNet(), ddpm)
    assert type(p.scheduler) is UniPCMultistepScheduler and torch.equal(p.scheduler.betas, ddpm.betas)
    assert p.clip_sample is False and p.clip_sample_range == 1.0
    assert type(UniPCPipeline(_NoUNet(), SchedulerConfigCarrier("UniPCMultistepScheduler")).scheduler) is UniPCMultistepScheduler
    assert UniPCPipeline(_NoUNet(), s, clip_sample=True).scheduler is s
    import inspect
    from baddiffusion_amd.pipelines import PNDMPipeline
    sig, pndm = inspect.signature(UniPCPipeline.__call__), inspect.signature(PNDMPipeline.__call__)
    assert list(sig.parameters) == list(pndm.parameters) and sig.parameters["num_inference_steps"].default is None
    assert UniPCPipeline.default_steps == 10 and "__call__" not in vars(UniPCPipeline)      # the call is _MultistepPipeline's
    # one loop, two thin subclasses
    assert issubclass(UniPCPipeline, _MultistepPipeline) and issubclass(DPMSolverPipeline, _MultistepPipeline)
    assert "_sample" not in vars(UniPCPipeline) and "_sample" not in vars(DPMSolverPipeline)


def test_errors_are_loud():
    x = torch.zeros(2, 3, 8, 8)
    s = _sched()
    with pytest.raises(ValueError, match="Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler"):
        s.step(x, 999, x)
    with pytest.raises(ValueError, match="Number of inference steps is 'None'"):
        s._plan(0)
    s.set_timesteps(10)
    with pytest.raises(RuntimeError, match=r"UniPCMultistepScheduler\.step runs on the GPU only"):
        s.step(x, 999, x)
    for kind in ("sample", "v_prediction"):
        v = _sched(prediction_type=kind)
        v.set_timesteps(10)
        with pytest.raises(ValueError, match="prediction_type"):
            v.step(x, 999, x)
    from baddiffusion_amd import ops
    with pytest.raises(RuntimeError):
        ops.unipc_step(x, x, 1.0, 1.0)


def test_load_and_save_scheduler_round_trip(tmp_path):
    from baddiffusion_amd.model import load_scheduler, save_scheduler
    from baddiffusion_amd.schedulers import UniPCMultistepScheduler
    s = _sched(num_train_timesteps=400, beta_schedule="scaled_linear", solver_order=3, predict_x0=False, solver_type="bh1",
               lower_order_final=False, disable_corrector=[0, 3])
    save_scheduler(s, str(tmp_path / "scheduler"))
    saved = json.load(open(tmp_path / "scheduler" / "scheduler_config.json"))
    assert saved["_class_name"] == "UniPCMultistepScheduler" and saved["solver_order"] == 3 and saved["disable_corrector"] == [0, 3]
    back = load_scheduler(str(tmp_path / "scheduler"))
    assert type(back) is UniPCMultistepScheduler and dict(back.config) == dict(s.config)
    assert torch.equal(back.betas, s.betas) and torch.equal(back.lambda_t, s.lambda_t)


# ---------------------------------------------------------------------------------------------------- wiring
def test_sched_name_wiring():
    from baddiffusion_amd.model import DiffuserModelSched
    from baddiffusion_amd.pipelines import PNDMPipeline, UniPCPipeline
    from baddiffusion_amd.schedulers import PNDMScheduler, SchedulerConfigCarrier, UniPCMultistepScheduler
    from baddiffusion_amd.sched_names import SCHEDS
    assert {n: r.sched_kw["solver_order"] for n, r in SCHEDS.items() if r.scheduler is UniPCMultistepScheduler} == UNIPC_NAMES
    assert all(SCHEDS[n].carrier is None and not SCHEDS[n].native_only for n in UNIPC_NAMES)     # no PNDM conversion, not native-only
    get = lambda name, **kw: DiffuserModelSched.get_pretrained("DDPM-CIFAR10-32", noise_sched_type=name, allow_random_init=True, **kw)
    for name, order in UNIPC_NAMES.items():
        for native in (False, True):
            m, s, gp = get(name, clip_sample=True, native_sched=native)
            assert type(s) is UniPCMultistepScheduler
            assert (s.config.solver_order, s.config.solver_type, s.config.predict_x0) == (order, "bh2", True)
            assert s.config.num_train_timesteps == 1000 and torch.equal(s.betas, torch.linspace(0.0001, 0.02, 1000))
            p = gp(m, s)
            assert type(p) is UniPCPipeline and p.scheduler is s and p.clip_sample is True
            del m, p
    m, s, gp = get("UNIPC_O2-SCHED", clip_sample=False)
    assert gp(m, s).clip_sample is False
    m, s, gp = DiffuserModelSched.get_model_sched(image_size=32, channels=3, model_type=DiffuserModelSched.DDPM_CIFAR10_DEFAULT,
                                                  noise_sched_type="UNIPC_O3-SCHED")
    assert type(s) is UniPCMultistepScheduler and type(gp(m, s)) is UniPCPipeline
    del m
    # the reference's own name is unchanged: the config carrier + PNDM without the opt-in, refused with it
    m, s, gp = get("UNIPC-SCHED", clip_sample=True)
    assert type(s) is SchedulerConfigCarrier and s.class_name == "UniPCMultistepScheduler"
    p = gp(m, s)
    assert type(p) is PNDMPipeline and type(p.scheduler) is PNDMScheduler
    with pytest.raises(NotImplementedError, match="UNIPC-SCHED"):
        get("UNIPC-SCHED", native_sched=True)


def test_cli_accepts_the_names_and_args_json_round_trips(tmp_path, monkeypatch):
    import baddiffusion as cli
    monkeypatch.chdir(tmp_path)
    assert set(UNIPC_NAMES) < set(cli.SCHED_CHOICES) and "UNIPC-SCHED" in cli.SCHED_CHOICES
    base = ["--project", "default", "--dataset", "CIFAR10", "--batch", "64", "--ckpt", "DDPM-CIFAR10-32", "-o"]
    for name in UNIPC_NAMES:
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
        cli.parse_args(["--sched", "UNIPC_O4-SCHED"])


def test_native_sched_help_says_where_unipc_lives(capsys):
    import baddiffusion as cli
    with pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    text = "".join(capsys.readouterr().out.split())             # argparse wraps the text, at hyphens too
    assert "UNIPC_O1-SCHED/UNIPC_O2-SCHED/UNIPC_O3-SCHED" in text and "UniPCPipeline" in text


def test_elijah_defense_accepts_the_names(tmp_path):
    import elijah_defense as E
    from baddiffusion_amd.pipelines import DDIMPipeline, UniPCPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    assert set(UNIPC_NAMES) < set(E.SCHED_CHOICES) and "UNIPC-SCHED" not in E.SCHED_CHOICES
    ckpt_sched = DDPMScheduler(num_train_timesteps=400)
    for name, order in UNIPC_NAMES.items():
        cfg = E.get_config(["--ckpt", "x", "--sched", name, "--infer_steps", "12", "--output_dir", str(tmp_path)])
        assert cfg.sched == name and cfg.infer_steps == 12
        p = E.make_pipeline(cfg, _NoUNet(), ckpt_sched)
        assert type(p) is UniPCPipeline
        assert (p.scheduler.config.solver_order, p.scheduler.config.solver_type, p.scheduler.config.predict_x0) == (order, "bh2", True)
        assert torch.equal(p.scheduler.betas, ckpt_sched.betas)
    cfg = E.get_config(["--ckpt", "x", "--output_dir", str(tmp_path)])
    assert type(E.make_pipeline(cfg, _NoUNet(), ckpt_sched)) is DDIMPipeline


# ---------------------------------------------------------------------------------------------------- the C ABI
def _desc(L, **kw):
    d = L.UnipcStepDesc(n=16, model_output=4096, sample=8192, last_sample=12288, h1=16384, h2=20480, h3=24576, m0_out=28672,
                        corrected_out=32768, prev_out=36864, convert=1, alpha_s=0.8, sigma_s=0.6, kl=1.0, k0=1.0, k1=1.0, k2=1.0, k3=1.0,
                        px=1.0, p0=1.0, p1=1.0, p2=1.0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_unipc_step_rejects_bad_arguments_without_gpu():
    """the argument checks run on the host before any launch: negative status and a bd_last_error that names the entry point"""
    from baddiffusion_amd import _lib as L
    lib, INVALID = L.load(), -1
    assert lib.bd_unipc_step(None, None) == INVALID and b"bd_unipc_step: null descriptor" in lib.bd_last_error()
    cases = [(dict(n=0), b"n=0"), (dict(n=-4), b"n=-4"), (dict(model_output=None), b"null pointer"), (dict(sample=None), b"null pointer"),
             (dict(prev_out=None), b"null pointer"), (dict(h1=None), b"last_sample without h1"),
             (dict(model_output=4100), b"model_output is not 16-byte aligned"), (dict(sample=8200), b"sample is not 16-byte aligned"),
             (dict(last_sample=12292), b"last_sample is not 16-byte aligned"), (dict(h1=16388), b"h1 is not 16-byte aligned"),
             (dict(h2=20488), b"h2 is not 16-byte aligned"), (dict(h3=24580), b"h3 is not 16-byte aligned"),
             (dict(m0_out=28676), b"m0_out is not 16-byte aligned"), (dict(corrected_out=32776), b"corrected_out is not 16-byte aligned"),
             (dict(prev_out=36868), b"prev_out is not 16-byte aligned"),
             # partial overlaps: 16 floats = 64 bytes
             (dict(prev_out=8192 + 16), b"prev_out overlaps sample"), (dict(prev_out=8192 - 48), b"prev_out overlaps sample"),
             (dict(prev_out=4096 + 32), b"prev_out overlaps model_output"), (dict(prev_out=12288 + 16), b"prev_out overlaps last_sample"),
             (dict(m0_out=24576 + 16), b"m0_out overlaps h3"), (dict(m0_out=20480 - 16), b"m0_out overlaps h2"),
             (dict(m0_out=16384 + 48), b"m0_out overlaps h1"), (dict(corrected_out=12288 + 16), b"corrected_out overlaps last_sample"),
             (dict(corrected_out=8192 - 16), b"corrected_out overlaps sample"), (dict(corrected_out=24576 + 32), b"corrected_out overlaps h3"),
             # outputs among themselves: never, not even by identical base
             (dict(m0_out=36864), b"m0_out overlaps prev_out"), (dict(m0_out=36864 + 48), b"m0_out overlaps prev_out"),
             (dict(corrected_out=36864), b"corrected_out overlaps prev_out"), (dict(corrected_out=28672 + 16), b"corrected_out overlaps m0_out"),
             (dict(m0_out=8192, prev_out=8192), b"m0_out overlaps prev_out"),
             (dict(corrected_out=12288, m0_out=12288), b"corrected_out overlaps m0_out")]
    for kw, what in cases:
        assert lib.bd_unipc_step(ctypes.byref(_desc(L, **kw)), None) == INVALID, kw
        msg = lib.bd_last_error()
        assert b"bd_unipc_step" in msg and what in msg, (kw, msg)


def test_descriptor_layout_matches_the_header():
    from baddiffusion_amd import _lib as L
    fields = ("last_sample", "h3", "m0_out", "corrected_out", "prev_out", "convert", "x0_range", "kl", "k3", "px", "p2", "clip", "clip_range")
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "bd_hip.h"\nint main(){printf("%zu", sizeof(bd_unipc_step_desc));' + \
           "".join(f'printf(" %zu", offsetof(bd_unipc_step_desc, {f}));' for f in fields) + 'printf("\\n");return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    D = L.UnipcStepDesc
    assert got == [ctypes.sizeof(D)] + [getattr(D, f).offset for f in fields]
