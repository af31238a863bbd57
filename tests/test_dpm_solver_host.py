"""CPU: the host side of DPM-Solver(++) sampling -- the timestep tables and every stand-in chain of the reference
(tests/golden/dpm_solver.npz, written by make_golden_dpm.py from the imported diffusers DPMSolverMultistepScheduler) against
DPMSolverMultistepScheduler._plan driven through a torch restatement of bd_dpm_step's formula, configuration and persistence, what is
rejected before any launch, the opt-in wiring (native_sched, --native_sched / --infer_steps, elijah_defense.py --sched) and the C ABI's
argument checks.  Nothing here needs a GPU."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests.golden import cases as C
from tests.golden import cases_dpm as CD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DPM_NAMES = {"DPM_SOLVER_PP_O1-SCHED": (1, "dpmsolver++"), "DPM_SOLVER_O1-SCHED": (1, "dpmsolver"),
             "DPM_SOLVER_PP_O2-SCHED": (2, "dpmsolver++"), "DPM_SOLVER_O2-SCHED": (2, "dpmsolver"),
             "DPM_SOLVER_PP_O3-SCHED": (3, "dpmsolver++"), "DPM_SOLVER_O3-SCHED": (3, "dpmsolver")}


class _NoUNet:
    """what a pipeline needs of a UNet before its first evaluation"""
    device = torch.device("cpu")


def _sched(**kw):
    from baddiffusion_amd.schedulers import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(**kw)


def kernel_formula(plan, pp, x0_clip, e, x, m1, m2, clip=None):
    """bd_dpm_step's formula (include/bd_hip.h) in fp32 torch arithmetic, in its stated order: (m0, prev)"""
    order, alpha_s, sigma_s, cx, c0, c1, c2 = plan
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    m0 = (x - f(sigma_s) * e) / f(alpha_s) if pp else e
    if x0_clip:
        m0 = m0.clamp(-1.0, 1.0)
    prev = f(cx) * x + f(c0) * m0
    if order >= 2:
        prev = prev + f(c1) * m1
    if order >= 3:
        prev = prev + f(c2) * m2
    if clip is not None:
        prev = prev.clamp(-clip, clip)
    return m0, prev


# ---------------------------------------------------------------------------------------------------- timesteps
@pytest.mark.parametrize("n", CD.TIMESTEP_NS)
def test_timesteps_equal_the_reference(n, golden):
    s = _sched()
    s.set_timesteps(n)
    want = golden("dpm_solver")[f"ts_{n}"]
    assert s.timesteps.dtype == torch.int64 and np.array_equal(s.timesteps.numpy(), want)
    assert s.num_inference_steps == len(want)


def test_timestep_fixture_is_the_documented_one(golden):
    g = golden("dpm_solver")
    assert g["ts_4"].tolist() == [999, 749, 500, 250] and g["ts_1"].tolist() == [999]
    assert len(g["ts_1000"]) == 999 and len(set(g["ts_1000"].tolist())) == 999           # the duplicate is removed
    s = _sched()
    s.lower_order_nums = 2
    s.set_timesteps(1000)
    assert s.num_inference_steps == 999 and s.lower_order_nums == 0                      # history and warm-up reset


# ---------------------------------------------------------------------------------------------------- chains
def test_chain_fixture_covers_the_documented_cases(golden):
    g = golden("dpm_solver")
    assert len(CD.CHAIN_CASES) == 39 and all(f"chain_{CD.chain_tag(*c)}" in g.files for c in CD.CHAIN_CASES)
    assert max(float(g[f"chain_dev64_{CD.chain_tag(*c)}"]) for c in CD.CHAIN_CASES) < 3e-6


@pytest.mark.parametrize("case", CD.CHAIN_CASES, ids=lambda c: CD.chain_tag(*c))
def test_plan_reproduces_the_reference_chain(case, golden):
    """_plan's flattened coefficients through the kernel's formula: every intermediate sample within max(4e-6, 4 * dev64) * max|ref| of
    the reference's, dev64 being the reference's own distance from the recurrence in fp64 (the bound of the RePaint stand-in chain)"""
    algorithm, solver_type, order, n, thr = case
    g, tag = golden("dpm_solver"), CD.chain_tag(*case)
    ref, dev64 = g[f"chain_{tag}"], float(g[f"chain_dev64_{tag}"])
    bound = max(4e-6, 4 * dev64)
    s = _sched(**CD.scheduler_kwargs(algorithm, solver_type, order, thr))
    s.set_timesteps(n)
    assert len(ref) == n
    x, hist, orders, worst = C.pndm_init(), [], [], 0.0
    for i, t in enumerate(s.timesteps.tolist()):
        plan = s._plan(i)
        orders.append(plan[0])
        m0, x = kernel_formula(plan, algorithm == "dpmsolver++", thr, C.pndm_fake_model(x, t), x, hist[-1] if hist else None,
                               hist[-2] if len(hist) > 1 else None)
        hist = (hist + [m0])[-3:]
        s._advance()
        dev = float(np.abs(x.numpy() - ref[i]).max() / np.abs(ref[i]).max())
        worst = max(worst, dev)
        assert dev <= bound, (i, t, dev, bound)
    # warm-up orders, and the lower-order ending below 15 steps only
    want = [min(order, i + 1) for i in range(n)]
    if n < 15:
        want[-1] = 1
        if order == 3:
            want[-2] = min(want[-2], 2)
    assert orders == want
    print(f"MEASURE dpm stand-in chain {tag} (host formula): worst step deviation {worst:.3e}, bound {bound:.3e}")


def test_plan_first_order_is_the_reference_scalars():
    s = _sched(algorithm_type="dpmsolver++")
    s.set_timesteps(10)
    order, alpha_s, sigma_s, cx, c0, c1, c2 = s._plan(0)
    t, p = int(s.timesteps[0]), int(s.timesteps[1])
    h = s.lambda_t[p] - s.lambda_t[t]
    assert order == 1 and (c1, c2) == (0.0, 0.0)
    assert alpha_s == float(s.alpha_t[t]) and sigma_s == float(s.sigma_t[t])
    assert cx == float(s.sigma_t[p] / s.sigma_t[t]) and c0 == float(-(s.alpha_t[p] * (torch.exp(-h) - 1.0)))
    assert s.alpha_t.dtype == s.sigma_t.dtype == s.lambda_t.dtype == torch.float32
    assert torch.equal(s.lambda_t, torch.log(s.alpha_t) - torch.log(s.sigma_t))
    # the last step goes to timestep 0, not past it
    s.lower_order_nums = 2
    e = _sched(algorithm_type="dpmsolver")
    e.set_timesteps(20)
    _, _, _, cx, _, _, _ = e._plan(19)
    assert cx == float(e.alpha_t[0] / e.alpha_t[int(e.timesteps[-1])])


def test_plan_is_kept_per_schedule_and_warm_up_state():
    s = _sched(solver_order=3, algorithm_type="dpmsolver")
    s.set_timesteps(20)
    for lower in (0, 1, 2):
        s.lower_order_nums = lower
        for i in (lower, 7, 19):
            assert s._plan(i) == s._plan_scalars(i) and s._plan(i)[0] == min(3, lower + 1)
    kept = s._plan(7)
    s.set_timesteps(20)                                 # the same schedule again: kept; the warm-up state is part of the key
    assert s.lower_order_nums == 0 and s._plan(7)[0] == 1 and s._plan(7) == s._plan_scalars(7)
    s.lower_order_nums = 2
    assert s._plan(7) is kept
    s.set_timesteps(10)                                 # another schedule: recomputed
    s.lower_order_nums = 2
    assert s._plan(7) != kept and s._plan(7) == s._plan_scalars(7)
    s.config.solver_type = "heun"                       # an assigned option is seen too
    s.lower_order_nums = 1
    assert s._plan(7) == s._plan_scalars(7)


# ---------------------------------------------------------------------------------------------------- configuration
def test_from_config_of_a_unipc_style_config():
    from baddiffusion_amd.pipelines import DPMSolverPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler, DPMSolverMultistepScheduler, SchedulerConfigCarrier
    unipc = {"num_train_timesteps": 500, "beta_start": 0.0002, "beta_end": 0.03, "beta_schedule": "scaled_linear", "trained_betas": None,
             "solver_order": 3, "prediction_type": "epsilon", "thresholding": False, "dynamic_thresholding_ratio": 0.995,
             "sample_max_value": 1.0, "predict_x0": True, "solver_type": "bh2", "lower_order_final": True, "disable_corrector": [],
             "solver_p": None}
    s = DPMSolverMultistepScheduler.from_config(unipc)
    assert s.config.solver_type == "midpoint" and s.config.algorithm_type == "dpmsolver++" and s.config.solver_order == 3
    assert len(s) == 500 and s.order == 1 and "predict_x0" not in s.config
    d = DPMSolverMultistepScheduler.from_config({"algorithm_type": "deis", "solver_type": "logrho"})
    assert d.config.algorithm_type == "dpmsolver++" and d.config.solver_type == "midpoint" and d.config.solver_order == 2
    with pytest.raises(NotImplementedError):
        _sched(algorithm_type="unipc")
    with pytest.raises(NotImplementedError):
        _sched(solver_type="euler")
    with pytest.raises(NotImplementedError):
        _sched(beta_schedule="squaredcos_cap_v2")
    # the pipeline converts any other scheduler from its config and keeps a DPM-Solver scheduler as it is
    ddpm = DDPMScheduler(num_train_timesteps=400, clip_sample=False)
    p = DPMSolverPipeline(_NoUNet(), ddpm)
    assert type(p.scheduler) is DPMSolverMultistepScheduler and torch.equal(p.scheduler.betas, ddpm.betas)
    assert p.clip_sample is False and p.clip_sample_range == 1.0
    assert type(DPMSolverPipeline(_NoUNet(), SchedulerConfigCarrier("DPMSolverMultistepScheduler")).scheduler) is DPMSolverMultistepScheduler
    assert DPMSolverPipeline(_NoUNet(), s, clip_sample=True).scheduler is s
    import inspect
    from baddiffusion_amd.pipelines import PNDMPipeline
    sig, pndm = inspect.signature(DPMSolverPipeline.__call__), inspect.signature(PNDMPipeline.__call__)
    assert list(sig.parameters) == list(pndm.parameters) and sig.parameters["num_inference_steps"].default is None
    assert DPMSolverPipeline.default_steps == 20 and PNDMPipeline.default_steps == 50 and "__call__" not in vars(DPMSolverPipeline)


def test_errors_are_loud():
    x = torch.zeros(2, 3, 8, 8)
    s = _sched()
    with pytest.raises(ValueError, match="Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler"):
        s.step(x, 999, x)
    with pytest.raises(ValueError, match="Number of inference steps is 'None'"):
        s._plan(0)
    s.set_timesteps(10)
    with pytest.raises(RuntimeError, match=r"DPMSolverMultistepScheduler\.step runs on the GPU only"):
        s.step(x, 999, x)
    for kind in ("sample", "v_prediction"):
        v = _sched(prediction_type=kind)
        v.set_timesteps(10)
        with pytest.raises(ValueError, match="prediction_type"):
            v.step(x, 999, x)
    with pytest.raises(NotImplementedError, match="use_karras_sigmas"):
        _sched(use_karras_sigmas=True)
    with pytest.raises(NotImplementedError, match="sample_max_value"):
        _sched(thresholding=True, sample_max_value=2.0)
    assert _sched(thresholding=True, sample_max_value=1.0).config.thresholding is True
    from baddiffusion_amd import ops
    with pytest.raises(RuntimeError):
        ops.dpm_step(x, x, 1.0, 1.0)


def test_load_and_save_scheduler_round_trip(tmp_path):
    from baddiffusion_amd.model import load_scheduler, save_scheduler
    from baddiffusion_amd.schedulers import DPMSolverMultistepScheduler
    s = _sched(num_train_timesteps=400, beta_schedule="scaled_linear", solver_order=3, algorithm_type="dpmsolver", solver_type="heun",
               lower_order_final=False)
    save_scheduler(s, str(tmp_path / "scheduler"))
    saved = json.load(open(tmp_path / "scheduler" / "scheduler_config.json"))
    assert saved["_class_name"] == "DPMSolverMultistepScheduler" and saved["solver_order"] == 3
    back = load_scheduler(str(tmp_path / "scheduler"))
    assert type(back) is DPMSolverMultistepScheduler and dict(back.config) == dict(s.config)
    assert torch.equal(back.betas, s.betas) and torch.equal(back.lambda_t, s.lambda_t)


# ---------------------------------------------------------------------------------------------------- opt-in wiring
def test_native_sched_wiring():
    from baddiffusion_amd.model import DiffuserModelSched
    from baddiffusion_amd.pipelines import DDIMPipeline, DPMSolverPipeline, PNDMPipeline
    from baddiffusion_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, PNDMScheduler, SchedulerConfigCarrier
    from baddiffusion_amd.sched_names import SCHEDS
    assert {n: (r.sched_kw["solver_order"], r.sched_kw["algorithm_type"]) for n, r in SCHEDS.items() if r.native_only} == DPM_NAMES
    assert all(SCHEDS[n].scheduler is DPMSolverMultistepScheduler for n in DPM_NAMES)
    get = lambda name, **kw: DiffuserModelSched.get_pretrained("DDPM-CIFAR10-32", noise_sched_type=name, allow_random_init=True, **kw)
    # without the opt-in: the reference's conversion to PNDM, as before
    m, s, gp = get("DPM_SOLVER_PP_O2-SCHED", clip_sample=True)
    assert type(s) is SchedulerConfigCarrier and s.class_name == "DPMSolverMultistepScheduler"
    p = gp(m, s)
    assert type(p) is PNDMPipeline and type(p.scheduler) is PNDMScheduler and p.clip_sample is True
    # with it: the solver the name spells out
    m, s, gp = get("DPM_SOLVER_O3-SCHED", clip_sample=True, native_sched=True)
    assert type(s) is DPMSolverMultistepScheduler and (s.config.solver_order, s.config.algorithm_type) == (3, "dpmsolver")
    assert s.config.num_train_timesteps == 1000 and torch.equal(s.betas, torch.linspace(0.0001, 0.02, 1000))
    p = gp(m, s)
    assert type(p) is DPMSolverPipeline and p.scheduler is s and p.clip_sample is True
    del m, p
    for name in ("UNIPC-SCHED", "DEIS-SCHED", "HEUN-SCHED", "LMSD-SCHED"):
        with pytest.raises(NotImplementedError, match=name):
            get(name, native_sched=True)
    # DDIM and PNDM are unaffected by the switch
    m, s, gp = get("DDIM-SCHED", native_sched=True)
    assert type(s) is DDIMScheduler and type(gp(m, s)) is DDIMPipeline
    m, s, gp = get("PNDM-SCHED", native_sched=True)
    assert type(s) is PNDMScheduler and type(gp(m, s)) is PNDMPipeline
    import inspect
    for fn in (DiffuserModelSched.get_pretrained, DiffuserModelSched.get_trained, DiffuserModelSched.get_model_sched):
        assert inspect.signature(fn).parameters["native_sched"].default is False


def test_cli_whitelist(tmp_path, monkeypatch):
    import baddiffusion as cli
    monkeypatch.chdir(tmp_path)
    base = ["--project", "default", "--dataset", "CIFAR10", "--batch", "64", "--ckpt", "DDPM-CIFAR10-32", "-o"]
    plain = cli.setup(["--mode", "train"] + base, write=False)
    assert plain.native_sched is False and plain.infer_steps is None                    # existing commands are unchanged
    cfg = cli.setup(["--mode", "train", "--sched", "DPM_SOLVER_PP_O2-SCHED", "--native_sched", "--infer_steps", "10"] + base)
    assert cfg.native_sched is True and cfg.infer_steps == 10
    saved = json.load(open(os.path.join(cfg.output_dir, "args.json")))
    assert saved["native_sched"] is True and saved["infer_steps"] == 10
    for mode in ("sampling", "measure"):
        c = cli.setup(["--mode", mode, "--ckpt", cfg.output_dir, "--native_sched", "--infer_steps", "15"], write=False)
        assert c.native_sched is True and c.infer_steps == 15 and c.sched == "DPM_SOLVER_PP_O2-SCHED"
        c = cli.setup(["--mode", mode, "--ckpt", cfg.output_dir], write=False)           # the sampler is that command's choice
        assert c.native_sched is False and c.infer_steps == 10
    with pytest.raises(NotImplementedError, match="native_sched"):
        cli.setup(["--mode", "resume", "--ckpt", cfg.output_dir, "--native_sched"], write=False)
    with pytest.raises(NotImplementedError, match="infer_steps"):
        cli.setup(["--mode", "resume", "--ckpt", cfg.output_dir, "--infer_steps", "5"], write=False)
    assert cli.setup(["--mode", "resume", "--ckpt", cfg.output_dir], write=False).native_sched is True


def test_with_default_steps_reaches_calls_that_name_no_count():
    from baddiffusion_amd.pipelines import DDPMPipeline, with_default_steps
    from baddiffusion_amd.schedulers import DDPMScheduler

    class Probe(DDPMPipeline):
        def __call__(self, batch_size=1, num_inference_steps=1000, **kw):
            return num_inference_steps
    p = with_default_steps(Probe(_NoUNet(), DDPMScheduler()), 7)
    assert p() == 7 and p(num_inference_steps=3) == 3 and type(p).__name__ == "Probe" and isinstance(p, Probe)
    assert p.noise_draws() == 6 and p.noise_draws(num_inference_steps=4) == 3            # DDPM draws for every t > 0


def test_elijah_defense_accepts_the_dpm_names(tmp_path):
    import elijah_defense as E
    from baddiffusion_amd.pipelines import DDIMPipeline, DPMSolverPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    assert set(DPM_NAMES) < set(E.SCHED_CHOICES) and "UNIPC-SCHED" not in E.SCHED_CHOICES
    ckpt_sched = DDPMScheduler(num_train_timesteps=400)
    for name, (order, algorithm) in DPM_NAMES.items():
        cfg = E.get_config(["--ckpt", "x", "--sched", name, "--infer_steps", "12", "--output_dir", str(tmp_path)])
        assert cfg.sched == name and cfg.infer_steps == 12
        p = E.make_pipeline(cfg, _NoUNet(), ckpt_sched)
        assert type(p) is DPMSolverPipeline and (p.scheduler.config.solver_order, p.scheduler.config.algorithm_type) == (order, algorithm)
        assert torch.equal(p.scheduler.betas, ckpt_sched.betas)
    cfg = E.get_config(["--ckpt", "x", "--output_dir", str(tmp_path)])
    assert type(E.make_pipeline(cfg, _NoUNet(), ckpt_sched)) is DDIMPipeline and cfg.infer_steps == 50
    with pytest.raises(SystemExit):
        E.get_config(["--ckpt", "x", "--sched", "UNIPC-SCHED", "--output_dir", str(tmp_path)])


# ---------------------------------------------------------------------------------------------------- the C ABI
def _desc(L, **kw):
    d = L.DpmStepDesc(n=16, model_output=4096, sample=8192, m1=12288, m2=16384, m0_out=20480, prev_out=24576, convert=1, alpha_s=0.8,
                      sigma_s=0.6, cx=1.0, c0=1.0, c1=1.0, c2=1.0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_dpm_step_rejects_bad_arguments_without_gpu():
    """the argument checks run on the host before any launch: negative status and a bd_last_error that names the entry point"""
    from baddiffusion_amd import _lib as L
    lib, INVALID = L.load(), -1
    assert lib.bd_dpm_step(None, None) == INVALID and b"bd_dpm_step: null descriptor" in lib.bd_last_error()
    cases = [(dict(n=0), b"n=0"), (dict(n=-4), b"n=-4"), (dict(model_output=None), b"null pointer"), (dict(sample=None), b"null pointer"),
             (dict(prev_out=None), b"null pointer"), (dict(model_output=4100), b"model_output is not 16-byte aligned"),
             (dict(sample=8200), b"sample is not 16-byte aligned"), (dict(m1=12292), b"m1 is not 16-byte aligned"),
             (dict(m2=16392), b"m2 is not 16-byte aligned"), (dict(m0_out=20484), b"m0_out is not 16-byte aligned"),
             (dict(prev_out=24580), b"prev_out is not 16-byte aligned"),
             # partial overlaps: 16 floats = 64 bytes
             (dict(prev_out=8192 + 16), b"prev_out overlaps sample"), (dict(prev_out=8192 - 48), b"prev_out overlaps sample"),
             (dict(prev_out=4096 + 32), b"prev_out overlaps model_output"), (dict(m0_out=16384 + 16), b"m0_out overlaps m2"),
             (dict(m0_out=12288 - 16), b"m0_out overlaps m1"), (dict(m0_out=24576), b"m0_out overlaps prev_out"),
             (dict(m0_out=24576 + 48), b"m0_out overlaps prev_out"), (dict(m0_out=8192, prev_out=8192), b"m0_out overlaps prev_out")]
    for kw, what in cases:
        assert lib.bd_dpm_step(ctypes.byref(_desc(L, **kw)), None) == INVALID, kw
        msg = lib.bd_last_error()
        assert b"bd_dpm_step" in msg and what in msg, (kw, msg)


def test_descriptor_layout_matches_the_header():
    from baddiffusion_amd import _lib as L
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "bd_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(bd_dpm_step_desc), ' \
           'offsetof(bd_dpm_step_desc, prev_out), offsetof(bd_dpm_step_desc, cx), offsetof(bd_dpm_step_desc, clip_range));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    D = L.DpmStepDesc
    assert got == [ctypes.sizeof(D), D.prev_out.offset, D.cx.offset, D.clip_range.offset]
