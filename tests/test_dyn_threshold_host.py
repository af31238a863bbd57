"""CPU: dynamic thresholding for DDPM and DDIM without a GPU -- the restated quantile and thresholded steps (tests/_threshold_exact.py)
against the reference's stored values (tests/golden/threshold.npz, written by make_golden_threshold.py) bit for bit, the exact host fmaf,
the C ABI (descriptor layouts, exported symbols, argument rejections, the plan query), the config round trip, and the factory and
command-line wiring."""
import ctypes
import json
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import _step_exact as X
from tests import _threshold_exact as T
from tests.golden import cases as C
from tests.golden import cases_threshold as CT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
f32 = np.float32


class _NoUNet:
    """what a pipeline needs of a UNet before its first evaluation"""
    device = torch.device("cpu")


# ---------------------------------------------------------------------------------------------------- the restatement
def test_round_to_f32_is_round_to_nearest_even():
    one, ulp = Fraction(1), Fraction(1, 2 ** 23)
    assert T.round_to_f32(one + ulp / 2) == f32(1)                                  # a tie: down to even
    assert T.round_to_f32(one + ulp + ulp / 2) == f32(1) + f32(2.0 ** -22)          # a tie: up to even
    assert T.round_to_f32(one + ulp / 2 + Fraction(1, 2 ** 80)) == np.nextafter(f32(1), f32(2))
    tiny = Fraction(1, 2 ** 149)                                                    # the smallest denormal
    assert T.round_to_f32(tiny) == f32(2.0 ** -149) and T.round_to_f32(tiny / 2) == 0 and T.round_to_f32(3 * tiny / 2) == f32(2.0 ** -148)
    assert T.round_to_f32(-tiny * 5) == -f32(5 * 2.0 ** -149)
    big = Fraction(int(np.finfo(f32).max.astype(np.float64)))
    assert T.round_to_f32(big) == np.finfo(f32).max and np.isinf(T.round_to_f32(big * 2))
    rng = np.random.default_rng(0)
    for v in rng.standard_normal(200) * 10.0 ** rng.uniform(-40, 30, 200):          # float64 -> fp32 is one correctly rounded step
        assert T.round_to_f32(Fraction(float(v))) == f32(v)


def test_fma32_rounds_once():
    # a * b + c where the float64 detour rounds twice: the exact sum lies just above a tie of fp32 that float64 cannot see
    a, b = f32(1 + 2.0 ** -12), f32(1 + 2.0 ** -12)                                 # a b = 1 + 2^-11 + 2^-24: exact in float64
    c = f32(2.0 ** -60)
    assert T.fma32(a, b, c) == np.nextafter(f32(1 + 2.0 ** -11), f32(2))            # above the tie: up
    assert f32(np.float64(a) * np.float64(b) + np.float64(c)) == f32(1 + 2.0 ** -11)       # the detour lost c, met the tie, went to even
    assert np.isnan(T.fma32(0.0, np.inf, 1.0)) and T.fma32(2.0, 3.0, 1.0) == 7 and np.isinf(T.fma32(1.0, np.inf, 1.0))
    assert T.fma32(0.25, 2.0 ** -149, 0.0) == 0 and T.fma32(0.75, 2.0 ** -149, 0.0) == f32(2.0 ** -149)


@pytest.mark.parametrize("shape", CT.Q_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_quantile_statement_equals_torch_quantile(golden, shape):
    """the two-branch fused interpolation on the sorted |x|, in every regime and at every ratio, against torch.quantile's stored bits"""
    B, m = shape
    g = golden("threshold")
    for regime in CT.REGIMES:
        x = CT.quantile_input(B, m, regime).numpy()
        for q in CT.QS:
            CT.assert_nan_equal_bits(T.abs_quantile_stmt(x, q), CT.quantile_expected(g, B, m, regime, q))


def test_quantile_cases_cover_what_they_name(golden):
    g = golden("threshold")
    assert {(1, 1), (2, 2), (3, 7), (2, 192), (5, 193), (3, 105), (2, 3072), (3, 3073), (2, 12288), (2, 196608), (300, 192)} <= set(CT.Q_SHAPES)
    assert {(2, CT.SWITCH_M + d) for d in (-1, 0, 1)} <= set(CT.Q_SHAPES) and set(CT.QS) == {0.995, 0.9, 0.5, 1.0, 0.0}
    x = CT.quantile_input(5, 193, "quarters")
    assert bool((x * 4 == torch.round(x * 4)).all()) and x.abs().unique().numel() < 40             # crowded buckets
    lo, hi, _ = T.quantile_ranks(0.9, 193)
    s = np.sort(np.abs(x.numpy()), axis=1)
    assert (s[:, lo] == s[:, hi]).any()                                                             # the bracketing values tie
    assert CT.quantile_input(3, 105, "equal").abs().unique().tolist() == [1.25]
    low = CT.quantile_input(2, 3072, "lowbits").abs().view(torch.int32)
    assert int((low >> 10).unique().numel()) == 1 and int(low.unique().numel()) > 900              # one prefix of 21 bits
    tiny = CT.quantile_input(2, 3072, "tiny")
    bits = tiny.view(torch.int32)
    assert bool((bits == 0).any()) and bool((bits == -(2 ** 31)).any()) and float(tiny.abs().max()) < 1.1754944e-38 and float(tiny.abs().max()) > 0
    assert np.all(CT.quantile_expected(g, 2, 3072, "tiny", 0.0) == 0) and np.all(CT.quantile_expected(g, 2, 3072, "tiny", 0.0).view(np.uint32) == 0)
    nan = CT.quantile_expected(g, 5, 193, "nan", 0.0)
    assert np.isnan(nan[0]) and not np.isnan(nan[1:]).any()
    assert np.isnan(CT.quantile_expected(g, 5, 193, "inf", 0.995)[-1]) and np.isfinite(CT.quantile_expected(g, 5, 193, "inf", 0.9)).all()
    # the other branch, or the unfused form of the right one, is not the reference's arithmetic: the cases tell them apart
    miss_unfused = miss_other = 0
    for regime in ("spread",):
        a = np.sort(np.abs(CT.quantile_input(300, 192, regime).numpy()), axis=1)
        for q in (0.995, 0.9, 0.5):
            want = CT.quantile_expected(g, 300, 192, regime, q)
            lo, hi, w = T.quantile_ranks(q, 192)
            d = (a[:, hi] - a[:, lo]).astype(f32)
            if w < 0.5:
                unfused = a[:, lo] + w * d
                other = np.array([T.fma32(-di, f32(1) - w, bi) for di, bi in zip(d, a[:, hi])], dtype=f32)
            else:
                unfused = a[:, hi] - d * (f32(1) - w)
                other = np.array([T.fma32(w, di, ai) for di, ai in zip(d, a[:, lo])], dtype=f32)
            miss_unfused += int((unfused != want).sum())
            miss_other += int((other != want).sum())
    print(f"MEASURE quantile interpolation on 900 spread rows: the unfused form misses {miss_unfused}, the other branch {miss_other}")
    assert miss_unfused > 0 and miss_other > 0


@pytest.mark.parametrize("sched", ("ddpm", "ddim"))
def test_step_statement_equals_the_reference(golden, sched):
    """quantile + thresholded step restated in numpy fp32 against the reference scheduler's prev_sample and pred_original_sample: equal
    bits on every case, and the planted inputs reach all three regimes"""
    g = golden("threshold")
    _, ac = X.tables()
    cases = CT.DDPM_STEP_CASES if sched == "ddpm" else CT.DDIM_STEP_CASES
    seen, interior, wide = set(), 0, 0
    for i, case in enumerate(cases):
        t, kind, smax, ratio, shape = case
        x, e, z = (v.numpy() for v in CT.step_inputs(sched, i, case, torch.from_numpy(ac)))
        if sched == "ddpm":
            prev, x0, q = T.ddpm_thr_stmt(ac, T.ddpm_case(t, t - 1, kind), x, e, z, smax, ratio)
        else:
            prev, x0, q = T.ddim_thr_stmt(ac, T.ddim_case(t, t - 1000 // CT.DDIM_STEPS, kind), x, e, z, smax, ratio)
        want_prev, want_x0 = CT.step_expected(g, sched, i)
        assert X.same_bits(prev, want_prev) and X.same_bits(x0, want_x0), case
        assert float(np.abs(x0).max()) <= 1.0
        regimes = {CT.regime_of(float(v), smax) for v in q}
        seen |= regimes
        wide += smax > 1.0
        interior += smax > 1.0 and 1 in regimes
    assert seen == {0, 1, 2} and 2 * interior >= wide
    want = {(t, k, s, r, sh) for t in (C.DDPM_TS if sched == "ddpm" else C.DDIM_TS) for k in (CT.VARIANCE_TYPES if sched == "ddpm" else CT.ETAS)
            for s in (1.0, 1.5, 3.0) for r in (0.995, 0.9) for sh in ((2, 3, 8, 8), (3, 3, 5, 7))}
    assert set(cases) == want and len(cases) == len(want)


@pytest.mark.parametrize("case", CT.CHAIN_CASES, ids=lambda c: CT.chain_tag(*c))
def test_chain_statement_equals_the_reference(golden, case):
    sched, smax = case
    g = golden("threshold")
    ref = g[CT.chain_tag(sched, smax)]
    xs = T.chain_stmt(sched, smax, CT.CHAIN_RATIO, CT.CHAIN_STEPS, C.pndm_fake_model, C.pndm_init(), CT.CHAIN_NOISE_SEED)
    assert len(xs) == len(ref) == CT.CHAIN_STEPS
    for i, (x, want) in enumerate(zip(xs, ref)):
        assert X.same_bits(x, want), (case, i)
    assert 0 < float(g[f"{CT.chain_tag(sched, smax)}_dev64"]) < 1e-5


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_descriptor_layouts_match_the_header():
    from baddiffusion_amd import _lib as L
    fields = {"bd_ddpm_step_desc": (L.DdpmStepDesc, ("clip_defense_range", "x0_quantile", "image_elems", "sample_max_value")),
              "bd_ddim_step_desc": (L.DdimStepDesc, ("clip_sample_range", "x0_quantile", "image_elems", "sample_max_value")),
              "bd_abs_quantile_desc": (L.AbsQuantileDesc, ("m", "x", "model_output", "alphas_cumprod", "n_alphas", "t", "q", "out", "workspace",
                                                           "workspace_bytes")),
              "bd_abs_quantile_plan_info": (L.AbsQuantilePlanInfo, ("path", "workgroups", "threads", "values_per_thread", "passes", "switch_m",
                                                                    "workspace_bytes"))}
    body = "".join(f'printf("%zu ", sizeof({n}));' + "".join(f'printf("%zu ", offsetof({n}, {f}));' for f in fs) for n, (_, fs) in fields.items())
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "bd_hip.h"\nint main(){' + body + 'printf("%d %d", BD_AQ_REGISTERS, BD_AQ_STREAM);return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    want = []
    for cls, fs in fields.values():
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fs]
    assert got == want + [L.AQ_REGISTERS, L.AQ_STREAM]
    # the new fields stand at the end: what came before keeps its place
    for cls in (L.DdpmStepDesc, L.DdimStepDesc):
        assert [n for n, _ in cls._fields_][-3:] == ["x0_quantile", "image_elems", "sample_max_value"]


def test_symbols_are_declared_exported_and_bound():
    from baddiffusion_amd import _lib as L
    from baddiffusion_amd import ops
    from tests.test_abi import header_symbols
    new = {"bd_abs_quantile", "bd_abs_quantile_workspace_bytes", "bd_abs_quantile_plan"}
    assert new <= set(header_symbols()) and new <= set(L.SIGNATURES)
    lib = L.load()
    exported = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    for name in new:
        assert f" T {name}\n" in exported and getattr(lib, name) is not None
    assert callable(ops.abs_quantile) and callable(ops.abs_quantile_plan)


def _qdesc(L, **kw):
    p = 4096                  # an address that is never dereferenced: every call below returns before its launch
    base = dict(B=2, m=192, x=p, model_output=None, alphas_cumprod=None, n_alphas=0, t=0, q=0.995, out=2 * p, workspace=None, workspace_bytes=0)
    base.update(kw)
    return L.AbsQuantileDesc(**base)


def test_quantile_rejections_without_a_gpu():
    from baddiffusion_amd import _lib as L
    lib = L.load()
    assert lib.bd_abs_quantile(None, None) == INVALID and b"null descriptor" in lib.bd_last_error()
    cases = [(dict(x=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(B=0), b"B=0 must be positive"),
             (dict(B=-3), b"B=-3 must be positive"), (dict(m=0), b"m=0 must be positive"), (dict(m=-1), b"m=-1 must be positive"),
             (dict(B=2, m=2 ** 30), b"below 2^31"), (dict(B=1, m=2 ** 31), b"below 2^31"), (dict(B=65536, m=32768), b"below 2^31"),
             (dict(q=-0.001), b"must lie in [0, 1]"), (dict(q=1.001), b"must lie in [0, 1]"), (dict(q=float("nan")), b"must lie in [0, 1]"),
             (dict(model_output=8192), b"without alphas_cumprod"),
             (dict(model_output=8192, alphas_cumprod=12288, n_alphas=1000, t=1000), b"t=1000 outside the table of 1000"),
             (dict(model_output=8192, alphas_cumprod=12288, n_alphas=1000, t=-1), b"t=-1 outside the table of 1000")]
    for kw, what in cases:
        assert lib.bd_abs_quantile(ctypes.byref(_qdesc(L, **kw)), None) == INVALID, kw
        msg = lib.bd_last_error()
        assert b"bd_abs_quantile" in msg and what in msg, (kw, msg)
    info = L.AbsQuantilePlanInfo()
    assert lib.bd_abs_quantile_plan(2, 192, None) == INVALID and b"null output" in lib.bd_last_error()
    for B, m in ((0, 5), (5, 0), (2, 2 ** 30)):
        assert lib.bd_abs_quantile_plan(B, m, ctypes.byref(info)) == INVALID and b"bd_abs_quantile_plan" in lib.bd_last_error()


def test_step_rejections_without_a_gpu():
    from baddiffusion_amd import _lib as L
    lib = L.load()
    p = 4096
    common = dict(model_output=p, sample=2 * p, noise=3 * p, prev_sample=4 * p, alphas_cumprod=5 * p, t=5, prev_t=4, x0_quantile=6 * p,
                  sample_max_value=1.5)
    for fn, cls, name in ((lib.bd_ddpm_step, L.DdpmStepDesc, b"bd_ddpm_step"), (lib.bd_ddim_step, L.DdimStepDesc, b"bd_ddim_step")):
        for kw, what in ((dict(n=384, image_elems=0), b"no multiple of image_elems=0"), (dict(n=384, image_elems=-192), b"no multiple"),
                         (dict(n=385, image_elems=192), b"n=385 that is no multiple of image_elems=192"),
                         (dict(n=2 ** 31, image_elems=2 ** 20), b">= 2^31")):
            assert fn(ctypes.byref(cls(**common, **kw)), None) == INVALID, kw
            msg = lib.bd_last_error()
            assert name in msg and what in msg, (kw, msg)


def test_plan_query():
    from baddiffusion_amd import ops
    for B, m in CT.Q_SHAPES:
        p = ops.abs_quantile_plan(B, m)
        registers = m <= CT.SWITCH_M
        assert p["path"] == (0 if registers else 1) and p["workgroups"] == B and p["passes"] == 3 and p["switch_m"] == CT.SWITCH_M
        assert p["threads"] == (256 if registers else 1024) and p["workspace_bytes"] == 0
        assert p["threads"] * p["values_per_thread"] >= m                     # every value has a slot
        if not registers:
            assert p["values_per_thread"] == -(-m // 1024)
    assert ops.abs_quantile_plan(2048, 3072)["path"] == 0 and ops.abs_quantile_plan(4, 196608)["path"] == 1      # the two workloads
    # the constants the plan states are the ones in the source
    src = open(os.path.join(ROOT, "baddiffusion_amd", "csrc", "elementwise.hip")).read()
    assert "AQ_REG_THREADS = 256, AQ_REG_VPT = 16;" in src and "AQ_STREAM_THREADS = 1024;" in src
    with pytest.raises(RuntimeError, match="B=0 must be positive"):
        ops.abs_quantile_plan(0, 5)


def test_ops_refuse_cpu_tensors_and_bad_layouts():
    from baddiffusion_amd import ops
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.abs_quantile(x, 0.5)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.ddpm_step(x, x, x, torch.zeros(10), 5, 4, x0_quantile=torch.zeros(2))


# ---------------------------------------------------------------------------------------------------- config, factory, command lines
def test_config_round_trip(tmp_path):
    from baddiffusion_amd.model import load_scheduler, save_scheduler
    from baddiffusion_amd.pipelines import DDIMPipeline
    from baddiffusion_amd.schedulers import DDIMScheduler, DDPMScheduler
    for cls in (DDPMScheduler, DDIMScheduler):
        s = cls(**CT.scheduler_kwargs(1.5, 0.9))
        d = tmp_path / cls.__name__
        save_scheduler(s, str(d))
        saved = json.load(open(d / "scheduler_config.json"))
        assert (saved["thresholding"], saved["sample_max_value"], saved["dynamic_thresholding_ratio"]) == (True, 1.5, 0.9)
        back = load_scheduler(str(d))
        assert type(back) is cls and dict(back.config) == dict(s.config)
        # DDIMPipeline re-creates its scheduler from the config: the three keys survive
        p = DDIMPipeline(_NoUNet(), s)
        assert type(p.scheduler) is DDIMScheduler
        assert (p.scheduler.config.thresholding, p.scheduler.config.sample_max_value, p.scheduler.config.dynamic_thresholding_ratio) == (True, 1.5, 0.9)
    assert {"thresholding", "dynamic_thresholding_ratio", "sample_max_value"} <= set(DDIMScheduler._KEYS)
    assert DDPMScheduler().config.thresholding is False and DDIMScheduler().config.thresholding is False


def test_factory_takes_dyn_threshold():
    import inspect
    from baddiffusion_amd.model import DiffuserModelSched
    from baddiffusion_amd.pipelines import DDIMPipeline, DDPMPipeline
    from baddiffusion_amd.schedulers import DDIMScheduler, DDPMScheduler
    get = lambda name, **kw: DiffuserModelSched.get_pretrained("DDPM-CIFAR10-32", noise_sched_type=name, allow_random_init=True, **kw)      # noqa: E731
    for name, scls, pcls in (("DDPM-SCHED", DDPMScheduler, DDPMPipeline), ("DDIM-SCHED", DDIMScheduler, DDIMPipeline), (None, DDPMScheduler, DDPMPipeline)):
        m, s, gp = get(name, dyn_threshold=1.5)
        assert type(s) is scls and (s.config.thresholding, s.config.sample_max_value, s.config.dynamic_thresholding_ratio) == (True, 1.5, 0.995)
        p = gp(m, s)
        assert type(p) is pcls and p.scheduler.config.thresholding is True and p.scheduler.config.sample_max_value == 1.5
        m, s, _ = get(name, dyn_threshold=3.0, dyn_threshold_ratio=0.9)
        assert (s.config.sample_max_value, s.config.dynamic_thresholding_ratio) == (3.0, 0.9)
        m, s, _ = get(name)
        assert s.config.thresholding is False and s.config.sample_max_value == 1.0
        del m
    from baddiffusion_amd.sched_names import SCHEDS
    others = sorted(set(SCHEDS) - {"DDPM-SCHED", "DDIM-SCHED"})
    assert len(others) > 20 and not any(SCHEDS[name].dyn_threshold for name in others)
    for name in others:
        for native in (False, True):
            with pytest.raises(NotImplementedError, match=f"dyn_threshold with {name}: dynamic thresholding runs in the DDPM and DDIM steps only"):
                get(name, dyn_threshold=1.5, native_sched=native)
    with pytest.raises(ValueError, match="must be >= 1"):
        get("DDPM-SCHED", dyn_threshold=0.5)
    with pytest.raises(ValueError, match="dyn_threshold_ratio=1.5"):
        get("DDIM-SCHED", dyn_threshold=1.5, dyn_threshold_ratio=1.5)
    for fn in (DiffuserModelSched._get_model_sched, DiffuserModelSched.get_pretrained, DiffuserModelSched.get_trained):
        sig = inspect.signature(fn).parameters
        assert sig["dyn_threshold"].default is None and sig["dyn_threshold_ratio"].default == 0.995


def test_cli_whitelist_and_records(tmp_path, monkeypatch):
    import baddiffusion as cli
    monkeypatch.chdir(tmp_path)
    base = ["--project", "default", "--dataset", "CIFAR10", "--batch", "64", "--ckpt", "DDPM-CIFAR10-32", "-o"]
    plain = cli.setup(["--mode", "train"] + base, write=False)
    assert plain.dyn_threshold is None and plain.dyn_threshold_ratio == 0.995            # existing commands are unchanged
    cfg = cli.setup(["--mode", "train", "--sched", "DDIM-SCHED", "--dyn_threshold", "1.5"] + base)
    assert cfg.dyn_threshold == 1.5 and cfg.dyn_threshold_ratio == 0.995
    saved = json.load(open(os.path.join(cfg.output_dir, "args.json")))
    assert saved["dyn_threshold"] == 1.5 and saved["dyn_threshold_ratio"] is None
    for mode, record in (("sampling", "sampling.json"), ("measure", "measure.json")):
        c = cli.setup(["--mode", mode, "--ckpt", cfg.output_dir, "--dyn_threshold", "3.0", "--dyn_threshold_ratio", "0.9"])
        assert c.dyn_threshold == 3.0 and c.dyn_threshold_ratio == 0.9 and c.sched == "DDIM-SCHED"
        rec = json.load(open(os.path.join(cfg.output_dir, record)))
        assert rec["dyn_threshold"] == 3.0 and rec["dyn_threshold_ratio"] == 0.9
        assert cli.setup(["--mode", mode, "--ckpt", cfg.output_dir], write=False).dyn_threshold == 1.5      # the run's own, as --infer_steps
    with pytest.raises(NotImplementedError, match="dyn_threshold"):
        cli.setup(["--mode", "resume", "--ckpt", cfg.output_dir, "--dyn_threshold", "1.5"], write=False)
    with pytest.raises(ValueError, match="--dyn_threshold_ratio needs --dyn_threshold"):
        cli.setup(["--mode", "train", "--dyn_threshold_ratio", "0.9"] + base, write=False)
    # the score file names the clamp its samples were drawn with
    import inspect
    assert "dyn_threshold=float(config.dyn_threshold)" in inspect.getsource(cli.measure)


def test_elijah_and_inpaint_command_lines(tmp_path):
    import elijah_defense as E
    import inpaint_eval as I
    from baddiffusion_amd.pipelines import DDIMPipeline, DDPMPipeline
    from baddiffusion_amd.schedulers import DDIMScheduler, DDPMScheduler
    ckpt_sched = DDPMScheduler(num_train_timesteps=400)
    for name, pcls, scls in (("DDIM-SCHED", DDIMPipeline, DDIMScheduler), ("DDPM-SCHED", DDPMPipeline, DDPMScheduler)):
        cfg = E.get_config(["--ckpt", "x", "--sched", name, "--dyn_threshold", "1.5", "--dyn_threshold_ratio", "0.9", "--output_dir", str(tmp_path)])
        assert (cfg.dyn_threshold, cfg.dyn_threshold_ratio) == (1.5, 0.9)
        rec = json.load(open(os.path.join(cfg.output_dir, "config.json")))
        assert (rec["dyn_threshold"], rec["dyn_threshold_ratio"]) == (1.5, 0.9)
        p = E.make_pipeline(cfg, _NoUNet(), ckpt_sched)
        assert type(p) is pcls and type(p.scheduler) is scls and torch.equal(p.scheduler.betas, ckpt_sched.betas)
        assert (p.scheduler.config.thresholding, p.scheduler.config.sample_max_value, p.scheduler.config.dynamic_thresholding_ratio) == (True, 1.5, 0.9)
        assert ckpt_sched.config.thresholding is False                       # the scheduler that is saved back keeps its config
        plain = E.make_pipeline(E.get_config(["--ckpt", "x", "--sched", name, "--output_dir", str(tmp_path)]), _NoUNet(), ckpt_sched)
        assert plain.scheduler.config.thresholding is False
    for name in ("DPM_SOLVER_PP_O2-SCHED", "UNIPC_O2-SCHED", "DEIS_O3-SCHED", "HEUN_O2-SCHED", "LMSD_O4-SCHED"):
        with pytest.raises(NotImplementedError, match=f"dyn_threshold with {name}"):
            E.get_config(["--ckpt", "x", "--sched", name, "--dyn_threshold", "1.5", "--output_dir", str(tmp_path)])
    with pytest.raises(SystemExit):
        E.get_config(["--ckpt", "x", "--dyn_threshold_ratio", "0.9", "--output_dir", str(tmp_path)])
    assert 'result["dyn_threshold"]' in open(os.path.join(ROOT, "elijah_defense.py")).read()
    # inpainting samples through RePaint, which has no thresholding: the flag is known there and refused with the reason
    with pytest.raises(NotImplementedError, match="RePaintScheduler, which has no dynamic thresholding"):
        I.get_config(["--ckpt", "x", "--dyn_threshold", "1.5", "--output_dir", str(tmp_path)])
    assert I.get_config(["--ckpt", "x", "--output_dir", str(tmp_path)]).clip is True
