"""CPU: the host side of RePaint inpainting -- the timestep schedule against the reference's (tests/golden/repaint.npz), draw counts,
scheduler configuration and persistence, what is rejected before any launch (CPU tensors, PIL inputs, bad descriptor fields), the ctypes
descriptor layouts, and inpaint_eval.py's command line.  Nothing here needs a GPU."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.golden import cases_repaint as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoUNet:
    """what RePaintPipeline needs of a UNet before its first evaluation"""
    device = torch.device("cpu")


def _pipe(scheduler=None):
    from baddiffusion_amd.pipelines import RePaintPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    return RePaintPipeline(unet=_NoUNet(), scheduler=scheduler or DDPMScheduler())


@pytest.mark.parametrize("case", CR.TIMESTEP_CASES, ids=lambda c: "_".join(map(str, c)))
def test_timesteps_equal_the_reference(case, golden):
    from baddiffusion_amd.schedulers import RePaintScheduler
    s = RePaintScheduler()
    s.set_timesteps(*case)
    want = golden("repaint")["ts_%d_%d_%d" % case]
    assert s.timesteps.dtype == torch.int64 and np.array_equal(s.timesteps.numpy(), want)
    assert s.num_inference_steps == case[0]


def test_timestep_fixture_is_the_documented_one(golden):
    g = golden("repaint")
    assert g["ts_4_1_2"].tolist() == CR.TS_4_1_2
    assert len(g["ts_250_10_10"]) == 4570 and len(g["ts_10_2_3"]) == 42 and len(g["ts_6_2_2"]) == 14
    assert g["ts_3_5_5"].tolist() == [666, 333, 0]                                      # no jumps


def test_set_timesteps_clamps_to_the_training_length():
    from baddiffusion_amd.schedulers import RePaintScheduler
    s = RePaintScheduler(num_train_timesteps=100)
    s.set_timesteps(250, 10, 10)
    assert s.num_inference_steps == 100 and int(s.timesteps.max()) == 99 and int(s.timesteps[-1]) == 0


def test_noise_draws_counts():
    p = _pipe()
    assert p.noise_draws(num_inference_steps=4, jump_length=1, jump_n_sample=2) == 757          # 7 evaluations + 3 undos of 250 sub-steps
    assert p._counts(4, 1, 2) == (7, 3)
    assert p._counts(250, 10, 10) == (2410, 2160)
    assert p.noise_draws() == 2410 + 2160 * 4
    assert p.noise_draws(num_inference_steps=10, jump_length=2, jump_n_sample=3) == 26 + 16 * 100
    assert p.noise_draws(num_inference_steps=3, jump_length=5, jump_n_sample=5) == 3


def test_from_config_of_a_ddpm_scheduler():
    from baddiffusion_amd.schedulers import DDPMScheduler, RePaintScheduler
    d = DDPMScheduler(num_train_timesteps=500, beta_start=0.0002, beta_end=0.03, beta_schedule="scaled_linear", clip_sample=False,
                      variance_type="fixed_large")
    s = RePaintScheduler.from_config(d.config)
    assert dict(s.config) == {"num_train_timesteps": 500, "beta_start": 0.0002, "beta_end": 0.03, "beta_schedule": "scaled_linear", "eta": 0.0,
                              "trained_betas": None, "clip_sample": False}
    assert torch.equal(s.betas, d.betas) and torch.equal(s.alphas_cumprod, d.alphas_cumprod)
    assert float(s.final_alpha_cumprod) == 1.0 and s.eta == 0.0 and len(s) == 500
    s.eta = 0.75                                                                        # assignable, as the reference's pipeline does
    assert s.eta == 0.75
    assert type(_pipe(d).scheduler) is RePaintScheduler and _pipe(d).scheduler.config.clip_sample is False
    with pytest.raises(NotImplementedError):
        RePaintScheduler(beta_schedule="squaredcos_cap_v2")


def test_get_variance_is_the_reference_formula():
    from baddiffusion_amd.schedulers import RePaintScheduler
    s = RePaintScheduler()
    s.set_timesteps(10)
    ac = s.alphas_cumprod
    assert float(s._get_variance(500)) == float(((1 - ac[400]) / (1 - ac[500])) * (1 - ac[500] / ac[400]))
    assert float(s._get_variance(0)) == 0.0                                             # prev_t < 0: final_alpha_cumprod = 1


def test_add_noise_raises_with_the_reference_message():
    from baddiffusion_amd.schedulers import RePaintScheduler
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(NotImplementedError, match=r"Use `DDPMScheduler.add_noise\(\)` to train for sampling with RePaint."):
        RePaintScheduler().add_noise(x, x, torch.tensor([0]))


def test_cpu_tensors_and_pil_inputs_are_rejected():
    from PIL import Image
    from baddiffusion_amd import ops
    from baddiffusion_amd.schedulers import RePaintScheduler
    s = RePaintScheduler()
    s.set_timesteps(10)
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(RuntimeError):
        s.step(x, 500, x, x, torch.ones(1, 1, 8, 8))
    with pytest.raises(RuntimeError):
        s.undo_step(x, 400)
    with pytest.raises(RuntimeError):
        ops.repaint_step(x, x, x, x, x, s.alphas_cumprod, 500, 400)
    with pytest.raises(RuntimeError):
        ops.repaint_undo(x, [x], s.betas, 400)
    pil = Image.new("RGB", (16, 16))
    with pytest.raises(TypeError, match="PIL"):
        _pipe()(pil, torch.ones(1, 1, 16, 16))
    with pytest.raises(TypeError, match="PIL"):
        _pipe()(torch.zeros(1, 3, 16, 16), pil.convert("L"))


def test_load_and_save_scheduler_round_trip(tmp_path):
    from baddiffusion_amd.model import load_scheduler, save_scheduler
    from baddiffusion_amd.schedulers import RePaintScheduler
    s = RePaintScheduler(num_train_timesteps=400, beta_schedule="scaled_linear", eta=0.5, clip_sample=False)
    save_scheduler(s, str(tmp_path / "scheduler"))
    saved = json.load(open(tmp_path / "scheduler" / "scheduler_config.json"))
    assert saved["_class_name"] == "RePaintScheduler"
    back = load_scheduler(str(tmp_path / "scheduler"))
    assert type(back) is RePaintScheduler and dict(back.config) == dict(s.config) and back.eta == 0.5
    assert torch.equal(back.betas, s.betas)


# ---------------------------------------------------------------------------------------------------- the C ABI
def _step_desc(L, **kw):
    d = L.RepaintStepDesc(N=2, C=3, H=4, W=4, model_output=16, sample=16, noise=16, prev_sample=16, original_image=16, mask=16,
                          alphas_cumprod=16, n_alphas=1000, t=500, prev_t=400, final_alpha_cumprod=1.0)
    for i, s in enumerate((48, 16, 4, 1)):
        d.stride[i] = d.orig_stride[i] = d.mask_stride[i] = s
    for k, v in kw.items():
        if isinstance(v, tuple):
            for i, s in enumerate(v):
                getattr(d, k)[i] = s
        else:
            setattr(d, k, v)
    return d


def _undo_desc(L, **kw):
    d = L.RepaintUndoDesc(N=2, C=3, H=4, W=4, sample=16, out=16, betas=16, n_betas=1000, t=400, k=4)
    for i, s in enumerate((48, 16, 4, 1)):
        d.stride[i] = s
    for k, v in kw.items():
        if isinstance(v, tuple):
            for i, s in enumerate(v):
                getattr(d, k)[i] = s
        else:
            setattr(d, k, v)
    return d


def test_entry_points_reject_bad_arguments_without_gpu():
    """every check runs on the host before any launch: negative status, a message naming the entry point, the device never touched (the
    pointers in these descriptors are not addresses of anything)"""
    from baddiffusion_amd import _lib as L
    lib = L.load()
    INVALID = -1

    def step_fails(what, **kw):
        assert lib.bd_repaint_step(ctypes.byref(_step_desc(L, **kw)), None) == INVALID, kw
        msg = lib.bd_last_error()
        assert b"bd_repaint_step" in msg and what in msg, msg

    assert lib.bd_repaint_step(None, None) == INVALID and b"bd_repaint_step: null descriptor" in lib.bd_last_error()
    for field in ("model_output", "sample", "noise", "prev_sample", "original_image", "mask", "alphas_cumprod"):
        step_fails(b"null pointer", **{field: None})
    step_fails(b"t=-1", t=-1)
    step_fails(b"outside the table", t=1000)
    step_fails(b"must be positive", N=0)
    step_fails(b"must be positive", W=-4)
    step_fails(b"negative stride", stride=(48, 16, 4, -1))
    step_fails(b"negative stride", mask_stride=(0, 0, -4, 1))
    step_fails(b"negative stride", shift=16, shift_stride=(0, -16, 4, 1))
    step_fails(b"not a dense layout", stride=(96, 16, 4, 1))
    step_fails(b"not a dense layout", stride=(48, 16, 4, 2))
    big = dict(N=1 << 15, C=1, H=256, W=256, stride=(1 << 16, 1, 256, 1))           # 2^31 elements: the coordinates are 32-bit
    assert lib.bd_repaint_step(ctypes.byref(_step_desc(L, **big)), None) == -2 and b"bd_repaint_step" in lib.bd_last_error()
    assert lib.bd_repaint_undo(ctypes.byref(_undo_desc(L, **big)), (ctypes.c_void_p * 4)(16, 16, 16, 16), None) == -2
    assert b"bd_repaint_undo" in lib.bd_last_error() and b"not supported" in lib.bd_last_error()

    noises = (ctypes.c_void_p * 4)(16, 16, 16, 16)

    def undo_fails(what, nz=noises, **kw):
        assert lib.bd_repaint_undo(ctypes.byref(_undo_desc(L, **kw)), nz, None) == INVALID, kw
        msg = lib.bd_last_error()
        assert b"bd_repaint_undo" in msg and what in msg, msg

    assert lib.bd_repaint_undo(None, noises, None) == INVALID and b"bd_repaint_undo: null descriptor" in lib.bd_last_error()
    undo_fails(b"null pointer", nz=None)
    for field in ("sample", "out", "betas"):
        undo_fails(b"null pointer", **{field: None})
    undo_fails(b"k=0", k=0)
    undo_fails(b"t=-1", t=-1)
    undo_fails(b"exceeds the table", t=997)                         # t + k = 1001 > 1000
    undo_fails(b"exceeds the table", t=400, k=4, n_betas=403)
    undo_fails(b"must be positive", C=0)
    undo_fails(b"negative stride", stride=(48, -16, 4, 1))
    undo_fails(b"not a dense layout", stride=(48, 16, 8, 1))
    undo_fails(b"noises[2] is null", nz=(ctypes.c_void_p * 4)(16, 16, None, 16))


def test_descriptor_sizes_match_the_header():
    """ctypes mirrors vs sizeof() computed by the C compiler from the header, and the per-launch limit of the undo"""
    from baddiffusion_amd import _lib as L
    names = {"bd_repaint_step_desc": L.RepaintStepDesc, "bd_repaint_undo_desc": L.RepaintUndoDesc}
    prog = ('#include <stdio.h>\n#include "bd_hip.h"\nint main(){' + "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names) +
            'printf("max %d\\n", BD_REPAINT_UNDO_MAX);return 0;}')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True).stdout.strip().splitlines())
    for n, cls in names.items():
        assert ctypes.sizeof(cls) == int(out[n]), (n, ctypes.sizeof(cls), out[n])
    assert int(out["max"]) == L.REPAINT_UNDO_MAX >= 4


# ---------------------------------------------------------------------------------------------------- inpaint_eval.py
def test_inpaint_eval_get_config(tmp_path):
    import inpaint_eval as E
    ckpt = tmp_path / "ckpt_small"
    ckpt.mkdir()
    base = ["--ckpt", str(ckpt), "--output_dir", str(tmp_path / "out")]
    cfg = E.get_config(base)
    assert (cfg.n, cfg.batch, cfg.mask, cfg.infer_steps, cfg.jump_length, cfg.jump_n_sample, cfg.eta) == (16, 16, "box", 250, 10, 10, 0.0)
    assert cfg.target is None and cfg.trigger == "BOX_14" and cfg.asr_threshold is None and cfg.consistent is False and cfg.seed == 0
    assert os.path.basename(cfg.output_dir) == "res_inpaint_box_is250_j10x10_eta0.0_ckpt_small"
    cfg = E.get_config(base + ["--target", "HAT"])
    assert cfg.target == "HAT" and cfg.asr_threshold == 1e-3                              # the default applies once --target is given
    cfg = E.get_config(base + ["--mask", "half", "--n", "4", "--batch", "2", "--infer_steps", "4", "--jump_length", "1", "--jump_n_sample", "2",
                               "--eta", "1.0", "--trigger", "STOP_SIGN_14", "--target", "SHIFT", "--asr_threshold", "0.01", "--consistent",
                               "--dataset", "CIFAR10", "--dataset_path", str(tmp_path), "--seed", "3"])
    assert (cfg.mask, cfg.n, cfg.batch, cfg.infer_steps, cfg.jump_length, cfg.jump_n_sample, cfg.eta) == ("half", 4, 2, 4, 1, 2, 1.0)
    assert (cfg.trigger, cfg.target, cfg.asr_threshold, cfg.consistent, cfg.seed) == ("STOP_SIGN_14", "SHIFT", 0.01, True, 3)
    assert os.path.basename(cfg.output_dir) == "res_inpaint_half_is4_j1x2_eta1.0_consistent_ckpt_small"
    saved = json.load(open(os.path.join(cfg.output_dir, "config.json")))
    assert saved["mask"] == "half" and saved["consistent"] is True and saved["asr_threshold"] == 0.01
    with pytest.raises(SystemExit):
        E.get_config(base + ["--asr_threshold", "0.01"])
    with pytest.raises(SystemExit):
        E.get_config(base + ["--mask", "circle"])


def test_inpaint_eval_masks():
    import inpaint_eval as E
    box, half = E.make_mask("box", 16), E.make_mask("half", 16)
    assert box.shape == half.shape == (1, 1, 16, 16)
    assert float((box == 0).float().mean()) == 0.25 and bool((box[0, 0, 4:12, 4:12] == 0).all()) and float(box.sum()) == 192
    assert bool((half[..., 8:] == 0).all()) and bool((half[..., :8] == 1).all())
