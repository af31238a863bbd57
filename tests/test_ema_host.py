"""CPU: the EMA of the weights without a GPU -- the decay schedule, state-dict keys and validation messages of ema.EMAModel against
values recorded from the reference's EMAModel (tests/golden/ema_decay.json, made by tests/golden/make_golden_ema.py), the host-side
argument checks of bd_adam_clip_ema / bd_adam_clip_ema_dev / bd_ema_update, and the overlap / range check as a stand-alone program
under the host sanitizers."""
import ast
import ctypes
import json
import os
import subprocess

import pytest
import torch

from tests.golden import cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "ema_decay.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def model():
    from baddiffusion_amd.unet import unet_from_config
    return unet_from_config(C.SMALL_CFGS["small"])


def _kw(fx, name):
    return {k: ast.literal_eval(v) for k, v in fx["settings"][name].items()}


@pytest.mark.parametrize("name", ["default", "warmup_p23", "warmup_p34_g2", "after3", "min05", "warmup_p34"])
def test_decay_schedule_equals_reference(fx, model, name):
    """get_decay(k), k = 0..40 and {1 000, 31 623, 10^6}: Python-float arithmetic in the reference's order, so == with no tolerance"""
    from baddiffusion_amd.ema import EMAModel
    e = EMAModel(model, **_kw(fx, name))
    assert fx["steps"][:41] == list(range(41)) and fx["steps"][41:] == [1000, 31623, 10 ** 6]
    for k, want in zip(fx["steps"], fx["decay"][name]):
        assert e.get_decay(k) == float(want), (name, k, e.get_decay(k), want)


def test_advance_counts_and_rounds_like_step(fx, model):
    """advance(): optimization_step + 1, cur_decay_value = the schedule's value, returns fl32(1 - decay) (what torch makes of the
    Python scalar in one_minus_decay * (s - p))"""
    import numpy as np
    from baddiffusion_amd.ema import EMAModel
    e = EMAModel(model, **_kw(fx, "warmup_p34"))
    for k in range(1, 8):
        omd = e.advance()
        want = float(fx["decay"]["warmup_p34"][k])
        assert e.optimization_step == k and e.cur_decay_value == want
        assert omd == float(np.float32(1 - want)) and 0.0 <= omd <= 1.0


def test_state_dict_keys_and_validation_messages(fx, model):
    from baddiffusion_amd.ema import EMAModel
    e = EMAModel(model, decay=0.99, min_decay=0.25, update_after_step=2, use_ema_warmup=True, inv_gamma=3, power=0.5)
    sd = e.state_dict()
    assert list(sd.keys()) == fx["state_dict_keys"]
    assert sd["shadow_params"] is e.shadow and torch.equal(e.shadow, model.flat.detach()) and e.shadow.data_ptr() != model.flat.data_ptr()
    for key in ("decay", "min_decay", "inv_gamma", "power"):
        bad = {k: ast.literal_eval(v) for k, v in fx["errors"][key]["state"].items()}
        with pytest.raises(ValueError) as err:
            EMAModel(model).load_state_dict(bad)
        assert str(err.value) == fx["errors"][key]["message"], key
    with pytest.raises(RuntimeError) as err:
        EMAModel(model).restore(model)
    assert str(err.value) == fx["errors"]["restore"]["message"]
    # a round trip: scalars and shadow arrive, the shadow IN PLACE (an engine holds its address)
    e.optimization_step = 5
    e.shadow.add_(1.0)
    e2 = EMAModel(model)
    ptr = e2.shadow.data_ptr()
    e2.load_state_dict(e.state_dict())
    assert {k: v for k, v in e2.state_dict().items() if k != "shadow_params"} == {k: v for k, v in e.state_dict().items() if k != "shadow_params"}
    assert e2.optimization_step == 5 and torch.equal(e2.shadow, e.shadow) and e2.shadow.data_ptr() == ptr
    with pytest.raises(ValueError):
        e2.load_state_dict({"shadow_params": torch.zeros(3)})


def test_averaged_state_dict_goes_through_the_offset_table(model):
    from baddiffusion_amd.ema import EMAModel
    e = EMAModel(model)
    e.shadow.copy_(torch.arange(e.shadow.numel(), dtype=torch.float32))
    avg, own = e.averaged_state_dict(model), model.state_dict()
    assert list(avg.keys()) == list(own.keys())
    for k in own:
        assert avg[k].shape == own[k].shape
    saved = model.flat.detach().clone()
    model.load_state_dict(avg)
    try:       # loading the averaged dict writes exactly the shadow's tensor elements (pads are not part of any tensor)
        mask = torch.ones(model.num_flat, dtype=torch.bool)
        for lo, hi in model._pads:
            mask[lo:hi] = False
        assert torch.equal(model.flat.detach()[mask], e.shadow[mask])
    finally:
        model.flat.data.copy_(saved)


# ---- argument checks of the three entry points: on the host, before any launch ---------------------------------------------------
def _bufs(n=16):
    arr = (ctypes.c_float * (6 * n))()
    base = ctypes.addressof(arr)
    return arr, [base + 4 * n * k for k in range(6)]       # p, g, m, v, ema, (spare)


def test_entry_points_reject_bad_arguments_without_gpu():
    from baddiffusion_amd import _lib as L
    lib = L.load()
    n = 16
    keep, (p, g, m, v, ema, _) = _bufs(n)
    ss = ctypes.c_double(1.0); ssp = ctypes.addressof(ss)
    hyper = (ctypes.c_float * 3)(); hp = ctypes.addressof(hyper)

    def fused(p=p, g=g, m=m, v=v, ema=ema, n=n, omd=0.5, ssp=ssp, step=1):
        return lib.bd_adam_clip_ema(p, g, m, v, ema, n, ssp, 1.0, 2e-4, 0.9, 0.999, 1e-8, step, omd, None, None)

    def dev(p=p, g=g, m=m, v=v, ema=ema, n=n, hp=hp, ssp=ssp):
        return lib.bd_adam_clip_ema_dev(p, g, m, v, ema, n, ssp, 1.0, hp, 0.9, 0.999, 1e-8, None, None)

    def alone(ema=ema, p=p, n=n, omd=0.5):
        return lib.bd_ema_update(ema, p, n, omd, None)

    def rejected(status, name):
        return status < 0 and name in lib.bd_last_error()

    # null pointers, n <= 0
    for kw in ({"p": None}, {"g": None}, {"m": None}, {"v": None}, {"ema": None}, {"ssp": None}, {"n": 0}, {"n": -3}):
        assert rejected(fused(**kw), b"bd_adam_clip_ema:"), kw
        assert rejected(dev(**kw), b"bd_adam_clip_ema_dev:"), kw
    assert rejected(dev(hp=None), b"bd_adam_clip_ema_dev:")
    assert rejected(fused(step=0), b"bd_adam_clip_ema:")
    for kw in ({"ema": None}, {"p": None}, {"n": 0}):
        assert rejected(alone(**kw), b"bd_ema_update:"), kw
    # one_minus_decay outside [0, 1] or not a number
    for omd in (-0.1, 1.5, float("nan"), float("inf")):
        assert rejected(fused(omd=omd), b"bd_adam_clip_ema:") and b"one_minus_decay" in lib.bd_last_error(), omd
        assert rejected(alone(omd=omd), b"bd_ema_update:") and b"one_minus_decay" in lib.bd_last_error(), omd
    # the shadow overlapping p, m, v or g as a range of n floats: equal, shifted by one float, sharing only the last element
    for other in (p, g, m, v):
        for shift in (0, 4, 4 * (n - 1), -4 * (n - 1)):
            assert rejected(fused(ema=other + shift), b"bd_adam_clip_ema:") and b"overlaps" in lib.bd_last_error(), (other, shift)
    for shift in (0, 4, 4 * (n - 1), -4 * (n - 1)):
        assert rejected(alone(ema=p + shift), b"bd_ema_update:") and b"overlaps" in lib.bd_last_error(), shift
    del keep


def test_overlap_and_range_check_under_host_sanitizers(tmp_path):
    """csrc/ema_check.h (the host function behind the checks above) with its own main, built with -fsanitize=address,undefined and
    run as a stand-alone program: no python, no GPU; the sanitizer runtimes are linked statically, so nothing has to be preloaded"""
    csrc = os.path.join(ROOT, "baddiffusion_amd", "csrc")
    exe = str(tmp_path / "ema_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", csrc, os.path.join(csrc, "ema_check_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ema_check: ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


# ---- command line: flags, persistence, which weights a later command reads --------------------------------------------------------
def test_cli_flags_persist_and_choose_the_weights(tmp_path):
    """--use_ema / --ema_inv_gamma / --ema_power / --ema_max_decay (diffusers' train_unconditional.py names and defaults) reach the config,
    are written to args.json so that --mode resume finds them, and --mode sampling | measure read the averaged weights only when asked"""
    import baddiffusion as cli
    base = ["--dataset", "CIFAR10", "--batch", "128", "--epoch", "1", "--ckpt", "DDPM-CIFAR10-32", "--result", str(tmp_path), "-o"]
    plain = cli.setup(["--mode", "train", "--postfix", "plain"] + base)
    assert plain.use_ema is False and (plain.ema_inv_gamma, plain.ema_power, plain.ema_max_decay) == (1.0, 0.75, 0.9999)
    assert cli.make_ema(plain, None) is None
    cfg = cli.setup(["--mode", "train", "--use_ema", "--ema_power", "0.6", "--ema_max_decay", "0.999", "--ema_inv_gamma", "2.0"] + base)
    assert cfg.use_ema is True and (cfg.ema_inv_gamma, cfg.ema_power, cfg.ema_max_decay) == (2.0, 0.6, 0.999)
    saved = json.load(open(os.path.join(cfg.output_dir, "args.json")))
    assert saved["use_ema"] is True and saved["ema_power"] == 0.6 and saved["ema_max_decay"] == 0.999 and saved["ema_inv_gamma"] == 2.0
    assert json.load(open(os.path.join(cfg.output_dir, "config.json")))["use_ema"] is True
    res = cli.setup(["--mode", "resume", "--ckpt", cfg.output_dir], write=False)
    assert res.use_ema is True and (res.ema_inv_gamma, res.ema_power, res.ema_max_decay) == (2.0, 0.6, 0.999)
    for mode in ("sampling", "measure"):
        assert cli.setup(["--mode", mode, "--ckpt", cfg.output_dir], write=False).use_ema is False
        assert cli.setup(["--mode", mode, "--ckpt", cfg.output_dir, "--use_ema"], write=False).use_ema is True
    with pytest.raises(NotImplementedError):       # resume takes its options from args.json, like every other training option
        cli.setup(["--mode", "resume", "--ckpt", cfg.output_dir, "--use_ema"], write=False)
    assert cli.setup(["--mode", "resume", "--ckpt", plain.output_dir], write=False).use_ema is False


def test_cli_make_ema_matches_the_reference_script(fx, model):
    """make_ema: use_ema_warmup=True with the flags' values (train_unconditional.py:465-473); the default flags give the recorded schedule"""
    import baddiffusion as cli
    cfg = cli.TrainingConfig()
    cfg.use_ema = True
    e = cli.make_ema(cfg, model)
    assert (e.decay, e.use_ema_warmup, e.inv_gamma, e.power, e.min_decay, e.update_after_step) == (0.9999, True, 1.0, 0.75, 0.0, 0)
    assert [e.get_decay(k) for k in fx["steps"]] == [float(x) for x in fx["decay"]["warmup_p34"]]


def test_to_keeps_the_shadow_fp32_and_in_place(model):
    """to(): another dtype is refused (the kernels read fp32 only); the shadow's own device moves nothing, so an address handed to an
    engine stays valid; a real move is refused once an engine is attached"""
    from baddiffusion_amd.ema import EMAModel
    e = EMAModel(model)
    ptr = e.shadow.data_ptr()
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(TypeError):
            e.to(dtype=dt)
    e.to("cpu"); e.to(torch.device("cpu"), dtype=torch.float32); e.to()
    assert e.shadow.data_ptr() == ptr and e.shadow.dtype == torch.float32
    e.attached = True
    e.to("cpu")                                   # same device: still nothing to do
    with pytest.raises(RuntimeError, match="TrainEngine"):
        e.to("meta")
    assert e.shadow.data_ptr() == ptr
    e.attached = False
    e.store(model)
    e.to("meta")
    assert e.shadow.device.type == "meta" and e.temp_stored_params.device.type == "meta"
