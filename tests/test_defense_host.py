"""CPU: the host-side contract of the detection kernels (bd_pairwise_sqdist, bd_total_variation: argument checks that run before any
launch), the device-only rule of the new metrics, detect_backdoor's threshold and elijah_defense.get_config."""
import ctypes
import json
import os

import pytest
import torch


def _dummy():
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16       # 16-byte aligned, never dereferenced
    return buf, ctypes.c_void_p(p)


def test_pairwise_sqdist_rejects_bad_arguments_without_gpu():
    from baddiffusion_amd import _lib as L
    lib = L.load()
    buf, p = _dummy()
    ok = dict(x=p, ldx=192, N=8, D=192, d2=p, ldd=8, ws=None, wsb=0)

    def call(**kw):
        a = {**ok, **kw}
        return lib.bd_pairwise_sqdist(a["x"], a["ldx"], a["N"], a["D"], a["d2"], a["ldd"], a["ws"], a["wsb"], None)
    for kw, word in (({"x": None}, b"null"), ({"d2": None}, b"null"), ({"ldx": 191}, b"ldx"), ({"ldd": 7}, b"ldd"), ({"N": 0}, b"N="),
                     ({"D": 0}, b"D="), ({"x": ctypes.c_void_p(p.value + 2)}, b"aligned")):
        assert call(**kw) < 0, kw
        err = lib.bd_last_error()
        assert b"bd_pairwise_sqdist" in err and word in err, (kw, err)
    # a shape whose D is split over workgroups needs a workspace: missing or short is an error of its own
    N, D = 8, 196608
    need = lib.bd_pairwise_sqdist_workspace_bytes(N, D)
    assert need > 0
    for ws, wsb in ((None, need), (p, need - 1), (p, 0)):
        assert lib.bd_pairwise_sqdist(p, D, N, D, p, N, ws, wsb, None) == -4          # BD_ERR_WORKSPACE
        err = lib.bd_last_error()
        assert b"bd_pairwise_sqdist" in err and b"workspace" in err, err


def test_pairwise_sqdist_workspace_is_monotone_in_d():
    from baddiffusion_amd import _lib as L
    lib = L.load()
    assert lib.bd_pairwise_sqdist_workspace_bytes(0, 16) == 0 and lib.bd_pairwise_sqdist_workspace_bytes(16, 0) == 0
    for N in (1, 8, 64, 65, 256):
        sizes = [lib.bd_pairwise_sqdist_workspace_bytes(N, D) for D in
                 (1, 31, 32, 255, 256, 511, 512, 513, 3072, 3073, 12288, 49152, 196607, 196608, 196609, 786432, 1 << 24)]
        assert sizes == sorted(sizes), (N, sizes)
        assert sizes[0] == 0 and sizes[-1] > 0, (N, sizes)
        assert all(s % (64 * 64 * 4) == 0 for s in sizes), (N, sizes)      # whole 64 x 64 fp32 tiles


def test_total_variation_rejects_bad_arguments_without_gpu():
    from baddiffusion_amd import _lib as L
    lib = L.load()
    buf, p = _dummy()
    for args in ((None, 1, 3, 8, 8, 192, 64, 8, 1, p), (p, 1, 3, 8, 8, 192, 64, 8, 1, None), (p, 0, 3, 8, 8, 192, 64, 8, 1, p),
                 (p, 1, 3, 0, 8, 192, 64, 8, 1, p), (p, 1, 3, 8, 0, 192, 64, 8, 1, p), (p, 1, 1 << 11, 1 << 10, 1 << 10, 1, 1, 1, 1, p)):
        assert lib.bd_total_variation(*args, None) < 0, args
        assert b"bd_total_variation" in lib.bd_last_error()


def test_new_metrics_are_device_only():
    from baddiffusion_amd import metrics
    x = torch.rand(4, 3, 8, 8)
    for fn in (metrics.pairwise_sqdist, metrics.uniformity, metrics.total_variation):
        with pytest.raises(RuntimeError, match="device tensors required"):
            fn(x)
    with pytest.raises(ValueError, match="at least two"):
        metrics.uniformity(x[:1])
    with pytest.raises(ValueError, match="at least two"):
        metrics.uniformity(x[:0])


def test_detect_backdoor_requires_max_ratio():
    from baddiffusion_amd.defense import detect_backdoor
    with pytest.raises(TypeError):
        detect_backdoor({"uniformity_ratio": 0.01})
    with pytest.raises(TypeError):
        detect_backdoor({"uniformity_ratio": 0.01}, 0.5)                   # keyword-only: no positional threshold either
    assert detect_backdoor({"uniformity_ratio": 0.01}, max_ratio=0.5) is True
    assert detect_backdoor({"uniformity_ratio": 0.5}, max_ratio=0.5) is False
    assert detect_backdoor({"uniformity_ratio": 0.9}, max_ratio=0.5) is False


def test_elijah_get_config_names_the_output_directory(tmp_path):
    import elijah_defense as E
    ckpt = tmp_path / "ckpts" / "res_DDPM-CIFAR10-32_CIFAR10_ep50_c1.0_p0.1_BOX_14-HAT"
    ckpt.mkdir(parents=True)
    cfg = E.get_config(["--ckpt", str(ckpt) + "/", "--output_dir", str(tmp_path / "out"), "--inv_steps", "7", "--lam", "0.25",
                        "--remove_steps", "3", "--learning_rate", "1e-05", "--tag", "t1", "--detect_n", "32", "--sched", "DDPM-SCHED",
                        "--infer_steps", "9", "--inv_batch", "5", "--inv_lr", "0.2", "--batch", "6", "--seed", "4", "--gpu", "0"])
    name = "res_elijah_inv7_lam0.25_rm3_lr1e-05_t1_res_DDPM-CIFAR10-32_CIFAR10_ep50_c1.0_p0.1_BOX_14-HAT"
    assert cfg.output_dir == os.path.join(str(tmp_path / "out"), name)
    saved = json.load(open(os.path.join(cfg.output_dir, "config.json")))
    assert saved["inv_steps"] == 7 and saved["lam"] == 0.25 and saved["remove_steps"] == 3 and saved["learning_rate"] == 1e-5
    assert saved["detect_n"] == 32 and saved["sched"] == "DDPM-SCHED" and saved["infer_steps"] == 9 and saved["max_ratio"] is None
    assert saved["inv_batch"] == 5 and saved["inv_lr"] == 0.2 and saved["batch"] == 6 and saved["seed"] == 4 and saved["tag"] == "t1"
    assert saved["output_dir"] == cfg.output_dir and saved["ckpt"] == str(ckpt) + "/"
    cfg2 = E.get_config(["--ckpt", str(ckpt), "--output_dir", str(tmp_path / "out"), "--max_ratio", "0.4"])
    assert os.path.basename(cfg2.output_dir) == "res_elijah_inv100_lam0.5_rm200_lr2e-05_" + ckpt.name
    assert cfg2.max_ratio == 0.4 and cfg2.sched == "DDIM-SCHED"
    with pytest.raises(SystemExit):
        E.get_config(["--ckpt", str(ckpt), "--sched", "PNDM-SCHED"])
