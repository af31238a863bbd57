"""CPU: the single-pass bf16 compute mode (BD_MODE_BF16) is accepted by every host-side entry point -- the enum, the plan, the
Python model constructors, the environment default and the split-plane descriptors -- without a GPU."""
import ctypes
import os
import re

import pytest

from oracle import unet_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_modes():
    src = open(os.path.join(ROOT, "include", "bd_hip.h")).read()
    body = re.search(r"enum\s+bd_compute_mode\s*\{([^}]*)\}", src).group(1)
    return {k: int(v) for k, v in re.findall(r"(BD_MODE_\w+)\s*=\s*(\d+)", body)}


def test_compute_modes_match_header_enum():
    from baddiffusion_amd.unet import COMPUTE_MODES
    modes = _header_modes()
    assert modes["BD_MODE_BF16"] == 2
    assert COMPUTE_MODES["bf16"] == modes["BD_MODE_BF16"]
    assert COMPUTE_MODES["bf16x3"] == modes["BD_MODE_BF16X3"] and COMPUTE_MODES["f32"] == modes["BD_MODE_F32"]


def test_models_construct_in_bf16_mode_on_the_host():
    from baddiffusion_amd.unet import UNet2DModel, unet_from_config
    m = unet_from_config(U.CIFAR10_32, compute_mode="bf16")
    assert m.compute_mode == "bf16"
    assert sum(v.numel() for v in m.state_dict().values()) == 35746307
    m2 = UNet2DModel(sample_size=16, block_out_channels=(128, 256), layers_per_block=1, down_block_types=("DownBlock2D", "DownBlock2D"),
                     up_block_types=("UpBlock2D", "UpBlock2D"), compute_mode="bf16")
    assert m2.compute_mode == "bf16"
    m2.set_compute_mode("bf16x3").set_compute_mode("bf16").set_compute_mode("f32")
    assert m2.compute_mode == "f32"
    with pytest.raises(ValueError):
        UNet2DModel(sample_size=16, block_out_channels=(128, 256), layers_per_block=1, down_block_types=("DownBlock2D", "DownBlock2D"),
                    up_block_types=("UpBlock2D", "UpBlock2D"), compute_mode="fp16")


def test_environment_selects_bf16_mode(monkeypatch):
    from baddiffusion_amd.unet import unet_from_config
    monkeypatch.setenv("BD_COMPUTE_MODE", "bf16")
    assert unet_from_config(U.CIFAR10_32).compute_mode == "bf16"
    monkeypatch.setenv("BD_COMPUTE_MODE", "bf16x3")
    assert unet_from_config(U.CIFAR10_32).compute_mode == "bf16x3"


def _small_cfg(lib_mod, mode):
    cfg = lib_mod.UnetConfig()
    cfg.sample_size = 32; cfg.in_channels = 3; cfg.out_channels = 3; cfg.num_blocks = 2; cfg.layers_per_block = 1
    cfg.block_out_channels[0] = 128; cfg.block_out_channels[1] = 256
    cfg.flip_sin_to_cos = 1; cfg.freq_shift = 0.0; cfg.norm_eps = 1e-5; cfg.norm_num_groups = 32
    cfg.mid_block_scale_factor = 1.0; cfg.compute_mode = mode
    return cfg


def test_c_abi_accepts_bf16_and_rejects_unknown_modes():
    from baddiffusion_amd import _lib as L
    lib = L.load()
    h = ctypes.c_void_p()
    assert lib.bd_unet_create(ctypes.byref(_small_cfg(L, 2)), ctypes.byref(h)) == 0, lib.bd_last_error()
    try:
        assert lib.bd_unet_set_compute_mode(h, 1) == 0
        assert lib.bd_unet_set_compute_mode(h, 2) == 0
        assert lib.bd_unet_set_compute_mode(h, 0) == 0
        assert lib.bd_unet_set_compute_mode(h, 3) == -1
        assert b"bd_unet_set_compute_mode" in lib.bd_last_error()
    finally:
        lib.bd_unet_destroy(h)
    h2 = ctypes.c_void_p()
    assert lib.bd_unet_create(ctypes.byref(_small_cfg(L, 3)), ctypes.byref(h2)) == -1
    assert b"compute_mode" in lib.bd_last_error()


def test_split_plane_descriptors_carry_a_mode_and_reject_unknown_values():
    """argument checks run on the host before any launch: an unknown mode is BD_ERR_INVALID with a message"""
    from baddiffusion_amd import _lib as L
    lib = L.load()
    dummy = 1 << 20           # a 128-byte aligned non-null address: never dereferenced, the mode check fails first
    d = L.GemmSpDesc(M=128, N=128, K=32, batch=1, a=dummy, lda=32, b=dummy, ldb=32, c=dummy, ldc=128, mode=3)
    assert lib.bd_gemm_sp(ctypes.byref(d), None) == -1 and b"mode" in lib.bd_last_error()
    p = L.ConvPsDesc(B=1, H=16, W=16, K=128, N=128, direction=1, x_split=dummy, ldx=128, w_split=dummy, y=dummy, ldy=128, mode=3)
    assert lib.bd_conv3x3_ps(ctypes.byref(p), None) == -1 and b"mode" in lib.bd_last_error()
    w = L.ConvPsWgradDesc(B=1, H=16, W=16, Cin=128, Cout=128, x_split=dummy, ldx=128, dy_split=dummy, lddy=128, dw=dummy, mode=7)
    assert lib.bd_conv3x3_ps_wgrad(ctypes.byref(w), None) == -1 and b"mode" in lib.bd_last_error()
    s2 = L.ConvS2DgradDesc(B=1, Ho=8, Wo=8, Cin=128, Cout=128, dy_split=dummy, lddy=128, wT_split=dummy, dx=dummy, lddx=128, mode=-1)
    assert lib.bd_conv3x3_s2_dgrad_ps(ctypes.byref(s2), None) == -1 and b"mode" in lib.bd_last_error()
    u = L.UpsampleConvDesc(B=1, H=8, W=8, Cin=128, Cout=128, x_split=dummy, ldx=128, e_split=dummy, y=dummy, ldy=128, mode=5)
    assert lib.bd_upsample_conv_fwd(ctypes.byref(u), None) == -1 and b"mode" in lib.bd_last_error()
    a = L.AttnSpDesc(B=1, heads=1, N=256, dh=256, qkv_split=dummy, ld=768, scale=1.0, o_split=dummy, ldo=256, mode=4)
    assert lib.bd_attn_sp_fwd(ctypes.byref(a), None) == -1 and b"mode" in lib.bd_last_error()
    g = L.IgemmDesc(M=64, N=64, K=64, batch_outer=1, batch_inner=1, C=dummy, ldc=64, mode=3)
    assert lib.bd_igemm(ctypes.byref(g), None) == -1 and b"compute mode" in lib.bd_last_error()
