"""CPU: the input-gradient fixtures (tests/golden/input_grad.npz, computed by the imported reference UNet2DModel with autograd on its
input) against the oracle's own autograd, and the host-side contract of bd_unet_backward_input (declared, exported, argument checks
that run before any device call)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import loss_ref, sched_ref
from oracle import unet_ref as U
from tests.golden import cases as C
from tests.golden import cases_input_grad as CI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def relerr(a, b):
    a = torch.as_tensor(np.asarray(a)).double(); b = torch.as_tensor(np.asarray(b)).double()
    return float((a - b).norm() / b.norm())


def oracle_train_dx(cfg, seed, B):
    P = U.gen_params(cfg, seed)
    _, a, ac = sched_ref.make_tables()
    x0, R, t, eps = C.train_inputs(cfg, B)
    x_noisy, target = loss_ref.q_sample(a, ac, x0, R, t, eps)
    x_noisy = x_noisy.detach().contiguous().requires_grad_(True)
    F.mse_loss(target, U.unet_forward(cfg, P, x_noisy, t)).backward()
    return x_noisy.grad


@pytest.mark.parametrize("tag", list(CI.TRAIN_CASES))
def test_oracle_dx_train_cases_vs_reference(golden, tag):
    """d mse(target, pred) / d x_noisy by the oracle's autograd against the reference's: 1e-4 norm-relative, the bound
    test_oracle_golden.py puts on whole-network gradient vectors."""
    g = golden("input_grad")
    cfg, seed, B = CI.TRAIN_CASES[tag]
    dx = oracle_train_dx(cfg, seed, B)
    if tag == "cifar128":
        assert relerr(dx[list(C.FULL_ROWS)], g[f"{tag}_dx_rows"]) < 1e-4
        sq = (dx.double() ** 2).sum(dim=(1, 2, 3)).numpy()
        np.testing.assert_allclose(sq, g[f"{tag}_dx_sumsq"], rtol=1e-4)
        np.testing.assert_allclose(dx.double().sum(dim=(1, 2, 3)).numpy(), g[f"{tag}_dx_sum"], rtol=0,
                                   atol=1e-4 * float(np.sqrt(g[f"{tag}_dx_sumsq"].max() * dx[0].numel())))
    else:
        assert relerr(dx, g[f"{tag}_dx"]) < 1e-4


@pytest.mark.parametrize("tag", list(CI.CELEBA_CASES))
def test_oracle_dx_celeba_vs_reference(golden, tag):
    g = golden("input_grad")
    seed, stride = CI.CELEBA_CASES[tag]
    cfg = U.CELEBA_HQ_256
    P = U.gen_params(cfg, seed)
    x, t, dout = C.celeba_full_inputs() if tag == "celeba256" else C.celeba_b4_inputs()
    x = x.clone().requires_grad_(True)
    U.unet_forward(cfg, P, x, t).backward(dout)
    dx = x.grad
    assert relerr(dx[:, :, ::stride, ::stride], g[f"{tag}_dx_slices"]) < 1e-4
    np.testing.assert_allclose((dx.double() ** 2).sum(dim=(1, 2, 3)).numpy(), g[f"{tag}_dx_sumsq"], rtol=1e-4)
    np.testing.assert_allclose(dx.double().sum(dim=(1, 2, 3)).numpy(), g[f"{tag}_dx_sum"], rtol=0,
                               atol=1e-4 * float(np.sqrt(g[f"{tag}_dx_sumsq"].max() * dx[0].numel())))


def test_oracle_inversion_loop_vs_reference(golden):
    """invert_trigger's loop written out on the oracle: losses 1e-5 relative, final tau 1e-4 norm-relative."""
    g = golden("input_grad")
    cfg = C.SMALL_CFGS[CI.INV_CFG]
    P = U.gen_params(cfg, CI.INV_SEED)
    tau = torch.zeros(cfg.in_channels, cfg.sample_size, cfg.sample_size, requires_grad=True)
    opt = torch.optim.SGD([tau], lr=CI.INV_LR)
    losses = []
    for x in CI.inv_noises():
        T = torch.full((x.shape[0],), CI.INV_T, dtype=torch.int64)
        eps = U.unet_forward(cfg, P, x + tau, T)
        loss = ((eps.mean(0) - CI.INV_LAM * tau) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    np.testing.assert_allclose(losses, g["inv_small_losses"], rtol=1e-5)
    assert relerr(tau.detach(), g["inv_small_tau"]) < 1e-4
    assert float(np.linalg.norm(g["inv_small_tau"])) > 0.5        # steps 2 and 3 really depend on tau


def test_backward_input_declared_and_exported():
    from baddiffusion_amd.build import build_lib
    from baddiffusion_amd import _lib as L
    lib_path = build_lib(force=False, verbose=False)
    src = open(os.path.join(ROOT, "include", "bd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bbd_unet_backward_input\s*\(", src)
    exported = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True).stdout
    assert " T bd_unet_backward_input" in exported
    assert "bd_unet_backward_input" in L.SIGNATURES


def test_backward_input_rejects_bad_arguments_without_gpu():
    """host-only plan: the checks run before any device call -- BD_ERR_INVALID (-1) with a bd_last_error text"""
    from baddiffusion_amd import _lib as L
    from baddiffusion_amd.unet import unet_from_config
    lib = L.load()
    m = unet_from_config(C.SMALL_CFGS["small"])          # CPU module: the plan is a host object
    cin = m.config.in_channels
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)      # 16-byte aligned dummy, never dereferenced
    args = lambda dx, lddx, params=p: (m._plan, 2, params, p, cin, p, m.config.out_channels, None, dx, lddx, None, 0, None)
    assert lib.bd_unet_backward_input(*args(None, cin)) == -1
    assert b"bd_unet_backward_input" in lib.bd_last_error() and b"dx" in lib.bd_last_error()
    assert lib.bd_unet_backward_input(*args(p, cin - 1)) == -1
    assert b"lddx" in lib.bd_last_error()
    assert lib.bd_unet_backward_input(*args(p, cin, ctypes.c_void_p(p.value + 4))) == -1
    assert b"aligned" in lib.bd_last_error()
    assert lib.bd_unet_backward_input(None, 2, p, p, cin, p, 3, None, p, cin, None, 0, None) == -1
