"""GPU: the gradient with respect to the UNet input (bd_unet_backward_input, conv_in's direct data-gradient kernel, the
data-gradient-only backward schedule) and inversion.invert_trigger, against vectors the imported reference UNet2DModel computed with
autograd on its input (tests/golden/make_golden_input_grad.py -> input_grad.npz) and against the CPU oracle.
Tolerances are the project's own: 1e-3 norm-relative for whole-network gradients (BASELINE.json north_star, as test_hip_unet.py),
1e-5 / 2e-5 for the thin fp32 kernels (test_thin_convs_direct_kernels)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import loss_ref, sched_ref
from oracle import unet_ref as U
from tests.golden import cases as C
from tests.golden import cases_input_grad as CI


@pytest.fixture(scope="module")
def bd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import baddiffusion_amd.unet as unet
    import baddiffusion_amd.ops as ops
    return unet, ops


def relerr(a, b):
    a = a.detach().cpu().double(); b = torch.as_tensor(np.asarray(b)).double() if not torch.is_tensor(b) else b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def make_model(unet, cfg, seed, mode, **kw):
    m = unet.unet_from_config(cfg, **kw).cuda()
    m.load_state_dict(U.gen_params(cfg, seed))
    return m.set_compute_mode(mode)


def prof_counts():
    from baddiffusion_amd import _lib as L
    lib = L.load()
    out = {}
    for c in range(lib.bd_prof_num_classes()):
        name = ctypes.c_char_p(); n = ctypes.c_int64(); ms = ctypes.c_double(); fl = ctypes.c_double(); by = ctypes.c_double()
        L.check(lib.bd_prof_get(c, ctypes.byref(name), ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)), "bd_prof_get")
        out[name.value.decode()] = int(n.value)
    return out


class profiling:
    def __enter__(self):
        from baddiffusion_amd import _lib as L
        self.lib = L.load()
        torch.cuda.synchronize()
        self.lib.bd_prof_reset(); self.lib.bd_prof_enable(1)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.lib.bd_prof_enable(0); self.lib.bd_prof_reset()


# ---------------------------------------------------------------------------------------------------- 3. the kernel
@pytest.mark.parametrize("B,H,W,C_,Cin", [(3, 32, 32, 128, 3), (2, 8, 64, 256, 3), (1, 256, 256, 128, 3), (2, 16, 16, 128, 3), (5, 4, 12, 128, 3),
                                          (2, 32, 32, 128, 1)])
def test_conv_in_dgrad_direct_kernel(bd, B, H, W, C_, Cin):
    """conv_in's data gradient (C -> Cin, the contract direction with flipped taps; conv_thin.hip thin_contract_dgrad_kernel for
    Cin in {1, 3}, C % 128 == 0, W % 32 == 0, the implicit GEMM with a Cin-wide output otherwise) against fp64 F.conv2d autograd,
    and -- for the shapes the direct kernel claims -- its profiling class counts one launch per call."""
    _, ops = bd
    g = torch.Generator().manual_seed(B * 100 + W + Cin)
    x = torch.randn(B, H, W, Cin, generator=g)
    w_in = torch.randn(C_, 3, 3, Cin, generator=g) * 0.2          # [Cout][kh][kw][Cin]
    dy = torch.randn(B, H, W, C_, generator=g)
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    F.conv2d(xr, w_in.double().permute(0, 3, 1, 2), None, padding=1).backward(dy.double().permute(0, 3, 1, 2))
    dx_ref = xr.grad.permute(0, 2, 3, 1)
    direct = Cin in (1, 3) and C_ % 128 == 0 and W % 32 == 0
    for mode in (0, 1):
        with profiling():
            gx = ops.conv3x3_dgrad(dy.cuda(), w_in.cuda(), (B, H, W, Cin), mode=mode)
            n1 = prof_counts().get("conv_thin_dgrad_in", 0)
            gx2 = ops.conv3x3_dgrad(dy.cuda(), w_in.cuda(), (B, H, W, Cin), mode=mode)
            n2 = prof_counts().get("conv_thin_dgrad_in", 0)
        e = relerr(gx, dx_ref)
        print(f"MEASURE conv_in_dgrad {(B, H, W, C_, Cin)} mode {mode} direct {direct} {e:.3e}")
        assert e < (1e-5 if mode == 0 else 2e-5), (mode, e)
        assert torch.equal(gx, gx2)
        assert (n1, n2) == ((1, 2) if direct else (0, 0)), (direct, n1, n2)


# ---------------------------------------------------------------------------------------------------- 4. sample.grad
def train_case_dx(m, cfg, B, layout):
    """d mse(target, pred) / d x_noisy through the product; x_noisy / target from the oracle's q_sample (the fixture's inputs)"""
    _, a, ac = sched_ref.make_tables()
    x0, R, t, eps = C.train_inputs(cfg, B)
    x_noisy, target = loss_ref.q_sample(a, ac, x0, R, t, eps)
    x = x_noisy.cuda().contiguous()
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    x = x.detach().requires_grad_(True)
    pred = m(x, t.cuda(), return_dict=False)[0]
    F.mse_loss(target.cuda(), pred).backward()
    assert x.grad is not None and x.grad.shape == x.shape
    return x.grad


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("tag", ["small", "small_default", "cifar"])
def test_sample_grad_small_cases_vs_reference(bd, golden, tag, mode, layout):
    unet, _ = bd
    cfg, seed, B = CI.TRAIN_CASES[tag]
    m = make_model(unet, cfg, seed, mode)
    dx = train_case_dx(m, cfg, B, layout)
    e = relerr(dx, golden("input_grad")[f"{tag}_dx"])
    print(f"MEASURE sample_grad {tag} {mode} {layout} {e:.3e}")
    assert e < 1e-3, e


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_sample_grad_cifar_full_batch_vs_reference(bd, golden, mode):
    """batch 128: rows of both half-batch pipelines of the forward, and every sample's sum of squares"""
    unet, _ = bd
    g = golden("input_grad"); tag = "cifar128"
    cfg, seed, B = CI.TRAIN_CASES[tag]
    m = make_model(unet, cfg, seed, mode)
    dx = train_case_dx(m, cfg, B, "nchw")
    e = relerr(dx[list(C.FULL_ROWS)], g[f"{tag}_dx_rows"])
    sq = (dx.double() ** 2).sum(dim=(1, 2, 3)).cpu().numpy()
    print(f"MEASURE sample_grad {tag} {mode} rows {e:.3e} sumsq {np.abs(sq / g[f'{tag}_dx_sumsq'] - 1).max():.3e}")
    assert e < 1e-3, e
    np.testing.assert_allclose(sq, g[f"{tag}_dx_sumsq"], rtol=1e-3)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("tag", ["celeba256", "celeba256b4"])
def test_sample_grad_celeba_vs_reference(bd, golden, tag, mode):
    unet, _ = bd
    g = golden("input_grad")
    seed, stride = CI.CELEBA_CASES[tag]
    m = make_model(unet, U.CELEBA_HQ_256, seed, mode)
    x, t, dout = C.celeba_full_inputs() if tag == "celeba256" else C.celeba_b4_inputs()
    x = x.cuda().requires_grad_(True)
    m(x, t.cuda(), return_dict=False)[0].backward(dout.cuda())
    e = relerr(x.grad[:, :, ::stride, ::stride], g[f"{tag}_dx_slices"])
    sq = (x.grad.double() ** 2).sum(dim=(1, 2, 3)).cpu().numpy()
    print(f"MEASURE sample_grad {tag} {mode} slices {e:.3e} sumsq {np.abs(sq / g[f'{tag}_dx_sumsq'] - 1).max():.3e}")
    assert e < 1e-3, e
    np.testing.assert_allclose(sq, g[f"{tag}_dx_sumsq"], rtol=1e-3)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_sample_grad_through_center_input_sample(bd, mode):
    """center_input_sample=True (x -> 2x - 1 in front of the network): the gradient reaches the caller's tensor through it"""
    unet, _ = bd
    cfg = C.SMALL_CFGS["small"]
    P = U.gen_params(cfg, 7)
    m = make_model(unet, cfg, 7, mode, center_input_sample=True)
    x = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(31))
    t = torch.tensor([17, 803])
    dout = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(32))
    xr = x.clone().requires_grad_(True)
    U.unet_forward(cfg, P, 2 * xr - 1.0, t).backward(dout)
    xg = x.cuda().requires_grad_(True)
    m(xg, t.cuda(), return_dict=False)[0].backward(dout.cuda())
    e = relerr(xg.grad, xr.grad)
    print(f"MEASURE sample_grad center_input_sample {mode} {e:.3e}")
    assert e < 1e-3, e


# ---------------------------------------------------------------------------------------------------- 5. schedules agree
def _fwd_bwd(m, x, t, dout, x_grad, w_grad):
    m.flat.requires_grad_(w_grad)
    m.flat.grad = None
    xx = x.detach().clone().requires_grad_(x_grad)
    m(xx, t, return_dict=False)[0].backward(dout)
    return xx.grad, (None if m.flat.grad is None else m.flat.grad.detach().clone())


@pytest.mark.parametrize("which", ["cifar128", "celeba256b4"])
def test_schedules_agree_bit_for_bit(bd, which):
    """dx of the data-gradient-only schedule == dx of the full backward; the full backward's weight gradients are those of a pass
    without an input gradient (existing behaviour unchanged); two identical runs are bit-identical; frozen weights get no gradient"""
    unet, _ = bd
    if which == "cifar128":
        m = make_model(unet, U.CIFAR10_32, 0, "bf16x3")
        x = torch.randn(128, 3, 32, 32, generator=torch.Generator().manual_seed(3)).cuda()
        t = torch.randint(0, 1000, (128,), generator=torch.Generator().manual_seed(4)).cuda()
        dout = torch.randn(128, 3, 32, 32, generator=torch.Generator().manual_seed(5)).cuda() / (128 * 3072)
    else:
        m = make_model(unet, U.CELEBA_HQ_256, 5, "bf16x3")
        x, t, dout = (v.cuda() for v in C.celeba_b4_inputs())
    try:
        dx_frozen, g_frozen = _fwd_bwd(m, x, t, dout, True, False)
        assert g_frozen is None and m.flat.grad is None
        dx_both, g_both = _fwd_bwd(m, x, t, dout, True, True)
        none, g_w = _fwd_bwd(m, x, t, dout, False, True)
        assert none is None
        dx_both2, g_both2 = _fwd_bwd(m, x, t, dout, True, True)
        dx_frozen2, _ = _fwd_bwd(m, x, t, dout, True, False)
    finally:
        m.flat.requires_grad_(True)
    assert torch.isfinite(dx_frozen).all() and float(dx_frozen.abs().max()) > 0
    assert torch.equal(dx_frozen, dx_both)
    assert torch.equal(g_both, g_w)
    assert torch.equal(dx_both, dx_both2) and torch.equal(g_both, g_both2) and torch.equal(dx_frozen, dx_frozen2)


# ---------------------------------------------------------------------------------------------------- 6. no weight-gradient launch
def test_frozen_weights_launch_no_weight_gradient(bd):
    """structural: with the in-library profiler on, a frozen-weight forward + backward records zero launches in every class whose
    name contains `wgrad`; the same pass with trainable weights records some"""
    unet, _ = bd
    m = make_model(unet, U.CIFAR10_32, 0, "bf16x3")
    x = torch.randn(32, 3, 32, 32, generator=torch.Generator().manual_seed(3)).cuda()
    t = torch.randint(0, 1000, (32,), generator=torch.Generator().manual_seed(4)).cuda()
    dout = torch.randn(32, 3, 32, 32, generator=torch.Generator().manual_seed(5)).cuda() / (32 * 3072)
    try:
        with profiling():
            _fwd_bwd(m, x, t, dout, True, False)
            torch.cuda.synchronize()
            frozen = prof_counts()
        with profiling():
            _fwd_bwd(m, x, t, dout, True, True)
            torch.cuda.synchronize()
            train = prof_counts()
    finally:
        m.flat.requires_grad_(True)
    print("MEASURE prof frozen", frozen, "trainable", train)
    assert frozen.get("conv_thin_dgrad_in", 0) == 1 and train.get("conv_thin_dgrad_in", 0) == 1
    assert sum(n for k, n in frozen.items() if "wgrad" in k) == 0, frozen
    assert sum(n for k, n in train.items() if "wgrad" in k) > 0, train
    assert sum(n for k, n in frozen.items() if "dgrad" in k) == sum(n for k, n in train.items() if "dgrad" in k)


# ---------------------------------------------------------------------------------------------------- 7. single-pass bf16
# Measured on the MI355X (profiles/input_grad_error.json): norm-relative error of dx against the reference's,
#   cifar128 rows (FULL_ROWS):   bf16 1.130e-2, bf16x3 2.295e-5
#   celeba256b4 slices (::8):    bf16 8.154e-3, bf16x3 1.721e-5
# The bound is 3x the measured bf16 error (test_bf16_mode.py's rule); bf16 must be worse than bf16x3 on the same input.
BF16_MEASURED = {"cifar128": 1.130e-2, "celeba256b4": 8.154e-3}


@pytest.mark.parametrize("tag", ["cifar128", "celeba256b4"])
def test_sample_grad_single_pass_bf16(bd, golden, tag):
    unet, _ = bd
    g = golden("input_grad")
    res = {}
    if tag == "cifar128":
        cfg, seed, B = CI.TRAIN_CASES[tag]
        m = make_model(unet, cfg, seed, "bf16")
        for mode in ("bf16", "bf16x3"):
            m.set_compute_mode(mode)
            res[mode] = relerr(train_case_dx(m, cfg, B, "nchw")[list(C.FULL_ROWS)], g[f"{tag}_dx_rows"])
    else:
        seed, stride = CI.CELEBA_CASES[tag]
        m = make_model(unet, U.CELEBA_HQ_256, seed, "bf16")
        x, t, dout = C.celeba_b4_inputs()
        for mode in ("bf16", "bf16x3"):
            m.set_compute_mode(mode)
            m.flat.grad = None
            xx = x.cuda().requires_grad_(True)
            m(xx, t.cuda(), return_dict=False)[0].backward(dout.cuda())
            res[mode] = relerr(xx.grad[:, :, ::stride, ::stride], g[f"{tag}_dx_slices"])
    print(f"MEASURE sample_grad_bf16 {tag} bf16 {res['bf16']:.3e} bf16x3 {res['bf16x3']:.3e}")
    assert res["bf16x3"] < 1e-3, res
    assert res["bf16"] > res["bf16x3"], res
    assert res["bf16"] < 3 * BF16_MEASURED[tag], res


# ---------------------------------------------------------------------------------------------------- 8. trigger inversion
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_invert_trigger_vs_reference(bd, golden, mode):
    unet, _ = bd
    from baddiffusion_amd.inversion import invert_trigger
    g = golden("input_grad")
    cfg = C.SMALL_CFGS[CI.INV_CFG]
    m = make_model(unet, cfg, CI.INV_SEED, mode)
    sentinel = torch.full_like(m.flat.data, 0.25)
    m.flat.grad = sentinel
    tau, losses = invert_trigger(m, steps=CI.INV_STEPS, batch=CI.INV_BATCH, lam=CI.INV_LAM, timestep=CI.INV_T,
                                 noises=[n.cuda() for n in CI.inv_noises()],
                                 optimizer=lambda ps: torch.optim.SGD(ps, lr=CI.INV_LR))
    print(f"MEASURE invert_trigger {mode} losses {losses} ref {g['inv_small_losses'].tolist()} tau {relerr(tau, g['inv_small_tau']):.3e}")
    assert tau.shape == (cfg.in_channels, cfg.sample_size, cfg.sample_size) and len(losses) == CI.INV_STEPS
    np.testing.assert_allclose(losses, g["inv_small_losses"], rtol=1e-4)
    assert relerr(tau, g["inv_small_tau"]) < 1e-3
    assert all(p.requires_grad for p in m.parameters())
    assert m.flat.grad is sentinel and bool((sentinel == 0.25).all())
