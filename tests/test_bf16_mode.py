"""GPU: the single-pass bf16 compute mode (BD_MODE_BF16, include/bd_hip.h): every matrix product rounds its operands once to bf16 (RNE, the hi
plane of the split mode) and issues ONE v_mfma_f32_32x32x16_bf16 per product with fp32 accumulation; everything else stays fp32.

Each kernel family is checked against an fp64 contraction of the bf16-rounded operands (torch's .to(torch.bfloat16) rounds to nearest even):
the single-pass result sits at the fp32-accumulation level from it, while the three-product result of the same inputs lands at least 10x further
away -- which shows that the single-pass instantiation really ran.  The whole network is then checked against the goldens (G10, G12, G14) with
bounds set from measurement, and for schedule independence, determinism and clean mode switches."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import sched_ref
from oracle import unet_ref as U
from tests.golden import cases as C

F32, BF16X3, BF16 = 0, 1, 2


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from baddiffusion_amd import ops as o
    return o


def relerr(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rnd(x):
    """bf16 RNE of x, as fp64"""
    return x.to(torch.bfloat16).double()


def planes_to_f32(p):
    """split planes [rows, C/32, 2, 32] int16 -> fp32 [rows, C] (hi + lo)"""
    b = p.view(torch.bfloat16).float()
    return (b[:, :, 0, :] + b[:, :, 1, :]).reshape(p.shape[0], -1)


def conv_refs(x, w, dy, stride=1, pad=1, asym=False, ups=False):
    """fp64 forward / data gradient / weight gradient of conv3x3 (NHWC, w [Cout,3,3,Cin]) on bf16-rounded operands; bias gradient of the
    UNROUNDED dy (the bias gradients keep fp32-grade sums in every mode)"""
    xr = rnd(x).permute(0, 3, 1, 2).requires_grad_(True)
    wr = rnd(w).permute(0, 3, 1, 2).requires_grad_(True)
    xin = F.interpolate(xr, scale_factor=2.0, mode="nearest") if ups else xr
    if asym:
        xin = F.pad(xin, (0, 1, 0, 1))
    y = F.conv2d(xin, wr, None, stride=stride, padding=0 if asym else pad)
    y.backward(rnd(dy).permute(0, 3, 1, 2))
    return (y.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), wr.grad.permute(0, 2, 3, 1),
            dy.double().sum(dim=(0, 1, 2)))


def _pair(name, got1, got3, ref, bound):
    """single pass at the accumulation level; three products >= 10x further from the rounded reference"""
    e1, e3 = relerr(got1, ref), relerr(got3, ref)
    print(f"MEASURE {name} bf16 {e1:.3e} bf16x3 {e3:.3e}")
    assert e1 < bound, (name, e1)
    assert e3 > 10 * e1, (name, e1, e3)


# Single-pass error against the rounded fp64 reference, measured on MI355X: 4e-8 - 1.9e-7 for every convolution / GEMM family (bf16x3 on the same
# inputs: 1.5e-3 - 2.4e-3), attn_sp 4.2e-6 (it also rounds P; bf16x3 3.2e-3).  Held to 3x the largest.
TOL = 6e-7
TOL_ATTN = 1.3e-5    # forward.  The backward (tests/test_attn_sp_exact.py, held to 3x there): dS^T 2.8e-6, dv 2.4e-6, dq 3.8e-5, dk 3.8e-5 -- dq / dk contract the rounded dS
TOL_BIAS = 7.5e-6    # bias gradients keep fp32-grade sums (hi + lo of dY, or fp32 column sums) against the UNROUNDED fp64 sum: measured <= 2.5e-6


def _bias(name, got, ref):
    e = relerr(got, ref)
    print(f"MEASURE {name} {e:.3e}")
    assert e < TOL_BIAS, (name, e)


@pytest.mark.parametrize("B,S,Cin,Cout", [(2, 8, 96, 160), (4, 16, 128, 128)])
def test_igemm_conv_against_rounded_operands(ops, B, S, Cin, Cout):
    """the igemm split path (launch_tile<..., true>) in its single-pass instantiation: conv forward (on the fly and from pre-split weights,
    presplit_ok), data gradient, weight gradient + fused bias gradient"""
    g = torch.Generator().manual_seed(B * 100 + S)
    x = torch.randn(B, S, S, Cin, generator=g).cuda(); dy = torch.randn(B, S, S, Cout, generator=g).cuda()
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) * 0.05).cuda(); bias = torch.randn(Cout, generator=g).cuda()
    y_ref, dx_ref, dw_ref, db_ref = conv_refs(x.cpu(), w.cpu(), dy.cpu())
    y_ref = y_ref + bias.cpu().double()
    _pair("igemm_fwd", ops.conv3x3_fwd(x, w, bias, mode=BF16), ops.conv3x3_fwd(x, w, bias, mode=BF16X3), y_ref, TOL)
    if Cin % 32 == 0:
        ws = ops.split_bf16(w)
        _pair("igemm_fwd_presplit", ops.conv3x3_fwd(x, w, bias, mode=BF16, w_split=ws), ops.conv3x3_fwd(x, w, bias, mode=BF16X3, w_split=ws), y_ref, TOL)
    _pair("igemm_dgrad", ops.conv3x3_dgrad(dy, w, (B, S, S, Cin), mode=BF16), ops.conv3x3_dgrad(dy, w, (B, S, S, Cin), mode=BF16X3), dx_ref, TOL)
    dw1, db1 = ops.conv3x3_wgrad(x, dy, mode=BF16, with_db=True)
    dw3, _ = ops.conv3x3_wgrad(x, dy, mode=BF16X3, with_db=True)
    _pair("igemm_wgrad", dw1, dw3, dw_ref, TOL)
    _bias("igemm_db", db1, db_ref)


def test_igemm_gemm_against_rounded_operands(ops):
    """dense GEMMs (the 1x1 shortcuts, linear layers, unfused attention) through the same kernels, with the fused column sum"""
    g = torch.Generator().manual_seed(11)
    a = torch.randn(384, 512, generator=g).cuda(); b = torch.randn(320, 512, generator=g).cuda()
    ref = rnd(a.cpu()) @ rnd(b.cpu()).T
    _pair("igemm_gemm_nt", ops.gemm(a, b, mode=BF16), ops.gemm(a, b, mode=BF16X3), ref, TOL)
    at = a.T.contiguous()
    _pair("igemm_gemm_tn", ops.gemm(at, b, trans_a=True, mode=BF16), ops.gemm(at, b, trans_a=True, mode=BF16X3), ref, TOL)


@pytest.mark.parametrize("B,S,Cin,Cout", [(3, 8, 256, 128), (48, 16, 128, 256), (16, 32, 128, 128)])
def test_conv_ps_family_against_rounded_operands(ops, B, S, Cin, Cout):
    """bd_conv3x3_ps (+1 / -1) and bd_conv3x3_ps_wgrad (wgrad / wgrad3 by shape).  At 256 CUs the three shapes reach conv_ps128 in its four-stage
    split form (3 x 8 x 8, both directions), conv_ps3 (48 x 16 x 16 forward; its data gradient is conv_ps128, two stages) and conv_ps128 in its
    two-stage split form (16 x 32 x 32) -- not the general 256 x 128 kernel (conv_ps_kernel), which tests/test_conv_ps_dispatch.py covers
    together with the other branches these shapes miss."""
    g = torch.Generator().manual_seed(B * 1000 + S)
    x = torch.randn(B, S, S, Cin, generator=g).cuda(); dy = torch.randn(B, S, S, Cout, generator=g).cuda()
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) * 0.05).cuda(); bias = torch.randn(Cout, generator=g).cuda()
    y_ref, dx_ref, dw_ref, db_ref = conv_refs(x, w, dy)
    y_ref = y_ref + bias.double()
    xs, dys, ws, wts = ops.split_rows(x), ops.split_rows(dy), ops.split_bf16(w), ops.split_wT(w)
    run = lambda m: ops.conv3x3_ps(xs, ws, B, S, S, Cin, Cout, 1, bias=bias, mode=m)
    _pair(f"conv_ps_fwd_{B}x{S}", run(BF16), run(BF16X3), y_ref, TOL)
    run = lambda m: ops.conv3x3_ps(dys, wts, B, S, S, Cout, Cin, -1, mode=m)
    _pair(f"conv_ps_dgrad_{B}x{S}", run(BF16), run(BF16X3), dx_ref, TOL)
    dw1, db1 = ops.conv3x3_ps_wgrad(xs, dys, B, S, S, Cin, Cout, with_db=True, mode=BF16)
    dw3, db3 = ops.conv3x3_ps_wgrad(xs, dys, B, S, S, Cin, Cout, with_db=True, mode=BF16X3)
    _pair(f"conv_ps_wgrad_{B}x{S}", dw1, dw3, dw_ref, TOL)
    _bias(f"conv_ps_db_{B}x{S}", db1, db_ref)                             # bias gradient: hi + lo of dY in both modes
    assert relerr(db1, db3) < TOL_BIAS
    dw1b = ops.conv3x3_ps_wgrad(xs, dys, B, S, S, Cin, Cout, mode=BF16)
    assert torch.equal(dw1, dw1b)


@pytest.mark.parametrize("B,H,W,C_", [(4, 8, 8, 128), (16, 16, 16, 128)])
def test_conv_phase_family_against_rounded_operands(ops, B, H, W, C_):
    """conv_ph.hip: the upsample convolution (forward, data gradient; the PHASE weight gradient in conv_ps.hip) and the stride-2 data gradient.
    The phase forms multiply SUMS of weight taps, so the weights here are multiples of 2^-6 below 8 in magnitude: every sum of up to four taps
    is exact in bf16 and the only rounded operand is the activation / gradient, as in the literal form."""
    g = torch.Generator().manual_seed(B + H)
    x = torch.randn(B, H, W, C_, generator=g).cuda(); dy = torch.randn(B, 2 * H, 2 * W, C_, generator=g).cuda()
    w = (torch.randint(-8, 9, (C_, 3, 3, C_), generator=g).float() / 64).cuda(); bias = torch.randn(C_, generator=g).cuda()
    y_ref, dx_ref, dw_ref, db_ref = conv_refs(x, w, dy, ups=True)
    y_ref = y_ref + bias.double()
    xs, dys = ops.split_rows(x), ops.split_rows(dy)
    e, et = ops.upsample_weights(w)
    run = lambda m: ops.upsample_conv_fwd(xs, e, B, H, W, C_, C_, bias=bias, mode=m)
    _pair("ph_ups_fwd", run(BF16), run(BF16X3), y_ref, TOL)
    run = lambda m: ops.upsample_conv_dgrad(dys, et, B, H, W, C_, C_, mode=m)
    _pair("ph_ups_dgrad", run(BF16), run(BF16X3), dx_ref, TOL)
    dw1, db1 = ops.upsample_conv_wgrad(xs, dys, B, H, W, C_, C_, with_db=True, mode=BF16)
    dw3, _ = ops.upsample_conv_wgrad(xs, dys, B, H, W, C_, C_, with_db=True, mode=BF16X3)
    _pair("ph_ups_wgrad", dw1, dw3, dw_ref, TOL)
    _bias("ph_ups_db", db1, db_ref)
    # stride-2 data gradient (Downsample2D), both paddings
    xf = torch.randn(B, 2 * H, 2 * W, C_, generator=g).cuda(); dyc = torch.randn(B, H, W, C_, generator=g).cuda()
    wf = (torch.randn(C_, 3, 3, C_, generator=g) * 0.05).cuda()
    dys2, wt = ops.split_rows(dyc), ops.split_wT(wf)
    for pad in (0, 1):
        _, dx2_ref, _, _ = conv_refs(xf, wf, dyc, stride=2, pad=pad, asym=(pad == 0))
        run = lambda m: ops.conv3x3_s2_dgrad_ps(dys2, wt, B, H, W, C_, C_, pad=pad, mode=m)
        _pair(f"ph_s2_dgrad_pad{pad}", run(BF16), run(BF16X3), dx2_ref, TOL)


@pytest.mark.parametrize("akm,bkm", [(False, False), (False, True), (True, True)])
def test_gemm_sp_against_rounded_operands(ops, akm, bkm):
    g = torch.Generator().manual_seed(7 + 2 * akm + bkm)
    M, N, K = 256, 384, 512
    a = torch.randn(M, K, generator=g).cuda(); b = torch.randn(N, K, generator=g).cuda()
    a_s = ops.split_rows(a.T.contiguous() if akm else a); b_s = ops.split_rows(b.T.contiguous() if bkm else b)
    ref = rnd(a) @ rnd(b).T
    kw = dict(a_kmajor=akm, b_kmajor=bkm)
    if akm and bkm:
        c1, _, cs1 = ops.gemm_sp(a_s, b_s, M, N, K, want_colsum=True, mode=BF16, **kw)
        c3, _, _ = ops.gemm_sp(a_s, b_s, M, N, K, want_colsum=True, mode=BF16X3, **kw)
        _bias("gemm_sp_colsum", cs1, a.double().sum(dim=1))     # column sums keep hi + lo
    else:
        c1, _ = ops.gemm_sp(a_s, b_s, M, N, K, mode=BF16, **kw)
        c3, _ = ops.gemm_sp(a_s, b_s, M, N, K, mode=BF16X3, **kw)
    _pair(f"gemm_sp_{int(akm)}{int(bkm)}", c1[0], c3[0], ref, TOL)


def test_attn_sp_forward_against_rounded_operands(ops):
    """the fused attention core: S = q k^T on rounded q, k; fp32 softmax; P rounded to bf16 before P v (as the split mode's hi plane)"""
    g = torch.Generator().manual_seed(5)
    B, N, Cc = 2, 256, 256
    scale = Cc ** -0.5
    qkv = torch.randn(B * N, 3 * Cc, generator=g).cuda()
    qs = ops.split_rows(qkv)
    q, k, v = (rnd(t).reshape(B, N, Cc) for t in qkv.split(Cc, dim=1))
    p = torch.softmax(scale * (q @ k.transpose(1, 2)), dim=-1)
    ref = (rnd(p) @ v).reshape(B * N, Cc)
    o1, _ = ops.attn_sp_fwd(qs, B, 1, scale, want_pt=False, mode=BF16)
    o3, _ = ops.attn_sp_fwd(qs, B, 1, scale, want_pt=False, mode=BF16X3)
    _pair("attn_sp_fwd", planes_to_f32(o1), planes_to_f32(o3), ref, TOL_ATTN)


def test_thin_convs_take_the_matrix_path(ops):
    """the 3-channel convolutions (conv_thin.hip) run their MFMA kernels in bf16 mode (three products there, like bf16x3), not the FMA path"""
    g = torch.Generator().manual_seed(3)
    x3 = torch.randn(4, 32, 32, 3, generator=g).cuda(); w_in = (torch.randn(128, 3, 3, 3, generator=g) * 0.1).cuda()
    dy = torch.randn(4, 32, 32, 128, generator=g).cuda()
    y1, y3, y0 = (ops.conv3x3_fwd(x3, w_in, mode=m) for m in (BF16, BF16X3, F32))
    assert torch.equal(y1, y3) and not torch.equal(y1, y0)
    (w1, b1), (w3, b3) = (ops.conv3x3_wgrad(x3, dy, mode=m, with_db=True) for m in (BF16, BF16X3))
    assert torch.equal(w1, w3) and torch.equal(b1, b3)


# ------------------------------------------------------------------------------------------------ whole network
def _cifar_step(m, ops, golden):
    g = golden("full_size"); tag = "cifar128"
    _, a, ac = sched_ref.make_tables()
    x0, R, t, eps = C.train_inputs(U.CIFAR10_32, 128)
    xn, tg = ops.qsample(x0.cuda(), R.cuda(), eps.cuda(), t.cuda(), a.cuda(), ac.cuda())
    m.flat.grad = None
    pred = m(xn.permute(0, 3, 1, 2), t.cuda(), return_dict=False)[0]
    loss, dp = ops.loss_fwd_bwd(pred.permute(0, 2, 3, 1), tg, "l2")
    pred.backward(dp.reshape(pred.permute(0, 2, 3, 1).shape).permute(0, 3, 1, 2))
    names = [str(s) for s in g[f"{tag}_names"]]
    grads = m.logical_grads()
    gn = np.array([float(grads[k].double().norm()) for k in names])
    ref = g[f"{tag}_gradnorms"]
    big = ref > 1e-3 * ref.max()
    norm = float(ops.sumsq(m.flat.grad).sqrt())
    return {"pred": relerr(pred.detach()[list(C.FULL_ROWS)], torch.as_tensor(g[f"{tag}_pred_rows"])),
            "loss": abs(float(loss) - float(g[f"{tag}_loss"])) / abs(float(g[f"{tag}_loss"])),
            "gradnorm": float((np.abs(gn - ref) / ref)[big].max()),
            "clip": abs(norm - float(g[f"{tag}_total_norm"])) / float(g[f"{tag}_total_norm"])}


def test_cifar_full_batch_against_golden(ops, golden):
    """G10: DDPM-CIFAR10-32 at batch 128 -- prediction rows, loss, per-tensor gradient norms, clip norm"""
    import baddiffusion_amd.unet as unet
    m = unet.unet_from_config(U.CIFAR10_32, compute_mode="bf16").cuda()
    m.load_state_dict(U.gen_params(U.CIFAR10_32, 0))
    e1 = _cifar_step(m, ops, golden)
    m.set_compute_mode("bf16x3")
    e3 = _cifar_step(m, ops, golden)
    print("MEASURE cifar128 bf16", e1, "bf16x3", e3)
    # measured: prediction rows 6.0e-3, loss 1.2e-4, per-tensor gradient norms <= 1.7e-3, clip norm 1.4e-6 (bf16x3: 1.3e-5 / 1e-7 / 2.8e-6 / 1.5e-6)
    assert e1["pred"] < 1.5e-2 and e1["loss"] < 3.5e-4 and e1["gradnorm"] < 5e-3 and e1["clip"] < 4e-6, e1
    assert e1["pred"] > e3["pred"], (e1, e3)


def test_celeba256_batch4_against_golden(ops, golden):
    """G12: the 256x256 network at B = 4 (strip-order conv_ps3 / wgrad3, igemm attention at dh = 512)"""
    import baddiffusion_amd.unet as unet
    g = golden("full_size_b4"); tag = "celeba256b4"
    m = unet.unet_from_config(U.CELEBA_HQ_256, compute_mode="bf16").cuda()
    m.load_state_dict(U.gen_params(U.CELEBA_HQ_256, 5))
    res = {}
    for mode in ("bf16", "bf16x3"):
        m.set_compute_mode(mode)
        m.flat.grad = None
        x, t, dout = C.celeba_b4_inputs()
        out = m(x.cuda(), t.cuda(), return_dict=False)[0]
        e_out = relerr(out.detach()[:, :, ::16, ::16], torch.as_tensor(g[f"{tag}_out_slices"]))
        out.backward(dout.cuda())
        names = [str(s) for s in g[f"{tag}_names"]]
        grads = m.logical_grads()
        gn = np.array([float(grads[k].double().norm()) for k in names])
        ref = g[f"{tag}_gradnorms"]
        big = ref > 1e-3 * ref.max()
        res[mode] = (e_out, float((np.abs(gn - ref) / ref)[big].max()))
    print("MEASURE celeba256b4", res)
    # measured: output slices 5.5e-3, per-tensor gradient norms <= 6.4e-3 (bf16x3: 1.2e-5 / 1.3e-5)
    assert res["bf16"][0] < 1.5e-2 and res["bf16"][1] < 1.9e-2, res
    assert res["bf16"][0] > res["bf16x3"][0], res


def _inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, 3, 32, 32, generator=g).cuda(), torch.randint(0, 1000, (n,), generator=g).cuda(),
            torch.randn(n, 3, 32, 32, generator=g).cuda() / (n * 3072))


@pytest.fixture(scope="module")
def cifar(ops):
    import baddiffusion_amd.unet as unet
    m = unet.unet_from_config(U.CIFAR10_32, compute_mode="bf16").cuda()
    m.load_state_dict(U.gen_params(U.CIFAR10_32, 5))
    return m


def _fwd_bwd(m, x, t, d):
    m.flat.grad = None
    out = m(x, t, return_dict=False)[0]
    out.backward(d)
    return out.detach().clone(), m.flat.grad.detach().clone()


def test_schedule_independence_and_determinism(cifar):
    """Two identical runs are bit-identical.  Across schedules (two streams vs one, a row inside batches of 3 / 33 / 128 / 129 vs the batch of
    one) the kernels sum in another fp32 order, and in this mode that difference does not stay at the fp32 level: a perturbation d of a value
    moves its bf16 rounding with probability ~ d / ulp_bf16, so each rounded layer turns d into ~sqrt(d * ulp_bf16), and after a few layers the
    two schedules differ by the mode's own rounding noise.  Measured: output 4.0e-3, gradient 1.0e-2, rows 4.5e-3 -- the same order as the
    distance between the bf16 and bf16x3 results of the same batch (5.4e-3).  Held to 2.5x."""
    m = cifar
    m.set_compute_mode("bf16")
    x, t, d = _inputs(128, 3)
    a = _fwd_bwd(m, x, t, d)
    b = _fwd_bwd(m, x, t, d)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])           # two identical runs: bit-identical
    m.set_aux_stream(False)
    try:
        s = _fwd_bwd(m, x, t, d)
    finally:
        m.set_aux_stream(True)
    e_out, e_grad = relerr(s[0], a[0]), relerr(s[1], a[1])
    print(f"MEASURE single_stream out {e_out:.3e} grad {e_grad:.3e}")
    assert e_out < 1e-2 and e_grad < 2.5e-2
    x, t, _ = _inputs(129, 1)
    worst = 0.0
    with torch.no_grad():
        ones = {j: m(x[j: j + 1], t[j: j + 1], return_dict=False)[0].clone() for j in (0, 1, 2, 32, 64, 127, 128)}
        for B in (3, 33, 128, 129):
            out = m(x[:B], t[:B], return_dict=False)[0]
            for j, o in ones.items():
                if j < B:
                    worst = max(worst, relerr(out[j: j + 1], o))
    print(f"MEASURE rows_vs_batch_of_one {worst:.3e}")
    assert worst < 1.2e-2


def test_mode_switches_leave_no_state(cifar):
    m = cifar
    x, t, d = _inputs(16, 4)
    for seq in (("bf16x3", "bf16", "bf16x3"), ("f32", "bf16", "f32"), ("bf16", "bf16x3", "bf16")):
        res = []
        for mode in seq:
            m.set_compute_mode(mode)
            res.append(_fwd_bwd(m, x, t, d))
        assert torch.equal(res[0][0], res[2][0]) and torch.equal(res[0][1], res[2][1]), seq
        assert not torch.equal(res[0][0], res[1][0]), seq
    m.set_compute_mode("bf16")


def test_training_trajectory_and_sampling(golden):
    """G14: the 32-step TrainEngine trajectory in bf16 mode, then five DDPM steps from the trigger-initialised images"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests.test_hip_round5 import _replay_trajectory
    from baddiffusion_amd.pipelines import DDPMPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    gpu = torch.device("cuda")
    g = golden("trajectory")
    losses, norms, lrs, sd, m, trigger, target = _replay_trajectory("bf16", gpu)
    assert np.isfinite(losses).all() and np.isfinite(norms).all()
    rl_steps = np.abs(losses - g["loss"]) / g["loss"]
    rl = float(rl_steps.max())
    worst, mean = {}, {}
    for clip in (True, False):
        pipe = DDPMPipeline(m, DDPMScheduler(clip_sample=clip))
        init = C.traj_sample_init() + trigger.unsqueeze(0)
        r = pipe(batch_size=init.shape[0], generator=torch.Generator().manual_seed(C.PIPE_SEED), init=init, output_type=None,
                 num_inference_steps=C.TRAJ_SAMPLE_STEPS)
        err = np.abs(r.images - g[f"ddpm{C.TRAJ_SAMPLE_STEPS}_trigger_init_{int(clip)}"])
        worst[clip], mean[clip] = float(err.max()), float(err.mean())
    print(f"MEASURE trajectory loss_rel warmup {rl_steps[: C.TRAJ_WARMUP].max():.3e} all {rl:.3e} median {np.median(rl_steps):.3e} "
          f"images max {worst} mean {mean}")
    # Measured: the first step's loss 2.6e-6 from the golden, 2.0e-3 at most over the first eight steps; then the trajectory parts from the fp64
    # one (Adam's m / sqrt(v) turns the ~1e-3 gradient differences of this small network into whole +-lr moves of single weights, and the pre-clip
    # norm is as sensitive here as in the split mode, only from a larger start): 0.19 at worst over 32 steps, median 0.02.  The sampled images
    # carry that drift: mean |error| 0.083 with clipping, 0.0094 without, max 0.28 with clipping.
    assert rl_steps[0] < 1e-5 and rl_steps[:8].max() < 6e-3 and rl < 0.5 and np.median(rl_steps) < 0.045, rl_steps
    assert worst[True] < 0.6, worst
    assert mean[True] < 0.2 and mean[False] < 0.025, mean
