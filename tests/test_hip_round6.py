"""Round 6: size-independent properties of the hot path at BASELINE's full sizes, through the C ABI (bd_unet_forward / bd_unet_backward).

The goldens pin fixed batches (G7 B = 2, G10 B = 128, G12 256 x 256 B = 4).  The plan, however, picks kernels by batch size -- two half-batch forward
pipelines from 32 K pixels, K splits of the 8 x 8 / 4 x 4 levels by tile count, 128- vs 256-row tiles, ragged last tiles -- so the properties
the DOMAIN guarantees are checked across those switches:
  * samples are independent all the way through a UNet2DModel (GroupNorm is per sample, attention per sample: unet_2d.py:216-297): row j of a
    batch of any size equals the batch-of-one evaluation of sample j;
  * the gradient is additive over samples: grads(batch) == grads(first part) + grads(rest) for dL/dpred given;
  * a data-parallel step is the same computation: the all-reduced sum over r::world shards of the batch equals the one-process gradient (the
    1/world pre-scale of dL/dpred)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_ref as U


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import baddiffusion_amd.unet as unet
    m = unet.unet_from_config(U.CIFAR10_32).cuda()
    m.load_state_dict(U.gen_params(U.CIFAR10_32, 5))
    return m


def relerr(a, b):
    a = a.detach().double(); b = b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 32, 32, 3, generator=g).cuda()
    t = torch.randint(0, 1000, (n,), generator=g).cuda()
    d = torch.randn(n, 32, 32, 3, generator=g).cuda()
    return x, t, d


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
def test_rows_of_any_batch_equal_the_batch_of_one(model, mode):
    """B = 1, 3 (ragged 128-row tiles at 4 x 4: 48 rows), 33 (two pipelines of 16 + 17), 129 (64 + 65), 128, 379 (189 + 190: the 8 x 8 level is
    a "large" layer there and runs the general 256 x 128 kernel, conv_ps_kernel, with a ragged last tile -- rows 188 / 189 sit either side of
    the pipeline boundary, 378 is the last row): every row against its own B = 1 evaluation.  Tolerance 2e-5 relative: the products are the
    same, the K-split / tile choice (fp32 summation order) follows the batch."""
    m = model
    m.set_compute_mode(mode)
    try:
        x, t, _ = _inputs(379, 1)
        with torch.no_grad():
            ones = {j: m._run_forward(m.flat.data, x[j: j + 1].contiguous(), t[j: j + 1].contiguous(), False)[0].clone()
                    for j in (0, 1, 2, 16, 32, 64, 127, 128, 188, 189, 378)}
            for B in (3, 33, 128, 129, 379):
                out = m._run_forward(m.flat.data, x[:B].contiguous(), t[:B].contiguous(), False)[0]
                assert bool(torch.isfinite(out).all())
                for j, o in ones.items():
                    if j < B:
                        assert relerr(out[j: j + 1], o) < (2e-5 if mode == "bf16x3" else 5e-6), (mode, B, j)
    finally:
        m.set_compute_mode("bf16x3")


def test_gradient_is_additive_over_samples(model):
    """grads(B = 40) == grads(rows 0..32) + grads(rows 33..39) for the same dL/dpred rows (5e-5 relative on the whole flat gradient -- measured
    1.6e-5: both sides carry their own split-bf16 rounding, and a random unit-variance dL/dpred makes the sums cancel heavily -- and 5e-4 on every
    parameter tensor whose gradient is not rounding noise), across the two-pipeline switch (40 and 33 rows run as two pipelines, 7 as one)."""
    m = model
    x, t, d = _inputs(40, 2)

    def grads(lo, hi):
        xs, ts, ds = x[lo:hi].contiguous(), t[lo:hi].contiguous(), d[lo:hi].contiguous()
        _, ws = m._run_forward(m.flat.data, xs, ts, True)
        g = m._run_backward(m.flat.data, xs, ds, ws).clone()
        m._release_ws(ws)
        return g

    whole, a, b = grads(0, 40), grads(0, 33), grads(33, 40)
    assert relerr(a + b, whole) < 5e-5
    for name, (off, shape, _) in m._table.items():
        n = int(np.prod(shape))
        w = whole[off: off + n]
        if name.endswith("key.bias") or float(w.norm()) < 1e-6 * float(whole.norm()):      # mathematically zero / rounding-level gradients
            continue
        assert relerr((a + b)[off: off + n], w) < 5e-4, name


def test_sharded_gradient_sum_equals_one_process(model):
    """SURVEY 8(e) at the per-GPU size of BASELINE configs[2]: the sum over rank shards r::world of the (1/world pre-scaled) gradient equals the
    gradient of the global batch -- world 4 x 32 rows against one pass over 128, the arithmetic of the RCCL all-reduce done here by plain addition."""
    m = model
    from baddiffusion_amd import ops
    x, t, _ = _inputs(128, 3)
    tgt = torch.randn(128, 32, 32, 3, generator=torch.Generator().manual_seed(9)).cuda()

    def grads(rows, scale):
        xs, ts, tg = x[rows].contiguous(), t[rows].contiguous(), tgt[rows].contiguous()
        pred, ws = m._run_forward(m.flat.data, xs, ts, True)
        loss, dpred = ops.loss_fwd_bwd(pred, tg, "l2", grad_scale=scale)
        g = m._run_backward(m.flat.data, xs, dpred, ws).clone()
        m._release_ws(ws)
        return float(loss), g

    l1, g1 = grads(slice(0, 128), 1.0)
    world = 4
    parts = [grads(slice(r, 128, world), 1.0 / world) for r in range(world)]
    gsum = sum(g for _, g in parts)
    assert relerr(gsum, g1) < 1e-5
    assert abs(sum(l for l, _ in parts) / world - l1) < 1e-5 * abs(l1)
