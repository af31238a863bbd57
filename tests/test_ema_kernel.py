"""GPU: the EMA shadow update fused into clip + Adam (bd_adam_clip_ema, bd_adam_clip_ema_dev) and on its own (bd_ema_update).

Reference: diffusers' EMAModel.step, training_utils.py:200-202 -- `s_param.sub_(one_minus_decay * (s_param - param))`, evaluated by
torch on the CPU from the old shadow and the kernel's own p output; all comparisons are torch.equal (the three fp32 roundings of that
expression are reproduced, not approximated).  p, m, v and the gradient norm must be the bits of bd_adam_clip on the same inputs.

Sizes: 1, 5, 1023 and one ragged element range more than a pass of the full grid (8192 blocks of TPB = 256 threads, elementwise.hip), so
the stride loop takes a second, partial trip.  The shadow sits dense in a tensor of its own, and again one float into a NaN-filled
buffer (4-byte aligned only); p, m and v sit inside NaN-filled buffers too, and everything outside [0, n) must stay NaN."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TPB, GRID_CAP = 256, 8192            # elementwise.hip: constexpr TPB; nblocks(n, TPB, 8192) of the clip + Adam launches
SIZES = [1, 5, 1023, TPB * GRID_CAP + 77]
DECAYS = [0.0, 2 / 11, 0.9999, 1.0]
PAD = 4                              # floats of NaN margin on both sides of p, m, v (keeps them 16-byte aligned)
LR, B1, B2, EPS, STEP, MAX_NORM = 2e-4, 0.9, 0.999, 1e-8, 2, 1.0


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


_INPUTS = {}


def inputs(n):
    """host tensors shared by every case of one size (never modified): p, m, v >= 0, old shadow, a unit-norm gradient direction"""
    if n not in _INPUTS:
        g = torch.Generator().manual_seed(1000 + n % 997)
        p = torch.randn(n, generator=g)
        m = torch.randn(n, generator=g) * 1e-2
        v = torch.rand(n, generator=g) * 1e-3
        s = p + torch.randn(n, generator=g) * 1e-2
        d = torch.randn(n, generator=g)
        _INPUTS[n] = (p, m, v, s, d / d.norm())
    return _INPUTS[n]


def padded(x, lead, trail, dev):
    buf = torch.full((lead + x.numel() + trail,), float("nan"), device=dev)
    buf[lead: lead + x.numel()].copy_(x)
    return buf


def margins_nan(buf, lead, n):
    return bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + n:]).all()) and not bool(torch.isnan(buf[lead: lead + n]).any())


class Bufs:
    """device copies of one size's inputs: p, m, v in NaN-margined buffers; the shadow dense (offset 0 of its own tensor) or one float
    into a NaN-filled buffer"""

    def __init__(self, n, gnorm, shadow_offset, dev):
        p, m, v, s, d = inputs(n)
        self.n = n
        self.P, self.M, self.V = (padded(x, PAD, PAD, dev) for x in (p, m, v))
        self.p, self.m, self.v = (b[PAD: PAD + n] for b in (self.P, self.M, self.V))
        self.so = shadow_offset
        self.S = padded(s, shadow_offset, 1 if shadow_offset else 0, dev)
        self.s = self.S[shadow_offset: shadow_offset + n]
        assert self.s.data_ptr() % 16 == (4 * shadow_offset) % 16
        self.g = (d * gnorm).to(dev)
        self.gn = torch.full((3,), float("nan"), device=dev)       # the norm goes to element 1

    def outputs_in_bounds(self):
        return all(margins_nan(b, PAD, self.n) for b in (self.P, self.M, self.V)) and margins_nan(self.S, self.so, self.n) \
            and bool(torch.isnan(self.gn[0])) and bool(torch.isnan(self.gn[2]))

    def cpu(self):
        return tuple(t.cpu().clone() for t in (self.p, self.m, self.v, self.s, self.gn[1]))


def omd32(decay):
    return float(np.float32(1 - decay))


@pytest.mark.parametrize("shadow_offset", [0, 1], ids=["dense", "offset1"])
@pytest.mark.parametrize("n", SIZES)
def test_fused_dev_and_standalone_forms(gpu, n, shadow_offset):
    from baddiffusion_amd import _lib as L
    from baddiffusion_amd import ops
    lib = L.load()
    _, _, _, s_old, _ = inputs(n)
    for gnorm in (30.0, 0.5):                 # clip active (coef = 1 / 30) and not (coef = 1)
        # bd_adam_clip on clones of the same inputs: what p, m, v and the norm must be
        base = Bufs(n, gnorm, shadow_offset, gpu)
        ss = ops.sumsq(base.g)
        ops.adam_clip(base.p, base.g, base.m, base.v, ss, STEP, LR, MAX_NORM, (B1, B2), EPS, grad_norm_out=base.gn[1:2])
        bp, bm, bv, bs, bgn = base.cpu()
        assert base.outputs_in_bounds() and torch.equal(bs, s_old)
        assert (abs(float(bgn) - gnorm) < 1e-4 * gnorm) and not torch.equal(bp, inputs(n)[0])
        for decay in DECAYS:
            omd = omd32(decay)
            what = (n, shadow_offset, gnorm, decay)
            # the reference's expression on the CPU, from the old shadow and the kernel's own p
            want = s_old.clone().sub_((1 - decay) * (s_old - bp))

            def fused():
                b = Bufs(n, gnorm, shadow_offset, gpu)
                ops.adam_clip(b.p, b.g, b.m, b.v, ss, STEP, LR, MAX_NORM, (B1, B2), EPS, grad_norm_out=b.gn[1:2], ema=b.s,
                              one_minus_decay=omd)
                assert b.outputs_in_bounds(), what
                return b.cpu()
            fp, fm, fv, fs, fgn = fused()
            assert torch.equal(fp, bp) and torch.equal(fm, bm) and torch.equal(fv, bv) and torch.equal(fgn, bgn), what
            assert torch.equal(fs, want), (what, float((fs - want).abs().max()))
            if decay == 1.0:
                assert torch.equal(fs, s_old), what
            # a second call on the same inputs
            assert all(torch.equal(a, b) for a, b in zip(fused(), (fp, fm, fv, fs, fgn))), what
            # the device-scalar form with the same three fp32 scalars
            b = Bufs(n, gnorm, shadow_offset, gpu)
            hyper = torch.tensor([LR / (1 - B1 ** STEP), math.sqrt(1 - B2 ** STEP), omd], dtype=torch.float32).to(gpu)
            L.check(lib.bd_adam_clip_ema_dev(b.p.data_ptr(), b.g.data_ptr(), b.m.data_ptr(), b.v.data_ptr(), b.s.data_ptr(), n, ss.data_ptr(),
                                             MAX_NORM, hyper.data_ptr(), B1, B2, EPS, b.gn[1:2].data_ptr(), L.stream()), "bd_adam_clip_ema_dev")
            assert b.outputs_in_bounds(), what
            assert all(torch.equal(x, y) for x, y in zip(b.cpu(), (fp, fm, fv, fs, fgn))), what
            # the stand-alone update on the same p
            b = Bufs(n, gnorm, shadow_offset, gpu)
            b.p.copy_(bp)
            ops.ema_update(b.s, b.p, omd)
            assert b.outputs_in_bounds(), what
            ap, am, av, as_, _ = b.cpu()
            assert torch.equal(as_, fs) and torch.equal(ap, bp) and torch.equal(am, inputs(n)[1]) and torch.equal(av, inputs(n)[2]), what


def test_ops_wrappers_refuse_mismatched_shadow(gpu):
    from baddiffusion_amd import ops
    p = torch.zeros(8, device=gpu); s = torch.zeros(9, device=gpu)
    with pytest.raises(TypeError):
        ops.ema_update(s, p, 0.5)
    with pytest.raises(TypeError):
        ops.ema_update(torch.zeros(16, device=gpu)[::2], p, 0.5)
    with pytest.raises(ValueError):
        ops.adam_clip(p, p.clone(), p.clone(), p.clone(), ops.sumsq(p), 1, 1e-3, ema=p.clone())
    with pytest.raises(RuntimeError):      # the library's own overlap check, through the wrapper
        ops.ema_update(p, p, 0.5)
