"""References of the dynamic-thresholding tests: bd_abs_quantile and the thresholded bd_ddpm_step / bd_ddim_step (csrc/elementwise.hip) as
numpy-float32 statements, one rounding per operation in the kernels' order, in the style of tests/_step_exact.py (whose coefficient
functions they use).  tests/test_dyn_threshold_host.py ties them to the golden vectors (tests/golden/threshold.npz, written by the
reference on the CPU); tests/test_dyn_threshold.py holds the kernels to EQUAL BITS against them.  Nothing here touches a device or
imports the product's kernels.

The interpolation of the quantile is a fused multiply-add in the reference's arithmetic (at::lerp on the CPU) and in the kernel (an
explicit fmaf).  numpy has none, and a float64 product-and-sum rounded to float32 rounds twice, so `fma32` forms a * b + c exactly in
rational arithmetic and rounds once, to nearest-even, denormals included.  Only B values per case go through it."""
from fractions import Fraction
from types import SimpleNamespace as NS

import numpy as np
import torch

from tests import _step_exact as X

f32 = np.float32


def round_to_f32(fr):
    """the fp32 nearest to the rational fr, ties to even, gradual underflow, overflow to inf"""
    if fr == 0:
        return f32(0)
    sign, mag = (-1.0 if fr < 0 else 1.0), abs(fr)
    e = mag.numerator.bit_length() - mag.denominator.bit_length()          # 2^(e-1) <= mag < 2^(e+1)
    if mag < Fraction(2) ** e:
        e -= 1                                                              # now 2^e <= mag < 2^(e+1)
    qexp = max(e, -126) - 23                                                # the spacing of fp32 in that binade
    n = mag / Fraction(2) ** qexp
    lo = n.numerator // n.denominator
    rest = n - lo
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    if lo * Fraction(2) ** qexp > Fraction(int(np.finfo(f32).max.astype(np.float64))):
        return f32(sign * np.inf)
    return f32(sign * float(lo) * 2.0 ** qexp)                              # lo <= 2^24 and the power are exact in float64


def fma32(a, b, c):
    """fmaf(a, b, c): a * b + c rounded once"""
    a, b, c = f32(a), f32(b), f32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore"):
            return f32(np.float64(a) * np.float64(b) + np.float64(c))       # the IEEE result is inf or NaN either way
    return round_to_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def quantile_ranks(q, m):
    """(lo, hi, w) of torch.quantile in fp32: rank = q (m - 1), lo = floor, hi = ceil, w = rank - lo"""
    rank = f32(q) * f32(m - 1)
    below = np.floor(rank)
    w = f32(rank - below)
    lo = min(int(below), m - 1)
    return lo, min(lo + (1 if w > 0 else 0), m - 1), w


def abs_quantile_stmt(x, q):
    """bd_abs_quantile: [B] float32 from [B, ...] float32.  a, b = the order statistics of |x| at lo and hi; d = b - a;
    w < 0.5 ? fmaf(w, d, a) : fmaf(-d, 1 - w, b); NaN for a row that holds one"""
    x = np.asarray(x, dtype=f32)
    a = np.sort(np.abs(x.reshape(x.shape[0], -1)), axis=1)                  # -0 has become 0; NaNs sort last
    lo, hi, w = quantile_ranks(q, a.shape[1])
    out = np.empty(a.shape[0], dtype=f32)
    with np.errstate(invalid="ignore"):
        for b, row in enumerate(a):
            if np.isnan(row[-1]):
                out[b] = np.nan
                continue
            d = f32(row[hi] - row[lo])
            out[b] = fma32(w, d, row[lo]) if w < f32(0.5) else fma32(-d, f32(1) - w, row[hi])
    return out


def threshold_stmt(x0, q, smax):
    """x0_threshold of the step kernels: s = clamp(q, 1, sample_max_value) per image, a NaN staying NaN; clamp(x0, -s, s) / s"""
    q = np.asarray(q, dtype=f32).reshape((-1,) + (1,) * (x0.ndim - 1))
    with np.errstate(invalid="ignore"):
        s = np.where(np.isnan(q), q, np.minimum(np.maximum(q, f32(1)), f32(smax))).astype(f32)
        return (np.minimum(np.maximum(x0, -s), s) / s).astype(f32)


def x0_stmt(ac, t, x, e):
    """x0_pred: (x - sqrt(1 - a_t) e) / sqrt(a_t), as ddpm_stmt / ddim_stmt form it"""
    a_t = ac.astype(f32)[t]
    return (x - np.sqrt(f32(1) - a_t) * e) / np.sqrt(a_t)


def ddpm_thr_stmt(ac, c, x, e, z, smax, ratio=None, q=None):
    """(prev_sample, pred_original, raw quantile) of bd_abs_quantile + thresholded bd_ddpm_step; c as _step_exact._dp (clip is ignored).
    x, e, z are [B, ...]; q (the raw quantiles) is computed from `ratio` unless given"""
    sb, sa, c0, ct, sd = X.ddpm_coef(ac, c)
    x, e = x.astype(f32), e.astype(f32)
    x0 = (x - sb * e) / sa
    if q is None:
        q = abs_quantile_stmt(x0, ratio)
    x0 = threshold_stmt(x0, q, smax)
    prev = c0 * x0 + ct * x
    if c.t > 0:
        prev = prev + sd * z.astype(f32)
    if c.cdef is not None:
        prev = X.clamp(prev, f32(c.cdef))
    return prev, x0, q


def ddim_thr_stmt(ac, c, x, e, z, smax, ratio=None, q=None):
    """the same for bd_ddim_step; c as _step_exact._di"""
    sb, sa, sd, dr, sap = X.ddim_coef(ac, c)
    x, e = x.astype(f32), e.astype(f32)
    x0 = (x - sb * e) / sa
    if q is None:
        q = abs_quantile_stmt(x0, ratio)
    x0 = threshold_stmt(x0, q, smax)
    prev = sap * x0 + dr * e
    if c.eta > 0:
        prev = prev + sd * z.astype(f32)
    return prev, x0, q


def ddpm_case(t, prev_t, variance_type, cdef=None):
    return NS(t=t, prev_t=prev_t, vt={"fixed_small": 0, "fixed_large": 1}[variance_type], clip=None, cdef=cdef, x0=True, noise=True)


def ddim_case(t, prev_t, eta, final=1.0):
    return NS(t=t, prev_t=prev_t, final=final, eta=eta, clip=None, x0=True)


def chain_stmt(sched, smax, ratio, steps, model, x, noise_seed):
    """every sample of a thresholded DDPM / DDIM chain of `steps` steps over the 1000-step table, the stand-in `model` evaluated by
    torch on the CPU, the DDPM variance noise drawn from a CPU generator as the schedulers draw it"""
    _, ac = X.tables()
    stride = 1000 // steps
    g = torch.Generator().manual_seed(noise_seed)
    x = x.numpy().astype(f32)
    out = []
    for t in range((steps - 1) * stride, -1, -stride):
        e = model(torch.from_numpy(x), t).numpy()
        if sched == "ddpm":
            z = torch.randn(x.shape, generator=g).numpy() if t > 0 else None
            x = ddpm_thr_stmt(ac, ddpm_case(t, t - stride, "fixed_small"), x, e, z, smax, ratio)[0]
        else:
            x = ddim_thr_stmt(ac, ddim_case(t, t - stride, 0.0), x, e, None, smax, ratio)[0]
        out.append(x)
    return out
