"""Shared cases of the variational-bound fixtures (tests/golden/vb.npz): imported by make_golden_vb.py (CPU, where the reference can be
imported) and by tests/test_vb_host.py / tests/test_vb.py, so both sides build the same inputs from the same seeds.

`kernel_formula` restates bd_vb_terms (include/bd_hip.h, baddiffusion_amd/likelihood.py) with torch ops, generic in dtype:
  * float64: the contract -- x0_hat formed in float32 from the float32 alphas_cumprod table, everything after it in float64 with the
    float64 schedule scalars.  Every expected value of the fixture is this evaluation on the float32 inputs.
  * float32: the same element arithmetic in float32 with the schedule scalars rounded to float32 (the tables the kernel is handed); the
    mean is taken in float64, as the kernel accumulates.  Its distance from the float64 value is stored beside each expected value as
    `d32`: the error of the number format, the yardstick of the tests' bound max(4e-6 |ref|, 4 d32).
`textbook_nll` is the t = 0 element written as Phi(z+) - Phi(z-), the form the kernel is NOT defined in."""
import math

import numpy as np
import torch

T = 1000
BETA_START, BETA_END = 0.0001, 0.02
VARIANCE_TYPES = ("fixed_small", "fixed_large")
LN2 = math.log(2.0)
FLOOR_BITS = -math.log(1e-12) / LN2                  # 39.86...: a pixel whose bin has less than 1e-12 of the mass
TS_MIX = (0, 1, 2, 500, T - 1, T)
# D = 1, 255, 257, 8191, 8192, 8193, 3 * 8192 + 5 (one chunk of 8192 logical elements per workgroup): C in {1, 3}, W = 1, H = 1, non-square
SHAPES = ((1, 1, 1), (3, 5, 17), (1, 1, 257), (1, 8191, 1), (1, 64, 128), (3, 1, 2731), (1, 47, 523))
NS = (1, 5)
BIG_N, BIG_SHAPE, BIG_TS = 65535 + 3, (1, 3, 5), (0, 1, T, 500)      # three rows more than one launch's grid.y; four distinct rows repeated
REGIME_SHAPE = (3, 32, 32)
REGIME_SCALES = (0.003, 0.01, 0.03, 0.1)
# floor share of each scale regime (the share of pixels with P < 1e-12), asserted by the generator
REGIME_FLOOR = {0.003: (0.0, 0.0), 0.01: (0.0, 0.0), 0.03: (0.03, 0.09), 0.1: (0.45, 0.65)}
E2E_CFG, E2E_PARAM_SEED, E2E_N, E2E_TS, E2E_DATA_SEED, E2E_NOISE_SEED = "small", 7, 4, (0, 1, 2, 250, T - 1), 77, 4243


def schedule():
    """(betas, alphas, alphas_cumprod) in float32, as schedulers._Base._make_tables builds the linear schedule"""
    betas = torch.linspace(BETA_START, BETA_END, T, dtype=torch.float32)
    alphas = 1.0 - betas
    return betas, alphas, torch.cumprod(alphas, dim=0)


def tables64(vt):
    """the closed forms of the issue in float64 from the float32 tables: dict of float64 tensors sigma2 [T] (entry 0 = sigma2_dec),
    c0 [T], delta [T], add / mul [T + 1] (bits = (add[t] + mul[t] * mean element term) / ln 2) and the float inv_sigma_dec"""
    betas, _, ab = schedule()
    b, ab = betas.double(), ab.double()
    abp = torch.cat((torch.ones(1, dtype=torch.float64), ab[:-1]))
    btilde = b * (1 - abp) / (1 - ab)
    c0 = abp.sqrt() * b / (1 - ab)
    sigma2 = (btilde if vt == "fixed_small" else b).clone()
    sigma2[0] = btilde[1]
    delta = torch.zeros(T, dtype=torch.float64)
    delta[1:] = sigma2[1:].log() - btilde[1:].log()
    add, mul = torch.zeros(T + 1, dtype=torch.float64), torch.ones(T + 1, dtype=torch.float64)
    add[1:T] = 0.5 * (-1 + delta[1:] + torch.exp(-delta[1:]))
    mul[1:T] = 0.5 * c0[1:] ** 2 / sigma2[1:]
    add[T] = 0.5 * (-1 - torch.log(1 - ab[-1]) + (1 - ab[-1]))
    mul[T] = 0.5 * ab[-1]
    return {"sigma2": sigma2, "c0": c0, "delta": delta, "add": add, "mul": mul, "inv_sigma_dec": 1.0 / math.sqrt(float(btilde[1]))}


def data_x0(u):
    """the data path's normalisation of uint8 values, in float32: u = 0 and u = 255 land in the two edge bins and nothing else does"""
    return (u.to(torch.float32) / 255.0) / (1.0 + 1e-5) * 2.0 - 1.0


def coef(t):
    """(sqrt(abar_t), sqrt(1 - abar_t)) as 0-dim float32 tensors.  The roots are numpy's scalar float32 sqrt, which is correctly rounded on
    every host as the device's sqrtf is; torch.sqrt on the CPU was seen one ulp off on one host, and at t = T-1 the division by
    sqrt(abar_t) = 0.0064 turns one ulp of sqrt(1 - abar_t) into 2e-4 / sqrt(D) of a row's mean square."""
    a = np.float32(schedule()[2][t].item())
    return torch.tensor(np.sqrt(a)), torch.tensor(np.sqrt(np.float32(1.0) - a))


def x0_hat(x_t, eps, t, clip):
    """the predicted clean image in float32, the expression of the step kernels"""
    sa, sb = coef(t)
    xh = (x_t - sb * eps) / sa
    return xh.clamp(-1.0, 1.0) if clip else xh


def _dec_z(x0, xh, inv_sigma, dtype):
    d = x0.to(dtype) - xh.to(dtype)
    h = torch.tensor(1.0 / 255.0, dtype=dtype)
    s = torch.tensor(inv_sigma, dtype=torch.float64).to(dtype)
    return (d + h) * s, (d - h) * s


def dec_prob(x0, xh, inv_sigma, dtype):
    """P_i of the discretised Gaussian decoder, erfc on the tail side (before the floor)"""
    zp, zm = _dec_z(x0, xh, inv_sigma, dtype)
    r2 = torch.tensor(math.sqrt(0.5), dtype=dtype)
    lo, hi, tail = x0 < -0.999, x0 > 0.999, zm > 0
    a = torch.where(lo, -zp, torch.where(hi | tail, zm, -zp))
    b = torch.where(tail, zp, -zm)
    return 0.5 * (torch.special.erfc(a * r2) - torch.where(lo | hi, torch.zeros_like(b), torch.special.erfc(b * r2)))


def _floored_nll(P):
    return -torch.log(torch.where(P < 1e-12, torch.full_like(P, 1e-12), P))          # by comparison: a NaN stays a NaN


def dec_nll(x0, xh, inv_sigma, dtype):
    return _floored_nll(dec_prob(x0, xh, inv_sigma, dtype))


def textbook_nll(x0, xh, inv_sigma, dtype):
    """the same element as Phi(z+) - Phi(z-) with Phi(z) = (1 + erf(z / sqrt 2)) / 2"""
    zp, zm = _dec_z(x0, xh, inv_sigma, dtype)
    r2 = torch.tensor(math.sqrt(0.5), dtype=dtype)
    Phi = lambda z: 0.5 * (1 + torch.erf(z * r2))
    P = torch.where(x0 < -0.999, Phi(zp), torch.where(x0 > 0.999, 1 - Phi(zm), Phi(zp) - Phi(zm)))
    return _floored_nll(P)


def floor_share(x0, xh, inv_sigma):
    return float((dec_prob(x0, xh, inv_sigma, torch.float64) < 1e-12).double().mean())


def kernel_formula(x0, x_t, eps, ts, vt, clip, dtype, nll=dec_nll):
    """(bits [N], x0_mse [N]) as float64 tensors: rows n of float32 [N,C,H,W] inputs at timesteps ts[n] in [0, T]"""
    tab = tables64(vt)
    rnd = lambda v: torch.as_tensor(v, dtype=torch.float64).to(dtype).double()       # a schedule scalar as this dtype holds it
    bits, mse = [], []
    for n, t in enumerate(int(t) for t in ts):
        v = x0[n]
        if t == T:
            e = m2 = v.to(dtype) * v.to(dtype)
        else:
            xh = x0_hat(x_t[n], eps[n], t, clip)
            df = v.to(dtype) - xh.to(dtype)
            m2 = df * df
            e = nll(v, xh, float(rnd(tab["inv_sigma_dec"])), dtype) if t == 0 else m2
        bits.append((rnd(tab["add"][t]) + rnd(tab["mul"][t]) * e.double().mean()) / LN2)
        mse.append(m2.double().mean())
    return torch.stack(bits), torch.stack(mse)


def exact_randn(shape, g):
    """unit-variance bell-shaped float32 values built from integers alone (twelve uniform 16-bit draws, Irwin-Hall; the tails end at 6),
    every one of them exactly representable: the regenerated inputs do not depend on any host's transcendental functions (see coef)"""
    s = torch.randint(0, 1 << 16, (12,) + tuple(shape), generator=g).sum(0)
    return (s - 6 * (1 << 16)).to(torch.float32) / float(1 << 16)


def make_rows(seed, N, shape, ts, s0=0.01, s=0.1, u=None, err=None):
    """float32 (x0, x_t, eps) [N, *shape]: data-like x0 from random uint8 (or `u`), x_t = q_sample(x0, noise) at ts[n], and eps such that the
    prediction is x0_hat = x0 + scale * err with scale = s0 in t = 0 rows and s elsewhere (err: exact_randn unless given).  Prior rows
    keep noise / err in x_t / eps: the kernel must not read them.  Integer draws and correctly rounded float32 operations only."""
    g = torch.Generator().manual_seed(seed)
    full = (N,) + tuple(shape)
    if u is None:
        u = torch.randint(0, 256, full, generator=g)
    x0 = data_x0(u)
    noise = exact_randn(full, g)
    if err is None:
        err = exact_randn(full, g)
    x_t, eps = noise.clone(), err.clone()
    for n, t in enumerate(int(t) for t in ts):
        if t < T:
            sa, sb = coef(t)
            x_t[n] = sa * x0[n] + sb * noise[n]
            eps[n] = noise[n] - (sa / sb) * (s0 if t == 0 else s) * err[n]
    return x0, x_t, eps


def mixed_ts(N, i):
    """N timesteps out of TS_MIX, rotated by the case index so that every value is met at every N over the cases"""
    return tuple(TS_MIX[(i + k) % len(TS_MIX)] for k in range(N))


def kernel_cases():
    """(tag, shape, N, ts, variance_type, clip, seed) of the shape cases"""
    i = 0
    for shape in SHAPES:
        for N in NS:
            for vt in VARIANCE_TYPES:
                for clip in (True, False):
                    yield f"{'x'.join(map(str, shape))}_n{N}_{vt}_{int(clip)}", shape, N, mixed_ts(N, i), vt, clip, 100 + i
                    i += 1


def big_rows():
    return make_rows(7001, len(BIG_TS), BIG_SHAPE, BIG_TS)


def regime_rows():
    """{name: (x0, x_t, eps, clip)} of one t = 0 row each at REGIME_SHAPE"""
    shape, full = REGIME_SHAPE, (1,) + REGIME_SHAPE
    out = {f"s{s}": make_rows(8000 + k, 1, shape, (0,), s0=s) + (True,) for k, s in enumerate(REGIME_SCALES)}
    out["u0"] = make_rows(8010, 1, shape, (0,), u=torch.zeros(full, dtype=torch.int64)) + (True,)
    out["u255"] = make_rows(8011, 1, shape, (0,), u=torch.full(full, 255, dtype=torch.int64)) + (True,)
    g = torch.Generator().manual_seed(8012)
    pick = torch.randint(0, 3, full, generator=g)
    u = torch.where(pick == 0, torch.zeros(full, dtype=torch.int64), torch.where(pick == 1, torch.full(full, 255, dtype=torch.int64),
                                                                                torch.randint(0, 256, full, generator=g)))
    out["mix"] = make_rows(8013, 1, shape, (0,), u=u) + (True,)
    # x0_hat = x0 + 0.5, unclipped: 68 sigma off; no edge values, whose bins are open-ended
    out["floor"] = make_rows(8014, 1, shape, (0,), s0=0.5, u=torch.randint(1, 255, full, generator=g), err=torch.ones(full)) + (False,)
    x0, x_t, eps = make_rows(8015, 1, shape, (0,))
    eps[0, 1, 2, 3] = float("nan")
    out["nan"] = (x0, x_t, eps, True)
    return out


def e2e_clean():
    """uint8 [E2E_N, 16, 16, 3] images with both edge values present"""
    u = torch.randint(0, 256, (E2E_N, 16, 16, 3), generator=torch.Generator().manual_seed(E2E_DATA_SEED), dtype=torch.uint8)
    u[:, 0, :4] = 0
    u[:, 1, :4] = 255
    return u


def e2e_noises(C=3, S=16):
    """{t: randn(E2E_N, C, S, S)} in the order bits_per_dim draws: the largest t first"""
    g = torch.Generator().manual_seed(E2E_NOISE_SEED)
    return {t: torch.randn(E2E_N, C, S, S, generator=g) for t in sorted(E2E_TS, reverse=True)}
