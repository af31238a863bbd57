"""Shared seeds / shapes of the dynamic-thresholding fixtures (tests/golden/threshold.npz): imported by make_golden_threshold.py
(reference side, CPU) and by tests/test_dyn_threshold*.py, so both sides build the same inputs; only expected outputs are stored.

Quantile cases: every (B, m) of Q_SHAPES x every regime of REGIMES x every ratio of QS; expected torch.quantile(|x|.reshape(B, -1), q, dim=1).
Step cases: the reference's DDPMScheduler.step / DDIMScheduler.step with thresholding=True on PLANTED inputs -- seeded random (x, e) at
t >= 500 put every image's quantile of |x0| far above sample_max_value, where its value never matters; here x = sa u + sb e with a scale
per image on u, so that the quantile lands below 1, inside (1, sample_max_value) and above sample_max_value in turn.
Chains: 10 steps from cases.pndm_init() with cases.pndm_fake_model, and DDIM chains of the small UNet."""
import numpy as np
import torch

from tests.golden.cases import DDIM_TS, DDPM_TS

# ---------------------------------------------------------------------------------------------------- quantile
SWITCH_M = 4096                                  # bd_abs_quantile_plan(..).switch_m: the largest m of the registers path
Q_SHAPES = ((1, 1), (2, 2), (3, 7), (2, 192), (5, 193), (3, 105), (2, 3072), (3, 3073), (2, 12288), (2, 196608), (300, 192),
            (2, SWITCH_M - 1), (2, SWITCH_M), (2, SWITCH_M + 1))
QS = (0.995, 0.9, 0.5, 1.0, 0.0)
REGIMES = ("normal0", "normal1", "normal2", "spread", "quarters", "equal", "lowbits", "tiny", "nan", "inf")
NORMAL_SCALE = {"normal0": 1.0, "normal1": 4.0, "normal2": 0.25}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def quantile_input(B, m, regime):
    """[B, m] float32.  normal*: randn at three scales; spread: randn * 2^k, k in -10 .. 10, so that the two values around the rank lie far
    apart and the rounding of the interpolation shows (between neighbours of a normal sample every form of it agrees); quarters: multiples of 0.25 (crowded buckets, the bracketing values tie); equal:
    +-1.25 everywhere; lowbits: +-(1.5 + k 2^-23), k < 1024 (only the last radix pass tells them apart); tiny: 0, -0 and denormals of
    both signs; nan: normal0 with one NaN in row 0; inf: normal0 with +inf and -inf in the last row (one inf when m == 1)"""
    seed = 7919 * B + m + 101 * REGIMES.index(regime)
    if regime in NORMAL_SCALE or regime in ("nan", "inf"):
        x = torch.randn(B, m, generator=_gen(seed)) * NORMAL_SCALE.get(regime, 1.0)
        if regime == "nan":
            x[0, m // 2] = float("nan")
        if regime == "inf":
            x[B - 1, 0] = float("inf")
            x[B - 1, m - 1] = float("-inf")
        return x
    if regime == "spread":
        return torch.ldexp(torch.randn(B, m, generator=_gen(seed)), torch.randint(-10, 11, (B, m), generator=_gen(seed + 1)))      # exact
    if regime == "quarters":
        return torch.round(torch.randn(B, m, generator=_gen(seed)) * 8) / 4
    sign = torch.randint(0, 2, (B, m), generator=_gen(seed + 1), dtype=torch.int32) << 31
    if regime == "equal":
        mag = torch.full((B, m), 1.25).view(torch.int32)
    elif regime == "lowbits":
        mag = torch.full((B, m), 1.5).view(torch.int32) | torch.randint(0, 1024, (B, m), generator=_gen(seed), dtype=torch.int32)
    elif regime == "tiny":
        mag = torch.randint(0, 1 << 23, (B, m), generator=_gen(seed), dtype=torch.int32)
        mag[torch.rand(B, m, generator=_gen(seed + 2)) < 0.5] = 0                    # half of them zeros, of either sign
    else:
        raise ValueError(regime)
    return (mag | sign).view(torch.float32)


def quantile_key(B, m):
    return f"q_{B}x{m}"


def quantile_expected(g, B, m, regime, q):
    """the stored [B] vector of a case: one array [regime, ratio, B] per shape"""
    return np.asarray(g[quantile_key(B, m)])[REGIMES.index(regime), QS.index(q)]


# ---------------------------------------------------------------------------------------------------- steps
SAMPLE_MAX_VALUES = (1.0, 1.5, 3.0)
RATIOS = (0.995, 0.9)
SHAPE_A, SHAPE_B = (2, 3, 8, 8), (3, 3, 5, 7)               # m = 192; m = 105, odd
DDIM_STEPS = 50                                             # set_timesteps(50): prev_t = t - 20, as sched.npz
ETAS = (0.0, 0.5)
VARIANCE_TYPES = ("fixed_small", "fixed_large")
Z_OF_RATIO = {0.995: 2.807, 0.9: 1.645}                    # the two-sided normal quantiles: P(|Z| < z) = ratio


def _cases(ts, kinds):
    """(t, kind, sample_max_value, ratio, shape): the full cross"""
    return tuple((t, k, smax, r, shape) for t in ts for k in kinds for smax in SAMPLE_MAX_VALUES for r in RATIOS for shape in (SHAPE_A, SHAPE_B))


DDPM_STEP_CASES = _cases(DDPM_TS, VARIANCE_TYPES)           # kind = variance_type
DDIM_STEP_CASES = _cases(DDIM_TS, ETAS)                     # kind = eta


def step_key(sched, shape):
    return f"{sched}_steps_{'x'.join(map(str, shape))}"


def step_expected(g, sched, index):
    """(prev_sample, pred_original_sample) of case `index` of the scheduler's list: one array [case, 2, *shape] per shape, in list order"""
    cases = DDPM_STEP_CASES if sched == "ddpm" else DDIM_STEP_CASES
    shape = cases[index][4]
    row = sum(1 for c in cases[:index] if c[4] == shape)
    both = np.asarray(g[step_key(sched, shape)])[row]
    return both[0], both[1]


def step_id(case):
    t, kind, smax, ratio, shape = case
    return f"t{t}-{kind}-s{smax}-r{ratio}-{'x'.join(map(str, shape))}"


def regime_targets(smax):
    """the quantile of |x0| an image is aimed at: below 1, inside (1, sample_max_value) (none at 1.0: above again), above it"""
    return (0.7, (1.0 + smax) / 2 if smax > 1.0 else 1.6 * smax, 1.6 * smax)


def step_inputs(sched, index, case, alphas_cumprod):
    """(x, e, z) float32 tensors of the case's shape: x = sa u + sb e with u = randn * (target / z(ratio)) per image, the target rotating
    through regime_targets with the image and the case index; z is the variance noise"""
    t, _, smax, ratio, shape = case
    seed = 5000 + 17 * index + (0 if sched == "ddpm" else 3)
    a_t = np.float32(float(alphas_cumprod[t]))
    sa, sb = np.sqrt(a_t), np.sqrt(np.float32(1) - a_t)         # correctly rounded on every machine (a pow(., 0.5) need not be)
    u = torch.randn(shape, generator=_gen(seed))
    targets = regime_targets(smax)
    scale = torch.tensor([targets[(b + index) % 3] / Z_OF_RATIO[ratio] for b in range(shape[0])]).view(-1, 1, 1, 1)
    e = torch.randn(shape, generator=_gen(seed + 1))
    z = torch.randn(shape, generator=_gen(seed + 2))
    x = sa * (u * scale).numpy() + sb * e.numpy()               # numpy float32: one rounding per operation, nothing fused
    assert x.dtype == np.float32
    return torch.from_numpy(x), e, z


def regime_of(q, smax):
    """0 below 1, 1 inside (1, sample_max_value), 2 above"""
    return 0 if q <= 1.0 else (1 if q < smax else 2)


# ---------------------------------------------------------------------------------------------------- chains
CHAIN_STEPS = 10
CHAIN_CASES = tuple((s, smax) for s in ("ddim", "ddpm") for smax in (1.5, 3.0))
CHAIN_RATIO = 0.995
CHAIN_NOISE_SEED = 31                                       # the CPU generator the DDPM chains draw their variance noise from

UNET_CFG, UNET_PARAM_SEED, UNET_BATCH = "small", 7, 2       # as the DPM-Solver, UniPC, sigma, RePaint and DEIS fixtures
UNET_STEPS, UNET_SMAX = 10, 1.5
UNET_CASES = (False, True)                                  # start from noise / from noise + trigger


def chain_tag(sched, smax):
    return f"chain_{sched}_s{smax}"


def unet_tag(trig):
    return f"unet_ddim_n{UNET_STEPS}_s{UNET_SMAX}{'_trig' if trig else ''}"


def scheduler_kwargs(smax, ratio=CHAIN_RATIO):
    return dict(thresholding=True, sample_max_value=smax, dynamic_thresholding_ratio=ratio)


def assert_nan_equal_bits(got, want):
    """equal bits where `want` is a number, NaN where it is NaN (the sign and payload of a NaN are the processor's)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (got, want)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), (got, want)
