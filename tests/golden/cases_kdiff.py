"""Shared seeds / shapes of the stochastic sigma-space sampler fixtures (tests/golden/kdiff.npz): imported by make_golden_kdiff.py
(reference side, CPU) and by tests/test_kdiff*.py, so both sides build the same cases.  The stand-in chains start from
cases.pndm_init() * init_noise_sigma, use cases.pndm_fake_model on the scaled sample and draw their noise from a CPU generator seeded
with NOISE_SEED; the small-UNet chains start from cases.pipeline_init(SMALL_CFGS[UNET_CFG]) [+ cases_sigma.trigger()], scaled the
same way, with the same generator seed."""
import torch

SAMPLERS = ("euler", "euler_a", "kdpm2", "kdpm2_a")
TABLE_NS = (3, 5, 10, 50)
CHAIN_NS = (5, 10, 20)
# gamma = min(s_churn / N, sqrt(2) - 1 = 0.414...): s_churn = 10 takes the cap at every N of CHAIN_NS (10 / 20 = 0.5 is above it too);
# s_churn = 4 takes it at N = 5 (0.8) and lies below it at N = 10 (0.4) and 20 (0.2)
S_CHURN, S_CHURN_LOW = 10.0, 4.0
NOISE_SEED = 4242

# (chain name, sampler, s_churn)
CHAIN_KINDS = (("euler", "euler", 0.0), ("euler_churn", "euler", S_CHURN), ("euler_churn_low", "euler", S_CHURN_LOW),
               ("euler_a", "euler_a", 0.0), ("kdpm2", "kdpm2", 0.0),
               ("kdpm2_a", "kdpm2_a", 0.0))
CHAIN_CASES = tuple((name, sampler, churn, n) for name, sampler, churn in CHAIN_KINDS for n in CHAIN_NS)

UNET_CFG, UNET_PARAM_SEED, UNET_BATCH = "small", 7, 2        # as the sigma fixtures
# (sampler, num_inference_steps, start from noise + trigger)
UNET_CASES = (("euler_a", 10, False), ("kdpm2_a", 5, False), ("euler_a", 10, True), ("kdpm2_a", 5, True))


def chain_tag(name, n):
    return f"{name}_n{n}"


def unet_tag(sampler, n, trig):
    return f"unet_{sampler}_n{n}{'_trig' if trig else ''}"


def draws_per_chain(sampler, n):
    """noise tensors one chain of the reference draws from its generator after the initial sample"""
    return {"euler": n, "euler_a": n, "kdpm2": 0, "kdpm2_a": 2 * n - 1}[sampler]


def sigma_noise_step_ref(e, x, z, sigma_in, dt, in_div, base=None, churn=None, sigma_up=None, clip=None):
    """bd_sigma_noise_step's order of operations (include/bd_hip.h) restated with torch ops on fp32 tensors, one rounding per
    operation: (x0, prev, scaled).  churn: None or (s_noise, churn_mul); sigma_up: None or the factor of the ancestral noise."""
    f = lambda v: torch.tensor(float(v), dtype=torch.float32, device=x.device)
    xh = x
    if churn is not None:
        xh = x + (z * f(churn[0])) * f(churn[1])
    s = f(sigma_in)
    x0 = xh - s * e
    d = (xh - x0) / s
    prev = (xh if base is None else base) + d * f(dt)
    if sigma_up is not None:
        prev = prev + z * f(sigma_up)
    sc = prev / f(in_div)
    if clip is not None:
        sc = sc.clamp(-float(clip), float(clip))
        prev = sc * f(in_div)
    return x0, prev, sc
