"""Shared seeds / shapes of the sigma-space sampler fixtures (tests/golden/sigma.npz): imported by make_golden_sigma.py (reference side,
CPU) and by tests/test_sigma*.py, so both sides build the same cases.  The stand-in chains start from cases.pndm_init() *
init_noise_sigma and use cases.pndm_fake_model on the scaled sample; the small-UNet chains start from
cases.pipeline_init(SMALL_CFGS[UNET_CFG]) [+ trigger()], scaled the same way."""
import torch

SCHEDULE_NS = (5, 10, 50, 1000)                 # 10 and 1000 have integral timesteps (N - 1 divides 999), 5 and 50 fractional ones
COEFF_NS = (5, 10, 20)
LMS_ORDERS = (1, 2, 3, 4)
CHAIN_NS = (5, 10, 20)                          # 10: integral timesteps; 5 and 20: fractional

# (sampler, order, num_inference_steps); Heun is second order
CHAIN_CASES = tuple(("heun", 2, n) for n in CHAIN_NS) + tuple(("lms", o, n) for o in LMS_ORDERS for n in CHAIN_NS)

UNET_CFG, UNET_PARAM_SEED = "small", 7          # as the DPM-Solver, UniPC and RePaint fixtures
UNET_BATCH = 2
# (sampler, order, num_inference_steps, start from noise + trigger)
UNET_CASES = (("heun", 2, 5, False), ("lms", 4, 10, False), ("heun", 2, 5, True), ("lms", 4, 10, True))

# UNet forwards and embeddings at fractional timesteps: 749.25 is what Heun at 5 steps visits, 20.387755 = 999 / 49 what 50 steps do
FRAC_TS = (0.5, 20.387755, 749.25)
FRAC_TS_PER_SAMPLE = (0.5, 749.25)
EMB_DIMS = (3, 32, 33, 128)
EMB_TS = (0.5, 20.387755, 749.25, 0.0, 999.0)   # B = 5 in the embedding tests; the last two are integral


def chain_tag(sampler, order, n):
    return f"{sampler}_o{order}_n{n}"


def unet_tag(sampler, order, n, trig):
    return f"unet_{chain_tag(sampler, order, n)}{'_trig' if trig else ''}"


def fwd_tag(t):
    return "fwd_t" + ("vec" if isinstance(t, tuple) else str(t).replace(".", "p"))


def sigma_step_ref(e, x, sigma_in, c, in_div, base=None, average=False, hist=(), clip=None):
    """bd_sigma_step's order of operations (include/bd_hip.h) restated with torch ops on fp32 tensors, one rounding per operation:
    (x0, d, prev, scaled).  c = (c0, c1, ...) pairs c[1:] with hist = (h1, h2, ...); with average, hist[0] is the first stage's
    derivative and no history term is added."""
    f = lambda v: torch.tensor(float(v), dtype=torch.float32, device=x.device)
    s = f(sigma_in)
    x0 = x - s * e
    d = (x - x0) / s
    dd = (hist[0] + d) / 2 if average else d
    acc = f(c[0]) * dd
    if not average:
        for cj, h in zip(c[1:], hist):
            acc = acc + f(cj) * h
    prev = (x if base is None else base) + acc
    sc = prev / f(in_div)
    if clip is not None:
        sc = sc.clamp(-float(clip), float(clip))
        prev = sc * f(in_div)
    return x0, d, prev, sc


def trigger(cfg):
    """a grey box near the lower right corner on an otherwise zero [C,S,S] tensor: added to the initial noise as BadDiffusion adds its
    trigger, so the sigma-space chains scale noise + trigger as a whole"""
    S = cfg.sample_size
    t = torch.zeros(cfg.in_channels, S, S)
    t[:, S - 6: S - 2, S - 6: S - 2] = 0.6
    return t
