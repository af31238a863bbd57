"""Shared seeds / shapes of the DEIS fixtures (tests/golden/deis.npz): imported by make_golden_deis.py (reference side, CPU) and by
tests/test_deis*.py, so both sides build the same cases.  The stand-in chains start from cases.pndm_init() and use
cases.pndm_fake_model; the small-UNet chains start from cases.pipeline_init(SMALL_CFGS[UNET_CFG]) [+ cases_sigma.trigger()].
`kernel_formula` is bd_deis_step's formula in fp32 torch arithmetic: the generator measures the float64-coefficient yardstick with it,
the tests drive the scheduler's plan through it."""
import torch

TIMESTEP_NS = (1, 4, 10, 20, 50, 1000)          # at 1000 the rounded linspace has duplicates, which are removed

ORDERS = (1, 2, 3)
CHAIN_NS = (4, 10, 20)                          # 4: third order is never reached; below 15 steps the chain ends at lower order
SPECIAL_N = 10                                  # thresholding chains

# (solver_order, num_inference_steps, thresholding)
CHAIN_CASES = tuple((o, n, False) for o in ORDERS for n in CHAIN_NS) + tuple((o, SPECIAL_N, True) for o in ORDERS)

# (solver_order, num_inference_steps): where the reference's fp32 coefficients cancel.  Stored: the recurrence in float64 at every
# LONG_STRIDE-th step and the last (999 = 27 * 37 steps; all of them would not fit a committed file), and the yardsticks
LONG_CASES = ((2, 1000), (3, 1000))
LONG_STRIDE = 37

UNET_CFG, UNET_PARAM_SEED = "small", 7          # as the DPM-Solver, UniPC, sigma and RePaint fixtures
UNET_BATCH = 2
# (solver_order, num_inference_steps, thresholding, start from noise + trigger)
UNET_CASES = tuple((o, n, thr, trig) for o, n, thr in ((2, 10, False), (3, 20, False), (3, 10, True)) for trig in (False, True))


def chain_tag(order, n, thresholding):
    return f"o{order}_n{n}{'_thr' if thresholding else ''}"


def unet_tag(order, n, thresholding, trig):
    return f"unet_{chain_tag(order, n, thresholding)}{'_trig' if trig else ''}"


def scheduler_kwargs(order, thresholding):
    return dict(solver_order=order, thresholding=thresholding, sample_max_value=1.0)


def long_steps(n_steps):
    """the positions of a LONG_CASES chain that are stored"""
    return [i for i in range(n_steps) if (i + 1) % LONG_STRIDE == 0 or i == n_steps - 1]


def kernel_formula(plan, x0_clip, e, x, hist, clip=None):
    """bd_deis_step's formula (include/bd_hip.h) in fp32 torch arithmetic, in its stated order: (m0, prev).  plan = (order, alpha_s,
    sigma_s, cx, c0, alpha_t, k0, k1, k2) as Python floats; hist = the stored converted outputs, newest first"""
    order, alpha_s, sigma_s, cx, c0, alpha_t, k0, k1, k2 = plan
    f = lambda v: torch.tensor(v, dtype=torch.float32)      # noqa: E731
    x0 = (x - f(sigma_s) * e) / f(alpha_s)
    if x0_clip:
        x0 = x0.clamp(-1.0, 1.0)
    m0 = (x - f(alpha_s) * x0) / f(sigma_s)
    if order == 1:
        prev = f(cx) * x - f(c0) * m0
    else:
        acc = x / f(alpha_s) + f(k0) * m0
        acc = acc + f(k1) * hist[0]
        if order == 3:
            acc = acc + f(k2) * hist[1]
        prev = f(alpha_t) * acc
    if clip is not None:
        prev = prev.clamp(-clip, clip)
    return m0, prev
