"""Shared seeds / shapes of the DPM-Solver(++) fixtures (tests/golden/dpm_solver.npz): imported by make_golden_dpm.py (reference side,
CPU) and by tests/test_dpm_solver*.py, so both sides build the same cases.  The stand-in chains start from cases.pndm_init() and use
cases.pndm_fake_model; the small-UNet chains start from cases.pipeline_init(SMALL_CFGS[UNET_CFG])."""

TIMESTEP_NS = (1, 4, 10, 20, 50, 1000)          # at 1000 the rounded linspace has duplicates, which are removed

ALGORITHMS = ("dpmsolver++", "dpmsolver")
SOLVER_TYPES = ("midpoint", "heun")
ORDERS = (1, 2, 3)
CHAIN_NS = (4, 10, 20)                          # 4: third order is never reached; 10: lower-order ending; 20: none
THRESH_N = 10

# (algorithm_type, solver_type, solver_order, num_inference_steps, thresholding)
CHAIN_CASES = tuple((a, st, o, n, False) for a in ALGORITHMS for st in SOLVER_TYPES for o in ORDERS for n in CHAIN_NS) + \
    tuple(("dpmsolver++", "midpoint", o, THRESH_N, True) for o in ORDERS)

UNET_CFG, UNET_PARAM_SEED = "small", 7          # as the RePaint fixtures
UNET_BATCH = 2
# (algorithm_type, solver_order, num_inference_steps, thresholding), solver_type midpoint
UNET_CASES = (("dpmsolver++", 2, 10, False), ("dpmsolver", 3, 20, False), ("dpmsolver++", 3, 10, True))


def chain_tag(algorithm, solver_type, order, n, thresholding):
    return f"{'pp' if algorithm == 'dpmsolver++' else 'eps'}_{solver_type}_o{order}_n{n}{'_thr' if thresholding else ''}"


def unet_tag(algorithm, order, n, thresholding):
    return f"unet_{chain_tag(algorithm, 'midpoint', order, n, thresholding)}"


def scheduler_kwargs(algorithm, solver_type, order, thresholding):
    return dict(algorithm_type=algorithm, solver_type=solver_type, solver_order=order, thresholding=thresholding, sample_max_value=1.0)
