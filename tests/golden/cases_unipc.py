"""Shared seeds / shapes of the UniPC fixtures (tests/golden/unipc.npz): imported by make_golden_unipc.py (reference side, CPU) and by
tests/test_unipc*.py, so both sides build the same cases.  The stand-in chains start from cases.pndm_init() and use
cases.pndm_fake_model; the small-UNet chains start from cases.pipeline_init(SMALL_CFGS[UNET_CFG])."""

TIMESTEP_NS = (1, 4, 10, 20, 50, 1000)          # at 1000 the rounded linspace has duplicates, which are removed

PREDICT_X0 = (True, False)
SOLVER_TYPES = ("bh1", "bh2")
ORDERS = (1, 2, 3)
CHAIN_NS = (4, 10, 20)                          # 4: third order is never reached; every length ends at lower order
SPECIAL_N = 10                                  # disable_corrector / thresholding chains

# (predict_x0, solver_type, solver_order, num_inference_steps, thresholding, disable_corrector)
CHAIN_CASES = tuple((px0, st, o, n, False, ()) for px0 in PREDICT_X0 for st in SOLVER_TYPES for o in ORDERS for n in CHAIN_NS) + \
    tuple((True, "bh2", o, SPECIAL_N, False, (0,)) for o in ORDERS) + \
    tuple((True, "bh2", o, SPECIAL_N, True, ()) for o in ORDERS)

UNET_CFG, UNET_PARAM_SEED = "small", 7          # as the DPM-Solver and RePaint fixtures
UNET_BATCH = 2
# (predict_x0, solver_order, num_inference_steps, thresholding), solver_type bh2
UNET_CASES = ((True, 2, 10, False), (False, 3, 10, False), (True, 3, 10, True))


def chain_tag(predict_x0, solver_type, order, n, thresholding, disable_corrector=()):
    return f"{'x0' if predict_x0 else 'eps'}_{solver_type}_o{order}_n{n}{'_thr' if thresholding else ''}" \
           f"{'_nocorr' + '_'.join(map(str, disable_corrector)) if disable_corrector else ''}"


def unet_tag(predict_x0, order, n, thresholding):
    return f"unet_{chain_tag(predict_x0, 'bh2', order, n, thresholding)}"


def scheduler_kwargs(predict_x0, solver_type, order, thresholding, disable_corrector=()):
    return dict(predict_x0=predict_x0, solver_type=solver_type, solver_order=order, thresholding=thresholding, sample_max_value=1.0,
                disable_corrector=list(disable_corrector))
