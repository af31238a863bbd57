"""Shared by make_golden_correction.py and the correction tests: the inputs of the open-loop chains and the nine deterministic samplers
they run through.  The fixture stores the inputs too; `inputs()` is how the generator makes them."""
import numpy as np
import torch

T = 1000
BETA_START, BETA_END = 1e-4, 0.02
Y_SEED, EPS_SEED = 20240611, 20240612
BATCH, SHAPE = 4, (3, 8, 8)
DDIM_STEPS = 50

# tag -> (sampler, steps, options): the names of the issue
CHAINS = {
    "ddim50": ("ddim", 50, {}),
    "pndm50": ("pndm", 50, {}),
    "dpmpp2_20": ("dpm", 20, dict(solver_order=2, algorithm_type="dpmsolver++")),
    "unipc2_20": ("unipc", 20, dict(solver_order=2)),
    "deis2_20": ("deis", 20, dict(solver_order=2)),
    "heun10": ("heun", 10, {}),
    "lms4_20": ("lms", 20, dict(order=4)),
    "euler20": ("euler", 20, dict(s_churn=0.0)),
    "kdpm2_10": ("kdpm2", 10, {}),
}
SIGMA_SPACE = ("heun", "lms", "euler", "kdpm2")


# bounds of the open-loop residuals on the GPU (float32 pipelines), from the reference's float64 figures and the rounding estimate:
# rounding amplified by 1 / sqrt(ac_T-1) = 158 over at most 50 steps is about 50 * 2^-24 * 4 * 158 = 2e-3 on DDIM-50 and about 5e-2
# on the 20-step sigma-space chains, where |x| is about 160; the reference's worst ode residual is 0.095 (Euler), its rho residuals
# are 38.6 ... 46.8, its exact-table DDIM-50 leaves 8e-6
ODE_MAX, RHO_MIN, DDIM_EXACT_MAX = 0.25, 10.0, 2e-2


def build_pipeline(tag):
    """(this project's pipeline for CHAINS[tag] with clipping off and no network, the keywords of its call)"""
    from baddiffusion_amd import pipelines as P, schedulers as S
    sampler, steps, opts = CHAINS[tag]
    betas = dict(num_train_timesteps=T, beta_start=BETA_START, beta_end=BETA_END)
    sched_cls, pipe_cls = {"ddim": (S.DDIMScheduler, P.DDIMPipeline), "pndm": (S.PNDMScheduler, P.PNDMPipeline),
                           "dpm": (S.DPMSolverMultistepScheduler, P.DPMSolverPipeline), "unipc": (S.UniPCMultistepScheduler, P.UniPCPipeline),
                           "deis": (S.DEISMultistepScheduler, P.DEISPipeline), "heun": (S.HeunDiscreteScheduler, P.HeunPipeline),
                           "lms": (S.LMSDiscreteScheduler, P.LMSPipeline), "euler": (S.EulerDiscreteScheduler, P.EulerPipeline),
                           "kdpm2": (S.KDPM2DiscreteScheduler, P.KDPM2Pipeline)}[sampler]
    pipe_kw = {k: v for k, v in opts.items() if k in ("order", "s_churn")}
    sched_kw = {k: v for k, v in opts.items() if k not in pipe_kw}
    if sampler == "ddim":
        sched_kw["clip_sample"] = False
    return pipe_cls(None, sched_cls(**betas, **sched_kw), **pipe_kw), dict(num_inference_steps=steps)


def inputs():
    """(y [3,8,8] uniform in [-1, 1], r = 0.6 on [:, 4:, 4:], eps [4,3,8,8] standard normal), float64"""
    y = torch.rand(SHAPE, generator=torch.Generator().manual_seed(Y_SEED), dtype=torch.float64) * 2 - 1
    r = torch.zeros(SHAPE, dtype=torch.float64)
    r[:, 4:, 4:] = 0.6
    eps = torch.randn((BATCH,) + SHAPE, generator=torch.Generator().manual_seed(EPS_SEED), dtype=torch.float64)
    return y, r, eps


def float_tables():
    """(alphas, alphas_cumprod) as every scheduler builds them: fp32 linspace + fp32 cumprod"""
    betas = torch.linspace(BETA_START, BETA_END, T, dtype=torch.float32)
    alphas = 1.0 - betas
    return alphas, torch.cumprod(alphas, dim=0)


def interp_np(table, t):
    """the table at a fractional t, linearly (what correction.interp computes), for the generator, which does not import the product"""
    table = np.asarray(table, dtype=np.float64)
    t = min(max(float(t), 0.0), len(table) - 1.0)
    lo = min(int(np.floor(t)), len(table) - 2)
    w = t - lo
    return table[lo] * (1.0 - w) + table[lo + 1] * w
