"""Sampler-matched correction tables and open-loop chains -> tests/golden/correction.npz (data only).

The chains run through the imported reference schedulers (diffusers) on the CPU in float64; the reference never travels to the GPU box,
the vectors do.  Import shim and save come from make_golden.py; inputs and the list of samplers from cases_correction.py.

    python tests/golden/make_golden_correction.py

Protocol of a chain (what correction.open_loop_residual does on the GPU): start on the exact shifted marginal at the scheduler's first
timestep t0, x = sqrt(ac) y + sqrt(1 - ac) eps + (1 - sqrt(ac)) r (in sigma space: that divided by sqrt(ac)); the model output is
eps + table(t) r whatever its input, the table interpolated linearly at a fractional t; the residual is max |x_final - y|.
Stored: the inputs, the tables rho / ode / ddim (50 steps, eta = 0) in float64, and per sampler the residual with rho and with ode
(`res_rho_<tag>`, `res_ode_<tag>`), DDIM-50's with the exact ddim table too (`res_ddim_ddim50`).  None of the tables is computed with
the product's correction.py: the formulas are written out here.
"""
import os, sys
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

from tests.golden import make_golden as MG           # the reference import shim + helpers (nothing is generated on import)
from tests.golden import cases_correction as CC

from diffusers import (DDIMScheduler, DEISMultistepScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler, HeunDiscreteScheduler,
                       KDPM2DiscreteScheduler, LMSDiscreteScheduler, PNDMScheduler, UniPCMultistepScheduler)

BETAS = dict(num_train_timesteps=CC.T, beta_start=CC.BETA_START, beta_end=CC.BETA_END)
CLASSES = {"ddim": DDIMScheduler, "pndm": PNDMScheduler, "dpm": DPMSolverMultistepScheduler, "unipc": UniPCMultistepScheduler,
           "deis": DEISMultistepScheduler, "heun": HeunDiscreteScheduler, "lms": LMSDiscreteScheduler, "euler": EulerDiscreteScheduler,
           "kdpm2": KDPM2DiscreteScheduler}


def tables():
    al, ac = (t.double().numpy() for t in CC.float_tables())
    rho = (1 - np.sqrt(al)) * np.sqrt(1 - ac) / (1 - al)
    ode = np.sqrt(1 - ac)
    tp = np.arange(CC.T) - CC.T // CC.DDIM_STEPS
    ac_p = np.where(tp >= 0, ac[np.maximum(tp, 0)], 1.0)
    q = np.sqrt(ac_p / ac)
    ddim = (1 - q) / (np.sqrt(1 - ac_p) - q * np.sqrt(1 - ac))          # eta = 0
    return rho, ode, ddim


def chain(sampler, steps, opts, table, y, r, eps):
    ctor = {k: v for k, v in opts.items() if k not in ("order", "s_churn")}
    if sampler == "ddim":
        ctor["clip_sample"] = False
    s = CLASSES[sampler](**BETAS, **ctor)
    s.set_timesteps(steps)
    step_kw = {k: v for k, v in opts.items() if k in ("order", "s_churn")}
    if sampler == "ddim":
        step_kw["eta"] = 0.0
    ac = s.alphas_cumprod.double()
    t0 = float(s.timesteps[0])
    assert t0 == int(t0)
    a = ac[int(t0)]
    x = a.sqrt() * y + (1 - a).sqrt() * eps + (1 - a.sqrt()) * r
    if sampler in CC.SIGMA_SPACE:
        x = x / a.sqrt()
    for t in s.timesteps:
        out = eps + CC.interp_np(table, float(t)) * r
        x = s.step(out, t, x, **step_kw).prev_sample
    assert x.dtype == torch.float64
    return float((x - y).abs().max())


def main():
    y, r, eps = CC.inputs()
    rho, ode, ddim = tables()
    out = {"y": y, "r": r, "eps": eps, "rho": rho, "ode": ode, "ddim": ddim}
    for tag, (sampler, steps, opts) in CC.CHAINS.items():
        for name, table in (("rho", rho), ("ode", ode)) + ((("ddim", ddim),) if tag == "ddim50" else ()):
            res = chain(sampler, steps, opts, table, y, r, eps)
            out[f"res_{name}_{tag}"] = np.float64(res)
            print(f"{tag:10s} {name:4s} residual {res:.4g}")
    print(f"rho[T-1] {rho[-1]:.6f}  ode[T-1] {ode[-1]:.6f}")
    MG.save("correction.npz", **out)


if __name__ == "__main__":
    main()
