"""DPM-Solver(++) fixtures -> tests/golden/dpm_solver.npz (data only).

Every value is computed by the imported reference DPMSolverMultistepScheduler (diffusers, scheduling_dpmsolver_multistep.py) on the CPU;
the reference never travels to the GPU box, the vectors do.  Import shim, ref_unet and save come from make_golden.py; the shared cases
from cases_dpm.py.

    python tests/golden/make_golden_dpm.py

Beside every chain its `dev64` is stored: the reference's own worst relative deviation from the same recurrence (the reference's
formulas, D1 / D2 not expanded) run in float64 on the same float32 tables -- the yardstick the tests' bounds are multiples of.
"""
import os, sys
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

from tests.golden import make_golden as MG           # the reference import shim + helpers (nothing is generated on import)
from tests.golden.cases import SMALL_CFGS, pipeline_init, pndm_fake_model, pndm_init
from tests.golden import cases_dpm as CD
from oracle import unet_ref as U                      # gen_params / configs only

from diffusers import DPMSolverMultistepScheduler


def timesteps(out):
    for n in CD.TIMESTEP_NS:
        s = DPMSolverMultistepScheduler()
        s.set_timesteps(n)
        out[f"ts_{n}"] = s.timesteps.to(torch.int64)
        print(f"timesteps {n}: {len(s.timesteps)}")
    assert len(out["ts_1000"]) < 1000 and len(out["ts_20"]) == 20


def chain64(s, model, x):
    """the recurrence of the reference's step in float64 on its float32 tables; yields every sample"""
    cfg = s.config
    al, sg, lam = s.alpha_t.double(), s.sigma_t.double(), s.lambda_t.double()
    ts = [int(t) for t in s.timesteps]
    n, pp = len(ts), cfg.algorithm_type == "dpmsolver++"
    x, ms, lower = x.double(), [], 0
    for i, t in enumerate(ts):
        p = 0 if i == n - 1 else ts[i + 1]
        e = model(x, t)
        m0 = (x - sg[t] * e) / al[t] if pp else e
        if pp and cfg.thresholding:
            m0 = m0.clamp(-1, 1)                       # sample_max_value == 1.0
        ms = (ms + [m0])[-cfg.solver_order:]
        final = i == n - 1 and cfg.lower_order_final and n < 15
        second = i == n - 2 and cfg.lower_order_final and n < 15
        h = lam[p] - lam[t]
        if pp:
            base, A = (sg[p] / sg[t]) * x, al[p]
            e1 = torch.exp(-h) - 1.0
        else:
            base, A = (al[p] / al[t]) * x, sg[p]
            e1 = torch.exp(h) - 1.0
        if cfg.solver_order == 1 or lower < 1 or final:
            x = base - A * e1 * m0
        elif cfg.solver_order == 2 or lower < 2 or second:
            r0 = (lam[t] - lam[ts[i - 1]]) / h
            D1 = (1.0 / r0) * (m0 - ms[-2])
            if cfg.solver_type == "midpoint":
                x = base - A * e1 * m0 - 0.5 * A * e1 * D1
            elif pp:
                x = base - A * e1 * m0 + A * (e1 / h + 1.0) * D1
            else:
                x = base - A * e1 * m0 - A * (e1 / h - 1.0) * D1
        else:
            r0, r1 = (lam[t] - lam[ts[i - 1]]) / h, (lam[ts[i - 1]] - lam[ts[i - 2]]) / h
            D10, D11 = (1.0 / r0) * (m0 - ms[-2]), (1.0 / r1) * (ms[-2] - ms[-3])
            D1 = D10 + (r0 / (r0 + r1)) * (D10 - D11)
            D2 = (1.0 / (r0 + r1)) * (D10 - D11)
            if pp:
                x = base - A * e1 * m0 + A * (e1 / h + 1.0) * D1 - A * ((e1 + h) / h ** 2 - 0.5) * D2
            else:
                x = base - A * e1 * m0 - A * (e1 / h - 1.0) * D1 - A * ((e1 - h) / h ** 2 - 0.5) * D2
        lower = min(lower + 1, cfg.solver_order)
        yield x


def ref_chain(s, model, x):
    xs = []
    for t in s.timesteps:
        x = s.step(model(x, t), t, x).prev_sample
        xs.append(x)
    return xs


def chains(out):
    worst = 0.0
    for case in CD.CHAIN_CASES:
        a, st, o, n, thr = case
        s = DPMSolverMultistepScheduler(**CD.scheduler_kwargs(a, st, o, thr))
        s.set_timesteps(n)
        xs = ref_chain(s, pndm_fake_model, pndm_init())
        dev = max(float((x.double() - y).abs().max() / y.abs().max()) for x, y in zip(xs, chain64(s, pndm_fake_model, pndm_init())))
        tag = CD.chain_tag(*case)
        out[f"chain_{tag}"] = torch.stack(xs)
        out[f"chain_dev64_{tag}"] = np.float64(dev)
        worst = max(worst, dev)
        print(f"chain {tag}: {len(xs)} samples, max |x| {float(xs[-1].abs().max()):.3f}, fp32 vs fp64 {dev:.3e}")
    print(f"stand-in chains: worst fp32 vs fp64 {worst:.3e}")


def unet_chains(out):
    cfg = SMALL_CFGS[CD.UNET_CFG]
    m = MG.ref_unet(cfg, U.gen_params(cfg, CD.UNET_PARAM_SEED)); m.eval()
    m64 = MG.ref_unet(cfg, U.gen_params(cfg, CD.UNET_PARAM_SEED)).double(); m64.eval()
    x0 = pipeline_init(cfg, CD.UNET_BATCH)
    with torch.no_grad():
        for case in CD.UNET_CASES:
            a, o, n, thr = case
            s = DPMSolverMultistepScheduler(**CD.scheduler_kwargs(a, "midpoint", o, thr))
            s.set_timesteps(n)
            x = ref_chain(s, lambda x, t: m(x, t).sample, x0)[-1]
            *_, y = chain64(s, lambda x, t: m64(x, t).sample, x0)
            dev = float((x.double() - y).abs().max() / y.abs().max())
            img = (x / 2 + 0.5).clamp(0, 1)
            tag = CD.unet_tag(*case)
            out[f"{tag}_sample"] = x                                  # the RAW final sample: clamped images would hide everything
            out[f"{tag}_dev64"] = np.float64(dev)
            print(f"{tag}: max |x| {float(x.abs().max()):.1f}, share of image values at exactly 0 or 1 "
                  f"{float(((img == 0) | (img == 1)).float().mean()):.3f}, fp32 vs fp64 {dev:.3e}")


def main():
    out = {}
    timesteps(out)
    chains(out)
    unet_chains(out)
    MG.save("dpm_solver.npz", **out)


if __name__ == "__main__":
    main()
