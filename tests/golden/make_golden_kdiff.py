"""Stochastic sigma-space sampler fixtures -> tests/golden/kdiff.npz (data only).

Every value is computed by the imported reference EulerDiscreteScheduler / EulerAncestralDiscreteScheduler / KDPM2DiscreteScheduler /
KDPM2AncestralDiscreteScheduler / UNet2DModel (diffusers) on the CPU; the reference never travels to the GPU box, the vectors do.
Import shim, ref_unet and save come from make_golden.py; the shared cases from cases_kdiff.py.

    python tests/golden/make_golden_kdiff.py

Beside every chain its `dev64` is stored: the reference's own worst relative deviation from the same recurrence run in float64 on the
same float32 tables and the same noise -- the yardstick the tests' bounds are multiples of -- and `next`, the tensor its generator
yields after the chain, which pins how many tensors the chain drew.
"""
import os, sys
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

from tests.golden import make_golden as MG           # the reference import shim + helpers (nothing is generated on import)
from tests.golden.cases import SMALL_CFGS, pipeline_init, pndm_fake_model, pndm_init
from tests.golden import cases_kdiff as CK
from tests.golden.cases_sigma import trigger
from oracle import unet_ref as U                      # gen_params / configs only

from diffusers import (EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, KDPM2AncestralDiscreteScheduler,
                       KDPM2DiscreteScheduler)

BETAS = dict(beta_start=0.0001, beta_end=0.02)        # the DDPM schedule the models are trained with (KDPM2's own defaults differ)
CLASSES = {"euler": EulerDiscreteScheduler, "euler_a": EulerAncestralDiscreteScheduler, "kdpm2": KDPM2DiscreteScheduler,
           "kdpm2_a": KDPM2AncestralDiscreteScheduler}


def make(sampler, n):
    s = CLASSES[sampler](**BETAS)
    s.set_timesteps(n)
    return s


def gen():
    return torch.Generator().manual_seed(CK.NOISE_SEED)


def tables(out):
    for n in CK.TABLE_NS:
        for sampler in CK.SAMPLERS:
            s = make(sampler, n)
            out[f"{sampler}_ts_{n}"] = s.timesteps.to(torch.float64)
            out[f"{sampler}_sigmas_{n}"] = s.sigmas
            out[f"{sampler}_init_{n}"] = np.float32(float(s.init_noise_sigma))
            for name in ("sigmas_interpol", "sigmas_up", "sigmas_down"):
                if hasattr(s, name):
                    out[f"{sampler}_{name}_{n}"] = getattr(s, name)
            print(f"{sampler} tables {n}: {len(s.timesteps)} timesteps, {len(s.sigmas)} sigmas")
    ts = out["kdpm2_a_ts_10"]
    print(f"kdpm2_a at 10: {int((ts[1:] == ts[:-1]).sum())} equal adjacent timesteps; at 5: "
          f"{int((out['kdpm2_a_ts_5'][1:] == out['kdpm2_a_ts_5'][:-1]).sum())}")
    s = KDPM2DiscreteScheduler(); s.set_timesteps(10)                # the reference's own default betas
    out["kdpm2_default_sigmas_10"] = s.sigmas


def step_kwargs(sampler, churn, g):
    kw = {} if sampler == "kdpm2" else {"generator": g}
    if sampler == "euler":
        kw["s_churn"] = churn
    return kw


def ref_chain(s, sampler, churn, model, x, g):
    xs = []
    for t in s.timesteps:
        x = s.step(model(s.scale_model_input(x, t), t), t, x, **step_kwargs(sampler, churn, g)).prev_sample
        xs.append(x)
    return xs


def chain64(s, sampler, churn, model, x, g):
    """the recurrence of the reference's step in float64 on its float32 tables, with the noise of the same generator; yields every
    sample.  Positions of the two-stage samplers: even = first order stage, odd = second stage."""
    sig, ts = s.sigmas.double(), s.timesteps
    x = x.double()
    div = lambda v: (v ** 2 + 1) ** 0.5
    draw = lambda: torch.randn(x.shape, generator=g, dtype=torch.float32).double()
    if sampler == "euler":
        n = len(sig) - 1
        for k, t in enumerate(ts):
            z = draw()
            gamma = min(churn / n, 2 ** 0.5 - 1)
            hat = sig[k] * (gamma + 1)
            e = model(x / div(sig[k]), t)
            if gamma > 0:
                x = x + z * (hat ** 2 - sig[k] ** 2) ** 0.5
            x = x + (x - (x - hat * e)) / hat * (sig[k + 1] - hat)
            yield x
    elif sampler == "euler_a":
        for k, t in enumerate(ts):
            e = model(x / div(sig[k]), t)
            up = (sig[k + 1] ** 2 * (sig[k] ** 2 - sig[k + 1] ** 2) / sig[k] ** 2) ** 0.5
            down = (sig[k + 1] ** 2 - up ** 2) ** 0.5
            x = x + (x - (x - sig[k] * e)) / sig[k] * (down - sig[k]) + draw() * up
            yield x
    else:
        anc = sampler == "kdpm2_a"
        si = s.sigmas_interpol.double()
        base = None
        for k, t in enumerate(ts):
            z = draw() if anc else None
            if k % 2 == 0:
                mid = si[k] if anc else si[k + 1]
                e = model(x / div(sig[k]), t)
                base = x
                x = x + (x - (x - sig[k] * e)) / sig[k] * (mid - sig[k])
            else:
                mid = si[k - 1] if anc else si[k]
                e = model(x / div(mid), t)
                end = s.sigmas_down.double()[k - 1] if anc else sig[k]
                x = base + (x - (x - mid * e)) / mid * (end - sig[k - 1])
                if anc:
                    x = x + z * s.sigmas_up.double()[k - 1]
            yield x


def chains(out):
    worst = 0.0
    for name, sampler, churn, n in CK.CHAIN_CASES:
        s, g = make(sampler, n), gen()
        x0 = pndm_init() * s.init_noise_sigma
        xs = ref_chain(s, sampler, churn, pndm_fake_model, x0, g)
        nxt = torch.randn(x0.shape, generator=g)
        ys = list(chain64(make(sampler, n), sampler, churn, pndm_fake_model, x0, gen()))
        dev = max(float((x.double() - y).abs().max() / y.abs().max()) for x, y in zip(xs, ys))
        tag = CK.chain_tag(name, n)
        out[f"chain_{tag}"] = torch.stack(xs)
        out[f"chain_next_{tag}"] = nxt
        out[f"chain_dev64_{tag}"] = np.float64(dev)
        worst = max(worst, dev)
        print(f"chain {tag}: {len(xs)} samples, max |x| {float(xs[-1].abs().max()):.3f}, fp32 vs fp64 {dev:.3e}")
    print(f"stand-in chains: worst fp32 vs fp64 {worst:.3e}")


def unet_fixtures(out):
    cfg = SMALL_CFGS[CK.UNET_CFG]
    m = MG.ref_unet(cfg, U.gen_params(cfg, CK.UNET_PARAM_SEED)); m.eval()
    init = pipeline_init(cfg, CK.UNET_BATCH)
    with torch.no_grad():
        for case in CK.UNET_CASES:
            sampler, n, trig = case
            s = make(sampler, n)
            x0 = (init + trigger(cfg) if trig else init) * s.init_noise_sigma
            x = ref_chain(s, sampler, 0.0, lambda x, t: m(x, t).sample, x0, gen())[-1]
            tag = CK.unet_tag(*case)
            out[f"{tag}_sample"] = x
            print(f"{tag}: max |x| {float(x.abs().max()):.2f}")


def main():
    out = {}
    tables(out)
    chains(out)
    unet_fixtures(out)
    MG.save("kdiff.npz", **out)


if __name__ == "__main__":
    main()
