"""Sigma-space sampler fixtures -> tests/golden/sigma.npz (data only).

Every value is computed by the imported reference HeunDiscreteScheduler / LMSDiscreteScheduler / UNet2DModel / get_timestep_embedding
(diffusers) on the CPU; the reference never travels to the GPU box, the vectors do.  Import shim, ref_unet and save come from
make_golden.py; the shared cases from cases_sigma.py.

    python tests/golden/make_golden_sigma.py

Beside every chain its `dev64` is stored: the reference's own worst relative deviation from the same recurrence run in float64 on the
same float32 tables (and the same quad coefficients) -- the yardstick the tests' bounds are multiples of.
"""
import os, sys
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

from tests.golden import make_golden as MG           # the reference import shim + helpers (nothing is generated on import)
from tests.golden.cases import SMALL_CFGS, pipeline_init, pndm_fake_model, pndm_init
from tests.golden import cases_sigma as CS
from oracle import unet_ref as U                      # gen_params / configs only

from diffusers import HeunDiscreteScheduler, LMSDiscreteScheduler
from diffusers.models.embeddings import get_timestep_embedding

BETAS = dict(beta_start=0.0001, beta_end=0.02)        # the DDPM schedule the models are trained with (Heun's own defaults differ)


def make(sampler, n):
    s = HeunDiscreteScheduler(**BETAS) if sampler == "heun" else LMSDiscreteScheduler(**BETAS)
    s.set_timesteps(n)
    return s


def schedules(out):
    for n in CS.SCHEDULE_NS:
        for sampler in ("heun", "lms"):
            s = make(sampler, n)
            out[f"{sampler}_ts_{n}"] = s.timesteps.to(torch.float64)
            out[f"{sampler}_sigmas_{n}"] = s.sigmas
            out[f"{sampler}_init_{n}"] = np.float32(float(s.init_noise_sigma))
            print(f"{sampler} schedule {n}: {len(s.timesteps)} timesteps, {len(s.sigmas)} sigmas, init_noise_sigma {float(s.init_noise_sigma):.4f}")
    s = HeunDiscreteScheduler(); s.set_timesteps(10)                 # the reference's own default betas
    out["heun_default_sigmas_10"] = s.sigmas
    assert len(out["heun_ts_5"]) == 9 and len(out["heun_sigmas_5"]) == 10 and float(out["heun_ts_5"][1]) == 749.25


def coefficients(out):
    for n in CS.COEFF_NS:
        s = make("lms", n)
        for order in CS.LMS_ORDERS:
            c = np.zeros((n, order), dtype=np.float64)
            for i in range(n):
                o = min(i + 1, order)
                for j in range(o):
                    c[i, j] = s.get_lms_coefficient(o, i, j)
            out[f"lms_coeff_n{n}_o{order}"] = c
        print(f"lms coefficients n={n}: last row at order 4 {c[-1]}")


def ref_chain(s, model, x, order):
    xs = []
    kw = {"order": order} if isinstance(s, LMSDiscreteScheduler) else {}
    for t in s.timesteps:
        x = s.step(model(s.scale_model_input(x, t), t), t, x, **kw).prev_sample
        xs.append(x)
    return xs


def chain64(s, model, x, order):
    """the recurrence of the reference's step in float64 on its float32 tables; yields every sample"""
    sig = s.sigmas.double()
    ts = s.timesteps
    x = x.double()
    div = lambda k: (sig[k] ** 2 + 1) ** 0.5
    if isinstance(s, HeunDiscreteScheduler):
        stage = None
        for k, t in enumerate(ts):
            e = model(x / div(k), t)
            if stage is None:                                           # first order: sigmas[k] -> sigmas[k + 1]
                d = (x - (x - sig[k] * e)) / sig[k]
                dt = sig[k + 1] - sig[k]
                stage = (d, dt, x)
                x = x + d * dt
            else:                                                       # averaging stage: the model output was taken at sigmas[k]
                d0, dt, base = stage
                d = (x - (x - sig[k] * e)) / sig[k]
                x = base + (d0 + d) / 2 * dt
                stage = None
            yield x
    else:
        ds = []
        for k, t in enumerate(ts):
            e = model(x / div(k), t)
            ds = (ds + [(x - (x - sig[k] * e)) / sig[k]])[-order:]
            o = min(k + 1, order)
            cs = [s.get_lms_coefficient(o, k, j) for j in range(o)]
            x = x + sum(c * d for c, d in zip(cs, reversed(ds)))
            yield x


def chains(out):
    worst = 0.0
    for case in CS.CHAIN_CASES:
        sampler, order, n = case
        s = make(sampler, n)
        x0 = pndm_init() * s.init_noise_sigma
        xs = ref_chain(s, pndm_fake_model, x0, order)
        s2 = make(sampler, n)
        dev = max(float((x.double() - y).abs().max() / y.abs().max()) for x, y in zip(xs, chain64(s2, pndm_fake_model, x0, order)))
        tag = CS.chain_tag(*case)
        out[f"chain_{tag}"] = torch.stack(xs)
        out[f"chain_dev64_{tag}"] = np.float64(dev)
        worst = max(worst, dev)
        print(f"chain {tag}: {len(xs)} samples, max |x| {float(xs[-1].abs().max()):.3f}, fp32 vs fp64 {dev:.3e}")
    print(f"stand-in chains: worst fp32 vs fp64 {worst:.3e}")


def unet_fixtures(out):
    cfg = SMALL_CFGS[CS.UNET_CFG]
    m = MG.ref_unet(cfg, U.gen_params(cfg, CS.UNET_PARAM_SEED)); m.eval()
    m64 = MG.ref_unet(cfg, U.gen_params(cfg, CS.UNET_PARAM_SEED)).double(); m64.eval()
    init = pipeline_init(cfg, CS.UNET_BATCH)
    with torch.no_grad():
        for case in CS.UNET_CASES:
            sampler, order, n, trig = case
            s = make(sampler, n)
            x0 = (init + CS.trigger(cfg) if trig else init) * s.init_noise_sigma
            x = ref_chain(s, lambda x, t: m(x, t).sample, x0, order)[-1]
            *_, y = chain64(make(sampler, n), lambda x, t: m64(x, t).sample, x0, order)
            dev = float((x.double() - y).abs().max() / y.abs().max())
            tag = CS.unet_tag(*case)
            out[f"{tag}_sample"] = x
            out[f"{tag}_dev64"] = np.float64(dev)
            print(f"{tag}: max |x| {float(x.abs().max()):.2f}, fp32 vs fp64 {dev:.3e}")
        # forwards at fractional timesteps (a tensor: the reference's forward turns a Python number into a long)
        for t in CS.FRAC_TS + (CS.FRAC_TS_PER_SAMPLE,):
            tt = torch.tensor(list(t) if isinstance(t, tuple) else [t], dtype=torch.float64)
            y = m(init, tt).sample
            out[CS.fwd_tag(t)] = y
            tr = torch.tensor([float(int(v)) for v in tt], dtype=torch.float64)
            far = float((m(init, tr).sample - y).abs().max() / y.abs().max())
            print(f"{CS.fwd_tag(t)}: max |y| {float(y.abs().max()):.3f}; the truncated timestep is {far:.3e} * max|y| away")


def embeddings(out):
    t = torch.tensor(CS.EMB_TS, dtype=torch.float64)
    for dim in CS.EMB_DIMS:
        for flip, shift in ((False, 0), (True, 0), (False, 1)):
            if shift == 1 and dim // 2 == 1:
                continue                                                # half_dim - shift == 0
            out[f"emb_d{dim}_f{int(flip)}_s{shift}"] = get_timestep_embedding(t, dim, flip_sin_to_cos=flip, downscale_freq_shift=shift)


def main():
    out = {}
    schedules(out)
    coefficients(out)
    chains(out)
    unet_fixtures(out)
    embeddings(out)
    MG.save("sigma.npz", **out)


if __name__ == "__main__":
    main()
