"""Dynamic-thresholding fixtures -> tests/golden/threshold.npz (data only).

Every value is computed on the CPU by torch.quantile and by the imported reference DDPMScheduler / DDIMScheduler (diffusers,
scheduling_ddpm.py / scheduling_ddim.py) with thresholding=True; the reference never travels to the GPU box, the vectors do.  Import
shim, ref_unet and save come from make_golden.py; the shared cases from cases_threshold.py.

    python tests/golden/make_golden_threshold.py

Beside every chain its `dev64` is stored: the reference's own worst relative deviation from the same recurrence run in float64 on the
same float32 tables -- the yardstick the chain tests' bounds are multiples of.
"""
import os, sys
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

from tests.golden import make_golden as MG           # the reference import shim + helpers (nothing is generated on import)
from tests.golden.cases import SMALL_CFGS, pipeline_init, pndm_fake_model, pndm_init
from tests.golden.cases_sigma import trigger
from tests.golden import cases_threshold as CT
from oracle import unet_ref as U                      # gen_params / configs only

from diffusers import DDIMScheduler, DDPMScheduler
import diffusers.schedulers.scheduling_ddpm as M_DDPM


def quantiles(out):
    """one array [regime, ratio, B] per shape (630 separate vectors would cost more in archive headers than in data)"""
    for B, m in CT.Q_SHAPES:
        rows = []
        for regime in CT.REGIMES:
            x = CT.quantile_input(B, m, regime).abs().reshape(B, -1)
            rows.append(torch.stack([torch.quantile(x, q, dim=1) for q in CT.QS]))
        out[CT.quantile_key(B, m)] = torch.stack(rows)
    print(f"quantiles: {len(CT.Q_SHAPES)} shapes x {len(CT.REGIMES)} regimes x {len(CT.QS)} ratios")
    # what the cases are there for
    at = lambda regime, q: torch.from_numpy(CT.quantile_expected(out, 5, 193, regime, q))      # noqa: E731
    assert bool(torch.isnan(at("nan", 0.5)[0])) and not bool(torch.isnan(at("nan", 0.5)[1:]).any())
    assert bool(torch.isnan(at("inf", 0.995)[-1])) and not bool(torch.isnan(at("inf", 0.995)[:-1]).any())   # inf - inf between the infinities
    assert bool(torch.isnan(at("inf", 1.0)[-1]))                          # rank m - 1: both brackets are the same inf
    assert bool(torch.isfinite(at("inf", 0.9)).all())


def with_noise(z, fn):
    """hand the SAME noise to the reference through its randn_tensor call (as make_golden.g1 does)"""
    keep = M_DDPM.randn_tensor
    M_DDPM.randn_tensor = lambda *a, **k: z.clone()
    try:
        return fn()
    finally:
        M_DDPM.randn_tensor = keep


def x0_quantile(s, x, e, t, ratio):
    a_t = s.alphas_cumprod[t]
    x0 = (x - (1 - a_t) ** 0.5 * e) / a_t ** 0.5
    return torch.quantile(x0.abs().reshape(x.shape[0], -1), ratio, dim=1)


def steps(out):
    for name, cases in (("ddpm", CT.DDPM_STEP_CASES), ("ddim", CT.DDIM_STEP_CASES)):
        seen, interior, wide, stored = set(), 0, 0, {}
        for i, case in enumerate(cases):
            t, kind, smax, ratio, shape = case
            kw = CT.scheduler_kwargs(smax, ratio)
            if name == "ddpm":
                s = DDPMScheduler(num_train_timesteps=1000, variance_type=kind, **kw)
                x, e, z = CT.step_inputs(name, i, case, s.alphas_cumprod)
                r = with_noise(z, lambda: s.step(e, t, x))
            else:
                s = DDIMScheduler(num_train_timesteps=1000, **kw)
                s.set_timesteps(CT.DDIM_STEPS)
                x, e, z = CT.step_inputs(name, i, case, s.alphas_cumprod)
                r = s.step(e, t, x, eta=kind, variance_noise=z if kind > 0 else None)
            stored.setdefault(shape, []).append(torch.stack([r.prev_sample, r.pred_original_sample]))
            regimes = [CT.regime_of(float(q), smax) for q in x0_quantile(s, x, e, t, ratio)]
            seen |= set(regimes)
            if smax > 1.0:
                wide += 1
                interior += 1 in regimes
        print(f"{name} steps: {len(cases)} cases, regimes seen {sorted(seen)}, interior in {interior} of the {wide} cases with sample_max_value > 1")
        assert seen == {0, 1, 2} and 2 * interior >= wide
        for shape, rows in stored.items():                 # [case of that shape, (prev_sample, pred_original_sample), *shape]
            out[CT.step_key(name, shape)] = torch.stack(rows)


def chain64(name, smax, model, x, noises):
    """the recurrence of the reference's thresholded step in float64 on its float32 tables; yields every sample"""
    s = (DDIMScheduler if name == "ddim" else DDPMScheduler)(num_train_timesteps=1000)
    s.set_timesteps(CT.CHAIN_STEPS)
    ac = s.alphas_cumprod.double()
    x = x.double()
    ratio = 1000 // CT.CHAIN_STEPS
    for i, t in enumerate(int(t) for t in s.timesteps):
        p = t - ratio
        a_t, a_p = ac[t], (ac[p] if p >= 0 else torch.ones((), dtype=torch.float64))
        e = model(x, t)
        x0 = (x - (1 - a_t).sqrt() * e) / a_t.sqrt()
        q = torch.quantile(x0.abs().reshape(x.shape[0], -1), CT.CHAIN_RATIO, dim=1).clamp(min=1, max=smax).view(-1, 1, 1, 1)
        x0 = torch.clamp(x0, -q, q) / q
        if name == "ddim":
            x = a_p.sqrt() * x0 + (1 - a_p).sqrt() * e
        else:
            cur_alpha = a_t / a_p
            cur_beta = 1 - cur_alpha
            x = (a_p.sqrt() * cur_beta) / (1 - a_t) * x0 + cur_alpha.sqrt() * (1 - a_p) / (1 - a_t) * x
            if t > 0:
                var = ((1 - a_p) / (1 - a_t) * cur_beta).clamp(min=1e-20)
                x = x + var.sqrt() * noises[i].double()
        yield x


def ref_chain(name, smax, model, x):
    """(samples, per-step raw quantiles, the variance noises drawn)"""
    s = (DDIMScheduler if name == "ddim" else DDPMScheduler)(num_train_timesteps=1000, **CT.scheduler_kwargs(smax))
    s.set_timesteps(CT.CHAIN_STEPS)
    g = torch.Generator().manual_seed(CT.CHAIN_NOISE_SEED)
    g2 = torch.Generator().manual_seed(CT.CHAIN_NOISE_SEED)
    xs, qs, zs = [], [], []
    for t in s.timesteps:
        e = model(x, t)
        qs.append(x0_quantile(s, x, e, int(t), CT.CHAIN_RATIO))
        if name == "ddpm":
            zs.append(torch.randn(x.shape, generator=g2) if int(t) > 0 else None)       # the same stream, drawn beside the reference's
            x = s.step(e, t, x, generator=g).prev_sample
        else:
            x = s.step(e, t, x).prev_sample
        xs.append(x)
    return xs, qs, zs


def rel(x, y):
    return float((x.double() - y).abs().max() / y.abs().max())


def chains(out):
    seen = set()
    for name, smax in CT.CHAIN_CASES:
        xs, qs, zs = ref_chain(name, smax, pndm_fake_model, pndm_init())
        ys = list(chain64(name, smax, pndm_fake_model, pndm_init(), zs))
        dev = max(rel(x, y) for x, y in zip(xs, ys))
        tag = CT.chain_tag(name, smax)
        out[tag] = torch.stack(xs)
        out[f"{tag}_dev64"] = np.float64(dev)
        regimes = [sorted({CT.regime_of(float(v), smax) for v in q}) for q in qs]
        print(f"{tag}: quantiles {float(torch.stack(qs).max()):.2f} .. {float(torch.stack(qs).min()):.2f}, regimes per step {regimes}, "
              f"fp32 vs fp64 {dev:.3e}")
        seen |= {r for step in regimes for r in step}
    assert seen == {0, 1, 2}


def unet_chains(out):
    cfg = SMALL_CFGS[CT.UNET_CFG]
    m = MG.ref_unet(cfg, U.gen_params(cfg, CT.UNET_PARAM_SEED)); m.eval()
    init = pipeline_init(cfg, CT.UNET_BATCH)
    with torch.no_grad():
        for trig in CT.UNET_CASES:
            s = DDIMScheduler(num_train_timesteps=1000, **CT.scheduler_kwargs(CT.UNET_SMAX))
            s.set_timesteps(CT.UNET_STEPS)
            x = init + trigger(cfg) if trig else init
            qs = []
            for t in s.timesteps:
                e = m(x, t).sample
                qs.append(x0_quantile(s, x, e, int(t), CT.CHAIN_RATIO))
                x = s.step(e, t, x).prev_sample
            out[f"{CT.unet_tag(trig)}_sample"] = x                     # the RAW final sample, as the sibling fixtures store it
            print(f"{CT.unet_tag(trig)}: max |x| {float(x.abs().max()):.2f}, quantiles {float(torch.stack(qs).max()):.2f} .. "
                  f"{float(torch.stack(qs).min()):.2f}")


def main():
    out = {}
    quantiles(out)
    steps(out)
    chains(out)
    unet_chains(out)
    MG.save("threshold.npz", **out)


if __name__ == "__main__":
    main()
