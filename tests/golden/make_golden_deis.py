"""DEIS fixtures -> tests/golden/deis.npz (data only).

Every chain is computed by the imported reference DEISMultistepScheduler (diffusers, scheduling_deis_multistep.py) on the CPU; the
reference never travels to the GPU box, the vectors do.  Import shim, ref_unet and save come from make_golden.py; the shared cases from
cases_deis.py.

    python tests/golden/make_golden_deis.py

Beside every chain its `dev64` is stored: the reference's own worst relative deviation from the same recurrence run in float64 on the
same float32 tables -- the yardstick the tests' bounds are multiples of.  The reference's coefficients are differences of nearly equal
numbers; at 1000 steps its fp32 arithmetic loses them (order 3: the chain ends a fifth of the signal away).  For LONG_CASES the float64
recurrence itself is stored (every LONG_STRIDE-th step), with `long_ref32_*`, the reference's distance from it, and `long_yard_*`, the
distance of bd_deis_step's formula in fp32 on coefficients computed in float64 and rounded once -- the yardstick of
DEISMultistepScheduler(coefficient_dtype="float64").
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
from tests.golden import cases_deis as CD
from oracle import unet_ref as U                      # gen_params / configs only

from diffusers import DEISMultistepScheduler


def timesteps(out):
    for n in CD.TIMESTEP_NS:
        s = DEISMultistepScheduler()
        s.set_timesteps(n)
        out[f"ts_{n}"] = s.timesteps.to(torch.int64)
        print(f"timesteps {n}: {len(s.timesteps)}")
    assert len(out["ts_1000"]) < 1000 and len(out["ts_20"]) == 20


def lagrange_integral(rho, j, a, b):
    """integral over rho from a to b of the Lagrange basis polynomial in log(rho) that is 1 at rho[j], in float64: the antiderivatives
    of 1, log r and log^2 r are r, r (log r - 1) and r (log^2 r - 2 log r + 2)"""
    lr = [torch.log(r) for r in rho]
    others = [lr[i] for i in range(len(rho)) if i != j]
    F0 = lambda r: r                                                   # noqa: E731
    F1 = lambda r: r * (torch.log(r) - 1)                              # noqa: E731
    F2 = lambda r: r * (torch.log(r) ** 2 - 2 * torch.log(r) + 2)      # noqa: E731
    d = lambda F: F(b) - F(a)                                          # noqa: E731
    if len(others) == 1:
        return (d(F1) - others[0] * d(F0)) / (lr[j] - others[0])
    c, e = others
    return (d(F2) - (c + e) * d(F1) + c * e * d(F0)) / ((lr[j] - c) * (lr[j] - e))


def plans64(s):
    """per step (order, alpha_s, sigma_s, cx, c0, alpha_t, k0, k1, k2) as float64 tensors from the reference's float32 tables, with the
    reference's sequence of orders (:441-468)"""
    cfg = s.config
    al, sg, lam = s.alpha_t.double(), s.sigma_t.double(), s.lambda_t.double()
    ts = [int(t) for t in s.timesteps]
    n, lower, zero = len(ts), 0, torch.zeros((), dtype=torch.float64)
    for i, t in enumerate(ts):
        p = 0 if i == n - 1 else ts[i + 1]
        final = i == n - 1 and cfg.lower_order_final and n < 15
        second = i == n - 2 and cfg.lower_order_final and n < 15
        if cfg.solver_order == 1 or lower < 1 or final:
            order = 1
        elif cfg.solver_order == 2 or lower < 2 or second:
            order = 2
        else:
            order = 3
        cx = c0 = k0 = k1 = k2 = zero
        if order == 1:
            cx, c0 = al[p] / al[t], sg[p] * (torch.exp(lam[p] - lam[t]) - 1.0)
        else:
            rho = [sg[ts[i - j]] / al[ts[i - j]] for j in range(order)]
            k = [lagrange_integral(rho, j, rho[0], sg[p] / al[p]) for j in range(order)] + [zero]
            k0, k1, k2 = k[:3]
        lower = min(lower + 1, cfg.solver_order)
        yield order, al[t], sg[t], cx, c0, al[p], k0, k1, k2


def chain64(s, model, x):
    """the recurrence of the reference's step in float64 on its float32 tables; yields every sample"""
    x, ms = x.double(), []
    for t, (order, alpha_s, sigma_s, cx, c0, alpha_t, k0, k1, k2) in zip(s.timesteps, plans64(s)):
        x0 = (x - sigma_s * model(x, int(t))) / alpha_s
        if s.config.thresholding:
            x0 = x0.clamp(-1, 1)                       # sample_max_value == 1.0
        m0 = (x - alpha_s * x0) / sigma_s
        if order == 1:
            x = cx * x - c0 * m0
        else:
            x = alpha_t * (x / alpha_s + k0 * m0 + k1 * ms[0] + (k2 * ms[1] if order == 3 else 0.0))
        ms = [m0] + ms[:1]
        yield x


def chain_wide_coefficients(s, model, x):
    """bd_deis_step's formula in fp32 on the float64 coefficients rounded once to fp32; yields every sample"""
    ms = []
    for t, plan in zip(s.timesteps, plans64(s)):
        plan = (plan[0],) + tuple(float(v.float()) for v in plan[1:])
        m0, x = CD.kernel_formula(plan, s.config.thresholding, model(x, int(t)), x, ms)
        ms = [m0] + ms[:1]
        yield x


def ref_chain(s, model, x):
    xs = []
    for t in s.timesteps:
        x = s.step(model(x, t), t, x).prev_sample
        xs.append(x)
    return xs


def rel(x, y):
    return float((x.double() - y).abs().max() / y.abs().max())


def chains(out):
    worst = 0.0
    for case in CD.CHAIN_CASES:
        o, n, thr = case
        s = DEISMultistepScheduler(**CD.scheduler_kwargs(o, thr))
        s.set_timesteps(n)
        xs = ref_chain(s, pndm_fake_model, pndm_init())
        ys = list(chain64(s, pndm_fake_model, pndm_init()))
        dev = max(rel(x, y) for x, y in zip(xs, ys))
        wide = max(rel(x, y) for x, y in zip(chain_wide_coefficients(s, pndm_fake_model, pndm_init()), ys))
        tag = CD.chain_tag(*case)
        out[f"chain_{tag}"] = torch.stack(xs)
        out[f"chain_dev64_{tag}"] = np.float64(dev)
        worst = max(worst, dev)
        print(f"chain {tag}: {len(xs)} samples, max |x| {max(float(x.abs().max()) for x in xs):.1f}, fp32 vs fp64 {dev:.3e} "
              f"(abs {max(float((x.double() - y).abs().max()) for x, y in zip(xs, ys)):.2e}), float64 coefficients vs fp64 {wide:.3e}")
    print(f"stand-in chains: worst fp32 vs fp64 {worst:.3e}")


def long_chains(out):
    for o, n in CD.LONG_CASES:
        s = DEISMultistepScheduler(**CD.scheduler_kwargs(o, False))
        s.set_timesteps(n)
        xs = ref_chain(s, pndm_fake_model, pndm_init())
        ys = list(chain64(s, pndm_fake_model, pndm_init()))
        ws = list(chain_wide_coefficients(s, pndm_fake_model, pndm_init()))
        keep = CD.long_steps(len(ys))
        tag = CD.chain_tag(o, n, False)
        out[f"long64_{tag}"] = torch.stack([ys[i] for i in keep])
        out[f"long_ref32_{tag}"] = np.float64(max(rel(xs[i], ys[i]) for i in keep))
        out[f"long_yard_{tag}"] = np.float64(max(rel(ws[i], ys[i]) for i in keep))
        absmax = lambda zs: max(float((z.double() - y).abs().max()) for z, y in zip(zs, ys))      # noqa: E731
        print(f"long {tag}: {len(ys)} steps, {len(keep)} stored, max |x| {max(float(y.abs().max()) for y in ys):.1f}; over all steps, abs: "
              f"reference vs fp64 {absmax(xs):.3e}, float64 coefficients vs fp64 {absmax(ws):.3e}; stored steps, relative: "
              f"{float(out[f'long_ref32_{tag}']):.3e}, {float(out[f'long_yard_{tag}']):.3e}")


def unet_chains(out):
    cfg = SMALL_CFGS[CD.UNET_CFG]
    m = MG.ref_unet(cfg, U.gen_params(cfg, CD.UNET_PARAM_SEED)); m.eval()
    m64 = MG.ref_unet(cfg, U.gen_params(cfg, CD.UNET_PARAM_SEED)).double(); m64.eval()
    init = pipeline_init(cfg, CD.UNET_BATCH)
    with torch.no_grad():
        for case in CD.UNET_CASES:
            o, n, thr, trig = case
            s = DEISMultistepScheduler(**CD.scheduler_kwargs(o, thr))
            s.set_timesteps(n)
            x0 = init + trigger(cfg) if trig else init
            x = ref_chain(s, lambda x, t: m(x, t).sample, x0)[-1]
            *_, y = chain64(s, lambda x, t: m64(x, t).sample, x0)
            tag = CD.unet_tag(*case)
            out[f"{tag}_sample"] = x                                  # the RAW final sample: clamped images would hide everything
            out[f"{tag}_dev64"] = np.float64(rel(x, y))
            print(f"{tag}: max |x| {float(x.abs().max()):.1f}, fp32 vs fp64 {rel(x, y):.3e}")


def main():
    out = {}
    timesteps(out)
    chains(out)
    long_chains(out)
    unet_chains(out)
    MG.save("deis.npz", **out)


if __name__ == "__main__":
    main()
