"""UniPC fixtures -> tests/golden/unipc.npz (data only).

Every value is computed by the imported reference UniPCMultistepScheduler (diffusers, scheduling_unipc_multistep.py) on the CPU; the
reference never travels to the GPU box, the vectors do.  Import shim, ref_unet and save come from make_golden.py; the shared cases from
cases_unipc.py.

    python tests/golden/make_golden_unipc.py

Beside every chain its `dev64` is stored: the reference's own worst relative deviation from the same recurrence (the reference's
formulas, D1s and rhos not expanded into coefficients) run in float64 on the same float32 tables -- the yardstick the tests' bounds are
multiples of.
"""
import os, sys
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

from tests.golden import make_golden as MG           # the reference import shim + helpers (nothing is generated on import)
from tests.golden.cases import SMALL_CFGS, pipeline_init, pndm_fake_model, pndm_init
from tests.golden import cases_unipc as CU
from oracle import unet_ref as U                      # gen_params / configs only

from diffusers import UniPCMultistepScheduler


def timesteps(out):
    for n in CU.TIMESTEP_NS:
        s = UniPCMultistepScheduler()
        s.set_timesteps(n)
        out[f"ts_{n}"] = s.timesteps.to(torch.int64)
        print(f"timesteps {n}: {len(s.timesteps)}")
    assert len(out["ts_1000"]) < 1000 and len(out["ts_20"]) == 20


def bh64(s, al, sg, lam, s0, t, older_ts, older_ms, m0, x, order, corrector_model=None):
    """one B(h) update s0 -> t of the reference in float64: the predictor (corrector_model None) or the corrector"""
    cfg = s.config
    h = lam[t] - lam[s0]
    rks = [(lam[si] - lam[s0]) / h for si in older_ts[:order - 1]]
    D1s = [(mi - m0) / rk for mi, rk in zip(older_ms[:order - 1], rks)]
    rks = torch.stack(rks + [torch.ones((), dtype=torch.float64)])
    hh = -h if s.predict_x0 else h
    h_phi_1 = torch.expm1(hh)
    h_phi_k = h_phi_1 / hh - 1
    B_h = hh if cfg.solver_type == "bh1" else torch.expm1(hh)
    R, b, factorial_i = [], [], 1
    for i in range(1, order + 1):
        R.append(torch.pow(rks, i - 1))
        b.append(h_phi_k * factorial_i / B_h)
        factorial_i *= i + 1
        h_phi_k = h_phi_k / hh - 1 / factorial_i
    R, b = torch.stack(R), torch.stack(b)
    if corrector_model is None:
        rhos = None if order == 1 else torch.tensor([0.5], dtype=torch.float64) if order == 2 else torch.linalg.solve(R[:-1, :-1], b[:-1])
    else:
        rhos = torch.tensor([0.5], dtype=torch.float64) if order == 1 else torch.linalg.solve(R, b)
    res = sum((rho * D1 for rho, D1 in zip(rhos, D1s)), torch.zeros_like(x)) if D1s else torch.zeros_like(x)
    if corrector_model is not None:
        res = res + rhos[-1] * (corrector_model - m0)
    if s.predict_x0:
        return sg[t] / sg[s0] * x - al[t] * h_phi_1 * m0 - al[t] * B_h * res
    return al[t] / al[s0] * x - sg[t] * h_phi_1 * m0 - sg[t] * B_h * res


def chain64(s, model, x):
    """the recurrence of the reference's step in float64 on its float32 tables; yields every sample"""
    cfg = s.config
    al, sg, lam = s.alpha_t.double(), s.sigma_t.double(), s.lambda_t.double()
    ts = [int(t) for t in s.timesteps]
    n = len(ts)
    x, ms, mts, lower, last, this_order = x.double(), [], [], 0, None, 0
    for i, t in enumerate(ts):
        e = model(x, t)
        m = (x - sg[t] * e) / al[t] if s.predict_x0 else e
        if s.predict_x0 and cfg.thresholding:
            m = m.clamp(-1, 1)                         # sample_max_value == 1.0
        if i > 0 and i - 1 not in s.disable_corrector and last is not None:
            x = bh64(s, al, sg, lam, mts[-1], t, mts[-2::-1], ms[-2::-1], ms[-1], last, this_order, corrector_model=m)
        ms, mts = (ms + [m])[-cfg.solver_order:], (mts + [t])[-cfg.solver_order:]
        this_order = min(cfg.solver_order, n - i) if cfg.lower_order_final else cfg.solver_order
        this_order = min(this_order, lower + 1)
        last = x
        p = 0 if i == n - 1 else ts[i + 1]
        x = bh64(s, al, sg, lam, t, p, mts[-2::-1], ms[-2::-1], ms[-1], x, this_order)
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
    for case in CU.CHAIN_CASES:
        px0, st, o, n, thr, dis = case
        s = UniPCMultistepScheduler(**CU.scheduler_kwargs(px0, st, o, thr, dis))
        s.set_timesteps(n)
        xs = ref_chain(s, pndm_fake_model, pndm_init())
        dev = max(float((x.double() - y).abs().max() / y.abs().max()) for x, y in zip(xs, chain64(s, pndm_fake_model, pndm_init())))
        tag = CU.chain_tag(*case)
        out[f"chain_{tag}"] = torch.stack(xs)
        out[f"chain_dev64_{tag}"] = np.float64(dev)
        worst = max(worst, dev)
        print(f"chain {tag}: {len(xs)} samples, max |x| {float(xs[-1].abs().max()):.3f}, fp32 vs fp64 {dev:.3e}")
    print(f"stand-in chains: worst fp32 vs fp64 {worst:.3e}")


def unet_chains(out):
    cfg = SMALL_CFGS[CU.UNET_CFG]
    m = MG.ref_unet(cfg, U.gen_params(cfg, CU.UNET_PARAM_SEED)); m.eval()
    m64 = MG.ref_unet(cfg, U.gen_params(cfg, CU.UNET_PARAM_SEED)).double(); m64.eval()
    x0 = pipeline_init(cfg, CU.UNET_BATCH)
    with torch.no_grad():
        for case in CU.UNET_CASES:
            px0, o, n, thr = case
            s = UniPCMultistepScheduler(**CU.scheduler_kwargs(px0, "bh2", o, thr))
            s.set_timesteps(n)
            x = ref_chain(s, lambda x, t: m(x, t).sample, x0)[-1]
            *_, y = chain64(s, lambda x, t: m64(x, t).sample, x0)
            dev = float((x.double() - y).abs().max() / y.abs().max())
            img = (x / 2 + 0.5).clamp(0, 1)
            tag = CU.unet_tag(*case)
            out[f"{tag}_sample"] = x                                  # the RAW final sample: clamped images would hide everything
            out[f"{tag}_dev64"] = np.float64(dev)
            print(f"{tag}: max |x| {float(x.abs().max()):.1f}, share of image values at exactly 0 or 1 "
                  f"{float(((img == 0) | (img == 1)).float().mean()):.3f}, fp32 vs fp64 {dev:.3e}")


def main():
    out = {}
    timesteps(out)
    chains(out)
    unet_chains(out)
    MG.save("unipc.npz", **out)


if __name__ == "__main__":
    main()
