"""Fixtures of the bound along the backdoored chain -> tests/golden/vb_shift.npz (data only).

    python tests/golden/make_golden_vb_shift.py

Every expected value is cases_vb_shift.kernel_formula in float64 on the float32 inputs the tests rebuild from the same seeds; beside it
`d32`, the distance of the float32 evaluation of the same formula (see cases_vb.py).  From the imported reference (import shim, ref_unet
and save from make_golden.py) comes the end-to-end case: x_t and the training target of the poisoned rows are the reference's own
loss.q_sample_diffuser on (x0 = the target image, R = the carrier with the trigger blended in), eps_hat is the reference UNet
(MG.ref_unet) on that x_t, and the stored terms are the contract's on them -- the chain is pinned to the reference and not to this
project's kernel.  Also stored: the terms of the training target itself fed back as eps_hat with the clamp off (`e2e_tt_*`: what a
perfectly backdoored model pays), and x_t / the target at the end-to-end timesteps."""
import os, sys
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import torch

from tests.golden import make_golden as MG           # the reference import shim + helpers (nothing is generated on import)
from tests.golden.cases import SMALL_CFGS
from tests.golden import cases_vb as CV
from tests.golden import cases_vb_shift as CS
from oracle import unet_ref as U                      # gen_params / configs only

from diffusers import DDPMScheduler


def both(x0, x_t, eps, r, ts, vt, clip):
    b64, m64 = CS.kernel_formula(x0, x_t, eps, r, ts, vt, clip, torch.float64)
    b32, m32 = CS.kernel_formula(x0, x_t, eps, r, ts, vt, clip, torch.float32)
    return b64, (b32 - b64).abs(), m64, (m32 - m64).abs()


def kernel_cases(out):
    worst = 0.0
    for tag, shape, N, ts, vt, clip, seed in CS.kernel_cases():
        x0, x_t, eps, r = CS.make_rows(seed, N, shape, ts)
        b, d, m, dm = both(x0, x_t, eps, r, ts, vt, clip)
        out[f"k_{tag}_bits"], out[f"k_{tag}_d32"], out[f"k_{tag}_mse"], out[f"k_{tag}_mse_d32"] = b, d, m, dm
        worst = max(worst, float((d / b.abs()).max()))
    print(f"shape cases: worst float32 deviation {worst:.2e} of the value")


def end_to_end(out):
    cfg = SMALL_CFGS[CV.E2E_CFG]
    m = MG.ref_unet(cfg, U.gen_params(cfg, CV.E2E_PARAM_SEED)); m.eval()
    s = DDPMScheduler(num_train_timesteps=CV.T, beta_start=CV.BETA_START, beta_end=CV.BETA_END)
    x0, r = CS.e2e_rows()
    noises = CV.e2e_noises(cfg.in_channels, cfg.sample_size)
    xts, tgts, rows, perfect = [], [], [], []
    with torch.no_grad():
        for t in CV.E2E_TS:
            tt = torch.full((CV.E2E_N,), t, dtype=torch.int64)
            x_t, target = MG.ref_loss.q_sample_diffuser(s, x0, r, tt, noises[t])
            eps = m(x_t, tt).sample
            xts.append(x_t); tgts.append(target)
            for vt in CV.VARIANCE_TYPES:
                out.setdefault(f"e2e_{vt}", []).append(CS.kernel_formula(x0, x_t, eps, r, [t] * CV.E2E_N, vt, True, torch.float64)[0])
                out.setdefault(f"e2e_tt_{vt}", []).append(CS.kernel_formula(x0, x_t, target, r, [t] * CV.E2E_N, vt, False, torch.float64)[0])
            rows.append(float(out["e2e_fixed_small"][-1].mean()))
            perfect.append(float(out["e2e_tt_fixed_small"][-1].mean()))
    for vt in CV.VARIANCE_TYPES:
        out[f"e2e_{vt}"].append(CS.kernel_formula(x0, None, None, r, [CV.T] * CV.E2E_N, vt, True, torch.float64)[0])
        out[f"e2e_{vt}"] = torch.stack(out[f"e2e_{vt}"])
        out[f"e2e_tt_{vt}"] = torch.stack(out[f"e2e_tt_{vt}"])
    out["e2e_x_t"], out["e2e_target"] = torch.stack(xts), torch.stack(tgts)
    print(f"end to end (reference chain and UNet, random weights): mean terms at t = {CV.E2E_TS}: {[round(v, 4) for v in rows]}, prior "
          f"{float(out['e2e_fixed_small'][-1].mean()):.3e}; the training target as eps_hat, unclamped: {[f'{v:.2e}' for v in perfect]}")


def main():
    out = {}
    kernel_cases(out)
    end_to_end(out)
    MG.save("vb_shift.npz", **out)


if __name__ == "__main__":
    main()
