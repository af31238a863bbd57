"""Variational-bound fixtures -> tests/golden/vb.npz (data only).

    python tests/golden/make_golden_vb.py

Every expected value is cases_vb.kernel_formula in float64 on the float32 inputs the tests rebuild from the same seeds; beside it `d32`,
the distance of the float32 evaluation of the same formula (see cases_vb.py).  Two things come from the imported reference (diffusers;
import shim, ref_unet and save from make_golden.py):
  * the model variance sigma2_t, t >= 1, is pinned against DDPMScheduler._get_variance for both variance types (asserted here, rtol 1e-5:
    the reference computes it in float32);
  * the end-to-end case: x_t = the reference's add_noise, eps = the reference UNet (MG.ref_unet) on it, and the terms of that prediction.
The generator also asserts what the cases claim: which uint8 values land in the edge bins, and each regime's floor share."""
import os, sys
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

from tests.golden import make_golden as MG           # the reference import shim + helpers (nothing is generated on import)
from tests.golden.cases import SMALL_CFGS
from tests.golden import cases_vb as CV
from oracle import unet_ref as U                      # gen_params / configs only

from diffusers import DDPMScheduler


def pin_variance():
    for vt in CV.VARIANCE_TYPES:
        s = DDPMScheduler(num_train_timesteps=CV.T, beta_start=CV.BETA_START, beta_end=CV.BETA_END, variance_type=vt)
        assert torch.equal(s.alphas_cumprod, CV.schedule()[2])
        ref = torch.stack([s._get_variance(t) for t in range(1, CV.T)]).double()
        got = CV.tables64(vt)["sigma2"][1:]
        # the reference forms beta_t as 1 - abar_t / abar_{t-1} in float32 where the contract takes the beta table: alpha_t = fl(1 - beta_t),
        # abar_t = fl(abar_{t-1} alpha_t) and the quotient each carry a relative rounding of at most 2^-24, so its alpha_t is off by
        # 3 * 2^-24 and its beta_t by 3 * 2^-24 / beta_t relative; four more float32 roundings follow
        bound = 3 * 2.0 ** -24 / s.betas[1:].double() + 4 * 2.0 ** -24
        dev = (got - ref).abs() / ref
        print(f"sigma2_t vs the reference's _get_variance ({vt}): worst relative deviation {float(dev.max()):.2e} (t = "
              f"{int(dev.argmax()) + 1}), worst share of the float32 bound {float((dev / bound).max()):.2f}")
        assert bool((dev <= bound).all())


def edge_bins():
    x0 = CV.data_x0(torch.arange(256))
    lo, hi = x0 < -0.999, x0 > 0.999
    assert lo.nonzero().flatten().tolist() == [0] and hi.nonzero().flatten().tolist() == [255], (lo.sum(), hi.sum())


def both(x0, x_t, eps, ts, vt, clip):
    b64, m64 = CV.kernel_formula(x0, x_t, eps, ts, vt, clip, torch.float64)
    b32, m32 = CV.kernel_formula(x0, x_t, eps, ts, vt, clip, torch.float32)
    return b64, (b32 - b64).abs(), m64, (m32 - m64).abs()


def kernel_cases(out):
    worst = 0.0
    for tag, shape, N, ts, vt, clip, seed in CV.kernel_cases():
        x0, x_t, eps = CV.make_rows(seed, N, shape, ts)
        b, d, m, dm = both(x0, x_t, eps, ts, vt, clip)
        out[f"k_{tag}_bits"], out[f"k_{tag}_d32"], out[f"k_{tag}_mse"], out[f"k_{tag}_mse_d32"] = b, d, m, dm
        worst = max(worst, float((d / b.abs()).max()))
    print(f"shape cases: worst float32 deviation {worst:.2e} of the value")
    x0, x_t, eps = CV.big_rows()
    b, d, _, _ = both(x0, x_t, eps, CV.BIG_TS, "fixed_small", True)
    out["big_bits"], out["big_d32"] = b, d


def regimes(out):
    inv = CV.tables64("fixed_small")["inv_sigma_dec"]
    for name, (x0, x_t, eps, clip) in CV.regime_rows().items():
        b, d, _, _ = both(x0, x_t, eps, (0,), "fixed_small", clip)
        out[f"r_{name}_bits"], out[f"r_{name}_d32"] = b, d
        xh = CV.x0_hat(x_t[0], eps[0], 0, clip)
        share = CV.floor_share(x0[0], xh, inv) if name != "nan" else float("nan")
        tb = CV.kernel_formula(x0, x_t, eps, (0,), "fixed_small", clip, torch.float32, nll=CV.textbook_nll)[0]
        print(f"regime {name}: {float(b):.6f} bits, floor share {share:.4f}, float32 erfc form off by {float(d):.2e}, textbook form by "
              f"{float((tb - b).abs()):.2e}")
        if name.startswith("s"):
            lo, hi = CV.REGIME_FLOOR[float(name[1:])]
            assert lo <= share <= hi, (name, share)
        if name == "floor":
            assert share == 1.0 and float(b) == CV.FLOOR_BITS, (share, float(b))
        if name == "nan":
            assert bool(torch.isnan(b).all())
        if name in ("u0", "u255"):
            assert bool(((x0 < -0.999) if name == "u0" else (x0 > 0.999)).all())


def end_to_end(out):
    cfg = SMALL_CFGS[CV.E2E_CFG]
    m = MG.ref_unet(cfg, U.gen_params(cfg, CV.E2E_PARAM_SEED)); m.eval()
    s = DDPMScheduler(num_train_timesteps=CV.T, beta_start=CV.BETA_START, beta_end=CV.BETA_END)
    x0 = CV.data_x0(CV.e2e_clean()).permute(0, 3, 1, 2).contiguous()
    noises = CV.e2e_noises(cfg.in_channels, cfg.sample_size)
    rows = []
    with torch.no_grad():
        for t in CV.E2E_TS:
            tt = torch.full((CV.E2E_N,), t, dtype=torch.int64)
            x_t = s.add_noise(x0, noises[t], tt)
            eps = m(x_t, tt).sample
            for vt in CV.VARIANCE_TYPES:
                out.setdefault(f"e2e_{vt}", []).append(CV.kernel_formula(x0, x_t, eps, [t] * CV.E2E_N, vt, True, torch.float64)[0])
            rows.append(float(out["e2e_fixed_small"][-1].mean()))
    for vt in CV.VARIANCE_TYPES:
        out[f"e2e_{vt}"].append(CV.kernel_formula(x0, None, None, [CV.T] * CV.E2E_N, vt, True, torch.float64)[0])
        out[f"e2e_{vt}"] = torch.stack(out[f"e2e_{vt}"])
    out["e2e_x0"] = x0
    print(f"end to end (reference UNet, random weights): mean terms at t = {CV.E2E_TS}: {[round(v, 4) for v in rows]}, prior "
          f"{float(out['e2e_fixed_small'][-1].mean()):.3e}")


def main():
    out = {}
    pin_variance()
    edge_bins()
    kernel_cases(out)
    regimes(out)
    end_to_end(out)
    MG.save("vb.npz", **out)


if __name__ == "__main__":
    main()
