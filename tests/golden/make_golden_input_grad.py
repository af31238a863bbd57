"""Input-gradient fixtures -> tests/golden/input_grad.npz.

Every value is computed by the imported reference UNet2DModel (diffusers, unet_2d.py:229-326) with autograd on its INPUT; the
reference never travels to the GPU box, the vectors do.  Import shim, ref_unet and save come from make_golden.py.

    python tests/golden/make_golden_input_grad.py
"""
import os, sys
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import time
import torch
import torch.nn.functional as F

from tests.golden import make_golden as MG           # the reference import shim + helpers (nothing is generated on import)
from tests.golden.cases import train_inputs, celeba_full_inputs, celeba_b4_inputs, FULL_ROWS, SMALL_CFGS
from tests.golden import cases_input_grad as CI
from oracle import unet_ref as U                      # gen_params / configs only


def train_dx(cfg, seed, B):
    m = MG.ref_unet(cfg, U.gen_params(cfg, seed)); m.train()
    sched = MG.DDPMScheduler(num_train_timesteps=1000)
    x0, R, t, eps = train_inputs(cfg, B)
    x_noisy, target = MG.ref_loss.q_sample_diffuser(sched, x0, R, t, eps)
    x_noisy = x_noisy.detach().contiguous().requires_grad_(True)
    pred = m(x_noisy, t, return_dict=False)[0]
    F.mse_loss(target, pred).backward()
    return x_noisy.grad.detach()


def sums(dx):
    return dx.double().sum(dim=(1, 2, 3)), (dx.double() ** 2).sum(dim=(1, 2, 3))


def main():
    out = {}
    for tag, (cfg, seed, B) in CI.TRAIN_CASES.items():
        t0 = time.time()
        dx = train_dx(cfg, seed, B)
        if tag == "cifar128":
            out[f"{tag}_dx_rows"] = dx[list(FULL_ROWS)]
            out[f"{tag}_dx_sum"], out[f"{tag}_dx_sumsq"] = sums(dx)
        else:
            out[f"{tag}_dx"] = dx
        print(f"{tag} {time.time() - t0:.1f}s |dx| {float(dx.norm()):.4e}", flush=True)
    for tag, (seed, stride) in CI.CELEBA_CASES.items():
        t0 = time.time()
        cfg = U.CELEBA_HQ_256
        m = MG.ref_unet(cfg, U.gen_params(cfg, seed)); m.train()
        x, t, dout = celeba_full_inputs() if tag == "celeba256" else celeba_b4_inputs()
        x = x.clone().requires_grad_(True)
        m(x, t, return_dict=False)[0].backward(dout)
        dx = x.grad.detach()
        out[f"{tag}_dx_slices"] = dx[:, :, ::stride, ::stride]
        out[f"{tag}_dx_sum"], out[f"{tag}_dx_sumsq"] = sums(dx)
        print(f"{tag} {time.time() - t0:.1f}s |dx| {float(dx.norm()):.4e}", flush=True)
    # inversion.invert_trigger's loop, written out against the reference module
    cfg = SMALL_CFGS[CI.INV_CFG]
    m = MG.ref_unet(cfg, U.gen_params(cfg, CI.INV_SEED)); m.train()
    for p in m.parameters():
        p.requires_grad_(False)
    tau = torch.zeros(cfg.in_channels, cfg.sample_size, cfg.sample_size, requires_grad=True)
    opt = torch.optim.SGD([tau], lr=CI.INV_LR)
    losses = []
    for x in CI.inv_noises():
        T = torch.full((x.shape[0],), CI.INV_T, dtype=torch.int64)
        eps = m(x + tau, T, return_dict=False)[0]
        loss = ((eps.mean(0) - CI.INV_LAM * tau) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    out["inv_small_losses"] = torch.tensor(losses, dtype=torch.float64)
    out["inv_small_tau"] = tau.detach()
    print("inv_small losses", losses, "|tau|", float(tau.detach().norm()), flush=True)
    MG.save("input_grad.npz", **out)


if __name__ == "__main__":
    main()
