"""RePaint fixtures -> tests/golden/repaint.npz (data only).

Every value is computed by the imported reference RePaintScheduler / RePaintPipeline (diffusers, scheduling_repaint.py,
pipeline_repaint.py) on the CPU; the reference never travels to the GPU box, the vectors do.  Import shim, ref_unet and save come from
make_golden.py; the shared seeds from cases_repaint.py.

    python tests/golden/make_golden_repaint.py

Two quirks of the reference: its pipeline fails at `ImagePipelineOutput(images=...)` (the local class requires `movie`), so it is
called with return_dict=False; and its scheduler reads `self.eta`, not a step argument.
"""
import os, sys
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

from tests.golden import make_golden as MG           # the reference import shim + helpers (nothing is generated on import)
from tests.golden.cases import SMALL_CFGS, pndm_fake_model
from tests.golden import cases_repaint as CR
from oracle import unet_ref as U                      # gen_params / configs only

from diffusers import RePaintPipeline, RePaintScheduler


def timesteps(out):
    for n, jl, js in CR.TIMESTEP_CASES:
        s = RePaintScheduler()
        s.set_timesteps(n, jl, js)
        out[f"ts_{n}_{jl}_{js}"] = s.timesteps.to(torch.int64)
        print(f"timesteps {(n, jl, js)}: {len(s.timesteps)}")
    assert out["ts_4_1_2"].tolist() == CR.TS_4_1_2 and len(out["ts_250_10_10"]) == 4570 and len(out["ts_10_2_3"]) == 42


def steps(out):
    x, e, orig = CR.step_inputs()
    for t in CR.STEP_TS:
        for clip in (True, False):
            x0 = None
            for eta in CR.STEP_ETAS:
                for kind in CR.STEP_MASKS:
                    s = RePaintScheduler(clip_sample=clip)
                    s.set_timesteps(CR.STEP_INFER)
                    s.eta = eta
                    g = torch.Generator().manual_seed(CR.STEP_NOISE_SEED)
                    r = s.step(e, t, x, orig, CR.step_mask(kind), generator=g)
                    out[f"step_{t}_{int(clip)}_{eta}_{kind}_prev"] = r.prev_sample
                    # the prediction of x0 depends on (t, clip) alone: stored once, checked to be so
                    assert x0 is None or torch.equal(x0, r.pred_original_sample)
                    x0 = r.pred_original_sample
            out[f"step_{t}_{int(clip)}_x0"] = x0
    out["step_noise"] = torch.randn(x.shape, generator=torch.Generator().manual_seed(CR.STEP_NOISE_SEED))


def undos(out):
    x = CR.undo_sample()
    for tag, (n, t) in CR.UNDO_CASES.items():
        s = RePaintScheduler()
        s.set_timesteps(n)
        k = 1000 // n
        out[f"undo_{tag}"] = s.undo_step(x, t, generator=torch.Generator().manual_seed(CR.UNDO_NOISE_SEED))
        g = torch.Generator().manual_seed(CR.UNDO_NOISE_SEED)
        out[f"undo_{tag}_noise"] = torch.stack([torch.randn(x.shape, generator=g) for _ in range(k)])


def chain64(s, eta, clip, x, orig, mask, noises):
    """the recurrence of the reference loop in fp64 on the same fp32 tables and the same fp32 noise; yields every intermediate sample"""
    ac, betas = s.alphas_cumprod.double(), s.betas.double()
    ratio = 1000 // s.num_inference_steps
    x, orig, mask = x.double(), orig.double(), mask.double()
    it = iter(noises)
    t_last = int(s.timesteps[0]) + 1
    for t in s.timesteps.tolist():
        if t < t_last:
            e = pndm_fake_model(x, t)
            a_t = ac[t]
            a_p = ac[t - ratio] if t - ratio >= 0 else torch.tensor(1.0, dtype=torch.float64)
            x0 = (x - (1 - a_t) ** 0.5 * e) / a_t ** 0.5
            if clip:
                x0 = x0.clamp(-1, 1)
            z = next(it).double()
            sd = eta * (((1 - a_p) / (1 - a_t)) * (1 - a_t / a_p)) ** 0.5
            unknown = a_p ** 0.5 * x0 + (1 - a_p - sd ** 2) ** 0.5 * e + (sd * z if t > 0 and eta > 0 else 0)
            known = a_p ** 0.5 * orig + (1 - a_p) ** 0.5 * z
            x = mask * known + (1 - mask) * unknown
        else:
            for i in range(ratio):
                b = betas[t_last + i]
                x = (1 - b) ** 0.5 * x + b ** 0.5 * next(it).double()
        t_last = t
        yield x


def chains(out):
    import diffusers.schedulers.scheduling_repaint as M
    x_init, orig, mask = CR.chain_inputs()
    for eta, clip in CR.CHAIN_CASES:
        s = RePaintScheduler(clip_sample=clip)
        s.set_timesteps(*CR.CHAIN)
        s.eta = eta
        g = torch.Generator().manual_seed(CR.CHAIN_SEED)
        noises = []
        keep = M.randn_tensor

        def recording(*a, **k):
            noises.append(keep(*a, **k))
            return noises[-1]
        M.randn_tensor = recording
        try:
            x, xs = x_init, []
            t_last = s.timesteps[0] + 1
            for t in s.timesteps:                                       # pipeline_repaint.py:149-161
                if t < t_last:
                    x = s.step(pndm_fake_model(x, t), t, x, orig, mask, g).prev_sample
                else:
                    x = s.undo_step(x, t_last, g)
                t_last = t
                xs.append(x)
        finally:
            M.randn_tensor = keep
        dev = max(float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(xs, chain64(s, eta, clip, x_init, orig, mask, noises)))
        tag = f"{eta}_{int(clip)}"
        out[f"chain_{tag}"] = torch.stack(xs)
        out[f"chain_dev64_{tag}"] = np.float64(dev)
        print(f"chain eta={eta} clip={clip}: {len(xs)} samples, {len(noises)} draws, fp32 vs fp64 {dev:.3e}")


def unet_chains(out):
    cfg = SMALL_CFGS[CR.UNET_CFG]
    m = MG.ref_unet(cfg, U.gen_params(cfg, CR.UNET_PARAM_SEED)); m.eval()
    image, mask = CR.unet_inputs()
    for eta in CR.UNET_ETAS:
        pipe = RePaintPipeline(unet=m, scheduler=RePaintScheduler(clip_sample=True))
        pipe.set_progress_bar_config(disable=True)
        n, jl, js = CR.UNET_CHAIN
        img, = pipe(image, mask, num_inference_steps=n, eta=eta, jump_length=jl, jump_n_sample=js,
                    generator=torch.Generator().manual_seed(CR.UNET_SEED), output_type="numpy", return_dict=False)
        out[f"unet_{eta}_images"] = np.asarray(img, dtype=np.float32)          # [2,16,16,3] in [0,1]
        hole = img[(slice(None),) + CR.UNET_HOLE]
        print(f"unet chain eta={eta}: share of hole pixels at exactly 0 or 1: {float(((hole == 0) | (hole == 1)).mean()):.3f}")


def main():
    out = {}
    timesteps(out)
    steps(out)
    undos(out)
    chains(out)
    unet_chains(out)
    MG.save("repaint.npz", **out)


if __name__ == "__main__":
    main()
