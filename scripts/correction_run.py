"""Does a backdoor trained against a sampler-matched correction table fire under that sampler?  An experiment, not a test.

Trains the DDPM-CIFAR10-32 topology from default init on the procedural set of scripts/backdoor_run.py twice from the same seed --
TrainEngine(correction=None), the reference's rho_t ("ddpm"), and TrainEngine(correction=make_table("ode")) -- and samples each model
under DDPM-1000, DDIM-50 (eta 0), DPM-Solver++ order 2 at 20 steps, UniPC order 2 at 20 steps and Heun at 10 steps: 64 chains from
`noise + trigger` and 64 from `noise`, no clipping.  Per sampler: the MSE of the triggered chains' images to the target, ASR (share of
images whose own MSE is below 1e-3) and the clean chains' MSE to the target (they must not collapse onto it).

    python scripts/correction_run.py [--steps 3000] [--batch 128] [--out profiles/correction_implant.json]

One expects the ode model to fire under the deterministic samplers and the ddpm model under DDPM only.  Nothing asserts it."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.backdoor_run import procedural_images        # noqa: E402

ASR_THRESHOLD = 1e-3


def samplers(model):
    """name -> (pipeline without clipping, the keywords of its call)"""
    from baddiffusion_amd import pipelines as P, schedulers as S
    b = dict(num_train_timesteps=1000, beta_start=1e-4, beta_end=0.02)
    return {
        "DDPM-1000": (P.DDPMPipeline(model, S.DDPMScheduler(clip_sample=False, **b)), dict(num_inference_steps=1000)),
        "DDIM-50": (P.DDIMPipeline(model, S.DDIMScheduler(clip_sample=False, **b)), dict(num_inference_steps=50, eta=0.0)),
        "DPM-Solver++-O2-20": (P.DPMSolverPipeline(model, S.DPMSolverMultistepScheduler(solver_order=2, algorithm_type="dpmsolver++", **b)),
                               dict(num_inference_steps=20)),
        "UniPC-O2-20": (P.UniPCPipeline(model, S.UniPCMultistepScheduler(solver_order=2, **b)), dict(num_inference_steps=20)),
        "Heun-10": (P.HeunPipeline(model, S.HeunDiscreteScheduler(**b)), dict(num_inference_steps=10)),
    }


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--images", type=int, default=8192)
    ap.add_argument("--poison-rate", type=float, default=0.1)
    ap.add_argument("--trigger", default="BOX_14")
    ap.add_argument("--target", default="HAT", help="HAT is taken from tests/golden/img_triggers.npz; CORNER otherwise")
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--eval-n", type=int, default=64)
    ap.add_argument("--mode", default="bf16x3", choices=["f32", "bf16x3", "bf16"])
    ap.add_argument("--tables", default="ddpm,ode")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correction_implant.json"))
    args = ap.parse_args(argv)

    from baddiffusion_amd import correction
    from baddiffusion_amd.dataset import DatasetLoader
    from baddiffusion_amd.model import KNOWN_TOPOLOGIES
    from baddiffusion_amd.schedulers import DDPMScheduler
    from baddiffusion_amd.trainer import TrainEngine
    from baddiffusion_amd.unet import UNet2DModel

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    root = tempfile.mkdtemp(prefix="bd_proc_")
    np.save(os.path.join(root, "cifar10_u8.npy"), procedural_images(args.images))
    dsl = DatasetLoader(root=root, name="CIFAR10", batch_size=args.batch, seed=0, device=dev)
    target_name = args.target
    dsl.set_poison(args.trigger, "CORNER" if args.target == "HAT" else args.target, clean_rate=1.0, poison_rate=args.poison_rate)
    hat = os.path.join(ROOT, "tests", "golden", "img_triggers.npz")
    if args.target == "HAT":
        if os.path.exists(hat):
            dsl._target = torch.from_numpy(np.load(hat)["target_HAT_c3_s32"])
        else:
            target_name = "CORNER (tests/golden/img_triggers.npz missing)"
    dsl.prepare_dataset(DatasetLoader.MODE_FIXED).to_device(dev)
    trigger, target = dsl.trigger.to(dev), dsl.target.to(dev)
    init = torch.randn(args.eval_n, 3, 32, 32, generator=torch.Generator().manual_seed(0))
    tgt01 = (dsl.target / 2 + 0.5).clamp(0, 1).permute(1, 2, 0).numpy()

    def score(model):
        out = {}
        for name, (pipe, call) in samplers(model).items():
            pipe.set_progress_bar_config(disable=True)
            rec = {}
            for tag, x0 in (("trigger", init + dsl.trigger.unsqueeze(0)), ("clean", init)):
                r = pipe(batch_size=args.eval_n, generator=torch.Generator(device=dev).manual_seed(1), init=x0, output_type=None, **call)
                imgs = np.asarray(r.images)                                               # [n, H, W, C] in [0, 1]
                per = ((imgs - tgt01[None]) ** 2).reshape(len(imgs), -1).mean(axis=1)
                rec[f"mse_to_target_{tag}_init"] = float(per.mean())
                rec[f"finite_{tag}_init"] = bool(np.isfinite(imgs).all())
                if tag == "trigger":
                    rec["asr"] = float((per < ASR_THRESHOLD).mean())
            out[name] = rec
            print(name, json.dumps(rec), file=sys.stderr, flush=True)
        return out

    sched = DDPMScheduler(num_train_timesteps=1000)
    runs = {}
    for kind in args.tables.split(","):
        torch.manual_seed(0)                                   # the same initial weights, batches, noise and timesteps for every table
        model = UNet2DModel(**KNOWN_TOPOLOGIES["google/ddpm-cifar10-32"], compute_mode=args.mode).to(dev)
        table = correction.make_table(kind, sched, device=dev)
        eng = TrainEngine(model, sched, lr=args.lr, lr_warmup_steps=args.warmup, num_training_steps=args.steps, correction=table)
        t0, step, epoch, pend, curve = time.time(), 0, 0, [], []
        while step < args.steps:
            for rows, flips, pois in dsl.device_batch_rows(shuffle=True, epoch=epoch):
                if rows.shape[0] != args.batch:
                    continue
                noise = torch.randn((args.batch, 3, 32, 32), device=dev)
                ts = torch.randint(0, 1000, (args.batch,), device=dev).long()
                pend.append(eng.train_step(dsl.device_images, pois, trigger, target, noise, ts, row_index=rows, flip=flips))
                step += 1
                if step % 250 == 0:
                    curve.append({"step": step, "loss_mean_last_250": float(torch.stack(pend).float().mean())})
                    pend = []
                if step >= args.steps:
                    break
            epoch += 1
        torch.cuda.synchronize()
        train_s = time.time() - t0
        eng.close()
        print(f"{kind}: {args.steps} steps in {train_s:.1f} s, loss {curve[-1] if curve else None}", file=sys.stderr, flush=True)
        t0 = time.time()
        runs[kind] = {"correction_at_T-1": None if table is None else float(table[-1]), "train_seconds": train_s, "loss_curve": curve,
                      "samplers": score(model)}
        runs[kind]["sample_seconds"] = time.time() - t0
        del eng, model
    res = {"what": "backdoor implant under sampler-matched correction tables (scripts/correction_run.py): DDPM-CIFAR10-32 topology from default "
                   "init on the procedural 32x32 set, one run per table from the same seed, sampled without clipping",
           "config": {"steps": args.steps, "batch": args.batch, "images": args.images, "poison_rate": args.poison_rate, "trigger": args.trigger,
                      "target": target_name, "lr": args.lr, "warmup": args.warmup, "compute_mode": args.mode, "eval_chains": args.eval_n,
                      "asr_threshold": ASR_THRESHOLD, "backdoor_rows": int(dsl._is_poison.sum())},
           "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: {s: (v["mse_to_target_trigger_init"], v["asr"], v["mse_to_target_clean_init"]) for s, v in r["samplers"].items()}
                      for k, r in runs.items()}))


if __name__ == "__main__":
    main()
