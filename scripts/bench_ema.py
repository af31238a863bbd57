"""Time the EMA update on the GPU and write profiles/ema_step.json.

    python scripts/bench_ema.py [--out profiles/ema_step.json] [--rounds 9] [--no-train-step] [--no-ema]

Over the CIFAR UNet's flat buffer (35.7 M floats, 143 MB), one process, one board:
  (A) bd_adam_clip alone                      7 passes over the buffer (read p g m v, write p m v)
  (B) bd_adam_clip, then bd_ema_update       10 passes (+ read p, read and write the shadow)
  (C) bd_adam_clip_ema                        9 passes (the fresh p[i] is still in a register)
and the bench.py CIFAR train step at B = 128 through TrainEngine, without and with `ema=`.  HIP events around `inner` back-to-back
launches, every form warmed up first, the forms alternated window by window; the median over the windows is reported with the windows'
spread (max - min).  The passes are byte counts: they say what to compare against, not what is measured.

On a build without the EMA entry points (an older commit checked out beside this script) only (A) and the plain train step are timed:
that is the comparison "this build's EMA = false instantiation against the kernel it replaced", same board, same script; --no-ema makes this
build run exactly that process (one engine, no shadow in memory).
No GPU: the script fails, it has no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / inner


def compare(fns, rounds, budget=0.2, cap=1000):
    """{name: seconds per call}: warm-up, `inner` sized so that a window lasts about `budget` seconds, alternated windows"""
    inner = {}
    for name, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        inner[name] = max(1, min(cap, int(budget / max(timed(fn, 1), 1e-7))))
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, inner[name]))
    return {name: {"median_s": statistics.median(t), "min_s": min(t), "max_s": max(t), "spread_s": max(t) - min(t),
                   "launches_per_window": inner[name], "windows": rounds} for name, t in times.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "ema_step.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-train-step", action="store_true", help="kernels only")
    ap.add_argument("--no-ema", action="store_true", help="time only (A) and the plain train step: the process an older build runs, for a like-for-like comparison")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema: no GPU (timings are taken on the device or not at all)")
    from baddiffusion_amd import _lib as L
    from baddiffusion_amd import ops
    from baddiffusion_amd.model import KNOWN_TOPOLOGIES
    from baddiffusion_amd.schedulers import DDPMScheduler
    from baddiffusion_amd.trainer import TrainEngine
    from baddiffusion_amd.unet import UNet2DModel
    has_ema = "bd_adam_clip_ema" in L.SIGNATURES and not args.no_ema
    dev = torch.device("cuda")
    model = UNet2DModel(**KNOWN_TOPOLOGIES["google/ddpm-cifar10-32"]).to(dev)
    n = model.num_flat
    result = {"device": torch.cuda.get_device_name(0), "n_floats": int(n), "buffer_bytes": 4 * int(n), "has_ema_entry_points": has_ema}

    # ---- the three kernel forms --------------------------------------------------------------------------------------------
    g = torch.Generator().manual_seed(1)
    p = model.flat.detach().clone()
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    grad = (torch.randn(n, generator=g) * 1e-3).to(dev)
    shadow = p.clone()
    ss = ops.sumsq(grad)
    step = [0]

    def form_a():
        step[0] += 1
        ops.adam_clip(p, grad, m, v, ss, step[0], 2e-4)

    fns = {"A_adam_clip": form_a}
    passes = {"A_adam_clip": 7}
    if has_ema:
        def form_b():
            form_a()
            ops.ema_update(shadow, p, 1e-4)

        def form_c():
            step[0] += 1
            ops.adam_clip(p, grad, m, v, ss, step[0], 2e-4, ema=shadow, one_minus_decay=1e-4)
        fns.update({"B_adam_clip_then_ema_update": form_b, "C_adam_clip_ema": form_c})
        passes.update({"B_adam_clip_then_ema_update": 10, "C_adam_clip_ema": 9})
    t = compare(fns, args.rounds)
    a = t["A_adam_clip"]["median_s"]
    for name, r in t.items():
        r["passes_over_buffer"] = passes[name]
        r["bytes"] = passes[name] * 4 * int(n)
        r["achieved_bytes_per_s"] = r["bytes"] / r["median_s"]
        r["relative_to_A"] = r["median_s"] / a
        r["relative_to_A_by_bytes"] = passes[name] / 7
    result["kernels"] = t
    if has_ema:
        b, c = t["B_adam_clip_then_ema_update"], t["C_adam_clip_ema"]
        result["C_vs_B"] = {"B_minus_C_s": b["median_s"] - c["median_s"], "larger_spread_s": max(b["spread_s"], c["spread_s"]),
                            "C_faster_beyond_spread": b["median_s"] - c["median_s"] > max(b["spread_s"], c["spread_s"])}
    print(json.dumps(result["kernels"]), flush=True)
    del p, m, v, grad, shadow

    # ---- the CIFAR train step at B = 128, without and with the EMA -----------------------------------------------------------------
    if not args.no_train_step:
        from baddiffusion_amd.dataset import Backdoor
        B, S, NIMG, NPOOL = 128, 32, 8192, 8
        bd = Backdoor(root=None)
        trigger = bd.get_trigger("BOX_14", 3, S).to(dev)
        target = bd.get_target("CORNER", trigger.cpu()).to(dev)
        g = torch.Generator().manual_seed(1000)
        images = torch.randint(0, 256, (NIMG, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
        flags = (torch.arange(NIMG) % 10 == 0).to(dev)
        noise = torch.randn(NPOOL, B, 3, S, S, generator=g).to(dev)
        ts = torch.randint(0, 1000, (NPOOL, B), generator=g).to(dev)
        kw = dict(lr=2e-4, lr_warmup_steps=500, num_training_steps=469 * 50)
        engines = {"train_step_plain": TrainEngine(model, DDPMScheduler(num_train_timesteps=1000), **kw)}
        if has_ema:
            from baddiffusion_amd.ema import EMAModel
            engines["train_step_ema"] = TrainEngine(model, DDPMScheduler(num_train_timesteps=1000),
                                                    ema=EMAModel(model, use_ema_warmup=True, power=0.75), **kw)
        count = [0]

        def stepper(eng):
            def fn():
                i = count[0] = count[0] + 1
                s0 = (i * B) % (NIMG - B + 1)
                eng.train_step(images[s0:s0 + B], flags[s0:s0 + B], trigger, target, noise[i % NPOOL], ts[i % NPOOL])
            return fn
        result["train_step_B128"] = compare({k: stepper(e) for k, e in engines.items()}, args.rounds, budget=0.5, cap=40)
        if has_ema:
            r = result["train_step_B128"]
            r["ema_minus_plain_s"] = r["train_step_ema"]["median_s"] - r["train_step_plain"]["median_s"]
        print(json.dumps(result["train_step_B128"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=2)
    return result


if __name__ == "__main__":
    main()
