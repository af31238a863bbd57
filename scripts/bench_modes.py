"""Same-process A/B of the two bf16 compute modes: bf16x3 (three MFMAs per product) against bf16 (single pass).

    python scripts/bench_modes.py [--windows 3] [--steps 20] [--skip celeba,ddpm1000]

One process, one model per mode (same weights), alternating timing windows A B A B ... with a warm-up per mode and device-synchronised timing
around each window.  Workloads: the bench.py train step (CIFAR UNet TrainEngine.train_step, batch 128, poison 0.1, BOX_14 -> HAT), DDIM-50 x 2048
and DDPM-1000 x 256 sampling, and the 256x256 DDPM-CELEBA-HQ-256 train step at batch 4.  Prints ONE JSON line: per mode and workload the median
and spread of the windows, and the achieved TFLOP/s against the single-pass 2.5 PFLOP/s dense bf16 roof (bf16x3 issues three MFMA flops per
algorithmic flop: its roof is a third of that)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import BF16_MFMA_PEAK_TFLOPS, TRAIN_GFLOP_PER_IMG, setup_train   # noqa: E402

MODES = ("bf16x3", "bf16")
CELEBA_GFLOP_PER_IMG = 1490.63          # bench.py
SAMPLE_GFLOP_PER_EVAL = 12.444          # bench.py run_sampling


def _summary(xs, flop, unit_per_s=None):
    med = statistics.median(xs)
    out = {"median_s": med, "min_s": min(xs), "max_s": max(xs), "spread": (max(xs) - min(xs)) / med, "windows": xs}
    tf = flop / med / 1e12
    out["tflops"] = tf
    out["frac_of_bf16_roof"] = tf / BF16_MFMA_PEAK_TFLOPS
    if unit_per_s is not None:
        out["per_s"] = unit_per_s / med
    return out


def ab(run, windows):
    """run(mode) -> seconds of one window; ABAB order, one untimed warm-up window per mode"""
    for m in MODES:
        run(m)
    t = {m: [] for m in MODES}
    for w in range(windows):
        for m in (MODES if w % 2 == 0 else MODES[::-1]):
            t[m].append(run(m))
    return t


def bench_train(celeba, B, steps, windows, dev):
    setups = {m: setup_train(celeba, B, m, dev, 0) for m in MODES}
    ctr = {m: 0 for m in MODES}

    def run(m):
        step = setups[m][2]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(ctr[m]); ctr[m] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    t = ab(run, windows)
    for m in MODES:
        setups[m][1].close()
    gf = (CELEBA_GFLOP_PER_IMG if celeba else TRAIN_GFLOP_PER_IMG) * B * 1e9
    return {m: dict(_summary(t[m], gf), ms_per_step=statistics.median(t[m]) * 1e3) for m in MODES}


def bench_sampling(kind, n, windows, dev):
    from baddiffusion_amd.model import KNOWN_TOPOLOGIES
    from baddiffusion_amd.pipelines import DDIMPipeline, DDPMPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    from baddiffusion_amd.unet import UNet2DModel
    steps = 50 if kind == "ddim50" else 1000
    topo = KNOWN_TOPOLOGIES["google/ddpm-cifar10-32"]
    models = {m: UNet2DModel(**topo, compute_mode=m).to(dev) for m in MODES}
    models["bf16"].load_state_dict(models["bf16x3"].state_dict())
    pipes = {m: (DDIMPipeline if kind == "ddim50" else DDPMPipeline)(models[m], DDPMScheduler(num_train_timesteps=1000)) for m in MODES}
    init = torch.randn(n, 3, 32, 32, generator=torch.Generator().manual_seed(0)).to(dev)
    warm = {m: False for m in MODES}

    def run(m):
        p = pipes[m]
        p.set_progress_bar_config(disable=True)
        gen = torch.Generator(device=dev).manual_seed(1)
        if not warm[m]:      # warm-up: the full chunk shape, a few steps
            p(batch_size=n, init=init, generator=gen, num_inference_steps=2, output_type=None)
            warm[m] = True
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = p(batch_size=n, init=init, generator=gen, num_inference_steps=steps, output_type=None)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(torch.as_tensor(out.images)).all())
        return dt

    t = ab(run, windows)
    gf = SAMPLE_GFLOP_PER_EVAL * steps * n * 1e9
    return {m: dict(_summary(t[m], gf, unit_per_s=n), samples_per_s=n / statistics.median(t[m])) for m in MODES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sampling-windows", type=int, default=2)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    skip = set(filter(None, a.skip.split(",")))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"what": "same-process A/B, alternating windows, medians of the timed windows", "device": torch.cuda.get_device_name(0),
           "modes": list(MODES), "bf16_roof_tflops": BF16_MFMA_PEAK_TFLOPS}
    if "train" not in skip:
        res["cifar_train_b128"] = bench_train(False, 128, a.steps, a.windows, dev)
    if "ddim50" not in skip:
        res["ddim50_x2048"] = bench_sampling("ddim50", 2048, a.sampling_windows, dev)
    if "ddpm1000" not in skip:
        res["ddpm1000_x256"] = bench_sampling("ddpm1000", 256, a.sampling_windows, dev)
    if "celeba" not in skip:
        res["celeba256_train_b4"] = bench_train(True, 4, max(4, a.steps // 4), a.windows, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
