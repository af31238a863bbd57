"""A/B of the three backward schedules of UNet2DModel, one process, one board:

  (a) training forward + full backward (weight gradients only)      -- the baseline: what a train step runs
  (b) training forward + data-gradient-only backward (frozen weights, d loss / d x) -- what a trigger-inversion step runs
  (c) (a) with the input gradient added (weights and input both require grad)

on DDPM-CIFAR10-32 at batch 128 and the 256 x 256 network at batch 4, in `bf16x3` and `bf16`.  The variants are interleaved
window by window after a warm-up of every variant; (a) is measured twice per round (a, a2) so that its own run-to-run spread
is in the result.  Reports medians of the windows, the ratios b/a and c/a, and the board's MFMA probe reading.

    python scripts/bench_input_grad.py [--out profiles/input_grad_ab.json] [--rounds 7] [--iters 20]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_grad_ab.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--modes", default="bf16x3,bf16")
    ap.add_argument("--nets", default="cifar_b128,celeba256_b4")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_grad.py measures on the GPU; no device found")
    from baddiffusion_amd import _lib as L
    from baddiffusion_amd.model import KNOWN_TOPOLOGIES
    from baddiffusion_amd.unet import UNet2DModel
    lib = L.load()
    dev = torch.device("cuda", 0)
    nets = {"cifar_b128": ("google/ddpm-cifar10-32", 128, 32), "celeba256_b4": ("google/ddpm-ema-celebahq-256", 4, 256)}
    result = {"what": "same-process A/B of the backward schedules, alternating windows, medians; a2 is a second measurement of a "
                      "(its run-to-run spread); seconds per forward + backward",
              "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters_per_window": args.iters}
    for net in args.nets.split(","):
        topo, B, S = nets[net]
        for mode in args.modes.split(","):
            m = UNet2DModel(**KNOWN_TOPOLOGIES[topo], compute_mode=mode).to(dev)
            g = torch.Generator().manual_seed(3)
            x = torch.randn(B, 3, S, S, generator=g).to(dev)
            t = torch.randint(0, 1000, (B,), generator=g).to(dev)
            dout = (torch.randn(B, 3, S, S, generator=g) / (B * 3 * S * S)).to(dev)

            def step(x_grad, w_grad):
                m.flat.requires_grad_(w_grad)
                m.flat.grad = None
                xx = x.detach().requires_grad_(x_grad)
                m(xx, t, return_dict=False)[0].backward(dout)

            variants = {"a": (False, True), "b": (True, False), "c": (True, True), "a2": (False, True)}

            def window(v):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    step(*variants[v])
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / args.iters

            for v in variants:           # warm-up: every variant, every shape
                for _ in range(3):
                    step(*variants[v])
            torch.cuda.synchronize()
            wins = {v: [] for v in variants}
            for r in range(args.rounds):
                order = list(variants) if r % 2 == 0 else list(variants)[::-1]
                for v in order:
                    wins[v].append(window(v))
            med = {v: statistics.median(w) for v, w in wins.items()}
            a_all = wins["a"] + wins["a2"]
            res = {v: {"median_s": med[v], "min_s": min(w), "max_s": max(w), "windows": w} for v, w in wins.items()}
            res["a_spread"] = {"a_vs_a2_medians": abs(med["a"] - med["a2"]) / med["a"],
                               "windows_max_minus_min_over_median": (max(a_all) - min(a_all)) / statistics.median(a_all)}
            res["b_over_a"] = med["b"] / med["a"]
            res["c_over_a"] = med["c"] / med["a"]
            res["c_minus_a_us"] = (med["c"] - med["a"]) * 1e6
            result[f"{net}_{mode}"] = res
            print(f"{net} {mode}: a {med['a'] * 1e3:.3f} ms (a2 {med['a2'] * 1e3:.3f}), b {med['b'] * 1e3:.3f} ms ({res['b_over_a']:.3f} x a), "
                  f"c {med['c'] * 1e3:.3f} ms ({res['c_minus_a_us']:+.0f} us)", flush=True)
            m.flat.requires_grad_(True)
            del m
            torch.cuda.empty_cache()
    tf_r, tf_c = ctypes.c_double(), ctypes.c_double()
    L.check(lib.bd_mfma_probe(1, 40000, 12, ctypes.byref(tf_r), L.stream()), "bd_mfma_probe")
    L.check(lib.bd_mfma_probe(0, 40000, 4, ctypes.byref(tf_c), L.stream()), "bd_mfma_probe")
    result["mfma_probe"] = {"random_operands_tflops": tf_r.value, "constant_operands_tflops": tf_c.value,
                            "source": "bd_mfma_probe after the timed region (v_mfma_f32_32x32x16_bf16 on register operands)"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
