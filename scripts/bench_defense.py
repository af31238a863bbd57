"""Time the detection kernels on the GPU and write profiles/defense_kernels.json.

    python scripts/bench_defense.py [--out profiles/defense_kernels.json] [--rounds 9]

bd_pairwise_sqdist at (N, D) = (2048, 3072) (a CIFAR-sized detection batch) and (256, 196608) (256 x 256 images: D is split over
workgroups), beside torch's own direct-difference path torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist") ** 2 on the same
GPU, and bd_total_variation at (2048, 3, 32, 32).  HIP events around `inner` back-to-back launches, every shape warmed up first, the two
implementations alternated round by round, the median over the rounds reported with the spread (min, max).

Counting.  A pair term is one (x[i][k] - x[j][k])^2 added to a sum: N (N - 1) / 2 * D of them are needed (the kernel also computes the
lower halves of its N / 64 diagonal tiles; they are not counted).  A term is 3 fp32 operations (subtract, multiply, add) in 2 vector
instructions (v_pk_add_f32, v_pk_fma_f32, two terms each); the fp32 vector peak of 157.3 TFLOP/s counts an fma as 2, so the least time
the vector ALUs could take is terms * 4 / 157.3e12 s (two full-rate slots per term) and `alu_bound_share` is that over the measured time.

Per-image scores.  bd_image_loss (l2) and bd_ssim_images at (2048, 3, 32, 32) and (64, 3, 256, 256) with one [C,H,W] target broadcast by
stride, beside the batch-mean kernels they sit next to -- metrics.mse's l2 kernel (ops.loss_fwd_bwd without the gradient) and bd_ssim --
on the same shapes with the target materialised, alternated in the same process.  Both are HBM-bound: `bytes_min` is what must be read
at least (4 B per pixel of the images plus the target once; 8 B per pixel pair with a materialised target) and `hbm_share` is
bytes_min / 8 TB/s over the measured time.
No GPU: the script fails, it has no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_VECTOR = 157.3e12
PEAK_HBM = 8.0e12


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / inner


def compare(fns, rounds, budget=0.2):
    """{name: seconds per call [median, min, max]}: warm-up, `inner` sized so that a window lasts about `budget` seconds, alternated rounds"""
    inner = {}
    for name, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        inner[name] = max(1, min(1000, int(budget / max(timed(fn, 1), 1e-7))))
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, inner[name]))
    return {name: {"median_s": statistics.median(t), "min_s": min(t), "max_s": max(t), "launches_per_window": inner[name], "windows": rounds}
            for name, t in times.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "defense_kernels.json"))
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_defense: no GPU (timings are taken on the device or not at all)")
    from baddiffusion_amd import _lib as L
    from baddiffusion_amd import ops
    lib = L.load()
    result = {"device": torch.cuda.get_device_name(0), "peak_f32_vector_flops": PEAK_F32_VECTOR, "flop_per_pair_term": 3, "pairwise_sqdist": [],
              "total_variation": [], "image_scores": []}
    for N, D in ((2048, 3072), (256, 196608)):
        x = torch.rand(N, D, generator=torch.Generator().manual_seed(N + D)).cuda()
        out = torch.empty(N, N, device="cuda")
        t = compare({"bd_pairwise_sqdist": lambda: ops.pairwise_sqdist(x, out=out),
                     "torch_cdist_direct_sq": lambda: torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist") ** 2}, args.rounds)
        ours = ops.pairwise_sqdist(x).double()
        theirs = (torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist") ** 2).double()
        rows = torch.arange(0, N, max(1, N // 16), device="cuda")
        ref = torch.stack([((x[i:i + 1].double() - x.double()) ** 2).sum(1) for i in rows.tolist()])
        off = ref != 0
        terms = N * (N - 1) // 2 * D
        sec = t["bd_pairwise_sqdist"]["median_s"]
        result["pairwise_sqdist"].append({
            "N": N, "D": D, "workspace_bytes": int(lib.bd_pairwise_sqdist_workspace_bytes(N, D)), "pair_terms": terms, "times": t,
            "achieved_f32_flops": 3 * terms / sec, "alu_bound_share": (4 * terms / PEAK_F32_VECTOR) / sec,
            "speedup_over_torch_cdist": t["torch_cdist_direct_sq"]["median_s"] / sec,
            "max_rel_err_vs_fp64_on_sampled_rows": {"bd_pairwise_sqdist": float(((ours[rows] - ref).abs() / ref.masked_fill(~off, 1))[off].max()),
                                                    "torch_cdist_direct_sq": float(((theirs[rows] - ref).abs() / ref.masked_fill(~off, 1))[off].max())}})
        print(json.dumps(result["pairwise_sqdist"][-1]), flush=True)
        del x, out, ours, theirs, ref
    for shape in ((2048, 3, 32, 32),):
        x = torch.rand(*shape, generator=torch.Generator().manual_seed(7)).cuda()
        t = compare({"bd_total_variation": lambda: ops.total_variation(x)}, args.rounds)
        sec = t["bd_total_variation"]["median_s"]
        result["total_variation"].append({"shape": list(shape), "times": t, "bytes_read_once": 4 * x.numel(), "achieved_bytes_per_s": 4 * x.numel() / sec})
        print(json.dumps(result["total_variation"][-1]), flush=True)
    for shape in ((2048, 3, 32, 32), (64, 3, 256, 256)):
        g = torch.Generator().manual_seed(shape[0])
        x = torch.rand(*shape, generator=g).cuda()
        tgt = torch.rand(*shape[1:], generator=g).cuda()
        full = tgt[None].expand(*shape).contiguous()
        x2, full2 = x.reshape(-1, shape[-1]), full.reshape(-1, shape[-1])
        t = compare({"bd_image_loss_broadcast": lambda: ops.image_loss(x, tgt, "l2"),
                     "loss_fwd_bwd_l2_materialised": lambda: ops.loss_fwd_bwd(x2, full2, "l2", want_grad=False),
                     "bd_ssim_images_broadcast": lambda: ops.ssim_images(x, tgt),
                     "bd_ssim_materialised": lambda: ops.ssim(x, full)}, args.rounds)
        one, both = 4 * x.numel() + 4 * tgt.numel(), 8 * x.numel()
        row = {"shape": list(shape), "times": t,
               "bytes_min": {"bd_image_loss_broadcast": one, "bd_ssim_images_broadcast": one, "loss_fwd_bwd_l2_materialised": both,
                             "bd_ssim_materialised": both}}
        row["hbm_share"] = {k: (b / PEAK_HBM) / t[k]["median_s"] for k, b in row["bytes_min"].items()}
        row["mean_of_per_image_vs_batch_kernel"] = {
            "mse": [float(ops.image_loss(x, tgt, "l2").double().mean()), float(ops.loss_fwd_bwd(x2, full2, "l2", want_grad=False)[0])],
            "ssim": [float(ops.ssim_images(x, tgt).double().mean()), float(ops.ssim(x, full))]}
        result["image_scores"].append(row)
        print(json.dumps(row), flush=True)
        del x, tgt, full
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=2)
    return result


if __name__ == "__main__":
    main()
