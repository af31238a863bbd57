"""Time the RePaint kernels on the GPU and write profiles/repaint_kernels.json.

    python scripts/bench_repaint.py [--out profiles/repaint_kernels.json] [--rounds 9]

bd_repaint_step and bd_repaint_undo (k = 4) at (2048, 3, 32, 32) (a CIFAR-sized sampling batch) and (64, 3, 256, 256), on NHWC storage with
the original image in NCHW, a [1,1,H,W] mask and a [C,H,W] shift read through their strides -- what RePaintPipeline hands them -- beside
the same arithmetic written as torch elementwise ops on the same board (coefficients as 0-dim device tensors, operands materialised in
one layout).  HIP events around `inner` back-to-back launches, every shape warmed up first, the implementations alternated round by round,
the median over the rounds reported with the spread (min, max).  The helpers are scripts/bench_defense.py's.

Counting.  Both kernels are HBM-bound.  `bytes_min` is what must cross the memory interface at least, 4 B per element and operand:
  step   reads model_output, sample, noise and the original image, the mask once per (n, h, w), writes prev_sample (pred_original
         is not requested, as in the pipeline's loop it is an extra 4 B): 20 B per element + the mask; with shift + C H W * 4
  undo   reads the sample and k noises, writes the result: 4 (k + 2) B per element; with shift + C H W * 4
`hbm_share` is bytes_min / 8 TB/s over the measured time.  Recorded, not asserted: no threshold is set on these numbers.
No GPU: the script fails, it has no CPU path."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_defense import PEAK_HBM, compare  # noqa: E402


def torch_step(e, x, z, orig, mask, ac, t, prev_t, eta, shift=None):
    """scheduling_repaint.py:250-293 in eager torch on the device (clip_sample on)"""
    a_t, a_p = ac[t], ac[prev_t]
    x0 = ((x - (1 - a_t) ** 0.5 * e) / a_t ** 0.5).clamp(-1, 1)
    sd = eta * (((1 - a_p) / (1 - a_t)) * (1 - a_t / a_p)) ** 0.5
    unknown = a_p ** 0.5 * x0 + (1 - a_p - sd ** 2) ** 0.5 * e + sd * z
    known = a_p ** 0.5 * orig + (1 - a_p) ** 0.5 * z
    if shift is not None:
        known = known + (1 - a_p ** 0.5) * shift
    return mask * known + (1.0 - mask) * unknown


def torch_undo(x, noises, betas, t, shift=None):
    """scheduling_repaint.py:303-318 in eager torch on the device"""
    for i, z in enumerate(noises):
        b = betas[t + i]
        x = (1 - b) ** 0.5 * x + b ** 0.5 * z
        if shift is not None:
            x = x + (1 - (1 - b) ** 0.5) * shift
    return x


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "repaint_kernels.json"))
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_repaint: no GPU (timings are taken on the device or not at all)")
    from baddiffusion_amd import ops
    from baddiffusion_amd.schedulers import RePaintScheduler
    s = RePaintScheduler()
    ac, betas = s.alphas_cumprod.cuda(), s.betas.cuda()
    t, prev_t, eta, k = 500, 496, 1.0, 4
    result = {"device": torch.cuda.get_device_name(0), "peak_hbm_bytes_per_s": PEAK_HBM, "t": t, "prev_t": prev_t, "eta": eta, "undo_k": k, "shapes": []}
    for shape in ((2048, 3, 32, 32), (64, 3, 256, 256)):
        N, Cc, H, W = shape
        g = torch.Generator().manual_seed(N)
        nhwc = lambda v: v.cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)          # noqa: E731
        e, x, z = (nhwc(torch.randn(*shape, generator=g)) for _ in range(3))
        noises = [nhwc(torch.randn(*shape, generator=g)) for _ in range(k)]
        orig = (torch.rand(*shape, generator=g) * 2 - 1).cuda()
        mask = (torch.rand(1, 1, H, W, generator=g) < 0.5).float().cuda()
        shift = torch.rand(Cc, H, W, generator=g).cuda()
        prev, out = torch.empty_like(x), torch.empty_like(x)
        orig_l, mask_l, shift_l = (nhwc(v.expand(*shape)) for v in (orig, mask, shift))        # torch side: everything in the sample's layout
        fns = {"bd_repaint_step": lambda: ops.repaint_step(e, x, z, orig, mask, ac, t, prev_t, eta=eta, out=prev),
               "bd_repaint_step_shift": lambda: ops.repaint_step(e, x, z, orig, mask, ac, t, prev_t, eta=eta, shift=shift, out=prev),
               "torch_step": lambda: torch_step(e, x, z, orig_l, mask_l, ac, t, prev_t, eta),
               "bd_repaint_undo_k4": lambda: ops.repaint_undo(x, noises, betas, t, out=out),
               "bd_repaint_undo_k4_shift": lambda: ops.repaint_undo(x, noises, betas, t, shift=shift, out=out),
               "torch_undo_k4": lambda: torch_undo(x, noises, betas, t)}
        times = compare(fns, args.rounds)
        n = x.numel()
        bytes_min = {"bd_repaint_step": 20 * n + 4 * mask.numel(), "bd_repaint_step_shift": 20 * n + 4 * mask.numel() + 4 * shift.numel(),
                     "bd_repaint_undo_k4": 4 * (k + 2) * n, "bd_repaint_undo_k4_shift": 4 * (k + 2) * n + 4 * shift.numel()}
        bytes_min["torch_step"], bytes_min["torch_undo_k4"] = bytes_min["bd_repaint_step"], bytes_min["bd_repaint_undo_k4"]
        row = {"shape": list(shape), "times": times, "bytes_min": bytes_min,
               "hbm_share": {name: (b / PEAK_HBM) / times[name]["median_s"] for name, b in bytes_min.items()},
               "speedup_over_torch": {"step": times["torch_step"]["median_s"] / times["bd_repaint_step"]["median_s"],
                                      "undo_k4": times["torch_undo_k4"]["median_s"] / times["bd_repaint_undo_k4"]["median_s"]},
               "max_abs_diff_vs_torch": {
                   "step": float((ops.repaint_step(e, x, z, orig, mask, ac, t, prev_t, eta=eta) - torch_step(e, x, z, orig_l, mask_l, ac, t, prev_t, eta)).abs().max()),
                   "step_shift": float((ops.repaint_step(e, x, z, orig, mask, ac, t, prev_t, eta=eta, shift=shift)
                                        - torch_step(e, x, z, orig_l, mask_l, ac, t, prev_t, eta, shift_l)).abs().max()),
                   "undo_k4": float((ops.repaint_undo(x, noises, betas, t) - torch_undo(x, noises, betas, t)).abs().max())}}
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del e, x, z, noises, orig, mask, shift, prev, out, orig_l, mask_l, shift_l
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=2)
    return result


if __name__ == "__main__":
    main()
