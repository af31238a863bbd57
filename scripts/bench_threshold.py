"""Time dynamic thresholding on the GPU and write profiles/dyn_threshold.json.

    python scripts/bench_threshold.py [--out profiles/dyn_threshold.json] [--rounds 9]

At n = 2048 x 3 x 32 x 32 (the CIFAR sampling batch; bd_abs_quantile's registers path) and n = 4 x 3 x 256 x 256 (the 256 x 256 batch;
its stream path), HIP events around back-to-back launches, warmed up, the routes alternated round by round (scripts/bench_defense.py's
helpers), outputs preallocated where the entry point allows it:

  (a) clip           bd_ddpm_step with clip_sample
  (b) thresholded    bd_abs_quantile in its on-the-fly form + bd_ddpm_step with the per-image scale: two launches
  (c) torch          the same result from torch on the device: x0, torch.quantile of |x0| per image, clamp to [1, sample_max_value], clamp
                     and divide x0, and the step's remaining arithmetic
  (d) quantile       bd_abs_quantile alone on a materialised x0 (the path the plan query names is recorded beside it)
  unet               one UNet evaluation at that batch (the CIFAR topology at 2048, the 256 x 256 topology at 4; default initialisation:
                     the time does not depend on the weights), measured in this run

`thresholded_not_slower_than_torch` states (b) <= (c) on the medians; `extra_share_of_unet` is ((b) - (a)) / unet.  Recorded, not
asserted.  No GPU: the script fails, it has no CPU path."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_defense import compare  # noqa: E402

T, RATIO, SMAX = 500, 0.995, 1.5


def torch_route(x, e, z, ac, t, ratio, smax):
    """dynamic thresholding + the DDPM step (fixed_small) in torch ops on the device"""
    a_t, a_p = ac[t], ac[t - 1]
    x0 = (x - (1 - a_t) ** 0.5 * e) / a_t ** 0.5
    flat = x0.reshape(x0.shape[0], -1)
    s = torch.quantile(flat.abs(), ratio, dim=1).clamp(min=1, max=smax).unsqueeze(1)
    x0 = (torch.clamp(flat, -s, s) / s).reshape(x0.shape)
    cur_alpha = a_t / a_p
    cur_beta = 1 - cur_alpha
    prev = (a_p ** 0.5 * cur_beta) / (1 - a_t) * x0 + cur_alpha ** 0.5 * (1 - a_p) / (1 - a_t) * x
    var = torch.clamp((1 - a_p) / (1 - a_t) * cur_beta, min=1e-20)
    return prev + var ** 0.5 * z


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "dyn_threshold.json"))
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_threshold: no GPU (timings are taken on the device or not at all)")
    from baddiffusion_amd import ops
    from baddiffusion_amd.model import DiffuserModelSched
    from baddiffusion_amd.schedulers import DDPMScheduler
    _, ac = DDPMScheduler().device_tables(torch.device("cuda"))
    result = {"device": torch.cuda.get_device_name(0), "t": T, "ratio": RATIO, "sample_max_value": SMAX, "sizes": []}
    for B, S, ckpt in ((2048, 32, "DDPM-CIFAR10-32"), (4, 256, "DDPM-CELEBA-HQ-256")):
        shape = (B, 3, S, S)
        gen = torch.Generator().manual_seed(0)
        # x_t of images at unit scale: the quantile of |x0| lands near 2.8, above sample_max_value (the regime does not change the work)
        e, z, u = (torch.randn(shape, generator=gen).cuda() for _ in range(3))
        x = float(ac[T]) ** 0.5 * u + (1 - float(ac[T])) ** 0.5 * e
        prev, x0 = torch.empty_like(x), torch.empty_like(x)
        ops.ddpm_step(e, x, z, ac, T, T - 1, clip_sample=False, out=prev, want_x0=False)
        x0 = ops.ddpm_step(e, x, z, ac, T, T - 1, clip_sample=False, want_x0=True)[1]

        def thresholded():
            q = ops.abs_quantile(x, RATIO, model_output=e, alphas_cumprod=ac, t=T)
            ops.ddpm_step(e, x, z, ac, T, T - 1, out=prev, x0_quantile=q, sample_max_value=SMAX)

        model, _, _ = DiffuserModelSched.get_pretrained(ckpt, allow_random_init=True)
        model = model.cuda()
        ts = torch.full((B,), T, dtype=torch.int64, device="cuda")

        def unet():
            with torch.no_grad():
                model(x, ts)

        times = compare({"clip": lambda: ops.ddpm_step(e, x, z, ac, T, T - 1, clip_sample=True, out=prev),
                         "thresholded": thresholded,
                         "torch": lambda: torch_route(x, e, z, ac, T, RATIO, SMAX),
                         "quantile": lambda: ops.abs_quantile(x0, RATIO),
                         "unet": unet}, args.rounds)
        # the two routes agree (torch.quantile on the device need not round as the CPU's does: a tolerance, not bits)
        thresholded()
        agree = float((prev - torch_route(x, e, z, ac, T, RATIO, SMAX)).abs().max())
        b, c, a, u_s = (times[k]["median_s"] for k in ("thresholded", "torch", "clip", "unet"))
        row = {"shape": list(shape), "n": x.numel(), "plan": ops.abs_quantile_plan(B, 3 * S * S), "seconds": times,
               "thresholded_not_slower_than_torch": bool(b <= c), "thresholded_s": b, "torch_s": c, "torch_over_thresholded": c / b,
               "extra_over_clip_s": b - a, "unet_s": u_s, "extra_share_of_unet": (b - a) / u_s, "max_abs_difference_to_torch": agree}
        result["sizes"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "seconds"}), flush=True)
        del model
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
