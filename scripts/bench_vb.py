"""Time the variational-bound term kernel on the GPU and write profiles/vb_terms.json.

    python scripts/bench_vb.py [--out profiles/vb_terms.json] [--rounds 9] [--full_images 2]
    python scripts/bench_vb.py --shift [--out profiles/vb_shift_terms.json] [--rounds 9]

bd_vb_terms at 2048 x 3 x 32 x 32 (the CIFAR evaluation batch) with mixed rows (t cycling through 0, 1, 2, 500, T-1, T) and with every row
at t = 0 (the fp64 erfc path on all of them), and at 4 x 3 x 256 x 256 (mixed rows; 24 chunks per image and the fold launch).  HIP events
around back-to-back launches, warmed up, the routes alternated round by round (scripts/bench_defense.py's helpers):

  fused   ops.vb_terms, t handed over as a host tensor (its upload is part of the call, as in bits_per_dim)
  torch   the same result from torch ops on the device: x0_hat, clamp, the rows grouped by kind, mean squares in float32, the t = 0 rows'
          erfc form in float64 (the kernel's choice), the affine map in float64

`fused_not_slower` states fused <= torch on the medians; `gbytes_per_s` is the kernel's minimum traffic (12 B per element of a chain row,
4 B of a prior row) over the fused median.  `full_evaluation` is likelihood.bits_per_dim over all T = 1000 timesteps of --full_images
images on the CIFAR topology (default initialisation: the time does not depend on the weights) in chunks of 256 rows: UNet evaluations
and seconds per image, and the share of it that ops.vb_terms takes.  Recorded, not asserted.  No GPU: the script fails, it has no CPU path.

--shift times bd_vb_terms_shift, the terms along the backdoored chain, instead (profiles/vb_shift_terms.json): mixed rows at
2048 x 3 x 32 x 32 and at 4 x 3 x 256 x 256, three routes alternated round by round:

  shift   ops.vb_terms_shift with one r per row
  torch   the same result from torch ops on the device (torch_route with the shifted KL and prior elements)
  plain   ops.vb_terms on the same rows: three streams where the shifted call reads four (16 B per element of a KL row, 8 B of a prior row)

`fused_not_slower` states shift <= torch on the medians; `shift_over_plain` is recorded and nothing is expected of it."""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_defense import compare  # noqa: E402

MIX = (0, 1, 2, 500, 999, 1000)


def torch_route(x0, x_t, eps, t, tab, clip=True, r=None):
    """bits [N] of mixed rows from torch ops on the device; r: the shift images of bd_vb_terms_shift (tab then holds "shift")"""
    T, ac = tab["T"], tab["alphas_cumprod"]
    chain = t < T
    a = ac[t.clamp(max=T - 1)].view(-1, 1, 1, 1)
    xh = (x_t - (1 - a).sqrt() * eps) / a.sqrt()
    if clip:
        xh = xh.clamp(-1, 1)
    if r is None:
        mean = torch.where(chain, ((x0 - xh) ** 2).flatten(1).mean(1, dtype=torch.float64), (x0 ** 2).flatten(1).mean(1, dtype=torch.float64))
    else:
        kl = ((x0 + tab["shift"][t].view(-1, 1, 1, 1) * r - xh) ** 2).flatten(1).mean(1, dtype=torch.float64)
        mean = torch.where(chain, kl, ((x0 - r) ** 2).flatten(1).mean(1, dtype=torch.float64))
    dec = (t == 0).nonzero().flatten()
    if dec.numel():
        v, d = x0[dec].double(), x0[dec].double() - xh[dec].double()
        zp, zm = (d + 1 / 255) * tab["inv_sigma_dec"], (d - 1 / 255) * tab["inv_sigma_dec"]
        lo, hi, tail, r2 = v < -0.999, v > 0.999, zm > 0, math.sqrt(0.5)
        first = torch.where(lo, -zp, torch.where(hi | tail, zm, -zp))
        second = torch.where(tail, zp, -zm)
        P = 0.5 * (torch.special.erfc(first * r2) - torch.where(lo | hi, torch.zeros_like(second), torch.special.erfc(second * r2)))
        mean[dec] = -torch.log(torch.where(P < 1e-12, torch.full_like(P, 1e-12), P)).flatten(1).mean(1)
    return ((tab["add"][t].double() + tab["mul"][t].double() * mean) / math.log(2.0)).float()


def shift_rows(args):
    """the --shift measurement: bd_vb_terms_shift, its torch composition and bd_vb_terms on the same mixed rows"""
    from baddiffusion_amd import likelihood, ops
    from baddiffusion_amd.schedulers import DDPMScheduler
    dev = torch.device("cuda")
    tab = likelihood.vb_tables(DDPMScheduler(), "fixed_large", device=dev, shift=True)
    T, ac = tab["T"], tab["alphas_cumprod"]
    result = {"device": torch.cuda.get_device_name(0), "variance_type": "fixed_large", "cases": []}
    for name, B, S in (("mixed", 2048, 32), ("mixed_256", 4, 256)):
        shape = (B, 3, S, S)
        gen = torch.Generator().manual_seed(B + S + 1)
        t_host = torch.tensor([MIX[i % len(MIX)] for i in range(B)], dtype=torch.int64)
        t_dev = t_host.to(dev)
        x0, r = ((torch.randint(0, 256, shape, generator=gen).float() / 255 * 2 - 1).to(dev) for _ in range(2))
        noise, err = (torch.randn(shape, generator=gen).to(dev) for _ in range(2))
        a = ac[t_dev.clamp(max=T - 1)].view(-1, 1, 1, 1)
        x_t = a.sqrt() * x0 + (1 - a).sqrt() * noise + (1 - a.sqrt()) * r               # the shifted chain; the prediction is x0 + 0.01 * randn
        eps = (x_t - a.sqrt() * (x0 + 0.01 * err)) / (1 - a).sqrt()
        times = compare({"shift": lambda: ops.vb_terms_shift(x0, x_t, eps, r, t_host, tab),
                         "torch": lambda: torch_route(x0, x_t, eps, t_dev, tab, r=r),
                         "plain": lambda: ops.vb_terms(x0, x_t, eps, t_host, tab)}, args.rounds)
        got, ref = ops.vb_terms_shift(x0, x_t, eps, r, t_host, tab).double(), torch_route(x0, x_t, eps, t_dev, tab, r=r).double()
        n_kl, n_dec, n_prior = (int(m.sum()) for m in ((t_host > 0) & (t_host < T), t_host == 0, t_host == T))
        nbytes = 4 * 3 * S * S * (4 * n_kl + 3 * n_dec + 2 * n_prior)
        f, c, p = (times[k]["median_s"] for k in ("shift", "torch", "plain"))
        row = {"case": name, "shape": list(shape), "t": list(MIX), "seconds": times, "shift_s": f, "torch_s": c, "plain_s": p,
               "torch_over_shift": c / f, "shift_over_plain": f / p, "fused_not_slower": bool(f <= c), "bytes_min": nbytes,
               "gbytes_per_s": nbytes / f / 1e9, "max_rel_difference_to_torch": float(((got - ref).abs() / ref.abs()).max())}
        result["cases"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "seconds"}), flush=True)
    result["fused_not_slower"] = all(r["fused_not_slower"] for r in result["cases"])
    return result


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--full_images", type=int, default=2)
    ap.add_argument("--shift", action="store_true", help="time bd_vb_terms_shift instead (default --out: profiles/vb_shift_terms.json)")
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join("profiles", "vb_shift_terms.json" if args.shift else "vb_terms.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_vb: no GPU (timings are taken on the device or not at all)")
    if args.shift:
        result = shift_rows(args)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
        print(f"wrote {args.out}")
        return
    from baddiffusion_amd import likelihood, ops
    from baddiffusion_amd.model import DiffuserModelSched
    from baddiffusion_amd.schedulers import DDPMScheduler
    dev = torch.device("cuda")
    sched = DDPMScheduler()
    tab = likelihood.vb_tables(sched, "fixed_large", device=dev)
    T = tab["T"]
    ac = tab["alphas_cumprod"]
    result = {"device": torch.cuda.get_device_name(0), "variance_type": "fixed_large", "cases": []}
    for name, B, S, ts in (("mixed", 2048, 32, MIX), ("all_t0", 2048, 32, (0,)), ("mixed_256", 4, 256, MIX)):
        shape = (B, 3, S, S)
        gen = torch.Generator().manual_seed(B + S)
        t_host = torch.tensor([ts[i % len(ts)] for i in range(B)], dtype=torch.int64)
        t_dev = t_host.to(dev)
        x0 = (torch.randint(0, 256, shape, generator=gen).float() / 255 * 2 - 1).to(dev)
        noise, err = (torch.randn(shape, generator=gen).to(dev) for _ in range(2))
        a = ac[t_dev.clamp(max=T - 1)].view(-1, 1, 1, 1)
        x_t = a.sqrt() * x0 + (1 - a).sqrt() * noise
        eps = noise - (a.sqrt() / (1 - a).sqrt()) * 0.01 * err                         # the prediction is x0 + 0.01 * randn at every t
        times = compare({"fused": lambda: ops.vb_terms(x0, x_t, eps, t_host, tab),
                         "torch": lambda: torch_route(x0, x_t, eps, t_dev, tab)}, args.rounds)
        got, ref = ops.vb_terms(x0, x_t, eps, t_host, tab).double(), torch_route(x0, x_t, eps, t_dev, tab).double()
        nbytes = 4 * 3 * S * S * int((t_host < T).sum()) * 3 + 4 * 3 * S * S * int((t_host == T).sum())
        f, c = times["fused"]["median_s"], times["torch"]["median_s"]
        row = {"case": name, "shape": list(shape), "t": list(ts), "seconds": times, "fused_s": f, "torch_s": c, "torch_over_fused": c / f,
               "fused_not_slower": bool(f <= c), "bytes_min": nbytes, "gbytes_per_s": nbytes / f / 1e9,
               "max_rel_difference_to_torch": float(((got - ref).abs() / ref.abs()).max())}
        result["cases"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "seconds"}), flush=True)
    result["fused_not_slower"] = all(r["fused_not_slower"] for r in result["cases"])
    # a full evaluation: all T timesteps of a few images on the CIFAR topology
    model, _, _ = DiffuserModelSched.get_pretrained("DDPM-CIFAR10-32", allow_random_init=True)
    model = model.cuda()
    n = int(args.full_images)
    clean = torch.randint(0, 256, (n, 32, 32, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).to(dev)
    calls, vb_s, keep_model, keep_vb = [], [], model.forward, ops.vb_terms

    def timed_vb(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = keep_vb(*a, **k)
        torch.cuda.synchronize()
        vb_s.append(time.perf_counter() - t0)
        return out

    likelihood.bits_per_dim(model, sched, clean, timesteps=(0, 1, 500), generator=torch.Generator(device=dev).manual_seed(0))      # warm-up
    model.forward = lambda *a, **k: calls.append(a[0].shape[0]) or keep_model(*a, **k)
    ops.vb_terms = timed_vb
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = likelihood.bits_per_dim(model, sched, clean, generator=torch.Generator(device=dev).manual_seed(0), max_batch_n=256)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    finally:
        model.forward, ops.vb_terms = keep_model, keep_vb
    result["full_evaluation"] = {"topology": "DDPM-CIFAR10-32", "compute_mode": model.compute_mode, "images": n, "timesteps": T, "max_batch_n": 256,
                                 "unet_evaluations_per_image": sum(calls) / n, "unet_forwards": len(calls), "seconds": total,
                                 "seconds_per_image": total / n, "vb_terms_calls": len(vb_s), "vb_terms_seconds": sum(vb_s),
                                 "vb_terms_share": sum(vb_s) / total, "complete": bool(res["complete"]), "mean_bpd_random_weights": res["mean_bpd"]}
    print(json.dumps(result["full_evaluation"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
