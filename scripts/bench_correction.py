"""Measurements for the sampler-matched correction tables, on the GPU:

    python scripts/bench_correction.py [--rounds 9] [--out profiles/poison_corr.json] [--chains-out profiles/correction_chains.json]

  (1) bd_poison_qsample against bd_poison_qsample_corr in one process at the training call's size: uint8 images, B = 128, 3 x 32 x 32,
      gather and flip on, 10 % poisoned rows.  The table variant trades two sqrtf and a divide for one load from a 4 KB table; both move
      the same bytes.  HIP events around `inner` back-to-back launches, the two forms alternated window by window; the median over the
      windows with the windows' spread (max - min).  -> profiles/poison_corr.json
  (2) the open-loop residual (correction.open_loop_residual) of the nine deterministic samplers with the reference's rho and with the ode
      table, DDIM-50's with its exact table, on the inputs of tests/golden/correction.npz, and the share of its bound each uses (bounds:
      tests/golden/cases_correction.py).  -> profiles/correction_chains.json
Nothing is asserted.  No GPU: the script fails, it has no CPU path."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / inner


def compare(fns, rounds, budget=0.2, cap=2000):
    inner = {}
    for name, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        inner[name] = max(1, min(cap, int(budget / max(timed(fn, 20) , 1e-7))))
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, inner[name]))
    return {name: {"median_s": statistics.median(t), "min_s": min(t), "max_s": max(t), "spread_s": max(t) - min(t),
                   "launches_per_window": inner[name], "windows": rounds} for name, t in times.items()}


def kernels(rounds):
    import ctypes as C
    from baddiffusion_amd import _lib as L, correction
    from baddiffusion_amd.dataset import Backdoor
    from baddiffusion_amd.schedulers import DDPMScheduler
    dev = torch.device("cuda")
    B, S, NIMG = 128, 32, 8192
    sched = DDPMScheduler()
    al, ac = sched.device_tables(dev)
    corr = correction.make_table("ode", sched, device=dev)
    bd = Backdoor(root=None)
    trigger = bd.get_trigger("BOX_14", 3, S).to(dev).contiguous()
    target = bd.get_target("CORNER", trigger.cpu()).to(dev).contiguous()
    g = torch.Generator().manual_seed(1000)
    images = torch.randint(0, 256, (NIMG, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    rows = torch.randint(0, NIMG, (B,), generator=g).to(dev)
    flip = (torch.rand(B, generator=g) < 0.5).to(torch.uint8).to(dev)
    pois = (torch.arange(B) % 10 == 0).to(torch.uint8).to(dev)
    noise = torch.randn(B, 3, S, S, generator=g).to(dev)
    t = torch.randint(0, 1000, (B,), generator=g).to(dev)
    xn, tg = torch.empty(B, S, S, 3, device=dev), torch.empty(B, S, S, 3, device=dev)
    # the entry points themselves, on prebuilt descriptors: the wrapper's allocations are the same for both and are not the subject
    kw = dict(B=B, C=3, H=S, W=S, images_u8=L.ptr(images), is_poison=L.ptr(pois), trigger=L.ptr(trigger), target_img=L.ptr(target),
              noise=L.ptr(noise), timesteps=L.ptr(t), alphas=L.ptr(al), alphas_cumprod=L.ptr(ac), vmin=-1.0, x_noisy=L.ptr(xn), ld_noisy=3,
              target=L.ptr(tg), ld_target=3, row_index=L.ptr(rows), flip=L.ptr(flip))
    lib = L.load()
    d_old, d_new = L.PoisonQsampleDesc(**kw), L.PoisonQsampleCorrDesc(corr=L.ptr(corr), **kw)
    st = L.stream()

    def old():
        L.check(lib.bd_poison_qsample(C.byref(d_old), st), "bd_poison_qsample")

    def new():
        L.check(lib.bd_poison_qsample_corr(C.byref(d_new), st), "bd_poison_qsample_corr")
    r = compare({"bd_poison_qsample": old, "bd_poison_qsample_corr": new}, rounds)
    a, b = r["bd_poison_qsample"], r["bd_poison_qsample_corr"]
    bytes_moved = B * S * S * 3 * (1 + 4 + 4 + 4)            # uint8 image in, noise in, x_noisy and target out
    for v in r.values():
        v["bytes"] = bytes_moved
    return {"device": torch.cuda.get_device_name(0), "shape": {"B": B, "C": 3, "H": S, "W": S, "images": "uint8, gather + flip", "poisoned": 0.1},
            "kernels": r, "corr_minus_plain_s": b["median_s"] - a["median_s"], "larger_spread_s": max(a["spread_s"], b["spread_s"]),
            "equal_within_spread": abs(b["median_s"] - a["median_s"]) <= max(a["spread_s"], b["spread_s"])}


def chains():
    from baddiffusion_amd import correction
    from tests.golden import cases_correction as CC
    g = np.load(os.path.join(ROOT, "tests", "golden", "correction.npz"))
    kw = dict(target=g["y"], trigger=g["r"], eps=g["eps"])
    out = {"bounds": {"ode_max": CC.ODE_MAX, "rho_min": CC.RHO_MIN, "ddim_exact_max": CC.DDIM_EXACT_MAX}, "chains": {}}
    for tag in CC.CHAINS:
        pipe, call = CC.build_pipeline(tag)
        ode = correction.open_loop_residual(pipe, g["ode"], **kw, **call)
        rho = correction.open_loop_residual(pipe, g["rho"], **kw, **call)
        rec = {"ode": ode, "ode_reference_fp64": float(g["res_ode_" + tag]), "ode_share_of_bound": ode / CC.ODE_MAX,
               "rho": rho, "rho_reference_fp64": float(g["res_rho_" + tag]), "rho_over_bound": rho / CC.RHO_MIN}
        if tag == "ddim50":
            ex = correction.open_loop_residual(pipe, g["ddim"], **kw, **call)
            rec.update(ddim_exact=ex, ddim_exact_reference_fp64=float(g["res_ddim_ddim50"]), ddim_exact_share_of_bound=ex / CC.DDIM_EXACT_MAX)
        out["chains"][tag] = rec
        print(tag, json.dumps(rec), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "poison_corr.json"))
    ap.add_argument("--chains-out", default=os.path.join("profiles", "correction_chains.json"))
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_correction: no GPU (timings are taken on the device or not at all)")
    for path, fn in ((args.out, lambda: kernels(args.rounds)), (args.chains_out, chains)):
        res = fn()
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=2)
    print(json.dumps(json.load(open(args.out))["kernels"]))


if __name__ == "__main__":
    main()
