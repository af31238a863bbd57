"""Time the stochastic sigma-space sampling loops and the noise step launch on the GPU and write profiles/kdiff_sampling.json.

    python scripts/bench_kdiff.py [--out profiles/kdiff_sampling.json] [--samples 2048] [--rounds 9]

One process, the DDPM-CIFAR10-32 topology with default initialisation (the arithmetic does not depend on the weights), the default
compute mode, `--samples` chains from one seeded noise batch, generator=None (the noise is drawn on the device, the throughput
mode).  Loops, in this order, warmed up and timed as scripts/bench_samplers.py does: DDIM-50, Euler-ancestral at 20 steps
(EulerAncestralPipeline: 20 UNet evaluations, 20 noise tensors), KDPM2-ancestral at 10 steps (KDPM2AncestralPipeline: 19 evaluations, 9
noise tensors), DDIM-50 again.  The two DDIM-50 repeats give the spread of this run; `kdiff_vs_ddim` states whether each loop's ms per
evaluation exceeds DDIM-50's (the mean of the two repeats) by no more than that spread -- the expectation being that throughput
follows the UNet evaluations.

Step launch: bd_sigma_noise_step with the ancestral noise and its scaled output (reads model_output, sample, noise; writes prev_sample
and the scaled sample: 5 streams of 4 B per element) against the same arithmetic from the launches that exist without it: bd_sigma_step
without its scaled output (2 reads + 1 write), one bd_lincomb for the noise term (prev + sigma_up noise, in place: 2 + 1) and
bd_scale_input (1 + 1): 8 streams.  n = samples * 3 * 32 * 32, outputs preallocated on both routes, HIP events around back-to-back
launches, the routes alternated round by round (scripts/bench_defense.py's helpers).  `hbm_share` is bytes / 8 TB/s over the measured
time.  Recorded, not asserted.  No GPU: the script fails, it has no CPU path."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_defense import PEAK_HBM, compare  # noqa: E402
from scripts.bench_samplers import time_loop  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "kdiff_sampling.json"))
    ap.add_argument("--samples", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_kdiff: no GPU (timings are taken on the device or not at all)")
    from baddiffusion_amd import ops
    from baddiffusion_amd.model import DiffuserModelSched
    from baddiffusion_amd.pipelines import DDIMPipeline, EulerAncestralPipeline, KDPM2AncestralPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    model, _, _ = DiffuserModelSched.get_pretrained("DDPM-CIFAR10-32", allow_random_init=True)
    model = model.cuda()
    n = args.samples
    init = torch.randn(n, 3, 32, 32, generator=torch.Generator().manual_seed(0)).cuda()
    steps_of = lambda p: len(p.scheduler.timesteps)                                               # noqa: E731
    plan = [("ddim50_a", DDIMPipeline(model, DDPMScheduler()), 50), ("euler_a_20", EulerAncestralPipeline(model, DDPMScheduler()), 20),
            ("kdpm2_a_10", KDPM2AncestralPipeline(model, DDPMScheduler()), 10), ("ddim50_b", DDIMPipeline(model, DDPMScheduler()), 50)]
    result = {"device": torch.cuda.get_device_name(0), "topology": "DDPM-CIFAR10-32", "samples": n,
              "compute_mode": getattr(model, "compute_mode", None), "output_type": "u8", "generator": None, "loops": {}}
    for name, pipe, steps in plan:
        result["loops"][name] = time_loop(pipe, init, steps, steps_of)
        print(name, json.dumps(result["loops"][name]), flush=True)
    L = result["loops"]
    a, b = L["ddim50_a"]["ms_per_evaluation"], L["ddim50_b"]["ms_per_evaluation"]
    spread, ddim = abs(a - b), (a + b) / 2
    result["kdiff_vs_ddim"] = {"ddim50_ms_per_evaluation": [a, b], "ddim50_spread_ms": spread}
    for name in ("euler_a_20", "kdpm2_a_10"):
        excess = L[name]["ms_per_evaluation"] - ddim
        result["kdiff_vs_ddim"][name] = {"ms_per_evaluation": L[name]["ms_per_evaluation"], "unet_evaluations": L[name]["unet_evaluations"],
                                         "excess_over_ddim50_ms": excess, "within_ddim50_spread": bool(excess <= spread),
                                         "samples_per_s": L[name]["samples_per_s"]}
    print(json.dumps(result["kdiff_vs_ddim"]), flush=True)

    # ---- bd_sigma_noise_step (ancestral noise, scaled output) against bd_sigma_step + bd_lincomb + bd_scale_input
    numel = n * 3 * 32 * 32
    g = torch.Generator().manual_seed(1)
    e, x, z = (torch.randn(numel, generator=g).cuda() for _ in range(3))
    sigma, dt, in_div, up = 2.5, -1.4, 1.9, 0.8
    prev_f, sc_f, prev_l, sc_l = (torch.empty_like(x) for _ in range(4))

    def fused():
        ops.sigma_noise_step(e, x, z, sigma, dt, in_div, sigma_up=up, scaled_out=sc_f, out=prev_f)

    def three_launches():
        ops.sigma_step(e, x, sigma, dt, in_div, out=prev_l)
        ops.lincomb([prev_l, z], [1.0, up], out=prev_l)
        ops.scale_input(prev_l, 1.0, in_div, out=sc_l)
    names = {"bd_sigma_noise_step_up_scaled": fused, "bd_sigma_step_plus_lincomb_plus_scale_input": three_launches}
    times = compare(names, args.rounds)
    for fn in names.values():
        fn()
    bytes_moved = {"bd_sigma_noise_step_up_scaled": 5 * 4 * numel, "bd_sigma_step_plus_lincomb_plus_scale_input": 8 * 4 * numel}
    fused_t, unfused_t = (times[k]["median_s"] for k in names)
    result["noise_step_kernel"] = {
        "n": numel, "times": times, "bytes": bytes_moved,
        "hbm_share": {k: (v / PEAK_HBM) / times[k]["median_s"] for k, v in bytes_moved.items()},
        "unfused_over_fused": unfused_t / fused_t, "fused_not_slower": bool(fused_t <= unfused_t),
        "max_abs_diff_between_routes": {"prev": float((prev_f - prev_l).abs().max()), "scaled": float((sc_f - sc_l).abs().max())}}
    print(json.dumps(result["noise_step_kernel"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=2)
    return result


if __name__ == "__main__":
    main()
