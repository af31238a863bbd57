"""Time the sampling loops side by side on the GPU and write profiles/deis_sampling.json (profiles/dpm_solver_sampling.json,
profiles/unipc_sampling.json and profiles/sigma_sampling.json are earlier runs of this script, before the UniPC rows, before the
sigma-space rows and before the DEIS rows).

    python scripts/bench_samplers.py [--out profiles/deis_sampling.json] [--samples 2048] [--rounds 9]

One process, the DDPM-CIFAR10-32 topology with default initialisation (the arithmetic does not depend on the weights), the default compute
mode, `--samples` chains from one seeded noise batch.  Loops, in this order: DDIM-50, PNDM-50 (59 UNet evaluations), DPM-Solver++ order 2
at 20 and at 10 steps (DPMSolverPipeline), UniPC order 2 at 20 and at 10 steps and order 3 at 10 (UniPCPipeline, bh2, predict_x0), LMS
order 4 at 20 steps (LMSPipeline) and Heun at 10 steps (HeunPipeline: 19 UNet evaluations), DEIS order 2 at 20 steps and order 3 at 10
(DEISPipeline, the reference's coefficient arithmetic), DDIM-50 again.  Every loop is warmed up on its full chunk shape at a few steps and with its whole schedule on 64 samples (a sampling job runs
the same schedule chunk after chunk, and DPMSolverMultistepScheduler keeps the host scalars of the schedule it ran last), then timed
with a host clock between two device synchronisations.  output_type="u8" throughout (device images, what batch_sampling_save asks for),
so no loop is charged a copy of its images to the host.  Recorded per loop: seconds, samples/s, UNet evaluations and ms per evaluation.
The two DDIM-50 repeats give the spread of this run; `dpm_vs_ddim` states whether the DPM pipeline's ms per evaluation exceeds DDIM-50's
(the mean of the two repeats) by no more than that spread; `unipc_vs_dpm` states the same for each UniPC loop against the DPM loop of the
same step count; `sigma_vs_dpm` states it for the two sigma-space loops against DPM-Solver++ at 20 steps, whose evaluations run the same
UNet on the same batch -- the expectation being that throughput follows the UNet evaluations, N for LMS and 2N - 1 for Heun;
`deis_vs_dpm` states it for each DEIS loop against the DPM loop of the same step count.

Step kernel: bd_dpm_step at order 2 (reads model_output, sample, m1; writes m0 and prev_sample: 5 streams of 4 B per element) against
the same update as two bd_lincomb launches (x0 = sample / alpha - (sigma / alpha) eps: 2 reads + 1 write; prev = cx sample + c0 x0 +
c1 m1: 3 reads + 1 write: 7 streams; no clamp of x0 on that route), n = samples * 3 * 32 * 32, outputs preallocated on both routes, HIP
events around back-to-back launches, the routes alternated round by round (scripts/bench_defense.py's helpers).  `hbm_share` is
bytes / 8 TB/s over the measured time.  bd_unipc_step at order 2 in the steady state (reads model_output, sample, last_sample, h1, h2; writes m0, the corrected sample and
prev_sample: 8 streams) against the same step as three bd_lincomb launches (x0: 2 reads + 1 write; corrected = kl last + k0 x0 + k1 h1 +
k2 h2: 4 + 1; prev = px corrected + p0 x0 + p1 h1: 3 + 1: 12 streams), measured the same way.  bd_sigma_step as the LMS order 4 step in
the steady state with its scaled output (reads model_output, sample, h1, h2, h3; writes the derivative, prev_sample and the scaled
sample: 8 streams) against the same arithmetic as three bd_lincomb launches (x0 = sample - sigma eps: 2 + 1; d = (sample - x0) / sigma:
2 + 1; prev = sample + c0 d + c1 h1 + c2 h2 + c3 h3: 5 + 1) plus a separate bd_scale_input (1 + 1): 14 streams, and against the
shortcut that takes the model output for the derivative (mathematically equal, not bitwise: one bd_lincomb of 5 + 1 and the
bd_scale_input: 8 streams, but no stored derivative).  bd_deis_step at order 3 (reads model_output, sample, m1, m2; writes m0 and
prev_sample: 6 streams) against the same arithmetic as three bd_lincomb launches (x0 = sample / alpha - (sigma / alpha) eps: 2 + 1; m0 =
sample / sigma - (alpha / sigma) x0, the conversion back: 2 + 1; prev = (alpha_t / alpha) sample + alpha_t k0 m0 + alpha_t k1 m1 +
alpha_t k2 m2: 4 + 1: 11 streams; equal mathematically, not bitwise).  Recorded, not asserted.  No GPU: the script fails, it has no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_defense import PEAK_HBM, compare  # noqa: E402


def time_loop(pipe, init, steps, evals_of):
    n = init.shape[0]
    pipe.set_progress_bar_config(disable=True)
    pipe(batch_size=n, init=init, num_inference_steps=5, output_type="u8")                      # warm-up: the full chunk shape at a few steps
    pipe(batch_size=n, init=init[:min(n, 64)], num_inference_steps=steps, output_type="u8")      # + the whole schedule on a small chunk
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = pipe(batch_size=n, init=init, num_inference_steps=steps, output_type="u8")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    evals = evals_of(pipe)
    return {"steps": steps, "unet_evaluations": evals, "seconds": dt, "samples_per_s": n / dt, "ms_per_evaluation": dt / evals * 1e3,
            "images_shape": list(out.images.shape)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "deis_sampling.json"))
    ap.add_argument("--samples", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_samplers: no GPU (timings are taken on the device or not at all)")
    from baddiffusion_amd import ops
    from baddiffusion_amd.model import DiffuserModelSched
    from baddiffusion_amd.pipelines import DDIMPipeline, DEISPipeline, DPMSolverPipeline, HeunPipeline, LMSPipeline, PNDMPipeline, UniPCPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler, DEISMultistepScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler
    model, _, _ = DiffuserModelSched.get_pretrained("DDPM-CIFAR10-32", allow_random_init=True)
    model = model.cuda()
    n = args.samples
    init = torch.randn(n, 3, 32, 32, generator=torch.Generator().manual_seed(0)).cuda()
    steps_of = lambda p: len(p.scheduler.timesteps)                                               # noqa: E731
    mk_dpm = lambda: DPMSolverPipeline(model, DPMSolverMultistepScheduler(solver_order=2, algorithm_type="dpmsolver++"))   # noqa: E731
    mk_unipc = lambda order: UniPCPipeline(model, UniPCMultistepScheduler(solver_order=order))      # noqa: E731
    mk_deis = lambda order: DEISPipeline(model, DEISMultistepScheduler(solver_order=order))         # noqa: E731
    plan = [("ddim50_a", DDIMPipeline(model, DDPMScheduler()), 50), ("pndm50", PNDMPipeline(model, DDPMScheduler()), 50),
            ("dpmpp_o2_20", mk_dpm(), 20), ("dpmpp_o2_10", mk_dpm(), 10), ("unipc_o2_20", mk_unipc(2), 20), ("unipc_o2_10", mk_unipc(2), 10),
            ("unipc_o3_10", mk_unipc(3), 10), ("lms_o4_20", LMSPipeline(model, DDPMScheduler(), order=4), 20),
            ("heun_10", HeunPipeline(model, DDPMScheduler()), 10), ("deis_o2_20", mk_deis(2), 20), ("deis_o3_10", mk_deis(3), 10),
            ("ddim50_b", DDIMPipeline(model, DDPMScheduler()), 50)]
    result = {"device": torch.cuda.get_device_name(0), "topology": "DDPM-CIFAR10-32", "samples": n,
              "compute_mode": getattr(model, "compute_mode", None), "output_type": "u8", "loops": {}}
    for name, pipe, steps in plan:
        result["loops"][name] = time_loop(pipe, init, steps, steps_of)
        print(name, json.dumps(result["loops"][name]), flush=True)
    L = result["loops"]
    a, b = L["ddim50_a"]["ms_per_evaluation"], L["ddim50_b"]["ms_per_evaluation"]
    spread, ddim = abs(a - b), (a + b) / 2
    result["dpm_vs_ddim"] = {"ddim50_ms_per_evaluation": [a, b], "ddim50_spread_ms": spread}
    for name in ("dpmpp_o2_20", "dpmpp_o2_10"):
        excess = L[name]["ms_per_evaluation"] - ddim
        result["dpm_vs_ddim"][name] = {"ms_per_evaluation": L[name]["ms_per_evaluation"], "excess_over_ddim50_ms": excess,
                                       "within_ddim50_spread": bool(excess <= spread),
                                       "speedup_over_ddim50": L[name]["samples_per_s"] / (n / statistics.mean((L["ddim50_a"]["seconds"], L["ddim50_b"]["seconds"]))),
                                       "evaluation_ratio": 50 / L[name]["unet_evaluations"]}
    print(json.dumps(result["dpm_vs_ddim"]), flush=True)
    result["unipc_vs_dpm"] = {"ddim50_spread_ms": spread}
    for name, dpm in (("unipc_o2_20", "dpmpp_o2_20"), ("unipc_o2_10", "dpmpp_o2_10"), ("unipc_o3_10", "dpmpp_o2_10")):
        excess = L[name]["ms_per_evaluation"] - L[dpm]["ms_per_evaluation"]
        result["unipc_vs_dpm"][name] = {"ms_per_evaluation": L[name]["ms_per_evaluation"], "dpm_loop": dpm,
                                        "dpm_ms_per_evaluation": L[dpm]["ms_per_evaluation"], "excess_over_dpm_ms": excess,
                                        "within_ddim50_spread": bool(excess <= spread),
                                        "excess_over_ddim50_ms": L[name]["ms_per_evaluation"] - ddim,
                                        "samples_per_s": L[name]["samples_per_s"]}
    print(json.dumps(result["unipc_vs_dpm"]), flush=True)
    result["sigma_vs_dpm"] = {"ddim50_spread_ms": spread, "ddim50_ms_per_evaluation": ddim,
                              "dpmpp_o2_20_ms_per_evaluation": L["dpmpp_o2_20"]["ms_per_evaluation"]}
    for name in ("lms_o4_20", "heun_10"):
        excess = L[name]["ms_per_evaluation"] - L["dpmpp_o2_20"]["ms_per_evaluation"]
        result["sigma_vs_dpm"][name] = {"ms_per_evaluation": L[name]["ms_per_evaluation"], "unet_evaluations": L[name]["unet_evaluations"],
                                        "excess_over_dpm_ms": excess, "within_ddim50_spread": bool(excess <= spread),
                                        "excess_over_ddim50_ms": L[name]["ms_per_evaluation"] - ddim, "samples_per_s": L[name]["samples_per_s"]}
    print(json.dumps(result["sigma_vs_dpm"]), flush=True)
    result["deis_vs_dpm"] = {"ddim50_spread_ms": spread, "ddim50_ms_per_evaluation": [a, b]}
    for name, dpm in (("deis_o2_20", "dpmpp_o2_20"), ("deis_o3_10", "dpmpp_o2_10")):
        excess = L[name]["ms_per_evaluation"] - L[dpm]["ms_per_evaluation"]
        result["deis_vs_dpm"][name] = {"ms_per_evaluation": L[name]["ms_per_evaluation"], "dpm_loop": dpm,
                                       "dpm_ms_per_evaluation": L[dpm]["ms_per_evaluation"], "excess_over_dpm_ms": excess,
                                       "within_ddim50_spread": bool(excess <= spread),
                                       "excess_over_ddim50_ms": L[name]["ms_per_evaluation"] - ddim, "samples_per_s": L[name]["samples_per_s"]}
    print(json.dumps(result["deis_vs_dpm"]), flush=True)

    # ---- the step kernel against the two-launch route
    numel = n * 3 * 32 * 32
    g = torch.Generator().manual_seed(1)
    e, x, m1 = (torch.randn(numel, generator=g).cuda() for _ in range(3))
    alpha_s, sigma_s, cx, c0, c1 = 0.8, 0.6, 0.9, 0.35, -0.5
    m0_f, prev_f, m0_l, prev_l = (torch.empty_like(x) for _ in range(4))

    def fused():
        ops.dpm_step(e, x, cx, c0, m1=m1, c1=c1, convert=(alpha_s, sigma_s), m0_out=m0_f, out=prev_f)

    def two_launches():
        ops.lincomb([x, e], [1.0 / alpha_s, -sigma_s / alpha_s], out=m0_l)
        ops.lincomb([x, m0_l, m1], [cx, c0, c1], out=prev_l)
    times = compare({"bd_dpm_step_order2": fused, "bd_lincomb_x2": two_launches}, args.rounds)
    fused(); two_launches()
    bytes_moved = {"bd_dpm_step_order2": 5 * 4 * numel, "bd_lincomb_x2": 7 * 4 * numel}
    result["step_kernel"] = {"n": numel, "times": times, "bytes": bytes_moved,
                             "hbm_share": {k: (v / PEAK_HBM) / times[k]["median_s"] for k, v in bytes_moved.items()},
                             "two_launches_over_fused": times["bd_lincomb_x2"]["median_s"] / times["bd_dpm_step_order2"]["median_s"],
                             "fused_not_slower": bool(times["bd_dpm_step_order2"]["median_s"] <= times["bd_lincomb_x2"]["median_s"]),
                             "max_abs_diff_between_routes": {"m0": float((m0_f - m0_l).abs().max()), "prev": float((prev_f - prev_l).abs().max())}}
    print(json.dumps(result["step_kernel"]), flush=True)

    # ---- the UniPC step kernel (order 2, steady state: corrector + predictor) against the three-launch route
    last, h1, h2 = (torch.randn(numel, generator=g).cuda() for _ in range(3))
    kl, k0, k1, k2, px, p0, p1 = 0.9, -0.25, 0.3, -0.15, 0.85, 0.35, -0.5
    um0_f, uxc_f, uprev_f, um0_l, uxc_l, uprev_l = (torch.empty_like(x) for _ in range(6))

    def unipc_fused():
        ops.unipc_step(e, x, px, p0, h1=h1, p1=p1, h2=h2, p2=0.0, last_sample=last, kl=kl, k0=k0, k1=k1, k2=k2,
                       convert=(alpha_s, sigma_s), m0_out=um0_f, corrected_out=uxc_f, out=uprev_f)

    def three_launches():
        ops.lincomb([x, e], [1.0 / alpha_s, -sigma_s / alpha_s], out=um0_l)
        ops.lincomb([last, um0_l, h1, h2], [kl, k0, k1, k2], out=uxc_l)
        ops.lincomb([uxc_l, um0_l, h1], [px, p0, p1], out=uprev_l)
    times = compare({"bd_unipc_step_order2": unipc_fused, "bd_lincomb_x3": three_launches}, args.rounds)
    unipc_fused(); three_launches()
    bytes_moved = {"bd_unipc_step_order2": 8 * 4 * numel, "bd_lincomb_x3": 12 * 4 * numel}
    result["unipc_step_kernel"] = {
        "n": numel, "times": times, "bytes": bytes_moved,
        "hbm_share": {k: (v / PEAK_HBM) / times[k]["median_s"] for k, v in bytes_moved.items()},
        "three_launches_over_fused": times["bd_lincomb_x3"]["median_s"] / times["bd_unipc_step_order2"]["median_s"],
        "fused_not_slower": bool(times["bd_unipc_step_order2"]["median_s"] <= times["bd_lincomb_x3"]["median_s"]),
        "max_abs_diff_between_routes": {"m0": float((um0_f - um0_l).abs().max()), "corrected": float((uxc_f - uxc_l).abs().max()),
                                        "prev": float((uprev_f - uprev_l).abs().max())}}
    print(json.dumps(result["unipc_step_kernel"]), flush=True)

    # ---- bd_sigma_step (LMS order 4, steady state, with the scaled output) against bd_lincomb launches + a separate bd_scale_input
    h3 = torch.randn(numel, generator=g).cuda()
    sigma, in_div, s0, s1, s2, s3 = 2.5, 1.9, -0.8, 0.3, -0.12, 0.02
    d_f, sprev_f, sc_f, x0_l, d_l, sprev_l, sc_l, sprev_s, sc_s = (torch.empty_like(x) for _ in range(9))

    def sigma_fused():
        ops.sigma_step(e, x, sigma, s0, in_div, h1=h1, c1=s1, h2=h2, c2=s2, h3=h3, c3=s3, d_out=d_f, scaled_out=sc_f, out=sprev_f)

    def lincombs_plus_scale():
        ops.lincomb([x, e], [1.0, -sigma], out=x0_l)
        ops.lincomb([x, x0_l], [1.0 / sigma, -1.0 / sigma], out=d_l)
        ops.lincomb([x, d_l, h1, h2, h3], [1.0, s0, s1, s2, s3], out=sprev_l)
        ops.scale_input(sprev_l, 1.0, in_div, out=sc_l)

    def shortcut_plus_scale():
        ops.lincomb([x, e, h1, h2, h3], [1.0, s0, s1, s2, s3], out=sprev_s)
        ops.scale_input(sprev_s, 1.0, in_div, out=sc_s)
    names = {"bd_sigma_step_lms4_scaled": sigma_fused, "bd_lincomb_x3_plus_scale_input": lincombs_plus_scale,
             "bd_lincomb_x1_plus_scale_input": shortcut_plus_scale}
    times = compare(names, args.rounds)
    for fn in names.values():
        fn()
    bytes_moved = {"bd_sigma_step_lms4_scaled": 8 * 4 * numel, "bd_lincomb_x3_plus_scale_input": 14 * 4 * numel,
                   "bd_lincomb_x1_plus_scale_input": 8 * 4 * numel}
    fused_t = times["bd_sigma_step_lms4_scaled"]["median_s"]
    result["sigma_step_kernel"] = {
        "n": numel, "times": times, "bytes": bytes_moved,
        "hbm_share": {k: (v / PEAK_HBM) / times[k]["median_s"] for k, v in bytes_moved.items()},
        "unfused_over_fused": times["bd_lincomb_x3_plus_scale_input"]["median_s"] / fused_t,
        "shortcut_over_fused": times["bd_lincomb_x1_plus_scale_input"]["median_s"] / fused_t,
        "fused_not_slower": bool(fused_t <= times["bd_lincomb_x3_plus_scale_input"]["median_s"]),
        "fused_not_slower_than_shortcut": bool(fused_t <= times["bd_lincomb_x1_plus_scale_input"]["median_s"]),
        "max_abs_diff_between_routes": {"derivative": float((d_f - d_l).abs().max()), "prev": float((sprev_f - sprev_l).abs().max()),
                                        "scaled": float((sc_f - sc_l).abs().max()), "prev_shortcut": float((sprev_f - sprev_s).abs().max())}}
    print(json.dumps(result["sigma_step_kernel"]), flush=True)

    # ---- bd_deis_step (order 3) against three bd_lincomb launches: x0, the conversion back to eps, the update
    alpha_t, d0, d1, d2 = 0.9, -0.5, 0.3, -0.15
    dm0_f, dprev_f, dx0_l, dm0_l, dprev_l = (torch.empty_like(x) for _ in range(5))

    def deis_fused():
        ops.deis_step(e, x, alpha_s, sigma_s, m1=h1, alpha_t=alpha_t, k0=d0, k1=d1, m2=h2, k2=d2, m0_out=dm0_f, out=dprev_f)

    def deis_three_launches():
        ops.lincomb([x, e], [1.0 / alpha_s, -sigma_s / alpha_s], out=dx0_l)
        ops.lincomb([x, dx0_l], [1.0 / sigma_s, -alpha_s / sigma_s], out=dm0_l)
        ops.lincomb([x, dm0_l, h1, h2], [alpha_t / alpha_s, alpha_t * d0, alpha_t * d1, alpha_t * d2], out=dprev_l)
    times = compare({"bd_deis_step_order3": deis_fused, "bd_lincomb_x3": deis_three_launches}, args.rounds)
    deis_fused(); deis_three_launches()
    bytes_moved = {"bd_deis_step_order3": 6 * 4 * numel, "bd_lincomb_x3": 11 * 4 * numel}
    result["deis_step_kernel"] = {
        "n": numel, "times": times, "bytes": bytes_moved,
        "hbm_share": {k: (v / PEAK_HBM) / times[k]["median_s"] for k, v in bytes_moved.items()},
        "three_launches_over_fused": times["bd_lincomb_x3"]["median_s"] / times["bd_deis_step_order3"]["median_s"],
        "fused_not_slower": bool(times["bd_deis_step_order3"]["median_s"] <= times["bd_lincomb_x3"]["median_s"]),
        "max_abs_diff_between_routes": {"m0": float((dm0_f - dm0_l).abs().max()), "prev": float((dprev_f - dprev_l).abs().max())}}
    print(json.dumps(result["deis_step_kernel"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=2)
    return result


if __name__ == "__main__":
    main()
