"""Time the quality-metric strip kernels on the GPU and write profiles/quality_metrics.json.

    python scripts/bench_quality.py [--out profiles/quality_metrics.json] [--rounds 9] [--n 10000] [--kid_n 1000] [--d 2048]

bd_knn_sqradius (k = 3 and 5) on n x d features, bd_cross_count_min n x n x d and bd_poly3_rowsum kid_n x kid_n x d, each beside the
same result from torch on the same device: torch.cdist(rows, x, compute_mode="donot_use_mm_for_euclid_dist") ** 2 in row chunks of
1000 (the direct-difference path: the one with comparable arithmetic; the n x n matrix is never whole there either) followed by
kthvalue / the comparison and the row minimum, and for the polynomial kernel an fp32 matmul followed by the fp64 cube and row sum.
The protocol is bench_defense.py's: HIP events around back-to-back launches, every path warmed up first, the implementations alternated
round by round, the median over the rounds with the spread.  The results of the two paths are compared before they are timed.

Counting.  A pair term is one (a[i][k] - b[j][k])^2 (or a[i][k] * b[j][k]) added to a sum: Na * Nb * D of them (a self call computes
both (i, j) and (j, i); both are counted, because both are computed).  A difference term is 3 fp32 operations in 2 packed instructions,
a product term 2 operations in 1; `achieved_f32_flops` is operations per second, to be read beside bd_pairwise_sqdist's 47.3 TFLOP/s
(profiles/defense_kernels.json), and `alu_bound_share` the time the packed instructions need at the fp32 vector peak of 157.3 TFLOP/s
(an fma counts 2) over the measured time.
`fused_not_slower`: the fused median is not above the torch median.  Nothing here is tuned to make it true.
No GPU: the script fails, it has no CPU path."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_defense import PEAK_F32_VECTOR, compare  # noqa: E402

CHUNK = 1000


def torch_sqdist_chunks(a, b):
    for s in range(0, a.shape[0], CHUNK):
        yield s, torch.cdist(a[s:s + CHUNK], b, compute_mode="donot_use_mm_for_euclid_dist") ** 2


def torch_knn(x, k):
    out = []
    for s, d in torch_sqdist_chunks(x, x):
        i = torch.arange(d.shape[0], device=x.device)
        d[i, i + s] = float("inf")
        out.append(d.kthvalue(k, dim=1).values)
    return torch.cat(out)


def torch_count_min(a, b, radius2):
    cs, ms = [], []
    for _, d in torch_sqdist_chunks(a, b):
        cs.append((d <= radius2[None]).sum(1, dtype=torch.int32))
        ms.append(d.min(1).values)
    return torch.cat(cs), torch.cat(ms)


def torch_poly3(a, b):
    return ((a @ b.t()).double() / a.shape[1] + 1.0).pow(3).sum(1)


def rel(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "quality_metrics.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--kid_n", type=int, default=1000)
    ap.add_argument("--d", type=int, default=2048)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_quality: no GPU (timings are taken on the device or not at all)")
    from baddiffusion_amd import _lib as L
    from baddiffusion_amd import ops
    lib = L.load()
    N, M, D = args.n, args.kid_n, args.d
    g = torch.Generator().manual_seed(N + D)
    x = (0.5 * torch.randn(N, D, generator=g).abs()).cuda()                  # non-negative, of the size of pool3 features
    y = (0.5 * torch.randn(N, D, generator=g).abs() + 0.01).cuda()
    result = {"device": torch.cuda.get_device_name(0), "peak_f32_vector_flops": PEAK_F32_VECTOR,
              "bd_pairwise_sqdist_achieved_f32_flops_for_comparison": 47.3e12, "torch_row_chunk": CHUNK, "cases": []}

    def record(name, shape, fused, other, terms, flop_per_term, instr_flops_per_term, agreement, workspace):
        t = compare({name: fused, "torch": other}, args.rounds)
        sec = t[name]["median_s"]
        row = {"kernel": name, "Na": shape[0], "Nb": shape[1], "D": shape[2], "plan": ops.cross_plan(*shape), "workspace_bytes": int(workspace),
               "pair_terms": terms, "times": t, "achieved_f32_flops": flop_per_term * terms / sec,
               "alu_bound_share": (instr_flops_per_term * terms / PEAK_F32_VECTOR) / sec, "speedup_over_torch": t["torch"]["median_s"] / sec,
               "fused_not_slower": bool(sec <= t["torch"]["median_s"]), "agreement_with_torch": agreement}
        if not row["fused_not_slower"]:
            row["note"] = (f"SLOWER than the torch path at this shape ({sec * 1e6:.1f} us against {t['torch']['median_s'] * 1e6:.1f} us): "
                           f"{row['plan']['strips'] * row['plan']['csplit']} workgroups of {row['plan']['tiles_per_split']} tile(s) each on "
                           f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; D is not split and the dot products run on the fp32 "
                           "vector ALUs, torch's matmul on the matrix cores (DESIGN.md section 3)")
        result["cases"].append(row)
        print(json.dumps(row), flush=True)

    for k in (3, 5):
        ours, theirs = ops.knn_sqradius(x, k), torch_knn(x, k)
        record(f"bd_knn_sqradius_k{k}", (N, N, D), lambda: ops.knn_sqradius(x, k), lambda: torch_knn(x, k), N * N * D, 3, 4,
               {"max_rel_diff": rel(ours, theirs)}, lib.bd_knn_sqradius_workspace_bytes(N, D, k))
    radius = ops.knn_sqradius(y, 5)
    (oc, om), (tc, tm) = ops.cross_count_min(x, y, radius), torch_count_min(x, y, radius)
    record("bd_cross_count_min", (N, N, D), lambda: ops.cross_count_min(x, y, radius), lambda: torch_count_min(x, y, radius), N * N * D, 3, 4,
           {"min_d2_max_rel_diff": rel(om, tm), "rows_whose_count_differs": int((oc != tc).sum()), "largest_count_difference": int((oc - tc).abs().max())},
           lib.bd_cross_count_min_workspace_bytes(N, N, D))
    a, b = x[:M].contiguous(), y[:M].contiguous()
    record("bd_poly3_rowsum", (M, M, D), lambda: ops.poly3_rowsum(a, b), lambda: torch_poly3(a, b), M * M * D, 2, 2,
           {"max_rel_diff": rel(ops.poly3_rowsum(a, b), torch_poly3(a, b))}, lib.bd_poly3_rowsum_workspace_bytes(M, M, D))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=2)
    return result


if __name__ == "__main__":
    main()
