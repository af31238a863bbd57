"""Equivalence of two builds of the native library around a host-only change of csrc/unet_plan.cpp (profiles/plan_step_helpers.json).

Every sub-command works on the tree in the CURRENT DIRECTORY (its baddiffusion_amd package and libbd_hip.so), one build per process:

  plans OUT.json        no device needed: 4 topologies x f32 / bf16x3 / bf16 x training 0/1 x batch sizes -> bd_unet_workspace_bytes,
                        bd_unet_num_params, every bd_unet_param_info row and every bd_unet_segment_range_k
  dump OUTDIR           on the GPU: prediction, loss, flat gradient and dx of seeded forwards + backwards (whole, input-gradient with and
                        without weight gradients, segment by segment under the deferred join) as tensors, plus the launch census
  gnplans OUT.json      no device needed: bd_gn_plan (both directions), bd_gn_fwd_takes_stats, bd_gn_bwd_defers and bd_gn_workspace_bytes on a
                        grid of shapes that holds every dispatch branch and the shapes the launchers turn away
  compare A B OUT.json  A, B: two `plans` or `gnplans` files (exact equality) or two `dump` folders (torch.equal tensor by tensor, census class by class)
  symbols LIB_A LIB_B OUT.json   the exported bd_* symbols of two builds (nm -D)
  speed PARENT OUT.json [N]      on the GPU: N (default 3) alternating windows parent / this tree of the bench.py CIFAR step, each in a child
                                 process of its own under a time limit; stops at the first failing window

usage (parent = an exported, built copy of the parent commit):
  (cd parent && python NEW/scripts/plan_step_helpers.py plans /tmp/p.json) && python scripts/plan_step_helpers.py plans /tmp/n.json
  python scripts/plan_step_helpers.py compare /tmp/p.json /tmp/n.json /tmp/plans_cmp.json
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.getcwd())

MODES = ("f32", "bf16x3", "bf16")
BATCHES = (1, 2, 4, 8, 33, 40, 64, 128)


def topologies():
    from oracle import unet_ref as U
    from tests.golden import cases
    return {"small": cases.SMALL_CFGS["small"], "small_default": cases.SMALL_CFGS["small_default"], "cifar": U.CIFAR10_32,
            "celeba256": U.CELEBA_HQ_256}


def plans(out):
    """host-only: the plan object never touches the device"""
    from baddiffusion_amd import _lib as L
    from baddiffusion_amd.unet import unet_from_config
    lib = L.load()
    rows = {}
    for name, cfg in topologies().items():
        for mode in MODES:
            m = unet_from_config(cfg, compute_mode=mode)
            h = m._plan
            segs = []
            for s in range(lib.bd_unet_num_segments(h)):
                for k in range(lib.bd_unet_segment_num_ranges(h, s)):
                    lo, hi = C.c_int64(), C.c_int64()
                    L.check(lib.bd_unet_segment_range_k(h, s, k, C.byref(lo), C.byref(hi)))
                    segs.append([s, k, lo.value, hi.value])
            table = [[k, off, list(shp), lay] for k, (off, shp, lay) in m._table.items()]
            for training in (0, 1):
                for B in BATCHES[:4] if cfg.sample_size == 256 else BATCHES:
                    rows[f"{name}|{mode}|train{training}|B{B}"] = {
                        "workspace_bytes": m.workspace_bytes(B, training), "num_params": m.num_flat, "params": table, "segments": segs}
    knobs = {k: os.environ[k] for k in ("BD_GSPLIT", "BD_SHORTCUT_SP", "BD_CONV_PS", "BD_FWD_PIPES_MINPX") if k in os.environ}
    json.dump({"knobs": knobs, "plans": rows}, open(out, "w"))
    print(f"{len(rows)} plans -> {out}")


GN_B = (1, 2, 3, 4, 5, 40, 128, 170, 171, 256, 257, 513, 515, 2048, 65535, 65536)
GN_HW = (16, 64, 256, 900, 1024, 2000, 4096, 4100, 65536)
GN_CG = ((24, 6), (64, 32), (96, 8), (128, 32), (256, 2), (256, 32), (384, 32), (512, 32), (768, 32), (1024, 32), (4096, 32), (4100, 4), (130, 32),
         (126, 6))
GN_FIELDS = ("resident", "nt", "cb", "q", "R", "E", "emax", "S", "threads", "r", "per")     # (workspace_bytes came later: not compared)


def gnplans(out):
    """host-only: the GroupNorm queries, return codes of the rejected shapes included"""
    from baddiffusion_amd import _lib as L
    lib = L.load()
    rows = {}
    for B in GN_B:
        for HW in GN_HW:
            for Cc, G in GN_CG:
                row = {"takes_stats": lib.bd_gn_fwd_takes_stats(B, HW, Cc, G), "defers": lib.bd_gn_bwd_defers(B, HW, Cc, G),
                       "workspace_bound": lib.bd_gn_workspace_bytes(B, Cc)}
                for backward in (0, 1):
                    p = L.GnPlanInfo()
                    rc = lib.bd_gn_plan(B, HW, Cc, G, backward, C.byref(p))
                    row[f"plan{backward}"] = [rc] + [getattr(p, f) for f in GN_FIELDS]
                rows[f"B{B}|HW{HW}|C{Cc}|G{G}"] = row
    json.dump({"knobs": {}, "plans": rows}, open(out, "w"))
    print(f"{len(rows)} shapes -> {out}")


# (topology, mode, B): what each one reaches is listed in profiles/plan_step_helpers.json
DUMP_CONFIGS = (("cifar", "bf16x3", 8), ("cifar", "bf16x3", 40), ("cifar", "bf16x3", 128), ("cifar", "f32", 40), ("cifar", "bf16", 40),
                ("celeba256", "bf16x3", 2))
INPUT_GRAD = ("cifar", "bf16x3", 8)
SEGMENTED = ("cifar", "bf16x3", 40)
CENSUS = (("cifar", "bf16x3", 40), ("celeba256", "bf16x3", 2))


def dump(outdir):
    import torch
    from baddiffusion_amd import _lib as L
    from baddiffusion_amd import ops
    from baddiffusion_amd.unet import unet_from_config
    from oracle import unet_ref as U
    os.makedirs(outdir, exist_ok=True)
    lib = L.load()
    topo = topologies()
    census = {}
    for name in ("cifar", "celeba256"):
        cfg = topo[name]
        m = unet_from_config(cfg).cuda()
        m.load_state_dict(U.gen_params(cfg, 7))
        flat = m.flat.data
        S = cfg.sample_size
        for tname, mode, B in DUMP_CONFIGS:
            if tname != name:
                continue
            m.set_compute_mode(mode)
            g = torch.Generator().manual_seed(1000 + B)
            x = torch.randn(B, S, S, 3, generator=g).cuda()
            tg = torch.randn(B, S, S, 3, generator=g).cuda()
            t = torch.randint(0, 1000, (B,), generator=g).cuda()
            tag = f"{name}_{mode}_B{B}"
            res = {}

            def forward():
                pred, ws = m._run_forward(flat, x, t, training=True)
                loss, dpred = ops.loss_fwd_bwd(pred, tg, "l2")
                return pred, ws, loss, dpred

            pred, ws, loss, dpred = forward()
            res["pred"], res["loss"] = pred.clone(), loss.clone()
            res["grads"] = m._run_backward(flat, x, dpred, ws)
            m._release_ws(ws)
            if (name, mode, B) == INPUT_GRAD:       # bd_unet_backward_input: the data-gradient-only schedule, then with gradients
                pred, ws, loss, dpred = forward()
                _, res["dx_only"] = m._run_backward_input(flat, x, dpred, ws, with_grads=False)
                m._release_ws(ws)
                pred, ws, loss, dpred = forward()
                res["grads_with_dx"], res["dx"] = m._run_backward_input(flat, x, dpred, ws, with_grads=True)
                m._release_ws(ws)
            if (name, mode, B) == SEGMENTED:        # segment by segment, weight gradients joined only through bd_unet_stream_wait_aux
                pred, ws, loss, dpred = forward()
                grads = torch.zeros(m.num_flat, device="cuda")
                L.check(lib.bd_unet_set_deferred_join(m._plan, 1))
                lo, hi = C.c_int64(), C.c_int64()
                for s in range(lib.bd_unet_num_segments(m._plan)):
                    L.check(lib.bd_unet_backward_segment(m._plan, s, B, flat.data_ptr(), x.data_ptr(), 3, dpred.data_ptr(), 3, grads.data_ptr(),
                                                         ws.data_ptr(), ws.numel(), L.stream(), C.byref(lo), C.byref(hi)), "backward_segment")
                L.check(lib.bd_unet_stream_wait_aux(m._plan, L.stream()))
                L.check(lib.bd_unet_set_deferred_join(m._plan, 0))
                res["grads_segmented"] = grads
                m._release_ws(ws)
            if (name, mode, B) in CENSUS:           # per-class launch counts of one training forward + backward
                torch.cuda.synchronize()
                lib.bd_prof_enable(1); lib.bd_prof_reset()
                pred, ws, loss, dpred = forward()
                m._run_backward(flat, x, dpred, ws)
                torch.cuda.synchronize()
                rows = {}
                for i in range(lib.bd_prof_num_classes()):
                    nm, cnt, a, b, c = C.c_char_p(), C.c_int64(), C.c_double(), C.c_double(), C.c_double()
                    lib.bd_prof_get(i, C.byref(nm), C.byref(cnt), C.byref(a), C.byref(b), C.byref(c))
                    rows[nm.value.decode()] = rows.get(nm.value.decode(), 0) + cnt.value
                lib.bd_prof_enable(0)
                m._release_ws(ws)
                census[tag] = rows
            torch.cuda.synchronize()
            torch.save({k: v.cpu() for k, v in res.items()}, os.path.join(outdir, tag + ".pt"))
            print(tag, "loss", float(res["loss"]), "grad norm", float(res["grads"].double().norm()), flush=True)
            m._ws_pool = {}
        del m
        torch.cuda.empty_cache()
    json.dump(census, open(os.path.join(outdir, "census.json"), "w"), indent=1)


def compare(a, b, out):
    if os.path.isfile(a):
        A, B = json.load(open(a)), json.load(open(b))
        keys = sorted(set(A["plans"]) | set(B["plans"]))
        bad = [k for k in keys if A["plans"].get(k) != B["plans"].get(k)]
        same_knobs = A["knobs"] == B["knobs"]      # two sweeps under different knobs do not compare: counts as a mismatch
        rep = {"knobs": A["knobs"], "same_knobs": same_knobs, "plans": len(keys), "mismatches": len(bad) + (0 if same_knobs else 1), "mismatching": bad[:20],
               "param_rows": sum(len(v.get("params", ())) for v in A["plans"].values()),
               "segment_ranges": sum(len(v.get("segments", ())) for v in A["plans"].values())}
    else:
        import torch
        rep = {"rows": {}, "census": {}}
        files = sorted(f for f in set(os.listdir(a)) | set(os.listdir(b)) if f.endswith(".pt"))
        for f in files:
            ta, tb = torch.load(os.path.join(a, f)), torch.load(os.path.join(b, f))
            row = {k: bool(k in tb and torch.equal(ta[k], tb[k])) for k in ta}
            row.update({k: False for k in tb if k not in ta})
            row["loss_value"] = float(ta["loss"]); row["grad_norm"] = float(ta["grads"].double().norm())
            row["finite"] = bool(all(torch.isfinite(v).all() for v in ta.values()))
            rep["rows"][f[:-3]] = row
        def census(d):      # a missing census is a mismatch (an empty one never equals the other side's), not an exception
            f = os.path.join(d, "census.json")
            return json.load(open(f)) if os.path.isfile(f) else {}
        ca, cb = census(a), census(b)
        for k in sorted(set(ca) | set(cb)):
            ra, rb = ca.get(k, {}), cb.get(k, {})
            rep["census"][k] = {"classes": len(ra), "launches": sum(ra.values()), "equal": ra == rb,
                                "differ": {c: [ra.get(c), rb.get(c)] for c in sorted(set(ra) | set(rb)) if ra.get(c) != rb.get(c)}}
        rep["configurations"] = len(files)
        rep["differing"] = sum(1 for r in rep["rows"].values() if not all(v for k, v in r.items() if isinstance(v, bool)))
        rep["census_equal"] = bool(ca) and bool(cb) and all(r["equal"] for r in rep["census"].values())
        rep["mismatches"] = rep["differing"] + (0 if rep["census_equal"] else 1)
    json.dump(rep, open(out, "w"), indent=1)
    print(json.dumps({k: v for k, v in rep.items() if k not in ("rows",)}, indent=1))
    return 1 if rep["mismatches"] else 0


def symbols(lib_a, lib_b, out):
    import subprocess

    def syms(lib):
        txt = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
        return sorted(l.split()[-1] for l in txt.splitlines() if l.split()[-1].startswith("bd_"))
    a, b = syms(lib_a), syms(lib_b)
    rep = {"bd_symbols": len(a), "only_in_a": sorted(set(a) - set(b)), "only_in_b": sorted(set(b) - set(a)), "same": a == b}
    json.dump(rep, open(out, "w"), indent=1)
    print(json.dumps(rep))
    return 0 if rep["same"] else 1


def _find(o, key):
    if isinstance(o, dict):
        if key in o:
            return o[key]
        o = list(o.values())
    if isinstance(o, list):
        for v in o:
            r = _find(v, key)
            if r is not None:
                return r
    return None


def speed(parent, out, rounds=3):
    """bench.py --gpus 1 --steps 20 --warmup 5 (CIFAR topology, B = 128, bf16x3), parent and this tree alternately on one board; the new
    medians must lie inside [min, max] of the parent's own windows"""
    import statistics
    import subprocess
    trees = {"parent": os.path.abspath(parent), "new": os.getcwd()}
    ms = {k: [] for k in trees}; host = {k: [] for k in trees}
    rep = {"command": "bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline --full --no-sampling --no-fid --no-celeba --no-dp-sweep "
                      "(--full: the detail object carries host_enqueue_ms_plain)", "windows": int(rounds)}
    for r in range(int(rounds)):
        for name, tree in trees.items():
            detail = os.path.join(os.path.dirname(os.path.abspath(out)), f"bench_detail_{name}_{r}.json")
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--full", "--no-sampling", "--no-fid",
                                "--no-celeba", "--no-dp-sweep", "--detail-file", detail],
                               cwd=tree, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                rep["error"] = f"{name} window {r}: rc {p.returncode}: {p.stderr[-400:]}"
                json.dump(rep, open(out, "w"), indent=1)
                print(rep["error"])
                return 1
            line = json.loads(p.stdout.strip().splitlines()[-1])
            he = _find(line, "host_enqueue_ms_plain")
            if he is None and os.path.isfile(detail):
                he = _find(json.load(open(detail)), "host_enqueue_ms_plain")
            ms[name].append(line["ms_per_step"]); host[name].append(he)
            print(name, r, "ms_per_step", line["ms_per_step"], "host_enqueue_ms_plain", he, flush=True)
    for key, vals in (("ms_per_step", ms), ("host_enqueue_ms_plain", host)):
        lo, hi = min(vals["parent"]), max(vals["parent"])
        med = {k: statistics.median(v) for k, v in vals.items()}
        rep[key] = {"windows": vals, "median": med, "parent_min_max": [lo, hi], "parent_range": hi - lo, "new_median_inside_parent_range": lo <= med["new"] <= hi}
    json.dump(rep, open(out, "w"), indent=1)
    print(json.dumps({k: {"median": v["median"], "parent_min_max": v["parent_min_max"], "inside": v["new_median_inside_parent_range"]}
                      for k, v in rep.items() if isinstance(v, dict)}, indent=1))
    return 0


if __name__ == "__main__":
    cmd = sys.argv[1]
    sys.exit({"plans": plans, "gnplans": gnplans, "dump": dump, "compare": compare, "symbols": symbols, "speed": speed}[cmd](*sys.argv[2:]) or 0)
