"""Compare two AMDGPU assembly files (hipcc --cuda-device-only -S) kernel by kernel: resources and opcode histograms.

    python scripts/compare_isa.py OLD.s NEW.s [--json OUT.json] [--name LABEL]

A refactor that must not change generated code passes when both files hold the same kernel symbols and, per kernel, the register counts,
LDS and scratch sizes, spill counts, occupancy and code length are equal and so is the multiset of opcodes (first token of every
instruction line).  Register names and the order of instructions may differ.  Exit status 1 when any kernel differs.
"""
import argparse
import collections
import json
import re
import sys

META = [".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".sgpr_spill_count",
        ".vgpr_spill_count"]


def parse(path):
    """-> {kernel symbol: {"res": {...}, "ops": Counter}}"""
    funcs, cur, trailer = {}, None, None
    meta, entry = {}, None
    with open(path) as f:
        for line in f:
            s = line.strip()
            m = re.match(r"\.type\s+(\S+),@function", s)
            if m:
                cur = {"res": {}, "ops": collections.Counter()}
                funcs[m.group(1)] = trailer = cur
                continue
            if s.startswith(".Lfunc_end"):
                cur = None
                continue
            if cur is not None:
                if s and s[0] not in ".;" and not s.endswith(":"):
                    cur["ops"][s.split()[0]] += 1
                continue
            m = re.match(r"; (codeLenInByte|Occupancy)\s*[=:]\s*(\d+)", s)
            if m and trailer is not None:
                trailer["res"][m.group(1)] = int(m.group(2))
                continue
            # .amdgpu_metadata: one "- .agpr_count" item per kernel, keys in alphabetical order, .name among them
            if s.startswith("- .agpr_count:"):
                entry = {}
                s = s[2:]
            m = re.match(r"(\.\w+):\s+(\S+)$", s)
            if m and entry is not None:
                if m.group(1) in META:
                    entry[m.group(1)] = int(m.group(2))
                elif m.group(1) == ".name":
                    meta[m.group(2)] = entry
    kernels = {}
    for name, res in meta.items():
        if name in funcs:
            funcs[name]["res"].update(res)
            kernels[name] = funcs[name]
    return kernels


def compare(old, new):
    a, b = parse(old), parse(new)
    rows = []
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            rows.append({"kernel": name, "match": False, "only_in": "old" if name in a else "new"})
            continue
        ra, rb = a[name]["res"], b[name]["res"]
        res_diff = {k: [ra.get(k), rb.get(k)] for k in sorted(set(ra) | set(rb)) if ra.get(k) != rb.get(k)}
        oa, ob = a[name]["ops"], b[name]["ops"]
        op_diff = {k: [oa.get(k, 0), ob.get(k, 0)] for k in sorted(set(oa) | set(ob)) if oa.get(k, 0) != ob.get(k, 0)}
        row = {"kernel": name, "match": not res_diff and not op_diff, "instructions": sum(ob.values())}
        row.update({k.lstrip("."): v for k, v in rb.items()})
        if res_diff:
            row["resource_diff_old_new"] = res_diff
        if op_diff:
            row["opcode_diff_old_new"] = op_diff
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--json", help="append the table to this JSON file under --name")
    ap.add_argument("--name", help="label of this pair in the JSON file (default: the new file's name)")
    args = ap.parse_args()
    rows = compare(args.old, args.new)
    for r in rows:
        extra = {k: v for k, v in r.items() if k.endswith("_old_new") or k == "only_in"}
        print(f"{'ok  ' if r['match'] else 'DIFF'} {r['kernel']}  vgpr {r.get('vgpr_count')} agpr {r.get('agpr_count')} sgpr {r.get('sgpr_count')} "
              f"lds {r.get('group_segment_fixed_size')} scratch {r.get('private_segment_fixed_size')} occ {r.get('Occupancy')} "
              f"bytes {r.get('codeLenInByte')}" + (f"  {json.dumps(extra)}" if extra else ""))
    bad = [r["kernel"] for r in rows if not r["match"]]
    print(f"{len(rows)} kernels, {len(bad)} differ")
    if args.json:
        try:
            with open(args.json) as f:
                table = json.load(f)
        except FileNotFoundError:
            table = {}
        table[args.name or args.new] = {"kernels": len(rows), "differ": bad, "rows": rows}
        with open(args.json, "w") as f:
            json.dump(table, f, indent=1)
            f.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
