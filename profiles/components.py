"""What the surface components (cuberille_set_components) cost, and that they cost nothing while they are off.  Same volume,
same session, warm, medians; every timed leg is a process of its own, alternated three times (the spread of the three is the
yardstick, as in profiles/cell_pixels.py).  The first kernel family here whose cost depends on topology rather than size.

Workloads, device-resident (triangles + projection, bench.py's walk):
  ml:     1024^3 float32 Marschner-Lobb, iso 0.5 (bench.py's generate_block)
  labels: 1024^3 uint8 nested spheres (profiles/cell_pixels.py's) with the band [1, 255]: a handful of large components
  noise:  1024^3 uint8 gradient noise, iso 128 (bench.py's noise workload): very many components -- the case that decides
          whether the feature is usable
Legs:
  off: this tree, the setting off
  par: the PARENT commit's package (--parent-tree: a checkout of it with its library built), which never heard of the setting
  on:  this tree, the setting on
1. off against par: no code on that path changed, so the two must lie within the run's own A/B spread.
2. on - off: the time the pass adds per extraction, and K; ms_emit_cells of the stage-timed extractions holds the pass too.
ms_total / ms_pass are medians of plain extractions, ms_emit_cells of extractions with stage timing on.

The new kernels beside k_emit_cells: `--role on --workload <w>` under `rocprofv3 --kernel-trace --stats`, a run of its own; the
expectation (no gate) is the pass below the walk of the same run on the Marschner-Lobb volume.

    python profiles/components.py --parent-tree DIR [--workloads ml,labels,noise] [--out profiles/components.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REPS = 9
WORKLOADS = ("ml", "labels", "noise")


def role(args):
    """One timed leg in this process; prints one JSON line.  Leg par imports the package of --tree and never names the new symbol."""
    tree = os.path.abspath(args.tree) if args.tree else ROOT
    sys.path.insert(0, tree)
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import __graft_entry__ as graft
    import bench
    from cell_pixels import nested_spheres
    pkg = graft.load_package()
    n = 256 if args.small else 1024                  # (--small: a quick functional pass of the script itself)
    ex = pkg.Extractor(0)
    ex.warm_up()
    if args.workload == "ml":
        dtype, iso, thr = bench.WORKLOADS["marschner_lobb"]
        vol = bench.generate_block(pkg, torch, "marschner_lobb", n, 0, n, None, "cuda")
    elif args.workload == "noise":
        dtype, iso, thr = bench.WORKLOADS["noise"]
        vol = bench.generate_block(pkg, torch, "noise", n, 0, n, None, "cuda")
    else:
        dtype, iso, thr = np.uint8, 1, 0.5
        vol = nested_spheres(torch, n)
        ex.set_band(1, 255, 1, 0)
    torch.cuda.synchronize()
    row = {"role": args.role, "workload": args.workload, "n": n, "tree": "parent" if args.tree else "tree"}
    desc = pkg.make_desc(dtype, (n, n, n))
    if args.role == "on":
        ex.set_components(True)
    prm = pkg.make_params(iso, triangles=True, project=True, threshold=thr, step=0.25, relax=0.95, max_steps=50)
    for stages in (0, 1):
        ex.debug_option("stage_timing", stages)
        got = []
        for _ in range(REPS + 3):                  # (the first ones size the workspace and take the exact launches)
            got.append(ex.extract_device(vol.data_ptr(), desc, prm))
        got = got[3:]
        if not stages:
            row["ms_total"] = statistics.median(r.ms_total for r in got)
            row["ms_pass"] = statistics.median(r.ms_pass for r in got)
            row["ms_total_min_max"] = [min(r.ms_total for r in got), max(r.ms_total for r in got)]
        else:
            row["ms_emit_cells"] = statistics.median(r.ms_emit_cells for r in got)
            row["ms_project"] = statistics.median(r.ms_project for r in got)
            row["ms_emit_cells_min_max"] = [min(r.ms_emit_cells for r in got), max(r.ms_emit_cells for r in got)]
    row["n_points"], row["n_cells"] = int(got[-1].n_points), int(got[-1].n_cells)
    row["proj_iterations"] = int(got[-1].proj_iterations)
    if args.role == "on":
        _, _, counts = ex.download_components()
        row["n_components"] = int(ex.n_components())
        assert int(counts.sum()) == row["n_cells"] and len(counts) == row["n_components"]
        row["largest_components_cells"] = [int(v) for v in np.sort(counts)[::-1][:8]]
        row["components_of_at_most_24_cells"] = int((counts <= 24).sum())
    ex.close()
    print(json.dumps(row), flush=True)


def child(argv, timeout=900):
    out = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=timeout)
    if out.returncode != 0:
        raise RuntimeError("%s failed (%d):\n%s" % (" ".join(argv), out.returncode, out.stderr[-2000:]))
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--role", choices=["off", "par", "on"], default=None)
    ap.add_argument("--workload", choices=WORKLOADS, default="ml")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--tree", default="")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "components.json"))
    a = ap.parse_args()
    if a.role:
        return role(a)
    if not a.parent_tree:
        sys.exit("--parent-tree: a checkout of the parent commit with its library built")
    parent = os.path.abspath(a.parent_tree)
    me = os.path.abspath(__file__)
    small = ["--small"] if a.small else []
    out = {"workloads": {"ml": "1024^3 float32 Marschner-Lobb, iso 0.5, bench walk",
                         "labels": "1024^3 uint8 nested spheres (shells of 12 voxels), band [1, 255] -> 1 / 0, iso 1, bench walk",
                         "noise": "1024^3 uint8 gradient noise, iso 128, bench walk"},
           "reps_per_process": REPS, "device": {}}
    med = statistics.median
    for workload in a.workloads.split(","):
        w = ["--workload", workload] + small
        rounds = []
        for _ in range(a.rounds):
            r = {"off": child([me, "--role", "off"] + w), "par": child([me, "--role", "par", "--tree", parent] + w),
                 "on": child([me, "--role", "on"] + w)}
            assert all(r["off"][k] == r["par"][k] == r["on"][k] for k in ("n_points", "n_cells", "proj_iterations")), r
            rounds.append(r)
            print(json.dumps({k: {f: v.get(f) for f in ("ms_total", "ms_pass", "ms_emit_cells", "n_components")} for k, v in r.items()}),
                  flush=True)
        tot = {k: [r[k]["ms_total"] for r in rounds] for k in rounds[0]}
        out["device"][workload] = {
            "rounds": rounds,
            "n_components": rounds[-1]["on"]["n_components"],
            "ms_total": {k: med(v) for k, v in tot.items()},
            "spread_ms": {k: max(v) - min(v) for k, v in tot.items()},
            "off_minus_parent_ms": med(tot["off"]) - med(tot["par"]),
            "added_by_the_components_ms": med(r["on"]["ms_total"] - r["off"]["ms_total"] for r in rounds),
            "ms_emit_cells": {k: med(r[k]["ms_emit_cells"] for r in rounds) for k in rounds[0]},
            "ms_project": {k: med(r[k]["ms_project"] for r in rounds) for k in rounds[0]},
            "added_to_ms_emit_cells_ms": med(r["on"]["ms_emit_cells"] - r["off"]["ms_emit_cells"] for r in rounds),
        }
        with open(a.out, "w") as f:                    # (kept as it grows: a run cut short leaves what it had)
            json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
