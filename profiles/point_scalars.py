"""What the point scalars (cuberille_set_point_scalars) cost, and that they cost nothing while they are off.  Same volume, same
session, warm, medians; every timed leg is a process of its own, alternated three times (the spread of the three is the
yardstick, as in profiles/point_normals.py, which this script is modelled on).

Workload, device-resident, bench.py's own (generate_block, WORKLOADS: triangles + projection, its walk):
  ml:    1024^3 float32 Marschner-Lobb, iso 0.5 (11.1 M points)
The second image of leg `on`: a second 1024^3 float32 volume on the device (a copy of the first, device to device, handed over
with CUBERILLE_MEM_DEVICE), under the same geometry: every point is inside it.
Legs:
  off: this tree, the setting off
  par: the PARENT commit's library (--parent-tree: a checkout of it with its library built), which never heard of the setting
  on:  this tree, the setting on
1. off against par: no code on that path changed, so the two must lie within the run's own A/B spread.
2. on - off: the time the point scalars add per extraction; ms_project of the stage-timed extractions holds the pass too.

k_point_scalars<float> beside k_point_normals<float,0>: `--role both --workload ml` (both settings on) under
`rocprofv3 --kernel-trace --stats`, a run of its own; the expectation is k_point_scalars below k_point_normals on the same
volume and box (8 site loads per vertex against a gathered 4 x 4 x 4).

    python profiles/point_scalars.py --parent-tree DIR [--out profiles/point_scalars.json]
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
SHAPES = {"ml": ("marschner_lobb", 1024)}


def role(args):
    """One timed leg in this process; prints one JSON line.  Leg par imports the package of --tree and never names the new symbol."""
    tree = os.path.abspath(args.tree) if args.tree else ROOT
    sys.path.insert(0, tree)
    import torch
    import __graft_entry__ as graft
    import bench
    pkg = graft.load_package()
    workload, n = SHAPES[args.workload]
    if args.small:                                   # (a quick functional pass of the script itself)
        n = 256
    dtype, iso, thr = bench.WORKLOADS[workload]
    vol = bench.generate_block(pkg, torch, workload, n, 0, n, None, "cuda")
    torch.cuda.synchronize()
    row = {"role": args.role, "workload": args.workload, "n": n, "tree": "parent" if args.tree else "tree"}
    desc = pkg.make_desc(dtype, (n, n, n))
    ex = pkg.Extractor(0)
    ex.warm_up()
    second = None
    if args.role in ("on", "both"):
        second = vol.clone()                           # a second volume of the same size on the device
        torch.cuda.synchronize()
        ex.set_point_scalars((second.data_ptr(), desc))
    if args.role == "both":
        ex.set_point_normals(True)
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
            row["ms_project"] = statistics.median(r.ms_project for r in got)
            row["ms_project_min_max"] = [min(r.ms_project for r in got), max(r.ms_project for r in got)]
    row["n_points"], row["n_cells"] = int(got[-1].n_points), int(got[-1].n_cells)
    row["proj_iterations"] = int(got[-1].proj_iterations)
    if args.role in ("on", "both"):
        import numpy as np
        val = ex.download_point_scalars()
        row["outside_points"] = int(np.isnan(val).sum())
        row["median_abs_residual"] = float(np.nanmedian(np.abs(val - iso)))
    ex.close()
    print(json.dumps(row), flush=True)


def child(argv, timeout=900):
    out = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=timeout)
    if out.returncode != 0:
        raise RuntimeError("%s failed (%d):\n%s" % (" ".join(argv), out.returncode, out.stderr[-2000:]))
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--role", choices=["off", "par", "on", "both"], default=None)
    ap.add_argument("--workload", choices=sorted(SHAPES), default="ml")
    ap.add_argument("--tree", default="")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "point_scalars.json"))
    a = ap.parse_args()
    if a.role:
        return role(a)
    if not a.parent_tree:
        sys.exit("--parent-tree: a checkout of the parent commit with its library built")
    parent = os.path.abspath(a.parent_tree)
    me = os.path.abspath(__file__)
    small = ["--small"] if a.small else []
    out = {"workloads": {"ml": "1024^3 float32 Marschner-Lobb, iso 0.5, bench walk; the second image a device copy of it"},
           "reps_per_process": REPS, "device": {}}
    med = statistics.median
    for workload in ("ml",):
        w = ["--workload", workload] + small
        rounds = []
        for _ in range(a.rounds):
            r = {"off": child([me, "--role", "off"] + w), "par": child([me, "--role", "par", "--tree", parent] + w),
                 "on": child([me, "--role", "on"] + w)}
            assert all(r["off"][k] == r["par"][k] == r["on"][k] for k in ("n_points", "n_cells", "proj_iterations")), r
            rounds.append(r)
            print(json.dumps({k: {f: v.get(f) for f in ("ms_total", "ms_pass", "ms_project")} for k, v in r.items()}), flush=True)
        tot = {k: [r[k]["ms_total"] for r in rounds] for k in rounds[0]}
        out["device"][workload] = {
            "rounds": rounds,
            "ms_total": {k: med(v) for k, v in tot.items()},
            "spread_ms": {k: max(v) - min(v) for k, v in tot.items()},
            "off_minus_parent_ms": med(tot["off"]) - med(tot["par"]),
            "added_by_the_point_scalars_ms": med(r["on"]["ms_total"] - r["off"]["ms_total"] for r in rounds),
            "ms_project": {k: med(r[k]["ms_project"] for r in rounds) for k in rounds[0]},
            "added_to_ms_project_ms": med(r["on"]["ms_project"] - r["off"]["ms_project"] for r in rounds),
        }
        with open(a.out, "w") as f:                    # (kept as it grows: a run cut short leaves what it had)
            json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
