"""What meshing a label or a value band in place (cuberille_set_band) costs against the route a caller had to take before: a
thresholded copy (itk::BinaryThresholdImageFilter's output), then the extraction of the copy.  Same volume, same session, warm,
medians; every timed leg is a process of its own, alternated three times (the spread of the three is the yardstick, as in
profiles/region_extract.py).

Workloads, both device-resident, triangles + projection with bench.py's walk, band values 1 / 0 at iso 1:
  labels: 1024^3 uint8, nested spheres labelled 0 .. 4, the band = labels 2 .. 3
  ml:     1024^3 float32 Marschner-Lobb (volumes.marschner_lobb), the band = 0.4 .. 0.6
Legs:
  a: this tree, set_band on the volume as it is
  b: the PARENT commit's package (--parent-tree: a checkout of it with its library built) on the thresholded copy
  c: the copy itself, torch.where on the device, timed by events (measured in leg b's process)
  p: this tree, band off, the plain sweep of the SAME buffer (iso = the band's lower bound): the sweep's A/B partner
ms_total / ms_pass are medians of plain extractions, ms_classify / ms_project of extractions with stage timing on.

The kernels of leg a alone: `--role a --workload labels` under `rocprofv3 --kernel-trace --stats`, a run of its own.

    python profiles/band_extract.py --parent-tree DIR [--out profiles/band_extract.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WALK = dict(threshold=0.002, step=0.25, relax=0.95, max_steps=50)   # bench.py's workload
REPS = 9
BANDS = {"labels": (2, 3), "ml": (0.4, 0.6)}


def volume(pkg, torch, workload, n):
    if workload == "ml":
        return pkg.volumes.marschner_lobb(n, xp=torch, device="cuda").contiguous()
    z = torch.arange(n, device="cuda", dtype=torch.float32).view(-1, 1, 1)
    y = torch.arange(n, device="cuda", dtype=torch.float32).view(1, -1, 1)
    x = torch.arange(n, device="cuda", dtype=torch.float32).view(1, 1, -1)
    r = torch.sqrt((x - n * 0.49) ** 2 + (y - n * 0.52) ** 2 + (z - n * 0.47) ** 2)
    lab = torch.zeros((n, n, n), device="cuda", dtype=torch.uint8)
    for f in (0.45, 0.38, 0.27, 0.15):
        lab += (r < n * f).to(torch.uint8)
    return lab


def role(args):
    """One timed leg in this process; prints one JSON line.  Leg b imports the package of --tree and never names the new symbol."""
    tree = os.path.abspath(args.tree) if args.tree else ROOT
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import __graft_entry__ as graft
    pkg = graft.load_package()
    n = 256 if args.small else 1024                  # (--small: a quick functional pass of the script itself)
    vol = volume(pkg, torch, args.workload, n)
    lower, upper = BANDS[args.workload]
    dtype = np.uint8 if args.workload == "labels" else np.float32
    torch.cuda.synchronize()
    row = {"role": args.role, "workload": args.workload, "tree": "parent" if args.tree else "tree"}
    vox, iso = vol, 1
    if args.role == "b":
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ms = []
        one, zero = torch.ones((), dtype=vol.dtype, device="cuda"), torch.zeros((), dtype=vol.dtype, device="cuda")
        for _ in range(REPS + 2):
            ev[0].record()
            vox = torch.where((vol >= lower) & (vol <= upper), one, zero)
            ev[1].record()
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        row["ms_threshold_copy"] = statistics.median(ms[2:])
        assert vox.dtype == vol.dtype
    elif args.role == "p":
        iso = lower
    desc = pkg.make_desc(dtype, (n, n, n))
    ex = pkg.Extractor(0)
    ex.warm_up()
    if args.role == "a":
        ex.set_band(lower, upper, 1, 0)
    prm = pkg.make_params(iso, **WALK)
    for stages in (0, 1):
        ex.debug_option("stage_timing", stages)
        got = []
        for _ in range(REPS + 3):                  # (the first ones size the workspace and take the exact launches)
            got.append(ex.extract_device(vox.data_ptr(), desc, prm))
        got = got[3:]
        if not stages:
            row["ms_total"] = statistics.median(r.ms_total for r in got)
            row["ms_pass"] = statistics.median(r.ms_pass for r in got)
            row["ms_total_min_max"] = [min(r.ms_total for r in got), max(r.ms_total for r in got)]
        else:
            row["ms_project"] = statistics.median(r.ms_project for r in got)
            row["ms_classify"] = statistics.median(r.ms_classify for r in got)
            row["ms_classify_min_max"] = [min(r.ms_classify for r in got), max(r.ms_classify for r in got)]
    row["n_points"], row["n_cells"] = int(got[-1].n_points), int(got[-1].n_cells)
    row["proj_iterations"] = int(got[-1].proj_iterations)
    ex.close()
    print(json.dumps(row), flush=True)


def child(argv, timeout=600):
    out = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=timeout)
    if out.returncode != 0:
        raise RuntimeError("%s failed (%d):\n%s" % (" ".join(argv), out.returncode, out.stderr[-2000:]))
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--role", choices=["a", "b", "p"], default=None)
    ap.add_argument("--workload", choices=sorted(BANDS), default="labels")
    ap.add_argument("--tree", default="")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "band_extract.json"))
    a = ap.parse_args()
    if a.role:
        return role(a)
    if not a.parent_tree:
        sys.exit("--parent-tree: a checkout of the parent commit with its library built")
    parent = os.path.abspath(a.parent_tree)
    me = os.path.abspath(__file__)
    small = ["--small"] if a.small else []
    out = {"workloads": {"labels": "1024^3 uint8 nested-sphere labels 0..4, band 2..3, values 1 / 0, iso 1, bench walk",
                         "ml": "1024^3 float32 Marschner-Lobb, band 0.4..0.6, values 1 / 0, iso 1, bench walk"},
           "reps_per_process": REPS, "device": {}}
    med = statistics.median
    for workload in ("labels", "ml"):
        w = ["--workload", workload] + small
        rounds = []
        for _ in range(a.rounds):
            r = {"a": child([me, "--role", "a"] + w), "b": child([me, "--role", "b", "--tree", parent] + w),
                 "p": child([me, "--role", "p"] + w)}
            assert all(r["a"][k] == r["b"][k] for k in ("n_points", "n_cells", "proj_iterations")), r
            rounds.append(r)
            print(json.dumps({k: {f: v.get(f) for f in ("ms_threshold_copy", "ms_total", "ms_classify", "ms_project")} for k, v in r.items()}), flush=True)
        tot = {k: [r[k]["ms_total"] for r in rounds] for k in rounds[0]}
        sweep = {k: [r[k]["ms_classify"] for r in rounds] for k in rounds[0]}
        out["device"][workload] = {
            "rounds": rounds,
            "a_band_ms": med(tot["a"]), "a_spread_ms": max(tot["a"]) - min(tot["a"]),
            "b_extract_of_copy_ms": med(tot["b"]), "b_spread_ms": max(tot["b"]) - min(tot["b"]),
            "c_threshold_copy_ms": med(r["b"]["ms_threshold_copy"] for r in rounds),
            "b_plus_c_ms": med(r["b"]["ms_total"] + r["b"]["ms_threshold_copy"] for r in rounds),
            "sweep_ms": {k: med(v) for k, v in sweep.items()},
            "sweep_spread_ms": {k: max(v) - min(v) for k, v in sweep.items()},
            "walk_ms": {k: med(r[k]["ms_project"] for r in rounds) for k in rounds[0]},
        }
        with open(a.out, "w") as f:                    # (kept as it grows: a run cut short leaves what it had)
            json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
