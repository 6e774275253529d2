"""What cuberille_keep_components costs, what it replaces, and that the extraction beside it is what it was.  The 1024^3 uint8
gradient-noise extraction of bench.py (iso 128, triangles + projection: 31.0 M points, 61.9 M triangles, K = 168), device
resident, warm, medians; every timed leg is a process of its own, alternated three times (the spread of the three is the
yardstick, as in profiles/components.py).

Legs:
  par:  the PARENT commit's package (--parent-tree: a checkout of it with its library built), components on
  on:   this tree, components on -- the new function is never called: the two must lie within the run's own A/B spread
  keep: this tree, components on, and behind every extraction one cuberille_keep_components -- `ms` of LARGEST and of
        MIN_CELLS 1000, each on a fresh extraction, and the kept sizes
  host: the route the keep replaces, once: download() + download_components() + tests/keep_ref.py on the host, wall time
The expectation (no gate): the keep below the extraction of the same volume with components off, 3.26 ms in
profiles/components.json.

The kernels: `--role keep` under `rocprofv3 --kernel-trace --stats`, a run of its own
(profiles/keep_components_kernel_stats.csv).

    python profiles/keep_components.py --parent-tree DIR [--out profiles/keep_components.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REPS = 9
MIN_CELLS = 1000


def role(args):
    """One timed leg in this process; prints one JSON line.  Leg par imports the package of --tree and never names the new symbol."""
    tree = os.path.abspath(args.tree) if args.tree else ROOT
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import __graft_entry__ as graft
    import bench
    pkg = graft.load_package()
    n = 256 if args.small else 1024                  # (--small: a quick functional pass of the script itself)
    ex = pkg.Extractor(0)
    ex.warm_up()
    dtype, iso, thr = bench.WORKLOADS["noise"]
    vol = bench.generate_block(pkg, torch, "noise", n, 0, n, None, "cuda")
    torch.cuda.synchronize()
    row = {"role": args.role, "n": n, "tree": "parent" if args.tree else "tree"}
    desc = pkg.make_desc(dtype, (n, n, n))
    ex.set_components(True)
    prm = pkg.make_params(iso, triangles=True, project=True, threshold=thr, step=0.25, relax=0.95, max_steps=50)
    got = [ex.extract_device(vol.data_ptr(), desc, prm) for _ in range(REPS + 3)][3:]    # (the first ones size the workspace)
    row["ms_total"] = statistics.median(r.ms_total for r in got)
    row["ms_total_min_max"] = [min(r.ms_total for r in got), max(r.ms_total for r in got)]
    row["n_points"], row["n_cells"], row["n_components"] = int(got[-1].n_points), int(got[-1].n_cells), int(ex.n_components())
    if args.role in ("keep", "host"):
        counts = ex.download_components()[2]
        row["largest_components_cells"] = [int(v) for v in np.sort(counts)[::-1][:4]]
    if args.role == "keep":
        for name, rule, bound in (("largest", "largest", 0), ("min_cells_%d" % MIN_CELLS, "min_cells", MIN_CELLS)):
            ms, sizes = [], None
            for _ in range(REPS + 1):
                ex.extract_device(vol.data_ptr(), desc, prm)
                out = ex.keep_components(rule, bound)
                ms.append(out[3])
                sizes = out[:3]
            ms = ms[1:]                                # (the first call reserves the spare rows)
            row[name] = {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)], "n_points": sizes[0], "n_cells": sizes[1],
                         "n_components": sizes[2]}
            # kept twice in a row: everything is kept, no compaction kernel runs
            row[name]["ms_when_all_is_kept"] = ex.keep_components(rule, bound)[3]
    if args.role == "host":
        import keep_ref
        ex.extract_device(vol.data_ptr(), desc, prm)
        t0 = time.perf_counter()
        mesh = ex.download()
        rows = ex.download_components()
        t1 = time.perf_counter()
        row["download_s"] = t1 - t0
        for name, rule, bound in (("largest", "largest", 0), ("min_cells_%d" % MIN_CELLS, "min_cells", MIN_CELLS)):
            t1 = time.perf_counter()
            kept = keep_ref.apply(rule, mesh.points, mesh.cells, *rows, n=bound)
            row[name] = {"host_filter_s": time.perf_counter() - t1, "n_points": len(kept.points), "n_cells": len(kept.cells)}
            got = ex.keep_components(rule, bound)
            assert got[:3] == (len(kept.points), len(kept.cells), len(kept.component_cells)), (got, name)
            after = ex.download()
            assert after.points.tobytes() == kept.points.tobytes() and after.cells.tobytes() == kept.cells.tobytes(), name
            row[name]["device_result_equals_host_filter"] = True
            ex.extract_device(vol.data_ptr(), desc, prm)
    ex.close()
    print(json.dumps(row), flush=True)


def child(argv, timeout=900):
    out = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=timeout)
    if out.returncode != 0:
        raise RuntimeError("%s failed (%d):\n%s" % (" ".join(argv), out.returncode, out.stderr[-2000:]))
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--role", choices=["par", "on", "keep", "host"], default=None)
    ap.add_argument("--tree", default="")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "keep_components.json"))
    a = ap.parse_args()
    if a.role:
        return role(a)
    if not a.parent_tree:
        sys.exit("--parent-tree: a checkout of the parent commit with its library built")
    parent = os.path.abspath(a.parent_tree)
    me = os.path.abspath(__file__)
    small = ["--small"] if a.small else []
    med = statistics.median
    out = {"workload": "1024^3 uint8 gradient noise, iso 128, bench walk, components on", "reps_per_process": REPS,
           "expectation_ms": 3.26, "rounds": []}
    for _ in range(a.rounds):
        r = {"par": child([me, "--role", "par", "--tree", parent] + small), "on": child([me, "--role", "on"] + small),
             "keep": child([me, "--role", "keep"] + small)}
        assert all(r["par"][k] == r["on"][k] == r["keep"][k] for k in ("n_points", "n_cells", "n_components")), r
        out["rounds"].append(r)
        print(json.dumps({k: v["ms_total"] for k, v in r.items()}), json.dumps({k: v["ms"] for k, v in r["keep"].items()
                                                                                  if isinstance(v, dict)}), flush=True)
        rounds = out["rounds"]
        tot = {k: [x[k]["ms_total"] for x in rounds] for k in ("par", "on", "keep")}
        out["extraction_ms_total"] = {k: med(v) for k, v in tot.items()}
        out["extraction_spread_ms"] = {k: max(v) - min(v) for k, v in tot.items()}
        out["on_minus_parent_ms"] = med(tot["on"]) - med(tot["par"])
        for name in ("largest", "min_cells_%d" % MIN_CELLS):
            ms = [x["keep"][name]["ms"] for x in rounds]
            out["keep_" + name] = dict(rounds[-1]["keep"][name], ms=med(ms), ms_of_the_rounds=ms,
                                       below_the_expectation=med(ms) < out["expectation_ms"])
        with open(a.out, "w") as f:                    # (kept as it grows: a run cut short leaves what it had)
            json.dump(out, f, indent=1)
    out["host_route"] = child([me, "--role", "host"] + small, timeout=1500)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
