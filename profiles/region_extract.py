"""What extracting a box in place (cuberille_set_region) costs against the route a caller had to take before: a cropped copy,
then the extraction of the copy with its start index kept.  Same box, same session, warm, medians; every timed leg is a
process of its own, alternated three times (the spread of the three is the yardstick, as in profiles/border_pad.py).

Workload: the 1024^3 box at buffer position (128, 64, 32) of a 1280 x 1152 x 1088 float32 Marschner-Lobb volume (the first 1088
slices and 1152 rows of volumes.marschner_lobb(1280)), iso 0.5, triangles + projection with bench.py's walk -- as an identity
image, and a second time as an axis-aligned one with spacing (0.7, 0.7, 2.5).
  A: the PARENT commit's package (--parent-tree: a checkout of it with its library built): the crop copy, timed by events
     (torch .contiguous() of the view), + extract_device of the copy with index_start = the box's place
  B: this tree, set_region on the whole buffer
  C: either package on the contiguous copy with the region off and index_start 0 (the fast walk forms' reference time)
ms_total / ms_pass are medians of plain extractions, ms_classify / ms_project of extractions with stage timing on.
Host route (--host N): itk/tests/region_update --synthetic N, the central (N/2)^3 box: host crop loop + Update() against
SetExtractionRegion + Update().

The kernels of leg B alone: `--role B` under `rocprofv3 --kernel-trace --stats`, a run of its own.

    python profiles/region_extract.py --parent-tree DIR [--host 1024] [--out profiles/region_extract.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ISO = 0.5
WALK = dict(threshold=0.002, step=0.25, relax=0.95, max_steps=50)   # bench.py's workload
REPS = 9
BUF, START, SIZE = (1280, 1152, 1088), (128, 64, 32), (1024, 1024, 1024)


def role(args):
    """One timed leg in this process; prints one JSON line.  A and a parent's C import the package of --tree and never name
    the new symbol."""
    tree = os.path.abspath(args.tree) if args.tree else ROOT
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import __graft_entry__ as graft
    pkg = graft.load_package()
    buf, start, size = BUF, START, SIZE
    if args.small:                                   # (a quick functional pass of the script itself)
        buf, start, size = (320, 288, 272), (32, 16, 8), (256, 256, 256)
    whole = pkg.volumes.marschner_lobb(buf[0], z0=0, z1=buf[2], xp=torch, device="cuda")[:, :buf[1], :].contiguous()
    view = whole[start[2]:start[2] + size[2], start[1]:start[1] + size[1], start[0]:start[0] + size[0]]
    torch.cuda.synchronize()
    spacing = tuple(args.spacing)
    row = {"role": args.role, "spacing": list(spacing), "tree": "parent" if args.tree else "tree"}
    if args.role == "A":
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ms = []
        for _ in range(REPS + 2):
            ev[0].record()
            vox = view.contiguous()
            ev[1].record()
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        row["ms_crop_copy"] = statistics.median(ms[2:])
        desc = pkg.make_desc(np.float32, size, spacing=spacing, index_start=start)
    elif args.role == "C":
        vox = view.contiguous()
        desc = pkg.make_desc(np.float32, size, spacing=spacing)
    else:
        vox = whole
        desc = pkg.make_desc(np.float32, buf, spacing=spacing)
    torch.cuda.synchronize()
    ex = pkg.Extractor(0)
    ex.warm_up()
    if args.role == "B":
        ex.set_region(start, size)
    prm = pkg.make_params(ISO, **WALK)
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
    row["n_points"], row["n_cells"] = int(got[-1].n_points), int(got[-1].n_cells)
    row["proj_iterations"] = int(got[-1].proj_iterations)
    ex.close()
    print(json.dumps(row), flush=True)


def child(argv, cwd=None, timeout=600):
    out = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=timeout, cwd=cwd)
    if out.returncode != 0:
        raise RuntimeError("%s failed (%d):\n%s" % (" ".join(argv), out.returncode, out.stderr[-2000:]))
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--role", choices=["A", "B", "C"], default=None)
    ap.add_argument("--tree", default="")
    ap.add_argument("--spacing", type=float, nargs=3, default=[1.0, 1.0, 1.0])
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--host", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "region_extract.json"))
    a = ap.parse_args()
    if a.role:
        return role(a)
    if not a.parent_tree:
        sys.exit("--parent-tree: a checkout of the parent commit with its library built")
    parent = os.path.abspath(a.parent_tree)
    me = os.path.abspath(__file__)
    small = ["--small"] if a.small else []
    out = {"workload": "box %s at %s of a %s float32 Marschner-Lobb buffer, iso %g, bench walk" % (SIZE, START, BUF, ISO),
           "reps_per_process": REPS, "device": {}}
    med = statistics.median
    for spacing in ((1.0, 1.0, 1.0), (0.7, 0.7, 2.5)):
        sp = ["--spacing"] + [str(v) for v in spacing]
        rounds = []
        for _ in range(a.rounds):
            r = {"A": child([me, "--role", "A", "--tree", parent] + sp + small),
                 "B": child([me, "--role", "B"] + sp + small),
                 "C_parent": child([me, "--role", "C", "--tree", parent] + sp + small),
                 "C_tree": child([me, "--role", "C"] + sp + small)}
            # (A and B mesh the same image; C's start index is 0, so its coordinates round elsewhere: the two libraries alike)
            same = lambda x, y: all(r[x][k] == r[y][k] for k in ("n_points", "n_cells", "proj_iterations"))
            assert same("A", "B") and same("C_parent", "C_tree"), r
            rounds.append(r)
            print(json.dumps({k: {f: v.get(f) for f in ("ms_crop_copy", "ms_total", "ms_classify", "ms_project")} for k, v in r.items()}), flush=True)
        tot = {k: [r[k]["ms_total"] for r in rounds] for k in rounds[0]}
        a_whole = [r["A"]["ms_total"] + r["A"]["ms_crop_copy"] for r in rounds]
        out["device"]["spacing %g %g %g" % spacing] = {
            "rounds": rounds,
            "A_copy_plus_extract_ms": med(a_whole), "A_crop_copy_ms": med(r["A"]["ms_crop_copy"] for r in rounds),
            "A_extract_ms": med(tot["A"]), "B_ms": med(tot["B"]), "B_spread_ms": max(tot["B"]) - min(tot["B"]),
            "A_spread_ms": max(tot["A"]) - min(tot["A"]),
            "C_parent_ms": med(tot["C_parent"]), "C_tree_ms": med(tot["C_tree"]),
            "C_spread_ms": max(max(tot["C_parent"]) - min(tot["C_parent"]), max(tot["C_tree"]) - min(tot["C_tree"])),
            "sweep_ms": {k: med(r[k]["ms_classify"] for r in rounds) for k in rounds[0]},
            "walk_ms": {k: med(r[k]["ms_project"] for r in rounds) for k in rounds[0]},
        }
        with open(a.out, "w") as f:                    # (kept as it grows: a run cut short leaves what it had)
            json.dump(out, f, indent=1)
    if a.host:
        exe = os.path.join(ROOT, "midas-journal-740_amd", "itk", "build", "region_update")
        n = a.host
        run = subprocess.run([exe, "--synthetic", str(n), str(ISO)] + [str(n // 4)] * 3 + [str(n // 2)] * 3,
                             capture_output=True, text=True, timeout=900)
        out["host"] = {"n": n, "box": n // 2, "returncode": run.returncode, "region_update": run.stdout.strip()}
        print(run.stdout.strip(), run.stderr[-500:], flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
