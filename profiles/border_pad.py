"""What the implied border (cuberille_set_border) costs against the route a caller had to take before: a padded copy, then the
extraction of the padded buffer.  Same box, same session, warm, medians; every timed extraction is a process of its own,
alternated old / new three times (the spread of the three is the yardstick, as in profiles/ab.sh).

1. Device-resident float32 Marschner-Lobb whose surface meets the border: the inner N^3 of volumes.marschner_lobb(N + 2) --
   padded by one voxel of 0 it IS that volume, so both routes extract the same image.
     new: this tree's library, set_border(1, 0), the N^3 buffer                     -> ms_total, ms_pass, ms_project
     old: the PARENT commit's package (--parent-tree: a checkout of it with its library built), the explicitly padded
          (N + 2)^3 buffer with index_start - 1                                     -> the same three
          + the device-side pad copy the old route needs first (torch.nn.functional.pad)
   ms_total / ms_pass are medians of plain extractions, ms_project of extractions with stage timing on.
2. Host-resident N^3 float32 through the drop-in filter: itk/tests/pad_update.cxx -- itk::ConstantPadImageFilter, then the
   filter, against PadBorderOn() -- with the pad filter's time shown separately (--host N; 0: not).
3. The unpadded default on the same box: bench.py --gpus 1 of the parent's tree and of this one, alternated.

The kernels of the new route alone: run `--role new --n N` under `rocprofv3 --kernel-trace --stats` (a run of its own).

    python profiles/border_pad.py --parent-tree DIR [--sizes 1022 1024] [--host 1024] [--out profiles/border_pad.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ISO = 0.5
WALK = dict(threshold=0.002, step=0.25, relax=0.95, max_steps=50)   # bench.py's workload
REPS = 9


def role(args):
    """One timed route in this process; prints one JSON line.  `old` imports the package of --tree (the parent's checkout)
    and never names the new symbol."""
    tree = os.path.abspath(args.tree) if args.tree else ROOT
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import __graft_entry__ as graft
    pkg = graft.load_package()
    n = args.n
    inner = pkg.volumes.marschner_lobb(n + 2, xp=torch, device="cuda")[1:-1, 1:-1, 1:-1].contiguous()
    torch.cuda.synchronize()
    row = {"role": args.role, "n": n}
    if args.role == "old":
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        pad_ms = []
        for _ in range(REPS + 2):
            ev[0].record()
            vox = torch.nn.functional.pad(inner, (1, 1, 1, 1, 1, 1))
            ev[1].record()
            torch.cuda.synchronize()
            pad_ms.append(ev[0].elapsed_time(ev[1]))
        row["ms_pad_copy"] = statistics.median(pad_ms[2:])
        del inner
        desc = pkg.make_desc(np.float32, (n + 2,) * 3, index_start=(-1, -1, -1))
    else:
        vox = inner
        desc = pkg.make_desc(np.float32, (n,) * 3)
    ex = pkg.Extractor(0)
    ex.warm_up()
    if args.role == "new":
        ex.set_border(1, 0)
    prm = pkg.make_params(ISO, **WALK)
    torch.cuda.synchronize()
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
    ap.add_argument("--role", choices=["new", "old"], default=None)
    ap.add_argument("--n", type=int, default=1022)
    ap.add_argument("--tree", default="")
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--sizes", type=int, nargs="*", default=[1022, 1024])
    ap.add_argument("--host", type=int, default=1024)
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "border_pad.json"))
    a = ap.parse_args()
    if a.role:
        return role(a)
    if not a.parent_tree:
        sys.exit("--parent-tree: a checkout of the parent commit with its library built")
    parent = os.path.abspath(a.parent_tree)
    me = os.path.abspath(__file__)
    out = {"workload": "inner N^3 of marschner_lobb(N + 2) float32, iso %g, bench walk" % ISO, "reps_per_process": REPS, "device": {}}
    for n in a.sizes:
        rounds = []
        for _ in range(3):
            old = child([me, "--role", "old", "--n", str(n), "--tree", parent])
            new = child([me, "--role", "new", "--n", str(n)])
            assert (old["n_points"], old["n_cells"], old["proj_iterations"]) == (new["n_points"], new["n_cells"], new["proj_iterations"])
            rounds.append({"old": old, "new": new})
            print(json.dumps({"n": n, "old_ms_total": old["ms_total"], "old_ms_pad_copy": old["ms_pad_copy"],
                              "new_ms_total": new["ms_total"]}), flush=True)
        olds, news = [r["old"]["ms_total"] for r in rounds], [r["new"]["ms_total"] for r in rounds]
        out["device"][str(n)] = {
            "rounds": rounds,
            "old_ms_total_median": statistics.median(olds), "old_ms_total_spread": max(olds) - min(olds),
            "old_ms_pad_copy_median": statistics.median(r["old"]["ms_pad_copy"] for r in rounds),
            "new_ms_total_median": statistics.median(news), "new_ms_total_spread": max(news) - min(news),
            "new_minus_old_ms": statistics.median(news) - statistics.median(olds),
        }
    if a.host:
        sys.path.insert(0, ROOT)
        import numpy as np
        import __graft_entry__ as graft
        pkg = graft.load_package()
        n = a.host
        inner = np.ascontiguousarray(pkg.volumes.marschner_lobb(n + 2).astype(np.float32)[1:-1, 1:-1, 1:-1])
        exe = os.path.join(ROOT, "midas-journal-740_amd", "itk", "build", "pad_update")
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "inner.mha")
            pkg.write_mha(path, pkg.Volume(inner), compress=False)
            del inner
            run = subprocess.run([exe, path, str(ISO), "0", "1"], capture_output=True, text=True, timeout=900)
        out["host"] = {"n": n, "returncode": run.returncode, "pad_update": run.stdout.strip()}
        print(run.stdout.strip(), run.stderr[-500:], flush=True)
    if not a.no_bench:
        rows = []
        for _ in range(3):
            for name, tree in (("parent", parent), ("tree", ROOT)):
                d = child([os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree)
                rows.append({"which": name, "ms_per_step": d["ms_per_step"], "pass_ms": d["roofline"]["pass_ms"]})
                print(json.dumps(rows[-1]), flush=True)
        out["bench_default_unpadded"] = rows
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
