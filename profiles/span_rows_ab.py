"""Same-box A/B of the row sweeps (k_classify_span_rows, k_classify_words) against the parent commit's library
(csrc/libcuberille_prev.so, built by `bash profiles/ab.sh`, selected through CUBERILLE_LIB): ms_classify with stage timing on,
the median of REPS warm extractions per process; parent and tree in alternating processes, three rounds, one session (the
protocol of profiles/ab.sh and profiles/border_pad.py).  The spread of the parent's three rounds is what one box does to an
unchanged kernel: the tree passes where its median of medians is at most the parent's median plus that spread.

Shapes: plain ragged rows -- the 1000^3 float32 sphere field and a 1000 x 1000 x 300 uint8 volume; the border -- the inner
1022^3 of marschner_lobb(1024) float32 with set_border(1, 0); the region -- a 1024^3 float32 box of a 1280 x 1152 x 1088 buffer.

    python profiles/span_rows_ab.py [--out profiles/span_rows_ab.json] [--shapes ...]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PREV = os.path.join(ROOT, "midas-journal-740_amd", "csrc", "libcuberille_prev.so")
REPS = 11
SHAPES = ("plain_f32_1000", "plain_u8_1000x1000x300", "border_f32_1022", "region_f32_1024")


def role(shape):
    """One shape in this process, with the library CUBERILLE_LIB names; prints one JSON line."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import __graft_entry__ as graft
    pkg = graft.load_package()
    ex = pkg.Extractor(0)
    ex.warm_up()
    iso = 0.5
    if shape == "plain_f32_1000":
        vox = pkg.volumes.sphere_sdf(1000, 0, 1000, xp=torch, device=torch.device("cuda", 0)).contiguous()
        desc, iso = pkg.make_desc(np.float32, (1000, 1000, 1000)), 0.0
    elif shape == "plain_u8_1000x1000x300":
        f = pkg.volumes.sphere_sdf(1000, 350, 650, xp=torch, device=torch.device("cuda", 0))
        vox = (f < 0).to(torch.uint8).mul_(200).contiguous()
        del f
        desc, iso = pkg.make_desc(np.uint8, (1000, 1000, 300)), 100
    elif shape == "border_f32_1022":
        vox = pkg.volumes.marschner_lobb(1024, xp=torch, device="cuda")[1:-1, 1:-1, 1:-1].contiguous()
        desc = pkg.make_desc(np.float32, (1022,) * 3)
        ex.set_border(1, 0)
    else:
        buf, start, size = (1280, 1152, 1088), (128, 64, 32), (1024, 1024, 1024)
        vox = pkg.volumes.marschner_lobb(buf[0], z0=0, z1=buf[2], xp=torch, device="cuda")[:, :buf[1], :].contiguous()
        desc = pkg.make_desc(np.float32, buf)
        ex.set_region(start, size)
    torch.cuda.synchronize()
    prm = pkg.make_params(iso, triangles=False, project=False)
    ex.debug_option("stage_timing", 1)
    got = [ex.extract_device(vox.data_ptr(), desc, prm) for _ in range(REPS + 3)][3:]   # (the first ones size the workspace)
    ms = [r.ms_classify for r in got]
    print(json.dumps({"shape": shape, "lib": os.path.basename(os.environ.get("CUBERILLE_LIB", "libcuberille_hip.so")),
                      "ms_classify": statistics.median(ms), "ms_classify_min_max": [min(ms), max(ms)],
                      "n_points": int(got[-1].n_points), "n_cells": int(got[-1].n_cells)}), flush=True)
    ex.close()


def child(shape, lib):
    env = dict(os.environ)
    env.pop("CUBERILLE_LIB", None)
    if lib:
        env["CUBERILLE_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", shape], capture_output=True, text=True, timeout=300, env=env)
    if out.returncode != 0:
        raise RuntimeError("%s with %s failed (%d):\n%s" % (shape, lib or "the tree's library", out.returncode, out.stderr[-2000:]))
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--role", default=None)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(HERE, "span_rows_ab.json"))
    a = ap.parse_args()
    if a.role:
        return role(a.role)
    out = {"quantity": "ms_classify, stage timing on, median of %d warm extractions per process" % REPS, "shapes": {}}
    for shape in a.shapes:
        rounds = []
        for _ in range(3):
            prev, tree = child(shape, PREV), child(shape, None)
            assert (prev["n_points"], prev["n_cells"]) == (tree["n_points"], tree["n_cells"]), (prev, tree)
            rounds.append({"parent": prev, "tree": tree})
        p, t = [r["parent"]["ms_classify"] for r in rounds], [r["tree"]["ms_classify"] for r in rounds]
        row = {"rounds": rounds, "parent_median": statistics.median(p), "parent_spread": max(p) - min(p),
               "tree_median": statistics.median(t), "tree_spread": max(t) - min(t)}
        row["within_gate"] = row["tree_median"] <= row["parent_median"] + row["parent_spread"]
        out["shapes"][shape] = row
        print("%-24s parent %.4f (spread %.4f)  tree %.4f (spread %.4f)  %s" % (
            shape, row["parent_median"], row["parent_spread"], row["tree_median"], row["tree_spread"],
            "within" if row["within_gate"] else "OUTSIDE"), flush=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
