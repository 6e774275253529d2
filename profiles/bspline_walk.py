"""The B-spline walk (cuberille_set_interpolator, CUBERILLE_INTERP_BSPLINE) on Marschner-Lobb float32 volumes with the bench's
walk parameters (iso 0.5, threshold 0.002, step 0.25, relaxation 0.95, at most 50 steps).

For each size: ms_project with stage timing on -- the linear walk, and the B-spline prefilter + walk -- and the bytes the
prefilter must move.  Per voxel, float coefficients, float input: the x pass reads the input (4), writes and reads the
double causal values (8 + 8) and writes the coefficients (4); the y and z passes read the coefficients (4), write and read
the causal values (8 + 8) and write the coefficients (4): 72 bytes.  The prefilter's kernels alone (k_bs_rows, k_bs_lines)
are timed by running this under `rocprofv3 --kernel-trace --stats` (profiles/bspline_kernel_stats.csv).  With --host-walk N,
the drop-in filter (itk/tests/bspline_walk.cxx filter) at N^3: the device route, and the host route with 16 and 1 threads.
Each is the LAST of several Update() calls on one filter (warm: context, workspace, code objects set up; the first one of a
process also reserves the coefficient image), split into the filter's own intervals: device time, the extraction call
(upload + device work), the download and the itk::Mesh fill -- the last three both routes share; the host route adds its
walk (its single-threaded prefilter of the user's interpolator object included) and its triangle split on top.

    python profiles/bspline_walk.py --sizes 512 1024 --host-walk 256 [--out profiles/bspline_walk.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import __graft_entry__ as graft  # noqa: E402

PREFILTER_BYTES_PER_VOXEL = 72          # float coefficients, float input (see the head of this file)
ISO = 0.5
WALK = dict(threshold=0.002, step=0.25, relax=0.95, max_steps=50)   # bench.py's workload


def stage_ms(pkg, ex, vox_dev, desc, prm, bspline, reps=3):
    A = pkg._abi
    ex.set_interpolator(A.INTERP_BSPLINE if bspline else A.INTERP_LINEAR, 3, 32, 32)
    best = None
    for _ in range(reps + 1):                     # (the first one warms the workspace up)
        res = ex.extract_device(vox_dev, desc, prm)
        if best is None or res.ms_project < best.ms_project:
            best = res
    ex.set_interpolator(A.INTERP_LINEAR)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--host-walk", type=int, default=0, help="edge of the volume the host route is timed at (0: not)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = graft.load_package()
    import torch
    ex = pkg.Extractor(0)
    ex.debug_option("stage_timing", 1)
    out = {"iso": ISO, "sizes": {}}
    for n in a.sizes:
        vox = pkg.volumes.marschner_lobb(n, xp=torch, device="cuda").contiguous()
        torch.cuda.synchronize()
        desc = pkg.make_desc(np.float32, (n, n, n))
        prm = pkg.make_params(ISO, **WALK)
        lin = stage_ms(pkg, ex, vox.data_ptr(), desc, prm, False)
        bs = stage_ms(pkg, ex, vox.data_ptr(), desc, prm, True)
        row = {"n_points": int(bs.n_points), "linear_ms_project": lin.ms_project, "bspline_ms_project": bs.ms_project,
               "linear_iterations": int(lin.proj_iterations), "bspline_iterations": int(bs.proj_iterations),
               "prefilter_bytes": PREFILTER_BYTES_PER_VOXEL * n ** 3}
        out["sizes"][str(n)] = row
        print(json.dumps({"n": n, **row}), flush=True)
        del vox
        torch.cuda.empty_cache()
    ex.close()
    if a.host_walk:
        import bspline_ref as ref
        n = a.host_walk
        vox = pkg.volumes.marschner_lobb(n).astype(np.float32)
        with tempfile.TemporaryDirectory() as tmp:
            raw = os.path.join(tmp, "ml.raw")
            vox.tofile(raw)
            host = {}
            for route, threads, repeat in (("device", 1, 5), ("host", 16, 3), ("host", 1, 2)):
                t0 = time.time()
                r = subprocess.run([ref.walk_exe(), "filter", raw, route, str(threads), "32", repr(ISO), "1", "1", repr(WALK["threshold"]),
                                    repr(WALK["step"]), repr(WALK["relax"]), str(WALK["max_steps"]), os.path.join(tmp, "p.raw"), os.path.join(tmp, "c.raw"),
                                    "raw", "f32", str(n), str(n), str(n), "repeat", str(repeat)], capture_output=True, text=True, timeout=3000)
                assert r.returncode == 0, r.stderr
                pts, cells, secs, dev_s, ext_s, dl_s, fill_s = r.stdout.split()[:7]
                host["%s_%d" % (route, threads)] = {"update_s": float(secs), "device_s": float(dev_s), "extract_s": float(ext_s),
                                                   "download_s": float(dl_s), "mesh_fill_s": float(fill_s), "updates": repeat,
                                                   "process_s": time.time() - t0, "points": int(pts), "cells": int(cells)}
                print(json.dumps({"n": n, "route": route, "threads": threads, **host["%s_%d" % (route, threads)]}), flush=True)
        out["host_walk"] = {"n": n, **host,
                            "speedup_vs_host16": host["host_16"]["update_s"] / host["device_1"]["update_s"]}
        print(json.dumps({"speedup_vs_host16": out["host_walk"]["speedup_vs_host16"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
