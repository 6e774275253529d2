"""The project's CPU sides that the witnesses of tests/independent_ref.py are compared with: the reference's own filter binary
where oracle/_ref/ holds it, else the oracle (tests/test_reference_filter.py holds the two to each other bit for bit); for the
B-spline walk the drop-in's host walk (itk/build/bspline_walk, held to the reference binary there too).  Shared by
tests/test_independent.py and tests/golden/make_independent_tolerances.py.  TEST INFRASTRUCTURE ONLY."""
import json
import os
import subprocess
import tempfile

import numpy as np

import bspline_ref
import independent_ref as ind
import ref_filter as rf

TOLERANCES = os.path.join(rf.GOLDEN, "independent_tolerances.json")
FACTOR = 4.0                      # every test allows this many times the recorded deviation
COEFFICIENT_SHAPES = [(2, 3, 5), (7, 9, 13), (18, 19, 20), (40, 33, 70), (5, 4, 259)]      # [z, y, x]


_RECORDED = None


def allowed(family):
    """FACTOR times the deviation tests/golden/independent_tolerances.json records for the family."""
    global _RECORDED
    if _RECORDED is None:
        with open(TOLERANCES) as f:
            _RECORDED = json.load(f)
        assert _RECORDED["factor"] == FACTOR
    return FACTOR * _RECORDED["families"][family]


def geometry_of(case):
    """spacing, origin, direction and start index of the MATERIALISED image of the case, as oracle.run takes them."""
    img = ind.image_of(case)
    return dict(spacing=tuple(img.spacing), origin=tuple(img.origin), direction=img.direction, index_start=tuple(int(s) for s in img.start))


def walk_kw(case):
    return dict(threshold=case["threshold"], step=case["step"], relax=case["relax"], max_steps=case["max_steps"])


def start_points(oracle, case):
    """The lattice points the sweep emits with the projection off (float32 [n, 3])."""
    vox, _ = ind.materialised(case)
    return oracle.run(vox, case["iso"], triangles=0, project=0, **geometry_of(case)).points


def _reference_binary(case, vox, geo):
    lines = ["pixel %s" % rf.PIXEL_NAMES[vox.dtype], "interp linear"]
    lines += rf._geometry_lines("", vox, dict(spacing=geo["spacing"], origin=geo["origin"], direction=geo["direction"], start=geo["index_start"]))
    lines += rf.iso_lines(vox.dtype, case["iso"])
    lines += ["triangles 0", "project 1", "threshold %s" % float(case["threshold"]).hex(), "step %s" % float(case["step"]).hex(),
              "relax %s" % float(case["relax"]).hex(), "max_steps %d" % int(case["max_steps"]), "pad 0"]
    with tempfile.TemporaryDirectory() as tmp:
        cpath, opath = os.path.join(tmp, "case"), os.path.join(tmp, "mesh")
        with open(cpath, "wb") as f:
            f.write(("\n".join(lines) + "\nend\n").encode("ascii"))
            f.write(vox.astype(vox.dtype.newbyteorder("<")).tobytes())
        p = subprocess.run([rf.binary(case["variant"]), cpath, opath], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert p.returncode == 0, (case["name"], p.stdout.decode(errors="replace")[-2000:])
        raw = open(opath, "rb").read()
    n = int(np.frombuffer(raw, dtype="<u8", count=1)[0])
    return np.frombuffer(raw, dtype="<f4", count=3 * n, offset=24).reshape(n, 3).copy()


def reference_walk(oracle, case, start=None):
    """The final vertices (float32 [n, 3]) of the case on the project's CPU side, and which side that was."""
    vox, _ = ind.materialised(case)
    geo = geometry_of(case)
    if case["interp"].startswith("bspline"):
        assert case["variant"] == 0 and not case["gradient"]
        start = start_points(oracle, case) if start is None else start
        bits = case["interp"][len("bspline"):]
        nz, ny, nx = vox.shape
        with tempfile.TemporaryDirectory() as tmp:
            raw, sp, op = (os.path.join(tmp, k) for k in "vso")
            vox.tofile(raw)
            np.ascontiguousarray(start, dtype="<f4").tofile(sp)
            r = subprocess.run([bspline_ref.walk_exe(), "walk", raw, rf.PIXEL_NAMES[vox.dtype], str(nx), str(ny), str(nz), bits,
                                bspline_ref.geometry_arg(geo["spacing"], geo["origin"], geo["direction"], geo["index_start"]),
                                repr(float(case["iso"])), repr(float(case["threshold"])), repr(float(case["step"])), repr(float(case["relax"])),
                                str(case["max_steps"]), sp, str(len(start)), op], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, (case["name"], r.stdout, r.stderr)
            return np.fromfile(op, dtype="<f4").reshape(-1, 3), "host walk"
    if not case["gradient"] and rf.available(case["variant"]):
        return _reference_binary(case, vox, geo), "reference binary"
    m = oracle.run(vox, case["iso"], triangles=0, project=1, variant=case["variant"], gradient=case["gradient"], **dict(walk_kw(case), **geo))
    return m.points, "oracle"


def oracle_counters(oracle, case):
    vox, _ = ind.materialised(case)
    m = oracle.run(vox, case["iso"], triangles=0, project=1, variant=case["variant"], gradient=case["gradient"],
                   **dict(walk_kw(case), **geometry_of(case)))
    return m.info


_WITNESSED = {}


def witnessed(case, start):
    """(Witness, its walk from `start`, the fragile mask), once per case and start points."""
    key = (case["name"], np.ascontiguousarray(start).tobytes())
    if key not in _WITNESSED:
        wit = ind.Witness(case)
        walk = wit.walk(start)
        _WITNESSED[key] = (wit, walk, wit.fragility(start, walk))
    return _WITNESSED[key]


def family_of(case):
    if case["gradient"]:
        return "gaussian_walk"
    if case["interp"].startswith("bspline"):
        return "bspline_walk_" + case["interp"][len("bspline"):]
    return "linear_walk_v%d" % case["variant"]


def coefficient_volume(shape, dtype, seed=17):
    rng = np.random.default_rng(seed + sum(shape))
    dtype = np.dtype(dtype)
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        return rng.integers(info.min, info.max, size=shape, dtype=dtype, endpoint=True)
    return (rng.standard_normal(shape) * 100.0).astype(dtype)


def coefficient_deviation(got, vox):
    """max |got - scipy's coefficients| as a share of the largest coefficient."""
    want = ind.bspline_coefficients(vox)
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())
