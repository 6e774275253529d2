"""Point scalars without a GPU (cuberille_set_point_scalars): the new symbols exist and refuse a null context; the reference
the GPU tests hold the kernel to (tests/point_scalars_ref.py: the oracle's interpolation primitive plus the inside test)
agrees with an independent witness (tests/independent_ref.py: np.linalg.inv and scipy's map_coordinates) at the oracle's
points of the GPU tests' cases that lie at least a voxel inside the second image; and the host-only table of the new row
(csrc/tests/point_scalars_table.hip), plain and under the address and undefined-behaviour sanitizers.

The cases of the GPU tests (tests/test_gpu_point_scalars.py) are defined here, so that both files speak of the same ones.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import independent_ref
import point_scalars_ref
from conftest import ROOT
from test_normals import GEOMETRIES, blob, rot

NEW = ("cuberille_set_point_scalars", "cuberille_point_scalars_device", "cuberille_point_scalars_download")
CSRC = os.path.join(ROOT, "midas-journal-740_amd", "csrc")
TOLERANCE = os.path.join(ROOT, "tests", "golden", "point_scalars_tolerance.json")
ALL_TYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64, np.int64, np.uint64]


def typed_noise(dtype, shape=(5, 7, 9), seed=23):
    """Noise of `shape` ([z, y, x]) in the type; the 4- and 8-byte integers scaled past 2^24 / 2^53, where (float) and (double)
    round (the scales of test_gpu_normals.typed_blob)."""
    dt = np.dtype(dtype)
    f = np.random.default_rng(seed).random(shape) * 100.0
    if dt.kind == "f":
        return (f - 40.0).astype(dt)
    scale = {1: 1, 2: 300, 4: 20000001, 8: (1 << 55) + 12345}[dt.itemsize]
    shift = 50 if dt.kind == "i" else 0
    return np.array([int((v - shift) * scale) for v in f.reshape(-1)], dtype=object).astype(dt).reshape(shape)


# Case 1: B of 9 x 7 x 5 under an identity geometry at origin (2, 3, 1), on test_normals.blob() (14 x 12 x 10).
CASE1_GEO = dict(origin=(2.0, 3.0, 1.0))
# Case 2: the blob under GEOMETRIES["spacing"] / ["rotated"] with a start index of (5, -3, 7); B of 12 x 10 x 8 with spacing
# (1.1, 0.9, 1.7), index_start (2, -1, 3), direction rot(1, 0.3) or rot(1, 0.3) @ rot(2, -0.2), origin (4, 0.5, 14) -- moved to
# (10, -28, 14) under "rotated", where the mesh lies elsewhere -- so that at least a tenth of the points are inside and a tenth
# outside (asserted by the GPU test; here on the CPU 53-97 and 56-79 of the oracle's 302 points are inside)
CASE2_START = (5, -3, 7)
CASE2_SHAPE = (8, 10, 12)
CASE2_DIRECTIONS = {"r1": rot(1, 0.3), "r12": rot(1, 0.3) @ rot(2, -0.2)}
CASE2_ORIGIN = {"spacing": (4.0, 0.5, 14.0), "rotated": (10.0, -28.0, 14.0)}


def case2_geo(geometry, direction):
    return dict(spacing=(1.1, 0.9, 1.7), origin=CASE2_ORIGIN[geometry], index_start=(2, -1, 3), direction=CASE2_DIRECTIONS[direction])


def witness_cases(oracle):
    """(name, B, B's geometry, the oracle's points) of the cases the witness is held against."""
    vol, iso = blob()
    out = []
    for project in (True, False):
        pts = oracle.run(vol, iso, project=project).points
        for dtype in (np.uint8, np.int16, np.float32, np.float64):
            out.append(("case1/%s/%d" % (np.dtype(dtype).name, project), typed_noise(dtype), CASE1_GEO, pts))
        for geometry in ("spacing", "rotated"):
            p2 = oracle.run(vol, iso, project=project, index_start=CASE2_START, **GEOMETRIES[geometry]).points
            for direction in CASE2_DIRECTIONS:
                out.append(("case2/%s/%s/%d" % (geometry, direction, project), typed_noise(np.float32, CASE2_SHAPE), case2_geo(geometry, direction), p2))
    return out


def witness_difference(oracle, b, geo, points):
    """The largest |oracle primitive - witness| over the points at least a voxel inside B, relative to max |B|; and how many."""
    g = point_scalars_ref.geo_of(geo)
    img = independent_ref.Image(b, g["spacing"], g["origin"], g["direction"], g["index_start"])
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    deep = img.face_distance(p) >= 1.5            # (the faces lie half a voxel outside the outermost centres)
    deep &= np.isfinite(p).all(axis=1)
    if not deep.any():
        return 0.0, 0
    ours = point_scalars_ref.interpolated(oracle, b, points[deep], **geo)
    theirs = independent_ref.linear_value(img)(p[deep])
    return float(np.abs(ours - theirs).max() / np.abs(b.astype(np.float64)).max()), int(deep.sum())


def test_symbols_in_header_binding_and_library(pkg):
    header = open(os.path.join(ROOT, "include", "cuberille_hip.h")).read()
    lib = pkg._abi.lib()
    dyn = subprocess.run(["nm", "-D", pkg._abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), name + " is not declared in the header"
        assert name in pkg._abi.EXPORTS, name + " is not in _abi.EXPORTS"
        assert re.search(r" T %s$" % name, dyn, re.M), name + " is not exported by the library"
        assert getattr(lib, name).argtypes is not None
    assert re.search(r"CUBERILLE_MEM_HOST = 0, CUBERILLE_MEM_DEVICE = 1", header)
    assert (pkg._abi.MEM_HOST, pkg._abi.MEM_DEVICE) == (0, 1)
    for kernel in ("k_point_scalars", "k_keep_scatter_point_scalars"):
        assert kernel in dyn, "no %s kernel in the library" % kernel
    assert lib.cuberille_abi_version() == pkg._abi.ABI_VERSION == 13
    for n in ("set_point_scalars", "download_point_scalars", "point_scalars_device"):
        assert callable(getattr(pkg.Extractor, n)), n
    assert callable(pkg.ExtractorGroup.set_point_scalars)
    for n in ("SetPointScalarImage", "SetPointScalarOutsideValue", "GetPointScalars"):
        assert callable(getattr(pkg.CuberilleImageToMeshFilter, n)), n


def test_null_context_is_an_argument_error(pkg):
    lib = pkg._abi.lib()
    desc = pkg.make_desc(np.uint8, (2, 2, 2))
    vox = np.zeros(8, np.uint8)
    assert lib.cuberille_set_point_scalars(None, C.byref(desc), C.c_void_p(vox.ctypes.data), 0, 0.0) == pkg._abi.ERR_ARGUMENT
    assert lib.cuberille_set_point_scalars(None, None, None, 0, 0.0) == pkg._abi.ERR_ARGUMENT
    p = C.c_void_p(7)
    assert lib.cuberille_point_scalars_device(None, C.byref(p)) == pkg._abi.ERR_ARGUMENT and p.value == 7
    assert lib.cuberille_point_scalars_download(None, None, 0) == pkg._abi.ERR_ARGUMENT


def test_reference_against_the_independent_witness(oracle):
    """4x the largest difference tests/golden/make_point_scalars_tolerance.py measured on its CPU between the oracle primitive
    and the witness (the margin of independent_tolerances.json, for the same reason: another CPU's libm and scipy build round
    a little differently)."""
    table = json.load(open(TOLERANCE))
    bound = table["factor"] * table["relative_to_max_abs"]
    assert table["factor"] == 4.0 and bound > 0.0
    seen = 0
    for name, b, geo, points in witness_cases(oracle):
        diff, n = witness_difference(oracle, b, geo, points)
        print("%-32s %4d points a voxel inside, relative difference %.3e (bound %.3e)" % (name, n, diff, bound))
        assert diff <= bound, (name, diff, bound)
        assert n == table["cases"][name]["points"], (name, n)
        seen += n
    assert seen >= 300


def test_inside_test_of_the_reference():
    """The faces: lower closed, upper open, a NaN outside; no point fragile under a unit matrix."""
    b = np.zeros((5, 7, 9), np.float32)
    pts = np.array([[1.5, 2.5, 0.5], [10.5, 2.5, 0.5], [10.499999, 9.49999, 5.49999], [1.4999999, 3, 1], [np.nan, 3, 1], [2, 3, 5.5]], np.float32)
    inside, fragile = point_scalars_ref.inside_and_fragile(b, pts, **CASE1_GEO)
    assert inside.tolist() == [True, False, True, False, False, False] and not fragile.any()
    inside, fragile = point_scalars_ref.inside_and_fragile(b, pts, spacing=(1.0, 1.0, 2.0), origin=(2.0, 3.0, 1.0))
    assert fragile[0] and fragile[1] and not fragile[5]        # (on a face in x; two voxels from every face)


def _table(sanitize):
    target = "build/point_scalars_table" + ("_san" if sanitize else "")
    subprocess.check_call(["make", "-s", "-C", CSRC, target])                  # (make knows whether it is stale)
    run = subprocess.run([os.path.join(CSRC, target)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "point_scalars_table ok" in run.stdout, run.stdout + run.stderr


def test_point_scalars_table():
    _table(False)


def test_point_scalars_table_under_sanitizers():
    _table(True)
