"""The reference's own filter, compiled unchanged (oracle/Makefile, target `ref`; oracle/ref_filter_main.cxx), as a checker:
writes a case file, runs oracle/_ref/ref_filter*, returns points and cells.  Plus the case list that
tests/test_reference_filter.py, tests/test_gpu_reference_filter.py and tests/golden/make_reference_filter_digests.py share.

A case is a JSON-able dict, so that tests/golden/reference_filter_digests.json can record it next to the digest of what the
REFERENCE binary produced for it:
    name, variant (0: ref_filter, 1: ref_filter_advanced, 2: ref_filter_linesearch), interp, volume, geometry, first,
    iso, triangles, project, threshold, step, relax, max_steps, pad
`volume` says how the voxels are made (make_volume), `geometry` overrides spacing / origin / direction / start of an image
made without one, `first` is None or the {volume, geometry} of the input of the filter object's first Update().
"""
import hashlib
import json
import math
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
BINARIES = ("ref_filter", "ref_filter_advanced", "ref_filter_linesearch")
DIGESTS = os.path.join(GOLDEN, "reference_filter_digests.json")

PIXEL_NAMES = {np.dtype(np.uint8): "u8", np.dtype(np.int8): "i8", np.dtype(np.uint16): "u16", np.dtype(np.int16): "i16",
               np.dtype(np.uint32): "u32", np.dtype(np.int32): "i32", np.dtype(np.float32): "f32", np.dtype(np.float64): "f64",
               np.dtype(np.int64): "i64", np.dtype(np.uint64): "u64"}
DTYPES = ["uint8", "int8", "uint16", "int16", "uint32", "int32", "float32", "float64", "int64", "uint64"]
UNIT = dict(spacing=[1.0, 1.0, 1.0], origin=[0.0, 0.0, 0.0], direction=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], start=[0, 0, 0])


def binary(variant=0):
    return os.path.join(REF_DIR, BINARIES[variant])


def available(variant=0):
    return os.path.exists(binary(variant))


def point_bytes(points):
    """As tests/conftest.py: float32 bits with every NaN replaced by 0x7fc00000."""
    bits = np.ascontiguousarray(points).astype("<f4").view("<u4").copy()
    bits[np.isnan(points)] = 0x7fc00000
    return bits.tobytes()


def digest(points, cells):
    return dict(points=int(points.shape[0]), cells=int(cells.shape[0]),
                points_sha256=hashlib.sha256(point_bytes(points)).hexdigest(),
                cells_sha256=hashlib.sha256(np.ascontiguousarray(cells).astype("<u8").tobytes()).hexdigest())


# ---- volumes ---------------------------------------------------------------------------------------------------------

def _read_mha(name):
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    return graft.load_package().read_mha(os.path.join(GOLDEN, "data", name))


def _field(shape, seed):
    """A smooth float64 field with a closed surface at 0 well inside `shape` ([z, y, x]) plus a seeded ripple."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    c = [(n - 1) / 2 + o for n, o in zip((nx, ny, nz), rng.uniform(-0.4, 0.4, 3))]
    r = 0.33 * min(nx, ny, nz)
    a = rng.uniform(0.8, 1.7, 3)
    return r - np.sqrt((x - c[0]) ** 2 + 0.8 * (y - c[1]) ** 2 + (z - c[2]) ** 2) + 0.15 * np.sin(a[0] * x) * np.cos(a[1] * y + a[2] * z)


def make_volume(spec):
    """(voxels [z, y, x], geometry dict or None)."""
    kind = spec["kind"]
    if kind == "mha":
        v = _read_mha(spec["input"])
        geo = dict(spacing=list(v.spacing), origin=list(v.origin), direction=[float(d) for d in np.asarray(v.direction).reshape(9)],
                   start=[0, 0, 0]) if spec.get("own_geometry", True) else None
        return v.voxels, geo
    dt = np.dtype(spec["dtype"])
    shape = tuple(spec["shape"])
    rng = np.random.default_rng(spec.get("seed", 0))
    if kind == "random":
        # dense noise: `base` + integers of [0, span), for float types with a fraction added
        vox = rng.integers(0, spec["span"], size=shape, dtype=np.int64)
        if dt.kind == "f":
            vox = (vox.astype(np.float64) + rng.random(shape) + spec.get("base", 0)).astype(dt)
        elif dt == np.dtype(np.uint64):
            vox = vox.astype(np.uint64) + np.uint64(spec.get("base", 0))
        else:
            vox = (vox + spec.get("base", 0)).astype(dt)
    elif kind == "field":
        # the smooth field scaled into the type: value = base + scale * f
        f = _field(shape, spec.get("seed", 0)) * spec.get("scale", 1.0)
        if dt.kind == "f":
            vox = (f + spec.get("base", 0)).astype(dt)
        elif dt == np.dtype(np.uint64):
            vox = np.rint(f - f.min()).astype(np.uint64) + np.uint64(spec.get("base", 0))
        else:
            vox = (np.rint(f).astype(np.int64) + spec.get("base", 0)).astype(dt)
    elif kind == "boxes":
        # `boxes`: [z0, z1, y0, y1, x0, x1, value] on a background (quirks Q1, Q2, Q4)
        vox = np.full(shape, spec.get("background", 0), dtype=dt)
        for z0, z1, y0, y1, x0, x1, value in spec["boxes"]:
            vox[z0:z1, y0:y1, x0:x1] = value
    else:
        raise ValueError(kind)
    for z, y, x, value in spec.get("poke", []):          # single voxels: "nan", "inf", "-inf", "-0.0" or a number
        vox[z, y, x] = float(value)
    return np.ascontiguousarray(vox), None


def case_inputs(case):
    """(voxels, geometry, first) with first = None or (voxels, geometry)."""
    vox, geo = make_volume(case["volume"])
    geo = dict(UNIT, **(case.get("geometry") or geo or {}))
    first = None
    if case.get("first"):
        fvox, fgeo = make_volume(case["first"]["volume"])
        first = (fvox, dict(UNIT, **(case["first"].get("geometry") or fgeo or {})))
    return vox, geo, first


def pixel_max(dt):
    dt = np.dtype(dt)
    return float(np.finfo(dt).max) if dt.kind == "f" else float(np.iinfo(dt).max)


def effective(case, vox):
    """What the filter OBJECT's setters make of the numbers a caller hands them, for the entry points that take them per run
    and have no setters (oracle.run, the library's C ABI): the threshold clamped to [0, max pixel] (h:210), the relaxation to
    [0, 1] (h:223), a non-negative step to [0, 100000] (h:216).  A negative step is the constructor's -1 and goes through AS IT
    IS: replacing it by the default -- of the first input, for good (txx:82-85) -- is the entry point's own job."""
    thr = min(max(case["threshold"], 0.0), pixel_max(vox.dtype))
    relax = min(max(case["relax"], 0.0), 1.0)
    step = case["step"] if case["step"] < 0.0 else min(case["step"], 100000.0)
    return thr, step, relax


def iso_of(case):
    """The case's iso value as a number (an infinite one is written as a string, so that the recorded cases stay plain JSON)."""
    return float(case["iso"]) if isinstance(case["iso"], str) else case["iso"]


# ---- the binary ------------------------------------------------------------------------------------------------------

def _geometry_lines(prefix, vox, geo):
    nz, ny, nx = vox.shape
    return ["%sdims %d %d %d" % (prefix, nx, ny, nz),
            "%sspacing %s" % (prefix, " ".join(float(v).hex() for v in geo["spacing"])),
            "%sorigin %s" % (prefix, " ".join(float(v).hex() for v in geo["origin"])),
            "%sdirection %s" % (prefix, " ".join(float(v).hex() for v in np.asarray(geo["direction"], dtype=np.float64).reshape(9))),
            "%sstart %d %d %d" % ((prefix,) + tuple(int(v) for v in geo["start"]))]


def iso_lines(dtype, iso):
    if np.dtype(dtype) in (np.dtype(np.int64), np.dtype(np.uint64)):
        # as oracle.run and the library: the C cast of the value, truncated toward zero
        return ["iso_int %d" % (int(iso) if isinstance(iso, (int, np.integer)) else math.trunc(float(iso)))]
    return ["iso %s" % float(iso).hex()]


def run_reference(case, workdir=None):
    """Run the case through the reference binary of its variant; (points float32 [n, 3], cells uint64 [m, 3 | 4])."""
    vox, geo, first = case_inputs(case)
    lines = ["pixel %s" % PIXEL_NAMES[vox.dtype], "interp %s" % case.get("interp", "linear")]
    lines += _geometry_lines("", vox, geo)
    if first:
        assert first[0].dtype == vox.dtype
        lines += ["first 1"] + _geometry_lines("first_", first[0], first[1])
    lines += iso_lines(vox.dtype, iso_of(case))
    lines += ["triangles %d" % int(case["triangles"]), "project %d" % int(case["project"]),
              "threshold %s" % float(case["threshold"]).hex(), "step %s" % float(case["step"]).hex(),
              "relax %s" % float(case["relax"]).hex(), "max_steps %d" % int(case["max_steps"]), "pad %d" % int(bool(case.get("pad")))]
    with tempfile.TemporaryDirectory(dir=workdir) as tmp:
        cpath, opath = os.path.join(tmp, "case"), os.path.join(tmp, "mesh")
        with open(cpath, "wb") as f:
            f.write(("\n".join(lines) + "\nend\n").encode("ascii"))
            if first:
                f.write(first[0].astype(first[0].dtype.newbyteorder("<")).tobytes())
            f.write(vox.astype(vox.dtype.newbyteorder("<")).tobytes())
        p = subprocess.run([binary(case.get("variant", 0)), cpath, opath], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        if p.returncode != 0:
            raise RuntimeError("%s: exit %d: %s" % (case["name"], p.returncode, p.stdout.decode(errors="replace")[-2000:]))
        raw = open(opath, "rb").read()
    n, m, k = (int(v) for v in np.frombuffer(raw, dtype="<u8", count=3))
    points = np.frombuffer(raw, dtype="<f4", count=3 * n, offset=24).reshape(n, 3).copy()
    cells = np.frombuffer(raw, dtype="<u8", count=k * m, offset=24 + 12 * n).reshape(m, k).copy()
    return points, cells


def run_oracle(oracle, case):
    """The same case through the oracle (oracle.run); the padded recipe as np.pad with the start index moved down by one."""
    vox, geo, first = case_inputs(case)
    thr, step, relax = effective(case, vox)
    start = list(geo["start"])
    if case.get("pad"):
        vox = np.pad(vox, 1, mode="constant", constant_values=0)
        start = [s - 1 for s in start]
    kw = dict(triangles=case["triangles"], project=case["project"], threshold=thr, step=step, relax=relax, max_steps=case["max_steps"],
              spacing=tuple(geo["spacing"]), origin=tuple(geo["origin"]), direction=np.asarray(geo["direction"]).reshape(3, 3),
              index_start=tuple(start), variant=case.get("variant", 0))
    if first:
        fg = first[1]
        kw["first"] = (first[0], tuple(fg["spacing"]), tuple(fg["origin"]), np.asarray(fg["direction"]).reshape(3, 3), tuple(fg["start"]))
    m = oracle.run(vox, iso_of(case), **kw)
    return m.points, m.cells


def first_difference(points, cells, rpoints, rcells):
    """None when the two meshes are the same, bit for bit (NaN coordinates compare as NaN); else a line naming the first
    differing cell and vertex with the values on both sides."""
    if points.shape != rpoints.shape or cells.shape != rcells.shape:
        return "counts differ: %s points / %s cells against the reference's %s / %s" % (points.shape, cells.shape, rpoints.shape, rcells.shape)
    out = []
    bad = np.argwhere((cells != rcells).any(axis=1))
    if len(bad):
        i = int(bad[0][0])
        out.append("%d cells differ, first: cell %d is %s, the reference's %s" % (len(bad), i, cells[i].tolist(), rcells[i].tolist()))
    a = np.frombuffer(point_bytes(points), dtype="<u4").reshape(-1, 3)
    b = np.frombuffer(point_bytes(rpoints), dtype="<u4").reshape(-1, 3)
    bad = np.argwhere((a != b).any(axis=1))
    if len(bad):
        i = int(bad[0][0])
        out.append("%d vertices differ, first: vertex %d is %s (%s), the reference's %s (%s)" % (
            len(bad), i, points[i].tolist(), [hex(v) for v in a[i]], rpoints[i].tolist(), [hex(v) for v in b[i]]))
    return "; ".join(out) if out else None


# ---- the cases -------------------------------------------------------------------------------------------------------

def _case(name, volume, iso, triangles=1, project=1, threshold=0.5, step=0.25, relax=0.95, max_steps=50, **more):
    c = dict(name=name, variant=0, interp="linear", volume=volume, geometry=None, first=None, iso=iso, triangles=int(triangles),
             project=int(project), threshold=threshold, step=step, relax=relax, max_steps=int(max_steps), pad=0)
    c.update(more)
    return c


def _params(r):
    return dict(triangles=r["triangles"], project=r["project"], threshold=r["threshold"], step=r["step"], relax=r["relax"], max_steps=r["max_steps"])


def _rows(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def ctest_cases():
    """The 19 rows of the reference's CTest table, each volume with its own geometry."""
    return [_case("ctest/" + r["name"], dict(kind="mha", input=r["input"]), r["iso"], **_params(r)) for r in _rows("ctest_cases.json")]


def mesh_digest_cases():
    """The 44 rows of mesh_digests.json (the oracle's frozen meshes of the Data volumes)."""
    return [(_case("mesh_digests/%02d/%s" % (i, r["input"]), dict(kind="mha", input=r["input"]), r["iso"], **_params(r)), r)
            for i, r in enumerate(_rows("mesh_digests.json"))]


def later_update_cases():
    """The 22 rows of later_update_digests.json: a buffered region with a start index, and quirk Q3 as a real second Update()."""
    out = []
    for i, r in enumerate(_rows("later_update_digests.json")):
        if r["first"]:
            c = _case("later_update/%02d/%s_after_%s" % (i, r["input"], r["first"]), dict(kind="mha", input=r["input"], own_geometry=False),
                      r["iso"], first=dict(volume=dict(kind="mha", input=r["first"]), geometry=None), **_params(r))
        else:
            c = _case("later_update/%02d/%s_start" % (i, r["input"]), dict(kind="mha", input=r["input"], own_geometry=False), r["iso"],
                      geometry=dict(UNIT, spacing=r["spacing"], origin=r["origin"], start=r["index_start"]), **_params(r))
        out.append((c, r))
    return out


def variant_cases():
    """The rows of variant_digests.json of the central-difference gradient: the two compiled-out projection branches."""
    return [(_case("variant/%02d/%s_v%d" % (i, r["input"], r["variant"]), dict(kind="mha", input=r["input"]), r["iso"], variant=r["variant"],
                   **_params(r)), r)
            for i, r in enumerate(_rows("variant_digests.json")) if r["gradient"] == 0]


SHAPES = [[1, 9, 8], [9, 1, 8], [8, 9, 1], [2, 7, 9], [7, 2, 9], [9, 7, 2], [5, 4, 63], [3, 5, 64], [4, 3, 65], [130, 9, 7]]   # [z, y, x]


def pixel_type_cases():
    """All ten pixel types x quads / triangles x projection on / off on seeded dense noise; the shapes -- an axis of length 1 and
    of 2, rows of 63 / 64 / 65, a 7 x 9 x 130 -- go round so that every type meets every kind."""
    out = []
    for t, dt in enumerate(DTYPES):
        for k, (tri, proj) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)]):
            shape = SHAPES[(3 * t + 5 * k) % len(SHAPES)]
            base = -50 if np.dtype(dt).kind in "if" else 0
            out.append(_case("types/%s/tri%d_proj%d_%s" % (dt, tri, proj, "x".join(str(v) for v in shape)),
                             dict(kind="random", dtype=dt, shape=shape, seed=1000 + 10 * t + k, span=100, base=base),
                             base + 50, triangles=tri, project=proj, threshold=2.0, step=0.25, max_steps=12))
    for i, shape in enumerate(SHAPES):             # and every shape once with the flagship type, projected triangles
        out.append(_case("types/shape/%s" % "x".join(str(v) for v in shape), dict(kind="random", dtype="float32", shape=shape, seed=1200 + i, span=100),
                         50.25, threshold=2.0, max_steps=12))
    return out


def cast_cases():
    """Integer iso values with a fractional part, iso at a type's extremes, voxels past 2^24 and 2^53."""
    out = []
    for dt, iso in [("uint8", 127.75), ("int8", -3.5), ("int8", 3.5), ("uint16", 40000.9), ("int16", -1234.25), ("uint32", 70000.5), ("int32", -70000.5),
                    ("int64", -20.5), ("uint64", 20.5)]:
        lo = {"uint8": 120, "int8": -8, "uint16": 39990, "int16": -1240, "uint32": 69990, "int32": -70010, "int64": -30, "uint64": 10}[dt]
        out.append(_case("cast/fraction/%s_%s" % (dt, iso), dict(kind="random", dtype=dt, shape=[6, 7, 8], seed=len(out), span=20, base=lo), iso,
                         threshold=0.75, max_steps=10))
    for dt in ("uint8", "int8", "uint16", "int16", "int32", "uint32"):
        info = np.iinfo(dt)
        out.append(_case("cast/extreme/%s_max" % dt, dict(kind="random", dtype=dt, shape=[5, 6, 7], seed=40 + len(out), span=3, base=int(info.max) - 2),
                         int(info.max), threshold=0.25, max_steps=6))
        out.append(_case("cast/extreme/%s_min" % dt, dict(kind="random", dtype=dt, shape=[5, 6, 7], seed=40 + len(out), span=3, base=int(info.min)),
                         int(info.min), threshold=0.25, max_steps=6))
        out.append(_case("cast/extreme/%s_min_plus_1" % dt, dict(kind="random", dtype=dt, shape=[5, 6, 7], seed=40 + len(out), span=3, base=int(info.min)),
                         int(info.min) + 1, threshold=0.25, max_steps=6))
    for dt in ("int64", "uint64"):
        info = np.iinfo(dt)
        out.append(_case("cast/extreme/%s_max" % dt, dict(kind="random", dtype=dt, shape=[5, 6, 7], seed=60 + len(out), span=3, base=int(info.max) - 2),
                         int(info.max), threshold=0.25, max_steps=6))
        out.append(_case("cast/extreme/%s_min" % dt, dict(kind="random", dtype=dt, shape=[5, 6, 7], seed=60 + len(out), span=3, base=int(info.min)),
                         int(info.min), threshold=0.25, max_steps=6))
        out.append(_case("cast/extreme/%s_min_plus_1" % dt, dict(kind="random", dtype=dt, shape=[5, 6, 7], seed=60 + len(out), span=3, base=int(info.min)),
                         int(info.min) + 1, threshold=0.25, max_steps=6))
    for dt in ("float32", "float64"):
        top = float(np.finfo(dt).max)
        out.append(_case("cast/extreme/%s_max" % dt, dict(kind="boxes", dtype=dt, shape=[5, 6, 7], boxes=[[1, 3, 2, 4, 2, 5, top], [3, 4, 1, 2, 1, 2, top / 2]]),
                         top, project=0))
        out.append(_case("cast/extreme/%s_lowest" % dt, dict(kind="boxes", dtype=dt, shape=[5, 6, 7], background=-top, boxes=[[1, 3, 2, 4, 2, 5, 0.0]]),
                         -top, project=0))
        out.append(_case("cast/extreme/%s_above_lowest" % dt, dict(kind="boxes", dtype=dt, shape=[5, 6, 7], background=-top, boxes=[[1, 3, 2, 4, 2, 5, -top / 2]]),
                         -top / 2, project=0))
    for dt, base in [("int64", (1 << 53) + 1), ("uint64", (1 << 63) + (1 << 53) + 1), ("int64", -(1 << 60) + 1), ("uint64", (1 << 24) + 1),
                     ("int64", (1 << 24) + 1), ("uint32", (1 << 24) + 1), ("int32", -(1 << 30) + 1), ("float64", float((1 << 24) + 1))]:
        for proj in (0, 1):
            # noise of 0 .. 39 above `base`: odd values that float (24 bits) and, past 2^53, double round
            out.append(_case("cast/wide/%s_%s_proj%d" % (dt, base, proj), dict(kind="random", dtype=dt, shape=[6, 7, 9], seed=70 + len(out), span=40, base=base),
                             base + 20, project=proj, threshold=1.5, max_steps=10))
    return out


def _rot(deg_z, deg_x):
    a, b = math.radians(deg_z), math.radians(deg_x)
    rz = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(b), -math.sin(b)], [0.0, math.sin(b), math.cos(b)]])
    return [float(v) for v in (rz @ rx).reshape(9)]


GEOMETRIES = {
    "anisotropic": dict(UNIT, spacing=[0.7, 1.3, 0.9]),
    "origin_off_grid": dict(UNIT, origin=[3.3, -2.1, 0.77]),
    "rotated": dict(UNIT, spacing=[0.7, 1.3, 0.9], origin=[3.3, -2.1, 0.77], direction=_rot(21.0, -13.0)),
    "sheared": dict(UNIT, spacing=[1.1, 0.8, 1.25], direction=[1.0, 0.2, 0.0, 0.0, 1.0, 0.3, 0.1, 0.0, 1.0]),
    "start_index": dict(UNIT, spacing=[0.5, 2.0, 1.0], origin=[4.5, -6.0, 3.0], start=[1000, -37, 512]),
    "all": dict(spacing=[0.7, 1.3, 0.9], origin=[3.3, -2.1, 0.77], direction=_rot(21.0, -13.0), start=[1000, -37, 512]),
}


def geometry_cases():
    out = []
    for variant in (0, 1, 2):
        for i, (name, geo) in enumerate(sorted(GEOMETRIES.items())):
            for dt, scale, iso, thr in [("float32", 1.0, 0.0, 0.01), ("uint8", 30.0, 128, 0.5)]:
                out.append(_case("geometry/%s/%s_v%d" % (name, dt, variant), dict(kind="field", dtype=dt, shape=[11, 12, 13], seed=300 + i, scale=scale,
                                                                                base=0 if dt == "float32" else 128),
                                 iso, threshold=thr, step=0.2, relax=0.9, max_steps=14, variant=variant, geometry=geo))
    return out


def quirk_cases():
    out = []
    one = lambda z, v=255: [z, z + 1, 2, 5, 2, 6, v]
    # Q1: empty slices between occupied ones, the first and the last slice included
    for name, zs in [("gap1", [2, 4]), ("gap2_first_last", [0, 3, 9]), ("first_second_last", [0, 1, 9]), ("every_other", [0, 2, 4, 6, 8])]:
        for tri, proj in [(0, 0), (1, 1)]:
            out.append(_case("quirk/Q1/%s_tri%d_proj%d" % (name, tri, proj), dict(kind="boxes", dtype="uint8", shape=[10, 7, 8], boxes=[one(z) for z in zs]),
                             128, triangles=tri, project=proj))
    # Q2: an object on every face of the border, and one in a corner
    faces = {"x0": [3, 5, 3, 5, 0, 2, 200], "x1": [3, 5, 3, 5, 7, 9, 200], "y0": [3, 5, 0, 2, 3, 5, 200], "y1": [3, 5, 6, 8, 3, 5, 200],
             "z0": [0, 2, 3, 5, 3, 5, 200], "z1": [5, 7, 3, 5, 3, 5, 200], "corner": [0, 2, 0, 2, 0, 2, 200], "all": None}
    for name, box in sorted(faces.items()):
        boxes = [b for b in faces.values() if b] if box is None else [box]
        for variant in ((0, 1, 2) if name in ("all", "corner") else (0,)):
            out.append(_case("quirk/Q2/%s_v%d" % (name, variant), dict(kind="boxes", dtype="uint8", shape=[7, 8, 9], boxes=boxes), 100, variant=variant,
                             max_steps=14))
    out.append(_case("quirk/Q2/full_volume", dict(kind="boxes", dtype="uint8", shape=[4, 4, 4], background=255, boxes=[]), 128))
    # Q4: a plateau -- the gradient is zero where the walk starts, Normalize() divides by zero, the vertex goes NaN
    for dt in ("uint8", "float32", "float64"):
        for variant in (0, 1, 2):
            # (the line search then has no sample that beats its start, see points_defined: quads, so that no split hangs on it)
            out.append(_case("quirk/Q4/plateau_%s_v%d" % (dt, variant), dict(kind="boxes", dtype=dt, shape=[9, 9, 9], boxes=[[2, 7, 2, 7, 2, 7, 100]]), 50,
                             threshold=0.5, variant=variant, max_steps=14, triangles=int(variant != 2), points_undefined=int(variant == 2)))
    # voxels that are not numbers, infinite, or a negative zero
    for dt in ("float32", "float64"):
        for name, pokes, iso in [("nan", [[4, 4, 4, "nan"], [2, 3, 3, "nan"]], 0.0), ("inf", [[4, 4, 4, "inf"], [1, 2, 6, "-inf"]], 0.0),
                                 ("negzero", [[4, 4, 5, "-0.0"], [4, 5, 4, "-0.0"], [3, 3, 3, "-0.0"]], 0.0),
                                 ("negzero_iso", [[4, 4, 5, "-0.0"], [6, 6, 6, "0.0"]], -0.0), ("inf_iso", [[4, 4, 4, "inf"], [4, 4, 5, "inf"]], "inf")]:
            for proj in (0, 1):
                out.append(_case("quirk/special/%s_%s_proj%d" % (name, dt, proj), dict(kind="field", dtype=dt, shape=[9, 9, 9], seed=500, poke=pokes),
                                 iso, project=proj, threshold=0.01, max_steps=10))
    return out


def walk_cases():
    out = []
    vol = dict(kind="field", dtype="float32", shape=[11, 12, 13], seed=600)
    geo = GEOMETRIES["anisotropic"]
    for variant in (0, 1, 2):
        for max_steps in (0, 1, 3, 4, 5, 9):
            out.append(_case("walk/max_steps_%d_v%d" % (max_steps, variant), vol, 0.0, threshold=0.001, step=0.3, relax=0.9, max_steps=max_steps,
                             variant=variant, geometry=geo, triangles=int(points_defined(dict(variant=variant, project=1, max_steps=max_steps)))))
        for relax in (1.0, 0.5):
            out.append(_case("walk/relax_%s_v%d" % (relax, variant), vol, 0.0, threshold=0.001, step=0.3, relax=relax, max_steps=14, variant=variant,
                             geometry=geo))
        for name, thr in [("none_meets", 0.0), ("all_meet", 1.0e30), ("negative_clamps_to_0", -1.0)]:
            out.append(_case("walk/threshold_%s_v%d" % (name, variant), vol, 0.0, threshold=thr, step=0.3, relax=0.9, max_steps=14, variant=variant,
                             geometry=geo))
        # the clamps of the other setters, and the threshold's upper clamp at the pixel type's maximum
        out.append(_case("walk/relax_clamped_v%d" % variant, vol, 0.0, threshold=0.001, step=0.3, relax=1.5, max_steps=8, variant=variant))
        out.append(_case("walk/threshold_clamped_u8_v%d" % variant, dict(kind="field", dtype="uint8", shape=[9, 9, 9], seed=601, scale=60.0, base=100), 100,
                         threshold=1000.0, step=0.3, max_steps=8, variant=variant))
        # step -1: the default is taken from the FIRST input's spacing and sticks for the second Update() (txx:82-85)
        out.append(_case("walk/step_default_v%d" % variant, vol, 0.0, threshold=0.001, step=-1.0, relax=0.9, max_steps=14, variant=variant, geometry=geo))
        out.append(_case("walk/step_default_sticks_v%d" % variant, vol, 0.0, threshold=0.001, step=-1.0, relax=0.9, max_steps=14, variant=variant,
                         geometry=geo, first=dict(volume=dict(kind="field", dtype="float32", shape=[9, 10, 8], seed=602),
                                                  geometry=dict(UNIT, spacing=[2.0, 0.5, 1.0], origin=[0.5, 0.25, -1.0]))))
    return out


def border_cases():
    """The class comment's recipe: ConstantPadImageFilter by one pixel, then the filter."""
    out = []
    for dt, iso in [("uint8", 128), ("int16", 0), ("float32", 50.5)]:
        for name, geo in [("unit", None), ("all", GEOMETRIES["all"])]:
            for tri, proj in [(0, 0), (1, 1)]:
                out.append(_case("border/%s_%s_tri%d_proj%d" % (dt, name, tri, proj),
                                 dict(kind="random", dtype=dt, shape=[5, 6, 7], seed=700 + len(out), span=200, base=-100 if dt == "int16" else 0), iso,
                                 triangles=tri, project=proj, threshold=1.0, max_steps=10, geometry=geo, pad=1))
    return out


def bspline_cases():
    """The reference driver's B-spline configuration (BSplineInterpolateImageFunction<Image, float, float> and
    <Image, double, double>, order 3) on the CTest volumes that project and on one tilted geometry."""
    out = []
    for r in _rows("ctest_cases.json"):
        if r["project"] and r["input"] not in [c["volume"]["input"] for c in out]:
            out.append(_case("bspline/" + r["name"], dict(kind="mha", input=r["input"]), r["iso"], interp="bspline_f", **_params(r)))
    for interp in ("bspline_f", "bspline_d"):
        out.append(_case("bspline/tilted_" + interp, dict(kind="field", dtype="float32", shape=[11, 12, 13], seed=800), 0.0, threshold=0.001,
                         step=0.2, relax=0.9, max_steps=14, interp=interp, geometry=GEOMETRIES["all"]))
    return out


def split_quads(points, quads):
    """txx:295-307 on arrays: each quad as two triangles, cut along the diagonal 1-3 unless 0-2 is strictly shorter; squared
    lengths summed in double over x, y, z in that order (I10)."""
    p = points.astype(np.float64)
    d = lambda a, b: ((p[quads[:, b], 0] - p[quads[:, a], 0]) ** 2 + (p[quads[:, b], 1] - p[quads[:, a], 1]) ** 2) + (p[quads[:, b], 2] - p[quads[:, a], 2]) ** 2
    first = d(0, 2) >= d(1, 3)
    tri = np.where(first[:, None], quads[:, [0, 1, 3, 1, 2, 3]], quads[:, [0, 1, 2, 0, 2, 3]])
    return tri.reshape(-1, 3)


def synthetic_cases():
    return pixel_type_cases() + cast_cases() + geometry_cases() + quirk_cases() + walk_cases() + border_cases()


def points_defined(case):
    """The line search (txx:398-437) returns `bestVertex`, which it never initialises: with fewer than four steps there is no
    sample at all, and where the normal is not a number (quirk Q4) no sample's metric compares below the start value: the
    reference's coordinates are then whatever its stack held.  Those cases compare quads and counts only."""
    if case.get("points_undefined"):
        return False
    return not (case.get("variant", 0) == 2 and case["project"] and case["max_steps"] // 2 <= 1)


def undefined_vertices(case):
    """Line search only: the vertices at which the REFERENCE's result is not defined.  The line search returns `bestVertex`,
    which it never initialises (txx:404,437): where no sample's metric is below its start value the compiled reference returns
    whatever its stack held, usually an earlier vertex's result.  That happens where the normal is not a number -- a zero
    gradient, Normalize() divides by zero (Q4) -- and the mask is taken from the reference itself, not from the side under
    test: its DEFAULT branch, run from the same start with threshold 0 and no steps to spare, adds `normal * step` to the
    vertex, so exactly those vertices come out NaN.  Oracle and HIP leave such a vertex where it started."""
    if case.get("variant", 0) != 2 or not case["project"]:
        return None
    points, _ = run_reference(dict(case, variant=0, threshold=0.0, max_steps=0, triangles=0))
    return np.isnan(points).any(axis=1)


def masked(mask, points, cells):
    """(points, cells) with the coordinates of the masked vertices and, for triangles, the two rows of every quad that touches
    one (its split hangs on the undefined coordinates; the four ids a quad joins are the same however it is split) zeroed."""
    if mask is None or not np.asarray(mask).any():
        return points, cells
    mask = np.asarray(mask, dtype=bool)
    points = np.where(mask[:, None], np.float32(0), points)
    if cells.shape[1] == 3:
        touched = np.repeat(mask[cells].any(axis=1).reshape(-1, 2).any(axis=1), 2)
        cells = np.where(touched[:, None], np.uint64(0), cells)
    return points, cells


def difference_outside(mask, points, cells, rpoints, rcells):
    """first_difference, leaving out what `masked` leaves out; quads are compared in full."""
    if points.shape != rpoints.shape or cells.shape != rcells.shape or mask is None or not mask.any():
        return first_difference(points, cells, rpoints, rcells)
    if cells.shape[1] == 3:
        for q in np.flatnonzero(mask[cells].any(axis=1).reshape(-1, 2).any(axis=1)):
            if set(cells[2 * q:2 * q + 2].ravel().tolist()) != set(rcells[2 * q:2 * q + 2].ravel().tolist()):
                return "quad %d joins other vertices than the reference's" % q
    return first_difference(*(masked(mask, points, cells) + masked(mask, rpoints, rcells)))


# the only cases in which the line search meets a zero gradient (undefined_vertices): pinned by name
UNDEFINED_VARIANT_ROWS = ["variant/10/blob3.mha_v2"]


def recorded_cases():
    """Every case whose reference result tests/golden/reference_filter_digests.json records: the synthetic ones, and the CTest
    table (small).  The digest rows of the Data volumes are already recorded, by the oracle, in the files they come from; the
    direct tests hold those files to the reference binary."""
    return ctest_cases() + synthetic_cases()
