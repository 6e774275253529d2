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
ENVELOPE_FINITE = os.path.join(GOLDEN, "envelope_finite_vertices.json")      # {family: {rest of the case name: [finite vertices, vertices]}}, from the binary
BSPLINE_DIGESTS = os.path.join(GOLDEN, "envelope_bspline_digests.json")      # rows as DIGESTS', of bspline_envelope_cases()

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
        if spec.get("whole"):
            # the type's whole range, uint64's included (an int64 draw cannot reach it)
            vox = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, size=shape, dtype=dt, endpoint=True)
            return np.ascontiguousarray(vox), None
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
            with np.errstate(over="ignore"):                 # (a scale past the type's largest number: infinite voxels, meant)
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
    if spec.get("band"):
        # the copy itk::BinaryThresholdImageFilter would hand the filter: [lower, upper, inside, outside] in the pixel type
        lower, upper, inside, outside = (np.asarray(v, dtype=dt) for v in spec["band"])
        vox = np.where((lower <= vox) & (vox <= upper), inside, outside).astype(dt)
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


def run_oracle(oracle, case, **more):
    """The same case through the oracle (oracle.run); the padded recipe as np.pad with the start index moved down by one.
    more: further arguments of oracle.run (gradient=1: the recursive-Gaussian gradient, which the reference compiles out)."""
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
    kw.update(more)
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


# ---- the envelope: the same walk at the edges of the number range -----------------------------------------------------
# [7, 8, 9] fields and [6, 7, 9] noise: the smallest at which every vertex still has a full gradient ring and the walk takes
# several passes.  Every family runs the default branch and the advanced one; the line search (variant 2) only where
# max |voxel - iso| < LINESEARCH_BOUND over the whole volume: `bestMetric` starts at 10000 (txx:405), every interpolated value
# is a convex combination of voxels, so under that rule the first sample beats it and `bestVertex` (txx:404,437) is assigned.
# Above it the reference returns stack contents (seen at a float32 field scaled by 1e6 and at full-range int16 noise), which
# is why the large magnitudes and the spans carry variants 0 and 1 only and the line search has scales and a span of its own.

LINESEARCH_BOUND = 10000.0
ENV_ROTATED = dict(UNIT, spacing=[0.7, 1.3, 0.9], direction=_rot(21.0, -13.0))
ENV_DIAGONAL = dict(UNIT, spacing=[0.25, 0.5, 3.0])                     # identity direction: the kernels' GEOM 1 form
ENV_F32_GEOMETRIES = [("unit", None), ("rotated", ENV_ROTATED), ("diagonal", ENV_DIAGONAL)]
ENV_F64_GEOMETRIES = [("rotated", ENV_ROTATED), ("unit", None)]
ENV_F32_SCALES = [1e-42, 1e-30, 1e-20, 1e15, 1e30, 1e37, 1e38, 1.5e38, 2e38, 3e38]
ENV_F64_SCALES = [1e-310, 1e-44, 1e-38, 1e-30, 1e30, 1e38, 2e38, 4e38, 1e200, 1e300]
ENV_LINESEARCH_SCALES = [1e-42, 1e-30, 1e-20, 1e3]
# 1e38 leaves 96 % of the B-spline walk's vertices finite and 2e38 only 4 %: the scale between them is the mixed one
ENV_BSPLINE_SCALES = [1e-30, 1e30, 1e38, 1.4e38, 2e38]
ENV_LIMIT = 1 << 30
ENV_STARTS = [[ENV_LIMIT, ENV_LIMIT, ENV_LIMIT], [-ENV_LIMIT, -ENV_LIMIT, -ENV_LIMIT], [ENV_LIMIT - 9, -ENV_LIMIT, 12345678],
              [(1 << 24) + 1, -(1 << 24) - 1, 1 << 29]]
# the mixed-share condition (tests/test_reference_filter.py): name prefix of each magnitude family that must have a case whose
# vertices are neither nearly all finite nor nearly all NaN
ENV_MIXED_FAMILIES = ["envelope/magnitude/float32_unit_", "envelope/magnitude/float32_rotated_", "envelope/magnitude/float32_diagonal_",
                      "envelope/magnitude/float64_rotated_", "envelope_bspline/magnitude_float32_"]


def note_finite(record, case, points):
    """record[family][rest of the name] = [finite vertices, vertices] for a case of one of ENV_MIXED_FAMILIES (ENVELOPE_FINITE)."""
    for family in ENV_MIXED_FAMILIES:
        if case["name"].startswith(family):
            record.setdefault(family, {})[case["name"][len(family):]] = [int(np.isfinite(points).all(axis=1).sum()), len(points)]


def _env_field(dtype, scale=1.0):
    return dict(kind="field", dtype=dtype, shape=[7, 8, 9], seed=900 if dtype == "float32" else 901, scale=scale)


def _env(out, name, volume, iso, variants=(0, 1, 2), threshold=0.01, step=0.2, **more):
    more.setdefault("relax", 0.9)
    for v in variants:
        out.append(_case("envelope/%s_v%d" % (name, v), volume, iso, variant=v, threshold=threshold, step=step, max_steps=8, **more))


def envelope_magnitude_cases():
    out = []
    for dt, scales, geos in (("float32", ENV_F32_SCALES, ENV_F32_GEOMETRIES), ("float64", ENV_F64_SCALES, ENV_F64_GEOMETRIES)):
        for gname, geo in geos:
            for s in scales:
                _env(out, "magnitude/%s_%s_%g" % (dt, gname, s), _env_field(dt, s), 0.0, variants=(0, 1), threshold=0.0, step=0.25, geometry=geo)
            for s in ENV_LINESEARCH_SCALES:
                _env(out, "magnitude/%s_%s_%g" % (dt, gname, s), _env_field(dt, s), 0.0, variants=(2,), threshold=0.0, step=0.25, geometry=geo)
    return out


def envelope_span_cases():
    """Integer noise over the type's whole range, iso at its middle; the line search on a span of 9999 at int32's lowest."""
    out = []
    for dt in ("int16", "uint16", "int32", "uint32", "int64", "uint64"):
        info = np.iinfo(dt)
        for proj in (0, 1):
            _env(out, "span/%s_proj%d" % (dt, proj), dict(kind="random", dtype=dt, shape=[6, 7, 9], seed=77, whole=1),
                 (int(info.max) + int(info.min) + 1) // 2, variants=(0, 1), step=0.25, project=proj)
    _env(out, "span/int32_lowest_9999", dict(kind="random", dtype="int32", shape=[6, 7, 9], seed=78, span=9999, base=-(1 << 31)),
         -(1 << 31) + 4999, variants=(2,), step=0.25)
    return out


def envelope_geometry_cases():
    """Spacing, origin and start index at their extremes, a step far below and far above a voxel, a direction matrix near
    singular, no relaxation."""
    out = []
    vol = _env_field("float32")
    for s in (1e-60, 1e-30, 1e-12, 1e-4, 1e4, 1e12, 1e30, 1e60):
        # At 1e-60 and 1e60 the float gradient overflows or vanishes, Normalize() (txx:409) makes every normal NaN, no sample's
        # metric compares below bestMetric (txx:430) and the line search returns the unassigned bestVertex (txx:404,437) at
        # EVERY vertex: undefined in the reference, taken out (4 cases).  The other two branches are defined there (all NaN).
        variants = (0, 1) if s in (1e-60, 1e60) else (0, 1, 2)
        _env(out, "spacing/isotropic_%g" % s, vol, 0.0, variants=variants, step=0.25 * s, geometry=dict(UNIT, spacing=[s, s, s]))
        _env(out, "spacing/rotated_%g" % s, vol, 0.0, variants=variants, step=0.25 * min(s, 1.0 / s),
             geometry=dict(ENV_ROTATED, spacing=[s, 1.0, 1.0 / s]))
    for o in (1e5, 1e7, 1e9, 1e15, 1e30):
        _env(out, "origin/aligned_%g" % o, vol, 0.0, geometry=dict(UNIT, origin=[o, -o, o / 3], spacing=[0.7, 1.3, 0.9]))
        _env(out, "origin/rotated_%g" % o, vol, 0.0, geometry=dict(ENV_ROTATED, origin=[o, -o, o / 3]))
    for st in ENV_STARTS:
        _env(out, "start/unit_%d_%d_%d" % tuple(st), vol, 0.0, geometry=dict(UNIT, start=st))
        _env(out, "start/all_%d_%d_%d" % tuple(st), vol, 0.0, geometry=dict(GEOMETRIES["all"], start=st))
    for step in (1e-300, 1e-30, 1e-9, 50.0, 1e5):
        _env(out, "step/%g" % step, vol, 0.0, step=step, geometry=GEOMETRIES["anisotropic"])
    for e in (1e-3, 1e-8, 1e-14):
        _env(out, "shear/%g" % e, vol, 0.0, geometry=dict(UNIT, direction=[1.0, 1.0 - e, 0.0, 0.0, e, 0.0, 0.0, 0.0, 1.0]))
    _env(out, "relax_0", vol, 0.0, relax=0.0)
    return out


def envelope_pad_cases():
    """One case per family again behind the class comment's recipe (ConstantPadImageFilter by one pixel): the twins that
    cuberille_set_border is held to.  (The padded image starts one index lower, so the start-index twin is the one that stays
    inside the legal range.)"""
    names = ["magnitude/float32_rotated_2e+38", "magnitude/float64_rotated_2e+38", "span/int64_proj1", "spacing/rotated_1e-12",
             "origin/rotated_1e+09", "start/all_%d_%d_%d" % tuple(ENV_STARTS[3]), "step/50", "shear/1e-14", "relax_0"]
    byname = {c["name"]: c for c in envelope_magnitude_cases() + envelope_span_cases() + envelope_geometry_cases()}
    return [dict(byname["envelope/%s_v0" % n], name="envelope/pad/%s_v0" % n, pad=1) for n in names]


ENV_BAND_TWINS = ["magnitude/float32_unit_1e+30", "magnitude/float32_rotated_1e-42", "magnitude/float32_diagonal_1e+38",
                  "magnitude/float64_rotated_1e+300", "spacing/isotropic_1e-30", "spacing/rotated_1e-12", "origin/aligned_1e+07",
                  "origin/rotated_1e+07", "start/all_%d_%d_%d" % tuple(ENV_STARTS[2]), "step/1e-09", "shear/1e-14"]


def envelope_band_cases():
    """One case per geometry again on the {0, 1} copy of its field -- 1 where iso <= voxel <= the type's largest number, so an
    infinite voxel is outside --, iso 1: the twins that cuberille_set_band on the field itself is held to.  (Where float32
    vertices are coarser than a voxel -- the start index, the squeezed spacing, the shear -- the walk reads a clamped, flat corner
    of the {0, 1} image and every vertex goes NaN (quirk Q4); the others stay finite, origin/aligned_1e+07 in part.)"""
    byname = {c["name"]: c for c in envelope_magnitude_cases() + envelope_geometry_cases()}
    out = []
    for n in ENV_BAND_TWINS:
        c = byname["envelope/%s_v0" % n]
        band = [c["iso"], pixel_max(c["volume"]["dtype"]), 1, 0]
        out.append(dict(c, name="envelope/band/%s_v0" % n, volume=dict(c["volume"], band=band), iso=1, threshold=0.01))
    return out


ENVELOPE_GROUPS = ["envelope_magnitude_cases", "envelope_span_cases", "envelope_geometry_cases", "envelope_pad_cases", "envelope_band_cases"]


def envelope_cases():
    return envelope_magnitude_cases() + envelope_span_cases() + envelope_geometry_cases() + envelope_pad_cases() + envelope_band_cases()


def recursive_gaussian_restated_cases():
    """The envelope cases that tests/restate.py's recursive-Gaussian restatement covers (tests/test_oracle.py): the default
    branch on an identity direction, of the families that run with that gradient on the GPU (tests/test_gpu_envelope.py)."""
    return [c for c in envelope_magnitude_cases() + envelope_geometry_cases()
            if c["variant"] == 0 and envelope_family(c) in ("magnitude", "spacing", "origin")
            and (c["geometry"] is None or c["geometry"]["direction"] == UNIT["direction"])]


def envelope_family(case):
    """'magnitude', 'span', 'spacing', 'origin', 'start', 'step', 'shear', 'relax_0', 'pad' or 'band'."""
    family = case["name"].split("/")[1]
    return "relax_0" if family.startswith("relax_0") else family


def linesearch_defined(case):
    """The rule above, on the inputs alone."""
    vox, _, _ = case_inputs(case)
    if vox.dtype.kind == "f":
        return bool(np.max(np.abs(vox.astype(np.float64) - float(iso_of(case)))) < LINESEARCH_BOUND)
    iso = int(iso_of(case))
    return max(abs(int(vox.max()) - iso), abs(int(vox.min()) - iso)) < LINESEARCH_BOUND


def bspline_envelope_cases():
    """The B-spline instantiations at the same edges; held as bspline_cases() are, the binary against the host walk and the
    HIP walk against the binary (there is no oracle for it)."""
    out = []
    walk = dict(threshold=0.001, step=0.2, relax=0.9, max_steps=8)
    vol = lambda s=1.0, dt="float32": dict(kind="field", dtype=dt, shape=[7, 8, 9], seed=800, scale=s)
    for ip in ("bspline_f", "bspline_d"):
        add = lambda name, v, **kw: out.append(_case("envelope_bspline/%s_%s" % (name, ip), v, 0.0, interp=ip, **dict(walk, **kw)))
        add("origin_1e+07", vol(), geometry=dict(ENV_ROTATED, origin=[1e7, -1e7, 1e7 / 3]))
        add("start_limit", vol(), geometry=dict(ENV_ROTATED, start=[ENV_LIMIT, -ENV_LIMIT, ENV_LIMIT - 9]))
        add("spacing_isotropic_0.0001", vol(), geometry=dict(UNIT, spacing=[1e-4, 1e-4, 1e-4]), step=0.2e-4)
        add("spacing_10000_1_0.0001", vol(), geometry=dict(UNIT, spacing=[1e4, 1.0, 1e-4]), step=0.2e-4)
        for s in ENV_BSPLINE_SCALES:
            add("magnitude_float32_%g" % s, vol(s), threshold=0.0)          # (no threshold a scaled-down field meets at once)
        add("magnitude_float64_1e+200", vol(1e200, "float64"), threshold=0.0)
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
    return pixel_type_cases() + cast_cases() + geometry_cases() + quirk_cases() + walk_cases() + border_cases() + envelope_cases()


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
