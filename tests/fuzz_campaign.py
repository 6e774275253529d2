#!/usr/bin/env python3
"""A differential campaign of the HIP path against the oracle, longer and wider than the suite's fixed cases -- run by hand on
a GPU box, its summary committed under profiles/:

    python tests/fuzz_campaign.py --seconds 600 --seed 1 > gpurun_out/fuzz_seed1.log

Every case is a pure function of (seed, case): draw_case() draws a RECIPE from np.random.default_rng([seed, case]) -- no GPU,
no oracle; the recipe survives JSON and holds all that is needed to build the voxels again --, expected() asks the references
for the mesh (and the normals, the cell pixels, the components), run_case() asks the library.  A recipe a run printed replays alone:

    python tests/fuzz_campaign.py --seed 1 --case 4711          (or --replay '<the recipe>' / --replay recipe.json)

(with the options the run had: --big, --max-voxels, --kind ... enter the draw; a FAILED line holds the whole recipe and needs
none.  The replay runs on a fresh context: a difference that needs what earlier cases left there shows in the run alone.)

A recipe holds a volume (shape with ragged / whole-word / one-voxel-thick rows, one of the ten pixel types, a noise, blob,
plane or shell field, blanked slices for quirk Q1, non-finite voxels now and then), a geometry (spacing, origin, a rotation or a
flip as direction matrix, a start index), the filter's eight parameters, a projection branch and

  kind    whole   the volume as it is, through one of the eight routes of the C ABI -- host upload, resident volume, streamed
                  upload, Z-slabs stitched by hand, count + emit, a held gradient (quirk Q3), a development switch that forces a
                  fallback kernel;                                       reference: the oracle on the volume
          border  cuberille_set_border(1, c): host, device, stream, count + emit;
                                                                         reference: the oracle on np.pad(vox, 1, c), start - 1
          region  cuberille_set_region on a buffer larger than the box: host (plain, or the chunk pipeline forced), device,
                  count + emit;                                          reference: the oracle on the contiguous crop, start moved
          band    cuberille_set_band: host, device, count + emit;        reference: the oracle on test_band.band_image
          bspline cuberille_set_interpolator, 32 / 64 bits: host, device, stream;
                                         reference: the oracle's lattice points walked by the drop-in's host walk (a subprocess)
  normals cuberille_set_point_normals on;   reference: normals_ref.normals on the frame image at the REFERENCE's points
  cell_pixels  cuberille_set_cell_pixels on, on every route of one whole volume (the held gradient too, not the slabs), every
          kind, with or without normals;   reference: cell_pixels_ref.cell_pixels on the view's frame BEFORE the band mapping
          (the caller's raw pixel; the ring's constant where the ring is inside), compared as bytes
  components   cuberille_set_components on, the same routes and kinds (frames of up to COMPONENTS_MAX_VOXELS voxels: the
          reference's time);   reference: components_ref.components on the REFERENCE's cells -- three rows as bytes, K, and the
          definition's properties (test_components.check_properties)
  keep    (with components) cuberille_keep_components behind the last extraction, one stage or two -- largest, a minimum of
          cells picked among 0, max + 1 and the sorted counts' quantiles, a mask drawn from a stream of its own, kept bytes of
          2 .. 255 among them; every argument resolved on the REFERENCE's counts (keep_arguments) --, and behind every repeat that
          runs with components on.  After each stage everything the library says of its mesh is taken again: counts, points and
          cells through the route's own accessor, normals, cell pixels, the three rows, K, the device pointers, the counters;
                                         reference: keep_ref.keep on the reference mesh, components_ref's rows, normals_ref's
          normals and cell_pixels_ref's pixels -- the kept mesh is held to the oracle's own mesh, never to rows the library
          handed out.  The context stays as the keep left it: rows sized by the kept counts in place, the extraction's as spare
          rows -- the next case toggles settings, changes the pixel width, or launches blindly on that (counted: behind_keep)
  emit_offset  count + emit: the id offset handed to cuberille_emit -- 0, below 10^6, or 2^32 and more --, taken off the cells
          before the comparison; labels and pixels never carry it
  repeat  the case three times on the context, the third mesh compared (the blind launch sized by its own history); the first
          of the three runs with cell pixels and components OFF, and its points, cells and counters are the bytes of the third
  refusal one call the header lists as refused, made first: CUBERILLE_ERR_ARGUMENT with that refusal's words, and the case
          itself still equal; refusal_slab (whole volumes): with cell pixels or components on, cuberille_count of a slab that
          is not the whole volume, likewise

and every case runs on the context the cases before it used, whatever they left there: the settings of a case are taken back
behind it, the workspace and its history stay, and so do the normals row of a normals case, the pixel row of a cell-pixel case
and the rows of a components case unless the recipe drops them -- the next case with that setting then finds rows sized by
another mesh, of another view, pixel width or cell count (counted in the summary).  Comparisons are exact: ids, cell order,
the float bits of every coordinate (conftest.assert_same_mesh), the bits of every normal (normals_ref.same_normals), the walk's
counters, the bytes of every cell pixel and label.  TEST INFRASTRUCTURE: the oracle is the checker here, never the thing
measured or shipped.
What was drawn before cell pixels and components existed comes from the stream it came from, draw for draw; the keys above that
are new come from a second one, the keep from a third (draw_case; tests/golden/campaign_recipe_digests.json and
campaign_celldata_recipe_digests.json): the cases of the committed logs replay.
Prints one progress line every ~20 s; exit code 1 with the failing case's recipe if a mesh ever differs."""
import argparse
import copy
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
from conftest import assert_same_mesh  # noqa: E402

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64, np.int64, np.uint64]
XS = [1, 2, 5, 31, 63, 64, 65, 100, 127, 128, 129, 192, 200, 256, 257, 320]

KINDS = ["whole", "border", "region", "band", "bspline"]
ROUTES = {"whole": ["host", "device", "stream", "slabs", "thin_slabs", "count_emit", "held", "switch"],
          "border": ["host", "device", "stream", "count_emit"],
          "region": ["host", "host_chunked", "device", "count_emit"],
          "band": ["host", "device", "count_emit"],
          "bspline": ["host", "device", "stream"]}
# the development switches of the "switch" route; a view case may carry one too (the views share the whole volume's launch path:
# count, points, cells and the walk all read Tuning, whatever the sampler's form)
SWITCHES = [("no_cmap", 1), ("no_heads", 1), ("no_vqueue", 1), ("count_variant", 1), ("count_variant", 2), ("count_variant", 3),
            ("count_variant", 0), ("points_variant", 2), ("points_variant", 1), ("points_variant", 0), ("classify_variant", 1),
            ("proj_literal", 1), ("cmap_linear", 1), ("no_stream_classify", 1), ("proj_short", 1), ("proj_short", 0),
            ("count_no_fold", 1)]
# the routes on which cuberille_set_point_normals is offered (not on slabs, not with a held gradient)
NORMALS_ROUTES = ("host", "host_chunked", "device", "stream", "count_emit", "switch")
# normals_ref.gradient_image calls the oracle once per voxel from Python (about 2 us each): a frame of this many voxels takes
# well under a second; a larger case is drawn without normals
NORMALS_MAX_VOXELS = 40000
# the routes on which cuberille_set_cell_pixels and cuberille_set_components are offered: every route of one whole volume -- the
# held gradient too: the header lists no refusal of either with it --, not the slabs
CELLDATA_ROUTES = ("host", "host_chunked", "device", "stream", "count_emit", "switch", "held")
# components_ref.components propagates minima through numpy until nothing moves: measured on the largest cases of seed 1 at
# --max-voxels 900000 (frames of 350 000 to 480 000 voxels, noise meshes of up to 785 000 cells) it takes 0.2 to 2.3 s, at most
# 5 us per voxel of the frame -- a frame of this many voxels stays below 0.75 s, a larger case is drawn without components.
# cell_pixels_ref took at most 0.05 s on the same cases: no cap.
COMPONENTS_MAX_VOXELS = 150000
# one subprocess per B-spline case, and ITK's class evaluates 64 taps per step on one thread: small volumes only
BSPLINE_MAX_VOXELS = 12000
COUNTERS = ("proj_iterations", "proj_stop_threshold", "proj_stop_steps")
REFUSALS = {"whole": ["normals_rg", "bspline_variant", "bspline_held", "cell_pixels_slab", "components_slab"],
            "bspline": ["normals_rg", "bspline_variant", "bspline_held"],
            "border": ["pair", "variant", "held", "rg"],
            "region": ["pair", "stream", "variant", "held", "rg"],
            "band": ["pair", "stream", "variant", "held", "rg"]}
# recipe["refusal"] is drawn among the first names only, as it was before the two slab refusals existed (the draws of the first
# stream do not move: tests/golden/campaign_recipe_digests.json); those two are drawn from the second stream as recipe["refusal_slab"]
REFUSALS_FIRST_STREAM = {"whole": 3}
SLAB_REFUSALS = {"cell_pixels_slab": "cell_pixels", "components_slab": "components"}
DEFAULT_OPTIONS = dict(max_voxels=900000, big=False, recursive_gaussian=False, kind=None, dtype=None, route=None, max_rows=None,
                       cell_pixels=None, components=None, keep=None, envelope=False)
# --envelope: the edges of the number range (tests/ref_filter.py's envelope cases, drawn).  The line search starts its best
# metric at 10000 (txx:405): where |voxel - iso| reaches that everywhere the reference never assigns its result, so a
# line-search case redraws its voxel scale until max |voxel - iso| over the finite voxels is below it.
ENVELOPE_VOXEL_EXP = {"float32": (-120, 126), "float64": (-1000, 1000)}
ENVELOPE_SPACING_EXP = (-100, 100)
ENVELOPE_LIMIT = 1 << 30
LINESEARCH_BOUND = 10000.0
KEEP_RULES = ("largest", "min_cells", "mask")


def draw_field(rng, shape, dt, big=True):
    """(voxels, iso): the inside set is what matters to the topology, the values to the walk.  big False: the 8-byte types
    stay below 2^53 (the draw is made all the same, so the stream does not depend on it)."""
    nz, ny, nx = shape
    kind = rng.choice(["noise", "blobs", "plane", "shell", "smooth_noise"])
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    if kind == "noise":
        f = rng.random(shape) - rng.choice([0.05, 0.3, 0.5, 0.8])
    elif kind == "smooth_noise":
        f = rng.random(shape)
        for ax in range(3):
            if shape[ax] > 2:
                f = (f + np.roll(f, 1, ax) + np.roll(f, -1, ax)) / 3.0
        f = f - np.quantile(f, rng.choice([0.2, 0.5, 0.85]))
    elif kind == "blobs":
        f = np.full(shape, -1.0)
        for _ in range(int(rng.integers(1, 5))):
            c = [rng.uniform(0, n) for n in (nx, ny, nz)]
            r = rng.uniform(1.0, 0.6 * max(2.0, min(max(nx, 2), 24)))
            s = rng.uniform(0.5, 2.0, size=3)
            d = np.sqrt(((x - c[0]) / s[0]) ** 2 + ((y - c[1]) / s[1]) ** 2 + ((z - c[2]) / s[2]) ** 2)
            f = np.maximum(f, (r - d) / max(r, 1.0))
    elif kind == "plane":
        n = rng.normal(size=3)
        n /= np.linalg.norm(n) + 1e-9
        f = (x - nx / 2.0) * n[0] + (y - ny / 2.0) * n[1] + (z - nz / 2.0) * n[2] + rng.uniform(-1, 1)
        f = f / (np.abs(f).max() + 1e-9)
    else:
        c = [nx / 2.0 + rng.uniform(-2, 2), ny / 2.0 + rng.uniform(-2, 2), nz / 2.0 + rng.uniform(-2, 2)]
        d = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
        r = rng.uniform(1.5, 0.5 * max(3.0, min(nx, ny * 3, nz * 3)))
        f = (1.0 - np.abs(d - r) / max(r, 1.0)) - 0.8
    dt = np.dtype(dt)
    if dt.kind == "f":
        vox = (f * rng.choice([1.0, 37.5, 1e-3])).astype(dt)
        iso = 0.0
        if rng.random() < 0.06 and vox.size > 8:              # non-finite voxels (quirk Q4's relatives)
            idx = tuple(rng.integers(0, n) for n in shape)
            vox[idx] = rng.choice([np.inf, -np.inf, np.nan])
    else:
        info = np.iinfo(dt)
        lo, hi = (0, min(info.max, 240)) if info.min == 0 else (max(info.min, -120), min(info.max, 120))
        mid = (lo + hi) / 2.0
        g = np.clip(mid + f * (hi - lo) * 0.5 * rng.choice([1.0, 0.3]), lo, hi)
        vox = np.rint(g).astype(dt)
        iso = int(np.rint(mid)) + int(rng.integers(0, 2))
        if dt.itemsize == 8 and rng.random() < 0.5 and big:       # beyond 2^53: a double cannot hold these
            off = (1 << 60) if info.min == 0 else -(1 << 60)
            vox = vox + dt.type(off)
            iso = int(iso) + off
    if rng.random() < 0.25 and nz > 2:
        for _ in range(int(rng.integers(1, 3))):
            vox[int(rng.integers(0, nz))] = vox.min()                 # an empty slice (or a full one when min is inside)
    return np.ascontiguousarray(vox), iso


def to_device(torch, a):
    """A host array on the GPU as a tensor of the same bytes (torch has no arithmetic for some unsigned types: signed views)."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "u" and a.dtype.itemsize > 1:
        a = a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return torch.from_numpy(a).cuda()


def draw_geometry(rng):
    spacing = tuple(float(v) for v in rng.choice([0.25, 0.5, 1.0, 1.0, 1.7, 3.0], size=3))
    origin = tuple(float(v) for v in rng.normal(0, 7, size=3).round(3)) if rng.random() < 0.7 else (0.0, 0.0, 0.0)
    u = rng.random()
    if u < 0.55:
        d = np.eye(3)
    elif u < 0.85:
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        d = q
    else:
        d = np.eye(3)[rng.permutation(3)] * rng.choice([-1.0, 1.0], size=3)[:, None]
    return spacing, origin, np.ascontiguousarray(d, dtype=np.float64)


def geometry_form(recipe):
    """identity / axis-aligned / general, by the rule of the walk's three forms (cuberille_kernels.hip, launch_project): the unit
    direction matrix and a caller's region that starts at index 0 with unit spacing is the identity form, with any other spacing
    the axis-aligned one; everything else -- a rotation, a flip, a region that starts elsewhere -- takes the general form.  The
    kernels of cuberille_set_region take the start index at run time in every form: there the matrices alone decide."""
    d = np.asarray(recipe["direction"], dtype=np.float64)
    moved = tuple(int(v) for v in recipe["index_start"]) != (0, 0, 0) and recipe["kind"] != "region"
    if not np.array_equal(d, np.eye(3)) or moved:
        return "general"
    return "identity" if tuple(recipe["spacing"]) == (1.0, 1.0, 1.0) else "axis-aligned"


# ---- the voxels of a recipe -----------------------------------------------------------------------------------------------
def _field(spec):
    vox, iso = draw_field(np.random.default_rng(spec["rng"]), tuple(spec["shape"]), np.dtype(spec["dtype"]), big=spec.get("big", True))
    if spec.get("scale_exp"):                              # --envelope: a power of two, so the scaling is exact until it leaves the type
        with np.errstate(over="ignore", under="ignore"):
            vox = np.ldexp(vox, int(spec["scale_exp"])).astype(vox.dtype)
    return vox, iso


def _draw_envelope(rng, dt):
    """The envelope's own stream: a power-of-two voxel scale (float types), a power-of-two spacing scale, an origin of up to
    1e9, and in one case of ten a start index near +-2^30 (far enough inside for a border's ring and a region's box)."""
    both = {name: int(rng.integers(lo, hi + 1)) for name, (lo, hi) in sorted(ENVELOPE_VOXEL_EXP.items())}
    env = dict(voxel_exp=both.get(np.dtype(dt).name, 0), spacing_exp=int(rng.integers(ENVELOPE_SPACING_EXP[0], ENVELOPE_SPACING_EXP[1] + 1)),
               origin=[float(v) for v in rng.uniform(-1.0, 1.0, size=3) * 10.0 ** rng.uniform(0.0, 9.0)], start=None)
    near, signs, inside = rng.random() < 0.1, rng.choice([-1, 1], size=3), rng.integers(40, 100, size=3)
    if near:
        env["start"] = [int(s) * (ENVELOPE_LIMIT - int(r)) for s, r in zip(signs, inside)]
    return env


def linesearch_defined(vox, iso):
    """The campaign's form of the 10000 rule: max |voxel - iso| < 10000 over the FINITE voxels.  Weaker on purpose than
    ref_filter.linesearch_defined, which takes the whole volume: draw_field pokes an infinite or NaN voxel now and then, no scale
    brings that under the bound, and the campaign's truth is the oracle, which is defined there -- the rule only keeps the
    scaled field itself where the reference is defined too."""
    v = vox[np.isfinite(vox)] if vox.dtype.kind == "f" else vox
    if not v.size:
        return True
    if vox.dtype.kind == "f":
        return bool(np.max(np.abs(v.astype(np.float64) - float(iso))) < LINESEARCH_BOUND)
    return max(abs(int(v.max()) - int(iso)), abs(int(v.min()) - int(iso))) < LINESEARCH_BOUND


def voxels(recipe):
    """The buffer the library is handed, built again from the recipe alone."""
    return _field(recipe["field"])[0]


def frame_start(recipe):
    s = [int(v) for v in recipe["index_start"]]
    if recipe["kind"] == "border":
        return tuple(v - 1 for v in s)
    if recipe["kind"] == "region":
        return tuple(a + int(b) for a, b in zip(s, recipe["region"]["start"]))
    return tuple(s)


def frame(recipe, vox=None):
    """(image, start index) the reference is handed: the volume, its padded copy, the crop, or B."""
    vox = voxels(recipe) if vox is None else vox
    kind = recipe["kind"]
    if kind == "border":
        c = recipe["border"]["value"]
        c = float(c) if vox.dtype.kind == "f" else int(c)
        return np.pad(vox, 1, constant_values=vox.dtype.type(c)), frame_start(recipe)
    if kind == "region":
        (x0, y0, z0), (nx, ny, nz) = recipe["region"]["start"], recipe["region"]["size"]
        return np.ascontiguousarray(vox[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx]), frame_start(recipe)
    if kind == "band":
        from test_band import band_image
        b = recipe["band"]
        return np.ascontiguousarray(band_image(vox, _num(b["lower"]), _num(b["upper"]), _num(b["inside"]), _num(b["outside"]))[0]), frame_start(recipe)
    return vox, frame_start(recipe)


def _num(v):
    """A value of a recipe: JSON has no infinities, so the float bounds that are not finite travel as strings."""
    return float(v) if isinstance(v, str) else v


def _jnum(v):
    if isinstance(v, (float, np.floating)) and not np.isfinite(v):
        return repr(float(v))
    if isinstance(v, (int, np.integer)):
        return int(v)
    return float(v)


def inside_set(img, iso):
    """The sweep's predicate !(pixel < iso) in the pixel type (a NaN pixel is inside): cell_pixels_ref.inside_of."""
    import cell_pixels_ref
    return cell_pixels_ref.inside_of(img, iso if img.dtype.kind == "f" else int(iso))


def has_q1_gap(img, iso):
    """An empty slice between occupied ones in the frame (quirk Q1)."""
    occ = np.flatnonzero(inside_set(img, iso).reshape(img.shape[0], -1).any(axis=1))
    return len(occ) >= 2 and (occ[-1] - occ[0] + 1) > len(occ)


# ---- 1. the recipe ---------------------------------------------------------------------------------------------------------
def draw_case(seed, case, options=None):
    """The recipe of case `case` of seed `seed`: a dict of plain numbers, lists and strings.  options: DEFAULT_OPTIONS' keys
    -- max_voxels, big (up to 120 rows and slices), recursive_gaussian, and kind / dtype / route / cell_pixels / components /
    keep to fix what a stratified slice fixes (they are recorded, so the recipe alone still says everything; cell_pixels /
    components / keep True: every case that can takes it; keep may name the rule).  Needs no GPU and no oracle.

    Two streams: np.random.default_rng([seed, case]) draws everything the campaign drew before cell pixels and components
    existed, in the order it drew it then -- no draw of it may move, tests/golden/campaign_recipe_digests.json pins them --, and
    np.random.default_rng([seed, case, 3]) draws cell_pixels, components, drop_cell_rows, emit_offset and refusal_slab -- pinned in
    turn by tests/golden/campaign_celldata_recipe_digests.json --, np.random.default_rng([seed, case, 4]) draws keep
    ([seed, case, 1] is the field's stream, [seed, case, 2] that of a held case's first volume, [seed, case, 5] a keep's mask,
    [seed, case, 6] the drop-in campaign's).  options["envelope"]: np.random.default_rng([seed, case, 7]) draws recipe["envelope"]
    (_draw_envelope; tests/golden/campaign_envelope_recipe_digests.json); off, no draw is made and no key is added."""
    opt = dict(DEFAULT_OPTIONS)
    opt.update(options or {})
    rng = np.random.default_rng([int(seed), int(case)])
    kind = opt["kind"] or str(rng.choice(KINDS, p=[0.46, 0.15, 0.17, 0.15, 0.07]))
    top = opt["max_rows"] or (120 if opt["big"] else 40)
    nx = int(rng.choice(XS))
    ny = int(rng.integers(1, top + 1))
    nz = int(rng.integers(1, top + 1))
    cap = min(opt["max_voxels"], BSPLINE_MAX_VOXELS) if kind == "bspline" else opt["max_voxels"]
    if kind == "bspline":
        nx = int(rng.choice(XS[:8]))
    while nx * ny * nz > cap:
        ny = max(1, ny // 2)
        nz = max(1, nz // 2)
        if ny == 1 and nz == 1 and nx * ny * nz > cap:
            nx = max(1, nx // 2)
    dt = np.dtype(opt["dtype"] if opt["dtype"] is not None else DTYPES[int(rng.integers(0, len(DTYPES)))])
    spacing, origin, direction = draw_geometry(rng)
    start = tuple(int(v) for v in rng.integers(-3000, 3000, size=3)) if rng.random() < 0.3 else (0, 0, 0)
    env = env_rng = None
    if opt["envelope"]:
        # (the first stream draws what it always drew; the envelope moves spacing, origin and start behind it, and the step,
        #  a multiple of the smallest spacing, with them)
        env_rng = np.random.default_rng([int(seed), int(case), 7])
        env = _draw_envelope(env_rng, dt)
        spacing = tuple(float(np.ldexp(v, env["spacing_exp"])) for v in spacing)
        origin = tuple(env["origin"])
        start = tuple(env["start"]) if env["start"] else start
    project = bool(rng.random() < 0.75)
    variant = int(rng.choice([0, 0, 0, 1, 2])) if project and kind == "whole" else 0
    kw = dict(triangles=bool(rng.integers(0, 2)), project=project,
              threshold=float(rng.choice([0.0, 0.01, 0.2, 5.0])) * (1.0 if dt.kind != "f" else 0.05),
              step=float(rng.choice([0.1, 0.25, 0.6, 1.3])) * min(spacing),
              relax=float(rng.choice([0.5, 0.9, 0.95, 1.0])), max_steps=int(rng.choice([0, 1, 4, 25, 50])), variant=variant)
    route = opt["route"] or str(rng.choice(ROUTES[kind]))
    recipe = dict(seed=int(seed), case=int(case), kind=kind, dtype=dt.name, route=route, kw=kw, spacing=list(spacing), origin=list(origin),
                  direction=direction.tolist(), index_start=list(start))

    # the buffer: the box of a region case lies inside a larger one
    shape = [nz, ny, nx]
    if kind == "region":
        form = str(rng.choice(["full_xy", "thin", "residue", "words_in_ragged", "ragged_in_words", "whole_buffer", "any"]))
        size = [nx, ny, nz]
        if form == "thin":
            size[int(rng.integers(0, 3))] = 1
        if form == "words_in_ragged":
            size[0] = int(rng.choice([64, 128, 192]))
        lo = [int(rng.integers(0, 17)), int(rng.integers(0, 4)), int(rng.integers(0, 4))]       # x0: every byte residue mod 16
        hi = [int(rng.integers(0, 9)), int(rng.integers(0, 4)), int(rng.integers(0, 4))]
        if form == "full_xy":
            lo[0] = lo[1] = hi[0] = hi[1] = 0
            lo[2] += 1
        elif form == "whole_buffer":
            lo, hi = [0, 0, 0], [0, 0, 0]
        elif form == "words_in_ragged":
            hi[0] += (lo[0] + size[0] + hi[0]) % 64 == 0
        elif form == "ragged_in_words":
            hi[0] += -(lo[0] + size[0] + hi[0]) % 64
        buf = [lo[k] + size[k] + hi[k] for k in range(3)]
        while buf[0] * buf[1] * buf[2] > 2 * opt["max_voxels"] and (size[1] > 1 or size[2] > 1):
            size[1], size[2] = max(1, size[1] // 2), max(1, size[2] // 2)
            buf = [lo[k] + size[k] + hi[k] for k in range(3)]
        recipe["region"] = dict(form=form, start=lo, size=size)
        shape = [buf[2], buf[1], buf[0]]
    recipe["field"] = dict(rng=[int(seed), int(case), 1], shape=shape, dtype=dt.name, big=kind != "bspline")
    if env:
        recipe["envelope"] = env
        recipe["field"]["scale_exp"] = env["voxel_exp"]
    vox, iso = _field(recipe["field"])
    while env and variant == 2 and dt.kind == "f" and not linesearch_defined(vox, iso):       # (integer voxels are not scaled)
        lo, hi = ENVELOPE_VOXEL_EXP[dt.name]
        env["voxel_exp"] = recipe["field"]["scale_exp"] = int(env_rng.integers(lo, hi + 1))
        vox, iso = _field(recipe["field"])
    recipe["iso"] = iso if dt.kind == "f" else int(iso)

    if kind == "border":
        recipe["border"] = dict(value=_jnum(_draw_border_value(rng, dt, iso)))
    elif kind == "band":
        recipe["band"] = _draw_band(rng, dt, vox)
        recipe["iso"] = recipe["band"].pop("iso")
    elif kind == "bspline":
        recipe["bspline"] = dict(bits=int(rng.choice([32, 64])))

    if kind == "whole":
        _draw_whole_route(rng, recipe, vox, opt)
    elif kind == "region" and route == "host_chunked":
        recipe["chunk_kib"] = int(rng.choice([1, 4, 16, 64]))
    if kind in ("border", "region", "band") and rng.random() < 0.2:
        name, val = SWITCHES[int(rng.integers(0, len(SWITCHES)))]
        recipe["switch"] = [name, val]
    if kind in ("border", "band") and recipe["route"] == "host" and rng.random() < 0.15:
        recipe["chunk_kib"] = int(rng.choice([1, 4, 16, 64]))

    img, _ = frame(recipe, vox)
    want_normals = rng.random() < 0.3
    recipe["normals"] = bool(want_normals and recipe["route"] in NORMALS_ROUTES and img.size <= NORMALS_MAX_VOXELS
                             and recipe["kw"].get("gradient", 0) == 0)
    recipe["repeat"] = 3 if rng.random() < 0.12 and recipe["route"] not in ("slabs", "thin_slabs", "held") else 1
    pick = rng.random() < 0.15, int(rng.integers(0, 8))
    if pick[0] and recipe["route"] not in ("slabs", "thin_slabs", "held"):
        names = REFUSALS[kind][:REFUSALS_FIRST_STREAM.get(kind)]
        recipe["refusal"] = names[pick[1] % len(names)]
        if recipe["refusal"] == "rg" and min(recipe["field"]["shape"]) < 4:
            recipe["refusal"] = "variant"       # (shorter lines are refused for their length, not for the view)
    # behind a normals case the setting stays on -- its row, sized by this mesh, is there for the next case -- or is switched off
    recipe["drop_normals_row"] = bool(rng.random() < 0.25)
    _draw_cell_data(np.random.default_rng([int(seed), int(case), 3]), recipe, opt, img.size)
    _draw_keep(np.random.default_rng([int(seed), int(case), 4]), recipe, opt)
    return recipe


def _draw_cell_data(rng, recipe, opt, frame_voxels):
    """The second stream: cell pixels, components (independent of each other, of normals and of the kind: neither pass depends
    on the interpolator), whether their rows stay behind the case, the id offset of a count + emit, a refused slab."""
    offered = {"cell_pixels": recipe["route"] in CELLDATA_ROUTES,
               "components": recipe["route"] in CELLDATA_ROUTES and frame_voxels <= COMPONENTS_MAX_VOXELS}
    draws = {"cell_pixels": bool(rng.random() < 0.35), "components": bool(rng.random() < 0.35)}
    for key in ("cell_pixels", "components"):
        recipe[key] = bool(offered[key] and (draws[key] if opt[key] is None else opt[key]))
    # behind the case the two settings are switched off, which frees their rows, or left on for the next case
    recipe["drop_cell_rows"] = bool(rng.random() < 0.25) or recipe["route"] == "held"      # (held: a context of its own)
    u, small, high = rng.random(), int(rng.integers(1, 10 ** 6)), bool(rng.random() < 0.4)
    if recipe["route"] == "count_emit":
        recipe["emit_offset"] = 0 if u < 0.5 else (2 ** 32 + small if high else small)
    name = ["cell_pixels_slab", "components_slab"][int(rng.integers(0, 2))]
    if rng.random() < 0.08 and recipe["kind"] == "whole" and recipe["route"] not in ("slabs", "thin_slabs", "held"):
        recipe["refusal_slab"] = name


def _draw_keep(rng, recipe, opt):
    """The third stream: recipe["keep"], a cuberille_keep_components behind the case's last extraction (and behind every repeat
    that runs with components on) -- None unless components are on.  The draw cannot know K, so it holds a rule and the means to
    resolve its argument later (keep_arguments):

      {"rule": "largest"}
      {"rule": "min_cells", "pick": "zero" (keeps all) | "above_max" (max + 1: drops all) | "quantile", "quantile": q,
       "plus_one": bool}                    quantile: counts[j] or counts[j] + 1 at j = floor(q K) of the sorted counts
      {"rule": "mask", "stream": [seed, case, 5], "form": "random" | "all_but_largest", "p": the probability of a kept byte,
       "odd_bytes": bool}                   odd_bytes: some kept bytes hold a value of 2 .. 255 (the ABI says non-zero)
      "then": None, or a second stage ("largest" or "min_cells") resolved on the first keep's result

    opt["keep"]: None (about half of the components cases), True / False (every case that can / none), or a rule's name (every
    case that can, with that rule).  Every draw is made whatever the options and the rule are."""
    wanted = bool(rng.random() < 0.5)
    rule = KEEP_RULES[int(rng.integers(0, 3))]

    def min_cells():
        u, q, plus = rng.random(), float(rng.random()), bool(rng.integers(0, 2))
        pick = "zero" if u < 0.1 else ("above_max" if u < 0.2 else "quantile")
        return dict(rule="min_cells", pick=pick, quantile=round(q, 6), plus_one=plus)
    stages = {"largest": dict(rule="largest"), "min_cells": min_cells(),
              "mask": dict(rule="mask", stream=[recipe["seed"], recipe["case"], 5],
                           form="all_but_largest" if rng.random() < 0.2 else "random",
                           p=float(rng.choice([0.0, 0.1, 0.5, 0.5, 0.9, 1.0])), odd_bytes=bool(rng.random() < 0.4))}
    second = [None, dict(rule="largest"), min_cells()][int(rng.choice([0, 0, 0, 0, 1, 2, 2]))]
    if isinstance(opt["keep"], str):
        assert opt["keep"] in KEEP_RULES, opt["keep"]
        wanted, rule = True, opt["keep"]
    elif opt["keep"] is not None:
        wanted = bool(opt["keep"])
    recipe["keep"] = dict(stages[rule], then=second) if wanted and recipe["components"] else None


def keep_stages(keep):
    """The stages of a recipe's keep in the order they run: one, or two with `then`."""
    if not keep:
        return []
    first = {k: v for k, v in keep.items() if k != "then"}
    return [first] + ([keep["then"]] if keep.get("then") else [])


def keep_arguments(stage, component_cells):
    """(rule, n, mask) of cuberille_keep_components for one stage on a mesh with these component counts -- the REFERENCE's, never
    the library's.  Pure: the mask's bytes come from the stage's own stream."""
    counts = np.asarray(component_cells, dtype=np.uint64)
    k = len(counts)
    rule = stage["rule"]
    if rule == "largest":
        return "largest", 0, None
    if rule == "min_cells":
        if stage["pick"] == "zero":
            return "min_cells", 0, None
        if stage["pick"] == "above_max":
            return "min_cells", (int(counts.max()) if k else 0) + 1, None
        at = int(np.sort(counts)[min(int(stage["quantile"] * k), k - 1)]) if k else 0
        return "min_cells", at + int(bool(stage["plus_one"])), None
    assert rule == "mask", rule
    rng = np.random.default_rng(stage["stream"])
    kept, odd, values = rng.random(k) < stage["p"], rng.random(k) < 0.3, rng.integers(2, 256, size=k)
    if stage["form"] == "all_but_largest":
        kept = np.arange(k) != (int(np.argmax(counts)) if k else -1)
    mask = np.where(kept, np.where(odd & bool(stage["odd_bytes"]), values, 1), 0).astype(np.uint8)
    return "mask", 0, mask


def _draw_border_value(rng, dt, iso):
    """What border_check accepts for the pixel type: `converts` takes a value inside the range of an 8- to 32-bit integer type
    and ANY double for the floating types -- a NaN or an infinite ring included --; the 64-bit integer types take what they hold."""
    if dt.kind == "f":
        fin = np.finfo(dt)
        return [float(fin.min), float(fin.max), 0.0, -0.0, iso - 1.0, iso + 1.0, float(iso), float("inf"), float("-inf"), float("nan")][int(rng.integers(0, 10))]
    info = np.iinfo(dt)
    choices = [int(info.min), int(info.max), 0 if info.min <= 0 else int(info.min), int(iso) - 1, int(iso), int(iso) + 1, int(iso) - 7, int(iso) + 7]
    return int(min(max(choices[int(rng.integers(0, len(choices)))], int(info.min)), int(info.max)))


def _draw_band(rng, dt, vox):
    """Bounds from the volume's own values (the band is neither empty nor everything in most cases); now and then lower ==
    upper, the inverted choice, the constant case, and for the floating types signed zeros and infinities as bounds."""
    finite = vox[np.isfinite(vox)] if dt.kind == "f" else vox.ravel()
    vals = np.unique(finite)
    if len(vals) == 0:
        vals = np.zeros(1, dtype=dt)
    a, b = sorted(int(v) for v in rng.integers(0, len(vals), size=2))
    u = rng.random()
    if u < 0.15:
        b = a                                                    # a single label
    lower, upper = vals[a].item(), vals[b].item()
    if dt.kind == "f":
        w = rng.random()
        if w < 0.08:
            lower = float("-inf")
        elif w < 0.16:
            upper = float("inf")
        elif w < 0.22 and upper >= 0.0:
            lower = [0.0, -0.0][int(rng.integers(0, 2))]
        elif w < 0.28 and lower <= 0.0:
            upper = [0.0, -0.0][int(rng.integers(0, 2))]
    if dt.kind == "f":
        triples = [(1.0, 0.0, 1.0), (0.0, 1.0, 1.0), (200.0, 10.0, 100.0), (-2.5, 7.25, 0.0), (1.0, 0.0, 0.5)]
    elif dt == np.dtype(np.int8):
        triples = [(1, 0, 1), (0, 1, 1), (100, 10, 50), (-100, 100, 0)]
    else:
        triples = [(1, 0, 1), (0, 1, 1), (200, 10, 100), (7, 3, 5)]
    inside, outside, iso = triples[int(rng.integers(0, len(triples)))]
    if dt.itemsize == 8 and dt.kind in "iu" and rng.random() < 0.4:      # B's two values and the iso value past 2^53 as well
        off = (1 << 61) + 1
        inside, outside, iso = inside + off, outside + off, iso + off
    if rng.random() < 0.07:
        outside = inside                                          # bin == bout: the bit volume is constant, the mesh empty
    return dict(lower=_jnum(lower), upper=_jnum(upper), inside=_jnum(inside), outside=_jnum(outside), iso=_jnum(iso))


def _draw_whole_route(rng, recipe, vox, opt):
    """The draws the eight routes of a whole volume make beyond the route's name."""
    route, kw = recipe["route"], recipe["kw"]
    nz, ny, nx = vox.shape
    dt = vox.dtype
    if opt["recursive_gaussian"] and kw["project"] and min(nx, ny, nz) >= 4 and route in ("host", "device", "stream", "count_emit", "switch"):
        kw["gradient"] = 1                         # USE_GRADIENT_RECURSIVE_GAUSSIAN (whole volumes, four voxels along every axis)
    if route == "switch":
        name, val = SWITCHES[int(rng.integers(0, len(SWITCHES)))]
        recipe["switch"] = [name, val]
    elif route == "held":
        # quirk Q3: a first volume of its own (same pixel type), then this one along the first one's gradient
        fshape = [int(rng.integers(2, 20)), int(rng.integers(2, 20)), int(rng.choice([3, 17, 64, 70]))]
        fs, fo, fd = draw_geometry(rng)
        fstart = [int(v) for v in rng.integers(-100, 100, size=3)] if rng.random() < 0.3 else [0, 0, 0]
        kw["project"] = True
        recipe["first"] = dict(field=dict(rng=[recipe["seed"], recipe["case"], 2], shape=fshape, dtype=dt.name), spacing=list(fs),
                               origin=list(fo), direction=fd.tolist(), index_start=fstart)
    elif route in ("slabs", "thin_slabs"):
        thin = route == "thin_slabs"
        occupied = bool(inside_set(vox, recipe["iso"]).reshape(nz, -1).any(axis=1).all())
        coin = rng.random() < 0.5
        if nz < 3 or not occupied or kw["variant"] != 0 and (thin or coin):
            recipe["route"] = "host"        # (quirk Q1 across a cut needs the ranks' protocol: tests/test_gpu_slabs.py)
        else:
            ncut = int(rng.integers(1, min(4, nz - 1) + 1))
            recipe["cuts"] = [0] + sorted(set(int(v) for v in rng.integers(1, nz, size=ncut))) + [nz]


# ---- 2. the references -----------------------------------------------------------------------------------------------------
def _geo(recipe):
    return dict(spacing=tuple(recipe["spacing"]), origin=tuple(recipe["origin"]), direction=np.asarray(recipe["direction"], dtype=np.float64))


def _oracle_kw(recipe):
    return dict(recipe["kw"], **_geo(recipe))


def expected(oracle, recipe, vox=None):
    """{"mesh": the reference mesh (with .info, the walk's counters, where the reference has them), "normals": the reference
    normals or None, "cell_pixels": cell_pixels_ref's row or None, "components": components_ref's three rows ON THE REFERENCE'S
    CELLS or None, "kept": one keep_ref.Kept per stage of the recipe's keep, "keep_args": the (rule, n, mask) of each stage
    (kept_expected)}.  Never the library."""
    vox = voxels(recipe) if vox is None else vox
    img, start = frame(recipe, vox)
    okw = _oracle_kw(recipe)
    if recipe["kind"] == "bspline":
        mesh = _bspline_expected(oracle, recipe, img, start)
    elif recipe["route"] == "held":
        f = recipe["first"]
        first = (_field(f["field"])[0], tuple(f["spacing"]), tuple(f["origin"]), np.asarray(f["direction"], dtype=np.float64), tuple(f["index_start"]))
        mesh = oracle.run(img, recipe["iso"], first=first, index_start=start, **okw)
    else:
        mesh = oracle.run(img, recipe["iso"], index_start=start, **okw)
    normals = None
    if recipe.get("normals"):
        import normals_ref
        normals = normals_ref.normals(oracle, img, mesh.points, start, **_geo(recipe)) if len(mesh.points) else np.zeros((0, 3), dtype=np.float32)
    pixels = components = None
    if recipe.get("cell_pixels"):
        import cell_pixels_ref
        pixels = cell_pixels_ref.cell_pixels(*cell_pixels_view(recipe, vox), bool(recipe["kw"]["triangles"]))
    if recipe.get("components"):
        import components_ref
        components = components_ref.components(mesh.cells, len(mesh.points))
    kept, keep_args = kept_expected(recipe, mesh, normals, pixels, components)
    return {"mesh": mesh, "normals": normals, "cell_pixels": pixels, "components": components, "kept": kept, "keep_args": keep_args}


def kept_expected(recipe, mesh, normals, pixels, components):
    """(one keep_ref.Kept per stage of recipe["keep"], the (rule, n, mask) each stage resolves to): keep_ref.keep on the
    reference mesh, components_ref's rows, normals_ref's normals and cell_pixels_ref's pixels -- a stage behind another on the
    first one's result.  Offset 0: the reference's cells carry none."""
    import keep_ref
    kept, args = [], []
    if recipe.get("keep"):
        now = keep_ref.Kept(mesh.points, np.asarray(mesh.cells, dtype=np.uint64), components[0], components[1], components[2], normals, pixels)
        for stage in keep_stages(recipe["keep"]):
            rule, n, mask = keep_arguments(stage, now.component_cells)
            now = keep_ref.keep(keep_ref.decide(rule, now.component_cells, n, mask), now.points, now.cells, now.point_component,
                                now.cell_component, now.component_cells, offset=0, normals=now.normals, cell_pixels=now.cell_pixels)
            kept.append(now)
            args.append((rule, n, mask))
    return kept, args


def cell_pixels_view(recipe, vox):
    """(frame, inside) of cell_pixels_ref's view constructors: the frame BEFORE the band mapping -- with a band the caller's raw
    volume --, the ring's constant where the ring is inside."""
    import cell_pixels_ref as cp
    kind, iso = recipe["kind"], recipe["iso"]
    iso = iso if vox.dtype.kind == "f" else int(iso)
    if kind == "border":
        c = recipe["border"]["value"]
        return cp.border(vox, float(c) if vox.dtype.kind == "f" else int(c), iso)
    if kind == "region":
        return cp.region(vox, recipe["region"]["start"], recipe["region"]["size"], iso)
    if kind == "band":
        b = recipe["band"]
        return cp.band(vox, _num(b["lower"]), _num(b["upper"]), _num(b["inside"]), _num(b["outside"]), iso)
    return cp.whole(vox, iso)


def _bspline_expected(oracle, recipe, img, start):
    """The oracle's lattice points and cells (the sweep does not depend on the interpolator), every point walked by the
    drop-in's host walk through ITK's own class (bspline_ref.walk_exe(), mode `walk`: needs no GPU)."""
    import bspline_ref
    kw = recipe["kw"]
    if not kw["project"]:
        return oracle.run(img, recipe["iso"], index_start=start, **_oracle_kw(recipe))
    # (quads: the triangles are cut along the shorter diagonal of the WALKED quad, txx:295-307 -- ref_filter.split_quads below)
    flat = oracle.run(img, recipe["iso"], index_start=start, **dict(_oracle_kw(recipe), project=False, triangles=False))
    flat.info = None                                   # (the host walk keeps no counters)
    if not len(flat.points):
        flat.cells = flat.cells.reshape(0, 3 if kw["triangles"] else 4)
        return flat
    nz, ny, nx = img.shape
    with tempfile.TemporaryDirectory() as tmp:
        raw, sp, op = (os.path.join(tmp, n) for n in ("v.raw", "s.raw", "o.raw"))
        img.tofile(raw)
        flat.points.astype("<f4").tofile(sp)
        g = _geo(recipe)
        r = subprocess.run([bspline_ref.walk_exe(), "walk", raw, bspline_ref.PIXEL_NAMES[img.dtype], str(nx), str(ny), str(nz),
                            str(recipe["bspline"]["bits"]), bspline_ref.geometry_arg(g["spacing"], g["origin"], g["direction"], start),
                            repr(float(recipe["iso"])), repr(kw["threshold"]), repr(kw["step"]), repr(kw["relax"]), str(kw["max_steps"]),
                            sp, str(len(flat.points)), op], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout, r.stderr)
        flat.points = np.fromfile(op, dtype="<f4").reshape(-1, 3)
    if kw["triangles"]:
        from ref_filter import split_quads
        flat.cells = np.ascontiguousarray(split_quads(flat.points, flat.cells)).astype(np.uint64)
    return flat


# ---- 3. the library --------------------------------------------------------------------------------------------------------
def open_contexts(pkg):
    return {"ex": pkg.Extractor(0), "held": pkg.Extractor(0)}


def close_contexts(contexts):
    for name in ("ex", "held"):
        contexts[name].close()


# what the message of each refusal says (the code alone would not tell it from another reason to refuse)
REFUSAL_TEXT = {"pair": "together with", "stream": "cuberille_extract_stream", "variant": "default projection branch only",
                "held": "holding a gradient", "rg": "central-difference gradient only", "normals_rg": "point normals",
                "bspline_variant": "B-spline interpolator walks the default projection branch",
                "bspline_held": "B-spline interpolator is not offered on a context holding a gradient",
                "cell_pixels_slab": "cell pixels", "components_slab": "components"}


def _refused(pkg, ex, recipe, vox, desc, normals_on=False):
    """One call the header lists as refused, with this case's volume: CUBERILLE_ERR_ARGUMENT with the text of THAT refusal, and
    the context as it was.  The normals setting is not touched (switching it off would free the row a case before left), so
    with it on the recursive-Gaussian gradient is refused for the normals' sake first."""
    A = pkg._abi
    name, kind = recipe["refusal"], recipe["kind"]
    kw = dict(recipe["kw"], project=name != "normals_rg", variant=0)     # (normals_rg: without the walk the lines may be short)
    kw.pop("gradient", None)
    text = "point normals" if name == "rg" and normals_on else REFUSAL_TEXT[name]
    vol = pkg.Volume(vox, spacing=tuple(recipe["spacing"]), origin=tuple(recipe["origin"]), direction=np.asarray(recipe["direction"]),
                     index_start=tuple(recipe["index_start"]))
    iso = recipe["iso"]
    try:
        if kind in ("border", "region", "band"):
            _set_view(ex, recipe)
        if name == "pair":            # a second view beside the case's own
            if kind == "border":
                ex.set_band(iso, iso, 1, 0) if np.dtype(recipe["dtype"]).kind != "f" else ex.set_band(0.0, 1.0, 1.0, 0.0)
            else:
                ex.set_border(1, 0)
            call = lambda: ex.extract_host(vol, pkg.make_params(iso, **kw))                      # noqa: E731
        elif name == "stream":
            call = lambda: ex.extract_stream(desc, lambda dst, z0, z1: dst.__setitem__(Ellipsis, vox[z0:z1]), pkg.make_params(iso, **kw))  # noqa: E731
        elif name in ("variant", "bspline_variant"):
            if name == "bspline_variant":
                ex.set_interpolator(A.INTERP_BSPLINE, 3, 32, 32)
            call = lambda: ex.extract_host(vol, pkg.make_params(iso, **dict(kw, variant=1 + recipe["case"] % 2)))   # noqa: E731
        elif name in ("held", "bspline_held"):
            if name == "bspline_held":
                ex.set_interpolator(A.INTERP_BSPLINE, 3, 64, 64)
            ex.hold_gradient(True)
            call = lambda: ex.extract_host(vol, pkg.make_params(iso, **kw))                      # noqa: E731
        elif name == "rg":
            call = lambda: ex.extract_host(vol, pkg.make_params(iso, **dict(kw, gradient=1)))    # noqa: E731
        elif name == "normals_rg":
            ex.set_point_normals(True)
            call = lambda: ex.extract_host(vol, pkg.make_params(iso, **dict(kw, gradient=1)))    # noqa: E731
        else:
            raise ValueError(name)
        try:
            call()
        except A.CuberilleError as e:
            assert e.code == A.ERR_ARGUMENT, "refusal %s: code %d (%s), not CUBERILLE_ERR_ARGUMENT" % (name, e.code, e)
            assert text in str(e), "refusal %s: refused for another reason: %s" % (name, e)
        else:
            raise AssertionError("refusal %s: the call was accepted" % name)
    finally:
        _clear_settings(pkg, ex)


def _refused_slab(pkg, ex, recipe, vox, on):
    """cell_pixels_slab / components_slab: with the setting on, cuberille_count of a slab that is not the whole volume --
    CUBERILLE_ERR_ARGUMENT, the message names the setting.  on: {"normals", "cell_pixels", "components"} -> whether a case
    before left that setting on; none of them is switched off here (that would free its row), and count_prepare asks them in
    this order, so the message names the first that is on.  A setting switched on for the call is switched off behind it."""
    import torch
    A = pkg._abi
    name = recipe["refusal_slab"]
    mine = SLAB_REFUSALS[name]
    nz, ny, nx = vox.shape
    kw = dict(recipe["kw"], variant=0)
    kw.pop("gradient", None)
    now = dict(on, **{mine: True})
    text = next(REFUSAL_TEXT[t] for k, t in (("normals", "normals_rg"), ("cell_pixels", "cell_pixels_slab"), ("components", "components_slab")) if now[k])
    desc = pkg.make_desc(vox.dtype, (nx, ny, nz), tuple(recipe["spacing"]), tuple(recipe["origin"]), np.asarray(recipe["direction"], dtype=np.float64),
                         tuple(recipe["index_start"]))
    dev = to_device(torch, vox)
    torch.cuda.synchronize()
    setter = ex.set_cell_pixels if mine == "cell_pixels" else ex.set_components
    setter(True)
    try:
        # the buffer's slices as the lower part of a volume one slice taller: consistent ranges, not the whole volume
        ex.count(dev.data_ptr(), desc, pkg.make_params(recipe["iso"], **kw), A.Slab(nz + 1, 0, 0, nz, 0, 0))
    except A.CuberilleError as e:
        assert e.code == A.ERR_ARGUMENT, "refusal %s: code %d (%s), not CUBERILLE_ERR_ARGUMENT" % (name, e.code, e)
        assert text in str(e), "refusal %s: refused for another reason: %s" % (name, e)
    else:
        raise AssertionError("refusal %s: the call was accepted" % name)
    finally:
        if not on[mine]:
            setter(False)


def _set_view(ex, recipe):
    kind = recipe["kind"]
    if kind == "border":
        ex.set_border(1, _num(recipe["border"]["value"]))
    elif kind == "region":
        ex.set_region(recipe["region"]["start"], recipe["region"]["size"])
    elif kind == "band":
        b = recipe["band"]
        ex.set_band(_num(b["lower"]), _num(b["upper"]), _num(b["inside"]), _num(b["outside"]))


def _clear_settings(pkg, ex):
    ex.set_border(0, 0)
    ex.clear_region()
    ex.clear_band()
    ex.hold_gradient(False)
    ex.set_interpolator(pkg._abi.INTERP_LINEAR)
    # (cuberille_set_point_normals, cuberille_set_cell_pixels and cuberille_set_components are the case's to set: off would free
    #  the rows)
    ex.debug_option("defaults", 0)


def _keep(pkg, ex, rule, n, mask):
    """ex.keep_components -- but a mask that holds bytes other than 0 and 1 goes to the C ABI as it is (the Python wrapper hands
    the library `mask != 0`: through it the library would never see such a byte), and ex.result is renewed the way the wrapper
    renews it."""
    if mask is None or not (np.asarray(mask) > 1).any():
        return ex.keep_components(rule, n, mask)
    import ctypes as C
    A = pkg._abi
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    npnt, ncell, k, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float()
    A.check(ex._ctx, A.lib().cuberille_keep_components(ex._ctx, A.KEEP_MASK, 0, C.c_void_p(m.ctypes.data), int(m.size), C.byref(npnt),
                                                       C.byref(ncell), C.byref(k), C.byref(ms)))
    res = type(ex.result).from_buffer_copy(ex.result)
    res.n_points, res.n_cells = npnt.value, ncell.value
    ex.result = res
    return int(npnt.value), int(ncell.value), int(k.value), float(ms.value)


def _keep_stage(pkg, ex, recipe, args):
    """One cuberille_keep_components on the context and everything the library then says of its mesh."""
    before = {k: int(getattr(ex.result, k)) for k in COUNTERS}
    k_before = ex.n_components()
    returned = _keep(pkg, ex, *args)
    if recipe["route"] == "device":
        host = ex.mesh_host()                              # (taken before the keep too: it must be fetched again)
        mesh = pkg.Mesh(host.points.copy(), host.cells.copy())
    else:
        mesh = ex.download()
    return {"returned": tuple(returned[:3]), "ms": returned[3], "result": (int(ex.result.n_points), int(ex.result.n_cells)), "mesh": mesh,
            "normals": ex.download_normals() if recipe.get("normals") else None,
            "cell_pixels": ex.download_cell_pixels() if recipe.get("cell_pixels") else None,
            "components": ex.download_components(), "n_components": ex.n_components(),
            "null": tuple(p is None or p == 0 for p in ex.components_device()),
            "counters_before": before, "counters": {k: int(getattr(ex.result, k)) for k in COUNTERS}, "k_before": k_before}


def moved_by_keep(stages):
    """Whether a stage of a case's keeps kept some but not all -- 0 < K' < K: the mesh's rows then changed places with spare rows
    sized by the kept counts, and the context is left that way.  stages: (K before, K') per stage."""
    return any(0 < int(k2) < int(k) for k, k2 in stages)


def run_case(pkg, contexts, recipe, vox=None, stats=None, keeps=()):
    """keeps: the (rule, n, mask) of every stage of recipe["keep"], resolved on the REFERENCE's counts (expected()["keep_args"]);
    "kept": what _keep_stage recorded behind each; "keep_before": whether the case before on the context left it behind a keep
    that moved the rows (moved_by_keep).
    {"mesh", "normals" (or None), "counters" (or None), "cell_pixels" (or None), "components" (three rows, or None),
    "n_components", "first_mesh" / "first_counters" (a case that repeats: its first repeat, run with cell pixels and components
    off), "emit_offset", "row_before", "pixels_row_before", "components_row_before"} of the library for the recipe, on the
    contexts as the cases before left them (the settings a case makes are taken back behind it; the workspace, its sizes, its
    history and -- unless the recipe drops them -- the normals row of a normals case, the pixel row of a cell-pixel case and the
    rows of a components case stay).  row_before: the points of the mesh whose normals row the context still held when the case
    began, or None; pixels_row_before: (cells, bytes per pixel) of the mesh whose pixel row it held; components_row_before:
    (points, cells) of the mesh whose component rows it held."""
    import torch
    vox = voxels(recipe) if vox is None else vox
    dt = vox.dtype
    nz, ny, nx = vox.shape
    kind, route, kw, iso = recipe["kind"], recipe["route"], recipe["kw"], recipe["iso"]
    spacing, origin, direction, start = tuple(recipe["spacing"]), tuple(recipe["origin"]), np.asarray(recipe["direction"], dtype=np.float64), tuple(recipe["index_start"])
    ex = contexts["held"] if route == "held" else contexts["ex"]
    vol = pkg.Volume(vox, spacing=spacing, origin=origin, direction=direction, index_start=start)
    desc = pkg.make_desc(dt, (nx, ny, nz), spacing, origin, direction, start)
    prm = pkg.make_params(iso, **kw)
    held = route == "held"
    row_before = contexts.get("normals_row") if not held else None
    pixels_row_before = contexts.get("pixels_row") if not held else None
    components_row_before = contexts.get("components_row") if not held else None
    keep_before = bool(contexts.get("behind_keep")) if not held else False
    kept = []
    if recipe.get("refusal"):
        _refused(pkg, ex, recipe, vox, desc, row_before is not None)
    if recipe.get("refusal_slab"):
        # (the refusal normals_rg switches the normals on for its call and leaves them to the case, which sets them next)
        _refused_slab(pkg, ex, recipe, vox, {"normals": row_before is not None or recipe.get("refusal") == "normals_rg",
                                             "cell_pixels": pixels_row_before is not None,
                                             "components": components_row_before is not None})
    want_pixels, want_components = bool(recipe.get("cell_pixels")), bool(recipe.get("components"))
    repeat = int(recipe.get("repeat", 1))
    offset = int(recipe.get("emit_offset", 0))
    mesh = normals = counters = pixels = components = n_components = first_mesh = first_counters = None
    try:
        _set_view(ex, recipe)
        if kind == "bspline":
            ex.set_interpolator(pkg._abi.INTERP_BSPLINE, 3, recipe["bspline"]["bits"], recipe["bspline"]["bits"])
        if recipe.get("switch"):
            ex.debug_option(recipe["switch"][0], recipe["switch"][1])
        if recipe.get("chunk_kib"):
            ex.debug_option("upload_chunk_kib", recipe["chunk_kib"])
        ex.set_point_normals(bool(recipe.get("normals")))
        for rep in range(repeat):
            # a case that repeats runs its first repeat with the two settings OFF (which frees what rows there were): points,
            # cells and counters are the bytes of the same extraction with the setting off -- compare() holds them to that
            first_off = repeat > 1 and rep == 0
            ex.set_cell_pixels(want_pixels and not first_off)
            ex.set_components(want_components and not first_off)
            if rep == 1:
                first_mesh, first_counters = mesh, counters
            res = None
            if route in ("host", "host_chunked", "switch"):
                res = ex.extract_host(vol, prm)
                mesh = ex.download()
            elif route == "device":
                dev = to_device(torch, vox)
                torch.cuda.synchronize()
                res = ex.extract_device(dev.data_ptr(), desc, prm)
                mesh = ex.mesh_host()
                mesh = pkg.Mesh(mesh.points.copy(), mesh.cells.copy())
            elif route == "stream":
                def source(dst, z0, z1):
                    dst[...] = vox[z0:z1]
                res = ex.extract_stream(desc, source, prm)
                mesh = ex.download()
            elif route == "count_emit":
                dev = to_device(torch, vox)
                torch.cuda.synchronize()
                n_p, n_c = ex.count(dev.data_ptr(), desc, prm)
                res = ex.emit(offset)           # (with cell pixels on the emit reads the voxels: dev lives until here)
                mesh = ex.download()
                assert (n_p, n_c) == (mesh.points.shape[0], mesh.cells.shape[0])
            elif held:
                # quirk Q3: a first volume of its own (same pixel type), then this one along the first one's gradient
                f = recipe["first"]
                fvox = _field(f["field"])[0]
                ex.hold_gradient(False)
                ex.hold_gradient(True)
                ex.extract_host(pkg.Volume(fvox, spacing=tuple(f["spacing"]), origin=tuple(f["origin"]),
                                           direction=np.asarray(f["direction"], dtype=np.float64), index_start=tuple(f["index_start"])), prm)
                ex.extract_host(vol, prm)
                mesh = ex.download()
            else:   # slabs stitched by hand: counts, id offsets, concatenation; thin: 3 + 3 halo slices, escaped walks again
                thin = route == "thin_slabs"
                below, above = pkg.required_halo(desc, prm)
                cuts = recipe["cuts"]
                pts, cells, poff = [], [], 0
                tb, ta = pkg.cuberille.minimum_halo(desc, prm)
                for a, b in zip(cuts[:-1], cuts[1:]):
                    lo, hi = (max(a - tb - 1, 0), min(b + ta + 1, nz)) if thin else (max(a - below, 0), min(b + above, nz))
                    dev = to_device(torch, vox[lo:hi])
                    torch.cuda.synchronize()
                    sdesc = pkg.make_desc(dt, (nx, ny, hi - lo), spacing, origin, direction, start)
                    n_p, n_c = ex.count(dev.data_ptr(), sdesc, prm, pkg._abi.Slab(nz, lo, a, b, 0, pkg._abi.SLAB_THIN_HALO if thin else 0))
                    if thin:
                        ex.emit_points()
                        n_esc = ex.escaped_count()
                        if stats is not None:
                            stats["escaped_walks"] = stats.get("escaped_walks", 0) + int(n_esc)
                        if n_esc:
                            dlo, dhi = max(a - below, 0), min(b + above, nz)
                            deep = to_device(torch, vox[dlo:dhi])
                            torch.cuda.synchronize()
                            ex.reproject_escaped(deep.data_ptr(), dlo, dhi - dlo)
                    ex.emit(poff)
                    m = ex.download()
                    pts.append(m.points)
                    cells.append(m.cells)
                    poff += n_p
                mesh = pkg.Mesh(np.concatenate(pts), np.concatenate(cells))
            if res is not None:
                counters = {k: int(getattr(res, k)) for k in COUNTERS}
            if recipe.get("normals"):
                normals = ex.download_normals()
            if keeps and want_components and not first_off and rep + 1 < repeat:
                # every repeat that runs with components on keeps too: the next extraction is launched behind a keep
                for args in keeps:
                    _keep(pkg, ex, *args)
        # (after the last repeat)
        if want_pixels:
            pixels = ex.download_cell_pixels()
        if want_components:
            components = ex.download_components()
            n_components = ex.n_components()
        for args in keeps:
            kept.append(_keep_stage(pkg, ex, recipe, args))
    finally:
        _clear_settings(pkg, ex)
        if not held:
            contexts["normals_row"] = contexts["pixels_row"] = contexts["components_row"] = None
            contexts["behind_keep"] = False
    n_points, n_cells = int(mesh.points.shape[0]), int(mesh.cells.shape[0])
    rows = {"normals_row": row_after(recipe, n_points), "pixels_row": pixels_row_after(recipe, n_cells),
            "components_row": components_row_after(recipe, n_points, n_cells)}
    for name, setter in (("normals_row", ex.set_point_normals), ("pixels_row", ex.set_cell_pixels), ("components_row", ex.set_components)):
        if rows[name] is None:
            setter(False)
    if not held:
        contexts.update(rows)
        contexts["behind_keep"] = moved_by_keep([(g["k_before"], g["returned"][2]) for g in kept])
    return {"kept": kept, "keep_before": keep_before, "mesh": mesh, "normals": normals, "counters": counters, "cell_pixels": pixels, "components": components,
            "n_components": n_components, "first_mesh": first_mesh, "first_counters": first_counters, "emit_offset": offset, "row_before": row_before,
            "pixels_row_before": pixels_row_before, "components_row_before": components_row_before}


def row_after(recipe, n_points):
    """The points of the mesh whose normals row a case leaves on its context (None: no row -- no normals, or dropped)."""
    return n_points if recipe.get("normals") and not recipe.get("drop_normals_row") else None


def pixels_row_after(recipe, n_cells):
    """(cells, bytes per pixel) of the mesh whose cell-pixel row a case leaves on its context (None: no row)."""
    keep = recipe.get("cell_pixels") and not recipe.get("drop_cell_rows") and recipe["route"] != "held"
    return (int(n_cells), np.dtype(recipe["dtype"]).itemsize) if keep else None


def components_row_after(recipe, n_points, n_cells):
    """(points, cells) of the mesh whose component rows a case leaves on its context (None: no rows)."""
    keep = recipe.get("components") and not recipe.get("drop_cell_rows") and recipe["route"] != "held"
    return (int(n_points), int(n_cells)) if keep else None


def meets_pixels_row_of_another_size(row_before, recipe, n_cells):
    """A cell-pixel case on a context that still holds the row of a mesh of another cell count or pixel width.  (A case that
    repeats frees the row in its first repeat, which runs with the setting off: it meets none.)"""
    return bool(recipe.get("cell_pixels") and recipe.get("repeat", 1) == 1 and row_before is not None
                and tuple(row_before) != (int(n_cells), np.dtype(recipe["dtype"]).itemsize))


def meets_components_row_of_another_size(row_before, recipe, n_points, n_cells):
    """A components case on a context that still holds the rows of a mesh of other point or cell counts."""
    return bool(recipe.get("components") and recipe.get("repeat", 1) == 1 and row_before is not None
                and tuple(row_before) != (int(n_points), int(n_cells)))


def meets_row_of_another_size(row_before, recipe, n_points):
    """A normals case on a context that still holds the row of a mesh of another size."""
    return bool(recipe.get("normals")) and row_before is not None and row_before != n_points


def behind_keep(keep_before, rows_before, recipe):
    """The settings -- among "normals", "cell_pixels", "components" -- that the case has on, whose row the case before left on
    the context, that case having run a keep with 0 < K' < K: the row the case finds is one sized by the kept counts, its
    extraction-sized partner a spare row.  rows_before: (normals row, pixels row, components row) as the *_row_after functions
    gave them.  (A case that repeats switches cell pixels and components off in its first repeat: it meets the normals row only.)"""
    if not keep_before:
        return ()
    once = recipe.get("repeat", 1) == 1
    on = (bool(recipe.get("normals")), bool(recipe.get("cell_pixels")) and once, bool(recipe.get("components")) and once)
    return tuple(name for name, mine, row in zip(("normals", "cell_pixels", "components"), on, rows_before) if mine and row is not None)


def compare_kept(got, want, offset=0):
    """The stages of a case's keep, each exact: points and cells (the id offset taken off: every id is >= offset and below offset
    + kept points), normals, cell pixels and the three rows as bytes, the returned counts, ex.result's counts and K the
    reference's, the device pointers null exactly where a count is 0, the walk's counters those before the keep, the
    definition's properties on the kept rows."""
    import normals_ref
    import test_components as cases
    stages, kept = got.get("kept") or [], want.get("kept") or []
    assert len(stages) == len(kept), "%d keep stages ran, the recipe holds %d" % (len(stages), len(kept))
    for i, (g, w) in enumerate(zip(stages, kept)):
        what = "keep stage %d" % i
        n_points, n_cells, k = len(w.points), len(w.cells), len(w.component_cells)
        mesh = copy.copy(g["mesh"])
        if len(mesh.cells):
            assert int(mesh.cells.min()) >= offset and int(mesh.cells.max()) < offset + n_points, \
                (what, "a kept cell id outside [offset, offset + kept points)", int(mesh.cells.min()), int(mesh.cells.max()), offset, n_points)
        mesh.cells = mesh.cells - np.uint64(offset)
        try:
            assert_same_mesh(mesh, w)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (what, e)) from e
        assert tuple(g["returned"]) == (n_points, n_cells, k), (what, "returned counts", g["returned"], (n_points, n_cells, k))
        assert tuple(g["result"]) == (n_points, n_cells), (what, "result counts", g["result"], (n_points, n_cells))
        assert g["n_components"] == k, (what, "K", g["n_components"], k)
        if w.normals is not None:
            assert g["normals"] is not None, (what, "no normals came back")
            normals_ref.same_normals(g["normals"], w.normals, what + ": normals")
        if w.cell_pixels is not None:
            p = g["cell_pixels"]
            assert p is not None, (what, "no cell pixels came back")
            assert p.dtype == w.cell_pixels.dtype and p.shape == w.cell_pixels.shape and p.tobytes() == w.cell_pixels.tobytes(), (what, "cell pixels")
        rows = (w.point_component, w.cell_component, w.component_cells)
        cases.same(g["components"], rows, what + ": components")
        assert tuple(g["null"]) == (n_points == 0, n_cells == 0, k == 0), (what, "null device pointers", g["null"], (n_points, n_cells, k))
        assert g["counters"] == g["counters_before"], (what, "counters changed by the keep", g["counters_before"], g["counters"])
        cases.check_properties(w.cells, n_points, g["components"], what + ": components")


def compare(got, want):
    """The first difference as an AssertionError: mesh (the id offset of a count + emit taken off its cells; the first repeat's
    mesh, extracted with cell pixels and components off, byte for byte the last one's), then counters, normals, cell pixels
    (as bytes: a NaN's payload and the sign of a zero count), components (three rows as bytes, K, the definition's properties)."""
    import normals_ref
    mesh, offset = got["mesh"], int(got.get("emit_offset") or 0)
    if offset:
        if len(mesh.cells):
            assert int(mesh.cells.min()) >= offset, ("a cell id below the id offset", int(mesh.cells.min()), offset)
        mesh = copy.copy(mesh)
        mesh.cells = mesh.cells - np.uint64(offset)
    assert_same_mesh(mesh, want["mesh"])
    first = got.get("first_mesh")
    if first is not None:
        for name in ("points", "cells"):
            a, b = getattr(first, name), getattr(got["mesh"], name)
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), \
                "%s with cell pixels and components off differ from those with the settings on" % name
    info = getattr(want["mesh"], "info", None)
    if got["counters"] is not None and info is not None:
        assert got["counters"] == {k: info[k] for k in COUNTERS}, ("counters", got["counters"], {k: info[k] for k in COUNTERS})
    if first is not None:
        assert got.get("first_counters") == got["counters"], ("counters with cell pixels and components off", got.get("first_counters"), got["counters"])
    if want["normals"] is not None:
        assert got["normals"] is not None, "no normals came back"
        normals_ref.same_normals(got["normals"], want["normals"], "normals")
    if want.get("cell_pixels") is not None:
        g, w = got.get("cell_pixels"), want["cell_pixels"]
        assert g is not None, "no cell pixels came back"
        assert g.dtype == w.dtype and g.shape == w.shape == (len(want["mesh"].cells),), ("cell pixels", g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            at = int(np.argmax((g.view(np.uint8) != w.view(np.uint8)).reshape(len(g), -1).any(axis=1)))
            raise AssertionError("cell pixels: first difference at cell %d: %r, reference %r" % (at, g[at], w[at]))
    if want.get("components") is not None:
        import test_components as cases
        g, w = got.get("components"), want["components"]
        assert g is not None, "no components came back"
        cases.same(g, w, "components")
        assert got.get("n_components") == len(w[2]), ("K", got.get("n_components"), len(w[2]))
        cases.check_properties(want["mesh"].cells, len(want["mesh"].points), g, "components")
    compare_kept(got, want, offset)


def tally(stats, recipe, got, want):
    mesh = got["mesh"]
    stats["cases"] += 1
    stats["points"] += int(mesh.points.shape[0])
    stats["cells"] += int(mesh.cells.shape[0])
    stats["nan_points"] += int(np.isnan(mesh.points).any(axis=1).sum()) if mesh.points.size else 0
    for key, val in (("routes", recipe["route"]), ("dtypes", recipe["dtype"]), ("kinds", recipe["kind"])):
        stats[key][val] = stats[key].get(val, 0) + 1
    stats["with_normals"] += int(bool(recipe.get("normals")))
    stats["normals_on_a_row_of_another_size"] += int(meets_row_of_another_size(got.get("row_before"), recipe, int(mesh.points.shape[0])))
    stats["nan_normals"] += int(np.isnan(want["normals"]).any(axis=1).sum()) if want["normals"] is not None and want["normals"].size else 0
    stats["repeats"] += int(recipe.get("repeat", 1) > 1)
    stats["after_refusal"] += int(bool(recipe.get("refusal")) or bool(recipe.get("refusal_slab")))
    stats["with_switch"] += int(bool(recipe.get("switch")) or bool(recipe.get("chunk_kib")))
    for name in (recipe.get("refusal"), recipe.get("refusal_slab")):
        if name:
            key = "%s:%s" % (recipe["kind"], name)
            stats["refusals"][key] = stats["refusals"].get(key, 0) + 1
    n_points, n_cells = int(mesh.points.shape[0]), int(mesh.cells.shape[0])
    pix, comp = bool(recipe.get("cell_pixels")), bool(recipe.get("components"))
    stats["with_cell_pixels"] += int(pix)
    stats["with_components"] += int(comp)
    stats["with_normals_cell_pixels_and_components"] += int(pix and comp and bool(recipe.get("normals")))
    if comp:
        stats["components_found"] += len(want["components"][2])
        stats["with_two_components_or_more"] += int(len(want["components"][2]) >= 2)
    stats["cell_pixels_on_a_row_of_another_size"] += int(meets_pixels_row_of_another_size(got.get("pixels_row_before"), recipe, n_cells))
    stats["components_on_rows_of_another_size"] += int(meets_components_row_of_another_size(got.get("components_row_before"), recipe, n_points, n_cells))
    stats["nonzero_id_offsets"] += int(bool(recipe.get("emit_offset")))
    if recipe.get("keep"):
        ks = [len(want["components"][2])] + [len(w.component_cells) for w in want["kept"]]
        stats["keeps"][recipe["keep"]["rule"]] = stats["keeps"].get(recipe["keep"]["rule"], 0) + 1
        stats["keeps_that_dropped"] += int(any(b < a for a, b in zip(ks, ks[1:])))
        stats["keeps_some_of_several"] += int(moved_by_keep(list(zip(ks, ks[1:]))))
        stats["keeps_to_nothing"] += int(ks[0] > 0 and ks[-1] == 0)
        stats["chained_keeps"] += int(len(ks) > 2)
        stats["keeps_on_mask_bytes_other_than_0_and_1"] += int(any(m is not None and (m > 1).any() for _, _, m in want["keep_args"]))
    stats["behind_keep"] += int(bool(behind_keep(got.get("keep_before"), (got.get("row_before"), got.get("pixels_row_before"),
                                                                          got.get("components_row_before")), recipe)))


def new_stats():
    return {"cases": 0, "points": 0, "cells": 0, "routes": {}, "dtypes": {}, "kinds": {}, "with_normals": 0, "normals_on_a_row_of_another_size": 0, "nan_normals": 0, "repeats": 0,
            "after_refusal": 0, "refusals": {}, "with_switch": 0, "refused_slab_alias": 0, "nan_points": 0,
            "with_cell_pixels": 0, "with_components": 0, "with_normals_cell_pixels_and_components": 0, "components_found": 0,
            "with_two_components_or_more": 0, "cell_pixels_on_a_row_of_another_size": 0, "components_on_rows_of_another_size": 0,
            "nonzero_id_offsets": 0, "keeps": {}, "keeps_that_dropped": 0, "keeps_some_of_several": 0, "keeps_to_nothing": 0,
            "chained_keeps": 0, "keeps_on_mask_bytes_other_than_0_and_1": 0, "behind_keep": 0}


def one_case(pkg, oracle, contexts, recipe, stats=None):
    """Run and compare one recipe; returns (got, want).  Raises at the first difference."""
    vox = voxels(recipe)
    want = expected(oracle, recipe, vox)
    got = run_case(pkg, contexts, recipe, vox, stats, want["keep_args"])
    compare(got, want)
    return got, want


# ---- the seeded slice of the GPU suite (tests/test_gpu_campaign.py; its conditions: tests/test_campaign_scripts.py) ------------
# kind: (seed, number of cases).  Case i of a kind takes pixel type DTYPES[i % 10] and the kind's routes in turn; everything else
# is drawn.  The seeds are the first for which the oracle alone shows every condition of slice_conditions().
SLICE_OPTIONS = dict(max_rows=12, max_voxels=30000)
SLICE = {"whole": (54, 24), "border": (4, 20), "region": (1, 20), "band": (1, 20), "bspline": (5, 20)}


def slice_recipes(kind, seed=None, n=None):
    """Cell pixels and components are fixed by a RULE OF THE CASE NUMBER i, not by a seed: cell pixels on where
    (i + i // 10) % 2 == 0 -- the pixel type is DTYPES[i % 10], so the parity alternates from one decade to the next and all ten
    types take it --, components on where i % 3 != 2 -- the empty meshes of the region and band slices (cases 10; 1 and 16) are
    among them -- and both on every route that offers them.  Everything else of the second stream (the rows kept or dropped,
    the id offset, a refused slab) is drawn.  Every components case keeps (recipe["keep"]), by the rule
    KEEP_RULES[(i // 2) % 3]; the pick, the mask and a second stage are drawn from the third stream."""
    seed = SLICE[kind][0] if seed is None else seed
    n = SLICE[kind][1] if n is None else n
    return [draw_case(seed, i, dict(SLICE_OPTIONS, kind=kind, dtype=np.dtype(DTYPES[i % len(DTYPES)]).name,
                                    route=ROUTES[kind][i % len(ROUTES[kind])], cell_pixels=(i + i // 10) % 2 == 0,
                                    components=i % 3 != 2, keep=KEEP_RULES[(i // 2) % 3])) for i in range(n)]


# the envelope's slice: every kind and route in turn, a float type in two cases of three, nothing but the mesh (and the normals
# the first stream draws) compared
ENVELOPE_SLICE = (2, 60)        # (the first seed for which the oracle alone shows every condition of envelope_slice_conditions())


def envelope_slice_recipes(seed=None, n=None):
    seed = ENVELOPE_SLICE[0] if seed is None else seed
    n = ENVELOPE_SLICE[1] if n is None else n
    out = []
    for i in range(n):
        kind = KINDS[i % len(KINDS)]
        dtype = ("float32", "float64")[(i // 3) % 2] if i % 3 else np.dtype(DTYPES[i % len(DTYPES)]).name
        out.append(draw_case(seed, i, dict(SLICE_OPTIONS, kind=kind, dtype=dtype, route=ROUTES[kind][(i // len(KINDS)) % len(ROUTES[kind])],
                                           cell_pixels=False, components=False, keep=False, envelope=True)))
    return out


def envelope_slice_conditions(recipes, wants):
    """What the envelope's slice must show, from the recipes and the references alone, as the list of what is missing."""
    missing = []
    def need(ok, what):
        if not ok:
            missing.append(what)
    env = [r["envelope"] for r in recipes]
    need({r["kind"] for r in recipes} == set(KINDS), "every kind")
    for dt, (lo, hi) in ENVELOPE_VOXEL_EXP.items():
        mine = [e["voxel_exp"] for r, e in zip(recipes, env) if r["dtype"] == dt]
        need(mine and min(mine) < lo // 2 and max(mine) > hi // 2, "%s voxel scales in the lower and in the upper quarter of the exponents" % dt)
    need(min(e["spacing_exp"] for e in env) < -50 and max(e["spacing_exp"] for e in env) > 50, "spacing scales below 2^-50 and above 2^50")
    need(max(max(abs(v) for v in e["origin"]) for e in env) > 1e8, "an origin beyond 1e8")
    need(sum(e["start"] is not None for e in env) >= 3, "three start indices near +-2^30")
    need(all(linesearch_defined(voxels(r), r["iso"]) for r in recipes if r["kw"]["variant"] == 2), "every line-search case under the 10000 rule")
    need(any(r["kw"]["variant"] == 2 and r["kw"]["project"] for r in recipes), "a line-search case")
    walked = [w["mesh"].points for r, w in zip(recipes, wants) if r["kw"]["project"] and r["kw"]["max_steps"] > 0 and len(w["mesh"].points)]
    need(sum(bool(np.isfinite(p).all()) for p in walked) >= 5, "five walked meshes that stay finite")
    need(sum(bool(np.isnan(p).any()) for p in walked) >= 5, "five walked meshes with NaN coordinates")
    need(4 * sum(len(w["mesh"].points) == 0 for w in wants) <= len(wants), "at most a quarter of the cases with an empty reference mesh")
    return missing


def slice_facts(recipe, want, row_before=None, pixels_row_before=None, components_row_before=None, keep_before=False):
    """What one executed case of the slice contributes to the conditions, from the recipe and the reference alone.  row_before,
    pixels_row_before, components_row_before: what row_after(), pixels_row_after(), components_row_after() gave for the case
    before it on the context, keep_before: whether that case ran a keep that kept some of several (slice_sequence_facts follows
    them through a kind's cases).  keep: None, or the keep's facts -- its rule, `ks` (K before and behind every stage), whether
    the kept part of any stage holds a NaN coordinate or normal, whether a mask holds a byte other than 0 and 1."""
    keep = None
    if recipe.get("keep"):
        ks = [len(want["components"][2])] + [len(w.component_cells) for w in want["kept"]]
        keep = dict(rule=recipe["keep"]["rule"], ks=ks, chained=len(ks) > 2, some=moved_by_keep(list(zip(ks, ks[1:]))),
                    first_some=0 < ks[1] < ks[0],
                    nan=any(bool(np.isnan(w.points).any()) or (w.normals is not None and bool(np.isnan(w.normals).any())) for w in want["kept"]),
                    odd_mask=any(m is not None and bool((m > 1).any()) for _, _, m in want["keep_args"]))
    img, _ = frame(recipe)
    pts, nrm = want["mesh"].points, want["normals"]
    n_cells = len(want["mesh"].cells)
    pix, comp = want.get("cell_pixels"), want.get("components")
    return dict(walks=bool(recipe["kw"]["project"]) and recipe["kw"]["max_steps"] > 0 and len(pts) > 0,
                other_row=meets_row_of_another_size(row_before, recipe, len(pts)),
                cell_pixels=pix is not None, components=comp is not None, K=len(comp[2]) if comp is not None else None,
                offset=int(recipe.get("emit_offset", 0)), switch=bool(recipe.get("switch")),
                # a border case with cell pixels whose constant is not below the iso value: the ring is inside
                ring_inside=pix is not None and recipe["kind"] == "border" and bool(cell_pixels_view(recipe, voxels(recipe))[1][0, 0, 0]),
                # a band case with cell pixels whose cells carry at least two distinct raw pixels
                raw_values=pix is not None and recipe["kind"] == "band" and len(pix) > 0
                and len(np.unique(pix.view(np.uint8).reshape(len(pix), -1), axis=0)) >= 2,
                other_pixels_row=meets_pixels_row_of_another_size(pixels_row_before, recipe, n_cells),
                other_components_row=meets_components_row_of_another_size(components_row_before, recipe, len(pts), n_cells),
                kind=recipe["kind"], dtype=recipe["dtype"], route=recipe["route"], triangles=bool(recipe["kw"]["triangles"]),
                project=bool(recipe["kw"]["project"]), form=geometry_form(recipe), moved=any(int(v) for v in recipe["index_start"]),
                q1=bool(has_q1_gap(img, recipe["iso"])), empty=len(pts) == 0, nan_points=bool(np.isnan(pts).any()),
                normals=nrm is not None and len(nrm) > 0, nan_normals=nrm is not None and bool(np.isnan(nrm).any()),
                repeat=recipe.get("repeat", 1) > 1, refusal=recipe.get("refusal"),
                refused=bool(recipe.get("refusal") or recipe.get("refusal_slab")), keep=keep,
                behind_keep=behind_keep(keep_before, (row_before, pixels_row_before, components_row_before), recipe))


def slice_sequence_facts(recipes, wants):
    """slice_facts of a kind's cases in the order they run on their one context."""
    facts, rows = [], (None, None, None, False)
    for recipe, want in zip(recipes, wants):
        held = recipe["route"] == "held"                      # (a context of its own, never with normals, its rows always dropped)
        facts.append(slice_facts(recipe, want, *((None, None, None, False) if held else rows)))
        if not held:
            n_points, n_cells = len(want["mesh"].points), len(want["mesh"].cells)
            keep = facts[-1]["keep"]
            rows = (row_after(recipe, n_points), pixels_row_after(recipe, n_cells), components_row_after(recipe, n_points, n_cells),
                    bool(keep and keep["some"]))
    return facts


def slice_conditions(kind, facts):
    """The conditions a kind's slice must meet, as a list of those it misses (empty: all hold)."""
    missing = []
    def need(ok, what):
        if not ok:
            missing.append("%s: %s" % (kind, what))
    need(all(f["kind"] == kind for f in facts), "a case of another kind")
    need({f["dtype"] for f in facts} == {np.dtype(d).name for d in DTYPES}, "all ten pixel types")
    for r in ROUTES[kind]:
        need(sum(f["route"] == r for f in facts) >= 2, "route %s at least twice" % r)
    need({f["triangles"] for f in facts} == {True, False}, "quads and triangles")
    need({f["project"] for f in facts} == {True, False}, "projection on and off")
    # (the form is the walk kernel's: it exists where vertices are projected with at least one step)
    need({f["form"] for f in facts if f["walks"]} == {"identity", "axis-aligned", "general"}, "the three geometry forms, each on a case that walks")
    need(any(f["moved"] for f in facts), "a start index other than 0")
    need(any(f["q1"] and not f["empty"] for f in facts), "an empty slice between occupied ones (quirk Q1)")
    if kind in ("border", "region", "band"):
        need(any(f["refusal"] for f in facts), "a case behind a refused call")
    need(4 * sum(f["empty"] for f in facts) <= len(facts), "at most a quarter of the cases with an empty reference mesh")
    for key, name in (("cell_pixels", "cell pixels"), ("components", "components")):
        mine = [f for f in facts if f[key]]
        need(len(mine) >= 5, "at least 5 cases with %s" % name)
        need({f["triangles"] for f in mine} == {True, False}, "quads and triangles with %s" % name)
        need(4 * sum(f["empty"] for f in mine) <= len(mine), "at most a quarter of the cases with %s with an empty reference mesh" % name)
    if kind != "bspline":
        need(any(f["components"] and f["K"] == 1 for f in facts), "a components case with K = 1")
        need(any(f["components"] and f["K"] >= 2 for f in facts), "a components case with K >= 2")
    need(any(f["cell_pixels"] and f["components"] for f in facts), "a case with cell pixels and components")
    keeps = [f for f in facts if f["keep"]]
    need(len(keeps) >= 5, "at least 5 keep cases")
    need({f["triangles"] for f in keeps} == {True, False}, "quads and triangles among the keep cases")
    need(sum(f["keep"]["first_some"] for f in keeps) >= 4, "at least 4 keep cases with 0 < K' < K")
    return missing


def slice_conditions_overall(facts):
    """... and those of the whole slice (facts: of every kind together)."""
    missing = []
    def need(ok, what):
        if not ok:
            missing.append(what)
    need(any(f["nan_points"] for f in facts), "a case with NaN coordinates in the reference mesh")
    need(any(f["normals"] and f["nan_normals"] for f in facts), "a normals case with a NaN normal")
    need(any(f["normals"] and not f["nan_normals"] for f in facts), "a normals case without a NaN normal")
    need(any(f["repeat"] for f in facts), "a repeat case")
    need(any(f["repeat"] and f["normals"] for f in facts), "a repeat case with normals")
    need(any(f["other_row"] for f in facts), "a normals case on a context whose previous case left a normals row of another size")
    need({f["kind"] for f in facts} == set(KINDS), "the cases of every kind")
    for k in ("border", "region", "band"):
        need(any(f["kind"] == k and f["refusal"] for f in facts), "a refusal case of kind %s" % k)
    pix, comp = [f for f in facts if f["cell_pixels"]], [f for f in facts if f["components"]]
    need({f["dtype"] for f in pix} == {np.dtype(d).name for d in DTYPES}, "cell pixels of all ten pixel types")
    need(any(f["normals"] and f["cell_pixels"] and f["components"] for f in facts), "a case with normals, cell pixels and components together")
    need(any(f["empty"] and f["K"] == 0 for f in comp), "a components case with an empty mesh (K = 0, null rows)")
    need(any(f["q1"] and not f["empty"] for f in comp), "a components case on a mesh with a Q1 gap")
    need(any(f["K"] > 64 for f in comp), "a components case with K > 64")
    need(any(f["ring_inside"] for f in facts), "a border case with cell pixels whose ring is inside")
    need(any(f["raw_values"] for f in facts), "a band case whose cell pixels carry two distinct raw values")
    for mine, name in ((pix, "cell pixels"), (comp, "components")):
        need(any(f["repeat"] for f in mine), "a repeat case with %s" % name)
        need(any(f["refused"] for f in mine), "a case with %s behind a refused call" % name)
        need(any(f["switch"] for f in mine), "a case with %s under a development switch" % name)
    need(any(f["route"] == "count_emit" and f["offset"] > 0 for f in comp), "a count + emit components case with a non-zero id offset")
    need(any(f["route"] == "count_emit" and f["offset"] >= 2 ** 32 for f in comp), "a count + emit components case with an id offset of at least 2^32")
    need(any(f["other_pixels_row"] for f in facts), "a cell-pixel case on a context whose previous case left a row of another size")
    need(any(f["other_components_row"] for f in facts), "a components case on a context whose previous case left rows of another size")
    keeps = [f for f in facts if f["keep"]]
    first, last = (lambda f: f["keep"]["ks"][0]), (lambda f: f["keep"]["ks"][-1])
    dropped = lambda f: any(b < a for a, b in zip(f["keep"]["ks"], f["keep"]["ks"][1:]))        # noqa: E731
    for rule in KEEP_RULES:
        need(sum(f["keep"]["rule"] == rule and f["keep"]["first_some"] for f in keeps) >= 3, "the keep rule %s at least 3 times with 0 < K' < K" % rule)
    need(any(first(f) >= 1 and last(f) == 0 for f in keeps), "a keep with K' = 0 from K >= 1")
    need(any(first(f) >= 2 and f["keep"]["ks"][1] == first(f) for f in keeps), "a keep with K' = K >= 2 (nothing moves)")
    need(any(first(f) == 0 and f["empty"] for f in keeps), "a keep on an empty mesh (K = 0)")
    need(any(f["normals"] and not f["cell_pixels"] for f in keeps), "a keep with normals")
    need(any(f["cell_pixels"] and not f["normals"] for f in keeps), "a keep with cell pixels")
    need(any(f["normals"] and f["cell_pixels"] for f in keeps), "a keep with normals and cell pixels")
    need(any(f["keep"]["nan"] for f in keeps), "a keep with NaN coordinates or a NaN normal in the kept part")
    need(any(first(f) > 64 for f in keeps), "a keep at K > 64")
    need(any(f["route"] == "count_emit" and f["offset"] >= 2 ** 32 and dropped(f) for f in keeps),
         "a count + emit keep with an id offset of at least 2^32 that drops something")
    need(any(f["repeat"] for f in keeps), "a keep in a repeating case")
    need(any(f["route"] == "held" for f in keeps), "a keep on the held route")
    need(any(f["switch"] for f in keeps), "a keep under a development switch")
    need(any(f["refused"] for f in keeps), "a keep behind a refused call")
    need(any(f["keep"]["chained"] for f in keeps), "a chained keep")
    need(any(f["keep"]["odd_mask"] for f in keeps), "a keep whose mask holds a byte other than 0 and 1")
    for name, text in (("normals", "normals"), ("cell_pixels", "cell pixels"), ("components", "components")):
        need(any(name in f["behind_keep"] for f in facts), "a case with %s behind a keep (behind_keep)" % text)
    return missing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-voxels", type=int, default=900000)
    ap.add_argument("--recursive-gaussian", action="store_true", help="every case that can takes the recursive-Gaussian gradient (h:21)")
    ap.add_argument("--cell-pixels", action="store_true", help="every case that can takes cuberille_set_cell_pixels")
    ap.add_argument("--components", action="store_true", help="every case that can takes cuberille_set_components")
    ap.add_argument("--keep", action="store_true", help="every case with components takes a cuberille_keep_components behind it")
    ap.add_argument("--envelope", action="store_true", help="the edges of the number range: voxel scales of 2^-120 .. 2^126 (float32) and 2^-1000 .. 2^1000 (float64), spacing scales of 2^-100 .. 2^100, "
                    "origins up to 1e9, start indices near +-2^30")
    ap.add_argument("--big", action="store_true", help="up to 120 rows and slices (fewer, larger cases: set --max-voxels too)")
    ap.add_argument("--kind", choices=KINDS, default=None, help="draw this kind only")
    ap.add_argument("--dtype", default=None, help="draw this pixel type only (a numpy name)")
    ap.add_argument("--route", default=None, help="draw this route only (with --kind)")
    ap.add_argument("--max-rows", type=int, default=None, help="rows and slices up to this many (default 40, 120 with --big)")
    ap.add_argument("--case", type=int, default=None, help="run this one case of --seed (with the options the run had) and print the first difference")
    ap.add_argument("--replay", default=None, help="run one recipe: its JSON, or a file that holds it (a FAILED line is accepted as it is)")
    args = ap.parse_args()
    options = dict(max_voxels=args.max_voxels, big=args.big, recursive_gaussian=args.recursive_gaussian, kind=args.kind,
                   dtype=args.dtype, route=args.route, max_rows=args.max_rows, cell_pixels=args.cell_pixels or None,
                   components=args.components or None, keep=args.keep or None, envelope=args.envelope)
    pkg = graft.load_package()
    oracle = graft.load_oracle()
    oracle.build()
    contexts = open_contexts(pkg)
    try:
        if args.replay is not None or args.case is not None:
            if args.replay is not None:
                text = open(args.replay).read() if os.path.exists(args.replay) else args.replay
                recipe = json.loads(text)
                recipe = recipe.get("FAILED", recipe)
            else:
                recipe = draw_case(args.seed, args.case, options)
            print(json.dumps({"recipe": recipe}), flush=True)
            try:
                got, _ = one_case(pkg, oracle, contexts, recipe)
            except Exception as e:  # noqa: BLE001
                print(json.dumps({"FAILED": recipe, "error": "%s: %s" % (type(e).__name__, str(e)[:400])}), flush=True)
                return 1
            print(json.dumps({"identical": True, "points": int(got["mesh"].points.shape[0]), "cells": int(got["mesh"].cells.shape[0])}), flush=True)
            return 0
        t0 = last = time.time()
        stats = new_stats()
        case = -1
        while time.time() - t0 < args.seconds:
            case += 1
            recipe = draw_case(args.seed, case, options)
            try:
                got, want = one_case(pkg, oracle, contexts, recipe, stats)
            except Exception as e:  # noqa: BLE001
                print(json.dumps({"FAILED": recipe, "error": "%s: %s" % (type(e).__name__, str(e)[:400])}), flush=True)
                return 1
            tally(stats, recipe, got, want)
            if time.time() - last > 20:
                last = time.time()
                print("t %.0f s: %d cases, %d points, %d cells, %d with cell pixels (%d on a row of another size), %d with components "
                      "(%d on rows of another size, %d components, %d cases with two or more), %d with normals and both, %d id offsets, "
                      "keeps %s (%d dropped, %d to nothing, %d chained, %d cases behind one), "
                      "all identical" % (last - t0, stats["cases"], stats["points"], stats["cells"], stats["with_cell_pixels"],
                                         stats["cell_pixels_on_a_row_of_another_size"], stats["with_components"],
                                         stats["components_on_rows_of_another_size"], stats["components_found"],
                                         stats["with_two_components_or_more"], stats["with_normals_cell_pixels_and_components"],
                                         stats["nonzero_id_offsets"], json.dumps(stats["keeps"], sort_keys=True), stats["keeps_that_dropped"],
                                         stats["keeps_to_nothing"], stats["chained_keeps"], stats["behind_keep"]), flush=True)
    finally:
        close_contexts(contexts)
    stats["seconds"] = round(time.time() - t0, 1)
    stats["seed"] = args.seed
    stats["options"] = {k: v for k, v in options.items() if v not in (None, False)}
    stats["identical"] = True
    print(json.dumps(stats), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
