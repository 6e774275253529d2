#!/usr/bin/env python3
"""A differential campaign through the C++ drop-in filter, itk::CuberilleImageToMeshFilter, update after update -- run by hand on
a GPU box, its summary committed under profiles/:

    python tests/fuzz_dropin.py --seconds 300 --seed 1 > fuzz_dropin_seed1.log

The cases are those of tests/fuzz_campaign.py -- draw_case(seed, case) there draws the volume, the geometry, the eight parameters,
the view (border, region, band), the B-spline's width, normals, cell pixels, components, the keep and the repeat; its expected()
gives every reference, never the library -- and each carries a `dropin` entry drawn from a stream of its own,
np.random.default_rng([seed, case, 6]) (no earlier stream moves: tests/golden/campaign_dropin_recipe_digests.json pins this one,
the two older digest files stay as they are):

  path      device      LinearInterpolateImageFunction: the walk on the GPU
            group       SetDevices with `members` (2, 3 or 8) copies of device 0: the volume cut into z-slabs
            host_walk   a user's class that derives from the linear interpolator and inherits its Evaluate(): the filter cannot
                        know that, does the topology on the GPU (on `hw_members` slabs, now and then) and walks on the host
                        with `threads` threads -- the reference is the SAME oracle mesh, bit for bit
            stale       ReproduceStaleGradientOn(): the recipe's first image, one Update(), then the case's -- the oracle's first= run
            (a B-spline case: device = SetBSplineOnDevice(true), host_walk = false, ITK-lite's own class on the host)
  traits    static (itk::Mesh<float, 3>) or dynamic (itk::Mesh<double, 3, DefaultDynamicMeshTraits>: filled element by element)
  fresh     a new filter object for this case (else the one the cases before left), with eager setup on or off
  release   ReleaseHostMeshAfterFillOn()
  sticky    the step length is not set: the object keeps what it has -- the default, max spacing * 0.25, resolved ONCE by the first
            Update() of the object (txx:82-85), or the last value a case set.  The generator follows every object and hands the
            oracle the step the object holds by then; GetProjectVertexStepLength() is compared as well
  mask_as   where the recipe's keep drew the `mask` rule, which the filter does not offer: `largest` or a minimum of cells.  A
            keep of two stages is KeepLargestComponentOn() followed by SetMinimumComponentCells(n), the filter's fixed order;
            every n is resolved on the REFERENCE's counts (fuzz_campaign.keep_arguments)
  refusal   one combination the header documents as refused (REFUSALS), made on the case's object FIRST, on the case's image with
            every other switch off: Update() throws, the message holds the refusal's words, every accessor and the mesh are empty
            (the header's rule) -- and the case itself, next on that object, must be right in full
  plain     None, `after` or `around`: a further Update() of the same object on the same image with every switch off, behind the
            case (and ahead of it): what was on is off, and the accessors must be empty again

A case is one to four LINES of a script (tests of the filter: refusal, plain, main -- with the stale route's first image --, plain);
midas-journal-740_amd/itk/build/fuzz_update runs a script's lines in order in ONE process, one long-lived filter object per (pixel
type, interpolator type, mesh traits), and writes what the public API of the mesh and the filter hands out as bytes; compare_line
holds every row to the reference, exactly: conftest.assert_same_mesh, normals_ref.same_normals, bytes for every other row, a NaN
equal to a NaN, no tolerance anywhere.  Cell data is the reference's pixels cast to the mesh's pixel type by numpy.

The compiled-out projection and gradient variants (USE_ADVANCED_PROJECTION, USE_LINESEARCH_PROJECTION,
USE_GRADIENT_RECURSIVE_GAUSSIAN) need builds of their own with the macro defined: they stay with the reference-driver tests and are
out of scope here -- every drop-in recipe takes the default branch.  So are the development switches and the chunked upload of the C
ABI's campaign, which the filter does not expose.

A hand run takes the cases in batches of BATCH, one process per batch under a `timeout` of its own, objects kept within a batch;
it stops at the first batch whose process fails or whose case differs and prints the `--seed S --case N` that replays it: the cases
of N's batch up to N, in one process, as the run had them.  TEST INFRASTRUCTURE: the oracle is the checker, never the thing shipped."""
import argparse
import copy
import json
import os
import subprocess
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fuzz_campaign as fz  # noqa: E402
from conftest import assert_same_mesh  # noqa: E402

PIX = {"uint8": "u8", "int8": "i8", "uint16": "u16", "int16": "i16", "uint32": "u32", "int32": "i32", "float32": "f32",
       "float64": "f64", "int64": "i64", "uint64": "u64"}
# cuberille_image_desc::pixel_type (include/cuberille_hip.h) as the dry mode prints it
PIXEL_CODES = {"uint8": 0, "int8": 1, "uint16": 2, "int16": 3, "uint32": 4, "int32": 5, "float32": 6, "float64": 7, "int64": 8, "uint64": 9}
PATHS = {"whole": ["device", "group", "host_walk", "stale"], "border": ["device"], "region": ["device"], "band": ["device"],
         "bspline": ["device", "host_walk"]}
BATCH = 25

# name: (the paths whose object can make it, a fragment the message must contain).  hw_*: the host walk with what it does not
# offer; grp_*: SetDevices of two with what a slab does not offer; the last two: arguments refused whatever the route.
LINEAR = ("device", "group", "stale")
REFUSALS = {
    "hw_border": (("host_walk",), "an implied border (PadBorderOn / cuberille_set_border) is not offered with an interpolator that takes the host walk"),
    "hw_region": (("host_walk",), "an extraction region (SetExtractionRegion / cuberille_set_region) is not offered with an interpolator that takes the host walk"),
    "hw_band": (("host_walk",), "a band (InsideBandOn / cuberille_set_band) is not offered with an interpolator that takes the host walk"),
    "hw_normals": (("host_walk",), "point normals (GeneratePointNormalsOn / cuberille_set_point_normals) are not offered with an interpolator that takes the host walk"),
    "hw_keep": (("host_walk",), "keeping components (KeepLargestComponentOn / SetMinimumComponentCells / cuberille_keep_components) is not offered with an interpolator"),
    "grp_region": (LINEAR, "an extraction region (SetExtractionRegion / cuberille_set_region) is not offered with SetDevices of more than one device"),
    "grp_border": (LINEAR, "has an implied border set (cuberille_set_border)"),
    "grp_band": (LINEAR, "has a band set (cuberille_set_band)"),
    "grp_normals": (LINEAR, "has point normals set (cuberille_set_point_normals)"),
    "grp_celldata": (LINEAR, "has cell pixels set (cuberille_set_cell_pixels)"),
    "grp_components": (LINEAR, "has components set (cuberille_set_components)"),
    "band_inverted": (("device", "group", "stale", "host_walk"), "the lower bound is above the upper bound"),
    "region_outside": (("device", "group", "stale", "host_walk"), "lie inside the input's buffered region"),
}
REFUSAL_NAMES = sorted(REFUSALS)
# the switches a line can have on; SWITCHES_ON_OFF: those the slice must show on in one line and off in the next of the same object
SWITCHES_ON_OFF = ("border", "region", "bandon", "normals", "celldata", "components", "largest", "mincells", "stale", "devices", "release")
DEFAULT_OPTIONS = dict(fz.DEFAULT_OPTIONS, path=None, traits=None, fresh=None, eager=None, release=None, sticky=None, refusal=None,
                       plain=None, members=None, project=None)


# ---- 1. the recipe ---------------------------------------------------------------------------------------------------------
def draw_dropin(seed, case, kind, opt):
    """The `dropin` entry: every draw is made whatever the options fix, so that the stream does not depend on them."""
    rng = np.random.default_rng([int(seed), int(case), 6])
    paths = PATHS[kind]
    path = str(paths[int(rng.integers(0, len(paths)))])
    dynamic = bool(rng.random() < 0.35)
    members, hw_members, threads = int(rng.choice([2, 3, 8])), int(rng.choice([0, 0, 0, 2, 3])), int(rng.choice([1, 4]))
    fresh, eager, release, sticky = bool(rng.random() < 0.15), bool(rng.random() < 0.7), bool(rng.random() < 0.25), bool(rng.random() < 0.3)
    mask_as = ["largest", "min_cells"][int(rng.integers(0, 2))]
    u, q, plus = rng.random(), float(rng.random()), bool(rng.integers(0, 2))
    mask_min = dict(rule="min_cells", pick="zero" if u < 0.1 else ("above_max" if u < 0.2 else "quantile"), quantile=round(q, 6), plus_one=plus)
    refuse, which = bool(rng.random() < 0.3), int(rng.integers(0, 1 << 16))
    plain = [None, None, None, "after", "after", "around"][int(rng.integers(0, 6))]
    pick = lambda name, drawn: drawn if opt.get(name) is None else opt[name]          # noqa: E731
    path = pick("path", path)
    assert path in paths, (kind, path)
    d = dict(path=path, traits=pick("traits", "dynamic" if dynamic else "static"), members=int(pick("members", members)), hw_members=hw_members,
             threads=threads, fresh=bool(pick("fresh", fresh)), eager=bool(pick("eager", eager)), release=bool(pick("release", release)),
             sticky=bool(pick("sticky", sticky)), mask_as=mask_as, mask_min=mask_min, plain=pick("plain", plain) or None)
    if kind == "bspline" or path == "host_walk":
        d["traits"] = "static"                           # (the dynamic mesh is instantiated beside the linear interpolator)
    names = [n for n in REFUSAL_NAMES if path in REFUSALS[n][0] and not (kind == "bspline" and n[:3] in ("hw_", "grp"))]
    refusal = names[which % len(names)] if refuse else None
    if opt.get("refusal") is not None:
        refusal = opt["refusal"] or None
        assert refusal is None or refusal in names, (refusal, path, kind)
    d["refusal"] = refusal
    return d


def draw_case(seed, case, options=None):
    """fuzz_campaign.draw_case(seed, case) with the route fixed to what the filter does (a host image; `held` for the stale
    path), what the filter does not expose taken out, what a path refuses switched off, the keep mapped to the filter's two rules
    -- and the `dropin` entry.  A pure function of (seed, case, options); needs no GPU and no oracle."""
    opt = dict(DEFAULT_OPTIONS)
    opt.update(options or {})
    kind = opt["kind"] or str(np.random.default_rng([int(seed), int(case)]).choice(fz.KINDS, p=[0.46, 0.15, 0.17, 0.15, 0.07]))
    d = draw_dropin(seed, case, kind, opt)
    path = d["path"]
    fopt = {k: opt[k] for k in fz.DEFAULT_OPTIONS}
    fopt.update(kind=kind, route="held" if path == "stale" else "host", recursive_gaussian=False)
    slabs = path == "group" or (path == "host_walk" and kind == "whole" and d["hw_members"] > 0)
    if slabs:                                            # a slab offers neither cell pixels nor components
        fopt.update(cell_pixels=False, components=False)
    recipe = fz.draw_case(seed, case, fopt)
    assert recipe["kind"] == kind
    for key in ("refusal", "refusal_slab", "switch", "chunk_kib", "emit_offset"):       # the C ABI's own: not the filter's
        recipe.pop(key, None)
    recipe["kw"]["variant"] = 0
    if opt["project"] is not None:                       # (a slice's host-walk cases: all of them walk)
        recipe["kw"]["project"] = bool(opt["project"])
    recipe["kw"].pop("gradient", None)
    host_walks = path == "host_walk" and recipe["kw"]["project"]
    if slabs or host_walks or path == "stale":
        recipe["normals"] = False
    if host_walks or not recipe.get("components"):
        recipe["keep"] = None
    if recipe.get("keep"):
        recipe["keep"] = filter_keep(recipe["keep"], d)
    recipe["dropin"] = d
    return recipe


def filter_keep(keep, d):
    """A recipe's keep as the filter offers it: `largest`, a minimum of cells, or largest and then a minimum."""
    stages = [dict(s) for s in fz.keep_stages(keep)]
    for i, s in enumerate(stages):
        if s["rule"] == "mask":
            stages[i] = dict(rule="largest") if d["mask_as"] == "largest" else dict(d["mask_min"])
    largest = any(s["rule"] == "largest" for s in stages)
    minimum = next((s for s in stages if s["rule"] == "min_cells"), None)
    if largest:
        return dict(rule="largest", then=minimum if len(stages) > 1 else None)
    return dict(minimum, then=None)


# ---- 2. lines ----------------------------------------------------------------------------------------------------------------
def _pixel_text(v, dt):
    if np.dtype(dt).kind == "f":
        v = float(fz._num(v))
        return "nan" if v != v else ("inf" if v == np.inf else ("-inf" if v == -np.inf else float(np.dtype(dt).type(v)).hex()))
    return str(int(v))


def _real(v):
    v = float(v)
    return "nan" if v != v else ("inf" if v == np.inf else ("-inf" if v == -np.inf else v.hex()))


def _plain_recipe(recipe):
    """The recipe of a `plain` line: the same buffer and parameters, every switch off."""
    r = copy.deepcopy(recipe)
    if r["kind"] != "bspline":
        r["kind"] = "whole"
    for key in ("border", "region", "band", "first"):
        r.pop(key, None)
    r.update(route="host", normals=False, cell_pixels=False, components=False, keep=None, repeat=1)
    return r


def _base_settings(recipe):
    d, kind = recipe["dropin"], recipe["kind"]
    interp = "bspline%d" % recipe["bspline"]["bits"] if kind == "bspline" else ("inherit" if d["path"] == "host_walk" else "linear")
    kw = recipe["kw"]
    return dict(pix=PIX[recipe["dtype"]], dtype=recipe["dtype"], interp=interp, traits=d["traits"], fresh=False, eager=d["eager"], release=False,
                field=recipe["field"], spacing=list(recipe["spacing"]), origin=list(recipe["origin"]), direction=np.asarray(recipe["direction"], dtype=np.float64).ravel().tolist(),
                start=list(recipe["index_start"]), iso=recipe["iso"], tri=bool(kw["triangles"]), project=bool(kw["project"]), thr=kw["threshold"],
                step=None if d["sticky"] else kw["step"], relax=kw["relax"], maxsteps=int(kw["max_steps"]), devices=0, threads=d["threads"],
                border=None, region=None, band=None, bandon=False, normals=False, celldata=False, components=False, largest=False, mincells=0,
                stale=False, bsplinedev=not (kind == "bspline" and d["path"] == "host_walk"), updates=1, first=None)


def _refusal_settings(recipe, s):
    """The base settings with the one thing that is refused."""
    name = recipe["dropin"]["refusal"]
    dt = np.dtype(recipe["dtype"])
    nz, ny, nx = recipe["field"]["shape"]
    start = [int(v) for v in recipe["index_start"]]
    s = dict(s)
    band = [0.0, 1.0, 1.0, 0.0] if dt.kind == "f" else [int(recipe["iso"]), int(recipe["iso"]), 1, 0]
    if name[:3] == "hw_":
        s["project"] = True                             # (without projection nothing walks, on the host or elsewhere)
    if name[:4] == "grp_":
        s["devices"] = 2
    what = name.split("_", 1)[1]
    if name == "region_outside":
        s["region"] = start + [nx + 1, ny, nz]
    elif name == "band_inverted":
        s.update(band=[band[1] + 1, band[0], band[2], band[3]], bandon=True)
    elif what == "border":
        s["border"] = 0
    elif what == "region":
        s["region"] = start + [nx, ny, nz]
    elif what == "band":
        s.update(band=band, bandon=True)
    elif what == "normals":
        s["normals"] = True
    elif what == "celldata":
        s["celldata"] = True
    elif what == "components":
        s["components"] = True
    elif what == "keep":
        s["largest"] = True
    else:
        raise ValueError(name)
    return s


def case_lines(recipe, want):
    """The lines of one case, in order: dicts of sub, settings (what the script line says), recipe (what the reference is asked
    for: None for a refusal) and refusal.  want: fuzz_campaign.expected() of the recipe, whose keep_args hold every n."""
    d, kind = recipe["dropin"], recipe["kind"]
    base = _base_settings(recipe)
    main = dict(base, release=d["release"], normals=bool(recipe["normals"]), celldata=bool(recipe["cell_pixels"]), components=bool(recipe["components"]),
                updates=int(recipe.get("repeat", 1)))
    if d["path"] == "group":
        main["devices"] = d["members"]
    elif d["path"] == "host_walk" and kind == "whole":
        main["devices"] = d["hw_members"]
    elif d["path"] == "stale":
        f = recipe["first"]
        main.update(stale=True, first=dict(field=f["field"], spacing=list(f["spacing"]), origin=list(f["origin"]),
                                           direction=np.asarray(f["direction"], dtype=np.float64).ravel().tolist(), start=list(f["index_start"])))
    if kind == "border":
        main["border"] = recipe["border"]["value"]
    elif kind == "region":
        main["region"] = [a + int(b) for a, b in zip(recipe["index_start"], recipe["region"]["start"])] + [int(v) for v in recipe["region"]["size"]]
    elif kind == "band":
        b = recipe["band"]
        main.update(band=[b["lower"], b["upper"], b["inside"], b["outside"]], bandon=True)
    for stage, (rule, n, _) in zip(fz.keep_stages(recipe.get("keep")), want["keep_args"]):
        if rule == "largest":
            main["largest"] = True
        else:
            main["mincells"] = int(n)
    plain = dict(sub="plain", settings=dict(base), recipe=_plain_recipe(recipe), refusal=None)
    lines = []
    if d["refusal"]:
        lines.append(dict(sub="refusal", settings=_refusal_settings(recipe, base), recipe=None, refusal=d["refusal"]))
    if d["plain"] == "around":
        lines.append(copy.deepcopy(plain))
    lines.append(dict(sub="main", settings=main, recipe=recipe, refusal=None))
    if d["plain"]:
        lines.append(copy.deepcopy(plain))
    lines[0]["settings"]["fresh"] = d["fresh"]
    for line in lines:
        line["case"], line["seed"] = recipe["case"], recipe["seed"]
    return lines


def object_key(s):
    return (s["pix"], s["interp"], s["traits"])


def follow_objects(lines):
    """What the generator knows of every object by each line, written into the line: `step` (the step length the object holds
    when the line's LAST Update() runs -- what the oracle is handed and GetProjectVertexStepLength() must say), `step_default`
    (that value is a default resolved by an earlier image), `before` (the settings of the line before on the same object, or
    None), and a stale line on an object that still holds a gradient is made fresh (the reference never drops that image: the
    mesh would follow an earlier case's)."""
    objects = {}
    for line in lines:
        s = line["settings"]
        key = object_key(s)
        if s["stale"] and objects.get(key, {}).get("holds"):
            s["fresh"] = True
        if s["fresh"] or key not in objects:
            objects[key] = dict(step=None, default=False, holds=False, before=None)
        o = objects[key]
        if s["step"] is not None:
            o.update(step=min(max(float(s["step"]), 0.0), 100000.0), default=False)
        elif o["step"] is None:                        # resolved by the first image this object updates on
            spacing = s["first"]["spacing"] if s["first"] else s["spacing"]
            o.update(step=max(float(v) for v in spacing) * 0.25, default=True)
        line["step"], line["step_default"], line["before"] = o["step"], o["default"], o["before"]
        # the held image goes when a single context updates with the switch off (a refusal leaves before that, a group never asks)
        if s["stale"]:
            o["holds"] = True
        elif line["sub"] != "refusal" and not s["devices"]:
            o["holds"] = False
        o["before"] = dict(s, threw=line["sub"] == "refusal")
    return lines


def script_line(number, line, vol_path, first_path=None):
    s = line["settings"]
    dt = s["dtype"]
    nz, ny, nx = s["field"]["shape"]
    words = ["line=%d" % number, "case=%d" % line["case"], "sub=%s" % line["sub"], "pix=%s" % s["pix"], "interp=%s" % s["interp"], "traits=%s" % s["traits"],
             "fresh=%d" % s["fresh"], "eager=%d" % s["eager"], "release=%d" % s["release"], "vol=%s" % vol_path, "dims=%d,%d,%d" % (nx, ny, nz),
             "spacing=" + ",".join(_real(v) for v in s["spacing"]), "origin=" + ",".join(_real(v) for v in s["origin"]),
             "direction=" + ",".join(_real(v) for v in s["direction"]), "start=" + ",".join(str(int(v)) for v in s["start"]),
             "iso=" + _pixel_text(s["iso"], dt), "tri=%d" % s["tri"], "project=%d" % s["project"], "thr=" + _real(s["thr"]),
             "step=" + ("keep" if s["step"] is None else _real(s["step"])), "relax=" + _real(s["relax"]), "maxsteps=%d" % s["maxsteps"],
             "devices=%d" % s["devices"], "threads=%d" % s["threads"]]
    if s["border"] is not None:
        words.append("border=" + _pixel_text(s["border"], dt))
    if s["region"] is not None:
        words.append("region=" + ",".join(str(int(v)) for v in s["region"]))
    if s["band"] is not None:
        words.append("band=" + ",".join(_pixel_text(v, dt) for v in s["band"]))
    words += ["bandon=%d" % s["bandon"], "normals=%d" % s["normals"], "celldata=%d" % s["celldata"], "components=%d" % s["components"],
              "largest=%d" % s["largest"], "mincells=%d" % s["mincells"], "stale=%d" % s["stale"], "bsplinedev=%d" % s["bsplinedev"], "updates=%d" % s["updates"]]
    if s["first"] is not None:
        f = s["first"]
        fz_, fy, fx = f["field"]["shape"]
        words += ["first_vol=%s" % first_path, "first_dims=%d,%d,%d" % (fx, fy, fz_), "first_spacing=" + ",".join(_real(v) for v in f["spacing"]),
                  "first_origin=" + ",".join(_real(v) for v in f["origin"]), "first_direction=" + ",".join(_real(v) for v in f["direction"]),
                  "first_start=" + ",".join(str(int(v)) for v in f["start"])]
    return " ".join(words)


# ---- 3. references -----------------------------------------------------------------------------------------------------------
def mesh_pixel_dtype(traits):
    return np.dtype(np.float64 if traits == "dynamic" else np.float32)


def reference(oracle, line):
    """What fuzz_update must write for the line, from the references alone: {"threw", "fragment"} for a refusal, else every row
    and figure (of the kept mesh where the line keeps).  The oracle is handed the step the object holds (line["step"])."""
    s = line["settings"]
    empty = dict(points=np.zeros((0, 3), np.float32), cells=np.zeros((0, 3), np.uint64), celldata=None, normals=np.zeros((0, 3), np.float32),
                 pixels=np.zeros(0, np.dtype(s["dtype"])), pcomp=np.zeros(0, np.uint32), ccomp=np.zeros(0, np.uint32), counts=np.zeros(0, np.uint64), K=0)
    if line["sub"] == "refusal":
        return dict(empty, threw=True, fragment=REFUSALS[line["refusal"]][1], step=line["step"], slabs=None, want=None)
    recipe = copy.deepcopy(line["recipe"])
    recipe["kw"]["step"] = line["step"]
    want = fz.expected(oracle, recipe)
    mesh = want["mesh"]
    ref = dict(empty, threw=False, fragment=None, step=line["step"], want=want,
               slabs=min(s["devices"], s["field"]["shape"][0]) if s["devices"] > 1 and s["interp"][:7] != "bspline" and not s["stale"] else 1)
    ref["points"], ref["cells"] = np.ascontiguousarray(mesh.points, dtype=np.float32), np.ascontiguousarray(mesh.cells, dtype=np.uint64)
    normals, pixels, components = want["normals"], want["cell_pixels"], want["components"]
    if want["kept"]:
        k = want["kept"][-1]
        ref["points"], ref["cells"] = np.ascontiguousarray(k.points, dtype=np.float32), np.ascontiguousarray(k.cells, dtype=np.uint64)
        normals, pixels, components = k.normals, k.cell_pixels, (k.point_component, k.cell_component, k.component_cells)
    ref["cells"] = ref["cells"].reshape(-1, 3 if s["tri"] else 4)
    if normals is not None:
        ref["normals"] = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    if pixels is not None:
        ref["pixels"] = np.ascontiguousarray(pixels)
        # (the container is made by the first SetCellData(id, value), as itk::Mesh makes it: a mesh without cells has none)
        with np.errstate(over="ignore", invalid="ignore"):
            ref["celldata"] = ref["pixels"].astype(mesh_pixel_dtype(s["traits"])) if len(ref["pixels"]) else None
    if components is not None:
        ref["pcomp"], ref["ccomp"], ref["counts"] = (np.ascontiguousarray(a) for a in components)
        ref["K"] = len(ref["counts"])
    return ref


def write_reference(ref, outdir, number, traits="static"):
    """The files fuzz_update would write for a line whose results are the reference's (the comparer's own test fabricates them)."""
    base = os.path.join(outdir, "%d." % number)
    cells = ref["cells"]
    rows = dict(points=ref["points"], arity=np.full(len(cells), cells.shape[1] if cells.ndim == 2 else 0, np.uint8), cells=cells,
                celldata=ref["celldata"] if ref["celldata"] is not None else np.zeros(0, mesh_pixel_dtype(traits)), normals=ref["normals"],
                pixels=ref["pixels"], pcomp=ref["pcomp"], ccomp=ref["ccomp"], counts=ref["counts"])
    for name, a in rows.items():
        np.ascontiguousarray(a).tofile(base + name)
    with open(base + "meta", "w") as f:
        f.write("threw=%d\nwhat=%s\npoints=%d\ncells=%d\ncelldata=%d\ncelldata_missing=0\nK=%d\nslabs=%d\nstep=%s\n" % (
            ref["threw"], "itk::ERROR: " + ref["fragment"] if ref["threw"] else "", len(ref["points"]), len(cells), ref["celldata"] is not None,
            ref["K"], ref["slabs"] or 0, _real(ref["step"])))


def read_line(outdir, number, s):
    """What fuzz_update wrote for line `number` (settings s: the pixel type and the traits say how the bytes read)."""
    base = os.path.join(outdir, "%d." % number)
    meta = {}
    with open(base + "meta") as f:
        for text in f.read().splitlines():
            k, _, v = text.partition("=")
            meta[k] = v
    rd = lambda name, dt: np.fromfile(base + name, dtype=dt)                      # noqa: E731
    got = dict(threw=meta["threw"] == "1", what=meta["what"], n_points=int(meta["points"]), n_cells=int(meta["cells"]), has_celldata=meta["celldata"] == "1",
               celldata_missing=int(meta["celldata_missing"]), K=int(meta["K"]), slabs=int(meta["slabs"]), step=float.fromhex(meta["step"]),
               points=rd("points", np.float32).reshape(-1, 3), arity=rd("arity", np.uint8), cells=rd("cells", np.uint64),
               celldata=rd("celldata", mesh_pixel_dtype(s["traits"])), normals=rd("normals", np.float32).reshape(-1, 3), pixels=rd("pixels", np.dtype(s["dtype"])),
               pcomp=rd("pcomp", np.uint32), ccomp=rd("ccomp", np.uint32), counts=rd("counts", np.uint64))
    return got


def _same_bytes(got, want, what, nan_equal=False):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() == want.tobytes():
        return
    diff = (got.view(np.uint8) != want.view(np.uint8)).reshape(len(got), -1).any(axis=1)
    if nan_equal and got.dtype.kind == "f":
        diff &= ~(np.isnan(got) & np.isnan(want)).reshape(len(got), -1).all(axis=1)
    assert not diff.any(), "%s: %d differ, first at %d: %r, reference %r" % (what, int(diff.sum()), int(np.argmax(diff)), got[np.argmax(diff)], want[np.argmax(diff)])


def compare_line(got, ref):
    """The first difference between what fuzz_update wrote and the reference, as an AssertionError.  Exact."""
    import normals_ref
    if ref["threw"]:
        assert got["threw"], "the refused combination was accepted"
        assert ref["fragment"] in got["what"], "refused for another reason: %s" % got["what"]
    else:
        assert not got["threw"], "Update() threw: %s" % got["what"]
        assert got["slabs"] == ref["slabs"], ("GetLastNumberOfSlabs", got["slabs"], ref["slabs"])
    assert got["step"] == ref["step"], ("GetProjectVertexStepLength", got["step"], ref["step"])
    assert got["n_points"] == len(got["points"]) and got["n_cells"] == len(got["arity"])
    cells = ref["cells"]
    arity = cells.shape[1]
    assert (got["arity"] == arity).all(), ("a cell of %d points among the mesh's" % arity, np.unique(got["arity"]).tolist())
    assert len(got["cells"]) == arity * len(got["arity"]), "the cells' ids are not their arities' sum"
    assert_same_mesh(SimpleNamespace(points=got["points"], cells=got["cells"].reshape(-1, arity)), SimpleNamespace(points=ref["points"], cells=cells))
    assert got["has_celldata"] == (ref["celldata"] is not None), "the mesh has %s cell-data container" % ("a" if got["has_celldata"] else "no")
    if ref["celldata"] is not None:
        assert got["celldata_missing"] == 0, "%d cells without cell data" % got["celldata_missing"]
        _same_bytes(got["celldata"], ref["celldata"], "cell data", nan_equal=True)
    else:
        assert len(got["celldata"]) == 0
    normals_ref.same_normals(got["normals"], ref["normals"], "normals")
    _same_bytes(got["pixels"], ref["pixels"], "cell pixels")
    for name in ("pcomp", "ccomp", "counts"):
        _same_bytes(got[name], ref[name], name)
    assert got["K"] == ref["K"], ("GetNumberOfComponents", got["K"], ref["K"])


# ---- 4. a batch: one script, one process ------------------------------------------------------------------------------------------
_MADE = set()


def exe():
    """itk/build/fuzz_update, made by build(); make decides once per process whether it is missing or older than its sources.
    A binary that cannot be had is an error, never a skip."""
    path = os.path.join(ROOT, "midas-journal-740_amd", "itk", "build", "fuzz_update")
    if path not in _MADE:
        _MADE.add(path)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "midas-journal-740_amd", "itk"), "build/fuzz_update"])
    assert os.path.exists(path), path
    return path


def prepare(oracle, recipes, tmp=None):
    """(lines, refs, script): the lines of the recipes in order on their objects (follow_objects), the reference of every line,
    and the script's text -- the volumes written under tmp (None: no files, `-` in their place, for the dry mode)."""
    lines = []
    for recipe in recipes:
        lines += case_lines(recipe, fz.expected(oracle, recipe) if recipe.get("keep") else dict(keep_args=[]))
    follow_objects(lines)
    refs, text = [], []
    for number, line in enumerate(lines):
        refs.append(reference(oracle, line))
        vol = first = "-"
        if tmp is not None:
            vol = os.path.join(tmp, "v%d.raw" % number)
            fz._field(line["settings"]["field"])[0].tofile(vol)
            if line["settings"]["first"]:
                first = os.path.join(tmp, "f%d.raw" % number)
                fz._field(line["settings"]["first"]["field"])[0].tofile(first)
        text.append(script_line(number, line, vol, first))
    return lines, refs, "\n".join(text) + "\n"


def replay_words(line):
    return "--seed %d --case %d" % (line["seed"], line["case"])


def run_batch(oracle, recipes, seconds=120):
    """One script in one process under a timeout of its own; every line compared.  Returns (lines, refs, wall seconds of the
    process); raises AssertionError naming the case that replays the first failure."""
    with tempfile.TemporaryDirectory() as tmp:
        lines, refs, script = prepare(oracle, recipes, tmp)
        path = os.path.join(tmp, "script.txt")
        with open(path, "w") as f:
            f.write(script)
        out = os.path.join(tmp, "out")
        os.mkdir(out)
        t0 = time.time()
        r = subprocess.run(["timeout", "-k", "10", str(int(seconds)), exe(), "run", path, out], capture_output=True, text=True)
        wall = time.time() - t0
        done = sum(os.path.exists(os.path.join(out, "%d.meta" % n)) for n in range(len(lines)))
        if r.returncode != 0:
            at = lines[min(done, len(lines) - 1)]
            raise AssertionError("fuzz_update exited with %d at line %d of %d (%s): replay with %s\n%s\n%s" % (
                r.returncode, done, len(lines), script.splitlines()[min(done, len(lines) - 1)], replay_words(at), r.stdout[-2000:], r.stderr[-2000:]))
        for number, (line, ref) in enumerate(zip(lines, refs)):
            try:
                compare_line(read_line(out, number, line["settings"]), ref)
            except AssertionError as e:
                raise AssertionError("%s line %d (%s of case %d, %s %s %s): %s\n  replay with %s\n  %s" % (
                    line["recipe"]["kind"] if line["recipe"] else "refusal", number, line["sub"], line["case"], line["settings"]["pix"], line["settings"]["interp"],
                    line["settings"]["traits"], e, replay_words(line), script.splitlines()[number])) from e
    return lines, refs, wall


# ---- the dry mode: every setter against every getter, no GPU ---------------------------------------------------------------------
def _number(text, dt=None):
    """A printed value in a form that compares: the integer types as int, the floating ones as float.hex() -- the sign of a zero
    counts, a NaN is a NaN."""
    if dt is not None and np.dtype(dt).kind != "f":
        return int(text)
    v = float(text) if text.lstrip("-") in ("nan", "inf") else float.fromhex(text)
    return "nan" if v != v else v.hex()


def dry_getters(lines):
    """What `fuzz_update dry` must print for the lines, one dict per line: every getter after the line's setters, with the
    reference's clamps (h:209-228: the threshold into [0, NumericTraits<InputPixelType>::max()], the step length into [0, 100000],
    the relaxation into [0, 1]) and the drop-in's (1 .. 256 host-walk threads); the step length is the last one SET on the object
    (-1 on an object no line has set it on: nothing updates here); the image description and the buffer box are the recipe's."""
    out, steps = [], {}
    for line in lines:
        s = line["settings"]
        dt = np.dtype(s["dtype"])
        key = object_key(s)
        if s["fresh"] or key not in steps:
            steps[key] = -1.0
        if s["step"] is not None:
            steps[key] = min(max(float(s["step"]), 0.0), 100000.0)
        top = float(np.finfo(dt).max) if dt.kind == "f" else float(np.iinfo(dt).max)
        pixel = lambda v: _number(_pixel_text(v, dt), dt)                    # noqa: E731
        nz, ny, nx = s["field"]["shape"]
        band = s["band"] if s["band"] is not None else [0, 0, 1, 0]
        g = dict(iso=pixel(s["iso"]), tri=int(s["tri"]), project=int(s["project"]), thr=min(max(float(s["thr"]), 0.0), top).hex(), step=steps[key].hex(),
                 relax=min(max(float(s["relax"]), 0.0), 1.0).hex(), maxsteps=s["maxsteps"], devices=s["devices"], threads=min(max(s["threads"], 1), 256),
                 release=int(s["release"]), stale=int(s["stale"]), bsplinedev=int(s["bsplinedev"]), eager=0, padborder=int(s["border"] is not None),
                 border=pixel(s["border"] if s["border"] is not None else 0), hasregion=int(s["region"] is not None), bandon=int(s["bandon"]),
                 band=[pixel(v) for v in band], normals=int(s["normals"]), celldata=int(s["celldata"]), components=int(s["components"]),
                 largest=int(s["largest"]), mincells=int(s["mincells"]), described=1, pixel_type=PIXEL_CODES[s["dtype"]], desc_dims=[nx, ny, nz],
                 desc_start=[int(v) for v in s["start"]], desc_spacing=[float(v).hex() for v in s["spacing"]], desc_origin=[float(v).hex() for v in s["origin"]],
                 desc_direction=[float(v).hex() for v in s["direction"]],
                 box=[int(a) - int(b) for a, b in zip(s["region"][:3], s["start"])] + [int(v) for v in s["region"][3:]] if s["region"] is not None else [0] * 6)
        if s["region"] is not None:
            g["region"] = [int(v) for v in s["region"]]
        out.append(g)
    return out


def parse_dry(text, lines):
    """The dicts `fuzz_update dry` printed, in dry_getters' form."""
    out = []
    for row, line in zip(text.splitlines(), lines):
        dt = line["settings"]["dtype"]
        w = dict(word.split("=", 1) for word in row.split())
        assert "device_not_0" not in w
        g = {}
        for k, v in w.items():
            if k == "line":
                continue
            if k in ("iso", "border"):
                g[k] = _number(v, dt)
            elif k == "band":
                g[k] = [_number(x, dt) for x in v.split(",")]
            elif k in ("thr", "step", "relax"):
                g[k] = _number(v)
            elif k in ("desc_spacing", "desc_origin", "desc_direction"):
                g[k] = [_number(x) for x in v.split(",")]
            elif k in ("desc_dims", "desc_start", "box", "region"):
                g[k] = [int(x) for x in v.split(",")]
            else:
                g[k] = int(v)
        out.append(g)
    return out


def run_dry(script):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "script.txt")
        with open(path, "w") as f:
            f.write(script)
        r = subprocess.run([exe(), "dry", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-1000:])
    return r.stdout


# ---- 5. the seeded slice of the GPU suite (tests/test_gpu_dropin_campaign.py; on the oracle alone: tests/test_campaign_scripts.py) ----
# kind: seed.  20 cases per kind; case i takes pixel type DTYPES[i % 10]; the path, the refusal, the plain lines and the object's
# switches follow RULES OF THE CASE NUMBER (slice_options), everything else is drawn.  The seeds are the first for which the oracle
# alone shows slice_conditions() and the cap on empty meshes.
SLICE_CASES = 20
SLICE = {"whole": 1, "border": 1, "region": 1, "band": 1, "bspline": 1}


def slice_options(kind, i):
    """The options of case i of a kind's slice.
    whole: the host walk where (i + i // 10) is even -- all ten pixel types --, the other ten cases group (2, 3, 8, 8 members), stale
    and device in turn; the host-walk cases all project; every host-walk case is behind one of the five hw_ refusals in turn, every other whole case behind
    a grp_ refusal or one of the two argument refusals in turn.  Views: the device path, a refusal ahead of every third case.
    Every third case is followed by a plain line, every sixth surrounded; every seventh object is fresh, eager setup off on every
    other of those; release on every fourth case; the step left alone on every third."""
    o = dict(fz.SLICE_OPTIONS, kind=kind, dtype=np.dtype(fz.DTYPES[i % len(fz.DTYPES)]).name, cell_pixels=(i + i // 10) % 2 == 0,
             components=i % 3 != 2, keep=fz.KEEP_RULES[(i // 2) % 3], fresh=i % 7 == 3, eager=i % 14 != 3, release=i % 4 == 1, sticky=i % 3 == 1,
             plain=[None, "after", None, "around", None, "after"][i % 6], refusal="")
    others = ["grp_region", "grp_border", "grp_band", "grp_normals", "grp_celldata", "grp_components", "band_inverted", "region_outside"]
    if kind == "whole":
        if (i + i // 10) % 2 == 0:
            j = i // 2
            o.update(path="host_walk", project=True, refusal=["hw_border", "hw_region", "hw_band", "hw_normals", "hw_keep", "band_inverted", "region_outside", ""][j % 8])
        else:
            j = i // 2
            o.update(path=["group", "stale", "group", "stale", "device"][j % 5], members=[2, 3, 8, 8][(j // 2) % 4], refusal=others[j % 8],
                     traits="dynamic" if j % 5 == 4 else "static")
            if o["path"] == "stale":
                o.update(fresh=True, sticky=True)       # the default resolved on the first image sticks on the second
                if j % 5 == 3:                          # ... where no line of the case's own image comes first
                    o.update(refusal="", plain="after")
    elif kind == "bspline":
        o.update(path=["device", "host_walk"][i % 2], refusal=["", "band_inverted", "", "", "region_outside", ""][i % 6])
    else:
        o.update(path="device", traits="dynamic" if i % 3 == 0 else "static", refusal=([others[(i // 3) % 8]] + ["", ""])[i % 3])
    return o


def slice_recipes(kind, seed=None):
    seed = SLICE[kind] if seed is None else seed
    return [draw_case(seed, i, slice_options(kind, i)) for i in range(SLICE_CASES)]


def slice_facts(lines, refs):
    """What every executed line contributes to the conditions, from the lines and the references alone."""
    facts = []
    for line, ref in zip(lines, refs):
        s, want, before = line["settings"], ref["want"], line["before"]
        recipe = line["recipe"]
        f = dict(sub=line["sub"], case=line["case"], refusal=line["refusal"], threw=ref["threw"], key=object_key(s), dtype=s["dtype"], interp=s["interp"],
                 traits=s["traits"], devices=s["devices"], slices=s["field"]["shape"][0], fresh=s["fresh"], eager=s["eager"], release=s["release"],
                 stale=s["stale"], tri=s["tri"], project=s["project"], updates=s["updates"], celldata=s["celldata"], normals=s["normals"],
                 components=s["components"], keeps=s["largest"] or s["mincells"] > 0, kind=recipe["kind"] if recipe else None,
                 behind_throw=bool(before and before["threw"]), behind_release=bool(before and before["release"] and not before["threw"]),
                 behind_stale=bool(before and before["stale"] and not s["stale"] and not s["fresh"]),
                 turned_off=tuple(k for k in SWITCHES_ON_OFF if before and not before["threw"] and not s["fresh"] and before[k] not in (None, False, 0) and s[k] in (None, False, 0)))
        if ref["threw"]:
            facts.append(f)
            continue
        mesh = want["mesh"]
        img, _ = fz.frame(line["recipe"])
        inside = fz.inside_set(img, recipe["iso"])
        walks = bool(s["project"]) and len(mesh.points) > 0       # (a limit of 0 steps still takes two: txx:466-471)
        host_walk = walks and s["interp"] == "inherit"
        vox = fz.voxels(recipe)
        ks = None
        if recipe.get("keep"):
            ks = [len(want["components"][2])] + [len(k.component_cells) for k in want["kept"]]
        spacing_now = max(float(v) for v in s["spacing"]) * 0.25
        f.update(empty=len(mesh.points) == 0, walks=walks, host_walk=host_walk,
                 path="host_walk" if s["interp"] == "inherit" else ("group" if s["devices"] > 1 else ("stale" if s["stale"] else "device")),
                 general=not np.array_equal(np.asarray(s["direction"]).reshape(3, 3), np.eye(3)), moved=any(int(v) for v in s["start"]),
                 beyond_2_53=vox.dtype.kind in "iu" and vox.dtype.itemsize == 8 and bool((np.abs(vox.astype(np.float64)) > 2.0 ** 53).any()),
                 at_border=bool(inside[0].any() or inside[-1].any() or inside[:, 0].any() or inside[:, -1].any() or inside[:, :, 0].any() or inside[:, :, -1].any()),
                 ks=ks, all_off=not (s["normals"] or s["celldata"] or s["components"] or s["largest"] or s["mincells"]),
                 sticks=s["step"] is None and line["step_default"] and line["step"] != spacing_now and walks)
        facts.append(f)
    return facts


def slice_conditions(facts):
    """The conditions of the whole slice, all kinds together, as a list of those it misses (empty: all hold)."""
    missing = []

    def need(ok, what):
        if not ok:
            missing.append(what)
    ran = [f for f in facts if not f["threw"]]
    mains = [f for f in ran if f["sub"] == "main"]
    all_types = {np.dtype(d).name for d in fz.DTYPES}
    need({f["dtype"] for f in mains if f["path"] == "device"} == all_types, "all ten pixel types on the device path")
    need({f["dtype"] for f in mains if f["path"] == "host_walk" and f["host_walk"]} == all_types, "all ten pixel types on the host-walk path, each on a case that walks")
    for p in ("device", "group", "host_walk", "stale"):
        need(sum(f["path"] == p for f in mains) >= 4, "the path %s at least four times" % p)
    for n in (2, 3, 8):
        need(any(f["path"] == "group" and f["devices"] == n for f in mains), "a group of %d members" % n)
    need(any(f["devices"] > f["slices"] for f in mains), "a group with fewer slices than members")
    hw = [f for f in mains if f["host_walk"]]
    need(any(f["general"] for f in hw), "the host walk on a rotated geometry")
    need(any(f["moved"] for f in hw), "the host walk on a start index other than 0")
    need(any(f["beyond_2_53"] for f in hw), "the host walk on a 64-bit pixel type with values beyond 2^53")
    need(any(f["at_border"] for f in hw), "the host walk on a surface that meets the image border")
    need(any(f["celldata"] and f["tri"] for f in hw) and any(f["components"] and f["tri"] for f in hw), "the host walk's doubling of cell pixels and of components")
    need({f["tri"] for f in mains} == {True, False}, "quads and triangles")
    need({f["project"] for f in mains} == {True, False}, "projection on and off")
    need(any(f["traits"] == "dynamic" and f["celldata"] and not f["empty"] for f in mains), "dynamic traits with cell data")
    need(any(f["sticks"] for f in ran), "a default step length that sticks on an image of another largest spacing")
    for k in SWITCHES_ON_OFF:
        need(any(k in f["turned_off"] and f["all_off"] for f in ran), "the switch %s on in one line and off in the next of the same object" % k)
    went = {}                                            # per object: 1 single, 2 then group, 3 then single again
    for f in facts:
        state = went.get(f["key"], 0)
        if state == 3:
            continue
        if f["threw"]:
            state = 0
        else:
            state = 0 if f["fresh"] else state
            group = f["devices"] > 1
            state = {0: 0 if group else 1, 1: 2 if group else 1, 2: 2 if group else 3}[state]
        went[f["key"]] = state
    need(any(v == 3 for v in went.values()), "an object that goes single, then group, then single")
    need(any(f["behind_stale"] for f in ran), "stale followed by non-stale on the same object")
    need(any(f["fresh"] and not f["eager"] for f in facts), "a fresh object with eager setup off")
    need(any(f["behind_release"] for f in ran), "release-host-mesh on, followed by another update")
    for name in REFUSAL_NAMES:
        need(any(f["refusal"] == name for f in facts), "the refusal %s" % name)
    for i, f in enumerate(facts):
        if f["threw"]:
            need(i + 1 < len(facts) and not facts[i + 1]["threw"] and facts[i + 1]["key"] == f["key"] and facts[i + 1]["behind_throw"],
                 "the refusal of case %d followed by a full case on its object" % f["case"])
    keeps = [f for f in mains if f["ks"]]
    need(any(any(b < a for a, b in zip(f["ks"], f["ks"][1:])) for f in keeps), "a keep that drops something")
    need(any(f["ks"][0] >= 1 and f["ks"][-1] == 0 for f in keeps), "a keep that leaves nothing")
    need(any(f["normals"] and f["celldata"] and f["keeps"] for f in keeps), "a keep with normals and cell data")
    need(any(f["updates"] == 3 for f in mains), "a repeat (three updates)")
    for kind in fz.KINDS:
        mine = [f for f in mains if f["kind"] == kind]
        need(len(mine) == SLICE_CASES, "%d cases of kind %s" % (SLICE_CASES, kind))
        need(4 * sum(f["empty"] for f in mine) <= len(mine), "at most a quarter of the %s cases with an empty reference mesh" % kind)
    return missing


# ---- 6. hand runs ---------------------------------------------------------------------------------------------------------------
def tally(stats, lines, refs):
    for f in slice_facts(lines, refs):
        stats["lines"] += 1
        if f["threw"]:
            stats["refusals"][f["refusal"]] = stats["refusals"].get(f["refusal"], 0) + 1
            continue
        stats["behind_refusal"] += int(f["behind_throw"])
        if f["sub"] == "plain":
            stats["plain_lines"] += 1
            continue
        stats["cases"] += 1
        for key, val in (("paths", f["path"]), ("kinds", f["kind"]), ("dtypes", f["dtype"]), ("interpolators", f["interp"]), ("traits", f["traits"])):
            stats[key][val] = stats[key].get(val, 0) + 1
        for key in ("normals", "celldata", "components", "keeps", "empty", "host_walk", "sticks", "fresh", "release", "behind_stale"):
            stats[key] += int(bool(f[key]))
        stats["repeats"] += int(f["updates"] > 1)


def new_stats():
    return dict(cases=0, lines=0, plain_lines=0, refusals={}, behind_refusal=0, paths={}, kinds={}, dtypes={}, interpolators={}, traits={}, normals=0,
                celldata=0, components=0, keeps=0, empty=0, host_walk=0, sticks=0, fresh=0, release=0, behind_stale=0, repeats=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--case", type=int, default=None, help="replay this case of --seed as the run had it: the cases of its batch up to it, in one process")
    ap.add_argument("--kind", choices=fz.KINDS, default=None, help="draw this kind only")
    ap.add_argument("--max-voxels", type=int, default=60000)
    ap.add_argument("--max-rows", type=int, default=24)
    ap.add_argument("--batch-seconds", type=int, default=240, help="the time limit of one batch's process")
    args = ap.parse_args()
    options = dict(max_voxels=args.max_voxels, max_rows=args.max_rows, kind=args.kind)
    import __graft_entry__ as graft
    oracle = graft.load_oracle()
    oracle.build()
    if args.case is not None:
        first = args.case - args.case % BATCH
        recipes = [draw_case(args.seed, c, options) for c in range(first, args.case + 1)]
        print(json.dumps({"recipe": recipes[-1]}), flush=True)
        try:
            lines, _, _ = run_batch(oracle, recipes, args.batch_seconds)
        except AssertionError as e:
            print(json.dumps({"FAILED": recipes[-1], "error": str(e)[:3000]}), flush=True)
            return 1
        print(json.dumps({"identical": True, "cases": len(recipes), "lines": len(lines)}), flush=True)
        return 0
    t0 = last = time.time()
    stats, first = new_stats(), 0
    while time.time() - t0 < args.seconds:
        recipes = [draw_case(args.seed, c, options) for c in range(first, first + BATCH)]
        try:
            lines, refs, _ = run_batch(oracle, recipes, args.batch_seconds)
        except AssertionError as e:                       # the first failing batch ends the run: no retry
            print(json.dumps({"FAILED_BATCH": [first, first + BATCH], "seed": args.seed, "error": str(e)[:3000]}), flush=True)
            return 1
        tally(stats, lines, refs)
        first += BATCH
        if time.time() - last > 20:
            last = time.time()
            print("t %.0f s: %d cases in %d lines, paths %s, %d refusals, %d plain lines, all identical" % (
                last - t0, stats["cases"], stats["lines"], json.dumps(stats["paths"], sort_keys=True), sum(stats["refusals"].values()), stats["plain_lines"]), flush=True)
    stats.update(seconds=round(time.time() - t0, 1), seed=args.seed, options={k: v for k, v in options.items() if v is not None}, identical=True)
    print(json.dumps(stats, sort_keys=True), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
