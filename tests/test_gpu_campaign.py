"""A seeded slice of the differential campaign (tests/fuzz_campaign.py) in the GPU suite: one test per kind -- the whole volume
(with normals and repeats), cuberille_set_border, cuberille_set_region, cuberille_set_band, the B-spline walk -- each a fixed list
of (seed, case) pairs run in order on ONE context of the test's own, so that every case meets what the cases before it left
there: the launch sizes of another frame, a workspace sized for a padded grid or a box, a normals row that exists or not, the
pixel row and the component rows of a mesh of another view, pixel width or cell count.

The references are never the library: the oracle on the volume, on the padded copy, on the crop, on test_band.band_image; the
oracle's lattice points walked by the drop-in's host walk through ITK's B-spline class; normals_ref.normals at the reference's
points; cell_pixels_ref.cell_pixels on the view's frame before the band mapping; components_ref.components on the REFERENCE's
cells.  Comparisons are exact (conftest.assert_same_mesh, normals_ref.same_normals, the walk's counters equal, cell pixels and
the three component rows as bytes, K; a case that repeats runs its first repeat with cell pixels and components off, and that
mesh is byte for byte the last repeat's).

Cell pixels (cuberille_set_cell_pixels) are on where (i + i // 10) % 2 == 0, components (cuberille_set_components) where
i % 3 != 2, on every route that offers them (not the slabs); a count + emit case hands cuberille_emit the id offset its recipe
drew.  Per kind: at least 5 cases with each setting, quads and triangles with each, a case with both, at most a quarter of the
cases of each with an empty reference mesh, and (all but the B-spline) a components case with K = 1 and one with K >= 2.  Over
the whole slice: cell pixels of all ten pixel types; normals, cell pixels and components together; components on an empty mesh
(K = 0, null rows), on a mesh with a Q1 gap, with K > 64 (the slice reaches K = 311); a border whose ring is inside, a band
whose cells carry two raw values; a repeat, a refused call ahead and a development switch with each setting; a count + emit
components case with a non-zero id offset and one of 2^32 or more; a cell-pixel case and a components case on a context that
still holds the rows of a mesh of another size -- the rows the run met are held to the rows the recipes foretell.

Every components case keeps (cuberille_keep_components, recipe["keep"]): the rule is KEEP_RULES[(i // 2) % 3] -- largest,
min_cells, mask --, the pick, the mask's bytes and a second stage are drawn, every argument is resolved on the REFERENCE's counts,
and after each stage the library's counts, mesh (mesh_host() on the device route, download() elsewhere), normals, cell pixels,
rows, K, device pointers and counters are held to keep_ref.keep on the oracle's mesh and the references' rows -- nothing of it
is the library's.  In a repeating case the second extraction keeps too, and the third, launched blindly behind that keep, is
still the first one's mesh.  The context stays as the keep left it.  Per kind: at least 5 keep cases, quads and triangles among
them, at least 4 whose first stage keeps some of several (0 < K' < K; the B-spline slice, checked on the oracle and the host walk, has 6).  Over the whole
slice: each rule at least 3 times with 0 < K' < K; K' = 0 from K >= 1; K' = K >= 2 (nothing moves); a keep on an empty mesh;
with normals, with cell pixels, with both; with NaN coordinates or a NaN normal in the kept part (the slice offers several: the
border's cases 3, 4, 6, 10, 12, region 18, band 15); at K > 64 (K = 311, 110, 85 and 67); a count + emit keep with an id offset of 2^32
and more that drops something (region, case 7); in a repeating case; on the held route; under a development switch; behind a
refused call; chained; on a mask with bytes other than 0 and 1; and, for normals, cell pixels and components each, a case with
the setting on whose predecessor on the context ran a keep with 0 < K' < K and left that setting's row (behind_keep) -- the
cases that ran behind a keep, by what the library returned, are held to those the recipes foretell.

Case i of a kind takes pixel type DTYPES[i % 10] and the kind's routes in turn; everything else is drawn, and the seeds
(fuzz_campaign.SLICE) are the first for which the oracle alone shows the conditions of fuzz_campaign.slice_conditions: all ten pixel
types, every route at least twice, quads and triangles, projection on and off, the three geometry forms, a start index other
than 0 -- each form on a case whose vertices walk --, an empty slice between occupied ones (quirk Q1), a refusal ahead of a case
of every view kind, at most a quarter of the cases with an empty reference mesh; over the whole slice NaN coordinates, normals
with and without a NaN, a repeat (with normals too), and a normals case on a context that still holds the normals row of a mesh
of another size (a normals case leaves its row behind unless its recipe drops it).  tests/test_campaign_scripts.py asserts them
without a GPU; each test here asserts them again over the cases it executed, test_whole_slice_conditions those of all five kinds
together (it runs whatever kind has not run yet in this process, so it never passes for want of cases).

Volumes: the XS row lengths; a volume (of a region case: its box) has at most 12 rows and slices and at most 30 000 voxels.  A
region case's buffer is larger than its box by up to 16 + 8 voxels along x (up to 63 more where the buffer's rows are made
whole words round a ragged box) and 3 + 3 (one more below a box that spans x and y) along y and z: at most 19 rows and slices,
60 000 voxels.  Wall time of each test on an MI355X box (16 host
threads, the references included), pytest's own figures: whole volume 2.0 s (24 cases in 0.35 s; the rest is the first context of
the process loading the code objects), border 0.15 s, region 0.07 s, band 0.12 s, B-spline 0.31 s (20 cases each, the B-spline's
with one subprocess per projecting case).  With the keeps -- one or two per components case, every row downloaded a second time,
the numpy reference of a keep -- measured the same way: whole volume 2.06 s (24 cases in 0.34 s), border 0.15 s, region 0.07 s,
band 0.12 s, B-spline 0.30 s: what a keep adds is below the figures' last digit.
"""
import time

import numpy as np
import pytest

import fuzz_campaign as fz

pytestmark = pytest.mark.gpu

_FACTS = {}


def _run_slice(pkg, oracle, kind):
    """The facts of a kind's cases, executed once per process."""
    if kind in _FACTS:
        return _FACTS[kind]
    recipes = fz.slice_recipes(kind)
    contexts = fz.open_contexts(pkg)
    wants, rows, behind = [], [], []
    t0 = time.time()
    try:
        for recipe in recipes:
            try:
                got, want = fz.one_case(pkg, oracle, contexts, recipe)
            except AssertionError as e:
                raise AssertionError("seed %d case %d (%s %s %s): %s" % (recipe["seed"], recipe["case"], kind, recipe["dtype"], recipe["route"], e)) from e
            wants.append(want)
            n_points, n_cells = len(got["mesh"].points), len(got["mesh"].cells)
            rows.append((fz.meets_row_of_another_size(got["row_before"], recipe, n_points),
                         fz.meets_pixels_row_of_another_size(got["pixels_row_before"], recipe, n_cells),
                         fz.meets_components_row_of_another_size(got["components_row_before"], recipe, n_points, n_cells)))
            assert (got["cell_pixels"] is not None) == recipe["cell_pixels"] and (got["components"] is not None) == recipe["components"]
            # every components case keeps, every stage ran, and the case knows whether it ran behind a keep that moved the rows
            assert len(got["kept"]) == len(fz.keep_stages(recipe["keep"])) == len(want["kept"]) and bool(got["kept"]) == recipe["components"]
            behind.append(fz.behind_keep(got["keep_before"], (got["row_before"], got["pixels_row_before"], got["components_row_before"]), recipe))
    finally:
        fz.close_contexts(contexts)
    print("%s: %d cases in %.2f s" % (kind, len(wants), time.time() - t0))
    assert len(wants) == len(recipes) == fz.SLICE[kind][1]                 # no case is skipped
    facts = fz.slice_sequence_facts(recipes, wants)
    # the rows the run met -- normals, cell pixels, components -- are the rows the recipes foretell
    assert [(f["other_row"], f["other_pixels_row"], f["other_components_row"]) for f in facts] == rows
    # ... and so are the cases that ran behind a keep: what the library returned (K, K') against what the reference foretells
    assert [f["behind_keep"] for f in facts] == behind
    assert fz.slice_conditions(kind, facts) == []
    _FACTS[kind] = facts
    return facts


def test_whole_volume_slice(pkg, oracle):
    _run_slice(pkg, oracle, "whole")


def test_border_slice(pkg, oracle):
    _run_slice(pkg, oracle, "border")


def test_region_slice(pkg, oracle):
    _run_slice(pkg, oracle, "region")


def test_band_slice(pkg, oracle):
    _run_slice(pkg, oracle, "band")


def test_bspline_slice(pkg, oracle):
    _run_slice(pkg, oracle, "bspline")


def test_envelope_slice(pkg, oracle):
    """fuzz_campaign.py --envelope, a seeded slice: voxel scales of 2^-120 .. 2^126 (float32) and 2^-1000 .. 2^1000 (float64), spacing scales of 2^-100 .. 2^100, origins up
    to 1e9, start indices near +-2^30, on every kind and route in turn, each mesh (and the normals the case draws) equal to
    the references'.  Its conditions: tests/test_campaign_scripts.py."""
    recipes = fz.envelope_slice_recipes()
    assert len(recipes) == fz.ENVELOPE_SLICE[1] == 60 and all(r["envelope"] for r in recipes)
    contexts = fz.open_contexts(pkg)
    wants = []
    try:
        for recipe in recipes:
            try:
                got, want = fz.one_case(pkg, oracle, contexts, recipe)
            except AssertionError as e:
                raise AssertionError("seed %d case %d (%s %s %s, envelope %s): %s" % (recipe["seed"], recipe["case"], recipe["kind"], recipe["dtype"],
                                                                                      recipe["route"], recipe["envelope"], e)) from e
            wants.append(want)
    finally:
        fz.close_contexts(contexts)
    assert fz.envelope_slice_conditions(recipes, wants) == []


def test_whole_slice_conditions(pkg, oracle):
    """What the slice must hold over all five kinds together, over the cases executed (a kind that has not run yet in this
    process runs here)."""
    facts = [f for kind in fz.KINDS for f in _run_slice(pkg, oracle, kind)]
    assert len(facts) == sum(n for _, n in fz.SLICE.values())
    assert fz.slice_conditions_overall(facts) == []
