"""A seeded slice of the differential campaign (tests/fuzz_campaign.py) in the GPU suite: one test per kind -- the whole volume
(with normals and repeats), cuberille_set_border, cuberille_set_region, cuberille_set_band, the B-spline walk -- each a fixed list
of (seed, case) pairs run in order on ONE context of the test's own, so that every case meets what the cases before it left
there: the launch sizes of another frame, a workspace sized for a padded grid or a box, a normals row that exists or not.

The references are never the library: the oracle on the volume, on the padded copy, on the crop, on test_band.band_image; the
oracle's lattice points walked by the drop-in's host walk through ITK's B-spline class; normals_ref.normals at the reference's
points.  Comparisons are exact (conftest.assert_same_mesh, normals_ref.same_normals, the walk's counters equal).

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
threads, the references included), pytest's own figures: whole volume 1.9 s (24 cases in 0.14 s; the rest is the first context of
the process loading the code objects), border 0.24 s, region 0.14 s, band 0.12 s, B-spline 0.36 s (20 cases each, the B-spline's
with one subprocess per projecting case).
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
    wants, rows = [], []
    t0 = time.time()
    try:
        for recipe in recipes:
            try:
                got, want = fz.one_case(pkg, oracle, contexts, recipe)
            except AssertionError as e:
                raise AssertionError("seed %d case %d (%s %s %s): %s" % (recipe["seed"], recipe["case"], kind, recipe["dtype"], recipe["route"], e)) from e
            wants.append(want)
            rows.append(fz.meets_row_of_another_size(got["row_before"], recipe, len(got["mesh"].points)))
    finally:
        fz.close_contexts(contexts)
    print("%s: %d cases in %.2f s" % (kind, len(wants), time.time() - t0))
    assert len(wants) == len(recipes) == fz.SLICE[kind][1]                 # no case is skipped
    facts = fz.slice_sequence_facts(recipes, wants)
    assert [f["other_row"] for f in facts] == rows                         # the rows the run met are the rows the recipes foretell
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


def test_whole_slice_conditions(pkg, oracle):
    """What the slice must hold over all five kinds together, over the cases executed (a kind that has not run yet in this
    process runs here)."""
    facts = [f for kind in fz.KINDS for f in _run_slice(pkg, oracle, kind)]
    assert len(facts) == sum(n for _, n in fz.SLICE.values())
    assert fz.slice_conditions_overall(facts) == []
