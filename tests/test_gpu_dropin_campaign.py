"""A seeded slice of the differential campaign through the C++ drop-in filter (tests/fuzz_dropin.py) in the GPU suite: one test
per kind -- the whole volume, PadBorderOn, SetExtractionRegion, InsideBandOn, the B-spline interpolator --, each ONE script of 20
cases run in order by ONE process of midas-journal-740_amd/itk/build/fuzz_update, which keeps one itk::CuberilleImageToMeshFilter
object per (pixel type, interpolator type, mesh traits) alive and reuses it for every line that names the triple: each Update()
meets what the updates before left on the object -- a context or a group, a held gradient, a view, the three attribute switches,
vectors of another mesh, a cell-data container, the sticky step length.

The references are never the library: fuzz_campaign.expected() (the oracle on the volume, the padded copy, the crop, the band
image; its first= run for the stale gradient; its lattice points walked through ITK-lite's B-spline class; normals_ref,
cell_pixels_ref, components_ref, keep_ref on the oracle's own mesh), handed the step length the object holds by then.  What the
binary read back through the mesh's public API -- GetPoint, GetCell / PointIdsBegin with each cell's arity, GetCellData or the
missing container -- and the filter's accessors, GetLastNumberOfSlabs() and GetProjectVertexStepLength() are compared exactly:
conftest.assert_same_mesh, normals_ref.same_normals, bytes for every other row, no tolerance anywhere.  The host walk through an
interpolator that inherits the linear one's Evaluate() is held to the SAME oracle mesh as the device walk, bit for bit.

A case is up to four lines: a refused combination first (fuzz_dropin.REFUSALS: the message must hold the refusal's words, and
the mesh and every accessor must be empty, the header's rule for a throwing Update()), a plain line with every switch off ahead,
the case, a plain line behind.  Case i takes pixel type DTYPES[i % 10]; fuzz_dropin.slice_options fixes the path, the refusal, the
plain lines, fresh objects, eager setup, release and the sticky step by rules of i, everything else is drawn, and the seeds
(fuzz_dropin.SLICE) are the first for which the oracle alone shows fuzz_dropin.slice_conditions: all ten pixel types on the device
path and on the host-walk path (every one of those walks); each path at least four times; groups of 2, 3 and 8 members, one with
fewer slices than members; the host walk on a rotated geometry, a start index other than 0, 64-bit pixels beyond 2^53, a surface
at the image border, and with cell pixels and components on triangles (its doubling); quads and triangles, projection on and off,
dynamic traits with cell data; a default step length that sticks on an image of another largest spacing; every switch on in one
line and off in the next of the same object with the accessors empty; an object that goes single, group, single; stale followed
by non-stale; a fresh object with eager setup off; release-host-mesh followed by another update; every refusal of the table, each
followed by a full case on its object; a keep that drops something, one that leaves nothing, one with normals and cell data; three
updates in a row; at most a quarter of a kind's cases with an empty reference mesh.  tests/test_campaign_scripts.py asserts them
without a GPU; test_dropin_slice_conditions asserts them again over the lines the five processes executed (a kind that has not
run yet in this process runs there, so it never passes for want of cases).  No case is skipped; a missing binary is built by
make, and a failure of that fails the test.

Volumes: the C ABI slice's sizes (fuzz_campaign.SLICE_OPTIONS: at most 12 rows and slices, 30 000 voxels; a region's buffer up to
19 rows and slices, 60 000 voxels).  Wall time of each test on an MI355X box (the references included), pytest's own
figures: whole volume 1.03 s (20 cases in 58 lines, the process 0.89 s), border 0.88 s (47 lines, the process 0.58 s), region
0.67 s (47 lines, 0.55 s), band 0.65 s (47 lines, 0.47 s), B-spline 0.98 s (48 lines, 0.37 s; the rest is the host walk of the
reference, one subprocess per projecting case); the conditions over all five 0.00 s when the kinds have run.
"""
import pytest

import fuzz_campaign as fz
import fuzz_dropin as fd

pytestmark = pytest.mark.gpu

_FACTS = {}


def _run_slice(oracle, kind):
    """The facts of a kind's lines, executed once per process."""
    if kind in _FACTS:
        return _FACTS[kind]
    recipes = fd.slice_recipes(kind)
    lines, refs, wall = fd.run_batch(oracle, recipes, seconds=120)
    print("%s: %d cases, %d lines, the process took %.2f s" % (kind, len(recipes), len(lines), wall))
    facts = fd.slice_facts(lines, refs)
    assert len(recipes) == fd.SLICE_CASES == sum(f["sub"] == "main" for f in facts)              # no case is skipped
    _FACTS[kind] = facts
    return facts


def test_whole_volume_slice(pkg, oracle):
    _run_slice(oracle, "whole")


def test_border_slice(pkg, oracle):
    _run_slice(oracle, "border")


def test_region_slice(pkg, oracle):
    _run_slice(oracle, "region")


def test_band_slice(pkg, oracle):
    _run_slice(oracle, "band")


def test_bspline_slice(pkg, oracle):
    _run_slice(oracle, "bspline")


def test_dropin_slice_conditions(pkg, oracle):
    """What the slice must hold over all five kinds together, over the lines executed."""
    facts = [f for kind in fz.KINDS for f in _run_slice(oracle, kind)]
    assert fd.slice_conditions(facts) == []
