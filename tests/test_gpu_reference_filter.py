"""The HIP path against the REFERENCE's own filter code, directly: Extractor meshes against what oracle/_ref/ref_filter*
(the reference's itkCuberilleImageToMeshFilter.{h,txx} compiled unchanged, see tests/ref_filter.py) produce for the same case
lists as tests/test_reference_filter.py -- every pixel type, geometry, quirk, both switched projection branches, the
B-spline device walk, cuberille_hold_gradient against a real second Update(), cuberille_set_border against the
pad-then-filter recipe -- bit for bit.  Reads only oracle/_ref/ binaries and tests/golden/; where the binaries did not travel
the direct tests skip and test_hip_matches_recorded_reference_results still holds the HIP path to the recorded results."""
import json

import numpy as np
import pytest

import ref_filter as rf
from test_reference_filter import GROUPS, RECORDED_WITH_UNDEFINED_VERTICES

pytestmark = pytest.mark.gpu

needs_binary = pytest.mark.skipif(not rf.available(0), reason="oracle/_ref/ref_filter is not built (no reference tree at build time)")


@pytest.fixture()
def ex(pkg):
    pkg._abi.build()
    e = pkg.Extractor(0)
    yield e
    e.close()


def run_hip(pkg, ex, case):
    vox, geo, first = rf.case_inputs(case)
    thr, step, relax = rf.effective(case, vox)          # (a negative step goes to the library as it is)
    prm = pkg.make_params(rf.iso_of(case), case["triangles"], case["project"], thr, step, relax, case["max_steps"], variant=case.get("variant", 0))
    vol = lambda v, g: pkg.Volume(v, g["spacing"], g["origin"], np.asarray(g["direction"]).reshape(3, 3), g["start"])
    bits = {"linear": None, "bspline_f": 32, "bspline_d": 64}[case.get("interp", "linear")]
    try:
        if bits:
            ex.set_interpolator(pkg._abi.INTERP_BSPLINE, 3, bits, bits)
        ex.set_border(1 if case.get("pad") else 0, 0)
        if first:
            ex.hold_gradient(True)
            ex.extract_host(vol(*first), prm)               # the filter object's first Update()
        ex.extract_host(vol(vox, geo), prm)
        mesh = ex.download()
        return mesh.points, mesh.cells
    finally:
        ex.hold_gradient(False)
        ex.set_border(0, 0)
        ex.set_interpolator(pkg._abi.INTERP_LINEAR)


def _hold(pkg, oracle, ex, case):
    points, cells = run_hip(pkg, ex, case)
    rpoints, rcells = rf.run_reference(case)
    if not rf.points_defined(case):
        assert not case["triangles"], case["name"]
        assert points.shape == rpoints.shape and np.array_equal(cells, rcells), case["name"]
        return
    diff = rf.difference_outside(rf.undefined_vertices(case), points, cells, rpoints, rcells)
    assert diff is None, "%s: %s" % (case["name"], diff)


@needs_binary
def test_data_volumes_against_the_reference_filter(pkg, oracle, ex):
    """The CTest table, the rows of mesh_digests.json, the start-index and Q3 rows of later_update_digests.json (hold_gradient
    against a real second Update()) and the switched branches on every Data volume."""
    cases = rf.ctest_cases() + [c for c, _ in rf.mesh_digest_cases() + rf.later_update_cases() + rf.variant_cases()]
    assert len(cases) == 19 + 44 + 22 + 22
    for case in cases:
        _hold(pkg, oracle, ex, case)


@needs_binary
@pytest.mark.parametrize("group,count", GROUPS)
def test_hip_against_the_reference_filter(pkg, oracle, ex, group, count):
    cases = getattr(rf, group)()
    assert len(cases) == count
    for case in cases:
        _hold(pkg, oracle, ex, case)


@needs_binary
def test_bspline_device_walk_against_the_reference_filter(pkg, oracle, ex):
    cases = rf.bspline_cases()
    assert len(cases) == 9
    for case in cases:
        points, cells = run_hip(pkg, ex, case)
        diff = rf.first_difference(points, cells, *rf.run_reference(case))
        assert diff is None, "%s: %s" % (case["name"], diff)


@needs_binary
def test_bspline_envelope_device_walk_against_the_reference_filter(pkg, oracle, ex):
    """The B-spline device walk at the edges of the number range (ref_filter.bspline_envelope_cases): an origin of 1e7, a start
    index at +-2^30, spacings of 1e-4 and 1e4, voxels from 1e-30 up to where the coefficients overflow."""
    cases = rf.bspline_envelope_cases()
    assert len(cases) == 20
    for case in cases:
        points, cells = run_hip(pkg, ex, case)
        diff = rf.first_difference(points, cells, *rf.run_reference(case))
        assert diff is None, "%s: %s" % (case["name"], diff)


def test_bspline_envelope_matches_recorded_reference_results(pkg, oracle, ex):
    """tests/golden/envelope_bspline_digests.json alone, where the binaries did not travel."""
    with open(rf.BSPLINE_DIGESTS) as f:
        rows = json.load(f)
    cases = rf.bspline_envelope_cases()
    assert len(rows) == len(cases) == 20
    for case, row in zip(cases, rows):
        assert row["case"] == case, case["name"]
        d = rf.digest(*run_hip(pkg, ex, case))
        assert {k: d[k] for k in d} == {k: row[k] for k in d}, case["name"]


def test_hip_matches_recorded_reference_results(pkg, oracle, ex):
    """tests/golden/reference_filter_digests.json alone: meaningful where the binaries did not travel."""
    with open(rf.DIGESTS) as f:
        rows = json.load(f)
    cases = rf.recorded_cases()
    assert len(rows) == len(cases) == 19 + sum(n for _, n in GROUPS)
    undefined = []
    for case, row in zip(cases, rows):
        assert row["case"] == case, case["name"]
        points, cells = run_hip(pkg, ex, case)
        assert (len(points), len(cells)) == (row["points"], row["cells"]), case["name"]
        mask = np.zeros(len(points), dtype=bool)
        mask[row["undefined_vertices"]] = True              # named by the file, found from the reference (ref_filter.undefined_vertices)
        if mask.any():
            undefined.append(case["name"])
        d = rf.digest(*rf.masked(mask, points, cells))
        assert d["cells_sha256"] == row["cells_sha256"], case["name"]
        if rf.points_defined(case):
            assert d["points_sha256"] == row["points_sha256"], case["name"]
        else:
            assert not case["triangles"], case["name"]
    assert undefined == RECORDED_WITH_UNDEFINED_VERTICES
