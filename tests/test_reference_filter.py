"""The oracle against the REFERENCE's own filter code: oracle/_ref/ref_filter* are the reference's
itkCuberilleImageToMeshFilter.{h,txx}, compiled unchanged (oracle/Makefile, target `ref`) against ITK-lite's host section,
around a driver of our own (oracle/ref_filter_main.cxx).  Every comparison is bit for bit: the same counts, ids, order, cells
and float coordinates (NaN compared as NaN); there is no tolerance anywhere.

This pins the FILTER -- traversal, lookup maps, id assignment, cell order, the split rule, casts and promotions, the control
flow of all three walk branches -- not ITK: the ITK primitives underneath (interpolation, gradient, transforms) are our own on
both sides.

The direct tests skip only where oracle/_ref/ref_filter does not exist (no reference tree at build time);
test_oracle_matches_recorded_reference_results then still holds the oracle to what the binary produced where it does exist
(tests/golden/reference_filter_digests.json, written by tests/golden/make_reference_filter_digests.py from the binary alone).
"""
import json

import numpy as np
import pytest

import ref_filter as rf

needs_binary = pytest.mark.skipif(not rf.available(0), reason="oracle/_ref/ref_filter is not built (no reference tree at build time)")


def _hold(oracle, case):
    points, cells = rf.run_oracle(oracle, case)
    rpoints, rcells = rf.run_reference(case)
    if not rf.points_defined(case):
        assert not case["triangles"], case["name"]
        assert points.shape == rpoints.shape and np.array_equal(cells, rcells), case["name"]
        return rpoints, rcells
    diff = rf.difference_outside(rf.undefined_vertices(case), points, cells, rpoints, rcells)
    assert diff is None, "%s: %s" % (case["name"], diff)
    return rpoints, rcells


def _check_row(case, row, rpoints, rcells):
    d = rf.digest(rpoints, rcells)
    assert (d["points"], d["cells"]) == (row["points"], row["cells"]), case["name"]
    assert d["points_sha256"] == row["points_sha256"] and d["cells_sha256"] == row["cells_sha256"], case["name"]


@needs_binary
def test_all_three_binaries_are_built():
    assert all(rf.available(v) for v in (0, 1, 2))


@needs_binary
def test_ctest_table_through_the_reference_filter(oracle):
    """The 19 rows of the reference's CTest table, each volume with its own geometry: the counts the table asserts, and the
    oracle's mesh equal to the reference filter's."""
    cases = rf.ctest_cases()
    rows = rf._rows("ctest_cases.json")
    assert len(cases) == len(rows) == 19
    for case, row in zip(cases, rows):
        rpoints, rcells = _hold(oracle, case)
        assert (len(rpoints), len(rcells)) == (row["points"], row["cells"]), case["name"]


@needs_binary
def test_mesh_digests_reproduced_by_the_reference_filter(oracle):
    """Every row of mesh_digests.json -- the oracle's frozen output -- reproduced by the reference binary."""
    cases = rf.mesh_digest_cases()
    assert len(cases) == 44
    for case, row in cases:
        _check_row(case, row, *rf.run_reference(case))


@needs_binary
def test_later_update_digests_reproduced_by_the_reference_filter(oracle):
    """later_update_digests.json: the start-index rows, and the Q3 rows as a real second Update() of one filter object."""
    cases = rf.later_update_cases()
    assert len(cases) == 22 and sum(1 for c, _ in cases if c["first"]) == 11
    for case, row in cases:
        _check_row(case, row, *rf.run_reference(case))


@needs_binary
def test_variant_digests_reproduced_by_the_switched_reference_filters(oracle):
    """The gradient == 0 rows of variant_digests.json through ref_filter_advanced and ref_filter_linesearch."""
    cases = rf.variant_cases()
    assert len(cases) == 22 and sorted({c["variant"] for c, _ in cases}) == [1, 2]
    undefined = []
    for case, row in cases:
        rpoints, rcells = _hold(oracle, case)
        mask = rf.undefined_vertices(case)
        if mask is not None and mask.any():
            # the oracle's frozen row keeps such a vertex where it started; the reference's bytes there are not defined: the row
            # is held to the reference outside those vertices (_hold above), and its counts
            assert (len(rpoints), len(rcells)) == (row["points"], row["cells"])
            undefined.append(case["name"])
        else:
            _check_row(case, row, rpoints, rcells)
    assert undefined == rf.UNDEFINED_VARIANT_ROWS           # one row: blob3's line search meets a zero gradient


GROUPS = [("pixel_type_cases", 50), ("cast_cases", 55), ("geometry_cases", 36), ("quirk_cases", 50), ("walk_cases", 45), ("border_cases", 12),
          ("envelope_magnitude_cases", 120), ("envelope_span_cases", 25), ("envelope_geometry_cases", 125), ("envelope_pad_cases", 9),
          ("envelope_band_cases", 11)]


@needs_binary
@pytest.mark.parametrize("group,count", GROUPS)
def test_oracle_against_the_reference_filter(oracle, group, count):
    cases = getattr(rf, group)()
    assert len(cases) == count and len({c["name"] for c in cases}) == count
    for case in cases:
        _hold(oracle, case)


def test_case_lists_cover_what_they_claim():
    types = rf.pixel_type_cases()
    assert {(c["volume"]["dtype"], c["triangles"], c["project"]) for c in types[:40]} == {(d, t, p) for d in rf.DTYPES for t in (0, 1) for p in (0, 1)}
    shapes = {tuple(c["volume"]["shape"]) for c in types}
    assert {(1, 9, 8), (2, 7, 9), (5, 4, 63), (3, 5, 64), (4, 3, 65), (130, 9, 7)} <= shapes
    assert {c["variant"] for c in rf.geometry_cases()} == {c["variant"] for c in rf.walk_cases()} == {0, 1, 2}
    assert {c["max_steps"] for c in rf.walk_cases()} >= {0, 1, 3} and {c["relax"] for c in rf.walk_cases()} >= {1.0, 0.5}
    assert any(c["first"] and c["step"] < 0 for c in rf.walk_cases())
    assert all(c["pad"] for c in rf.border_cases())
    # the envelope: every family on both switched branches, the line search only where the reference defines it -- on the inputs
    env = rf.envelope_cases()
    assert [g for g, _ in GROUPS[-5:]] == rf.ENVELOPE_GROUPS and sum(n for _, n in GROUPS[-5:]) == len(env)
    assert rf.synthetic_cases()[-len(env):] == env                      # appended: the earlier rows of the digest file keep their place
    families = {}
    for c in env:
        families.setdefault(rf.envelope_family(c), set()).add(c["variant"])
        assert c["triangles"] == 1 and rf.points_defined(c) and c["max_steps"] == 8 and c["threshold"] in (0.0, 0.01), c["name"]
        assert tuple(c["volume"]["shape"]) == ((7, 8, 9) if c["volume"]["kind"] == "field" else (6, 7, 9)), c["name"]
        if c["variant"] == 2:
            assert rf.linesearch_defined(c), c["name"]
    assert families == dict({f: {0, 1, 2} for f in ("magnitude", "span", "spacing", "origin", "start", "step", "shear", "relax_0")}, pad={0}, band={0})
    large = [c for c in env if c["variant"] != 2 and rf.envelope_family(c) in ("magnitude", "span") and not rf.linesearch_defined(c)]
    assert len(large) >= 2 * (6 * 3 + 5 * 2 + 6 * 2)                     # what the rule keeps from the line search runs the other two
    whole = {c["volume"]["dtype"]: rf.case_inputs(c)[0] for c in rf.envelope_span_cases() if c["volume"].get("whole")}
    assert sorted(whole) == ["int16", "int32", "int64", "uint16", "uint32", "uint64"]
    for dt, vox in whole.items():                                       # the whole range of the type: both top bits drawn, uint64's too
        info = np.iinfo(dt)
        assert int(vox.max()) > info.max - (info.max - info.min) // 16 and int(vox.min()) < info.min + (info.max - info.min) // 16, dt
    starts = {tuple(c["geometry"]["start"]) for c in env if rf.envelope_family(c) == "start"}
    assert starts == {tuple(s) for s in rf.ENV_STARTS} and max(abs(v) for s in starts for v in s) == 1 << 30
    bs = rf.bspline_envelope_cases()
    assert len(bs) == 20 and {c["interp"] for c in bs} == {"bspline_f", "bspline_d"} and len({c["name"] for c in bs}) == 20


def test_envelope_magnitude_families_are_mixed():
    """A family whose vertices are all finite or all NaN says little: from the reference's recorded output alone
    (tests/golden/envelope_finite_vertices.json, written with the digests from the binary) each magnitude family has a case whose
    share of finite vertices lies strictly between 5 % and 95 %."""
    with open(rf.ENVELOPE_FINITE) as f:
        recorded = json.load(f)
    names = [c["name"] for c in rf.envelope_cases() + rf.bspline_envelope_cases()]
    assert sorted(recorded) == sorted(rf.ENV_MIXED_FAMILIES)
    for family in rf.ENV_MIXED_FAMILIES:
        assert sorted(family + rest for rest in recorded[family]) == sorted(n for n in names if n.startswith(family)), family
        shares = {rest: finite / points for rest, (finite, points) in recorded[family].items()}
        assert shares and any(0.05 < s < 0.95 for s in shares.values()), (family, shares)


@needs_binary
def test_envelope_finite_vertices_are_the_reference_filters():
    with open(rf.ENVELOPE_FINITE) as f:
        recorded = json.load(f)
    again = {}
    for case in rf.envelope_magnitude_cases() + rf.bspline_envelope_cases():
        rf.note_finite(again, case, rf.run_reference(case)[0])
    assert again == recorded


@needs_binary
def test_bspline_instantiations_against_the_host_walk(tmp_path):
    """The reference filter instantiated with BSplineInterpolateImageFunction<Image, float, float> / <..., double, double>
    (order 3, as its driver writes it) against the drop-in's host walk -- HostGradient + HostWalk of
    itkCuberilleImageToMeshFilter.txx through the same interpolator class, run by itk/tests/bspline_walk.cxx without a GPU --
    from the reference's own unprojected vertices: every walked vertex bit for bit, and the triangles the reference makes of
    them equal to the split rule applied to those vertices."""
    cases = rf.bspline_cases()
    assert len(cases) == 9
    _bspline_host_walk(tmp_path, cases)


@needs_binary
def test_bspline_envelope_against_the_host_walk(tmp_path):
    """The same at the edges of the number range (ref_filter.bspline_envelope_cases)."""
    cases = rf.bspline_envelope_cases()
    assert len(cases) == 20
    # (at an origin of 1e7 or a start index of 2^30 a float32 coordinate's last place is 1 or 128, a step of 0.2 is below it:
    # those walks may leave every vertex where it started)
    _bspline_host_walk(tmp_path, cases, moved=lambda case: "/spacing" in case["name"] or "/magnitude" in case["name"])


def _bspline_host_walk(tmp_path, cases, moved=lambda case: True):
    import subprocess
    from bspline_ref import geometry_arg, walk_exe
    for n, case in enumerate(cases):
        vox, geo, _ = rf.case_inputs(case)
        assert vox.dtype in (np.uint8, np.float32, np.float64)
        start, quads = rf.run_reference(dict(case, interp="linear", project=0, triangles=0))
        rpoints, rquads = rf.run_reference(dict(case, triangles=0))
        assert np.array_equal(quads, rquads) and len(start) == len(rpoints) > 0, case["name"]
        thr, step, relax = rf.effective(case, vox)
        raw, sp, op = (str(tmp_path / ("%s%d.raw" % (k, n))) for k in "vso")
        vox.tofile(raw)
        start.astype("<f4").tofile(sp)
        nz, ny, nx = vox.shape
        r = subprocess.run([walk_exe(), "walk", raw, rf.PIXEL_NAMES[vox.dtype], str(nx), str(ny), str(nz), "32" if case["interp"] == "bspline_f" else "64",
                            geometry_arg(geo["spacing"], geo["origin"], np.asarray(geo["direction"]).reshape(3, 3), geo["start"]),
                            repr(float(case["iso"])), repr(thr), repr(step), repr(relax), str(case["max_steps"]), sp, str(len(start)), op],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (case["name"], r.stdout, r.stderr)
        got = np.fromfile(op, dtype="<f4").reshape(-1, 3)
        diff = rf.first_difference(got, quads, rpoints, rquads)
        assert diff is None, "%s: %s" % (case["name"], diff)
        assert not moved(case) or not np.array_equal(got, start), case["name"]  # the walk moved them
        tpoints, tcells = rf.run_reference(dict(case, triangles=1))
        diff = rf.first_difference(got, rf.split_quads(got, quads), tpoints, tcells)
        assert diff is None, "%s (triangles): %s" % (case["name"], diff)


def test_oracle_matches_recorded_reference_results(oracle):
    """tests/golden/reference_filter_digests.json: what the REFERENCE binary produced, per case; needs no binary.  Where the
    line search leaves vertices undefined the file names them (found from the reference itself, ref_filter.undefined_vertices)
    and its digests leave them out (ref_filter.masked); everything else of such a mesh is held like any other."""
    with open(rf.DIGESTS) as f:
        rows = json.load(f)
    cases = rf.recorded_cases()
    assert len(rows) == len(cases) == 19 + sum(n for _, n in GROUPS)
    undefined = []
    for case, row in zip(cases, rows):
        assert row["case"] == case, case["name"]            # the file describes the case it was made from
        points, cells = rf.run_oracle(oracle, case)
        assert (len(points), len(cells)) == (row["points"], row["cells"]), case["name"]
        mask = np.zeros(len(points), dtype=bool)
        mask[row["undefined_vertices"]] = True
        if mask.any():
            undefined.append(case["name"])
        d = rf.digest(*rf.masked(mask, points, cells))
        assert d["cells_sha256"] == row["cells_sha256"], case["name"]
        if rf.points_defined(case):
            assert d["points_sha256"] == row["points_sha256"], case["name"]
        else:
            assert not case["triangles"] and row["points_sha256"] is None, case["name"]
    assert undefined == RECORDED_WITH_UNDEFINED_VERTICES


# the recorded cases whose line search meets a zero gradient somewhere (their rows list the vertices)
RECORDED_WITH_UNDEFINED_VERTICES = []
