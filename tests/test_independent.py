"""The project's CPU sides held to witnesses that share nothing with them (tests/independent_ref.py: float64 numpy + scipy):
the oracle's mesh and the reference filter's (the binaries of oracle/_ref/ where they exist), the drop-in's host B-spline walk,
the B-spline classes and their restatement, the recursive-Gaussian restatement and the oracle's walk along that gradient, and
normals_ref -- every one of which was written from the same reading of ITK as the code it checks.

Tolerances are not chosen here: tests/golden/independent_tolerances.json records what the witnesses are from the reference
(make_independent_tolerances.py), every comparison allows independent_sides.FACTOR times that, on the vertices the witness
alone calls not fragile.  The conditions under which a case may be relied on are asserted here, from the witness alone."""
import ast
import importlib.util
import json
import os

import numpy as np
import pytest

import independent_ref as ind
import independent_sides as sides
import ref_filter as rf

CASES = ind.independent_cases()
BY_NAME = {c["name"]: c for c in CASES}


def _generator():
    path = os.path.join(rf.GOLDEN, "make_independent_tolerances.py")
    spec = importlib.util.spec_from_file_location("make_independent_tolerances", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def measured(tmp_path_factory, oracle):
    """Everything the generator measures, measured again here, once."""
    return _generator().measure(tmp_path_factory.mktemp("independent"), strict=False)


def test_the_witnesses_import_nothing_of_the_project():
    with open(ind.__file__) as f:
        tree = ast.parse(f.read())
    roots = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            roots |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            assert node.level == 0, "a relative import"
            roots.add(node.module.split(".")[0])
        elif isinstance(node, ast.Call) and getattr(node.func, "id", "") in ("__import__", "exec", "eval"):
            raise AssertionError("an import that the import list does not show")
    assert roots and roots <= {"numpy", "scipy", "math", "mpmath"}, roots
    assert "importlib" not in roots


def test_the_case_list_covers_what_it_is_meant_to():
    names = [c["name"] for c in CASES]
    assert len(names) == len(set(names))
    assert {c["vox"].dtype.name for c in CASES} >= {"uint8", "int16", "float32", "float64"}
    assert {c["geometry_name"] for c in CASES} == set(ind.GEOMETRIES)
    assert {c["variant"] for c in CASES} == {0, 1, 2}
    assert {c["interp"] for c in CASES} == {"linear", "bspline32", "bspline64"}
    assert {c["gradient"] for c in CASES} == {0, 1}
    assert {c["view"]["kind"] for c in CASES if c["view"]} == {"border", "region", "band"}
    assert {r for c in CASES for r in c["reach"]} == {ind.THRESHOLD, ind.STEPS, ind.SWAPS, ind.SEARCH}
    for c in CASES:
        vox, _ = ind.materialised(c)
        assert np.abs(vox.astype(np.float64) - c["iso"]).max() < ind.LINESEARCH_START, c["name"]
        assert min(vox.shape) >= 4 and c["step"] > 0, c["name"]
        assert len(sides_start(c)) <= 4000, c["name"]


_STARTS = {}


def sides_start(case):
    import __graft_entry__ as graft
    if case["name"] not in _STARTS:
        _STARTS[case["name"]] = sides.start_points(graft.load_oracle(), case)
    return _STARTS[case["name"]]


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_case_conditions_hold_by_the_witness_alone(name):
    """At most a tenth of the vertices fragile, a wave's worth left, every stop reason the case is meant to reach reached by
    eight vertices that are not fragile; and the start points are where ITK's index transform puts the lattice."""
    case = BY_NAME[name]
    start = sides_start(case)
    wit, walk, fragile = sides.witnessed(case, start)
    assert ind.case_conditions(walk, fragile, case) is None, ind.case_conditions(walk, fragile, case)
    # float vertices: half a unit in the last place of the largest coordinate, in voxels
    eps = 2.0 ** -24 * max(1.0, float(np.abs(start).max())) / float(wit.img.spacing.min())
    assert wit.img.lattice_residual(start).max() <= 4.0 * eps, name
    assert wit.img.face_distance(start.astype(np.float64)).min() >= 1.0, name


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_reference_walk_against_the_witness(measured, name):
    """The reference binary's vertices (the oracle's where there is none; the host walk's for the B-spline)."""
    row = measured["cases"][name]
    print(name, row)
    assert row["voxels"] <= sides.allowed(row["family"]), (name, row)
    if "radians" in row:
        assert row["radians"] <= sides.allowed("normals_angle"), (name, row)       # normals_ref.normals


@pytest.mark.parametrize("name", sorted(n for n, c in BY_NAME.items() if c["interp"] == "linear"))
def test_oracle_walk_and_counters_against_the_witness(oracle, name):
    """The oracle's own mesh whatever binaries exist, and its stop counters: the stops by threshold lie in [T, T + F] and those
    by the step count in [S, S + F], T and S the witness's on the vertices that are not fragile, F the fragile ones."""
    case = BY_NAME[name]
    start = sides_start(case)
    wit, walk, fragile = sides.witnessed(case, start)
    vox, _ = ind.materialised(case)
    m = oracle.run(vox, case["iso"], triangles=0, project=1, variant=case["variant"], gradient=case["gradient"],
                   **dict(sides.walk_kw(case), **sides.geometry_of(case)))
    dev = wit.img.voxels_between(m.points, walk.points)[~fragile]
    print(name, "oracle: %.3g voxels over %d of %d vertices" % (dev.max(), (~fragile).sum(), len(fragile)))
    assert dev.max() <= sides.allowed(sides.family_of(case)), name
    if case["variant"] != 2:
        F = int(fragile.sum())
        T, S = walk.count(ind.THRESHOLD, ~fragile), walk.count(ind.STEPS, ~fragile)
        assert T <= m.info["proj_stop_threshold"] <= T + F, (name, T, F, m.info)
        assert S <= m.info["proj_stop_steps"] <= S + F, (name, S, F, m.info)


@pytest.mark.parametrize("family", ["coefficients_32", "coefficients_64", "bspline_evaluate_32", "bspline_evaluate_64", "gaussian_gradient"])
def test_bspline_classes_and_gaussian_restatement_against_scipy(measured, family):
    """`bspline_walk coeffs` / `eval` (the host classes) and bspline_ref against spline_filter / map_coordinates, at points
    outside the buffer too; restate.recursive_gaussian_gradient against the sampled Gaussian derivative, four sigma from the
    faces."""
    print(family, measured["families"][family])
    assert measured["families"][family] <= sides.allowed(family)


def test_recorded_tolerances_are_what_this_machine_measures(measured):
    """Neither side of the file is stale: what is measured here lies within FACTOR of what is recorded, both ways; and no
    position family (the Gaussian walk apart) is recorded beyond 1e-3 voxel."""
    with open(sides.TOLERANCES) as f:
        recorded = json.load(f)
    assert sorted(recorded["families"]) == sorted(measured["families"])
    assert sorted(recorded["cases"]) == sorted(measured["cases"]) == sorted(BY_NAME)
    for family, value in recorded["families"].items():
        got = measured["families"][family]
        assert got <= sides.FACTOR * value and value <= sides.FACTOR * got, (family, value, got)
        if family.endswith(("_v0", "_v1", "_v2", "walk_32", "walk_64")):
            assert value <= 1.0e-3, family


def test_zero_gradient_gives_no_normal_in_the_witness_either(oracle):
    """The two sheets (quirk Q4): on the faces that look at each other the witness gradient is exactly zero at the lattice
    points away from the sheets' edges, and normals_ref gives NaN exactly there."""
    import normals_ref
    vox = ind.two_sheets()
    pts = oracle.run(vox, 100, triangles=0, project=0).points
    img = ind.Image(vox)
    _, norm = ind.normal_function(img, ind.central_gradient(img))(pts.astype(np.float64))
    zero = norm == 0.0
    assert 8 <= zero.sum() < len(pts)
    got = normals_ref.normals(oracle, vox, pts)
    assert np.array_equal(np.isnan(got).any(axis=1), zero)
