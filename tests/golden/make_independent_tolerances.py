"""Writes tests/golden/independent_tolerances.json: how far the witnesses of tests/independent_ref.py (float64 numpy + scipy,
nothing of the project's) are from the REFERENCE on this CPU -- the reference filter's binaries where oracle/_ref/ holds them,
else the oracle, which tests/test_reference_filter.py holds to them bit for bit; for the B-spline and the recursive Gaussian
the host classes and the restatements.  Never from GPU output.

Per family the largest deviation over the vertices that are not fragile (independent_ref.Witness.fragility, from the witness
alone):
    linear_walk_v0 / _v1 / _v2     final vertices, voxels, per branch of the walk
    bspline_walk_32 / _64          final vertices, voxels, per coefficient type
    gaussian_walk                  final vertices, voxels (carries the recursion's approximation of the Gaussian)
    normals_angle                  radians between the normals at the final vertices
    coefficients_32 / _64          the coefficient image, as a share of the largest coefficient
    bspline_evaluate_32 / _64      the interpolated value, as a share of the largest
    gaussian_gradient              the recursion against the sampled Gaussian derivative, as a share of the largest gradient
The tests allow independent_sides.FACTOR times these.  A walk family (the Gaussian one apart) beyond 1e-3 voxel means that a
witness or the fragility rule is wrong: the script stops there instead of recording it."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import __graft_entry__ as graft  # noqa: E402
import bspline_ref  # noqa: E402
import independent_ref as ind  # noqa: E402
import independent_sides as sides  # noqa: E402
import normals_ref  # noqa: E402
import restate  # noqa: E402

POSITION_LIMIT = 1.0e-3          # voxels
COEFFICIENT_PIXELS = ["uint8", "int16", "int32", "float32", "float64"]
GAUSSIAN_SPACINGS = [(1.0, 1.0, 1.0), (0.8, 1.0, 1.25)]


def walk_deviation(oracle, case, strict=True):
    """(deviation in voxels over the vertices that are not fragile, the witness, its walk, the fragile mask, the reference's
    vertices)."""
    start = sides.start_points(oracle, case)
    wit, walk, fragile = sides.witnessed(case, start)
    problem = ind.case_conditions(walk, fragile, case)
    assert problem is None or not strict, problem
    ref, _ = sides.reference_walk(oracle, case, start)
    dev = wit.img.voxels_between(ref, walk.points)[~fragile]
    assert np.isfinite(dev).all(), case["name"]
    return float(dev.max()), wit, walk, fragile, ref


def is_normals_case(case):
    return case["variant"] == 0 and case["interp"] == "linear" and not case["gradient"]


def normals_deviation(oracle, case, wit, walk, fragile, ref):
    vox, start = ind.materialised(case)
    geo = sides.geometry_of(case)
    want = normals_ref.normals(oracle, vox, ref, index_start=start, spacing=geo["spacing"], origin=geo["origin"], direction=geo["direction"])
    got, _ = wit.normal(walk.points)
    angle = ind.angle_between(got, want)[~fragile]
    assert np.isfinite(angle).all(), case["name"]
    return float(angle.max())


def evaluation_points(img, rng, n=400):
    """Physical points all over the buffer and up to three voxels outside it."""
    c = rng.uniform(-3.5, img.n + 2.5, size=(n, 3)) + img.start
    return img.index_to_physical(c)


def gaussian_inner(shape, spacing):
    """The part of a [z, y, x] volume at least four sigma from every face."""
    sigma = max(spacing)
    m = [int(np.ceil(4.0 * sigma / s)) for s in spacing]
    inner = (slice(m[2], shape[0] - m[2]), slice(m[1], shape[1] - m[1]), slice(m[0], shape[2] - m[0]))
    assert all(s.stop - s.start >= 2 for s in inner), (shape, spacing)
    return inner


def gaussian_gradient_deviation(vox, spacing):
    want = ind.gaussian_gradient(ind.Image(vox, spacing))
    got = restate.recursive_gaussian_gradient(vox, spacing)
    inner = gaussian_inner(vox.shape, spacing)
    return float(np.abs(got - want)[inner].max() / np.abs(want).max())


def measure(tmp, strict=True):
    """strict: stop where a case does not meet its conditions or a walk is beyond POSITION_LIMIT (the generator); the tests
    measure without and assert per case."""
    oracle = graft.load_oracle()
    families, cases = {}, {}

    def note(family, value):
        families[family] = max(families.get(family, 0.0), value)

    for case in ind.independent_cases():
        dev, wit, walk, fragile, ref = walk_deviation(oracle, case, strict)
        family = sides.family_of(case)
        if strict and family != "gaussian_walk":
            assert dev <= POSITION_LIMIT, "%s: %.3g voxels from the reference on a vertex that is not fragile" % (case["name"], dev)
        note(family, dev)
        cases[case["name"]] = dict(family=family, vertices=len(fragile), fragile=int(fragile.sum()), voxels=dev)
        if is_normals_case(case):
            angle = normals_deviation(oracle, case, wit, walk, fragile, ref)
            note("normals_angle", angle)
            cases[case["name"]]["radians"] = angle
    rng = np.random.default_rng(41)
    for bits in (32, 64):
        ctype = np.float32 if bits == 32 else np.float64
        for shape in sides.COEFFICIENT_SHAPES:
            for dt in COEFFICIENT_PIXELS:
                vox = sides.coefficient_volume(shape, dt)
                for got in (bspline_ref.run_coeffs(tmp, vox, bits), bspline_ref.coefficients(vox, ctype)):
                    note("coefficients_%d" % bits, sides.coefficient_deviation(got, vox))
        for geo in ("rot_a", "start"):
            vox = ind.blob()
            g = ind.GEOMETRIES[geo]
            img = ind.Image(vox, g["spacing"], g["origin"], g.get("direction"), g.get("start", (0, 0, 0)))
            pts = evaluation_points(img, rng)
            want = ind.bspline_value(img)(pts)
            garg = bspline_ref.geometry_arg(g["spacing"], g["origin"], g.get("direction"), g.get("start", (0, 0, 0)))
            for got in (bspline_ref.run_eval(tmp, vox, bits, pts, garg),
                        bspline_ref.evaluate(bspline_ref.coefficients(vox, ctype), pts, g["spacing"], g["origin"], g.get("direction"),
                                             g.get("start", (0, 0, 0)), ctype)):
                note("bspline_evaluate_%d" % bits, float(np.abs(got - want).max() / np.abs(want).max()))
    for vox in (ind.ball("float32"), ind.blob()):
        for spacing in GAUSSIAN_SPACINGS:
            note("gaussian_gradient", gaussian_gradient_deviation(vox, spacing))
    return dict(factor=sides.FACTOR, families=families, cases=cases)


def dumps(result):
    lines = ["{", ' "factor": %s,' % json.dumps(result["factor"]), ' "families": {']
    lines += ["  %s: %s%s" % (json.dumps(k), json.dumps(v), "," if i + 1 < len(result["families"]) else "")
              for i, (k, v) in enumerate(sorted(result["families"].items()))]
    lines += [" },", ' "cases": {']
    lines += ["  %s: %s%s" % (json.dumps(k), json.dumps(v, sort_keys=True), "," if i + 1 < len(result["cases"]) else "")
              for i, (k, v) in enumerate(sorted(result["cases"].items()))]
    lines += [" }", "}"]
    return "\n".join(lines) + "\n"


def main():
    import pathlib
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        result = measure(pathlib.Path(tmp))
    with open(sides.TOLERANCES, "w") as f:
        f.write(dumps(result))
    for k, v in sorted(result["families"].items()):
        print("%-24s %.3g" % (k, v))
    print("-> %s" % sides.TOLERANCES)


if __name__ == "__main__":
    main()
