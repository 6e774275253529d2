"""Writes tests/golden/point_scalars_tolerance.json: how far the witness of the linear interpolation (tests/independent_ref.py:
np.linalg.inv and scipy's map_coordinates, nothing of the project's) is from the oracle's primitive
cuberille_oracle_interpolate on this CPU, at the oracle's points of the cases of tests/test_point_scalars.py that lie at least a
voxel inside the second image.  Never from GPU output.

One figure: the largest |primitive - witness| over all cases, relative to max |B| of its case.  The test allows `factor` times
it -- the margin of independent_tolerances.json, for the same reason: another CPU's libm and scipy build round a little
differently.  A figure beyond 1e-6 means that the witness or the reference reads the geometry wrongly (the float32 points are
widened exactly, both sides work in double): the script stops there instead of recording it."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import __graft_entry__ as graft  # noqa: E402
import test_point_scalars as cases  # noqa: E402

FACTOR = 4.0
LIMIT = 1.0e-6


def main():
    oracle = graft.load_oracle()
    oracle.build()
    table, worst = {}, 0.0
    for name, b, geo, points in cases.witness_cases(oracle):
        diff, n = cases.witness_difference(oracle, b, geo, points)
        assert diff <= LIMIT, (name, diff)
        table[name] = dict(points=n, relative=diff)
        worst = max(worst, diff)
        print("%-32s %4d points, %.3e" % (name, n, diff))
    lines = ["{", ' "factor": %s,' % json.dumps(FACTOR), ' "relative_to_max_abs": %s,' % json.dumps(worst), ' "cases": {']
    lines += ["  %s: %s%s" % (json.dumps(k), json.dumps(v, sort_keys=True), "," if i + 1 < len(table) else "")
              for i, (k, v) in enumerate(sorted(table.items()))]
    lines += [" }", "}"]
    with open(cases.TOLERANCE, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("-> %s: %.3e" % (cases.TOLERANCE, worst))


if __name__ == "__main__":
    main()
