"""Writes tests/golden/reference_filter_digests.json from the output of the REFERENCE's own filter (oracle/_ref/ref_filter*,
built by `make -C oracle ref` where the reference tree is present) -- never from the oracle: per case of
tests/ref_filter.py:recorded_cases the case itself (parameters, seed or input), the counts and the SHA-256 of the points
(float32 bits, NaN canonical) and of the cells (uint64).  Where the line search leaves the coordinates undefined
for a whole mesh (ref_filter.points_defined) the points digest is recorded as null; where it does so at single vertices
(ref_filter.undefined_vertices, found from the reference's default branch) the row lists them and the digests leave them out
(ref_filter.masked).  Plain JSON: json.dumps(allow_nan=False).

Beside it, from the same binary: envelope_bspline_digests.json, the same rows for ref_filter.bspline_envelope_cases (which have no
oracle and so no place in the first file), and envelope_finite_vertices.json, per case of the magnitude families how many of
its vertices are finite -- what tests/test_reference_filter.py's mixed-share condition reads."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ref_filter as rf  # noqa: E402


def main():
    assert all(rf.available(v) for v in (0, 1, 2)), "build oracle/_ref/ref_filter* first (make -C oracle ref)"
    rows, finite = [], {}
    for case in rf.recorded_cases():
        points, cells = rf.run_reference(case)
        rf.note_finite(finite, case, points)
        mask = rf.undefined_vertices(case) if rf.points_defined(case) else None
        d = rf.digest(*rf.masked(mask, points, cells))
        if not rf.points_defined(case):
            d["points_sha256"] = None
        rows.append(dict(case=case, undefined_vertices=[] if mask is None else [int(i) for i in np.flatnonzero(mask)], **d))
    with open(rf.DIGESTS, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True, allow_nan=False) for r in rows) + "\n]\n")
    print("%d rows -> %s" % (len(rows), rf.DIGESTS))
    rows = []
    for case in rf.bspline_envelope_cases():
        points, cells = rf.run_reference(case)
        rf.note_finite(finite, case, points)
        rows.append(dict(case=case, undefined_vertices=[], **rf.digest(points, cells)))
    with open(rf.BSPLINE_DIGESTS, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True, allow_nan=False) for r in rows) + "\n]\n")
    with open(rf.ENVELOPE_FINITE, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(finite[k])) for k in rf.ENV_MIXED_FAMILIES) + "\n}\n")
    print("%d rows -> %s, %d families -> %s" % (len(rows), rf.BSPLINE_DIGESTS, len(finite), rf.ENVELOPE_FINITE))


if __name__ == "__main__":
    main()
