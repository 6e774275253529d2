#!/usr/bin/env python3
"""Regenerate tests/golden/closed_border_cases.json: the meshes of volumes whose surface meets the image border.

FROZEN ORACLE OUTPUT, not reference output.  The volumes the reference ships were padded by hand so that no
iso-surface pixel lies on an edge (its documented limitation, h:54-57); cropped to their central half along every axis
(v[n//4 : 3*n//4] per numpy axis) they do.  For each crop, at the iso value of the volume's first CTest row, this
stores how many inside voxels lie on the crop's six border faces (summed per face), the counts of the OPEN mesh (the crop as it is: holes where
the object meets the border) and, for {quads, triangles} x {projection off, on}, the counts and SHA-256 digests of the
CLOSED mesh: the oracle's mesh of np.pad(crop, 1, constant_values=0) with the start index one lower and the same origin,
spacing and direction -- what itk::ConstantPadImageFilter hands the reference, and the definition of
cuberille_set_border.  Parameters: the oracle's defaults (threshold 0.5, step a quarter of the largest spacing, relaxation
0.95, 50 steps).
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import __graft_entry__ as graft  # noqa: E402

from make_mesh_digests import digest  # noqa: E402


def central_half(v):
    return np.ascontiguousarray(v[tuple(slice(n // 4, 3 * n // 4) for n in v.shape)])


def border_inside(crop, iso):
    """Inside voxels on the six border faces, counted per face (a voxel on an edge of the volume counts for each of its faces)."""
    inside = ~(crop < np.asarray(iso).astype(crop.dtype))
    return sum(int(inside.take(k, axis=a).sum()) for a in range(3) for k in (0, -1))


def edge_multiplicities(cells):
    """How many edges of a triangle mesh lie in 1, 2, 3 ... triangles, as {multiplicity: edges}."""
    e = np.sort(np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]]), axis=1)
    _, n = np.unique(e, axis=0, return_counts=True)
    return {int(k): int(v) for k, v in zip(*np.unique(n, return_counts=True))}


def closed(oracle, vol, crop, iso, pad_value=0, index_start=(0, 0, 0), **kw):
    """The definition: the oracle on the explicitly padded crop, one index lower."""
    padded = np.pad(crop, 1, constant_values=pad_value)
    return oracle.run(padded, iso, spacing=vol.spacing, origin=vol.origin, direction=vol.direction,
                      index_start=tuple(int(s) - 1 for s in index_start), **kw)


def main():
    pkg, oracle = graft.load_package(), graft.load_oracle()
    oracle.build()
    cases = json.load(open(os.path.join(HERE, "ctest_cases.json")))
    iso_of = {}
    for c in cases:
        iso_of.setdefault(c["input"], c["iso"])
    rows = []
    for name in sorted(iso_of):
        vol = pkg.read_mha(os.path.join(HERE, "data", name))
        crop = central_half(vol.voxels)
        iso = iso_of[name]
        opened = oracle.run(crop, iso, spacing=vol.spacing, origin=vol.origin, direction=vol.direction)
        row = dict(input=name, iso=iso, crop_dims_zyx=list(crop.shape), inside_voxels_on_border=border_inside(crop, iso),
                   pad_value=0, open_points=int(opened.points.shape[0]), open_cells=int(opened.cells.shape[0]), closed=[])
        for tri in (0, 1):
            for proj in (0, 1):
                m = closed(oracle, vol, crop, iso, triangles=tri, project=proj)
                row["closed"].append(dict(triangles=tri, project=proj, **digest(m)))
                if tri and proj:
                    # a closed mesh has no edge in ONE triangle.  Two everywhere, except that voxels which touch along an edge
                    # only share that edge's two vertices in a cuberille mesh: such an edge lies in four triangles (the
                    # reference's meshes of blob2 and blob3, uncropped and unpadded, have them too)
                    row["closed_edge_multiplicities"] = edge_multiplicities(m.cells)
                    row["open_edge_multiplicities"] = edge_multiplicities(opened.cells)
        rows.append(row)
        last = row["closed"][-1]
        print("%-18s iso %-4s border %-5d open %d / %d  closed %d / %d" % (
            name, iso, row["inside_voxels_on_border"], row["open_points"], row["open_cells"], last["points"], last["cells"]))
    out = dict(note="frozen ORACLE output (tests/golden/make_closed_border_cases.py), not reference output", cases=rows)
    with open(os.path.join(HERE, "closed_border_cases.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
