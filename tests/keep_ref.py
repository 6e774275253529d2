"""Compaction of a mesh by component (cuberille_keep_components), in numpy: the reference the GPU path is held to, applied to the
arrays the library hands out before the call.

    kp = keepK[point_component];  kc = keepK[cell_component]
    new_index  = cumsum(kp) - 1;  new_number = cumsum(keepK) - 1
    points'          = points[kp]            normals' = normals[kp]
    cells'           = new_index[cells[kc] - offset] + offset
    cell_pixels'     = cell_pixels[kc]
    point_component' = new_number[point_component[kp]]
    cell_component'  = new_number[cell_component[kc]]
    component_cells' = component_cells[keepK];   K' = keepK.sum()

Every point of a kept component is kept and the order is preserved, so the new rows are the components of the new mesh
(tests/components_ref.py) -- tests/test_keep_components.py holds this module to that.  No scipy.
"""
from collections import namedtuple

import numpy as np

LARGEST, MIN_CELLS, MASK = 0, 1, 2

Kept = namedtuple("Kept", "points cells point_component cell_component component_cells normals cell_pixels")


def decide(rule, component_cells, n=0, mask=None):
    """keepK: bool[K]."""
    counts = np.asarray(component_cells, dtype=np.uint64)
    k = len(counts)
    if rule in (LARGEST, "largest"):
        keep = np.zeros(k, dtype=bool)
        if k:
            keep[int(np.argmax(counts))] = True          # (argmax: the first of equals, the smaller component number)
        return keep
    if rule in (MIN_CELLS, "min_cells"):
        return counts >= np.uint64(n)
    if rule in (MASK, "mask"):
        mask = np.asarray(mask)
        assert mask.shape == (k,), (mask.shape, k)
        return mask != 0
    raise ValueError("unknown rule %r" % (rule,))


def keep(keepK, points, cells, point_component, cell_component, component_cells, offset=0, normals=None, cell_pixels=None):
    """The kept part of the mesh, order preserved; cells hold index + offset before and after."""
    keepK = np.asarray(keepK, dtype=bool)
    cells = np.asarray(cells, dtype=np.uint64)
    kp = keepK[point_component] if len(point_component) else np.zeros(0, dtype=bool)
    kc = keepK[cell_component] if len(cell_component) else np.zeros(0, dtype=bool)
    new_index = np.cumsum(kp, dtype=np.int64) - 1
    new_number = (np.cumsum(keepK, dtype=np.int64) - 1).astype(np.uint32)
    kept_cells = cells[kc]
    if kept_cells.size:
        old = kept_cells.astype(np.int64) - int(offset)
        assert kp[old].all(), "a kept cell holds a dropped point"
        kept_cells = (new_index[old] + int(offset)).astype(np.uint64)
    return Kept(points=np.ascontiguousarray(points[kp]), cells=np.ascontiguousarray(kept_cells.reshape(-1, cells.shape[1])),
                point_component=new_number[point_component[kp]].astype(np.uint32),
                cell_component=new_number[cell_component[kc]].astype(np.uint32),
                component_cells=np.asarray(component_cells, dtype=np.uint64)[keepK],
                normals=None if normals is None else np.ascontiguousarray(normals[kp]),
                cell_pixels=None if cell_pixels is None else np.ascontiguousarray(cell_pixels[kc]))


def apply(rule, points, cells, point_component, cell_component, component_cells, n=0, mask=None, **rows):
    """decide + keep."""
    return keep(decide(rule, component_cells, n, mask), points, cells, point_component, cell_component, component_cells, **rows)
