"""The surface components of a mesh by their definition (cuberille_set_components), in numpy: the reference the GPU pass is held to.

Two points are joined when one cell holds both; a component is a class of the transitive closure; a point that no cell holds
is a component of its own with zero cells; components are numbered 0 .. K-1 in the order of their smallest point index.

Minimum propagation to a fixed point: every point starts with its own index as label; a round gives every cell the minimum
label of its points and every point the minimum over its cells (np.minimum.at), then replaces every label by its label's label
(pointer jumping: a label is a point index of the same component, so this only shortens the way).  Labels only decrease and stay
inside the component; at the fixed point all points of a cell agree, hence all points of a component, and the label is the
component's smallest index because that point never changes its own.  np.unique then numbers the labels in increasing order.
No scipy.
"""
import numpy as np


def components(cells, n_points, offset=0):
    """cells: [n_cells, 3 | 4] point ids (index + offset) -> (point_component uint32[n_points], cell_component uint32[n_cells],
    component_cells uint64[K])."""
    n_points = int(n_points)
    cells = np.asarray(cells)
    idx = (cells.astype(np.int64) - int(offset)).reshape(len(cells), cells.shape[1] if cells.ndim == 2 else 1)
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < n_points)
    label = np.arange(n_points, dtype=np.int64)
    while len(idx):
        low = label[idx].min(axis=1)
        new = label.copy()
        np.minimum.at(new, idx.reshape(-1), np.repeat(low, idx.shape[1]))
        for _ in range(3):
            new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    roots, point_component = np.unique(label, return_inverse=True)
    point_component = point_component.reshape(-1).astype(np.uint32)
    cell_component = point_component[idx[:, 0]] if len(idx) else np.zeros(0, dtype=np.uint32)
    component_cells = np.bincount(cell_component, minlength=len(roots)).astype(np.uint64)
    return point_component, cell_component.astype(np.uint32), component_cells
