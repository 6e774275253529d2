"""The reference of the cell pixels (cuberille_set_cell_pixels), in numpy alone.

The quads of a mesh are numbered as DESIGN.md section 2 item 1 says: quad (u, f) exists when in(u) and not in(u + OFF[f]), a
neighbour beyond the image clamped onto u itself (so it counts as inside: no face at the image border), and the quads stand in
voxel raster order, then f ascending.  The cell pixel of quad (u, f) is I(u), the pixel of its inside voxel in the image's own
type; with triangles cells 2k and 2k + 1 both carry quad k's.  I is the view's frame BEFORE any band mapping: the padded image,
the box, and with a band the caller's raw volume (the inside set is the band image's).
tests/test_cell_pixels.py holds this enumeration to the oracle's cells; tests/test_gpu_cell_pixels.py holds the library to it.
"""
import numpy as np

from test_band import band_image

# face f -> (dx, dy, dz): -x, -y, +x, +y, -z, +z
OFF = ((-1, 0, 0), (0, -1, 0), (1, 0, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def inside_of(image, iso):
    """The sweep's predicate !(pixel < iso) in the pixel type (a NaN is inside).  [z, y, x] bool"""
    return ~(image < np.asarray(iso, dtype=image.dtype))


def face_mask(inside):
    """[z, y, x, f]: voxel inside and its neighbour across face f not (the clamped neighbour of a border voxel is itself)."""
    nz, ny, nx = inside.shape
    mask = np.zeros(inside.shape + (6,), dtype=bool)
    for f, (dx, dy, dz) in enumerate(OFF):
        zz = np.clip(np.arange(nz) + dz, 0, nz - 1)
        yy = np.clip(np.arange(ny) + dy, 0, ny - 1)
        xx = np.clip(np.arange(nx) + dx, 0, nx - 1)
        mask[..., f] = inside & ~inside[np.ix_(zz, yy, xx)]
    return mask


def quads(inside):
    """(x, y, z, f) of every quad, in quad order."""
    z, y, x, f = np.nonzero(face_mask(inside))
    return x, y, z, f


def cell_pixels(frame, inside, triangles):
    """One value of frame's dtype per cell, in cell order."""
    x, y, z, _ = quads(inside)
    q = frame[z, y, x]
    return np.repeat(q, 2) if triangles else q


def whole(vox, iso):
    return vox, inside_of(vox, iso)


def border(vox, constant, iso):
    """cuberille_set_border(1, constant): the padded image."""
    frame = np.pad(vox, 1, constant_values=np.asarray(constant, dtype=vox.dtype))
    return frame, inside_of(frame, iso)


def region(vox, start_xyz, size_xyz, iso):
    """cuberille_set_region: the box."""
    (x0, y0, z0), (sx, sy, sz) = start_xyz, size_xyz
    frame = np.ascontiguousarray(vox[z0:z0 + sz, y0:y0 + sy, x0:x0 + sx])
    return frame, inside_of(frame, iso)


def band(vox, lower, upper, inside, outside, iso):
    """cuberille_set_band: the caller's raw volume; the inside set is that of the band image B."""
    B, _ = band_image(vox, lower, upper, inside, outside)
    return vox, inside_of(B, iso)
