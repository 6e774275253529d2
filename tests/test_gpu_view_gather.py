"""Every form of the vertex side's gather under every source view, held to the oracle bit for bit.

The views are whole, border, region (a pitched box with a non-zero start, and an unpitched box at start 0) and band; the pixel
types uint8, float32 and float64; each case runs with projection, point normals and cell pixels on, in quads and in triangles,
and is compared with the oracle on the MATERIALISED copy -- the padded, the cropped or the thresholded volume (the definitions
of test_gpu_border.py, test_gpu_region.py and test_gpu_band.py): cells (they hold the ids) exactly, points, normals and pixels
as bits.

Two volumes (x, y, z):
  (a) 24 x 20 x 16, a ball of radius 4 at the centre -- for the border view that size is the caller's buffer.  Every vertex sits
      in a cell whose gradient ring is in memory, under the border's stricter rule too: a wave takes the immediate-offset form.
  (b) 9 x 8 x 7, a ball of radius 5 cut by all six faces.  Every unit cell touches the rim and the vertices on the faces give
      non-unit cells: the clamped form, the ring's select and the generic taps.
Both conditions are asserted on the CPU, from numpy and the oracle alone, before the volumes are relied on.
"""
import numpy as np
import pytest

import cell_pixels_ref
import normals_ref
from conftest import assert_same_mesh
from normals_ref import same_normals
from test_band import band_image
from test_gpu_border import expected as padded_expected
from test_gpu_region import crop, expected as cropped_expected

pytestmark = pytest.mark.gpu

KW = dict(threshold=0.5, step=-1.0, relax=0.95, max_steps=50, project=1)
ISO = 100
VOLUMES = {"a": ((24, 20, 16), 4.0), "b": ((9, 8, 7), 5.0)}
PIXELS = [np.uint8, np.float32, np.float64]
VIEWS = ["whole", "border", "region_pitched", "region_at_0", "band"]
BOX_START = (3, 2, 1)                                 # the pitched box's place in its buffer


def ball(name, dtype):
    """[z, y, x]: ISO + 20 (R - r), r the distance from the volume's centre -- !(pixel < ISO) is the ball of radius R."""
    (nx, ny, nz), R = VOLUMES[name]
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    f = ISO + 20.0 * (R - np.sqrt((x - (nx - 1) / 2) ** 2 + (y - (ny - 1) / 2) ** 2 + (z - (nz - 1) / 2) ** 2))
    return np.clip(np.rint(f), 0, 255).astype(dtype) if np.dtype(dtype).kind == "u" else f.astype(dtype)


def lattice(oracle, vox):
    return oracle.run(vox, ISO, **dict(KW, project=0, triangles=0)).points


def check_volume_a(oracle, vox):
    """At least 64 vertices (a wave's worth), each -- at the lattice start and where the walk leaves it -- in a cell that lies
    with its gradient ring inside the volume: 1 <= lo and lo + 2 < n on every axis, which is the padded frame's rule
    (2 <= lo + 1, lo + 1 + 3 < n + 2) as well."""
    pts = lattice(oracle, vox)
    assert len(pts) >= 64, len(pts)
    walked = oracle.run(vox, ISO, **dict(KW, triangles=0)).points
    for p in (pts, walked):
        lo = np.floor(p.astype(np.float64))
        assert (lo >= 1).all() and (lo + 2 < np.array(vox.shape[::-1])).all()


def check_volume_b(oracle, vox):
    """Vertices with a coordinate on each of the six faces of the image (index -0.5 and n - 0.5: a cell clamped to one voxel's
    width), and no unit cell away from the rim."""
    pts = lattice(oracle, vox)
    n = np.array(vox.shape[::-1])
    for k in range(3):
        assert (pts[:, k] == -0.5).any() and (pts[:, k] == n[k] - 0.5).any(), ("no vertex on a face of axis", k)
    lo = np.floor(pts.astype(np.float64))
    assert ((lo < 1) | (lo + 2 >= n)).any(axis=1).all()


CHECKS = {"a": check_volume_a, "b": check_volume_b}


@pytest.fixture()
def ex(pkg):
    e = pkg.Extractor(0)
    yield e
    e.close()


def view_case(pkg, oracle, ex, view, vox, triangles):
    """Sets the view on `ex` -> (the volume to extract, the iso value, the oracle's mesh of the materialised copy, that copy, its
    start index, the frame and the inside set of the cell pixels)."""
    kw = dict(KW, triangles=triangles)
    dt = vox.dtype
    rng = np.random.default_rng(5)
    if view == "whole":
        return pkg.Volume(vox), ISO, oracle.run(vox, ISO, **kw), vox, (0, 0, 0), cell_pixels_ref.whole(vox, ISO)
    if view == "border":
        c = 3                                          # below the iso value: the ring closes the ball the faces cut
        ex.set_border(1, c)
        return (pkg.Volume(vox), ISO, padded_expected(oracle, vox, ISO, c, **kw), np.pad(vox, 1, constant_values=dt.type(c)),
                (-1, -1, -1), cell_pixels_ref.border(vox, c, ISO))
    if view in ("region_pitched", "region_at_0"):
        # the volume as a box of a larger buffer of other values: in the middle of it, or its first slices (whole rows, whole
        # slices: nothing pitched, start index 0)
        nz, ny, nx = vox.shape
        start, around = (BOX_START, (nz + 3, ny + 5, nx + 7)) if view == "region_pitched" else ((0, 0, 0), (nz + 2, ny, nx))
        buf = rng.integers(0, 255, around).astype(dt)
        buf[start[2]:start[2] + nz, start[1]:start[1] + ny, start[0]:start[0] + nx] = vox
        size = (nx, ny, nz)
        assert np.array_equal(crop(buf, start, size), vox)
        ex.set_region(start, size)
        return (pkg.Volume(buf), ISO, cropped_expected(oracle, buf, start, size, ISO, **kw), vox, start,
                cell_pixels_ref.region(buf, start, size, ISO))
    assert view == "band"
    lower, upper = ISO, float(vox.max())                # the ball again, as the band's two values
    B, band = band_image(vox, lower, upper, 1, 0)
    assert np.array_equal(band, ~(vox < dt.type(ISO)))
    ex.set_band(lower, upper, 1, 0)
    return pkg.Volume(vox), 1, oracle.run(B, 1, **kw), B, (0, 0, 0), cell_pixels_ref.band(vox, lower, upper, 1, 0, 1)


@pytest.mark.parametrize("dtype", PIXELS, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", sorted(VOLUMES))
def test_every_view_equals_the_oracle_on_the_materialised_copy(pkg, oracle, ex, name, dtype):
    vox = ball(name, dtype)
    CHECKS[name](oracle, vox)
    for view in VIEWS:
        grad = None
        for triangles in (0, 1):
            vol, iso, want, copy, at, (frame, inside) = view_case(pkg, oracle, ex, view, vox, triangles)
            what = (name, np.dtype(dtype).name, view, "triangles" if triangles else "quads")
            assert len(want.points) >= (64 if name == "a" else 8) and len(want.cells) > 0, what
            ex.set_point_normals(True)
            ex.set_cell_pixels(True)
            ex.extract_host(vol, pkg.make_params(iso, **dict(KW, triangles=triangles)))
            mesh, nrm, pix = ex.download(), ex.download_normals(), ex.download_cell_pixels()
            print(what, mesh.points.shape, mesh.cells.shape)
            assert_same_mesh(mesh, want)
            assert np.array_equal(np.isnan(mesh.points), np.isnan(want.points)), what
            if grad is None:
                grad = normals_ref.gradient_image(oracle, copy)
            same_normals(nrm, normals_ref.normals(oracle, copy, want.points, index_start=at, grad=grad), what)
            ref = cell_pixels_ref.cell_pixels(frame, inside, triangles)
            assert pix.dtype == ref.dtype and pix.tobytes() == ref.tobytes(), what
            ex.set_border(0, 0)
            ex.clear_region()
            ex.clear_band()
