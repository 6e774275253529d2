"""cuberille_set_cell_pixels without a GPU: the exported symbols, and the numpy reference of tests/cell_pixels_ref.py held to the
oracle.

The oracle numbers no faces; its cells say which (voxel, face) each quad is geometrically.  With unit geometry a lattice corner c
stands at the point c - 1/2, so the four points of a quad of an unprojected mesh share one coordinate (the face's axis), their
mean is the centre of the face, and the two voxels that share the face sit half a voxel to either side of it along that axis:
exactly one of them is inside, and the face code follows from the axis and the side.  The reference's enumeration must give that
(voxel, face) sequence, and the oracle's triangles 2k and 2k + 1 must use only quad k's vertices.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import cell_pixels_ref as ref
from conftest import ROOT

SYMBOLS = ("cuberille_set_cell_pixels", "cuberille_cell_pixels_device", "cuberille_cell_pixels_download")


def label_volume(shape, seed):
    """uint8 labels 0 .. 5 at random, voxel by voxel, a little more than half of them background, with one isolated voxel (all six
    faces) planted.  [z, y, x]"""
    rng = np.random.default_rng(seed)
    vox = (rng.integers(1, 6, shape) * (rng.random(shape) < 0.45)).astype(np.uint8)
    z, y, x = shape[0] // 2, shape[1] // 2, shape[2] // 2
    vox[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2] = 0
    vox[z, y, x] = 3
    return vox


def cases():
    """name -> (frame, inside, the image the oracle meshes, its iso value)"""
    a, b = label_volume((5, 6, 70), 3), label_volume((3, 4, 130), 5)
    out = {"5x6x70": ref.whole(a, 1) + (a, 1), "3x4x130": ref.whole(b, 1) + (b, 1)}
    for name, constant in (("border below iso", 0), ("border at or above iso", 3)):
        frame, inside = ref.border(a, constant, 2)
        out[name] = (frame, inside, frame, 2)
    frame, inside = ref.region(a, (3, 1, 1), (61, 4, 3), 1)
    out["region"] = (frame, inside, frame, 1)
    frame, inside = ref.band(b, 2, 4, 1, 0, 1)
    out["band"] = (frame, inside, np.where((b >= 2) & (b <= 4), np.uint8(1), np.uint8(0)), 1)
    return out


CASES = cases()


def test_symbols_in_header_binding_and_library(pkg):
    header = open(os.path.join(ROOT, "include", "cuberille_hip.h")).read()
    lib = pkg._abi.lib()
    dyn = subprocess.run(["nm", "-D", pkg._abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in pkg._abi.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
        assert re.search(r" T %s$" % name, dyn, re.M), name
    assert "k_cell_pixels" in dyn, "no k_cell_pixels kernel in the library"
    assert lib.cuberille_abi_version() == pkg._abi.ABI_VERSION == 13
    assert "deliberate" in header[header.index("Cell pixels (new symbols"):header.index("int cuberille_set_cell_pixels(")]
    for cls, names in ((pkg.Extractor, ("set_cell_pixels", "download_cell_pixels", "cell_pixels_device")),
                       (pkg.ExtractorGroup, ("set_cell_pixels",)),
                       (pkg.CuberilleImageToMeshFilter, ("SetSavePixelAsCellData", "GetSavePixelAsCellData", "SavePixelAsCellDataOn",
                                                         "SavePixelAsCellDataOff", "GetCellPixels"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls.__name__, n)
    assert any(row[0] == "_cell_pixels_on" and "cell pixels" in row[2] for row in pkg.CuberilleImageToMeshFilter._NOT_IN_A_GROUP)


def geometric_reading(mesh, inside):
    """(x, y, z, f) of every quad of an unprojected quad mesh of unit geometry, read off its corners."""
    p = mesh.points[mesh.cells.astype(np.int64)].astype(np.float64)          # [n, 4, 3]
    flat = (p == p[:, :1, :]).all(axis=1)                                       # [n, 3]: the coordinate all four corners share
    assert (flat.sum(axis=1) == 1).all()
    axis = flat.argmax(axis=1)
    centre = p.mean(axis=1)
    n = np.arange(len(p))
    lo, hi = centre.copy(), centre.copy()
    lo[n, axis] -= 0.5
    hi[n, axis] += 0.5
    lo, hi = np.rint(lo).astype(np.int64), np.rint(hi).astype(np.int64)
    nz, ny, nx = inside.shape
    for v in (lo, hi):                                                          # (no face at the image border: both voxels exist)
        assert (v >= 0).all() and (v[:, 0] < nx).all() and (v[:, 1] < ny).all() and (v[:, 2] < nz).all()
    in_lo, in_hi = inside[lo[:, 2], lo[:, 1], lo[:, 0]], inside[hi[:, 2], hi[:, 1], hi[:, 0]]
    assert (in_lo != in_hi).all(), "exactly one side of a face is inside"
    u = np.where(in_lo[:, None], lo, hi)
    # the voxel on the low side is inside: the face looks along +axis (x: 2, y: 3, z: 5), else along -axis (x: 0, y: 1, z: 4)
    f = np.where(in_lo, np.array([2, 3, 5])[axis], np.array([0, 1, 4])[axis])
    return u[:, 0], u[:, 1], u[:, 2], f


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_is_the_oracles_numbering(oracle, name):
    frame, inside, image, iso = CASES[name]
    assert np.array_equal(inside, ref.inside_of(image, iso))
    x, y, z, f = ref.quads(inside)
    n = len(x)
    # the case is worth its name: several waves and a ragged last one, a voxel with all six faces, several cell values
    assert n > 256 and n % 64 != 0, n
    assert ref.face_mask(inside).all(axis=3).any(), "no voxel with all six faces"
    pix = ref.cell_pixels(frame, inside, False)
    assert pix.dtype == frame.dtype and len(np.unique(pix)) >= 3
    if name == "border at or above iso":
        nz, ny, nx = frame.shape
        ring = (x == 0) | (x == nx - 1) | (y == 0) | (y == ny - 1) | (z == 0) | (z == nz - 1)
        assert ring.any() and (pix[ring] == 3).all(), "no quad whose inside voxel lies on the ring"
    if name == "band":
        assert set(np.unique(pix)) == {2, 3, 4}
    quad = oracle.run(image, iso, triangles=False, project=False)
    assert len(quad.cells) == n
    gx, gy, gz, gf = geometric_reading(quad, inside)
    assert np.array_equal(gx, x) and np.array_equal(gy, y) and np.array_equal(gz, z) and np.array_equal(gf, f)
    # triangles 2k and 2k + 1 use only quad k's vertices, with the projection on or off
    for project in (False, True):
        tri = oracle.run(image, iso, triangles=True, project=project)
        assert len(tri.cells) == 2 * n
        q = np.repeat(quad.cells, 2, axis=0)
        assert (tri.cells[:, :, None] == q[:, None, :]).any(axis=2).all()
    t = ref.cell_pixels(frame, inside, True)
    assert np.array_equal(t[0::2], pix) and np.array_equal(t[1::2], pix)
