"""Point normals without a GPU: the new symbols exist, and the reference the GPU tests hold the kernel to
(tests/normals_ref.py) IS the vector the oracle's walk follows -- shown with the one-step identity.

With threshold = 0, relaxation = 0, max_steps = 0 and step length s the oracle's walk makes exactly one step of length s from
the lattice start v0 along N(v0) and a second of length 0, so its result is float32(v0 + double(N(v0)) * (+-s)), the sign by
the interpolated value against the iso value; every vertex is compared bit for bit.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import normals_ref
from conftest import ROOT

STEP = 0.37
NEW = ("cuberille_set_point_normals", "cuberille_normals_device", "cuberille_normals_download")


def rot(ax, ang):
    c, s = np.cos(ang), np.sin(ang)
    r = np.eye(3)
    i, j = [(1, 2), (0, 2), (0, 1)][ax]
    r[i, i] = r[j, j] = c
    r[i, j], r[j, i] = -s, s
    return r


def blob(n=(10, 12, 14), seed=5):
    """10 x 12 x 14 float32: a Gaussian blob plus noise, and a block at a corner so that clamped taps occur."""
    rng = np.random.default_rng(seed)
    z, y, x = np.mgrid[0:n[0], 0:n[1], 0:n[2]].astype(np.float32)
    vol = (np.exp(-((x - 6.3) ** 2 + (y - 5.1) ** 2 + (z - 4.2) ** 2) / 14.0) * 100 + rng.random(n, dtype=np.float32) * 3).astype(np.float32)
    vol[0:3, 0:4, 0:5] = 90
    return vol, 40.0


GEOMETRIES = {
    "identity": dict(),
    "spacing": dict(spacing=(0.7, 1.3, 2.5), origin=(3.0, -2.0, 10.5)),
    "rotated": dict(spacing=(0.7, 1.3, 2.5), origin=(3.0, -2.0, 10.5), direction=rot(2, 0.4) @ rot(0, 1.1)),
}


def test_symbols_in_header_binding_and_library(pkg):
    header = open(os.path.join(ROOT, "include", "cuberille_hip.h")).read()
    declared = set(re.findall(r"\b(cuberille_[a-z_0-9]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name + " is not declared in include/cuberille_hip.h"
        assert name in pkg._abi.EXPORTS, name + " is not in _abi.EXPORTS"
    pkg._abi.build()
    lib = pkg._abi.lib()
    for name in NEW:
        assert getattr(lib, name).argtypes, name + " has no binding"
    exported = subprocess.run(["nm", "-D", "--defined-only", pkg._abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\bT %s$" % name, exported, re.M), name + " is not exported by the built library"
    assert "k_point_normals" in exported, "the library holds no k_point_normals kernel"
    for cls, methods in ((pkg.Extractor, ("set_point_normals", "download_normals", "normals_device")),
                         (pkg.ExtractorGroup, ("set_point_normals",)),
                         (pkg.CuberilleImageToMeshFilter, ("SetGeneratePointNormals", "GeneratePointNormalsOn", "GeneratePointNormalsOff",
                                                           "GetPointNormals"))):
        for m in methods:
            assert callable(getattr(cls, m, None)), (cls.__name__, m)


@pytest.mark.parametrize("istart", [(0, 0, 0), (5, -3, 7)], ids=["start0", "start5-3+7"])
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_one_step_identity(oracle, geometry, istart):
    vol, iso = blob()
    geo = GEOMETRIES[geometry]
    v0 = oracle.run(vol, iso, project=False, index_start=istart, **geo).points
    v1 = oracle.run(vol, iso, project=True, threshold=0.0, step=STEP, relax=0.0, max_steps=0, index_start=istart, **geo).points
    nrm = normals_ref.normals(oracle, vol, v0, index_start=istart, **geo)
    want = normals_ref.one_step(oracle, vol, iso, v0, nrm, STEP, index_start=istart, **geo)
    assert len(v0) == len(v1) == 302
    assert not np.isnan(v1).any() and not np.isnan(nrm).any()
    assert want.tobytes() == v1.tobytes(), "%d vertices differ" % int((want.view(np.uint32) != v1.view(np.uint32)).any(axis=1).sum())
    # unit length within float rounding, and not one constant direction
    assert np.all(np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0) < 1e-6)
    assert len(np.unique(nrm, axis=0)) > 100
    if geometry == "identity" and istart == (0, 0, 0):
        import restate
        for p, n in list(zip(v0, nrm))[::7]:
            r = restate.py_normal(oracle, vol, [float(c) for c in p])
            assert np.array([r[k] for k in range(3)], dtype=np.float32).tobytes() == n.tobytes()


def zero_gradient_volume():
    """A smooth blob, and beside it a patch whose voxels alternate between two constants with period 2 along every axis: a
    central difference looks two voxels apart, so inside the patch every tap pair is equal, the gradient is exactly zero at every
    site, and the surface around each bright voxel there has vertices with N = 0 / 0 = NaN (quirk Q4).  (A plateau alone cannot do
    it at a lattice start: a vertex exists where its 2 x 2 x 2 voxels differ, and next to a lone step some tap pair differs too.)"""
    n = (12, 14, 26)
    z, y, x = np.mgrid[0:n[0], 0:n[1], 0:n[2]].astype(np.float32)
    vol = (np.exp(-((x - 6.0) ** 2 + (y - 6.5) ** 2 + (z - 5.5) ** 2) / 12.0) * 100).astype(np.float32)
    zi, yi, xi = np.mgrid[0:n[0], 0:n[1], 0:n[2]]
    patch = (xi >= 15) & (xi <= 23) & (yi >= 2) & (yi <= 11) & (zi >= 2) & (zi <= 9)
    vol[patch] = np.where((xi + yi + zi) % 2 == 0, np.float32(80.0), np.float32(0.0))[patch]
    return vol, 40.0


def test_zero_gradient_gives_nan_exactly_where_the_oracle_does(oracle):
    vol, iso = zero_gradient_volume()
    v0 = oracle.run(vol, iso, project=False).points
    v1 = oracle.run(vol, iso, project=True, threshold=0.0, step=STEP, relax=0.0, max_steps=0).points
    nrm = normals_ref.normals(oracle, vol, v0)
    nan_ref, nan_oracle = np.isnan(nrm).any(axis=1), np.isnan(v1).any(axis=1)
    print("%d vertices, %d with a NaN normal, %d NaN in the oracle's one-step walk" % (len(v0), int(nan_ref.sum()), int(nan_oracle.sum())))
    # the condition on the volume, held by the oracle alone: some, and at most half
    assert 0 < int(nan_oracle.sum()) <= len(v0) // 2
    assert np.array_equal(nan_ref, nan_oracle)
    # a NaN normal is NaN in all three components (0 / 0 each)
    assert np.array_equal(np.isnan(nrm).all(axis=1), nan_ref)
    want = normals_ref.one_step(oracle, vol, iso, v0, nrm, STEP)
    ok = ~nan_ref
    assert want[ok].tobytes() == v1[ok].tobytes()
