"""cuberille_set_components without a GPU: the exported symbols, and the numpy reference of tests/components_ref.py held to a
second, independent statement of the definition -- a breadth-first walk over "cells that share a point" in plain Python -- on the
oracle's meshes of the GPU cases' volumes and of the tests/golden/data volumes; then the properties the definition promises.
"""
import ctypes as C
import os
import re
import subprocess
from collections import deque

import numpy as np
import pytest

import components_ref as ref
from conftest import ROOT

SYMBOLS = ("cuberille_set_components", "cuberille_components_info", "cuberille_components_device", "cuberille_components_download")


# ---- the volumes of the cases ([z, y, x], uint8, iso 1 unless said), shared with tests/test_gpu_components.py -----------------
def one_voxel():
    vox = np.zeros((3, 3, 3), dtype=np.uint8)
    vox[1, 1, 1] = 1
    return vox


def pair(dz, dy, dx):
    """Two voxels, the second (dx, dy, dz) from the first: (1, 1, 1) touch at a corner only, (1, 1, 0) at an edge only,
    (2, 0, 0) have one empty voxel between them."""
    vox = np.zeros((5, 5, 6), dtype=np.uint8)
    vox[1, 1, 1] = 1
    vox[1 + dz, 1 + dy, 1 + dx] = 1
    return vox


def isolated_voxels(shift=0):
    """Every second index on each axis of 64 x 64 x 32 (x, y, z): 16 384 voxels that touch nothing, 131 072 points -- the scan's
    block sums (512) and their scan (2 blocks) both take more than one block, the roots sit at a regular stride.  shift: the
    same volume one voxel on in x, so that roots fall on other lanes."""
    vox = np.zeros((32, 64, 64), dtype=np.uint8)
    vox[0::2, 0::2, 0::2] = 1
    return np.roll(vox, shift, axis=2) if shift else vox


def comb():
    """Teeth one voxel thick along z at every second (x, y) of 33 x 33 x 40, joined only by a full plate in the last slice."""
    vox = np.zeros((40, 33, 33), dtype=np.uint8)
    vox[:, 0::2, 0::2] = 1
    vox[39] = 1
    return vox


def serpentine():
    """A one-voxel-thick boustrophedon path through 32 x 32 x 16: in every second slice, rows along x at every second y, joined
    at x = 31 and x = 0 in turn -- a walk from (x, y) = (0, 0) to (0, 30) --, and the slices joined by one voxel at the walk's end
    and start in turn: one long chain, its smallest point index at one end."""
    vox = np.zeros((16, 32, 32), dtype=np.uint8)
    for k, z in enumerate(range(0, 16, 2)):
        for j in range(16):
            vox[z, 2 * j, :] = 1
            if j < 15:
                vox[z, 2 * j + 1, 31 if j % 2 == 0 else 0] = 1
        if z + 2 < 16:
            vox[z + 1, 30 if k % 2 == 0 else 0, 0] = 1
    return vox


def gradient_noise(shape=(48, 52, 70), seed=11, cell=5):
    """uint8 gradient noise: random values on a coarse lattice, interpolated linearly along each axis.  Rows of 70: two words,
    the second ragged."""
    rng = np.random.default_rng(seed)
    coarse = rng.random(tuple(s // cell + 2 for s in shape))
    out = coarse
    for axis, n in enumerate(shape):
        pos = np.arange(n) / cell
        i = pos.astype(np.int64)
        t = (pos - i).reshape([-1 if a == axis else 1 for a in range(3)])
        out = np.take(out, i, axis=axis) * (1 - t) + np.take(out, i + 1, axis=axis) * t
    return np.round(out * 255).astype(np.uint8)


def noise_isos(vox):
    return [int(v) for v in np.quantile(vox, (0.3, 0.55, 0.8))]


def two_pieces_in_a_box():
    """An object that a region cuts in two: a U whose bottom lies outside the box (start (2, 2, 2), size (20, 8, 6))."""
    vox = np.zeros((10, 14, 26), dtype=np.uint8)
    vox[3:7, 4:8, 4:8] = 7                                                      # one arm
    vox[3:7, 4:8, 14:18] = 7                                                    # the other
    vox[3:7, 11:13, 4:18] = 7                                                   # the bottom, y 11 .. 12: outside a box that ends at y = 9
    vox[3:7, 8:11, 4:8] = 7
    vox[3:7, 8:11, 14:18] = 7
    return vox, (2, 2, 2), (20, 8, 6)


# ---- the second statement of the definition ------------------------------------------------------------------------------------
def walk(cells, n_points):
    """Breadth first over "cells that share a point", in plain Python: points in increasing index start a component each unless an
    earlier walk reached them."""
    cells = [[int(v) for v in c] for c in np.asarray(cells)]
    of_point = [[] for _ in range(n_points)]
    for c, ids in enumerate(cells):
        for p in ids:
            of_point[p].append(c)
    point_component = [-1] * n_points
    seen = [False] * len(cells)
    k = 0
    for start in range(n_points):
        if point_component[start] >= 0:
            continue
        point_component[start] = k
        todo = deque([start])
        while todo:
            p = todo.popleft()
            for c in of_point[p]:
                if not seen[c]:
                    seen[c] = True
                    for q in cells[c]:
                        if point_component[q] < 0:
                            point_component[q] = k
                            todo.append(q)
        k += 1
    cell_component = [point_component[ids[0]] for ids in cells]
    counts = [0] * k
    for c in cell_component:
        counts[c] += 1
    return (np.array(point_component, dtype=np.uint32), np.array(cell_component, dtype=np.uint32), np.array(counts, dtype=np.uint64))


def same(got, want, what):
    for g, w, name in zip(got, want, ("point_component", "cell_component", "component_cells")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name, "first difference at %d" % int(np.argmax(g != w)))


def check_properties(cells, n_points, got, what):
    pc, cc, counts = got
    k = len(counts)
    assert pc.dtype == np.uint32 and cc.dtype == np.uint32 and counts.dtype == np.uint64
    assert int(counts.sum()) == len(cells), what
    if n_points:
        assert k == int(pc.max()) + 1 and k <= n_points
        first = np.full(k, n_points, dtype=np.int64)
        np.minimum.at(first, pc, np.arange(n_points))
        assert (np.diff(first) > 0).all(), (what, "the numbering does not increase with the smallest point index")
    if len(cells):
        assert (pc[np.asarray(cells).astype(np.int64)] == cc[:, None]).all(), (what, "a cell with points of two components")


CASES = {"one voxel": (one_voxel, 1, 1), "corner pair": (lambda: pair(1, 1, 1), 1, 1), "edge pair": (lambda: pair(0, 1, 1), 1, 1),
         "separated pair": (lambda: pair(0, 0, 2), 1, 2), "isolated voxels": (isolated_voxels, 1, 1024),
         "isolated voxels shifted": (lambda: isolated_voxels(1), 1, 1024), "comb": (comb, 1, 1), "serpentine": (serpentine, 1, 1)}
# (isolated voxels: the oracle always reproduces quirk Q1 -- across an empty slice a voxel's lower corners are the vertices of the
#  occupied slice below -- so the 16 voxels of a z column share points and the oracle's mesh has 32 x 32 = 1024 components; the
#  library with q1 off gives the 16 384 separate cubes and 131 072 points, tests/test_gpu_components.py runs both)


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_against_the_walk_on_the_cases(oracle, name):
    make, iso, k = CASES[name]
    vox = make()
    quads = oracle.run(vox, iso, triangles=False, project=False)
    n = len(quads.points)
    got = ref.components(quads.cells, n)
    same(got, walk(quads.cells, n), name)
    check_properties(quads.cells, n, got, name)
    assert len(got[2]) == k, (name, len(got[2]))
    if name == "one voxel":
        assert n == 8 and len(quads.cells) == 6
    # triangles: the two halves of a quad share their diagonal -- the same point labels, the counts doubled
    tri = oracle.run(vox, iso, triangles=True, project=True)
    t = ref.components(tri.cells, n)
    assert t[0].tobytes() == got[0].tobytes() and (t[2] == 2 * got[2]).all()
    assert np.array_equal(t[1][0::2], got[1]) and np.array_equal(t[1][1::2], got[1])
    # the order of the cells means nothing to the points, and the cells' labels move with them
    perm = np.random.default_rng(5).permutation(len(quads.cells))
    p = ref.components(quads.cells[perm], n)
    assert p[0].tobytes() == got[0].tobytes() and p[2].tobytes() == got[2].tobytes() and np.array_equal(p[1], got[1][perm])
    # ... and an id offset is taken off
    o = ref.components(quads.cells + np.uint64(1000), n, offset=1000)
    same(o, got, name + " offset")


def test_reference_against_the_walk_on_noise(oracle):
    vox = gradient_noise()
    isos = noise_isos(vox)
    assert len(set(isos)) == 3
    ks = []
    for iso, triangles in ((isos[0], False), (isos[1], True), (isos[2], False)):
        mesh = oracle.run(vox, iso, triangles=triangles, project=False)
        n = len(mesh.points)
        got = ref.components(mesh.cells, n)
        same(got, walk(mesh.cells, n), ("noise", iso))
        check_properties(mesh.cells, n, got, ("noise", iso))
        ks.append(len(got[2]))
    print("noise: iso", isos, "components", ks)
    assert max(ks) >= 3, ks


def test_reference_against_the_walk_on_the_golden_volumes(oracle, volumes, ctest_cases):
    done = set()
    for c in ctest_cases:
        if c["input"] in done:
            continue
        done.add(c["input"])
        mesh = oracle.run(volumes(c["input"]).voxels, c["iso"], triangles=bool(c["triangles"]), project=False)
        n = len(mesh.points)
        got = ref.components(mesh.cells, n)
        same(got, walk(mesh.cells, n), c["input"])
        check_properties(mesh.cells, n, got, c["input"])
    assert len(done) >= 5


def test_orphan_points_and_the_empty_mesh():
    pc, cc, counts = ref.components(np.zeros((0, 4), dtype=np.uint64), 0)
    assert pc.shape == cc.shape == counts.shape == (0,) and pc.dtype == np.uint32 and counts.dtype == np.uint64
    # points 1 and 4 belong to no cell: components of their own with zero cells, numbered where their index falls
    cells = np.array([[0, 2, 3, 5], [5, 3, 6, 7]], dtype=np.uint64)
    got = ref.components(cells, 9)
    assert got[0].tolist() == [0, 1, 0, 0, 2, 0, 0, 0, 3] and got[1].tolist() == [0, 0] and got[2].tolist() == [2, 0, 0, 0]
    same(got, walk(cells, 9), "orphans")


def test_symbols_in_header_binding_and_library(pkg):
    header = open(os.path.join(ROOT, "include", "cuberille_hip.h")).read()
    lib = pkg._abi.lib()
    dyn = subprocess.run(["nm", "-D", pkg._abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in pkg._abi.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
        assert re.search(r" T %s$" % name, dyn, re.M), name
    for kernel in ("k_comp_hook", "k_comp_flatten", "k_comp_scan", "k_comp_relabel_cells"):
        assert kernel in dyn, "no %s kernel in the library" % kernel
    assert lib.cuberille_abi_version() == pkg._abi.ABI_VERSION == 13
    for cls, names in ((pkg.Extractor, ("set_components", "download_components", "components_device", "n_components")),
                       (pkg.ExtractorGroup, ("set_components",)),
                       (pkg.CuberilleImageToMeshFilter, ("SetGenerateComponents", "GetGenerateComponents", "GenerateComponentsOn",
                                                         "GenerateComponentsOff", "GetPointComponents", "GetCellComponents",
                                                         "GetComponentCellCounts", "GetNumberOfComponents"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls.__name__, n)
    assert any(row[0] == "_components_on" and "components" in row[2] for row in pkg.CuberilleImageToMeshFilter._NOT_IN_A_GROUP)


def test_scan_plan_program():
    """csrc/tests/components_plan.hip: the numbering's block plan at every size where it takes another shape.  No GPU."""
    csrc = os.path.join(ROOT, "midas-journal-740_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "build/components_plan"])  # (make knows whether it is stale)
    run = subprocess.run([os.path.join(csrc, "build", "components_plan")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "components_plan ok" in run.stdout, run.stdout + run.stderr


def test_host_only_answers(pkg):
    """No context: the new entry points answer ERR_ARGUMENT, they do not crash.  No device: the filter mirror with the switch on
    raises the library's ERR_NO_DEVICE from Update() like every other switch; several devices are refused before one is touched."""
    lib = pkg._abi.lib()
    k = C.c_uint64(7)
    assert lib.cuberille_set_components(None, 1) == pkg._abi.ERR_ARGUMENT
    assert lib.cuberille_components_info(None, C.byref(k)) == pkg._abi.ERR_ARGUMENT
    assert lib.cuberille_components_device(None, None, None, None) == pkg._abi.ERR_ARGUMENT
    assert lib.cuberille_components_download(None, None, None, None, 0) == pkg._abi.ERR_ARGUMENT
    f = pkg.CuberilleImageToMeshFilter()
    assert not f.GetGenerateComponents() and f.GetPointComponents() is None and f.GetNumberOfComponents() == 0
    f.GenerateComponentsOn()
    assert f.GetGenerateComponents()
    f.SetInput(pkg.Volume(one_voxel()))
    f.SetIsoSurfaceValue(1)
    if lib.cuberille_device_count() <= 0:
        with pytest.raises(pkg._abi.CuberilleError) as e:
            f.Update()
        assert e.value.code == pkg._abi.ERR_NO_DEVICE
    g = pkg.CuberilleImageToMeshFilter(devices=[0, 0])
    g.SetInput(pkg.Volume(one_voxel()))
    g.SetIsoSurfaceValue(1)
    g.GenerateComponentsOn()
    with pytest.raises(pkg._abi.CuberilleError) as e:
        g.Update()
    assert e.value.code == pkg._abi.ERR_ARGUMENT and "components" in str(e.value)
