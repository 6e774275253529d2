"""cuberille_keep_components without a GPU: the exported symbol, and the numpy reference of tests/keep_ref.py held to the property
that makes it a reference -- the rows it gives for the kept mesh are the components of the kept mesh (tests/components_ref.py),
numbered by smallest point index -- on the oracle's meshes of the GPU cases' volumes; composition, idempotence, the tie rule, the
MIN_CELLS bound on both sides, all and nothing.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import components_ref as cref
import keep_ref
import test_components as cases
from conftest import ROOT


def mesh_rows(points, cells, offset=0):
    """(points, cells, point_component, cell_component, component_cells) of a mesh, the rows from the components' reference."""
    return (points, cells) + tuple(cref.components(cells, len(points), offset))


def same_rows(kept, what, offset=0):
    """Closure: the rows keep_ref hands out equal the components of the mesh it hands out."""
    want = cref.components(kept.cells, len(kept.points), offset)
    cases.same((kept.point_component, kept.cell_component, kept.component_cells), want, what)
    cases.check_properties(kept.cells.astype(np.int64) - offset, len(kept.points), want, what)
    assert kept.cells.dtype == np.uint64 and kept.point_component.dtype == np.uint32 and kept.component_cells.dtype == np.uint64


def same_mesh(a, b, what):
    for name in ("points", "cells", "point_component", "cell_component", "component_cells"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, name)


def as_kept(rows):
    return keep_ref.Kept(*rows, normals=None, cell_pixels=None)


def exercise(rows, what, offset=0):
    """Every property of the contract on one mesh -> the component counts."""
    points, cells, pc, cc, counts = rows
    k = len(counts)
    # all is the identity, none is empty
    everything = keep_ref.apply(keep_ref.MIN_CELLS, *rows, n=0, offset=offset)
    same_mesh(everything, as_kept(rows), (what, "all"))
    nothing = keep_ref.apply(keep_ref.MASK, *rows, mask=np.zeros(k, dtype=np.uint8), offset=offset)
    assert len(nothing.points) == len(nothing.cells) == len(nothing.component_cells) == 0 and nothing.cells.shape[1:] == cells.shape[1:]
    same_rows(nothing, (what, "none"), offset)
    if not k:
        assert not keep_ref.decide(keep_ref.LARGEST, counts).any()
        return counts
    # LARGEST: the first maximum; closure; idempotence
    largest = keep_ref.apply(keep_ref.LARGEST, *rows, offset=offset)
    winner = int(np.argmax(counts))
    assert largest.component_cells.tolist() == [int(counts[winner])] and len(largest.cells) == int(counts[winner])
    assert len(largest.points) == int((pc == winner).sum())
    same_rows(largest, (what, "largest"), offset)
    again = keep_ref.apply(keep_ref.LARGEST, *largest[:5], offset=offset)
    same_mesh(again, largest, (what, "largest twice"))
    # MIN_CELLS at a count and one above it
    for bound in sorted(set(int(c) for c in counts))[:3] + [int(counts.max())]:
        at = keep_ref.apply(keep_ref.MIN_CELLS, *rows, n=bound, offset=offset)
        above = keep_ref.apply(keep_ref.MIN_CELLS, *rows, n=bound + 1, offset=offset)
        assert at.component_cells.tolist() == [int(c) for c in counts if c >= bound]
        assert above.component_cells.tolist() == [int(c) for c in counts if c > bound]
        same_rows(at, (what, "min_cells", bound), offset)
        same_rows(above, (what, "min_cells", bound + 1), offset)
    # MASK, every other component; composition: a second keep on the result equals one keep by the product of the decisions
    mask = (np.arange(k) % 2 == 0).astype(np.uint8)
    half = keep_ref.apply(keep_ref.MASK, *rows, mask=mask, offset=offset)
    same_rows(half, (what, "mask"), offset)
    bound = int(np.median(counts))
    second = keep_ref.apply(keep_ref.MIN_CELLS, *half[:5], n=bound, offset=offset)
    at_once = keep_ref.keep((mask != 0) & (counts >= bound), *rows, offset=offset)
    same_mesh(second, at_once, (what, "composition"))
    same_mesh(keep_ref.apply(keep_ref.LARGEST, *half[:5], offset=offset),
              keep_ref.keep(np.arange(k) == int(np.argmax(np.where(mask != 0, counts.astype(np.int64), -1))), *rows, offset=offset),
              (what, "largest behind a mask"))
    return counts


NOISE = {  # iso: (quads, K, the largest component, its cells) -- the oracle's meshes of test_components.gradient_noise()
    102: (45059, 24, 1, 43737), 130: (50653, 11, 0, 50272), 160: (38514, 47, 2, 29224)}


def test_reference_on_noise(oracle):
    vox = cases.gradient_noise()
    isos = cases.noise_isos(vox)
    assert isos == sorted(NOISE), isos
    for iso in isos:
        quads, k, winner, cells_of_winner = NOISE[iso]
        for triangles in (False, True):
            mesh = oracle.run(vox, iso, triangles=triangles, project=False)
            rows = mesh_rows(mesh.points, mesh.cells)
            counts = exercise(rows, ("noise", iso, triangles))
            f = 2 if triangles else 1
            assert len(mesh.cells) == quads * f and len(counts) == k
            assert int(np.argmax(counts)) == winner and int(counts[winner]) == cells_of_winner * f
            assert int((counts == counts.max()).sum()) == 1                    # one largest component, no tie
            # the comparison never runs on a case where nothing happens: components and cells are dropped, and kept
            largest = keep_ref.apply(keep_ref.LARGEST, *rows)
            assert 0 < len(largest.cells) < len(mesh.cells) and 0 < len(largest.points) < len(mesh.points)
            specks = keep_ref.apply(keep_ref.MIN_CELLS, *rows, n=1000 * f)
            assert 1 <= len(specks.component_cells) < k and 0 < len(specks.cells) < len(mesh.cells)
    # iso 160: the winner is not component 0, the next two have 3 970 and 3 001 quads, LARGEST drops 24 % of the cells
    mesh = oracle.run(vox, 160, triangles=False, project=False)
    counts = cref.components(mesh.cells, len(mesh.points))[2]
    assert sorted(int(c) for c in counts)[-3:] == [3001, 3970, 29224]
    assert round(100 * (1 - 29224 / 38514)) == 24


def test_reference_on_the_small_cases(oracle):
    for name, vox in (("one voxel", cases.one_voxel()), ("corner pair", cases.pair(1, 1, 1)), ("edge pair", cases.pair(0, 1, 1)),
                      ("separated pair", cases.pair(0, 0, 2)), ("isolated voxels", cases.isolated_voxels())):
        for triangles in (False, True):
            mesh = oracle.run(vox, 1, triangles=triangles, project=False)
            rows = mesh_rows(mesh.points, mesh.cells)
            counts = exercise(rows, (name, triangles))
            if name == "separated pair":
                # a tie: counts [6, 6] -- LARGEST keeps component 0
                f = 2 if triangles else 1
                assert counts.tolist() == [6 * f, 6 * f]
                kept = keep_ref.apply(keep_ref.LARGEST, *rows)
                assert keep_ref.decide(keep_ref.LARGEST, counts).tolist() == [True, False]
                assert kept.points.tobytes() == mesh.points[rows[2] == 0].tobytes() and len(kept.points) == 8
                assert len(kept.cells) == 6 * f and int(rows[2][0]) == 0                 # (component 0: that of point 0)
    # an id offset stays in the kept cells
    mesh = oracle.run(cases.pair(0, 0, 2), 1, triangles=True, project=False)
    off = 2 ** 32 + 5
    rows = mesh_rows(mesh.points, mesh.cells + np.uint64(off), off)
    exercise(rows, "offset", off)
    kept = keep_ref.apply(keep_ref.MASK, *rows, mask=[0, 1], offset=off)
    assert int(kept.cells.min()) == off and int(kept.cells.max()) == off + 7


def test_orphan_points_and_the_empty_mesh():
    empty = mesh_rows(np.zeros((0, 3), dtype=np.float32), np.zeros((0, 4), dtype=np.uint64))
    exercise(empty, "empty")
    # points 1 and 4 belong to no cell: components of their own with zero cells
    cells = np.array([[0, 2, 3, 5], [5, 3, 6, 7]], dtype=np.uint64)
    points = np.arange(27, dtype=np.float32).reshape(9, 3)
    rows = mesh_rows(points, cells)
    assert rows[4].tolist() == [2, 0, 0, 0]
    exercise(rows, "orphans")
    # MIN_CELLS 0 keeps the components of zero cells, 1 drops them; an orphan alone can be kept
    assert len(keep_ref.apply(keep_ref.MIN_CELLS, *rows, n=0).points) == 9
    one = keep_ref.apply(keep_ref.MIN_CELLS, *rows, n=1)
    assert len(one.points) == 6 and one.cells.tolist() == [[0, 1, 2, 3], [3, 2, 4, 5]] and one.component_cells.tolist() == [2]
    orphan = keep_ref.apply(keep_ref.MASK, *rows, mask=[0, 0, 1, 0])
    assert orphan.points.tolist() == [points[4].tolist()] and len(orphan.cells) == 0 and orphan.component_cells.tolist() == [0]
    same_rows(orphan, "an orphan alone")
    # normals and cell pixels travel with their points and cells
    kept = keep_ref.apply(keep_ref.LARGEST, *rows, normals=-points, cell_pixels=np.array([7, 9], dtype=np.int16))
    assert kept.normals.tobytes() == (-kept.points).tobytes() and kept.cell_pixels.tolist() == [7, 9] and kept.cell_pixels.dtype == np.int16


def test_symbol_in_header_binding_and_library(pkg):
    header = open(os.path.join(ROOT, "include", "cuberille_hip.h")).read()
    lib = pkg._abi.lib()
    dyn = subprocess.run(["nm", "-D", pkg._abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    name = "cuberille_keep_components"
    assert re.search(r"^int %s\(" % name, header, re.M)
    assert re.search(r"CUBERILLE_KEEP_LARGEST = 0, CUBERILLE_KEEP_MIN_CELLS = 1, CUBERILLE_KEEP_MASK = 2", header)
    assert name in pkg._abi.EXPORTS and getattr(lib, name).argtypes is not None
    assert re.search(r" T %s$" % name, dyn, re.M)
    assert (pkg._abi.KEEP_LARGEST, pkg._abi.KEEP_MIN_CELLS, pkg._abi.KEEP_MASK) == (keep_ref.LARGEST, keep_ref.MIN_CELLS, keep_ref.MASK) == (0, 1, 2)
    for kernel in ("k_keep_largest", "k_keep_sums", "k_keep_scatter_points", "k_keep_scatter_cells"):
        assert kernel in dyn, "no %s kernel in the library" % kernel
    assert lib.cuberille_abi_version() == pkg._abi.ABI_VERSION == 13
    assert callable(pkg.Extractor.keep_components)
    for n in ("SetKeepLargestComponent", "GetKeepLargestComponent", "KeepLargestComponentOn", "KeepLargestComponentOff",
              "SetMinimumComponentCells", "GetMinimumComponentCells"):
        assert callable(getattr(pkg.CuberilleImageToMeshFilter, n)), n
    rows = pkg.CuberilleImageToMeshFilter._NOT_IN_A_GROUP
    assert any(r[0] == "_keep_largest" and "components" in r[2] for r in rows) and any(r[0] == "_min_component_cells" for r in rows)
    itk = os.path.join(ROOT, "midas-journal-740_amd", "itk")
    assert "keep_update" in open(os.path.join(itk, "Makefile")).read()
    drop_in = open(os.path.join(itk, "itkCuberilleImageToMeshFilter.h")).read()
    for n in ("KeepLargestComponent", "MinimumComponentCells"):
        assert n in drop_in, n


def test_host_only_answers(pkg):
    """No context: ERR_ARGUMENT whatever the rule, known or not; nothing is written through the result pointers.  The filter
    mirror's switches without a device: they are settings until Update(), and several devices are refused before one is touched."""
    lib = pkg._abi.lib()
    n = C.c_uint64(7)
    ms = C.c_float(3.0)
    for rule in (0, 1, 2, 3, -1, 99):
        assert lib.cuberille_keep_components(None, rule, 0, None, 0, C.byref(n), C.byref(n), C.byref(n), C.byref(ms)) == pkg._abi.ERR_ARGUMENT
    assert n.value == 7 and ms.value == 3.0
    f = pkg.CuberilleImageToMeshFilter()
    assert not f.GetKeepLargestComponent() and f.GetMinimumComponentCells() == 0
    f.KeepLargestComponentOn()
    f.SetMinimumComponentCells(12)
    assert f.GetKeepLargestComponent() and f.GetMinimumComponentCells() == 12
    f.KeepLargestComponentOff()
    assert not f.GetKeepLargestComponent()
    with pytest.raises(ValueError):
        f.SetMinimumComponentCells(-1)
    for switch in (lambda g: g.KeepLargestComponentOn(), lambda g: g.SetMinimumComponentCells(5)):
        g = pkg.CuberilleImageToMeshFilter(devices=[0, 0])
        g.SetInput(pkg.Volume(cases.one_voxel()))
        g.SetIsoSurfaceValue(1)
        switch(g)
        with pytest.raises(pkg._abi.CuberilleError) as e:
            g.Update()
        assert e.value.code == pkg._abi.ERR_ARGUMENT and "components" in str(e.value)
