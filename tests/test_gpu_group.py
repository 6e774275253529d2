"""-m gpu: the context group (include/cuberille_hip.h: cuberille_group_*, ExtractorGroup, the drop-in's SetDevices /
CUBERILLE_DEVICES) against the oracle -- or, at sizes the oracle cannot take, against the oracle-pinned single context:
ids, cell order and float bits.  Several contexts on device 0 stand for several GPUs: the group's code is the same."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, assert_same_mesh
from gpu_helpers import _read_vtk_polydata

pytestmark = pytest.mark.gpu

REF_BIN = os.path.join(ROOT, "oracle", "_ref")
DATA = ["blob0.mha", "blob1.mha", "blob2.mha", "blob3.mha", "blob4.mha", "fuel.mha", "hydrogenAtom.mha",
        "marschnerlobb.mha", "neghip.mha", "nucleon.mha", "silicium.mha"]


@pytest.fixture(scope="module")
def groups(pkg):
    made = {}

    def get(n):
        if n not in made:
            made[n] = pkg.ExtractorGroup([0] * n)
        return made[n]
    yield get
    for g in made.values():
        g.close()


def _group_mesh(pkg, g, vol, iso, **kw):
    prm = pkg.make_params(iso, **kw)
    res = g.extract_host(vol, prm)
    mesh = g.download()
    assert (res.n_points, res.n_cells) == (mesh.GetNumberOfPoints(), mesh.GetNumberOfCells())
    return res, mesh


def _oracle(oracle, vol, iso, **kw):
    kw = dict(kw)
    kw.pop("q1", None)
    return oracle.run(vol.voxels, iso, spacing=vol.spacing, origin=vol.origin, direction=vol.direction,
                      index_start=vol.index_start, **kw)


def test_every_data_volume_with_2_3_and_8_contexts(pkg, oracle, volumes, ctest_cases, groups):
    iso_of = {c["input"]: c["iso"] for c in ctest_cases}
    assert sorted(iso_of) == sorted(DATA)
    for name in DATA:
        vol = volumes(name)
        for tri in (True, False):
            for proj in (True, False):
                kw = dict(triangles=tri, project=proj, threshold=0.2, step=0.24, relax=0.95, max_steps=50)
                ref = _oracle(oracle, vol, iso_of[name], **kw)
                for n in (2, 3, 8):
                    res, mesh = _group_mesh(pkg, groups(n), vol, iso_of[name], **kw)
                    assert_same_mesh(mesh, ref)
                    used = min(n, vol.dims[2])
                    slabs = [groups(n).slab_result(i) for i in range(used)]
                    assert sum(s.n_points for s in slabs) == res.n_points
                    assert sum(s.n_cells for s in slabs) == res.n_cells
                    assert sum(s.proj_iterations for s in slabs) == res.proj_iterations
                    assert res.ms_total == max(s.ms_total for s in slabs)
                    assert res.verts_per_cell == (3 if tri else 4)


def _q1_volume(case):
    """The quirk-Q1-across-a-cut constructions of tests/test_gpu_slabs.py, restated: (voxels, iso, slabs)."""
    if case == "two_voxels_empty_rank_between":
        vox = np.zeros((48, 8, 8), dtype=np.uint8)          # 3 slabs of 16 slices; the middle one holds nothing
        vox[10, 3, 3] = 255
        vox[10, 4, 3] = 255
        vox[40, 3, 3] = 255
        return vox, 128, 3
    if case == "nothing_occupied_below":                    # slab 1's first occupied slice has nothing below it anywhere
        rng = np.random.default_rng(5)
        vox = np.zeros((64, 12, 70), dtype=np.uint8)
        vox[40:50] = (rng.random((10, 12, 70)) < 0.3) * 255
        return vox, 128, 2
    if case == "source_in_the_halo":                        # cut at 20; slices 16..21 empty, source slice 15 in the halo
        rng = np.random.default_rng(3)
        vox = np.zeros((40, 12, 70), dtype=np.uint8)
        vox[8:16] = (rng.random((8, 12, 70)) < 0.3) * 255
        vox[22:30] = (rng.random((8, 12, 70)) < 0.3) * 255
        return vox, 128, 2
    rng = np.random.default_rng(11)
    fill = lambda a, b: (rng.random((b - a, 12, 70)) < 0.3) * 255      # noqa: E731
    if case == "ghost_lowest_occupied":                     # cut at 20; slice 19 is the lowest occupied slice
        vox = np.zeros((40, 12, 70), dtype=np.uint8)
        vox[19:28] = fill(19, 28)
        return vox, 128, 2
    if case == "ghost_source_in_the_halo":                  # 14..15 occupied, 16..18 empty, 19.. occupied
        vox = np.zeros((40, 12, 70), dtype=np.uint8)
        vox[14:16] = fill(14, 16)
        vox[19:28] = fill(19, 28)
        return vox, 128, 2
    if case == "ghost_source_below_the_buffer":             # cut at 32; 10..12, then 31.. occupied
        vox = np.zeros((64, 12, 70), dtype=np.uint8)
        vox[10:13] = fill(10, 13)
        vox[31:40] = fill(31, 40)
        return vox, 128, 2
    assert case == "ghost_and_owned_share_a_source"         # 3 slabs of 16; slice 3, then 31..: slabs 1 and 2 go back to 3
    vox = np.zeros((48, 12, 70), dtype=np.uint8)
    vox[3:4] = fill(3, 4)
    vox[31:40] = fill(31, 40)
    return vox, 128, 3


@pytest.mark.parametrize("case", ["two_voxels_empty_rank_between", "source_in_the_halo", "ghost_lowest_occupied",
                                  "ghost_source_in_the_halo", "ghost_source_below_the_buffer",
                                  "ghost_and_owned_share_a_source", "nothing_occupied_below"])
def test_empty_slice_aliasing_across_the_cuts(pkg, oracle, groups, case):
    vox, iso, n = _q1_volume(case)
    vol = pkg.Volume(vox)
    kw = dict(triangles=True, project=True, threshold=0.2, step=0.25, relax=0.95, max_steps=50)
    ref = _oracle(oracle, vol, iso, **kw)
    closed_pts, _ = oracle.closed_form_counts(vox, iso)
    assert (len(ref.points) < closed_pts) == (case not in ("ghost_lowest_occupied", "nothing_occupied_below"))
    for m in (n, n + 1):
        _, mesh = _group_mesh(pkg, groups(m), vol, iso, **kw)
        assert_same_mesh(mesh, ref)
    # without the quirk: the oracle's own counts (no re-use), the single context's mesh
    ex = pkg.Extractor(0)
    try:
        prm = pkg.make_params(iso, q1=False, **kw)
        ex.extract_host(vol, prm)
        single = ex.download()
    finally:
        ex.close()
    _, mesh = _group_mesh(pkg, groups(n), vol, iso, q1=False, **kw)
    assert_same_mesh(mesh, single)
    assert mesh.GetNumberOfPoints() == closed_pts


def test_one_slice_slabs_and_more_members_than_slices(pkg, oracle, groups):
    rng = np.random.default_rng(21)
    for nz, n in ((8, 8), (3, 8), (5, 3)):
        vox = (rng.random((nz, 13, 70)) < 0.35).astype(np.uint8) * 200
        vol = pkg.Volume(vox)
        kw = dict(triangles=True, project=True, threshold=0.2, step=0.24, relax=0.95, max_steps=30)
        ref = _oracle(oracle, vol, 100, **kw)
        res, mesh = _group_mesh(pkg, groups(n), vol, 100, **kw)
        assert_same_mesh(mesh, ref)
        assert len(groups(n).plan(pkg.make_desc(np.uint8, vol.dims), pkg.make_params(100, **kw))) == min(n, nz)
        with pytest.raises(pkg._abi.CuberilleError):
            groups(n).slab_result(min(n, nz))


def test_every_pixel_type_tilted_and_offset(pkg, oracle, groups):
    rng = np.random.default_rng(8)
    a = np.deg2rad(12.0)
    direction = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    base = rng.random((23, 17, 29))
    for dt in (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64, np.int64, np.uint64):
        vox = (base * 100).astype(dt)
        vol = pkg.Volume(vox, spacing=(0.9, 1.1, 0.7), origin=(3.0, -1.5, 2.25), direction=direction, index_start=(5, -3, 11))
        kw = dict(triangles=True, project=True, threshold=0.5, step=-1.0, relax=0.95, max_steps=50)
        ref = _oracle(oracle, vol, 50, **kw)
        _, mesh = _group_mesh(pkg, groups(3), vol, 50, **kw)
        assert_same_mesh(mesh, ref)


@pytest.mark.parametrize("variant", [1, 2])
def test_compiled_out_projection_branches(pkg, oracle, volumes, groups, variant):
    for name, iso in (("fuel.mha", 15), ("neghip.mha", 55)):
        vol = volumes(name)
        kw = dict(triangles=True, project=True, threshold=0.2, step=0.24, relax=0.95, max_steps=50, variant=variant)
        _, mesh = _group_mesh(pkg, groups(3), vol, iso, **kw)
        assert_same_mesh(mesh, _oracle(oracle, vol, iso, **kw))


def test_1024_marschner_lobb_chunked_slabs_equal_the_single_context(pkg, extractor, groups):
    """Slabs of more than a GiB: every member takes the chunked upload."""
    import torch
    n = 1024
    vox = torch.cat([pkg.volumes.marschner_lobb(n, a, min(a + 64, n), xp=torch, device="cuda") for a in range(0, n, 64)])
    vol = pkg.Volume(vox.cpu().numpy())
    del vox
    torch.cuda.empty_cache()
    desc = pkg.make_desc(np.float32, (n, n, n))
    prm = pkg.make_params(0.5, triangles=True, project=True, threshold=0.002, step=0.25, relax=0.95, max_steps=50)
    cuts = groups(2).plan(desc, prm)
    assert all((c[3] - c[2]) * n * n * 4 >= (1 << 30) for c in cuts)
    extractor.extract_host(vol, prm)
    single = extractor.mesh_host()
    res, mesh = _group_mesh(pkg, groups(2), vol, 0.5, triangles=True, project=True, threshold=0.002, step=0.25, relax=0.95,
                            max_steps=50)
    assert res.n_points > 10 ** 7
    assert_same_mesh(mesh, single)


def test_refusals_leave_the_group_usable(pkg, oracle, volumes, groups):
    vol = volumes("fuel.mha")
    g = groups(2)
    with pytest.raises(pkg._abi.CuberilleError) as e:
        g.extract_host(vol, pkg.make_params(15, gradient=pkg.cuberille.GRADIENT_RECURSIVE_GAUSSIAN))
    assert e.value.code == pkg._abi.ERR_ARGUMENT and "recursive-Gaussian" in str(e.value)
    lib = pkg._abi.lib()
    ctx = g.context(1)
    assert lib.cuberille_set_interpolator(ctx, pkg._abi.INTERP_BSPLINE, 3, 32, 32) == 0
    with pytest.raises(pkg._abi.CuberilleError) as e:
        g.extract_host(vol, pkg.make_params(15))
    assert e.value.code == pkg._abi.ERR_ARGUMENT and "member 1" in str(e.value) and "B-spline" in str(e.value)
    assert lib.cuberille_set_interpolator(ctx, pkg._abi.INTERP_LINEAR, 3, 0, 0) == 0
    assert lib.cuberille_hold_gradient(g.context(0), 1) == 0
    with pytest.raises(pkg._abi.CuberilleError) as e:
        g.extract_host(vol, pkg.make_params(15))
    assert e.value.code == pkg._abi.ERR_ARGUMENT and "member 0" in str(e.value) and "gradient" in str(e.value)
    assert lib.cuberille_hold_gradient(g.context(0), 0) == 0
    kw = dict(triangles=True, project=True, threshold=0.2, step=0.24, relax=0.95, max_steps=50)
    _, mesh = _group_mesh(pkg, g, vol, 15, **kw)
    assert_same_mesh(mesh, _oracle(oracle, vol, 15, **kw))


def test_a_failing_slab_drains_and_the_next_call_is_right(pkg, oracle, volumes):
    vol = volumes("neghip.mha")
    kw = dict(triangles=True, project=True, threshold=0.2, step=0.24, relax=0.95, max_steps=50)
    ref = _oracle(oracle, vol, 55, **kw)
    for slab in (1, 2):
        g = pkg.ExtractorGroup([0, 0, 0])
        try:
            g.debug_fail_alloc(slab, 0)                   # the first device allocation of that slab's worker
            with pytest.raises(pkg._abi.CuberilleError) as e:
                g.extract_host(vol, pkg.make_params(55, **kw))
            assert e.value.code == pkg._abi.ERR_HIP and ("slab %d:" % slab) in str(e.value), str(e.value)
            _, mesh = _group_mesh(pkg, g, vol, 55, **kw)
            assert_same_mesh(mesh, ref)
        finally:
            g.close()


def test_warm_up_reserves_what_the_extraction_asks_for(pkg):
    rng = np.random.default_rng(4)
    for nx in (128, 70):                                  # whole-word and ragged rows
        vox = (rng.random((40, 24, nx)) < 0.3).astype(np.uint8) * 200
        vol = pkg.Volume(vox)
        desc = pkg.make_desc(np.uint8, vol.dims)
        prm = pkg.make_params(100)
        cold = pkg.ExtractorGroup([0, 0, 0])
        warm = pkg.ExtractorGroup([0, 0, 0])
        try:
            cold.debug_fail_alloc(-1, 0)                  # every slab: its first allocation fails
            with pytest.raises(pkg._abi.CuberilleError):
                cold.extract_host(vol, prm)
            warm.warm_up(desc, prm)
            warm.debug_fail_alloc(-1, 0)                  # nothing of the upload and count allocates any more
            warm.extract_host(vol, prm)
        finally:
            cold.close()
            warm.close()


def test_filter_routes(pkg, oracle, volumes):
    vol = volumes("nucleon.mha")
    f = pkg.CuberilleImageToMeshFilter(device=0, devices=[0, 0, 0])
    f.SetInput(vol)
    f.SetIsoSurfaceValue(140)
    f.Update()
    assert f.GetLastNumberOfSlabs() == 3
    assert_same_mesh(f.GetOutput(), _oracle(oracle, vol, 140))
    f.SetReproduceStaleGradient(True)                     # a slab cannot: the single context
    f.Update()
    assert f.GetLastNumberOfSlabs() == 1
    f.SetReproduceStaleGradient(False)
    f.SetBSplineInterpolator()
    f.Update()
    assert f.GetLastNumberOfSlabs() == 1
    f.SetLinearInterpolator()
    f.SetDevices([])
    f.Update()
    assert f.GetLastNumberOfSlabs() == 1
    assert_same_mesh(f.GetOutput(), _oracle(oracle, vol, 140))


def test_reference_driver_unchanged_split(oracle, volumes, ctest_cases, tmp_path):
    """The reference's unchanged CuberilleTest01, its process told CUBERILLE_DEVICES: every CTest row passes its own
    count check, and each file equals the oracle's mesh and, byte for byte, the file of a run without the variable."""
    exe = os.path.join(REF_BIN, "CuberilleTest01")
    if not os.path.exists(exe):
        pytest.skip("reference drivers not built: build() makes oracle/_ref/ only where the reference sources are")
    # a driver compiled against a drop-in header without the group never reads the variable: it would pass the rows below
    # on one context and prove nothing (build() rebuilds the drivers when the drop-in's content changes, where the
    # reference sources are; test_unchanged_driver_of_ours_split covers the variable without them)
    syms = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True).stdout
    if "cuberille_group_extract_host" not in syms:
        pytest.skip("oracle/_ref/CuberilleTest01 was built against a drop-in header without the context group")
    for c in ctest_cases:
        args = [os.path.join(GOLDEN, "data", c["input"]), None, str(c["iso"]), str(c["points"]), str(c["cells"]),
                str(c["triangles"]), str(c["project"]), repr(c["threshold"]), repr(c["step"]), repr(c["relax"]),
                str(c["max_steps"])]
        files = {}
        for devices in (None, "0,0", "0,0,0"):
            env = dict(os.environ)
            env.pop("CUBERILLE_DEVICES", None)
            if devices:
                env["CUBERILLE_DEVICES"] = devices
            out = str(tmp_path / ("%s_%s.vtk" % (c["name"], devices or "one")))
            args[1] = out
            r = subprocess.run([exe, "Test01"] + args, capture_output=True, text=True, timeout=120, env=env)
            assert r.returncode == 0, (c["name"], devices, r.stdout[-400:], r.stderr[-400:])
            assert "Mesh has %d vertices and %d cells" % (c["points"], c["cells"]) in r.stdout
            files[devices] = open(out, "rb").read()
        assert files["0,0"] == files[None] and files["0,0,0"] == files[None], c["name"]
        pts, cells = _read_vtk_polydata(str(tmp_path / ("%s_0,0.vtk" % c["name"])))
        ref = oracle.run(volumes(c["input"]).voxels, c["iso"], c["triangles"], c["project"], c["threshold"], c["step"],
                         c["relax"], c["max_steps"])
        assert np.array_equal(cells, ref.cells.astype(np.int64)), c["name"]
        np.testing.assert_allclose(pts, ref.points, rtol=1e-6, atol=0)
    # a malformed value: the driver fails the reference's way, naming the variable
    c = ctest_cases[0]
    env = dict(os.environ, CUBERILLE_DEVICES="0;1")
    r = subprocess.run([exe, "Test01", os.path.join(GOLDEN, "data", c["input"]), str(tmp_path / "bad.vtk"), str(c["iso"]),
                        str(c["points"]), str(c["cells"])], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "CUBERILLE_DEVICES" in r.stderr


def test_unchanged_driver_of_ours_split(pkg, tmp_path):
    """itk/tests/end_to_end.cxx, which knows nothing of the group, with CUBERILLE_DEVICES in its environment: the
    filter's default devices come from the variable; the mesh written through itk::VTKPolyDataWriter and the flat file
    (the group's cuberille_group_mesh_write_vtk) agree, and both equal, byte for byte, a run without the variable.  A
    malformed value fails Update(), naming the variable."""
    exe = os.path.join(ROOT, "midas-journal-740_amd", "itk", "build", "end_to_end")
    if not os.path.exists(exe):
        pytest.skip("itk/build/end_to_end not built (build() makes it)")
    files = {}
    for devices in (None, "0,0", "0,0,0"):
        env = dict(os.environ)
        env.pop("CUBERILLE_DEVICES", None)
        if devices:
            env["CUBERILLE_DEVICES"] = devices
        prefix = str(tmp_path / ("e2e_%s" % (devices or "one")))
        r = subprocess.run([exe, "96", prefix], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (devices, r.stdout[-400:], r.stderr[-400:])
        assert '"same_bytes": true' in r.stdout
        files[devices] = (open(prefix + "_mesh.vtk", "rb").read(), open(prefix + "_flat.vtk", "rb").read())
    assert files["0,0"] == files[None] and files["0,0,0"] == files[None]
    env = dict(os.environ, CUBERILLE_DEVICES="0;1")
    r = subprocess.run([exe, "16", str(tmp_path / "bad")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "CUBERILLE_DEVICES" in r.stderr, (r.stdout[-400:], r.stderr[-400:])


def test_multi_update_driver(pkg):
    exe = os.path.join(ROOT, "midas-journal-740_amd", "itk", "build", "multi_update")
    if not os.path.exists(exe):
        pytest.skip("itk/build/multi_update not built (build() makes it)")
    r = subprocess.run([exe, "128", "0,0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-400:])
    assert '"same_bytes": true' in r.stdout and '"slabs": 2' in r.stdout
