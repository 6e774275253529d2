"""The B-spline walk on the GPU (cuberille_set_interpolator, CUBERILLE_INTERP_BSPLINE): the device coefficient image and
the device walk held bit for bit to itk_lite's BSplineInterpolateImageFunction through itk/tests/bspline_walk.cxx, the
drop-in filter's device route against its host route, and the refusals of the C ABI."""
import os
import subprocess

import numpy as np
import pytest

import bspline_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 3), (17, 18, 19), (40, 1, 2), (3, 17, 40), (18, 19, 1), (2, 40, 17), (19, 3, 18)]
PIXELS = [np.uint8, np.int16, np.float32, np.float64, np.uint64]
GEOMETRIES = {
    "anisotropic": dict(spacing=(0.7, 1.3, 2.1), origin=(-3.5, 2.25, 10.0)),
    "rotated": dict(spacing=(1.1, 0.9, 1.7), origin=(1.0, -2.0, 0.5),
                    direction=[[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]]),
    "start_index": dict(spacing=(1.0, 2.0, 0.5), origin=(0.25, 0.0, -1.0), start=(5, -3, 12)),
}


@pytest.fixture(scope="module")
def ex(pkg):
    """A context of this module's own: the B-spline setting stays off the session's shared extractor."""
    pkg._abi.build()
    e = pkg.Extractor(0)
    yield e
    e.close()


def _volume(rng, shape, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.uint64:
        return rng.integers(0, 2 ** 64 - 1, size=shape, dtype=np.uint64, endpoint=True)
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        return rng.integers(info.min, info.max, size=shape, dtype=dtype, endpoint=True)
    return (rng.standard_normal(shape) * 100.0).astype(dtype)


def _iso(vol):
    v = np.sort(vol.ravel())
    return v[len(v) // 2].item()          # the median: half the voxels inside, vertices wherever a line has both kinds


def _same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.size == 0:
        return
    bad = a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)
    n = int(bad.any(axis=1).sum())
    assert n == 0, "%s: %d of %d values differ" % (what, n, a.size)


def _bspline_extract(pkg, ex, vol, bits, **prm):
    ex.set_interpolator(pkg._abi.INTERP_BSPLINE, 3, bits, bits)
    try:
        res = ex.extract_host(vol, pkg.make_params(**prm))
        mesh = ex.download()
    finally:
        ex.set_interpolator(pkg._abi.INTERP_LINEAR)
    return res, mesh


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("dtype", PIXELS, ids=lambda d: np.dtype(d).name)
def test_device_coefficients_equal_the_class(pkg, ex, tmp_path, dtype, bits):
    rng = np.random.default_rng(17 + bits)
    for shape in SHAPES:
        vox = _volume(rng, shape, dtype)
        vol = pkg.Volume(vox)
        res, _ = _bspline_extract(pkg, ex, vol, bits, iso=_iso(vox))
        assert res.n_points > 0, shape
        got = ex.bspline_coefficients(vol.dims, bits)
        _same_bytes(got, ref.run_coeffs(tmp_path, vox, bits), "%s %s" % (np.dtype(dtype).name, shape))


@pytest.mark.parametrize("bits", [32, 64])
def test_device_coefficients_of_a_large_volume(pkg, ex, tmp_path, bits):
    # x-lines of 259 voxels span nine LDS tiles; more than 65 536 rows
    n = (257, 258, 259)
    zz, yy, xx = np.meshgrid(*[np.arange(k, dtype=np.float32) for k in n], indexing="ij")
    vox = (np.sin(xx * 0.05) * 40 + np.cos(yy * 0.031) * 30 + zz * 0.1).astype(np.float32)
    vol = pkg.Volume(vox)
    res, _ = _bspline_extract(pkg, ex, vol, bits, iso=5.0)
    assert res.n_points > 0
    _same_bytes(ex.bspline_coefficients(vol.dims, bits), ref.run_coeffs(tmp_path, vox, bits), "256^3")


def _filter(tmp, volume_args, route, threads, bits, row, tri, extra=()):
    pts, cells = str(tmp / ("p_%s.raw" % route)), str(tmp / ("c_%s.raw" % route))
    r = subprocess.run([ref.walk_exe(), "filter"] + list(volume_args[:1]) +
                       [route, str(threads), str(bits), repr(float(row["iso"])), str(int(tri)), str(int(row["project"])),
                        repr(float(row["threshold"])), repr(float(row["step"])), repr(float(row["relax"])), str(int(row["max_steps"])),
                        pts, cells] + list(volume_args[1:]) + list(extra),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    n_p, n_c = (int(v) for v in r.stdout.split()[:2])
    p = np.fromfile(pts, dtype=np.float32).reshape(-1, 3)
    c = np.fromfile(cells, dtype=np.uint64)
    assert len(p) == n_p
    return p, c.reshape(n_c, -1) if n_c else c.reshape(0, 3 if tri else 4)


def _abi_mesh(pkg, ex, vol, bits, row, tri):
    res, mesh = _bspline_extract(pkg, ex, vol, bits, iso=row["iso"], triangles=tri, project=bool(row["project"]),
                                 threshold=row["threshold"], step=row["step"], relax=row["relax"], max_steps=row["max_steps"])
    if row["project"]:
        assert res.proj_stop_threshold + res.proj_stop_steps == res.n_points
    return mesh


@pytest.mark.parametrize("bits", [32, 64])
def test_ctest_rows_equal_the_host_walk(pkg, ex, volumes, ctest_cases, tmp_path, bits):
    assert len(ctest_cases) == 19
    for row in ctest_cases:
        vol = volumes(row["input"])
        for tri in (True, False):
            mesh = _abi_mesh(pkg, ex, vol, bits, row, tri)
            p, c = _filter(tmp_path, [os.path.join(GOLDEN, "data", row["input"])], "host", 4, bits, row, tri)
            what = "%s tri=%d" % (row["name"], tri)
            _same_bytes(mesh.points, p, what + " points")
            _same_bytes(mesh.cells.astype(np.uint64), c, what + " cells")
            if bool(tri) == bool(row["triangles"]):
                assert (mesh.GetNumberOfPoints(), mesh.GetNumberOfCells()) == (row["points"], row["cells"]), what


def _blob(n=(29, 23, 31)):
    zz, yy, xx = np.meshgrid(*[np.arange(k, dtype=np.float64) for k in n], indexing="ij")
    c = [(k - 1) / 2.0 for k in n]
    r = np.sqrt(((zz - c[0]) / 1.0) ** 2 + ((yy - c[1]) / 0.8) ** 2 + ((xx - c[2]) / 1.1) ** 2)
    return (100.0 - 9.0 * r + 3.0 * np.sin(xx * 0.7) * np.cos(yy * 0.5)).astype(np.float32)


ROW = dict(iso=40.0, project=1, threshold=0.05, step=0.3, relax=0.95, max_steps=60)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_geometries_equal_the_host_walk(pkg, ex, tmp_path, geo, bits):
    vox = _blob()
    g = GEOMETRIES[geo]
    vol = pkg.Volume(vox, spacing=g.get("spacing", (1, 1, 1)), origin=g.get("origin", (0, 0, 0)), direction=g.get("direction"),
                     index_start=g.get("start", (0, 0, 0)))
    raw = str(tmp_path / "blob.raw")
    vox.tofile(raw)
    nz, ny, nx = vox.shape
    args = [raw, "raw", "f32", str(nx), str(ny), str(nz), "geometry", ref.geometry_arg(**g)]
    for tri in (True, False):
        mesh = _abi_mesh(pkg, ex, vol, bits, ROW, tri)
        p, c = _filter(tmp_path, args, "host", 8, bits, ROW, tri)
        _same_bytes(mesh.points, p, "%s tri=%d points" % (geo, tri))
        _same_bytes(mesh.cells.astype(np.uint64), c, "%s tri=%d cells" % (geo, tri))


@pytest.mark.parametrize("bits", [32, 64])
def test_filter_device_route_equals_host_route(tmp_path, ctest_cases, bits):
    ml = [r for r in ctest_cases if r["input"] == "marschnerlobb.mha" and r["project"]][0]
    args = [os.path.join(GOLDEN, "data", "marschnerlobb.mha")]
    for tri in (True, False):
        ph, ch = _filter(tmp_path, args, "host", 4, bits, ml, tri)
        pd, cd = _filter(tmp_path, args, "device", 1, bits, ml, tri)
        _same_bytes(pd, ph, "points tri=%d" % tri)
        _same_bytes(cd, ch, "cells tri=%d" % tri)
    # a rotated geometry with a start index, through a raw file
    vox = _blob()
    raw = str(tmp_path / "blob.raw")
    vox.tofile(raw)
    nz, ny, nx = vox.shape
    g = dict(GEOMETRIES["rotated"], start=(2, -7, 4))
    args = [raw, "raw", "f32", str(nx), str(ny), str(nz), "geometry", ref.geometry_arg(**g)]
    ph, ch = _filter(tmp_path, args, "host", 4, bits, ROW, True)
    pd, cd = _filter(tmp_path, args, "device", 1, bits, ROW, True)
    _same_bytes(pd, ph, "rotated points")
    _same_bytes(cd, ch, "rotated cells")


def test_other_spline_orders_take_the_host_walk(tmp_path, ctest_cases):
    ml = [r for r in ctest_cases if r["input"] == "marschnerlobb.mha" and r["project"]][0]
    args = [os.path.join(GOLDEN, "data", "marschnerlobb.mha")]
    pd, cd = _filter(tmp_path, args, "device", 1, 32, ml, True, extra=["order", "2"])
    ph, ch = _filter(tmp_path, args, "host", 4, 32, ml, True, extra=["order", "2"])
    assert len(pd) == ml["points"] and len(cd) > 0
    _same_bytes(pd, ph, "order 2 points")
    _same_bytes(cd, ch, "order 2 cells")
    # (order 2 walks elsewhere than order 3)
    p3, _ = _filter(tmp_path, args, "host", 4, 32, ml, True)
    assert not np.array_equal(p3.view(np.uint32), pd.view(np.uint32))


@pytest.mark.parametrize("bits", [32, 64])
def test_every_whole_volume_entry_point_walks_the_bspline(pkg, ex, bits):
    """extract_device, extract_stream and a one-rank step give the mesh extract_host gives (which the tests above hold to
    the class); the step runs behind a linear one on the same context, whose sizes would let it launch blindly -- the
    B-spline walk must take the sized path and still come out right."""
    import torch
    A = pkg._abi
    vox = _blob()
    g = GEOMETRIES["rotated"]
    vol = pkg.Volume(vox, spacing=g["spacing"], origin=g["origin"], direction=g["direction"])
    prm = dict(ROW, triangles=True)
    res_h, want = _bspline_extract(pkg, ex, vol, bits, **prm)
    assert res_h.n_points > 0 and res_h.proj_stop_threshold > 0
    desc = pkg.make_desc(vox.dtype, vol.dims, vol.spacing, vol.origin, vol.direction)
    dev = torch.from_numpy(vox).cuda()
    torch.cuda.synchronize()

    def same(got, what):
        _same_bytes(got.points, want.points, what + " points")
        _same_bytes(got.cells, want.cells, what + " cells")

    ex.set_interpolator(A.INTERP_BSPLINE, 3, bits, bits)
    try:
        res = ex.extract_device(dev.data_ptr(), desc, pkg.make_params(**prm))
        assert res.proj_stop_threshold + res.proj_stop_steps == res.n_points == res_h.n_points
        same(ex.download(), "extract_device")
        assert ex.bspline_coefficients().shape == vox.shape

        def source(dst, z0, z1):
            dst[...] = vox[z0:z1]
        ex.extract_stream(desc, source, pkg.make_params(**prm))
        same(ex.download(), "extract_stream")

        for interp in (A.INTERP_LINEAR, A.INTERP_BSPLINE):     # the linear step leaves the history a blind launch reads
            ex.set_interpolator(interp, 3, bits, bits)
            ptr, _ = ex.step_begin(dev.data_ptr(), desc, pkg.make_params(**prm))
            res, done = ex.step_end(ptr, 1, 0)
            if not done:
                res = ex.emit(0)
        assert res.proj_stop_threshold + res.proj_stop_steps == res.n_points
        same(ex.download(), "step")
    finally:
        ex.set_interpolator(A.INTERP_LINEAR)


def test_refusals_leave_the_context_usable(pkg, volumes):
    vol = volumes("fuel.mha")
    prm = dict(iso=15, threshold=0.2, step=0.24, relax=0.9, max_steps=100)
    fresh = pkg.Extractor(0)
    try:
        fresh.extract_host(vol, pkg.make_params(**prm))
        want = fresh.download()
    finally:
        fresh.close()
    ctx = pkg.Extractor(0)
    A = pkg._abi
    try:
        def refused(fn):
            with pytest.raises(A.CuberilleError) as e:
                fn()
            assert e.value.code == A.ERR_ARGUMENT, e.value
            ctx.set_interpolator(A.INTERP_LINEAR)
            ctx.hold_gradient(False)
            ctx.extract_host(vol, pkg.make_params(**prm))
            got = ctx.download()
            assert np.array_equal(got.cells, want.cells)
            assert np.array_equal(got.points.view(np.uint32), want.points.view(np.uint32))

        refused(lambda: ctx.set_interpolator(A.INTERP_BSPLINE, 2, 32, 32))
        refused(lambda: ctx.set_interpolator(A.INTERP_BSPLINE, 3, 32, 64))
        refused(lambda: ctx.set_interpolator(A.INTERP_BSPLINE, 3, 16, 16))
        refused(lambda: ctx.set_interpolator(7, 3, 32, 32))

        def with_bspline(**kw):
            def go():
                ctx.set_interpolator(A.INTERP_BSPLINE, 3, 32, 32)
                ctx.extract_host(vol, pkg.make_params(**dict(prm, **kw)))
            return go
        refused(with_bspline(variant=1))         # CUBERILLE_PROJECT_ADVANCED
        refused(with_bspline(gradient=1))

        def holding():
            ctx.hold_gradient(True)
            with_bspline()()
        refused(holding)

        def slab():
            import torch
            ctx.set_interpolator(A.INTERP_BSPLINE, 3, 32, 32)
            vox = torch.from_numpy(np.ascontiguousarray(vol.voxels)).cuda()
            torch.cuda.synchronize()
            desc = pkg.make_desc(vol.voxels.dtype, vol.dims, vol.spacing, vol.origin, vol.direction)
            nz = vol.dims[2]
            s = A.Slab()
            s.global_nz, s.z_begin, s.own_z0, s.own_z1 = nz, 0, 0, nz // 2
            ctx.extract_device(vox.data_ptr(), desc, pkg.make_params(**prm), slab=s)
        refused(slab)
        # the B-spline works again on the same context after all of that
        ctx.set_interpolator(A.INTERP_BSPLINE, 3, 32, 32)
        res = ctx.extract_host(vol, pkg.make_params(**prm))
        assert res.proj_stop_threshold + res.proj_stop_steps == res.n_points == want.GetNumberOfPoints()
    finally:
        ctx.close()


def test_filter_mirror_routes_through_the_library(pkg, volumes, ctest_cases, tmp_path):
    ml = [r for r in ctest_cases if r["input"] == "marschnerlobb.mha" and r["project"]][0]
    f = pkg.CuberilleImageToMeshFilter(device=0)
    f.SetInput(volumes(ml["input"]))
    f.SetIsoSurfaceValue(ml["iso"])
    f.SetGenerateTriangleFaces(True)
    f.SetProjectVertexSurfaceDistanceThreshold(ml["threshold"])
    f.SetProjectVertexStepLength(ml["step"])
    f.SetProjectVertexStepLengthRelaxationFactor(ml["relax"])
    f.SetProjectVertexMaximumNumberOfSteps(ml["max_steps"])
    f.SetBSplineInterpolator(3, np.float32, np.float32)
    f.Update()
    p, c = _filter(tmp_path, [os.path.join(GOLDEN, "data", ml["input"])], "host", 4, 32, ml, True)
    _same_bytes(f.GetOutput().points, p, "points")
    f.SetLinearInterpolator()
    f.Update()
    assert not np.array_equal(f.GetOutput().points.view(np.uint32), p.view(np.uint32))
