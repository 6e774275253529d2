"""Point scalars on the GPU (cuberille_set_point_scalars): the library's row against the reference of tests/point_scalars_ref.py
-- the oracle's interpolation primitive plus the inside test, held to an independent witness by tests/test_point_scalars.py --
evaluated at the library's own downloaded points and compared bit for bit, a NaN matching any NaN.  Every test also holds
points, cells and counters to the bytes of the same extraction with the setting off.
"""
import ctypes as C

import numpy as np
import pytest

import keep_ref
import point_scalars_ref as ref
from conftest import point_bytes
from point_scalars_ref import same_scalars
from test_normals import GEOMETRIES, STEP, blob, zero_gradient_volume
from test_point_scalars import ALL_TYPES, CASE1_GEO, CASE2_SHAPE, CASE2_START, CASE2_DIRECTIONS, case2_geo, typed_noise

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 4
KW = dict(threshold=0.5, step=-1.0, relax=0.95, max_steps=50)
COUNTERS = ("n_points", "n_cells", "verts_per_cell", "proj_iterations", "proj_stop_threshold", "proj_stop_steps", "n_escaped")
NAN = float("nan")


@pytest.fixture()
def ex(pkg):
    e = pkg.Extractor(0)
    yield e
    e.close()


def counters(res):
    return {k: int(getattr(res, k)) for k in COUNTERS}


def volume_of(pkg, b, geo):
    g = ref.geo_of(geo)
    return pkg.Volume(b, spacing=g["spacing"], origin=g["origin"], direction=g["direction"], index_start=g["index_start"])


def off_then_on(ex, run, image, outside=NAN, what=""):
    """run() once with the setting off and once with it on (image: what Extractor.set_point_scalars takes): the mesh and the
    counters must be the same bytes.  Returns the mesh, the result and the row of the second run."""
    ex.set_point_scalars(None)
    r0 = run()
    m0, c0 = ex.download(), counters(r0)
    ex.set_point_scalars(image, outside)
    r1 = run()
    m1, row = ex.download(), ex.download_point_scalars()
    assert point_bytes(m0.points) == point_bytes(m1.points), (what, "the setting moved a point")
    assert m0.cells.tobytes() == m1.cells.tobytes(), (what, "the setting moved a cell")
    assert c0 == counters(r1), (what, c0, counters(r1))
    assert row.shape == (len(m1.points),) and row.dtype == np.float64
    return m1, r1, row


def params(pkg, iso, project=1, triangles=1, **kw):
    return pkg.make_params(iso, **dict(KW, project=project, triangles=triangles, **kw))


# ---- 1: all ten pixel types ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ALL_TYPES, ids=lambda d: np.dtype(d).name)
def test_all_pixel_types(pkg, oracle, ex, dtype):
    vox, iso = blob()
    b = typed_noise(dtype)
    for project in (1, 0):
        mesh, res, row = off_then_on(ex, lambda: ex.extract_host(pkg.Volume(vox), params(pkg, iso, project)), volume_of(pkg, b, CASE1_GEO))
        inside, fragile = ref.check(oracle, row, b, mesh.points, what=(np.dtype(dtype).name, project), **CASE1_GEO)
        assert len(row) == 302 and int(inside.sum()) == (149 if project else 146) and np.isnan(row[~inside]).all()
        if not project:            # 104 lattice points lie exactly on a face of the inside test: >= against < decided exactly
            ci = ref.continuous_index(mesh.points, **CASE1_GEO)
            assert int(np.any((ci == -0.5) | (ci == np.array([9, 7, 5]) - 0.5), axis=1).sum()) == 104


# ---- 2: geometries -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("direction", sorted(CASE2_DIRECTIONS))
@pytest.mark.parametrize("geometry", ["spacing", "rotated"])
def test_geometries(pkg, oracle, ex, geometry, direction):
    vox, iso = blob()
    vol = pkg.Volume(vox, index_start=CASE2_START, **GEOMETRIES[geometry])
    b, geo = typed_noise(np.float32, CASE2_SHAPE), case2_geo(geometry, direction)
    for project in (1, 0):
        mesh, res, row = off_then_on(ex, lambda: ex.extract_host(vol, params(pkg, iso, project)), volume_of(pkg, b, geo), -7.5)
        inside, fragile = ref.check(oracle, row, b, mesh.points, -7.5, what=(geometry, direction, project), **geo)
        n = len(row)
        print(geometry, direction, project, "inside", int(inside.sum()), "of", n, "fragile", int(fragile.sum()))
        assert inside.sum() >= n / 10 and (~inside).sum() >= n / 10 and not fragile.any()


# ---- 3, 4: thin images and row ends ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(5, 7, 1), (5, 1, 9), (1, 7, 9), (1, 1, 1)], ids=lambda s: "%dx%dx%d" % s[::-1])
def test_thin_second_image(pkg, oracle, ex, shape, dtype):
    """lo = hi = 0 along an axis; with nx = 1 the row of one pixel, which no pair is loaded from."""
    vox, iso = blob()
    b = typed_noise(dtype, shape)
    # (the one pixel a quarter voxel from a lattice corner of the surface: on the CPU 3 of the oracle's points are inside, 1 with
    #  the projection off)
    geo = dict(origin=(8.75, 4.75, 1.75) if shape == (1, 1, 1) else CASE1_GEO["origin"])
    for project in (1, 0):
        mesh, res, row = off_then_on(ex, lambda: ex.extract_host(pkg.Volume(vox), params(pkg, iso, project)), volume_of(pkg, b, geo))
        inside, _ = ref.check(oracle, row, b, mesh.points, what=(shape, project), **geo)
        print(shape, np.dtype(dtype).name, project, "inside", int(inside.sum()))
        assert inside.any()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=lambda d: np.dtype(d).name)
def test_row_ends(pkg, oracle, ex, dtype):
    """nx of 2, 3, 63, 64, 65: every byte residue of a row's start occurs (rows lie nx pixels apart), and B ends inside the mesh
    along x, so that points fall in the last column's cell -- hi clamped to lo, the pair taken one pixel further down."""
    vox, iso = blob()
    for nx in (2, 3, 63, 64, 65):
        b = typed_noise(dtype, (6, 8, nx), seed=nx)
        # the last column at x = 6.25 (blob: 14 wide) whatever nx: the lattice corners at x = 6.5 fall in its cell, a quarter in
        geo = dict(origin=(6.25 - (nx - 1), 2.0, 2.0))
        for project in (1, 0):
            mesh, res, row = off_then_on(ex, lambda: ex.extract_host(pkg.Volume(vox), params(pkg, iso, project)), volume_of(pkg, b, geo))
            inside, _ = ref.check(oracle, row, b, mesh.points, what=(nx, project), **geo)
            ci = ref.continuous_index(mesh.points, **geo)
            last = inside & (ci[:, 0] >= nx - 1)
            print(np.dtype(dtype).name, nx, project, "inside", int(inside.sum()), "last column's cell", int(last.sum()))
            assert last.any(), (nx, project)


# ---- 5, 6: NaN vertices and the outside value ------------------------------------------------------------------------------------

def test_nan_vertices_get_the_outside_value(pkg, oracle, ex):
    vox, iso = zero_gradient_volume()
    b = typed_noise(np.float32, tuple(vox.shape))
    # (the one-step walk of test_normals: within the default threshold these vertices would not move at all)
    prm = pkg.make_params(iso, threshold=0.0, step=STEP, relax=0.0, max_steps=0, project=1, triangles=1)
    mesh, res, row = off_then_on(ex, lambda: ex.extract_host(pkg.Volume(vox), prm), pkg.Volume(b), 123.25)
    nan = np.isnan(mesh.points).any(axis=1)
    assert nan.any() and not nan.all()
    assert (row[nan] == 123.25).all()
    ref.check(oracle, row, b, mesh.points, 123.25, what="zero gradient")


def test_outside_value_bit_for_bit(pkg, oracle, ex):
    vox, iso = blob()
    b = typed_noise(np.int16)
    payload = 0x7ff80000deadbeef
    for bits in (None, 0x8000000000000000, int(np.array([1e300]).view(np.uint64)[0]), payload):
        outside = NAN if bits is None else float(np.array([bits], dtype=np.uint64).view(np.float64)[0])
        want_bits = int(np.array([outside]).view(np.uint64)[0]) if bits is None else bits
        mesh, res, row = off_then_on(ex, lambda: ex.extract_host(pkg.Volume(vox), params(pkg, iso, 1)), volume_of(pkg, b, CASE1_GEO), outside)
        want, inside, _ = ref.scalars(oracle, b, mesh.points, want_bits, **CASE1_GEO)
        assert (~inside).sum() > 100
        ref.same_scalars_bits(row[~inside], want[~inside], hex(want_bits))
        same_scalars(row, want, hex(want_bits))


# ---- 7: several workgroups, the volume itself by device pointer, the routes -------------------------------------------------------

def gradient_noise(shape=(36, 40, 48)):
    rng = np.random.default_rng(7)
    z, y, x = np.mgrid[0:shape[0], 0:shape[1], 0:shape[2]].astype(np.float64)
    f = 60.0 + 1.5 * x + 0.7 * y - 0.9 * z + rng.random(shape) * 90.0
    return np.clip(f, 0, 255).astype(np.uint8), 128


def test_launch_shapes_and_routes(pkg, oracle, ex):
    import torch
    vox, iso = gradient_noise()
    vol = pkg.Volume(vox)
    desc = pkg.make_desc(vox.dtype, vol.dims)
    dev = torch.from_numpy(vox.reshape(-1)).cuda()
    torch.cuda.synchronize()
    prm = params(pkg, iso, 1)
    image = (dev.data_ptr(), desc)                       # B is the volume being extracted: the residual use

    def stream():
        return ex.extract_stream(desc, lambda dst, z0, z1: dst.__setitem__(slice(None), vox[z0:z1]), prm)

    def count_emit(offset, ahead):
        ex.count(dev.data_ptr(), desc, prm)
        if ahead:
            ex.emit_points()
        return ex.emit(offset)

    want = first = None
    for name, run in (("extract_host", lambda: ex.extract_host(vol, prm)),
                      ("extract_device", lambda: ex.extract_device(dev.data_ptr(), desc, prm)),
                      ("extract_device again", lambda: ex.extract_device(dev.data_ptr(), desc, prm)),
                      ("extract_stream", stream),
                      ("count + emit_points + emit(2^32 + 5)", lambda: count_emit(2 ** 32 + 5, True)),
                      ("count + emit", lambda: count_emit(0, False))):
        mesh, res, row = off_then_on(ex, run, image, what=name)
        if want is None:
            n = len(mesh.points)
            assert n > 4096 and n % 256 != 0, n
            want, inside, _ = ref.scalars(oracle, vox, mesh.points)
            first = point_bytes(mesh.points)
            assert ex.point_scalars_device()
            residual = np.abs(row[inside] - iso)
            print("points", n, "inside", int(inside.sum()), "median |f(v) - iso|", float(np.median(residual)))
        assert point_bytes(mesh.points) == first, name
        same_scalars(row, want, name)
        if "2^32" in name:
            assert int(mesh.cells.min()) >= 2 ** 32 + 5
    # an empty mesh: a null pointer and an empty download
    empty = pkg.Volume(np.zeros((9, 10, 11), dtype=np.uint8))
    mesh, res, row = off_then_on(ex, lambda: ex.extract_host(empty, prm), image, what="empty")
    assert res.n_points == 0 and row.shape == (0,) and ex.point_scalars_device() is None


# ---- 8: independence of views ------------------------------------------------------------------------------------------------

def test_views_bspline_and_the_other_outputs(pkg, oracle, ex):
    vox, iso = blob()
    vol = pkg.Volume(vox)
    b = typed_noise(np.float32)
    image = volume_of(pkg, b, CASE1_GEO)
    prm = params(pkg, iso, 1)

    def held(what, p=prm):
        mesh, res, row = off_then_on(ex, lambda: ex.extract_host(vol, p), image, what=what)
        assert len(row) > 50
        ref.check(oracle, row, b, mesh.points, what=what, **CASE1_GEO)
        return mesh, row

    ex.set_border(1, 0.0)
    held("border")
    ex.set_border(0, 0)
    ex.set_region((2, 1, 1), (10, 9, 8))
    held("region")
    ex.clear_region()
    ex.set_band(40.0, 200.0, 1, 0)
    held("band", params(pkg, 1, 1))
    ex.clear_band()
    ex.set_interpolator(pkg._abi.INTERP_BSPLINE, 3, 32, 32)
    held("bspline")
    ex.set_interpolator(pkg._abi.INTERP_LINEAR)
    for variant in (1, 2):
        held("variant %d" % variant, params(pkg, iso, 1, variant=variant))
    held("recursive gaussian", params(pkg, iso, 1, gradient=1))
    ex.hold_gradient(True)
    ex.extract_host(vol, prm)                # (the context's first projecting extraction: every later one walks its gradient)
    held("held gradient")
    ex.hold_gradient(False)
    # normals, cell pixels and components on beside it: their rows are the bytes of the run without the point scalars
    ex.set_point_normals(True)
    ex.set_cell_pixels(True)
    ex.set_components(True)
    ex.set_point_scalars(None)
    ex.extract_host(vol, prm)
    others = (ex.download_normals().tobytes(), ex.download_cell_pixels().tobytes(), [a.tobytes() for a in ex.download_components()])
    mesh, row = held("all four")
    assert (ex.download_normals().tobytes(), ex.download_cell_pixels().tobytes(), [a.tobytes() for a in ex.download_components()]) == others


# ---- 9: the row across extractions -------------------------------------------------------------------------------------------

def test_row_across_extractions_and_memory(pkg, oracle):
    big, biso = gradient_noise()
    small, siso = blob()
    b1, b2 = typed_noise(np.float32), typed_noise(np.uint16, (6, 6, 6), seed=3)
    e = pkg.Extractor(0)
    try:
        def run(vox, iso, b, geo, what):
            e.extract_host(pkg.Volume(vox), params(pkg, iso, 1))
            pts, row = e.download().points, e.download_point_scalars()
            ref.check(oracle, row, b, pts, what=what, **geo)
            return len(row)

        for _ in range(2):                       # (the second one takes the blind launches and their covering sizes)
            e.extract_host(pkg.Volume(big), params(pkg, biso, 1))
        before = e.device_bytes()
        e.set_point_scalars(volume_of(pkg, b1, CASE1_GEO))
        n_big = run(big, biso, b1, CASE1_GEO, "large")
        assert e.device_bytes() - before >= 8 * n_big + b1.nbytes
        run(small, siso, b1, CASE1_GEO, "small after large")
        e.set_point_scalars(volume_of(pkg, b2, dict(origin=(4.0, 4.0, 3.0))))           # replaced by another image of another type
        run(small, siso, b2, dict(origin=(4.0, 4.0, 3.0)), "replaced")
        run(big, biso, b2, dict(origin=(4.0, 4.0, 3.0)), "large again")
        e.set_point_scalars(None)
        for fn in (e.download_point_scalars, e.point_scalars_device):
            with pytest.raises(pkg._abi.CuberilleError) as err:
                fn()
            assert err.value.code == STATE and "no point scalars: the last extraction ran with the setting off (cuberille_set_point_scalars)" in str(err.value)
        assert e.device_bytes() == before
        e.extract_host(pkg.Volume(big), params(pkg, biso, 1))
        assert e.device_bytes() == before
        with pytest.raises(pkg._abi.CuberilleError) as err:
            e.download_point_scalars()
        assert err.value.code == STATE
        e.set_point_scalars(volume_of(pkg, b1, CASE1_GEO))
        with pytest.raises(pkg._abi.CuberilleError) as err:      # (set, but the last extraction ran without)
            e.download_point_scalars()
        assert err.value.code == STATE
        run(small, siso, b1, CASE1_GEO, "on again")
    finally:
        e.close()


# ---- 10: keep ----------------------------------------------------------------------------------------------------------------

def two_objects():
    vox = np.zeros((12, 14, 20), dtype=np.uint8)
    z, y, x = np.mgrid[0:12, 0:14, 0:20]
    vox[(x - 5) ** 2 + (y - 6) ** 2 + (z - 6) ** 2 <= 16] = 200
    vox[(x - 14) ** 2 + (y - 7) ** 2 + (z - 5) ** 2 <= 5] = 180
    vox[2, 2, 17] = 220
    return vox, 100


def test_keep_components(pkg, oracle, ex):
    vox, iso = two_objects()
    b = typed_noise(np.float64, (8, 9, 10))
    geo = dict(origin=(3.0, 2.0, 2.0))
    ex.set_components(True)
    ex.set_point_normals(True)
    ex.set_point_scalars(volume_of(pkg, b, geo), -0.0)

    def fresh():
        ex.extract_host(pkg.Volume(vox), params(pkg, iso, 1))
        mesh, row = ex.download(), ex.download_point_scalars()
        want, inside, _ = ref.scalars(oracle, b, mesh.points, -0.0, **geo)
        same_scalars(row, want, "before the keep")
        assert inside.any() and not inside.all()
        return mesh, want

    def kp_of(rule, n=0):
        pc, cc, counts = ex.download_components()
        return keep_ref.decide(rule, counts, n)[pc]

    mesh, want = fresh()
    assert ex.n_components() == 3
    # largest
    kp = kp_of("largest")
    ex.keep_components("largest")
    row = ex.download_point_scalars()
    assert row.tobytes() == want[kp].tobytes() and len(row) == int(ex.result.n_points) and 0 < len(row) < len(want)
    assert point_bytes(ex.download().points) == point_bytes(mesh.points[kp])
    # ... the kept row is the reference at the kept points, and a second keep composes
    same_scalars(row, ref.scalars(oracle, b, ex.download().points, -0.0, **geo)[0], "after the keep")
    ex.keep_components("largest")
    assert ex.download_point_scalars().tobytes() == row.tobytes()
    # min_cells: the two larger ones, then the larger one of those
    mesh, want = fresh()
    pc, cc, counts = ex.download_components()
    n = int(np.sort(counts)[1])
    kp = kp_of("min_cells", n)
    ex.keep_components("min_cells", n)
    row = ex.download_point_scalars()
    assert row.tobytes() == want[kp].tobytes() and ex.n_components() == 2
    kp2 = kp_of("largest")
    ex.keep_components("largest")
    assert ex.download_point_scalars().tobytes() == row[kp2].tobytes()
    # a keep that keeps everything moves no byte
    mesh, want = fresh()
    ptr = ex.point_scalars_device()
    ex.keep_components("min_cells", 0)
    assert ex.point_scalars_device() == ptr and ex.download_point_scalars().tobytes() == want.tobytes()
    # a keep to nothing: an empty download
    ex.keep_components("min_cells", 10 ** 9)
    assert ex.download_point_scalars().shape == (0,) and ex.point_scalars_device() is None
    # the next extraction is a fresh one
    fresh()


# ---- 11: VTK -----------------------------------------------------------------------------------------------------------------

def test_vtk_block(pkg, oracle, ex, tmp_path):
    vox, iso = blob()
    b = typed_noise(np.float64)
    for others in (False, True):
        ex.set_point_normals(others)
        ex.set_components(others)
        ex.set_point_scalars(None)
        ex.extract_host(pkg.Volume(vox), params(pkg, iso, 1))
        off, on = str(tmp_path / "off.vtk"), str(tmp_path / "on.vtk")
        ex.write_vtk(off)
        ex.set_point_scalars(volume_of(pkg, b, CASE1_GEO))
        ex.extract_host(pkg.Volume(vox), params(pkg, iso, 1))
        row = ex.download_point_scalars()
        ex.write_vtk(on)
        a, t = open(off, "rb").read(), open(on, "rb").read()
        n = len(row)
        head = b"SCALARS point_scalar double 1\nLOOKUP_TABLE default\n"
        if not others:
            assert b"POINT_DATA" not in a
            head = b"POINT_DATA %d\n" % n + head
        at = t.index(head)
        body = t[at + len(head):].split(b"\n")
        values = np.array([float(v) for v in body[:n]], dtype=np.float64)
        same_scalars(values, row, "the values parse back")
        assert np.isnan(row).any() and np.isfinite(row).any()
        rest = b"\n".join(body[n:])
        assert t[:at] + rest == a, "the file with the setting on is the file with it off plus the block"
        if others:                   # last in POINT_DATA: behind the normals and the point labels, ahead of CELL_DATA
            assert t.index(b"NORMALS") < t.index(b"SCALARS component") < at < t.index(b"CELL_DATA")


# ---- 12: refusals ------------------------------------------------------------------------------------------------------------

def test_every_refusal_then_a_plain_extraction(pkg, oracle, ex):
    import torch
    vox, iso = blob()
    vol = pkg.Volume(vox)
    desc = pkg.make_desc(vox.dtype, vol.dims)
    dev = torch.from_numpy(vox.reshape(-1)).cuda()
    torch.cuda.synchronize()
    prm = params(pkg, iso, 1)
    b = typed_noise(np.float32)
    image = volume_of(pkg, b, CASE1_GEO)

    def refused(fn, code=ARG):
        with pytest.raises(pkg._abi.CuberilleError) as e:
            fn()
        assert e.value.code == code and "point scalars" in str(e.value), str(e.value)

    def plain():
        ex.extract_host(vol, prm)
        m = ex.download()
        ref.check(oracle, ex.download_point_scalars(), b, m.points, what="plain", **CASE1_GEO)
        return m

    ex.set_point_scalars(image)
    first = plain()
    slab = pkg._abi.Slab(global_nz=40, z_begin=10, own_z0=12, own_z1=16)
    refused(lambda: ex.extract_device(dev.data_ptr(), desc, prm, slab))
    refused(lambda: ex.count(dev.data_ptr(), desc, prm, slab))
    refused(lambda: ex.step_begin(dev.data_ptr(), desc, prm))
    refused(lambda: ex.step_classify(dev.data_ptr(), desc, prm))
    plain()
    g = pkg.ExtractorGroup([0, 0])
    try:
        g.set_point_scalars(image)
        with pytest.raises(pkg._abi.CuberilleError) as e:
            g.extract_host(vol, prm)
        assert e.value.code == ARG and "point scalars" in str(e.value)
        g.set_point_scalars(None)
        g.extract_host(vol, prm)
        assert point_bytes(g.download().points) == point_bytes(first.points)
    finally:
        g.close()
    # a bad description, a null pointer, a bad location: the setting stays as it was
    lib, ctx = ex._lib, ex._ctx
    good = pkg.make_desc(np.float32, (9, 7, 5), origin=CASE1_GEO["origin"])
    host = np.ascontiguousarray(b)
    for change in (lambda d: setattr(d, "pixel_type", 77), lambda d: d.dims.__setitem__(1, 0), lambda d: d.spacing.__setitem__(2, 0.0),
                   lambda d: d.direction.__setitem__(slice(0, 9), [0.0] * 9), lambda d: d.index_start.__setitem__(0, 2 ** 31)):
        d = pkg.make_desc(np.float32, (9, 7, 5), origin=CASE1_GEO["origin"])
        change(d)
        refused(lambda: pkg._abi.check(ctx, lib.cuberille_set_point_scalars(ctx, C.byref(d), C.c_void_p(host.ctypes.data), 0, 0.0)))
    refused(lambda: pkg._abi.check(ctx, lib.cuberille_set_point_scalars(ctx, C.byref(good), None, 0, 0.0)))
    refused(lambda: pkg._abi.check(ctx, lib.cuberille_set_point_scalars(ctx, C.byref(good), C.c_void_p(host.ctypes.data), 2, 0.0)))
    m = plain()
    # a capacity too small
    out = np.empty(len(m.points), dtype=np.float64)
    refused(lambda: pkg._abi.check(ctx, lib.cuberille_point_scalars_download(ctx, C.c_void_p(out.ctypes.data), out.nbytes - 1)))
    pkg._abi.check(ctx, lib.cuberille_point_scalars_download(ctx, C.c_void_p(out.ctypes.data), out.nbytes))
    assert out.tobytes() == ex.download_point_scalars().tobytes()
    assert point_bytes(plain().points) == point_bytes(first.points)


def test_python_filter_mirror(pkg, oracle):
    vox, iso = blob()
    b = typed_noise(np.int16)
    f = pkg.CuberilleImageToMeshFilter(device=0)
    f.SetInput(pkg.Volume(vox))
    f.SetIsoSurfaceValue(iso)
    f.Update()
    assert f.GetPointScalars() is None
    points = f.GetOutput().points
    f.SetPointScalarImage(volume_of(pkg, b, CASE1_GEO))
    f.SetPointScalarOutsideValue(-1.0)
    f.Update()
    assert point_bytes(f.GetOutput().points) == point_bytes(points)
    ref.check(oracle, f.GetPointScalars(), b, points, -1.0, what="filter mirror", **CASE1_GEO)
    f.SetPointScalarImage(None)
    f.Update()
    assert f.GetPointScalars() is None
