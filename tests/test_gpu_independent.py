"""The HIP path held to the witnesses of tests/independent_ref.py DIRECTLY -- float64 numpy + scipy that share nothing with the
project -- not by way of the oracle: the device coefficient image against scipy's spline_filter; the final vertices of every
case of independent_cases() through extract_host, extract_device and count + emit, through the walk's other forms (one vertex
per lane without refills, the literal interpolation, the general-geometry kernel forced on an identity image, the
lane-per-vertex kernel of a held gradient); the stop counters; the point normals.

Every comparison is on the vertices the witness alone calls not fragile, within independent_sides.FACTOR times what
tests/golden/independent_tolerances.json records of the witnesses against the reference on the CPU; the walk starts from the
lattice points the library itself emits with the projection off."""
import numpy as np
import pytest

import independent_ref as ind
import independent_sides as sides

pytestmark = pytest.mark.gpu

CASES = ind.independent_cases()
BY_NAME = {c["name"]: c for c in CASES}
COEFFICIENT_PIXELS = ["uint8", "int16", "int32", "float32", "float64"]
# the walk's other forms: linear interpolation, default branch, central differences, the whole volume
FORM_CASES = ["ball/float32/identity", "ball/uint8/rot_a", "blob/aniso/thr0.01", "blob/start/thr0.5"]
FORMS = {"no_refill": ("proj_refill=64", "proj_chunk=64"), "refill_at_3": ("proj_refill=3", "proj_chunk=128"), "literal": ("proj_literal=1",),
         "general_geometry": ("proj_ident=0",), "held_gradient": ()}


@pytest.fixture(scope="module")
def ex(pkg):
    """A context of this module's own: views, interpolators and switches stay off the session's shared extractor."""
    pkg._abi.build()
    e = pkg.Extractor(0)
    yield e
    e.close()


def _volume(pkg, case):
    g = case["geometry"]
    return pkg.Volume(case["vox"], spacing=g.get("spacing", (1.0, 1.0, 1.0)), origin=g.get("origin", (0.0, 0.0, 0.0)),
                      direction=g.get("direction"), index_start=g.get("start", (0, 0, 0)))


def _params(pkg, case, project=True):
    return pkg.make_params(case["iso"], triangles=False, project=project, threshold=case["threshold"], step=case["step"], relax=case["relax"],
                           max_steps=case["max_steps"], variant=case["variant"], gradient=case["gradient"])


class _Settings:
    """The case's view and interpolator on the context, taken off again on the way out."""

    def __init__(self, pkg, ex, case):
        self.pkg, self.ex, self.case = pkg, ex, case

    def __enter__(self):
        view, A = self.case["view"], self.pkg._abi
        if view and view["kind"] == "border":
            self.ex.set_border(1, view["value"])
        elif view and view["kind"] == "region":
            self.ex.set_region(view["start"], view["size"])
        elif view:
            self.ex.set_band(*view["band"])
        if self.case["interp"].startswith("bspline"):
            bits = int(self.case["interp"][len("bspline"):])
            self.ex.set_interpolator(A.INTERP_BSPLINE, 3, bits, bits)

    def __exit__(self, *exc):
        self.ex.set_interpolator(self.pkg._abi.INTERP_LINEAR)
        self.ex.set_border(0, 0)
        self.ex.clear_region()
        self.ex.clear_band()
        self.ex.set_point_normals(False)
        self.ex.hold_gradient(False)
        self.ex.debug_option("defaults", 0)


def _lattice(pkg, ex, case, vol):
    """The start points: what the library emits with the projection off (and where the witness's index transform puts them)."""
    ex.extract_host(vol, _params(pkg, case, project=False))
    start = ex.download().points
    img = ind.image_of(case)
    eps = 2.0 ** -24 * max(1.0, float(np.abs(start).max())) / float(img.spacing.min())
    assert len(start) >= 64 and img.lattice_residual(start).max() <= 4.0 * eps, case["name"]
    return start


def _held(case, witnessed, points, res, what):
    wit, walk, fragile = witnessed
    kept = ~fragile
    assert points.shape == walk.points.shape, what
    with np.errstate(invalid="ignore"):
        dev = wit.img.voxels_between(points, walk.points)[kept]
    print(what, "%.3g voxels over %d of %d vertices (allowed %.3g)" % (np.nanmax(dev), kept.sum(), len(kept), sides.allowed(sides.family_of(case))))
    assert np.isfinite(dev).all() and dev.max() <= sides.allowed(sides.family_of(case)), what
    if case["variant"] != 2:
        F = int(fragile.sum())
        T, S = walk.count(ind.THRESHOLD, kept), walk.count(ind.STEPS, kept)
        assert T <= res.proj_stop_threshold <= T + F, (what, T, F, res.proj_stop_threshold)
        assert S <= res.proj_stop_steps <= S + F, (what, S, F, res.proj_stop_steps)


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_final_vertices_counters_and_normals(pkg, ex, name):
    import torch
    case = BY_NAME[name]
    vol = _volume(pkg, case)
    with _Settings(pkg, ex, case):
        start = _lattice(pkg, ex, case, vol)
        witnessed = sides.witnessed(case, start)
        wit, walk, fragile = witnessed
        assert ind.case_conditions(walk, fragile, case) is None
        prm = _params(pkg, case)
        normals = case["variant"] == 0 and case["interp"] == "linear" and not case["gradient"]
        ex.set_point_normals(normals)
        res = ex.extract_host(vol, prm)
        _held(case, witnessed, ex.download().points, res, name + " extract_host")
        if normals:
            # the angle to the witness's normal at the witness's vertex; NaN nowhere on vertices that are not fragile
            want, norm = wit.normal(walk.points)
            angle = ind.angle_between(ex.download_normals(), want)[~fragile]
            print(name, "normals: %.3g rad (allowed %.3g)" % (np.nanmax(angle), sides.allowed("normals_angle")))
            assert np.isfinite(angle).all() and angle.max() <= sides.allowed("normals_angle"), name
        ex.set_point_normals(False)
        desc = pkg.make_desc(vol.voxels.dtype, vol.dims, vol.spacing, vol.origin, vol.direction, vol.index_start)
        dev = torch.from_numpy(vol.voxels.reshape(-1)).cuda()
        torch.cuda.synchronize()
        res = ex.extract_device(dev.data_ptr(), desc, prm)
        _held(case, witnessed, ex.download().points, res, name + " extract_device")
        ex.count(dev.data_ptr(), desc, prm)
        res = ex.emit(0)
        _held(case, witnessed, ex.download().points, res, name + " count + emit")


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", FORM_CASES)
def test_other_forms_of_the_walk(pkg, ex, name, form):
    case = BY_NAME[name]
    assert case["variant"] == 0 and case["interp"] == "linear" and not case["gradient"] and not case["view"]
    vol = _volume(pkg, case)
    with _Settings(pkg, ex, case):
        start = _lattice(pkg, ex, case, vol)
        witnessed = sides.witnessed(case, start)
        for o in FORMS[form]:
            option, _, value = o.partition("=")
            ex.debug_option(option, int(value))
        if form == "held_gradient":
            # the first projecting extraction keeps its gradient image, this one walks along it: the image is the same one
            ex.hold_gradient(True)
            ex.extract_host(vol, _params(pkg, case))
            assert ex.gradient_held == vol.voxels.shape
        res = ex.extract_host(vol, _params(pkg, case))
        _held(case, witnessed, ex.download().points, res, "%s %s" % (name, form))


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("dtype", COEFFICIENT_PIXELS)
def test_coefficient_image_against_scipy(pkg, ex, dtype, bits):
    """Extractor.bspline_coefficients against spline_filter(order=3, mode='mirror') on the pixels cast to float64: lines
    shorter than the horizon of 18 (the full mirror sum), of 18, 19 and 20 around it, longer ones (the truncated sum), and
    x-lines of 259 over several LDS tiles."""
    A = pkg._abi
    try:
        for shape in sides.COEFFICIENT_SHAPES:
            vox = sides.coefficient_volume(shape, dtype)
            vol = pkg.Volume(vox)
            flat = np.sort(vox.ravel())
            ex.set_interpolator(A.INTERP_BSPLINE, 3, bits, bits)
            res = ex.extract_host(vol, pkg.make_params(flat[len(flat) // 2].item()))
            assert res.n_points > 0, shape
            got = ex.bspline_coefficients(vol.dims, bits)
            dev = sides.coefficient_deviation(got, vox)
            print(dtype, bits, shape, "%.3g of the largest coefficient (allowed %.3g)" % (dev, sides.allowed("coefficients_%d" % bits)))
            assert dev <= sides.allowed("coefficients_%d" % bits), (dtype, bits, shape)
    finally:
        ex.set_interpolator(A.INTERP_LINEAR)


def test_no_normal_exactly_where_the_witness_gradient_is_zero(pkg, ex):
    """The two sheets (quirk Q4), projection off: the normal is NaN exactly at the lattice points where the witness's
    interpolated gradient is exactly zero, and within tolerance of the witness's everywhere else."""
    vox = ind.two_sheets()
    try:
        ex.set_point_normals(True)
        ex.extract_host(pkg.Volume(vox), pkg.make_params(100, triangles=False, project=False))
        pts, got = ex.download().points, ex.download_normals()
    finally:
        ex.set_point_normals(False)
    img = ind.Image(vox)
    want, norm = ind.normal_function(img, ind.central_gradient(img))(pts.astype(np.float64))
    zero = norm == 0.0
    assert 8 <= zero.sum() < len(pts)
    assert np.array_equal(np.isnan(got).any(axis=1), zero)
    assert ind.angle_between(got[~zero], want[~zero]).max() <= sides.allowed("normals_angle")
