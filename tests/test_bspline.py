"""The B-spline interpolator without a GPU: itk_lite's BSplineInterpolateImageFunction (itk/itk_lite/itkBSplineLite.h,
through itk/tests/bspline_walk.cxx) held bit for bit to the numpy restatement in tests/bspline_ref.py, properties of the
spline that need nobody's memory of ITK, and the new symbols of the C ABI."""
import os
import re

import numpy as np
import pytest

import bspline_ref as ref

ROOT = ref.ROOT
# every line length 1, 2, 3, 17, 18, 19, 40 along every axis (numpy shapes are z, y, x): N = 1 is left alone, N <= 18
# takes the full mirror sum of the causal init, N >= 19 the truncated one
SHAPES = [(1, 2, 3), (17, 18, 19), (40, 1, 2), (3, 17, 40), (18, 19, 1), (2, 40, 17), (19, 3, 18)]
PIXELS = [np.uint8, np.int16, np.float32, np.float64, np.uint64]


def _volume(rng, shape, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.uint64:
        return rng.integers(0, 2 ** 64 - 1, size=shape, dtype=np.uint64, endpoint=True)
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        return rng.integers(info.min, info.max, size=shape, dtype=dtype, endpoint=True)
    return (rng.standard_normal(shape) * 100.0).astype(dtype)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    bad = a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)
    nbad = int(bad.any(axis=1).sum())
    assert nbad == 0, "%d of %d values differ" % (nbad, a.size)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("dtype", PIXELS, ids=lambda d: np.dtype(d).name)
def test_coefficients_match_restatement(tmp_path, dtype, bits):
    rng = np.random.default_rng(7 + bits)
    for shape in SHAPES:
        vol = _volume(rng, shape, dtype)
        got = ref.run_coeffs(tmp_path, vol, bits)
        _same_bits(got, ref.coefficients(vol, np.float64 if bits == 64 else np.float32))


GEOMETRIES = {
    "identity": dict(),
    "anisotropic": dict(spacing=(0.7, 1.3, 2.1), origin=(-3.5, 2.25, 10.0)),
    "rotated": dict(spacing=(1.1, 0.9, 1.7), origin=(1.0, -2.0, 0.5),
                    direction=[[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]]),
    "start_index": dict(spacing=(1.0, 2.0, 0.5), origin=(0.25, 0.0, -1.0), start=(5, -3, 12)),
}


def _points(rng, shape, geo, n=400):
    """Physical points whose continuous indices lie inside, on the samples and edges of, and outside the buffer."""
    nz, ny, nx = shape
    start = np.asarray(geo.get("start", (0, 0, 0)), dtype=np.float64)
    size = np.array([nx, ny, nz], dtype=np.float64)
    ci = np.concatenate([
        start + rng.uniform(0, 1, (n, 3)) * (size - 1),                      # inside
        start + rng.integers(0, [nx, ny, nz], (n // 4, 3)).astype(np.float64),   # on samples
        start + rng.uniform(-1.5 * size, 2.5 * size, (n, 3)),              # far outside (mirror, several periods)
        start + np.array([[0, 0, 0], size - 1, [-0.5, -0.25, -1.0], size - 0.5, size, [-1, -1, -1]], dtype=np.float64),
    ])
    spacing = np.asarray(geo.get("spacing", (1.0, 1.0, 1.0)))
    direction = np.asarray(geo.get("direction", np.eye(3)))
    origin = np.asarray(geo.get("origin", (0.0, 0.0, 0.0)))
    return origin + (ci * spacing) @ direction.T


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=lambda d: np.dtype(d).name)
def test_values_match_restatement(tmp_path, geo, bits, dtype):
    rng = np.random.default_rng(11)
    shape = (9, 13, 7)
    vol = _volume(rng, shape, dtype)
    g = GEOMETRIES[geo]
    pts = _points(rng, shape, g)
    got = ref.run_eval(tmp_path, vol, bits, pts, ref.geometry_arg(**g))
    ctype = np.float64 if bits == 64 else np.float32
    want = ref.evaluate(ref.coefficients(vol, ctype), pts, ctype=ctype, **g)
    _same_bits(got, want)


# Lines of up to 18 pixels take the exact mirror sum: the samples come back within rounding -- float coefficients carry
# about 1e-7 of the image's magnitude each, so a small sample beside large ones is held to 1e-5 of that magnitude.  Longer
# lines take ITK's truncated power sum (m_Tolerance = 1e-10: the terms beyond z^18 are dropped), which leaves an error of
# about 1e-10 of the magnitude in the coefficients: a relative 1e-12 cannot hold there for doubles, they get that bound.
@pytest.mark.parametrize("bits,shape,tol", [(32, (11, 6, 17), 1e-5), (64, (11, 6, 17), 1e-12),
                                            (32, (23, 6, 40), 1e-5), (64, (23, 6, 40), 1e-9)])
def test_samples_are_reproduced_at_integer_indices(tmp_path, bits, shape, tol):
    rng = np.random.default_rng(3)
    vol = (rng.uniform(1.0, 100.0, shape)).astype(np.float64 if bits == 64 else np.float32)
    zz, yy, xx = np.meshgrid(*[np.arange(n) for n in vol.shape], indexing="ij")
    pts = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1).astype(np.float64)
    got = ref.run_eval(tmp_path, vol, bits, pts, ref.geometry_arg())
    np.testing.assert_allclose(got, vol.ravel().astype(np.float64), rtol=0, atol=tol * float(np.abs(vol).max()))


# A constant image: with float coefficients the coefficient image IS the constant, bit for bit, on every line length; the
# values then differ from it by the rounding of the 64-tap sum alone.  With double coefficients the truncated causal init
# of the lines longer than 18 (see above) leaves about 1e-10 of the constant.  (Exactly the constant back everywhere, as one
# might hope, is not what ITK's algorithm gives.)
@pytest.mark.parametrize("bits,tol", [(32, 1e-14), (64, 1e-9)])
def test_constant_image_is_reproduced(tmp_path, bits, tol):
    vol = np.full((7, 20, 18), 42.0, dtype=np.float32)
    if bits == 32:
        assert np.array_equal(ref.run_coeffs(tmp_path, vol, 32), vol)
    rng = np.random.default_rng(5)
    pts = _points(rng, vol.shape, {}, n=200)
    got = ref.run_eval(tmp_path, vol, bits, pts, ref.geometry_arg())
    np.testing.assert_allclose(got, 42.0, rtol=tol, atol=0)


# Away from every border (the mirror is not a ramp; its effect decays as |z|^d = 0.268^d) a linear ramp comes back
@pytest.mark.parametrize("bits,rtol", [(32, 1e-5), (64, 1e-11)])
def test_linear_ramp_is_reproduced_away_from_the_border(tmp_path, bits, rtol):
    n = 64
    zz, yy, xx = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    vol = (10.0 + 0.5 * xx + 1.25 * yy - 0.75 * zz + 40.0).astype(np.float64 if bits == 64 else np.float32)
    rng = np.random.default_rng(9)
    ci = rng.uniform(26.0, 37.0, (300, 3))
    got = ref.run_eval(tmp_path, vol, bits, ci, ref.geometry_arg())
    want = 10.0 + 0.5 * ci[:, 0] + 1.25 * ci[:, 1] - 0.75 * ci[:, 2] + 40.0
    np.testing.assert_allclose(got, want, rtol=rtol, atol=0)


def test_header_and_binding_export_the_interpolator_symbols(pkg):
    with open(os.path.join(ROOT, "include", "cuberille_hip.h")) as f:
        text = f.read()
    for name in ("cuberille_set_interpolator", "cuberille_bspline_coefficients", "cuberille_bspline_coefficients_info"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in pkg._abi.EXPORTS, name
    assert re.search(r"CUBERILLE_INTERP_LINEAR = 0, CUBERILLE_INTERP_BSPLINE = 1", text)
    assert (pkg._abi.INTERP_LINEAR, pkg._abi.INTERP_BSPLINE) == (0, 1)
    assert pkg._abi.ABI_VERSION == 13 and "#define CUBERILLE_ABI_VERSION 13" in text


def test_filter_mirror_takes_only_what_the_library_implements(pkg):
    f = pkg.CuberilleImageToMeshFilter.__new__(pkg.CuberilleImageToMeshFilter)
    f._bspline = None
    f.SetBSplineInterpolator(3, np.float64, np.float64)
    assert f._bspline == (64, 64)
    f.SetBSplineInterpolator(coordinate=32, coefficient=32)
    assert f._bspline == (32, 32)
    for bad in (dict(order=2), dict(coordinate=np.float32, coefficient=np.float64), dict(coordinate=16, coefficient=16)):
        with pytest.raises(ValueError):
            f.SetBSplineInterpolator(**bad)
    f.SetLinearInterpolator()
    assert f._bspline is None
