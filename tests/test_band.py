"""cuberille_set_band without a GPU: the validator, its Python mirror, the exported symbols -- and the identity the band
sweep rests on, shown on the oracle.

The feature's definition: with a band set, an extraction of I gives the mesh of
    B(u) = (lower <= I(u) && I(u) <= upper) ? inside : outside                (all four values in I's pixel type)
what itk::BinaryThresholdImageFilter makes of I.  B takes two values, so the sweep's inside(u) = !(B(u) < iso) is
`bin` = !(inside < iso) in the band and `bout` = !(outside < iso) outside it: band(u) XOR bout where they differ, a constant
where they are equal.  The oracle has no window on its inside set; a mesh without projection is a function of that set alone
(and of nothing else of the pixel values), so the identity is checked as: the oracle's mesh of B at iso equals its mesh of
the PREDICATE volume (band XOR bout as uint8 0 / 1) at iso 1 -- and both constant cases give no mesh at all.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

PIXELS = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64, np.int64, np.uint64]
INTEGERS = [d for d in PIXELS if np.dtype(d).kind in "iu"]
ARG = 1
# (inside, outside, iso): bin != bout plain, bin != bout inverted, and other values than 0 / 1
VALUE_CHOICES = [(1, 0, 1), (0, 1, 1), (200, 10, 100)]


def code(pkg, dtype):
    return int(pkg.make_desc(dtype, (1, 1, 1)).pixel_type)


def raw_check(pkg, pixel_type, band):
    """cuberille_band_check itself: doubles, and the 64 bits a 64-bit integer type would hold."""
    v = (C.c_double * 4)(*[float(x) for x in band])
    ints = []
    for x in band:
        try:
            ints.append(((int(x) + (1 << 63)) % (1 << 64)) - (1 << 63))
        except (OverflowError, ValueError):
            ints.append(0)
    return pkg._abi.lib().cuberille_band_check(pixel_type, v, (C.c_int64 * 4)(*ints))


def both(pkg, dtype, band):
    """The validator's verdict (True: accepted), asserted equal to check_band's."""
    rc = raw_check(pkg, code(pkg, dtype), band)
    assert rc in (0, ARG), rc
    if rc == 0:
        pkg.check_band(code(pkg, dtype), band)
    else:
        with pytest.raises(pkg._abi.CuberilleError) as e:
            pkg.check_band(code(pkg, dtype), band)
        assert e.value.code == ARG and "band" in str(e.value)
        assert b"band" in pkg._abi.lib().cuberille_last_error(None)
    return rc == 0


def test_symbols_in_header_binding_and_library(pkg):
    header = open(os.path.join(ROOT, "include", "cuberille_hip.h")).read()
    for name in ("cuberille_set_band", "cuberille_band_check"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in pkg._abi.EXPORTS
        assert getattr(pkg._abi.lib(), name) is not None
    assert pkg._abi.lib().cuberille_abi_version() == pkg._abi.ABI_VERSION == 13


@pytest.mark.parametrize("dtype", PIXELS, ids=[np.dtype(d).name for d in PIXELS])
def test_validator_per_pixel_type(pkg, dtype):
    dt = np.dtype(dtype)
    assert both(pkg, dtype, (1, 1, 1, 0))                       # a single label
    assert both(pkg, dtype, (3, 5, 1, 0))
    assert both(pkg, dtype, (3, 5, 0, 1))
    assert not both(pkg, dtype, (5, 3, 1, 0))                   # lower > upper: ITK throws
    assert not both(pkg, dtype, (float("nan"), 3, 1, 0))        # NaN bounds
    assert not both(pkg, dtype, (1, float("nan"), 1, 0))
    if dt.kind in "iu":
        info = np.iinfo(dt)
        assert both(pkg, dtype, (int(info.min), int(info.max), 1, 0))            # the whole range, 64-bit ends included
        assert both(pkg, dtype, (int(info.max), int(info.max), int(info.max), int(info.min)))
        for k in range(4):                                      # one past either end, and a fraction, in every place
            for bad in (int(info.max) + 1, int(info.min) - 1, 0.5):
                band = [1, 2, 1, 0]
                band[k] = bad
                assert not both(pkg, dtype, tuple(band)), (k, bad)
        if dt.kind == "u":
            assert not both(pkg, dtype, (-1, 3, 1, 0))          # -1 in the unsigned types
        else:
            assert both(pkg, dtype, (-1, 3, 1, 0))
        assert not both(pkg, dtype, (1, float("inf"), 1, 0))
    else:
        assert both(pkg, dtype, (-0.5, 0.25, 1.5, -2.0))
        assert both(pkg, dtype, (float("-inf"), float("inf"), 1, 0))
        assert both(pkg, dtype, (0.0, 1.0, float("nan"), float("inf")))          # values are the image's to hold
        assert both(pkg, dtype, (-0.0, 0.0, 1, 0))


def test_validator_named_cases(pkg):
    assert not both(pkg, np.uint8, (0, 256, 1, 0))              # 256 in uint8
    assert both(pkg, np.uint8, (0, 255, 1, 0))
    assert both(pkg, np.uint16, (0, 256, 1, 0))
    assert not both(pkg, np.int8, (-129, 0, 1, 0))
    # 2^63 through vi: a uint64 holds it (the same 64 bits as -2^63), an int64 does not; 2^64 wraps to 0 and is refused
    assert both(pkg, np.uint64, (1 << 63, (1 << 64) - 1, 1, 0))
    assert both(pkg, np.uint64, (5, 1 << 63, 1, 0))             # ordered as UNSIGNED 64-bit values
    assert not both(pkg, np.uint64, (1 << 63, 5, 1, 0))
    assert not both(pkg, np.int64, (0, 1 << 63, 1, 0))
    assert both(pkg, np.int64, (-(1 << 63), (1 << 63) - 1, 1, 0))
    assert not both(pkg, np.uint64, (0, 1 << 64, 1, 0))
    assert both(pkg, np.int64, ((1 << 62) + 1, (1 << 62) + 3, 1, 0))            # not doubles: told apart by vi
    assert not both(pkg, np.int64, ((1 << 62) + 3, (1 << 62) + 1, 1, 0))
    assert raw_check(pkg, 99, (1, 2, 1, 0)) == ARG              # unknown pixel type
    assert pkg._abi.lib().cuberille_band_check(0, None, None) == ARG
    pkg.check_band(0, None)                                     # no band: nothing to check


def blobs(shape, seed, labels=6):
    """A seeded blob field: labels 0 .. labels-1, every label present, blobs a few voxels across.  [z, y, x]"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(shape)
    for ax in range(3):                                         # a separable box blur, three voxels wide, twice
        for _ in range(2):
            f = (np.roll(f, 1, ax) + f + np.roll(f, -1, ax)) / 3.0
    q = np.quantile(f, np.linspace(0, 1, labels + 1)[1:-1])
    return np.digitize(f, q).astype(np.uint8), f


def band_image(vox, lower, upper, inside, outside):
    """B, as itk::BinaryThresholdImageFilter<Image<T>, Image<T>> documents it: all four values in the pixel type."""
    dt = vox.dtype
    lo, up = np.asarray(lower, dtype=dt), np.asarray(upper, dtype=dt)
    band = (lo <= vox) & (vox <= up)                            # NaN fails both comparisons: outside
    return np.where(band, np.asarray(inside, dtype=dt), np.asarray(outside, dtype=dt)).astype(dt), band


def predicate(band, inside, outside, iso, dt):
    """What the band sweep writes: band XOR bout where bin != bout, the constant bout elsewhere."""
    iso_t = np.asarray(iso, dtype=dt)
    bin_, bout = not (np.asarray(inside, dtype=dt) < iso_t), not (np.asarray(outside, dtype=dt) < iso_t)
    return (band ^ bout) if bin_ != bout else np.full(band.shape, bout)


@pytest.mark.parametrize("values", VALUE_CHOICES, ids=["1-0-iso1", "0-1-iso1", "200-10-iso100"])
def test_sweep_identity_on_the_oracle(oracle, values):
    inside, outside, iso = values
    labels, f = blobs((17, 23, 40), 7)
    assert set(np.unique(labels)) == set(range(6))
    fields = [(labels, 2, 3), (labels, 4, 4), (labels.astype(np.int16), 0, 1),
              ((f / f.std() * 30.0).astype(np.float32), -20.0, 35.5)]
    nan = (f / f.std() * 30.0).astype(np.float32)
    nan[3, 5, 7] = np.nan
    nan[8:10, 9:12, 20:25] = np.nan
    fields.append((nan, -20.0, 35.5))
    for vox, lower, upper in fields:
        B, band = band_image(vox, lower, upper, inside, outside)
        P = predicate(band, inside, outside, iso, vox.dtype)
        assert P.any() and not P.all()
        if np.isnan(vox).any():
            assert not band[np.isnan(vox)].any()                # NaN is outside the band ...
            assert (P[np.isnan(vox)] == (outside >= iso)).all() # ... and inside after the inversion
        for tri in (True, False):
            a = oracle.run(B, iso, triangles=tri, project=False)
            b = oracle.run(P.astype(np.uint8), 1, triangles=tri, project=False)
            assert len(a.cells) > 0
            assert np.array_equal(a.cells, b.cells) and a.points.tobytes() == b.points.tobytes(), (vox.dtype, lower, upper, tri)


@pytest.mark.parametrize("values", [(5, 3, 2), (5, 3, 9), (1, 1, 1)], ids=["all-inside", "all-outside", "equal-values"])
def test_constant_cases_give_empty_meshes(oracle, values):
    """bin == bout: both of B's values lie on one side of the iso value, the bit volume is constant -- no mesh either way
    (quirk Q2 for the all-inside volume)."""
    inside, outside, iso = values
    labels, _ = blobs((17, 23, 40), 7)
    B, band = band_image(labels, 2, 3, inside, outside)
    P = predicate(band, inside, outside, iso, labels.dtype)
    assert P.all() or not P.any()
    for vol, level in ((B, iso), (P.astype(np.uint8), 1)):
        m = oracle.run(vol, level, project=False)
        assert len(m.points) == 0 and len(m.cells) == 0
