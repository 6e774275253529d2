"""The reference of the point scalars (cuberille_set_point_scalars): for every point of a mesh the value of a second image B.

1. the inside test in float64 numpy: ci = inv(direction @ diag(spacing)) @ (p - origin), inside when
   index_start - 0.5 <= ci < index_start + n - 0.5 on every axis (a NaN fails it);
2. inside, cuberille_oracle_interpolate on B at the float32 point widened to double -- the primitive tests/test_oracle.py
   pins --, called with the description built once, as normals_ref.interpolated does;
3. outside, the caller's outside value, bit for bit.

The reference's ci does not round like the kernel's under a non-unit matrix (numpy's inverse and product against the
library's cofactor inverse and its sum in a fixed order), so a point whose reference ci lies within FRAGILE of a face of the
inside test on any axis is *fragile*: either outcome is accepted for it.  That is a condition on the point, not a measurement
of the library.  Under an identity matrix ci = p - origin exactly, no point is fragile and the comparison is exact.
"""
import ctypes as C

import numpy as np

FRAGILE = 1e-6
GEO = dict(spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=np.eye(3), index_start=(0, 0, 0))


def geo_of(kw):
    g = dict(GEO)
    g.update({k: v for k, v in kw.items() if k in GEO and v is not None})
    return g


def unit_matrix(**kw):
    g = geo_of(kw)
    return np.array_equal(np.asarray(g["direction"], dtype=np.float64).reshape(3, 3) @ np.diag(g["spacing"]), np.eye(3))


def continuous_index(points, **kw):
    """float64 [n, 3]: the continuous index of each float32 point in B's INDEX space (the origin is the position of index 0)."""
    g = geo_of(kw)
    p = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    cv = p - np.asarray(g["origin"], dtype=np.float64)
    if unit_matrix(**kw):
        return cv
    m = np.linalg.inv(np.asarray(g["direction"], dtype=np.float64).reshape(3, 3) @ np.diag(np.asarray(g["spacing"], dtype=np.float64)))
    with np.errstate(all="ignore"):
        return cv @ m.T


def inside_and_fragile(b, points, **kw):
    """(inside bool[n], fragile bool[n]) of the points against image b ([z, y, x])."""
    g = geo_of(kw)
    ci = continuous_index(points, **kw)
    n = np.array(b.shape[::-1], dtype=np.float64)
    lo = np.asarray(g["index_start"], dtype=np.float64) - 0.5
    hi = lo + n
    with np.errstate(all="ignore"):
        inside = np.all((lo <= ci) & (ci < hi), axis=1)
        if unit_matrix(**kw):
            fragile = np.zeros(len(ci), dtype=bool)
        else:
            fragile = np.any((np.abs(ci - lo) <= FRAGILE) | (np.abs(ci - hi) <= FRAGILE), axis=1)
    return inside, fragile


def interpolated(oracle, b, points, **kw):
    """float64 [n]: cuberille_oracle_interpolate(B, p) at every float32 point widened to double, whether inside or not (outside
    the oracle's interpolation clamps as ITK 3's does; NaN points give 0-weight garbage the caller never looks at)."""
    g = geo_of(kw)
    fn = oracle.lib().cuberille_oracle_interpolate
    img, keep = oracle._image(b, g["spacing"], g["origin"], g["direction"], g["index_start"])
    ref = C.byref(img)
    p = (C.c_double * 3)()
    out = np.empty(len(points), dtype=np.float64)
    for n, v in enumerate(np.asarray(points, dtype=np.float32).reshape(-1, 3)):
        if np.isnan(v).any():
            out[n] = np.nan
            continue
        p[0], p[1], p[2] = float(v[0]), float(v[1]), float(v[2])
        out[n] = fn(ref, p)
    return out


def as_bits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).view(np.uint64)


def outside_array(n, outside):
    """n copies of the 64 bits of `outside` (a float, or a uint64 bit pattern given as an int)."""
    bits = np.uint64(outside) if isinstance(outside, (int, np.integer)) else as_bits(np.array([outside]))[0]
    return np.full(n, bits, dtype=np.uint64).view(np.float64)


def scalars(oracle, b, points, outside=float("nan"), **kw):
    """(want float64[n], inside bool[n], fragile bool[n]): the row the library must leave for `points`."""
    inside, fragile = inside_and_fragile(b, points, **kw)
    value = interpolated(oracle, b, points, **kw)
    want = outside_array(len(inside), outside)
    want[inside] = value[inside]
    return want, inside, fragile


def same_scalars(got, want, what=""):
    """64-bit patterns equal, a NaN matching any NaN."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (as_bits(got) != as_bits(want)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), "%s: %d point scalars differ in their bits, first at %s: %r / %r" % (
        what, int(bad.sum()), np.argwhere(bad)[0], got[bad][0], want[bad][0])


def same_scalars_bits(got, want, what=""):
    """64-bit patterns equal, NaNs included (the outside value's payload)."""
    bad = as_bits(got) != as_bits(want)
    assert not bad.any(), "%s: %d point scalars differ in their bits, first at %s" % (what, int(bad.sum()), np.argwhere(bad)[0])


def check(oracle, got, b, points, outside=float("nan"), what="", max_fragile=0.01, **kw):
    """got against the reference: exact (same_scalars) at every point that is not fragile; at a fragile point either the
    interpolated value or the outside value.  Returns (inside, fragile)."""
    want, inside, fragile = scalars(oracle, b, points, outside, **kw)
    got = np.ascontiguousarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if unit_matrix(**kw):
        assert not fragile.any()
    else:
        assert fragile.sum() <= max_fragile * max(len(fragile), 1), (what, "fragile points", int(fragile.sum()), len(fragile))
    same_scalars(got[~fragile], want[~fragile], what)
    if fragile.any():
        value, out = interpolated(oracle, b, points, **kw), outside_array(len(want), outside)
        for i in np.flatnonzero(fragile):
            ok_in = as_bits(got[i:i + 1])[0] == as_bits(value[i:i + 1])[0] or (np.isnan(got[i]) and np.isnan(value[i]))
            ok_out = as_bits(got[i:i + 1])[0] == as_bits(out[i:i + 1])[0] or (np.isnan(got[i]) and np.isnan(out[i]))
            assert ok_in or ok_out, (what, "fragile point", int(i), got[i], value[i])
    return inside, fragile
