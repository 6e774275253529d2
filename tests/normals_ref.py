"""The reference of the point normals (cuberille_set_point_normals): N(p) built from the two oracle primitives that
tests/test_oracle.py pins, not restated by hand.

1. the float gradient image: cuberille_oracle_gradient_at_index at every voxel, with the image's geometry (I6);
2. per component, cuberille_oracle_interpolate(component volume, p, geometry, index_start) (I4, I5, I7: the sum in double in
   counter order, zero weights skipped, stopped once the weights sum to exactly 1);
3. narrowed to float32;
4. Normalize() (I8): the double sqrt of the sum of squares, float32(double(c) / norm) -- no zero guard (quirk Q4: 0 / 0 is NaN).

The two primitives are the C symbols behind oracle.gradient_at_index and oracle.interpolate, called with the image
description built once per volume instead of once per voxel (the per-call wrappers rebuild it: two orders of magnitude
slower over a whole image, the same bits).
"""
import ctypes as C

import numpy as np

GEO = dict(spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=np.eye(3))


def _geo(kw):
    g = dict(GEO)
    g.update({k: v for k, v in kw.items() if k in GEO and v is not None})
    return g


def gradient_image(oracle, vol, **kw):
    """float32 [nz, ny, nx, 3]: oracle.gradient_at_index at every voxel (the start index does not enter a gradient)."""
    g = _geo(kw)
    img, keep = oracle._image(vol, g["spacing"], g["origin"], g["direction"])
    fn = oracle.lib().cuberille_oracle_gradient_at_index
    ref = C.byref(img)
    nz, ny, nx = keep.shape
    idx, out = (C.c_int64 * 3)(), (C.c_float * 3)()
    rows = []
    for k in range(nz):
        idx[2] = k
        for j in range(ny):
            idx[1] = j
            for i in range(nx):
                idx[0] = i
                fn(ref, idx, out)
                rows.append((out[0], out[1], out[2]))
    return np.array(rows, dtype=np.float32).reshape(nz, ny, nx, 3)


def interpolated(oracle, grad, points, index_start=(0, 0, 0), **kw):
    """float32 [n, 3]: per component oracle.interpolate of the gradient image at every point, narrowed to float32."""
    g = _geo(kw)
    fn = oracle.lib().cuberille_oracle_interpolate
    comps = [oracle._image(np.ascontiguousarray(grad[..., c]), g["spacing"], g["origin"], g["direction"], index_start) for c in range(3)]
    refs = [C.byref(img) for img, _ in comps]
    p = (C.c_double * 3)()
    acc = np.empty((len(points), 3), dtype=np.float32)
    for n, v in enumerate(np.asarray(points, dtype=np.float32)):
        p[0], p[1], p[2] = float(v[0]), float(v[1]), float(v[2])
        acc[n, 0], acc[n, 1], acc[n, 2] = fn(refs[0], p), fn(refs[1], p), fn(refs[2], p)
    return acc


def normalize(acc):
    """I8 on float32 [n, 3]: ((0 + c0 c0) + c1 c1) + c2 c2 in double, its IEEE sqrt, float32(double(c) / norm); NaN where the
    gradient is zero."""
    a = np.asarray(acc, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        sq = a[:, 0] * a[:, 0]
        sq = sq + a[:, 1] * a[:, 1]
        sq = sq + a[:, 2] * a[:, 2]
        return (a / np.sqrt(sq)[:, None]).astype(np.float32)


def normals(oracle, vol, points, index_start=(0, 0, 0), grad=None, **kw):
    """N(p) for every row of `points` (float32 [n, 3], the three floats as a points buffer holds them) in the image `vol`
    ([z, y, x]) with spacing / origin / direction / index_start.  grad: gradient_image(vol, geometry) when the caller has it."""
    if grad is None:
        grad = gradient_image(oracle, vol, **kw)
    return normalize(interpolated(oracle, grad, points, index_start, **kw))


def one_step(oracle, vol, iso, v0, nrm, step, index_start=(0, 0, 0), **kw):
    """Where the walk's first pass takes the lattice start v0 along N(v0): float32(v0 + double(N) * (+-step)), the sign by
    the interpolated value against the iso value (txx:455-467)."""
    g = _geo(kw)
    img, keep = oracle._image(vol, g["spacing"], g["origin"], g["direction"], index_start)
    fn, ref = oracle.lib().cuberille_oracle_interpolate, C.byref(img)
    p = (C.c_double * 3)()
    out = np.empty((len(v0), 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        for n, v in enumerate(np.asarray(v0, dtype=np.float32)):
            p[0], p[1], p[2] = float(v[0]), float(v[1]), float(v[2])
            s = step if fn(ref, p) < iso else -step
            out[n] = [np.float32(float(v[k]) + float(nrm[n, k]) * s) for k in range(3)]
    return out


def same_normals(got, want, what=""):
    """Byte for byte, except that a NaN matches any NaN."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    bad = diff & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), "%s: %d normal components differ in their bits, first at %s: %r / %r" % (
        what, int(bad.sum()), np.argwhere(bad)[0], got[bad][0], want[bad][0])
