"""Independent witnesses for the walk, the normals, the B-spline and the recursive-Gaussian gradient.

Plain float64 numpy + scipy, written from ITK's documented definitions (the contract I1-I12 of SURVEY.md) and the control
flow of the reference's ProjectVertexToIsoSurface (txx:340-473).  This file loads NOTHING of the project: not the oracle,
not the restatements next to it, not the package (tests/test_independent.py reads the list below).  Where the project's
own checkers share a reading of ITK with the code they check, these do not: the index transform is a matrix and
np.linalg.inv, the interpolators are scipy.ndimage's (an implementation of the same published algorithms by other people),
the gradient is a difference of shifted arrays.

Arrays are numpy-ordered [z, y, x]; points, indices, spacings and start indices are (x, y, z).

What the witnesses do NOT reproduce is the reference's rounding: its vertices are float, its gradient image is float, its
sums have an order.  A witness therefore agrees to a tolerance (tests/golden/independent_tolerances.json, measured against
the reference), and only on vertices whose walk is not FRAGILE -- a walk that took a decision so close to its boundary that
the rounding decides it, judged here from the witness alone (fragility()).
"""
import math

import numpy as np
from scipy import ndimage

THRESHOLD, STEPS, SWAPS, SEARCH, DEAD = 0, 1, 2, 3, 4      # why a walk ended; DEAD: a normal that is not a number (quirk Q4)
REASONS = {THRESHOLD: "threshold", STEPS: "steps", SWAPS: "swaps", SEARCH: "search", DEAD: "dead"}

PROBE = 1.0e-6            # voxels: how far the fragility probes move a start point
PROBE_GAIN = 100.0        # a walk that ends more than this many times that far from its own unperturbed end is fragile
MARGIN = 1.0e-3           # a decision closer to its boundary than this share of the quantity's scale is fragile
GAUSSIAN_PROBE = 0.01     # the share by which a probe of the recursive-Gaussian walk scales one component of the gradient
ROUNDING_PROBES = 6       # walks with every position moved by up to twice the rounding of a float coordinate
FACE = 1.0                # voxels: a walk that came this close to a face of the buffer is fragile (clamping: no witness)


# ---- geometry --------------------------------------------------------------------------------------------------------

class Image:
    """A buffered region: voxels [z, y, x], spacing, origin, direction (3 x 3) and the ITK index of the first voxel."""

    def __init__(self, vox, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=None, start=(0, 0, 0)):
        self.vox = np.asarray(vox)
        self.f = self.vox.astype(np.float64)
        self.spacing = np.asarray(spacing, dtype=np.float64)
        self.origin = np.asarray(origin, dtype=np.float64)
        self.direction = np.eye(3) if direction is None else np.asarray(direction, dtype=np.float64).reshape(3, 3)
        self.start = np.asarray(start, dtype=np.float64)
        self.n = np.asarray(self.vox.shape[::-1], dtype=np.float64)
        self.i2p = self.direction @ np.diag(self.spacing)          # index -> physical: origin + D diag(spacing) index
        self.p2i = np.linalg.inv(self.i2p)

    def index_to_physical(self, index):
        return self.origin + np.asarray(index, dtype=np.float64) @ self.i2p.T

    def continuous_index(self, points):
        return (np.asarray(points, dtype=np.float64) - self.origin) @ self.p2i.T

    def buffer_position(self, points):
        """Where in the buffer (x, y, z; voxel centres at whole numbers from 0) the physical points lie."""
        return self.continuous_index(points) - self.start

    def voxels_between(self, a, b):
        """The distance of two sets of physical points in voxels: the largest index component of the difference."""
        return np.abs((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) @ self.p2i.T).max(axis=1)

    def face_distance(self, points):
        """Voxels from the nearest face of the buffer (the faces lie half a voxel outside the outermost centres)."""
        c = self.buffer_position(points)
        return np.minimum(c + 0.5, self.n - 0.5 - c).min(axis=1)

    def lattice_residual(self, points):
        """The start points of the walk are index_to_physical(whole index) - spacing / 2 (txx:266-270: the half spacing is taken
        off the PHYSICAL point, whatever the direction).  Returns how far, in voxels, each point is from such a point."""
        c = self.continuous_index(np.asarray(points, dtype=np.float64) + 0.5 * self.spacing)
        return np.abs(c - np.rint(c)).max(axis=1)


def _coords(img, points):
    return img.buffer_position(points)[:, ::-1].T          # map_coordinates wants (z, y, x) rows


# ---- value -----------------------------------------------------------------------------------------------------------

def linear_value(img):
    """LinearInterpolateImageFunction::Evaluate at physical points (I4, I5); outside the buffer the nearest pixel."""
    return lambda p: ndimage.map_coordinates(img.f, _coords(img, p), order=1, mode="nearest")


def bspline_coefficients(vox):
    """BSplineDecompositionImageFilter, order 3: the Unser / Thevenaz prefilter with whole-sample mirror boundaries."""
    return ndimage.spline_filter(np.asarray(vox).astype(np.float64), order=3, mode="mirror", output=np.float64)


def bspline_evaluate(coef, zyx):
    return ndimage.map_coordinates(coef, zyx, order=3, mode="mirror", prefilter=False)


def bspline_value(img):
    """BSplineInterpolateImageFunction::Evaluate, order 3, at physical points."""
    coef = bspline_coefficients(img.vox)
    return lambda p: bspline_evaluate(coef, _coords(img, p))


# ---- gradient --------------------------------------------------------------------------------------------------------

def central_gradient(img):
    """GradientImageFilter (I2, I6): central differences with replicated edge pixels over twice the spacing, taken to
    physical space by the direction matrix.  float64 [z, y, x, 3]."""
    g = np.empty(img.f.shape + (3,), dtype=np.float64)
    for k in range(3):
        ax = 2 - k
        pad = np.pad(img.f, [(1, 1) if a == ax else (0, 0) for a in range(3)], mode="edge")
        hi = np.take(pad, np.arange(2, pad.shape[ax]), axis=ax)
        lo = np.take(pad, np.arange(0, pad.shape[ax] - 2), axis=ax)
        g[..., k] = (hi - lo) / (2.0 * img.spacing[k])
    return g @ img.direction.T


def gaussian_gradient(img):
    """GradientRecursiveGaussianImageFilter, sigma = the largest spacing, NormalizeAcrossScale on (txx:488-491), as the
    filter it approximates: the sampled Gaussian derivative along the component's axis, the sampled Gaussian along the others,
    times sigma, per physical unit.  float64 [z, y, x, 3]."""
    sigma = float(img.spacing.max())
    g = np.empty(img.f.shape + (3,), dtype=np.float64)
    for k in range(3):
        d = img.f
        for j in range(3):
            d = ndimage.gaussian_filter1d(d, sigma / img.spacing[j], axis=2 - j, order=1 if j == k else 0, mode="nearest", truncate=8.0)
        g[..., k] = d * sigma / img.spacing[k]
    return g @ img.direction.T


def normal_function(img, grad):
    """VectorLinearInterpolateImageFunction::Evaluate of the gradient image + Normalize() (I7, I8): (unit vectors, the norms
    before normalising).  A zero gradient gives NaN (quirk Q4)."""
    def normal(p):
        zyx = _coords(img, p)
        g = np.stack([ndimage.map_coordinates(np.ascontiguousarray(grad[..., k]), zyx, order=1, mode="nearest") for k in range(3)], axis=1)
        norm = np.sqrt((g * g).sum(axis=1))
        with np.errstate(all="ignore"):
            return g / norm[:, None], norm
    return normal


# ---- the three walks -------------------------------------------------------------------------------------------------

class Walk:
    """What a walk leaves per vertex: points (the final positions), reason (THRESHOLD ...), margin (the least margin of any
    decision it took, as a share of the quantity's scale), gnorm (the least norm of a gradient before normalising), face (the
    least distance of any visited position from the buffer's faces, voxels), passes, path (a hash of every decision taken)."""

    def __init__(self, img, start):
        n = len(start)
        self.img = img
        self.points = np.array(start, dtype=np.float64)
        self.reason = np.full(n, -1, dtype=np.int64)
        self.margin = np.full(n, np.inf)
        self.gnorm = np.full(n, np.inf)
        self.face = img.face_distance(self.points) if n else np.zeros(0)
        self.passes = np.zeros(n, dtype=np.int64)
        self.path = np.zeros(n, dtype=np.uint64)

    def took(self, who, code):
        """Add what a pass decided (a small whole number per vertex) to the hash of the vertex's decisions."""
        self.path[who] = self.path[who] * np.uint64(1000003) + (np.asarray(code).astype(np.uint64) + np.uint64(1))

    def visited(self, who, points):
        ok = np.isfinite(points).all(axis=1)
        self.face[who[ok]] = np.minimum(self.face[who[ok]], self.img.face_distance(points[ok]))

    def decided(self, who, margin, scale):
        with np.errstate(all="ignore"):
            rel = np.where(scale > 0, margin / scale, np.inf)
        rel = np.where(np.isnan(rel), 0.0, rel)
        self.margin[who] = np.minimum(self.margin[who], rel)

    def gradient(self, who, norm):
        self.gnorm[who] = np.minimum(self.gnorm[who], np.where(np.isnan(norm), 0.0, norm))

    def count(self, reason, keep=None):
        m = self.reason == reason
        return int((m & keep).sum() if keep is not None else m.sum())


def _finite(p):
    return np.isfinite(p).all(axis=1)


def _still(p):
    """The witness keeps every position it computes as it is; a fragility probe passes a function that moves them a little."""
    return p


def walk_default(img, value, normal, start, iso, thr, step, relax, max_steps, jitter=_still):
    """txx:439-473."""
    w = Walk(img, start)
    active = np.ones(len(start), dtype=bool)
    number_of_steps = 0
    while active.any():
        a = np.flatnonzero(active)
        w.passes[a] += 1
        nrm, norm = normal(w.points[a])                                  # txx:451-452
        w.gradient(a, norm)
        v = value(w.points[a])                                           # txx:455
        d = np.abs(v - iso)
        w.decided(a, np.abs(d - thr), np.full(len(a), float(thr)))       # txx:456
        w.decided(a[d >= thr], d[d >= thr], np.full(int((d >= thr).sum()), float(thr)))   # txx:463, taken when not stopped
        stop = d < thr
        w.took(a, np.where(stop, 0, np.where(v < iso, 1, 2)))
        w.reason[a[stop]] = THRESHOLD
        active[a[stop]] = False
        go = a[~stop]
        sign = np.where(v[~stop] < iso, 1.0, -1.0)                       # txx:463
        w.points[go] = jitter(w.points[go] + nrm[~stop] * sign[:, None] * step)  # txx:464-467
        step *= relax                                                    # txx:468
        dead = ~_finite(w.points[go])
        w.reason[go[dead]] = DEAD
        active[go[dead]] = False
        go = go[~dead]
        w.visited(go, w.points[go])
        if number_of_steps > max_steps:                                  # txx:469: numberOfSteps++ > max
            w.reason[go] = STEPS
            active[go] = False
        number_of_steps += 1
    return w


def walk_advanced(img, value, normal, start, iso, thr, step, relax, max_steps, jitter=_still):
    """txx:340-397 (USE_ADVANCED_PROJECTION)."""
    w = Walk(img, start)
    n = len(start)
    active = np.ones(n, dtype=bool)
    previous = np.full(n, -1, dtype=np.int64)
    swaps = np.zeros(n, dtype=np.int64)
    number_of_steps = 0
    while active.any():
        a = np.flatnonzero(active)
        w.passes[a] += 1
        nrm, norm = normal(w.points[a])                                  # txx:356-357
        w.gradient(a, norm)
        t0 = jitter(w.points[a] + nrm * +1.0 * step)                     # txx:362-363
        t1 = jitter(w.points[a] + nrm * -1.0 * step)
        step *= relax                                                    # txx:365
        dead = ~(_finite(t0) & _finite(t1))
        w.points[a[dead]] = np.nan
        w.reason[a[dead]] = DEAD
        active[a[dead]] = False
        a, t0, t1 = a[~dead], t0[~dead], t1[~dead]
        w.visited(a, t0)
        w.visited(a, t1)
        d0 = np.abs(value(t0) - iso)                                     # txx:368-371
        d1 = np.abs(value(t1) - iso)
        i = np.where(d0 <= d1, 0, 1)                                     # txx:372
        w.decided(a, np.abs(d0 - d1), np.maximum(d0, d1))
        previous[a] = np.where(previous[a] < 0, i, previous[a])          # txx:373 (never updated again)
        swaps[a] += previous[a] != i                                     # txx:374
        w.points[a] = np.where((i == 0)[:, None], t0, t1)                # txx:375
        d = np.where(i == 0, d0, d1)
        w.decided(a, np.abs(d - thr), np.full(len(a), float(thr)))       # txx:378
        stop = d < thr
        w.took(a, 2 * i + stop)
        w.reason[a[stop]] = THRESHOLD
        active[a[stop]] = False
        a = a[~stop]
        if number_of_steps > max_steps:                                  # txx:385
            w.reason[a] = STEPS
            active[a] = False
            a = a[:0]
        number_of_steps += 1
        many = swaps[a] >= 5                                             # txx:392
        w.reason[a[many]] = SWAPS
        active[a[many]] = False
    return w


LINESEARCH_START = 10000.0          # txx:405: bestMetric


def walk_linesearch(img, value, normal, start, iso, thr, step, relax, max_steps, jitter=_still):
    """txx:398-437 (USE_LINESEARCH_PROJECTION).  Where no sample beats the start value the reference returns an unassigned
    vertex; such a vertex stays where it started and is DEAD (the project's documented choice)."""
    w = Walk(img, start)
    n = len(start)
    w.passes[:] = 1
    nrm, norm = normal(w.points)                                         # txx:408-409
    w.gradient(np.arange(n), norm)
    best = np.full(n, LINESEARCH_START)
    second = np.full(n, np.inf)
    best_point = w.points.copy()
    found = np.zeros(n, dtype=bool)
    which = np.zeros(n, dtype=np.int64)
    everyone = np.arange(n)
    sample = 0
    for sign in (-1.0, 1.0):                                             # txx:412
        for j in range(1, int(max_steps) // 2):                          # txx:415: unsigned division
            d = float(j) / (float(max_steps) / 2.0)                      # txx:418
            temp = jitter(w.points + nrm * sign * step * d)              # txx:421
            ok = _finite(temp)
            w.visited(everyone[ok], temp[ok])
            metric = np.full(n, np.nan)
            metric[ok] = np.abs(value(temp[ok]) - iso)                   # txx:424-425
            better = metric < best                                       # txx:430
            second = np.where(better, best, np.where(np.isnan(metric), second, np.minimum(second, metric)))
            best = np.where(better, metric, best)
            best_point[better] = temp[better]
            found |= better
            sample += 1
            which[better] = sample
    w.decided(everyone, second - best, second)
    w.took(everyone, which)
    w.points = best_point                                                # txx:437
    w.reason[:] = np.where(found, SEARCH, DEAD)
    return w


WALKS = {0: walk_default, 1: walk_advanced, 2: walk_linesearch}


# ---- cases -----------------------------------------------------------------------------------------------------------

def materialised(case):
    """(voxels, start index) of the image a case's walk runs in: the volume itself, or the padded / cropped / thresholded copy
    of its view -- what ConstantPadImageFilter, ExtractImageFilter (index kept) or BinaryThresholdImageFilter would hand on."""
    vox = case["vox"]
    start = tuple(case["geometry"].get("start", (0, 0, 0)))
    view = case.get("view")
    if not view:
        return vox, start
    if view["kind"] == "border":
        return np.pad(vox, 1, mode="constant", constant_values=vox.dtype.type(view["value"])), tuple(s - 1 for s in start)
    if view["kind"] == "region":
        (x, y, z), (nx, ny, nz) = view["start"], view["size"]
        return np.ascontiguousarray(vox[z:z + nz, y:y + ny, x:x + nx]), (start[0] + x, start[1] + y, start[2] + z)
    assert view["kind"] == "band"
    lower, upper, inside, outside = (vox.dtype.type(v) for v in view["band"])
    return np.where((lower <= vox) & (vox <= upper), inside, outside).astype(vox.dtype), start


def image_of(case):
    vox, start = materialised(case)
    g = case["geometry"]
    return Image(vox, g.get("spacing", (1.0, 1.0, 1.0)), g.get("origin", (0.0, 0.0, 0.0)), g.get("direction"), start)


class Witness:
    """The witness functions of one case: its image, value(points), normal(points) -> (unit vectors, norms), walk(start)."""

    def __init__(self, case):
        self.case = case
        self.img = image_of(case)
        self.value = bspline_value(self.img) if case["interp"].startswith("bspline") else linear_value(self.img)
        self.grad = gaussian_gradient(self.img) if case["gradient"] else central_gradient(self.img)
        self.normal = normal_function(self.img, self.grad)

    def walk(self, start, normal=None, jitter=_still):
        c = self.case
        return WALKS[c["variant"]](self.img, self.value, normal or self.normal, np.asarray(start, dtype=np.float64), float(c["iso"]),
                                   float(c["threshold"]), float(c["step"]), float(c["relax"]), int(c["max_steps"]), jitter)

    def fragility(self, start, walk=None):
        """bool per vertex, from the witness alone: the walk repeated from start points moved by +-PROBE voxels along each axis
        ends more than PROBE_GAIN times that far from its own unperturbed end (or for another reason); or, every position moved
        by what the reference's float vertices round away (rounding), takes another decision anywhere; or a decision's margin
        is below MARGIN of the quantity's scale; or a visited position came within FACE voxels of a face of the buffer -- there
        the clamping of the neighbours is the project's own choice and no witness exists; or the walk
        met a gradient that is zero (quirk Q4: the reference's vertex is NaN from there on, or undefined in the line search) or
        below MARGIN of the largest in the image: the direction of a vanishing vector is decided by its rounding."""
        start = np.asarray(start, dtype=np.float64)
        w = self.walk(start) if walk is None else walk
        scale = np.sqrt((self.grad * self.grad).sum(axis=-1)).max()
        # (the recursion's error is a share of the LARGEST gradient: a gradient of a tenth of that is off by ten times the share)
        low = (10.0 * GAUSSIAN_PROBE if self.case["gradient"] else MARGIN) * scale
        fragile = (w.margin < MARGIN) | (w.face < FACE) | (w.reason == DEAD) | ~(w.gnorm > low) | ~_finite(w.points)
        for k in range(3):
            for s in (-1.0, 1.0):
                moved = self.walk(start + s * PROBE * self.img.i2p[:, k])
                with np.errstate(invalid="ignore"):
                    far = self.img.voxels_between(moved.points, w.points)
                fragile |= ~(far <= PROBE_GAIN * PROBE) | (moved.reason != w.reason)
                if self.case["gradient"]:
                    # The recursion only approximates the Gaussian derivative this witness computes, to about half a percent of
                    # the largest gradient (Deriche's fourth-order fit; measured in tests/test_independent.py): a walk whose
                    # decisions change when one component of the gradient image is a percent larger or smaller is decided
                    # by that approximation.
                    scaled = self.grad.copy()
                    scaled[..., k] *= 1.0 + s * GAUSSIAN_PROBE
                    moved = self.walk(start, normal_function(self.img, scaled))
                    fragile |= (moved.path != w.path) | (moved.reason != w.reason)
        for seed in range(ROUNDING_PROBES):
            moved = self.walk(start, jitter=self.rounding(start, seed))
            with np.errstate(invalid="ignore"):
                far = self.img.voxels_between(moved.points, w.points)
            # (a vertex that twice the reference's rounding moves by half of the 1e-3 voxel to which the witnesses are held at
            #  the most cannot be held to that)
            fragile |= (moved.path != w.path) | (moved.reason != w.reason) | ~(far <= 0.5e-3)
        return fragile

    def rounding(self, start, seed):
        """The reference keeps its vertex in float (I9, I11): every position a pass computes is rounded, each coordinate by up
        to half a unit in its last place -- 2^-24 of the coordinate.  Where a kink of the field bends the walks apart, a pass
        hands that on enlarged, which probes of the START do not see: the first passes, down to the surface, draw them
        together again.  So these probes move every position the witness computes, by a random amount of up to twice the
        reference's rounding at the largest coordinate (seeded: the same probes every time).  A walk whose decisions -- a stop,
        a sign, a side, the best sample -- or whose end then change says nothing about a walk in float."""
        rng = np.random.default_rng(740 + seed)
        reach = max(float(np.abs(np.asarray(start, dtype=np.float64)).max()) if len(start) else 1.0, 1.0)
        return lambda p: p + rng.uniform(-1.0, 1.0, p.shape) * (2.0 ** -23 * reach)


def angle_between(a, b):
    """The angle in radians between the rows of a and b (unit vectors or not); NaN where either is NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        cross = np.linalg.norm(np.cross(a, b), axis=1)
        return np.arctan2(cross, (a * b).sum(axis=1))


def _rot(deg_x, deg_y, deg_z, order):
    cx, sx, cy, sy, cz, sz = (f(math.radians(d)) for d in (deg_x, deg_y, deg_z) for f in (math.cos, math.sin))
    m = {"x": np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]]),
         "y": np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]]),
         "z": np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])}
    return m[order[0]] @ m[order[1]] @ m[order[2]]


ANISO = dict(spacing=(0.7, 1.3, 2.1), origin=(10.0, -20.0, 5.0))
GEOMETRIES = {
    "identity": dict(),
    "aniso": dict(ANISO),
    "rot_a": dict(ANISO, direction=_rot(40.0, -15.0, 25.0, "zyx")),
    "rot_b": dict(ANISO, direction=_rot(70.0, 10.0, -50.0, "xzy")),
    "shear": dict(spacing=(1.1, 0.8, 1.25), origin=(-3.0, 2.0, 0.5), direction=np.array([[1.0, 0.15, 0.0], [0.0, 1.0, 0.1], [0.05, 0.0, 1.0]])),
    "start": dict(spacing=(1.0, 2.0, 0.5), origin=(0.25, 0.0, -1.0), start=(5, -3, 12)),
}

BALL_ISO = 100


def ball(dtype, shape=(16, 20, 24), radius=5.0):
    """[z, y, x]: BALL_ISO + 20 (R - r) around a centre slightly off the volume's: !(pixel < iso) is the ball of radius R."""
    nz, ny, nx = shape
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    r = np.sqrt((x - (nx - 1) / 2 - 0.21) ** 2 + (y - (ny - 1) / 2 + 0.13) ** 2 + (z - (nz - 1) / 2 - 0.07) ** 2)
    f = BALL_ISO + 20.0 * (radius - r)
    dtype = np.dtype(dtype)
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        return np.clip(np.rint(f), info.min, info.max).astype(dtype)
    return f.astype(dtype)


def blob(shape=(20, 22, 26), seed=740):
    """[z, y, x] float32: Gaussian-filtered noise scaled to +-100, with a 3-voxel rim of -100 so that no surface meets the
    border (iso 0)."""
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.standard_normal(shape), 2.0, mode="nearest")
    f = f * (100.0 / np.abs(f).max())
    rim = np.ones(shape, dtype=bool)
    rim[3:-3, 3:-3, 3:-3] = False
    f[rim] = -100.0
    return f.astype(np.float32)


def box_at_the_face(shape=(16, 20, 12)):
    """[z, y, x] float32: BALL_ISO + 20 d, d the least of the distances to the six sides of a box that keeps 2.6 voxels from
    every face but the low x one, where its gently waved side lies 0.65 .. 0.85 voxels inside the first voxel centre."""
    nz, ny, nx = shape
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    d = np.minimum.reduce([x - 0.75 - 0.1 * np.sin(0.5 * y) * np.cos(0.4 * z), (nx - 5.7) - x, y - 2.6, (ny - 3.6) - y, z - 2.6, (nz - 3.6) - z])
    return (BALL_ISO + 20.0 * d).astype(np.float32)


def two_sheets(dtype=np.uint8):
    """[z, y, x]: two one-voxel sheets of 200 with one empty plane between them.  On the faces that look at each other, away
    from the sheets' edges, every gradient the lattice point averages is exactly zero: the normal there is NaN (quirk Q4)."""
    vox = np.zeros((9, 12, 12), dtype=dtype)
    vox[3, 2:10, 2:10] = 200
    vox[5, 2:10, 2:10] = 200
    return vox


def _step(geometry):
    return 0.25 * max(geometry.get("spacing", (1.0, 1.0, 1.0)))        # the reference's default, written out


def _case(name, vox, geo, iso, threshold, reach, variant=0, interp="linear", gradient=0, view=None, step=None, relax=0.95, max_steps=50):
    g = GEOMETRIES[geo]
    return dict(name=name, vox=vox, geometry=g, geometry_name=geo, iso=iso, threshold=threshold, step=_step(g) if step is None else step,
                relax=relax, max_steps=max_steps, variant=variant, interp=interp, gradient=gradient, view=view, reach=list(reach))


_CASES = None


def independent_cases():
    """The cases of tests/test_independent.py, tests/test_gpu_independent.py and tests/golden/make_independent_tolerances.py:
    dicts of name, vox, geometry, iso, threshold, step, relax, max_steps, variant, interp ("linear", "bspline32", "bspline64"),
    gradient (0 central, 1 recursive Gaussian), view (None or the border / region / band setting) and reach: the stop reasons
    the case is meant to reach with at least eight vertices that are not fragile.  Every volume has max |voxel - iso| < 10000
    (the line search's start value)."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    balls = {dt: ball(dt) for dt in ("uint8", "int16", "float32", "float64")}
    bl = blob()
    # the ball, linear, central: every geometry in float32, every pixel type on two geometries
    for geo in GEOMETRIES:
        out.append(_case("ball/float32/%s" % geo, balls["float32"], geo, BALL_ISO, 0.5, [THRESHOLD]))
    for dt in ("uint8", "int16", "float64"):
        for geo in ("identity", "rot_a"):
            # (whole-number pixels: a lattice start averages eight of them and sits on a multiple of 1/8; 0.45 is none)
            out.append(_case("ball/%s/%s" % (dt, geo), balls[dt], geo, BALL_ISO, 0.45 if dt != "float64" else 0.5, [THRESHOLD]))
    # the blob at both thresholds; few steps: walks that end by the step count
    # (threshold 0.01 is five ten-thousandths of a voxel on this field.  With the default fifty passes and relaxation 0.95 the
    #  steps shrink to a fiftieth of a voxel and every pass is one more stop-or-go decision that close to its boundary: a
    #  quarter of the vertices come out fragile.  Eight passes that shrink by 0.85 end with steps of a twentieth of a voxel and
    #  keep nine in ten; both ways of ending are reached.)
    tight = dict(relax=0.85, max_steps=8)
    for geo in ("identity", "aniso", "rot_b", "shear", "start"):
        out.append(_case("blob/%s/thr0.5" % geo, bl, geo, 0.0, 0.5, [THRESHOLD]))
        out.append(_case("blob/%s/thr0.01" % geo, bl, geo, 0.0, 0.01, [THRESHOLD, STEPS], **tight))
    out.append(_case("blob/identity/steps", bl, "identity", 0.0, 0.01, [THRESHOLD, STEPS], max_steps=3))
    out.append(_case("blob/rot_a/steps", bl, "rot_a", 0.0, 0.01, [THRESHOLD, STEPS], max_steps=2))
    # the two compiled-out branches
    for geo, vox, name, iso, thr in [("rot_a", balls["float32"], "ball", BALL_ISO, 0.5), ("identity", bl, "blob", 0.0, 0.5),
                                     ("aniso", bl, "blob", 0.0, 0.01)]:
        out.append(_case("advanced/%s/%s/thr%g" % (name, geo, thr), vox, geo, iso, thr, [THRESHOLD, SWAPS], variant=1))
        # (a line of twice the default step to either side, in 24 samples)
        out.append(_case("linesearch/%s/%s" % (name, geo), vox, geo, iso, thr, [SEARCH], variant=2, step=2.0 * _step(GEOMETRIES[geo])))
    out.append(_case("advanced/blob/identity/steps", bl, "identity", 0.0, 0.001, [STEPS], variant=1, max_steps=3))
    # the B-spline interpolator, both coefficient types
    for bits in (32, 64):
        out.append(_case("bspline%d/ball/float32/identity" % bits, balls["float32"], "identity", BALL_ISO, 0.5, [THRESHOLD], interp="bspline%d" % bits))
        out.append(_case("bspline%d/ball/int16/start" % bits, balls["int16"], "start", BALL_ISO, 0.45, [THRESHOLD], interp="bspline%d" % bits))
        out.append(_case("bspline%d/blob/rot_a/thr0.01" % bits, bl, "rot_a", 0.0, 0.01, [THRESHOLD, STEPS], interp="bspline%d" % bits, **tight))
        # A box whose low x side lies three quarters of a voxel inside the first voxel centre: the walks of that side start at
        # position 0.5 and end between the first two centres -- a voxel and more from the face, no neighbour clamped -- while the
        # spline's first tap lies at -1, outside the buffer: the only case that reads the mirror boundary of the evaluation.
        # The threshold of 0.01: a walk's steps are whole, so a value that is a little off shows only in the decisions it
        # changes, and these walks take ten each.
        out.append(dict(_case("bspline%d/box_at_the_face" % bits, box_at_the_face(), "identity", BALL_ISO, 0.01, [THRESHOLD, STEPS],
                              interp="bspline%d" % bits, **tight), near_face=64))
    # the recursive-Gaussian gradient (identity direction: all the project's own restatement covers)
    out.append(_case("gaussian/ball/float32/identity", balls["float32"], "identity", BALL_ISO, 0.5, [THRESHOLD], gradient=1))
    # (not the blob: smoothed over the rim its gradient all but vanishes at a few dozen vertices, where half a percent of the
    #  largest gradient turns the normal by tens of degrees -- the approximation, not a primitive, would decide those)
    out.append(_case("gaussian/ball/float32/aniso", balls["float32"], "aniso", BALL_ISO, 0.5, [THRESHOLD], gradient=1))
    # the three source views, each on the materialised copy
    out.append(_case("view/border", balls["float32"], "aniso", BALL_ISO, 0.5, [THRESHOLD], view=dict(kind="border", value=3)))
    buf = np.random.default_rng(5).integers(0, 255, (16 + 3, 20 + 5, 24 + 7)).astype(np.float32)
    buf[1:17, 2:22, 3:27] = balls["float32"]
    out.append(_case("view/region", buf, "start", BALL_ISO, 0.5, [THRESHOLD], view=dict(kind="region", start=(3, 2, 1), size=(24, 20, 16))))
    # the band's copy holds 0 and 1 only: a lattice start sits on a multiple of 1/8 (1 - 0.5 is one), so 0.45
    out.append(_case("view/band", balls["uint8"], "identity", 1, 0.45, [THRESHOLD],
                     view=dict(kind="band", band=(BALL_ISO, int(balls["uint8"].max()), 1, 0))))
    _CASES = out
    return out


def case_conditions(walk, fragile, case):
    """The conditions a case must meet before it is relied on, from the witness alone: None, or what is wrong."""
    n = len(fragile)
    kept = ~fragile
    if fragile.sum() > 0.10 * n:
        return "%s: %d of %d vertices are fragile (more than 10 %%)" % (case["name"], fragile.sum(), n)
    if kept.sum() < 64:
        return "%s: %d vertices remain (less than a wave)" % (case["name"], kept.sum())
    for r in case["reach"]:
        if walk.count(r, kept) < 8:
            return "%s: only %d vertices that are not fragile end by %s" % (case["name"], walk.count(r, kept), REASONS[r])
    if case.get("near_face"):
        # vertices that stayed a voxel from every face and END within a voxel and a half of one: a spline tap outside the buffer
        with np.errstate(invalid="ignore"):
            near = int((kept & (walk.img.face_distance(walk.points) < 1.5)).sum())
        if near < case["near_face"]:
            return "%s: only %d vertices that are not fragile walk between the first two voxel centres" % (case["name"], near)
    return None
