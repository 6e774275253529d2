"""Every form of the walk at the edges of the number range: the envelope cases of tests/ref_filter.py (voxels from subnormal
to infinite, integer noise over a type's whole range, spacings of 1e-60 .. 1e60, origins up to 1e30, start indices at +-2^30,
steps of 1e-300 .. 1e5, a direction matrix near singular) through each launch shape and source view the library has, against
the REFERENCE filter's result for the same case, bit for bit (NaN compared as NaN; no tolerance anywhere):

  the general geometry form forced (proj_ident 0), the literal gradient (proj_literal 1), the launch shapes of short and of
  long walks (proj_short 1 / 0); a resident volume, count + emit; two slabs, two thin-halo slabs with
  cuberille_reproject_escaped (the default branch: the library offers a thin halo with no other); the box of a larger pitched
  buffer (cuberille_set_region, the default branch again: the header offers a region with no other); cuberille_set_border against the pad-then-filter twin; cuberille_set_band against the twin on
  the {0, 1} copy; the point normals.

tests/test_gpu_reference_filter.py runs the same cases through extract_host with default tuning, which is one launch shape and
whatever geometry form the case takes.  The routes are fuzz_campaign.run_case's (the campaign's own driver), handed a recipe
made from the case.  The reference is the binary where oracle/_ref/ travelled, tests/golden/reference_filter_digests.json
(written from the binary alone) otherwise; reads nothing else."""
import json

import numpy as np
import pytest

import fuzz_campaign as fc
import normals_ref
import ref_filter as rf

pytestmark = pytest.mark.gpu

FAMILIES = ["magnitude/float32", "magnitude/float64", "span", "spacing", "origin", "start", "step", "shear", "relax_0"]
SWITCHES = [("proj_ident", 0), ("proj_literal", 1), ("proj_short", 0), ("proj_short", 1)]
REGION_LOW, REGION_HIGH = (3, 2, 1), (5, 1, 2)          # voxels of the buffer before / behind the box, (x, y, z)
REGION_REFUSAL = "the region's start index (the buffer's + the box's) must lie within +-2^30"
BORDER_REFUSAL = "the bordered region's start index must lie within +-2^30"
needs_binary = pytest.mark.skipif(not rf.available(0), reason="oracle/_ref/ref_filter is not built (no reference tree at build time)")

_reference = {}
_rows = {}


def cases_of(family):
    """The projected cases of one family (the pad and band twins run in tests of their own)."""
    out = [c for c in rf.envelope_magnitude_cases() + rf.envelope_span_cases() + rf.envelope_geometry_cases()
           if c["name"].startswith("envelope/" + family) and c["project"]]
    assert out, family
    return out


def test_the_families_are_the_whole_envelope():
    names = [c["name"] for f in FAMILIES for c in cases_of(f)]
    assert sorted(names) == sorted(c["name"] for c in rf.envelope_cases() if c["project"] and not c["pad"] and "band" not in c["volume"])


def row_of(case):
    if not _rows:
        with open(rf.DIGESTS) as f:
            _rows.update({r["case"]["name"]: r for r in json.load(f)})
    row = _rows[case["name"]]
    assert row["case"] == case, case["name"]
    return row


def hold(case, points, cells, what):
    """The mesh of `case` through the form `what` against the reference filter's: the binary's where it travelled, its recorded
    digest otherwise."""
    what = "%s through %s" % (case["name"], what)
    assert rf.points_defined(case)
    if rf.available(case["variant"]):
        if case["name"] not in _reference:
            _reference[case["name"]] = rf.run_reference(case) + (rf.undefined_vertices(case),)
        rpoints, rcells, mask = _reference[case["name"]]
        diff = rf.difference_outside(mask, points, cells, rpoints, rcells)
        assert diff is None, "%s: %s" % (what, diff)
        return
    row = row_of(case)
    assert (len(points), len(cells)) == (row["points"], row["cells"]), what
    mask = np.zeros(len(points), dtype=bool)
    mask[row["undefined_vertices"]] = True
    d = rf.digest(*rf.masked(mask, points, cells))
    assert d["cells_sha256"] == row["cells_sha256"] and d["points_sha256"] == row["points_sha256"], what


def recipe_of(case, vox, geo, route, kind="whole", **more):
    """The campaign's recipe (fuzz_campaign.run_case) of an envelope case: the filter object's clamps applied (ref_filter.effective)."""
    thr, step, relax = rf.effective(case, vox)
    kw = dict(triangles=bool(case["triangles"]), project=bool(case["project"]), threshold=thr, step=step, relax=relax,
              max_steps=case["max_steps"], variant=case["variant"])
    iso = rf.iso_of(case)
    recipe = dict(seed=0, case=0, kind=kind, dtype=vox.dtype.name, route=route, kw=kw, spacing=list(geo["spacing"]), origin=list(geo["origin"]),
                  direction=np.asarray(geo["direction"], dtype=np.float64).reshape(3, 3).tolist(), index_start=[int(v) for v in geo["start"]],
                  iso=iso if vox.dtype.kind == "f" else int(iso), normals=False, repeat=1)
    recipe.update(more)
    return recipe


@pytest.fixture(scope="module")
def contexts(pkg):
    pkg._abi.build()
    ctx = {"ex": pkg.Extractor(0)}
    yield ctx
    ctx["ex"].close()


def run(pkg, contexts, recipe, vox):
    got = fc.run_case(pkg, contexts, recipe, vox=vox)
    return got["mesh"].points, got["mesh"].cells, got


@pytest.mark.parametrize("family", FAMILIES)
def test_launch_shapes_and_resident_routes(pkg, contexts, family):
    """The general geometry form forced where the case would take the identity or the diagonal one, the literal gradient, the
    launch shapes of short and of long walks; a resident volume; count + emit."""
    for case in cases_of(family):
        vox, geo, _ = rf.case_inputs(case)
        for name, value in SWITCHES:
            points, cells, _ = run(pkg, contexts, recipe_of(case, vox, geo, "switch", switch=[name, value]), vox)
            hold(case, points, cells, "%s %d" % (name, value))
        for route in ("device", "count_emit"):
            points, cells, _ = run(pkg, contexts, recipe_of(case, vox, geo, route), vox)
            hold(case, points, cells, route)


@pytest.mark.parametrize("family", FAMILIES)
def test_two_slabs_and_two_thin_halo_slabs(pkg, contexts, family):
    """Two slabs with the full halo on every branch; two thin-halo slabs on the default branch, the walks that leave the thin
    halo walked again by cuberille_reproject_escaped -- a step of 50 or 1e5 takes all of them out.  The stitched mesh is the
    reference's."""
    escaped = 0
    for case in cases_of(family):
        vox, geo, _ = rf.case_inputs(case)
        cuts = [0, vox.shape[0] // 2, vox.shape[0]]
        for route in ("slabs", "thin_slabs") if case["variant"] == 0 else ("slabs",):
            stats = {}
            got = fc.run_case(pkg, contexts, recipe_of(case, vox, geo, route, cuts=cuts), vox=vox, stats=stats)
            escaped += stats.get("escaped_walks", 0)
            hold(case, got["mesh"].points, got["mesh"].cells, route)
    if family == "step":
        assert escaped > 0                  # the documented path ran: reproject_escaped, not a refusal


def region_buffer(vox, low):
    """A buffer with the volume as its box at `low` (x, y, z): around it what would show in the mesh if it were read -- NaN for
    the float types, noise over the whole range for the others."""
    nz, ny, nx = vox.shape
    shape = (nz + low[2] + REGION_HIGH[2], ny + low[1] + REGION_HIGH[1], nx + low[0] + REGION_HIGH[0])
    if vox.dtype.kind == "f":
        buf = np.full(shape, np.nan, dtype=vox.dtype)
    else:
        info = np.iinfo(vox.dtype)
        buf = np.random.default_rng(5).integers(info.min, info.max, size=shape, dtype=vox.dtype, endpoint=True)
    buf[low[2]:low[2] + nz, low[1]:low[1] + ny, low[0]:low[0] + nx] = vox
    return buf


@pytest.mark.parametrize("family", FAMILIES)
def test_as_the_box_of_a_larger_buffer(pkg, contexts, family):
    """cuberille_set_region on a pitched buffer: the buffer's start index is the case's less the box's position, so the box is
    the case's image, start index and all (an axis whose start index is -2^30 keeps the box at the buffer's edge: the buffer
    cannot start lower).  And where the case's start index is +2^30 the buffer may not start THERE with the box further in: the
    sum leaves the legal range, refused in cuberille_region_desc's words."""
    limit = rf.ENV_LIMIT
    for case in cases_of(family):
        if case["variant"] != 0:            # (the header offers a region with the default projection branch only)
            continue
        vox, geo, _ = rf.case_inputs(case)
        nz, ny, nx = vox.shape
        low = tuple(0 if s - l < -limit else l for s, l in zip(geo["start"], REGION_LOW))
        buf = region_buffer(vox, low)
        bgeo = dict(geo, start=[s - l for s, l in zip(geo["start"], low)])
        region = dict(form="envelope", start=list(low), size=[nx, ny, nz])
        for route in ("host", "device", "count_emit"):
            points, cells, _ = run(pkg, contexts, recipe_of(case, buf, bgeo, route, kind="region", region=region), buf)
            hold(case, points, cells, "region/" + route)
        if max(geo["start"]) == limit:
            buf = region_buffer(vox, REGION_LOW)
            with pytest.raises(pkg._abi.CuberilleError) as refused:
                run(pkg, contexts, recipe_of(case, buf, geo, "host", kind="region", region=dict(region, start=list(REGION_LOW))), buf)
            assert refused.value.code == pkg._abi.ERR_LIMIT and REGION_REFUSAL in str(refused.value), case["name"]


def test_the_border_against_the_padded_twins(pkg, contexts):
    """cuberille_set_border(1, 0) on the volume itself against ConstantPadImageFilter-then-filter through the reference: the
    recorded twins, one case per family -- what holds the border where the binaries did not travel (every case:
    test_the_border_on_every_case)."""
    cases = rf.envelope_pad_cases()
    assert len(cases) == 9 and all(c["pad"] for c in cases)
    for case in cases:
        vox, geo, _ = rf.case_inputs(case)
        for route in ("host", "device", "count_emit"):
            points, cells, _ = run(pkg, contexts, recipe_of(case, vox, geo, route, kind="border", border=dict(value=0)), vox)
            hold(case, points, cells, "border/" + route)


@needs_binary
@pytest.mark.parametrize("family", FAMILIES)
def test_the_border_on_every_case(pkg, contexts, family):
    """cuberille_set_border(1, 0) on EVERY default-branch case (the header offers a border with no other branch) against the
    same case with pad = 1 through the reference binary -- the ring walked in the identity, the diagonal and the general form
    at every magnitude, span, spacing, origin, start and step.  Where the binaries did not travel the nine recorded twins
    above stand in.  A start index of -2^30 on any axis: the ring would start one index lower, outside the legal range, and
    the call is refused in the header's words."""
    ran = refused = 0
    for case in cases_of(family):
        if case["variant"] != 0:
            continue
        vox, geo, _ = rf.case_inputs(case)
        twin = dict(case, name=case["name"].replace("envelope/", "envelope/pad/", 1), pad=1)
        for route in ("host", "device", "count_emit"):
            recipe = recipe_of(twin, vox, geo, route, kind="border", border=dict(value=0))
            if min(geo["start"]) == -rf.ENV_LIMIT:
                with pytest.raises(pkg._abi.CuberilleError) as no:
                    run(pkg, contexts, recipe, vox)
                assert no.value.code == pkg._abi.ERR_LIMIT and BORDER_REFUSAL in str(no.value), (case["name"], route)
                refused += 1
                continue
            points, cells, _ = run(pkg, contexts, recipe, vox)
            rpoints, rcells = rf.run_reference(twin)
            diff = rf.first_difference(points, cells, rpoints, rcells)
            assert diff is None, "%s through border/%s: %s" % (twin["name"], route, diff)
            ran += 1
    assert ran and (refused > 0) == (family == "start")


def test_the_band_against_the_thresholded_twins(pkg, contexts):
    """cuberille_set_band on the field itself against the reference on the {0, 1} copy (ref_filter.envelope_band_cases)."""
    cases = rf.envelope_band_cases()
    assert len(cases) == 11
    for case in cases:
        spec = dict(case["volume"])
        lower, upper, inside, outside = spec.pop("band")
        vox, geo, _ = rf.case_inputs(dict(case, volume=spec))           # the field as the caller holds it
        mapped, _, _ = rf.case_inputs(case)
        assert set(np.unique(mapped)) == {0, 1} and not np.array_equal(vox, mapped)
        band = dict(lower=lower, upper=upper, inside=inside, outside=outside)
        for route in ("host", "device", "count_emit"):
            points, cells, _ = run(pkg, contexts, recipe_of(case, vox, geo, route, kind="band", band=band), vox)
            hold(case, points, cells, "band/" + route)


@pytest.mark.parametrize("family", FAMILIES)
def test_point_normals(pkg, oracle, contexts, family):
    """cuberille_set_point_normals on the default branch: N(p) at every final vertex against tests/normals_ref.py -- built
    from the oracle's two pinned primitives -- at the REFERENCE's vertices, bit for bit (same_normals: a NaN matches a NaN)."""
    for case in cases_of(family):
        if case["variant"] != 0:
            continue
        vox, geo, _ = rf.case_inputs(case)
        points, cells, got = run(pkg, contexts, recipe_of(case, vox, geo, "host", normals=True, drop_normals_row=True), vox)
        hold(case, points, cells, "host with point normals")
        # (held to the reference just above: the library's vertices ARE the reference's, NaN for NaN)
        want = normals_ref.normals(oracle, vox, points, tuple(geo["start"]), spacing=tuple(geo["spacing"]), origin=tuple(geo["origin"]),
                                   direction=np.asarray(geo["direction"], dtype=np.float64).reshape(3, 3))
        share = float(np.isnan(want).any(axis=1).mean())
        normals_ref.same_normals(got["normals"], want, "%s (%.0f %% of the reference normals are NaN)" % (case["name"], 100 * share))


@pytest.mark.parametrize("family", ["magnitude/float32", "magnitude/float64", "spacing", "origin"])
def test_recursive_gaussian_gradient(pkg, oracle, contexts, family):
    """gradient = 1, the recursive-Gaussian gradient the reference compiles out (k_rg_pass: float lines, double recursion;
    the walk along a double gradient image), on the whole volume, every branch: against oracle.run(gradient=1) -- the
    reference binary has no such gradient.  The oracle's filter is a restatement: tests/test_oracle.py holds it to a second one
    on those of these cases that have an identity direction and walk the default branch."""
    restated = {c["name"] for c in rf.recursive_gaussian_restated_cases()}
    cases = cases_of(family)
    assert restated & {c["name"] for c in cases}
    for case in cases:
        vox, geo, _ = rf.case_inputs(case)
        assert min(vox.shape) >= 4
        want = rf.run_oracle(oracle, case, gradient=1)
        for route in ("host", "device"):
            recipe = recipe_of(case, vox, geo, route)
            recipe["kw"]["gradient"] = 1
            points, cells, _ = run(pkg, contexts, recipe, vox)
            diff = rf.first_difference(points, cells, *want)
            assert diff is None, "%s through %s with the recursive-Gaussian gradient: %s" % (case["name"], route, diff)
