"""-m "not gpu": the hand-run campaign and profile scripts stay importable, and the campaign's generators stay inside what the
oracle accepts (every drawn volume, geometry, start index and held first volume runs through it) -- so that the scripts do not rot
between the rounds in which somebody runs them on a GPU box.  The campaign's new dimensions too: every drawn border value, box
and band passes its validator, every drawn recipe survives JSON, rebuilds the same bytes and runs through expected(); and the
seeded slice of tests/test_gpu_campaign.py holds the conditions that keep it from hiding a failure, shown on the oracle alone.
Cell pixels, components, their rows and the id offset come from a stream of their own: what the campaign drew before them is
held, draw for draw, to a fixture recorded on the commit before (tests/golden/campaign_recipe_digests.json)."""
import glob
import json
import os
import py_compile

import numpy as np

from conftest import ROOT


def test_scripts_compile():
    files = glob.glob(os.path.join(ROOT, "profiles", "*.py")) + glob.glob(os.path.join(ROOT, "tests", "*.py")) + \
        glob.glob(os.path.join(ROOT, "midas-journal-740_amd", "*.py")) + [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    assert len(files) > 30
    for f in files:
        py_compile.compile(f, doraise=True)


def test_campaign_generators_run_through_the_oracle(oracle):
    import fuzz_campaign as fz
    rng = np.random.default_rng(11)
    kinds = set()
    for case in range(40):
        nx = int(rng.choice(fz.XS[:10]))
        ny, nz = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        dt = fz.DTYPES[case % len(fz.DTYPES)]
        vox, iso = fz.draw_field(rng, (nz, ny, nx), dt)
        assert vox.shape == (nz, ny, nx) and vox.dtype == np.dtype(dt) and vox.flags["C_CONTIGUOUS"]
        spacing, origin, direction = fz.draw_geometry(rng)
        assert abs(abs(np.linalg.det(direction)) - 1.0) < 1e-9
        start = tuple(int(v) for v in rng.integers(-3000, 3000, size=3))
        kw = dict(triangles=bool(case & 1), project=True, threshold=0.01, step=0.25 * min(spacing), relax=0.9, max_steps=6)
        mesh = oracle.run(vox, iso, spacing=spacing, origin=origin, direction=direction, index_start=start, **kw)
        assert mesh.cells.shape[1] == (3 if case & 1 else 4)
        if case % 5 == 0 and mesh.points.shape[0]:
            fvox, _ = fz.draw_field(rng, (5, 6, 7), dt)
            fs, fo, fd = fz.draw_geometry(rng)
            held = oracle.run(vox, iso, spacing=spacing, origin=origin, direction=direction, index_start=start,
                              first=(fvox, fs, fo, fd, (3, -2, 1)), **kw)
            assert held.points.shape == mesh.points.shape and np.array_equal(held.cells.shape, mesh.cells.shape)
        kinds.add(np.dtype(dt).kind)
    assert kinds == {"u", "i", "f"}
    # the device copy helper keeps the bytes of the unsigned types torch cannot hold as such
    class _T:
        @staticmethod
        def from_numpy(a):
            class _R:
                def __init__(self, arr): self.arr = arr
                def cuda(self): return self.arr
            return _R(a)
    for dt in (np.uint16, np.uint32, np.uint64, np.uint8, np.float32):
        a = (np.arange(24).reshape(2, 3, 4) * 1000).astype(dt)
        b = fz.to_device(_T, a)
        assert b.tobytes() == a.tobytes() and b.dtype.itemsize == a.dtype.itemsize


def _recipes(n, **options):
    import fuzz_campaign as fz
    return [fz.draw_case(23, case, dict(max_rows=10, max_voxels=20000, **options)) for case in range(n)]


def test_drawn_views_pass_their_validators(pkg):
    """No GPU: the ring's value by border_check's rule (check_border for the 64-bit integer types, the range of the type for the
    others -- `converts` takes any double for the floating types, a NaN or infinite ring included), the box by
    cuberille_region_desc, the band by cuberille_band_check."""
    import fuzz_campaign as fz
    seen = {"nonfinite_ring": 0, "single_label": 0, "constant_band": 0, "inf_bound": 0, "zero_bound": 0, "forms": set(), "residues": set()}
    for kind in ("border", "region", "band"):
        for r in _recipes(300, kind=kind):
            dt = np.dtype(r["dtype"])
            code = int(pkg.make_desc(dt, (1, 1, 1)).pixel_type)
            nz, ny, nx = r["field"]["shape"]
            desc = pkg.make_desc(dt, (nx, ny, nz), r["spacing"], r["origin"], np.asarray(r["direction"]), r["index_start"])
            if kind == "border":
                c = fz._num(r["border"]["value"])
                if dt.kind == "f":
                    seen["nonfinite_ring"] += int(not np.isfinite(c))
                else:
                    info = np.iinfo(dt)
                    assert isinstance(c, int) and int(info.min) <= c <= int(info.max), r
                    pkg.cuberille.check_border(code, (1, c))
            elif kind == "region":
                box = pkg.region_desc(desc, r["region"]["start"], r["region"]["size"])
                assert list(box.dims) == r["region"]["size"] and list(box.index_start) == list(fz.frame_start(r))
                seen["forms"].add(r["region"]["form"])
                seen["residues"].add((r["region"]["start"][0] * dt.itemsize) % 16)
                if r["region"]["form"] == "full_xy":
                    assert r["region"]["size"][:2] == [nx, ny] and r["region"]["start"][:2] == [0, 0]
                if r["region"]["form"] == "whole_buffer":
                    assert r["region"]["size"] == [nx, ny, nz]
                if r["region"]["form"] == "words_in_ragged":
                    assert r["region"]["size"][0] % 64 == 0 and nx % 64 != 0
                if r["region"]["form"] == "ragged_in_words":
                    assert nx % 64 == 0
            else:
                b = [fz._num(r["band"][k]) for k in ("lower", "upper", "inside", "outside")]
                pkg.check_band(code, tuple(b))
                seen["single_label"] += int(b[0] == b[1])
                seen["constant_band"] += int(b[2] == b[3])
                seen["inf_bound"] += int(dt.kind == "f" and (np.isinf(b[0]) or np.isinf(b[1])))
                seen["zero_bound"] += int(dt.kind == "f" and (b[0] == 0.0 or b[1] == 0.0))
    assert seen["forms"] == {"full_xy", "thin", "residue", "words_in_ragged", "ragged_in_words", "whole_buffer", "any"}
    assert seen["residues"] == set(range(16))
    assert min(seen[k] for k in ("nonfinite_ring", "single_label", "constant_band", "inf_bound", "zero_bound")) > 0, seen


def test_the_first_stream_draws_what_it_drew():
    """tests/golden/campaign_recipe_digests.json, recorded on the commit before cell pixels, components and the id offset
    entered the recipe (tests/golden/make_campaign_recipe_digests.py): restricted to the keys a recipe had then, every recipe of
    seeds 1 and 11 (cases 0 .. 299, default options) and of the five slice lists is byte for byte the recipe of that commit --
    the slice's seeds keep what they were chosen for, the cases of the committed logs replay -- and what is new is drawn from a
    stream of its own."""
    import sys
    import fuzz_campaign as fz
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_campaign_recipe_digests as mk
    finally:
        sys.path.pop(0)
    with open(os.path.join(ROOT, "tests", "golden", "campaign_recipe_digests.json")) as f:
        fixture = json.load(f)
    assert fixture["cases"] == mk.CASES == 300 and sorted(fixture["seeds"]) == ["1", "11"] and sorted(fixture["slices"]) == sorted(fz.KINDS)
    assert "cell_pixels" not in fixture["keys"] and {"kind", "dtype", "route", "kw", "field", "refusal", "drop_normals_row"} <= set(fixture["keys"])
    seeds, slices, recipes = mk.collect(fz, set(fixture["keys"]))
    for name, got, want in [("seed " + s, seeds[s], fixture["seeds"][s]) for s in sorted(seeds)] + [(k, slices[k], fixture["slices"][k]) for k in fz.KINDS]:
        assert len(got) == len(want)
        moved = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
        assert moved == [], "%s: the earlier draws of cases %s moved" % (name, moved[:10])
    # ... and the recipes of today hold the earlier keys and these, no others
    new = {"cell_pixels", "components", "drop_cell_rows", "emit_offset", "refusal_slab"}
    assert {k for r in recipes for k in r} == set(fixture["keys"]) | new


def test_recipes_survive_json_and_run_through_the_references(oracle):
    """Every kind, route, normals, repeat and refusal the campaign draws: the recipe is plain data, its JSON round trip rebuilds
    the same voxel bytes and the same expected mesh (and normals), and draw_case is a pure function of (seed, case)."""
    import fuzz_campaign as fz
    import test_components as cases
    from conftest import assert_same_mesh
    from normals_ref import same_normals
    seen = {"kinds": set(), "routes": set(), "normals": 0, "repeat": 0, "refusals": set(), "switch": 0, "beyond_2_53": 0}
    new = {"cell_pixels": 0, "components": 0, "all_three": 0, "drop_cell_rows": 0, "offset": 0, "offset_2_32": 0, "held": 0,
           "bspline": 0, "refusal_slab": set()}
    recipes = _recipes(160)
    assert recipes == _recipes(160)
    for r in recipes:
        text = json.dumps(r)
        back = json.loads(text)
        assert back == r and json.dumps(back) == text
        vox = fz.voxels(r)
        assert fz.voxels(back).tobytes() == vox.tobytes() and vox.dtype == np.dtype(r["dtype"]) and list(vox.shape) == r["field"]["shape"]
        want, again = fz.expected(oracle, r), fz.expected(oracle, back)
        assert_same_mesh(again["mesh"], want["mesh"])
        assert want["mesh"].cells.shape[1] == (3 if r["kw"]["triangles"] else 4)
        assert (want["normals"] is not None) == bool(r["normals"])
        if r["normals"]:
            same_normals(again["normals"], want["normals"])
            assert want["normals"].shape == want["mesh"].points.shape
            assert fz.frame(r)[0].size <= fz.NORMALS_MAX_VOXELS and r["route"] in fz.NORMALS_ROUTES
        if r["kind"] != "whole":
            assert r["kw"]["variant"] == 0 and "gradient" not in r["kw"] and r["route"] in fz.ROUTES[r["kind"]]
        if r["kind"] == "bspline":
            assert vox.size <= fz.BSPLINE_MAX_VOXELS and r["bspline"]["bits"] in (32, 64)
        seen["kinds"].add(r["kind"])
        seen["routes"].add(r["route"])
        seen["normals"] += int(r["normals"])
        seen["repeat"] += int(r["repeat"] == 3)
        seen["switch"] += int("switch" in r and r["kind"] != "whole")
        seen["beyond_2_53"] += int(vox.dtype.itemsize == 8 and vox.dtype.kind in "iu" and abs(int(vox.ravel()[0])) > 1 << 53)
        assert isinstance(r["drop_normals_row"], bool)
        if r.get("refusal"):
            assert r["refusal"] in fz.REFUSALS[r["kind"]] and r["refusal"] in fz.REFUSAL_TEXT
            assert r["refusal"] != "rg" or min(r["field"]["shape"]) >= 4     # (else the lines' length would be the reason)
            seen["refusals"].add(r["refusal"])
        # cell pixels, components, their rows, the id offset, the refused slab
        assert all(isinstance(r[k], bool) for k in ("cell_pixels", "components", "drop_cell_rows"))
        assert (want["cell_pixels"] is not None) == r["cell_pixels"] and (want["components"] is not None) == r["components"]
        assert ("emit_offset" in r) == (r["route"] == "count_emit")
        if r["route"] in ("slabs", "thin_slabs"):
            assert not r["cell_pixels"] and not r["components"]
        if r["cell_pixels"]:
            w, a = want["cell_pixels"], again["cell_pixels"]
            assert w.dtype == vox.dtype and w.shape == (len(want["mesh"].cells),) and a.dtype == w.dtype and a.tobytes() == w.tobytes()
        if r["components"]:
            cases.same(again["components"], want["components"], "components")
            cases.check_properties(want["mesh"].cells, len(want["mesh"].points), want["components"], "components")
            assert len(want["components"][0]) == len(want["mesh"].points) and len(want["components"][1]) == len(want["mesh"].cells)
        if "emit_offset" in r:
            assert isinstance(r["emit_offset"], int) and (0 <= r["emit_offset"] < 10 ** 6 or 2 ** 32 <= r["emit_offset"] < 2 ** 32 + 10 ** 6)
            new["offset"] += int(r["emit_offset"] > 0)
            new["offset_2_32"] += int(r["emit_offset"] >= 2 ** 32)
        if r["route"] == "held":
            assert r["drop_cell_rows"]
        if "refusal_slab" in r:
            assert r["kind"] == "whole" and r["route"] not in ("slabs", "thin_slabs", "held")
            assert r["refusal_slab"] in fz.SLAB_REFUSALS and r["refusal_slab"] in fz.REFUSALS["whole"] and r["refusal_slab"] in fz.REFUSAL_TEXT
            new["refusal_slab"].add(r["refusal_slab"])
        assert r.get("refusal") not in fz.SLAB_REFUSALS
        new["cell_pixels"] += int(r["cell_pixels"])
        new["components"] += int(r["components"])
        new["all_three"] += int(r["cell_pixels"] and r["components"] and r["normals"])
        new["drop_cell_rows"] += int(r["drop_cell_rows"])
        new["held"] += int(r["route"] == "held" and (r["cell_pixels"] or r["components"]))
        new["bspline"] += int(r["kind"] == "bspline" and (r["cell_pixels"] or r["components"]))
    assert min(v for k, v in new.items() if k != "refusal_slab") > 0 and new["refusal_slab"] == set(fz.SLAB_REFUSALS), new
    assert fz.REFUSAL_TEXT["cell_pixels_slab"] == "cell pixels" and fz.REFUSAL_TEXT["components_slab"] == "components"
    # the options fix the two settings wherever the route offers them, and nothing else moves
    for on in (True, False):
        fixed = _recipes(160, cell_pixels=on, components=on)
        for r, f in zip(recipes, fixed):
            assert f["cell_pixels"] == f["components"] == (on and r["route"] in fz.CELLDATA_ROUTES)
            assert {k: v for k, v in f.items() if k not in ("cell_pixels", "components")} == {k: v for k, v in r.items() if k not in ("cell_pixels", "components")}
    assert seen["kinds"] == set(fz.KINDS)
    assert seen["routes"] >= {"host", "device", "stream", "slabs", "thin_slabs", "count_emit", "held", "switch", "host_chunked"}
    assert len(seen["refusals"]) >= 5 and min(seen[k] for k in ("normals", "repeat", "switch", "beyond_2_53")) > 0, seen


def test_gpu_slice_conditions_hold_on_the_oracle(oracle):
    """The seeded slice of tests/test_gpu_campaign.py, from draw_case and the oracle alone: per kind and over the whole slice."""
    import fuzz_campaign as fz
    facts = []
    for kind in fz.KINDS:
        recipes = fz.slice_recipes(kind)
        assert len(recipes) == fz.SLICE[kind][1] >= 20
        for i, r in enumerate(recipes):
            assert (r["seed"], r["case"], r["kind"]) == (fz.SLICE[kind][0], i, kind)
            assert r["dtype"] == np.dtype(fz.DTYPES[i % 10]).name
            buf = r["field"]["shape"]                                        # [nz, ny, nx]
            box = r["region"]["size"][::-1] if kind == "region" else buf
            assert max(box[:2]) <= 12 and box[2] <= max(fz.XS) and np.prod(box) <= 30000
            assert all(0 <= b - a <= m for a, b, m in zip(box, buf, (7, 7, 87))) and np.prod(buf) <= 60000
            # cell pixels and components by the rule of the case number, wherever the route offers them
            offered = r["route"] in fz.CELLDATA_ROUTES
            assert r["cell_pixels"] == (offered and (i + i // 10) % 2 == 0) and r["components"] == (offered and i % 3 != 2)
        wants = [fz.expected(oracle, r) for r in recipes]
        mine = fz.slice_sequence_facts(recipes, wants)
        assert fz.slice_conditions(kind, mine) == []
        for r, w, f in zip(recipes, wants, mine):
            assert f["cell_pixels"] == r["cell_pixels"] and f["components"] == r["components"]
            if r["cell_pixels"]:
                assert len(w["cell_pixels"]) == len(w["mesh"].cells) and w["cell_pixels"].dtype == np.dtype(r["dtype"])
            if r["components"]:
                assert f["K"] == len(w["components"][2]) and (f["K"] == 0) == f["empty"]
        facts += mine
    assert fz.slice_conditions_overall(facts) == []
    # the conditions see what they are there for: without its cases each is reported missing
    assert any("K > 64" in m for m in fz.slice_conditions_overall([f for f in facts if not (f["components"] and f["K"] > 64)]))
    assert any("2^32" in m for m in fz.slice_conditions_overall([f for f in facts if f["offset"] < 2 ** 32]))
    assert any("pixel types" in m for m in fz.slice_conditions_overall([f for f in facts if not (f["cell_pixels"] and f["dtype"] == "float64")]))
    assert any("row of another size" in m for m in fz.slice_conditions_overall([f for f in facts if not f["other_pixels_row"]]))
    whole = [f for f in facts if f["kind"] == "whole"]
    assert any("K >= 2" in m for m in fz.slice_conditions("whole", [f for f in whole if not (f["components"] and f["K"] >= 2)]))


def test_compare_sees_one_bit(oracle):
    """compare() is the campaign's only judge: a mesh against itself passes, and one flipped bit of a coordinate, a swapped cell,
    a counter off by one or one flipped bit of a normal each fail; so do one flipped bit of a cell pixel, one label off by one in
    each of the three component rows, a K off by one, a missing row, a cell id below the id offset, and a first repeat (the
    settings off) whose mesh differs from the last by one bit."""
    import copy
    import fuzz_campaign as fz
    import pytest
    r = next(r for r in _recipes(200, kind="border", cell_pixels=True, components=True) if r["normals"] and r["kw"]["project"])
    assert r == next(dict(q, cell_pixels=True, components=True) for q in _recipes(200, kind="border") if q["normals"] and q["kw"]["project"])
    want = fz.expected(oracle, r)
    assert len(want["mesh"].points) > 3 and len(want["mesh"].cells) > 1 and len(want["cell_pixels"]) == len(want["mesh"].cells)

    def got():
        m = want["mesh"]
        return {"mesh": copy.deepcopy(m), "normals": want["normals"].copy(), "counters": {k: m.info[k] for k in fz.COUNTERS},
                "cell_pixels": want["cell_pixels"].copy(), "components": tuple(a.copy() for a in want["components"]),
                "n_components": len(want["components"][2])}
    fz.compare(got(), want)
    g = got()
    g["mesh"].points.view(np.uint32)[2, 1] ^= 1
    with pytest.raises(AssertionError):
        fz.compare(g, want)
    g = got()
    g["mesh"].cells[[0, 1]] = g["mesh"].cells[[1, 0]]
    with pytest.raises(AssertionError):
        fz.compare(g, want)
    g = got()
    g["counters"]["proj_iterations"] += 1
    with pytest.raises(AssertionError):
        fz.compare(g, want)
    g = got()
    finite = np.argwhere(np.isfinite(g["normals"]))
    assert len(finite)
    g["normals"].view(np.uint32)[tuple(finite[0])] ^= 1
    with pytest.raises(AssertionError):
        fz.compare(g, want)
    g = got()
    g["normals"] = None
    with pytest.raises(AssertionError):
        fz.compare(g, want)
    # cell pixels: one bit, the dtype, a missing row
    g = got()
    g["cell_pixels"].view(np.uint8)[-1] ^= 1
    with pytest.raises(AssertionError, match="cell pixels"):
        fz.compare(g, want)
    g = got()
    g["cell_pixels"] = g["cell_pixels"][:-1]
    with pytest.raises(AssertionError, match="cell pixels"):
        fz.compare(g, want)
    g = got()
    g["cell_pixels"] = None
    with pytest.raises(AssertionError, match="no cell pixels"):
        fz.compare(g, want)
    # components: one label off by one in each of the three rows, K, a missing row
    for row in range(3):
        g = got()
        g["components"][row][-1] += 1
        with pytest.raises(AssertionError, match="component"):
            fz.compare(g, want)
    g = got()
    g["n_components"] += 1
    with pytest.raises(AssertionError, match="K"):
        fz.compare(g, want)
    for row in range(3):
        g = got()
        g["components"] = tuple(a[:-1] if k == row else a for k, a in enumerate(g["components"]))
        with pytest.raises(AssertionError, match="component"):
            fz.compare(g, want)
    g = got()
    g["components"] = None
    with pytest.raises(AssertionError, match="no components"):
        fz.compare(g, want)
    # the id offset: taken off the cells; a cell below it, or an offset the cells do not carry, fails
    g = got()
    g["emit_offset"] = 2 ** 32 + 5
    with pytest.raises(AssertionError, match="id offset"):
        fz.compare(g, want)
    g = got()
    g["emit_offset"] = 2 ** 32 + 5
    g["mesh"].cells = g["mesh"].cells + np.uint64(2 ** 32 + 5)
    carried = copy.deepcopy(g["mesh"])
    fz.compare(g, want)
    # a case that repeats: the first repeat ran with the settings off, its mesh and counters are the last one's
    g["first_mesh"], g["first_counters"] = carried, dict(g["counters"])
    fz.compare(g, want)
    g["first_mesh"].points.view(np.uint32)[1, 2] ^= 1
    with pytest.raises(AssertionError, match="off"):
        fz.compare(g, want)
    g["first_mesh"] = copy.deepcopy(g["mesh"])
    g["first_counters"]["proj_stop_steps"] += 1
    with pytest.raises(AssertionError, match="off"):
        fz.compare(g, want)
