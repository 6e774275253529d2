"""-m "not gpu": the hand-run campaign and profile scripts stay importable, and the campaign's generators stay inside what the
oracle accepts (every drawn volume, geometry, start index and held first volume runs through it) -- so that the scripts do not rot
between the rounds in which somebody runs them on a GPU box.  The campaign's new dimensions too: every drawn border value, box
and band passes its validator, every drawn recipe survives JSON, rebuilds the same bytes and runs through expected(); and the
seeded slice of tests/test_gpu_campaign.py holds the conditions that keep it from hiding a failure, shown on the oracle alone.
Cell pixels, components, their rows and the id offset come from a stream of their own: what the campaign drew before them is
held, draw for draw, to a fixture recorded on the commit before (tests/golden/campaign_recipe_digests.json); the keep comes from a
third stream, and a second fixture (campaign_celldata_recipe_digests.json) holds the second stream the same way.  The keep's
reference is keep_ref.keep on the oracle's mesh and the references' rows: its closure, its purity and compare()'s eye for one bit
of a kept row are shown here on the oracle alone."""
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
    stream of its own.  tests/golden/campaign_celldata_recipe_digests.json, recorded the same way on the commit before `keep`
    entered the recipe, holds the second stream -- cell pixels, components, their rows, the id offset, the refused slab -- to what
    it drew then: the only key beyond that fixture's is `keep`, from a third stream."""
    import sys
    import fuzz_campaign as fz
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_campaign_recipe_digests as mk
    finally:
        sys.path.pop(0)
    second = {"cell_pixels", "components", "drop_cell_rows", "emit_offset", "refusal_slab"}
    for name, new in (("campaign_recipe_digests.json", second | {"keep"}), ("campaign_celldata_recipe_digests.json", {"keep"})):
        with open(os.path.join(ROOT, "tests", "golden", name)) as f:
            fixture = json.load(f)
        assert fixture["cases"] == mk.CASES == 300 and sorted(fixture["seeds"]) == ["1", "11"] and sorted(fixture["slices"]) == sorted(fz.KINDS)
        assert {"kind", "dtype", "route", "kw", "field", "refusal", "drop_normals_row"} <= set(fixture["keys"]) and "keep" not in fixture["keys"]
        assert ("cell_pixels" in fixture["keys"]) == (new == {"keep"}) == (second <= set(fixture["keys"]))
        seeds, slices, recipes = mk.collect(fz, set(fixture["keys"]))
        for what, got, want in [("seed " + s, seeds[s], fixture["seeds"][s]) for s in sorted(seeds)] + [(k, slices[k], fixture["slices"][k]) for k in fz.KINDS]:
            assert len(got) == len(want)
            moved = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
            assert moved == [], "%s, %s: the earlier draws of cases %s moved" % (name, what, moved[:10])
        # ... and the recipes of today hold the earlier keys and these, no others
        assert {k for r in recipes for k in r} == set(fixture["keys"]) | new


def test_the_envelope_stream_draws_what_its_digests_say():
    """tests/golden/campaign_envelope_recipe_digests.json (tests/golden/make_campaign_recipe_digests.py --envelope): every recipe
    drawn with the option `envelope` on, seeds 1 and 11, cases 0 .. 299, and the slice of tests/test_gpu_campaign.py, in blocks
    of 25 cases, whole and as their `envelope` entries alone.  Off, the option adds no key and moves no draw (test_the_first_stream_draws_what_it_drew); on, the
    first stream still draws what it drew: everything the envelope does not touch is the plain recipe's."""
    import sys
    import fuzz_campaign as fz
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_campaign_recipe_digests as mk
    finally:
        sys.path.pop(0)
    with open(os.path.join(ROOT, "tests", "golden", "campaign_envelope_recipe_digests.json")) as f:
        fixture = json.load(f)
    assert mk.collect_envelope(fz) == fixture
    assert fixture["envelope_keys"] == ["origin", "spacing_exp", "start", "voxel_exp"] and len(fixture["slice"]) == -(-fz.ENVELOPE_SLICE[1] // mk.ENVELOPE_BLOCK)
    touched = {"envelope", "spacing", "origin", "index_start", "field", "iso", "kw", "band", "normals", "cuts", "route", "keep", "first"}
    near = 0
    for case in range(120):
        plain, env = fz.draw_case(1, case), fz.draw_case(1, case, dict(envelope=True))
        assert "envelope" not in plain and set(env) - set(plain) <= {"envelope", "cuts"}
        assert {k: v for k, v in env.items() if k not in touched} == {k: v for k, v in plain.items() if k not in touched}, case
        e = env["envelope"]
        k = e["spacing_exp"]
        assert -100 <= k <= 100 and env["spacing"] == [float(np.ldexp(v, k)) for v in plain["spacing"]] and env["origin"] == e["origin"]
        assert max(abs(v) for v in e["origin"]) <= 1e9
        lo, hi = fz.ENVELOPE_VOXEL_EXP.get(env["dtype"], (0, 0))
        assert lo <= e["voxel_exp"] <= hi and env["field"].get("scale_exp") == e["voxel_exp"]
        if e["start"]:
            near += 1
            assert env["index_start"] == e["start"] and all((1 << 30) - 100 < abs(v) <= (1 << 30) - 40 for v in e["start"])
        else:
            assert env["index_start"] == plain["index_start"]
        if env["kw"]["variant"] == 2:
            assert fz.linesearch_defined(fz.voxels(env), env["iso"]), case
        if e["voxel_exp"] and np.dtype(env["dtype"]).kind == "f":       # a power of two: the finite voxels scale exactly, or leave the type
            a, b = fz.voxels(dict(plain, field=dict(env["field"], scale_exp=0))).astype(np.float64), fz.voxels(env).astype(np.float64)
            exact = np.isfinite(b) & (b != 0) & (np.abs(b) >= np.finfo(env["dtype"]).tiny)
            assert np.array_equal(np.ldexp(a[exact], e["voxel_exp"]), b[exact]), case
    assert 4 <= near <= 25                                              # one case of ten


def test_envelope_slice_conditions_hold_on_the_oracle(oracle):
    """The envelope's seeded slice of tests/test_gpu_campaign.py shows what envelope_slice_conditions asks -- every kind, voxel
    scales at both ends of both float types, spacings beyond 2^+-50, start indices near +-2^30, line-search cases under the
    10000 rule, walked meshes that stay finite and walked meshes that go NaN -- from the recipes and the references alone."""
    import fuzz_campaign as fz
    recipes = fz.envelope_slice_recipes()
    assert len(recipes) == 60 and recipes == json.loads(json.dumps(recipes))
    wants = [fz.expected(oracle, r) for r in recipes]
    assert fz.envelope_slice_conditions(recipes, wants) == []


def test_recipes_survive_json_and_run_through_the_references(oracle):
    """Every kind, route, normals, repeat and refusal the campaign draws: the recipe is plain data, its JSON round trip rebuilds
    the same voxel bytes and the same expected mesh (and normals), and draw_case is a pure function of (seed, case).  The keep
    (recipe["keep"]): there only with components, resolved by a pure keep_arguments on the reference's counts, every stage's rows
    the components of the kept reference mesh; the three rules, a second stage, K' = 0 and K' = K are all seen."""
    import components_ref
    import fuzz_campaign as fz
    import test_components as cases
    from conftest import assert_same_mesh
    from normals_ref import same_normals
    seen = {"kinds": set(), "routes": set(), "normals": 0, "repeat": 0, "refusals": set(), "switch": 0, "beyond_2_53": 0}
    new = {"cell_pixels": 0, "components": 0, "all_three": 0, "drop_cell_rows": 0, "offset": 0, "offset_2_32": 0, "held": 0,
           "bspline": 0, "refusal_slab": set()}
    keeps = {"largest": 0, "min_cells": 0, "mask": 0, "then": 0, "to_nothing": 0, "all_kept": 0, "some": 0, "odd_bytes": 0}
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
        # the keep: only with components; plain data (the round trip above); its stages resolved on the reference's counts
        assert "keep" in r and (r["keep"] is None or r["components"])
        stages = fz.keep_stages(r["keep"])
        assert len(want["kept"]) == len(want["keep_args"]) == len(stages) and len(stages) == (0 if r["keep"] is None else 1 + bool(r["keep"]["then"]))
        counts = want["components"][2] if r["components"] else None
        for stage, kept, args, more in zip(stages, want["kept"], want["keep_args"], again["kept"]):
            assert stage["rule"] in fz.KEEP_RULES and args[0] == stage["rule"]
            held = counts.copy()
            twice = fz.keep_arguments(stage, counts), fz.keep_arguments(json.loads(json.dumps(stage)), list(counts))
            assert counts.tobytes() == held.tobytes()
            for a in twice:
                assert a[:2] == args[:2] and (a[2] is None) == (args[2] is None) == (stage["rule"] != "mask")
                assert a[2] is None or (a[2].dtype == np.uint8 and a[2].shape == (len(counts),) and a[2].tobytes() == args[2].tobytes())
            assert all(getattr(kept, n) is None if getattr(more, n) is None else getattr(kept, n).tobytes() == getattr(more, n).tobytes() for n in kept._fields)
            assert (kept.normals is not None) == r["normals"] and (kept.cell_pixels is not None) == r["cell_pixels"]
            # closure: the kept rows are the components of the kept mesh
            rows = (kept.point_component, kept.cell_component, kept.component_cells)
            cases.same(rows, components_ref.components(kept.cells, len(kept.points)), "closure")
            cases.check_properties(kept.cells, len(kept.points), rows, "kept")
            assert kept.cells.shape[1:] == want["mesh"].cells.shape[1:] and len(kept.component_cells) <= len(counts)
            if stage is stages[0]:
                keeps[stage["rule"]] += 1
                keeps["all_kept"] += int(len(kept.component_cells) == len(counts) >= 2)
                keeps["some"] += int(0 < len(kept.component_cells) < len(counts))
            keeps["odd_bytes"] += int(args[2] is not None and bool((args[2] > 1).any()))
            counts = kept.component_cells
        if stages:
            keeps["then"] += int(len(stages) == 2)
            keeps["to_nothing"] += int(len(want["components"][2]) >= 1 and len(want["kept"][-1].component_cells) == 0)
        new["cell_pixels"] += int(r["cell_pixels"])
        new["components"] += int(r["components"])
        new["all_three"] += int(r["cell_pixels"] and r["components"] and r["normals"])
        new["drop_cell_rows"] += int(r["drop_cell_rows"])
        new["held"] += int(r["route"] == "held" and (r["cell_pixels"] or r["components"]))
        new["bspline"] += int(r["kind"] == "bspline" and (r["cell_pixels"] or r["components"]))
    assert min(v for k, v in new.items() if k != "refusal_slab") > 0 and new["refusal_slab"] == set(fz.SLAB_REFUSALS), new
    assert fz.REFUSAL_TEXT["cell_pixels_slab"] == "cell pixels" and fz.REFUSAL_TEXT["components_slab"] == "components"
    assert min(keeps.values()) > 0, keeps
    # the options fix the two settings wherever the route offers them, and nothing else moves
    for on in (True, False):
        fixed = _recipes(160, cell_pixels=on, components=on)
        for r, f in zip(recipes, fixed):
            assert f["cell_pixels"] == f["components"] == (on and r["route"] in fz.CELLDATA_ROUTES)
            # (the keep is drawn from a stream of its own and is there only with components)
            assert f["keep"] is None or f["components"]
            assert {k: v for k, v in f.items() if k not in ("cell_pixels", "components", "keep")} == {k: v for k, v in r.items() if k not in ("cell_pixels", "components", "keep")}
        kept = _recipes(160, keep=on)
        for r, f in zip(recipes, kept):
            assert (f["keep"] is not None) == (on and r["components"])
            assert r["keep"] is None or f["keep"] is None or f["keep"] == r["keep"]
            assert {k: v for k, v in f.items() if k != "keep"} == {k: v for k, v in r.items() if k != "keep"}
    assert seen["kinds"] == set(fz.KINDS)
    assert seen["routes"] >= {"host", "device", "stream", "slabs", "thin_slabs", "count_emit", "held", "switch", "host_chunked"}
    assert len(seen["refusals"]) >= 5 and min(seen[k] for k in ("normals", "repeat", "switch", "beyond_2_53")) > 0, seen


def test_gpu_slice_conditions_hold_on_the_oracle(oracle):
    """The seeded slice of tests/test_gpu_campaign.py, from draw_case and the oracle alone: per kind and over the whole slice --
    the keep's conditions among them (fuzz_campaign.slice_conditions, slice_conditions_overall)."""
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
            # every components case keeps, by the rule of the case number
            assert (r["keep"] is not None) == r["components"]
            assert r["keep"] is None or r["keep"]["rule"] == ("largest", "min_cells", "mask")[(i // 2) % 3]
        wants = [fz.expected(oracle, r) for r in recipes]
        mine = fz.slice_sequence_facts(recipes, wants)
        assert fz.slice_conditions(kind, mine) == []
        for r, w, f in zip(recipes, wants, mine):
            assert f["cell_pixels"] == r["cell_pixels"] and f["components"] == r["components"]
            if r["cell_pixels"]:
                assert len(w["cell_pixels"]) == len(w["mesh"].cells) and w["cell_pixels"].dtype == np.dtype(r["dtype"])
            if r["components"]:
                assert f["K"] == len(w["components"][2]) and (f["K"] == 0) == f["empty"]
                assert f["keep"]["ks"][0] == f["K"] and len(f["keep"]["ks"]) == 1 + len(w["kept"]) == 2 + bool(r["keep"]["then"])
            else:
                assert f["keep"] is None and w["kept"] == []
        facts += mine
    assert fz.slice_conditions_overall(facts) == []
    # the conditions see what they are there for: without its cases each is reported missing
    assert any("K > 64" in m for m in fz.slice_conditions_overall([f for f in facts if not (f["components"] and f["K"] > 64)]))
    assert any("2^32" in m for m in fz.slice_conditions_overall([f for f in facts if f["offset"] < 2 ** 32]))
    assert any("pixel types" in m for m in fz.slice_conditions_overall([f for f in facts if not (f["cell_pixels"] and f["dtype"] == "float64")]))
    assert any("row of another size" in m for m in fz.slice_conditions_overall([f for f in facts if not f["other_pixels_row"]]))
    # ... the keep's too: K' = 0, the id offset of 2^32 and more that drops something, each setting behind a keep, the rules
    gone = fz.slice_conditions_overall([f for f in facts if not (f["keep"] and f["keep"]["ks"][0] >= 1 and f["keep"]["ks"][-1] == 0)])
    assert any("K' = 0" in m for m in gone), gone
    gone = fz.slice_conditions_overall([f for f in facts if not (f["keep"] and f["offset"] >= 2 ** 32 and f["keep"]["ks"][-1] < f["keep"]["ks"][0])])
    assert any("2^32 that drops something" in m for m in gone), gone
    for name, text in (("normals", "normals"), ("cell_pixels", "cell pixels"), ("components", "components")):
        gone = fz.slice_conditions_overall([f for f in facts if name not in f["behind_keep"]])
        assert any("%s behind a keep" % text in m for m in gone), gone
    gone = fz.slice_conditions_overall([f for f in facts if not (f["keep"] and f["keep"]["rule"] == "mask" and f["keep"]["first_some"])])
    assert any("rule mask" in m for m in gone), gone
    assert any("K > 64" in m and "keep" in m for m in fz.slice_conditions_overall([f for f in facts if not (f["keep"] and f["K"] > 64)]))
    whole = [f for f in facts if f["kind"] == "whole"]
    assert any("0 < K' < K" in m for m in fz.slice_conditions("whole", [f for f in whole if not (f["keep"] and f["keep"]["first_some"])]))
    assert any("K >= 2" in m for m in fz.slice_conditions("whole", [f for f in whole if not (f["components"] and f["K"] >= 2)]))


def test_compare_sees_one_bit(oracle):
    """compare() is the campaign's only judge: a mesh against itself passes, and one flipped bit of a coordinate, a swapped cell,
    a counter off by one or one flipped bit of a normal each fail; so do one flipped bit of a cell pixel, one label off by one in
    each of the three component rows, a K off by one, a missing row, a cell id below the id offset, and a first repeat (the
    settings off) whose mesh differs from the last by one bit.  The keep, on a recipe with normals, cell pixels, components and a
    keep that drops something, the reference against itself: one flipped bit in a kept point, normal or cell pixel, one kept cell
    id left un-renumbered, one label off by one in each kept row, K' or a returned count off by one, a counter changed by the
    keep, a missing stage and a non-null pointer for an empty row each fail."""
    import copy
    import fuzz_campaign as fz
    import pytest
    r = next(r for r in _recipes(200, kind="border", cell_pixels=True, components=True) if r["normals"] and r["kw"]["project"])
    # (the keep is drawn from a stream of its own: it is the one thing the options' recipe holds beyond the plain one's)
    assert r == next(dict(q, cell_pixels=True, components=True, keep=r["keep"]) for q in _recipes(200, kind="border") if q["normals"] and q["kw"]["project"])
    want = fz.expected(oracle, r)
    assert len(want["mesh"].points) > 3 and len(want["mesh"].cells) > 1 and len(want["cell_pixels"]) == len(want["mesh"].cells)

    def stage(w, k_before, counters):
        """What run_case records behind one keep, from the reference's own Kept."""
        mesh = copy.deepcopy(want["mesh"])
        mesh.points, mesh.cells = w.points.copy(), w.cells.copy()
        sizes = (len(w.points), len(w.cells), len(w.component_cells))
        return {"returned": sizes, "ms": 0.0, "result": sizes[:2], "mesh": mesh, "normals": None if w.normals is None else w.normals.copy(),
                "cell_pixels": None if w.cell_pixels is None else w.cell_pixels.copy(),
                "components": (w.point_component.copy(), w.cell_component.copy(), w.component_cells.copy()), "n_components": sizes[2],
                "null": tuple(n == 0 for n in sizes), "counters_before": dict(counters), "counters": dict(counters), "k_before": k_before}

    def got(want=want):
        m = want["mesh"]
        counters = {k: m.info[k] for k in fz.COUNTERS}
        ks = [len(want["components"][2])] + [len(w.component_cells) for w in want["kept"]]
        return {"mesh": copy.deepcopy(m), "normals": want["normals"].copy(), "counters": counters,
                "cell_pixels": want["cell_pixels"].copy(), "components": tuple(a.copy() for a in want["components"]),
                "n_components": len(want["components"][2]), "kept": [stage(w, k, counters) for w, k in zip(want["kept"], ks)]}
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

    # ---- the keep: the reference against itself, stage by stage ----
    for rk in _recipes(200, kind="border", cell_pixels=True, components=True, keep="min_cells"):
        if not (rk["normals"] and rk["kw"]["project"] and rk["keep"]["pick"] == "quantile"):
            continue
        wk = fz.expected(oracle, rk)
        first = wk["kept"][0]
        # the cells of the mesh that the first stage keeps, with the ids they had before: some of them are renumbered
        old = wk["mesh"].cells[np.isin(wk["components"][1], np.flatnonzero(np.isin(wk["components"][2], first.component_cells)))]
        if 0 < len(first.component_cells) < len(wk["components"][2]) and len(first.cells) > 1 and old.shape == first.cells.shape \
                and (old != first.cells).any() and np.isfinite(first.normals).any():
            break
    else:
        raise AssertionError("no recipe with normals, cell pixels, components and a keep that drops something")
    assert len(first.points) < len(wk["mesh"].points) and len(first.cells) < len(wk["mesh"].cells) and first.cell_pixels is not None
    fz.compare(got(wk), wk)

    def fails(change, match):
        g = got(wk)
        change(g["kept"][0], g)
        with pytest.raises(AssertionError, match=match):
            fz.compare(g, wk)

    def flip(row, at):
        row.view(np.uint8 if row.dtype.itemsize == 1 else np.uint32)[at] ^= 1
    moved = tuple(np.argwhere(old != first.cells)[0])
    finite = tuple(np.argwhere(np.isfinite(first.normals))[0])
    fails(lambda k, g: flip(k["mesh"].points, (1, 2)), "keep stage 0")                              # one bit of a kept point
    fails(lambda k, g: flip(k["normals"], finite), "keep stage 0: normals")                         # ... of a kept normal
    fails(lambda k, g: flip(k["cell_pixels"].view(np.uint8), -1), "cell pixels")                    # ... of a kept cell pixel
    fails(lambda k, g: k["mesh"].cells.__setitem__(moved, old[moved]), "keep stage 0")              # one id left un-renumbered
    for row in range(3):
        fails(lambda k, g: k["components"][row].__setitem__(-1, k["components"][row][-1] + 1), "component")
    fails(lambda k, g: k.__setitem__("n_components", k["n_components"] + 1), "K")
    for at in range(3):
        fails(lambda k, g: k.__setitem__("returned", tuple(v + (i == at) for i, v in enumerate(k["returned"]))), "returned counts")
    fails(lambda k, g: k.__setitem__("result", (k["result"][0], k["result"][1] - 1)), "result counts")
    fails(lambda k, g: k["counters"].__setitem__("proj_iterations", k["counters"]["proj_iterations"] + 1), "counters changed by the keep")
    fails(lambda k, g: g["kept"].pop(), "keep stages ran")                                          # a missing stage
    fails(lambda k, g: g.__setitem__("kept", []), "keep stages ran")
    fails(lambda k, g: k.__setitem__("null", (False, False, True)), "null device pointers")
    # an id offset: carried by the kept cells, taken off; a kept id outside [offset, offset + kept points) fails
    g = got(wk)
    g["emit_offset"] = 2 ** 32 + 5
    g["mesh"].cells = g["mesh"].cells + np.uint64(2 ** 32 + 5)
    with pytest.raises(AssertionError, match="kept cell id outside"):
        fz.compare(g, wk)
    for k in g["kept"]:
        k["mesh"].cells = k["mesh"].cells + np.uint64(2 ** 32 + 5)
    fz.compare(g, wk)
    g["kept"][0]["mesh"].cells[0, 0] = np.uint64(2 ** 32 + 5 + len(first.points))
    with pytest.raises(AssertionError, match="kept cell id outside"):
        fz.compare(g, wk)
    # a keep to nothing: every pointer of an empty row is null, and a non-null one fails
    nothing = dict(rk, keep=dict(rule="min_cells", pick="above_max", quantile=0.0, plus_one=False, then=None))
    wn = fz.expected(oracle, nothing)
    assert len(wn["kept"]) == 1 and len(wn["kept"][0].points) == len(wn["kept"][0].cells) == len(wn["kept"][0].component_cells) == 0
    fz.compare(got(wn), wn)
    for at in range(3):
        g = got(wn)
        g["kept"][0]["null"] = tuple(i != at for i in range(3))
        with pytest.raises(AssertionError, match="null device pointers"):
            fz.compare(g, wn)


# ---- the campaign through the C++ drop-in filter (tests/fuzz_dropin.py, tests/test_gpu_dropin_campaign.py) -------------------------
_DROPIN = {}


def _dropin_slice(oracle):
    """{kind: (lines, references, script)} of the drop-in slice, prepared once per process (no GPU: the oracle and the numpy
    references alone; the volumes are not written)."""
    import fuzz_campaign as fz
    import fuzz_dropin as fd
    if not _DROPIN:
        for kind in fz.KINDS:
            _DROPIN[kind] = fd.prepare(oracle, fd.slice_recipes(kind))
    return _DROPIN


def test_the_dropin_stream_draws_what_its_digests_say():
    """tests/golden/campaign_dropin_recipe_digests.json (tests/golden/make_campaign_recipe_digests.py --dropin): every recipe of
    fuzz_dropin.draw_case for seeds 1 and 11, cases 0 .. 299, and of the five slice lists, whole and as its `dropin` entry alone.
    The entry comes from a stream of its own -- the two older fixtures, which test_the_first_stream_draws_what_it_drew holds
    fuzz_campaign.draw_case to, are not touched by it -- and a drop-in recipe is fuzz_campaign's recipe of the same (seed, case)
    wherever the filter's route leaves the draw alone."""
    import sys
    import fuzz_campaign as fz
    import fuzz_dropin as fd
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_campaign_recipe_digests as mk
    finally:
        sys.path.pop(0)
    with open(os.path.join(ROOT, "tests", "golden", "campaign_dropin_recipe_digests.json")) as f:
        fixture = json.load(f)
    assert mk.collect_dropin(fd) == fixture
    assert fixture["slice_seeds"] == fd.SLICE and sorted(fixture["slices"]) == sorted(fz.KINDS) and fixture["cases"] == 300
    # pure, plain data, and the volume, the geometry and the parameters are the C ABI campaign's of the same (seed, case)
    for case in range(60):
        r = fd.draw_case(11, case)
        assert r == fd.draw_case(11, case) == json.loads(json.dumps(r))
        q = fz.draw_case(11, case, dict(route=r["route"], kind=r["kind"]))
        for key in ("kind", "dtype", "field", "spacing", "origin", "direction", "index_start", "iso", "border", "region", "band", "bspline", "first"):
            assert r.get(key) == q.get(key), (case, key)
        assert r["kw"] == dict(q["kw"], variant=0) and set(r["dropin"]) == set(fixture["dropin_keys"])
        assert r["keep"] is None or r["keep"]["rule"] in ("largest", "min_cells") and (r["keep"]["then"] is None or r["keep"]["rule"] == "largest" and r["keep"]["then"]["rule"] == "min_cells")


def test_dropin_scripts_round_trip_through_the_binary(oracle):
    """Recipe -> script -> the binary's mode without a GPU -> getters, for every line of the slice: every setter lands, the image
    description and the buffer box are the recipe's, nan / inf / 64-bit values arrive exact -- and, on lines made for it, the
    reference's clamps hold (the threshold against NumericTraits<InputPixelType>::max(), the step length, the relaxation factor,
    the host-walk threads)."""
    import copy
    import fuzz_campaign as fz
    import fuzz_dropin as fd
    seen = {"inf": 0, "beyond_2_53": 0, "region": 0, "band": 0, "moved": 0, "keep_step": 0, "lines": 0}
    for kind in fz.KINDS:
        lines, _, script = _dropin_slice(oracle)[kind]
        got, want = fd.parse_dry(fd.run_dry(script), lines), fd.dry_getters(lines)
        assert len(got) == len(want) == len(lines) == len(script.splitlines())
        for number, (g, w) in enumerate(zip(got, want)):
            assert g == w, (kind, number, {k: (g.get(k), w.get(k)) for k in set(g) | set(w) if g.get(k) != w.get(k)})
            s = lines[number]["settings"]
            values = [s["iso"], s["border"]] + list(s["band"] or [])
            seen["inf"] += any(isinstance(v, str) and "inf" in v for v in values)
            seen["beyond_2_53"] += any(isinstance(v, int) and abs(v) > 2 ** 53 for v in values)
            seen["region"] += s["region"] is not None and any(g["box"][:3])
            seen["band"] += bool(s["bandon"])
            seen["moved"] += any(s["start"])
            seen["keep_step"] += s["step"] is None
            seen["lines"] += 1
    assert min(seen.values()) > 0, seen
    # the clamps, on lines of the slice whose values are pushed past them
    lines = copy.deepcopy([l for l in _dropin_slice(oracle)["whole"][0] if l["settings"]["dtype"] in ("uint8", "int8", "int64", "float32")][:8])
    for i, line in enumerate(lines):
        line["settings"].update(thr=[1000.0, -3.0, 1e30, 1e300][i % 4], step=[-5.0, 1e6, 0.0, 123.5][i % 4], relax=[2.0, -1.0, 1.0, 0.25][i % 4],
                                threads=[0, 1000, 4, 256][i % 4], fresh=True)
        if line["settings"]["dtype"] == "float32":       # (the slice draws no NaN: a ring of NaN, a band of -inf .. inf mapped to -0 and NaN)
            line["settings"].update(border="nan", band=["-inf", "inf", -0.0, "nan"], bandon=True)
    script = "\n".join(fd.script_line(n, l, "-", "-") for n, l in enumerate(lines)) + "\n"
    got, want = fd.parse_dry(fd.run_dry(script), lines), fd.dry_getters(lines)
    assert got == want
    assert any(g["border"] == "nan" and g["band"] == [float("-inf").hex(), float("inf").hex(), (-0.0).hex(), "nan"] for g in got)
    by = {l["settings"]["dtype"]: g for l, g in zip(lines, got) if l["settings"]["thr"] == 1000.0}
    assert any(g["thr"] == float(hi).hex() for dt, hi in (("uint8", 255), ("int8", 127)) for g in [by.get(dt)] if g), by
    assert {g["step"] for g in got} == {0.0.hex(), 100000.0.hex(), 123.5.hex()} and {g["relax"] for g in got} == {1.0.hex(), 0.0.hex(), 0.25.hex()}
    assert {g["threads"] for g in got} == {1, 256, 4}


def test_dropin_slice_conditions_hold_on_the_oracle(oracle):
    """The seeded slice of tests/test_gpu_dropin_campaign.py from the recipes and the oracle alone: fuzz_dropin.slice_conditions,
    the cap on empty reference meshes among them; the conditions see what they are there for."""
    import fuzz_campaign as fz
    import fuzz_dropin as fd
    facts = []
    for kind in fz.KINDS:
        lines, refs, _ = _dropin_slice(oracle)[kind]
        recipes = fd.slice_recipes(kind)
        assert len(recipes) == 20 and [l["case"] for l in lines if l["sub"] == "main"] == list(range(20))
        for i, r in enumerate(recipes):
            assert (r["seed"], r["case"], r["kind"], r["dtype"]) == (fd.SLICE[kind], i, kind, np.dtype(fz.DTYPES[i % 10]).name)
            buf = r["field"]["shape"]
            box = r["region"]["size"][::-1] if kind == "region" else buf
            assert max(box[:2]) <= 12 and np.prod(box) <= 30000 and np.prod(buf) <= 60000
        mine = fd.slice_facts(lines, refs)
        mains = [f for f in mine if f["sub"] == "main"]
        assert len(mains) == 20 and 4 * sum(f["empty"] for f in mains) <= 20
        facts += mine
    assert fd.slice_conditions(facts) == []
    gone = lambda keep: fd.slice_conditions([f for f in facts if keep(f)])                      # noqa: E731
    assert any("hw_keep" in m for m in gone(lambda f: f["refusal"] != "hw_keep"))
    assert any("followed by a full case" in m for m in gone(lambda f: not f["behind_throw"]))
    assert any("fewer slices" in m for m in gone(lambda f: f["threw"] or f["devices"] <= f["slices"]))
    assert any("2^53" in m for m in gone(lambda f: f["threw"] or not (f["host_walk"] and f["beyond_2_53"])))
    assert any("sticks" in m for m in gone(lambda f: f["threw"] or not f["sticks"]))
    assert any("switch stale" in m for m in gone(lambda f: "stale" not in f["turned_off"]))
    assert any("single, then group" in m for m in gone(lambda f: f["threw"] or f["devices"] <= 1))
    assert any("leaves nothing" in m for m in gone(lambda f: f["threw"] or not (f["ks"] and f["ks"][-1] == 0)))
    assert any("host-walk path" in m for m in gone(lambda f: f["threw"] or not (f["interp"] == "inherit" and f["dtype"] == "uint64")))


def test_the_dropin_comparer_sees_one_bit(oracle, tmp_path):
    """fuzz_dropin.compare_line is the drop-in campaign's only judge.  From a fabricated output directory that equals the
    reference (fuzz_dropin.write_reference: the files the binary writes) the comparison passes; one flipped bit in a point, a cell
    id, a cell datum, a normal, a cell pixel, each of the three component rows, K, the slab count or the step length fails it, and
    so do a dropped cell-data container, a cell of another arity, an Update() that threw, a refusal that was accepted and a
    refusal with another text."""
    import fuzz_dropin as fd
    import pytest
    import fuzz_campaign as fz
    lines, refs, number = next((ls, rs, n) for ls, rs, _ in (_dropin_slice(oracle)[k] for k in fz.KINDS) for n, (l, r) in enumerate(zip(ls, rs))
                               if not r["threw"] and l["settings"]["normals"] and l["settings"]["celldata"] and l["settings"]["components"]
                               and len(r["cells"]) > 1 and r["K"] >= 1 and np.isfinite(r["normals"]).any())
    line, ref = lines[number], refs[number]
    s = line["settings"]
    out = str(tmp_path)

    def fresh():
        fd.write_reference(ref, out, number, s["traits"])
    fresh()
    fd.compare_line(fd.read_line(out, number, s), ref)
    base = os.path.join(out, "%d." % number)
    finite = int(np.flatnonzero(np.isfinite(ref["normals"]).ravel())[0])
    for name, byte, match in (("points", 4, "coordinates differ"), ("cells", 8, "cell topology"), ("celldata", 0, "cell data"), ("normals", 4 * finite, "normals"),
                              ("pixels", 0, "cell pixels"), ("pcomp", 0, "pcomp"), ("ccomp", 0, "ccomp"), ("counts", 0, "counts"), ("arity", 1, "a cell of")):
        fresh()
        raw = bytearray(open(base + name, "rb").read())
        raw[byte] ^= 1
        open(base + name, "wb").write(bytes(raw))
        with pytest.raises(AssertionError, match=match):
            fd.compare_line(fd.read_line(out, number, s), ref)

    def meta(change):
        fresh()
        text = open(base + "meta").read()
        changed = change(text)
        assert changed != text
        open(base + "meta", "w").write(changed)
    meta(lambda t: t.replace("K=%d" % ref["K"], "K=%d" % (ref["K"] ^ 1)))
    with pytest.raises(AssertionError, match="GetNumberOfComponents"):
        fd.compare_line(fd.read_line(out, number, s), ref)
    meta(lambda t: t.replace("slabs=1", "slabs=0"))
    with pytest.raises(AssertionError, match="GetLastNumberOfSlabs"):
        fd.compare_line(fd.read_line(out, number, s), ref)
    meta(lambda t: t.replace("step=" + fd._real(ref["step"]), "step=" + fd._real(np.nextafter(ref["step"], 1e9))))
    with pytest.raises(AssertionError, match="GetProjectVertexStepLength"):
        fd.compare_line(fd.read_line(out, number, s), ref)
    meta(lambda t: t.replace("celldata=1", "celldata=0"))
    open(base + "celldata", "wb").close()
    with pytest.raises(AssertionError, match="no cell-data container"):
        fd.compare_line(fd.read_line(out, number, s), ref)
    meta(lambda t: t.replace("threw=0", "threw=1"))
    with pytest.raises(AssertionError, match="threw"):
        fd.compare_line(fd.read_line(out, number, s), ref)
    # a refusal: its own words pass; accepted, or refused in other words, fails; so does an accessor that is not empty
    number = next(n for n, r in enumerate(refs) if r["threw"])
    line, ref = lines[number], refs[number]
    s, base = line["settings"], os.path.join(out, "%d." % number)
    fresh()
    fd.compare_line(fd.read_line(out, number, s), ref)
    meta(lambda t: t.replace(ref["fragment"], "another reason to refuse"))
    with pytest.raises(AssertionError, match="refused for another reason"):
        fd.compare_line(fd.read_line(out, number, s), ref)
    meta(lambda t: t.replace("threw=1", "threw=0"))
    with pytest.raises(AssertionError, match="was accepted"):
        fd.compare_line(fd.read_line(out, number, s), ref)
    fresh()
    np.zeros(3, np.float32).tofile(base + "normals")
    with pytest.raises(AssertionError, match="normals"):
        fd.compare_line(fd.read_line(out, number, s), ref)
