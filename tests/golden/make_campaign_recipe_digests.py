#!/usr/bin/env python3
"""Regenerate tests/golden/campaign_recipe_digests.json: what tests/fuzz_campaign.py's draw_case drew BEFORE cell pixels,
components and the emit offset entered the recipe -- to be run on a checkout of that commit (61de589), never on a later one:

    python tests/golden/make_campaign_recipe_digests.py --tests /path/to/parent/checkout/tests

  keys     the keys a recipe of that commit can hold (the union over every recipe digested)
  seeds    for seeds 1 and 11, cases 0 .. 299, default options: sha256 of json.dumps(recipe, sort_keys=True)
  slices   the same for the five slice_recipes(kind) lists

The seeds of the slice were chosen for what they produce, and the cases logged in profiles/fuzz_views_seed*.log and
profiles/r5_fuzz_campaign_*.log replay from --seed S --case N: tests/test_campaign_scripts.py recomputes every digest from the
draw_case of the day, restricted to `keys`, and requires equality -- a new key is drawn from a stream of its own.
--out names the fixture: campaign_celldata_recipe_digests.json is the same record taken on the commit before the keep entered the
recipe (070778d) -- it holds the keys of the second stream too (cell_pixels, components, drop_cell_rows, emit_offset,
refusal_slab), which the keep's third stream must not move.
--dropin writes campaign_dropin_recipe_digests.json instead, on the checkout of the day: the recipes of tests/fuzz_dropin.py
-- fuzz_campaign's with the `dropin` entry from a stream of its own, np.random.default_rng([seed, case, 6]) -- for the same seeds
and cases and the five slice_recipes(kind) lists of fuzz_dropin, each digested whole and as its `dropin` entry alone.
--envelope writes campaign_envelope_recipe_digests.json, on the checkout of the day: the recipes draw_case draws with the
option `envelope` on -- their `envelope` entry from np.random.default_rng([seed, case, 7]) -- for the same seeds and cases and
fuzz_campaign.envelope_slice_recipes(), digested in blocks of 25 cases, whole and as their `envelope` entries alone.
Needs no GPU and no oracle."""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = (1, 11)
CASES = 300
ENVELOPE_BLOCK = 25


def digest(recipe, keys=None):
    """sha256 of the recipe's JSON with sorted keys; keys: the top-level keys that count (None: all)."""
    if keys is not None:
        recipe = {k: v for k, v in recipe.items() if k in keys}
    return hashlib.sha256(json.dumps(recipe, sort_keys=True).encode()).hexdigest()


def collect(fz, keys=None):
    """(seeds, slices, recipes): the digests in the fixture's layout, and every recipe they were taken from."""
    by_seed = {str(s): [fz.draw_case(s, c) for c in range(CASES)] for s in SEEDS}
    by_kind = {kind: fz.slice_recipes(kind) for kind in fz.KINDS}
    recipes = [r for rs in list(by_seed.values()) + list(by_kind.values()) for r in rs]
    return ({s: [digest(r, keys) for r in rs] for s, rs in by_seed.items()},
            {k: [digest(r, keys) for r in rs] for k, rs in by_kind.items()}, recipes)


def collect_dropin(fd):
    """The fixture of the drop-in campaign's stream: per seed and per slice, (digest of the recipe, digest of its dropin entry)."""
    by_seed = {str(s): [fd.draw_case(s, c) for c in range(CASES)] for s in SEEDS}
    by_kind = {kind: fd.slice_recipes(kind) for kind in fd.fz.KINDS}
    both = lambda rs: [[digest(r), digest(r["dropin"])] for r in rs]                                 # noqa: E731
    return dict(cases=CASES, seeds={s: both(rs) for s, rs in by_seed.items()}, slices={k: both(rs) for k, rs in by_kind.items()},
                slice_seeds=dict(fd.SLICE), dropin_keys=sorted({k for rs in by_seed.values() for r in rs for k in r["dropin"]}))


def collect_envelope(fz):
    """The fixture of the envelope's stream: per seed and for the slice, (digest of the recipe, digest of its envelope entry)."""
    by_seed = {str(s): [fz.draw_case(s, c, dict(envelope=True)) for c in range(CASES)] for s in SEEDS}
    # (one digest per block of ENVELOPE_BLOCK cases, of the recipes and of their envelope entries: a moved draw names its block)
    blocks = lambda rs: [rs[i:i + ENVELOPE_BLOCK] for i in range(0, len(rs), ENVELOPE_BLOCK)]        # noqa: E731
    both = lambda rs: [[digest(b), digest([r["envelope"] for r in b])] for b in blocks(rs)]         # noqa: E731
    return dict(cases=CASES, seeds={s: both(rs) for s, rs in by_seed.items()}, slice=both(fz.envelope_slice_recipes()),
                slice_seed=list(fz.ENVELOPE_SLICE), envelope_keys=sorted({k for rs in by_seed.values() for r in rs for k in r["envelope"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envelope", action="store_true", help="write campaign_envelope_recipe_digests.json from draw_case(envelope=True)")
    ap.add_argument("--dropin", action="store_true", help="write campaign_dropin_recipe_digests.json from tests/fuzz_dropin.py")
    ap.add_argument("--tests", default=os.path.dirname(HERE), help="the tests/ directory of the checkout whose draw_case is recorded")
    ap.add_argument("--out", default="campaign_recipe_digests.json", help="the fixture's file name in tests/golden/")
    args = ap.parse_args()
    tests = os.path.abspath(args.tests)
    sys.path.insert(0, os.path.dirname(tests))
    sys.path.insert(0, tests)
    import fuzz_campaign as fz
    assert os.path.dirname(os.path.abspath(fz.__file__)) == tests, fz.__file__
    if args.envelope:
        with open(os.path.join(HERE, "campaign_envelope_recipe_digests.json"), "w") as f:
            json.dump(collect_envelope(fz), f)
            f.write("\n")
        return
    if args.dropin:
        import fuzz_dropin as fd
        with open(os.path.join(HERE, "campaign_dropin_recipe_digests.json"), "w") as f:
            json.dump(collect_dropin(fd), f, indent=1)
            f.write("\n")
        return
    seeds, slices, recipes = collect(fz)
    keys = sorted({k for r in recipes for k in r})
    with open(os.path.join(HERE, os.path.basename(args.out)), "w") as f:
        json.dump(dict(keys=keys, cases=CASES, seeds=seeds, slices=slices), f, indent=1)
        f.write("\n")
    print(len(keys), "keys,", len(recipes), "recipes")


if __name__ == "__main__":
    main()
