"""Zamboni's scour, merge and pack off the C3 distribution: the reference-made streams of
tests/zam_streams.py (rows over MT_GRAN and over one wave of text, streams that settle at once,
markers and trailing newlines on pages, a document that empties and regrows, hand-built combs
whose far pages are scoured block by block) on every tier that compiles the in-place routes in
(mt_paged.h pg_scour_inplace / pg_pack_inplace).  Correctness is the reference's: text, length,
leaf partition, segment rows, property sets, status; checksums are the C restatement's; the
window route (a delta-log handle) must give the same rows.  `last_zamboni()` shows which route
ran, so that no case passes with its route never reached; its values are printed by every test.

Route readings that the code implies and the counters confirmed on an MI355X (trigger batches
of the comb cases at the bench's C3 capacities; see _COMB_ROUTES, which also says where the
counters corrected a first reading) are asserted; they are conditions that a route was
reached, not correctness numbers."""
import json
import os

import numpy as np
import pytest

import golden_util as gu
import zam_streams as zs

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_caps(name):
    """The bench's capacities for C3 (P_C3) or C4 (P_C4) behind a 16-segment LDS tier."""
    import bench
    cfg = dict(json.load(open(os.path.join(REPO, "bench", "configs.json")))[name], ops=10000)
    return dict(bench.capacities(cfg), lds_seg_capacity=16)


# the paged capacity sets of tests/test_zamboni_inplace_pack.py, with no delta log here
PARITY = {
    "paged": dict(lds_seg_capacity=-1, page_capacity=256, unsettled_capacity=2048, page_heap_capacity=2048),
    "tight": dict(lds_seg_capacity=16, page_capacity=256, unsettled_capacity=2048, page_heap_capacity=2048,
                  lds_page_capacity=24, lds_unsettled_capacity=40, lds_page_heap_capacity=40),
    "narrow": dict(lds_seg_capacity=16, page_capacity=256, unsettled_capacity=2048, page_heap_capacity=2048,
                   lds_page_capacity=200, lds_unsettled_capacity=600, lds_page_heap_capacity=600,
                   lds_narrow_overlap=1),
    "grow": dict(lds_seg_capacity=16, page_capacity=12, unsettled_capacity=16, page_heap_capacity=16),
}
FLAT = dict(seg_capacity=8192, text_capacity=1 << 17)
# paged_text1k: a 1024-unit text arena.  pg_arena_room keeps at least 4096 units free, so an
# arena this small is handed to the growth step at the documents' first messages until it has
# been doubled past 8192 units; from there the giant keepers of the comb's `short` and `mid`
# cases (3.4k and 24k units, moved whole by a merge) go through compaction inside and between
# messages and further doublings
TIER_NAMES = ["bench_c3", "bench_c4", "paged", "tight", "narrow", "grow", "paged_text1k"]


def _tier_caps(tier):
    if tier == "bench_c3":
        return _bench_caps("c3")
    if tier == "bench_c4":
        return _bench_caps("c4")
    if tier == "paged_text1k":
        return dict(FLAT, **PARITY["paged"], text_capacity=1024)
    return dict(FLAT, **PARITY[tier])


@pytest.fixture(scope="module")
def prepared(oracle_lib):
    """name -> a fixture encoded once: arrays, the reference's outputs in id space, the C
    restatement's checksums and statuses (shared by the module's tests, never modified)."""
    cache = {}

    def get(name):
        if name not in cache:
            fx = gu.load(name)
            interner = gu.interner_for(fx)
            a = gu.encode_docs(fx, interner)
            osums, ost = oracle_lib.replay_batch(a, threads=4)
            for v in a.values():
                v.setflags(write=False)
            cache[name] = dict(fx=fx, interner=interner, a=a, osums=osums, ost=ost,
                               exp=[gu.expected(d, interner) for d in fx["docs"]])
        return cache[name]

    yield get
    cache.clear()


def _outputs(mt, i, log):
    rows, leaves = mt.get_segments(i)
    return dict(text=mt.get_text(i), length=mt.get_length(i), leaves=leaves, segs=rows,
                seg_props=mt.get_all_segment_props(i), deltas=mt.get_delta_log(i) if log else None,
                status=int(mt.status()[i]))


def _mismatches(mt, docs, exps, log=False):
    bad = []
    for i, (doc, exp) in enumerate(zip(docs, exps)):
        errs = gu.compare_oracle(_outputs(mt, i, log), exp if log else dict(exp, deltas=None))
        if errs:
            bad.append((doc["doc"], errs))
    return bad


def _replay(p, **caps):
    from fluidframework_amd import MergeTreeBatch
    a = p["a"]
    mt = MergeTreeBatch(len(p["fx"]["docs"]), **caps)
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    return mt


@pytest.fixture(scope="module")
def bench_c3(prepared):
    """name -> the fixture replayed at the bench's C3 capacities without a delta log (shared by
    the module's tests, read only; the handles are released with the module)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _replay(prepared(name), delta_log_capacity=0, **_bench_caps("c3"))
        return cache[name]

    yield get
    cache.clear()


def _fallback_share(z):
    return z["fallback"] / max(z["in_place"] + z["fallback"], 1)


# ---------------------------------------------------------------- a. every fixture, every eligible tier
@pytest.mark.parametrize("tier", TIER_NAMES)
@pytest.mark.parametrize("name", gu.ZAM_FIXTURES)
def test_every_eligible_tier_matches_reference(prepared, bench_c3, name, tier):
    """No delta log: every document equals the reference (text, length, leaf partition, segment
    rows, property sets, status) and its checksums the C restatement's."""
    p = prepared(name)
    assert (p["ost"] == 0).all()
    mt = bench_c3(name) if tier == "bench_c3" else _replay(p, delta_log_capacity=0, **_tier_caps(tier))
    z = mt.last_zamboni()
    print(name, tier, z, mt.last_grown())
    assert np.array_equal(mt.status(), p["ost"]), mt.status()
    bad = _mismatches(mt, p["fx"]["docs"], p["exp"])
    assert not bad, bad[:4]
    assert np.array_equal(mt.checksums(), p["osums"])
    assert z["in_place_packs"] <= z["in_place"], z
    if name != "ref_zam_comb":
        assert z["in_place"] > 0, z


def test_random_streams_reach_the_routes(bench_c3):
    """At the bench's C3 capacities: all four generated fixtures scour in place; the streams that
    settle at once and the document that empties also repack pages in place; ref_zam_long, whose
    join candidates are regularly over MT_GRAN (the serial plan decides), falls back to the
    window for a larger share of its scours than ref_c3 does."""
    z = {name: bench_c3(name).last_zamboni()
         for name in ["ref_zam_long", "ref_zam_settle", "ref_zam_marks", "ref_zam_shrink", "ref_c3"]}
    print("routes", z, {k: round(_fallback_share(v), 4) for k, v in z.items()})
    for name in gu.ZAM_FIXTURES[:4]:
        assert z[name]["in_place"] > 0, (name, z[name])
    assert z["ref_zam_settle"]["in_place_packs"] > 0 and z["ref_zam_shrink"]["in_place_packs"] > 0, z
    assert _fallback_share(z["ref_zam_long"]) > _fallback_share(z["ref_c3"]), z


@pytest.mark.parametrize("name", gu.ZAM_FIXTURES)
def test_equals_the_window_route(prepared, bench_c3, name):
    """A handle with a delta log stays on the window route (scour_range, pack, pg_win_sync, the
    window's flush): segment rows, leaf partition and text of every document are equal on both
    routes, and the window route's delta records are the reference's."""
    p = prepared(name)
    win = _replay(p, **dict(_bench_caps("c3"), delta_log_capacity=1 << 18))
    inp = bench_c3(name)
    assert (win.status() == 0).all() and (inp.status() == 0).all()
    assert win.last_zamboni()["in_place"] == 0, win.last_zamboni()
    bad = []
    for i in range(len(p["fx"]["docs"])):
        rows_w, leaves_w = win.get_segments(i)
        rows_p, leaves_p = inp.get_segments(i)
        if leaves_w != leaves_p:
            bad.append((i, "leaves"))
        elif not np.array_equal(rows_w, rows_p):
            bad.append((i, "rows"))
        elif win.get_text(i) != inp.get_text(i):
            bad.append((i, "text"))
    assert not bad, bad
    bad = _mismatches(win, p["fx"]["docs"], p["exp"], log=True)
    assert not bad, bad[:4]


# ---------------------------------------------------------------- c, d. the comb at its checkpoints
# What the trigger batches (the four after the prefix) of each comb case show at the bench's C3
# capacities.  The counters count zamboni's scours outside the window only (in place, or through
# the window after all); a scour in the window's own page counts nowhere, and `fallback` lumps
# every reason together (serial plan, nb > 8, p2.big, arena room, the pg_pack1 exit): which exit
# a fallback took cannot be told without per-reason counters, which the kernels do not have.
#   window: every counted scour goes through the window, none is done in place.  For `long` and
#     `rmlong` the code gives the reason: every far block's plan has a join candidate over
#     MT_GRAN (ScourPlan.big), and pg_scour_inplace returns before anything else.  For `short`,
#     `mid` and `rm` the likely exits are the pg_pack1 one (each far scour leaves one row in its
#     block and few on its page) and, once the keeper has passed MT_GRAN, p2.big; the test shows
#     only that the in-place pack never completed;
#   mixed: both routes occur.
# The first reading was "at least 100" counted scours on every case.  An MI355X gave fewer
# (trigger batches, in_place / fallback / in_place_packs): short 0/39/0, mid 0/39/0, long
# 0/77/0, nl 31/51/5, mark 36/44/16, props2 8/37/8, rm 0/46/0, rmlong 0/73/0.  A fallback moves
# the window to the far page, whose other blocks are then scoured as the window's own and
# counted nowhere; in `short`, `mid` and `rm` the tree also collapses into the window's page
# within the first 100 trigger messages (all 39 / 39 / 46 fall there).  So the count is not
# asserted, the route of the counted scours is.
_COMB_ROUTES = {"long": "window", "rmlong": "window", "short": "window", "mid": "window", "rm": "window",
                "nl": "mixed", "mark": "mixed", "props2": "mixed"}
_COMB_HANDLES = {
    "bench_c3": lambda: dict(_bench_caps("c3"), delta_log_capacity=0),
    "paged_log": lambda: dict(FLAT, **PARITY["paged"], delta_log_capacity=1 << 16),
}


@pytest.mark.parametrize("handle", list(_COMB_HANDLES))
@pytest.mark.parametrize("case", list(zs.COMB_CASES))
def test_comb_checkpoints(case, handle):
    """One comb case applied in batches that end at its checkpoints (after the prefix, after
    every 100 trigger messages), on a handle of its own: every checkpoint equals the reference's
    replay of the truncated log (with the delta log: its records too), so a state that is wrong
    in the middle and healed later does not pass; `last_zamboni()`, cleared when a batch starts
    (mt_batch_apply_async), is read after every batch and summed over the trigger batches.
    Route evidence at the bench's C3 capacities (_COMB_ROUTES): the expectation of at least 100
    counted scours per case was corrected after the counters gave 39-82 (a scour in the
    window's own page is not counted); asserted instead: `long`, `rmlong`, `short`, `mid`, `rm`
    send every counted scour through the window, `nl`, `mark`, `props2` take both routes."""
    from fluidframework_amd import MergeTreeBatch
    fx = gu.load("ref_zam_comb")
    doc = next(d for d in fx["docs"] if d["doc"] == case)
    interner = gu.interner_for(fx)
    a = gu.encode_docs(fx, interner, [doc])
    cps = gu.checkpoints(doc)
    assert len(cps) == 1 + zs.COMB_TRIGGER // zs.COMB_STEP
    log = handle == "paged_log"
    mt = MergeTreeBatch(1, **_COMB_HANDLES[handle]())
    mt.load_initial_text(a["seed_off"], a["seed"])
    total = dict(in_place=0, fallback=0, in_place_packs=0)
    for j, ((n, out), part) in enumerate(zip(cps, gu.batches_to(a, [doc], [[n for n, _ in cps]]))):
        mt.apply_arrays(part)
        z = mt.last_zamboni()
        print(case, handle, "after", n, "messages", z)
        if j > 0:
            total = {k: total[k] + z[k] for k in total}
        bad = _mismatches(mt, [doc], [gu.expected(dict(doc, out=out), interner)], log=log)
        assert not bad, (n, bad)
    print(case, handle, "trigger batches", total)
    if log:
        assert total["in_place"] == 0, total
        return
    route = _COMB_ROUTES[case]
    if route == "window":
        assert total["fallback"] > 0 and total["in_place"] == 0 and total["in_place_packs"] == 0, total
    else:
        assert total["in_place"] > 0 and total["fallback"] > 0, total
