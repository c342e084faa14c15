"""Zamboni's in-place pack (mt_paged.h pg_pack_inplace): a scour that leaves its leaf block under
four segments makes `pack` regroup the page's leaf blocks; on the tiers that scour in place
(no delta log, page metadata in LDS) both scours and the regrouping now run on the page's rows
in registers and go straight to the page in HBM.  Every output must stay what the window route
computes -- rows, leaf partition, text, checksums -- and `last_zamboni()["in_place_packs"]`
must show that the route was taken, so that no test passes with it never reached."""
import json
import os

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS, OPS = 32, 1500   # ~600 live segments, ~25 pages per document at the end (up.depth > 2)


def _cfg(name, ops):
    return dict(json.load(open(os.path.join(REPO, "bench", "configs.json")))[name], ops=ops)


def _bench_caps(name):
    """The bench's capacities for C3 (P_C3) or C4 (P_C4) behind a 16-segment LDS tier: documents
    go paged within their first messages."""
    import bench
    return dict(bench.capacities(_cfg(name, 10000)), lds_seg_capacity=16)


# the paged capacity sets of tests/test_gpu_parity.py (TIERS), with no delta log here
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


def _tier_caps(tier):
    if tier == "bench_c3":
        return _bench_caps("c3")
    if tier == "bench_c4":
        return _bench_caps("c4")
    return dict(FLAT, **PARITY[tier])


@pytest.fixture(scope="module")
def stream(oracle_lib):
    """32 documents x 1500 messages of the C3 configuration, generated on the device once; the
    C restatement's checksums of their replay from the seeds (shared, never modified)."""
    from fluidframework_amd import MergeTreeBatch
    cfg = _cfg("c3", OPS)
    mt = MergeTreeBatch(DOCS, delta_log_capacity=0, **_bench_caps("c3"))
    host = mt.generate(cfg).download()
    seed_off, seed = mt.generated_seeds(cfg)
    a = dict(host, seed_off=seed_off, seed=seed)
    osums, ost = oracle_lib.replay_batch(a, threads=4)
    assert (ost == 0).all()
    for v in a.values():
        v.setflags(write=False)
    return dict(a=a, osums=osums)


def _replay(stream, **caps):
    from fluidframework_amd import MergeTreeBatch
    a = stream["a"]
    mt = MergeTreeBatch(DOCS, **caps)
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    return mt


@pytest.fixture(scope="module")
def bench_c3(stream):
    """The stream replayed at the bench's C3 capacities without a delta log (shared, read only)."""
    return _replay(stream, delta_log_capacity=0, **_bench_caps("c3"))


@pytest.mark.parametrize("tier", ["bench_c3", "bench_c4", "paged", "tight", "narrow", "grow"])
def test_generated_stream_every_eligible_tier(stream, tier):
    """Every tier that compiles the route in replays the stream to the oracle's checksums and
    repacks pages in place; `in_place_packs` counts a subset of `in_place`."""
    mt = _replay(stream, delta_log_capacity=0, **_tier_caps(tier))
    assert (mt.status() == 0).all(), mt.status()
    assert np.array_equal(mt.checksums(), stream["osums"])
    z = mt.last_zamboni()
    print(tier, z)
    assert 0 < z["in_place_packs"] <= z["in_place"], z


def test_equals_the_window_route(stream, bench_c3):
    """A handle with a delta log stays on the window route (scour_range, pack, pg_win_sync, the
    window's flush): segment rows, leaf partition -- exactly what a pack changes -- and text of
    all 32 documents are equal on both routes."""
    win = _replay(stream, **dict(_bench_caps("c3"), delta_log_capacity=1 << 16))
    assert (win.status() == 0).all() and (bench_c3.status() == 0).all()
    assert win.last_zamboni()["in_place"] == 0 and bench_c3.last_zamboni()["in_place_packs"] > 0
    bad = []
    for i in range(DOCS):
        rows_w, leaves_w = win.get_segments(i)
        rows_p, leaves_p = bench_c3.get_segments(i)
        if leaves_w != leaves_p:
            bad.append((i, "leaves"))
        elif not np.array_equal(rows_w, rows_p):
            bad.append((i, "rows"))
        elif win.get_text(i) != bench_c3.get_text(i):
            bad.append((i, "text"))
    assert not bad, bad


@pytest.mark.parametrize("name", ["ref_ext", "ref_c3", "ref_combine"])
def test_reference_fixtures(oracle_lib, name):
    """Streams made by the reference (markers, newlines, insert properties, combining annotates)
    at the bench's C3 capacities without a delta log: text, leaf partition, segment rows,
    property sets and status equal the reference's."""
    from fluidframework_amd import MergeTreeBatch
    fx = gu.load(name)
    interner = gu.interner_for(fx)
    a = gu.encode_docs(fx, interner)
    mt = MergeTreeBatch(len(fx["docs"]), delta_log_capacity=0, **_bench_caps("c3"))
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    osums, ost = oracle_lib.replay_batch(a, threads=2)
    assert np.array_equal(mt.status(), ost)
    assert np.array_equal(mt.checksums(), osums)
    bad = []
    for i, doc in enumerate(fx["docs"]):
        exp = dict(gu.expected(doc, interner), deltas=None)
        rows, leaves = mt.get_segments(i)
        got = dict(text=mt.get_text(i), length=mt.get_length(i), leaves=leaves, segs=rows,
                   seg_props=mt.get_all_segment_props(i), deltas=None, status=int(mt.status()[i]))
        errs = gu.compare_oracle(got, exp, status=int(ost[i]))
        if errs:
            bad.append((doc["doc"], errs))
    assert not bad, bad[:4]
    z = mt.last_zamboni()
    print(name, z)
    if name == "ref_c3":
        assert z["in_place_packs"] > 0, z


@pytest.mark.parametrize("tier", ["delta_log", "hm"])
def test_ineligible_handles_never_pack_in_place(stream, tier):
    """A handle with a delta log, and one at a 200k-message size class's capacities (page
    metadata in HBM), stay on the window route."""
    if tier == "delta_log":
        caps = dict(_bench_caps("c3"), delta_log_capacity=1 << 16)
    else:
        import bench
        import bench_skew
        caps = dict(bench_skew.class_caps(bench, _cfg("c3", 10000), 200000), lds_seg_capacity=16,
                    delta_log_capacity=0)
        assert caps["page_capacity"] >= 512
    mt = _replay(stream, **caps)
    assert (mt.status() == 0).all(), mt.status()
    assert np.array_equal(mt.checksums(), stream["osums"])
    assert mt.last_zamboni()["in_place_packs"] == 0, mt.last_zamboni()


def test_arena_room_fallback(stream, bench_c3):
    """A 4096-unit text arena: the merges of both scours together regularly do not fit without a
    compaction, which is decided before rows, metadata, arena text or counters are written; the
    window route (whose text_ensure compacts) runs instead, so `fallback` exceeds the count at
    the bench's own arena and the checksums stay the oracle's."""
    base = bench_c3.last_zamboni()
    mt = _replay(stream, delta_log_capacity=0, **dict(_bench_caps("c3"), text_capacity=4096))
    assert (mt.status() == 0).all(), mt.status()
    assert np.array_equal(mt.checksums(), stream["osums"])
    z = mt.last_zamboni()
    print(base, z)
    assert z["fallback"] > base["fallback"], (base, z)
