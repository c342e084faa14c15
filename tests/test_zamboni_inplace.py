"""Zamboni's in-place scour (mt_paged.h pg_scour_inplace): the segment zamboni pops usually lies
on a page other than the one staged in LDS; tiers without a delta log and with their page
metadata in LDS scour its leaf block on the page's rows in HBM instead of moving the window
there.  Every output must stay what the window path computes (the reference's, the C
restatement's), and mt_last_zamboni must show that the path -- and its fallback to the window
path -- was actually taken, so that no test passes with the path never reached."""
import json
import os

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS, OPS = 32, 1500   # ~600 live segments, ~25 pages per document at the end


def _c3(ops):
    return dict(json.load(open(os.path.join(REPO, "bench", "configs.json")))["c3"], ops=ops)


def _c4(ops):
    return dict(json.load(open(os.path.join(REPO, "bench", "configs.json")))["c4"], ops=ops)


def _bench_c3_caps():
    """The bench's C3 capacities (they select P_C3) behind a 16-segment LDS tier: documents go
    paged within their first messages."""
    import bench
    caps = dict(bench.capacities(_c3(10000)), lds_seg_capacity=16)
    assert (caps["lds_page_capacity"], caps["lds_unsettled_capacity"], caps["lds_page_heap_capacity"]) == (192, 220, 192)
    return caps


def _bench_c4_caps():
    import bench
    caps = dict(bench.capacities(_c4(10000)), lds_seg_capacity=16)
    assert (caps["lds_page_capacity"], caps["lds_unsettled_capacity"], caps["lds_page_heap_capacity"]) == (224, 1900, 900)
    return caps


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
FLAT = dict(seg_capacity=8192, text_capacity=1 << 17)   # (what the parity tests give the flat arrays)


def _tier_caps(tier):
    if tier == "bench_c3":
        return _bench_c3_caps()
    if tier == "bench_c4":
        return _bench_c4_caps()
    return dict(FLAT, **PARITY[tier])


@pytest.fixture(scope="module")
def stream(oracle_lib):
    """32 documents x 1500 messages of the C3 configuration, generated on the device once; the
    C restatement's checksums of their replay from the seeds (shared, never modified)."""
    from fluidframework_amd import MergeTreeBatch
    cfg = _c3(OPS)
    mt = MergeTreeBatch(DOCS, delta_log_capacity=0, **_bench_c3_caps())
    batch = mt.generate(cfg)
    host = batch.download()
    gen_z = mt.last_zamboni()
    seed_off, seed = mt.generated_seeds(cfg)
    a = dict(host, seed_off=seed_off, seed=seed)
    osums, ost = oracle_lib.replay_batch(a, threads=4)
    assert (ost == 0).all()
    assert np.array_equal(mt.checksums(), osums), "the generated state differs from the oracle's replay"
    for v in a.values():
        v.setflags(write=False)
    return dict(a=a, osums=osums, gen_z=gen_z)


def _replay(stream, **caps):
    from fluidframework_amd import MergeTreeBatch
    a = stream["a"]
    mt = MergeTreeBatch(DOCS, **caps)
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    return mt


def test_generator_takes_the_path(stream):
    """The paged generator applies its messages through the same driver."""
    assert stream["gen_z"]["in_place"] > 0 and stream["gen_z"]["fallback"] > 0, stream["gen_z"]


@pytest.mark.parametrize("tier", ["bench_c3", "bench_c4", "paged", "tight", "narrow", "grow"])
def test_generated_stream_every_eligible_tier(stream, tier):
    """Every tier that compiles the path in (P_C3, P_C4 / packed, full, tight, narrow, and the
    growth step's big region) replays the stream to the oracle's checksums, scouring both in
    place and -- where a pack, the serial plan or a compaction is needed -- through the window."""
    mt = _replay(stream, delta_log_capacity=0, **_tier_caps(tier))
    assert (mt.status() == 0).all(), mt.status()
    assert np.array_equal(mt.checksums(), stream["osums"])
    z = mt.last_zamboni()
    print(tier, z, mt.last_paged_peaks())
    assert z["in_place"] > 0 and z["fallback"] > 0, z


@pytest.mark.parametrize("name", ["ref_ext", "ref_c3", "ref_combine"])
def test_reference_fixtures_markers_newlines_props(oracle_lib, name):
    """Streams made by the reference with markers, newlines, insert properties and combining
    annotates, at the bench's C3 capacities without a delta log: text, leaf partition, segment
    rows and property sets equal the reference's, the checksums the C restatement's."""
    from fluidframework_amd import MergeTreeBatch
    fx = gu.load(name)
    interner = gu.interner_for(fx)
    a = gu.encode_docs(fx, interner)
    mt = MergeTreeBatch(len(fx["docs"]), delta_log_capacity=0, **_bench_c3_caps())
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
    assert z["in_place"] > 0, z


@pytest.mark.parametrize("tier", ["delta_log", "hm"])
def test_ineligible_tiers_stay_on_the_window_path(stream, tier):
    """A handle with a delta log, and one at a 200k-message size class's capacities (page
    metadata in HBM), never scour in place; their outputs equal the oracle's all the same."""
    if tier == "delta_log":
        caps = dict(_bench_c3_caps(), delta_log_capacity=1 << 16)
    else:
        import bench
        import bench_skew
        caps = dict(bench_skew.class_caps(bench, _c3(10000), 200000), lds_seg_capacity=16, delta_log_capacity=0)
        assert caps["page_capacity"] >= 512
    mt = _replay(stream, **caps)
    assert (mt.status() == 0).all(), mt.status()
    assert np.array_equal(mt.checksums(), stream["osums"])
    assert mt.last_zamboni()["in_place"] == 0, mt.last_zamboni()


def test_arena_room_fallback(stream):
    """A 4096-unit text arena: merges regularly find it full, so the scour goes through the
    window path (whose text_ensure compacts; the growth step raises the arena as documents
    outgrow it) -- decided before anything of the in-place attempt is stored.  The other two
    fallbacks (serial plan, pack) are decided from the rows, not from the arena's fill, so the
    same stream at the bench's own arena gives their count (8848 of 27535 scours when this was
    written); the small arena must add to it (8864)."""
    base = _replay(stream, delta_log_capacity=0, **_bench_c3_caps()).last_zamboni()
    mt = _replay(stream, delta_log_capacity=0, **dict(_bench_c3_caps(), text_capacity=4096))
    assert (mt.status() == 0).all(), mt.status()
    assert np.array_equal(mt.checksums(), stream["osums"])
    z = mt.last_zamboni()
    print(base, z, mt.last_grown())
    assert z["fallback"] > base["fallback"] > 0 and z["in_place"] > 0, (base, z)
