"""A remove or annotate whose two ends lie strictly inside one page's view span takes the
single-page path of pg_op_range (mt_paged.h): one page search, both boundary splits and the
marking pass on the staged page, one metadata sync.  Every other range message -- an end at a
page's view end, a range over several pages, a tier with a delta log or its page metadata in HBM
-- goes the general way, and a single-page message whose split gives the page its eighth leaf
block leaves the path for it.  The checksums carry the per-message delta hash, so a wrong page,
split or mark at any message fails a case; `last_range_paths()` shows which way messages went."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS, OPS = 32, 1500
TIERS = ["bench_c3", "bench_c4", "paged", "tight", "narrow", "grow", "hm", "delta_log"]
OP_REMOVE, OP_ANNOTATE = 1, 2


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


def _hm_caps():
    import bench
    import bench_skew
    caps = dict(bench_skew.class_caps(bench, _c3(10000), 200000), lds_seg_capacity=16)
    assert caps["page_capacity"] >= 512
    return caps


# the paged capacity sets of tests/test_gpu_parity.py (TIERS)
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
    """Capacities and delta-log size of a named handle."""
    if tier == "bench_c3":
        return dict(_bench_c3_caps(), delta_log_capacity=0)
    if tier == "bench_c4":
        return dict(_bench_c4_caps(), delta_log_capacity=0)
    if tier == "hm":
        return dict(_hm_caps(), delta_log_capacity=0)
    if tier == "delta_log":
        return dict(_bench_c3_caps(), delta_log_capacity=1 << 16)
    return dict(FLAT, delta_log_capacity=0, **PARITY[tier])


def _replay(s, **caps):
    from fluidframework_amd import MergeTreeBatch
    a = s["a"]
    mt = MergeTreeBatch(s["docs"], **caps)
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    return mt


def _range_messages(a):
    k = a["ops"]["kind"]
    return int(((k == OP_REMOVE) | (k == OP_ANNOTATE)).sum())


@pytest.fixture(scope="module")
def stream(oracle_lib):
    """32 documents x 1500 messages of the C3 configuration, generated on the device once; the
    C restatement's checksums of their replay from the seeds (shared, never modified)."""
    from fluidframework_amd import MergeTreeBatch
    cfg = _c3(OPS)
    mt = MergeTreeBatch(DOCS, delta_log_capacity=0, **_bench_c3_caps())
    batch = mt.generate(cfg)
    host = batch.download()
    seed_off, seed = mt.generated_seeds(cfg)
    a = dict(host, seed_off=seed_off, seed=seed)
    osums, ost = oracle_lib.replay_batch(a, threads=4)
    assert (ost == 0).all()
    assert np.array_equal(mt.checksums(), osums), "the generated state differs from the oracle's replay"
    for v in a.values():
        v.setflags(write=False)
    return dict(a=a, osums=osums, docs=DOCS, ranges=_range_messages(a))


@pytest.mark.parametrize("tier", TIERS)
def test_generated_stream_every_tier(stream, tier):
    """Every paged tier replays the stream to the oracle's checksums, twice: behind the 16-segment
    LDS tier of the tier table, where a document's first messages run flat before it is
    converted (118 of the batch's 23 983 removes and annotates), and paged from the load on
    (`lds_seg_capacity=-1`), where every remove and annotate of the batch reaches pg_op_range:
    there the three counters must account for all of them.  The tiers with page metadata in HBM
    or a delta log never take the single-page path."""
    for caps in (_tier_caps(tier), dict(_tier_caps(tier), lds_seg_capacity=-1)):
        mt = _replay(stream, **caps)
        assert (mt.status() == 0).all(), mt.status()
        assert np.array_equal(mt.checksums(), stream["osums"])
        paths = mt.last_range_paths()
        print(tier, "lds", caps["lds_seg_capacity"], paths, "range messages", stream["ranges"])
        if tier == "bench_c3":
            assert paths["one_page"] > 0 and paths["general"] > 0, paths
        if tier in ("hm", "delta_log"):
            assert paths["one_page"] == 0 and paths["split_fallback"] == 0, paths
        counted = paths["one_page"] + paths["split_fallback"] + paths["general"]
        if caps["lds_seg_capacity"] == -1:   # paged from the load on: every range message is counted
            assert counted == stream["ranges"], paths
        else:                                # behind the LDS tier: all but the few applied flat
            assert 0 < counted <= stream["ranges"], paths


# values of a build with -DMT_NO_RANGE1 (the general path for every range message) on the
# generated stream at the bench's C3 capacities
NO_RANGE1_ZAMBONI = {"in_place": 25644, "fallback": 1821, "in_place_packs": 6969}
NO_RANGE1_PEAKS = {"pages": 30, "unsettled": 123, "heap": 70, "segments": 677, "tight_handovers": 0}


def test_same_scours_and_peaks_as_general_path(stream):
    """The single-page path leaves every page, heap and table as the general path does: zamboni
    takes the same routes (`last_zamboni()`) and the high-water marks are the same
    (`last_paged_peaks()`) as in a build without the path."""
    mt = _replay(stream, **_tier_caps("bench_c3"))
    assert (mt.status() == 0).all(), mt.status()
    z, peaks = mt.last_zamboni(), mt.last_paged_peaks()
    print("zamboni", z, "peaks", peaks)
    assert z == NO_RANGE1_ZAMBONI
    assert peaks == NO_RANGE1_PEAKS


# ---------------------------------------------------------------- documents built by hand
class _Doc:
    """Messages of one document; sequence numbers count up from 1."""

    def __init__(self):
        self.msgs = []

    @property
    def seq(self):
        return len(self.msgs)

    def send(self, client, op, ref=None, msn=0):
        seq = self.seq + 1
        self.msgs.append(dict(clientId=f"client-{client}", sequenceNumber=seq,
                              referenceSequenceNumber=seq - 1 if ref is None else ref,
                              minimumSequenceNumber=msn, type="op", contents=op))


def _ins(pos, text, props=None):
    return {"type": 0, "pos1": pos, "seg": {"text": text, "props": props} if props else text}


def _rem(p1, p2):
    return {"type": 1, "pos1": p1, "pos2": p2}


def _ann(p1, p2, props):
    return {"type": 2, "pos1": p1, "pos2": p2, "props": props}


SPANS = (1, 2, 3, 5)
SEED = "seed"


def _text(d, segs):
    """`segs` three-unit segments appended behind the seed, each with a property set of its own;
    the minimum sequence number stays 0 throughout, so nothing merges or settles.  Returns the
    text's length."""
    for i in range(segs):
        d.send(1, _ins(len(SEED) + 3 * i, "abc", {"k1": i}))
    return len(SEED) + 3 * segs


def _annotate_sweep():
    """(a) 48 three-unit segments (148 units with the seed, several pages once the sweep has cut
    them), then annotates (p, p + m) at every p of the text for m in 1, 2, 3, 5: every alignment
    of p1 and p2 against segment and page edges -- p1 at a page's first unit, p2 at a page's view
    end (the general path), both cuts inside one segment, ranges over two pages.  Ranges over
    three pages are not reached here -- a page holds at least 16 one-unit segments, so five units
    never span one -- and are covered only by (b), whose pages of view length 0 lie inside its
    ranges.  The m = 1 sweep cuts every segment in three, so pages split during it and
    single-page messages leave the path for those splits (test_annotate_sweep_takes_every_path
    asserts it on this document alone); the text did not have to be lengthened for
    `split_fallback` to count."""
    d = _Doc()
    n = _text(d, 48)
    for m in SPANS:
        for p in range(0, n - m + 1):
            d.send(1, _ann(p, p + m, {"k2": m}))
    return SEED, d.msgs


def _remove_sweep():
    """(b) The sweep with removes, issued by two writers in turn.  Writer 2 stays at the reference
    sequence number of the finished text, so it sees none of writer 1's removes: its ranges
    overlap them (overlapping removes), and in writer 1's view whole runs of rows -- pages, in
    the end -- have length 0 at the cuts.  Each writer's positions are those of its own view: a
    remove takes (p, p + m) there and the sweep moves on one unit past it, for m in 1, 2, 3, 5 in
    turn over 132 three-unit segments, until the writer's view is used up."""
    d = _Doc()
    n = _text(d, 132)
    r0 = d.seq
    gone = [set() for _ in range(n)]   # writers that removed each unit of the finished text

    def view(w):   # units writer w sees: 2 sees only its own removes, 1 sees all
        return [u for u in range(n) if not (gone[u] if w == 1 else 2 in gone[u])]

    p = {1: 0, 2: 1}
    k = 0
    while True:
        w = 1 + k % 2
        m = SPANS[(k // 2) % len(SPANS)]
        v = view(w)
        if p[w] + m > len(v) or k >= 400:
            break
        if w == 1:
            d.send(1, _rem(p[w], p[w] + m))
        else:
            d.send(2, _rem(p[w], p[w] + m), ref=r0)
        for u in v[p[w]:p[w] + m]:
            gone[u].add(w)
        p[w] += 1
        k += 1
    return SEED, d.msgs


def _inverted_ranges():
    """(d) Ranges nobody validates: pos2 below pos1, and pos2 == pos1.  The reference (and the
    general path) splits at pos1, then at pos2 wherever that lies -- in an earlier page, when a
    page edge is between them -- and marks nothing; at pos1 == pos2 on a page's first unit it
    touches nothing at all.  None of these may take the single-page path, whose one search
    stands for three only when start <= pos1 < pos2 < the page's view end.  64 three-unit
    segments (several pages), then at every p of the text an empty range (p, p) and the
    inverted ranges (p, p - 1), (p, p - 3) and (p, p - 7), as annotates and removes in turn,
    the last by a second writer that stays at the finished text's sequence number: every
    alignment of both ends against segment and page edges, across a page edge and inside one
    page.  Proper ranges (p, p + 2) follow every eighth p, so single-page messages run on pages
    the inverted ones have just cut."""
    d = _Doc()
    n = _text(d, 64)
    r0 = d.seq
    for p in range(0, n + 1):
        d.send(1, _ann(p, p, {"k3": 0}) if p % 2 else _rem(p, p))
        if p >= 1:
            d.send(1, _rem(p, p - 1) if p % 2 else _ann(p, p - 1, {"k3": 1}))
        if p >= 3:
            d.send(1, _ann(p, p - 3, {"k3": 3}) if p % 2 else _rem(p, p - 3))
        if p >= 7:   # (inverted removes take nothing away: writer 2's view stays the finished text)
            d.send(2, _rem(p, p - 7) if p % 2 else _ann(p, p - 7, {"k3": 7}), ref=r0)
        if p % 8 == 0 and p + 2 <= n:
            d.send(1, _ann(p, p + 2, {"k3": 2}))
    return SEED, d.msgs


HAND = [_annotate_sweep, _remove_sweep]


def _hand_batch(oracle_lib, builders):
    from fluidframework_amd.wire import Batch, Interner
    b = Batch(Interner(synthetic=True))
    for f in builders:
        seed, msgs = f()
        b.add_doc(seed, msgs)
    a = b.arrays()
    osums, ost = oracle_lib.replay_batch(a, threads=2)
    assert (ost == 0).all(), ost
    for v in a.values():
        v.setflags(write=False)
    return dict(a=a, osums=osums, docs=len(builders), ranges=_range_messages(a))


@pytest.fixture(scope="module")
def hand(oracle_lib):
    """The hand-built documents as one batch, checked on the CPU first: the oracle replays every
    one with status 0 (every position lies inside its writer's view)."""
    return _hand_batch(oracle_lib, HAND)


@pytest.fixture(scope="module")
def hand_annotate(oracle_lib):
    return _hand_batch(oracle_lib, [_annotate_sweep])


@pytest.mark.parametrize("tier", ["bench_c3", "paged", "narrow"])
def test_hand_built_sweeps(hand, tier):
    """(a) the annotate sweep and (b) the remove sweep of two writers: all three ways are taken,
    and the counters account for every range message."""
    mt = _replay(hand, **_tier_caps(tier))
    assert (mt.status() == 0).all(), mt.status()
    paths = mt.last_range_paths()
    print(tier, paths, mt.last_paged_peaks())
    assert all(mt.is_paged(d) for d in range(hand["docs"]))
    assert np.array_equal(mt.checksums(), hand["osums"])
    assert paths["one_page"] > 0 and paths["split_fallback"] > 0 and paths["general"] > 0, paths


@pytest.mark.parametrize("tier", ["bench_c3", "paged", "narrow"])
def test_annotate_sweep_takes_every_path(hand_annotate, tier):
    """Sweep (a) alone takes all three ways: the single-page path, out of it for a page split,
    and the general path (p2 at a page's view end, ranges over two pages)."""
    mt = _replay(hand_annotate, **_tier_caps(tier))
    assert (mt.status() == 0).all(), mt.status()
    paths = mt.last_range_paths()
    print(tier, paths, mt.last_paged_peaks())
    assert np.array_equal(mt.checksums(), hand_annotate["osums"])
    assert paths["one_page"] > 0 and paths["split_fallback"] > 0 and paths["general"] > 0, paths
    assert paths["one_page"] + paths["split_fallback"] + paths["general"] == hand_annotate["ranges"], paths


@pytest.fixture(scope="module")
def hand_inverted(oracle_lib):
    return _hand_batch(oracle_lib, [_inverted_ranges])


@pytest.mark.parametrize("tier", ["bench_c3", "paged", "narrow"])
def test_inverted_and_empty_ranges(hand_inverted, tier):
    """(d) pos2 <= pos1: the oracle's checksums (its splits at both ends, its ids, every later
    delta hash), and none of those messages on the single-page path -- only the proper ranges
    among them can take it."""
    mt = _replay(hand_inverted, **_tier_caps(tier))
    assert (mt.status() == 0).all(), mt.status()
    paths = mt.last_range_paths()
    ops = hand_inverted["a"]["ops"]
    rng = (ops["kind"] == OP_REMOVE) | (ops["kind"] == OP_ANNOTATE)
    proper = int((rng & (ops["pos1"] < ops["pos2"])).sum())
    print(tier, paths, "proper ranges", proper, "of", hand_inverted["ranges"], mt.last_paged_peaks())
    assert mt.is_paged(0)
    assert np.array_equal(mt.checksums(), hand_inverted["osums"])
    assert paths["one_page"] + paths["split_fallback"] + paths["general"] == hand_inverted["ranges"], paths
    assert 0 < paths["one_page"] + paths["split_fallback"] <= proper, paths


@pytest.mark.parametrize("tier", ["bench_c3", "paged", "narrow"])
def test_props_compaction_inside_range_mark(hand_annotate, tier):
    """(c) The annotate sweep on a handle with room for 384 property records: the sweep's 585
    annotates write about 1600 records and the document holds up to 148 live ones, so the record
    arena is compacted (paged_props_compact, from range_mark's props_ensure) every hundred-odd
    messages on the single-page path, some of them right after a boundary split that the page's
    metadata has not seen yet.  384 leaves the compacted arena under 7/8 full with a step's 64
    records in hand, so no tier hands the document on or fails it for the arena."""
    mt = _replay(hand_annotate, **dict(_tier_caps(tier), props_capacity=384))
    assert (mt.status() == 0).all(), mt.status()
    paths = mt.last_range_paths()
    print(tier, paths)
    assert paths["one_page"] > 0, paths
    assert np.array_equal(mt.checksums(), hand_annotate["osums"])
