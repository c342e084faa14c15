"""The view pass refreshes the window's unsettled-table entries (mt_paged.h pg_views_refresh)
instead of leaving them to the flush; the page search (pg_find) then reads the refreshed table's
view lengths.  Both sit on every message's path, and the checksums carry the per-message delta
hash, so one wrong page search, view length or table entry at any message fails a case."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS, OPS = 32, 1500
LONG_DOCS, LONG_OPS = 8, 8000


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


def _generated(oracle_lib, docs, ops):
    from fluidframework_amd import MergeTreeBatch
    cfg = _c3(ops)
    mt = MergeTreeBatch(docs, delta_log_capacity=0, **_bench_c3_caps())
    batch = mt.generate(cfg)
    host = batch.download()
    peaks = mt.last_paged_peaks()
    seed_off, seed = mt.generated_seeds(cfg)
    a = dict(host, seed_off=seed_off, seed=seed)
    osums, ost = oracle_lib.replay_batch(a, threads=4)
    assert (ost == 0).all()
    assert np.array_equal(mt.checksums(), osums), "the generated state differs from the oracle's replay"
    for v in a.values():
        v.setflags(write=False)
    return dict(a=a, osums=osums, docs=docs, gen_peaks=peaks)


@pytest.fixture(scope="module")
def stream(oracle_lib):
    """32 documents x 1500 messages of the C3 configuration, generated on the device once; the
    C restatement's checksums of their replay from the seeds (shared, never modified)."""
    return _generated(oracle_lib, DOCS, OPS)


@pytest.fixture(scope="module")
def long_stream(oracle_lib):
    """8 documents x 8000 C3 messages: directories that grow past 128 pages."""
    return _generated(oracle_lib, LONG_DOCS, LONG_OPS)


def _replay(s, **caps):
    from fluidframework_amd import MergeTreeBatch
    a = s["a"]
    mt = MergeTreeBatch(s["docs"], **caps)
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    return mt


@pytest.mark.parametrize("tier", ["bench_c3", "bench_c4", "paged", "tight", "narrow", "grow", "hm", "delta_log"])
def test_generated_stream_every_tier(stream, tier):
    """Every paged tier (compile-time and run-time capacities, packed, narrow, page metadata in
    HBM, with a delta log) replays the stream to the oracle's checksums.  On `tight` (an LDS
    table of 40 entries) the refresh's appends run at the bound pg_room keeps, and documents are
    handed on in the middle of the stream."""
    mt = _replay(stream, **_tier_caps(tier))
    assert (mt.status() == 0).all(), mt.status()
    assert np.array_equal(mt.checksums(), stream["osums"])
    peaks = mt.last_paged_peaks()
    print(tier, peaks)
    if tier == "tight":
        assert peaks["tight_handovers"] > 0, peaks


def test_long_directories(long_stream):
    """Directories of one, two and three chunks of 64 positions over one stream: they pass 64
    and 128 pages (130 at the end) at the bench's C3 capacities, and nothing is handed on."""
    mt = _replay(long_stream, **_tier_caps("bench_c3"))
    assert (mt.status() == 0).all(), mt.status()
    peaks = mt.last_paged_peaks()
    print(peaks, long_stream["gen_peaks"])
    assert peaks["pages"] > 128, peaks
    assert peaks["tight_handovers"] == 0, peaks
    assert np.array_equal(mt.checksums(), long_stream["osums"])


# ---------------------------------------------------------------- streams built by hand
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


def _same_page_twice():
    """(a) One writer that has seen everything works around position 10 for 300 messages
    (inserts with and without properties, annotates, removes), the minimum sequence number 20
    behind: consecutive messages act on the same page, so the view refreshes the table, the op
    dirties it again, and the rebuild at the flush follows messages later.  Ends with (d): an
    insert at the view's total length and ranges whose pos2 is the total."""
    d = _Doc()
    n = 40   # the writer's view length (seed: 40 units)
    for i in range(300):
        msn = max(0, d.seq - 20)
        k = i % 6
        if k in (0, 1, 3):
            d.send(1, _ins(10 + i % 3, "ab", {"k1": i % 5} if k == 1 else None), msn=msn)
            n += 2
        elif k == 2:
            d.send(1, _ann(9, 13, {"k2": i}), msn=msn)
        elif k == 4:
            d.send(1, _rem(11, 12), msn=msn)
            n -= 1
        else:
            d.send(1, _ann(10 + i % 2, 11 + i % 2, {"k3": i}), msn=msn)
    msn = d.seq - 20
    d.send(1, _ins(n, "end"), msn=msn)
    n += 3
    d.send(1, _ann(n - 5, n, {"k4": 1}), msn=msn)
    d.send(1, _rem(n - 2, n), msn=msn)
    n -= 2
    d.send(1, _ins(n, "z", {"k1": 9}), msn=msn)
    return "s" * 40, d.msgs


def _split_after_refresh():
    """(b) 260 one-unit inserts at position 7, each with a property set of its own (no two
    merge; the minimum sequence number stays 0): every message after the first finds the window
    changed, refreshes at the view, and each time the page's eighth leaf block appears the same
    message rebuilds the entries again in the page split."""
    d = _Doc()
    for i in range(260):
        d.send(1, _ins(7, "x", {"k5": i}))
    return "seedtext" * 2, d.msgs


def _zero_length_pages():
    """(c) Writer 2 stays at the reference sequence number it had before writer 1 put 150
    one-unit segments (alternating property sets: none merge) into the middle of the text, and
    the minimum sequence number is held below it: in writer 2's view those segments -- whole
    pages of them -- have length 0, all at one point, the gap at position 20.  Writer 2 inserts
    at the gap, before and after it, removes and annotates ranges that end at, start at and
    straddle it (searches strict and not, at page boundaries), and ends with (d): an insert at
    its view's total length and ranges whose pos2 is the total."""
    d = _Doc()
    d.send(1, _ins(40, "!"))      # 41 units; both writers have seen this
    d.send(2, _ann(0, 2, {"k6": 2}))
    r0 = d.seq                    # writer 2's reference sequence number from here on
    for i in range(150):
        d.send(1, _ins(20 + i, "y", {"k7": i % 2}), msn=1)
    n = 41                        # writer 2's view: the seed, "!", and its own ops
    g = 20

    def w2(op):
        d.send(2, op, ref=r0, msn=1)

    w2(_ins(g, "G"))
    n += 1
    w2(_ins(g - 1, "B"))
    n += 1
    g += 1                        # (the gap is at g or g + 1 now: its own insert landed beside it)
    w2(_ins(g + 2, "A"))
    n += 1
    for p1, p2 in ((g - 3, g), (g, g + 1), (g + 1, g + 3), (g - 1, g + 2)):
        w2(_ann(p1, p2, {"k6": p1}))
    for p1, p2 in ((g - 2, g), (g, g + 1), (g - 1, g + 1)):   # (positions shift down as units go)
        w2(_rem(p1, p2))
        n -= p2 - p1
    for p in (g - 3, g - 2, g - 1, g):
        w2(_ins(p, "i"))
        n += 1
        w2(_ann(p, p + 1, {"k8": p}))
    w2(_ins(n, "E"))
    n += 1
    w2(_ann(n - 3, n, {"k9": 1}))
    w2(_rem(n - 1, n))
    n -= 1
    w2(_ann(0, n, {"k10": 1}))
    # writer 1, which sees everything, goes on around the same place
    m = 41 + 150 + sum(1 for x in d.msgs[r0 + 150:] if x["contents"]["type"] == 0) - \
        sum(x["contents"]["pos2"] - x["contents"]["pos1"] for x in d.msgs[r0 + 150:] if x["contents"]["type"] == 1)
    for i in range(20):
        d.send(1, _ins(25 + 3 * i, "w"), msn=1)
        m += 1
    d.send(1, _ins(m, "END"), msn=1)
    m += 3
    d.send(1, _rem(m - 4, m), msn=1)
    return "t" * 40, d.msgs


HAND = [_same_page_twice, _split_after_refresh, _zero_length_pages]


@pytest.fixture(scope="module")
def hand(oracle_lib):
    """The hand-built documents as one batch, checked on the CPU first: the oracle replays every
    one with status 0 (every position lies inside its writer's view)."""
    from fluidframework_amd.wire import Batch, Interner
    b = Batch(Interner(synthetic=True))
    for f in HAND:
        seed, msgs = f()
        b.add_doc(seed, msgs)
    a = b.arrays()
    osums, ost = oracle_lib.replay_batch(a, threads=2)
    assert (ost == 0).all(), ost
    for v in a.values():
        v.setflags(write=False)
    return dict(a=a, osums=osums, docs=len(HAND))


@pytest.mark.parametrize("tier", ["bench_c3", "paged", "narrow"])
def test_hand_built_streams(hand, tier):
    """(a) same page twice, (b) page split right after the refresh, (c) pages of view length 0
    with searches at their edges, (d) past the end.  Every document is paged; the streams are a
    few hundred messages each and reach 16 pages at most (printed below), one chunk of the
    directory -- the long directories are test_long_directories'.  Document (b) holds 259
    unsettled segments at its end: more than the 220 entries of the bench's C3 table, so on
    `bench_c3` it is handed to the next tier in the middle of its stream."""
    mt = _replay(hand, **_tier_caps(tier))
    assert (mt.status() == 0).all(), mt.status()
    print(tier, mt.last_paged_peaks())
    assert all(mt.is_paged(d) for d in range(hand["docs"]))
    assert np.array_equal(mt.checksums(), hand["osums"])
