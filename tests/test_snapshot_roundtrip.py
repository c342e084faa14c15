"""The device round trip of cold catch-up (what bench.py --config c5 times): extract_snapshots_raw
-> snapshot.load_arrays_from_extract(chunk) -> a fresh handle (mt_load_snapshots, or
mt_snapshots_upload + load_async) -> the tail.  The oracle is the C restatement loading the same
arrays and replaying the same tail (pyoracle.load_replay_batch = Client.load + applyMsg):
statuses and checksums per document; after the load alone the segment table, leaf blocks and
property sets of a sample of documents equal OracleDoc.load(...).outputs().  Headers larger
than the flat capacities go through k_load_convert (paged at load); summaries with body chunks
load or fail as the reference's loadBody does (MT_DOC_INSERT_FAILED, MT_DOC_ALIASED)."""
import json
import os

import numpy as np
import pytest

import snap_util as su
from test_gpu_parity import SNAP_TIERS, _gpu_batch
from test_range_one_page import _bench_c3_caps, _bench_c4_caps, _hm_caps

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
STREAMS = {"c3": (16, 1200, 1000), "c4": (8, 800, 600)}     # documents, messages, messages before the summary
LOAD_TIERS = ["lds", "hbm", "paged", "tiny_paged", "paged_load", "grow", "hm"]

GEN_CAPS = {"c3": _bench_c3_caps, "c4": _bench_c4_caps}    # the handle a stream is generated on


def _cfg(name, ops):
    return dict(json.load(open(os.path.join(REPO, "bench", "configs.json")))[name], ops=ops)


def _caps(tier):
    return dict(_hm_caps(), delta_log_capacity=0) if tier == "hm" else SNAP_TIERS[tier]


def _handle(n, tier):
    from fluidframework_amd import MergeTreeBatch
    return MergeTreeBatch(n, **_caps(tier)) if tier == "hm" else _gpu_batch(n, **_caps(tier))


def _extract_head(a, cut, n):
    """The documents after their first `cut` messages, extracted on the device."""
    mt = _gpu_batch(n, lds_seg_capacity=0)
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(su.slice_records(a, 0, cut))
    assert (mt.status() == 0).all()
    raw = mt.extract_snapshots_raw()
    mt.close()
    return raw


def _outputs(mt, d):
    rows, leaves = mt.get_segments(d)
    return dict(text=mt.get_text(d), length=mt.get_length(d), leaves=list(leaves), segs=rows.tolist(),
                seg_props=mt.get_all_segment_props(d), status=int(mt.status()[d]))


def _oracle_loaded(oracle_lib, la, d):
    lo, hi = int(la["doc_off"][d]), int(la["doc_off"][d + 1])
    o = oracle_lib.OracleDoc.load(la["segs"][lo:hi], la["n_header"][d], la["text"], la["props"],
                                  la["min_seq"][d], la["cur_seq"][d]).outputs()
    return dict(text=o["text"], length=o["length"], leaves=list(o["leaves"]), segs=o["segs"].tolist(),
                seg_props=o["seg_props"], status=o["status"])


def _sub(la, lo, hi):
    """Summaries lo .. hi of load arrays (arenas shared, offsets absolute)."""
    off = la["doc_off"]
    return dict(la, segs=la["segs"][off[lo]:off[hi]], doc_off=off[lo:hi + 1] - off[lo], n_header=la["n_header"][lo:hi],
                min_seq=la["min_seq"][lo:hi], cur_seq=la["cur_seq"][lo:hi])


@pytest.fixture(scope="module")
def heads(oracle_lib):
    """Per stream: the generated arrays, the header-only load arrays of the device's own
    extraction after the cut (checked against the restatement's extraction), the tail batch and
    the restatement's statuses and checksums of load + tail."""
    from fluidframework_amd.snapshot import load_arrays_from_extract
    out = {}
    for name, (docs, ops, cut) in STREAMS.items():
        a = su.generated_stream(oracle_lib, _cfg(name, ops), docs, GEN_CAPS[name]())
        raw = _extract_head(a, cut, docs)
        want, _ = oracle_lib.replay_extract_batch(a, op_limit=cut, threads=8)
        assert not su.diff_docs(su.split_raw(raw), su.split_raw(want))
        la = load_arrays_from_extract(*raw, chunk_size=10000)
        assert (la["n_header"] == np.diff(la["doc_off"])).all()          # header only
        tail = su.slice_records(a, cut, None)
        osums, ost = oracle_lib.load_replay_batch(la, tail, threads=8)
        assert (ost == 0).all()
        out[name] = dict(a=a, la=la, tail=tail, osums=osums, ost=ost, docs=docs, raw=raw)
    return out


@pytest.mark.parametrize("tier", LOAD_TIERS)
@pytest.mark.parametrize("name", list(STREAMS))
def test_header_only_round_trip(oracle_lib, heads, name, tier):
    """Header-only summaries loaded by mt_load_snapshots at every tier, then the tail.  On the
    HBM-metadata handle (seg_capacity 256, unsettled_capacity 216) the C4 headers (565-745
    records, up to 782 unsettled segments at lag 1000) outgrow the paged capacities at the load:
    the load's growth step pages them in the big region (last_grown)."""
    s = heads[name]
    mt = _handle(s["docs"], tier)
    mt.load_snapshots(s["la"])
    assert (mt.status() == 0).all(), mt.status()
    for d in (0, s["docs"] // 2, s["docs"] - 1):
        assert _outputs(mt, d) == _oracle_loaded(oracle_lib, s["la"], d), (name, tier, d)
    paged = [mt.is_paged(d) for d in range(s["docs"])]
    print(name, tier, "paged after the load", sum(paged), "of", s["docs"], mt.last_grown())
    if (name, tier) == ("c4", "hm"):
        assert all(paged) and mt.last_grown()["in_big_region"] == s["docs"]
    if tier == "paged_load":   # headers of 350-750 records at seg_capacity 48: paged at the load
        assert all(paged)
    mt.apply_arrays(s["tail"])
    assert np.array_equal(mt.status(), s["ost"])
    assert np.array_equal(mt.checksums(), s["osums"]), (name, tier)
    print(name, tier, "paged after the tail", sum(mt.is_paged(d) for d in range(s["docs"])), mt.last_paged_peaks())
    mt.close()


@pytest.mark.parametrize("tier", ["lds", "paged_load"])
@pytest.mark.parametrize("name", list(STREAMS))
def test_header_only_round_trip_async(heads, name, tier):
    """upload_snapshots(...).load_async() + upload(tail).apply_async(), and the same with the
    summaries uploaded in two document ranges."""
    s = heads[name]
    n = s["docs"]
    for ranges in ([(0, n)], [(0, n // 3), (n // 3, n)]):
        mt = _handle(n, tier)
        held = []
        for lo, hi in ranges:
            snaps = mt.upload_snapshots(_sub(s["la"], lo, hi), doc_lo=lo)
            snaps.load_async()
            held.append(snaps)
        b = mt.upload(s["tail"])
        b.apply_async()
        mt.sync()
        assert np.array_equal(mt.status(), s["ost"]), ranges
        assert np.array_equal(mt.checksums(), s["osums"]), (name, tier, ranges)
        b.free()
        for snaps in held:
            snaps.free()
        mt.close()


def test_settled_round_trip_is_a_fixed_point(oracle_lib, heads):
    """Settled header-only documents: extract -> load -> extract again gives the same records."""
    from fluidframework_amd.snapshot import load_arrays_from_extract
    s = heads["c3"]
    a, n = s["a"], s["docs"]
    _, _, cut = STREAMS["c3"]
    # settle: one non-op record per document moving minSeq to the current sequence number
    head = su.slice_records(a, 0, cut)
    ops = head["ops"].copy()
    settle = np.zeros(n, dtype=ops.dtype)
    settle["seq"] = settle["min_seq"] = cut + 1
    settle["ref_seq"] = cut
    settle["client"] = 1
    settle["kind"] = 3
    settle["props"] = 0xFFFFFFFF
    off = head["doc_off"]
    parts, new_off = [], [0]
    for d in range(n):
        parts += [ops[off[d]:off[d + 1]], settle[d:d + 1]]
        new_off.append(new_off[-1] + int(off[d + 1] - off[d]) + 1)
    settled = dict(head, ops=np.concatenate(parts), doc_off=np.asarray(new_off, dtype=np.int64))
    want, (_, st) = oracle_lib.replay_extract_batch(settled, threads=8)
    assert (st == 0).all()
    mt = _gpu_batch(n, lds_seg_capacity=0)
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(settled)
    assert (mt.status() == 0).all()
    first = mt.extract_snapshots_raw()
    assert not su.diff_docs(su.split_raw(first), su.split_raw(want))
    assert not (first[1]["flags"] & 0x10).any()          # settled: no merge info
    for tier in ("lds", "paged_load"):
        mt2 = _handle(n, tier)
        mt2.load_snapshots(load_arrays_from_extract(*first, chunk_size=10000))
        assert (mt2.status() == 0).all()
        again = mt2.extract_snapshots_raw()
        assert not su.diff_docs(su.split_raw(again), su.split_raw(first)), tier
        mt2.close()
    mt.close()


def test_large_headers_page_at_load(oracle_lib):
    """Two C3 documents of 12000 messages (about 4000 records each) loaded at seg_capacity 48:
    k_load_convert pages each header into more than 64 pages, the directory's second chunk, and
    a 200-message tail replays on it to the restatement's checksums."""
    from fluidframework_amd.snapshot import load_arrays_from_extract
    docs, ops, cut = 2, 12000, 11800
    a = su.generated_stream(oracle_lib, _cfg("c3", ops), docs, _hm_caps())
    raw = _extract_head(a, cut, docs)
    want, _ = oracle_lib.replay_extract_batch(a, op_limit=cut, threads=2)
    assert not su.diff_docs(su.split_raw(raw), su.split_raw(want))
    la = load_arrays_from_extract(*raw, chunk_size=1 << 30)
    tail = su.slice_records(a, cut, None)
    osums, ost = oracle_lib.load_replay_batch(la, tail, threads=2)
    assert (ost == 0).all()
    mt = _handle(docs, "paged_load")
    mt.load_snapshots(la)
    assert (mt.status() == 0).all(), mt.status()
    pages = [su.doc_header(mt, d)[3] for d in range(docs)]
    # (the load keeps no high-water marks: last_paged_peaks() counts a batch's or a generation's;
    # the directory's own page count is in the document header)
    print("large headers: records", np.diff(la["doc_off"]).tolist(), "pages after the load", pages)
    assert all(su.doc_header(mt, d)[2] for d in range(docs)) and min(pages) > 64, pages
    for d in range(docs):
        assert _outputs(mt, d) == _oracle_loaded(oracle_lib, la, d), d
    mt.apply_arrays(tail)
    assert np.array_equal(mt.status(), ost)
    assert np.array_equal(mt.checksums(), osums)
    print("large headers: after the tail", mt.last_paged_peaks())
    assert mt.last_paged_peaks()["pages"] > 64
    mt.close()


@pytest.fixture(scope="module")
def bodies(oracle_lib):
    """Summaries with body chunks: 16 C3 documents after 300 messages, the even ones settled
    before the extraction (every writer's last reference sequence number at the end: a
    non-op message moves minSeq there), the odd ones unsettled (their bodies carry merge info,
    which the reference's loadBody fails on).  Checked on the CPU before any GPU time: at least
    half of the documents load and replay with status 0 in the restatement."""
    n, ops, cut = 16, 500, 300
    a = su.generated_stream(oracle_lib, _cfg("c3", ops), n, _bench_c3_caps())
    head = su.slice_records(a, 0, cut)
    op = head["ops"]
    off = head["doc_off"]
    assert len(a["text"]) > 64
    parts, new_off = [], [0]
    for d in range(n):
        parts.append(op[off[d]:off[d + 1]])
        k = int(off[d + 1] - off[d])
        if d % 2 == 0:
            s = np.zeros(1, dtype=op.dtype)
            s["seq"] = s["min_seq"] = cut + 1
            s["ref_seq"] = cut
            s["client"] = 1
            s["kind"] = 3
            s["props"] = 0xFFFFFFFF
            parts.append(s)
            k += 1
        new_off.append(new_off[-1] + k)
    head = dict(head, ops=np.concatenate(parts), doc_off=np.asarray(new_off, dtype=np.int64))
    # the tail: six messages per document by writer 1, each at refSeq = the sequence number
    # before it (valid in any replica that loaded): inserts at the front, removes, annotates
    # (text and a property record borrowed from the stream's arenas)
    pr = int(a["ops"]["props"][np.flatnonzero(a["ops"]["kind"] == 2)[0]])
    t = np.zeros(6 * n, dtype=op.dtype)
    for d in range(n):
        cur = cut + 1 if d % 2 == 0 else cut
        msn = cur if d % 2 == 0 else int(op[off[d + 1] - 1]["min_seq"])
        for k, (kind, p1, p2, props) in enumerate([(0, 0, 3, 0xFFFFFFFF), (1, 1, 2, 0xFFFFFFFF), (2, 0, 4, pr),
                                                  (0, 2, 5, 0xFFFFFFFF), (1, 0, 3, 0xFFFFFFFF), (2, 1, 6, pr)]):
            r = t[6 * d + k]
            r["seq"], r["ref_seq"], r["min_seq"] = cur + 1 + k, cur + k, msn
            r["kind"], r["pos1"], r["pos2"], r["props"], r["client"] = kind, p1, p2, props, 1
            r["payload"] = 7 * k
    tail = dict(a, ops=t, doc_off=np.arange(0, 6 * n + 1, 6, dtype=np.int64))
    return dict(a=a, head=head, tail=tail, n=n)


@pytest.mark.parametrize("chunk", [150, 5])
def test_bodies_round_trip(oracle_lib, bodies, chunk):
    """chunk = 150, and a chunk smaller than the longest record (every record but the first is
    in the body): the statuses of load + tail agree with the restatement document by
    document, the checksums of the documents that loaded are equal, and at least half of the
    documents load with status 0."""
    from fluidframework_amd.snapshot import load_arrays_from_extract
    a, n = bodies["a"], bodies["n"]
    src = _gpu_batch(n, lds_seg_capacity=0)
    src.load_initial_text(a["seed_off"], a["seed"])
    src.apply_arrays(bodies["head"])
    assert (src.status() == 0).all()
    raw = src.extract_snapshots_raw()
    src.close()
    want, _ = oracle_lib.replay_extract_batch(bodies["head"], threads=8)
    assert not su.diff_docs(su.split_raw(raw), su.split_raw(want))
    la = load_arrays_from_extract(*raw, chunk_size=chunk)
    assert (la["n_header"] < np.diff(la["doc_off"])).all()              # every summary has a body
    assert chunk >= 150 or int(raw[1]["len"].max()) > chunk
    osums, ost = oracle_lib.load_replay_batch(la, bodies["tail"], threads=8)
    print("chunk", chunk, "oracle statuses", ost.tolist())
    assert int((ost == 0).sum()) * 2 >= n, ost
    assert (ost[0::2] == 0).all()                                        # the settled documents load
    assert (ost != 0).any()                                              # and unsettled bodies fail
    for tier in ("lds", "paged_load"):
        mt = _handle(n, tier)
        mt.load_snapshots(la)
        mt.apply_arrays(bodies["tail"])
        assert np.array_equal(mt.status(), ost), (tier, mt.status(), ost)
        ok = ost == 0
        assert np.array_equal(mt.checksums()[ok], osums[ok]), tier
        mt.close()
