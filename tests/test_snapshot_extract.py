"""k_extract (mt_extract_snapshots = SnapshotV1.extractSync, MT/snapshotV1.ts:156-252) against
the C restatement's orc_extract (oracle/mt_oracle.c, pinned byte for byte to the reference's
own summaries by tests/test_extract.py), record for record: every mt_seg_rec field, each
record's text slice and property pairs, the per-document counts and the window -- on generated
streams at every storage tier and several points of the stream, on hand-built documents that
meet each coalescing rule at its edge (tests/snap_util.py), and on live (participant) handles,
whose unacked inserts and pending removes the summary elides."""
import json
import os

import numpy as np
import pytest

import golden_util as gu
import snap_util as su
from test_gpu_parity import TIERS, _gpu_batch
from test_range_one_page import _bench_c3_caps, _bench_c4_caps, _hm_caps

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = (0, 1, 300, None)         # messages applied before each extraction (None: all)
STREAMS = {"c3": (16, 1200), "c4": (8, 800)}
FLAT = dict(seg_capacity=8192, text_capacity=1 << 17, delta_log_capacity=0)
ALL_TIERS = list(TIERS) + ["bench_c3", "hm"]
PAGED_TIERS = ("paged", "tiny_paged", "tight", "narrow", "grow", "bench_c3", "hm")


def tier_caps(tier):
    if tier == "bench_c3":
        return dict(_bench_c3_caps(), delta_log_capacity=0)
    if tier == "hm":
        return dict(_hm_caps(), delta_log_capacity=0)
    return dict(FLAT, page_capacity=-1) | TIERS[tier]


GEN_CAPS = {"c3": _bench_c3_caps, "c4": _bench_c4_caps}    # the handle a stream is generated on


def _cfg(name, ops):
    return dict(json.load(open(os.path.join(REPO, "bench", "configs.json")))[name], ops=ops)


@pytest.fixture(scope="module")
def streams(oracle_lib):
    """The C3 and C4 streams, generated on the device once, and the restatement's extraction
    of every document after POINTS messages (shared, never modified)."""
    out = {}
    for name, (docs, ops) in STREAMS.items():
        a = su.generated_stream(oracle_lib, _cfg(name, ops), docs, GEN_CAPS[name]())
        want = {}
        for p in POINTS:
            raw, (_, st) = oracle_lib.replay_extract_batch(a, op_limit=-1 if p is None else p, threads=8)
            assert (st == 0).all()
            want[p] = su.split_raw(raw)
        out[name] = dict(a=a, want=want, docs=docs)
    return out


@pytest.mark.parametrize("tier", ALL_TIERS)
@pytest.mark.parametrize("name", list(STREAMS))
def test_generated_streams_every_tier(streams, name, tier):
    """The stream applied in slices with an extraction between them: after 0, 1, 300 and all
    messages the device's records equal the restatement's."""
    from fluidframework_amd import MergeTreeBatch
    s = streams[name]
    a = s["a"]
    mt = MergeTreeBatch(s["docs"], **tier_caps(tier))
    mt.load_initial_text(a["seed_off"], a["seed"])
    done = 0
    peak_pages = 0
    for p in POINTS:
        if p != 0:
            mt.apply_arrays(su.slice_records(a, done, p))
            done = p
            peak_pages = max(peak_pages, mt.last_paged_peaks()["pages"])
        assert (mt.status() == 0).all(), (p, mt.status())
        bad = su.diff_docs(su.split_raw(mt.extract_snapshots_raw()), s["want"][p])
        assert not bad, (name, tier, p, bad[:3])
    paged = [mt.is_paged(d) for d in range(s["docs"])]
    print(name, tier, "paged documents", sum(paged), "of", s["docs"], "peak pages", peak_pages)
    if tier in PAGED_TIERS:
        assert all(paged)
    if tier == "grow":
        assert peak_pages > 16
    if tier in ("lds", "hbm", "tiny"):
        assert not any(paged)
    mt.close()


# ---------------------------------------------------------------- hand-built documents
HAND_TIERS = {"lds": TIERS["lds"], "paged": TIERS["paged"], "grow": TIERS["grow"]}


@pytest.fixture(scope="module")
def hand(oracle_lib):
    docs = su.handbuilt_docs()
    b, a = su.encode(docs)
    raw, (_, st) = oracle_lib.replay_extract_batch(a, threads=4)
    assert st.tolist() == [0] * len(docs)          # the oracle on the CPU first
    return dict(names=list(docs), a=a, want=su.split_raw(raw))


@pytest.mark.parametrize("tier", list(HAND_TIERS))
def test_handbuilt_rules(hand, tier):
    """(a) the 256-unit rule at 255 / 256 / 257, (b) newlines, (c) markers, (d) property sets
    compared as sets, {} against none, values that never match, (e) segments and removals at
    minSeq and minSeq + 1, (f) runs of 40 and of 140 segments over page edges, (g) empty documents.
    For (f) the 140-segment run carries the guarantee: a page has 64 segment slots, so it lies over
    at least two page edges wherever they are (the page table is not readable from here); the
    40-segment run lies in a document of 5 pages, and a kernel that resets its candidate at a page
    edge splits it too (tried once with such a build: 51 records for 49)."""
    a = hand["a"]
    mt = _gpu_batch(len(hand["names"]), **HAND_TIERS[tier])
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    assert (mt.status() == 0).all(), mt.status()
    got = su.split_raw(mt.extract_snapshots_raw())
    bad = [(hand["names"][d],) + tuple(rest) for d, *rest in su.diff_docs(got, hand["want"])]
    assert not bad, (tier, bad[:4])
    if tier != "lds":
        for name in ("run40", "run140"):
            _, _, paged, pages = su.doc_header(mt, hand["names"].index(name))
            print(tier, name, "pages", pages)
            assert paged
            # 140 segments cannot lie in fewer than three 64-slot pages: two page edges inside the run
            assert name != "run140" or pages >= 4
    mt.close()


@pytest.mark.parametrize("tier", list(HAND_TIERS))
def test_arena_halves(oracle_lib, tier):
    """(h) Extraction after the text and property arenas have been compacted into their other
    halves (text_half / props_half of the header are 1 at some extraction points): records,
    text and properties equal the restatement's after every round of the document."""
    docs = su.arena_docs()
    b, a = su.encode(docs)
    n = int(a["doc_off"][1])
    cuts = [i + 1 for i in range(n) if a["ops"]["kind"][i] == 3] + [n]     # after each round's non-op message
    # (a tier keeps a step's 64 property records in hand: 128 leaves room for the ~10 live ones)
    mt = _gpu_batch(1, **dict(HAND_TIERS[tier], text_capacity=512, props_capacity=128))
    mt.load_initial_text(a["seed_off"], a["seed"])
    done = 0
    halves = set()
    for c in cuts:
        mt.apply_arrays(su.slice_records(a, done, c))
        done = c
        assert (mt.status() == 0).all(), (c, mt.status(), mt.debug_raw(0)[1][su.HDR_PAD:su.HDR_PAD + 4])
        raw, (_, st) = oracle_lib.replay_extract_batch(a, op_limit=c)
        assert st.tolist() == [0]
        bad = su.diff_docs(su.split_raw(mt.extract_snapshots_raw()), su.split_raw(raw))
        assert not bad, (tier, c, bad[:3])
        th, ph, _, _ = su.doc_header(mt, 0)
        halves.add(("text", th))
        halves.add(("props", ph))
    print(tier, sorted(halves))
    assert ("text", 1) in halves and ("props", 1) in halves, halves
    mt.close()


@pytest.mark.parametrize("tier", list(HAND_TIERS))
def test_failed_neighbour(oracle_lib, tier):
    """(i) Three documents, the middle one failing (an insert past the end:
    MT_DOC_INSERT_FAILED).  A failed document stops at its failing message: its extraction is
    that of the messages before it (window included), and its neighbours' records, text and
    property offsets are exact."""
    def body(fail):
        d = su.Doc("seed", filler=4)
        d.append("ab", {"k1": 1})
        d.append("cd", {"k1": 1})
        d.noop(d.seq)
        if fail:
            d.insert(d.length + 3, "past the end")
            d.length -= len("past the end")
        d.append("ef", {"k2": 2})
        d.append("gh")
        d.settle()
        return d
    docs = {"left": body(False), "failed": body(True), "right": body(False)}
    b, a = su.encode(docs, gu.Interner())
    raw, (_, st) = oracle_lib.replay_extract_batch(a, threads=2)
    assert st.tolist() == [0, 1, 0]
    want = su.split_raw(raw)
    # the failed document = its first messages alone (the failing insert is message 8)
    n_before = next(i for i, m in enumerate(docs["failed"].msgs) if m["contents"] and m["contents"].get("seg") == "past the end")
    stopped = dict(docs)
    stopped["failed"] = su.Doc("seed")
    stopped["failed"].msgs = docs["failed"].msgs[:n_before]
    _, a2 = su.encode(stopped, gu.Interner())
    raw2, (_, st2) = oracle_lib.replay_extract_batch(a2)
    assert st2.tolist() == [0, 0, 0]
    want_stopped = su.split_raw(raw2)
    assert not su.diff_docs([want[1]], [want_stopped[1]])
    # "seed\n", three "\n", "abcd" {k1}: 5 records, 12 text units, 3 property words; window (6, 7)
    assert su.norm_doc(want[1])["counts"] == (5, 12, 3) and su.norm_doc(want[1])["window"] == (6, 7)
    mt = _gpu_batch(3, **HAND_TIERS[tier])
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    assert mt.status().tolist() == [0, 1, 0]
    bad = su.diff_docs(su.split_raw(mt.extract_snapshots_raw()), want)
    assert not bad, (tier, bad)
    mt.close()


# ---------------------------------------------------------------- live handles
LIVE_HANDLES = {"hbm": dict(lds=-1, caps=None), "lds64": dict(lds=64, caps=None),
                "grow": dict(lds=-1, caps=dict(seg_capacity=64, text_capacity=1024, live_group_capacity=16))}


@pytest.mark.parametrize("handle", list(LIVE_HANDLES))
def test_live_handles_match_reference_and_oracle(oracle_lib, handle):
    """LiveClient documents of ref_live_snap: at every point where the reference's participant
    wrote its summary, the device's extraction encodes to those bytes and equals orc_extract of
    the participant restatement (unacked inserts and pending removes elided, :189)."""
    from fluidframework_amd.live import OP_GROUP, LiveClient
    from test_extract import live_steps
    fx = gu.load("ref_live_snap")
    h = LIVE_HANDLES[handle]
    n_points = 0
    for doc in fx["docs"]:
        interner = gu.Interner(synthetic=True)
        a, steps, names = live_steps(doc, gu.Interner(synthetic=True))
        od = oracle_lib.OracleDoc.new(a["seed"][: a["seed_off"][1]])
        lc = LiveClient(doc["seed_text"], interner=interner, lds_seg_capacity=h["lds"],
                        **(h["caps"] or dict(seg_capacity=16384, text_capacity=1 << 17)))
        lc.startOrUpdateCollaboration("local-0")
        unseq = []
        events = iter(doc["events"])
        for st in steps:
            if st[0] == "S":
                lc.flush()
                got = lc.mt.extract_snapshots()[0]
                want = od.extract()
                bad = su.diff_docs([got], [want])
                assert not bad, (handle, doc["doc"], n_points, bad)
                short = {v: k for k, v in lc.short.items() if v != 0}
                assert su.chunks_of(got, interner, {**short, 0: st[1]}, fx["config"]["chunk"]) == st[2]
                n_points += 1
                continue
            ev = next(events)
            if st[0] == "L":
                op = ev[1]
                if op["type"] == 0:
                    assert lc.insertSegmentLocal(op["pos1"], op["seg"]) == op
                elif op["type"] == 1:
                    assert lc.removeRangeLocal(op["pos1"], op["pos2"]) == op
                else:
                    assert lc.annotateRangeLocal(op["pos1"], op["pos2"], op["props"], op.get("combiningOp")) == op
                assert od.apply_all(a["ops"][st[1]:st[2]], a["text"], a["props"]) == 0
                unseq.append(op)
            elif st[0] == "M":
                _, cid, seq, ref, msn, op = ev
                lc.applyMsg(dict(clientId=cid, sequenceNumber=seq, referenceSequenceNumber=ref,
                                 minimumSequenceNumber=msn, type="op", contents=op))
                assert od.apply_all(a["ops"][st[1]:st[2]], a["text"], a["props"]) == 0
                if st[3]:
                    unseq.pop(0)
            else:
                lc.startOrUpdateCollaboration(st[1])
                assert [lc.regeneratePendingOp(o) for o in unseq] == st[2]
                for op in unseq:
                    for m in (op["ops"] if op["type"] == OP_GROUP else [op]):
                        assert od.regenerate(m["type"]) is not None
                unseq = list(st[2])
        lc.close()
    assert n_points >= 20
