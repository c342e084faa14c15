"""Bulk cursor read-outs on the device (mt_locate_segments / mt_locate_uids /
mt_get_view_lengths_bulk / mt_resolve_remote_positions, MergeTreeBatch.locate_segments /
locate_uids / get_view_lengths_bulk / resolve_remote_positions / locate_segments_device, the Node
facade's getContainingSegments / getPositions / resolveRemoteClientPosition):
MergeTree.getContainingSegment, getPosition and getLength for many (doc, pos | uid, refSeq,
client) cursors in one launch.

Expected values are the reference's own (tests/golden/ref_readouts*: every containing query's
offset, view position, observer position, length and marker type; every view's length) and, where
no fixture holds them, the single-query calls and a host derivation from the raw segment rows.
The device answers a remote view from prefix sums of its leaves' view lengths, which is the
reference's tree exactly when getLength in the view (`n`) equals the sum of the leaves (`leaves`);
the other views' queries take the host path, and the tests pin which ones those are."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch   # before the replay library loads: both then share one HIP runtime (as in bench.py)

import golden_util as gu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = -(1 << 31)          # MT_RSEQ_NONE
LOCAL_BASE = 0x40000000    # MT_LOCAL_BASE: unacked sequence numbers (live handles)
HOST = 1                   # MT_HIT_HOST
FIELDS = ("row", "uid", "position", "offset", "length", "seq", "client", "removed_seq", "removed_client",
          "marker_ref_type")

# the storage tiers of tests/test_events.py (READ_TIERS), copied
TIERS = {"lds": dict(lds_seg_capacity=0, page_capacity=-1), "hbm": dict(lds_seg_capacity=-1, page_capacity=-1),
         "paged": dict(lds_seg_capacity=-1, page_capacity=256, unsettled_capacity=2048, page_heap_capacity=2048),
         "tight": dict(lds_seg_capacity=16, page_capacity=256, unsettled_capacity=2048, page_heap_capacity=2048,
                       lds_page_capacity=24, lds_unsettled_capacity=40, lds_page_heap_capacity=40),
         "narrow": dict(lds_seg_capacity=16, page_capacity=256, unsettled_capacity=2048,
                        page_heap_capacity=2048, lds_page_capacity=200, lds_unsettled_capacity=600,
                        lds_page_heap_capacity=600, lds_narrow_overlap=1),
         "grow": dict(lds_seg_capacity=16, page_capacity=12, unsettled_capacity=16, page_heap_capacity=16),
         # >= 512 pages and no delta log: the page metadata in HBM (kHM)
         "hm": dict(lds_seg_capacity=-1, page_capacity=1600, unsettled_capacity=2048, page_heap_capacity=2048)}
PAGED_LOAD = dict(seg_capacity=48, lds_seg_capacity=16, props_capacity=4096, page_capacity=256,
                  unsettled_capacity=2048, page_heap_capacity=2048)

# queries whose view has n != leaves in the fixture's `lengths` (answered by the host path), of all
HOST_PATH = {"ref_readouts": (428, 3802), "ref_readouts_wide": (888, 4788), "ref_readouts_xl": (738, 2484)}

_cursors = {}


def _fixture_cursors(name):
    """The fixture's containing queries and views as arrays, with what the reference gives (once)."""
    if name in _cursors:
        return _cursors[name]
    fx = gu.load(name)
    q = dict(doc=[], pos=[], ref=[], cli=[], found=[], offset=[], vpos=[], lpos=[], length=[], marker=[], host=[],
             view_n=[])
    v = dict(doc=[], ref=[], cli=[], n=[])
    obs_len = []
    for i, d in enumerate(fx["docs"]):
        n_of = {(r, c): (n, leaves) for r, c, n, _, leaves in d["lengths"]}
        obs_len.append(next(n for r, c, n, _, _ in d["lengths"] if c == 0))
        for r, c, n, _, _ in d["lengths"]:
            v["doc"].append(i), v["ref"].append(r), v["cli"].append(c), v["n"].append(n)
        for pos, ref, cli, exp, _ in d["containing"]:
            n, leaves = n_of[(ref, cli)]
            q["doc"].append(i), q["pos"].append(pos), q["ref"].append(ref), q["cli"].append(cli)
            q["host"].append(n != leaves), q["view_n"].append(n), q["found"].append(exp is not None)
            offset, vpos, lpos, clen, _, state = exp if exp is not None else (0, 0, 0, 0, None, {})
            q["offset"].append(offset), q["vpos"].append(vpos), q["lpos"].append(lpos), q["length"].append(clen)
            q["marker"].append(state.get("m", -1))
    q = {k: np.asarray(x, dtype=bool if k in ("found", "host") else np.int64) for k, x in q.items()}
    v = {k: np.asarray(x, dtype=np.int64) for k, x in v.items()}
    q["obs_len"] = np.asarray(obs_len, dtype=np.int64)[q["doc"]]
    _cursors[name] = (fx, q, v)
    return _cursors[name]


def test_host_path_condition_counts_derive_from_the_fixtures():
    """The views in which the reference's getLength differs from the sum of its leaves: how many
    containing queries of each fixture lie in one (CPU; the GPU test asserts the set).  None is
    an observer (client 0) query."""
    for name, (host, total) in HOST_PATH.items():
        _, q, _ = _fixture_cursors(name)
        assert (int(q["host"].sum()), len(q["host"])) == (host, total), name
        assert (q["cli"] == 0).any() and not q["host"][q["cli"] == 0].any(), name


def _batch(n_docs, **kw):
    from fluidframework_amd import MergeTreeBatch
    kw.setdefault("seg_capacity", 8192)
    kw.setdefault("text_capacity", 1 << 17)
    return MergeTreeBatch(n_docs, **kw)


def _replay(name, tier, **kw):
    fx = gu.load(name)
    a = gu.encode_docs(fx, gu.interner_for(fx))
    mt = _batch(len(fx["docs"]), **dict(TIERS[tier], **kw))
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    return fx, mt


# ---------------------------------------------------------------- 1. reference parity
@pytest.mark.gpu
@pytest.mark.parametrize("name,tier", [("ref_readouts", t) for t in ("lds", "hbm", "paged", "tight", "narrow", "grow")] +
                         [("ref_readouts_wide", "paged"), ("ref_readouts_xl", "paged"), ("ref_readouts_xl", "hm")])
def test_bulk_segments_match_reference(name, tier):
    """One locate_segments call for every containing query of the fixture, one locate_uids call
    for the segments found (in the query's view, and in the observer view), one
    get_view_lengths_bulk call for every view (ref_readouts_xl: a fixed-seed sample of 20 000) and
    one resolve_remote_positions call equal the reference; the records flagged as answered by the
    host path are exactly those of the views with n != leaves."""
    fx, q, v = _fixture_cursors(name)
    a = gu.encode_docs(fx, gu.Interner())
    mt = _batch(len(fx["docs"]), **TIERS[tier])
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    assert (mt.status() == 0).all()
    hits = mt.locate_segments(q["doc"], q["pos"], q["ref"], q["cli"])
    queries, host, ms = mt.last_locate()
    assert (queries, host) == (len(q["doc"]), HOST_PATH[name][0]) and ms > 0
    f = q["found"]
    assert np.array_equal(hits["row"] >= 0, f)
    for got, want in (("offset", "offset"), ("position", "vpos"), ("local_position", "lpos"), ("length", "length"),
                      ("marker_ref_type", "marker")):
        bad = np.flatnonzero(hits[got][f] != q[want][f])
        assert len(bad) == 0, (got, bad[:5], hits[f][bad[:5]], q[want][f][bad[:5]])
    assert np.array_equal((hits["flags"] & HOST) != 0, q["host"])
    assert not (hits["flags"] & ~np.uint32(HOST)).any()
    # getPosition of the segments found, by id: in the query's view and in the observer view
    by_uid = mt.locate_uids(q["doc"][f], hits["uid"][f], q["ref"][f], q["cli"][f])
    assert np.array_equal(by_uid["position"], q["vpos"][f]) and np.array_equal(by_uid["local_position"], q["lpos"][f])
    assert np.array_equal(by_uid["row"], hits["row"][f]) and not by_uid["offset"].any()
    assert np.array_equal((by_uid["flags"] & HOST) != 0, q["host"][f])
    obs = mt.locate_uids(q["doc"][f], hits["uid"][f])
    assert np.array_equal(obs["position"], q["lpos"][f]) and np.array_equal(obs["local_position"], q["lpos"][f])
    assert not obs["flags"].any() and mt.last_locate()[1] == 0
    # getLength in every view
    sel = np.arange(len(v["doc"]))
    if name == "ref_readouts_xl":
        sel = np.sort(np.random.default_rng(20241020).choice(len(sel), 20000, replace=False))
    assert np.array_equal(mt.get_view_lengths_bulk(v["doc"][sel], v["ref"][sel], v["cli"][sel]), v["n"][sel])
    assert mt.last_locate()[1] == 0   # exact in every view: no host path
    # resolveRemoteClientPosition
    want = np.where(f, q["lpos"] + q["offset"], np.where(q["pos"] == q["view_n"], q["obs_len"], -1))
    assert (want[~f] >= 0).any()
    assert np.array_equal(mt.resolve_remote_positions(q["doc"], q["pos"], q["ref"], q["cli"]), want)
    # one past the view's length, in the views whose leaves add up to it: no segment, undefined
    e = ~f & ~q["host"]
    assert (mt.resolve_remote_positions(q["doc"][e], q["view_n"][e] + 1, q["ref"][e], q["cli"][e]) == -1).all() and e.any()


# ---------------------------------------------------------------- the single-query comparison
def _table(mt, d):
    """Document d's rows from the raw segment records, as the bulk record's fields, with the
    observer position of every row (the host derivation of an observer-view answer)."""
    raw, hdr = mt.debug_raw(d)
    a = raw.view(np.int32)
    seq, rseq = a[:, 1].copy(), a[:, 2].copy()
    t = dict(length=a[:, 0].copy(), client=(a[:, 3] << 16) >> 16, removed_client=np.where(rseq == NONE, NONE, a[:, 3] >> 16),
             uid=raw[:, 6] & 0x7FFFFFFF, marker_ref_type=np.where(raw[:, 6] >> 31, a[:, 4], -1))
    t["seq"] = np.where(seq >= LOCAL_BASE, -1, seq)
    t["removed_seq"] = np.where(rseq >= LOCAL_BASE, -1, rseq)
    vis = np.where(rseq == NONE, t["length"], 0)
    t["position"] = np.cumsum(vis) - vis
    t["end"] = np.cumsum(vis)
    t["cur_seq"], t["min_seq"], t["pages"] = int(hdr[3]), int(hdr[4]), int(hdr[25])
    return t


def _check_observer_table(hits, t, pos=None, uids=None):
    """Observer-view records against the host derivation: by position (the first row whose
    inclusive prefix exceeds pos) or by uid."""
    n = len(t["length"])
    if pos is not None:
        row = np.searchsorted(t["end"], np.asarray(pos), side="right")
    else:
        where = {int(u): i for i, u in enumerate(t["uid"])}
        row = np.asarray([where.get(int(u), n) for u in uids])
    ok = row < n
    assert np.array_equal(hits["row"], np.where(ok, row, -1))
    r = row[ok]
    for k in ("uid", "position", "length", "seq", "client", "removed_seq", "removed_client", "marker_ref_type"):
        assert np.array_equal(hits[k][ok], t[k][r]), k
    assert np.array_equal(hits["local_position"][ok], t["position"][r])
    assert np.array_equal(hits["offset"][ok], (np.asarray(pos)[ok] - t["position"][r]) if pos is not None else 0 * r)
    assert not hits["flags"].any()


def _check_single(mt, hits, d, keys, ref, cli, by_uid):
    """Bulk records against the single-query calls, one by one."""
    for h, k in zip(hits, keys):
        one = (mt.get_segment_by_uid(d, int(k), ref, cli, text_cap=1) if by_uid
               else mt.get_containing_segment(d, int(k), ref, cli, text_cap=1))
        where = (d, int(k), ref, cli, by_uid)
        if one is None:
            assert h["row"] == -1, (where, h)
            continue
        assert tuple(int(h[x]) for x in FIELDS) == tuple(int(one[x]) for x in FIELDS), (where, h, one)
        assert h["local_position"] == mt.get_segment_by_uid(d, int(h["uid"]), text_cap=1)["position"], where


def _edge_positions(t):
    """First and last position of every visible row (so of every page and every 64-row chunk),
    and the ends of the document."""
    length = int(t["end"][-1]) if len(t["end"]) else 0
    vis = t["end"] > t["position"]
    pos = np.concatenate([t["position"][vis], t["end"][vis] - 1, [0, length - 1, length, length + 1]])
    return np.unique(pos[pos >= 0]).astype(np.int32), length


# ---------------------------------------------------------------- 2. edges
@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["lds", "hbm"])
def test_bulk_segments_flat_chunk_edges(tier):
    """Flat documents of 63, 64, 65, 128 and 129 rows built by hand (one seed segment, then
    inserts at the front by two writers; two rows removed whole): every position from 0 to
    length + 1 in the observer view, a sample in a remote view and every uid equal the
    single-query calls / the row table."""
    from fluidframework_amd.wire import Batch, Interner
    sizes = [63, 64, 65, 128, 129]
    b = Batch(Interner(synthetic=True))
    for n in sizes:
        msgs, seq = [], 0
        for k in range(n - 1):
            seq += 1
            msgs.append(dict(clientId=f"client-{1 + k % 2}", sequenceNumber=seq, referenceSequenceNumber=seq - 1,
                             minimumSequenceNumber=0, type="op",
                             contents={"type": 0, "pos1": 0, "seg": {"text": "abc"[: 1 + k % 3]}}))
        # rows in document order: the inserts, latest first, then the seed; remove row 0 and then
        # row 5 whole (no split: the row count stays n)
        lens = [1 + k % 3 for k in reversed(range(n - 1))] + [2]
        for lo, hi in ((0, lens[0]), (sum(lens[1:5]), sum(lens[1:6]))):
            seq += 1
            msgs.append(dict(clientId="client-1", sequenceNumber=seq, referenceSequenceNumber=seq - 1,
                             minimumSequenceNumber=0, type="op", contents={"type": 1, "pos1": lo, "pos2": hi}))
        b.add_doc("zz", msgs)
    a = b.arrays()
    mt = _batch(len(sizes), **TIERS[tier])
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    assert (mt.status() == 0).all()
    rng = np.random.default_rng(3)
    for d, n in enumerate(sizes):
        t = _table(mt, d)
        assert len(t["length"]) == n and not mt.is_paged(d) and (t["removed_seq"] != NONE).sum() == 2
        length = int(t["end"][-1])
        assert length == mt.get_length(d)
        pos = np.arange(0, length + 2, dtype=np.int32)
        hits = mt.locate_segments([d] * len(pos), pos)
        _check_observer_table(hits, t, pos=pos)
        sample = np.unique(np.concatenate([rng.integers(0, length, 12), [0, length - 1, length, length + 1]]))
        _check_single(mt, hits[sample], d, pos[sample], 0, 0, False)
        uids = np.concatenate([t["uid"], [0xFFFFFFF]])
        _check_observer_table(mt.locate_uids([d] * len(uids), uids), t, uids=uids)
        # a writer's view half-way through the stream: the later rows of the other writer are not in it
        ref = t["cur_seq"] // 2
        rhits = mt.locate_segments([d] * len(sample), pos[sample], ref, 1)
        _check_single(mt, rhits, d, pos[sample], ref, 1, False)
        ru = mt.locate_uids([d] * 8, uids[::max(len(uids) // 8, 1)][:8], ref, 2)
        _check_single(mt, ru, d, uids[::max(len(uids) // 8, 1)][:8], ref, 2, True)


@pytest.mark.gpu
def test_bulk_segments_paged_page_edges():
    """ref_c3_full in the paged layout (more than 64 pages per document: the page skip's
    directory chunk): the first and last position of every visible row -- so of every page and
    every 64-row chunk -- with length - 1, length and length + 1, and every uid, a gone one and
    one above the uid map's size, equal the row table; a sample equals the single-query calls."""
    fx, mt = _replay("ref_c3_full", "paged")
    assert (mt.status() == 0).all()
    rng = np.random.default_rng(17)
    for d in range(len(fx["docs"])):
        t = _table(mt, d)
        assert mt.is_paged(d) and t["pages"] > 64, t["pages"]
        pos, length = _edge_positions(t)
        assert length == fx["docs"][d]["out"]["length"]
        hits = mt.locate_segments([d] * len(pos), pos)
        _check_observer_table(hits, t, pos=pos)
        # ids stay below the uid map's size on a paged document (renumbered before they reach
        # it): an id above it walks the rows and reads as gone, like one that left the tree
        uids = np.concatenate([t["uid"], [0xFFFFFFF, (1 << 24) + 5]])
        by_uid = mt.locate_uids([d] * len(uids), uids)
        _check_observer_table(by_uid, t, uids=uids)
        if d == 0:
            sample = np.concatenate([rng.integers(0, len(pos), 20), [len(pos) - 3, len(pos) - 2, len(pos) - 1]])
            _check_single(mt, hits[sample], d, pos[sample], 0, 0, False)
            us = np.concatenate([rng.integers(0, len(uids), 10), [len(uids) - 2, len(uids) - 1]])
            _check_single(mt, by_uid[us], d, uids[us], 0, 0, True)
            ref = (t["min_seq"] + t["cur_seq"]) // 2
            rh = mt.locate_segments([d] * len(sample), pos[sample], ref, 2)
            _check_single(mt, rh, d, pos[sample], ref, 2, False)


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["lds", "paged"])
def test_bulk_segments_empty_documents_markers_and_removed_rows(tier):
    """ref_zam_shrink (a document emptied to length 0: position 0 finds no segment) and ref_ext
    (markers; removed rows, of view length 0, found by uid): every position and every uid."""
    for name in ("ref_zam_shrink", "ref_ext"):
        fx, mt = _replay(name, tier)
        assert (mt.status() == 0).all()
        markers = gone = empty = 0
        for d, doc in enumerate(fx["docs"]):
            t = _table(mt, d)
            length = doc["out"]["length"]
            pos = np.arange(0, length + 2, dtype=np.int32)
            hits = mt.locate_segments([d] * len(pos), pos)
            _check_observer_table(hits, t, pos=pos)
            by_uid = mt.locate_uids([d] * len(t["uid"]), t["uid"])
            _check_observer_table(by_uid, t, uids=t["uid"])
            markers += int((hits["marker_ref_type"][hits["row"] >= 0] >= 0).sum())
            gone += int((by_uid["removed_seq"] != NONE).sum())
            if length == 0:
                empty += 1
                assert hits["row"].tolist() == [-1, -1]
                assert mt.get_containing_segment(d, 0) is None
                assert mt.resolve_remote_positions([d, d], [0, 1], 0, 0).tolist() == [0, -1]
            sample = pos[:: max(len(pos) // 6, 1)]
            _check_single(mt, mt.locate_segments([d] * len(sample), sample), d, sample, 0, 0, False)
        if name == "ref_zam_shrink":
            assert empty >= 1
        else:
            assert markers > 0 and gone > 0


# ---------------------------------------------------------------- 3. page skip on == off
@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["paged", "grow", "hm"])
def test_bulk_segments_page_skip_equals_row_walk(tier, monkeypatch):
    """Observer view, by position and by uid: the records with the page skip (directory prefix
    sums of PageMeta.obs, the uid map as a hint) equal those of the plain row walk
    (MT_LOCATE_ROW_WALK=1), record for record; the directory's obs sum equals get_length."""
    fx, mt = _replay("ref_c3_full", tier)
    assert (mt.status() == 0).all()
    n = len(fx["docs"])
    assert all(mt.is_paged(d) for d in range(n))
    if tier == "grow":
        assert mt.last_grown()["in_big_region"] == n
    docs, pos, udocs, uids = [], [], [], []
    for d in range(n):
        t = _table(mt, d)
        p, _ = _edge_positions(t)
        docs += [d] * len(p)
        pos += p.tolist()
        udocs += [d] * (len(t["uid"]) + 1)
        uids += t["uid"].tolist() + [0xFFFFFFF]
    res = {}
    for walk in ("0", "1"):
        monkeypatch.setenv("MT_LOCATE_ROW_WALK", walk)
        res[walk] = (mt.locate_segments(docs, pos), mt.locate_uids(udocs, uids),
                     mt.get_view_lengths_bulk(np.arange(n)), mt.resolve_remote_positions(docs, pos, 0, 0))
    for on, off in zip(res["0"], res["1"]):
        assert np.array_equal(on, off)
    assert (res["0"][0]["row"] >= 0).sum() > 64 * n and (res["0"][1]["row"] < 0).sum() == n
    # (skip on: the observer length is the sum of the directory's PageMeta.obs)
    assert res["0"][2].tolist() == [mt.get_length(d) for d in range(n)] == [d["out"]["length"] for d in fx["docs"]]


# ---------------------------------------------------------------- 4. live handle
def _msg(ev):
    _, cid, seq, ref, msn, op = ev
    return dict(clientId=cid, sequenceNumber=seq, referenceSequenceNumber=ref, minimumSequenceNumber=msn,
                type="op", contents=op)


@pytest.mark.gpu
def test_bulk_segments_live_handle():
    """ref_live replayed through LiveClient up to its reconnects (unacked inserts and pending
    removes exist): every row by uid and a set of positions, in the local view and in a remote
    writer's, equal the single-query calls -- unassigned seq / removed_seq read -1 in both."""
    from fluidframework_amd.live import LiveClient
    from fluidframework_amd.wire import Interner
    doc = gu.load("ref_live")["docs"][0]
    lc = LiveClient(doc["seed_text"], interner=Interner(synthetic=True), seg_capacity=16384, text_capacity=1 << 17)
    lc.startOrUpdateCollaboration("local-0")
    unseq, checked, unassigned = [], 0, 0
    for ev in doc["events"]:
        if ev[0] == "L":
            op = ev[1]
            if op["type"] == 0:
                lc.insertSegmentLocal(op["pos1"], op["seg"])
            elif op["type"] == 1:
                lc.removeRangeLocal(op["pos1"], op["pos2"])
            else:
                lc.annotateRangeLocal(op["pos1"], op["pos2"], op["props"], op.get("combiningOp"))
            unseq.append(op)
        elif ev[0] == "M":
            if ev[1] == lc.long_client_id:
                unseq.pop(0)
            lc.applyMsg(_msg(ev))
        else:
            lc.flush()
            if checked < 2 and lc.pendingCounts()[1] > 0:
                mt = lc.mt
                t = _table(mt, 0)
                length = int(t["end"][-1])
                uids = t["uid"][:: max(len(t["uid"]) // 40, 1)]
                pend = t["uid"][(t["seq"] == -1) | (t["removed_seq"] == -1)][:12]
                uids = np.unique(np.concatenate([uids, pend])).astype(np.uint32)
                by_uid = mt.locate_uids([0] * len(t["uid"]), t["uid"])
                _check_observer_table(by_uid, t, uids=t["uid"])
                unassigned += int(((by_uid["seq"] == -1) | (by_uid["removed_seq"] == -1)).sum())
                pos = np.unique(np.concatenate([np.linspace(0, length, 12).astype(np.int32), [length - 1, length + 1]]))
                for ref, cli in ((0, 0), (t["cur_seq"], 1)):
                    _check_single(mt, mt.locate_uids([0] * len(uids), uids, ref, cli), 0, uids, ref, cli, True)
                    _check_single(mt, mt.locate_segments([0] * len(pos), pos, ref, cli), 0, pos, ref, cli, False)
                checked += 1
            lc.startOrUpdateCollaboration(ev[1])
            unseq = [lc.regeneratePendingOp(o) for o in unseq]
    assert checked > 0 and unassigned > 0


# ---------------------------------------------------------------- 5. failed and snapshot-loaded documents
def _check_against_single(mt, d, rng, remote_client=1):
    t = _table(mt, d)
    length = int(t["end"][-1]) if len(t["end"]) else 0
    pos = np.unique(np.concatenate([rng.integers(0, max(length, 1), 6), [0, max(length - 1, 0), length, length + 1]]))
    pos = pos.astype(np.int32)
    uids = np.concatenate([t["uid"][:: max(len(t["uid"]) // 6, 1)], [0xFFFFFFF]]).astype(np.uint32)
    _check_observer_table(mt.locate_segments([d] * len(pos), pos), t, pos=pos)
    _check_observer_table(mt.locate_uids([d] * len(t["uid"]), t["uid"]), t, uids=t["uid"])
    for ref, cli in ((0, 0), (t["cur_seq"], remote_client), (t["min_seq"], remote_client)):
        _check_single(mt, mt.locate_segments([d] * len(pos), pos, ref, cli), d, pos, ref, cli, False)
        _check_single(mt, mt.locate_uids([d] * len(uids), uids, ref, cli), d, uids, ref, cli, True)
    views = [(t["cur_seq"], remote_client), (t["min_seq"], remote_client), (0, 0)]
    assert mt.get_view_lengths_bulk([d] * 3, [r for r, _ in views], [c for _, c in views]).tolist() == \
        mt.get_view_lengths([d] * 3, [r for r, _ in views], [c for _, c in views]).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["lds", "paged"])
def test_bulk_segments_failed_documents_answer_from_where_they_stopped(tier):
    fx, mt = _replay("ref_errors", tier)
    st = mt.status()
    assert (st != 0).any()
    rng = np.random.default_rng(23)
    for d in np.flatnonzero(st != 0)[:6]:
        _check_against_single(mt, int(d), rng)
        assert mt.get_view_lengths_bulk([int(d)]).tolist() == [mt.get_length(int(d))]


@pytest.mark.gpu
def test_bulk_segments_snapshot_loaded_handle():
    """ref_snap loaded as summaries (large headers paged at load), then the tail."""
    fx = gu.load("ref_snap")
    docs = fx["docs"]
    la, oa = gu.encode_snap_docs(fx, gu.Interner(), docs)
    mt = _batch(len(docs), **PAGED_LOAD)
    mt.load_snapshots(la)
    st = mt.status()
    assert any(mt.is_paged(i) for i in range(len(docs)) if st[i] == 0)
    rng = np.random.default_rng(29)
    for step in range(2):
        for d in [i for i in range(len(docs)) if not gu.snap_status(docs[i])][:4]:
            _check_against_single(mt, d, rng)
        if step == 0:
            mt.apply_arrays(oa)
    ok = [i for i, d in enumerate(docs) if not gu.snap_status(d)]
    assert mt.get_view_lengths_bulk(ok).tolist() == [docs[i]["out"]["length"] for i in ok]


# ---------------------------------------------------------------- 6. arguments
@pytest.mark.gpu
def test_bulk_segments_arguments():
    """doc >= n_docs, pos < 0 and a remote refSeq of minSeq - 1 raise (and name the query); n = 0
    works; one document queried 1000 times; NULL ref_seq / client are the observer view."""
    from fluidframework_amd import _native
    fx, mt = _replay("ref_readouts", "paged")
    n = len(fx["docs"])
    with pytest.raises(RuntimeError):
        mt.locate_segments([0, n], [0, 0])
    with pytest.raises(RuntimeError):
        mt.locate_uids([n], [1])
    with pytest.raises(RuntimeError):
        mt.get_view_lengths_bulk([n])
    with pytest.raises(RuntimeError):
        mt.locate_segments([0, 1], [3, -1])
    with pytest.raises(RuntimeError):
        mt.resolve_remote_positions([0], [-1], 0, 0)
    low = int(fx["docs"][1]["minSeq"]) - 1
    for call in (lambda: mt.locate_segments([0, 1], [0, 0], [int(fx["docs"][0]["minSeq"]), low], [1, 1]),
                 lambda: mt.locate_uids([0, 1], [1, 1], [int(fx["docs"][0]["minSeq"]), low], [1, 1]),
                 lambda: mt.get_view_lengths_bulk([1], [low], [1]),
                 lambda: mt.get_view_lengths_bulk([1], [int(fx["docs"][1]["currentSeq"]) + 1], [1]),
                 lambda: mt.resolve_remote_positions([1], [0], [low], [1])):
        with pytest.raises(RuntimeError, match="collab window"):
            call()
    with pytest.raises(RuntimeError, match="query 1"):
        mt.locate_segments([0, 1], [0, 0], [int(fx["docs"][0]["minSeq"]), low], [1, 1])
    # client 0 is the observer view whatever the refSeq
    assert mt.get_view_lengths_bulk([1], [low], [0]).tolist() == [mt.get_length(1)]
    # n = 0
    assert len(mt.locate_segments([], [])) == 0 and len(mt.locate_uids([], [])) == 0
    assert len(mt.get_view_lengths_bulk([])) == 0 and len(mt.resolve_remote_positions([], [], [], [])) == 0
    assert mt.last_locate()[:2] == (0, 0)
    # one document 1000 times
    length = mt.get_length(2)
    pos = (np.arange(1000, dtype=np.int32) * 7) % (length + 2)
    t = _table(mt, 2)
    hits = mt.locate_segments([2] * 1000, pos)
    _check_observer_table(hits, t, pos=pos)
    assert mt.last_locate()[:2] == (1000, 0)
    # NULL ref_seq / client: the observer view; docs NULL: documents 0..n-1
    lib, h = mt.lib, mt.h
    out = np.zeros(n, dtype=_native.SEG_HIT_DTYPE)
    p3 = np.full(n, 3, dtype=np.int32)
    assert lib.mt_locate_segments(h, n, None, _native.ptr(p3), None, None, _native.ptr(out)) == 0
    assert np.array_equal(out, mt.locate_segments(np.arange(n), p3, 0, 0))
    assert lib.mt_locate_segments(h, n + 1, None, _native.ptr(p3), None, None, _native.ptr(out)) == _native.MT_E_INVALID
    zeros = np.zeros(n, dtype=np.int32)
    assert lib.mt_locate_segments(h, n, None, _native.ptr(p3), _native.ptr(zeros), None, _native.ptr(out)) == \
        _native.MT_E_INVALID   # (ref_seq and client come together)
    lens = np.zeros(n, dtype=np.int32)
    assert lib.mt_get_view_lengths_bulk(h, n, None, None, None, _native.ptr(lens)) == 0
    assert lens.tolist() == [mt.get_length(d) for d in range(n)]


# ---------------------------------------------------------------- 7. device variant
@pytest.mark.gpu
def test_bulk_segments_device_variant_equals_host_variant():
    """Every containing query of ref_readouts (host-path ones included) and the uids found."""
    from fluidframework_amd import _native
    fx, q, _ = _fixture_cursors("ref_readouts")
    _, mt = _replay("ref_readouts", "paged")
    hits = mt.locate_segments(q["doc"], q["pos"], q["ref"], q["cli"])
    assert (hits["flags"] & HOST).sum() == HOST_PATH["ref_readouts"][0]
    dev = mt.locate_segments_device(q["doc"], q["pos"], q["ref"], q["cli"])
    assert dev.is_cuda and dev.dtype == torch.int32 and tuple(dev.shape) == (len(hits), 12)
    assert mt.last_locate()[:2] == (len(hits), HOST_PATH["ref_readouts"][0])
    assert np.array_equal(dev.cpu().numpy().view(_native.SEG_HIT_DTYPE).reshape(-1), hits)
    f = hits["row"] >= 0
    by_uid = mt.locate_uids(q["doc"][f], hits["uid"][f], q["ref"][f], q["cli"][f])
    dev = mt.locate_segments_device(q["doc"][f], uids=hits["uid"][f], ref_seq=q["ref"][f], client=q["cli"][f])
    assert np.array_equal(dev.cpu().numpy().view(_native.SEG_HIT_DTYPE).reshape(-1), by_uid)
    obs = mt.locate_segments_device(np.arange(len(fx["docs"])), 5)
    assert np.array_equal(obs.cpu().numpy().view(_native.SEG_HIT_DTYPE).reshape(-1),
                          mt.locate_segments(np.arange(len(fx["docs"])), 5))


# ---------------------------------------------------------------- 8. Node facade
@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_bulk_segments_node_facade():
    """GpuMergeTreeBatch.getContainingSegments / getPositions and
    GpuClient.resolveRemoteClientPosition on ref_readouts equal the reference; undefined where
    the reference returns none."""
    from fluidframework_amd import build
    build.build()
    build.build_snapdec()
    build.build_node_addon()
    fx, q, _ = _fixture_cursors("ref_readouts")
    out = subprocess.run(["node", os.path.join(REPO, "tests", "js", "bulk_segments_tool.js"),
                          os.path.join(gu.GOLDEN, "ref_readouts.json.gz")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)
    f = q["found"]
    cont = got["containing"]
    assert len(cont) == len(f)
    assert [c is not None for c in cont] == f.tolist()
    for k, want in (("offset", "offset"), ("position", "vpos"), ("localPosition", "lpos"), ("length", "length")):
        assert [c[k] for c in cont if c is not None] == q[want][f].tolist(), k
    assert [c["hostPath"] for c in cont if c is not None] == q["host"][f].tolist()
    assert [(-1 if c["markerRefType"] is None else c["markerRefType"]) for c in cont if c is not None] == \
        q["marker"][f].tolist()
    assert [p["position"] for p in got["positions"]] == q["vpos"][f].tolist()
    assert [p["localPosition"] for p in got["positions"]] == q["lpos"][f].tolist()
    assert got["gone"] == [None]
    want = np.where(f, q["lpos"] + q["offset"], np.where(q["pos"] == q["view_n"], q["obs_len"], -1))
    assert got["resolved"] == [None if w < 0 else int(w) for w in want]
    assert got["beyond"] == [None, None]


# ---------------------------------------------------------------- 9. the C ABI (no GPU)
def test_bulk_segments_symbols_exported_and_bound():
    """The built library exports the new symbols and _native.SIGNATURES binds them with the
    header's argument lists; the record is 48 bytes."""
    import ctypes
    from fluidframework_amd import build, _native
    build.build()
    lib = _native.load()
    P, U32, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    want = {
        "mt_locate_segments": [P, U32, P, P, P, P, P],
        "mt_locate_uids": [P, U32, P, P, P, P, P],
        "mt_locate_segments_device": [P, U32, P, P, P, P, P],
        "mt_locate_uids_device": [P, U32, P, P, P, P, P],
        "mt_get_view_lengths_bulk": [P, U32, P, P, P, P],
        "mt_resolve_remote_positions": [P, U32, P, P, P, P, P],
        "mt_last_locate": [P, P, P],
    }
    sigs = {s[0]: s for s in _native.SIGNATURES}
    for name, args in want.items():
        assert hasattr(lib, name), name
        assert name in sigs, name
        assert sigs[name][1] is I and list(sigs[name][2]) == args, name
        assert getattr(lib, name).argtypes == args
    assert _native.SEG_HIT_DTYPE.itemsize == 48
    assert _native.SEG_HIT_DTYPE.names == ("row", "uid", "position", "offset", "local_position", "length", "seq",
                                           "client", "removed_seq", "removed_client", "marker_ref_type", "flags")
