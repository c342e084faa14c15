"""Bulk marker queries on the device (mt_find_tiles / mt_find_markers_by_id,
MergeTreeBatch.find_tiles / find_tiles_device / find_markers_by_id / last_tiles):
SharedString.findTile and getMarkerFromId for many (doc, pos, label, direction) / (doc, id)
queries in one launch.

Expected values are the reference's own (tests/golden/ref_tiles.json.gz, made by
tests/golden/make_tiles.py from the streams of tests/tile_streams.py: at every checkpoint the
segment table, Client.findTile for a query list and getMarkerFromId for every id inserted).
tests/tile_util.py restates the rule over rows; test 1 pins the restatement on the reference, the
generated-batch test uses it where no fixture holds the answers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch   # before the replay library loads: both then share one HIP runtime (as in bench.py)

import golden_util as gu
import tile_streams
import tile_util

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = -(1 << 31)          # MT_RSEQ_NONE
DUP = 2                    # MT_MARK_DUP
LABELS = tile_streams.LABELS

# the storage tiers of tests/test_bulk_segments.py, copied
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

_fx = {}


def _fixture():
    if not _fx:
        _fx["fx"] = gu.load("ref_tiles")
    return _fx["fx"]


def _rows(cp):
    return [(ln, bool(rm), rt, props) for ln, rm, rt, props in cp["segs"]]


def _page_of(cp):
    out = []
    for p, n in enumerate(cp["pages"]):
        out += [p] * n
    return out


# ---------------------------------------------------------------- 1. the rule, on the reference
def test_tile_rule_equals_the_reference_and_the_fixture_holds_every_class():
    """tile_util over the reference's own segment tables equals every recorded findTile and
    getMarkerFromId answer, at every checkpoint; and the fixture holds the classes the device
    tests rely on (asserted, so that none is silently absent)."""
    fx = _fixture()
    assert fx["labels"] == LABELS
    assert [d["msgs"] for d in fx["docs"]] == [log["msgs"] for log in tile_streams.logs()]
    own = away = nothing = edge_hit = edge_miss = present = gone = 0
    flat = paged = emptied = chunked = 0
    kinds = set()
    for d in fx["docs"]:
        for cp in d["checkpoints"]:
            rows = _rows(cp)
            assert sum(cp["leaves"]) == sum(cp["pages"]) == len(rows)
            obs = [0 if r[1] else r[0] for r in rows]
            assert sum(obs) == cp["length"]
            ends = np.cumsum(obs)
            page = _page_of(cp)
            n_pages = len(cp["pages"])
            flat += 10 <= len(rows) <= 60
            paged += 3 <= n_pages <= 30
            chunked += n_pages >= 70
            emptied += cp["length"] == 0 and len(rows) > 0
            for r in rows:
                if r[2] is not None:
                    labels = (r[3] or {}).get(tile_util.TILE_KEY)
                    kinds.add((r[2] & 1, json.dumps(labels), tile_util.ID_KEY in (r[3] or {}), r[1]))
            for pos, lab, prec, row, tpos in cp["tiles"]:
                got = tile_util.find_tile(rows, pos, LABELS[lab], bool(prec))
                assert (got or (-1, -1)) == (row, tpos), (d["doc"], cp["n"], pos, LABELS[lab], prec, got, row, tpos)
                if row < 0:
                    nothing += 1
                elif pos is not None and pos < cp["length"]:
                    hit = int(np.searchsorted(ends, pos, side="right"))
                    if page[hit] == page[row]:
                        own += 1
                    else:
                        away += 1
                if not prec and pos == cp["length"] and rows:
                    if rows[-1][1] and tile_util.qualifies(rows[-1], LABELS[lab]):
                        edge_hit += 1
                        assert row == len(rows) - 1 and tpos == cp["length"]
                    else:
                        edge_miss += 1
            ids = [i for i, _, _, _ in cp["ids"]]
            assert len(set(ids)) == len(ids)                                    # no duplicate ids
            for mid, row, linked, found in cp["ids"]:
                assert found == 1                                               # the map is never erased
                got = tile_util.marker_from_id(rows, mid)
                # the first deviation: a marker zamboni has unlinked reads as gone here
                assert (row >= 0) == bool(linked), (d["doc"], mid)
                assert (got[0] if got else -1) == row and not (got and got[2]), (d["doc"], cp["n"], mid, got, row)
                if row < 0:
                    gone += 1
                elif rows[row][1]:
                    present += 1
    assert min(own, away, nothing) >= 50, (own, away, nothing)
    assert edge_hit >= 10 and edge_miss >= 10, (edge_hit, edge_miss)
    assert present >= 10 and gone >= 10, (present, gone)
    assert flat >= 8 and paged >= 4 and chunked >= 1 and emptied >= 2, (flat, paged, chunked, emptied)
    # two labels in lists, both at once, a string value, labels without the Tile bit, an id and no
    # labels, removed markers that qualify
    want = [(1, '["pg"]'), (1, '["cell"]'), (1, '["pg", "cell"]'), (1, '"pg"'), (0, '["pg"]'), (1, "null"), (1, "[]")]
    for tile_bit, labels in want:
        assert any(k[0] == tile_bit and k[1] == labels for k in kinds), (tile_bit, labels)
    assert any(k[1] == "null" and k[2] for k in kinds) and any(k[0] and k[1] == '["pg"]' and k[3] for k in kinds)


# ---------------------------------------------------------------- helpers of the device tests
def _batch(n_docs, **kw):
    from fluidframework_amd import MergeTreeBatch
    kw.setdefault("seg_capacity", 8192)
    kw.setdefault("text_capacity", 1 << 17)
    return MergeTreeBatch(n_docs, **kw)


def _cuts(doc, k):
    """k message counts, ascending, the last one the whole log, holding the document's
    checkpoints (gu.batches_to wants as many cuts for every document)."""
    cps = [cp["n"] for cp in doc["checkpoints"]]
    cuts = set(cps)
    fill = (n for n in range(1, len(doc["msgs"])) if n not in cuts)
    while len(cuts) < k:
        cuts.add(next(fill))
    return sorted(cuts)


def _replay_slices(tier, **kw):
    """The fixture replayed on a tier in slices that end at the checkpoints: yields (mt, interner,
    [(doc index, checkpoint)] reached by the slice just applied)."""
    fx = _fixture()
    docs = fx["docs"]
    interner = gu.Interner()
    a = gu.encode_docs(fx, interner)
    k = max(len(d["checkpoints"]) for d in docs)
    cuts = [_cuts(d, k) for d in docs]
    mt = _batch(len(docs), **dict(TIERS[tier], **kw))
    mt.load_initial_text(a["seed_off"], a["seed"])
    for j, part in enumerate(gu.batches_to(a, docs, cuts)):
        mt.apply_arrays(part)
        assert (mt.status() == 0).all()
        at = [(i, cp) for i, d in enumerate(docs) for cp in d["checkpoints"] if cp["n"] == cuts[i][j]]
        yield mt, interner, at


def _tile_queries(at):
    q = dict(doc=[], pos=[], label=[], prec=[], row=[], tpos=[])
    for i, cp in at:
        for pos, lab, prec, row, tpos in cp["tiles"]:
            q["doc"].append(i), q["pos"].append(pos), q["label"].append(LABELS[lab]), q["prec"].append(prec)
            q["row"].append(row), q["tpos"].append(tpos)
    return q


def _id_queries(at):
    q = dict(doc=[], id=[], row=[])
    for i, cp in at:
        for mid, row, _, _ in cp["ids"]:
            q["doc"].append(i), q["id"].append(mid), q["row"].append(row)
    return q


def _table(mt, d):
    """Document d's rows as the record's fields: get_segments' columns, the ids of the raw
    records and every row's observer position."""
    seg, _ = mt.get_segments(d)
    raw, hdr = mt.debug_raw(d)
    assert len(seg) == len(raw)
    vis = np.where(seg[:, 3] == NONE, seg[:, 0], 0)
    return dict(length=seg[:, 0], seq=seg[:, 1], client=seg[:, 2], removed_seq=seg[:, 3],
                removed_client=seg[:, 4], marker_ref_type=seg[:, 6], uid=raw[:, 6] & 0x7FFFFFFF,
                position=np.cumsum(vis) - vis, pages=int(hdr[25]), paged=bool(hdr[24]))


def _check_hits(mt, hits, docs, rows, positions=None, tables=None):
    """Records against the expected rows: row -1 records are empty; the others carry every field
    of get_segments' row, the marker's observer position twice and offset 0."""
    tables = {} if tables is None else tables
    rows = np.asarray(rows)
    bad = np.flatnonzero(hits["row"] != rows)
    assert len(bad) == 0, (bad[:5], hits[bad[:5]], rows[bad[:5]])
    none = hits[rows < 0]
    assert not any(none[k].any() for k in none.dtype.names if k != "row")
    for d in sorted(set(np.asarray(docs)[rows >= 0].tolist())):
        if d not in tables:
            tables[d] = _table(mt, d)
        t = tables[d]
        m = (np.asarray(docs) == d) & (rows >= 0)
        r = rows[m]
        for k in ("length", "seq", "client", "removed_seq", "removed_client", "marker_ref_type", "uid", "position"):
            assert np.array_equal(hits[k][m], t[k][r]), (d, k)
        assert np.array_equal(hits["local_position"][m], t["position"][r]) and not hits["offset"][m].any()
        assert (hits["marker_ref_type"][m] >= 0).all()
    if positions is not None:
        f = rows >= 0
        assert np.array_equal(hits["position"][f], np.asarray(positions)[f])
    return tables


# ---------------------------------------------------------------- 2. reference parity
@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["lds", "hbm", "paged", "tight", "narrow", "grow", "hm"])
def test_bulk_tiles_match_reference(tier):
    """The fixture replayed in slices that end at its checkpoints: at every checkpoint one
    find_tiles call for all its findTile queries and one find_markers_by_id call for all its ids
    equal the reference, and every field of a record is its row's."""
    final = 0
    for mt, interner, at in _replay_slices(tier):
        q = _tile_queries(at)
        hits = mt.find_tiles(q["doc"], q["pos"], q["label"], q["prec"], interner=interner)
        queries, examined, ms = mt.last_tiles()
        assert queries == len(q["doc"]) and examined > 0 and ms > 0
        assert not hits["flags"].any()
        tables = _check_hits(mt, hits, q["doc"], q["row"], q["tpos"])
        ids = _id_queries(at)
        by_id = mt.find_markers_by_id(ids["doc"], ids["id"], interner=interner)
        assert not by_id["flags"].any()            # (unique ids: no MT_MARK_DUP)
        _check_hits(mt, by_id, ids["doc"], ids["row"], tables=tables)
        assert mt.last_tiles()[0] == len(ids["doc"])
        final = at
    fx = _fixture()
    assert len(final) == len(fx["docs"])           # the last slice ends every document
    big = next(i for i, d in enumerate(fx["docs"]) if d["doc"] == "big0")
    t = _table(mt, big)
    if tier in ("paged", "hm", "tight", "narrow", "grow"):
        assert t["paged"] and t["pages"] > 64, t["pages"]   # the directory scan crosses a 64-position chunk
    if tier in ("lds", "hbm"):
        assert not t["paged"] and len(t["uid"]) > 64


def _final_queries(mt, interner, at):
    q = _tile_queries(at)
    return mt.find_tiles(q["doc"], q["pos"], q["label"], q["prec"], interner=interner)


@pytest.mark.gpu
def test_bulk_tiles_page_skip_equals_row_walk():
    """The final checkpoint's queries on the paged tier, in a child process that runs with
    MT_LOCATE_ROW_WALK=1 (the kernel walks from row 0), give the records of this process (H's
    page by the directory, then away from it page by page); the walk examines more rows."""
    for mt, interner, at in _replay_slices("paged"):
        pass
    hits = _final_queries(mt, interner, at)
    examined = mt.last_tiles()[1]
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "row-walk"], capture_output=True, text=True,
                         timeout=300, env=dict(os.environ, MT_LOCATE_ROW_WALK="1", PYTHONPATH=os.pathsep.join(
                             [REPO, os.path.join(REPO, "tests")] + os.environ.get("PYTHONPATH", "").split(os.pathsep))))
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got["walk"] == "1"
    walked = np.asarray(got["hits"], dtype=np.int64)
    mine = np.stack([hits[k].astype(np.int64) for k in hits.dtype.names], axis=1)
    assert np.array_equal(walked, mine)
    assert got["examined"] > examined > 0


def _row_walk_child():
    """(child process of the test above) the same replay and queries; prints the records."""
    for mt, interner, at in _replay_slices("paged"):
        pass
    hits = _final_queries(mt, interner, at)
    print(json.dumps(dict(walk=os.environ.get("MT_LOCATE_ROW_WALK"), examined=mt.last_tiles()[1],
                          hits=np.stack([hits[k].astype(np.int64) for k in hits.dtype.names], axis=1).tolist())))


# ---------------------------------------------------------------- 3. arguments
@pytest.mark.gpu
def test_bulk_tiles_arguments():
    """Documents repeated and permuted, docs NULL, n == 0, the device form, a label the interner
    never saw, every MT_E_INVALID case (the message names the query), and the handle still
    answering after each error."""
    from fluidframework_amd import _native
    for mt, interner, at in _replay_slices("paged"):
        pass
    fx = _fixture()
    n = len(fx["docs"])
    q = _tile_queries(at)
    want = mt.find_tiles(q["doc"], q["pos"], q["label"], q["prec"], interner=interner)
    assert (want["row"] >= 0).sum() > 100
    # permuted (documents repeat throughout the list already)
    perm = np.random.default_rng(5).permutation(len(q["doc"]))
    got = mt.find_tiles([q["doc"][i] for i in perm], [q["pos"][i] for i in perm], [q["label"][i] for i in perm],
                        [q["prec"][i] for i in perm], interner=interner)
    assert np.array_equal(got, want[perm])
    # the device form
    dev = mt.find_tiles_device(q["doc"], q["pos"], q["label"], q["prec"], interner=interner)
    assert dev.is_cuda and dev.dtype == torch.int32 and tuple(dev.shape) == (len(want), 12)
    assert np.array_equal(dev.cpu().numpy().view(_native.SEG_HIT_DTYPE).reshape(-1), want)
    assert mt.last_tiles()[0] == len(want)
    # docs None: documents 0..n-1; one label and one direction for all
    assert np.array_equal(mt.find_tiles(None, 3, "pg", interner=interner),
                          mt.find_tiles(np.arange(n), [3] * n, ["pg"] * n, [1] * n, interner=interner))
    assert np.array_equal(mt.find_tiles(None, None, "cell", False, interner=interner),
                          mt.find_tiles(np.arange(n), [None] * n, ["cell"] * n, [0] * n, interner=interner))
    # n == 0
    assert len(mt.find_tiles([], [], [], interner=interner)) == 0 and mt.last_tiles()[:2] == (0, 0)
    assert len(mt.find_markers_by_id([], [], interner=interner)) == 0
    # a label, an id and keys the interner never saw: no answer, no error
    assert (mt.find_tiles(None, 0, "never-seen", interner=interner)["row"] == -1).all()
    assert (mt.find_markers_by_id([0, 1], ["never-seen", ""], interner=interner)["row"] == -1).all()
    assert (mt.find_tiles(None, 0, "pg", interner=gu.Interner())["row"] == -1).all()
    assert (mt.find_markers_by_id([0], ["x"], interner=gu.Interner(synthetic=True))["row"] == -1).all()
    # the interner grows: the label table follows
    grown = "zz-grown"
    assert (mt.find_tiles(None, None, grown, interner=interner)["row"] == -1).all()
    interner.val([grown])
    assert mt._label_ids(interner, grown) == [len(interner.vals) - 1]
    # MT_E_INVALID, refused before any launch, naming the query; the handle answers afterwards
    lib, h = mt.lib, mt.h
    key = interner.key_ids["referenceTileLabels"]
    pg = np.asarray(mt._label_ids(interner, "pg"), dtype=np.uint32)
    assert len(pg) >= 2
    out = np.zeros(4, dtype=_native.SEG_HIT_DTYPE)

    def call(docs=(0, 1), pos=(0, 0), label=(0, 0), off=None, vals=None, n_labels=1):
        docs, pos = np.asarray(docs, dtype=np.uint32), np.asarray(pos, dtype=np.int32)
        label = np.asarray(label, dtype=np.uint32)
        off = np.asarray([0, len(pg)] if off is None else off, dtype=np.uint32)
        vals = np.asarray(pg if vals is None else vals, dtype=np.uint32)
        rc = lib.mt_find_tiles(h, len(docs), _native.ptr(docs), _native.ptr(pos), None, _native.ptr(label), key, n_labels,
                               _native.ptr(off), _native.ptr(vals), _native.ptr(out))
        return rc, lib.mt_last_error(h).decode()

    assert call()[0] == 0
    ok = out[:2].copy()
    assert np.array_equal(ok, mt.find_tiles([0, 1], 0, "pg", interner=interner))   # preceding NULL: all 1
    for kw, text in ((dict(pos=(0, -2)), "query 1"), (dict(label=(0, 1)), "query 1"), (dict(docs=(0, n)), "query 1"),
                     (dict(off=[0, 2, 1], n_labels=2), "monotonic"), (dict(off=[1, 2]), "offsets"),
                     (dict(vals=pg[::-1].copy()), "sorted"), (dict(vals=[pg[0], pg[0]], off=[0, 2]), "sorted"),
                     (dict(vals=[pg[0] | 0x80000000], off=[0, 1]), "flag"), (dict(vals=[pg[0] | 0x40000000], off=[0, 1]), "flag"),
                     (dict(vals=[0xFFFFFFFF], off=[0, 1]), "null"), (dict(vals=[0xFFFFFFFE], off=[0, 1]), "null")):
        rc, err = call(**kw)
        assert rc == _native.MT_E_INVALID and "mt_find_tiles" in err and text in err, (kw, rc, err)
        assert call()[0] == 0 and np.array_equal(out[:2], ok)
    with pytest.raises(RuntimeError, match="query 2"):
        mt.find_tiles([0, 1, n], 0, "pg", interner=interner)
    with pytest.raises(RuntimeError, match="query 0"):
        mt.find_markers_by_id([n], ["x"], interner=interner)
    # docs NULL with more queries than documents
    z = np.zeros(n + 1, dtype=np.uint32)
    assert lib.mt_find_tiles(h, n + 1, None, _native.ptr(z.view(np.int32)), None, _native.ptr(z), key, 1,
                             _native.ptr(np.asarray([0, len(pg)], dtype=np.uint32)), _native.ptr(pg),
                             _native.ptr(np.zeros(n + 1, dtype=_native.SEG_HIT_DTYPE))) == _native.MT_E_INVALID
    assert np.array_equal(mt.find_tiles(q["doc"], q["pos"], q["label"], q["prec"], interner=interner), want)


@pytest.mark.gpu
def test_bulk_tiles_live_handle_is_refused():
    from fluidframework_amd.live import LiveClient
    from fluidframework_amd.wire import Interner
    interner = Interner()
    lc = LiveClient("abc", interner=interner, seg_capacity=512, text_capacity=1 << 12)
    lc.startOrUpdateCollaboration("local-0")
    lc.flush()
    with pytest.raises(RuntimeError, match="not built for live handles"):
        lc.mt.find_tiles([0], [0], "pg", interner=interner)
    with pytest.raises(RuntimeError, match="not built for live handles"):
        lc.mt.find_markers_by_id([0], ["m"], interner=interner)
    assert lc.mt.locate_segments([0], [0])["row"].tolist() == [0]   # the handle goes on answering


def _handle_rows(mt, d, interner):
    """Document d's rows in tile_util's form, from get_segments and get_all_segment_props."""
    seg, _ = mt.get_segments(d)
    props = mt.get_all_segment_props(d)
    assert len(props) == len(seg)
    return [(int(s[0]), bool(s[3] != NONE), int(s[6]) if s[6] >= 0 else None,
             None if p is None else {interner.key_name(k): interner.val_value(v) for k, v in p})
            for s, p in zip(seg, props)]


def _check_against_util(mt, interner, docs, pos, labels, prec):
    hits = mt.find_tiles(docs, pos, labels, prec, interner=interner)
    rows = {d: _handle_rows(mt, d, interner) for d in set(docs)}
    want = [tile_util.find_tile(rows[d], p, s, bool(f)) or (-1, -1) for d, p, s, f in zip(docs, pos, labels, prec)]
    _check_hits(mt, hits, docs, [w[0] for w in want], [w[1] for w in want])
    return hits, rows


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["lds", "paged"])
def test_bulk_tiles_failed_documents_answer_from_where_they_stopped(tier):
    fx = gu.load("ref_errors")
    interner = gu.interner_for(fx)
    a = gu.encode_docs(fx, interner)
    mt = _batch(len(fx["docs"]), **TIERS[tier])
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    failed = np.flatnonzero(mt.status() != 0)[:6].tolist()
    assert failed
    docs, pos, labels, prec = [], [], [], []
    for d in failed:
        length = mt.get_length(d)
        for p in (0, length // 2, length, length + 1, None):
            for f in (1, 0):
                docs.append(d), pos.append(p), labels.append("pg"), prec.append(f)
    _check_against_util(mt, interner, docs, pos, labels, prec)
    assert (mt.find_markers_by_id(failed, ["m"] * len(failed), interner=interner)["row"] == -1).all()
    assert (mt.status() != 0).sum() >= len(failed)


# ---------------------------------------------------------------- 4. the independent check
@pytest.mark.gpu
def test_bulk_tiles_generated_batch_equals_host_scan():
    """64 generated marker documents (tile_streams, other seeds; the tight tier): the device
    answers equal tile_util over get_segments + get_all_segment_props of the same handle; ids by the same scan, duplicates included (one id inserted twice: the first row
    answers and the record carries MT_MARK_DUP)."""
    from fluidframework_amd.wire import Batch
    cfgs = [dict(name=f"gen{i}", seed=8800 + i, msgs=40 + 9 * i, lag=(16, 64, 700)[i % 3], p_marker=0.15, p_insert=0.55,
                 p_remove=0.25, text_max=6, seed_len=16, end=(None, "marker", "empty", "text")[i % 4], checkpoints=1)
            for i in range(64)]
    logs = [tile_streams.build(c) for c in cfgs]
    dup_id = "gen0-dup"
    for k in (0, 1):   # the same id on two markers of document 0
        _, seq, _, msn, _ = logs[0]["msgs"][-1]
        logs[0]["msgs"].append([1, seq + 1, seq, msn, {"pos1": k, "type": 0, "seg": {
            "marker": {"refType": 1}, "props": {"referenceTileLabels": ["pg"], "markerId": dup_id}}}])
    interner = gu.Interner()
    b = Batch(interner)
    for log in logs:
        b.add_doc(log["seed_text"], gu.compact_msgs_to_dicts(log["msgs"]))
    a = b.arrays()
    mt = _batch(64, **TIERS["tight"])
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    assert (mt.status() == 0).all()
    paged = sum(mt.is_paged(d) for d in range(64))
    assert paged >= 8, paged
    rng = np.random.default_rng(41)
    docs, pos, labels, prec = [], [], [], []
    for d in range(64):
        length = mt.get_length(d)
        ps = [None, 0, max(length - 1, 0), length, length + 1] + rng.integers(0, length + 1, 10).tolist()
        for p in ps:
            for s in LABELS:
                for f in (1, 0):
                    docs.append(d), pos.append(p), labels.append(s), prec.append(f)
    hits, rows = _check_against_util(mt, interner, docs, pos, labels, prec)
    assert (hits["row"] >= 0).sum() > 1000 and (hits["row"] < 0).sum() > 1000
    idocs, ids = [], []
    for d, log in enumerate(logs):
        for m in log["msgs"]:
            mid = (m[4].get("seg", {}).get("props") or {}).get("markerId") if isinstance(m[4].get("seg"), dict) else None
            if mid and mid != dup_id:
                idocs.append(d), ids.append(mid)
        idocs.append(d), ids.append(f"gen{d}-m0")   # never inserted
    by_id = mt.find_markers_by_id(idocs, ids, interner=interner)
    want = [tile_util.marker_from_id(rows[d], i) for d, i in zip(idocs, ids)]
    _check_hits(mt, by_id, idocs, [w[0] if w else -1 for w in want], [w[1] if w else -1 for w in want])
    assert not by_id["flags"].any() and (by_id["row"] >= 0).sum() > 50 and (by_id["row"] < 0).sum() >= 64
    assert (by_id["removed_seq"][by_id["row"] >= 0] != NONE).any()           # removed, still in the tree
    dup = mt.find_markers_by_id([0], [dup_id], interner=interner)
    w = tile_util.marker_from_id(rows[0], dup_id)
    assert w[2] and dup["row"][0] == w[0] and dup["flags"][0] == DUP and dup["position"][0] == w[1]


# ---------------------------------------------------------------- 5. the C ABI (no GPU)
def test_bulk_tiles_symbols_exported_and_bound():
    import ctypes
    from fluidframework_amd import build, _native
    build.build()
    lib = _native.load()
    P, U32, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    want = {"mt_find_tiles": [P, U32, P, P, P, P, U32, U32, P, P, P],
            "mt_find_tiles_device": [P, U32, P, P, P, P, U32, U32, P, P, P],
            "mt_find_markers_by_id": [P, U32, P, U32, P, P],
            "mt_find_markers_by_id_device": [P, U32, P, U32, P, P],
            "mt_last_tiles": [P, P, P]}
    sigs = {s[0]: s for s in _native.SIGNATURES}
    for name, args in want.items():
        assert hasattr(lib, name) and name in sigs, name
        assert sigs[name][1] is I and list(sigs[name][2]) == args, name
    assert _native.SEG_HIT_DTYPE.itemsize == 48 and _native.MT_MARK_DUP == 2


if __name__ == "__main__" and sys.argv[1:] == ["row-walk"]:
    _row_walk_child()
