"""Bulk and ranged property-run read-out on the device (mt_get_prop_runs_bulk /
mt_get_prop_runs_bulk_device, MergeTreeBatch.get_prop_runs_raw / get_prop_runs_bulk /
get_properties_at_positions / get_prop_runs_device, the Node facade's getPropertiesAtPositions /
getPropertyRuns): mt_get_prop_runs clipped to [start, end) for many (doc, start, end) queries in
one counting pass and one gather.

Every check has two parts.  (A) values: a result's runs, expanded to one property set per
position, equal the reference's `out.segs[*].props` at that position as sets of (key, value)
ids (sets on purpose: the fixtures hold adjacent segments whose equal property objects differ in
key order, which word-wise coalescing may or may not join).  (B) structure: the result equals
get_prop_runs(doc) clipped to [start, end) on the host -- the same rows and the same record
words -- and its records are packed back to back behind word_off."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch   # before the replay library loads: both then share one HIP runtime (as in bench.py)

import golden_util as gu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF   # a row's record: no properties
PAGE_SLOTS = 64     # MT_PG_SLOTS: segments a page holds at most (csrc/mt_device.h)
EMPTY = frozenset()


# ---------------------------------------------------------------- the host derivation
def _ids(props, interner):
    """A reference property object as a set of (key id, value id) words."""
    if not props:
        return EMPTY
    return frozenset((interner.key(k) & 0xFFFFFFFF, interner.val(gu.from_fixture(v)) & 0xFFFFFFFF)
                     for k, v in props.items())


def _ref_sets(out, interner):
    """The reference's property set at every position of the observer view."""
    sets = []
    for r in out["segs"]:
        if r["rseq"] is None:
            sets += [_ids(r["props"], interner)] * r["len"]
    assert len(sets) == out["length"]
    return sets


def _visible_rows(out):
    """[(position, length, is_marker)] of the reference's visible segment rows."""
    rows, pos = [], 0
    for r in out["segs"]:
        if r["rseq"] is None:
            rows.append((pos, r["len"], r["marker"] is not None))
            pos += r["len"]
    return rows


def _clamp(s, e, ln):
    e = ln if e is None or e < 0 else min(e, ln)
    s = min(max(0 if s is None else s, 0), ln)
    return s, max(e, s)


def _clip(runs, s, e, ln):
    """get_prop_runs(doc) rows clipped to [s, e) (clamped into [0, ln])."""
    s, e = _clamp(s, e, ln)
    out = []
    for p, l, pairs in runs:
        lo, hi = max(p, s), min(p + l, e)
        if hi > lo:
            out.append((lo, hi - lo, pairs))
    return out


def _decode(raw):
    """(run_off, word_off, runs, records) -> per query [(position, length, pairs | None)], with
    the packing checked: a query's records lie back to back in row order and fill its slot."""
    run_off, word_off, runs, recs = raw
    assert run_off[0] == 0 and word_off[0] == 0 and len(run_off) == len(word_off)
    assert run_off[-1] == len(runs) and word_off[-1] == len(recs)
    assert (np.diff(run_off) >= 0).all() and (np.diff(word_off) >= 0).all()
    rows, words = runs.tolist(), recs.tolist()
    out = []
    for q in range(len(run_off) - 1):
        w0, w1 = int(word_off[q]), int(word_off[q + 1])
        at, res = 0, []
        for p, l, r in rows[int(run_off[q]): int(run_off[q + 1])]:
            if r == NONE:
                res.append((p, l, None))
                continue
            assert r == at, (q, r, at)
            n = words[w0 + r]
            res.append((p, l, [(words[w0 + r + 1 + 2 * j], words[w0 + r + 2 + 2 * j]) for j in range(n)]))
            at += 1 + 2 * n
        assert at == w1 - w0, (q, at, w1 - w0)
        out.append(res)
    return out


class _Handle:
    """A replayed handle with what the checks compare against, computed once."""

    def __init__(self, mt, lengths, sets=None):
        self.mt = mt
        self.lengths = lengths      # per document: the observer length
        self.sets = sets            # per document: the reference's set per position (None: no (A))
        self._host = {}

    def host(self, d):
        if d not in self._host:
            self._host[d] = self.mt.get_prop_runs(d)
        return self._host[d]


def _check_queries(H, queries):
    """One get_prop_runs_raw call for queries [(doc, start, end)]: (A) and (B).  Returns the
    decoded results."""
    docs = np.array([q[0] for q in queries], dtype=np.uint32)
    start = np.array([q[1] for q in queries], dtype=np.int32)
    end = np.array([q[2] for q in queries], dtype=np.int32)
    got = _decode(H.mt.get_prop_runs_raw(docs, start, end))
    assert len(got) == len(queries)
    bad = []
    for q, (d, s, e) in enumerate(queries):
        ln = H.lengths[d]
        if got[q] != _clip(H.host(d), s, e, ln):                       # (B)
            bad.append(("B", q, d, s, e))
            continue
        if H.sets is None or H.sets.get(d) is None:
            continue
        cs, ce = _clamp(s, e, ln)
        at = cs
        for p, l, pairs in got[q]:                                      # (A)
            ok = p == at and l > 0 and len(set(pairs or [])) == len(pairs or [])
            if not ok or any(H.sets[d][x] != frozenset(pairs or []) for x in range(p, p + l)):
                bad.append(("A", q, d, s, e, p, l))
                break
            at = p + l
        else:
            if at != ce:
                bad.append(("A-cover", q, d, s, e, at, ce))
    assert not bad, bad[:6]
    return got


# ---------------------------------------------------------------- handles
def _gpu_batch(n_docs, **kw):
    """A handle for one storage tier, as tests/test_gpu_parity.py builds them."""
    from fluidframework_amd import MergeTreeBatch
    kw.setdefault("delta_log_capacity", 1 << 18)
    kw.setdefault("seg_capacity", 8192)
    kw.setdefault("text_capacity", 1 << 17)
    kw.setdefault("page_capacity", -1)
    return MergeTreeBatch(n_docs, **kw)


PAGED = dict(lds_seg_capacity=-1, page_capacity=256, unsettled_capacity=2048, page_heap_capacity=2048)
TIERS = {
    "lds": dict(lds_seg_capacity=0),
    "hbm": dict(lds_seg_capacity=-1),
    "tiny": dict(lds_seg_capacity=16),
    "paged": dict(PAGED),
    "tiny_paged": dict(PAGED, lds_seg_capacity=16),
    "tight": dict(PAGED, lds_seg_capacity=16, lds_page_capacity=24, lds_unsettled_capacity=40,
                  lds_page_heap_capacity=40),
    "grow": dict(lds_seg_capacity=16, page_capacity=12, unsettled_capacity=16, page_heap_capacity=16),
    "hm": dict(PAGED, page_capacity=600),
}
PAGED_LOAD = dict(seg_capacity=48, lds_seg_capacity=16, props_capacity=4096, page_capacity=256,
                  unsettled_capacity=2048, page_heap_capacity=2048)

_fixtures = {}


def _fixture(name):
    if name not in _fixtures:
        _fixtures[name] = gu.load(name)
    return _fixtures[name]


def _replay(name, tier, **kw):
    """(fixture, _Handle) of a fixture replayed on one tier; the interner that encoded the ops
    names the reference's keys and values."""
    fx = _fixture(name)
    interner = gu.interner_for(fx)
    a = gu.encode_docs(fx, interner)
    mt = _gpu_batch(len(fx["docs"]), **dict(TIERS[tier], **kw))
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    sets = {d: _ref_sets(doc["out"], interner) for d, doc in enumerate(fx["docs"])}
    return fx, _Handle(mt, [doc["out"]["length"] for doc in fx["docs"]], sets)


# ---------------------------------------------------------------- 1. whole documents, every tier
@pytest.mark.gpu
@pytest.mark.parametrize("tier", list(TIERS))
@pytest.mark.parametrize("name", ["ref_small", "ref_ext", "ref_c3", "ref_combine", "ref_zam_long"])
def test_bulk_props_whole_documents_match_reference(name, tier):
    """All documents in one call: (A) and (B); 24 fixed-seed ranges per document; for the
    fixtures with markers, ranges that begin at, end at, and hold only a marker; ref_small (no
    properties at all) answers exactly one run without a record per document."""
    fx, H = _replay(name, tier)
    mt, n = H.mt, len(fx["docs"])
    assert (mt.status() == 0).all()
    whole = _check_queries(H, [(d, 0, -1) for d in range(n)])
    assert _decode(mt.get_prop_runs_raw()) == whole == mt.get_prop_runs_bulk()
    assert whole == [H.host(d) for d in range(n)]
    if name == "ref_small":
        run_off, word_off, runs, recs = mt.get_prop_runs_raw()
        assert len(recs) == 0 and (word_off == 0).all()
        assert np.array_equal(run_off, np.arange(n + 1))
        assert runs.tolist() == [[0, H.lengths[d], NONE] for d in range(n)]
    else:
        assert any(p for res in whole for _, _, p in res)
    rng = np.random.default_rng(20240611)
    queries, n_marks = [], 0
    for d in range(n):
        ln = H.lengths[d]
        for _ in range(24):
            s = int(rng.integers(0, ln + 1))
            queries.append((d, s, int(rng.integers(s, ln + 1))))
        marks = [p for p, _, marker in _visible_rows(fx["docs"][d]["out"]) if marker]
        n_marks += len(marks)
        for m in marks[:4]:   # ranges that begin at, end at, and hold only a marker
            queries += [(d, m, m + 1), (d, max(m - 2, 0), m + 1), (d, m, min(m + 3, ln))]
    if name in ("ref_ext", "ref_combine"):
        assert n_marks == {"ref_ext": 33, "ref_combine": 47}[name]
    _check_queries(H, queries)


# ---------------------------------------------------------------- 2. chunk and page edges
def _edge_queries(doc, d, rng, total=200):
    """200 queries of document d: the named edge cases, chosen from the reference's rows so
    that each provably occurs, then fixed-seed random ranges."""
    rows = _visible_rows(doc["out"])
    ln = doc["out"]["length"]
    long_rows = [i for i, (_, n, marker) in enumerate(rows) if n >= 3 and not marker]
    assert len(long_rows) > 200
    cases = {}
    p, n, _ = rows[long_rows[7]]
    cases["start == end"] = (p + 1, p + 1)
    cases["inside one segment"] = (p + 1, p + n - 1)
    i = long_rows[20]
    j = next(k for k in long_rows if k >= i + 70)
    cases["mid-segment to mid-segment across > 64 segments"] = (rows[i][0] + 1, rows[j][0] + 1)
    assert j - i > PAGE_SLOTS
    i2 = long_rows[100]
    j2 = next(k for k in long_rows if k >= i2 + 3 * PAGE_SLOTS)
    cases["across several pages"] = (rows[i2][0] + 2, rows[j2][0] + 2)
    cases["start in the last page"] = (rows[-5][0], ln)
    cases["end = -1"] = (rows[long_rows[50]][0] + 1, -1)
    cases["start past the length"] = (ln + 5, ln + 10)
    cases["start past the length, end = -1"] = (ln + 1, -1)
    cases["negative start"] = (-3, 5)
    cases["end past the length"] = (ln - 3, ln + 100)
    cases["start > end"] = (40, 10)
    cases["whole document"] = (0, ln)
    cases["one position"] = (p, p + 1)
    queries = [(d, s, e) for s, e in cases.values()]
    while len(queries) < total:
        s = int(rng.integers(0, ln + 1))
        width = int(rng.integers(0, [4, 40, 400, ln + 1][int(rng.integers(0, 4))]))
        queries.append((d, s, min(s + width, ln)))
    return queries


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["paged", "grow"])
def test_bulk_props_chunk_and_page_edges(tier):
    """ref_c3_full (documents of ~3.5k segments, 60+ pages) in the paged layout and in the
    growth step's big region: 200 queries per document packed back to back."""
    fx, H = _replay("ref_c3_full", tier, delta_log_capacity=1 << 20)
    mt, n = H.mt, len(fx["docs"])
    assert (mt.status() == 0).all()
    assert all(mt.is_paged(d) for d in range(n))
    if tier == "grow":
        assert mt.last_grown()["in_big_region"] == n
    rng = np.random.default_rng(7)
    queries = []
    for d, doc in enumerate(fx["docs"]):
        q = _edge_queries(doc, d, rng)
        assert len(q) == 200
        queries += q
    got = _check_queries(H, queries)
    counts = [len(r) for r in got]
    assert 0 in counts and 1 in counts and max(counts) > 64


# ---------------------------------------------------------------- 3. long runs, built by hand
def _hand_doc(seq0, n_ins, scale, model):
    """One writer that has seen everything (referenceSequenceNumber = sequenceNumber - 1,
    minimumSequenceNumber 0: nothing is coalesced): n_ins single-unit inserts at varying
    positions, three one-key annotates, then every third unit of a range removed (from the
    top, so lower positions hold).  model: the per-unit list of (unit, dict), seeded by the
    caller and updated in place."""
    msgs = []

    def send(op):
        seq = seq0 + len(msgs) + 1
        msgs.append(dict(clientId="client-1", sequenceNumber=seq, referenceSequenceNumber=seq - 1,
                         minimumSequenceNumber=0, type="op", contents=op))

    for i in range(n_ins):
        pos = (i * 37 + 11) % (len(model) + 1)
        ch = chr(0x41 + i % 26)
        send({"type": 0, "pos1": pos, "seg": ch})
        model.insert(pos, (ch, {}))
    for key, val, (a, b) in (("k1", 5, (10, 170)), ("k2", 6, (60, 70)), ("k3", 7, (130, 131))):
        a, b = a * scale, b * scale
        send({"type": 2, "pos1": a, "pos2": b, "props": {key: val}})
        for x in range(a, b):
            model[x] = (model[x][0], dict(model[x][1], **{key: val}))
    for p in reversed(range(20 * scale, 120 * scale, 3)):
        send({"type": 1, "pos1": p, "pos2": p + 1})
        del model[p]
    return msgs


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["hbm", "paged"])
def test_bulk_props_long_runs_built_by_hand(tier):
    """Document 0 is the recipe as specified: 4 seeded units, 200 single-unit inserts, annotates
    over [10, 170), [60, 70), [130, 131), every third unit of [20, 120) removed.  Its longest
    single-set run is [70, 130): 60 segments, so the run of more than 128 segments that the
    chunk-without-a-head case needs cannot occur in it; document 1 is the same recipe three
    times the size (600 inserts, [30, 510), [180, 210), [390, 393), every third unit of
    [60, 360)), whose run over [210, 390) holds 180 segments before the removes.  Document 2 is
    empty, document 3 has everything removed.  Expected values come from the per-unit model."""
    from fluidframework_amd.wire import Batch, Interner
    interner = Interner(synthetic=True)
    b = Batch(interner)
    models = [[(c, {}) for c in "abcd"], [(c, {}) for c in "abcd"], [], [(c, {}) for c in "abcdef"]]
    b.add_doc("abcd", _hand_doc(0, 200, 1, models[0]))
    b.add_doc("abcd", _hand_doc(0, 600, 3, models[1]))
    b.add_doc("", [])
    gone = [dict(clientId="client-1", sequenceNumber=1, referenceSequenceNumber=0, minimumSequenceNumber=0,
                 type="op", contents={"type": 2, "pos1": 1, "pos2": 5, "props": {"k4": 9}}),
            dict(clientId="client-1", sequenceNumber=2, referenceSequenceNumber=1, minimumSequenceNumber=0,
                 type="op", contents={"type": 1, "pos1": 0, "pos2": 6})]
    b.add_doc("abcdef", gone)
    models[3] = []
    a = b.arrays()
    mt = _gpu_batch(4, **TIERS[tier])
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    assert (mt.status() == 0).all()
    assert mt.get_texts() == ["".join(u for u, _ in m) for m in models]
    sets = {d: [_ids(p, interner) for _, p in m] for d, m in enumerate(models)}
    H = _Handle(mt, [len(m) for m in models], sets)
    whole = _check_queries(H, [(d, 0, -1) for d in range(4)])
    assert whole[2] == [] and whole[3] == []
    for res in whole:   # maximal runs: the key order cannot differ here
        assert all(frozenset(x[2] or []) != frozenset(y[2] or []) for x, y in zip(res, res[1:]))
    # the default view of document 1: a run of more than 128 segments (a chunk without a head),
    # with removed segments inside runs
    segs = mt.get_segments(1)[0]
    assert all(int(r[0]) == 1 for r in segs)   # nothing was coalesced
    pos, first_seg, last_seg = 0, {}, {}
    for i, r in enumerate(segs):
        if int(r[3]) == gu.INT_MIN:
            first_seg.setdefault(pos, i)
            last_seg[pos] = i
            pos += int(r[0])
    spans = [(first_seg[p], last_seg[p + l - 1], l) for p, l, _ in whole[1]]
    assert max(l for _, _, l in spans) > 128                                   # visible segments of a run
    assert any(hi - lo + 1 > l for lo, hi, l in spans)                        # removed ones inside a run
    assert any(hi - lo + 1 > 128 and l < hi - lo + 1 for lo, hi, l in spans)
    rng = np.random.default_rng(3)
    queries = []
    for d in range(4):
        ln = H.lengths[d]
        queries += [(d, 0, ln), (d, 1, ln - 1), (d, ln, ln), (d, 2, 1), (d, ln // 2, -1), (d, 63, 65), (d, 64, 128)]
        for _ in range(40):
            s = int(rng.integers(0, ln + 1))
            queries.append((d, s, int(rng.integers(s, ln + 1))))
    order = rng.permutation(len(queries))
    _check_queries(H, [queries[i] for i in order])


# ---------------------------------------------------------------- 4. point queries
def _want_point(H, d, p):
    if p < 0 or p >= H.lengths[d]:
        return None
    return H.sets[d][p]


@pytest.mark.gpu
def test_bulk_props_point_queries():
    """get_properties_at_positions for every position of every ref_ext document plus -1, the
    length, the length + 5 and 2**31 - 1: the reference's set inside, None outside.  On
    ref_c3_full 2000 fixed-seed (doc, pos) pairs in one call, and get_properties_at_position
    agrees on 50 of them."""
    fx, H = _replay("ref_ext", "paged")
    docs, pos = [], []
    for d, ln in enumerate(H.lengths):
        ps = list(range(ln)) + [-1, ln, ln + 5, 2 ** 31 - 1]
        docs += [d] * len(ps)
        pos += ps
    got = H.mt.get_properties_at_positions(docs, pos)
    assert len(got) == len(pos)
    seen_props = 0
    for d, p, g in zip(docs, pos, got):
        want = _want_point(H, d, p)
        if want is None:
            assert g is None, (d, p, g)
        else:
            assert frozenset(g or []) == want, (d, p, g)
            seen_props += bool(g)
    assert seen_props > 0

    fx, H = _replay("ref_c3_full", "paged", delta_log_capacity=1 << 20)
    rng = np.random.default_rng(41)
    docs = rng.integers(0, len(fx["docs"]), 2000)
    pos = np.array([int(rng.integers(0, H.lengths[d])) for d in docs])
    got = H.mt.get_properties_at_positions(docs, pos)
    for d, p, g in zip(docs.tolist(), pos.tolist(), got):
        assert frozenset(g or []) == H.sets[d][p], (d, p, g)
    for k in range(0, 2000, 40):
        assert H.mt.get_properties_at_position(int(docs[k]), int(pos[k])) == got[k]


# ---------------------------------------------------------------- 5. arguments
@pytest.mark.gpu
def test_bulk_props_arguments():
    """docs as a shuffled subset with repeats; scalars broadcast; a sizing call returns the
    filling call's offsets; cap_runs or cap_words one short is MT_E_OVERFLOW with both outputs
    untouched and both offset arrays filled; sentinels after the results stay; doc == n_docs and
    n = n_docs + 1 without docs are MT_E_INVALID; n = 0 works."""
    from fluidframework_amd import _native
    fx, H = _replay("ref_c3", "paged")
    mt, n = H.mt, len(fx["docs"])
    docs = np.array([3, 0, 0, 2, 3, 0, 1, 3], dtype=np.uint32) % n
    assert mt.get_prop_runs_bulk(docs) == [H.host(int(d)) for d in docs]
    start = np.arange(len(docs), dtype=np.int32) * 5 + 1
    end = start + np.array([1, 2, 300, 7, 0, 65, 64, 1000], dtype=np.int32)
    _check_queries(H, list(zip(docs.tolist(), start.tolist(), end.tolist())))
    # scalars broadcast; an end of None is the document's length
    assert mt.get_prop_runs_bulk(docs, 2, 90) == [_clip(H.host(int(d)), 2, 90, H.lengths[d]) for d in docs]
    assert mt.get_prop_runs_bulk([1], [4], [None]) == [_clip(H.host(1), 4, None, H.lengths[1])]

    lib, h = mt.lib, mt.h
    nq = len(docs)
    args = (h, nq, _native.ptr(docs), _native.ptr(start), _native.ptr(end))
    ro_size, wo_size = np.full(nq + 1, -7, dtype=np.int64), np.full(nq + 1, -7, dtype=np.int64)
    assert lib.mt_get_prop_runs_bulk(*args, _native.ptr(ro_size), _native.ptr(wo_size), None, 0, None, 0) == 0
    nr, nw = int(ro_size[-1]), int(wo_size[-1])
    assert nr > 0 and nw > 0 and ro_size[0] == 0 and wo_size[0] == 0
    runs = np.full(3 * (nr + 2), 0xABCDABCD, dtype=np.uint32)
    recs = np.full(nw + 2, 0xABCDABCD, dtype=np.uint32)
    for cap_r, cap_w in ((nr - 1, nw), (nr, nw - 1)):
        ro, wo = np.zeros(nq + 1, dtype=np.int64), np.zeros(nq + 1, dtype=np.int64)
        assert lib.mt_get_prop_runs_bulk(*args, _native.ptr(ro), _native.ptr(wo), _native.ptr(runs), cap_r,
                                         _native.ptr(recs), cap_w) == _native.MT_E_OVERFLOW
        assert (runs == 0xABCDABCD).all() and (recs == 0xABCDABCD).all()
        assert np.array_equal(ro, ro_size) and np.array_equal(wo, wo_size)
        msg = lib.mt_last_error(h).decode()
        assert str(nr) in msg and str(nw) in msg
    ro, wo = np.zeros(nq + 1, dtype=np.int64), np.zeros(nq + 1, dtype=np.int64)
    assert lib.mt_get_prop_runs_bulk(*args, _native.ptr(ro), _native.ptr(wo), _native.ptr(runs), nr,
                                     _native.ptr(recs), nw) == 0
    assert np.array_equal(ro, ro_size) and np.array_equal(wo, wo_size)
    assert (runs[3 * nr:] == 0xABCDABCD).all() and (recs[nw:] == 0xABCDABCD).all()
    ro2, wo2, runs2, recs2 = mt.get_prop_runs_raw(docs, start, end)
    assert np.array_equal(ro2, ro_size) and np.array_equal(wo2, wo_size)
    assert np.array_equal(runs2.reshape(-1), runs[:3 * nr]) and np.array_equal(recs2, recs[:nw])

    bad = docs.copy()
    bad[4] = n
    assert lib.mt_get_prop_runs_bulk(h, nq, _native.ptr(bad), None, None, _native.ptr(ro), _native.ptr(wo),
                                     None, 0, None, 0) == _native.MT_E_INVALID
    # docs NULL addresses documents 0..n-1: more queries than documents are refused
    ro_n, wo_n = np.zeros(n + 2, dtype=np.int64), np.zeros(n + 2, dtype=np.int64)
    assert lib.mt_get_prop_runs_bulk(h, n + 1, None, None, None, _native.ptr(ro_n), _native.ptr(wo_n),
                                     None, 0, None, 0) == _native.MT_E_INVALID
    with pytest.raises(RuntimeError):
        mt.get_prop_runs_bulk([n])
    assert mt.get_prop_runs_bulk([]) == []
    assert mt.get_properties_at_positions([], []) == []
    ro0, wo0, runs0, recs0 = mt.get_prop_runs_raw([])
    assert ro0.tolist() == [0] and wo0.tolist() == [0] and len(runs0) == 0 and len(recs0) == 0


# ---------------------------------------------------------------- 6. failed documents
@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["lds", "paged"])
def test_bulk_props_failed_documents_answer_from_where_they_stopped(tier):
    """ref_errors: (B) against get_prop_runs, (A) against the fixture's state at the throw."""
    fx, H = _replay("ref_errors", tier)
    n = len(fx["docs"])
    assert (H.mt.status() != 0).any()
    whole = _check_queries(H, [(d, 0, -1) for d in range(n)])
    assert whole == [H.host(d) for d in range(n)]
    rng = np.random.default_rng(13)
    queries = []
    for d in range(n):
        for _ in range(8):
            s = int(rng.integers(0, H.lengths[d] + 1))
            queries.append((d, s, int(rng.integers(s, H.lengths[d] + 1))))
    _check_queries(H, queries)


# ---------------------------------------------------------------- 7. live handle
def _msg(ev):
    _, cid, seq, ref, msn, op = ev
    return dict(clientId=cid, sequenceNumber=seq, referenceSequenceNumber=ref, minimumSequenceNumber=msn,
                type="op", contents=op)


@pytest.mark.gpu
def test_bulk_props_live_handle():
    """ref_live replayed through LiveClient: (B) at every reconnect (unacked inserts in, pending
    removes out); (A) and (B) after the last event; getPropertiesAtPosition at 20 positions."""
    from fluidframework_amd.live import LiveClient
    from fluidframework_amd.wire import Interner
    fx = gu.load("ref_live")
    rng = np.random.default_rng(5)
    for doc in fx["docs"]:
        interner = Interner(synthetic=True)
        lc = LiveClient(doc["seed_text"], interner=interner, seg_capacity=16384, text_capacity=1 << 17)
        lc.startOrUpdateCollaboration("local-0")
        unseq, checked = [], 0
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
                assert lc.pendingCounts()[1] > 0 or not unseq
                now = _Handle(lc.mt, [lc.mt.get_length(0)])
                ln = now.lengths[0]
                _check_queries(now, [(0, 0, -1), (0, ln // 3, 2 * ln // 3), (0, ln // 2, ln // 2 + 1)])
                checked += 1
                lc.startOrUpdateCollaboration(ev[1])
                unseq = [lc.regeneratePendingOp(o) for o in unseq]
        lc.flush()
        assert checked > 0
        H = _Handle(lc.mt, [doc["out"]["length"]], {0: _ref_sets(doc["out"], interner)})
        ln = H.lengths[0]
        queries = [(0, 0, -1), (0, ln // 3, 2 * ln // 3)]
        for _ in range(20):
            s = int(rng.integers(0, ln + 1))
            queries.append((0, s, int(rng.integers(s, ln + 1))))
        _check_queries(H, queries)
        for p in rng.integers(0, ln, 20).tolist():
            assert frozenset(lc.getPropertiesAtPosition(p) or []) == H.sets[0][p], p


# ---------------------------------------------------------------- 8. snapshot-loaded handle
@pytest.mark.gpu
def test_bulk_props_snapshot_loaded_handle():
    """ref_snap on the paged_load capacities (large headers paged at load), after the tail: (A)
    and (B) for the documents the reference loads."""
    fx = gu.load("ref_snap")
    docs = fx["docs"]
    interner = gu.Interner()
    la, oa = gu.encode_snap_docs(fx, interner, docs)
    mt = _gpu_batch(len(docs), **PAGED_LOAD)
    mt.load_snapshots(la)
    st = mt.status()
    assert any(mt.is_paged(i) for i in range(len(docs)) if st[i] == 0)
    mt.apply_arrays(oa)
    good = [i for i, d in enumerate(docs) if not gu.snap_status(d)]
    assert len(good) >= 8
    H = _Handle(mt, [d["out"]["length"] if i in good else 0 for i, d in enumerate(docs)],
                {i: _ref_sets(docs[i]["out"], interner) for i in good})
    _check_queries(H, [(i, 0, -1) for i in good] + [(i, 7, H.lengths[i] - 7) for i in good])


# ---------------------------------------------------------------- 9. device variant
@pytest.mark.gpu
def test_bulk_props_device_variant_equals_host_variant():
    fx, H = _replay("ref_c3", "paged")
    mt, n = H.mt, len(fx["docs"])
    rng = np.random.default_rng(11)
    docs = rng.integers(0, n, 300).astype(np.uint32)
    start = rng.integers(0, 3000, 300).astype(np.int32)
    end = (start + rng.integers(0, 200, 300)).astype(np.int32)
    end[::17] = -1
    for args in ((None, None, None), (docs, start, end)):
        host = mt.get_prop_runs_raw(*args)
        dev = mt.get_prop_runs_device(*args)
        assert all(t.is_cuda and t.device.index == mt.device for t in dev)
        assert [t.dtype for t in dev] == [torch.int64, torch.int64, torch.int32, torch.int32]
        assert dev[2].shape == (len(host[2]), 3)
        for hv, dv in zip(host, dev):
            assert np.array_equal(dv.cpu().numpy().view(hv.dtype), hv)
    # into a caller's tensors; one row short: refused, the tensors untouched
    ro, wo, runs, recs = mt.get_prop_runs_raw(docs, start, end)
    fill = 0x5A5A5A5A
    t_runs = torch.full((len(runs) + 3, 3), fill, dtype=torch.int32, device="cuda")
    t_recs = torch.full((len(recs) + 5,), fill, dtype=torch.int32, device="cuda")
    dro, dwo, druns, drecs = mt.get_prop_runs_device(docs, start, end, out=(t_runs, t_recs))
    assert np.array_equal(dro.cpu().numpy(), ro) and np.array_equal(dwo.cpu().numpy(), wo)
    host_runs, host_recs = t_runs.cpu().numpy().view(np.uint32), t_recs.cpu().numpy().view(np.uint32)
    assert np.array_equal(host_runs[:len(runs)], runs) and (host_runs[len(runs):] == fill).all()
    assert np.array_equal(host_recs[:len(recs)], recs) and (host_recs[len(recs):] == fill).all()
    assert druns.data_ptr() == t_runs.data_ptr() and drecs.data_ptr() == t_recs.data_ptr()
    small = torch.full((len(runs) - 1, 3), fill, dtype=torch.int32, device="cuda")
    t_recs.fill_(fill)
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        mt.get_prop_runs_device(docs, start, end, out=(small, t_recs))
    assert (small.cpu().numpy().view(np.uint32) == fill).all()
    assert (t_recs.cpu().numpy().view(np.uint32) == fill).all()
    with pytest.raises(ValueError):
        mt.get_prop_runs_device(docs, start, end, out=(t_runs.to(torch.int64), t_recs))


# ---------------------------------------------------------------- 10. Node facade
def _js_ranges(ln):
    return [[0, ln // 2], [ln // 3, ln // 3 + 1], [5, None], [None, 7], [ln - 3, ln + 10], [2, 2], [1, ln - 1],
            [ln // 4, ln // 4 + 130]]


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
@pytest.mark.parametrize("name", ["ref_ext", "ref_combine"])
def test_bulk_props_node_facade(name, tmp_path):
    """GpuMergeTreeBatch.getPropertiesAtPositions (every position of every document, and
    positions outside) and GpuClient.getPropertyRuns (whole documents and ranges) equal the
    reference's property objects per position; GpuClient.getPropertiesAtPosition agrees."""
    from fluidframework_amd import build
    build.build()
    build.build_snapdec()
    build.build_node_addon()
    fx = _fixture(name)
    lens = [d["out"]["length"] for d in fx["docs"]]
    ranges = [_js_ranges(ln) for ln in lens]
    rf = tmp_path / "ranges.json"
    rf.write_text(json.dumps(ranges))
    out = subprocess.run(["node", os.path.join(REPO, "tests", "js", "bulk_props_tool.js"),
                          os.path.join(gu.GOLDEN, name + ".json.gz"), str(rf)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)

    def per_position(doc):
        want = []
        for s in doc["out"]["segs"]:
            if s["rseq"] is None:
                want += [s["props"] or None] * s["len"]
        return want

    def expand(runs, s, e, ln):
        s, e = _clamp(s, e, ln)
        at, res = s, []
        for r in runs:
            assert r["position"] == at and r["length"] > 0, (r, at)
            res += [r.get("props") or None] * r["length"]
            at += r["length"]
        assert at == e, (at, e)
        return res

    seen = 0
    for d, (doc, g) in enumerate(zip(fx["docs"], got["docs"])):
        want, ln = per_position(doc), lens[d]
        assert [p or None for p in g["points"]] == want, d
        assert g["outside"] == [None, None, None, None]
        assert expand(g["whole"], None, None, ln) == want
        for (s, e), runs in zip(ranges[d], g["ranges"]):
            cs, ce = _clamp(s, e, ln)
            assert expand(runs, s, e, ln) == want[cs:ce], (d, s, e)
        for p, props in g["single"]:
            assert (props or None) == want[p], (d, p)
        seen += sum(1 for w in want if w)
    assert seen > 0


# ---------------------------------------------------------------- 11. the C ABI (no GPU)
def test_bulk_props_symbols_exported_and_bound():
    """The built library exports the three symbols and _native.SIGNATURES binds them with the
    header's argument lists."""
    import ctypes
    from fluidframework_amd import build, _native
    build.build()
    lib = _native.load()
    P, U32, U64, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    want = {
        "mt_get_prop_runs_bulk": [P, U32, P, P, P, P, P, P, U64, P, U64],
        "mt_get_prop_runs_bulk_device": [P, U32, P, P, P, P, P, P, U64, P, U64],
        "mt_last_props_ms": [P, P],
    }
    sigs = {s[0]: s for s in _native.SIGNATURES}
    for name, args in want.items():
        assert hasattr(lib, name), name
        assert name in sigs, name
        assert sigs[name][1] is I and list(sigs[name][2]) == args, name
        assert getattr(lib, name).argtypes == args
