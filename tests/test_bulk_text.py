"""Bulk and ranged text read-out on the device (mt_get_texts / mt_get_texts_device,
MergeTreeBatch.get_texts*, the Node facade's getTexts / getText(start, end) /
getText*WithPlaceholders / createTextHelper().getText): MergeTreeTextHelper.getText(currentSeq,
local client, placeholder, start, end) for many (doc, start, end) queries in one launch.

Expected values come from the reference-made fixtures, bit-exact: the position-space string of
a document is built on the host from the reference's final text and segment rows -- visible text
rows take their units from the reference text in order, visible markers are one placeholder
slot each -- and a query is its [start:end] with the marker slots dropped (placeholder "") or
replaced (" "): a restatement of MT/textSegment.ts:241-263 over reference data."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch   # before the replay library loads: both then share one HIP runtime (as in bench.py)

import golden_util as gu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = -1   # a marker's slot in a position-space array
PAGE_SLOTS = 64   # MT_PG_SLOTS: segments a page holds at most (csrc/mt_device.h)


# ---------------------------------------------------------------- the host derivation
def _units(s):
    return np.frombuffer(s.encode("utf-16-le", errors="surrogatepass"), dtype="<u2").astype(np.int32)


def _string(units):
    return np.asarray(units, dtype="<u2").tobytes().decode("utf-16-le", errors="surrogatepass")


def _visible_rows(out):
    """[(position, length, is_marker)] of the reference's visible segment rows."""
    rows, pos = [], 0
    for r in out["segs"]:
        if r["rseq"] is None:
            rows.append((pos, r["len"], r["marker"] is not None))
            pos += r["len"]
    return rows


def _slots(out):
    """The document in position space: one UTF-16 unit or MARK per position."""
    text = _units(out["text"])
    parts, k = [], 0
    for _, n, marker in _visible_rows(out):
        if marker:
            parts.append(np.full(n, MARK, dtype=np.int32))
        else:
            parts.append(text[k:k + n])
            k += n
    assert k == len(text)
    s = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
    assert len(s) == out["length"]
    return s


def _derive(slots, start, end, placeholder):
    """getText(placeholder, start, end) with start / end clamped into [0, length]."""
    n = len(slots)
    e = n if end is None or end < 0 else min(end, n)
    s = min(max(0 if start is None else start, 0), n)
    part = slots[s:e] if s < e else slots[:0]
    if placeholder == "":
        return part[part != MARK]
    return np.where(part == MARK, ord(placeholder), part)


def _check_queries(mt, slots_of, queries, placeholder):
    """One get_texts_raw call for queries [(doc, start, end)] against the derivation; returns off."""
    docs = np.array([q[0] for q in queries], dtype=np.uint32)
    start = np.array([q[1] for q in queries], dtype=np.int32)
    end = np.array([q[2] for q in queries], dtype=np.int32)
    off, units = mt.get_texts_raw(docs, start, end, placeholder)
    assert off[0] == 0 and len(off) == len(queries) + 1 and off[-1] == len(units)
    bad = []
    for q, (d, s, e) in enumerate(queries):
        want = _derive(slots_of[d], s, e, placeholder)
        got = units[off[q]:off[q + 1]].astype(np.int32)
        if len(got) != len(want) or not np.array_equal(got, want):
            bad.append((q, d, s, e, len(got), len(want)))
    assert not bad, (placeholder, bad[:6])
    return off


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

_replayed = {}


def _fixture(name):
    """(fixture, position-space arrays per document), loaded once."""
    if name not in _replayed:
        fx = gu.load(name)
        _replayed[name] = (fx, [_slots(d["out"]) for d in fx["docs"]])
    return _replayed[name]


def _replay(name, tier, **kw):
    fx, slots = _fixture(name)
    a = gu.encode_docs(fx, gu.interner_for(fx))
    mt = _gpu_batch(len(fx["docs"]), **dict(TIERS[tier], **kw))
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    return fx, slots, mt


# ---------------------------------------------------------------- 1. whole documents, every tier
@pytest.mark.gpu
@pytest.mark.parametrize("tier", list(TIERS))
@pytest.mark.parametrize("name", ["ref_small", "ref_ext", "ref_c3", "ref_zam_long"])
def test_bulk_text_whole_documents_match_reference(name, tier):
    """get_texts() equals the reference's text of every document and get_text(d); with the " "
    placeholder it is the position-space string (ref_ext: markers); a fixed-seed set of ranges
    per document equals the derivation with both placeholders."""
    fx, slots, mt = _replay(name, tier)
    n = len(fx["docs"])
    assert (mt.status() == 0).all()
    got = mt.get_texts()
    assert got == [d["out"]["text"] for d in fx["docs"]]
    assert got == [mt.get_text(d) for d in range(n)]
    assert mt.get_texts(placeholder=" ") == [_string(_derive(s, None, None, " ")) for s in slots]
    if name == "ref_ext":
        assert any((s == MARK).any() for s in slots)
    rng = np.random.default_rng(20240611)
    queries = []
    for d in range(n):
        ln = len(slots[d])
        for _ in range(24):
            s = int(rng.integers(0, ln + 1))
            queries.append((d, s, int(rng.integers(s, ln + 1))))
        marks = np.flatnonzero(slots[d] == MARK)
        for m in marks[:4]:   # ranges that begin at, end at, and hold only a marker
            queries += [(d, int(m), int(m) + 1), (d, max(int(m) - 2, 0), int(m) + 1), (d, int(m), min(int(m) + 3, ln))]
    for placeholder in ("", " "):
        _check_queries(mt, slots, queries, placeholder)


# ---------------------------------------------------------------- 2. chunk, page, alignment edges
def _edge_queries(doc, d, rng, total=200):
    """200 queries of document d: the named edge cases, chosen from the reference's rows so
    that each provably occurs, then fixed-seed random ranges.  Returns (queries, cases)."""
    rows = [r for r in _visible_rows(doc["out"])]
    ln = doc["out"]["length"]
    long_rows = [i for i, (_, n, marker) in enumerate(rows) if n >= 3 and not marker]
    assert len(long_rows) > 200
    cases = {}
    p, n, _ = rows[long_rows[7]]
    cases["start == end"] = (p + 1, p + 1)
    cases["inside one segment"] = (p + 1, p + n - 1)
    # from the middle of row i to the middle of a row 70+ rows later: more than 64 segments, and
    # -- a page holding at most 64 -- at least one page boundary of a paged document
    i = long_rows[20]
    j = next(k for k in long_rows if k >= i + 70)
    cases["mid-segment to mid-segment across > 64 segments"] = (rows[i][0] + 1, rows[j][0] + 1)
    assert j - i > PAGE_SLOTS
    i2 = long_rows[100]
    j2 = next(k for k in long_rows if k >= i2 + 3 * PAGE_SLOTS)
    cases["across several pages"] = (rows[i2][0] + 2, rows[j2][0] + 2)
    cases["end = -1"] = (rows[long_rows[50]][0] + 1, -1)
    cases["start past the length"] = (ln + 5, ln + 10)
    cases["start past the length, end = -1"] = (ln + 1, -1)
    cases["start == length"] = (ln, ln)
    cases["negative start"] = (-3, 5)
    cases["end past the length"] = (ln - 3, ln + 100)
    cases["start > end"] = (40, 10)
    cases["whole document"] = (0, ln)
    cases["one unit"] = (p, p + 1)
    queries = [(d, s, e) for s, e in cases.values()]
    while len(queries) < total:
        s = int(rng.integers(0, ln + 1))
        width = int(rng.integers(0, [4, 40, 400, ln + 1][int(rng.integers(0, 4))]))
        queries.append((d, s, min(s + width, ln)))
    return queries, cases


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["paged", "grow"])
def test_bulk_text_chunk_page_and_alignment_edges(tier):
    """ref_c3_full (documents of ~3.5k segments, ~60+ pages) in the paged layout and in the
    growth step's big region: whole texts equal the reference; 200 queries per document,
    packed back to back (odd and even destination offsets), equal the derivation with both
    placeholders."""
    fx, slots, mt = _replay("ref_c3_full", tier, delta_log_capacity=1 << 20)
    n = len(fx["docs"])
    assert (mt.status() == 0).all()
    assert all(mt.is_paged(d) for d in range(n))
    if tier == "grow":
        assert mt.last_grown()["in_big_region"] == n
    assert mt.get_texts() == [d["out"]["text"] for d in fx["docs"]]
    rng = np.random.default_rng(7)
    queries = []
    for d, doc in enumerate(fx["docs"]):
        q, cases = _edge_queries(doc, d, rng)
        assert len(q) == 200
        queries += q
    for placeholder in ("", " "):
        off = _check_queries(mt, slots, queries, placeholder)
        starts = off[:-1][np.diff(off) > 0]   # destinations of the non-empty results
        assert (starts % 2 == 0).any() and (starts % 2 == 1).any()
        lens = np.diff(off)
        assert (lens % 2 == 1).any() and (lens == 0).any() and (lens > 64 * 3).any()


# ---------------------------------------------------------------- 3. long segments and empties
def _seed_text(n, salt):
    return "".join(chr(0x21 + (i * 7 + salt) % 0x5E) if i % 11 else chr(0x4E00 + (i + salt) % 977) for i in range(n))


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["lds", "paged"])
def test_bulk_text_long_segments_and_empties(tier):
    """Documents seeded through load_initial_text and no ops: empty, 1 unit, 63 / 64 / 65 / 129
    units in one segment, 300 units; then one batch that removes everything from one document.
    Expected values are the seeded strings themselves."""
    from fluidframework_amd.wire import Batch, Interner
    texts = [_seed_text(n, 3 * k) for k, n in enumerate([0, 1, 63, 64, 65, 129, 300])]
    gone = 5
    b = Batch(Interner(synthetic=True))
    for d, t in enumerate(texts):
        rm = dict(clientId="client-1", sequenceNumber=1, referenceSequenceNumber=0, minimumSequenceNumber=0,
                  type="op", contents={"type": 1, "pos1": 0, "pos2": len(t)})
        b.add_doc(t, [rm] if d == gone else [])
    a = b.arrays()
    mt = _gpu_batch(len(texts), **TIERS[tier])
    mt.load_initial_text(a["seed_off"], a["seed"])
    for d in (2, 3, 4, 5):   # one segment each
        assert len(mt.get_segments(d)[0]) == 1
    rng = np.random.default_rng(99)
    for step in range(2):
        slots = [_units(t) for t in texts]
        assert mt.get_texts() == texts
        assert mt.get_texts() == [mt.get_text(d) for d in range(len(texts))]
        queries = []
        for d, t in enumerate(texts):
            ln = len(t)
            queries += [(d, 0, -1), (d, 0, ln), (d, 1, ln), (d, 0, ln - 1), (d, 1, ln - 1), (d, ln, ln), (d, 2, 1),
                        (d, ln // 2, -1), (d, 63, 65), (d, 64, 128), (d, 1, 2)]
            for _ in range(12):
                s = int(rng.integers(0, ln + 1))
                queries.append((d, s, int(rng.integers(s, ln + 1))))
        # (interleaved so that neighbours in the output differ in document and alignment)
        order = rng.permutation(len(queries))
        queries = [queries[i] for i in order]
        for placeholder in ("", " "):
            _check_queries(mt, slots, queries, placeholder)
        if step == 0:
            mt.apply_arrays(a)
            assert (mt.status() == 0).all()
            texts[gone] = ""


# ---------------------------------------------------------------- 4. arguments
@pytest.mark.gpu
def test_bulk_text_arguments():
    """docs as a shuffled subset with repeats; a cap one unit short is MT_E_OVERFLOW with the
    output untouched; doc == n_docs is MT_E_INVALID; a sizing call returns the filling call's
    off."""
    from fluidframework_amd import _native
    fx, slots, mt = _replay("ref_c3", "paged")
    n = len(fx["docs"])
    docs = np.array([3, 0, 0, 2, 3, 0, 1, 3], dtype=np.uint32) % n
    assert mt.get_texts(docs) == [fx["docs"][d]["out"]["text"] for d in docs]
    start = np.arange(len(docs), dtype=np.int32) * 5 + 1
    end = start + np.array([1, 2, 300, 7, 0, 65, 64, 1000], dtype=np.int32)
    _check_queries(mt, slots, list(zip(docs.tolist(), start.tolist(), end.tolist())), "")
    # scalars broadcast; an end of None is the document's length
    assert mt.get_texts(docs, 2, 9) == [fx["docs"][d]["out"]["text"][2:9] for d in docs]
    assert mt.get_texts([1], [4], [None]) == [fx["docs"][1]["out"]["text"][4:]]

    lib, h = mt.lib, mt.h
    off_size = np.full(len(docs) + 1, -7, dtype=np.int64)
    args = (h, len(docs), _native.ptr(docs), _native.ptr(start), _native.ptr(end), 0)
    assert lib.mt_get_texts(*args, _native.ptr(off_size), None, 0) == 0
    total = int(off_size[-1])
    assert total == sum(len(_derive(slots[d], s, e, "")) for d, s, e in zip(docs, start, end)) > 0
    out = np.full(total + 2, 0xABCD, dtype=np.uint16)
    off_short = np.zeros(len(docs) + 1, dtype=np.int64)
    assert lib.mt_get_texts(*args, _native.ptr(off_short), _native.ptr(out), total - 1) == _native.MT_E_OVERFLOW
    assert (out == 0xABCD).all()
    assert np.array_equal(off_short, off_size)   # off always receives the prefix sums
    off_fill = np.zeros(len(docs) + 1, dtype=np.int64)
    assert lib.mt_get_texts(*args, _native.ptr(off_fill), _native.ptr(out), total) == 0
    assert np.array_equal(off_fill, off_size)
    assert (out[total:] == 0xABCD).all()
    off2, units = mt.get_texts_raw(docs, start, end)
    assert np.array_equal(off2, off_size) and np.array_equal(units, out[:total])

    bad = docs.copy()
    bad[4] = n
    off_bad = np.zeros(len(docs) + 1, dtype=np.int64)
    assert lib.mt_get_texts(h, len(bad), _native.ptr(bad), None, None, 0, _native.ptr(off_bad), None, 0) == \
        _native.MT_E_INVALID
    # docs NULL addresses documents 0..n-1: more queries than documents are refused
    off_n = np.zeros(n + 2, dtype=np.int64)
    assert lib.mt_get_texts(h, n + 1, None, None, None, 0, _native.ptr(off_n), None, 0) == _native.MT_E_INVALID
    with pytest.raises(RuntimeError):
        mt.get_texts([n])
    with pytest.raises(ValueError):
        mt.get_texts(placeholder="ab")
    assert mt.get_texts([]) == []


# ---------------------------------------------------------------- 5. failed documents
@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["lds", "paged"])
def test_bulk_text_failed_documents_answer_from_where_they_stopped(tier):
    fx, slots, mt = _replay("ref_errors", tier)
    n = len(fx["docs"])
    assert (mt.status() != 0).any()
    got = mt.get_texts()
    assert got == [mt.get_text(d) for d in range(n)]
    assert got == [d["out"]["text"] for d in fx["docs"]]   # the reference's state at its throw


# ---------------------------------------------------------------- 6. live handle
def _msg(ev):
    _, cid, seq, ref, msn, op = ev
    return dict(clientId=cid, sequenceNumber=seq, referenceSequenceNumber=ref, minimumSequenceNumber=msn,
                type="op", contents=op)


@pytest.mark.gpu
def test_bulk_text_live_handle():
    """ref_live replayed through LiveClient: at every reconnect (unacked inserts in, pending
    removes out) get_texts() equals get_text(0); after the last event both equal the
    reference's text, and ranges equal the derivation."""
    from fluidframework_amd.live import LiveClient
    from fluidframework_amd.wire import Interner
    fx = gu.load("ref_live")
    rng = np.random.default_rng(5)
    for doc in fx["docs"]:
        lc = LiveClient(doc["seed_text"], interner=Interner(synthetic=True), seg_capacity=16384,
                        text_capacity=1 << 17)
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
                assert lc.mt.get_texts() == [lc.mt.get_text(0)]
                checked += 1
                lc.startOrUpdateCollaboration(ev[1])
                unseq = [lc.regeneratePendingOp(o) for o in unseq]
        lc.flush()
        assert checked > 0
        assert lc.mt.get_texts() == [lc.mt.get_text(0)] == [doc["out"]["text"]]
        slots = [_slots(doc["out"])]
        ln = len(slots[0])
        queries = [(0, 0, -1), (0, ln // 3, 2 * ln // 3)]
        for _ in range(20):
            s = int(rng.integers(0, ln + 1))
            queries.append((0, s, int(rng.integers(s, ln + 1))))
        _check_queries(lc.mt, slots, queries, " ")


# ---------------------------------------------------------------- 7. snapshot-loaded handle
@pytest.mark.gpu
def test_bulk_text_snapshot_loaded_handle():
    """ref_snap on the paged_load capacities (large headers paged at load), then the tail:
    get_texts() equals the reference's text; documents the reference fails to load answer as
    get_text does."""
    fx = gu.load("ref_snap")
    docs = fx["docs"]
    la, oa = gu.encode_snap_docs(fx, gu.Interner(), docs)
    mt = _gpu_batch(len(docs), **PAGED_LOAD)
    mt.load_snapshots(la)
    loaded = mt.get_texts()
    st = mt.status()
    assert any(mt.is_paged(i) for i in range(len(docs)) if st[i] == 0)
    mt.apply_arrays(oa)
    got = mt.get_texts()
    ok = 0
    for i, d in enumerate(docs):
        if gu.snap_status(d):
            assert got[i] == mt.get_text(i)
            continue
        assert loaded[i] == d["load_out"]["text"], d["doc"]
        assert got[i] == d["out"]["text"], d["doc"]
        ok += 1
    assert ok >= 8
    _check_queries(mt, {i: _slots(d["out"]) for i, d in enumerate(docs) if not gu.snap_status(d)},
                   [(i, 7, d["out"]["length"] - 7) for i, d in enumerate(docs) if not gu.snap_status(d)], " ")


# ---------------------------------------------------------------- 8. device variant
@pytest.mark.gpu
def test_bulk_text_device_variant_equals_host_variant():
    fx, slots, mt = _replay("ref_c3", "paged")
    n = len(fx["docs"])
    rng = np.random.default_rng(11)
    docs = rng.integers(0, n, 300).astype(np.uint32)
    start = rng.integers(0, 3000, 300).astype(np.int32)
    end = (start + rng.integers(0, 200, 300)).astype(np.int32)
    end[::17] = -1
    for args in ((None, None, None), (docs, start, end)):
        for placeholder in ("", " "):
            off, units = mt.get_texts_raw(*args, placeholder)
            doff, dunits = mt.get_texts_device(*args, placeholder)
            assert doff.is_cuda and dunits.is_cuda and doff.dtype == torch.int64 and dunits.dtype == torch.int16
            assert np.array_equal(doff.cpu().numpy(), off)
            assert np.array_equal(dunits.cpu().numpy().view(np.uint16), units)
    # into a caller's tensor at an odd unit offset (a 2-byte-aligned destination); one unit short: refused
    off, units = mt.get_texts_raw(docs, start, end)
    buf = torch.full((len(units) + 9,), 0x5A5A, dtype=torch.int16, device="cuda")
    doff, dunits = mt.get_texts_device(docs, start, end, out=buf[1:])
    assert np.array_equal(doff.cpu().numpy(), off)
    host = buf.cpu().numpy().view(np.uint16)
    assert np.array_equal(host[1:1 + len(units)], units)
    assert host[0] == 0x5A5A and (host[1 + len(units):] == 0x5A5A).all()
    small = torch.full((len(units) - 1,), 0x5A5A, dtype=torch.int16, device="cuda")
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        mt.get_texts_device(docs, start, end, out=small)
    assert (small.cpu().numpy().view(np.uint16) == 0x5A5A).all()


# ---------------------------------------------------------------- 9. Node facade
def _js_ranges(ln):
    return [[0, ln // 2], [ln // 3, ln // 3 + 1], [5, None], [None, 7], [ln - 3, ln + 10], [2, 2], [1, ln - 1],
            [ln // 4, ln // 4 + 130]]


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
@pytest.mark.parametrize("name", ["ref_ext", "ref_c3"])
def test_bulk_text_node_facade(name, tmp_path):
    """GpuMergeTreeBatch.getTexts, GpuClient.getText(s, e) / getTextRangeWithPlaceholders(s, e) /
    getTextWithPlaceholders and createTextHelper().getText(currentSeq, localId, " ") equal the
    derivation; a foreign (refSeq, clientId) and a two-unit placeholder throw."""
    from fluidframework_amd import build
    build.build()
    build.build_snapdec()
    build.build_node_addon()
    fx, slots = _fixture(name)
    ranges = [_js_ranges(len(s)) for s in slots]
    rf = tmp_path / "ranges.json"
    rf.write_text(json.dumps(ranges))
    out = subprocess.run(["node", os.path.join(REPO, "tests", "js", "bulk_text_tool.js"),
                          os.path.join(gu.GOLDEN, name + ".json.gz"), str(rf)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)
    texts = [d["out"]["text"] for d in fx["docs"]]
    assert got["texts"] == texts
    assert got["some"] == [texts[-1], texts[0], texts[0]]
    for d, (g, s) in enumerate(zip(got["docs"], slots)):
        assert g["ranges"] == [_string(_derive(s, a, b, "")) for a, b in ranges[d]], d
        assert g["helperRange"] == g["ranges"]
        assert g["placeholders"] == [_string(_derive(s, a, b, " ")) for a, b in ranges[d]], d
        assert g["helper"] == g["wholePlaceholders"] == _string(_derive(s, None, None, " "))
        assert g["whole"] == g["helperNoArgs"] == texts[d]
        assert all(m and "own view" in m for m in g["foreign"]), g["foreign"]
        assert g["longPlaceholder"] and "placeholder" in g["longPlaceholder"]
