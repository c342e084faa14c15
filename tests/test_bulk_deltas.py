"""Bulk delta-log drain (mt_get_delta_logs) against the single-document call
it replaces (mt_get_delta_log), the Python restatement of its rows (tests/delta_util.py) and,
for the plain fixtures, the reference's own callbacks."""
import ctypes

import numpy as np
import pytest
import torch   # before the replay library loads: both then share one HIP runtime (as in bench.py)

import delta_util as du
import golden_util as gu

pytestmark = pytest.mark.gpu

DL = 1 << 18
E_INVALID, E_OVERFLOW = -1, -5
# the storage tiers of tests/test_gpu_parity.py (TIERS), copied; "hm": >= 512 pages, so the log is
# written by the kHM tier (RICH_TIERS there)
TIERS = {
    "lds": dict(lds_seg_capacity=0),
    "hbm": dict(lds_seg_capacity=-1),
    "paged": dict(lds_seg_capacity=-1, page_capacity=256, unsettled_capacity=2048, page_heap_capacity=2048),
    "grow": dict(lds_seg_capacity=16, page_capacity=12, unsettled_capacity=16, page_heap_capacity=16),
    "hm": dict(lds_seg_capacity=-1, page_capacity=600, unsettled_capacity=2048, page_heap_capacity=2048),
}
# fixture, handle options, rich log?
CASES = {
    "ref_small": ("ref_small", dict(), False),
    "ref_ext": ("ref_ext", dict(), False),
    "ref_combine": ("ref_combine", dict(), False),
    "ref_rich": ("ref_rich", dict(delta_log_mode=1, delta_log_capacity=1 << 20), True),
    "ref_rich_ordinals": ("ref_rich", dict(delta_log_mode=1, delta_log_capacity=1 << 20, segment_ordinals=1), True),
}


def _handle(n_docs, **kw):
    from fluidframework_amd import MergeTreeBatch
    kw.setdefault("delta_log_capacity", DL)
    kw.setdefault("seg_capacity", 8192)
    kw.setdefault("text_capacity", 1 << 17)
    kw.setdefault("page_capacity", -1)
    return MergeTreeBatch(n_docs, **kw)


def _arrays(name):
    fx = gu.load(name)
    interner = gu.Interner() if name == "ref_rich" else gu.interner_for(fx)
    return fx, interner, gu.encode_docs(fx, interner)


_replays = {}


def _replayed(case, tier):
    """(fixture, handle, [get_delta_log(i)]) of a fixture replayed whole on a tier, once; the
    tests that share it only read."""
    if (case, tier) not in _replays:
        name, opts, _ = CASES[case]
        fx, _, a = _arrays(name)
        mt = _handle(len(fx["docs"]), **dict(TIERS[tier], **opts))
        mt.load_initial_text(a["seed_off"], a["seed"])
        mt.apply_arrays(a)
        assert (mt.status() == 0).all()
        _replays[(case, tier)] = (fx, mt, [mt.get_delta_log(i) for i in range(len(fx["docs"]))])
    return _replays[(case, tier)]


def _check_words(off, words, singles, docs=None, from_word=None):
    docs = range(len(singles)) if docs is None else docs
    assert len(off) == len(docs) + 1 and off[0] == 0 and off[-1] == len(words)
    for q, d in enumerate(docs):
        f = 0 if from_word is None else int(from_word[q])
        assert words[off[q]:off[q + 1]].tolist() == singles[d][f:], (q, d, f)


def _check_rows(off, words, row_off, rows, rich, flags=None):
    want_off, want, bad = du.expected_rows(off, words, rich, rows.dtype)
    assert np.array_equal(row_off, want_off)
    assert np.array_equal(rows, want)
    if flags is not None:
        assert [bool(f & du.BAD) for f in flags] == bad


# ---------------------------------------------------------------- equals the single call; rows
@pytest.mark.parametrize("tier", ["lds", "hbm", "paged", "grow"])
@pytest.mark.parametrize("case", list(CASES))
def test_bulk_deltas_equal_single_call_and_rows(case, tier):
    """words[off[i]:off[i + 1]] == get_delta_log(i) for every document, with and without rows;
    the rows equal the restatement's walk of the drained words (plain, rich, rich + ordinals)
    and, for the plain fixtures, the reference's (seq, kind, position, length) per delta segment."""
    from fluidframework_amd import _native
    fx, mt, singles = _replayed(case, tier)
    rich = CASES[case][2]
    off, words, flags = mt.get_delta_logs()
    _check_words(off, words, singles)
    assert not flags.any() and sum(len(s) for s in singles) > 1000
    off2, words2, row_off, rows, flags2 = mt.get_delta_logs(ranges=True)
    assert np.array_equal(off, off2) and np.array_equal(words, words2) and not flags2.any()
    assert rows.dtype == _native.DELTA_RANGE_DTYPE and row_off[-1] == len(rows) > 0
    _check_rows(off, words, row_off, rows, rich)
    for i, doc in enumerate(fx["docs"]):
        r = rows[row_off[i]:row_off[i + 1]]
        assert (r["query"] == i).all()
        if not rich:
            assert list(zip(r["seq"].tolist(), r["kind"].tolist(), r["position"].tolist(),
                            r["length"].tolist())) == du.reference_ranges(doc), doc["doc"]
            assert (r["uid"] == du.NO_UID).all()
    if case == "ref_rich_ordinals":
        assert (rows["uid"] != du.NO_UID).any() and (rows["position"][rows["kind"] < 0] >= 0).all()
    if case == "ref_rich":
        assert (rows["kind"] < 0).any() and (rows["position"][rows["kind"] < 0] == -1).all()


def test_bulk_deltas_khm_tier():
    """A handle of >= 512 pages per document writes its log from the kHM tier (the page metadata
    in HBM): the same storage, the same read-out (ref_rich as in test_gpu_parity's RICH_TIERS
    "hm": a rich log)."""
    _, mt, singles = _replayed("ref_rich", "hm")
    off, words, row_off, rows, flags = mt.get_delta_logs(ranges=True)
    _check_words(off, words, singles)
    _check_rows(off, words, row_off, rows, True, flags)
    assert not flags.any()


def test_bulk_deltas_khm_tier_xl_document():
    """The first document of ref_readouts_xl (60k C3 messages, ~1k pages) on the kHM tier with a
    log: half a million words in one span."""
    fx = gu.load("ref_readouts_xl")
    a = gu.encode_docs(fx, gu.interner_for(fx), fx["docs"][:1])
    mt = _handle(1, delta_log_capacity=1 << 21, lds_seg_capacity=-1, page_capacity=1600, unsettled_capacity=2048,
                 page_heap_capacity=2048)
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    assert (mt.status() == 0).all() and mt.is_paged(0)
    single = mt.get_delta_log(0)
    off, words, row_off, rows, flags = mt.get_delta_logs(ranges=True)
    assert len(single) > 300000 and not flags.any()
    _check_words(off, words, [single])
    _check_rows(off, words, row_off, rows, False, flags)
    assert len(rows) > 60000


def test_bulk_deltas_live_handle():
    """ref_live on live handles: propertyDeltas undefined is npd == -1 (no pairs follow)."""
    import test_live_client as tlc
    undefined = 0
    for doc in gu.load("ref_live")["docs"]:
        lc, _, errs = tlc._run_doc(doc)
        assert not errs
        single = lc.mt.get_delta_log(0)
        off, words, row_off, rows, flags = lc.mt.get_delta_logs(ranges=True)
        _check_words(off, words, [single])
        _check_rows(off, words, row_off, rows, False, flags)
        assert not flags.any() and len(rows) > 100
        undefined += sum(single[r["word"] + 2] == -1 for r in rows if r["kind"] == 2)
        lc.close()
    assert undefined > 0


def test_bulk_deltas_device_form():
    """Torch tensors equal the host form."""
    for case in ("ref_small", "ref_rich_ordinals"):
        _, mt, _ = _replayed(case, "paged")
        off, words, row_off, rows, flags = mt.get_delta_logs(ranges=True)
        d_off, d_words, d_row_off, d_rows, d_flags = mt.get_delta_logs_device(ranges=True)
        assert d_words.is_cuda and d_rows.is_cuda and d_off.is_cuda
        assert np.array_equal(d_off.cpu().numpy(), off) and np.array_equal(d_words.cpu().numpy(), words)
        assert np.array_equal(d_row_off.cpu().numpy(), row_off) and not d_flags.cpu().numpy().any()
        assert np.array_equal(d_rows.cpu().numpy().view(rows.dtype).reshape(-1), rows)
        docs = np.array([3, 1, 1], dtype=np.uint32)
        fw = np.array([0, 0, 10 ** 6], dtype=np.int32)
        h = mt.get_delta_logs(docs, fw)
        d = mt.get_delta_logs_device(docs, fw)
        assert len(d) == 3 and all(np.array_equal(x.cpu().numpy().astype(np.int64), np.asarray(y).astype(np.int64))
                                   for x, y in zip(d, h))
        assert h[2].tolist() == [0, 0, du.PAST]


# ---------------------------------------------------------------- query shapes
def test_bulk_deltas_query_shapes():
    fx, mt, singles = _replayed("ref_small", "paged")
    n = len(singles)
    assert n == 24
    for docs in (list(range(n))[::-1], [5, 2, 17, 9], [7] * 5, []):
        off, words, row_off, rows, flags = mt.get_delta_logs(np.asarray(docs, dtype=np.uint32), ranges=True)
        _check_words(off, words, singles, docs)
        _check_rows(off, words, row_off, rows, False, flags)
        assert len(flags) == len(docs) and not flags.any()
    off, words, flags = mt.get_delta_logs(docs=None)
    _check_words(off, words, singles)
    # 2051 queries: the device scan's threads take chunks of 3 and the last threads none
    docs = np.array([2, 0, 1], dtype=np.uint32)[np.arange(2051) % 3]
    off, words, row_off, rows, flags = mt.get_delta_logs(docs, ranges=True)
    _check_words(off, words, singles, docs.tolist())
    assert (rows["query"] == np.repeat(np.arange(2051), np.diff(row_off))).all()
    one = [du.rows(singles[d], False) for d in range(3)]
    assert np.array_equal(np.diff(row_off), [len(one[d]) for d in docs.tolist()])
    d = mt.get_delta_logs_device(docs, ranges=True)
    assert np.array_equal(d[0].cpu().numpy(), off) and np.array_equal(d[2].cpu().numpy(), row_off)
    assert np.array_equal(d[1].cpu().numpy(), words)
    assert np.array_equal(d[3].cpu().numpy().view(rows.dtype).reshape(-1), rows)
    # a document the handle does not have
    rc = mt.lib.mt_get_delta_logs(mt.h, 1, ctypes.c_void_p(np.array([n], dtype=np.uint32).ctypes.data), None,
                                  ctypes.c_void_p(np.zeros(2, dtype=np.int64).ctypes.data), None, None, None, 0, None, 0)
    assert rc == E_INVALID and "query 0" in mt.lib.mt_last_error(mt.h).decode()


def test_bulk_deltas_handle_without_a_log():
    mt = _handle(4, delta_log_capacity=0)
    off, words, row_off, rows, flags = mt.get_delta_logs(ranges=True)
    assert off.tolist() == [0] * 5 and row_off.tolist() == [0] * 5 and len(words) == 0 and len(rows) == 0
    assert flags.tolist() == [0] * 4
    d = mt.get_delta_logs_device(ranges=True)
    assert d[0].cpu().tolist() == [0] * 5 and d[2].cpu().tolist() == [0] * 5 and d[4].cpu().tolist() == [0] * 4
    mt.delta_log_reset_docs([1, 2])
    assert mt.get_delta_log(0) == []


# ---------------------------------------------------------------- word counts and alignment
N_ALIGN = 72


def _align_batch():
    """Document d: d single-character inserts (a record of 5 words each); every third document
    from the sixth on also one remove over its first 2 .. 5 segments (3 + 2 k words)."""
    from fluidframework_amd.wire import Batch, Interner
    b = Batch(Interner(synthetic=True))
    for d in range(N_ALIGN):
        msgs = [dict(clientId="client-1", sequenceNumber=t + 1, referenceSequenceNumber=t, minimumSequenceNumber=0,
                     contents=dict(type=0, pos1=0, seg=chr(97 + t % 26))) for t in range(d)]
        if d >= 6 and d % 3 == 0:
            msgs.append(dict(clientId="client-2", sequenceNumber=d + 1, referenceSequenceNumber=d,
                             minimumSequenceNumber=0, contents=dict(type=1, pos1=0, pos2=2 + d % 4)))
        b.add_doc("", msgs)
    return b.arrays()


def test_bulk_deltas_word_counts_and_alignment():
    """Log lengths of every residue mod 4, below and above 64 and 256 words; source offsets even
    and odd (from_word one 5-word record in) against arbitrary destination offsets: every
    pairing of source and destination alignment of the vector copy, its heads and tails."""
    a = _align_batch()
    mt = _handle(N_ALIGN, **TIERS["paged"])
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    assert (mt.status() == 0).all()
    singles = [mt.get_delta_log(d) for d in range(N_ALIGN)]
    lens = [len(s) for s in singles]
    assert lens[:6] == [0, 5, 10, 15, 20, 25] and lens[6] == 30 + 3 + 2 * 4 and lens[9] == 45 + 3 + 2 * 3
    assert {x % 4 for x in lens} == {0, 1, 2, 3} and min(lens) == 0 and max(lens) > 256
    assert any(32 < x < 64 for x in lens) and any(64 < x < 128 for x in lens) and any(128 < x < 256 for x in lens)
    docs = np.arange(1, N_ALIGN, dtype=np.uint32)
    for fw in (None, np.full(len(docs), 5, dtype=np.int32), np.where(np.arange(len(docs)) % 2, 5, 0).astype(np.int32),
               np.where(np.arange(len(docs)) % 3, 0, 5).astype(np.int32)):
        off, words, row_off, rows, flags = mt.get_delta_logs(docs, fw, ranges=True)
        _check_words(off, words, singles, docs.tolist(), fw)
        _check_rows(off, words, row_off, rows, False, flags)
        assert not flags.any()
        d = mt.get_delta_logs_device(docs, fw)
        assert np.array_equal(d[1].cpu().numpy(), words)
    # the removes' records hold several entries; their rows share seq and record
    off, words, row_off, rows, flags = mt.get_delta_logs(np.array([9], dtype=np.uint32), ranges=True)
    rem = rows[rows["kind"] == 1]
    assert len(rem) == 3 and len(set(rem["record"].tolist())) == 1 and (rem["seq"] == 10).all()
    assert rem["word"].tolist() == [48, 50, 52]


# ---------------------------------------------------------------- cursors
def test_bulk_deltas_cursors_across_batches():
    """A reader that keeps each document's word count drains only what a later batch appended."""
    fx, interner, a = _arrays("ref_small")
    n = len(fx["docs"])
    b1, b2 = gu.batches_to(a, fx["docs"], [[30, len(d["msgs"])] for d in fx["docs"]])
    mt = _handle(n, **TIERS["paged"])
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(b1)
    off1, words1, flags1 = mt.get_delta_logs()
    have = np.diff(off1).astype(np.int32)
    assert (have > 0).all() and not flags1.any()
    same = mt.get_delta_logs(from_word=have)
    assert same[0].tolist() == [0] * (n + 1) and len(same[1]) == 0 and not same[2].any()   # from_word == have
    past = mt.get_delta_logs(from_word=have + 1)
    assert past[0].tolist() == [0] * (n + 1) and (past[2] == du.PAST).all()
    mt.apply_arrays(b2)
    off2, words2, row_off2, rows2, flags2 = mt.get_delta_logs(from_word=have, ranges=True)
    assert not flags2.any() and (np.diff(off2) > 0).all()
    _check_rows(off2, words2, row_off2, rows2, False)
    for i, doc in enumerate(fx["docs"]):
        whole = words1[off1[i]:off1[i + 1]].tolist() + words2[off2[i]:off2[i + 1]].tolist()
        assert whole == mt.get_delta_log(i) == gu.expected(doc, interner)["deltas"], i
    fw = np.zeros(n, dtype=np.int32)
    fw[3] = -1
    with pytest.raises(RuntimeError, match=r"\(-1\).*query 3"):
        mt.get_delta_logs(from_word=fw)


# ---------------------------------------------------------------- overflow
def _ext_overflowed():
    """ref_ext on logs of 301 words (test_gpu_delta_log_overflow_keeps_whole_records) plus one
    document given no messages."""
    fx = gu.load("ref_ext")
    interner = gu.interner_for(fx)
    a = gu.encode_docs(fx, interner, fx["docs"] + [dict(seed_text="", msgs=[])])
    mt = _handle(len(fx["docs"]) + 1, delta_log_capacity=301)
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    assert (mt.status() == 0).all()
    return fx, interner, mt


def _p(x):
    return None if x is None else ctypes.c_void_p(x.ctypes.data)


def test_bulk_deltas_overflow_is_per_query():
    from fluidframework_amd import DeltaLogOverflow
    fx, interner, mt = _ext_overflowed()
    n = len(fx["docs"]) + 1
    off, words, row_off, rows, flags = mt.get_delta_logs(ranges=True)
    assert flags.tolist() == [du.OVERFLOWED] * (n - 1) + [0]
    for i, doc in enumerate(fx["docs"]):
        kept = words[off[i]:off[i + 1]].tolist()
        want = gu.expected(doc, interner)["deltas"]
        assert 0 < len(kept) <= 301 and kept == want[:len(kept)] and len(want) > 301
        with pytest.raises(DeltaLogOverflow) as ei:
            mt.get_delta_log(i)
        assert ei.value.records == kept
    assert off[n] == off[n - 1]
    _check_rows(off, words, row_off, rows, False, flags)     # whole records were kept: no MT_DLOG_BAD
    # flags == NULL: MT_E_OVERFLOW after everything is filled, naming the first such query
    docs = np.array([n - 1, 2, 0], dtype=np.uint32)
    o, ro = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    out = np.full(1000, -7, dtype=np.int32)
    rw = np.zeros(1000, dtype=rows.dtype)
    rc = mt.lib.mt_get_delta_logs(mt.h, 3, _p(docs), None, _p(o), _p(ro), None, _p(out), 1000, _p(rw), 1000)
    assert rc == E_OVERFLOW and "query 1" in mt.lib.mt_last_error(mt.h).decode()
    assert o.tolist() == [0, 0, off[3] - off[2], off[3] - off[2] + off[1]]
    assert out[:o[3]].tolist() == words[off[2]:off[3]].tolist() + words[:off[1]].tolist() and (out[o[3]:] == -7).all()
    assert ro[3] == (row_off[3] - row_off[2]) + row_off[1]
    assert rw[:ro[3]]["seq"].tolist() == rows[row_off[2]:row_off[3]]["seq"].tolist() + rows[:row_off[1]]["seq"].tolist()
    # an output one word short: MT_E_OVERFLOW, offsets written, out and rows untouched
    fl = np.zeros(3, dtype=np.uint32)
    o2, out2 = np.zeros(4, dtype=np.int64), np.full(1000, -7, dtype=np.int32)
    rw2 = np.zeros(1000, dtype=rows.dtype)
    rc = mt.lib.mt_get_delta_logs(mt.h, 3, _p(docs), None, _p(o2), _p(ro), _p(fl), _p(out2), int(o[3]) - 1, _p(rw2), 1000)
    msg = mt.lib.mt_last_error(mt.h).decode()
    assert rc == E_OVERFLOW and f"need {o[3]} words and {ro[3]} rows" in msg and f"hold {o[3] - 1} words" in msg
    assert o2.tolist() == o.tolist() and (out2 == -7).all() and not rw2["seq"].any()
    assert fl.tolist() == [0, du.OVERFLOWED, du.OVERFLOWED]
    rc = mt.lib.mt_get_delta_logs(mt.h, 3, _p(docs), None, _p(o2), _p(ro), _p(fl), _p(out2), 1000, _p(rw2), int(ro[3]) - 1)
    assert rc == E_OVERFLOW and (out2 == -7).all() and not rw2["seq"].any()


# ---------------------------------------------------------------- per-document reset
def test_delta_log_reset_docs():
    """Reset documents read empty with their overflow flag cleared and log the next batch from
    word 0; the others keep their records (and their flag) and append."""
    fx, interner, mt = _ext_overflowed()
    before = mt.get_delta_logs()
    mt.delta_log_reset_docs([0, 2, 2, 0])                       # (duplicates are harmless)
    off, words, flags = mt.get_delta_logs()
    assert flags[[0, 2]].tolist() == [0, 0] and off[1] == 0 and off[3] == off[2]
    keep = [i for i in range(len(flags)) if i not in (0, 2)]
    assert flags[keep].tolist() == before[2][keep].tolist()
    for i in keep:
        assert words[off[i]:off[i + 1]].tolist() == before[1][before[0][i]:before[0][i + 1]].tolist()
    assert mt.lib.mt_delta_log_reset_docs(mt.h, 1, _p(np.array([len(flags)], dtype=np.uint32))) == E_INVALID
    # two batches on logs that hold everything
    fx, interner, a = _arrays("ref_small")
    n = len(fx["docs"])
    b1, b2 = gu.batches_to(a, fx["docs"], [[30, len(d["msgs"])] for d in fx["docs"]])
    mt = _handle(n, **TIERS["paged"])
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(b1)
    have = np.diff(mt.get_delta_logs()[0])
    half = np.arange(0, n, 2, dtype=np.uint32)
    mt.delta_log_reset_docs(half)
    off, words, flags = mt.get_delta_logs()
    assert (np.diff(off)[half] == 0).all() and np.array_equal(np.diff(off)[1::2], have[1::2]) and not flags.any()
    mt.apply_arrays(b2)
    off, words, flags = mt.get_delta_logs()
    for i, doc in enumerate(fx["docs"]):
        want = gu.expected(doc, interner)["deltas"]
        assert words[off[i]:off[i + 1]].tolist() == (want[have[i]:] if i % 2 == 0 else want), i
