"""Shared by the summary-extraction tests (test_extract.py on the CPU, test_snapshot_extract.py
and test_snapshot_roundtrip.py on the GPU): extracted records in a comparable form, the
summary text of an extraction, and the hand-built documents of the extraction cases."""
import numpy as np

from fluidframework_amd.snapshot import F_MARKER, NO_PROPS, encode_chunks, record_specs

REC_FIELDS = ("len", "seq", "removed_seq", "client", "removed_client", "flags")
FILLER = 24              # Doc(filler=...): three leaf blocks of "\n" segments ahead of a case


def chunks_of(ex, interner, names, chunk):
    """The summary blobs ({path: JSON text}) of one document's extraction (a dict as
    OracleDoc.extract / MergeTreeBatch.extract_snapshots give it)."""
    specs, lengths = record_specs(ex["segs"], ex["text"], ex["props"], interner, names)
    return encode_chunks(specs, lengths, ex["min_seq"], ex["cur_seq"], chunk)


def split_raw(raw):
    """extract_snapshots_raw's layout -> one dict per document (offsets are per document)."""
    counts, recs, text, props, mn, cu = raw
    out = []
    r0 = t0 = p0 = 0
    for d in range(len(counts)):
        nr, nt, npr = (int(x) for x in counts[d])
        out.append(dict(segs=recs[r0:r0 + nr], text=text[t0:t0 + nt], props=props[p0:p0 + npr],
                        min_seq=int(mn[d]), cur_seq=int(cu[d])))
        r0, t0, p0 = r0 + nr, t0 + nt, p0 + npr
    return out


def norm_doc(ex):
    """One document's extraction as comparable values: the window, the counts, and per record
    every mt_seg_rec field (payload: a marker's refType; a text record's offset is checked as
    the running text length), its text slice and its property pairs sorted by key id (the
    device keeps a set in its storage order; the byte-exact order is pinned on the CPU against
    the reference's summaries).  Offsets must tile the arenas: text and props are consumed in
    record order without gaps."""
    recs = []
    t_at = p_at = 0
    for r in ex["segs"]:
        row = [int(r[f]) for f in REC_FIELDS]
        if r["flags"] & F_MARKER:
            row.append(("marker", int(r["payload"])))
        else:
            p0, ln = int(r["payload"]), int(r["len"])
            assert p0 == t_at, ("text offset", p0, t_at)
            row.append(("text", np.asarray(ex["text"][p0:p0 + ln]).tobytes()))
            t_at += ln
        if int(r["props"]) == NO_PROPS:
            row.append(None)
        else:
            o = int(r["props"])
            assert o == p_at, ("props offset", o, p_at)
            n = int(ex["props"][o])
            row.append(tuple(sorted((int(ex["props"][o + 1 + 2 * j]), int(ex["props"][o + 2 + 2 * j]))
                                    for j in range(n))))
            p_at += 1 + 2 * n
        assert bytes(r["_pad"]) == bytes(7)
        recs.append(tuple(row))
    return dict(window=(ex["min_seq"], ex["cur_seq"]), counts=(len(ex["segs"]), t_at, p_at),
                arenas=(len(ex["text"]), len(ex["props"])), recs=recs)


def diff_docs(got, want):
    """[(doc, what)] where two lists of extractions differ (norm_doc of each)."""
    bad = []
    for d, (g, w) in enumerate(zip(got, want)):
        g, w = norm_doc(g), norm_doc(w)
        for k in ("window", "counts", "arenas"):
            if g[k] != w[k]:
                bad.append((d, k, g[k], w[k]))
        if g["recs"] != w["recs"]:
            i = next((i for i, (a, b) in enumerate(zip(g["recs"], w["recs"])) if a != b), min(len(g["recs"]), len(w["recs"])))
            bad.append((d, "record", i, g["recs"][i:i + 1], w["recs"][i:i + 1]))
    assert len(got) == len(want)
    return bad


# ---------------------------------------------------------------- hand-built documents
class Doc:
    """Messages of one hand-built document: writers "a" / "b" take turns so that neighbouring
    inserts are not merged in the tree before the minimum sequence number passes them
    (zamboni only merges below it), every op at refSeq = seq - 1; settle() ends with a
    non-op message whose minimumSequenceNumber is the last op's sequence number."""

    def __init__(self, seed="", filler=0):
        self.seed = seed
        self.msgs = []
        self.seq = 0
        self.length = len(seed)
        self.msn = 0
        # `filler` one-unit "\n" segments first (none can be appended to): when the minimum
        # sequence number finally moves, zamboni's two scours of that message go to these, the
        # oldest blocks, and the case's own run stays unmerged in the tree -- only the
        # extraction coalesces it
        for _ in range(filler):
            self.append("\n")

    def _msg(self, contents, client=None, typ="op", msn=None, ref=None):
        self.seq += 1
        if msn is not None:
            self.msn = msn
        self.msgs.append(dict(clientId=client or ("a" if self.seq % 2 else "b"), sequenceNumber=self.seq,
                              referenceSequenceNumber=self.seq - 1 if ref is None else ref,
                              minimumSequenceNumber=self.msn, type=typ, contents=contents))
        return self.seq

    def insert(self, pos, text, props=None, **kw):
        seg = text if props is None else {"text": text, "props": props}
        self.length += len(text)
        return self._msg({"pos1": pos, "seg": seg, "type": 0}, **kw)

    def append(self, text, props=None, **kw):
        return self.insert(self.length, text, props, **kw)

    def marker(self, pos, ref_type, props=None, **kw):
        seg = {"marker": {"refType": ref_type}}
        if props is not None:
            seg["props"] = props
        self.length += 1
        return self._msg({"pos1": pos, "seg": seg, "type": 0}, **kw)

    def remove(self, p1, p2, **kw):
        self.length -= p2 - p1
        return self._msg({"pos1": p1, "pos2": p2, "type": 1}, **kw)

    def annotate(self, p1, p2, props, comb=None, **kw):
        op = {"pos1": p1, "pos2": p2, "props": props, "type": 2}
        if comb:
            op["combiningOp"] = comb
        return self._msg(op, **kw)

    def noop(self, msn):
        return self._msg(None, typ="noop", msn=msn)

    def settle(self, msn=None):
        """minSeq := the last op's sequence number (or msn) by one non-op message."""
        self.noop(self.seq if msn is None else msn)


def _run(d, n, unit="x", props=None):
    for i in range(n):
        d.append(unit if isinstance(unit, str) else unit(i), props)


def handbuilt_docs():
    """{case name: Doc} -- the extraction cases (see tests/test_snapshot_extract.py)."""
    docs = {}
    # (a) granularity: canAppend holds when either side is <= 256 units.  Three runs whose
    # running length passes 255 / 256 / 257 (then one more unit), each followed by a 256-unit
    # and then a 257-unit segment; a newline ends each block
    for name, run in (("gran255", 255), ("gran256", 256), ("gran257", 257)):
        d = Doc(filler=FILLER)
        d.append("p" * (run - 3))
        d.append("q")
        d.append("r")
        d.append("s")             # the run is now `run` units long
        d.append("B" * 257)       # joins iff the run is <= 256 units (255, 256: yes; 257: no)
        d.append("A" * 256)       # this side is <= 256: joins whatever the run's length
        d.append("C" * 257)       # prev > 256 and this > 256: a new record
        d.append("D" * 257)       # 257 after 257: a new record again
        d.append("u")             # prev 257 > 256 but this <= 256: joins
        d.settle()
        docs[name] = d
    # (b) newlines
    d = Doc(filler=FILLER)
    d.append("ab")
    d.append("cd\n")              # ends the run: the next segment opens a new record
    d.append("ef")
    d.append("\n")                # a run whose last appended segment is "\n" alone
    d.append("")                  # a zero-length insert (the reference applies nothing)
    d.append("gh")
    d.append("\n")
    d.settle()
    docs["newlines"] = d
    # (c) markers between text, with and without properties
    d = Doc(filler=FILLER)
    d.append("ab")
    d.marker(d.length, 1)
    d.append("cd")
    d.marker(d.length, 2, {"k1": 5})
    d.marker(d.length, 3, {})
    d.append("ef", {"k1": 5})
    d.append("gh", {"k1": 5})
    d.settle()
    docs["markers"] = d
    # (d) property matching: equal sets stored in different key order; {} against none; a
    # value matchProperties never finds equal on both neighbours
    d = Doc(filler=FILLER)
    o = d.length
    d.append("aa")
    d.append("bb")
    d.append("cc")
    d.append("dd", {})            # {} is a property set: no match with `undefined`
    d.append("ee", {})
    d.append("ff")
    d.append("gg", {"k3": "s"})
    d.append("hh", {"k3": "s"})
    d.append("ii", {"k1": 1, "k2": 2})
    d.append("jj", {"k2": 2, "k1": 1})       # the same set, other insertion order
    d.append("kk", {"k1": 1, "k2": 3})       # same keys, one value differs
    d.append("ll", {"k1": 1})                # a subset
    d.annotate(o, o + 2, {"k1": 1})
    d.annotate(o, o + 2, {"k2": 2})              # aa: k1 then k2
    d.annotate(o + 2, o + 4, {"k2": 2})
    d.annotate(o + 2, o + 4, {"k1": 1})              # bb: k2 then k1
    d.annotate(o + 4, o + 6, {"k1": 1})              # cc: k1 only
    d.annotate(o + 12, o + 16, {"k3": 1}, comb={"name": "incr", "defaultValue": 0})   # gg, hh: incr on a string -> NaN
    d.settle()
    docs["props"] = d
    # (e) window edges: seq == minSeq / minSeq + 1, removedSeq == minSeq / minSeq + 1
    d = Doc("0123456789")
    d.append("ab")
    d.append("cd")
    d.remove(0, 2)
    r1 = d.remove(2, 4)           # removedSeq == minSeq: elided
    d.remove(4, 6)                # removedSeq == minSeq + 1: kept, with removal info
    s0 = d.append("ef")           # seq == minSeq + 2 ... see below
    assert r1 + 2 == s0
    d.append("gh")
    d.noop(r1)
    docs["edges_removed"] = d
    d = Doc("0123456789")
    d.append("ab")
    s = d.append("cd")            # seq == minSeq: below the window, coalescible
    d.append("ef")                # seq == minSeq + 1: merge info with seq / client
    d.append("gh")
    d.noop(s)
    docs["edges_inserted"] = d
    # (f) a coalescible run of 40 one-unit segments among others (a page is a level-1 node: at
    # most 7 leaf blocks, 64 segment slots), and one of 140: longer than two whole pages, so it
    # lies over at least two page edges wherever the edges are
    for name, run in (("run40", 40), ("run140", 140)):
        d = Doc("S" * 7, filler=FILLER)
        _run(d, run, lambda i: "abcdefghij"[i % 10])
        d.append("\n")
        _run(d, 9, "z")
        for _ in range(FILLER):
            d.append("\n")
        d.noop(d.seq)             # one message only: zamboni has not merged the run in the tree
        docs[name] = d
    # (g) empty cases
    docs["empty"] = Doc()
    docs["seed_only"] = Doc("seed text\n")
    d = Doc("abcdef")
    d.append("gh")
    d.remove(0, 4)
    d.remove(0, d.length)
    d.settle()
    docs["all_removed"] = d
    return docs


def arena_docs():
    """(h) documents driven through text and property compaction: a run of inserts with
    properties, most of them removed again below the minimum sequence number, again and
    again -- the live text and property sets stay small while the arenas' fill passes their
    capacity several times."""
    d = Doc("seed")
    for rnd in range(48):
        for i in range(6):
            d.append("abcdefghijklmnopqrstuvwxyz012345"[: 20 + i], {"k1": rnd, "k2": i})
        d.annotate(0, 4, {"k3": rnd})
        d.remove(4, d.length - 30)
        d.noop(d.seq)
    d.append("tail", {"k1": 1})
    d.settle()
    return {"arena": d}


def encode(docs, interner=None):
    """wire.Batch of hand-built documents (in dict order): (batch, arrays)."""
    from fluidframework_amd.wire import Batch, Interner
    b = Batch(interner or Interner())
    for d in docs.values():
        b.add_doc(d.seed, d.msgs)
    return b, b.arrays()


# ---------------------------------------------------------------- generated streams
def slice_records(a, lo, hi):
    """The batch holding records [lo, hi) of every document of `a` (clipped to its length;
    hi None: to the end); arenas are shared."""
    off = a["doc_off"]
    idx = []
    for d in range(len(off) - 1):
        n = int(off[d + 1] - off[d])
        h = n if hi is None else min(hi, n)
        idx.append(np.arange(off[d] + min(lo, n), off[d] + h))
    doc_off = np.concatenate([[0], np.cumsum([len(i) for i in idx])]).astype(np.int64)
    return dict(a, ops=a["ops"][np.concatenate(idx)] if idx else a["ops"][:0], doc_off=doc_off)


def generated_stream(oracle_lib, cfg, docs, caps):
    """`docs` documents of `cfg`, generated on the device once and checked against the C
    restatement's replay from the seeds: read-only arrays {ops, doc_off, text, props, seed_off,
    seed} (one record per message)."""
    from fluidframework_amd import MergeTreeBatch
    mt = MergeTreeBatch(docs, delta_log_capacity=0, **caps)
    host = mt.generate(cfg).download()
    seed_off, seed = mt.generated_seeds(cfg)
    a = dict(host, seed_off=seed_off, seed=seed)
    osums, ost = oracle_lib.replay_batch(a, threads=8)
    assert (ost == 0).all()
    assert np.array_equal(mt.checksums(), osums), "the generated state differs from the oracle's replay"
    assert (np.diff(a["doc_off"]) == cfg["ops"]).all()
    for v in a.values():
        v.setflags(write=False)
    mt.close()
    return a


# Words of the 32-word document header that debug_raw returns (mt_device.h: DocHdr is n_seg,
# depth, heap_n, cur_seq, min_seq, text_top, text_half, props_top, props_half, ...; its pad[]
# starts at word 24 and is indexed by HDR_PAGED = 0, HDR_NPAGES = 1)
HDR_TEXT_HALF, HDR_PROPS_HALF = 6, 8
HDR_PAD = 24
HDR_PAGED, HDR_NPAGES = HDR_PAD + 0, HDR_PAD + 1


def doc_header(mt, doc):
    """(text_half, props_half, paged, pages) of a document's header."""
    h = mt.debug_raw(doc)[1]
    assert bool(h[HDR_PAGED]) == mt.is_paged(doc)   # (the binding's own reading of the same word)
    return int(h[HDR_TEXT_HALF]), int(h[HDR_PROPS_HALF]), bool(h[HDR_PAGED]), int(h[HDR_NPAGES])
