"""Bulk segment walk and text in a remote (refSeq, client) view (mt_walk_segments_view,
MergeTreeBatch.walk_segments(ref_seq=, client=) / get_texts_view / last_walk_view):
MergeTree.mapRange({leaf}, refSeq, clientId, accum, start, end) and
MergeTreeTextHelper.getText(refSeq, clientId, placeholder, start, end) for many queries.

Expected values are the reference's own (tests/golden/ref_view_walk.json.gz, made by
tests/golden/make_view_walk.py: at every checkpoint the segment table with insert / removal stamps
and overlap lists, the tree's child counts, and per sampled view getLength, the leaves' nodeLength
sum, mapRange's visits for a query list and getText for some of them).  tests/view_walk_util.py
restates the rules over rows; the first test pins the restatement on the reference.

One cross-check holds for N == L views only and is asserted for those: locate_segments at a
visited row's position names that row at offset 0.  In a stale view with N != L the reference's
own searchBlock does not find every row at the pos nodeMap hands the leaf action (212 of the
fixture's 5301 such rows: a later block of negative length shortens what is left of pos); the CPU
test counts them so that the restriction is a measured one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch   # before the replay library loads: both then share one HIP runtime (as in bench.py)

import golden_util as gu
import view_walk_util as vu
import walk_util

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = -(1 << 31)          # MT_RSEQ_NONE
NOTHING = 0xFFFFFFFF       # mt_walk_row.text / .props: nothing there
HOST = 1                   # MT_WALK_HOST

# the storage tiers of tests/test_bulk_walk.py, copied
TIERS = {"lds": dict(lds_seg_capacity=0, page_capacity=-1), "hbm": dict(lds_seg_capacity=-1, page_capacity=-1),
         "paged": dict(lds_seg_capacity=-1, page_capacity=256, unsettled_capacity=2048, page_heap_capacity=2048),
         "tight": dict(lds_seg_capacity=16, page_capacity=256, unsettled_capacity=2048, page_heap_capacity=2048,
                       lds_page_capacity=24, lds_unsettled_capacity=40, lds_page_heap_capacity=40),
         "narrow": dict(lds_seg_capacity=16, page_capacity=256, unsettled_capacity=2048,
                        page_heap_capacity=2048, lds_page_capacity=200, lds_unsettled_capacity=600,
                        lds_page_heap_capacity=600, lds_narrow_overlap=1),
         "grow": dict(lds_seg_capacity=16, page_capacity=12, unsettled_capacity=16, page_heap_capacity=16),
         "hm": dict(lds_seg_capacity=-1, page_capacity=1600, unsettled_capacity=2048, page_heap_capacity=2048)}
ALL_TIERS = ["lds", "hbm", "paged", "tight", "narrow", "grow", "hm"]
WIDE_TIERS = ["paged", "tight", "narrow", "grow", "hm"]     # 64-bit masks with overflow sets behind them

_fx = {}


def _fixture():
    """The fixture with each document's messages put back from where they came (cut at the
    document's last checkpoint), the reference shared by every test and left unchanged."""
    if not _fx:
        fx = gu.load("ref_view_walk")
        logs = {log["doc"]: log for log in vu.logs()}
        for d in fx["docs"]:
            log = logs[d["doc"]]
            assert [cp["n"] for cp in d["checkpoints"]] == log["checkpoints"] and d["source"] == log["source"]
            d["seed_text"], d["msgs"] = log["seed_text"], log["msgs"][:log["checkpoints"][-1]]
        _fx["fx"] = fx
    return _fx["fx"]


def _view(v):
    return (v["refSeq"], v["client"])


# ---------------------------------------------------------------- 1. the rules, on the reference
def test_view_rules_equal_the_reference_and_the_fixture_holds_every_class():
    """Over the reference's own tables: the tree rule (nodeMap on partial lengths) equals every
    recorded visit list, the flat rule equals it in every N == L view, the text rule equals every
    recorded text, sum pl / sum vl are the recorded N / L; and the fixture holds the classes the
    device tests rely on (asserted, so that none is silently absent)."""
    fx = _fixture()
    c = dict(obs_unseen=0, obs_only=0, own_insert=0, own_remove=0, overlap_only=0, overflow=0, tree_differs=0,
             reversed_hit=0, inside=0, boundary=0, across=0, beyond64=0, empty=0, text_swap=0, open_end=0, stale_views=0,
             host_views=0, host_rows_not_found=0, host_rows=0)
    shapes = dict(flat=0, paged=0, big=0, wide=0)
    for d in fx["docs"]:
        last = d["checkpoints"][-1]
        shapes["wide"] += d["source"] == "ref_wide400"
        shapes["flat"] += d["source"] == "walk_streams" and 5 <= len(last["segs"]) <= 64
        shapes["paged"] += d["source"] == "walk_streams" and 174 <= len(last["segs"]) <= 704
        shapes["big"] += len(last["segs"]) >= 3000 and len(last["levels"][1]) > 64
        for cp in d["checkpoints"]:
            rows, lv = cp["segs"], cp["levels"]
            assert sum(lv[0]) == len(rows) and len(lv[-1]) == 1
            for a, b in zip(lv, lv[1:]):
                assert sum(b) == len(a)
            for r in rows:
                assert (r[vu.TEXT] is None) == (r[vu.RTYPE] is not None)
                assert r[vu.TEXT] is None or len(r[vu.TEXT]) == r[vu.LEN]
            page, at = [], 0            # each row's level-1 node
            for p, blocks in enumerate(lv[1] if len(lv) > 1 else [len(lv[0])]):
                n = sum(lv[0][at:at + blocks])
                page += [p] * n
                at += blocks
            wide_ovl = len({o for r in rows for o in r[vu.OVL]}) > 63      # more overlap clients than mask slots
            assert cp["views"][0]["refSeq"] is None
            for v in cp["views"]:
                view = _view(v)
                r_, c_ = view
                t = vu.View(rows, lv, view)
                vl = t.vl
                assert (t.N, t.L) == (v["N"], v["L"]), (d["doc"], cp["n"], view)
                remote = r_ is not None
                assert not remote or cp["minSeq"] <= r_ <= cp["currentSeq"]
                flat_ok = v["N"] == v["L"]
                assert flat_ok or v["stale"]        # a view at or above the writer's latest refSeq has N == L
                c["stale_views"] += v["stale"]
                c["host_views"] += not flat_ok
                if remote:
                    for row, n in zip(rows, vl):
                        ins, gone = vu.vis(row, view)
                        c["obs_only"] += row[vu.RSEQ] is None and row[vu.LEN] > 0 and not ins and row[vu.CLI] != c_
                        by_seq = row[vu.RSEQ] is not None and row[vu.RSEQ] <= r_
                        if row[vu.RSEQ] is not None and ins and not by_seq:
                            own, ovl = row[vu.RCLI] == c_, c_ in row[vu.OVL]
                            c["own_remove"] += own and not ovl
                            c["overlap_only"] += ovl and not own
                            c["overflow"] += ovl and not own and wide_ovl
                found = set()
                for start, end, visits in v["walks"]:
                    got = t.tree_walk(start, end)
                    assert got == visits, (d["doc"], cp["n"], view, start, end, got[:3], visits[:3])
                    flat = t.flat_walk(start, end)
                    if flat_ok:
                        assert flat == visits, (d["doc"], cp["n"], view, start, end, flat[:3], visits[:3])
                    else:
                        c["tree_differs"] += flat != visits
                    vr = [x[0] for x in visits]
                    c["empty"] += not visits
                    c["open_end"] += end is None
                    if remote:
                        c["obs_unseen"] += sum(rows[i][vu.RSEQ] is not None for i in vr)
                        c["own_insert"] += sum(rows[i][vu.CLI] == c_ and rows[i][vu.SEQ] > r_ for i in vr)
                    if start is not None and start == end and 0 < start < v["L"] and flat_ok:
                        c["inside"] += len(visits) == 1 and 0 < visits[0][2] < rows[vr[0]][vu.LEN]
                        c["boundary"] += not visits
                    if start is not None and end is not None and start > end:
                        c["reversed_hit"] += len(visits) == 1
                    if remote and visits and start is not None and end is not None and start < end:
                        ps = {page[i] for i in vr}
                        c["across"] += len(ps) > 1
                        c["beyond64"] += min(ps) >= 64
                    for i, p, _, _ in visits:
                        if (i, p) not in found:
                            found.add((i, p))
                            hit = t.tree_search(p) == (i, 0)
                            assert hit or not flat_ok, (d["doc"], cp["n"], view, i, p)
                            c["host_rows"] += not flat_ok
                            c["host_rows_not_found"] += not hit
                for i, ph, text in v["texts"]:
                    start, end, visits = v["walks"][i]
                    assert vu.text_of(rows, visits, ph) == text, (d["doc"], cp["n"], view, start, end)
                    c["text_swap"] += any(rows[x][vu.TEXT] is not None and e < s_ and
                                          walk_util.clipped(rows[x][vu.TEXT], s_, e) != "" for x, _, s_, e in visits)
    for k, n in c.items():
        assert n >= (1 if k == "beyond64" else 10), (k, c)
    assert shapes["flat"] >= 12 and shapes["paged"] >= 4 and shapes["big"] >= 1 and shapes["wide"] == 1, shapes


def test_view_walk_fixture_is_the_streams():
    """Every document of the fixture is one of view_walk_util.logs(), with its checkpoints."""
    fx = _fixture()
    assert [d["doc"] for d in fx["docs"]] == [log["doc"] for log in vu.logs()]


def test_view_walk_symbols_exported_and_bound():
    import ctypes
    from fluidframework_amd import build, _native, MergeTreeBatch
    build.build()
    lib = _native.load()
    P, U32, U64, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    walk = [P, U32, P, P, P, P, P, U32, P, P, P, P, U64, P, U64, P, U64]
    want = {"mt_walk_segments_view": walk, "mt_walk_segments_view_device": walk, "mt_last_walk_view": [P, P, P]}
    sigs = {s[0]: s for s in _native.SIGNATURES}
    for name, args in want.items():
        assert hasattr(lib, name) and name in sigs, name
        assert sigs[name][1] is I and list(sigs[name][2]) == args, name
    assert _native.MT_WALK_HOST == 1
    for name in ("last_walk_view", "get_texts_view"):
        assert callable(getattr(MergeTreeBatch, name))


# ---------------------------------------------------------------- helpers of the device tests
def _batch(n_docs, **kw):
    from fluidframework_amd import MergeTreeBatch
    kw.setdefault("seg_capacity", 8192)
    kw.setdefault("text_capacity", 1 << 17)
    return MergeTreeBatch(n_docs, **kw)


def _cuts(doc, k):
    cps = [cp["n"] for cp in doc["checkpoints"]]
    cuts = set(cps)
    fill = (n for n in range(1, len(doc["msgs"])) if n not in cuts)
    while len(cuts) < k:
        cuts.add(next(fill))
    return sorted(cuts)


def _replay_slices(tier, wide, **kw):
    """The fixture's walk_streams documents (or, wide, its ref_wide400 one) replayed on a tier in
    slices that end at the checkpoints: yields (mt, interner, [(doc index, checkpoint)] reached)."""
    docs = [d for d in _fixture()["docs"] if (d["source"] == "ref_wide400") == wide]
    interner = gu.Interner()
    a = gu.encode_docs(dict(docs=docs), interner)
    k = max(len(d["checkpoints"]) for d in docs)
    cuts = [_cuts(d, k) for d in docs]
    mt = _batch(len(docs), **dict(TIERS[tier], **kw))
    mt.load_initial_text(a["seed_off"], a["seed"])
    for j, part in enumerate(gu.batches_to(a, docs, cuts)):
        mt.apply_arrays(part)
        assert (mt.status() == 0).all(), mt.status()
        at = [(i, cp) for i, d in enumerate(docs) for cp in d["checkpoints"] if cp["n"] == cuts[i][j]]
        yield mt, interner, at


def _queries(at):
    """Every view's queries of the checkpoints reached, as one call's columns; the replica's own
    view asks as client 0."""
    q = dict(doc=[], start=[], end=[], ref=[], cli=[], visits=[], cp=[], view=[], text=[])
    for i, cp in at:
        for v in cp["views"]:
            texts = {j: (ph, text) for j, ph, text in v["texts"]}
            for j, (start, end, visits) in enumerate(v["walks"]):
                q["doc"].append(i), q["start"].append(start), q["end"].append(end), q["visits"].append(visits)
                q["ref"].append(0 if v["refSeq"] is None else v["refSeq"]), q["cli"].append(v["client"])
                q["cp"].append(cp), q["view"].append(v), q["text"].append(texts.get(j))
    return q


def _walk(mt, q, **kw):
    return mt.walk_segments(q["doc"], q["start"], q["end"], ref_seq=q["ref"], client=q["cli"], **kw)


def _split(res):
    """walk_segments' result as per-query lists [(rows, texts, props)] (tests/test_bulk_walk.py)."""
    row_off, rows, text_off, units, word_off, recs = res
    raw, words = units.tobytes(), recs.tolist()
    out = []
    for q in range(len(row_off) - 1):
        rs = rows[int(row_off[q]):int(row_off[q + 1])]
        t0, w0 = int(text_off[q]), int(word_off[q])
        texts, props = [], []
        for r in rs:
            if r["text"] == NOTHING:
                texts.append(None)
            else:
                lo = t0 + int(r["text"])
                assert lo + int(r["length"]) <= int(text_off[q + 1])
                texts.append(raw[2 * lo: 2 * (lo + int(r["length"]))].decode("utf-16-le", errors="surrogatepass"))
            if r["props"] == NOTHING:
                props.append(None)
            else:
                w = w0 + int(r["props"])
                assert w + 1 + 2 * words[w] <= int(word_off[q + 1])
                props.append(tuple(words[w + 1: w + 1 + 2 * words[w]]))
        out.append((rs, texts, props))
    return out


def _decode(props, interner, cache):
    if props is None:
        return None
    if props not in cache:
        cache[props] = {interner.key_name(props[j]): interner.val_value(props[j + 1]) for j in range(0, len(props), 2)}
    return cache[props]


def _check_reference(mt, interner, q, res):
    """Every query's records against the reference's visits and segment table, field by field;
    the host flag against N != L; the texts against getText; an undefined end against the view's
    length; the N == L remote rows against locate_segments."""
    per = _split(res)
    assert len(per) == len(q["doc"])
    cache = {}
    loc = dict(doc=[], pos=[], ref=[], cli=[], uid=[])
    host_want = 0
    for (rs, texts, props), d, visits, cp, v, start, end in zip(per, q["doc"], q["visits"], q["cp"], q["view"],
                                                                q["start"], q["end"]):
        got = np.stack([rs["row"], rs["position"], rs["start"], rs["end"]], axis=1).tolist() if len(rs) else []
        assert got == visits, (d, cp["n"], _view(v), start, end, got[:3], visits[:3])
        host = v["N"] != v["L"]
        host_want += host
        assert (rs["flags"] == (HOST if host else 0)).all(), (d, cp["n"], _view(v), start, end)
        for r, text, pr in zip(rs, texts, props):
            ln, seq, cli, _, _, _, rt, rprops, rtext = cp["segs"][int(r["row"])]
            assert (int(r["length"]), int(r["seq"]), int(r["client"])) == (ln, seq, cli), (d, cp["n"], r)
            assert int(r["marker_ref_type"]) == (-1 if rt is None else rt)
            assert text == rtext, (d, cp["n"], int(r["row"]), text, rtext)
            assert _decode(pr, interner, cache) == rprops, (d, cp["n"], int(r["row"]), pr, rprops)
        if end is None and len(rs):
            assert (rs["end"] + rs["position"] == v["N"]).all()
        if v["refSeq"] is not None and not host and len(rs):
            n = len(rs)
            loc["doc"] += [d] * n
            loc["ref"] += [v["refSeq"]] * n
            loc["cli"] += [v["client"]] * n
            loc["pos"] += rs["position"].tolist()
            loc["uid"] += rs["uid"].tolist()
    assert mt.last_walk_view()[:2] == (len(q["doc"]), host_want)
    # the table-based page seek: every remote query of a paged document that the device answered
    paged = {d: mt.is_paged(d) for d in set(q["doc"])}
    skipped = sum(paged[d] and v["refSeq"] is not None and v["N"] == v["L"] for d, v in zip(q["doc"], q["view"]))
    assert mt.last_walk_view()[2] == (0 if os.environ.get("MT_LOCATE_ROW_WALK") == "1" else skipped)
    assert len(loc["doc"]) > 0
    hits = mt.locate_segments(loc["doc"], loc["pos"], loc["ref"], loc["cli"])
    assert np.array_equal(hits["uid"], np.asarray(loc["uid"], dtype=np.uint32)) and not hits["offset"].any()
    # getText: the queries the reference answered
    ask = [j for j, t in enumerate(q["text"]) if t is not None]
    for ph in ("", " "):
        js = [j for j in ask if q["text"][j][0] == ph]
        got = mt.get_texts_view([q["doc"][j] for j in js], [q["start"][j] for j in js], [q["end"][j] for j in js],
                                [q["ref"][j] for j in js], [q["cli"][j] for j in js], placeholder=ph)
        assert got == [q["text"][j][1] for j in js]
    # an undefined end is get_view_lengths_bulk's value
    remote = [j for j, v in enumerate(q["view"]) if v["refSeq"] is not None and q["end"][j] is None]
    lens = mt.get_view_lengths_bulk([q["doc"][j] for j in remote], [q["ref"][j] for j in remote],
                                    [q["cli"][j] for j in remote])
    assert lens.tolist() == [q["view"][j]["N"] for j in remote]
    return per


# ---------------------------------------------------------------- 2. reference parity
@pytest.mark.gpu
@pytest.mark.parametrize("tier", ALL_TIERS)
def test_view_walk_matches_reference(tier):
    """The walk_streams documents replayed in slices that end at their checkpoints: at every
    checkpoint one call for every view's queries of all documents (documents and views repeat
    throughout the call) equals what the reference's mapRange handed its leaf action; the queries
    flagged MT_WALK_HOST are exactly those of the N != L views."""
    final = 0
    for mt, interner, at in _replay_slices(tier, False):
        q = _queries(at)
        _check_reference(mt, interner, q, _walk(mt, q))
        assert all(x > 0 for x in mt.last_walk_view()[3:])
        final = at
    assert len(final) == sum(d["source"] == "walk_streams" for d in _fixture()["docs"])
    big = next(i for i, cp in final if len(cp["segs"]) >= 3000)
    raw, hdr = mt.debug_raw(big)
    if tier in ("paged", "hm", "tight", "narrow", "grow"):
        assert hdr[24] and hdr[25] > 64, hdr[25]
    else:
        assert not hdr[24] and len(raw) > 64


@pytest.mark.gpu
@pytest.mark.parametrize("tier", WIDE_TIERS)
def test_view_walk_wide_document_matches_reference(tier):
    """The ref_wide400 document (200 writers, concurrent removes) on the tiers with 64-bit masks:
    rows gone by overlap membership alone, with the list in an overflow set where the clients
    outnumber the slots; the narrow tier hands the document on with its sets live."""
    for mt, interner, at in _replay_slices(tier, True):
        q = _queries(at)
        _check_reference(mt, interner, q, _walk(mt, q))
    assert mt.is_paged(0)
    assert mt.get_overlap_arena(0)["largest_set"] >= 2        # overflow sets were made


def _final(tier="paged", wide=False):
    for mt, interner, at in _replay_slices(tier, wide):
        pass
    return mt, interner, _queries(at)


def _flat(res):
    row_off, rows, text_off, units, word_off, recs = res
    return dict(row_off=row_off.tolist(), text_off=text_off.tolist(), word_off=word_off.tolist(),
                rows=np.stack([rows[k].astype(np.int64) for k in rows.dtype.names], axis=1).tolist() if len(rows) else [],
                text=units.tolist(), records=recs.tolist())


# ---------------------------------------------------------------- 3. page skip equals row walk
def _stream_queries(mt, docs):
    """Views and ranges for documents no fixture holds answers for ([msgs applied] per document):
    the last four writers (short ids: order of first appearance, as the encoder numbers them),
    each at its latest refSeq, currentSeq, minSeq, the one below its latest and the middle of the
    window; the whole document, eight windows of about 60 positions, one empty range inside."""
    q = dict(doc=[], start=[], end=[], ref=[], cli=[])
    for d, msgs in enumerate(docs):
        hdr = mt.debug_raw(d)[1]
        cur, low = int(hdr[3]), int(hdr[4])
        short, latest = {}, {}
        for m in msgs:
            k = short.setdefault(m[0], len(short) + 1)
            latest.pop(k, None)
            latest[k] = m[2]
        views = []
        for k in list(latest)[-4:]:
            for r in dict.fromkeys([latest[k], cur, low, latest[k] - 1, (cur + low) // 2]):
                if low <= r <= cur:
                    views.append((r, k))
        lens = mt.get_view_lengths_bulk([d] * len(views), [r for r, _ in views], [c for _, c in views]).tolist()
        for (r, c), n in zip(views, lens):
            ranges = [(0, None), (n // 2, n // 2)] + [(j * n // 8, j * n // 8 + 60) for j in range(8)]
            for s_, e in ranges:
                q["doc"].append(d), q["start"].append(max(s_, 0)), q["end"].append(e), q["ref"].append(r), q["cli"].append(c)
    return q


def _digest(res):
    import hashlib
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in res)).hexdigest()


def _skip_results(tier):
    """What the page-skip test compares between the two settings, per group of streams: the
    digest of one walk_segments call for every view and range, its rows, and last_walk_view's
    (queries, host-answered, page skips), with the remote queries on paged documents."""
    out = []

    def record(name, mt, q):
        res = _walk(mt, q)
        paged = {d: mt.is_paged(d) for d in set(q["doc"])}
        remote_paged = sum(paged[d] and c != 0 for d, c in zip(q["doc"], q["cli"]))
        host = np.zeros(len(q["doc"]), dtype=bool)
        for j in range(len(q["doc"])):
            host[j] = (res[1][int(res[0][j]):int(res[0][j + 1])]["flags"] == HOST).any()
        out.append(dict(name=name, digest=_digest(res), rows=len(res[1]), last=list(mt.last_walk_view()[:3]),
                        remote_paged=remote_paged, host_rows=int(host.sum()), all_paged=all(paged.values())))

    # the fixture's streams, every sampled view at every checkpoint
    for wide in (False, True):
        for j, (mt, interner, at) in enumerate(_replay_slices(tier, wide)):
            record(f"fixture wide={wide} slice {j}", mt, _queries(at))
    # ref_zam_shrink, and both ref_wide400 streams at several cut points (inputs only)
    for name, cuts in (("ref_zam_shrink", [5000]), ("ref_wide400", [400, 1100, 2200, 3000])):
        fx = gu.load(name)
        docs = fx["docs"]
        interner = gu.interner_for(fx)
        a = gu.encode_docs(fx, interner)
        mt = _batch(len(docs), **TIERS[tier])
        mt.load_initial_text(a["seed_off"], a["seed"])
        assert cuts[-1] == len(docs[0]["msgs"])
        for cut, part in zip(cuts, gu.batches_to(a, docs, [cuts] * len(docs))):
            mt.apply_arrays(part)
            assert (mt.status() == 0).all()
            record(f"{name} cut {cut}", mt, _stream_queries(mt, [d["msgs"][:cut] for d in docs]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["paged", "tight", "grow", "hm"])
def test_view_walk_page_skip_equals_row_walk(tier):
    """Every sampled view of the fixture's streams at every checkpoint, ref_zam_shrink, and the
    ref_wide400 streams at four cut points: a child process that runs with MT_LOCATE_ROW_WALK=1
    (every remote walk starts at row 0 and takes N and L from the rows) gives this process's
    results byte for byte, offsets and host-answered queries included, while here
    last_walk_view() shows the table-based seek taken by every remote query of a paged document
    that the device answered, and there by none."""
    mine = _skip_results(tier)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "row-walk", tier], capture_output=True, text=True,
                         timeout=300, env=dict(os.environ, MT_LOCATE_ROW_WALK="1", PYTHONPATH=os.pathsep.join(
                             [REPO, os.path.join(REPO, "tests")] + os.environ.get("PYTHONPATH", "").split(os.pathsep))))
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got["walk"] == "1" and len(got["res"]) == len(mine)
    skips = 0
    for a, b in zip(mine, got["res"]):
        assert (a["name"], a["digest"], a["rows"], a["last"][:2]) == (b["name"], b["digest"], b["rows"], b["last"][:2]), (a, b)
        assert b["last"][2] == 0, b
        # (a host-answered query without rows is still host-answered: the count bounds it)
        assert a["remote_paged"] - a["last"][1] <= a["last"][2] <= a["remote_paged"] - (a["host_rows"] if a["all_paged"] else 0), a
        if a["all_paged"]:
            assert a["last"][2] == a["remote_paged"] - a["last"][1], a
        skips += a["last"][2]
        assert a["rows"] > 100
    assert skips > 1000, skips


def _row_walk_child(tier):
    print(json.dumps(dict(walk=os.environ.get("MT_LOCATE_ROW_WALK"), res=_skip_results(tier))))


# ---------------------------------------------------------------- 4. the replica's own view, subsets, the device form
@pytest.mark.gpu
def test_view_walk_own_view_what_subsets_and_device_form():
    """client 0 and NULL view arrays equal mt_walk_segments byte for byte; rows only, text only
    and props only give the same rows; the _device form equals the host form, offsets and the
    host-answered queries' slots included."""
    from fluidframework_amd import _native
    mt, interner, q = _final()
    plain = mt.walk_segments(q["doc"], q["start"], q["end"])
    lib, h = mt.lib, mt.h
    docs = np.asarray(q["doc"], dtype=np.uint32)
    start = np.asarray([0 if s is None else s for s in q["start"]], dtype=np.int32)
    end = np.asarray([-1 if e is None else e for e in q["end"]], dtype=np.int32)
    n = len(docs)
    for ref, cli in ((np.asarray(q["ref"], dtype=np.int32), np.zeros(n, dtype=np.int32)), (None, None)):
        offs = [np.zeros(n + 1, dtype=np.int64) for _ in range(3)]
        rows = np.zeros(len(plain[1]), dtype=_native.WALK_ROW_DTYPE)
        text, recs = np.zeros(len(plain[3]), dtype=np.uint16), np.zeros(len(plain[5]), dtype=np.uint32)
        rc = lib.mt_walk_segments_view(h, n, _native.ptr(docs), _native.ptr(start), _native.ptr(end), _native.ptr(ref),
                                       _native.ptr(cli), 3, _native.ptr(offs[0]), _native.ptr(offs[1]),
                                       _native.ptr(offs[2]), _native.ptr(rows), len(rows), _native.ptr(text), len(text),
                                       _native.ptr(recs), len(recs))
        assert rc == 0, lib.mt_last_error(h).decode()
        for a, b in zip((offs[0], rows, offs[1], text, offs[2], recs), plain):
            assert a.tobytes() == b.tobytes()
        assert mt.last_walk_view()[:3] == (n, 0, 0)      # (the replica's own view: no remote query, no table seek)
    # what subsets, in the views
    full = _walk(mt, q)
    row_off, rows, text_off, units, word_off, recs = full
    assert (rows["flags"] == HOST).any() and (rows["flags"] == 0).any()
    names = [k for k in rows.dtype.names if k not in ("text", "props")]
    for text, props in ((False, False), (True, False), (False, True)):
        r_off, r, t_off, t, w_off, w = _walk(mt, q, text=text, props=props)
        assert np.array_equal(r_off, row_off)
        for k in names:
            assert np.array_equal(r[k], rows[k]), k
        if text:
            assert np.array_equal(t_off, text_off) and np.array_equal(t, units) and np.array_equal(r["text"], rows["text"])
        else:
            assert not t_off.any() and len(t) == 0 and (r["text"] == NOTHING).all()
        if props:
            assert np.array_equal(w_off, word_off) and np.array_equal(w, recs) and np.array_equal(r["props"], rows["props"])
        else:
            assert not w_off.any() and len(w) == 0 and (r["props"] == NOTHING).all()
    # the device form
    dev = mt.walk_segments_device(q["doc"], q["start"], q["end"], ref_seq=q["ref"], client=q["cli"])
    assert all(t.is_cuda for t in dev)
    host = [t.cpu().numpy() for t in dev]
    assert np.array_equal(host[0], row_off) and np.array_equal(host[2], text_off) and np.array_equal(host[4], word_off)
    assert np.array_equal(host[1].view(_native.WALK_ROW_DTYPE).reshape(-1), rows)
    assert np.array_equal(host[3].view(np.uint16), units) and np.array_equal(host[5].view(np.uint32), recs)
    assert mt.last_walk_view()[1] > 0


# ---------------------------------------------------------------- 5. arguments
@pytest.mark.gpu
def test_view_walk_arguments():
    """One of the two view arrays alone and a negative client (MT_E_INVALID before any launch), a
    refSeq outside the window (MT_E_INVALID, the query named), the sizing call, each capacity one
    short (MT_E_OVERFLOW, nothing written), n == 0."""
    from fluidframework_amd import _native
    mt, interner, q = _final()
    lib, h = mt.lib, mt.h
    want = _walk(mt, q)
    docs = np.asarray(q["doc"], dtype=np.uint32)
    start = np.asarray([0 if s is None else s for s in q["start"]], dtype=np.int32)
    end = np.asarray([-1 if e is None else e for e in q["end"]], dtype=np.int32)
    ref, cli = np.asarray(q["ref"], dtype=np.int32), np.asarray(q["cli"], dtype=np.int32)
    n = len(docs)
    offs = [np.full(n + 1, -1, dtype=np.int64) for _ in range(3)]

    def call(rows=None, cap_rows=0, text=None, cap_text=0, recs=None, cap_words=0, docs=docs, start=start, end=end,
             ref=ref, cli=cli, n=n):
        rc = lib.mt_walk_segments_view(h, n, _native.ptr(docs), _native.ptr(start), _native.ptr(end), _native.ptr(ref),
                                       _native.ptr(cli), 3, _native.ptr(offs[0]), _native.ptr(offs[1]),
                                       _native.ptr(offs[2]), _native.ptr(rows), cap_rows, _native.ptr(text), cap_text,
                                       _native.ptr(recs), cap_words)
        return rc, lib.mt_last_error(h).decode()

    assert call()[0] == 0                       # sizing only
    assert all(np.array_equal(o, w) for o, w in zip(offs, (want[0], want[2], want[4])))
    nr, nt, nw = (int(o[n]) for o in offs)
    assert (nr, nt, nw) == (len(want[1]), len(want[3]), len(want[5])) and min(nr, nt, nw) > 0
    for short in range(3):
        rows = np.full(nr, 0x55, dtype=np.uint8).repeat(48).view(_native.WALK_ROW_DTYPE)
        text = np.full(nt, 0x5555, dtype=np.uint16)
        recs = np.full(nw, 0x55555555, dtype=np.uint32)
        caps = [nr, nt, nw]
        caps[short] -= 1
        rc, err = call(rows, caps[0], text, caps[1], recs, caps[2])
        assert rc == _native.MT_E_OVERFLOW, (short, rc, err)
        assert all(str(x) in err for x in (nr, nt, nw)) and "mt_walk_segments_view" in err, err
        assert (rows.view(np.uint8) == 0x55).all() and (text == 0x5555).all() and (recs == 0x55555555).all()
    rows = np.zeros(nr, dtype=_native.WALK_ROW_DTYPE)
    text, recs = np.zeros(nt, dtype=np.uint16), np.zeros(nw, dtype=np.uint32)
    assert call(rows, nr, text, nt, recs, nw)[0] == 0
    assert np.array_equal(rows, want[1]) and np.array_equal(text, want[3]) and np.array_equal(recs, want[5])
    # refused before any launch
    two = np.asarray([0, 1], dtype=np.uint32)
    z2 = np.zeros(2, dtype=np.int32)
    cur = [int(mt.debug_raw(d)[1][3]) for d in (0, 1)]
    mins = [int(mt.debug_raw(d)[1][4]) for d in (0, 1)]
    ok = dict(docs=two, start=z2, end=z2 - 1, ref=np.asarray(cur, dtype=np.int32), cli=z2 + 1, n=2)
    for kw, word in ((dict(ref=None), "both"), (dict(cli=None), "both"),
                     (dict(cli=np.asarray([1, -1], dtype=np.int32)), "query 1")):
        for o in offs:
            o[:] = -1
        rc, err = call(**dict(ok, **kw))
        assert rc == _native.MT_E_INVALID and "mt_walk_segments_view" in err and word in err, (kw, rc, err)
        assert all((o == -1).all() for o in offs)
        assert call(**ok)[0] == 0
    # a refSeq outside [minSeq, currentSeq]: the first such query is named; client 0 ignores its refSeq
    for bad in (cur[1] + 1, mins[1] - 1):
        rc, err = call(**dict(ok, ref=np.asarray([cur[0], bad], dtype=np.int32)))
        assert rc == _native.MT_E_INVALID and "query 1" in err and "refSeq " + str(bad) in err, (rc, err)
        assert call(**dict(ok, ref=np.asarray([cur[0], bad], dtype=np.int32), cli=np.asarray([1, 0], dtype=np.int32)))[0] == 0
    with pytest.raises(RuntimeError, match="query 0"):
        mt.walk_segments([0, 1], 0, None, ref_seq=[cur[0] + 7, cur[1]], client=1)
    with pytest.raises(RuntimeError):
        mt.walk_segments([0, 1], 0, None, ref_seq=cur)
    with pytest.raises(ValueError):
        mt.get_texts_view([0], 0, None, cur[0], 1, placeholder="*")
    # n == 0
    res = mt.walk_segments([], [], [], ref_seq=[], client=[])
    assert [len(x) for x in res] == [1, 0, 1, 0, 1, 0] and not any(res[k].any() for k in (0, 2, 4))
    assert mt.last_walk_view() == (0, 0, 0, 0.0, 0.0)
    again = _walk(mt, q)
    assert all(np.array_equal(a, b) for a, b in zip(again, want))


# ---------------------------------------------------------------- 6. failed documents, 7. a live handle
def _self_consistent(mt, d, views, rng):
    """Document d walked in the views (whole, and a few ranges): every visited row of a query the
    device answered is the one locate_segments names at its position, offset 0; positions tile
    the view; an undefined end is get_view_lengths_bulk's value."""
    lens = mt.get_view_lengths_bulk([d] * len(views), [r for r, _ in views], [c for _, c in views]).tolist()
    docs, start, end, ref, cli, n_of = [], [], [], [], [], []
    for (r, c), n in zip(views, lens):
        ranges = [(0, None), (n // 3, n // 3), (n // 2, max(n // 2 - 2, 0))]
        ranges += [tuple(sorted(rng.integers(0, n + 2, 2).tolist())) for _ in range(4)]
        for s, e in ranges:
            docs.append(d), start.append(s), end.append(e), ref.append(r), cli.append(c), n_of.append(n)
    row_off, rows, _, _, _, _ = mt.walk_segments(docs, start, end, ref_seq=ref, client=cli)
    checked = 0
    for j in range(len(docs)):
        rs = rows[int(row_off[j]):int(row_off[j + 1])]
        if not len(rs) or (rs["flags"] == HOST).any():
            continue
        hits = mt.locate_segments([d] * len(rs), rs["position"], ref[j], cli[j])
        assert np.array_equal(hits["uid"], rs["uid"]) and not hits["offset"].any(), (d, j)
        assert np.array_equal(hits["row"], rs["row"])
        if end[j] is None:
            assert (rs["end"] + rs["position"] == n_of[j]).all() and rs["position"][0] == 0
            assert (np.diff(rs["position"]) > 0).all()
        checked += len(rs)
    return checked


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["lds", "paged"])
def test_view_walk_failed_documents_answer_from_where_they_stopped(tier):
    fx = gu.load("ref_errors")
    interner = gu.interner_for(fx)
    a = gu.encode_docs(fx, interner)
    mt = _batch(len(fx["docs"]), **TIERS[tier])
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    failed = np.flatnonzero(mt.status() != 0)[:6].tolist()
    assert failed
    rng = np.random.default_rng(5)
    checked = 0
    for d in failed:
        hdr = mt.debug_raw(d)[1]
        cur, low = int(hdr[3]), int(hdr[4])
        checked += _self_consistent(mt, d, [(cur, 1), (low, 2), ((cur + low) // 2, 1), (0, 0)], rng)
    assert checked > 0 and (mt.status() != 0).sum() >= len(failed)


def _msg(ev):
    _, cid, seq, ref, msn, op = ev
    return dict(clientId=cid, sequenceNumber=seq, referenceSequenceNumber=ref, minimumSequenceNumber=msn,
                type="op", contents=op)


@pytest.mark.gpu
def test_view_walk_live_handle():
    """ref_live replayed through LiveClient: at its reconnects (unacked inserts in, pending
    removes out) and after its last event the walk in remote writers' views is consistent with
    locate_segments and get_view_lengths_bulk in the same views."""
    from fluidframework_amd.live import LiveClient
    from fluidframework_amd.wire import Interner
    doc = gu.load("ref_live")["docs"][0]
    lc = LiveClient(doc["seed_text"], interner=Interner(synthetic=True), seg_capacity=16384, text_capacity=1 << 17)
    lc.startOrUpdateCollaboration("local-0")
    rng = np.random.default_rng(11)
    state = dict(checked=0, rows=0)

    def check():
        hdr = lc.mt.debug_raw(0)[1]
        cur, low = int(hdr[3]), int(hdr[4])
        state["rows"] += _self_consistent(lc.mt, 0, [(cur, 1), (cur, 2), (low, 1), (0, 0)], rng)
        state["checked"] += 1

    unseq = []
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
            if state["checked"] < 2 and lc.pendingCounts()[1] > 0:
                check()
            lc.startOrUpdateCollaboration(ev[1])
            unseq = [lc.regeneratePendingOp(o) for o in unseq]
    lc.flush()
    check()
    assert state["checked"] >= 2 and state["rows"] > 0, state


if __name__ == "__main__" and sys.argv[1:2] == ["row-walk"]:
    _row_walk_child(sys.argv[2])
