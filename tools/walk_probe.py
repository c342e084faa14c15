"""Segment walk probe (GPU box): the setting of tools/tile_probe.py -- C3-shaped streams with
markers (tests/tile_streams.py: p_marker 0.05, 2000 messages; --distinct streams built on the host
and repeated to --docs documents) replayed on the default handle -- then
  (a) one walk_segments call of one whole-document query per document, and one call of
      --per-doc windows of about --window positions per document: wall time and the two kernels'
      times (HIP events, mt_last_walk_ms),
  (b) the same rows the way a caller gets them without the call: per document get_segments +
      get_all_segment_props + get_text and a host scan (the rule of tests/walk_util.py),
  (c) the walk started at the page the directory names for start, and with MT_LOCATE_ROW_WALK=1
      (from row 0),
  (d) rows only against rows, text and property records,
and asserts both sides of (a)/(b) and of (c) equal.  One warm-up, the median of --runs runs.
Writes profiles/readout/bulk_walk.json.
    python tools/walk_probe.py [--docs 4096] [--ops 2000] [--runs 5] [--per-doc 16] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
from readout_probe import HBM_BYTES_PER_S, median_s   # noqa: E402
from tile_probe import handle                          # noqa: E402

NONE = -(1 << 31)
ROW_BYTES = 16 + 16           # segA and segB of one row
QUERY_BYTES = 128 + 3 * 8 + 4 + 3 * 16   # the header, the counts, the end, the offsets of the gather
PAGE_DIR_BYTES = 2 + 12       # a directory entry and its PageMeta
OUT_ROW_BYTES = 48


def host_tables(mt, docs):
    """What a caller fetches today, per document: (observer position, observer length) of every
    row, its text (None: a marker or removed) and property pairs."""
    out = {}
    for d in docs:
        seg, _ = mt.get_segments(d)
        props = mt.get_all_segment_props(d)
        text = mt.get_text(d)
        obs = np.where(seg[:, 3] == NONE, seg[:, 0], 0).astype(np.int64)
        pos = np.cumsum(obs) - obs
        is_text = (seg[:, 6] < 0) & (obs > 0)
        t_at = np.cumsum(np.where(is_text, obs, 0)) - np.where(is_text, obs, 0)
        out[d] = (pos, obs, is_text, t_at, text, props)
    return out


def host_loop(mt, docs, start, end):
    """The visits without the call: each document fetched once, its ranges answered on the host.
    Returns per query (rows, total text units of the visited text rows, record words)."""
    res = [None] * len(docs)
    tables = host_tables(mt, sorted(set(docs.tolist())))
    for q, (d, s, e) in enumerate(zip(docs.tolist(), start.tolist(), end.tolist())):
        pos, obs, is_text, t_at, text, props = tables[d]
        if e < 0:
            e = int(obs.sum())
        vis = np.flatnonzero((obs > 0) & (pos < e) & (pos + obs > s))
        units = int(obs[vis][is_text[vis]].sum())
        words = sum(1 + 2 * len(props[i]) for i in vis.tolist() if props[i] is not None)
        res[q] = (vis, units, words, [text[t_at[i]:t_at[i] + obs[i]] if is_text[i] else None for i in vis.tolist()])
    return res


def check(walk, loop):
    row_off, rows, text_off, units, word_off, recs = walk
    raw = units.tobytes()
    for q, (vis, n_units, n_words, texts) in enumerate(loop):
        rs = rows[int(row_off[q]):int(row_off[q + 1])]
        assert np.array_equal(rs["row"], vis), f"query {q}: rows differ from the host scan"
        assert int(text_off[q + 1] - text_off[q]) == n_units and int(word_off[q + 1] - word_off[q]) == n_words, q
        t0 = int(text_off[q])
        for r, t in zip(rs, texts):
            if t is not None:
                lo = t0 + int(r["text"])
                assert raw[2 * lo:2 * (lo + len(t))].decode("utf-16-le", errors="surrogatepass") == t, q


def kernel_ms(call, last, runs):
    call()
    ms = []
    for _ in range(runs):
        call()
        ms.append(last())
    return [statistics.median(m[i] for m in ms) for i in (0, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--ops", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--per-doc", type=int, default=16)
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "readout", "bulk_walk.json"))
    args = ap.parse_args()
    assert args.runs >= 5
    mt, _ = handle(args.docs, args.ops, args.distinct)
    n = args.docs
    rng = np.random.default_rng(4)
    lengths = mt.get_view_lengths_bulk(np.arange(n))
    step = max(n // 64, 1)
    raws = [mt.debug_raw(d) for d in range(0, n, step)]
    pages = float(np.mean([int(h[25]) for _, h in raws]))
    n_rows = float(np.mean([len(r) for r, _ in raws]))
    paged = sum(int(h[24]) != 0 for _, h in raws)
    res = {}
    for name, per_doc in (("whole_documents", 1), ("windows", args.per_doc)):
        docs = np.repeat(np.arange(n, dtype=np.uint32), per_doc)
        if per_doc == 1:
            start = np.zeros(n, dtype=np.int32)
            end = np.full(n, -1, dtype=np.int32)
        else:
            start = (rng.random(len(docs)) * np.maximum(lengths[docs] - args.window, 1)).astype(np.int32)
            end = np.minimum(start + args.window, lengths[docs]).astype(np.int32)
        got = {}

        def bulk(**kw):
            got["bulk"] = mt.walk_segments(docs, start, end, **kw)

        def loop():
            got["loop"] = host_loop(mt, docs, start, end)

        ab = {}
        for walk in ("0", "1"):
            os.environ["MT_LOCATE_ROW_WALK"] = walk
            bulk()
            ab[walk] = dict(res=got["bulk"], bulk_s=median_s(bulk, args.runs), kernel_ms=kernel_ms(bulk, mt.last_walk, args.runs))
        os.environ["MT_LOCATE_ROW_WALK"] = "0"
        assert all(np.array_equal(a, b) for a, b in zip(ab["0"]["res"], ab["1"]["res"])), "page skip differs from the row walk"
        rows_only_s = median_s(lambda: bulk(text=False, props=False), args.runs)
        rows_only_ms = kernel_ms(lambda: bulk(text=False, props=False), mt.last_walk, args.runs)
        assert np.array_equal(got["bulk"][0], ab["0"]["res"][0])
        loop_s = median_s(loop, args.runs)
        check(ab["0"]["res"], got["loop"])
        row_off, rows, text_off, units, word_off, recs = ab["0"]["res"]
        nq = len(docs)
        # modelled bytes: the rows a walk reads (whole documents: all of them; a window with the
        # page skip: the pages it touches, about two; from row 0: half the document on average)
        # plus the results written
        out_bytes = len(rows) * OUT_ROW_BYTES + len(units) * 2 + len(recs) * 4
        read_rows = {"0": (n_rows if per_doc == 1 else min(n_rows, 2 * n_rows / max(pages, 1.0))) * nq,
                     "1": (n_rows if per_doc == 1 else n_rows / 2) * nq}
        one = {}
        for walk, form in (("0", "page_skip"), ("1", "row_walk")):
            cnt_ms, gat_ms = ab[walk]["kernel_ms"]
            model = int(nq * QUERY_BYTES + 2 * read_rows[walk] * ROW_BYTES + out_bytes + len(units) * 2 + len(recs) * 4 +
                        (nq * min(pages, 64.0) * PAGE_DIR_BYTES * 2 if walk == "0" else 0))
            one[form] = dict(walk_segments_s=ab[walk]["bulk_s"], count_kernel_ms=cnt_ms, gather_kernel_ms=gat_ms,
                             bytes_model=model, bytes_per_s=model / ((cnt_ms + gat_ms) * 1e-3),
                             fraction_of_hbm_8TBps=model / ((cnt_ms + gat_ms) * 1e-3) / HBM_BYTES_PER_S)
        res[name] = dict(queries=nq, rows=int(len(rows)), text_units=int(len(units)), record_words=int(len(recs)),
                         host_loop_s=loop_s, walk_segments_s=ab["0"]["bulk_s"], speedup=loop_s / ab["0"]["bulk_s"], **one,
                         page_skip_kernel_speedup=sum(ab["1"]["kernel_ms"]) / sum(ab["0"]["kernel_ms"]),
                         rows_only=dict(walk_segments_s=rows_only_s, count_kernel_ms=rows_only_ms[0],
                                        gather_kernel_ms=rows_only_ms[1]))
    out = dict(config="c3 shape with markers (tests/tile_streams.py), p_marker 0.05", docs=n, distinct_streams=args.distinct,
               ops_per_doc=args.ops, runs=args.runs, window=args.window, handle="default (paged)",
               sampled_docs_paged=f"{paged} of {len(raws)}", sampled_mean_pages=pages, sampled_mean_rows=n_rows, **res,
               bytes_model_note="a model, not a measurement: per query 204 B (header, counts, end, offsets); 32 B per row "
                                "read, in both passes (whole documents: every row; windows: two pages with the page "
                                "skip plus 14 B per directory entry of one 64-page chunk, half the document from row "
                                "0); the results written (48 B per row, the text, the records) and their sources "
                                "read; most of it is served by L2 / MALL, so the fraction is of the quoted 8 TB/s HBM "
                                "rate, not measured HBM traffic",
               not_measured="the _device form, the Node facade, other window sizes and text lengths, flat (lds / hbm "
                            "tier) documents, live handles; the host loop's time is dominated by its per-document "
                            "fetches and Python row building, which a C caller would pay differently",
               results_equal=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
