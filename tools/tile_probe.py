"""Marker query probe (GPU box): C3-shaped streams with markers (tests/tile_streams.py: p_marker
0.05, 2000 messages; the device generator makes no markers, so --distinct streams are built on the
host and repeated to --docs documents) replayed on the default handle, then, for the label "pg",
  (a) one find_tiles call for one cursor per document and for --per-doc cursors per document
      (half of them preceding, half following), wall time and kernel time (HIP events,
      mt_last_tiles),
  (b) the same answers the way a caller gets them without the call: per document get_segments +
      get_all_segment_props and a host scan (the rule of tests/tile_util.py),
  (c) rows examined per query with H's page found by the directory and the outward page walk, and
      with MT_LOCATE_ROW_WALK=1 (from row 0),
and asserts both sides of (a)/(b) and of (c) equal.  One warm-up, the median of --runs runs.
Writes profiles/readout/bulk_tiles.json.
    python tools/tile_probe.py [--docs 4096] [--ops 2000] [--runs 5] [--per-doc 16] [--out FILE]"""
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
import tile_streams   # noqa: E402
import tile_util      # noqa: E402

LABEL = "pg"
NONE = -(1 << 31)
ROW_BYTES = 16 + 16           # segA and segB of one row
RECORD_BYTES = 4 * 17         # a marker's property record
QUERY_BYTES = 128 + 48 + 4    # the document header, the record, the rows-examined word
PAGE_DIR_BYTES = 2 + 12       # a directory entry and its PageMeta


def handle(n_docs, ops, distinct):
    from fluidframework_amd import MergeTreeBatch
    from fluidframework_amd.wire import Batch, Interner, compact_msgs_to_dicts
    interner = Interner()
    b = Batch(interner)
    for i in range(distinct):
        log = tile_streams.build(dict(name=f"probe{i}", seed=9900 + i, msgs=ops, lag=64, p_marker=0.05, p_insert=0.5,
                                      p_remove=0.3, text_max=8, seed_len=64, end=None, checkpoints=1))
        b.add_doc(log["seed_text"], compact_msgs_to_dicts(log["msgs"]))
    a = b.arrays()
    # the distinct streams repeated: op records and seeds tiled, the arenas shared
    reps = n_docs // distinct
    assert reps * distinct == n_docs
    per = np.diff(a["doc_off"])
    seeds = np.diff(a["seed_off"])
    a = dict(a, ops=np.tile(a["ops"], reps),
             doc_off=np.concatenate([[0], np.cumsum(np.tile(per, reps))]).astype(np.int64),
             seed=np.tile(a["seed"], reps),
             seed_off=np.concatenate([[0], np.cumsum(np.tile(seeds, reps))]).astype(np.int64))
    mt = MergeTreeBatch(n_docs)
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    assert (mt.status() == 0).all(), "document failure"
    return mt, interner


def host_rows(mt, d, interner):
    seg, _ = mt.get_segments(d)
    props = mt.get_all_segment_props(d)
    return [(int(s[0]), bool(s[3] != NONE), int(s[6]) if s[6] >= 0 else None,
             None if p is None else {interner.key_name(k): interner.val_value(v) for k, v in p})
            for s, p in zip(seg, props)]


def host_loop(mt, interner, docs, pos, prec):
    """The answers without the call: each document fetched once, its cursors answered on the host
    (the rule of tests/tile_util.find_tile, vectorised over the document's cursors)."""
    out = np.full((len(docs), 2), -1, dtype=np.int64)
    order = np.argsort(docs, kind="stable")
    bounds = np.flatnonzero(np.diff(docs[order], prepend=-1, append=-1))
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        q = order[lo:hi]
        rows = host_rows(mt, int(docs[q[0]]), interner)
        obs = np.asarray([0 if r[1] else r[0] for r in rows], dtype=np.int64)
        ends = np.cumsum(obs)
        length = int(ends[-1]) if len(rows) else 0
        ok = np.flatnonzero([tile_util.qualifies(r, LABEL) and o > 0 for r, o in zip(rows, obs)])
        hit = np.searchsorted(ends, pos[q], side="right")          # H (len(rows): none)
        before = np.searchsorted(ok, np.minimum(hit, len(rows) - 1), side="right") - 1
        after = np.searchsorted(ok, hit, side="left")
        for k, i in enumerate(q):
            got = -1
            if prec[i]:
                got = ok[before[k]] if before[k] >= 0 else -1
            elif pos[i] < length:
                got = ok[after[k]] if after[k] < len(ok) else -1
            elif pos[i] == length and rows and tile_util.qualifies(rows[-1], LABEL):
                got = len(rows) - 1
            if got >= 0:
                out[i] = (got, ends[got] - obs[got])
    return out


def kernel_ms(call, last, runs):
    call()
    ms = []
    for _ in range(runs):
        call()
        ms.append(last()[2])
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--ops", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--per-doc", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "readout", "bulk_tiles.json"))
    args = ap.parse_args()
    assert args.runs >= 5
    mt, interner = handle(args.docs, args.ops, args.distinct)
    n = args.docs
    rng = np.random.default_rng(2)
    lengths = mt.get_view_lengths_bulk(np.arange(n))
    step = max(n // 64, 1)
    raws = [mt.debug_raw(d) for d in range(0, n, step)]
    pages = float(np.mean([int(h[25]) for _, h in raws]))
    rows = float(np.mean([len(r) for r, _ in raws]))
    markers = float(np.mean([(r[:, 6] >> 31).mean() for r, _ in raws]))
    paged = sum(int(h[24]) != 0 for _, h in raws)
    res = {}
    for name, per_doc in (("one_per_doc", 1), ("many", args.per_doc)):
        docs = np.repeat(np.arange(n, dtype=np.uint32), per_doc)
        pos = (rng.random(len(docs)) * lengths[docs]).astype(np.int32)
        prec = (np.arange(len(docs)) % 2 == 0)
        got = {}

        def bulk():
            got["bulk"] = mt.find_tiles(docs, pos, LABEL, prec, interner=interner)

        def loop():
            got["loop"] = host_loop(mt, interner, docs, pos, prec)

        ab = {}
        for walk in ("0", "1"):
            os.environ["MT_LOCATE_ROW_WALK"] = walk
            bulk()
            ab[walk] = dict(hits=got["bulk"].copy(), examined=mt.last_tiles()[1], bulk_s=median_s(bulk, args.runs),
                            kernel_ms=kernel_ms(bulk, mt.last_tiles, args.runs))
        os.environ["MT_LOCATE_ROW_WALK"] = "0"
        assert np.array_equal(ab["0"]["hits"], ab["1"]["hits"]), "page skip differs from the row walk"
        loop_s = median_s(loop, args.runs)
        hits = ab["0"]["hits"]
        assert np.array_equal(hits["row"], got["loop"][:, 0]), "find_tiles differs from the host scan (row)"
        f = hits["row"] >= 0
        assert np.array_equal(hits["position"][f], got["loop"][f, 1]), "find_tiles differs from the host scan (position)"
        nq = len(docs)
        one = {}
        for walk, form in (("0", "page_skip"), ("1", "row_walk")):
            ex = ab[walk]["examined"]
            model = int(nq * QUERY_BYTES + ex * (ROW_BYTES + markers * RECORD_BYTES) +
                        (nq * min(pages, 64.0) * PAGE_DIR_BYTES if walk == "0" else 0))
            one[form] = dict(find_tiles_s=ab[walk]["bulk_s"], kernel_ms=ab[walk]["kernel_ms"],
                             rows_examined_per_query=ex / nq, bytes_model=model,
                             bytes_per_s=model / (ab[walk]["kernel_ms"] * 1e-3),
                             fraction_of_hbm_8TBps=model / (ab[walk]["kernel_ms"] * 1e-3) / HBM_BYTES_PER_S)
        res[name] = dict(cursors=nq, answered=int(f.sum()), host_loop_s=loop_s, find_tiles_s=ab["0"]["bulk_s"],
                         speedup=loop_s / ab["0"]["bulk_s"], **one,
                         page_skip_kernel_speedup=ab["1"]["kernel_ms"] / ab["0"]["kernel_ms"])
    out = dict(config="c3 shape with markers (tests/tile_streams.py), p_marker 0.05, label 'pg'", docs=n,
               distinct_streams=args.distinct, ops_per_doc=args.ops, runs=args.runs, handle="default (paged)",
               sampled_docs_paged=f"{paged} of {len(raws)}", sampled_mean_pages=pages, sampled_mean_rows=rows,
               sampled_marker_fraction=markers, **res,
               bytes_model_note="a model, not a measurement: per query 180 B (header, record, counter), 32 B per row "
                                "examined plus 68 B of property record for the marker share of them, and, with the "
                                "page skip, 14 B per directory entry of one 64-page chunk; most of it is served by L2 "
                                "/ MALL, so the fraction is of the quoted 8 TB/s HBM rate, not measured HBM traffic",
               not_measured="the _device form, find_markers_by_id, other labels and marker densities, the Node facade",
               results_equal=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
