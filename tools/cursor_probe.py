"""Cursor read-out probe (GPU box): on the handle of tools/readout_probe.py (C3 streams on the
default paged handle) times, for observer-view cursors,
  (a) a loop of get_containing_segment(doc, pos) calls, one cursor per document,
  (b) one locate_segments call for the same cursors,
  (c) a loop of get_segment_by_uid(doc, uid) calls for the segments (a) found,
  (d) one locate_uids call for the same,
  (e) one locate_segments / locate_uids call for --per-doc cursors per document with the page
      skip on and off (MT_LOCATE_ROW_WALK=1: every row walked), wall time and kernel time (HIP
      events, mt_last_locate),
  (f) the same cursors in a writer's view at currentSeq (every row walked, the host path for the
      views the device does not answer) and get_view_lengths_bulk against the get_view_lengths
      loop,
and asserts that the two sides of each pair are equal.  One warm-up, the median of --runs runs.
Writes profiles/readout/bulk_segments.json.
    python tools/cursor_probe.py [--docs 4096] [--ops 2000] [--runs 5] [--per-doc 16] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from readout_probe import HBM_BYTES_PER_S, handle, median_s   # noqa: E402

ROW_BYTES = 16 + 8 + 16       # segA, the overlap mask, segB of one row
QUERY_BYTES = 128 + 512 + 64  # the document header, the overlap slots, the record and its mark
PAGE_DIR_BYTES = 2 + 12       # a directory entry and its PageMeta
SAME = ("row", "uid", "position", "offset", "length", "seq", "client", "removed_seq", "removed_client",
        "marker_ref_type")


def kernel_ms(call, last, runs):
    call()
    ms = []
    for _ in range(runs):
        call()
        ms.append(last()[2])
    return statistics.median(ms)


def as_records(singles):
    from fluidframework_amd import _native
    out = np.zeros(len(singles), dtype=_native.SEG_HIT_DTYPE)
    out["row"] = -1
    for i, r in enumerate(singles):
        if r is not None:
            for k in SAME:
                out[k][i] = r[k]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--ops", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--per-doc", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "readout", "bulk_segments.json"))
    args = ap.parse_args()
    assert args.runs >= 5
    mt = handle(args.docs, args.ops)
    n = args.docs
    rng = np.random.default_rng(1)
    lengths = mt.get_view_lengths_bulk(np.arange(n))
    assert lengths.tolist()[:64] == [mt.get_length(d) for d in range(64)]
    docs = np.arange(n, dtype=np.uint32)
    pos = (rng.random(n) * lengths).astype(np.int32)
    res = {}

    def loop_pos():
        res["a"] = as_records([mt.get_containing_segment(int(d), int(p), text_cap=1) for d, p in zip(docs, pos)])

    def bulk_pos():
        res["b"] = mt.locate_segments(docs, pos)

    bulk_pos()
    found = res["b"]["row"] >= 0
    udocs, uids = docs[found], res["b"]["uid"][found]

    def loop_uid():
        res["c"] = as_records([mt.get_segment_by_uid(int(d), int(u), text_cap=1) for d, u in zip(udocs, uids)])

    def bulk_uid():
        res["d"] = mt.locate_uids(udocs, uids)

    bulk_pos_s = median_s(bulk_pos, args.runs)
    bulk_uid_s = median_s(bulk_uid, args.runs)
    loop_pos_s = median_s(loop_pos, args.runs)
    loop_uid_s = median_s(loop_uid, args.runs)
    for x, y in (("a", "b"), ("c", "d")):
        for k in SAME:
            assert np.array_equal(res[x][k], res[y][k]), f"bulk differs from the single-query loop in {k}"

    # (e) many cursors per document: page skip on / off
    many_docs = np.repeat(docs, args.per_doc)
    many_pos = (rng.random(len(many_docs)) * lengths[many_docs]).astype(np.int32)
    ab = {}
    for walk in ("0", "1"):
        os.environ["MT_LOCATE_ROW_WALK"] = walk
        hits = mt.locate_segments(many_docs, many_pos)
        mu = hits["uid"][hits["row"] >= 0]
        md = many_docs[hits["row"] >= 0]
        ab[walk] = dict(
            hits=hits, by_uid=mt.locate_uids(md, mu),
            pos_s=median_s(lambda: mt.locate_segments(many_docs, many_pos), args.runs),
            uid_s=median_s(lambda: mt.locate_uids(md, mu), args.runs),
            pos_kernel_ms=kernel_ms(lambda: mt.locate_segments(many_docs, many_pos), mt.last_locate, args.runs),
            uid_kernel_ms=kernel_ms(lambda: mt.locate_uids(md, mu), mt.last_locate, args.runs),
            len_kernel_ms=kernel_ms(lambda: mt.get_view_lengths_bulk(docs), mt.last_locate, args.runs))
    os.environ["MT_LOCATE_ROW_WALK"] = "0"
    assert np.array_equal(ab["0"]["hits"], ab["1"]["hits"]), "page skip differs from the row walk (by position)"
    assert np.array_equal(ab["0"]["by_uid"], ab["1"]["by_uid"]), "page skip differs from the row walk (by uid)"

    # the bytes each form has to read (a model from the results: rows up to the hit for the walk; one
    # directory and one page for the skip), pages and rows from a sample of the documents
    step = max(n // 64, 1)
    sample = list(range(0, n, step))
    raws = [mt.debug_raw(d) for d in sample]
    pages = float(np.mean([int(h[25]) for _, h in raws]))
    rows = float(np.mean([len(r) for r, _ in raws]))
    paged = sum(int(h[24]) != 0 for _, h in raws)
    nq = len(many_docs)
    hit_rows = ab["0"]["hits"]["row"].astype(np.int64)
    walk_bytes = int(nq * QUERY_BYTES + (hit_rows + 1).clip(min=0).sum() * ROW_BYTES)
    skip_bytes = int(nq * (QUERY_BYTES + min(pages, 64.0) * PAGE_DIR_BYTES + rows / max(pages, 1.0) * ROW_BYTES))

    # (f) a writer's view: every row walked on the device; the views it does not answer on the host
    cur = np.asarray([int(h[3]) for _, h in raws], dtype=np.int32)
    rdocs = np.repeat(np.asarray(sample, dtype=np.uint32), args.per_doc)
    rref = np.repeat(cur, args.per_doc)
    rpos = (rng.random(len(rdocs)) * lengths[rdocs]).astype(np.int32)
    remote = mt.locate_segments(rdocs, rpos, rref, 1)
    remote_q, remote_host, _ = mt.last_locate()
    remote_kernel_ms = kernel_ms(lambda: mt.locate_segments(rdocs, rpos, rref, 1), mt.last_locate, args.runs)
    remote_s = median_s(lambda: mt.locate_segments(rdocs, rpos, rref, 1), args.runs)
    one = as_records([mt.get_containing_segment(int(d), int(p), int(r), 1, text_cap=1)
                      for d, p, r in zip(rdocs[::args.per_doc], rpos[::args.per_doc], rref[::args.per_doc])])
    for k in SAME:
        assert np.array_equal(one[k], remote[k][::args.per_doc]), f"remote view: bulk differs from the single query in {k}"
    sdocs = np.asarray(sample, dtype=np.uint32)
    ones = np.ones(len(sample), dtype=np.int32)
    lens_loop_s = median_s(lambda: [mt.get_view_lengths([d], [int(c)], [1]) for d, c in zip(sample, cur)], args.runs)
    lens_bulk_s = median_s(lambda: mt.get_view_lengths_bulk(sdocs, cur, ones), args.runs)
    assert mt.get_view_lengths_bulk(sdocs, cur, ones).tolist() == mt.get_view_lengths(sdocs, cur, ones).tolist()

    on, off = ab["0"], ab["1"]
    default = "page skip" if on["pos_kernel_ms"] <= off["pos_kernel_ms"] else "row walk"
    out = dict(config="c3", docs=n, ops_per_doc=args.ops, runs=args.runs, handle="default (paged)",
               sampled_docs_paged=f"{paged} of {len(sample)}", sampled_mean_pages=pages, sampled_mean_rows=rows,
               cursors_one_per_doc=n, loop_get_containing_segment_s=loop_pos_s, bulk_locate_segments_s=bulk_pos_s,
               by_position_speedup=loop_pos_s / bulk_pos_s,
               uid_cursors=int(len(uids)), loop_get_segment_by_uid_s=loop_uid_s, bulk_locate_uids_s=bulk_uid_s,
               by_uid_speedup=loop_uid_s / bulk_uid_s,
               cursors_many=nq, cursors_per_doc=args.per_doc,
               page_skip=dict(locate_segments_s=on["pos_s"], locate_uids_s=on["uid_s"],
                              locate_segments_kernel_ms=on["pos_kernel_ms"], locate_uids_kernel_ms=on["uid_kernel_ms"],
                              view_lengths_kernel_ms=on["len_kernel_ms"], bytes_model=skip_bytes,
                              bytes_per_s=skip_bytes / (on["pos_kernel_ms"] * 1e-3),
                              fraction_of_hbm_8TBps=skip_bytes / (on["pos_kernel_ms"] * 1e-3) / HBM_BYTES_PER_S),
               row_walk=dict(locate_segments_s=off["pos_s"], locate_uids_s=off["uid_s"],
                             locate_segments_kernel_ms=off["pos_kernel_ms"], locate_uids_kernel_ms=off["uid_kernel_ms"],
                             view_lengths_kernel_ms=off["len_kernel_ms"], bytes_model=walk_bytes,
                             bytes_per_s=walk_bytes / (off["pos_kernel_ms"] * 1e-3),
                             fraction_of_hbm_8TBps=walk_bytes / (off["pos_kernel_ms"] * 1e-3) / HBM_BYTES_PER_S),
               page_skip_kernel_speedup_by_position=off["pos_kernel_ms"] / on["pos_kernel_ms"],
               page_skip_kernel_speedup_by_uid=off["uid_kernel_ms"] / on["uid_kernel_ms"],
               faster_form=default,
               bytes_model_note="per query 704 B (header, overlap slots, record) + 40 B per row read: rows up to "
                                "the hit (row walk), or 14 B per directory entry of one 64-page chunk and one mean "
                                "page (page skip); most of it is served by L2 / MALL, so the fraction is of the "
                                "quoted HBM rate, not a measured HBM traffic",
               remote_view=dict(cursors=int(remote_q), host_path=int(remote_host), locate_segments_s=remote_s,
                                locate_segments_kernel_ms=remote_kernel_ms, views=len(sample),
                                loop_get_view_lengths_s=lens_loop_s, bulk_get_view_lengths_s=lens_bulk_s,
                                view_lengths_speedup=lens_loop_s / lens_bulk_s),
               results_equal=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
