"""Remote-view segment walk probe (GPU box): the setting of tools/walk_probe.py -- C3-shaped
streams with markers (tests/tile_streams.py: 2000 messages, four writers in turn, every op at
refSeq = seq - 1; --distinct streams repeated to --docs documents) on the default paged handle.
Document d is asked in the view of writer 1 + d % 4, for whole documents and for --per-doc
windows of about --window positions:
  (a) one walk_segments(ref_seq=, client=) call with the view at the writer's latest refSeq and at
      currentSeq: wall time and the two kernels' times (HIP events, mt_last_walk_view),
  (b) what a caller has without the call: per document get_segments + get_all_segment_props +
      get_text and the view rule on the host (tests/view_walk_util.py's vl), timed on a sample of
      --host-docs documents; rows and positions of both sides are asserted equal there (the text
      of a row the observer no longer sees is not in get_text at all: the loop cannot produce it),
  (c) the table-based page seek against MT_LOCATE_ROW_WALK=1 (every remote walk from row 0),
      results asserted equal,
  (d) the remote walk against the observer walk (client 0) on the same ranges,
  (e) a stale batch -- every view one below the writer's latest refSeq -- whose N != L queries are
      answered on the host: their count and the call's wall time, stated apart.
One warm-up, the median of --runs runs.  Writes profiles/readout/bulk_view_walk.json.
    python tools/view_walk_probe.py [--docs 4096] [--ops 2000] [--runs 5] [--per-doc 16] [--out FILE]"""
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
from readout_probe import median_s   # noqa: E402
from tile_probe import handle         # noqa: E402

NONE = -(1 << 31)


def host_loop(mt, docs, start, end, ref, cli):
    """The visits without the call: each document fetched once (segments, property sets, text),
    its ranges answered on the host by the view rule.  Per query (rows, positions)."""
    tables = {}
    for d in sorted(set(docs.tolist())):
        seg, _ = mt.get_segments(d)
        mt.get_all_segment_props(d)
        mt.get_text(d)
        assert not seg[:, 5].any(), "the probe's streams have no overlapping removes"
        tables[d] = seg
    out = []
    for d, s, e, r, c in zip(docs.tolist(), start.tolist(), end.tolist(), ref.tolist(), cli.tolist()):
        seg = tables[d]
        ins = (seg[:, 2] == c) | (seg[:, 1] <= r)
        gone = (seg[:, 3] != NONE) & ((seg[:, 4] == c) | (seg[:, 3] <= r))
        vl = np.where(ins & ~gone, seg[:, 0], 0).astype(np.int64)
        assert not (gone & ~ins & (seg[:, 0] > 0)).any(), "N != L in a view meant to be current"
        pos = np.cumsum(vl) - vl
        if e < 0:
            e = int(vl.sum())
        vis = np.flatnonzero((vl > 0) & (pos < e) & (pos + vl > s))
        out.append((vis, pos[vis]))
    return out


def kernel_ms(call, mt, runs):
    call()
    ms = []
    for _ in range(runs):
        call()
        ms.append(mt.last_walk_view()[3:])
    return [statistics.median(m[i] for m in ms) for i in (0, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--ops", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--per-doc", type=int, default=16)
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--host-docs", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "readout", "bulk_view_walk.json"))
    args = ap.parse_args()
    assert args.runs >= 5 and args.ops % 4 == 0
    mt, _ = handle(args.docs, args.ops, args.distinct)
    n = args.docs
    rng = np.random.default_rng(4)
    cur = args.ops                                   # message i (from 0) has seq i + 1, writer 1 + i % 4, refSeq i
    writer = (1 + np.arange(n) % 4).astype(np.int32)
    latest = (args.ops - 4 + (writer - 1)).astype(np.int32)      # the refSeq of the writer's last message
    step = max(n // 64, 1)
    raws = [mt.debug_raw(d) for d in range(0, n, step)]
    assert all(int(h[3]) == cur for _, h in raws)
    paged = sum(int(h[24]) != 0 for _, h in raws)
    res = {}
    for kind, ref_doc in (("latest_ref_seq", latest), ("current_seq", np.full(n, cur, dtype=np.int32))):
        lengths = mt.get_view_lengths_bulk(np.arange(n), ref_doc, writer)
        for name, per_doc in (("whole_documents", 1), ("windows", args.per_doc)):
            docs = np.repeat(np.arange(n, dtype=np.uint32), per_doc)
            ref, cli = ref_doc[docs], writer[docs]
            if per_doc == 1:
                start = np.zeros(n, dtype=np.int32)
                end = np.full(n, -1, dtype=np.int32)
            else:
                start = (rng.random(len(docs)) * np.maximum(lengths[docs] - args.window, 1)).astype(np.int32)
                end = np.minimum(start + args.window, lengths[docs]).astype(np.int32)
            got = {}

            def remote():
                got["r"] = mt.walk_segments(docs, start, end, ref_seq=ref, client=cli)

            def observer():
                got["o"] = mt.walk_segments(docs, start, end)

            ab = {}
            for walk in ("0", "1"):
                os.environ["MT_LOCATE_ROW_WALK"] = walk
                remote()
                last = mt.last_walk_view()
                ab[walk] = dict(res=got["r"], s=median_s(remote, args.runs), ms=kernel_ms(remote, mt, args.runs),
                                host=last[1], skips=last[2])
            os.environ["MT_LOCATE_ROW_WALK"] = "0"
            assert all(np.array_equal(a, b) for a, b in zip(ab["0"]["res"], ab["1"]["res"])), "page skip differs from the row walk"
            assert ab["0"]["host"] == ab["1"]["host"] == 0 and ab["1"]["skips"] == 0
            obs_s = median_s(observer, args.runs)
            observer()
            obs_ms = mt.last_walk()
            # the host loop, on a sample of the documents
            hd = np.flatnonzero(docs < args.host_docs)
            sub = (docs[hd], start[hd], end[hd], ref[hd], cli[hd])
            loop_s = median_s(lambda: got.__setitem__("l", host_loop(mt, *sub)), args.runs)
            row_off, rows = ab["0"]["res"][0], ab["0"]["res"][1]
            for q, (vis, pos) in zip(hd.tolist(), got["l"]):
                rs = rows[int(row_off[q]):int(row_off[q + 1])]
                assert np.array_equal(rs["row"], vis) and np.array_equal(rs["position"], pos), f"query {q}"
            sub_call_s = median_s(lambda: mt.walk_segments(*sub[:3], ref_seq=sub[3], client=sub[4]), args.runs)
            res[f"{kind}/{name}"] = dict(
                queries=len(docs), rows=int(len(rows)), page_skips=ab["0"]["skips"],
                page_skip=dict(walk_segments_s=ab["0"]["s"], count_kernel_ms=ab["0"]["ms"][0], gather_kernel_ms=ab["0"]["ms"][1]),
                row_walk=dict(walk_segments_s=ab["1"]["s"], count_kernel_ms=ab["1"]["ms"][0], gather_kernel_ms=ab["1"]["ms"][1]),
                page_skip_kernel_speedup=sum(ab["1"]["ms"]) / sum(ab["0"]["ms"]),
                observer_walk=dict(walk_segments_s=obs_s, count_kernel_ms=obs_ms[0], gather_kernel_ms=obs_ms[1],
                                   rows=int(len(got["o"][1]))),
                remote_over_observer_kernel_time=sum(ab["0"]["ms"]) / sum(obs_ms),
                host_loop_sample=dict(documents=args.host_docs, queries=len(hd), host_loop_s=loop_s,
                                      walk_segments_s=sub_call_s, speedup=loop_s / sub_call_s))
    # (e) a stale batch: one below the writer's latest refSeq, whole documents
    docs = np.arange(n, dtype=np.uint32)
    stale = {}

    def stale_call():
        stale["r"] = mt.walk_segments(docs, 0, None, ref_seq=latest - 1, client=writer)

    stale_s = median_s(stale_call, args.runs)
    last = mt.last_walk_view()
    res["stale_batch_whole_documents"] = dict(queries=n, host_answered=last[1], page_skips=last[2], walk_segments_s=stale_s,
                                              rows=int(len(stale["r"][1])),
                                              host_rows=int((stale["r"][1]["flags"] == 1).sum()))
    out = dict(config="c3 shape with markers (tests/tile_streams.py), p_marker 0.05", docs=n, distinct_streams=args.distinct,
               ops_per_doc=args.ops, runs=args.runs, window=args.window, handle="default (paged)",
               sampled_docs_paged=f"{paged} of {len(raws)}",
               sampled_mean_pages=float(np.mean([int(h[25]) for _, h in raws])),
               sampled_mean_rows=float(np.mean([len(r) for r, _ in raws])), **res,
               not_measured="the _device form, the Node facade, get_texts_view, other window sizes, flat (lds / hbm tier) "
                            "documents, live handles, streams with concurrent writers (overlap and overflow sets); the "
                            "host loop is timed on a sample of the documents and is dominated by its per-document fetches "
                            "and Python row building, which a C caller would pay differently",
               results_equal=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
