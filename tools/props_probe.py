"""Property read-out probe (GPU box): on the handle of tools/readout_probe.py (C3 streams on the
default paged handle) times
  (a) the per-document read-out, a get_prop_runs(doc) loop over every document,
  (b) one get_prop_runs_raw() call and one get_prop_runs_bulk() call,
  (c) one point lookup per document done through the host path: get_prop_runs(doc) and a search
      of its rows (what get_properties_at_position did before it moved onto the bulk call),
  (d) one get_properties_at_positions call for the same (doc, position) pairs,
  (e) k_props_count and k_props_gather alone by HIP events (mt_last_props_ms), next to the text
      kernels of the same handle (mt_last_text_ms),
and asserts that (a) equals (b) and (c) equals (d).  One warm-up, the median of --runs runs.
Writes profiles/readout/bulk_props.json.
    python tools/props_probe.py [--docs 4096] [--ops 2000] [--runs 5] [--out FILE]"""
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


def kernel_ms(call, last, runs):
    call()
    c, g = [], []
    for _ in range(runs):
        call()
        ms = last()
        c.append(ms[0])
        g.append(ms[1])
    return statistics.median(c), statistics.median(g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--ops", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "readout", "bulk_props.json"))
    args = ap.parse_args()
    assert args.runs >= 5
    mt = handle(args.docs, args.ops)
    n = args.docs
    count_ms, gather_ms = kernel_ms(mt.get_prop_runs_raw, mt.last_props_ms, args.runs)
    text_count_ms, text_gather_ms = kernel_ms(mt.get_texts_raw, mt.last_text_ms, args.runs)
    rng = np.random.default_rng(1)
    lengths = np.diff(mt.get_texts_raw(placeholder=" ")[0])
    docs = np.arange(n, dtype=np.uint32)
    pos = (rng.random(n) * lengths).astype(np.int64)   # (an empty document: position 0, outside)
    res = {}

    def loop():
        res["a"] = [mt.get_prop_runs(d) for d in range(n)]

    def bulk():
        res["b"] = mt.get_prop_runs_bulk()

    def points_host():
        out = []
        for d, p in zip(docs.tolist(), pos.tolist()):
            out.append(next((pr for s, l, pr in mt.get_prop_runs(d) if s <= p < s + l), None))
        res["c"] = out

    def points_bulk():
        res["d"] = mt.get_properties_at_positions(docs, pos)

    bulk_s = median_s(bulk, args.runs)
    raw_s = median_s(mt.get_prop_runs_raw, args.runs)
    points_bulk_s = median_s(points_bulk, args.runs)
    loop_s = median_s(loop, args.runs)
    points_host_s = median_s(points_host, args.runs)
    assert res["a"] == res["b"], "get_prop_runs_bulk() differs from the get_prop_runs(doc) loop"
    assert res["c"] == res["d"], "get_properties_at_positions differs from the host search"
    run_off, word_off, runs, recs = mt.get_prop_runs_raw()
    written = int(runs.nbytes + recs.nbytes)
    step = max(n // 64, 1)
    paged = sum(mt.is_paged(d) for d in range(0, n, step))
    out = dict(config="c3", docs=n, ops_per_doc=args.ops, runs=args.runs, handle="default (paged)",
               sampled_docs_paged=f"{paged} of {len(range(0, n, step))}",
               runs_returned=int(len(runs)), record_words_returned=int(len(recs)), bytes_written=written,
               per_document_loop_s=loop_s, bulk_get_prop_runs_s=bulk_s, bulk_get_prop_runs_raw_s=raw_s,
               bulk_speedup=loop_s / bulk_s, bulk_raw_speedup=loop_s / raw_s,
               point_lookups=n, points_host_path_s=points_host_s, points_bulk_s=points_bulk_s,
               points_speedup=points_host_s / points_bulk_s,
               count_kernel_ms=count_ms, gather_kernel_ms=gather_ms,
               gather_bytes_written_per_s=written / (gather_ms * 1e-3),
               gather_fraction_of_hbm_8TBps=written / (gather_ms * 1e-3) / HBM_BYTES_PER_S,
               text_count_kernel_ms=text_count_ms, text_gather_kernel_ms=text_gather_ms,
               gather_form="one lane per run head copies its record (<= 17 words)",
               results_equal=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
