"""Delta-log drain probe (GPU box): C3 streams on the default paged handle with a delta log
(the setting of tools/readout_probe.py) times
  (a) the loop of get_delta_log(doc) calls over every document,
  (b) one get_delta_logs call for the same documents,
  (c) one get_delta_logs call with the rows (one per delta segment),
  (d) get_delta_logs_device, with and without rows (results left on the device),
reads the kernel times of (b) and (c) from mt_last_dlog_ms (HIP events) and asserts that the
words of (a) and (b) are equal and the rows of (c) are the words' (every row's header read back
from the words at its offset).  One warm-up, the median of --runs runs.  Writes
profiles/readout/bulk_deltas.json.
    python tools/delta_probe.py [--docs 4096] [--ops 2000] [--runs 5] [--log-capacity 32768] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from readout_probe import HBM_BYTES_PER_S, median_s   # noqa: E402


def handle(docs, ops, log_capacity):
    """readout_probe.handle with a delta log on the replaying handle."""
    import bench
    from fluidframework_amd import MergeTreeBatch
    cfg = dict(json.load(open(os.path.join(REPO, "bench", "configs.json")))["c3"], ops=ops)
    gen = MergeTreeBatch(docs, **bench.capacities(cfg))
    host = gen.generate(cfg).download()
    seed_off, seed = gen.generated_seeds(cfg)
    gen.close()
    mt = MergeTreeBatch(docs, delta_log_capacity=log_capacity)
    mt.load_initial_text(seed_off, seed)
    mt.apply_arrays(host)
    assert (mt.status() == 0).all(), "document failure"
    return mt


def kernel_ms(mt, call, runs):
    call()
    c, g = [], []
    for _ in range(runs):
        call()
        ms = mt.last_dlog_ms()
        c.append(ms[0])
        g.append(ms[1])
    return statistics.median(c), statistics.median(g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--ops", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--log-capacity", type=int, default=1 << 15)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "readout", "bulk_deltas.json"))
    args = ap.parse_args()
    assert args.runs >= 5
    import torch   # noqa: F401  (before the library loads: the device form shares its HIP runtime)
    mt = handle(args.docs, args.ops, args.log_capacity)
    n = args.docs
    res = {}

    def loop():
        res["a"] = [mt.get_delta_log(d) for d in range(n)]

    def bulk():
        res["b"] = mt.get_delta_logs()

    def bulk_rows():
        res["c"] = mt.get_delta_logs(ranges=True)

    bulk_s = median_s(bulk, args.runs)
    rows_s = median_s(bulk_rows, args.runs)
    dev_s = median_s(lambda: mt.get_delta_logs_device(), args.runs)
    dev_rows_s = median_s(lambda: mt.get_delta_logs_device(ranges=True), args.runs)
    loop_s = median_s(loop, args.runs)
    bulk_ms = kernel_ms(mt, bulk, args.runs)
    rows_ms = kernel_ms(mt, bulk_rows, args.runs)

    off, words, flags = res["b"]
    assert not flags.any(), "a document overflowed its log: raise --log-capacity"
    assert len(off) == n + 1 and all(words[off[d]:off[d + 1]].tolist() == res["a"][d] for d in range(n)), \
        "the bulk drain differs from the get_delta_log loop"
    off2, words2, row_off, rows, flags2 = res["c"]
    assert np.array_equal(off, off2) and np.array_equal(words, words2) and not flags2.any()
    at = off[rows["query"]] + rows["word"]
    plain = rows["kind"] >= 0
    assert np.array_equal(words[at[plain]], rows["position"][plain]) and np.array_equal(words[at[plain] + 1],
                                                                                        rows["length"][plain])
    n_records = int(np.sum([r + 1 for r in rows["record"][row_off[1:][np.diff(row_off) > 0] - 1]]))

    n_words, n_rows = int(off[n]), int(row_off[n])
    copy_bytes = 2 * 4 * n_words + n * (128 + 8 + 8)                  # words read and written, header, offsets
    walk_bytes = 4 * n_words                                          # every word's cache line is touched once
    rows_bytes = copy_bytes + 2 * walk_bytes + 32 * n_rows            # counting walk, fill walk, the rows
    out = dict(config="c3", docs=n, ops_per_doc=args.ops, runs=args.runs, handle="default (paged), delta log",
               delta_log_capacity=args.log_capacity, words=n_words, rows=n_rows, records=n_records,
               mean_words_per_doc=n_words / n,
               loop_get_delta_log_s=loop_s, loop_per_doc_ms=loop_s / n * 1e3,
               bulk_get_delta_logs_s=bulk_s, bulk_speedup=loop_s / bulk_s,
               bulk_with_rows_s=rows_s, bulk_with_rows_speedup=loop_s / rows_s,
               device_form_s=dev_s, device_form_with_rows_s=dev_rows_s,
               kernels_ms=dict(count=bulk_ms[0], gather=bulk_ms[1]),
               kernels_with_rows_ms=dict(count_and_walk=rows_ms[0], gather_and_fill=rows_ms[1]),
               copy_bytes_model=copy_bytes, copy_bytes_per_s=copy_bytes / (bulk_ms[1] * 1e-3),
               copy_fraction_of_hbm_8TBps=copy_bytes / (bulk_ms[1] * 1e-3) / HBM_BYTES_PER_S,
               rows_bytes_model=rows_bytes,
               walk_ns_per_record=(rows_ms[0] - bulk_ms[0]) * 1e6 / max(n_records / n, 1.0),
               bytes_model_note="copy: 8 B per word (read + write) + 144 B per query; rows: + 4 B per word for each "
                                "of the two walks + 32 B per row.  The walk is latency-bound (one dependent load per "
                                "record header), so walk_ns_per_record -- the counting pass's extra time over the "
                                "records of one document, every document walked concurrently -- is the figure that "
                                "describes it, not a bandwidth",
               results_equal=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
