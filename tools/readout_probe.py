"""Text read-out probe (GPU box): on a generated C3 handle (bench/configs.json c3 at a reduced
size, the default paged handle) times the per-document read-out -- a get_text(doc) loop over
every document -- against one bulk get_texts() call, and the gather kernel alone by HIP events
(mt_last_text_ms); asserts the two results equal.  One warm-up, the median of --runs runs.
MT_TEXT_PER_SEGMENT=1 (a child process: the library reads it per call) times the k_extract-style
per-segment copy in place of the lane-per-unit gather.  Writes profiles/readout/bulk_text.json.
    python tools/readout_probe.py [--docs 4096] [--ops 2000] [--runs 5]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_BYTES_PER_S = 8e12   # the MI355X figure the project quotes


def median_s(fn, runs):
    fn()   # warm-up
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def handle(docs, ops):
    import bench
    from fluidframework_amd import MergeTreeBatch
    cfg = dict(json.load(open(os.path.join(REPO, "bench", "configs.json")))["c3"], ops=ops)
    # the generator runs on a handle sized for the workload (it does not grow documents); the
    # stream is then replayed on the default (paged, unbounded) handle a catch-up job would hold
    gen = MergeTreeBatch(docs, **bench.capacities(cfg))
    host = gen.generate(cfg).download()
    seed_off, seed = gen.generated_seeds(cfg)
    gen.close()
    mt = MergeTreeBatch(docs)
    mt.load_initial_text(seed_off, seed)
    mt.apply_arrays(host)
    assert (mt.status() == 0).all(), "document failure"
    return mt


def kernel_ms(mt, runs):
    """Median device time of the counting pass and the gather over `runs` get_texts_raw calls."""
    mt.get_texts_raw()
    c, g = [], []
    for _ in range(runs):
        mt.get_texts_raw()
        ms = mt.last_text_ms()
        c.append(ms[0])
        g.append(ms[1])
    return statistics.median(c), statistics.median(g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--ops", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true", help="print the kernel times as JSON and exit")
    args = ap.parse_args()
    assert args.runs >= 5
    mt = handle(args.docs, args.ops)
    count_ms, gather_ms = kernel_ms(mt, args.runs)
    if args.kernel_only:
        print(json.dumps(dict(count_ms=count_ms, gather_ms=gather_ms)))
        return
    per_doc = [None]
    bulk = [None]

    def loop():
        per_doc[0] = [mt.get_text(d) for d in range(args.docs)]

    def one_call():
        bulk[0] = mt.get_texts()

    bulk_s = median_s(one_call, args.runs)
    raw_s = median_s(mt.get_texts_raw, args.runs)
    loop_s = median_s(loop, args.runs)
    assert per_doc[0] == bulk[0], "get_texts() differs from the get_text(doc) loop"
    off, units = mt.get_texts_raw()
    paged = sum(mt.is_paged(d) for d in range(0, args.docs, max(args.docs // 64, 1)))
    # the A/B: the per-segment copy in a child process (kernel times only)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--docs", str(args.docs), "--ops", str(args.ops),
                            "--runs", str(args.runs), "--kernel-only"], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, MT_TEXT_PER_SEGMENT="1"))
    assert child.returncode == 0, child.stderr[-2000:]
    per_seg = json.loads(child.stdout.strip().splitlines()[-1])
    written = int(len(units)) * 2
    out = dict(config="c3", docs=args.docs, ops_per_doc=args.ops, runs=args.runs, handle="default (paged)",
               sampled_docs_paged=f"{paged} of {len(range(0, args.docs, max(args.docs // 64, 1)))}",
               units_returned=int(len(units)), bytes_written=written,
               per_document_loop_s=loop_s, bulk_get_texts_s=bulk_s, bulk_get_texts_raw_s=raw_s,
               bulk_speedup=loop_s / bulk_s,
               count_kernel_ms=count_ms, gather_kernel_ms=gather_ms,
               gather_bytes_written_per_s=written / (gather_ms * 1e-3),
               gather_fraction_of_hbm_8TBps=written / (gather_ms * 1e-3) / HBM_BYTES_PER_S,
               per_segment_copy_gather_kernel_ms=per_seg["gather_ms"],
               results_equal=True)
    os.makedirs(os.path.join(REPO, "profiles", "readout"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "readout", "bulk_text.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
