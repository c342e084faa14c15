"""bench.py end to end on the GPU at a small size (48 C3 documents x 300 messages): a plain
run times exactly --steps steps and reports the timed figures only, --full adds the roofline
and the CPU baseline, and --dump-outputs writes the last step's per-document outputs -- equal
to the CPU oracle's, and the same from run to run."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE = ["--docs", "48", "--ops", "300"]
NAMES = ("status", "length", "n_segments", "text_hash", "props_hash", "delta_hash",
         "text_sample", "text_sample_docs", "text_sample_off")


def _run(monkeypatch, capsys, argv):
    import bench
    import fluidframework_amd as ff
    applied = []
    apply_async = ff.DeviceBatch.apply_async
    monkeypatch.setattr(ff.DeviceBatch, "apply_async", lambda self: (applied.append(1), apply_async(self))[1])
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1"] + SIZE + argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), len(applied)


def test_gpu_bench_plain_then_full_dump_the_same_outputs(monkeypatch, capsys, tmp_path, oracle_lib):
    import bench
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line, applied = _run(monkeypatch, capsys, ["--steps", "3", "--warmup", "2", "--dump-outputs", a])
    assert applied == 5 and (line["steps"], line["warmup"]) == (3, 2)
    assert line["unit"] == "ops/s" and line["higher_is_better"] is True and line["dtype"] == "int32"
    assert line["metric"].startswith("sequenced merge-tree ops applied/sec")
    n_ops = line["config"]["ops_per_step"]
    assert n_ops == 48 * 300 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(n_ops * 1000.0 / line["ms_per_step"], rel=1e-3)
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["ingest"] is None
    assert line["parity"] == {"replay_equals_generation": True, "oracle_sample": None, "shards": None}

    got = {n: np.load(os.path.join(a, n + ".npy")) for n in NAMES}
    assert all(v.dtype == np.float64 for v in got.values())
    cfg = dict(json.load(open(os.path.join(bench.REPO, "bench", "configs.json")))["c3"], ops=300)
    ref = bench.oracle_checksums(cfg, list(range(48)), 4)
    assert not got["status"].any()
    for k in ("length", "n_segments"):
        assert np.array_equal(got[k], ref[k])
    for k in ("text_hash", "props_hash", "delta_hash"):
        assert np.array_equal(got[k][:, 0], ref[k] >> np.uint64(32))
        assert np.array_equal(got[k][:, 1], ref[k] & np.uint64(0xFFFFFFFF))
    off = got["text_sample_off"].astype(int)
    assert np.array_equal(np.diff(off), ref["length"][got["text_sample_docs"].astype(int)])

    full, applied = _run(monkeypatch, capsys, ["--steps", "1", "--warmup", "0", "--full", "--no-ingest",
                                               "--dump-outputs", b])
    assert applied == 1 and full["ms_per_step"] > 0
    assert full["roofline"]["kernel_ms"] > 0 and full["roofline"]["alg_bytes_per_launch"] > 0
    assert full["cpu_baseline"]["value"] > 0
    assert full["parity"]["replay_equals_generation"] is True
    assert full["parity"]["oracle_sample"] == {"docs_checked": 48, "mismatches": 0}
    for n in NAMES:
        assert np.array_equal(got[n], np.load(os.path.join(b, n + ".npy")))
