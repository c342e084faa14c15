"""The Node facade's bulk delta-log drain (native getDeltaLogs / deltaLogResetDocs, the one
drain per flush of GpuMergeTreeBatch, getDeltaRanges) against the per-document getDeltaLog, the
reference's callbacks and the Python restatement of the rows (tests/delta_util.py)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import delta_util as du
import golden_util as gu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tests", "js", "bulk_deltas_tool.js")
FIXTURE = os.path.join(gu.GOLDEN, "ref_small.json.gz")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")]
ROW = np.dtype([("query", "<i4"), ("record", "<i4"), ("seq", "<i4"), ("kind", "<i4"), ("position", "<i4"),
                ("length", "<i4"), ("word", "<i4"), ("uid", "<u4")])
FIRST = 30   # messages of the first of the two flushes


def _node(*args):
    from fluidframework_amd import build
    build.build()
    build.build_snapdec()
    build.build_node_addon()
    out = subprocess.run(["node", TOOL, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout)


def _rows(flat):
    return np.asarray(flat, dtype=np.int32).view(ROW).reshape(-1)


def test_js_get_delta_logs_equal_get_delta_log_and_python_rows():
    fx = gu.load("ref_small")
    interner = gu.Interner()   # real interning in encode order, as the JS encoder does
    gu.encode_docs(fx, interner)
    got = _node("slices", FIXTURE)
    assert got["equal"] == [True] * len(fx["docs"]) and got["flags"] == [0] * len(fx["docs"])
    off, words = np.asarray(got["off"], dtype=np.int64), np.asarray(got["words"], dtype=np.int32)
    for i, doc in enumerate(fx["docs"]):
        assert words[off[i]:off[i + 1]].tolist() == gu.expected(doc, interner)["deltas"], i
    want_off, want, bad = du.expected_rows(off, words, False, ROW)
    assert not any(bad) and got["rowOff"] == want_off.tolist() and np.array_equal(_rows(got["rows"]), want)
    assert got["subEqual"] == [True] * 4 and got["subFlags"] == [0] * 4 and got["noRows"]
    lens = np.diff(off).tolist()
    assert got["afterReset"] == [0 if i in (1, 3) else n for i, n in enumerate(lens)]


def _ref_calls(doc):
    return [[seq, kind, [list(x) for x in segs]] for seq, kind, n, segs in doc["out"]["deltas"]]


@pytest.mark.parametrize("ranges", [0, 1])
def test_js_batch_drains_views_in_one_call_across_flushes(ranges):
    """Views on 3 of 8 documents, two flushes: each view's callbacks equal the reference's raw
    callback stream, as before; with deltaRanges, every flush's rows equal the restatement's walk
    of that flush's records of every document."""
    fx = gu.load("ref_small")
    got = _node("views", FIXTURE, str(ranges), str(FIRST))
    assert got["error"] is None, got["error"]
    assert sorted(got["calls"]) == ["1", "4", "6"]
    for i in (1, 4, 6):
        assert got["calls"][str(i)] == _ref_calls(fx["docs"][i]), i
    if not ranges:
        assert got["ranges"] == [None, None]
        return
    interner = gu.Interner()
    for f, r in enumerate(got["ranges"]):
        per = []
        for doc in fx["docs"][:8]:
            cut = doc["msgs"][FIRST - 1][1]   # the first flush's last sequence number
            recs = [d for d in doc["out"]["deltas"] if (d[0] <= cut) == (f == 0)]
            per.append(gu.expected(dict(doc, out=dict(doc["out"], deltas=recs)), interner)["deltas"])
        off = np.concatenate([[0], np.cumsum([len(p) for p in per])])
        want_off, want, bad = du.expected_rows(off, [w for p in per for w in p], False, ROW)
        assert not any(bad) and r["rowOff"] == want_off.tolist() and r["flags"] == [0] * 8
        assert np.array_equal(_rows(r["rows"]), want), f
        assert len(want) > 100
