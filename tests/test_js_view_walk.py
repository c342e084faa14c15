"""The Node facade's walk in a (refSeq, client) view (native walkSegmentsView,
GpuMergeTreeBatch.walkSegments with {refSeq, clientId}, GpuClient.mergeTree.mapRange /
cloneSegments, GpuClient.getTextInView) against the reference's own answers
(tests/golden/ref_view_walk.json.gz, final checkpoints of one flat and one paged document): the
leaf action's arguments, every visited segment's fields and text, the clones, the texts, the early
exit, and the "not offered" throws."""
import json
import os
import shutil
import subprocess

import pytest

import view_walk_util as vu
from test_view_walk import _fixture

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tests", "js", "view_walk_tool.js")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")]


def test_js_map_range_clone_segments_and_text_in_view_equal_the_reference(tmp_path):
    from fluidframework_amd import build
    build.build()
    build.build_snapdec()
    build.build_node_addon()
    docs = [d for d in _fixture()["docs"] if d["doc"] in ("flat10", "paged0")]
    assert len(docs) == 2
    last = [d["checkpoints"][-1] for d in docs]
    inp = tmp_path / "docs.json"
    inp.write_text(json.dumps([dict(doc=d["doc"], seed_text=d["seed_text"], msgs=d["msgs"], views=[
        dict(refSeq=v["refSeq"], client=v["client"], walks=[w[:2] for w in v["walks"]], texts=[t[:2] for t in v["texts"]])
        for v in cp["views"]]) for d, cp in zip(docs, last)]))
    out = subprocess.run(["node", TOOL, str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)
    visited = stops = texts = host = 0
    for d, cp, g in zip(docs, last, got["docs"]):
        segs = cp["segs"]
        for v, walks, clones, mine_texts in zip(cp["views"], g["walks"], g["clones"], g["texts"]):
            host += v["N"] != v["L"]
            for (start, end, visits), mine in zip(v["walks"], walks):
                want = [[pos, s, e, segs[row][vu.LEN], segs[row][vu.SEQ], segs[row][vu.CLI], segs[row][vu.TEXT],
                         segs[row][vu.RTYPE]] for row, pos, s, e in visits]
                assert mine == want, (d["doc"], v["refSeq"], v["client"], start, end, mine[:2], want[:2])
                visited += len(want)
            first = v["walks"][0][2]
            assert clones == [[[segs[row][vu.LEN], segs[row][vu.TEXT]] for row, _, _, _ in first], True]
            assert mine_texts == [t[2] for t in v["texts"]], (d["doc"], v["refSeq"], v["client"])
            texts += len(mine_texts)
        assert g["args"]["checked"] == g["args"]["ok"] == sum(len(w[2]) for v in cp["views"] for w in v["walks"])
        for stop_at, n, total in g["stops"]:
            assert n == min(stop_at, total)
            stops += n < total
        throws = dict(g["throws"])
        for k in ("pre", "post", "shift", "contains"):
            assert throws[k] is not None and "not offered" in throws[k], throws
        assert "splitRange" in throws["splitRange"] and throws["star"] is not None
    assert visited > 3000 and stops > 10 and texts > 100 and host > 0, (visited, stops, texts, host)
