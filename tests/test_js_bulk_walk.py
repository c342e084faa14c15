"""The Node facade's segment walk (native walkSegments, GpuMergeTreeBatch.walkSegments,
GpuClient.walkSegments / getTextAndMarkers / getRangeExtentsOfPosition) against the reference's
own answers (tests/golden/ref_walk.json.gz, final checkpoint), replayed in one flush and in
flushes of 37 messages: the handler's arguments, every visited segment's fields, text and
properties in key order, the early stop, one object per segment, and the splitRange throw."""
import json
import os
import shutil
import subprocess

import pytest

import golden_util as gu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tests", "js", "bulk_walk_tool.js")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")]


def _entries(props):
    return None if props is None else [[k, v] for k, v in props.items()]


@pytest.mark.parametrize("flush_every", [0, 37])
def test_js_walk_segments_and_text_and_markers_equal_the_reference(flush_every):
    from fluidframework_amd import build
    build.build()
    build.build_snapdec()
    build.build_node_addon()
    out = subprocess.run(["node", TOOL, os.path.join(gu.GOLDEN, "ref_walk.json.gz"), str(flush_every)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)
    fx = gu.load("ref_walk")
    visited = stops = same = texts = extents = 0
    for d, g in zip(fx["docs"], got["docs"]):
        cp = d["checkpoints"][-1]
        segs = cp["segs"]
        assert len(g["walks"]) == len(cp["walks"])
        for (start, end, visits), mine in zip(cp["walks"], g["walks"]):
            want = [[pos, s, e, segs[row][0], segs[row][5], segs[row][6], segs[row][4], segs[row][2], _entries(segs[row][3])]
                    for row, pos, s, e in visits]
            assert mine == want, (d["doc"], start, end, mine[:2], want[:2])
            visited += len(want)
        assert g["args"]["checked"] == g["args"]["ok"] == sum(len(v) for _, _, v in cp["walks"])
        for stop_at, n, total in g["stops"]:
            assert n == min(stop_at, total), (d["doc"], stop_at, n, total)
            stops += n < total
        assert g["same"]["checked"] == g["same"]["ok"], (d["doc"], g["same"])
        same += g["same"]["ok"]
        for (ptext, markers), (mtext, mmarkers) in zip(cp["tam"], g["tam"]):
            assert mtext == ptext, d["doc"]
            assert mmarkers == [[segs[row][2], _entries(segs[row][3])] for row in markers], d["doc"]
            texts += len(ptext)
        assert g["extents"] == cp["extents"], d["doc"]
        extents += len(cp["extents"])
    assert visited > 5000 and stops > 20 and same > 100 and texts > 100 and extents > 50, (visited, stops, same, texts, extents)
    assert got["batch"] is True
    assert got["split"] is not None and "splitRange" in got["split"]
