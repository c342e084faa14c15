"""The Node facade's marker queries (native findTiles / findMarkersById,
GpuMergeTreeBatch.findTiles / getMarkersFromIds, GpuClient.findTile / getMarkerFromId) against the
reference's own answers (tests/golden/ref_tiles.json.gz, final checkpoint), replayed in one flush
and in flushes of 37 messages; the returned tile is the object the delta events carried."""
import json
import os
import shutil
import subprocess

import pytest

import golden_util as gu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tests", "js", "bulk_tiles_tool.js")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")]


@pytest.mark.parametrize("flush_every", [0, 37])
def test_js_find_tile_and_get_marker_from_id_equal_the_reference(flush_every):
    from fluidframework_amd import build
    build.build()
    build.build_snapdec()
    build.build_node_addon()
    out = subprocess.run(["node", TOOL, os.path.join(gu.GOLDEN, "ref_tiles.json.gz"), str(flush_every)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)
    fx = gu.load("ref_tiles")
    found = same = by_id = gone = 0
    for d, g in zip(fx["docs"], got["docs"]):
        cp = d["checkpoints"][-1]
        assert g["tiles"] == [None if row < 0 else [row, tpos] for _, _, _, row, tpos in cp["tiles"]], d["doc"]
        assert g["ids"] == [None if row < 0 else row for _, row, _, _ in cp["ids"]], d["doc"]
        c, b = g["client"], g["byId"]
        assert c["checked"] > 0 and c["posEqual"] == c["checked"] and c["sameObject"] == c["checked"], (d["doc"], c)
        assert b["checked"] == len(cp["ids"]) and b["sameObject"] == b["checked"], (d["doc"], b)
        assert b["gone"] == sum(row < 0 for _, row, _, _ in cp["ids"])
        found += sum(t is not None for t in g["tiles"])
        same += c["checked"]
        by_id += b["checked"] - b["gone"]
        gone += b["gone"]
    assert found > 500 and same > 500 and by_id > 50 and gone > 10
    assert got["never"] == [None, None, None]
