"""The remote-view segment-walk fixture, made by the reference itself (runs only where the
reference is present; the tests read the committed data).

The streams of tests/walk_streams.py and one document of tests/golden/ref_wide400.json.gz (200
writers with concurrent removes: overlap lists beyond the 63 slots) are replayed by the transpiled
reference (oracle/build_ref.py -> oracle/_ref) through tests/golden/view_walk_harness.mjs, which
records at every checkpoint the collab window, the segment table with each row's insert and
removal stamps and overlap list, the tree's child counts by level, and per sampled (refSeq,
client) view getLength, the leaves' nodeLength sum, what MergeTree.mapRange handed its leaf action
for a list of ranges and createTextHelper().getText for some of them.  The messages are not
stored again: tests/view_walk_util.py takes them from where they came.  Output:
tests/golden/ref_view_walk.json.gz (data only): {docs: [{doc, source, checkpoints: [...]}]}."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import view_walk_util  # noqa: E402


def main():
    if not os.path.isdir(os.path.join(REPO, "oracle", "_ref")):
        subprocess.check_call([sys.executable, os.path.join(REPO, "oracle", "build_ref.py")])
    logs = view_walk_util.logs()
    with tempfile.TemporaryDirectory() as td:
        ip, op = os.path.join(td, "in.json"), os.path.join(td, "out.json")
        with open(ip, "w") as f:
            json.dump({"docs": logs}, f)
        subprocess.check_call(["node", os.path.join(HERE, "view_walk_harness.mjs"), ip, op])
        with open(op) as f:
            ref = json.load(f)
    docs = []
    for log, r in zip(logs, ref["docs"]):
        assert r["doc"] == log["doc"] and [c["n"] for c in r["checkpoints"]] == log["checkpoints"]
        docs.append(dict(doc=log["doc"], source=log["source"], checkpoints=r["checkpoints"]))
    path = os.path.join(HERE, "ref_view_walk.json.gz")
    with gzip.GzipFile(path, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps({"config": {"ext": True}, "docs": docs}, separators=(",", ":")).encode())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
