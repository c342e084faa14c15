"""The segment-walk fixture, made by the reference itself (runs only where the reference is
present; the tests read the committed data).

The streams of tests/walk_streams.py are replayed by the transpiled reference (oracle/build_ref.py
-> oracle/_ref) through tests/golden/walk_harness.mjs, which records at every checkpoint the
segment table (lengths, removal, refType, properties, text, seq, short client) with its leaf and
level-1 partition, what Client.walkSegments handed its handler for a list of ranges, what
getTextAndMarkers answers for every label of tile_streams.LABELS, and getRangeExtentsOfPosition at
a few positions.  Output: tests/golden/ref_walk.json.gz (data only): {labels, docs: [{doc,
seed_text, msgs, checkpoints: [...]}]}."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
import walk_streams  # noqa: E402


def main():
    if not os.path.isdir(os.path.join(REPO, "oracle", "_ref")):
        subprocess.check_call([sys.executable, os.path.join(REPO, "oracle", "build_ref.py")])
    logs = walk_streams.logs()
    with tempfile.TemporaryDirectory() as td:
        ip, op = os.path.join(td, "in.json"), os.path.join(td, "out.json")
        with open(ip, "w") as f:
            json.dump({"labels": walk_streams.LABELS, "docs": logs}, f)
        subprocess.check_call(["node", os.path.join(HERE, "walk_harness.mjs"), ip, op])
        with open(op) as f:
            ref = json.load(f)
    docs = []
    for log, r in zip(logs, ref["docs"]):
        assert r["doc"] == log["doc"] and [c["n"] for c in r["checkpoints"]] == log["checkpoints"]
        docs.append(dict(doc=log["doc"], seed_text=log["seed_text"], msgs=log["msgs"], checkpoints=r["checkpoints"]))
    path = os.path.join(HERE, "ref_walk.json.gz")
    with gzip.GzipFile(path, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps({"config": {"ext": True}, "labels": walk_streams.LABELS, "docs": docs},
                           separators=(",", ":")).encode())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
