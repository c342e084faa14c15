"""Builders of the tile-marker streams (tests/golden/ref_tiles.json.gz): one definition shared by
tests/golden/make_tiles.py, which has the reference replay what is built here and record its
findTile / getMarkerFromId answers, and by the tests.  Pure Python, no reference, no GPU.

Every op is issued at the current view (ref_seq = seq - 1), so a document's length follows by
plain arithmetic; min_seq trails by `lag` messages, so removed rows -- markers among them -- stay
in the tree that long before zamboni unlinks them.  Messages are compact: [writer, seq, ref_seq,
min_seq, op].  No annotate carries referenceTileLabels or markerId."""
import random

TILE_KEY, ID_KEY = "referenceTileLabels", "markerId"
# the labels asked for: two that markers carry in lists, one only the string value "pg" yields
# (JavaScript iterates a string by character), one no marker has
LABELS = ["pg", "cell", "p", "none"]

# marker kinds: (weight, refType, labels value or None, with id)
#   refType 1: Tile; 3: Tile | NestBegin; 2, 0: no Tile bit
KINDS = [
    (5, 1, ["pg"], True),
    (3, 1, ["cell"], False),
    (2, 3, ["pg", "cell"], True),     # both labels
    (2, 1, "pg", False),              # a string value: yields "p" and "g"
    (2, 2, ["pg"], True),             # labels, but no Tile bit
    (2, 1, None, True),               # an id and no labels
    (1, 0, None, True),
    (1, 1, None, False),              # no properties at all
    (1, 1, [], False),                # an empty list: truthy, yields nothing
]

# name -> config; `end`: the tail of the stream
#   "marker": a tile marker appended at the end and removed (the last row is a removed qualifying
#             marker), "text": the same with a text row, "empty": everything removed, None: nothing
FLAT = [dict(name=f"flat{i}", seed=7100 + i, msgs=14 + 3 * i, lag=400, p_marker=0.35, p_insert=0.7, p_remove=0.15,
             text_max=4, seed_len=3, end=("marker", "marker", "text", "empty")[i % 4], checkpoints=2)
        for i in range(16)]
PAGED = [dict(name=f"paged{i}", seed=7300 + i, msgs=600, lag=(64, 150, 600)[i % 3], p_marker=0.1, p_insert=0.5,
              p_remove=0.3, text_max=8, seed_len=64, end=(None, "marker", "empty", None)[i % 4], checkpoints=3)
         for i in range(4)]
# >= 70 level-1 nodes: the directory scan crosses a 64-position chunk
BIG = [dict(name="big0", seed=7500, msgs=2000, lag=3000, p_marker=0.06, p_insert=0.86, p_remove=0.05, text_max=3,
            seed_len=8, end="marker", checkpoints=1)]
CONFIGS = FLAT + PAGED + BIG


def _text(rng, n):
    return "".join(chr(97 + rng.randrange(26)) for _ in range(n))


def build(cfg):
    """One message log: dict(doc, seed_text, msgs, checkpoints) -- checkpoints are message counts,
    ascending, the last one the whole log."""
    rng = random.Random(cfg["seed"])
    seed_text = _text(rng, cfg["seed_len"])
    length, seq, msn, ids = len(seed_text), 0, 0, 0
    msgs = []
    weights = [k[0] for k in KINDS]

    def emit(op):
        nonlocal seq, msn
        seq += 1
        msn = max(msn, seq - 1 - cfg["lag"])
        msgs.append([1 + len(msgs) % 4, seq, seq - 1, msn, op])

    def marker(ref_type, labels, with_id):
        nonlocal ids
        props = {}
        if labels is not None:
            props[TILE_KEY] = labels
        if with_id:
            ids += 1
            props[ID_KEY] = f"{cfg['name']}-m{ids}"
        seg = {"marker": {"refType": ref_type}}
        if props:
            seg["props"] = props
        return seg

    for _ in range(cfg["msgs"]):
        u = rng.random()
        if length == 0 or u < cfg["p_insert"]:
            pos = rng.randrange(length + 1)
            if rng.random() < cfg["p_marker"]:
                _, ref_type, labels, with_id = rng.choices(KINDS, weights)[0]
                emit({"pos1": pos, "seg": marker(ref_type, labels, with_id), "type": 0})
                length += 1
            else:
                text = _text(rng, 1 + rng.randrange(cfg["text_max"]))
                seg = {"text": text, "props": {"k0": rng.randrange(4)}} if rng.random() < 0.2 else text
                emit({"pos1": pos, "seg": seg, "type": 0})
                length += len(text)
        else:
            p1 = rng.randrange(length)
            n = 1
            while n < 64 and rng.random() < 0.75:
                n += 1
            p2 = min(p1 + n, length)
            if u < cfg["p_insert"] + cfg["p_remove"]:
                emit({"pos1": p1, "pos2": p2, "type": 1})
                length -= p2 - p1
            else:   # an annotate (markers in the range take the key too)
                emit({"pos1": p1, "pos2": p2, "props": {f"k{1 + rng.randrange(2)}": rng.randrange(4)}, "type": 2})
    body = len(msgs)
    end = cfg["end"]
    if end == "empty":
        while length > 0:
            n = min(length, 1 + rng.randrange(40))
            p1 = rng.randrange(length - n + 1)
            emit({"pos1": p1, "pos2": p1 + n, "type": 1})
            length -= n
    elif end in ("marker", "text"):
        seg = marker(3, ["pg", "cell"], True) if end == "marker" else "z"
        emit({"pos1": length, "seg": seg, "type": 0})
        emit({"pos1": length, "pos2": length + 1, "type": 1})
    k = cfg["checkpoints"]
    cps = sorted({max(1, body * (j + 1) // k) for j in range(k - 1)} | {len(msgs)})
    return dict(doc=cfg["name"], seed_text=seed_text, msgs=msgs, checkpoints=cps, sample=cfg.get("sample", 1))


def logs():
    return [build(c) for c in CONFIGS]
