"""Builders of the segment-walk streams (tests/golden/ref_walk.json.gz): one definition shared by
tests/golden/make_walk.py, which has the reference replay what is built here and record what
Client.walkSegments hands its handler, getTextAndMarkers and getRangeExtentsOfPosition, and by
the tests.  Pure Python, no reference, no GPU.

The markers are the kinds of tests/tile_streams.py; added here is what those streams lack: text
inserts of 65-300 units (odd and even lengths: one row's text crosses the 64-lane dealing of the
gather and lands on odd destination offsets), inserted property sets {}, of 1-3 keys and none,
annotates that set font-weight / text-decoration to truthy values, to falsy ones (0, "") and to
null (which deletes the key), and min-seq lags that keep removed rows in the tree.

Every op is issued at the current view (ref_seq = seq - 1), so a document's length follows by
plain arithmetic.  Messages are compact: [writer, seq, ref_seq, min_seq, op]."""
import random

from tile_streams import ID_KEY, KINDS, LABELS, TILE_KEY  # noqa: F401  (LABELS: the labels asked for)

BOLD, UNDERLINE = "font-weight", "text-decoration"
TAG_VALUES = ["bold", 1, "underline", 0, "", None]      # truthy, truthy, truthy, falsy, falsy, delete

# name -> config; `end`: "empty": everything removed at the end, "marker": a labelled tile marker
# appended (the text after the last labelled marker is then empty), None: nothing
FLAT = [dict(name=f"flat{i}", seed=9100 + i, msgs=6 + 2 * i, lag=(400, 6)[i % 2], p_marker=0.25, p_insert=0.7,
             p_remove=0.12, p_long=0.2, text_max=5, seed_len=(3, 70, 0, 131)[i % 4],
             end=(None, None, "marker", None)[i % 4], checkpoints=2)
        for i in range(12)]
EMPTIED = [dict(name="emptied0", seed=9200, msgs=14, lag=400, p_marker=0.25, p_insert=0.7, p_remove=0.12, p_long=0.2,
                text_max=5, seed_len=9, end="empty", checkpoints=2)]
PAGED = [dict(name=f"paged{i}", seed=9300 + i, msgs=(420, 480, 500, 700)[i], lag=(64, 150, 600, 30)[i], p_marker=0.1,
              p_insert=0.5, p_remove=0.27, p_long=0.04, text_max=8, seed_len=64, end=(None, "marker", None, None)[i],
              checkpoints=(3, 2, 3, 2)[i])
         for i in range(4)]
# >= 70 level-1 nodes: the directory scan crosses a 64-position chunk
BIG = [dict(name="big0", seed=9500, msgs=2000, lag=3000, p_marker=0.06, p_insert=0.84, p_remove=0.05, p_long=0.01,
            text_max=3, seed_len=8, end=None, checkpoints=1)]
CONFIGS = FLAT + EMPTIED + PAGED + BIG


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

    def text_seg():
        if rng.random() < cfg["p_long"]:
            text = _text(rng, 65 + rng.randrange(236))          # 65..300, odd and even
        else:
            text = _text(rng, 1 + rng.randrange(cfg["text_max"]))
        u = rng.random()
        if u < 0.15:
            return text, {"text": text, "props": {}}
        if u < 0.45:
            keys = rng.sample(["k0", "k1", "k2", BOLD, UNDERLINE], 1 + rng.randrange(3))
            props = {k: (rng.choice(["bold", 1, 0, ""]) if k in (BOLD, UNDERLINE) else rng.randrange(4)) for k in keys}
            return text, {"text": text, "props": props}
        return text, text

    for _ in range(cfg["msgs"]):
        u = rng.random()
        if length == 0 or u < cfg["p_insert"]:
            pos = rng.randrange(length + 1)
            if rng.random() < cfg["p_marker"]:
                _, ref_type, labels, with_id = rng.choices(KINDS, weights)[0]
                emit({"pos1": pos, "seg": marker(ref_type, labels, with_id), "type": 0})
                length += 1
            else:
                text, seg = text_seg()
                emit({"pos1": pos, "seg": seg, "type": 0})
                length += len(text)
        else:
            p1 = rng.randrange(length)
            n = 1
            while n < 96 and rng.random() < 0.8:
                n += 1
            p2 = min(p1 + n, length)
            if u < cfg["p_insert"] + cfg["p_remove"]:
                emit({"pos1": p1, "pos2": p2, "type": 1})
                length -= p2 - p1
            else:   # an annotate (markers in the range take the key too)
                v = rng.random()
                if v < 0.6:
                    props = {rng.choice([BOLD, UNDERLINE]): rng.choice(TAG_VALUES)}
                elif v < 0.7:
                    props = {BOLD: rng.choice(TAG_VALUES), UNDERLINE: rng.choice(TAG_VALUES)}
                else:
                    props = {f"k{rng.randrange(3)}": rng.choice([0, 1, 2, 3, None])}
                emit({"pos1": p1, "pos2": p2, "props": props, "type": 2})
    body = len(msgs)
    if cfg["end"] == "empty":
        while length > 0:
            n = min(length, 1 + rng.randrange(40))
            p1 = rng.randrange(length - n + 1)
            emit({"pos1": p1, "pos2": p1 + n, "type": 1})
            length -= n
    elif cfg["end"] == "marker":
        emit({"pos1": length, "seg": marker(3, ["pg", "cell"], True), "type": 0})
    k = cfg["checkpoints"]
    cps = sorted({max(1, body * (j + 1) // k) for j in range(k - 1)} | {len(msgs)})
    return dict(doc=cfg["name"], seed_text=seed_text, msgs=msgs, checkpoints=cps)


def logs():
    return [build(c) for c in CONFIGS]
