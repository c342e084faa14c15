"""Builders of the zamboni stream fixtures (tests/golden/ref_zam_*.json.gz): one definition
shared by tests/golden/make_golden.py --zamboni, which has the reference replay what is built
here, and by the tests, which check the committed data against it.  Pure Python, no reference,
no GPU: configs of the generated streams, the hand-built message logs (compact messages
[writer, seq, ref_seq, min_seq, op]) and plain arithmetic on them."""
import random

MT_GRAN = 256   # TextSegment.TextSegmentGranularity: no append to a row longer than this
MT_WAVE = 64    # rows per gather iteration of a merge (scour_group)

# ---------------------------------------------------------------- generated streams (harness "gen", ext)
_ZERO = {"p_insert_props": 0, "p_marker": 0, "p_rewrite": 0, "p_group": 0, "p_noop": 0, "p_empty": 0, "p_oob": 0}
RANDOM_CONFIGS = {
    # rows far over MT_GRAN and over one wave of text: the serial plan (ScourPlan.big), the
    # pl.big / p2.big fallbacks of the in-place routes, scour_group's second gather iteration
    "ref_zam_long": {"ext": True, "seed": 9143, "ops": 3000, "writers": 6, "lag": 48, "seed_len": 600,
                     "p_insert": 0.45, "p_remove": 0.3, "text_max": 300, "p_newline": 0.002,
                     "p_len_continue": 0.97, "p_insert_props": 0.1, "n_keys": 2, "max_keys_per_op": 1,
                     "p_marker": 0.02, "p_rewrite": 0.2, "p_group": 0.02, "p_noop": 0.02, "p_empty": 0.01,
                     "p_oob": 0.01},
    # three writers two messages behind, no properties, no newlines: nearly every message settles
    # and merges (thousands of APPENDs), rows grow past MT_GRAN by appends alone
    "ref_zam_settle": dict(_ZERO, ext=True, seed=9202, ops=3000, writers=3, lag=2, seed_len=64, p_insert=0.6,
                           p_remove=0.25, text_max=40, p_newline=0, p_len_continue=0.8, n_keys=1,
                           max_keys_per_op=1),
    # paged documents full of markers and trailing newlines: what the in-place plan carries
    # across lanes (the group's last member's newline flag, the marker bit of the uid word)
    "ref_zam_marks": {"ext": True, "seed": 9306, "ops": 5000, "writers": 4, "lag": 32, "seed_len": 64,
                      "p_insert": 0.55, "p_remove": 0.15, "text_max": 6, "p_newline": 0.2,
                      "p_len_continue": 0.7, "p_insert_props": 0.1, "n_keys": 2, "max_keys_per_op": 1,
                      "p_marker": 0.3, "p_rewrite": 0.2, "p_group": 0.02, "p_noop": 0.02, "p_empty": 0.01,
                      "p_oob": 0.01},
}
RANDOM_DOCS = 4

# ---------------------------------------------------------------- ref_zam_shrink
SHRINK_FROM, SHRINK_DOCS = "ref_c3", 4
SHRINK_TAIL = 2500        # messages after the ref_c3 part
SHRINK_LOW, SHRINK_HIGH = 3, 1500
SHRINK_SEED = 9404


def _tail_text(rng, n):
    return "".join(chr(97 + rng.randrange(26)) for _ in range(n))


def shrink_tail(msgs, length, writers, seed):
    """The tail after a document's ref_c3 messages: every op is issued at the current view
    (ref_seq = seq - 1, min_seq = max(previous, seq - 1 - 64)), so the document's length follows
    by plain arithmetic.  Removes (geometric length, continue .85, cap 64) with 15 % inserts
    until the length is <= SHRINK_LOW, 80 % inserts until it is >= SHRINK_HIGH, removes again
    to the end.  Returns the SHRINK_TAIL messages."""
    rng = random.Random(seed)
    seq, msn = msgs[-1][1], msgs[-1][3]
    out, phase = [], 0
    while len(out) < SHRINK_TAIL:
        seq += 1
        msn = max(msn, seq - 1 - 64)
        if phase == 0 and length <= SHRINK_LOW:
            phase = 1
        elif phase == 1 and length >= SHRINK_HIGH:
            phase = 2
        p_ins = 0.8 if phase == 1 else 0.15
        if length == 0 or rng.random() < p_ins:
            text = _tail_text(rng, 1 + rng.randrange(8))
            op = {"pos1": rng.randrange(length + 1), "seg": text, "type": 0}
            length += len(text)
        else:
            p1 = rng.randrange(length)
            n = 1
            while n < 64 and rng.random() < 0.85:
                n += 1
            p2 = min(p1 + n, length)
            op = {"pos1": p1, "pos2": p2, "type": 1}
            length -= p2 - p1
        out.append([1 + len(out) % writers, seq, seq - 1, msn, op])
    return out


def tail_lengths(length, tail):
    """The document's length after each tail message, from `length` before the first."""
    out = []
    for m in tail:
        op = m[4]
        length += len(op["seg"]) if op["type"] == 0 else op["pos1"] - op["pos2"]
        out.append(length)
    return out


def shrink_doc(doc, writers, index):
    """One ref_zam_shrink message log from a ref_c3 document (its messages, then the tail).  The
    tail's seed is the first from SHRINK_SEED + 100 * index on whose first phase ends at length
    0 exactly (it stops at <= SHRINK_LOW), so that the tree empties before it grows again."""
    for seed in range(SHRINK_SEED + 100 * index, SHRINK_SEED + 100 * index + 100):
        tail = shrink_tail(doc["msgs"], doc["out"]["length"], writers, seed)
        ln = tail_lengths(doc["out"]["length"], tail)
        if 0 in ln and max(ln[ln.index(0):]) >= SHRINK_HIGH:
            return dict(doc=doc["doc"], seed_text=doc["seed_text"], msgs=doc["msgs"] + tail)
    raise AssertionError("no tail seed empties the document")


# ---------------------------------------------------------------- ref_zam_comb
COMB_PREFIX, COMB_TRIGGER, COMB_STEP = 600, 400, 100
# case: (unit, newline every, marker every, props cycle, remove every)
COMB_CASES = {
    "short": dict(unit=5),
    "mid": dict(unit=40),
    "long": dict(unit=300),
    "nl": dict(unit=5, nl=3),
    "mark": dict(unit=5, mark=5),
    "props2": dict(unit=5, props=(1, 1, 2, 2)),
    "rm": dict(unit=5, rm=2),
    "rmlong": dict(unit=300, rm=3),
}
# the reference's final state per case: (rows, leaf blocks, APPEND, UNLINK), asserted on the
# committed fixture by tests/test_oracle.py
COMB_FINAL = {
    "short": (2, 1, 998, 0),      # everything collapses: rows of 3399 and 1 units
    "mid": (2, 1, 998, 0),        # rows of 24399 and 1 units
    "long": (601, 150, 399, 0),   # every join candidate is over MT_GRAN: only the tail merges
    "nl": (241, 55, 759, 0),
    "mark": (265, 60, 735, 0),
    "props2": (302, 73, 698, 0),
    "rm": (2, 1, 698, 300),
    "rmlong": (401, 86, 399, 200),
}


def _unit_text(i, unit):
    return "".join(chr(97 + (7 * i + j) % 26) for j in range(unit))


def comb_doc(case):
    """(message log, checkpoints) of one comb case.  Prefix: COMB_PREFIX inserts at the
    document's end from three writers in turn with min_seq 0 -- nothing settles, the tree is a
    comb of four-row leaf blocks -- then, for the `rm` cases, removes of every rm-th row, still
    unsettled.  Trigger: COMB_TRIGGER one-unit inserts at the end with min_seq = seq - 1: the
    op's page stays the last one while zamboni pops the oldest segments, block by block, on
    the far pages.  Checkpoints: the message counts after the prefix and after every
    COMB_STEP trigger messages."""
    c = COMB_CASES[case]
    unit = c["unit"]
    msgs, rows, length, seq = [], [], 0, 0
    for i in range(COMB_PREFIX):
        seq += 1
        if c.get("mark") and i % c["mark"] == c["mark"] - 1:
            seg, n = {"marker": {"refType": 1}}, 1
        else:
            text = _unit_text(i, unit)
            if c.get("nl") and i % c["nl"] == c["nl"] - 1:
                text = text[:-1] + "\n"
            seg, n = text, unit
            if c.get("props"):
                seg = {"text": text, "props": {"k0": c["props"][i % len(c["props"])]}}
        msgs.append([1 + i % 3, seq, seq - 1, 0, {"pos1": length, "seg": seg, "type": 0}])
        rows.append((length, n))
        length += n
    if c.get("rm"):   # from the end backwards: the positions of the rows before stand
        for i in reversed(range(COMB_PREFIX)):
            if i % c["rm"] == c["rm"] - 1:
                seq += 1
                p, n = rows[i]
                msgs.append([1 + seq % 3, seq, seq - 1, 0, {"pos1": p, "pos2": p + n, "type": 1}])
                length -= n
    n_prefix = len(msgs)
    for i in range(COMB_TRIGGER):
        seq += 1
        msgs.append([1 + i % 3, seq, seq - 1, seq - 1, {"pos1": length, "seg": chr(65 + i % 26), "type": 0}])
        length += 1
    return dict(doc=case, seed_text="", msgs=msgs), list(range(n_prefix, len(msgs) + 1, COMB_STEP))


# ---------------------------------------------------------------- fixture conditions
def row_stats(out):
    """What a fixture is for, read off the reference's final tree: rows, rows over MT_WAVE and
    over MT_GRAN units, the longest row, leaf blocks, markers, rows ending in a newline."""
    segs = out["segs"]
    ends, pos = 0, 0
    for r in segs:
        if r["rseq"] is None and r["marker"] is None:   # (markers have no text)
            if r["len"] > 0 and out["text"][pos + r["len"] - 1] == "\n":
                ends += 1
            pos += r["len"]
    return dict(rows=len(segs), over_wave=sum(r["len"] > MT_WAVE for r in segs),
                over_gran=sum(r["len"] > MT_GRAN for r in segs), longest=max([r["len"] for r in segs] + [0]),
                blocks=len(out["leaves"]), markers=sum(r["marker"] is not None for r in segs), nl_rows=ends)
