"""The rows of mt_get_delta_logs restated in Python: golden_util.parse_rich_log's walk of a
delta log (plain or rich, with or without segment ordinals, live handles' npd == -1), keeping
per entry what mt_delta_range holds instead of the segments' state.  The device walk
(csrc/mt_dlog.h) is compared against this on the GPU (tests/test_bulk_deltas.py) and, compiled
as a host program under the sanitizers, on the CPU (tests/test_dlog_walk.py)."""
import numpy as np

NO_UID = 0xFFFFFFFF
OVERFLOWED, PAST, BAD = 1, 2, 4
FIELDS = ("record", "seq", "kind", "position", "length", "word", "uid")


class BadSpan(Exception):
    """The words are not a whole number of well-formed records."""


class _Span:
    def __init__(self, words):
        self.w = [int(x) for x in words]
        self.i = 0

    def take(self):
        if self.i >= len(self.w):
            raise BadSpan(self.i)
        self.i += 1
        return self.w[self.i - 1]

    def skip(self, k):
        """Steps over k words that must all be there (k < 0 is malformed)."""
        if k < 0 or k > len(self.w) - self.i:
            raise BadSpan(self.i)
        self.i += k


def rows(words, rich, bounds=None):
    """[(record, seq, kind, position, length, word, uid)] of the span's entries in order; raises
    BadSpan when the span does not end exactly on a record's end or a count steps outside it.
    bounds: a list that receives the offset of every record's end."""
    s, out, record = _Span(words), [], 0
    while s.i < len(s.w):
        seq, kind, n = s.take(), s.take(), s.take()
        if n < 0:
            raise BadSpan(s.i)
        for _ in range(n):
            word, position, uid = s.i, -1, NO_UID
            if kind >= 0:
                position, length = s.take(), s.take()
                if kind == 2:
                    s.skip(2 * max(s.take(), 0))      # npd (-1: propertyDeltas undefined)
            else:
                length = s.take()
            if rich:
                flags = s.take()
                s.skip(1 if flags & 1 else (length + 1) // 2 if length >= 0 else -1)
                s.skip(2 * max(s.take(), 0))          # np (-1: no properties)
                if flags & 4:
                    uid, epos, olen = s.take() & 0xFFFFFFFF, s.take(), s.take()
                    s.skip(max(olen, 0))
                    if kind < 0:
                        position = epos
            out.append((record, seq, kind, position, length, word, uid))
        record += 1
        if bounds is not None:
            bounds.append(s.i)
    return out


def rows_or_none(words, rich):
    try:
        return rows(words, rich)
    except BadSpan:
        return None


def expected_rows(off, words, rich, dtype):
    """(row_off, rows, bad) of a drained result: query q's words are words[off[q]:off[q + 1]];
    bad[q]: the query's span is malformed (zero rows, MT_DLOG_BAD)."""
    per, bad = [], []
    for q in range(len(off) - 1):
        r = rows_or_none(words[int(off[q]):int(off[q + 1])], rich)
        bad.append(r is None)
        per.append([(q,) + x for x in (r or [])])
    row_off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64)
    flat = [x for p in per for x in p]
    return row_off, np.array(flat, dtype=dtype) if flat else np.zeros(0, dtype=dtype), bad


def reference_ranges(doc):
    """(seq, kind, position, length) of every delta segment of a plain fixture document, from the
    reference's own callbacks."""
    return [(seq, kind, s[0], s[1]) for seq, kind, n, dsegs in doc["out"]["deltas"] for s in dsegs]
