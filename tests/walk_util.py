"""Client.walkSegments and MergeTreeTextHelper.getTextAndMarkers restated over a document's
rows, for the tests (the rule of DESIGN section 25; tests/test_bulk_walk.py pins it on the
reference's own answers).

A row is (length, removed, ref_type, props, text): ref_type None for a text row, props a dict or
None, text None for a marker.  Scope is the replica's own view: a row's observer length is its
length unless it is removed."""
import tile_util

BOLD, UNDERLINE = "font-weight", "text-decoration"


def js_truthy(v):
    return not (v is None or v is False or v == 0 or v == "" or v != v)


def walk(rows, start=None, end=None):
    """[(row, pos, start - pos, end - pos)] for the rows nodeMap visits (MT/mergeTree.ts:2936-2998):
    observer length > 0, pos < end, pos + length > start; start None: 0, end None: the length."""
    obs = [0 if r[1] else r[0] for r in rows]
    s = 0 if start is None else start
    e = sum(obs) if end is None else end
    out, pos = [], 0
    for i, n in enumerate(obs):
        if n > 0 and pos < e and pos + n > s:
            out.append((i, pos, s - pos, e - pos))
        pos += n
    return out


def js_substring(text, start, end):
    """String.prototype.substring: both ends clamped into [0, length], swapped when start > end."""
    a, b = (min(max(x, 0), len(text)) for x in (start, end))
    return text[min(a, b):max(a, b)]


def clipped(text, start, end):
    """What gatherText appends of a visited text row (MT/textSegment.ts:241-252)."""
    if start <= 0 and end >= len(text):
        return text
    if start < 0:
        start = 0
    return text[start:] if end >= len(text) else js_substring(text, start, end)


def text_and_markers(rows, label, visits=None):
    """(parallelText, rows of parallelMarkers): gatherText in its parallelArrays mode over a walk of
    the whole document (or the given visits), MT/textSegment.ts:188-275 -- the <b> / <u> tags of
    truthy font-weight / text-decoration with the tagsInProgress bookkeeping as written there;
    a marker holding the label closes a text; the text after the last one is dropped."""
    texts, markers, cur, in_progress = [], [], "", []
    for i, _, s, e in (walk(rows) if visits is None else visits):
        _, _, ref_type, props, text = rows[i]
        if ref_type is None:
            tags = [t for t, k in (("b", BOLD), ("u", UNDERLINE)) if props and js_truthy(props.get(k))]
            begin, end_tags, init, rem = "", "", [], []
            if tags:
                for t in tags:
                    if t not in in_progress:
                        begin += f"<{t}>"
                        init.append(t)
                for t in in_progress:
                    if t not in tags:
                        end_tags += f"</{t}>"
                        rem.append(t)
                in_progress += init[::-1]
            else:
                for t in in_progress:
                    end_tags += f"</{t}>"
                    rem.append(t)
            for t in rem:
                if t in in_progress:
                    in_progress.remove(t)
            cur += end_tags + begin + clipped(text, s, e)
        elif tile_util.qualifies(rows[i][:4], label):
            markers.append(i)
            texts.append(cur)
            cur = ""
    return texts, markers


def range_extents(rows, pos):
    """Client.getRangeExtentsOfPosition (MT/client.ts:1026-1043): (posStart, posAfterEnd) of the row
    holding pos, (None, None) when there is none."""
    at = 0
    for r in rows:
        n = 0 if r[1] else r[0]
        if 0 <= pos - at < n:
            return at, at + r[0]
        at += n
    return None, None
