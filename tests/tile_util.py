"""SharedString.findTile / getMarkerFromId restated over a document's rows, for the tests (the
rule of DESIGN section 24; tests/test_bulk_tiles.py pins it on the reference's own answers).

A row is (length, removed, ref_type, props): ref_type None for a text row, props a dict or None.
Scope is the replica's own view: a row's observer length is its length unless it is removed."""
TILE_KEY, ID_KEY = "referenceTileLabels", "markerId"
TILE_BIT = 1   # ReferenceType.Tile


def yields(value, label):
    """JavaScript's `for (const x of value) if (x === label)` (MT/mergeTree.ts:626-635) for the
    values that can be iterated: a list yields its elements, a string its characters.  Falsy
    values have no labels (refHasTileLabels); any other truthy value makes the reference throw
    and counts here as not holding the label."""
    if isinstance(value, list):
        return any(isinstance(x, str) and x == label for x in value)
    if isinstance(value, str):
        return len(label) == 1 and label in value
    return False


def qualifies(row, label):
    _, _, ref_type, props = row
    return (ref_type is not None and (ref_type & TILE_BIT) != 0 and props is not None and TILE_KEY in props
            and yields(props[TILE_KEY], label))


def find_tile(rows, pos, label, preceding=True):
    """(row, observer position of the marker) or None; pos None: undefined."""
    obs = [0 if r[1] else r[0] for r in rows]
    start, acc = [], 0
    for n in obs:
        start.append(acc)
        acc += n
    length = acc
    ok = [qualifies(r, label) and obs[i] > 0 for i, r in enumerate(rows)]
    # H: the first row whose inclusive observer prefix exceeds pos
    hit = None
    if pos is not None:
        hit = next((i for i in range(len(rows)) if start[i] + obs[i] > pos), None)
    if preceding:
        last = len(rows) - 1 if hit is None else hit
        got = next((i for i in range(last, -1, -1) if ok[i]), None)
    elif pos is None:
        got = next((i for i in range(len(rows)) if ok[i]), None)
    elif pos > length:
        got = None
    elif pos == length:
        # the descent takes the last child at every level: the last row, asked no visibility
        got = len(rows) - 1 if rows and qualifies(rows[-1], label) else None
    else:
        got = next((i for i in range(hit, len(rows)) if ok[i]), None)
    return None if got is None else (got, start[got])


def marker_from_id(rows, marker_id):
    """(row, observer position, duplicate) of the first marker row -- removed or not -- whose
    properties hold markerId == marker_id, or None."""
    got = [i for i, r in enumerate(rows) if r[2] is not None and r[3] is not None and r[3].get(ID_KEY) == marker_id]
    if not got or not marker_id:
        return None
    return got[0], sum(0 if r[1] else r[0] for r in rows[:got[0]]), len(got) > 1
