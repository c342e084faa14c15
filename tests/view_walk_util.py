"""MergeTree.mapRange with a leaf action in a (refSeq, client) view, and MergeTreeTextHelper.getText
on it, restated over a document's rows for the tests (the rule of DESIGN section 26;
tests/test_view_walk.py pins it on the reference's own answers), and the streams of the fixture
tests/golden/ref_view_walk.json.gz (shared with tests/golden/make_view_walk.py).

A row is [length, seq, client, removedSeq | None, removedClient | None, overlap ids, refType | None
(a text row), properties | None, text | None (a marker)].  A view is (refSeq, client); refSeq None
is the replica's own view.  In a view a row is
    ins  = client == c or seq <= refSeq
    gone = removed and (removedClient == c or c in overlap or removedSeq <= refSeq)
its length vl = length if ins and not gone else 0 (nodeLength, MT/mergeTree.ts:1692-1732) and its
term in every ancestor's partial length pl = length * (ins - gone) (MT/partialLengths.ts).  The
replica's own view: vl = pl = length unless removed."""
import walk_streams
import walk_util

LEN, SEQ, CLI, RSEQ, RCLI, OVL, RTYPE, PROPS, TEXT = range(9)


def logs():
    """The fixture's message logs: walk_streams' documents, then one ref_wide400 document at two
    cut points.  writers / whole / seed steer the harness' sampling (fewer views and no
    whole-document walks in every view where the rows are many)."""
    import golden_util as gu
    out = []
    for i, log in enumerate(walk_streams.logs()):
        rows_many = len(log["msgs"]) >= 400
        out.append(dict(log, source="walk_streams", writers=2 if len(log["msgs"]) >= 2000 else (3 if rows_many else 4),
                        whole=0 if rows_many else 1, seed=4100 + i))
    wide = gu.load("ref_wide400")["docs"][0]
    out.append(dict(doc="wide400_0", seed_text=wide["seed_text"], msgs=wide["msgs"], checkpoints=[700, 1500],
                    source="ref_wide400", writers=6, whole=0, seed=4200))
    return out


def vis(row, view):
    """(ins, gone) of a row in a view."""
    r, c = view
    removed = row[RSEQ] is not None
    if r is None:
        return True, removed
    ins = row[CLI] == c or (row[SEQ] != -1 and row[SEQ] <= r)
    gone = removed and (row[RCLI] == c or c in row[OVL] or (row[RSEQ] != -1 and row[RSEQ] <= r))
    return ins, gone


def lengths(rows, view):
    """([vl], [pl]) per row."""
    vl, pl = [], []
    for row in rows:
        ins, gone = vis(row, view)
        vl.append(row[LEN] if ins and not gone else 0)
        pl.append(row[LEN] * (int(ins) - int(gone)))
    return vl, pl


class View:
    """A checkpoint's rows and tree (levels[l]: the child counts of the nodes of level l in
    document order; levels[0]: rows per leaf block, the last level: the root) in one view: vl and
    pl per row, and every node's partial length P[l][b] (the sum of its rows' pl)."""

    def __init__(self, rows, levels, view):
        self.levels = levels
        self.vl, self.pl = lengths(rows, view)
        self.first, self.P = [], []
        below = self.pl
        for counts in levels:
            f, at, sums = [], 0, []
            for n in counts:
                f.append(at)
                sums.append(sum(below[at:at + n]))
                at += n
            assert at == len(below)
            self.first.append(f)
            self.P.append(sums)
            below = sums
        assert len(levels[-1]) == 1
        self.N, self.L = sum(self.pl), sum(self.vl)

    def flat_walk(self, start=None, end=None):
        """The flat rule (N == L): [[row, pos, start - pos, end - pos]] for the rows with vl > 0,
        pos < end and pos + vl > start on the exclusive vl prefix; end None: N."""
        s = 0 if start is None else start
        e = self.N if end is None else end
        out, pos = [], 0
        for i, n in enumerate(self.vl):
            if n > 0 and pos < e and pos + n > s:
                out.append([i, pos, s - pos, e - pos])
            pos += n
        return out

    def tree_walk(self, start=None, end=None):
        """nodeMap (MT/mergeTree.ts:2936-2998): a leaf's length is vl, an interior node's its
        partial length; a child is entered when end > 0, len > 0 and start < len on the start
        and end shifted by the lengths before it."""
        first, P, levels, vl = self.first, self.P, self.levels, self.vl
        out = []

        def node_map(level, b, pos, s, e):
            for k in range(first[level][b], first[level][b] + levels[level][b]):
                n = vl[k] if level == 0 else P[level - 1][k]
                if e > 0 and n > 0 and s < n:
                    if level == 0:
                        out.append([k, pos, s, e])
                    else:
                        node_map(level - 1, k, pos, s, e)
                pos, s, e = pos + n, s - n, e - n

        node_map(len(levels) - 1, 0, 0, 0 if start is None else start, self.N if end is None else end)
        return out

    def tree_search(self, pos):
        """searchBlock (MT/mergeTree.ts:1830-1862): at every level the first child whose length
        exceeds what is left of pos, interior children by their partial lengths, no
        backtracking: (row, offset), or (None, None)."""
        b = 0
        for level in range(len(self.levels) - 1, -1, -1):
            hit = None
            for k in range(self.first[level][b], self.first[level][b] + self.levels[level][b]):
                n = self.vl[k] if level == 0 else self.P[level - 1][k]
                if pos < n:
                    hit = k
                    break
                pos -= n
            if hit is None:
                return None, None
            b = hit
        return b, pos


def text_of(rows, visits, placeholder):
    """gatherText over a visit list (MT/textSegment.ts:188-275, no tags outside parallelArrays...
    the plain getText mode): clipped texts, a marker as its length's worth of placeholders."""
    out = ""
    for i, _, s, e in visits:
        row = rows[i]
        if row[RTYPE] is None:
            out += walk_util.clipped(row[TEXT], s, e)
        else:
            out += placeholder * row[LEN]
    return out
