"""The delta-log walk (csrc/mt_dlog.h) as a host program under AddressSanitizer and
UndefinedBehaviorSanitizer (CPU).  tests/dlog_walk_main.cpp copies every span into a heap
allocation of exactly its size, so a load outside the span is a report and a failed run: this
is where the walk's bounds are proven.  Well-formed spans are the reference-made logs of the
fixtures (the words the device logs must equal: tests/test_gpu_parity.py, test_live_client.py)
and must give the rows of the Python restatement (tests/delta_util.py); truncated, mid-record
and hostile spans must give BAD -- or whatever the restatement reads in them -- and no report."""
import os
import subprocess

import pytest

import delta_util as du
import golden_util as gu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MAX, I32_MIN = 0x7FFFFFFF, -(1 << 31)


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    """Runs spans [(rich, words)] through the sanitized program -> [rows | None] per span."""
    d = tmp_path_factory.mktemp("dlog_walk")
    exe = str(d / "dlog_walk")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(REPO, "tests", "dlog_walk_main.cpp")], check=True)
    count = [0]

    def run(spans):
        count[0] += 1
        path = str(d / f"spans{count[0]}.txt")
        with open(path, "w") as fh:
            for rich, words in spans:
                fh.write(" ".join(str(x) for x in [int(bool(rich)), len(words)] + [_i32(int(w)) for w in words]) + "\n")
        p = subprocess.run([exe, path], capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
        lines, out, i = p.stdout.split("\n"), [], 0
        for _ in spans:
            if lines[i] == "BAD":
                out.append(None)
                i += 1
                continue
            tag, n = lines[i].split()
            assert tag == "OK"
            out.append([tuple(int(x) for x in ln.split()) for ln in lines[i + 1:i + 1 + int(n)]])
            i += 1 + int(n)
        assert lines[i:] == [""]
        return out

    return run


# ---------------------------------------------------------------- reference-made logs
def _plain_logs(name):
    fx = gu.load(name)
    interner = gu.interner_for(fx)
    return [gu.expected(doc, interner)["deltas"] for doc in fx["docs"]]


def _live_logs():
    from fluidframework_amd.wire import Interner
    fx = gu.load("ref_live")
    return [gu.expected_live(doc, Interner(synthetic=True))["deltas"] for doc in fx["docs"]]


def _encode_rich(events, ext=None):
    """expected_rich's form -> the words of a rich log (the inverse of gu.parse_rich_log).  ext:
    a function (event index, segment index) -> (uid, position, ordinal tuple | None) for a
    segment_ordinals log."""
    w = []

    def state(st, ln, e, k):
        props = st[2]
        flags = (1 if st[0] == "m" else 0) | (2 if props is not None else 0) | (4 if ext else 0)
        w.append(flags)
        if st[0] == "m":
            w.append(st[1])
        else:
            b = st[1].encode("utf-16-le", errors="surrogatepass")
            units = [b[2 * j] | (b[2 * j + 1] << 8) for j in range(len(b) // 2)]
            assert len(units) == ln
            units += [0] * (len(units) & 1)
            w.extend(units[2 * j] | (units[2 * j + 1] << 16) for j in range(len(units) // 2))
        w.append(-1 if props is None else len(props))
        for key, val in props or ():
            w.extend([key, val])
        if ext:
            uid, pos, o = ext(e, k)
            w.extend([uid, pos, -1 if o is None else len(o)] + list(o or ()))

    for e, ev in enumerate(events):
        if ev[0] == "D":
            _, seq, kind, segs = ev
            w.extend([seq, kind, len(segs)])
            for k, (pos, ln, pd, st) in enumerate(segs):
                w.extend([pos, ln])
                if kind == 2:
                    w.append(len(pd))
                    for key, old in pd:
                        w.extend([key, old])
                state(st, ln, e, k)
        else:
            _, kind, segs = ev
            w.extend([0, kind, len(segs)])
            for k, (ln, st) in enumerate(segs):
                w.append(ln)
                state(st, ln, e, k)
    return [_i32(x) for x in w]


def _some_ext(e, k):
    """A made-up [uid, position, ordinal]: every ordinal length from none to 4."""
    o = [None, (), (7,), (7, 0), (1, 2, 3), (9, 9, 9, 9)][(e + k) % 6]
    return (0 if o is None else 1000 + 3 * e + k, e % 50, o)


def _rich_logs():
    fx = gu.load("ref_rich")
    interner = gu.Interner()
    out = []
    for doc in fx["docs"]:
        events = gu.expected_rich(doc, interner)
        plain, ord_ = _encode_rich(events), _encode_rich(events, _some_ext)
        assert gu.parse_rich_log(plain) == events     # the encoder is parse_rich_log's inverse
        got_ext = []
        assert gu.parse_rich_log(ord_, got_ext) == events
        assert got_ext == [[_some_ext(e, k) for k in range(len(ev[-1]))] for e, ev in enumerate(events)]
        out.append((plain, ord_))
    return out


def _whole_records(words, rich, limit):
    """The longest prefix of whole records within `limit` words, and the record boundaries in it."""
    bounds = [0]
    du.rows(words, rich, bounds)
    bounds = [b for b in bounds if b <= limit]
    return words[:bounds[-1]], bounds


def test_walk_matches_restatement_on_reference_logs(walker):
    """Plain (ref_small), live (ref_live: npd == -1 where propertyDeltas is undefined), rich and
    rich + ordinals (ref_rich) logs, whole: the rows of the restatement; for the plain ones also
    the reference's own (seq, kind, position, length) per delta segment."""
    spans = [(False, w) for w in _plain_logs("ref_small")] + [(False, w) for w in _live_logs()]
    for plain, ord_ in _rich_logs():
        spans += [(True, plain), (True, ord_)]
    assert any(-1 in [w[r[5] + 2] for r in du.rows(w, False) if r[2] == 2] for w in _live_logs())   # npd == -1 occurs
    got = walker(spans)
    n_rows = 0
    for (rich, w), g in zip(spans, got):
        assert g is not None and g == du.rows(w, rich)
        n_rows += len(g)
    assert n_rows > 5000
    fx = gu.load("ref_small")
    for doc, g in zip(fx["docs"], got):
        assert [(r[1], r[2], r[3], r[4]) for r in g] == du.reference_ranges(doc)
    # a maintenance row's position is its ext position; without ordinals it is -1
    rich_rows = [(g, spans[i][1]) for i, g in enumerate(got) if spans[i][0]]
    assert any(r[2] < 0 and r[3] >= 0 and r[6] != du.NO_UID for g, _ in rich_rows for r in g)
    assert any(r[2] < 0 and r[3] == -1 and r[6] == du.NO_UID for g, _ in rich_rows for r in g)


@pytest.mark.parametrize("kind", ["plain", "rich_ordinals"])
def test_walk_truncations_and_mid_record_starts(walker, kind):
    """Every prefix and every suffix of a log's head: a prefix is well formed exactly when it ends
    on a record boundary; a suffix that starts inside a record is BAD unless the restatement
    reads it as records too; never a load outside the span."""
    rich = kind != "plain"
    full = _rich_logs()[0][1] if rich else _plain_logs("ref_small")[0]
    words, bounds = _whole_records(full, rich, 400)
    assert 200 < len(words) <= 400 and len(bounds) > 10
    spans = [(rich, words[:k]) for k in range(len(words) + 1)] + [(rich, words[k:]) for k in range(len(words) + 1)]
    got = walker(spans)
    want = [du.rows_or_none(w, rich) for _, w in spans]
    assert got == want
    for k in range(len(words) + 1):
        assert (got[k] is not None) == (k in bounds), k
    mid = [k for k in range(len(words) + 1) if k not in bounds]
    # (small integers often read as records, so many mid-record suffixes are well formed words;
    # the last two suffixes hold fewer than a header's three words and cannot be)
    assert got[2 * len(words)] is None and got[2 * len(words) - 1] is None and len(mid) > 100


def test_walk_hostile_counts(walker):
    """n, npd, np, the text length and olen at 0x7FFFFFFF, negative and INT_MIN."""
    cases = []   # (rich, words, well formed?)
    for v in (I32_MAX, -1, I32_MIN, 2):
        cases.append((False, [1, 0, v], False))
        cases.append((True, [1, -2, v], False))
        cases.append((False, [1, 0, v, 5, 1], False))
    for v, ok in ((I32_MAX, False), (3, False), (-1, True), (I32_MIN, True), (0, True)):
        cases.append((False, [1, 2, 1, 0, 3, v], ok))                              # npd
        cases.append((True, [1, 0, 1, 0, 2, 2, 0x00410041, v], ok))                # np
        cases.append((True, [1, 0, 1, 0, 2, 4, 0x00410041, -1, 77, 5, v], ok))     # olen
        cases.append((True, [0, -1, 1, 2, 4, 0x00410041, -1, 77, 5, v], ok))       # olen, maintenance
    for v in (I32_MAX, I32_MAX - 1, -1, I32_MIN, 3):
        cases.append((True, [1, 0, 1, 0, v, 0, 0x00410041, -1], False))            # text length vs the words left
    cases.append((True, [1, 0, 1, 0, I32_MAX, 1, 0, -1], True))                    # (a marker's length is not a count)
    cases.append((False, [], True))
    cases.append((True, [], True))
    cases.append((False, [1, 0, 0], True))
    cases.append((False, [1, 0, 0, 1], False))
    cases.append((False, [1, 0], False))
    got = walker([(r, w) for r, w, _ in cases])
    for (rich, w, ok), g in zip(cases, got):
        assert (g is not None) == ok, (rich, w)
        assert g == du.rows_or_none(w, rich), (rich, w)
    # records with n == 0 advance `record` and add no row
    (g,) = walker([(False, [1, 0, 0, 2, 0, 1, 4, 1, 3, 1, 0])])
    assert g == [(1, 2, 0, 4, 1, 6, du.NO_UID)]
