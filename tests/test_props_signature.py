"""The property-set signature in the segment row (csrc/mt_engine.h SEGF_PSIG_MASK): twelve bits
of the flags word hold the sum modulo 4096 of one mix per stored {key, value} pair of the record
the row's handle names.  Zamboni's matchProperties answers "different" from two rows' bits alone
and reads the records only when the bits agree, so the bits must follow the record through every
writer (insert, annotate with replace / delete / append / rewrite / a combining op's table, the
merges' keepers, page packs, conversions, hand-overs, growth): stale bits would keep equal
neighbours apart.  Equal bits decide nothing, so distinct sets whose signatures collide must
stay apart too.  Everything is compared with the C restatement, which compares contents only."""
import itertools
import json
import os

import numpy as np
import pytest

import golden_util as gu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


# ---------------------------------------------------------------- the host function (no GPU)
def _sig(pairs):
    from fluidframework_amd import props_signature
    return props_signature(pairs)


def test_host_signature_is_a_sum_of_pair_mixes():
    """mt_props_signature does not depend on the pairs' order, is 0 for no pairs, fits twelve
    bits, and adding / removing / replacing a pair moves it by that pair's own mix modulo 4096
    (what annotate_record does from the stored bits alone)."""
    rng = np.random.default_rng(7)
    assert _sig([]) == 0
    mixes = set()
    for _ in range(200):
        n = int(rng.integers(1, 9))
        keys = rng.choice(64, size=n, replace=False)
        pairs = [(int(k), int(rng.integers(0, 1 << 31))) for k in keys]
        s = _sig(pairs)
        assert 0 <= s < 4096
        assert _sig(pairs[::-1]) == s
        assert _sig([pairs[i] for i in rng.permutation(n)]) == s
        assert s == sum(_sig([p]) for p in pairs) % 4096
        # remove the last pair; replace the first one's value
        assert _sig(pairs[:-1]) == (s - _sig([pairs[-1]])) % 4096
        k0, v0 = pairs[0]
        assert _sig([(k0, v0 ^ 1)] + pairs[1:]) == (s - _sig([(k0, v0)]) + _sig([(k0, v0 ^ 1)])) % 4096
        mixes.update(_sig([p]) for p in pairs)
    assert len(mixes) > 500, "the mix hardly spreads"
    # the flag bits of a value id take part (a falsy 0 and a plain 0 are different values)
    assert _sig([(1, 0)]) != _sig([(1, 0x80000000)])


# ---------------------------------------------------------------- handles
def _c3(ops):
    return dict(json.load(open(os.path.join(REPO, "bench", "configs.json")))["c3"], ops=ops)


def _bench_c3_caps():
    """The bench's C3 capacities (they select P_C3) behind a 16-segment LDS tier."""
    import bench
    caps = dict(bench.capacities(_c3(10000)), lds_seg_capacity=16)
    assert (caps["lds_page_capacity"], caps["lds_unsettled_capacity"], caps["lds_page_heap_capacity"]) == (192, 220, 192)
    return caps


PARITY = {
    "paged": dict(lds_seg_capacity=-1, page_capacity=256, unsettled_capacity=2048, page_heap_capacity=2048),
    "narrow": dict(lds_seg_capacity=16, page_capacity=256, unsettled_capacity=2048, page_heap_capacity=2048,
                   lds_page_capacity=200, lds_unsettled_capacity=600, lds_page_heap_capacity=600,
                   lds_narrow_overlap=1),
    "grow": dict(lds_seg_capacity=16, page_capacity=12, unsettled_capacity=16, page_heap_capacity=16),
}
FLAT = dict(seg_capacity=8192, text_capacity=1 << 17)
TIERS = ["bench_c3", "paged", "narrow", "delta_log", "flat"]


def _tier_caps(tier):
    if tier == "bench_c3":
        return dict(_bench_c3_caps(), delta_log_capacity=0)
    if tier == "delta_log":   # the window route: no in-place scour
        return dict(_bench_c3_caps(), delta_log_capacity=1 << 16)
    if tier == "flat":
        return dict(FLAT, delta_log_capacity=0)
    return dict(FLAT, delta_log_capacity=0, **PARITY[tier])


# ---------------------------------------------------------------- documents built by hand
class _Doc:
    """Messages of one document by one writer; sequence numbers count up from 1."""

    def __init__(self, seed="seed"):
        self.seed = seed
        self.msgs = []
        self.len = len(seed)

    @property
    def seq(self):
        return len(self.msgs)

    def send(self, op, msn=0):
        seq = self.seq + 1
        self.msgs.append(dict(clientId="client-1", sequenceNumber=seq, referenceSequenceNumber=seq - 1,
                              minimumSequenceNumber=msn, type="op", contents=op))

    def ins(self, text, props=None):
        """Appends a segment; returns its range."""
        p = self.len
        self.send({"type": 0, "pos1": p, "seg": {"text": text, "props": props} if props else text})
        self.len += len(text)
        return p, p + len(text)

    def ann(self, rng, props, comb=None):
        op = {"type": 2, "pos1": rng[0], "pos2": rng[1], "props": props}
        if comb:
            op["combiningOp"] = comb
        self.send(op)

    def settle(self, n=48):
        """The minimum sequence number follows the messages: everything before settles, and
        zamboni gets n messages to scour what it queued."""
        for _ in range(n):
            p = self.len
            self.send({"type": 0, "pos1": p, "seg": "z"}, msn=self.seq)
            self.len += 1


REWRITE = {"name": "rewrite"}
K = lambda *kv: {f"k{k}": v for k, v in zip(kv[::2], kv[1::2])}   # noqa: E731


def _routes(d, tail):
    """Seven three-unit neighbours.  Five reach {k1: 1, k2: 2} by different routes -- an insert
    with the set, an annotate adding k1 behind k2 (the other key order), two annotates on a bare
    segment, a third key added and nulled again, a rewrite over another set -- and must end as
    one segment once settled; the sixth differs in one value and must stay apart, as must the
    seventh (the set again) behind it.  `tail` names the texts."""
    d.ins("a" + tail, K(1, 1, 2, 2))
    r = d.ins("b" + tail, K(2, 2))
    d.ann(r, K(1, 1))
    r = d.ins("c" + tail)
    d.ann(r, K(2, 2))
    d.ann(r, K(1, 1))
    r = d.ins("d" + tail, K(1, 1, 2, 2))
    d.ann(r, K(3, 5))
    d.ann(r, K(3, None))
    r = d.ins("e" + tail, K(1, 9, 4, 4))
    d.ann(r, K(1, 1, 2, 2), REWRITE)
    d.ins("f" + tail, K(1, 1, 2, 3))
    d.ins("g" + tail, K(1, 1, 2, 2))
    d.ins("|")


def _doc_routes():
    d = _Doc()
    for i in range(6):   # 42 segments and their splits: several pages
        _routes(d, "%02d" % i)
    d.settle()
    return d


def _collisions(per_size=4):
    """Pairs of distinct property sets over keys 1..8 x values 1..16, one to three keys each,
    whose signatures are equal -- found with the host function, as the device computes them;
    up to per_size pairs whose second set has one, two and three keys."""
    ids = [(k, v) for k in range(1, 9) for v in range(1, 17)]
    mix = {p: _sig([p]) for p in ids}
    seen, out = {}, []
    for n in (1, 2, 3):
        got = 0
        for keys in itertools.combinations(range(1, 9), n):
            for vals in itertools.product(range(1, 17), repeat=n):
                if got == per_size:
                    break
                s = tuple(zip(keys, vals))
                sg = sum(mix[p] for p in s) % 4096
                a = seen.get(sg)
                if a is None:
                    seen[sg] = s
                elif _sig(a) == _sig(s):   # (the whole sets, by the function itself)
                    out.append((a, s))
                    got += 1
                    del seen[sg]           # every set in one pair at most
    return out


def _doc_collisions(pairs):
    """Each colliding pair (A, B) on adjacent segments, B once more behind them: A | B must stay
    apart although their bits agree, B | B must merge."""
    d = _Doc()
    for a, b in pairs:
        d.ins("aaa", {f"k{k}": v for k, v in a})
        d.ins("bbb", {f"k{k}": v for k, v in b})
        d.ins("ccc", {f"k{k}": v for k, v in reversed(b)})
        d.ins("|")
    d.settle()
    return d


def _doc_bounds():
    """Old sets of 0, 1, 4, 5 and 8 keys under ops of 1, 2 and 3 keys with replaced, new and
    nulled keys and rewrites; each result beside a segment inserted with the same set in another
    key order (they must merge) and one that differs (it must not)."""
    d = _Doc()
    for s in (0, 1, 4, 5, 8):
        old = {f"k{k}": 10 + k for k in range(1, s + 1)}
        new_key = "k9" if s < 8 else "k8"   # (a ninth key would pass MT_KMAX)
        ops = [
            ({"k1": 3}, None),
            ({"k1": 4, new_key: 5}, None),
            ({"k1": None, "k2": 6, new_key: 7}, None),
            ({"k2": 8, new_key: None}, None),
            ({"k1": 3, "k2": 0}, REWRITE),
            ({new_key: 2}, REWRITE),
        ]
        for props, comb in ops:
            r = d.ins("xyz", dict(old) if old else None)
            d.ann(r, props, comb)
            # the same result, reached in one insert with its keys reversed
            if comb:   # rewrite: the op's own non-null pairs are what is left
                res = {k: v for k, v in props.items() if v is not None}
            else:
                res = dict(old)
                res.update(props)
                res = {k: v for k, v in res.items() if v is not None}
            if res:
                d.ins("uvw", dict(reversed(list(res.items()))))
                k0 = next(iter(res))
                d.ins("rst", dict(res, **{k0: 99}))
            d.ins("|")
    d.settle(64)
    return d


def _doc_payload_and_props():
    """Inserts whose text (at most eight units) and property record (at most four pairs) both
    come with the message, next to longer texts and larger records; equal neighbours merge."""
    d = _Doc()
    for i in range(10):
        for text in ("ab", "abcdefgh", "abcdefghi", "a" * 40):
            for n in (1, 2, 4, 5):
                p = {f"k{k}": k + i for k in range(1, n + 1)}
                d.ins(text, p)
                d.ins(text[::-1], dict(reversed(list(p.items()))))
        d.ins("|")
    d.settle(64)
    return d


def _doc_table():
    """A combining op (incr: the host's table) over sets with and without its key, then plain
    annotates over the results.  Real value ids: the interner is not synthetic."""
    d = _Doc()
    incr = {"name": "incr", "defaultValue": 1}
    for i in range(12):
        r1 = d.ins("abc", {"n": i % 3, "w": "x"})
        r2 = d.ins("def", {"w": "x"})
        d.ann((r1[0], r2[1]), {"n": 1}, incr)
        d.ann(r1, {"n": 7})
        d.ann(r2, {"n": 7})
        d.ins("|")
    d.settle()
    return d


def _prepare(oracle_lib, docs, synthetic=True):
    """The documents as one batch; the C restatement's checksums, statuses and full outputs."""
    from fluidframework_amd.wire import Batch, Interner
    b = Batch(Interner(synthetic=synthetic))
    for d in docs:
        b.add_doc(d.seed, d.msgs)
    a = b.arrays()
    osums, ost = oracle_lib.replay_batch(a, threads=2)
    assert (ost == 0).all(), ost
    exp = []
    for i in range(len(docs)):
        od = oracle_lib.OracleDoc.new(a["seed"][a["seed_off"][i]:a["seed_off"][i + 1]])
        assert od.apply_all(a["ops"][a["doc_off"][i]:a["doc_off"][i + 1]], a["text"], a["props"]) == 0
        o = od.outputs()
        exp.append(dict(o, segs=o["segs"].tolist(), deltas=None))
    for v in a.values():
        v.setflags(write=False)
    return dict(a=a, osums=osums, exp=exp, docs=len(docs))


def _texts(exp):
    """The live segments' texts of a document without removes, in order."""
    out, p = [], 0
    for r in exp["segs"]:
        out.append(exp["text"][p:p + r[0]])
        p += r[0]
    assert p == len(exp["text"])
    return out


@pytest.fixture(scope="module")
def hand(oracle_lib):
    """Twelve hand-built documents (a few hundred messages each), checked on the CPU first: the
    restatement itself must merge and keep apart what the cases say, so that a case cannot pass
    on a stream that never reaches it."""
    pairs = _collisions()
    assert len(pairs) >= 8, len(pairs)
    for a, b in pairs:
        assert a != b and sorted(a) != sorted(b) and _sig(a) == _sig(b)
    docs = [_doc_routes(), _doc_collisions(pairs), _doc_bounds(), _doc_payload_and_props()] * 3
    p = _prepare(oracle_lib, docs)
    t = _texts(p["exp"][0])
    whole = 0
    for i in range(6):
        tail = "%02d" % i
        # five routes, one segment -- or two, where a leaf block's edge falls between them
        # (scourNode merges inside one block)
        five = "".join(c + tail for c in "abcde")
        cut = [x for x in t if x and five.startswith(x)] + [x for x in t if x and five.endswith(x)]
        assert five in t or "".join(cut[:1] + cut[1:2]) == five, t
        whole += five in t
        assert "f" + tail in t and "g" + tail in t, t           # one value differs: apart
    assert whole >= 3, t
    t = _texts(p["exp"][1])
    assert t.count("aaa") == len(pairs) and t.count("bbbccc") == len(pairs), t
    t = _texts(p["exp"][2])
    assert t.count("xyzuvw") == 30 and t.count("rst") == 30, t   # 5 old sizes x 6 ops
    t = _texts(p["exp"][3])
    assert "abba" in t and "abcdefghhgfedcba" in t, t[:8]
    p["pairs"] = pairs
    return p


def _replay(p, **caps):
    from fluidframework_amd import MergeTreeBatch
    a = p["a"]
    mt = MergeTreeBatch(p["docs"], **caps)
    mt.load_initial_text(a["seed_off"], a["seed"])
    mt.apply_arrays(a)
    return mt


def _mismatches(mt, p):
    bad = []
    for i, exp in enumerate(p["exp"]):
        rows, leaves = mt.get_segments(i)
        got = dict(text=mt.get_text(i), length=mt.get_length(i), leaves=leaves, segs=rows,
                   seg_props=mt.get_all_segment_props(i), deltas=None, status=int(mt.status()[i]))
        errs = gu.compare_oracle(got, exp)
        if errs:
            bad.append((i, errs))
    return bad


def _check_rows(mt, docs):
    """Every row's bits equal mt_props_signature of the record its handle names; the raw
    read-out does not show them."""
    n_sets = 0
    for d in docs:
        sigs = mt.debug_props_sigs(d)
        props = mt.get_all_segment_props(d)
        assert len(sigs) == len(props)
        want = [0 if p is None else _sig(p) for p in props]
        bad = [(i, int(sigs[i]), want[i], props[i]) for i in range(len(props)) if int(sigs[i]) != want[i]]
        assert not bad, (d, bad[:4])
        n_sets += sum(1 for p in props if p)
        assert not (mt.debug_raw(d)[0][:, 7] & 0xFFF0).any()
    return n_sets


@gpu
@pytest.mark.parametrize("tier", TIERS)
def test_hand_built_sets(hand, tier):
    """Equal sets reached by different routes merge, sets differing in one value and distinct
    sets with colliding signatures stay apart, on both sides of every size bound of the annotate
    and insert paths: text, leaf partition, rows and property sets are the restatement's, the
    checksums (every message's delta hash) too, and every row's bits match its record."""
    mt = _replay(hand, **_tier_caps(tier))
    assert (mt.status() == 0).all(), mt.status()
    assert np.array_equal(mt.checksums(), hand["osums"])
    assert not _mismatches(mt, hand)
    if tier != "flat":
        assert all(mt.is_paged(d) for d in range(hand["docs"]))
    print(tier, mt.last_zamboni(), "rows with a set:", _check_rows(mt, range(hand["docs"])))


@gpu
@pytest.mark.parametrize("tier", ["bench_c3", "paged", "flat"])
def test_combining_op_table(oracle_lib, tier):
    """A combining op's table (never taken from the message's lanes, never on the annotate fast
    path) and the NaN it leaves (SEGF_NOMATCH beside the signature bits)."""
    p = _prepare(oracle_lib, [_doc_table()] * 8, synthetic=False)
    mt = _replay(p, **_tier_caps(tier))
    assert (mt.status() == 0).all(), mt.status()
    assert np.array_equal(mt.checksums(), p["osums"])
    assert not _mismatches(mt, p)
    assert _check_rows(mt, range(p["docs"])) > 0


@pytest.fixture(scope="module")
def stream(oracle_lib):
    """32 documents x 1500 messages of the C3 configuration, generated on the device once."""
    from fluidframework_amd import MergeTreeBatch
    cfg = _c3(1500)
    mt = MergeTreeBatch(32, delta_log_capacity=0, **_bench_c3_caps())
    batch = mt.generate(cfg)
    host = batch.download()
    seed_off, seed = mt.generated_seeds(cfg)
    a = dict(host, seed_off=seed_off, seed=seed)
    osums, ost = oracle_lib.replay_batch(a, threads=4)
    assert (ost == 0).all()
    assert np.array_equal(mt.checksums(), osums)
    n_gen = _check_rows(mt, range(32))   # the generator writes rows through the same engine
    assert n_gen > 0
    for v in a.values():
        v.setflags(write=False)
    return dict(a=a, osums=osums, docs=32)


@gpu
@pytest.mark.parametrize("tier", ["bench_c3", "paged", "grow"])
def test_invariant_after_generated_stream(stream, tier):
    """After 32 x 1500 generated C3 messages -- conversions from the flat tier, splits, in-place
    scours and packs, window scours, record compactions, and on `grow` hand-overs and growth
    copies -- every row's bits equal the signature of its record."""
    caps = _tier_caps(tier) if tier != "grow" else dict(FLAT, delta_log_capacity=0, **PARITY["grow"])
    mt = _replay(stream, **caps)
    assert (mt.status() == 0).all(), mt.status()
    assert np.array_equal(mt.checksums(), stream["osums"])
    n = _check_rows(mt, range(stream["docs"]))
    print(tier, "rows with a set:", n, mt.last_zamboni(), mt.last_paged_peaks())
    assert n > 1000
