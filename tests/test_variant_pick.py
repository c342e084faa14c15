"""Which kernel variant a launch runs, and the dynamic LDS it is given, pinned without a GPU.

`mt_debug_pick` answers from the library's own variant table (csrc/mt_variants.h, mt_replay.hip
"kernel variants").  tests/golden/variant_picks.json holds, for every launch of `grid()`, the
name and LDS bytes that the hand-written launch ladders chose before the table replaced them
(recorded from those ladders, not from the table): a change that sent a launch to another
kernel, or sized its LDS differently from the kernel's own layout, fails here instead of
showing only in the benchmark.

The grid holds the launches a handle can make: a paged launch is packed only as a wide tight
tier (never narrow, never the big region's), and the big region's launches are wide.  The
library has no kernel for the other combinations and says so (test_unbuildable_launches)."""
import itertools
import json
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "variant_picks.json")
LDS_LIMIT = 160 * 1024

C3, C4 = (192, 192, 220), (224, 900, 1900)   # P_C3's and P_C4's compile-time (PP, PH, UT)


def _off_by_one(caps):
    out = [caps]
    for i in range(3):
        for d in (-1, 1):
            c = list(caps)
            c[i] += d
            out.append(tuple(c))
    return out


# (delta_log, ordinals): segment ordinals ride on the rich delta log
LOGS = [(0, 0), (1, 0), (1, 1)]
# (big, narrow, packed) of a paged replay launch
PAGED_KINDS = [(0, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 0)]
# PP at the MT_HM_PAGES threshold, and a layout above 64 KiB
PAGED_CAPS = _off_by_one(C3) + _off_by_one(C4) + [(511, 1024, 512), (512, 1024, 512), (256, 2048, 2048)]
FLAT_CAPS = [(192, 128, 96), (64, 64, 64)]   # the LDS tier's (S, B, H)
HBM_BLOCKS = [64, 1088, 16384]               # the HBM tier's B (the last: above 64 KiB)
GEN_WORDS = [4, 130]                         # 1 and 64 writers


def grid():
    """Every described launch, as keyword arguments of _native.debug_pick."""
    q = []
    for (dl, _), live, wpg, (S, B, H) in itertools.product(LOGS[:2], (0, 1), (1, 2), FLAT_CAPS):
        q.append(dict(launch="replay_lds", delta_log=dl, live=live, wpg=wpg, S=S, B=B, H=H))
    for (dl, _), live, B in itertools.product(LOGS[:2], (0, 1), HBM_BLOCKS):
        q.append(dict(launch="replay_hbm", delta_log=dl, live=live, wpg=1, B=B))
    for (dl, od), (big, narrow, packed), (PP, PH, UT) in itertools.product(LOGS, PAGED_KINDS, PAGED_CAPS):
        q.append(dict(launch="replay_paged", delta_log=dl, ordinals=od, big=big, narrow=narrow, packed=packed,
                      PP=PP, PH=PH, UT=UT))
    # the last tier's rounds: grow 1 (a capacity was raised), 2 (only the arenas can still grow)
    for (dl, od), big, grow, (PP, PH, UT) in itertools.product(LOGS, (0, 1), (1, 2), PAGED_CAPS[-3:]):
        q.append(dict(launch="replay_paged", delta_log=dl, ordinals=od, big=big, grow=grow, PP=PP, PH=PH, UT=UT))
    for (dl, _), live, (S, B, H), gw in itertools.product(LOGS[:2], (0, 1), FLAT_CAPS, GEN_WORDS):
        q.append(dict(launch="generate_lds", delta_log=dl, live=live, wpg=1, S=S, B=B, H=H, gen_words=gw))
    for (dl, _), B, gw in itertools.product(LOGS[:2], HBM_BLOCKS[:2], GEN_WORDS):
        q.append(dict(launch="generate_hbm", delta_log=dl, wpg=1, B=B, gen_words=gw))
    for (dl, _), narrow, (PP, PH, UT), gw in itertools.product(LOGS[:2], (0, 1), [C3] + PAGED_CAPS[-2:], GEN_WORDS):
        q.append(dict(launch="generate_paged", delta_log=dl, narrow=narrow, PP=PP, PH=PH, UT=UT, gen_words=gw))
    for (dl, od), big, (PP, PH, UT) in itertools.product(LOGS, (0, 1), [(64, 256, 256)] + PAGED_CAPS[-2:]):
        q.append(dict(launch="load_convert", delta_log=dl, ordinals=od, big=big, PP=PP, PH=PH, UT=UT))
    for (dl, _), narrow, (PP, PH, UT) in itertools.product(LOGS[:2], (0, 1), [C3, C4] + PAGED_CAPS[-2:]):
        q.append(dict(launch="occupancy", delta_log=dl, narrow=narrow, PP=PP, PH=PH, UT=UT))
    return q


@pytest.fixture(scope="module")
def native():
    from fluidframework_amd import _native, build
    build.build()
    return _native


def test_picks_equal_the_recorded_ladders(native):
    rows = json.load(open(FIXTURE))
    queries = grid()
    assert [r["query"] for r in rows] == queries, "the fixture is not this grid's"
    got = [native.debug_pick(**q) for q in queries]
    bad = [(q, g, (r["name"], r["lds"])) for q, g, r in zip(queries, got, rows) if g != (r["name"], r["lds"])]
    assert not bad, f"{len(bad)} of {len(rows)} picks differ, first: {bad[:3]}"
    # no pick exceeds the LDS a launch may stage where the recorded one did not
    assert not [q for q, g, r in zip(queries, got, rows) if g[1] > LDS_LIMIT >= r["lds"]]


def test_every_variant_is_picked(native):
    from fluidframework_amd import build
    text = open(os.path.join(REPO, "fluidframework_amd", "csrc", "mt_variants.h")).read()
    names = set(re.findall(r"^\s*X\((\w+),", text, flags=re.M))
    assert len(names) == 31 and names == {name for name, _ in build.variants()}
    picked = {native.debug_pick(**q)[0] for q in grid()}
    assert picked == names, sorted(names ^ picked)


@pytest.mark.parametrize("kind", [dict(narrow=1, packed=1), dict(big=1, narrow=1), dict(big=1, packed=1)])
def test_unbuildable_launches(native, kind):
    """No handle makes these launches and no kernel is compiled for them: an error, not a
    neighbouring kernel with another LDS layout."""
    assert native.debug_pick(launch="replay_paged", PP=256, PH=2048, UT=2048, **kind) is None


@pytest.mark.gpu
def test_gpu_two_handles_keep_their_lds_limit(native, oracle_lib):
    """A kernel's dynamic-LDS limit above 64 KiB belongs to the process, not to a handle.  Two
    paged handles whose layouts both pass 64 KiB, the larger created first, share the last
    tier's kernel: creating the smaller one must not lower the limit under the larger one.
    Two documents of the reference's 60-message streams replay on the larger handle after the
    smaller one exists, then on the smaller; both equal the oracle.
    (Before the limit was kept per kernel and never lowered, the second handle's creation set
    the smaller value under the first.  Run once on that library, the case passed as well: the
    HIP runtime of ROCm 7.2 on the MI355X did not reject the larger launch.  The test pins the
    rule the code now follows, not a failure that was observed.)"""
    import numpy as np

    import golden_util as gu
    from fluidframework_amd import MergeTreeBatch
    fx = gu.load("ref_small")
    docs = fx["docs"][:2]
    a = gu.encode_docs(fx, gu.interner_for(fx), docs)
    caps = [dict(page_capacity=256, page_heap_capacity=3072, unsettled_capacity=3072),
            dict(page_capacity=256, page_heap_capacity=2048, unsettled_capacity=2048)]
    picks = [native.debug_pick(launch="replay_paged", PP=c["page_capacity"], PH=c["page_heap_capacity"],
                               UT=c["unsettled_capacity"]) for c in caps]
    assert picks[0][0] == picks[1][0] == "P_FULL"
    assert 64 * 1024 < picks[1][1] < picks[0][1] < LDS_LIMIT
    # LDS tier off: every document takes the paged launch
    larger, smaller = [MergeTreeBatch(len(docs), lds_seg_capacity=-1, delta_log_capacity=0, **c) for c in caps]
    osums, ost = oracle_lib.replay_batch(a, threads=2)
    assert (ost == 0).all()
    for mt in (larger, smaller):
        mt.load_initial_text(a["seed_off"], a["seed"])
        mt.apply_arrays(a)
        assert (mt.status() == 0).all() and all(mt.is_paged(i) for i in range(len(docs)))
        sums = mt.checksums()
        for f in ("length", "text_hash", "props_hash", "delta_hash", "n_segments"):
            assert np.array_equal(sums[f], osums[f]), f
