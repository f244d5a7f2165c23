"""Reference and shared inputs of the pattern sid-list tests (test_pattern_sids.py,
test_pattern_sids_gpu.py).  Not a test module.

The reference is the definition: the sorted sequence ids whose merged sequence
(brute.spade_eid_view) contains the pattern (brute._contains).  The generators and the pattern
forms are pattern_support_ref's; the cases added here state their lists from the way the DB is
built.

Run as a script (`python pattern_sids_ref.py`), this module asks for the lists of
child_cases() on the GPU and prints {name: [off, sid]} as JSON: the child process of the hook
test, started with FSM_PS_PIVOT, FSM_PS_SLICE_TILES or FSM_PS_SLICE_SIDS set.
"""
import json
import os
import random
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import pattern_support_ref as ref  # noqa: E402  (puts the repository and the package on sys.path)
from oracle import brute  # noqa: E402

I32_MAX = (1 << 31) - 1


def constants():
    """pattern_support_ref.constants() and the staging size of the write, from the source."""
    out = ref.constants()
    with open(ref.SUPPORT_SRC) as f:
        m = re.search(r"^constexpr\s+uint64_t\s+kPsSliceSids\s*=\s*(\d+)\s*;", f.read(), re.M)
    assert m, "no constexpr uint64_t kPsSliceSids in pattern_support.hip"
    out["kPsSliceSids"] = int(m.group(1))
    return out


# ---------------------------------------------------------------- the reference
def by_definition(records, patterns):
    """One ascending sid list per pattern."""
    view = brute.spade_eid_view(records)
    out = []
    for p in patterns:
        fp = [frozenset(X) for X in p]
        out.append(sorted(sid for sid, seq in view.items() if brute._contains(seq, fp)))
    return out


def split(off, sid):
    """(off, sid) arrays -> list of lists, with the invariants every result has."""
    off, sid = np.asarray(off), np.asarray(sid)
    assert off.dtype == np.int64 and sid.dtype == np.int32
    assert off[0] == 0 and off[-1] == len(sid) and (np.diff(off) >= 0).all()
    o, s = off.tolist(), sid.tolist()
    lists = [s[o[p]:o[p + 1]] for p in range(len(o) - 1)]
    for L in lists:
        assert all(a < b for a, b in zip(L, L[1:])), "a list is not strictly ascending"
    return lists


# ---------------------------------------------------------------- tile edges
def tile_edge_lists(case):
    """What tile_edge_case's docstring says: every row of the pivot holds the pattern except,
    without `full` (expected = L - 1), the last of them.  Rows are sids."""
    pivot = str(case["pivot"])
    rows = [sid for sid, ln in case["records"] if pivot in ln.split()]
    assert len(rows) == case["pivot_rows"]
    return [rows if case["expected"][0] == len(rows) else rows[:-1]]


LANE_SHAPES = ("lane0", "lane63", "even", "none")


def lane_case(shape, T):
    """3 T rows hold the pivot 9 (sids 10, 13, 16, ...), so its ordered list fills three
    tiles; all rows of the first and the last tile hold <(9)(1)>, and of the middle tile
    only the lanes `shape` names (the others hold 1 before 9).  Eight more rows hold 1 alone,
    so 9 is the pivot.  <(9)> lists every pivot row."""
    keep = {"lane0": {0}, "lane63": {T - 1}, "even": set(range(0, T, 2)), "none": set()}[shape]
    recs, exp = [], []
    for k in range(3 * T):
        sid = 10 + 3 * k
        hit = not T <= k < 2 * T or (k - T) in keep
        recs.append((sid, ref.line([(9,), (1,)] if hit else [(1,), (9,)])))
        if hit:
            exp.append(sid)
    recs += [(5000 + k, ref.line([(1,)])) for k in range(8)]
    return {"records": recs, "patterns": [((9,), (1,)), ((9,),)], "expected": [exp, [10 + 3 * k for k in range(3 * T)]]}


def dead_tiles_case(T):
    """Patterns without survivors that own tiles (their pivot has rows, no row holds them),
    first, between two patterns with survivors, and last; `all_dead` is a call of only such."""
    recs = [(2 * k + 1, ref.line([(9,), (1,)])) for k in range(T + 6)]
    recs += [(1000 + k, ref.line([(1,)])) for k in range(8)]
    recs += [(2000 + k, ref.line([(2,), (3,)])) for k in range(5)]
    nine, twos = [2 * k + 1 for k in range(T + 6)], [2000 + k for k in range(5)]
    pats = [((1,), (9,)), ((9,), (1,)), ((3,), (2,)), ((2,), (3,)), ((1, 9),)]
    return {"records": recs, "patterns": pats, "expected": [[], nine, [], twos, []],
            "all_dead": [((1,), (9,)), ((3,), (2,)), ((1, 9),), ((9,), (9,))]}


def order_case(T, seed=11):
    """4 T + 1 pivot rows given in shuffled sid order (the host flatten sorts them)."""
    sids = random.Random(seed).sample(range(1, 100000), 4 * T + 1 + 8)
    recs = [(s, ref.line([(9,), (1,)] if k % 3 else [(1,), (9,)])) for k, s in enumerate(sids[:4 * T + 1])]
    recs += [(s, ref.line([(1,)])) for s in sids[4 * T + 1:]]
    assert [s for s, _ in recs] != sorted(s for s, _ in recs)
    return {"records": recs, "patterns": [((9,), (1,)), ((9,),), ((1,), (9,)), ((1,),)]}


# ---------------------------------------------------------------- ids are not row indexes
def sid_case():
    """Sids 3, 9, 10, 1000, 2^31 - 1.  Sid 9 has two records of which only the merged row
    holds <(1)(2)>; sid 1000's record is "-2" alone, between two sids that hold the pattern;
    sid 3 holds 2 before 1.  `text`: the records in descending sid order; `tokens`: the same
    DB, ascending, sid 9's records as the one they merge to."""
    text = [(I32_MAX, "1 -1 2 -1 -2"), (1000, "-2"), (10, "1 -1 2 -1 -2"), (9, "3 -1 2 -1 -2"), (9, "1 -1 -2"),
            (3, "2 -1 1 -1 -2")]
    merged = [(3, "2 -1 1 -1 -2"), (9, "1 3 -1 2 -1 -2"), (10, "1 -1 2 -1 -2"), (1000, "-2"), (I32_MAX, "1 -1 2 -1 -2")]
    pats = [((1,), (2,)), ((2,),), ((1, 3),), ((3,), (2,)), ((2,), (1,))]
    exp = [[9, 10, I32_MAX], [3, 9, 10, I32_MAX], [9], [9], [3]]
    return {"text": text, "merged": merged, "tokens": ref.tokens_of(merged), "patterns": pats, "expected": exp}


# ---------------------------------------------------------------- the child of the hook test
def child_cases():
    """pattern_support_ref.child_cases(): the random DBs with every pattern of up to 3 items,
    and the tile-edge DBs."""
    return ref.child_cases()


def list_cases(eng, cases):
    import spark_fsm_amd as fsm
    res = {}
    for name, (recs, pats) in cases.items():
        db = eng.db_from_spmf(recs, fsm.MODE_SPADE)
        try:
            off, sid = eng.pattern_sids(db, pats)
            res[name] = [off.tolist(), sid.tolist()]
        finally:
            db.free()
    return res


def _child():
    import spark_fsm_amd as fsm
    with fsm.Engine(0) as eng:
        print(json.dumps(list_cases(eng, child_cases())))


if __name__ == "__main__":
    _child()
