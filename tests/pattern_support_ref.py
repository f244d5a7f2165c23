"""References and shared inputs of the pattern support tests (test_pattern_support.py,
test_pattern_support_gpu.py).  Not a test module.

A pattern is a tuple of ascending item tuples; a case is a dict with `records` (the
(sid, spmf_line) pairs), `patterns` and `expected`, the counts that follow from the way the
DB is built (stated in each generator), not from either reference:

  by_definition(records, patterns)       brute.spade_eid_view + brute._contains
  by_oracle(seq_off, tokens, patterns)   oracle.pattern_support, one pattern at a time

Run as a script (`python pattern_support_ref.py`), this module counts child_cases() on the
GPU and prints {name: counts} as JSON: the child process of the forced-pivot test, started
with FSM_PS_PIVOT (or FSM_PS_SLICE_TILES) set.
"""
import json
import os
import re
import sys
from itertools import combinations, product

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "spark-fsm_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import brute  # noqa: E402

SUPPORT_SRC = os.path.join(ROOT, "spark-fsm_amd", "csrc", "pattern_support.hip")


def constants():
    """The geometry constants of pattern_support.hip, read from its own constexpr lines."""
    with open(SUPPORT_SRC) as f:
        src = f.read()
    out = {}
    for name in ("kPsTile", "kPsBlock", "kPsSetRegs"):
        m = re.search(r"^constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src, re.M)
        assert m, "no constexpr int %s in pattern_support.hip" % name
        out[name] = int(m.group(1))
    return out


# ---------------------------------------------------------------- references
def by_definition(records, patterns):
    seqs = list(brute.spade_eid_view(records).values())
    out = []
    for p in patterns:
        fp = [frozenset(X) for X in p]
        out.append(sum(1 for s in seqs if brute._contains(s, fp)))
    return out


def by_oracle(seq_off, tokens, patterns):
    from oracle import oracle
    return [int(oracle.pattern_support(seq_off, tokens, p)) for p in patterns]


# ---------------------------------------------------------------- forms
def line(itemsets):
    return " ".join(" ".join(map(str, X)) + " -1" for X in itemsets) + " -2"


def records_of(rows):
    """rows: one list of itemsets per sequence -> (sid, line) records, sids 0..n-1."""
    return [(sid, line(r)) for sid, r in enumerate(rows)]


def tokens_of(records):
    """(sids, seq_off, tokens) of records without <t> tokens."""
    toks, off = [], [0]
    for _sid, ln in records:
        toks.extend(int(t) for t in ln.split())
        off.append(len(toks))
    return (np.array([s for s, _ in records], np.int32), np.array(off, np.int64), np.array(toks, np.int64))


def items_of(records):
    return sorted({i for s in brute.spade_eid_view(records).values() for X in s for i in X})


_COMPOSITIONS = {1: [(1,)], 2: [(1, 1), (2,)], 3: [(1, 1, 1), (1, 2), (2, 1), (3,)]}


def small_patterns(items, max_items=3):
    """Every pattern of at most max_items items over `items`."""
    out = []
    for m in range(1, max_items + 1):
        for comp in _COMPOSITIONS[m]:
            out.extend(product(*[list(combinations(items, k)) for k in comp]))
    return out


def to_csr(patterns, support=None):
    po, so, it = [0], [0], []
    for sets in patterns:
        for X in sets:
            it.extend(X)
            so.append(len(it))
        po.append(len(so) - 1)
    return (None if support is None else np.asarray(support, np.int32), np.array(po, np.int64),
            np.array(so, np.int64), np.array(it, np.int32))


def csr_patterns(csr):
    _sup, po, so, it = (None if a is None else np.asarray(a).tolist() for a in csr)
    return [tuple(tuple(it[so[s]:so[s + 1]]) for s in range(po[p], po[p + 1])) for p in range(len(po) - 1)]


# ---------------------------------------------------------------- hand cases
def hand_cases():
    """name -> case with stated answers."""
    a, b, c = 1, 2, 3
    cases = {}
    # <(a b)> needs both at one eid, <(a)(b)> a strictly before b
    recs = records_of([[(a, b)], [(a,), (b,)], [(b,), (a,)], [(a, b), (b,)], [(c,)]])
    cases["itemset_vs_sequence"] = {"records": recs, "patterns": [((a, b),), ((a,), (b,)), ((b,), (a,)), ((a, b), (b,))],
                                    "expected": [2, 2, 1, 1]}
    # <a -> a> needs two occurrences
    recs = records_of([[(a,)], [(a,), (a,)], [(a,), (b,), (a,)], [(a, b)], [(b,), (a,)]])
    cases["repeat_needs_two"] = {"records": recs, "patterns": [((a,), (a,)), ((a,), (a,), (a,)), ((a,),)],
                                 "expected": [2, 0, 5]}
    # explicit timestamps with ties: the two itemsets at <5> are one eid
    recs = [(0, "<5> 1 -1 <5> 2 -1 <9> 3 -1 -2"), (1, "<5> 1 -1 <6> 2 -1 <6> 3 -1 -2"), (2, "<2> 2 -1 <1> 1 -1 -2")]
    cases["timestamp_ties"] = {"records": recs,
                               "patterns": [((a, b),), ((a,), (b,)), ((b, c),), ((a, b), (c,)), ((b,), (c,)), ((a,), (c,))],
                               "expected": [1, 2, 1, 1, 1, 2]}
    # two records of one sid are one row, counted once; the second record's eids restart at 1
    recs = [(7, line([(a,), (b,)])), (7, line([(c,), (a,)])), (8, line([(a,)]))]
    cases["one_sid_two_records"] = {"records": recs,
                                    "patterns": [((a,),), ((a, c),), ((a,), (a,)), ((c,), (b,)), ((a, c), (a, b)), ((b,), (c,))],
                                    "expected": [2, 1, 1, 1, 1, 0]}
    # unknown items (below, between, above the DB's), more itemsets than the DB's 64 eids
    recs = records_of([[(10,), (20,)], [(10, 20)], [(20,), (10,)]])
    cases["cannot_match"] = {"records": recs,
                             "patterns": [((5,),), ((15,),), ((25,),), ((10,), (15,)), ((10, 25),), ((10,),) * 65,
                                          ((10,), (20,), (10,)), ((10,), (20,))],
                             "expected": [0, 0, 0, 0, 0, 0, 0, 1]}
    # duplicates are separate entries with equal counts
    recs = records_of([[(a,), (b,)], [(a,), (b,)], [(b,)]])
    cases["duplicates"] = {"records": recs, "patterns": [((a,), (b,)), ((b,),), ((a,), (b,)), ((b,),), ((a,), (b,))],
                           "expected": [2, 3, 2, 3, 2]}
    return cases


# ---------------------------------------------------------------- tile edges
PIVOT_PLACES = ("first", "middle", "last", "inset")


def tile_edge_case(L, place, full):
    """The rare item 9 (the pivot: the shortest list) occurs in exactly L rows; every
    other item of the pattern occurs in at least L + 8 rows.  All of 9's rows hold the pattern
    except, without `full`, the LAST of them, which holds the pattern's itemsets in
    reverse order (all items occur once per row, so it does not contain the pattern):
    the answer is L with `full`, L - 1 without."""
    pat = {"first": ((9,), (1,), (2,)), "middle": ((1,), (9,), (2,)), "last": ((1,), (2,), (9,)),
           "inset": ((1,), (8, 9, 10))}[place]
    others = tuple((i,) for X in pat for i in X if i != 9)
    rows = []
    for k in range(L):
        rows.append(list(pat))
        if k % 16 == 0:  # rows without the pivot in between
            rows.append(list(others))
    # at least 8 such rows, two of them after the last pivot row
    rows += [list(others)] * max(2, 8 - sum(1 for r in rows if r == list(others)))
    last = max(k for k, r in enumerate(rows) if r == list(pat))
    if not full:
        rows[last] = list(reversed(pat))
    return {"records": records_of(rows), "patterns": [pat], "expected": [L if full else L - 1], "pivot": 9,
            "pivot_rows": L}


def shared_launch_case(T):
    """Pivot lists of 1, 2 and 4T + 1 rows in one launch: item 10 occurs in row 0 only,
    item 11 in rows 1 and 2, item 12 in the 4T + 1 rows after them; every row has 1
    before 2 except row 2."""
    rows = [[(10,), (1,), (2,)], [(11,), (1,), (2,)], [(11,), (2,), (1,)]] + [[(12,), (1,), (2,)]] * (4 * T + 1)
    pats = [((10,), (1,)), ((11,), (1,), (2,)), ((12,), (2,)), ((1,), (2,)), ((11,), (2,)), ((10,), (2,), (1,))]
    return {"records": records_of(rows), "patterns": pats, "expected": [1, 1, 4 * T + 1, 4 * T + 3, 2, 0]}


def tile_lengths(T):
    return (T - 1, T, T + 1, 4 * T - 1, 4 * T, 4 * T + 1)


def tile_cases(T):
    out = {}
    for L in tile_lengths(T):
        for place in PIVOT_PLACES:
            for full in (True, False):
                out["L%d-%s-%s" % (L, place, "full" if full else "short")] = tile_edge_case(L, place, full)
    out["shared-launch"] = shared_launch_case(T)
    return out


# ---------------------------------------------------------------- row lengths
ROW_LENGTHS = (1, 2, 63, 64, 65, 1000)
SEARCHED = ("first", "last", "below", "between", "above")


def row_length_case(n):
    """Two equal rows of n distinct items (the even values 100, 102, ...), each holding
    all of them in two itemsets (every item at eids 0 and 1), and for every searched
    value three one-item filler rows, so a searched value has a longer list than the
    row's other items.  The partner of a searched value x is the row's middle item
    (n >= 3: the shortest list, so it is the pivot and x is searched in the n-item row),
    else the row's other or only item.  The patterns are <(partner x)> and <(partner)(x)>:
    both count 2 when x is in the row, 0 when it is not (below = 50, between = 101,
    above = 100 + 2n + 1; known items, through their filler rows)."""
    S = [100 + 2 * k for k in range(n)]
    absent = {"below": 50, "between": 101, "above": 100 + 2 * n + 1}
    searched = {"first": S[0], "last": S[-1]}
    searched.update(absent)
    rows = [[tuple(S), tuple(S)], [tuple(S), tuple(S)]]
    for x in sorted(set(searched.values())):
        rows += [[(x,)]] * 3
    pats, exp, names = [], [], []
    for where in SEARCHED:
        x = searched[where]
        if n >= 3:
            pivot = S[n // 2]
        else:
            pivot = S[-1] if x == S[0] else S[0]
        present = x in S
        if x == pivot:  # n == 1: the row's only item is both
            pats += [((x,),), ((x,), (x,))]
            exp += [5, 2]  # (the filler rows hold it once, at one eid)
        else:
            pats += [(tuple(sorted((pivot, x))),), ((pivot,), (x,))]
            exp += [2 if present else 0] * 2
        names += [where] * 2
    return {"records": records_of(rows), "patterns": pats, "expected": exp, "names": names, "row_items": n}


# ---------------------------------------------------------------- mask widths
MASK_WIDTHS = (1, 2, 16, 64, 128)


def mask_width_case(W):
    """Two equal sequences of exactly 64 W itemsets (W mask words), one unique noise item
    per eid.  Triple k = (e1, e2, e3) plants items 10k+1, 10k+2, 10k+3 at those eids only:
    <(10k+1)(10k+2)(10k+3)> counts 2; its twin 10k+5, 10k+6, 10k+7 sits at (e1, e2, e3 - 1),
    where the last two share an eid: the twin counts 0.  Items 5 and 6 share only the eid
    64 (W - 1) + 5 (5 is also at eid 0, 6 at eid 1): their AND is non-zero in the last word
    only; item 7 sits at the last eid.  A 12-item itemset follows (below)."""
    E = 64 * W
    triples = [t for t in ((62, 63, 64), (63, 64, 65), (E - 3, E - 2, E - 1)) if t[2] < E]
    sets = [[100000 + e] for e in range(E)]
    pats, exp = [], []
    for k, (e1, e2, e3) in enumerate(triples, start=1):
        for base, eids in ((10 * k, (e1, e2, e3)), (10 * k + 4, (e1, e2, e3 - 1))):
            for j, e in enumerate(eids, start=1):
                sets[e].append(base + j)
            pats.append(((base + 1,), (base + 2,), (base + 3,)))
            exp.append(2 if base == 10 * k else 0)
    last_word = 64 * (W - 1) + 5
    sets[0].append(5)
    sets[1].append(6)
    sets[last_word] += [5, 6]
    sets[E - 1].append(7)
    pats += [((5, 6),), ((5, 6), (7,)), ((5,), (6,), (5, 6)), ((7,), (5, 6)), ((5, 6), (5, 6))]
    exp += [2, 2, 2, 0, 0]
    # an itemset of 12 items (more than kPsSetRegs): all of 201..212 meet only at eid
    # 64 (W - 1) + 7; 201..211 also meet at eid 3, where 212 is missing (it sits at eid 4)
    big, meet = tuple(range(201, 213)), 64 * (W - 1) + 7
    sets[meet] += list(big)
    sets[3] += list(big[:-1])
    sets[4].append(big[-1])
    pats += [(big,), (big[:-1],), (big, (7,)), ((7,), big), (big[:-1], big), (big, big), ((212,), big[:-1])]
    exp += [2, 2, 2, 0, 2, 0, 2]
    row = [tuple(sorted(s)) for s in sets]
    return {"records": records_of([row, row]), "patterns": pats, "expected": exp, "W": W, "eids": E,
            "triples": triples}


# ---------------------------------------------------------------- long pattern
def long_pattern_case(length=3000):
    """One pattern of `length` single-item itemsets: 40 values in rotation, then the value
    99 once, as its last item.  Three rows are exactly the pattern; two rows are the
    pattern without its last itemset.  The pattern counts 3, its prefix of length - 1
    counts 5."""
    body = tuple(((k % 40) + 1,) for k in range(length - 1))
    pat = body + ((99,),)
    rows = [list(pat)] * 3 + [list(body)] * 2
    return {"records": records_of(rows), "patterns": [pat, body], "expected": [3, 5]}


# ---------------------------------------------------------------- the child of the forced-pivot test
def child_cases():
    """name -> (records, patterns): the random DBs of the round trip with every pattern of up
    to 3 items over their items, and the tile-edge DBs."""
    import pattern_filter_ref as fref
    out = {}
    for seed in range(fref.N_RANDOM):
        recs, _sup = fref.random_db(seed)
        out["random%d" % seed] = (recs, small_patterns(items_of(recs)))
    for name, case in tile_cases(constants()["kPsTile"]).items():
        out[name] = (case["records"], case["patterns"])
    return out


def count_cases(eng, cases):
    import spark_fsm_amd as fsm
    res = {}
    for name, (recs, pats) in cases.items():
        db = eng.db_from_spmf(recs, fsm.MODE_SPADE)
        try:
            res[name] = eng.pattern_supports(db, pats).tolist()
        finally:
            db.free()
    return res


def _child():
    import spark_fsm_amd as fsm
    with fsm.Engine(0) as eng:
        print(json.dumps(count_cases(eng, child_cases())))


if __name__ == "__main__":
    _child()
