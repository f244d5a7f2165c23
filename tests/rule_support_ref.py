"""References and shared inputs of the rule support tests (test_rule_support.py,
test_rule_support_gpu.py).  Not a test module.

A rule is a pair (X, Y) of ascending item tuples; a result is a triple (support, ante,
confidence).  A case is a dict with `records` (the (sid, spmf_line) pairs, dense sids),
`rules` and `expected`, the triples that follow from the way the DB is built (stated in each
generator), not from either reference:

  by_definition(records, rules)       brute.tsr_view, pure Python, any side length
  by_oracle(seq_off, tokens, rules)   oracle.rule_support, one rule at a time (sides of at
                                      most ORACLE_MAX_SIDE items: the oracle's buffers)

Run as a script (`python rule_support_ref.py`), this module scores child_cases() on the GPU
and prints {name: triples} as JSON: the child process of the hook test, started with
FSM_RS_PIVOT or FSM_RS_SLICE_TILES set.
"""
import json
import os
import re
import sys
from itertools import combinations

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "spark-fsm_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import brute  # noqa: E402

SUPPORT_SRC = os.path.join(ROOT, "spark-fsm_amd", "csrc", "rule_support.hip")
ORACLE_MAX_SIDE = 256
ABSENT = 99  # an item no random DB holds


def constants():
    """The geometry constants of rule_support.hip, read from its own constexpr lines."""
    with open(SUPPORT_SRC) as f:
        src = f.read()
    out = {}
    for name in ("kRsTile", "kRsBlock"):
        m = re.search(r"^constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src, re.M)
        assert m, "no constexpr int %s in rule_support.hip" % name
        out[name] = int(m.group(1))
    return out


def triple(sup, ante):
    """(support, ante, confidence) with the engine's confidence: support / ante, 0.0 at ante 0."""
    return (sup, ante, sup / ante if ante else 0.0)


# ---------------------------------------------------------------- references
def first_last(records):
    """Per sequence: ({item: first itemset index}, {item: last itemset index})."""
    out = []
    for s in brute.tsr_view(records):
        f, l = {}, {}
        for j, X in enumerate(s):
            for it in X:
                f.setdefault(it, j)
                l[it] = j
        out.append((f, l))
    return out


def by_definition(records, rules):
    fl = first_last(records)
    out = []
    for r in rules:
        X, Y = r[0], r[1]
        ante = sup = 0
        for f, l in fl:
            if all(x in f for x in X):
                ante += 1
                if all(y in l for y in Y) and max(f[x] for x in X) < min(l[y] for y in Y):
                    sup += 1
        out.append(triple(sup, ante))
    return out


def by_oracle(seq_off, tokens, rules):
    from oracle import oracle
    out = []
    for r in rules:
        assert len(r[0]) <= ORACLE_MAX_SIDE and len(r[1]) <= ORACLE_MAX_SIDE
        out.append(triple(*oracle.rule_support(seq_off, tokens, list(r[0]), list(r[1]))))
    return out


def oracle_allows(rules):
    return all(len(r[0]) <= ORACLE_MAX_SIDE and len(r[1]) <= ORACLE_MAX_SIDE for r in rules)


# ---------------------------------------------------------------- forms
def line(itemsets):
    return " ".join(" ".join(map(str, X)) + " -1" for X in itemsets) + " -2"


def records_of(rows):
    """rows: one list of itemsets per sequence -> (sid, line) records, sids 0..n-1."""
    return [(sid, line(r)) for sid, r in enumerate(rows)]


def tokens_of(records):
    """(sids, seq_off, tokens) of records."""
    toks, off = [], [0]
    for _sid, ln in records:
        toks.extend(int(t) for t in ln.split())
        off.append(len(toks))
    return (np.array([s for s, _ in records], np.int32), np.array(off, np.int64), np.array(toks, np.int64))


def items_of(records):
    return sorted({i for f, _l in first_last(records) for i in f})


def to_csr(rules):
    xo, xs, yo, ys = [0], [], [0], []
    for r in rules:
        xs.extend(r[0])
        ys.extend(r[1])
        xo.append(len(xs))
        yo.append(len(ys))
    return (np.array(xo, np.int64), np.array(xs, np.int32), np.array(yo, np.int64), np.array(ys, np.int32))


def triples_of(result):
    """Engine.rule_supports' three arrays -> a list of (support, ante, confidence)."""
    sup, ante, conf = result
    assert sup.dtype == np.int32 and ante.dtype == np.int32 and conf.dtype == np.float64
    assert sup.shape == ante.shape == conf.shape and sup.ndim == 1
    return list(zip(sup.tolist(), ante.tolist(), conf.tolist()))


# ---------------------------------------------------------------- hand cases
def hand_cases():
    """name -> case with stated answers (x = 1, y = 2, z = 3)."""
    x, y, z = 1, 2, 3
    one = ((x,), (y,))
    cases = {}
    cases["same_itemset_does_not_hold"] = {"records": records_of([[(x, y)]]), "rules": [one], "expected": [triple(0, 1)]}
    cases["x_before_y_holds"] = {"records": records_of([[(x,), (y,)]]), "rules": [one], "expected": [triple(1, 1)]}
    cases["y_only_before_x"] = {"records": records_of([[(y,), (x,)]]), "rules": [one], "expected": [triple(0, 1)]}
    # first_x = 0 < last_y = 1
    cases["x_at_0_and_2_y_at_1"] = {"records": records_of([[(x,), (y,), (x,)]]), "rules": [one, ((y,), (x,))],
                                    "expected": [triple(1, 1), triple(1, 1)]}
    # first_x = 1 < last_y = 2
    cases["y_at_0_and_2_x_at_1"] = {"records": records_of([[(y,), (x,), (y,)]]), "rules": [one, ((y,), (x,))],
                                    "expected": [triple(1, 1), triple(1, 1)]}
    # X = {1, 3}: row 0 has first_3 = 1 < last_2 = 2; row 1 has first_3 = 2 > last_2 = 1 (first_1 = 0 alone
    # would pass); row 2 lacks 3
    cases["later_first_of_x_decides"] = {"records": records_of([[(x,), (z,), (y,)], [(x,), (y,), (z,)], [(x,), (y,)]]),
                                         "rules": [((x, z), (y,)), one], "expected": [triple(1, 2), triple(3, 3)]}
    # Y = {2, 3}: row 0 has last_2 = 1 > first_1 = 0; row 1 has last_2 = 0 < first_1 = 1 (last_3 = 2 alone
    # would pass); row 2 lacks 3
    cases["earlier_last_of_y_decides"] = {"records": records_of([[(x,), (y,), (z,)], [(y,), (x,), (z,)], [(x,), (y,)]]),
                                          "rules": [((x,), (y, z)), ((x,), (z,))], "expected": [triple(1, 3), triple(2, 3)]}
    # row 0's 2 comes after its last -1: the row does not hold it
    cases["item_after_the_last_separator"] = {"records": [(0, "1 -1 2 -2"), (1, "1 -1 2 -1 -2")],
                                              "rules": [one, ((y,), (x,)), ((x, y), (z,))],
                                              "expected": [triple(1, 2), triple(0, 1), triple(0, 1)]}
    recs = records_of([[(10,), (20,)], [(10,), (20,)], [(20,), (10,)]])
    # values below, between and above the DB's
    cases["unknown_item_in_x"] = {"records": recs, "rules": [((5, 10), (20,)), ((10, 15), (20,)), ((10, 25), (20,)), ((25,), (10,))],
                                  "expected": [triple(0, 0)] * 4}
    cases["unknown_item_in_y"] = {"records": recs, "rules": [((10,), (5, 20)), ((10,), (15,)), ((10,), (20, 25)), ((10,), (20,))],
                                  "expected": [triple(0, 3)] * 3 + [triple(2, 3)]}
    cases["repeated_rule"] = {"records": recs, "rules": [((10,), (20,)), ((20,), (10,)), ((10,), (20,)), ((20,), (10,)), ((10,), (20,))],
                              "expected": [triple(2, 3), triple(1, 3)] * 2 + [triple(2, 3)]}
    return cases


# ---------------------------------------------------------------- random DBs
def all_rules(items):
    """Every rule X => Y over disjoint non-empty subsets of `items`."""
    out = []
    subsets = [c for r in range(1, len(items) + 1) for c in combinations(items, r)]
    for X in subsets:
        sx = set(X)
        out.extend((X, Y) for Y in subsets if not sx & set(Y))
    return out


_random = {}


def random_case(seed):
    """pattern_filter_ref.random_db(seed) with every rule over its items and ABSENT; expected
    is by_definition (the one reference of these DBs), computed once."""
    if seed not in _random:
        import pattern_filter_ref as fref
        recs, _sup = fref.random_db(seed)
        rules = all_rules(items_of(recs) + [ABSENT])
        _random[seed] = {"records": recs, "rules": rules, "expected": by_definition(recs, rules)}
    return _random[seed]


# what the 20 random DBs hold (asserted by the CPU and the GPU test, so that a generator
# change cannot empty a class silently)
RANDOM_TOTALS = {"rules": 10770, "ante0": 3754, "sup0": 4338, "partial": 2666, "full": 12}
RANDOM_MIN_PARTIAL = 11  # every DB has at least this many rules with 0 < support < ante


def classes(expected):
    c = {"rules": len(expected), "ante0": 0, "sup0": 0, "partial": 0, "full": 0}
    for sup, ante, _conf in expected:
        c["ante0" if ante == 0 else "sup0" if sup == 0 else "partial" if sup < ante else "full"] += 1
    return c


# ---------------------------------------------------------------- tile edges
PIVOT_PLACES = ("first", "middle", "last")
TILE_MODES = ("full", "lacks", "order")
Y_ITEM = 20


def tile_lengths(T):
    return (1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1)


def failing_rows(L):
    return sorted({0, L // 2, L - 1})


def tile_edge_case(L, place, mode, fail=0):
    """X has three items; its pivot 9 (the rare one) sits in exactly the L rows sid 0 .. L - 1,
    as X's first, middle or last item.  Those rows hold X in itemset 0 and y = 20 in itemset
    1, so they all hold the rule: (L, L) with mode "full".  Otherwise row `fail` differs:
      "lacks"  it lacks a non-pivot item of X                        -> (L - 1, L - 1)
      "order"  its y is in X's itemset (fail == 0) or before it      -> (L - 1, L)
    3 L filler rows (3 L + 1 with "lacks") hold X's other two items and y, not 9: the other
    items of X and y are in 4 L rows (or 4 L + 1), so 9 is the rare one."""
    X = {"first": (9, 11, 12), "middle": (1, 9, 12), "last": (1, 2, 9)}[place]
    others = tuple(i for i in X if i != 9)
    rows = [[X, (Y_ITEM,)] for _ in range(L)]
    exp = triple(L, L)
    if mode == "lacks":
        drop = others[fail % 2]
        rows[fail] = [tuple(i for i in X if i != drop), (Y_ITEM,)]
        exp = triple(L - 1, L - 1)
    elif mode == "order":
        rows[fail] = [tuple(sorted(X + (Y_ITEM,)))] if fail == 0 else [(Y_ITEM,), X]
        exp = triple(L - 1, L)
    else:
        assert mode == "full"
    rows += [[others, (Y_ITEM,)]] * (3 * L + (1 if mode == "lacks" else 0))
    return {"records": records_of(rows), "rules": [(X, (Y_ITEM,))], "expected": [exp], "pivot": 9, "pivot_rows": L,
            "others": others}


def tile_cases(T):
    out = {}
    for L in tile_lengths(T):
        for place in PIVOT_PLACES:
            out["L%d-%s-full" % (L, place)] = tile_edge_case(L, place, "full")
            for mode in ("lacks", "order"):
                for f in failing_rows(L):
                    out["L%d-%s-%s-%d" % (L, place, mode, f)] = tile_edge_case(L, place, mode, f)
    return out


def n_tile_cases(T):
    return sum(3 * (1 + 2 * len(failing_rows(L))) for L in tile_lengths(T))


def mixed_launch_case(T):
    """Pivot lists of 1, T + 1, 0 (dead) and 3 T entries interleaved in one call: item 10 is in
    row 0 only, item 11 in the next T + 1 rows, item 12 in the 3 T rows after them.  Every
    row has 1 beside its rare item in itemset 0 and 2 in itemset 1, except the last row of
    11 and the first and last row of 12, which have 2 first.  The first and the last rule
    are dead (an unknown X item), and a rule with an unknown Y sits between two live ones."""
    rows = [[(1, 10), (2,)]] + [[(1, 11), (2,)]] * T + [[(2,), (1, 11)]]
    rows += [[(2,), (1, 12)]] + [[(1, 12), (2,)]] * (3 * T - 2) + [[(2,), (1, 12)]]
    rules = [((99,), (1,)), ((10,), (2,)), ((11,), (2,)), ((10, 98), (2,)), ((12,), (2,)), ((11,), (97,)),
             ((10, 12), (2,)), ((1, 12), (2,)), ((98,), (2,))]
    exp = [triple(0, 0), triple(1, 1), triple(T, T + 1), triple(0, 0), triple(3 * T - 2, 3 * T), triple(0, T + 1),
           triple(0, 0), triple(3 * T - 2, 3 * T), triple(0, 0)]
    return {"records": records_of(rows), "rules": rules, "expected": exp, "lists": {10: 1, 11: T + 1, 12: 3 * T}}


# ---------------------------------------------------------------- row lengths
ROW_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1000)


def row_length_case(n):
    """Two rows of n distinct items (the even values 100, 102, ...): row 0 holds all of them
    in itemsets 0 and 1 (first 0, last 1: every rule over them holds), row 1 in itemset 0
    only (first = last: none holds).  Rule items sit at the row's lowest, middle and highest
    value: every ordered pair of these scores (1, 2).  The absent odd values 51 (below all),
    101 (between) and 100 + 2 n + 1 (above all) are known to the DB through three one-item
    rows each, so their lists are longer than the row items' and the row's middle item stays
    the pivot: an odd value in X is searched in the n-item rows and gives (0, 0), in Y (0, 2)."""
    S = [100 + 2 * k for k in range(n)]
    odd = (51, 101, 100 + 2 * n + 1)
    rows = [[tuple(S), tuple(S)], [tuple(S)]]
    for o in odd:
        rows += [[(o,)]] * 3
    lo, mid, hi = S[0], S[n // 2], S[-1]
    rules, exp = [], []
    for a in sorted({lo, mid, hi}):
        for b in sorted({lo, mid, hi}):
            if a != b:
                rules.append(((a,), (b,)))
                exp.append(triple(1, 2))
    if n >= 3:
        rules.append(((lo, hi), (mid,)))
        exp.append(triple(1, 2))
    for k, o in enumerate(odd):
        other = odd[(k + 1) % 3]
        rules += [(tuple(sorted((mid, o))), (other,)), ((mid,), (o,))]
        exp += [triple(0, 0), triple(0, 2)]
        if n >= 2:
            rules.append(((mid,), tuple(sorted((lo if mid != lo else hi, o)))))
            exp.append(triple(0, 2))
    return {"records": records_of(rows), "rules": rules, "expected": exp, "row_items": n}


# ---------------------------------------------------------------- long sides
def long_side_case(m=300):
    """X = 1 .. m and Y = 1001 .. 1000 + m (m = 300: past the miner's kMaxSide and past the
    oracle's buffers).  Row 0 holds X then Y; row 1 lacks X's last item; row 2 has the first
    item of Y only in itemset 0, before X in itemset 1; row 3 holds X only: (1, 3, 1/3)."""
    X, Y = tuple(range(1, m + 1)), tuple(range(1001, 1001 + m))
    rows = [[X, Y], [X[:-1], Y], [(Y[0],), X, Y[1:]], [X]]
    return {"records": records_of(rows), "rules": [(X, Y)], "expected": [triple(1, 3)]}


# ---------------------------------------------------------------- sid edges
SID_EDGE_SIZES = (129, 1025, 32769)
SID_EDGE_RULES = [((1,), (2,)), ((3,), (4,)), ((2,), (1,))]


def sid_edge_expected(edb):
    """The triples of SID_EDGE_RULES on edge_dbs.tsr_sid_edges(N), from how it is built: 1 -> 2
    holds at the m deciding sids, the only rows with 1: (m, m).  3 -> 4 holds at the m - 1
    rows <3, 4>, and 2 -> 1 nowhere; but the rows that hold one item alone hold 2 at sids
    = 0 and 3 at sids = 1 (mod 4), and a row with 3 (with 2) alone holds the whole
    antecedent of 3 -> 4 (of 2 -> 1): by the definition of ante these rows count, so
    3 -> 4 scores (m - 1, m - 1 + lone3) and 2 -> 1 scores (0, m + lone2), not (m - 1, m - 1)
    and (0, m)."""
    m = len(edb.deciding)
    taken = set(edb.deciding) | set(edb.second)
    lone = [s for s in range(len(edb)) if s not in taken]
    lone2, lone3 = sum(1 for s in lone if s % 4 == 0), sum(1 for s in lone if s % 4 == 1)
    assert lone2 > 0 and lone3 > 0
    return [triple(m, m), triple(m - 1, m - 1 + lone3), triple(0, m + lone2)]


# ---------------------------------------------------------------- the child of the hook test
def child_cases():
    """name -> case: the random DBs, the tile-edge DBs and the mixed launch."""
    import pattern_filter_ref as fref
    T = constants()["kRsTile"]
    out = {}
    for seed in range(fref.N_RANDOM):
        out["random%d" % seed] = random_case(seed)
    out.update(tile_cases(T))
    out["mixed-launch"] = mixed_launch_case(T)
    return out


def score_cases(eng, cases):
    import spark_fsm_amd as fsm
    res = {}
    for name, case in cases.items():
        db = eng.db_from_spmf(case["records"], fsm.MODE_TSR)
        try:
            res[name] = [list(t) for t in triples_of(eng.rule_supports(db, case["rules"]))]
        finally:
            db.free()
    return res


def _child():
    import spark_fsm_amd as fsm
    with fsm.Engine(0) as eng:
        print(json.dumps(score_cases(eng, child_cases())))


if __name__ == "__main__":
    _child()
