"""The reference and the shared inputs of the rule prediction tests (test_rule_predict.py,
test_rule_predict_gpu.py).  Not a test module.

A scored rule is a tuple (X, Y, support, confidence) of two ascending item tuples and the two
scores; a result is one list of (item, rule index) pairs per row.  A case is a dict with
`records` (the (sid, spmf_line) pairs, dense sids), `rules`, `topn` and `expected`, the lists
that follow from the way the DB is built (stated in each generator), not from the reference:

  by_definition(records, rules, topn)   pure Python on rule_support_ref.first_last

Run as a script (`python rule_predict_ref.py`), this module predicts child_cases() on the GPU
and prints {"results": {name: lists}, "launches": {name: k_rp_match launches}} as JSON: the
child process of the hook test, started with FSM_RP_SLICE_ROWS or FSM_RP_PIVOT set.
"""
import json
import os
import random
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "spark-fsm_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import rule_support_ref as sref  # noqa: E402

PREDICT_SRC = os.path.join(ROOT, "spark-fsm_amd", "csrc", "rule_predict.hip")
ALL = 10 ** 6  # a topn above every list length of the cases here
TOPN_MAX = 2 ** 31 - 1


def constants():
    """The geometry constants of rule_predict.hip, read from its own constexpr lines."""
    with open(PREDICT_SRC) as f:
        src = f.read()
    out = {}
    for name in ("kRpTile", "kRpBlock", "kRpRecordBytes"):
        m = re.search(r"^constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src, re.M)
        assert m, "no constexpr int %s in rule_predict.hip" % name
        out[name] = int(m.group(1))
    return out


# ---------------------------------------------------------------- the reference
def rank_order(rules):
    """The rule indexes in rank order: confidence descending, support descending, index ascending."""
    return sorted(range(len(rules)), key=lambda r: (-rules[r][3], -rules[r][2], r))


def open_ranks(records, rules):
    """Per row: {item: ascending ranks of the rules under which the item is open in the row}."""
    order = rank_order(rules)
    rank = {r: k for k, r in enumerate(order)}
    out = []
    for f, l in sref.first_last(records):
        opened = {}
        for r, rule in enumerate(rules):
            X, Y = rule[0], rule[1]
            if all(x in f for x in X):  # r fires
                fx = max(f[x] for x in X)
                for y in Y:
                    if y not in l or l[y] <= fx:  # y has not occurred strictly after X was complete
                        opened.setdefault(y, []).append(rank[r])
        out.append({y: sorted(rk) for y, rk in opened.items()})
    return out, order


def by_definition(records, rules, topn):
    assert topn >= 1
    rows, order = open_ranks(records, rules)
    out = []
    for opened in rows:
        lst = sorted((rk[0], y) for y, rk in opened.items())  # by the best rule's rank, then by item value
        out.append([(y, order[rk]) for rk, y in lst[:topn]])
    return out


def lists_of(result):
    """Engine.rule_predictions' three arrays -> one list of (item, rule index) pairs per row."""
    import numpy as np
    off, item, rule = result
    assert off.dtype == np.int64 and item.dtype == np.int32 and rule.dtype == np.int32
    assert off.ndim == item.ndim == rule.ndim == 1 and item.shape == rule.shape
    off = off.tolist()
    assert off[0] == 0 and off[-1] == len(item) and all(a <= b for a, b in zip(off, off[1:]))
    pairs = list(zip(item.tolist(), rule.tolist()))
    return [pairs[off[s]:off[s + 1]] for s in range(len(off) - 1)]


def scored(records, rules):
    """(X, Y) rules with the scores rule_support_ref.by_definition gives them on the records."""
    return [(r[0], r[1], sup, conf) for r, (sup, _ante, conf) in zip(rules, sref.by_definition(records, rules))]


def case(rows, rules, expected, topn=10):
    return {"records": sref.records_of(rows), "rules": rules, "topn": topn, "expected": expected}


# ---------------------------------------------------------------- hand cases
def hand_cases():
    """name -> case with stated answers (x = 1, y = 2, z = 3)."""
    x, y, z = 1, 2, 3
    one = [((x,), (y,), 1, 1.0)]
    c = {}
    # --- which items are open
    c["open_y_absent"] = case([[(x,)]], one, [[(y, 0)]])
    c["open_y_only_before_x"] = case([[(y,), (x,)]], one, [[(y, 0)]])
    c["open_last_y_equals_fx"] = case([[(x, y)]], one, [[(y, 0)]])  # the same itemset: not strictly after
    c["open_not_y_after_x"] = case([[(x,), (y,)]], one, [[]])
    c["open_not_y_before_and_after_x"] = case([[(y,), (x,), (y,)]], one, [[]])
    # fx is the LATER first of X: 2 lies after 1 but not after 3
    c["open_later_first_of_x_decides"] = case([[(x,), (y,), (z,)]], [((x, z), (y,), 1, 1.0)], [[(y, 0)]])
    c["open_half_of_a_two_item_y"] = case([[(x,), (y,)]], [((x,), (y, z), 1, 1.0)], [[(z, 0)]])
    c["open_x_not_held"] = case([[(x,)], [(z,)]], [((x, z), (y,), 1, 1.0)], [[], []])
    ten = [[(10,), (20,)], [(20,)]]
    # values below, between and above the DB's
    c["open_unknown_y_is_predicted"] = case(ten, [((10,), (5, 15, 20, 25), 1, 1.0)], [[(5, 0), (15, 0), (25, 0)], []])
    c["open_unknown_x_predicts_nothing"] = case(ten, [((5, 10), (20,), 1, 1.0), ((10, 15), (30,), 1, 1.0),
                                                      ((20, 25), (10,), 1, 1.0), ((25,), (10,), 1, 1.0)], [[], []])
    # rule_support_ref's item_after_the_last_separator: row 0's 2 comes after its last -1, so the row
    # holds 1 alone; row 1 holds 1 then 2.  1 => 2 scores (1, 0.5) there, the other two (0, 0.0)
    sep = sref.hand_cases()["item_after_the_last_separator"]
    srules = scored(sep["records"], sep["rules"])
    assert [(r[2], r[3]) for r in srules] == [(1, 0.5), (0, 0.0), (0, 0.0)]
    c["open_item_after_the_last_separator"] = {"records": sep["records"], "rules": srules, "topn": 10,
                                               "expected": [[(y, 0)], [(x, 1), (z, 2)]]}
    # --- which rule is the best one
    both = [[(x, z)]]
    c["rank_by_confidence"] = case(both, [((x,), (y,), 5, 0.5), ((z,), (y,), 1, 0.9)], [[(y, 1)]])
    c["rank_confidence_tie_by_support"] = case(both, [((x,), (y,), 3, 0.5), ((z,), (y,), 7, 0.5)], [[(y, 1)]])
    c["rank_full_tie_by_index"] = case(both, [((x,), (y,), 3, 0.5), ((z,), (y,), 3, 0.5)], [[(y, 0)]])
    c["rank_repeated_rules"] = case(both, [((x,), (y,), 3, 0.5)] * 3 + [((x,), (4,), 3, 0.5)] * 2, [[(y, 0), (4, 3)]])
    c["rank_two_items_of_one_rule_by_value"] = case(both, [((x,), (5,), 1, 0.2), ((z,), (4, 9), 1, 0.7), ((x,), (6,), 1, 0.7)],
                                                    [[(4, 1), (9, 1), (6, 2), (5, 0)]])
    c["rank_items_by_their_best_rule"] = case(both, [((x,), (5,), 1, 0.3), ((x,), (4,), 1, 0.9), ((z,), (5,), 1, 0.95)],
                                              [[(5, 2), (4, 1)]])
    # --- topn
    three = [((x,), (7,), 1, 0.1), ((x,), (8,), 1, 0.3), ((x,), (9,), 1, 0.2)]
    full = [(8, 1), (9, 2), (7, 0)]
    rows = [[(x,)], [(z,)], [(x,), (8,)]]
    for name, topn in (("topn_1", 1), ("topn_equal_to_the_length", 3), ("topn_one_above_the_length", 4), ("topn_max", TOPN_MAX)):
        c[name] = case(rows, three, [full[:topn], [], [(9, 2), (7, 0)][:topn]], topn)
    return c


# ---------------------------------------------------------------- random DBs
_random = {}
RANDOM_TOPNS = (1, 3, ALL)
CONFIDENT = 0.5


def random_case(seed):
    """rule_support_ref.random_case(seed) with every rule scored by definition; expected[topn]
    is by_definition (the one reference of these DBs), computed once.  Every non-empty row
    holds some item a, and a => ABSENT fires there with ABSENT open, so with every rule no list
    is empty.  `confident` are the rules of confidence CONFIDENT and more, in input order (a
    rule set as a user would keep it), and confident_expected[topn] their lists: rows in which
    every confident rule that fires is fulfilled have an empty one."""
    if seed not in _random:
        base = sref.random_case(seed)
        rules = [(r[0], r[1], sup, conf) for r, (sup, _a, conf) in zip(base["rules"], base["expected"])]
        conf = [r for r in rules if r[3] >= CONFIDENT]
        _random[seed] = {"records": base["records"], "rules": rules, "support_triples": base["expected"],
                         "expected": {t: by_definition(base["records"], rules, t) for t in RANDOM_TOPNS},
                         "confident": conf,
                         "confident_expected": {t: by_definition(base["records"], conf, t) for t in RANDOM_TOPNS}}
    return _random[seed]


# what the 20 random DBs hold (asserted by the CPU and the GPU test, so that a generator
# change cannot empty a class silently).  With every rule: rows, rows with an empty list (none:
# see random_case), lists cut by topn = 3, entries, and the entries whose best rule beat its
# runner-up (the next rule under which the item is open) only by support at equal confidence,
# or only by index at equal confidence and support.  With the confident rules: the rules and
# the rows with an empty list.
RANDOM_TOTALS = {"rows": 372, "empty": 0, "cut3": 198, "entries": 1333, "by_support": 26, "by_index": 659,
                 "confident_rules": 608, "confident_empty": 111}
RANDOM_POSITIVE = ("confident_empty", "cut3", "by_support", "by_index")  # the four classes that must not be empty


def random_classes(records, rules):
    rows, order = open_ranks(records, rules)
    c = {k: 0 for k in ("rows", "empty", "cut3", "entries", "by_support", "by_index")}
    for opened in rows:
        c["rows"] += 1
        c["empty"] += not opened
        c["cut3"] += len(opened) > 3
        for rk in opened.values():
            c["entries"] += 1
            if len(rk) > 1:
                a, b = rules[order[rk[0]]], rules[order[rk[1]]]
                if a[3] == b[3]:
                    c["by_support" if a[2] != b[2] else "by_index"] += 1
    return c


def classes_of_lists(lists3, lists_all):
    """The classes that show in results: rows, empty lists, lists cut by topn = 3, entries."""
    return {"rows": len(lists_all), "empty": sum(1 for l in lists_all if not l),
            "cut3": sum(1 for a, b in zip(lists3, lists_all) if len(a) < len(b)), "entries": sum(len(l) for l in lists_all)}


def partial_rules(seed, limit=25):
    """Up to `limit` rules of the random case with 0 < support < ante, spread over the class,
    with their (support, ante)."""
    rc = random_case(seed)
    part = [(r, t) for r, t in zip(rc["rules"], rc["support_triples"]) if 0 < t[0] < t[1]]
    step = max(1, len(part) // limit)
    return part[::step][:limit]


# ---------------------------------------------------------------- tile edges
def tile_case(L, place, mode, fail=0):
    """rule_support_ref.tile_edge_case with its one rule scored (1, 1.0): "full" predicts nothing
    in any row (the L pivot rows hold the rule, the fillers lack the pivot), "lacks" nothing
    either (row `fail` does not fire), "order" Y_ITEM at row `fail` only (its y is in X's
    itemset or before it)."""
    t = sref.tile_edge_case(L, place, mode, fail)
    (X, Y), = t["rules"]
    exp = [[] for _ in t["records"]]
    if mode == "order":
        exp[fail] = [(sref.Y_ITEM, 0)]
    return {"records": t["records"], "rules": [(X, Y, 1, 1.0)], "topn": 10, "expected": exp, "pivot_rows": L}


def tile_inverse_case(L, place):
    """Every one of the L pivot rows has y before X: all L rows predict y, the 3 L filler rows
    (X's other items and y, not the pivot) predict nothing."""
    X = {"first": (9, 11, 12), "middle": (1, 9, 12), "last": (1, 2, 9)}[place]
    others = tuple(i for i in X if i != 9)
    rows = [[(sref.Y_ITEM,), X]] * L + [[others, (sref.Y_ITEM,)]] * (3 * L)
    return case(rows, [(X, (sref.Y_ITEM,), 1, 1.0)], [[(sref.Y_ITEM, 0)]] * L + [[]] * (3 * L))


def tile_cases(T):
    out = {}
    for L in sref.tile_lengths(T):
        for place in sref.PIVOT_PLACES:
            out["L%d-%s-full" % (L, place)] = tile_case(L, place, "full")
            out["L%d-%s-inverse" % (L, place)] = tile_inverse_case(L, place)
            for mode in ("lacks", "order"):
                for f in sref.failing_rows(L):
                    out["L%d-%s-%s-%d" % (L, place, mode, f)] = tile_case(L, place, mode, f)
    return out


def n_tile_cases(T):
    return sum(3 * (2 + 2 * len(sref.failing_rows(L))) for L in sref.tile_lengths(T))


# ---------------------------------------------------------------- segment lengths of one row
SEGMENT_SIZES = (1, 63, 64, 65, 1000)
SHARED = 5000


def segment_case(m, shared=False, topn=ALL):
    """Rows 0 and 2 hold the items 1 .. m in one itemset, rows 1 and 3 (interleaved by sid)
    item 1 alone, row 4 the even consequents (so half of the consequents are items of the DB,
    half are unknown to it; no rule fires there).  Rule j is (j + 1,) => (2001 + j,) with
    support 1 and the j-th of m distinct confidences in a shuffled order: all m rules fire in
    rows 0 and 2, whose list is every consequent in confidence order, and rule 0 alone in rows
    1 and 3.  shared: every rule has the one consequent SHARED instead, so a long row has one
    entry, owned by the rule of the highest confidence."""
    perm = list(range(m))
    random.Random(m).shuffle(perm)
    rules = [((j + 1,), (SHARED if shared else 2001 + j,), 1, (perm[j] + 1) / (m + 1)) for j in range(m)]
    longrow, short = [tuple(range(1, m + 1))], [(1,)]
    rows = [longrow, short, longrow, short, [tuple(2001 + j for j in range(0, m, 2))]]
    by_conf = sorted(range(m), key=lambda j: -rules[j][3])
    if shared:
        full = [(SHARED, by_conf[0])]
        one = [(SHARED, 0)]
    else:
        full = [(2001 + j, j) for j in by_conf]
        one = [(2001, 0)]
    return case(rows, rules, [full[:topn], one, full[:topn], one, []], topn)


def segment_cases():
    out = {}
    for m in SEGMENT_SIZES:
        for topn in sorted({1, m - 1, m, ALL} - {0}):
            out["m%d-top%d" % (m, topn)] = segment_case(m, False, topn)
        out["m%d-shared" % m] = segment_case(m, True)
    return out


# ---------------------------------------------------------------- row counts
def sid_edge_case(edb):
    """rule_support_ref.SID_EDGE_RULES (1 => 2, 3 => 4, 2 => 1) scored by definition on
    edge_dbs.tsr_sid_edges(N).  The deciding rows <1, 2> predict nothing from 1 => 2, which
    holds there, but 2 => 1 fires in them with 1 only before 2, so their list is (1, rule 2);
    the rows <3, 4> predict nothing; a row with 2 alone predicts 1 (rule 2), a row with 3
    alone 4 (rule 1), the rows with 5 or 6 alone nothing."""
    rules = [(r[0], r[1], t[0], t[2]) for r, t in zip(sref.SID_EDGE_RULES, sref.sid_edge_expected(edb))]
    taken = set(edb.deciding) | set(edb.second)
    exp = []
    for s in range(len(edb)):
        if s in edb.deciding:
            exp.append([(1, 2)])
        elif s in taken:
            exp.append([])
        else:
            exp.append({0: [(1, 2)], 1: [(4, 1)]}.get(s % 4, []))
    return {"rules": rules, "topn": 10, "expected": exp}


# ---------------------------------------------------------------- long sides
def long_side_case(m=300):
    """rule_support_ref.long_side_case with its rule scored (1, 1 / 3).  Row 0 holds X then Y and
    row 1 does not fire: no prediction.  Row 2 has Y[0] only before X: exactly Y[0].  Row 3
    holds X alone: the rule fires and the row holds no item of Y, so all of Y is open there."""
    base = sref.long_side_case(m)
    (X, Y), = base["rules"]
    (sup, _ante, conf), = base["expected"]
    return {"records": base["records"], "rules": [(X, Y, sup, conf)], "topn": ALL,
            "expected": [[], [], [(Y[0], 0)], [(y, 0) for y in Y]]}


# ---------------------------------------------------------------- the child of the hook test
def child_cases():
    """name -> case: the random DBs (topn = 3 and uncut), the tile-edge DBs and the segment cases."""
    import pattern_filter_ref as fref
    T = constants()["kRpTile"]
    out = {}
    for seed in range(fref.N_RANDOM):
        rc = random_case(seed)
        for topn in (3, ALL):
            out["random%d-top%d" % (seed, topn)] = {"records": rc["records"], "rules": rc["rules"], "topn": topn,
                                                    "expected": rc["expected"][topn]}
        out["random%d-confident" % seed] = {"records": rc["records"], "rules": rc["confident"], "topn": 3,
                                            "expected": rc["confident_expected"][3]}
    out.update(tile_cases(T))
    out.update(segment_cases())
    return out


def predict_cases(eng, cases):
    """-> ({name: lists}, {name: launches of k_rp_match})"""
    import spark_fsm_amd as fsm
    res, launches = {}, {}
    dbs = {}  # one DB per distinct record list (the cases of a family share theirs)
    try:
        for name, c in cases.items():
            key = id(c["records"])
            if key not in dbs:
                for db in dbs.values():
                    db.free()
                dbs = {key: eng.db_from_spmf(c["records"], fsm.MODE_TSR)}
            got = lists_of(eng.rule_predictions(dbs[key], c["rules"], c["topn"]))
            res[name] = [[list(p) for p in row] for row in got]
            launches[name] = sum(k["launches"] for k in eng.kernel_stats() if k["name"] == "k_rp_match")
    finally:
        for db in dbs.values():
            db.free()
    return res, launches


def _child():
    import spark_fsm_amd as fsm
    with fsm.Engine(0) as eng:
        res, launches = predict_cases(eng, child_cases())
    print(json.dumps({"results": res, "launches": launches}))


if __name__ == "__main__":
    _child()
