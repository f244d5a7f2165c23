"""References and shared inputs of the closed / maximal pattern filter tests
(test_pattern_filter.py, test_pattern_filter_gpu.py).  Not a test module.

A pattern is (itemsets, support): itemsets a tuple of ascending item tuples.  Both
references return the kept indexes, ascending.

  definitional(pats, keep)  quadratic, by definition: P is dropped iff some other pattern
                            strictly contains it (and has equal support, for closed)
  by_deletion(pats, keep)   linear, by the one-item-deletion lemma: P is
                            dropped iff deleting one item from some pattern of the set
                            (of equal support, for closed) yields P

The two agree on a COMPLETE frequent set with anti-monotone supports; every input
built here that both are applied to is closed under one-item deletions.

Run as a script (`python pattern_filter_ref.py`), this module filters collision_sets()
on the GPU and prints {name: {keep: kept_idx}} as JSON: the child process of the
forced-collision test, started with FSM_PF_HASH_BITS set.
"""
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "spark-fsm_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle.brute import _contains  # noqa: E402

KEEPS = ("closed", "maximal")
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


# ---------------------------------------------------------------- references
_def_cache = {}


def _definitional_flags(pats):
    """[(has a strict super-pattern, has one of equal support)] per pattern, against ALL
    patterns (a pattern with no more items cannot strictly contain another)."""
    hit = _def_cache.get(id(pats))
    if hit is not None and hit[0] is pats:
        return hit[1]
    pool = {}
    fs = [[pool.setdefault(X, frozenset(X)) for X in sets] for sets, _ in pats]
    size = [sum(len(X) for X in sets) for sets, _ in pats]
    flags = []
    for i, (ps, psup) in enumerate(pats):
        any_sup, eq_sup = False, False
        for j, (qs, qsup) in enumerate(pats):
            if j == i or size[j] <= size[i] or (any_sup and (eq_sup or qsup != psup)):
                continue
            if _contains(fs[j], fs[i]):
                any_sup = True
                eq_sup = eq_sup or qsup == psup
        flags.append((any_sup, eq_sup))
    _def_cache.clear()
    _def_cache[id(pats)] = (pats, flags)
    return flags


def definitional(pats, keep):
    assert keep in KEEPS
    flags = _definitional_flags(pats)
    return [i for i, (a, e) in enumerate(flags) if not (e if keep == "closed" else a)]


def tokens(sets):
    """The canonical key: one (item, starts-a-new-itemset) token per item."""
    return tuple((it, k == 0) for X in sets for k, it in enumerate(X))


def deletions(sets):
    """Every pattern that deleting one item yields (an emptied itemset disappears;
    its neighbours are not merged)."""
    for s, X in enumerate(sets):
        for k in range(len(X)):
            Y = X[:k] + X[k + 1:]
            yield sets[:s] + ((Y,) if Y else ()) + sets[s + 1:]


def by_deletion(pats, keep):
    assert keep in KEEPS
    closed = keep == "closed"
    index = {}
    for i, (sets, sup) in enumerate(pats):
        index.setdefault((tokens(sets), sup if closed else None), []).append(i)
    drop = set()
    for sets, sup in pats:
        if sum(len(X) for X in sets) < 2:
            continue
        for d in deletions(sets):
            drop.update(index.get((tokens(d), sup if closed else None), ()))
    return [i for i in range(len(pats)) if i not in drop]


# ---------------------------------------------------------------- CSR forms
def to_csr(pats):
    sup, po, so, it = [], [0], [0], []
    for sets, s in pats:
        sup.append(s)
        for X in sets:
            it.extend(X)
            so.append(len(it))
        po.append(len(so) - 1)
    return (np.array(sup, np.int32), np.array(po, np.int64), np.array(so, np.int64), np.array(it, np.int32))


def from_csr(csr):
    sup, po, so, it = (np.asarray(a).tolist() for a in csr)
    return [(tuple(tuple(it[so[s]:so[s + 1]]) for s in range(po[p], po[p + 1])), sup[p]) for p in range(len(sup))]


def take(csr, idx):
    """The patterns idx (ascending) of a CSR, as a CSR."""
    sup, po, so, it = (np.asarray(a) for a in csr)
    idx = np.asarray(idx, np.int64)
    nsets = po[idx + 1] - po[idx]
    set_idx = np.repeat(po[idx] - np.concatenate(([0], np.cumsum(nsets)[:-1])), nsets) + np.arange(int(nsets.sum()))
    nit = so[set_idx + 1] - so[set_idx]
    item_idx = np.repeat(so[set_idx] - np.concatenate(([0], np.cumsum(nit)[:-1])), nit) + np.arange(int(nit.sum()))
    return (sup[idx].astype(np.int32), np.concatenate(([0], np.cumsum(nsets))).astype(np.int64),
            np.concatenate(([0], np.cumsum(nit))).astype(np.int64), it[item_idx].astype(np.int32))


def csr_equal(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------- hand cases
def _seq(*items):
    return tuple((i,) for i in items)


def down_closure(sets):
    """sets and everything repeated one-item deletions yield, longest first, distinct."""
    out, level = [sets], {sets}
    while level:
        level = {d for p in level for d in deletions(p) if d}
        out.extend(sorted(level))
    return out


def hand_cases():
    """name -> patterns; each closed under one-item deletions where it matters, so both
    references apply.  `known` holds the kept indexes where the answer is stated."""
    a, b, c, d = 1, 2, 3, 4
    cases = {}
    cases["n1"] = [(_seq(a), 5)]
    cases["one_item_only"] = [(_seq(a), 5), (_seq(b), 5), (_seq(c), 4), (_seq(a), 3)]
    # prefix chain of equal support, then a drop in support
    cases["prefix_chain"] = [(_seq(a), 9), (_seq(a, b), 9), (_seq(a, b, c), 9), (_seq(a, b, c, d), 7)]
    # <(a)(b)(c)> minus b is <(a)(c)>, never <(a c)>
    cases["no_merge"] = [(_seq(a, b, c), 4), (((a, c),), 4), (_seq(a, c), 4), (_seq(a, b), 4), (_seq(b, c), 4),
                         (_seq(a), 4), (_seq(b), 4), (_seq(c), 4)]
    # <(a b)> and <(a)(b)> do not contain each other
    cases["itemset_vs_sequence"] = [(((a, b),), 6), (_seq(a, b), 6), (_seq(a), 6), (_seq(b), 6)]
    # an item deleted from the first, middle and last position of an itemset
    cases["itemset_positions"] = [(((a, b, c),), 5), (((b, c),), 5), (((a, c),), 5), (((a, b),), 5),
                                  (_seq(a), 5), (_seq(b), 5), (_seq(c), 5), (((a, d),), 5), (_seq(d), 5)]
    # the same inside a longer pattern: the itemset's neighbours keep their own starts
    mid = ((d,), (a, b, c), (d,))
    cases["itemset_positions_inner"] = [(mid, 3)] + [(p, 3) for p in deletions(mid)] + [(((d,), (a, b, c, d)), 3)]
    # a singleton itemset deleted at the start, middle and end, with neighbours that would merge wrongly
    q = ((a,), (b,), (c,), (d,))
    cases["singleton_positions"] = ([(q, 8)] + [(p, 8) for p in deletions(q)] +
                                    [(((a, b), (c,)), 8), (((a,), (b, c)), 8), (((a, b), (d,)), 8), (((a,), (c, d)), 8),
                                     (((b, c), (d,)), 8), (((b,), (c, d)), 8)])
    q = ((a, b), (c,), (a, b))
    cases["singleton_between_itemsets"] = [(q, 2)] + [(p, 2) for p in deletions(q)] + [(((a, b), (a, b, c)), 2),
                                                                                     (((a, b, c), (a, b)), 2)]
    # the same tokens with different supports: closed keeps both, maximal drops the shorter
    cases["support_differs"] = [(_seq(a, b), 7), (_seq(a, b, c), 5), (_seq(a), 7), (_seq(b), 7)]
    # repeated items: every deletion of a->a->a is a->a
    cases["repeated_items"] = [(_seq(a, a, a), 3), (_seq(a, a), 3), (_seq(a), 4)]
    # items drawn from {INT32_MIN, -1, 0, 1, INT32_MAX}: a 7-item pattern and all its sub-patterns
    q = ((I32_MIN, -1, 0), (I32_MAX,), (1,), (I32_MIN, I32_MAX))
    cases["extreme_items"] = [(p, 2 + (7 - sum(len(X) for X in p)) // 3) for p in down_closure(q)]
    # an exact duplicate is a separate entry and does not drop its twin
    cases["duplicate"] = [(_seq(a, b), 4), (_seq(a, b), 4), (_seq(a), 4), (_seq(a), 4), (_seq(b), 5)]
    cases["duplicate_long"] = [(_seq(a, b, c), 4), (_seq(a, b), 4), (_seq(a, b), 4), (_seq(a, b, c), 4)]
    return cases


KNOWN = {  # name -> {keep: kept indexes}
    "n1": {"closed": [0], "maximal": [0]},
    "one_item_only": {"closed": [0, 1, 2, 3], "maximal": [0, 1, 2, 3]},
    "prefix_chain": {"closed": [2, 3], "maximal": [3]},
    "no_merge": {"closed": [0, 1], "maximal": [0, 1]},
    "itemset_vs_sequence": {"closed": [0, 1], "maximal": [0, 1]},
    "support_differs": {"closed": [0, 1], "maximal": [1]},
    "repeated_items": {"closed": [0, 2], "maximal": [0]},
    "duplicate": {"closed": [0, 1, 4], "maximal": [0, 1]},
    "duplicate_long": {"closed": [0, 3], "maximal": [0, 3]},
}


# ---------------------------------------------------------------- geometry sets
def prefix_set(length=300, support=7):
    """All prefixes of one sequence of `length` single-item itemsets, equal support:
    length * (length + 1) / 2 items; only the longest is closed."""
    rng = random.Random(300)
    seq = tuple((rng.randint(1, 5),) for _ in range(length))
    return [(seq[:k], support) for k in range(1, length + 1)]


def long_pattern_csr(length=3000, support=4):
    """One pattern of `length` distinct single-item itemsets followed by its `length`
    one-item deletions, equal support: only the first is closed (and maximal).  Built
    as a CSR directly (9 M items)."""
    base = np.arange(1, length + 1, dtype=np.int32)
    rows = [base] + [np.delete(base, k) for k in range(length)]
    items = np.concatenate(rows)
    n = length + 1
    sizes = np.array([len(r) for r in rows], np.int64)
    po = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    so = np.arange(len(items) + 1, dtype=np.int64)
    return (np.full(n, support, np.int32), po, so, items)


def long_pattern_list(length=3000, support=4):
    """long_pattern_csr as a pattern list (the itemset tuples are shared)."""
    pool = [(i,) for i in range(1, length + 1)]
    full = tuple(pool)
    return [(full, support)] + [(full[:k] + full[k + 1:], support) for k in range(length)]


def level_set(n):
    """The first n sequences over {1, 2, 3, 4} in order of length (all of a length before
    the next: closed under deletions), with the anti-monotone support 1000 - the sum of
    the item weights (0, 1, 0, 2): extending by item 1 or 3 keeps the support."""
    w = {1: 0, 2: 1, 3: 0, 4: 2}
    out, level = [], [()]
    while len(out) < n:
        level = [p + (x,) for p in level for x in (1, 2, 3, 4)]
        for p in level:
            if len(out) == n:
                break
            out.append((_seq(*p), 1000 - sum(w[x] for x in p)))
    return out


def item_count_set(total):
    """Prefix chains of single items whose item counts sum to `total` (255, 256, 257)."""
    out, left, base = [], total, 10
    while left:
        k = 1
        while k <= left and k <= 21:
            out.append((_seq(*range(base, base + k)), 5))
            left -= k
            k += 1
        base += 100
    assert sum(len(s) for s, _ in out) == total
    return out


def geometry_sets():
    sets = {"prefix300": prefix_set()}
    for n in (1023, 1024, 1025, 2047, 2048, 2049):
        sets["level_n%d" % n] = level_set(n)
    for t in (255, 256, 257):
        sets["items%d" % t] = item_count_set(t)
    return sets


def collision_sets():
    """The sets of at most 2,049 patterns that run again with forced hash collisions."""
    out = dict(hand_cases())
    out.update(geometry_sets())
    return out


# ---------------------------------------------------------------- random tiny DBs
def random_db(seed):
    """(records, support): <= 30 sequences over <= 6 items, itemsets of 1-3 items."""
    rng = random.Random(7000 + seed)
    nitems = rng.randint(3, 6)
    recs = []
    for sid in range(rng.randint(8, 30)):
        sets = []
        for _ in range(rng.randint(1, 5)):
            sets.append(sorted(rng.sample(range(1, nitems + 1), rng.randint(1, min(3, nitems)))))
        recs.append((sid, " ".join(" ".join(map(str, X)) + " -1" for X in sets) + " -2"))
    return recs, rng.choice((0.1, 0.15, 0.2, 0.3))


N_RANDOM = 20
MAX_RANDOM_PATTERNS = 1500
_mined = {}


def mined_random_db(seed):
    """(records, support, complete set by the CPU oracle); the support is raised until the
    set has at most MAX_RANDOM_PATTERNS patterns (the quadratic reference stays in seconds)."""
    if seed not in _mined:
        from oracle import oracle
        recs, sup = random_db(seed)
        while True:
            pats = oracle.spade(recs, sup)["patterns"]
            if len(pats) <= MAX_RANDOM_PATTERNS:
                break
            sup += 0.05
        _mined[seed] = (recs, sup, [(tuple(tuple(X) for X in s), int(c)) for s, c in pats])
    return _mined[seed]


def _child():
    import spark_fsm_amd as fsm
    res = {}
    with fsm.Engine(0) as eng:
        for name, pats in collision_sets().items():
            csr = to_csr(pats)
            res[name] = {}
            for keep in KEEPS:
                out, idx = eng.filter_patterns(csr, keep)
                if not csr_equal(out, take(csr, idx)):
                    raise AssertionError("%s/%s: result is not the kept patterns in order" % (name, keep))
                res[name][keep] = idx.tolist()
    print(json.dumps(res))


if __name__ == "__main__":
    _child()
