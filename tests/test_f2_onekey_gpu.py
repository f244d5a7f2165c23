"""k_f2_tri's one-kind wave step against its three-kind one, and the CPU oracle.

A wave step of the root F2 (unordered pairs, W = 1) writes its keys with one store when no
pair of the step has more than one of its three kinds (i -> j), (j -> i), (i, j), and per kind
otherwise.  Every DB here is one gadget row of n frequent entries (two for `runs`) placed on
one of those paths, plus short rows, mined at minsup 2:

  * one single-item row per item: every item is frequent, no pair is;
  * per targeted pair (the first and last partners of the first, second, middle and last but
    one entry, the gadget's own pair, and all pairs up to n = 8) and per kind one two-item row
    with that relation: a witness where the gadget row holds the relation (support exactly 2),
    a decoy where it does not (exactly 1); the same per repeat (i -> i) of a targeted item;
  * per neighbouring partner of a targeted pair a decoy for the kinds the gadget row does not
    hold, so every counter next to a targeted one stands at exactly 1.

A dropped, duplicated, mis-kinded or misplaced key then moves a 2-sequence into or out of the
result.  Gadgets (items in rank order 0 .. n - 1, k_f2_tri's lanes):

  single      every item once, partners before, after and in the same itemset: one-kind steps only
  allmulti    every item in the same two itemsets: every pair has three kinds, every repeat exists
  multi a b   item b twice, <.. {b} {a b} ..>, in an otherwise single row: (a, b) alone has two
              kinds, in the run of a; the repeat sits in the run of b
  repeat i    item i twice, alone in two adjacent itemsets: a repeat and no pair of two kinds
  both a b    item a twice, <.. {a} {a b} ..>: the repeat and the two-kind pair in one run
  runs        two rows of 7 and 15 entries, a two-kind pair in each: steps of several runs
  noise       single and multi rows with infrequent items below, between and above the others
              (n >= 15; from n = 63 on the row has more than 64 entries and is read from the DB)

at n = 2, 3, 15, 16, 31, 32, 63 (the folded segment sizes, n + 1 lanes), 64 (unfolded) and 70
(rows read from the DB); all of it once more on two ranks, where a row's active entries are a
sub-range."""
import random

import pytest

import edge_dbs as E

pytestmark = pytest.mark.gpu

LENGTHS = (2, 3, 15, 16, 31, 32, 63, 64, 70)


def val(base, k):
    return base + 2 * k  # even values: the odd ones between them are the infrequent items


class Gadget:
    """One row over items val(base, 0 .. n - 1) as itemsets; `multi`, `repeats`: what it claims
    (rank pairs with more than one kind, ranks at two eids); `pairs`: rank pairs to target."""

    def __init__(self, kind, n, base, sets, multi, repeats, pairs=()):
        self.kind, self.n, self.base = kind, n, base
        self.sets = [s for s in sets if s]
        self.multi, self.repeats, self.pairs = set(multi), set(repeats), list(pairs)
        self.eids = {}
        for e, s in enumerate(self.sets):
            for it in s:
                self.eids.setdefault(it, []).append(e)

    def holds(self, x, y, kind):
        """kind 0: x -> y, 1: y -> x, 2: (x y); x == y: the repeat (kind 0 alone)."""
        ex, ey = self.eids[x], self.eids[y]
        if kind == 0:
            return min(ex) < max(ey)
        if kind == 1:
            return x != y and min(ey) < max(ex)
        return x != y and bool(set(ex) & set(ey))

    def kinds(self, a, b):
        return sum(self.holds(val(self.base, a), val(self.base, b), k) for k in range(3))


def single_sets(n, base, seed):
    order = list(range(n))
    random.Random(seed).shuffle(order)
    return [sorted(val(base, k) for k in order[q:q + 2]) for q in range(0, n, 2)]


def with_twice(n, base, seed, twice, partner=None):
    """The single row with item `twice` taken out and put back as {twice} {twice, partner}
    (partner None: {twice} {twice}) in the middle of the row."""
    out = {val(base, twice)} | ({val(base, partner)} if partner is not None else set())
    sets = [[x for x in s if x not in out] for s in single_sets(n, base, seed)]
    sets = [s for s in sets if s]
    m = len(sets) // 2
    return sets[:m] + [[val(base, twice)], sorted(out)] + sets[m:]


def add_noise(g, m):
    """m infrequent items (odd values, once in the DB) spread by value over the row, one below
    and one above every frequent item, appended to the row's itemsets in turn."""
    zs = [g.base - 1, val(g.base, g.n) + 1] + [val(g.base, (q * g.n) // m) + 1 for q in range(m - 2)]
    assert len(set(zs)) == m
    sets = [list(s) for s in g.sets]
    for q, z in enumerate(zs):
        sets[(q * 3) % len(sets)].append(z)
    out = Gadget(g.kind + "+noise", g.n, g.base, [sorted(s) for s in sets], g.multi, g.repeats, g.pairs)
    out.noise = zs
    return out


def make_gadget(kind, n, base=10, seed=1, a=None, b=None):
    if kind == "single":
        return Gadget(kind, n, base, single_sets(n, base, seed), (), ())
    if kind == "allmulti":
        row = [val(base, k) for k in range(n)]
        return Gadget(kind, n, base, [row, row], [(i, j) for i in range(n) for j in range(i + 1, n)], range(n))
    if kind == "multi":
        return Gadget(kind, n, base, with_twice(n, base, seed, b, a), [(a, b)], [b], [(a, b)])
    if kind == "both":
        return Gadget(kind, n, base, with_twice(n, base, seed, a, b), [(a, b)], [a], [(a, b)])
    assert kind == "repeat"
    return Gadget(kind, n, base, with_twice(n, base, seed, a), (), [a], [(a, a + 1)] if a + 1 < n else [(a - 1, a)])


def targets(g):
    n = g.n
    if n <= 8:
        return [(i, j) for i in range(n) for j in range(i + 1, n)]
    m = n // 2
    out = list(g.pairs)
    for i in (0, 1, m, n - 2):
        for j in (i + 1, i + 2, m, n - 2, n - 1):
            if i < j < n and (i, j) not in out:
                out.append((i, j))
    return out


def build_db(gadgets, name):
    rows, want2, want1 = [], set(), set()
    for g in gadgets:
        rows.append(E._row(g.sets))
    for g in gadgets:
        v = lambda k: val(g.base, k)
        rows.extend(E._row([[v(k)]]) for k in range(g.n))
        tg = targets(g)
        tset = set(tg)

        def rel(x, y, kind):
            return ((x,), (y,)) if kind == 0 else ((y,), (x,)) if kind == 1 else ((min(x, y), max(x, y)),)

        for i, j in tg:
            for kind in range(3):
                p = rel(v(i), v(j), kind)
                rows.append(E._row([list(s) for s in p]))
                (want2 if g.holds(v(i), v(j), kind) else want1).add(p)
            for i2, j2 in ((i, j - 1), (i, j + 1), (i - 1, j), (i + 1, j)):
                if not (0 <= i2 < j2 < g.n) or (i2, j2) in tset:
                    continue
                for kind in range(3):
                    p = rel(v(i2), v(j2), kind)
                    if not g.holds(v(i2), v(j2), kind) and p not in want1:
                        rows.append(E._row([list(s) for s in p]))
                        want1.add(p)
        for k in sorted({k for pr in tg for k in pr} | g.repeats):
            p = ((v(k),), (v(k),))
            rows.append(E._row([[v(k)], [v(k)]]))
            (want2 if g.holds(v(k), v(k), 0) else want1).add(p)
    db = E.EdgeDB(rows, name)
    db.gadgets, db.want2, db.want1 = gadgets, want2, want1
    return db


def pick_pairs(n):
    out = []
    for p in ((0, 1), (0, n - 1), (n - 2, n - 1), (n // 2 - 1, n // 2 + 1)):
        if 0 <= p[0] < p[1] < n and p not in out:
            out.append(p)
    return out


def cases(family):
    """[(name, db)] of a family, built once per process."""
    def make():
        out = []
        for n in LENGTHS:
            if family in ("single", "allmulti"):
                gs = [make_gadget(family, n)]
            elif family in ("multi", "both"):
                gs = [make_gadget(family, n, a=a, b=b, seed=a + b) for a, b in pick_pairs(n)]
            elif family == "repeat":
                gs = [make_gadget("repeat", n, a=a) for a in (0, n - 1)]
            elif family == "noise" and n >= 15:
                a, b = pick_pairs(n)[-1]
                gs = [add_noise(make_gadget("single", n), 5), add_noise(make_gadget("multi", n, a=a, b=b), 5)]
            else:
                continue
            out.extend(("%s-n%d-%d" % (family, n, q), build_db([g], g.kind)) for q, g in enumerate(gs))
        if family == "runs":
            gs = [make_gadget("multi", 7, base=10, a=2, b=5), make_gadget("both", 15, base=100, a=3, b=14)]
            out.append(("runs-7-15", build_db(gs, "runs")))
        return out
    return E._cached(("onekey", family), make)


FAMILIES = ("single", "allmulti", "multi", "both", "repeat", "runs", "noise")

_REF = {}


def ref(name, db):
    if name not in _REF:
        from oracle import oracle
        _REF[name] = oracle.spade_tokens(db.seq_off, db.tokens, db.support)
    return _REF[name]


@pytest.fixture(scope="module", params=["one-rank", "two-ranks"])
def eng(request):
    import spark_fsm_amd
    e = spark_fsm_amd.Engine(0) if request.param == "one-rank" else spark_fsm_amd.Engine(devices=[0, 0])
    yield e
    e.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_shape(family):
    """What the docstrings claim, from the rows and the oracle: the two-kind pairs and the repeats
    of every gadget row are exactly the named ones, the row lengths are the named ones, every
    targeted relation the gadget holds has support exactly 2 and no other 2-sequence is frequent."""
    for name, db in cases(family):
        o = ref(name, db)
        assert o["minsup"] == 2, name
        freq1 = {p[0][0] for p, _ in o["patterns"] if len(p) == 1 and len(p[0]) == 1}
        for g in db.gadgets:
            items = [val(g.base, k) for k in range(g.n)]
            assert set(items) <= freq1 and not (set(getattr(g, "noise", ())) & freq1), name
            assert len(set(g.eids) & freq1) == g.n, name
            multi = {(i, j) for i in range(g.n) for j in range(i + 1, g.n) if g.kinds(i, j) > 1}
            assert multi == g.multi, name
            assert all(g.kinds(i, j) >= 1 for i in range(g.n) for j in range(i + 1, g.n)), name
            assert {k for k in range(g.n) if len(g.eids[items[k]]) > 1} == g.repeats, name
            if g.kind == "allmulti":
                assert all(g.kinds(i, j) == 3 for i, j in multi), name
            if hasattr(g, "noise"):
                zs = set(g.noise)
                assert min(zs) < items[0] and max(zs) > items[-1] and any(items[0] < z < items[-1] for z in zs), name
                assert len(g.eids) == g.n + len(zs), name
        two = {p: s for p, s in o["patterns"] if sum(len(s_) for s_ in p) == 2}
        assert set(two) == db.want2, name
        assert all(s == 2 for s in two.values()), name
        assert db.want2 and not (db.want2 & db.want1), name
        assert len(db.rows) <= 400, (name, len(db.rows))


@pytest.mark.parametrize("family", FAMILIES)
def test_onekey(eng, family):
    from spark_fsm_amd import MODE_SPADE
    for name, db in cases(family):
        o = ref(name, db)
        h = eng.db_from_tokens(db.sids, db.seq_off, db.tokens, MODE_SPADE)
        try:
            pats, meta = eng.spade(h, db.support)
            assert meta["minsup"] == o["minsup"], name
            assert sorted(pats) == o["patterns"], name
            assert eng.stats()["joins"] == o["joins"], name
        finally:
            h.free()
