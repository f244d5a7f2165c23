"""Threshold-tight databases placed on the kernels' geometry constants.

TEST INFRASTRUCTURE ONLY (plain Python, no GPU).  Two ideas:

* threshold-tight: every candidate the miner counts is exactly at the
  threshold (support == minsup) or exactly one below it, so a count that is
  off by one anywhere (a pair counted twice, one sequence's contribution
  dropped) changes the frequent set instead of hiding behind a margin;
* the generators say where their rows and runs fall (`geometry`), so a test
  can assert that its DB really has the length / offset it is named after
  (a 64-entry run at lane 0, a run that starts at range - 1, ...).

Families: `tight_spade` (hub sequences), `wide_mask_db` (one sequence of E
itemsets), `word_sweep_db` (one decision on every word boundary of the mask),
`big_row_db` (one DB row of n entries), `tsr_long_rows`, `tsr_sid_edges`,
and `k0_image`, the DB image by definition from the token rules (SPADE.scala:53-106, :151-210; TSR.scala:52-94, :109-143); and the TSR
families placed on the expansion kernels' constants (`tsr_constants`, read
from tsr_engine.hip): `tsr_probe_edges`, `tsr_kid_edges`, `tsr_chain`,
`tsr_pair_edges`; and `tall_spade`, SPADE along the sequence axis: R short rows mined at a
minsup in the thousands, the supporting rows placed on the root F2's row blocks
(`spade_constants`, `f2_row_blocks`, read from spade_engine.hip), with the K0 cases
of the same sizes (`k0_stage_case`, `k0_extreme_cases`, `with_lead`).
"""
import os
import random
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_SRC = os.path.join(ROOT, "spark-fsm_amd", "csrc", "spade_engine.hip")


class EdgeDB:
    """A database as token rows (-1 closes an itemset, -2 ends the row), with
    the views the engine and the oracle take: SPMF text records and the token
    arrays (sids 0..N-1)."""

    def __init__(self, rows, name=""):
        self.rows = rows
        self.name = name
        lens = [len(r) for r in rows]
        self.seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.tokens = np.fromiter((t for r in rows for t in r), dtype=np.int64, count=int(self.seq_off[-1]))
        self.sids = np.arange(len(rows), dtype=np.int32)

    def __len__(self):
        return len(self.rows)

    def records(self):
        return [(s, " ".join(map(str, r))) for s, r in enumerate(self.rows)]

    @property
    def support(self):
        """The relative support that makes minsup = ceil(support * N) = 2."""
        return 1.5 / len(self.rows)


def _row(itemsets, end=True):
    out = []
    for s in itemsets:
        out.extend(s)
        out.append(-1)
    if end:
        out.append(-2)
    return out


def itemsets_of(row):
    """Closed itemsets of a token row, empty ones included (TSR indexes count them)."""
    sets, cur = [], []
    for t in row:
        if t == -1:
            sets.append(cur)
            cur = []
        elif t != -2:
            cur.append(t)
    return sets


# ---------------------------------------------------------------- SPADE hubs
def _selected_ranks(n):
    """Rank pairs (a < b) of a hub of n items that get a private two-item
    sequence: first, last, middle, middle +- 1 and their neighbours (at most 8)."""
    if n < 2:
        return []
    m = n // 2
    cand = [(0, 1), (n - 2, n - 1), (0, n - 1), (m - 1, m), (m, m + 1), (0, m), (m, n - 1), (1, n - 2)]
    out = []
    for a, b in cand:
        if 0 <= a < b < n and (a, b) not in out:
            out.append((a, b))
    return out


class TightSpade(EdgeDB):
    """tight_spade's result: the DB plus what it claims about itself.

    selected      {pattern: 2}: the planted multi-item patterns over hub items
                  (without the common prefix), every one at support 2
    singles       {item: support} of every frequent non-prefix item
    prefix_items  the common one-item itemsets A1..Ad heading every sequence
    hub_rows      row index of each hub
    hub_items     per hub: its frequent items in ascending value (rank) order
    rest_sample   per hub: pairs of ranks (first, last, middle ...) that were NOT selected
    """

    def expected(self):
        """The complete frequent set at minsup 2, in closed form: every ordered
        sub-chain of the prefix, alone (support N) or followed by a frequent
        single item or a selected pattern (their own supports)."""
        N = len(self.rows)
        base = {((i,),): s for i, s in self.singles.items()}
        base.update(self.selected)
        d = len(self.prefix_items)
        out = dict(base)
        for bits in range(1, 1 << d):
            chain = tuple((self.prefix_items[k],) for k in range(d) if bits >> k & 1)
            out[chain] = N
            for p, s in base.items():
                out[chain + p] = s
        return sorted(out.items())

    def root_entries(self):
        """(frequent item, sequence) entries of the root class at minsup 2."""
        freq = set(self.singles) | set(self.prefix_items)
        return sum(len({t for t in r if t >= 0} & freq) for r in self.rows)


STRETCH_BASE = 1 << 18  # values of the itemsets `stretch` adds: above every item of a stretched hub family


def tight_spade(lengths, per_set=1, lead=0, prefix=0, pad=0, noise=0, dup=False, filler=0, hub_last=False, seed=1,
                stretch=0):
    """The hub family.  For each n in `lengths` one hub sequence holds n fresh
    items, `per_set` per itemset, in shuffled order (rank is not position).
    Each item has one private single-item sequence (support 2); a few pairs
    chosen by rank (`_selected_ranks`) have one private two-item sequence that
    repeats the pair's relation in the hub (x -> y, or (x y) in one itemset),
    and with `dup` the lowest item of each hub is placed twice and x -> x is
    selected.  At minsup 2 every selected relation has support exactly 2, every
    other pair of a hub exactly 1, and no triple of hub items reaches 2.

    prefix = d  prepends the one-item itemsets A1 .. Ad (items 1..d, the lowest
                ranks) to every sequence: the same structure reappears in the
                classes [A1], [A1 -> A2], ...
    lead = j    (int, or one per hub) puts j filler sequences right before that
                hub; pad = p puts p prefix-only sequences before the first hub
                (root run d, [A1] run d - 1): together they place a run start
    filler = F  at least F frequent filler items, two single-item sequences each
    noise = m   m infrequent items interleaved (by value and by itemset) in
                every hub: the DB row grows past its frequent entries
    hub_last    the last hub is the last sequence (its runs end at E)
    stretch = T every hub sequence has exactly T itemsets: unique infrequent one-item
                itemsets go between the hub's own (its first stays right behind the
                prefix, its last becomes itemset T - 1), so the hub's eids spread
                over all the words of a mask of ceil(T / 64) words
    """
    rng = random.Random(seed)
    lengths = list(lengths)
    leads = [lead] + [0] * (len(lengths) - 1) if isinstance(lead, int) else list(lead)
    assert len(leads) == len(lengths)
    d = prefix
    pre = [[a] for a in range(1, d + 1)]
    nfill = max(filler, (sum(leads) + 1) // 2)
    fill_items = list(range(d + 1, d + 1 + nfill))
    fill_rows = [_row(pre + [[f]]) for f in fill_items for _ in (0, 1)]
    base = d + 1 + nfill
    rows, hub_rows, hub_items, rest = [_row(pre) for _ in range(pad)] if d else [], [], [], []
    assert d or not pad
    singles = {f: 2 for f in fill_items}
    selected, tail, fi, nstretch = {}, [], 0, 0
    for n, j in zip(lengths, leads):
        items = [base + 2 * i for i in range(n)]
        noise_items = [base + 2 * (i * n // max(noise, 1)) + 1 for i in range(noise)]
        assert len(set(noise_items)) == noise
        base += 2 * n + 2
        order = items[:]
        rng.shuffle(order)
        sets = [sorted(order[k:k + per_set]) for k in range(0, n, per_set)]
        for k, z in enumerate(noise_items):
            sets[k % len(sets)].append(z)
        where = {x: k for k, s in enumerate(sets) for x in s}
        if dup:
            sets.append([items[0]])
        for x in items:
            singles[x] = 2
            tail.append(_row(pre + [[x]]))
        sel = _selected_ranks(n)
        for a, b in sel:
            x, y = items[a], items[b]
            if where[x] == where[y]:
                p = ((x, y),)
            elif where[x] < where[y]:
                p = ((x,), (y,))
            else:
                p = ((y,), (x,))
            selected[p] = 2
            singles[x] += 1
            singles[y] += 1
            tail.append(_row(pre + [list(s) for s in p]))
        if dup:
            x = items[0]
            selected[((x,), (x,))] = 2
            singles[x] += 1
            tail.append(_row(pre + [[x], [x]]))
        m = n // 2
        rest.append([(a, b) for a, b in [(0, 2), (n - 3, n - 1), (m - 2, m), (m - 1, m + 1), (0, n - 2), (1, n - 1), (1, m)]
                     if 0 <= a < b < n and (a, b) not in sel])
        rows.extend(fill_rows[fi:fi + j])
        fi += j
        hub_rows.append(len(rows))
        hub_items.append(items)
        if stretch:
            T, n0 = stretch - d, len(sets)
            assert T >= n0, "the hub has more itemsets than `stretch`"
            at = {(k * (T - 1) // (n0 - 1) if n0 > 1 else 0): s for k, s in enumerate(sets)}
            assert len(at) == n0
            sets = [at[k] if k in at else [STRETCH_BASE + nstretch + k] for k in range(T)]
            nstretch += T
        rows.append(_row(pre + sets))
    rest_rows = fill_rows[fi:] + tail
    rng.shuffle(rest_rows)
    if hub_last:
        hub = rows.pop()
        rows.extend(rest_rows)
        hub_rows[-1] = len(rows)
        rows.append(hub)
    else:
        rows.extend(rest_rows)
    assert not stretch or base <= STRETCH_BASE
    db = TightSpade(rows, "tight%s/%d" % (lengths, per_set))
    db.kw = dict(lengths=lengths, per_set=per_set, lead=lead, prefix=prefix, pad=pad, noise=noise, dup=dup,
                 filler=filler, hub_last=hub_last, seed=seed, stretch=stretch)
    db.selected, db.singles, db.prefix_items = selected, singles, list(range(1, d + 1))
    db.hub_rows, db.hub_items, db.rest_sample = hub_rows, hub_items, rest
    return db


def closed_form_ref(db):
    """The oracle's answer for a large filler DB (prefix = 1) without mining it: the patterns are
    expected(); the joins are those of the root (F members: F^2 + F (F - 1) / 2) and of [A1]
    (F - 1 members) plus a constant of the hub structure, which filler items do not touch; the
    constant is read off the oracle's join count on the same DB built with 20 filler items
    (tests/test_edge_dbs.py checks the form against the oracle at sizes it can mine quickly)."""
    from oracle import oracle
    assert db.kw["prefix"] == 1 and not db.kw["pad"] and not db.kw["lead"]

    def base(F):
        return F * F + F * (F - 1) // 2 + (F - 1) * (F - 1) + (F - 1) * (F - 2) // 2
    twin = tight_spade(**dict(db.kw, filler=20))
    F0, F = len(twin.singles) + 1, len(db.singles) + 1
    c = oracle.spade_tokens(twin.seq_off, twin.tokens, twin.support)["joins"] - base(F0)
    return {"patterns": db.expected(), "joins": base(F) + c, "minsup": 2}


def relation(db, hub, a, b):
    """The pair of ranks (a, b) of a hub as the pattern the hub itself holds."""
    sets = itemsets_of(db.rows[db.hub_rows[hub]])
    x, y = db.hub_items[hub][a], db.hub_items[hub][b]
    wx = next(k for k, s in enumerate(sets) if x in s)
    wy = next(k for k, s in enumerate(sets) if y in s)
    if wx == wy:
        return ((min(x, y), max(x, y)),)
    return ((x,), (y,)) if wx < wy else ((y,), (x,))


def place(level, start, prefix):
    """(lead, pad) for tight_spade so that the first hub's run starts at entry
    `start` of the root class (level 0: a filler sequence is a run of
    prefix + 1, a prefix-only one of prefix) or of [A1] (level 1: prefix and
    prefix - 1).  geometry() then confirms the placement."""
    big = prefix + 1 - level
    small = big - 1
    if small == 0:
        assert start % big == 0
        return start // big, 0
    for pad in range(0, big):
        if (start - pad * small) >= 0 and (start - pad * small) % big == 0:
            return (start - pad * small) // big, pad
    raise AssertionError("no placement")


# ---------------------------------------------------------------- geometry
def wave_ranges():
    """Entries per wave range of k_emit2 (root, W = 1 lattice, W > 1 lattice)
    and of k_count2, read from the engine source's own #define lines."""
    with open(ENGINE_SRC) as f:
        src = f.read()
    out = {}
    for key, name in (("root", "FSM_E2_RANGE_ROOT"), ("lattice", "FSM_E2_RANGE"), ("lattice_w", "FSM_E2_RANGE_W"),
                      ("count2", "FSM_C2_RANGE")):
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, src, re.M)
        assert m, "no #define %s in spade_engine.hip" % name
        out[key] = int(m.group(1))
    return out


def geometry(rows, minsup, classes=True):
    """Run layout by definition.  A class is stored one run per sequence that
    contains its prefix, one entry per member present, sequences in sid order.

    root     [(start, length)]: frequent items of each sequence (the root slab)
    root_db  the same over all distinct items (the DB rows the DB-direct root reads)
    classes  {A: [(start, length)]} for each frequent item A: the members
             A -> x and (A x) with support >= minsup present in each sequence
    E        entries in all (root, root_db, and per class)
    """
    seqs = []
    for r in rows:
        fl = {}
        for k, s in enumerate(x for x in itemsets_of(r) if x):
            for it in s:
                f = fl.setdefault(it, [k, k, set()])
                f[1] = k
                f[2].add(k)
        seqs.append(fl)
    sup = {}
    for fl in seqs:
        for it in fl:
            sup[it] = sup.get(it, 0) + 1
    freq = {i for i, c in sup.items() if c >= minsup}

    def runs(lens):
        out, at = [], 0
        for n in lens:
            if n:
                out.append((at, n))
            at += n
        return out, at

    g = {"ranges": wave_ranges()}
    g["root"], g["E_root"] = runs(len(freq & set(fl)) for fl in seqs)
    g["root_db"], g["E_db"] = runs(len(fl) for fl in seqs)
    if not classes:
        return g
    psup, present = {}, []
    for fl in seqs:
        mem = {}
        its = sorted(i for i in fl if i in freq)
        for a in its:
            fa = fl[a]
            for x in its:
                fx = fl[x]
                if fa[0] < fx[1]:
                    mem.setdefault(a, []).append((x, 0))
                if x > a and fa[2] & fx[2]:
                    mem.setdefault(a, []).append((x, 1))
        present.append(mem)
        for a, ms in mem.items():
            for m in ms:
                psup[(a, m)] = psup.get((a, m), 0) + 1
    g["classes"], g["E_class"] = {}, {}
    for a in sorted(freq):
        g["classes"][a], g["E_class"][a] = runs(
            sum(1 for m in mem.get(a, ()) if psup[(a, m)] >= minsup) for mem in present)
    return g


def run_at(runs, start=None, length=None, end=None):
    """The runs of a layout with the given start / length / end (any of them)."""
    return [(s, n) for s, n in runs if (start is None or s == start) and (length is None or n == length)
            and (end is None or s + n == end)]


# ---------------------------------------------------------------- wide masks
class Planted(EdgeDB):
    def expected(self):
        out = {((i,),): s for i, s in self.singles.items()}
        out.update(self.selected)
        return sorted(out.items())

    def root_entries(self):
        freq = set(self.singles)
        return sum(len({t for t in r if t >= 0} & freq) for r in self.rows)


def _plant(rows_before, big, planted_at, name):
    """Shared tail of wide_mask_db / big_row_db: `big` is the long sequence as
    itemsets, planted_at {item: itemset index}; every planted item gets a
    private sequence, the neighbouring planted pairs and (first, last) get a
    private two-item sequence repeating their relation, the other pairs stay
    at support 1."""
    its = sorted(planted_at, key=lambda i: (planted_at[i], i))
    singles = {i: 2 for i in its}
    sel = [(its[k], its[k + 1]) for k in range(0, len(its) - 1, 2)]
    if len(its) > 2:
        sel.append((its[0], its[-1]))
    if len(its) > 3:
        sel.append((its[1], its[-2]))
    if len(its) > 1 and planted_at[its[-2]] == planted_at[its[-1]] and (its[-2], its[-1]) not in sel:
        sel.append((its[-2], its[-1]))
    selected, tail = {}, [_row([[i]]) for i in its]
    for x, y in sel:
        p = ((min(x, y), max(x, y)),) if planted_at[x] == planted_at[y] else ((x,), (y,))
        selected[p] = 2
        singles[x] += 1
        singles[y] += 1
        tail.append(_row([list(s) for s in p]))
    rest = [(x, y) for a, x in enumerate(its) for y in its[a + 1:] if (x, y) not in sel]
    db = Planted(rows_before + [_row(big, end=False)] + tail, name)
    db.selected, db.singles, db.planted_at, db.rest_pairs, db.big_row = selected, singles, planted_at, rest, len(rows_before)
    return db


def wide_mask_db(E, shared_last=True):
    """One sequence of exactly E non-empty itemsets, each one unique (infrequent)
    noise item, except that planted items 1..6 take the itemsets at eids 0, 1,
    63, 64, E - 2, E - 1 (those below E, once each); with `shared_last` item 7
    shares the last itemset.  Without it the row is exactly 2 E tokens (at
    E = 4,096 the 8,192 tokens of the longest row the device build takes)."""
    big = [[1000 + k] for k in range(E)]
    planted_at = {}
    for it, e in zip(range(1, 7), (0, 1, 63, 64, E - 2, E - 1)):
        if 0 <= e < E and e not in planted_at.values():
            planted_at[it] = e
            big[e] = [it]
    if shared_last:
        planted_at[7] = E - 1
        big[E - 1].append(7)
    db = _plant([_row([[8]]), _row([[8]])], big, planted_at, "wide-mask-%d" % E)
    db.singles[8] = 2
    return db


class WordSweep(Planted):
    """word_sweep_db's result.
    t2, t1     the decisions (patterns) that hold / do not hold in S: support exactly 2 / exactly 1
    boundary   {decision: k}, gadget {decision: label}
    ks, eids   the boundaries swept, and {item: eids in S}"""

    def words_of(self, patterns):
        """The boundaries (word indexes) of the decisions that share a planted item with any of
        `patterns`: where to look when a comparison fails."""
        own = {}
        for p, k in self.boundary.items():
            for s in p:
                for it in s:
                    own[it] = (k, self.gadget[p])
        return sorted({own[it] for p in patterns for s in p for it in s if it in own})


def _eids_of(eids, pattern):
    """The first eid at which `pattern` ends in a sequence given as {item: eids}, or None: greedy
    by definition (each itemset at the earliest eid after the one before that holds all its items)."""
    prev = -1
    for s in pattern:
        common = set(eids.get(s[0], ()))
        for it in s[1:]:
            common &= set(eids.get(it, ()))
        later = [e for e in common if e > prev]
        if not later:
            return None
        prev = min(later)
    return prev


def _sub_patterns(p):
    """Every non-empty sub-pattern of p (items removed, empty itemsets dropped)."""
    flat = [(k, it) for k, s in enumerate(p) for it in s]
    out = set()
    for bits in range(1, 1 << len(flat)):
        sets = {}
        for j, (k, it) in enumerate(flat):
            if bits >> j & 1:
                sets.setdefault(k, []).append(it)
        out.add(tuple(tuple(sets[k]) for k in sorted(sets)))
    return out


def prefix_parents(p):
    """The two prefix-class parents of a pattern of two or more items: p without its last item,
    and p without the item before it."""
    flat = [(k, it) for k, s in enumerate(p) for it in s]
    out = []
    for drop in (len(flat) - 1, len(flat) - 2):
        sets = {}
        for j, (k, it) in enumerate(flat):
            if j != drop:
                sets.setdefault(k, []).append(it)
        out.append(tuple(tuple(sets[k]) for k in sorted(sets)))
    return out


def word_sweep_db(W, ks=None, E=None):
    """One sequence S of E itemsets (default 64 W: W mask words), one unique infrequent item in
    each, and for every word boundary k in `ks` (default 1 .. W - 1) a set of gadgets around
    b = 64 k - 1, the last bit of word k - 1 (b + 1 is the first bit of word k).  d is a decoy eid
    in an earlier word (two words back where there is one, otherwise in word 0), d2 = d + 3.

    A gadget uses fresh items and makes ONE decision, a pattern p whose only other sequence is p
    itself: its support is exactly 2 if S holds p (`t2`) and exactly 1 if not (`t1`), every one of
    its items has support 2, and both its prefix-class parents hold in S (support 2), so the
    lattice reaches the decision through tight parents.  x@e: item x sits at eid e of S.

    G1a  a@b, c@b+1: a -> c holds          (temporal count across the boundary)
    G1b  a@b, c@b+1: c -> a does not
    G1c  a@b, c@b:   a -> c does not        (the same eid is not "after")
    G2a  p@{d, b+1}, q@b+1: (p q) holds     (the only common bit is in word k)
    G2b  p@{d, b+1}, q@b: (p q) does not    (the eid ranges overlap, the AND is empty)
    G3   x@b, y@{d, b+1}, z@b+1: x -> y -> z does not  (temporal child: bits <= lo cleared, its new
         lo found in word k; an uncleared decoy makes it hold)
    G4   the same with z@b+2: holds
    G5a  w@d, p@{d2, b+1}, q@b+1, r@b+1: w -> (p q) -> r does not  (the child of an equality join
         as the owner of a temporal join)
    G5b  the same with r@b+2: holds
    G6a  x@b, y@{b, b+1}, z@b+1: x -> y -> z does not  (the partner's bit AT lo is cleared too: lo
         the last bit of word k - 1, the whole word goes)
    G6b  x@b+1, y@{b+1, b+2}, z@b+2: the same with lo the first bit of word k
    G7   x@d, y@{b, b+2}, z@b+1: x -> y -> z holds  (the child's lo is the last bit of word k - 1
         while word k holds a later bit)
    G8   x@b+1, y@{d, 64 (k+1)}, z@64 (k+1): x -> y -> z does not  (lo in word k, the partner's
         only later bit in word k + 1: word k + 1 is kept whole, the new lo found there)
    G9a  x@d, y@{d2, b+1}, q@b+1: x -> (y q) holds  (a temporal child keeps its bit in word k,
         and its hi there passes the range prefilter)
    G9b  the same with q@b: does not
    Gadgets that need eid b + 2 (or 64 (k + 1)) are left out where S ends before it."""
    E = 64 * W if E is None else E
    ks = list(range(1, W)) if ks is None else list(ks)
    big = [[1000000 + e] for e in range(E)]
    eids, t2, t1, boundary, gadget = {}, [], [], {}, {}
    nxt = [1]

    def fresh(*at):
        out = []
        for es in at:
            it = nxt[0]
            nxt[0] += 1
            es = (es,) if isinstance(es, int) else tuple(es)
            assert all(0 <= e < E for e in es)
            eids[it] = sorted(es)
            for e in es:
                big[e].append(it)
            out.append(it)
        return out

    def decide(k, label, p, holds):
        assert (_eids_of(eids, p) is not None) == holds, (k, label)
        (t2 if holds else t1).append(p)
        boundary[p], gadget[p] = k, label

    for k in ks:
        b = 64 * k - 1
        assert 0 < b and b + 1 < E
        d = 64 * (k - 2) + 5 if k >= 3 else 5
        d2 = d + 3
        a, c = fresh(b, b + 1)
        decide(k, "G1a", ((a,), (c,)), True)
        a, c = fresh(b, b + 1)
        decide(k, "G1b", ((c,), (a,)), False)
        a, c = fresh(b, b)
        decide(k, "G1c", ((a,), (c,)), False)
        p, q = fresh((d, b + 1), b + 1)
        decide(k, "G2a", ((p, q),), True)
        p, q = fresh((d, b + 1), b)
        decide(k, "G2b", ((p, q),), False)
        x, y, z = fresh(b, (d, b + 1), b + 1)
        decide(k, "G3", ((x,), (y,), (z,)), False)
        w, p, q, r = fresh(d, (d2, b + 1), b + 1, b + 1)
        decide(k, "G5a", ((w,), (p, q), (r,)), False)
        x, y, z = fresh(b, (b, b + 1), b + 1)
        decide(k, "G6a", ((x,), (y,), (z,)), False)
        x, y, q = fresh(d, (d2, b + 1), b + 1)
        decide(k, "G9a", ((x,), (y, q)), True)
        x, y, q = fresh(d, (d2, b + 1), b)
        decide(k, "G9b", ((x,), (y, q)), False)
        if b + 2 < E:
            x, y, z = fresh(b, (d, b + 1), b + 2)
            decide(k, "G4", ((x,), (y,), (z,)), True)
            w, p, q, r = fresh(d, (d2, b + 1), b + 1, b + 2)
            decide(k, "G5b", ((w,), (p, q), (r,)), True)
            x, y, z = fresh(b + 1, (b + 1, b + 2), b + 2)
            decide(k, "G6b", ((x,), (y,), (z,)), False)
            x, y, z = fresh(d, (b, b + 2), b + 1)
            decide(k, "G7", ((x,), (y,), (z,)), True)
        if 64 * (k + 1) < E:
            x, y, z = fresh(b + 1, (d, 64 * (k + 1)), 64 * (k + 1))
            decide(k, "G8", ((x,), (y,), (z,)), False)
    decisions = t2 + t1
    rows = [_row([sorted(s) for s in big])] + [_row([list(s) for s in p]) for p in decisions]
    db = WordSweep(rows, "word-sweep-W%d-E%d" % (W, E))
    db.singles = {it: 2 for it in eids}
    # closed form: a multi-item pattern over planted items is held by one private sequence at
    # most (the gadgets share no item), so it is frequent iff it is a sub-pattern of a decision and S holds it
    db.selected = {}
    for p in decisions:
        for q in _sub_patterns(p):
            if sum(len(s) for s in q) > 1 and _eids_of(eids, q) is not None:
                db.selected[q] = 2
    db.W, db.E, db.ks, db.eids, db.t2, db.t1, db.boundary, db.gadget = W, E, ks, eids, t2, t1, boundary, gadget
    return db


def big_row_db(n, nsets=60):
    """One DB row of exactly n distinct items over `nsets` itemsets (W = 1), three
    of them frequent: the lowest, the middle and the highest value of the row."""
    vals = list(range(10, 10 + n))
    big = [vals[k::nsets] for k in range(nsets)]
    big = [s for s in big if s]
    planted = (vals[0], vals[n // 2], vals[-1])
    planted_at = {it: next(k for k, s in enumerate(big) if it in s) for it in planted}
    assert len(planted_at) == 3
    return _plant([], big, planted_at, "big-row-%d" % n)


def planted_relation(db, x, y):
    ax, ay = db.planted_at[x], db.planted_at[y]
    if ax == ay:
        return ((min(x, y), max(x, y)),)
    return ((x,), (y,)) if ax < ay else ((y,), (x,))


# ---------------------------------------------------------------- TSR
def tsr_long_rows(T, N=8, tight=(), short_between=0):
    """All N sequences hold items 1, 2, 3 in itemsets 0, 1, 2 (five rules of
    support N among them).  Tail item j (10 + j, j < T) sits in itemset 0 in half
    of the sequences and in itemset 3 in the other half; a tail item listed in
    `tight` (by j) sits in itemset 0 in N - 1 sequences and in itemset 3 in one.
    Every tail item has support N; every rule with a tail item has support
    <= N - 1 (t -> 2, t -> 3 reach exactly N - 1 for a tight t).
    short_between = m puts m sequences <2, 1> after each long one: they are in
    the domain of every rule over 1 and 2 (one-entry rows between the long ones)
    and add the rule 2 -> 1 above the threshold, which stays N."""
    tight = set(tight)
    rows = []
    for s in range(N):
        head, back = [1], []
        for j in range(T):
            if j in tight:
                at0 = s != j % N
            else:
                at0 = (s + j) % 2 == 0
            (head if at0 else back).append(10 + j)
        rows.append(_row([head, [2], [3], back]))
        for _ in range(short_between):
            rows.append(_row([[2], [1]]))
    db = EdgeDB(rows, "tsr-long-%d" % T)
    db.T, db.N, db.tight = T, N, sorted(tight)
    return db


SID_EDGES = (31, 32, 127, 128, 1023, 1024, 32767, 32768)


def tsr_sid_edges(N):
    """Six items, N sequences.  Rule 1 -> 2 holds exactly at sids 0, 1, the edge
    sids below N (SID_EDGES) and N - 1: support m.  Rule 3 -> 4 holds at m - 1
    other sids.  Every other sequence holds one item alone (2, 3, 5 or 6: no rule),
    so with minconf 0 and k = 1 the answer is 1 -> 2 alone, and it is lost or
    tied as soon as one deciding sid is not counted; k = 2 returns both."""
    deciding = sorted({0, 1, N - 1} | {e for e in SID_EDGES if e < N})
    m = len(deciding)
    others = [s for s in range(2, N) if s not in deciding]
    step = max(1, len(others) // (m - 1))
    second = others[::step][:m - 1]
    assert len(second) == m - 1
    rows = []
    for s in range(N):
        if s in deciding:
            rows.append(_row([[1], [2]]))
        elif s in second:
            rows.append(_row([[3], [4]]))
        else:
            rows.append(_row([[(2, 3, 5, 6)[s % 4]]]))
    db = EdgeDB(rows, "tsr-sids-%d" % N)
    db.deciding, db.second = deciding, second
    return db


def tsr_deep_index(last_index):
    """Two sequences whose last itemset index is `last_index` (empty itemsets in
    between count), plus short ones: rules 1 -> 2 (support 3) and 1 -> 3, 3 -> 2
    (support 2) across the whole index range."""
    deep = [1, -1] + [-1] * (last_index - 2) + [3, -1, 2, -1, -2]
    assert len(itemsets_of(deep)) == last_index + 1
    return EdgeDB([deep, list(deep), _row([[1], [2]]), _row([[2], [1]])], "tsr-deep-%d" % last_index)


# ---------------------------------------------------------------- K0 image
def k0_image(rows, mode):
    """The DB image by definition, as fsm_db_export lays it out.  mode "spade":
    -1 closes an itemset, -2 is ignored, items after the last -1 are dropped; an
    entry per distinct item of a row in ascending value, its mask the set of
    eids (rank of the itemset among the row's non-empty closed itemsets) it
    occurs at; mask_words the smallest power of two covering the longest row's
    eids; max_occ the most closed item tokens of one row.  mode "tsr": an
    entry's first / last are the 0-based itemset indexes counting every -1.
    Item ids are dense ranks over the values of all entries."""
    ent = []  # per row: sorted [(value, eids)]
    max_eids = max_occ = 0
    for r in rows:
        closed, cur = [], []
        for t in r:
            if t == -1:
                closed.append(cur)
                cur = []
            elif t != -2:
                cur.append(int(t))
        occ = {}
        if mode == "spade":
            closed = [s for s in closed if s]
            max_occ = max(max_occ, sum(len(s) for s in closed))
        max_eids = max(max_eids, len(closed))
        for e, s in enumerate(closed):
            for it in s:
                occ.setdefault(it, []).append(e)
        ent.append(sorted(occ.items()))
    vals = sorted({v for row in ent for v, _ in row})
    dense = {v: k for k, v in enumerate(vals)}
    E = sum(len(row) for row in ent)
    img = {"rows": len(rows), "entries": E, "items": len(vals),
           "row_off": np.concatenate([[0], np.cumsum([len(row) for row in ent])]).astype(np.uint32),
           "item": np.array([dense[v] for row in ent for v, _ in row], dtype=np.uint32),
           "item_val": np.array(vals, dtype=np.int32)}
    if mode == "spade":
        W = 1
        while W * 64 < max_eids:
            W *= 2
        mask = np.zeros((E, W), dtype=np.uint64)
        q = 0
        for row in ent:
            for _, es in row:
                for e in es:
                    mask[q, e >> 6] |= np.uint64(1 << (e & 63))
                q += 1
        img.update(mask_words=W, max_occ=max_occ, mask=mask.reshape(-1))
    else:
        img["first"] = np.array([es[0] for row in ent for _, es in row], dtype=np.uint32)
        img["last"] = np.array([es[-1] for row in ent for _, es in row], dtype=np.uint32)
    return img


# ---------------------------------------------------------------- case tables
# The DBs of tests/test_edges_gpu.py, built once per process; tests/test_edge_dbs.py
# proves the claims (tightness, geometry) of the very same objects without a GPU.
F2_LENGTHS = (1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 62, 63, 64, 65, 66, 127, 128, 129)
LATTICE_SHORT = (63, 64, 65, 66)
LATTICE_LONG = (127, 128, 129, 192, 193, 256, 257)
RK_SIZES = (2047, 2048, 2049, 4096, 4097)
FREQ_RECS_ROWS = 16385
MASK_E = (63, 64, 65, 128, 129, 4096, 4097, 65535, 65536)
MASK_W = (1, 1, 2, 2, 4, 64, 128, 1024, 1024)
TSR_T = (4095, 4096, 4097, 4200, 8300)
TSR_N = (31, 32, 33, 127, 128, 129, 1023, 1024, 1025, 32767, 32768, 32769)

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def hub_run(db, g, hub, level):
    """(start, length) of hub `hub`'s run in the root class (level 0, the slab
    layout), in the DB rows (level "db") or in [A1] (level 1)."""
    layout = g["classes"].get(1, []) if level == 1 else g["root_db" if level == "db" else "root"]
    # runs are listed for sequences with entries: in these families every sequence has some
    assert len(layout) == len(db.rows), "a sequence without entries: runs are not row-aligned"
    return layout[db.hub_rows[hub]]


def f2_cases():
    """Family 1, root F2 row lengths: (name, db, {hub: DB row length})."""
    def make():
        out = []
        db = tight_spade(F2_LENGTHS, per_set=3, seed=2)
        out.append(("all", db, {h: n for h, n in enumerate(F2_LENGTHS)}))
        ns = (15, 32, 33, 61, 62, 63, 64)
        db = tight_spade(ns, per_set=3, noise=3, seed=3)  # rl > 64 with n <= 64 frequent
        out.append(("noise", db, {h: n + 3 for h, n in enumerate(ns)}))
        ns = (3, 4, 63, 64, 65)
        db = tight_spade(ns, per_set=3, dup=True, seed=4)
        out.append(("dup", db, {h: n for h, n in enumerate(ns)}))
        return out
    return _cached("f2", make)


def lattice_cases(w):
    """Family 2, lattice windows at mask width w (1, 2, 4 or 8), prefix = 2:
    (name, db, level, claim) where claim is a dict of geometry facts to assert:
    {"length": L} for hub 0's run at `level`, {"start": s}, {"end_is_E": True}.
    At w = 4 and 8 every hub is stretched to exactly 64 w itemsets (tight_spade's
    `stretch`): its entries' eids lie in every word of the mask."""
    def make():
        out = []
        d = 2
        st = 64 * w if w > 2 else 0
        # run lengths: a hub of n items is a run of n + 2 in the root, n + 1 in [A1], n in [A1 -> A2]
        ns = sorted({L - k for L in LATTICE_SHORT + LATTICE_LONG for k in (0, 1)})
        if w == 1:
            out.append(("lengths", tight_spade(ns, per_set=5, prefix=d, seed=5), 1,
                        {"lengths": [n + 1 for n in ns]}))
        else:  # 64 < itemsets <= 128 in the longest sequence (w = 2); per_set = 3: 257 items fit 254 itemsets
            out.append(("lengths", tight_spade(ns, per_set=3, prefix=d, seed=5, stretch=st), 1,
                        {"lengths": [n + 1 for n in ns]}))
        n = 63  # a 64-entry run in [A1]
        ps = 3 if w == 1 else 1  # per_set = 1: 65 itemsets, two mask words
        for r in range(64, 513, 64):
            for start in (r - 63, r - 1, r):
                lead, pad = place(1, start, d)
                db = tight_spade([n], per_set=ps, prefix=d, lead=lead, pad=pad, seed=start, stretch=st)
                out.append(("L1-start%d" % start, db, 1, {"start": start, "length": 64}))
                if w == 1:  # the same placement in the root class (no prefix: every filler run is one entry)
                    db = tight_spade([64], per_set=ps, lead=start, seed=start)
                    out.append(("L0-start%d" % start, db, 0, {"start": start, "length": 64}))
        db = tight_spade([20, n], per_set=ps, prefix=d, lead=[3, 5], hub_last=True, seed=6, stretch=st)
        out.append(("hub-last", db, 1, {"end_is_E": True, "length": 64}))
        return out
    return _cached(("lattice", w), make)


def check_lattice_claim(db, level, claim, minsup=2):
    """Assert that the DB has the geometry its case is named after; returns the geometry."""
    g = geometry(db.rows, minsup)
    if "lengths" in claim:
        got = [hub_run(db, g, h, level)[1] for h in range(len(db.hub_rows))]
        assert got == claim["lengths"], (got, claim)
        return g
    hub = len(db.hub_rows) - 1
    s, n = hub_run(db, g, hub, level)
    if "start" in claim:
        assert s == claim["start"], (s, claim)
    if "length" in claim:
        assert n == claim["length"], (n, claim)
    if claim.get("end_is_E"):
        assert s + n == (g["E_class"][1] if level == 1 else g["E_root"])
    return g


def mask_width(db):
    """u64 mask words of a SPADE DB: the smallest power of two covering the most
    non-empty itemsets of one sequence."""
    e = max(sum(1 for s in itemsets_of(r) if s) for r in db.rows)
    w = 1
    while w * 64 < e:
        w *= 2
    return w


def rk_cases():
    """Family 3, row-table sizes: (name, db, rows of the root batch, rows of the
    first-level batch).  prefix = 1 and one hub of 5: the root batch has one
    counter row per frequent item (F), the first-level batch one per member:
    F - 1 members A1 -> x plus one per selected pattern."""
    def make():
        out = []
        nsel = len(_selected_ranks(5))
        for F in RK_SIZES + (FREQ_RECS_ROWS,):
            for which, Fx in (("root", F), ("level1", F + 1 - nsel)):
                db = tight_spade([5], per_set=2, prefix=1, filler=Fx - 6, seed=F)
                out.append(("%s-%d" % (which, F), db, Fx, Fx - 1 + nsel))
        return out
    return _cached("rk", make)


ONE_ROW_GROUP_F = (8192, 8193, 10923, 10924, 16384)


def one_row_group_cases():
    """(F, db): F frequent items whose root counter row (2 F counters) takes more than half
    of a rank group's 32,768 counters from F = 8,193 on, so the ordered root F2 holds one row
    per group; 16,384 is the last F it takes (8,192: the last with two rows per group).  10,923 is
    the last F of the unordered layout (its first row has 1 + 3 (F - 1) counters), 10,924 the first
    that takes the ordered one by default."""
    return _cached("one_row", lambda: [(F, tight_spade([5], per_set=2, prefix=1, filler=F - 6, seed=7))
                                       for F in ONE_ROW_GROUP_F])


def mask_cases():
    return _cached("mask", lambda: [(E, W, wide_mask_db(E, shared_last=E != 4096)) for E, W in zip(MASK_E, MASK_W)])


SWEEP_W = (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)


def sweep_ks(W):
    """The word boundaries word_sweep_db takes at width W: every one at the register-held widths
    (the kernels' word loops are unrolled: each word has code of its own), and at the runtime
    widths (loops over the words) the first two, both sides of word 64 (4,096 eids: the device
    build's limit), the middle and the last."""
    if W <= 64:
        return list(range(1, W))
    return sorted({1, 2, 63, 64, 65, W // 2 - 1, W // 2, W - 1})


def sweep_case(W):
    return _cached(("sweep", W), lambda: word_sweep_db(W, sweep_ks(W)))


def big_row_cases():
    return _cached("bigrow", lambda: [(n, big_row_db(n)) for n in (65535, 65536)])


def tsr_long_cases():
    """(name, db, k, minconf): tsr_long_rows at TSR_T with the first, middle and
    last tail item tight, and a mixed DB with short sequences between the long ones
    (there 1 -> 2 has confidence 8 / 32)."""
    def make():
        out = [("T%d" % T, tsr_long_rows(T, tight=(0, T // 2, T - 1)), 5, 0.5) for T in TSR_T]
        out.append(("mixed", tsr_long_rows(4200, tight=(0, 2100, 4199), short_between=3), 5, 0.2))
        return out
    return _cached("tsr_long", make)


def tsr_sid_cases():
    return _cached("tsr_sid", lambda: [(N, tsr_sid_edges(N)) for N in TSR_N])


def k0_cases():
    """(name, rows, modes, device build expected) for the K0 image comparison."""
    def make():
        rng = random.Random(8)
        out = []

        def rnd(L, items=40):
            return [rng.choice((-1, -1, -2)) if rng.random() < 0.3 else rng.randint(1, items) for _ in range(L)]
        # token counts on the wave / block / host switches; a short closed row beside each
        for L in (0, 1, 63, 64, 65, 8191, 8192, 8193):
            rows = [rnd(L)[:max(L - 1, 0)] + ([-1] if L else []), [1, 2, -1, 3, -1, -2], rnd(30)]
            out.append(("tokens-%d" % L, rows, ("spade", "tsr"), L <= 8192))
        one = [5, -1] * 4096  # one item in all 4,096 itemsets of an 8,192-token row
        out.append(("one-item-4096-sets", [one, [5, -1, 6, -1]], ("spade", "tsr"), True))
        rep = [t for k in range(4096) for t in (1 + rng.randrange(16), -1 if k % 3 else -2)]
        rep[-1] = -1
        out.append(("16-items-repeated", [rep, [1, -1]], ("spade", "tsr"), True))
        for rng_items, ok in ((2 ** 19 - 1, True), (2 ** 19, True), (2 ** 19 + 1, True), (2 ** 27, True),
                              (2 ** 27 + 1, False)):
            lo, hi = 7, 7 + rng_items - 1  # hi - lo + 1 values in the range, three of them present
            mid = lo + rng_items // 2
            rows = [[hi, -1, lo, mid, -1, lo, -1], [mid, -1, hi, -1], [lo, hi, -1]]
            out.append(("range-%d" % rng_items, rows, ("spade", "tsr"), ok))
        for E, ok in ((4096, True), (4097, False)):
            row = [t for k in range(E) for t in (1 + k % 50, -1)]
            out.append(("eids-%d" % E, [row, [1, -1, 2, -1]], ("spade",), ok))
        return out
    return _cached("k0", make)


# ---------------------------------------------------------------- TSR on the expansion kernels' constants
TSR_SRC = os.path.join(ROOT, "spark-fsm_amd", "csrc", "tsr_engine.hip")


def tsr_constants():
    """The constants of tsr_engine.hip the TSR families below are placed on, read from the source
    itself (every one must be found), plus what the kernels derive from them:
    group       sids per rank-directory entry (bm_rank: one 16-byte group of four 32-bit words)
    wave_groups sids per wave of k_rank_dir (64 groups), rank_round per block round (kBlock groups)
    exp_win     domain rows per k_exp_rows window (kExpWin = 2 kXBlock)
    reduce_range kids per k_expand_reduce block (ceil(kPassKids / kCollectBlocks))
    dl_round    bitmap words (AND branch) or list sids (list branch) per k_dl block round
    pair_batch0 items of the pair phase's first batch (doubling up to 4,096)"""
    def make():
        with open(TSR_SRC) as f:
            src = f.read()
        out = {}
        m = re.search(r"^#define\s+FSM_TSR_XBLOCK\s+(\d+)\b", src, re.M)
        assert m, "no #define FSM_TSR_XBLOCK in tsr_engine.hip"
        out["FSM_TSR_XBLOCK"] = int(m.group(1))
        for name in ("kPassKids", "kCollectBlocks", "kDomThreads", "kBlock", "kDlUnroll", "kExpSpb", "kExpBatch",
                     "kExpBatchWide", "kWideMinsup"):
            m = re.search(r"^constexpr\s+(?:int|uint32_t)\s+%s\s*=\s*(\d+)\s*;" % name, src, re.M)
            assert m, "no constexpr %s in tsr_engine.hip" % name
            out[name] = int(m.group(1))
        assert re.search(r"kExpWin\s*=\s*2\s*\*\s*kXBlock\s*;", src), "kExpWin is no longer 2 * kXBlock"
        assert re.search(r"g\s*=\s*sid\s*>>\s*7\b", src), "bm_rank no longer takes 128-sid groups"
        m = re.search(r"uint32_t\s+nb_items\s*=\s*(\d+)\s*;", src)
        assert m, "no first pair batch size (nb_items) in tsr_engine.hip"
        out["pair_batch0"] = int(m.group(1))
        out["group"] = 128
        out["wave_groups"] = 64 * out["group"]
        out["rank_round"] = out["kBlock"] * out["group"]
        out["exp_win"] = 2 * out["FSM_TSR_XBLOCK"]
        out["reduce_range"] = -(-out["kPassKids"] // out["kCollectBlocks"])
        out["dl_round"] = out["kBlock"] * out["kDlUnroll"]
        return out
    return dict(_cached("tsr_constants", make))


def probe_edges():
    """Sids one before and on the group, wave-of-groups, round and two-round edges of k_rank_dir
    (127, 128, 8,191, 8,192, 32,767, 32,768, 65,535, 65,536 with 256 threads per block)."""
    c = tsr_constants()
    return tuple(s for e in (c["group"], c["wave_groups"], c["rank_round"], 2 * c["rank_round"]) for s in (e - 1, e))


def window_edges():
    """Sids one before and on the first two window ends of k_exp_rows (1,023, 1,024, 2,047, 2,048)."""
    w = tsr_constants()["exp_win"]
    return (w - 1, w, 2 * w - 1, 2 * w)


def bitmap_words(N):
    """Words of a sid bitmap: whole 128-sid groups."""
    return (N + 127) // 128 * 4


def tsr_probe_edges(N, extra=(), edges=None, dl=None, sup3=None):
    """Two item triples, (1, 2, 3) and (11, 12, 13); every sequence holds all six items in three
    itemsets.  A triple (a, b, c) HOLDS in a row <{a}, {c}, {b}> and FAILS in <{b}, {c}, {a}>; the
    two triples share the itemsets of a row (<{a, a'}, {c, c'}, {b, b'}>, each triple in its own
    order).  A fail row has the same items, so it is in every domain and is probed like a hold
    row, with first / last values that make the rule fail.

    Triple 1 holds exactly at the `deciding` sids: 0, 1, N - 1, every sid of `edges` (default
    probe_edges()) below N, and `extra`: m = len(deciding) rows, so a -> b, a -> c, c -> b,
    a -> {b, c}, {a, c} -> b and the rules that add 13 (present in every row's middle itemset)
    have support exactly m.  Triple 2 holds at m - 1 other sids spread between them (`second`):
    its rules have support m - 1.  The reversed rules (b -> a ...) have support N - m and
    N - m + 1.  A rank that is off by one at a deciding row or at a fail row reads another row's
    first / last and moves a count across the line between m and m - 1.

    dl = "and":  item 3 is removed from the fail rows at and beside the edge sids (`removed`),
                 so |sids({1, 3})| = N - len(removed), counted by k_dl's AND branch
                 (sup(3) >= bitmap words);
    dl = "list": item 3 stays in the hold rows of both triples, in those fail rows and in evenly
                 spread others, sup3 sequences in all (default: bitmap words - 2, the longest list the
                 list branch takes), and is removed everywhere else."""
    edges = probe_edges() if edges is None else tuple(edges)
    deciding = sorted({0, 1, N - 1} | {e for e in edges if e < N} | {e for e in extra if 0 <= e < N})
    m = len(deciding)
    dset = set(deciding)
    beside = sorted({s for e in edges for s in (e - 2, e - 1, e, e + 1) if 0 <= s < N} - dset)
    others = [s for s in range(2, N) if s not in dset and s not in beside]
    step = max(1, len(others) // (m - 1))
    second = others[::step][:m - 1]
    assert len(second) == m - 1, (N, m)
    sset = set(second)
    if dl is None:
        removed = set()
    elif dl == "and":
        removed = set(beside)
        assert N - len(removed) >= bitmap_words(N)
    else:
        assert dl == "list"
        n3 = bitmap_words(N) - 2 if sup3 is None else sup3
        keep = list(deciding) + second + beside
        rest = [s for s in others if s not in sset]
        need = n3 - len(keep)
        assert 0 < need <= len(rest), (N, n3)
        keep += rest[::max(1, len(rest) // need)][:need]
        assert len(keep) == n3 < bitmap_words(N) or sup3 is not None
        removed = set(range(N)) - set(keep)
    rows = []
    for s in range(N):
        h1, h2 = s in dset, s in sset
        head = [1 if h1 else 2, 11 if h2 else 12]
        tail = [2 if h1 else 1, 12 if h2 else 11]
        rows.append(_row([head, [13] if s in removed else [3, 13], tail]))
    db = EdgeDB(rows, "tsr-probe-%d%s%s" % (N, "-" + dl if dl else "", "+%d" % len(extra) if extra else ""))
    db.N, db.m, db.deciding, db.second, db.removed, db.dl, db.edges = N, m, deciding, second, sorted(removed), dl, edges
    db.minconf = 0.0
    return db


def item_sid_masks(db):
    """{item: bool array over the sids} by definition."""
    lens = np.diff(db.seq_off)
    seq_of = np.repeat(np.arange(len(db.rows)), lens)
    out = {}
    for it in np.unique(db.tokens[db.tokens >= 0]):
        mk = np.zeros(len(db.rows), dtype=bool)
        mk[seq_of[db.tokens == it]] = True
        out[int(it)] = mk
    return out


def tsr_domain_sum(db, rules):
    """Sum over the rules of |sids(X u Y)| (the sequences holding every item of the rule, in any
    order): what the expansions of exactly these rules walk as their domains."""
    masks = item_sid_masks(db)
    memo, tot = {}, 0
    for r in rules:
        key = tuple(sorted(r[0] + r[1]))
        if key not in memo:
            mk = masks[key[0]].copy()
            for it in key[1:]:
                mk &= masks[it]
            memo[key] = int(mk.sum())
        tot += memo[key]
    return tot


def tsr_kid_edges(T, low, tight_kids):
    """tsr_long_rows(T) with every item value raised by `low`, plus (low > 0) eight filler
    sequences of ONE itemset holding the items 1 .. low: the fillers have support 8 like every
    other item (all are kept whatever the pair phase's threshold: K = low + 3 + T kids) and a
    single itemset yields no rule.  Dense kids: fillers 0 .. low - 1, the core items low,
    low + 1, low + 2, tail item j low + 3 + j.  `tight_kids` names the tight tail items by kid.
    lo_abs = min(max X, max Y) + 1 of the five core rules is low + 1 or low + 2."""
    tight = sorted(k - (low + 3) for k in tight_kids)
    assert all(0 <= j < T for j in tight), (T, low, tight_kids)
    base = tsr_long_rows(T, tight=tight)
    rows = [[t + low if t > 0 else t for t in r] for r in base.rows]
    if low:
        rows += [_row([list(range(1, low + 1))]) for _ in range(8)]
    db = EdgeDB(rows, "tsr-kids-%d-low%d" % (T, low))
    db.T, db.N, db.low, db.tight, db.tight_kids, db.K = T, 8, low, tight, sorted(tight_kids), low + 3 + T
    db.core = (low + 1, low + 2, low + 3)
    db.tail_item = lambda j: low + 10 + j
    db.minconf = 0.5
    return db


def kid_lo_abs(db, X, Y):
    """lo_abs of a rule by definition: the dense rank (kid, every item kept) of
    min(max X, max Y), plus one."""
    vals = sorted({t for r in db.rows for t in r if t >= 0})
    return vals.index(min(max(X), max(Y))) + 1


def tsr_chain(n, copies):
    """`copies` sequences <{1}, {2}, ..., {n}>, one that lacks item n, and two reversed ones
    (first and last sid), which are in every domain and hold no forward rule.  The forward rules
    X -> Y (max X < min Y) have support copies + 1 without item n and copies with it, the
    reversed ones 2; |X u Y| goes up to n."""
    fwd = _row([[i] for i in range(1, n + 1)])
    rev = _row([[i] for i in range(n, 0, -1)])
    h = copies // 2
    rows = [list(rev)] + [list(fwd) for _ in range(h)] + [_row([[i] for i in range(1, n)])]
    rows += [list(fwd) for _ in range(copies - h)] + [list(rev)]
    db = EdgeDB(rows, "tsr-chain-%d-%d" % (n, copies))
    db.n, db.copies, db.minconf = n, copies, 0.0
    return db


def pair_batch_starts(U):
    """First dense item id of every pair-phase batch after the first (16, 48, 112, 240, 496 ...:
    batches double from pair_batch0 up to 4,096 items while their candidates stay few)."""
    out, a, nb = [], 0, tsr_constants()["pair_batch0"]
    while a + nb < U:
        a += nb
        out.append(a)
        nb = min(2 * nb, 4096)
    return out


def tsr_pair_edges(U, m=4, starts=None, offs=(1, 63, 64, 65), seed=9):
    """U items (values 1 .. U, dense id = value - 1), every one in m single-item sequences of its
    own (support >= m: all are kept).  The only rules are the planted pairs i -> j and j -> i:
    i (dense) the last item of a pair-phase batch and the first of the next (`starts`, default
    pair_batch_starts(U)), j in {i + 1, i + 63, i + 64, i + 65, U - 1} (k_pairs_compact walks j
    from i + 1 in steps of 64 lanes).  Pair p has i -> j in a sequences <{i}, {j}> and j -> i in
    b sequences <{j}, {i}>, (a, b) cycling through (m, m - 1), (m - 1, m), (m, m),
    (m - 1, m - 1).  The sequences are shuffled (seeded), so every sid slice holds a mixture."""
    starts = pair_batch_starts(U) if starts is None else list(starts)
    ids = sorted({e - 1 for e in starts} | set(starts))
    pairs = []
    for i in ids:
        for j in [i + o for o in offs] + [U - 1]:
            if i < j < U and (i, j) not in pairs:
                pairs.append((i, j))
    rows, planted = [], {}
    for p, (i, j) in enumerate(pairs):
        a, b = ((m, m - 1), (m - 1, m), (m, m), (m - 1, m - 1))[p % 4]
        rows += [_row([[i + 1], [j + 1]]) for _ in range(a)] + [_row([[j + 1], [i + 1]]) for _ in range(b)]
        planted[((i + 1,), (j + 1,))] = a
        planted[((j + 1,), (i + 1,))] = b
    rows += [_row([[d + 1]]) for d in range(U) for _ in range(m)]
    random.Random(seed).shuffle(rows)
    db = EdgeDB(rows, "tsr-pairs-%d" % U)
    db.U, db.m, db.pairs, db.planted, db.starts, db.minconf = U, m, pairs, planted, starts, 0.0
    return db


# ---- case tables of tests/test_tsr_edges_gpu.py (tests/test_edge_dbs.py proves them on the CPU)
def tsr_all_rules(db, t=1):
    """oracle.tsr_all of a DB at threshold t and the DB's minconf, once per process."""
    def make():
        from oracle import oracle
        return oracle.tsr_all(db.seq_off, db.tokens, t, db.minconf)["rules"]
    return _cached(("tsr_all", id(db), t), make)


def tsr_modes(db):
    """[(mode, k, final minsup)]: exhaustive (k = every valid rule: final minsup 1) and tight
    (k = the rules with support >= m: the rules planted at m - 1 are left out)."""
    rules = tsr_all_rules(db)
    return [("exhaustive", len(rules), 1), ("tight", sum(1 for r in rules if r[2] >= db.m), db.m)]


def probe_sizes():
    return tuple(e + 1 for e in probe_edges()[1::2])


def shard_cuts(N):
    """The sids N r / R - 1 and N r / R at which the sharded pair phase cuts (R = 2, 3)."""
    return tuple(sorted({s for R in (2, 3) for r in range(1, R) for s in (N * r // R - 1, N * r // R)}))


def tsr_probe_cases():
    """{name: db}: family A.  N one past each rank-directory edge, and one group past the round
    edge; the k_dl variants (item 3 removed) at N = 8,193 and 65,537; and the DBs whose deciding
    sids include the shard cuts."""
    def make():
        sizes = probe_sizes()
        out = {"N%d" % N: tsr_probe_edges(N) for N in sizes}
        # one group past a block round of k_rank_dir: with N = 32,769 the only sid of the second round is a
        # hold row whose rank without the carry is sid 0's, a hold row too; here the fail rows 32,769 ..
        # 32,896 would read the entries of the sids 1 .. 128, three of them hold rows
        c = tsr_constants()
        N = c["rank_round"] + c["group"] + 1
        out["N%d" % N] = tsr_probe_edges(N)
        for N in (sizes[1], sizes[3]):
            for dl in ("and", "list"):
                out["N%d-dl-%s" % (N, dl)] = tsr_probe_edges(N, dl=dl)
            out["N%d-cuts" % N] = tsr_probe_edges(N, extra=shard_cuts(N))
        return out
    return _cached("tsr_probe", make)


def tsr_window_cases():
    """{name: db}: family B.  N on 1,023 .. 2,049 (domains of one, two and three windows, the
    last of 1,023, 1,024 or one row), and three DBs of 1,030 sequences whose big rules (2 -> 1:
    the N - m fail rows of triple 1) keep exactly 1,025, 1,024 and 1,023 rows for their children."""
    def make():
        w = tsr_constants()["exp_win"]
        we = window_edges()
        out = {"N%d" % N: tsr_probe_edges(N, edges=we) for N in (w - 1, w, w + 1, 2 * w, 2 * w + 1)}
        for n_extra in (0, 1, 2):
            db = tsr_probe_edges(w + 6, extra=(500, 700)[:n_extra], edges=we)
            out["plist%d" % (db.N - db.m)] = db
        return out
    return _cached("tsr_window", make)


def tsr_kid_cases():
    """{name: db}: family C.  low on kPassKids - 3 .. kPassKids - 1 with T = 4,200, and low = 0
    with T = 8,300; the tight tail kids on the pass edges, the first and last tail kid and the
    reduce-range edges of pass 1."""
    def make():
        c = tsr_constants()
        P, q = c["kPassKids"], c["reduce_range"]
        out = {}
        for low in (P - 3, P - 2, P - 1):
            T = 4200
            first, last = low + 3, low + 3 + T - 1
            kids = {k for k in (P - 1, P, P + 1) if k >= first} | {first, last, P + q - 1, P + q}
            out["low%d" % low] = tsr_kid_edges(T, low, sorted(kids))
        out["low0"] = tsr_kid_edges(8300, 0, [q - 1, q, P - 1, P, P + 1, 2 * P - 1, 2 * P])
        return out
    return _cached("tsr_kid", make)


def tsr_kid_modes(db):
    """[(mode, k, final minsup)] of a family C DB: k = 5 (the core rules, final minsup 8: a tight kid
    counted 8 adds a rule), and k = the two-item rules of support >= 7, which ends the pair phase at
    minsup 7 before the tail x tail pairs: the answer then holds rules of every tight tail item at
    exactly 7 (a tight kid counted 6 loses them).  A k that keeps the threshold lower costs the top-k
    restatement tens of seconds per DB."""
    k7 = sum(1 for r in tsr_all_rules(db, 7) if len(r[0]) + len(r[1]) == 2)
    return [("k5", 5, 8), ("pairs7", k7, 7)]


def tsr_chain_cases():
    """{name: (db, [(mode, k, final minsup)])}: family D.  n = 5, 9, 10 exhaustively, and n = 10
    with copies = kWideMinsup - 1 (forward rules at kWideMinsup, those with item n one below) at
    the two k that end the pair phase at kWideMinsup (k = the two-item rules at that support:
    wide batches) and at kWideMinsup - 1 (one more: the k-th two-item rule holds item n; the
    expansions then raise the minsup to kWideMinsup again).  Rules that tie the final minsup
    stay, so both answers are every rule at or above kWideMinsup."""
    def make():
        W = tsr_constants()["kWideMinsup"]
        out = {}
        for n in (5, 9, 10):
            db = tsr_chain(n, 6)
            db.m = 6
            out["n%d" % n] = (db, tsr_modes(db))
        db = tsr_chain(10, W - 1)
        at_w = sum(1 for r in tsr_all_rules(db) if len(r[0]) + len(r[1]) == 2 and r[2] >= W)
        out["n10-wide"] = (db, [("pairs-end-%d" % W, at_w, W), ("pairs-end-%d" % (W - 1), at_w + 1, W)])
        return out
    return _cached("tsr_chain", make)


def pair_phase_threshold(rules, k):
    """The minsup the pair phase ends at: the k-th largest support among the two-item rules
    (1 while fewer than k are known)."""
    sups = sorted((r[2] for r in rules if len(r[0]) + len(r[1]) == 2), reverse=True)
    return sups[k - 1] if len(sups) >= k else 1


def tsr_pair_case():
    return _cached("tsr_pair", lambda: tsr_pair_edges(600))


# ---------------------------------------------------------------- SPADE along the sequence axis
K0_SRC = os.path.join(ROOT, "spark-fsm_amd", "csrc", "k0_build.hip")
UTIL_SRC = os.path.join(ROOT, "spark-fsm_amd", "csrc", "device_util.hip")


def spade_constants():
    """The constants of spade_engine.hip (and the scan tile of device_util.hip) the tall DBs are
    placed on, read from the source itself (every one must be found): kF2MaxRows, kF2MaxBlocks,
    kChunk, the default of FSM_F2_BLOCKS and the lower bound of rpb in Miner::f2_geometry, and
    kScanTile = kScanT * kScanV."""
    def make():
        with open(ENGINE_SRC) as f:
            src = f.read()
        out = {}
        for name in ("kF2MaxRows", "kF2MaxBlocks", "kChunk"):
            m = re.search(r"^constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, src, re.M)
            assert m, "no constexpr %s in spade_engine.hip" % name
            out[name] = int(m.group(1))
        m = re.search(r'clamped\("FSM_F2_BLOCKS",\s*1,\s*kF2MaxBlocks,\s*(\d+)\)', src)
        assert m, "no default of FSM_F2_BLOCKS in spade_engine.hip"
        out["f2_blocks"] = int(m.group(1))
        m = re.search(r"g\.rpb\s*=\s*std::min<uint32_t>\(kF2MaxRows,\s*std::max<uint32_t>\((\d+)u,\s*"
                      r"\(g\.R \+ nb_want - 1\) / nb_want\)\);", src)
        assert m, "Miner::f2_geometry no longer derives rpb as min(kF2MaxRows, max(16, ceil(R / blocks)))"
        out["rpb_min"] = int(m.group(1))
        assert re.search(r"g\.nblk\s*=\s*\(g\.R \+ g\.rpb - 1\) / g\.rpb;", src), "nblk is no longer ceil(R / rpb)"
        with open(UTIL_SRC) as f:
            util = f.read()
        t = re.search(r"^constexpr\s+int\s+kScanT\s*=\s*(\d+)\s*;", util, re.M)
        v = re.search(r"^constexpr\s+int\s+kScanV\s*=\s*(\d+)\s*;", util, re.M)
        assert t and v and re.search(r"kScanTile\s*=\s*kScanT\s*\*\s*kScanV\s*;", util), "no kScanTile in device_util.hip"
        out["kScanTile"] = int(t.group(1)) * int(v.group(1))
        return out
    return dict(_cached("spade_constants", make))


def f2_row_blocks(R, f2_blocks=None):
    """(rpb, nblk) of the root F2 as Miner::f2_geometry derives them for R rows under
    FSM_F2_BLOCKS = f2_blocks (None: the default), or None where the group path does not apply
    (more rows than kF2MaxBlocks blocks of rpb rows cover)."""
    c = spade_constants()
    want = min(c["f2_blocks"] if f2_blocks is None else f2_blocks, c["kF2MaxBlocks"])
    rpb = min(c["kF2MaxRows"], max(c["rpb_min"], -(-R // want)))
    if rpb * c["kF2MaxBlocks"] < R:
        return None
    return rpb, -(-R // rpb)


def policy_name(pol):
    return pol[0] if len(pol) == 1 else "%s(%d)" % pol


def tall_policy_rows(R, pol):
    """(critical rows, critical row c) of a policy whose rows do not depend on S, or None where
    the policy has no row at this R (edges and lone need a second block).  Blocks are the B rows
    [k B, (k + 1) B), the last one partial."""
    kind = pol[0]
    if kind == "dense":
        return list(range(R)), R - 1
    if kind in ("head", "tail"):
        return [], 0 if kind == "head" else R - 1
    B = pol[1]
    nb = -(-R // B)
    if kind == "every":
        rows = {0, R - 1}
        for k in range(nb):
            rows.add(min(R, (k + 1) * B) - 1 if k % 2 else k * B)
        return sorted(rows), R - 1
    if nb < 2:
        return None
    if kind == "edges":
        return sorted({r for k in range(1, nb) for r in (k * B - 1, k * B)}), (nb - 1) * B
    assert kind == "lone"
    first = (nb - 1) * B
    c = first + (R - first) // 2
    return [c], c


TALL_MIN_S = 8
# the slots (itemsets after the prefix) of a placement's gadgets, in the two layouts a placement's
# rows alternate between: the gadgets in this order, and in the reverse order
_TALL_ORDER = (("F", 1), ("T+", 2), ("T-", 2), ("E+", 1), ("E-", 1), ("C+", 3), ("C-", 3))
TALL_SLOTS = sum(n for _, n in _TALL_ORDER)
TALL_ITEMS = 16


def _tall_slot_maps():
    maps = []
    for order in (_TALL_ORDER, _TALL_ORDER[::-1]):
        at, s = {}, 0
        for g, n in order:
            at[g] = s
            s += n
        maps.append(at)
    return maps


class TallSpade(EdgeDB):
    """tall_spade's result.
    S            the minsup the DB is mined at; `support` the relative support that gives it
    placements   {policy label: sorted rows of P}, crit {policy label: critical row c}
    items        {policy label: {"f", "g", "x", "y", "u", "v", "p", "q", "p2", "q2", "cx", "cy", "cz", "dx",
                 "dy", "dz": item}}: F1+ f, F1- g, T+ x -> y, T- u -> v, E+ (p q), E- (p2 q2),
                 C+ cx -> cy -> cz, C- dx -> dy -> dz
    t2, t1       the decisions of support exactly S / exactly S - 1; policy_of, gadget {decision: label}
    member       per row: the number of placements it belongs to"""

    @property
    def support(self):
        return 1.0 if self.S == len(self.rows) else (self.S - 0.5) / len(self.rows)

    def where(self, p):
        pol = self.policy_of[p]
        return "R = %d, policy %s, critical row %d, gadget %s" % (len(self.rows), pol, self.crit[pol], self.gadget[p])

    def root_entries(self):
        """(frequent item, sequence) entries of the root class: every item but the F1- ones."""
        rare = {it["g"] for it in self.items.values()}
        return int(np.count_nonzero((self.tokens >= 0) & ~np.isin(self.tokens, list(rare))))


def tall_spade(R, S, policies, prefix=1, seed=1):
    """R short sequences mined at minsup S (None: the most rows any policy needs, at least
    TALL_MIN_S).  Every row starts with the one-item itemsets A1 .. Ad (d = prefix, items 1 .. d), so
    every row holds a frequent entry and R is the engine's row count.

    For each policy (tall_policy_rows; head is rows 0 .. S - 1, tail R - S .. R - 1) a placement P
    of exactly S rows: the policy's critical rows, padded with seeded-random others (rows that are
    critical to no policy first; for `lone`, rows outside the last block), and ONE critical row c
    in P.  Sixteen fresh items per placement, each in no row outside P, plant the gadgets:

    F1+  f in every row of P                                   support S
    F1-  g in P without c                                      S - 1
    T+   x -> y in every row                                   S
    T-   u -> v in P without c, v -> u in c                    u, v: S; u -> v: S - 1
    E+   (p q) in every row                                    S
    E-   (p2 q2) in P without c; in c p2 and q2 in neighbouring itemsets      p2, q2: S; (p2 q2): S - 1
    C+   cx -> cy -> cz in every row                           S, through the parents cx -> cy and cx -> cz at S
    C-   dx -> dy -> dz in P without c, dx -> dz -> dy in c    dx -> dy, dx -> dz: S; the chain: S - 1

    A lost increment at c, or anywhere in P, turns an S into S - 1; a repeated one an S - 1 into S.
    With the prefix every decision repeats behind every sub-chain of A1 .. Ad (one and two classes
    down).  The gadgets of a placement take TALL_SLOTS itemsets in a fixed order in the even rows
    of P and in the reverse order in the odd ones, so a pattern over two gadgets holds in about
    half of P and stays below S; a row of several placements merges their itemsets slot by slot
    (two placements share fewer than S rows).  A row of m placements has at most
    16 m + TALL_SLOTS + 2 d + 1 tokens: at most 64 for m <= 2 (and for m = 3 with d = 1); the few
    rows that more placements share are longer.  Rows of no placement hold the prefix alone."""
    rng = random.Random(seed)
    d = prefix
    pols = []
    for pol in policies:
        got = tall_policy_rows(R, pol)
        if got is not None:
            pols.append((policy_name(pol), pol, got[0], got[1]))
    if S is None:
        S = max([TALL_MIN_S] + [len(rows) for _, _, rows, _ in pols])
    assert 2 <= S <= R and all(len(rows) <= S for _, _, rows, _ in pols)
    in_crit = set(r for _, _, rows, _ in pols for r in rows)
    placements, crit = {}, {}
    for label, pol, rows, c in pols:
        if pol[0] == "head":
            rows = list(range(S))
        elif pol[0] == "tail":
            rows = list(range(R - S, R))
        have = set(rows)
        if len(rows) < S:
            limit = (-(-R // pol[1]) - 1) * pol[1] if pol[0] == "lone" else R
            cand = [r for r in range(limit) if r not in have]
            rng.shuffle(cand)
            cand.sort(key=lambda r: r in in_crit)  # stable: rows critical to no policy first
            rows = rows + cand[:S - len(rows)]
        assert len(set(rows)) == S and c in rows, label
        placements[label], crit[label] = sorted(rows), c
    assert len({tuple(p) for p in placements.values()}) == len(placements), "two policies with the same placement"

    maps = _tall_slot_maps()
    slots = {}  # row -> TALL_SLOTS item lists
    items, member = {}, np.zeros(R, dtype=np.int32)
    t2, t1, policy_of, gadget = [], [], {}, {}
    chains = [tuple((a,) for a in range(1, d + 1) if bits >> (a - 1) & 1) for bits in range(1 << d)]
    for j, (label, P) in enumerate(placements.items()):
        base = d + 1 + TALL_ITEMS * j
        names = ("f", "g", "x", "y", "u", "v", "p", "q", "p2", "q2", "cx", "cy", "cz", "dx", "dy", "dz")
        it = items[label] = {n: base + k for k, n in enumerate(names)}
        c = crit[label]
        for k, r in enumerate(P):
            at = maps[k & 1]
            sl = slots.setdefault(r, [[] for _ in range(TALL_SLOTS)])
            member[r] += 1
            isc = r == c

            def put(g, off, name):
                sl[at[g] + off].append(it[name])
            put("F", 0, "f")
            if not isc:
                put("F", 0, "g")
            put("T+", 0, "x"), put("T+", 1, "y")
            put("T-", 1 if isc else 0, "u"), put("T-", 0 if isc else 1, "v")
            put("E+", 0, "p"), put("E+", 0, "q")
            put("E-", 0, "p2")
            if isc:  # the itemset behind E-'s own: the next gadget's first, or one of this row's own
                nxt = at["E-"] + 1
                assert nxt < TALL_SLOTS
                sl[nxt].append(it["q2"])
            else:
                put("E-", 0, "q2")
            put("C+", 0, "cx"), put("C+", 1, "cy"), put("C+", 2, "cz")
            put("C-", 0, "dx"), put("C-", 2 if isc else 1, "dy"), put("C-", 1 if isc else 2, "dz")
        hold = [("F1+", ((it["f"],),)), ("T+", ((it["x"],), (it["y"],))), ("E+", ((it["p"], it["q"]),)),
                ("C+", ((it["cx"],), (it["cy"],), (it["cz"],))),
                ("C+ parent", ((it["cx"],), (it["cy"],))), ("C+ parent", ((it["cx"],), (it["cz"],))),
                ("C- parent", ((it["dx"],), (it["dy"],))), ("C- parent", ((it["dx"],), (it["dz"],)))]
        hold += [("%s item" % g, ((it[n],),)) for g, n in (("T-", "u"), ("T-", "v"), ("E-", "p2"), ("E-", "q2"))]
        fail = [("F1-", ((it["g"],),)), ("T-", ((it["u"],), (it["v"],))), ("E-", ((it["p2"], it["q2"]),)),
                ("C-", ((it["dx"],), (it["dy"],), (it["dz"],)))]
        for ch in chains:
            for lst, dec in ((t2, hold), (t1, fail)):
                for g, p in dec:
                    q = ch + p
                    lst.append(q)
                    policy_of[q], gadget[q] = label, g if not ch else "%s behind %d prefix item(s)" % (g, len(ch))
    pre = [t for a in range(1, d + 1) for t in (a, -1)]
    plain = pre + [-2]
    rows = [plain] * R
    for r, sl in slots.items():
        rows[r] = pre + _row([sorted(s) for s in sl if s])
    db = TallSpade(rows, "tall-R%d-S%d-%s" % (R, S, "+".join(placements)))
    db.S, db.R, db.prefix_items, db.placements, db.crit, db.items = S, R, list(range(1, d + 1)), placements, crit, items
    db.t2, db.t1, db.policy_of, db.gadget, db.member = t2, t1, policy_of, gadget, member
    return db


# FSM_F2_BLOCKS (None: the default) and the R of each tall DB; TALL_GEOMETRY is what the issue
# states for them, asserted against f2_row_blocks in tests/test_edge_dbs.py
TALL_R = ((None, (15, 16, 17)), (None, (16383, 16384, 16385)), (None, (65535, 65536, 65537)),
          (1, (4095, 4096, 4097)), (2048, (32767, 32768, 32769)))
TALL_GEOMETRY = {15: (16, 1), 16: (16, 1), 17: (16, 2), 16383: (16, 1024), 16384: (16, 1024), 16385: (17, 964),
                 65535: (64, 1024), 65536: (64, 1024), 65537: (65, 1009), 4095: (4095, 1), 4096: (4096, 1),
                 4097: (4096, 2), 32767: (16, 2048), 32768: (16, 2048), 32769: (17, 1928)}
TALL_PREFIX2 = (16, 4097, 65536)  # these R carry two prefix items (decisions two classes down)
TALL_MATRIX_R = (4097, 16385)
TALL_NEAR_R = 65537


def tall_blocks_env(R):
    """The FSM_F2_BLOCKS a tall DB of R rows is placed for (None: the default)."""
    return [b for b, rs in TALL_R if R in rs][0]


def tall_env(R):
    b = tall_blocks_env(R)
    return "" if b is None else "FSM_F2_BLOCKS=%d" % b


def tall_case(R, dense=False):
    """The tall DB of R rows: every(B), edges(B), lone(B) for B = the root F2's rpb at this R and
    its FSM_F2_BLOCKS and for B = 64 (the wave and tile sizes; without edges(64) where rpb divides
    64), head and tail, all in one DB at the S the largest of them needs; dense: the DB with S = R, every row in P, c = R - 1."""
    def make():
        d = 2 if R in TALL_PREFIX2 else 1
        if dense == "near":  # a minsup just below 2^16 under counts above it, three classes down
            return tall_spade(R, R - 2, [("head",)], prefix=3, seed=R)
        if dense:
            return tall_spade(R, R, [("dense",)], prefix=d, seed=R)
        rpb, _ = f2_row_blocks(R, tall_blocks_env(R))
        pols = [(kind, rpb) for kind in ("every", "edges", "lone")]
        if rpb != 64:  # where rpb divides 64 every row of edges(64) is a row of edges(rpb) already
            pols += [(kind, 64) for kind in ("every", "edges", "lone") if kind != "edges" or 64 % rpb]
        pols += [("head",), ("tail",)]
        return tall_spade(R, None, pols, prefix=d, seed=R)
    return _cached(("tall", R, dense), make)


def tall_all_r():
    return [R for _, rs in TALL_R for R in rs]


# ---------------------------------------------------------------- K0 and the scan on the same sizes
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
K0_TALL_R = (4095, 4096, 4097, 32767, 32768, 32769)
K0_STAGE_R = (524287, 524288, 524289)
K0_STAGE_VARIANTS = ("last-max", "last-min", "first")
K0_LEAD = (INT32_MAX, -1, 0, -1, 7)  # tokens before seq_off[0]: they belong to no row


def k0_stage_constants():
    """k0_build.hip's kStageBytes, kK0Wave, kK0Long, kK0Threads and the grid cap of k0_rows, read from the source."""
    def make():
        with open(K0_SRC) as f:
            src = f.read()
        out = {}
        m = re.search(r"^constexpr\s+uint64_t\s+kStageBytes\s*=\s*uint64_t\((\d+)\)\s*<<\s*(\d+)\s*;", src, re.M)
        assert m, "no kStageBytes in k0_build.hip"
        out["kStageBytes"] = int(m.group(1)) << int(m.group(2))
        for name in ("kK0Wave", "kK0Long", "kK0Threads"):
            m = re.search(r"^constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, src, re.M)
            assert m, "no %s in k0_build.hip" % name
            out[name] = int(m.group(1))
        m = re.search(r"grid_rows\s*=.*kK0Threads - 1\) / kK0Threads,\s*(\d+)\)\);", src)
        assert m, "no grid cap of k0_rows in k0_build.hip"
        out["rows_grid"] = int(m.group(1))
        out["rows_lap"] = out["rows_grid"] * out["kK0Threads"] // 64  # waves (rows) per grid-stride lap
        return out
    return dict(_cached("k0_constants", make))


def k0_extreme_cases():
    """(name, rows, modes): item values within 2^20 of INT32_MAX and of INT32_MIN (the extremes
    themselves included, and repeated within a row), on the wave path (a row of exactly 64 tokens
    and 32 itemsets) and on the block path (a row of 8,192 tokens).  The sort key of an item is
    value ^ 0x80000000 over its eid: for INT32_MAX its high word is all ones, as in the sentinel
    key of a lane without an item.  Negative values are items in SPADE only."""
    def make():
        rng = random.Random(9)
        out = []
        for side, lo, hi, modes in (("max", INT32_MAX - 2 ** 20, INT32_MAX, ("spade", "tsr")),
                                    ("min", INT32_MIN, INT32_MIN + 2 ** 20, ("spade",))):
            ends = (lo, hi, hi - 1, lo + 1)
            for path, sets in (("wave", 32), ("block", 4096)):
                vals = [ends[k % 4] if k % 5 == 0 or k == sets - 1 else rng.randint(lo, hi) for k in range(sets)]
                vals[-1] = hi if side == "max" else lo  # the extreme in the last itemset too
                row = [t for v in vals for t in (v, -1)]
                out.append(("int32-%s-%s" % (side, path), [row, [hi, -1, lo, -1], [lo, hi, -1, -2]], modes))
        return out
    return _cached("k0_extreme", make)


def k0_stage_case(R, variant):
    """R rows <x, -1> as token arrays (sids, seq_off, tokens), and their image in closed form (one
    entry per row at eid / itemset 0; `mode` picks the fields).  The n + 1 offsets and the 2 R
    tokens end on both sides of one staging chunk.  x is 100 + r % 1,000 except for the smallest
    (7) and the largest (5,000) value: last-max / last-min put one of them in the last row alone
    (the row of the last two tokens: at R = 524,289 a chunk of its own), `first` puts them in rows
    0 and 1."""
    x = 100 + np.arange(R, dtype=np.int64) % 1000
    if variant == "last-max":
        x[-1] = 5000
    elif variant == "last-min":
        x[-1] = 7
    else:
        assert variant == "first"
        x[0], x[1] = 7, 5000
    tokens = np.empty(2 * R, dtype=np.int64)
    tokens[0::2], tokens[1::2] = x, -1
    vals = np.unique(x)

    def image(mode):
        img = {"rows": R, "entries": R, "items": len(vals), "row_off": np.arange(R + 1, dtype=np.uint32),
               "item": np.searchsorted(vals, x).astype(np.uint32), "item_val": vals.astype(np.int32)}
        if mode == "spade":
            img.update(mask_words=1, max_occ=1, mask=np.ones(R, dtype=np.uint64))
        else:
            img.update(first=np.zeros(R, dtype=np.uint32), last=np.zeros(R, dtype=np.uint32))
        return img
    return np.arange(R, dtype=np.int32), 2 * np.arange(R + 1, dtype=np.int64), tokens, image


def with_lead(db, lead=K0_LEAD):
    """(seq_off, tokens) of a DB with `lead` tokens in front that belong to no row: seq_off[0] = len(lead)."""
    return db.seq_off + len(lead), np.concatenate([np.array(lead, dtype=np.int64), db.tokens])
