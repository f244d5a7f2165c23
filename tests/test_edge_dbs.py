"""CPU tests of tests/edge_dbs.py: the threshold-tight families mean what they
claim, so tests/test_edges_gpu.py and tests/test_tsr_edges_gpu.py are sensitive
to a count that is off by one.  No GPU.

For every family: at its small sizes the oracle's answer against the
definitional enumerator (oracle/brute.py); at every size the GPU tests use,
the tightness claim itself, re-counted by definition (oracle.pattern_support /
oracle.rule_support): every selected relation exactly at the threshold, a
sample of the rest (first, last and middle ranks included) exactly one below;
and the geometry each case is named after."""
import math

import numpy as np
import pytest

import edge_dbs as E
from oracle import brute, oracle


def psup(db, p):
    return oracle.pattern_support(db.seq_off, db.tokens, p)


def assert_tight_hubs(db, minsup=2):
    """Selected relations at minsup, sampled other pairs of each hub one below;
    behind every sub-chain of the prefix as well."""
    chains = [()] + [tuple((a,) for a in db.prefix_items[:k]) for k in range(1, len(db.prefix_items) + 1)]
    for c in chains:
        for p in db.selected:
            assert psup(db, c + p) == minsup, (c, p)
        for h, pairs in enumerate(db.rest_sample):
            for a, b in pairs:
                p = E.relation(db, h, a, b)
                assert p not in db.selected
                assert psup(db, c + p) == minsup - 1, (c, h, a, b)
    for h, items in enumerate(db.hub_items):  # no triple of hub items reaches the threshold
        for p in db.selected:
            if len(p) == 2 and p[0][0] in items and len(items) > 2:
                z = next(i for i in items if (i,) not in p)
                assert psup(db, p + ((z,),)) < minsup and psup(db, ((z,),) + p) < minsup


# ------------------------------------------------------------ brute, small sizes
@pytest.mark.parametrize("kw", [
    dict(lengths=[1, 2, 3], per_set=1), dict(lengths=[4, 6], per_set=3), dict(lengths=[5, 6], per_set=2, prefix=1),
    dict(lengths=[4, 6], per_set=2, prefix=1, dup=True, noise=2), dict(lengths=[6], per_set=1, lead=3, hub_last=True),
], ids=str)
def test_tight_spade_small_vs_brute(kw):
    db = E.tight_spade(**kw)
    o = oracle.spade(db.records(), db.support)
    assert o["minsup"] == 2
    assert o["patterns"] == brute.brute_spade(db.records(), db.support) == db.expected()
    assert_tight_hubs(db)


def test_wide_mask_small_vs_brute():
    for e in (3, 5, 66):
        db = E.wide_mask_db(e)
        o = oracle.spade(db.records(), db.support)
        assert o["minsup"] == 2 and o["patterns"] == brute.brute_spade(db.records(), db.support) == db.expected()


@pytest.mark.parametrize("N", [8, 31, 32, 33, 40])
def test_tsr_sid_edges_small_vs_brute(N):
    db = E.tsr_sid_edges(N)
    recs = db.records()
    valid = brute.brute_tsr_valid(recs, 0.0)
    for k in (1, 2):
        o = oracle.tsr(recs, k, 0.0)
        brute.check_tsr(o["rules"], valid, k)
        assert [r[:2] for r in o["rules"]] == [((1,), (2,)), ((3,), (4,))][:k]


@pytest.mark.parametrize("T", [2, 5, 6])
def test_tsr_long_rows_small_vs_brute(T):
    db = E.tsr_long_rows(T, tight=(0, T - 1))
    recs = db.records()
    o = oracle.tsr(recs, 5, 0.5)
    brute.check_tsr(o["rules"], brute.brute_tsr_valid(recs, 0.5), 5)
    assert o["final_minsup"] == 8 and len(o["rules"]) == 5


# ------------------------------------------------------------ tightness, GPU sizes
def test_f2_cases_tight_and_row_lengths():
    for name, db, row_len in E.f2_cases():
        assert oracle.spade_tokens(db.seq_off, db.tokens, db.support)["patterns"] == db.expected(), name
        assert_tight_hubs(db)
        g = E.geometry(db.rows, 2, classes=False)
        for h, n in row_len.items():
            assert E.hub_run(db, g, h, "db")[1] == n
            assert E.hub_run(db, g, h, 0)[1] == len(db.hub_items[h])
        assert g["E_root"] == db.root_entries()
    # the row lengths sit on k_f2_tri's branches: folded (n + 1 <= 64), unfolded (n = 64), rows over 64
    lens = set(E.F2_LENGTHS)
    assert {63, 64, 65} <= lens and any(n % 2 for n in lens) and any(n % 2 == 0 for n in lens)
    noise = dict((n, d) for n, d, _ in E.f2_cases())["noise"]
    assert any(len(noise.hub_items[h]) <= 64 < E.hub_run(noise, E.geometry(noise.rows, 2, classes=False), h, "db")[1]
               for h in range(len(noise.hub_rows)))


@pytest.mark.parametrize("w", [1, 2, 4, 8])
def test_lattice_cases_tight_and_placed(w):
    rg = E.wave_ranges()
    assert all(v > 0 and v % 64 == 0 for v in rg.values())
    starts = {0: set(), 1: set()}
    for name, db, level, claim in E.lattice_cases(w):
        assert E.mask_width(db) == w, name
        E.check_lattice_claim(db, level, claim)
        if w > 2:  # stretched hubs: exactly 64 w itemsets, the hub's own from right behind the prefix to the last
            for h, r in enumerate(db.hub_rows):
                sets, own = E.itemsets_of(db.rows[r]), set(db.hub_items[h])
                at = [k for k, s in enumerate(sets) if own & set(s)]
                assert len(sets) == 64 * w and at[0] == 2 and at[-1] == 64 * w - 1, name
                assert {k >> 6 for k in at} == set(range(w)), name
        if "start" in claim:
            starts[level].add(claim["start"])
        if name == "lengths" or name.endswith(("start64", "start511", "start512")) or name == "hub-last":
            assert oracle.spade_tokens(db.seq_off, db.tokens, db.support)["patterns"] == db.expected(), name
            assert_tight_hubs(db)
    # a 64-entry run starting 63 before, one before and on every wave range boundary up to 512
    for level, key in ((1, "lattice" if w == 1 else "lattice_w"), (1, "count2")) + (((0, "root"),) if w == 1 else ()):
        r = rg[key]
        for m in range(r, 513, r):
            assert {m - 63, m - 1, m} <= starts[level], (key, m)


def test_rk_cases_sizes():
    for name, db, f_root, f_l1 in E.rk_cases():
        if f_root > 5000:
            continue  # (16,385 rows: checked in closed form below, the oracle takes seconds)
        o = oracle.spade_tokens(db.seq_off, db.tokens, db.support)
        assert o["patterns"] == db.expected(), name
        assert sum(1 for p, _ in o["patterns"] if len(p) == 1 and len(p[0]) == 1) == f_root
        assert sum(1 for p, _ in o["patterns"] if sum(len(s) for s in p) == 2) == f_l1
    sizes = {f for _, _, f, _ in E.rk_cases()} | {f for _, _, _, f in E.rk_cases()}
    assert set(E.RK_SIZES) | {E.FREQ_RECS_ROWS} <= sizes
    big = [db for n, db, _, _ in E.rk_cases() if n == "root-%d" % E.FREQ_RECS_ROWS][0]
    assert len(big.singles) + len(big.prefix_items) == E.FREQ_RECS_ROWS
    assert_tight_hubs(big)


@pytest.mark.parametrize("F,seed", [(300, 7), (2049, 7), (1500, 16385)])
def test_closed_form_ref_vs_oracle(F, seed):
    """The closed form the largest GPU cases are compared with (patterns and joins) equals the
    oracle's mine at sizes it takes quickly, with the hub structures (seeds) of those cases."""
    db = E.tight_spade([5], per_set=2, prefix=1, filler=F - 6, seed=seed)
    o = oracle.spade_tokens(db.seq_off, db.tokens, db.support)
    ref = E.closed_form_ref(db)
    assert o["patterns"] == ref["patterns"] and o["joins"] == ref["joins"] and o["minsup"] == 2


def test_one_row_group_cases_sizes():
    for F, db in E.one_row_group_cases():
        assert len(db.singles) + len(db.prefix_items) == F and len(db.expected()) == 2 * (F - 1 + len(db.selected)) + 1
        assert_tight_hubs(db)
    assert 2 * 8192 * 2 <= 32768 < 2 * 8193 * 2 and 2 * 16384 <= 32768 < 2 * 16385


def test_mask_and_big_row_cases_tight():
    for Ee, W, db in E.mask_cases():
        assert E.mask_width(db) == W
        sets = [s for s in E.itemsets_of(db.rows[db.big_row]) if s]
        assert len(sets) == Ee and sorted(db.planted_at.values())[0] == 0 and max(db.planted_at.values()) == Ee - 1
        if Ee == 4096:
            assert len(db.rows[db.big_row]) == 8192
        for p in db.selected:
            assert psup(db, p) == 2
        for x, y in db.rest_pairs:
            assert psup(db, E.planted_relation(db, x, y)) == 1
        assert db.rest_pairs
    for n, db in E.big_row_cases():
        assert len({t for t in db.rows[db.big_row] if t >= 0}) == n and E.mask_width(db) == 1
        assert oracle.spade_tokens(db.seq_off, db.tokens, db.support)["patterns"] == db.expected()
        for p in db.selected:
            assert psup(db, p) == 2
        for x, y in db.rest_pairs:
            assert psup(db, E.planted_relation(db, x, y)) == 1


# ------------------------------------------------------------ word sweep
SWEEP_LABELS = {"G1a", "G1b", "G1c", "G2a", "G2b", "G3", "G4", "G5a", "G5b", "G6a", "G6b", "G7", "G8", "G9a", "G9b"}


def assert_sweep_tight(db, frequent):
    """Every t2 decision at exactly 2, every t1 decision at exactly 1, re-counted by definition;
    both prefix-class parents of every decision frequent at exactly 2 (`frequent`: the oracle's
    mine as a dict)."""
    assert db.t2 and db.t1 and not set(db.t2) & set(db.t1)
    for want, pats in ((2, db.t2), (1, db.t1)):
        for p in pats:
            assert psup(db, p) == want, (db.name, db.boundary[p], db.gadget[p], p)
            assert (p in frequent) == (want == 2)
            for parent in E.prefix_parents(p):
                assert frequent.get(parent) == 2, (db.name, db.boundary[p], db.gadget[p], parent)


@pytest.mark.parametrize("W,Ee,ks", [(2, 70, None), (2, 128, None), (4, 256, (1, 3)), (4, 200, (2, 3))], ids=str)
def test_word_sweep_small_vs_brute(W, Ee, ks):
    db = E.word_sweep_db(W, ks, Ee)
    o = oracle.spade(db.records(), db.support)
    assert o["minsup"] == 2 and E.mask_width(db) == W
    assert o["patterns"] == brute.brute_spade(db.records(), db.support) == db.expected()
    assert_sweep_tight(db, dict(o["patterns"]))
    # S ends right after the boundary: the gadgets that need eid b + 2 are left out, the rest stays
    if Ee == 70:
        assert {db.gadget[p] for p in db.t2 + db.t1} == SWEEP_LABELS - {"G8"}
        cut = E.word_sweep_db(2, E=65)
        assert {cut.gadget[p] for p in cut.t2 + cut.t1} == SWEEP_LABELS - {"G4", "G5b", "G6b", "G7", "G8"}
        assert_sweep_tight(cut, dict(oracle.spade(cut.records(), cut.support)["patterns"]))


@pytest.mark.parametrize("W", E.SWEEP_W)
def test_word_sweep_cases_tight_and_placed(W):
    """The DBs of test_mask_word_sweep: the mask width, the boundaries each case claims (every
    one at the register-held widths; 1, 2, 63, 64, 65, W / 2 - 1, W / 2 and W - 1 at the runtime
    widths), every gadget at every boundary, every decision exactly on its threshold through
    tight parents, and the generator's closed form equal to the oracle's mine."""
    db = E.sweep_case(W)
    assert E.mask_width(db) == W == db.W and db.E == 64 * W
    assert len([s for s in E.itemsets_of(db.rows[0]) if s]) == 64 * W
    want = set(range(1, W)) if W <= 64 else {1, 2, 63, 64, 65, W // 2 - 1, W // 2, W - 1}
    assert set(db.ks) == want == set(db.boundary.values())
    for k in want:
        labels = {db.gadget[p] for p in db.t2 + db.t1 if db.boundary[p] == k}
        assert labels == SWEEP_LABELS - ({"G8"} if k == W - 1 else set()), (W, k)
    o = oracle.spade_tokens(db.seq_off, db.tokens, db.support)
    assert o["minsup"] == 2 and o["patterns"] == db.expected()
    assert_sweep_tight(db, dict(o["patterns"]))
    # the eids the gadgets are named after: a decision of boundary k has an item on eid 64 k - 1 or 64 k
    for p, k in db.boundary.items():
        es = {e for s in p for it in s for e in db.eids[it]}
        assert es & {64 * k - 1, 64 * k} and max(es) <= 64 * (k + 1), (W, k, db.gadget[p])


def test_word_sweep_off_threshold_is_noticed():
    """A second private sequence for one gadget moves its decision off the threshold: the
    tightness assertions trip."""
    db = E.word_sweep_db(2)
    moved = E.EdgeDB(db.rows + [db.rows[1 + len(db.t2)]])
    moved.t2, moved.t1, moved.boundary, moved.gadget, moved.name = db.t2, db.t1, db.boundary, db.gadget, "moved"
    o = oracle.spade_tokens(moved.seq_off, moved.tokens, 1.5 / len(moved.rows))
    assert o["minsup"] == 2
    with pytest.raises(AssertionError):
        assert_sweep_tight(moved, dict(o["patterns"]))
    assert psup(moved, db.t1[0]) == 2


def test_tsr_long_cases_tight():
    for name, db, k, mc in E.tsr_long_cases():
        o = oracle.tsr(db.records(), k, mc)
        assert o["final_minsup"] == 8 and [r[2] for r in o["rules"]][-5:] == [8] * 5, name
        assert len(o["rules"]) == (6 if name == "mixed" else 5)
        T = db.T
        for j in db.tight:  # one below the final minsup
            for y in (2, 3):
                assert oracle.rule_support(db.seq_off, db.tokens, [10 + j], [y])[0] == 7
        for j in (1, T // 2 + 1, T - 2):  # a non-tight tail item: half of the long rows
            assert oracle.rule_support(db.seq_off, db.tokens, [10 + j], [2])[0] == 4
            assert oracle.rule_support(db.seq_off, db.tokens, [1], [10 + j])[0] == 4
        # the long rows keep more than one chunk (4,096 entries) past the rule's items
        long_rows = [r for r in db.rows if len({t for t in r if t >= 10}) == T]
        assert len(long_rows) == db.N == 8


def test_tsr_sid_cases_tight():
    for N, db in E.tsr_sid_cases():
        m = len(db.deciding)
        assert db.deciding[-1] == N - 1 and all(e in db.deciding for e in E.SID_EDGES if e < N)
        assert oracle.rule_support(db.seq_off, db.tokens, [1], [2]) == (m, m)
        assert oracle.rule_support(db.seq_off, db.tokens, [3], [4])[0] == m - 1
        o = oracle.tsr(db.records(), 1, 0.0)
        assert [r[:3] for r in o["rules"]] == [((1,), (2,), m)] and o["final_minsup"] == m
    for L in (65535, 65536):
        db = E.tsr_deep_index(L)
        assert len(E.itemsets_of(db.rows[0])) == L + 1
        assert oracle.rule_support(db.seq_off, db.tokens, [1], [2])[0] == 3


# ------------------------------------------------------------ K0 image by definition
def test_k0_image_small_known_answer():
    rows = [[3, 1, -1, -1, 1, -1, 9, -2], [], [7, -1, 3, 3, -1]]
    s = E.k0_image(rows, "spade")
    assert s["row_off"].tolist() == [0, 2, 2, 4] and s["item_val"].tolist() == [1, 3, 7]
    assert s["item"].tolist() == [0, 1, 1, 2] and s["mask"].tolist() == [3, 1, 2, 1]
    assert s["mask_words"] == 1 and s["max_occ"] == 3
    t = E.k0_image(rows, "tsr")
    assert t["first"].tolist() == [0, 0, 1, 0] and t["last"].tolist() == [2, 0, 1, 0]
    names = [c[0] for c in E.k0_cases()]
    assert {"tokens-64", "tokens-65", "tokens-8192", "tokens-8193", "eids-4096", "eids-4097"} <= set(names)
    for name, rows, modes, dev in E.k0_cases():
        if name.startswith("eids-"):
            assert E.k0_image(rows, "spade")["mask_words"] == (64 if dev else 128)


# ------------------------------------------------------------ TSR families on the expansion kernels' constants
def rsup(db, X, Y):
    return oracle.rule_support(db.seq_off, db.tokens, list(X), list(Y))


def assert_modes(db, modes):
    """oracle.tsr at each mode's k returns exactly the rules of tsr_all at or above the mode's
    final minsup (every valid rule in exhaustive mode), and ends at that minsup."""
    allr = E.tsr_all_rules(db)
    for mode, k, final in modes:
        o = oracle.tsr(db.records(), k, db.minconf)
        assert o["final_minsup"] == final, (db.name, mode)
        assert o["rules"] == [r for r in allr if r[2] >= final], (db.name, mode)


def holds_at(db, X, Y):
    """The sids where X => Y holds, from the rows by definition."""
    out = []
    for s, r in enumerate(db.rows):
        first, last = {}, {}
        for j, st in enumerate(E.itemsets_of(r)):
            for it in st:
                first.setdefault(it, j)
                last[it] = j
        if all(x in first for x in X) and all(y in last for y in Y) and \
                max(first[x] for x in X) < min(last[y] for y in Y):
            out.append(s)
    return out


def test_tsr_constants_found():
    c = E.tsr_constants()
    for key in ("FSM_TSR_XBLOCK", "kPassKids", "kCollectBlocks", "kDomThreads", "kBlock", "kDlUnroll", "kExpSpb",
                "kExpBatch", "kExpBatchWide", "kWideMinsup", "pair_batch0"):
        assert c[key] > 0, key
    # the edge sids follow the constants: groups, a wave of groups, a block round and two of k_rank_dir; a
    # block round of k_dl (words of 32 sids) ends where two rounds of k_rank_dir do
    assert E.probe_edges() == tuple(s for e in (128, 64 * 128, c["kBlock"] * 128, c["kBlock"] * 256) for s in (e - 1, e))
    assert c["dl_round"] * 32 in (c["rank_round"], 2 * c["rank_round"])
    assert E.window_edges()[1] == 2 * c["FSM_TSR_XBLOCK"]


@pytest.mark.parametrize("kw", [dict(N=12, edges=(5, 6)), dict(N=20, edges=(7, 8), dl="and"),
                                dict(N=24, edges=(7, 8), extra=(15,), dl="list", sup3=16)], ids=str)
def test_tsr_probe_edges_small_vs_brute(kw):
    db = E.tsr_probe_edges(**kw)
    recs = db.records()
    valid = brute.brute_tsr_valid(recs, 0.0)
    allr = E.tsr_all_rules(db)
    assert {(x, y): (s, c) for x, y, s, c in allr} == valid
    for mode, k, final in E.tsr_modes(db):
        o = oracle.tsr(recs, k, 0.0)
        brute.check_tsr(o["rules"], valid, k)
        assert o["final_minsup"] == final and o["rules"] == [r for r in allr if r[2] >= final]
    assert valid[((1,), (2,))][0] == db.m and valid[((11,), (12,))][0] == db.m - 1


def test_tsr_kid_edges_small_vs_brute():
    db = E.tsr_kid_edges(4, 2, [5, 8])
    recs = db.records()
    valid = brute.brute_tsr_valid(recs, 0.5)
    o = oracle.tsr(recs, 5, 0.5)
    brute.check_tsr(o["rules"], valid, 5)
    assert o["final_minsup"] == 8 and len(o["rules"]) == 5
    assert valid[((db.tail_item(0),), (db.core[1],))][0] == 7 and valid[((db.tail_item(3),), (db.core[2],))][0] == 7
    assert {(x, y): (s, c) for x, y, s, c in E.tsr_all_rules(db, 7)} == {r: v for r, v in valid.items() if v[0] >= 7}


@pytest.mark.parametrize("n,copies", [(3, 3), (4, 3), (5, 4)])
def test_tsr_chain_small_vs_brute(n, copies):
    db = E.tsr_chain(n, copies)
    db.m = copies
    recs = db.records()
    valid = brute.brute_tsr_valid(recs, 0.0)
    allr = E.tsr_all_rules(db)
    assert {(x, y): (s, c) for x, y, s, c in allr} == valid
    for mode, k, final in E.tsr_modes(db):
        o = oracle.tsr(recs, k, 0.0)
        brute.check_tsr(o["rules"], valid, k)
        assert o["final_minsup"] == final and o["rules"] == [r for r in allr if r[2] >= final]


def test_tsr_pair_edges_small_vs_brute():
    db = E.tsr_pair_edges(9, m=2, starts=(4,), offs=(1, 2, 3))
    recs = db.records()
    valid = brute.brute_tsr_valid(recs, 0.0)
    assert {r: v[0] for r, v in valid.items()} == db.planted
    for mode, k, final in E.tsr_modes(db):
        o = oracle.tsr(recs, k, 0.0)
        brute.check_tsr(o["rules"], valid, k)
        assert o["final_minsup"] == final


@pytest.mark.parametrize("name", list(E.tsr_probe_cases()) + ["B-" + n for n in E.tsr_window_cases()])
def test_tsr_probe_and_window_cases(name):
    """Families A and B at the sizes the GPU tests use: the two modes, the planted rules at
    exactly m and m - 1, the deciding sids on the edges, the k_dl variants' denominators, the
    domain (every sid) in windows, and the kept rows of the big rules."""
    c = E.tsr_constants()
    fam_b = name.startswith("B-")
    db = E.tsr_window_cases()[name[2:]] if fam_b else E.tsr_probe_cases()[name]
    N, m = db.N, db.m
    modes = E.tsr_modes(db)
    assert_modes(db, modes)
    allr = E.tsr_all_rules(db)
    at_m = [r for r in allr if r[2] == m]
    assert at_m and len(at_m) == len([r for r in allr if r[2] == m - 1])
    assert modes[1][1] == len([r for r in allr if r[2] >= m]) < modes[0][1] == len(allr)
    # triple 1 holds exactly at the deciding sids, triple 2 at one fewer, spread between them
    assert holds_at(db, [1], [2]) == db.deciding and len(db.deciding) == m
    assert holds_at(db, [11], [12]) == sorted(db.second) and len(db.second) == m - 1
    assert not set(db.second) & set(db.deciding) and db.second[0] > db.deciding[1] and db.second[-1] < N - 1
    assert {0, 1, N - 1} | {e for e in db.edges if e < N} <= set(db.deciding)
    if not fam_b:  # N is one past an edge, or one group past the round edge
        assert N - 1 in db.edges or N - 1 == c["rank_round"] + c["group"]
    n3 = N - len(db.removed)
    for X, Y, s in (([1], [2], m), ([1], [3], m), ([3], [2], m), ([1, 3], [2], m), ([1], [2, 3], m), ([1], [13], m),
                    ([11], [12], m - 1), ([11], [13], m - 1), ([11, 13], [12], m - 1), ([3], [12], m - 1)):
        assert rsup(db, X, Y)[0] == s, (X, Y)
    assert rsup(db, [2], [1]) == (N - m, N) and rsup(db, [12], [11]) == (N - m + 1, N)
    # every sequence holds the five items besides 3: every domain without item 3 is all N sids
    masks = E.item_sid_masks(db)
    assert all(masks[i].all() for i in (1, 2, 11, 12, 13)) and int(masks[3].sum()) == n3
    assert E.tsr_domain_sum(db, allr) == sum(n3 if 3 in r[0] + r[1] else N for r in allr)
    if db.dl:
        # |sids({1, 3})| is not N, and the confidence of {1, 3} => 2 is m over it: it depends on the sids
        # item 3 was removed from
        assert rsup(db, [1, 3], [2]) == (m, n3) and n3 != N
        conf = [r[3] for r in allr if r[:2] == ((1, 3), (2,))]
        assert conf == [m / n3] and conf != [m / N]
        assert set(db.removed).isdisjoint(db.deciding)
        NW = E.bitmap_words(N)
        if db.dl == "and":
            # sup(3) >= bitmap words: the AND branch; the removed sids lie within two of an edge, on both
            # sides of the word edges, and (N = 65,537) the bitmap is one word longer than a block round
            assert n3 >= NW and all(min(abs(s - e) for e in db.edges) <= 2 for s in db.removed)
            assert {e - 2 for e in db.edges[::2] if e < N} <= set(db.removed)
            assert {e + 1 for e in db.edges[1::2] if e + 1 < N - 1} <= set(db.removed)
            assert NW > c["kBlock"] and (N < 65537 or NW > c["dl_round"])
        else:
            # sup(3) < bitmap words: the list branch, over more than one thread round (and, at N = 65,537,
            # two sids more than one block round of kBlock kDlUnroll)
            assert NW - 2 == n3 > c["kBlock"] and (N < 65537 or n3 == c["dl_round"] + 2)
    if name.endswith("-cuts"):
        assert set(E.shard_cuts(N)) <= set(db.deciding) and len(E.shard_cuts(N)) >= 5
    if fam_b:
        w = c["exp_win"]
        # at supports of a few units a slot gets one block (2 sup <= kExpSpb): its domain, all N sids, is
        # ceil(N / w) windows; the big rules keep N - m (N - m + 1) rows for their children
        assert 2 * m <= c["kExpSpb"] and (N - m) > c["kExpSpb"]
        if name[2:].startswith("N"):
            assert (N, -(-N // w), (N - 1) % w + 1) in ((w - 1, 1, w - 1), (w, 1, w), (w + 1, 2, 1), (2 * w, 2, w),
                                                        (2 * w + 1, 3, 1))
        else:
            assert N - m == int(name[7:]) and len(holds_at(db, [2], [1])) == N - m


def test_tsr_window_cases_cover_the_parent_list_edges():
    w = E.tsr_constants()["exp_win"]
    cases = E.tsr_window_cases()
    assert {db.N for db in cases.values()} >= {w - 1, w, w + 1, 2 * w, 2 * w + 1}
    assert {db.N - db.m for n, db in cases.items() if n.startswith("plist")} == {w - 1, w, w + 1}


@pytest.mark.parametrize("name", list(E.tsr_kid_cases()))
def test_tsr_kid_cases_placed(name):
    """Family C: K = low + 3 + T kids, all of support 8; the tight tail items sit on the kids the
    case names (dense rank of the item value), their rules are at 7 and the core rules at 8; lo_abs
    of the core rules covers kPassKids - 1, kPassKids and kPassKids + 1 over the three lows."""
    c = E.tsr_constants()
    P, q = c["kPassKids"], c["reduce_range"]
    for db in [E.tsr_kid_cases()[name]]:
        vals = sorted({t for r in db.rows for t in r if t >= 0})
        sup = {}
        for r in db.rows:
            for t in set(r):
                if t >= 0:
                    sup[t] = sup.get(t, 0) + 1
        assert len(vals) == db.K == db.low + 3 + db.T and set(sup.values()) == {8}, name
        assert [vals.index(v) for v in db.core] == [db.low, db.low + 1, db.low + 2]
        a7 = E.tsr_all_rules(db, 7)
        o = oracle.tsr(db.records(), 5, 0.5)
        assert o["final_minsup"] == 8 and o["rules"] == [r for r in a7 if r[2] >= 8] and len(o["rules"]) == 5, name
        tight_rules = [r for r in a7 if r[2] == 7]
        assert {r[2] for r in a7} == {7, 8}
        for j, kid in zip(db.tight, db.tight_kids):
            t = db.tail_item(j)
            assert vals.index(t) == kid, name
            for y in db.core[1:]:
                assert rsup(db, [t], [y]) == (7, 8) and ((t,), (y,), 7, 7 / 8) in tight_rules
        assert {x for r in tight_rules for x in r[0] + r[1]} - set(db.core) == {db.tail_item(j) for j in db.tight}
        for j in (1, db.T // 2 + 1, db.T - 2):
            if j not in db.tight:
                assert rsup(db, [db.tail_item(j)], [db.core[1]])[0] == 4
        # the second mode: the pair phase ends at 7, and the answer keeps rules of every tight item at 7
        (_, k5, f5), (_, k7, f7) = E.tsr_kid_modes(db)
        assert (k5, f5, f7) == (5, 8, 7) and E.pair_phase_threshold(a7, k7) == 7 and E.pair_phase_threshold(a7, k7 - 1) == 7
        o7 = oracle.tsr(db.records(), k7, 0.5)
        assert o7["final_minsup"] == 7 and set(o7["rules"]) <= set(a7) and set(o["rules"]) <= set(o7["rules"])
        for j in db.tight:
            assert any(db.tail_item(j) in r[0] + r[1] and r[2] == 7 for r in o7["rules"]), (name, j)
        los = {E.kid_lo_abs(db, r[0], r[1]) for r in o["rules"]}
        assert los == {db.low + 1, db.low + 2}, name
        if db.low:
            first, last = db.low + 3, db.K - 1
            assert {first, last, P + q - 1, P + q} | {k for k in (P - 1, P, P + 1) if k >= first} == set(db.tight_kids)
            assert len(db.rows) == 16 and all(len(E.itemsets_of(r)) == 1 for r in db.rows[8:])
            assert -(-db.K // P) == 3  # three kid passes; the fillers end in the last kids of pass 0
        else:
            assert db.tight_kids == [q - 1, q, P - 1, P, P + 1, 2 * P - 1, 2 * P] and db.K > 2 * P


def test_tsr_kid_cases_cover_the_pass_start():
    P = E.tsr_constants()["kPassKids"]
    lows = {db.low for db in E.tsr_kid_cases().values() if db.low}
    assert lows == {P - 3, P - 2, P - 1}  # lo_abs = low + 1, low + 2 (proved per DB above)
    assert {lo for low in lows for lo in (low + 1, low + 2)} >= {P - 1, P, P + 1}


def test_tsr_chain_cases_placed():
    """Family D: rules up to |X u Y| = n (4 / 5 and 8 / 9 items: DomProbe's rounds of 4, k_exp_domain's of 8),
    more than 20 full launches in exhaustive mode at n = 10, and the pair-phase thresholds of the wide DB."""
    c = E.tsr_constants()
    W = c["kWideMinsup"]
    sizes = set()
    for name, (db, modes) in E.tsr_chain_cases().items():
        assert_modes(db, modes)
        allr = E.tsr_all_rules(db)
        sizes |= {len(r[0]) + len(r[1]) for r in allr}
        assert max(len(r[0]) + len(r[1]) for r in allr) == db.n
        assert rsup(db, [1], [2])[0] == db.copies + 1 and rsup(db, [1], [db.n])[0] == db.copies
        assert rsup(db, [2], [1])[0] == 2
        if name == "n10":
            assert modes[0][1] > 20 * c["kExpBatch"]
        if name == "n10-wide":
            (_, k_w, f_w), (_, k_n, f_n) = modes
            assert E.pair_phase_threshold(allr, k_w) == W and E.pair_phase_threshold(allr, k_n) == W - 1
            assert f_w == f_n == W and db.copies + 1 == W
        else:
            assert all(E.pair_phase_threshold(allr, k) == 1 for _, k, _ in modes)
    assert {4, 5, 8, 9, 10} <= sizes


def test_tsr_pair_case_placed():
    """Family E: the planted pairs are the only rules, at exactly m and m - 1; i on the last item of a batch
    and the first of the next, j one, 63, 64 and 65 past it and the last item."""
    c = E.tsr_constants()
    db = E.tsr_pair_case()
    assert db.starts == [16, 48, 112, 240, 496] and c["pair_batch0"] == 16
    allr = E.tsr_all_rules(db)
    assert {r[:2]: r[2] for r in allr} == db.planted and set(db.planted.values()) == {db.m, db.m - 1}
    for (X, Y), s in db.planted.items():
        assert rsup(db, X, Y)[0] == s
    assert_modes(db, E.tsr_modes(db))
    masks = E.item_sid_masks(db)
    assert sorted(masks) == list(range(1, db.U + 1)) and min(int(v.sum()) for v in masks.values()) >= db.m
    ids = {i for i, _ in db.pairs}
    assert ids == {15, 16, 47, 48, 111, 112, 239, 240, 495, 496}
    for i in ids:
        assert {j - i for a, j in db.pairs if a == i} == {1, 63, 64, 65, db.U - 1 - i}


# ------------------------------------------------------------ SPADE along the sequence axis
def test_tall_geometry_table():
    """rpb and nblk of the root F2 for every R of the tall DBs, as Miner::f2_geometry's formula
    (its constants read from spade_engine.hip) gives them, against the stated table."""
    c = E.spade_constants()
    assert c["kF2MaxRows"] >= 64 and c["kF2MaxBlocks"] >= c["f2_blocks"] and c["rpb_min"] <= 64
    assert sorted(E.TALL_GEOMETRY) == sorted(E.tall_all_r())
    for blocks, rs in E.TALL_R:
        for R in rs:
            assert E.f2_row_blocks(R, blocks) == E.TALL_GEOMETRY[R], (blocks, R)
    # what the families are named after: nblk reaches kF2MaxBlocks, rpb reaches kF2MaxRows, and at
    # 4,097 rows in one target block the last block holds one row
    assert E.f2_row_blocks(32768, 2048) == (16, c["kF2MaxBlocks"])
    assert E.f2_row_blocks(4096, 1) == (c["kF2MaxRows"], 1) and 4097 - E.f2_row_blocks(4097, 1)[0] == 1
    # the branch no case takes: more rows than kF2MaxBlocks blocks of kF2MaxRows rows
    most = c["kF2MaxRows"] * c["kF2MaxBlocks"]
    assert E.f2_row_blocks(most) == (c["kF2MaxRows"], c["kF2MaxBlocks"]) and E.f2_row_blocks(most + 1) is None
    # the sizes also lie on both sides of a scan tile, and of one lap of k0_rows' waves
    k0 = E.k0_stage_constants()
    assert {c["kScanTile"] - 1, c["kScanTile"], c["kScanTile"] + 1} <= set(E.tall_all_r()) & set(E.K0_TALL_R)
    assert {k0["rows_lap"] - 1, k0["rows_lap"], k0["rows_lap"] + 1} <= set(E.tall_all_r()) & set(E.K0_TALL_R)


def _tall_policy_claims(db, R):
    """Each placement's rows are the first / last / only rows of blocks that its policy names."""
    rpb, nblk = E.f2_row_blocks(R, E.tall_blocks_env(R))
    seen = set()
    for label, P in db.placements.items():
        Pset, c = set(P), db.crit[label]
        assert len(P) == len(Pset) == db.S and c in Pset and 0 <= P[0] and P[-1] < R, label
        kind = label.split("(")[0]
        seen.add(label)
        if kind == "dense":
            assert P == list(range(R)) and c == R - 1
            continue
        if kind == "head":
            assert P == list(range(db.S)) and c == 0
            continue
        if kind == "tail":
            assert P == list(range(R - db.S, R)) and c == R - 1
            continue
        B = int(label.split("(")[1][:-1])
        assert B in (rpb, 64), label
        nb = -(-R // B)
        last = range((nb - 1) * B, R)  # the last block, partial unless B divides R
        if kind == "every":
            assert {0, R - 1} <= Pset and c == R - 1, label
            for k in range(nb):
                first, end = k * B, min(R, (k + 1) * B) - 1
                assert (end if k % 2 else first) in Pset, (label, k)
        elif kind == "edges":
            assert nb >= 2 and c == last[0], label
            for k in range(1, nb):
                assert k * B - 1 in Pset and k * B in Pset, (label, k)
        else:
            assert kind == "lone" and nb >= 2 and [r for r in P if r in last] == [c], label
    return seen, rpb, nblk


@pytest.mark.parametrize("dense", [False, True], ids=["placed", "dense"])
@pytest.mark.parametrize("R", E.tall_all_r())
def test_tall_spade_claims(R, dense):
    """Every tall DB: the policies' geometry, every gadget item's support (S; the F1- item S - 1)
    and rows (its placement and no other row), the row lengths, and the oracle's answer: minsup S,
    every t2 decision at exactly S, no t1 decision; the t1 decisions hold in exactly S - 1 rows."""
    db = E.tall_case(R, dense)
    S = db.S
    assert len(db.rows) == R and math.ceil(db.support * R) == S and (db.support == 1.0) == dense
    seen, rpb, nblk = _tall_policy_claims(db, R)
    if dense:
        assert S == R and seen == {"dense"}
    else:
        want = {"every(%d)" % rpb, "every(64)", "head", "tail"}
        if nblk >= 2:  # a second block: a first row of the last block, and a last block to be alone in
            want |= {"edges(%d)" % rpb, "lone(%d)" % rpb}
        assert want <= seen and S == max([E.TALL_MIN_S] + [
            len(E.tall_policy_rows(R, (l.split("(")[0], int(l.split("(")[1][:-1])))[0]) for l in seen if "(" in l])
        assert S > 100 or R <= 17
        # the last row of a partial last block / the only row of a block supports a decision
        assert R - 1 in db.placements["every(%d)" % rpb]
    _tall_row_item_oracle_claims(db, R)


def _tall_row_item_oracle_claims(db, R):
    """The row lengths, every gadget item's rows, and the oracle's answer on every decision; returns that answer."""
    S = db.S
    d = len(db.prefix_items)
    lens = np.diff(db.seq_off)
    seq_of = np.repeat(np.arange(R), lens)
    assert all(r[:2 * d] == [t for a in db.prefix_items for t in (a, -1)] for r in db.rows[:64] + db.rows[-64:])
    assert np.all(lens <= 16 * db.member + np.where(db.member > 0, E.TALL_SLOTS, 0) + 2 * d + 1)
    assert np.all(lens[db.member <= 2] <= 64) and (R <= 17 or np.count_nonzero(lens > 64) <= R // 50) and lens.max() <= 128
    for label, P in db.placements.items():
        for name, it in db.items[label].items():
            rows = seq_of[db.tokens == it]
            want = [r for r in P if r != db.crit[label]] if name == "g" else P
            assert rows.tolist() == want, (label, name)
    o = oracle.spade_tokens(db.seq_off, db.tokens, db.support)
    assert o["minsup"] == S
    got = dict(o["patterns"])
    for p in db.t2:
        assert got.get(p) == S, db.where(p)
    for p in db.t1:
        assert p not in got, db.where(p)
    assert len(set(db.t2 + db.t1)) == len(db.t2) + len(db.t1)
    for p in db.t1[:: max(1, len(db.t1) // 16)]:
        assert psup(db, p) == S - 1, db.where(p)
    assert db.root_entries() == sum(s for p, s in o["patterns"] if len(p) == 1 and len(p[0]) == 1)
    return got


def test_tall_near_dense_claims():
    """The near-dense DB: a minsup just below 2^16 under lattice counts above it.  65,537 rows, the
    head placement of S = 65,535 rows, three prefix items: A1 -> A2 -> A3 (counted in a class, not by
    the root F2) and every one of its sub-chains has support 65,537, the decisions 65,535 / 65,534."""
    R = E.TALL_NEAR_R
    db = E.tall_case(R, "near")
    assert db.S == R - 2 == 2 ** 16 - 1 and math.ceil(db.support * R) == db.S and len(db.prefix_items) == 3
    _tall_policy_claims(db, R)
    got = _tall_row_item_oracle_claims(db, R)
    for p in (((1,), (2,), (3,)), ((1,), (2,)), ((2,), (3,)), ((1,), (3,))):
        assert got[p] == R > 2 ** 16


@pytest.mark.parametrize("R", [15, 16, 17, 200])
def test_tall_spade_small_vs_brute(R):
    """At the smallest R, and at one of a few hundred rows, the oracle equals the definitional enumerator."""
    if R == 200:
        dbs = [E.tall_spade(200, None, [("every", 16), ("lone", 16), ("tail",)], prefix=1, seed=3),
               E.tall_spade(200, 200, [("dense",)], prefix=2, seed=3)]
    else:
        dbs = [E.tall_case(R), E.tall_case(R, dense=True)]
    for db in dbs:
        o = oracle.spade_tokens(db.seq_off, db.tokens, db.support)
        assert o["minsup"] == db.S
        assert o["patterns"] == brute.brute_spade(db.records(), db.support), db.name


# ------------------------------------------------------------ K0 on the same sizes
def test_k0_stage_sizes_and_closed_form():
    """The staging cases end on both sides of one chunk of offsets and of tokens, and their closed
    form is the image by definition (checked at a size k0_image takes at once)."""
    k0 = E.k0_stage_constants()
    per_off, per_tok = k0["kStageBytes"] // 8, k0["kStageBytes"] // 4
    assert [2 * R - per_tok for R in E.K0_STAGE_R] == [-2, 0, 2]         # tokens: the last chunk is one row
    assert [R + 1 - per_off for R in E.K0_STAGE_R] == [0, 1, 2]          # offsets: exactly one chunk, then 1 and 2 more
    for variant in E.K0_STAGE_VARIANTS:
        sids, so, tok, image = E.k0_stage_case(2500, variant)
        rows = [tok[so[r]:so[r + 1]].tolist() for r in range(2500)]
        for mode in ("spade", "tsr"):
            ref, img = E.k0_image(rows, mode), image(mode)
            assert sorted(ref) == sorted(img)
            for key, want in ref.items():
                assert np.array_equal(np.asarray(img[key]).astype(np.int64), np.asarray(want).astype(np.int64)), (variant, mode, key)
        lo, hi = int(tok[tok >= 0].min()), int(tok.max())
        at = {"last-max": [(hi, 2499)], "last-min": [(lo, 2499)], "first": [(lo, 0), (hi, 1)]}[variant]
        for v, r in at:
            assert np.flatnonzero(tok == v).tolist() == [2 * r]


def test_k0_extreme_cases():
    k0 = E.k0_stage_constants()
    for name, rows, modes in E.k0_extreme_cases():
        vals = [t for r in rows for t in r if t not in (-1, -2)]
        assert max(vals) - min(vals) == 2 ** 20 and all(E.INT32_MIN <= v <= E.INT32_MAX for v in vals)
        assert (E.INT32_MAX in vals) == ("max" in name) and (E.INT32_MIN in vals) == ("min" in name)
        assert len(rows[0]) == (k0["kK0Wave"] if "wave" in name else k0["kK0Long"])
        assert rows[0][-2] in (E.INT32_MAX, E.INT32_MIN) and len(set(rows[0])) < len(rows[0]) // 2 + 1
        assert ("tsr" in modes) == (min(vals) >= 0)
