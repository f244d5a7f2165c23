"""CPU tests of tests/edge_dbs.py: the threshold-tight families mean what they
claim, so tests/test_edges_gpu.py is sensitive to a count that is off by one.
No GPU.

For every family: at its small sizes the oracle's answer against the
definitional enumerator (oracle/brute.py); at every size the GPU tests use,
the tightness claim itself, re-counted by definition (oracle.pattern_support /
oracle.rule_support): every selected relation exactly at the threshold, a
sample of the rest (first, last and middle ranks included) exactly one below;
and the geometry each case is named after."""
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


@pytest.mark.parametrize("w", [1, 2])
def test_lattice_cases_tight_and_placed(w):
    rg = E.wave_ranges()
    assert all(v > 0 and v % 64 == 0 for v in rg.values())
    starts = {0: set(), 1: set()}
    for name, db, level, claim in E.lattice_cases(w):
        assert E.mask_width(db) == w, name
        E.check_lattice_claim(db, level, claim)
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
