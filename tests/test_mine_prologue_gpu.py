"""What a mine no longer repeats per call: the F1 supports stay with the DB handle (k_f1 runs in
a handle's first unsharded mine only; FSM_F1_CACHE=0 counts every mine), and k_f2_tri is
launched behind the plan's scan without waiting for the slot total where the DB's key bound
B = (sum of the bounded plan's table) + (alignment - 1) x regions passes the cursor limit and
the budget (FSM_F2_AHEAD=0 waits as before).

An engine made with verbose=True reports the scanned slot total N ("[fsm] root F2 plan: bound,
N key slots") and, on the ahead path, the bound ("[fsm] root F2 keys ahead: bound B"); the
tests read both from stderr.  Every mine is compared with the CPU oracle.

The synced fallback is not driven through a small mem_budget here: the table's own guard asks
for bytes <= budget / 8, and for quest(1500) (94 row blocks x 8,226 items x 4 B = 3.09 MB, so a
budget of 24.7 MB at least) 2 B is at most 2 x (1,731,843 + 7 x 8,192 x 94) = 14.2 MB at any
support (the table's sum, and 94 regions for each of the at most 8,192 rank groups the bounded
plan takes), so no budget keeps the table and fails the bound.  test_ahead_off_is_the_same_mine
runs that path."""
import re

import pytest

import edge_dbs as E
import test_root_plan_gpu as RP
from test_root_plan_gpu import PLAN, plan_db, quest, ref

pytestmark = pytest.mark.gpu

AHEAD = re.compile(r"\[fsm\] root F2 keys ahead: bound (\d+)")
ALIGN = 8  # key alignment of the root F2 regions (Miner::kF2Align)


class Mined(RP.Mined):
    def run(self, support, key):
        """One mine compared with the oracle (patterns, minsup, joins); returns a dict of what it reported."""
        self.capfd.readouterr()
        pats, meta = self.eng.spade(self.h, support)
        err = self.capfd.readouterr().err
        o = ref(key, self.seq_off, self.tokens, support)
        assert meta["minsup"] == o["minsup"], key
        assert sorted(pats) == o["patterns"], key
        assert self.eng.stats()["joins"] == o["joins"], key
        plans, aheads = PLAN.findall(err), AHEAD.findall(err)
        assert len(plans) <= 1 and len(aheads) <= 1, err
        return {"pats": sorted(pats), "joins": o["joins"], "plan": plans[0][0] if plans else None,
                "N": int(plans[0][1]) if plans else None, "B": int(aheads[0]) if aheads else None,
                "names": {k["name"] for k in self.eng.kernel_stats()}}


@pytest.fixture(scope="module")
def veng():
    import spark_fsm_amd
    e = spark_fsm_amd.Engine(0, verbose=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pdb():
    return plan_db()


@pytest.fixture(scope="module")
def q1500():
    return quest(1500, 3)


@pytest.fixture(scope="module")
def q700():
    return quest(700, 4)


def all_frequent_db():
    """40 rows = three row blocks (16, 16, 8) in which every one of the 23 items is frequent at
    minsup 2: twenty rows of 1 to 9 items in itemsets of three, each row twice.

    It stands in for plan_db() at minsup 1, which cannot be mined by the engine or by the oracle:
    with every item frequent, each of the 2^68 sub-patterns of its 68-entry row is a pattern.
    What that case is for holds here: with no infrequent item the bounded plan's capacities are
    the table's sums themselves, so the scanned total is at least the table's sum."""
    base = []
    for i in range(20):
        n = 1 + (i * 4) % 9
        items = sorted({(i + 5 * j) % 23 + 1 for j in range(n)})
        base.append(E._row([items[k:k + 3] for k in range(0, len(items), 3)]))
    return E.EdgeDB(base + base, "allfreq")


@pytest.fixture(scope="module")
def adb():
    return all_frequent_db()


def test_all_frequent_db_shape(adb):
    o = ref("allfreq", adb.seq_off, adb.tokens, adb.support)
    items = {t for r in adb.rows for t in r if t >= 0}
    assert o["minsup"] == 2 and len(adb.rows) == 40
    assert sorted(p[0][0] for p, _ in o["patterns"] if len(p) == 1 and len(p[0]) == 1) == sorted(items)
    assert sorted({len({t for t in r if t >= 0}) for r in adb.rows}) == list(range(1, 10))


def sup_of(db, minsup):
    """a relative support with ceil(support * N) = minsup"""
    return (minsup - 0.5) / len(db.rows)


Q_SUPS = (0.015, 0.004, 0.015)


def test_f1_kept_across_supports(veng, capfd, q1500, pdb):
    m = Mined(veng, capfd, q1500.sids, q1500.seq_off, q1500.tokens)
    try:
        got = [m.run(s, ("quest1500", s)) for s in Q_SUPS]
    finally:
        m.free()
    assert [("k_f1" in g["names"]) for g in got] == [True, False, False]
    assert got[0]["pats"] == got[2]["pats"] and len(got[1]["pats"]) > len(got[0]["pats"]) > 0
    nf = [sum(1 for p, _ in g["pats"] if len(p) == 1 and len(p[0]) == 1) for g in got]
    assert nf == [138, 2326, 138]
    # a mine in which nothing is frequent (it launches no root at all) leaves the supports as they were
    m = Mined(veng, capfd, pdb.sids, pdb.seq_off, pdb.tokens)
    try:
        got = [m.run(sup_of(pdb, 2), "plan"), m.run(1.0, ("plan", "none")), m.run(sup_of(pdb, 2), "plan")]
    finally:
        m.free()
    assert [("k_f1" in g["names"]) for g in got] == [True, False, False]
    assert got[0]["pats"] and not got[1]["pats"] and got[2]["pats"] == got[0]["pats"]


def test_two_handles_interleaved(veng, capfd, q1500, q700, pdb):
    a = Mined(veng, capfd, q1500.sids, q1500.seq_off, q1500.tokens)
    b = Mined(veng, capfd, q700.sids, q700.seq_off, q700.tokens)
    try:
        seen = []
        for i in range(2):
            seen.append("k_f1" in a.run(0.015, ("quest1500", 0.015))["names"])
            seen.append("k_f1" in b.run(0.008, ("quest700", 0.008))["names"])
        assert seen == [True, True, False, False]
        # A's handle freed, another DB made (the allocator may hand out A's address again): it counts its own F1
        a.free()
        a = Mined(veng, capfd, pdb.sids, pdb.seq_off, pdb.tokens)
        g = a.run(pdb.support, "plan")
        assert "k_f1" in g["names"] and g["pats"]
        assert "k_f1" not in b.run(0.008, ("quest700", 0.008))["names"]
    finally:
        a.free()
        b.free()


def test_f1_cache_off_counts_every_mine(veng, capfd, q1500, monkeypatch):
    m = Mined(veng, capfd, q1500.sids, q1500.seq_off, q1500.tokens)
    try:
        cached = [m.run(s, ("quest1500", s)) for s in Q_SUPS]
    finally:
        m.free()
    monkeypatch.setenv("FSM_F1_CACHE", "0")
    m = Mined(veng, capfd, q1500.sids, q1500.seq_off, q1500.tokens)
    try:
        plain = [m.run(s, ("quest1500", s)) for s in Q_SUPS]
    finally:
        m.free()
    assert all("k_f1" in g["names"] for g in plain)
    assert [g["pats"] for g in plain] == [g["pats"] for g in cached]
    assert [g["N"] for g in plain] == [g["N"] for g in cached]


def closed_form_sum(db):
    """the bounded plan's table summed over every item and row block: a row of n distinct items
    adds n + 3 n (n - 1) / 2 (its entry at position p: 1 + 3 (n - 1 - p))"""
    lens = [len({t for t in r if t >= 0}) for r in db.rows]
    return sum(n + 3 * n * (n - 1) // 2 for n in lens)


def test_bound_covers_the_scanned_total(veng, capfd, adb, pdb, q1500, monkeypatch):
    m = Mined(veng, capfd, adb.sids, adb.seq_off, adb.tokens)
    try:
        one = m.run(adb.support, "allfreq")
    finally:
        m.free()
    m = Mined(veng, capfd, pdb.sids, pdb.seq_off, pdb.tokens)
    try:
        two = m.run(sup_of(pdb, 2), "plan")
    finally:
        m.free()
    for g in (one, two):
        assert g["plan"] == "bound" and g["B"] is not None and g["N"] <= g["B"], g
    # every item frequent: each region holds its whole share of the table, rounded up, and the
    # bound adds (alignment - 1) per region (40 and 36 rows: three row blocks each)
    s_all = closed_form_sum(adb)
    assert s_all <= one["N"] <= one["B"]
    assert (one["B"] - s_all) % ((ALIGN - 1) * 3) == 0 and one["B"] > s_all
    # infrequent items in every position: the capacities count them as partners, the total stays under the sum
    s_plan = closed_form_sum(pdb)
    assert two["N"] < s_plan < two["B"] and (two["B"] - s_plan) % ((ALIGN - 1) * 3) == 0
    m = Mined(veng, capfd, q1500.sids, q1500.seq_off, q1500.tokens)
    try:
        qs = [m.run(s, ("quest1500", s)) for s in (0.015, 0.004, 0.002)]
    finally:
        m.free()
    s_q = closed_form_sum(q1500_rows(q1500))
    nblk = (1500 + 15) // 16
    for g in qs:
        assert g["plan"] == "bound" and g["B"] is not None and g["N"] <= g["B"], g
        assert g["B"] > s_q and (g["B"] - s_q) % ((ALIGN - 1) * nblk) == 0
    assert qs[0]["N"] < qs[1]["N"] < qs[2]["N"] and qs[0]["B"] <= qs[1]["B"] <= qs[2]["B"]
    # the exact plan has no table and no bound: it waits for its total
    monkeypatch.setenv("FSM_F2_PLAN", "exact")
    m = Mined(veng, capfd, pdb.sids, pdb.seq_off, pdb.tokens)
    try:
        g = m.run(sup_of(pdb, 2), "plan")
    finally:
        m.free()
    assert g["plan"] == "exact" and g["B"] is None


class q1500_rows:
    """the rows of a generated DB as token lists (closed_form_sum reads .rows)"""

    def __init__(self, ds):
        so, tk = list(ds.seq_off), list(ds.tokens)
        self.rows = [tk[so[i]:so[i + 1]] for i in range(len(so) - 1)]


def test_ahead_off_is_the_same_mine(veng, capfd, adb, pdb, q1500, monkeypatch):
    cases = [(adb, adb.support, "allfreq"), (pdb, sup_of(pdb, 2), "plan")] + \
        [(q1500, s, ("quest1500", s)) for s in (0.015, 0.004, 0.002)]
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("FSM_F2_AHEAD", mode)
        hs = {}
        try:
            for db, sup, key in cases:
                if id(db) not in hs:
                    hs[id(db)] = Mined(veng, capfd, db.sids, db.seq_off, db.tokens)
                got[mode, key] = hs[id(db)].run(sup, key)
        finally:
            for h in hs.values():
                h.free()
    for _, _, key in cases:
        on, off = got["1", key], got["0", key]
        assert on["pats"] == off["pats"] and on["joins"] == off["joins"]
        assert on["plan"] == off["plan"] == "bound" and on["N"] == off["N"]
        assert on["B"] is not None and off["B"] is None


def test_geometry_change_rebuilds_table_and_bound(veng, capfd, q1500, monkeypatch):
    m = Mined(veng, capfd, q1500.sids, q1500.seq_off, q1500.tokens)
    try:
        a = m.run(0.004, ("quest1500", 0.004))       # 1,500 rows in blocks of 16 (the smallest): 94 blocks
        monkeypatch.setenv("FSM_F2_BLOCKS", "10")    # 10 blocks of 150 rows
        b = m.run(0.004, ("quest1500", 0.004))
        monkeypatch.delenv("FSM_F2_BLOCKS")
        c = m.run(0.004, ("quest1500", 0.004))
    finally:
        m.free()
    assert [("k_f2_bound_tab" in g["names"]) for g in (a, b, c)] == [True, True, True]
    assert all("k_f1" not in g["names"] for g in (b, c))
    for g in (a, b, c):
        assert g["plan"] == "bound" and g["B"] is not None and g["N"] <= g["B"]
    # fewer regions: less alignment in the bound (the table's sum is the DB's, whatever the blocks)
    assert b["B"] < a["B"] == c["B"] and a["N"] == c["N"]
    s_q = closed_form_sum(q1500_rows(q1500))
    assert (a["B"] - s_q) % ((ALIGN - 1) * 94) == 0 and (b["B"] - s_q) % ((ALIGN - 1) * 10) == 0
    assert (a["B"] - s_q) // 94 == (b["B"] - s_q) // 10  # (alignment - 1) x the rank groups, the same in both


def test_sharded_mine_counts_f1_and_waits(capfd, pdb):
    import spark_fsm_amd
    names, errs = [], []
    with spark_fsm_amd.Engine(devices=[0, 0], verbose=True) as e:
        m = RP.Mined(e, capfd, pdb.sids, pdb.seq_off, pdb.tokens)
        try:
            for _ in range(2):
                capfd.readouterr()
                pats, meta = e.spade(m.h, pdb.support)
                errs.append(capfd.readouterr().err)
                names.append({k["name"] for k in e.kernel_stats()})
                assert sorted(pats) == ref("plan", pdb.seq_off, pdb.tokens, pdb.support)["patterns"]
        finally:
            m.free()
    assert all("k_f1" in n for n in names)
    assert not any(AHEAD.search(err) for err in errs)
