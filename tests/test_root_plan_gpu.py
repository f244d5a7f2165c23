"""The root F2 plan from the DB's table (FSM_F2_PLAN=bound, the default) against the exact
plan walked from the rows (FSM_F2_PLAN=exact) and the CPU oracle.

The bounded plan sizes an entry's key region by the entries after it in its row, frequent or
not, so it differs from the exact one exactly where infrequent items sit in a row; the table
is built once per DB and row block geometry and reused by every later mine whatever its
minsup.  An engine made with verbose=True reports the plan it took and its key slots
("[fsm] root F2 plan: bound, N key slots"), which the tests read from stderr."""
import re

import pytest

import edge_dbs as E

pytestmark = pytest.mark.gpu

A, B, C, D = 100, 200, 300, 400  # the frequent items; every other item occurs once


def plan_db():
    """36 rows = three row blocks of 16 (the smallest block), minsup 2:
      * rows with infrequent items before, between and after the frequent ones, and rows
        without a frequent item;
      * two rows of 68 and 66 entries (k_f2_tri's long-row path: more than 64), three and
        two of them frequent, the rest spread below, between and above those;
      * short rows (one or two entries) from row 10 to row 35: both block boundaries (16, 32)
        fall inside the run."""
    nxt = {"lo": 0, "mid": 100, "hi": 400}

    def u(where):  # a fresh infrequent item below A, between the frequent items, or above D
        nxt[where] += 1
        v = nxt[where]
        while v in (A, B, C, D):
            nxt[where] += 1
            v = nxt[where]
        assert v < 100 or where != "lo"
        return v

    def long_row(freq, n):
        items = sorted(freq + [u("lo") for _ in range(20)] + [u("mid") for _ in range(n - 40 - len(freq))] +
                       [u("hi") for _ in range(20)])
        assert len(items) == n
        return E._row([items[i:i + 4] for i in range(0, n, 4)])  # 4 items per itemset: at most 17 eids, W = 1

    rows = [
        E._row([[u("lo"), A], [u("mid"), B], [u("hi")]]),
        E._row([[A], [B], [C]]),
        E._row([[u("lo")], [u("hi")]]),
        long_row([A, C, D], 68),
        E._row([[A, u("mid"), D]]),
        long_row([B, C], 66),
        E._row([[u("mid")], [B], [u("mid")], [C], [u("hi")]]),
        E._row([[u("lo"), u("mid"), u("hi")]]),
        E._row([[A], [u("lo")], [B, D]]),
        E._row([[D], [C], [u("hi")], [A]]),
    ]
    short = [lambda: [[A]], lambda: [[B, C]], lambda: [[u("mid")]], lambda: [[D]], lambda: [[C], [D]],
             lambda: [[u("hi")]], lambda: [[A, B]], lambda: [[B]], lambda: [[u("lo"), C]]]
    for i in range(26):
        rows.append(E._row(short[i % len(short)]()))
    assert len(rows) == 36
    return E.EdgeDB(rows, "plan")


_REF = {}


def ref(key, seq_off, tokens, support):
    if key not in _REF:
        from oracle import oracle
        _REF[key] = oracle.spade_tokens(seq_off, tokens, support)
    return _REF[key]


PLAN = re.compile(r"\[fsm\] root F2 plan: (bound|exact), (\d+) key slots")


class Mined:
    def __init__(self, eng, capfd, sids, seq_off, tokens):
        from spark_fsm_amd import MODE_SPADE
        self.eng, self.capfd = eng, capfd
        self.seq_off, self.tokens = seq_off, tokens
        self.h = eng.db_from_tokens(sids, seq_off, tokens, MODE_SPADE)

    def mine(self, support, key):
        """One mine compared with the oracle; returns (patterns, plan taken or None, key slots, kernel names)."""
        self.capfd.readouterr()
        pats, meta = self.eng.spade(self.h, support)
        err = self.capfd.readouterr().err
        o = ref(key, self.seq_off, self.tokens, support)
        assert meta["minsup"] == o["minsup"] or not o["patterns"]
        assert sorted(pats) == o["patterns"], key
        assert self.eng.stats()["joins"] == o["joins"], key
        m = PLAN.search(err)
        names = {k["name"] for k in self.eng.kernel_stats()}
        return sorted(pats), m and m.group(1), m and int(m.group(2)), names

    def free(self):
        self.h.free()


@pytest.fixture(scope="module")
def veng():
    import spark_fsm_amd
    e = spark_fsm_amd.Engine(0, verbose=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pdb():
    return plan_db()


def test_plan_db_shape(pdb):
    """What plan_db's docstring says, from the rows and the oracle."""
    o = ref("plan", pdb.seq_off, pdb.tokens, pdb.support)
    assert o["minsup"] == 2
    assert sorted(p[0][0] for p, _ in o["patterns"] if len(p) == 1 and len(p[0]) == 1) == [A, B, C, D]
    lens = [len({t for t in r if t >= 0}) for r in pdb.rows]
    assert sorted(lens)[-2:] == [66, 68] and all(n <= 2 for n in lens[10:])
    assert any(not ({A, B, C, D} & set(r)) for r in pdb.rows[:10])


def test_bound_differs_from_exact(veng, capfd, pdb, monkeypatch):
    """Both plans give the oracle's patterns; the bounded one reserves more key slots (the
    infrequent items count as partners) and builds the DB's table, the exact one neither."""
    got = {}
    for plan in ("bound", "exact"):
        monkeypatch.setenv("FSM_F2_PLAN", plan)
        m = Mined(veng, capfd, pdb.sids, pdb.seq_off, pdb.tokens)
        try:
            got[plan] = m.mine(pdb.support, "plan")
        finally:
            m.free()
    pats_b, took_b, slots_b, names_b = got["bound"]
    pats_e, took_e, slots_e, names_e = got["exact"]
    assert pats_b == pats_e
    assert (took_b, took_e) == ("bound", "exact")
    assert slots_b > slots_e
    assert "k_f2_bound_tab" in names_b and "k_f2_bound_tab" not in names_e


def quest(n, seed):
    from tools import gen
    return gen.quest(n, seed=seed)


def test_table_reuse(veng, capfd):
    """One DB handle at a high minsup (one rank group), a low one (hundreds of groups) and
    the high one again, then a DB of another size on the same engine: every mine equals the
    oracle, and only a DB's first mine builds its table."""
    ds = quest(1500, 3)
    m = Mined(veng, capfd, ds.sids, ds.seq_off, ds.tokens)
    try:
        for i, sup in enumerate((0.015, 0.004, 0.015)):
            pats, took, _, names = m.mine(sup, ("quest1500", sup))
            assert pats and took == "bound"
            assert ("k_f2_bound_tab" in names) == (i == 0)
        nf = [sum(1 for p, _ in ref(("quest1500", s), None, None, s)["patterns"] if len(p) == 1 and len(p[0]) == 1)
              for s in (0.015, 0.004)]
        assert nf == [138, 2326]  # frequent items: the rank groups grow with their square
    finally:
        m.free()
    ds2 = quest(700, 4)
    m2 = Mined(veng, capfd, ds2.sids, ds2.seq_off, ds2.tokens)
    try:
        for i, sup in enumerate((0.008, 0.008)):
            pats, took, _, names = m2.mine(sup, ("quest700", sup))
            assert pats and took == "bound"
            assert ("k_f2_bound_tab" in names) == (i == 0)
    finally:
        m2.free()


def test_size_guard_takes_exact_plan(veng, capfd, pdb, monkeypatch):
    """FSM_F2_TAB_MAX=0: no table fits the guard, so the mine takes the exact plan."""
    monkeypatch.setenv("FSM_F2_TAB_MAX", "0")
    m = Mined(veng, capfd, pdb.sids, pdb.seq_off, pdb.tokens)
    try:
        _, took, _, names = m.mine(pdb.support, "plan")
    finally:
        m.free()
    assert took == "exact" and "k_f2_bound_tab" not in names


def test_sharded_mine_keeps_exact_plan(capfd, pdb):
    """Two in-process ranks on one device: the sharded root never takes the bounded plan, and
    the mine equals the single-rank one (the oracle's)."""
    import spark_fsm_amd
    with spark_fsm_amd.Engine(devices=[0, 0], verbose=True) as e:
        m = Mined(e, capfd, pdb.sids, pdb.seq_off, pdb.tokens)
        try:
            capfd.readouterr()
            pats, meta = e.spade(m.h, pdb.support)
            err = capfd.readouterr().err
            names = {k["name"] for k in e.kernel_stats()}
        finally:
            m.free()
    assert sorted(pats) == ref("plan", pdb.seq_off, pdb.tokens, pdb.support)["patterns"]
    assert not any(t[0] == "bound" for t in PLAN.findall(err)) and "k_f2_bound_tab" not in names
