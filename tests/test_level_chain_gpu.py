"""The lattice levels' record chain: k_freq_recs leaves every counter row's record count and
run start behind, k_rk_tables and k_rk_run order the runs before the host has read the
record count, and whatever makes the host drop that pass (more records than the first
buffer holds, FSM_DEVORDER=0) must still give the same mine.

One DB (chain_db) puts every ordering edge into its first-level batch; every pattern in it
has support exactly 2 = minsup (each sequence is written twice), or a multiple where
sequences share a prefix.  All results are compared with the CPU oracle, pattern for pattern and
with the join count."""
import pytest

import edge_dbs as E

pytestmark = pytest.mark.gpu

RK_TILE = 2048  # kRkTile: counter rows per k_rk_tables block
FILLER = 2100   # filler pairs: one empty counter row each, so the rows pass RK_TILE with room


def seqs(*itemsets):
    return [E._row([list(s) for s in itemsets])] * 2


def chain_db():
    """Items ascend with their rank, so the counter rows of the first-level batch (one per
    frequent 2-pattern, in class then member order) come in this order:

      low block    a -> b with a -> b -> c and a -> (b c): a sequence and an itemset extension by the
                   same partner item c, in one row;
                   d -> e whose only record is d -> (e f): a lone itemset extension, which
                   opens no child class;
                   h -> p with 70 records h -> p -> c_i (more than one wave step), followed
                   by the 70 empty rows h -> c_i and the 70 empty rows p -> c_i
      filler       FILLER rows x_i -> y_i without records: the rows pass one k_rk_tables tile
      high block   the low block's first two shapes again, past the tile boundary
      last         y -> z, the last row, empty
    """
    rows = []

    def shapes(a, b, c, d, e, f):
        out = seqs([a], [b], [c]) + seqs([a], [b, c])
        out += seqs([d], [e, f])
        return out

    rows += shapes(1, 2, 3, 4, 5, 6)
    h, p = 10, 11
    for i in range(70):
        rows += seqs([h], [p], [20 + i])
    base = 1000
    for i in range(FILLER):
        rows += seqs([base + 2 * i], [base + 2 * i + 1])
    top = base + 2 * FILLER + 10
    rows += shapes(top, top + 1, top + 2, top + 3, top + 4, top + 5)
    rows += seqs([top + 10], [top + 11])
    return E.EdgeDB(rows, "chain")


_REF = {}


def ref(db):
    """The oracle's answer, once per DB."""
    if db.name not in _REF:
        from oracle import oracle
        o = oracle.spade_tokens(db.seq_off, db.tokens, db.support)
        assert o["minsup"] == 2
        _REF[db.name] = o
    return _REF[db.name]


@pytest.fixture(scope="module")
def eng():
    import spark_fsm_amd
    e = spark_fsm_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def db():
    return chain_db()


def mine(eng, db):
    from spark_fsm_amd import MODE_SPADE
    h = eng.db_from_tokens(db.sids, db.seq_off, db.tokens, MODE_SPADE)
    try:
        pats, meta = eng.spade(h, db.support)
    finally:
        h.free()
    assert meta["minsup"] == 2
    return sorted(pats), eng.stats(), {k["name"]: k["launches"] for k in eng.kernel_stats()}


def check(eng, db):
    o = ref(db)
    pats, st, ks = mine(eng, db)
    if pats != o["patterns"]:
        got, exp = dict(pats), dict(o["patterns"])
        diff = [(p, got.get(p), exp.get(p)) for p in sorted(set(got) | set(exp)) if got.get(p) != exp.get(p)]
        raise AssertionError("%s: %d patterns differ (pattern, GPU, oracle): %r" % (db.name, len(diff), diff[:6]))
    assert st["joins"] == o["joins"]
    return pats, ks


def test_chain_db_shape(db):
    """The DB has what its docstring says (from the oracle's patterns: no GPU result involved)."""
    pats = dict(ref(db)["patterns"])
    two = sorted(p for p in pats if sum(len(s) for s in p) == 2)
    three = [p for p in pats if sum(len(s) for s in p) == 3]
    assert len(two) > RK_TILE + 8  # the counter rows of the first-level batch
    # records per row: the 3-patterns by the 2-pattern they extend (their first two items)

    def parent(p):
        flat = [(k, i) for k, s in enumerate(p) for i in s][:2]
        return ((flat[0][1],), (flat[1][1],)) if flat[0][0] != flat[1][0] else ((flat[0][1], flat[1][1]),)
    per = {}
    for p in three:
        per.setdefault(parent(p), []).append(p)
    assert sorted(per[((1,), (2,))]) == [((1,), (2,), (3,)), ((1,), (2, 3))]
    assert per[((4,), (5,))] == [((4,), (5, 6))]
    assert len(per[((10,), (11,))]) == 70
    assert ((10,), (20,)) in pats and ((10,), (20,)) not in per
    assert max(two) not in per  # the last row is empty
    assert not any(sum(len(s) for s in p) > 3 for p in pats)  # the second-level batch has no record at all


@pytest.mark.parametrize("env", ["", "FSM_DEVORDER=0"], ids=lambda e: e or "default")
def test_ordering_edges(eng, db, env, monkeypatch):
    """The chain DB, ordered ahead of the count read-back (default) and on the host."""
    for kv in env.split():
        monkeypatch.setenv(*kv.split("="))
    check(eng, db)


def test_extraction_retry(eng, db, monkeypatch):
    """The first record buffer capped at 16 records (FSM_FREQ_CAP; uncapped it is
    max(4 x rows, 4096), which no DB the oracle mines in seconds overflows): the first-level
    batch has 76 and more, so its first pass overflows, the ordering launched behind it is
    dropped, and the batch is extracted once more at the exact size."""
    _, ks0 = check(eng, db)
    monkeypatch.setenv("FSM_FREQ_CAP", "16")
    _, ks1 = check(eng, db)
    assert ks1["k_freq_recs"] == ks0["k_freq_recs"] + 1
    monkeypatch.setenv("FSM_FREQ_CAP", "75")  # one record short: only the last run crosses the cap
    check(eng, db)
    monkeypatch.setenv("FSM_DEVORDER", "0")
    check(eng, db)


@pytest.mark.parametrize("rows", [seqs([7]), seqs([7], [7]), seqs([7], [8]) + seqs([9])[:1]],
                         ids=["one-item", "one-item-twice", "two-items"])
def test_empty_results(eng, rows):
    """A root with one frequent item (no pair, and the pair 7 -> 7), and batches without any
    record (the last batch of every mine; here the first-level one)."""
    d = E.EdgeDB(rows + [E._row([[100 + i]]) for i in range(len(rows) // 2)], "empty-%d-%d" % (len(rows), len(rows[0])))
    check(eng, d)
