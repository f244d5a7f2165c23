"""GPU parity of TSR on the expansion kernels' geometry constants, with threshold-tight DBs.

The DBs come from tests/edge_dbs.py (tsr_probe_edges, tsr_kid_edges, tsr_chain, tsr_pair_edges),
placed on the constants read from tsr_engine.hip itself (edge_dbs.tsr_constants): rank-directory
groups and rounds (k_rank_dir, bm_rank, k_vfl, DomProbe), the 1,024-sid windows of k_exp_rows over
domains and parent lists, kid passes with the klo cut and the reduce ranges (k_expand_reduce), both
branches of k_dl, the operand rounds of DomProbe and k_exp_domain, and the pair phase's batch and
slice edges.  tests/test_edge_dbs.py proves each placement and each planted support on the same
objects without a GPU.

Every case compares the rules (X, Y, support, confidence bit for bit) and the final minsup with
oracle.tsr, whose answer tests/test_edge_dbs.py ties to oracle.tsr_all (every valid rule by
definition).  Each DB runs in two modes: exhaustive (k = every valid rule: each counter of each
expansion comes back as a rule with its support, the minsup stays 1) and tight (k = the rules at
support >= m: the rules planted at m - 1 must be absent, the final minsup is m, and k_alive and the
rising launch minsup take part).  Family C runs at k = 5 and at k = its two-item rules of support
>= 7 (edge_dbs.tsr_kid_modes): a k that keeps the threshold lower costs the top-k restatement tens
of seconds per DB through the tail x tail pairs.

Evidence that a path ran comes from Engine.stats() where a counter shows it (exp_domain,
exp_bitmap_bytes, exp_entries); where none does (list-mode domains, kid passes, reduce ranges, the
k_dl branch, pair batches) the CPU proof of the geometry is the evidence."""
import pytest

import edge_dbs as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fsm():
    import spark_fsm_amd
    return spark_fsm_amd


@pytest.fixture(scope="module")
def eng(fsm):
    e = fsm.Engine(0)
    yield e
    e.close()


def gpu_tsr(eng, db, k, minconf):
    from spark_fsm_amd import MODE_TSR
    h = eng.db_from_tokens(db.sids, db.seq_off, db.tokens, MODE_TSR)
    try:
        rules, meta = eng.tsr(h, k, minconf)
    finally:
        h.free()
    rules.sort(key=lambda t: (-t[2], t[0], t[1]))
    return rules, meta, eng.stats()


_ORACLE = {}


def tsr_ref(db, k):
    """oracle.tsr of a DB at k (and the DB's minconf), computed once per session and left unchanged."""
    key = (id(db), k)
    if key not in _ORACLE:
        from oracle import oracle
        _ORACLE[key] = (db, oracle.tsr(db.records(), k, db.minconf))
    return _ORACLE[key][1]


def check_tsr(eng, db, mode, k, final):
    o = tsr_ref(db, k)
    assert o["final_minsup"] == final, (db.name, mode)
    rules, meta, st = gpu_tsr(eng, db, k, db.minconf)
    if rules != o["rules"]:
        got, exp = {r[:2]: r[2:] for r in rules}, {r[:2]: r[2:] for r in o["rules"]}
        diff = [(r, got.get(r), exp.get(r)) for r in sorted(set(got) | set(exp)) if got.get(r) != exp.get(r)]
        raise AssertionError("%s %s: %d rules differ (rule, GPU, oracle): %r" % (db.name, mode, len(diff), diff[:6]))
    assert meta["final_minsup"] == final, (db.name, mode)
    if mode == "exhaustive":
        assert len(rules) == k
    elif mode == "tight":
        assert len(rules) == k and min(r[2] for r in rules) == db.m
    return st


def check_modes(eng, db, modes=None):
    return {mode: check_tsr(eng, db, mode, k, final) for mode, k, final in (modes or E.tsr_modes(db))}


def setenv(monkeypatch, env):
    for kv in env.split():
        k, v = kv.split("=")
        monkeypatch.setenv(k, v)


def check_plist_evidence(eng, db, monkeypatch, st_default):
    """Lists off, exhaustive mode: every valid rule is expanded once over the sids holding its items, so
    exp_domain is the generator's sum and exp_bitmap_bytes one bitmap per item of every rule; with the
    lists (the default) fewer bitmaps are read: children took their parents' kept rows."""
    monkeypatch.setenv("FSM_TSR_PLIST", "0")
    mode, k, final = E.tsr_modes(db)[0]
    st = check_tsr(eng, db, mode, k, final)
    monkeypatch.delenv("FSM_TSR_PLIST")
    allr = E.tsr_all_rules(db)
    assert st["exp_domain"] == E.tsr_domain_sum(db, allr), db.name
    assert st["exp_bitmap_bytes"] == sum(len(r[0]) + len(r[1]) for r in allr) * E.bitmap_words(db.N) * 4, db.name
    assert 0 < st_default["exp_bitmap_bytes"] < st["exp_bitmap_bytes"], db.name


# ------------------------------------------------------------ A. rank-directory and bitmap edges
@pytest.mark.parametrize("name", list(E.tsr_probe_cases()))
def test_probed_sids_on_rank_edges(eng, name, monkeypatch):
    """Two triples of items in every sequence; triple 1 holds at the sids 0, 1, 127 / 128, 8,191 / 8,192,
    32,767 / 32,768, 65,535 / 65,536 and N - 1 (the group, wave, round and two-round edges of k_rank_dir),
    triple 2 at one sid fewer; every other row fails with the same items, so it is probed too.  A rank off
    by one moves a candidate count across m / m - 1.  The dl variants remove item 3 around the edges, so
    that |sids({1, 3})| (k_dl: the AND branch, or the list branch with item 3 in bitmap words - 2
    sequences) decides the confidence of {1, 3} => 2."""
    db = E.tsr_probe_cases()[name]
    st = check_modes(eng, db)
    check_plist_evidence(eng, db, monkeypatch, st["exhaustive"])


# ------------------------------------------------------------ B. domain windows and parent lists
WINDOW_ENVS = ["", "FSM_TSR_SPB=100000", "FSM_TSR_SPB=4", "FSM_TSR_PLSPB=100000"]


@pytest.mark.parametrize("env", WINDOW_ENVS, ids=lambda e: e or "default")
def test_domain_windows_and_parent_lists(eng, env, monkeypatch):
    """Family A on N = 1,023 .. 2,049 with the deciding sids on 1,023 / 1,024 / 2,047 / 2,048: the rules
    of support m get one block, whose domain (every sid) is one, two or three windows of k_exp_rows;
    FSM_TSR_SPB=100000 gives the big rules one block too, FSM_TSR_SPB=4 many blocks of a few rows,
    FSM_TSR_PLSPB=100000 walks each parent list (N - m rows, and exactly 1,023 / 1,024 / 1,025 in the
    plist DBs) in one block's windows."""
    setenv(monkeypatch, env)
    for name, db in E.tsr_window_cases().items():
        st = check_modes(eng, db)
        if not env:
            check_plist_evidence(eng, db, monkeypatch, st["exhaustive"])


# ------------------------------------------------------------ C. kid passes, the klo cut, reduce ranges
@pytest.mark.parametrize("env", ["", "FSM_TSR_PASS_KIDS=37"], ids=lambda e: e or "default")
@pytest.mark.parametrize("name", list(E.tsr_kid_cases()))
def test_kid_pass_and_reduce_range_edges(eng, name, env, monkeypatch):
    """tsr_long_rows behind 4,093 / 4,094 / 4,095 filler kids: lo_abs of the core rules falls on 4,095,
    4,096 (a pass start) and 4,097, the tight tail kids (support 7, one below the final minsup 8) on the
    pass edges, the first and last tail kid and 4,096 + 511 / + 512 (two reduce ranges of pass 1); and
    low = 0 with tight kids 511 / 512, 4,095 / 4,096 / 4,097, 8,191 / 8,192.  Under the default pass
    width and 37 kids per pass.  (No counter names the pass or range a record came from: the kids are
    proved on the CPU.)  Two k: 5 (final minsup 8, a tight kid counted once too often adds a rule) and the
    number of two-item rules at 7 and above (final minsup 7: rules of every tight kid at exactly 7)."""
    setenv(monkeypatch, env)
    db = E.tsr_kid_cases()[name]
    for mode, k, final in E.tsr_kid_modes(db):
        st = check_tsr(eng, db, mode, k, final)
        assert st["exp_entries"] > db.N * 4096  # the long rows exceed a chunk


# ------------------------------------------------------------ D. operand rounds and full batches
CHAIN_ENVS = ["", "FSM_TSR_DOMAIN=bitmap", "FSM_TSR_DOMAIN=list", "FSM_TSR_PLIST=0", "FSM_TSR_DLMEMO=0"]


@pytest.mark.parametrize("env", CHAIN_ENVS, ids=lambda e: e or "default")
def test_operand_rounds_and_full_batches(eng, env, monkeypatch):
    """Chains <{1}, ..., {n}> (n = 5, 9, 10) with two reversed sequences in every domain: rules of up to n
    items (DomProbe takes 4 per round, k_exp_domain 8 operands), 8,194 rules at n = 10 (more than 20
    launches of full batches, the slot search at both ends), and the DB whose pair phase ends at
    kWideMinsup (wide batches) or one below, by k.  With the parent lists on, a child probes only the item
    it added, so DomProbe's later rounds run under FSM_TSR_PLIST=0, and k_exp_domain's split of a sid
    list under FSM_TSR_DOMAIN=list."""
    setenv(monkeypatch, env)
    for name, (db, modes) in E.tsr_chain_cases().items():
        st = check_modes(eng, db, modes)
        if env == "FSM_TSR_PLIST=0" and "exhaustive" in st:
            allr = E.tsr_all_rules(db)
            assert st["exhaustive"]["exp_domain"] == E.tsr_domain_sum(db, allr), name


# ------------------------------------------------------------ E. pair phase
@pytest.mark.parametrize("env", ["", "FSM_TSR_PAIR_RECS=64"], ids=lambda e: e or "default")
def test_pair_phase_batch_edges(eng, env, monkeypatch):
    """600 kept items; the only rules are pairs i => j / j => i at support m or m - 1 with i the last item
    of a pair batch and the first of the next (15 / 16 ... 495 / 496) and j at i + 1, i + 63 / 64 / 65
    (k_pairs_compact's 64-lane steps) and the last item."""
    setenv(monkeypatch, env)
    db = E.tsr_pair_case()
    st = check_modes(eng, db)
    assert st["tight"]["exp_domain"] > 0


# ------------------------------------------------------------ knobs are per mine
def test_knobs_are_read_per_mine(fsm, eng, monkeypatch):
    """One engine, one resident DB (family B, N = 1,023, tight mode), mined five times: default,
    FSM_TSR_BATCH=1, default, FSM_TSR_MAX_KIDS=0, default.  Every mine sees the environment as it is
    when it starts: one rule per launch takes more launches than the default batch, no kept item
    allowed on the bitmap path reads no bitmap (the list path), and the default mines in between
    are untouched by either (all their counters equal; the ms_* fields are clock readings)."""
    db = E.tsr_window_cases()["N%d" % (E.tsr_constants()["exp_win"] - 1)]
    mode, k, final = E.tsr_modes(db)[1]
    o = tsr_ref(db, k)
    assert o["final_minsup"] == final
    h = eng.db_from_tokens(db.sids, db.seq_off, db.tokens, fsm.MODE_TSR)
    stats = []
    try:
        for env in ("", "FSM_TSR_BATCH=1", "", "FSM_TSR_MAX_KIDS=0", ""):
            with monkeypatch.context() as mp:
                setenv(mp, env)
                rules, meta = eng.tsr(h, k, db.minconf)
            rules.sort(key=lambda t: (-t[2], t[0], t[1]))
            assert rules == o["rules"], env
            assert meta["final_minsup"] == final, env
            stats.append({n: v for n, v in eng.stats().items() if not n.startswith("ms_")})
    finally:
        h.free()
    default, batch1, default2, no_kids, default3 = stats
    assert batch1["count_launches"] > default["count_launches"]
    assert no_kids["exp_bitmap_bytes"] == 0
    assert all(st["exp_bitmap_bytes"] > 0 for st in (default, batch1, default2, default3))
    assert default == default2 == default3


# ------------------------------------------------------------ F. in-process ranks
@pytest.mark.parametrize("shard_min", ["0", ""], ids=["shard-every-launch", "shard-default"])
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=lambda d: "ranks%d" % len(d))
def test_inproc_ranks_on_tsr_edges(fsm, devices, shard_min, monkeypatch):
    """Families A (deciding sids also on the pair phase's sid cuts N r / R - 1 and N r / R), B, C and E
    over two and three in-process ranks: the sharded pair phase and, with FSM_TSR_SHARD_MIN=0, every
    launch's slots split over the ranks."""
    if shard_min:
        monkeypatch.setenv("FSM_TSR_SHARD_MIN", shard_min)
    sizes = E.probe_sizes()
    with fsm.Engine(devices=list(devices)) as e:
        for N in (sizes[3], sizes[1]):
            check_modes(e, E.tsr_probe_cases()["N%d-cuts" % N])
        check_modes(e, E.tsr_window_cases()["N%d" % (2 * E.tsr_constants()["exp_win"] + 1)])
        kid_db = E.tsr_kid_cases()["low%d" % (E.tsr_constants()["kPassKids"] - 2)]
        check_modes(e, kid_db, E.tsr_kid_modes(kid_db))
        check_modes(e, E.tsr_pair_case())
