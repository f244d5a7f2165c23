"""GPU parity on the kernels' geometry constants, with threshold-tight DBs.

The DBs come from tests/edge_dbs.py: every candidate counter sits exactly at
minsup or exactly one below, so a count, emit or F2 kernel that is off by one
anywhere changes the frequent set; and each DB is placed on a constant the
kernels branch on (row and run lengths 63 / 64 / 65, run starts around the
wave ranges, tile and mode-switch row counts, mask widths up to 1,024 words
and every word boundary of a mask,
TSR rows longer than one chunk, deciding sids on word and group boundaries).
tests/test_edge_dbs.py proves those claims on the same objects without a GPU.

Every SPADE case compares patterns, the join count and root_entries, every TSR
case rules and final minsup, with the CPU oracle (or the generator's closed
form where noted); the K0 cases compare both fsm_db_export images with the
image written from the token rules by definition (edge_dbs.k0_image)."""
import numpy as np
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


def gpu_spade(eng, db, text=False):
    from spark_fsm_amd import MODE_SPADE
    if text:
        h = eng.db_from_spmf(db.records(), MODE_SPADE)
    else:
        h = eng.db_from_tokens(db.sids, db.seq_off, db.tokens, MODE_SPADE)
    k0 = eng.stats()["k0_device"]
    try:
        pats, meta = eng.spade(h, db.support)
    finally:
        h.free()
    st = eng.stats()
    st["k0_device"] = k0
    return sorted(pats), meta, st


def gpu_tsr(eng, db, k, minconf, text=False):
    from spark_fsm_amd import MODE_TSR
    if text:
        h = eng.db_from_spmf(db.records(), MODE_TSR)
    else:
        h = eng.db_from_tokens(db.sids, db.seq_off, db.tokens, MODE_TSR)
    try:
        rules, meta = eng.tsr(h, k, minconf)
    finally:
        h.free()
    rules.sort(key=lambda t: (-t[2], t[0], t[1]))
    return rules, meta, eng.stats()


_ORACLE = {}


def spade_ref(db, closed=False, minsup=2):
    """The oracle's answer for a DB, computed once per session and left unchanged.  closed: the
    generator's closed form (edge_dbs.closed_form_ref) for the DBs of 8,192 and more frequent
    items, which the oracle takes 3 to 12 s each to mine.  minsup: what the DB is mined at (the
    tall DBs of edge_dbs.tall_spade state their own; they list decisions, not a closed form)."""
    if id(db) not in _ORACLE:
        from oracle import oracle
        if closed:
            o = E.closed_form_ref(db)
        else:
            o = oracle.spade_tokens(db.seq_off, db.tokens, db.support)
        assert o["minsup"] == minsup, db.name
        if isinstance(db, E.TallSpade):
            got = dict(o["patterns"])
            assert all(got.get(p) == db.S for p in db.t2) and not any(p in got for p in db.t1), db.name
        else:
            assert o["patterns"] == db.expected(), db.name  # the closed form agrees
        _ORACLE[id(db)] = (db, o)
    return _ORACLE[id(db)][1]


def tsr_ref(db, k, minconf):
    key = (id(db), k, minconf)
    if key not in _ORACLE:
        from oracle import oracle
        _ORACLE[key] = (db, oracle.tsr(db.records(), k, minconf))
    return _ORACLE[key][1]


def check_spade(eng, db, text=False, closed=False, root=True, minsup=2):
    o = spade_ref(db, closed, minsup)
    pats, meta, st = gpu_spade(eng, db, text)
    assert meta["minsup"] == minsup, db.name
    if pats != o["patterns"]:
        got, exp = dict(pats), dict(o["patterns"])
        diff = [(p, got.get(p), exp.get(p)) for p in sorted(set(got) | set(exp)) if got.get(p) != exp.get(p)]
        raise AssertionError("%s: %d patterns differ (pattern, GPU, oracle): %r" % (db.name, len(diff), diff[:6]))
    assert st["joins"] == o["joins"], db.name
    if root:
        assert st["root_entries"] == db.root_entries(), db.name
    return st


def setenv(monkeypatch, env):
    for kv in env.split():
        k, v = kv.split("=")
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------ 1. root F2 row lengths
@pytest.mark.parametrize("env", ["", "FSM_F2_TRI=0", "FSM_ROOT_DB=0", "FSM_ROOT_PATH=atomic"], ids=lambda e: e or "default")
def test_root_f2_row_lengths(eng, env, monkeypatch):
    """Hub rows of 1..129 entries (k_f2_tri: folded for n + 1 <= 64, unfolded at
    n = 64, the wave-uniform walk above; odd rows fold their middle entry onto
    itself), rows that pass 64 entries only with their infrequent items, and an
    item placed twice, under the unordered F2, the ordered one (k_f2_keys), the
    root slab and the atomic root."""
    setenv(monkeypatch, env)
    for name, db, row_len in E.f2_cases():
        g = E._cached(("f2geo", name), lambda: E.geometry(db.rows, 2, classes=False))
        for h, n in row_len.items():
            assert E.hub_run(db, g, h, "db")[1] == n
        check_spade(eng, db)
        check_spade(eng, db, text=True)


# ------------------------------------------------------------ 2. lattice windows
LATTICE_ENVS = ["", "FSM_COUNT_PATH=keys", "FSM_COUNT_PATH=atomic FSM_COUNT_KERNEL=thread", "FSM_EMIT_PATH=chunk",
                "FSM_EMIT_CAP=17", "FSM_COUNT_PATH=sparse"]


@pytest.mark.parametrize("env", LATTICE_ENVS, ids=lambda e: e.replace(" ", ",") or "default")
@pytest.mark.parametrize("w", [1, 2, 4, 8])
def test_lattice_windows(eng, w, env, monkeypatch):
    """Runs of 63..66 entries and of 127..257 (the long-run list) in [A1] and
    [A1 -> A2]; a 64-entry run starting 63 before, one before and on every
    multiple of 64 up to 512 (the wave ranges of k_emit2: root 128, W = 1
    lattice 192, W > 1 lattice 64, and of k_count2: 256) in [A1] and in the
    root; a hub that is the last run (it ends at E).  W = 1, 2, and 4 and 8 (the
    other two instantiations of k_emit2 / k_count2), where every hub is stretched
    over the whole mask: its entries' bits lie in every word."""
    setenv(monkeypatch, env)
    for name, db, level, claim in E.lattice_cases(w):
        E._cached(("latgeo", w, name), lambda: E.check_lattice_claim(db, level, claim) and True)
        st = check_spade(eng, db)
        assert st["mask_words"] == w, name


# ------------------------------------------------------------ 3. row-table sizes
@pytest.mark.parametrize("env", ["", "FSM_DEVORDER=0"], ids=lambda e: e or "default")
def test_row_table_sizes(eng, env, monkeypatch):
    """2,047 / 2,048 / 2,049 / 4,096 / 4,097 counter rows in the root batch and
    in the first-level batch (k_rk_tables tiles 2,048 rows; each block sums what
    precedes its tile)."""
    setenv(monkeypatch, env)
    for name, db, f_root, f_l1 in E.rk_cases():
        if f_root > 5000:
            continue
        assert len(db.singles) + len(db.prefix_items) == f_root and f_root - 1 + len(db.selected) == f_l1
        check_spade(eng, db)


def test_freq_recs_mode_switch(eng):
    """16,385 counter rows: one more than the one-pass extraction takes (root
    batch, and first-level batch).  Compared with the generator's closed form, not with a
    mine of the oracle (12 s per DB here); the closed form is checked against the oracle at
    smaller sizes in tests/test_edge_dbs.py."""
    for name, db, f_root, f_l1 in E.rk_cases():
        if f_root > 5000:
            assert E.FREQ_RECS_ROWS in (f_root, f_l1)
            check_spade(eng, db, closed=True)


@pytest.mark.parametrize("env", ["", "FSM_F2_TRI=0", "FSM_ROOT_DB=0"], ids=lambda e: e or "default")
def test_root_f2_one_row_per_group(eng, env, monkeypatch):
    """8,192 / 8,193 / 10,923 / 10,924 / 16,384 frequent items: from 8,193 on a root counter row takes
    more than half a rank group, so the ordered root F2 (k_f2_keys; the default above the
    unordered layout's limit, and FSM_F2_TRI=0 / the root slab below it) keeps one row per group
    and the rank -> group multiplier is 2^32.  (This test found it held as 0: every row went to
    group 0, and k_f2_count's LDS counters were indexed past their 32,768.)"""
    setenv(monkeypatch, env)
    for F, db in E.one_row_group_cases():
        assert len(db.singles) + len(db.prefix_items) == F
        check_spade(eng, db, closed=True)


# ------------------------------------------------------------ 4. mask widths
@pytest.mark.parametrize("E_W", list(zip(E.MASK_E, E.MASK_W)), ids=lambda x: "E%d" % x[0])
def test_mask_widths(eng, E_W):
    """Exactly E itemsets in one sequence, planted items on eids 0, 1, 63, 64,
    E - 2, E - 1: the mask widths on both sides of each power of two up to the
    widest legal mask (65,536 eids, W = 1,024, last eid 0xFFFF).  Text path and
    token path; the device build takes up to 4,096 eids."""
    Ee, W = E_W
    db = [d for e, _, d in E.mask_cases() if e == Ee][0]
    st = check_spade(eng, db, text=True)
    assert st["mask_words"] == W
    st = check_spade(eng, db)
    assert st["mask_words"] == W
    assert st["k0_device"] == (1 if Ee <= 4096 else 0)


SWEEP_ENVS = ["", "FSM_EMIT_PATH=chunk", "FSM_COUNT_PATH=atomic FSM_COUNT_KERNEL=thread", "FSM_COUNT_PATH=keys",
              "FSM_COUNT_PATH=sparse", "FSM_ROOT_DB=0", "FSM_EMIT_CAP=0"]
# k_emit2, k_count2 and the DB-direct root exist at W = 1, 2, 4, 8: from 16 words on FSM_EMIT_PATH=chunk and
# FSM_ROOT_DB=0 select what the default runs already (FSM_COUNT_PATH=atomic still forces the count path)
SWEEP_CASES = [(W, env) for W in E.SWEEP_W for env in SWEEP_ENVS
               if W <= 8 or env not in ("FSM_EMIT_PATH=chunk", "FSM_ROOT_DB=0")]


def check_sweep(eng, db, text):
    """check_spade; a failure names the word boundaries (and gadgets) of the differing patterns."""
    o = spade_ref(db)
    try:
        return check_spade(eng, db, text=text)
    except AssertionError as err:
        pats, _, _ = gpu_spade(eng, db, text)
        got, exp = dict(pats), dict(o["patterns"])
        diff = [p for p in set(got) | set(exp) if got.get(p) != exp.get(p)]
        raise AssertionError("%s: (word boundary, gadget) of the %d differing patterns: %r; %s"
                             % (db.name, len(diff), db.words_of(diff), err)) from None


@pytest.mark.parametrize("W,env", SWEEP_CASES, ids=lambda x: x if isinstance(x, int) else x.replace(" ", ",") or "default")
def test_mask_word_sweep(eng, W, env, monkeypatch):
    """One decision (support exactly 2 or exactly 1) on every word boundary of the mask at the
    register-held widths 2 .. 64, and on boundaries 1, 2, 63, 64, 65, W / 2 - 1, W / 2, W - 1 at
    the runtime widths 128 .. 1,024 (edge_dbs.word_sweep_db): temporal and equality counts whose
    deciding bit is the first of word k, temporal children cleared up to the last bit of word
    k - 1 or the first of word k whose new lo lies in word k or k + 1, children of equality
    joins, and joins that read those children's masks and lo / hi.  Token path and text path."""
    setenv(monkeypatch, env)
    db = E.sweep_case(W)
    for text in (False, True):
        st = check_sweep(eng, db, text)
        assert st["mask_words"] == W
        if not text:  # the device build takes rows of up to 8,192 tokens and 4,096 eids: S at W = 64 is longer
            assert st["k0_device"] == (1 if db.E <= 4096 and len(db.rows[0]) <= 8192 else 0)


@pytest.mark.parametrize("W", E.SWEEP_W)
def test_mask_word_sweep_supports(eng, W):
    """k_ps_count on the same words: the support of every decision of the sweep, given as a
    pattern, is 2 where S holds it and 1 where it does not."""
    from spark_fsm_amd import MODE_SPADE
    db = E.sweep_case(W)
    h = eng.db_from_tokens(db.sids, db.seq_off, db.tokens, MODE_SPADE)
    try:
        got = eng.pattern_supports(h, db.t2 + db.t1).tolist()
    finally:
        h.free()
    want = [2] * len(db.t2) + [1] * len(db.t1)
    bad = [(db.boundary[p], db.gadget[p], g, w) for p, g, w in zip(db.t2 + db.t1, got, want) if g != w]
    assert not bad, "W = %d: (word boundary, gadget, GPU, expected): %r" % (W, bad[:8])


# ------------------------------------------------------------ 5. a DB row of 65,535 / 65,536 entries
@pytest.mark.parametrize("n", [65535, 65536])
def test_db_row_of_64k_entries(eng, n):
    """Three frequent items in a row of n distinct items: above 65,535 entries
    the offset-in-row field does not hold the row and the mine keeps the root slab."""
    db = [d for m, d in E.big_row_cases() if m == n][0]
    check_spade(eng, db, text=True)
    check_spade(eng, db)


# ------------------------------------------------------------ 6. in-process ranks
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=lambda d: "ranks%d" % len(d))
def test_inproc_ranks_on_edges(fsm, devices):
    """Families 1 and 2 under in-process ranks: each rank's F2 takes a member
    sub-range [a0, a1) of every row (k_f2_tri's fold over an active sub-range)."""
    with fsm.Engine(devices=list(devices)) as e:
        # (root_entries is left out: with the root rows shared among ranks, whose figure the stats
        # report is not part of the contract)
        for name, db, _ in E.f2_cases():
            check_spade(e, db, root=False)
        for name, db, level, claim in E.lattice_cases(1):
            if name == "lengths" or name == "hub-last" or name.endswith(("start1", "start127", "start128", "start192")):
                check_spade(e, db, root=False)


# ------------------------------------------------------------ 7. TSR
@pytest.mark.parametrize("name", [c[0] for c in E.tsr_long_cases()])
def test_tsr_rows_longer_than_a_chunk(eng, name):
    """Rows of T tail items past the rule's items (k_exp_rows walks a row of
    more than 4,096 kept entries by its own branch): five rules at the final
    minsup 8, tail rules one below."""
    _, db, k, mc = [c for c in E.tsr_long_cases() if c[0] == name][0]
    o = tsr_ref(db, k, mc)
    rules, meta, st = gpu_tsr(eng, db, k, mc)
    assert rules == o["rules"] and meta["final_minsup"] == o["final_minsup"] == 8
    if db.T > 4096:
        assert st["exp_entries"] > db.N * 4096


TSR_ENVS = ["", "FSM_TSR_DOMAIN=bitmap", "FSM_TSR_DOMAIN=list", "FSM_TSR_PLIST=0"]


@pytest.mark.parametrize("env", TSR_ENVS, ids=lambda e: e or "default")
def test_tsr_deciding_sids(eng, env, monkeypatch):
    """Two rules one support apart; the sequences that decide sit at sids 31 /
    32, 127 / 128, 1,023 / 1,024, 32,767 / 32,768 and N - 1, for N on both sides
    of each: k = 1 returns the winner alone, k = 2 both."""
    setenv(monkeypatch, env)
    for N, db in E.tsr_sid_cases():
        for k in (1, 2):
            o = tsr_ref(db, k, 0.0)
            rules, meta, _ = gpu_tsr(eng, db, k, 0.0)
            assert rules == o["rules"] and meta["final_minsup"] == o["final_minsup"], (N, k)
            assert len(rules) == k


@pytest.mark.parametrize("last_index", [65535, 65536])
def test_tsr_itemset_index_limit(eng, last_index):
    """A last itemset index of 65,535 fits the packed rows' 16-bit fields; 65,536
    takes the list path.  Empty itemsets count."""
    db = E._cached(("deep", last_index), lambda: E.tsr_deep_index(last_index))
    for k in (1, 3, 10):
        o = tsr_ref(db, k, 0.0)
        for text in (False, True):
            rules, meta, _ = gpu_tsr(eng, db, k, 0.0, text=text)
            assert rules == o["rules"] and meta["final_minsup"] == o["final_minsup"]


# ------------------------------------------------------------ 8. K0 against the definition
def _assert_image(img, ref, name):
    for key, want in ref.items():
        got = img[key]
        if isinstance(want, np.ndarray):
            assert got.shape == want.shape and np.array_equal(got.astype(want.dtype), want), (name, key)
        else:
            assert got == want, (name, key)


@pytest.mark.parametrize("name", [c[0] for c in E.k0_cases()])
def test_k0_image_by_definition(eng, fsm, name, monkeypatch):
    """Both DB builds (the device build and FSM_K0=host) against the image
    written from the token rules in plain Python: rows on the wave / block /
    host switches (64 / 65, 8,192 / 8,193 tokens), one item in all 4,096
    itemsets, 16 items repeated through a row, item value ranges around the LDS
    bitmap (2^19) and the device limit (2^27), 4,096 / 4,097 eids."""
    _, rows, modes, dev = [c for c in E.k0_cases() if c[0] == name][0]
    db = E.EdgeDB(rows, name)
    for mode in modes:
        ref = E.k0_image(rows, mode)
        m = fsm.MODE_SPADE if mode == "spade" else fsm.MODE_TSR
        for k0 in ("device", "host"):
            if k0 == "host":
                monkeypatch.setenv("FSM_K0", "host")
            else:
                monkeypatch.delenv("FSM_K0", raising=False)
            h = eng.db_from_tokens(db.sids, db.seq_off, db.tokens, m)
            try:
                img = eng.db_export(h)
                used = eng.stats()["k0_device"]
            finally:
                h.free()
            assert used == (1 if dev and k0 == "device" else 0), (name, mode, k0)
            _assert_image(img, ref, (name, mode, k0))
