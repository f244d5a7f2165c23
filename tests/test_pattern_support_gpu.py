"""GPU tests of fsm_patterns_support (supports of given patterns in a resident SPADE DB):
the counts against the stated answers of tests/pattern_support_ref.py's generators, its two
references, and the supports the miner itself reports."""
import ctypes
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pattern_filter_ref as fref
import pattern_support_ref as ref
import spark_fsm_amd as fsm
from spark_fsm_amd import _lib
from tools import gen

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T = ref.constants()["kPsTile"]
MEDIUM = {"D": 200, "seed": 1, "support": 0.07, "n": 51490}  # as in test_pattern_filter_gpu.py
INDEX_ROWS = ["k_ps_index_hist", "k_scan", "k_ps_index_off", "k_ps_index_scatter"]


@pytest.fixture(scope="module")
def eng():
    with fsm.Engine(0) as e:
        yield e


def count(eng, records, patterns, mode=fsm.MODE_SPADE):
    db = eng.db_from_spmf(records, mode)
    try:
        got = eng.pattern_supports(db, patterns)
        assert got.dtype == np.int32 and got.shape == (len(patterns),)
        return got.tolist()
    finally:
        db.free()


def check_case(eng, case, definition=True):
    got = count(eng, case["records"], case["patterns"])
    assert got == case["expected"]
    if definition:
        assert got == ref.by_definition(case["records"], case["patterns"])


# ------------------------------------------------------------------ 1. hand cases
@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_hand_cases(eng, name):
    check_case(eng, ref.hand_cases()[name])


def test_input_forms_support_none_and_the_empty_set(eng):
    case = ref.hand_cases()["itemset_vs_sequence"]
    pats, exp = case["patterns"], case["expected"]
    db = eng.db_from_spmf(case["records"], fsm.MODE_SPADE)
    try:
        csr = ref.to_csr(pats)
        assert csr[0] is None
        assert eng.pattern_supports(db, csr).tolist() == exp
        assert eng.pattern_supports(db, ref.to_csr(pats, support=[99] * len(pats))).tolist() == exp  # ignored
        assert eng.pattern_supports(db, list(pats)).tolist() == exp
        assert eng.pattern_supports(db, [(p, 1234) for p in pats]).tolist() == exp
        assert fsm.pattern_supports(db, pats).tolist() == exp
        assert fsm.pattern_supports(case["records"], pats, engine=eng).tolist() == exp
        for empty in ([], ref.to_csr([])):
            got = eng.pattern_supports(db, empty)
            assert got.dtype == np.int32 and got.shape == (0,)
    finally:
        db.free()


def _raw(eng, db, csr, out, n=None, n_items=None):
    po, so, it = (np.ascontiguousarray(a, dt) for a, dt in zip(csr[1:], (np.int64, np.int64, np.int32)))
    P = ctypes.POINTER
    pats = _lib.Patterns(len(po) - 1 if n is None else n, None, po.ctypes.data_as(P(ctypes.c_int64)),
                         so.ctypes.data_as(P(ctypes.c_int64)), it.ctypes.data_as(P(ctypes.c_int32)), len(so) - 1,
                         len(it) if n_items is None else n_items, 0, 0)
    return eng._L.fsm_patterns_support(eng._ctx, db.handle, ctypes.byref(pats), out.ctypes.data_as(P(ctypes.c_int32)))


def test_errors_leave_the_output_and_the_statistics(eng):
    case = ref.hand_cases()["itemset_vs_sequence"]
    good = ref.to_csr(case["patterns"])
    db = eng.db_from_spmf(case["records"], fsm.MODE_SPADE)
    tdb = eng.db_from_spmf(case["records"], fsm.MODE_TSR)
    try:
        eng.spade(db, 0.2)
        before = eng.stats()
        out = np.full(len(case["patterns"]), -7, np.int32)
        bad = {
            "descending_itemset": (None, [0, 1, 2], [0, 2, 3], [2, 1, 1]),
            "equal_items": (None, [0, 1, 2], [0, 2, 3], [1, 1, 1]),
            "pattern_without_itemsets": (None, [0, 1, 1, 2], [0, 1, 2], [1, 2]),
            "empty_itemset": (None, [0, 1, 2], [0, 0, 2], [1, 2]),
            "pat_off_not_monotone": (None, [0, 2, 1, 3], [0, 1, 2, 3], [1, 2, 1]),
            "set_off_not_monotone": (None, [0, 1, 2, 3], [0, 2, 1, 3], [1, 2, 1]),
        }
        for name, csr in bad.items():
            assert _raw(eng, db, csr, out) == _lib.FSM_EINVAL, name
            assert eng._L.fsm_last_error(eng._ctx), name
            with pytest.raises(fsm.FsmError) as e:
                eng.pattern_supports(db, tuple(None if a is None else np.array(a) for a in csr))
            assert e.value.code == _lib.FSM_EINVAL, name
        assert _raw(eng, db, good, out, n=-1) == _lib.FSM_EINVAL
        assert _raw(eng, db, good, out, n=(1 << 32) - 2) == _lib.FSM_ELIMIT
        assert _raw(eng, db, good, out, n_items=(1 << 32) - 2) == _lib.FSM_ELIMIT
        assert _raw(eng, tdb, good, out) == _lib.FSM_EINVAL  # a TSR-mode DB
        with pytest.raises(fsm.FsmError) as e:
            eng.pattern_supports(tdb, case["patterns"])
        assert e.value.code == _lib.FSM_EINVAL
        assert eng._L.fsm_patterns_support(eng._ctx, db.handle, None, None) == _lib.FSM_EINVAL
        assert out.tolist() == [-7] * len(out)
        # a following valid call still works, and fsm_stats is left as the mine set it
        assert _raw(eng, db, good, out) == _lib.FSM_OK and out.tolist() == case["expected"]
        assert eng.stats() == before
        ks = eng.kernel_stats()
        assert [k["name"] for k in ks] == INDEX_ROWS + ["k_ps_count"]
        assert all(k["alg_bytes"] > 0 and k["launches"] == 1 for k in ks)
    finally:
        db.free()
        tdb.free()


# ------------------------------------------------------------------ 2. round trip on random DBs
@pytest.mark.parametrize("seed", range(fref.N_RANDOM))
def test_round_trip_on_random_dbs(eng, seed):
    recs, sup, complete = fref.mined_random_db(seed)
    db = eng.db_from_spmf(recs, fsm.MODE_SPADE)
    try:
        mined, _ = eng.spade(db, sup)
        assert sorted(mined) == complete
        assert eng.pattern_supports(db, mined).tolist() == [s for _p, s in mined]
        # every pattern of up to 3 items, the infrequent ones included (15 of the 20 DBs have some)
        pats = ref.small_patterns(ref.items_of(recs))
        assert eng.pattern_supports(db, pats).tolist() == ref.by_definition(recs, pats)
    finally:
        db.free()


# ------------------------------------------------------------------ 3. tile edges
@pytest.mark.parametrize("L", ref.tile_lengths(T))
def test_tile_edges(eng, L):
    for place in ref.PIVOT_PLACES:
        for full in (True, False):
            case = ref.tile_edge_case(L, place, full)
            assert case["expected"] == [L if full else L - 1]
            check_case(eng, case, definition=False)  # (the CPU test holds the generator to the definition)


def test_short_and_long_lists_share_a_launch(eng):
    check_case(eng, ref.shared_launch_case(T))


# ------------------------------------------------------------------ 4. row lengths
@pytest.mark.parametrize("n", ref.ROW_LENGTHS)
def test_row_lengths_of_the_in_row_search(eng, n):
    case = ref.row_length_case(n)
    db = eng.db_from_spmf(case["records"], fsm.MODE_SPADE)
    try:
        img = eng.db_export(db)
        assert np.diff(img["row_off"])[:2].tolist() == [n, n] and img["mask_words"] == 1
        assert eng.pattern_supports(db, case["patterns"]).tolist() == case["expected"]
    finally:
        db.free()


# ------------------------------------------------------------------ 5. mask widths
@pytest.mark.parametrize("W", ref.MASK_WIDTHS)
def test_mask_widths(eng, W):
    case = ref.mask_width_case(W)
    db = eng.db_from_spmf(case["records"], fsm.MODE_SPADE)
    try:
        assert eng.db_export(db)["mask_words"] == W
        assert eng.pattern_supports(db, case["patterns"]).tolist() == case["expected"]
    finally:
        db.free()


def test_wide_mask_db_of_the_edge_tests(eng):
    import edge_dbs
    edb = edge_dbs.wide_mask_db(129)  # W = 4; items 1..7 planted at eids 0, 1, 63, 64, 127, 128, 128
    # only the long sequence holds these; then the generator's own closed-form counts
    pats = [((1,), (2,), (3,), (4,), (5,), (6,)), ((4,), (3,)), ((5,), (6, 7)), ((6,), (7,))]
    exp = [1, 0, 1, 0]
    for p, s in edb.expected():
        pats.append(p)
        exp.append(s)
    assert ((3,), (4,)) in pats and ((6, 7),) in pats and len(pats) == 4 + 8 + 6
    db = eng.db_from_tokens(edb.sids, edb.seq_off, edb.tokens, fsm.MODE_SPADE)
    try:
        assert eng.db_export(db)["mask_words"] == 4
        got = eng.pattern_supports(db, pats).tolist()
        assert got == exp == ref.by_oracle(edb.seq_off, edb.tokens, pats)
    finally:
        db.free()


# ------------------------------------------------------------------ 6. long pattern
def test_pattern_of_3000_itemsets(eng):
    case = ref.long_pattern_case(3000)
    got = count(eng, case["records"], case["patterns"])
    assert got == case["expected"] == [3, 5]
    # on a DB of 64 eids the same patterns cannot match
    small = ref.hand_cases()["duplicates"]["records"]
    assert count(eng, small, case["patterns"]) == [0, 0]


# ------------------------------------------------------------------ 7. medium
def test_medium_recount_and_new_data(eng):
    from oracle import oracle  # noqa: F401  (by_oracle's library)
    ds = gen.sign(D=MEDIUM["D"], seed=MEDIUM["seed"])
    db = eng.db_from_tokens(ds.sids, ds.seq_off, ds.tokens, fsm.MODE_SPADE)
    try:
        csr, meta = eng.spade_csr(db, MEDIUM["support"], copy=True)
        assert meta["n"] == MEDIUM["n"]
        got = eng.pattern_supports(db, csr)
        assert np.array_equal(got, csr[0])
    finally:
        db.free()
    ds2 = gen.sign(D=MEDIUM["D"], seed=2)
    db2 = eng.db_from_tokens(ds2.sids, ds2.seq_off, ds2.tokens, fsm.MODE_SPADE)
    try:
        got2 = eng.pattern_supports(db2, (None,) + tuple(csr[1:]))
    finally:
        db2.free()
    assert got2.shape == (MEDIUM["n"],) and int(got2.max()) <= MEDIUM["D"] and int(got2.min()) >= 0
    sample = sorted(random.Random(51490).sample(range(MEDIUM["n"]), 300))
    pats = ref.csr_patterns(fref.take(csr, sample))
    assert got2[sample].tolist() == ref.by_oracle(ds2.seq_off, ds2.tokens, pats)


# ------------------------------------------------------------------ 8. builds and contexts
def test_builds_and_contexts_agree(eng):
    ds = gen.quest(2000, seed=1)
    db = eng.db_from_tokens(ds.sids, ds.seq_off, ds.tokens, fsm.MODE_SPADE)
    try:
        assert eng.stats()["k0_device"]
        csr, _meta = eng.spade_csr(db, 0.01, copy=True)
        assert len(csr[0]) > 100
        first = eng.pattern_supports(db, csr)
        rows1 = [k["name"] for k in eng.kernel_stats()]
        again = eng.pattern_supports(db, csr)
        rows2 = [k["name"] for k in eng.kernel_stats()]
    finally:
        db.free()
    assert np.array_equal(first, csr[0]) and np.array_equal(again, first)
    assert rows1 == INDEX_ROWS + ["k_ps_count"] and rows2 == ["k_ps_count"]  # the index is reused
    db = eng.db_from_spmf(ds.records(), fsm.MODE_SPADE)
    try:
        assert not eng.stats()["k0_device"]
        assert np.array_equal(eng.pattern_supports(db, csr), first)
    finally:
        db.free()
    with fsm.Engine(devices=[0, 0]) as grp:
        gdb = grp.db_from_tokens(ds.sids, ds.seq_off, ds.tokens, fsm.MODE_SPADE)
        try:
            assert np.array_equal(grp.pattern_supports(gdb, csr), first)
            assert [k["name"] for k in grp.kernel_stats()] == INDEX_ROWS + ["k_ps_count"]
        finally:
            gdb.free()


# ------------------------------------------------------------------ 9. forced pivot
@pytest.fixture(scope="module")
def default_counts(eng):
    return ref.count_cases(eng, ref.child_cases())


@pytest.mark.parametrize("hook", ["FSM_PS_PIVOT=first", "FSM_PS_PIVOT=last", "FSM_PS_SLICE_TILES=3"])
def test_forced_pivot_and_launch_slices(default_counts, hook):
    """FSM_PS_PIVOT overrides the pivot choice, FSM_PS_SLICE_TILES the tiles per launch: either
    may change the speed, never a count."""
    key, val = hook.split("=")
    env = dict(os.environ)
    env[key] = val
    r = subprocess.run([sys.executable, os.path.join(HERE, "pattern_support_ref.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    cases = ref.child_cases()
    assert sorted(got) == sorted(cases) and len(got) == fref.N_RANDOM + 6 * 4 * 2 + 1
    for name in cases:
        assert got[name] == default_counts[name], name
    tiles = ref.tile_cases(T)
    for name, case in tiles.items():
        assert got[name] == case["expected"], name
