"""GPU tests of fsm_patterns_sids (the sequence ids of the rows that hold given patterns in a
resident SPADE DB): the lists against the definition (tests/pattern_sids_ref.py), the stated
lists of the generators, the supports the miner and fsm_patterns_support report, and the
call's contract on errors, caps, hooks, statistics and contexts."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pattern_filter_ref as fref
import pattern_sids_ref as sref
import pattern_support_ref as ref
import spark_fsm_amd as fsm
from spark_fsm_amd import _lib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T = ref.constants()["kPsTile"]
INDEX_ROWS = ["k_ps_index_hist", "k_scan", "k_ps_index_off", "k_ps_index_scatter"]
ORDER_ROW = "k_ps_index_order"
CALL_ROWS = ["k_ps_match", "k_scan", "k_ps_sids_write"]


@pytest.fixture(scope="module")
def eng():
    with fsm.Engine(0) as e:
        yield e


def lists_of(eng, records, patterns, **kw):
    db = eng.db_from_spmf(records, fsm.MODE_SPADE)
    try:
        off, sid = eng.pattern_sids(db, patterns, **kw)
        assert off.shape == (len(patterns) + 1,)
        return sref.split(off, sid)
    finally:
        db.free()


def names(eng):
    return [k["name"] for k in eng.kernel_stats()]


# ------------------------------------------------------------------ E1. hand cases
@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_hand_cases(eng, name):
    case = ref.hand_cases()[name]
    got = lists_of(eng, case["records"], case["patterns"])
    assert got == sref.by_definition(case["records"], case["patterns"])
    assert [len(x) for x in got] == case["expected"]
    if name == "one_sid_two_records":
        assert got[0] == [7, 8]  # ids, not row numbers
    if name == "cannot_match":
        assert got == [[]] * 7 + [[0]]
        pats = case["patterns"]
        # empty lists at the start, in the middle and at the end of the input
        mixed = [pats[0], pats[7], pats[3], pats[5], pats[7], pats[2]]
        assert lists_of(eng, case["records"], mixed) == [[], [0], [], [], [0], []]
    if name == "duplicates":
        assert got[0] == got[2] == got[4] == [0, 1] and got[1] == got[3] == [0, 1, 2]


def test_input_forms_views_and_the_empty_set(eng):
    case = ref.hand_cases()["itemset_vs_sequence"]
    pats = case["patterns"]
    exp = sref.by_definition(case["records"], pats)
    db = eng.db_from_spmf(case["records"], fsm.MODE_SPADE)
    try:
        for form in (ref.to_csr(pats), ref.to_csr(pats, support=[99] * len(pats)), list(pats), [(p, 12) for p in pats]):
            assert sref.split(*eng.pattern_sids(db, form)) == exp
        off, sid = eng.pattern_sids(db, pats)
        assert not off.flags.writeable and not sid.flags.writeable
        off2, sid2 = eng.pattern_sids(db, pats, copy=True)
        assert off2.flags.writeable and sid2.flags.writeable and sref.split(off2, sid2) == exp
        assert fsm.pattern_sids(db, pats) == exp
        assert fsm.pattern_sids(case["records"], pats, engine=eng) == exp
        for empty in ([], ref.to_csr([])):
            off, sid = eng.pattern_sids(db, empty)
            assert off.tolist() == [0] and off.dtype == np.int64 and sid.shape == (0,) and sid.dtype == np.int32
    finally:
        db.free()


# ------------------------------------------------------------------ E2. ids are not row indexes
def test_ids_are_the_callers_not_row_indexes_in_both_builds(eng):
    case = sref.sid_case()
    assert [s for s, _ in case["text"]] == sorted((s for s, _ in case["text"]), reverse=True)
    db = eng.db_from_spmf(case["text"], fsm.MODE_SPADE)  # the host flatten (descending sids, a shared sid)
    try:
        assert not eng.stats()["k0_device"]
        host = sref.split(*eng.pattern_sids(db, case["patterns"]))
    finally:
        db.free()
    sids, seq_off, tokens = case["tokens"]
    assert sids.tolist() == [3, 9, 10, 1000, sref.I32_MAX]
    db = eng.db_from_tokens(sids, seq_off, tokens, fsm.MODE_SPADE)
    try:
        assert eng.stats()["k0_device"] == 1
        dev = sref.split(*eng.pattern_sids(db, case["patterns"]))
    finally:
        db.free()
    assert host == dev == case["expected"]
    assert all(1000 not in x for x in host)  # the record without any item is in no list


# ------------------------------------------------------------------ E3. tile edges
@pytest.mark.parametrize("L", ref.tile_lengths(T))
def test_tile_edges(eng, L):
    for place in ref.PIVOT_PLACES:
        for full in (True, False):
            case = ref.tile_edge_case(L, place, full)
            assert lists_of(eng, case["records"], case["patterns"]) == sref.tile_edge_lists(case), (place, full)


@pytest.mark.parametrize("shape", sref.LANE_SHAPES)
def test_survivor_lanes_of_a_tile_between_two_full_tiles(eng, shape):
    case = sref.lane_case(shape, T)
    assert lists_of(eng, case["records"], case["patterns"]) == case["expected"]


# ------------------------------------------------------------------ E4. dead patterns that own tiles
def test_patterns_without_survivors_that_own_tiles(eng):
    case = sref.dead_tiles_case(T)
    assert lists_of(eng, case["records"], case["patterns"]) == case["expected"]
    shared = ref.shared_launch_case(T)
    got = lists_of(eng, shared["records"], shared["patterns"])
    assert got == sref.by_definition(shared["records"], shared["patterns"])
    assert [len(x) for x in got] == shared["expected"]
    db = eng.db_from_spmf(case["records"], fsm.MODE_SPADE)
    try:
        off, sid = eng.pattern_sids(db, case["all_dead"])
        assert off.tolist() == [0] * (len(case["all_dead"]) + 1) and sid.shape == (0,)
        assert "k_ps_match" in names(eng) and "k_ps_sids_write" not in names(eng)  # tiles, and nothing to write
    finally:
        db.free()


# ------------------------------------------------------------------ E5. mask widths
@pytest.mark.parametrize("W", (1, 2, 128))
def test_mask_widths(eng, W):
    case = ref.mask_width_case(W)
    assert any(len(X) == 12 for p in case["patterns"] for X in p)
    db = eng.db_from_spmf(case["records"], fsm.MODE_SPADE)
    try:
        assert eng.db_export(db)["mask_words"] == W
        got = sref.split(*eng.pattern_sids(db, case["patterns"]))
    finally:
        db.free()
    assert got == [[0, 1] if e == 2 else [] for e in case["expected"]]


# ------------------------------------------------------------------ E6. order
def test_lists_ascend_whatever_the_input_order(eng):
    case = sref.order_case(T)
    db = eng.db_from_spmf(case["records"], fsm.MODE_SPADE)
    try:
        got = sref.split(*eng.pattern_sids(db, case["patterns"]))  # (split asserts strictly ascending)
        first = names(eng)
    finally:
        db.free()
    assert got == sref.by_definition(case["records"], case["patterns"])
    assert len(got[1]) == 4 * T + 1
    assert ORDER_ROW in first  # the ordering ran


# ------------------------------------------------------------------ E7. round trip
@pytest.mark.parametrize("seed", range(fref.N_RANDOM))
def test_round_trip_on_random_dbs(eng, seed):
    recs, sup, _complete = fref.mined_random_db(seed)
    db = eng.db_from_spmf(recs, fsm.MODE_SPADE)
    try:
        mined, _ = eng.spade(db, sup)
        off, sid = eng.pattern_sids(db, mined)
        counts = eng.pattern_supports(db, mined).tolist()
    finally:
        db.free()
    pats = [p for p, _s in mined]
    assert np.diff(off).tolist() == [s for _p, s in mined] == counts
    assert sref.split(off, sid) == sref.by_definition(recs, pats)


# ------------------------------------------------------------------ E8. slicing and hooks
@pytest.fixture(scope="module")
def default_lists(eng):
    return sref.list_cases(eng, sref.child_cases())


@pytest.mark.parametrize("hook", ["FSM_PS_PIVOT=first", "FSM_PS_PIVOT=last", "FSM_PS_SLICE_TILES=3",
                                  "FSM_PS_SLICE_SIDS=5", "FSM_PS_SLICE_SIDS=1"])
def test_hooks_change_no_list(default_lists, hook):
    """The pivot choice, the tiles per launch and the ids per write slice may change the speed,
    never a list."""
    key, val = hook.split("=")
    env = dict(os.environ)
    env[key] = val
    r = subprocess.run([sys.executable, os.path.join(HERE, "pattern_sids_ref.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    cases = sref.child_cases()
    assert sorted(got) == sorted(cases) and len(got) == fref.N_RANDOM + 6 * 4 * 2 + 1
    for name in cases:
        assert got[name] == default_lists[name], name
    for name, case in ref.tile_cases(T).items():
        assert np.diff(got[name][0]).tolist() == case["expected"], name


def test_default_lists_are_the_definition(default_lists):
    for name, (recs, pats) in sref.child_cases().items():
        off, sid = default_lists[name]
        assert sref.split(np.array(off, np.int64), np.array(sid, np.int32)) == sref.by_definition(recs, pats), name


# ------------------------------------------------------------------ E9 / E10. cap and errors
def _raw(eng, db, csr, out, max_sids=0, n=None, n_items=None):
    po, so, it = (np.ascontiguousarray(a, dt) for a, dt in zip(csr[1:], (np.int64, np.int64, np.int32)))
    P = ctypes.POINTER
    pats = _lib.Patterns(len(po) - 1 if n is None else n, None, po.ctypes.data_as(P(ctypes.c_int64)),
                         so.ctypes.data_as(P(ctypes.c_int64)), it.ctypes.data_as(P(ctypes.c_int32)), len(so) - 1,
                         len(it) if n_items is None else n_items, 0, 0)
    return eng._L.fsm_patterns_sids(eng._ctx, db.handle if db is not None else None, ctypes.byref(pats), max_sids,
                                    ctypes.byref(out) if out is not None else None)


def _marker():
    return ctypes.cast(0x1234, ctypes.POINTER(_lib.SidLists))


def _untouched(out):
    return ctypes.cast(out, ctypes.c_void_p).value == 0x1234


def test_cap(eng):
    case = sref.dead_tiles_case(T)
    total = sum(len(x) for x in case["expected"])
    assert total == T + 6 + 5
    csr = ref.to_csr(case["patterns"])
    db = eng.db_from_spmf(case["records"], fsm.MODE_SPADE)
    try:
        assert sref.split(*eng.pattern_sids(db, csr, max_sids=total)) == case["expected"]
        assert sref.split(*eng.pattern_sids(db, csr, max_sids=0)) == case["expected"]
        out = _marker()
        assert _raw(eng, db, csr, out, max_sids=total - 1) == _lib.FSM_ELIMIT
        assert _untouched(out)
        assert str(total) in eng._L.fsm_last_error(eng._ctx).decode()
        with pytest.raises(fsm.FsmError) as e:
            eng.pattern_sids(db, csr, max_sids=total - 1)
        assert e.value.code == _lib.FSM_ELIMIT and str(total) in e.value.msg
        assert sref.split(*eng.pattern_sids(db, csr, max_sids=-1)) == case["expected"]
    finally:
        db.free()


def test_errors_leave_the_output_and_the_statistics(eng):
    case = ref.hand_cases()["itemset_vs_sequence"]
    good = ref.to_csr(case["patterns"])
    exp = sref.by_definition(case["records"], case["patterns"])
    db = eng.db_from_spmf(case["records"], fsm.MODE_SPADE)
    tdb = eng.db_from_spmf(case["records"], fsm.MODE_TSR)
    try:
        eng.spade(db, 0.2)
        before, kbefore = eng.stats(), eng.kernel_stats()
        out = _marker()
        bad = {
            "descending_offset": (None, [0, 2, 1, 3], [0, 1, 2, 3], [1, 2, 1]),
            "set_off_not_monotone": (None, [0, 1, 2, 3], [0, 2, 1, 3], [1, 2, 1]),
            "empty_itemset": (None, [0, 1, 2], [0, 0, 2], [1, 2]),
            "unsorted_items": (None, [0, 1, 2], [0, 2, 3], [2, 1, 1]),
            "equal_items": (None, [0, 1, 2], [0, 2, 3], [1, 1, 1]),
            "pattern_without_itemsets": (None, [0, 1, 1, 2], [0, 1, 2], [1, 2]),
        }
        for name, csr in bad.items():
            assert _raw(eng, db, csr, out) == _lib.FSM_EINVAL, name
            assert eng._L.fsm_last_error(eng._ctx), name
            with pytest.raises(fsm.FsmError) as e:
                eng.pattern_sids(db, tuple(None if a is None else np.array(a) for a in csr))
            assert e.value.code == _lib.FSM_EINVAL, name
        assert _raw(eng, db, good, out, n=-1) == _lib.FSM_EINVAL
        assert _raw(eng, db, good, out, n=(1 << 32) - 2) == _lib.FSM_ELIMIT
        assert _raw(eng, db, good, out, n_items=(1 << 32) - 2) == _lib.FSM_ELIMIT
        assert _raw(eng, tdb, good, out) == _lib.FSM_EINVAL  # a TSR-mode DB
        with pytest.raises(fsm.FsmError) as e:
            eng.pattern_sids(tdb, case["patterns"])
        assert e.value.code == _lib.FSM_EINVAL
        # NULL db, in and out with a live context
        assert _raw(eng, None, good, out) == _lib.FSM_EINVAL
        assert eng._L.fsm_patterns_sids(eng._ctx, db.handle, None, 0, ctypes.byref(out)) == _lib.FSM_EINVAL
        assert _raw(eng, db, good, None) == _lib.FSM_EINVAL
        with fsm.Engine(0) as other:  # a DB of another context
            assert other._L.fsm_patterns_sids(other._ctx, db.handle, ctypes.byref(_lib.Patterns()), 0,
                                              ctypes.byref(out)) == _lib.FSM_EINVAL
        assert _untouched(out)
        assert eng.stats() == before and eng.kernel_stats() == kbefore
        # a following valid call still works, and fsm_stats is left as the mine set it
        res = ctypes.POINTER(_lib.SidLists)()
        assert _raw(eng, db, good, res) == _lib.FSM_OK
        try:
            r = res.contents
            assert r.n == len(exp) and r.n_sids == sum(len(x) for x in exp)
            assert [r.off[p] for p in range(r.n + 1)] == np.cumsum([0] + [len(x) for x in exp]).tolist()
            assert [r.sid[k] for k in range(r.n_sids)] == [s for x in exp for s in x]
        finally:
            eng._L.fsm_sidlists_free(res)
        assert eng.stats() == before
    finally:
        db.free()
        tdb.free()


# ------------------------------------------------------------------ E11. statistics
def test_kernel_statistics_and_counts_around_the_reordering(eng):
    case = ref.shared_launch_case(T)
    pats = case["patterns"]
    db = eng.db_from_spmf(case["records"], fsm.MODE_SPADE)
    try:
        eng.spade(db, 0.5)
        before = eng.stats()
        first = sref.split(*eng.pattern_sids(db, pats))
        rows1, ks1 = names(eng), eng.kernel_stats()
        again = sref.split(*eng.pattern_sids(db, pats))
        rows2 = names(eng)
        assert eng.stats() == before
    finally:
        db.free()
    assert first == again == sref.by_definition(case["records"], pats)
    # (k_scan: the index build's scan and the call's are one row)
    assert rows1 == INDEX_ROWS + [ORDER_ROW, "k_ps_match", "k_ps_sids_write"]
    assert set(rows1) == set(INDEX_ROWS) | {ORDER_ROW} | set(CALL_ROWS)
    assert {k["name"]: k["launches"] for k in ks1}["k_scan"] == 2
    assert rows2 == CALL_ROWS
    assert all(k["alg_bytes"] > 0 and k["launches"] >= 1 for k in ks1)
    # the counts before and after the lists were reordered
    db = eng.db_from_spmf(case["records"], fsm.MODE_SPADE)
    try:
        c1 = eng.pattern_supports(db, pats).tolist()
        assert names(eng) == INDEX_ROWS + ["k_ps_count"]
        lists = sref.split(*eng.pattern_sids(db, pats))
        assert names(eng) == [ORDER_ROW] + CALL_ROWS  # the index is there: only its order is made
        c2 = eng.pattern_supports(db, pats).tolist()
        assert names(eng) == ["k_ps_count"]
    finally:
        db.free()
    assert c1 == c2 == case["expected"] == [len(x) for x in lists]


# ------------------------------------------------------------------ E12. contexts
def test_group_context_and_two_dbs_on_one_context(eng):
    a, b = sref.lane_case("even", T), sref.sid_case()
    dba = eng.db_from_spmf(a["records"], fsm.MODE_SPADE)
    dbb = eng.db_from_spmf(b["text"], fsm.MODE_SPADE)
    try:
        la = sref.split(*eng.pattern_sids(dba, a["patterns"]))
        lb = sref.split(*eng.pattern_sids(dbb, b["patterns"]))
        la2 = sref.split(*eng.pattern_sids(dba, a["patterns"]))
    finally:
        dba.free()
        dbb.free()
    assert la == la2 == a["expected"] and lb == b["expected"]  # each DB keeps its own sid table
    with fsm.Engine(devices=[0, 0]) as grp:
        for recs, pats, exp in ((a["records"], a["patterns"], la), (b["text"], b["patterns"], lb)):
            gdb = grp.db_from_spmf(recs, fsm.MODE_SPADE)
            try:
                assert sref.split(*grp.pattern_sids(gdb, pats)) == exp
                assert [k["name"] for k in grp.kernel_stats()] == INDEX_ROWS + [ORDER_ROW, "k_ps_match", "k_ps_sids_write"]
            finally:
                gdb.free()
        sids, seq_off, tokens = b["tokens"]
        gdb = grp.db_from_tokens(sids, seq_off, tokens, fsm.MODE_SPADE)
        try:
            assert sref.split(*grp.pattern_sids(gdb, b["patterns"])) == lb
        finally:
            gdb.free()
