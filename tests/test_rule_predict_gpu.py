"""GPU tests of fsm_rules_predict (per row of a resident TSR DB, the items given rules say
should come next): the results against the stated answers of tests/rule_predict_ref.py's
generators, its reference by definition, and the counts fsm_rules_support gives on the same DB."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_dbs
import pattern_filter_ref as fref
import rule_predict_ref as ref
import rule_support_ref as sref
import spark_fsm_amd as fsm
from spark_fsm_amd import _lib
from tools import gen

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T = ref.constants()["kRpTile"]


@pytest.fixture(scope="module")
def eng():
    with fsm.Engine(0) as e:
        yield e


def predict(eng, records, rules, topn):
    db = eng.db_from_spmf(records, fsm.MODE_TSR)
    try:
        got = ref.lists_of(eng.rule_predictions(db, rules, topn))
        assert len(got) == len(records)
        return got
    finally:
        db.free()


def check_case(eng, case, definition=True):
    got = predict(eng, case["records"], case["rules"], case["topn"])
    assert got == case["expected"]
    if definition:
        assert got == ref.by_definition(case["records"], case["rules"], case["topn"])


# ------------------------------------------------------------------ 1. hand cases
@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_hand_cases(eng, name):
    check_case(eng, ref.hand_cases()[name])


def test_input_forms_views_and_the_empty_rule_set(eng):
    case = ref.hand_cases()["rank_two_items_of_one_rule_by_value"]
    rules, exp = case["rules"], case["expected"]
    db = eng.db_from_spmf(case["records"], fsm.MODE_TSR)
    try:
        for form in (rules, fsm.scored_rules_csr(rules), tuple(a.tolist() for a in fsm.scored_rules_csr(rules))):
            assert ref.lists_of(eng.rule_predictions(db, form, 10)) == exp
        assert fsm.rule_predictions(db, rules, 10) == exp
        assert fsm.rule_predictions(case["records"], rules, 10, engine=eng) == exp
        view = eng.rule_predictions(db, rules, 10)
        assert not any(a.flags.writeable for a in view)
        copy = eng.rule_predictions(db, rules, 10, copy=True)
        assert all(a.flags.writeable for a in copy) and all(np.array_equal(a, b) for a, b in zip(view, copy))
        for empty in ([], fsm.scored_rules_csr([])):  # n == 0: every list is empty
            off, item, rule = eng.rule_predictions(db, empty, 5)
            assert off.tolist() == [0] * (len(case["records"]) + 1) and item.shape == rule.shape == (0,)
            assert eng.kernel_stats() == []
        for form in ([r[:2] for r in rules], sref.to_csr(rules)):
            with pytest.raises(ValueError):
                eng.rule_predictions(db, form, 10)
    finally:
        db.free()
    # a MinedRules is read as the library holds it, scores included
    recs = sref.hand_cases()["later_first_of_x_decides"]["records"]
    db = eng.db_from_spmf(recs, fsm.MODE_TSR)
    try:
        mined = eng.tsr_mined(db, 10 ** 6, 0.0)
        assert mined.n > 2
        want = ref.by_definition(recs, mined.rules(), 10)
        assert any(want) and ref.lists_of(eng.rule_predictions(db, mined, 10)) == want
    finally:
        db.free()


# ------------------------------------------------------------------ 2. agreement with fsm_rules_support
def test_one_rule_predicts_where_it_fires_without_holding(eng):
    n = 0
    for seed in range(fref.N_RANDOM):
        rc = ref.random_case(seed)
        db = eng.db_from_spmf(rc["records"], fsm.MODE_TSR)
        try:
            part = ref.partial_rules(seed)
            assert 0 < len(part) <= 25
            sup, ante, _conf = eng.rule_supports(db, [r for r, _t in part])
            for k, (rule, (esup, eante, _c)) in enumerate(part):
                assert (int(sup[k]), int(ante[k])) == (esup, eante) and 0 < esup < eante
                off, _item, _rule = eng.rule_predictions(db, [rule], ref.ALL)
                assert int(np.count_nonzero(np.diff(off))) == int(ante[k]) - int(sup[k]), (seed, rule)
                n += 1
        finally:
            db.free()
    assert n >= 20 * sref.RANDOM_MIN_PARTIAL


# ------------------------------------------------------------------ 3. random DBs
def test_random_dbs_every_rule(eng):
    total = {k: 0 for k in ref.RANDOM_TOTALS}
    for seed in range(fref.N_RANDOM):
        rc = ref.random_case(seed)
        db = eng.db_from_spmf(rc["records"], fsm.MODE_TSR)
        try:
            got = {t: ref.lists_of(eng.rule_predictions(db, rc["rules"], t)) for t in ref.RANDOM_TOPNS}
            conf = {t: ref.lists_of(eng.rule_predictions(db, rc["confident"], t)) for t in ref.RANDOM_TOPNS}
        finally:
            db.free()
        for t in ref.RANDOM_TOPNS:
            assert got[t] == rc["expected"][t], (seed, t)
            assert conf[t] == rc["confident_expected"][t], (seed, t)
        for k, v in ref.classes_of_lists(got[3], got[ref.ALL]).items():
            total[k] += v
        cl = ref.random_classes(rc["records"], rc["rules"])  # (on the CPU: which tie-break decided an entry)
        total["by_support"] += cl["by_support"]
        total["by_index"] += cl["by_index"]
        total["confident_rules"] += len(rc["confident"])
        total["confident_empty"] += sum(1 for l in conf[ref.ALL] if not l)
    assert total == ref.RANDOM_TOTALS
    assert all(total[k] > 0 for k in ref.RANDOM_POSITIVE)


# ------------------------------------------------------------------ 4. tile edges
@pytest.mark.parametrize("L", sref.tile_lengths(T))
def test_tile_edges(eng, L):
    n = 0
    for place in sref.PIVOT_PLACES:
        full = ref.tile_case(L, place, "full")
        assert not any(full["expected"])
        check_case(eng, full, definition=False)  # (the CPU test holds the generators to the definition)
        inv = ref.tile_inverse_case(L, place)
        assert inv["expected"] == [[(sref.Y_ITEM, 0)]] * L + [[]] * (3 * L)
        check_case(eng, inv, definition=False)
        n += 2
        for f in sref.failing_rows(L):
            lacks, order = ref.tile_case(L, place, "lacks", f), ref.tile_case(L, place, "order", f)
            assert not any(lacks["expected"])
            assert [s for s, l in enumerate(order["expected"]) if l] == [f] and order["expected"][f] == [(sref.Y_ITEM, 0)]
            check_case(eng, lacks, definition=False)
            check_case(eng, order, definition=False)
            n += 2
    assert n == 3 * (2 + 2 * len(sref.failing_rows(L)))


# ------------------------------------------------------------------ 5. segment lengths of one row
@pytest.mark.parametrize("m", ref.SEGMENT_SIZES)
def test_segment_lengths(eng, m):
    cases = {n: c for n, c in ref.segment_cases().items() if n.startswith("m%d-" % m)}
    assert len(cases) == len({1, m - 1, m, ref.ALL} - {0}) + 1
    got, _launches = ref.predict_cases(eng, cases)
    for name, case in cases.items():
        assert [[tuple(p) for p in row] for row in got[name]] == case["expected"], name
    uncut = cases["m%d-top%d" % (m, ref.ALL)]["expected"]
    assert [len(l) for l in uncut] == [m, 1, m, 1, 0]
    assert [len(l) for l in cases["m%d-shared" % m]["expected"]] == [1, 1, 1, 1, 0]


# ------------------------------------------------------------------ 6. row counts
@pytest.mark.parametrize("N", sref.SID_EDGE_SIZES)
def test_sid_edges(eng, N):
    edb = edge_dbs.tsr_sid_edges(N)
    case = ref.sid_edge_case(edb)
    db = eng.db_from_tokens(edb.sids, edb.seq_off, edb.tokens, fsm.MODE_TSR)
    try:
        off, item, rule = eng.rule_predictions(db, case["rules"], case["topn"])
        got = ref.lists_of((off, item, rule))
    finally:
        db.free()
    assert len(off) == N + 1
    taken = set(edb.deciding) | set(edb.second)
    for s in edb.deciding:  # nothing from 1 => 2, which holds there
        assert all(r != 0 for _i, r in got[s]), s
    for s in range(N):
        if s not in taken and s % 4 == 0:
            assert got[s] == [(1, 2)], s  # a row with 2 alone
        if s not in taken and s % 4 == 1:
            assert got[s] == [(4, 1)], s  # a row with 3 alone
    assert got == case["expected"]
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(l) for l in case["expected"]])]).tolist()
    if N == sref.SID_EDGE_SIZES[0]:
        assert got == ref.by_definition(edb.records(), case["rules"], case["topn"])


# ------------------------------------------------------------------ 7. itemset indexes beyond 16 bits
@pytest.mark.parametrize("last", (65535, 65536, 70000))
def test_itemset_indexes_beyond_16_bits(eng, last):
    edb = edge_dbs.tsr_deep_index(last)
    pairs = [((a,), (b,)) for a in (1, 2, 3) for b in (1, 2, 3) if a != b]
    records = edb.records()
    rules = ref.scored(records, pairs + [((1, 3), (2,)), ((1,), (2, 3))])
    exp = ref.by_definition(records, rules, ref.ALL)
    # the deep rows hold 1 at 0, 3 at last - 1 and 2 at last: 2 => 3 fires with 3 one itemset before
    assert (3, pairs.index(((2,), (3,)))) in exp[0] and not any(i == 2 for i, _r in exp[0])
    db = eng.db_from_tokens(edb.sids, edb.seq_off, edb.tokens, fsm.MODE_TSR)
    try:
        assert int(eng.db_export(db)["last"].max()) == last
        assert ref.lists_of(eng.rule_predictions(db, rules, ref.ALL)) == exp
    finally:
        db.free()


# ------------------------------------------------------------------ 8. long sides
def test_sides_of_300_items(eng):
    """Rows 0 and 1 predict nothing (the rule holds; the rule does not fire) and row 2 exactly
    Y[0].  Row 3 holds X alone: the rule fires and no item of Y has occurred after X, so by the
    definition all 300 items of Y are open there, in value order."""
    case = ref.long_side_case(300)
    Y = case["rules"][0][1]
    assert case["expected"][:3] == [[], [], [(Y[0], 0)]] and case["expected"][3] == [(y, 0) for y in Y]
    check_case(eng, case)
    cut = dict(case, topn=7, expected=[l[:7] for l in case["expected"]])
    check_case(eng, cut)


# ------------------------------------------------------------------ 9. hooks
@pytest.fixture(scope="module")
def default_run(eng):
    return ref.predict_cases(eng, ref.child_cases())


HOOKS = ["FSM_RP_SLICE_ROWS=1", "FSM_RP_SLICE_ROWS=3", "FSM_RP_SLICE_ROWS=64", "FSM_RP_PIVOT=first", "FSM_RP_PIVOT=last"]


@pytest.mark.parametrize("hook", HOOKS)
def test_forced_row_slices_and_pivots(default_run, hook):
    """FSM_RP_SLICE_ROWS sets the rows per pass, FSM_RP_PIVOT overrides the pivot choice: either
    may change the speed, never a result.  The count launch is shared by the passes, so a call
    has one k_rp_match launch for the count and one per pass with records."""
    key, val = hook.split("=")
    env = dict(os.environ)
    env[key] = val
    r = subprocess.run([sys.executable, os.path.join(HERE, "rule_predict_ref.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    got, launches = out["results"], out["launches"]
    cases = ref.child_cases()
    dres, dlaunch = default_run
    assert sorted(got) == sorted(cases) and len(got) == 3 * fref.N_RANDOM + ref.n_tile_cases(T) + len(ref.segment_cases())
    for name, case in cases.items():
        assert got[name] == dres[name], name
        assert [[tuple(p) for p in row] for row in got[name]] == case["expected"], name
        # unforced: the count launch and one write pass; no record, no write pass
        assert dlaunch[name] == 2 if any(case["expected"]) else dlaunch[name] <= 1, name
    if key == "FSM_RP_SLICE_ROWS":
        n = int(val)
        for name, case in cases.items():
            # a write pass per range of n rows that holds a record, that is, a prediction
            ranges = len({s // n for s, l in enumerate(case["expected"]) if l})
            assert launches[name] == (1 + ranges if ranges else dlaunch[name]), name
        assert max(launches.values()) > 2  # more than one launch pair
        assert launches["L%d-first-inverse" % (2 * T + 1)] == 1 + (2 * T + 1 + n - 1) // n
    else:
        assert launches == dlaunch


# ------------------------------------------------------------------ 10. errors
def _raw(eng, db, csr, topn=3, n=None, out=None, ctx=None):
    P = ctypes.POINTER
    keep = [None if a is None else np.ascontiguousarray(a, dt) for a, dt in
            zip(csr, (np.int64, np.int32, np.int64, np.int32, np.int32, np.float64))]
    cts = (ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_double)
    p = [None if a is None else a.ctypes.data_as(P(ct)) for a, ct in zip(keep, cts)]
    rules = _lib.Rules(len(keep[0]) - 1 if n is None else n, p[4], p[5], p[0], p[1], p[2], p[3], 0, 0)
    rc = eng._L.fsm_rules_predict(eng._ctx if ctx is None else ctx, db.handle, ctypes.byref(rules), topn,
                                  None if out is None else ctypes.byref(out))
    del keep
    return rc


def test_errors_leave_the_output_and_the_statistics(eng):
    case = ref.hand_cases()["rank_two_items_of_one_rule_by_value"]
    good = fsm.scored_rules_csr(case["rules"])
    db = eng.db_from_spmf(case["records"], fsm.MODE_TSR)
    sdb = eng.db_from_spmf(case["records"], fsm.MODE_SPADE)
    L = eng._L
    addr = 0xDEAD0  # (never dereferenced: a failed call leaves *out as it was)

    def untouched(out):
        return ctypes.cast(out, ctypes.c_void_p).value == addr

    try:
        eng.tsr(db, 5, 0.0)
        before = eng.stats()
        out = ctypes.cast(ctypes.c_void_p(addr), ctypes.POINTER(_lib.Predictions))
        s2, c2 = [1, 1], [0.5, 0.5]
        bad = {  # (ante_off, ante, cons_off, cons, support, confidence); the first rule is good
            "x_descending": ([0, 1, 3], [1, 3, 1], [0, 1, 2], [2, 2], s2, c2),
            "y_descending": ([0, 1, 2], [1, 1], [0, 1, 3], [2, 3, 2], s2, c2),
            "x_equal_items": ([0, 1, 3], [1, 3, 3], [0, 1, 2], [2, 2], s2, c2),
            "y_equal_items": ([0, 1, 2], [1, 1], [0, 1, 3], [2, 3, 3], s2, c2),
            "empty_x": ([0, 1, 1], [1], [0, 1, 2], [2, 2], s2, c2),
            "empty_y": ([0, 1, 2], [1, 1], [0, 1, 1], [2], s2, c2),
            "item_on_both_sides": ([0, 1, 3], [1, 1, 3], [0, 1, 3], [2, 2, 3], s2, c2),
            "ante_off_not_monotone": ([0, 2, 1], [1, 3], [0, 1, 2], [2, 2], s2, c2),
            "cons_off_not_monotone": ([0, 1, 2], [1, 1], [0, 2, 1], [2, 3], s2, c2),
            "ante_off_not_from_0": ([1, 2, 3], [1, 1, 3], [0, 1, 2], [2, 2], s2, c2),
            "nan_confidence": ([0, 1, 2], [1, 1], [0, 1, 2], [2, 2], s2, [0.5, float("nan")]),
            "null_support": ([0, 1, 2], [1, 1], [0, 1, 2], [2, 2], None, c2),
            "null_confidence": ([0, 1, 2], [1, 1], [0, 1, 2], [2, 2], s2, None),
        }
        for name, csr in bad.items():
            assert _raw(eng, db, csr, out=out) == _lib.FSM_EINVAL, name
            assert b"fsm_rules_predict" in L.fsm_last_error(eng._ctx), name
            assert untouched(out), name
            if None not in csr:
                with pytest.raises(fsm.FsmError) as e:
                    eng.rule_predictions(db, tuple(np.array(a) for a in csr), 3)
                assert e.value.code == _lib.FSM_EINVAL, name

        def einval(rc):
            assert rc == _lib.FSM_EINVAL and b"fsm_rules_predict" in L.fsm_last_error(eng._ctx) and untouched(out)

        einval(_raw(eng, db, good, n=-1, out=out))
        einval(_raw(eng, db, good, topn=0, out=out))
        einval(_raw(eng, db, good, topn=-5, out=out))
        einval(_raw(eng, sdb, good, out=out))  # a SPADE-mode DB
        einval(_raw(eng, db, good, out=None))  # NULL out
        einval(L.fsm_rules_predict(eng._ctx, db.handle, None, 3, ctypes.byref(out)))  # NULL in
        einval(L.fsm_rules_predict(eng._ctx, None, None, 3, ctypes.byref(out)))  # NULL db
        with pytest.raises(fsm.FsmError) as e:
            eng.rule_predictions(sdb, case["rules"], 3)
        assert e.value.code == _lib.FSM_EINVAL
        with pytest.raises(fsm.FsmError) as e:
            eng.rule_predictions(db, case["rules"], 0)
        assert e.value.code == _lib.FSM_EINVAL
        with fsm.Engine(0) as other:  # a db of another context
            assert _raw(eng, db, good, out=out, ctx=other._ctx) == _lib.FSM_EINVAL
            assert b"fsm_rules_predict" in L.fsm_last_error(other._ctx) and untouched(out)
        # sizes over the limits: refused before an item is read
        for n_over, csr in ((1 << 31, good), ((1 << 32) - 2, good), (None, ([0, (1 << 32) - 2], [1], [0, 1], [2], [1], [0.5])),
                            (None, ([0, 1], [1], [0, (1 << 32) - 2], [2], [1], [0.5])),
                            (None, ([0, 1 << 31], [1], [0, (1 << 31) - 2], [2], [1], [0.5]))):
            assert _raw(eng, db, csr, n=n_over, out=out) == _lib.FSM_ELIMIT
            assert b"fsm_rules_predict" in L.fsm_last_error(eng._ctx) and untouched(out)
        # a following valid call still works, and fsm_stats is left as the mine set it
        res = ctypes.POINTER(_lib.Predictions)()
        assert _raw(eng, db, good, topn=10, out=res) == _lib.FSM_OK and res
        r = res.contents
        assert (r.n, r.n_preds) == (1, 4) and [r.off[k] for k in range(2)] == [0, 4]
        assert [(r.item[k], r.rule[k]) for k in range(4)] == case["expected"][0]
        L.fsm_predictions_free(res)
        assert eng.stats() == before
        ks = {k["name"]: k for k in eng.kernel_stats()}
        assert set(ks) == {"k_rp_match", "k_rp_sort", "k_rp_first", "k_rp_select", "k_scan"}
        assert all(k.startswith("k_rp_") or k == "k_scan" for k in ks)
        assert ks["k_rp_match"]["launches"] == 2 and ks["k_rp_sort"]["launches"] == 2 and ks["k_scan"]["launches"] == 2
        assert all(k["alg_bytes"] > 0 for k in ks.values())
    finally:
        db.free()
        sdb.free()


# ------------------------------------------------------------------ 11. builds and contexts
def test_builds_and_contexts_agree(eng):
    ds = gen.kosarak(D=3000, seed=1)
    db = eng.db_from_spmf(ds.records(), fsm.MODE_TSR)
    try:
        mined, _meta = eng.tsr(db, 50, 0.5)
    finally:
        db.free()
    assert len(mined) >= 50
    ds2 = gen.kosarak(D=3000, seed=2)
    recs2 = ds2.records()
    assert [s for s, _l in recs2] == list(range(len(recs2)))
    want = ref.by_definition(recs2, mined, 5)
    assert any(want)
    db = eng.db_from_spmf(recs2, fsm.MODE_TSR)
    try:
        assert ref.lists_of(eng.rule_predictions(db, mined, 5)) == want
        rows = {k["name"] for k in eng.kernel_stats()}
    finally:
        db.free()
    assert rows == {"k_rp_match", "k_rp_sort", "k_rp_first", "k_rp_select", "k_scan"}
    db = eng.db_from_tokens(ds2.sids, ds2.seq_off, ds2.tokens, fsm.MODE_TSR)
    try:
        assert ref.lists_of(eng.rule_predictions(db, mined, 5)) == want
    finally:
        db.free()
    with fsm.Engine(devices=[0, 0]) as grp:
        gdb = grp.db_from_tokens(ds2.sids, ds2.seq_off, ds2.tokens, fsm.MODE_TSR)
        try:
            assert ref.lists_of(grp.rule_predictions(gdb, mined, 5)) == want
            assert {k["name"] for k in grp.kernel_stats()} == rows
        finally:
            gdb.free()
