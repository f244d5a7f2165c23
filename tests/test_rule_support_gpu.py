"""GPU tests of fsm_rules_support (support, antecedent count and confidence of given rules in
a resident TSR DB): the results against the stated answers of tests/rule_support_ref.py's
generators, its two references, and the supports and confidences the miner itself reports."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_dbs
import pattern_filter_ref as fref
import rule_support_ref as ref
import spark_fsm_amd as fsm
from spark_fsm_amd import _lib
from tools import gen

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T = ref.constants()["kRsTile"]


@pytest.fixture(scope="module")
def eng():
    with fsm.Engine(0) as e:
        yield e


def score(eng, records, rules):
    db = eng.db_from_spmf(records, fsm.MODE_TSR)
    try:
        got = ref.triples_of(eng.rule_supports(db, rules))
        assert len(got) == len(rules)
        return got
    finally:
        db.free()


def check_case(eng, case, definition=True):
    got = score(eng, case["records"], case["rules"])
    assert got == case["expected"]
    if definition:
        assert got == ref.by_definition(case["records"], case["rules"])


# ------------------------------------------------------------------ 1. hand cases
@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_hand_cases(eng, name):
    case = ref.hand_cases()[name]
    check_case(eng, case)
    for sup, ante, conf in score(eng, case["records"], case["rules"]):
        assert conf == (sup / ante if ante else 0.0)


# ------------------------------------------------------------------ 2. input forms and empty sets
def _raw(eng, db, csr, out=None, ante=None, conf=None, n=None):
    xo, xs, yo, ys = (np.ascontiguousarray(a, dt) for a, dt in zip(csr, (np.int64, np.int32, np.int64, np.int32)))
    P = ctypes.POINTER
    rules = _lib.Rules(len(xo) - 1 if n is None else n, None, None, xo.ctypes.data_as(P(ctypes.c_int64)),
                       xs.ctypes.data_as(P(ctypes.c_int32)), yo.ctypes.data_as(P(ctypes.c_int64)),
                       ys.ctypes.data_as(P(ctypes.c_int32)), 0, 0)

    def ptr(a, ct):
        return None if a is None else a.ctypes.data_as(P(ct))

    return eng._L.fsm_rules_support(eng._ctx, db.handle, ctypes.byref(rules), ptr(out, ctypes.c_int32),
                                    ptr(ante, ctypes.c_int32), ptr(conf, ctypes.c_double))


def test_input_forms_null_outputs_and_the_empty_set(eng):
    case = ref.hand_cases()["later_first_of_x_decides"]
    rules, exp = case["rules"], case["expected"]
    db = eng.db_from_spmf(case["records"], fsm.MODE_TSR)
    try:
        mined = eng.tsr_mined(db, 10 ** 6, 0.0)
        mrules = mined.rules()
        assert len(mrules) > 2
        mexp = ref.by_definition(case["records"], mrules)
        assert ref.triples_of(eng.rule_supports(db, mined)) == mexp
        assert ref.triples_of(eng.rule_supports(db, mrules)) == mexp  # (X, Y, support, confidence)
        assert [(s, c) for s, _a, c in mexp] == [(m[2], m[3]) for m in mrules]
        assert ref.triples_of(eng.rule_supports(db, list(rules))) == exp
        assert ref.triples_of(eng.rule_supports(db, ref.to_csr(rules))) == exp
        assert ref.triples_of(eng.rule_supports(db, tuple(a.tolist() for a in ref.to_csr(rules)))) == exp
        assert ref.triples_of(fsm.rule_supports(db, rules)) == exp
        assert ref.triples_of(fsm.rule_supports(case["records"], rules, engine=eng)) == exp
        for empty in ([], ref.to_csr([])):
            got = eng.rule_supports(db, empty)
            assert [a.dtype for a in got] == [np.int32, np.int32, np.float64] and all(a.shape == (0,) for a in got)
        # NULL ante_out and NULL confidence_out are accepted, together and one at a time
        csr = ref.to_csr(rules)
        for want_ante in (False, True):
            for want_conf in (False, True):
                out = np.full(len(rules), -7, np.int32)
                ante = np.full(len(rules), -7, np.int32) if want_ante else None
                conf = np.full(len(rules), -7.0, np.float64) if want_conf else None
                assert _raw(eng, db, csr, out, ante, conf) == _lib.FSM_OK
                assert out.tolist() == [t[0] for t in exp]
                assert ante is None or ante.tolist() == [t[1] for t in exp]
                assert conf is None or conf.tolist() == [t[2] for t in exp]
    finally:
        db.free()


# ------------------------------------------------------------------ 3. errors
def test_errors_leave_the_outputs_and_the_statistics(eng):
    case = ref.hand_cases()["later_first_of_x_decides"]
    good = ref.to_csr(case["rules"])
    db = eng.db_from_spmf(case["records"], fsm.MODE_TSR)
    sdb = eng.db_from_spmf(case["records"], fsm.MODE_SPADE)
    try:
        eng.tsr(db, 5, 0.0)
        before = eng.stats()
        n = len(case["rules"])
        out, ante, conf = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, -7.0, np.float64)
        bad = {  # (ante_off, ante, cons_off, cons); the first rule is good
            "x_descending": ([0, 1, 3], [1, 3, 1], [0, 1, 2], [2, 2]),
            "y_descending": ([0, 1, 2], [1, 1], [0, 1, 3], [2, 3, 2]),
            "x_equal_items": ([0, 1, 3], [1, 3, 3], [0, 1, 2], [2, 2]),
            "y_equal_items": ([0, 1, 2], [1, 1], [0, 1, 3], [2, 3, 3]),
            "empty_x": ([0, 1, 1], [1], [0, 1, 2], [2, 2]),
            "empty_y": ([0, 1, 2], [1, 1], [0, 1, 1], [2]),
            "item_on_both_sides": ([0, 1, 3], [1, 1, 3], [0, 1, 3], [2, 2, 3]),
            "ante_off_not_monotone": ([0, 2, 1], [1, 3], [0, 1, 2], [2, 2]),
            "cons_off_not_monotone": ([0, 1, 2], [1, 1], [0, 2, 1], [2, 3]),
            "ante_off_not_from_0": ([1, 2, 3], [1, 1, 3], [0, 1, 2], [2, 2]),
        }
        for name, csr in bad.items():
            assert _raw(eng, db, csr, out, ante, conf) == _lib.FSM_EINVAL, name
            assert b"fsm_rules_support" in eng._L.fsm_last_error(eng._ctx), name
            with pytest.raises(fsm.FsmError) as e:
                eng.rule_supports(db, tuple(np.array(a) for a in csr))
            assert e.value.code == _lib.FSM_EINVAL, name
        assert _raw(eng, db, good, out, ante, conf, n=-1) == _lib.FSM_EINVAL
        assert eng._L.fsm_last_error(eng._ctx)
        # sizes over the u32 limits: refused before an item is read
        assert _raw(eng, db, good, out, ante, conf, n=(1 << 32) - 2) == _lib.FSM_ELIMIT
        assert _raw(eng, db, ([0, (1 << 32) - 2], [1], [0, 1], [2]), out, ante, conf) == _lib.FSM_ELIMIT
        assert _raw(eng, db, ([0, 1], [1], [0, (1 << 32) - 2], [2]), out, ante, conf) == _lib.FSM_ELIMIT
        assert _raw(eng, db, ([0, 1 << 31], [1], [0, (1 << 31) - 2], [2]), out, ante, conf) == _lib.FSM_ELIMIT
        assert _raw(eng, sdb, good, out, ante, conf) == _lib.FSM_EINVAL  # a SPADE-mode DB
        with pytest.raises(fsm.FsmError) as e:
            eng.rule_supports(sdb, case["rules"])
        assert e.value.code == _lib.FSM_EINVAL
        assert _raw(eng, db, good, None, ante, conf) == _lib.FSM_EINVAL  # NULL support_out
        assert eng._L.fsm_rules_support(eng._ctx, db.handle, None, None, None, None) == _lib.FSM_EINVAL
        with fsm.Engine(0) as other:  # a db of another context
            assert other._L.fsm_rules_support(other._ctx, db.handle, None, None, None, None) == _lib.FSM_EINVAL
            xo, xs, yo, ys = good
            P = ctypes.POINTER
            rules = _lib.Rules(n, None, None, xo.ctypes.data_as(P(ctypes.c_int64)), xs.ctypes.data_as(P(ctypes.c_int32)),
                               yo.ctypes.data_as(P(ctypes.c_int64)), ys.ctypes.data_as(P(ctypes.c_int32)), 0, 0)
            assert other._L.fsm_rules_support(other._ctx, db.handle, ctypes.byref(rules),
                                              out.ctypes.data_as(P(ctypes.c_int32)), None, None) == _lib.FSM_EINVAL
        assert out.tolist() == [-7] * n and ante.tolist() == [-7] * n and conf.tolist() == [-7.0] * n
        # a following valid call still works, and fsm_stats is left as the mine set it
        assert _raw(eng, db, good, out, ante, conf) == _lib.FSM_OK
        assert list(zip(out.tolist(), ante.tolist(), conf.tolist())) == case["expected"]
        assert eng.stats() == before
        ks = eng.kernel_stats()
        assert [k["name"] for k in ks] == ["k_rs_count"]
        assert ks[0]["launches"] == 1 and ks[0]["alg_bytes"] > 0
    finally:
        db.free()
        sdb.free()


# ------------------------------------------------------------------ 4. random DBs
def test_random_dbs_every_rule_and_the_mined_ones(eng):
    total = {k: 0 for k in ref.RANDOM_TOTALS}
    for seed in range(fref.N_RANDOM):
        case = ref.random_case(seed)
        db = eng.db_from_spmf(case["records"], fsm.MODE_TSR)
        try:
            got = ref.triples_of(eng.rule_supports(db, case["rules"]))
            assert got == case["expected"], seed
            cl = ref.classes(got)
            assert cl["partial"] >= ref.RANDOM_MIN_PARTIAL, seed
            for k in total:
                total[k] += cl[k]
            mined, _meta = eng.tsr(db, 10 ** 6, 0.0)
            assert len(mined) > 0
            again = ref.triples_of(eng.rule_supports(db, mined))
            assert [(s, c) for s, _a, c in again] == [(m[2], m[3]) for m in mined], seed
        finally:
            db.free()
    assert total == ref.RANDOM_TOTALS


# ------------------------------------------------------------------ 5. tile edges
@pytest.mark.parametrize("L", ref.tile_lengths(T))
def test_tile_edges(eng, L):
    n = 0
    for place in ref.PIVOT_PLACES:
        check_case(eng, ref.tile_edge_case(L, place, "full"), definition=False)
        n += 1
        for f in ref.failing_rows(L):
            lacks, order = ref.tile_edge_case(L, place, "lacks", f), ref.tile_edge_case(L, place, "order", f)
            assert lacks["expected"] == [ref.triple(L - 1, L - 1)] and order["expected"] == [ref.triple(L - 1, L)]
            check_case(eng, lacks, definition=False)  # (the CPU test holds the generator to the definition)
            check_case(eng, order, definition=False)
            n += 2
    assert n == 3 * (1 + 2 * len(ref.failing_rows(L)))


# ------------------------------------------------------------------ 6. short and long lists in one launch
def test_short_long_and_dead_rules_share_a_launch(eng):
    case = ref.mixed_launch_case(T)
    check_case(eng, case)
    assert eng.kernel_stats()[0]["launches"] == 1


# ------------------------------------------------------------------ 7. row lengths
@pytest.mark.parametrize("n", ref.ROW_LENGTHS)
def test_row_lengths_of_the_in_row_search(eng, n):
    case = ref.row_length_case(n)
    db = eng.db_from_spmf(case["records"], fsm.MODE_TSR)
    try:
        img = eng.db_export(db)
        assert np.diff(img["row_off"].astype(np.int64))[:2].tolist() == [n, n]
        assert ref.triples_of(eng.rule_supports(db, case["rules"])) == case["expected"]
    finally:
        db.free()


# ------------------------------------------------------------------ 8. itemset indexes beyond 16 bits
@pytest.mark.parametrize("last", (65535, 65536, 70000))
def test_itemset_indexes_beyond_16_bits(eng, last):
    edb = edge_dbs.tsr_deep_index(last)
    pairs = [((a,), (b,)) for a in (1, 2, 3) for b in (1, 2, 3) if a != b]
    rules = pairs + [((1, 3), (2,)), ((1,), (2, 3))]
    exp = ref.by_oracle(edb.seq_off, edb.tokens, rules)
    assert exp[rules.index(((1,), (2,)))] == ref.triple(3, 4) and exp[rules.index(((3,), (2,)))] == ref.triple(2, 2)
    db = eng.db_from_tokens(edb.sids, edb.seq_off, edb.tokens, fsm.MODE_TSR)
    try:
        assert int(eng.db_export(db)["last"].max()) == last
        assert ref.triples_of(eng.rule_supports(db, rules)) == exp
    finally:
        db.free()


# ------------------------------------------------------------------ 9. long sides
def test_sides_of_300_items(eng):
    case = ref.long_side_case(300)
    assert case["expected"] == [(1, 3, 1 / 3)]
    check_case(eng, case)


# ------------------------------------------------------------------ 10. sid edges
@pytest.mark.parametrize("N", ref.SID_EDGE_SIZES)
def test_sid_edges(eng, N):
    """1 -> 2 scores (m, m, 1.0), 3 -> 4 has support m - 1 and 2 -> 1 support 0.  The antes of
    the last two are those of the definition (ref.sid_edge_expected): the DB's one-item rows
    with 3 (with 2) hold the whole antecedent, so they are m - 1 + lone3 and m + lone2 (at
    N = 129: 36 and 33), not m - 1 and m."""
    edb = edge_dbs.tsr_sid_edges(N)
    m = len(edb.deciding)
    db = eng.db_from_tokens(edb.sids, edb.seq_off, edb.tokens, fsm.MODE_TSR)
    try:
        got = ref.triples_of(eng.rule_supports(db, ref.SID_EDGE_RULES))
    finally:
        db.free()
    assert got[0] == (m, m, 1.0) and got[1][0] == m - 1 and got[2][0] == 0
    assert got == ref.sid_edge_expected(edb) == ref.by_oracle(edb.seq_off, edb.tokens, ref.SID_EDGE_RULES)


# ------------------------------------------------------------------ 11. builds and contexts
def test_builds_and_contexts_agree(eng):
    ds = gen.kosarak(D=3000, seed=1)
    db = eng.db_from_spmf(ds.records(), fsm.MODE_TSR)
    try:
        mined, _meta = eng.tsr(db, 50, 0.5)
        assert len(mined) >= 50  # (k = 50 and the ties at the final minsup: 52 rules)
        want = [(m[2], m[3]) for m in mined]
        first = ref.triples_of(eng.rule_supports(db, mined))
        rows = [k["name"] for k in eng.kernel_stats()]
    finally:
        db.free()
    assert [(s, c) for s, _a, c in first] == want and rows == ["k_rs_count"]
    db = eng.db_from_tokens(ds.sids, ds.seq_off, ds.tokens, fsm.MODE_TSR)
    try:
        assert ref.triples_of(eng.rule_supports(db, mined)) == first
    finally:
        db.free()
    with fsm.Engine(devices=[0, 0]) as grp:
        gdb = grp.db_from_tokens(ds.sids, ds.seq_off, ds.tokens, fsm.MODE_TSR)
        try:
            assert ref.triples_of(grp.rule_supports(gdb, mined)) == first
            assert [k["name"] for k in grp.kernel_stats()] == ["k_rs_count"]
        finally:
            gdb.free()
    ds2 = gen.kosarak(D=3000, seed=2)
    db2 = eng.db_from_tokens(ds2.sids, ds2.seq_off, ds2.tokens, fsm.MODE_TSR)
    try:
        got2 = ref.triples_of(eng.rule_supports(db2, mined))
    finally:
        db2.free()
    assert got2 == ref.by_oracle(ds2.seq_off, ds2.tokens, mined)


# ------------------------------------------------------------------ 12. hooks
@pytest.fixture(scope="module")
def default_scores(eng):
    return ref.score_cases(eng, ref.child_cases())


@pytest.mark.parametrize("hook", ["FSM_RS_PIVOT=first", "FSM_RS_PIVOT=last", "FSM_RS_SLICE_TILES=3"])
def test_forced_pivot_and_launch_slices(default_scores, hook):
    """FSM_RS_PIVOT overrides the pivot choice, FSM_RS_SLICE_TILES the tiles per launch: either
    may change the speed, never a count."""
    key, val = hook.split("=")
    env = dict(os.environ)
    env[key] = val
    r = subprocess.run([sys.executable, os.path.join(HERE, "rule_support_ref.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    cases = ref.child_cases()
    assert sorted(got) == sorted(cases) and len(got) == fref.N_RANDOM + ref.n_tile_cases(T) + 1
    for name, case in cases.items():
        assert got[name] == default_scores[name], name
        assert [tuple(t) for t in got[name]] == case["expected"], name
