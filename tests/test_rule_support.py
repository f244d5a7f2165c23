"""CPU tests of fsm_rules_support: the entry point rejects bad arguments before any device
use, the Python wrapper's input forms reduce to the same arrays, and the references and case
generators of the GPU tests (tests/rule_support_ref.py) agree with each other and with their
stated answers."""
import ctypes

import numpy as np
import pytest

import edge_dbs
import pattern_filter_ref as fref
import rule_support_ref as ref
import spark_fsm_amd as fsm
from spark_fsm_amd import _lib

T = ref.constants()["kRsTile"]


@pytest.fixture(autouse=True, scope="module")
def entry_point():
    """The references and generators below are only worth holding to their answers while the
    library has the entry point they exist for."""
    assert hasattr(_lib.load(), "fsm_rules_support"), "libfsm.so has no fsm_rules_support"


def both_references(case):
    exp = ref.by_definition(case["records"], case["rules"])
    if ref.oracle_allows(case["rules"]):
        _sids, seq_off, tokens = ref.tokens_of(case["records"])
        assert ref.by_oracle(seq_off, tokens, case["rules"]) == exp
    return exp


def test_export_is_present():
    assert "fsm_rules_support" in _lib.EXPORTS
    assert hasattr(_lib.load(), "fsm_rules_support")
    assert callable(fsm.Engine.rule_supports) and callable(fsm.rule_supports)


def test_null_and_bad_arguments_are_einval():
    L = _lib.load()
    rules = _lib.Rules()
    out = np.full(4, -7, np.int32)
    ante = np.full(4, -7, np.int32)
    conf = np.full(4, -7.0, np.float64)
    outp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    antep = ante.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    confp = conf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    fake = ctypes.c_void_p(1)  # (never dereferenced: the null checks come first)
    assert L.fsm_rules_support(None, None, None, None, None, None) == _lib.FSM_EINVAL
    assert b"null" in L.fsm_last_error(None)
    assert L.fsm_rules_support(None, fake, ctypes.byref(rules), outp, antep, confp) == _lib.FSM_EINVAL
    assert L.fsm_rules_support(None, None, ctypes.byref(rules), outp, antep, confp) == _lib.FSM_EINVAL
    assert out.tolist() == [-7] * 4 and ante.tolist() == [-7] * 4 and conf.tolist() == [-7.0] * 4


def test_constants_are_read_from_the_source():
    c = ref.constants()
    assert c["kRsTile"] == 64 and c["kRsBlock"] % c["kRsTile"] == 0


def test_input_forms_reduce_to_the_same_arrays():
    rules = [((1, 3), (2,)), ((2,), (1, 3, 4)), ((7,), (8,))]
    want = ref.to_csr(rules)
    assert [a.tolist() for a in want] == [[0, 2, 3, 4], [1, 3, 2, 7], [0, 1, 4, 5], [2, 1, 3, 4, 8]]
    forms = [rules, [(x, y, 5, 0.5) for x, y in rules], [(list(x), list(y)) for x, y in rules], want,
             tuple(a.tolist() for a in want)]
    for form in forms:
        got = fsm.rules_csr(form)
        assert [a.dtype for a in got] == [np.int64, np.int32, np.int64, np.int32]
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert all(a.flags.c_contiguous for a in got)
    empty = fsm.rules_csr([])
    assert [a.tolist() for a in empty] == [[0], [], [0], []]
    assert [a.dtype for a in empty] == [np.int64, np.int32, np.int64, np.int32]
    # four rules in a tuple are rules, not the four arrays
    four = tuple(rules + [((5,), (6,))])
    assert [a.tolist() for a in fsm.rules_csr(four)] == [a.tolist() for a in ref.to_csr(list(four))]
    with pytest.raises(ValueError):
        fsm.rules_csr(([0, 1], [1], [0], []))


@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_hand_cases(name):
    case = ref.hand_cases()[name]
    assert both_references(case) == case["expected"]
    assert all(c == (s / a if a else 0.0) for s, a, c in case["expected"])


def test_hand_cases_cover_both_outcomes():
    exp = [t for case in ref.hand_cases().values() for t in case["expected"]]
    cl = ref.classes(exp)
    assert cl["ante0"] and cl["sup0"] and cl["partial"] and cl["full"]


def test_random_dbs_and_their_classes():
    total = {k: 0 for k in ref.RANDOM_TOTALS}
    for seed in range(fref.N_RANDOM):
        case = ref.random_case(seed)
        recs = case["records"]
        assert len(recs) <= 30 and [s for s, _ in recs] == list(range(len(recs)))
        items = ref.items_of(recs)
        assert len(items) <= 6 and ref.ABSENT not in items
        m = len(items) + 1
        assert len(case["rules"]) == 3 ** m - 2 ** (m + 1) + 1 == len(set(case["rules"]))
        assert both_references(case) == case["expected"]
        cl = ref.classes(case["expected"])
        assert cl["partial"] >= ref.RANDOM_MIN_PARTIAL, seed
        for (X, Y), (sup, ante, _c) in zip(case["rules"], case["expected"]):
            if ref.ABSENT in X:
                assert (sup, ante) == (0, 0)
            elif ref.ABSENT in Y:
                assert sup == 0
        for k in total:
            total[k] += cl[k]
    assert total == ref.RANDOM_TOTALS


def test_tile_cases_have_their_sizes_and_answers():
    cases = ref.tile_cases(T)
    assert len(cases) == ref.n_tile_cases(T) == 3 * (3 + 6 * 7)
    assert ref.tile_lengths(T) == (1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1)
    used = set()
    for name, case in cases.items():
        assert ref.by_definition(case["records"], case["rules"]) == case["expected"], name
        L = case["pivot_rows"]
        fl = ref.first_last(case["records"])
        lists = {}
        for sid, (f, _l) in enumerate(fl):
            for i in f:
                lists.setdefault(i, []).append(sid)
        assert lists[9] == list(range(L)), name  # the pivot's rows are sids 0 .. L - 1
        # the other items are common (about 4 L rows), so 9 is the rare one
        assert all(4 * L <= len(lists[i]) <= 4 * L + 1 for i in case["others"] + (ref.Y_ITEM,)), name
        (X, Y), (sup, ante, _c) = case["rules"][0], case["expected"][0]
        assert len(X) == 3 and (sup, ante) in ((L, L), (L - 1, L - 1), (L - 1, L))
        if sup < L:  # exactly one of the pivot's rows fails
            failing = [s for s in range(L) if ref.by_definition([(0, case["records"][s][1])], case["rules"])[0][0] == 0]
            assert len(failing) == 1
            used.add((L, failing[0]))
    for L in ref.tile_lengths(T):
        assert (L, 0) in used and (L, L - 1) in used


def test_mixed_launch_case():
    case = ref.mixed_launch_case(T)
    assert both_references(case) == case["expected"]
    fl = ref.first_last(case["records"])
    assert {i: sum(1 for f, _l in fl if i in f) for i in (10, 11, 12)} == case["lists"] == {10: 1, 11: T + 1, 12: 3 * T}
    exp = case["expected"]
    assert exp[0] == exp[-1] == ref.triple(0, 0)  # dead first and last
    assert exp[4][0] > 0 and exp[5] == ref.triple(0, T + 1) and exp[7][0] > 0  # unknown Y between two live rules


@pytest.mark.parametrize("n", ref.ROW_LENGTHS)
def test_row_length_cases(n):
    case = ref.row_length_case(n)
    fl = ref.first_last(case["records"])
    assert [len(f) for f, _l in fl[:2]] == [n, n]
    assert all(v % 2 == 0 for v in fl[0][0])
    assert both_references(case) == case["expected"]
    cl = ref.classes(case["expected"])
    assert cl["ante0"] == 3 and cl["sup0"] == (6 if n >= 2 else 3)
    assert cl["partial"] == (0 if n == 1 else 2 if n == 2 else 7)


def test_long_side_case():
    case = ref.long_side_case()
    (X, Y), = case["rules"]
    assert len(X) == len(Y) == 300 > ref.ORACLE_MAX_SIDE and not ref.oracle_allows(case["rules"])
    assert ref.by_definition(case["records"], case["rules"]) == case["expected"] == [(1, 3, 1 / 3)]


@pytest.mark.parametrize("last", (65535, 65536, 70000))
def test_deep_index_rules(last):
    db = edge_dbs.tsr_deep_index(last)
    rules = deep_rules()
    exp = ref.by_oracle(db.seq_off, db.tokens, rules)
    assert exp == ref.by_definition(db.records(), rules)
    assert exp[rules.index(((1,), (2,)))] == ref.triple(3, 4)
    assert exp[rules.index(((3,), (2,)))] == ref.triple(2, 2)


@pytest.mark.parametrize("N", ref.SID_EDGE_SIZES)
def test_sid_edge_answers(N):
    db = edge_dbs.tsr_sid_edges(N)
    m = len(db.deciding)
    exp = ref.sid_edge_expected(db)
    assert exp == ref.by_oracle(db.seq_off, db.tokens, ref.SID_EDGE_RULES)
    assert exp[0] == (m, m, 1.0) and exp[1][0] == m - 1 and exp[2][0] == 0
    assert exp[1][1] > m - 1 and exp[2][1] > m  # the one-item rows with 3 / with 2 hold the antecedent
    if N == 129:
        assert exp == ref.by_definition(db.records(), ref.SID_EDGE_RULES) and (exp[1][1], exp[2][1]) == (36, 33)


def deep_rules():
    pairs = [((a,), (b,)) for a in (1, 2, 3) for b in (1, 2, 3) if a != b]
    return pairs + [((1, 3), (2,)), ((1,), (2, 3))]
