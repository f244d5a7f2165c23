"""CPU tests of fsm_rules_predict: the library exports the entry point and rejects bad
arguments before any device use, the Python wrapper's input forms reduce to the same arrays
(a form without scores is refused), and the reference and the case generators of the GPU tests
(tests/rule_predict_ref.py) agree with each other and with their stated answers."""
import ctypes
import subprocess

import numpy as np
import pytest

import edge_dbs
import pattern_filter_ref as fref
import rule_predict_ref as ref
import rule_support_ref as sref
import spark_fsm_amd as fsm
from spark_fsm_amd import _lib

T = ref.constants()["kRpTile"]


def test_exports_are_present():
    for sym in ("fsm_rules_predict", "fsm_predictions_free"):
        assert sym in _lib.EXPORTS
        assert hasattr(_lib.load(), sym), "libfsm.so has no %s" % sym
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert {"fsm_rules_predict", "fsm_predictions_free"} <= defined
    assert callable(fsm.Engine.rule_predictions) and callable(fsm.rule_predictions) and callable(fsm.scored_rules_csr)


def test_abi_version_stays_7():
    assert _lib.load().fsm_abi_version() == 7


def test_null_arguments_are_einval_and_free_takes_null():
    L = _lib.load()
    rules = _lib.Rules()
    out = ctypes.POINTER(_lib.Predictions)()
    fake = ctypes.c_void_p(1)  # (never dereferenced: the null checks come first)
    assert L.fsm_rules_predict(None, None, None, 1, None) == _lib.FSM_EINVAL
    assert b"fsm_rules_predict" in L.fsm_last_error(None)
    assert L.fsm_rules_predict(None, fake, ctypes.byref(rules), 1, ctypes.byref(out)) == _lib.FSM_EINVAL
    assert L.fsm_rules_predict(None, None, ctypes.byref(rules), 1, ctypes.byref(out)) == _lib.FSM_EINVAL
    assert not out
    L.fsm_predictions_free(None)


def test_constants_are_read_from_the_source():
    c = ref.constants()
    assert c["kRpTile"] == 64 and c["kRpBlock"] % c["kRpTile"] == 0
    assert c["kRpRecordBytes"] >= 24  # two u64 key buffers and the sort's own buffer per record


def test_input_forms_reduce_to_the_same_arrays():
    rules = [((1, 3), (2,), 5, 0.5), ((2,), (1, 3, 4), 2, 0.25), ((7,), (8,), 9, 1.0)]
    xo, xs, yo, ys = sref.to_csr(rules)
    want = (xo, xs, yo, ys, np.array([5, 2, 9], np.int32), np.array([0.5, 0.25, 1.0], np.float64))
    forms = [rules, [list(r) for r in rules], want, tuple(a.tolist() for a in want)]
    for form in forms:
        got = fsm.scored_rules_csr(form)
        assert [a.dtype for a in got] == [np.int64, np.int32, np.int64, np.int32, np.int32, np.float64]
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert all(a.flags.c_contiguous for a in got)
    empty = fsm.scored_rules_csr([])
    assert [a.tolist() for a in empty] == [[0], [], [0], [], [], []]
    # six scored rules in a tuple are rules, not the six arrays
    six = tuple(rules * 2)
    assert [a.tolist() for a in fsm.scored_rules_csr(six)][:4] == [a.tolist() for a in sref.to_csr(list(six))]


def test_forms_without_scores_are_a_value_error():
    pairs = [((1,), (2,)), ((2,), (3,))]
    for form in (pairs, sref.to_csr(pairs), tuple(a.tolist() for a in sref.to_csr(pairs)), [((1,), (2,), 3)]):
        with pytest.raises(ValueError):
            fsm.scored_rules_csr(form)
    # one score per rule
    with pytest.raises(ValueError):
        fsm.scored_rules_csr(([0, 1], [1], [0, 1], [2], [1, 1], [0.5]))
    with pytest.raises(ValueError):
        fsm.scored_rules_csr(([0, 1], [1], [0, 1], [2], [1], [0.5, 0.5]))
    # the engine method refuses them before it touches its context or the DB
    for form in (pairs, sref.to_csr(pairs)):
        with pytest.raises(ValueError):
            fsm.Engine.rule_predictions(None, None, form, 3)


def test_rank_order():
    rules = [((1,), (2,), 3, 0.5), ((1,), (2,), 7, 0.5), ((1,), (2,), 1, 0.9), ((1,), (2,), 7, 0.5), ((1,), (2,), 0, 0.0)]
    assert ref.rank_order(rules) == [2, 1, 3, 0, 4]


@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_hand_cases(name):
    case = ref.hand_cases()[name]
    assert ref.by_definition(case["records"], case["rules"], case["topn"]) == case["expected"]


def test_hand_cases_cover_the_listed_situations():
    names = set(ref.hand_cases())
    assert len([n for n in names if n.startswith("open_")]) >= 10
    assert len([n for n in names if n.startswith("rank_")]) >= 5
    assert {"topn_1", "topn_equal_to_the_length", "topn_one_above_the_length", "topn_max"} <= names
    assert ref.hand_cases()["topn_max"]["topn"] == 2 ** 31 - 1


def test_a_rule_holds_where_it_fires_with_nothing_open():
    """The consequence the GPU test holds against fsm_rules_support: one rule alone predicts in
    exactly the ante - support rows in which it fires without holding."""
    n = 0
    for seed in range(fref.N_RANDOM):
        rc = ref.random_case(seed)
        part = ref.partial_rules(seed)
        assert 0 < len(part) <= 25
        for rule, (sup, ante, _c) in part:
            lists = ref.by_definition(rc["records"], [rule], ref.ALL)
            assert sum(1 for l in lists if l) == ante - sup > 0
            n += 1
    assert n >= 20 * sref.RANDOM_MIN_PARTIAL


def test_random_dbs_and_their_classes():
    total = {k: 0 for k in ref.RANDOM_TOTALS}
    for seed in range(fref.N_RANDOM):
        rc = ref.random_case(seed)
        assert len(rc["rules"]) == len(sref.random_case(seed)["rules"])
        cl = ref.random_classes(rc["records"], rc["rules"])
        shown = ref.classes_of_lists(rc["expected"][3], rc["expected"][ref.ALL])
        assert all(shown[k] == cl[k] for k in shown), seed
        assert all(len(l) <= 1 for l in rc["expected"][1]) and all(len(l) <= 3 for l in rc["expected"][3])
        for k in cl:
            total[k] += cl[k]
        total["confident_rules"] += len(rc["confident"])
        total["confident_empty"] += sum(1 for l in rc["confident_expected"][ref.ALL] if not l)
        # cutting a list changes nothing ahead of the cut
        for t in (1, 3):
            assert rc["confident_expected"][t] == [l[:t] for l in rc["confident_expected"][ref.ALL]]
            assert rc["expected"][t] == [l[:t] for l in rc["expected"][ref.ALL]]
    assert total == ref.RANDOM_TOTALS
    assert all(total[k] > 0 for k in ref.RANDOM_POSITIVE)


def test_tile_cases_have_their_sizes_and_answers():
    cases = ref.tile_cases(T)
    # per place: full and inverse at 7 lengths, lacks and order at 1 failing row (L = 1) or 3 (6 lengths)
    assert len(cases) == ref.n_tile_cases(T) == 3 * (2 * 7 + 2 * (1 + 3 * 6))
    for name, case in cases.items():
        assert ref.by_definition(case["records"], case["rules"], case["topn"]) == case["expected"], name
        nonempty = [s for s, l in enumerate(case["expected"]) if l]
        if name.endswith("inverse"):
            L = int(name[1:name.index("-")])
            assert nonempty == list(range(L)) and len(case["records"]) == 4 * L
        elif "-order-" in name:
            assert nonempty == [int(name.rsplit("-", 1)[1])]
        else:
            assert nonempty == []


@pytest.mark.parametrize("m", ref.SEGMENT_SIZES)
def test_segment_cases(m):
    for shared in (False, True):
        case = ref.segment_case(m, shared)
        assert ref.by_definition(case["records"], case["rules"], case["topn"]) == case["expected"]
        confs = [r[3] for r in case["rules"]]
        assert len(set(confs)) == m == len(case["rules"])
        long0, short1, long2, short3, last = case["expected"]
        assert long0 == long2 and short1 == short3 and last == []
        assert len(long0) == (1 if shared else m) and len(short1) == 1 and short1[0][1] == 0
        assert [confs[r] for _i, r in long0] == sorted((confs[r] for _i, r in long0), reverse=True)
        if shared:
            assert confs[long0[0][1]] == max(confs)
    names = [n for n in ref.segment_cases() if n.startswith("m%d-" % m)]
    assert len(names) == len({1, m - 1, m, ref.ALL} - {0}) + 1
    for n in names:
        case = ref.segment_cases()[n]
        assert ref.by_definition(case["records"], case["rules"], case["topn"]) == case["expected"], n


def test_sid_edge_case():
    edb = edge_dbs.tsr_sid_edges(129)
    case = ref.sid_edge_case(edb)
    assert ref.by_definition(edb.records(), case["rules"], case["topn"]) == case["expected"]
    assert [(r[2], r[3]) for r in case["rules"]] == [(t[0], t[2]) for t in sref.by_definition(edb.records(), sref.SID_EDGE_RULES)]
    assert all(case["expected"][s] == [(1, 2)] for s in edb.deciding) and all(case["expected"][s] == [] for s in edb.second)
    assert [(4, 1)] in case["expected"] and sum(1 for l in case["expected"] if not l) > len(edb.second)


def test_long_side_case():
    case = ref.long_side_case(300)
    (X, Y, sup, conf), = case["rules"]
    assert len(X) == len(Y) == 300 and (sup, conf) == (1, 1 / 3)
    assert ref.by_definition(case["records"], case["rules"], case["topn"]) == case["expected"]
    assert case["expected"][:3] == [[], [], [(Y[0], 0)]] and [i for i, _r in case["expected"][3]] == list(Y)
