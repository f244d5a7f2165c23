"""CPU tests of fsm_patterns_support: the entry point rejects bad arguments before any
device use, and the references and case generators of the GPU tests
(tests/pattern_support_ref.py) agree with each other and with their stated answers."""
import ctypes

import numpy as np
import pytest

import pattern_filter_ref as fref
import pattern_support_ref as ref
import spark_fsm_amd as fsm
from spark_fsm_amd import _lib


@pytest.fixture(autouse=True, scope="module")
def entry_point():
    """The references and generators below are only worth holding to their answers while the
    library has the entry point they exist for."""
    assert hasattr(_lib.load(), "fsm_patterns_support"), "libfsm.so has no fsm_patterns_support"


def test_export_is_present():
    assert "fsm_patterns_support" in _lib.EXPORTS
    assert hasattr(_lib.load(), "fsm_patterns_support")
    assert callable(fsm.Engine.pattern_supports) and callable(fsm.pattern_supports)


def test_null_and_bad_arguments_are_einval():
    L = _lib.load()
    pats = _lib.Patterns()
    out = np.full(4, -7, np.int32)
    outp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    fake = ctypes.c_void_p(1)  # (never dereferenced: the null checks come first)
    assert L.fsm_patterns_support(None, None, None, None) == _lib.FSM_EINVAL
    assert b"null" in L.fsm_last_error(None)
    assert L.fsm_patterns_support(None, fake, ctypes.byref(pats), outp) == _lib.FSM_EINVAL
    assert L.fsm_patterns_support(None, None, ctypes.byref(pats), outp) == _lib.FSM_EINVAL
    assert out.tolist() == [-7] * 4


def test_constants_are_read_from_the_source():
    c = ref.constants()
    assert c["kPsTile"] == 64 and c["kPsBlock"] % c["kPsTile"] == 0 and c["kPsSetRegs"] >= 1


@pytest.mark.parametrize("seed", range(fref.N_RANDOM))
def test_references_agree_on_random_dbs(seed):
    recs, _sup = fref.random_db(seed)
    items = ref.items_of(recs)
    beyond = [items[-1] + 1, items[0] - 1]  # two values the DB does not hold
    pats = ref.small_patterns(sorted(items + beyond))
    assert len(pats) > len(ref.small_patterns(items)) > 0
    _sids, seq_off, tokens = ref.tokens_of(recs)
    exp = ref.by_definition(recs, pats)
    assert exp == ref.by_oracle(seq_off, tokens, pats)
    assert all(0 <= c <= len(recs) for c in exp) and max(exp) > 0
    assert all(c == 0 for p, c in zip(pats, exp) if any(i in beyond for X in p for i in X))


@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_hand_cases(name):
    case = ref.hand_cases()[name]
    assert ref.by_definition(case["records"], case["patterns"]) == case["expected"]


def test_tile_cases_have_their_sizes_and_counts():
    T = ref.constants()["kPsTile"]
    cases = ref.tile_cases(T)
    assert len(cases) == 6 * 4 * 2 + 1
    for name, case in cases.items():
        assert ref.by_definition(case["records"], case["patterns"]) == case["expected"], name
        if name == "shared-launch":
            continue
        view = ref.brute.spade_eid_view(case["records"])
        lists = {}
        for sid, seq in view.items():
            for i in {i for X in seq for i in X}:
                lists.setdefault(i, []).append(sid)
        L = case["pivot_rows"]
        assert L in ref.tile_lengths(T) and len(lists[9]) == L and case["expected"][0] in (L, L - 1)
        assert all(len(v) >= L + 8 for i, v in lists.items() if i != 9), name  # 9 is the shortest list
        if case["expected"][0] == L - 1:  # the deciding row is the last of the pivot's list
            last = max(lists[9])
            assert ref.by_definition([case["records"][last]], case["patterns"]) == [0]
            assert last < len(case["records"]) - 1
    sl = ref.brute.spade_eid_view(cases["shared-launch"]["records"])
    occ = {i: sum(1 for s in sl.values() if any(i in X for X in s)) for i in (10, 11, 12)}
    assert occ == {10: 1, 11: 2, 12: 4 * T + 1}


@pytest.mark.parametrize("n", ref.ROW_LENGTHS)
def test_row_length_cases(n):
    case = ref.row_length_case(n)
    view = ref.brute.spade_eid_view(case["records"])
    assert [len({i for X in view[s] for i in X}) for s in (0, 1)] == [n, n]
    assert sorted(set(case["names"])) == sorted(ref.SEARCHED)
    assert ref.by_definition(case["records"], case["patterns"]) == case["expected"]


@pytest.mark.parametrize("W", ref.MASK_WIDTHS)
def test_mask_width_cases(W):
    case = ref.mask_width_case(W)
    view = ref.brute.spade_eid_view(case["records"])
    assert [len(view[s]) for s in (0, 1)] == [64 * W, 64 * W]
    assert len(case["triples"]) == (1 if W == 1 else 3)
    assert ref.by_definition(case["records"], case["patterns"]) == case["expected"]
    assert 0 in case["expected"] and 2 in case["expected"]


def test_long_pattern_case():
    case = ref.long_pattern_case()
    assert [sum(len(X) for X in p) for p in case["patterns"]] == [3000, 2999]
    assert ref.by_definition(case["records"], case["patterns"]) == case["expected"] == [3, 5]


def test_csr_forms_round_trip():
    pats = ref.hand_cases()["itemset_vs_sequence"]["patterns"]
    csr = ref.to_csr(pats)
    assert csr[0] is None and ref.csr_patterns(csr) == pats
    assert ref.csr_patterns(ref.to_csr([])) == []
