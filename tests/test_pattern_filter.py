"""CPU tests of the closed / maximal pattern filter: the entry point rejects bad
arguments before any device use, and the two references of the GPU tests
(tests/pattern_filter_ref.py) agree with each other and with the stated answers."""
import ctypes

import pytest

import pattern_filter_ref as ref
import spark_fsm_amd as fsm
from spark_fsm_amd import _lib

KEEP_CODES = {"closed": fsm.KEEP_CLOSED, "maximal": fsm.KEEP_MAXIMAL}


def test_null_arguments_are_einval():
    L = _lib.load()
    out = ctypes.POINTER(_lib.Patterns)()
    pats = _lib.Patterns()
    assert L.fsm_patterns_filter(None, ctypes.byref(pats), KEEP_CODES["closed"], ctypes.byref(out), None) == _lib.FSM_EINVAL
    assert L.fsm_patterns_filter(None, None, KEEP_CODES["maximal"], None, None) == _lib.FSM_EINVAL
    assert b"null" in L.fsm_last_error(None)
    assert not out


def test_constants_and_keep_names():
    assert KEEP_CODES == {"closed": 1, "maximal": 2}
    import inspect
    for fn in (fsm.Engine.spade_csr, fsm.Engine.spade, fsm.extract_rdd_patterns):
        assert inspect.signature(fn).parameters["keep"].default == "all"
    assert "fsm_patterns_filter" in _lib.EXPORTS


@pytest.mark.parametrize("seed", range(ref.N_RANDOM))
def test_references_agree_on_mined_random_dbs(seed):
    recs, _sup, pats = ref.mined_random_db(seed)
    assert 0 < len(pats) <= ref.MAX_RANDOM_PATTERNS and len(recs) <= 30
    for keep in ref.KEEPS:
        kept = ref.definitional(pats, keep)
        assert kept == ref.by_deletion(pats, keep)
        assert kept  # the longest pattern always stays
    # closed is a superset of maximal
    assert set(ref.definitional(pats, "maximal")) <= set(ref.definitional(pats, "closed"))


@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_hand_cases(name):
    pats = ref.hand_cases()[name]
    for keep in ref.KEEPS:
        kept = ref.definitional(pats, keep)
        assert kept == ref.by_deletion(pats, keep), keep
        if name in ref.KNOWN:
            assert kept == ref.KNOWN[name][keep], keep


def test_geometry_sets_have_their_sizes():
    sets = ref.geometry_sets()
    assert len(sets["prefix300"]) == 300 and sum(len(s) for s, _ in sets["prefix300"]) == 45150
    for n in (1023, 1024, 1025, 2047, 2048, 2049):
        assert len(sets["level_n%d" % n]) == n
    for t in (255, 256, 257):
        assert sum(len(X) for s, _ in sets["items%d" % t] for X in s) == t
    for keep in ref.KEEPS:
        assert ref.by_deletion(sets["prefix300"], keep) == [299] == ref.definitional(sets["prefix300"], keep)
        pats = sets["level_n1025"]
        assert ref.by_deletion(pats, keep) == ref.definitional(pats, keep)


def test_csr_round_trip_and_take():
    pats = ref.hand_cases()["singleton_between_itemsets"]
    csr = ref.to_csr(pats)
    assert ref.from_csr(csr) == pats
    assert ref.from_csr(ref.take(csr, [1, 3, 4])) == [pats[1], pats[3], pats[4]]
    assert ref.from_csr(ref.take(csr, [])) == []
