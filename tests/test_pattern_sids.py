"""CPU tests of fsm_patterns_sids: the ABI surface without a device, and the reference and
generators of tests/pattern_sids_ref.py that the GPU tests hold the engine to."""
import ctypes
import os
import re
import subprocess

import pytest

import pattern_filter_ref as fref
import pattern_sids_ref as sref
import pattern_support_ref as ref
from spark_fsm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = ref.constants()["kPsTile"]


# ------------------------------------------------------------------ C1
def test_both_symbols_are_exported():
    assert os.path.exists(_lib.LIB_PATH), "libfsm.so not built"
    L = ctypes.CDLL(_lib.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (fsm_\w+)", out))
    for name in ("fsm_patterns_sids", "fsm_sidlists_free"):
        assert hasattr(L, name), name
        assert name in exported and name in _lib.EXPORTS, name


# ------------------------------------------------------------------ C2
def test_null_arguments_are_rejected_and_leave_out():
    """Without a device there is no context to pass: every argument NULL in turn with a NULL
    context (the GPU test repeats db, in and out with a live one)."""
    L = _lib.load()
    P = ctypes.POINTER
    pats = _lib.Patterns()
    out = ctypes.cast(0x1234, P(_lib.SidLists))  # a marker value, never followed
    dummy = ctypes.c_void_p(0x10)  # never dereferenced: the NULL context is rejected first
    for db, pin, po in ((dummy, ctypes.byref(pats), ctypes.byref(out)), (None, ctypes.byref(pats), ctypes.byref(out)),
                        (dummy, None, ctypes.byref(out)), (dummy, ctypes.byref(pats), None), (None, None, None)):
        assert L.fsm_patterns_sids(None, db, pin, 0, po) == _lib.FSM_EINVAL
        assert ctypes.cast(out, ctypes.c_void_p).value == 0x1234
    assert L.fsm_last_error(None)
    assert L.fsm_sidlists_free(None) is None


# ------------------------------------------------------------------ C3
def test_sidlists_layout_matches_c_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fsm.h"\nint main(void){\n'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(fsm_sidlists), offsetof(fsm_sidlists, n),'
                   ' offsetof(fsm_sidlists, off), offsetof(fsm_sidlists, sid), offsetof(fsm_sidlists, n_sids));\n'
                   'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.SidLists
    assert got == [ctypes.sizeof(S), S.n.offset, S.off.offset, S.sid.offset, S.n_sids.offset] == [32, 0, 8, 16, 24]


# ------------------------------------------------------------------ C4
def test_the_staging_constant_is_read_from_the_source():
    c = sref.constants()
    assert c["kPsTile"] == 64 and c["kPsSliceSids"] >= c["kPsTile"]
    assert set(ref.constants()) < set(c)


# ------------------------------------------------------------------ C5
@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_reference_lengths_are_the_supports_on_the_hand_cases(name):
    case = ref.hand_cases()[name]
    lists = sref.by_definition(case["records"], case["patterns"])
    assert [len(x) for x in lists] == ref.by_definition(case["records"], case["patterns"]) == case["expected"]
    assert all(x == sorted(set(x)) for x in lists)


def test_reference_on_the_stated_hand_lists():
    h = ref.hand_cases()
    got = sref.by_definition(h["one_sid_two_records"]["records"], h["one_sid_two_records"]["patterns"])
    assert got == [[7, 8], [7], [7], [7], [7], []]
    got = sref.by_definition(h["cannot_match"]["records"], h["cannot_match"]["patterns"])
    assert got == [[]] * 7 + [[0]]
    got = sref.by_definition(h["duplicates"]["records"], h["duplicates"]["patterns"])
    assert got == [[0, 1], [0, 1, 2], [0, 1], [0, 1, 2], [0, 1]]


def test_reference_lengths_are_the_supports_on_the_random_dbs():
    for seed in range(fref.N_RANDOM):
        recs, _sup = fref.random_db(seed)
        pats = ref.small_patterns(ref.items_of(recs))
        assert [len(x) for x in sref.by_definition(recs, pats)] == ref.by_definition(recs, pats), seed


# ------------------------------------------------------------------ C6
def test_tile_edge_lists_are_what_the_docstrings_say():
    for L in ref.tile_lengths(T):
        for place in ref.PIVOT_PLACES:
            for full in (True, False):
                case = ref.tile_edge_case(L, place, full)
                exp = sref.tile_edge_lists(case)
                assert len(exp[0]) == (L if full else L - 1)
                assert exp == sref.by_definition(case["records"], case["patterns"]), (L, place, full)


def test_added_cases_state_the_definition():
    for shape in sref.LANE_SHAPES:
        case = sref.lane_case(shape, T)
        assert case["expected"] == sref.by_definition(case["records"], case["patterns"]), shape
        mid = [s for s in case["expected"][0] if 10 + 3 * T <= s < 10 + 3 * 2 * T]
        assert len(mid) == {"lane0": 1, "lane63": 1, "even": T // 2, "none": 0}[shape]
    case = sref.dead_tiles_case(T)
    assert case["expected"] == sref.by_definition(case["records"], case["patterns"])
    assert sref.by_definition(case["records"], case["all_dead"]) == [[]] * len(case["all_dead"])
    case = sref.sid_case()
    assert case["expected"] == sref.by_definition(case["text"], case["patterns"])
    assert case["expected"] == sref.by_definition(case["merged"], case["patterns"])
    # neither record of sid 9 holds <(1)(2)> on its own
    for rec in case["text"]:
        if rec[0] == 9:
            assert sref.by_definition([rec], case["patterns"][:1]) == [[]]
