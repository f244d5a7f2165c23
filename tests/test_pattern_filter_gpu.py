"""GPU tests of fsm_patterns_filter (closed / maximal patterns of a complete frequent
set): the set AND order of the kept patterns and kept_idx against the two references
of tests/pattern_filter_ref.py, for both keep values."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pattern_filter_ref as ref
import spark_fsm_amd as fsm
from spark_fsm_amd import _lib
from tools import gen

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# case 5: sign-shaped generator prefix chosen on the CPU with oracle.spade_tokens_csr:
# gen.sign(D=200, seed=1) at support 0.07 (minsup 15) has a complete set of 51,490 patterns
# (235,948 items), of which 49,460 are closed and 24,115 maximal
MEDIUM = {"D": 200, "seed": 1, "support": 0.07, "n": 51490, "n_items": 235948, "closed": 49460, "maximal": 24115}


@pytest.fixture(scope="module")
def eng():
    with fsm.Engine(0) as e:
        yield e


def run_filter(eng, csr, keep):
    out, idx = eng.filter_patterns(csr, keep)
    assert idx.dtype == np.int64
    assert ref.csr_equal(out, ref.take(csr, idx)), "the result is not the kept patterns in input order"
    return idx.tolist()


def check_list(eng, pats, both=True):
    csr = ref.to_csr(pats)
    got = {}
    for keep in ref.KEEPS:
        got[keep] = run_filter(eng, csr, keep)
        assert got[keep] == ref.by_deletion(pats, keep), keep
        if both:
            assert got[keep] == ref.definitional(pats, keep), keep
    return got


# ------------------------------------------------------------------ 1. hand-built CSRs
def test_empty_set(eng):
    csr = (np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int32))
    for keep in ref.KEEPS:
        out, idx = eng.filter_patterns(csr, keep)
        assert len(idx) == 0 and [len(a) for a in out] == [0, 1, 1, 0]
        assert out[1].tolist() == [0] and out[2].tolist() == [0]


@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_hand_cases(eng, name):
    got = check_list(eng, ref.hand_cases()[name])
    if name in ref.KNOWN:
        assert got == ref.KNOWN[name]


# ------------------------------------------------------------------ 2. geometry
@pytest.mark.parametrize("name", sorted(ref.geometry_sets()))
def test_geometry(eng, name):
    pats = ref.geometry_sets()[name]
    got = check_list(eng, pats, both=len(pats) <= 400)
    if name == "prefix300":
        assert got == {"closed": [299], "maximal": [299]}


def test_pattern_longer_than_a_block(eng):
    """One 3,000-item pattern and its 3,000 one-item deletions, equal support (9 M items)."""
    csr = ref.long_pattern_csr()
    pats = ref.long_pattern_list()
    assert len(pats) == 3001 and ref.from_csr(ref.take(csr, [0, 1, 3000])) == [pats[0], pats[1], pats[3000]]
    for keep in ref.KEEPS:
        assert run_filter(eng, csr, keep) == [0] == ref.definitional(pats, keep)


# ------------------------------------------------------------------ 3. forced collisions
@pytest.mark.parametrize("bits", ["0", "3"])
def test_forced_hash_collisions(eng, bits):
    """FSM_PF_HASH_BITS keeps only the low bits of every hash (0: one chain that wraps the
    table): the exact check after a hash match must give the unhooked result."""
    env = dict(os.environ, FSM_PF_HASH_BITS=bits)
    r = subprocess.run([sys.executable, os.path.join(HERE, "pattern_filter_ref.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    sets = ref.collision_sets()
    assert sorted(got) == sorted(sets)
    for name, pats in sets.items():
        assert len(pats) <= 2049
        csr = ref.to_csr(pats)
        for keep in ref.KEEPS:
            assert got[name][keep] == run_filter(eng, csr, keep) == ref.by_deletion(pats, keep), (name, keep)


# ------------------------------------------------------------------ 4. mined, tiny, definitional
@pytest.mark.parametrize("seed", range(ref.N_RANDOM))
def test_mined_random_db(eng, seed):
    recs, sup, complete = ref.mined_random_db(seed)
    db = eng.db_from_spmf(recs, fsm.MODE_SPADE)
    try:
        full, _ = eng.spade(db, sup)
        assert sorted(full) == complete
        for keep in ref.KEEPS:
            exp = {complete[i] for i in ref.definitional(complete, keep)}
            got, meta = eng.spade(db, sup, keep=keep)
            assert got == [p for p in full if p in exp], keep  # the kept patterns in the mine's order
            assert len(got) == len(exp) == meta["n"] and meta["n_mined"] == len(full)
    finally:
        db.free()


def test_extract_rdd_patterns_keep(eng):
    recs, sup, complete = ref.mined_random_db(0)
    exp = sorted(complete[i] for i in ref.definitional(complete, "closed"))
    got = fsm.extract_rdd_patterns(recs, sup, stats=False, engine=eng, keep="closed")
    assert sorted((p.itemsets, p.support) for p in got) == exp
    with pytest.raises(ValueError):
        eng.filter_patterns(ref.to_csr(complete), "open")


# ------------------------------------------------------------------ 5. mined, medium
@pytest.fixture(scope="module")
def medium(eng):
    ds = gen.sign(D=MEDIUM["D"], seed=MEDIUM["seed"])
    db = eng.db_from_tokens(ds.sids, ds.seq_off, ds.tokens, fsm.MODE_SPADE)
    csr, meta = eng.spade_csr(db, MEDIUM["support"], copy=True)
    pats = ref.from_csr(csr)
    exp = {keep: ref.by_deletion(pats, keep) for keep in ref.KEEPS}
    yield {"db": db, "csr": csr, "meta": meta, "exp": exp}
    db.free()


def test_medium_mined_set(eng, medium):
    csr, meta = medium["csr"], medium["meta"]
    assert meta["n"] == MEDIUM["n"] and len(csr[3]) == MEDIUM["n_items"]
    lines = fsm.PatternSet.from_csr(csr, meta).serialize().splitlines(keepends=True)
    assert len(lines) == MEDIUM["n"]
    for keep in ref.KEEPS:
        exp = medium["exp"][keep]
        assert len(exp) == MEDIUM[keep]
        assert run_filter(eng, csr, keep) == exp
        out, m2 = eng.spade_csr(medium["db"], MEDIUM["support"], keep=keep)
        assert ref.csr_equal(out, ref.take(csr, exp))
        assert m2["n"] == len(exp) and m2["n_mined"] == MEDIUM["n"]
        assert (m2["total"], m2["minsup"]) == (meta["total"], meta["minsup"])
        assert fsm.PatternSet.from_csr(out, m2).serialize() == "".join(lines[i] for i in exp)


# ------------------------------------------------------------------ 6. errors and contexts
def _raw(eng, csr, keep, n=None, n_sets=None, n_items=None, want_idx=True):
    sup, po, so, it = (np.ascontiguousarray(a, dt) for a, dt in zip(csr, (np.int32, np.int64, np.int64, np.int32)))
    P = ctypes.POINTER
    pats = _lib.Patterns(len(sup) if n is None else n, sup.ctypes.data_as(P(ctypes.c_int32)),
                         po.ctypes.data_as(P(ctypes.c_int64)), so.ctypes.data_as(P(ctypes.c_int64)),
                         it.ctypes.data_as(P(ctypes.c_int32)), len(so) - 1 if n_sets is None else n_sets,
                         len(it) if n_items is None else n_items, 77, 3)
    out = P(_lib.Patterns)()
    idx = np.full(max(len(sup), 1), -1, np.int64)
    rc = eng._L.fsm_patterns_filter(eng._ctx, ctypes.byref(pats), keep, ctypes.byref(out),
                                    idx.ctypes.data_as(P(ctypes.c_int64)) if want_idx else None)
    res = None
    if rc == _lib.FSM_OK:
        o = out.contents
        res = {"n": o.n, "total": o.total, "minsup": o.minsup, "idx": idx[:o.n].tolist(),
               "support": [o.support[i] for i in range(o.n)]}
        eng._L.fsm_patterns_free(out)
    else:
        assert not out
    return rc, res


GOOD = ([5, 5, 4], [0, 1, 2, 3], [0, 1, 3, 4], [1, 1, 2, 1])  # <(1)> 5, <(1 2)> 5, <(1)> 4


def _bad(sup=GOOD[0], po=GOOD[1], so=GOOD[2], it=GOOD[3]):
    return (sup, po, so, it)


MALFORMED = {
    "pat_off_not_monotone": _bad(po=[0, 2, 1, 3]),
    "pat_off_end": _bad(po=[0, 1, 2, 2]),
    "pat_off_start": _bad(po=[1, 1, 2, 3]),
    "pat_off_negative": _bad(po=[0, -1, 2, 3]),
    "pat_off_past_the_end": _bad(po=[0, 9, 2, 3]),
    "set_off_end": _bad(so=[0, 1, 3, 3]),
    "set_off_start": _bad(so=[1, 1, 3, 4]),
    "set_off_not_monotone": _bad(so=[0, 3, 1, 4]),
    "set_off_negative": _bad(so=[0, -2, 3, 4]),
    "set_off_past_the_end": _bad(so=[0, 99, 3, 4]),
    "pattern_without_itemsets": _bad(po=[0, 1, 1, 3]),
    "empty_itemset": _bad(so=[0, 1, 1, 4], it=[1, 5, 6, 7]),
    "items_descending": _bad(it=[1, 2, 1, 1]),
    "items_equal": _bad(it=[1, 1, 1, 1]),
}


def test_errors_and_statistics(eng, medium):
    # a mine first, so that stats() holds figures the filter must not touch
    eng.spade_csr(medium["db"], MEDIUM["support"])
    before = eng.stats()
    assert before["patterns"] == MEDIUM["n"]
    for name, csr in MALFORMED.items():
        for keep in (fsm.KEEP_CLOSED, fsm.KEEP_MAXIMAL):
            rc, _ = _raw(eng, csr, keep)
            assert rc == _lib.FSM_EINVAL, name
            assert eng._L.fsm_last_error(eng._ctx), name
    for keep in (0, 3, -1):
        assert _raw(eng, GOOD, keep)[0] == _lib.FSM_EINVAL
    assert _raw(eng, GOOD, fsm.KEEP_CLOSED, n=-1)[0] == _lib.FSM_EINVAL
    assert _raw(eng, GOOD, fsm.KEEP_CLOSED, n=0)[0] == _lib.FSM_EINVAL  # itemsets without patterns
    # the limits are checked before any array is read
    assert _raw(eng, GOOD, fsm.KEEP_CLOSED, n=(1 << 32) - 2)[0] == _lib.FSM_ELIMIT
    assert _raw(eng, GOOD, fsm.KEEP_MAXIMAL, n_items=(1 << 32) - 2)[0] == _lib.FSM_ELIMIT
    assert _raw(eng, GOOD, fsm.KEEP_MAXIMAL, n_items=(1 << 32) - 3)[0] == _lib.FSM_EINVAL
    assert eng._L.fsm_patterns_filter(eng._ctx, None, 1, None, None) == _lib.FSM_EINVAL
    # a following valid call still works; total and minsup are copied; kept_idx may be NULL
    rc, res = _raw(eng, GOOD, fsm.KEEP_CLOSED)
    assert rc == _lib.FSM_OK and res == {"n": 2, "total": 77, "minsup": 3, "idx": [1, 2], "support": [5, 4]}
    rc, res = _raw(eng, GOOD, fsm.KEEP_MAXIMAL, want_idx=False)
    assert rc == _lib.FSM_OK and res["n"] == 1 and res["support"] == [5]
    ks = eng.kernel_stats()
    assert [k["name"] for k in ks] == ["k_pf_hash", "k_pf_insert", "k_pf_probe"]
    assert all(k["alg_bytes"] > 0 and k["launches"] == 1 for k in ks)
    assert eng.stats() == before


def test_group_engine_filters_on_rank0(eng, medium):
    with fsm.Engine(devices=[0, 0]) as grp:
        for keep in ref.KEEPS:
            assert run_filter(grp, medium["csr"], keep) == medium["exp"][keep]
        assert [k["name"] for k in grp.kernel_stats()] == ["k_pf_hash", "k_pf_insert", "k_pf_probe"]
