"""GPU parity along the sequence axis of a SPADE mine: supports far above 2.

The DBs come from edge_dbs.tall_spade: R short sequences mined at a minsup S in the hundreds and
thousands (and S = R in the dense DBs), whose decisions have support exactly S or exactly S - 1,
with the supporting rows placed on the row blocks of the root F2 (first, last and only rows of the
blocks Miner::f2_geometry derives for that R and FSM_F2_BLOCKS, the last row of a partial last
block, row 0 and row R - 1) and on blocks of 64 rows.  A lost increment turns an S into S - 1, a
repeated one an S - 1 into S: either changes the frequent set.  tests/test_edge_dbs.py proves the
DBs' claims without a GPU.

Every case compares patterns, supports, the join count, root_entries and the minsup with the CPU
oracle, bit for bit; a failure names the decisions that differ (R, policy, critical row, gadget).
The K0 cases compare both DB builds with the image by definition."""
import pytest

import edge_dbs as E
import pattern_filter_ref as ref
from test_edges_gpu import _assert_image, check_spade, gpu_spade, setenv, spade_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fsm():
    import spark_fsm_amd
    return spark_fsm_amd


@pytest.fixture(scope="module")
def eng(fsm):
    e = fsm.Engine(0)
    yield e
    e.close()


def check_tall(eng, db, text=False, root=True):
    """check_spade at the DB's own minsup; a failure names every decision that differs."""
    o = spade_ref(db, minsup=db.S)
    try:
        return check_spade(eng, db, text=text, root=root, minsup=db.S)
    except AssertionError as err:
        got = dict(gpu_spade(eng, db, text)[0])
        bad = ["%s: GPU %r, expected %d" % (db.where(p), got.get(p), db.S) for p in db.t2 if got.get(p) != db.S]
        bad += ["%s: GPU %d, expected none (%d)" % (db.where(p), got[p], db.S - 1) for p in db.t1 if p in got]
        other = len(set(got.items()) ^ set(o["patterns"]))
        raise AssertionError("%s (%s path): %d decisions differ: %s; %d (pattern, support) pairs differ in all; %s"
                             % (db.name, "text" if text else "token", len(bad), bad[:6], other, err)) from None


def tall_dbs(R):
    """The placed and the dense DB of R rows; at 65,537 rows also the near-dense one (minsup 65,535,
    lattice counts of 65,537)."""
    return [E.tall_case(R), E.tall_case(R, dense=True)] + ([E.tall_case(R, "near")] if R == E.TALL_NEAR_R else [])


# ------------------------------------------------------------ 1. every R under its own FSM_F2_BLOCKS
@pytest.mark.parametrize("R", E.tall_all_r())
def test_tall_rows(eng, R, monkeypatch):
    """The placed DB (every / edges / lone on the root F2's row blocks and on blocks of 64 rows, head,
    tail: minsup S = the most rows any of them needs) and the dense DB (S = R, decisions at R and
    R - 1) of each R, under the FSM_F2_BLOCKS that gives the geometry the DB is placed on.  Token
    path (device build) and text path."""
    setenv(monkeypatch, E.tall_env(R))
    for db in tall_dbs(R):
        st = check_tall(eng, db)
        assert st["k0_device"] == 1, db.name
        check_tall(eng, db, text=True)


# ------------------------------------------------------------ 2. the paths of a mine, at 4,097 and 16,385 rows
TALL_ENVS = ["", "FSM_F2_TRI=0", "FSM_ROOT_DB=0", "FSM_ROOT_PATH=atomic", "FSM_COUNT_PATH=keys",
             "FSM_COUNT_PATH=atomic FSM_COUNT_KERNEL=thread", "FSM_COUNT_PATH=sparse", "FSM_COUNT_CHUNK=256",
             "FSM_EMIT_PATH=chunk", "FSM_EMIT_CAP=0", "FSM_EMIT_GRID=256", "FSM_DEVORDER=0", "FSM_KIDS=host"]


@pytest.mark.parametrize("env", TALL_ENVS, ids=lambda e: e.replace(" ", ",") or "default")
@pytest.mark.parametrize("R", E.TALL_MATRIX_R)
def test_tall_paths(eng, R, env, monkeypatch):
    """The same DBs through every root, count, emit and ordering path the knobs select: counts summed
    over thousands of rows, blocks and regions, child id-lists of S entries spread over S parent
    runs, and the support >= minsup ballot at a minsup of 128 .. 16,385."""
    setenv(monkeypatch, (E.tall_env(R) + " " + env).strip())
    for db in tall_dbs(R):
        check_tall(eng, db)


# ------------------------------------------------------------ 3. the decisions recounted
@pytest.mark.parametrize("R", E.tall_all_r())
def test_tall_supports(eng, R):
    """k_ps_count on pivot lists of S rows: the support of every decision, given as a pattern, is
    exactly S where it holds and exactly S - 1 where it does not."""
    from spark_fsm_amd import MODE_SPADE
    for db in tall_dbs(R):
        h = eng.db_from_tokens(db.sids, db.seq_off, db.tokens, MODE_SPADE)
        try:
            got = eng.pattern_supports(h, db.t2 + db.t1).tolist()
        finally:
            h.free()
        want = [db.S] * len(db.t2) + [db.S - 1] * len(db.t1)
        bad = ["%s: GPU %d, expected %d" % (db.where(p), g, w) for p, g, w in zip(db.t2 + db.t1, got, want) if g != w]
        assert not bad, "%s: %d decisions differ: %s" % (db.name, len(bad), bad[:6])


# ------------------------------------------------------------ 4. closed / maximal on equal supports
@pytest.mark.parametrize("R", E.TALL_MATRIX_R)
def test_tall_filters(eng, R, monkeypatch):
    """filter_patterns on the mined sets: every frequent pattern of a placement has support exactly
    S, so the closed filter decides on equal supports throughout."""
    setenv(monkeypatch, E.tall_env(R))
    for db in tall_dbs(R):
        pats = gpu_spade(eng, db)[0]
        assert pats == spade_ref(db, minsup=db.S)["patterns"], db.name
        csr = ref.to_csr(pats)
        for keep in ref.KEEPS:
            out, idx = eng.filter_patterns(csr, keep)
            assert ref.csr_equal(out, ref.take(csr, idx)), (db.name, keep)
            assert idx.tolist() == ref.by_deletion(pats, keep) == ref.definitional(pats, keep), (db.name, keep)


# ------------------------------------------------------------ 5. in-process ranks
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=lambda d: "ranks%d" % len(d))
def test_tall_inproc_ranks(fsm, devices, monkeypatch):
    with fsm.Engine(devices=list(devices)) as e:
        for R in E.TALL_MATRIX_R:
            setenv(monkeypatch, E.tall_env(R))
            for db in tall_dbs(R):
                check_tall(e, db, root=False)
            monkeypatch.delenv("FSM_F2_BLOCKS", raising=False)


# ------------------------------------------------------------ 6. K0 and the scan on the same sizes
def _both_builds(eng, fsm, monkeypatch, sids, seq_off, tokens, mode):
    """(image, k0_device) of the device build and of the FSM_K0=host build."""
    out = []
    m = fsm.MODE_SPADE if mode == "spade" else fsm.MODE_TSR
    for k0 in ("device", "host"):
        if k0 == "host":
            monkeypatch.setenv("FSM_K0", "host")
        else:
            monkeypatch.delenv("FSM_K0", raising=False)
        h = eng.db_from_tokens(sids, seq_off, tokens, m)
        try:
            out.append((eng.db_export(h), eng.stats()["k0_device"]))
        finally:
            h.free()
    monkeypatch.delenv("FSM_K0", raising=False)
    return out


@pytest.mark.parametrize("R", E.K0_TALL_R)
def test_k0_tall_images(eng, fsm, R, monkeypatch):
    """The placed tall DBs around one scan tile of rows (4,096) and around one lap of k0_rows' waves
    (32,768 rows), in both modes: device build, host build and the image by definition all equal."""
    db = E.tall_case(R)
    for mode in ("spade", "tsr"):
        want = E._cached(("tall-image", R, mode), lambda: E.k0_image(db.rows, mode))
        (dev, used), (host, used_h) = _both_builds(eng, fsm, monkeypatch, db.sids, db.seq_off, db.tokens, mode)
        assert (used, used_h) == (1, 0), (R, mode)
        _assert_image(dev, want, (R, mode, "device"))
        _assert_image(host, want, (R, mode, "host"))


@pytest.mark.parametrize("variant", E.K0_STAGE_VARIANTS)
@pytest.mark.parametrize("R", E.K0_STAGE_R)
def test_k0_staging_chunks(eng, fsm, R, variant, monkeypatch):
    """Rows <x, -1> whose offsets and tokens end one short of, on and one past a 4 MiB staging chunk;
    the smallest / largest item value lies in the last row alone (at 524,289 rows a chunk of two
    tokens, narrowed on one thread) or in the first rows alone.  Both builds against the closed
    form of the image (edge_dbs.k0_stage_case; checked against k0_image in tests/test_edge_dbs.py)."""
    sids, seq_off, tokens, image = E.k0_stage_case(R, variant)
    for mode in ("spade", "tsr"):
        want = image(mode)
        (dev, used), (host, used_h) = _both_builds(eng, fsm, monkeypatch, sids, seq_off, tokens, mode)
        assert (used, used_h) == (1, 0), (R, variant, mode)
        _assert_image(dev, want, (R, variant, mode, "device"))
        _assert_image(host, want, (R, variant, mode, "host"))


@pytest.mark.parametrize("name", [c[0] for c in E.k0_extreme_cases()])
def test_k0_int32_extremes(eng, fsm, name, monkeypatch):
    """Item values up to INT32_MAX and down to INT32_MIN on the wave path and on the block path."""
    _, rows, modes = [c for c in E.k0_extreme_cases() if c[0] == name][0]
    db = E.EdgeDB(rows, name)
    for mode in modes:
        want = E.k0_image(rows, mode)
        (dev, used), (host, used_h) = _both_builds(eng, fsm, monkeypatch, db.sids, db.seq_off, db.tokens, mode)
        assert (used, used_h) == (1, 0), (name, mode)  # the value range is 2^20 + 1: the device build takes it
        _assert_image(dev, want, (name, mode, "device"))
        _assert_image(host, want, (name, mode, "host"))


class _Lead:
    """A DB whose token array carries leading tokens that belong to no row (seq_off[0] != 0)."""

    def __init__(self, db):
        self.db, self.name, self.sids, self.support = db, db.name + "+lead", db.sids, db.support
        self.seq_off, self.tokens = E.with_lead(db)


@pytest.mark.parametrize("R", [17, 4097])
def test_leading_tokens_belong_to_no_row(eng, fsm, R, monkeypatch):
    """seq_off[0] = 5: both builds give the image of the rows alone, and the mine its result."""
    db = E.tall_case(R)
    lead = _Lead(db)
    assert lead.seq_off[0] == len(E.K0_LEAD) and lead.tokens[:5].tolist() == list(E.K0_LEAD)
    for mode in ("spade", "tsr"):
        want = E._cached(("tall-image", R, mode), lambda: E.k0_image(db.rows, mode))
        (dev, used), (host, used_h) = _both_builds(eng, fsm, monkeypatch, lead.sids, lead.seq_off, lead.tokens, mode)
        assert (used, used_h) == (1, 0), (R, mode)
        _assert_image(dev, want, (R, mode, "device"))
        _assert_image(host, want, (R, mode, "host"))
    setenv(monkeypatch, E.tall_env(R))
    o = spade_ref(db, minsup=db.S)
    for k0 in ("device", "host"):
        if k0 == "host":
            monkeypatch.setenv("FSM_K0", "host")
        pats, meta, st = gpu_spade(eng, lead)
        assert st["k0_device"] == (1 if k0 == "device" else 0)
        assert meta["minsup"] == db.S and pats == o["patterns"] and st["joins"] == o["joins"], (R, k0)
        assert st["root_entries"] == db.root_entries(), (R, k0)
