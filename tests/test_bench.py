"""bench.py's plain run and --dump-outputs.

A plain run (no --full) times the SPADE steps and nothing else: its line has the
headline fields and none of the legs that take runs of their own.  --dump-outputs
writes the last timed step's pattern CSR as float64 .npy files, the same from run
to run of the same arguments.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from digest import pattern_digest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("support", "pat_off", "set_off", "items")


def test_dump_outputs_exact_and_capped(tmp_path, monkeypatch):
    """Arrays within the cap are written whole and exactly (float64 holds every int32 and
    the int64 offsets); one over its share is reduced to the same seeded sample each time,
    in index order, and the files stay within DUMP_MAX_BYTES together."""
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 12)
    big = np.arange(1000, dtype=np.int64) * 3 + (1 << 40)
    small = np.array([2**31 - 1, -(2**31), 0, 7, 9], dtype=np.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("big", "small")}
    b = {n: np.load(str(tmp_path / "b" / (n + ".npy"))) for n in ("big", "small")}
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["small"], small.astype(np.float64))
    assert 0 < a["big"].size < big.size and np.all(np.diff(a["big"]) > 0)
    assert np.all(np.isin(a["big"].astype(np.int64), big))
    assert all(np.array_equal(a[n], b[n]) for n in a)
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))) <= 1 << 12


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """`bench.py --steps 2 --warmup 1 --dump-outputs DIR` on a 20,000-sequence DB: one JSON
    line with the headline fields and no CPU / TSR / config-2 leg, and the dumped CSR is the
    pattern set an Engine returns for the same DB and minsup."""
    import spark_fsm_amd as fsm
    from tools import gen
    D, support = 20000, 0.005
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--sequences", str(D), "--support", str(support), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "joins/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(d["extra"]["joins"] / (d["ms_per_step"] / 1000.0))
    assert d["roofline"]["kernel"] and d["extra"]["kernels"]  # from the warmup mine
    assert not {"cpu_baseline", "tsr_c4", "c2_complete"} & set(d)
    assert "cpu_baseline_all_cores" not in d["extra"]
    got = [np.load(str(out / (n + ".npy"))) for n in NAMES]
    assert sorted(os.listdir(str(out))) == sorted(n + ".npy" for n in NAMES)
    assert all(a.dtype == np.float64 for a in got)
    ds = gen.quest(D, seed=1)
    with fsm.Engine(0) as eng:
        db = eng.db_from_tokens(ds.sids, ds.seq_off, ds.tokens, fsm.MODE_SPADE)
        try:
            csr, meta = eng.spade_csr(db, support, copy=True)
        finally:
            db.free()
    assert d["extra"]["patterns"] == meta["n"] == len(got[0])
    assert pattern_digest(*[a.astype(np.int64) for a in got]) == pattern_digest(*csr)
