"""Supports of given patterns (fsm_patterns_support) next to the mine that produced them:

    python tools/bench_support.py [--only bible,sign,d1m,oracle] [--reps 3] > support.jsonl

Legs bible (BIBLE-shaped, minsup 0.4 %), sign (SIGN-shaped, 1.5 %) and d1m (Quest D1M, 0.1 %):
the DB is mined, the whole mined set is counted again on the same DB and the counts must
equal the mined supports.  One JSON line per leg: `ms_mine`, the first call's wall time (it
builds the DB's vertical index), the steady call's (median of --reps), the k_ps_* kernel
rows of both, the (pattern, row) containment tests of a call and their rate.
Leg oracle: oracle.pattern_support (one pattern at a time, one CPU thread) on a fixed sample
of 200 patterns of each of the other legs' shapes that ran, for a CPU per-pattern rate.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "spark-fsm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LEGS = {"bible": ("bible", {}, 0.004), "sign": ("sign", {}, 0.015), "d1m": ("quest", {"D": 1000000}, 0.001)}
SAMPLE = 200


def kernel_rows(ks):
    return [{"name": k["name"], "launches": k["launches"], "ms": round(k["ms"], 3), "alg_bytes": k["alg_bytes"],
             "GBps": round(k["alg_bytes"] / 1e9 / (k["ms"] / 1e3), 1) if k["ms"] else 0} for k in ks]


def pivot_tests(db_img, csr):
    """(pattern, row) tests of one call: the length of every pattern's shortest item list."""
    f1 = np.bincount(db_img["item"], minlength=db_img["items"])
    dense = np.searchsorted(db_img["item_val"], csr[3])
    first_item = csr[2][csr[1]]
    return int(np.minimum.reduceat(f1[dense], first_item[:-1]).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process, see _lib.py)
    import spark_fsm_amd as fsm
    from tools import gen
    want = [c for c in args.only.split(",") if c] or list(LEGS) + ["oracle"]
    samples = {}
    with fsm.Engine(0) as eng:
        for name in want:
            if name == "oracle":
                continue
            shape, kw, sup = LEGS[name]
            ds = getattr(gen, shape)(seed=1, **kw)
            db = eng.db_from_tokens(ds.sids, ds.seq_off, ds.tokens, fsm.MODE_SPADE)
            eng.spade_csr(db, sup)  # warmup
            csr, meta = eng.spade_csr(db, sup)
            ms_mine = eng.stats()["ms_mine"]
            t0 = time.perf_counter()
            got = eng.pattern_supports(db, csr)
            ms_first = (time.perf_counter() - t0) * 1000.0
            ks_first = eng.kernel_stats()
            assert np.array_equal(got, csr[0]), "%s: the recount differs from the mined supports" % name
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                got = eng.pattern_supports(db, csr)
                ts.append((time.perf_counter() - t0) * 1000.0)
            ks = eng.kernel_stats()
            assert np.array_equal(got, csr[0]), "%s: the second recount differs" % name
            ms = statistics.median(ts)
            tests = pivot_tests(eng.db_export(db), csr)
            ms_count = sum(k["ms"] for k in ks if k["name"] == "k_ps_count")
            print(json.dumps({
                "leg": name, "dataset": ds.name, "minsup": sup, "patterns": meta["n"], "items": int(len(csr[3])),
                "ms_mine": round(ms_mine, 3), "ms_first_call": round(ms_first, 3), "ms_steady_call": round(ms, 3),
                "steady_over_mine": round(ms / ms_mine, 3), "recount_equals_mine": True,
                "pattern_row_tests": tests,
                "tests_per_s_wall": round(tests / (ms / 1e3)), "tests_per_s_kernel": round(tests / (ms_count / 1e3)) if ms_count else 0,
                "patterns_per_s_wall": round(meta["n"] / (ms / 1e3)),
                "kernels_first_call": kernel_rows(ks_first), "kernels_steady_call": kernel_rows(ks)}), flush=True)
            idx = sorted(random.Random(200).sample(range(meta["n"]), min(SAMPLE, meta["n"])))
            so, it = csr[2].tolist(), csr[3].tolist()
            samples[name] = (ds, [tuple(tuple(it[so[s]:so[s + 1]]) for s in range(csr[1][p], csr[1][p + 1])) for p in idx],
                             [int(csr[0][p]) for p in idx])
            del csr, got
            db.free()
    if "oracle" in want:
        from oracle import oracle
        for name, (ds, pats, sups) in samples.items():
            t0 = time.perf_counter()
            got = [int(oracle.pattern_support(ds.seq_off, ds.tokens, p)) for p in pats]
            sec = time.perf_counter() - t0
            assert got == sups, "%s: the oracle differs from the mined supports" % name
            print(json.dumps({"leg": "oracle", "dataset": ds.name, "sample": len(pats), "ms_total": round(sec * 1e3, 3),
                              "ms_per_pattern": round(sec * 1e3 / len(pats), 4),
                              "patterns_per_s": round(len(pats) / sec, 1)}), flush=True)


if __name__ == "__main__":
    main()
