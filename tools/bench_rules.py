"""Scores of given rules (fsm_rules_support) next to the mine that produced them:

    python tools/bench_rules.py [--only c4,oracle] [--reps 5] > rules.jsonl

Leg c4: the Kosarak-shaped 990K DB is mined with tsr_c4's parameters (tools/bench_configs.py:
k = 1000, minconf 0.5), the mined rules are scored again on the same DB, and supports and
confidences must equal the mined ones.  One JSON line: `ms_mine`, the first call's wall time,
the steady call's (median of --reps), the k_rs_count row, the (rule, row) tests of a call
(the sum of the pivots' list lengths) and their rate.
Leg oracle: oracle.rule_support (one rule at a time, one CPU thread) on a fixed sample of 200
of those rules, for a CPU per-rule rate.
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

SAMPLE = 200


def kernel_rows(ks):
    return [{"name": k["name"], "launches": k["launches"], "ms": round(k["ms"], 3), "alg_bytes": k["alg_bytes"],
             "GBps": round(k["alg_bytes"] / 1e9 / (k["ms"] / 1e3), 1) if k["ms"] else 0} for k in ks]


def pivot_tests(db_img, rules):
    """(rule, row) tests of one call: the length of the shortest item list of every rule's X."""
    f1 = np.bincount(db_img["item"], minlength=db_img["items"])
    val = db_img["item_val"]
    return int(sum(min(int(f1[np.searchsorted(val, x)]) for x in r[0]) for r in rules))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process, see _lib.py)
    import spark_fsm_amd as fsm
    from tools import bench_configs
    want = [c for c in args.only.split(",") if c] or ["c4", "oracle"]
    algo, shape, kw, (k, minconf) = bench_configs.CONFIGS["c4"]
    assert algo == "tsr"
    ds = bench_configs.dataset(shape, kw)
    with fsm.Engine(0) as eng:
        db = eng.db_from_tokens(ds.sids, ds.seq_off, ds.tokens, fsm.MODE_TSR)
        eng.tsr(db, k, minconf)  # warmup
        rules, meta = eng.tsr(db, k, minconf)
        ms_mine = eng.stats()["ms_mine"]
        mined = [(r[2], r[3]) for r in rules]
        if "c4" in want:
            t0 = time.perf_counter()
            sup, ante, conf = eng.rule_supports(db, rules)
            ms_first = (time.perf_counter() - t0) * 1000.0
            assert list(zip(sup.tolist(), conf.tolist())) == mined, "c4: the scores differ from the mined ones"
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                sup, ante, conf = eng.rule_supports(db, rules)
                ts.append((time.perf_counter() - t0) * 1000.0)
            ks = eng.kernel_stats()
            assert list(zip(sup.tolist(), conf.tolist())) == mined, "c4: the second scores differ"
            ms = statistics.median(ts)
            tests = pivot_tests(eng.db_export(db), rules)
            ms_count = sum(s["ms"] for s in ks if s["name"] == "k_rs_count")
            print(json.dumps({
                "leg": "c4", "dataset": ds.name, "k": k, "minconf": minconf, "rules": len(rules),
                "final_minsup": meta["final_minsup"], "items": sum(len(r[0]) + len(r[1]) for r in rules),
                "longest_side": max(max(len(r[0]), len(r[1])) for r in rules),
                "ms_mine": round(ms_mine, 3), "ms_first_call": round(ms_first, 3), "ms_steady_call": round(ms, 3),
                "reps": args.reps, "steady_over_mine": round(ms / ms_mine, 4), "scores_equal_mine": True,
                "rule_row_tests": tests, "tests_per_s_wall": round(tests / (ms / 1e3)),
                "tests_per_s_kernel": round(tests / (ms_count / 1e3)) if ms_count else 0,
                "rules_per_s_wall": round(len(rules) / (ms / 1e3)), "kernels_steady_call": kernel_rows(ks)}), flush=True)
        db.free()
    if "oracle" in want:
        from oracle import oracle
        idx = sorted(random.Random(200).sample(range(len(rules)), min(SAMPLE, len(rules))))
        t0 = time.perf_counter()
        got = [oracle.rule_support(ds.seq_off, ds.tokens, list(rules[i][0]), list(rules[i][1])) for i in idx]
        sec = time.perf_counter() - t0
        assert [(s, s / a) for s, a in got] == [mined[i] for i in idx], "the oracle differs from the mined rules"
        print(json.dumps({"leg": "oracle", "dataset": ds.name, "sample": len(idx), "ms_total": round(sec * 1e3, 3),
                          "ms_per_rule": round(sec * 1e3 / len(idx), 4), "rules_per_s": round(len(idx) / sec, 2)}), flush=True)


if __name__ == "__main__":
    main()
