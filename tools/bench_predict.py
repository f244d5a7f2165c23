"""Predictions per row from given rules (fsm_rules_predict) next to their scores
(fsm_rules_support) on the same rules and DB:

    python tools/bench_predict.py [--reps 5] [--topn 10] > predict.jsonl

The Kosarak-shaped 990K DB is mined with tsr_c4's parameters (tools/bench_configs.py: k = 1000,
minconf 0.5), and the mined rules predict on their own DB with topn = 10.  One JSON line:
`ms_mine`, the first predict call's wall time, the steady call's (median of --reps), its kernel
rows, the share of the steady call spent outside the kernels (host share), the rows with a
list, the entries, and the same first / steady / kernel figures of fsm_rules_support.  A sample
of rows is checked against the definition (tests/rule_predict_ref.py) before anything is timed.
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
for p in (ROOT, os.path.join(ROOT, "spark-fsm_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SAMPLE = 300


def kernel_rows(ks):
    return [{"name": k["name"], "launches": k["launches"], "ms": round(k["ms"], 3), "alg_bytes": k["alg_bytes"],
             "GBps": round(k["alg_bytes"] / 1e9 / (k["ms"] / 1e3), 1) if k["ms"] else 0} for k in ks]


def timed(fn, reps):
    t0 = time.perf_counter()
    first = fn()
    ms_first = (time.perf_counter() - t0) * 1000.0
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        last = fn()
        ts.append((time.perf_counter() - t0) * 1000.0)
    return first, last, ms_first, statistics.median(ts)


def check_sample(ds, rules, topn, off, item, rule):
    """The lists of SAMPLE rows against the definition, each row as a one-row DB."""
    import rule_predict_ref as ref
    off = off.tolist()
    rng = random.Random(300)
    n = len(off) - 1
    rows = sorted(rng.sample(range(n), min(SAMPLE, n)))
    so, tok = ds.seq_off.tolist(), ds.tokens
    for s in rows:
        line = " ".join(map(str, tok[so[s]:so[s + 1]].tolist()))
        want = ref.by_definition([(0, line)], rules, topn)[0]
        got = list(zip(item[off[s]:off[s + 1]].tolist(), rule[off[s]:off[s + 1]].tolist()))
        assert got == want, "row %d: %r, by definition %r" % (s, got, want)
    return len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--topn", type=int, default=10)
    args = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process, see _lib.py)
    import spark_fsm_amd as fsm
    from tools import bench_configs
    algo, shape, kw, (k, minconf) = bench_configs.CONFIGS["c4"]
    assert algo == "tsr"
    ds = bench_configs.dataset(shape, kw)
    with fsm.Engine(0) as eng:
        db = eng.db_from_tokens(ds.sids, ds.seq_off, ds.tokens, fsm.MODE_TSR)
        eng.tsr(db, k, minconf)  # warmup
        rules, meta = eng.tsr(db, k, minconf)
        ms_mine = eng.stats()["ms_mine"]
        csr = fsm.scored_rules_csr(rules)  # (the arrays are made once: the calls below time the library)

        first, last, p_first, p_steady = timed(lambda: eng.rule_predictions(db, csr, args.topn), args.reps)
        pks = eng.kernel_stats()
        assert all(np.array_equal(a, b) for a, b in zip(first, last)), "two predict calls differ"
        off, item, rule = last
        checked = check_sample(ds, rules, args.topn, off, item, rule)
        lens = np.diff(off)
        p_kernel = sum(s["ms"] for s in pks)

        sfirst, slast, s_first, s_steady = timed(lambda: eng.rule_supports(db, csr[:4]), args.reps)
        sks = eng.kernel_stats()
        assert list(zip(slast[0].tolist(), slast[2].tolist())) == [(r[2], r[3]) for r in rules], "the scores differ from the mined ones"
        s_kernel = sum(s["ms"] for s in sks)
        db.free()
    print(json.dumps({
        "dataset": ds.name, "k": k, "minconf": minconf, "rules": len(rules), "final_minsup": meta["final_minsup"],
        "items": sum(len(r[0]) + len(r[1]) for r in rules), "topn": args.topn, "rows": int(len(lens)),
        "rows_with_a_list": int(np.count_nonzero(lens)), "entries": int(off[-1]), "longest_list": int(lens.max()),
        "rows_checked_by_definition": checked, "ms_mine": round(ms_mine, 3), "reps": args.reps,
        "predict": {"ms_first_call": round(p_first, 3), "ms_steady_call": round(p_steady, 3), "ms_kernels": round(p_kernel, 3),
                    "host_share": round(1.0 - p_kernel / p_steady, 3) if p_steady else 0, "kernels_steady_call": kernel_rows(pks)},
        "support": {"ms_first_call": round(s_first, 3), "ms_steady_call": round(s_steady, 3), "ms_kernels": round(s_kernel, 3),
                    "host_share": round(1.0 - s_kernel / s_steady, 3) if s_steady else 0, "kernels_steady_call": kernel_rows(sks)},
        "predict_over_support": round(p_steady / s_steady, 2) if s_steady else 0}), flush=True)


if __name__ == "__main__":
    main()
