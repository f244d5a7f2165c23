"""Sequence ids of given patterns (fsm_patterns_sids) next to the count of the same patterns:

    python tools/bench_sids.py [--only bible,sign,d1m] [--reps 3] [--max-sids N] > sids.jsonl

Legs bible (BIBLE-shaped, minsup 0.4 %), sign (SIGN-shaped, 1.5 %) and d1m (Quest D1M, 0.1 %),
as in tools/bench_support.py: the DB is mined (its sequence ids are 7, 10, 13, ..., not the row
numbers) and the ids of the whole mined set are asked for.  diff(off) must equal the mined
supports, and on a fixed sample of 200 patterns the ids must equal containment by definition
over the generated sequences.  One JSON line per leg: `ms_mine`, the first call's wall time (it
builds and orders the DB's vertical index), the steady call's (median of --reps, with their
spread), `n_sids`, the kernel rows of both, the write's GB/s on its stated bytes, and the steady
fsm_patterns_support call on the same input in the same process with the ratio of the two.
--max-sids (default 2^31) caps the result: a leg that needs more reports the total the library
states instead of allocating it.
"""
import argparse
import json
import os
import random
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "spark-fsm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tools.bench_support import LEGS, kernel_rows  # noqa: E402

SAMPLE = 200


def contains(seq, pattern):
    """brute._contains: the earliest itemset that holds each itemset of the pattern in turn."""
    pos = 0
    for X in pattern:
        while pos < len(seq) and not X <= seq[pos]:
            pos += 1
        if pos == len(seq):
            return False
        pos += 1
    return True


def sequence(ds, r):
    """Row r of a generated dataset as a list of itemsets (implicit timestamps 1, 2, ...)."""
    out, cur = [], set()
    for t in ds.tokens[ds.seq_off[r]:ds.seq_off[r + 1]].tolist():
        if t == -1:
            if cur:
                out.append(frozenset(cur))
            cur = set()
        elif t != -2:
            cur.add(t)
    return out


def check_sample(ds, sids, csr, off, sid, idx):
    """The ids of the patterns idx against the definition; only the rows that hold a pattern's
    rarest item are walked (no other row can contain it)."""
    row_of = np.repeat(np.arange(len(ds.sids)), np.diff(ds.seq_off))
    tok = ds.tokens[ds.seq_off[0]:ds.seq_off[-1]]
    items, counts = np.unique(tok[tok >= 0], return_counts=True)
    freq = dict(zip(items.tolist(), counts.tolist()))
    so, it = csr[2].tolist(), csr[3].tolist()
    seqs = {}
    for p in idx:
        pat = [frozenset(it[so[s]:so[s + 1]]) for s in range(csr[1][p], csr[1][p + 1])]
        rare = min((i for X in pat for i in X), key=lambda i: freq.get(i, 0))
        exp = []
        for r in np.unique(row_of[tok == rare]).tolist():
            if r not in seqs:
                seqs[r] = sequence(ds, r)
            if contains(seqs[r], pat):
                exp.append(int(sids[r]))
        got = sid[off[p]:off[p + 1]].tolist()
        assert got == exp, "pattern %d: the ids differ from the definition" % p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-sids", type=int, default=1 << 31)
    args = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process, see _lib.py)
    import spark_fsm_amd as fsm
    from tools import gen
    want = [c for c in args.only.split(",") if c] or list(LEGS)
    with fsm.Engine(0) as eng:
        for name in want:
            shape, kw, sup = LEGS[name]
            ds = getattr(gen, shape)(seed=1, **kw)
            sids = (7 + 3 * np.arange(len(ds.sids), dtype=np.int64)).astype(np.int32)
            db = eng.db_from_tokens(sids, ds.seq_off, ds.tokens, fsm.MODE_SPADE)
            eng.spade_csr(db, sup)  # warmup
            csr, meta = eng.spade_csr(db, sup)
            ms_mine = eng.stats()["ms_mine"]
            line = {"leg": name, "dataset": ds.name, "minsup": sup, "patterns": meta["n"], "items": int(len(csr[3])),
                    "ms_mine": round(ms_mine, 3), "max_sids": args.max_sids}
            t0 = time.perf_counter()
            try:
                off, sid = eng.pattern_sids(db, csr, max_sids=args.max_sids)
            except fsm.FsmError as e:
                if e.code != fsm.FSM_ELIMIT:
                    raise
                need = re.search(r"have (\d+) sequence ids", e.msg)
                line.update({"over_max_sids": True, "n_sids_needed": int(need.group(1)) if need else None,
                             "ms_refused_call": round((time.perf_counter() - t0) * 1000.0, 3)})
                print(json.dumps(line), flush=True)
                db.free()
                continue
            ms_first = (time.perf_counter() - t0) * 1000.0
            ks_first = eng.kernel_stats()
            assert np.array_equal(np.diff(off), csr[0]), "%s: diff(off) differs from the mined supports" % name
            idx = sorted(random.Random(200).sample(range(meta["n"]), min(SAMPLE, meta["n"])))
            check_sample(ds, sids, csr, off, sid, idx)
            n_sids = int(off[-1])
            del off, sid
            ts, tm = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                off, sid = eng.pattern_sids(db, csr, max_sids=args.max_sids)
                ts.append((time.perf_counter() - t0) * 1000.0)
                tm.append(sum(k["ms"] for k in eng.kernel_stats() if k["name"] == "k_ps_match"))
                ok = np.array_equal(np.diff(off), csr[0])
                del off, sid
                assert ok, "%s: a later call differs" % name
            ks = eng.kernel_stats()
            tc, tk = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                got = eng.pattern_supports(db, csr)
                tc.append((time.perf_counter() - t0) * 1000.0)
                tk.append(sum(k["ms"] for k in eng.kernel_stats() if k["name"] == "k_ps_count"))
            ks_count = eng.kernel_stats()
            assert np.array_equal(got, csr[0]), "%s: the recount differs from the mined supports" % name
            ms, ms_c = statistics.median(ts), statistics.median(tc)
            kms = {k["name"]: k["ms"] for k in ks}
            write = next((k for k in ks if k["name"] == "k_ps_sids_write"), None)
            ms_count, ms_match = statistics.median(tk), statistics.median(tm)
            line.update({
                "n_sids": n_sids, "diff_off_equals_mine": True, "sample_equals_definition": len(idx),
                "ms_first_call": round(ms_first, 3), "ms_steady_call": round(ms, 3),
                "ms_steady_calls": [round(t, 3) for t in ts],
                "ms_steady_kernels": round(sum(kms.values()), 3), "ms_steady_host": round(ms - sum(kms.values()), 3),
                "write_GBps": round(write["alg_bytes"] / 1e9 / (write["ms"] / 1e3), 1) if write and write["ms"] else 0,
                "ms_support_steady_call": round(ms_c, 3), "ms_support_steady_calls": [round(t, 3) for t in tc],
                "ms_k_ps_count": round(ms_count, 3), "ms_k_ps_count_reps": [round(t, 3) for t in tk],
                "ms_k_ps_match": round(ms_match, 3), "ms_k_ps_match_reps": [round(t, 3) for t in tm],
                "match_over_count": round(ms_match / ms_count, 3) if ms_count else 0,
                "sids_over_support_call": round(ms / ms_c, 3) if ms_c else 0,
                "kernels_first_call": kernel_rows(ks_first), "kernels_steady_call": kernel_rows(ks),
                "kernels_support_call": kernel_rows(ks_count)})
            print(json.dumps(line), flush=True)
            del csr, got
            db.free()


if __name__ == "__main__":
    main()
