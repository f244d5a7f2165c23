"""The closed / maximal pattern filter (fsm_patterns_filter) on the two word-stream
BASELINE configs, next to the mine it follows:

    python tools/bench_filter.py [--only c5-bible,c5-sign] [--reps 3] > filter.jsonl

One JSON line per config: patterns in, and for each keep value the patterns kept, the
wall time of the whole call (median of --reps after one warmup; input checks, upload,
kernels, read-back and host compaction), the device time of each kernel with the GB/s on
its algorithmic bytes, and `ms_mine` of the mine that produced the input.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "spark-fsm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIGS = {"c5-bible": ("bible", 0.004), "c5-sign": ("sign", 0.015)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process, see _lib.py)
    import spark_fsm_amd as fsm
    from tools import gen
    want = [c for c in args.only.split(",") if c] or list(CONFIGS)
    with fsm.Engine(0) as eng:
        for name in want:
            shape, sup = CONFIGS[name]
            ds = getattr(gen, shape)(seed=1)
            db = eng.db_from_tokens(ds.sids, ds.seq_off, ds.tokens, fsm.MODE_SPADE)
            eng.spade_csr(db, sup)  # warmup
            csr, meta = eng.spade_csr(db, sup)
            ms_mine = eng.stats()["ms_mine"]
            db.free()
            out = {"config": name, "dataset": ds.name, "minsup": sup, "patterns_in": meta["n"],
                   "items_in": int(len(csr[3])), "ms_mine": round(ms_mine, 3)}
            for keep in ("closed", "maximal"):
                eng.filter_patterns(csr, keep)  # warmup
                ts = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    kept, idx = eng.filter_patterns(csr, keep)
                    ts.append((time.perf_counter() - t0) * 1000.0)
                ks = eng.kernel_stats()
                ms = statistics.median(ts)
                out[keep] = {"patterns_kept": int(len(idx)), "ms_filter_wall": round(ms, 3),
                             "ms_kernels": round(sum(k["ms"] for k in ks), 3),
                             "filter_over_mine": round(ms / ms_mine, 3),
                             "kernels": [{"name": k["name"], "ms": round(k["ms"], 3), "alg_bytes": k["alg_bytes"],
                                          "GBps": round(k["alg_bytes"] / 1e9 / (k["ms"] / 1e3), 1) if k["ms"] else 0}
                                         for k in ks]}
                del kept, idx
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
