"""Per-row figures of the root F2's unordered pairs, on the CPU (numpy and tools/gen.py):

    python tools/f2_pair_stats.py quest --D 200000 --support 0.001 [--rows 20000] [--seed 1]
    python tools/f2_pair_stats.py recur --D 100000 --support 0.005

For the frequent entries of a row (one per distinct frequent item, its mask the eids it occurs
at) an unordered pair i < j has up to three keys, (i -> j), (j -> i) and (i, j), and an entry a
repeat key (i -> i) when it occurs at two eids.  k_f2_tri writes a wave step with one store
when no pair of the step has two kinds; this prints how often a pair has, and the row lengths
that choose the kernel's paths.  Item supports come from the whole DB, the per-row figures
from its first --rows rows.  Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def frequent_items(ds, minsup):
    tok, so = ds.tokens, ds.seq_off
    row = np.repeat(np.arange(len(so) - 1, dtype=np.int64), np.diff(so))
    keep = tok >= 0
    pairs = np.unique(row[keep] * (int(tok.max()) + 1) + tok[keep])
    items, sup = np.unique(pairs % (int(tok.max()) + 1), return_counts=True)
    return set(items[sup >= minsup].tolist())


def row_entries(tokens, freq):
    """(lo, hi, mask) arrays of the row's frequent entries; eids count the non-empty itemsets."""
    occ, eid, filled = {}, 0, False
    for t in tokens:
        if t == -1:
            eid += filled
            filled = False
        elif t >= 0:
            filled = True
            if t in freq:
                occ[t] = occ.get(t, 0) | (1 << eid)
    masks = [occ[i] for i in sorted(occ)]
    lo = np.array([(m & -m).bit_length() - 1 for m in masks], dtype=np.int64)
    hi = np.array([m.bit_length() - 1 for m in masks], dtype=np.int64)
    return lo, hi, masks


def stats(ds, support, rows):
    minsup = max(1, math.ceil(support * len(ds)))
    freq = frequent_items(ds, minsup)
    rows = min(rows, len(ds))
    tot = dict(entries=0, pairs=0, keys=0, multi=0, repeats=0, gt32=0, gt63=0, rows_multi=0)
    tk = ds.tokens.tolist()
    for r in range(rows):
        lo, hi, masks = row_entries(tk[ds.seq_off[r]:ds.seq_off[r + 1]], freq)
        n = len(masks)
        tot["entries"] += n
        tot["gt32"] += n > 32
        tot["gt63"] += n > 63
        rep = int((lo < hi).sum())
        tot["repeats"] += rep
        tot["keys"] += rep
        if n < 2:
            continue
        iu = np.triu_indices(n, 1)
        t0 = lo[iu[0]] < hi[iu[1]]
        t1 = lo[iu[1]] < hi[iu[0]]
        if max(masks) < 1 << 63:
            mk = np.array(masks, dtype=np.int64)
            t2 = (mk[iu[0]] & mk[iu[1]]) != 0
        else:
            t2 = np.array([(masks[a] & masks[b]) != 0 for a, b in zip(*iu)])
        kinds = t0.astype(np.int64) + t1 + t2
        assert kinds.min() >= 1  # two distinct entries always have a key
        tot["pairs"] += len(kinds)
        tot["keys"] += int(kinds.sum())
        m = int((kinds > 1).sum())
        tot["multi"] += m
        tot["rows_multi"] += m > 0
    return {
        "dataset": ds.name, "support": support, "minsup": minsup, "frequent_items": len(freq), "rows": rows,
        "entries_per_row": round(tot["entries"] / rows, 2),
        "pairs_per_row": round(tot["pairs"] / rows, 2),
        "keys_per_row": round(tot["keys"] / rows, 2),
        "multi_kind_pairs_pct": round(100.0 * tot["multi"] / max(tot["pairs"], 1), 3),
        "repeats_per_row": round(tot["repeats"] / rows, 3),
        "rows_with_multi_kind_pct": round(100.0 * tot["rows_multi"] / rows, 2),
        "rows_gt32_pct": round(100.0 * tot["gt32"] / rows, 2),
        "rows_gt63_pct": round(100.0 * tot["gt63"] / rows, 3),
    }


def main():
    from tools import gen
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", choices=["quest", "recur", "bible", "sign"])
    ap.add_argument("--D", type=int, default=0)
    ap.add_argument("--support", type=float, default=0.001)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    kw = {"D": a.D} if a.D else {}
    ds = gen.quest(a.D or 200000, seed=a.seed) if a.shape == "quest" else getattr(gen, a.shape)(seed=a.seed, **kw)
    print(json.dumps(stats(ds, a.support, a.rows)))


if __name__ == "__main__":
    main()
