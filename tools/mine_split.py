"""Where the SPADE mines of a kernel trace begin (tools/ktrace_gaps.py, tools/pmc_summary.py).

Only the first unsharded mine of a DB handle launches k_f1 (the F1 supports stay with the
DB), so a mine is found by k_f1 where it has one and by its root plan otherwise:

  * a mine begins at k_f1;
  * else at its first root plan kernel (k_f2_plan_bound, k_f2_plan_db, k_root_count).  A plan
    kernel that follows a mine's start with no k_f2_count in between belongs to that mine
    (the plan behind a k_f1, or the exact plan behind a bounded one that passed the limits);
  * a mine that begins at a plan kernel also takes the small launches directly before it
    (the zeroed block's fill and the table uploads, k_copy_mapped), back to the previous
    mine's last copy: they are its first launches.

starts(names) takes the kernel names in launch order and returns the index of every mine's
first launch.  With another first kernel than k_f1 (ktrace_gaps.py --start) only that kernel
begins a mine.
"""
import re

PLAN = ("k_f2_plan_bound", "k_f2_plan_db", "k_root_count")
HEAD = ("k_copy_mapped", "fillBuffer")


def base(name):
    """k_f2_count of 'void fsm::(anonymous namespace)::k_f2_count<false, true>(...)'"""
    m = re.search(r"\b(k0?_\w+)", name)
    return m.group(1) if m else name


def starts(names, first="k_f1"):
    out = []
    counted = True  # the open mine's root F2 is counted (or no mine is open): a plan kernel opens the next
    for i, n in enumerate(names):
        b = base(n)
        if b == first:
            out.append(i)
            counted = False
        elif b in PLAN and counted and first == "k_f1":
            j = i
            lo = out[-1] + 1 if out else 0
            while j > lo and any(h in names[j - 1] for h in HEAD):
                j -= 1
            out.append(j)
            counted = False
        elif b == "k_f2_count" or b.startswith(("k_emit", "k_count")):  # (a root without rank groups: the lattice)
            counted = True
    return out


def split(rows, name_of, first="k_f1"):
    """rows (in launch order) cut into mines; what precedes the first mine is dropped"""
    s = starts([name_of(r) for r in rows], first)
    return [rows[a:z] for a, z in zip(s, s[1:] + [len(rows)])]
