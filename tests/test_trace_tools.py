"""tools/ktrace_gaps.py and tools/pmc_summary.py find the mines of a trace in which only a
handle's first mine launches k_f1: the later ones begin at their root plan (with the small
launches before it).  The fixture is a hand-written launch list of three mines behind a DB
build; one variant has its last mine on the exact plan, one falls back from the bounded plan
to the exact one inside its last mine."""
import csv
import importlib
import os

import pytest

FILL = "__amd_rocclr_fillBufferAligned"
COPY = "__amd_rocclr_copyBuffer"
MAPPED = "fsm::k_copy_mapped(void*, void const*, unsigned long)"
NS = "void fsm::(anonymous namespace)::"


def k(name, targs=""):
    return NS + name + targs + "(unsigned int const*, unsigned int)"


BUILD = [k("k0_count"), "void fsm::k_scan<unsigned int>(unsigned int const*)", k("k0_write"), COPY]
LEVEL = [k("k_rk_hist"), k("k_emit2", "<1, true>"), MAPPED, FILL, k("k_count2", "<1>"), k("k_freq_recs"), COPY]
TAIL = [MAPPED, COPY]  # the last level's table upload and the pair test counter's read-back


def root(plan):
    return plan + [FILL, "void fsm::k_scan<unsigned int>(unsigned int const*)", COPY, k("k_f2_tri"), MAPPED,
                   k("k_f2_count", "<false, true>"), COPY]


BOUND = [k("k_f2_plan_bound"), k("k_mem_db")]
EXACT = [k("k_f2_plan_db")]
# a handle's first mine: k_f1 and its read-back, the one-time tables, then the plan
MINE0 = [FILL, FILL, k("k_f1"), COPY, k("k_db_pos"), COPY, MAPPED, MAPPED, k("k_f2_bound_tab"), COPY] + root(BOUND) + \
    LEVEL + TAIL
HEAD = [FILL, MAPPED, MAPPED]  # a later mine's first launches: the zeroed block, the two table uploads


def later(plan, levels):
    return HEAD + root(plan) + LEVEL * levels + TAIL


VARIANTS = {
    "bound": [MINE0, later(BOUND, 2), later(BOUND, 1)],
    "last_exact": [MINE0, later(BOUND, 2), later(EXACT, 1)],
    # the bounded plan passed the limits: the exact plan runs behind it in the same mine
    "fallback": [MINE0, later(BOUND, 2), HEAD + BOUND + [FILL, COPY] + root(EXACT) + LEVEL + TAIL],
}


def tool(name):
    return importlib.import_module("tools." + name)


def launches(mines):
    """(dispatch id, kernel name) of the whole run, and every mine's dispatch ids; a mine that
    starts at k_f1 is found from k_f1 on (the fills before it go to what precedes it)"""
    names = list(BUILD)
    ids = []
    for m in mines:
        skip = 0
        while k("k_f1") in m and m[skip] != k("k_f1"):
            skip += 1
        names += m[:skip]
        ids.append(list(range(len(names) + 1, len(names) + 1 + len(m) - skip)))
        names += m[skip:]
    return list(enumerate(names, 1)), ids


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_mine_split_starts(variant):
    ms = tool("mine_split")
    disp, ids = launches(VARIANTS[variant])
    got = ms.starts([n for _, n in disp])
    assert [i + 1 for i in got] == [m[0] for m in ids]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("pick", [None, 1, 2, 0])
def test_ktrace_gaps_picks_the_mine(variant, pick, tmp_path, capsys, monkeypatch):
    disp, ids = launches(VARIANTS[variant])
    path = tmp_path / "run_kernel_trace.csv"
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Kind", "Kernel_Name", "Start_Timestamp", "End_Timestamp"])
        for i, n in disp:  # 10 us apart, 4 us long
            w.writerow(["KERNEL_DISPATCH", n, 1000000 + 10000 * i, 1000000 + 10000 * i + 4000])
    argv = ["ktrace_gaps.py", str(path)] + ([] if pick is None else ["--mine", str(pick)])
    monkeypatch.setattr("sys.argv", argv)
    tool("ktrace_gaps").main()
    out = capsys.readouterr().out.strip().split("\n")
    want = ids[-1 if pick is None else pick]
    lines, total = out[:-1], out[-1]
    assert len(lines) == len(want)
    assert "of 3:" in total and "%d launches" % len(want) in total
    by_id = dict(disp)
    short = tool("ktrace_gaps").short
    assert [ln.split(None, 4)[4] for ln in lines] == [short(by_id[i]) for i in want]  # (t, "+", gap, length, name)
    # the offsets restart at the mine's first launch
    assert float(lines[0].split()[0]) == 0.0
    assert abs(float(lines[-1].split()[0]) - 0.010 * (len(want) - 1)) < 1e-9


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_pmc_summary_picks_the_mine(variant, tmp_path):
    pmc = tool("pmc_summary")
    disp, ids = launches(VARIANTS[variant])
    # a pass of two counters: two rows per dispatch, written dispatch by dispatch
    rows = [{"Dispatch_Id": str(i), "Kernel_Name": n, "Counter_Name": c, "Counter_Value": "1"}
            for i, n in disp for c in ("SQ_WAVES", "SQ_INSTS_VALU")]
    did = lambda rs: sorted({int(r["Dispatch_Id"]) for r in rs})
    assert did(pmc.last_mine(rows)) == ids[2]
    assert did(pmc.nth_mine(rows, 1)) == ids[1]
    assert did(pmc.nth_mine(rows, 0)) == ids[0]
    assert len(pmc.last_mine(rows)) == 2 * len(ids[2])
    # through the command line: the last mine's dispatch counts per kernel
    d = tmp_path / "pass" / "host"
    os.makedirs(d)
    with open(d / "run_counter_collection.csv", "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)
    import json
    import subprocess
    import sys
    out = tmp_path / "summary.json"
    subprocess.run([sys.executable, os.path.join(os.path.dirname(pmc.__file__), "pmc_summary.py"), "--last-mine",
                    str(out), str(tmp_path / "pass")], check=True, capture_output=True)
    ks = json.load(open(out))["kernels"]
    by_id = dict(disp)
    assert "k_f1" not in ks and "k_f2_bound_tab" not in ks
    assert ks["k_f2_keys"]["dispatches"] == 1 and ks["k_f2_count"]["dispatches"] == 1
    assert ks["k_f2_plan"]["dispatches"] == sum(1 for i in ids[2] if "k_f2_plan" in by_id[i] or "k_mem_db" in by_id[i])
    assert sum(v["dispatches"] for v in ks.values()) == len(ids[2])


def test_trace_without_a_mine_is_kept_whole():
    pmc = tool("pmc_summary")
    rows = [{"Dispatch_Id": str(i), "Kernel_Name": n, "Counter_Name": "SQ_WAVES", "Counter_Value": "1"}
            for i, n in enumerate(BUILD, 1)]
    assert pmc.last_mine(rows) == rows
