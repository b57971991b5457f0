#!/usr/bin/env python3
"""Filter alternatives (AND-groups joined by OR) against the calls they replace, same
answers, one process.

Workload: lineitem (default SF10) read from a file on one GPU, its compressed
image resident in HBM after the warm-up.  The arms alternate (one warm-up each,
then --reps repetitions; medians and spread, max - min, of the host clock
around the synchronous call).  Everything is fixed before the first run:

  rev = sum_expr(l_extendedprice * (1 - l_discount)); aggs = [rev, count(*)]
  base = l_shipinstruct = 'DELIVER IN PERSON' AND l_shipmode IN ('AIR', 'REG AIR')
  parts_i = the key set of the l_partkey values with key % 25 == i (i = 0, 1, 2: disjoint, 4 % of the parts each)
  branch_i = l_partkey IN parts_i AND l_quantity in [1, 11] / [10, 20] / [20, 30]

  Q19    one call:  aggregate(aggs) under base AND AnyOf(branch_0, branch_1, branch_2)      (TPC-H Q19's lineitem side)
  Q19x3  the parent's way: three calls, aggregate(aggs) under base AND branch_i, summed -- valid because the part
         sets are disjoint, so no row is in two branches
  Q19np  the base-filter scan delivering l_partkey, l_quantity, l_extendedprice, l_discount, the OR in numpy
  base   aggregate(aggs) under base alone: what the alternatives are added to
  closed aggregate(aggs) under base AND AnyOf(two branches of ordinary terms): alt_kernel alone, no plane, no merge

Arms that must agree are checked in every repetition.  No ratio is fixed in
advance: an arm counts as faster than another when the medians differ by more
than the larger spread of the two (DESIGN.md section 24's rule).

With --parent-pkg DIR (a built checkout of the parent commit's package directory)
the calls without alternatives -- Q6, Q1 grouped, count(*) GROUP BY l_orderkey
hashed -- run on the parent's and this build in one process, alternating per
repetition, and the differences are set against the parent's own spread.

    python scripts/alt_rate.py --scale 10 --reps 5 --parent-pkg ../parent/duckdb-fastlane_amd \\
        > profiles/alt/alt_rate_sf10.txt

Kernel times come from runs of their own under the profiler: --trace ARM makes
only four calls of that arm, and --summarize DIR reads the kernel trace such a
run left (full batches only: the last batch of a call is smaller):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/alt_rate.py --scale 10 --trace Q19
    python scripts/alt_rate.py --summarize DIR >> profiles/alt/alt_kernel_trace_sf10.txt
"""
import argparse
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
import pkgload  # noqa: E402
from cond_rate import load_pkg, report, summarize, timed, verdict  # noqa: E402

Y1994, Y1995 = 8766, 9131           # 1994-01-01 and 1995-01-01
Q1_DAY = 10471                      # 1998-09-02
QTY_RANGES = [(100, 1100), (1000, 2000), (2000, 3000)]   # l_quantity is DECIMAL(15, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="generator threads")
    ap.add_argument("--max-groups", type=int, default=1 << 24, help="the hashed call's max_groups")
    ap.add_argument("--parent-pkg", default="", help="the parent commit's built package directory")
    ap.add_argument("--note", default="", help="a line about the run copied into the output")
    ap.add_argument("--trace", metavar="ARM", default="", help="only four calls of this arm: the run to put under "
                    "rocprofv3 --kernel-trace")
    ap.add_argument("--summarize", metavar="DIR", help="print the kernel times of the trace a --trace run left in DIR")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    fl = pkgload.load()
    fd, path = tempfile.mkstemp(suffix=".fls", dir=os.environ.get("TMPDIR", "/tmp"))
    os.close(fd)
    try:
        fl.gen_image("lineitem", a.scale, 0, 0, None, a.threads).write(path)
        conn = fl.Connection([0])
        t = conn.read_fls(path)
        col = {s[0]: c for c, s in enumerate(t.schema())}
        OKEY, PART, QTY, PRICE, DISC, TAX, RFLAG, STATUS, SHIP, INSTRUCT, MODE = (col[n] for n in (
            "l_orderkey", "l_partkey", "l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag",
            "l_linestatus", "l_shipdate", "l_shipinstruct", "l_shipmode"))
        nrows, nrg = t.nrows, t.nrowgroups
        print(f"# lineitem SF{a.scale:g}: {nrows} rows, {nrg} row groups, {os.path.getsize(path) / 1e9:.3f} GB file, 1 GPU, "
              f"{a.reps} repetitions per arm after one warm-up each, arms alternating")
        if a.note:
            print(f"# {a.note}")
        z = [t.zonemap(rg, PART) for rg in range(nrg)]
        plo, phi = min(x[0] for x in z), max(x[1] for x in z)
        keys = np.arange(plo, phi + 1, dtype=np.int64)
        parts = [conn.keyset(keys[keys % 25 == i]) for i in range(3)]
        del keys
        rev = ("sum_expr", [(0, 1, PRICE), (100, -1, DISC)])
        aggs = [rev, ("count",)]
        base = [(INSTRUCT, "=", "DELIVER IN PERSON"), (MODE, "=", "AIR", 1), (MODE, "=", "REG AIR", 1)]
        branches = [[(PART, "in_set", parts[i]), (QTY, ">=", lo), (QTY, "<=", hi)] for i, (lo, hi) in enumerate(QTY_RANGES)]
        closed = [[(QTY, ">=", lo), (QTY, "<=", hi)] for lo, hi in (QTY_RANGES[0], QTY_RANGES[2])]

        def q19x3():
            got = [t.aggregate(aggs, base + b) for b in branches]
            return [sum(g[0] or 0 for g in got), sum(g[1] for g in got)]

        def q19np():
            total = count = 0
            for _rg, _first, _sel, arrs in t.scan_filtered(base, cols=[PART, QTY, PRICE, DISC]):
                part = arrs[PART].view(np.int32)
                qty, price, disc = (arrs[c].view(np.int64) for c in (QTY, PRICE, DISC))
                m = np.zeros(len(part), bool)
                for i, (lo, hi) in enumerate(QTY_RANGES):
                    m |= (part % 25 == i) & (qty >= lo) & (qty <= hi)
                total += int(np.sum(price[m] * (100 - disc[m])))
                count += int(m.sum())
            return [total, count]
        arms = {
            "Q19": lambda: t.aggregate(aggs, base + [fl.AnyOf(*branches)]),
            "Q19x3": q19x3,
            "Q19np": q19np,
            "base": lambda: t.aggregate(aggs, base),
            "closed": lambda: t.aggregate(aggs, base + [fl.AnyOf(*closed)]),
        }
        what = {"Q19": "aggregate([rev, count(*)]) under base AND AnyOf(three branches: a part set and a quantity range each)",
                "Q19x3": "three calls, aggregate([rev, count(*)]) under base AND one branch each, summed",
                "Q19np": "scan_filtered(base) delivering four columns, the three branches in numpy",
                "base": "aggregate([rev, count(*)]) under base alone",
                "closed": "aggregate([rev, count(*)]) under base AND AnyOf(two quantity ranges): ordinary terms only"}
        if a.trace:
            for _ in range(4):
                print(f"# {a.trace}", arms[a.trace](), flush=True)
            t.close()
            conn.close()
            return
        want = {}
        for k, fn in arms.items():                                                # one warm-up each
            want[k] = fn()
            print(f"warm-up {k} done", file=sys.stderr, flush=True)
        if not want["Q19"] == want["Q19x3"] == want["Q19np"]:
            raise SystemExit(f"the arms disagree: {want}")
        assert 0 < want["Q19"][1] < want["closed"][1] < want["base"][1], want
        times = {k: [] for k in arms}
        for _ in range(max(1, a.reps)):
            for k, fn in arms.items():
                s, out = timed(fn)
                assert out == want[k], (k, out, want[k])
                times[k].append(s)
            print(f"repetition {len(times['Q19'])} done", file=sys.stderr, flush=True)
        med, spread = report("one call with alternatives against the calls it replaces", arms, what, times)
        for x, y in (("Q19", "Q19x3"), ("Q19", "Q19np"), ("Q19", "base"), ("closed", "base")):
            verdict(med, spread, x, y)
        batches = (nrg + 7) // 8
        print(f"# per batch ({batches} batches of 8 row groups): {1e6 * (med['closed'] - med['base']) / batches:.2f} us from "
              f"closed - base (one launch), {1e6 * (med['Q19'] - med['base']) / batches:.2f} us from Q19 - base (five "
              "launches: alt_kernel, three key-set probes, the merge; host clock, whole call)")
        print(f"# answers: Q19 = Q19x3 = Q19np = {want['Q19']}; base {want['base']}; closed {want['closed']}")
        for h in parts:
            h.close()
        t.close()
        conn.close()
        if not a.parent_pkg:
            return
        # ---- the calls without alternatives, parent and head alternating in this process
        mods = {"parent": load_pkg(a.parent_pkg, "fls_parent"), "head": fl}
        tabs = {k: m.Connection([0]).read_fls(path) for k, m in mods.items()}
        q6 = [(SHIP, ">=", Y1994), (SHIP, "<", Y1995), (DISC, ">=", 5), (DISC, "<=", 7), (QTY, "<", 2400)]
        q6_aggs = [("sum_product", PRICE, DISC), ("count",)]
        q1_aggs = [("sum", QTY), ("sum", PRICE), rev, ("sum_expr", [(0, 1, PRICE), (100, -1, DISC), (100, 1, TAX)]),
                   ("sum", DISC), ("count",)]
        calls = {
            "Q6": lambda tb: tb.aggregate(q6_aggs, q6),
            "Q1": lambda tb: tb.aggregate_grouped([RFLAG, STATUS], q1_aggs, [(SHIP, "<=", Q1_DAY)]),
            "H": lambda tb: (lambda g: (g.ngroups, int(np.sum(g.count[0]))))(tb.aggregate_hashed([OKEY], [("count",)], a.max_groups)),
        }
        names = [f"{c}.{b}" for c in calls for b in mods]
        want = {}
        for c, fn in calls.items():
            for b in mods:
                want[c, b] = fn(tabs[b])
            assert want[c, "parent"] == want[c, "head"], c
            print(f"warm-up {c} done", file=sys.stderr, flush=True)
        times = {n: [] for n in names}
        for r in range(max(1, a.reps)):
            for c, fn in calls.items():
                for b in (list(mods) if r % 2 == 0 else list(mods)[::-1]):
                    s, out = timed(lambda: fn(tabs[b]))
                    assert out == want[c, b], (c, b)
                    times[f"{c}.{b}"].append(s)
        what = {n: {"Q6": "the Q6 call", "Q1": "Q1 grouped by l_returnflag, l_linestatus",
                    "H": "count(*) GROUP BY l_orderkey, hashed"}[n.split(".")[0]] + ", " + n.split(".")[1] + "'s library"
                for n in names}
        med, spread = report("calls without alternatives, parent and head interleaved", names, what, times)
        for c in calls:
            verdict(med, spread, f"{c}.head", f"{c}.parent", lim=spread[f"{c}.parent"])
        for tb in tabs.values():
            tb.close()
    finally:
        os.unlink(path)


if __name__ == "__main__":
    main()
