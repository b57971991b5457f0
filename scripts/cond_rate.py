#!/usr/bin/env python3
"""Filtered aggregates (agg FILTER (WHERE cond)) against the calls they replace, same
answers, one process.

Workload: lineitem (default SF10) read from a file on one GPU, its compressed
image resident in HBM after the warm-up.  The arms alternate (one warm-up each,
then --reps repetitions; medians and spread, max - min, of the host clock
around the synchronous call).  Everything is fixed before the first run:

  rev = sum_expr(l_extendedprice * (1 - l_discount)); month = l_shipdate in [1995-09-01, 1995-10-01);
  promo = the key set of every third l_partkey (a third of the parts, as PROMO% is about a sixth of p_type)

  Q14   one call:  aggregate([rev FILTER (l_partkey IN promo), rev]) under month
  Q14x2 the parent's way: aggregate([rev]) under month AND l_partkey IN promo, then aggregate([rev]) under month
  Q12   one call:  aggregate([count(*) FILTER (l_orderkey IN high), count(*) FILTER (l_orderkey NOT IN high)])
        under Q12's lineitem terms; high = the l_orderkey values with key % 5 < 2 (two of five priorities)
  Q12g  the key-map way: aggregate_grouped([map(l_orderkey -> 1 if high else 0)], [count(*)]) under the same terms
  Q6    the Q6 call (sum_product(l_extendedprice, l_discount), count(*) under the Q6 terms), no condition
  Q6c1 / Q6c4 / Q6c8: the same call plus 1 / 4 / 8 conditioned counts, each under an ordinary condition
        of its own (l_quantity < 3 * i AND l_discount >= 0.01): prices cond_kernel per condition

Arms that must agree are checked in every repetition.  No ratio is fixed in
advance: an arm counts as faster than another when the medians differ by more
than the larger spread of the two (DESIGN.md section 24's rule).

With --parent-pkg DIR (a built checkout of the parent commit's package directory)
the unconditioned calls -- Q6, Q1 grouped, count(*) GROUP BY l_orderkey hashed --
run on the parent's and this build in one process, alternating per repetition,
and the differences are set against the parent's own spread.

    python scripts/cond_rate.py --scale 10 --reps 5 --parent-pkg ../parent/duckdb-fastlane_amd \\
        > profiles/cond/cond_rate_sf10.txt

Kernel times come from runs of their own under the profiler: --trace ARM makes
only four calls of that arm, and --summarize DIR reads the kernel trace such a
run left (full batches only: the last batch of a call is smaller):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/cond_rate.py --scale 10 --trace Q6c8
    python scripts/cond_rate.py --summarize DIR >> profiles/cond/cond_kernel_trace_sf10.txt
"""
import argparse
import csv
import glob
import importlib.util
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import pkgload  # noqa: E402

D_950901, D_951001 = 9374, 9404     # 1995-09-01 and 1995-10-01 as DATE days
Y1994, Y1995 = 8766, 9131           # 1994-01-01 and 1995-01-01
Q1_DAY = 10471                      # 1998-09-02


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def load_pkg(pkg_dir, name):
    spec = importlib.util.spec_from_file_location(name, Path(pkg_dir) / "__init__.py",
                                                  submodule_search_locations=[str(pkg_dir)])
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def summarize(trace_dir):
    """per kernel: its launches, and the durations of those with the full grid"""
    for f in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)):
        runs = {}
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1]
            runs.setdefault(name, []).append(
                ((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, int(r["Grid_Size_X"]), int(r["Scratch_Size"])))
        print(f"# {os.path.basename(f)}: durations per launch in us, full batches only")
        print("| kernel | launches | full batches | median | min | max | scratch |")
        print("|---|---|---|---|---|---|---|")
        for name, v in sorted(runs.items(), key=lambda kv: -sum(x[0] for x in kv[1])):
            full = max(x[1] for x in v)
            d = [x[0] for x in v if x[1] == full]
            print(f"| {name} | {len(v)} | {len(d)} | {statistics.median(d):.2f} | {min(d):.2f} | {max(d):.2f} | "
                  f"{max(x[2] for x in v)} B |")


def report(title, arms, what, times, extra=None):
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    print(f"## {title}")
    print("| arm | call | median | spread (max - min) | all |")
    print("|---|---|---|---|---|")
    for k in arms:
        print(f"| {k} | {what[k]} | {1e3 * med[k]:.2f} ms | {1e3 * spread[k]:.2f} ms | "
              f"{' '.join(f'{1e3 * x:.2f}' for x in times[k])} |")
    return med, spread


def verdict(med, spread, x, y, lim=None):
    d = med[x] - med[y]
    lim = max(spread[x], spread[y]) if lim is None else lim
    word = "no difference by the rule" if abs(d) <= lim else (f"{x} slower" if d > 0 else f"{x} faster")
    print(f"# {x} - {y} = {1e3 * d:+.2f} ms against a spread of {1e3 * lim:.2f} ms: {word}")


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
        OKEY, PART, QTY, PRICE, DISC, TAX, RFLAG, STATUS, SHIP, COMMIT, RECEIPT, MODE = (col[n] for n in (
            "l_orderkey", "l_partkey", "l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag",
            "l_linestatus", "l_shipdate", "l_commitdate", "l_receiptdate", "l_shipmode"))
        nrows, nrg = t.nrows, t.nrowgroups
        print(f"# lineitem SF{a.scale:g}: {nrows} rows, {nrg} row groups, {os.path.getsize(path) / 1e9:.3f} GB file, 1 GPU, "
              f"{a.reps} repetitions per arm after one warm-up each, arms alternating")
        if a.note:
            print(f"# {a.note}")

        def span(c):
            z = [t.zonemap(rg, c) for rg in range(nrg)]
            return min(x[0] for x in z), max(x[1] for x in z)
        plo, phi = span(PART)
        promo = conn.keyset(np.arange(plo, phi + 1, 3, dtype=np.int64))
        olo, ohi = span(OKEY)
        okeys = np.arange(olo, ohi + 1, dtype=np.int64)
        is_high = okeys % 5 < 2
        high = conn.keyset(okeys[is_high])
        prio = conn.keymap(okeys, is_high.astype(np.uint16))
        del okeys, is_high
        rev = ("sum_expr", [(0, 1, PRICE), (100, -1, DISC)])
        month = [(SHIP, ">=", D_950901), (SHIP, "<", D_951001)]
        q12 = [(COMMIT, "<", fl.Col(RECEIPT)), (SHIP, "<", fl.Col(COMMIT)), (MODE, "=", "MAIL", 1), (MODE, "=", "SHIP", 1),
               (RECEIPT, ">=", Y1994), (RECEIPT, "<", Y1995)]
        q6 = [(SHIP, ">=", Y1994), (SHIP, "<", Y1995), (DISC, ">=", 5), (DISC, "<=", 7), (QTY, "<", 2400)]
        q6_aggs = [("sum_product", PRICE, DISC), ("count",)]

        def q6c(n):
            return q6_aggs + [fl.When(("count",), [(QTY, "<", 300 * (i + 1)), (DISC, ">=", 1)]) for i in range(n)]

        def q14x2():
            return t.aggregate([rev], month + [(PART, "in_set", promo)]) + t.aggregate([rev], month)

        def q12g():
            got = dict(t.aggregate_grouped([("map", OKEY, prio)], [("count",)], q12))
            return [got.get((1,), [0])[0], got.get((0,), [0])[0]]
        arms = {
            "Q14": lambda: t.aggregate([fl.When(rev, [(PART, "in_set", promo)]), rev], month),
            "Q14x2": q14x2,
            "Q12": lambda: t.aggregate([fl.When(("count",), [(OKEY, "in_set", high)]),
                                        fl.When(("count",), [(OKEY, "not_in_set", high)])], q12),
            "Q12g": q12g,
            "Q6": lambda: t.aggregate(q6c(0), q6),
            "Q6c1": lambda: t.aggregate(q6c(1), q6),
            "Q6c4": lambda: t.aggregate(q6c(4), q6),
            "Q6c8": lambda: t.aggregate(q6c(8), q6),
        }
        what = {"Q14": "aggregate([rev FILTER (l_partkey IN promo), rev]) under one month of l_shipdate",
                "Q14x2": "two calls: aggregate([rev]) under the month AND the set term, then under the month",
                "Q12": "aggregate of two conditioned counts (l_orderkey [NOT] IN high) under Q12's terms",
                "Q12g": "aggregate_grouped by the key map l_orderkey -> high / low under Q12's terms",
                "Q6": "the Q6 call, no condition", "Q6c1": "Q6 + 1 conditioned count", "Q6c4": "Q6 + 4 conditioned counts",
                "Q6c8": "Q6 + 8 conditioned counts, a condition each"}
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
        if want["Q14"] != want["Q14x2"] or want["Q12"] != want["Q12g"]:
            raise SystemExit(f"the arms disagree: {want}")
        for k in ("Q6c1", "Q6c4", "Q6c8"):
            assert want[k][:2] == want["Q6"] and all(0 < x <= want["Q6"][1] for x in want[k][2:]), (k, want[k])
        assert want["Q14"][0] and 0 < want["Q14"][0] < want["Q14"][1] and min(want["Q12"]) > 0, want
        times = {k: [] for k in arms}
        for _ in range(max(1, a.reps)):
            for k, fn in arms.items():
                s, out = timed(fn)
                assert out == want[k], (k, out, want[k])
                times[k].append(s)
            print(f"repetition {len(times['Q14'])} done", file=sys.stderr, flush=True)
        med, spread = report("conditioned calls against the calls they replace", arms, what, times)
        for x, y in (("Q14", "Q14x2"), ("Q12", "Q12g"), ("Q6c1", "Q6"), ("Q6c4", "Q6"), ("Q6c8", "Q6")):
            verdict(med, spread, x, y)
        batches = (nrg + 7) // 8
        print(f"# per condition and batch ({batches} batches of 8 row groups): "
              f"{1e6 * (med['Q6c8'] - med['Q6']) / 8 / batches:.2f} us from Q6c8 - Q6, "
              f"{1e6 * (med['Q6c1'] - med['Q6']) / batches:.2f} us from Q6c1 - Q6 (host clock, whole call)")
        print(f"# answers: Q14 = Q14x2 = {want['Q14']}; Q12 = Q12g = {want['Q12']}; Q6 {want['Q6']}; Q6c8 {want['Q6c8']}")
        for h in (promo, high, prio):
            h.close()
        t.close()
        conn.close()
        if not a.parent_pkg:
            return
        # ---- the unconditioned calls, parent and head alternating in this process
        mods = {"parent": load_pkg(a.parent_pkg, "fls_parent"), "head": fl}
        tabs = {k: m.Connection([0]).read_fls(path) for k, m in mods.items()}
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
        med, spread = report("unconditioned calls, parent and head interleaved", names, what, times)
        for c in calls:
            verdict(med, spread, f"{c}.head", f"{c}.parent", lim=spread[f"{c}.parent"])
        for tb in tabs.values():
            tb.close()
    finally:
        os.unlink(path)


if __name__ == "__main__":
    main()
