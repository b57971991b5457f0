#!/usr/bin/env python3
"""Column-to-column filter terms (`a < b` pushdown) against the alternatives, same answers, one process.

Workload: lineitem (default SF10) read from a file on one GPU, its compressed
image resident in HBM after the warm-up.  The arms alternate (one warm-up each,
then --reps repetitions; medians and spread, max - min, of the host clock
around the synchronous call).  The filters are fixed before the first run:

  Q12: l_commitdate < l_receiptdate AND l_shipdate < l_commitdate AND l_shipmode IN ('MAIL', 'SHIP')
       AND l_receiptdate >= 1994-01-01 AND l_receiptdate < 1995-01-01   (the real Q12 lineitem predicate)

  A:  Table.aggregate([count(*), sum(l_extendedprice)]) under Q12 -- the pushed-down call
  Ag: Table.aggregate_grouped([l_shipmode], the same aggregates) under Q12 without its l_shipmode term (a
      VARCHAR key is grouped by dictionary code and cannot also be read by a filter term): all seven
      modes come back and the MAIL and SHIP groups are Q12's answer
  C / Cg: the same two calls without the two column terms; A - C prices the feature
  B:  the only route without column terms: scan_filtered under the remaining terms delivering the three
      date columns and the price, then the two comparisons and the reduction in numpy
  D:  l_commitdate < l_receiptdate alone under aggregate_hashed([l_orderkey], [count(*)]): the Q4 / Q21 shape
  D0: the same hashed call with no filter

A and B must return equal values in every repetition; Ag's MAIL and SHIP groups must add
up to A.  No ratio is fixed in advance: an arm counts as faster than another when
the medians differ by more than the larger spread of the two (DESIGN.md
section 24's rule); the script prints the verdicts by that rule.

    python scripts/colcmp_rate.py --scale 10 --reps 5 > profiles/colcmp/colcmp_rate_sf10.txt

Kernel times come from a run of their own under the profiler: --trace makes
only four calls of arm A and then four of aggregate under l_commitdate <
l_receiptdate alone, and --summarize DIR reads the kernel trace that run left
(the first half of a kernel's launches belong to Q12, the second half to the
single term; the last batch of a call is smaller and is left out):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/colcmp_rate.py --scale 10 --trace
    python scripts/colcmp_rate.py --summarize DIR > profiles/colcmp/colcmp_kernel_trace_sf10.txt
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import pkgload  # noqa: E402

Y1994, Y1995 = 8766, 9131           # 1994-01-01 and 1995-01-01 as DATE days


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def summarize(trace_dir):
    """per kernel: all launches, then the full batches of each half of the run"""
    for f in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)):
        runs = {}
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1]
            runs.setdefault(name, []).append(
                ((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, int(r["Grid_Size_X"]), int(r["Scratch_Size"])))
        print(f"# {os.path.basename(f)}: durations per launch in us; Q12 = the first half of a kernel's launches (four calls "
              f"of arm A), one term = the second half (l_commitdate < l_receiptdate alone); full batches only in the halves")
        print("| kernel | launches | median | min | max | Q12 full batches | Q12 median | min | max | one term median | min | max | "
              "scratch |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        for name, v in sorted(runs.items(), key=lambda kv: -sum(x[0] for x in kv[1])):
            d = [x[0] for x in v]
            row = f"| {name} | {len(d)} | {statistics.median(d):.2f} | {min(d):.2f} | {max(d):.2f} |"
            full_grid, half = max(x[1] for x in v), len(v) // 2
            parts = [[x[0] for x in part if x[1] == full_grid] for part in (v[:half], v[half:])]
            if "_kernel" in name and all(parts):
                row += f" {len(parts[0])} |" + "".join(f" {statistics.median(q):.2f} | {min(q):.2f} | {max(q):.2f} |" for q in parts)
            else:
                row += " - | - | - | - | - | - | - |"
            print(row + f" {max(x[2] for x in v)} B |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="generator threads")
    ap.add_argument("--max-groups", type=int, default=1 << 24, help="arm D's max_groups")
    ap.add_argument("--note", default="", help="a line about the run (the machine lease) copied into the output")
    ap.add_argument("--trace", action="store_true", help="only four calls of arm A, then four of aggregate under "
                    "l_commitdate < l_receiptdate alone: the run to put under rocprofv3 --kernel-trace")
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
        sch = t.schema()
        col = {s[0]: c for c, s in enumerate(sch)}
        OKEY, PRICE, SHIP, COMMIT, RECEIPT, MODE = (col[n] for n in ("l_orderkey", "l_extendedprice", "l_shipdate",
                                                                     "l_commitdate", "l_receiptdate", "l_shipmode"))
        nrows = t.nrows
        aggs = [("count",), ("sum", PRICE)]
        rest = [(MODE, "=", "MAIL", 1), (MODE, "=", "SHIP", 1), (RECEIPT, ">=", Y1994), (RECEIPT, "<", Y1995)]
        cterms = [(COMMIT, "<", fl.Col(RECEIPT)), (SHIP, "<", fl.Col(COMMIT))]
        q12 = cterms + rest
        year = rest[2:]                                                           # the grouped arms: no l_shipmode term
        q4 = [(COMMIT, "<", fl.Col(RECEIPT))]
        print(f"# lineitem SF{a.scale:g}: {nrows} rows, {t.nrowgroups} row groups, {os.path.getsize(path) / 1e9:.3f} GB "
              f"file, 1 GPU, {a.reps} repetitions per arm after one warm-up each, arms alternating; "
              f"count(*), sum(l_extendedprice)")
        if a.note:
            print(f"# {a.note}")
        if a.trace:
            for _ in range(4):
                print("# Q12", t.aggregate(aggs, filt=q12), flush=True)
            for _ in range(4):
                print("# one term", t.aggregate(aggs, filt=q4), flush=True)
            t.close()
            conn.close()
            return

        def arm_b():
            rows = total = 0
            dt = fl.NP_DTYPE[sch[SHIP][1]]
            for _, _, sel, arrays in t.scan_filtered(rest, cols=[SHIP, COMMIT, RECEIPT, PRICE]):
                s, c, r = (arrays[x].view(dt) for x in (SHIP, COMMIT, RECEIPT))
                m = (c < r) & (s < c)
                rows += int(m.sum())
                total += int(arrays[PRICE].view(fl.NP_DTYPE[sch[PRICE][1]])[m].sum())
            return [rows, total if rows else None]

        arms = {
            "A": lambda: t.aggregate(aggs, filt=q12),
            "C": lambda: t.aggregate(aggs, filt=rest),
            "Ag": lambda: t.aggregate_grouped([MODE], aggs, filt=cterms + year),
            "Cg": lambda: t.aggregate_grouped([MODE], aggs, filt=year),
            "B": arm_b,
            "D": lambda: t.aggregate_hashed([OKEY], [("count",)], a.max_groups, filt=q4),
            "D0": lambda: t.aggregate_hashed([OKEY], [("count",)], a.max_groups),
        }
        want, pruned = {}, {}
        for k, fn in arms.items():                                                # one warm-up each
            want[k] = fn()
            pruned[k] = t.pruned
            print(f"warm-up {k} done", file=sys.stderr, flush=True)
        for k in ("D", "D0"):
            want[k] = (want[k].ngroups, int(np.sum(want[k].count[0])))
        if want["A"] != want["B"]:
            raise SystemExit(f"the arms disagree: pushed down {want['A']}, host {want['B']}")
        q12_groups = [v for (mode,), v in want["Ag"] if mode in (b"MAIL", b"SHIP")]
        assert [sum(v[0] for v in q12_groups), sum(v[1] for v in q12_groups)] == want["A"], want["Ag"]
        times = {k: [] for k in arms}
        for _ in range(max(1, a.reps)):
            for k, fn in arms.items():
                s, out = timed(fn)
                if k in ("D", "D0"):
                    out = (out.ngroups, int(np.sum(out.count[0])))
                assert out == want[k], (k, out, want[k])
                times[k].append(s)
            print(f"repetition {len(times['A'])} done", file=sys.stderr, flush=True)
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = {k: max(v) - min(v) for k, v in times.items()}
        sel = {"A": want["A"][0], "C": want["C"][0], "Ag": sum(v[0] for _, v in want["Ag"]),
               "Cg": sum(v[0] for _, v in want["Cg"]), "B": want["B"][0],
               "D": want["D"][1], "D0": want["D0"][1]}
        what = {"A": "aggregate under Q12 (two column terms)", "C": "aggregate, Q12 without the column terms",
                "Ag": "aggregate_grouped by l_shipmode under Q12 less its l_shipmode term",
                "Cg": "aggregate_grouped, without the column terms",
                "B": "scan_filtered of 3 dates + price under the remaining terms, numpy compare and sum",
                "D": "aggregate_hashed by l_orderkey under l_commitdate < l_receiptdate", "D0": "aggregate_hashed, no filter"}
        print("| arm | call | rows selected | selectivity | median | spread (max - min) | all | row groups pruned |")
        print("|---|---|---|---|---|---|---|---|")
        for k in arms:
            print(f"| {k} | {what[k]} | {sel[k]} | {sel[k] / nrows:.4f} | {1e3 * med[k]:.2f} ms | {1e3 * spread[k]:.2f} ms | "
                  f"{' '.join(f'{1e3 * x:.2f}' for x in times[k])} | {pruned[k]} |")

        def verdict(x, y):
            d, lim = med[x] - med[y], max(spread[x], spread[y])
            word = "no difference by the rule" if abs(d) <= lim else (f"{x} slower" if d > 0 else f"{x} faster")
            return f"# {x} - {y} = {1e3 * d:+.2f} ms against a larger spread of {1e3 * lim:.2f} ms: {word}"
        for x, y in (("A", "C"), ("Ag", "Cg"), ("A", "B"), ("D", "D0")):
            print(verdict(x, y))
        print(f"# answers: A = B = {want['A']}; C {want['C']}; Ag {want['Ag']}; D {want['D'][0]} groups over "
              f"{want['D'][1]} rows; D0 {want['D0'][0]} groups over {want['D0'][1]} rows")
        bytes_res, _ = fl.Connection.resident_info(0)
        print(f"# resident image {bytes_res / 1e9:.3f} GB; A and B returned equal values in every repetition")
        t.close()
        conn.close()
    finally:
        os.unlink(path)


if __name__ == "__main__":
    main()
