#!/usr/bin/env python3
"""Aggregate pushdown against the delivering scan, same answers, one process.

Workload: lineitem (default SF10) read from a file on one GPU, its compressed
image resident in HBM after the warm-up.  Two queries, each by two arms that
alternate (one warm-up each, then --reps repetitions, medians of the host
clock around the synchronous call):

  Q6          A: Table.aggregate([sum_product(l_extendedprice, l_discount), count(*)]) under the Q6 terms
              B: scan_filtered(Q6, cols=[l_extendedprice, l_discount]) + a numpy reduction
                 (the only way without the aggregate pushdown)
  unfiltered  A: Table.aggregate([sum(l_quantity), min(l_shipdate), max(l_shipdate), count(*)])
              B: scan(cols=[l_quantity, l_shipdate]) + numpy

  Q1          A: Table.aggregate_grouped by l_returnflag, l_linestatus of TPC-H Q1's sums -- sum(l_quantity),
                 sum(l_extendedprice), sum(l_extendedprice * (1 - l_discount)),
                 sum(l_extendedprice * (1 - l_discount) * (1 + l_tax)) -- with sum(l_discount) and count(*), from
                 which the query's averages follow, under the shipdate term
              B: scan_filtered of the same six columns + a numpy group-by summed in Python integers (the only way
                 without the grouped call)
              C: Table.aggregate of the same aggregates and filter, ungrouped: the floor the grouping is paid on top of

The arms' answers are compared before anything is printed.

    python scripts/agg_rate.py --scale 10 --reps 5 > all.txt        (--query picks one of them)
    python scripts/agg_rate.py --scale 10 --reps 5 --query q1 > profiles/agg/q1_full_sf10.txt
(profiles/agg/group_rate_sf10.txt is the same query with sum(l_extendedprice * l_discount) standing in for the
two products, as the script measured it before the engine had sums of affine factors.)
"""
import argparse
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import pkgload  # noqa: E402

DAY_1994, DAY_1995 = 8766, 9131
C_QTY, C_PRICE, C_DISC, C_SHIPDATE = 4, 5, 6, 10
Q6 = [(C_SHIPDATE, ">=", DAY_1994), (C_SHIPDATE, "<", DAY_1995), (C_DISC, ">=", 5), (C_DISC, "<=", 7),
      (C_QTY, "<", 2400)]


def q6_aggregate(t):
    return t.aggregate([("sum_product", C_PRICE, C_DISC), ("count",)], filt=Q6)


def q6_scan(t):
    total, rows = 0, 0
    for _, _, sel, arrays in t.scan_filtered(Q6, cols=[C_PRICE, C_DISC]):
        price, disc = arrays[C_PRICE].view(np.int64), arrays[C_DISC].view(np.int64)
        total += int(np.dot(price, disc))   # < 2^63 per row group: 65,536 x 1.1e7 x 10
        rows += len(sel)
    return [total if rows else None, rows]


def plain_aggregate(t):
    return t.aggregate([("sum", C_QTY), ("min", C_SHIPDATE), ("max", C_SHIPDATE), ("count",)])


def plain_scan(t):
    total, lo, hi, rows = 0, None, None, 0
    for _, arrays in t.scan(cols=[C_QTY, C_SHIPDATE]):
        qty, ship = arrays[C_QTY].view(np.int64), arrays[C_SHIPDATE].view(np.int32)
        total += int(qty.sum())
        a, b = int(ship.min()), int(ship.max())
        lo, hi = (a if lo is None else min(lo, a)), (b if hi is None else max(hi, b))
        rows += len(qty)
    return [total, lo, hi, rows]


# ---- TPC-H Q1: the grouped call (profiles/agg/q1_full_sf10.txt)
C_TAX, C_RFLAG, C_STATUS = 7, 8, 9
Q1_DAY = 10471                      # 1998-09-02 as DATE days
Q1 = [(C_SHIPDATE, "<=", Q1_DAY)]
Q1_KEYS = [C_RFLAG, C_STATUS]
# DECIMAL(15, 2) columns: 1 is 100 in their unit; sum_disc_price has scale 4, sum_charge scale 6
Q1_AGGS = [("sum", C_QTY), ("sum", C_PRICE), ("sum_expr", [(0, 1, C_PRICE), (100, -1, C_DISC)]),
           ("sum_expr", [(0, 1, C_PRICE), (100, -1, C_DISC), (100, 1, C_TAX)]), ("sum", C_DISC), ("count",)]


Q1_COLS = [C_QTY, C_PRICE, C_DISC, C_TAX, C_RFLAG, C_STATUS]


def q1_grouped(t):
    return [(list(k), v) for k, v in t.aggregate_grouped(Q1_KEYS, Q1_AGGS, filt=Q1)]


def q1_ungrouped(t):
    return t.aggregate(Q1_AGGS, filt=Q1)


def _short_strings(rec):
    """string_t records of strings of at most 8 bytes -> (lengths, their bytes as one uint64 each)"""
    rec = rec.reshape(-1, 16)
    lens = rec[:, :4].copy().view(np.uint32).reshape(-1)
    assert len(lens) == 0 or int(lens.max()) <= 8
    return lens, rec[:, 4:12].copy().view(np.uint64).reshape(-1)


def q1_scan(t):
    """the qualifying rows of the six columns over the link, grouped with numpy;
    groups in order of their first row, as the grouped call returns them"""
    groups = {}
    for _, _, sel, arrays in t.scan_filtered(Q1, cols=Q1_COLS):
        if len(sel) == 0:
            continue
        qty, price, disc, tax = (arrays[c].view(np.int64) for c in (C_QTY, C_PRICE, C_DISC, C_TAX))
        (la, ka), (lb, kb) = _short_strings(arrays[C_RFLAG]), _short_strings(arrays[C_STATUS])
        if int(la.max()) <= 4 and int(lb.max()) <= 4:   # both keys in one word: one sort
            combo, first, inv = np.unique(ka | (kb << np.uint64(32)), return_index=True, return_inverse=True)
        else:
            ua, ia = np.unique(ka, return_inverse=True)
            ub, ib = np.unique(kb, return_inverse=True)
            combo, first, inv = np.unique(ia * len(ub) + ib, return_index=True, return_inverse=True)
        disc_price = price * (100 - disc)    # < 2^63 per row group: 65,536 x 1.1e7 x 100
        charge = disc_price * (100 + tax)    # ... x 108 = 7.8e15
        for g in np.argsort(first):
            m = inv == g
            r = int(first[g])
            key = (bytes(ka[r:r + 1].view(np.uint8)[:la[r]]), bytes(kb[r:r + 1].view(np.uint8)[:lb[r]]))
            acc = groups.setdefault(key, [0, 0, 0, 0, 0, 0])
            for i, x in enumerate((qty, price, disc_price, charge, disc)):
                acc[i] += int(x[m].sum())    # the row group's sum in int64, the table's in Python integers
            acc[5] += int(m.sum())
    return [(list(k), v) for k, v in groups.items()]


def q1_arm(fl, t, nrows, reps):
    arms = (("A Table.aggregate_grouped      ", q1_grouped), ("B scan_filtered + numpy group", q1_scan),
            ("C Table.aggregate (ungrouped)  ", q1_ungrouped))
    want = [fn(t) for _, fn in arms]         # warm-up: the image becomes resident, buffers are allocated
    if want[0] != want[1]:
        raise SystemExit(f"Q1: the arms disagree: grouped {want[0]}, scan {want[1]}")
    if [sum(v[i] for _, v in want[0]) for i in range(len(Q1_AGGS))] != want[2]:
        raise SystemExit(f"Q1: the groups do not add up to the ungrouped call: {want[0]}, {want[2]}")
    times = [[] for _ in arms]
    for _ in range(max(1, reps)):
        for k, (_, fn) in enumerate(arms):
            s, out = timed(fn, t)
            assert out == want[k], (k, out, want[k])
            times[k].append(s)
    med = [statistics.median(x) for x in times]
    bytes_res, _ = fl.Connection.resident_info(0)
    print("Q1: group by l_returnflag, l_linestatus of sum(l_quantity), sum(l_extendedprice), "
          "sum(l_extendedprice * (1 - l_discount)), sum(l_extendedprice * (1 - l_discount) * (1 + l_tax)), "
          "sum(l_discount), count(*) where l_shipdate <= 1998-09-02")
    for k, v in want[0]:
        print(f"Q1: group {[x.decode() for x in k]}: {v}")
    for (name, _), m, x in zip(arms, med, times):
        print(f"Q1: {name} median {1e3 * m:9.3f} ms  ({nrows / m:.3e} rows/s)  all {' '.join(f'{1e3 * y:.3f}' for y in x)}")
    print(f"Q1: B / A = {med[1] / med[0]:.2f}   A / C = {med[0] / med[2]:.2f}  (resident image {bytes_res / 1e9:.3f} GB)")
    for (name, _), x in zip(arms, times):
        print(f"Q1: {name} spread: min {1e3 * min(x):.3f} ms, max {1e3 * max(x):.3f} ms over {len(x)} repetitions")
    # where B's time goes: its scan alone, the rows delivered and dropped
    alone = []
    for _ in range(max(1, reps)):
        t0 = time.perf_counter()
        rows = sum(len(sel) for _, _, sel, _ in t.scan_filtered(Q1, cols=Q1_COLS))
        alone.append(time.perf_counter() - t0)
    m = statistics.median(alone)
    print(f"Q1: (B's scan_filtered alone, {rows} rows delivered, no grouping: median {1e3 * m:9.3f} ms; "
          f"the rest of B is numpy)")


def timed(fn, t):
    t0 = time.perf_counter()
    out = fn(t)
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="generator threads")
    ap.add_argument("--query", choices=["all", "q1", "q6", "unfiltered"], default="all")
    a = ap.parse_args()
    fl = pkgload.load()
    fd, path = tempfile.mkstemp(suffix=".fls", dir=os.environ.get("TMPDIR", "/tmp"))
    os.close(fd)
    try:
        fl.gen_image("lineitem", a.scale, 0, 0, None, a.threads).write(path)
        conn = fl.Connection([0])
        t = conn.read_fls(path)
        nrows = t.nrows
        print(f"# lineitem SF{a.scale:g}: {nrows} rows, {t.nrowgroups} row groups, {os.path.getsize(path) / 1e9:.3f} GB file, "
              f"1 GPU, {a.reps} repetitions per arm after one warm-up each, arms alternating")
        if a.query in ("all", "q1"):
            q1_arm(fl, t, nrows, a.reps)
        for name, agg, scan in (("Q6", q6_aggregate, q6_scan), ("unfiltered", plain_aggregate, plain_scan)):
            if a.query not in ("all", name.lower()):
                continue
            ra, rb = agg(t), scan(t)          # warm-up: the image becomes resident, buffers are allocated
            if ra != rb:
                raise SystemExit(f"{name}: the arms disagree: aggregate {ra}, scan {rb}")
            ta, tb = [], []
            for _ in range(max(1, a.reps)):
                s, out = timed(agg, t)
                assert out == ra, (name, out, ra)
                ta.append(s)
                s, out = timed(scan, t)
                assert out == rb, (name, out, rb)
                tb.append(s)
            ma, mb = statistics.median(ta), statistics.median(tb)
            bytes_res, _ = fl.Connection.resident_info(0)
            print(f"{name}: answer {ra}")
            print(f"{name}: A Table.aggregate        median {1e3 * ma:9.3f} ms  ({nrows / ma:.3e} rows/s)  "
                  f"all {' '.join(f'{1e3 * x:.3f}' for x in ta)}")
            print(f"{name}: B scan + numpy reduction median {1e3 * mb:9.3f} ms  ({nrows / mb:.3e} rows/s)  "
                  f"all {' '.join(f'{1e3 * x:.3f}' for x in tb)}")
            print(f"{name}: B / A = {mb / ma:.2f}  (resident image {bytes_res / 1e9:.3f} GB)")
        t.close()
        conn.close()
    finally:
        os.unlink(path)


if __name__ == "__main__":
    main()
