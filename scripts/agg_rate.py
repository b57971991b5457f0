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

The arms' answers are compared before anything is printed.

    python scripts/agg_rate.py --scale 10 --reps 5 > profiles/agg/agg_rate_sf10.txt
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


def timed(fn, t):
    t0 = time.perf_counter()
    out = fn(t)
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="generator threads")
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
        for name, agg, scan in (("Q6", q6_aggregate, q6_scan), ("unfiltered", plain_aggregate, plain_scan)):
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
