#!/usr/bin/env python3
"""Top-N pushdown against the delivering scan, same answers, one process.

Workload: lineitem (default SF10) read from a file on one GPU, its compressed
image resident in HBM after the warm-up.  Per query three arms alternate (one
warm-up each, then --reps repetitions, medians of the host clock around the
synchronous call):

  A: Table.topn(key, k, cols=DELIVER, filt, desc) -- phase 1 (selection in HBM) and phase 2 (late
     materialisation of the winners' row groups) also timed separately inside the call, on the host clock
  B: scan_filtered (or scan) of the key and the delivered columns + numpy argpartition and sort per row group,
     then over the row groups' candidates (the only way to the same answer without the pushdown)
  C: Table.aggregate of max(key) (min for an ascending key) under the same filter: the same decode and
     filter with the cheapest reduction, the floor phase 1 can approach

Queries: l_extendedprice DESC for k in {10, 100, 1024}, unfiltered and under the Q6 terms, delivering
l_orderkey, l_extendedprice, l_shipdate, l_shipmode; l_orderkey ASC, k = 10, unfiltered (the zone maps prune all
but one row group).  A and B must return identical rows and values in every repetition.

    python scripts/topn_rate.py --scale 10 --reps 5 > profiles/topn/topn_rate_sf10.txt
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
C_OKEY, C_QTY, C_PRICE, C_DISC, C_SHIPDATE, C_MODE = 0, 4, 5, 6, 10, 14
Q6 = [(C_SHIPDATE, ">=", DAY_1994), (C_SHIPDATE, "<", DAY_1995), (C_DISC, ">=", 5), (C_DISC, "<=", 7),
      (C_QTY, "<", 2400)]
DELIVER = [C_OKEY, C_PRICE, C_SHIPDATE, C_MODE]


def best_k(keys, rows, k, desc):
    """positions of the k best of one batch of (key, global row) pairs by (key, row): an argpartition finds the
    k-th key, every row up to and including its ties is sorted"""
    order = -keys if desc else keys       # (DECIMAL(15, 2) prices and order keys: the negation cannot overflow)
    if len(order) > k:
        part = np.argpartition(order, k - 1)[:k]
        cand = np.nonzero(order <= order[part].max())[0]
    else:
        cand = np.arange(len(order))
    return cand[np.lexsort((rows[cand], order[cand]))[:k]]


def topn_scan(fl, t, key, k, filt, desc):
    """arm B: (rows, {column: values}) of the k best rows, through a scan of the key and the delivered columns"""
    sch = t.schema()
    cols = sorted(set(DELIVER + [key]))
    if filt:
        parts = ((first, sel, arrays) for _, first, sel, arrays in t.scan_filtered(filt, cols=cols))
    else:
        parts = ((first, None, arrays) for first, arrays in t.scan(cols=cols))
    keep_rows, keep = [], {c: [] for c in cols}
    for first, sel, arrays in parts:
        keys = arrays[key].view(fl.NP_DTYPE[sch[key][1]])
        if len(keys) == 0:
            continue
        rows = np.uint64(first) + (np.arange(len(keys), dtype=np.uint64) if sel is None else sel.astype(np.uint64))
        at = best_k(keys, rows, k, desc)
        keep_rows.append(rows[at])
        for c in cols:
            ob = sch[c][4]
            keep[c].append(arrays[c].reshape(-1, ob)[at].copy())
    if not keep_rows:
        return np.zeros(0, np.uint64), {c: [] for c in DELIVER}
    rows = np.concatenate(keep_rows)
    vals = {c: np.concatenate(keep[c]) for c in cols}
    at = best_k(vals[key].reshape(-1).view(fl.NP_DTYPE[sch[key][1]]), rows, k, desc)
    out = {}
    for c in DELIVER:
        raw = vals[c][at].reshape(-1)
        out[c] = fl.string_t_decode(raw) if sch[c][1] in fl.STRING_TYPES else raw.view(fl.NP_DTYPE[sch[c][1]])
    return rows[at], out


def topn_call(t, key, k, filt, desc):
    """arm A: the same shape as arm B's answer, and the call's phase times"""
    rows, values, valid = t.topn(key, k, cols=DELIVER, filt=filt, desc=desc)
    assert all(valid[c] is None for c in DELIVER)
    return rows, {c: values[c] for c in DELIVER}


def same(a, b):
    if not np.array_equal(a[0], b[0]):
        return False
    for c in DELIVER:
        x, y = a[1][c], b[1][c]
        if (x != y) if isinstance(x, list) else not np.array_equal(x, y):
            return False
    return True


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="generator threads")
    ap.add_argument("--note", default="", help="a line about the run (the machine lease) copied into the output")
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
              f"1 GPU, {a.reps} repetitions per arm after one warm-up each, arms alternating; delivered columns "
              f"l_orderkey, l_extendedprice, l_shipdate, l_shipmode")
        if a.note:
            print(f"# {a.note}")
        queries = [("l_extendedprice DESC", C_PRICE, True, k, name, filt)
                   for name, filt in (("unfiltered", None), ("Q6", Q6)) for k in (10, 100, 1024)]
        queries.append(("l_orderkey ASC", C_OKEY, False, 10, "unfiltered", None))
        print("| query | k | filter | A topn | A phase 1 | A phase 2 | B scan + numpy | C aggregate | B / A | A / C | "
              "row groups pruned |")
        print("|---|---|---|---|---|---|---|---|---|---|---|")
        detail = []
        for text, key, desc, k, fname, filt in queries:
            arm_a = lambda: topn_call(t, key, k, filt, desc)                      # noqa: E731
            arm_b = lambda: topn_scan(fl, t, key, k, filt, desc)                  # noqa: E731
            arm_c = lambda: t.aggregate([("max" if desc else "min", key)], filt=filt)   # noqa: E731
            want_a, want_b, want_c = arm_a(), arm_b(), arm_c()    # warm-up: the image becomes resident
            if not same(want_a, want_b):
                raise SystemExit(f"{text} k={k} {fname}: the arms disagree: topn rows {want_a[0][:5]}, scan rows "
                                 f"{want_b[0][:5]}")
            if len(want_a[0]) and int(want_a[1][key][0]) != want_c[0]:
                raise SystemExit(f"{text} k={k} {fname}: the best key {want_a[1][key][0]} is not the aggregate's {want_c[0]}")
            ta, tb, tc, p1, p2 = [], [], [], [], []
            for _ in range(max(1, a.reps)):
                s, out = timed(arm_a)
                assert same(out, want_b), (text, k, fname)
                ta.append(s)
                p1.append(t.topn_ms[0])
                p2.append(t.topn_ms[1])
                pruned = t.pruned
                s, out = timed(arm_b)
                assert same(out, want_a), (text, k, fname)
                tb.append(s)
                s, out = timed(arm_c)
                assert out == want_c, (text, k, fname)
                tc.append(s)
            ma, mb, mc = (statistics.median(x) for x in (ta, tb, tc))
            print(f"| {text} | {k} | {fname} | {1e3 * ma:.2f} ms | {statistics.median(p1):.2f} ms | "
                  f"{statistics.median(p2):.2f} ms | {1e3 * mb:.1f} ms | {1e3 * mc:.2f} ms | {mb / ma:.1f} | "
                  f"{ma / mc:.2f} | {pruned} |")
            detail.append(f"# {text} k={k} {fname}: {len(want_a[0])} rows returned, first row {int(want_a[0][0])}, "
                          f"best key {int(want_a[1][key][0])}; A all {' '.join(f'{1e3 * x:.2f}' for x in ta)} ms; "
                          f"B all {' '.join(f'{1e3 * x:.1f}' for x in tb)} ms; C all {' '.join(f'{1e3 * x:.2f}' for x in tc)} ms")
        print("\n".join(detail))
        bytes_res, _ = fl.Connection.resident_info(0)
        print(f"# resident image {bytes_res / 1e9:.3f} GB; A and B returned identical rows and values in every repetition")
        t.close()
        conn.close()
    finally:
        os.unlink(path)


if __name__ == "__main__":
    main()
