#!/usr/bin/env python3
"""Hash aggregate pushdown against the delivering scan, same answers, one process.

Workload: lineitem (default SF10) read from a file on one GPU, its compressed
image resident in HBM after the warm-up.  Three queries; the arms of each
alternate (one warm-up each, then --reps repetitions, medians of the host clock
around the synchronous call):

  (a) orderkey    GROUP BY l_orderkey of sum(l_quantity), count(*): about 1.5 M x SF groups
                  A1: Table.aggregate_hashed, runs of equal keys combined on chip (the default)
                  A0: the same with FLS_HASHAGG_COMBINE=0: one set of atomics per row
                  B:  scan of [l_orderkey, l_quantity] + np.unique / np.bincount (the only way without the call)
  (b) q3          the Q3 shape: l_orderkey IN a key set of a fifth of the orders, l_shipdate > 1995-03-15,
                  GROUP BY l_orderkey of sum(l_extendedprice * (1 - l_discount))
                  A1 / A0 as above; B: scan_filtered of [l_orderkey, l_extendedprice, l_discount] + numpy
  (c) linenumber  GROUP BY l_linenumber (7 groups) of sum(l_quantity), count(*): what the atomics cost where
                  the grouped call applies
                  A1 / A0 as above; G: Table.aggregate_grouped; B: scan + numpy

A's time is the Python call, which ends with the result's arrays copied into
numpy; to_list is not called.  The phases the library times itself (the scan,
extraction + D2H, merge + unpacking) and the table's bytes are printed per
arm.  The arms' answers are compared before anything is printed.

    python scripts/hashagg_rate.py --scale 10 --reps 5 > profiles/hashagg/hashagg_rate_sf10.txt
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

C_OKEY, C_LINE, C_QTY, C_PRICE, C_DISC, C_SHIPDATE = 0, 3, 4, 5, 6, 10
DAY_Q3 = 9204                        # 1995-03-15 as DATE days
REVENUE = ("sum_expr", [(0, 1, C_PRICE), (100, -1, C_DISC)])    # scale 4


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def canon_hashed(h, nsum):
    """(keys ascending, [aggregate arrays in that order]); sums as int64 (asserted to fit)"""
    keys = h.key_values[0].view(np.int64)
    o = np.argsort(keys, kind="stable")
    out = []
    for a in range(len(h.count)):
        if a < nsum:
            lo = h.lo[a].view(np.int64)
            assert np.array_equal(h.hi[a], (lo >> 63).view(np.uint64)), "a sum does not fit 64 bits"
            out.append(lo[o])
        else:
            out.append(h.count[a].view(np.int64)[o])
    return keys[o], out


def numpy_groups(keys, sums, count):
    """np.unique + np.bincount over delivered columns: (keys ascending, [sums..., count])"""
    uniq, inv = np.unique(keys, return_inverse=True)
    out = []
    for x in sums:
        assert len(x) == 0 or float(np.abs(x).max()) * len(x) < 2.0 ** 53     # bincount adds in binary64: exact
        out.append(np.bincount(inv, weights=x, minlength=len(uniq)).astype(np.int64))
    if count:
        out.append(np.bincount(inv, minlength=len(uniq)).astype(np.int64))
    return uniq, out


def same(a, b):
    return np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def run_query(name, title, nrows, reps, arms, canon):
    """arms: [(label, fn)], fn() -> result; canon(label, result) -> comparable"""
    want = [canon(label, fn()) for label, fn in arms]       # warm-up: the image becomes resident, buffers are allocated
    for (label, _), w in zip(arms[1:], want[1:]):
        if not same(want[0], w):
            raise SystemExit(f"{name}: arm {label!r} disagrees with arm {arms[0][0]!r}")
    times = [[] for _ in arms]
    last = [None] * len(arms)
    for _ in range(max(1, reps)):
        for k, (label, fn) in enumerate(arms):
            s, out = timed(fn)
            times[k].append(s)
            last[k] = out
    for (label, _), out, w in zip(arms, last, want):
        assert same(canon(label, out), w), (name, label)
    med = [statistics.median(x) for x in times]
    print(f"{name}: {title}")
    print(f"{name}: {len(want[0][0])} groups; every arm returned the same keys and values")
    for (label, _), m, x, out in zip(arms, med, times, last):
        print(f"{name}: {label:<40s} median {1e3 * m:10.3f} ms  ({nrows / m:.3e} rows/s)  "
              f"all {' '.join(f'{1e3 * y:.3f}' for y in x)}")
        if hasattr(out, "table_bytes"):
            print(f"{name}:   last repetition inside the call: scan {out.scan_ms:.3f} ms, extraction + D2H "
                  f"{out.extract_ms:.3f} ms, merge + unpacking {out.merge_ms:.3f} ms; table {out.table_bytes / 1e6:.1f} MB")
    return dict(zip((label for label, _ in arms), med))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="generator threads")
    ap.add_argument("--query", choices=["all", "orderkey", "q3", "linenumber"], default="all")
    a = ap.parse_args()
    fl = pkgload.load()
    if fl.device_count() < 1:
        raise SystemExit("hashagg_rate.py measures on a GPU and found none")
    fd, path = tempfile.mkstemp(suffix=".fls", dir=os.environ.get("TMPDIR", "/tmp"))
    os.close(fd)

    def combine(on):
        os.environ["FLS_HASHAGG_COMBINE"] = "1" if on else "0"

    try:
        fl.gen_image("lineitem", a.scale, 0, 0, None, a.threads).write(path)
        conn = fl.Connection([0])
        t = conn.read_fls(path)
        nrows = t.nrows
        print(f"# lineitem SF{a.scale:g}: {nrows} rows, {t.nrowgroups} row groups, {os.path.getsize(path) / 1e9:.3f} GB "
              f"file, 1 GPU, {a.reps} repetitions per arm after one warm-up each, arms alternating")

        def hashed(keys, aggs, max_groups, filt, on):
            def fn():
                combine(on)
                return t.aggregate_hashed(keys, aggs, max_groups, filt=filt)
            return fn

        def hcanon(nsum):
            return lambda label, out: canon_hashed(out, nsum) if hasattr(out, "table_bytes") else out

        if a.query in ("all", "orderkey"):
            def scan_okey():
                ks, qs = [], []
                for _, arrays in t.scan(cols=[C_OKEY, C_QTY]):
                    ks.append(arrays[C_OKEY].view(np.int64))
                    qs.append(arrays[C_QTY].view(np.int64))
                return numpy_groups(np.concatenate(ks), [np.concatenate(qs)], True)
            ngroups = len(scan_okey()[0])
            aggs = [("sum", C_QTY), ("count",)]
            run_query("orderkey", "group by l_orderkey of sum(l_quantity), count(*)", nrows, a.reps,
                      [("A1 aggregate_hashed, runs combined", hashed([C_OKEY], aggs, ngroups, None, True)),
                       ("A0 aggregate_hashed, one set per row", hashed([C_OKEY], aggs, ngroups, None, False)),
                       ("B  scan + np.unique / np.bincount", scan_okey)], hcanon(1))
        if a.query in ("all", "q3"):
            top = int(t.zonemap(t.nrowgroups - 1, C_OKEY)[1])
            ks = conn.keyset(np.arange(5, top + 1, 5, dtype=np.int64), signed=True)      # a fifth of the order keys
            filt = [(C_OKEY, "in_set", ks), (C_SHIPDATE, ">", DAY_Q3)]

            def scan_q3():
                kk, rr = [], []
                for _, _, sel, arrays in t.scan_filtered(filt, cols=[C_OKEY, C_PRICE, C_DISC]):
                    kk.append(arrays[C_OKEY].view(np.int64))
                    rr.append(arrays[C_PRICE].view(np.int64) * (100 - arrays[C_DISC].view(np.int64)))
                return numpy_groups(np.concatenate(kk), [np.concatenate(rr)], False)
            ngroups = max(1, len(scan_q3()[0]))
            run_query("q3", "group by l_orderkey of sum(l_extendedprice * (1 - l_discount)) where l_orderkey in "
                      f"a key set of {ks.info.count} keys and l_shipdate > 1995-03-15", nrows, a.reps,
                      [("A1 aggregate_hashed, runs combined", hashed([C_OKEY], [REVENUE], ngroups, filt, True)),
                       ("A0 aggregate_hashed, one set per row", hashed([C_OKEY], [REVENUE], ngroups, filt, False)),
                       ("B  scan_filtered + numpy", scan_q3)], hcanon(1))
            ks.close()
        if a.query in ("all", "linenumber"):
            aggs = [("sum", C_QTY), ("count",)]

            def scan_line():
                ks, qs = [], []
                for _, arrays in t.scan(cols=[C_LINE, C_QTY]):
                    ks.append(arrays[C_LINE].view(np.int32))
                    qs.append(arrays[C_QTY].view(np.int64))
                keys, out = numpy_groups(np.concatenate(ks), [np.concatenate(qs)], True)
                return keys.astype(np.int64), out

            def grouped():
                got = sorted(t.aggregate_grouped([C_LINE], aggs))
                return (np.array([k[0] for k, _ in got], np.int64),
                        [np.array([v[i] for _, v in got], np.int64) for i in range(2)])
            run_query("linenumber", "group by l_linenumber of sum(l_quantity), count(*)", nrows, a.reps,
                      [("A1 aggregate_hashed, runs combined", hashed([C_LINE], aggs, 16, None, True)),
                       ("A0 aggregate_hashed, one set per row", hashed([C_LINE], aggs, 16, None, False)),
                       ("G  aggregate_grouped", grouped),
                       ("B  scan + np.unique / np.bincount", scan_line)], hcanon(1))
        bytes_res, _ = fl.Connection.resident_info(0)
        print(f"# resident image {bytes_res / 1e9:.3f} GB")
        t.close()
        conn.close()
    finally:
        os.environ.pop("FLS_HASHAGG_COMBINE", None)
        os.unlink(path)


if __name__ == "__main__":
    main()
