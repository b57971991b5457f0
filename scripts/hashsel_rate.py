#!/usr/bin/env python3
"""Selecting a hash aggregate's groups on the GPU against selecting them in numpy, same answers, one process.

Workload: lineitem (default SF10) read from a file on one GPU, its compressed
image resident in HBM after the warm-up.  Three queries of two arms each; the
arms alternate (one warm-up each, then --reps repetitions, medians of the host
clock around the synchronous calls):

  (q18)     the Q18 shape: GROUP BY l_orderkey of sum(l_quantity), count(*) HAVING sum(l_quantity) > 300
            S: Table.aggregate_hashed(having=[(0, ">", 30000)])
            B: the plain Table.aggregate_hashed, then the same HAVING over its arrays in numpy
  (q3)      the Q3 shape: l_orderkey IN a key set of a fifth of the orders, l_shipdate > 1995-03-15,
            GROUP BY l_orderkey of sum(l_extendedprice * (1 - l_discount)) ORDER BY 1 DESC LIMIT 10
            S: Table.aggregate_hashed(order_by=(0, "desc"), limit=10)
            B: the plain call, then np.partition / np.lexsort by (-value, first row)
  (allpass) (q18)'s GROUP BY with a HAVING every group passes, count(*) > 0: what the selection itself costs
            S: Table.aggregate_hashed(having=[(1, ">", 0)])
            B: the plain call, which returns the same groups

B is the only way to these answers without the selection.  A time is the
Python call (and for B the numpy selection after it), which ends with the
result's arrays copied into numpy; to_list is not called.  The phases the
library times itself and the selection's statistics are printed per arm.  The
arms' answers are compared before anything is printed.  An arm is called
faster when the medians differ by more than the larger spread (max - min) of
the two arms' repetitions.

    python scripts/hashsel_rate.py --scale 10 --reps 5 --out profiles/hashsel/hashsel_rate_sf10.txt
"""
import argparse
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

C_OKEY, C_QTY, C_PRICE, C_DISC, C_SHIPDATE = 0, 4, 5, 6, 10
DAY_Q3 = 9204                        # 1995-03-15 as DATE days
REVENUE = ("sum_expr", [(0, 1, C_PRICE), (100, -1, C_DISC)])    # scale 4
QTY_300 = 30000                      # 300 at scale 2


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


class Chosen:
    """what an arm answers: the chosen groups' arrays, and the HashGroups they came from"""

    def __init__(self, h, idx=None):
        pick = (lambda x: x) if idx is None else (lambda x: x[idx])
        self.h = h
        self.keys = pick(h.key_values[0].view(np.int64))
        self.first = pick(h.first_row)
        self.vals = [pick(x) for a in range(len(h.count)) for x in (h.count[a], h.lo[a], h.hi[a])]

    def canon(self, ordered):
        o = np.arange(len(self.keys)) if ordered else np.argsort(self.keys, kind="stable")
        return [self.keys[o], self.first[o]] + [v[o] for v in self.vals]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def run_query(out, name, title, nrows, reps, arms, ordered):
    """arms: [(label, fn)], fn() -> Chosen; the first arm is the selection, the second its baseline"""
    want = [fn().canon(ordered) for _, fn in arms]       # warm-up: the image becomes resident, buffers are allocated
    if not same(want[0], want[1]):
        raise SystemExit(f"{name}: the arms disagree")
    times = [[] for _ in arms]
    last = [None] * len(arms)
    for _ in range(max(1, reps)):
        for k, (_, fn) in enumerate(arms):
            s, res = timed(fn)
            times[k].append(s)
            last[k] = res
    for res, w in zip(last, want):
        assert same(res.canon(ordered), w), name
    med = [statistics.median(x) for x in times]
    spread = [max(x) - min(x) for x in times]
    print(f"{name}: {title}", file=out)
    print(f"{name}: {len(want[0][0])} groups returned; both arms returned the same keys, first rows and values"
          f"{', in the same order' if ordered else ''}", file=out)
    for (label, _), m, sp, x, res in zip(arms, med, spread, times, last):
        h = res.h
        print(f"{name}: {label:<46s} median {1e3 * m:10.3f} ms  spread {1e3 * sp:8.3f} ms  ({nrows / m:.3e} rows/s)  "
              f"all {' '.join(f'{1e3 * y:.3f}' for y in x)}", file=out)
        print(f"{name}:   last repetition inside the call: scan {h.scan_ms:.3f} ms, extraction + D2H (with the device's "
              f"selection) {h.extract_ms:.3f} ms, merge + unpacking {h.merge_ms:.3f} ms; selection {h.select_ms:.3f} ms "
              f"{'on the device' if h.selected_on_device else 'not on the device'}; groups formed {h.groups_total}, "
              f"passed {h.groups_passed}, returned {len(h)}; table {h.table_bytes / 1e6:.1f} MB", file=out)
    diff, tol = med[1] - med[0], max(spread)
    verdict = "faster than" if diff > tol else ("slower than" if -diff > tol else "within the spread of")
    print(f"{name}: the selection is {verdict} its baseline: medians differ by {1e3 * diff:.3f} ms "
          f"({med[1] / med[0]:.2f}x), the larger spread is {1e3 * tol:.3f} ms", file=out)
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="generator threads")
    ap.add_argument("--query", choices=["all", "q18", "q3", "allpass"], default="all")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hashsel" / "hashsel_rate_sf10.txt"))
    a = ap.parse_args()
    fl = pkgload.load()
    if fl.device_count() < 1:
        raise SystemExit("hashsel_rate.py measures on a GPU and found none")
    fd, path = tempfile.mkstemp(suffix=".fls", dir=os.environ.get("TMPDIR", "/tmp"))
    os.close(fd)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    try:
        fl.gen_image("lineitem", a.scale, 0, 0, None, a.threads).write(path)
        conn = fl.Connection([0])
        t = conn.read_fls(path)
        nrows = t.nrows
        top = int(t.zonemap(t.nrowgroups - 1, C_OKEY)[1])
        with open(a.out, "w") as out:
            print(f"# lineitem SF{a.scale:g}: {nrows} rows, {t.nrowgroups} row groups, "
                  f"{os.path.getsize(path) / 1e9:.3f} GB file, 1 GPU, {a.reps} repetitions per arm after one warm-up "
                  f"each, arms alternating", file=out)
            if a.query in ("all", "q18", "allpass"):
                aggs = [("sum", C_QTY), ("count",)]
                ngroups = len(t.aggregate_hashed([C_OKEY], aggs, top))       # the distinct keys: the tightest table

                def plain():
                    return t.aggregate_hashed([C_OKEY], aggs, ngroups)
            if a.query in ("all", "q18"):
                def q18_numpy():
                    h = plain()
                    return Chosen(h, np.nonzero((h.lo[0].view(np.int64) > QTY_300) & (h.hi[0] == 0))[0])
                run_query(out, "q18", "group by l_orderkey of sum(l_quantity), count(*) having sum(l_quantity) > 300",
                          nrows, a.reps,
                          [("S aggregate_hashed(having=)", lambda: Chosen(t.aggregate_hashed(
                              [C_OKEY], aggs, ngroups, having=[(0, ">", QTY_300)]))),
                           ("B aggregate_hashed + the HAVING in numpy", q18_numpy)], False)
            if a.query in ("all", "q3"):
                ks = conn.keyset(np.arange(5, top + 1, 5, dtype=np.int64), signed=True)      # a fifth of the order keys
                filt = [(C_OKEY, "in_set", ks), (C_SHIPDATE, ">", DAY_Q3)]
                n3 = max(1, len(t.aggregate_hashed([C_OKEY], [REVENUE], ks.info.count, filt=filt)))

                def q3_numpy():
                    h = t.aggregate_hashed([C_OKEY], [REVENUE], n3, filt=filt)
                    v = h.lo[0].view(np.int64)
                    assert not h.hi[0].any(), "a revenue does not fit 64 bits"
                    k = min(10, len(v))
                    cand = np.nonzero(v >= np.partition(v, len(v) - k)[len(v) - k])[0] if k else np.zeros(0, np.int64)
                    return Chosen(h, cand[np.lexsort((h.first_row[cand], -v[cand]))][:k])
                run_query(out, "q3", "group by l_orderkey of sum(l_extendedprice * (1 - l_discount)) where l_orderkey "
                          f"in a key set of {ks.info.count} keys and l_shipdate > 1995-03-15 order by 1 desc limit 10",
                          nrows, a.reps,
                          [("S aggregate_hashed(order_by=, limit=10)", lambda: Chosen(t.aggregate_hashed(
                              [C_OKEY], [REVENUE], n3, filt=filt, order_by=(0, "desc"), limit=10))),
                           ("B aggregate_hashed + np.partition / np.lexsort", q3_numpy)], True)
                ks.close()
            if a.query in ("all", "allpass"):
                run_query(out, "allpass", "group by l_orderkey of sum(l_quantity), count(*) having count(*) > 0",
                          nrows, a.reps,
                          [("S aggregate_hashed(having=), every group passes", lambda: Chosen(t.aggregate_hashed(
                              [C_OKEY], aggs, ngroups, having=[(1, ">", 0)]))),
                           ("B aggregate_hashed", lambda: Chosen(plain()))], False)
            bytes_res, _ = fl.Connection.resident_info(0)
            print(f"# resident image {bytes_res / 1e9:.3f} GB", file=out)
        t.close()
        conn.close()
        sys.stdout.write(Path(a.out).read_text())
    finally:
        os.unlink(path)


if __name__ == "__main__":
    main()
