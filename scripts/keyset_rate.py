#!/usr/bin/env python3
"""Key-set filter terms (semi-join pushdown) against the delivering scan, same answers, one process.

Workload: lineitem (default SF10) read from a file on one GPU, its compressed
image resident in HBM after the warm-up.  Per query three arms alternate (one
warm-up each, then --reps repetitions, medians of the host clock around the
synchronous call):

  A: Table.aggregate([sum(l_extendedprice), count(*)]) under (l_orderkey, "in_set", set) -- the pushed-down call
  B: scan of l_orderkey and l_extendedprice over the link, one np.isin over the table's keys and a sum
     (what a caller does without the pushdown)
  C: the same aggregate with no filter: the floor (decode + reduction, no probe)

The query list is fixed before the first run: seeded random subsets of the
distinct order keys of about 10^3, 10^5, 10^6 keys and half of all orders, each
as auto, forced bitmap and forced hash; one NOT IN query (10^5 keys, auto); and
a Q3-shaped query whose set Table.keyset builds from a filtered scan of the
table (l_shipdate < 1995-03-15 and l_quantity < 5) and which adds the ordinary
term l_shipdate > 1995-03-15.  A and B must return equal values in every
repetition.

    python scripts/keyset_rate.py --scale 10 --reps 5 > profiles/keyset/keyset_rate_sf10.txt
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

C_OKEY, C_QTY, C_PRICE, C_SHIPDATE = 0, 4, 5, 10
DAY_Q3 = 9204                       # 1995-03-15 as DATE days
AGGS = [("sum", C_PRICE), ("count",)]
FORMS = {"auto": 0, "bitmap": 1, "hash": 2}
L2_BYTES, MALL_BYTES = 4 << 20, 256 << 20   # L2 per XCD, Infinity Cache


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def scan_columns(fl, t, cols):
    """arm B's transfer: the whole columns over the link, as numpy arrays"""
    sch = t.schema()
    parts = {c: [] for c in cols}
    for _, arrays in t.scan(cols=cols):
        for c in cols:
            parts[c].append(arrays[c].view(fl.NP_DTYPE[sch[c][1]]))
    return {c: np.concatenate(parts[c]) for c in cols}


def arm_b(fl, t, keys, negate, ship_after=None):
    cols = scan_columns(fl, t, [C_OKEY, C_PRICE] + ([C_SHIPDATE] if ship_after is not None else []))
    m = np.isin(cols[C_OKEY], keys)
    if negate:
        m = ~m
    if ship_after is not None:
        m &= cols[C_SHIPDATE] > ship_after
    rows = int(m.sum())
    return [int(cols[C_PRICE][m].sum()) if rows else None, rows]


def footprint(nbytes):
    where = "fits one XCD's 4 MiB L2" if nbytes <= L2_BYTES else \
        "past L2, fits the 256 MiB Infinity Cache" if nbytes <= MALL_BYTES else "past the Infinity Cache (HBM)"
    return f"{nbytes / (1 << 20):.3f} MiB ({where})"


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
        print(f"# lineitem SF{a.scale:g}: {nrows} rows, {t.nrowgroups} row groups, {os.path.getsize(path) / 1e9:.3f} GB "
              f"file, 1 GPU, {a.reps} repetitions per arm after one warm-up each, arms alternating; "
              f"sum(l_extendedprice), count(*)")
        if a.note:
            print(f"# {a.note}")
        okey = scan_columns(fl, t, [C_OKEY])[C_OKEY]
        distinct = np.unique(okey)
        del okey
        print(f"# {len(distinct)} distinct order keys in [{int(distinct[0])}, {int(distinct[-1])}]")
        # ---- the query list, fixed before the first run
        rng = np.random.default_rng(2024)
        sizes = [n for n in (10 ** 3, 10 ** 5, 10 ** 6) if n < len(distinct) // 2] + [len(distinct) // 2]
        subsets = {n: np.sort(rng.choice(distinct, n, replace=False)) for n in sizes}
        queries = [(f"IN {n} keys", n, form, False, None) for n in sizes for form in FORMS]
        not_in_n = sizes[min(1, len(sizes) - 1)]
        queries.append((f"NOT IN {not_in_n} keys", not_in_n, "auto", True, None))
        queries.append(("Q3 shape: IN Table.keyset(...) AND l_shipdate > 1995-03-15", None, "auto", False, DAY_Q3))
        floor = lambda: t.aggregate(AGGS)                                         # noqa: E731
        want_c = floor()
        print("| query | form asked | form built | set image | A pushed down | B scan + np.isin | C no filter | B / A | "
              "A - C | rows selected | row groups pruned |")
        print("|---|---|---|---|---|---|---|---|---|---|---|")
        detail = []
        for text, n, form, negate, ship_after in queries:
            if n is None:
                build = [(C_SHIPDATE, "<", DAY_Q3), (C_QTY, "<", 500)]
                tb, ks = timed(lambda: t.keyset(C_OKEY, build))
                keys = np.unique(scan_filtered_keys(fl, t, build))
                detail.append(f"# {text}: Table.keyset built {ks.info.count} keys in {1e3 * tb:.1f} ms (one filtered scan "
                              f"of l_orderkey + the host construction)")
                assert ks.info.count == len(keys)
            else:
                keys = subsets[n]
                ks = conn.keyset(keys, form=FORMS[form])
            info = ks.info
            filt = [(C_OKEY, "not_in_set" if negate else "in_set", ks)]
            if ship_after is not None:
                filt.append((C_SHIPDATE, ">", ship_after))
            fa = lambda: t.aggregate(AGGS, filt=filt)                             # noqa: E731
            fb = lambda: arm_b(fl, t, keys, negate, ship_after)                   # noqa: E731
            want_a, want_b = fa(), fb()                                           # warm-up: the set reaches the GPU
            if want_a != want_b:
                raise SystemExit(f"{text} ({form}): the arms disagree: pushed down {want_a}, scan {want_b}")
            ta, tb, tc = [], [], []
            for _ in range(max(1, a.reps)):
                s, out = timed(fa)
                assert out == want_b, (text, form, out, want_b)
                ta.append(s)
                pruned = t.pruned
                s, out = timed(fb)
                assert out == want_a, (text, form, out, want_a)
                tb.append(s)
                s, out = timed(floor)
                assert out == want_c, (text, form)
                tc.append(s)
            ma, mb, mc = (statistics.median(x) for x in (ta, tb, tc))
            built = {1: "bitmap", 2: "hash"}[info.form]
            print(f"| {text} | {form} | {built} | {footprint(info.device_bytes)} | {1e3 * ma:.2f} ms | {1e3 * mb:.1f} ms | "
                  f"{1e3 * mc:.2f} ms | {mb / ma:.1f} | {1e3 * (ma - mc):+.2f} ms | {want_a[1]} | {pruned} |")
            detail.append(f"# {text} ({form} -> {built}, capacity {info.capacity}, longest probe {info.max_probe}): answer "
                          f"{want_a}; A all {' '.join(f'{1e3 * x:.2f}' for x in ta)} ms; B all "
                          f"{' '.join(f'{1e3 * x:.1f}' for x in tb)} ms; C all {' '.join(f'{1e3 * x:.2f}' for x in tc)} ms")
            ks.close()
        print("\n".join(detail))
        bytes_res, _ = fl.Connection.resident_info(0)
        print(f"# resident image {bytes_res / 1e9:.3f} GB (the sets' images are not part of it); unfiltered answer {want_c}; "
              f"A and B returned equal values in every repetition")
        t.close()
        conn.close()
    finally:
        os.unlink(path)


def scan_filtered_keys(fl, t, filt):
    parts = [arrays[C_OKEY].view(np.int64) for _, _, _, arrays in t.scan_filtered(filt, cols=[C_OKEY])]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


if __name__ == "__main__":
    main()
