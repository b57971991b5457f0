#!/usr/bin/env python3
"""Map filter terms (`col op map[key]` pushdown) against the alternatives, same answers, one process.

Workload: lineitem (default SF10) read from a file on one GPU, its compressed
image resident in HBM after the warm-up.  The arms alternate (one warm-up each,
then --reps repetitions; medians and spread, max - min, of the host clock
around the synchronous call).  The queries are fixed before the first run:

  thresholds: ceil(sum(l_quantity) / (5 count(l_quantity))) per l_partkey from
      aggregate_hashed([l_partkey], [sum(l_quantity), count(l_quantity)]) (timed once, not an arm): over
      the integers l_quantity < threshold is l_quantity < 0.2 * avg(l_quantity)

  Q17 shape: sum(l_extendedprice), count(*) under l_partkey IN <the parts p with p % 1000 = 7, ~0.1 %>
             AND l_quantity < threshold[l_partkey]
    A:  Table.aggregate under both terms -- the pushed-down call (the map in its auto form)
    B:  scan_filtered under the key set delivering l_partkey, l_quantity, l_extendedprice, then a numpy
        lookup, compare and sum -- the only route without map terms
    C:  Table.aggregate under the key set alone, the floor; A - C prices the map term behind a key set

  every row probes: the same aggregates under l_quantity < threshold[l_partkey] alone
    Ad: the map forced dense;  Ah: the map forced hash
    B2: scan_filtered of the three columns with no filter, numpy lookup, compare and sum
    C2: Table.aggregate with no filter, the floor

A and B (Ad, Ah and B2) must return equal values in every repetition.  No
target time or ratio is fixed in advance; an arm counts as faster than another
when the medians differ by more than the larger spread of the two (DESIGN.md
section 24's rule); the script prints the verdicts by that rule.

    python scripts/valuemap_rate.py --scale 10 --reps 5 > profiles/valuemap/valuemap_rate_sf10.txt

--untouched runs only queries that use nothing of this feature (Q6, Q1
grouped, GROUP BY l_orderkey, one key-set and one column-pair query), from the
checkout --root names (default: this one), over the file --file names: the
process to alternate between this commit and its parent.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

Y1994, Y1995 = 8766, 9131           # 1994-01-01 and 1995-01-01 as DATE days


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def run_arms(arms, reps, same, t, norm=lambda k, out: out):
    """one warm-up each, then reps alternating repetitions; `same`: groups of arms whose results must be equal"""
    want, pruned = {}, {}
    for k, fn in arms.items():
        want[k] = norm(k, fn())
        pruned[k] = t.pruned
        print(f"warm-up {k} done", file=sys.stderr, flush=True)
    for group in same:
        for k in group[1:]:
            if want[k] != want[group[0]]:
                raise SystemExit(f"the arms disagree: {group[0]} {want[group[0]]}, {k} {want[k]}")
    times = {k: [] for k in arms}
    for _ in range(max(1, reps)):
        for k, fn in arms.items():
            s, out = timed(fn)
            assert norm(k, out) == want[k], (k, out, want[k])
            times[k].append(s)
        print(f"repetition {len(times[next(iter(arms))])} done", file=sys.stderr, flush=True)
    return want, pruned, times


def table(arms, what, want, pruned, times, nrows, rows_of):
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    print("| arm | call | rows selected | selectivity | median | spread (max - min) | all | row groups pruned |")
    print("|---|---|---|---|---|---|---|---|")
    for k in arms:
        n = rows_of(want[k])
        print(f"| {k} | {what[k]} | {n} | {n / nrows:.5f} | {1e3 * med[k]:.2f} ms | {1e3 * spread[k]:.2f} ms | "
              f"{' '.join(f'{1e3 * x:.2f}' for x in times[k])} | {pruned[k]} |")
    return med, spread


def verdict(med, spread, x, y):
    d, lim = med[x] - med[y], max(spread[x], spread[y])
    word = "no difference by the rule" if abs(d) <= lim else (f"{x} slower" if d > 0 else f"{x} faster")
    return (f"# {x} - {y} = {1e3 * d:+.2f} ms, {x} / {y} = {med[x] / med[y]:.2f}, against a larger spread of "
            f"{1e3 * lim:.2f} ms: {word}")


def untouched(fl, t, a, col):
    """queries that use nothing of the map terms; every call exists on the parent commit"""
    OKEY, PART, QTY, PRICE, DISC, TAX, RFLAG, LSTAT, SHIP, COMMIT, RECEIPT = (
        col[n] for n in ("l_orderkey", "l_partkey", "l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag",
                         "l_linestatus", "l_shipdate", "l_commitdate", "l_receiptdate"))
    conn = t.conn
    ks = conn.keyset(np.arange(7, int(200_000 * a.scale) + 1, 1000, dtype=np.int64))   # ~0.1 % of the parts
    q6 = [(SHIP, ">=", Y1994), (SHIP, "<", Y1995), (DISC, ">=", 5), (DISC, "<=", 7), (QTY, "<", 2400)]
    q1 = [("sum", QTY), ("sum", PRICE), ("sum_expr", [(0, 1, PRICE), (100, -1, DISC)]),
          ("sum_expr", [(0, 1, PRICE), (100, -1, DISC), (100, 1, TAX)]), ("count",)]
    arms = {
        "Q6": lambda: t.aggregate([("sum_product", PRICE, DISC), ("count",)], filt=q6),
        "Q1 grouped": lambda: t.aggregate_grouped([RFLAG, LSTAT], q1, filt=[(SHIP, "<=", 10471)]),
        "GROUP BY l_orderkey": lambda: t.aggregate_hashed([OKEY], [("count",), ("sum", QTY)], a.max_groups),
        "key set": lambda: t.aggregate([("sum", PRICE), ("count",)], filt=[(PART, "in_set", ks)]),
        "column pair": lambda: t.aggregate([("sum", PRICE), ("count",)], filt=[(COMMIT, "<", fl.Col(RECEIPT)),
                                                                               (SHIP, "<", fl.Col(COMMIT))]),
    }
    norm = lambda k, out: (out.ngroups, int(np.sum(out.count[0]))) if k == "GROUP BY l_orderkey" else out  # noqa: E731
    want, _, times = run_arms(arms, a.reps, [], t, norm)
    print(f"{a.label}: " + "; ".join(f"{k} {1e3 * statistics.median(v):.2f} ms (min {1e3 * min(v):.2f}, max {1e3 * max(v):.2f})"
                                     for k, v in times.items()))
    print(f"# {a.label} answers: Q6 {want['Q6']}; key set {want['key set']}; column pair {want['column pair']}; "
          f"GROUP BY l_orderkey {want['GROUP BY l_orderkey']}", file=sys.stderr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="generator threads")
    ap.add_argument("--max-groups", type=int, default=1 << 24, help="max_groups of the hashed calls")
    ap.add_argument("--note", default="", help="a line about the run copied into the output")
    ap.add_argument("--file", default="", help="an .fls file of the workload to read (written first if it is not there) "
                    "instead of a temporary one")
    ap.add_argument("--untouched", action="store_true", help="only the queries that use nothing of this feature")
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]), help="the checkout whose package runs")
    ap.add_argument("--label", default="this commit", help="--untouched: the name of the build in the output")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import pkgload
    fl = pkgload.load()
    path, temp = a.file, False
    if not path:
        fd, path = tempfile.mkstemp(suffix=".fls", dir=os.environ.get("TMPDIR", "/tmp"))
        os.close(fd)
        temp = True
    try:
        if temp or not os.path.exists(path):
            fl.gen_image("lineitem", a.scale, 0, 0, None, a.threads).write(path)
        conn = fl.Connection([0])
        t = conn.read_fls(path)
        sch = t.schema()
        col = {s[0]: c for c, s in enumerate(sch)}
        if a.untouched:
            untouched(fl, t, a, col)
            t.close()
            conn.close()
            return
        PART, QTY, PRICE = (col[n] for n in ("l_partkey", "l_quantity", "l_extendedprice"))
        nrows = t.nrows
        print(f"# lineitem SF{a.scale:g}: {nrows} rows, {t.nrowgroups} row groups, {os.path.getsize(path) / 1e9:.3f} GB "
              f"file, 1 GPU, {a.reps} repetitions per arm after one warm-up each, arms alternating; "
              f"sum(l_extendedprice), count(*)")
        if a.note:
            print(f"# {a.note}")
        # the build side: thresholds per part from the hash aggregate, then the maps (host builds)
        s_hash, hg = timed(lambda: t.aggregate_hashed([PART], [("sum", QTY), ("count", QTY)], a.max_groups))
        parts = hg.key_values[0].view(np.int64)
        sums, cnts = hg.lo[0].astype(np.int64), hg.lo[1].astype(np.int64)
        assert int(cnts.min()) > 0 and not hg.hi[0].any()
        thr = -(-sums // (5 * cnts))
        s_auto, vm = timed(lambda: conn.valuemap(parts, thr))
        s_dense, vmd = timed(lambda: conn.valuemap(parts, thr, form=fl.VALUEMAP_DENSE))
        s_hashf, vmh = timed(lambda: conn.valuemap(parts, thr, form=fl.VALUEMAP_HASH))
        brand = parts[parts % 1000 == 7]
        ks = conn.keyset(brand)
        form = {1: "dense", 2: "hash"}
        print(f"# build side: aggregate_hashed by l_partkey {1e3 * s_hash:.1f} ms ({hg.ngroups} parts, once); value maps on "
              f"the host: auto {1e3 * s_auto:.1f} ms ({form[vm.info.form]}, {vm.info.device_bytes / 1e6:.1f} MB), dense "
              f"{1e3 * s_dense:.1f} ms ({vmd.info.device_bytes / 1e6:.1f} MB), hash {1e3 * s_hashf:.1f} ms "
              f"({vmh.info.device_bytes / 1e6:.1f} MB, max_probe {vmh.info.max_probe}); thresholds {int(thr.min())} to "
              f"{int(thr.max())}; key set of {len(brand)} parts ({len(brand) / len(parts):.4%} of them)")
        # arm B's lookup: a numpy array over [min part, max part], -1 where there is no part
        pmin = int(parts.min())
        lut = np.full(int(parts.max()) - pmin + 1, -1, np.int64)
        lut[parts - pmin] = thr
        dpart, dqty, dprice = (fl.NP_DTYPE[sch[c][1]] for c in (PART, QTY, PRICE))

        def host(filt):
            rows = total = 0
            for _, _, sel, arrays in t.scan_filtered(filt, cols=[PART, QTY, PRICE]):
                p, q = arrays[PART].view(dpart).astype(np.int64), arrays[QTY].view(dqty).astype(np.int64)
                m = q < lut[p - pmin]                       # (a part without a threshold has -1: no quantity is below it)
                rows += int(m.sum())
                total += int(arrays[PRICE].view(dprice)[m].astype(np.int64).sum())
            return [total if rows else None, rows]

        aggs = [("sum", PRICE), ("count",)]
        in_set = [(PART, "in_set", ks)]
        arms = {
            "A": lambda: t.aggregate(aggs, filt=in_set + [(QTY, "<", fl.Mapped(PART, vm))]),
            "B": lambda: host(in_set),
            "C": lambda: t.aggregate(aggs, filt=in_set),
            "Ad": lambda: t.aggregate(aggs, filt=[(QTY, "<", fl.Mapped(PART, vmd))]),
            "Ah": lambda: t.aggregate(aggs, filt=[(QTY, "<", fl.Mapped(PART, vmh))]),
            "B2": lambda: host([]),
            "C2": lambda: t.aggregate(aggs),
        }
        what = {"A": "aggregate under l_partkey IN set AND l_quantity < map[l_partkey]",
                "B": "scan_filtered of 3 columns under the key set, numpy lookup, compare and sum",
                "C": "aggregate under the key set alone (the floor)",
                "Ad": "aggregate under l_quantity < map[l_partkey] alone, dense map (every row probes)",
                "Ah": "the same, hash map", "B2": "scan_filtered of 3 columns, no filter, numpy lookup, compare and sum",
                "C2": "aggregate, no filter (the floor)"}
        want, pruned, times = run_arms(arms, a.reps, [("A", "B"), ("Ad", "Ah", "B2")], t)
        med, spread = table(arms, what, want, pruned, times, nrows, lambda w: w[1])
        for x, y in (("B", "A"), ("A", "C"), ("B2", "Ad"), ("B2", "Ah"), ("Ad", "C2"), ("Ah", "C2"), ("Ah", "Ad")):
            print(verdict(med, spread, x, y))
        print(f"# answers: A = B = {want['A']}; C {want['C']}; Ad = Ah = B2 = {want['Ad']}; C2 {want['C2']}")
        bytes_res, _ = fl.Connection.resident_info(0)
        print(f"# resident image {bytes_res / 1e9:.3f} GB; A and B, and Ad, Ah and B2, returned equal values in every "
              f"repetition.  Not separated: the kernel's own time from the launch and descriptor work of one more kernel "
              f"per batch (no kernel trace was taken), and the probe's gather from the two coalesced column loads")
        t.close()
        conn.close()
    finally:
        if temp:
            os.unlink(path)


if __name__ == "__main__":
    main()
