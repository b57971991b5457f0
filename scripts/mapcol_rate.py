#!/usr/bin/env python3
"""Mapped columns (map[key] as an aggregate operand and a hash GROUP BY key) against the alternatives,
same answers, one process.

Workload: lineitem (default SF10) read from a file on one GPU, its compressed
image resident in HBM after the warm-up.  The arms alternate (one warm-up each,
then --reps repetitions; medians and spread, max - min, of the host clock
around the synchronous call).  The build sides are synthesised by rules fixed
here: cust[o] = 1 + (o * 2654435761) mod (150000 * SF) for every order o, and
cost[p] = 90000 + (p * 37) mod 100001 for every part p.  The queries:

  (a) Q10 shape: revenue = sum(l_extendedprice * (100 - l_discount)), count(*) under l_returnflag = 'R',
      the 20 largest revenues
    A:  aggregate_hashed([Mapped(l_orderkey, cust)], ..., order_by=(0, "desc"), limit=20) -- the pushed-down call
    B:  scan_filtered of l_orderkey, l_extendedprice, l_discount under the flag, then the numpy lookup,
        group-by and top 20 -- the only route without mapped columns
    C:  the same hashed call grouped by plain l_orderkey: A - C is what the gather and the smaller table
        cost or save
  (b) sum(l_quantity * cost[l_partkey]), count(*), no filter (every row probes)
    Dd: aggregate([sum_product(l_quantity, Mapped(l_partkey, cost))]) with the map forced dense;  Dh: forced hash
    E:  the same call with a plain second column, sum_product(l_quantity, l_extendedprice)
    F:  scan_filtered of l_partkey and l_quantity, numpy lookup, multiply and sum

A and B (Dd, Dh and F) must return equal values in every repetition.  No target
time or ratio is fixed in advance; an arm counts as faster than another when
the medians differ by more than the larger spread of the two (DESIGN.md section
24's rule); the script prints the verdicts by that rule.

    python scripts/mapcol_rate.py --scale 10 --reps 5 > profiles/mapcol/mapcol_rate_sf10.txt

--events: (c) the kernel's own time per batch.  The process runs with the
library's per-batch HIP events on (FLS_SCAN_PROFILE=1: one pair around each
batch's kernels on its stream) and, per call of E, Dd, Dh, C and A, reads the
summed stream time and the batch count from the report the library prints when
the table closes; a mapped call minus its plain counterpart, per batch, is
mapval_kernel plus its descriptor upload (the reduce kernel reads an 8-byte
derived column where the plain call reads a decoded one: not separated).

--untouched: (d) only queries that use nothing of this feature (Q6, Q1
grouped, GROUP BY l_orderkey), from the checkout --root names (default: this
one), over the file --file names: the process to alternate between this commit
and its parent.
"""
import argparse
import os
import re
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
            assert norm(k, out) == want[k], (k, norm(k, out), want[k])
            times[k].append(s)
        print(f"repetition {len(times[next(iter(arms))])} done", file=sys.stderr, flush=True)
    return want, pruned, times


def table(arms, what, pruned, times):
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    print("| arm | call | median | spread (max - min) | all | row groups pruned |")
    print("|---|---|---|---|---|---|")
    for k in arms:
        print(f"| {k} | {what[k]} | {1e3 * med[k]:.2f} ms | {1e3 * spread[k]:.2f} ms | "
              f"{' '.join(f'{1e3 * x:.2f}' for x in times[k])} | {pruned[k]} |")
    return med, spread


def verdict(med, spread, x, y):
    d, lim = med[x] - med[y], max(spread[x], spread[y])
    word = "no difference by the rule" if abs(d) <= lim else (f"{x} slower" if d > 0 else f"{x} faster")
    return (f"# {x} - {y} = {1e3 * d:+.2f} ms, {x} / {y} = {med[x] / med[y]:.2f}, against a larger spread of "
            f"{1e3 * lim:.2f} ms: {word}")


def untouched(fl, t, a, col):
    """queries that use nothing of the mapped columns; every call exists on the parent commit"""
    OKEY, QTY, PRICE, DISC, TAX, RFLAG, LSTAT, SHIP = (
        col[n] for n in ("l_orderkey", "l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag",
                         "l_linestatus", "l_shipdate"))
    q6 = [(SHIP, ">=", Y1994), (SHIP, "<", Y1995), (DISC, ">=", 5), (DISC, "<=", 7), (QTY, "<", 2400)]
    q1 = [("sum", QTY), ("sum", PRICE), ("sum_expr", [(0, 1, PRICE), (100, -1, DISC)]),
          ("sum_expr", [(0, 1, PRICE), (100, -1, DISC), (100, 1, TAX)]), ("count",)]
    arms = {
        "Q6": lambda: t.aggregate([("sum_product", PRICE, DISC), ("count",)], filt=q6),
        "Q1 grouped": lambda: t.aggregate_grouped([RFLAG, LSTAT], q1, filt=[(SHIP, "<=", 10471)]),
        "GROUP BY l_orderkey": lambda: t.aggregate_hashed([OKEY], [("count",), ("sum", QTY)], a.max_groups),
    }
    norm = lambda k, out: (out.ngroups, int(np.sum(out.count[0]))) if k == "GROUP BY l_orderkey" else out  # noqa: E731
    want, _, times = run_arms(arms, a.reps, [], t, norm)
    print(f"{a.label}: " + "; ".join(f"{k} {1e3 * statistics.median(v):.2f} ms (min {1e3 * min(v):.2f}, max {1e3 * max(v):.2f})"
                                     for k, v in times.items()))
    print(f"# {a.label} answers: Q6 {want['Q6']}; GROUP BY l_orderkey {want['GROUP BY l_orderkey']}", file=sys.stderr)


def closing_report(t):
    """close the table and return what the library printed to stderr while it did (the FLS_SCAN_PROFILE report)"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            t.close()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def events(fl, conn, path, calls, reps):
    """per call: the summed stream time of the batches' kernels and the batch count, from the library's HIP events"""
    rows = {}
    for name, make in calls.items():
        t = conn.read_fls(path)
        make(t)()                                   # warm-up: the image goes resident, the maps are uploaded
        closing_report(t)                           # (its report is discarded)
        t = conn.read_fls(path)
        fn = make(t)
        for _ in range(reps):
            fn()
        rep = closing_report(t)
        m = re.search(r"GPU decode \(events\)\s+([0-9.]+) ms\s+(\d+) calls", rep)
        if not m:
            raise SystemExit(f"no event line in the report of {name}:\n{rep}")
        rows[name] = (float(m.group(1)), int(m.group(2)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="generator threads")
    ap.add_argument("--max-groups", type=int, default=1 << 24, help="max_groups of the hashed calls")
    ap.add_argument("--note", default="", help="a line about the run copied into the output")
    ap.add_argument("--file", default="", help="an .fls file of the workload to read (written first if it is not there) "
                    "instead of a temporary one")
    ap.add_argument("--events", action="store_true", help="(c): the batches' kernel time from the library's HIP events")
    ap.add_argument("--untouched", action="store_true", help="(d): only the queries that use nothing of this feature")
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]), help="the checkout whose package runs")
    ap.add_argument("--label", default="this commit", help="--untouched: the name of the build in the output")
    a = ap.parse_args()
    if a.events:
        os.environ["FLS_SCAN_PROFILE"] = "1"        # (read once, at the library's first scan)
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
        OKEY, PART, QTY, PRICE, DISC, RFLAG = (col[n] for n in ("l_orderkey", "l_partkey", "l_quantity", "l_extendedprice",
                                                                "l_discount", "l_returnflag"))
        nrows = t.nrows
        # the build sides (host builds): every order's customer, every part's cost
        s_ord, hg = timed(lambda: t.aggregate_hashed([OKEY], [("count",)], a.max_groups))
        orders = np.sort(hg.key_values[0].view(np.int64))
        ncust = max(1, int(150000 * a.scale))
        cust_of = 1 + (orders * 2654435761) % ncust
        s_cust, cust = timed(lambda: conn.valuemap(orders, cust_of))
        nparts = int(200000 * a.scale)
        parts = np.arange(1, nparts + 1, dtype=np.int64)
        cost_of = 90000 + (parts * 37) % 100001
        s_dense, costd = timed(lambda: conn.valuemap(parts, cost_of, form=fl.VALUEMAP_DENSE))
        s_hashf, costh = timed(lambda: conn.valuemap(parts, cost_of, form=fl.VALUEMAP_HASH))
        form = {1: "dense", 2: "hash"}
        rev = ("sum_expr", [(0, 1, PRICE), (100, -1, DISC)])
        flag = [(RFLAG, "=", "R")]
        K = fl.Mapped(OKEY, cust)

        def q10(tab, key):
            return lambda: tab.aggregate_hashed([key], [rev, ("count",)], a.max_groups, filt=flag, order_by=(0, "desc"),
                                                limit=20)

        def cost_sum(tab, second):
            return lambda: tab.aggregate([("sum_product", QTY, second), ("count",)])

        if a.events:
            calls = {"E": lambda tab: cost_sum(tab, PRICE), "Dd": lambda tab: cost_sum(tab, fl.Mapped(PART, costd)),
                     "Dh": lambda tab: cost_sum(tab, fl.Mapped(PART, costh)), "C": lambda tab: q10(tab, OKEY),
                     "A": lambda tab: q10(tab, K)}
            nrgs = t.nrowgroups
            t.close()
            rows = events(fl, conn, path, calls, a.reps)
            print(f"# (c) lineitem SF{a.scale:g}, {nrows} rows: the batches' kernels on their streams, from the library's HIP "
                  f"events (FLS_SCAN_PROFILE), {a.reps} calls each after a warm-up; {nrgs} row groups, a batch is "
                  f"FLS_SCAN_BATCH (default 8) of them: 524,288 rows where they are full")
            print("| call | stream time, all batches | batches | per batch |")
            print("|---|---|---|---|")
            for k, (ms, n) in rows.items():
                print(f"| {k} | {ms:.2f} ms | {n} | {1e3 * ms / max(1, n):.1f} us |")
            for x, y in (("Dd", "E"), ("Dh", "E"), ("A", "C")):
                d = rows[x][0] / max(1, rows[x][1]) - rows[y][0] / max(1, rows[y][1])
                print(f"# {x} - {y} per batch: {1e3 * d:+.1f} us (mapval_kernel, its descriptors, and the reduce kernel's "
                      f"8-byte derived operand in place of a decoded column)")
            conn.close()
            return
        print(f"# lineitem SF{a.scale:g}: {nrows} rows, {t.nrowgroups} row groups, {os.path.getsize(path) / 1e9:.3f} GB "
              f"file, 1 GPU, {a.reps} repetitions per arm after one warm-up each, arms alternating")
        if a.note:
            print(f"# {a.note}")
        print(f"# build sides: aggregate_hashed by l_orderkey {1e3 * s_ord:.1f} ms ({len(orders)} orders, once); customer "
              f"map on the host {1e3 * s_cust:.1f} ms ({form[cust.info.form]}, {cust.info.device_bytes / 1e6:.1f} MB, "
              f"{ncust} customers); cost maps of {nparts} parts: dense {1e3 * s_dense:.1f} ms "
              f"({costd.info.device_bytes / 1e6:.1f} MB), hash {1e3 * s_hashf:.1f} ms ({costh.info.device_bytes / 1e6:.1f} MB, "
              f"max_probe {costh.info.max_probe})")
        dt = {c: fl.NP_DTYPE[sch[c][1]] for c in (OKEY, PART, QTY, PRICE, DISC)}

        def host_q10():
            ks, rs, firsts = [], [], []
            for _, first, sel, arrays in t.scan_filtered(flag, cols=[OKEY, PRICE, DISC]):
                o = arrays[OKEY].view(dt[OKEY]).astype(np.int64)
                ks.append(cust_of[np.searchsorted(orders, o)])         # (every order has a customer)
                rs.append(arrays[PRICE].view(dt[PRICE]).astype(np.int64) * (100 - arrays[DISC].view(dt[DISC]).astype(np.int64)))
                firsts.append(sel.astype(np.int64) + first)
            k, r, f = np.concatenate(ks), np.concatenate(rs), np.concatenate(firsts)
            u, idx, inv = np.unique(k, return_index=True, return_inverse=True)
            sums = np.bincount(inv, weights=r.astype(np.float64)).astype(np.int64)   # (exact: every sum is below 2^53)
            cnt = np.bincount(inv)
            best = np.lexsort((f[idx], -sums))[:20]
            return [(int(u[i]), int(sums[i]), int(cnt[i])) for i in best]

        lut = np.zeros(nparts + 1, np.int64)
        lut[parts] = cost_of

        def host_cost():
            total = rows = 0
            for _, _, _, arrays in t.scan_filtered([], cols=[PART, QTY]):
                p, q = arrays[PART].view(dt[PART]).astype(np.int64), arrays[QTY].view(dt[QTY]).astype(np.int64)
                total += int((q * lut[p]).sum())
                rows += len(p)
            return [total, rows]

        arms = {"A": q10(t, K), "B": host_q10, "C": q10(t, OKEY), "Dd": cost_sum(t, fl.Mapped(PART, costd)),
                "Dh": cost_sum(t, fl.Mapped(PART, costh)), "E": cost_sum(t, PRICE), "F": host_cost}
        what = {"A": "aggregate_hashed by cust[l_orderkey], revenue and count under the flag, top 20",
                "B": "scan_filtered of 3 columns under the flag, numpy lookup, group-by and top 20",
                "C": "the same hashed call by plain l_orderkey",
                "Dd": "aggregate sum(l_quantity * cost[l_partkey]), dense map (every row probes)", "Dh": "the same, hash map",
                "E": "aggregate sum(l_quantity * l_extendedprice): a plain second column",
                "F": "scan_filtered of 2 columns, numpy lookup, multiply and sum"}

        def norm(k, out):
            if k in ("A", "C"):
                return [(key[0], v[0], v[1]) for key, v in out.to_list()]
            return out

        want, pruned, times = run_arms(arms, a.reps, [("A", "B"), ("Dd", "Dh", "F")], t, norm)
        med, spread = table(arms, what, pruned, times)
        for x, y in (("B", "A"), ("A", "C"), ("F", "Dd"), ("F", "Dh"), ("Dd", "E"), ("Dh", "E"), ("Dh", "Dd")):
            print(verdict(med, spread, x, y))
        print(f"# answers: A = B, best group {want['A'][0]}; C best group {want['C'][0]}; Dd = Dh = F = {want['Dd']}; "
              f"E {want['E']}")
        bytes_res, _ = fl.Connection.resident_info(0)
        print(f"# resident image {bytes_res / 1e9:.3f} GB; A and B, and Dd, Dh and F, returned equal values in every "
              f"repetition.  Not measured here: other scale factors, several GPUs")
        t.close()
        conn.close()
    finally:
        if temp:
            os.unlink(path)


if __name__ == "__main__":
    main()
