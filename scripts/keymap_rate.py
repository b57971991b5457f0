#!/usr/bin/env python3
"""Key-map group keys (GROUP BY a joined attribute) against the delivering scan, same answers, one process.

Workload: lineitem (default SF10) read from a file on one GPU, its compressed
image resident in HBM after the warm-up.  Per query three arms alternate (one
warm-up each, then --reps repetitions, medians of the host clock around the
synchronous call):

  A: Table.aggregate_grouped with a ("map", column, keymap) key -- the pushed-down call
  B: scan_filtered of the needed columns over the link, a numpy lookup of the key's code and a numpy
     group-by (what a caller does without the pushdown)
  C: the same aggregates under the same filter grouped by plain low-cardinality column(s), no map:
     the floor A can approach (decode + filter + grouped reduction, no probe)

The query list is fixed before the first run:

  Q5 shape   l_suppkey -> 25 codes ("nation" = (7 * suppkey + 3) mod 25 for every distinct supplier key),
             sum_expr(l_extendedprice * (1 - l_discount)) and count(*), l_shipdate in 1994; the map as
             auto, forced dense and forced hash; C groups by l_linenumber
  Q12 shape  l_orderkey -> {0, 1} for every distinct order key (the "priority class" of the order: a hash
             bit of the key), grouped with l_shipmode, count(*), l_receiptdate in 1994; the map forced
             dense and forced hash; C groups by l_shipmode and l_linestatus

A and B must return equal groups, in the same order, with equal values in every repetition.

    python scripts/keymap_rate.py --scale 10 --reps 5 > profiles/keymap/keymap_rate_sf10.txt
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

C_OKEY, C_SUPP, C_LINE, C_PRICE, C_DISC, C_STATUS, C_SHIPDATE, C_RECEIPT, C_MODE = 0, 2, 3, 5, 6, 9, 10, 12, 14
DAY_1994, DAY_1995 = 8766, 9131
FORMS = {"auto": 0, "dense": 1, "hash": 2}
L2_BYTES, MALL_BYTES = 4 << 20, 256 << 20   # L2 per XCD, Infinity Cache


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def scan_columns(fl, t, cols, filt=None):
    """arm B's transfer: the (selected rows of the) columns over the link, as numpy arrays"""
    sch = t.schema()
    parts = {c: [] for c in cols}
    it = (arrays for _, _, _, arrays in t.scan_filtered(filt, cols=cols)) if filt else \
        (arrays for _, arrays in t.scan(cols=cols))
    for arrays in it:
        for c in cols:
            a = arrays[c]
            parts[c].append(a.view(np.uint64).reshape(-1, 2) if sch[c][1] in fl.STRING_TYPES else
                            a.view(fl.NP_DTYPE[sch[c][1]]))
    return {c: np.concatenate(parts[c]) for c in cols}


def lookup(keys, codes, col):
    """the code of every value of col (all present in the sorted keys)"""
    return codes[np.searchsorted(keys, col)]


def grouped(group, measures):
    """[(group id, [int sums..., count])] in order of first occurrence, exact int64 sums"""
    uniq, first, inv = np.unique(group, return_index=True, return_inverse=True)
    order = np.argsort(inv, kind="stable")
    starts = np.searchsorted(inv[order], np.arange(len(uniq)))
    sums = [np.add.reduceat(m[order], starts) for m in measures]
    counts = np.bincount(inv, minlength=len(uniq))
    return [(uniq[u], [int(s[u]) for s in sums] + [int(counts[u])]) for u in np.argsort(first)]


def arm_b_q5(fl, t, filt, keys, codes):
    cols = scan_columns(fl, t, [C_SUPP, C_PRICE, C_DISC], filt)
    rev = cols[C_PRICE] * (100 - cols[C_DISC])
    return [((int(g),), v) for g, v in grouped(lookup(keys, codes, cols[C_SUPP]), [rev])]


def arm_b_q12(fl, t, filt, keys, codes):
    cols = scan_columns(fl, t, [C_OKEY, C_MODE], filt)
    rec = cols[C_MODE]                                    # string_t records: the modes are short, inlined strings
    mode_id, mode_first = np.unique(rec[:, 0] * np.uint64(31) + rec[:, 1], return_index=True)
    names = {int(m): bytes(rec[i].view(np.uint8)[4:4 + int(rec[i, 0] & np.uint64(0xFFFFFFFF))])
             for m, i in zip(mode_id, mode_first)}
    mid = np.searchsorted(mode_id, rec[:, 0] * np.uint64(31) + rec[:, 1])
    code = lookup(keys, codes, cols[C_OKEY]).astype(np.int64)
    return [((int(g) % 2, names[int(mode_id[int(g) // 2])]), v) for g, v in grouped(mid * 2 + code, [])]


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
        print(f"# lineitem SF{a.scale:g}: {t.nrows} rows, {t.nrowgroups} row groups, {os.path.getsize(path) / 1e9:.3f} GB "
              f"file, 1 GPU, {a.reps} repetitions per arm after one warm-up each, arms alternating", flush=True)
        if a.note:
            print(f"# {a.note}")
        # ---- the build sides and the query list, fixed before the first run
        keycols = scan_columns(fl, t, [C_SUPP, C_OKEY])
        supp, okey = np.unique(keycols[C_SUPP]), np.unique(keycols[C_OKEY])
        del keycols
        nation = ((supp.astype(np.int64) * 7 + 3) % 25).astype(np.uint16)
        prio = ((okey.astype(np.uint64) * np.uint64(2654435761) >> np.uint64(7)) & np.uint64(1)).astype(np.uint16)
        print(f"# {len(supp)} distinct supplier keys in [{int(supp[0])}, {int(supp[-1])}] -> 25 codes; {len(okey)} distinct "
              f"order keys in [{int(okey[0])}, {int(okey[-1])}] -> 2 codes", flush=True)
        q5 = dict(text="Q5 shape: l_suppkey -> 25 codes, sum_expr + count(*), l_shipdate in 1994", col=C_SUPP, keys=supp,
                  codes=nation, aggs=[("sum_expr", [(0, 1, C_PRICE), (100, -1, C_DISC)]), ("count",)],
                  filt=[(C_SHIPDATE, ">=", DAY_1994), (C_SHIPDATE, "<", DAY_1995)], more=[], plain=[C_LINE], b=arm_b_q5)
        q12 = dict(text="Q12 shape: l_orderkey -> {0, 1} with l_shipmode, count(*), l_receiptdate in 1994", col=C_OKEY,
                   keys=okey, codes=prio, aggs=[("count",)],
                   filt=[(C_RECEIPT, ">=", DAY_1994), (C_RECEIPT, "<", DAY_1995)], more=[C_MODE],
                   plain=[C_STATUS, C_MODE], b=arm_b_q12)
        queries = [(q5, f) for f in ("auto", "dense", "hash")] + [(q12, f) for f in ("dense", "hash")]
        print("| query | form asked | form built | map image | build | A pushed down | B scan + numpy | C plain key | B / A | "
              "A - C | groups | rows grouped | row groups pruned |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        detail = []
        for q, form in queries:
            tbuild, km = timed(lambda: conn.keymap(q["keys"], q["codes"], form=FORMS[form]))
            info = km.info
            fa = lambda: t.aggregate_grouped([("map", q["col"], km)] + q["more"], q["aggs"], filt=q["filt"])   # noqa: E731
            fb = lambda: q["b"](fl, t, q["filt"], q["keys"], q["codes"])                                         # noqa: E731
            fc = lambda: t.aggregate_grouped(q["plain"], q["aggs"], filt=q["filt"])                              # noqa: E731
            want_a, want_b, want_c = fa(), fb(), fc()                        # warm-up: the map reaches the GPU
            if want_a != want_b:
                raise SystemExit(f"{q['text']} ({form}): the arms disagree: pushed down {want_a[:3]}, scan {want_b[:3]}")
            ta, tb, tc = [], [], []
            for _ in range(max(1, a.reps)):
                s, out = timed(fa)
                assert out == want_b, (q["text"], form)
                ta.append(s)
                pruned = t.pruned
                s, out = timed(fb)
                assert out == want_a, (q["text"], form)
                tb.append(s)
                s, out = timed(fc)
                assert out == want_c, (q["text"], form)
                tc.append(s)
            ma, mb, mc = (statistics.median(x) for x in (ta, tb, tc))
            built = {1: "dense", 2: "hash"}[info.form]
            rows = sum(v[-1] for _, v in want_a)
            print(f"| {q['text']} | {form} | {built} | {footprint(info.device_bytes)} | {1e3 * tbuild:.0f} ms | "
                  f"{1e3 * ma:.2f} ms | {1e3 * mb:.1f} ms | {1e3 * mc:.2f} ms | {mb / ma:.1f} | {1e3 * (ma - mc):+.2f} ms | "
                  f"{len(want_a)} | {rows} | {pruned} |", flush=True)
            detail.append(f"# {q['text']} ({form} -> {built}, {info.count} keys, capacity {info.capacity}, longest probe "
                          f"{info.max_probe}): first group {want_a[0]}; C has {len(want_c)} groups; A all "
                          f"{' '.join(f'{1e3 * x:.2f}' for x in ta)} ms; B all {' '.join(f'{1e3 * x:.1f}' for x in tb)} ms; "
                          f"C all {' '.join(f'{1e3 * x:.2f}' for x in tc)} ms")
            km.close()
        print("\n".join(detail))
        bytes_res, _ = fl.Connection.resident_info(0)
        print(f"# resident image {bytes_res / 1e9:.3f} GB (the maps' images are not part of it); A and B returned equal "
              f"groups, order and values in every repetition")
        t.close()
        conn.close()
    finally:
        os.unlink(path)


if __name__ == "__main__":
    main()
