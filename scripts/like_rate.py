#!/usr/bin/env python3
"""String pattern filter terms (LIKE pushdown) against the alternatives, same answers, one process.

Workload: lineitem_full (default SF10; l_comment FSST-compressed) read from a
file on one GPU, its compressed image resident in HBM after the warm-up.
Three filters, fixed before the first run, words from the generator's own
vocabulary (csrc/fls_text.hpp, csrc/fls_writer.cpp):

  1. l_shipinstruct LIKE 'TAKE%'            a prefix on a DICT column
  2. l_comment LIKE '%furious%'             one word anywhere in an FSST column
  3. l_comment LIKE '%regular%deposits%'    two words in order

Per filter the arms alternate (one warm-up each, then --reps repetitions,
medians of the host clock around the synchronous call):

  A: Table.aggregate([count(*), sum(l_extendedprice)]) under the LIKE term -- the pushed-down call
  E: the same aggregate under an `=` string term on the same column: what filter_kernel already costs there
  C: the same aggregate with no filter: the floor (decode + reduction)
  B: the host alternative: a scan delivering the column and l_extendedprice over the link and Python
     matching (bytes.startswith / find) -- over the first --host-rowgroups row groups only, once, and
     scaled by rows to the whole table (the Python matching of 60 M strings takes minutes)

A's answer must equal B's over B's row groups in the run.

    python scripts/like_rate.py --scale 10 --reps 5 > profiles/like/like_rate_sf10.txt
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

C_PRICE, C_INSTR, C_COMMENT = 5, 13, 15
AGGS = [("count",), ("sum", C_PRICE)]
FILTERS = [
    ("l_shipinstruct LIKE 'TAKE%'", C_INSTR, b"TAKE%", lambda s: s.startswith(b"TAKE"), b"TAKE BACK RETURN"),
    ("l_comment LIKE '%furious%'", C_COMMENT, b"%furious%", lambda s: b"furious" in s, b"furiously regular deposits"),
    ("l_comment LIKE '%regular%deposits%'", C_COMMENT, b"%regular%deposits%",
     lambda s: 0 <= s.find(b"regular") and s.find(b"deposits", s.find(b"regular") + 7) >= 0, b"furiously regular deposits"),
]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def host_arm(fl, t, col, match, rg_end):
    """arm B over row groups [0, rg_end): deliver the column and the price, match in Python"""
    rows = total = n = 0
    for _, arrays in t.scan(cols=[col, C_PRICE], rg_end=rg_end):
        m = np.fromiter((match(s) for s in fl.string_t_decode(arrays[col])), dtype=bool)
        price = arrays[C_PRICE].view(fl.NP_DTYPE[t.schema()[C_PRICE][1]])
        n += len(m)
        rows += int(m.sum())
        total += int(price[m].sum())
    return [rows, total if rows else None], n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="generator threads")
    ap.add_argument("--host-rowgroups", type=int, default=32, help="row groups the host arm scans (0: skip the arm)")
    ap.add_argument("--note", default="", help="a line about the run (the machine lease) copied into the output")
    a = ap.parse_args()
    fl = pkgload.load()
    fd, path = tempfile.mkstemp(suffix=".fls", dir=os.environ.get("TMPDIR", "/tmp"))
    os.close(fd)
    try:
        fl.gen_image("lineitem_full", a.scale, 0, 0, None, a.threads).write(path)
        conn = fl.Connection([0])
        t = conn.read_fls(path)
        sch = t.schema()
        assert [sch[c][0] for c in (C_PRICE, C_INSTR, C_COMMENT)] == ["l_extendedprice", "l_shipinstruct", "l_comment"]
        nrows = t.nrows
        print(f"# lineitem_full SF{a.scale:g}: {nrows} rows, {t.nrowgroups} row groups, {os.path.getsize(path) / 1e9:.3f} GB "
              f"file, 1 GPU, {a.reps} repetitions per arm after one warm-up each, arms alternating; "
              f"count(*), sum(l_extendedprice)")
        if a.note:
            print(f"# {a.note}")
        floor = lambda: t.aggregate(AGGS)                                         # noqa: E731
        want_c = floor()
        hrg = min(a.host_rowgroups, t.nrowgroups)
        print("| filter | selectivity | A pushed down LIKE | E pushed down = | C no filter | A - C | A - E | "
              f"B host (first {hrg} row groups) | B scaled to the table | B scaled / A | row groups pruned |")
        print("|---|---|---|---|---|---|---|---|---|---|---|")
        detail = []
        for text, col, pat, match, eq_const in FILTERS:
            filt = [(col, "like", pat)]
            fa = lambda: t.aggregate(AGGS, filt=filt)                             # noqa: E731
            fe = lambda: t.aggregate(AGGS, filt=[(col, "=", eq_const)])           # noqa: E731
            want_a, want_e = fa(), fe()
            ta, te, tc = [], [], []
            for _ in range(max(1, a.reps)):
                s, out = timed(fa)
                assert out == want_a, (text, out, want_a)
                ta.append(s)
                pruned = t.pruned
                s, out = timed(fe)
                assert out == want_e, text
                te.append(s)
                s, out = timed(floor)
                assert out == want_c, text
                tc.append(s)
            ma, me, mc = (statistics.median(x) for x in (ta, te, tc))
            if hrg:
                host_arm(fl, t, col, match, min(2, hrg))                          # warm-up
                tb, (want_b, nb) = timed(lambda: host_arm(fl, t, col, match, hrg))
                got = t.aggregate(AGGS, filt=filt, rg_end=hrg)
                if got != want_b:
                    raise SystemExit(f"{text}: the arms disagree over {hrg} row groups: pushed down {got}, host {want_b}")
                scaled = tb * nrows / nb
                btxt = f"{1e3 * tb:.0f} ms | {scaled:.1f} s | {scaled / ma:.0f}"
            else:
                btxt = "- | - | -"
            print(f"| {text} | {want_a[0] / nrows:.4f} | {1e3 * ma:.2f} ms | {1e3 * me:.2f} ms | {1e3 * mc:.2f} ms | "
                  f"{1e3 * (ma - mc):+.2f} ms | {1e3 * (ma - me):+.2f} ms | {btxt} | {pruned} |")
            detail.append(f"# {text}: answer {want_a}; = {eq_const!r} answer {want_e}; A all "
                          f"{' '.join(f'{1e3 * x:.2f}' for x in ta)} ms; E all {' '.join(f'{1e3 * x:.2f}' for x in te)} ms; "
                          f"C all {' '.join(f'{1e3 * x:.2f}' for x in tc)} ms")
        print("\n".join(detail))
        bytes_res, _ = fl.Connection.resident_info(0)
        print(f"# resident image {bytes_res / 1e9:.3f} GB; unfiltered answer {want_c}; the pushed-down and the host "
              f"answers were equal over the host arm's row groups")
        t.close()
        conn.close()
    finally:
        os.unlink(path)


if __name__ == "__main__":
    main()
