#!/usr/bin/env python3
"""Key sets built on the GPU from a filtered scan
against the parent's host build of the same sets.

Workload: lineitem (default SF10) written to a file once; every arm is a
process of its own that opens the file on one GPU, makes one warm-up call per
query (after which the compressed image is resident in HBM) and --reps timed
ones (medians and spread, max - min, of the host clock around the synchronous
call).  The processes run one after the other, alternating between the builds:

  A      Table.keyset of this build (fls_keyset_from_scan)
  B      the same calls on the parent commit's package (--parent-pkg DIR, a
         built copy of its package directory): a filtered scan of the key
         column, np.unique, fls_keyset_create
  A-nw   A with FLS_KEYSET_BUILD_WINDOW=0: no LDS window, one global atomic per row

Queries, fixed before the first run:

  okey    l_orderkey, unfiltered (sorted, about four rows per key)
  q3      l_orderkey under l_orderkey < the key a third into the table AND l_shipdate < 1994-08-23 (day 9000):
          the build of section 21's Q3 shape
  part    l_partkey, unfiltered (unsorted, 30 rows per key)
  supp    l_suppkey, unfiltered (unsorted, 600 rows per key)
  okset   l_orderkey under l_orderkey IN (the keys with key % 5 < 2)

Every arm also times, on its build, the calls this change does not touch: Q6,
Q1 grouped and section 21's Q3 aggregate under the q3 set.  For A the split of
a call into scan, bitmap D2H and host finish is what FLS_SCAN_PROFILE=1 prints
(--profile makes one extra, untimed call per query with it set).

    python scripts/keyset_build_rate.py --scale 10 --reps 5 --parent-pkg ../parent/duckdb-fastlane_amd \\
        > profiles/keyset/keyset_build_sf10.txt
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
Y1994, Y1995 = 8766, 9131           # 1994-01-01 and 1995-01-01
Q1_DAY = 10471                      # 1998-09-02
Q3_DAY = 9000
QUERIES = ["okey", "q3", "part", "supp", "okset"]
OTHERS = ["Q6", "Q1", "Q3agg"]


def load_pkg(pkg_dir, name):
    spec = importlib.util.spec_from_file_location(name, Path(pkg_dir) / "__init__.py",
                                                  submodule_search_locations=[str(pkg_dir)])
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def child(a):
    """one arm: every query on one build, one JSON line on stdout"""
    fl = load_pkg(a.pkg, "fls_arm")
    conn = fl.Connection([0])
    t = conn.read_fls(a.file)
    col = {s[0]: c for c, s in enumerate(t.schema())}
    OKEY, PART, SUPP, QTY, PRICE, DISC, TAX, RFLAG, STATUS, SHIP = (col[n] for n in (
        "l_orderkey", "l_partkey", "l_suppkey", "l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag",
        "l_linestatus", "l_shipdate"))
    nrows = t.nrows
    cut = int(fl.gen_values("lineitem", OKEY, nrows // 3, 1, np.int64, a.scale)[0])
    lo, hi = t.zonemap(0, OKEY)[0], t.zonemap(t.nrowgroups - 1, OKEY)[1]
    keys = np.arange(lo, hi + 1, dtype=np.int64)
    some = conn.keyset(keys[keys % 5 < 2])
    del keys
    q3 = [(OKEY, "<", cut), (SHIP, "<", Q3_DAY)]
    builds = {"okey": (OKEY, None), "q3": (OKEY, q3), "part": (PART, None), "supp": (SUPP, None),
              "okset": (OKEY, [(OKEY, "in_set", some)])}
    out = {"arm": a.child, "nrows": nrows, "nrg": t.nrowgroups, "times": {}, "sets": {}, "info": {}}
    for q in QUERIES:
        c, filt = builds[q]
        times = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            ks = t.keyset(c, filt)
            dt = time.perf_counter() - t0
            i = ks.info
            desc = [int(i.count), int(i.form), int(i.device_bytes), int(i.min), int(i.max), int(i.max_probe)]
            assert out["sets"].setdefault(q, desc) == desc, (q, desc)
            bi = getattr(ks, "build_info", None)
            if bi is not None:
                out["info"][q] = {n: int(getattr(bi, n)) for n, _ in bi._fields_}
            ks.close()
            if rep:
                times.append(dt)
            print(f"{a.child} {q} {'warm-up' if not rep else rep} {1e3 * dt:.1f} ms", file=sys.stderr, flush=True)
        out["times"][q] = times
    # the calls this change does not touch
    ks3 = t.keyset(OKEY, q3)
    rev = ("sum_expr", [(0, 1, PRICE), (100, -1, DISC)])
    calls = {
        "Q6": lambda: t.aggregate([("sum_product", PRICE, DISC), ("count",)],
                                  [(SHIP, ">=", Y1994), (SHIP, "<", Y1995), (DISC, ">=", 5), (DISC, "<=", 7), (QTY, "<", 2400)]),
        "Q1": lambda: t.aggregate_grouped([RFLAG, STATUS], [("sum", QTY), ("sum", PRICE), rev, ("sum", DISC), ("count",)],
                                          [(SHIP, "<=", Q1_DAY)]),
        "Q3agg": lambda: t.aggregate([("count",), ("sum", PRICE)], [(OKEY, "in_set", ks3), (SHIP, ">=", Q3_DAY)]),
    }
    out["answers"] = {}
    for k, fn in calls.items():
        times = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            got = fn()
            dt = time.perf_counter() - t0
            if rep:
                times.append(dt)
        out["times"][k] = times
        out["answers"][k] = repr(got)
    t.close()
    conn.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="generator threads")
    ap.add_argument("--parent-pkg", default="", help="the parent commit's built package directory (arm B)")
    ap.add_argument("--note", default="", help="a line about the run copied into the output")
    ap.add_argument("--profile", action="store_true", help="after the arms, one process of A under FLS_SCAN_PROFILE=1")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--pkg", default="", help=argparse.SUPPRESS)
    ap.add_argument("--file", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    sys.path.insert(0, str(ROOT))
    import pkgload
    fl = pkgload.load()
    fd, path = tempfile.mkstemp(suffix=".fls", dir=os.environ.get("TMPDIR", "/tmp"))
    os.close(fd)
    try:
        fl.gen_image("lineitem", a.scale, 0, 0, None, a.threads).write(path)
        print(f"# lineitem SF{a.scale:g}, {os.path.getsize(path) / 1e9:.3f} GB file, 1 GPU; every arm a process of its "
              f"own, one warm-up and {a.reps} repetitions per query, host clock around Table.keyset", flush=True)
        if a.note:
            print(f"# {a.note}")
        head = str(pkgload.PKG_DIR)
        arms = [("A", head, {})]
        if a.parent_pkg:
            arms.append(("B", a.parent_pkg, {}))
        arms.append(("A-nw", head, {"FLS_KEYSET_BUILD_WINDOW": "0"}))
        res = {}
        for name, pkg, env in arms:
            cmd = [sys.executable, __file__, "--child", name, "--pkg", pkg, "--file", path, "--scale", str(a.scale),
                   "--reps", str(a.reps)]
            r = subprocess.run(cmd, env={**os.environ, **env}, stdout=subprocess.PIPE, text=True, check=True)
            res[name] = json.loads(r.stdout.strip().splitlines()[-1])
            print(f"arm {name} done", file=sys.stderr, flush=True)
        first = res["A"]
        print(f"# {first['nrows']} rows, {first['nrg']} row groups")
        for name in res:
            assert res[name]["sets"] == first["sets"], (name, res[name]["sets"], first["sets"])
        print("# every arm built the same sets (count, form, device bytes, min, max, max_probe):")
        for q in QUERIES:
            print(f"#   {q}: {first['sets'][q]}")
        print("## the builds")
        print("| query | arm | median | spread (max - min) | all (ms) |")
        print("|---|---|---|---|---|")
        for q in QUERIES + OTHERS:
            for name in res:
                v = res[name]["times"][q]
                print(f"| {q} | {name} | {1e3 * statistics.median(v):.2f} ms | {1e3 * (max(v) - min(v)):.2f} ms | "
                      f"{' '.join(f'{1e3 * x:.1f}' for x in v)} |")
        print("## what crossed PCIe towards the host")
        print("| query | rows that set a bit | collecting span | bitmap | A: d2h_bytes | B: 8 or 4 bytes per selected row |")
        print("|---|---|---|---|---|---|")
        width = {"okey": 8, "q3": 8, "okset": 8, "part": 4, "supp": 4}
        for q in QUERIES:
            i = first["info"][q]
            print(f"| {q} | {i['rows_selected']} | {i['span'] + 1} | {i['bitmap_bytes']} B | {i['d2h_bytes']} B | "
                  f"{width[q] * i['rows_selected']} B |")
        for k in OTHERS:
            assert len({res[n]["answers"][k] for n in res}) == 1, k
        print("# Q6, Q1 and Q3agg returned the same values on every arm")
        if a.profile:
            cmd = [sys.executable, __file__, "--child", "A-profile", "--pkg", head, "--file", path, "--scale", str(a.scale),
                   "--reps", "1"]
            r = subprocess.run(cmd, env={**os.environ, "FLS_SCAN_PROFILE": "1"}, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, text=True, check=True)
            print("## A under FLS_SCAN_PROFILE=1 (a process of its own; per call, in the order okey, q3, part, supp, okset, "
                  "each twice)")
            for line in r.stderr.splitlines():
                if "keyset build" in line:
                    print("# " + line.strip())
    finally:
        os.unlink(path)


if __name__ == "__main__":
    main()
