#!/usr/bin/env python3
"""Value maps and key maps built on the GPU from a filtered scan (DESIGN.md
section 32) against the parent's host build of the same maps.

Workloads: lineitem (default SF10) from the seeded generator, and three
dimension tables at the TPC-H cardinalities of the same scale factor, built
with numpy and write_image because csrc/fls_gen.hpp generates lineitem only
(orders: o_orderkey as in lineitem's key space (4 of every 32 numbers unused),
o_custkey uniform, o_orderdate uniform over the TPC-H range; partsupp-like:
ps_partkey 1..200000 SF unique, a cost; supplier: s_suppkey unique, a nation
code 0..24).  All four are written to files once; every arm is a process of
its own that opens the files on one GPU, makes one warm-up call per query
(after which the compressed images are resident in HBM) and --reps timed ones
(medians and spread, max - min, of the host clock around the synchronous
Python call).  The processes run one after the other, alternating:

  A   Table.valuemap / Table.keymap of this build (fls_valuemap_from_scan,
      fls_keymap_from_scan)
  B   the same calls on the parent commit's package (--parent-pkg DIR, a built
      copy of its package directory): a filtered scan of both columns,
      np.concatenate, fls_valuemap_create / fls_keymap_create

Queries, fixed before the first run:

  orders   o_orderkey -> o_custkey, unfiltered (the Q10 build side)
  odate    ... under o_orderdate in [1994-01-01, 1995-01-01) (the Q3 / Q10 date range)
  cost     ps_partkey -> cost, unique keys (Q9's shape)
  lsupp    l_orderkey -> l_suppkey on lineitem under l_linenumber = 1: a sorted fact-side key
  nation   key map s_suppkey -> nation code (25 codes)

Every arm also times, on its build, calls this change does not touch: Q6, Q1
grouped and one mapped call (mapcol_rate's Q10 shape: aggregate_hashed by
cust[l_orderkey] under l_returnflag = 'R').  For A the split of a call into
scan, compact + D2H and host finish is what FLS_SCAN_PROFILE=1 prints
(--profile makes one extra process with it set).

    python scripts/valuemap_build_rate.py --scale 10 --reps 5 --parent-pkg ../parent/duckdb-fastlane_amd \\
        > profiles/valuemap/valuemap_build_sf10.txt
"""
import argparse
import importlib.util
import json
import os
import shutil
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
QUERIES = ["orders", "odate", "cost", "lsupp", "nation"]
OTHERS = ["Q6", "Q1", "Q10map"]
BYTES = {"orders": 8 + 4, "odate": 8 + 4, "cost": 4 + 8, "lsupp": 8 + 4, "nation": 4 + 1}  # B: key + value per selected row


def load_pkg(pkg_dir, name):
    spec = importlib.util.spec_from_file_location(name, Path(pkg_dir) / "__init__.py",
                                                  submodule_search_locations=[str(pkg_dir)])
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def write_dims(fl, scale, d):
    """the dimension tables at the TPC-H cardinalities, numpy + write_image"""
    rng = np.random.default_rng(10)
    no = int(1_500_000 * scale)
    i = np.arange(no, dtype=np.int64)
    okey = (i // 8) * 32 + i % 8 + 1                                   # the sparse o_orderkey of dbgen
    cust = rng.integers(1, int(150_000 * scale) + 1, no).astype(np.int32)
    odate = rng.integers(8035, 10441, no).astype(np.int32)             # 1992-01-01 .. 1998-08-02
    fl.write_image([("o_orderkey", fl.INT64, okey, fl.ENC_AUTO), ("o_custkey", fl.INT32, cust, fl.ENC_AUTO),
                    ("o_orderdate", fl.DATE, odate, fl.ENC_AUTO)]).write(str(d / "orders.fls"))
    npart = int(200_000 * scale)
    fl.write_image([("ps_partkey", fl.INT32, np.arange(1, npart + 1, dtype=np.int32), fl.ENC_AUTO),
                    ("cost", fl.INT64, rng.integers(100, 100_001, npart).astype(np.int64), fl.ENC_AUTO)]
                   ).write(str(d / "partsupp.fls"))
    ns = int(10_000 * scale)
    fl.write_image([("s_suppkey", fl.INT32, np.arange(1, ns + 1, dtype=np.int32), fl.ENC_AUTO),
                    ("nation", fl.INT8, rng.integers(0, 25, ns).astype(np.int8), fl.ENC_AUTO)]
                   ).write(str(d / "supplier.fls"))


def child(a):
    """one arm: every query on one build, one JSON line on stdout"""
    fl = load_pkg(a.pkg, "fls_arm")
    conn = fl.Connection([0])
    d = Path(a.dir)
    li, orders, ps, supp = (conn.read_fls(str(d / f)) for f in ("lineitem.fls", "orders.fls", "partsupp.fls",
                                                                  "supplier.fls"))
    col = {s[0]: c for c, s in enumerate(li.schema())}
    OKEY, SUPP, LNUM, QTY, PRICE, DISC, RFLAG, STATUS, SHIP = (col[n] for n in (
        "l_orderkey", "l_suppkey", "l_linenumber", "l_quantity", "l_extendedprice", "l_discount", "l_returnflag",
        "l_linestatus", "l_shipdate"))
    builds = {"orders": lambda: orders.valuemap(0, 1),
              "odate": lambda: orders.valuemap(0, 1, [(2, ">=", Y1994), (2, "<", Y1995)]),
              "cost": lambda: ps.valuemap(0, 1),
              "lsupp": lambda: li.valuemap(OKEY, SUPP, [(LNUM, "=", 1)]),
              "nation": lambda: supp.keymap(0, 1)}
    out = {"arm": a.child, "rows": {"lineitem": li.nrows, "orders": orders.nrows, "partsupp": ps.nrows,
                                    "supplier": supp.nrows}, "times": {}, "maps": {}, "info": {}}
    for q in QUERIES:
        times = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            m = builds[q]()
            dt = time.perf_counter() - t0
            i = m.info
            desc = [int(getattr(i, n)) for n, _ in i._fields_]
            assert out["maps"].setdefault(q, desc) == desc, (q, desc)
            bi = getattr(m, "build_info", None)
            if bi is not None:
                out["info"][q] = {n: int(getattr(bi, n)) for n, _ in bi._fields_}
            m.close()
            if rep:
                times.append(dt)
            print(f"{a.child} {q} {'warm-up' if not rep else rep} {1e3 * dt:.1f} ms", file=sys.stderr, flush=True)
        out["times"][q] = times
    # the calls this change does not touch
    custmap = orders.valuemap(0, 1)
    rev = ("sum_expr", [(0, 1, PRICE), (100, -1, DISC)])
    q10 = lambda g: [g.key_values[0].tolist(), g.lo[0].tolist(), g.count[1].tolist()]  # noqa: E731
    calls = {
        "Q6": lambda: li.aggregate([("sum_product", PRICE, DISC), ("count",)],
                                   [(SHIP, ">=", Y1994), (SHIP, "<", Y1995), (DISC, ">=", 5), (DISC, "<=", 7), (QTY, "<", 2400)]),
        "Q1": lambda: li.aggregate_grouped([RFLAG, STATUS], [("sum", QTY), ("sum", PRICE), rev, ("sum", DISC), ("count",)],
                                           [(SHIP, "<=", Q1_DAY)]),
        "Q10map": lambda: q10(li.aggregate_hashed([fl.Mapped(OKEY, custmap)], [rev, ("count",)], 1 << 22,
                                                  [(RFLAG, "=", "R")], order_by=(0, "desc"), limit=20)),
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
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1, help="how often the pair of arms runs (A B A B ...)")
    ap.add_argument("--threads", type=int, default=16, help="generator threads")
    ap.add_argument("--parent-pkg", default="", help="the parent commit's built package directory (arm B)")
    ap.add_argument("--note", default="", help="a line about the run copied into the output")
    ap.add_argument("--profile", action="store_true", help="after the arms, one process of A under FLS_SCAN_PROFILE=1")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--pkg", default="", help=argparse.SUPPRESS)
    ap.add_argument("--dir", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    sys.path.insert(0, str(ROOT))
    import pkgload
    fl = pkgload.load()
    d = Path(tempfile.mkdtemp(dir=os.environ.get("TMPDIR", "/tmp")))
    try:
        fl.gen_image("lineitem", a.scale, 0, 0, None, a.threads).write(str(d / "lineitem.fls"))
        write_dims(fl, a.scale, d)
        print(f"# SF{a.scale:g}: lineitem from the generator, orders / partsupp-like / supplier from numpy + write_image "
              f"(fls_gen.hpp has no such tables), {sum(f.stat().st_size for f in d.iterdir()) / 1e9:.3f} GB of files, "
              f"1 GPU; every arm a process of its own, one warm-up and {a.reps} repetitions per query, host clock around "
              "the Python call", flush=True)
        if a.note:
            print(f"# {a.note}")
        head = str(pkgload.PKG_DIR)
        arms = [("A", head)] + ([("B", a.parent_pkg)] if a.parent_pkg else [])
        res = {}
        for r in range(a.rounds):
            for name, pkg in arms:
                cmd = [sys.executable, __file__, "--child", name, "--pkg", pkg, "--dir", str(d), "--reps", str(a.reps)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True)
                got = json.loads(p.stdout.strip().splitlines()[-1])
                if name in res:                                     # a later round: more repetitions of the same arm
                    assert got["maps"] == res[name]["maps"]
                    for k, v in got["times"].items():
                        res[name]["times"][k] += v
                else:
                    res[name] = got
                print(f"arm {name} round {r + 1} done", file=sys.stderr, flush=True)
        first = res["A"]
        print(f"# rows: {first['rows']}")
        for name in res:
            assert res[name]["maps"] == first["maps"], (name, res[name]["maps"], first["maps"])
        print("# every arm built the same maps (every fls_*_info field):")
        for q in QUERIES:
            print(f"#   {q}: {first['maps'][q]}")
        print("## the builds")
        print("| query | arm | median | spread (max - min) | all (ms) |")
        print("|---|---|---|---|---|")
        for q in QUERIES + OTHERS:
            for name in res:
                v = res[name]["times"][q]
                print(f"| {q} | {name} | {1e3 * statistics.median(v):.2f} ms | {1e3 * (max(v) - min(v)):.2f} ms | "
                      f"{' '.join(f'{1e3 * x:.1f}' for x in v)} |")
        print("## what crossed PCIe towards the host")
        print("| query | selected rows | keys | collecting span | scratch per GPU | A: d2h_bytes | B: key + value bytes per "
              "selected row |")
        print("|---|---|---|---|---|---|---|")
        for q in QUERIES:
            i = first["info"].get(q)
            if i is None:
                print(f"| {q} | (the gate sent A to the host route) | | | | | |")
                continue
            print(f"| {q} | {i['rows_selected']} | {i['keys']} | {i['span'] + 1} | {i['scratch_bytes']} B | "
                  f"{i['d2h_bytes']} B | {BYTES[q] * i['rows_selected']} B |")
        for k in OTHERS:
            assert len({res[n]["answers"][k] for n in res}) == 1, k
        print("# Q6, Q1 and Q10map returned the same values on every arm")
        if a.profile:
            cmd = [sys.executable, __file__, "--child", "A-profile", "--pkg", head, "--dir", str(d), "--reps", "1"]
            p = subprocess.run(cmd, env={**os.environ, "FLS_SCAN_PROFILE": "1"}, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, text=True, check=True)
            print("## A under FLS_SCAN_PROFILE=1 (a process of its own; per call, in the order orders, odate, cost, lsupp, "
                  "nation, each twice, then orders once more)")
            for line in p.stderr.splitlines():
                if "map build:" in line:
                    print("# " + line.strip())
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
