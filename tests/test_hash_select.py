"""Choosing among a hash aggregate's groups on the GPU: HAVING terms and
ORDER BY one aggregate LIMIT k (fls_aggregate_hashed_select /
Table.aggregate_hashed(having=, order_by=, limit=); csrc/fls_hashsel.hip).

Expected values come from the inputs: tests/test_hash_aggregate.py's py_groups
over the arrays handed to write_image (FLOAT / DOUBLE MIN / MAX recomputed here
in the filter's float order, which Python's min / max do not follow), then the
selection in plain Python with exact integers: a NULL aggregate satisfies no
term, floats compare with NaN equal to NaN and above every number and -0 equal
to 0, and the result order is (NULL placement, value, first row).  Everything
compares exactly.

CPU tests: the exported symbols, every argument error, the call that passes
its checks and fails on the missing GPU, the all-pruned call and its
statistics, the kernels' resources.  GPU tests: every op against every kind of
value, conjunctions and the two extremes, ORDER BY / LIMIT through a merge
tree of two levels, with a filter and a row-group range, reproducibility
across batch sizes, slots and pipelines with the several-pipeline fallback, the
limit, and the Q18 and Q3 shapes."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import filter_mask
from test_group_aggregate import C_DISC, C_OKEY, C_PRICE, C_QTY, C_SHIPDATE
from test_hash_aggregate import (D3, MANY_AGGS, N1, RG, accepted, conn0, lineitem, many,  # noqa: F401 (fixtures)
                                 py_groups)

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "duckdb-fastlane_amd" / "libflsgpu.so"

ERR_ARG, ERR_DEVICE, ERR_LIMIT = -3, -4, -8
OPS = {"=": lambda c: c == 0, "!=": lambda c: c != 0, "<": lambda c: c < 0, "<=": lambda c: c <= 0,
       ">": lambda c: c > 0, ">=": lambda c: c >= 0}


# ------------------------------------------------------------ expected values
def fcmp(a, b):
    """the filter's float order: NaN equals NaN and sits above every number, -0 equals 0"""
    na, nb = a != a, b != b
    if na or nb:
        return 0 if na == nb else (1 if na else -1)
    return (a > b) - (a < b)


def groups(cols, valid, keys, aggs, sel, first_row=0):
    """py_groups, with FLOAT / DOUBLE MIN / MAX in the filter's float order"""
    flt = [j for j, a in enumerate(aggs) if a[0] in ("min", "max") and cols[a[1]].dtype.kind == "f"]
    want = py_groups(cols, valid, keys, [("count", a[1]) if j in flt else a for j, a in enumerate(aggs)], sel,
                     first_row)
    every = np.ones(len(sel), bool)
    kc = [cols[c].tolist() for c in keys]
    kv = [valid.get(c, every).tolist() for c in keys]
    for j in flt:
        op, c = aggs[j]
        x, ok = cols[c].tolist(), valid.get(c, every).tolist()
        best = {}
        for i in np.nonzero(sel)[0].tolist():
            if not ok[i]:
                continue
            key = tuple(col[i] if v[i] else None for col, v in zip(kc, kv))
            if key not in best or fcmp(x[i], best[key]) == (-1 if op == "min" else 1):
                best[key] = x[i]
        for key, (_, vals) in want.items():
            vals[j] = best.get(key)
    return want


def holds(v, op, c):
    if v is None:
        return False
    if isinstance(v, float):
        return OPS[op](fcmp(v, float(c)))
    return OPS[op]((v > c) - (v < c))


def order_of(order_by):
    ob = tuple(order_by) if isinstance(order_by, (tuple, list)) else (order_by,)
    return ob[0], len(ob) > 1 and ob[1] == "desc", len(ob) > 2


def select(want, having=None, order_by=None, limit=None):
    """(the chosen [(key, first row, values)], in result order where there is
    one, else by first row; the groups that pass HAVING)"""
    rows = [(k, f, v) for k, (f, v) in want.items() if all(holds(v[a], op, c) for a, op, c in having or ())]
    passed = len(rows)
    rows.sort(key=lambda r: r[1])
    if order_by is not None:
        a, desc, nulls_first = order_of(order_by)

        def key(r):
            v = r[2][a]
            if v is None:
                return (0 if nulls_first else 1, 0, r[1])
            if isinstance(v, float):
                k = (1, 0.0) if v != v else (0, v + 0.0)
                k = (-k[0], -k[1]) if desc else k
            else:
                k = -v if desc else v
            return (1 if nulls_first else 0, k, r[1])
        rows.sort(key=key)
    if limit:
        rows = rows[:limit]
    return rows, passed


def norm(rows):
    def one(v):
        return "nan" if isinstance(v, float) and v != v else (v + 0.0 if isinstance(v, float) else v)
    return [(k, f, [one(x) for x in v]) for k, f, v in rows]


def got_rows(h):
    return [(k, int(f), v) for (k, v), f in zip(h.to_list(ordered=False), h.first_row.tolist())]


def check(h, want, having=None, order_by=None, limit=None, what=""):
    rows, passed = select(want, having, order_by, limit)
    what = (what, having, order_by, limit)
    got = got_rows(h)
    assert (h.groups_total, h.groups_passed, len(h)) == (len(want), passed, len(rows)), what
    if order_by is None and not limit:
        got.sort(key=lambda r: r[1])
    else:   # the arrays and to_list() are in result order
        assert [k for k, _ in h.to_list()] == [k for k, _, _ in rows], what
    assert norm(got) == norm(rows), what
    return rows


# ------------------------------------------------------------------ CPU tests
def test_library_exports_the_select_call(_built):
    lib = C.CDLL(str(LIB))
    for name in ("fls_aggregate_hashed_select", "fls_hash_result_select_stats"):
        assert hasattr(lib, name), name


@pytest.fixture(scope="module")
def small(fl):
    n = 1500
    img = fl.write_image([("k", fl.INT32, np.arange(n, dtype=np.int32) % 300, fl.ENC_AUTO),
                          ("x", fl.INT64, np.arange(n, dtype=np.int64) - 700, fl.ENC_AUTO),
                          ("d", fl.DOUBLE, np.arange(n) % 7 * 0.5, fl.ENC_AUTO),
                          ("u", fl.UINT64, np.arange(n, dtype=np.uint64), fl.ENC_AUTO)], rowgroup=RG)
    t = fl.Connection([0]).read_image(img)
    yield t
    t.close()


SMALL_AGGS = [("count",), ("sum", 1), ("min", 2), ("max", 3)]


@pytest.mark.parametrize("kw,what", [
    (dict(having=[(0, ">", 1)] * 9), "having 8:"),                                   # nhaving > 8
    (dict(having=[(0, ">", 1), (4, ">", 1)]), "having 1:"),                          # an aggregate index >= n
    (dict(having=[(0, 6, 1)]), "having 0:"),                                         # FLS_CMP_IS_NULL
    (dict(having=[(1, "<", 5), (1, ">", 0), (3, 9, 1)]), "having 2:"),               # FLS_CMP_IN_SET
    (dict(having=[(0, ">", 1.5)]), "having 0:"),                                     # a float against a count
    (dict(having=[(1, ">", 0), (1, "=", 0.0)]), "having 1:"),                        # ... against an integer sum
    (dict(having=[(3, "<", 2.0)]), "having 0:"),                                     # ... against a UINT64 MAX
    (dict(having=[(2, ">", 1)]), "having 0:"),                                       # an int against a DOUBLE MIN
    (dict(order_by=1), "order:"),                                                    # an order without a limit
    (dict(order_by=(1, "desc"), limit=0), "order:"),
    (dict(order_by=(4, "desc"), limit=5), "order:"),                                 # an aggregate index >= n
    (dict(order_by=(0, "asc"), limit=1025), "order:"),
    (dict(limit=1025), "order:"),                                                    # a limit above 1024
    (dict(having=[(0, ">", 1)], limit=5000), "order:"),
])
def test_selection_argument_errors(fl, small, kw, what):
    with pytest.raises(fl.FlsError) as e:
        small.aggregate_hashed([0], SMALL_AGGS, 1000, **kw)
    assert e.value.code == ERR_ARG and what in e.value.msg, e.value
    # the grouping's own errors come first, with the plain call's messages
    with pytest.raises(fl.FlsError) as e:
        small.aggregate_hashed([0, 99], SMALL_AGGS, 1000, **kw)
    assert e.value.code == ERR_ARG and "key 1:" in e.value.msg, e.value


def test_python_argument_forms(fl, small):
    for kw in (dict(having=[(0, "is_null", 1)]), dict(having=[(0, "~", 1)]), dict(having=[(0, ">", 1 << 128)]),
               dict(order_by=(0, "down"), limit=1), dict(order_by=(0, "desc", "nulls_last"), limit=1)):
        with pytest.raises(ValueError):
            small.aggregate_hashed([0], SMALL_AGGS, 1000, **kw)


def test_a_selection_passes_the_checks_and_needs_a_gpu(fl, small):
    """every form of a valid selection gets past the argument checks; without a
    GPU the table cannot be allocated, and the error names its bytes"""
    for kw in (dict(having=[]), dict(having=[(0, ">", 2)]), dict(limit=1024), dict(order_by=0, limit=1),
               dict(having=[(1, "!=", -(1 << 127)), (1, "<=", (1 << 127) - 1), (2, ">=", float("nan")),
                            (3, "<", 1 << 64), (3, ">", -1), (0, "=", 5), (2, "<", -0.0), (1, ">", 0)],
                    order_by=(2, "desc", "nulls_first"), limit=7)):
        h = accepted(fl, lambda: small.aggregate_hashed([0], SMALL_AGGS, 1000, **kw))
        assert h is None or h.groups_total == 300
    # the table stays usable
    assert len(small.aggregate_hashed([0], SMALL_AGGS, 100, filt=[(1, "<", -5000)], having=[(0, ">", 0)])) == 0


def test_no_row_group_to_read_selects_nothing_without_a_gpu(fl, small):
    kw = dict(having=[(0, ">", 0), (1, "!=", 7)], order_by=(1, "desc"), limit=10)
    for h in (small.aggregate_hashed([0], SMALL_AGGS, 1000, filt=[(1, "<", -5000)], **kw),
              small.aggregate_hashed([0], SMALL_AGGS, 1000, rg_begin=1, rg_end=1, **kw),
              small.aggregate_hashed([0], SMALL_AGGS, 1000, rg_begin=1, rg_end=1)):
        assert len(h) == 0 and h.to_list() == [] and h.first_row.shape == (0,) and len(h.count) == 4
        assert (h.groups_total, h.groups_passed, h.selected_on_device) == (0, 0, False)


def test_select_kernel_resources():
    """each of the selection's kernels is there once, without scratch or spills"""
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    res = kernel_resources.resources(str(LIB))
    for kernel in ("group_select_kernel", "group_topk_kernel", "group_topk_merge_kernel", "group_gather_kernel"):
        hits = {k: v for k, v in res.items() if kernel in k}
        assert len(hits) == 1, (kernel, hits)
        for name, r in hits.items():
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)


# ------------------------------------------------------------------ GPU tests
# ---- 1. HAVING: every op against every kind of value
NG = 40


@pytest.fixture(scope="module")
def seltab(fl, conn0):
    rng = np.random.default_rng(20261020)
    n = N1
    i = np.arange(n)
    grp = rng.integers(0, NG, n)
    kv = rng.random(n) >= 0.05                                     # NULL keys: a group of its own
    k = (grp * 11 - 200).astype(np.int16)
    s = rng.integers(-1000, 1001, n).astype(np.int64)
    s[grp % 2 == 0] -= 600                                         # sums on both sides of 0
    # ~100 rows a group near +2^62, near -2^62, or both: the sums pass 2^64 upwards, downwards, or cancel
    sgn = np.where(grp % 3 == 0, 1, np.where(grp % 3 == 1, -1, np.where(i % 2 == 0, 1, -1)))
    v62 = ((np.int64(2**62) + rng.integers(0, 1 << 40, n)) * sgn).astype(np.int64)
    u64 = np.uint64(2**64 - 1) - rng.integers(0, 1 << 30, n).astype(np.uint64)
    m64 = rng.integers(-2**63, 2**63, n, dtype=np.int64)
    i32 = rng.integers(-2**31, 2**31, n).astype(np.int32)
    g = np.round(rng.normal(0, 10, n), 2)
    zero = grp < 6                                                 # groups of -0.0 and +0.0 alone
    g[zero] = np.array([0.0, -0.0])[rng.integers(0, 2, int(zero.sum()))]
    g[(grp >= 6) & (grp < 10) & (rng.random(n) < 0.3)] = np.nan    # groups with NaN
    g[(grp == 10) & (i % 3 == 0)] = np.inf
    g[(grp == 11) & (i % 3 == 0)] = -np.inf
    nv = grp % 7 != 3                                              # the operand is NULL on every row of these groups
    nx = rng.integers(-50, 50, n).astype(np.int32)
    img = fl.write_image([("k", fl.INT16, np.ma.array(k, mask=~kv), fl.ENC_AUTO), ("s", fl.INT64, s, fl.ENC_AUTO),
                          ("v62", fl.INT64, v62, fl.ENC_AUTO), ("u64", fl.UINT64, u64, fl.ENC_AUTO),
                          ("m64", fl.INT64, m64, fl.ENC_AUTO), ("i32", fl.INT32, i32, fl.ENC_AUTO),
                          ("g", fl.DOUBLE, g, fl.ENC_AUTO),
                          ("nx", fl.INT32, np.ma.array(nx, mask=~nv), fl.ENC_AUTO)], rowgroup=RG)
    t = conn0.read_image(img)
    cols, valid = {0: k, 1: s, 2: v62, 3: u64, 4: m64, 5: i32, 6: g, 7: nx}, {0: kv, 7: nv}
    want = groups(cols, valid, [0], SEL_AGGS, np.ones(n, bool))
    assert len(want) == NG + 1 and (None,) in want
    yield img, t, cols, valid, want
    t.close()


SEL_AGGS = [("count",), ("sum", 1), ("sum", 2), ("min", 4), ("max", 3), ("max", 5), ("min", 6), ("max", 6),
            ("sum", 7), ("count", 7), ("min", 7)]
A_COUNT, A_SUM, A_WIDE, A_MIN64, A_MAXU64, A_MAX32, A_MINF, A_MAXF, A_NULLSUM, A_NULLCNT, A_NULLMIN = range(11)
FLOAT_CONSTS = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 1.5]


def having_constants(agg, want):
    vals = sorted(v[agg] for _, v in want.values() if v[agg] is not None and v[agg] == v[agg])
    lo, mid, hi = vals[0], vals[len(vals) // 2], vals[-1]
    if agg in (A_MINF, A_MAXF):
        return FLOAT_CONSTS + [mid, lo, hi]
    near = [lo, mid, mid - 1, mid + 1, hi]
    if agg == A_COUNT:        # a count is never negative and holds 64 bits
        return near + [0, -1, 1 << 64, -(1 << 127)]
    if agg == A_SUM:          # constants on both sides of a negative and of a positive sum
        neg, pos = [v for v in vals if v < 0], [v for v in vals if v > 0]
        return near + [0, neg[0] - 1, neg[-1], neg[-1] + 1, pos[0] - 1, pos[0], pos[-1] + 1]
    if agg == A_WIDE:         # ... that differ from a group's sum in the high word only, or in the low word only
        assert lo < -2**64 and hi > 2**64
        return near + [mid + (1 << 64), mid - (1 << 64), lo + (1 << 64), hi - (1 << 64), hi - 1, lo + 1, 0,
                       (1 << 127) - 1, -(1 << 127)]
    if agg == A_MIN64:        # INT64 MIN: past the type on both sides
        return near + [-2**63, 2**63 - 1, 2**63, -2**63 - 1, 1 << 100]
    if agg == A_MAXU64:       # UINT64 MAX near 2^64: compares unsigned, the constant signed
        assert lo > 2**63
        return near + [2**64 - 1, 2**64, -1, 2**63, -(1 << 70)]
    if agg == A_MAX32:        # INT32 MAX: a constant outside INT32 holds always or never
        return near + [2**31 - 1, 2**31, -2**31 - 1, 2**63, -2**63 - 1, 1 << 64, -(1 << 64)]
    return near + [0]


@pytest.mark.gpu
@pytest.mark.parametrize("agg", range(len(SEL_AGGS)), ids=["count", "sum", "wide_sum", "min_i64", "max_u64", "max_i32",
                                                           "min_double", "max_double", "null_sum", "null_count",
                                                           "null_min"])
def test_gpu_having_every_op_and_value_kind(fl, gpu, seltab, agg):
    img, t, cols, valid, want = seltab
    null_groups = {k for k, (_, v) in want.items() if v[agg] is None}
    assert bool(null_groups) == (agg in (A_NULLSUM, A_NULLMIN))
    outcomes = set()
    for c in having_constants(agg, want):
        for op in OPS:
            h = t.aggregate_hashed([0], SEL_AGGS, 64, having=[(agg, op, c)])
            rows = check(h, want, [(agg, op, c)], what=SEL_AGGS[agg])
            assert h.selected_on_device
            # a group whose operand is NULL in every row fails every term, != included
            assert not null_groups & {k for k, _, _ in rows}
            outcomes.add(0 if not rows else (2 if len(rows) == len(want) - len(null_groups) else 1))
            if rows and len(rows) + len(null_groups) == len(want):
                assert (None,) in {k for k, _, _ in rows}       # the NULL-key group is selected like any other
    assert outcomes == {0, 1, 2}                                 # none, some and all of the groups passed


# ---- 2. conjunctions and the two extremes
@pytest.mark.gpu
def test_gpu_conjunctions_and_the_two_extremes(fl, gpu, seltab):
    img, t, cols, valid, want = seltab
    counts = sorted(v[A_COUNT] for _, v in want.values())
    cmid = counts[len(counts) // 2]
    for having in ([(A_COUNT, ">=", cmid), (A_SUM, "<", 0)],
                   [(A_WIDE, ">", 0), (A_MAXF, "<", float("nan"))],
                   [(A_COUNT, ">=", cmid), (A_SUM, "<", 0), (A_NULLSUM, "!=", 0)],
                   [(A_MAXU64, ">", 2**63), (A_MIN64, "<", 0), (A_MINF, "<", 0.0)],
                   [(A_NULLCNT, "=", 0), (A_COUNT, ">", 0)],
                   [(A_NULLCNT, "=", 0), (A_NULLMIN, "<", 100)],       # count 0 means NULL: nothing passes
                   [(a, "!=", 0.5 if a in (A_MINF, A_MAXF) else -7) for a in range(8)]):
        rows = check(t.aggregate_hashed([0], SEL_AGGS, 64, having=having), want, having)
        assert 0 < len(rows) < len(want) or having[0][0] == A_NULLCNT or len(having) == 8, having
    # no group passes: zero groups, and the groups were formed
    h = t.aggregate_hashed([0], SEL_AGGS, 64, having=[(A_COUNT, ">", 0), (A_COUNT, "<", 0)])
    assert len(h) == 0 and h.groups_total == len(want) > 0 and h.groups_passed == 0 and h.to_list() == []
    assert h.selected_on_device
    # every group passes: the plain call's set exactly
    plain = t.aggregate_hashed([0], SEL_AGGS, 64)
    every = t.aggregate_hashed([0], SEL_AGGS, 64, having=[(A_COUNT, ">", 0), (A_MAXU64, ">=", 0)])
    check(every, want, [(A_COUNT, ">", 0)])
    assert norm(sorted(got_rows(every), key=lambda r: r[1])) == norm(sorted(got_rows(plain), key=lambda r: r[1]))
    assert every.groups_passed == every.groups_total == len(plain) == len(want)
    # the plain call's statistics, and an empty selection is the plain call
    assert (plain.groups_total, plain.groups_passed, plain.selected_on_device) == (len(want), len(want), False)
    empty = t.aggregate_hashed([0], SEL_AGGS, 64, having=[])
    assert norm(sorted(got_rows(empty), key=lambda r: r[1])) == norm(sorted(got_rows(plain), key=lambda r: r[1]))
    assert not empty.selected_on_device and len(empty.to_list()) == len(plain.to_list())


# ---- 3. ORDER BY / LIMIT
DO = 2500                      # three lists of at most 1024 candidates: a merge tree of two levels, an odd list count
ORD_AGGS = [("count",), ("sum", 2), ("sum", 3), ("min", 1), ("max", 3)]
O_COUNT, O_TIE, O_SUM, O_ID, O_MAX = range(5)


@pytest.fixture(scope="module")
def ordtab(fl, conn0):
    rng = np.random.default_rng(99)
    n = 3 * RG
    ident = np.concatenate([np.arange(DO), rng.integers(0, DO, n - DO)])[rng.permutation(n)]
    k = (ident * 37 - 50000).astype(np.int32)
    tie = rng.integers(0, 3, n).astype(np.int8)                    # hundreds of groups share each sum
    x = rng.integers(-10**6, 10**6, n).astype(np.int64)
    img = fl.write_image([("k", fl.INT32, k, fl.ENC_AUTO), ("id", fl.INT32, ident.astype(np.int32), fl.ENC_AUTO),
                          ("tie", fl.INT8, tie, fl.ENC_AUTO), ("x", fl.INT64, x, fl.ENC_AUTO)], rowgroup=RG)
    t = conn0.read_image(img)
    cols = {0: k, 1: ident.astype(np.int32), 2: tie, 3: x}
    want = groups(cols, {}, [0], ORD_AGGS, np.ones(n, bool))
    assert len(want) == DO
    yield img, t, cols, want
    t.close()


ORD_CASES = [dict(order_by=(a, d), limit=k) for a in (O_TIE, O_SUM) for d in ("asc", "desc") for k in (1, 7, 1024)] + [
    # exactly 1,024 and 1,025 passing groups; a k larger than the number of passing groups
    dict(having=[(O_ID, "<", 1024)], order_by=(O_SUM, d), limit=1024) for d in ("asc", "desc")] + [
    dict(having=[(O_ID, "<=", 1024)], order_by=(O_TIE, d), limit=k) for d in ("asc", "desc") for k in (1024, 7)] + [
    dict(having=[(O_ID, "<", 500)], order_by=(O_TIE, d), limit=1024) for d in ("asc", "desc")] + [
    dict(having=[(O_ID, ">=", 2400), (O_COUNT, "=", 1)], order_by=(O_COUNT, "desc"), limit=1024),
    dict(order_by=O_COUNT, limit=1024), dict(order_by=(O_MAX, "desc"), limit=7),
    # a limit without an order: the first k groups by first row
    dict(limit=1), dict(limit=7), dict(limit=1024), dict(having=[(O_TIE, "=", 1)], limit=1024),
    dict(having=[(O_ID, "<", 1025)], limit=1024), dict(having=[(O_ID, "<", 3)], limit=7)]


def run_ordtab(t, want=None):
    out = []
    for kw in ORD_CASES:
        h = t.aggregate_hashed([0], ORD_AGGS, DO, **kw)
        if want is not None:
            check(h, want, **kw)
        out.append((got_rows(h), h.groups_total, h.groups_passed))
    return out


@pytest.mark.gpu
def test_gpu_order_by_and_limit_through_the_merge_tree(fl, gpu, ordtab):
    img, t, cols, want = ordtab
    ties = [v[O_TIE] for _, v in want.values()]
    assert min(ties.count(s) for s in (0, 1, 2)) > 300            # the first row decides among hundreds
    assert select(want, [(O_ID, "<", 1024)])[1] == 1024 and select(want, [(O_ID, "<=", 1024)])[1] == 1025
    run_ordtab(t, want)
    h = t.aggregate_hashed([0], ORD_AGGS, DO, order_by=(O_TIE, "desc"), limit=1024)
    assert h.selected_on_device and h.groups_passed == DO and len(h) == 1024
    # in both directions equal sums come by first row ascending
    for d in ("asc", "desc"):
        h = t.aggregate_hashed([0], ORD_AGGS, DO, order_by=(O_TIE, d), limit=700)
        s, f = h.lo[O_TIE].tolist(), h.first_row.tolist()
        assert all((s[j] < s[j + 1]) if s[j] != s[j + 1] and d == "asc" else (s[j] > s[j + 1]) if s[j] != s[j + 1]
                   else f[j] < f[j + 1] for j in range(len(s) - 1))


SEL_ORD_CASES = [dict(order_by=(a, d) + nf, limit=k)
                 for a in (A_WIDE, A_MAXF, A_MINF, A_NULLSUM, A_NULLMIN, A_MAXU64, A_MIN64, A_NULLCNT)
                 for d in ("asc", "desc") for nf in ((), ("nulls_first",)) for k in (7, 1024)] + [
    dict(having=[(A_NULLCNT, "=", 0)], order_by=(A_NULLSUM, "desc"), limit=3),     # NULLs alone
    dict(having=[(A_MAXF, "=", float("nan"))], order_by=(A_MAXF, "asc"), limit=9),
    dict(having=[(A_SUM, "<", 0)], order_by=A_SUM, limit=5), dict(having=[(A_SUM, "<", 0)], limit=5)]


def run_seltab(t, want=None):
    out = []
    for kw in SEL_ORD_CASES:
        h = t.aggregate_hashed([0], SEL_AGGS, 64, **kw)
        if want is not None:
            check(h, want, **kw)
        out.append((norm(got_rows(h)), h.groups_total, h.groups_passed))
    return out


@pytest.mark.gpu
def test_gpu_order_by_floats_nulls_and_wide_sums(fl, gpu, seltab, conn0):
    img, t, cols, valid, want = seltab
    assert sum(1 for _, v in want.values() if v[A_MAXF] != v[A_MAXF]) >= 4        # NaN groups: the largest value
    assert sum(1 for _, v in want.values() if v[A_NULLSUM] is None) >= 5
    run_seltab(t, want)
    first = t.aggregate_hashed([0], SEL_AGGS, 64, order_by=(A_NULLSUM, "desc", "nulls_first"), limit=7).to_list()
    last = t.aggregate_hashed([0], SEL_AGGS, 64, order_by=(A_NULLSUM, "desc"), limit=1024).to_list()
    assert all(v[A_NULLSUM] is None for _, v in first[:5]) and first[0][1][A_NULLSUM] is None
    assert last[0][1][A_NULLSUM] is not None and last[-1][1][A_NULLSUM] is None and len(last) == len(want)
    top = t.aggregate_hashed([0], SEL_AGGS, 64, order_by=(A_MAXF, "desc"), limit=4).to_list()
    assert all(v[A_MAXF] != v[A_MAXF] for _, v in top)
    # 128-bit sums that differ only in the high word: group g holds 2 (g % 5 + 1) rows of 2^63
    rows = np.concatenate([np.full(2 * (g % 5 + 1), g) for g in range(30)])
    u = np.full(len(rows), 2**63, dtype=np.uint64)
    t2 = conn0.read_image(fl.write_image([("k", fl.INT8, rows.astype(np.int8), fl.ENC_AUTO),
                                          ("u", fl.UINT64, u, fl.ENC_AUTO)], rowgroup=RG))
    try:
        aggs = [("sum", 1), ("count",)]
        w2 = groups({0: rows.astype(np.int8), 1: u}, {}, [0], aggs, np.ones(len(rows), bool))
        assert {v[0] for _, v in w2.values()} == {m << 64 for m in range(1, 6)}
        for kw in (dict(order_by=(0, "desc"), limit=8), dict(order_by=0, limit=8), dict(order_by=0, limit=1024),
                   dict(having=[(0, ">", 2 << 64)], order_by=(0, "desc"), limit=1024),
                   dict(having=[(0, "<=", 3 << 64), (0, "!=", 1 << 64)]), dict(having=[(0, "=", (4 << 64) + 1)]),
                   dict(having=[(0, ">=", (4 << 64) + 1)]), dict(having=[(0, "<", (2 << 64) - 1)], limit=2)):
            check(t2.aggregate_hashed([0], aggs, 32, **kw), w2, **kw)
    finally:
        t2.close()


# ---- 4. with a filter and a row-group range
@pytest.mark.gpu
def test_gpu_selection_under_a_filter_and_a_row_group_range(fl, gpu, conn0):
    # test_gpu_filtered_out_and_tail_rows_make_no_group's table
    rng = np.random.default_rng(5)
    n = N1
    f = rng.integers(0, 2, n).astype(np.int8)
    k = np.where(f == 1, rng.integers(1, 400, n), rng.integers(1000, 1400, n)).astype(np.int32)
    kv = rng.random(n) >= 0.1
    x = rng.integers(-100, 100, n).astype(np.int64)
    img = fl.write_image([("k", fl.INT32, np.ma.array(k, mask=~kv), fl.ENC_AUTO), ("f", fl.INT8, f, fl.ENC_AUTO),
                          ("x", fl.INT64, x, fl.ENC_AUTO)], rowgroup=RG)
    t = conn0.read_image(img)
    cols, valid = {0: k, 1: f, 2: x}, {0: kv}
    aggs = [("count",), ("sum", 2), ("count", 0)]
    filt = [(1, "=", 1)]
    sel = filter_mask(cols, filt, n)
    try:
        for r0, r1 in ((0, 5), (4, 5), (2, 5), (1, 3)):
            rows = np.zeros(n, bool)
            rows[r0 * RG:min(n, r1 * RG)] = True
            want = groups(cols, valid, [0], aggs, rows & sel)
            assert want and all(key[0] is None or key[0] < 400 for key in want)
            for kw in (dict(having=[(1, "<", 0)]), dict(having=[(0, ">", 1), (1, ">=", -20)]),
                       dict(order_by=(1, "desc"), limit=5), dict(order_by=(0, "asc"), limit=1024), dict(limit=3),
                       dict(having=[(2, "=", 0)]),                                   # the NULL-key group alone
                       dict(having=[(1, "<", 0)], order_by=(0, "desc", "nulls_first"), limit=7)):
                h = t.aggregate_hashed([0], aggs, 1024, filt=filt, rg_begin=r0, rg_end=r1, **kw)
                got = check(h, want, what=(r0, r1), **kw)
                # the selection sees the selected rows' groups only; first rows are table indices
                assert all(r0 * RG <= fr < min(n, r1 * RG) and sel[fr] for _, fr, _ in got)
                assert h.groups_total == len(want)
    finally:
        t.close()


# ---- 5. reproducibility and the several-pipeline fallback
@pytest.mark.gpu
def test_gpu_selection_is_identical_across_batches_and_pipelines(fl, gpu, seltab, ordtab, monkeypatch):
    simg, ts, scols, svalid, swant = seltab
    oimg, to, ocols, owant = ordtab
    having = [[(A_COUNT, ">=", 100), (A_SUM, "<", 0)], [(A_WIDE, ">", 0)], [(A_MAXF, "=", float("nan"))],
              [(A_NULLSUM, "!=", 0)], [(A_MINF, "<=", -0.0), (A_MAXU64, ">", 2**63)]]

    def run(ts, to):   # (the batch size is read when a scan starts)
        sets = []
        for hv in having:
            h = ts.aggregate_hashed([0], SEL_AGGS, 64, having=hv)
            sets.append((norm(sorted(got_rows(h), key=lambda r: r[1])), h.groups_total, h.groups_passed))
        return sets, run_seltab(ts), run_ordtab(to)

    monkeypatch.delenv("FLS_SCAN_BATCH", raising=False)
    base = run(ts, to)
    assert base[0] == [(norm(select(swant, hv)[0]), len(swant), select(swant, hv)[1]) for hv in having]
    for batch in ("1", "3"):
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)
        assert run(ts, to) == base, batch
    monkeypatch.setenv("FLS_SCAN_BATCH", "1")
    monkeypatch.setenv("FLS_SCAN_SLOTS", "4")
    assert run(ts, to) == base, "batch 1, four slots"
    monkeypatch.delenv("FLS_SCAN_SLOTS")
    monkeypatch.delenv("FLS_SCAN_BATCH")
    # two pipelines (the same GPU listed twice): every key of seltab is in both shards, most of ordtab's in one
    conn2 = fl.Connection([0, 0])
    ts2, to2 = conn2.read_image(simg), conn2.read_image(oimg)
    try:
        assert run(ts2, to2) == base, "two pipelines"
        h = ts2.aggregate_hashed([0], SEL_AGGS, 64, having=[(A_COUNT, ">", 0)], order_by=A_SUM, limit=5)
        assert not h.selected_on_device and h.groups_total == len(swant)
        # a range inside one shard: one pipeline holds the groups, and the device decides
        h = ts2.aggregate_hashed([0], SEL_AGGS, 64, having=[(A_COUNT, ">", 0)], rg_begin=0, rg_end=1)
        assert h.selected_on_device and h.groups_passed == h.groups_total == len(h)
    finally:
        ts2.close()
        to2.close()
        conn2.close()


@pytest.mark.gpu
def test_gpu_two_pipelines_decide_on_the_merged_value(fl, gpu, conn0):
    """Two 1024-row row groups, one per pipeline.  Key 1 sums to 60 in each
    shard and passes `sum > 100` only merged; key 2 sums to 150 in the first
    shard alone and to 50 merged: it must fail.  Keys 3.. live in one shard."""
    n = 2 * RG
    k = np.concatenate([np.arange(RG) % 50 + 3, np.arange(RG) % 50 + 53]).astype(np.int32)
    x = np.ones(n, dtype=np.int64)
    for rows, key, val in (((0, 1, 2), 1, 20), ((RG, RG + 1, RG + 2), 1, 20), ((5, 6, 7), 2, 50),
                           ((RG + 5, RG + 6), 2, -50)):
        k[list(rows)] = key
        x[list(rows)] = val
    img = fl.write_image([("k", fl.INT32, k, fl.ENC_AUTO), ("x", fl.INT64, x, fl.ENC_AUTO)], rowgroup=RG)
    cols = {0: k, 1: x}
    aggs = [("sum", 1), ("count",)]
    want = groups(cols, {}, [0], aggs, np.ones(n, bool))
    assert want[(1,)][1] == [120, 6] and want[(2,)][1] == [50, 5]
    cases = (dict(having=[(0, ">", 100)]), dict(having=[(0, ">", 100)], order_by=(0, "desc"), limit=3),
             dict(order_by=(0, "desc"), limit=2), dict(having=[(0, "<=", 50), (1, "=", 5)]), dict(limit=4))
    t1 = conn0.read_image(img)
    conn2 = fl.Connection([0, 0])
    t2 = conn2.read_image(img)
    try:
        for kw in cases:
            h1, h2 = t1.aggregate_hashed([0], aggs, 128, **kw), t2.aggregate_hashed([0], aggs, 128, **kw)
            check(h1, want, **kw)
            check(h2, want, **kw)
            assert h1.selected_on_device and not h2.selected_on_device
            assert got_rows(h1) == got_rows(h2) or (len(kw) == 1 and "having" in kw)
        got = {key for key, _, _ in got_rows(t2.aggregate_hashed([0], aggs, 128, having=[(0, ">", 100)]))}
        assert (1,) in got and (2,) not in got
        # either shard alone decides the other way
        alone = {key for key, _, _ in got_rows(t1.aggregate_hashed([0], aggs, 128, having=[(0, ">", 100)],
                                                                   rg_begin=0, rg_end=1))}
        assert (1,) not in alone and (2,) in alone
    finally:
        t1.close()
        t2.close()
        conn2.close()


# ---- 6. the limit still holds
@pytest.mark.gpu
def test_gpu_max_groups_still_limits_a_selecting_call(fl, gpu, many):
    img, t, cols = many
    want = groups(cols, {}, [0], MANY_AGGS, np.ones(len(cols[0]), bool))
    for kw in (dict(having=[(1, ">", 0)]), dict(order_by=(1, "desc"), limit=10), dict(limit=5)):
        with pytest.raises(fl.FlsError) as e:
            t.aggregate_hashed([0], MANY_AGGS, D3 - 1, **kw)
        assert e.value.code == ERR_LIMIT and "max_groups" in e.value.msg and str(D3 - 1) in e.value.msg, e.value
        # the same table answers a correct call, with the tightest table
        check(t.aggregate_hashed([0], MANY_AGGS, D3, **kw), want, **kw)
    assert t.aggregate([("count",), ("sum", 1)]) == [len(cols[0]), int(cols[1].sum())]


# ---- 7. the queries
@pytest.mark.gpu
def test_gpu_q18_shape_having_on_the_device(fl, gpu, lineitem):
    t, cols = lineitem
    okey, qty = cols[C_OKEY], cols[C_QTY].astype(np.int64)
    keys, first, inv = np.unique(okey, return_index=True, return_inverse=True)
    sums = np.zeros(len(keys), np.int64)
    np.add.at(sums, inv, qty)
    counts = np.bincount(inv, minlength=len(keys))
    ndist = len(keys)
    big = sums > 25000                                  # sum(l_quantity) > 250
    assert 0 < big.sum() < ndist
    h = t.aggregate_hashed([C_OKEY], [("sum", C_QTY), ("count",)], ndist, having=[(0, ">", 25000)])
    assert h.groups_total == ndist and h.groups_passed == len(h) == int(big.sum()) and h.selected_on_device
    o = np.argsort(h.key_values[0].view(np.int64))
    assert np.array_equal(h.key_values[0].view(np.int64)[o], keys[big]) and not h.key_null[0].any()
    assert np.array_equal(h.lo[0][o].view(np.int64), sums[big]) and not h.hi[0].any()
    assert np.array_equal(h.count[1][o], counts[big].astype(np.uint64))
    assert np.array_equal(h.first_row[o], first[big].astype(np.uint64))


@pytest.mark.gpu
def test_gpu_q3_shape_top_ten_revenues(fl, gpu, lineitem, conn0):
    t, cols = lineitem
    okey = cols[C_OKEY]
    orders = np.unique(okey)[::3]                       # the build side: a third of the orders
    ks = conn0.keyset(orders, signed=True)
    try:
        filt = [(C_OKEY, "in_set", ks), (C_SHIPDATE, ">", 9000)]
        aggs = [("sum_expr", [(0, 1, C_PRICE), (100, -1, C_DISC)])]
        plain = t.aggregate_hashed([C_OKEY], aggs, len(orders), filt=filt)
        best = sorted(got_rows(plain), key=lambda r: (-r[2][0], r[1]))[:10]
        assert len(plain) > 1000
        h = t.aggregate_hashed([C_OKEY], aggs, len(orders), filt=filt, order_by=(0, "desc"), limit=10)
        assert got_rows(h) == best and [(k, v) for k, _, v in best] == h.to_list()
        assert h.groups_total == h.groups_passed == len(plain) and h.selected_on_device
        # against the inputs, too
        sel = np.isin(okey, orders) & (cols[C_SHIPDATE] > 9000)
        want = groups(cols, {}, [C_OKEY], aggs, sel)
        check(h, want, order_by=(0, "desc"), limit=10)
    finally:
        ks.close()
