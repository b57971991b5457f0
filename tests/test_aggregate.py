"""Aggregate pushdown: COUNT, SUM, MIN, MAX and SUM of products reduced on the
GPU (fls_aggregate / Table.aggregate; csrc/fls_agg.hip).

Expected values come from the inputs themselves -- the seeded generators'
gen_values, or the arrays handed to write_image -- reduced in Python with
exact integers, under helpers.filter_mask for the selection and the arrays'
own validity.  Integer results, counts, MIN / MAX and NULL-ness compare
exactly; float MIN / MAX by value (a zero of either sign matches, any NaN
matches NaN); a binary64 sum against math.fsum of the contributing values
within (n - 1) * 2^-53 * sum |x_i|, the first-order worst-case bound of any
summation order over n values (derived, not measured; used only on inputs
without inf / NaN).

CPU tests: the exported symbol, argument errors, the SUM_PRODUCT overflow
guard, the all-pruned call (no device work), the kernel's resources.  GPU
tests: every width and encoding, NULLs, floats, reproducibility across batch
sizes and GPU counts, lineitem under the filter suite's predicates, FSST / ALP
filter columns."""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import filter_mask, rand64

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "duckdb-fastlane_amd" / "libflsgpu.so"

ERR_ARG, ERR_DEVICE = -3, -4
DAY_1994, DAY_1995 = 8766, 9131       # 1994-01-01, 1995-01-01 as DATE days
C_OKEY, C_PART, C_LINE, C_QTY, C_PRICE, C_DISC = 0, 1, 3, 4, 5, 6
C_RFLAG, C_SHIPDATE, C_INSTRUCT, C_MODE = 8, 10, 13, 14

# the named predicates of tests/test_filter.py, restated
Q6 = [(C_SHIPDATE, ">=", DAY_1994), (C_SHIPDATE, "<", DAY_1995), (C_DISC, ">=", 5), (C_DISC, "<=", 7),
      (C_QTY, "<", 2400)]
PREDICATES = {
    "q6": Q6,
    "okey_range": [(C_OKEY, ">=", 30000), (C_OKEY, "<", 130000)],
    "mode_in": [(C_MODE, "=", "AIR", 1), (C_MODE, "=", "MAIL", 1), (C_LINE, "<=", 2)],
    "long_string": [(C_INSTRUCT, "=", "DELIVER IN PERSON")],
    "string_range": [(C_INSTRUCT, ">", "COLLECT COD"), (C_INSTRUCT, "<=", "NONE"), (C_RFLAG, "!=", "N")],
    "string_prefix_tie": [(C_INSTRUCT, "<", "TAKE BACK RETURNZ"), (C_INSTRUCT, ">=", "TAKE")],
    "nothing": [(C_PART, "<", 0)],
    "or_across_columns": [(C_LINE, "=", 7, 5), (C_DISC, "=", 0, 5)],
    "is_null": [(C_PART, "is_null", None)],
    "is_not_null": [(C_PART, "is_not_null", None), (C_PRICE, ">", 9000000)],
}


# ------------------------------------------------------------ expected values
def isum(vals, m):
    """exact sum of the integer values under mask m, or None over no row"""
    return sum(int(x) for x in vals[m]) if m.any() else None


def expect_int(fn, vals, m, vals2=None):
    """count / sum / min / max / sum_product of integer values under mask m
    (selected and valid rows), in Python integers"""
    if fn == "count":
        return int(m.sum())
    if not m.any():
        return None
    if fn == "sum":
        return isum(vals, m)
    if fn == "sum_product":
        return sum(int(a) * int(b) for a, b in zip(vals[m], vals2[m]))
    return int(vals[m].min()) if fn == "min" else int(vals[m].max())


def expect_float_minmax(fn, vals, m):
    """DuckDB's float order: NaN above every number, -0 == 0"""
    v = vals[m].astype(np.float64)
    if len(v) == 0:
        return None
    nan = np.isnan(v)
    if fn == "max":
        return float("nan") if nan.any() else float(v.max())
    return float("nan") if nan.all() else float(v[~nan].min())


def same_float(got, want):
    if want is None or got is None:
        return got is None and want is None
    if math.isnan(want):
        return math.isnan(got)
    return got == want   # by value: -0.0 == 0.0


def check_float_sum(got, vals, m, what=""):
    """a binary64 sum of finite values within the derived bound"""
    v = [float(x) for x in vals[m]]
    if not v:
        assert got is None, what
        return
    assert all(math.isfinite(x) for x in v)
    exact = math.fsum(v)
    tol = (len(v) - 1) * 2.0 ** -53 * math.fsum(abs(x) for x in v)
    print(f"{what}: sum {got!r} fsum {exact!r} |diff| {abs(got - exact):.3e} bound {tol:.3e} (n = {len(v)})")
    assert abs(got - exact) <= tol, (what, got, exact, tol)


# ------------------------------------------------------------------ CPU tests
def test_library_exports_fls_aggregate(_built):
    assert hasattr(C.CDLL(str(LIB)), "fls_aggregate")


@pytest.fixture(scope="module")
def small_lineitem(fl):
    t = fl.Connection([0]).read_image(fl.gen_image("lineitem", 0.01))
    yield t
    t.close()


@pytest.mark.parametrize("aggs,what", [
    ([], None),                                        # n == 0
    ([("count",)] * 33, None),                          # n > 32
    ([("count",), ("sum", 99)], "aggregate 1"),         # a column out of range
    ([("count", 99)], "aggregate 0"),
    ([("count",), ("count",), (9, C_QTY)], "aggregate 2"),      # an unknown function
    ([("sum", C_MODE)], "aggregate 0"),                 # SUM / MIN / MAX / SUM_PRODUCT of a string column
    ([("count", C_MODE), ("min", C_MODE)], "aggregate 1"),
    ([("max", C_INSTRUCT)], "aggregate 0"),
    ([("sum_product", C_QTY, C_MODE)], "aggregate 0"),
    ([("sum_product", C_MODE, C_QTY)], "aggregate 0"),
    ([("sum_product", C_QTY, 99)], "aggregate 0"),
])
def test_argument_errors(fl, small_lineitem, aggs, what):
    with pytest.raises(fl.FlsError) as e:
        small_lineitem.aggregate(aggs)
    assert e.value.code == ERR_ARG, e.value
    if what:
        assert what + ":" in e.value.msg, e.value


def test_sum_product_float_operand_is_an_argument_error(fl):
    n = 1500
    img = fl.write_image([("i", fl.INT32, np.arange(n, dtype=np.int32), fl.ENC_AUTO),
                          ("d", fl.DOUBLE, np.arange(n) * 0.5, fl.ENC_AUTO),
                          ("f", fl.FLOAT, np.arange(n, dtype=np.float32), fl.ENC_AUTO)], rowgroup=1024)
    t = fl.Connection([0]).read_image(img)
    for a, b in [(0, 1), (1, 0), (2, 0), (1, 2)]:
        with pytest.raises(fl.FlsError) as e:
            t.aggregate([("count",), ("sum_product", a, b)])
        assert e.value.code == ERR_ARG and "aggregate 1:" in e.value.msg, e.value


def test_sum_product_overflow_guard(fl, small_lineitem):
    rng = np.random.default_rng(11)
    n = 3000
    a = rand64(rng, n).view(np.int64)
    b = rand64(rng, n).view(np.int64)
    a[0], b[0] = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    img = fl.write_image([("a", fl.INT64, a, fl.ENC_AUTO), ("b", fl.INT64, b, fl.ENC_AUTO)], rowgroup=1024)
    t = fl.Connection([0]).read_image(img)
    with pytest.raises(fl.FlsError) as e:
        t.aggregate([("sum_product", 0, 1)])
    assert e.value.code == ERR_ARG and "aggregate 0:" in e.value.msg and "may overflow 128 bits" in e.value.msg
    # l_extendedprice x l_discount is far below 2^127: the guard lets it through
    # (without a GPU the call then fails on the device, not on its arguments)
    if fl.device_count() > 0:
        assert small_lineitem.aggregate([("sum_product", C_PRICE, C_DISC)])[0] > 0
    else:
        with pytest.raises(fl.FlsError) as e:
            small_lineitem.aggregate([("sum_product", C_PRICE, C_DISC)])
        assert e.value.code == ERR_DEVICE, e.value


def test_everything_pruned_needs_no_gpu(fl):
    t = fl.Connection([0]).read_image(fl.gen_image("lineitem", 0.1))
    got = t.aggregate([("count",), ("sum", C_QTY), ("min", C_SHIPDATE)], filt=[(C_PART, "<", 0)])
    assert got == [0, None, None]
    assert t.pruned == t.nrowgroups == 10
    # an empty row-group range: the same, nothing pruned
    assert t.aggregate([("count",), ("count", C_MODE), ("max", C_QTY)], rg_begin=3, rg_end=3) == [0, 0, None]
    assert t.pruned == 0


def test_aggregate_kernel_resources():
    """the kernel keeps its accumulators in registers: no scratch, no spill"""
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    res = kernel_resources.resources(str(LIB))
    hits = {k: v for k, v in res.items() if "aggregate_kernel" in k}
    assert len(hits) == 1, hits
    for name, r in hits.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)


# ------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def conn0(fl):
    """one connection (one scan pipeline on GPU 0) for the tables of this module"""
    conn = fl.Connection([0])
    yield conn
    conn.close()


RG1 = 2048
N1 = 2 * RG1 + 1024 + 37   # three row groups; the last: one full vector and a 37-row tail vector


@pytest.fixture(scope="module")
def widths(fl, conn0):
    """every integer-like type and width, and the forced encodings"""
    rng = np.random.default_rng(20240613)
    n = N1

    def full(dt):
        ii = np.iinfo(dt)
        if ii.bits == 64:
            return rand64(rng, n).view(dt)
        return rng.integers(ii.min, int(ii.max) + 1, n).astype(dt)

    big = (rand64(rng, n) >> np.uint64(2)) | np.uint64(1 << 62)          # [2^62, 2^63)
    runs = np.repeat(rng.integers(-10**9, 10**9, (n + 49) // 50), 50)[:n].astype(np.int32)
    five = np.array([-32768, -3, 0, 7, 32767], dtype=np.int16)[rng.integers(0, 5, n)]
    spec = [
        ("i8", fl.INT8, full(np.int8), fl.ENC_AUTO), ("i16", fl.INT16, full(np.int16), fl.ENC_AUTO),
        ("i32", fl.INT32, full(np.int32), fl.ENC_AUTO), ("i64", fl.INT64, full(np.int64), fl.ENC_AUTO),
        ("u8", fl.UINT8, full(np.uint8), fl.ENC_AUTO), ("u16", fl.UINT16, full(np.uint16), fl.ENC_AUTO),
        ("u32", fl.UINT32, full(np.uint32), fl.ENC_AUTO), ("u64", fl.UINT64, full(np.uint64), fl.ENC_AUTO),
        ("b", fl.BOOLEAN, rng.integers(0, 2, n).astype(np.uint8), fl.ENC_AUTO),
        ("dt", fl.DATE, rng.integers(-50000, 50001, n).astype(np.int32), fl.ENC_AUTO),
        ("dec", fl.DECIMAL, rng.integers(-9 * 10**17, 9 * 10**17 + 1, n).astype(np.int64), fl.ENC_AUTO, 18, 2),
        ("big", fl.INT64, big.astype(np.int64), fl.ENC_AUTO),
        ("nbig", fl.INT64, -big.astype(np.int64), fl.ENC_AUTO),
        ("sorted", fl.INT64, np.sort(rng.integers(-2**40, 2**40, n)).astype(np.int64), fl.ENC_DELTA),
        ("runs", fl.INT32, runs, fl.ENC_RLE),
        ("five", fl.INT16, five, fl.ENC_DICT),
    ]
    img = fl.write_image(spec, rowgroup=RG1)
    cols = {c: s[2] for c, s in enumerate(spec)}
    t = conn0.read_image(img)
    yield img, cols, [s[0] for s in spec], t
    t.close()


W_I8, W_I16, W_I32, W_DEC, W_BIG, W_NBIG = 0, 1, 2, 10, 11, 12


def widths_aggs(ncols):
    aggs = [("count",)]
    for c in range(ncols):
        aggs += [("count", c), ("sum", c), ("min", c), ("max", c)]
    return aggs


def run_chunked(t, aggs, filt=None, **kw):
    """at most 32 aggregates per call"""
    out = []
    for i in range(0, len(aggs), 32):
        out += t.aggregate(aggs[i:i + 32], filt=filt, **kw)
    return out


def widths_expected(cols, aggs, sel):
    out = []
    for a in aggs:
        if len(a) == 1:
            out.append(int(sel.sum()))
        elif a[0] == "sum_product":
            out.append(expect_int("sum_product", cols[a[1]], sel, cols[a[2]]))
        else:
            out.append(expect_int(a[0], cols[a[1]], sel))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [None, [(W_I32, "<", 0)]], ids=["all", "i32_negative"])
def test_gpu_every_width_and_encoding(fl, gpu, widths, filt):
    img, cols, names, t = widths
    assert t.nrowgroups == 3 and t.nrows == N1
    aggs = widths_aggs(len(cols)) + [("sum_product", W_I32, W_I16), ("sum_product", W_DEC, W_I8)]
    sel = filter_mask(cols, filt, N1) if filt else np.ones(N1, bool)
    got = run_chunked(t, aggs, filt)
    want = widths_expected(cols, aggs, sel)
    for a, g, w in zip(aggs, got, want):
        assert g == w, (a, names[a[1]] if len(a) > 1 else "*", g, w)
    # the sums of the [2^62, 2^63) column and its negation pass 2^64 in both signs
    if filt is None:
        assert want[aggs.index(("sum", W_BIG))] > 2**64 and want[aggs.index(("sum", W_NBIG))] < -2**64


@pytest.mark.gpu
def test_gpu_more_than_32_aggregates_is_an_error(fl, gpu, widths):
    img, cols, names, t = widths
    assert len(t.aggregate([("sum", c % 16) for c in range(32)])) == 32
    with pytest.raises(fl.FlsError) as e:
        t.aggregate([("sum", c % 16) for c in range(33)])
    assert e.value.code == ERR_ARG


# ---- NULLs
RG2 = 1024
N2 = 3 * RG2 + 5


@pytest.fixture(scope="module")
def nulls(fl, conn0):
    rng = np.random.default_rng(99)
    n = N2
    # x: row group 0 holds [1000, 2000), the later rows [-5000, -4000): a
    # placeholder (whatever the writer stores at NULL rows) read into a result
    # changes MIN and SUM in the one, MAX and SUM in the other
    x = np.where(np.arange(n) < RG2, rng.integers(1000, 2000, n), rng.integers(-5000, -4000, n)).astype(np.int32)
    xv = rng.random(n) >= 0.3
    xv[RG2:2 * RG2] = False                       # row group 1 entirely NULL
    xv[2 * RG2:3 * RG2] = False
    xv[3 * RG2 - 1] = True                        # a vector whose only valid row is its last
    y = np.round(rng.normal(0, 10, n), 2)
    yv = rng.random(n) >= 0.2
    sv = rng.random(n) >= 0.25
    s = [f"s{i % 13}" if sv[i] else None for i in range(n)]
    img = fl.write_image([("x", fl.INT32, np.ma.array(x, mask=~xv), fl.ENC_AUTO),
                          ("y", fl.DOUBLE, np.ma.array(y, mask=~yv), fl.ENC_AUTO),
                          ("s", fl.VARCHAR, s, fl.ENC_AUTO)], rowgroup=RG2)
    t = conn0.read_image(img)
    yield t, {0: x, 1: y}, {0: xv, 1: yv, 2: sv}
    t.close()


def null_aware_mask(cols, valid, terms, n):
    """helpers.filter_mask per term, with NULL semantics: a NULL row satisfies
    IS NULL and no comparison"""
    out = np.ones(n, bool)
    for col, op, val in terms:
        if op == "is_null":
            out &= ~valid[col]
        elif op == "is_not_null":
            out &= valid[col]
        else:
            out &= valid[col] & filter_mask(cols, [(col, op, val)], n)
    return out


NULL_AGGS = [("count",), ("count", 0), ("count", 2), ("sum", 0), ("min", 0), ("max", 0), ("sum", 1)]


def check_nulls(t, cols, valid, terms, r0, r1):
    n = N2
    sel = null_aware_mask(cols, valid, terms, n)
    rows = np.zeros(n, bool)
    rows[r0 * RG2:min(n, r1 * RG2)] = True
    sel &= rows
    got = t.aggregate(NULL_AGGS, filt=terms, rg_begin=r0, rg_end=r1)
    mx = sel & valid[0]
    assert got[:6] == [int(sel.sum()), int(mx.sum()), int((sel & valid[2]).sum()), expect_int("sum", cols[0], mx),
                       expect_int("min", cols[0], mx), expect_int("max", cols[0], mx)], (terms, r0, r1, got)
    check_float_sum(got[6], cols[1], sel & valid[1], f"sum(y) under {terms} rg [{r0},{r1})")
    return got


@pytest.mark.gpu
def test_gpu_nulls(fl, gpu, nulls):
    t, cols, valid = nulls
    assert t.nrowgroups == 4
    check_nulls(t, cols, valid, [], 0, 4)
    got = check_nulls(t, cols, valid, [(0, "is_null", None)], 0, 4)
    assert got[1] == 0 and got[3] is None and got[4] is None and got[5] is None
    check_nulls(t, cols, valid, [(0, "is_not_null", None), (1, ">", 0.0)], 0, 4)
    got = check_nulls(t, cols, valid, [], 1, 2)   # the all-NULL row group alone
    assert got[0] == RG2 and got[1] == 0 and got[3:6] == [None, None, None]
    check_nulls(t, cols, valid, [], 2, 3)         # the vector whose only valid row is its last
    check_nulls(t, cols, valid, [], 3, 4)         # the 5-row tail


# ---- floats
@pytest.fixture(scope="module")
def floats(fl, conn0):
    rng = np.random.default_rng(4242)
    n = N1
    d = np.round(rng.normal(0, 10, n), 2)
    f = d.astype(np.float32)
    pool = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e300, 1.5, -1.5])
    g = pool[rng.integers(0, len(pool), n)]
    img = fl.write_image([("d", fl.DOUBLE, d, fl.ENC_AUTO), ("f", fl.FLOAT, f, fl.ENC_AUTO),
                          ("g", fl.DOUBLE, g, fl.ENC_AUTO)], rowgroup=RG1)
    t = conn0.read_image(img)
    yield img, {0: d, 1: f, 2: g}, t
    t.close()


@pytest.mark.gpu
def test_gpu_floats(fl, gpu, floats):
    img, cols, t = floats
    every = np.ones(N1, bool)
    got = t.aggregate([("sum", 0), ("min", 0), ("max", 0), ("sum", 1), ("min", 1), ("max", 1), ("count", 0)])
    check_float_sum(got[0], cols[0], every, "sum(d)")
    check_float_sum(got[3], cols[1], every, "sum(f)")
    for k, (fn, c) in {1: ("min", 0), 2: ("max", 0), 4: ("min", 1), 5: ("max", 1)}.items():
        assert same_float(got[k], expect_float_minmax(fn, cols[c], every)), (fn, c, got[k])
    assert got[6] == N1
    # a filter on d itself: a second block path (mask from the filter kernel)
    sel = filter_mask(cols, [(0, ">", 2.5)], N1)
    got = t.aggregate([("sum", 0), ("sum", 1), ("min", 1), ("count",)], filt=[(0, ">", 2.5)])
    check_float_sum(got[0], cols[0], sel, "sum(d) where d > 2.5")
    check_float_sum(got[1], cols[1], sel, "sum(f) where d > 2.5")
    assert same_float(got[2], expect_float_minmax("min", cols[1], sel)) and got[3] == int(sel.sum())
    # NaN, infinities and signed zeros
    g = cols[2]
    mx, mn, sm = t.aggregate([("max", 2), ("min", 2), ("sum", 2)])
    assert math.isnan(mx) and mn == -math.inf and math.isnan(sm)
    terms = [(2, ">", 0.0), (2, "!=", float("nan"))]
    sel = filter_mask(cols, terms, N1)
    sm, mx, mn, cnt = t.aggregate([("sum", 2), ("max", 2), ("min", 2), ("count",)], filt=terms)
    assert sm == math.inf and mx == math.inf and mn == 1.5 and cnt == int(sel.sum())
    terms = [(2, "<", 1e300), (2, ">", -1e300)]
    sel = filter_mask(cols, terms, N1)
    assert np.isfinite(g[sel]).all() and sel.any()
    sm, mx, mn, cnt = t.aggregate([("sum", 2), ("max", 2), ("min", 2), ("count", 2)], filt=terms)
    check_float_sum(sm, g, sel, "sum(g) finite")
    assert (mx, mn, cnt) == (1.5, -1.5, int(sel.sum()))


# ---- reproducibility
def _bits(x):
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])


@pytest.mark.gpu
def test_gpu_results_are_bit_identical_across_batches_and_gpus(fl, gpu, widths, floats, monkeypatch):
    wimg, wcols, _, tw = widths
    fimg, fcols, tf = floats
    iaggs = widths_aggs(len(wcols))

    def run(tf, tw):   # (the batch size is read when a scan starts)
        sums = tf.aggregate([("sum", 0), ("sum", 1)])
        return [_bits(s) for s in sums], run_chunked(tw, iaggs)

    monkeypatch.delenv("FLS_SCAN_BATCH", raising=False)
    base = run(tf, tw)
    assert base[1] == widths_expected(wcols, iaggs, np.ones(N1, bool))
    for batch in ("1", "3"):
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)
        assert run(tf, tw) == base, batch
    monkeypatch.setenv("FLS_SCAN_BATCH", "1")
    monkeypatch.setenv("FLS_SCAN_SLOTS", "4")       # four batches in flight, the last two on recycled host batches
    assert run(tf, tw) == base, "batch 1, four slots"
    monkeypatch.delenv("FLS_SCAN_SLOTS")
    monkeypatch.setenv("FLS_SCAN_BATCH", "3")
    # the row groups sharded over two pipelines (the same GPU listed twice)
    conn2 = fl.Connection([0, 0])
    tf2, tw2 = conn2.read_image(fimg), conn2.read_image(wimg)
    try:
        assert run(tf2, tw2) == base, "batch 3, two pipelines"
        monkeypatch.delenv("FLS_SCAN_BATCH")
        assert run(tf2, tw2) == base, "default batch, two pipelines"
    finally:
        tf2.close()
        tw2.close()
        conn2.close()


@pytest.mark.gpu
def test_gpu_failed_refill_ends_every_reducing_scan_with_its_error(gpu):
    """The three reducing scans (aggregate, grouped aggregate, top-N) share one
    driver: a batch refill that cannot be enqueued (FLS_TEST_FAIL_ENQUEUE, as
    in tests/test_scan_errors.py) must come back from each as that error, and
    the next call on the table must start clean.  In a child process: the hook
    counts the enqueues made while it is set, over the whole process."""
    import os
    import subprocess
    code = """
import os
import numpy as np
import pkgload
fl = pkgload.load()
RG = 1024
v = np.arange(3 * RG, dtype=np.int32)
img = fl.write_image([("v", fl.INT32, v, fl.ENC_FFOR), ("g", fl.INT32, v % 3, fl.ENC_FFOR)], rowgroup=RG)
t = fl.Connection([0]).read_image(img)
assert t.nrowgroups == 3                      # three batches of one row group on two slots
calls = {"aggregate": lambda: t.aggregate([("sum", 0), ("count",)]),
         "grouped": lambda: t.aggregate_grouped([1], [("sum", 0)]),
         # (under a filter that keeps every row: without one the key's zone maps leave one row group to read)
         "topn": lambda: t.topn(0, 5, desc=True, filt=[(0, ">=", 0)])[0].tolist()}
want = {name: f() for name, f in calls.items()}
assert want["aggregate"] == [int(v.sum()), len(v)] and want["topn"] == [len(v) - 1 - i for i in range(5)], want
# a failing call makes three enqueues: two when the scan starts, then the
# refill at the first row group's hand-out, which is the one that fails
for i, (name, f) in enumerate(calls.items()):
    os.environ["FLS_TEST_FAIL_ENQUEUE"] = str(3 * (i + 1))
    try:
        f()
        print(name, "no error")
    except fl.FlsError as e:
        print(name, e.msg)
    del os.environ["FLS_TEST_FAIL_ENQUEUE"]
    assert f() == want[name], name
"""
    out = subprocess.run([sys.executable, "-c", code], env={**os.environ, "FLS_SCAN_BATCH": "1"},
                         capture_output=True, text=True, timeout=120, cwd=str(ROOT))
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert [ln.split()[0] for ln in lines] == ["aggregate", "grouped", "topn"], out.stdout
    assert all("injected batch enqueue failure" in ln for ln in lines), out.stdout


# ---- lineitem
SF = 0.1
WL = "lineitem"


@pytest.fixture(scope="module")
def lineitem(fl, conn0):
    img = fl.gen_image(WL, SF)
    t = conn0.read_image(img)
    n = t.nrows
    cols = {}
    for c, (name, ty, _, _, _) in enumerate(t.schema()):
        if ty == fl.VARCHAR:
            codes = fl.gen_values(WL, c, 0, n, np.uint32, SF)
            words = []
            while (s := fl.gen_dict_string(WL, c, len(words))) is not None:
                words.append(s.encode())
            cols[c] = [words[k] for k in codes]
        else:
            cols[c] = fl.gen_values(WL, c, 0, n, fl.NP_DTYPE[ty], SF)
    yield img, t, cols
    t.close()


LI_AGGS = [("count",), ("sum", C_QTY), ("sum_product", C_PRICE, C_DISC), ("min", C_SHIPDATE), ("max", C_SHIPDATE),
           ("count", C_MODE)]


def lineitem_expected(cols, terms, n):
    sel = filter_mask(cols, terms, n)
    k = int(sel.sum())
    if k == 0:
        return [0, None, None, None, None, 0]
    qty = cols[C_QTY][sel].astype(object)
    prod = cols[C_PRICE][sel].astype(object) * cols[C_DISC][sel].astype(object)
    ship = cols[C_SHIPDATE][sel]
    return [k, int(qty.sum()), int(prod.sum()), int(ship.min()), int(ship.max()), k]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PREDICATES))
def test_gpu_lineitem_predicates(fl, gpu, lineitem, name):
    img, t, cols = lineitem
    assert t.nrowgroups == 10   # the default batch of 8 splits it
    terms = PREDICATES[name]
    assert t.aggregate(LI_AGGS, filt=terms) == lineitem_expected(cols, terms, t.nrows)
    assert t.pruned == sum(not t.may_match(rg, terms) for rg in range(t.nrowgroups))


@pytest.mark.gpu
def test_gpu_lineitem_no_state_leaks_between_calls(fl, gpu, lineitem):
    img, t, cols = lineitem
    n = t.nrows
    assert t.aggregate(LI_AGGS, filt=Q6) == lineitem_expected(cols, Q6, n)
    other = PREDICATES["okey_range"]
    assert t.aggregate(LI_AGGS, filt=other) == lineitem_expected(cols, other, n)
    assert t.aggregate(LI_AGGS) == lineitem_expected(cols, [], n)
    # a plain scan after an aggregate still delivers the right rows
    got = list(t.scan(cols=[C_OKEY, C_QTY], rg_begin=9, rg_end=10))
    assert len(got) == 1
    first_row, arrays = got[0]
    assert first_row == 9 * 65536
    assert np.array_equal(arrays[C_OKEY].view(np.int64), cols[C_OKEY][first_row:])
    assert np.array_equal(arrays[C_QTY].view(np.int64), cols[C_QTY][first_row:])
    assert arrays[C_PRICE] is None


# ---- FSST / ALP filter columns
@pytest.mark.gpu
def test_gpu_fsst_filter_column(fl, gpu, conn0):
    wl, sf = "lineitem_full", 0.02
    terms = [(15, ">=", "furiously"), (15, "<", "q")]
    t = conn0.read_image(fl.gen_image(wl, sf))
    n = t.nrows
    cols = {15: fl.gen_strings(wl, 15, 0, n, sf), C_QTY: fl.gen_values(wl, C_QTY, 0, n, np.int64, sf)}
    sel = filter_mask(cols, terms, n)
    assert sel.any() and not sel.all()
    assert t.aggregate([("count",), ("sum", C_QTY), ("count", 15)], filt=terms) == \
        [int(sel.sum()), isum(cols[C_QTY], sel), int(sel.sum())]


@pytest.mark.gpu
def test_gpu_alp_double_sum(fl, gpu, conn0):
    wl, sf = "lineitem_dbl", 0.02
    terms = [(4, "<", 24.0), (6, ">=", 0.05), (6, "<=", 0.07)]
    t = conn0.read_image(fl.gen_image(wl, sf))
    n = t.nrows
    assert t.schema()[4][1] == fl.DOUBLE
    cols = {c: fl.gen_values(wl, c, 0, n, np.float64, sf) for c in (4, 6)}
    sel = filter_mask(cols, terms, n)
    got = t.aggregate([("sum", 4), ("count",), ("min", 4), ("max", 4)], filt=terms)
    check_float_sum(got[0], cols[4], sel, "sum(l_quantity) lineitem_dbl")
    assert got[1] == int(sel.sum())
    assert same_float(got[2], expect_float_minmax("min", cols[4], sel))
    assert same_float(got[3], expect_float_minmax("max", cols[4], sel))
