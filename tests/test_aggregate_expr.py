"""SUM of a product of affine column terms (FLS_AGG_SUM_EXPR, function code 6):
the exact integer sum of prod (k + s * column) over one to three factors,
ungrouped (fls_aggregate_exprs + fls_aggregate / Table.aggregate's
("sum_expr", [(k, s, col), ...]); csrc/fls_agg.hip).

Expected values are Python integers computed from the arrays handed to
write_image or from the seeded generators' gen_values, under
helpers.filter_mask for the selection and the arrays' own validity.  Every
comparison is exact.

CPU tests: the exported symbol, every refusal of fls_aggregate_exprs
("expression i:") and of the aggregate calls ("aggregate i:"), the 128-bit
overflow bound, the all-pruned call (no device work), clearing the list.  GPU
tests: one to three factors over every integer width and signedness with both
signs of s and k, products past 2^64 in both signs, NULLs in each factor
column, a filter and a partial tail vector, a repeated column, the equalities
with sum_product and sum, reproducibility across batch sizes, and TPC-H Q1's
two measures on lineitem."""
import ctypes as C
import datetime
from pathlib import Path

import numpy as np
import pytest

from helpers import filter_mask, rand64

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "duckdb-fastlane_amd" / "libflsgpu.so"

ERR_ARG, ERR_DEVICE = -3, -4
C_PART, C_QTY, C_PRICE, C_DISC, C_TAX, C_SHIPDATE, C_MODE = 1, 4, 5, 6, 7, 10, 14
Q1_DAY = (datetime.date(1998, 9, 2) - datetime.date(1970, 1, 1)).days
DISC_PRICE = [(0, 1, C_PRICE), (100, -1, C_DISC)]                       # price * (1 - discount), scale 4
CHARGE = [(0, 1, C_PRICE), (100, -1, C_DISC), (100, 1, C_TAX)]          # ... * (1 + tax), scale 6


# ------------------------------------------------------------ expected values
def expect_expr(cols, factors, sel, valid=None):
    """(sum or None, count) of prod (k + s * x) over the rows of sel where every
    factor's column is valid, in Python integers"""
    m = sel.copy()
    if valid:
        for _, _, c in factors:
            m &= valid[c]
    rows = np.nonzero(m)[0]
    if len(rows) == 0:
        return None, 0
    total = 0
    for r in rows:
        p = 1
        for k, s, c in factors:
            p *= k + s * int(cols[c][r])
        total += p
    return total, len(rows)


def raw_value(v):
    """an AggregateValue as (value or None, count)"""
    if v.kind == 0:
        return None, int(v.count)
    x = (int(v.hi) << 64) | int(v.lo)
    return (x - (1 << 128) if x >> 127 else x), int(v.count)


# ------------------------------------------------------------------ CPU tests
def test_library_exports_fls_aggregate_exprs(_built):
    assert hasattr(C.CDLL(str(LIB)), "fls_aggregate_exprs")


def test_function_table_names_sum_expr(fl):
    assert fl.AGG_FNS["sum_expr"] == 6


@pytest.fixture(scope="module")
def small_lineitem(fl):
    t = fl.Connection([0]).read_image(fl.gen_image("lineitem", 0.01))
    yield t
    t.close()


OK = [(0, 1, C_QTY)]


@pytest.mark.parametrize("exprs,what", [
    ([[]], "expression 0"),                                           # nfactors outside 1..3
    ([OK, [(0, 1, C_QTY)] * 4], "expression 1"),
    ([[(1, 0, C_QTY)]], "expression 0"),                              # a sign that is not +1 / -1
    ([OK, OK, [(1, 1, C_QTY), (1, 2, C_DISC)]], "expression 2"),
    ([[(1, -2, C_QTY)]], "expression 0"),
    ([[(0, 1, 99)]], "expression 0"),                                 # a column out of range
    ([OK, [(0, 1, C_QTY), (5, -1, 16)]], "expression 1"),
    ([[(0, 1, C_MODE)]], "expression 0"),                             # a VARCHAR column
    ([OK, [(0, 1, C_PRICE), (1, -1, C_DISC), (0, 1, C_MODE)]], "expression 1"),
])
def test_expression_refusals(fl, small_lineitem, exprs, what):
    with pytest.raises(fl.FlsError) as e:
        small_lineitem.set_aggregate_exprs(exprs)
    assert e.value.code == ERR_ARG and what + ":" in e.value.msg, e.value
    # the same through Table.aggregate, which sets the list itself
    with pytest.raises(fl.FlsError) as e:
        small_lineitem.aggregate([("sum_expr", x) for x in exprs])
    assert e.value.code == ERR_ARG and what + ":" in e.value.msg, e.value


def test_more_than_32_expressions_are_refused(fl, small_lineitem):
    with pytest.raises(fl.FlsError) as e:
        small_lineitem.set_aggregate_exprs([OK] * 33)
    assert e.value.code == ERR_ARG, e.value


def test_float_double_and_blob_factor_columns_are_refused(fl):
    n = 1500
    img = fl.write_image([("i", fl.INT32, np.arange(n, dtype=np.int32), fl.ENC_AUTO),
                          ("d", fl.DOUBLE, np.arange(n) * 0.5, fl.ENC_AUTO),
                          ("f", fl.FLOAT, np.arange(n, dtype=np.float32), fl.ENC_AUTO),
                          ("b", fl.BLOB, [b"x", b"y"] * (n // 2), fl.ENC_DICT)], rowgroup=1024)
    t = fl.Connection([0]).read_image(img)
    for c in (1, 2, 3):
        with pytest.raises(fl.FlsError) as e:
            t.set_aggregate_exprs([[(0, 1, 0)], [(0, 1, 0), (1, -1, c)]])
        assert e.value.code == ERR_ARG and "expression 1:" in e.value.msg, e.value
    t.close()


def test_expression_index_out_of_range_names_the_aggregate(fl, small_lineitem):
    t = small_lineitem
    t.set_aggregate_exprs(None)
    with pytest.raises(fl.FlsError) as e:
        t.aggregate_raw([(6, 0)])
    assert e.value.code == ERR_ARG and "aggregate 0:" in e.value.msg, e.value
    t.set_aggregate_exprs([OK, DISC_PRICE])
    try:
        with pytest.raises(fl.FlsError) as e:
            t.aggregate_raw([("count",), (6, 1), (6, 2)])
        assert e.value.code == ERR_ARG and "aggregate 2:" in e.value.msg, e.value
        with pytest.raises(fl.FlsError) as e:
            t.aggregate_grouped([C_MODE], [(6, 5)])
        assert e.value.code == ERR_ARG and "aggregate 0:" in e.value.msg, e.value
        # code 9 stays an unknown function
        with pytest.raises(fl.FlsError) as e:
            t.aggregate_raw([(9, 0)])
        assert e.value.code == ERR_ARG and "unknown function" in e.value.msg, e.value
    finally:
        t.set_aggregate_exprs(None)


def test_clearing_the_list(fl, small_lineitem):
    t = small_lineitem
    nothing = [(C_PART, "<", 0)]          # prunes every row group: the accepted call needs no device
    t.set_aggregate_exprs([DISC_PRICE])
    t.set_filter(nothing)
    try:
        assert raw_value(t.aggregate_raw([(6, 0)])[0]) == (None, 0)   # sticky: read at call time
        assert raw_value(t.aggregate_raw([(6, 0)])[0]) == (None, 0)
        t.set_aggregate_exprs([])                                      # n = 0 clears
        with pytest.raises(fl.FlsError) as e:
            t.aggregate_raw([(6, 0)])
        assert e.value.code == ERR_ARG and "aggregate 0:" in e.value.msg, e.value
    finally:
        t.set_filter(None)
        t.set_aggregate_exprs(None)


def test_everything_pruned_needs_no_gpu(fl):
    t = fl.Connection([0]).read_image(fl.gen_image("lineitem", 0.1))
    aggs = [("count",), ("sum_expr", DISC_PRICE), ("sum_expr", CHARGE)]
    t.set_filter([(C_PART, "<", 0)])
    try:
        got = [raw_value(v) for v in t.aggregate_raw(aggs)]
    finally:
        t.set_filter(None)
    assert got == [(0, 0), (None, 0), (None, 0)]
    assert t.pruned == t.nrowgroups == 10
    assert t.aggregate(aggs, filt=[(C_PART, "<", 0)]) == [0, None, None]
    assert t.aggregate_grouped([C_MODE], aggs, filt=[(C_PART, "<", 0)]) == []
    # Table.aggregate left no list behind
    with pytest.raises(fl.FlsError) as e:
        t.aggregate_raw([(6, 0)])
    assert "aggregate 0:" in e.value.msg
    t.close()


def test_overflow_bound(fl):
    ii = np.iinfo(np.int64)
    full = np.array([ii.min, ii.max], dtype=np.int64)
    x = np.array([-5, 1000], dtype=np.int64)
    y = np.array([-(2**20), 2**20], dtype=np.int64)
    img = fl.write_image([("a", fl.INT64, full, fl.ENC_AUTO), ("b", fl.INT64, full[::-1].copy(), fl.ENC_AUTO),
                          ("c", fl.INT64, full, fl.ENC_AUTO), ("x", fl.INT64, x, fl.ENC_AUTO),
                          ("y", fl.INT64, y, fl.ENC_AUTO)], rowgroup=1024)
    t = fl.Connection([0]).read_image(img)
    # 2 rows x (2^63)^3 is far past 2^127
    for call in (lambda a: t.aggregate(a), lambda a: t.aggregate_grouped([3], a)):
        with pytest.raises(fl.FlsError) as e:
            call([("count",), ("sum_expr", [(0, 1, 0), (0, -1, 1), (7, 1, 2)])])
        assert e.value.code == ERR_ARG and "aggregate 1:" in e.value.msg and "may overflow 128 bits" in e.value.msg
    # the constant counts: 2 x (2^63 + 2^63 - 1)^2 reaches 2^127, 2 x (2^63)^2 = 2^127 does too
    with pytest.raises(fl.FlsError) as e:
        t.aggregate([("sum_expr", [(ii.max, -1, 0), (ii.max, -1, 1)])])
    assert "may overflow 128 bits" in e.value.msg
    with pytest.raises(fl.FlsError) as e:
        t.aggregate([("sum_expr", [(0, 1, 0), (0, 1, 1)])])
    assert "may overflow 128 bits" in e.value.msg
    # (2^62 - x) * y over small zone-map ranges: 2 x (2^62 + 5) x 2^20 is far below; the guard lets it
    # through (without a GPU the call then fails on the device, not on its arguments)
    ok = [("sum_expr", [(2**62, -1, 3), (0, 1, 4)])]
    if fl.device_count() > 0:
        assert t.aggregate(ok) == [(2**62 + 5) * -(2**20) + (2**62 - 1000) * 2**20]
    else:
        with pytest.raises(fl.FlsError) as e:
            t.aggregate(ok)
        assert e.value.code == ERR_DEVICE, e.value
    t.close()


# ------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def conn0(fl):
    conn = fl.Connection([0])
    yield conn
    conn.close()


RG = 1024
N = 2 * RG + 37     # three row groups; the last is a 37-row partial vector


@pytest.fixture(scope="module")
def widths(fl, conn0):
    """every integer-like type at its full range, three columns near +-2^38
    and a UINT64 column near 2^64 - 1"""
    rng = np.random.default_rng(20250611)
    n = N

    def full(dt):
        ii = np.iinfo(dt)
        if ii.bits == 64:
            return rand64(rng, n).view(dt)
        return rng.integers(ii.min, int(ii.max) + 1, n).astype(dt)

    def m38():
        v = rng.integers(2**37, 2**38, n)
        return np.where(rng.random(n) < 0.5, -v, v).astype(np.int64)

    u64hi = (np.uint64(2**64 - 1) - rng.integers(0, 1000, n).astype(np.uint64))
    spec = [
        ("i8", fl.INT8, full(np.int8), fl.ENC_AUTO), ("i16", fl.INT16, full(np.int16), fl.ENC_AUTO),
        ("i32", fl.INT32, full(np.int32), fl.ENC_AUTO), ("i64", fl.INT64, full(np.int64), fl.ENC_AUTO),
        ("u8", fl.UINT8, full(np.uint8), fl.ENC_AUTO), ("u16", fl.UINT16, full(np.uint16), fl.ENC_AUTO),
        ("u32", fl.UINT32, full(np.uint32), fl.ENC_AUTO), ("u64", fl.UINT64, full(np.uint64), fl.ENC_AUTO),
        ("dt", fl.DATE, rng.integers(-50000, 50001, n).astype(np.int32), fl.ENC_AUTO),
        ("dec", fl.DECIMAL, rng.integers(-9 * 10**17, 9 * 10**17 + 1, n).astype(np.int64), fl.ENC_AUTO, 18, 2),
        ("ma", fl.INT64, m38(), fl.ENC_AUTO), ("mb", fl.INT64, m38(), fl.ENC_AUTO), ("mc", fl.INT64, m38(), fl.ENC_AUTO),
        ("u64hi", fl.UINT64, u64hi, fl.ENC_AUTO),
    ]
    img = fl.write_image(spec, rowgroup=RG)
    cols = {c: s[2] for c, s in enumerate(spec)}
    t = conn0.read_image(img)
    yield img, cols, t
    t.close()


I8, I16, I32, I64, U8, U16, U32, U64, DT, DEC, MA, MB, MC, U64HI = range(14)

EXPRS = [
    # one factor: every type, both signs of s, negative and positive k
    [(5, 1, I8)], [(-7, -1, I16)], [(100, -1, I32)], [(-(2**40), 1, I64)], [(3, 1, U8)], [(-3, -1, U16)],
    [(2**33, -1, U32)], [(-1, 1, U64)], [(20000, -1, DT)], [(10**18, -1, DEC)], [(2**63 - 1, -1, I64)],
    [(-(2**63), 1, U64HI)],
    # two factors
    [(1, -1, I8), (1, 1, U8)], [(0, 1, I64), (-5, -1, U32)], [(2**62, -1, DEC), (7, 1, I16)],
    [(0, -1, U64), (3, 1, I32)], [(5, -1, U64HI), (0, 1, MA)], [(-9, 1, U16), (-(2**33), 1, DT)],
    # the same column in two and in three factors
    [(0, 1, I32), (0, 1, I32)], [(12, 1, DT), (-12, -1, DT)], [(0, 1, MA), (0, 1, MA), (0, -1, MA)],
    # three factors
    [(0, 1, I64), (1, -1, I32), (2, 1, I16)], [(9, -1, U64), (0, 1, I32), (-1, 1, I8)],
    [(2**20, 1, MA), (-(2**20), -1, MB), (1, 1, MC)], [(0, -1, MA), (0, -1, MB), (0, -1, MC)],
    [(100, -1, U8), (100, 1, U16), (0, 1, DEC)], [(-1, -1, DT), (2**31, -1, U32), (-(2**15), 1, I16)],
]


def run_chunked(t, aggs, filt=None):
    """at most 32 aggregates per call"""
    out = []
    for i in range(0, len(aggs), 32):
        t.set_filter(filt)
        try:
            out += [raw_value(v) for v in t.aggregate_raw(aggs[i:i + 32])]
        finally:
            t.set_filter(None)
    return out


@pytest.fixture(scope="module")
def widths_expected(widths):
    """(sum, count) per expression of EXPRS, unfiltered and under i32 < 0: computed once"""
    img, cols, t = widths
    out = {}
    for name, filt in (("all", None), ("i32_negative", [(I32, "<", 0)])):
        sel = filter_mask(cols, filt, N) if filt else np.ones(N, bool)
        out[name] = (filt, sel, [expect_expr(cols, e, sel) for e in EXPRS])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["all", "i32_negative"])
def test_gpu_every_width_sign_and_factor_count(fl, gpu, widths, widths_expected, name):
    img, cols, t = widths
    assert t.nrowgroups == 3 and t.nrows == N
    filt, sel, want = widths_expected[name]
    assert 0 < sel[2 * RG:].sum()                 # the partial tail vector contributes
    got = run_chunked(t, [("sum_expr", e) for e in EXPRS], filt)
    for e, g, w in zip(EXPRS, got, want):
        assert g == w, (e, g, w)
        assert g[1] == int(sel.sum())
    # Table.aggregate returns the sums alone
    assert t.aggregate([("sum_expr", e) for e in EXPRS[-8:]], filt=filt) == [w[0] for w in want[-8:]]


def test_products_pass_2_64_in_both_signs(widths):
    """the inputs do what the test above relies on: single products beyond
    +-2^64, and beyond +-2^100 for the three factors near 2^38"""
    img, cols, t = widths
    prod3 = [int(a) * int(b) * int(c) for a, b, c in zip(cols[MA], cols[MB], cols[MC])]
    assert max(prod3) > 2**100 and min(prod3) < -2**100
    prod2 = [(5 - int(u)) * int(a) for u, a in zip(cols[U64HI], cols[MA])]
    assert max(prod2) > 2**64 and min(prod2) < -2**64
    assert (cols[U64HI] > np.uint64(2**64 - 1001)).all()


@pytest.mark.gpu
def test_gpu_equals_sum_product_and_sum(fl, gpu, widths):
    img, cols, t = widths
    pairs = [(I32, I16), (DEC, I8), (U64, I32), (I64, U32), (MA, MB), (DT, DT)]
    for filt in (None, [(I32, "<", 0)]):
        got = t.aggregate([("sum_expr", [(0, 1, a), (0, 1, b)]) for a, b in pairs] +
                          [("sum_product", a, b) for a, b in pairs], filt=filt)
        assert got[:len(pairs)] == got[len(pairs):], filt
        got = t.aggregate([("sum_expr", [(0, 1, c)]) for c in range(14)] + [("sum", c) for c in range(14)], filt=filt)
        assert got[:14] == got[14:], filt


# ---- NULLs
@pytest.fixture(scope="module")
def nulls(fl, conn0):
    rng = np.random.default_rng(77)
    n = N
    a = rng.integers(-2**31, 2**31, n).astype(np.int32)
    b = rng.integers(0, 2**16, n).astype(np.uint16)
    c = rng.integers(-10**12, 10**12, n).astype(np.int64)
    va, vb, vc = rng.random(n) >= 0.3, rng.random(n) >= 0.2, rng.random(n) >= 0.5
    va[RG:2 * RG] = False            # a: row group 1 entirely NULL
    vb[2 * RG:] = True               # b: no NULL in the tail row group
    vc[2 * RG:] = False
    vc[N - 1] = True                 # c: the tail's only valid row is the last of the table
    e = rng.integers(1, 100, n).astype(np.int8)
    ve = ~va                         # e: valid exactly where a is NULL
    img = fl.write_image([("a", fl.INT32, np.ma.array(a, mask=~va), fl.ENC_AUTO),
                          ("b", fl.UINT16, np.ma.array(b, mask=~vb), fl.ENC_AUTO),
                          ("c", fl.INT64, np.ma.array(c, mask=~vc), fl.ENC_AUTO),
                          ("e", fl.INT8, np.ma.array(e, mask=~ve), fl.ENC_AUTO),
                          ("f", fl.INT32, np.arange(n, dtype=np.int32), fl.ENC_AUTO)], rowgroup=RG)
    t = conn0.read_image(img)
    yield t, {0: a, 1: b, 2: c, 3: e, 4: np.arange(n, dtype=np.int32)}, {0: va, 1: vb, 2: vc, 3: ve,
                                                                      4: np.ones(n, bool)}
    t.close()


NULL_EXPRS = [
    [(1, -1, 0)], [(-4, 1, 1)], [(10**12, -1, 2)],                     # NULLs in each column alone
    [(0, 1, 4), (1, 1, 0)], [(0, 1, 4), (0, -1, 1)], [(5, 1, 4), (0, 1, 2)],
    [(0, 1, 0), (7, -1, 1)], [(0, 1, 1), (0, 1, 2)], [(3, -1, 0), (0, 1, 2)],
    [(0, 1, 4), (2, 1, 0), (0, 1, 4)], [(1, 1, 4), (1, 1, 4), (-2, -1, 2)],
    [(0, 1, 0), (7, -1, 1), (1, 1, 2)],                                # ... and in all three together
    [(0, 1, 0), (0, 1, 3)], [(1, 1, 3), (2, 1, 1), (3, -1, 0)],        # no row contributes
]


@pytest.mark.gpu
@pytest.mark.parametrize("filt,rgs", [(None, (0, 3)), ([(4, ">=", 700)], (0, 3)), (None, (1, 2)), (None, (2, 3)),
                                      ([(0, "is_null", None)], (0, 3))],
                         ids=["all", "f_ge_700", "rg1_a_all_null", "tail", "a_is_null"])
def test_gpu_nulls_in_each_factor_column(fl, gpu, nulls, filt, rgs):
    t, cols, valid = nulls
    sel = np.zeros(N, bool)
    sel[rgs[0] * RG:min(N, rgs[1] * RG)] = True
    for col, op, val in filt or []:
        sel &= ~valid[col] if op == "is_null" else valid[col] & filter_mask(cols, [(col, op, val)], N)
    t.set_filter(filt)
    try:
        got = [raw_value(v) for v in t.aggregate_raw([("sum_expr", e) for e in NULL_EXPRS], *rgs)]
    finally:
        t.set_filter(None)
    want = [expect_expr(cols, e, sel, valid) for e in NULL_EXPRS]
    for e, g, w in zip(NULL_EXPRS, got, want):
        assert g == w, (e, g, w)
    assert got[-2:] == [(None, 0), (None, 0)]
    if rgs == (1, 2):        # every expression over a is NULL there, the others are not
        assert got[0] == (None, 0) and got[1][1] > 0
    if rgs == (2, 3) and not filt:
        assert got[2][1] == 1


# ---- reproducibility
@pytest.mark.gpu
def test_gpu_results_are_identical_across_batch_sizes(fl, gpu, widths, widths_expected, nulls, monkeypatch):
    img, cols, t = widths
    tn = nulls[0]
    aggs = [("sum_expr", e) for e in EXPRS]

    def run():   # (the batch size is read when a scan starts)
        return run_chunked(t, aggs), run_chunked(tn, [("sum_expr", e) for e in NULL_EXPRS], [(4, ">=", 700)])

    monkeypatch.delenv("FLS_SCAN_BATCH", raising=False)
    base = run()
    assert base[0] == widths_expected["all"][2]
    for batch in ("1", "3"):
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)
        assert run() == base, batch
    # the row groups sharded over two pipelines (the same GPU listed twice)
    conn2 = fl.Connection([0, 0])
    t2 = conn2.read_image(img)
    try:
        assert run_chunked(t2, aggs) == base[0], "batch 3, two pipelines"
    finally:
        t2.close()
        conn2.close()


# ---- lineitem
@pytest.mark.gpu
def test_gpu_lineitem_q1_measures(fl, gpu, conn0):
    wl, sf = "lineitem", 0.01
    t = conn0.read_image(fl.gen_image(wl, sf))
    n = t.nrows
    assert [t.schema()[c][0] for c in (C_PRICE, C_DISC, C_TAX, C_SHIPDATE)] == \
        ["l_extendedprice", "l_discount", "l_tax", "l_shipdate"]
    cols = {c: fl.gen_values(wl, c, 0, n, fl.NP_DTYPE[t.schema()[c][1]], sf) for c in (C_PRICE, C_DISC, C_TAX, C_SHIPDATE)}
    terms = [(C_SHIPDATE, "<=", Q1_DAY)]
    sel = filter_mask(cols, terms, n)
    assert sel.any() and not sel.all()
    price, disc, tax = (cols[c][sel].astype(object) for c in (C_PRICE, C_DISC, C_TAX))
    disc_price = int((price * (100 - disc)).sum())
    charge = int((price * (100 - disc) * (100 + tax)).sum())
    got = t.aggregate([("sum_expr", DISC_PRICE), ("sum_expr", CHARGE), ("count",)], filt=terms)
    assert got == [disc_price, charge, int(sel.sum())]
    t.close()
