"""`fastlanes_aggregate(path, aggregates[, filter])`: the SQL face of the
aggregate pushdown (extension/src/scanner/fastlanes_aggregate.cpp), run
through the extension harness.

CPU tests bind only (limit=0: names, types and the BinderException texts come
from the footer, no GPU).  GPU tests compare the one returned row with
Table.aggregate on the same file and filter, rendered as the harness renders
BIGINT / DECIMAL / DATE values elsewhere."""
import datetime

import numpy as np
import pytest

from ext_harness import Ext, ExtError

C_PART, C_QTY, C_PRICE, C_DISC, C_SHIPDATE = 1, 4, 5, 6, 10
DAY_1994, DAY_1995 = 8766, 9131
Q6 = [(C_SHIPDATE, ">=", DAY_1994), (C_SHIPDATE, "<", DAY_1995), (C_DISC, ">=", 5), (C_DISC, "<=", 7),
      (C_QTY, "<", 2400)]
Q6_TEXT = ("l_shipdate >= DATE '1994-01-01' AND l_shipdate < DATE '1995-01-01' AND l_discount >= 0.05 "
           "AND l_discount <= 0.07 AND l_quantity < 24")
FIVE = "count(*), sum(l_quantity), min(l_shipdate), max(l_extendedprice), sum(l_extendedprice * l_discount)"
FIVE_AGGS = [("count",), ("sum", C_QTY), ("min", C_SHIPDATE), ("max", C_PRICE), ("sum_product", C_PRICE, C_DISC)]
FIVE_NAMES = ["count(*)", "sum(l_quantity)", "min(l_shipdate)", "max(l_extendedprice)",
              "sum(l_extendedprice * l_discount)"]
FIVE_TYPES = ["BIGINT", "DECIMAL(18,2)", "DATE", "DECIMAL(15,2)", "DECIMAL(18,4)"]


@pytest.fixture(scope="module")
def ext(_built):
    e = Ext()
    yield e
    e.close()


def decimal_text(v, scale):
    if v is None:
        return None
    s = "-" if v < 0 else ""
    v = abs(v)
    return f"{s}{v // 10**scale}.{v % 10**scale:0{scale}d}"


def date_text(days):
    return None if days is None else (datetime.date(1970, 1, 1) + datetime.timedelta(days=days)).isoformat()


def render_five(vals):
    cnt, qty, ship, price, prod = vals
    return [str(cnt), decimal_text(qty, 2), date_text(ship), decimal_text(price, 2), decimal_text(prod, 4)]


# ------------------------------------------------------------------ CPU tests
@pytest.fixture(scope="module")
def small_file(fl, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("agg") / "li.fls")
    fl.gen_image("lineitem", 0.01).write(p)
    return p


def test_bind_names_and_types(ext, small_file):
    assert ext.has_function("fastlanes_aggregate")
    names, types, rows = ext.query("fastlanes_aggregate", small_file, FIVE, limit=0)
    assert names == FIVE_NAMES and types == FIVE_TYPES and rows == []
    # the three-argument form; names are the items' trimmed text, columns match as in DuckDB
    names, types, rows = ext.query("fastlanes_aggregate", small_file,
                                   "  count(l_shipmode) ,SUM(L_LINENUMBER),max( l_orderkey )", Q6_TEXT, limit=0)
    assert names == ["count(l_shipmode)", "SUM(L_LINENUMBER)", "max( l_orderkey )"]
    assert types == ["BIGINT", "BIGINT", "BIGINT"] and rows == []


@pytest.mark.parametrize("args,quoted", [
    (("sum(l_nosuch)",), '"l_nosuch"'),                                        # an unknown column
    (("count(*), avg(l_quantity)",), '"avg"'),                                 # an unknown function
    (("sum(l_shipmode)",), '"sum(l_shipmode)"'),                               # sum of a VARCHAR column
    (("count(*)", "l_discount >= 0.055"), '"0.055"'),                          # too many fractional digits
    (("count(*)", "l_quantity < 24 OR l_quantity > 30"), '"OR"'),              # an OR in the filter
    (("count(*)", "(l_quantity < 24)"), '"("'),
    (("count(*)", "l_nosuch = 1"), '"l_nosuch"'),
    (("count(*)", "l_shipdate >= '1994-01-01'"), "'1994-01-01'"),               # ill-typed literals
    (("count(*)", "l_quantity < 'x'"), "'x'"),
    (("sum(l_quantity * l_shipmode)",), '"l_shipmode"'),
    (("min(l_quantity",), '"min(l_quantity"'),
])
def test_bind_errors_quote_the_offending_text(ext, small_file, args, quoted):
    with pytest.raises(ExtError) as e:
        ext.query("fastlanes_aggregate", small_file, *args, limit=0)
    assert "fastlanes_aggregate" in str(e.value) and quoted in str(e.value), e.value


def test_bind_needs_two_or_three_string_arguments(ext, small_file):
    with pytest.raises(ExtError, match="No function matches"):
        ext.query("fastlanes_aggregate", small_file, limit=0)
    with pytest.raises(ExtError, match="Failed to open FastLanes file"):
        ext.query("fastlanes_aggregate", small_file + ".missing", "count(*)", limit=0)


# ------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def lineitem_file(fl, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("agg") / "li01.fls")
    fl.gen_image("lineitem", 0.1).write(p)
    conn = fl.Connection([0])
    t = conn.read_fls(p)
    yield p, t
    t.close()
    conn.close()


@pytest.mark.gpu
def test_gpu_sql_q6_matches_table_aggregate(fl, gpu, ext, lineitem_file):
    p, t = lineitem_file
    names, types, rows = ext.query("fastlanes_aggregate", p, FIVE, Q6_TEXT)
    assert names == FIVE_NAMES and types == FIVE_TYPES
    want = t.aggregate(FIVE_AGGS, filt=Q6)
    assert want[0] > 0
    assert rows == [render_five(want)]


@pytest.mark.gpu
def test_gpu_sql_without_filter(fl, gpu, ext, lineitem_file):
    p, t = lineitem_file
    _, _, rows = ext.query("fastlanes_aggregate", p, FIVE)
    want = t.aggregate(FIVE_AGGS)
    assert want[0] == t.nrows
    assert rows == [render_five(want)]


@pytest.mark.gpu
def test_gpu_sql_everything_pruned(fl, gpu, ext, lineitem_file):
    p, t = lineitem_file
    _, _, rows = ext.query("fastlanes_aggregate", p, FIVE, "l_partkey < 0")
    assert rows == [["0", None, None, None, None]]


@pytest.mark.gpu
def test_gpu_sql_sum_past_64_bits_is_out_of_range(fl, gpu, ext, tmp_path):
    rng = np.random.default_rng(5)
    n = 2 * 2048 + 1024 + 37
    big = (rng.integers(0, 1 << 62, n, dtype=np.int64) | np.int64(1 << 62))     # [2^62, 2^63)
    p = str(tmp_path / "big.fls")
    fl.write_image([("big", fl.INT64, big, fl.ENC_AUTO)], rowgroup=2048).write(p)
    with pytest.raises(ExtError) as e:
        ext.query("fastlanes_aggregate", p, "count(*), sum(big)")
    assert "Out of Range Error" in str(e.value) and "sum(big)" in str(e.value) and "BIGINT" in str(e.value), e.value
    # min / max / count of the same column fit and are delivered
    _, _, rows = ext.query("fastlanes_aggregate", p, "count(big), min(big), max(big)")
    assert rows == [[str(n), str(int(big.min())), str(int(big.max()))]]
