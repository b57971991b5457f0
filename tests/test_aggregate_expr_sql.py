"""`sum(F * F [* F])` and `sum(F)` over affine factors in
`fastlanes_aggregate(path, aggregates[, filter[, group_by]])`
(extension/src/scanner/fastlanes_aggregate.cpp), run through the extension
harness: a factor is a column, `(literal - column)`, `(literal + column)`,
`(column + literal)` or `(column - literal)`.

CPU tests bind only (limit=0: names, types and the BinderException texts come
from the footer, no GPU).  GPU tests compare the returned rows with
Table.aggregate / Table.aggregate_grouped on the same file and filter, rendered
as tests/test_aggregate_sql.py renders BIGINT / DECIMAL values."""
import datetime

import numpy as np
import pytest

from ext_harness import Ext, ExtError
from test_aggregate_sql import decimal_text

C_QTY, C_PRICE, C_DISC, C_TAX, C_RFLAG, C_STATUS, C_SHIPDATE = 4, 5, 6, 7, 8, 9, 10
Q1_DAY = (datetime.date(1998, 9, 2) - datetime.date(1970, 1, 1)).days
DISC_PRICE_SQL = "sum(l_extendedprice * (1 - l_discount))"
CHARGE_SQL = "sum(l_extendedprice * (1 - l_discount) * (1 + l_tax))"
Q1_LIST = f"sum(l_quantity), sum(l_extendedprice), {DISC_PRICE_SQL}, {CHARGE_SQL}, sum(l_discount), count(*)"
Q1_AGGS = [("sum", C_QTY), ("sum", C_PRICE), ("sum_expr", [(0, 1, C_PRICE), (100, -1, C_DISC)]),
           ("sum_expr", [(0, 1, C_PRICE), (100, -1, C_DISC), (100, 1, C_TAX)]), ("sum", C_DISC), ("count",)]
Q1_TYPES = ["DECIMAL(18,2)", "DECIMAL(18,2)", "DECIMAL(18,4)", "DECIMAL(18,6)", "DECIMAL(18,2)", "BIGINT"]
Q1_FILTER = "l_shipdate <= DATE '1998-09-02'"


@pytest.fixture(scope="module")
def ext(_built):
    e = Ext()
    yield e
    e.close()


def render_q1(vals):
    qty, price, disc_price, charge, disc, cnt = vals
    return [decimal_text(qty, 2), decimal_text(price, 2), decimal_text(disc_price, 4), decimal_text(charge, 6),
            decimal_text(disc, 2), str(cnt)]


# ------------------------------------------------------------------ CPU tests
@pytest.fixture(scope="module")
def small_file(fl, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("aggx") / "li.fls")
    fl.gen_image("lineitem", 0.01).write(p)
    return p


@pytest.fixture(scope="module")
def typed_file(fl, tmp_path_factory):
    """integer columns of several widths, a DECIMAL(18, 10), a DOUBLE and a FLOAT"""
    p = str(tmp_path_factory.mktemp("aggx") / "typed.fls")
    n = 1500
    i = np.arange(n)
    fl.write_image([("i", fl.INT32, (i % 7 - 3).astype(np.int32), fl.ENC_AUTO),
                    ("u", fl.UINT64, (i * 3).astype(np.uint64), fl.ENC_AUTO),
                    ("s", fl.INT16, (i % 5).astype(np.int16), fl.ENC_AUTO),
                    ("w", fl.DECIMAL, (i * 11).astype(np.int64), fl.ENC_AUTO, 18, 10),
                    ("d", fl.DOUBLE, i * 0.5, fl.ENC_AUTO),
                    ("f", fl.FLOAT, i.astype(np.float32), fl.ENC_AUTO)], rowgroup=1024).write(p)
    return p


def test_bind_names_and_types(ext, small_file):
    names, types, rows = ext.query("fastlanes_aggregate", small_file, Q1_LIST, limit=0)
    assert names == [s.strip() for s in Q1_LIST.split(",")] and types == Q1_TYPES and rows == []
    # names are the items' trimmed text; every factor form; the grouped form puts its keys first
    items = [" sum( (1 - l_discount) ) ", "SUM((l_tax + 0.5)*(L_DISCOUNT - 1))", "sum((-2+l_linenumber) * l_quantity)",
             "sum(l_extendedprice * l_discount)", "sum(l_linenumber*l_linenumber*(3 - l_linenumber))"]
    names, types, rows = ext.query("fastlanes_aggregate", small_file, ",".join(items), Q1_FILTER,
                                   "l_returnflag, l_linestatus", limit=0)
    assert names == ["l_returnflag", "l_linestatus"] + [s.strip() for s in items]
    assert types == ["VARCHAR", "VARCHAR", "DECIMAL(18,2)", "DECIMAL(18,4)", "DECIMAL(18,2)", "DECIMAL(18,4)", "BIGINT"]


def test_bind_integer_columns_give_bigint(ext, typed_file):
    names, types, rows = ext.query("fastlanes_aggregate", typed_file,
                                   "sum(i * (10 - s)), sum((u + 1) * i * s), sum((7 - i)), sum(i * s), sum(w * (2 + i))",
                                   limit=0)
    assert types == ["BIGINT", "BIGINT", "BIGINT", "BIGINT", "DECIMAL(18,10)"] and rows == []


@pytest.mark.parametrize("item,quoted", [
    ("sum(l_extendedprice * (0.055 - l_discount))", '"0.055"'),          # a literal the scale cannot hold
    ("sum((1.5 + l_linenumber))", '"1.5"'),                              # ... nor an integer column
    ("sum((x - l_discount))", '"x"'),                                    # not a literal
    ("sum(l_extendedprice * (1 - l_shipmode))", '"l_shipmode"'),         # a string factor column
    ("sum(l_quantity * l_shipmode * l_tax)", '"l_shipmode"'),
    ("sum(l_quantity * l_discount * l_tax * l_extendedprice)",
     '"sum(l_quantity * l_discount * l_tax * l_extendedprice)"'),        # more than three factors
    ("sum(l_quantity * ((1 - l_discount)))", '"sum(l_quantity * ((1 - l_discount)))"'),    # nested parentheses
    ("sum(l_quantity * (1 - l_discount)", '"sum(l_quantity * (1 - l_discount)"'),          # unbalanced
    ("sum(l_quantity * 1 - l_discount))", '"sum(l_quantity * 1 - l_discount))"'),
    ("sum(l_quantity * (1 + 2))", '"(1 + 2)"'),                          # a literal-only factor
    ("sum(l_quantity * (l_tax + l_discount))", '"(l_tax + l_discount)"'),  # two columns in a factor
    ("sum(l_quantity * (l_tax))", '"(l_tax)"'),                          # no operator
    ("sum(l_quantity * (1 - l_nosuch))", '"(1 - l_nosuch)"'),
    ("min(l_quantity * (1 - l_discount))", '"min(l_quantity * (1 - l_discount))"'),      # products are for sum
    ("sum(l_quantity * )", '""'),
])
def test_bind_errors_quote_the_offending_text(ext, small_file, item, quoted):
    for extra in ((), (Q1_FILTER, "l_returnflag")):
        with pytest.raises(ExtError) as e:
            ext.query("fastlanes_aggregate", small_file, "count(*), " + item, *extra, limit=0)
        assert "fastlanes_aggregate" in str(e.value) and quoted in str(e.value), e.value


@pytest.mark.parametrize("item,quoted", [
    ("sum(w * w)", '"sum(w * w)"'),                                      # the scales add up past 18
    ("sum(w * (1 - w))", '"sum(w * (1 - w))"'),
    ("sum(i * (1 - d))", '"d"'),                                         # DOUBLE / FLOAT factor columns
    ("sum((f + 1) * i)", '"f"'),
    ("sum((18446744073709551615 - u))", '"18446744073709551615"'),       # a constant past int64
])
def test_bind_errors_by_column_type(ext, typed_file, item, quoted):
    with pytest.raises(ExtError) as e:
        ext.query("fastlanes_aggregate", typed_file, item, limit=0)
    assert "fastlanes_aggregate" in str(e.value) and quoted in str(e.value), e.value


# ------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def lineitem_file(fl, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("aggx") / "li01.fls")
    fl.gen_image("lineitem", 0.1).write(p)
    conn = fl.Connection([0])
    t = conn.read_fls(p)
    yield p, t
    t.close()
    conn.close()


@pytest.mark.gpu
def test_gpu_sql_full_q1_matches_table_aggregate_grouped(fl, gpu, ext, lineitem_file):
    p, t = lineitem_file
    names, types, rows = ext.query("fastlanes_aggregate", p, Q1_LIST, Q1_FILTER, "l_returnflag, l_linestatus")
    assert names[:2] == ["l_returnflag", "l_linestatus"] and types == ["VARCHAR", "VARCHAR"] + Q1_TYPES
    want = t.aggregate_grouped([C_RFLAG, C_STATUS], Q1_AGGS, filt=[(C_SHIPDATE, "<=", Q1_DAY)])
    assert len(want) > 1 and sum(v[5] for _, v in want) < t.nrows
    assert rows == [[k.decode() for k in key] + render_q1(vals) for key, vals in want]
    # the expression list is set per query and cleared after it: a second query gives the same rows
    assert ext.query("fastlanes_aggregate", p, Q1_LIST, Q1_FILTER, "l_returnflag, l_linestatus")[2] == rows


@pytest.mark.gpu
def test_gpu_sql_ungrouped_q1_matches_table_aggregate(fl, gpu, ext, lineitem_file):
    p, t = lineitem_file
    names, types, rows = ext.query("fastlanes_aggregate", p, Q1_LIST, Q1_FILTER)
    assert types == Q1_TYPES
    want = t.aggregate(Q1_AGGS, filt=[(C_SHIPDATE, "<=", Q1_DAY)])
    assert rows == [render_q1(want)]
    # the other factor forms, against the same sums written with the Python tuples
    _, types, rows = ext.query("fastlanes_aggregate", p,
                               "sum((l_discount - 1) * l_extendedprice), sum((0.02 + l_tax)), "
                               "sum((l_linenumber + -3) * (5 - l_linenumber) * l_linenumber)", Q1_FILTER)
    assert types == ["DECIMAL(18,4)", "DECIMAL(18,2)", "BIGINT"]
    want = t.aggregate([("sum_expr", [(-100, 1, C_DISC), (0, 1, C_PRICE)]), ("sum_expr", [(2, 1, C_TAX)]),
                        ("sum_expr", [(-3, 1, 3), (5, -1, 3), (0, 1, 3)])], filt=[(C_SHIPDATE, "<=", Q1_DAY)])
    assert rows == [[decimal_text(want[0], 4), decimal_text(want[1], 2), str(want[2])]]
