"""`fastlanes_aggregate(path, aggregates, filter, group_by)`: the SQL face of the
grouped aggregate pushdown (extension/src/scanner/fastlanes_aggregate.cpp), run
through the extension harness.

CPU tests bind only (limit=0: names, types and the BinderException texts come
from the footer, no GPU).  GPU tests compare the returned rows with
Table.aggregate_grouped on the same file and filter, rendered as
tests/test_aggregate_sql.py renders BIGINT / DECIMAL / DATE values, or with the
arrays the file was written from."""
import datetime

import numpy as np
import pytest

from ext_harness import Ext, ExtError
from test_aggregate_sql import FIVE, FIVE_NAMES, FIVE_TYPES, Q6_TEXT, decimal_text

C_LINE, C_QTY, C_PRICE, C_DISC, C_RFLAG, C_STATUS, C_SHIPDATE, C_MODE = 3, 4, 5, 6, 8, 9, 10, 14
Q1_DAY = (datetime.date(1998, 9, 2) - datetime.date(1970, 1, 1)).days
Q1_LIST = "sum(l_quantity), sum(l_extendedprice), sum(l_extendedprice * l_discount), sum(l_discount), count(*)"
Q1_AGGS = [("sum", C_QTY), ("sum", C_PRICE), ("sum_product", C_PRICE, C_DISC), ("sum", C_DISC), ("count",)]
Q1_FILTER = "l_shipdate <= DATE '1998-09-02'"


@pytest.fixture(scope="module")
def ext(_built):
    e = Ext()
    yield e
    e.close()


def render_q1(vals):
    qty, price, prod, disc, cnt = vals
    return [decimal_text(qty, 2), decimal_text(price, 2), decimal_text(prod, 4), decimal_text(disc, 2), str(cnt)]


def render_key(k):
    return None if k is None else (k.decode() if isinstance(k, bytes) else str(k))


# ------------------------------------------------------------------ CPU tests
@pytest.fixture(scope="module")
def small_file(fl, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("gagg") / "li.fls")
    fl.gen_image("lineitem", 0.01).write(p)
    return p


@pytest.fixture(scope="module")
def typed_file(fl, tmp_path_factory):
    """a DOUBLE, a FLOAT and a BLOB column beside an integer one"""
    p = str(tmp_path_factory.mktemp("gagg") / "typed.fls")
    n = 1500
    fl.write_image([("i", fl.INT32, np.arange(n, dtype=np.int32) % 3, fl.ENC_AUTO),
                    ("d", fl.DOUBLE, np.arange(n) % 2 * 0.5, fl.ENC_AUTO),
                    ("f", fl.FLOAT, (np.arange(n) % 2).astype(np.float32), fl.ENC_AUTO),
                    ("b", fl.BLOB, [b"x", b"y"] * (n // 2), fl.ENC_DICT)], rowgroup=1024).write(p)
    return p


def test_bind_puts_the_key_columns_first(ext, small_file):
    names, types, rows = ext.query("fastlanes_aggregate", small_file, FIVE, "", "l_returnflag, l_linestatus", limit=0)
    assert names == ["l_returnflag", "l_linestatus"] + FIVE_NAMES
    assert types == ["VARCHAR", "VARCHAR"] + FIVE_TYPES and rows == []
    # named and typed as the table's columns, matched as DuckDB matches identifiers; under a filter
    names, types, rows = ext.query("fastlanes_aggregate", small_file, "count(*)", Q6_TEXT,
                                   " L_SHIPDATE ,l_linenumber,l_quantity, l_shipmode ", limit=0)
    assert names == ["l_shipdate", "l_linenumber", "l_quantity", "l_shipmode", "count(*)"]
    assert types == ["DATE", "INTEGER", "DECIMAL(15,2)", "VARCHAR", "BIGINT"] and rows == []


FIVE_KEYS = "l_returnflag, l_linestatus, l_shipmode, l_linenumber, l_shipinstruct"


@pytest.mark.parametrize("group_by,quoted", [
    ("l_returnflag, l_nosuch", '"l_nosuch"'),                          # an unknown key column
    (FIVE_KEYS, '"' + FIVE_KEYS + '"'),                                 # more than four keys
    ("l_linestatus, l_returnflag, l_linestatus", '"l_linestatus"'),     # a repeated key
    ("l_returnflag,,l_linestatus", '"l_returnflag,,l_linestatus"'),     # an empty item
    ("l_returnflag,", '"l_returnflag,"'),
    ("", '""'),
])
def test_bind_errors_quote_the_offending_text(ext, small_file, group_by, quoted):
    with pytest.raises(ExtError) as e:
        ext.query("fastlanes_aggregate", small_file, "count(*)", "", group_by, limit=0)
    assert "fastlanes_aggregate" in str(e.value) and quoted in str(e.value), e.value


@pytest.mark.parametrize("key,type_name", [("d", "DOUBLE"), ("f", "FLOAT"), ("b", "BLOB")])
def test_bind_refuses_float_and_blob_keys(ext, typed_file, key, type_name):
    with pytest.raises(ExtError) as e:
        ext.query("fastlanes_aggregate", typed_file, "count(*)", "", "i, " + key, limit=0)
    assert "fastlanes_aggregate" in str(e.value) and f'"{key}"' in str(e.value) and type_name in str(e.value), e.value
    names, types, _ = ext.query("fastlanes_aggregate", typed_file, "count(*), sum(d)", "", "i", limit=0)
    assert names == ["i", "count(*)", "sum(d)"] and types == ["INTEGER", "BIGINT", "DOUBLE"]


def test_two_and_three_argument_forms_bind_as_before(ext, small_file):
    names, types, rows = ext.query("fastlanes_aggregate", small_file, FIVE, limit=0)
    assert names == FIVE_NAMES and types == FIVE_TYPES and rows == []
    names, types, rows = ext.query("fastlanes_aggregate", small_file, FIVE, Q6_TEXT, limit=0)
    assert names == FIVE_NAMES and types == FIVE_TYPES and rows == []
    with pytest.raises(ExtError, match="No function matches"):
        ext.query("fastlanes_aggregate", small_file, FIVE, "", "l_returnflag", "extra", limit=0)


# ------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def lineitem_file(fl, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("gagg") / "li01.fls")
    fl.gen_image("lineitem", 0.1).write(p)
    conn = fl.Connection([0])
    t = conn.read_fls(p)
    yield p, t
    t.close()
    conn.close()


@pytest.mark.gpu
def test_gpu_sql_q1_matches_table_aggregate_grouped(fl, gpu, ext, lineitem_file):
    p, t = lineitem_file
    names, types, rows = ext.query("fastlanes_aggregate", p, Q1_LIST, Q1_FILTER, "l_returnflag, l_linestatus")
    assert names[:2] == ["l_returnflag", "l_linestatus"] and types[:2] == ["VARCHAR", "VARCHAR"]
    assert types[2:] == ["DECIMAL(18,2)", "DECIMAL(18,2)", "DECIMAL(18,4)", "DECIMAL(18,2)", "BIGINT"]
    want = t.aggregate_grouped([C_RFLAG, C_STATUS], Q1_AGGS, filt=[(C_SHIPDATE, "<=", Q1_DAY)])
    assert len(want) > 1 and sum(v[4] for _, v in want) < t.nrows
    assert rows == [[render_key(k) for k in key] + render_q1(vals) for key, vals in want]


@pytest.mark.gpu
def test_gpu_sql_blank_filter_means_none(fl, gpu, ext, lineitem_file):
    p, t = lineitem_file
    want = t.aggregate_grouped([C_MODE, C_LINE], Q1_AGGS)
    assert sum(v[4] for _, v in want) == t.nrows
    for blank in ("", "   "):
        names, types, rows = ext.query("fastlanes_aggregate", p, Q1_LIST, blank, "l_shipmode, l_linenumber")
        assert types[:2] == ["VARCHAR", "INTEGER"]
        assert rows == [[render_key(k) for k in key] + render_q1(vals) for key, vals in want]
    # a per-chunk refusal surfaces with the engine's message: the key is read by the filter
    with pytest.raises(ExtError) as e:
        ext.query("fastlanes_aggregate", p, "count(*)", "l_shipmode = 'AIR'", "l_linenumber, l_shipmode")
    assert "key 1:" in str(e.value) and "filter" in str(e.value), e.value


@pytest.mark.gpu
def test_gpu_sql_limit_error_names_the_limit_and_the_way_out(fl, gpu, ext, tmp_path):
    n = 2048
    p = str(tmp_path / "k65.fls")
    fl.write_image([("k65", fl.INT16, (np.arange(n) % 65).astype(np.int16), fl.ENC_AUTO)], rowgroup=1024).write(p)
    with pytest.raises(ExtError) as e:
        ext.query("fastlanes_aggregate", p, "count(*)", "", "k65")
    msg = str(e.value)
    assert "fastlanes_aggregate" in msg and "64" in msg and "read_fastlanes" in msg and "GROUP BY" in msg, msg
    # the same file within the capacity
    _, _, rows = ext.query("fastlanes_aggregate", p, "count(*)", "k65 < 64", "k65")
    assert [r[0] for r in rows] == [str(k) for k in range(64)]


@pytest.mark.gpu
def test_gpu_sql_more_groups_than_one_chunk_arrive_complete_and_in_order(fl, gpu, ext, tmp_path):
    """40 row groups of one vector, 64 keys each, all different: 2560 groups,
    more than STANDARD_VECTOR_SIZE = 2048"""
    nrg, rg = 40, 1024
    i = np.arange(nrg * rg)
    k = (i // rg * 64 + i % 64).astype(np.int32)
    x = (i * 7 % 1000 - 500).astype(np.int64)
    p = str(tmp_path / "many.fls")
    fl.write_image([("k", fl.INT32, k, fl.ENC_AUTO), ("x", fl.INT64, x, fl.ENC_AUTO)], rowgroup=rg).write(p)
    names, types, rows = ext.query("fastlanes_aggregate", p, "count(*), sum(x)", "", "k")
    assert names == ["k", "count(*)", "sum(x)"] and types == ["INTEGER", "BIGINT", "BIGINT"]
    assert len(rows) == nrg * 64
    assert rows == [[str(g), "16", str(int(x[k == g].sum()))] for g in range(nrg * 64)]
