"""`fastlanes_topn(path, order_by, k[, filter[, columns]])`: the SQL face of
the top-N pushdown (extension/src/scanner/fastlanes_topn.cpp), run through
the extension harness.

CPU tests bind only (limit=0: names, types and the BinderException texts come
from the footer, no GPU).  GPU tests compare the returned rows with Table.topn
on the same file, rendered as the harness renders BIGINT / DECIMAL / DATE
values elsewhere."""
import datetime

import numpy as np
import pytest

from ext_harness import Ext, ExtError

LI_NAMES = ["l_orderkey", "l_partkey", "l_suppkey", "l_linenumber", "l_quantity", "l_extendedprice", "l_discount",
            "l_tax", "l_returnflag", "l_linestatus", "l_shipdate", "l_commitdate", "l_receiptdate", "l_shipinstruct",
            "l_shipmode"]
LI_TYPES = ["BIGINT", "INTEGER", "INTEGER", "INTEGER", "DECIMAL(15,2)", "DECIMAL(15,2)", "DECIMAL(15,2)",
            "DECIMAL(15,2)", "VARCHAR", "VARCHAR", "DATE", "DATE", "DATE", "VARCHAR", "VARCHAR"]


@pytest.fixture(scope="module")
def ext(_built):
    e = Ext()
    yield e
    e.close()


def decimal_text(v, scale):
    s = "-" if v < 0 else ""
    v = abs(int(v))
    return f"{s}{v // 10**scale}.{v % 10**scale:0{scale}d}"


def date_text(days):
    return (datetime.date(1970, 1, 1) + datetime.timedelta(days=int(days))).isoformat()


# ------------------------------------------------------------------ CPU tests
@pytest.fixture(scope="module")
def small_file(fl, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("topn") / "li.fls")
    fl.gen_image("lineitem", 0.01).write(p)
    return p


def test_bind_names_and_types(ext, small_file):
    assert ext.has_function("fastlanes_topn")
    names, types, rows = ext.query("fastlanes_topn", small_file, "l_extendedprice DESC", 10, limit=0)
    assert names == LI_NAMES and types == LI_TYPES and rows == []
    # a listed subset comes in the listed order; columns match as in DuckDB
    names, types, rows = ext.query("fastlanes_topn", small_file, '  "L_ORDERKEY"  asc  nulls  FIRST ', 0,
                                   "l_quantity < 24", " l_shipmode ,L_SHIPDATE,l_orderkey", limit=0)
    assert names == ["l_shipmode", "l_shipdate", "l_orderkey"] and types == ["VARCHAR", "DATE", "BIGINT"]
    # a blank filter and a blank list: no filter, every column
    names, types, _ = ext.query("fastlanes_topn", small_file, "l_shipdate", 1024, " ", "", limit=0)
    assert names == LI_NAMES and types == LI_TYPES


@pytest.mark.parametrize("args,quoted", [
    (("l_nosuch DESC", 10), '"l_nosuch"'),                                     # an unknown order column
    (("l_shipmode", 10), '"l_shipmode"'),                                      # a VARCHAR order column
    (("", 10), 'order_by ""'),                                                 # malformed order_by texts
    (("l_orderkey DOWN", 10), '"down"'),
    (("l_orderkey DESC NULLS", 10), '"nulls"'),
    (("l_orderkey NULLS MIDDLE", 10), '"nulls middle"'),
    (("l_orderkey DESC ASC", 10), '"asc"'),
    (("l_orderkey, l_partkey", 10), '"l_orderkey,"'),
    (("l_orderkey", -3), '"-3"'),                                              # a negative k
    (("l_orderkey", 10, "", "l_orderkey,,l_partkey"), '"l_orderkey,,l_partkey"'),   # an empty list item
    (("l_orderkey", 10, "", "l_orderkey, l_nosuch"), '"l_nosuch"'),            # an unknown listed column
    (("l_orderkey", 10, "", "l_partkey, L_PARTKEY"), '"L_PARTKEY"'),           # a repeated one
    (("l_orderkey", 10, "l_quantity < 24 OR l_quantity > 30"), '"OR"'),        # the shared filter grammar
    (("l_orderkey", 10, "l_discount >= 0.055"), '"0.055"'),
])
def test_bind_errors_quote_the_offending_text(ext, small_file, args, quoted):
    with pytest.raises(ExtError) as e:
        ext.query("fastlanes_topn", small_file, *args, limit=0)
    msg = str(e.value)
    assert msg.startswith("fastlanes_topn: ") and quoted in msg, msg      # (a BinderException carries no class prefix)


def test_k_above_the_limit_points_at_read_fastlanes(ext, small_file):
    with pytest.raises(ExtError) as e:
        ext.query("fastlanes_topn", small_file, "l_orderkey", 1025, limit=0)
    msg = str(e.value)
    assert "1024" in msg and "read_fastlanes" in msg and "ORDER BY" in msg and "LIMIT" in msg, msg


def test_bind_argument_shapes(ext, small_file):
    with pytest.raises(ExtError, match="No function matches"):
        ext.query("fastlanes_topn", small_file, "l_orderkey", limit=0)
    with pytest.raises(ExtError, match="No function matches"):
        ext.query("fastlanes_topn", small_file, "l_orderkey", "10", limit=0)     # k as a string
    with pytest.raises(ExtError, match="Failed to open FastLanes file"):
        ext.query("fastlanes_topn", small_file + ".missing", "l_orderkey", 10, limit=0)


def test_fastlanes_aggregate_keeps_its_messages(ext, small_file):
    """the lexer and literal parser moved to a shared header: the aggregate
    function's errors still carry its own name"""
    with pytest.raises(ExtError) as e:
        ext.query("fastlanes_aggregate", small_file, "count(*)", "l_quantity < 'x'", limit=0)
    assert "fastlanes_aggregate" in str(e.value) and "fastlanes_topn" not in str(e.value)


# ------------------------------------------------------------------ GPU tests
N = 3 * 1024 + 200


@pytest.fixture(scope="module")
def sql_file(fl, tmp_path_factory):
    rng = np.random.default_rng(9)
    big = rng.integers(-10 ** 12, 10 ** 12, N, dtype=np.int64)
    dec = rng.integers(-10 ** 9, 10 ** 9, N, dtype=np.int64)
    day = rng.integers(8000, 11000, N).astype(np.int32)
    words = [b"AIR", b"MAIL", b"a shipping mode over twelve bytes", b"RAIL"]
    mode = [words[i] for i in rng.integers(0, 4, N)]
    null = rng.random(N) < 0.4
    opt = np.ma.masked_array(rng.integers(0, 100, N).astype(np.int32), mask=null)
    p = str(tmp_path_factory.mktemp("topn") / "t.fls")
    fl.write_image([("big", fl.INT64, big, fl.ENC_AUTO), ("dec", fl.DECIMAL, dec, fl.ENC_AUTO, 15, 2),
                    ("day", fl.DATE, day, fl.ENC_AUTO), ("mode", fl.VARCHAR, mode, fl.ENC_DICT),
                    ("opt", fl.INT32, opt, fl.ENC_AUTO)], rowgroup=1024).write(p)
    conn = fl.Connection([0])
    t = conn.read_fls(p)
    yield p, t
    t.close()
    conn.close()


def render(values, valid, nrows, cols):
    """Table.topn's values of the table columns `cols` as the harness renders them"""
    out = []
    for i in range(nrows):
        row = []
        for c in cols:
            if valid[c] is not None and not valid[c][i]:
                row.append(None)
            elif c == 1:
                row.append(decimal_text(values[c][i], 2))
            elif c == 2:
                row.append(date_text(values[c][i]))
            elif c == 3:
                row.append(values[c][i].decode())
            else:
                row.append(str(int(values[c][i])))
        out.append(row)
    return out


@pytest.mark.gpu
def test_gpu_sql_matches_table_topn(fl, gpu, ext, sql_file):
    p, t = sql_file
    names, types, rows = ext.query("fastlanes_topn", p, "dec DESC", 25)
    assert names == ["big", "dec", "day", "mode", "opt"]
    assert types == ["BIGINT", "DECIMAL(15,2)", "DATE", "VARCHAR", "INTEGER"]
    r, values, valid = t.topn(1, 25, desc=True)
    assert len(r) == 25 and rows == render(values, valid, 25, range(5))
    assert any(v is None for row in rows for v in row)       # the NULLs of `opt` come through
    # with a filter and a column list (in the listed order)
    _, _, rows = ext.query("fastlanes_topn", p, "big", 100, "day >= DATE '1995-01-01' AND mode = 'MAIL'", "mode, big,day")
    r, values, valid = t.topn(0, 100, filt=[(2, ">=", 9131), (3, "=", "MAIL")])
    assert len(r) == 100 and rows == render(values, valid, 100, [3, 0, 2])
    assert all(row[0] == "MAIL" for row in rows)


@pytest.mark.gpu
def test_gpu_sql_desc_nulls_first_and_k_past_the_table(fl, gpu, ext, sql_file):
    p, t = sql_file
    _, _, rows = ext.query("fastlanes_topn", p, "opt DESC NULLS FIRST", 1024, "", "opt,big")
    r, values, valid = t.topn(4, 1024, desc=True, nulls_first=True)
    assert rows == render(values, valid, 1024, [4, 0])
    assert rows[0][0] is None and rows[-1][0] is None        # more than 1024 NULLs: they fill the result
    # fewer qualifying rows than k: that many, in chunks that end when the result does
    filt_text, filt = "day < DATE '1992-01-01'", [(2, "<", 8035)]
    _, _, rows = ext.query("fastlanes_topn", p, "day desc nulls last", 1024, filt_text)
    r, values, valid = t.topn(2, 1024, filt=filt, desc=True)
    assert 0 < len(r) < 1024 and rows == render(values, valid, len(r), range(5))
    # k larger than a small table
    _, _, rows = ext.query("fastlanes_topn", p, "big", 1024, "big >= 0 AND opt IS NOT NULL AND day = DATE '1995-06-01'")
    r, values, valid = t.topn(0, 1024, filt=[(0, ">=", 0), (4, "is_not_null", None), (2, "=", 9282)])
    assert rows == render(values, valid, len(r), range(5))
    _, _, rows = ext.query("fastlanes_topn", p, "big", 0)
    assert rows == []
