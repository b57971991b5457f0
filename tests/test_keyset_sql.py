"""The SQL faces of the key-set filter terms, through
the extension harness: read_fastlanes maps an InFilter of more than 16 values
on an integer-like column to one key-set term, and the filter text of
fastlanes_aggregate / fastlanes_topn learns `column [NOT] IN (literal, ...)`.

The harness shows a query's rows, not the terms the scan pushed down: whether
a list went through a key set or through EQ terms cannot be observed from
here, so the read_fastlanes tests assert results only -- a list on either side
of the 16-value threshold against numpy and against the other path's rows.

CPU tests bind only (limit=0: the BinderException texts come from the footer)."""
import datetime

import numpy as np
import pytest

from ext_harness import Ext, ExtError

RG = 1024
N = 5 * 1024 + 333
C_ID, C_K, C_D, C_P, C_S, C_N = range(6)
MODES = ["AIR", "MAIL", "RAIL", "SHIP", "TRUCK", "FOB", "REG AIR"] + [f"mode{i:02d}" for i in range(20)]
EPOCH = datetime.date(1970, 1, 1)


@pytest.fixture(scope="module")
def ext(_built):
    e = Ext()
    yield e
    e.close()


@pytest.fixture(scope="module")
def table(fl, tmp_path_factory):
    """id (row number), k BIGINT sorted with repeats, d DATE, p DECIMAL(15,2),
    s VARCHAR of 27 values, n INTEGER with NULLs"""
    rng = np.random.default_rng(5)
    ids = np.arange(N, dtype=np.int32)
    k = np.sort(rng.integers(0, 9000, N)).astype(np.int64)
    d = rng.integers(8766, 8766 + 400, N).astype(np.int32)
    p = rng.integers(0, 300, N).astype(np.int64) * 25
    s = [MODES[i] for i in rng.integers(0, len(MODES), N)]
    nv = rng.integers(0, 40, N).astype(np.int32)
    null = rng.random(N) < 0.25
    path = str(tmp_path_factory.mktemp("ksql") / "t.fls")
    fl.write_image([("id", fl.INT32, ids, fl.ENC_AUTO), ("k", fl.INT64, k, fl.ENC_AUTO),
                    ("d", fl.DATE, d, fl.ENC_AUTO), ("p", fl.DECIMAL, p, fl.ENC_AUTO, 15, 2),
                    ("s", fl.VARCHAR, s, fl.ENC_DICT), ("n", fl.INT32, np.ma.masked_array(nv, mask=null), fl.ENC_AUTO)],
                   rowgroup=RG, path=path)
    return path, {"id": ids, "k": k, "d": d, "p": p, "s": np.array(s), "n": nv, "n_valid": ~null}


def date_text(days):
    return (EPOCH + datetime.timedelta(days=int(days))).isoformat()


def dec_text(v):
    return f"{int(v) // 100}.{int(v) % 100:02d}"


# ------------------------------------------------------------------ CPU tests
FUNCS = [("fastlanes_aggregate", ("count(*)",), ()), ("fastlanes_topn", ("id", 5), ())]


@pytest.mark.parametrize("fn,head,tail", FUNCS)
@pytest.mark.parametrize("text,quoted", [
    ("k IN ()", ['"k"', "empty", '"k IN ()"']),                                   # an empty list
    ("k NOT IN ( )", ['"k"', "empty", '"k NOT IN ( )"']),
    ("k IN (1, 'x')", ["\"'x'\" is not a number", '"k IN (1, \'x\')"']),           # literals of the wrong type
    ("d IN (DATE '1994-01-01', 8766)", ['"8766"']),
    ("s IN ('AIR', 5)", ['"5"']),
    ("p NOT IN (1.5, 2.555)", ['"2.555"']),
    ("k IN 1, 2", ['"("', '"k IN 1, 2"']),                                        # a missing parenthesis
    ("k IN (1, 2", ['")" is missing after the IN list', '"k IN (1, 2"']),
    ("k IN (1, 2 AND id < 5", ['"AND"']),
    ("k NOT IN (1,", ['")" is missing after the NOT IN list', '"k NOT IN (1,"']),
    ("k NOT 5", ["NOT IN", '"k NOT 5"']),
    ("k IN (1 2)", ['"2"']),
])
def test_in_list_bind_errors_quote_the_text(ext, table, fn, head, tail, text, quoted):
    path, _ = table
    with pytest.raises(ExtError) as e:
        ext.query(fn, path, *head, text, *tail, limit=0)
    msg = str(e.value)
    assert msg.startswith(fn + ": "), msg
    for q in quoted:
        assert q in msg, (q, msg)


@pytest.mark.parametrize("fn,head,tail", FUNCS)
def test_in_lists_bind_without_a_gpu(ext, table, fn, head, tail):
    path, _ = table
    for text in ("k IN (1, 2, 3)", "k in (1,2,3) AND d NOT IN (DATE '1994-01-01') and id < 7",
                 "s IN ('AIR', 'it''s') AND p NOT IN (1.25, 2.5) AND n IN (NULL, 4)",
                 '"k" NOT IN (-5, NULL)', "n IN (NULL)"):
        names, _, rows = ext.query(fn, path, *head, text, *tail, limit=0)
        assert names and rows == []


def test_read_fastlanes_binds_long_in_lists_without_a_gpu(ext, table):
    path, _ = table
    for n in (16, 17, 3000):
        names, _, rows = ext.query("read_fastlanes", path, proj=[C_ID], limit=0,
                                   where=[(C_K, "IN " + "|".join(str(3 * i) for i in range(n)))])
        assert names == ["id"] and rows == []


# ------------------------------------------------------------------ GPU tests
def in_rows(ext, path, col, values, proj=(C_ID,), **kw):
    return ext.query("read_fastlanes", path, proj=list(proj), where=[(col, "IN " + "|".join(map(str, values)))],
                     **kw)[2]


@pytest.mark.gpu
def test_gpu_read_fastlanes_in_lists_around_the_threshold(fl, gpu, ext, table):
    path, cols = table
    rng = np.random.default_rng(6)
    present = np.unique(cols["k"])
    v17 = [int(x) for x in rng.choice(present, 15, replace=False)] + [-3, 20000]    # two values that match nothing
    v16 = v17[:16]
    rows16, rows17 = in_rows(ext, path, C_K, v16, proj=(C_ID, C_K)), in_rows(ext, path, C_K, v17, proj=(C_ID, C_K))
    for vals, rows in ((v16, rows16), (v17, rows17)):
        want = np.nonzero(np.isin(cols["k"], vals))[0]
        assert len(want) > 0
        assert rows == [[str(i), str(cols["k"][i])] for i in want], len(vals)      # the host filter's rows
    # 17 values (a key set) against the 16-value path: its rows plus the 17th value's
    extra = in_rows(ext, path, C_K, [v17[16]], proj=(C_ID, C_K))
    assert sorted(rows17, key=lambda r: int(r[0])) == sorted(rows16 + extra, key=lambda r: int(r[0]))
    # 3,000 values, against numpy and against the same list as EQ terms (an InFilter's values under an OR)
    v3000 = [int(x) for x in rng.choice(9000, 3000, replace=False)]
    rows = in_rows(ext, path, C_K, v3000)
    want = np.nonzero(np.isin(cols["k"], v3000))[0]
    assert 0 < len(want) < N and rows == [[str(i)] for i in want]
    eq = ext.query("read_fastlanes", path, proj=[C_ID],
                   where=[(C_K, "OR " + "|".join(f"= {v}" for v in v3000))])[2]
    assert eq == rows
    # with other pushed-down terms, a second thread count, and on a DATE column
    dates = sorted({int(x) for x in rng.choice(cols["d"], 40)})
    got = ext.query("read_fastlanes", path, proj=[C_ID], threads=4,
                    where=[(C_K, "IN " + "|".join(map(str, v3000))), (C_D, "IN " + "|".join(map(date_text, dates))),
                           (C_ID, ">= 100")])[2]
    m = np.isin(cols["k"], v3000) & np.isin(cols["d"], dates) & (cols["id"] >= 100)
    assert m.any() and got == [[str(i)] for i in np.nonzero(m)[0]]
    # a set with no key in the table prunes every row group
    assert in_rows(ext, path, C_K, [20000 + i for i in range(17)]) == []
    # NULL rows of the probed column never match
    nvals = list(range(0, 34, 2))
    assert len(nvals) == 17
    want = np.nonzero(np.isin(cols["n"], nvals) & cols["n_valid"])[0]
    assert in_rows(ext, path, C_N, nvals) == [[str(i)] for i in want]


@pytest.mark.gpu
def test_gpu_read_fastlanes_long_varchar_list_stays_eq_terms(fl, gpu, ext, table):
    path, cols = table
    vals = MODES[3:20]
    assert len(vals) == 17
    rows = in_rows(ext, path, C_S, vals, proj=(C_ID, C_S))
    want = np.nonzero(np.isin(cols["s"], vals))[0]
    assert 0 < len(want) < N and rows == [[str(i), str(cols["s"][i])] for i in want]


IN_TEXTS = [
    ("k IN (%s)", "k", lambda c: [int(x) for x in np.unique(c["k"])[::7][:40]] + [-1, 99999], str),
    ("d IN (%s)", "d", lambda c: sorted({int(x) for x in c["d"][::50]}), lambda v: f"DATE '{date_text(v)}'"),
    ("p IN (%s)", "p", lambda c: sorted({int(x) for x in c["p"][::40]}) + [1], dec_text),
    ("s IN (%s)", "s", lambda c: ["AIR", "mode03", "REG AIR", "nosuch"], lambda v: f"'{v}'"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("text,col,values,lit", IN_TEXTS, ids=[t[1] for t in IN_TEXTS])
def test_gpu_filter_text_in_lists(fl, gpu, ext, table, text, col, values, lit, negate):
    path, cols = table
    vals = values(cols)
    filt = (text.replace(" IN ", " NOT IN ") if negate else text) % ", ".join(lit(v) for v in vals)
    m = np.isin(cols[col], vals)
    if negate:
        m = ~m
    m2 = m & (cols["id"] >= 70)
    assert 0 < m2.sum() < N
    # fastlanes_aggregate: count(*), sum(k), min(id) under the list and an ordinary term
    _, _, rows = ext.query("fastlanes_aggregate", path, "count(*), sum(k), min(id)", filt + " AND id >= 70")
    assert rows == [[str(int(m2.sum())), str(int(cols["k"][m2].sum())), str(int(cols["id"][m2].min()))]]
    # fastlanes_topn: the 50 largest k (ties by row) under the list alone
    _, _, rows = ext.query("fastlanes_topn", path, "k DESC", 50, filt, "id, k")
    cand = np.nonzero(m)[0]
    order = cand[np.lexsort((cand, -cols["k"][cand]))][:50]
    assert rows == [[str(i), str(cols["k"][i])] for i in order]


@pytest.mark.gpu
def test_gpu_null_in_a_list_follows_sql(fl, gpu, ext, table):
    path, cols = table
    count = lambda filt: int(ext.query("fastlanes_aggregate", path, "count(*)", filt)[2][0][0])   # noqa: E731
    valid = cols["n_valid"]
    some = int((np.isin(cols["n"], [3, 5]) & valid).sum())
    assert some > 0
    assert count("n IN (3, 5)") == some
    assert count("n IN (3, NULL, 5)") == some                   # a NULL in an IN list is ignored
    assert count("n IN (NULL)") == 0
    assert count("n NOT IN (3, 5)") == int((~np.isin(cols["n"], [3, 5]) & valid).sum())   # NULL rows match neither
    assert count("n NOT IN (3, NULL)") == 0                     # a NULL in a NOT IN list leaves no row
    assert count("s IN ('AIR', NULL)") == int((cols["s"] == "AIR").sum())
    assert count("s NOT IN ('AIR', NULL)") == 0
    assert count("s NOT IN ('AIR', 'MAIL')") == int((~np.isin(cols["s"], ["AIR", "MAIL"])).sum())
    _, _, rows = ext.query("fastlanes_topn", path, "id", 5, "n NOT IN (NULL)", "id")
    assert rows == []
