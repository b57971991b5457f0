"""The SQL face of the column-to-column filter terms,
through the extension harness: the filter text of fastlanes_aggregate /
fastlanes_topn learns `column op column`.  The right side is a column when it
is an identifier the schema resolves and neither NULL nor the start of a typed
literal (DATE '...').

CPU tests bind only (limit=0: the BinderException texts come from the footer).
GPU tests compare the SQL functions with numpy under the same terms."""
import numpy as np
import pytest

from ext_harness import Ext, ExtError

RG = 1024
N = 2 * 1024 + 37
MODES = ["AIR", "MAIL", "RAIL", "SHIP", "TRUCK"]


@pytest.fixture(scope="module")
def ext(_built):
    e = Ext()
    yield e
    e.close()


@pytest.fixture(scope="module")
def table(fl, tmp_path_factory):
    """id (row number), three DATE columns d0 d1 d2 (d2 with NULLs), a and b
    BIGINT from a small pool, u UTINYINT, k BIGINT, s and r VARCHAR, f DOUBLE
    (small integers, NaN and both infinities),
    and a DATE column named like the keyword: "date" """
    rng = np.random.default_rng(11)
    ids = np.arange(N, dtype=np.int32)
    d0, d1, d2 = (rng.integers(9000, 9040, N).astype(np.int32) for _ in range(3))
    null = rng.random(N) < 0.2
    a, b = (rng.integers(-3, 4, N).astype(np.int64) for _ in range(2))
    u = rng.integers(0, 7, N).astype(np.uint8)
    k = rng.integers(0, 5000, N).astype(np.int64)
    s = [MODES[i] for i in rng.integers(0, len(MODES), N)]
    f = rng.integers(-3, 4, N).astype(np.float64)
    f[rng.random(N) < 0.1] = np.nan
    f[rng.random(N) < 0.1] = np.inf
    f[rng.random(N) < 0.05] = -np.inf
    dk = rng.integers(9000, 9040, N).astype(np.int32)
    path = str(tmp_path_factory.mktemp("colsql") / "t.fls")
    A = fl.ENC_AUTO
    fl.write_image([("id", fl.INT32, ids, A), ("d0", fl.DATE, d0, A), ("d1", fl.DATE, d1, A),
                    ("d2", fl.DATE, np.ma.masked_array(d2, mask=null), A), ("a", fl.INT64, a, A), ("b", fl.INT64, b, A),
                    ("u", fl.UINT8, u, A), ("k", fl.INT64, k, A), ("s", fl.VARCHAR, s, fl.ENC_DICT),
                    ("r", fl.VARCHAR, s, fl.ENC_DICT), ("f", fl.DOUBLE, f, A), ("date", fl.DATE, dk, A)],
                   rowgroup=RG, path=path)
    return path, {"id": ids, "d0": d0, "d1": d1, "d2": d2, "d2_valid": ~null, "a": a, "b": b, "u": u, "k": k,
                  "s": np.array(s), "f": f, "date": dk}


FUNCS = [("fastlanes_aggregate", ("count(*)",), ()), ("fastlanes_topn", ("id", 5), ())]


# ------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("fn,head,tail", FUNCS)
@pytest.mark.parametrize("text,quoted", [
    ("d1 < nosuch", ['"nosuch"', "not found", '"d1 < nosuch"']),                            # an unknown right identifier
    ("a <> B2 AND id < 5", ['"B2"', "not found"]),
    ("s = r", ['"s"', '"r"', "VARCHAR", "strings are compared with constants only", '"s = r"']),   # a VARCHAR pair
    ("a < s", ['"a"', '"s"', "VARCHAR"]),
    ("a < u", ['"a"', '"u"', "BIGINT", "UTINYINT", "a signed column against an unsigned column"]),  # mixed signedness
    ("u >= a", ['"u"', '"a"', "a signed column against an unsigned column"]),
    ("a = f", ['"a"', '"f"', "DOUBLE", "an integer-like column against a float"]),
    ("d1 < a", ['"d1"', '"a"', "DATE", "a DATE column against a non-DATE column"]),
    ("d1 < d2 OR a < b", ['"OR"']),
    ("d1 < DATE d2", ["only AND joins filter terms", '"d2"']),            # no string follows: the column "date"
    # NULL is no column: refused by the literal parser as before (pins existing behaviour, passes without the feature)
    ("d1 < NULL", ['"NULL"']),
    ("f = nano", ['"nano"', "not found"]),                                # a word that is neither a column nor a literal
])
def test_column_term_bind_errors_quote_the_text(ext, table, fn, head, tail, text, quoted):
    path, _ = table
    with pytest.raises(ExtError) as e:
        ext.query(fn, path, *head, text, *tail, limit=0)
    msg = str(e.value)
    assert msg.startswith(fn + ": "), msg
    for q in quoted:
        assert q in msg, (q, msg)


@pytest.mark.parametrize("fn,head,tail", FUNCS)
def test_column_terms_bind_without_a_gpu(ext, table, fn, head, tail):
    path, _ = table
    for text in ("d1 < d2", "d1 < d2 AND d0 < d1", "a <> b", "a != B and \"a\" <= \"b\"", "a = a", "d0 >= D1 and id < 7",
                 "d1 < d2 AND k IN (1, 2, 3) AND s LIKE 'MA%' AND id >= 5",
                 # still literals: a typed DATE literal, and a column named like the keyword on either side
                 "d1 < DATE '1995-01-01'", "date < DATE '1995-01-01'", "date < d1", "d1 >= date AND d1 < date '1994-09-01'",
                 # ... and the words the float literal parser reads: no column has these names
                 "f = nan", "f < inf", "f >= infinity", "f <> NaN AND f > -1e308 AND a <> b"):
        names, _, rows = ext.query(fn, path, *head, text, *tail, limit=0)
        assert names and rows == []


# ------------------------------------------------------------------ GPU tests
def masks(cols):
    v = cols["d2_valid"]
    return [
        ("d1 < d2", (cols["d1"] < cols["d2"]) & v),
        ("d1 < d2 AND d0 < d1", (cols["d1"] < cols["d2"]) & v & (cols["d0"] < cols["d1"])),
        ("a <> b", cols["a"] != cols["b"]),
        ("d1 <= d2 AND id >= 70 AND k IN (" + ", ".join(str(i) for i in range(0, 5000, 3)) + ") AND s LIKE '%AI%'",
         (cols["d1"] <= cols["d2"]) & v & (cols["id"] >= 70) & (cols["k"] % 3 == 0) &
         np.isin(cols["s"], ["AIR", "MAIL", "RAIL"])),
        # the right side still a literal where it is a typed literal; the keyword-named column on either side
        ("d1 < DATE '1994-09-01'", cols["d1"] < 9009),
        ("date < DATE '1994-09-01' AND d1 >= date", (cols["date"] < 9009) & (cols["d1"] >= cols["date"])),
        ("a >= b AND b >= a", cols["a"] == cols["b"]),
        # float words stay literals: NaN equals NaN and sits above every number
        ("f = nan", np.isnan(cols["f"])),
        ("f < inf", ~np.isnan(cols["f"]) & (cols["f"] < np.inf)),
        ("f >= infinity", np.isnan(cols["f"]) | (cols["f"] == np.inf)),
        ("f <> NaN AND f > -1e308 AND a <> b", ~np.isnan(cols["f"]) & (cols["f"] > -1e308) & (cols["a"] != cols["b"])),
        ("d2 = d2", v),                                                       # a NULL satisfies no operator
        ("d2 <> d2", np.zeros(N, bool)),
    ]


@pytest.mark.gpu
def test_gpu_filter_text_column_terms(fl, gpu, ext, table):
    path, cols = table
    assert (np.datetime64("1970-01-01") + 9009) == np.datetime64("1994-09-01")
    for text, m in masks(cols):
        assert m.any() or text == "d2 <> d2", text
        _, _, rows = ext.query("fastlanes_aggregate", path, "count(*), sum(k)", text)
        assert rows == [[str(int(m.sum())), str(int(cols["k"][m].sum())) if m.any() else None]], text
        # the 30 largest k (ties by row) under the same filter
        _, _, rows = ext.query("fastlanes_topn", path, "k DESC", 30, text, "id, k")
        cand = np.nonzero(m)[0]
        order = cand[np.lexsort((cand, -cols["k"][cand]))][:30]
        assert rows == [[str(i), str(cols["k"][i])] for i in order], text
