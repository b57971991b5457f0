"""The SQL face of the pattern filter terms, through the extension harness: the
filter text of fastlanes_aggregate / fastlanes_topn learns
`column [NOT] LIKE 'pattern' [ESCAPE 'c']`.

CPU tests bind only (limit=0: the BinderException texts come from the footer).
GPU tests compare the SQL functions with the Python API's results under the
same term, and both with the reference matcher (like_ref.py)."""
import numpy as np
import pytest

from ext_harness import Ext, ExtError
from like_ref import POOL, like_mask

RG = 1024
N = 2 * 1024 + 37
C_ID, C_K, C_S, C_F, C_B = range(5)


@pytest.fixture(scope="module")
def ext(_built):
    e = Ext()
    yield e
    e.close()


@pytest.fixture(scope="module")
def table(fl, tmp_path_factory):
    """id (row number), k BIGINT, s VARCHAR (DICT) and f VARCHAR (FSST) over the LIKE pool, b BLOB"""
    rng = np.random.default_rng(9)
    ids = np.arange(N, dtype=np.int32)
    k = rng.integers(0, 5000, N).astype(np.int64)
    s = [POOL[i] for i in rng.integers(0, len(POOL), N)]
    path = str(tmp_path_factory.mktemp("likesql") / "t.fls")
    fl.write_image([("id", fl.INT32, ids, fl.ENC_AUTO), ("k", fl.INT64, k, fl.ENC_AUTO),
                    ("s", fl.VARCHAR, s, fl.ENC_DICT), ("f", fl.VARCHAR, s, fl.ENC_FSST),
                    ("b", fl.BLOB, s, fl.ENC_FSST)], rowgroup=RG, path=path)
    return path, {C_ID: ids, C_K: k, C_S: s, C_F: s}


FUNCS = [("fastlanes_aggregate", ("count(*)",), ()), ("fastlanes_topn", ("id", 5), ())]


@pytest.mark.parametrize("fn,head,tail", FUNCS)
@pytest.mark.parametrize("text,quoted", [
    ("s LIKE 'a%' ESCAPE 'ab'", ["ESCAPE", "\"'ab'\"", "\"s LIKE 'a%' ESCAPE 'ab'\""]),       # not one byte
    ("s LIKE 'a%' ESCAPE ''", ["ESCAPE", "\"''\""]),
    ("s LIKE 'a%' ESCAPE 5", ["ESCAPE", '"5"']),
    ("s NOT LIKE 'a%' ESCAPE", ["ESCAPE", "\"s NOT LIKE 'a%' ESCAPE\""]),
    ("k LIKE '1%'", ["LIKE needs a VARCHAR column", '"k"', "BIGINT", "\"k LIKE '1%'\""]),     # a non-string column
    ("id NOT LIKE '1%'", ["NOT LIKE needs a VARCHAR column", '"id"']),
    ("b LIKE 'a%'", ["LIKE needs a VARCHAR column", '"b"', "BLOB"]),
    ("s LIKE 'ab\\' ESCAPE '\\'", ["\"'ab\\'\"", "ends in its escape byte", "\"s LIKE 'ab\\' ESCAPE '\\'\""]),
    ("s LIKE 'ab!!!' ESCAPE '!'", ["\"'ab!!!'\"", "ends in its escape byte"]),
    ("s LIKE 5", ["a quoted pattern is expected after LIKE", '"5"', '"s LIKE 5"']),
    ("s NOT LIKE", ["a quoted pattern is expected after NOT LIKE", '"s NOT LIKE"']),
    ("s LIKE 'a%' OR id < 5", ['"OR"']),
    ("s NOT 'a%'", ["NOT IN or NOT LIKE", "\"s NOT 'a%'\""]),
])
def test_like_bind_errors_quote_the_text(ext, table, fn, head, tail, text, quoted):
    path, _ = table
    with pytest.raises(ExtError) as e:
        ext.query(fn, path, *head, text, *tail, limit=0)
    msg = str(e.value)
    assert msg.startswith(fn + ": "), msg
    for q in quoted:
        assert q in msg, (q, msg)


@pytest.mark.parametrize("fn,head,tail", FUNCS)
def test_like_binds_without_a_gpu(ext, table, fn, head, tail):
    path, _ = table
    for text in ("s LIKE 'abcd%'", "s like '%' and f NOT LIKE '%it''s%' AND id < 7",
                 "s LIKE '100\\%' ESCAPE '\\' AND f not like 'a!_b' escape '!' AND k IN (1, 2)",
                 '"s" NOT LIKE \'\'', "s LIKE NULL", "f NOT LIKE NULL AND id >= 3", "s LIKE 'ab!!' ESCAPE '!'"):
        names, _, rows = ext.query(fn, path, *head, text, *tail, limit=0)
        assert names and rows == []


# ------------------------------------------------------------------ GPU tests
SQL_PATTERNS = [("abcd%", None), ("%abc%", None), ("%ab%abc", None), ("caf_", None), ("100\\%", "\\"), ("a\\_b", "\\"),
                ("a!_b", "!"), ("%a%a%a%a%b", None), ("", None), ("_", None), ("it's", None)]


def sql_term(col, negate, pat, esc):
    text = f"{col} {'NOT LIKE' if negate else 'LIKE'} '{pat.replace(chr(39), chr(39) * 2)}'"
    return text + (f" ESCAPE '{esc}'" if esc else "")


@pytest.mark.gpu
@pytest.mark.parametrize("col,c", [("s", C_S), ("f", C_F)])
def test_gpu_filter_text_like(fl, gpu, ext, table, col, c):
    path, cols = table
    t = fl.Connection([0]).read_fls(path)
    kinds = set()
    for pat, esc in SQL_PATTERNS:
        for negate in (False, True):
            term = (c, "not_like" if negate else "like", pat if esc is None else (pat, esc))
            m = like_mask(cols, [term], N)
            kinds.add("none" if not m.any() else "all" if m.all() else "part")
            text = sql_term(col, negate, pat, esc)
            # fastlanes_aggregate under the pattern and an ordinary term
            m2 = m & (cols[C_ID] >= 70)
            _, _, rows = ext.query("fastlanes_aggregate", path, "count(*), sum(k)", text + " AND id >= 70")
            assert rows == [[str(int(m2.sum())), str(int(cols[C_K][m2].sum())) if m2.any() else None]], text
            # fastlanes_topn: the 30 largest k (ties by row) under the pattern alone
            _, _, rows = ext.query("fastlanes_topn", path, "k DESC", 30, text, "id, k")
            cand = np.nonzero(m)[0]
            order = cand[np.lexsort((cand, -cols[C_K][cand]))][:30]
            assert rows == [[str(i), str(cols[C_K][i])] for i in order], text
            # ... and the Python API's results under the same term
            assert t.aggregate([("count",)], filt=[term, (C_ID, ">=", 70)])[0] == int(m2.sum()), text
            assert np.array_equal(t.topn(C_K, 30, cols=[C_ID], filt=[term], desc=True)[0], order.astype(np.uint64)), text
    assert kinds == {"none", "all", "part"}
    _, _, rows = ext.query("fastlanes_aggregate", path, "count(*)", f"{col} LIKE NULL")
    assert rows == [["0"]]
