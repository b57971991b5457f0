"""The SQL face of the filter's alternatives, through
the extension harness: the filter text of fastlanes_aggregate / fastlanes_topn
learns one parenthesised OR group among its AND-ed items,

    filter := item (AND item)*
    item   := term | '(' branch (OR branch)+ ')'
    branch := term | '(' term (AND term)* ')'

CPU tests bind only (limit=0: the BinderException texts come from the footer).
GPU tests compare the SQL functions with numpy under TPC-H Q19's shape."""
import numpy as np
import pytest

from ext_harness import Ext, ExtError

RG = 1024
N = 2 * 1024 + 333
TAIL = 2 * 1024
MODES = ["AIR", "AIR REG", "MAIL", "SHIP"]
INSTRUCT = ["DELIVER IN PERSON", "COLLECT COD", "NONE"]


@pytest.fixture(scope="module")
def ext(_built):
    e = Ext()
    yield e
    e.close()


def make_columns():
    """lineitem's Q19 columns in small: id (row number), partkey BIGINT in
    [0, 60), qty INTEGER in [1, 35], price BIGINT, mode and instruct VARCHAR,
    n a nullable BIGINT"""
    rng = np.random.default_rng(19)
    ids = np.arange(N, dtype=np.int32)
    partkey = rng.integers(0, 60, N).astype(np.int64)
    qty = rng.integers(1, 36, N).astype(np.int32)
    price = rng.integers(100, 100000, N).astype(np.int64)
    mode = [MODES[i] for i in rng.integers(0, len(MODES), N)]
    instruct = [INSTRUCT[i] for i in rng.integers(0, len(INSTRUCT), N)]
    null = rng.random(N) < 0.3
    nv = rng.integers(0, 10, N).astype(np.int64)
    return {"id": ids, "partkey": partkey, "qty": qty, "price": price, "mode": np.array(mode),
            "instruct": np.array(instruct), "n": nv, "n_valid": ~null}


COLS = make_columns()   # computed once, shared and never changed


@pytest.fixture(scope="module")
def table(fl, tmp_path_factory):
    c = COLS
    path = str(tmp_path_factory.mktemp("altsql") / "t.fls")
    A = fl.ENC_AUTO
    fl.write_image([("id", fl.INT32, c["id"], A), ("partkey", fl.INT64, c["partkey"], A), ("qty", fl.INT32, c["qty"], A),
                    ("price", fl.INT64, c["price"], A), ("mode", fl.VARCHAR, list(c["mode"]), fl.ENC_DICT),
                    ("instruct", fl.VARCHAR, list(c["instruct"]), fl.ENC_DICT),
                    ("n", fl.INT64, np.ma.masked_array(c["n"], mask=~c["n_valid"]), A)],
                   rowgroup=RG, path=path)
    return path, c


FUNCS = [("fastlanes_aggregate", ("count(*)",), ()), ("fastlanes_topn", ("id", 5), ())]
NINE = " OR ".join(f"qty = {i}" for i in range(1, 10))


# ------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("fn,head,tail", FUNCS)
@pytest.mark.parametrize("text,quoted", [
    ("qty < 5 OR qty > 30", ["only AND joins filter terms", '"OR"']),                # an OR outside parentheses
    ("id < 9 AND qty < 5 OR qty > 30", ['"OR"']),
    ("(qty < 5 OR qty > 30) AND (id < 9 OR id > 99)", ["a second OR group", '"(id < 9 OR id > 99)"', "one per filter"]),
    (f"id > 3 AND ({NINE})", ["more than 8 branches", f'"id > 3 AND ({NINE})"']),
    ("(qty < 5 OR ((id < 9) AND qty > 30))", ["a parenthesis nested deeper than a branch", '"(id < 9) AND qty > 30))"']),
    ("((qty < 5 OR qty > 30))", ['"(qty < 5 OR"', 'found "OR"']),                    # a branch holds no OR of its own
    ("(qty < 5 AND id < 9 OR qty > 30)", ['"qty < 5 AND"', '"AND"', "takes its own parentheses"]),
    ("(qty < 5)", ['"("', '"(qty < 5)"', "holds no OR"]),
    ("(qty < 5 OR qty > 30", ['"qty > 30"', '"end of text"']),
    ("(qty < 5 OR (qty > 30 AND id < 9)", ['"end of text"']),
    ("(qty < 5 OR nosuch > 30)", ['"nosuch"', "not found"]),                          # a term's own refusal, inside a branch
    ("(qty < 5 OR (mode LIKE 3))", ["a quoted pattern is expected after LIKE", '"3"']),
])
def test_or_group_bind_errors_quote_the_text(ext, table, fn, head, tail, text, quoted):
    path, _ = table
    with pytest.raises(ExtError) as e:
        ext.query(fn, path, *head, text, *tail, limit=0)
    msg = str(e.value)
    assert msg.startswith(fn + ": "), msg
    for q in quoted:
        assert q in msg, (q, msg)


def test_no_or_group_in_a_condition(ext, table):
    path, _ = table
    with pytest.raises(ExtError) as e:
        ext.query("fastlanes_aggregate", path, "count(*) FILTER (WHERE (qty < 5 OR qty > 30))", "", limit=0)
    msg = str(e.value)
    assert msg.startswith("fastlanes_aggregate: ") and "an OR group is not supported in a FILTER (WHERE ...) condition" in msg
    assert '"(qty < 5 OR qty > 30)"' in msg
    # ... while the call's filter takes one beside a conditioned aggregate
    names, _, rows = ext.query("fastlanes_aggregate", path, "count(*) FILTER (WHERE qty < 5)", "(id < 9 OR id > 99)", limit=0)
    assert names and rows == []


Q19 = ("instruct = 'DELIVER IN PERSON' AND mode IN ('AIR', 'AIR REG') AND "
       "((partkey IN (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20) AND qty >= 1 AND qty <= 15) "
       "OR (partkey IN (10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29) AND qty >= 10 "
       "AND qty <= 25) "
       "OR (partkey IN (30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45) AND qty >= 20 AND qty <= 30))")


@pytest.mark.parametrize("fn,head,tail", FUNCS)
def test_or_groups_bind_without_a_gpu(ext, table, fn, head, tail):
    path, _ = table
    for text in (Q19, "(qty < 5 OR qty > 30)", "(qty < 5 OR qty > 30 OR id = 7)", "id > 3 AND (qty < 5 OR qty > 30) AND id < 2000",
                 "(qty < 5 OR (qty > 30 AND id < 9))", "((qty < 5) OR (qty > 30))",
                 "(qty < 5 or (qty > 30 And id < 9)) aNd mode like 'AIR%'",
                 "(partkey IN (1, 2) OR mode NOT LIKE 'A%' OR n IS NULL OR id < qty)",
                 "(" + " OR ".join(f"qty = {i}" for i in range(1, 9)) + ")"):
        names, _, rows = ext.query(fn, path, *head, text, *tail, limit=0)
        assert names and rows == []


# ------------------------------------------------------------------ GPU tests
def q19_masks(c):
    base = (c["instruct"] == "DELIVER IN PERSON") & np.isin(c["mode"], ["AIR", "AIR REG"])
    alts = [np.isin(c["partkey"], range(1, 21)) & (c["qty"] >= 1) & (c["qty"] <= 15),
            np.isin(c["partkey"], range(10, 30)) & (c["qty"] >= 10) & (c["qty"] <= 25),
            np.isin(c["partkey"], range(30, 46)) & (c["qty"] >= 20) & (c["qty"] <= 30)]
    return base, alts


def group_cases(c):
    """(filter text, the AND-ed items' mask, the branches' masks)"""
    v = c["n_valid"]
    return [
        ("(qty < 8 OR qty > 25 OR partkey < 6 OR id > 2300)", np.ones(N, bool),
         [c["qty"] < 8, c["qty"] > 25, c["partkey"] < 6, c["id"] > 2300]),
        ("((qty < 8) or (qty > 25 and n >= 5) Or partkey < 6 oR (Id > 2300)) and mode <> 'MAIL'", c["mode"] != "MAIL",
         [c["qty"] < 8, (c["qty"] > 25) & (c["n"] >= 5) & v, c["partkey"] < 6, c["id"] > 2300]),
        ("id >= 100 AND (mode LIKE 'AIR%' OR (partkey IN (1, 2, 3, 4, 5, 6, 7, 8) AND qty < 20) OR (qty < n AND id >= 1000)"
         " OR n IS NULL)", c["id"] >= 100,
         [np.char.startswith(c["mode"], "AIR"), np.isin(c["partkey"], range(1, 9)) & (c["qty"] < 20),
          (c["qty"] < c["n"]) & v & (c["id"] >= 1000), ~v]),
    ]


def facts(base, alts, tail=True):
    """the union selects some but not all of the base filter's rows, every
    branch a row of its own, two of them overlap; in the table and in the
    partial tail vector"""
    for sl in (slice(None), slice(TAIL, None))[:2 if tail else 1]:
        within = [a[sl] & base[sl] for a in alts]
        union = np.any(within, axis=0)
        assert 0 < union.sum() < base[sl].sum(), (union.sum(), base[sl].sum())
        for i, a in enumerate(within):
            others = np.any([o for j, o in enumerate(within) if j != i], axis=0)
            assert (a & ~others).any(), i
        assert any((within[i] & within[j]).any() for i in range(len(within)) for j in range(i))


def test_reference_facts_hold():
    """what the GPU tests assert before they compare, checked without a GPU too"""
    base, alts = q19_masks(COLS)
    facts(base, alts, tail=False)   # Q19's selectivity leaves the 333-row tail too few such rows: the group cases cover it
    for _text, b, a in group_cases(COLS):
        facts(b, a)


def check_sql(ext, path, cols, text, m):
    _, _, rows = ext.query("fastlanes_aggregate", path, "count(*), sum(price)", text)
    assert rows == [[str(int(m.sum())), str(int(cols["price"][m].sum()))]], text
    _, _, rows = ext.query("fastlanes_topn", path, "price DESC", 30, text, "id, price")
    cand = np.nonzero(m)[0]
    order = cand[np.lexsort((cand, -cols["price"][cand]))][:30]
    assert rows == [[str(i), str(cols["price"][i])] for i in order], text


@pytest.mark.gpu
def test_gpu_q19_shape(fl, gpu, ext, table):
    path, cols = table
    base, alts = q19_masks(cols)
    facts(base, alts, tail=False)
    m = base & np.any(alts, axis=0)
    check_sql(ext, path, cols, Q19, m)
    # grouped under the same filter
    _, _, rows = ext.query("fastlanes_aggregate", path, "count(*)", Q19, "qty")
    want = {int(k): int((m & (cols["qty"] == k)).sum()) for k in np.unique(cols["qty"][m])}
    assert len(want) > 3 and sorted(rows) == sorted([str(k), str(v)] for k, v in want.items())


@pytest.mark.gpu
def test_gpu_branches_with_and_without_parentheses_in_any_case(fl, gpu, ext, table):
    path, cols = table
    for text, base, alts in group_cases(cols):
        facts(base, alts)
        check_sql(ext, path, cols, text, base & np.any(alts, axis=0))
