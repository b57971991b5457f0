"""The SQL face of the filtered aggregates, through the
extension harness: an item of fastlanes_aggregate's list may end in
`FILTER (WHERE <filter text>)`, the text in the grammar of the third argument.

CPU tests bind only (limit=0: names, types and the BinderException texts come
from the footer).  The GPU test compares one Q14-shaped row with
Table.aggregate under the same conditions."""
import numpy as np
import pytest

from ext_harness import Ext, ExtError

RG = 1024
N = 2 * 1024 + 37
TYPES = ["PROMO BRUSHED TIN", "PROMO PLATED STEEL", "STANDARD POLISHED BRASS", "ECONOMY ANODIZED NICKEL"]
C_ID, C_PRICE, C_DISC, C_PART, C_TYPE, C_SHIP, C_COMMIT = range(7)


@pytest.fixture(scope="module")
def ext(_built):
    e = Ext()
    yield e
    e.close()


@pytest.fixture(scope="module")
def table(fl, tmp_path_factory):
    rng = np.random.default_rng(14)
    cols = {"id": np.arange(N, dtype=np.int32), "price": rng.integers(100, 10 ** 6, N).astype(np.int64),
            "disc": rng.integers(0, 11, N).astype(np.int64), "part": rng.integers(1, 200, N).astype(np.int64),
            "ptype": [TYPES[i] for i in rng.integers(0, len(TYPES), N)],
            "ship": rng.integers(9000, 9060, N).astype(np.int32), "commit": rng.integers(9000, 9060, N).astype(np.int32)}
    path = str(tmp_path_factory.mktemp("aggfilter") / "t.fls")
    A = fl.ENC_AUTO
    fl.write_image([("id", fl.INT32, cols["id"], A), ("price", fl.DECIMAL, cols["price"], A, 15, 2),
                    ("disc", fl.DECIMAL, cols["disc"], A, 15, 2), ("part", fl.INT64, cols["part"], A),
                    ("ptype", fl.VARCHAR, cols["ptype"], fl.ENC_DICT), ("ship", fl.DATE, cols["ship"], A),
                    ("commit", fl.DATE, cols["commit"], A)], rowgroup=RG, path=path)
    return path, cols


REV = "sum(price * (1 - disc))"
PROMO = ", ".join(str(i) for i in range(1, 200, 3))


# ------------------------------------------------------------------ CPU tests
def test_names_and_types_are_the_items_own(ext, table):
    path, _ = table
    items = [REV + " FILTER (WHERE part IN (" + PROMO + "))", REV, "count(*) filter (where ptype like 'PROMO%')",
             "count(*)", "min(ship)  Filter ( Where ship < commit AND disc >= 0.05 )", "min(ship)",
             "sum(price) FILTER (WHERE ptype = 'a, b) FILTER (' AND id < 7)", "count(id) FILTER(WHERE id IS NOT NULL)"]
    for extra in ((), ("ship >= DATE '1994-09-01'",), ("", "part")):
        names, types, rows = ext.query("fastlanes_aggregate", path, ", ".join(items), *extra, limit=0)
        k = 1 if len(extra) == 2 else 0
        assert names[k:] == items and rows == []
        assert types[k:][0] == types[k:][1] and types[k:][2] == types[k:][3] and types[k:][4] == types[k:][5]
        assert types[k:][0].startswith("DECIMAL(18,4") and types[k:][2] == "BIGINT" and types[k:][4] == "DATE"


@pytest.mark.parametrize("item,quoted", [
    ("count(*) FILTER (WHERE nosuch = 1)", ['"nosuch"', "not found", '"nosuch = 1"']),
    ("count(*) FILTER (WHERE id < 5 OR id > 9)", ['"OR"', '"id < 5 OR id > 9"']),
    ("count(*) FILTER (WHERE ship < part)", ['"ship"', '"part"', "a DATE column against a non-DATE column"]),
    ("count(*) FILTER (WHERE part LIKE 'a%')", ['"part"']),
    ("count(*) FILTER (WHERE )", ["FILTER (WHERE ...) is expected", '"FILTER (WHERE )"']),
    ("count(*) FILTER (id < 5)", ["FILTER (WHERE ...) is expected", '"FILTER (id < 5)"']),
    ("count(*) FILTER WHERE id < 5", ["FILTER (WHERE ...) is expected", '"FILTER WHERE id < 5"']),
    ("count(*) WHERE id < 5", ["FILTER (WHERE ...) is expected", '"WHERE id < 5"']),
    ("count(*) FILTER (WHEREid < 5)", ["FILTER (WHERE ...) is expected"]),
    ("count(*) FILTER (WHERE (id < 5))", ['"(id < 5)"']),
    ("sum(nosuch) FILTER (WHERE id < 5)", ['"nosuch"', "not found", '"sum(nosuch)"']),
])
def test_bind_errors_quote_the_text(ext, table, item, quoted):
    path, _ = table
    with pytest.raises(ExtError) as e:
        ext.query("fastlanes_aggregate", path, "count(*), " + item, limit=0)
    msg = str(e.value)
    assert msg.startswith("fastlanes_aggregate: "), msg
    for q in quoted:
        assert q in msg, (q, msg)


def test_identical_text_shares_a_condition_and_the_ninth_is_refused(ext, table):
    path, _ = table
    eight = [f"count(*) FILTER (WHERE id < {i})" for i in range(8)]
    names, _, _ = ext.query("fastlanes_aggregate", path, ", ".join(eight + ["sum(price) FILTER (WHERE id < 3)"] * 3), limit=0)
    assert len(names) == 11
    with pytest.raises(ExtError) as e:
        ext.query("fastlanes_aggregate", path, ", ".join(eight + ["count(*) FILTER (WHERE id < 8)"]), limit=0)
    assert "at most 8 different FILTER conditions" in str(e.value) and '"id < 8"' in str(e.value)


# ------------------------------------------------------------------ GPU test
@pytest.mark.gpu
def test_gpu_q14_shaped_row_matches_table_aggregate(fl, gpu, ext, table):
    path, cols = table
    promo = list(range(1, 200, 3))
    items = [REV + " FILTER (WHERE part IN (" + PROMO + "))", REV, "count(*) FILTER (WHERE ptype LIKE 'PROMO%')",
             "count(*) FILTER (WHERE ship < commit)", "count(*)"]
    where = "ship >= DATE '1994-09-10' AND ship < DATE '1994-10-10'"
    _, _, rows = ext.query("fastlanes_aggregate", path, ", ".join(items), where)
    conn = fl.Connection([0])
    t = conn.read_fls(path)
    ks = conn.keyset(np.array(promo, np.int64))
    rev = ("sum_expr", [(0, 1, C_PRICE), (100, -1, C_DISC)])
    got = t.aggregate([fl.When(rev, [(C_PART, "in_set", ks)]), rev, fl.When(("count",), [(C_TYPE, "like", "PROMO%")]),
                       fl.When(("count",), [(C_SHIP, "<", fl.Col(C_COMMIT))]), ("count",)],
                      [(C_SHIP, ">=", 9018), (C_SHIP, "<", 9048)])
    assert (np.datetime64("1970-01-01") + 9018) == np.datetime64("1994-09-10")
    m = (cols["ship"] >= 9018) & (cols["ship"] < 9048)
    in_set = np.isin(cols["part"], promo)
    revs = cols["price"] * (100 - cols["disc"])
    assert got == [int(revs[m & in_set].sum()), int(revs[m].sum()),
                   int((m & np.array([s.startswith("PROMO") for s in cols["ptype"]])).sum()),
                   int((m & (cols["ship"] < cols["commit"])).sum()), int(m.sum())]
    assert 0 < got[0] < got[1] and 0 < got[2] < got[4] and 0 < got[3] < got[4]
    dec = lambda x: f"{x // 10000}.{x % 10000:04d}"  # noqa: E731
    assert rows == [[dec(got[0]), dec(got[1]), str(got[2]), str(got[3]), str(got[4])]]
    ks.close()
    t.close()
    conn.close()
