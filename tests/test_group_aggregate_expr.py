"""SUM of a product of affine column terms per group (FLS_AGG_SUM_EXPR through
fls_aggregate_grouped / Table.aggregate_grouped; csrc/fls_groupagg.hip).

Expected values are Python integers over each group's rows, from the seeded
generators' gen_values or the arrays handed to write_image; every comparison
is exact."""
import datetime

import numpy as np
import pytest

from helpers import filter_mask
from test_aggregate_expr import CHARGE, DISC_PRICE, expect_expr
from test_group_aggregate import groups_of, lineitem_groups

C_QTY, C_PRICE, C_DISC, C_TAX, C_RFLAG, C_STATUS, C_SHIPDATE = 4, 5, 6, 7, 8, 9, 10
Q1_DAY = (datetime.date(1998, 9, 2) - datetime.date(1970, 1, 1)).days
Q1_TERMS = [(C_SHIPDATE, "<=", Q1_DAY)]
Q1_AGGS = [("sum", C_QTY), ("sum", C_PRICE), ("sum_expr", DISC_PRICE), ("sum_expr", CHARGE), ("sum", C_DISC),
           ("count",)]


@pytest.fixture(scope="module")
def conn0(fl):
    conn = fl.Connection([0])
    yield conn
    conn.close()


@pytest.mark.gpu
def test_gpu_lineitem_q1_grouped(fl, gpu, conn0):
    wl, sf = "lineitem", 0.01
    t = conn0.read_image(fl.gen_image(wl, sf))
    n = t.nrows
    cols, words = {}, {}
    for c in (C_QTY, C_PRICE, C_DISC, C_TAX, C_RFLAG, C_STATUS, C_SHIPDATE):
        ty = t.schema()[c][1]
        if ty == fl.VARCHAR:
            cols[c] = fl.gen_values(wl, c, 0, n, np.uint32, sf)     # dictionary codes of the generator
            words[c] = []
            while (s := fl.gen_dict_string(wl, c, len(words[c]))) is not None:
                words[c].append(s.encode())
        else:
            cols[c] = fl.gen_values(wl, c, 0, n, fl.NP_DTYPE[ty], sf)
    sel = filter_mask(cols, Q1_TERMS, n)
    want = lineitem_groups(cols, words, [C_RFLAG, C_STATUS], sel)
    got = t.aggregate_grouped([C_RFLAG, C_STATUS], Q1_AGGS, filt=Q1_TERMS)
    assert [k for k, _ in got] == [k for k, _ in want] and len(got) > 1
    for (key, vals), (_, rows) in zip(got, want):
        qty, price, disc, tax = (cols[c][rows].astype(object) for c in (C_QTY, C_PRICE, C_DISC, C_TAX))
        assert vals == [int(qty.sum()), int(price.sum()), int((price * (100 - disc)).sum()),
                        int((price * (100 - disc) * (100 + tax)).sum()), int(disc.sum()), len(rows)], key
    # the groups add up to the ungrouped call
    plain = t.aggregate(Q1_AGGS, filt=Q1_TERMS)
    assert [sum(vals[i] for _, vals in got) for i in range(len(Q1_AGGS))] == plain
    t.close()


RG = 1024
N = 2 * RG + 37


@pytest.fixture(scope="module")
def keyed(fl, conn0):
    """a constant key, a key with 64 distinct values in every vector, and
    three factor columns with NULLs"""
    rng = np.random.default_rng(4711)
    n = N
    a = rng.integers(-2**38, 2**38, n).astype(np.int64)
    b = rng.integers(-2**31, 2**31, n).astype(np.int32)
    u = rng.integers(0, 2**16, n).astype(np.uint16)
    va, vb, vu = rng.random(n) >= 0.3, rng.random(n) >= 0.25, rng.random(n) >= 0.1
    va[RG:RG + 64] = False      # the first row of every key in vector 1 is NULL in a
    k64 = (np.arange(n) % 64).astype(np.int16)
    vb[k64 == 5] = False        # a group no row of which is valid in b
    one = np.zeros(n, dtype=np.int8)
    img = fl.write_image([("one", fl.INT8, one, fl.ENC_AUTO), ("k64", fl.INT16, k64, fl.ENC_AUTO),
                          ("a", fl.INT64, np.ma.array(a, mask=~va), fl.ENC_AUTO),
                          ("b", fl.INT32, np.ma.array(b, mask=~vb), fl.ENC_AUTO),
                          ("u", fl.UINT16, np.ma.array(u, mask=~vu), fl.ENC_AUTO)], rowgroup=RG)
    t = conn0.read_image(img)
    every = np.ones(n, bool)
    yield t, {0: one, 1: k64, 2: a, 3: b, 4: u}, {0: every, 1: every, 2: va, 3: vb, 4: vu}
    t.close()


KEYED_EXPRS = [[(2**38, -1, 2)], [(0, 1, 2), (1, -1, 3)], [(0, 1, 2), (0, 1, 2)], [(-3, 1, 4), (0, -1, 3), (2**20, 1, 2)],
               [(100, -1, 4), (100, 1, 4), (7, -1, 4)]]


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [None, [(3, "<", 0)]], ids=["all", "b_negative"])
def test_gpu_one_group_equals_the_ungrouped_call(fl, gpu, keyed, filt):
    t, cols, valid = keyed
    aggs = [("count",)] + [("sum_expr", e) for e in KEYED_EXPRS] + [("sum_product", 2, 3), ("sum", 2)]
    got = t.aggregate_grouped([0], aggs, filt=filt)
    plain = t.aggregate(aggs, filt=filt)
    assert got == [((0,), plain)]
    sel = np.ones(N, bool) if filt is None else valid[3] & filter_mask(cols, filt, N)
    assert plain[1:1 + len(KEYED_EXPRS)] == [expect_expr(cols, e, sel, valid)[0] for e in KEYED_EXPRS]


@pytest.mark.gpu
def test_gpu_64_keys_in_a_vector_with_nulls_in_a_factor_column(fl, gpu, keyed):
    t, cols, valid = keyed
    aggs = [("sum_expr", e) for e in KEYED_EXPRS]
    got = t.aggregate_grouped([1], aggs)
    want = groups_of([cols[1]], [None], np.ones(N, bool))
    assert [k for k, _ in got] == [k for k, _ in want] == [(k,) for k in range(64)]
    for (key, vals), (_, m) in zip(got, want):
        assert vals == [expect_expr(cols, e, m, valid)[0] for e in KEYED_EXPRS], key
    # key 5 has no row valid in b: NULL where b is a factor, a value elsewhere
    assert got[5][1][1] is None and got[5][1][3] is None and got[5][1][0] is not None
