"""Grouped aggregate pushdown: GROUP BY on low-cardinality keys reduced on the
GPU (fls_aggregate_grouped / Table.aggregate_grouped; csrc/fls_groupagg.hip).

Expected values come from the inputs themselves -- the arrays handed to
write_image, or the seeded generators -- grouped in Python in order of each
key's first selected row, under helpers.filter_mask for the selection and the
arrays' own validity, and reduced with exact integers as tests/test_aggregate.py
does.  Keys, group order, integer results, counts, MIN / MAX and NULL-ness
compare exactly; a per-group binary64 sum against math.fsum within
(n - 1) * 2^-53 * sum |x_i| (test_aggregate.check_float_sum, on finite inputs).

CPU tests: the exported symbols, every argument error, the all-pruned call, the
kernels' resources.  GPU tests: every key type and encoding, dictionaries that
differ per row group, 2-byte codes, several keys with NULLs, rows that must not
make a group, the two capacities, one group against the ungrouped call bit for
bit, reproducibility across batch sizes and pipelines, lineitem Q1."""
import ctypes as C
import datetime
import math
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import filter_mask, rand64
from test_aggregate import check_float_sum, expect_float_minmax, expect_int, null_aware_mask, same_float

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "duckdb-fastlane_amd" / "libflsgpu.so"

ERR_ARG, ERR_DEVICE, ERR_LIMIT = -3, -4, -8
C_OKEY, C_PART, C_LINE, C_QTY, C_PRICE, C_DISC = 0, 1, 3, 4, 5, 6
C_RFLAG, C_STATUS, C_SHIPDATE, C_INSTRUCT, C_MODE, C_COMMENT = 8, 9, 10, 13, 14, 15
DAY_1994, DAY_1995 = 8766, 9131
Q1_DAY = (datetime.date(1998, 9, 2) - datetime.date(1970, 1, 1)).days
Q6 = [(C_SHIPDATE, ">=", DAY_1994), (C_SHIPDATE, "<", DAY_1995), (C_DISC, ">=", 5), (C_DISC, "<=", 7),
      (C_QTY, "<", 2400)]


# ------------------------------------------------------------ expected values
def py_key(x):
    return x if x is None or isinstance(x, bytes) else int(x)


def groups_of(keycols, keyvalid, sel):
    """[(key tuple, row mask)] in order of each key's first selected row; a
    NULL key element is None whatever the array holds there"""
    rows = {}
    for i in np.nonzero(sel)[0]:
        k = tuple(None if (v is not None and not v[i]) else py_key(c[i]) for c, v in zip(keycols, keyvalid))
        rows.setdefault(k, []).append(i)
    out = []
    for k, r in rows.items():
        m = np.zeros(len(sel), bool)
        m[r] = True
        out.append((k, m))
    return out


def check_groups(got, keys, aggs, cols, valid, sel, what=""):
    """got = aggregate_grouped's result against the grouping of the inputs;
    valid[c]: the column's validity (absent: no NULL)"""
    want = groups_of([cols[c] for c in keys], [valid.get(c) for c in keys], sel)
    assert [g[0] for g in got] == [w[0] for w in want], (what, [g[0] for g in got][:8], [w[0] for w in want][:8])
    every = np.ones(len(sel), bool)
    for (key, vals), (_, m) in zip(got, want):
        assert len(vals) == len(aggs)
        for a, g in zip(aggs, vals):
            tag = (what, key, a)
            if len(a) == 1:
                assert g == int(m.sum()), tag
                continue
            mm = m & valid.get(a[1], every)
            if a[0] == "sum_product":
                mm = mm & valid.get(a[2], every)
                assert g == expect_int("sum_product", cols[a[1]], mm, cols[a[2]]), tag
            elif a[0] == "count":
                assert g == int(mm.sum()), tag
            elif cols[a[1]].dtype.kind == "f":
                if a[0] == "sum":
                    check_float_sum(g, cols[a[1]], mm, f"{what} {key} {a}")
                else:
                    assert same_float(g, expect_float_minmax(a[0], cols[a[1]], mm)), tag
            else:
                assert g == expect_int(a[0], cols[a[1]], mm), tag + (g,)


def bits(x):
    return None if x is None else (int(np.array([x], dtype=np.float64).view(np.uint64)[0]) if isinstance(x, float) else x)


def as_bits(res):
    return [(k, [bits(v) for v in vals]) for k, vals in res]


# ------------------------------------------------------------------ CPU tests
def test_library_exports_the_grouped_call(_built):
    lib = C.CDLL(str(LIB))
    for name in ("fls_aggregate_grouped", "fls_group_result_ngroups", "fls_group_result_key",
                 "fls_group_result_values", "fls_group_result_free"):
        assert hasattr(lib, name), name


@pytest.fixture(scope="module")
def small_full(fl):
    t = fl.Connection([0]).read_image(fl.gen_image("lineitem_full", 0.01))
    yield t
    t.close()


@pytest.mark.parametrize("keys,filt,what,word", [
    ([], None, None, None),                                            # nkeys == 0
    ([C_RFLAG, C_STATUS, C_MODE, C_LINE, C_INSTRUCT], None, None, None),  # nkeys > 4
    ([C_RFLAG, 99], None, "key 1", "out of range"),
    ([99], None, "key 0", "out of range"),
    ([C_RFLAG, C_LINE, C_RFLAG], None, "key 2", None),                  # listed twice
    ([C_STATUS, C_COMMENT], None, "key 1", "dictionary"),               # FSST l_comment: not DICT
    ([C_LINE, C_MODE], [(C_MODE, "=", "AIR")], "key 1", "filter"),      # a VARCHAR key the filter reads
    ([C_OKEY, C_QTY], None, "key 1", "128"),                            # 64 + 64 + 2 bits
    ([C_LINE, C_OKEY, C_PRICE], None, "key 2", "128"),
])
def test_key_argument_errors(fl, small_full, keys, filt, what, word):
    with pytest.raises(fl.FlsError) as e:
        small_full.aggregate_grouped(keys, [("count",)], filt=filt)
    assert e.value.code == ERR_ARG, e.value
    if what:
        assert what + ":" in e.value.msg, e.value
    if word:
        assert word in e.value.msg, e.value


def test_float_and_blob_keys_are_argument_errors(fl):
    n = 1500
    img = fl.write_image([("i", fl.INT32, np.arange(n, dtype=np.int32) % 3, fl.ENC_AUTO),
                          ("d", fl.DOUBLE, np.arange(n) % 2 * 0.5, fl.ENC_AUTO),
                          ("f", fl.FLOAT, (np.arange(n) % 2).astype(np.float32), fl.ENC_AUTO),
                          ("b", fl.BLOB, [b"x", b"y"] * (n // 2), fl.ENC_DICT)], rowgroup=1024)
    t = fl.Connection([0]).read_image(img)
    for c in (1, 2, 3):
        with pytest.raises(fl.FlsError) as e:
            t.aggregate_grouped([0, c], [("count",)])
        assert e.value.code == ERR_ARG and "key 1:" in e.value.msg, e.value
    t.close()


@pytest.mark.parametrize("aggs,what", [
    ([], None),
    ([("count",)] * 33, None),
    ([("count",), ("sum", 99)], "aggregate 1"),
    ([("count",), ("count",), (9, C_QTY)], "aggregate 2"),
    ([("sum", C_MODE)], "aggregate 0"),
    ([("sum_product", C_QTY, C_MODE)], "aggregate 0"),
    ([("sum_product", C_QTY, 99)], "aggregate 0"),
])
def test_aggregate_argument_errors_through_the_grouped_call(fl, small_full, aggs, what):
    with pytest.raises(fl.FlsError) as e:
        small_full.aggregate_grouped([C_RFLAG], aggs)
    assert e.value.code == ERR_ARG, e.value
    if what:
        assert what + ":" in e.value.msg, e.value


def test_sum_product_overflow_guard_through_the_grouped_call(fl):
    rng = np.random.default_rng(11)
    n = 3000
    a = rand64(rng, n).view(np.int64)
    b = rand64(rng, n).view(np.int64)
    a[0], b[0] = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    img = fl.write_image([("a", fl.INT64, a, fl.ENC_AUTO), ("b", fl.INT64, b, fl.ENC_AUTO),
                          ("k", fl.INT8, (np.arange(n) % 3).astype(np.int8), fl.ENC_AUTO)], rowgroup=1024)
    t = fl.Connection([0]).read_image(img)
    with pytest.raises(fl.FlsError) as e:
        t.aggregate_grouped([2], [("sum_product", 0, 1)])
    assert e.value.code == ERR_ARG and "aggregate 0:" in e.value.msg and "may overflow 128 bits" in e.value.msg
    t.close()


def test_no_row_group_to_read_needs_no_gpu(fl):
    t = fl.Connection([0]).read_image(fl.gen_image("lineitem", 0.1))
    aggs = [("count",), ("sum", C_QTY), ("min", C_SHIPDATE)]
    assert t.aggregate_grouped([C_RFLAG, C_STATUS], aggs, filt=[(C_PART, "<", 0)]) == []
    assert t.pruned == t.nrowgroups == 10
    # an empty row-group range: the same, nothing pruned
    assert t.aggregate_grouped([C_LINE], aggs, rg_begin=3, rg_end=3) == []
    assert t.pruned == 0
    t.close()


def test_group_kernel_resources():
    """both kernels keep their state in registers and LDS: no scratch, no spill"""
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    res = kernel_resources.resources(str(LIB))
    for kernel in ("group_vector_kernel", "group_rowgroup_kernel"):
        hits = {k: v for k, v in res.items() if kernel in k}
        assert len(hits) == 1, (kernel, hits)
        for name, r in hits.items():
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)


# ------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def conn0(fl):
    conn = fl.Connection([0])
    yield conn
    conn.close()


RG1 = 2048
N1 = 2 * RG1 + 1024 + 37   # three row groups; the last: one full vector and a 37-row tail vector


# ---- 1. integer keys of every type and encoding
@pytest.fixture(scope="module")
def intkeys(fl, conn0):
    rng = np.random.default_rng(20250117)
    n = N1

    def few(dt, extra=(-3, 0, 7)):
        ii = np.iinfo(dt)
        pool = sorted({ii.min, ii.max} | {v for v in extra if ii.min <= v <= ii.max})
        return np.array(pool, dtype=dt)[rng.integers(0, len(pool), n)]

    def full(dt):
        ii = np.iinfo(dt)
        if ii.bits == 64:
            return rand64(rng, n).view(dt)
        return rng.integers(ii.min, int(ii.max) + 1, n).astype(dt)

    big = (rand64(rng, n) >> np.uint64(2)) | np.uint64(1 << 62)          # [2^62, 2^63)
    dec_pool = np.array([-999999999999999999, -1, 0, 250, 999999999999999999], dtype=np.int64)
    date_pool = np.array([-2**31, -1, 0, 10957, 2**31 - 1], dtype=np.int32)
    runs = np.repeat(np.array([-2**31, 5, 2**31 - 1], np.int32)[rng.integers(0, 3, (n + 49) // 50)], 50)[:n]
    spec = [
        # keys: at most five values each, the type's extremes among them
        ("k_i8", fl.INT8, few(np.int8), fl.ENC_AUTO), ("k_i16", fl.INT16, few(np.int16), fl.ENC_AUTO),
        ("k_i32", fl.INT32, few(np.int32), fl.ENC_AUTO), ("k_i64", fl.INT64, few(np.int64), fl.ENC_AUTO),
        ("k_u8", fl.UINT8, few(np.uint8), fl.ENC_AUTO), ("k_u16", fl.UINT16, few(np.uint16), fl.ENC_AUTO),
        ("k_u32", fl.UINT32, few(np.uint32), fl.ENC_AUTO), ("k_u64", fl.UINT64, few(np.uint64), fl.ENC_AUTO),
        ("k_b", fl.BOOLEAN, rng.integers(0, 2, n).astype(np.uint8), fl.ENC_AUTO),
        ("k_dt", fl.DATE, date_pool[rng.integers(0, 5, n)], fl.ENC_AUTO),
        ("k_dec", fl.DECIMAL, dec_pool[rng.integers(0, 5, n)], fl.ENC_AUTO, 18, 2),
        ("k_dict", fl.INT16, few(np.int16), fl.ENC_DICT),
        ("k_rle", fl.INT32, runs, fl.ENC_RLE),
        ("k_delta", fl.INT64, np.sort(few(np.int64)), fl.ENC_DELTA),
        # operands over the full range
        ("i8", fl.INT8, full(np.int8), fl.ENC_AUTO), ("i16", fl.INT16, full(np.int16), fl.ENC_AUTO),
        ("i32", fl.INT32, full(np.int32), fl.ENC_AUTO), ("i64", fl.INT64, full(np.int64), fl.ENC_AUTO),
        ("u64", fl.UINT64, full(np.uint64), fl.ENC_AUTO), ("big", fl.INT64, big.astype(np.int64), fl.ENC_AUTO),
    ]
    img = fl.write_image(spec, rowgroup=RG1)
    cols = {c: s[2] for c, s in enumerate(spec)}
    t = conn0.read_image(img)
    yield img, cols, [s[0] for s in spec], t
    t.close()


NKEYCOLS = 14
O_I8, O_I16, O_I32, O_I64, O_U64, O_BIG = 14, 15, 16, 17, 18, 19
INT_AGGS = [("count",), ("count", O_I8), ("sum", O_I64), ("min", O_I32), ("max", O_I32), ("sum", O_BIG),
            ("sum_product", O_I32, O_I16), ("sum", O_U64), ("min", O_U64), ("max", O_I8), ("min", O_I64)]


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [None, [(O_I32, "<", 0)]], ids=["all", "i32_negative"])
def test_gpu_integer_keys_of_every_type_and_encoding(fl, gpu, intkeys, filt):
    img, cols, names, t = intkeys
    assert t.nrowgroups == 3 and t.nrows == N1
    sel = filter_mask(cols, filt, N1) if filt else np.ones(N1, bool)
    for k in range(NKEYCOLS):
        got = t.aggregate_grouped([k], INT_AGGS, filt=filt)
        assert 1 < len(got) <= 5, (names[k], len(got))
        check_groups(got, [k], INT_AGGS, cols, {}, sel, names[k])
        if filt is None:   # the [2^62, 2^63) column passes 2^64 inside every group
            assert all(vals[5] > 2**64 for _, vals in got), names[k]
    # the extremes came back sign- / zero-extended by column type
    assert {k[0] for k, _ in t.aggregate_grouped([0], [("count",)])} >= {-128, 127}
    assert {k[0] for k, _ in t.aggregate_grouped([7], [("count",)])} >= {0, 2**64 - 1}
    assert {k[0] for k, _ in t.aggregate_grouped([3], [("count",)])} >= {-2**63, 2**63 - 1}


# ---- 2. DICT VARCHAR keys: dictionaries that differ per row group, 2-byte codes
LONG = "a string longer than twelve bytes"


@pytest.fixture(scope="module")
def strkeys(fl, conn0):
    rng = np.random.default_rng(7)
    n = N1
    pools = [["A", "B"], ["B", "C", LONG], ["C"]]
    s = []
    for i in range(n):
        p = pools[min(i // RG1, 2)]
        s.append(p[int(rng.integers(0, len(p)))])
    # w: 300 strings per row group, every one of them in every vector; the
    # filter f = 1 leaves 40 of them (codes stay 2 bytes wide: the chunk's
    # dictionary has 300 entries)
    w = [f"w{i % 300:03d}-{i // RG1}" for i in range(n)]
    f = np.array([1 if i % 300 < 40 else 0 for i in range(n)], dtype=np.int8)
    x = rng.integers(-10**6, 10**6, n).astype(np.int32)
    img = fl.write_image([("s", fl.VARCHAR, s, fl.ENC_DICT), ("w", fl.VARCHAR, w, fl.ENC_DICT),
                          ("f", fl.INT8, f, fl.ENC_AUTO), ("x", fl.INT32, x, fl.ENC_AUTO)], rowgroup=RG1)
    t = conn0.read_image(img)
    cols = {0: [v.encode() for v in s], 1: [v.encode() for v in w], 2: f, 3: x}
    yield t, cols
    t.close()


STR_AGGS = [("count",), ("sum", 3), ("min", 3), ("max", 3), ("count", 1)]


@pytest.mark.gpu
def test_gpu_varchar_keys_merge_by_string_across_row_groups(fl, gpu, strkeys):
    t, cols = strkeys
    assert t.nrowgroups == 3
    every = np.ones(N1, bool)
    got = t.aggregate_grouped([0], STR_AGGS)
    check_groups(got, [0], STR_AGGS, cols, {}, every, "s")
    assert sorted(k[0] for k, _ in got) == [b"A", b"B", b"C", LONG.encode()]   # B and C: one group each
    # one row group at a time: the codes mean that row group's strings
    for rg in range(3):
        rows = np.zeros(N1, bool)
        rows[rg * RG1:(rg + 1) * RG1] = True
        check_groups(t.aggregate_grouped([0], STR_AGGS, rg_begin=rg, rg_end=rg + 1), [0], STR_AGGS, cols, {}, rows,
                     f"s rg {rg}")
    # under a filter on another column
    filt = [(3, ">", 0)]
    check_groups(t.aggregate_grouped([0], STR_AGGS, filt=filt), [0], STR_AGGS, cols, {}, filter_mask(cols, filt, N1),
                 "s where x > 0")


@pytest.mark.gpu
def test_gpu_varchar_key_with_two_byte_codes(fl, gpu, strkeys):
    t, cols = strkeys
    filt = [(2, "=", 1)]
    sel = filter_mask(cols, filt, N1)
    got = t.aggregate_grouped([1], STR_AGGS, filt=filt)
    assert len(got) == 3 * 40
    check_groups(got, [1], STR_AGGS, cols, {}, sel, "w where f = 1")
    got = t.aggregate_grouped([2, 1], STR_AGGS, filt=filt)
    check_groups(got, [2, 1], STR_AGGS, cols, {}, sel, "f, w where f = 1")
    # unfiltered every vector holds 300 keys: past the per-vector capacity
    with pytest.raises(fl.FlsError) as e:
        t.aggregate_grouped([1], STR_AGGS)
    assert e.value.code == ERR_LIMIT, e.value


# ---- 3. several keys, NULLs in keys and operands
RG2 = 1024
N2 = 3 * RG2 + 5


@pytest.fixture(scope="module")
def mixed(fl, conn0):
    rng = np.random.default_rng(31)
    n = N2
    sv = rng.random(n) >= 0.25
    sv[RG2:2 * RG2] = False                       # row group 1: the key chunk entirely NULL
    s = [["ab", LONG][int(rng.integers(0, 2))] if sv[i] else None for i in range(n)]
    d = np.array([-5, 19000], dtype=np.int32)[rng.integers(0, 2, n)]
    dv = rng.random(n) >= 0.2
    k = np.array([-128, 127], dtype=np.int8)[rng.integers(0, 2, n)]
    kv = rng.random(n) >= 0.1
    b = rng.integers(0, 2, n).astype(np.uint8)
    # placeholders: the writer stores 0 at the masked rows, which is no key value of d or k
    x = np.where(np.arange(n) < RG2, rng.integers(1000, 2000, n), rng.integers(-5000, -4000, n)).astype(np.int32)
    xv = rng.random(n) >= 0.3
    y = np.round(rng.normal(0, 10, n), 2)
    yv = rng.random(n) >= 0.2
    img = fl.write_image([("s", fl.VARCHAR, s, fl.ENC_DICT), ("d", fl.DATE, np.ma.array(d, mask=~dv), fl.ENC_AUTO),
                          ("k", fl.INT8, np.ma.array(k, mask=~kv), fl.ENC_AUTO), ("b", fl.BOOLEAN, b, fl.ENC_AUTO),
                          ("x", fl.INT32, np.ma.array(x, mask=~xv), fl.ENC_AUTO),
                          ("y", fl.DOUBLE, np.ma.array(y, mask=~yv), fl.ENC_AUTO)], rowgroup=RG2)
    t = conn0.read_image(img)
    cols = {0: [v.encode() if v is not None else None for v in s], 1: d, 2: k, 3: b, 4: x, 5: y}
    valid = {0: sv, 1: dv, 2: kv, 4: xv, 5: yv}
    yield img, t, cols, valid
    t.close()


MIX_AGGS = [("count",), ("count", 4), ("sum", 4), ("min", 4), ("max", 4), ("sum", 5), ("min", 5), ("count", 0),
            ("sum_product", 4, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("keys", [[0, 1], [0, 1, 2, 3], [2], [3, 0]], ids=["s_d", "s_d_k_b", "k", "b_s"])
def test_gpu_mixed_keys_with_nulls(fl, gpu, mixed, keys):
    img, t, cols, valid = mixed
    assert t.nrowgroups == 4
    for terms in ([], [(4, "is_not_null", None), (5, ">", 0.0)], [(2, "is_null", None)], [(4, "<", 0)]):
        sel = null_aware_mask(cols, valid, terms, N2)
        got = t.aggregate_grouped(keys, MIX_AGGS, filt=terms)
        check_groups(got, keys, MIX_AGGS, cols, valid, sel, f"{keys} under {terms}")
        assert sum(vals[0] for _, vals in got) == int(sel.sum())
        if terms == [(4, "<", 0)] and 0 in keys:
            # x < 0 leaves row groups 1.. only; a NULL key is one group, never a placeholder string
            assert any(k[keys.index(0)] is None for k, _ in got) and all(k[keys.index(0)] != b"" for k, _ in got)
    # the all-NULL key chunk alone, and the 5-row tail
    for r0, r1 in ((1, 2), (3, 4)):
        rows = np.zeros(N2, bool)
        rows[r0 * RG2:min(N2, r1 * RG2)] = True
        check_groups(t.aggregate_grouped(keys, MIX_AGGS, rg_begin=r0, rg_end=r1), keys, MIX_AGGS, cols, valid, rows,
                     f"{keys} rg [{r0},{r1})")


# ---- 4. rows that must not make a group
@pytest.mark.gpu
def test_gpu_filtered_out_and_tail_rows_make_no_group(fl, gpu, conn0):
    rng = np.random.default_rng(5)
    n = N1
    f = rng.integers(0, 2, n).astype(np.int8)
    k = np.where(f == 1, rng.integers(1, 4, n), 99).astype(np.int32)    # 99 only where the filter fails
    kv = rng.random(n) >= 0.1                                          # NULL keys: the placeholder 0 is no key value
    x = rng.integers(-100, 100, n).astype(np.int64)
    img = fl.write_image([("k", fl.INT32, np.ma.array(k, mask=~kv), fl.ENC_AUTO), ("f", fl.INT8, f, fl.ENC_AUTO),
                          ("x", fl.INT64, x, fl.ENC_AUTO)], rowgroup=RG1)
    t = conn0.read_image(img)
    cols, valid = {0: k, 1: f, 2: x}, {0: kv}
    aggs = [("count",), ("sum", 2), ("count", 0)]
    try:
        filt = [(1, "=", 1)]
        sel = filter_mask(cols, filt, n)
        got = t.aggregate_grouped([0], aggs, filt=filt)
        check_groups(got, [0], aggs, cols, valid, sel, "k where f = 1")
        assert {key[0] for key, _ in got} == {1, 2, 3, None}
        # unfiltered: 99 is a group, the placeholder 0 is not, and the 37-row tail adds no row
        got = t.aggregate_grouped([0], aggs)
        check_groups(got, [0], aggs, cols, valid, np.ones(n, bool), "k")
        assert {key[0] for key, _ in got} == {1, 2, 3, 99, None}
        assert sum(vals[0] for _, vals in got) == n
        # the last row group alone: 1024 + 37 rows, no group from beyond them
        rows = np.zeros(n, bool)
        rows[2 * RG1:] = True
        got = t.aggregate_grouped([0], aggs, rg_begin=2, rg_end=3)
        check_groups(got, [0], aggs, cols, valid, rows, "k, last row group")
        assert sum(vals[0] for _, vals in got) == 1024 + 37
    finally:
        t.close()


# ---- 5. the capacities
RG5 = 8192
N5 = RG5 + 64     # the second row group: 64 rows, so 64 of k65's keys


@pytest.fixture(scope="module")
def limits(fl, conn0):
    i = np.arange(N5)
    v, r = (i % RG5) // 1024, i % 1024
    # vectors 0..3 of a row group hold 64 keys each, disjoint: 256 in the row
    # group; vectors 4..7 repeat the first 64
    k256 = np.where(v < 4, 64 * v + r % 64, r % 64).astype(np.int16)
    k257 = k256.copy()
    k257[4 * 1024 + 63::64][:16] = 256           # vector 4: key 63 gives way to a 257th key (still 64 in the vector)
    k65 = (r % 65).astype(np.int16)              # 65 keys in every vector
    small = (i % 3).astype(np.int8)
    x = (i * 7 % 1000 - 500).astype(np.int32)
    img = fl.write_image([("k256", fl.INT16, k256, fl.ENC_AUTO), ("k257", fl.INT16, k257, fl.ENC_AUTO),
                          ("k65", fl.INT16, k65, fl.ENC_AUTO), ("small", fl.INT8, small, fl.ENC_AUTO),
                          ("x", fl.INT32, x, fl.ENC_AUTO)], rowgroup=RG5)
    t = conn0.read_image(img)
    yield t, {0: k256, 1: k257, 2: k65, 3: small, 4: x}
    t.close()


LIM_AGGS = [("count",), ("sum", 4), ("min", 4)]


@pytest.mark.gpu
def test_gpu_capacities_are_guarded(fl, gpu, limits):
    t, cols = limits
    every = np.ones(N5, bool)
    assert t.nrowgroups == 2
    assert len(set(cols[1][4096:5120].tolist())) == 64 and len(set(cols[1][:RG5].tolist())) == 257

    def still_works():
        check_groups(t.aggregate_grouped([3], LIM_AGGS), [3], LIM_AGGS, cols, {}, every, "small")
        assert t.aggregate([("count",), ("sum", 4)]) == [N5, int(cols[4].astype(np.int64).sum())]

    # 64 keys in a vector, 4 x 64 = 256 in the row group: within both capacities
    got = t.aggregate_grouped([0], LIM_AGGS)
    assert len(got) == 256
    check_groups(got, [0], LIM_AGGS, cols, {}, every, "k256")
    # a 65th key in a vector
    with pytest.raises(fl.FlsError) as e:
        t.aggregate_grouped([2], LIM_AGGS)
    assert e.value.code == ERR_LIMIT and "64" in e.value.msg and "scan" in e.value.msg, e.value
    still_works()
    # a 257th key in a row group
    with pytest.raises(fl.FlsError) as e:
        t.aggregate_grouped([1], LIM_AGGS)
    assert e.value.code == ERR_LIMIT and "256" in e.value.msg and "scan" in e.value.msg, e.value
    still_works()
    # the second row group alone has 64 keys of k65's 65: fine
    rows = np.zeros(N5, bool)
    rows[RG5:] = True
    check_groups(t.aggregate_grouped([2], LIM_AGGS, rg_begin=1, rg_end=2), [2], LIM_AGGS, cols, {}, rows, "k65 tail")
    # a filter that leaves 64 of the 65 in every vector: the capacity counts selected rows
    filt = [(2, "<", 64)]
    check_groups(t.aggregate_grouped([2], LIM_AGGS, filt=filt), [2], LIM_AGGS, cols, {}, filter_mask(cols, filt, N5),
                 "k65 < 64")


# ---- 6. one group equals the ungrouped call, bit for bit
@pytest.fixture(scope="module")
def floats(fl, conn0):
    rng = np.random.default_rng(4242)
    n = N1
    d = np.round(rng.normal(0, 10, n), 2)
    f = d.astype(np.float32)
    pool = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e300, 1.5, -1.5])
    g = pool[rng.integers(0, len(pool), n)]
    z = np.array([0.0, -0.0])[rng.integers(0, 2, n)]
    i = rand64(rng, n).view(np.int64)
    one = np.full(n, 7, dtype=np.int8)
    few = (np.arange(n) * 2654435761 % 5).astype(np.int8)
    img = fl.write_image([("d", fl.DOUBLE, d, fl.ENC_AUTO), ("f", fl.FLOAT, f, fl.ENC_AUTO),
                          ("g", fl.DOUBLE, g, fl.ENC_AUTO), ("z", fl.DOUBLE, z, fl.ENC_AUTO),
                          ("i", fl.INT64, i, fl.ENC_AUTO), ("one", fl.INT8, one, fl.ENC_AUTO),
                          ("few", fl.INT8, few, fl.ENC_AUTO)], rowgroup=RG1)
    t = conn0.read_image(img)
    yield img, {0: d, 1: f, 2: g, 3: z, 4: i, 5: one, 6: few}, t
    t.close()


FLOAT_AGGS = [("count",)] + [(fn, c) for c in (0, 1, 2, 3, 4) for fn in ("sum", "min", "max", "count")]


@pytest.mark.gpu
def test_gpu_one_group_equals_the_ungrouped_call_bit_for_bit(fl, gpu, floats):
    img, cols, t = floats
    for filt in (None, [(0, ">", 2.5)], [(2, "<", 1e300), (2, ">", -1e300)], [(4, "<", 0)]):
        plain = t.aggregate(FLOAT_AGGS, filt=filt)
        got = t.aggregate_grouped([5], FLOAT_AGGS, filt=filt)
        assert len(got) == 1 and got[0][0] == (7,)
        assert [bits(v) for v in got[0][1]] == [bits(v) for v in plain], filt
    # (the ungrouped sums above are the ones test_aggregate.py checks against math.fsum)
    assert math.isnan(t.aggregate_grouped([5], [("sum", 2)])[0][1][0])


@pytest.mark.gpu
def test_gpu_float_sums_per_group(fl, gpu, floats):
    img, cols, t = floats
    aggs = [("count",), ("sum", 0), ("sum", 1), ("min", 0), ("max", 1), ("min", 2), ("max", 2), ("sum", 4)]
    for filt in (None, [(0, ">", 2.5)]):
        sel = filter_mask(cols, filt, N1) if filt else np.ones(N1, bool)
        check_groups(t.aggregate_grouped([6], aggs, filt=filt), [6], aggs, cols, {}, sel, f"few under {filt}")


# ---- 7. reproducibility
@pytest.mark.gpu
def test_gpu_results_are_bit_identical_across_batches_and_pipelines(fl, gpu, floats, mixed, monkeypatch):
    fimg, fcols, tf = floats
    mimg, tm, mcols, mvalid = mixed
    faggs = [("count",), ("sum", 0), ("sum", 1), ("sum", 4), ("min", 2)]

    def run(tf, tm):   # (the batch size is read when a scan starts)
        return (as_bits(tf.aggregate_grouped([6], faggs)), as_bits(tf.aggregate_grouped([6], faggs, filt=[(0, ">", 2.5)])),
                as_bits(tm.aggregate_grouped([0, 1, 2, 3], MIX_AGGS)))

    monkeypatch.delenv("FLS_SCAN_BATCH", raising=False)
    base = run(tf, tm)
    check_groups(tm.aggregate_grouped([0, 1, 2, 3], MIX_AGGS), [0, 1, 2, 3], MIX_AGGS, mcols, mvalid, np.ones(N2, bool))
    for batch in ("1", "3", "8"):
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)
        assert run(tf, tm) == base, batch
    monkeypatch.setenv("FLS_SCAN_BATCH", "1")
    monkeypatch.setenv("FLS_SCAN_SLOTS", "4")       # four batches in flight, the last two on recycled host batches
    assert run(tf, tm) == base, "batch 1, four slots"
    monkeypatch.delenv("FLS_SCAN_SLOTS")
    # the row groups sharded over two pipelines (the same GPU listed twice)
    monkeypatch.setenv("FLS_SCAN_BATCH", "3")
    conn2 = fl.Connection([0, 0])
    tf2, tm2 = conn2.read_image(fimg), conn2.read_image(mimg)
    try:
        assert run(tf2, tm2) == base, "batch 3, two pipelines"
        monkeypatch.delenv("FLS_SCAN_BATCH")
        assert run(tf2, tm2) == base, "default batch, two pipelines"
    finally:
        tf2.close()
        tm2.close()
        conn2.close()


# ---- 8. lineitem
SF = 0.1
WL = "lineitem"


@pytest.fixture(scope="module")
def lineitem(fl, conn0):
    img = fl.gen_image(WL, SF)
    t = conn0.read_image(img)
    n = t.nrows
    cols, words = {}, {}
    for c, (name, ty, _, _, _) in enumerate(t.schema()):
        if ty == fl.VARCHAR:
            cols[c] = fl.gen_values(WL, c, 0, n, np.uint32, SF)     # dictionary codes of the generator
            words[c] = []
            while (s := fl.gen_dict_string(WL, c, len(words[c]))) is not None:
                words[c].append(s.encode())
        else:
            cols[c] = fl.gen_values(WL, c, 0, n, fl.NP_DTYPE[ty], SF)
    yield t, cols, words
    t.close()


def lineitem_groups(cols, words, keys, sel):
    """[(key tuple, row mask)] in first-occurrence order, by numpy"""
    idx = np.nonzero(sel)[0]
    combo = np.zeros(len(idx), dtype=np.int64)
    for c in keys:
        combo = combo * 1000 + cols[c][idx].astype(np.int64)
    _, first, inv = np.unique(combo, return_index=True, return_inverse=True)
    out = []
    for u in np.argsort(first):
        rows = idx[inv == u]
        key = tuple(words[c][int(cols[c][rows[0]])] if c in words else int(cols[c][rows[0]]) for c in keys)
        out.append((key, rows))
    return out


Q1_AGGS = [("sum", C_QTY), ("sum", C_PRICE), ("sum_product", C_PRICE, C_DISC), ("sum", C_DISC), ("count",),
           ("min", C_SHIPDATE), ("max", C_SHIPDATE), ("count", C_MODE)]


@pytest.mark.gpu
@pytest.mark.parametrize("keys,terms", [([C_RFLAG, C_STATUS], [(C_SHIPDATE, "<=", Q1_DAY)]), ([C_MODE, C_LINE], Q6)],
                         ids=["q1", "mode_line_q6"])
def test_gpu_lineitem_grouped(fl, gpu, lineitem, keys, terms):
    t, cols, words = lineitem
    assert t.nrowgroups == 10   # the default batch of 8 splits it
    strs = {c: [words[c][k] for k in cols[c]] for c in words if any(term[0] == c for term in terms)}
    sel = filter_mask({**cols, **strs}, terms, t.nrows)
    want = lineitem_groups(cols, words, keys, sel)
    got = t.aggregate_grouped(keys, Q1_AGGS, filt=terms)
    assert [k for k, _ in got] == [k for k, _ in want]
    assert len(got) > 1
    for (key, vals), (_, rows) in zip(got, want):
        qty, price, disc, ship = (cols[c][rows].astype(np.int64) for c in (C_QTY, C_PRICE, C_DISC, C_SHIPDATE))
        assert vals == [int(qty.sum()), int(price.sum()), int((price * disc).sum()), int(disc.sum()), len(rows),
                        int(ship.min()), int(ship.max()), len(rows)], key
    assert t.pruned == sum(not t.may_match(rg, terms) for rg in range(t.nrowgroups))
    # the grouped results add up to the ungrouped call's
    plain = t.aggregate(Q1_AGGS[:5], filt=terms)
    assert [sum(vals[i] for _, vals in got) for i in range(5)] == plain
