"""Hash aggregate pushdown: GROUP BY on keys of any cardinality, reduced in a
hash table in HBM (fls_aggregate_hashed / Table.aggregate_hashed;
csrc/fls_hashagg.hip).

Expected values come from the inputs themselves -- the arrays handed to
write_image, or the seeded generators -- grouped in Python with exact integers:
tests/test_group_aggregate.py's groups_of / check_groups where the groups are
few, one pass over the selected rows into a dictionary (py_groups) where they
are thousands.  Keys, first rows, counts, integer results, MIN / MAX and
NULL-ness compare exactly; the call returns no binary64 sum.

CPU tests: the exported symbols, every argument error, the 63-bit limit of the
packed key, the call that passes its checks and fails on the missing GPU, the
all-pruned call, the kernels' resources.  GPU tests: every key type and
encoding, NULL keys and operands, more groups than rows per vector, the
tightest table, the limit, one key over every batch, 128-bit carries, MIN /
MAX, rows that make no group and first rows, equality with the grouped call,
reproducibility across batch sizes, slots and pipelines, the Q18 shape."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import filter_mask, rand64
from test_aggregate import null_aware_mask, same_float
from test_group_aggregate import (C_DISC, C_LINE, C_MODE, C_OKEY, C_PRICE, C_QTY, C_SHIPDATE, Q6, as_bits,
                                  check_groups, groups_of)

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "duckdb-fastlane_amd" / "libflsgpu.so"

ERR_ARG, ERR_DEVICE, ERR_LIMIT = -3, -4, -8
RG = 1024


# ------------------------------------------------------------ expected values
def py_groups(cols, valid, keys, aggs, sel, first_row=0):
    """{key tuple: (first selected row, values)} by one pass over the selected
    rows in exact Python integers; aggs as aggregate() takes them (no float
    sums); a NULL key element is None"""
    every = np.ones(len(sel), bool)
    kc = [cols[c].tolist() for c in keys]
    kv = [valid.get(c, every).tolist() for c in keys]
    ops = []
    for a in aggs:
        if len(a) == 1:
            ops.append(("star", None, None))
        elif a[0] == "sum_expr":
            m = every.copy()
            for _, _, c in a[1]:
                m &= valid.get(c, every)
            ops.append(("expr", [(k, s, cols[c].tolist()) for k, s, c in a[1]], m.tolist()))
        elif a[0] == "sum_product":
            ops.append(("prod", (cols[a[1]].tolist(), cols[a[2]].tolist()),
                        (valid.get(a[1], every) & valid.get(a[2], every)).tolist()))
        else:
            ops.append((a[0], cols[a[1]].tolist(), valid.get(a[1], every).tolist()))
    out = {}
    for i in np.nonzero(sel)[0].tolist():
        key = tuple(c[i] if v[i] else None for c, v in zip(kc, kv))
        g = out.get(key)
        if g is None:
            g = out[key] = (first_row + i, [0 if op[0] in ("star", "count") else None for op in ops])
        vals = g[1]
        for j, (op, x, ok) in enumerate(ops):
            if op == "star":
                vals[j] += 1
                continue
            if not ok[i]:
                continue
            if op == "count":
                vals[j] += 1
                continue
            if op == "expr":
                v = 1
                for k, s, col in x:
                    v *= k + s * col[i]
            elif op == "prod":
                v = x[0][i] * x[1][i]
            else:
                v = x[i]
            if vals[j] is None:
                vals[j] = v
            elif op == "min":
                vals[j] = min(vals[j], v)
            elif op == "max":
                vals[j] = max(vals[j], v)
            else:
                vals[j] += v
    return out


def as_dict(h):
    """a HashGroups as {key tuple: (first row, values)}; every key once"""
    rows = h.to_list(ordered=False)
    out = {k: (int(f), v) for (k, v), f in zip(rows, h.first_row.tolist())}
    assert len(out) == len(rows) == len(h), "a key came back twice"
    return out


def check_hashed(h, cols, valid, keys, aggs, sel, first_row=0, what=""):
    want = py_groups(cols, valid, keys, aggs, sel, first_row)
    got = as_dict(h)
    assert got.keys() == want.keys(), (what, len(got), len(want))
    for k, w in want.items():
        assert got[k] == w, (what, k, got[k], w)
    # the canonical order: by first row
    assert [k for k, _ in h.to_list()] == sorted(want, key=lambda k: want[k][0]), what


# ------------------------------------------------------------------ CPU tests
def accepted(fl, call):
    """call() gets past every argument check: without a GPU its table cannot
    be allocated, and the error names the bytes; with one it returns"""
    if fl.device_count() > 0:
        return call()
    with pytest.raises(fl.FlsError) as e:
        call()
    assert e.value.code == ERR_DEVICE and "bytes" in e.value.msg, e.value
    return None


def test_library_exports_the_hashed_call(_built):
    lib = C.CDLL(str(LIB))
    for name in ("fls_aggregate_hashed", "fls_hash_result_ngroups", "fls_hash_result_first_rows",
                 "fls_hash_result_key", "fls_hash_result_aggregate", "fls_hash_result_free"):
        assert hasattr(lib, name), name


@pytest.fixture(scope="module")
def small_full(fl):
    t = fl.Connection([0]).read_image(fl.gen_image("lineitem_full", 0.01))
    yield t
    t.close()


C_RFLAG = 8


@pytest.mark.parametrize("keys,what,word", [
    ([], None, "keys"),                                               # nkeys == 0
    ([C_LINE, C_QTY, C_DISC, C_SHIPDATE, C_OKEY], None, "keys"),      # nkeys > 4
    ([C_LINE, 99], "key 1", "out of range"),
    ([99], "key 0", "out of range"),
    ([C_LINE, C_QTY, C_LINE], "key 2", "already"),                    # listed twice
    ([C_LINE, C_RFLAG], "key 1", "VARCHAR"),                          # a dictionary code is no key here
    ([0x80000000], "key 0", "mapped"),                                # FLS_KEY_MAPPED | 0
    ([C_LINE, 0x80000001], "key 1", "mapped"),
])
def test_key_argument_errors(fl, small_full, keys, what, word):
    with pytest.raises(fl.FlsError) as e:
        small_full.aggregate_hashed(keys, [("count",)], 1000)
    assert e.value.code == ERR_ARG, e.value
    if what:
        assert what + ":" in e.value.msg, e.value
    assert word in e.value.msg, e.value


def test_float_and_blob_keys_are_argument_errors(fl):
    n = 1500
    img = fl.write_image([("i", fl.INT32, np.arange(n, dtype=np.int32) % 3, fl.ENC_AUTO),
                          ("d", fl.DOUBLE, np.arange(n) % 2 * 0.5, fl.ENC_AUTO),
                          ("f", fl.FLOAT, (np.arange(n) % 2).astype(np.float32), fl.ENC_AUTO),
                          ("b", fl.BLOB, [b"x", b"y"] * (n // 2), fl.ENC_DICT)], rowgroup=RG)
    t = fl.Connection([0]).read_image(img)
    for c in (1, 2, 3):
        with pytest.raises(fl.FlsError) as e:
            t.aggregate_hashed([0, c], [("count",)], 16)
        assert e.value.code == ERR_ARG and "key 1:" in e.value.msg, e.value
    # a FLOAT / DOUBLE sum is refused by name; MIN / MAX of the same columns pass the checks
    for c in (1, 2):
        with pytest.raises(fl.FlsError) as e:
            t.aggregate_hashed([0], [("count",), ("sum", c)], 16)
        assert e.value.code == ERR_ARG and "aggregate 1:" in e.value.msg and "order-dependent" in e.value.msg, e.value
        accepted(fl, lambda: t.aggregate_hashed([0], [("min", c), ("max", c)], 16))
    t.close()


@pytest.mark.parametrize("aggs,what", [
    ([], None),
    ([("count",)] * 33, None),
    ([("count",), ("sum", 99)], "aggregate 1"),
    ([("count",), ("count",), (9, C_QTY)], "aggregate 2"),
    ([("sum", C_MODE)], "aggregate 0"),
    ([("sum_product", C_QTY, C_MODE)], "aggregate 0"),
    ([("sum_product", C_QTY, 99)], "aggregate 0"),
    ([("count",), (6, 0)], "aggregate 1"),                             # SUM_EXPR without an expression list
])
def test_aggregate_argument_errors_through_the_hashed_call(fl, small_full, aggs, what):
    with pytest.raises(fl.FlsError) as e:
        small_full.aggregate_hashed([C_LINE], aggs, 1000)
    assert e.value.code == ERR_ARG, e.value
    if what:
        assert what + ":" in e.value.msg, e.value


def test_sum_product_overflow_guard_through_the_hashed_call(fl):
    rng = np.random.default_rng(11)
    n = 3000
    a = rand64(rng, n).view(np.int64)
    b = rand64(rng, n).view(np.int64)
    a[0], b[0] = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    img = fl.write_image([("a", fl.INT64, a, fl.ENC_AUTO), ("b", fl.INT64, b, fl.ENC_AUTO),
                          ("k", fl.INT8, (np.arange(n) % 3).astype(np.int8), fl.ENC_AUTO)], rowgroup=RG)
    t = fl.Connection([0]).read_image(img)
    with pytest.raises(fl.FlsError) as e:
        t.aggregate_hashed([2], [("sum_product", 0, 1)], 16)
    assert e.value.code == ERR_ARG and "aggregate 0:" in e.value.msg and "may overflow 128 bits" in e.value.msg
    t.close()


@pytest.mark.parametrize("max_groups", [0, 2**28 + 1])
def test_max_groups_out_of_range(fl, small_full, max_groups):
    with pytest.raises(fl.FlsError) as e:
        small_full.aggregate_hashed([C_LINE], [("count",)], max_groups)
    assert e.value.code == ERR_ARG and "max_groups" in e.value.msg, e.value


def test_packed_key_is_limited_to_63_bits(fl, small_full):
    """The packed key takes, per key, the bits of max - min of its zone maps
    plus a NULL bit.  The generated lineitem's own [l_orderkey, l_quantity]
    needs 16 + 13 + 2 bits at this scale and passes the checks (below); the
    refusal needs the ranges a real fact table has, so the columns here carry
    them: an order key spanning 2^45 and a DECIMAL quantity spanning 2^17."""
    n = 6000
    i = np.arange(n, dtype=np.int64)
    okey = i * ((1 << 45) // n)
    qty = (i % 7) * ((1 << 17) // 7)
    full = np.where(i % 2 == 0, np.iinfo(np.int64).min, np.iinfo(np.int64).max)
    ufull = np.where(i % 2 == 0, np.uint64(0), np.uint64(2**64 - 1))
    img = fl.write_image([("l_orderkey", fl.INT64, okey, fl.ENC_AUTO),
                          ("l_quantity", fl.DECIMAL, qty, fl.ENC_AUTO, 15, 2),
                          ("full", fl.INT64, full, fl.ENC_AUTO),
                          ("u", fl.UINT64, ufull, fl.ENC_AUTO),
                          ("small", fl.INT8, (i % 5).astype(np.int8), fl.ENC_AUTO)], rowgroup=RG)
    t = fl.Connection([0]).read_image(img)
    try:
        with pytest.raises(fl.FlsError) as e:
            t.aggregate_hashed([0, 1], [("count",)], 4096)
        assert e.value.code == ERR_ARG and "key 1:" in e.value.msg and "63" in e.value.msg, e.value
        assert "needs 64 bits" in e.value.msg, e.value                 # 45 + 17 + 2
        # a full-range 64-bit column cannot be a key, alone or after another
        for keys, what in (([2], "key 0:"), ([3], "key 0:"), ([4, 2], "key 1:")):
            with pytest.raises(fl.FlsError) as e:
                t.aggregate_hashed(keys, [("count",)], 4096)
            assert e.value.code == ERR_ARG and what in e.value.msg and "63" in e.value.msg, (keys, e.value)
        # one row group of the six has a narrower range: 43 + 17 + 2 bits, and the pair fits
        accepted(fl, lambda: t.aggregate_hashed([0, 1], [("count",)], 4096, rg_begin=0, rg_end=1))
    finally:
        t.close()
    # 63 bits exactly are accepted: 62 value bits and the NULL bit
    wide = np.array([0, (1 << 62) - 1] * 600, dtype=np.int64)
    t = fl.Connection([0]).read_image(fl.write_image([("w", fl.INT64, wide, fl.ENC_AUTO)], rowgroup=RG))
    h = accepted(fl, lambda: t.aggregate_hashed([0], [("count",)], 16))
    assert h is None or dict(h.to_list()) == {(0,): [600], ((1 << 62) - 1,): [600]}
    t.close()


def test_orderkey_passes_the_checks_and_needs_a_gpu(fl, small_full):
    """l_orderkey alone -- the key fls_aggregate_grouped's limits refuse -- gets
    past every argument check; without a GPU the table cannot be allocated,
    and the error names its bytes"""
    if fl.device_count() > 0:
        h = small_full.aggregate_hashed([C_OKEY], [("count",), ("sum", C_QTY)], 1 << 15)
        assert len(h) == len(np.unique(fl.gen_values("lineitem_full", C_OKEY, 0, small_full.nrows, np.int64, 0.01)))
        return
    for keys in ([C_OKEY], [C_OKEY, C_QTY]):
        with pytest.raises(fl.FlsError) as e:
            small_full.aggregate_hashed(keys, [("count",), ("sum", C_QTY)], 1 << 15)
        assert e.value.code == ERR_DEVICE and "bytes" in e.value.msg, e.value
    # 2^16 slots of 6 fields (the key, the first row, count(*), the sum's count / lo / hi) and the header
    assert str((1 << 16) * 6 * 8 + 128) in e.value.msg, e.value
    # the table stays usable
    assert len(small_full.aggregate_hashed([C_OKEY], [("count",)], 100, filt=[(C_QTY, "<", 0)])) == 0


def test_no_row_group_to_read_needs_no_gpu(fl):
    t = fl.Connection([0]).read_image(fl.gen_image("lineitem", 0.1))
    aggs = [("count",), ("sum", C_QTY), ("min", C_SHIPDATE)]
    h = t.aggregate_hashed([C_OKEY], aggs, 1 << 20, filt=[(1, "<", 0)])
    assert len(h) == 0 and h.to_list() == [] and h.first_row.shape == (0,) and len(h.count) == 3
    assert t.pruned == t.nrowgroups == 10
    # an empty row-group range: the same, nothing pruned
    assert t.aggregate_hashed([C_OKEY, C_LINE], aggs, 1 << 20, rg_begin=3, rg_end=3).to_list() == []
    assert t.pruned == 0
    t.close()


def test_hash_kernel_resources():
    """both kernels keep their state in registers: no scratch, no spill"""
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    res = kernel_resources.resources(str(LIB))
    for kernel in ("hash_insert_kernel", "hash_extract_kernel"):
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


N1 = 4 * RG + 37   # five row groups; the last: a 37-row tail vector


# ---- 1. keys of every integer-like type and encoding
@pytest.fixture(scope="module")
def intkeys(fl, conn0):
    rng = np.random.default_rng(20251020)
    n = N1

    def pool(dt, lo, hi, k=40):
        """k values of [lo, hi], both ends among them"""
        p = np.unique(np.concatenate([[lo, hi], rng.integers(lo, hi, k - 2, dtype=np.int64)]))
        return p.astype(dt)[rng.integers(0, len(p), n)]

    def full(dt):
        ii = np.iinfo(dt)
        if ii.bits == 64:
            return rand64(rng, n).view(dt)
        return rng.integers(ii.min, int(ii.max) + 1, n).astype(dt)

    u64 = (np.uint64(2**64 - 1) - rng.integers(0, 500, n).astype(np.uint64))            # near 2^64
    u64[:2] = [2**64 - 1, 2**64 - 500]
    i64 = np.int64(-2**62) + rng.integers(-300, 300, n)                                 # near -2^62
    big = (rand64(rng, n) >> np.uint64(2)) | np.uint64(1 << 62)                         # [2^62, 2^63)
    runs = np.repeat(np.array([-2**31, 5, 2**31 - 1], np.int64)[rng.integers(0, 3, (n + 49) // 50)], 50)[:n]
    spec = [
        ("k_i8", fl.INT8, full(np.int8), fl.ENC_AUTO),                                   # the whole type
        ("k_i16", fl.INT16, pool(np.int16, -32768, 200), fl.ENC_AUTO),                   # a negative minimum
        ("k_i32", fl.INT32, pool(np.int32, -70000, 70000, 700), fl.ENC_AUTO),            # ~700 groups
        ("k_i64", fl.INT64, i64, fl.ENC_AUTO),
        ("k_u8", fl.UINT8, full(np.uint8), fl.ENC_AUTO),
        ("k_u16", fl.UINT16, pool(np.uint16, 3, 65535), fl.ENC_AUTO),
        ("k_u32", fl.UINT32, pool(np.uint32, 2**31 - 5, 2**32 - 1), fl.ENC_AUTO),
        ("k_u64", fl.UINT64, u64, fl.ENC_AUTO),
        ("k_b", fl.BOOLEAN, rng.integers(0, 2, n).astype(np.uint8), fl.ENC_AUTO),
        ("k_dt", fl.DATE, pool(np.int32, -2**31, 2**31 - 1, 12), fl.ENC_AUTO),            # the whole DATE range
        ("k_dec", fl.DECIMAL, pool(np.int64, -999999999999, 999999999999), fl.ENC_AUTO, 18, 2),
        ("k_dict", fl.INT16, pool(np.int16, -5, 900, 9), fl.ENC_DICT),
        ("k_rle", fl.INT32, runs.astype(np.int32), fl.ENC_RLE),
        ("k_delta", fl.INT64, np.sort(pool(np.int64, -10**9, 10**9, 300)), fl.ENC_DELTA),
        # operands over the full range
        ("i8", fl.INT8, full(np.int8), fl.ENC_AUTO), ("i16", fl.INT16, full(np.int16), fl.ENC_AUTO),
        ("i32", fl.INT32, full(np.int32), fl.ENC_AUTO), ("i64", fl.INT64, full(np.int64), fl.ENC_AUTO),
        ("u64", fl.UINT64, full(np.uint64), fl.ENC_AUTO), ("big", fl.INT64, big.astype(np.int64), fl.ENC_AUTO),
    ]
    img = fl.write_image(spec, rowgroup=RG)
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
    assert t.nrowgroups == 5 and t.nrows == N1
    sel = filter_mask(cols, filt, N1) if filt else np.ones(N1, bool)
    for k in range(NKEYCOLS):
        h = t.aggregate_hashed([k], INT_AGGS, 1024, filt=filt)
        check_hashed(h, cols, {}, [k], INT_AGGS, sel, what=names[k])
        assert len(h) == len(np.unique(cols[k][sel])) > 1, names[k]
    # the extremes came back sign- / zero-extended by column type
    for k, lo, hi in ((0, -128, 127), (7, 2**64 - 500, 2**64 - 1), (3, int(cols[3].min()), int(cols[3].max())),
                      (9, -2**31, 2**31 - 1), (1, -32768, 200)):
        got = {key[0] for key, _ in t.aggregate_hashed([k], [("count",)], 1024).to_list()}
        assert {lo, hi} <= got and min(got) == lo and max(got) == hi, names[k]
    # few groups: the grouped call's own checker, in first-occurrence order
    check_groups(t.aggregate_hashed([8], INT_AGGS, 4, filt=filt).to_list(), [8], INT_AGGS, cols, {}, sel, "k_b")
    check_groups(t.aggregate_hashed([11, 12], INT_AGGS, 64, filt=filt).to_list(), [11, 12], INT_AGGS, cols, {}, sel,
                 "k_dict, k_rle")
    # two, three and four keys of mixed width: 8 + 16 + 18 + 10 bits and four NULL bits
    for keys in ([0, 5], [2, 8, 11], [0, 5, 2, 3]):
        h = t.aggregate_hashed(keys, INT_AGGS, 8192, filt=filt)
        check_hashed(h, cols, {}, keys, INT_AGGS, sel, what=str(keys))


# ---- 1b. NULLs in keys and operands
N2 = 3 * RG + 5


@pytest.fixture(scope="module")
def nullkeys(fl, conn0):
    rng = np.random.default_rng(31)
    n = N2
    d = np.array([-5, 19000, 7], dtype=np.int32)[rng.integers(0, 3, n)]
    dv = rng.random(n) >= 0.2
    k = rng.integers(-128, 128, n).astype(np.int8)
    kv = rng.random(n) >= 0.1
    u = rng.integers(40000, 40400, n).astype(np.uint16)
    uv = rng.random(n) >= 0.25
    uv[RG:2 * RG] = False                         # row group 1: the key chunk entirely NULL
    b = rng.integers(0, 2, n).astype(np.uint8)
    # placeholders: the writer stores 0 at the masked rows, which is outside u's range and no value of d
    x = np.where(np.arange(n) < RG, rng.integers(1000, 2000, n), rng.integers(-5000, -4000, n)).astype(np.int32)
    xv = rng.random(n) >= 0.3
    y = np.round(rng.normal(0, 10, n), 2)
    yv = rng.random(n) >= 0.2
    img = fl.write_image([("u", fl.UINT16, np.ma.array(u, mask=~uv), fl.ENC_AUTO),
                          ("d", fl.DATE, np.ma.array(d, mask=~dv), fl.ENC_AUTO),
                          ("k", fl.INT8, np.ma.array(k, mask=~kv), fl.ENC_AUTO), ("b", fl.BOOLEAN, b, fl.ENC_AUTO),
                          ("x", fl.INT32, np.ma.array(x, mask=~xv), fl.ENC_AUTO),
                          ("y", fl.DOUBLE, np.ma.array(y, mask=~yv), fl.ENC_AUTO)], rowgroup=RG)
    t = conn0.read_image(img)
    cols = {0: u, 1: d, 2: k, 3: b, 4: x, 5: y}
    valid = {0: uv, 1: dv, 2: kv, 4: xv, 5: yv}
    yield img, t, cols, valid
    t.close()


NULL_AGGS = [("count",), ("count", 4), ("sum", 4), ("min", 4), ("max", 4), ("count", 0), ("sum_product", 4, 2),
             ("sum_expr", [(10, 1, 4), (3, -1, 2)]), ("count", 5)]
NULL_TERMS = ([], [(4, "is_not_null", None), (5, ">", 0.0)], [(2, "is_null", None)], [(4, "<", 0)])


@pytest.mark.gpu
@pytest.mark.parametrize("keys", [[0, 1], [0, 1, 2, 3], [2], [3, 0]], ids=["u_d", "u_d_k_b", "k", "b_u"])
def test_gpu_keys_and_operands_with_nulls(fl, gpu, nullkeys, keys):
    img, t, cols, valid = nullkeys
    assert t.nrowgroups == 4
    for terms in NULL_TERMS:
        sel = null_aware_mask(cols, valid, terms, N2)
        h = t.aggregate_hashed(keys, NULL_AGGS, 4096, filt=terms)
        check_hashed(h, cols, valid, keys, NULL_AGGS, sel, what=f"{keys} under {terms}")
        assert int(h.count[0].sum()) == int(sel.sum())
        if 0 in keys:   # a NULL key is one group per combination of the others, never the placeholder 0
            q = keys.index(0)
            assert h.key_null[q].any() and not (h.key_values[q][~h.key_null[q]] == 0).any()
            assert (h.key_values[q][h.key_null[q]] == 0).all()
    # the all-NULL key chunk alone, and the 5-row tail
    for r0, r1 in ((1, 2), (3, 4)):
        rows = np.zeros(N2, bool)
        rows[r0 * RG:min(N2, r1 * RG)] = True
        check_hashed(t.aggregate_hashed(keys, NULL_AGGS, 4096, rg_begin=r0, rg_end=r1), cols, valid, keys, NULL_AGGS,
                     rows, what=f"{keys} rg [{r0},{r1})")
    # few groups through the grouped call's checker (no sum_expr there)
    aggs = NULL_AGGS[:7]
    check_groups(t.aggregate_hashed([1, 3], aggs, 16).to_list(), [1, 3], aggs, cols, valid, np.ones(N2, bool), "d, b")


# ---- 2. more groups than rows per vector, the tightest table; 3. the limit
N3, D3 = 3 * RG, 3000


@pytest.fixture(scope="module")
def many(fl, conn0):
    rng = np.random.default_rng(77)
    # 3,000 distinct keys; 36 of the 72 repeats are one key, whose run straddles row groups 0 | 1 once sorted
    k = np.concatenate([np.arange(D3), rng.integers(0, D3, 36), np.full(36, 1000)]) * 37 - 50000
    k = k[rng.permutation(N3)].astype(np.int32)
    x = rng.integers(-10**6, 10**6, N3).astype(np.int64)
    srt = np.sort(k)                                                                     # the same keys in runs
    img = fl.write_image([("k", fl.INT32, k, fl.ENC_AUTO), ("x", fl.INT64, x, fl.ENC_AUTO),
                          ("s", fl.INT32, srt, fl.ENC_AUTO)], rowgroup=RG)
    t = conn0.read_image(img)
    yield img, t, {0: k, 1: x, 2: srt}
    t.close()


MANY_AGGS = [("count",), ("sum", 1), ("min", 1), ("max", 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("max_groups", [4096, D3], ids=["roomy", "tightest"])
def test_gpu_more_groups_than_rows_per_vector(fl, gpu, many, max_groups):
    img, t, cols = many
    every = np.ones(N3, bool)
    assert len(np.unique(cols[0])) == D3
    for key in (0, 2):   # scattered keys, and the same keys sorted: runs of equal keys in adjacent lanes
        h = t.aggregate_hashed([key], MANY_AGGS, max_groups)
        assert len(h) == D3
        check_hashed(h, cols, {}, [key], MANY_AGGS, every, what=f"key {key}, max_groups {max_groups}")
    # the next power of two >= 2 * max_groups slots -- 8,192 for 4,096 and for the distinct count itself, the
    # smallest table that holds these keys -- of ten fields (the key, the first row, count(*), the sum's
    # count / lo / hi, count and lo of MIN and of MAX) after a 16-word header
    assert h.table_bytes == (16 + 8192 * 10) * 8


@pytest.mark.gpu
def test_gpu_limit_is_an_error_and_the_table_stays_usable(fl, gpu, many):
    img, t, cols = many
    with pytest.raises(fl.FlsError) as e:
        t.aggregate_hashed([0], MANY_AGGS, D3 - 1)
    assert e.value.code == ERR_LIMIT and "max_groups" in e.value.msg and str(D3 - 1) in e.value.msg, e.value
    check_hashed(t.aggregate_hashed([0], MANY_AGGS, D3), cols, {}, [0], MANY_AGGS, np.ones(N3, bool), what="after")
    assert t.aggregate([("count",), ("sum", 1)]) == [N3, int(cols[1].sum())]
    # the limit counts selected rows' keys only
    filt = [(0, "<", 0)]
    sel = filter_mask(cols, filt, N3)
    d = len(np.unique(cols[0][sel]))
    assert 0 < d < D3 - 1
    check_hashed(t.aggregate_hashed([0], MANY_AGGS, d, filt=filt), cols, {}, [0], MANY_AGGS, sel, what="filtered")
    with pytest.raises(fl.FlsError) as e:
        t.aggregate_hashed([0], MANY_AGGS, d - 1, filt=filt)
    assert e.value.code == ERR_LIMIT, e.value


# ---- 4. one key over every vector, row group and batch; 5. 128-bit carries; 6. MIN / MAX
@pytest.fixture(scope="module")
def wide(fl, conn0):
    rng = np.random.default_rng(4242)
    n = N1
    i = np.arange(n)
    one = np.full(n, 7, dtype=np.int8)
    sgn = (i * 2654435761 % 3).astype(np.int8)                 # 0: near +2^62, 1: near -2^62, 2: both
    r = rng.integers(0, 1 << 40, n)
    pos, neg = np.int64(2**62) + r, np.int64(-2**62) - r
    v62 = np.where(sgn == 0, pos, np.where(sgn == 1, neg, np.where(i % 2 == 0, pos, neg))).astype(np.int64)
    u64 = np.uint64(2**64 - 1) - rng.integers(0, 1 << 30, n).astype(np.uint64)
    a = rng.integers(-2**31, 2**31, n).astype(np.int32)
    b = rng.integers(-2**63, 2**63, n, dtype=np.int64)
    c = rng.integers(0, 11, n).astype(np.int8)
    pool = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e300, 1.5, -1.5])
    g = pool[rng.integers(0, len(pool), n)]
    z = np.array([0.0, -0.0])[rng.integers(0, 2, n)]
    f = np.round(rng.normal(0, 10, n), 2).astype(np.float32)
    few = (i * 2654435761 % 5).astype(np.int8)
    nv = few != 3                                              # the operand is NULL on every row of group 3
    img = fl.write_image([("one", fl.INT8, one, fl.ENC_AUTO), ("sgn", fl.INT8, sgn, fl.ENC_AUTO),
                          ("v62", fl.INT64, v62, fl.ENC_AUTO), ("u64", fl.UINT64, u64, fl.ENC_AUTO),
                          ("a", fl.INT32, a, fl.ENC_AUTO), ("b", fl.INT64, b, fl.ENC_AUTO),
                          ("c", fl.INT8, c, fl.ENC_AUTO), ("g", fl.DOUBLE, g, fl.ENC_AUTO),
                          ("z", fl.DOUBLE, z, fl.ENC_AUTO), ("f", fl.FLOAT, f, fl.ENC_AUTO),
                          ("few", fl.INT8, few, fl.ENC_AUTO),
                          ("nx", fl.INT32, np.ma.array(a, mask=~nv), fl.ENC_AUTO),
                          ("ng", fl.DOUBLE, np.ma.array(g, mask=~nv), fl.ENC_AUTO)], rowgroup=RG)
    t = conn0.read_image(img)
    cols = {0: one, 1: sgn, 2: v62, 3: u64, 4: a, 5: b, 6: c, 7: g, 8: z, 9: f, 10: few, 11: a, 12: g}
    yield img, t, cols, {11: nv, 12: nv}
    t.close()


EXPR3 = [(0, 1, 4), (100, -1, 6), (-7, 1, 5)]       # a * (100 - c) * (b - 7): past 2^96 per row
CARRY_AGGS = [("count",), ("sum", 2), ("sum", 3), ("sum_product", 4, 5), ("sum_expr", EXPR3), ("min", 2), ("max", 3)]
ONE_AGGS = CARRY_AGGS + [("min", 7), ("max", 7), ("min", 8), ("max", 9), ("min", 9), ("count", 11), ("max", 5)]


@pytest.mark.gpu
def test_gpu_one_key_over_every_batch_equals_the_ungrouped_call(fl, gpu, wide, monkeypatch):
    img, t, cols, valid = wide
    monkeypatch.setenv("FLS_SCAN_BATCH", "1")      # five batches, two slots' streams into one slot of the table
    for filt in (None, [(4, "<", 0)], [(7, "<", 1e300), (7, ">", -1e300)]):
        plain = t.aggregate(ONE_AGGS, filt=filt)
        h = t.aggregate_hashed([0], ONE_AGGS, 1, filt=filt)
        got = h.to_list()
        assert len(got) == 1 and got[0][0] == (7,)
        assert as_bits(got)[0][1] == as_bits([((7,), plain)])[0][1], filt
        sel = filter_mask(cols, filt, N1) if filt else np.ones(N1, bool)
        assert int(h.first_row[0]) == int(np.nonzero(sel)[0][0])
    assert abs(plain[1]) > 0 and t.aggregate(ONE_AGGS)[2] > 2**64


@pytest.mark.gpu
def test_gpu_sums_carry_into_the_high_word(fl, gpu, wide):
    img, t, cols, valid = wide
    every = np.ones(N1, bool)
    h = t.aggregate_hashed([1], CARRY_AGGS, 8)
    check_hashed(h, cols, valid, [1], CARRY_AGGS, every, what="sgn")
    got = dict(h.to_list())
    # ~1,400 rows a group: the sums pass 2^64 upwards and downwards, and cancel to a small value in group 2
    assert got[(0,)][1] > 2**70 and got[(1,)][1] < -2**70 and abs(got[(2,)][1]) < 2**64
    assert all(v[2] > 2**73 for v in got.values())               # the UINT64 sum
    assert any(abs(v[4]) > 2**100 for v in got.values())          # the three-factor product sum
    check_groups(t.aggregate_hashed([1], CARRY_AGGS[:4], 8).to_list(), [1], CARRY_AGGS[:4], cols, valid, every, "sgn")


MINMAX_AGGS = [("min", 2), ("max", 2), ("min", 3), ("max", 3), ("min", 4), ("max", 4), ("min", 7), ("max", 7),
               ("min", 8), ("max", 8), ("min", 9), ("max", 9), ("min", 11), ("max", 12), ("count", 11), ("count", 12),
               ("sum", 11), ("count",)]


@pytest.mark.gpu
def test_gpu_min_max_of_integers_and_floats(fl, gpu, wide):
    img, t, cols, valid = wide
    for filt in (None, [(4, ">", 0)]):
        sel = filter_mask(cols, filt, N1) if filt else np.ones(N1, bool)
        got = t.aggregate_hashed([10], MINMAX_AGGS, 5, filt=filt).to_list()
        # check_groups compares FLOAT / DOUBLE MIN / MAX with same_float: NaN above every number, -0 == 0
        check_groups(got, [10], MINMAX_AGGS, cols, valid, sel, f"few under {filt}")
        by = dict(got)
        # the operand is NULL on every row of group 3: None, with count 0
        assert by[(3,)][12:17] == [None, None, 0, 0, None] and by[(3,)][17] > 0
        assert all(by[(k,)][12] is not None and by[(k,)][14] > 0 for k in (0, 1, 2, 4))
    assert any(same_float(v[7], float("nan")) for v in by.values())


# ---- 7. rows that make no group, and first rows
@pytest.mark.gpu
def test_gpu_filtered_out_and_tail_rows_make_no_group(fl, gpu, conn0):
    rng = np.random.default_rng(5)
    n = N1
    f = rng.integers(0, 2, n).astype(np.int8)
    k = np.where(f == 1, rng.integers(1, 400, n), rng.integers(1000, 1400, n)).astype(np.int32)  # >= 1000 only where the filter fails
    kv = rng.random(n) >= 0.1                                          # NULL keys: the placeholder 0 is no key value
    x = rng.integers(-100, 100, n).astype(np.int64)
    img = fl.write_image([("k", fl.INT32, np.ma.array(k, mask=~kv), fl.ENC_AUTO), ("f", fl.INT8, f, fl.ENC_AUTO),
                          ("x", fl.INT64, x, fl.ENC_AUTO)], rowgroup=RG)
    t = conn0.read_image(img)
    cols, valid = {0: k, 1: f, 2: x}, {0: kv}
    aggs = [("count",), ("sum", 2), ("count", 0)]
    try:
        filt = [(1, "=", 1)]
        sel = filter_mask(cols, filt, n)
        h = t.aggregate_hashed([0], aggs, 1024, filt=filt)
        check_hashed(h, cols, valid, [0], aggs, sel, what="k where f = 1")
        keys = {key[0] for key, _ in h.to_list()}
        assert None in keys and 0 not in keys and all(key is None or key < 400 for key in keys)
        # unfiltered: the keys >= 1000 are groups, the placeholder 0 is not, and the 37-row tail adds no row
        h = t.aggregate_hashed([0], aggs, 1024)
        check_hashed(h, cols, valid, [0], aggs, np.ones(n, bool), what="k")
        assert int(h.count[0].sum()) == n and 0 not in {key[0] for key, _ in h.to_list()}
        # the last row group alone: 37 rows, first rows are indices into the table, not into the range
        for r0, r1 in ((4, 5), (2, 5), (1, 3)):
            rows = np.zeros(n, bool)
            rows[r0 * RG:min(n, r1 * RG)] = True
            h = t.aggregate_hashed([0], aggs, 1024, filt=filt, rg_begin=r0, rg_end=r1)
            check_hashed(h, cols, valid, [0], aggs, rows & sel, what=f"k, row groups [{r0},{r1})")
            assert int(h.first_row.min()) >= r0 * RG and int(h.count[0].sum()) == int((rows & sel).sum())
        assert int(t.aggregate_hashed([0], aggs, 64, rg_begin=4, rg_end=5).count[0].sum()) == 37
    finally:
        t.close()


# ---- 8. equality with the grouped call
LINE_AGGS = [("sum", C_QTY), ("sum", C_PRICE), ("sum_product", C_PRICE, C_DISC), ("sum", C_DISC), ("count",),
             ("min", C_SHIPDATE), ("max", C_SHIPDATE), ("count", C_MODE),
             ("sum_expr", [(0, 1, C_PRICE), (100, -1, C_DISC)])]
SF, WL = 0.01, "lineitem"


@pytest.fixture(scope="module")
def lineitem(fl, conn0):
    t = conn0.read_image(fl.gen_image(WL, SF))
    cols = {c: fl.gen_values(WL, c, 0, t.nrows, fl.NP_DTYPE[ty], SF)
            for c, (name, ty, _, _, _) in enumerate(t.schema()) if ty != fl.VARCHAR}
    yield t, cols
    t.close()


@pytest.mark.gpu
def test_gpu_equals_the_grouped_call_where_both_accept(fl, gpu, lineitem, conn0):
    """Q6's terms select 879 distinct (l_linenumber, l_shipdate) pairs in the
    generated image's single 60,175-row row group, past the grouped call's 256
    per row group; so the two-key comparison also runs on the same rows
    rewritten with 4,096-row row groups, which the grouped call accepts, and
    the hashed results of the two images must agree with it and each other."""
    t, cols = lineitem
    one = t.aggregate_hashed([C_LINE], LINE_AGGS, 16, filt=Q6).to_list()
    assert one == t.aggregate_grouped([C_LINE], LINE_AGGS, filt=Q6) and len(one) == 7
    assert t.aggregate_hashed([C_LINE], LINE_AGGS, 7).to_list() == t.aggregate_grouped([C_LINE], LINE_AGGS)
    spec = [(name, ty, cols.get(c, ["x"] * t.nrows), fl.ENC_DICT if ty == fl.VARCHAR else fl.ENC_AUTO) +
            ((width, scale) if ty == fl.DECIMAL else ()) for c, (name, ty, width, scale, _) in enumerate(t.schema())]
    t2 = conn0.read_image(fl.write_image(spec, rowgroup=4096))
    try:
        keys = [C_LINE, C_SHIPDATE]
        two = t2.aggregate_hashed(keys, LINE_AGGS, 2048, filt=Q6).to_list()
        assert two == t2.aggregate_grouped(keys, LINE_AGGS, filt=Q6) and len(two) > 256
        assert t.aggregate_hashed(keys, LINE_AGGS, 2048, filt=Q6).to_list() == two
        assert t2.aggregate_hashed([C_LINE], LINE_AGGS, 16, filt=Q6).to_list() == one
    finally:
        t2.close()
    sel = filter_mask(cols, Q6, t.nrows)
    assert len(two) == len(groups_of([cols[C_LINE], cols[C_SHIPDATE]], [None, None], sel))


# ---- 9. reproducibility
def canon(h):
    """the groups as a sorted set of (key, first row, value bits) and as the ordered list"""
    rows = as_bits(h.to_list(ordered=False))
    return sorted(((k, int(f), v) for (k, v), f in zip(rows, h.first_row.tolist())), key=repr), as_bits(h.to_list())


@pytest.mark.gpu
def test_gpu_results_are_identical_across_batches_and_pipelines(fl, gpu, nullkeys, many, wide, monkeypatch):
    nimg, tn, ncols, nvalid = nullkeys
    mimg, tm, mcols = many
    wimg, tw, wcols, wvalid = wide

    def run(tn, tm, tw, max_many=D3):   # (the batch size is read when a scan starts)
        return (canon(tn.aggregate_hashed([0, 1, 2, 3], NULL_AGGS, 4096)),
                canon(tm.aggregate_hashed([0], MANY_AGGS, max_many)),
                canon(tm.aggregate_hashed([2], MANY_AGGS, max_many, filt=[(1, ">", 0)])),
                canon(tw.aggregate_hashed([10], CARRY_AGGS + MINMAX_AGGS, 8)),
                canon(tw.aggregate_hashed([0], ONE_AGGS, 1)))

    monkeypatch.delenv("FLS_SCAN_BATCH", raising=False)
    base = run(tn, tm, tw)
    for batch in ("1", "3", "8"):
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)
        assert run(tn, tm, tw) == base, batch
    monkeypatch.setenv("FLS_SCAN_BATCH", "1")
    monkeypatch.setenv("FLS_SCAN_SLOTS", "4")       # four slots' streams insert into one table
    assert run(tn, tm, tw) == base, "batch 1, four slots"
    monkeypatch.delenv("FLS_SCAN_SLOTS")
    # the row groups sharded over two pipelines (the same GPU listed twice): the one key of `wide`, its
    # five and the sorted key of `many` whose run crosses the boundary are in both shards
    monkeypatch.setenv("FLS_SCAN_BATCH", "3")
    conn2 = fl.Connection([0, 0])
    tn2, tm2, tw2 = conn2.read_image(nimg), conn2.read_image(mimg), conn2.read_image(wimg)
    try:
        assert run(tn2, tm2, tw2) == base, "batch 3, two pipelines"
        monkeypatch.delenv("FLS_SCAN_BATCH")
        assert run(tn2, tm2, tw2) == base, "default batch, two pipelines"
        # the limit is a pipeline's: each shard's keys fit a max_groups the whole table's do not
        srt = mcols[2]
        d0, d1 = len(np.unique(srt[:RG])), len(np.unique(srt[RG:]))   # row group 0 | row groups 1 and 2
        assert srt[RG - 1] == srt[RG] and max(d0, d1) < D3 < d0 + d1
        part = canon(tm2.aggregate_hashed([2], MANY_AGGS, max(d0, d1)))
        assert part == canon(tm.aggregate_hashed([2], MANY_AGGS, D3)) and len(part[1]) == D3
        with pytest.raises(fl.FlsError) as e:
            tm.aggregate_hashed([2], MANY_AGGS, max(d0, d1))
        assert e.value.code == ERR_LIMIT, e.value
    finally:
        tn2.close()
        tm2.close()
        tw2.close()
        conn2.close()


# ---- 10. the Q18 shape
@pytest.mark.gpu
def test_gpu_group_by_orderkey(fl, gpu, lineitem, conn0):
    t, cols = lineitem
    okey, qty = cols[C_OKEY], cols[C_QTY].astype(np.int64)

    def expect(sel):
        keys, first, inv = np.unique(okey[sel], return_index=True, return_inverse=True)
        sums = [0] * len(keys)
        for g, q in zip(inv.tolist(), qty[sel].tolist()):
            sums[g] += q
        return keys, np.nonzero(sel)[0][first], sums, np.bincount(inv, minlength=len(keys))

    def check(h, sel):
        keys, first, sums, counts = expect(sel)
        assert len(h) == len(keys)
        o = np.argsort(h.key_values[0].view(np.int64))
        assert np.array_equal(h.key_values[0].view(np.int64)[o], keys) and not h.key_null[0].any()
        assert np.array_equal(h.first_row[o], first.astype(np.uint64))
        assert np.array_equal(h.count[1][o], counts.astype(np.uint64)) and np.array_equal(h.count[0], h.count[1])
        assert [(hi << 64 | lo) for lo, hi in zip(h.lo[0][o].tolist(), h.hi[0][o].tolist())] == sums
        assert (h.kind[0] == fl.AGGV_INT).all() and np.array_equal(h.lo[1], h.count[1])

    every = np.ones(t.nrows, bool)
    ndist = len(np.unique(okey))
    assert ndist > 15000
    aggs = [("sum", C_QTY), ("count",)]
    h = t.aggregate_hashed([C_OKEY], aggs, ndist)
    check(h, every)
    assert h.table_bytes == (16 + 32768 * 6) * 8
    # Q18's inner query is this GROUP BY; its outer one reads the orders the HAVING keeps through a key set
    keys, _, sums, _ = expect(every)
    big = keys[np.array(sums) > 25000]                  # sum(l_quantity) > 250
    assert 0 < len(big) < ndist
    ks = conn0.keyset(big, signed=True)
    try:
        filt = [(C_OKEY, "in_set", ks), (C_SHIPDATE, ">", 9000)]
        sel = np.isin(okey, big) & (cols[C_SHIPDATE] > 9000)
        check(t.aggregate_hashed([C_OKEY], aggs, len(big), filt=filt), sel)
    finally:
        ks.close()
