"""Mapped columns: map[key] as an aggregate operand, a
sum_expr factor and a hash GROUP BY key (fls_aggregate_value_bindings,
FLS_COL_MAPPED, fl.Mapped in aggs and keys).  The argument checks, the
overflow bounds, the key layout and the row-group pruning run without a GPU;
mapval_kernel runs on the GPU through fls_aggregate, fls_aggregate_grouped and
fls_aggregate_hashed[_select], against a Python dict and numpy written here
(never against the code under test).

Shapes as tests/test_valuemap.py: 4096-row row groups, N = 2 * 4096 + 1061
rows (the last row group one full vector plus a 37-row partial word), and a
`pick` column that empties one whole vector and several 64-row words before
the binding runs."""
import ctypes as C

import numpy as np
import pytest

from test_keyset import KEY_TYPES, colliding_keys, key_pool, type_range

RG = 4096
N = 2 * RG + 1061
M64 = (1 << 64) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ERR_ARG = -3
DENSE, HASH = 1, 2
COL_MAPPED = 0x40000000


# ---- the reference: a Python dict over the generated columns
def looked_up(key, d, ok=None):
    """(present, value) per row of the key column: the dict lookup at valid rows; values as Python ints"""
    present = np.zeros(len(key), bool)
    val = [0] * len(key)
    for i, k in enumerate(key.tolist()):
        if ok is not None and not ok[i]:
            continue
        b = d.get(int(k))
        if b is not None:
            present[i] = True
            val[i] = int(b)
    return present, val


def ev(kind, vals, ok, idx):
    """one aggregate over the rows idx: Python ints, exact"""
    if kind == "count*":
        return len(idx)
    rows = [i for i in idx.tolist() if ok is None or ok[i]]
    if kind == "count":
        return len(rows)
    if not rows:
        return None
    xs = [int(vals[i]) for i in rows]
    return {"sum": sum, "min": min, "max": max}[kind](xs)


def pick_column():
    """1 everywhere but one whole vector and several 64-row words"""
    pick = np.ones(N, np.int8)
    pick[1024:2048] = 0
    for w in (0, 3, 17, 64 + 5, 64 + 6, 128 + 15, 128 + 16):
        pick[64 * w:64 * w + 64] = 0
    pick[N - 37:] = 1
    pick[N - 37 + 5] = 0
    return pick


def key_groups(lo, hi, pool, rng, form):
    """the keys of the maps of one key type: about two thirds of the column's
    values (a third absent), some keys no row holds and the type's ends; a
    dense map spans at most 2^28 keys, so a wide type gets one map per cluster"""
    signed = lo < 0
    part = [v for v in pool if rng.random() < 0.66] or pool[:1]
    absent = [v for v in (lo + 5, hi - 5, 3, 1234) if lo <= v <= hi and v not in pool]
    edges = [lo, hi]
    if form == HASH or hi - lo < 1 << 28:
        return [part + absent + edges]
    return [[v for v in part + absent + edges if v - lo < 1 << 20], [v for v in part + absent + edges if hi - v < 1 << 20],
            [v for v in part + absent + [-1 if signed else 0] if abs(v) < 1 << 20]]


@pytest.fixture(scope="module")
def conn(fl):
    c = fl.Connection([0])
    yield c
    c.close()


def vmap(conn, d, signed=True, value_signed=True, form=0):
    return conn.valuemap(list(d), list(d.values()), signed=signed, value_signed=value_signed, form=form)


# ------------------------------------------------------------------ CPU tests
def test_library_exports_the_value_bindings(fl):
    assert hasattr(fl.lib, "fls_aggregate_value_bindings")
    assert C.sizeof(fl.ValueBinding) == 16
    assert (fl.ValueBinding.col.offset, fl.ValueBinding.flags.offset, fl.ValueBinding.map.offset) == (0, 4, 8)
    assert fl.COL_MAPPED == COL_MAPPED and fl.VALUEMAP_KEEP_UNMATCHED == 1
    a, b = fl.Mapped(3, None), fl.Mapped(3, None)
    assert a == b and hash(a) == hash(b) and a != fl.Mapped(3, None, keep_unmatched=True) and a != fl.Mapped(4, None)
    assert repr(fl.Mapped(3, None, keep_unmatched=True)) == "Mapped(3, None, keep_unmatched=True)"


# columns of `typed`
T_I64, T_U32, T_F, T_S, T_DEC38, T_BIG = range(6)


@pytest.fixture(scope="module")
def typed(fl, conn):
    n = 2048
    big = np.full(n, 1 << 54, np.int64)
    cols = [("i64", fl.INT64, np.arange(n, dtype=np.int64) % 50, fl.ENC_AUTO),
            ("u32", fl.UINT32, np.arange(n, dtype=np.uint32), fl.ENC_AUTO),
            ("f", fl.DOUBLE, np.arange(n, dtype=np.float64), fl.ENC_AUTO),
            ("s", fl.VARCHAR, [b"a", b"b"] * (n // 2), fl.ENC_DICT),
            ("d38", fl.DECIMAL, np.arange(n, dtype=np.int64), fl.ENC_AUTO, 38, 2),
            ("big", fl.INT64, big, fl.ENC_AUTO)]
    t = conn.read_image(fl.write_image(cols, rowgroup=1024))
    yield t
    t.set_aggregate_value_bindings(None)
    t.close()


def refused(fl, what, fn):
    with pytest.raises(fl.FlsError, match=what) as e:
        fn()
    assert e.value.code == ERR_ARG, e.value


def test_argument_errors_before_any_device_work(fl, conn, typed):
    t = typed
    vm, um = vmap(conn, {1: 5, 2: 6}), vmap(conn, {1: 5}, signed=False)
    km, ks = conn.keymap([1, 2, 3], [0, 1, 2]), conn.keyset([1, 2, 3])
    sb = t.set_aggregate_value_bindings
    refused(fl, r"value binding 1: column 99 out of range", lambda: sb([(T_I64, vm), (99, vm)]))
    refused(fl, r"value binding 0: .*VARCHAR / BLOB / FLOAT / DOUBLE", lambda: sb([(T_F, vm)]))
    refused(fl, r"value binding 0: .*VARCHAR / BLOB / FLOAT / DOUBLE", lambda: sb([(T_S, vm)]))
    refused(fl, r"value binding 0: .*DECIMAL wider than 64 bits", lambda: sb([(T_DEC38, vm)]))
    refused(fl, r"value binding 0: the value map's key kind is unsigned, column 0 is signed", lambda: sb([(T_I64, um)]))
    refused(fl, r"value binding 0: the value map's key kind is signed, column 1 is unsigned", lambda: sb([(T_U32, vm)]))
    for h in (ks.h, km.h, 0, 0xDEADBEEF):
        refused(fl, r"value binding 0: map 0x[0-9a-f]+ is not a live value map", lambda: sb([(T_I64, h)]))
    refused(fl, r"value binding 0: unknown flag bits 0x6", lambda: sb([(T_I64, vm, 7)]))
    refused(fl, r"5 bindings \(at most 4\)", lambda: sb([(T_I64, vm)] * 5))
    # FLS_COL_MAPPED | i with i at or past the bindings set
    sb([(T_I64, vm)])
    try:
        M1 = COL_MAPPED | 1
        for call in (lambda a: t.aggregate_raw(a), lambda a: t.aggregate_grouped([T_U32], a),
                     lambda a: t.aggregate_hashed([T_U32], a, 64)):
            refused(fl, r"aggregate 1: no value binding 1 \(1 set", lambda: call([("count",), ("sum", M1)]))
            refused(fl, r"aggregate 0: no value binding 1 \(1 set", lambda: call([("sum_product", T_I64, M1)]))
            refused(fl, r"aggregate 0: no value binding 1 \(1 set", lambda: call([("count", M1)]))
        refused(fl, r"expression 0: no value binding 1 \(1 set", lambda: t.set_aggregate_exprs([[(0, 1, M1)]]))
        refused(fl, r"key 1: no value binding 1 \(1 set", lambda: t.aggregate_hashed([T_U32, M1], [("count",)], 64))
        refused(fl, r"key 1: value binding 0 is key 0 already",
                lambda: t.aggregate_hashed([COL_MAPPED, COL_MAPPED], [("count",)], 64))
        # FLS_COL_MAPPED anywhere else
        refused(fl, r"key 0: a mapped column \(FLS_COL_MAPPED\) cannot be a grouped aggregate's key",
                lambda: t.aggregate_grouped([COL_MAPPED], [("count",)]))
        refused(fl, r"order key: a mapped column \(FLS_COL_MAPPED\) cannot be a top-N key", lambda: t.topn(COL_MAPPED, 3))
        refused(fl, r"a mapped column \(FLS_COL_MAPPED\) cannot be a filter term's column",
                lambda: t.set_filter([(COL_MAPPED, "<", 3)]))
        refused(fl, r"filter term 0: right column 1073741824 out of range",
                lambda: t.set_filter([(T_I64, "<", fl.Col(COL_MAPPED))]))
        refused(fl, r"filter term 0: key column 1073741824 out of range",
                lambda: t.set_filter([(T_I64, "<", fl.Mapped(COL_MAPPED, vm))]))
        refused(fl, r"condition 0, term 0: a mapped column \(FLS_COL_MAPPED\) cannot be a filter term's column",
                lambda: t.aggregate([fl.When(("count",), [(COL_MAPPED, "<", 3)])]))
        refused(fl, r"alternative 0, term 0: a mapped column \(FLS_COL_MAPPED\) cannot be a filter term's column",
                lambda: t.aggregate([("count",)], [fl.AnyOf([(COL_MAPPED, "<", 3)])]))
        refused(fl, r"column 1073741824 out of range", lambda: t.keyset(COL_MAPPED))   # (Table.keyset asks for the column first)
        out = C.c_void_p()
        assert fl.lib.fls_keyset_from_scan(t.h, COL_MAPPED, 0, t.nrowgroups, 0, C.byref(out), None) == ERR_ARG
        # a delivered column: the C call takes a byte per column (fls_scan_begin's col_mask), so the bit cannot be
        # said there; Python's column lists refuse it by name
        for cols in ([COL_MAPPED], [T_I64, fl.Mapped(T_I64, vm)]):
            with pytest.raises(ValueError, match="a mapped column cannot be delivered"):
                list(t.scan_filtered([(T_I64, "<", 3)], cols=cols))
            with pytest.raises(ValueError, match="a mapped column cannot be delivered"):
                t.topn(T_I64, 3, cols=cols)
    finally:
        sb(None)
        t.set_filter(None)
    # Python: where a Mapped means nothing
    with pytest.raises(ValueError, match="keep_unmatched"):
        t.set_filter([(T_I64, "<", fl.Mapped(T_I64, vm, keep_unmatched=True))])
    with pytest.raises(ValueError, match=r'\("map", col, keymap\)'):
        t.aggregate_grouped([fl.Mapped(T_I64, vm)], [("count",)])


def test_the_overflow_bounds_take_the_maps_value_range(fl, conn, typed):
    """2048 rows x 2^54 (column `big`) x 2^63 (the map's values) = 2^128: refused.  The bound is taken before the
    bindings prune, so maps whose keys no row holds show it without a GPU: refused with values near 2^63, accepted
    (then every row group pruned: NULL) with small ones or none"""
    t = typed
    huge, small = vmap(conn, {-5: I64_MAX - 5, -6: 3}), vmap(conn, {-5: 1000, -6: -1000})
    neg = vmap(conn, {-5: I64_MIN + 9, -6: 3})
    uhuge = vmap(conn, {-5: M64 - 1}, value_signed=False)
    empty = vmap(conn, {})
    for m, ok in ((huge, False), (neg, False), (uhuge, False), (small, True), (empty, True)):
        for aggs in ([("sum_product", T_BIG, fl.Mapped(T_I64, m))], [("sum_product", fl.Mapped(T_I64, m), T_BIG)],
                     [("sum_expr", [(0, 1, T_BIG), (7, -1, fl.Mapped(T_I64, m))])]):
            if ok:
                assert t.aggregate(aggs) == [None] and t.pruned == 2
                assert t.aggregate_hashed([T_U32], aggs, 64).to_list() == []
            else:
                refused(fl, r"aggregate 0: SUM_(PRODUCT|EXPR) .*may overflow 128 bits", lambda: t.aggregate(aggs))
                refused(fl, r"aggregate 0: SUM_(PRODUCT|EXPR) .*may overflow 128 bits",
                        lambda: t.aggregate_hashed([T_U32], aggs, 64))


def test_a_packed_hash_key_over_63_bits_is_refused(fl, conn, typed):
    t = typed
    wide = vmap(conn, {1: 0, 2: 1 << 62})                      # 63 value bits + NULL bit
    refused(fl, r"key 0: the packed key needs 64 bits",
            lambda: t.aggregate_hashed([fl.Mapped(T_I64, wide)], [("count",)], 64))
    span62 = vmap(conn, {1: -(1 << 61), 2: (1 << 61) - 1})     # 62 bits + NULL: fits alone
    assert t.aggregate_hashed([fl.Mapped(T_I64, span62)], [("count",)], 64, rg_begin=0, rg_end=0).to_list() == []
    refused(fl, r"key 0: the packed key needs 75 bits",          # 62 + 11 (u32: 0 .. 2047) + 2 NULL bits
            lambda: t.aggregate_hashed([fl.Mapped(T_I64, span62), T_U32], [("count",)], 64))
    # an empty map: 0 value bits plus the NULL bit, inner: no row group, no device work
    assert t.aggregate_hashed([fl.Mapped(T_I64, vmap(conn, {}))], [("count",)], 64).to_list() == []


NRG_P = 5


@pytest.fixture(scope="module")
def prunetab(fl, conn):
    """row groups of 1024 rows; key: sorted INT64, row group r in [1000 r, 1000 r + 900]; nkey: the same with NULLs
    and an all-NULL row group 2"""
    rng = np.random.default_rng(2)
    rows = 1024
    key = np.concatenate([np.sort(rng.integers(1000 * r, 1000 * r + 901, rows)) for r in range(NRG_P)]).astype(np.int64)
    null = rng.random(len(key)) < 0.1
    null[2 * rows:3 * rows] = True
    t = conn.read_image(fl.write_image([("key", fl.INT64, key, fl.ENC_AUTO),
                                        ("nkey", fl.INT64, np.ma.masked_array(key, mask=null), fl.ENC_AUTO)],
                                       rowgroup=rows))
    assert t.nrowgroups == NRG_P
    yield t, key
    t.close()


def test_host_pruning_of_inner_and_kept_bindings(fl, conn, prunetab):
    t, _ = prunetab
    miss = vmap(conn, {-3: 1, 901: 2, 99999: 3})               # no key in any row group's range
    for m in (miss, vmap(conn, {}), vmap(conn, {}, form=HASH)):
        M = fl.Mapped(0, m)
        assert t.aggregate([("count",), ("sum", M), ("min", M)]) == [0, None, None] and t.pruned == NRG_P
        assert t.aggregate_grouped([0], [("count", M)]) == [] and t.pruned == NRG_P
        assert t.aggregate_hashed([M], [("count",), ("sum", M)], 64).to_list() == [] and t.pruned == NRG_P
        assert t.aggregate_hashed([0], [("sum", M)], 64, order_by=(0, "desc"), limit=3).to_list() == []
    # the all-NULL key chunk and the row groups outside the key range go: the scan then needs a GPU, so read the
    # verdict through a range that holds only prunable row groups
    some = vmap(conn, {2500: 1, 4100: 2})                      # row groups 2 and 4
    assert t.aggregate([("count", fl.Mapped(0, some))], rg_begin=0, rg_end=2) == [0] and t.pruned == 2
    assert t.aggregate([("count", fl.Mapped(0, some))], rg_begin=3, rg_end=4) == [0] and t.pruned == 1
    assert t.aggregate([("count", fl.Mapped(1, some))], rg_begin=0, rg_end=4) == [0] and t.pruned == 4   # rg 2 all NULL


@pytest.mark.gpu
def test_gpu_pruning_counts_and_kept_bindings_prune_nothing(fl, gpu, conn, prunetab):
    t, key = prunetab
    k2, k4 = int(key[2 * 1024 + 500]), int(key[4 * 1024 + 500])    # a key of row group 2 and one of row group 4
    some = vmap(conn, {k2: 1, k4: 2})
    hits = int(np.isin(key, [k2, k4]).sum())
    assert t.aggregate([("count",), ("count", fl.Mapped(0, some))]) == [hits, hits] and t.pruned == 3
    kept = fl.Mapped(0, some, keep_unmatched=True)
    assert t.aggregate([("count",), ("count", kept)]) == [len(key), hits] and t.pruned == 0
    assert t.aggregate([("count",), ("sum", fl.Mapped(0, vmap(conn, {}), keep_unmatched=True))]) == [len(key), None]
    assert t.pruned == 0


# ------------------------------------------------------------------ GPU tests
C_PICK = len(KEY_TYPES)


@pytest.fixture(scope="module")
def typetab(fl, conn):
    """a key column of every type with NULLs, then pick"""
    rng = np.random.default_rng(21)
    specs, cols, ok, pools = [], {}, {}, {}
    for c, name in enumerate(KEY_TYPES):
        ty = getattr(fl, name)
        pool = key_pool(fl, name, rng)
        vals = np.array([pool[j] for j in rng.integers(0, len(pool), N)], dtype=object).astype(fl.NP_DTYPE[ty])
        null = rng.random(N) < 0.1
        specs.append((f"c{c}", ty, np.ma.masked_array(vals, mask=null), fl.ENC_FFOR, *((15, 2) if name == "DECIMAL" else ())))
        cols[c], ok[c], pools[c] = vals, ~null, pool
    cols[C_PICK] = pick_column()
    specs.append(("pick", fl.INT8, cols[C_PICK], fl.ENC_AUTO))
    t = conn.read_image(fl.write_image(specs, rowgroup=RG))
    assert t.nrowgroups == 3 and t.nrows == N
    yield t, cols, ok, pools
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", KEY_TYPES)
def test_gpu_operand_of_every_key_type_against_the_dict(fl, gpu, conn, typetab, name):
    t, cols, ok, pools = typetab
    k = KEY_TYPES.index(name)
    lo, hi = type_range(fl, name)
    sel = cols[C_PICK] == 1
    for form in (DENSE, HASH):
        rng = np.random.default_rng(k)
        seen = 0
        for keys in key_groups(lo, hi, pools[k], rng, form):
            d = {key: ((key * 7 + 3) % 1000) - 500 for key in keys}
            m = vmap(conn, d, signed=lo < 0, form=form)
            assert m.info.form == form
            present, val = looked_up(cols[k], d, ok[k])
            counts = {}
            for keep in (False, True):
                M = fl.Mapped(k, m, keep_unmatched=keep)
                got = t.aggregate([("count",), ("count", M), ("sum", M), ("min", M), ("max", M)], [(C_PICK, "=", 1)])
                idx = np.nonzero(sel if keep else sel & present)[0]
                want = [ev("count*", None, None, idx)] + [ev(f, val, present, idx) for f in ("count", "sum", "min", "max")]
                assert got == want, (name, form, keep)
                counts[keep] = got
            assert counts[False][0] < counts[True][0] and counts[False][1] == counts[True][1] > 0
            seen += counts[False][1]
            m.close()
        assert seen > 0


@pytest.mark.gpu
@pytest.mark.parametrize("form", [DENSE, HASH])
def test_gpu_value_extremes_are_exact(fl, gpu, conn, typetab, form):
    t, cols, ok, pools = typetab
    k = KEY_TYPES.index("INT16")
    pool = sorted(set(pools[k]))[:40]
    sel = cols[C_PICK] == 1
    sd = {key: (I64_MIN, I64_MAX, -1, 0, 1)[i % 5] for i, key in enumerate(pool)}
    ud = {key: (M64, 0, 1 << 63, M64 - 1)[i % 4] for i, key in enumerate(pool)}
    allmax = {key: I64_MAX for key in pool}
    for d, vs in ((sd, True), (ud, False), (allmax, True)):
        m = vmap(conn, d, value_signed=vs, form=form)
        present, val = looked_up(cols[k], d, ok[k])
        M = fl.Mapped(k, m)
        got = t.aggregate([("count",), ("sum", M), ("min", M), ("max", M)], [(C_PICK, "=", 1)])
        idx = np.nonzero(sel & present)[0]
        assert got == [len(idx), ev("sum", val, None, idx), ev("min", val, None, idx), ev("max", val, None, idx)]
        if d is allmax:
            assert len(idx) > 2000 and got[1] == len(idx) * I64_MAX > 1 << 74
        m.close()


# columns of `facttab`
F_OKEY, F_SUPP, F_GRP, F_PART, F_PRICE, F_DISC, F_QTY, F_PICK = range(8)


@pytest.fixture(scope="module")
def facttab(fl, conn):
    rng = np.random.default_rng(28)
    okey = np.sort(rng.integers(0, 1500, N)).astype(np.int64)
    supp = rng.integers(1, 40, N).astype(np.int32)
    grp = rng.integers(0, 5, N).astype(np.int8)
    part = rng.integers(0, 200, N).astype(np.int32)
    price = rng.integers(100, 10 ** 7, N).astype(np.int64)
    disc = rng.integers(0, 11, N).astype(np.int64)
    qty = rng.integers(1, 51, N).astype(np.int64)
    nq = rng.random(N) < 0.1
    pick = pick_column()
    A = fl.ENC_AUTO
    img = fl.write_image([("okey", fl.INT64, okey, A), ("supp", fl.INT32, supp, A), ("grp", fl.INT8, grp, A),
                          ("part", fl.INT32, part, A), ("price", fl.DECIMAL, price, A, 15, 2),
                          ("disc", fl.DECIMAL, disc, A, 15, 2),
                          ("qty", fl.DECIMAL, np.ma.masked_array(qty, mask=nq), A, 15, 2), ("pick", fl.INT8, pick, A)],
                         rowgroup=RG)
    t = conn.read_image(img)
    cols = {F_OKEY: okey, F_SUPP: supp, F_GRP: grp, F_PART: part, F_PRICE: price, F_DISC: disc,
            F_QTY: np.where(nq, 0, qty).astype(np.int64), F_PICK: pick}
    yield t, cols, ~nq, img
    t.close()


def cost_dict():
    return {p: 900 + (p * 37) % 5000 for p in range(200) if p % 3}          # a third of the parts absent


@pytest.mark.gpu
@pytest.mark.parametrize("form", [DENSE, HASH])
def test_gpu_products_and_the_q9_identity(fl, gpu, conn, facttab, form):
    t, cols, qok, _ = facttab
    d = cost_dict()
    m = vmap(conn, d, form=form)
    present, cost = looked_up(cols[F_PART], d)
    cost = np.array(cost, dtype=object)
    qty, price, disc = (cols[c].astype(object) for c in (F_QTY, F_PRICE, F_DISC))
    sel = cols[F_PICK] == 1
    for keep in (False, True):
        M = fl.Mapped(F_PART, m, keep_unmatched=keep)
        aggs = [("sum_product", F_QTY, M), ("sum_product", M, F_QTY),
                ("sum_expr", [(5, -1, M)]),
                ("sum_expr", [(0, 1, F_QTY), (-3, 1, M)]),
                ("sum_expr", [(100, -1, F_DISC), (0, 1, M), (7, -1, F_QTY)]),
                ("sum_expr", [(0, 1, F_PRICE), (100, -1, F_DISC)]), ("count",)]
        got = t.aggregate(aggs, [(F_PICK, "=", 1)])
        rows = sel if keep else sel & present
        both = rows & present & qok
        want = [int((qty * cost)[both].sum()), int((qty * cost)[both].sum()), int((5 - cost)[rows & present].sum()),
                int((qty * (cost - 3))[both].sum()), int(((100 - disc) * cost * (7 - qty))[both].sum()),
                int((price * (100 - disc))[rows].sum()), int(rows.sum())]
        assert got == want, (form, keep)
        # Q9 on the fact table: sum(price * (100 - disc)) - 100 * sum(cost[part] * qty), both sides over the joined rows
        if not keep:
            assert got[5] - 100 * got[0] == int((price * (100 - disc))[rows].sum()) - 100 * int((qty * cost)[both].sum())
    m.close()


def ref_groups(keycols, rows, aggs):
    """{key tuple: [values]} over the rows; keycols: (values, ok) per key (None for a NULL key);
    aggs: (kind, vals, ok)"""
    buckets = {}
    for i in np.nonzero(rows)[0].tolist():
        key = tuple(None if (okk is not None and not okk[i]) else int(v[i]) for v, okk in keycols)
        buckets.setdefault(key, []).append(i)
    return {k: [ev(kind, vals, okk, np.array(ix)) for kind, vals, okk in aggs] for k, ix in buckets.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [False, True])
def test_gpu_all_three_calls_under_a_combined_filter(fl, gpu, conn, facttab, keep):
    t, cols, qok, _ = facttab
    d = cost_dict()
    m = vmap(conn, d, form=HASH)
    dated = {int(k): 9 + (int(k) * 7) % 30 for k in np.unique(cols[F_OKEY]) if k % 4}
    other = vmap(conn, dated, form=DENSE)
    ks = conn.keyset([s for s in range(1, 40) if s % 5])
    M = fl.Mapped(F_PART, m, keep_unmatched=keep)
    filt = [(F_PICK, "=", 1), (F_SUPP, "in_set", ks), (F_QTY, "<", fl.Mapped(F_OKEY, other)),
            fl.AnyOf([(F_GRP, "<", 2)], [(F_DISC, ">=", 8)])]
    aggs = [("count",), ("count", M), ("sum", M), ("min", M), ("max", M), ("sum_product", F_QTY, M),
            fl.When(("sum", M), [(F_DISC, "<", 5)])]
    present, cost = looked_up(cols[F_PART], d)
    p2, dval = looked_up(cols[F_OKEY], dated)
    sel = ((cols[F_PICK] == 1) & (cols[F_SUPP] % 5 != 0) & qok & p2 & (cols[F_QTY] < np.array(dval)) &
           ((cols[F_GRP] < 2) | (cols[F_DISC] >= 8)))
    rows = sel if keep else sel & present
    prod = (cols[F_QTY].astype(object) * np.array(cost, dtype=object)).tolist()
    ref = [("count*", None, None), ("count", cost, present), ("sum", cost, present), ("min", cost, present),
           ("max", cost, present), ("sum", prod, present & qok), ("sum", cost, present & (cols[F_DISC] < 5))]
    assert 500 < rows.sum() < sel.sum() + 1
    idx = np.nonzero(rows)[0]
    assert t.aggregate(aggs, filt) == [ev(k_, v, o, idx) for k_, v, o in ref]
    got = dict(t.aggregate_grouped([F_GRP], aggs, filt))
    assert got == ref_groups([(cols[F_GRP], None)], rows, ref)
    got = dict(t.aggregate_hashed([F_SUPP], aggs, 64, filt=filt).to_list())
    assert got == ref_groups([(cols[F_SUPP], None)], rows, ref)
    m.close()
    other.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [DENSE, HASH])
def test_gpu_mapped_hash_keys(fl, gpu, conn, facttab, form):
    t, cols, qok, _ = facttab
    okeys = [int(k) for k in np.unique(cols[F_OKEY])]
    cd = {k: 100000 + (k * 11) % 307 for k in okeys if k % 3}                # about 300 customers, a third of the orders absent
    cust = vmap(conn, cd, form=form)
    present, cval = looked_up(cols[F_OKEY], cd)
    d = cost_dict()
    cost_m = vmap(conn, d)
    pc, cost = looked_up(cols[F_PART], d)
    sel = cols[F_PICK] == 1
    filt = [(F_PICK, "=", 1)]
    ref = [("count*", None, None), ("sum", cols[F_PRICE].tolist(), None), ("count", None, qok)]
    aggs = [("count",), ("sum", F_PRICE), ("count", F_QTY)]
    # one mapped key, inner and kept
    for keep in (False, True):
        K = fl.Mapped(F_OKEY, cust, keep_unmatched=keep)
        h = t.aggregate_hashed([K], aggs, 1024, filt=filt)
        assert h.key_signed == [True]
        want = ref_groups([(cval, present)], sel if keep else sel & present, ref)
        assert dict(h.to_list()) == want and len(want) > 250
        assert ((None,) in want) == keep
        if keep:
            assert want[(None,)][0] == int((sel & ~present).sum()) > 0
    # a mapped key and a plain one
    K = fl.Mapped(F_OKEY, cust)
    h = t.aggregate_hashed([K, F_GRP], aggs, 4096, filt=filt)
    assert dict(h.to_list()) == ref_groups([(cval, present), (cols[F_GRP], None)], sel & present, ref)
    # two mapped keys over one key column and two maps, one inner, one kept
    sd = {k: k % 7 for k in okeys if k % 2}
    seg = vmap(conn, sd, value_signed=False, form=form)
    ps, sval = looked_up(cols[F_OKEY], sd)
    h = t.aggregate_hashed([K, fl.Mapped(F_OKEY, seg, keep_unmatched=True)], aggs, 4096, filt=filt)
    assert h.key_signed == [True, False]
    want = ref_groups([(cval, present), (sval, ps)], sel & present, ref)
    assert dict(h.to_list()) == want and any(k[1] is None for k in want)
    # having and order_by ... limit over a sum with a mapped operand, grouped by a mapped key
    CM = fl.Mapped(F_PART, cost_m)
    rows = sel & present & pc
    groups = ref_groups([(cval, present)], rows, [("sum", cost, None), ("count*", None, None)])
    firsts = {}
    for i in np.nonzero(rows)[0].tolist():
        firsts.setdefault((cval[i],), i)
    thr = sorted(v[0] for v in groups.values())[len(groups) // 2]
    h = t.aggregate_hashed([K], [("sum", CM), ("count",)], 1024, filt=filt, having=[(0, ">", thr)])
    assert dict(h.to_list()) == {k: v for k, v in groups.items() if v[0] > thr} and 0 < len(h) < len(groups)
    h = t.aggregate_hashed([K], [("sum", CM), ("count",)], 1024, filt=filt, order_by=(0, "desc"), limit=7)
    best = sorted(groups.items(), key=lambda kv: (-kv[1][0], firsts[kv[0]]))[:7]
    assert h.to_list() == [(k, v) for k, v in best]
    # the identity map on the key column: the groups of the plain-key call exactly
    ident = vmap(conn, {k: k for k in okeys}, form=form)
    a = t.aggregate_hashed([fl.Mapped(F_OKEY, ident)], aggs, 2048, filt=filt)
    b = t.aggregate_hashed([F_OKEY], aggs, 2048, filt=filt)
    assert a.to_list() == b.to_list() and len(b) > 1000
    oa, ob = np.argsort(a.first_row), np.argsort(b.first_row)
    assert np.array_equal(a.first_row[oa], b.first_row[ob]) and np.array_equal(a.key_values[0][oa], b.key_values[0][ob])
    for x in (cust, cost_m, seg, ident):
        x.close()


@pytest.mark.gpu
@pytest.mark.parametrize("home", [5, 127])
def test_gpu_colliding_keys_at_max_probe(fl, gpu, conn, home):
    keys = colliding_keys(50, 7, home)
    others = colliding_keys(90, 7, home)[50:]
    rng = np.random.default_rng(51)
    pool = np.array(keys + others + [0, M64], dtype=np.uint64)
    kcol = pool[rng.integers(0, len(pool), N)]
    d = {key: M64 - j for j, key in enumerate(keys)}
    m = vmap(conn, d, signed=False, value_signed=False, form=HASH)
    assert m.info.max_probe == 50
    t = conn.read_image(fl.write_image([("k", fl.UINT64, kcol, fl.ENC_AUTO)], rowgroup=RG))
    try:
        present, val = looked_up(kcol, d)
        idx = np.nonzero(present)[0]
        M = fl.Mapped(0, m)
        assert t.aggregate([("count",), ("sum", M), ("min", M), ("max", M)]) == \
            [len(idx), ev("sum", val, None, idx), ev("min", val, None, idx), ev("max", val, None, idx)]
        h = t.aggregate_hashed([M], [("count",)], 128)
        assert h.key_signed == [False]
        assert dict(h.to_list()) == ref_groups([(val, present)], present, [("count*", None, None)])
    finally:
        t.close()
        m.close()


@pytest.mark.gpu
def test_gpu_results_identical_across_batches_slots_and_pipelines(fl, gpu, conn, facttab, monkeypatch):
    t, cols, qok, img = facttab
    monkeypatch.delenv("FLS_SCAN_BATCH", raising=False)
    monkeypatch.delenv("FLS_SCAN_SLOTS", raising=False)
    d = cost_dict()
    okeys = [int(k) for k in np.unique(cols[F_OKEY])]
    cd = {k: 100000 + (k * 11) % 307 for k in okeys if k % 3}

    def run(c, tab):   # (the maps belong to the table's connection)
        M = fl.Mapped(F_PART, vmap(c, d, form=HASH), keep_unmatched=True)
        K = fl.Mapped(F_OKEY, vmap(c, cd, form=DENSE))
        aggs = [("count",), ("sum", M), ("sum_product", F_QTY, M), fl.When(("max", M), [(F_DISC, "<", 5)])]
        filt = [(F_PICK, "=", 1)]
        return (tab.aggregate(aggs, filt), tab.aggregate_grouped([F_GRP], aggs, filt),
                tab.aggregate_hashed([K], aggs, 1024, filt=filt).to_list())

    base = run(conn, t)
    present, cost = looked_up(cols[F_PART], d)
    sel = cols[F_PICK] == 1
    assert base[0][:2] == [int(sel.sum()), ev("sum", cost, present, np.nonzero(sel)[0])]
    for batch, slots in (("1", "1"), ("1", "2"), ("2", "3")):
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)
        monkeypatch.setenv("FLS_SCAN_SLOTS", slots)
        assert run(conn, t) == base, (batch, slots)
    monkeypatch.delenv("FLS_SCAN_SLOTS")
    monkeypatch.setenv("FLS_SCAN_BATCH", "1")
    two = fl.Connection([0, 0])                                 # two scan pipelines on one device
    try:
        tm = two.read_image(img)
        assert run(two, tm) == base
        tm.close()
    finally:
        two.close()


@pytest.mark.gpu
def test_gpu_lifetime_and_unused_bindings(fl, gpu, conn, facttab):
    t, cols, qok, _ = facttab
    d = cost_dict()
    m = vmap(conn, d)
    present, cost = looked_up(cols[F_PART], d)
    plain = [("count",), ("sum", F_PRICE)]
    before = (t.aggregate(plain), t.pruned, t.aggregate_grouped([F_GRP], plain), t.aggregate_hashed([F_SUPP], plain, 64).to_list())
    # set, then the handle freed, then the call: the binding holds a reference
    t.set_aggregate_value_bindings([(F_PART, m), (F_OKEY, vmap(conn, {}))])   # (an unused empty inner map prunes nothing)
    try:
        h = m.h
        m.close()
        with pytest.raises(fl.FlsError, match="value binding 0: map 0x[0-9a-f]+ is not a live value map") as e:
            t.set_aggregate_value_bindings([(F_PART, h)])
        assert e.value.code == ERR_ARG
        got = [fl._agg_value(v) for v in t.aggregate_raw([("count",), ("sum", COL_MAPPED | 0)])]
        idx = np.nonzero(present)[0]
        assert got == [len(idx), ev("sum", cost, None, idx)]
        # with bindings set, a call that names none of them is what it was
        after = (t.aggregate(plain), t.pruned, t.aggregate_grouped([F_GRP], plain),
                 t.aggregate_hashed([F_SUPP], plain, 64).to_list())
        assert after == before and before[0][0] == N and before[1] == 0
    finally:
        t.set_aggregate_value_bindings(None)


L_ORDERKEY, L_PRICE, L_DISC, L_RFLAG = 0, 5, 6, 8


@pytest.mark.gpu
def test_gpu_lineitem_q10_shape(fl, gpu, conn):
    """TPC-H Q10's shape on generated lineitem at SF 0.01: GROUP BY
    cust[l_orderkey] of revenue and count under l_returnflag = 'R', top 20 by
    revenue; the customer of an order is synthesised by an injective-per-order
    rule, and the check is numpy's top 20 with ties resolved by first row"""
    wl, sf = "lineitem", 0.01
    t = conn.read_image(fl.gen_image(wl, sf))
    try:
        n = t.nrows
        okey = fl.gen_values(wl, L_ORDERKEY, 0, n, np.int64, sf)
        price = fl.gen_values(wl, L_PRICE, 0, n, np.int64, sf)
        disc = fl.gen_values(wl, L_DISC, 0, n, np.int64, sf)
        cd = {int(k): 1 + (int(k) * 2654435761 % 1500) for k in np.unique(okey) if k % 10}   # a tenth of the orders unknown
        cust = vmap(conn, cd)
        filt = [(L_RFLAG, "=", "R")]
        ret = np.zeros(n, bool)                                 # the rows of the (long-tested) string filter itself
        for _, first, sel, _ in t.scan_filtered(filt, cols=[L_ORDERKEY]):
            ret[sel.astype(np.int64) + first] = True
        present, cval = looked_up(okey, cd)
        rows = ret & present
        rev = (price.astype(object) * (100 - disc.astype(object))).tolist()
        groups = ref_groups([(cval, present)], rows, [("sum", rev, None), ("count*", None, None)])
        firsts = {}
        for i in np.nonzero(rows)[0].tolist():
            firsts.setdefault((cval[i],), i)
        best = sorted(groups.items(), key=lambda kv: (-kv[1][0], firsts[kv[0]]))[:20]
        h = t.aggregate_hashed([fl.Mapped(L_ORDERKEY, cust)],
                               [("sum_expr", [(0, 1, L_PRICE), (100, -1, L_DISC)]), ("count",)], 4096, filt=filt,
                               order_by=(0, "desc"), limit=20)
        assert h.to_list() == [(k, v) for k, v in best] and len(groups) > 500 and 0 < rows.sum() < ret.sum()
        assert h.groups_total == len(groups)
    finally:
        t.close()
