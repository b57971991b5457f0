"""Top-N pushdown (fls_topn / Table.topn): ORDER BY key
[DESC] LIMIT k selected on the GPU.  Expected values come from the inputs
alone: the total order -- NULL rank, then the key with every NaN above +inf
and -0 equal to +0, then the global row -- is restated in numpy (np.lexsort
and a slice) over the arrays handed to write_image or the seeded generators,
under helpers.filter_mask's selection.  Row indices compare exactly, delivered
values exactly where valid, float keys by bits.

CPU: the export, every argument error (raised before any device work: this
host has no GPU), the empty results, the host-side zone-map pruning counts and
the kernels' resources.  GPU: every key type in both directions, ties, NULL
placement, filters, delivered columns, determinism over batch sizes and
pipelines, MIN / MAX consistency and lineitem."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import filter_mask, fsst_text, rand64, special_doubles

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "duckdb-fastlane_amd" / "libflsgpu.so"

ERR_ARG, ERR_LIMIT = -3, -8
RG = 1024
N_T = 5 * 1024 + 333      # five whole vectors and a partial tail
KS = (1, 63, 64, 65, 1024)


# ---- the total order, restated
def expected_order(vals, valid, sel, k, desc=False, nulls_first=False):
    """indices of the k best selected rows of vals (numpy column) by
    (NULL rank, key, row); valid: bool per row or None"""
    n = len(vals)
    rows = np.arange(n)
    ok = np.ones(n, bool) if valid is None else valid
    null_rank = np.where(ok, 1, 0) if nulls_first else np.where(ok, 0, 1)
    if vals.dtype.kind == "f":
        v = vals.astype(np.float64)
        nan = np.isnan(v) & ok
        v = np.where(nan | ~ok, 0.0, v) + 0.0          # -0 + 0 = +0: one zero
        nan_rank = np.where(nan, 1, 0)
        if desc:
            v, nan_rank = -v, 1 - nan_rank
        nan_rank = np.where(ok, nan_rank, 0)
        idx = np.lexsort((rows, v, nan_rank, null_rank))
    else:
        if vals.dtype.kind == "i":
            u = vals.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)
        else:
            u = vals.astype(np.uint64)
        if desc:
            u = ~u
        u = np.where(ok, u, np.uint64(0))
        idx = np.lexsort((rows, u, null_rank))
    return idx[sel[idx]][:k]


def bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def check_topn(fl, t, cols, order_by, k, desc=False, nulls_first=False, filt=None, deliver=None, valid=None,
               rg_begin=0, rg_end=None, rowgroup=RG):
    """Table.topn against the numpy order: rows, and the delivered columns'
    values (by bits for floats) and validity"""
    valid = valid or {}
    n = t.nrows
    r0 = rg_begin * rowgroup
    r1 = n if rg_end is None else min(n, rg_end * rowgroup)
    sel = filter_mask(cols, filt or [], n, valid)
    sel[:r0] = False
    sel[r1:] = False
    want = expected_order(cols[order_by], valid.get(order_by), sel, k, desc, nulls_first)
    rows, values, ok = t.topn(order_by, k, cols=deliver, filt=filt, desc=desc, nulls_first=nulls_first,
                              rg_begin=rg_begin, rg_end=rg_end)
    assert rows.dtype == np.uint64
    assert np.array_equal(rows, want.astype(np.uint64)), (order_by, k, desc, nulls_first, rows[:8], want[:8])
    for c in (range(t.ncols) if deliver is None else deliver):
        v = valid.get(c)
        keep = np.ones(len(want), bool) if v is None else v[want]
        if keep.all():
            assert ok[c] is None, c
        else:
            assert np.array_equal(ok[c], keep), c
        if isinstance(cols[c], list):
            assert [g for g, m in zip(values[c], keep) if m] == [cols[c][i] for i in want[keep]], c
        else:
            assert values[c].dtype == cols[c].dtype, c
            assert np.array_equal(bits(values[c][keep]), bits(cols[c][want[keep]])), c
    for c in range(t.ncols):
        if deliver is not None and c not in deliver:
            assert values[c] is None and ok[c] is None
    return rows


# ---- CPU: exports, arguments, empty results
def test_library_exports_fls_topn(_built):
    so = C.CDLL(str(LIB))
    for name in ("fls_topn", "fls_topn_result_nrows", "fls_topn_result_rows", "fls_topn_result_column",
                 "fls_topn_result_times", "fls_topn_result_free", "fls_topn_pruned"):
        assert hasattr(so, name), name


@pytest.fixture(scope="module")
def argtab(fl):
    n = 3 * RG
    ids = np.arange(n, dtype=np.int64)
    img = fl.write_image([("i", fl.INT64, ids, fl.ENC_AUTO), ("s", fl.VARCHAR, [b"x"] * n, fl.ENC_DICT),
                          ("b", fl.BLOB, [b"y"] * n, fl.ENC_FSST), ("w", fl.DECIMAL, ids, fl.ENC_AUTO, 20, 2),
                          ("d", fl.DECIMAL, ids, fl.ENC_AUTO, 15, 2)], rowgroup=RG)
    t = fl.Connection([0]).read_image(img)
    yield t
    t.close()


@pytest.mark.parametrize("kw,what", [
    (dict(order_by=5, k=1), r"order key: column 5 out of range"),
    (dict(order_by=1, k=1), r"order key: a VARCHAR / BLOB column \(1\)"),
    (dict(order_by=2, k=1), r"order key: a VARCHAR / BLOB column \(2\)"),
    (dict(order_by=3, k=1), r"order key: DECIMAL\(20\) column 3 is wider than 64 bits"),
    (dict(order_by=0, k=1, cols=[]), r"order key: col_mask names no column"),
    (dict(order_by=0, k=1, rg_begin=2, rg_end=1), r"order key: row-group range \[2,1\) out of bounds"),
    (dict(order_by=0, k=1, rg_end=4), r"order key: row-group range \[0,4\) out of bounds"),
])
def test_argument_errors_before_any_device_work(fl, argtab, kw, what):
    with pytest.raises(fl.FlsError, match=what) as ei:
        argtab.topn(**kw)
    assert ei.value.code == ERR_ARG
    # the table stays usable
    assert len(argtab.topn(0, 0)[0]) == 0


def test_k_above_the_cap_is_a_limit_error(fl, argtab):
    with pytest.raises(fl.FlsError, match=r"k = 1025 is above 1024 \(kMaxTopN\); scan") as ei:
        argtab.topn(0, 1025)
    assert ei.value.code == ERR_LIMIT


def test_empty_results_need_no_gpu(fl, argtab):
    for kw in (dict(k=0), dict(k=5, rg_begin=1, rg_end=1), dict(k=5, filt=[(0, "<", 0)]),
               dict(k=5, filt=[(0, ">", 10 ** 9)], cols=[4])):
        rows, values, valid = argtab.topn(0, **kw)
        assert rows.dtype == np.uint64 and len(rows) == 0
        for c in kw.get("cols", range(argtab.ncols)):
            assert len(values[c]) == 0 and valid[c] is None
    assert argtab.topn(0, 5, filt=[(0, "<", 0)])[0].size == 0 and argtab.pruned == 3
    empty = fl.Connection([0]).read_image(fl.write_image([("i", fl.INT32, np.zeros(0, np.int32), fl.ENC_AUTO)]))
    assert len(empty.topn(0, 10)[0]) == 0


# ---- CPU: zone-map pruning by the k-th bound (host only)
PRUNE_RGS = 16


def prune_table(fl, vals, **kw):
    return fl.Connection([0]).read_image(fl.write_image([("k", fl.INT64, vals, fl.ENC_AUTO),
                                                         ("f", fl.INT32, np.arange(len(vals), dtype=np.int32),
                                                          fl.ENC_AUTO)], rowgroup=RG, **kw))


def test_zone_map_pruning_counts(fl):
    n = PRUNE_RGS * RG
    sorted_vals = np.arange(n, dtype=np.int64) * 3 - 7000
    t = prune_table(fl, sorted_vals)
    assert t.nrowgroups == PRUNE_RGS
    assert t.topn_pruned(0, 10) == 15
    assert t.topn_pruned(0, 10, desc=True) == 15
    assert t.topn_pruned(0, 1024) == 15 and t.topn_pruned(0, 1024, desc=True) == 15
    assert t.topn_pruned(0, 1025 - 1, rg_begin=4) == 11
    assert t.topn_pruned(0, 1) == 15 and t.topn_pruned(0, 0) == 0
    # the boundary value duplicated across two row groups: the tie is kept
    dup = sorted_vals.copy()
    dup[RG] = dup[RG - 1]
    td = prune_table(fl, dup)
    assert td.topn_pruned(0, 10) == 14 and td.topn_pruned(0, 1024) == 14
    assert td.topn_pruned(0, 10, desc=True) == 15
    dupd = sorted_vals.copy()
    dupd[-RG - 1] = dupd[-RG]
    assert prune_table(fl, dupd).topn_pruned(0, 10, desc=True) == 14
    # with a filter set only the filter prunes
    t.set_filter([(1, ">=", 12 * RG)])
    try:
        assert t.topn_pruned(0, 10) == 12
    finally:
        t.set_filter(None)
    t.set_filter([(1, ">=", 0)])
    try:
        assert t.topn_pruned(0, 10) == 0
    finally:
        t.set_filter(None)
    # a FLOAT / DOUBLE key is not pruned this way
    tf = fl.Connection([0]).read_image(fl.write_image([("k", fl.DOUBLE, sorted_vals.astype(np.float64),
                                                        fl.ENC_AUTO)], rowgroup=RG))
    assert tf.topn_pruned(0, 10) == 0


def test_zone_map_pruning_with_nulls(fl):
    n = PRUNE_RGS * RG
    vals = np.ma.masked_array(np.arange(n, dtype=np.int64), mask=np.zeros(n, bool))
    vals.mask[9 * RG + 5] = True          # one NULL in row group 9
    vals.mask[12 * RG:13 * RG] = True     # row group 12 all NULL: no zone map, always read
    t = prune_table(fl, vals)
    assert t.zonemap(9, 0)[2] & 8 and t.zonemap(12, 0)[2] & 16
    # NULLS LAST: the NULL is behind every value, the strict test on the values decides
    assert t.topn_pruned(0, 10) == 14
    # NULLS FIRST: the row group with a NULL is kept
    assert t.topn_pruned(0, 10, nulls_first=True) == 13
    # descending: row group 15 guarantees the bound; 9 and 12 as above
    assert t.topn_pruned(0, 10, desc=True) == 14
    assert t.topn_pruned(0, 10, desc=True, nulls_first=True) == 13
    # a row group with a NULL guarantees no row: the bound comes from the other one, which it beats
    first = np.ma.masked_array(np.arange(2 * RG, dtype=np.int64), mask=np.zeros(2 * RG, bool))
    first.mask[3] = True
    assert prune_table(fl, first).topn_pruned(0, 10) == 0


def test_topn_kernel_resources():
    """Both kernels: no scratch, no VGPR spill, within the register and LDS
    budget DESIGN.md section 20 states: at most 64 VGPRs (eight waves per
    SIMD), LDS 12 KB + the four wave counts in stage 1 and 24 KB in stage 2."""
    if not LIB.exists():
        pytest.skip("libflsgpu.so not built")
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    res = kernel_resources.resources(str(LIB))
    budgets = {"topn_vector_kernel": (64, 12 * 1024 + 16), "topn_merge_kernel": (64, 24 * 1024)}
    for part, (vgprs, lds) in budgets.items():
        hits = {k: v for k, v in res.items() if part in k}
        assert len(hits) == 1, (part, sorted(res))
        for name, r in hits.items():
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
            assert r["vgpr"] + r["agpr"] <= vgprs and r["lds"] <= lds, (name, r)


# ---- GPU
@pytest.fixture(scope="module")
def conn0(fl):
    conn = fl.Connection([0])
    yield conn
    conn.close()


def int_values(dtype, n, rng):
    """random values of the whole range with the minimum and the maximum among
    them, each more than once (ties at the edges of the DESC inversion)"""
    info = np.iinfo(dtype)
    v = rand64(rng, n).astype(dtype) if info.bits == 64 else \
        rng.integers(info.min, int(info.max) + 1, n, dtype=np.int64).astype(dtype)
    at = rng.choice(n, 8, replace=False)
    v[at[:4]] = info.min
    v[at[4:]] = info.max
    return v


KEY_TYPES = ["INT8", "INT16", "INT32", "INT64", "UINT8", "UINT16", "UINT32", "UINT64", "BOOLEAN", "DATE", "DECIMAL",
             "FLOAT", "DOUBLE"]


def key_column(fl, name, rng):
    ty = getattr(fl, name)
    if name == "BOOLEAN":
        return ty, rng.integers(0, 2, N_T).astype(np.uint8), ()
    if name == "DECIMAL":
        v = rng.integers(-10 ** 15 + 1, 10 ** 15, N_T, dtype=np.int64)
        v[[5, 1029]] = -10 ** 15 + 1
        v[[77, 5200]] = 10 ** 15 - 1
        return ty, v, (15, 2)
    if name in ("FLOAT", "DOUBLE"):
        v = special_doubles(N_T, rng)
        mix = rng.random(N_T) < 0.5
        v[mix] = rng.standard_normal(int(mix.sum())) * 1e3
        with np.errstate(over="ignore"):     # 1e300 as a FLOAT is +inf
            return ty, v.astype(fl.NP_DTYPE[ty]), ()
    return ty, int_values(fl.NP_DTYPE[ty], N_T, rng), ()


@pytest.mark.gpu
@pytest.mark.parametrize("name", KEY_TYPES)
def test_gpu_every_key_type(fl, gpu, conn0, name):
    rng = np.random.default_rng(KEY_TYPES.index(name))
    ty, vals, ws = key_column(fl, name, rng)
    ids = np.arange(N_T, dtype=np.int32)
    t = conn0.read_image(fl.write_image([("k", ty, vals, fl.ENC_AUTO, *ws), ("id", fl.INT32, ids, fl.ENC_AUTO)],
                                        rowgroup=RG))
    cols = {0: vals, 1: ids}
    try:
        for desc in (False, True):
            for k in KS:
                check_topn(fl, t, cols, 0, k, desc=desc)
    finally:
        t.close()


@pytest.mark.gpu
def test_gpu_ties_break_by_row_index(fl, gpu, conn0):
    n = 3 * 2048 + 100
    const = np.full(n, 7, np.int32)
    two = (np.arange(n) // 700 % 2).astype(np.int16)   # runs of 700 cross vector and row-group boundaries
    zeros = np.where(np.arange(n) % 3 == 0, -0.0, 0.0)
    nans = np.full(n, np.nan)
    nans[1::2] = np.float64(np.array([0x7FF8000000000001], np.uint64).view(np.float64)[0])
    t = conn0.read_image(fl.write_image([("c", fl.INT32, const, fl.ENC_AUTO), ("t", fl.INT16, two, fl.ENC_AUTO),
                                         ("z", fl.DOUBLE, zeros, fl.ENC_AUTO), ("n", fl.DOUBLE, nans, fl.ENC_AUTO)],
                                        rowgroup=2048))
    cols = {0: const, 1: two, 2: zeros, 3: nans}
    try:
        for desc in (False, True):
            for k in (1, 100, 1024):
                rows = check_topn(fl, t, cols, 0, k, desc=desc, rowgroup=2048)
                assert np.array_equal(rows, np.arange(k, dtype=np.uint64))      # a constant: the first k rows
                for c in (2, 3):                                                # -0 / +0 and NaN / NaN are ties
                    assert np.array_equal(check_topn(fl, t, cols, c, k, desc=desc, rowgroup=2048),
                                          np.arange(k, dtype=np.uint64))
            for k in (1, 699, 700, 701, 1024):
                check_topn(fl, t, cols, 1, k, desc=desc, rowgroup=2048)
    finally:
        t.close()


@pytest.mark.gpu
def test_gpu_odd_vector_counts_in_the_merge_tree(fl, gpu, conn0):
    """row groups of five vectors (three levels, an odd list at two of them) and
    a last one of four with a partial tail; few distinct keys, so ties cross
    every boundary of the tree"""
    rowgroup = 5 * 1024
    n = 2 * rowgroup + 3 * 1024 + 17
    rng = np.random.default_rng(17)
    key = rng.integers(-40, 40, n).astype(np.int16)
    wide = rand64(rng, n).astype(np.uint64)
    ids = np.arange(n, dtype=np.int32)
    t = conn0.read_image(fl.write_image([("k", fl.INT16, key, fl.ENC_AUTO), ("w", fl.UINT64, wide, fl.ENC_AUTO),
                                         ("id", fl.INT32, ids, fl.ENC_AUTO)], rowgroup=rowgroup))
    cols = {0: key, 1: wide, 2: ids}
    holes = [(2, "<", 2048, 1), (2, ">=", 3072, 1), (2, "<", 11000)]     # empties vector 2 and the tail
    try:
        assert t.nrowgroups == 3
        for c in (0, 1):
            for desc in (False, True):
                for k in (1, 100, 1024):
                    check_topn(fl, t, cols, c, k, desc=desc, rowgroup=rowgroup)
                    check_topn(fl, t, cols, c, k, desc=desc, filt=holes, deliver=[2], rowgroup=rowgroup)
    finally:
        t.close()


@pytest.fixture(scope="module")
def nulltab(fl, conn0):
    """2048-row row groups: row group 0 has NULLs in its first vector and an
    all-NULL second vector, row group 1 is all NULL, 2 has none, 3 (partial)
    some"""
    n = 3 * 2048 + 1500
    rng = np.random.default_rng(11)
    vals = rng.integers(-1000, 1000, n).astype(np.int32)
    null = np.zeros(n, bool)
    null[:1024] = rng.random(1024) < 0.3
    null[1024:2048] = True
    null[2048:4096] = True
    null[6144:] = rng.random(n - 6144) < 0.5
    dbl = special_doubles(n, rng)
    ids = np.arange(n, dtype=np.int32)
    img = fl.write_image([("k", fl.INT32, np.ma.masked_array(vals, mask=null), fl.ENC_AUTO),
                          ("d", fl.DOUBLE, np.ma.masked_array(dbl, mask=null[::-1].copy()), fl.ENC_AUTO),
                          ("id", fl.INT32, ids, fl.ENC_AUTO)], rowgroup=2048)
    t = conn0.read_image(img)
    yield t, {0: vals, 1: dbl, 2: ids}, {0: ~null, 1: ~null[::-1]}
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key", [0, 1], ids=["int32", "double"])
def test_gpu_null_keys(fl, gpu, nulltab, key):
    t, cols, valid = nulltab
    nonnull = int(valid[key].sum())
    for desc in (False, True):
        for nulls_first in (False, True):
            for k in (10, 1024):                  # below the non-NULL rows
                assert k < nonnull
                check_topn(fl, t, cols, key, k, desc=desc, nulls_first=nulls_first, valid=valid, rowgroup=2048)
            # above them, through a filter that leaves few values: NULLs fill the result
            filt = [(2, "<", 3000)] if key == 0 else [(2, ">=", t.nrows - 3000)]
            assert 0 < int((valid[key] & filter_mask(cols, filt, t.nrows)).sum()) < 1024
            check_topn(fl, t, cols, key, 1024, desc=desc, nulls_first=nulls_first, filt=filt, valid=valid,
                       rowgroup=2048)


@pytest.fixture(scope="module")
def filtertab(fl, conn0):
    n = 6 * 2048 + 77
    rng = np.random.default_rng(5)
    key = rand64(rng, n).astype(np.int64)
    ids = np.arange(n, dtype=np.int32)
    vec = (ids // 1024).astype(np.int32)
    words = [b"alpha", b"beta", b"a string over twelve bytes", b"gamma"]
    dct = [words[i] for i in rng.integers(0, 4, n)]
    txt = [s.encode() for s in fsst_text(n, rng)]
    img = fl.write_image([("k", fl.INT64, key, fl.ENC_AUTO), ("id", fl.INT32, ids, fl.ENC_AUTO),
                          ("vec", fl.INT32, vec, fl.ENC_AUTO), ("d", fl.VARCHAR, dct, fl.ENC_DICT),
                          ("f", fl.VARCHAR, txt, fl.ENC_FSST)], rowgroup=2048)
    t = conn0.read_image(img)
    yield t, {0: key, 1: ids, 2: vec, 3: dct, 4: txt}
    t.close()


@pytest.mark.gpu
def test_gpu_under_a_filter(fl, gpu, filtertab):
    t, cols = filtertab
    cases = {
        "empties some vectors": [(2, "=", 1, 1), (2, "=", 4, 1), (2, "=", 7, 1), (2, "=", 12, 1)],
        "empties whole row groups": [(2, ">=", 6), (2, "<", 10)],
        "fewer than k rows": [(1, ">=", 2040), (1, "<", 2055)],
        "dict string": [(3, "=", "a string over twelve bytes")],
        "fsst string": [(4, ">=", "f"), (4, "<", "s")],
        "no row at all": [(1, "<", 0)],
    }
    for what, filt in cases.items():
        for desc in (False, True):
            for k in (1, 64, 1024):
                check_topn(fl, t, cols, 0, k, desc=desc, filt=filt, deliver=[0, 1], rowgroup=2048)
        if what == "empties whole row groups":
            assert t.pruned == 5
        if what == "fewer than k rows":
            assert len(t.topn(0, 64, filt=filt)[0]) == 15
    # a row-group range
    check_topn(fl, t, cols, 0, 100, rg_begin=2, rg_end=5, rowgroup=2048)
    check_topn(fl, t, cols, 0, 100, filt=cases["dict string"], rg_begin=5, rg_end=7, rowgroup=2048)


@pytest.mark.gpu
def test_gpu_delivered_columns_and_result_outlives_the_table(fl, gpu, conn0):
    n = 4 * RG + 50
    rng = np.random.default_rng(21)
    key = rng.integers(-10 ** 6, 10 ** 6, n).astype(np.int32)
    i64 = rand64(rng, n).astype(np.int64)
    dbl = special_doubles(n, rng)
    long_words = [b"short", b"exactly12byt", b"thirteen byte", b"a considerably longer dictionary string", b""]
    dct = [long_words[i] for i in rng.integers(0, len(long_words), n)]
    txt = [s.encode() for s in fsst_text(n, rng)]
    null = rng.random(n) < 0.3
    nul = np.ma.masked_array(rng.integers(0, 1000, n).astype(np.int16), mask=null)
    snull = [None if z else s for s, z in zip(txt, null[::-1])]
    img = fl.write_image([("k", fl.INT32, key, fl.ENC_AUTO), ("i", fl.INT64, i64, fl.ENC_AUTO),
                          ("x", fl.DOUBLE, dbl, fl.ENC_AUTO), ("d", fl.VARCHAR, dct, fl.ENC_DICT),
                          ("f", fl.VARCHAR, txt, fl.ENC_FSST), ("n", fl.INT16, nul, fl.ENC_AUTO),
                          ("sn", fl.VARCHAR, snull, fl.ENC_AUTO)], rowgroup=RG)
    cols = {0: key, 1: i64, 2: dbl, 3: dct, 4: txt, 5: nul.filled(0), 6: txt}
    valid = {5: ~null, 6: ~null[::-1]}
    t = conn0.read_image(img)
    res = C.c_void_p()
    try:
        for k in (1, 40, 1024):
            check_topn(fl, t, cols, 0, k, valid=valid)
            check_topn(fl, t, cols, 0, k, desc=True, valid=valid, deliver=[3, 4, 5, 6])
        check_topn(fl, t, cols, 5, 700, valid=valid, nulls_first=True, deliver=[1, 5, 6])
        # the key column is delivered only if masked in
        rows, values, ok = t.topn(0, 5, cols=[2])
        assert values[0] is None and values[2] is not None
        # the raw result owns its bytes: it is read below, after the table is closed
        key_spec = fl.OrderKey(col=0, desc=1, nulls_first=0)
        assert fl.lib.fls_topn(t.h, C.byref(key_spec), 50, None, 0, t.nrowgroups, C.byref(res)) == 0
    finally:
        t.close()
    try:
        assert fl.lib.fls_topn_result_nrows(res) == 50
        rows = np.ctypeslib.as_array(fl.lib.fls_topn_result_rows(res), shape=(50,)).copy()
        want = expected_order(key, None, np.ones(n, bool), 50, desc=True)
        assert np.array_equal(rows, want.astype(np.uint64))
        for c in (3, 4):
            pv, pw = C.c_void_p(), C.POINTER(C.c_uint64)()
            assert fl.lib.fls_topn_result_column(res, c, C.byref(pv), C.byref(pw)) == 0
            raw = np.ctypeslib.as_array(C.cast(pv, C.POINTER(C.c_uint8)), shape=(50 * 16,)).copy()
            assert fl.string_t_decode(raw) == [cols[c][i] for i in want]
            assert not pw
        assert fl.lib.fls_topn_result_column(res, 7, None, None) == ERR_ARG
    finally:
        fl.lib.fls_topn_result_free(res)


@pytest.mark.gpu
def test_gpu_results_are_identical_across_batches_and_pipelines(fl, gpu, conn0, monkeypatch):
    nrg = 23
    n = nrg * RG - 400
    rng = np.random.default_rng(3)
    key = rng.integers(0, 50, n).astype(np.int64)       # many ties across row groups
    dbl = special_doubles(n, rng)
    ids = np.arange(n, dtype=np.int32)
    img = fl.write_image([("k", fl.INT64, key, fl.ENC_AUTO), ("x", fl.DOUBLE, dbl, fl.ENC_AUTO),
                          ("id", fl.INT32, ids, fl.ENC_AUTO)], rowgroup=RG)
    cols = {0: key, 1: dbl, 2: ids}
    filt = [(2, ">=", 1500)]

    def run(t):     # (the batch size is read when a scan starts)
        out = []
        for c in (0, 1):
            for desc in (False, True):
                for f in (None, filt):
                    rows, values, _ = t.topn(c, 1000, filt=f, desc=desc)
                    out.append((rows.tobytes(), bits(values[c]).tobytes(), values[2].tobytes()))
        return out

    t = conn0.read_image(img)
    assert t.nrowgroups == nrg
    monkeypatch.delenv("FLS_SCAN_BATCH", raising=False)
    base = run(t)
    check_topn(fl, t, cols, 0, 1000, filt=filt)
    check_topn(fl, t, cols, 1, 1000, desc=True)
    for batch in ("1", "3"):
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)
        assert run(t) == base, batch
    monkeypatch.setenv("FLS_SCAN_SLOTS", "4")       # four batches in flight, the last two on recycled host batches
    assert run(t) == base, "batch 3, four slots"
    monkeypatch.delenv("FLS_SCAN_SLOTS")
    conn2 = fl.Connection([0, 0])       # the row groups sharded over two pipelines
    t2 = conn2.read_image(img)
    try:
        assert run(t2) == base, "batch 3, two pipelines"
        monkeypatch.delenv("FLS_SCAN_BATCH")
        assert run(t2) == base, "default batch, two pipelines"
    finally:
        t2.close()
        conn2.close()
        t.close()


@pytest.mark.gpu
def test_gpu_k1_equals_min_and_max(fl, gpu, filtertab, nulltab):
    t, cols = filtertab
    for filt in (None, [(2, "=", 3, 1), (2, "=", 9, 1)], [(3, "=", "beta")]):
        mn, mx = t.aggregate([("min", 0), ("max", 0)], filt=filt)
        assert int(t.topn(0, 1, cols=[0], filt=filt)[1][0][0]) == mn
        assert int(t.topn(0, 1, cols=[0], filt=filt, desc=True)[1][0][0]) == mx
    tn, ncols, _ = nulltab
    for c in (0, 1):
        mn, mx = tn.aggregate([("min", c), ("max", c)])
        lo, hi = tn.topn(c, 1, cols=[c])[1][c][0], tn.topn(c, 1, cols=[c], desc=True)[1][c][0]
        if c == 1:       # NaN is the maximum; -0 and +0 are one value
            assert (np.isnan(mx) and np.isnan(hi)) or hi == mx
            assert lo == mn
        else:
            assert (int(lo), int(hi)) == (mn, mx)


# ---- lineitem at the scale of tests/test_aggregate.py
SF, WL = 0.1, "lineitem"
DAY_1994, DAY_1995 = 8766, 9131
C_OKEY, C_QTY, C_PRICE, C_DISC, C_SHIPDATE = 0, 4, 5, 6, 10
Q6 = [(C_SHIPDATE, ">=", DAY_1994), (C_SHIPDATE, "<", DAY_1995), (C_DISC, ">=", 5), (C_DISC, "<=", 7),
      (C_QTY, "<", 2400)]


def test_lineitem_orderkey_reads_one_row_group(fl):
    t = fl.Connection([0]).read_image(fl.gen_image(WL, SF))
    assert t.nrowgroups > 2
    assert t.topn_pruned(C_OKEY, 10) == t.nrowgroups - 1


@pytest.mark.gpu
def test_gpu_lineitem(fl, gpu, conn0):
    t = conn0.read_image(fl.gen_image(WL, SF))
    n = t.nrows
    cols = {}
    for c, (name, ty, _, _, _) in enumerate(t.schema()):
        if ty == fl.VARCHAR:
            codes = fl.gen_values(WL, c, 0, n, np.uint32, SF)
            words = []
            while (s := fl.gen_dict_string(WL, c, len(words))) is not None:
                words.append(s.encode())
            cols[c] = [words[k] for k in codes]
        else:
            cols[c] = fl.gen_values(WL, c, 0, n, fl.NP_DTYPE[ty], SF)
    try:
        check_topn(fl, t, cols, C_PRICE, 10, desc=True, filt=Q6, rowgroup=fl.ROWGROUP)
        rows = check_topn(fl, t, cols, C_OKEY, 10, rowgroup=fl.ROWGROUP)
        assert np.array_equal(rows, np.arange(10, dtype=np.uint64))
        assert t.pruned == t.nrowgroups - 1
    finally:
        t.close()
