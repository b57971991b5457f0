"""Key sets built on the GPU from a filtered scan (fls_keyset_from_scan /
Table.keyset): the C call's refusals, the no-device-work
cases and the gate without a GPU; keyset_build_kernel on the GPU against
np.unique through every key type, encoding, atomic path, filter kind and
pipeline shape.

Small shapes throughout, as in test_keyset.py: 1024-row row groups, five whole
vectors and a partial tail."""
import ctypes as C

import numpy as np
import pytest

from test_keyset import KEY_TYPES, as_signed, key_pool, type_range

RG = 1024
N = 5 * 1024 + 333
M64 = (1 << 64) - 1
ERR_ARG, ERR_LIMIT = -3, -8
BITMAP, HASH = 1, 2
C_OKEY, C_PRICE, C_SHIPDATE = 0, 5, 10


# ---- helpers of this file
def is_signed(fl, ty):
    return ty in (fl.INT8, fl.INT16, fl.INT32, fl.INT64, fl.DATE, fl.DECIMAL)


def from_scan(fl, t, col, rg0=0, rg1=None, form=0):
    """the raw C call under the filter currently set: (KeySet, KeySetBuildInfo)"""
    h, info = C.c_void_p(), fl.KeySetBuildInfo()
    fl._check(fl.lib.fls_keyset_from_scan(t.h, col, rg0, t.nrowgroups if rg1 is None else rg1, form, C.byref(h),
                                          C.byref(info)))
    return fl.KeySet(h.value, t.conn, info), info


def same_info(fl, a, b):
    return all(getattr(a, n) == getattr(b, n) for n, _ in fl.KeySetInfo._fields_)


def scan_rows(t, filt, col):
    rows = [sel.astype(np.int64) + first for _, first, sel, _ in t.scan_filtered(filt, cols=[col])]
    return np.concatenate(rows) if rows else np.zeros(0, np.int64)


def check_set(fl, conn, t, col, vals, sel, ks, form=0, pool=None, valid=None, device=True, info=None):
    """the four checks of a set built from column col (values vals, numpy) over
    the rows sel (bool per row, NULL rows excluded) against the reference
    conn.keyset(np.unique(vals[sel]))"""
    want = np.unique(vals[sel])
    ref = conn.keyset(want, signed=is_signed(fl, t.column(col).type), form=form)
    try:
        # 1. the image's description, field for field
        assert same_info(fl, ks.info, ref.info), [(n, getattr(ks.info, n), getattr(ref.info, n))
                                                  for n, _ in fl.KeySetInfo._fields_]
        # 2. membership over the pool and its neighbours
        members = {int(v) & M64 for v in want}
        probes = {int(v) + d for v in (pool if pool is not None else np.unique(vals)) for d in (-1, 0, 1)}
        for p in probes:
            assert ks.contains(p) == ((p & M64) in members), p
        # 3. a scan under the built set selects the rows whose value is one of the keys
        hit = np.isin(vals, want) if len(want) else np.zeros(len(vals), bool)
        if valid is not None:
            hit &= valid
        assert np.array_equal(scan_rows(t, [(col, "in_set", ks)], col), np.nonzero(hit)[0])
        # 4. what the build says of itself
        bi = ks.build_info if info is None else info
        if not device:
            assert bi is None
            return
        assert bi is not None and bi.rows_selected == int(sel.sum()), (bi and bi.rows_selected, int(sel.sum()))
        if bi.bitmap_bytes > 1 << 20:                      # the gate's second arm decided
            assert bi.d2h_bytes < 8 * bi.rows_selected
        if bi.rowgroups_read:
            assert bi.bitmap_bytes == (bi.span // 64 + 1) * 8 and bi.d2h_bytes >= bi.bitmap_bytes
    finally:
        ref.close()


def check_build(fl, conn, t, col, vals, sel, filt=None, forms=(0,), **kw):
    for form in forms:
        ks = t.keyset(col, filt, form=form)
        try:
            check_set(fl, conn, t, col, vals, sel, ks, form=form, **kw)
        finally:
            ks.close()


@pytest.fixture(scope="module")
def conn(fl):
    c = fl.Connection([0])
    yield c
    c.close()


# ------------------------------------------------------------------ CPU tests
def test_library_exports_the_build_call(fl):
    assert hasattr(fl.lib, "fls_keyset_from_scan")
    assert C.sizeof(fl.KeySetBuildInfo) == 48


@pytest.fixture(scope="module")
def typed(fl, conn):
    """one column per kind of type the argument checks tell apart (test_keyset.typed)"""
    n = 2 * RG + 100
    rng = np.random.default_rng(1)
    cols = [("i", fl.INT32, rng.integers(-50, 50, n).astype(np.int32), fl.ENC_AUTO),
            ("u", fl.UINT16, rng.integers(0, 50, n).astype(np.uint16), fl.ENC_AUTO),
            ("s", fl.VARCHAR, [f"s{i % 7}" for i in range(n)], fl.ENC_DICT),
            ("f", fl.FLOAT, rng.random(n).astype(np.float32), fl.ENC_AUTO),
            ("d", fl.DOUBLE, rng.random(n), fl.ENC_AUTO),
            ("w", fl.DECIMAL, rng.integers(0, 9, n).astype(np.int64), fl.ENC_AUTO, 15, 2),
            ("x", fl.DECIMAL, rng.integers(0, 9, n).astype(np.int64), fl.ENC_AUTO, 20, 2),
            ("b", fl.BLOB, [b"y%d" % (i % 5) for i in range(n)], fl.ENC_FSST)]
    t = conn.read_image(fl.write_image(cols, rowgroup=RG))
    yield t
    t.close()


def test_argument_refusals_come_before_any_device_work(fl, conn, typed):
    t = typed
    h, info = C.c_void_p(), fl.KeySetBuildInfo()
    call = lambda *a: fl.lib.fls_keyset_from_scan(*a, C.byref(h), C.byref(info))    # noqa: E731
    nrg = t.nrowgroups
    assert call(t.h, t.ncols, 0, nrg, 0) == ERR_ARG and "column 8 out of range" in fl.last_error()
    for col in (2, 3, 4, 7):                                                         # VARCHAR, FLOAT, DOUBLE, BLOB
        assert call(t.h, col, 0, nrg, 0) == ERR_ARG
        assert f"VARCHAR / BLOB / FLOAT / DOUBLE column ({col})" in fl.last_error()
    assert call(t.h, 6, 0, nrg, 0) == ERR_ARG and "DECIMAL wider than 64 bits (column 6)" in fl.last_error()
    for form in (-1, 3):
        assert call(t.h, 0, 0, nrg, form) == ERR_ARG
        assert f"form {form} (0 auto, 1 bitmap, 2 hash)" in fl.last_error()
    for rg0, rg1 in ((0, nrg + 1), (2, 1), (nrg + 1, nrg + 2)):
        assert call(t.h, 0, rg0, rg1, 0) == ERR_ARG and "row-group range" in fl.last_error()
    assert fl.lib.fls_keyset_from_scan(None, 0, 0, nrg, 0, C.byref(h), None) == ERR_ARG
    assert fl.lib.fls_keyset_from_scan(t.h, 0, 0, nrg, 0, None, None) == ERR_ARG
    assert h.value is None
    # the Python call keeps its own refusal
    for col in (2, 3, 4, 7):
        with pytest.raises(ValueError, match="not integer-like"):
            t.keyset(col)


def test_no_surviving_row_group_gives_the_empty_set_without_a_gpu(fl, conn, typed):
    t = typed
    for form in (0, BITMAP, HASH):
        ref = conn.keyset([], form=form).info
        # every row group pruned by the filter's zone maps
        ks = t.keyset(0, [(0, ">", 1000)], form=form)
        assert same_info(fl, ks.info, ref) and not ks.contains(0)
        bi = ks.build_info
        assert (bi.rows_selected, bi.bitmap_bytes, bi.d2h_bytes, bi.rowgroups_read, bi.rowgroups_pruned) == \
            (0, 0, 0, 0, t.nrowgroups)
        # ... by an empty set, by alternatives none of which may match
        e = conn.keyset([])
        assert t.keyset(1, [(0, "in_set", e)], form=form).info.count == 0
        assert t.keyset(5, [fl.AnyOf([(0, ">", 1000)], [(1, ">", 1000)])], form=form).info.count == 0
        # an empty range through the C call, signed and unsigned columns
        for col, kind in ((0, 0), (1, 1), (5, 0)):
            ks, bi = from_scan(fl, t, col, 1, 1, form)
            assert same_info(fl, ks.info, conn.keyset([], signed=kind == 0, form=form).info)
            assert (bi.rowgroups_read, bi.rowgroups_pruned, bi.d2h_bytes) == (0, 0, 0)
            # the set sits in the registry like any other: usable in a filter, freed by its handle
            t.set_filter([(col, "in_set", ks)])
            t.set_filter([])
            ks.close()
            assert fl.lib.fls_keyset_contains(ks.h or 0, 1) == ERR_ARG


def test_all_null_key_chunks_are_skipped_without_a_gpu(fl, conn):
    vals = np.ma.masked_array(np.arange(2 * RG, dtype=np.int64), mask=np.ones(2 * RG, bool))
    t = conn.read_image(fl.write_image([("k", fl.INT64, vals, fl.ENC_AUTO)], rowgroup=RG))
    try:
        ks = t.keyset(0)
        assert ks.info.count == 0
        assert (ks.build_info.rowgroups_read, ks.build_info.rowgroups_pruned) == (0, 2)
    finally:
        t.close()


def test_the_gate_refuses_wide_ranges_before_any_device_work(fl, conn):
    rng = np.random.default_rng(5)
    wide = rng.integers(0, 1 << 20, N).astype(np.int64)
    wide[7], wide[N - 9] = -5, (1 << 32) - 5                        # the zone maps span exactly 2^32 values + 1
    mid = rng.integers(100, 1 << 20, N).astype(np.int64)
    mid[3], mid[N - 2] = 100, 100 + (1 << 24)                       # ... 2^24 + 1 values: a 2 MiB bitmap
    t = conn.read_image(fl.write_image([("w", fl.INT64, wide, fl.ENC_AUTO), ("m", fl.INT64, mid, fl.ENC_AUTO)],
                                       rowgroup=RG))
    try:
        h = C.c_void_p()
        for form in (0, BITMAP, HASH):
            assert fl.lib.fls_keyset_from_scan(t.h, 0, 0, t.nrowgroups, form, C.byref(h), None) == ERR_LIMIT
            msg = fl.last_error()
            assert f"span {(1 << 32) + 1} values" in msg and "kKeysetMaxSpan" in msg and f"{N * 8} bytes" in msg, msg
            assert fl.lib.fls_keyset_from_scan(t.h, 1, 0, t.nrowgroups, form, C.byref(h), None) == ERR_LIMIT
            msg = fl.last_error()
            bitmap = ((1 << 24) // 64 + 1) * 8                      # above 1 MiB and above N x 8
            assert bitmap > 1 << 20 and bitmap > N * 8
            assert f"span {(1 << 24) + 1} values" in msg and f"takes {bitmap} bytes" in msg and \
                f"at most {1 << 20}" in msg and f"{N * 8} bytes" in msg, msg
        assert h.value is None
        # a sub-range whose zone maps are narrow passes the gate's checks (and would need the GPU):
        # row group 1 alone spans less than 2^20 values
        lo, hi, _ = t.zonemap(1, 0)
        assert hi - lo < 1 << 20
    finally:
        t.close()


# ------------------------------------------------------------------ GPU tests
W = 1 << 20


def type_columns(fl, name, rng):
    """[(tag, pool)]: the key columns of one type.  A type whose whole range
    passes the gate draws from key_pool's edge clusters; a wider one gets a
    column per cluster, each confined to a 2^20 window (a 128 KiB bitmap) at
    the range's minimum, its maximum and, signed, around 0 / -1"""
    lo, hi = type_range(fl, name)
    pool = key_pool(fl, name, rng)
    if hi - lo < W:
        return [("all", pool)]
    far = [int(x) for x in rng.integers(0, 3000, 10)]
    out = [("lo", sorted({v for v in pool if v - lo < W} | {lo + W - 1 - x for x in far})),
           ("hi", sorted({v for v in pool if hi - v < W} | {hi - W + 1 + x for x in far}))]
    if lo < 0:
        out.append(("mid", sorted(v for v in pool if abs(v) < W // 2)))
    return out


@pytest.fixture(scope="module")
def typetab(fl, conn):
    rng = np.random.default_rng(21)
    specs, cols = [], {}
    for name in KEY_TYPES:
        ty = getattr(fl, name)
        for tag, pool in type_columns(fl, name, rng):
            vals = np.array([pool[i] for i in rng.integers(0, len(pool), N)], dtype=object).astype(fl.NP_DTYPE[ty])
            cols.setdefault(name, []).append((len(specs), vals, pool))
            specs.append((f"{name.lower()}_{tag}", ty, vals, fl.ENC_FFOR, *((15, 2) if name == "DECIMAL" else ())))
    t = conn.read_image(fl.write_image(specs, rowgroup=RG))
    yield t, cols
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", KEY_TYPES)
def test_gpu_every_key_type_against_unique(fl, gpu, conn, typetab, name):
    t, cols = typetab
    lo, hi = type_range(fl, name)
    assert len(cols[name]) == (1 if hi - lo < W else 3 if lo < 0 else 2)
    for c, vals, pool in cols[name]:
        assert lo in pool or hi in pool or -1 in pool                 # every column holds an edge of its type
        check_build(fl, conn, t, c, vals, np.ones(N, bool), forms=(0, BITMAP, HASH), pool=pool)
        # under a filter on the column itself: the upper half of its pool
        cut = pool[len(pool) // 2]
        check_build(fl, conn, t, c, vals, vals >= vals.dtype.type(cut), [(c, ">=", cut)], pool=pool)


@pytest.mark.gpu
def test_gpu_every_encoding_of_the_key_column(fl, gpu, conn):
    rng = np.random.default_rng(31)
    ffor = rng.integers(-500, 500, N).astype(np.int32)
    delta = (np.cumsum(rng.integers(0, 4, N)) - 4000).astype(np.int64)
    dic = (rng.integers(0, 9, N) * 1000003 - 3000009).astype(np.int64)
    rle = np.repeat(rng.integers(-20, 20, N // 50 + 1), 50)[:N].astype(np.int16)
    img = fl.write_image([("ffor", fl.INT32, ffor, fl.ENC_FFOR), ("delta", fl.INT64, delta, fl.ENC_DELTA),
                          ("dict", fl.INT64, dic, fl.ENC_DICT), ("rle", fl.INT16, rle, fl.ENC_RLE)], rowgroup=RG)
    from helpers import chunk_encodings
    assert {tuple(r) for r in chunk_encodings(img.tobytes())} == {(fl.ENC_FFOR, fl.ENC_DELTA, fl.ENC_DICT, fl.ENC_RLE)}
    t = conn.read_image(img)
    try:
        for c, vals in enumerate((ffor, delta, dic, rle)):
            check_build(fl, conn, t, c, vals, np.ones(N, bool), forms=(0, BITMAP, HASH))
            check_build(fl, conn, t, c, vals, ffor < 0, [(0, "<", 0)])
    finally:
        t.close()


@pytest.mark.gpu
def test_gpu_window_and_scattered_paths_and_the_64_dword_limit(fl, gpu, conn, monkeypatch):
    """a sorted column (every 64-row word inside a few dwords: the LDS window),
    the same values shuffled (one global atomic per row) and words whose values
    span 2046 to 2049 bits at every alignment within a dword, either side of
    the 64 dwords a window holds; all again with the window switched off"""
    rng = np.random.default_rng(33)
    srt = (np.cumsum(rng.integers(0, 3, N)) + 70000).astype(np.int64)      # about one key per row, duplicates
    shf = rng.permutation(srt)
    edge = np.empty(N, np.int64)
    for j in range((N + 63) // 64):
        n = min(64, N - 64 * j)
        first = 5000 * j + (j % 32)                                        # the word's smallest value, bit j % 32
        spread = 2046 + (j // 32 + j) % 4                                  # its largest: first + 2046 .. first + 2049
        w = first + rng.integers(0, spread + 1, n)
        w[0], w[-1] = first, first + spread
        edge[64 * j:64 * j + n] = rng.permutation(w)
    t = conn.read_image(fl.write_image([("s", fl.INT64, srt, fl.ENC_AUTO), ("x", fl.INT64, shf, fl.ENC_AUTO),
                                        ("e", fl.INT64, edge, fl.ENC_AUTO)], rowgroup=RG))
    try:
        for window in (None, "0"):
            if window is not None:
                monkeypatch.setenv("FLS_KEYSET_BUILD_WINDOW", window)
            for c, vals in enumerate((srt, shf, edge)):
                check_build(fl, conn, t, c, vals, np.ones(N, bool))
                check_build(fl, conn, t, c, vals, shf % 3 == 0, [(1, "in_set", conn.keyset(np.unique(shf[shf % 3 == 0])))])
    finally:
        t.close()


@pytest.mark.gpu
def test_gpu_nullable_key_column(fl, gpu, conn, monkeypatch):
    """NULLs never enter the set; the placeholder a NULL row decodes to (0)
    lies outside the column's zone maps and is never loaded; an all-NULL row
    group is skipped"""
    rng = np.random.default_rng(41)
    a = rng.integers(5000, 9000, N).astype(np.int32)
    null = rng.random(N) < 0.3
    null[2 * RG:3 * RG] = True                                             # row group 2: all NULL
    null[4 * RG:5 * RG] = False                                            # row group 4: no validity at all
    grp = rng.integers(0, 5, N).astype(np.int8)
    t = conn.read_image(fl.write_image([("a", fl.INT32, np.ma.masked_array(a, mask=null), fl.ENC_AUTO),
                                        ("g", fl.INT8, grp, fl.ENC_AUTO)], rowgroup=RG))
    try:
        assert t.validity(2, 0) is not None and t.validity(4, 0) is None
        for batch in ("1", "8"):
            monkeypatch.setenv("FLS_SCAN_BATCH", batch)                    # 8: one batch mixes chunks with / without validity
            ks = t.keyset(0)
            check_set(fl, conn, t, 0, a, ~null, ks, valid=~null)
            assert not ks.contains(0) and ks.build_info.rowgroups_pruned == 1
            assert as_signed(ks.build_info.base) >= 5000                   # the range never reached the placeholder
            ks.close()
            check_build(fl, conn, t, 0, a, ~null & (grp == 3), [(1, "=", 3)], valid=~null)
    finally:
        t.close()


@pytest.mark.gpu
def test_gpu_partial_last_vector_and_single_row(fl, gpu, conn):
    rng = np.random.default_rng(43)
    for n in (1, 63, 64, 65, 1023, 1025, RG + 1):
        vals = rng.integers(-40, 40, n).astype(np.int16)
        t = conn.read_image(fl.write_image([("k", fl.INT16, vals, fl.ENC_AUTO)], rowgroup=RG))
        try:
            check_build(fl, conn, t, 0, vals, np.ones(n, bool), forms=(0, HASH))
        finally:
            t.close()


@pytest.fixture(scope="module")
def facttab(fl, conn):
    """key, low-cardinality group, a nullable measure, two columns to compare, a string"""
    rng = np.random.default_rng(61)
    key = np.sort(rng.integers(0, 4000, N)).astype(np.int64)
    grp = rng.integers(0, 5, N).astype(np.int8)
    qty = rng.integers(1, 51, N).astype(np.int32)
    nm = rng.random(N) < 0.2
    a = rng.integers(0, 100, N).astype(np.int32)
    b = rng.integers(0, 100, N).astype(np.int32)
    words = [b"abacus", b"abbey", b"cab", b"about", b"zebra", b"ab", b"", b"lab coat"]
    s = [words[i] for i in rng.integers(0, len(words), N)]
    t = conn.read_image(fl.write_image([("key", fl.INT64, key, fl.ENC_AUTO), ("grp", fl.INT8, grp, fl.ENC_AUTO),
                                        ("qty", fl.INT32, np.ma.masked_array(qty, mask=nm), fl.ENC_AUTO),
                                        ("a", fl.INT32, a, fl.ENC_AUTO), ("b", fl.INT32, b, fl.ENC_AUTO),
                                        ("s", fl.VARCHAR, s, fl.ENC_DICT)], rowgroup=RG))
    yield t, {"key": key, "grp": grp, "qty": qty, "nm": nm, "a": a, "b": b, "s": s}
    t.close()


def fact_cases(fl, conn, c):
    """(filter, numpy mask) per kind of filter"""
    rng = np.random.default_rng(62)
    members = rng.choice(4000, 900, replace=False)
    inner = conn.keyset(members)
    ab = np.array([x.startswith(b"ab") for x in c["s"]])
    q = ~c["nm"]
    return [
        ("ordinary", [(1, "!=", 2), (2, ">", 10)], (c["grp"] != 2) & q & (c["qty"] > 10)),
        ("clauses", [(1, "=", 0, 1), (1, "=", 4, 1), (2, "is_null", None)], ((c["grp"] == 0) | (c["grp"] == 4)) & c["nm"]),
        ("key set", [(0, "in_set", inner), (1, "<", 3)], np.isin(c["key"], members) & (c["grp"] < 3)),
        ("not in set", [(0, "not_in_set", inner)], ~np.isin(c["key"], members)),
        ("like", [(5, "like", "ab%")], ab),
        ("column pair", [(3, "<", fl.Col(4)), (1, ">=", 1)], (c["a"] < c["b"]) & (c["grp"] >= 1)),
        ("any of", [(1, "<", 4), fl.AnyOf([(2, "<", 5)], [(3, ">", 50), (1, "=", 1)], [(5, "like", "%b")])],
         (c["grp"] < 4) & ((q & (c["qty"] < 5)) | ((c["a"] > 50) & (c["grp"] == 1)) |
                           np.array([x.endswith(b"b") for x in c["s"]]))),
        ("nothing", [(1, ">", 100)], np.zeros(N, bool)),
        ("nothing, not prunable", [(3, "<", fl.Col(3))], np.zeros(N, bool)),
    ]


@pytest.mark.gpu
def test_gpu_build_under_every_kind_of_filter(fl, gpu, conn, facttab):
    t, c = facttab
    for what, filt, m in fact_cases(fl, conn, c):
        assert m.any() or what.startswith("nothing"), what
        check_build(fl, conn, t, 0, c["key"], m, filt)
        # a nullable key column under the same filter
        check_build(fl, conn, t, 2, c["qty"], m & ~c["nm"], filt, valid=~c["nm"])
        # ... and the filter leaves nothing behind on the table
        assert sum(len(sel) for _, _, sel, _ in t.scan_filtered([], cols=[1])) == N


@pytest.mark.gpu
def test_gpu_results_identical_across_batches_slots_and_gpus(fl, gpu, conn, facttab, monkeypatch):
    t, c = facttab
    cases = fact_cases(fl, conn, c)[:4]
    for batch, slots in (("1", "1"), ("3", "2"), ("8", "2"), ("2", "3")):
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)
        monkeypatch.setenv("FLS_SCAN_SLOTS", slots)
        check_build(fl, conn, t, 0, c["key"], np.ones(N, bool), forms=(0, HASH))
        for _what, filt, m in cases:
            check_build(fl, conn, t, 0, c["key"], m, filt)
    monkeypatch.delenv("FLS_SCAN_BATCH")
    monkeypatch.delenv("FLS_SCAN_SLOTS")
    # every visible GPU, and one GPU listed twice (two pipelines share its bitmap)
    for devs in (list(range(gpu)), [0, 0]):
        call = fl.Connection(devs)
        try:
            tm = call.read_image(fl.write_image([("key", fl.INT64, c["key"], fl.ENC_AUTO),
                                                 ("grp", fl.INT8, c["grp"], fl.ENC_AUTO)], rowgroup=RG))
            check_build(fl, call, tm, 0, c["key"], np.ones(N, bool), forms=(0, HASH))
            check_build(fl, call, tm, 0, c["key"], c["grp"] == 2, [(1, "=", 2)])
            ks = tm.keyset(0, [(1, "=", 2)])
            assert ks.build_info.d2h_bytes >= len(set(devs)) * ks.build_info.bitmap_bytes
            tm.close()
        finally:
            call.close()


@pytest.mark.gpu
def test_gpu_rowgroup_subrange_through_the_c_call(fl, gpu, conn, facttab):
    t, c = facttab
    for rg0, rg1 in ((1, 3), (0, 1), (5, 6), (2, 6)):
        rows = np.zeros(N, bool)
        rows[rg0 * RG:rg1 * RG] = True
        for filt, m in (([], rows), ([(1, "=", 1)], rows & (c["grp"] == 1))):
            t.set_filter(filt)
            try:
                ks, info = from_scan(fl, t, 0, rg0, rg1)
            finally:
                t.set_filter([])
            check_set(fl, conn, t, 0, c["key"], m, ks, info=info)
            assert info.rowgroups_read == rg1 - rg0 and info.rowgroups_pruned == 0
            # the range is the union of the read row groups' zone maps
            zs = [t.zonemap(r, 0) for r in range(rg0, rg1)]
            assert as_signed(info.base) == min(z[0] for z in zs) and info.span == max(z[1] for z in zs) - as_signed(info.base)
            ks.close()


@pytest.mark.gpu
def test_gpu_host_route_and_gated_out_column_equal_the_device_route(fl, gpu, conn, facttab, monkeypatch):
    t, c = facttab
    filt, m = [(1, "!=", 2), (2, ">", 10)], (c["grp"] != 2) & ~c["nm"] & (c["qty"] > 10)
    dev = t.keyset(0, filt)
    monkeypatch.setenv("FLS_KEYSET_BUILD", "host")
    host = t.keyset(0, filt)
    assert dev.build_info is not None and host.build_info is None and same_info(fl, dev.info, host.info)
    check_set(fl, conn, t, 0, c["key"], m, host, device=False)
    monkeypatch.delenv("FLS_KEYSET_BUILD")
    # a column the gate refuses (its zone maps span 2^40 values): the host route, the same set
    rng = np.random.default_rng(64)
    wide = (rng.integers(0, 50, N) * ((1 << 40) // 49) - (1 << 39)).astype(np.int64)
    tw = conn.read_image(fl.write_image([("w", fl.INT64, wide, fl.ENC_AUTO), ("g", fl.INT8, c["grp"], fl.ENC_AUTO)],
                                        rowgroup=RG))
    try:
        check_build(fl, conn, tw, 0, wide, np.ones(N, bool), forms=(0, HASH), device=False)
        check_build(fl, conn, tw, 0, wide, c["grp"] == 0, [(1, "=", 0)], device=False)
    finally:
        tw.close()


@pytest.mark.gpu
def test_gpu_lineitem_semi_join_built_on_the_device(fl, gpu, conn):
    """TPC-H Q3's shape on a few row groups (test_keyset.test_gpu_lineitem_semi_join):
    the build side from a filtered scan, then the aggregate under the set"""
    wl, sf = "lineitem", 0.05
    t = conn.read_image(fl.gen_image(wl, sf))
    try:
        n = t.nrows
        okey = fl.gen_values(wl, C_OKEY, 0, n, np.int64, sf)
        price = fl.gen_values(wl, C_PRICE, 0, n, np.int64, sf)
        ship = fl.gen_values(wl, C_SHIPDATE, 0, n, np.int32, sf)
        cut_key, day = int(okey[n // 3]), 9000
        build = [(C_OKEY, "<", cut_key), (C_SHIPDATE, "<", day)]
        sel = (okey < cut_key) & (ship < day)
        keys = np.unique(okey[sel])
        for form in (0, BITMAP, HASH):
            ks = t.keyset(C_OKEY, build, form=form)
            ref = conn.keyset(keys, form=form)
            assert same_info(fl, ks.info, ref.info)
            bi = ks.build_info
            assert bi.rows_selected == int(sel.sum()) and bi.rowgroups_pruned >= 2
            assert bi.d2h_bytes < 8 * bi.rows_selected                     # the keys never crossed at full width
            assert all(ks.contains(int(k)) for k in keys[:200]) and not ks.contains(int(keys[-1]) + 1)
            mm = np.isin(okey, keys) & (ship >= day)
            got = t.aggregate([("count",), ("sum", C_PRICE)], [(C_OKEY, "in_set", ks), (C_SHIPDATE, ">=", day)])
            assert got == [int(mm.sum()), int(price[mm].sum())] and got[0] > 0
            ks.close()
            ref.close()
    finally:
        t.close()
