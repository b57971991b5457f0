"""Value maps and key maps built on the GPU from a filtered scan
(fls_valuemap_from_scan / fls_keymap_from_scan, Table.valuemap / Table.keymap,
DESIGN.md section 32): the C calls' refusals, the no-device-work cases and the
gate without a GPU; mapbuild_kernel and the two compaction kernels on the GPU
against Connection.valuemap / Connection.keymap over the numpy arrays the test
wrote, through every key type, value width, encoding, NULL pattern, duplicate
distance, filter kind and pipeline shape.

Small shapes throughout, as in test_keyset_build.py: 1024-row row groups, five
whole vectors and a partial tail (2048-row row groups where two vectors of one
row group matter)."""
import ctypes as C

import numpy as np
import pytest

from test_keyset import KEY_TYPES, as_signed, key_pool, type_range
from test_keyset_build import N, RG, fact_cases

M64 = (1 << 64) - 1
ERR_ARG, ERR_LIMIT = -3, -8
DENSE, HASH = 1, 2
I64 = np.iinfo(np.int64)
U64_MAX = (1 << 64) - 1


# ---- helpers of this file
def is_signed(fl, ty):
    return ty in (fl.INT8, fl.INT16, fl.INT32, fl.INT64, fl.DATE, fl.DECIMAL)


def from_scan(fl, t, kc, vc, rg0=0, rg1=None, form=0, keymap=False):
    """the raw C call under the filter currently set: (ValueMap | KeyMap, MapBuildInfo)"""
    h, info = C.c_void_p(), fl.MapBuildInfo()
    call = fl.lib.fls_keymap_from_scan if keymap else fl.lib.fls_valuemap_from_scan
    fl._check(call(t.h, kc, vc, rg0, t.nrowgroups if rg1 is None else rg1, form, C.byref(h), C.byref(info)))
    return (fl.KeyMap if keymap else fl.ValueMap)(h.value, t.conn, info), info


def same_info(a, b):
    return all(getattr(a, n) == getattr(b, n) for n, _ in type(a)._fields_)


def info_diff(a, b):
    return [(n, getattr(a, n), getattr(b, n)) for n, _ in type(a)._fields_ if getattr(a, n) != getattr(b, n)]


def function_of(keys, rng, pool):
    """one value of pool per distinct key: values[i] depends on keys[i] alone"""
    _, inv = np.unique(keys, return_inverse=True)
    pool = np.asarray(pool)
    return pool[rng.integers(0, len(pool), inv.max() + 1 if len(keys) else 0)][inv]


def pin(keys, vals, i, x):
    """the i-th distinct key's value becomes x"""
    vals[keys == np.unique(keys)[i]] = x


def probes_of(keys, pool=None):
    """present, absent and type-edge keys: the pool and its neighbours, 0 / -1 and the 64-bit ends"""
    src = np.unique(keys) if pool is None else pool
    return {int(v) + d for v in src for d in (-1, 0, 1)} | {0, -1, 1, int(I64.min), int(I64.max), U64_MAX}


def check_map(fl, conn, t, kc, vc, keys, vals, sel, m, form=0, pool=None, device=True, info=None, keymap=False,
              downstream=True):
    """the checks of a map key column kc -> value column vc (numpy: keys, vals)
    over the rows sel (bool per row, NULL rows of either column excluded)
    against the reference conn.valuemap / conn.keymap of those pairs"""
    ksg, vsg = is_signed(fl, t.column(kc).type), is_signed(fl, t.column(vc).type)
    if keymap:
        ref = conn.keymap(keys[sel], vals[sel], signed=ksg, form=form)
    else:
        ref = conn.valuemap(keys[sel], vals[sel], signed=ksg, value_signed=vsg, form=form)
    try:
        # 1. the image's description, field for field
        assert same_info(m.info, ref.info), info_diff(m.info, ref.info)
        # 2. every lookup over present, absent and type-edge keys
        for p in probes_of(keys, pool):
            assert m.lookup(p) == ref.lookup(p), p
        # 3. one downstream call gives the same result with either map
        if downstream:
            if keymap:
                got, want = (t.aggregate_grouped([("map", kc, x)], [("count",)]) for x in (m, ref))
            else:
                got, want = (t.aggregate([("count",)], [(vc, "<=", fl.Mapped(kc, x))]) for x in (m, ref))
            assert got == want, (got, want)
        # 4. what the build says of itself
        bi = m.build_info if info is None else info
        if not device:
            assert bi is None
            return
        nkeys = len(np.unique(keys[sel]))
        assert bi is not None and bi.rows_selected == int(sel.sum()), (bi and bi.rows_selected, int(sel.sum()))
        assert bi.keys == nkeys == m.info.count
        if bi.rowgroups_read:
            assert bi.scratch_bytes == 8 * (bi.span + 1)
            assert bi.d2h_bytes >= (bi.span + 64) // 64 * 8 + 8 * nkeys
    finally:
        ref.close()


def check_build(fl, conn, t, kc, vc, keys, vals, sel, filt=None, forms=(0,), keymap=False, **kw):
    for form in forms:
        m = (t.keymap if keymap else t.valuemap)(kc, vc, filt, form=form)
        try:
            check_map(fl, conn, t, kc, vc, keys, vals, sel, m, form=form, keymap=keymap, **kw)
        finally:
            m.close()


@pytest.fixture(scope="module")
def conn(fl):
    c = fl.Connection([0])
    yield c
    c.close()


# ------------------------------------------------------------------ CPU tests
def test_library_exports_the_build_calls(fl):
    assert hasattr(fl.lib, "fls_valuemap_from_scan") and hasattr(fl.lib, "fls_keymap_from_scan")
    assert C.sizeof(fl.MapBuildInfo) == 56


@pytest.fixture(scope="module")
def typed(fl, conn):
    """one column per kind of type the argument checks tell apart (test_keyset_build.typed)"""
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


@pytest.mark.parametrize("name", ["fls_valuemap_from_scan", "fls_keymap_from_scan"])
def test_argument_refusals_come_before_any_device_work(fl, conn, typed, name):
    t = typed
    h, info = C.c_void_p(), fl.MapBuildInfo()
    fn = getattr(fl.lib, name)
    call = lambda *a: fn(*a, C.byref(h), C.byref(info))    # noqa: E731
    nrg = t.nrowgroups
    for side in (0, 1):                                    # the key side, the value side
        pair = lambda c: (c, 0) if side == 0 else (0, c)   # noqa: E731
        assert call(t.h, *pair(t.ncols), 0, nrg, 0) == ERR_ARG and "column 8 out of range" in fl.last_error()
        assert call(t.h, *pair(fl.COL_MAPPED | 1), 0, nrg, 0) == ERR_ARG and "mapped column" in fl.last_error()
        for col in (2, 3, 4, 7):                           # VARCHAR, FLOAT, DOUBLE, BLOB
            assert call(t.h, *pair(col), 0, nrg, 0) == ERR_ARG
            assert f"VARCHAR / BLOB / FLOAT / DOUBLE column ({col})" in fl.last_error()
        assert call(t.h, *pair(6), 0, nrg, 0) == ERR_ARG and "DECIMAL wider than 64 bits (column 6)" in fl.last_error()
    for form in (-1, 3):
        assert call(t.h, 0, 1, 0, nrg, form) == ERR_ARG
        assert f"form {form} (0 auto, 1 dense, 2 hash)" in fl.last_error()
    for rg0, rg1 in ((0, nrg + 1), (2, 1), (nrg + 1, nrg + 2)):
        assert call(t.h, 0, 1, rg0, rg1, 0) == ERR_ARG and "row-group range" in fl.last_error()
        assert name in fl.last_error()
    assert fn(None, 0, 1, 0, nrg, 0, C.byref(h), None) == ERR_ARG
    assert fn(t.h, 0, 1, 0, nrg, 0, None, None) == ERR_ARG
    assert h.value is None
    # the Python calls keep their own refusal
    for col in (2, 3, 4, 7):
        with pytest.raises(ValueError, match="not integer-like"):
            (t.valuemap if "value" in name else t.keymap)(0, col)


def test_no_surviving_row_group_gives_the_empty_map_without_a_gpu(fl, conn, typed):
    t = typed
    for form in (0, DENSE, HASH):
        # every row group pruned by the filter's zone maps
        vm = t.valuemap(0, 1, [(0, ">", 1000)], form=form)
        assert same_info(vm.info, conn.valuemap([], [], value_signed=False, form=form).info) and vm.lookup(0) is None
        bi = vm.build_info
        assert (bi.rows_selected, bi.keys, bi.scratch_bytes, bi.d2h_bytes, bi.rowgroups_read, bi.rowgroups_pruned) == \
            (0, 0, 0, 0, 0, t.nrowgroups)
        km = t.keymap(1, 0, [(0, ">", 1000)], form=form)
        assert same_info(km.info, conn.keymap([], [], signed=False, form=form).info) and km.lookup(0) is None
        assert km.build_info.rowgroups_pruned == t.nrowgroups
        # ... by an empty set, by alternatives none of which may match
        e = conn.keyset([])
        assert t.valuemap(1, 5, [(0, "in_set", e)], form=form).info.count == 0
        assert t.keymap(5, 1, [fl.AnyOf([(0, ">", 1000)], [(1, ">", 1000)])], form=form).info.count == 0
        # an empty range through the C call: the map sits in its registry like any other
        for keymap in (False, True):
            m, bi = from_scan(fl, t, 0, 1, 1, 1, form, keymap=keymap)
            assert (m.info.count, bi.rowgroups_read, bi.rowgroups_pruned, bi.d2h_bytes) == (0, 0, 0, 0)
            m.close()
            assert (fl.lib.fls_keymap_lookup(m.h or 0, 1, None) if keymap else
                    fl.lib.fls_valuemap_lookup(m.h or 0, 1, None)) == ERR_ARG


def test_all_null_key_or_value_chunks_are_skipped_without_a_gpu(fl, conn):
    gone = np.ma.masked_array(np.arange(2 * RG, dtype=np.int64), mask=np.ones(2 * RG, bool))
    full = np.arange(2 * RG, dtype=np.int64)
    t = conn.read_image(fl.write_image([("n", fl.INT64, gone, fl.ENC_AUTO), ("v", fl.INT64, full, fl.ENC_AUTO)],
                                       rowgroup=RG))
    try:
        for kc, vc in ((0, 1), (1, 0)):
            for m in (t.valuemap(kc, vc), t.keymap(kc, vc)):
                assert m.info.count == 0
                assert (m.build_info.rowgroups_read, m.build_info.rowgroups_pruned) == (0, 2)
    finally:
        t.close()


def test_the_gate_refuses_before_any_device_work(fl, conn):
    rng = np.random.default_rng(5)
    wide = rng.integers(0, 1 << 16, N).astype(np.int64)
    wide[7], wide[N - 9] = -5, (1 << 28) - 5                        # the zone maps span exactly 2^28 values + 1
    mid = rng.integers(100, 1 << 16, N).astype(np.int64)
    mid[3], mid[N - 2] = 100, 100 + (1 << 17)                       # ... 2^17 + 1 values: 1 MiB + 8 bytes of slots
    top = rng.integers(-9, 9, N).astype(np.int64)
    top[RG + 5] = I64.max                                           # row group 1's zone map reaches INT64_MAX
    utop = rng.integers(0, 9, N).astype(np.uint64)
    utop[RG + 5] = U64_MAX                                          # ... UINT64_MAX
    near = np.where(top == I64.max, I64.max - 1, top)               # one below: no refusal
    small = rng.integers(0, 500, N).astype(np.int32)
    t = conn.read_image(fl.write_image([("w", fl.INT64, wide, fl.ENC_AUTO), ("m", fl.INT64, mid, fl.ENC_AUTO),
                                        ("top", fl.INT64, top, fl.ENC_AUTO), ("utop", fl.UINT64, utop, fl.ENC_AUTO),
                                        ("near", fl.INT64, near, fl.ENC_AUTO), ("k", fl.INT32, small, fl.ENC_AUTO)],
                                       rowgroup=RG))
    hash_image = 16 << 14                                           # N rows: capacity 2^14
    assert 2 * N <= 1 << 14 < 4 * N
    try:
        h = C.c_void_p()
        for fn in (fl.lib.fls_valuemap_from_scan, fl.lib.fls_keymap_from_scan):
            for form in (0, DENSE, HASH):
                assert fn(t.h, 0, 5, 0, t.nrowgroups, form, C.byref(h), None) == ERR_LIMIT
                msg = fl.last_error()
                assert f"span {(1 << 28) + 1} values" in msg and "kValuemapMaxSpan" in msg, msg
                assert fn(t.h, 1, 5, 0, t.nrowgroups, form, C.byref(h), None) == ERR_LIMIT
                msg = fl.last_error()
                scratch = 8 * ((1 << 17) + 1)                       # above 1 MiB and above the hash image of N rows
                assert scratch > 1 << 20 and scratch > hash_image
                assert f"span {(1 << 17) + 1} values" in msg and f"takes {scratch} bytes" in msg and \
                    f"at most {1 << 20}" in msg and f"the {hash_image} bytes the hash image of {N} rows" in msg, msg
                assert fn(t.h, 5, 2, 0, t.nrowgroups, form, C.byref(h), None) == ERR_LIMIT
                msg = fl.last_error()
                assert f"value column 2 reaches {I64.max} (INT64_MAX) in row group 1" in msg, msg
                assert fn(t.h, 5, 3, 0, t.nrowgroups, form, C.byref(h), None) == ERR_LIMIT
                msg = fl.last_error()
                assert f"value column 3 reaches {U64_MAX} (UINT64_MAX) in row group 1" in msg, msg
            assert h.value is None
            # the same columns in a narrow sub-range pass the gate's checks (and then need the GPU):
            # row group 2 alone spans less than 2^16 keys and holds neither maximum
            lo, hi, _ = t.zonemap(2, 0)
            assert hi - lo < 1 << 16
            for kc, vc in ((0, 5), (1, 5), (5, 2), (5, 3)):
                rc = fn(t.h, kc, vc, 2, 3, 0, C.byref(h), None)
                assert rc not in (ERR_LIMIT, ERR_ARG), fl.last_error()
                if rc == 0:
                    (fl.lib.fls_valuemap_free if fn is fl.lib.fls_valuemap_from_scan else fl.lib.fls_keymap_free)(h)
            # ... and INT64_MAX - 1 is a value like any other
            rc = fn(t.h, 5, 4, 0, t.nrowgroups, 0, C.byref(h), None)
            assert rc != ERR_LIMIT, fl.last_error()
            if rc == 0:
                (fl.lib.fls_valuemap_free if fn is fl.lib.fls_valuemap_from_scan else fl.lib.fls_keymap_free)(h)
    finally:
        t.close()


# ------------------------------------------------------------------ GPU tests
W = 1 << 16


def type_columns(fl, name, rng):
    """[(tag, pool)]: the key columns of one type.  A type whose whole range
    passes the gate draws from key_pool's edge clusters; a wider one gets a
    column per cluster, each confined to a 2^16 window (512 KiB of slots) at
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


VALUE_EDGES = [int(I64.min), int(I64.max) - 1, -1, 0, 1, 1 << 40, -(1 << 40)]


@pytest.fixture(scope="module")
def typetab(fl, conn):
    """per key type its columns, then one INT64 value column per key column: a function of the key"""
    rng = np.random.default_rng(21)
    specs, cols = [], {}
    for name in KEY_TYPES:
        ty = getattr(fl, name)
        for tag, pool in type_columns(fl, name, rng):
            keys = np.array([pool[i] for i in rng.integers(0, len(pool), N)], dtype=object).astype(fl.NP_DTYPE[ty])
            cols.setdefault(name, []).append([len(specs), keys, pool])
            specs.append((f"{name.lower()}_{tag}", ty, keys, fl.ENC_FFOR, *((15, 2) if name == "DECIMAL" else ())))
    for name in KEY_TYPES:
        for ent in cols[name]:
            vals = function_of(ent[1], rng, np.array(VALUE_EDGES + [int(x) for x in rng.integers(-99, 99, 30)], np.int64))
            pin(ent[1], vals, 0, I64.min)
            pin(ent[1], vals, -1, I64.max - 1)
            ent += [len(specs), vals]
            specs.append((f"v{ent[0]}", fl.INT64, vals, fl.ENC_AUTO))
    t = conn.read_image(fl.write_image(specs, rowgroup=RG))
    yield t, cols
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", KEY_TYPES)
def test_gpu_every_key_type(fl, gpu, conn, typetab, name):
    t, cols = typetab
    lo, hi = type_range(fl, name)
    assert len(cols[name]) == (1 if hi - lo < W else 3 if lo < 0 else 2)
    for kc, keys, pool, vc, vals in cols[name]:
        assert lo in pool or hi in pool or -1 in pool                 # every column holds an edge of its type
        assert {int(I64.min), int(I64.max) - 1} <= {int(v) for v in vals}
        check_build(fl, conn, t, kc, vc, keys, vals, np.ones(N, bool), forms=(0, DENSE, HASH), pool=pool)
        # under a filter on the key column itself: the upper half of its pool
        cut = pool[len(pool) // 2]
        check_build(fl, conn, t, kc, vc, keys, vals, keys >= keys.dtype.type(cut), [(kc, ">=", cut)], pool=pool)


@pytest.mark.gpu
def test_gpu_every_value_width_and_sign(fl, gpu, conn):
    """1, 2, 4 and 8-byte signed and unsigned value columns with their types'
    ends (the 8-byte ones: one below the all-ones pattern of their order)"""
    rng = np.random.default_rng(23)
    keys = rng.integers(-300, 300, N).astype(np.int32)
    specs, vals = [("k", fl.INT32, keys, fl.ENC_AUTO)], []
    for name in ("INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "DATE", "BOOLEAN"):
        ty = getattr(fl, name)
        lo, hi = type_range(fl, name)
        top = hi - 1 if name in ("INT64", "UINT64") else hi
        pool = np.array([lo, top, *[int(x) for x in rng.integers(max(lo, -50), min(top, 50) + 1, 20)]],
                        dtype=object).astype(fl.NP_DTYPE[ty])
        v = function_of(keys, rng, pool)
        pin(keys, v, 0, pool[0])
        pin(keys, v, -1, pool[1])
        assert v.min() == pool.min() and v.max() == pool.max()
        vals.append(v)
        specs.append((name.lower(), ty, v, fl.ENC_AUTO))
    t = conn.read_image(fl.write_image(specs, rowgroup=RG))
    try:
        for vc, v in enumerate(vals, start=1):
            check_build(fl, conn, t, 0, vc, keys, v, np.ones(N, bool), forms=(0, HASH))
            check_build(fl, conn, t, 0, vc, keys, v, keys < 0, [(0, "<", 0)])
    finally:
        t.close()


@pytest.mark.gpu
def test_gpu_every_encoding_of_the_key_column(fl, gpu, conn):
    rng = np.random.default_rng(31)
    ffor = rng.integers(-500, 500, N).astype(np.int32)
    delta = (np.cumsum(rng.integers(0, 4, N)) - 4000).astype(np.int64)
    dic = (rng.integers(0, 9, N) * 1003 - 3009).astype(np.int64)
    rle = np.repeat(rng.integers(-20, 20, N // 50 + 1), 50)[:N].astype(np.int16)
    ks = (ffor, delta, dic, rle)
    vs = [function_of(k, rng, np.arange(0, 40, dtype=np.int32)) for k in ks]
    img = fl.write_image([("ffor", fl.INT32, ffor, fl.ENC_FFOR), ("delta", fl.INT64, delta, fl.ENC_DELTA),
                          ("dict", fl.INT64, dic, fl.ENC_DICT), ("rle", fl.INT16, rle, fl.ENC_RLE)] +
                         [(f"v{i}", fl.INT32, v, fl.ENC_AUTO) for i, v in enumerate(vs)], rowgroup=RG)
    from helpers import chunk_encodings
    assert {tuple(r[:4]) for r in chunk_encodings(img.tobytes())} == {(fl.ENC_FFOR, fl.ENC_DELTA, fl.ENC_DICT, fl.ENC_RLE)}
    t = conn.read_image(img)
    try:
        for c, (k, v) in enumerate(zip(ks, vs)):
            check_build(fl, conn, t, c, 4 + c, k, v, np.ones(N, bool), forms=(0, DENSE, HASH))
            check_build(fl, conn, t, c, 4 + c, k, v, ffor < 0, [(0, "<", 0)])
            check_build(fl, conn, t, c, 4 + c, k, v, np.ones(N, bool), keymap=True)
    finally:
        t.close()


@pytest.mark.gpu
def test_gpu_nullable_key_value_and_both(fl, gpu, conn, monkeypatch):
    """a NULL on either side keeps the row out; the placeholder a NULL row
    decodes to (0) is never loaded: as a key it lies outside the column's zone
    maps, as a value it differs from every real one and would be a conflict;
    an all-NULL chunk of either column skips its row group"""
    rng = np.random.default_rng(41)
    k = rng.integers(5000, 9000, N).astype(np.int32)
    v = function_of(k, rng, np.arange(1, 90, dtype=np.int64))          # no real value is the placeholder
    kn, vn = rng.random(N) < 0.3, rng.random(N) < 0.3
    kn[2 * RG:3 * RG] = True                                           # row group 2: the key chunk all NULL
    vn[3 * RG:4 * RG] = True                                           # row group 3: the value chunk all NULL
    kn[4 * RG:5 * RG] = vn[4 * RG:5 * RG] = False                      # row group 4: no validity at all
    grp = rng.integers(0, 5, N).astype(np.int8)
    t = conn.read_image(fl.write_image([("k", fl.INT32, np.ma.masked_array(k, mask=kn), fl.ENC_AUTO),
                                        ("v", fl.INT64, np.ma.masked_array(v, mask=vn), fl.ENC_AUTO),
                                        ("k2", fl.INT32, k, fl.ENC_AUTO), ("v2", fl.INT64, v, fl.ENC_AUTO),
                                        ("g", fl.INT8, grp, fl.ENC_AUTO)], rowgroup=RG))
    try:
        for batch in ("1", "8"):
            monkeypatch.setenv("FLS_SCAN_BATCH", batch)                # 8: one batch mixes chunks with / without validity
            for kc, vc, null, pruned in ((0, 3, kn, 1), (2, 1, vn, 1), (0, 1, kn | vn, 2)):
                vm = t.valuemap(kc, vc)
                check_map(fl, conn, t, kc, vc, k, v, ~null, vm, downstream=False)
                assert vm.lookup(0) is None and vm.build_info.rowgroups_pruned == pruned
                assert as_signed(vm.build_info.base) >= 5000           # the range never reached the placeholder
                vm.close()
                check_build(fl, conn, t, kc, vc, k, v, ~null & (grp == 3), [(4, "=", 3)], downstream=False)
                check_build(fl, conn, t, kc, vc, k, v, ~null & (grp == 3), [(4, "=", 3)], keymap=True, downstream=False)
    finally:
        t.close()


@pytest.mark.gpu
def test_gpu_single_row_partial_vector_and_the_ends_of_the_range(fl, gpu, conn):
    rng = np.random.default_rng(43)
    for n in (1, 63, 64, 65, 1023, 1025, RG + 1):
        k = rng.integers(-40, 40, n).astype(np.int16)
        v = function_of(k, rng, np.arange(0, 50, dtype=np.uint16))
        t = conn.read_image(fl.write_image([("k", fl.INT16, k, fl.ENC_AUTO), ("v", fl.UINT16, v, fl.ENC_AUTO)],
                                           rowgroup=RG))
        try:
            check_build(fl, conn, t, 0, 1, k, v, np.ones(n, bool), forms=(0, HASH))
            check_build(fl, conn, t, 0, 1, k, v, np.ones(n, bool), keymap=True)
            vm = t.valuemap(0, 1)
            bi = vm.build_info                                         # a key at base and one at base + span
            assert as_signed(bi.base) == int(k.min()) and bi.span == int(k.max()) - int(k.min())
            assert vm.lookup(int(k.min())) is not None and vm.lookup(int(k.max())) is not None
            vm.close()
        finally:
            t.close()


# ---- one key twice: the distances that take different paths through the collect kernel
RG2 = 2048
N2 = 3 * RG2 + 100
DISTANCES = {"one 64-row word": (3, 40), "two waves of one block": (3, 300), "two vectors": (3, 1500),
             "two row groups": (3, N2 - 5)}
DUP_KEY = 7771                                                          # inside the other keys' range, none of them


def dup_image(fl, rows, values):
    """unique keys but DUP_KEY at `rows`, with `values` there (and as its codes in a third column)"""
    rng = np.random.default_rng(71)
    k = rng.permutation(np.arange(1000, 1000 + N2, dtype=np.int64) * 3)
    v = (k * 7 - 11).astype(np.int64)
    c = (k % 97).astype(np.int16)
    for r, x in zip(rows, values):
        k[r], v[r], c[r] = DUP_KEY, x, x
    return fl.write_image([("k", fl.INT64, k, fl.ENC_AUTO), ("v", fl.INT64, v, fl.ENC_AUTO),
                           ("c", fl.INT16, c, fl.ENC_AUTO)], rowgroup=RG2), k, v


def assert_conflict(fl, t, key, monkeypatch):
    for keymap in (False, True):
        with pytest.raises(fl.FlsError) as e:
            t.keymap(0, 2) if keymap else t.valuemap(0, 1)
        assert e.value.code == ERR_ARG and f"({key})" in e.value.msg and "a map is a function" in e.value.msg, e.value.msg
    monkeypatch.setenv("FLS_VALUEMAP_BUILD", "host")
    with pytest.raises(fl.FlsError, match="a map is a function"):
        t.valuemap(0, 1)
    monkeypatch.delenv("FLS_VALUEMAP_BUILD")


@pytest.mark.gpu
@pytest.mark.parametrize("where", sorted(DISTANCES))
def test_gpu_one_key_twice_at_every_distance(fl, gpu, conn, where, monkeypatch):
    rows = DISTANCES[where]
    key = DUP_KEY
    # the same value twice: one map, the same as everywhere else
    img, k, v = dup_image(fl, rows, (5, 5))
    t = conn.read_image(img)
    try:
        check_build(fl, conn, t, 0, 1, k, v, np.ones(N2, bool), forms=(0, HASH))
        vm = t.valuemap(0, 1)
        assert vm.lookup(key) == 5 and vm.build_info.keys == N2 - 1 and vm.build_info.rows_selected == N2
        vm.close()
    finally:
        t.close()
    # two values: no function, on both routes
    img, k, v = dup_image(fl, rows, (5, 6))
    t = conn.read_image(img)
    try:
        assert_conflict(fl, t, key, monkeypatch)
        # ... unless the filter keeps only one of the two rows
        check_build(fl, conn, t, 0, 1, k, v, v != 6, [(1, "!=", 6)])
    finally:
        t.close()


@pytest.mark.gpu
def test_gpu_duplicates_across_batches_slots_and_gpus(fl, gpu, conn, monkeypatch):
    key = DUP_KEY
    same = {w: dup_image(fl, DISTANCES[w], (5, 5)) for w in ("two vectors", "two row groups")}
    diff = {w: dup_image(fl, DISTANCES[w], (5, 6)) for w in ("two vectors", "two row groups")}
    infos = []

    def run(call):
        for w in same:
            img, k, v = same[w]
            t = call.read_image(img)
            check_build(fl, call, t, 0, 1, k, v, np.ones(N2, bool), downstream=False)
            vm = t.valuemap(0, 1)
            infos.append((w, vm.build_info.keys, [getattr(vm.info, n) for n, _ in fl.ValueMapInfo._fields_]))
            vm.close()
            t.close()
            t = call.read_image(diff[w][0])
            assert_conflict(fl, t, key, monkeypatch)
            t.close()

    for batch, slots in (("1", "1"), ("3", "2"), ("2", "3")):
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)
        monkeypatch.setenv("FLS_SCAN_SLOTS", slots)
        run(conn)
    monkeypatch.delenv("FLS_SCAN_BATCH")
    monkeypatch.delenv("FLS_SCAN_SLOTS")
    # every visible GPU (the two rows on two of them), and one GPU listed twice (two pipelines share its array)
    for devs in (list(range(gpu)), [0, 0]):
        call = fl.Connection(devs)
        try:
            run(call)
            img, k, v = same["two row groups"]
            t = call.read_image(img)
            vm = t.valuemap(0, 1)
            bi = vm.build_info
            assert bi.d2h_bytes >= min(len(set(devs)), t.nrowgroups) * ((bi.span + 64) // 64 * 8) + 8 * bi.keys
            vm.close()
            t.close()
        finally:
            call.close()
    # the map and build_info.keys are identical across all of those
    for w in same:
        assert len({repr(x[1:]) for x in infos if x[0] == w}) == 1, infos
    assert {x[1] for x in infos} == {N2 - 1}


@pytest.mark.gpu
def test_gpu_two_conflicting_keys_and_a_three_valued_key(fl, gpu, conn):
    rng = np.random.default_rng(73)
    k = rng.permutation(np.arange(N, dtype=np.int64) * 2 + 100)
    v = (k + 1).astype(np.int64)
    # two keys with two values each, in different row groups
    k2, v2 = k.copy(), v.copy()
    k2[[10, RG + 10]], v2[[10, RG + 10]] = 5001, (1, 2)
    k2[[3 * RG + 1, 4 * RG + 1]], v2[[3 * RG + 1, 4 * RG + 1]] = 7001, (3, 4)
    # one key listed a, b, a
    k3, v3 = k.copy(), v.copy()
    k3[[20, 700, 2 * RG + 20]], v3[[20, 700, 2 * RG + 20]] = 6001, (8, 9, 8)
    t = conn.read_image(fl.write_image([("k2", fl.INT64, k2, fl.ENC_AUTO), ("v2", fl.INT64, v2, fl.ENC_AUTO),
                                        ("k3", fl.INT64, k3, fl.ENC_AUTO), ("v3", fl.INT64, v3, fl.ENC_AUTO)], rowgroup=RG))
    try:
        with pytest.raises(fl.FlsError) as e:
            t.valuemap(0, 1)
        assert e.value.code == ERR_ARG and ("(5001)" in e.value.msg or "(7001)" in e.value.msg), e.value.msg
        assert "a map is a function" in e.value.msg
        with pytest.raises(fl.FlsError) as e:
            t.valuemap(2, 3)
        assert e.value.code == ERR_ARG and "(6001)" in e.value.msg and "a map is a function" in e.value.msg, e.value.msg
        # without the odd one out it is a map again
        check_build(fl, conn, t, 2, 3, k3, v3, v3 != 9, [(3, "!=", 9)])
    finally:
        t.close()


@pytest.fixture(scope="module")
def maptab(fl, conn):
    """test_keyset_build.facttab's columns, then a value that is a function of the key and a code of it"""
    rng = np.random.default_rng(61)
    key = np.sort(rng.integers(0, 4000, N)).astype(np.int64)
    grp = rng.integers(0, 5, N).astype(np.int8)
    qty = rng.integers(1, 51, N).astype(np.int32)
    nm = rng.random(N) < 0.2
    a = rng.integers(0, 100, N).astype(np.int32)
    b = rng.integers(0, 100, N).astype(np.int32)
    words = [b"abacus", b"abbey", b"cab", b"about", b"zebra", b"ab", b"", b"lab coat"]
    s = [words[i] for i in rng.integers(0, len(words), N)]
    val = (key * 31 - 60000).astype(np.int64)
    code = (key % 25).astype(np.int16)
    t = conn.read_image(fl.write_image([("key", fl.INT64, key, fl.ENC_AUTO), ("grp", fl.INT8, grp, fl.ENC_AUTO),
                                        ("qty", fl.INT32, np.ma.masked_array(qty, mask=nm), fl.ENC_AUTO),
                                        ("a", fl.INT32, a, fl.ENC_AUTO), ("b", fl.INT32, b, fl.ENC_AUTO),
                                        ("s", fl.VARCHAR, s, fl.ENC_DICT), ("val", fl.INT64, val, fl.ENC_AUTO),
                                        ("code", fl.INT16, code, fl.ENC_AUTO)], rowgroup=RG))
    yield t, {"key": key, "grp": grp, "qty": qty, "nm": nm, "a": a, "b": b, "s": s, "val": val, "code": code}
    t.close()


@pytest.mark.gpu
def test_gpu_build_under_every_kind_of_filter(fl, gpu, conn, maptab):
    t, c = maptab
    cases = fact_cases(fl, conn, c)
    assert any(isinstance(x, fl.AnyOf) for _, filt, _ in cases for x in filt)
    for what, filt, m in cases:
        assert m.any() or what.startswith("nothing"), what
        check_build(fl, conn, t, 0, 6, c["key"], c["val"], m, filt)
        check_build(fl, conn, t, 0, 7, c["key"], c["code"], m, filt, keymap=True)
        # ... and the filter leaves nothing behind on the table
        assert sum(len(sel) for _, _, sel, _ in t.scan_filtered([], cols=[1])) == N


@pytest.mark.gpu
def test_gpu_rowgroup_subrange_through_the_c_call(fl, gpu, conn, maptab):
    t, c = maptab
    for rg0, rg1 in ((1, 3), (0, 1), (5, 6), (2, 6)):
        rows = np.zeros(N, bool)
        rows[rg0 * RG:rg1 * RG] = True
        for filt, m in (([], rows), ([(1, "=", 1)], rows & (c["grp"] == 1))):
            for keymap, vc, vals in ((False, 6, c["val"]), (True, 7, c["code"])):
                t.set_filter(filt)
                try:
                    mp, info = from_scan(fl, t, 0, vc, rg0, rg1, keymap=keymap)
                finally:
                    t.set_filter([])
                check_map(fl, conn, t, 0, vc, c["key"], vals, m, mp, info=info, keymap=keymap)
                assert info.rowgroups_read == rg1 - rg0 and info.rowgroups_pruned == 0
                # the range is the union of the read row groups' zone maps
                zs = [t.zonemap(r, 0) for r in range(rg0, rg1)]
                assert as_signed(info.base) == min(z[0] for z in zs)
                assert info.span == max(z[1] for z in zs) - as_signed(info.base)
                mp.close()


@pytest.mark.gpu
def test_gpu_keymap_values_at_and_past_the_ends_of_the_codes(fl, gpu, conn, monkeypatch):
    rng = np.random.default_rng(81)
    k = rng.permutation(np.arange(N, dtype=np.int32))
    ok = (k % 7).astype(np.int32)
    ok[5], ok[N - 5] = 0, 65534                                         # both ends are codes
    big, neg, both = ok.copy(), ok.copy(), ok.copy()
    big[RG + 1] = 65535
    neg[2 * RG + 1] = -1
    both[RG + 1], both[2 * RG + 1], both[9] = 70000, -1, -3             # the minimum when negative
    ubig = big.astype(np.uint32)
    clash = both.copy()                                                 # ... and a key with two values as well:
    kk = k.copy()                                                       # the value's range is still what is named
    kk[4 * RG + 1], clash[4 * RG + 1] = kk[7], clash[7] + 1
    t = conn.read_image(fl.write_image([("k", fl.INT32, k, fl.ENC_AUTO), ("ok", fl.INT32, ok, fl.ENC_AUTO),
                                        ("big", fl.INT32, big, fl.ENC_AUTO), ("neg", fl.INT32, neg, fl.ENC_AUTO),
                                        ("both", fl.INT32, both, fl.ENC_AUTO), ("ubig", fl.UINT32, ubig, fl.ENC_AUTO),
                                        ("kk", fl.INT32, kk, fl.ENC_AUTO), ("clash", fl.INT32, clash, fl.ENC_AUTO)],
                                       rowgroup=RG))
    try:
        check_build(fl, conn, t, 0, 1, k, ok, np.ones(N, bool), forms=(0, DENSE, HASH), keymap=True)
        km = t.keymap(0, 1)
        assert km.lookup(int(k[5])) == 0 and km.lookup(int(k[N - 5])) == 65534 and km.info.max_code == 65534
        for route in ("device", "host"):
            if route == "host":
                monkeypatch.setenv("FLS_KEYMAP_BUILD", "host")
            for vc, bad in ((2, 65535), (3, -1), (4, -3), (5, 65535), (7, -3)):
                with pytest.raises(ValueError) as e:
                    t.keymap(6 if vc == 7 else 0, vc)
                assert str(e.value) == f"keymap: value {bad} of column {vc} is outside [0, 65534]", (route, str(e.value))
            # the filter takes the value away: a map again
            check_build(fl, conn, t, 0, 2, k, big, big != 65535, [(2, "<", 65535)], keymap=True, device=route == "device")
        # the C call names the value too
        h = C.c_void_p()
        assert fl.lib.fls_keymap_from_scan(t.h, 0, 4, 0, t.nrowgroups, 0, C.byref(h), None) == ERR_ARG
        assert "value -3 of column 4 is outside [0, 65534]" in fl.last_error() and h.value is None
    finally:
        t.close()


@pytest.mark.gpu
def test_gpu_host_route_and_gated_out_columns_equal_the_device_route(fl, gpu, conn, maptab, monkeypatch):
    t, c = maptab
    filt, m = [(1, "!=", 2), (2, ">", 10)], (c["grp"] != 2) & ~c["nm"] & (c["qty"] > 10)
    dev_v, dev_k = t.valuemap(0, 6, filt), t.keymap(0, 7, filt)
    monkeypatch.setenv("FLS_VALUEMAP_BUILD", "host")
    monkeypatch.setenv("FLS_KEYMAP_BUILD", "host")
    host_v, host_k = t.valuemap(0, 6, filt), t.keymap(0, 7, filt)
    assert dev_v.build_info is not None and host_v.build_info is None and same_info(dev_v.info, host_v.info)
    assert dev_k.build_info is not None and host_k.build_info is None and same_info(dev_k.info, host_k.info)
    check_map(fl, conn, t, 0, 6, c["key"], c["val"], m, host_v, device=False)
    check_map(fl, conn, t, 0, 7, c["key"], c["code"], m, host_k, device=False, keymap=True)
    monkeypatch.delenv("FLS_VALUEMAP_BUILD")
    monkeypatch.delenv("FLS_KEYMAP_BUILD")
    # columns the gate refuses: a key column whose zone maps span 2^40 values, a value column that holds INT64_MAX
    rng = np.random.default_rng(64)
    wide = (rng.integers(0, 50, N) * ((1 << 40) // 49) - (1 << 39)).astype(np.int64)
    wv = (wide // 1000).astype(np.int64)
    top = np.where(c["key"] == c["key"][77], I64.max, c["val"]).astype(np.int64)
    code = (wide % 23).astype(np.int16)
    tw = conn.read_image(fl.write_image([("w", fl.INT64, wide, fl.ENC_AUTO), ("wv", fl.INT64, wv, fl.ENC_AUTO),
                                         ("g", fl.INT8, c["grp"], fl.ENC_AUTO), ("key", fl.INT64, c["key"], fl.ENC_AUTO),
                                         ("top", fl.INT64, top, fl.ENC_AUTO), ("code", fl.INT16, code, fl.ENC_AUTO)],
                                        rowgroup=RG))
    try:
        check_build(fl, conn, tw, 0, 1, wide, wv, np.ones(N, bool), forms=(0, HASH), device=False)
        check_build(fl, conn, tw, 0, 1, wide, wv, c["grp"] == 0, [(2, "=", 0)], device=False)
        check_build(fl, conn, tw, 0, 5, wide, code, np.ones(N, bool), device=False, keymap=True)
        check_build(fl, conn, tw, 3, 4, c["key"], top, np.ones(N, bool), device=False)
        vm = tw.valuemap(3, 4)
        assert vm.lookup(int(c["key"][77])) == I64.max
        vm.close()
    finally:
        tw.close()


@pytest.mark.gpu
def test_gpu_accounting_of_a_sparse_map(fl, gpu, conn):
    """every 64th key of the range: the host receives a presence word and a
    value per key and the counts, never the array"""
    n = 2000
    rng = np.random.default_rng(91)
    k = rng.permutation(np.arange(n, dtype=np.int64) * 64 + 12345)
    v = (k // 64).astype(np.int64)
    half = rng.random(n) < 0.5
    t = conn.read_image(fl.write_image([("k", fl.INT64, k, fl.ENC_AUTO), ("v", fl.INT64, v, fl.ENC_AUTO),
                                        ("h", fl.INT8, half.astype(np.int8), fl.ENC_AUTO)], rowgroup=RG))
    try:
        for filt, sel in (([], np.ones(n, bool)), ([(2, "=", 1)], half)):
            vm = t.valuemap(0, 1, filt)
            check_map(fl, conn, t, 0, 1, k, v, sel, vm)
            bi = vm.build_info
            assert bi.rows_selected == int(sel.sum()) == bi.keys
            assert bi.scratch_bytes == 8 * (bi.span + 1) and bi.span == 64 * (n - 1)
            assert (bi.span + 64) // 64 * 8 + 8 * bi.keys <= bi.d2h_bytes < bi.scratch_bytes
            vm.close()
    finally:
        t.close()
