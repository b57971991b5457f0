"""Key-map group keys (GROUP BY a joined dimension attribute, DESIGN.md section
22): the host construction (csrc/fls_keymap.hpp through fls_keymap_*), the
argument checks of the bindings and of mapped keys, the row-group pruning --
all without a GPU -- and keymap_kernel on the GPU through
Table.aggregate_grouped against a dict / numpy restatement written here.

Small shapes throughout: 1024-row row groups, five whole vectors and a partial
tail, maps from 0 to a few thousand keys."""
import ctypes as C
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import chunk_encodings, filter_mask, rand64
from test_keyset import KEY_TYPES, as_signed, colliding_keys, key_pool, type_range

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "duckdb-fastlane_amd" / "csrc"
LIB = ROOT / "duckdb-fastlane_amd" / "libflsgpu.so"
RG = 1024
N = 5 * 1024 + 333
M64 = (1 << 64) - 1
HASH_MUL = 0x9E3779B97F4A7C15
ERR_ARG, ERR_DEVICE, ERR_LIMIT = -3, -4, -8
DENSE, HASH = 1, 2
KEEP = "keep_unmatched"


# ---- helpers of this file
class M:
    """a key map and the dict it was made of (the Python side of a mapped key)"""

    def __init__(self, conn, d, signed=True, form=0):
        self.d = {int(k): int(v) for k, v in dict(d).items()}
        self.km = conn.keymap(list(self.d), list(self.d.values()), signed=signed, form=form)


def eng_keys(keys):
    """the keys as the engine takes them: M -> its KeyMap"""
    return [(k[0], k[1], k[2].km, *k[3:]) if isinstance(k, tuple) else k for k in keys]


def py_key(x):
    return x if x is None or isinstance(x, bytes) else int(x)


def want_groups(keys, cols, valid, sel):
    """[(key tuple, row mask)] in order of each key's first selected row.  A
    key is a column or ("map", col, M[, KEEP]): the code M gives the column's
    value; a NULL or unmatched row is dropped (inner) or carries None (KEEP).
    The value stored at a NULL row is never looked at."""
    rows = {}
    for i in np.nonzero(sel)[0]:
        key = []
        for spec in keys:
            c = spec[1] if isinstance(spec, tuple) else spec
            ok = valid.get(c)
            null = ok is not None and not ok[i]
            if not isinstance(spec, tuple):
                key.append(None if null else py_key(cols[c][i]))
                continue
            code = None if null else spec[2].d.get(int(cols[c][i]))
            if code is None and len(spec) == 3:
                key = None
                break
            key.append(code)
        if key is not None:
            rows.setdefault(tuple(key), []).append(i)
    out = []
    for k, r in rows.items():
        m = np.zeros(len(sel), bool)
        m[r] = True
        out.append((k, m))
    return out


def want_aggs(aggs, cols, valid, m):
    """the aggregates over the rows of m, in exact Python integers"""
    every = np.ones(len(m), bool)
    out = []
    for a in aggs:
        if len(a) == 1:
            out.append(int(m.sum()))
        elif a[0] == "sum_expr":
            mm = m.copy()
            for _, _, c in a[1]:
                mm &= valid.get(c, every)
            tot = 0
            for i in np.nonzero(mm)[0]:
                p = 1
                for k, s, c in a[1]:
                    p *= k + s * int(cols[c][i])
                tot += p
            out.append(tot if mm.any() else None)
        else:
            mm = m & valid.get(a[1], every)
            vals = [int(v) for v in cols[a[1]][mm]]
            out.append(len(vals) if a[0] == "count" else None if not vals else
                       {"sum": sum, "min": min, "max": max}[a[0]](vals))
    return out


def check_grouped(t, keys, aggs, cols, valid=None, filt=None, sel=None, what="", **kw):
    """aggregate_grouped against the restatement: the groups, their order and
    every value; returns the engine's result"""
    valid = valid or {}
    if sel is None:
        sel = filter_mask(cols, filt, t.nrows, valid) if filt else np.ones(t.nrows, bool)
    got = t.aggregate_grouped(eng_keys(keys), aggs, filt=filt, **kw)
    want = want_groups(keys, cols, valid, sel)
    assert [g[0] for g in got] == [w[0] for w in want], (what, [g[0] for g in got][:8], [w[0] for w in want][:8])
    for (key, vals), (_, m) in zip(got, want):
        assert vals == want_aggs(aggs, cols, valid, m), (what, key)
    return got


def bits(x):
    return None if x is None else (int(np.array([x], dtype=np.float64).view(np.uint64)[0]) if isinstance(x, float) else x)


def as_bits(res):
    return [(k, [bits(v) for v in vals]) for k, vals in res]


@pytest.fixture(scope="module")
def conn(fl):
    c = fl.Connection([0])
    yield c
    c.close()


# ------------------------------------------------------------------ CPU tests
def test_library_exports_the_keymap_functions(fl):
    for name in ("fls_keymap_create", "fls_keymap_free", "fls_keymap_info", "fls_keymap_lookup",
                 "fls_aggregate_key_bindings"):
        assert hasattr(fl.lib, name), name
    assert fl.KEY_MAPPED == 0x80000000 and fl.KEYMAP_KEEP_UNMATCHED == 1 and fl.KEYMAP_ABSENT == 0xFFFF


@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("form", [0, DENSE, HASH])
def test_lookup_equals_a_python_dict(fl, conn, signed, form):
    rng = np.random.default_rng(3 + form)
    lo, hi = (-(1 << 63), (1 << 63) - 1) if signed else (0, M64)
    edge = [0, -1 if signed else M64, (M64 - 1) if not signed else -2, lo, hi]
    sets = [
        [int(x) for x in rng.integers(-3000, 3000, 2000)] if signed else [int(x) for x in rng.integers(0, 6000, 2000)],
        [lo + int(x) for x in rng.integers(0, 5000, 700)],                      # near the type's minimum
        [hi - int(x) for x in rng.integers(0, 5000, 700)],                      # every early sentinel candidate
        [hi - i for i in range(40)],                                            # ~0, ~0 - 1, ... taken (unsigned)
        [-1 - i for i in range(40)] if signed else [0],                         # ... and as signed keys
        [lo, lo + 2, lo + 9],                                                   # holes in a dense array
    ]
    if form != DENSE:                                                           # wider than a dense map may be
        sets += [edge, [hi - i for i in range(40)] + [lo],
                 [int(x) - (1 << 63 if signed else 0) for x in rand64(rng, 3000)]]
    for keys in sets:
        ref = {k & M64: (int(k) * 31 + 7) % 65535 for k in keys}               # codes over the whole range, 65534 included
        ref[keys[0] & M64] = 65534
        ref[keys[-1] & M64] = 0
        m = conn.keymap(list(ref), list(ref.values()), signed=signed, form=form)
        info = m.info
        assert info.count == len(ref) and info.max_code == max(ref.values())
        assert info.kind == (0 if signed else 1) and (form == 0 or info.form == form)
        if info.form == HASH:
            assert info.empty not in ref and all(e in ref for e in range(M64, info.empty, -1))
        probes = set(edge) | {k + d for k in keys[:300] for d in (-1, 0, 1)} | {int(x) for x in rand64(rng, 200)}
        probes |= {info.empty, info.min - 1, info.max + 1}                      # one outside [min, max]
        for p in probes:
            assert m.lookup(p) == ref.get(p & M64), (form, signed, p)
        assert all(m.lookup(k) == v for k, v in ref.items())
        m.close()


def test_duplicates_conflicts_and_the_reserved_code(fl, conn):
    for form in (0, DENSE, HASH):
        m = conn.keymap([5, 1, 1, -1, 7, 7, 7], [3, 2, 2, 0, 65534, 65534, 65534], form=form)
        assert m.info.count == 4 and m.info.max_code == 65534                   # an equal duplicate is kept once
        assert [m.lookup(k) for k in (5, 1, -1, 7, 0, 6)] == [3, 2, 0, 65534, None, None]
        with pytest.raises(fl.FlsError, match=r"key 0x7 \(7\) is listed with the values 4 and 9") as e:
            conn.keymap([5, 7, 1, 7], [3, 9, 2, 4], form=form)                  # a map is a function
        assert e.value.code == ERR_ARG
        with pytest.raises(fl.FlsError, match=r"key 0xf+ \(-1\) .*values 1 and 2"):
            conn.keymap([-1, -1], [2, 1], form=form)
        with pytest.raises(fl.FlsError, match="65535") as e:
            conn.keymap([1, 2], [0, 65535], form=form)
        assert e.value.code == ERR_ARG
    for bad in ([65536], [-1], [1 << 40]):
        with pytest.raises(ValueError, match="outside"):
            conn.keymap([1], bad)
    with pytest.raises(ValueError, match="2 keys and 1 values"):
        conn.keymap([1, 2], [1])
    for bad in ([1.5], ["3"], [None]):                                          # a float is never truncated into a key
        with pytest.raises(TypeError, match="keymap"):
            conn.keymap(bad, [1])
    hsh = conn.keymap([5, 1, -1, 7, 1 << 40], [1, 2, 3, 4, 5], form=HASH).info
    assert (hsh.count, hsh.form, hsh.capacity, hsh.device_bytes) == (5, HASH, 16, 8 * 16 + 2 * 16)
    assert as_signed(hsh.min) == -1 and hsh.max == 1 << 40 and 1 <= hsh.max_probe <= 5 and hsh.empty == M64 - 1
    den = conn.keymap([5, 1, -1, 7], [1, 2, 3, 4], form=DENSE).info
    assert (den.count, den.form, den.capacity, den.max_probe, den.device_bytes) == (4, DENSE, 0, 0, 24)  # 9 codes, padded
    for form in (0, DENSE, HASH):
        e = conn.keymap([], [], form=form)
        assert e.info.count == 0 and e.lookup(0) is None and e.lookup(-1) is None and (form == 0 or e.info.form == form)


def test_the_map_does_not_depend_on_input_order(fl, conn):
    """info and every lookup here; the image's bytes in tests/fuzz/fuzz_keymap.cpp"""
    rng = np.random.default_rng(5)
    keys = [int(x) for x in np.unique(rng.integers(-4000, 4000, 1500))]
    vals = [k % 23 for k in keys]
    for form in (DENSE, HASH):
        a = conn.keymap(keys, vals, form=form)
        p = rng.permutation(len(keys))
        b = conn.keymap([keys[i] for i in p] + keys[:50], [vals[i] for i in p] + vals[:50], form=form)
        assert bytes(a.info) == bytes(b.info)
        assert all(a.lookup(k) == b.lookup(k) == v for k, v in zip(keys, vals))


def test_auto_rule_at_its_boundaries(fl, conn):
    """auto takes the dense array (2 bytes per value of [min, max], padded to
    8) when it is no larger than the hash image would be (10 bytes per slot),
    or at most 1 MiB: one key moved by one on either side of each bound"""
    # 3 keys: an 80-byte hash image (8 slots); the array over 2^19 values is exactly 1 MiB
    at = conn.keymap([10, 11, 10 + (1 << 19) - 1], [1, 2, 3]).info
    assert (at.form, at.device_bytes) == (DENSE, 1 << 20)
    past = conn.keymap([10, 11, 10 + (1 << 19)], [1, 2, 3]).info
    assert (past.form, past.device_bytes, past.capacity) == (HASH, 80, 8)
    # 2^17 + 1 keys: 2^19 slots, a 5 MiB hash image; the array over 5 * 2^19 values is exactly 5 MiB
    n = (1 << 17) + 1
    base = np.arange(n - 1, dtype=np.int64) - 1000
    codes = (np.arange(n) % 25).astype(np.uint16)
    at = conn.keymap(np.append(base, -1000 + 5 * (1 << 19) - 1), codes).info
    assert (at.count, at.form, at.device_bytes) == (n, DENSE, 5 << 20)
    past = conn.keymap(np.append(base, -1000 + 5 * (1 << 19)), codes).info
    assert (past.count, past.form, past.device_bytes, past.capacity) == (n, HASH, 5 << 20, 1 << 19)
    # past 2^31 values auto cannot take the array (test_limits: forcing it is FLS_ERR_LIMIT)
    assert conn.keymap([0, 1 << 31], [1, 2]).info.form == HASH


def test_limits(fl, conn):
    h = C.c_void_p()
    one_k, one_v = (C.c_uint64 * 1)(1), (C.c_uint16 * 1)(1)
    with pytest.raises(fl.FlsError) as e:                                        # n is checked before the buffers are read
        fl._check(fl.lib.fls_keymap_create(conn.h, one_k, one_v, fl.MAX_KEYSET_KEYS + 1, 0, 0, C.byref(h)))
    assert e.value.code == ERR_LIMIT and "kMaxKeysetKeys" in str(e.value)
    with pytest.raises(fl.FlsError) as e:                                        # span + 1 = 2^31 + 1, two keys
        conn.keymap([0, 1 << 31], [1, 2], form=DENSE)
    assert e.value.code == ERR_LIMIT and "2^31" in str(e.value)
    with pytest.raises(fl.FlsError) as e:
        conn.keymap([-5, (1 << 31) - 5], [1, 2], form=DENSE)
    assert e.value.code == ERR_LIMIT
    with pytest.raises(fl.FlsError) as e:
        conn.keymap([1], [1], form=3)
    assert e.value.code == ERR_ARG


@pytest.mark.parametrize("home", [5, 127])
def test_colliding_keys_probe_as_long_as_the_map(fl, conn, home):
    """50 keys sharing one home slot of the 128-slot table (built from the
    documented hash): the longest probe is their number, every one is found
    with its own code; home 127 wraps past the end of the table"""
    keys = colliding_keys(50, 7, home)
    assert len(set(keys)) == 50 and all(((k * HASH_MUL) & M64) >> 57 == home for k in keys)
    m = conn.keymap(keys, [j * 1000 for j in range(50)], signed=False, form=HASH)
    assert (m.info.capacity, m.info.max_probe, m.info.device_bytes) == (128, 50, 1280)
    assert [m.lookup(k) for k in keys] == [j * 1000 for j in range(50)]
    others = colliding_keys(80, 7, home)[50:]                                    # same home, not in the map
    assert all(m.lookup(k) is None for k in others) and m.lookup(m.info.empty) is None


@pytest.fixture(scope="module")
def typed(fl, conn):
    """one column per kind of type the argument checks tell apart"""
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


def test_argument_errors_name_the_binding_or_the_key_before_any_device_work(fl, conn, typed):
    t = typed
    sg, us = conn.keymap([1, 2, 3], [0, 1, 2]), conn.keymap([1, 2, 3], [0, 1, 2], signed=False)
    cnt = [("count",)]

    def refused(bindings, pattern):
        with pytest.raises(fl.FlsError, match=pattern) as e:
            t.set_key_bindings(bindings)
        assert e.value.code == ERR_ARG

    refused([(0, sg)] * 5, r"5 bindings \(at most 4\)")
    refused([(0, sg), (99, sg)], r"binding 1: column 99 out of range")
    for col in (2, 3, 4, 7):                                                     # VARCHAR, FLOAT, DOUBLE, BLOB
        refused([(0, sg), (1, us), (col, sg)], r"binding 2: .*VARCHAR / BLOB / FLOAT / DOUBLE")
    refused([(6, sg)], r"binding 0: .*DECIMAL wider than 64 bits \(column 6\)")    # DECIMAL(20, 2)
    refused([(0, us)], r"binding 0: the key map's kind is unsigned, column 0 is signed")
    refused([(0, sg), (1, sg)], r"binding 1: the key map's kind is signed, column 1 is unsigned")
    refused([(0, sg, 2)], r"binding 0: unknown flag bits 0x2")
    refused([(0, sg, 1), (0, sg, 0x80000001)], r"binding 1: unknown flag bits")
    refused([(0, sg), (0, 0xDEADBEEF)], r"binding 1: .*not a live key map")
    # through aggregate_grouped's key tuples: the same checks, the bindings cleared afterwards
    with pytest.raises(fl.FlsError, match=r"binding 1: .*VARCHAR") as e:
        t.aggregate_grouped([("map", 0, sg), ("map", 2, sg)], cnt)
    assert e.value.code == ERR_ARG
    with pytest.raises(ValueError, match="keep_unmatched"):
        t.aggregate_grouped([("map", 0, sg, "left")], cnt)
    # mapped keys of the grouped call
    with pytest.raises(fl.FlsError, match=r"key 0: no binding 0") as e:
        t.aggregate_grouped([fl.KEY_MAPPED | 0], cnt)
    assert e.value.code == ERR_ARG
    t.set_key_bindings([(0, sg), (5, sg, fl.KEYMAP_KEEP_UNMATCHED)])            # a DECIMAL of at most 64 bits is accepted
    try:
        with pytest.raises(fl.FlsError, match=r"key 1: no binding 2") as e:
            t.aggregate_grouped([0, fl.KEY_MAPPED | 2], cnt)
        assert e.value.code == ERR_ARG
        with pytest.raises(fl.FlsError, match=r"key 2: binding 1 is key 0 already") as e:
            t.aggregate_grouped([fl.KEY_MAPPED | 1, fl.KEY_MAPPED | 0, fl.KEY_MAPPED | 1], cnt)
        assert e.value.code == ERR_ARG
        with pytest.raises(fl.FlsError, match=r"key 1: column 99 out of range"):  # a plain key keeps its message
            t.aggregate_grouped([fl.KEY_MAPPED | 0, 99], cnt)
        with pytest.raises(fl.FlsError, match=r"5 keys \(1 to 4 per call\)"):     # a mapped key counts towards the four
            t.aggregate_grouped([fl.KEY_MAPPED | 0, fl.KEY_MAPPED | 1, 0, 1, 5], cnt)
        with pytest.raises(fl.FlsError, match=r"key 3: the packed key needs 132 bits"):  # 16 + 64 + 16 + 32 and 4 NULL bits
            t.aggregate_grouped([fl.KEY_MAPPED | 0, 5, fl.KEY_MAPPED | 1, 0], cnt)
    finally:
        t.set_key_bindings(None)
    with pytest.raises(fl.FlsError, match=r"key 0: no binding 0"):               # cleared
        t.aggregate_grouped([fl.KEY_MAPPED | 0], cnt)


def test_stale_keyset_and_garbage_handles_are_refused(fl, conn, typed):
    t = typed
    km = conn.keymap([1, 2, 3], [0, 1, 2])
    ks = conn.keyset([1, 2, 3])
    h = km.h
    t.set_key_bindings([(0, km)])
    t.set_key_bindings(None)
    km.close()
    km.close()                                                                   # idempotent
    for value in (h, ks.h, 0, 1, 0xDEADBEEF, id(t), M64):                        # stale, a key set's, garbage
        with pytest.raises(fl.FlsError, match="binding 0: .*not a live key map") as e:
            t.set_key_bindings([(0, value)])
        assert e.value.code == ERR_ARG
    fl.lib.fls_keymap_free(h)                                                    # a stale free is a no-op
    fl.lib.fls_keymap_free(ks.h)                                                 # ... and a key set is no map
    assert ks.contains(2)
    code = C.c_uint32()
    assert fl.lib.fls_keymap_lookup(h, 1, C.byref(code)) == ERR_ARG
    assert fl.lib.fls_keymap_lookup(ks.h, 1, C.byref(code)) == ERR_ARG
    assert fl.lib.fls_keymap_info(0xDEADBEEF, C.byref(fl.KeyMapInfo())) == ERR_ARG
    # a map handle is no key set either
    k2 = conn.keymap([1], [1])
    with pytest.raises(fl.FlsError, match="not a live key set"):
        t.set_filter([(0, "in_set", k2.h)])
    assert fl.lib.fls_keyset_contains(k2.h, 1) == ERR_ARG
    # the maps of a closed connection are gone with it
    c2 = fl.Connection([0])
    k3 = c2.keymap([1], [1])
    c2.close()
    with pytest.raises(fl.FlsError, match="not a live key map"):
        t.set_key_bindings([(0, k3.h)])
    k3.h = None


@pytest.fixture(scope="module")
def prunetab(fl, conn):
    """column 0 sorted INT64, column 1 the same values shuffled, column 2
    nullable with an all-NULL third row group"""
    rng = np.random.default_rng(2)
    srt = np.cumsum(rng.integers(1, 9, N)).astype(np.int64) - 9000
    shf = rng.permutation(srt)
    null = np.zeros(N, bool)
    null[2 * RG:3 * RG] = True
    null[rng.choice(N, 200, replace=False)] = True
    nul = np.ma.masked_array(srt.copy(), mask=null)
    t = conn.read_image(fl.write_image([("s", fl.INT64, srt, fl.ENC_AUTO), ("x", fl.INT64, shf, fl.ENC_AUTO),
                                        ("n", fl.INT64, nul, fl.ENC_AUTO)], rowgroup=RG))
    yield t, {0: srt, 1: shf, 2: srt}, {2: ~null}
    t.close()


def grouped_or_no_gpu(fl, t, keys, **kw):
    """the call's result, or None where it reached device work on a machine
    without a GPU (which is how a CPU test sees that a row group survived)"""
    try:
        return t.aggregate_grouped(keys, [("count",)], **kw)
    except fl.FlsError as e:
        assert e.code == ERR_DEVICE and fl.device_count() == 0, e
        return None


def test_pruning_exact_on_sorted_keep_unmatched_prunes_nothing(fl, conn, prunetab):
    t, cols, valid = prunetab
    rng = np.random.default_rng(4)
    srt = cols[0]
    maps = [M(conn, {int(k): 1 for k in srt[[3, 4, 2 * RG + 7]]}), M(conn, {int(srt[RG - 1]): 0, int(srt[RG]): 1}),
            M(conn, {int(srt[-1]): 5}), M(conn, {int(srt[0]) - 1: 1, int(srt[-1]) + 1: 2}),
            M(conn, {int(k): int(k) % 7 for k in rng.choice(srt, 40)}, form=HASH),
            M(conn, {int(k) + 1: 3 for k in srt[RG:RG + 300]}, form=DENSE)]
    for m in maps:
        for rg in range(t.nrowgroups):
            sl = slice(rg * RG, (rg + 1) * RG)
            lo, hi = int(srt[sl].min()), int(srt[sl].max())
            has = any(lo <= k <= hi for k in m.d)                                # exactly [min, max]
            got = grouped_or_no_gpu(fl, t, [("map", 0, m.km)], rg_begin=rg, rg_end=rg + 1)
            assert t.pruned == (0 if has else 1), (rg, sorted(m.d)[:4])
            if not has:
                assert got == []                                                 # no device work, no GPU needed
            elif got is not None:
                codes = [m.d[int(v)] for v in srt[sl] if int(v) in m.d]
                assert [k for (k,), _ in got] == list(dict.fromkeys(codes))
            # the nullable column: its all-NULL chunk is pruned, the others by their valid rows' range
            vs = srt[sl][valid[2][sl]]
            has2 = rg != 2 and any(int(vs.min()) <= k <= int(vs.max()) for k in m.d)
            got = grouped_or_no_gpu(fl, t, [("map", 2, m.km)], rg_begin=rg, rg_end=rg + 1)
            assert t.pruned == (0 if has2 else 1) and (has2 or got == [])
            # the shuffled column: conservative
            got = grouped_or_no_gpu(fl, t, [("map", 1, m.km)], rg_begin=rg, rg_end=rg + 1)
            if t.pruned:
                assert got == [] and not any(int(v) in m.d for v in cols[1][sl])
    # keep-unmatched prunes nothing: every row group is read, whatever the map holds
    far = M(conn, {int(srt[-1]) + 5: 1})
    for m in (far, M(conn, {})):
        got = grouped_or_no_gpu(fl, t, [("map", 0, m.km, KEEP)])
        assert t.pruned == 0 and got in (None, [((None,), [N])])
        got = grouped_or_no_gpu(fl, t, [("map", 2, m.km, KEEP)], rg_begin=2, rg_end=3)     # the all-NULL chunk too
        assert t.pruned == 0 and got in (None, [((None,), [RG])])
    # an inner binding and a filter prune together
    got = grouped_or_no_gpu(fl, t, [("map", 0, maps[0].km)], filt=[(0, ">", int(srt[RG]))])
    assert t.pruned == t.nrowgroups - 1 and got in (None, [((1,), [1])])


def test_empty_map_returns_zero_groups_without_a_gpu(fl, conn, prunetab):
    t, cols, valid = prunetab
    aggs = [("count",), ("sum", 0), ("min", 1)]
    for form in (0, DENSE, HASH):
        e = conn.keymap([], [], form=form)
        assert t.aggregate_grouped([("map", 0, e)], aggs) == [] and t.pruned == t.nrowgroups
        assert t.aggregate_grouped([1, ("map", 0, e)], aggs, filt=[(1, ">", 0)]) == [] and t.pruned == t.nrowgroups
    # a map with no key in any zone map prunes everything as well
    far = conn.keymap([int(cols[0][-1]) + 5, int(cols[0][0]) - 5], [1, 2])
    assert t.aggregate_grouped([("map", 0, far)], aggs) == [] and t.pruned == t.nrowgroups
    # ... and the bindings are gone after the call
    with pytest.raises(fl.FlsError, match="no binding 0"):
        t.aggregate_grouped([fl.KEY_MAPPED], aggs)


def test_keymap_kernel_resources():
    """keymap_kernel: no scratch, no spill, at most 64 VGPRs (eight waves per
    SIMD) and the four wave counts in LDS"""
    if not LIB.exists():
        pytest.skip("libflsgpu.so not built")
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    res = kernel_resources.resources(str(LIB))
    hits = {k: v for k, v in res.items() if "keymap_kernel" in k}
    assert len(hits) == 1, sorted(res)
    for name, r in hits.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 64 and r["lds"] <= 16, (name, r)


def test_keymap_construction_under_asan(tmp_path):
    """tests/fuzz/fuzz_keymap.cpp, a stand-alone program over the host-only
    header, built with -fsanitize=address,undefined: seeded random and
    adversarial maps, keymap_lookup against std::map"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path / "fuzz_keymap"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", str(CSRC), str(ROOT / "tests" / "fuzz" / "fuzz_keymap.cpp"),
                    "-o", str(out)], check=True)
    r = subprocess.run([str(out), "150", "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"sanitizer report or mismatch\n{r.stderr[-4000:]}"
    assert r.stdout.startswith("iterations 150 failures 0"), r.stdout


# ------------------------------------------------------------------ GPU tests
C_X = len(KEY_TYPES)          # typetab's measure column
TYPE_AGGS = [("count",), ("sum", C_X), ("min", C_X)]


@pytest.fixture(scope="module")
def typetab(fl, conn):
    rng = np.random.default_rng(21)
    specs, cols, pools = [], {}, {}
    for c, name in enumerate(KEY_TYPES):
        ty = getattr(fl, name)
        pool = key_pool(fl, name, rng)
        vals = np.array([pool[i] for i in rng.integers(0, len(pool), N)], dtype=object).astype(fl.NP_DTYPE[ty])
        specs.append((name.lower(), ty, vals, fl.ENC_FFOR, *((15, 2) if name == "DECIMAL" else ())))
        cols[c], pools[c] = vals, pool
    cols[C_X] = rng.integers(-10 ** 12, 10 ** 12, N).astype(np.int64)
    specs.append(("x", fl.INT64, cols[C_X], fl.ENC_AUTO))
    t = conn.read_image(fl.write_image(specs, rowgroup=RG))
    yield t, cols, pools
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["inner", KEEP])
@pytest.mark.parametrize("form", [DENSE, HASH])
@pytest.mark.parametrize("name", KEY_TYPES)
def test_gpu_every_key_type_against_the_dict(fl, gpu, conn, typetab, name, form, mode):
    t, cols, pools = typetab
    c = KEY_TYPES.index(name)
    lo, hi = type_range(fl, name)
    signed = lo < 0
    pool = pools[c]
    rng = np.random.default_rng(c)
    half = [v for v in pool if rng.random() < 0.5] or pool[:1]                   # about half of the distinct values
    absent = [v for v in (lo + 5, hi - 5, 3, 1234) if lo <= v <= hi and v not in pool]
    edges = [lo, hi] + ([-1 if signed else hi] if hi - lo >= (1 << 63) else [])
    if form == HASH or hi - lo < 1 << 31:
        groups = [half + absent + edges]
    else:
        # a dense map spans at most 2^31 values: the minimum, the maximum and -1 / ~0 each in a map of its own cluster
        groups = [[v for v in half + absent + edges if v - lo < 1 << 20],
                  [v for v in half + absent + edges if hi - v < 1 << 20],
                  [v for v in half + absent + [-1 if signed else 0] if abs(v) < 1 << 20]]
    for keys in groups:
        m = M(conn, {k: 3 * (i % 20) for i, k in enumerate(keys)}, signed=signed, form=form)   # at most 20 codes
        assert m.km.info.form == form
        spec = ("map", c, m) if mode == "inner" else ("map", c, m, KEEP)
        got = check_grouped(t, [spec], TYPE_AGGS, cols, what=(name, form, mode))
        n = sum(v[0] for _, v in got)
        assert (0 < n < N or name == "BOOLEAN") if mode == "inner" else n == N
        m.km.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [DENSE, HASH])
def test_gpu_every_encoding_of_the_key_column(fl, gpu, conn, form):
    rng = np.random.default_rng(31)
    ffor = rng.integers(-500, 500, N).astype(np.int32)
    delta = (np.cumsum(rng.integers(0, 4, N)) - 4000).astype(np.int64)
    dic = (rng.integers(0, 9, N) * 1000003 - 3000009).astype(np.int64)
    rle = np.repeat(rng.integers(-20, 20, N // 50 + 1), 50)[:N].astype(np.int16)
    auto = (rng.integers(0, 30, N) * 11).astype(np.uint32)
    img = fl.write_image([("ffor", fl.INT32, ffor, fl.ENC_FFOR), ("delta", fl.INT64, delta, fl.ENC_DELTA),
                          ("dict", fl.INT64, dic, fl.ENC_DICT), ("rle", fl.INT16, rle, fl.ENC_RLE),
                          ("auto", fl.UINT32, auto, fl.ENC_AUTO)], rowgroup=RG)
    assert {tuple(r[:4]) for r in chunk_encodings(img.tobytes())} == {(fl.ENC_FFOR, fl.ENC_DELTA, fl.ENC_DICT, fl.ENC_RLE)}
    t = conn.read_image(img)
    cols = {0: ffor, 1: delta, 2: dic, 3: rle, 4: auto}
    aggs = [("count",), ("sum", 0), ("max", 1)]
    try:
        for c in cols:
            present = np.unique(cols[c])
            some = max(1, min(len(present) // 2, 60))            # (the DICT column has nine distinct values)
            keys = [int(v) for v in rng.choice(present, some, replace=False)] + [int(present[-1]) + 1]   # one absent
            m = M(conn, {k: i % 17 for i, k in enumerate(keys)}, signed=c != 4, form=form)
            for spec in (("map", c, m), ("map", c, m, KEEP)):
                got = check_grouped(t, [spec], aggs, cols, what=(c, spec[3:]))
                assert 1 < len(got) <= 18
    finally:
        t.close()


@pytest.fixture(scope="module")
def nulltab(fl, conn):
    """column 0: NULLs everywhere (the placeholder stored at a NULL row is 0);
    column 1: NULLs in row groups 1 and 3 only, so a batch mixes row groups
    with and without validity; column 2: no NULL; column 3: a row id;
    column 4: a DICT VARCHAR of three strings"""
    rng = np.random.default_rng(41)
    a = rng.integers(-30, 30, N).astype(np.int32)
    b = rng.integers(0, 60, N).astype(np.uint16)
    c = rng.integers(-5, 6, N).astype(np.int8)
    na = rng.random(N) < 0.3
    nb = np.zeros(N, bool)
    nb[RG:2 * RG] = rng.random(RG) < 0.5
    nb[3 * RG:4 * RG] = rng.random(RG) < 0.5
    ids = np.arange(N, dtype=np.int32)
    s = [(b"air", b"rail", b"ship")[i] for i in rng.integers(0, 3, N)]
    t = conn.read_image(fl.write_image([("a", fl.INT32, np.ma.masked_array(a, mask=na), fl.ENC_AUTO),
                                        ("b", fl.UINT16, np.ma.masked_array(b, mask=nb), fl.ENC_AUTO),
                                        ("c", fl.INT8, c, fl.ENC_AUTO), ("id", fl.INT32, ids, fl.ENC_AUTO),
                                        ("s", fl.VARCHAR, [x.decode() for x in s], fl.ENC_DICT)], rowgroup=RG))
    # what the engine decodes at a NULL row is the writer's placeholder
    yield t, {0: np.where(na, 0, a).astype(np.int32), 1: np.where(nb, 0, b).astype(np.uint16), 2: c, 3: ids, 4: s}, \
        {0: ~na, 1: ~nb}
    t.close()


NULL_AGGS = [("count",), ("count", 0), ("sum", 1), ("min", 3), ("sum_expr", [(0, 1, 3), (100, -1, 2)])]


@pytest.mark.gpu
@pytest.mark.parametrize("form", [DENSE, HASH])
def test_gpu_null_key_rows(fl, gpu, conn, nulltab, form, monkeypatch):
    t, cols, valid = nulltab
    ma = M(conn, {0: 4, -7: 1, 3: 1, 29: 0, 1000: 9}, form=form)                # 0: the placeholder at the NULL rows
    mb = M(conn, {0: 0, 1: 1, 17: 1, 59: 65534}, signed=False, form=form)
    assert t.validity(0, 1) is None and t.validity(1, 1) is not None
    for batch in ("1", "8"):
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)              # 8: one batch mixes row groups with / without validity
        for c, m in ((0, ma), (1, mb)):
            inner = check_grouped(t, [("map", c, m)], NULL_AGGS, cols, valid, what=("inner", c, batch))
            assert all(k[0] is not None for k, _ in inner)                       # inner: never NULL
            # the placeholder 0 at a NULL row is a map key, and forms no group: code(0) counts the valid zeros only
            zeros = int(((cols[c] == 0) & valid[c]).sum())
            assert dict((k[0], v[0]) for k, v in inner)[m.d[0]] == zeros < int((cols[c] == 0).sum())
            kept = check_grouped(t, [("map", c, m, KEEP)], NULL_AGGS, cols, valid, what=("keep", c, batch))
            hit = np.array([int(v) in m.d for v in cols[c]]) & valid[c]
            assert dict((k[0], v[0]) for k, v in kept)[None] == N - int(hit.sum())   # NULL and unmatched rows together
            assert sum(v[0] for _, v in kept) == N and sum(v[0] for _, v in inner) == int(hit.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("form", [DENSE, HASH])
def test_gpu_mapped_keys_combined_with_filters(fl, gpu, conn, nulltab, form):
    t, cols, valid = nulltab
    ma = M(conn, {k: (k // 3) % 4 for k in range(-30, 30, 2)}, form=form)      # 4 codes: 5 x 11 keys with column 2
    mb = M(conn, {0: 0, 5: 1, 6: 1, 7: 2, 40: 2, 41: 3}, signed=False, form=form)
    sc = conn.keyset([-5, 0, 5], form=form)
    sb = conn.keyset([0, 5, 6, 7, 40, 41, 42], signed=False, form=form)
    sc_mask = np.isin(cols[2], [-5, 0, 5])
    sb_mask = np.isin(cols[1], [0, 5, 6, 7, 40, 41, 42]) & valid[1]
    cases = [
        (None, None),                                                             # no filter: the zero-term mask path
        ([(2, ">", 0)], None),                                                    # an ordinary term
        ([(2, "<", 0, 1), (2, ">", 3, 1), (1, "is_not_null", None)], None),
        ([(2, "in_set", sc)], sc_mask),                                           # a set term on another column
        ([(3, ">=", 64), (1, "in_set", sb), (2, "in_set", sc)], (cols[3] >= 64) & sb_mask & sc_mask),
        # ordinary terms that reject whole 64-row words and whole vectors
        ([(3, ">=", 64), (3, "<", 1024 + 128, 1), (3, ">=", 3 * 1024, 1)], None),
        ([(3, "<", 0)], None),                                                    # nothing left for the map
        ([(3, ">=", N - 5)], None),                                               # the partial tail only
        ([(0, "=", 4)], None),                                                    # the binding's column in the filter
    ]
    for filt, sel in cases:
        for keys in ([("map", 0, ma)], [("map", 0, ma, KEEP), 2], [("map", 0, ma), ("map", 1, mb, KEEP)]):
            check_grouped(t, keys, NULL_AGGS, cols, valid, filt=filt, sel=sel, what=(filt, len(keys)))
    # the tail vector's rows past nrows contribute nothing: every row is counted once, none twice
    got = check_grouped(t, [("map", 3, M(conn, {i: i % 3 for i in range(5 * RG, 6 * RG)}, form=form), KEEP)],
                        [("count",)], cols, valid, rg_begin=5, sel=cols[3] >= 5 * RG)
    assert sorted(got) == [((0,), [111]), ((1,), [111]), ((2,), [111])]           # 333 rows, no NULL group


@pytest.mark.gpu
def test_gpu_two_mapped_keys_with_plain_and_varchar_keys(fl, gpu, conn, nulltab):
    t, cols, valid = nulltab
    ma = M(conn, {k: k % 3 for k in range(-30, 30) if k % 4}, form=HASH)         # 3 codes, a quarter unmatched
    mb = M(conn, {k: k % 2 for k in range(0, 60, 3)}, signed=False, form=DENSE)  # 2 codes or NULL
    filt = [(2, ">=", 0), (2, "<=", 1)]                                           # c in {0, 1}: 3 x 3 x 3 x 2 = 54 keys at most
    for keys in ([("map", 0, ma), 4, ("map", 1, mb, KEEP), 2], [2, ("map", 1, mb, KEEP), ("map", 0, ma), 4],
                 [0, ("map", 0, ma)]):                                            # the bound column as a plain key as well
        got = check_grouped(t, keys, NULL_AGGS, cols, valid, filt=filt if len(keys) == 4 else [(0, "<", 0)],
                            what=len(keys))
        assert len(got) > 20


RG5 = 8192
N5 = RG5 + 64


@pytest.fixture(scope="module")
def limits(fl, conn):
    i = np.arange(N5)
    v, r = (i % RG5) // 1024, i % 1024
    # vectors 0..3 of a row group hold 64 values each, disjoint: 256 in the row group; vectors 4..7 repeat the first 64
    k256 = np.where(v < 4, 64 * v + r % 64, r % 64).astype(np.int32)
    k257 = k256.copy()
    k257[4 * 1024 + 63::64][:16] = 256           # vector 4: value 63 gives way to a 257th (still 64 in the vector)
    k65 = (r % 65).astype(np.int32)              # 65 values in every vector
    x = (i * 7 % 1000 - 500).astype(np.int32)
    t = conn.read_image(fl.write_image([("k256", fl.INT32, k256, fl.ENC_AUTO), ("k257", fl.INT32, k257, fl.ENC_AUTO),
                                        ("k65", fl.INT32, k65, fl.ENC_AUTO), ("x", fl.INT32, x, fl.ENC_AUTO)],
                                       rowgroup=RG5))
    yield t, {0: k256, 1: k257, 2: k65, 3: x}
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [DENSE, HASH])
def test_gpu_capacities_count_distinct_codes(fl, gpu, conn, limits, form):
    t, cols = limits
    aggs = [("count",), ("sum", 3), ("min", 3)]
    code = lambda k: 1000 + 7 * k                                                # noqa: E731  (injective)
    all257 = M(conn, {k: code(k) for k in range(257)}, form=form)
    first64 = M(conn, {k: code(k) for k in range(64)}, form=form)
    no256 = M(conn, {k: code(k) for k in range(256)}, form=form)
    folded = M(conn, {k: k % 64 for k in range(257)}, form=form)                 # 257 values onto 64 codes

    def still_works():
        check_grouped(t, [("map", 0, folded)], aggs, cols, what="folded")
        assert t.aggregate([("count",), ("sum", 3)]) == [N5, int(cols[3].astype(np.int64).sum())]

    # 64 codes in a vector, 4 x 64 = 256 in the row group: within both capacities
    assert len(check_grouped(t, [("map", 0, all257)], aggs, cols, what="k256")) == 256
    # 65 values in every vector: 65 codes is one too many, 64 of them mapped (inner) is fine
    with pytest.raises(fl.FlsError) as e:
        t.aggregate_grouped([("map", 2, all257.km)], aggs)
    assert e.value.code == ERR_LIMIT and "64" in e.value.msg and "scan" in e.value.msg, e.value
    still_works()
    assert len(check_grouped(t, [("map", 2, first64)], aggs, cols, what="k65 inner")) == 64
    with pytest.raises(fl.FlsError) as e:                                        # ... and the NULL group is a 65th key
        t.aggregate_grouped([("map", 2, first64.km, KEEP)], aggs)
    assert e.value.code == ERR_LIMIT
    still_works()
    # a 257th code in a row group; without it 256
    with pytest.raises(fl.FlsError) as e:
        t.aggregate_grouped([("map", 1, all257.km)], aggs)
    assert e.value.code == ERR_LIMIT and "256" in e.value.msg and "scan" in e.value.msg, e.value
    still_works()
    assert len(check_grouped(t, [("map", 1, no256)], aggs, cols, what="k257 inner")) == 256
    # the capacities count codes, not values
    assert len(check_grouped(t, [("map", 1, folded)], aggs, cols, what="k257 folded")) == 64
    assert len(check_grouped(t, [("map", 2, folded)], aggs, cols, what="k65 folded")) == 64


@pytest.mark.gpu
@pytest.mark.parametrize("home", [5, 127])
def test_gpu_colliding_keys(fl, gpu, conn, home):
    keys = colliding_keys(50, 7, home)
    others = colliding_keys(90, 7, home)[50:]
    rng = np.random.default_rng(51)
    pool = np.array(keys + others + [0, M64], dtype=np.uint64)
    vals = pool[rng.integers(0, len(pool), N)]
    m = M(conn, {k: j % 20 for j, k in enumerate(keys)}, signed=False, form=HASH)
    assert m.km.info.max_probe == 50
    t = conn.read_image(fl.write_image([("k", fl.UINT64, vals, fl.ENC_AUTO)], rowgroup=RG))
    try:
        for spec in (("map", 0, m), ("map", 0, m, KEEP)):
            got = check_grouped(t, [spec], [("count",), ("max", 0)], {0: vals}, what=spec[3:])
            assert len(got) == 20 + len(spec[3:])
    finally:
        t.close()


@pytest.fixture(scope="module")
def facttab(fl, conn):
    """a small fact table: a small-range key with NULLs, a DOUBLE measure with
    NaN, infinities and signed zeros, an integer measure with NULLs"""
    rng = np.random.default_rng(61)
    c = rng.integers(0, 40, N).astype(np.int16)
    nc = rng.random(N) < 0.1
    pool = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e300, 1.5, -1.5, 0.1])
    d = pool[rng.integers(0, len(pool), N)]
    d[c % 3 == 0] = np.round(rng.normal(0, 10, N), 2)[c % 3 == 0]                # a third of the keys: finite sums
    x = rng.integers(-10 ** 9, 10 ** 9, N).astype(np.int64)
    nx = rng.random(N) < 0.2
    img = fl.write_image([("c", fl.INT16, np.ma.masked_array(c, mask=nc), fl.ENC_AUTO),
                          ("d", fl.DOUBLE, d, fl.ENC_AUTO),
                          ("x", fl.INT64, np.ma.masked_array(x, mask=nx), fl.ENC_AUTO)], rowgroup=RG)
    t = conn.read_image(img)
    yield t, img
    t.close()


FACT_AGGS = [("count",), ("sum", 1), ("min", 1), ("max", 1), ("sum", 2), ("count", 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", [DENSE, HASH])
def test_gpu_identity_map_equals_the_plain_key_under_in_set(fl, gpu, conn, facttab, form):
    """a map v -> v restricted to S groups as the plain key does under
    `c IN S`, group for group and bit for bit; with one key, as fls_aggregate"""
    t, _ = facttab
    S = [1, 3, 4, 9, 12, 15, 20, 21, 27, 33, 38, 39, 77]
    m = conn.keymap(S, S, form=form)
    ks = conn.keyset(S)
    mapped = t.aggregate_grouped([("map", 0, m)], FACT_AGGS)
    plain = t.aggregate_grouped([0], FACT_AGGS, filt=[(0, "in_set", ks)])
    assert len(mapped) == 12 and as_bits(mapped) == as_bits(plain)
    assert any(isinstance(v[1], float) and v[1] != v[1] for _, v in mapped)      # a NaN sum among them
    # under further terms, and with the plain key beside the mapped one
    filt = [(2, "is_not_null", None), (1, "<", 1e300)]
    assert as_bits(t.aggregate_grouped([("map", 0, m)], FACT_AGGS, filt=filt)) == \
        as_bits(t.aggregate_grouped([0], FACT_AGGS, filt=filt + [(0, "in_set", ks)]))
    both = t.aggregate_grouped([0, ("map", 0, m)], FACT_AGGS)
    assert [(k[1],) for k, _ in both] == [k for k, _ in plain] and [v for _, v in as_bits(both)] == \
        [v for _, v in as_bits(plain)] and all(k[0] == k[1] for k, _ in both)
    # one group: the ungrouped call under the same set filter
    for key in (12, 4):                                                          # 12: finite sums; 4: NaN and infinities
        one, k1 = conn.keymap([key], [key], form=form), conn.keyset([key])
        got = t.aggregate_grouped([("map", 0, one)], FACT_AGGS)
        assert len(got) == 1 and got[0][0] == (key,)
        assert [bits(v) for v in got[0][1]] == [bits(v) for v in t.aggregate(FACT_AGGS, filt=[(0, "in_set", k1)])]


@pytest.mark.gpu
def test_gpu_results_identical_across_batches_slots_and_gpus(fl, gpu, conn, facttab, monkeypatch):
    t, img = facttab
    rng = np.random.default_rng(63)
    dmap = {int(k): int(k) % 11 for k in rng.choice(40, 25, replace=False)}

    def run(c, t):   # (the batch size is read when a scan starts; the maps belong to the table's connection)
        md, mh = M(c, dmap, form=DENSE), M(c, dmap, form=HASH)
        return (as_bits(t.aggregate_grouped([("map", 0, md.km)], FACT_AGGS)),
                as_bits(t.aggregate_grouped([("map", 0, mh.km, KEEP)], FACT_AGGS, filt=[(1, "<", 2.5)])),
                as_bits(t.aggregate_grouped([("map", 0, mh.km), 0], FACT_AGGS)))

    monkeypatch.delenv("FLS_SCAN_BATCH", raising=False)
    base = run(conn, t)
    assert 1 < len(base[0]) <= 11 and len(base[1]) == len(base[0]) + 1 and len(base[2]) == len(dmap)
    for batch in ("1", "3", "8"):
        for slots in ("1", "2"):
            monkeypatch.setenv("FLS_SCAN_BATCH", batch)
            monkeypatch.setenv("FLS_SCAN_SLOTS", slots)
            assert run(conn, t) == base, (batch, slots)
    monkeypatch.delenv("FLS_SCAN_SLOTS")
    # every visible GPU count: the row groups are sharded over them, so the map's image reaches each device
    monkeypatch.setenv("FLS_SCAN_BATCH", "1")
    for ndev in range(1, gpu + 1):
        call = fl.Connection(list(range(ndev)))
        try:
            tm = call.read_image(img)
            assert run(call, tm) == base, ndev
            tm.close()
        finally:
            call.close()
    # ... and two pipelines on one GPU
    monkeypatch.setenv("FLS_SCAN_BATCH", "3")
    c2 = fl.Connection([0, 0])
    try:
        t2 = c2.read_image(img)
        assert run(c2, t2) == base, "two pipelines"
        t2.close()
    finally:
        c2.close()


@pytest.mark.gpu
def test_gpu_one_map_serves_two_tables_and_survives_its_handle(fl, gpu, conn):
    rng = np.random.default_rng(71)
    a = rng.integers(0, 500, N).astype(np.int32)
    b = rng.integers(0, 500, 2 * RG + 77).astype(np.int32)
    ta = conn.read_image(fl.write_image([("a", fl.INT32, a, fl.ENC_AUTO)], rowgroup=RG))
    tb = conn.read_image(fl.write_image([("b", fl.INT32, b, fl.ENC_AUTO)], rowgroup=RG))
    aggs = [("count",), ("sum", 0)]
    try:
        m = M(conn, {int(k): int(k) % 9 for k in rng.choice(500, 120, replace=False)}, form=HASH)
        m2 = M(conn, {k: 100 + k % 4 for k in range(0, 500, 5)}, form=DENSE)
        for _ in range(2):                                                       # the cached image is reused
            check_grouped(ta, [("map", 0, m)], aggs, {0: a})
            check_grouped(tb, [("map", 0, m, KEEP)], aggs, {0: b})
        # bound, then freed before the call: the binding holds a reference
        ta.set_key_bindings([(0, m.km)])
        tb.set_key_bindings([(0, m.km, fl.KEYMAP_KEEP_UNMATCHED)])
        m.km.close()
        with pytest.raises(fl.FlsError, match="not a live key map"):
            ta.set_key_bindings([(0, 0)])                                        # (a failed setter leaves the bindings)
        key = [fl.KEY_MAPPED | 0]
        for t, vals, keep in ((ta, a, ()), (tb, b, (KEEP,))):
            want = want_groups([("map", 0, m, *keep)], {0: vals}, {}, np.ones(len(vals), bool))
            got = t.aggregate_grouped(key, aggs)
            assert [(k, v) for k, v in got] == [(k, want_aggs(aggs, {0: vals}, {}, w)) for k, w in want]
        # replacing the bindings between two calls takes effect
        ta.set_key_bindings([(0, m2.km)])
        got = ta.aggregate_grouped(key, aggs)
        want = want_groups([("map", 0, m2)], {0: a}, {}, np.ones(N, bool))
        assert [k for k, _ in got] == [k for k, _ in want] and {k[0] for k, _ in got} == {100, 101, 102, 103}
        ta.set_key_bindings([(0, m2.km, fl.KEYMAP_KEEP_UNMATCHED), (0, m2.km)])   # binding 1 is the inner one now
        assert [k for k, _ in ta.aggregate_grouped([fl.KEY_MAPPED | 1], aggs)] == [k for k, _ in want]
        assert ((None,) in [k for k, _ in ta.aggregate_grouped(key, aggs)])
        ta.set_key_bindings(None)
        tb.set_key_bindings(None)
    finally:
        ta.close()
        tb.close()


C_OKEY, C_SUPP, C_PRICE, C_DISC, C_SHIPDATE = 0, 2, 5, 6, 10
DAY_1994, DAY_1995 = 8766, 9131


@pytest.mark.gpu
def test_gpu_lineitem_q5_shape(fl, gpu, conn):
    """the build side from a scan of a small "supplier" table (Table.keymap:
    suppkey -> nationkey in [0, 25)), then revenue and count(*) per nation of
    the supplier under a one-year l_shipdate filter: TPC-H Q5's shape"""
    wl, sf = "lineitem", 0.05
    t = conn.read_image(fl.gen_image(wl, sf))
    try:
        n = t.nrows
        assert 4 <= t.nrowgroups <= 8
        supp = fl.gen_values(wl, C_SUPP, 0, n, fl.NP_DTYPE[t.column(C_SUPP).type], sf)
        price = fl.gen_values(wl, C_PRICE, 0, n, np.int64, sf)
        disc = fl.gen_values(wl, C_DISC, 0, n, np.int64, sf)
        ship = fl.gen_values(wl, C_SHIPDATE, 0, n, np.int32, sf)
        # the supplier table: most of lineitem's suppliers and some it never names; a few without a nation
        rng = np.random.default_rng(81)
        skeys = np.unique(np.concatenate([supp.astype(np.int64), np.arange(-3, 3)]))
        some = rng.random(len(skeys)) < 0.9
        some[:3] = True                                                          # (the negative keys stay)
        skeys = skeys[some]
        nation = ((skeys * 7 + 3) % 25).astype(np.int32)
        no_nation = rng.random(len(skeys)) < 0.02
        region = (nation % 5).astype(np.int8)
        st = conn.read_image(fl.write_image(
            [("s_suppkey", t.column(C_SUPP).type, skeys.astype(supp.dtype), fl.ENC_AUTO),
             ("s_nationkey", fl.INT32, np.ma.masked_array(nation, mask=no_nation), fl.ENC_AUTO),
             ("s_region", fl.INT8, region, fl.ENC_AUTO)], rowgroup=RG))
        aggs = [("sum_expr", [(0, 1, C_PRICE), (100, -1, C_DISC)]), ("count",)]
        filt = [(C_SHIPDATE, ">=", DAY_1994), (C_SHIPDATE, "<", DAY_1995)]
        for build, form in ((None, 0), ([(2, "=", 1)], DENSE), ([(2, "=", 1)], HASH)):
            km = st.keymap(0, 1, build, form=form)
            on = ~no_nation & (region == 1 if build else True)
            ref = dict(zip(skeys[on].tolist(), nation[on].tolist()))
            assert km.info.count == len(ref) and km.info.max_code == max(ref.values()) < 25
            assert all(km.lookup(k) == ref.get(k) for k in skeys[::7].tolist())
            got = t.aggregate_grouped([("map", C_SUPP, km)], aggs, filt=filt)
            sel = (ship >= DAY_1994) & (ship < DAY_1995)
            code = np.array([ref.get(int(k), -1) for k in supp])
            m = sel & (code >= 0)
            order = list(dict.fromkeys(code[m].tolist()))
            assert [k for k, _ in got] == [(c,) for c in order] and 1 < len(order) <= 25
            rev = price * (100 - disc)
            for (c,), vals in got:
                g = m & (code == c)
                assert vals == [int(rev[g].sum()), int(g.sum())], c
            assert sum(v[1] for _, v in got) == int(m.sum()) < int(sel.sum())
            km.close()
        with pytest.raises(ValueError, match="outside"):                         # a value that is no code
            st.keymap(1, 0)
        with pytest.raises(ValueError, match="not integer-like"):
            t.keymap(C_SUPP, 14)                                                 # l_shipmode
        st.close()
    finally:
        t.close()
