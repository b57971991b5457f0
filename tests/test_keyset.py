"""Key-set filter terms (`column IN set` / `NOT IN set`):
the host construction (csrc/fls_keyset.hpp through fls_keyset_*), the argument
checks, the zone-map pruning -- all without a GPU -- and keyset_kernel on the
GPU against np.isin, through the scan, the aggregates and top-N.

Small shapes throughout: 1024-row row groups, five whole vectors and a partial
tail, sets from 0 to a few thousand keys."""
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import filter_mask, rand64

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "duckdb-fastlane_amd" / "csrc"
LIB = ROOT / "duckdb-fastlane_amd" / "libflsgpu.so"
RG = 1024
N = 5 * 1024 + 333
M64 = (1 << 64) - 1
HASH_MUL = 0x9E3779B97F4A7C15
HASH_INV = pow(HASH_MUL, -1, 1 << 64)
ERR_ARG, ERR_LIMIT = -3, -8
BITMAP, HASH = 1, 2


# ---- helpers of this file
class S:
    """a key set and the values it was made of (the numpy side of a term)"""

    def __init__(self, conn, values, signed=True, form=0):
        self.values = [int(v) for v in values]
        self.ks = conn.keyset(self.values, signed=signed, form=form)


def eng(terms):
    """the terms as the engine takes them: S -> its KeySet"""
    return [(t[0], t[1], t[2].ks if isinstance(t[2], S) else t[2], *t[3:]) for t in terms]


def isin_mask(cols, terms, n, valid=None):
    """helpers.filter_mask extended with (col, "in_set" / "not_in_set", S): a
    set term is a clause of its own; a NULL row satisfies neither operator"""
    valid = valid or {}
    out = filter_mask(cols, [t for t in terms if t[1] not in ("in_set", "not_in_set")], n, valid)
    for col, op, s, *_ in terms:
        if op not in ("in_set", "not_in_set"):
            continue
        members = set(s.values)
        hit = np.fromiter((int(v) in members for v in cols[col]), bool, len(cols[col]))
        if op == "not_in_set":
            hit = ~hit
        ok = valid.get(col)
        out &= hit if ok is None else hit & ok
    return out


def scan_rows(t, terms, deliver=None):
    """(global rows selected, delivered arrays per column concatenated)"""
    rows, parts = [], {}
    for rg, first_row, sel, arrays in t.scan_filtered(eng(terms), cols=deliver):
        rows.append(sel.astype(np.int64) + first_row)
        for c in deliver or []:
            parts.setdefault(c, []).append(arrays[c])
    return (np.concatenate(rows) if rows else np.zeros(0, np.int64)), parts


def check_scan(fl, t, cols, terms, valid=None, deliver=None):
    want = np.nonzero(isin_mask(cols, terms, t.nrows, valid))[0]
    got, parts = scan_rows(t, terms, deliver)
    assert np.array_equal(got, want), (terms, len(got), len(want))
    for c in deliver or []:
        ty = t.column(c).type
        vals = np.concatenate(parts[c]).view(fl.NP_DTYPE[ty]) if parts.get(c) else np.zeros(0, fl.NP_DTYPE[ty])
        keep = np.ones(len(want), bool) if not valid or c not in valid else valid[c][want]
        assert np.array_equal(vals[keep], cols[c][want][keep]), (terms, c)
    return want


def colliding_keys(n, cap_log2, home):
    """n distinct keys whose documented home slot is `home` in a table of
    2^cap_log2 slots: key * HASH_MUL = home << (64 - cap_log2) | j"""
    return [(HASH_INV * ((home << (64 - cap_log2)) | j)) & M64 for j in range(1, n + 1)]


def as_signed(k):
    return k - (1 << 64) if k >> 63 else k


@pytest.fixture(scope="module")
def conn(fl):
    c = fl.Connection([0])
    yield c
    c.close()


# ------------------------------------------------------------------ CPU tests
def test_library_exports_the_keyset_functions(fl):
    for name in ("fls_keyset_create", "fls_keyset_free", "fls_keyset_info", "fls_keyset_contains"):
        assert hasattr(fl.lib, name), name
    assert fl.OPS["in_set"] == 9 and fl.OPS["not_in_set"] == 10


def test_deduplication_and_info_of_every_form(fl, conn):
    vals = [5, 1, 1, -1, 7, 7, 7, 1 << 40]
    h = conn.keyset(vals, form=HASH).info
    assert (h.count, h.form, h.capacity, h.device_bytes) == (5, HASH, 16, 128)        # next power of two >= 2 * 5
    assert as_signed(h.min) == -1 and h.max == 1 << 40 and 1 <= h.max_probe <= 5
    assert h.empty == M64 - 1                                                           # ~0 is the key -1
    a = conn.keyset(vals).info
    assert a.form == HASH                                                               # 2^40 values: no bitmap
    b = conn.keyset(vals[:-1], form=BITMAP).info
    assert (b.count, b.form, b.capacity, b.max_probe, b.device_bytes) == (4, BITMAP, 0, 0, 8)
    assert as_signed(b.min) == -1 and b.max == 7
    u = conn.keyset([3, M64, 0], signed=False).info
    assert (u.count, u.kind, u.min, u.max) == (3, 1, 0, M64)                            # unsigned order
    e = conn.keyset([])
    assert e.info.count == 0 and not e.contains(0) and not e.contains(-1)
    for form in (BITMAP, HASH):
        e = conn.keyset([], form=form)
        assert (e.info.count, e.info.form) == (0, form) and not e.contains(0) and not e.contains(M64)


def test_auto_rule_at_its_boundaries(fl, conn):
    """auto takes the bitmap when it is no larger than the hash table would
    be, or at most 1 MiB: one key moved by one on either side of each bound"""
    # 3 keys: a 64-byte hash table; the bitmap of span 2^23 - 1 is exactly 1 MiB
    at = conn.keyset([10, 11, 10 + (1 << 23) - 1]).info
    assert (at.form, at.device_bytes) == (BITMAP, 1 << 20)
    past = conn.keyset([10, 11, 10 + (1 << 23)]).info
    assert (past.form, past.device_bytes, past.capacity) == (HASH, 64, 8)
    # 2^17 + 1 keys: a 4 MiB hash table (2^19 slots); the bitmap of span 2^25 - 1 is exactly 4 MiB
    n = (1 << 17) + 1
    base = np.arange(n - 1, dtype=np.int64) - 1000
    at = conn.keyset(np.append(base, -1000 + (1 << 25) - 1)).info
    assert (at.count, at.form, at.device_bytes) == (n, BITMAP, 4 << 20)
    past = conn.keyset(np.append(base, -1000 + (1 << 25))).info
    assert (past.count, past.form, past.device_bytes, past.capacity) == (n, HASH, 4 << 20, 1 << 19)
    # one value past a span of 2^32 values auto cannot take the bitmap (test_limits: forcing it is FLS_ERR_LIMIT)
    assert conn.keyset([0, 1 << 32]).info.form == HASH


@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("form", [0, BITMAP, HASH])
def test_contains_equals_python_membership(fl, conn, signed, form):
    rng = np.random.default_rng(3 + form)
    lo, hi = (-(1 << 63), (1 << 63) - 1) if signed else (0, M64)
    edge = [0, -1 if signed else M64, (M64 - 1) if not signed else -2, lo, hi]
    sets = [
        [int(x) for x in rng.integers(-3000, 3000, 2000)] if signed else [int(x) for x in rng.integers(0, 6000, 2000)],
        [lo + int(x) for x in rng.integers(0, 5000, 700)],                      # near the type's minimum
        [hi - int(x) for x in rng.integers(0, 5000, 700)],                      # every early sentinel candidate
        [hi - i for i in range(40)],                                            # ~0, ~0 - 1, ... taken (unsigned)
        [-1 - i for i in range(40)] if signed else [0],                         # ... and as signed keys
    ]
    if form != BITMAP:                                                          # wider than a bitmap may be
        sets += [edge, [hi - i for i in range(40)] + [lo],
                 [int(x) - (1 << 63 if signed else 0) for x in rand64(rng, 3000)]]
    for vals in sets:
        ks = conn.keyset(vals, signed=signed, form=form)
        ref = {v & M64 for v in vals}
        assert ks.info.count == len(ref)
        if ks.info.form == HASH:
            assert ks.info.empty not in ref and all(e in ref for e in range(M64, ks.info.empty, -1))
        probes = set(edge) | {v + d for v in vals[:300] for d in (-1, 0, 1)} | {int(x) for x in rand64(rng, 200)}
        probes.add(ks.info.empty)
        for p in probes:
            assert ks.contains(p) == ((p & M64) in ref), (form, signed, p)
        ks.close()


@pytest.mark.parametrize("home", [5, 127])
def test_colliding_keys_probe_as_long_as_the_set(fl, conn, home):
    """50 keys sharing one home slot of the 128-slot table (built from the
    documented hash): the longest probe is the set size; home 127 wraps past
    the end of the table"""
    keys = colliding_keys(50, 7, home)
    assert len(set(keys)) == 50 and all(((k * HASH_MUL) & M64) >> 57 == home for k in keys)
    ks = conn.keyset(keys, signed=False, form=HASH)
    assert (ks.info.capacity, ks.info.max_probe) == (128, 50)
    assert all(ks.contains(k) for k in keys)
    others = colliding_keys(80, 7, home)[50:]                                    # same home, not in the set
    assert not any(ks.contains(k) for k in others)
    assert not ks.contains(ks.info.empty)


def test_limits(fl, conn):
    import ctypes as C
    h = C.c_void_p()
    with pytest.raises(fl.FlsError) as e:                                        # n is checked before keys is read
        fl._check(fl.lib.fls_keyset_create(conn.h, None, fl.MAX_KEYSET_KEYS + 1, 0, 0, C.byref(h)))
    assert e.value.code == ERR_LIMIT and "kMaxKeysetKeys" in str(e.value)
    with pytest.raises(fl.FlsError) as e:
        conn.keyset([0, 1 << 32], form=BITMAP)
    assert e.value.code == ERR_LIMIT and "2^32" in str(e.value)
    with pytest.raises(fl.FlsError) as e:
        conn.keyset([1], form=3)
    assert e.value.code == ERR_ARG
    # a float is never truncated into a key
    for bad in ([1, 1.7], np.array([1.0, 2.0]), ["3"], [None]):
        with pytest.raises(TypeError, match="keyset"):
            conn.keyset(bad)
    assert conn.keyset([True, np.int8(-1), np.uint64(M64)], signed=False).info.count == 2      # 1 and ~0


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


def test_argument_errors_name_the_term_before_any_device_work(fl, conn, typed):
    t = typed
    sg, us = conn.keyset([1, 2, 3]), conn.keyset([1, 2, 3], signed=False)
    for op in ("in_set", "not_in_set"):
        for col in (2, 3, 4, 7):                                                 # VARCHAR, FLOAT, DOUBLE, BLOB
            with pytest.raises(fl.FlsError, match=r"filter term 1: .*VARCHAR / BLOB / FLOAT / DOUBLE") as e:
                t.set_filter([(0, "<", 5), (col, op, sg)])
            assert e.value.code == ERR_ARG
        with pytest.raises(fl.FlsError, match=r"filter term 0: the key set's kind is unsigned, column 0 is signed"):
            t.set_filter([(0, op, us)])
        with pytest.raises(fl.FlsError, match=r"filter term 0: the key set's kind is signed, column 1 is unsigned"):
            t.may_match(0, [(1, op, sg)])
        with pytest.raises(fl.FlsError, match=r"filter term 1: .*shares clause 7 with term 0"):
            t.set_filter([(0, "=", 3, 7), (0, op, sg, 7)])
        with pytest.raises(fl.FlsError, match=r"filter term 0: .*shares clause 7"):
            t.set_filter([(0, op, sg, 7), (5, op, sg, 7)])
        with pytest.raises(fl.FlsError, match=r"filter term 0: .*DECIMAL wider than 64 bits \(column 6\)") as e:
            t.set_filter([(6, op, sg)])                                          # DECIMAL(20, 2)
        assert e.value.code == ERR_ARG
        with pytest.raises(fl.FlsError, match=r"filter term 1: .*DECIMAL wider than 64 bits \(column 6\)"):
            t.may_match(0, [(0, "<", 5), (6, op, sg)])
    with pytest.raises(fl.FlsError, match="filter operator 11 unknown"):
        t.set_filter([(0, 11, 0)])
    # a DECIMAL of at most 64 bits is accepted
    t.set_filter([(5, "in_set", sg), (0, "not_in_set", sg), (1, "in_set", us)])
    t.set_filter([])


def test_stale_and_garbage_handles_are_refused(fl, conn, typed):
    t = typed
    ks = conn.keyset([1, 2, 3])
    h = ks.h
    assert t.may_match(0, [(0, "in_set", ks)])
    ks.close()
    ks.close()                                                                   # idempotent
    for value in (h, 0, 1, 0xDEADBEEF, id(t), M64):
        with pytest.raises(fl.FlsError, match="filter term 0: .*not a live key set") as e:
            t.set_filter([(0, "in_set", value)])
        assert e.value.code == ERR_ARG
    fl.lib.fls_keyset_free(h)                                                    # a stale free is a no-op
    import ctypes as C
    assert fl.lib.fls_keyset_contains(h, 1) == ERR_ARG
    assert fl.lib.fls_keyset_info(0xDEADBEEF, C.byref(fl.KeySetInfo())) == ERR_ARG
    # the sets of a closed connection are gone with it
    c2 = fl.Connection([0])
    k2 = c2.keyset([1])
    c2.close()
    with pytest.raises(fl.FlsError, match="not a live key set"):
        t.set_filter([(0, "in_set", k2.h)])
    k2.h = None


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


def test_pruning_exact_on_sorted_conservative_on_unsorted(fl, conn, prunetab):
    t, cols, valid = prunetab
    rng = np.random.default_rng(4)
    srt = cols[0]
    sets = [S(conn, srt[[3, 4, 2 * RG + 7]]), S(conn, [int(srt[RG - 1]), int(srt[RG])]), S(conn, [int(srt[-1])]),
            S(conn, [int(srt[0]) - 1, int(srt[-1]) + 1]), S(conn, rng.choice(srt, 40), form=HASH),
            S(conn, srt[RG:RG + 300] + 1, form=BITMAP)]
    for s in sets:
        for rg in range(t.nrowgroups):
            sl = slice(rg * RG, (rg + 1) * RG)
            lo, hi = int(srt[sl].min()), int(srt[sl].max())
            has = any(lo <= v <= hi for v in s.values)
            assert t.may_match(rg, [(0, "in_set", s.ks)]) == has, (s.values[:4], rg)      # exactly [min, max]
            hit = np.isin(srt[sl], s.values).any()
            assert has or not hit
            if not t.may_match(rg, [(1, "in_set", s.ks)]):                                 # conservative
                assert not np.isin(cols[1][sl], s.values).any()
            assert t.may_match(rg, [(0, "not_in_set", s.ks)])
            # the all-NULL chunk matches neither operator; NOT IN prunes nothing else
            assert t.may_match(rg, [(2, "not_in_set", s.ks)]) == (rg != 2)
            assert t.may_match(rg, [(2, "in_set", s.ks)]) == (rg != 2 and any(
                int(srt[sl][valid[2][sl]].min()) <= v <= int(srt[sl][valid[2][sl]].max()) for v in s.values))


def test_empty_set_prunes_everything_without_a_gpu(fl, conn, prunetab):
    t, cols, valid = prunetab
    for form in (0, BITMAP, HASH):
        e = conn.keyset([], form=form)
        filt = [(0, "in_set", e)]
        assert not any(t.may_match(rg, filt) for rg in range(t.nrowgroups))
        assert list(t.scan_filtered(filt)) == [] and t.pruned == t.nrowgroups
        assert t.aggregate([("count",), ("sum", 0), ("min", 1)], filt) == [0, None, None]
        assert t.aggregate_grouped([0], [("count",)], filt) == []
        rows, values, _ = t.topn(0, 10, filt=filt)
        assert len(rows) == 0 and len(values[0]) == 0
    # a set with no key in any zone map prunes everything as well
    far = conn.keyset([int(cols[0][-1]) + 5, int(cols[0][0]) - 5])
    assert list(t.scan_filtered([(0, "in_set", far), (1, ">", 0)])) == [] and t.pruned == t.nrowgroups


def test_keyset_kernel_resources():
    """keyset_kernel: no scratch, no spill, at most 64 VGPRs (eight waves per
    SIMD) and the four wave counts in LDS"""
    if not LIB.exists():
        pytest.skip("libflsgpu.so not built")
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    res = kernel_resources.resources(str(LIB))
    hits = {k: v for k, v in res.items() if "keyset_kernel" in k}
    assert len(hits) == 1, sorted(res)
    for name, r in hits.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 64 and r["lds"] <= 16, (name, r)


def test_keyset_construction_under_asan(tmp_path):
    """tests/fuzz/fuzz_keyset.cpp, a stand-alone program over the host-only
    header, built with -fsanitize=address,undefined: seeded random and
    adversarial sets, contains against std::set"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path / "fuzz_keyset"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", str(CSRC), str(ROOT / "tests" / "fuzz" / "fuzz_keyset.cpp"),
                    "-o", str(out)], check=True)
    r = subprocess.run([str(out), "150", "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"sanitizer report or mismatch\n{r.stderr[-4000:]}"
    assert r.stdout.startswith("iterations 150 failures 0"), r.stdout


# ------------------------------------------------------------------ GPU tests
KEY_TYPES = ["INT8", "INT16", "INT32", "INT64", "UINT8", "UINT16", "UINT32", "UINT64", "BOOLEAN", "DATE", "DECIMAL"]


def type_range(fl, name):
    if name == "BOOLEAN":
        return 0, 1
    if name == "DECIMAL":
        return -(10 ** 15) + 1, 10 ** 15 - 1
    info = np.iinfo(fl.NP_DTYPE[getattr(fl, name)])
    return int(info.min), int(info.max)


def key_pool(fl, name, rng):
    """the values a key column draws from: clusters at the type's minimum, its
    maximum and around 0 / -1, so that sets of either form can hold the edges"""
    lo, hi = type_range(fl, name)
    if name == "BOOLEAN":
        return [0, 1]
    mid = [v for v in (-2, -1, 0, 1, 2, 77) if lo <= v <= hi]
    if hi - lo < 1 << 16:                                       # 8- and 16-bit types: a sample of the range
        return sorted({lo, lo + 1, hi - 1, hi, *mid, *[int(x) for x in rng.integers(lo, hi + 1, 40)]})
    return sorted({*[lo + int(x) for x in rng.integers(0, 3000, 20)], lo, lo + 1,
                   *[hi - int(x) for x in rng.integers(0, 3000, 20)], hi, hi - 1, *mid,
                   *[int(x) for x in rng.integers(max(lo, -3000), 3000, 20)]})


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
    t = conn.read_image(fl.write_image(specs, rowgroup=RG))
    yield t, cols, pools
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["in_set", "not_in_set"])
@pytest.mark.parametrize("form", [BITMAP, HASH])
@pytest.mark.parametrize("name", KEY_TYPES)
def test_gpu_every_key_type_against_isin(fl, gpu, conn, typetab, name, form, op):
    t, cols, pools = typetab
    c = KEY_TYPES.index(name)
    lo, hi = type_range(fl, name)
    signed = lo < 0
    pool = pools[c]
    rng = np.random.default_rng(c)
    half = [v for v in pool if rng.random() < 0.5]
    absent = [v for v in (lo + 5, hi - 5, 3, 1234) if lo <= v <= hi and v not in pool]
    edges = [lo, hi] + ([-1 if signed else hi] if hi - lo >= (1 << 63) else [])
    if form == HASH or hi - lo < 1 << 32:
        groups = [half + absent + edges]
    else:
        # a bitmap spans at most 2^32 values: the minimum, the maximum and -1 / ~0 each in a set of its own cluster
        groups = [[v for v in half + absent + edges if v - lo < 1 << 20],
                  [v for v in half + absent + edges if hi - v < 1 << 20],
                  [v for v in half + absent + [-1 if signed else 0] if abs(v) < 1 << 20]]
    for vals in groups:
        s = S(conn, vals, signed=signed, form=form)
        assert s.ks.info.form == form
        want = check_scan(fl, t, cols, [(c, op, s)], deliver=[c])
        assert 0 < len(want) < N or name == "BOOLEAN"
        s.ks.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [BITMAP, HASH])
def test_gpu_every_encoding_of_the_key_column(fl, gpu, conn, form):
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
    cols = {0: ffor, 1: delta, 2: dic, 3: rle}
    try:
        for c in cols:
            present = np.unique(cols[c])
            some = max(1, min(len(present) // 2, 60))            # (the DICT column has nine distinct values)
            vals = [int(v) for v in rng.choice(present, some, replace=False)] + [int(present[0]) - 1]
            s = S(conn, vals, form=form)
            for op in ("in_set", "not_in_set"):
                want = check_scan(fl, t, cols, [(c, op, s)], deliver=[c])
                assert 0 < len(want) < N
    finally:
        t.close()


@pytest.fixture(scope="module")
def nulltab(fl, conn):
    """column 0: NULLs everywhere (the placeholder stored at a NULL row is 0);
    column 1: NULLs in row groups 1 and 3 only, so a batch mixes row groups
    with and without validity; column 2: no NULL; column 3: a row id"""
    rng = np.random.default_rng(41)
    a = rng.integers(-30, 30, N).astype(np.int32)
    b = rng.integers(0, 60, N).astype(np.uint16)
    c = rng.integers(-5, 6, N).astype(np.int8)
    na = rng.random(N) < 0.3
    nb = np.zeros(N, bool)
    nb[RG:2 * RG] = rng.random(RG) < 0.5
    nb[3 * RG:4 * RG] = rng.random(RG) < 0.5
    ids = np.arange(N, dtype=np.int32)
    t = conn.read_image(fl.write_image([("a", fl.INT32, np.ma.masked_array(a, mask=na), fl.ENC_AUTO),
                                        ("b", fl.UINT16, np.ma.masked_array(b, mask=nb), fl.ENC_AUTO),
                                        ("c", fl.INT8, c, fl.ENC_AUTO), ("id", fl.INT32, ids, fl.ENC_AUTO)],
                                       rowgroup=RG))
    # what the engine decodes at a NULL row is the writer's placeholder
    yield t, {0: np.where(na, 0, a).astype(np.int32), 1: np.where(nb, 0, b).astype(np.uint16), 2: c, 3: ids}, \
        {0: ~na, 1: ~nb}
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [BITMAP, HASH])
def test_gpu_null_rows_satisfy_neither_operator(fl, gpu, conn, nulltab, form, monkeypatch):
    t, cols, valid = nulltab
    sa = S(conn, [0, -7, 3, 29, 1000], form=form)                # 0: the placeholder at the NULL rows
    sb = S(conn, [0, 1, 17, 59], signed=False, form=form)
    assert t.validity(0, 1) is None and t.validity(1, 1) is not None
    for batch in ("1", "8"):
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)              # 8: one batch mixes row groups with / without validity
        for term in [(0, "in_set", sa), (0, "not_in_set", sa), (1, "in_set", sb), (1, "not_in_set", sb)]:
            want = check_scan(fl, t, cols, [term], valid, deliver=[3])
            assert valid[term[0]][want].all() and 0 < len(want) < N
        inn = check_scan(fl, t, cols, [(0, "in_set", sa)], valid)
        out = check_scan(fl, t, cols, [(0, "not_in_set", sa)], valid)
        assert len(inn) + len(out) == int(valid[0].sum())        # the NULL rows are in neither


@pytest.mark.gpu
@pytest.mark.parametrize("form", [BITMAP, HASH])
def test_gpu_set_terms_combined_with_other_terms(fl, gpu, conn, nulltab, form):
    t, cols, valid = nulltab
    sa = S(conn, [int(x) for x in range(-30, 30, 3)], form=form)
    sb = S(conn, [0, 5, 6, 7, 40, 41], signed=False, form=form)
    sc = S(conn, [-5, 0, 5], form=form)
    cases = [
        [(0, "in_set", sa), (2, ">", 0)],                                         # a set term with ordinary terms
        [(2, "<", 0, 1), (2, ">", 3, 1), (0, "not_in_set", sa), (1, "is_not_null", None)],
        [(0, "in_set", sa), (1, "in_set", sb)],                                   # two set terms on two columns
        [(0, "in_set", sa), (1, "not_in_set", sb), (2, "in_set", sc)],            # set terms only
        [(2, "in_set", sc)],
        # the skip path: ordinary terms that reject whole 64-row words and whole vectors
        [(3, ">=", 64), (3, "<", 1024 + 128, 1), (3, ">=", 3 * 1024, 1), (0, "in_set", sa)],
        [(3, ">=", 2 * 1024 + 64), (3, "<", 2 * 1024 + 128), (2, "not_in_set", sc)],
        [(3, "<", 0), (0, "in_set", sa)],                                         # nothing left for the set
        [(3, ">=", N - 5), (2, "not_in_set", sc)],                                # the partial tail only
    ]
    for terms in cases:
        check_scan(fl, t, cols, terms, valid, deliver=[2, 3])


@pytest.mark.gpu
@pytest.mark.parametrize("home", [5, 127])
def test_gpu_colliding_keys(fl, gpu, conn, home):
    keys = colliding_keys(50, 7, home)
    others = colliding_keys(90, 7, home)[50:]
    rng = np.random.default_rng(51)
    pool = np.array(keys + others + [0, M64], dtype=np.uint64)
    vals = pool[rng.integers(0, len(pool), N)]
    s = S(conn, keys, signed=False, form=HASH)
    assert s.ks.info.max_probe == 50
    t = conn.read_image(fl.write_image([("k", fl.UINT64, vals, fl.ENC_AUTO)], rowgroup=RG))
    try:
        for op in ("in_set", "not_in_set"):
            want = check_scan(fl, t, {0: vals}, [(0, op, s)], deliver=[0])
            assert 0 < len(want) < N
    finally:
        t.close()


@pytest.fixture(scope="module")
def facttab(fl, conn):
    """a small fact table: key, low-cardinality group, measures, a nullable measure"""
    rng = np.random.default_rng(61)
    key = np.sort(rng.integers(0, 4000, N)).astype(np.int64)
    grp = rng.integers(0, 5, N).astype(np.int8)
    qty = rng.integers(1, 51, N).astype(np.int32)
    price = rng.integers(100, 10 ** 7, N).astype(np.int64)
    disc = rng.integers(0, 11, N).astype(np.int64)
    nm = rng.random(N) < 0.2
    t = conn.read_image(fl.write_image([("key", fl.INT64, key, fl.ENC_AUTO), ("grp", fl.INT8, grp, fl.ENC_AUTO),
                                        ("qty", fl.INT32, np.ma.masked_array(qty, mask=nm), fl.ENC_AUTO),
                                        ("price", fl.DECIMAL, price, fl.ENC_AUTO, 15, 2),
                                        ("disc", fl.DECIMAL, disc, fl.ENC_AUTO, 15, 2)], rowgroup=RG))
    yield t, {0: key, 1: grp, 2: qty, 3: price, 4: disc}, {2: ~nm}
    t.close()


def numpy_aggs(cols, valid, m):
    q = m & valid[2]
    price, disc = cols[3].astype(object), cols[4].astype(object)
    return [int(m.sum()), int(q.sum()), int(cols[2][q].astype(np.int64).sum()) if q.any() else None,
            int(cols[3][m].min()) if m.any() else None, int(cols[0][m].max()) if m.any() else None,
            int((price[m] * (100 - disc[m])).sum()) if m.any() else None]


AGGS = [("count",), ("count", 2), ("sum", 2), ("min", 3), ("max", 0), ("sum_expr", [(0, 1, 3), (100, -1, 4)])]


@pytest.mark.gpu
@pytest.mark.parametrize("form", [BITMAP, HASH])
def test_gpu_downstream_calls_under_a_set_term(fl, gpu, conn, facttab, form):
    t, cols, valid = facttab
    rng = np.random.default_rng(62)
    s = S(conn, rng.choice(4000, 900, replace=False), form=form)
    for terms in ([(0, "in_set", s)], [(0, "not_in_set", s), (1, "!=", 2)], [(0, "in_set", s), (2, "is_null", None)]):
        m = isin_mask(cols, terms, N, valid)
        assert t.aggregate(AGGS, eng(terms)) == numpy_aggs(cols, valid, m), terms
        # grouped: groups in order of first occurrence, values as the ungrouped call over the group's rows
        got = t.aggregate_grouped([1], AGGS, eng(terms))
        order = [int(g) for g in dict.fromkeys(cols[1][m].tolist())]
        assert [k for k, _ in got] == [(g,) for g in order], terms
        for (g,), vals in got:
            assert vals == numpy_aggs(cols, valid, m & (cols[1] == g)), (terms, g)
        # top-N: rows and delivered values
        for desc in (False, True):
            rows, values, _ = t.topn(3, 100, cols=[0, 3], filt=eng(terms), desc=desc)
            cand = np.nonzero(m)[0]
            k = cols[3][cand].astype(np.int64)
            order = cand[np.lexsort((cand, -k if desc else k))][:100]
            assert np.array_equal(rows.astype(np.int64), order), (terms, desc)
            assert np.array_equal(values[0], cols[0][order]) and np.array_equal(values[3], cols[3][order])


@pytest.mark.gpu
def test_gpu_results_identical_across_batches_slots_and_gpus(fl, gpu, conn, facttab, monkeypatch):
    t, cols, valid = facttab
    rng = np.random.default_rng(63)
    sets = [S(conn, rng.choice(4000, 700, replace=False), form=form) for form in (BITMAP, HASH)]
    img_terms = [[(0, "in_set", sets[0]), (1, "not_in_set", S(conn, [1, 3]))], [(0, "not_in_set", sets[1])]]
    want = [np.nonzero(isin_mask(cols, terms, N, valid))[0] for terms in img_terms]
    ref_aggs = [numpy_aggs(cols, valid, isin_mask(cols, terms, N, valid)) for terms in img_terms]
    for batch, slots in (("1", "1"), ("3", "2"), ("8", "2"), ("2", "3")):
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)
        monkeypatch.setenv("FLS_SCAN_SLOTS", slots)
        for terms, w, a in zip(img_terms, want, ref_aggs):
            assert np.array_equal(scan_rows(t, terms)[0], w), (batch, slots)
            assert t.aggregate(AGGS, eng(terms)) == a, (batch, slots)
    monkeypatch.delenv("FLS_SCAN_BATCH")
    monkeypatch.delenv("FLS_SCAN_SLOTS")
    # every visible GPU: the row groups are sharded over them, so the set's image reaches each device
    devs = list(range(gpu))
    call = fl.Connection(devs)
    try:
        # the same file on the multi-GPU connection, with sets of that connection
        img = fl.write_image([("key", fl.INT64, cols[0], fl.ENC_AUTO), ("grp", fl.INT8, cols[1], fl.ENC_AUTO)],
                             rowgroup=RG)
        tm = call.read_image(img)
        sm = S(call, sets[1].values, form=HASH)
        for op in ("in_set", "not_in_set"):
            m = isin_mask(cols, [(0, op, sm)], N)
            assert np.array_equal(scan_rows(tm, [(0, op, sm)])[0], np.nonzero(m)[0]), (op, devs)
            assert tm.aggregate([("count",), ("sum", 0)], eng([(0, op, sm)])) == \
                [int(m.sum()), int(cols[0][m].sum())], (op, devs)
        tm.close()
    finally:
        call.close()


@pytest.mark.gpu
def test_gpu_one_set_serves_two_tables_and_survives_its_handle(fl, gpu, conn):
    rng = np.random.default_rng(71)
    a = rng.integers(0, 500, N).astype(np.int32)
    b = rng.integers(0, 500, 2 * RG + 77).astype(np.int64)
    ta = conn.read_image(fl.write_image([("a", fl.INT32, a, fl.ENC_AUTO)], rowgroup=RG))
    tb = conn.read_image(fl.write_image([("b", fl.INT64, b, fl.ENC_AUTO)], rowgroup=RG))
    try:
        s = S(conn, rng.choice(500, 120, replace=False), form=HASH)
        for _ in range(2):                                                       # the cached image is reused
            assert np.array_equal(scan_rows(ta, [(0, "in_set", s)])[0], np.nonzero(np.isin(a, s.values))[0])
            assert np.array_equal(scan_rows(tb, [(0, "not_in_set", s)])[0], np.nonzero(~np.isin(b, s.values))[0])
        # freed after set_filter and before the scan: the filter holds a reference
        ta.set_filter([(0, "in_set", s.ks)])
        tb.set_filter([(0, "in_set", s.ks)])
        s.ks.close()
        with pytest.raises(fl.FlsError, match="not a live key set"):
            fl._check(fl.lib.fls_keyset_contains(0, 1))
        rows = []
        import ctypes as C
        fl._check(fl.lib.fls_scan_begin(ta.h, None, 0, ta.nrowgroups))
        out = fl.RowGroup()
        while fl._check(fl.lib.fls_scan_next(ta.h, C.byref(out))) == 1:
            sel = np.ctypeslib.as_array(out.sel, shape=(out.nrows,)).copy() if out.nrows else np.zeros(0, np.uint32)
            rows.append(sel.astype(np.int64) + out.first_row)
        assert np.array_equal(np.concatenate(rows), np.nonzero(np.isin(a, s.values))[0])
        assert tb.aggregate_raw([("count",)])[0].lo == int(np.isin(b, s.values).sum())
        ta.set_filter([])
        tb.set_filter([])
    finally:
        ta.close()
        tb.close()


C_OKEY, C_PRICE, C_SHIPDATE = 0, 5, 10


@pytest.mark.gpu
def test_gpu_lineitem_semi_join(fl, gpu, conn):
    """the build side from a filtered scan of the table itself (Table.keyset),
    then the aggregate under it: TPC-H Q3's shape on a few row groups"""
    wl, sf = "lineitem", 0.05
    t = conn.read_image(fl.gen_image(wl, sf))
    try:
        n = t.nrows
        assert 4 <= t.nrowgroups <= 8
        okey = fl.gen_values(wl, C_OKEY, 0, n, np.int64, sf)
        price = fl.gen_values(wl, C_PRICE, 0, n, np.int64, sf)
        ship = fl.gen_values(wl, C_SHIPDATE, 0, n, np.int32, sf)
        cut_key, day = int(okey[n // 3]), 9000
        build = [(C_OKEY, "<", cut_key), (C_SHIPDATE, "<", day)]
        for form in (0, BITMAP, HASH):
            ks = t.keyset(C_OKEY, build, form=form)
            keys = np.unique(okey[(okey < cut_key) & (ship < day)])
            assert ks.info.count == len(keys) and as_signed(ks.info.min) == keys[0] and ks.info.max == keys[-1]
            m = np.isin(okey, keys)
            got = t.aggregate([("count",), ("sum", C_PRICE)], [(C_OKEY, "in_set", ks), (C_SHIPDATE, ">=", day)])
            mm = m & (ship >= day)
            assert got == [int(mm.sum()), int(price[mm].sum())] and got[0] > 0
            # the keys are sorted in the file: the row groups past the build side's range hold no key
            without = sum(not np.isin(okey[r * fl.ROWGROUP:(r + 1) * fl.ROWGROUP], keys).any()
                          for r in range(t.nrowgroups))
            assert t.aggregate([("count",)], [(C_OKEY, "in_set", ks)]) == [int(m.sum())]
            assert t.pruned == without and without >= 2
            ks.close()
    finally:
        t.close()
