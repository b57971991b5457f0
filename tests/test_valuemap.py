"""Value maps and map filter terms (`col op map[key]`):
the host construction (csrc/fls_valuemap.hpp through fls_valuemap_*), the
argument checks of the terms and their row-group pruning -- all without a GPU
-- and mapcmp_kernel on the GPU through every consumer, against a dict / numpy
restatement written here (never against the code under test).

Small shapes throughout: 4096-row row groups, two whole ones and a last one of
one full vector plus a 37-row partial word; a `pick` column empties several
64-row words and one whole vector before the map term runs."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from helpers import chunk_encodings, filter_mask, rand64
from test_keyset import KEY_TYPES, as_signed, colliding_keys, key_pool, type_range

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "duckdb-fastlane_amd" / "csrc"
RG = 4096
N = 2 * RG + 1061                 # 1061 = one full vector + 37 rows
M64 = (1 << 64) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
HASH_MUL = 0x9E3779B97F4A7C15
ERR_ARG, ERR_DEVICE, ERR_LIMIT = -3, -4, -8
DENSE, HASH = 1, 2
CMP = ["=", "!=", "<", "<=", ">", ">="]
PYOP = {"=": lambda a, b: a == b, "!=": lambda a, b: a != b, "<": lambda a, b: a < b, "<=": lambda a, b: a <= b,
        ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}
SIGNED_TYPES = ("INT8", "INT16", "INT32", "INT64", "DATE", "DECIMAL")


# ---- the header's two size formulas, restated
def dense_bytes(span):
    return 8 * (span + 1) + 8 * ((span + 64) // 64)


def hash_capacity(n):
    cap = 1
    while cap < 2 * n:
        cap *= 2
    return cap


def hash_bytes(n):
    return 16 * hash_capacity(n)


def largest_span_within(limit):
    """the largest span whose dense image is at most `limit` bytes"""
    span = limit // 8
    while dense_bytes(span) > limit:
        span -= 1
    assert dense_bytes(span) <= limit < dense_bytes(span + 1)
    return span


# ---- the reference: a Python dict over the generated columns
class VM:
    """a value map and the dict it was made of"""

    def __init__(self, conn, d, signed=True, value_signed=True, form=0):
        self.d = {int(k): int(v) for k, v in dict(d).items()}
        self.value_signed = value_signed
        self.vm = conn.valuemap(list(self.d), list(self.d.values()), signed=signed, value_signed=value_signed, form=form)


def looked_up(key, d, value_signed):
    """(present, value) per row of the key column: the dict lookup, once per map"""
    dt = np.int64 if value_signed else np.uint64
    present = np.zeros(len(key), bool)
    val = np.zeros(len(key), dt)
    for i, k in enumerate(key.tolist()):
        b = d.get(int(k))
        if b is not None:
            present[i] = True
            val[i] = b
    return present, val


def map_mask(left, key, m, op, vl=None, vk=None):
    """rows where left and key are valid, the key is in the map and left op map[key]"""
    present, val = looked_up(key, m.d, m.value_signed)
    a = left.astype(np.int64 if m.value_signed else np.uint64)
    hit = present & PYOP[op](a, val)
    if vl is not None:
        hit &= vl
    if vk is not None:
        hit &= vk
    return hit


def scan_rows(t, terms):
    rows = [sel.astype(np.int64) + first for _, first, sel, _ in t.scan_filtered(terms, cols=[0])]
    return np.concatenate(rows) if rows else np.zeros(0, np.int64)


def pick_column():
    """1 everywhere but one whole vector and several 64-row words"""
    pick = np.ones(N, np.int8)
    pick[1024:2048] = 0                                   # one vector fully deselected
    for w in (0, 3, 17, 64 + 5, 64 + 6, 128 + 15, 128 + 16):   # 64-row words, the 37-row last one included (word 144)
        pick[64 * w:64 * w + 64] = 0
    pick[N - 37:] = 1
    pick[N - 37 + 5] = 0
    return pick


@pytest.fixture(scope="module")
def conn(fl):
    c = fl.Connection([0])
    yield c
    c.close()


# ------------------------------------------------------------------ CPU tests
def test_library_exports_the_valuemap_functions(fl):
    for name in ("fls_valuemap_create", "fls_valuemap_free", "fls_valuemap_info", "fls_valuemap_lookup"):
        assert hasattr(fl.lib, name), name
    assert (fl.VALUEMAP_AUTO, fl.VALUEMAP_DENSE, fl.VALUEMAP_HASH) == (0, 1, 2)
    assert [fl.OPS["map" + op] for op in CMP] == [19, 20, 21, 22, 23, 24]
    assert repr(fl.Mapped(3, None)) == "Mapped(3, None)"


def test_the_predicate_keeps_its_size_and_offsets(fl, tmp_path):
    """key_col is the tail of what was pad[7]: sizeof(fls_predicate) and the
    offsets of value, str and str_len are what they were, in ctypes and in C"""
    P = fl.Predicate
    assert C.sizeof(P) == 40
    assert (P.col.offset, P.clause.offset, P.op.offset, P.key_col.offset) == (0, 4, 8, 12)
    assert (P.value.offset, P.str.offset, P.str_len.offset) == (16, 24, 32)
    if shutil.which("gcc") is None:
        return
    src = tmp_path / "pred.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "flsgpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(fls_predicate), '
                   'offsetof(fls_predicate, op), offsetof(fls_predicate, key_col), offsetof(fls_predicate, value), '
                   'offsetof(fls_predicate, str), offsetof(fls_predicate, str_len)); return 0; }\n')
    exe = tmp_path / "pred"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [40, 8, 12, 16, 24, 32]


@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("form", [0, DENSE, HASH])
def test_lookup_equals_a_python_dict(fl, conn, signed, form):
    rng = np.random.default_rng(3 + form)
    lo, hi = (I64_MIN, I64_MAX) if signed else (0, M64)
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
    special = [0, I64_MIN & M64, I64_MAX, M64]                                  # as patterns
    for value_signed in (True, False):
        for keys in sets:
            ref = {k & M64: ((int(k) * 0x9E3779B1 + 7) & M64) for k in keys}
            for j, k in enumerate(list(ref)[:8]):
                ref[k] = special[j % 4]                                         # 0 at a present key among them
            pat = lambda v: as_signed(v) if value_signed else v                 # noqa: E731
            m = conn.valuemap(list(ref), [pat(v) for v in ref.values()], signed=signed, value_signed=value_signed,
                              form=form)
            info = m.info
            assert info.count == len(ref) and (form == 0 or info.form == form)
            assert info.key_kind == (0 if signed else 1) and info.value_kind == (0 if value_signed else 1)
            vs = [pat(v) for v in ref.values()]
            assert (pat(info.value_min), pat(info.value_max)) == (min(vs), max(vs))
            if info.form == HASH:
                assert info.empty not in ref and all(e in ref for e in range(M64, info.empty, -1))
                assert info.device_bytes == 16 * info.capacity == hash_bytes(len(ref))
            else:
                assert info.device_bytes == dense_bytes((info.key_max - info.key_min) & M64) and info.capacity == 0
            probes = set(edge) | {k + d for k in keys[:300] for d in (-1, 0, 1)} | {int(x) for x in rand64(rng, 200)}
            probes |= {info.empty, info.key_min - 1, info.key_max + 1}          # one outside [min, max]
            for p in probes:
                want = ref.get(p & M64)
                assert m.lookup(p) == (None if want is None else pat(want)), (form, signed, value_signed, p)
            zero = [k for k, v in ref.items() if v == 0]
            assert zero and all(m.lookup(k) == 0 for k in zero)                  # value 0 at a present key is found
            assert all(m.lookup(k) == pat(v) for k, v in ref.items())
            m.close()


def test_duplicates_conflicts_and_the_empty_map(fl, conn):
    for form in (0, DENSE, HASH):
        m = conn.valuemap([5, 1, 1, -1, 7, 7, 7], [3, -2, -2, 0, I64_MAX, I64_MAX, I64_MAX], form=form)
        assert m.info.count == 4                                                # an equal duplicate is kept once
        assert [m.lookup(k) for k in (5, 1, -1, 7, 0, 6)] == [3, -2, 0, I64_MAX, None, None]
        with pytest.raises(fl.FlsError, match=r"key 0x7 \(7\) is listed with the values 4 and 9") as e:
            conn.valuemap([5, 7, 1, 7], [3, 9, 2, 4], form=form)                # a map is a function
        assert e.value.code == ERR_ARG
        with pytest.raises(fl.FlsError, match=r"key 0xf+ \(-1\) .*values (-5 and 2|2 and -5)") as e:
            conn.valuemap([-1, -1], [2, -5], form=form)
        assert e.value.code == ERR_ARG
        with pytest.raises(fl.FlsError, match=r"key 0x3 \(3\) .*values 1 and 18446744073709551615"):
            conn.valuemap([3, 3], [M64, 1], value_signed=False, form=form)
        e = conn.valuemap([], [], form=form)                                    # n = 0: the empty map
        assert e.info.count == 0 and e.lookup(0) is None and e.lookup(-1) is None and (form == 0 or e.info.form == form)
        assert (e.info.value_min, e.info.value_max, e.info.key_min, e.info.key_max) == (0, 0, 0, 0)
    with pytest.raises(ValueError, match="2 keys and 1 values"):
        conn.valuemap([1, 2], [1])
    for bad in ([1.5], ["3"], [None]):                                          # a float is never truncated
        with pytest.raises(TypeError, match="valuemap"):
            conn.valuemap(bad, [1])
        with pytest.raises(TypeError, match="valuemap"):
            conn.valuemap([1], bad)
    hsh = conn.valuemap([5, 1, -1, 7, 1 << 40], [1, 2, 3, 4, 5], form=HASH).info
    assert (hsh.count, hsh.form, hsh.capacity, hsh.device_bytes) == (5, HASH, 16, 256)
    assert as_signed(hsh.key_min) == -1 and hsh.key_max == 1 << 40 and 1 <= hsh.max_probe <= 5 and hsh.empty == M64 - 1
    den = conn.valuemap([5, 1, -1, 7], [1, 2, 3, 4], form=DENSE).info
    assert (den.count, den.form, den.capacity, den.max_probe, den.device_bytes) == (4, DENSE, 0, 0, 9 * 8 + 8)   # 9 values, one presence word


def test_limits(fl, conn):
    h = C.c_void_p()
    one = (C.c_uint64 * 1)(1)
    with pytest.raises(fl.FlsError) as e:                                       # n is checked before the arrays are read
        fl._check(fl.lib.fls_valuemap_create(conn.h, one, one, fl.MAX_KEYSET_KEYS + 1, 0, 0, 0, C.byref(h)))
    assert e.value.code == ERR_LIMIT and "kMaxKeysetKeys" in str(e.value)
    with pytest.raises(fl.FlsError) as e:                                       # a span of 2^28 + 1 keys, two of them given
        conn.valuemap([0, 1 << 28], [1, 2], form=DENSE)
    assert e.value.code == ERR_LIMIT and "2^28" in str(e.value)
    with pytest.raises(fl.FlsError) as e:
        conn.valuemap([-5, (1 << 28) - 5], [1, 2], form=DENSE)
    assert e.value.code == ERR_LIMIT
    assert conn.valuemap([0, 1 << 28], [1, 2]).info.form == HASH                # auto cannot take the array there
    for kinds in ((2, 0, 0), (0, 2, 0), (0, 0, 3)):
        assert fl.lib.fls_valuemap_create(conn.h, one, one, 1, *kinds, C.byref(h)) == ERR_ARG


def test_auto_rule_at_both_boundaries_and_input_order(fl, conn):
    """auto takes the dense image (8 bytes per key of [min, max] plus one
    presence bit, in 8-byte words) when it is at most 1 MiB, or no larger than
    the hash image (16 bytes per slot): one key moved by one on either side of
    each bound flips the form; the cases come from the two size formulas"""
    # 3 keys: a 128-byte hash image (8 slots); the widest dense image within 1 MiB
    s1 = largest_span_within(1 << 20)
    at = conn.valuemap([10, 11, 10 + s1], [1, 2, 3]).info
    assert (at.form, at.device_bytes) == (DENSE, dense_bytes(s1)) and at.device_bytes <= 1 << 20
    past = conn.valuemap([10, 11, 10 + s1 + 1], [1, 2, 3]).info
    assert (past.form, past.device_bytes, past.capacity) == (HASH, hash_bytes(3), 8) and hash_bytes(3) == 128
    # 2^17 + 1 keys: 2^19 slots, an 8 MiB hash image; the widest dense image that is no larger
    n = (1 << 17) + 1
    assert hash_bytes(n) == 8 << 20
    s2 = largest_span_within(hash_bytes(n))
    assert s2 >= n and dense_bytes(s2) > 1 << 20
    base = np.arange(n - 1, dtype=np.int64) - 1000
    vals = (np.arange(n, dtype=np.int64) * 7) - 5
    at = conn.valuemap(np.append(base, -1000 + s2), vals).info
    assert (at.count, at.form, at.device_bytes) == (n, DENSE, dense_bytes(s2))
    past = conn.valuemap(np.append(base, -1000 + s2 + 1), vals).info
    assert (past.count, past.form, past.device_bytes, past.capacity) == (n, HASH, 8 << 20, 1 << 19)
    # info and every lookup do not depend on the input's order (the image's bytes: tests/fuzz/fuzz_valuemap.cpp)
    rng = np.random.default_rng(5)
    keys = [int(x) for x in np.unique(rng.integers(-4000, 4000, 1500))]
    vs = [k * k - 9 for k in keys]
    for form in (DENSE, HASH):
        a = conn.valuemap(keys, vs, form=form)
        p = rng.permutation(len(keys))
        b = conn.valuemap([keys[i] for i in p] + keys[:50], [vs[i] for i in p] + vs[:50], form=form)
        assert bytes(a.info) == bytes(b.info)
        assert all(a.lookup(k) == b.lookup(k) == v for k, v in zip(keys, vs))


@pytest.mark.parametrize("home", [5, 127])
def test_colliding_keys_probe_as_long_as_the_map(fl, conn, home):
    """50 keys sharing one home slot of the 128-slot table: the longest probe
    is their number, every one is found with its own value; home 127 wraps"""
    keys = colliding_keys(50, 7, home)
    assert len(set(keys)) == 50 and all(((k * HASH_MUL) & M64) >> 57 == home for k in keys)
    m = conn.valuemap(keys, [j * 1000 - 7 for j in range(50)], signed=False, form=HASH)
    assert (m.info.capacity, m.info.max_probe, m.info.device_bytes) == (128, 50, 2048)
    assert [m.lookup(k) for k in keys] == [j * 1000 - 7 for j in range(50)]
    others = colliding_keys(80, 7, home)[50:]                                    # same home, not in the map
    assert all(m.lookup(k) is None for k in others) and m.lookup(m.info.empty) is None


def test_valuemap_construction_under_asan(tmp_path):
    """tests/fuzz/fuzz_valuemap.cpp, a stand-alone program over the host-only
    header, built with -fsanitize=address,undefined: seeded random and
    adversarial maps, valuemap_lookup against std::map, the image's bytes"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path / "fuzz_valuemap"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", str(CSRC), str(ROOT / "tests" / "fuzz" / "fuzz_valuemap.cpp"),
                    "-o", str(out)], check=True)
    r = subprocess.run([str(out), "150", "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"sanitizer report or mismatch\n{r.stderr[-4000:]}"
    assert r.stdout.startswith("iterations 150 failures 0"), r.stdout


# columns of `typed`
T_I, T_U, T_S, T_F, T_D, T_W, T_X, T_B, T_DATE, T_BOOL = range(10)


@pytest.fixture(scope="module")
def typed(fl, conn):
    """one column per kind of type the argument checks tell apart"""
    n = 2 * 1024 + 100
    rng = np.random.default_rng(1)
    cols = [("i", fl.INT32, rng.integers(-50, 50, n).astype(np.int32), fl.ENC_AUTO),
            ("u", fl.UINT16, rng.integers(0, 50, n).astype(np.uint16), fl.ENC_AUTO),
            ("s", fl.VARCHAR, [f"s{i % 7}" for i in range(n)], fl.ENC_DICT),
            ("f", fl.FLOAT, rng.random(n).astype(np.float32), fl.ENC_AUTO),
            ("d", fl.DOUBLE, rng.random(n), fl.ENC_AUTO),
            ("w", fl.DECIMAL, rng.integers(0, 9, n).astype(np.int64), fl.ENC_AUTO, 15, 2),
            ("x", fl.DECIMAL, rng.integers(0, 9, n).astype(np.int64), fl.ENC_AUTO, 20, 2),
            ("b", fl.BLOB, [b"y%d" % (i % 5) for i in range(n)], fl.ENC_FSST),
            ("date", fl.DATE, rng.integers(9000, 9100, n).astype(np.int32), fl.ENC_AUTO),
            ("bool", fl.BOOLEAN, rng.integers(0, 2, n).astype(np.uint8), fl.ENC_AUTO)]
    t = conn.read_image(fl.write_image(cols, rowgroup=1024))
    yield t
    t.close()


def test_argument_errors_name_the_term_and_both_columns_before_any_device_work(fl, conn, typed):
    t = typed
    ss = conn.valuemap([1, 2, 3], [0, 1, 2])                                      # signed keys, signed values
    uu = conn.valuemap([1, 2, 3], [0, 1, 2], signed=False, value_signed=False)
    su = conn.valuemap([1, 2, 3], [0, 1, 2], signed=True, value_signed=False)     # signed keys, unsigned values
    us = conn.valuemap([1, 2, 3], [0, 1, 2], signed=False, value_signed=True)

    def refused(filt, pattern):
        with pytest.raises(fl.FlsError, match=pattern) as e:
            t.set_filter(filt)
        assert e.value.code == ERR_ARG
        if not any(isinstance(x, fl.AnyOf) for x in filt):
            with pytest.raises(fl.FlsError, match=pattern):                       # ... and through the pruning call
                t.may_match(0, filt)

    ok = (T_I, "<", 5)
    refused([ok, (T_I, "<", fl.Mapped(99, ss))], r"filter term 1: key column 99 out of range \(left column 0")
    for col in (T_S, T_F, T_D, T_B):                                              # VARCHAR, FLOAT, DOUBLE, BLOB
        refused([(col, "=", fl.Mapped(T_I, ss))],
                rf"filter term 0: .*VARCHAR / BLOB / FLOAT / DOUBLE column \(left column {col}, key column 0\)")
        refused([ok, (T_I, "=", fl.Mapped(col, ss))],
                rf"filter term 1: .*VARCHAR / BLOB / FLOAT / DOUBLE column \(left column 0, key column {col}\)")
    refused([(T_X, "<", fl.Mapped(T_I, ss))], r"filter term 0: .*DECIMAL wider than 64 bits \(left column 6, key column 0\)")
    refused([(T_I, "<", fl.Mapped(T_X, ss))], r"filter term 0: .*DECIMAL wider than 64 bits \(left column 0, key column 6\)")
    refused([(T_I, "<", fl.Mapped(T_I, su))], r"filter term 0: the value map's value kind is unsigned, left column 0 is signed")
    refused([(T_U, "<", fl.Mapped(T_I, ss))], r"filter term 0: the value map's value kind is signed, left column 1 is unsigned")
    refused([(T_BOOL, "<", fl.Mapped(T_I, ss))], r"value kind is signed, left column 9 is unsigned")
    refused([(T_I, "<", fl.Mapped(T_I, us))], r"filter term 0: the value map's key kind is unsigned, key column 0 is signed")
    refused([(T_I, "<", fl.Mapped(T_U, ss))], r"filter term 0: the value map's key kind is signed, key column 1 is unsigned")
    refused([(T_I, "<", fl.Mapped(T_I, ss), 4), (T_U, "=", 3, 4)],
            r"filter term 0: a map term shares clause 4 with term 1 .*left column 0, key column 0")
    refused([(T_U, "=", 3, 4), (T_I, "<", fl.Mapped(T_DATE, ss), 4)],
            r"filter term 1: a map term shares clause 4 with term 0 .*left column 0, key column 8")
    nine = [(T_I, op, fl.Mapped(T_I, ss)) for op in CMP] + [(T_W, "<", fl.Mapped(T_DATE, ss))] * 3
    refused(nine, r"filter term 8: more than 8 map terms in one term list \(left column 5, key column 8\)")
    t.set_filter(nine[:8])                                                        # eight are accepted
    # accepted pairs: DATE and DECIMAL are signed, BOOLEAN and UINT unsigned, the key may be the left column
    t.set_filter([(T_DATE, ">", fl.Mapped(T_W, ss)), (T_W, "!=", fl.Mapped(T_W, ss)), (T_U, "<=", fl.Mapped(T_BOOL, uu)),
                  (T_BOOL, "=", fl.Mapped(T_I, su)), (T_I, ">=", fl.Mapped(T_U, us))])
    t.set_filter([(T_I, "map<", (T_I, ss.h))])                                    # the raw op code and handle
    t.set_filter(None)
    with pytest.raises(TypeError, match="takes no mapped value"):
        t.set_filter([(T_I, "is_null", fl.Mapped(T_I, ss))])
    # inside an alternative and a condition: the same refusal, with its place
    refused([ok, fl.AnyOf([ok], [ok, (T_I, "<", fl.Mapped(T_U, ss))])],
            r"alternative 1, term 1: filter term 1: the value map's key kind is signed, key column 1")
    with pytest.raises(fl.FlsError, match=r"condition 0, term 0: filter term 0: .*value kind is unsigned") as e:
        t.aggregate([fl.When(("count",), [(T_I, "<", fl.Mapped(T_I, su))])])
    assert e.value.code == ERR_ARG
    # every other op ignores key_col
    arr, n, _ = t._preds([(T_I, "<", 5), (T_I, "<", fl.Col(T_I))])
    arr[0].key_col = arr[1].key_col = 0xFFFFFFFF
    assert fl.lib.fls_scan_filter(t.h, arr, n) == 0
    t.set_filter(None)
    # operator 25 is unknown
    with pytest.raises(fl.FlsError, match="filter operator 25 unknown"):
        t.set_filter([(T_I, 25, 0)])


def test_handles_of_one_kind_do_not_resolve_as_another(fl, conn, typed):
    t = typed
    vm, km, ks = conn.valuemap([1, 2, 3], [0, 1, 2]), conn.keymap([1, 2, 3], [0, 1, 2]), conn.keyset([1, 2, 3])
    h = vm.h
    t.set_filter([(T_I, "<", fl.Mapped(T_I, vm))])
    t.set_filter(None)
    vm.close()
    vm.close()                                                                   # idempotent
    for value in (h, ks.h, km.h, 0, 1, 0xDEADBEEF, id(t), M64):                  # freed, a key set's, a key map's, garbage
        with pytest.raises(fl.FlsError, match=r"filter term 0: filter operator 21 unknown for value 0x[0-9a-f]+: not a live value map \(left column 0, "
                                              r"key column 8\)") as e:
            t.set_filter([(T_I, "<", fl.Mapped(T_DATE, value))])
        assert e.value.code == ERR_ARG
    fl.lib.fls_valuemap_free(h)                                                  # a stale free is a no-op
    fl.lib.fls_valuemap_free(ks.h)                                               # ... and neither a key set
    fl.lib.fls_valuemap_free(km.h)                                               # ... nor a key map is a value map
    assert ks.contains(2) and km.lookup(2) == 1
    val = C.c_uint64()
    for bad in (h, ks.h, km.h):
        assert fl.lib.fls_valuemap_lookup(bad, 1, C.byref(val)) == ERR_ARG
        assert fl.lib.fls_valuemap_info(bad, C.byref(fl.ValueMapInfo())) == ERR_ARG
    # the reverse: a value-map handle is neither a key set nor a key map
    v2 = conn.valuemap([1], [1])
    with pytest.raises(fl.FlsError, match="not a live key set"):
        t.set_filter([(T_I, "in_set", v2.h)])
    with pytest.raises(fl.FlsError, match="not a live key map"):
        t.set_key_bindings([(T_I, v2.h)])
    assert fl.lib.fls_keyset_contains(v2.h, 1) == ERR_ARG
    assert fl.lib.fls_keymap_lookup(v2.h, 1, C.byref(C.c_uint32())) == ERR_ARG
    assert v2.lookup(1) == 1
    # the maps of a closed connection are gone with it
    c2 = fl.Connection([0])
    v3 = c2.valuemap([1], [1])
    c2.close()
    with pytest.raises(fl.FlsError, match="not a live value map"):
        t.set_filter([(T_I, "<", fl.Mapped(T_I, v3.h))])
    v3.h = None


# columns of `prunetab`
P_KEY, P_LEFT, P_NLEFT, P_NKEY = range(4)
NRG_P = 5


@pytest.fixture(scope="module")
def prunetab(fl, conn):
    """row groups of 1024 rows.  key: sorted INT64, row group r holds keys in
    [1000 r, 1000 r + 900]; left: INT32 in [100 r, 100 r + 50] with both ends
    present; nleft / nkey: the same with NULLs and an all-NULL row group 2"""
    rng = np.random.default_rng(2)
    rows = 1024
    key = np.concatenate([np.sort(rng.integers(1000 * r, 1000 * r + 901, rows)) for r in range(NRG_P)]).astype(np.int64)
    left = np.concatenate([rng.integers(100 * r, 100 * r + 51, rows) for r in range(NRG_P)]).astype(np.int32)
    for r in range(NRG_P):
        key[rows * r], key[rows * r + rows - 1] = 1000 * r, 1000 * r + 900
        left[rows * r], left[rows * r + 1] = 100 * r, 100 * r + 50
    null = rng.random(len(key)) < 0.1
    null[2 * rows:3 * rows] = True
    null[[0, 1, rows - 1]] = False
    specs = [("key", fl.INT64, key, fl.ENC_AUTO), ("left", fl.INT32, left, fl.ENC_AUTO),
             ("nleft", fl.INT32, np.ma.masked_array(left, mask=null), fl.ENC_AUTO),
             ("nkey", fl.INT64, np.ma.masked_array(key, mask=null), fl.ENC_AUTO)]
    img = fl.write_image(specs, rowgroup=rows)
    t = conn.read_image(img)
    assert t.nrowgroups == NRG_P
    yield t, img
    t.close()


def verdicts(t, filt):
    return [int(t.may_match(rg, filt)) for rg in range(t.nrowgroups)]


def test_pruning_by_the_key_range_the_value_range_and_nulls(fl, conn, prunetab):
    t, img = prunetab
    # the key range misses the map: only the row groups whose [min, max] holds a key survive (exact on a sorted column)
    m = conn.valuemap([950, 2000, 4900, 4901, -3], [10 ** 6] * 5)
    assert verdicts(t, [(P_LEFT, "<", fl.Mapped(P_KEY, m))]) == [0, 0, 1, 0, 1]
    assert verdicts(t, [(P_LEFT, "!=", fl.Mapped(P_KEY, conn.valuemap([901, 5000], [1, 2])))]) == [0] * 5
    # the value range [vmin, vmax] against the left zone map of row group 1, [100, 150]: each operator excluded,
    # and kept once a bound moves by one
    k1 = [1000, 1500, 1900]                                                       # keys of row group 1 only

    def rg1(op, vmin, vmax):
        vm = conn.valuemap(k1, [vmin, (vmin + vmax) // 2, vmax])
        v = verdicts(t, [(P_LEFT, op, fl.Mapped(P_KEY, vm))])
        assert v[0] == v[2] == v[3] == v[4] == 0                                  # (no key there)
        return v[1]

    assert (rg1("<", 50, 100), rg1("<", 50, 101)) == (0, 1)                       # min(a) < max(b)
    assert (rg1("<=", 50, 99), rg1("<=", 50, 100)) == (0, 1)
    assert (rg1(">", 150, 200), rg1(">", 149, 200)) == (0, 1)                     # max(a) > min(b)
    assert (rg1(">=", 151, 200), rg1(">=", 150, 200)) == (0, 1)
    assert (rg1("=", 151, 200), rg1("=", 150, 200)) == (0, 1)                     # the ranges intersect
    assert (rg1("=", 50, 99), rg1("=", 50, 100)) == (0, 1)
    one = conn.read_image(fl.write_image([("k", fl.INT64, np.full(1024, 7, np.int64), fl.ENC_AUTO),
                                          ("a", fl.INT32, np.full(1024, 42, np.int32), fl.ENC_AUTO)], rowgroup=1024))
    try:                                                                          # `!=`: one single value on both sides
        assert not one.may_match(0, [(1, "!=", fl.Mapped(0, conn.valuemap([7], [42])))])
        assert one.may_match(0, [(1, "!=", fl.Mapped(0, conn.valuemap([7], [43])))])
        assert one.may_match(0, [(1, "!=", fl.Mapped(0, conn.valuemap([7, 8], [42, 41])))])
    finally:
        one.close()
    # unsigned values order as unsigned: 2^63 is above every left value here
    big = conn.valuemap(k1, [1 << 63, (1 << 63) + 5, M64], value_signed=False)
    ut = conn.read_image(fl.write_image([("k", fl.INT64, np.full(1024, 1500, np.int64), fl.ENC_AUTO),
                                         ("a", fl.UINT32, np.arange(1024, dtype=np.uint32), fl.ENC_AUTO)], rowgroup=1024))
    try:
        assert [ut.may_match(0, [(1, op, fl.Mapped(0, big))]) for op in CMP] == [False, True, True, True, False, False]
    finally:
        ut.close()
    # an all-NULL left chunk and an all-NULL key chunk (row group 2 of the nullable columns)
    every = conn.valuemap(list(range(0, 5000, 50)), [10 ** 6] * 100)
    assert verdicts(t, [(P_LEFT, "<", fl.Mapped(P_KEY, every))]) == [1] * 5
    assert verdicts(t, [(P_NLEFT, "<", fl.Mapped(P_KEY, every))]) == [1, 1, 0, 1, 1]
    assert verdicts(t, [(P_LEFT, "<", fl.Mapped(P_NKEY, every))]) == [1, 1, 0, 1, 1]
    assert verdicts(t, [(P_NLEFT, "!=", fl.Mapped(P_NKEY, every))]) == [1, 1, 0, 1, 1]
    # the empty map prunes everything, in either form
    for form in (0, DENSE, HASH):
        e = conn.valuemap([], [], form=form)
        for op in CMP:
            assert verdicts(t, [(P_LEFT, op, fl.Mapped(P_KEY, e))]) == [0] * 5
    # a missing zone map keeps the row group (but not under the empty map)
    buf = bytearray(img.tobytes())
    at = buf.rfind(b"ZMAP")
    assert at > 0
    buf[at] ^= 0xFF                                                               # the optional section is no longer there
    bare = conn.read_image(bytes(buf))
    try:
        assert bare.zonemap(0, P_KEY) is None
        assert verdicts(bare, [(P_LEFT, "<", fl.Mapped(P_KEY, conn.valuemap([-3], [-10 ** 6])))]) == [1] * 5
        assert verdicts(bare, [(P_LEFT, "<", fl.Mapped(P_KEY, conn.valuemap([], [])))]) == [0] * 5
    finally:
        bare.close()


def test_consumers_under_a_map_that_prunes_everything_need_no_gpu(fl, conn, prunetab):
    t, _ = prunetab
    for vm in (conn.valuemap([], []), conn.valuemap([-3, 99999], [1, 2]), conn.valuemap([1000, 1900], [-5, -6])):
        filt = [(P_LEFT, ">=", 0), (P_LEFT, "<", fl.Mapped(P_KEY, vm))]
        assert list(t.scan_filtered(filt)) == [] and t.pruned == NRG_P
        assert t.aggregate([("count",), ("sum", P_LEFT), ("min", P_KEY)], filt) == [0, None, None]
        assert t.pruned == NRG_P
        assert t.aggregate_grouped([P_LEFT], [("count",)], filt) == []
        assert t.aggregate_hashed([P_KEY], [("count",)], 64, filt=filt).to_list() == []


# ------------------------------------------------------------------ GPU tests
C_PICK = 2 * len(KEY_TYPES)       # typetab: key columns 0..10, left columns 11..21, then pick


def left_pool(fl, name, rng):
    """left values: both ends of the type, their neighbours, and a sample around 0"""
    lo, hi = type_range(fl, name)
    if name == "BOOLEAN":
        return [0, 1]
    return sorted({lo, lo + 1, lo + 2, hi - 2, hi - 1, hi, *[v for v in (-3, -1, 0, 1, 2, 50) if lo <= v <= hi],
                   *[int(x) for x in rng.integers(max(lo, -100), min(hi, 100) + 1, 10)]})


@pytest.fixture(scope="module")
def typetab(fl, conn):
    rng = np.random.default_rng(21)
    specs, cols, pools = [], {}, {}
    for part, pool_of in ((0, key_pool), (len(KEY_TYPES), left_pool)):
        for i, name in enumerate(KEY_TYPES):
            c, ty = part + i, getattr(fl, name)
            pool = pool_of(fl, name, rng)
            vals = np.array([pool[j] for j in rng.integers(0, len(pool), N)], dtype=object).astype(fl.NP_DTYPE[ty])
            specs.append((f"c{c}", ty, vals, fl.ENC_FFOR, *((15, 2) if name == "DECIMAL" else ())))
            cols[c], pools[c] = vals, pool
    cols[C_PICK] = pick_column()
    specs.append(("pick", fl.INT8, cols[C_PICK], fl.ENC_AUTO))
    t = conn.read_image(fl.write_image(specs, rowgroup=RG))
    assert t.nrowgroups == 3 and t.nrows == N
    yield t, cols, pools
    t.close()


def key_groups(lo, hi, pool, rng, form):
    """the keys of the maps of one key type: about half of the column's
    values, some absent ones and the type's ends; a dense map spans at most
    2^28 keys, so a wide type gets one map per cluster"""
    signed = lo < 0
    half = [v for v in pool if rng.random() < 0.5] or pool[:1]
    absent = [v for v in (lo + 5, hi - 5, 3, 1234) if lo <= v <= hi and v not in pool]
    edges = [lo, hi] + ([-1 if signed else hi] if hi - lo >= (1 << 63) else [])
    if form == HASH or hi - lo < 1 << 28:
        return [half + absent + edges]
    return [[v for v in half + absent + edges if v - lo < 1 << 20], [v for v in half + absent + edges if hi - v < 1 << 20],
            [v for v in half + absent + [-1 if signed else 0] if abs(v) < 1 << 20]]


def check_all_ops(fl, t, cols, a, k, m, vl=None, vk=None, pick=True, what=()):
    """all six operators of (a op map[k]) through scan_filtered against the dict"""
    present, val = looked_up(cols[k], m.d, m.value_signed)
    left = cols[a].astype(np.int64 if m.value_signed else np.uint64)
    base = present.copy()
    for ok in (vl, vk):
        if ok is not None:
            base &= ok
    if pick:
        base &= cols[C_PICK] == 1
    seen = 0
    for op in CMP:
        want = np.nonzero(base & PYOP[op](left, val))[0]
        filt = [(a, op, fl.Mapped(k, m.vm))] + ([(C_PICK, "=", 1)] if pick else [])
        got = scan_rows(t, filt)
        assert np.array_equal(got, want), (what, op, len(got), len(want))
        seen += len(want)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("name", KEY_TYPES)
def test_gpu_every_key_type_against_the_dict(fl, gpu, conn, typetab, name):
    """the key column of every type, both forms, all six operators; the left
    column is the INT32 one, the values span its range"""
    t, cols, pools = typetab
    k = KEY_TYPES.index(name)
    a = len(KEY_TYPES) + KEY_TYPES.index("INT32")
    lo, hi = type_range(fl, name)
    vpool = pools[a]
    for form in (DENSE, HASH):
        rng = np.random.default_rng(k)
        total = 0
        for keys in key_groups(lo, hi, pools[k], rng, form):
            m = VM(conn, {key: vpool[(3 * i) % len(vpool)] for i, key in enumerate(keys)}, signed=lo < 0, form=form)
            assert m.vm.info.form == form
            total += check_all_ops(fl, t, cols, a, k, m, what=(name, form))
            m.vm.close()
        assert total > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", KEY_TYPES)
def test_gpu_every_left_type_against_the_dict(fl, gpu, conn, typetab, name):
    """the left column of every type, its signedness the value kind's; the
    values include both ends of the type and the left values straddle them;
    the key column is the INT16 one"""
    t, cols, pools = typetab
    a = len(KEY_TYPES) + KEY_TYPES.index(name)
    k = KEY_TYPES.index("INT16")
    lo, hi = type_range(fl, name)
    vsigned = name in SIGNED_TYPES
    vals = [lo, hi, lo + 1, hi - 1] + [v for v in (0, 1, 2, -1, 50) if lo <= v <= hi]
    keys = [v for i, v in enumerate(pools[k]) if i % 3 != 2] + [12345]            # a third of the keys absent
    for form in (DENSE, HASH):
        m = VM(conn, {key: vals[i % len(vals)] for i, key in enumerate(keys)}, value_signed=vsigned, form=form)
        assert check_all_ops(fl, t, cols, a, k, m, what=(name, form)) > 0
        assert check_all_ops(fl, t, cols, a, k, m, pick=False, what=(name, form, "no pick")) > 0
        m.vm.close()
    # the key column may be the left column itself
    if name != "BOOLEAN":
        m = VM(conn, {v: vals[i % len(vals)] for i, v in enumerate(pools[a][::2])}, signed=vsigned, value_signed=vsigned,
               form=HASH)
        assert check_all_ops(fl, t, cols, a, a, m, what=(name, "self")) > 0


@pytest.mark.gpu
def test_gpu_mixed_widths(fl, gpu, conn, typetab):
    """an INT8 / UINT8 left column against values that need 64 bits, and an
    INT64 / UINT64 left column against values of one byte"""
    t, cols, pools = typetab
    L = len(KEY_TYPES)
    k = KEY_TYPES.index("INT16")
    keys = pools[k]
    cases = [("INT8", True, [I64_MIN, I64_MAX, -129, 128, 1 << 40, -(1 << 40), -128, 127, 0]),
             ("UINT8", False, [M64, 1 << 63, 256, 1 << 40, 255, 0, 1]),
             ("INT64", True, [-128, 127, -1, 0, 1]), ("UINT64", False, [0, 1, 255]),
             ("INT64", True, [I64_MIN, I64_MAX, 0]), ("UINT64", False, [M64, M64 - 1, 0])]
    for name, vsigned, vals in cases:
        for form in (DENSE, HASH):
            m = VM(conn, {key: vals[i % len(vals)] for i, key in enumerate(keys)}, value_signed=vsigned, form=form)
            assert check_all_ops(fl, t, cols, L + KEY_TYPES.index(name), k, m, what=(name, form)) > 0


@pytest.fixture(scope="module")
def nulltab(fl, conn):
    """a: left with NULLs everywhere (the placeholder stored at a NULL row is
    0); k: key with NULLs in row group 1 only, so a batch mixes row groups
    with and without validity; b: left without NULL; pick"""
    rng = np.random.default_rng(41)
    a = rng.integers(-3, 4, N).astype(np.int32)
    k = rng.integers(0, 60, N).astype(np.int16)
    b = rng.integers(-3, 4, N).astype(np.int64)
    na = rng.random(N) < 0.3
    nk = np.zeros(N, bool)
    nk[RG:2 * RG] = rng.random(RG) < 0.5
    pick = pick_column()
    img = fl.write_image([("a", fl.INT32, np.ma.masked_array(a, mask=na), fl.ENC_AUTO),
                          ("k", fl.INT16, np.ma.masked_array(k, mask=nk), fl.ENC_AUTO),
                          ("b", fl.INT64, b, fl.ENC_AUTO), ("pick", fl.INT8, pick, fl.ENC_AUTO)], rowgroup=RG)
    t = conn.read_image(img)
    cols = {0: np.where(na, 0, a).astype(np.int32), 1: np.where(nk, 0, k).astype(np.int16), 2: b, 3: pick}
    yield t, cols, {0: ~na, 1: ~nk}, img
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [DENSE, HASH])
def test_gpu_nulls_and_absent_keys_satisfy_no_operator(fl, gpu, conn, nulltab, form):
    t, cols, valid, _ = nulltab
    # key 0 (the NULL rows' placeholder) is present with value 0 (their left placeholder): a NULL honoured by
    # neither side would hit `=`; keys 40.. are absent
    m = VM(conn, {key: (key % 7) - 3 for key in range(0, 40)} | {0: 0, 7: 0}, form=form)
    tcols = cols

    def run(a, k, vl, vk):
        present, val = looked_up(tcols[k], m.d, True)
        base = present & (vl if vl is not None else True) & (vk if vk is not None else True)
        union = np.zeros(N, bool)
        for op in CMP:
            want = base & PYOP[op](tcols[a].astype(np.int64), val)
            got = scan_rows(t, [(a, op, fl.Mapped(k, m.vm)), (3, "=", 1)])
            assert np.array_equal(got, np.nonzero(want & (tcols[3] == 1))[0]), (a, k, op)
            union |= want
        return union, base

    union, base = run(0, 1, valid[0], valid[1])
    assert np.array_equal(union, base) and 0 < base.sum() < N                    # `=` or `!=` holds exactly on the matched rows
    assert (~valid[0]).sum() > 0 and (~valid[1]).sum() > 0 and (tcols[1] >= 40).sum() > 0
    run(2, 1, None, valid[1])                                                     # NULLs in the key column only
    run(0, 2, valid[0], None)                                                     # ... in the left column only (key: b)
    # value 0 at a present key matches `= 0`
    zero_rows = valid[0] & valid[1] & np.isin(tcols[1], [0, 7]) & (tcols[0] == 0)
    got = scan_rows(t, [(0, "=", fl.Mapped(1, m.vm)), (1, "<=", 7), (0, "=", 0)])
    assert zero_rows.sum() > 0 and set(np.nonzero(zero_rows)[0]) <= set(got.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("form", [DENSE, HASH])
def test_gpu_every_encoding_of_the_key_column(fl, gpu, conn, form):
    rng = np.random.default_rng(31)
    ffor = rng.integers(-500, 500, N).astype(np.int32)
    delta = (np.cumsum(rng.integers(0, 4, N)) - 4000).astype(np.int64)
    dic = (rng.integers(0, 9, N) * 1000003 - 3000009).astype(np.int64)
    rle = np.repeat(rng.integers(-20, 20, N // 50 + 1), 50)[:N].astype(np.int16)
    left = rng.integers(-5, 6, N).astype(np.int8)
    img = fl.write_image([("ffor", fl.INT32, ffor, fl.ENC_FFOR), ("delta", fl.INT64, delta, fl.ENC_DELTA),
                          ("dict", fl.INT64, dic, fl.ENC_DICT), ("rle", fl.INT16, rle, fl.ENC_RLE),
                          ("left", fl.INT8, left, fl.ENC_AUTO)], rowgroup=RG)
    assert {tuple(r[:4]) for r in chunk_encodings(img.tobytes())} == {(fl.ENC_FFOR, fl.ENC_DELTA, fl.ENC_DICT, fl.ENC_RLE)}
    t = conn.read_image(img)
    cols = {0: ffor, 1: delta, 2: dic, 3: rle, 4: left}
    try:
        for c in range(4):
            present = np.unique(cols[c])
            some = max(1, min(len(present) // 2, 60))
            keys = [int(v) for v in rng.choice(present, some, replace=False)] + [int(present[-1]) + 1]   # one absent
            m = VM(conn, {key: (i % 11) - 5 for i, key in enumerate(keys)}, form=form)
            assert check_all_ops(fl, t, cols, 4, c, m, pick=False, what=(c, form)) > 0
    finally:
        t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("home", [5, 127])
def test_gpu_colliding_keys_at_max_probe(fl, gpu, conn, home):
    keys = colliding_keys(50, 7, home)
    others = colliding_keys(90, 7, home)[50:]
    rng = np.random.default_rng(51)
    pool = np.array(keys + others + [0, M64], dtype=np.uint64)
    kcol = pool[rng.integers(0, len(pool), N)]
    left = rng.integers(0, 50, N).astype(np.uint16)
    m = VM(conn, {key: j for j, key in enumerate(keys)}, signed=False, value_signed=False, form=HASH)
    assert m.vm.info.max_probe == 50
    t = conn.read_image(fl.write_image([("k", fl.UINT64, kcol, fl.ENC_AUTO), ("a", fl.UINT16, left, fl.ENC_AUTO)],
                                       rowgroup=RG))
    try:
        assert check_all_ops(fl, t, {0: kcol, 1: left}, 1, 0, m, pick=False, what=home) > 0
    finally:
        t.close()


# columns of `facttab`
F_OKEY, F_SUPP, F_GRP, F_D1, F_D2, F_PRICE, F_QTY = range(7)


@pytest.fixture(scope="module")
def facttab(fl, conn):
    """a small fact table: an order key (sorted), a supplier key, a
    low-cardinality group, two dates (the second nullable), a price and a
    quantity with NULLs"""
    rng = np.random.default_rng(28)
    okey = np.sort(rng.integers(0, 1500, N)).astype(np.int64)
    supp = rng.integers(1, 40, N).astype(np.int32)
    grp = rng.integers(0, 5, N).astype(np.int8)
    d1 = rng.integers(9000, 9030, N).astype(np.int32)
    d2 = rng.integers(9000, 9030, N).astype(np.int32)
    n2 = rng.random(N) < 0.2
    price = rng.integers(100, 10 ** 7, N).astype(np.int64)
    qty = rng.integers(1, 51, N).astype(np.int64)
    nq = rng.random(N) < 0.1
    A = fl.ENC_AUTO
    img = fl.write_image([("okey", fl.INT64, okey, A), ("supp", fl.INT32, supp, A), ("grp", fl.INT8, grp, A),
                          ("d1", fl.DATE, d1, A), ("d2", fl.DATE, np.ma.masked_array(d2, mask=n2), A),
                          ("price", fl.DECIMAL, price, A, 15, 2),
                          ("qty", fl.DECIMAL, np.ma.masked_array(qty, mask=nq), A, 15, 2)], rowgroup=RG)
    t = conn.read_image(img)
    cols = {F_OKEY: okey, F_SUPP: supp, F_GRP: grp, F_D1: d1, F_D2: np.where(n2, 0, d2).astype(np.int32),
            F_PRICE: price, F_QTY: np.where(nq, 0, qty).astype(np.int64)}
    yield t, cols, {F_D2: ~n2, F_QTY: ~nq}, img
    t.close()


def order_date_map(conn, cols, form=0, every=3):
    """okey -> an "order date" near the ship dates, for two of every three orders"""
    keys = [int(k) for k in np.unique(cols[F_OKEY]) if k % every]
    return VM(conn, {k: 9005 + (k * 7) % 20 for k in keys}, form=form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", [DENSE, HASH])
def test_gpu_every_consumer_under_a_combined_filter(fl, gpu, conn, facttab, form):
    """one query through aggregate, aggregate_grouped, aggregate_hashed, topn
    and Table.keyset: a map term (d1 > odate[okey]) beside an ordinary term, a
    key-set term and a column-pair term; every result against numpy"""
    t, cols, valid, _ = facttab
    m = order_date_map(conn, cols, form)
    supp_set = [s for s in range(1, 40) if s % 4]
    ks = conn.keyset(supp_set)
    filt = [(F_D1, ">", fl.Mapped(F_OKEY, m.vm)), (F_GRP, "!=", 2), (F_SUPP, "in_set", ks), (F_D1, "<=", fl.Col(F_D2))]
    sel = (map_mask(cols[F_D1], cols[F_OKEY], m, ">") & (cols[F_GRP] != 2) & np.isin(cols[F_SUPP], supp_set) &
           (cols[F_D1] <= cols[F_D2]) & valid[F_D2])
    assert 100 < sel.sum() < N // 2
    assert np.array_equal(scan_rows(t, filt), np.nonzero(sel)[0])
    vq = sel & valid[F_QTY]
    aggs = [("count",), ("count", F_QTY), ("sum", F_PRICE), ("sum", F_QTY), ("min", F_D1), ("max", F_OKEY)]

    def ref(mask):
        q = mask & valid[F_QTY]
        return [int(mask.sum()), int(q.sum()), int(cols[F_PRICE][mask].sum()) if mask.any() else None,
                int(cols[F_QTY][q].sum()) if q.any() else None, int(cols[F_D1][mask].min()) if mask.any() else None,
                int(cols[F_OKEY][mask].max()) if mask.any() else None]

    assert t.aggregate(aggs, filt) == ref(sel) and vq.sum() < sel.sum()
    grouped = t.aggregate_grouped([F_GRP], aggs, filt)
    order = list(dict.fromkeys(cols[F_GRP][sel].tolist()))
    assert [k for k, _ in grouped] == [(g,) for g in order] and len(order) == 4
    assert [v for _, v in grouped] == [ref(sel & (cols[F_GRP] == g)) for g in order]
    hashed = t.aggregate_hashed([F_OKEY], aggs, 4096, filt=filt).to_list()
    okeys = list(dict.fromkeys(cols[F_OKEY][sel].tolist()))
    assert [k for k, _ in hashed] == [(o,) for o in okeys]
    assert [v for _, v in hashed] == [ref(sel & (cols[F_OKEY] == o)) for o in okeys]
    for desc in (False, True):
        rows, values, _ = t.topn(F_PRICE, 100, cols=[F_OKEY, F_PRICE], filt=filt, desc=desc)
        cand = np.nonzero(sel)[0]
        key = cols[F_PRICE][cand]
        best = cand[np.lexsort((cand, -key if desc else key))][:100]
        assert np.array_equal(rows.astype(np.int64), best), desc
        assert np.array_equal(values[F_OKEY], cols[F_OKEY][best]) and np.array_equal(values[F_PRICE], cols[F_PRICE][best])
    built = t.keyset(F_SUPP, filt)                                               # the device build under the narrowed mask
    want = np.unique(cols[F_SUPP][sel])
    assert built.info.count == len(want) and all(built.contains(int(s)) for s in want)
    assert built.build_info is not None and built.build_info.rows_selected == int(sel.sum())
    # ... and the host builds that scan under the filter
    km = t.keymap(F_SUPP, F_GRP, [(F_D1, ">", fl.Mapped(F_OKEY, m.vm)), (F_SUPP, "=", 5), (F_GRP, "=", 1)])
    assert km.info.count == int((map_mask(cols[F_D1], cols[F_OKEY], m, ">") & (cols[F_SUPP] == 5) & (cols[F_GRP] == 1)).any())
    one = map_mask(cols[F_D1], cols[F_OKEY], m, ">") & (cols[F_GRP] == 1) & (cols[F_D1] == 9020)
    vm2 = t.valuemap(F_OKEY, F_D1, [(F_D1, ">", fl.Mapped(F_OKEY, m.vm)), (F_GRP, "=", 1), (F_D1, "=", 9020)])
    assert vm2.info.count == len(np.unique(cols[F_OKEY][one])) > 0
    assert all(vm2.lookup(int(k)) == 9020 for k in np.unique(cols[F_OKEY][one]))


@pytest.mark.gpu
def test_gpu_table_valuemap_leaves_nulls_out_and_refuses_conflicts(fl, gpu, conn, facttab):
    t, cols, valid, _ = facttab
    with pytest.raises(fl.FlsError, match="is listed with the values") as e:     # an order has several prices
        t.valuemap(F_OKEY, F_PRICE)
    assert e.value.code == ERR_ARG
    # supp -> qty over the rows of one (grp, d1) where each supplier has one quantity or several NULL ones
    rows = (cols[F_GRP] == 3) & (cols[F_D1] == 9011)
    first = {}
    for s, q, ok in zip(cols[F_SUPP][rows].tolist(), cols[F_QTY][rows].tolist(), valid[F_QTY][rows].tolist()):
        if ok:
            first.setdefault(s, set()).add(q)
    single = [s for s, qs in first.items() if len(qs) == 1]
    ks = conn.keyset(single)
    vm = t.valuemap(F_SUPP, F_QTY, [(F_GRP, "=", 3), (F_D1, "=", 9011), (F_SUPP, "in_set", ks)])
    assert vm.info.count == len(single) > 0 and vm.info.key_kind == 0 and vm.info.value_kind == 0
    assert all(vm.lookup(s) == next(iter(first[s])) for s in single)
    st = conn.read_image(fl.write_image([("s", fl.VARCHAR, ["a", "b"], fl.ENC_DICT),
                                         ("i", fl.INT32, np.arange(2, dtype=np.int32), fl.ENC_AUTO)], rowgroup=1024))
    try:
        with pytest.raises(ValueError, match="not integer-like"):
            st.valuemap(1, 0)
    finally:
        st.close()


@pytest.mark.gpu
def test_gpu_a_map_term_inside_a_condition(fl, gpu, conn, facttab):
    """sum(price) FILTER (WHERE d1 > odate[okey]) beside the same sum unconditioned"""
    t, cols, valid, _ = facttab
    m = order_date_map(conn, cols)
    base = cols[F_GRP] != 0
    cond = map_mask(cols[F_D1], cols[F_OKEY], m, ">")
    cond2 = map_mask(cols[F_D2], cols[F_OKEY], m, "<=", vl=valid[F_D2]) & (cols[F_SUPP] < 20)
    aggs = [("sum", F_PRICE), fl.When(("sum", F_PRICE), [(F_D1, ">", fl.Mapped(F_OKEY, m.vm))]), ("count",),
            fl.When(("count",), [(F_D1, ">", fl.Mapped(F_OKEY, m.vm))]),
            fl.When(("count", F_QTY), [(F_D2, "<=", fl.Mapped(F_OKEY, m.vm)), (F_SUPP, "<", 20)])]

    def ref(mask):
        return [int(cols[F_PRICE][mask].sum()), int(cols[F_PRICE][mask & cond].sum()), int(mask.sum()),
                int((mask & cond).sum()), int((mask & cond2 & valid[F_QTY]).sum())]

    got = t.aggregate(aggs, [(F_GRP, "!=", 0)])
    assert got == ref(base) and 0 < got[3] < got[2] and got[4] > 0
    grouped = t.aggregate_grouped([F_GRP], aggs, [(F_GRP, "!=", 0)])
    order = list(dict.fromkeys(cols[F_GRP][base].tolist()))
    assert grouped == [((g,), ref(base & (cols[F_GRP] == g))) for g in order]
    hashed = t.aggregate_hashed([F_SUPP], aggs, 256, filt=[(F_GRP, "!=", 0)]).to_list()
    supps = list(dict.fromkeys(cols[F_SUPP][base].tolist()))
    assert hashed == [((s,), ref(base & (cols[F_SUPP] == s))) for s in supps]


@pytest.mark.gpu
@pytest.mark.parametrize("form", [DENSE, HASH])
def test_gpu_two_map_terms_as_alternatives_and_as_a_conjunction(fl, gpu, conn, facttab, form):
    """the Q21 shape: supp != min_supp[okey] OR supp != max_supp[okey] (an
    order with more than one supplier), and the two terms AND-ed"""
    t, cols, valid, _ = facttab
    okey, supp = cols[F_OKEY], cols[F_SUPP]
    keep = [int(k) for k in np.unique(okey) if k % 5]                              # a fifth of the orders absent
    mn = VM(conn, {k: int(supp[okey == k].min()) for k in keep}, form=form)
    mx = VM(conn, {k: int(supp[okey == k].max()) for k in keep}, form=form)
    ne_mn, ne_mx = map_mask(supp, okey, mn, "!="), map_mask(supp, okey, mx, "!=")
    either = [(F_GRP, "<", 4), fl.AnyOf([(F_SUPP, "!=", fl.Mapped(F_OKEY, mn.vm))], [(F_SUPP, "!=", fl.Mapped(F_OKEY, mx.vm))])]
    want = (cols[F_GRP] < 4) & (ne_mn | ne_mx)
    assert 0 < want.sum() < (cols[F_GRP] < 4).sum()
    assert np.array_equal(scan_rows(t, either), np.nonzero(want)[0])
    assert t.aggregate([("count",), ("sum", F_PRICE)], either) == [int(want.sum()), int(cols[F_PRICE][want].sum())]
    # an alternative that mixes a map term with an ordinary and a key-set term
    ks = conn.keyset([3, 5, 8, 13, 21])
    mixed = [fl.AnyOf([(F_SUPP, "=", fl.Mapped(F_OKEY, mn.vm)), (F_D1, ">", 9010)],
                      [(F_SUPP, "in_set", ks), (F_SUPP, "=", fl.Mapped(F_OKEY, mx.vm))], [(F_GRP, "=", 0)])]
    want = ((map_mask(supp, okey, mn, "=") & (cols[F_D1] > 9010)) | (np.isin(supp, [3, 5, 8, 13, 21]) &
                                                                     map_mask(supp, okey, mx, "=")) | (cols[F_GRP] == 0))
    assert np.array_equal(scan_rows(t, mixed), np.nonzero(want)[0]) and 0 < want.sum() < N
    both = [(F_SUPP, "!=", fl.Mapped(F_OKEY, mn.vm)), (F_SUPP, "!=", fl.Mapped(F_OKEY, mx.vm))]
    assert np.array_equal(scan_rows(t, both), np.nonzero(ne_mn & ne_mx)[0]) and 0 < (ne_mn & ne_mx).sum()
    between = [(F_SUPP, ">=", fl.Mapped(F_OKEY, mn.vm)), (F_SUPP, "<=", fl.Mapped(F_OKEY, mx.vm))]
    present = np.isin(okey, keep)
    assert np.array_equal(scan_rows(t, between), np.nonzero(present)[0])          # min <= supp <= max wherever the order is there


@pytest.mark.gpu
def test_gpu_results_identical_across_batches_slots_and_pipelines(fl, gpu, conn, facttab, monkeypatch):
    t, cols, valid, img = facttab
    monkeypatch.delenv("FLS_SCAN_BATCH", raising=False)
    monkeypatch.delenv("FLS_SCAN_SLOTS", raising=False)
    dmap = order_date_map(conn, cols).d
    aggs = [("count",), ("sum", F_PRICE), ("count", F_QTY)]

    def run(c, tab):   # (the maps belong to the table's connection)
        md, mh = VM(c, dmap, form=DENSE), VM(c, dmap, form=HASH)
        a = aggs + [fl.When(("sum", F_QTY), [(F_D2, "<", fl.Mapped(F_OKEY, mh.vm))])]
        f1 = [(F_D1, ">", fl.Mapped(F_OKEY, md.vm)), (F_GRP, "!=", 1)]
        f2 = [fl.AnyOf([(F_D1, "<", fl.Mapped(F_OKEY, mh.vm))], [(F_D2, "=", fl.Mapped(F_OKEY, md.vm))])]
        return (np.sort(scan_rows(tab, f1)).tolist(), np.sort(scan_rows(tab, f2)).tolist(), tab.aggregate(a, f1),
                tab.aggregate_grouped([F_GRP], a, f2))

    base = run(conn, t)
    m = VM(conn, dmap)
    want1 = map_mask(cols[F_D1], cols[F_OKEY], m, ">") & (cols[F_GRP] != 1)
    want2 = map_mask(cols[F_D1], cols[F_OKEY], m, "<") | map_mask(cols[F_D2], cols[F_OKEY], m, "=", vl=valid[F_D2])
    assert base[0] == np.nonzero(want1)[0].tolist() and base[1] == np.nonzero(want2)[0].tolist()
    for batch, slots in (("1", "1"), ("1", "2"), ("2", "3")):                     # one row group per batch against the default
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)
        monkeypatch.setenv("FLS_SCAN_SLOTS", slots)
        assert run(conn, t) == base, (batch, slots)
    monkeypatch.delenv("FLS_SCAN_SLOTS")
    monkeypatch.setenv("FLS_SCAN_BATCH", "1")
    two = fl.Connection([0, 0])                                                   # two scan pipelines on one device
    try:
        tm = two.read_image(img)
        assert run(two, tm) == base
        tm.close()
    finally:
        two.close()


@pytest.mark.gpu
def test_gpu_one_map_serves_two_tables_and_survives_its_handle(fl, gpu, conn):
    rng = np.random.default_rng(71)
    ka, la = rng.integers(0, 500, N).astype(np.int32), rng.integers(0, 9, N).astype(np.int16)
    kb, lb = rng.integers(0, 500, RG + 77).astype(np.int32), rng.integers(0, 9, RG + 77).astype(np.int64)
    ta = conn.read_image(fl.write_image([("k", fl.INT32, ka, fl.ENC_AUTO), ("a", fl.INT16, la, fl.ENC_AUTO)], rowgroup=RG))
    tb = conn.read_image(fl.write_image([("a", fl.INT64, lb, fl.ENC_AUTO), ("k", fl.INT32, kb, fl.ENC_AUTO)], rowgroup=RG))
    try:
        m = VM(conn, {int(k): int(k) % 9 for k in rng.choice(500, 300, replace=False)}, form=HASH)
        for _ in range(2):                                                       # the cached image is reused
            assert check_all_ops(fl, ta, {0: ka, 1: la}, 1, 0, m, pick=False) > 0
            assert check_all_ops(fl, tb, {0: lb, 1: kb}, 0, 1, m, pick=False) > 0
        # the filter is set, then the handle freed before the scan: the term holds a reference
        want = map_mask(la, ka, m, "<")
        ta.set_filter([(1, "<", fl.Mapped(0, m.vm))])
        try:
            m.vm.close()
            with pytest.raises(fl.FlsError, match="not a live value map"):
                tb.set_filter([(0, "<", fl.Mapped(1, m.vm.h or 0))])
            got = ta.aggregate_raw([("count",), ("sum", 1)])
            assert [fl._agg_value(v) for v in got] == [int(want.sum()), int(la[want].sum())]
        finally:
            ta.set_filter(None)
    finally:
        ta.close()
        tb.close()


L_PARTKEY, L_QTY, L_PRICE = 1, 4, 5


@pytest.mark.gpu
def test_gpu_lineitem_q17_shape(fl, gpu, conn):
    """TPC-H Q17's shape on generated lineitem at SF 0.01: the thresholds
    0.2 * avg(l_quantity) per l_partkey come from aggregate_hashed, then
    sum(l_extendedprice), count(*) under l_partkey IN <brand's parts> AND
    l_quantity < threshold[l_partkey]; the check is numpy's"""
    wl, sf = "lineitem", 0.01
    t = conn.read_image(fl.gen_image(wl, sf))
    try:
        n = t.nrows
        part = fl.gen_values(wl, L_PARTKEY, 0, n, fl.NP_DTYPE[t.column(L_PARTKEY).type], sf).astype(np.int64)
        qty = fl.gen_values(wl, L_QTY, 0, n, fl.NP_DTYPE[t.column(L_QTY).type], sf).astype(np.int64)
        price = fl.gen_values(wl, L_PRICE, 0, n, np.int64, sf)
        groups = t.aggregate_hashed([L_PARTKEY], [("sum", L_QTY), ("count", L_QTY)], 1 << 16).to_list()
        # q < 0.2 * s / c  <=>  5 q c < s  <=>  q < ceil(s / (5 c)) over the integers
        thr = {k: -(-s // (5 * c)) for (k,), (s, c) in groups if c}
        sums, cnts = {}, {}
        for p, q in zip(part.tolist(), qty.tolist()):
            sums[p] = sums.get(p, 0) + q
            cnts[p] = cnts.get(p, 0) + 1
        assert thr == {p: -(-sums[p] // (5 * cnts[p])) for p in sums}             # (the build side itself, against Python)
        brand = [p for p in thr if p % 40 == 7]
        ks = conn.keyset(brand)
        for form in (DENSE, HASH):
            vm = conn.valuemap(list(thr), list(thr.values()), form=form)
            got = t.aggregate([("sum", L_PRICE), ("count",)],
                              [(L_PARTKEY, "in_set", ks), (L_QTY, "<", fl.Mapped(L_PARTKEY, vm))])
            sel = np.isin(part, brand) & (5 * qty * np.array([cnts[p] for p in part.tolist()]) <
                                          np.array([sums[p] for p in part.tolist()]))
            assert got == [int(price[sel].sum()), int(sel.sum())] and 0 < sel.sum() < np.isin(part, brand).sum()
            every = t.aggregate([("count",)], [(L_QTY, "<", fl.Mapped(L_PARTKEY, vm))])   # no key set: every row probes
            all_rows = 5 * qty * np.array([cnts[p] for p in part.tolist()]) < np.array([sums[p] for p in part.tolist()])
            assert every == [int(all_rows.sum())]
            vm.close()
    finally:
        t.close()
