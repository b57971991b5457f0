"""Column-to-column filter terms (`a op b` of the same row, DESIGN.md section
26): the exports, the argument checks and the zone-map pruning without a GPU,
and colcmp_kernel on the GPU against numpy, through the scan, the aggregates,
the grouped and hashed aggregates, top-N and a mapped key.

Small shapes throughout (test_keyset.py's): 1024-row row groups, five whole
vectors and a partial tail, the smallest shape with a partial word and a
partial vector.  Values come from small pools, so that equality is frequent,
and every pool holds the type's minimum and maximum, -1, 0 and 2^63 where the
type has them."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import filter_mask, special_doubles

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "duckdb-fastlane_amd" / "libflsgpu.so"
RG = 1024
N = 5 * 1024 + 333
M64 = (1 << 64) - 1
ERR_ARG = -3
ZM_VALID, ZM_HAS_NAN, ZM_ALL_NAN, ZM_HAS_NULL, ZM_ALL_NULL = 1, 2, 4, 8, 16
CMP = ["=", "!=", "<", "<=", ">", ">="]
HOLDS = {"=": lambda c: c == 0, "!=": lambda c: c != 0, "<": lambda c: c < 0, "<=": lambda c: c <= 0,
         ">": lambda c: c > 0, ">=": lambda c: c >= 0}


# ---- helpers of this file
def cmp_scalar(x, y):
    """-1 / 0 / 1 in the filter's order: exact on Python ints; floats with NaN
    equal to NaN and above every number, -0 equal to 0"""
    if isinstance(x, float) or isinstance(y, float):
        xn, yn = math.isnan(x), math.isnan(y)
        if xn or yn:
            return 0 if xn and yn else (1 if xn else -1)
    return (x > y) - (x < y)


def cmp_columns(a, b):
    """cmp_scalar per row.  Integers go through Python ints (numpy compares
    int64 with uint64 as float64); floats are widened to binary64 exactly"""
    if a.dtype.kind == "f":
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        an, bn = np.isnan(a64), np.isnan(b64)
        c = (a64 > b64).astype(np.int8) - (a64 < b64).astype(np.int8)
        return np.where(an & bn, 0, np.where(an, 1, np.where(bn, -1, c))).astype(np.int8)
    return np.fromiter((cmp_scalar(int(x), int(y)) for x, y in zip(a, b)), np.int8, len(a))


def colcmp_mask(fl, cols, terms, n, valid=None, sets=None):
    """helpers.filter_mask extended with (a, op, fl.Col(b)): a column term is a
    clause of its own and holds where both values are valid and a op b.  Also
    takes ("in_set", key of sets) and a prefix ("like", "p%") for the mixed
    filters of this file"""
    valid = valid or {}
    # the explicit spelling (a, "col<", b) is (a, "<", Col(b))
    terms = [(t[0], t[1][3:], fl.Col(t[2]), *t[3:]) if str(t[1]).startswith("col") else t for t in terms]
    special = lambda t: isinstance(t[2], fl.Col) or t[1] in ("in_set", "like")  # noqa: E731
    out = filter_mask(cols, [t for t in terms if not special(t)], n, valid)
    for col, op, val, *_ in terms:
        if isinstance(val, fl.Col):
            hit = HOLDS[op](cmp_columns(cols[col], cols[val.index]))
            for c in (col, val.index):
                if valid.get(c) is not None:
                    hit = hit & valid[c]
        elif op == "in_set":
            members = set(sets[val])
            hit = np.fromiter((int(v) in members for v in cols[col]), bool, n)
        elif op == "like":
            assert val.endswith("%") and "%" not in val[:-1] and "_" not in val
            hit = np.array([s.startswith(val[:-1].encode()) for s in cols[col]], bool)
        else:
            continue
        out &= hit
    return out


def scan_rows(t, terms, deliver=None):
    """(global rows selected, delivered arrays per column concatenated)"""
    rows, parts = [], {}
    for rg, first_row, sel, arrays in t.scan_filtered(terms, cols=deliver):
        rows.append(sel.astype(np.int64) + first_row)
        for c in deliver or []:
            parts.setdefault(c, []).append(arrays[c])
    return (np.concatenate(rows) if rows else np.zeros(0, np.int64)), parts


def check_scan(fl, t, cols, terms, valid=None, deliver=None, eng=None, sets=None):
    """the selection and the delivered values against numpy; eng: the terms as
    the engine takes them when they differ (key sets)"""
    want = np.nonzero(colcmp_mask(fl, cols, terms, t.nrows, valid, sets))[0]
    got, parts = scan_rows(t, eng or terms, deliver)
    assert np.array_equal(got, want), (terms, len(got), len(want))
    for c in deliver or []:
        ty = t.column(c).type
        vals = np.concatenate(parts[c]).view(fl.NP_DTYPE[ty]) if parts.get(c) else np.zeros(0, fl.NP_DTYPE[ty])
        keep = np.ones(len(want), bool) if not valid or c not in valid else valid[c][want]
        assert np.array_equal(vals[keep].view(np.uint8), cols[c][want][keep].view(np.uint8)), (terms, c)
    return want


def draw(pool, dtype, rng, n=N):
    return np.array([pool[i] for i in rng.integers(0, len(pool), n)], dtype=object).astype(dtype)


@pytest.fixture(scope="module")
def conn(fl):
    c = fl.Connection([0])
    yield c
    c.close()


(C_I8, C_I16, C_I32, C_I64, C_U8, C_U64, C_D1, C_D2, C_M1, C_M2, C_M3, C_MW, C_F, C_G, C_S, C_N1, C_N2, C_U64B, C_ID,
 C_B) = range(20)


@pytest.fixture(scope="module")
def typed(fl, conn):
    """one table for the argument checks and the GPU scans: every kind of type
    the checks tell apart, two nullable INT64 columns (n2 with an all-NULL
    third row group) and a row id"""
    rng = np.random.default_rng(26)
    i64 = [-(1 << 63), (1 << 63) - 1, -1, 0, 1, 5, -128, 127]
    u64 = [0, M64, 1 << 63, 1, 5, 255, (1 << 63) - 1]
    dec = [-(10 ** 15) + 1, 10 ** 15 - 1, -1, 0, 100, 101]
    f32 = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 0.1, 1 / 3, 3.4028234663852886e38, 1.0], dtype=np.float32)
    n1 = rng.random(N) < 0.3
    n2 = rng.random(N) < 0.3
    n2[2 * RG:3 * RG] = True
    v1, v2 = draw(i64, np.int64, rng), draw(i64, np.int64, rng)
    cols = {
        C_I8: draw([-128, 127, -1, 0, 1, 5], np.int8, rng), C_I16: draw([-32768, 32767, -1, 0, 5], np.int16, rng),
        C_I32: draw([-(1 << 31), (1 << 31) - 1, -1, 0, 5], np.int32, rng), C_I64: draw(i64, np.int64, rng),
        C_U8: draw([0, 255, 1, 5], np.uint8, rng), C_U64: draw(u64, np.uint64, rng),
        C_D1: draw([-(1 << 31), (1 << 31) - 1, -1, 0, 9000, 9001], np.int32, rng),
        C_D2: draw([-(1 << 31), (1 << 31) - 1, -1, 0, 9000, 9001], np.int32, rng),
        C_M1: draw(dec, np.int64, rng), C_M2: draw(dec, np.int64, rng), C_M3: draw(dec, np.int64, rng),
        C_MW: draw([0, 1, 2], np.int64, rng), C_F: f32[rng.integers(0, len(f32), N)], C_G: special_doubles(N, rng),
        C_S: [b"s%d" % (i % 7) for i in range(N)],
        # what the engine decodes at a NULL row is the writer's placeholder
        C_N1: np.where(n1, 0, v1), C_N2: np.where(n2, 0, v2), C_U64B: draw(u64, np.uint64, rng),
        C_ID: np.arange(N, dtype=np.int32), C_B: rng.integers(0, 2, N).astype(np.uint8),
    }
    A = fl.ENC_AUTO
    specs = [("i8", fl.INT8, cols[C_I8], A), ("i16", fl.INT16, cols[C_I16], A), ("i32", fl.INT32, cols[C_I32], A),
             ("i64", fl.INT64, cols[C_I64], A), ("u8", fl.UINT8, cols[C_U8], A), ("u64", fl.UINT64, cols[C_U64], A),
             ("d1", fl.DATE, cols[C_D1], A), ("d2", fl.DATE, cols[C_D2], A),
             ("m1", fl.DECIMAL, cols[C_M1], A, 15, 2), ("m2", fl.DECIMAL, cols[C_M2], A, 15, 2),
             ("m3", fl.DECIMAL, cols[C_M3], A, 15, 3), ("mw", fl.DECIMAL, cols[C_MW], A, 20, 2),
             ("f", fl.FLOAT, cols[C_F], A), ("g", fl.DOUBLE, cols[C_G], A),
             ("s", fl.VARCHAR, [s.decode() for s in cols[C_S]], fl.ENC_DICT),
             ("n1", fl.INT64, np.ma.masked_array(v1, mask=n1), A), ("n2", fl.INT64, np.ma.masked_array(v2, mask=n2), A),
             ("u64b", fl.UINT64, cols[C_U64B], A), ("id", fl.INT32, cols[C_ID], A), ("b", fl.BOOLEAN, cols[C_B], A)]
    t = conn.read_image(fl.write_image(specs, rowgroup=RG))
    yield t, cols, {C_N1: ~n1, C_N2: ~n2}
    t.close()


# ------------------------------------------------------------------ CPU tests
def test_exports_and_ops(fl):
    assert [fl.OPS[k] for k in ("col=", "col!=", "col<", "col<=", "col>", "col>=")] == [13, 14, 15, 16, 17, 18]
    assert (fl.COL_EQ, fl.COL_NE, fl.COL_LT, fl.COL_LE, fl.COL_GT, fl.COL_GE) == (13, 14, 15, 16, 17, 18)
    assert fl.Col(3).index == 3 and repr(fl.Col(3)) == "Col(3)"
    for k, v in fl.OPS.items():                                                   # every key that names EQ .. GE
        if v <= fl.GE:
            assert fl.OPS["col" + {"==": "=", "<>": "!="}.get(k, k)] == v + 13


def test_col_maps_to_the_column_op_with_the_index_as_value(fl, typed):
    t, _, _ = typed
    for k, v in fl.OPS.items():
        if v > fl.GE:
            continue
        arr, n, _ = t._preds([(C_D1, k, fl.Col(C_D2), 4), (C_I8, "col" + {"==": "=", "<>": "!="}.get(k, k), C_I64)])
        assert (n, arr[0].col, arr[0].op, arr[0].value, arr[0].clause) == (2, C_D1, v + 13, C_D2, 4)
        assert (arr[1].col, arr[1].op, arr[1].value) == (C_I8, v + 13, C_I64)
        assert not arr[0].str and arr[0].str_len == 0
    with pytest.raises(TypeError, match="takes no column"):
        t._preds([(C_I8, "is_null", fl.Col(C_I64))])
    with pytest.raises(TypeError, match="takes no column"):
        t._preds([(C_S, "like", fl.Col(C_S))])


REFUSALS = [
    (C_I8, 20, r"right column 20 out of range \(left column 0"),
    (C_I8, 1 << 40, r"right column 1099511627776 out of range"),
    (C_S, C_S, r"VARCHAR / BLOB column \(columns 14 and 14\)"),
    (C_I8, C_S, r"VARCHAR / BLOB column \(columns 0 and 14\)"),
    (C_S, C_I8, r"VARCHAR / BLOB column \(columns 14 and 0\)"),
    (C_I8, C_U8, r"signed column against an unsigned column \(columns 0 and 4\)"),
    (C_U64, C_I64, r"signed column against an unsigned column \(columns 5 and 3\)"),
    (C_B, C_I8, r"signed column against an unsigned column \(columns 19 and 0\)"),
    (C_I64, C_G, r"integer-like column against a FLOAT / DOUBLE column \(columns 3 and 13\)"),
    (C_F, C_U8, r"integer-like column against a FLOAT / DOUBLE column \(columns 12 and 4\)"),
    (C_D1, C_I32, r"DATE column against a non-DATE column \(columns 6 and 2\)"),
    (C_I32, C_D1, r"DATE column against a non-DATE column \(columns 2 and 6\)"),
    (C_M1, C_M3, r"DECIMALs of different scale, 2 and 3 \(columns 8 and 10\)"),
    (C_M1, C_MW, r"DECIMAL wider than 64 bits \(columns 8 and 11\)"),
    (C_MW, C_MW, r"DECIMAL wider than 64 bits \(columns 11 and 11\)"),
    (C_M1, C_I64, r"DECIMAL column against a non-DECIMAL column \(columns 8 and 3\)"),
]


@pytest.mark.parametrize("a,b,frag", REFUSALS)
def test_refusals_name_the_term_and_both_columns_before_any_device_work(fl, typed, a, b, frag):
    t, _, _ = typed
    for op in ("col=", "col!=", "col<", "col<=", "col>", "col>="):
        with pytest.raises(fl.FlsError, match=r"filter term 1: .*" + frag) as e:
            t.set_filter([(C_I8, "<", 5), (a, op, b)])
        assert e.value.code == ERR_ARG
    with pytest.raises(fl.FlsError, match=r"filter term 0: .*" + frag) as e:
        t.may_match(0, [(a, "<", fl.Col(b))])
    assert e.value.code == ERR_ARG


def test_operator_19_is_still_unknown_and_accepted_pairs_bind(fl, typed):
    t, _, _ = typed
    for op in (19, 20, 255):
        with pytest.raises(fl.FlsError, match=f"filter operator {op} unknown") as e:
            t.set_filter([(C_I8, op, C_I64)])
        assert e.value.code == ERR_ARG
    # every accepted pair, both ways round, and a column against itself
    for a, b in [(C_I8, C_I64), (C_I16, C_I32), (C_U8, C_U64), (C_U8, C_B), (C_D1, C_D2), (C_M1, C_M2), (C_F, C_G),
                 (C_F, C_F), (C_G, C_G), (C_N1, C_N2), (C_I64, C_I64)]:
        t.set_filter([(a, "<", fl.Col(b)), (b, ">=", fl.Col(a))])
    t.set_filter([])


def test_a_shared_clause_is_refused_from_either_position(fl, typed):
    t, _, _ = typed
    for filt, i in [([(C_I8, "<", fl.Col(C_I64), 7), (C_I8, "=", 3, 7)], 0),
                    ([(C_I8, "=", 3, 7), (C_I8, "<", fl.Col(C_I64), 7)], 1),
                    ([(C_I8, "<", fl.Col(C_I64), 7), (C_D1, ">", fl.Col(C_D2), 7)], 0),
                    ([(C_I8, "is_null", None, 2), (C_S, "=", "s1", 7), (C_D1, "col>", C_D2, 7)], 2)]:
        with pytest.raises(fl.FlsError, match=rf"filter term {i}: a column term shares clause 7 with term \d") as e:
            t.set_filter(filt)
        assert e.value.code == ERR_ARG
        with pytest.raises(fl.FlsError, match=rf"filter term {i}: a column term shares clause 7"):
            t.may_match(0, filt)


NRG_P = 7
C_PA, C_PB, C_PN, C_PF, C_PG, C_PU, C_PV = range(7)


@pytest.fixture(scope="module")
def prunetab(fl, conn):
    """sorted INT64 columns a and b whose row-group ranges are, in turn,
    disjoint (a below b, a above b), touching (either way), nested (either
    way) and one single value; n: b with NULLs and an all-NULL third row
    group; a DOUBLE f / FLOAT g pair with all-NaN and some-NaN zones; the
    UINT64 pair u / v across 2^63"""
    rng = np.random.default_rng(27)
    rows = [RG] * (NRG_P - 1) + [333]
    ra = [(0, 100), (200, 300), (0, 100), (100, 200), (0, 300), (100, 200), (7, 7)]
    rb = [(200, 300), (0, 100), (100, 200), (0, 100), (100, 200), (0, 300), (7, 7)]

    def fill(ranges):
        parts = []
        for (lo, hi), n in zip(ranges, rows):
            v = np.sort(rng.integers(lo, hi + 1, n))
            v[0], v[-1] = lo, hi
            parts.append(v)
        return np.concatenate(parts)
    a, b = fill(ra).astype(np.int64), fill(rb).astype(np.int64)
    n = len(a)
    null = rng.random(n) < 0.2
    null[2 * RG:3 * RG] = True
    nan = np.nan
    f = fill(ra).astype(np.float64) / 8
    g = (fill(rb).astype(np.float64) / 8).astype(np.float32)
    f[0:RG] = nan                                                  # rg 0: f all NaN
    f[RG:2 * RG:3] = nan                                           # rg 1: f some NaN
    g[2 * RG:3 * RG] = nan                                         # rg 2: g all NaN
    g[3 * RG + 5] = nan                                            # rg 3: g one NaN
    f[4 * RG:5 * RG:2] = nan                                       # rg 4: both some NaN
    g[4 * RG:5 * RG:5] = nan
    f[5 * RG:6 * RG] = nan                                         # rg 5: both all NaN
    g[5 * RG:6 * RG] = nan
    u = (fill(ra).astype(object) + ((1 << 63) - 150)).astype(np.uint64)
    v = (fill(rb).astype(object) + ((1 << 63) - 150)).astype(np.uint64)
    A = fl.ENC_AUTO
    t = conn.read_image(fl.write_image(
        [("a", fl.INT64, a, A), ("b", fl.INT64, b, A), ("n", fl.INT64, np.ma.masked_array(b, mask=null), A),
         ("f", fl.DOUBLE, f, A), ("g", fl.FLOAT, g, A), ("u", fl.UINT64, u, A), ("v", fl.UINT64, v, A)], rowgroup=RG))
    assert t.nrowgroups == NRG_P
    yield t, {C_PA: a, C_PB: b, C_PN: np.where(null, 0, b), C_PF: f, C_PG: g, C_PU: u, C_PV: v}, {C_PN: ~null}
    t.close()


def table_says(op, za, zb, is_float):
    """the pruning rule of DESIGN.md section 26 from two Table.zonemap results"""
    if (za and za[2] & ZM_ALL_NULL) or (zb and zb[2] & ZM_ALL_NULL):
        return False
    if za is None or zb is None or not (za[2] & ZM_VALID) or not (zb[2] & ZM_VALID):
        return True
    (alo, ahi, fa), (blo, bhi, fb) = za, zb
    if is_float:   # the substitution the constant terms make: an all-NaN zone starts at NaN, one with a NaN ends there
        alo, ahi = (math.nan if fa & ZM_ALL_NAN else alo), (math.nan if fa & ZM_HAS_NAN else ahi)
        blo, bhi = (math.nan if fb & ZM_ALL_NAN else blo), (math.nan if fb & ZM_HAS_NAN else bhi)
    c = cmp_scalar
    return {"<": c(alo, bhi) < 0, "<=": c(alo, bhi) <= 0, ">": c(ahi, blo) > 0, ">=": c(ahi, blo) >= 0,
            "=": c(alo, bhi) <= 0 and c(blo, ahi) <= 0,
            "!=": not (c(alo, ahi) == 0 and c(blo, bhi) == 0 and c(alo, blo) == 0)}[op]


@pytest.mark.parametrize("a,b", [(C_PA, C_PB), (C_PB, C_PA), (C_PA, C_PN), (C_PN, C_PA), (C_PF, C_PG), (C_PG, C_PF),
                                 (C_PU, C_PV), (C_PF, C_PF), (C_PA, C_PA)])
def test_pruning_follows_the_table_and_never_loses_a_row(fl, prunetab, a, b):
    t, cols, valid = prunetab
    is_float = cols[a].dtype.kind == "f"
    verdicts = set()
    for op in CMP:
        truth = colcmp_mask(fl, cols, [(a, op, fl.Col(b))], t.nrows, valid)
        for rg in range(NRG_P):
            want = table_says(op, t.zonemap(rg, a), t.zonemap(rg, b), is_float)
            got = t.may_match(rg, [(a, op, fl.Col(b))])
            assert got == want, (a, b, op, rg, t.zonemap(rg, a), t.zonemap(rg, b))
            assert got or not truth[rg * RG:(rg + 1) * RG].any(), (a, b, op, rg)   # conservative
            if C_PN in (a, b):
                assert got or rg == 2 or want is False
                if rg == 2:
                    assert not got                                                 # all NULL on either side
            verdicts.add(got)
    assert verdicts == {True, False} or a == b == C_PF


def test_pruning_verdicts_on_the_constructed_ranges(fl, prunetab):
    """the table spelled out for the integer pair: row groups 0..6 are a below
    b, a above b, touching at max(a) = min(b), touching at min(a) = max(b), b
    nested in a, a nested in b, one single value"""
    t, _, _ = prunetab
    expect = {"<": [1, 0, 1, 0, 1, 1, 0], "<=": [1, 0, 1, 1, 1, 1, 1], ">": [0, 1, 0, 1, 1, 1, 0],
              ">=": [0, 1, 1, 1, 1, 1, 1], "=": [0, 0, 1, 1, 1, 1, 1], "!=": [1, 1, 1, 1, 1, 1, 0]}
    for op, want in expect.items():
        assert [int(t.may_match(rg, [(C_PA, op, fl.Col(C_PB))])) for rg in range(NRG_P)] == want, op
        assert [int(t.may_match(rg, [(C_PU, op, fl.Col(C_PV))])) for rg in range(NRG_P)] == want, op
    # floats: rg 0 f all NaN against numbers, rg 2 g all NaN, rg 5 both all NaN
    ff = lambda op, rg: t.may_match(rg, [(C_PF, op, fl.Col(C_PG))])  # noqa: E731
    assert [ff(op, 0) for op in CMP] == [False, True, False, False, True, True]      # NaN is above every number
    assert [ff(op, 2) for op in CMP] == [False, True, True, True, False, False]
    assert [ff(op, 5) for op in CMP] == [True, False, False, True, False, True]      # NaN equals NaN
    assert all(ff(op, 4) for op in CMP)                                               # NaN somewhere on both sides


def apart_table(fl, conn):
    """lo in [0, 100] and hi in [200, 300] in every row group: hi < lo holds nowhere"""
    rng = np.random.default_rng(29)
    n = 2 * RG + 77
    return conn.read_image(fl.write_image([("lo", fl.INT16, rng.integers(0, 101, n).astype(np.int16), fl.ENC_AUTO),
                                           ("hi", fl.INT64, rng.integers(200, 301, n).astype(np.int64), fl.ENC_AUTO)],
                                          rowgroup=RG))


def test_a_column_term_pruned_everywhere_needs_no_gpu(fl, conn):
    t = apart_table(fl, conn)
    try:
        for filt in ([(1, "<", fl.Col(0))], [(0, ">=", fl.Col(1)), (0, ">", 5)], [(0, "=", fl.Col(1))]):
            assert not any(t.may_match(rg, filt) for rg in range(t.nrowgroups))
            assert list(t.scan_filtered(filt)) == [] and t.pruned == t.nrowgroups == 3
            assert t.aggregate([("count",), ("sum", 0)], filt) == [0, None]
            assert t.aggregate_grouped([0], [("count",)], filt) == []
    finally:
        t.close()


def test_colcmp_kernel_resources():
    """colcmp_kernel: no scratch, no spill, at most 64 VGPRs (eight waves per
    SIMD) and the four wave counts in LDS"""
    if not LIB.exists():
        pytest.skip("libflsgpu.so not built")
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    res = kernel_resources.resources(str(LIB))
    hits = {k: v for k, v in res.items() if "colcmp_kernel" in k}
    assert len(hits) == 1, sorted(res)
    for name, r in hits.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 64 and r["lds"] <= 16, (name, r)


# ------------------------------------------------------------------ GPU tests
PAIRS = [("int8_int64", C_I8, C_I64), ("int64_int8", C_I64, C_I8), ("int16_int32", C_I16, C_I32),
         ("uint8_uint64", C_U8, C_U64), ("uint64_uint64", C_U64, C_U64B), ("boolean_uint8", C_B, C_U8),
         ("date_date", C_D1, C_D2), ("decimal_decimal", C_M1, C_M2), ("float_double", C_F, C_G),
         ("double_float", C_G, C_F), ("self_int", C_I64, C_I64), ("self_double", C_G, C_G),
         ("null_left", C_N1, C_I64), ("null_right", C_I64, C_N2), ("null_both", C_N1, C_N2), ("self_null", C_N2, C_N2)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,a,b", PAIRS)
def test_gpu_scan_against_numpy(fl, gpu, conn, typed, name, a, b):
    t, cols, valid = typed
    counts = {}
    for op in CMP:
        want = check_scan(fl, t, cols, [(a, op, fl.Col(b))], valid, deliver=sorted({a, b, C_ID}))
        counts[op] = len(want)
    nvalid = int((valid.get(a, np.ones(N, bool)) & valid.get(b, np.ones(N, bool))).sum())
    # the six selections partition the rows valid on both sides; a NULL row is in none
    assert counts["="] + counts["!="] == counts["<"] + counts[">="] == counts["<="] + counts[">"] == nvalid
    if a == b:
        assert counts["="] == counts["<="] == nvalid and counts["<"] == counts["!="] == 0
    else:
        assert all(0 < counts[op] < N for op in CMP), counts


@pytest.mark.gpu
def test_gpu_2_to_the_63_against_1_is_unsigned(fl, gpu, conn):
    a = np.array([1 << 63, 1, M64, 0, 1 << 63] * 300, dtype=np.uint64)
    b = np.array([1, 1 << 63, 0, M64, 1 << 63] * 300, dtype=np.uint64)
    t = conn.read_image(fl.write_image([("a", fl.UINT64, a, fl.ENC_AUTO), ("b", fl.UINT64, b, fl.ENC_AUTO)], rowgroup=RG))
    try:
        for op, per5 in zip(CMP, ([4], [0, 1, 2, 3], [1, 3], [1, 3, 4], [0, 2], [0, 2, 4])):
            rows = scan_rows(t, [(0, op, fl.Col(1))])[0]
            assert np.array_equal(rows, np.array([i for i in range(1500) if i % 5 in per5])), op
    finally:
        t.close()


@pytest.mark.gpu
def test_gpu_all_four_mask_kernels_on_one_mask(fl, gpu, conn, typed):
    """a constant term, a column term, a key-set term and a LIKE term: filter,
    colcmp, keyset and strmatch kernels run in sequence on one mask"""
    t, cols, valid = typed
    keys = [-1, 5, (1 << 31) - 1]
    ks = conn.keyset(keys)
    try:
        for like in ("s1%", "s%", "x%"):
            terms = [(C_I64, ">", -5), (C_I8, "<=", fl.Col(C_I64)), (C_I32, "in_set", "k"), (C_S, "like", like)]
            eng = [terms[0], terms[1], (C_I32, "in_set", ks), terms[3]]
            want = check_scan(fl, t, cols, terms, valid, deliver=[C_I8, C_I64, C_ID], eng=eng, sets={"k": keys})
            assert (len(want) > 0) == (like != "x%")
        # the skip path: constant terms that empty whole words and whole vectors before the column term
        for lo, hi in ((64, 128), (2 * RG + 64, 2 * RG + 130), (N - 5, N), (0, 0)):
            check_scan(fl, t, cols, [(C_ID, ">=", lo), (C_ID, "<", hi), (C_D1, "!=", fl.Col(C_D2))], valid, deliver=[C_ID])
    finally:
        ks.close()


@pytest.mark.gpu
def test_gpu_two_column_terms_in_one_filter(fl, gpu, conn, typed):
    t, cols, valid = typed
    for terms in ([(C_D1, "<", fl.Col(C_D2)), (C_I8, ">=", fl.Col(C_I64))],
                  [(C_N1, "<=", fl.Col(C_N2)), (C_F, "!=", fl.Col(C_G)), (C_U8, "<", fl.Col(C_U64))],
                  [(C_D1, "col<", C_D2), (C_D2, "col<", C_D1)],                    # contradictory: no row
                  [(C_M1, "<", fl.Col(C_M2)), (C_M1, "is_not_null", None, 3), (C_I8, "=", 0, 3), (C_G, ">", fl.Col(C_F))]):
        want = check_scan(fl, t, cols, terms, valid, deliver=[C_ID])
        assert (len(want) == 0) == (terms[0][1] == "col<")


@pytest.fixture(scope="module")
def facttab(fl, conn):
    """a small fact table: key, low-cardinality group, two dates (the second
    nullable), a price, and flag = 1 where numpy finds d1 < d2"""
    rng = np.random.default_rng(28)
    key = np.sort(rng.integers(0, 4000, N)).astype(np.int64)
    grp = rng.integers(0, 5, N).astype(np.int8)
    d1 = rng.integers(9000, 9030, N).astype(np.int32)
    d2 = rng.integers(9000, 9030, N).astype(np.int32)
    nm = rng.random(N) < 0.2
    price = rng.integers(100, 10 ** 7, N).astype(np.int64)
    flag = ((d1 < d2) & ~nm).astype(np.int8)
    disc = rng.integers(0, 11, N).astype(np.int64)
    A = fl.ENC_AUTO
    specs = [("key", fl.INT64, key, A), ("grp", fl.INT8, grp, A), ("d1", fl.DATE, d1, A),
             ("d2", fl.DATE, np.ma.masked_array(d2, mask=nm), A), ("price", fl.DECIMAL, price, A, 15, 2),
             ("flag", fl.INT8, flag, A), ("disc", fl.DECIMAL, disc, A, 15, 2)]
    img = fl.write_image(specs, rowgroup=RG)
    t = conn.read_image(img)
    yield t, {0: key, 1: grp, 2: d1, 3: np.where(nm, 0, d2).astype(np.int32), 4: price, 5: flag, 6: disc}, {3: ~nm}, img
    t.close()


AGGS = [("count",), ("count", 3), ("sum", 4), ("min", 2), ("max", 3), ("sum_expr", [(0, 1, 4), (100, -1, 6)])]


@pytest.mark.gpu
def test_gpu_downstream_calls_under_a_column_term(fl, gpu, conn, facttab):
    """a < b against the same call over the rows numpy selects (flag = 1)"""
    t, cols, valid, _ = facttab
    for extra in ([], [(1, "!=", 2)]):
        col = [(2, "<", fl.Col(3))] + extra
        ref = [(5, "=", 1)] + extra
        m = colcmp_mask(fl, cols, col, N, valid)
        assert np.array_equal(m, filter_mask(cols, ref, N, valid)) and 0 < m.sum() < N
        got = t.aggregate(AGGS, col)
        assert got == t.aggregate(AGGS, ref)
        assert got[:3] == [int(m.sum()), int(m.sum()), int(cols[4][m].sum())]
        assert t.aggregate_grouped([1], AGGS, col) == t.aggregate_grouped([1], AGGS, ref)
        assert len(t.aggregate_grouped([1], AGGS, col)) == 5 - len(extra)
        hashed = t.aggregate_hashed([0], AGGS, 8192, filt=col).to_list()
        assert hashed == t.aggregate_hashed([0], AGGS, 8192, filt=ref).to_list()
        assert len(hashed) == len(np.unique(cols[0][m]))
        for sel in (dict(having=[(0, ">=", 2)]), dict(having=[(2, ">", 10 ** 7)], order_by=(2, "desc"), limit=10)):
            h = t.aggregate_hashed([0], AGGS, 8192, filt=col, **sel).to_list()
            assert h == t.aggregate_hashed([0], AGGS, 8192, filt=ref, **sel).to_list() and 0 < len(h) < len(hashed)
        for desc in (False, True):
            rows, values, _ = t.topn(4, 100, cols=[0, 4], filt=col, desc=desc)
            cand = np.nonzero(m)[0]
            k = cols[4][cand]
            order = cand[np.lexsort((cand, -k if desc else k))][:100]
            assert np.array_equal(rows.astype(np.int64), order), desc
            assert np.array_equal(values[0], cols[0][order]) and np.array_equal(values[4], cols[4][order])
        km = conn.keymap(np.arange(0, 4000, 2), np.arange(0, 4000, 2) % 3)
        try:
            for key in (("map", 0, km), ("map", 0, km, "keep_unmatched")):
                g = t.aggregate_grouped([key, 1], AGGS, col)
                assert g == t.aggregate_grouped([key, 1], AGGS, ref) and len(g) > 3
        finally:
            km.close()


@pytest.mark.gpu
def test_gpu_results_identical_across_batches_slots_and_gpus(fl, gpu, conn, facttab, monkeypatch):
    t, cols, valid, img = facttab
    filts = [[(2, "<", fl.Col(3))], [(3, ">=", fl.Col(2)), (1, "!=", 0), (0, "<", 3000, 9), (1, "=", 1, 9)]]
    want = [np.nonzero(colcmp_mask(fl, cols, f, N, valid))[0] for f in filts]
    aggs = [t.aggregate(AGGS, f) for f in filts]
    for batch, slots in (("1", "1"), ("3", "2"), ("8", "2"), ("2", "3")):
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)
        monkeypatch.setenv("FLS_SCAN_SLOTS", slots)
        for f, w, a in zip(filts, want, aggs):
            assert np.array_equal(scan_rows(t, f)[0], w), (batch, slots)
            assert t.aggregate(AGGS, f) == a, (batch, slots)
    monkeypatch.delenv("FLS_SCAN_BATCH")
    monkeypatch.delenv("FLS_SCAN_SLOTS")
    two = fl.Connection([0, 0])                                  # two scan pipelines on one device
    try:
        tm = two.read_image(img)
        for f, w, a in zip(filts, want, aggs):
            assert np.array_equal(np.sort(scan_rows(tm, f)[0]), w)
            assert tm.aggregate(AGGS, f) == a
        tm.close()
    finally:
        two.close()


@pytest.mark.gpu
def test_gpu_a_column_term_pruned_everywhere_yields_no_row_group(fl, gpu, conn, prunetab):
    t, cols, valid = prunetab
    ta = apart_table(fl, conn)
    try:
        assert list(ta.scan_filtered([(1, "<=", fl.Col(0))])) == [] and ta.pruned == ta.nrowgroups
        got = scan_rows(ta, [(0, "<", fl.Col(1))])[0]                    # ... and the opposite term keeps every row
        assert np.array_equal(got, np.arange(ta.nrows)) and ta.pruned == 0
    finally:
        ta.close()
    # and one that prunes some row groups delivers exactly the rest
    for op in CMP:
        filt = [(C_PA, op, fl.Col(C_PB))]
        kept = [rg for rg in range(NRG_P) if t.may_match(rg, filt)]
        assert [rg for rg, *_ in t.scan_filtered(filt)] == kept and t.pruned == NRG_P - len(kept)
        check_scan(fl, t, cols, filt, valid, deliver=[C_PA])
        check_scan(fl, t, cols, [(C_PF, op, fl.Col(C_PG))], valid)
        check_scan(fl, t, cols, [(C_PN, op, fl.Col(C_PA))], valid)
