"""Filtered aggregates, agg(...) FILTER (WHERE cond): the
export, the ctypes layout, the argument checks and the Python packing without a
GPU; cond_kernel and the reduce kernels' condition planes on the GPU against
numpy, ungrouped, grouped and hashed.

Shapes are test_colcmp.py's: 1024-row row groups, five whole vectors and a
partial tail of 333 rows (a partial word and a partial vector), small value
pools, a nullable column with an all-NULL row group.  The reference is numpy
through helpers.filter_mask plus the set / LIKE / column-pair extensions of
test_colcmp.py; each wanted value is the aggregate over where & cond & valid.
Every GPU test asserts that its condition selects some but not all of the
filter's rows, in the whole table and inside the partial tail vector."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

from helpers import filter_mask

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "duckdb-fastlane_amd" / "libflsgpu.so"
RG = 1024
N = 5 * 1024 + 333
TAIL = 5 * 1024
ERR_ARG = -3
HOLDS = {"=": lambda c: c == 0, "!=": lambda c: c != 0, "<": lambda c: c < 0, "<=": lambda c: c <= 0,
         ">": lambda c: c > 0, ">=": lambda c: c >= 0}

C_K, C_I, C_D, C_G, C_N, C_S, C_F, C_ID, C_J, C_OK, C_Q = range(11)
S_POOL = [b"PROMO BRUSHED COPPER", b"PROMO TIN", b"ECONOMY ANODIZED STEEL", b"STANDARD", b"", b"MEDIUM POLISHED BRASS"]
F_POOL = [b"deliver in person please", b"collect cod", b"take back return to sender", b"none", b"ship by air express"]


@pytest.fixture(scope="module")
def conn(fl):
    c = fl.Connection([0])
    yield c
    c.close()


@pytest.fixture(scope="module")
def tab(fl, conn):
    """k: four group keys; i, j: INT64 pools; d: DECIMAL(15,2); g: DOUBLE; n:
    nullable INT64 with an all-NULL third row group; s: VARCHAR, DICT; f:
    VARCHAR, FSST; id: the row; ok: a sorted key of four rows per value; q: a
    small quantity for products"""
    rng = np.random.default_rng(27)
    null = rng.random(N) < 0.3
    null[2 * RG:3 * RG] = True
    nv = rng.integers(-50, 50, N).astype(np.int64)
    cols = {
        C_K: rng.integers(0, 4, N).astype(np.int32),
        C_I: rng.choice(np.array([-(1 << 40), -7, -1, 0, 1, 5, 1 << 40, 12345], np.int64), N),
        C_D: rng.integers(-10 ** 6, 10 ** 6, N).astype(np.int64),
        C_G: np.round(rng.normal(0, 1000, N), 3),
        C_N: np.where(null, 0, nv),   # what the engine decodes at a NULL row is the writer's placeholder
        C_S: [S_POOL[x] for x in rng.integers(0, len(S_POOL), N)],
        C_F: [F_POOL[x] for x in rng.integers(0, len(F_POOL), N)],
        C_ID: np.arange(N, dtype=np.int32),
        C_J: rng.choice(np.array([-7, -1, 0, 1, 5, 9], np.int64), N),
        C_OK: (np.arange(N, dtype=np.int64) // 4) + 1000,
        C_Q: rng.integers(1, 51, N).astype(np.int32),
    }
    A = fl.ENC_AUTO
    specs = [("k", fl.INT32, cols[C_K], A), ("i", fl.INT64, cols[C_I], A), ("d", fl.DECIMAL, cols[C_D], A, 15, 2),
             ("g", fl.DOUBLE, cols[C_G], A), ("n", fl.INT64, np.ma.masked_array(nv, mask=null), A),
             ("s", fl.VARCHAR, [x.decode() for x in cols[C_S]], fl.ENC_DICT),
             ("f", fl.VARCHAR, [x.decode() for x in cols[C_F]], fl.ENC_FSST),
             ("id", fl.INT32, cols[C_ID], A), ("j", fl.INT64, cols[C_J], A), ("ok", fl.INT64, cols[C_OK], A),
             ("q", fl.INT32, cols[C_Q], A)]
    t = conn.read_image(fl.write_image(specs, rowgroup=RG))
    assert t.nrowgroups == 6
    yield t, cols, {C_N: ~null}
    t.close()


# ---- the reference
def cmp_columns(a, b):
    return np.fromiter(((int(x) > int(y)) - (int(x) < int(y)) for x, y in zip(a, b)), np.int8, len(a))


def ref_mask(fl, cols, terms, valid, sets=None):
    """helpers.filter_mask extended as test_colcmp.py's colcmp_mask: (a, op,
    fl.Col(b)), (col, "in_set" / "not_in_set", key of sets) and a prefix
    (col, "like" / "not_like", "p%"), each a clause of its own that holds only
    where the values are valid"""
    special = lambda t: isinstance(t[2], fl.Col) or t[1] in ("in_set", "not_in_set", "like", "not_like")  # noqa: E731
    out = filter_mask(cols, [t for t in terms if not special(t)], N, valid)
    for col, op, val, *_ in terms:
        if isinstance(val, fl.Col):
            hit = HOLDS[op](cmp_columns(cols[col], cols[val.index]))
            if valid.get(val.index) is not None:
                hit = hit & valid[val.index]
        elif op in ("in_set", "not_in_set"):
            members = set(sets[val])
            hit = np.fromiter((int(v) in members for v in cols[col]), bool, N) == (op == "in_set")
        elif op in ("like", "not_like"):
            assert val.endswith("%") and "%" not in val[:-1] and "_" not in val
            hit = np.array([s.startswith(val[:-1].encode()) for s in cols[col]], bool) == (op == "like")
        else:
            continue
        if valid.get(col) is not None:
            hit = hit & valid[col]
        out &= hit
    return out


def operand_valid(agg, valid):
    m = np.ones(N, bool)
    cs = [f[2] for f in agg[1]] if agg[0] == "sum_expr" else list(agg[1:])
    for c in cs:
        if valid.get(c) is not None:
            m &= valid[c]
    return m


def ref_value(agg, cols, m):
    """the aggregate over the rows of m (selected, condition true, operands
    valid) in Python integers; a DOUBLE sum as the list of its addends"""
    fn = agg[0]
    if fn == "count":
        return int(m.sum())
    if not m.any():
        return None
    if fn == "sum_expr":
        total = 0
        for r in np.nonzero(m)[0]:
            p = 1
            for k, sign, c in agg[1]:
                p *= k + sign * int(cols[c][r])
            total += p
        return total
    v = cols[agg[1]][m]
    if fn == "sum_product":
        return sum(int(a) * int(b) for a, b in zip(v, cols[agg[2]][m]))
    if v.dtype.kind == "f":
        return [float(x) for x in v] if fn == "sum" else (float(v.min()) if fn == "min" else float(v.max()))
    return sum(int(x) for x in v) if fn == "sum" else (int(v.min()) if fn == "min" else int(v.max()))


def check_value(got, want, what):
    if isinstance(want, list):   # a binary64 sum of finite values within its a-priori bound (test_aggregate.py's)
        exact = math.fsum(want)
        tol = (len(want) - 1) * 2.0 ** -53 * math.fsum(abs(x) for x in want)
        assert got is not None and abs(got - exact) <= tol, (what, got, exact, tol)
    else:
        assert got == want and type(got) is type(want), (what, got, want)


def nonvacuous(where, cond):
    """the condition selects some but not all of the filter's rows, in the
    table and inside the partial tail vector"""
    both = where & cond
    assert 0 < both.sum() < where.sum(), (both.sum(), where.sum())
    assert 0 < both[TAIL:].sum() < where[TAIL:].sum(), (both[TAIL:].sum(), where[TAIL:].sum())


def eng(terms, handles):
    """the terms as the engine takes them: a set's name replaced by its KeySet"""
    return [(t[0], t[1], handles[t[2]], *t[3:]) if t[1] in ("in_set", "not_in_set") else t for t in terms]


FUNCS = [("count",), ("count", C_N), ("sum", C_I), ("sum", C_D), ("sum", C_G), ("min", C_I), ("max", C_D),
         ("min", C_G), ("max", C_N), ("sum_product", C_D, C_Q), ("sum_product", C_N, C_J),
         ("sum_expr", [(0, 1, C_D), (100, -1, C_Q)]), ("sum_expr", [(0, 1, C_N), (3, 1, C_J), (-2, 1, C_Q)])]


# ------------------------------------------------------------------ CPU tests
def test_export_and_ctypes_layout(fl, _built):
    assert hasattr(C.CDLL(str(LIB)), "fls_aggregate_conditions")
    assert C.sizeof(fl.AggregateSpec) == 16 and fl.AggregateSpec.cond.offset == 12
    assert C.sizeof(fl.AggCondition) == 8 and fl.AggCondition.n.offset == 4
    assert fl.MAX_AGG_CONDITIONS == 8


def test_when_packs_and_dedupes(fl):
    c1 = [(C_I, ">", 0), (C_K, "=", 1, 4), (C_K, "=", 2, 4)]
    c2 = [(C_J, "<", fl.Col(C_I))]
    aggs = [("count",), fl.When(("count",), c1), fl.When(("sum", C_D), c2), fl.When(("sum_product", C_D, C_Q), list(c1)),
            fl.When(("sum_expr", [(0, 1, C_D)]), [(C_J, "<", fl.Col(C_I))]), ("sum_expr", [(1, -1, C_Q)])]
    arr, exprs, conds = fl._agg_specs(aggs)
    assert [a.cond for a in arr] == [0, 1, 2, 1, 2, 0]
    assert conds == [c1, c2]
    assert [(a.fn, a.col, a.col2) for a in arr] == [(0, 0, 0), (0, 0, 0), (2, C_D, 0), (5, C_D, C_Q), (6, 0, 0), (6, 1, 0)]
    assert exprs == [[(0, 1, C_D)], [(1, -1, C_Q)]]
    assert fl._agg_specs([("count",), ("sum", 3)])[2] == []
    assert repr(fl.When(("count",), [(1, "=", 2)])) == "When(('count',), [(1, '=', 2)])"


def raises_arg(fl, match):
    return pytest.raises(fl.FlsError, match=match)


def test_condition_list_errors(fl, conn, tab):
    t, _, _ = tab
    with raises_arg(fl, r"9 conditions \(at most 8\)") as e:
        t.set_aggregate_conditions([[(C_I, "=", 1)]] * 9)
    assert e.value.code == ERR_ARG
    with raises_arg(fl, r"condition 1: no term") as e:
        t.set_aggregate_conditions([[(C_I, "=", 1)], []])
    assert e.value.code == ERR_ARG
    # a range past npreds, through the C call itself
    preds, n, _keep = t._preds([(C_I, "=", 1), (C_I, "=", 2)])
    for first, cnt in [(1, 2), (3, 1), (0xFFFFFFFF, 2)]:
        rng = (fl.AggCondition * 2)()
        rng[0].first, rng[0].n, rng[1].first, rng[1].n = 0, 1, first, cnt
        rc = fl._lib.fls_aggregate_conditions(t.h, preds, n, rng, 2)
        assert rc == ERR_ARG and "condition 1: terms [" in fl.last_error() and "past the 2 predicates" in fl.last_error()
    ks = conn.keyset(np.array([1, 2, 3], np.int64))
    # every refusal fls_scan_filter gives a term, prefixed, the term's number local to the condition
    ok = [(C_I, "=", 1), (C_K, "=", 2)]
    for cond, frag in [
            ([(C_I, "=", 1), (99, "=", 1)], r"condition 1, term 1: filter column 99 out of range"),
            ([(C_I, 77, 1)], r"condition 1, term 0: filter operator 77 unknown"),
            ([(C_I, ">", 0), (C_I, ">", 1), (C_S, "in_set", ks)], r"condition 1, term 2: filter term 2: a key set cannot be probed"),
            ([(C_I, "in_set", 0x1235)], r"condition 1, term 0: filter term 0: value 0x1235 is not a live key set"),
            ([(C_I, "like", "a%")], r"condition 1, term 0: filter term 0: .*LIKE needs a VARCHAR column"),
            ([(C_S, "like", ("a%", "%"))], r"condition 1, term 0: filter term 0: the pattern ends in its escape byte"),
            ([(C_I, "<", fl.Col(C_S))], r"condition 1, term 0: filter term 0: a column comparison cannot read a VARCHAR"),
            ([(C_I, "<", fl.Col(C_G))], r"condition 1, term 0: filter term 0: an integer-like column against a FLOAT"),
            ([(C_K, "=", 1, 7), (C_I, "in_set", ks, 7)],
             r"condition 1, term 1: filter term 1: a key-set term shares clause 7 with term 0"),
            ([(C_S, "like", "a%", 7), (C_K, "=", 1, 7)],
             r"condition 1, term 0: filter term 0: a pattern term shares clause 7 with term 1"),
            ([(C_K, "=", 1, 3), (C_K, "=", 1, 7), (C_I, "<", fl.Col(C_J), 7)],
             r"condition 1, term 2: filter term 2: a column term shares clause 7 with term 1")]:
        with raises_arg(fl, frag) as e:
            t.set_aggregate_conditions([ok, cond])
        assert e.value.code == ERR_ARG
    # clause numbers are local to a condition: the same number in two conditions is no shared clause
    t.set_aggregate_conditions([[(C_I, "in_set", ks, 7)], [(C_K, "=", 1, 7)], [(C_I, "<", fl.Col(C_J), 7)]])
    t.set_aggregate_conditions(None)
    ks.close()


def spec(fl, *items):
    arr = (fl.AggregateSpec * len(items))()
    for a, (fn, col, cond) in zip(arr, items):
        a.fn, a.col, a.cond = fn, col, cond
    return arr


def test_condition_out_of_range_sticky_and_clear(fl, tab):
    """every aggregate call refuses a cond past the list before any device
    work (no GPU here); the list stays until it is replaced or cleared"""
    t, _, _ = tab
    out = (fl.AggregateValue * 2)()
    res = C.c_void_p()
    key = (C.c_uint32 * 1)(C_K)
    calls = [lambda a: fl._lib.fls_aggregate(t.h, a, 2, 0, 6, out),
             lambda a: fl._lib.fls_aggregate_grouped(t.h, key, 1, a, 2, 0, 6, C.byref(res)),
             lambda a: fl._lib.fls_aggregate_hashed(t.h, key, 1, a, 2, 16, 0, 6, C.byref(res))]
    for call in calls:
        assert call(spec(fl, (0, 0, 0), (0, 0, 1))) == ERR_ARG
        assert "aggregate 1: condition 0 out of range (0 set by fls_aggregate_conditions)" in fl.last_error()
    t.set_aggregate_conditions([[(C_I, ">", 0)], [(C_K, "=", 1)]])
    for _ in range(2):   # sticky: the same answer twice
        for call in calls:
            assert call(spec(fl, (0, 0, 2), (0, 0, 3))) == ERR_ARG
            assert "aggregate 1: condition 2 out of range (2 set by fls_aggregate_conditions)" in fl.last_error()
    t.set_aggregate_conditions([[(C_I, ">", 0)]])   # replaced as a whole
    assert calls[0](spec(fl, (0, 0, 0), (0, 0, 2))) == ERR_ARG
    assert "condition 1 out of range (1 set by" in fl.last_error()
    t.set_aggregate_conditions([])
    assert calls[0](spec(fl, (0, 0, 0), (0, 0, 1))) == ERR_ARG
    assert "condition 0 out of range (0 set by" in fl.last_error()
    # a failed replacement keeps the list
    t.set_aggregate_conditions([[(C_I, ">", 0)]])
    with raises_arg(fl, "condition 0, term 0"):
        t.set_aggregate_conditions([[(99, "=", 1)]])
    assert calls[0](spec(fl, (0, 0, 0), (0, 0, 2))) == ERR_ARG and "(1 set by" in fl.last_error()
    t.set_aggregate_conditions(None)


def test_grouped_refuses_a_condition_on_a_varchar_key(fl, tab):
    t, _, _ = tab
    with raises_arg(fl, r"key 1: VARCHAR column 5 is read by a term of condition 0") as e:
        t.aggregate_grouped([C_K, C_S], [("count",), fl.When(("count",), [(C_S, "=", "STANDARD")])])
    assert e.value.code == ERR_ARG
    with raises_arg(fl, r"key 0: VARCHAR column 5 is read by a term of condition 0"):
        t.aggregate_grouped([C_S], [fl.When(("sum", C_I), [(C_K, "=", 1), (C_S, "like", "PROMO%")])])
    # the wrappers cleared the list after the failed calls
    assert fl._lib.fls_aggregate(t.h, spec(fl, (0, 0, 1)), 1, 0, 6, (fl.AggregateValue * 1)()) == ERR_ARG
    assert "(0 set by fls_aggregate_conditions)" in fl.last_error()


# ------------------------------------------------------------------ GPU tests
WHERE = [(C_J, ">=", 0), (C_ID, "!=", 17)]
COND = [(C_I, ">", 0), (C_K, "<=", 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [None, WHERE], ids=["nofilter", "filter"])
def test_gpu_every_function_under_a_condition(fl, gpu, tab, filt, monkeypatch):
    t, cols, valid = tab
    where = ref_mask(fl, cols, filt or [], valid)
    cond = ref_mask(fl, cols, COND, valid)
    nonvacuous(where, cond)
    aggs = [fl.When(a, COND) for a in FUNCS] + FUNCS   # conditioned and plain in one call
    monkeypatch.delenv("FLS_SCAN_BATCH", raising=False)
    got = t.aggregate(aggs, filt)
    for a, g in zip(FUNCS, got[:len(FUNCS)]):
        check_value(g, ref_value(a, cols, where & cond & operand_valid(a, valid)), ("cond", a))
    for a, g in zip(FUNCS, got[len(FUNCS):]):
        check_value(g, ref_value(a, cols, where & operand_valid(a, valid)), ("plain", a))
    for batch in ("1", "3"):   # bit-identical across batch sizes (test_aggregate.py's arms), DOUBLE sums included
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)
        again = t.aggregate(aggs, filt)
        assert [repr(x) for x in again] == [repr(x) for x in got], batch


KIND_AGGS = [("count",), ("sum", C_D), ("count", C_N), ("sum_expr", [(0, 1, C_D), (100, -1, C_Q)])]
KINDS = {
    "or_clause": [(C_K, "=", 0, 1), (C_I, "<", -1, 1), (C_N, "is_null", None, 1)],
    "string_eq_dict": [(C_S, "=", "PROMO BRUSHED COPPER")],
    "string_ge_dict": [(C_S, ">=", "PROMO BRUSHED COPPER"), (C_S, "!=", "STANDARD")],
    "string_eq_fsst": [(C_F, "=", "take back return to sender")],
    "is_null": [(C_N, "is_null", None)],
    "is_not_null": [(C_N, "is_not_null", None), (C_K, "!=", 3)],
    "keyset_bitmap": [(C_I, "in_set", "bitmap")],
    "keyset_hash": [(C_I, "in_set", "hash")],
    "keyset_not_in": [(C_N, "not_in_set", "small")],
    "like": [(C_S, "like", "PROMO%")],
    "not_like_fsst": [(C_F, "not_like", "take%")],
    "column_pair": [(C_J, "<", ("@col", C_N))],   # (kind_terms makes it fl.Col(C_N))
    "mixed": [(C_K, "!=", 1), (C_S, "like", "PROMO%"), (C_I, "in_set", "hash"), (C_N, "is_not_null", None),
              (C_J, "<=", ("@col", C_I))],
}
SETS = {"bitmap": [-7, 0, 5, 12345], "hash": [-(1 << 40), 1, 1 << 40], "small": list(range(-50, 0))}


@pytest.fixture(scope="module")
def handles(fl, conn):
    h = {"bitmap": conn.keyset(np.array(SETS["bitmap"], np.int64), form=fl.KEYSET_BITMAP),
         "hash": conn.keyset(np.array(SETS["hash"], np.int64), form=fl.KEYSET_HASH),
         "small": conn.keyset(np.array(SETS["small"], np.int64))}
    assert h["bitmap"].info.form == fl.KEYSET_BITMAP and h["hash"].info.form == fl.KEYSET_HASH
    yield h
    for k in h.values():
        k.close()


def kind_terms(fl, name):
    return [(t[0], t[1], fl.Col(t[2][1]), *t[3:]) if isinstance(t[2], tuple) else t for t in KINDS[name]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(KINDS))
def test_gpu_condition_kinds(fl, gpu, tab, handles, name):
    t, cols, valid = tab
    terms = kind_terms(fl, name)
    for filt in (None, WHERE):
        where = ref_mask(fl, cols, filt or [], valid)
        cond = ref_mask(fl, cols, terms, valid, SETS)
        nonvacuous(where, cond)
        got = t.aggregate([fl.When(a, eng(terms, handles)) for a in KIND_AGGS] + [("count",)], filt)
        for a, g in zip(KIND_AGGS, got):
            check_value(g, ref_value(a, cols, where & cond & operand_valid(a, valid)), (name, a))
        assert got[-1] == int(where.sum())
        # consistency: the same aggregates from a call whose filter is where AND cond
        offset = [(c, op, v, *([100 + cl[0]] if cl else [])) for c, op, v, *cl in eng(terms, handles)]
        assert t.aggregate(KIND_AGGS, list(filt or []) + offset) == got[:-1], name


@pytest.mark.gpu
def test_gpu_eight_conditions_in_one_call(fl, gpu, tab, handles):
    t, cols, valid = tab
    conds = [[(C_K, "=", 0)], [(C_K, "=", 1), (C_I, ">", 0)], [(C_S, "like", "PROMO%")], [(C_I, "in_set", "hash")],
             [(C_J, "<", fl.Col(C_I))], [(C_N, "is_null", None)], [(C_F, "=", "none")],
             [(C_K, "=", 2, 1), (C_K, "=", 3, 1), (C_D, ">", 0)]]
    where = ref_mask(fl, cols, WHERE, valid)
    aggs, wants = [], []
    for c in conds:
        cond = ref_mask(fl, cols, c, valid, SETS)
        nonvacuous(where, cond)
        for a in (("count",), ("sum", C_D), ("max", C_N)):
            aggs.append(fl.When(a, eng(c, handles)))
            wants.append(ref_value(a, cols, where & cond & operand_valid(a, valid)))
    got = t.aggregate(aggs, WHERE)
    for a, g, w in zip(aggs, got, wants):
        check_value(g, w, a)
    assert len(set(got[0::3])) == 8   # eight different counts: no plane stands in for another
    with pytest.raises(fl.FlsError, match=r"9 conditions \(at most 8\)"):
        t.aggregate(aggs + [fl.When(("count",), [(C_K, "=", 9)])], WHERE)


@pytest.mark.gpu
def test_gpu_a_condition_prunes_nothing(fl, gpu, tab):
    t, cols, valid = tab
    filt = [(C_ID, ">=", RG)]   # prunes the first row group by its zone map
    never = [(C_ID, "<", 0)]    # no row group can match: as a filter it would prune all six
    assert not any(t.may_match(rg, never) for rg in range(6))
    where = ref_mask(fl, cols, filt, valid)
    plain = t.aggregate([("count",), ("sum", C_D)], filt)
    pruned = t.pruned
    assert pruned == 1
    got = t.aggregate([("count",), fl.When(("sum", C_D), never), fl.When(("count",), never), ("sum", C_D),
                       fl.When(("sum_expr", [(0, 1, C_D)]), never), fl.When(("min", C_G), never)], filt)
    assert t.pruned == pruned
    assert got == [int(where.sum()), None, 0, plain[1], None, None]
    # the raw record: count 0 and NULL
    t.set_aggregate_conditions([never])
    try:
        raw = t.aggregate_raw([(fl.AGG_FNS["sum"], C_D)])[0]   # unconditioned under a set list: exactly as before
        assert raw.count == N and raw.kind == fl.AGGV_INT
        arr = spec(fl, (fl.AGG_FNS["sum"], C_D, 1))
        out = (fl.AggregateValue * 1)()
        assert fl._lib.fls_aggregate(t.h, arr, 1, 0, 6, out) == 0
        assert out[0].count == 0 and out[0].kind == fl.AGGV_NULL
    finally:
        t.set_aggregate_conditions(None)


def group_by(cols, key, aggs_masks, where):
    """[(key, [mask per aggregate restricted to the key's rows])] in order of
    each key's first selected row"""
    keys = cols[key]
    first = {}
    for r in np.nonzero(where)[0]:
        first.setdefault(int(keys[r]), r)
    return [(k, [m & (keys == k) for m in aggs_masks]) for k in sorted(first, key=first.get)], first


GAGGS = [("count",), ("sum", C_D), ("sum", C_G), ("min", C_N), ("sum_expr", [(0, 1, C_D), (100, -1, C_Q)])]


@pytest.mark.gpu
def test_gpu_grouped_with_a_group_the_condition_never_meets(fl, gpu, tab, monkeypatch):
    t, cols, valid = tab
    cond = [(C_K, "!=", 2), (C_I, ">", 0)]   # group 2 exists and never meets it
    where, cm = ref_mask(fl, cols, WHERE, valid), ref_mask(fl, cols, cond, valid)
    nonvacuous(where, cm)
    aggs = [fl.When(a, cond) for a in GAGGS] + GAGGS
    masks = [where & cm & operand_valid(a, valid) for a in GAGGS] + [where & operand_valid(a, valid) for a in GAGGS]
    want, _ = group_by(cols, C_K, masks, where)
    monkeypatch.delenv("FLS_SCAN_BATCH", raising=False)
    got = t.aggregate_grouped([C_K], aggs, WHERE)
    assert [k for k, _ in got] == [(k,) for k, _ in want] and len(got) == 4
    for (k, vals), (_, ms) in zip(got, want):
        for a, g, m in zip(GAGGS + GAGGS, vals, ms):
            check_value(g, ref_value(a, cols, m), (k, a))
    two = dict(got)[(2,)]
    assert two[:5] == [0, None, None, None, None] and two[5] > 0 and two[6] is not None
    monkeypatch.setenv("FLS_SCAN_BATCH", "1")
    again = t.aggregate_grouped([C_K], aggs, WHERE)
    assert repr(again) == repr(got)
    # group membership follows the filter alone: the plain call forms the same groups with the same plain values
    plain = t.aggregate_grouped([C_K], GAGGS, WHERE)
    assert [(k, v[5:]) for k, v in again] == plain


HAGGS = [("count",), ("sum", C_D), ("max", C_N), ("sum_product", C_D, C_Q)]


@pytest.mark.gpu
def test_gpu_hashed_groups_first_rows_having_and_order(fl, gpu, tab):
    t, cols, valid = tab
    cond = [(C_K, "<=", 1), (C_S, "like", "PROMO%")]
    where, cm = ref_mask(fl, cols, WHERE, valid), ref_mask(fl, cols, cond, valid)
    nonvacuous(where, cm)
    aggs = [fl.When(a, cond) for a in HAGGS] + HAGGS
    masks = [where & cm & operand_valid(a, valid) for a in HAGGS] + [where & operand_valid(a, valid) for a in HAGGS]
    want, first = group_by(cols, C_OK, masks, where)
    hg = t.aggregate_hashed([C_OK], aggs, 4096, WHERE)
    got = hg.to_list()
    assert [k for k, _ in got] == [(k,) for k, _ in want]
    wants = {}
    for (k, vals), (_, ms) in zip(got, want):
        wants[k[0]] = [ref_value(a, cols, m) for a, m in zip(HAGGS + HAGGS, ms)]
        for a, g, w in zip(HAGGS + HAGGS, vals, wants[k[0]]):
            check_value(g, w, (k, a))
    empty = [k for k, w in wants.items() if w[0] == 0]
    assert empty and all(wants[k][1:4] == [None, None, None] and wants[k][4] > 0 for k in empty)   # such groups exist
    # the first rows are the filter's, with or without conditions
    plain = t.aggregate_hashed([C_OK], HAGGS, 4096, WHERE)
    order = np.argsort(hg.key_values[0])
    assert np.array_equal(np.sort(plain.key_values[0]), hg.key_values[0][order])
    assert np.array_equal(plain.first_row[np.argsort(plain.key_values[0])], hg.first_row[order])
    assert sorted(hg.first_row.tolist()) == sorted(first.values())
    # HAVING and ORDER BY on the conditioned sum (aggregate 1): a NULL satisfies no term and sorts last
    sel = t.aggregate_hashed([C_OK], aggs, 4096, WHERE, having=[(1, ">", 0)], order_by=(1, "desc"), limit=5)
    pos = sorted(((w[1], -first[k], k) for k, w in wants.items() if w[1] is not None and w[1] > 0), reverse=True)
    assert len(pos) > 5 and sel.groups_passed == len(pos)
    assert [(k[0], v[1]) for k, v in sel.to_list()] == [(k, s) for s, _, k in pos[:5]]
