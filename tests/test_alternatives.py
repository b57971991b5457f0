"""Filter alternatives, AND-groups joined by OR: the
export, the ctypes layout, the argument checks and the Python packing without a
GPU; alt_kernel, the narrowed planes and alt_merge_kernel on the GPU against
numpy, through every consumer of the scan's mask.

Shapes are test_agg_filter.py's: 1024-row row groups, five whole vectors and a
partial tail of 333 rows (a partial word and a partial vector), small value
pools, a nullable column with an all-NULL row group, a DICT and an FSST
VARCHAR, a sorted id.  The reference is numpy: helpers.filter_mask plus the
set / LIKE / column-pair extensions of test_agg_filter.py for the base filter
and for each alternative, OR-ed and then AND-ed.  Every case's reference is
checked first (facts): the union selects some but not all of the base
filter's rows, every alternative selects a row no other does, two of them
overlap (a double count would show), all of it inside the partial tail vector
too."""
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
SETS = {"bitmap": [-7, 0, 5, 12345], "hash": [-(1 << 40), 1, 1 << 40], "small": list(range(-50, 0))}


def make_columns():
    rng = np.random.default_rng(28)
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
    return cols, null, nv


COLS, NULL, NV = make_columns()   # computed once, shared and never changed
VALID = {C_N: ~NULL}


def make_image(fl):
    A = fl.ENC_AUTO
    specs = [("k", fl.INT32, COLS[C_K], A), ("i", fl.INT64, COLS[C_I], A), ("d", fl.DECIMAL, COLS[C_D], A, 15, 2),
             ("g", fl.DOUBLE, COLS[C_G], A), ("n", fl.INT64, np.ma.masked_array(NV, mask=NULL), A),
             ("s", fl.VARCHAR, [x.decode() for x in COLS[C_S]], fl.ENC_DICT),
             ("f", fl.VARCHAR, [x.decode() for x in COLS[C_F]], fl.ENC_FSST),
             ("id", fl.INT32, COLS[C_ID], A), ("j", fl.INT64, COLS[C_J], A), ("ok", fl.INT64, COLS[C_OK], A),
             ("q", fl.INT32, COLS[C_Q], A)]
    return fl.write_image(specs, rowgroup=RG)


@pytest.fixture(scope="module")
def conn(fl):
    c = fl.Connection([0])
    yield c
    c.close()


@pytest.fixture(scope="module")
def image(fl):
    return make_image(fl)


@pytest.fixture(scope="module")
def tab(fl, conn, image):
    t = conn.read_image(image)
    assert t.nrowgroups == 6
    yield t
    t.close()


@pytest.fixture(scope="module")
def handles(fl, conn):
    h = {"bitmap": conn.keyset(np.array(SETS["bitmap"], np.int64), form=fl.KEYSET_BITMAP),
         "hash": conn.keyset(np.array(SETS["hash"], np.int64), form=fl.KEYSET_HASH),
         "small": conn.keyset(np.array(SETS["small"], np.int64))}
    yield h
    for k in h.values():
        k.close()


# ---- the reference
def cmp_columns(a, b):
    return np.fromiter(((int(x) > int(y)) - (int(x) < int(y)) for x, y in zip(a, b)), np.int8, len(a))


def ref_mask(terms):
    """helpers.filter_mask extended as test_agg_filter.py's ref_mask: (a, op,
    ("@col", b)), (col, "in_set" / "not_in_set", name in SETS) and a prefix
    (col, "like" / "not_like", "p%"), each a clause of its own that holds only
    where the values are valid"""
    special = lambda t: isinstance(t[2], tuple) or t[1] in ("in_set", "not_in_set", "like", "not_like")  # noqa: E731
    out = filter_mask(COLS, [t for t in terms if not special(t)], N, VALID)
    for col, op, val, *_ in terms:
        if isinstance(val, tuple):
            hit = HOLDS[op](cmp_columns(COLS[col], COLS[val[1]]))
            if VALID.get(val[1]) is not None:
                hit = hit & VALID[val[1]]
        elif op in ("in_set", "not_in_set"):
            members = set(SETS[val])
            hit = np.fromiter((int(v) in members for v in COLS[col]), bool, N) == (op == "in_set")
        elif op in ("like", "not_like"):
            assert val.endswith("%") and "%" not in val[:-1] and "_" not in val
            hit = np.array([s.startswith(val[:-1].encode()) for s in COLS[col]], bool) == (op == "like")
        else:
            continue
        if VALID.get(col) is not None:
            hit = hit & VALID[col]
        out &= hit
    return out


def ref_select(base, alts):
    """(rows selected, the base filter's mask, each alternative's mask)"""
    b = ref_mask(base)
    am = [ref_mask(a) for a in alts]
    return b & np.any(am, axis=0), b, am


def facts(base, alts):
    """the four facts every GPU test asserts on its reference, in the table
    and inside the partial tail vector"""
    _, b, am = ref_select(base, alts)
    for sl in (slice(None), slice(TAIL, None)):
        bs = b[sl]
        within = [a[sl] & bs for a in am]
        union = np.any(within, axis=0)
        assert 0 < union.sum() < bs.sum(), (union.sum(), bs.sum())
        for i, a in enumerate(within):
            others = np.zeros(len(a), bool)
            for j, o in enumerate(within):
                if j != i:
                    others |= o
            assert (a & ~others).any(), ("alternative selects no row of its own", i)
        if len(within) > 1:
            assert any((within[i] & within[j]).any() for i in range(len(within)) for j in range(i)), "no overlap"


def eng(fl, terms, handles):
    """the terms as the engine takes them: a set's name replaced by its KeySet,
    ("@col", b) by fl.Col(b)"""
    out = []
    for t in terms:
        if t[1] in ("in_set", "not_in_set"):
            t = (t[0], t[1], handles[t[2]], *t[3:])
        elif isinstance(t[2], tuple):
            t = (t[0], t[1], fl.Col(t[2][1]), *t[3:])
        out.append(t)
    return out


def filt_of(fl, base, alts, handles):
    return eng(fl, base, handles) + [fl.AnyOf(*[eng(fl, a, handles) for a in alts])]


WHERE = [(C_J, ">=", 0), (C_ID, "!=", 17)]
CLOSED = [[(C_K, "=", 0), (C_Q, "<=", 30)],
          [(C_K, "=", 1, 1), (C_K, "=", 0, 1), (C_I, ">", 0)],
          [(C_Q, ">=", 25), (C_Q, "<=", 35)]]
OPEN = [[(C_I, "in_set", "bitmap")], [(C_S, "like", "PROMO%")], [(C_F, "like", "take%")], [(C_J, "<", ("@col", C_I))]]
MIX = [[(C_K, "=", 0), (C_Q, "<=", 30)],
       [(C_I, "in_set", "hash"), (C_K, "!=", 3)],
       [(C_S, "like", "PROMO%"), (C_J, "<", ("@col", C_I)), (C_Q, ">", 10)]]
NULLABLE = [[(C_N, ">", 10)], [(C_N, "is_null", None), (C_K, "=", 1)], [(C_N, "not_in_set", "small"), (C_K, "<=", 1)]]
ALONE = [[(C_I, "in_set", "hash"), (C_K, "!=", 3)]]
CASES = {"closed": (WHERE, CLOSED), "open": (WHERE, OPEN), "mix": (WHERE, MIX), "empty_base": ([], MIX),
         "alone": (WHERE, ALONE), "nullable": (WHERE, NULLABLE)}


# ------------------------------------------------------------------ CPU tests
def test_export_and_ctypes_layout(fl, _built):
    assert hasattr(C.CDLL(str(LIB)), "fls_scan_filter_alternatives")
    assert C.sizeof(fl.FilterAlternative) == 8 and fl.FilterAlternative.first.offset == 0
    assert fl.FilterAlternative.n.offset == 4
    assert fl.MAX_FILTER_ALTERNATIVES == 8


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_facts_hold(name):
    facts(*CASES[name])


def raises_arg(fl, match):
    return pytest.raises(fl.FlsError, match=match)


def test_alternative_list_errors(fl, conn, tab):
    t = tab
    with raises_arg(fl, r"9 alternatives \(at most 8\)") as e:
        t.set_filter_alternatives([[(C_I, "=", 1)]] * 9)
    assert e.value.code == ERR_ARG
    # an empty alternative and a range past npreds, through the C call itself
    preds, n, _keep = t._preds([(C_I, "=", 1), (C_I, "=", 2)])
    rng = (fl.FilterAlternative * 2)()
    rng[0].first, rng[0].n, rng[1].first, rng[1].n = 0, 1, 1, 0
    assert fl._lib.fls_scan_filter_alternatives(t.h, preds, n, rng, 2) == ERR_ARG
    assert "alternative 1: no term" in fl.last_error()
    for first, cnt in [(1, 2), (3, 1), (0xFFFFFFFF, 2)]:
        rng[1].first, rng[1].n = first, cnt
        rc = fl._lib.fls_scan_filter_alternatives(t.h, preds, n, rng, 2)
        assert rc == ERR_ARG and "alternative 1: terms [" in fl.last_error() and "past the 2 predicates" in fl.last_error()
    ks = conn.keyset(np.array([1, 2, 3], np.int64))
    # every refusal fls_scan_filter gives a term, prefixed, the term's number local to the alternative
    ok = [(C_I, "=", 1), (C_K, "=", 2)]
    for alt, frag in [
            ([(C_I, "=", 1), (99, "=", 1)], r"alternative 1, term 1: filter column 99 out of range"),
            ([(C_I, 77, 1)], r"alternative 1, term 0: filter operator 77 unknown"),
            ([(C_I, ">", 0), (C_I, ">", 1), (C_S, "in_set", ks)],
             r"alternative 1, term 2: filter term 2: a key set cannot be probed"),
            ([(C_I, "in_set", 0x1235)], r"alternative 1, term 0: filter term 0: value 0x1235 is not a live key set"),
            ([(C_I, "like", "a%")], r"alternative 1, term 0: filter term 0: .*LIKE needs a VARCHAR column"),
            ([(C_S, "like", ("a%", "%"))], r"alternative 1, term 0: filter term 0: the pattern ends in its escape byte"),
            ([(C_I, "<", fl.Col(C_S))], r"alternative 1, term 0: filter term 0: a column comparison cannot read a VARCHAR"),
            ([(C_I, "<", fl.Col(C_G))], r"alternative 1, term 0: filter term 0: an integer-like column against a FLOAT"),
            ([(C_K, "=", 1, 7), (C_I, "in_set", ks, 7)],
             r"alternative 1, term 1: filter term 1: a key-set term shares clause 7 with term 0"),
            ([(C_S, "like", "a%", 7), (C_K, "=", 1, 7)],
             r"alternative 1, term 0: filter term 0: a pattern term shares clause 7 with term 1"),
            ([(C_K, "=", 1, 3), (C_K, "=", 1, 7), (C_I, "<", fl.Col(C_J), 7)],
             r"alternative 1, term 2: filter term 2: a column term shares clause 7 with term 1")]:
        with raises_arg(fl, frag) as e:
            t.set_filter_alternatives([ok, alt])
        assert e.value.code == ERR_ARG
        with raises_arg(fl, frag):   # the same refusal through a filt, which leaves no half of the filter behind
            t.set_filter([(C_K, "=", 1), fl.AnyOf(ok, alt)])
    # the per-filter pattern limit holds per alternative: 8 pattern terms pass in each, a ninth is refused
    eight = [(C_S, "like", f"{c}%") for c in "abcdefgh"]
    t.set_filter_alternatives([eight, list(eight)])
    with raises_arg(fl, r"alternative 1, term \d: "):
        t.set_filter_alternatives([eight, eight + [(C_S, "like", "i%")]])
    # clause numbers are local to an alternative: the same number in two of them is no shared clause
    t.set_filter_alternatives([[(C_I, "in_set", ks, 7)], [(C_K, "=", 1, 7)], [(C_I, "<", fl.Col(C_J), 7)]])
    t.set_filter_alternatives(None)
    ks.close()


def test_grouped_refuses_an_alternative_on_a_varchar_key(fl, tab):
    t = tab
    with raises_arg(fl, r"key 1: VARCHAR column 5 is read by a term of alternative 1") as e:
        t.aggregate_grouped([C_K, C_S], [("count",)], [fl.AnyOf([(C_K, "=", 1)], [(C_S, "=", "STANDARD")])])
    assert e.value.code == ERR_ARG
    assert not t._alts_set   # the wrapper cleared the list after the failed call


def test_python_value_errors(fl, tab):
    t = tab
    one, two = [(C_K, "=", 1)], [(C_I, ">", 0)]
    for filt, frag in [([fl.AnyOf(one), fl.AnyOf(two)], "2 AnyOf elements"),
                       ([fl.AnyOf(one, [fl.AnyOf(two)])], "alternative 1 of the AnyOf holds an AnyOf"),
                       ([(C_K, "=", 1), fl.AnyOf()], "an empty AnyOf"),
                       ([fl.AnyOf(one, [])], "alternative 1 of the AnyOf is empty")]:
        for call in (t.set_filter, lambda f: t.aggregate([("count",)], f), lambda f: list(t.scan_filtered(f)),
                     lambda f: t.topn(C_ID, 3, filt=f)):
            with pytest.raises(ValueError, match=frag):
                call(filt)
    with pytest.raises(ValueError, match="When: a condition holds no AnyOf"):
        fl.When(("count",), [fl.AnyOf(one, two)])
    with pytest.raises(ValueError, match="an AnyOf is an element of a call's filt"):
        t.may_match(0, [fl.AnyOf(one, two)])
    with pytest.raises(ValueError, match="an AnyOf is an element of a call's filt"):
        t.set_aggregate_conditions([[fl.AnyOf(one, two)]])
    assert repr(fl.AnyOf(one, two)) == "AnyOf([(0, '=', 1)], [(1, '>', 0)])"


def test_a_filter_without_anyof_packs_as_before(fl, tab, monkeypatch):
    t = tab
    filt = [(C_K, "=", 1, 4), (C_K, "=", 2, 4), (C_S, "like", "PROMO%"), (C_J, "<", fl.Col(C_I)), (C_G, ">", 1.5)]
    base, alts = fl._split_filter(filt)
    assert base == filt and alts is None
    assert fl._split_filter(None) == ([], None)
    # ... and makes the one library call it made before
    calls = []
    real = fl._lib.fls_scan_filter_alternatives
    monkeypatch.setattr(fl._lib, "fls_scan_filter_alternatives", lambda *a: calls.append(a) or real(*a))
    t.set_filter(filt)
    t._clear_filter()
    assert calls == []
    # with an AnyOf: the base terms go to fls_scan_filter, the rest to the new call, and a plain filter clears them
    base, alts = fl._split_filter([filt[0], fl.AnyOf(filt[1:3], filt[3:]), filt[1]])
    assert base == [filt[0], filt[1]] and alts == [filt[1:3], filt[3:]]
    preds, k, ranges, n, _parts = t._pack_lists(alts)
    assert (k, n) == (4, 2) and [(r.first, r.n) for r in ranges] == [(0, 2), (2, 2)]
    assert [preds[i].col for i in range(k)] == [C_K, C_S, C_J, C_G]
    t.set_filter([filt[0], fl.AnyOf(filt[1:3], filt[3:])])
    assert t._alts_set and len(calls) == 1
    t.set_filter(filt)
    assert not t._alts_set and len(calls) == 2
    t._clear_filter()
    assert len(calls) == 2


# ------------------------------------------------------------------ GPU tests
def scan_rows(t, filt, deliver=None):
    """(global rows selected, delivered arrays per column concatenated)"""
    rows, parts = [], {}
    for rg, first_row, sel, arrays in t.scan_filtered(filt, cols=deliver):
        rows.append(sel.astype(np.int64) + first_row)
        for c in deliver or []:
            parts.setdefault(c, []).append(arrays[c])
    return (np.concatenate(rows) if rows else np.zeros(0, np.int64)), parts


DELIVER = [C_ID, C_D, C_N, C_S]


def check_scan(fl, t, filt, want):
    got, parts = scan_rows(t, filt, DELIVER)
    assert np.array_equal(got, want), (len(got), len(want))
    for c in (C_ID, C_D, C_N):
        vals = np.concatenate(parts[c]).view(fl.NP_DTYPE[t.column(c).type])
        keep = np.ones(len(want), bool) if c not in VALID else VALID[c][want]
        assert np.array_equal(vals[keep], COLS[c][want][keep]), c
    assert fl.string_t_decode(np.concatenate(parts[C_S])) == [COLS[C_S][r] for r in want]
    return got, parts


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["closed", "open", "mix", "empty_base", "nullable"])
def test_gpu_scan_filtered(fl, gpu, tab, handles, name):
    base, alts = CASES[name]
    facts(base, alts)
    want = np.nonzero(ref_select(base, alts)[0])[0]
    check_scan(fl, tab, filt_of(fl, base, alts, handles), want)
    assert not tab._alts_set   # cleared with the filter


@pytest.mark.gpu
def test_gpu_one_alternative_equals_its_terms_in_the_filter(fl, gpu, tab, handles):
    base, alts = CASES["alone"]
    facts(base, alts)
    want = np.nonzero(ref_select(base, alts)[0])[0]
    got, parts = check_scan(fl, tab, filt_of(fl, base, alts, handles), want)
    plain, pparts = scan_rows(tab, eng(fl, base + alts[0], handles), DELIVER)
    assert np.array_equal(got, plain)
    for c in DELIVER:
        assert np.array_equal(np.concatenate(parts[c]), np.concatenate(pparts[c])), c


AGGS = [("count",), ("count", C_N), ("sum", C_D), ("sum", C_G), ("min", C_I), ("max", C_N),
        ("sum_product", C_D, C_Q), ("sum_expr", [(0, 1, C_D), (100, -1, C_Q)])]


def operand_valid(agg):
    m = np.ones(N, bool)
    cs = [f[2] for f in agg[1]] if agg[0] == "sum_expr" else list(agg[1:])
    for c in cs:
        if VALID.get(c) is not None:
            m &= VALID[c]
    return m


def ref_value(agg, m):
    """the aggregate over the rows of m in Python integers; a DOUBLE sum as the list of its addends"""
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
                p *= k + sign * int(COLS[c][r])
            total += p
        return total
    v = COLS[agg[1]][m]
    if fn == "sum_product":
        return sum(int(a) * int(b) for a, b in zip(v, COLS[agg[2]][m]))
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


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["closed", "mix", "empty_base"])
def test_gpu_aggregate_counts_a_row_once(fl, gpu, tab, handles, name):
    base, alts = CASES[name]
    facts(base, alts)
    sel = ref_select(base, alts)[0]
    got = tab.aggregate(AGGS, filt_of(fl, base, alts, handles))
    for a, g in zip(AGGS, got):
        check_value(g, ref_value(a, sel & operand_valid(a)), (name, a))


@pytest.mark.gpu
def test_gpu_aggregate_with_a_condition_on_top(fl, gpu, tab, handles):
    base, alts = CASES["mix"]
    facts(base, alts)
    sel = ref_select(base, alts)[0]
    cond = [(C_I, ">", 0), (C_F, "not_like", "take%")]
    cm = ref_mask(cond)
    assert 0 < (sel & cm).sum() < sel.sum() and 0 < (sel & cm)[TAIL:].sum() < sel[TAIL:].sum()
    got = tab.aggregate([fl.When(a, cond) for a in AGGS] + AGGS, filt_of(fl, base, alts, handles))
    for a, g in zip(AGGS, got[:len(AGGS)]):
        check_value(g, ref_value(a, sel & cm & operand_valid(a)), ("cond", a))
    for a, g in zip(AGGS, got[len(AGGS):]):
        check_value(g, ref_value(a, sel & operand_valid(a)), ("plain", a))


def group_by(key_values, masks, where):
    """[(key, [mask per aggregate restricted to the key's rows])] in order of
    each key's first selected row"""
    first = {}
    for r in np.nonzero(where)[0]:
        first.setdefault(int(key_values[r]), r)
    return [(k, [m & (key_values == k) for m in masks]) for k in sorted(first, key=first.get)], first


GAGGS = [("count",), ("sum", C_D), ("sum", C_G), ("min", C_N), ("sum_expr", [(0, 1, C_D), (100, -1, C_Q)])]


@pytest.mark.gpu
def test_gpu_grouped_plain_and_mapped_key(fl, gpu, conn, tab, handles):
    base, alts = CASES["mix"]
    facts(base, alts)
    sel = ref_select(base, alts)[0]
    filt = filt_of(fl, base, alts, handles)
    want, _ = group_by(COLS[C_K], [sel & operand_valid(a) for a in GAGGS], sel)
    got = tab.aggregate_grouped([C_K], GAGGS, filt)
    assert [k for k, _ in got] == [(k,) for k, _ in want] and len(got) == 4
    for (k, vals), (_, ms) in zip(got, want):
        for a, g, m in zip(GAGGS, vals, ms):
            check_value(g, ref_value(a, m), (k, a))
    # a mapped key (an inner join on q: odd quantities belong to no group), which narrows the mask after the merge
    km = conn.keymap(np.arange(2, 51, 2), np.arange(2, 51, 2) % 3)
    try:
        inner = sel & (COLS[C_Q] % 2 == 0)
        code = (COLS[C_Q] % 3).astype(np.int64)
        want, _ = group_by(code, [inner & operand_valid(a) for a in GAGGS], inner)
        got = tab.aggregate_grouped([("map", C_Q, km)], GAGGS, filt)
        assert [k for k, _ in got] == [(k,) for k, _ in want] and len(got) == 3
        for (k, vals), (_, ms) in zip(got, want):
            for a, g, m in zip(GAGGS, vals, ms):
                check_value(g, ref_value(a, m), (k, a))
    finally:
        km.close()


HAGGS = [("count",), ("sum", C_D), ("max", C_N), ("sum_product", C_D, C_Q)]


@pytest.mark.gpu
def test_gpu_hashed_and_having(fl, gpu, tab, handles):
    base, alts = CASES["mix"]
    facts(base, alts)
    sel = ref_select(base, alts)[0]
    filt = filt_of(fl, base, alts, handles)
    want, first = group_by(COLS[C_OK], [sel & operand_valid(a) for a in HAGGS], sel)
    hg = tab.aggregate_hashed([C_OK], HAGGS, 4096, filt)
    got = hg.to_list()
    assert [k for k, _ in got] == [(k,) for k, _ in want]
    wants = {}
    for (k, vals), (_, ms) in zip(got, want):
        wants[k[0]] = [ref_value(a, m) for a, m in zip(HAGGS, ms)]
        for a, g, w in zip(HAGGS, vals, wants[k[0]]):
            check_value(g, w, (k, a))
    assert sorted(hg.first_row.tolist()) == sorted(first.values())
    # HAVING count(*) >= 2: a group of four rows that two alternatives select once each or one row twice would differ
    picked = tab.aggregate_hashed([C_OK], HAGGS, 4096, filt, having=[(0, ">=", 2)], order_by=(1, "desc"), limit=5)
    pos = sorted(((w[1], -first[k], k) for k, w in wants.items() if w[0] >= 2), reverse=True)
    assert len(pos) > 5 and picked.groups_passed == len(pos)
    assert [(k[0], v[1]) for k, v in picked.to_list()] == [(k, s) for s, _, k in pos[:5]]


@pytest.mark.gpu
def test_gpu_topn(fl, gpu, tab, handles):
    base, alts = CASES["mix"]
    facts(base, alts)
    sel = ref_select(base, alts)[0]
    filt = filt_of(fl, base, alts, handles)
    for desc in (False, True):
        rows, values, _ = tab.topn(C_D, 100, cols=[C_ID, C_D], filt=filt, desc=desc)
        cand = np.nonzero(sel)[0]
        k = COLS[C_D][cand]
        order = cand[np.lexsort((cand, -k if desc else k))][:100]
        assert np.array_equal(rows.astype(np.int64), order), desc
        assert np.array_equal(values[C_ID], COLS[C_ID][order]) and np.array_equal(values[C_D], COLS[C_D][order])
    # with alternatives and no base filter the scan is filtered: no zone-map cut on the sorted key
    sel0 = ref_select([], alts)[0]
    rows, _, _ = tab.topn(C_ID, 10, cols=[C_ID], filt=filt_of(fl, [], alts, handles), desc=True)
    assert np.array_equal(rows.astype(np.int64), np.nonzero(sel0)[0][::-1][:10])


@pytest.mark.gpu
def test_gpu_identical_across_batches_and_pipelines(fl, gpu, tab, image, handles, monkeypatch):
    cases = [CASES["mix"], CASES["open"], CASES["empty_base"]]
    for base, alts in cases:
        facts(base, alts)
    want = [np.nonzero(ref_select(b, a)[0])[0] for b, a in cases]
    filts = [filt_of(fl, b, a, handles) for b, a in cases]
    monkeypatch.delenv("FLS_SCAN_BATCH", raising=False)
    aggs = [tab.aggregate(AGGS, f) for f in filts]
    for batch in ("1", "3", "8"):
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)
        for f, w, a in zip(filts, want, aggs):
            assert np.array_equal(scan_rows(tab, f)[0], w), batch
            assert [repr(x) for x in tab.aggregate(AGGS, f)] == [repr(x) for x in a], batch
    monkeypatch.delenv("FLS_SCAN_BATCH")
    two = fl.Connection([0, 0])   # two scan pipelines on one device
    try:
        tm = two.read_image(image)
        sets2 = {k: two.keyset(np.array(v, np.int64)) for k, v in SETS.items()}
        for (b, a), w, g in zip(cases, want, aggs):
            f = filt_of(fl, b, a, sets2)
            assert np.array_equal(np.sort(scan_rows(tm, f)[0]), w)
            assert [repr(x) for x in tm.aggregate(AGGS, f)] == [repr(x) for x in g]
        for k in sets2.values():
            k.close()
        tm.close()
    finally:
        two.close()


@pytest.mark.gpu
def test_gpu_pruning_on_the_sorted_id(fl, gpu, tab):
    t = tab
    ends = fl.AnyOf([(C_ID, "<", 1024)], [(C_ID, ">=", 4096)])
    ids = COLS[C_ID]
    want = np.nonzero((ids < 1024) | (ids >= 4096))[0]
    assert np.array_equal(scan_rows(t, [ends])[0], want) and t.pruned == 3
    assert t.aggregate([("count",)], [ends]) == [len(want)] and t.pruned == 3
    # a base term that excludes row group 0
    want = np.nonzero(ids >= 4096)[0]
    assert np.array_equal(scan_rows(t, [(C_ID, ">=", 1024), ends])[0], want) and t.pruned == 4
    assert t.topn(C_ID, 5, cols=[C_ID], filt=[(C_ID, ">=", 1024), ends])[0].tolist() == want[:5].tolist()
    assert t.pruned == 4
    # row group 1: the first alternative's zone map excludes it, the second accepts it: read
    mixed = fl.AnyOf([(C_ID, "<", 1000)], [(C_ID, ">=", 1500), (C_ID, "<", 1600)])
    want = np.nonzero((ids < 1000) | ((ids >= 1500) & (ids < 1600)))[0]
    seen = [rg for rg, _, sel, _ in t.scan_filtered([mixed]) if len(sel)]
    assert seen == [0, 1] and t.pruned == 4
    assert np.array_equal(scan_rows(t, [mixed])[0], want)
    # every alternative ruled out everywhere: no row group to read, in every call
    never = fl.AnyOf([(C_ID, "<", 0)], [(C_ID, ">", N)])
    assert list(t.scan_filtered([never])) == [] and t.pruned == 6
    assert t.aggregate([("count",), ("sum", C_D)], [never]) == [0, None]
    assert t.aggregate_grouped([C_K], [("count",)], [never]) == []
    assert t.aggregate_hashed([C_OK], [("count",)], 16, [never]).to_list() == []
    assert len(t.topn(C_ID, 3, filt=[never])[0]) == 0


@pytest.mark.gpu
def test_gpu_a_freed_keyset_handle_stays_usable(fl, gpu, conn, tab):
    t = tab
    base, alts = CASES["mix"]
    sets = {k: conn.keyset(np.array(v, np.int64)) for k, v in SETS.items()}
    t.set_filter(filt_of(fl, base, alts, sets))
    for k in sets.values():
        k.close()   # the alternatives hold the sets as the filter holds them
    try:
        out = (fl.AggregateValue * 1)()
        arr = (fl.AggregateSpec * 1)()
        arr[0].fn = fl.AGG_FNS["count_star"]
        assert fl._lib.fls_aggregate(t.h, arr, 1, 0, 6, out) == 0, fl.last_error()
        assert out[0].lo == int(ref_select(base, alts)[0].sum())
    finally:
        t._clear_filter()
