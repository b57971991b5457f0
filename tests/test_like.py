"""String pattern filter terms: `column LIKE pattern [ESCAPE c]` / NOT LIKE
pushed down to the GPU (csrc/fls_strmatch.hpp, csrc/fls_strmatch.hip).

Small hand-built tables (1024-row row groups, a 37-row tail), the string pool
and the pattern list of like_ref.py.  Every expected value comes from
like_ref.ref_like, a memoised recursive matcher written from the semantics in
include/flsgpu.h, over the byte strings handed to write_image -- never from
the engine.  All comparisons exact."""
import numpy as np
import pytest

from helpers import chunk_encodings, rg_slice
from like_ref import (A299B, A300, OPS, PATTERNS, POOL, facts, like_mask, needs_retry, pat_text, ref_like, route,
                      term)

RG = 1024
N = 2 * RG + 37
BATCHES = [None, "1", "3"]        # FLS_SCAN_BATCH: the default (8 row groups), 1, 3
C_D, C_F, C_N, C_ID, C_G, C_K = range(6)
NAMES = {C_D: "d", C_F: "f", C_N: "n"}


def set_batch(monkeypatch, batch):
    if batch is None:
        monkeypatch.delenv("FLS_SCAN_BATCH", raising=False)
    else:
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)


def count_star(t, terms):
    return t.aggregate([("count",)], filt=terms)[0]


@pytest.fixture(scope="module")
def tab(fl):
    rng = np.random.default_rng(20250611)
    vals = [POOL[k] for k in rng.integers(0, len(POOL), N)]
    for i, s in enumerate(POOL):          # every string in the first row group, some around word ends
        vals[(61 * i) % RG] = s
    null = rng.random(N) < 0.2
    ids = np.arange(N, dtype=np.int32)
    g = (ids % 5).astype(np.int32)
    k = ((ids * 7919) % 600).astype(np.int32)
    img = fl.write_image([("d", fl.VARCHAR, vals, fl.ENC_DICT), ("f", fl.VARCHAR, vals, fl.ENC_FSST),
                          ("n", fl.VARCHAR, [None if z else v for v, z in zip(vals, null)], fl.ENC_AUTO),
                          ("id", fl.INT32, ids, fl.ENC_FFOR), ("g", fl.INT32, g, fl.ENC_AUTO),
                          ("k", fl.INT32, k, fl.ENC_AUTO)], rowgroup=RG)
    t = fl.Connection([0]).read_image(img)
    cols = {C_D: vals, C_F: vals, C_N: vals, C_ID: ids, C_G: g, C_K: k}
    return img, t, cols, {C_N: ~null}


# one VARCHAR column whose chunks are DICT, FSST, DICT, FSST (ENC_AUTO chooses per chunk)
N_M = 3 * RG + 37
M_WORDS = [b"abcdefghijklm", b"abcd", b"the green abc of abcdefghijklmnop", b"xabyabab", b"caf\xc3\xa9s"]


def mixed_rows():
    rng = np.random.default_rng(78)
    s = [M_WORDS[k] for k in rng.integers(0, len(M_WORDS), N_M)]
    for i in range(RG, 2 * RG):
        s[i] = POOL[i % len(POOL)][:40] + b" #%06d unique row" % i
    return s, np.arange(N_M, dtype=np.int32)


@pytest.fixture(scope="module")
def mixed(fl):
    s, ids = mixed_rows()
    img = fl.write_image([("s", fl.VARCHAR, s, fl.ENC_AUTO), ("id", fl.INT32, ids, fl.ENC_FFOR)], rowgroup=RG)
    return img, fl.Connection([0]).read_image(img), {0: s, 1: ids}


def check_scan(fl, t, cols, terms, deliver, valid=None):
    """check_filtered_scan of helpers.py with like_mask as the oracle: selection
    and delivered values bit-exact per row group, pruned row groups never delivered"""
    sch = t.schema()
    expect_pruned = sum(not t.may_match(rg, terms) for rg in range(t.nrowgroups))
    seen, total = set(), 0
    for rg, first_row, sel, arrays in t.scan_filtered(terms, cols=deliver):
        seen.add(rg)
        part = rg_slice(cols, rg, RG)
        n = t.rowgroup_rows(rg)
        want = np.nonzero(like_mask(part, terms, n, rg_slice(valid, rg, RG) if valid else None))[0]
        assert np.array_equal(sel, want), (rg, len(sel), len(want))
        total += len(sel)
        for c in deliver:
            keep = np.ones(len(want), bool) if not valid or c not in valid else valid[c][rg * RG + want]
            if sch[c][1] in fl.STRING_TYPES:
                got = fl.string_t_decode(arrays[c])
                assert len(got) == len(want), (sch[c][0], rg)
                assert [x for x, k in zip(got, keep) if k] == [part[c][i] for i in want[keep]], (sch[c][0], rg)
            else:
                got = arrays[c].view(fl.NP_DTYPE[sch[c][1]])
                assert np.array_equal(got[keep], part[c][want[keep]]), (sch[c][0], rg)
    assert t.pruned == expect_pruned
    assert len(seen) == t.nrowgroups - expect_pruned
    return total


# ------------------------------------------------------------------ CPU tests
def test_tables_are_what_the_tests_need(fl, ref, tab, mixed):
    img, t, cols, valid = tab
    assert set(cols[C_D]) == set(POOL)
    assert {len(s) for s in POOL} >= {0, 1, 4, 5, 12, 13, 36, 300}
    assert 0.1 < 1 - valid[C_N].mean() < 0.3
    rf = ref.RefFile(img)
    assert rf.strings_column(C_D) == cols[C_D] and rf.strings_column(C_F) == cols[C_F]
    encs = chunk_encodings(img.tobytes())
    assert [r[C_D] for r in encs] == [fl.ENC_DICT] * 3 and [r[C_F] for r in encs] == [fl.ENC_FSST] * 3
    mimg, mt, mcols = mixed
    assert [r[0] for r in chunk_encodings(mimg.tobytes())] == [fl.ENC_DICT, fl.ENC_FSST, fl.ENC_DICT, fl.ENC_FSST]
    assert ref.RefFile(mimg).strings_column(0) == mcols[0]


def test_matrix_is_not_vacuous(tab):
    img, t, cols, valid = tab
    kinds, routes = set(), set()
    for pat, esc in PATTERNS:
        s = int(like_mask(cols, [term(C_D, "like", pat, esc)], N).sum())
        kinds.add("none" if s == 0 else "all" if s == N else "part")
        for x in POOL:
            r = route(x, pat, esc)
            routes.add(r)
            if r in ("inline", "pointer"):
                routes.add((r, ref_like(x, pat, esc)))
            if needs_retry(x, pat, esc):
                routes.add("retry")
            if ref_like(x, pat, esc) and b"_" in pat and esc is None and any(b >= 0xC0 for b in x):
                routes.add("any1_multibyte")
    assert kinds == {"none", "all", "part"}
    # decided by length, by the inline prefix, from the record (<= 12 bytes), through a pointer
    # (DICT: the image; FSST: the batch heap -- columns d and f hold the same strings), each
    # with both verdicts where the matcher runs; a retry after %; _ over a multi-byte character
    assert routes >= {"length", "prefix", "inline", "pointer", ("inline", True), ("inline", False),
                      ("pointer", True), ("pointer", False), "retry", "any1_multibyte"}
    assert needs_retry(b"abxababc", b"%ab%abc", None)
    assert ref_like(A299B, b"%a%a%a%a%b", None) and not ref_like(A300, b"%a%a%a%a%b", None)
    assert facts(PATTERNS[-1][0])[0] == 256 and facts(PATTERNS[-2][0])[0] == 256
    for ch in ("é", "€", "\U0001F600"):
        assert ref_like(ch.encode(), b"_", None) and not ref_like(ch.encode(), b"__", None)
    assert ref_like(b"\x80", b"_", None) and ref_like(b"ab\x80c", b"ab_c", None) and ref_like(b"ab\xe2\x82", b"ab_", None)
    assert ref_like(b"\x80\x80", b"_", None)      # the position stands on the first: the second continues it


def test_pruning_exact_on_dict_and_absent_on_fsst(fl, tab):
    img, t, cols, valid = tab
    some_pruned = False
    for pat, esc in PATTERNS:
        for op in OPS:
            for rg in range(t.nrowgroups):
                n = t.rowgroup_rows(rg)
                hit = like_mask(rg_slice(cols, rg, RG), [term(C_D, op, pat, esc)], n).any()
                assert t.may_match(rg, [term(C_D, op, pat, esc)]) == hit, (pat_text(pat, esc), op, rg)
                assert t.may_match(rg, [term(C_F, op, pat, esc)]), (pat_text(pat, esc), op, rg)
                some_pruned |= not hit
    assert some_pruned


def test_pruning_sugar_and_null_pattern(fl, tab):
    img, t, cols, valid = tab
    for op, lit, pat in [("starts_with", b"100%", b"100\\%%"), ("ends_with", b"a_b", b"%a\\_b"),
                         ("contains", b"\\", b"%\\\\%"), ("contains", "gre", b"%gre%"), ("starts_with", b"zz", b"zz%")]:
        for rg in range(t.nrowgroups):
            want = like_mask(rg_slice(cols, rg, RG), [(C_D, "like", (pat, b"\\"))], t.rowgroup_rows(rg)).any()
            assert t.may_match(rg, [(C_D, op, lit)]) == want, (op, lit, rg)
    assert fl.like_escape(b"50%_\\x") == b"50\\%\\_\\\\x"
    for op in OPS + ["starts_with"]:
        assert not any(t.may_match(rg, [(C_D, op, None)]) for rg in range(t.nrowgroups))   # a NULL pattern: no row
    assert t.may_match(0, [(C_D, "like", "abcd")]) and t.may_match(0, [(C_D, "like", ("abc!_", "!"))]) is False
    with pytest.raises(ValueError, match="escape"):
        t.may_match(0, [(C_D, "like", (b"x", b"ab"))])


def test_all_null_rowgroup_is_pruned_for_both_ops(fl):
    vals = [b"abcd"] * RG + [None] * RG + [b"abcd", None] * 10
    img = fl.write_image([("s", fl.VARCHAR, vals, fl.ENC_AUTO)], rowgroup=RG)
    t = fl.Connection([0]).read_image(img)
    for op in OPS:
        for pat in (b"%", b"abcd", b"zz%"):
            got = [t.may_match(rg, [(0, op, pat)]) for rg in range(3)]
            hit = ref_like(b"abcd", pat) == (op == "like")
            # (the 20-row tail's chunk may carry a placeholder for its NULLs: conservative, not exact)
            assert got[:2] == [hit, False] and (got[2] or not hit), (op, pat)


def test_argument_errors_name_the_term(fl):
    img = fl.write_image([("s", fl.VARCHAR, [b"a", b"b"] * 8, fl.ENC_DICT), ("b", fl.BLOB, [b"a", b"b"] * 8, fl.ENC_FSST),
                          ("i", fl.INT32, np.arange(16, dtype=np.int32), fl.ENC_AUTO)], rowgroup=RG)
    t = fl.Connection([0]).read_image(img)
    ok = (0, "like", b"a%")
    assert t.may_match(0, [ok])
    for terms, text in [
        ([ok, (1, "like", b"a%")], r"filter term 1: .*LIKE needs a VARCHAR column"),          # BLOB
        ([(2, "not_like", b"1%")], r"filter term 0: filter operator 12 unknown for column 2: LIKE needs a VARCHAR column"),          # INT
        ([(2, "=", 3, 7), (0, "like", b"a%", 7)], r"filter term 1: a pattern term shares clause 7 with term 0"),
        ([(0, "like", b"a%", 7), (0, "not_like", b"b%", 7)], r"filter term 0: a pattern term shares clause 7"),
        ([ok] * 9, r"filter term 8: more than 8 pattern terms"),
        ([ok, (0, "like", b"a" * 257)], r"filter term 1: the pattern compiles to more than 256 tokens"),
        ([(0, "not_like", (b"ab\\", b"\\"))], r"filter term 0: the pattern ends in its escape byte"),
    ]:
        with pytest.raises(fl.FlsError, match=text) as e:
            t.may_match(0, terms)
        assert e.value.code == -3, terms          # FLS_ERR_ARG
        with pytest.raises(fl.FlsError, match=text):
            t.set_filter(terms)
    # the limits themselves are allowed
    assert t.may_match(0, [ok] * 8) and not t.may_match(0, [(0, "like", b"a" * 256)])
    assert t.may_match(0, [(0, "like", b"%" * 300 + b"a")])


# ------------------------------------------------------------------ GPU tests
def run_matrix(fl, t, cols, col, id_col, valid, n, name):
    for pat, esc in PATTERNS:
        for op in OPS:
            terms = [term(col, op, pat, esc)]
            what = f"{name} {op} {pat_text(pat, esc)}"
            want = int(like_mask(cols, terms, n, valid).sum())
            assert count_star(t, terms) == want, what
            try:
                total = check_scan(fl, t, cols, terms, [col, id_col], valid=valid)
            except AssertionError as e:
                raise AssertionError(f"{what}: {e}") from e
            assert total == want, what


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("col", [C_D, C_F, C_N], ids=lambda c: NAMES[c])
def test_gpu_like_matrix(fl, gpu, tab, monkeypatch, col, batch):
    set_batch(monkeypatch, batch)
    img, t, cols, valid = tab
    run_matrix(fl, t, cols, col, C_ID, valid, N, NAMES[col])


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES)
def test_gpu_like_matrix_mixed_encodings(fl, gpu, mixed, monkeypatch, batch):
    """Default batch: the four chunks (DICT, FSST, DICT, FSST) share one batch,
    so long strings are reached through the file image and the batch heap at once."""
    set_batch(monkeypatch, batch)
    img, t, cols = mixed
    run_matrix(fl, t, cols, 0, 1, None, N_M, "mixed")


PAT_A = (C_D, "like", b"abcd%")
PAT_B = (C_F, "not_like", b"%e%")
PAT_N = (C_N, "like", b"%a%")


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES)
def test_gpu_like_combined_with_other_terms(fl, gpu, tab, monkeypatch, batch):
    set_batch(monkeypatch, batch)
    img, t, cols, valid = tab
    ks = t.conn.keyset(np.arange(0, 600, 3), signed=True)
    combos = {
        "int_range": [PAT_A, (C_ID, ">=", 100), (C_ID, "<", 1900)],
        "in_set": [(C_K, "in_set", ks), PAT_N],
        "two_patterns": [PAT_A, PAT_B],
        "two_patterns_nullable": [PAT_N, (C_F, "like", b"%b%"), (C_D, "not_like", b"_")],
        "tail_only": [PAT_N, (C_ID, ">=", 2 * RG)],                      # live rows end mid-word (37-row tail)
        "words_emptied_first": [(C_ID, ">=", 700), (C_ID, "<", 725), (C_F, "like", b"%a%")],   # 25 rows of one word
        "or_clause_beside": [(C_ID, "<", 50, 1), (C_ID, ">=", 2000, 1), PAT_B],
    }
    isin = np.isin(cols[C_K], np.arange(0, 600, 3))
    for name, terms in combos.items():
        rest = [x for x in terms if x[1] != "in_set"]
        want = like_mask(cols, rest, N, valid) & (isin if len(rest) < len(terms) else True)
        clauses = {}
        for i, x in enumerate(rest):
            clauses.setdefault(x[3] if len(x) > 3 else -1 - i, []).append(x)
        parts = [like_mask(cols, c, N, valid) for c in clauses.values()] + ([isin] if len(rest) < len(terms) else [])
        assert np.array_equal(want, np.logical_and.reduce(parts)) and 0 < want.sum() < min(p.sum() for p in parts), name
        assert count_star(t, terms) == int(want.sum()), name
        got = [first + sel for _, first, sel, _ in t.scan_filtered(terms, cols=[C_ID])]
        assert np.array_equal(np.concatenate(got), np.nonzero(want)[0]), name
        ids = [a[C_ID].view(np.int32) for _, _, _, a in t.scan_filtered(terms, cols=[C_ID])]
        assert np.array_equal(np.concatenate(ids), cols[C_ID][want]), name


@pytest.mark.gpu
def test_gpu_pushdowns_under_a_pattern_filter(fl, gpu, tab):
    img, t, cols, valid = tab
    for terms in ([PAT_A], [PAT_N, PAT_B]):
        m = like_mask(cols, terms, N, valid)
        assert 0 < m.sum() < N
        ids, g, k = cols[C_ID][m].astype(np.int64), cols[C_G][m], cols[C_K][m]
        # ungrouped
        assert t.aggregate([("count",), ("sum", C_ID), ("min", C_ID), ("max", C_K)], filt=terms) == \
            [int(m.sum()), int(ids.sum()), int(ids.min()), int(k.max())]
        # grouped on g
        got = dict((key[0], vals) for key, vals in t.aggregate_grouped([C_G], [("count",), ("sum", C_ID)], filt=terms))
        assert got == {int(x): [int((g == x).sum()), int(ids[g == x].sum())] for x in np.unique(g)}
        # hashed on k
        hg = t.aggregate_hashed([C_K], [("count",), ("sum", C_ID)], 1024, filt=terms).to_list()
        assert dict((key[0], vals) for key, vals in hg) == \
            {int(x): [int((k == x).sum()), int(ids[k == x].sum())] for x in np.unique(k)}
        # top-N: the 20 largest k, ties by row
        rows, values, _ = t.topn(C_K, 20, cols=[C_ID, C_D], filt=terms, desc=True)
        cand = np.nonzero(m)[0]
        order = cand[np.lexsort((cand, -cols[C_K][cand].astype(np.int64)))][:20]
        assert np.array_equal(rows, order.astype(np.uint64))
        assert np.array_equal(values[C_ID], cols[C_ID][order]) and values[C_D] == [cols[C_D][i] for i in order]


@pytest.mark.gpu
def test_gpu_sugar_terms(fl, gpu, tab):
    img, t, cols, valid = tab
    for op, lit, pat in [("starts_with", b"100%", b"100\\%%"), ("ends_with", b"_b", b"%\\_b"),
                         ("contains", b"\\", b"%\\\\%"), ("contains", "abc", b"%abc%")]:
        want = like_mask(cols, [(C_N, "like", (pat, b"\\"))], N, valid)
        assert 0 < want.sum()
        assert count_star(t, [(C_N, op, lit)]) == int(want.sum()), (op, lit)
    assert count_star(t, [(C_D, "like", None)]) == 0 and count_star(t, [(C_D, "not_like", None)]) == 0
