"""The pushed-down filter at string, type and row-group edges.

filter_kernel and compact_kernel (csrc/fls_filter.hip) serve every filtered
scan, both aggregate kernels and SQL WHERE; tests/test_filter.py drives them
almost only over generated lineitem with 65536-row row groups.  Here they run
on small hand-built tables (1024- and 4096-row row groups, a ragged tail):

  A. every path of the string comparison (first-4-bytes shortcut, the <= 4
     byte exits, the =/!= length shortcut, inline records of at most 12 bytes,
     pointer records) over DICT, FSST and BLOB columns and a nullable one;
  B. one VARCHAR column that is DICT in some row groups of a scan batch and
     FSST in others (ENC_AUTO chooses per chunk);
  C. integer terms at each type's range ends, and constants outside the
     column's type but inside the 64-bit comparison domain;
  D. the compaction's cross-vector prefix, row index within the row group and
     empty-word skip with more than one row group per batch and ragged batches.

Every expected value is helpers.filter_mask or plain Python comparison over
the arrays handed to write_image, never the engine's; all comparisons exact."""
import numpy as np
import pytest

from ext_harness import Ext
from helpers import check_filtered_scan, chunk_encodings, filter_mask, rg_slice

RG = 1024
OPS6 = ["=", "!=", "<", "<=", ">", ">="]
BATCHES = [None, "1", "3"]        # FLS_SCAN_BATCH: the default (8 row groups), 1, 3


def set_batch(monkeypatch, batch):
    if batch is None:
        monkeypatch.delenv("FLS_SCAN_BATCH", raising=False)
    else:
        monkeypatch.setenv("FLS_SCAN_BATCH", batch)


def count_star(t, terms):
    return t.aggregate([("count",)], filt=terms)[0]


@pytest.fixture(scope="module")
def ext(_built):
    e = Ext()
    yield e
    e.close()


# ------------------------------------------------- A. string comparison matrix
S36 = b"abcdefghijklmnopqrstuvwxyz0123456789"
S13 = b"abcdefghijklm"
STRINGS = [b"", b"a", b"ab", b"abc", b"abcd", b"abcde", b"abcd\x00", b"abcd\xff", b"abc\x80", b"abc\x7f", b"abce",
           b"abd", b"b", b"ABCD", b"abcdefghijk", b"abcdefghijkl", S13, b"abcdefghijkl\x00", b"abcdefghijkL",
           b"abcdEfghijklm", S36, S36[:35], S36 + b"\x00", S36[:35] + b":", b"\xff", b"\xff" * 5, b"\x00",
           b"\x00" * 5]
CONSTANTS = STRINGS + [S36[:26], b"abcdf", b"zzzz", S36 + b"zz"]
N_A = 2 * RG + 37
A_D, A_F, A_B, A_N, A_ID = range(5)
A_NAMES = {A_D: "d", A_F: "f", A_B: "b", A_N: "n"}


@pytest.fixture(scope="module")
def strtab(fl):
    rng = np.random.default_rng(20240601)
    vals = [STRINGS[k] for k in rng.integers(0, len(STRINGS), N_A)]
    vals[-1] = S13
    null = rng.random(N_A) < 0.2
    ids = np.arange(N_A, dtype=np.int32)
    img = fl.write_image([("d", fl.VARCHAR, vals, fl.ENC_DICT), ("f", fl.VARCHAR, vals, fl.ENC_FSST),
                          ("b", fl.BLOB, vals, fl.ENC_FSST),
                          ("n", fl.VARCHAR, [None if z else v for v, z in zip(vals, null)], fl.ENC_AUTO),
                          ("id", fl.INT32, ids, fl.ENC_FFOR)], rowgroup=RG)
    t = fl.Connection([0]).read_image(img)
    cols = {A_D: vals, A_F: vals, A_B: vals, A_N: vals, A_ID: ids}
    return img, t, cols, {A_N: ~null}


def test_string_table_reaches_the_oracle(fl, ref, strtab):
    img, t, cols, valid = strtab
    assert set(cols[A_D]) == set(STRINGS) and len(cols[A_D][-1]) == 13
    assert 0.1 < 1 - valid[A_N].mean() < 0.3
    rf = ref.RefFile(img)
    for c in (A_D, A_F, A_B):
        assert rf.strings_column(c) == cols[c], A_NAMES[c]
    assert rf.strings_column(A_N) == [v if ok else b"" for v, ok in zip(cols[A_N], valid[A_N])]
    encs = chunk_encodings(img.tobytes())
    assert [r[A_D] for r in encs] == [fl.ENC_DICT] * 3
    assert [r[A_F] for r in encs] == [fl.ENC_FSST] * 3 and [r[A_B] for r in encs] == [fl.ENC_FSST] * 3


def test_string_pruning_exact_on_dict_and_absent_on_fsst(fl, strtab):
    img, t, cols, valid = strtab
    for k in CONSTANTS:
        for op in OPS6:
            for rg in range(t.nrowgroups):
                hit = filter_mask(rg_slice(cols, rg, RG), [(A_D, op, k)], t.rowgroup_rows(rg)).any()
                assert t.may_match(rg, [(A_D, op, k)]) == hit, (k, op, rg)
                assert t.may_match(rg, [(A_F, op, k)]), (k, op, rg)


def test_string_matrix_is_not_vacuous(strtab):
    img, t, cols, valid = strtab
    kinds = set()
    for k in CONSTANTS:
        for op in OPS6:
            s = int(filter_mask(cols, [(A_D, op, k)], N_A).sum())
            kinds.add("none" if s == 0 else "all" if s == N_A else "part")
    assert kinds == {"none", "all", "part"}


@pytest.mark.gpu
@pytest.mark.parametrize("col", [A_D, A_F, A_B, A_N], ids=lambda c: A_NAMES[c])
def test_gpu_string_matrix_scan(fl, gpu, strtab, col):
    img, t, cols, valid = strtab
    for k in CONSTANTS:
        for op in OPS6:
            try:
                check_filtered_scan(fl, t, cols, [(col, op, k)], [col, A_ID], rowgroup=RG, valid=valid)
            except AssertionError as e:
                raise AssertionError(f"{A_NAMES[col]} {op} {k!r}: {e}") from e


@pytest.mark.gpu
@pytest.mark.parametrize("col", [A_D, A_F, A_B, A_N], ids=lambda c: A_NAMES[c])
def test_gpu_string_matrix_count(fl, gpu, strtab, col):
    # the aggregate kernel's mask path over the same terms
    img, t, cols, valid = strtab
    for k in CONSTANTS:
        for op in OPS6:
            terms = [(col, op, k)]
            assert count_star(t, terms) == int(filter_mask(cols, terms, N_A, valid).sum()), (A_NAMES[col], op, k)


@pytest.mark.gpu
def test_gpu_string_nulls(fl, gpu, strtab):
    img, t, cols, valid = strtab
    ok = valid[A_N]
    empty = np.array([v == b"" for v in cols[A_N]])
    for terms, want in [([(A_N, "is_null", None)], ~ok), ([(A_N, "is_not_null", None)], ok),
                        ([(A_N, "!=", b"zzzz")], ok), ([(A_N, ">=", b"")], ok), ([(A_N, "=", b"")], ok & empty)]:
        assert np.array_equal(filter_mask(cols, terms, N_A, valid), want), terms   # the expectation itself
        total = check_filtered_scan(fl, t, cols, terms, [A_N, A_ID], rowgroup=RG, valid=valid)
        assert total == int(want.sum()) == count_star(t, terms), terms
    # is_null OR a comparison, in one clause
    terms = [(A_N, "is_null", None, 1), (A_N, "<", b"abcd", 1)]
    total = check_filtered_scan(fl, t, cols, terms, [A_ID], rowgroup=RG, valid=valid)
    assert total == int((~ok | (ok & np.array([v < b"abcd" for v in cols[A_N]]))).sum())


@pytest.mark.gpu
def test_gpu_string_or_clauses_across_encodings(fl, gpu, strtab):
    img, t, cols, valid = strtab
    c1 = [(A_D, "=", b"abcd", 1), (A_F, ">", S13, 1)]
    c2 = [(A_D, "<", b"abcd", 2), (A_F, ">=", S36, 2)]
    want = [int(filter_mask(cols, terms, N_A).sum()) for terms in (c1, c2, c1 + c2)]
    assert 0 < want[2] < min(want[:2]) and max(want[:2]) < N_A      # the conjunction narrows both clauses
    for terms, n in zip((c1, c2, c1 + c2), want):
        assert check_filtered_scan(fl, t, cols, terms, [A_D, A_F, A_ID], rowgroup=RG) == n == count_star(t, terms)


# ------------------------------------- B. one column, both encodings, one batch
WORDS5 = [b"DELIVER IN PERSON", b"TAKE BACK RETURN", b"COLLECT COD", b"NONE", b"take back returnz"]
N_B = 3 * RG + 37
B_TERMS = [(">=", b"TAKE BACK"), ("=", b"TAKE BACK RETURN"), ("!=", b"DELIVER IN PERSON"),
           ("<", b"TAKE BACK 001500"), (">", b"COLLECT COD")]


def mixed_rows():
    rng = np.random.default_rng(77)
    s = [WORDS5[k] for k in rng.integers(0, len(WORDS5), N_B)]
    for i in range(RG, 2 * RG):
        s[i] = b"TAKE BACK %06d unique text row" % i
    return s, np.arange(N_B, dtype=np.int32)


def mixed_image(fl):
    s, ids = mixed_rows()
    return fl.write_image([("s", fl.VARCHAR, s, fl.ENC_AUTO), ("id", fl.INT32, ids, fl.ENC_FFOR)], rowgroup=RG)


@pytest.fixture(scope="module")
def mixed(fl):
    s, ids = mixed_rows()
    img = mixed_image(fl)
    return img, fl.Connection([0]).read_image(img), {0: s, 1: ids}


def test_mixed_column_chunk_encodings(fl, ref, mixed):
    img, t, cols = mixed
    assert [r[0] for r in chunk_encodings(img.tobytes())] == [fl.ENC_DICT, fl.ENC_FSST, fl.ENC_DICT, fl.ENC_FSST]
    assert ref.RefFile(img).strings_column(0) == cols[0]
    # the terms below split the rows: neither nothing nor everything
    for op, k in B_TERMS:
        assert 0 < filter_mask(cols, [(0, op, k)], N_B).sum() < N_B, (op, k)


def test_mixed_column_refused_as_group_key(fl, mixed):
    img, t, cols = mixed
    with pytest.raises(fl.FlsError, match="not dictionary-encoded in row group 1"):
        t.aggregate_grouped([0], [("count",)])


@pytest.mark.gpu
def test_gpu_mixed_column_refused_as_group_key(fl, gpu, mixed):
    img, t, cols = mixed
    with pytest.raises(fl.FlsError, match="not dictionary-encoded in row group 1"):
        t.aggregate_grouped([0], [("count",)])
    with pytest.raises(fl.FlsError, match="not dictionary-encoded in row group 1"):
        t.aggregate_grouped([0], [("count",)], filt=[(1, ">=", RG)])


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES)
def test_gpu_mixed_column_unfiltered_scan(fl, gpu, mixed, monkeypatch, batch):
    set_batch(monkeypatch, batch)
    img, t, cols = mixed
    got, ids = [], []
    for first_row, arrays in t.scan():
        assert first_row == len(got)
        got += fl.string_t_decode(arrays[0])
        ids.append(arrays[1].view(np.int32))
    assert got == cols[0] and np.array_equal(np.concatenate(ids), cols[1])


@pytest.mark.gpu
@pytest.mark.parametrize("batch,devices", [(None, [0]), ("1", [0]), ("3", [0]), (None, [0, 0])],
                         ids=["default", "batch1", "batch3", "two_devices"])
def test_gpu_mixed_column_filtered_scan(fl, gpu, mixed, monkeypatch, batch, devices):
    """Default batch: the four chunks (DICT, FSST, DICT, FSST) share one batch,
    so a term's long-string pointers come from the file image and from the
    batch heap at once.  Batch 1 is the control: one encoding per batch."""
    set_batch(monkeypatch, batch)
    img, t, cols = mixed
    if devices != [0]:
        t = fl.Connection(devices).read_image(img)
    for op, k in B_TERMS:
        terms = [(0, op, k)]
        total = check_filtered_scan(fl, t, cols, terms, [0, 1], rowgroup=RG)
        assert total == int(filter_mask(cols, terms, N_B).sum()), (op, k)
        assert count_star(t, terms) == total, (op, k)


@pytest.mark.gpu
def test_gpu_mixed_column_read_fastlanes_where(fl, gpu, ext, mixed, tmpfile):
    img, t, cols = mixed
    p = tmpfile("mixed.fls")
    img.write(p)
    for where, keep in [("= TAKE BACK RETURN", {b"TAKE BACK RETURN"}),
                        ("IN TAKE BACK RETURN|NONE|TAKE BACK 001500 unique text row|take back returnz",
                         {b"TAKE BACK RETURN", b"NONE", b"TAKE BACK 001500 unique text row", b"take back returnz"})]:
        names, types, rows = ext.query("read_fastlanes", p, proj=[0, 1], where=[(0, where)])
        assert names == ["s", "id"]
        assert rows == [[s.decode(), str(i)] for i, s in enumerate(cols[0]) if s in keep], where
        assert any(r[0].startswith("TAKE BACK 0") for r in rows) == (len(keep) > 1)


# ------------------------------------------------ C. integer terms at type edges
INT_TYPES = ["INT8", "INT16", "INT32", "INT64", "UINT8", "UINT16", "UINT32", "UINT64", "DATE", "DECIMAL"]
N_C = 2 * RG + 37
PLANT_ROWS = [0, 63, 64, 1023, 1024, N_C - 1]


def int_edges(fl, tn):
    """(numpy dtype, its min and max, constants inside the type, constants
    outside it that the 64-bit comparison domain still holds)"""
    dt = np.dtype(fl.NP_DTYPE[getattr(fl, tn)])
    lo, hi = int(np.iinfo(dt).min), int(np.iinfo(dt).max)
    inside = {lo, lo + 1, 0, 1, hi - 1, hi} | ({-1} if lo < 0 else set())
    outside = []
    if dt.itemsize < 8:
        outside = ([lo - 1] if lo < 0 else []) + [hi + 1]
    return dt, lo, hi, sorted(inside), outside


@pytest.fixture(scope="module")
def inttab(fl):
    rng = np.random.default_rng(4242)
    spec, cols = [], {}
    for c, tn in enumerate(INT_TYPES):
        dt, lo, hi, _, _ = int_edges(fl, tn)
        v = rng.integers(lo, hi, N_C, dtype=dt, endpoint=True)
        plant = [lo, hi, 0] + ([-1] if lo < 0 else [])
        for j, r in enumerate(PLANT_ROWS):
            v[r] = plant[j % len(plant)]
        cols[c] = v
        spec.append((tn.lower(), getattr(fl, tn), v, fl.ENC_AUTO) + ((18, 2) if tn == "DECIMAL" else ()))
    img = fl.write_image(spec, rowgroup=RG)
    return img, fl.Connection([0]).read_image(img), cols


def test_int_table_reaches_the_oracle_and_zone_maps(fl, ref, inttab):
    img, t, cols = inttab
    rf = ref.RefFile(img)
    for c, tn in enumerate(INT_TYPES):
        dt = cols[c].dtype
        assert np.array_equal(rf.decode_column(c, nthreads=2).view(dt), cols[c]), tn
        for rg in range(t.nrowgroups):
            part = cols[c][rg * RG:(rg + 1) * RG]
            assert t.zonemap(rg, c)[:2] == (int(part.min()), int(part.max())), (tn, rg)


@pytest.mark.parametrize("c", range(len(INT_TYPES)), ids=INT_TYPES)
def test_int_pruning_conservative_and_total_outside_the_type(fl, inttab, c):
    img, t, cols = inttab
    dt, lo, hi, inside, outside = int_edges(fl, INT_TYPES[c])
    for k in inside + outside:
        for op in OPS6:
            m = filter_mask(cols, [(c, op, k)], N_C)
            for rg in range(t.nrowgroups):
                if not t.may_match(rg, [(c, op, k)]):
                    assert not m[rg * RG:(rg + 1) * RG].any(), (k, op, rg)
            if k in outside and not m.any():
                # below the type's minimum or above its maximum: no zone map can admit it
                assert not any(t.may_match(rg, [(c, op, k)]) for rg in range(t.nrowgroups)), (k, op)
    for k in outside:
        nothing = ["=", "<", "<="] if k < lo else ["=", ">", ">="]
        for op in OPS6:
            m = filter_mask(cols, [(c, op, k)], N_C)
            assert (not m.any()) if op in nothing else m.all(), (k, op)


@pytest.mark.gpu
@pytest.mark.parametrize("c", range(len(INT_TYPES)), ids=INT_TYPES)
def test_gpu_int_terms_at_type_edges(fl, gpu, inttab, c):
    img, t, cols = inttab
    dt, lo, hi, inside, outside = int_edges(fl, INT_TYPES[c])
    for k in inside + outside:
        for op in OPS6:
            terms = [(c, op, k)]
            want = int(filter_mask(cols, terms, N_C).sum())
            try:
                total = check_filtered_scan(fl, t, cols, terms, [c], rowgroup=RG)
            except AssertionError as e:
                raise AssertionError(f"{INT_TYPES[c]} {op} {k}: {e}") from e
            assert total == want, (k, op)
            if k in outside and want == 0:
                assert t.pruned == t.nrowgroups, (k, op)
            assert count_star(t, terms) == want, (k, op)


# -------------------------------------- D. compaction geometry, small row groups
D_I8, D_I16, D_I32, D_I64, D_S, D_ID, D_M2, D_M64, D_M1024, D_RND = range(10)
D_DELIVER = [D_I8, D_I16, D_I32, D_I64, D_S]
D_WORDS = [b"abc", b"abcdefghijkl", b"abcdefghijklmnopqrst"]     # 3, 12 and 20 bytes


def geometry_table(fl, rowgroup):
    n = 11 * rowgroup + 37
    rng = np.random.default_rng(rowgroup)
    ids = np.arange(n, dtype=np.int32)
    cols = {D_I8: rng.integers(-128, 127, n, dtype=np.int8, endpoint=True),
            D_I16: rng.integers(-2**15, 2**15 - 1, n, dtype=np.int16, endpoint=True),
            D_I32: rng.integers(-2**31, 2**31 - 1, n, dtype=np.int32, endpoint=True),
            D_I64: rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True),
            D_S: [D_WORDS[k] for k in rng.integers(0, 3, n)],
            D_ID: ids, D_M2: (ids % 2).astype(np.int32), D_M64: (ids % 64).astype(np.int32),
            D_M1024: (ids % 1024).astype(np.int32), D_RND: rng.integers(0, 256, n).astype(np.uint8)}
    ty = {D_I8: fl.INT8, D_I16: fl.INT16, D_I32: fl.INT32, D_I64: fl.INT64, D_S: fl.VARCHAR, D_RND: fl.UINT8}
    img = fl.write_image([(f"c{c}", ty.get(c, fl.INT32), cols[c], fl.ENC_DICT if c == D_S else fl.ENC_AUTO)
                          for c in range(10)], rowgroup=rowgroup)
    return n, fl.Connection([0]).read_image(img), cols


@pytest.fixture(scope="module")
def geometry(fl):
    made = {}

    def get(rowgroup):
        if rowgroup not in made:
            made[rowgroup] = geometry_table(fl, rowgroup)
        return made[rowgroup]
    return get


def selections(n, rowgroup):
    return {
        "nothing_unpruned": [(D_M2, "=", 1), (D_M2, "=", 0)],
        "everything": [(D_ID, ">=", 0)],
        "last_row": [(D_ID, "=", n - 1)],
        "first_of_vector": [(D_M1024, "=", 0)],
        "rows_63_64_of_vector": [(D_M1024, "=", 63, 1), (D_M1024, "=", 64, 1)],
        "rowgroup_5": [(D_ID, ">=", 5 * rowgroup), (D_ID, "<", 6 * rowgroup)],
        "alternating": [(D_M2, "=", 1)],
        "random_half": [(D_RND, "<", 128)],
    }


SELECTIONS = sorted(selections(0, 0))


@pytest.mark.parametrize("rowgroup", [1024, 4096])
def test_geometry_selections_are_what_they_claim(fl, geometry, rowgroup):
    n, t, cols = geometry(rowgroup)
    assert t.nrowgroups == 12 and t.rowgroup_rows(11) == 37
    sel = {k: filter_mask(cols, v, n) for k, v in selections(n, rowgroup).items()}
    ids = cols[D_ID]
    assert not sel["nothing_unpruned"].any() and sel["everything"].all()
    assert all(t.may_match(rg, selections(n, rowgroup)["nothing_unpruned"]) for rg in range(12))
    assert np.array_equal(np.nonzero(sel["last_row"])[0], [n - 1])
    assert np.array_equal(ids[sel["first_of_vector"]], np.arange(0, n, 1024))
    assert np.array_equal(ids[sel["rows_63_64_of_vector"]] % 1024, [63, 64] * (11 * rowgroup // 1024))
    assert np.array_equal(ids[sel["rowgroup_5"]], np.arange(5 * rowgroup, 6 * rowgroup))
    assert np.array_equal(ids[sel["alternating"]], np.arange(1, n, 2))
    assert 0.45 < sel["random_half"].mean() < 0.55


@pytest.mark.gpu
@pytest.mark.parametrize("name", SELECTIONS)
@pytest.mark.parametrize("rowgroup", [1024, 4096])
def test_gpu_compaction_geometry(fl, gpu, geometry, monkeypatch, rowgroup, name):
    n, t, cols = geometry(rowgroup)
    terms = selections(n, rowgroup)[name]
    want = filter_mask(cols, terms, n)
    runs = []
    for batch in BATCHES:
        set_batch(monkeypatch, batch)
        total = check_filtered_scan(fl, t, cols, terms, D_DELIVER, rowgroup=rowgroup)
        assert total == int(want.sum()), batch
        out = []
        for rg, first_row, sel, arrays in t.scan_filtered(terms, cols=D_DELIVER):
            assert first_row == rg * rowgroup, (batch, rg)
            assert len(sel) == 0 or int(sel.max()) < t.rowgroup_rows(rg), (batch, rg)
            if not want[rg * rowgroup:(rg + 1) * rowgroup].any():
                assert len(sel) == 0 and sel.dtype == np.uint32, (batch, rg)   # survived the pruning, selects nothing
            out.append((rg, sel.tobytes(), fl.string_t_decode(arrays[D_S]),
                        [arrays[c].tobytes() for c in D_DELIVER if c != D_S]))
        runs.append(out)
    assert runs[0] == runs[1] == runs[2]
    if name == "nothing_unpruned":
        assert [r[0] for r in runs[0]] == list(range(12)) and t.pruned == 0
    set_batch(monkeypatch, None)
    assert count_star(t, terms) == int(want.sum())


def _scan(t, narrow, filt):
    """every column of the filtered scan, narrowed delivery on or off"""
    t.set_filter(filt)
    t.narrow(narrow)
    out = None
    for first, arrays in t.scan():
        if out is None:
            out = [[] for _ in arrays]
        for c, a in enumerate(arrays):
            out[c].append(a)
    t.narrow(False)
    t.set_filter([])
    return [np.concatenate(x) if x else np.zeros(0, np.uint8) for x in out]


@pytest.mark.gpu
@pytest.mark.parametrize("rowgroup", [1024, 4096])
def test_gpu_geometry_narrowed_delivery_matches_full_width(fl, gpu, geometry, rowgroup):
    n, t, cols = geometry(rowgroup)
    terms = selections(n, rowgroup)["alternating"]
    want = np.nonzero(filter_mask(cols, terms, n))[0]
    full = _scan(t, False, terms)
    nar = _scan(t, True, terms)
    for c in range(10):
        if c == D_S:
            continue                     # string_t records hold pointers: compared by content above
        assert np.array_equal(full[c], nar[c]), c
        assert np.array_equal(full[c].view(cols[c].dtype), cols[c][want]), c
