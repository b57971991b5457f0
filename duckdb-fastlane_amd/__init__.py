"""duckdb-fastlane_amd -- MI355X FastLanes scan path, Python binding.

Thin ctypes view of the C-ABI in include/flsgpu.h and include/flswriter.h
(libflsgpu.so, built in-tree by `make -C duckdb-fastlane_amd`).  It exists for
tests and bench.py; the product boundary is the C-ABI itself, consumed by the
C++ DuckDB glue in extension/.  There is no CPU fallback: if the shared library
is missing, importing this package raises.

Load with pkgload.load() (the directory name has a hyphen).
"""
from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
# FLS_LIB selects an alternative in-tree build (A/B measurement of kernel variants)
LIB_PATH = _HERE / os.environ.get("FLS_LIB", "libflsgpu.so")

if not LIB_PATH.exists():
    raise ImportError(f"{LIB_PATH} not built: run `make -C {_HERE}` (hipcc --offload-arch=gfx950)")

_lib = C.CDLL(str(LIB_PATH))

# --- enums (include/flswriter.h) -------------------------------------------
INT8, INT16, INT32, INT64, UINT8, UINT16, UINT32, UINT64 = 1, 2, 3, 4, 5, 6, 7, 8
BOOLEAN, DATE, DECIMAL, FLOAT, DOUBLE, VARCHAR, BLOB = 9, 10, 11, 12, 13, 20, 21
STRING_TYPES = (VARCHAR, BLOB)
ENC_AUTO, ENC_FFOR, ENC_DELTA, ENC_DICT, ENC_RLE, ENC_ALP, ENC_FSST = 0, 1, 2, 3, 4, 5, 7

NP_DTYPE = {INT8: np.int8, INT16: np.int16, INT32: np.int32, INT64: np.int64,
            UINT8: np.uint8, UINT16: np.uint16, UINT32: np.uint32, UINT64: np.uint64,
            BOOLEAN: np.uint8, DATE: np.int32, DECIMAL: np.int64, FLOAT: np.float32, DOUBLE: np.float64}
TYPE_NAMES = {INT8: "TINYINT", INT16: "SMALLINT", INT32: "INTEGER", INT64: "BIGINT",
              UINT8: "UTINYINT", UINT16: "USMALLINT", UINT32: "UINTEGER", UINT64: "UBIGINT",
              DATE: "DATE", DECIMAL: "DECIMAL", FLOAT: "FLOAT", DOUBLE: "DOUBLE", VARCHAR: "VARCHAR",
              BOOLEAN: "BOOLEAN", BLOB: "BLOB"}
ROWGROUP = 65536


class FlsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[{code}] {msg}")
        self.code = code
        self.msg = msg


class ColumnInfo(C.Structure):
    _fields_ = [("name", C.c_char_p), ("type", C.c_uint8), ("width", C.c_uint8),
                ("scale", C.c_uint8), ("out_bytes", C.c_uint8)]


class RowGroup(C.Structure):
    _fields_ = [("rowgroup", C.c_uint32), ("nrows", C.c_uint32), ("first_row", C.c_uint64),
                ("ncols", C.c_uint32), ("columns", C.POINTER(C.c_void_p)),
                ("nrows_scanned", C.c_uint32), ("sel", C.POINTER(C.c_uint32)),
                ("validity", C.POINTER(C.c_void_p)), ("dict", C.POINTER(C.c_void_p)),
                ("dict_size", C.POINTER(C.c_uint32)), ("dict_width", C.POINTER(C.c_uint8)),
                ("narrow", C.POINTER(C.c_uint8)), ("narrow_base", C.POINTER(C.c_uint64))]


class Predicate(C.Structure):
    _fields_ = [("col", C.c_uint32), ("clause", C.c_uint32), ("op", C.c_uint8), ("pad", C.c_uint8 * 3),
                ("key_col", C.c_uint32),   # MAP_EQ .. MAP_GE: the key column (the tail of what was pad[7])
                ("value", C.c_uint64), ("str", C.c_char_p), ("str_len", C.c_uint64)]


# fls_cmp (include/flsgpu.h)
EQ, NE, LT, LE, GT, GE, IS_NULL, IS_NOT_NULL = range(8)
OPS = {"=": EQ, "==": EQ, "!=": NE, "<>": NE, "<": LT, "<=": LE, ">": GT, ">=": GE,
       "is_null": IS_NULL, "is_not_null": IS_NOT_NULL, "false": 8,
       "in_set": 9, "not_in_set": 10, "like": 11, "not_like": 12,
       "col=": 13, "col!=": 14, "col<": 15, "col<=": 16, "col>": 17, "col>=": 18,
       "map=": 19, "map!=": 20, "map<": 21, "map<=": 22, "map>": 23, "map>=": 24}
IN_SET, NOT_IN_SET = 9, 10
LIKE, NOT_LIKE = 11, 12
MAX_PATTERN_TERMS, MAX_PATTERN_TOKENS = 8, 256   # kMaxPatTerms, kMaxPatTokens
COL_EQ, COL_NE, COL_LT, COL_LE, COL_GT, COL_GE = range(13, 19)
MAP_EQ, MAP_NE, MAP_LT, MAP_LE, MAP_GT, MAP_GE = range(19, 25)
MAX_MAP_TERMS = 8                  # kMaxMapTerms


class Col:
    """the right-hand side of a column-to-column filter term: (a, "<", Col(b))
    holds for the rows where both columns are valid and a < b"""

    def __init__(self, index: int):
        self.index = int(index)

    def __repr__(self):
        return f"Col({self.index})"

    def __eq__(self, other):
        return isinstance(other, Col) and other.index == self.index

    def __hash__(self):
        return hash(("Col", self.index))


class Mapped:
    """the right-hand side of a map filter term: (a, "<", Mapped(key_col, vm))
    holds for the rows where column a and column key_col are valid, the key is
    in the ValueMap vm and a < vm[key]; a NULL on either side or an absent
    key satisfies no operator, "!=" included.

    A Mapped is also a column of its own, vm[key_col] (a 64-bit integer, NULL
    where the key is NULL or absent), wherever an aggregate tuple takes a
    column index -- ("sum", M), ("count", M), ("min" | "max", M),
    ("sum_product", a, M), a sum_expr factor (k, sign, M), the same inside
    When -- and as an element of aggregate_hashed's keys.  There it is an
    inner join by default (a selected row without a mapped value leaves the
    call's selection, count(*) included); keep_unmatched=True makes it a left
    join: the row stays, operands skip it and as a key it forms the NULL
    group.  In a filter term keep_unmatched=True is a ValueError: a NULL
    satisfies no operator there already."""

    def __init__(self, key_col: int, valuemap, keep_unmatched: bool = False):
        self.key_col = int(key_col)
        self.valuemap = valuemap
        self.keep_unmatched = bool(keep_unmatched)

    def _ident(self):
        vm = self.valuemap
        return (self.key_col, vm.h if isinstance(vm, ValueMap) else vm, id(vm), self.keep_unmatched)

    def __eq__(self, other):
        return isinstance(other, Mapped) and other._ident() == self._ident()

    def __hash__(self):
        return hash(("Mapped",) + self._ident())

    def __repr__(self):
        keep = ", keep_unmatched=True" if self.keep_unmatched else ""
        return f"Mapped({self.key_col}, {self.valuemap!r}{keep})"


def _pat_bytes(x, what):
    if isinstance(x, str):
        return x.encode()
    if isinstance(x, (bytes, bytearray, memoryview)):
        return bytes(x)
    raise TypeError(f"{what}: str or bytes expected, got {type(x).__name__}")


def like_escape(literal, escape=b"\\") -> bytes:
    """literal with `%`, `_` and the escape byte escaped: a LIKE pattern (under
    ESCAPE escape) that matches exactly the literal's bytes"""
    lit, e = _pat_bytes(literal, "like_escape"), _pat_bytes(escape, "like_escape")
    return b"".join(e + bytes([b]) if b in (0x25, 0x5F, e[0]) else bytes([b]) for b in lit)


# (col, sugar, literal) -> the LIKE pattern around the escaped literal, ESCAPE '\'
_LIKE_SUGAR = {"starts_with": (b"", b"%"), "ends_with": (b"%", b""), "contains": (b"%", b"%")}
# fls_keyset_form
KEYSET_AUTO, KEYSET_BITMAP, KEYSET_HASH = 0, 1, 2
MAX_KEYSET_KEYS = 1 << 28          # kMaxKeysetKeys
KEYSET_HASH_MUL = 0x9E3779B97F4A7C15


class KeySetInfo(C.Structure):     # fls_keyset_info_t
    _fields_ = [("count", C.c_uint64), ("form", C.c_uint32), ("kind", C.c_uint32), ("device_bytes", C.c_uint64),
                ("capacity", C.c_uint64), ("max_probe", C.c_uint32), ("pad", C.c_uint32), ("min", C.c_uint64),
                ("max", C.c_uint64), ("empty", C.c_uint64)]


class KeySetBuildInfo(C.Structure):     # fls_keyset_build_info_t
    _fields_ = [("rows_selected", C.c_uint64), ("bitmap_bytes", C.c_uint64), ("d2h_bytes", C.c_uint64),
                ("base", C.c_uint64), ("span", C.c_uint64), ("rowgroups_read", C.c_uint32),
                ("rowgroups_pruned", C.c_uint32)]


# fls_keymap_form, FLS_KEY_MAPPED, FLS_KEYMAP_KEEP_UNMATCHED
KEYMAP_AUTO, KEYMAP_DENSE, KEYMAP_HASH = 0, 1, 2
KEYMAP_ABSENT = 0xFFFF             # kKeymapAbsent: no code
KEYMAP_MAX_SPAN = 1 << 31          # kKeymapMaxSpan
KEY_MAPPED = 0x80000000
KEYMAP_KEEP_UNMATCHED = 1


class KeyMapInfo(C.Structure):     # fls_keymap_info_t
    _fields_ = [("count", C.c_uint64), ("form", C.c_uint32), ("kind", C.c_uint32), ("device_bytes", C.c_uint64),
                ("capacity", C.c_uint64), ("max_probe", C.c_uint32), ("max_code", C.c_uint32), ("min", C.c_uint64),
                ("max", C.c_uint64), ("empty", C.c_uint64)]


# fls_valuemap_form
VALUEMAP_AUTO, VALUEMAP_DENSE, VALUEMAP_HASH = 0, 1, 2
KIND_SIGNED, KIND_UNSIGNED = 0, 1  # fls_keyset_kind: a map's key_kind / value_kind
VALUEMAP_MAX_SPAN = 1 << 28        # kValuemapMaxSpan
VALUEMAP_SMALL_DENSE = 1 << 20     # kValuemapSmallDense (bytes)


class ValueMapInfo(C.Structure):   # fls_valuemap_info_t
    _fields_ = [("count", C.c_uint64), ("form", C.c_uint32), ("key_kind", C.c_uint32), ("value_kind", C.c_uint32),
                ("max_probe", C.c_uint32), ("device_bytes", C.c_uint64), ("capacity", C.c_uint64),
                ("key_min", C.c_uint64), ("key_max", C.c_uint64), ("value_min", C.c_uint64),
                ("value_max", C.c_uint64), ("empty", C.c_uint64)]


class MapBuildInfo(C.Structure):   # fls_map_build_info_t
    _fields_ = [("rows_selected", C.c_uint64), ("keys", C.c_uint64), ("scratch_bytes", C.c_uint64),
                ("d2h_bytes", C.c_uint64), ("base", C.c_uint64), ("span", C.c_uint64),
                ("rowgroups_read", C.c_uint32), ("rowgroups_pruned", C.c_uint32)]


class KeyBinding(C.Structure):     # fls_key_binding
    _fields_ = [("col", C.c_uint32), ("flags", C.c_uint32), ("map", C.c_uint64)]


# FLS_COL_MAPPED, FLS_VALUEMAP_KEEP_UNMATCHED
COL_MAPPED = 0x40000000
VALUEMAP_KEEP_UNMATCHED = 1
MAX_VALUE_BINDINGS = 4             # kMaxValueBindings


class ValueBinding(C.Structure):   # fls_value_binding
    _fields_ = [("col", C.c_uint32), ("flags", C.c_uint32), ("map", C.c_uint64)]


# fls_agg_fn / fls_aggregate_spec / fls_aggregate_value (include/flsgpu.h)
AGG_FNS = {"count_star": 0, "count": 1, "sum": 2, "min": 3, "max": 4, "sum_product": 5, "sum_expr": 6}
AGGV_NULL, AGGV_INT, AGGV_DOUBLE = 0, 1, 2


class AggregateSpec(C.Structure):
    _fields_ = [("fn", C.c_uint8), ("pad", C.c_uint8 * 3), ("col", C.c_uint32), ("col2", C.c_uint32),
                ("cond", C.c_uint32)]   # 0: none, i: condition i - 1 (fls_aggregate_conditions)


class AggCondition(C.Structure):   # fls_agg_condition: preds[first .. first + n)
    _fields_ = [("first", C.c_uint32), ("n", C.c_uint32)]


MAX_AGG_CONDITIONS = 8             # kMaxConds


class FilterAlternative(C.Structure):   # fls_filter_alternative: preds[first .. first + n)
    _fields_ = [("first", C.c_uint32), ("n", C.c_uint32)]


MAX_FILTER_ALTERNATIVES = 8        # kMaxConds


class AnyOf:
    """(filt_1 OR filt_2 OR ...) as one element of a filter: each argument a
    filter list as scan_filtered takes it (its terms AND-ed, clause numbers
    its own), the element true on a row where at least one of them is; a row
    counts once however many are.  At most one AnyOf per filter, of 1 to 8
    alternatives, none of them holding an AnyOf itself:

        filt = [(SHIPMODE, "=", "AIR"),
                fl.AnyOf([(PARTKEY, "in_set", s1), (QTY, ">=", 1), (QTY, "<=", 11)],
                         [(PARTKEY, "in_set", s2), (QTY, ">=", 10), (QTY, "<=", 20)])]

    Accepted wherever a method takes filt (fls_scan_filter_alternatives); not
    in When's condition nor in Table.may_match."""

    def __init__(self, *alternatives):
        self.alternatives = [list(a) for a in alternatives]

    def __repr__(self):
        return "AnyOf(" + ", ".join(repr(a) for a in self.alternatives) + ")"


def _split_filter(filt):
    """(base terms, alternatives or None) of a filter that may hold one AnyOf"""
    filt = list(filt or [])
    groups = [t for t in filt if isinstance(t, AnyOf)]
    if not groups:
        return filt, None
    if len(groups) > 1:
        raise ValueError(f"filter: {len(groups)} AnyOf elements (at most one per filter)")
    alts = groups[0].alternatives
    if not alts:
        raise ValueError("filter: an empty AnyOf (it takes at least one alternative)")
    for i, a in enumerate(alts):
        if not a:
            raise ValueError(f"filter: alternative {i} of the AnyOf is empty")
        if any(isinstance(t, AnyOf) for t in a):
            raise ValueError(f"filter: alternative {i} of the AnyOf holds an AnyOf (they do not nest)")
    return [t for t in filt if not isinstance(t, AnyOf)], alts


class When:
    """agg FILTER (WHERE filt): any aggregate tuple of aggregate() under a
    condition of its own, filt as scan_filtered takes it.  The aggregate
    counts a row when the call's filter selects it, filt holds there and its
    operands are valid there; filt prunes nothing and makes or removes no
    group.  Accepted anywhere in the aggs of aggregate(), aggregate_grouped()
    and aggregate_hashed()."""

    def __init__(self, agg, filt):
        if any(isinstance(term, AnyOf) for term in filt):
            raise ValueError("When: a condition holds no AnyOf")
        self.agg = tuple(agg)
        self.filt = [tuple(term) for term in filt]

    def __repr__(self):
        return f"When({self.agg!r}, {self.filt!r})"


class AggFactor(C.Structure):   # fls_agg_factor: k + sign * column
    _fields_ = [("col", C.c_uint32), ("sign", C.c_int8), ("pad", C.c_uint8 * 3), ("k", C.c_int64)]


class AggExpr(C.Structure):     # fls_agg_expr: the product of 1 to 3 factors
    _fields_ = [("nfactors", C.c_uint32), ("pad", C.c_uint32), ("f", AggFactor * 3)]


class AggregateValue(C.Structure):
    _fields_ = [("count", C.c_uint64), ("lo", C.c_uint64), ("hi", C.c_uint64), ("kind", C.c_uint8),
                ("pad", C.c_uint8 * 7)]


# fls_key_kind / fls_group_key (include/flsgpu.h)
KEYV_NULL, KEYV_INT, KEYV_STRING = 0, 1, 2
ERR_ARG, ERR_LIMIT = -3, -8


class GroupKey(C.Structure):
    _fields_ = [("kind", C.c_uint8), ("pad", C.c_uint8 * 7), ("lo", C.c_uint64), ("hi", C.c_uint64),
                ("str", C.c_void_p), ("str_len", C.c_uint64)]


class OrderKey(C.Structure):     # fls_order_key
    _fields_ = [("col", C.c_uint32), ("desc", C.c_uint8), ("nulls_first", C.c_uint8), ("pad", C.c_uint8 * 2)]


MAX_TOPN = 1024


class GroupHaving(C.Structure):  # fls_group_having: aggregate[agg] <op> constant
    _fields_ = [("agg", C.c_uint32), ("op", C.c_uint8), ("kind", C.c_uint8), ("pad", C.c_uint8 * 2),
                ("lo", C.c_uint64), ("hi", C.c_uint64)]


class GroupSelect(C.Structure):  # fls_group_select
    _fields_ = [("having", C.POINTER(GroupHaving)), ("nhaving", C.c_uint32), ("order_agg", C.c_uint32),
                ("desc", C.c_uint8), ("nulls_first", C.c_uint8), ("pad", C.c_uint8 * 2), ("limit", C.c_uint32)]


GROUP_ORDER_NONE = 0xFFFFFFFF     # FLS_GROUP_ORDER_NONE
MAX_GROUP_LIMIT = 1024            # kMaxGroupLimit
MAX_HAVING = 8                    # kMaxHaving


class DecodeStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("values", C.c_uint64), ("packed_bytes", C.c_uint64),
                ("meta_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("launches", C.c_uint32),
                ("timed_launches", C.c_uint32), ("kernel_ms_total", C.c_double)]

    @property
    def algo_bytes(self) -> int:
        return int(self.packed_bytes + self.meta_bytes + self.out_bytes)


class PartInfo(C.Structure):
    _fields_ = [("device", C.c_int), ("rg_begin", C.c_uint32), ("rg_end", C.c_uint32), ("first_row", C.c_uint64),
                ("nrows", C.c_uint64)]


def _sig(name, res, *args):
    f = getattr(_lib, name)
    f.restype = res
    f.argtypes = list(args)
    return f


_P = C.c_void_p
_sig("fls_last_error", C.c_char_p)
_sig("fls_version", C.c_char_p)
_sig("fls_config_default", C.c_int, C.c_char_p, C.POINTER(C.c_int64))
_sig("fls_config_value", C.c_int, C.c_char_p, C.POINTER(C.c_int64))
_sig("fls_config_count", C.c_int)
_sig("fls_config_name", C.c_char_p, C.c_int)
_sig("fls_device_count", C.c_int)
_sig("fls_connect", C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(_P))
_sig("fls_disconnect", None, _P)
_sig("fls_connection_trim", C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64))
_sig("fls_release_device_memory", C.c_int, C.c_int, C.POINTER(C.c_uint64))
_sig("fls_resident_info", C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32))
_sig("fls_read_fls", C.c_int, _P, C.c_char_p, C.POINTER(_P))
_sig("fls_read_fls_image", C.c_int, _P, _P, C.c_uint64, C.c_int, C.POINTER(_P))
_sig("fls_table_close", None, _P)
_sig("fls_table_ncols", C.c_uint32, _P)
_sig("fls_table_nrows", C.c_uint64, _P)
_sig("fls_table_row_offset", C.c_uint64, _P)
_sig("fls_table_nrowgroups", C.c_uint32, _P)
_sig("fls_table_rowgroup_rows", C.c_int64, _P, C.c_uint32)
_sig("fls_table_column", C.c_int, _P, C.c_uint32, C.POINTER(ColumnInfo))
_sig("fls_materialize", C.c_int, _P, C.c_uint32, C.POINTER(C.c_uint8), C.POINTER(RowGroup))
_sig("fls_scan_begin", C.c_int, _P, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32)
_sig("fls_scan_next", C.c_int, _P, C.POINTER(RowGroup))
_sig("fls_scan_acquire", C.c_int, _P, C.POINTER(RowGroup))
_sig("fls_scan_release", C.c_int, _P, C.c_uint32)
_sig("fls_scan_filter", C.c_int, _P, C.POINTER(Predicate), C.c_uint32)
_sig("fls_scan_pruned", C.c_int, _P)
_sig("fls_keyset_create", C.c_int, _P, _P, C.c_uint64, C.c_int, C.c_int, C.POINTER(_P))
_sig("fls_keyset_free", None, _P)
_sig("fls_keyset_info", C.c_int, _P, C.POINTER(KeySetInfo))
_sig("fls_keyset_contains", C.c_int, _P, C.c_uint64)
_sig("fls_keyset_from_scan", C.c_int, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_P),
     C.POINTER(KeySetBuildInfo))
_sig("fls_keymap_create", C.c_int, _P, _P, _P, C.c_uint64, C.c_int, C.c_int, C.POINTER(_P))
_sig("fls_keymap_free", None, _P)
_sig("fls_keymap_info", C.c_int, _P, C.POINTER(KeyMapInfo))
_sig("fls_keymap_lookup", C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint32))
_sig("fls_valuemap_create", C.c_int, _P, _P, _P, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(_P))
_sig("fls_valuemap_free", None, _P)
_sig("fls_valuemap_info", C.c_int, _P, C.POINTER(ValueMapInfo))
_sig("fls_valuemap_lookup", C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64))
_sig("fls_valuemap_from_scan", C.c_int, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_P),
     C.POINTER(MapBuildInfo))
_sig("fls_keymap_from_scan", C.c_int, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_P),
     C.POINTER(MapBuildInfo))
_sig("fls_aggregate_value_bindings", C.c_int, _P, C.POINTER(ValueBinding), C.c_uint32)
_sig("fls_aggregate_key_bindings", C.c_int, _P, C.POINTER(KeyBinding), C.c_uint32)
_sig("fls_aggregate", C.c_int, _P, C.POINTER(AggregateSpec), C.c_uint32, C.c_uint32, C.c_uint32,
     C.POINTER(AggregateValue))
_sig("fls_aggregate_exprs", C.c_int, _P, C.POINTER(AggExpr), C.c_uint32)
_sig("fls_aggregate_conditions", C.c_int, _P, C.POINTER(Predicate), C.c_uint32, C.POINTER(AggCondition), C.c_uint32)
_sig("fls_scan_filter_alternatives", C.c_int, _P, C.POINTER(Predicate), C.c_uint32, C.POINTER(FilterAlternative),
     C.c_uint32)
_sig("fls_aggregate_grouped", C.c_int, _P, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(AggregateSpec), C.c_uint32,
     C.c_uint32, C.c_uint32, C.POINTER(_P))
_sig("fls_group_result_ngroups", C.c_uint64, _P)
_sig("fls_group_result_key", C.c_int, _P, C.c_uint64, C.c_uint32, C.POINTER(GroupKey))
_sig("fls_group_result_values", C.POINTER(AggregateValue), _P, C.c_uint64)
_sig("fls_group_result_free", None, _P)
_PU64, _PU8 = C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint8))
_sig("fls_aggregate_hashed", C.c_int, _P, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(AggregateSpec), C.c_uint32,
     C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(_P))
_sig("fls_hash_result_ngroups", C.c_uint64, _P)
_sig("fls_hash_result_first_rows", C.c_int, _P, _PU64)
_sig("fls_hash_result_key", C.c_int, _P, C.c_uint32, _PU64, _PU8)
_sig("fls_hash_result_aggregate", C.c_int, _P, C.c_uint32, _PU64, _PU64, _PU64, _PU8)
_sig("fls_hash_result_stats", C.c_int, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double),
     C.POINTER(C.c_double))
_sig("fls_hash_result_free", None, _P)
_sig("fls_aggregate_hashed_select", C.c_int, _P, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(AggregateSpec),
     C.c_uint32, C.c_uint64, C.POINTER(GroupSelect), C.c_uint32, C.c_uint32, C.POINTER(_P))
_sig("fls_hash_result_select_stats", C.c_int, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int),
     C.POINTER(C.c_double))
_sig("fls_topn", C.c_int, _P, C.POINTER(OrderKey), C.c_uint32, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32,
     C.POINTER(_P))
_sig("fls_topn_pruned", C.c_int, _P, C.POINTER(OrderKey), C.c_uint32, C.c_uint32, C.c_uint32)
_sig("fls_topn_result_nrows", C.c_uint64, _P)
_sig("fls_topn_result_rows", C.POINTER(C.c_uint64), _P)
_sig("fls_topn_result_column", C.c_int, _P, C.c_uint32, C.POINTER(_P), C.POINTER(C.POINTER(C.c_uint64)))
_sig("fls_topn_result_times", C.c_int, _P, C.POINTER(C.c_double), C.POINTER(C.c_double))
_sig("fls_topn_result_free", None, _P)
_sig("fls_table_zonemap", C.c_int, _P, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
     C.POINTER(C.c_uint32))
_sig("fls_scan_dict_codes", C.c_int, _P, C.c_int)
_sig("fls_scan_narrow", C.c_int, _P, C.c_int)
_sig("fls_scan_defer_records", C.c_int, _P, C.c_int)
_sig("fls_scan_build_records", C.c_int, _P, C.POINTER(RowGroup))
_sig("fls_table_validity", C.c_int, _P, C.c_uint32, C.c_uint32, C.POINTER(C.POINTER(C.c_uint64)))
_sig("fls_rowgroup_may_match", C.c_int, _P, C.c_uint32, C.POINTER(Predicate), C.c_uint32)
_sig("fls_device_upload", C.c_int, _P, C.c_uint32, C.c_uint32)
_sig("fls_device_decode", C.c_int, _P, C.POINTER(C.c_uint8))
_sig("fls_device_sync", C.c_int, _P, C.POINTER(DecodeStats))
_sig("fls_device_column", C.c_int, _P, C.c_uint32, C.POINTER(_P), C.POINTER(C.c_uint64))
_sig("fls_device_copy_out", C.c_int, _P, C.c_uint32, C.c_uint64, C.c_uint64, _P)
_sig("fls_device_rows", C.c_uint64, _P)
_sig("fls_device_heap", C.c_int, _P, C.c_uint32, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_uint64))
_sig("fls_device_parts", C.c_int, _P)
_sig("fls_device_part", C.c_int, _P, C.c_uint32, C.POINTER(PartInfo))
_sig("fls_device_part_column", C.c_int, _P, C.c_uint32, C.c_uint32, C.POINTER(_P), C.POINTER(C.c_uint64))
_sig("fls_device_part_heap", C.c_int, _P, C.c_uint32, C.c_uint32, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_uint64))
_sig("fls_writer_new", _P, C.c_uint64)
_sig("fls_writer_free", None, _P)
_sig("fls_writer_add_column", C.c_int, _P, C.c_char_p, C.c_uint8, C.c_uint8, C.c_uint8, C.c_uint8)
_sig("fls_writer_add_rowgroup", C.c_int, _P, C.c_uint32, C.POINTER(_P), C.POINTER(_P))
_sig("fls_writer_set_threads", C.c_int, _P, C.c_int)
_sig("fls_writer_add_rowgroups", C.c_int, _P, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(_P), C.POINTER(_P))
_sig("fls_writer_add_rowgroups_v", C.c_int, _P, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(_P), C.POINTER(_P),
     C.POINTER(_P))
_sig("fls_writer_set_rowgroup_size", C.c_int, _P, C.c_uint32)
_sig("fls_writer_set_device", C.c_int, _P, C.c_int)
_sig("fls_device_alloc", C.c_int, C.c_int, C.c_uint64, C.POINTER(_P))
_sig("fls_device_free", C.c_int, C.c_int, _P)
_sig("fls_device_memcpy", C.c_int, C.c_int, _P, _P, C.c_uint64, C.c_int)
_sig("fls_encode_slot_bytes", C.c_uint64, C.c_uint8, C.c_uint8, C.c_uint32)
_sig("fls_encode_device", C.c_int, C.c_int, C.c_uint8, C.c_uint8, _P, C.c_uint64, C.c_uint32, _P,
     C.POINTER(C.c_uint64), C.POINTER(C.c_float))
_sig("fls_writer_finish_file", C.c_int, _P, C.c_char_p)
_sig("fls_writer_set_output", C.c_int, _P, C.c_char_p)
_sig("fls_writer_set_pipelined", C.c_int, _P, C.c_int)
_sig("fls_writer_finish_image", C.c_int, _P, C.POINTER(_P), C.POINTER(C.c_uint64))
_sig("fls_image_free", None, _P)
_sig("fls_gen_nrows", C.c_int64, C.c_char_p, C.c_double, C.c_uint64)
_sig("fls_gen_ncols", C.c_int, C.c_char_p)
_sig("fls_gen_image", C.c_int, C.c_char_p, C.c_double, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int,
     C.POINTER(_P), C.POINTER(C.c_uint64))
_sig("fls_gen_values", C.c_int, C.c_char_p, C.c_double, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, _P)
_sig("fls_gen_dict_string", C.c_char_p, C.c_char_p, C.c_int, C.c_uint32)
_sig("fls_gen_strings", C.c_int64, C.c_char_p, C.c_double, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, _P, _P,
     C.c_uint64)

lib = _lib


def _check(rc: int) -> int:
    if rc < 0:
        raise FlsError(rc, (_lib.fls_last_error() or b"").decode(errors="replace"))
    return rc


def last_error() -> str:
    return (_lib.fls_last_error() or b"").decode(errors="replace")


def version() -> str:
    return _lib.fls_version().decode()


def config() -> dict[str, tuple[int, int]]:
    """The deployment knobs: name -> (compiled default, value in effect)."""
    out = {}
    for i in range(_lib.fls_config_count()):
        name = _lib.fls_config_name(i)
        d, v = C.c_int64(), C.c_int64()
        _check(_lib.fls_config_default(name, C.byref(d)))
        _check(_lib.fls_config_value(name, C.byref(v)))
        out[name.decode()] = (d.value, v.value)
    return out


def device_count() -> int:
    return _lib.fls_device_count()


# --- images ------------------------------------------------------------------
class Image:
    """An .fls file image in host memory (library-allocated, freed on close)."""

    def __init__(self, ptr: int, length: int):
        self.ptr, self.len = ptr, length

    def tobytes(self) -> bytes:
        return C.string_at(self.ptr, self.len)

    def view(self) -> np.ndarray:
        return np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_uint8)), shape=(self.len,))

    def write(self, path: str) -> None:
        Path(path).write_bytes(self.tobytes())

    def close(self) -> None:
        if self.ptr:
            _lib.fls_image_free(self.ptr)
            self.ptr = None

    def __del__(self):
        self.close()


def _take_image(rc, p, n) -> Image:
    _check(rc)
    return Image(p.value, n.value)


def gen_nrows(workload: str, scale: float = 1.0, nrows: int = 0) -> int:
    return _check(_lib.fls_gen_nrows(workload.encode(), scale, nrows))


def gen_image(workload: str, scale: float = 1.0, nrows: int = 0, rg_begin: int = 0,
              rg_end: int | None = None, nthreads: int | None = None) -> Image:
    if rg_end is None:
        rg_end = 0xFFFFFFFF
    if nthreads is None:
        nthreads = min(16, os.cpu_count() or 1)
    p, n = _P(), C.c_uint64()
    rc = _lib.fls_gen_image(workload.encode(), scale, nrows, rg_begin, rg_end, nthreads, C.byref(p), C.byref(n))
    return _take_image(rc, p, n)


def gen_values(workload: str, col: int, row_begin: int, n: int, dtype, scale: float = 1.0,
               nrows: int = 0) -> np.ndarray:
    out = np.empty(n, dtype=dtype)
    _check(_lib.fls_gen_values(workload.encode(), scale, nrows, col, row_begin, n, out.ctypes.data))
    return out


def gen_strings(workload: str, col: int, row_begin: int, n: int, scale: float = 1.0, nrows: int = 0) -> list[bytes]:
    """Ground-truth strings of a generated VARCHAR column (dictionary or l_comment)."""
    offs = np.zeros(n + 1, dtype=np.uint32)
    cap = max(64, 48 * n)
    buf = np.empty(cap, dtype=np.uint8)
    got = _lib.fls_gen_strings(workload.encode(), scale, nrows, col, row_begin, n, offs.ctypes.data, buf.ctypes.data,
                               cap)
    if got < 0:
        _check(int(got))
    b = buf[:got].tobytes()
    return [b[offs[i]:offs[i + 1]] for i in range(n)]


def gen_dict_string(workload: str, col: int, code: int) -> str | None:
    s = _lib.fls_gen_dict_string(workload.encode(), col, code)
    return None if s is None else s.decode()


# --- writer ----------------------------------------------------------------
def write_image(columns, rowgroup: int = ROWGROUP, row_offset: int = 0, device: int = -1,
                batch: int = 1, threads: int = 0, path: str | None = None, stream: bool = False,
                pipelined: bool = False) -> Image | None:
    """columns: list of (name, type, values, encoding[, width, scale]).
    values: numpy int array for integer types, float array for FLOAT/DOUBLE
    (stored bit-exactly), list of str/bytes for VARCHAR.  NULLs: None entries
    of a list, or the masked entries of a numpy.ma array (the rows' validity
    goes to fls_writer_add_rowgroups_v).  device >= 0: the
    FFOR / DELTA integer columns are encoded on that GPU (same bytes).
    batch > 1: row groups go in `batch` at a time (fls_writer_add_rowgroups;
    same bytes).  threads > 0: writer threads (fls_writer_set_threads).
    path: the file is written there instead (fls_writer_finish_file: the
    same bytes, chunks written in parallel, no image); returns None.
    stream: with path, row groups go to the file as they are encoded
    (fls_writer_set_output; the same bytes).  pipelined: a call returns
    before its row groups are encoded (fls_writer_set_pipelined; the same
    bytes), so each batch's buffers are kept until the next call returns."""
    w = _lib.fls_writer_new(row_offset)
    try:
        _check(_lib.fls_writer_set_rowgroup_size(w, rowgroup))
        if threads > 0:
            _check(_lib.fls_writer_set_threads(w, threads))
        if device >= 0:
            _check(_lib.fls_writer_set_device(w, device))
        if stream and path is not None:
            _check(_lib.fls_writer_set_output(w, str(path).encode()))
        if pipelined:
            _check(_lib.fls_writer_set_pipelined(w, 1))
        n = None
        held = None  # pipelined: the previous call's buffers
        prepped = []
        for spec in columns:
            name, ty, vals, enc = spec[:4]
            width, scale = (spec[4], spec[5]) if len(spec) > 4 else (0, 0)
            _check(_lib.fls_writer_add_column(w, name.encode(), ty, width, scale, enc))
            valid = None
            if isinstance(vals, np.ma.MaskedArray):
                valid = ~np.ma.getmaskarray(vals)
                vals = vals.filled(0)
            elif isinstance(vals, list) and any(v is None for v in vals):
                valid = np.array([v is not None for v in vals], dtype=bool)
                vals = [(b"" if ty in STRING_TYPES else 0) if v is None else v for v in vals]
            if ty in STRING_TYPES:
                bs = [v.encode() if isinstance(v, str) else bytes(v) for v in vals]
                prepped.append(("s", bs, valid))
                cnt = len(bs)
            else:
                arr = np.ascontiguousarray(np.asarray(vals).astype(NP_DTYPE[ty]))
                prepped.append(("i", arr, valid))
                cnt = len(arr)
            if n is None:
                n = cnt
            elif n != cnt:
                raise ValueError("columns differ in length")
        nc = len(prepped)
        starts = list(range(0, n or 0, rowgroup))
        for b0 in range(0, len(starts), max(1, batch)):
            grp = starts[b0:b0 + max(1, batch)]
            keep = []
            data = (_P * (nc * len(grp)))()
            offs = (_P * (nc * len(grp)))()
            vmask = (_P * (nc * len(grp)))()
            rows = (C.c_uint32 * len(grp))()
            for k, r0 in enumerate(grp):
                r1 = min(n, r0 + rowgroup)
                rows[k] = r1 - r0
                for c, (kind, v, valid) in enumerate(prepped):
                    if valid is not None:
                        words = np.packbits(valid[r0:r1], bitorder="little")
                        words = np.concatenate([words, np.zeros((-len(words)) % 8, np.uint8)]).view(np.uint64)
                        keep.append(words)
                        vmask[k * nc + c] = words.ctypes.data
                    if kind == "i":
                        part = np.ascontiguousarray(v[r0:r1])
                        keep.append(part)
                        data[k * nc + c] = part.ctypes.data
                    else:
                        sl = v[r0:r1]
                        o = np.zeros(len(sl) + 1, dtype=np.uint32)
                        o[1:] = np.cumsum([len(x) for x in sl], dtype=np.uint64).astype(np.uint32)
                        buf = np.frombuffer(b"".join(sl) or b"\0", dtype=np.uint8).copy()
                        keep += [o, buf]
                        data[k * nc + c] = buf.ctypes.data
                        offs[k * nc + c] = o.ctypes.data
            if any(p[2] is not None for p in prepped):
                _check(_lib.fls_writer_add_rowgroups_v(w, len(grp), rows, data, offs, vmask))
            elif batch > 1:
                _check(_lib.fls_writer_add_rowgroups(w, len(grp), rows, data, offs))
            else:
                _check(_lib.fls_writer_add_rowgroup(w, rows[0], data, offs))
            held = (keep, data, offs, vmask, rows)
        if path is not None:
            _check(_lib.fls_writer_finish_file(w, str(path).encode()))
            return None
        p, ln = _P(), C.c_uint64()
        rc = _lib.fls_writer_finish_image(w, C.byref(p), C.byref(ln))
        return _take_image(rc, p, ln)
    finally:
        _lib.fls_writer_free(w)


def encode_device(device: int, ty: int, enc: int, d_values: int, nrows: int, d_out: int,
                  rowgroup: int = ROWGROUP):
    """GPU chunk encoder over a device-resident column (fls_encode_device):
    d_values / d_out are device addresses (e.g. torch tensor data_ptr()).
    Returns (chunk lengths, kernel ms); chunk i starts at
    d_out + i * encode_slot_bytes(ty, enc, rowgroup)."""
    nrg = (nrows + rowgroup - 1) // rowgroup
    lens = (C.c_uint64 * nrg)()
    ms = C.c_float()
    _check(_lib.fls_encode_device(device, ty, enc, d_values, nrows, rowgroup, d_out, lens, C.byref(ms)))
    return [int(x) for x in lens], float(ms.value)


def encode_slot_bytes(ty: int, enc: int, rowgroup: int = ROWGROUP) -> int:
    return int(_lib.fls_encode_slot_bytes(ty, enc, rowgroup))


class DeviceBuffer:
    """A raw device allocation through the engine's own HIP runtime
    (fls_device_alloc): no second runtime (e.g. torch's) in the process."""

    def __init__(self, nbytes: int, device: int = 0):
        self.device, self.nbytes = device, int(nbytes)
        p = _P()
        _check(_lib.fls_device_alloc(device, self.nbytes, C.byref(p)))
        self.ptr = p.value

    @classmethod
    def from_array(cls, arr: np.ndarray, device: int = 0) -> "DeviceBuffer":
        arr = np.ascontiguousarray(arr)
        b = cls(arr.nbytes, device)
        _check(_lib.fls_device_memcpy(device, b.ptr, arr.ctypes.data, arr.nbytes, 0))
        return b

    def read(self, offset: int = 0, nbytes: int | None = None) -> bytes:
        n = self.nbytes - offset if nbytes is None else nbytes
        out = np.empty(n, dtype=np.uint8)
        if n:
            _check(_lib.fls_device_memcpy(self.device, out.ctypes.data, self.ptr + offset, n, 1))
        return out.tobytes()

    def free(self):
        if self.ptr:
            _lib.fls_device_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        self.free()


# --- engine ----------------------------------------------------------------
class Connection:
    """fastlanes::connect() counterpart: a set of GPUs to shard row groups over."""

    def __init__(self, devices=None):
        h = _P()
        if devices:
            arr = (C.c_int * len(devices))(*devices)
            _check(_lib.fls_connect(arr, len(devices), C.byref(h)))
        else:
            _check(_lib.fls_connect(None, 0, C.byref(h)))
        self.h = h.value
        self.devices = list(devices) if devices else [0]

    def trim(self, keep_bytes: int = 0) -> int:
        """Free idle scan pipelines down to keep_bytes of pinned memory per
        GPU; returns the pinned bytes still idle."""
        left = C.c_uint64()
        _check(_lib.fls_connection_trim(self.h, keep_bytes, C.byref(left)))
        return left.value

    @staticmethod
    def release_device_memory(device: int = -1) -> int:
        """Free the HBM-resident file images no running scan uses on device
        (-1: every GPU); returns the bytes freed (fls_release_device_memory)."""
        freed = C.c_uint64()
        _check(_lib.fls_release_device_memory(device, C.byref(freed)))
        return freed.value

    @staticmethod
    def resident_info(device: int = -1):
        """(bytes, images) of the HBM-resident file images on device (-1: all)."""
        b, n = C.c_uint64(), C.c_uint32()
        _check(_lib.fls_resident_info(device, C.byref(b), C.byref(n)))
        return b.value, n.value

    def read_fls(self, path: str) -> "Table":
        h = _P()
        _check(_lib.fls_read_fls(self.h, str(path).encode(), C.byref(h)))
        return Table(h.value, self)

    def read_image(self, img, copy: bool = False) -> "Table":
        h = _P()
        if hasattr(img, "ptr") and hasattr(img, "len"):  # an Image (possibly from another loaded build)
            _check(_lib.fls_read_fls_image(self.h, img.ptr, img.len, int(copy), C.byref(h)))
            t = Table(h.value, self)
            t._keep = img
            return t
        buf = bytes(img)
        _check(_lib.fls_read_fls_image(self.h, buf, len(buf), 1, C.byref(h)))
        return Table(h.value, self)

    def keyset(self, values, signed: bool = True, form: int = KEYSET_AUTO) -> "KeySet":
        """A key set for (col, "in_set" / "not_in_set", keyset) filter terms
        (fls_keyset_create): values are integers of the probed column's
        physical type (DATE days, DECIMAL scaled), signed its order (False for
        UINT* and BOOLEAN columns), form 0 auto / 1 bitmap / 2 hash table.
        Built on the host; no GPU is needed.  TypeError for anything but
        integers (a float is never truncated into a key)."""
        a = _key_patterns(values, "keyset")
        h = _P()
        _check(_lib.fls_keyset_create(self.h, a.ctypes.data if a.size else None, a.size, 0 if signed else 1, form,
                                      C.byref(h)))
        return KeySet(h.value, self)

    def keymap(self, keys, values, signed: bool = True, form: int = KEYMAP_AUTO) -> "KeyMap":
        """A key map for ("map", col, keymap) GROUP BY keys (fls_keymap_create):
        keys as keyset() takes them, values their codes, integers in
        [0, 65534]; a key listed with two codes is refused.  form 0 auto /
        1 dense / 2 hash table.  Built on the host; no GPU is needed."""
        k = _key_patterns(keys, "keymap")
        v = _key_patterns(values, "keymap")
        if v.size != k.size:
            raise ValueError(f"keymap: {k.size} keys and {v.size} values")
        if v.size and int(v.max()) > KEYMAP_ABSENT:     # (a negative value is a pattern past 2^63)
            bad = int(v.max())
            raise ValueError(f"keymap: value {bad - (1 << 64) if bad >> 63 else bad} is outside [0, 65534]")
        v = np.ascontiguousarray(v.astype(np.uint16))   # (65535 itself is the library's to refuse)
        h = _P()
        _check(_lib.fls_keymap_create(self.h, k.ctypes.data if k.size else None, v.ctypes.data if v.size else None,
                                      k.size, 0 if signed else 1, form, C.byref(h)))
        return KeyMap(h.value, self)

    def valuemap(self, keys, values, signed: bool = True, value_signed: bool = True,
                 form: int = VALUEMAP_AUTO) -> "ValueMap":
        """A value map for (a, op, Mapped(key_col, valuemap)) filter terms
        (fls_valuemap_create): keys as keyset() takes them, values integers of
        the compared column's physical type (DATE days, DECIMAL scaled);
        signed / value_signed the order of the keys / of the values (False for
        UINT* and BOOLEAN columns).  A key listed with two values is refused.
        form 0 auto / 1 dense / 2 hash table.  Built on the host; no GPU is
        needed."""
        k = _key_patterns(keys, "valuemap")
        v = _key_patterns(values, "valuemap")
        if v.size != k.size:
            raise ValueError(f"valuemap: {k.size} keys and {v.size} values")
        h = _P()
        _check(_lib.fls_valuemap_create(self.h, k.ctypes.data if k.size else None, v.ctypes.data if v.size else None,
                                        k.size, 0 if signed else 1, 0 if value_signed else 1, form, C.byref(h)))
        return ValueMap(h.value, self)

    def close(self):
        if self.h:
            _lib.fls_disconnect(self.h)
            self.h = None


def _key_patterns(values, who: str) -> np.ndarray:
    """integers as the 64-bit patterns a key set or key map holds (uint64,
    contiguous); TypeError for anything but integers"""
    # (a list goes value by value: numpy would turn Python integers of mixed sign past 2^63 into floats)
    a = values if isinstance(values, np.ndarray) else np.asarray(list(values), dtype=object)
    if a.size == 0:
        a = np.zeros(0, np.uint64)
    elif a.dtype == object:
        vals = list(a.ravel())
        for v in vals:
            if not isinstance(v, (int, np.integer, np.bool_)):
                raise TypeError(f"{who}: {v!r} is not an integer")
        a = np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in vals], dtype=np.uint64)
    elif a.dtype.kind not in "iub":
        raise TypeError(f"{who}: values of dtype {a.dtype} are not integers")
    elif a.dtype.kind == "i":
        a = a.astype(np.int64).view(np.uint64)    # sign-extended patterns
    else:
        a = a.astype(np.uint64)
    return np.ascontiguousarray(a.ravel())


class KeyMap:
    """fls_keymap: the build side of a join whose payload is a GROUP BY code.
    The handle is a token the library looks up; a closed map in a binding is
    refused, never dereferenced.  build_info: the MapBuildInfo of a map
    Table.keymap built on the GPU (fls_keymap_from_scan), None for a map
    built on the host."""

    def __init__(self, h, conn, build_info=None):
        self.h, self.conn, self.build_info = h, conn, build_info

    @property
    def info(self) -> KeyMapInfo:
        out = KeyMapInfo()
        _check(_lib.fls_keymap_info(self.h, C.byref(out)))
        return out

    def lookup(self, key: int):
        """Host probe of the image a scan uploads: the code, or None."""
        code = C.c_uint32()
        found = _check(_lib.fls_keymap_lookup(self.h, int(key) & 0xFFFFFFFFFFFFFFFF, C.byref(code)))
        return code.value if found == 1 else None

    def close(self):
        if self.h:
            _lib.fls_keymap_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ValueMap:
    """fls_valuemap: the build side of a join whose payload is a value a row
    is compared with.  The handle is a token the library looks up; a closed
    map in a filter term is refused, never dereferenced.  build_info: the
    MapBuildInfo of a map Table.valuemap built on the GPU
    (fls_valuemap_from_scan), None for a map built on the host."""

    def __init__(self, h, conn, build_info=None):
        self.h, self.conn, self.build_info = h, conn, build_info

    @property
    def info(self) -> ValueMapInfo:
        out = ValueMapInfo()
        _check(_lib.fls_valuemap_info(self.h, C.byref(out)))
        return out

    def lookup(self, key: int):
        """Host probe of the image a scan uploads: the value (an int in the
        value kind's range), or None."""
        val = C.c_uint64()
        found = _check(_lib.fls_valuemap_lookup(self.h, int(key) & 0xFFFFFFFFFFFFFFFF, C.byref(val)))
        if found != 1:
            return None
        v = val.value
        return v - (1 << 64) if self.info.value_kind == KIND_SIGNED and v >> 63 else v

    def close(self):
        if self.h:
            _lib.fls_valuemap_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KeySet:
    """fls_keyset: the build side of a semi-join.  The handle is a token the
    library looks up; a closed set in a filter is refused, never dereferenced.
    build_info: the KeySetBuildInfo of a set Table.keyset built on the GPU
    (fls_keyset_from_scan), None for a set built on the host."""

    def __init__(self, h, conn, build_info=None):
        self.h, self.conn, self.build_info = h, conn, build_info

    @property
    def info(self) -> KeySetInfo:
        out = KeySetInfo()
        _check(_lib.fls_keyset_info(self.h, C.byref(out)))
        return out

    def contains(self, key: int) -> bool:
        """Host probe of the image a scan uploads."""
        return _check(_lib.fls_keyset_contains(self.h, int(key) & 0xFFFFFFFFFFFFFFFF)) == 1

    def close(self):
        if self.h:
            _lib.fls_keyset_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _mask(t: "Table", cols) -> C.Array | None:
    if cols is None:
        return None
    m = (C.c_uint8 * t.ncols)()
    for c in cols:
        if isinstance(c, Mapped) or (isinstance(c, int) and c & COL_MAPPED):
            raise ValueError(f"column {c!r}: a mapped column cannot be delivered (it exists only inside an aggregate "
                             "call, as an operand or a key of aggregate_hashed)")
        m[c] = 1
    return m


def _agg_exprs(exprs) -> C.Array:
    """fls_agg_expr[] of lists of (k, sign, col) factors, passed as given (the
    C call checks them)"""
    arr = (AggExpr * max(1, len(exprs)))()
    for i, factors in enumerate(exprs):
        arr[i].nfactors = len(factors)
        for j, (k, sign, col) in enumerate(factors[:3]):
            arr[i].f[j].k, arr[i].f[j].sign, arr[i].f[j].col = k, sign, col
    return arr


def _mapped_col(x, binds):
    """a column index as given, or for a Mapped COL_MAPPED | its place in
    binds, the call's list of distinct Mapped objects (appended to)"""
    if not isinstance(x, Mapped):
        return x
    if x not in binds:
        binds.append(x)
    return COL_MAPPED | binds.index(x)


def _agg_specs(aggs, binds=None):
    """fls_aggregate_spec[] of aggregate()'s tuples, the factor lists of its
    ("sum_expr", [...]) items in the order their specs index them, and the
    distinct conditions of its When items in the order their specs' cond - 1
    index them (equal conditions share one); a first element that is an int is
    passed through as the function code.  A Mapped in a column's place becomes
    COL_MAPPED | i and joins binds, the call's value bindings."""
    binds = [] if binds is None else binds
    arr = (AggregateSpec * max(1, len(aggs)))()
    exprs, conds = [], []
    for i, a in enumerate(aggs[:len(arr)]):
        if isinstance(a, When):
            if a.filt not in conds:
                conds.append(a.filt)
            arr[i].cond = conds.index(a.filt) + 1
            a = a.agg
        fn = a[0]
        if fn == "sum_expr":
            arr[i].fn = AGG_FNS[fn]
            arr[i].col = len(exprs)
            exprs.append([tuple(f[:2]) + (_mapped_col(f[2], binds),) + tuple(f[3:]) if len(f) > 2 else f
                          for f in a[1]])
            continue
        if isinstance(fn, str):
            fn = AGG_FNS["count_star" if fn == "count" and len(a) == 1 else fn]
        arr[i].fn = fn
        arr[i].col = _mapped_col(a[1], binds) if len(a) > 1 else 0
        arr[i].col2 = _mapped_col(a[2], binds) if len(a) > 2 else 0
    return arr, exprs, conds


def _agg_value(v: AggregateValue):
    """an fls_aggregate_value as aggregate() returns it"""
    if v.kind == AGGV_NULL:
        return None
    if v.kind == AGGV_DOUBLE:
        return float(np.array([v.lo], dtype=np.uint64).view(np.float64)[0])
    x = (v.hi << 64) | v.lo
    return x - (1 << 128) if x >> 127 else x


MAX_HASH_GROUPS = 1 << 28         # kMaxHashGroups


class HashGroups:
    """The groups of Table.aggregate_hashed, as numpy arrays copied out of the
    fls_hash_result, in unspecified order: first_row (uint64: the global row
    index of each group's first selected row), key_values[q] (uint64: key q's
    value sign- or zero-extended to 64 bits; view it as int64 for a signed
    column) and key_null[q] (bool), and per aggregate a the arrays count[a],
    lo[a], hi[a] (uint64) and kind[a] (uint8, AGGV_*) with
    fls_aggregate_value's meaning.  key_signed[q] says how key q extends.
    table_bytes is one pipeline's table; scan_ms, extract_ms (compaction and
    D2H) and merge_ms are the call's phases on the host clock.  Of a call
    with having / order_by / limit: groups_total (the groups formed),
    groups_passed (after HAVING, before LIMIT), selected_on_device (the
    selection ran on the GPU: one pipeline held the groups) and select_ms;
    with an order_by or a limit the arrays are in result order."""

    def __init__(self, res, key_signed, naggs: int, in_result_order: bool = False):
        n = self.ngroups = int(_lib.fls_hash_result_ngroups(res))
        self.key_signed = list(key_signed)
        self.in_result_order = in_result_order

        def arr(p, dtype):
            return np.ctypeslib.as_array(p, shape=(n,)).view(dtype).copy() if n else np.zeros(0, dtype)
        p64, p64b, p64c, p8 = (C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(),
                               C.POINTER(C.c_uint8)())
        _check(_lib.fls_hash_result_first_rows(res, C.byref(p64)))
        self.first_row = arr(p64, np.uint64)
        self.key_values, self.key_null = [], []
        for q in range(len(self.key_signed)):
            _check(_lib.fls_hash_result_key(res, q, C.byref(p64), C.byref(p8)))
            self.key_values.append(arr(p64, np.uint64))
            self.key_null.append(arr(p8, np.uint8).astype(bool))
        self.count, self.lo, self.hi, self.kind = [], [], [], []
        for a in range(naggs):
            _check(_lib.fls_hash_result_aggregate(res, a, C.byref(p64), C.byref(p64b), C.byref(p64c), C.byref(p8)))
            self.count.append(arr(p64, np.uint64))
            self.lo.append(arr(p64b, np.uint64))
            self.hi.append(arr(p64c, np.uint64))
            self.kind.append(arr(p8, np.uint8))
        tb, sm, em, mm = C.c_uint64(), C.c_double(), C.c_double(), C.c_double()
        _check(_lib.fls_hash_result_stats(res, C.byref(tb), C.byref(sm), C.byref(em), C.byref(mm)))
        self.table_bytes, self.scan_ms, self.extract_ms, self.merge_ms = tb.value, sm.value, em.value, mm.value
        gt, gp, od = C.c_uint64(), C.c_uint64(), C.c_int()
        _check(_lib.fls_hash_result_select_stats(res, C.byref(gt), C.byref(gp), C.byref(od), C.byref(sm)))
        self.groups_total, self.groups_passed = gt.value, gp.value
        self.selected_on_device, self.select_ms = bool(od.value), sm.value

    def __len__(self) -> int:
        return self.ngroups

    def to_list(self, ordered: bool = True) -> list:
        """[(key_tuple, values)] in aggregate_grouped's shape: a key element an
        int or None (NULL), values as aggregate() returns them.  ordered: by
        each group's first row, which is aggregate_grouped's order; the
        groups of a call with an order_by or a limit stay in result order."""
        by_first = ordered and not self.in_result_order
        order = np.argsort(self.first_row, kind="stable") if by_first else np.arange(self.ngroups)
        keys = []
        for v, nul, sg in zip(self.key_values, self.key_null, self.key_signed):
            vals = (v.view(np.int64) if sg else v).tolist()
            keys.append([None if z else x for x, z in zip(vals, nul.tolist())])
        cols = []
        for cnt, lo, hi, kind in zip(self.count, self.lo, self.hi, self.kind):
            dbl = lo.view(np.float64).tolist()
            col = []
            for k, l, h, d in zip(kind.tolist(), lo.tolist(), hi.tolist(), dbl):
                if k == AGGV_NULL:
                    col.append(None)
                elif k == AGGV_DOUBLE:
                    col.append(d)
                else:
                    x = (h << 64) | l
                    col.append(x - (1 << 128) if x >> 127 else x)
            cols.append(col)
        return [(tuple(k[g] for k in keys), [c[g] for c in cols]) for g in order.tolist()]


class Table:
    def __init__(self, h, conn):
        self.h, self.conn, self._keep = h, conn, None
        self._alts_set = False   # alternatives are set on the table (set_filter_alternatives)
        self._vbind_signed = []  # per value binding set: its map's values are signed (set_aggregate_value_bindings)

    def close(self):
        if self.h:
            _lib.fls_table_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ncols(self) -> int:
        return _lib.fls_table_ncols(self.h)

    @property
    def nrows(self) -> int:
        return _lib.fls_table_nrows(self.h)

    @property
    def row_offset(self) -> int:
        return _lib.fls_table_row_offset(self.h)

    @property
    def nrowgroups(self) -> int:
        return _lib.fls_table_nrowgroups(self.h)

    def rowgroup_rows(self, rg: int) -> int:
        return _check(_lib.fls_table_rowgroup_rows(self.h, rg))

    def column(self, c: int) -> ColumnInfo:
        ci = ColumnInfo()
        _check(_lib.fls_table_column(self.h, c, C.byref(ci)))
        return ci

    def schema(self):
        out = []
        for c in range(self.ncols):
            ci = self.column(c)
            out.append((ci.name.decode(), ci.type, ci.width, ci.scale, ci.out_bytes))
        return out

    # -- host-delivered decode (DataChunk path)
    def _rg_arrays(self, rg: RowGroup, copy=True):
        cols = []
        sch = self.schema()
        for c in range(rg.ncols):
            p = rg.columns[c]
            if not p:
                cols.append(None)
                continue
            ob = sch[c][4]
            narrowed = bool(rg.narrow and rg.narrow[c])
            if (rg.dict and rg.dict[c]) or narrowed:
                ob = rg.dict_width[c]  # dictionary codes / narrowed values
            if rg.nrows == 0:
                cols.append(np.zeros(0, dtype=np.uint8))
                continue
            a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(rg.nrows * ob,))
            if narrowed:  # widen: value = base + narrow (mod 2^64), in the column's width
                full = sch[c][4]
                w = a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[ob]).astype(np.uint64)
                v = (w + np.uint64(rg.narrow_base[c])).astype(np.uint64)
                a = v.view(np.uint8).reshape(-1, 8)[:, :full].reshape(-1).copy()
                cols.append(a)
                continue
            cols.append(a.copy() if copy else a)
        return cols

    @staticmethod
    def _rg_valid(rg: RowGroup):
        """per column: bool per delivered row (False = NULL), or None when every
        delivered row is valid (fls_rowgroup.validity)"""
        out = []
        for c in range(rg.ncols):
            p = rg.validity[c] if rg.validity else None
            if not p:
                out.append(None)
                continue
            nw = (rg.nrows + 63) // 64
            w = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(max(1, nw),))
            out.append(np.unpackbits(w.view(np.uint8), bitorder="little")[:rg.nrows].astype(bool))
        return out

    def scan_nulls(self, cols=None, rg_begin=0, rg_end=None):
        """scan() that also yields each row group's validity and selection:
        (first_row, arrays, valid per column (None: no NULL), sel or None)"""
        if rg_end is None:
            rg_end = self.nrowgroups
        _check(_lib.fls_scan_begin(self.h, _mask(self, cols), rg_begin, rg_end))
        out = RowGroup()
        while _check(_lib.fls_scan_next(self.h, C.byref(out))) == 1:
            sel = np.ctypeslib.as_array(out.sel, shape=(out.nrows,)).copy() if out.sel and out.nrows else None
            yield out.first_row, self._rg_arrays(out), self._rg_valid(out), sel

    def narrow(self, enable: bool = True):
        """fls_scan_narrow: the next scan delivers integer columns narrowed to
        their row groups' ranges (scan() widens them back)"""
        _check(_lib.fls_scan_narrow(self.h, int(enable)))

    def dict_codes(self, enable: bool = True):
        """fls_scan_dict_codes: the next scan delivers DICT string columns as
        codes (scan_dicts yields their dictionaries)"""
        _check(_lib.fls_scan_dict_codes(self.h, int(enable)))

    def scan_dicts(self, cols=None, rg_begin=0, rg_end=None):
        """scan() yielding (first_row, arrays, dicts): dicts[c] is the row
        group's dictionary (string_t records, bytes) for a coded column, whose
        array then holds its codes (u8 / u16), else None"""
        if rg_end is None:
            rg_end = self.nrowgroups
        _check(_lib.fls_scan_begin(self.h, _mask(self, cols), rg_begin, rg_end))
        out = RowGroup()
        while _check(_lib.fls_scan_next(self.h, C.byref(out))) == 1:
            dicts = []
            for c in range(out.ncols):
                p = out.dict[c] if out.dict else None
                dicts.append(None if not p else np.ctypeslib.as_array(
                    C.cast(p, C.POINTER(C.c_uint8)), shape=(16 * out.dict_size[c],)).copy())
            arrays = self._rg_arrays(out)
            for c, dct in enumerate(dicts):
                if dct is not None:
                    arrays[c] = arrays[c].view(np.uint8 if out.dict_width[c] == 1 else np.uint16)
            yield out.first_row, arrays, dicts

    def validity(self, rg: int, col: int):
        """fls_table_validity: the chunk's validity words, or None (no NULL)"""
        p = C.POINTER(C.c_uint64)()
        if _check(_lib.fls_table_validity(self.h, rg, col, C.byref(p))) == 0:
            return None
        n = self.rowgroup_rows(rg)
        return np.ctypeslib.as_array(p, shape=(16 * ((n + 1023) // 1024),)).copy()

    def materialize(self, rg: int, cols=None):
        out = RowGroup()
        _check(_lib.fls_materialize(self.h, rg, _mask(self, cols), C.byref(out)))
        return out.first_row, self._rg_arrays(out)

    def scan(self, cols=None, rg_begin=0, rg_end=None):
        if rg_end is None:
            rg_end = self.nrowgroups
        _check(_lib.fls_scan_begin(self.h, _mask(self, cols), rg_begin, rg_end))
        out = RowGroup()
        while _check(_lib.fls_scan_next(self.h, C.byref(out))) == 1:
            yield out.first_row, self._rg_arrays(out)

    # -- pushed-down filters
    def _preds(self, filt):
        """filt: list of (col, op, value[, clause]); op a fls_cmp or one of OPS;
        value int (integers, DATE days, DECIMAL scaled), float (FLOAT/DOUBLE) or
        str/bytes (VARCHAR), or a KeySet for "in_set" / "not_in_set" (a clause
        of its own).  Terms without a clause get their own clause.
        String patterns on a VARCHAR column (DuckDB's LIKE: `%` any bytes, `_`
        one character, case-sensitive; a clause of their own, a NULL row
        satisfies neither): (col, "like" / "not_like", pattern) or
        (col, "like", (pattern, escape)) with pattern str or bytes and escape
        one byte; a None pattern selects no row.  (col, "starts_with" /
        "ends_with" / "contains", literal) build the LIKE pattern around the
        literal, its `%`, `_` and `\\` escaped with `\\`.
        Two columns of the same row: (a, op, Col(b)) with op one of `=`, `!=`,
        `<`, `<=`, `>`, `>=` (or (a, "col<", b) with the index itself): both
        values valid and a op b; a clause of its own; two signed or two
        unsigned integer columns of any widths, two DATE, two DECIMAL of one
        scale, or FLOAT / DOUBLE in any mix.
        A column against a joined attribute: (a, op, Mapped(key_col, vm)) with
        op one of the six and vm a ValueMap (or (a, "map<", (key_col, vm)), or
        (a, "map<", vm) with the left column as its own key):
        both columns valid, the key in the map and a op vm[key]; a clause of
        its own, at most 8 per list; integer-like columns whose signedness
        matches the map's value / key kind."""
        if any(isinstance(term, AnyOf) for term in filt):
            raise ValueError("an AnyOf is an element of a call's filt, not of a condition, an alternative or "
                             "may_match's terms")
        sch = self.schema()
        arr = (Predicate * max(1, len(filt)))()
        keep = []
        for i, term in enumerate(filt):
            col, op, val = term[:3]
            if isinstance(op, str) and op in _LIKE_SUGAR and val is not None:
                pre, post = _LIKE_SUGAR[op]
                op, val = "like", (pre + like_escape(val) + post, b"\\")
            elif isinstance(op, str) and op in _LIKE_SUGAR:
                op = "like"
            p = arr[i]
            p.col = col
            p.clause = term[3] if len(term) > 3 else 1000000 + i
            p.op = OPS[op] if isinstance(op, str) else op
            ty = sch[col][1] if 0 <= col < len(sch) else None
            if isinstance(val, Col):
                if p.op > GE:
                    raise TypeError(f"filter term {i}: operator {op!r} takes no column on its right")
                p.op += COL_EQ
                val = val.index
            if isinstance(val, Mapped):
                if p.op > GE:
                    raise TypeError(f"filter term {i}: operator {op!r} takes no mapped value on its right")
                if val.keep_unmatched:
                    raise ValueError(f"filter term {i}: keep_unmatched=True means nothing in a filter term (a NULL "
                                     "satisfies no operator there already)")
                p.op += MAP_EQ
                val = (val.key_col, val.valuemap)
            if MAP_EQ <= p.op <= MAP_GE:
                kc, vm = val if isinstance(val, tuple) else (col, val)   # (a map alone: keyed by the left column itself)
                p.key_col = int(kc) & 0xFFFFFFFF
                p.value = (vm.h or 0) if isinstance(vm, ValueMap) else int(vm)   # the map's handle
                keep.append(vm)
            elif COL_EQ <= p.op <= COL_GE:
                p.value = int(val) & 0xFFFFFFFFFFFFFFFF   # the right column's index, no literal conversion
            elif p.op in (LIKE, NOT_LIKE):
                pat, esc = val if isinstance(val, tuple) else (val, None)
                if pat is None:
                    p.op = OPS["false"]   # a NULL pattern: no row
                    continue
                if ty not in STRING_TYPES:
                    continue              # the engine refuses the term by name
                b = _pat_bytes(pat, "like pattern")
                if esc is not None:
                    e = _pat_bytes(esc, "like escape")
                    if len(e) != 1 or e == b"\0":
                        raise ValueError(f"like: the escape {esc!r} is not one non-NUL byte")
                    p.value = e[0]
                buf = C.create_string_buffer(b, len(b) + 1)
                keep.append(buf)
                p.str = C.cast(buf, C.c_char_p)
                p.str_len = len(b)
            elif p.op in (IN_SET, NOT_IN_SET):
                p.value = (val.h or 0) if isinstance(val, KeySet) else int(val)   # the set's handle
                keep.append(val)
            elif val is None or ty is None:
                pass
            elif ty in STRING_TYPES:
                b = val.encode() if isinstance(val, str) else bytes(val)
                buf = C.create_string_buffer(b, len(b) + 1)
                keep.append(buf)
                p.str = C.cast(buf, C.c_char_p)
                p.str_len = len(b)
            elif ty == FLOAT:
                p.value = int(np.array([val], dtype=np.float32).view(np.uint32)[0])
            elif ty == DOUBLE:
                p.value = int(np.array([val], dtype=np.float64).view(np.uint64)[0])
            else:
                p.value = int(val) & 0xFFFFFFFFFFFFFFFF
        return arr, len(filt), keep

    def set_filter(self, filt):
        """The filter of the following scans and aggregate / top-N calls: its
        terms (fls_scan_filter) and, when it holds an AnyOf, that element's
        alternatives (fls_scan_filter_alternatives); without one, alternatives
        set earlier are cleared."""
        base, alts = _split_filter(filt)
        arr, n, keep = self._preds(base)
        packed = self._pack_lists(alts) if alts is not None else None
        _check(_lib.fls_scan_filter(self.h, arr, n))
        if packed is not None or self._alts_set:
            try:
                self._set_alternatives(packed)
            except FlsError:
                _lib.fls_scan_filter(self.h, None, 0)   # a refused AnyOf leaves no half of the filter behind
                raise

    def _pack_lists(self, lists, range_type=FilterAlternative):
        """several filters as one Predicate array and their ranges in it"""
        parts = [self._preds(c) for c in lists]
        preds = (Predicate * max(1, sum(n for _, n, _ in parts)))()
        ranges = (range_type * max(1, len(lists)))()
        k = 0
        for i, (arr, n, _keep) in enumerate(parts):
            ranges[i].first, ranges[i].n = k, n
            for j in range(n):
                preds[k + j] = arr[j]
            k += n
        return preds, k, ranges, len(lists), parts   # (parts keep the strings alive until the call has copied them)

    def _set_alternatives(self, packed):
        if packed is None:
            _check(_lib.fls_scan_filter_alternatives(self.h, None, 0, None, 0))
            self._alts_set = False
            return
        preds, k, ranges, n, _parts = packed
        _check(_lib.fls_scan_filter_alternatives(self.h, preds if k else None, k, ranges if n else None, n))
        self._alts_set = n > 0

    def set_filter_alternatives(self, alternatives):
        """fls_scan_filter_alternatives, the raw call: the alternatives (each a
        filter as scan_filtered takes it, at most 8) AND-ed as a group to the
        filter set by set_filter in the following calls; a row is selected
        where the filter and at least one alternative hold.  [] or None
        clears.  What an AnyOf element of a filt sets and clears per call."""
        self._set_alternatives(self._pack_lists(alternatives) if alternatives else None)

    def _clear_filter(self):
        _check(_lib.fls_scan_filter(self.h, None, 0))
        if self._alts_set:
            self._set_alternatives(None)

    def may_match(self, rg: int, filt) -> bool:
        arr, n, keep = self._preds(filt)   # (no AnyOf: the call takes explicit terms)
        return _check(_lib.fls_rowgroup_may_match(self.h, rg, arr, n)) == 1

    @property
    def pruned(self) -> int:
        return _check(_lib.fls_scan_pruned(self.h))

    def zonemap(self, rg: int, col: int):
        """(min, max, flags) in the column's comparison domain, or None."""
        lo, hi, fl = C.c_uint64(), C.c_uint64(), C.c_uint32()
        if _check(_lib.fls_table_zonemap(self.h, rg, col, C.byref(lo), C.byref(hi), C.byref(fl))) == 0:
            return None
        ty = self.column(col).type
        if ty in (FLOAT, DOUBLE):
            cv = lambda x: float(np.array([x], dtype=np.uint64).view(np.float64)[0])  # noqa: E731
        elif ty in (INT8, INT16, INT32, INT64, DATE, DECIMAL):
            cv = lambda x: int(np.array([x], dtype=np.uint64).view(np.int64)[0])  # noqa: E731
        else:
            cv = int
        return cv(lo.value), cv(hi.value), fl.value

    def scan_filtered(self, filt, cols=None, rg_begin=0, rg_end=None):
        """Filtered scan: yields (rowgroup, first_row, sel, arrays) with only the
        qualifying rows (sel = their indices within the row group)."""
        if rg_end is None:
            rg_end = self.nrowgroups
        self.set_filter(filt)
        try:
            _check(_lib.fls_scan_begin(self.h, _mask(self, cols), rg_begin, rg_end))
            out = RowGroup()
            while _check(_lib.fls_scan_next(self.h, C.byref(out))) == 1:
                if out.sel:
                    sel = np.ctypeslib.as_array(out.sel, shape=(out.nrows,)).copy() if out.nrows else \
                        np.zeros(0, np.uint32)
                else:
                    sel = np.arange(out.nrows, dtype=np.uint32)
                yield out.rowgroup, out.first_row, sel, self._rg_arrays(out)
        finally:
            self._clear_filter()

    def keyset(self, col: int, filt=None, form: int = KEYSET_AUTO) -> "KeySet":
        """The build side of a semi-join: the key set of the non-NULL values
        of one integer-like column (INT*, UINT*, BOOLEAN, DATE, DECIMAL of at
        most 64 bits) over the rows filt selects.  Use it as
        (col, "in_set", keyset) on this or another table of the same
        connection.  Built on the GPU (fls_keyset_from_scan: the selected keys
        are collected as bits over the range of the column's zone maps, and
        the set's build_info says what that took); where that range is too
        wide for the call (FlsError ERR_LIMIT), or with FLS_KEYSET_BUILD=host
        in the environment, from a filtered scan of the column on the host.
        The set is the same either way."""
        ci = self.column(col)
        if ci.type in STRING_TYPES or ci.type in (FLOAT, DOUBLE) or ci.out_bytes > 8:
            raise ValueError(f"keyset: column {col} ({TYPE_NAMES.get(ci.type, ci.type)}) is not integer-like")
        # (a DECIMAL wider than 64 bits is no key column of a filter term or of the device build)
        wide_decimal = ci.type == DECIMAL and ci.width > 18
        if os.environ.get("FLS_KEYSET_BUILD", "") != "host" and not wide_decimal:
            self.set_filter(filt or [])
            try:
                h, info = _P(), KeySetBuildInfo()
                _check(_lib.fls_keyset_from_scan(self.h, col, 0, self.nrowgroups, form, C.byref(h), C.byref(info)))
                return KeySet(h.value, self.conn, info)
            except FlsError as e:
                if e.code != ERR_LIMIT:
                    raise
            finally:
                self._clear_filter()
        terms = list(filt or []) + [(col, "is_not_null", None)]
        parts = [arrs[col].view(NP_DTYPE[ci.type]) for _, _, _, arrs in self.scan_filtered(terms, cols=[col])]
        vals = np.concatenate(parts) if parts else np.zeros(0, NP_DTYPE[ci.type])
        signed = ci.type in (INT8, INT16, INT32, INT64, DATE, DECIMAL)
        return self.conn.keyset(np.unique(vals), signed=signed, form=form)

    @staticmethod
    def _wide_decimal(cis) -> bool:
        # (a DECIMAL wider than 64 bits is no column of the device build)
        return any(ci.type == DECIMAL and ci.width > 18 for ci in cis)

    def _map_from_scan(self, call, key_col, value_col, filt, form):
        """The device build of keymap() / valuemap() under filt: (handle,
        MapBuildInfo), None where the call's gate sends the columns to the
        host route (ERR_LIMIT), or the FlsError of any other failure (for the
        caller to raise once the filter is cleared)."""
        self.set_filter(filt or [])
        try:
            h, info = _P(), MapBuildInfo()
            _check(call(self.h, key_col, value_col, 0, self.nrowgroups, form, C.byref(h), C.byref(info)))
            return h.value, info
        except FlsError as e:
            return None if e.code == ERR_LIMIT else e
        finally:
            self._clear_filter()

    def keymap(self, key_col: int, value_col: int, filt=None, form: int = KEYMAP_AUTO) -> "KeyMap":
        """The build side of a join: the key map key_col -> value_col of two
        integer-like columns of this (dimension) table over the rows filt
        selects; rows with a NULL in either column are left out.  A value
        outside [0, 65534] raises ValueError (also where a key has two values
        as well), a key with two different values raises.  Use it as ("map", col, keymap) in aggregate_grouped on this
        or another table of the same connection.  Built on the GPU
        (fls_keymap_from_scan: the selected pairs are collected in an array
        over the range of the key column's zone maps and compacted there; the
        map's build_info says what that took); where the call's gate refuses
        the columns (FlsError ERR_LIMIT), or with FLS_KEYMAP_BUILD=host in the
        environment, from a filtered scan of both columns on the host.  The
        map is the same either way."""
        cis = [self.column(c) for c in (key_col, value_col)]
        for c, ci in zip((key_col, value_col), cis):
            if ci.type in STRING_TYPES or ci.type in (FLOAT, DOUBLE) or ci.out_bytes > 8:
                raise ValueError(f"keymap: column {c} ({TYPE_NAMES.get(ci.type, ci.type)}) is not integer-like")
        if os.environ.get("FLS_KEYMAP_BUILD", "") != "host" and not self._wide_decimal(cis):
            got = self._map_from_scan(_lib.fls_keymap_from_scan, key_col, value_col, filt, form)
            if isinstance(got, FlsError):
                m = re.search(r"value (-?\d+) of column \d+ is outside \[0, 65534\]", got.msg)
                if m:
                    raise ValueError(f"keymap: value {int(m.group(1))} of column {value_col} is outside [0, 65534]")
                # a key with two values: the host route below checks the values' range over every
                # selected row first, so columns that hold both faults raise what they always raised
                if not (got.code == ERR_ARG and "a map is a function" in got.msg):
                    raise got
            elif got is not None:
                return KeyMap(got[0], self.conn, got[1])
        terms = list(filt or []) + [(key_col, "is_not_null", None), (value_col, "is_not_null", None)]
        ks, vs = [], []
        for _, _, _, arrs in self.scan_filtered(terms, cols=sorted({key_col, value_col})):
            ks.append(arrs[key_col].view(NP_DTYPE[cis[0].type]))
            vs.append(arrs[value_col].view(NP_DTYPE[cis[1].type]))
        keys = np.concatenate(ks) if ks else np.zeros(0, NP_DTYPE[cis[0].type])
        vals = np.concatenate(vs) if vs else np.zeros(0, NP_DTYPE[cis[1].type])
        if vals.size and (int(vals.min()) < 0 or int(vals.max()) >= KEYMAP_ABSENT):
            bad = int(vals.min()) if int(vals.min()) < 0 else int(vals.max())
            raise ValueError(f"keymap: value {bad} of column {value_col} is outside [0, 65534]")
        signed = cis[0].type in (INT8, INT16, INT32, INT64, DATE, DECIMAL)
        return self.conn.keymap(keys, vals.astype(np.uint16), signed=signed, form=form)

    def valuemap(self, key_col: int, value_col: int, filt=None, form: int = VALUEMAP_AUTO) -> "ValueMap":
        """The build side of a join: the value map key_col -> value_col of two
        integer-like columns of this (dimension) table over the rows filt
        selects; rows with a NULL in either column are left out, and a key
        with two different values raises.  Use it as
        (a, op, Mapped(col, valuemap)) on this or another table of the same
        connection.  Built on the GPU like keymap() (fls_valuemap_from_scan;
        the map's build_info says what that took); where the call's gate
        refuses the columns (FlsError ERR_LIMIT), or with
        FLS_VALUEMAP_BUILD=host in the environment, from a filtered scan of
        both columns on the host.  The map is the same either way."""
        cis = [self.column(c) for c in (key_col, value_col)]
        for c, ci in zip((key_col, value_col), cis):
            if ci.type in STRING_TYPES or ci.type in (FLOAT, DOUBLE) or ci.out_bytes > 8:
                raise ValueError(f"valuemap: column {c} ({TYPE_NAMES.get(ci.type, ci.type)}) is not integer-like")
        if os.environ.get("FLS_VALUEMAP_BUILD", "") != "host" and not self._wide_decimal(cis):
            got = self._map_from_scan(_lib.fls_valuemap_from_scan, key_col, value_col, filt, form)
            if isinstance(got, FlsError):
                raise got
            if got is not None:
                return ValueMap(got[0], self.conn, got[1])
        terms = list(filt or []) + [(key_col, "is_not_null", None), (value_col, "is_not_null", None)]
        ks, vs = [], []
        for _, _, _, arrs in self.scan_filtered(terms, cols=sorted({key_col, value_col})):
            ks.append(arrs[key_col].view(NP_DTYPE[cis[0].type]))
            vs.append(arrs[value_col].view(NP_DTYPE[cis[1].type]))
        keys = np.concatenate(ks) if ks else np.zeros(0, NP_DTYPE[cis[0].type])
        vals = np.concatenate(vs) if vs else np.zeros(0, NP_DTYPE[cis[1].type])
        sg = (INT8, INT16, INT32, INT64, DATE, DECIMAL)
        return self.conn.valuemap(keys, vals, signed=cis[0].type in sg, value_signed=cis[1].type in sg, form=form)

    def set_key_bindings(self, bindings):
        """fls_aggregate_key_bindings: what a key KEY_MAPPED | i names in the
        following aggregate_grouped calls; each binding (col, keymap) or
        (col, keymap, flags), keymap a KeyMap or a raw handle.  [] or None
        clears."""
        bindings = bindings or []
        arr = (KeyBinding * max(1, len(bindings)))()
        for i, b in enumerate(bindings[:len(arr)]):
            arr[i].col = b[0]
            arr[i].map = (b[1].h or 0) if isinstance(b[1], KeyMap) else int(b[1])
            arr[i].flags = b[2] if len(b) > 2 else 0
        _check(_lib.fls_aggregate_key_bindings(self.h, arr if bindings else None, len(bindings)))

    def set_aggregate_value_bindings(self, bindings):
        """fls_aggregate_value_bindings: what COL_MAPPED | i names in the
        following aggregate calls (an operand, a sum_expr factor, a key of
        aggregate_hashed); each binding a Mapped, or (col, valuemap) /
        (col, valuemap, flags) with valuemap a ValueMap or a raw handle.  [] or
        None clears.  What a Mapped in a call's aggs or keys sets and clears
        per call."""
        bindings = bindings or []
        arr = (ValueBinding * max(1, len(bindings)))()
        for i, b in enumerate(bindings[:len(arr)]):
            if isinstance(b, Mapped):
                b = (b.key_col, b.valuemap, VALUEMAP_KEEP_UNMATCHED if b.keep_unmatched else 0)
            arr[i].col = b[0]
            arr[i].map = (b[1].h or 0) if isinstance(b[1], ValueMap) else int(b[1])
            arr[i].flags = b[2] if len(b) > 2 else 0
        _check(_lib.fls_aggregate_value_bindings(self.h, arr if bindings else None, len(bindings)))
        # how each binding's values extend, for a raw COL_MAPPED | i key of aggregate_hashed (the handles are live here)
        self._vbind_signed = []
        for i in range(len(bindings)):
            info = ValueMapInfo()
            _check(_lib.fls_valuemap_info(arr[i].map, C.byref(info)))
            self._vbind_signed.append(info.value_kind == KIND_SIGNED)

    # -- aggregates reduced on the GPU
    def set_aggregate_exprs(self, exprs):
        """fls_aggregate_exprs: the expression list function code 6 (sum_expr)
        indexes in the following aggregate calls; each expression a list of 1
        to 3 (k, sign, col) factors k + sign * column.  [] or None clears."""
        exprs = exprs or []
        _check(_lib.fls_aggregate_exprs(self.h, _agg_exprs(exprs) if exprs else None, len(exprs)))

    def set_aggregate_conditions(self, conds):
        """fls_aggregate_conditions: the condition list an aggregate spec's
        cond = i + 1 indexes in the following aggregate calls (what When sets
        and clears per call); each condition a filter as scan_filtered takes
        it, at most 8.  [] or None clears."""
        conds = conds or []
        preds, k, ranges, n, _parts = self._pack_lists(conds, AggCondition)
        _check(_lib.fls_aggregate_conditions(self.h, preds if k else None, k, ranges if conds else None, n))

    def aggregate_raw(self, aggs, rg_begin=0, rg_end=None) -> list[AggregateValue]:
        """fls_aggregate under the filter currently set (set_filter): the raw
        fls_aggregate_value records.  aggs as for aggregate(); a first element
        that is an int is passed through as the function code (code 6 then
        indexes the list set by set_aggregate_exprs).  ("sum_expr", [...])
        items replace that list for the call and clear it afterwards."""
        if rg_end is None:
            rg_end = self.nrowgroups
        vbinds = []
        arr, exprs, conds = _agg_specs(aggs, vbinds)
        out = (AggregateValue * max(1, len(aggs)))()
        try:
            if vbinds:   # (before the expressions, whose factors name them)
                self.set_aggregate_value_bindings(vbinds)
            if exprs:
                self.set_aggregate_exprs(exprs)
            if conds:
                self.set_aggregate_conditions(conds)
            _check(_lib.fls_aggregate(self.h, arr, len(aggs), rg_begin, rg_end, out))
        finally:
            if exprs:
                self.set_aggregate_exprs(None)
            if conds:
                self.set_aggregate_conditions(None)
            if vbinds:
                self.set_aggregate_value_bindings(None)
        return list(out)[:len(aggs)]

    def aggregate(self, aggs, filt=None, rg_begin=0, rg_end=None) -> list:
        """Ungrouped aggregates evaluated on the GPU (fls_aggregate).  aggs: a
        list of ("count",) [count(*)], ("count", col), ("sum", col),
        ("min", col), ("max", col), ("sum_product", a, b),
        ("sum_expr", [(k, sign, col), ...]) [the exact integer sum of the
        product of 1 to 3 factors k + sign * col, sign +1 or -1, k in the
        column's physical unit], or When(agg, cond) [agg FILTER (WHERE cond):
        any of these over the rows of the call's filter where cond, a filter of
        its own, holds too]; filt as scan_filtered takes it.  Returns per aggregate an int (counts, integer
        sums at full 128-bit precision, integer MIN / MAX), a float (FLOAT /
        DOUBLE sums, MIN, MAX) or None (SUM / MIN / MAX over no row)."""
        self.set_filter(filt)
        try:
            vals = self.aggregate_raw(aggs, rg_begin, rg_end)
        finally:
            self._clear_filter()
        return [_agg_value(v) for v in vals]

    def aggregate_grouped(self, keys, aggs, filt=None, rg_begin=0, rg_end=None) -> list:
        """GROUP BY keys (1 to 4 of low cardinality) of the aggregates
        aggregate() takes, evaluated on the GPU (fls_aggregate_grouped).  A
        key is a column index, or ("map", col, keymap) /
        ("map", col, keymap, "keep_unmatched"): the code keymap gives column
        col -- an inner join by default (rows whose value is NULL or not in
        the map belong to no group), a left join with "keep_unmatched" (they
        form the NULL group).  An int with KEY_MAPPED set is passed through
        and names a binding set by set_key_bindings.  Returns
        [(key_tuple, values)] in order of each group's first row; a key
        element is an int (a mapped key: its code), bytes (a VARCHAR key) or
        None (NULL, a group of its own), values as aggregate() returns them.
        FlsError with code ERR_LIMIT past 64 distinct keys in a 1024-row
        vector or 256 in a row group."""
        if rg_end is None:
            rg_end = self.nrowgroups
        raw, binds = [], []
        for k in keys:
            if isinstance(k, Mapped):
                raise ValueError(f"aggregate_grouped: key {k!r}: a Mapped is a key of aggregate_hashed; a "
                                 'low-cardinality mapped key here is ("map", col, keymap) over a KeyMap')
            if isinstance(k, (tuple, list)):
                if len(k) not in (3, 4) or k[0] != "map" or (len(k) == 4 and k[3] != "keep_unmatched"):
                    raise ValueError(f"aggregate_grouped: key {k!r} is not a column or "
                                     '("map", col, keymap[, "keep_unmatched"])')
                raw.append(KEY_MAPPED | len(binds))
                binds.append((k[1], k[2], KEYMAP_KEEP_UNMATCHED if len(k) == 4 else 0))
            else:
                raw.append(k)
        karr = (C.c_uint32 * max(1, len(raw)))(*raw[:max(1, len(raw))])
        vbinds = []
        arr, exprs, conds = _agg_specs(aggs, vbinds)
        res = _P()
        self.set_filter(filt)
        try:
            if vbinds:   # (before the expressions, whose factors name them)
                self.set_aggregate_value_bindings(vbinds)
            if exprs:
                self.set_aggregate_exprs(exprs)
            if conds:
                self.set_aggregate_conditions(conds)
            if binds:
                self.set_key_bindings(binds)
            _check(_lib.fls_aggregate_grouped(self.h, karr, len(keys), arr, len(aggs), rg_begin, rg_end,
                                              C.byref(res)))
        finally:
            self._clear_filter()
            if exprs:
                self.set_aggregate_exprs(None)
            if conds:
                self.set_aggregate_conditions(None)
            if binds:
                self.set_key_bindings(None)
            if vbinds:
                self.set_aggregate_value_bindings(None)
        try:
            out = []
            k = GroupKey()
            for g in range(_lib.fls_group_result_ngroups(res)):
                key = []
                for q in range(len(keys)):
                    _check(_lib.fls_group_result_key(res, g, q, C.byref(k)))
                    if k.kind == KEYV_NULL:
                        key.append(None)
                    elif k.kind == KEYV_STRING:
                        key.append(C.string_at(k.str, k.str_len) if k.str_len else b"")
                    else:
                        x = (k.hi << 64) | k.lo
                        key.append(x - (1 << 128) if x >> 127 else x)
                vals = _lib.fls_group_result_values(res, g)
                out.append((tuple(key), [_agg_value(vals[i]) for i in range(len(aggs))]))
            return out
        finally:
            _lib.fls_group_result_free(res)

    @staticmethod
    def _group_select(having, order_by, limit):
        """the fls_group_select of aggregate_hashed's having / order_by / limit
        (and the array it points into, which must outlive the call)"""
        terms = (GroupHaving * max(1, len(having or ())))()
        for j, (agg, op, value) in enumerate(having or ()):
            if isinstance(op, str) and op not in ("=", "==", "!=", "<>", "<", "<=", ">", ">="):
                raise ValueError(f"aggregate_hashed: having {j}: op {op!r} is not one of = != < <= > >=")
            terms[j].agg, terms[j].op = agg, OPS[op] if isinstance(op, str) else op   # (an int: the code itself)
            if isinstance(value, float):
                terms[j].kind = AGGV_DOUBLE
                terms[j].lo = int(np.array([value], dtype=np.float64).view(np.uint64)[0])
            else:
                x = int(value)
                if not -(1 << 127) <= x < (1 << 127):
                    raise ValueError(f"aggregate_hashed: having {j}: {x} is no 128-bit integer")
                terms[j].kind = AGGV_INT
                terms[j].lo, terms[j].hi = x & (2**64 - 1), (x >> 64) & (2**64 - 1)
        sel = GroupSelect(having=terms, nhaving=len(having or ()), order_agg=GROUP_ORDER_NONE, limit=limit or 0)
        if order_by is not None:
            ob = tuple(order_by) if isinstance(order_by, (tuple, list)) else (order_by,)
            if (not 1 <= len(ob) <= 3 or (len(ob) > 1 and ob[1] not in ("asc", "desc"))
                    or (len(ob) > 2 and ob[2] != "nulls_first")):
                raise ValueError(f"aggregate_hashed: order_by {order_by!r} is not agg_index, (agg_index, "
                                 '"asc" | "desc") or (agg_index, "asc" | "desc", "nulls_first")')
            sel.order_agg = ob[0]
            sel.desc = int(len(ob) > 1 and ob[1] == "desc")
            sel.nulls_first = int(len(ob) > 2)
        return sel, terms

    def aggregate_hashed(self, keys, aggs, max_groups: int, filt=None, rg_begin=0, rg_end=None, having=None,
                         order_by=None, limit=None) -> HashGroups:
        """GROUP BY keys (1 to 4 integer-like columns of any cardinality up to
        max_groups) of the aggregates aggregate() takes, except FLOAT / DOUBLE
        sums, in a hash table in HBM (fls_aggregate_hashed): the call for
        GROUP BY l_orderkey, which aggregate_grouped refuses.  Returns a
        HashGroups of numpy arrays in unspecified order; its
        to_list() is aggregate_grouped's list.  The packed key (per key the
        bits of its zone maps' max - min over the range, plus a NULL bit)
        holds at most 63 bits.  FlsError with code ERR_LIMIT when one
        pipeline's row groups hold more than max_groups distinct keys among
        the selected rows: call again with a larger max_groups (each pipeline
        allocates the next power of two >= 2 * max_groups slots).
        having / order_by / limit choose among the groups on the GPU
        (fls_aggregate_hashed_select), so that only the chosen ones come back:
        having is a list of (agg_index, op, value), all of which must hold,
        op one of "=", "!=", "<", "<=", ">", ">=", value an int of up to 128
        bits, or a float against a FLOAT / DOUBLE MIN / MAX (a NULL aggregate
        satisfies no term); order_by is agg_index, (agg_index, "desc" | "asc")
        or (agg_index, "desc" | "asc", "nulls_first") and needs a limit of 1
        to 1024; ties go to the smaller first row, NULLs last by default; a
        limit alone gives the first groups by first row.  With an order_by or
        a limit the HashGroups and its to_list() are in result order.  With
        all three None the plain call is made."""
        if rg_end is None:
            rg_end = self.nrowgroups
        vbinds = []
        raw = [_mapped_col(k, vbinds) for k in keys]   # a Mapped key: COL_MAPPED | its value binding
        karr = (C.c_uint32 * max(1, len(raw)))(*raw[:max(1, len(raw))])
        arr, exprs, conds = _agg_specs(aggs, vbinds)
        res = _P()
        select = having is not None or order_by is not None or limit is not None
        if select:
            sel, terms = self._group_select(having, order_by, limit)
        self.set_filter(filt)
        try:
            if vbinds:   # (before the expressions, whose factors name them)
                self.set_aggregate_value_bindings(vbinds)
            if exprs:
                self.set_aggregate_exprs(exprs)
            if conds:
                self.set_aggregate_conditions(conds)
            vsigned = list(self._vbind_signed)   # (of the bindings in force for this call)
            if select:
                _check(_lib.fls_aggregate_hashed_select(self.h, karr, len(keys), arr, len(aggs), max_groups,
                                                        C.byref(sel), rg_begin, rg_end, C.byref(res)))
            else:
                _check(_lib.fls_aggregate_hashed(self.h, karr, len(keys), arr, len(aggs), max_groups, rg_begin,
                                                 rg_end, C.byref(res)))
        finally:
            self._clear_filter()
            if exprs:
                self.set_aggregate_exprs(None)
            if conds:
                self.set_aggregate_conditions(None)
            if vbinds:
                self.set_aggregate_value_bindings(None)
        try:
            # (a mapped key extends by its map's value kind: a raw COL_MAPPED | i key by what the setter recorded)
            signed = [vsigned[r & ~COL_MAPPED] if r & COL_MAPPED else
                      self.column(r).type in (INT8, INT16, INT32, INT64, DATE, DECIMAL) for r in raw]
            return HashGroups(res, signed, len(aggs), in_result_order=order_by is not None or bool(limit))
        finally:
            _lib.fls_hash_result_free(res)

    # -- ORDER BY key LIMIT k selected on the GPU
    def topn_pruned(self, order_by: int, k: int, desc=False, nulls_first=False, rg_begin=0, rg_end=None) -> int:
        """fls_topn_pruned (host only): the row groups topn() with these
        arguments would not read under the filter currently set (set_filter)"""
        if rg_end is None:
            rg_end = self.nrowgroups
        key = OrderKey(col=order_by, desc=int(bool(desc)), nulls_first=int(bool(nulls_first)))
        return _check(_lib.fls_topn_pruned(self.h, C.byref(key), k, rg_begin, rg_end))

    def topn(self, order_by: int, k: int, cols=None, filt=None, desc=False, nulls_first=False, rg_begin=0,
             rg_end=None):
        """The k best rows (k <= MAX_TOPN) ordered by column order_by, selected
        on the GPU (fls_topn): ascending or desc, NULL keys last or
        nulls_first, equal keys by row index; filt as scan_filtered takes it.
        Returns (rows, values, valid): rows the winners' global row indices
        (uint64) in result order; values[c] for each delivered column (cols,
        None = all) a numpy array in NP_DTYPE or a list of bytes for VARCHAR /
        BLOB, None for the others; valid[c] a bool array (False = NULL) or
        None when every returned row is valid.  Everything is a copy.
        self.topn_ms holds the call's (phase 1, phase 2) host-clock times."""
        if rg_end is None:
            rg_end = self.nrowgroups
        key = OrderKey(col=order_by, desc=int(bool(desc)), nulls_first=int(bool(nulls_first)))
        res = _P()
        self.set_filter(filt)
        try:
            _check(_lib.fls_topn(self.h, C.byref(key), k, _mask(self, cols), rg_begin, rg_end, C.byref(res)))
        finally:
            self._clear_filter()
        try:
            p1, p2 = C.c_double(), C.c_double()
            _check(_lib.fls_topn_result_times(res, C.byref(p1), C.byref(p2)))
            self.topn_ms = (p1.value, p2.value)   # the last call's phase 1 / phase 2, host clock
            n = _lib.fls_topn_result_nrows(res)
            rows = np.ctypeslib.as_array(_lib.fls_topn_result_rows(res), shape=(n,)).copy() if n else \
                np.zeros(0, np.uint64)
            sch = self.schema()
            values, valid = [None] * len(sch), [None] * len(sch)
            for c in (range(len(sch)) if cols is None else cols):
                ty, ob = sch[c][1], sch[c][4]
                pv, pw = _P(), C.POINTER(C.c_uint64)()
                _check(_lib.fls_topn_result_column(res, c, C.byref(pv), C.byref(pw)))
                raw = np.ctypeslib.as_array(C.cast(pv, C.POINTER(C.c_uint8)), shape=(n * ob,)).copy() if n else \
                    np.zeros(0, np.uint8)
                if pw and n:
                    w = np.ctypeslib.as_array(pw, shape=((n + 63) // 64,))
                    valid[c] = np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)
                if ty in STRING_TYPES:
                    strs = string_t_decode(raw)
                    if valid[c] is not None:
                        strs = [s if ok else b"" for s, ok in zip(strs, valid[c])]
                    values[c] = strs
                else:
                    values[c] = raw.view(NP_DTYPE[ty])
            return rows, values, valid
        finally:
            _lib.fls_topn_result_free(res)

    # -- device-resident decode (bench)
    def device_upload(self, rg_begin=0, rg_end=None):
        if rg_end is None:
            rg_end = self.nrowgroups
        _check(_lib.fls_device_upload(self.h, rg_begin, rg_end))

    def device_decode(self, cols=None):
        _check(_lib.fls_device_decode(self.h, _mask(self, cols)))

    def device_sync(self) -> DecodeStats:
        st = DecodeStats()
        _check(_lib.fls_device_sync(self.h, C.byref(st)))
        return st

    def device_column(self, c: int):
        p, n = _P(), C.c_uint64()
        _check(_lib.fls_device_column(self.h, c, C.byref(p), C.byref(n)))
        return p.value, n.value

    def device_parts(self) -> list[PartInfo]:
        """The resident parts: one per GPU holding row groups (device_upload
        splits the range over the connection's GPUs)."""
        out = []
        for i in range(_lib.fls_device_parts(self.h)):
            pi = PartInfo()
            _check(_lib.fls_device_part(self.h, i, C.byref(pi)))
            out.append(pi)
        return out

    def device_part_column(self, part: int, c: int):
        p, n = _P(), C.c_uint64()
        _check(_lib.fls_device_part_column(self.h, part, c, C.byref(p), C.byref(n)))
        return p.value, n.value

    @property
    def device_rows(self) -> int:
        return _lib.fls_device_rows(self.h)

    def device_copy_out(self, c: int, row: int = 0, n: int | None = None) -> np.ndarray:
        ob = self.column(c).out_bytes
        if n is None:
            n = self.device_rows - row
        buf = np.empty(n * ob, dtype=np.uint8)
        _check(_lib.fls_device_copy_out(self.h, c, row, n, buf.ctypes.data))
        return buf


def as_values(raw: np.ndarray, ty: int) -> np.ndarray:
    """View decoded raw bytes of an integer column as its numpy dtype."""
    return raw.view(NP_DTYPE[ty])


def string_t_decode(raw: np.ndarray) -> list[bytes]:
    """Decode DuckDB string_t records (host pointers dereferenced for >12 B)."""
    rec = raw.reshape(-1, 16)
    lens = rec[:, :4].copy().view(np.uint32).ravel()
    out = []
    for i in range(len(lens)):
        n = int(lens[i])
        if n <= 12:
            out.append(bytes(rec[i, 4:4 + n]))
        else:
            ptr = int(rec[i, 8:16].copy().view(np.uint64)[0])
            out.append(C.string_at(ptr, n))
    return out


# --- full-size GPU verification (libflscheck.so; tests / bench support) ------
_check_lib = None


def _checklib():
    global _check_lib
    if _check_lib is None:
        path = _HERE / "libflscheck.so"
        if not path.exists():
            raise ImportError(f"{path} not built")
        lib_ = C.CDLL(str(path))
        lib_.fls_check_workload.restype = C.c_int
        lib_.fls_check_workload.argtypes = [C.c_char_p, C.c_double, C.c_uint64, C.c_uint64, C.c_uint64,
                                            C.POINTER(_P), C.POINTER(C.c_uint8), C.c_int, C.POINTER(_P),
                                            C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
        lib_.fls_check_workload_on.restype = C.c_int
        lib_.fls_check_workload_on.argtypes = [C.c_int] + lib_.fls_check_workload.argtypes
        lib_.fls_check_last_error.restype = C.c_char_p
        _check_lib = lib_
    return _check_lib


def check_device_table(t: "Table", workload: str, scale: float = 1.0, nrows: int = 0) -> list[int]:
    """Mismatching rows per column of t's resident decoded columns vs the
    workload generator (computed on the GPU holding each resident part).
    Call after device_sync()."""
    lib_ = _checklib()
    nc = t.ncols
    total = gen_nrows(workload, scale, nrows)
    obs = (C.c_uint8 * nc)(*[t.column(c).out_bytes for c in range(nc)])
    dicts = (_P * nc)()
    keep = []
    for c in range(nc):
        if obs[c] == 16:
            words = []
            k = 0
            while (s := gen_dict_string(workload, c, k)) is not None:
                words.append(s.encode())
                k += 1
            if words:
                b = C.create_string_buffer(b"\0".join(words) + b"\0\0")
                keep.append(b)
                dicts[c] = C.cast(b, _P)
    mism_total = [0] * nc
    for i, part in enumerate(t.device_parts()):
        cols = (_P * nc)()
        deltas = (C.c_int64 * nc)()
        for c in range(nc):
            cols[c] = t.device_part_column(i, c)[0]
            dp, hp, hn = _P(), _P(), C.c_uint64()
            if obs[c] == 16 and _lib.fls_device_part_heap(t.h, i, c, C.byref(dp), C.byref(hp), C.byref(hn)) == 1:
                deltas[c] = (dp.value or 0) - (hp.value or 0)   # free text (FSST): no dictionary
        mism = (C.c_uint64 * nc)()
        rc = lib_.fls_check_workload_on(part.device, workload.encode(), scale, total, t.row_offset + part.first_row,
                                        part.nrows, cols, obs, nc, dicts, deltas, mism)
        if rc != 0:
            raise FlsError(rc, lib_.fls_check_last_error().decode())
        mism_total = [a + b for a, b in zip(mism_total, mism)]
    return mism_total
