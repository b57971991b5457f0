// fls_filter.hpp -- pushed-down scan filters (read_fastlanes filter_pushdown).
//
// The reference registers its scanner with filter_pushdown = false
// (src/scanner/scan_fastlanes.cpp:154), so DuckDB filters every decoded row on
// the CPU after the scan.  Here a filter is a conjunction of clauses, each a
// disjunction of terms `column <op> constant` -- the shape of DuckDB's
// TableFilterSet (ConstantFilter, ConjunctionAnd/Or, InFilter, IS [NOT] NULL).
// It is applied twice:
//   * on the host, per row group, against the footer zone maps and the DICT
//     dictionaries: row groups no row of which can qualify are never uploaded;
//   * on the GPU, per row, over the decoded batch in HBM (fls_filter.hip):
//     a selection mask, then only the qualifying rows of the delivered
//     columns are compacted and written to pinned host memory.
// The comparison semantics are DuckDB's, shared by both sides: signed /
// unsigned integers, IEEE floats with NaN equal to NaN and above every
// number and -0 == 0, strings compared bytewise (memcmp order, a proper
// prefix sorts first).  NULL rows (the chunks' validity bitmaps) satisfy
// IS NULL and no comparison, as in DuckDB; IS NOT NULL holds for the rest.
// A term may also test membership in a key set (`column IN set` / `NOT IN
// set`, fls_keyset.hpp): such a term is a clause of its own, pruned against
// the zone maps by the set's sorted keys and evaluated by a kernel of its own
// (fls_keyset.hip) that narrows the mask the filter kernel wrote.
// A string pattern term (`column LIKE pattern` / `NOT LIKE`, fls_strmatch.hpp)
// has the same shape: a clause of its own, pruned against the DICT
// dictionaries by the shared matcher and evaluated by strmatch_kernel
// (fls_strmatch.hip), which narrows the same mask after the key sets.
// A column term (`column op column` of the same row, OP_COL_EQ .. OP_COL_GE)
// is a clause of its own as well: pruned by comparing the two zone maps and
// evaluated by colcmp_kernel (fls_colcmp.hip), which narrows the mask right
// after filter_kernel -- two coalesced loads and a compare are cheaper than a
// probe or a string match, so the later kernels skip the words it empties.
// A filter may have alternatives (fls_scan_filter_alternatives): filters of
// this very shape of which at least one must hold beside it.  They prune a row
// group none of them can match, and on the GPU alt_kernel / alt_merge_kernel
// (fls_alt.hip) OR them into the mask the kernels above wrote.
// A map term (`column op map[key column]`, OP_MAP_EQ .. OP_MAP_GE,
// fls_valuemap.hpp) is a clause of its own too: pruned by the map's sorted
// keys and its value range against the two zone maps and evaluated by
// mapcmp_kernel (fls_mapcmp.hip), which narrows the mask after the key sets
// -- its 8-byte gather is the dearest probe, so it sees the fewest rows.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fls {

enum FilterKind : uint8_t {
    FK_INT = 0,    // signed integer (INT*, DATE days, DECIMAL scaled int64)
    FK_UINT = 1,   // unsigned integer
    FK_FLOAT = 2,  // FLOAT / DOUBLE, compared as double
    FK_STR = 3,    // VARCHAR (string_t records)
};
enum FilterOp : uint8_t {
    OP_EQ = 0, OP_NE = 1, OP_LT = 2, OP_LE = 3, OP_GT = 4, OP_GE = 5, OP_IS_NULL = 6, OP_IS_NOT_NULL = 7,
    OP_FALSE = 8,  // no row (col <op> NULL)
    // key-set membership (fls_keyset.hpp): a clause of its own, evaluated by
    // keyset_kernel after filter_kernel, never by eval_term
    OP_IN_SET = 9, OP_NOT_IN_SET = 10,
    // string patterns (fls_strmatch.hpp): a clause of its own, evaluated by
    // strmatch_kernel after keyset_kernel, never by eval_term
    OP_LIKE = 11, OP_NOT_LIKE = 12,
    // column against column: op - OP_COL_EQ is OP_EQ .. OP_GE; a clause of its
    // own, evaluated by colcmp_kernel after filter_kernel, never by eval_term
    OP_COL_EQ = 13, OP_COL_NE = 14, OP_COL_LT = 15, OP_COL_LE = 16, OP_COL_GT = 17, OP_COL_GE = 18,
    // column against the value a value map gives a key column of the same row
    // (fls_valuemap.hpp): op - OP_MAP_EQ is OP_EQ .. OP_GE; a clause of its
    // own, evaluated by mapcmp_kernel after keyset_kernel, never by eval_term
    OP_MAP_EQ = 19, OP_MAP_NE = 20, OP_MAP_LT = 21, OP_MAP_LE = 22, OP_MAP_GT = 23, OP_MAP_GE = 24
};

__host__ __device__ inline bool op_holds(uint8_t op, int c) {
    switch (op) {
    case OP_EQ: return c == 0;
    case OP_NE: return c != 0;
    case OP_LT: return c < 0;
    case OP_LE: return c <= 0;
    case OP_GT: return c > 0;
    case OP_GE: return c >= 0;
    case OP_IS_NULL: return false;
    case OP_FALSE: return false;
    default: return true;  // IS NOT NULL
    }
}

__host__ __device__ inline int cmp_int(int64_t a, int64_t b) { return a < b ? -1 : (a > b ? 1 : 0); }
__host__ __device__ inline int cmp_uint(uint64_t a, uint64_t b) { return a < b ? -1 : (a > b ? 1 : 0); }
// DuckDB float ordering: NaN == NaN, NaN > every number; -0 == 0
__host__ __device__ inline int cmp_float(double a, double b) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return na == nb ? 0 : (na ? 1 : -1);
    return a < b ? -1 : (a > b ? 1 : 0);
}
__host__ __device__ inline double as_double(uint64_t bits) {
    double d;
    __builtin_memcpy(&d, &bits, 8);
    return d;
}
// bytewise string comparison (DuckDB string_t ordering)
__host__ __device__ inline int cmp_bytes(const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb) {
    const uint32_t n = la < lb ? la : lb;
    for (uint32_t i = 0; i < n; ++i)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return la < lb ? -1 : (la > lb ? 1 : 0);
}

// A host address range the long strings (> 12 bytes) of a string column point
// into, and where its bytes are in HBM.  {0, 0, 0} holds no long string.
struct StrRange {             // 24 B
    uint64_t host_lo, host_hi;  // [host_lo, host_hi]: a string of len bytes at hp lies inside
                                // when host_lo <= hp and hp + len <= host_hi
    int64_t dev_delta;        // device address = host address + dev_delta
};

// One term of the filter as the kernel sees it, rebuilt per scan batch.
struct DevTerm {              // 96 B
    const uint8_t *col;       // decoded column of the batch in HBM (row 0 of the batch)
    const uint8_t *str;       // FK_STR: constant bytes in HBM
    uint64_t value;           // constant: int64 / uint64 / double bits
    // FK_STR: ENC_AUTO chooses DICT or FSST per chunk, so one batch can hold both;
    // a long string's pointer is accepted from either place
    StrRange heap;            // the batch's FSST heap of the column (FSST rows), or empty
    StrRange image;           // the uploaded part of the file image (DICT rows)
    uint32_t str_len;
    uint8_t kind, op, ob;     // FilterKind, FilterOp, bytes per decoded value
    uint8_t end_clause;       // 1 on the last term of a clause
    const uint64_t *valid;    // the column's validity words for the batch rows (HBM), or
                              // NULL when no row of the batch is NULL
    uint64_t pad;             // DevOut[] follows DevTerm[] in one buffer: keeps it 32-byte aligned
};
static_assert(sizeof(DevTerm) == 96, "DevTerm is 96 B");

// One delivered column of a filtered batch: qualifying rows of src (HBM) are
// compacted into dst (pinned host memory, written by the kernel over PCIe).
struct DevOut {               // 32 B
    const uint8_t *src;
    uint8_t *dst;
    uint32_t ob;
    uint32_t pad[3];
};
static_assert(sizeof(DevOut) == 32, "DevOut is 32 B");

enum : uint32_t { KERR_FILTER_STR = 16 };
// a narrowed column's decoded value outside [base, base + 2^(8 nw)): the zone
// maps the narrowing trusted do not bound the data (corrupt or foreign file)
enum : uint32_t { KERR_NARROW = 64 };

// Selection mask (one bit per row: 16 x u64 words per 1024-row vector) and
// per-vector counts for the nrows decoded rows of a batch.
hipError_t launch_filter(const DevTerm *d_terms, uint32_t nterms, uint32_t nrows, uint64_t *d_mask,
                         uint32_t *d_counts, uint32_t *d_err, hipStream_t stream);
// Compact the selected rows of nouts columns (and their row indices within
// their row group of rg_rows rows, into sel) in row order.
hipError_t launch_compact(const DevOut *d_outs, uint32_t nouts, const uint64_t *d_mask, const uint32_t *d_counts,
                          uint32_t nrows, uint32_t rg_rows, uint32_t *sel, hipStream_t stream);

// One key-set term (OP_IN_SET / OP_NOT_IN_SET) as keyset_kernel sees it,
// rebuilt per scan batch; the set's image (fls_keyset.hpp) lives in HBM with
// the set.  A row stays selected when its value is valid and in the set
// (negate: valid and not in it).
struct DevSetTerm {           // 64 B
    const uint8_t *col;       // decoded column of the batch in HBM (row 0 of the batch)
    const uint64_t *valid;    // as DevTerm::valid
    const uint64_t *table;    // bitmap words or hash slots
    uint64_t min, span;       // bitmap: bit (value - min) for value - min <= span
    uint64_t empty;           // hash: the empty slot's sentinel
    uint32_t cap_log2;        // hash: log2 of the capacity
    uint32_t max_probe;       // hash: slots a lookup examines at most
    uint8_t form;             // KS_BITMAP / KS_HASH
    uint8_t ob, sign;         // bytes per decoded value; values sign-extend to 64 bits
    uint8_t negate;           // NOT IN
    uint8_t pad[4];
};
static_assert(sizeof(DevSetTerm) == 64, "DevSetTerm is 64 B");
// a key-set descriptor no sound set produces (the probe loop itself is bounded)
enum : uint32_t { KERR_KEYSET = 512 };
// Narrows the mask and recomputes the counts launch_filter wrote for the same
// nrows rows (fls_keyset.hip).
hipError_t launch_keyset(const DevSetTerm *d_terms, uint32_t nterms, uint32_t nrows, uint64_t *d_mask,
                         uint32_t *d_counts, uint32_t *d_err, hipStream_t stream);

// The build of a key set from a scan (fls_keyset_from_scan) as
// keyset_build_kernel sees a batch: the selected, valid rows' keys of one
// column are collected as bits of a bitmap over [base, base + span] that the
// call's batches on one GPU share (bit d = key - base: bit d & 31 of dword
// d >> 5; span < 2^32, so the bitmap has span / 32 + 1 dwords at most 2^27).
struct DevKeyBuild {          // 56 B, a kernel argument
    const uint8_t *col;       // decoded column of the batch in HBM (row 0 of the batch)
    const uint64_t *valid;    // as DevTerm::valid
    const uint64_t *mask;     // the batch's selection mask, 16 words per vector
    uint32_t *bitmap;         // the collecting bitmap of the call on this GPU
    uint64_t base, span;
    uint32_t nrows;
    uint8_t ob, sign;         // bytes per decoded value; values sign-extend to 64 bits
    uint8_t window;           // clustered words go through the wave's LDS window (0: one global atomic per row)
    uint8_t pad;
};
static_assert(sizeof(DevKeyBuild) == 56, "DevKeyBuild is 56 B");
// a selected, valid key outside [base, base + span]: the zone maps that gave
// the range do not bound the data (corrupt or foreign file); it sets no bit
enum : uint32_t { KERR_KEYBUILD = 32768 };
// Collects the batch's keys into p.bitmap and writes per vector the rows that
// set a bit into d_counts (fls_keyset_build.hip).
hipError_t launch_keyset_build(const DevKeyBuild &p, uint32_t *d_counts, uint32_t *d_err, hipStream_t stream);

// The build of a value map or key map from a scan (fls_valuemap_from_scan,
// fls_keymap_from_scan) as mapbuild_kernel sees a batch: at every selected row
// where key and value are both valid, the value (in the value order,
// keyset_ord) goes into slot[key - base] of a collecting array over
// [base, base + span] that the call's batches on one GPU share.  slot has
// span + 4 entries, all ones before the first batch: span + 1 slots (span <
// 2^28) and, from slot[span + 1], the three cells one conflict records its
// key's d and the two values in (value order).
struct DevMapBuild {          // 72 B, a kernel argument
    const uint8_t *key;       // decoded key column of the batch in HBM (row 0 of the batch)
    const uint8_t *value;     // ... and the value column
    const uint64_t *vk, *vv;  // as DevTerm::valid, per column
    const uint64_t *mask;     // the batch's selection mask, 16 words per vector
    uint64_t *slot;           // the collecting array of the call on this GPU
    uint64_t base, span;
    uint32_t nrows;
    uint8_t obk, obv;         // bytes per decoded key / value
    uint8_t ksign, vsign;     // keys / values sign-extend to 64 bits; vsign: the value order is signed
};
static_assert(sizeof(DevMapBuild) == 72, "DevMapBuild is 72 B");
// a selected, valid key outside [base, base + span]: the zone maps that gave
// the range do not bound the data (corrupt or foreign file); it touches nothing
enum : uint32_t { KERR_MAPBUILD = 262144 };
// one key with two values among the call's rows on this GPU: no function
enum : uint32_t { KERR_MAPBUILD_CONFLICT = 524288 };
// Collects the batch's pairs into p.slot and writes per vector the rows that
// took part into d_counts (fls_mapbuild.hip).
hipError_t launch_mapbuild(const DevMapBuild &p, uint32_t *d_counts, uint32_t *d_err, hipStream_t stream);
// The compaction of a collecting array of n = span + 1 slots: one presence
// word per 64 slots into presence[(n + 63) / 64] and the present slots of
// each 1024-slot block counted into block_counts[(n + 1023) / 1024]; then,
// given the exclusive scan of those counts in block_offsets, the present
// slots' values (stored patterns again) in ascending slot order into
// out[0, nout).
hipError_t launch_mapbuild_presence(const uint64_t *slot, uint64_t n, uint64_t *presence, uint32_t *block_counts,
                                    hipStream_t stream);
hipError_t launch_mapbuild_gather(const uint64_t *slot, uint64_t n, const uint64_t *block_offsets, bool vsign,
                                  uint64_t *out, uint64_t nout, hipStream_t stream);

// One column term (OP_COL_EQ .. OP_COL_GE) as colcmp_kernel sees it, rebuilt
// per scan batch.  A row stays selected when both values are valid and
// `a op b` holds: op_holds(op, cmp_int | cmp_uint | cmp_float) over the values
// sign- (FK_INT) or zero-extended to 64 bits, a binary32 widened to binary64.
struct DevColTerm {           // 48 B
    const uint8_t *a, *b;     // the decoded left / right column of the batch in HBM (row 0 of the batch)
    const uint64_t *va, *vb;  // as DevTerm::valid, per side
    uint8_t oba, obb;         // bytes per decoded value: 1, 2, 4 or 8
    uint8_t kind;             // FK_INT / FK_UINT / FK_FLOAT, of both sides
    uint8_t op;               // OP_EQ .. OP_GE
    uint8_t f32a, f32b;       // FK_FLOAT: the side holds binary32 values (ob 4), else binary64 (ob 8)
    uint8_t pad[10];
};
static_assert(sizeof(DevColTerm) == 48, "DevColTerm is 48 B");
// a column-comparison descriptor no sound term produces (a width outside
// {1, 2, 4, 8}, a kind above FK_FLOAT, an op above OP_GE, binary32 flagged on
// an integer kind, a float side whose width does not fit its flag)
enum : uint32_t { KERR_COLCMP = 16384 };
// Narrows the mask and recomputes the counts launch_filter wrote for the same
// nrows rows (fls_colcmp.hip).
hipError_t launch_colcmp(const DevColTerm *d_terms, uint32_t nterms, uint32_t nrows, uint64_t *d_mask,
                         uint32_t *d_counts, uint32_t *d_err, hipStream_t stream);

// One map term (OP_MAP_EQ .. OP_MAP_GE) as mapcmp_kernel sees it, rebuilt per
// scan batch; the map's image (fls_valuemap.hpp) lives in HBM with the map.  A
// row stays selected when the left value and the key are valid, the key is in
// the map and `left op map[key]` holds: op_holds(op, cmp_int | cmp_uint) over
// the left value sign- (vsign) or zero-extended to 64 bits and the map's value.
// (DevMapTerm is the key maps' descriptor, fls_groupagg.hpp.)
struct DevMapCmpTerm {        // 80 B
    const uint8_t *a, *key;   // the decoded left / key column of the batch in HBM (row 0 of the batch)
    const uint64_t *va, *vk;  // as DevTerm::valid, per column
    const uint64_t *table;    // dense: values then presence words; hash: slots then values
    uint64_t min, span;       // dense: value (key - min) for key - min <= span
    uint64_t empty;           // hash: the empty slot's sentinel
    uint32_t cap_log2;        // hash: log2 of the capacity
    uint32_t max_probe;       // hash: slots a lookup examines at most
    uint8_t form;             // VM_DENSE / VM_HASH
    uint8_t oba, obk;         // bytes per decoded value: 1, 2, 4 or 8
    uint8_t ksign, vsign;     // keys / left values sign-extend to 64 bits; vsign: the comparison is signed
    uint8_t op;               // OP_EQ .. OP_GE
    uint8_t pad[2];
};
static_assert(sizeof(DevMapCmpTerm) == 80 && sizeof(DevMapCmpTerm) % 16 == 0, "DevMapCmpTerm is 80 B");
// a map-comparison descriptor no sound map produces (an unknown form, a width
// outside {1, 2, 4, 8}, an op above OP_GE, a dense span or a capacity past the
// format's limits, max_probe above the capacity)
enum : uint32_t { KERR_MAPCMP = 65536 };
// Narrows the mask and recomputes the counts launch_filter / launch_keyset
// wrote for the same nrows rows (fls_mapcmp.hip).
hipError_t launch_mapcmp(const DevMapCmpTerm *d_terms, uint32_t nterms, uint32_t nrows, uint64_t *d_mask,
                         uint32_t *d_counts, uint32_t *d_err, hipStream_t stream);

// One mapped column (fls_aggregate_value_bindings: map[key column] as an
// aggregate operand or a hash GROUP BY key) as mapval_kernel sees it, rebuilt
// per scan batch; the map's image (fls_valuemap.hpp) lives in HBM with the map.
// The kernel writes the map's value at every selected row whose key is valid
// and in the map into `out`, one uint64 per batch row, and the ballot of those
// rows into `ovalid`; the reduce kernels then read (out, 8 bytes, ovalid) as
// they read any column.  Both are DEFINED AT SELECTED ROWS ONLY: a 64-row word
// no row of which is selected is neither probed nor written.
struct DevMapValTerm {        // 80 B
    const uint8_t *key;       // the decoded key column of the batch in HBM (row 0 of the batch)
    const uint64_t *vk;       // as DevTerm::valid, of the key column
    const uint64_t *table;    // dense: values then presence words; hash: slots then values
    uint64_t *out;            // the derived column: one value per batch row (HBM)
    uint64_t *ovalid;         // the derived column's validity words, 16 per vector
    uint64_t min, span;       // dense: value (key - min) for key - min <= span
    uint64_t empty;           // hash: the empty slot's sentinel
    uint32_t cap_log2;        // hash: log2 of the capacity
    uint32_t max_probe;       // hash: slots a lookup examines at most
    uint8_t form;             // VM_DENSE / VM_HASH
    uint8_t obk;              // bytes per decoded key: 1, 2, 4 or 8
    uint8_t ksign;            // keys sign-extend to 64 bits
    uint8_t keep;             // keep-unmatched (left join): the mask is left alone
    uint8_t pad[4];
};
static_assert(sizeof(DevMapValTerm) == 80 && sizeof(DevMapValTerm) % 16 == 0, "DevMapValTerm is 80 B");
// a mapped-column descriptor no sound map produces (an unknown form, a key
// width outside {1, 2, 4, 8}, a dense span or a capacity past the format's
// limits, max_probe above the capacity)
enum : uint32_t { KERR_MAPVAL = 131072 };
// Probes the bindings' maps under the mask the filter's kernels wrote for the
// same nrows rows, writes the derived columns, narrows the mask by the inner
// bindings and recomputes the counts (fls_mapval.hip).
hipError_t launch_mapval(const DevMapValTerm *d_terms, uint32_t nterms, uint32_t nrows, uint64_t *d_mask,
                         uint32_t *d_counts, uint32_t *d_err, hipStream_t stream);

// One pattern term (OP_LIKE / OP_NOT_LIKE) as strmatch_kernel sees it, rebuilt
// per scan batch; the tokens (fls_strmatch.hpp) follow the descriptors in one
// buffer.  A row stays selected when its string is valid and matches (negate:
// valid and does not match).
struct DevPatTerm {           // 96 B
    const uint8_t *col;       // decoded string_t column of the batch in HBM (row 0 of the batch)
    const uint64_t *valid;    // as DevTerm::valid
    StrRange heap;            // as DevTerm::heap
    StrRange image;           // as DevTerm::image
    const uint16_t *tok;      // the compiled pattern in HBM
    uint32_t ntok;
    uint32_t min_len;         // a shorter string cannot match
    uint32_t prefix;          // the literal prefix's first prefix_len bytes, as a record's inline prefix word holds them
    uint8_t prefix_len;       // 0..4
    uint8_t negate;           // NOT LIKE
    uint8_t exact;            // no wildcard: a string longer than ntok cannot match
    uint8_t pad[9];
};
static_assert(sizeof(DevPatTerm) == 96 && sizeof(DevPatTerm) % 32 == 0, "DevPatTerm is 96 B");
// a pattern descriptor no sound pattern produces (ntok > 256, a token above
// 257, an inline prefix length above 4, tokens past the staged LDS)
enum : uint32_t { KERR_PATTERN = 8192 };
// Narrows the mask and recomputes the counts launch_filter / launch_keyset
// wrote for the same nrows rows (fls_strmatch.hip).  total_tokens: the sum of
// the terms' ntok, which sizes the launch's LDS.
hipError_t launch_strmatch(const DevPatTerm *d_terms, uint32_t nterms, uint32_t total_tokens, uint32_t nrows,
                           uint64_t *d_mask, uint32_t *d_counts, uint32_t *d_err, hipStream_t stream);

// The conditions of a call's aggregates (fls_aggregate_conditions) as
// cond_kernel sees them: condition c's ordinary terms are terms[first[c] ..
// first[c + 1]), the last term of each clause marked end_clause (a condition
// without ordinary terms has an empty range: its plane is the scan's mask).
constexpr uint32_t kMaxConds = 8;
struct CondList {
    uint32_t first[kMaxConds + 1];
    uint32_t n;
};
// One plane per condition, d_planes[c * 16 * nvec + 16 * v + word] =
// mask word & condition c over the word's rows, for the nrows decoded rows of
// a batch (nvec = its 1024-row vectors); d_mask as launch_aggregate takes it
// (nullptr: every row below nrows).  One launch for all conditions
// (fls_cond.hip).
hipError_t launch_conditions(const DevTerm *d_terms, const CondList &conds, uint32_t nrows, const uint64_t *d_mask,
                             uint64_t *d_planes, uint32_t *d_err, hipStream_t stream);

// The alternatives of a filter (fls_scan_filter_alternatives) as alt_kernel
// sees them: alternative a's ordinary terms are terms[first[a] .. first[a + 1])
// as in CondList (an empty range: the alternative starts from the mask); bit a
// of `closed` is set when no key-set, column-pair, map or pattern term follows.
struct AltList {
    uint32_t first[kMaxConds + 1];
    uint32_t n;
    uint32_t closed;
};
// The first step (fls_alt.hip): d_mask, which the filter's kernels wrote for
// the nrows decoded rows of a batch, becomes mask & (OR of the closed
// alternatives) with its per-vector counts in d_counts; an open alternative
// a's `mask & ordinary terms` goes to d_planes[a * 16 * nvec + 16 * v + word]
// for the narrowing kernels.  One launch for all alternatives.
hipError_t launch_alternatives(const DevTerm *d_terms, const AltList &alts, uint32_t nrows, uint64_t *d_mask,
                               uint64_t *d_planes, uint32_t *d_counts, uint32_t *d_err, hipStream_t stream);
// The last step, after the open planes were narrowed: d_mask |= the open
// alternatives' planes, and d_counts again.  No launch without an open one.
hipError_t launch_alt_merge(const AltList &alts, uint32_t nrows, uint64_t *d_mask, const uint64_t *d_planes,
                            uint32_t *d_counts, hipStream_t stream);

// Narrowed delivery (fls_scan_narrow): an integer column of a batch whose
// values, per row group, lie in [base, base + 2^(8 nw)) crosses PCIe as the
// nw-byte differences value - base (the host adds the base back).  Reads ob
// bytes and writes nw per row: HBM-side work that saves (ob - nw) bytes of
// PCIe per row.
struct DevNarrow {            // 32 B
    const uint8_t *src;       // decoded column of the batch (HBM, ob bytes per row)
    uint8_t *dst;             // narrowed copy (HBM, nw bytes per row)
    const uint64_t *base;     // per row group of the batch (row / rg_rows): the value subtracted
    uint8_t ob, nw, sign;     // widths; sign: values sign-extend from ob bytes
    uint8_t pad[5];
};
static_assert(sizeof(DevNarrow) == 32, "DevNarrow is 32 B");
hipError_t launch_narrow(const DevNarrow *d_cols, uint32_t ncols, uint32_t nrows, uint32_t rg_rows,
                         uint32_t *d_err, hipStream_t stream);

// Delivery of a batch's decoded columns and string heaps into pinned host
// memory by a copy kernel (FLS_SCAN_COPY_KERNEL, default 1) instead of the DMA engines: a
// hipMemcpy D2H ran 57.1 GB/s in some processes and 30.2 in others on one box (link at 32 GT/s x16 throughout), a copy kernel 54.7 in
// every process (profiles/r6/d2h_probe_r6an.txt).  Both pointers of a copy
// are 16-byte aligned (the caller sends the others through hipMemcpyAsync);
// up to kHostCopyMax copies per launch, passed by value.
struct HostCopy {
    const uint8_t *src;  // HBM or pinned host memory
    uint8_t *dst;        // the other
    uint64_t bytes;
};
constexpr uint32_t kHostCopyMax = 40;
constexpr uint32_t kHostCopyPiece = 64u << 10;  // bytes per block iteration
struct HostCopyList {
    HostCopy c[kHostCopyMax];
    uint32_t first[kHostCopyMax + 1];  // first piece of each copy; first[n] = total pieces
    uint32_t n;
};
hipError_t launch_host_copy(const HostCopy *copies, uint32_t n, hipStream_t stream);

}  // namespace fls
