/*
 * flsgpu.h -- C-ABI of the MI355X FastLanes decode engine (libflsgpu.so).
 *
 * This is the seam the reference's FastLanesFacade::Impl
 * (src/fastlanes_facade.cpp:12-20) crosses into its decode library.  Each
 * entry point names the cwida/FastLanes call it replaces:
 *
 *   fls_connect            fastlanes::connect()                src/fastlanes_facade.cpp:33
 *   fls_read_fls           Connection::read_fls(path)          src/fastlanes_facade.cpp:34
 *   fls_table_nrows/...    Rowgroup::RowCount()/ColCount()     src/fastlanes_facade.cpp:52-56,85
 *   fls_table_column       Rowgroup::internal_rowgroup[c] type src/fastlanes_facade.cpp:112-183
 *                          (typed schema: ext_fastlane::FastLanesFacade::
 *                          getColumnTypes/getColumnNames,
 *                          src/include/fastlanes_facade.hpp:34-35)
 *   fls_materialize        TableReader::get_rowgroup_reader(rg)
 *                          + RowgroupReader::materialize()     src/fastlanes_facade.cpp:41,48
 *   fls_scan_begin/next    the row-group loop the reference never wrote
 *                          (it decodes row group 0 only, :41)
 *   fls_scan_acquire/release  the same loop for a parallel DuckDB scan
 *                          (MaxThreads > 1, batch index = row group; the
 *                          reference pins MaxThreads to 1,
 *                          src/scanner/scan_fastlanes.cpp:43-45)
 *   fls_table_close/fls_disconnect  FastLanesFacade::closeFile  src/fastlanes_facade.cpp:202-210
 *
 * Conventions: plain pointers and sizes, no exceptions across the ABI; every
 * function returns 0 (or a count) on success and a negative fls_status on
 * error, with fls_last_error() holding a message for the calling thread.
 * Decoded columns are DuckDB physical layouts: int8..int64 little-endian,
 * DATE int32 days, DECIMAL int64 scaled, VARCHAR duckdb::string_t (16 B:
 * u32 length + 12 inline bytes, or u32 length + 4-byte prefix + char* into a
 * pinned host dictionary heap owned by the table).
 * A table handle is used by one host thread at a time (DuckDB's scan thread,
 * src/scanner/scan_fastlanes.cpp:43-45), except fls_scan_acquire/release,
 * which any number of threads may call concurrently between fls_scan_begin
 * and the next begin/close; internally there is one HIP stream set per GPU.
 */
#ifndef FLSGPU_H
#define FLSGPU_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum fls_status {
    FLS_OK = 0,
    FLS_ERR_IO = -1,        /* cannot open / read the file */
    FLS_ERR_FORMAT = -2,    /* not an .fls file or corrupt footer / chunk */
    FLS_ERR_ARG = -3,       /* bad argument (index out of range, NULL) */
    FLS_ERR_DEVICE = -4,    /* HIP runtime error or no usable GPU */
    FLS_ERR_STATE = -5,     /* call out of order (e.g. decode before upload) */
    FLS_ERR_NOMEM = -6,
    FLS_ERR_CONFIG = -7,    /* an FLS_* tuning variable names a kernel this build does not hold */
    FLS_ERR_LIMIT = -8      /* a documented capacity was exceeded (fls_aggregate_grouped, fls_aggregate_hashed, fls_topn, fls_keyset_create) */
} fls_status;

typedef struct fls_connection fls_connection;
typedef struct fls_table fls_table;

typedef struct fls_column_info {
    const char *name;   /* NUL-terminated, owned by the table */
    uint8_t type;       /* enum fls_type (flswriter.h) */
    uint8_t width;      /* DECIMAL width */
    uint8_t scale;      /* DECIMAL scale */
    uint8_t out_bytes;  /* bytes per decoded value (string_t = 16) */
} fls_column_info;

typedef struct fls_rowgroup {
    uint32_t rowgroup;            /* row-group index within the table */
    uint32_t nrows;               /* rows delivered (after a pushed-down filter) */
    uint64_t first_row;           /* global row index of the row group's first row */
    uint32_t ncols;
    const void *const *columns;   /* ncols pointers into pinned host memory;
                                     NULL for columns not selected */
    uint32_t nrows_scanned;       /* rows of the row group */
    const uint32_t *sel;          /* filtered scan: the delivered rows' indices
                                     within the row group (ascending); NULL
                                     when every row is delivered */
    const uint64_t *const *validity; /* ncols pointers: the delivered rows'
                                     validity mask in DuckDB's layout (bit i
                                     of word i / 64 set when delivered row i
                                     is not NULL), or NULL when every
                                     delivered row is valid (and for columns
                                     not selected).  Values at NULL rows are
                                     placeholders.  Valid as long as columns. */
    const void *const *dict;      /* ncols pointers (fls_scan_dict_codes): for a
                                     column delivered as dictionary codes in
                                     this row group, its dictionary as 16-byte
                                     string_t records (host); columns[c] then
                                     holds one code per delivered row,
                                     dict_width[c] bytes each (1 or 2, little
                                     endian).  NULL for other columns. */
    const uint32_t *dict_size;    /* ncols: entries of dict[c] */
    const uint8_t *dict_width;    /* ncols: bytes per delivered value */
    const uint8_t *narrow;        /* ncols (fls_scan_narrow): 1 when columns[c]
                                     holds value - narrow_base[c] as an
                                     unsigned dict_width[c]-byte integer (the
                                     value, mod 2^64, is their sum) */
    const uint64_t *narrow_base;  /* ncols: this row group's base */
} fls_rowgroup;

/* Pushed-down filter term: `column <op> constant` (DuckDB TableFilterSet:
 * ConstantFilter / IsNullFilter / IsNotNullFilter; ConjunctionOr and InFilter
 * become several terms of one clause, ConjunctionAnd several clauses).
 * Terms with equal `clause` are OR-ed, clauses are AND-ed.
 * FLS_CMP_IN_SET / FLS_CMP_NOT_IN_SET test membership in a key set
 * (fls_keyset_create below): `value` carries the set's handle.  IN_SET holds
 * for a row whose column is valid and whose decoded value, sign- or
 * zero-extended to 64 bits, is in the set; NOT_IN_SET for a valid row whose
 * value is not; a NULL row satisfies neither.  A set term is a clause of its
 * own, AND-ed with the rest (the semi-join / anti-join restriction of a fact
 * table by a filtered dimension's keys).
 * FLS_CMP_LIKE / FLS_CMP_NOT_LIKE match a VARCHAR column against a pattern
 * (DuckDB's LIKE): `str` / `str_len` carry the pattern, `value` is 0 for no
 * escape byte, else the escape byte (1..255).  The pattern is a byte string:
 * `%` matches any sequence of bytes, the empty one included; `_` matches one
 * character, that is one byte and every directly following continuation byte
 * ((b & 0xC0) == 0x80) -- which defines the result on ill-formed UTF-8 too: a
 * stray continuation byte the match position stands on is a character of its
 * own; every other byte matches itself, case-sensitively and bytewise; the
 * whole string must be consumed.  The escape byte followed by any byte x
 * matches x literally (so `%`, `_` and the escape byte itself can be matched);
 * a pattern ending in a lone escape byte is FLS_ERR_ARG.  A NULL row
 * satisfies neither LIKE nor NOT LIKE; a NULL pattern is FLS_CMP_FALSE.  A
 * BLOB or non-string column is FLS_ERR_ARG.  A pattern term is a clause of
 * its own, AND-ed with the rest; at most 8 pattern terms per filter and 256
 * tokens per pattern (a literal byte, `_`, or a run of `%` is one token),
 * more of either is FLS_ERR_ARG.  Pruning is exact on dictionary-encoded
 * chunks (the pattern is run on each dictionary string).
 * FLS_CMP_COL_EQ .. FLS_CMP_COL_GE compare two columns of the same row:
 * `op - FLS_CMP_COL_EQ` is the ordinary comparison FLS_CMP_EQ .. FLS_CMP_GE,
 * `col` the left column, `value` the index of the right column; `str` and
 * `str_len` are ignored.  The term holds for a row when both values are valid
 * and `left op right` holds in the order the constant terms use; a NULL on
 * either side satisfies no operator, `!=` included.  Integers are sign- or
 * zero-extended to 64 bits, so the two widths may differ (INT8 against
 * INT64).  FLOAT and DOUBLE compare as binary64, a FLOAT widened exactly:
 * NaN equals NaN and sits above every number, -0 equals 0.  Accepted pairs:
 * two signed integer columns; two unsigned integer columns (BOOLEAN
 * included); two DATE columns; two DECIMAL columns of at most 64 bits with
 * equal scale; two of FLOAT / DOUBLE in any mix.  The same column on both
 * sides is legal: `a = a` selects the valid rows, `a < a` none.  FLS_ERR_ARG,
 * naming the term and both columns, before any device work: a right column
 * out of range; VARCHAR / BLOB on either side; signed against unsigned; an
 * integer-like column against a float; DATE against a non-DATE; DECIMAL
 * against a non-DECIMAL, DECIMALs of different scale or one wider than 64
 * bits; a column term that shares its clause with another term (it is a
 * clause of its own, AND-ed with the rest).  A row group is pruned when
 * either side is all NULL or when the two zone maps exclude the comparison
 * (min(a) < max(b) for `<`, intersecting ranges for `=`, ...); a missing zone
 * map on either side keeps it.
 * FLS_CMP_MAP_EQ .. FLS_CMP_MAP_GE compare a column with the value a value
 * map (fls_valuemap_create below) gives a key column of the same row,
 * `left op map[key]`: `op - FLS_CMP_MAP_EQ` is the ordinary comparison, `col`
 * the left column, `key_col` the key column, `value` the map's handle; `str`
 * and `str_len` are ignored.  The term holds for a row when the left column
 * is valid, the key column is valid, the key (sign- or zero-extended to 64
 * bits) is in the map and `left op map[key]` holds.  A NULL on either side,
 * or a key the map does not hold, satisfies no operator, `!=` included: an
 * inner join whose payload would be NULL otherwise.  The left value is sign-
 * or zero-extended to 64 bits and compared as signed when the map's value
 * kind is signed, as unsigned otherwise.  The map's values are in the left
 * column's physical unit (DATE days, DECIMAL scaled): units are the caller's
 * business, nothing is rescaled.  The key column may be the left column or
 * any other column.  A map term is a clause of its own, AND-ed with the rest;
 * at most 8 map terms per term list (a filter, one condition, one
 * alternative).  FLS_ERR_ARG, naming the term and both columns, before any
 * device work: a key column out of range; VARCHAR / BLOB / FLOAT / DOUBLE on
 * either side; a DECIMAL wider than 64 bits on either side; a left column
 * whose signedness differs from the map's value kind, a key column whose
 * signedness differs from its key kind (signed ints, DATE and DECIMAL are
 * signed; unsigned ints and BOOLEAN unsigned); a handle that is not a live
 * value map ("filter operator 19 unknown for value 0x...: not a live value
 * map"); a map term sharing its clause; more than 8 map terms in a list.
 * A row group is pruned when the left or the key chunk is all NULL, the map
 * is empty, the key zone map holds no key of the map (exact on a sorted
 * column), or the left zone map against the map's [value_min, value_max]
 * excludes the comparison as for a column term; a missing zone map keeps it. */
typedef enum fls_cmp {
    FLS_CMP_EQ = 0, FLS_CMP_NE = 1, FLS_CMP_LT = 2, FLS_CMP_LE = 3, FLS_CMP_GT = 4, FLS_CMP_GE = 5,
    FLS_CMP_IS_NULL = 6, FLS_CMP_IS_NOT_NULL = 7,
    FLS_CMP_FALSE = 8,            /* holds for no row (a comparison with a NULL constant) */
    FLS_CMP_IN_SET = 9, FLS_CMP_NOT_IN_SET = 10,
    FLS_CMP_LIKE = 11, FLS_CMP_NOT_LIKE = 12,
    FLS_CMP_COL_EQ = 13, FLS_CMP_COL_NE = 14, FLS_CMP_COL_LT = 15, FLS_CMP_COL_LE = 16, FLS_CMP_COL_GT = 17,
    FLS_CMP_COL_GE = 18,          /* column against column: value is the right column's index */
    FLS_CMP_MAP_EQ = 19, FLS_CMP_MAP_NE = 20, FLS_CMP_MAP_LT = 21, FLS_CMP_MAP_LE = 22, FLS_CMP_MAP_GT = 23,
    FLS_CMP_MAP_GE = 24           /* column against map[key_col]: value is the fls_valuemap handle */
} fls_cmp;
typedef struct fls_predicate {
    uint32_t col;                 /* table column */
    uint32_t clause;
    uint8_t op;                   /* fls_cmp */
    uint8_t pad[3];
    uint32_t key_col;             /* MAP_EQ .. MAP_GE: the key column; every other op ignores it
                                     (the tail of what was pad[7]: size and offsets are unchanged) */
    uint64_t value;               /* constant in the column's physical type:
                                     signed ints / DATE days / DECIMAL scaled as
                                     int64, unsigned as uint64, FLOAT as IEEE
                                     binary32 bits (low 32), DOUBLE binary64 bits;
                                     IN_SET / NOT_IN_SET: the fls_keyset handle;
                                     LIKE / NOT_LIKE: the escape byte, 0 for none;
                                     COL_EQ .. COL_GE: the right column's index;
                                     MAP_EQ .. MAP_GE: the fls_valuemap handle */
    const char *str;              /* VARCHAR constant or LIKE pattern (copied) */
    uint64_t str_len;
} fls_predicate;

typedef struct fls_decode_stats {
    double kernel_ms;             /* duration of the last decode launch (HIP events) */
    uint64_t values;              /* values decoded by that launch */
    uint64_t packed_bytes;        /* algorithmic bytes read: bit-packed streams */
    uint64_t meta_bytes;          /* per-vector metadata, bases, dictionaries, run values */
    uint64_t out_bytes;           /* algorithmic bytes written: decoded columns */
    uint32_t launches;            /* decode launches since upload */
    uint32_t timed_launches;      /* launches since the previous fls_device_sync */
    double kernel_ms_total;       /* sum of their kernel durations (HIP events on the
                                     decode stream, one start/stop pair per launch) */
} fls_decode_stats;

const char *fls_last_error(void);
const char *fls_version(void);
/* Deployment knobs: the environment variables the library and the extension
 * read (FLS_IDLE_PINNED_MB, FLS_SCAN_RESIDENT_MB, FLS_COPY_BATCH, ...; the
 * list with each meaning is in INTEGRATION.md), defaults kept in one table
 * (csrc/fls_config.hpp).  fls_config_default: the compiled default;
 * fls_config_value: the value in effect (the environment's, else the
 * default); FLS_ERR_ARG for a name that is not a knob.  fls_config_count /
 * fls_config_name enumerate the knobs (NULL past the end).  Not in the
 * reference, which reads no environment. */
int fls_config_default(const char *name, int64_t *value);
int fls_config_value(const char *name, int64_t *value);
int fls_config_count(void);
const char *fls_config_name(int i);
/* Number of HIP devices visible (0 when there is no GPU). */
int fls_device_count(void);
/* Raw device buffers and copies on GPU `device`, for callers that hold no HIP
 * runtime of their own (bindings, tests, the encoder bench): kind 0 = host to
 * device, 1 = device to host, 2 = device to device. */
int fls_device_alloc(int device, uint64_t bytes, void **ptr);
int fls_device_free(int device, void *ptr);
int fls_device_memcpy(int device, void *dst, const void *src, uint64_t bytes, int kind);

/* fastlanes::connect(): devices = HIP ordinals to shard row groups over
 * (NULL/0 = device 0). */
int fls_connect(const int *devices, int ndevices, fls_connection **out);
void fls_disconnect(fls_connection *conn);
/* Free the connection's idle scan pipelines (streams, device slots, pinned
 * host batches kept for the next scan) down to keep_bytes of pinned memory
 * per GPU (0: all of them); idle_bytes (may be NULL) receives what stays.
 * Idle pinned memory is also capped per GPU when a scan ends
 * (FLS_IDLE_PINNED_MB, default 1024).  Not in the reference: a long-lived
 * host (DuckDB) uses it to hand page-locked memory back. */
int fls_connection_trim(fls_connection *conn, uint64_t keep_bytes, uint64_t *idle_bytes);
/* HBM-resident compressed images (the scan pipeline keeps a scanned file's
 * bytes in HBM so warm queries skip the H2D): one byte budget per GPU over
 * every cached file (FLS_SCAN_RESIDENT_MB, default 65,536), least recently
 * used images evicted first, never one a running scan uses.  Not in the
 * reference, whose closeFile (src/fastlanes_facade.cpp:202-210) releases
 * everything it holds.
 * fls_release_device_memory: free every image no running scan uses on
 * device (-1: every GPU); freed_bytes (may be NULL) receives the bytes freed.
 * fls_resident_info: the images' bytes and count on device (-1: every GPU). */
int fls_release_device_memory(int device, uint64_t *freed_bytes);
int fls_resident_info(int device, uint64_t *bytes, uint32_t *images);

/* Key sets: the build side of a semi-join pushed into the scan filter
 * (FLS_CMP_IN_SET / FLS_CMP_NOT_IN_SET).  fls_keyset_create builds the set of
 * keys[0, n) on the host -- no GPU is needed to create a set, query it or
 * prune with it.  keys are 64-bit patterns as fls_predicate.value carries a
 * constant of the column's physical type; kind is the order of the column the
 * set will be probed with (signed: INT*, DATE, DECIMAL; unsigned: UINT*,
 * BOOLEAN) and orders min / max and the pruning.  Duplicates are removed;
 * n = 0 is a valid empty set; sets hold no NULL.
 * form: 0 auto, 1 bitmap, 2 hash table.
 *   bitmap: one bit per value of [min, max] (max - min < 2^32).
 *   hash:   open addressing, linear probing, 8-byte slots, capacity the next
 *           power of two >= 2 * count (1 for the empty set); the home slot of
 *           key k is (k * 0x9E3779B97F4A7C15 mod 2^64) >> (64 - log2(capacity))
 *           (slot 0 when the capacity is 1); keys are inserted in ascending
 *           order of the set's kind, so the table is a pure function of the
 *           set.  An empty slot holds a sentinel: the largest 64-bit pattern
 *           that is not a key (~0, else ~0 - 1, ...), so every 64-bit key is
 *           representable.  max_probe is the largest number of slots examined
 *           to find a key of the set; every lookup, on the host and on the
 *           GPU, stops at a match, an empty slot or after max_probe slots.
 *   auto:   the bitmap when max - min < 2^32 and it is no larger than the hash
 *           table would be, or at most 1 MiB; else the hash table.
 * FLS_ERR_LIMIT: n above 2^28 (kMaxKeysetKeys; returned before keys is
 * read), a forced bitmap spanning more than 2^32 values.
 * The handle is an opaque token, never dereferenced: every call looks it up
 * among the live sets, and a stale or foreign value is FLS_ERR_ARG.
 * fls_scan_filter takes a reference on the set, so freeing the handle while a
 * filter or a running scan uses it is safe.  The set's image is uploaded to a
 * GPU by the first scan that probes it there and cached per device inside the
 * set until the set (and every filter holding it) or its connection is gone.
 * It does not count against FLS_SCAN_RESIDENT_MB, and fls_connection_trim and
 * fls_release_device_memory do not free it: free the set.  The upload is
 * synchronous (fls_keyset_info.device_bytes per GPU, up to 4 GiB at 2^28
 * keys) and is paid by the first batch on each device.  One set may serve
 * any number of tables.
 * fls_scan_filter / fls_rowgroup_may_match refuse with FLS_ERR_ARG before any
 * device work, the message naming the term ("filter term i: ..."): a set term
 * on a VARCHAR / BLOB / FLOAT / DOUBLE column or a DECIMAL wider than 64 bits,
 * a set whose kind differs from the column's, a handle that is not live, and
 * a set term that shares its clause with another term.
 * Pruning: under IN_SET a row group with a zone map is read only if a key
 * lies in [min, max] of its zone map (the empty set prunes every row group,
 * so the call does no device work); an all-NULL chunk matches neither
 * operator; NOT_IN_SET prunes nothing else.  Not in the reference. */
typedef struct fls_keyset fls_keyset;
typedef enum fls_keyset_kind { FLS_KEYSET_SIGNED = 0, FLS_KEYSET_UNSIGNED = 1 } fls_keyset_kind;
typedef enum fls_keyset_form { FLS_KEYSET_AUTO = 0, FLS_KEYSET_BITMAP = 1, FLS_KEYSET_HASH = 2 } fls_keyset_form;
typedef struct fls_keyset_info_t {
    uint64_t count;         /* distinct keys */
    uint32_t form;          /* the form chosen: FLS_KEYSET_BITMAP or FLS_KEYSET_HASH */
    uint32_t kind;          /* fls_keyset_kind */
    uint64_t device_bytes;  /* bytes of the image, per GPU that probes the set */
    uint64_t capacity;      /* hash: slots (0 for a bitmap) */
    uint32_t max_probe;     /* hash: longest probe sequence (0 for a bitmap or an empty set) */
    uint32_t pad;
    uint64_t min, max;      /* patterns, in the set's order (0 for the empty set) */
    uint64_t empty;         /* hash: the empty slot's sentinel */
} fls_keyset_info_t;
int fls_keyset_create(fls_connection *conn, const uint64_t *keys, uint64_t n, int kind, int form, fls_keyset **out);
void fls_keyset_free(fls_keyset *set);
int fls_keyset_info(const fls_keyset *set, fls_keyset_info_t *info);
/* Host probe of the very image a scan uploads: 1 in the set, 0 not. */
int fls_keyset_contains(const fls_keyset *set, uint64_t key);

/* The build side on the GPU: the set of the non-NULL values of column col over
 * the rows of row groups [rg_begin, rg_end) that the filter and alternatives
 * currently set on the table select (fls_scan_filter,
 * fls_scan_filter_alternatives) -- the set fls_keyset_create builds from those
 * values, image for image: the same form under the auto rule, min / max,
 * sentinel, max_probe and sorted keys.  Its kind follows the column (signed:
 * INT*, DATE, DECIMAL; unsigned: UINT*, BOOLEAN); it belongs to the table's
 * connection and is used, queried and freed like any other set.
 * The scan decodes the filter's, the alternatives' and the key column and
 * delivers nothing: the selected keys are collected on each GPU as bits of a
 * bitmap over the union of the key column's zone maps over the row groups
 * that survive pruning (the physical type's range where one of them has no
 * zone map; a row group whose key chunk is all NULL is skipped), and the host
 * receives span / 8 bytes per GPU instead of the keys.  That needs
 *   span + 1 <= 2^32, and
 *   a bitmap of at most 1 MiB, or no larger than the surviving row groups'
 *   rows times the column's width (the copy it replaces);
 * otherwise FLS_ERR_LIMIT before any device work, the message naming the span
 * and both sizes: build the set from a filtered scan and fls_keyset_create.
 * No surviving row group (an empty table or range, everything pruned) gives
 * the empty set without device work.
 * FLS_ERR_ARG before any device work: a column out of range, a VARCHAR / BLOB
 * / FLOAT / DOUBLE column, a DECIMAL wider than 64 bits, a form outside 0..2,
 * a row-group range outside the table.  FLS_ERR_FORMAT: a decoded key outside
 * the zone maps that gave the range (it sets no bit).
 * FLS_KEYSET_BUILD_WINDOW=0 (A/B) sends every row's atomic straight to HBM
 * instead of combining clustered rows in LDS first.  Not in the reference. */
typedef struct fls_keyset_build_info_t {
    uint64_t rows_selected;   /* selected, non-NULL rows that set a bit */
    uint64_t bitmap_bytes;    /* per device */
    uint64_t d2h_bytes;       /* everything the build copied to the host */
    uint64_t base, span;      /* the collecting range */
    uint32_t rowgroups_read, rowgroups_pruned;
} fls_keyset_build_info_t;
int fls_keyset_from_scan(fls_table *t, uint32_t col, uint32_t rg_begin, uint32_t rg_end, int form, fls_keyset **out,
                         fls_keyset_build_info_t *info /* may be NULL */);

/* Connection::read_fls(): parse footer + schema (no GPU work). */
int fls_read_fls(fls_connection *conn, const char *path, fls_table **out);
/* Same over an in-memory image (copy=0: caller keeps img alive). */
int fls_read_fls_image(fls_connection *conn, const void *img, uint64_t len, int copy, fls_table **out);
void fls_table_close(fls_table *t);

uint32_t fls_table_ncols(const fls_table *t);
uint64_t fls_table_nrows(const fls_table *t);
uint64_t fls_table_row_offset(const fls_table *t);
uint32_t fls_table_nrowgroups(const fls_table *t);
int64_t fls_table_rowgroup_rows(const fls_table *t, uint32_t rg);
int fls_table_column(const fls_table *t, uint32_t col, fls_column_info *out);

/* Decode the selected columns (col_mask[c] != 0; NULL = all) of one row group
 * on the GPU that owns it and deliver them into pinned host buffers owned by
 * the table, valid until the next materialize/scan call. */
int fls_materialize(fls_table *t, uint32_t rg, const uint8_t *col_mask, fls_rowgroup *out);

/* Streaming scan over row groups [rg_begin, rg_end) in order: row groups are
 * sharded contiguously over the connection's GPUs, uploaded once, decoded in
 * batches and copied to pinned host memory ahead of the consumer. */
int fls_scan_begin(fls_table *t, const uint8_t *col_mask, uint32_t rg_begin, uint32_t rg_end);
/* 1 = a row group was delivered into *out, 0 = end of scan, <0 = error.
 * The previous row group's buffers are released by the call. */
int fls_scan_next(fls_table *t, fls_rowgroup *out);
/* Filter for the following fls_scan_begin and fls_aggregate calls on this
 * table (n = 0 clears).  The scan then skips row groups whose zone maps / dictionaries
 * rule every row out, evaluates the filter per row on the GPU and delivers
 * only qualifying rows (fls_rowgroup.nrows / sel), in row order.  The
 * filter's columns are decoded whether or not col_mask delivers them. */
int fls_scan_filter(fls_table *t, const fls_predicate *preds, uint32_t n);
/* Alternatives of the filter: AND-groups joined by OR (TPC-H Q19's shape), for
 * the following fls_scan_begin, fls_aggregate*, fls_topn and every other call
 * that honours fls_scan_filter
 * (copied and replaced as a whole; at most 8 alternatives; nalts = 0 clears;
 * sticky like the filter, which fls_scan_filter keeps replacing alone).  A row
 * is selected when the filter set by fls_scan_filter selects it (an empty
 * filter selects every row) and at least one alternative is true there; it
 * counts once however many hold.  Alternative i is a filter of its own,
 * preds[first .. first + n) in the shape fls_scan_filter takes: a conjunction
 * of clauses (`clause` numbers are local to the alternative), a clause OR-ed
 * `column op constant` / IS [NOT] NULL terms or a single key-set, LIKE or
 * column-pair term; its key sets are kept alive as the filter keeps them, and
 * the filter's limits (8 pattern terms, 256 tokens) hold per alternative.  A
 * comparison on a NULL is not true, so `A OR B` selects a row when A is true
 * or B is true.  One alternative alone equals AND-ing its terms to the filter.
 * An aggregate condition (fls_aggregate_conditions) holds no alternatives.
 * Pruning: a row group is read when the filter may match it and at least one
 * alternative may (zone maps, DICT dictionaries, key-set keys and LIKE on
 * dictionaries per alternative, as for the filter); fls_scan_pruned, the
 * aggregate calls' overflow bounds and "no row group left" paths follow that
 * set, and a top-N scan with alternatives counts as filtered (no zone-map cut
 * on the key).  fls_rowgroup_may_match takes explicit terms and ignores the
 * list.  On the GPU, after the filter's kernels, one launch per batch
 * (csrc/fls_alt.hip) evaluates the ordinary terms of every alternative and
 * ORs those that hold nothing else into the mask; an alternative with key-set,
 * LIKE or column-pair terms gets a plane that the filter's kernels narrow, and
 * one more launch ORs the planes into the mask.  The consumers' kernels see an
 * ordinary mask.  The columns alternatives read are decoded whether or not
 * they are delivered.
 * FLS_ERR_ARG before any device work: more than 8 alternatives; "alternative
 * i:" n == 0 or a range past npreds; "alternative i, term j: <the refusal
 * fls_scan_filter gives the term>", j and the clause numbers local to the
 * alternative (the three "shares clause" refusals included); in
 * fls_aggregate_grouped an alternative term that reads a VARCHAR key column
 * (the filter's rule).  Not in the reference. */
typedef struct fls_filter_alternative { uint32_t first, n; } fls_filter_alternative;   /* preds[first .. first + n) */
int fls_scan_filter_alternatives(fls_table *t, const fls_predicate *preds, uint32_t npreds,
                                 const fls_filter_alternative *alts, uint32_t nalts);
/* Row groups the current scan skipped by zone maps / dictionaries. */
int fls_scan_pruned(const fls_table *t);

/* Ungrouped aggregates evaluated on the GPU over row groups [rg_begin, rg_end)
 * under the filter set by fls_scan_filter: the operand columns are decoded
 * into HBM, reduced there per 1024-row vector (csrc/fls_agg.hip), and only
 * the per-vector partial results cross PCIe; the call folds them in row order
 * and is synchronous.  A row contributes to an aggregate when the filter
 * selects it and the aggregate's operand column(s) are not NULL there.
 * Integer sums (INT*, UINT*, BOOLEAN, DATE, DECIMAL scaled) are exact 128-bit
 * two's-complement values; FLOAT / DOUBLE sums are binary64 (FLOAT widened
 * exactly) with IEEE propagation of NaN and infinities; float MIN / MAX use
 * the filter's order (NaN above every number, -0 == 0).  Every result,
 * binary64 sums included, is bit-identical whatever the batch size, slot
 * count or number of GPUs.  Row groups the filter's zone maps / dictionaries
 * rule out are skipped (fls_scan_pruned); when none is left the call does no
 * device work.  The call replaces a scan in progress on the table, as
 * fls_scan_begin does.  FLS_ERR_ARG (the message names the aggregate's index)
 * before any device work: n == 0 or n > 32, a column out of range, an unknown
 * function, SUM / MIN / MAX / SUM_PRODUCT of a VARCHAR / BLOB column,
 * SUM_PRODUCT with a FLOAT / DOUBLE operand, and a SUM_PRODUCT whose zone-map
 * bound (sum over the scanned row groups of rows * max|a| * max|b|) reaches
 * 2^127.  Not in the reference, which delivers every decoded row to DuckDB. */
typedef enum fls_agg_fn { FLS_AGG_COUNT_STAR = 0, FLS_AGG_COUNT = 1, FLS_AGG_SUM = 2,
                          FLS_AGG_MIN = 3, FLS_AGG_MAX = 4, FLS_AGG_SUM_PRODUCT = 5,
                          FLS_AGG_SUM_EXPR = 6 /* spec.col indexes the table's expression list */ } fls_agg_fn;
typedef struct fls_aggregate_spec {
    uint8_t fn; uint8_t pad[3]; uint32_t col; uint32_t col2;
    uint32_t cond;   /* 0: no condition; i: condition i - 1 of fls_aggregate_conditions (agg FILTER (WHERE ...)) */
} fls_aggregate_spec;
typedef enum fls_agg_kind { FLS_AGGV_NULL = 0, FLS_AGGV_INT = 1, FLS_AGGV_DOUBLE = 2 } fls_agg_kind;
typedef struct fls_aggregate_value {
    uint64_t count;   /* rows that contributed */
    uint64_t lo, hi;  /* INT: 128-bit two's complement (counts, integer sums, integer MIN/MAX sign- or
                         zero-extended); DOUBLE: binary64 bits in lo (float sums; FLOAT/DOUBLE MIN/MAX widened
                         to double as fls_table_zonemap does) */
    uint8_t kind;     /* NULL: SUM/MIN/MAX with no contributing row (DuckDB's NULL); counts are never NULL */
    uint8_t pad[7];
} fls_aggregate_value;
int fls_aggregate(fls_table *t, const fls_aggregate_spec *aggs, uint32_t n,
                  uint32_t rg_begin, uint32_t rg_end, fls_aggregate_value *out);
/* Expression list for FLS_AGG_SUM_EXPR in the following fls_aggregate and
 * fls_aggregate_grouped calls on this table (copied; n = 0 clears; n <= 32;
 * sticky like fls_scan_filter's terms).  An expression is the product of 1 to
 * 3 factors k + sign * column: sign is +1 or -1, k an int64 in the column's
 * physical unit (a DECIMAL constant scaled), the column INT*, UINT*, BOOLEAN,
 * DATE or DECIMAL; one column may appear in several factors.  SUM_EXPR is the
 * exact 128-bit two's-complement sum of the product, with SUM_PRODUCT's
 * filter, pruning and determinism: a row contributes when the filter selects
 * it and every factor's column is valid there; no such row gives
 * FLS_AGGV_NULL.  FLS_ERR_ARG naming "expression i" before any device work:
 * nfactors outside 1..3, a sign other than +1 / -1, a column out of range, a
 * VARCHAR / BLOB / FLOAT / DOUBLE column.  The aggregate calls refuse, naming
 * "aggregate i", a spec.col at or past the number of expressions set, and a
 * SUM_EXPR whose zone-map bound -- sum over the scanned row groups of rows *
 * prod max|k + sign * x|, the maxima taken at the ends of the zone-map range
 * (the type's range without a zone map, 0 for an all-NULL chunk), rounded
 * upwards -- reaches 2^127.  Not in the reference. */
typedef struct fls_agg_factor { uint32_t col; int8_t sign; uint8_t pad[3]; int64_t k; } fls_agg_factor;   /* k + sign * column */
typedef struct fls_agg_expr   { uint32_t nfactors; uint32_t pad; fls_agg_factor f[3]; } fls_agg_expr;     /* product of 1..3 factors */
int fls_aggregate_exprs(fls_table *t, const fls_agg_expr *exprs, uint32_t n);
/* Filtered aggregates: SQL's agg(...) FILTER (WHERE cond), in the following
 * fls_aggregate, fls_aggregate_grouped and fls_aggregate_hashed[_select] calls
 * (copied and replaced as a whole; at most 8 conditions; nconds = 0 clears;
 * sticky like fls_aggregate_exprs; fls_topn and plain scans ignore the list).
 * Condition i is a filter of its own, preds[first .. first + n) in the shape
 * fls_scan_filter takes: a conjunction of clauses (`clause` numbers are local
 * to the condition), a clause OR-ed `column op constant` / IS [NOT] NULL terms
 * or a single key-set, LIKE or column-pair term; its key sets are kept alive
 * as the filter keeps them.  An aggregate whose spec.cond is i + 1 counts a
 * row when the scan's filter selects it, condition i is true there (a
 * comparison on a NULL is not true) and its operands are valid there;
 * COUNT_STAR under a condition counts the rows where the condition is true;
 * spec.cond = 0 is the aggregate as before.  A condition prunes nothing and
 * selects no row: row-group pruning, group membership (grouped and hashed) and
 * the hashed call's first row follow the scan's filter alone, so a group in
 * which no row meets the condition is there with count 0 and a NULL SUM / MIN
 * / MAX.  The SUM_PRODUCT / SUM_EXPR overflow bounds ignore conditions (upper
 * bounds over a superset of the rows), HAVING / ORDER BY see a conditioned
 * aggregate like any other, and results are bit-identical across batch sizes,
 * slots, pipelines and GPU counts as before.  On the GPU one launch per batch
 * (csrc/fls_cond.hip) writes a plane of `filter & condition` words per
 * condition, which the reduce kernels AND in where they AND validity; key-set,
 * LIKE and column-pair terms narrow their plane through the filter's kernels.
 * The columns conditions read are decoded only in row groups the scan reads.
 * FLS_ERR_ARG before any device work: more than 8 conditions; "condition i:"
 * n == 0 or a range past npreds; "condition i, term j: <the refusal
 * fls_scan_filter gives the term>", j and the clause numbers local to the
 * condition (the three "shares clause" refusals included); in the aggregate
 * calls "aggregate i: condition k out of range (n set by
 * fls_aggregate_conditions)"; in fls_aggregate_grouped a condition term that
 * reads a VARCHAR key column (the filter's rule).  Not in the reference. */
typedef struct fls_agg_condition { uint32_t first, n; } fls_agg_condition;   /* preds[first .. first + n) */
int fls_aggregate_conditions(fls_table *t, const fls_predicate *preds, uint32_t npreds,
                             const fls_agg_condition *conds, uint32_t nconds);
/* GROUP BY keys[0..nkeys) of the same aggregates, for low-cardinality keys:
 * fls_aggregate's functions, filter, pruning, argument checks and numeric
 * results, per group.  The batch is reduced in HBM per (1024-row vector, key)
 * and merged per row group (csrc/fls_groupagg.hip); one table of at most 256
 * groups per row group crosses PCIe, and the call merges the row groups'
 * tables by key value.  A row belongs to a group when the filter selects it;
 * a key no selected row carries makes no group.  Within a group a row counts
 * for an aggregate exactly as in fls_aggregate.  Key columns (1 to 4): INT*,
 * UINT*, BOOLEAN, DATE, DECIMAL of at most 64 bits in any encoding (the key is
 * the decoded value), or a VARCHAR column whose chunk is DICT with at most
 * 65536 entries in every row group the scan reads (the key is the string; the
 * dictionaries may differ per row group).  A NULL key is a group of its own.
 * The packed key -- 8 x value bytes per integer key, 16 bits per VARCHAR key,
 * one NULL bit per key -- holds at most 128 bits.  Groups come in order of
 * first occurrence in table row order.  Every value, binary64 sums included,
 * is bit-identical whatever the batch size, slot count or number of GPUs, and
 * with a single group equals fls_aggregate's.  No row group to read (an empty
 * range, everything pruned): zero groups, no device work.
 * FLS_ERR_ARG before any device work, naming the key's index ("key 1: ..."):
 * nkeys == 0 or > 4, a key column out of range or listed twice, a FLOAT /
 * DOUBLE / BLOB key, a VARCHAR key with a non-DICT chunk (or a dictionary of
 * more than 65536 entries) in range, a VARCHAR key a filter term reads, a
 * packed key of more than 128 bits; and everything fls_aggregate refuses.
 * FLS_ERR_LIMIT: more than 64 distinct keys among one vector's selected rows,
 * or more than 256 in one row group (the kernels check before they write; fall
 * back to a scan).  The table stays usable.  The number of groups over the
 * table is not limited.
 * *out is owned by the caller (fls_group_result_free), strings included. */
typedef struct fls_group_result fls_group_result;
typedef enum fls_key_kind { FLS_KEYV_NULL = 0, FLS_KEYV_INT = 1, FLS_KEYV_STRING = 2 } fls_key_kind;
typedef struct fls_group_key {
    uint8_t kind;       /* fls_key_kind */
    uint8_t pad[7];
    uint64_t lo, hi;    /* INT: the value, sign- or zero-extended to 128 bits by column type */
    const char *str;    /* STRING: str_len bytes (not NUL-terminated), owned by the result */
    uint64_t str_len;
} fls_group_key;
int fls_aggregate_grouped(fls_table *t, const uint32_t *keys, uint32_t nkeys,
                          const fls_aggregate_spec *aggs, uint32_t n,
                          uint32_t rg_begin, uint32_t rg_end, fls_group_result **out);
uint64_t fls_group_result_ngroups(const fls_group_result *r);
/* key `key` (0 .. nkeys-1) of group `group`; FLS_ERR_ARG out of range */
int fls_group_result_key(const fls_group_result *r, uint64_t group, uint32_t key, fls_group_key *out);
/* the group's n values in the aggregates' order; NULL out of range */
const fls_aggregate_value *fls_group_result_values(const fls_group_result *r, uint64_t group);
void fls_group_result_free(fls_group_result *r);
/* GROUP BY keys[0..nkeys) of any cardinality up to max_groups: a hash
 * aggregate in HBM, for the keys fls_aggregate_grouped's 64 / 256 distinct-key
 * limits refuse (GROUP BY l_orderkey, l_partkey, l_suppkey).  The filter set by
 * fls_scan_filter (key sets included), the pruning, the decode, the resident
 * image, the batch pipeline and the sharding over pipelines are the other
 * aggregate calls'; only the reduction differs: every pipeline of the scan
 * owns one open-addressing table in HBM for the length of the call -- the next
 * power of two >= 2 * max_groups slots, one 8-byte array per field actually
 * needed: the packed key, the first row, per aggregate its count and, for
 * sums and MIN / MAX, lo and hi -- into which each batch inserts its selected
 * rows with device-scope atomics (csrc/fls_hashagg.hip).  After the scan the
 * occupied slots are compacted on the device, copied in one D2H per pipeline
 * and merged by key on the host when there are several pipelines.
 * Keys (1 to 4): INT*, UINT*, BOOLEAN, DATE, DECIMAL of at most 64 bits, in
 * any encoding; the key is the decoded value, a NULL key a group of its own.
 * The packed key holds at most 63 bits: per key the bits of max - min of its
 * zone maps over [rg_begin, rg_end) before pruning (the type's width where a
 * row group has no valid zone map; an all-NULL chunk adds nothing), plus one
 * NULL bit.  l_orderkey at SF 10 takes 26 + 1 bits; a full-range INT64 key is
 * refused.  A decoded value outside that range means a corrupt or foreign
 * file: FLS_ERR_FORMAT.
 * Aggregates: fls_aggregate's, with its argument checks and overflow bounds --
 * COUNT(*), COUNT(col), integer SUM, SUM_PRODUCT, SUM_EXPR, MIN / MAX of
 * integer and FLOAT / DOUBLE columns -- except SUM of a FLOAT / DOUBLE column:
 * an atomic float sum depends on arrival order, and no call here returns a
 * value that is not reproducible (fls_aggregate_grouped sums floats).
 * Groups come in unspecified order; first_rows gives the caller a canonical
 * one.  The set of (key, first row, values) is identical whatever the batch
 * size, slot count or number of pipelines, and where fls_aggregate_grouped
 * accepts the same arguments it equals that call's groups and values exactly.
 * No row group to read (an empty range, everything pruned): zero groups, no
 * device work, no table.
 * FLS_ERR_ARG before any device work, naming "key q:": nkeys == 0 or > 4, a
 * column out of range or listed twice, a VARCHAR key (a dictionary code means
 * a string of one row group only), a mapped key (FLS_KEY_MAPPED), a FLOAT /
 * DOUBLE / BLOB key, a packed key of more than 63 bits; naming "aggregate i:":
 * everything fls_aggregate refuses and a FLOAT / DOUBLE SUM; max_groups
 * outside 1 .. 2^28.
 * FLS_ERR_LIMIT: more than max_groups distinct keys among the selected rows of
 * one pipeline's row groups (the kernel checks before it writes; call again
 * with a larger max_groups).  FLS_ERR_DEVICE, naming the bytes: a table that
 * cannot be allocated.  The fls_table stays usable after either.
 * *out is owned by the caller (fls_hash_result_free); the accessors return
 * arrays of fls_hash_result_ngroups elements that live as long as the result:
 * first_rows  per group the global row index (fls_rowgroup.first_row + row)
 *             of its first selected row;
 * key         key `key`'s decoded value, sign- or zero-extended to 64 bits by
 *             column type (0 where is_null is 1);
 * aggregate   count / lo / hi / kind with fls_aggregate_value's meaning: a
 *             SUM / MIN / MAX with count 0 is FLS_AGGV_NULL;
 * stats       the bytes of one pipeline's table and the call's phases on the
 *             host clock: the scan, extraction + D2H, merge + unpacking (any
 *             pointer may be NULL).
 * Not in the reference. */
typedef struct fls_hash_result fls_hash_result;
int fls_aggregate_hashed(fls_table *t, const uint32_t *keys, uint32_t nkeys,
                         const fls_aggregate_spec *aggs, uint32_t n, uint64_t max_groups,
                         uint32_t rg_begin, uint32_t rg_end, fls_hash_result **out);
uint64_t fls_hash_result_ngroups(const fls_hash_result *r);
int fls_hash_result_first_rows(const fls_hash_result *r, const uint64_t **rows);
int fls_hash_result_key(const fls_hash_result *r, uint32_t key, const uint64_t **values, const uint8_t **is_null);
int fls_hash_result_aggregate(const fls_hash_result *r, uint32_t agg, const uint64_t **count,
                              const uint64_t **lo, const uint64_t **hi, const uint8_t **kind);
int fls_hash_result_stats(const fls_hash_result *r, uint64_t *table_bytes, double *scan_ms, double *extract_ms,
                          double *merge_ms);
void fls_hash_result_free(fls_hash_result *r);
/* fls_aggregate_hashed that returns only the groups a query wants: HAVING
 * (Q18: sum(l_quantity) > 300) and ORDER BY one aggregate LIMIT k (Q3: the ten
 * largest revenues), chosen in HBM where the scan left the groups, so that
 * only the chosen groups are compacted, copied and unpacked
 * (csrc/fls_hashsel.hip).  Keys, aggregates, filter, pruning, max_groups,
 * FLS_ERR_LIMIT and the "no row group to read" case are fls_aggregate_hashed's,
 * with the same checks and messages; sel == NULL, or a sel with no term, no
 * order and no limit, returns exactly what fls_aggregate_hashed returns.
 * HAVING: a group passes when every one of the nhaving (0 .. 8) terms
 * "aggregate[agg] op constant" holds.  An aggregate of kind FLS_AGGV_INT
 * (counts, integer sums, integer MIN / MAX) compares as a signed 128-bit
 * integer with the constant lo / hi (a UINT64 MIN / MAX zero-extended); a
 * FLOAT / DOUBLE MIN / MAX compares with the binary64 constant in lo in the
 * filter's float order: NaN equals NaN and sits above every number, -0 equals
 * 0.  A NULL aggregate (SUM / MIN / MAX with count 0) satisfies no term,
 * FLS_CMP_NE included.  The comparison runs on the fields as the table stores
 * them; the constant is translated once, and one outside what the field can
 * hold makes its term hold always or never.
 * ORDER BY / LIMIT: the result order is (NULL placement, the aggregate's
 * value, the group's first row); NULLs come last unless nulls_first, whether
 * ascending or descending; NaN is the largest value.  First rows are distinct
 * across groups, so no two groups compare equal and the list is unique.  With
 * an order, limit must be 1 .. 1024 and the result holds the best
 * min(limit, passed) groups in result order.  With FLS_GROUP_ORDER_NONE and
 * limit > 0 it holds the first `limit` passing groups by first row.  With
 * neither, the passing groups come in unspecified order.
 * Everything returned is identical whatever the batch size, slot count or
 * number of pipelines, and equals the plain call's groups with the same
 * selection applied on the host.  The selection runs on the GPU when one
 * pipeline holds the groups.  When several do, a key may straddle shards and
 * only its merged value can decide: all groups are extracted and merged as in
 * the plain call and the same selection, with the same comparators, runs on
 * the host (on_device = 0).
 * FLS_ERR_ARG before any device work, naming "having j:": nhaving > 8, an
 * aggregate index >= n, an op outside FLS_CMP_EQ .. FLS_CMP_GE, a constant
 * kind that is not the aggregate's; naming "order:": an aggregate index >= n,
 * an order without a limit, a limit above 1024.  FLS_ERR_LIMIT,
 * FLS_ERR_DEVICE and FLS_ERR_FORMAT as in the plain call; the fls_table stays
 * usable after each.
 * select_stats: groups_total the groups formed, groups_passed the groups after
 * HAVING and before LIMIT, on_device whether the selection ran on the GPU,
 * select_ms its time on the host clock (any pointer may be NULL); on a result
 * of the plain call total = passed = ngroups and on_device = 0.
 * Not in the reference. */
typedef struct fls_group_having {   /* aggregate[agg] <op> constant */
    uint32_t agg;                   /* index into aggs[] */
    uint8_t  op;                    /* FLS_CMP_EQ .. FLS_CMP_GE only */
    uint8_t  kind;                  /* FLS_AGGV_INT: lo/hi a 128-bit two's-complement constant;
                                       FLS_AGGV_DOUBLE: binary64 bits in lo */
    uint8_t  pad[2];
    uint64_t lo, hi;
} fls_group_having;
#define FLS_GROUP_ORDER_NONE 0xFFFFFFFFu
typedef struct fls_group_select {
    const fls_group_having *having; /* conjunction of nhaving terms, 0 .. 8 */
    uint32_t nhaving;
    uint32_t order_agg;             /* index into aggs[], or FLS_GROUP_ORDER_NONE */
    uint8_t  desc, nulls_first, pad[2];
    uint32_t limit;                 /* 0 = no limit; else 1 .. 1024 */
} fls_group_select;
int fls_aggregate_hashed_select(fls_table *t, const uint32_t *keys, uint32_t nkeys,
                                const fls_aggregate_spec *aggs, uint32_t n, uint64_t max_groups,
                                const fls_group_select *sel,
                                uint32_t rg_begin, uint32_t rg_end, fls_hash_result **out);
int fls_hash_result_select_stats(const fls_hash_result *r, uint64_t *groups_total,
                                 uint64_t *groups_passed, int *on_device, double *select_ms);

/* Key maps: GROUP BY an attribute of a joined dimension table.  A key map is
 * a function from 64-bit keys to 16-bit codes, built on the host from the
 * build side of the join (keys[i] -> values[i], i in [0, n)); bound to a
 * foreign-key column of a fact table, it lets fls_aggregate_grouped name
 * "the code the map gives this column" as a GROUP BY key: the nation of
 * l_suppkey, the priority class of l_orderkey.  No GPU is needed to create a
 * map, query it or prune with it.  keys and kind are a key set's (above);
 * values are codes in [0, 65534]: 0xFFFF marks "absent" inside the image and
 * is refused (FLS_ERR_ARG).  A key listed twice with one value is kept once;
 * with two values the map is no function: FLS_ERR_ARG naming the key and
 * both values.  n = 0 is a valid empty map.
 * form: 0 auto, 1 dense, 2 hash table.
 *   dense: uint16[max - min + 1] indexed by key - min (mod 2^64), holes hold
 *          0xFFFF, padded to 8 bytes; max - min + 1 <= 2^31 (a 4 GiB image).
 *   hash:  the key set's table (8-byte slots, capacity, home slot, ascending
 *          insertion, sentinel and max_probe exactly as documented above),
 *          followed at byte 8 * capacity by uint16[capacity]: the slots'
 *          codes, 0xFFFF in empty slots, padded to 8 bytes.
 *   auto:  dense when max - min + 1 <= 2^31 and the array is no larger than
 *          the hash image (10 bytes per slot, padded) would be, or at most
 *          1 MiB; else the hash table.
 * The image is a pure function of the map, whatever the order of the input.
 * FLS_ERR_LIMIT: n above 2^28 (returned before keys or values is read), a
 * forced dense map spanning more than 2^31 values.
 * Handles are a key set's: opaque counter tokens looked up among the live
 * maps, never dereferenced; a stale, foreign or key-set handle is FLS_ERR_ARG
 * (and a map handle is no key set).  A binding and a running scan hold
 * references, so freeing the handle or disconnecting while they use the map
 * is safe.  The image is uploaded to a GPU by the first batch that probes it
 * there (synchronously, fls_keymap_info.device_bytes per GPU), cached inside
 * the map and freed with its last reference; it does not count against
 * FLS_SCAN_RESIDENT_MB.  One map may serve any number of tables.
 * Not in the reference. */
typedef struct fls_keymap fls_keymap;
typedef enum fls_keymap_form { FLS_KEYMAP_AUTO = 0, FLS_KEYMAP_DENSE = 1, FLS_KEYMAP_HASH = 2 } fls_keymap_form;
typedef struct fls_keymap_info_t {
    uint64_t count;         /* distinct keys */
    uint32_t form;          /* the form chosen: FLS_KEYMAP_DENSE or FLS_KEYMAP_HASH */
    uint32_t kind;          /* fls_keyset_kind */
    uint64_t device_bytes;  /* bytes of the image, per GPU that probes the map */
    uint64_t capacity;      /* hash: slots (0 for a dense map) */
    uint32_t max_probe;     /* hash: longest probe sequence (0 for a dense or an empty map) */
    uint32_t max_code;      /* the largest code (0 for the empty map) */
    uint64_t min, max;      /* patterns, in the map's order (0 for the empty map) */
    uint64_t empty;         /* hash: the empty slot's sentinel */
} fls_keymap_info_t;
int fls_keymap_create(fls_connection *conn, const uint64_t *keys, const uint16_t *values, uint64_t n,
                      int kind /* fls_keyset_kind */, int form, fls_keymap **out);
void fls_keymap_free(fls_keymap *map);
int fls_keymap_info(const fls_keymap *map, fls_keymap_info_t *info);
/* Host probe of the very image a scan uploads: 1 found (*code set), 0 absent. */
int fls_keymap_lookup(const fls_keymap *map, uint64_t key, uint32_t *code);

/* Value maps: the build side of a join whose payload is a value a row is
 * compared with (FLS_CMP_MAP_EQ .. FLS_CMP_MAP_GE above): Q17's per-part
 * quantity threshold, Q2's minimum supply cost, Q21's min / max supplier of an
 * order, an order's date for `l_shipdate > o_orderdate + k`.  A value map is a
 * function from 64-bit keys to 64-bit values, built on the host like a key map
 * (keys[i] -> values[i], i in [0, n)); no GPU is needed to create a map, query
 * it or prune with it.  key_kind and value_kind are each a fls_keyset_kind:
 * the order of the keys (key_min / key_max, pruning) and of the values
 * (value_min / value_max and the comparison).  Every 64-bit pattern is a
 * value, 0 and 2^64 - 1 included.  A key listed twice with one value is kept
 * once; with two values the map is no function: FLS_ERR_ARG naming the key
 * and both values.  n = 0 is a valid empty map.
 * form: 0 auto, 1 dense, 2 hash table.
 *   dense: uint64[max - min + 1] indexed by key - min (mod 2^64), followed by
 *          a presence bitmap uint64[(max - min + 64) / 64] (a 64-bit value
 *          has no spare "absent" pattern: a hole holds value 0 and bit 0);
 *          max - min + 1 <= 2^28.
 *   hash:  the key set's table (8-byte slots, capacity, home slot, ascending
 *          insertion, sentinel and max_probe exactly as documented above),
 *          followed at byte 8 * capacity by uint64[capacity]: the slots'
 *          values, 0 in empty slots.
 *   auto:  dense when max - min + 1 <= 2^28 and the dense image is no larger
 *          than the hash image (16 bytes per slot) would be, or at most
 *          1 MiB; else the hash table.
 * The image is a pure function of the map, whatever the order of the input.
 * FLS_ERR_LIMIT: n above 2^28 (returned before keys or values is read), a
 * forced dense map spanning more than 2^28 keys.
 * Handles are opaque counter tokens looked up among the live value maps,
 * never dereferenced; a stale, foreign, key-set or key-map handle is
 * FLS_ERR_ARG (and a value-map handle is neither a key set nor a key map).  A
 * filter holding a map term and a running scan hold references, so freeing
 * the handle or disconnecting while they use the map is safe.  The image is
 * uploaded to a GPU by the first batch that probes it there (synchronously,
 * fls_valuemap_info.device_bytes per GPU), cached inside the map and freed
 * with its last reference; it does not count against FLS_SCAN_RESIDENT_MB.
 * One map may serve any number of tables.  Not in the reference. */
typedef struct fls_valuemap fls_valuemap;
typedef enum fls_valuemap_form { FLS_VALUEMAP_AUTO = 0, FLS_VALUEMAP_DENSE = 1, FLS_VALUEMAP_HASH = 2 } fls_valuemap_form;
typedef struct fls_valuemap_info_t {
    uint64_t count;         /* distinct keys */
    uint32_t form;          /* the form chosen: FLS_VALUEMAP_DENSE or FLS_VALUEMAP_HASH */
    uint32_t key_kind;      /* fls_keyset_kind of the keys */
    uint32_t value_kind;    /* fls_keyset_kind of the values */
    uint32_t max_probe;     /* hash: longest probe sequence (0 for a dense or an empty map) */
    uint64_t device_bytes;  /* bytes of the image, per GPU that probes the map */
    uint64_t capacity;      /* hash: slots (0 for a dense map) */
    uint64_t key_min, key_max;      /* patterns, in the key kind's order (0 for the empty map) */
    uint64_t value_min, value_max;  /* patterns, in the value kind's order (0 for the empty map) */
    uint64_t empty;         /* hash: the empty slot's sentinel */
} fls_valuemap_info_t;
int fls_valuemap_create(fls_connection *conn, const uint64_t *keys, const uint64_t *values, uint64_t n,
                        int key_kind /* fls_keyset_kind */, int value_kind /* fls_keyset_kind */, int form,
                        fls_valuemap **out);
void fls_valuemap_free(fls_valuemap *map);
int fls_valuemap_info(const fls_valuemap *map, fls_valuemap_info_t *info);
/* Host probe of the very image a scan uploads: 1 found (*value set), 0 absent. */
int fls_valuemap_lookup(const fls_valuemap *map, uint64_t key, uint64_t *value);

/* The build side of a join on the GPU: the map key_col -> value_col over the
 * rows of row groups [rg_begin, rg_end) that the filter and alternatives
 * currently set on the table select and where both columns are non-NULL --
 * the map fls_valuemap_create / fls_keymap_create builds from those pairs,
 * image for image: the same form under the auto rule, every fls_*_info field,
 * every lookup, every image word.  The kinds follow the columns (signed:
 * INT*, DATE, DECIMAL; unsigned: UINT*, BOOLEAN); the map belongs to the
 * table's connection and is used, queried and freed like any other map.
 * The scan decodes the filter's, the alternatives' and the two columns and
 * delivers nothing: on each GPU every selected pair goes into slot key - base
 * of one uint64 array over the union of the key column's zone maps over the
 * row groups that survive pruning (a row group whose key or value chunk is
 * all NULL is skipped) with one atomic minimum per row, which also detects a
 * key with two values exactly (csrc/fls_mapbuild.hip).  The array is then
 * compacted on the GPU, and the host receives (span + 64) / 64 presence words
 * and the distinct keys' values, already in key order, per GPU: never the
 * keys, never a duplicate row, never the array.  That needs
 *   span + 1 <= 2^28 (kValuemapMaxSpan),
 *   an array (8 bytes per value of the range) of at most 1 MiB, or no larger
 *   than the hash image of the surviving row groups' rows would be (the auto
 *   rule's own comparison of the dense form against the hash form), and
 *   a value column that cannot hold the all-ones pattern of its order
 *   (INT64_MAX signed, UINT64_MAX unsigned), which marks an untouched slot:
 *   narrower than 8 bytes, or every surviving row group with a zone map
 *   whose maximum is below it;
 * otherwise FLS_ERR_LIMIT before any device work, the message stating the
 * numbers: build the map from a filtered scan and fls_*map_create.
 * No surviving row group gives the empty map without device work.
 * FLS_ERR_ARG before any device work, naming the column: a mapped column, a
 * column out of range, a VARCHAR / BLOB / FLOAT / DOUBLE column, a DECIMAL
 * wider than 64 bits on either side, a form outside 0..2, a row-group range
 * outside the table.  FLS_ERR_ARG after the scan: a key with two values (the
 * message names one such key and ends "a map is a function"; with several,
 * which one is unspecified); fls_keymap_from_scan: a value outside
 * [0, 65534] (the smallest if it is negative, otherwise the largest).
 * FLS_ERR_FORMAT: a decoded key outside the zone maps that gave the range
 * (it touches nothing).  Not in the reference. */
typedef struct fls_map_build_info_t {
    uint64_t rows_selected;     /* selected rows with key and value both valid */
    uint64_t keys;              /* distinct keys in the finished map */
    uint64_t scratch_bytes;     /* collecting array, per device */
    uint64_t d2h_bytes;         /* everything the build copied to the host */
    uint64_t base, span;        /* collecting range of the key column */
    uint32_t rowgroups_read, rowgroups_pruned;
} fls_map_build_info_t;
int fls_valuemap_from_scan(fls_table *t, uint32_t key_col, uint32_t value_col, uint32_t rg_begin, uint32_t rg_end,
                           int form, fls_valuemap **out, fls_map_build_info_t *info /* may be NULL */);
int fls_keymap_from_scan(fls_table *t, uint32_t key_col, uint32_t value_col, uint32_t rg_begin, uint32_t rg_end,
                         int form, fls_keymap **out, fls_map_build_info_t *info /* may be NULL */);

/* Mapped GROUP BY keys.  fls_aggregate_key_bindings sets the table's bindings
 * (copied and replaced as a whole; n <= 4; n = 0 clears; sticky like
 * fls_aggregate_exprs): binding i says "probe map with column col".  In the
 * following fls_aggregate_grouped calls keys[q] = FLS_KEY_MAPPED | i means the
 * code binding i's map gives its column; bindings no key names are ignored.
 * A mapped key comes back as FLS_KEYV_INT with the code in lo (or
 * FLS_KEYV_NULL), takes 16 value bits and one NULL bit of the 128-bit packed
 * key, counts towards the 4 keys, and mixes with plain and VARCHAR keys in any
 * order; its column may also be a plain key, an operand or a filter column.
 * Default (inner join): a selected row whose column is NULL or whose value is
 * not in the map belongs to no group and counts nowhere, exactly as if the
 * filter carried `col IN keys(map)` as one more clause; the key is never NULL.
 * Row groups are pruned as under IN_SET (a zone map without a map key in
 * [min, max], an all-NULL chunk; the empty map prunes everything: zero groups,
 * no device work) and count in fls_scan_pruned.
 * FLS_KEYMAP_KEEP_UNMATCHED (left join): those rows form the NULL group, like
 * a NULL plain key, and nothing is pruned.
 * The codes are probed on the GPU per selected row (csrc/fls_keymap.hip) into
 * a derived 2-byte key column in HBM; everything fls_aggregate_grouped
 * promises -- first-occurrence order, the 64 / 256 distinct-key limits, values
 * bit-identical across batch size, slot and GPU count, one group equal to
 * fls_aggregate under the equivalent IN_SET filter -- holds unchanged.
 * FLS_ERR_ARG before any device work.  The setter, naming "binding i":
 * n > 4, a column out of range, a VARCHAR / BLOB / FLOAT / DOUBLE column or a
 * DECIMAL wider than 64 bits, a map whose kind differs from the column's
 * signedness, a handle that is not a live map, unknown flag bits.
 * fls_aggregate_grouped, naming "key q": FLS_KEY_MAPPED | i with no binding
 * i, and a binding named by two keys.  Not in the reference. */
#define FLS_KEY_MAPPED 0x80000000u     /* keys[q] = FLS_KEY_MAPPED | i : binding i of the table */
#define FLS_KEYMAP_KEEP_UNMATCHED 1u   /* left join: unmatched rows form the NULL group */
typedef struct fls_key_binding { uint32_t col; uint32_t flags; uint64_t map; /* the fls_keymap handle */ } fls_key_binding;
int fls_aggregate_key_bindings(fls_table *t, const fls_key_binding *b, uint32_t n);

/* Mapped columns: the join's payload itself.  fls_aggregate_value_bindings
 * sets the table's value bindings (copied and replaced as a whole; n <= 4;
 * n = 0 clears; sticky like fls_aggregate_key_bindings): binding i says "probe
 * value map `map` with column col".  The mapped column map[col] is a 64-bit
 * integer column, signed or unsigned by the map's value_kind, NULL at a row
 * where col is NULL or its value is not in the map.  In the following calls
 * FLS_COL_MAPPED | i names it
 *   - as fls_aggregate_spec.col / .col2 of COUNT, SUM, MIN, MAX and
 *     SUM_PRODUCT in fls_aggregate, fls_aggregate_grouped and
 *     fls_aggregate_hashed[_select], with or without a condition (spec.cond),
 *     and under HAVING / ORDER BY over such an aggregate: SUM is the exact
 *     128-bit sum, MIN / MAX come back as FLS_AGGV_INT sign- or zero-extended
 *     by value_kind, sum(l_quantity * cost[l_partkey]) is a SUM_PRODUCT;
 *   - as fls_agg_factor.col of fls_aggregate_exprs (k in the map's value unit);
 *   - as keys[q] of fls_aggregate_hashed[_select] (GROUP BY cust[l_orderkey]):
 *     the key's range is the map's [value_min, value_max] instead of zone
 *     maps, plus the NULL bit (an empty map: 0 value bits); fls_hash_result_key
 *     returns the mapped value, is_null the NULL group of a keep-unmatched
 *     binding.  The packed key still holds at most 63 bits.
 * Default (inner join), exactly as a key-map binding: a selected row whose
 * mapped value is NULL leaves the scan's selection, so count(*) and every
 * other aggregate of the call loses it; row groups are pruned as under IN_SET
 * on the map's keys (an all-NULL chunk, a zone map without a map key; an empty
 * map prunes everything: zero groups, NULL sums, no device work) and count in
 * fls_scan_pruned.  FLS_VALUEMAP_KEEP_UNMATCHED (left join): the selection is
 * left alone and nothing is pruned; the mapped column is simply NULL there:
 * operands skip the row, COUNT(mapped) does not count it, as a hash key it
 * forms the NULL group.
 * Only the bindings a call names are probed: a binding that is set but unused
 * narrows nothing and prunes nothing, so every call that names none behaves as
 * if none were set.  Each binding holds a reference to its map: freeing the
 * handle before the scan is fine.  The values are gathered on the GPU per
 * selected row (csrc/fls_mapval.hip) into a derived 8-byte column in HBM,
 * which the reduce kernels read like any other; the bit is 0x40000000 so that
 * FLS_KEY_MAPPED keeps its meaning in fls_aggregate_grouped's keys.
 * The overflow bounds of SUM_PRODUCT and SUM_EXPR take max(|value_min|,
 * |value_max|) of the map for a mapped operand (0 for an empty map).
 * FLS_ERR_ARG before any device work.  The setter, naming "value binding i":
 * n > 4, a column out of range, a VARCHAR / BLOB / FLOAT / DOUBLE column or a
 * DECIMAL wider than 64 bits, a map whose key kind differs from the column's
 * signedness, a handle that is not a live value map (a key-set or key-map
 * handle does not resolve), unknown flag bits.  The calls, naming "aggregate
 * i", "expression i" or "key q": FLS_COL_MAPPED | i with no binding i, the
 * same binding as two hash keys, and FLS_COL_MAPPED anywhere else: a key of
 * fls_aggregate_grouped (a key map gives low-cardinality mapped keys),
 * fls_topn's order key, a filter, condition or alternative term's col /
 * key_col, fls_keyset_from_scan's column.  A delivered column cannot name one:
 * col_mask holds a byte per table column, so the bit has no place there (the
 * Python column lists refuse it by name).  Not in the reference. */
#define FLS_COL_MAPPED 0x40000000u            /* col = FLS_COL_MAPPED | i : value binding i of the table */
#define FLS_VALUEMAP_KEEP_UNMATCHED 1u        /* left join: the mapped column is NULL at unmatched rows */
typedef struct fls_value_binding { uint32_t col; uint32_t flags; uint64_t map; /* the fls_valuemap handle */ } fls_value_binding;
int fls_aggregate_value_bindings(fls_table *t, const fls_value_binding *b, uint32_t n);
/* ORDER BY key [DESC] LIMIT k selected on the GPU: the k best rows of row
 * groups [rg_begin, rg_end) under the filter set by fls_scan_filter, ordered
 * by one key column; their global row indices and the values of the columns
 * col_mask names (NULL = every column; the key column only if masked in).
 * Phase 1 decodes the filter's columns and the key column into HBM, keeps the
 * best k candidates of every 1024-row vector and merges them per row group
 * (csrc/fls_topn.hip); one list of at most k 16-byte records per row group
 * crosses PCIe, and the call merges the row groups' lists.  Phase 2 decodes
 * the masked columns of the at most k row groups that hold a winner, as
 * fls_materialize does, and copies the winners' values out; the call is
 * synchronous.  Key column: INT*, UINT*, BOOLEAN, DATE, DECIMAL of at most 64
 * bits, FLOAT or DOUBLE in any encoding.  Integers order by value, floats in
 * the filter's order (every NaN above +inf, -0 equal to +0); desc inverts the
 * order.  NULL keys come after every value in both directions (DuckDB's
 * default, NULLS LAST) or, with nulls_first, before every value; the
 * placeholder stored at a NULL is never read.  Equal keys (-0 / +0 and NaN /
 * NaN included) are ordered by ascending global row index, so the result is
 * unique, and identical whatever the batch size, slot count or number of
 * GPUs.  A row takes part when the filter selects it.  Fewer than k such rows
 * give that many; none at all (an empty table or range, every row group
 * pruned, k = 0) give an empty result with no device work.  k <= 1024 (one
 * vector's worth): a larger k is FLS_ERR_LIMIT before any device work; scan
 * and sort instead.  Without a filter and with an integer-like key, row
 * groups whose zone map puts every value strictly behind the k-th bound the
 * other row groups' zone maps guarantee are not read (ties and row groups
 * without a zone map are; a row group with a NULL is kept under nulls_first);
 * they count in fls_scan_pruned.  FLOAT / DOUBLE keys and filtered calls are
 * not pruned this way (a filter prunes as in fls_scan_begin).
 * FLS_ERR_ARG before any device work, the message starting "order key:": a
 * key column out of range, a VARCHAR / BLOB key, a DECIMAL wider than 64
 * bits, a col_mask that names no column, rg_begin / rg_end out of bounds.
 * The call replaces a scan in progress on the table, as fls_aggregate does,
 * and the table stays usable after any error.  Not in the reference.
 * *out is owned by the caller (fls_topn_result_free) and stays valid after
 * the table is closed: values, validity and strings are copies. */
typedef struct fls_order_key { uint32_t col; uint8_t desc; uint8_t nulls_first; uint8_t pad[2]; } fls_order_key;
typedef struct fls_topn_result fls_topn_result;
int fls_topn(fls_table *t, const fls_order_key *key, uint32_t k, const uint8_t *col_mask,
             uint32_t rg_begin, uint32_t rg_end, fls_topn_result **out);
uint64_t fls_topn_result_nrows(const fls_topn_result *r);
/* global row indices, in result order */
const uint64_t *fls_topn_result_rows(const fls_topn_result *r);
/* nrows values of a delivered column in the scan's physical layout
 * (fls_column_info.out_bytes per row; VARCHAR / BLOB as 16-byte string_t
 * records whose long strings point into bytes the result owns) and their
 * validity in DuckDB's layout, or NULL when every returned row is valid.
 * FLS_ERR_ARG for a column that was not delivered. */
int fls_topn_result_column(const fls_topn_result *r, uint32_t col, const void **values,
                           const uint64_t **validity);
/* Host-clock milliseconds the call spent in phase 1 (the selection scan and
 * the merge) and in phase 2 (the late materialisation); either may be NULL. */
int fls_topn_result_times(const fls_topn_result *r, double *phase1_ms, double *phase2_ms);
void fls_topn_result_free(fls_topn_result *r);
/* Host only, of the fls_rowgroup_may_match family: the number of row groups of
 * [rg_begin, rg_end) an fls_topn call with this key and k would not read
 * under the filter currently set (what fls_scan_pruned reports after it);
 * fls_topn's argument checks apply. */
int fls_topn_pruned(const fls_table *t, const fls_order_key *key, uint32_t k, uint32_t rg_begin, uint32_t rg_end);
/* Zone map of column col in row group rg: 1 and *min / *max (int64, uint64
 * or double bits by column type, see fls_predicate.value; FLOAT widened to
 * double) and *flags (1 valid, 2 / 4 has / all NaN, 8 / 16 has / all NULL;
 * min / max over the non-NULL rows) when present, 0 when the file has none
 * for it. */
int fls_table_zonemap(const fls_table *t, uint32_t rg, uint32_t col, uint64_t *min, uint64_t *max, uint32_t *flags);
/* Dictionary-coded delivery for the next fls_scan_begin (enable != 0): a
 * delivered VARCHAR / BLOB column no filter term reads, whose chunks in a
 * batch are all DICT, crosses PCIe as 1- or 2-byte codes instead of 16-byte
 * string_t records (fls_rowgroup.dict / dict_width); what a DuckDB
 * dictionary vector needs.  Off by default. */
int fls_scan_dict_codes(fls_table *t, int enable);
/* Narrowed delivery for the next fls_scan_begin (enable != 0): a delivered
 * integer / DATE / DECIMAL column whose zone maps put every value of a
 * batch's row groups within 2^8, 2^16 or 2^32 of its row group's minimum
 * crosses PCIe as the 1-, 2- or 4-byte difference (fls_rowgroup.narrow /
 * narrow_base); the consumer adds the base back while filling its vectors.
 * Off by default. */
int fls_scan_narrow(fls_table *t, int enable);
/* With fls_scan_narrow (FLS_SCAN_STRLEN, default 1; 0 ships string_t
 * records instead: the lengths measured 7.81e8 against 6.78e8 rows/s on the
 * link-bound 16-thread read_fastlanes, profiles/r4/e2e_arms_strlen_r4t.txt),
 * an unfiltered scan also delivers FSST string columns
 * as their lengths (1, 2 or 4 bytes per row) plus the string heap, and the
 * string_t records are rebuilt on the host; fls_rowgroup shows them as
 * ordinary string_t columns.  fls_scan_acquire builds them unless
 * fls_scan_defer_records(t, 1) was set before fls_scan_begin: then the
 * consumer calls fls_scan_build_records(t, &rg) for each acquired row group
 * before reading its string columns (so a consumer that serialises its
 * acquires builds them in parallel, outside its lock). */
int fls_scan_defer_records(fls_table *t, int enable);
int fls_scan_build_records(fls_table *t, const fls_rowgroup *rg);
/* Validity of column col in row group rg: 1 and *words = its bitmaps in the
 * host image (16 u64 words per 1024-row vector, DuckDB's layout: bit i of
 * word j set when row 64 j + i is valid) when the chunk holds a NULL, 0 (and
 * *words = NULL) when every row is valid.  Valid while the table is open;
 * for consumers of the device-resident columns (fls_device_column). */
int fls_table_validity(const fls_table *t, uint32_t rg, uint32_t col, const uint64_t **words);
/* May a row of row group rg satisfy the filter?  (1 yes / 0 no; host only) */
int fls_rowgroup_may_match(const fls_table *t, uint32_t rg, const fls_predicate *preds, uint32_t n);

/* Thread-safe form for parallel consumers: claims the next row group in order
 * (1 = delivered, 0 = end, <0 = error); its buffers stay valid until
 * fls_scan_release(t, out->rowgroup), so a consumer may keep several row
 * groups (DuckDB vectors referencing the pinned columns, zero-copy).  A GPU's
 * batch slot is refilled as soon as every row group of its batch has been
 * handed out; the pinned host side of a batch goes back to a per-GPU pool when
 * its last row group is released (pool cap FLS_SCAN_HOST_BATCHES, default 64;
 * at the cap a refill waits for a release).  A failed refill is sticky: every
 * later acquire returns its error.  Do not mix with fls_scan_next on one scan. */
int fls_scan_acquire(fls_table *t, fls_rowgroup *out);
int fls_scan_release(fls_table *t, uint32_t rowgroup);

/* ---- device-resident mode (HBM roofline measurement, bench.py) ---------
 * Upload row groups [rg_begin, rg_end) of the table to HBM, split into
 * contiguous parts over the connection's GPUs (as a scan shards them; a GPU
 * gets no part when there are fewer row groups than GPUs), and allocate HBM
 * output columns for them. */
int fls_device_upload(fls_table *t, uint32_t rg_begin, uint32_t rg_end);
/* Enqueue ONE decode launch per GPU over every resident vector of the
 * selected columns (col_mask NULL = all) into HBM.  Asynchronous: the parts
 * decode concurrently. */
int fls_device_decode(fls_table *t, const uint8_t *col_mask);
/* Wait for the table's GPU work; fills *stats if non-NULL: values and bytes
 * summed over the parts, kernel_ms = the last launch, kernel_ms_total over the
 * launches since the previous sync, a launch timed as its slowest part. */
int fls_device_sync(fls_table *t, fls_decode_stats *stats);

typedef struct {
    int device;               /* HIP ordinal */
    uint32_t rg_begin, rg_end;
    uint64_t first_row;       /* first resident row, relative to the table's first row */
    uint64_t nrows;
} fls_device_part_info;
/* Number of resident parts (GPUs holding row groups) and each one's extent. */
int fls_device_parts(const fls_table *t);
int fls_device_part(const fls_table *t, uint32_t part, fls_device_part_info *out);
/* HBM address and byte size of a resident output column of one part. */
int fls_device_part_column(fls_table *t, uint32_t part, uint32_t col, void **dev_ptr, uint64_t *nbytes);
/* String heap of a part's resident FSST VARCHAR column (see fls_device_heap). */
int fls_device_part_heap(fls_table *t, uint32_t part, uint32_t col, void **dev_ptr, const void **host_ptr,
                         uint64_t *nbytes);
/* HBM address and byte size of a resident output column (single-part tables;
 * FLS_ERR_STATE when the table is split over several GPUs). */
int fls_device_column(fls_table *t, uint32_t col, void **dev_ptr, uint64_t *nbytes);
/* String heap of a resident FSST (free-text) VARCHAR column: its HBM address,
 * the host address the column's string_t pointers are based on (the heap's
 * host copy, filled by fls_device_copy_out) and its size.  Returns 1, or 0
 * (pointers NULL) for a column without one. */
int fls_device_heap(fls_table *t, uint32_t col, void **dev_ptr, const void **host_ptr, uint64_t *nbytes);
/* Copy rows [row, row+n) (relative to the first resident row, counted over
 * the parts in order) of a decoded column into host memory. */
int fls_device_copy_out(fls_table *t, uint32_t col, uint64_t row, uint64_t n, void *host_dst);
/* Rows resident on the GPUs (all parts). */
uint64_t fls_device_rows(const fls_table *t);

#ifdef __cplusplus
}
#endif
#endif
