// fls_hashagg.hpp -- hash aggregates over a decoded scan batch in HBM
// (fls_aggregate_hashed): fls_agg.hpp's integer functions and MIN / MAX per
// group of a GROUP BY over 1 to 4 integer-like key columns of any cardinality.
//
// Unlike the grouped call's per-vector tables (fls_groupagg.hpp) the groups
// live in one open-addressing table in HBM per scan pipeline, which persists
// across the batches of the scan and is updated with relaxed device-scope
// atomics by every batch's hash_insert_kernel; hash_extract_kernel compacts
// the occupied slots once the scan's streams have drained.
//
// Packed key (<= 63 bits): key q's value minus the smallest value its zone
// maps allow, at bit DevHashKey::shift, and one NULL bit per key at
// DevHashKey::null_bit.  A NULL row sets the NULL bit and leaves the value
// bits 0: the placeholder stored there is never loaded.  Bit 63 is always
// set, so a stored key is never 0: 0 marks an empty slot, and a slot is
// claimed by one 64-bit compare-and-swap.
//
// Table (uint64 words): kHashHdrWords of header -- word 0 the number of
// claimed slots, word 1 hash_extract_kernel's output cursor -- then one array
// of `cap` words per field: field 0 the packed keys, field 1 the complement
// of each group's first selected table row, then per aggregate only what it
// needs: its count, `lo` (sums, MIN / MAX) and `hi` (sums).  Every field's
// identity is 0 (MIN and the first row are kept as the maximum of the
// complement), so one memset initialises the table.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fls_agg.hpp"
#include "fls_groupagg.hpp"

namespace fls {

constexpr uint32_t kHashKeyBits = 63;             // the packed key; bit 63 marks a used slot
constexpr uint64_t kMaxHashGroups = 1ull << 28;   // max_groups of one call
constexpr uint32_t kHashHdrWords = 16;
constexpr uint32_t kHashFieldKeys = 0, kHashFieldFirst = 1, kHashFieldAggs = 2;

// device error flags (after KERR_KEYMAP, fls_groupagg.hpp)
enum : uint32_t {
    KERR_HASH_LIMIT = 2048,   // more distinct keys than max_groups, or no free slot: the row was dropped
    KERR_HASH_RANGE = 4096,   // a decoded key value outside the range its zone maps give
};

struct DevHashKey {           // 40 B
    const uint8_t *col;       // decoded key column of the batch in HBM
    const uint64_t *valid;    // validity words for the batch rows (HBM), or NULL: no NULL in the batch
    uint64_t min;             // the smallest value (sign-extended pattern of a signed column)
    uint64_t span;            // the largest value - min
    uint8_t ob;               // bytes per decoded value: 1, 2, 4 or 8
    uint8_t sign;             // values sign-extend to 64 bits
    uint8_t shift;            // bit of the packed key the value starts at
    uint8_t null_bit;         // bit of the packed key that marks NULL
    uint8_t pad[4];
};
static_assert(sizeof(DevHashKey) == 40, "DevHashKey is 40 B");

// The table fields of one aggregate (0: it has none of that kind).
struct DevHashFields {        // 8 B
    uint16_t count, lo, hi, pad;
};
static_assert(sizeof(DevHashFields) == 8, "DevHashFields is 8 B");

// What a batch's descriptor block holds after the DevAgg array's copy
// (sl.d_adesc): the keys, then the aggregates' fields.
constexpr size_t hash_desc_bytes() { return kMaxKeys * sizeof(DevHashKey) + kMaxAggs * sizeof(DevHashFields); }

// Words of a table of `cap` slots with nfields fields.
constexpr uint64_t hash_table_words(uint64_t cap, uint32_t nfields) { return kHashHdrWords + cap * nfields; }

// The slot a packed key starts probing at (cap a power of two); linear probing
// from there.  The host merge never needs it: it is the kernels' alone.
__host__ __device__ inline uint64_t hash_slot(uint64_t key, uint64_t cap) {
    key ^= key >> 33;
    key *= 0xFF51AFD7ED558CCDull;
    key ^= key >> 33;
    key *= 0xC4CEB9FE1A85EC53ull;
    key ^= key >> 33;
    return key & (cap - 1);
}

// Inserts the batch's selected rows into the table and accumulates their
// aggregates.  d_mask: filter_kernel's selection words (16 per vector), or
// nullptr = every row below nrows.  first_row: the table row index of the
// batch's row 0.  combine: merge runs of equal keys in adjacent lanes before
// the atomics.
hipError_t launch_hash_insert(const DevHashKey *d_keys, uint32_t nkeys, const DevAgg *d_aggs,
                              const DevHashFields *d_fields, uint32_t naggs, uint32_t nrows, const uint64_t *d_mask,
                              uint64_t first_row, uint64_t *d_table, uint64_t cap, uint32_t max_groups, bool combine,
                              uint32_t *d_err, hipStream_t stream);
// Appends every occupied slot's fields to d_out[field * nout + i], i below
// nout, in unspecified order; header word 1 counts them.
hipError_t launch_hash_extract(uint64_t *d_table, uint64_t cap, uint32_t nfields, uint64_t *d_out, uint64_t nout,
                               hipStream_t stream);

}  // namespace fls
