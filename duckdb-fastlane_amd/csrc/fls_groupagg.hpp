// fls_groupagg.hpp -- grouped aggregates over a decoded scan batch in HBM
// (fls_aggregate_grouped): fls_agg.hpp's seven functions per group of a
// low-cardinality GROUP BY over 1 to 4 key columns.
//
// Two launches per batch, no global atomics on data, nothing shared between
// blocks.  Stage 1 (one block per 1024-row vector) finds the vector's distinct
// packed keys in first-occurrence order and reduces every aggregate per key
// with fls_agg.hip's reduction order; stage 2 (one block per row group) merges
// the vectors' keys, in vector order, into the row group's table and folds
// their records.  The host merges the row groups' tables by key VALUE
// (fls_scan_agg.hip): a dictionary code means a string of its row group only.
//
// Packed key (<= 128 bits): key q's value -- the decoded column's raw bytes,
// or a DICT VARCHAR chunk's code in 16 bits -- at bit DevKey::shift, and one
// NULL bit per key at DevKey::null_bit.  A NULL row sets the NULL bit and
// leaves the value bits 0: the placeholder stored there is never loaded.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fls_agg.hpp"

namespace fls {

constexpr uint32_t kMaxKeys = 4;
constexpr uint32_t kMaxVecGroups = 64;   // distinct keys among one vector's selected rows
constexpr uint32_t kMaxRgGroups = 256;   // ... among one row group's

// device error flags (after KERR_NARROW, fls_filter.hpp)
enum : uint32_t { KERR_GROUP_VEC = 128, KERR_GROUP_RG = 256 };

struct DevKey {               // 32 B
    const uint8_t *col;       // decoded key column of the batch in HBM: values, or dictionary codes
    const uint64_t *valid;    // validity words for the batch rows (HBM), or NULL: no NULL in the batch
    uint8_t ob;               // bytes per decoded value / code: 1, 2, 4 or 8
    uint8_t shift;            // bit of the packed key the value starts at
    uint8_t null_bit;         // bit of the packed key that marks NULL
    uint8_t pad[13];
};
static_assert(sizeof(DevKey) == 32, "DevKey is 32 B");

struct GroupHdr {             // 16 B
    uint32_t ngroups;         // used slots
    uint32_t overflow;        // != 0: a capacity was exceeded, the slots are meaningless
    uint64_t pad;
};
static_assert(sizeof(GroupHdr) == 16, "GroupHdr is 16 B");

// Stage 1 output of one vector: GroupHdr, kMaxVecGroups keys (lo, hi), then
// AggRec[slot][aggregate].  Only the used slots are written.
constexpr size_t group_vec_stride(uint32_t naggs) {
    return sizeof(GroupHdr) + 16ull * kMaxVecGroups + (size_t)kMaxVecGroups * naggs * sizeof(AggRec);
}
// Stage 2 output of one row group (what crosses the link): GroupHdr,
// kMaxRgGroups keys, AggRec[slot][aggregate], then -- a binary64 sum folded
// per row group would not add up in the ungrouped call's order, vector after
// vector over the whole table -- the vectors' partial sums of every FLOAT /
// DOUBLE SUM: double[slot][float sum][vector of the row group], -0.0 where the
// group has no contributing row.
constexpr size_t group_rg_recs_off() { return sizeof(GroupHdr) + 16ull * kMaxRgGroups; }
constexpr size_t group_rg_fvec_off(uint32_t naggs) {
    return group_rg_recs_off() + (size_t)kMaxRgGroups * naggs * sizeof(AggRec);
}
constexpr size_t group_rg_stride(uint32_t naggs, uint32_t nfsum, uint32_t rg_vecs) {
    return group_rg_fvec_off(naggs) + 8ull * kMaxRgGroups * nfsum * rg_vecs;
}

// One mapped key (fls_aggregate_key_bindings) as keymap_kernel sees it,
// rebuilt per scan batch; the map's image (fls_keymap.hpp) lives in HBM with
// the map.  The kernel writes the code of every selected, valid row's value
// into `code`, which stage 1 then reads as a 2-byte key column.
struct DevMapTerm {           // 80 B
    const uint8_t *col;       // decoded column of the batch in HBM (row 0 of the batch)
    const uint64_t *valid;    // the column's validity words for the batch rows (HBM), or NULL
    const uint64_t *table;    // dense: uint16 codes; hash: the slots, then their uint16 codes
    uint16_t *code;           // the derived key column: one code per batch row (HBM)
    uint64_t *kvalid;         // keep-unmatched: the derived key's validity words, 16 per vector
    uint64_t min, span;       // dense: code (value - min) for value - min <= span
    uint64_t empty;           // hash: the empty slot's sentinel
    uint32_t cap_log2;        // hash: log2 of the capacity
    uint32_t max_probe;       // hash: slots a lookup examines at most
    uint8_t form;             // KM_DENSE / KM_HASH
    uint8_t ob, sign;         // bytes per decoded value; values sign-extend to 64 bits
    uint8_t keep;             // keep-unmatched (left join): the mask is left alone
    uint8_t pad[4];
};
static_assert(sizeof(DevMapTerm) == 80, "DevMapTerm is 80 B");
// a key-map descriptor no sound map produces (the probe loop itself is bounded)
enum : uint32_t { KERR_KEYMAP = 1024 };
// Probes the bindings' maps under the mask launch_filter / launch_keyset wrote
// for the same nrows rows, narrows it by the inner bindings and recomputes the
// counts (fls_keymap.hip).
hipError_t launch_keymap(const DevMapTerm *d_terms, uint32_t nterms, uint32_t nrows, uint64_t *d_mask,
                         uint32_t *d_counts, uint32_t *d_err, hipStream_t stream);

// Stage 1.  d_aggs[a].fslot numbers the FLOAT / DOUBLE sums (stage 2 reads it).
hipError_t launch_group_vectors(const DevKey *d_keys, uint32_t nkeys, const DevAgg *d_aggs, uint32_t naggs,
                                uint32_t nrows, const uint64_t *d_mask, uint8_t *d_vec_out, uint32_t *d_err,
                                hipStream_t stream);
// Stage 2.  d_rgvec: per row group of the batch its first vector and its
// vector count (<= rg_vecs).
hipError_t launch_group_rowgroups(const DevAgg *d_aggs, uint32_t naggs, uint32_t nfsum, const uint32_t *d_rgvec,
                                  uint32_t nrg, uint32_t rg_vecs, const uint8_t *d_vec_out, uint8_t *d_rg_out,
                                  uint32_t *d_err, hipStream_t stream);

}  // namespace fls
