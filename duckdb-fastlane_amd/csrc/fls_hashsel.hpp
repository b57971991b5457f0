// fls_hashsel.hpp -- choosing among the groups of a hash aggregate where they
// lie (fls_aggregate_hashed_select): HAVING terms and ORDER BY one aggregate
// LIMIT k over the table hash_insert_kernel left in HBM (fls_hashagg.hpp), so
// that only the chosen groups are compacted, copied and unpacked.
//
// Everything compares a slot's raw fields in their stored form.  The host
// translates each constant once (fls_scan_hashagg.hip): a count and a MAX are
// stored as they order (MAX as agg_key_int / agg_key_float or the plain
// unsigned value), a MIN as that key's complement -- the constant is
// complemented and the operator mirrored -- and a sum as a 128-bit
// two's-complement pair.  A constant outside what a field can hold has become
// HV_ALWAYS / HV_NEVER before a kernel sees it.  An aggregate that is NULL
// (its count field is 0) satisfies no term.
//
// Result order: records compare as (rank, key hi, key lo, first row), smaller
// is better.  rank places the NULL aggregates, the key is the aggregate as a
// 128-bit unsigned number in its order (inverted for DESC), and first rows
// are distinct across groups: no two records compare equal, so the best k are
// one fixed list whatever computes them.  having_pass, order_key and rec_less
// are the device's and the host's alike: the several-pipeline fallback applies
// them to the merged groups.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fls_hashagg.hpp"

namespace fls {

constexpr uint32_t kMaxHaving = 8;       // terms of one call
constexpr uint32_t kMaxGroupLimit = 1024;  // limit of one call: one block sorts that many records in LDS
constexpr uint32_t kHashHdrSelected = 2;   // header word group_select_kernel counts its survivors in
constexpr uint16_t kNoField = 0xFFFF;

enum HavingMode : uint8_t {
    HV_U64 = 0,     // field `val` against clo, unsigned
    HV_S128 = 1,    // fields (hi, val) against (chi, clo), signed 128-bit
    HV_ALWAYS = 2,  // holds for every group whose aggregate is not NULL
    HV_NEVER = 3,
};

struct DevHaving {            // 24 B
    uint64_t clo, chi;        // the constant in the field's stored form
    uint16_t val, hi;         // table fields (hi: HV_S128 only)
    uint16_t null_cnt;        // the count field that is 0 for a NULL aggregate, or kNoField: never NULL
    uint8_t op;               // FLS_CMP_EQ .. FLS_CMP_GE, in the stored form's order
    uint8_t mode;             // HavingMode
};
static_assert(sizeof(DevHaving) == 24, "DevHaving is 24 B");

enum OrderForm : uint8_t {
    OF_NONE = 0,    // no order: first rows alone (LIMIT without ORDER BY)
    OF_U64 = 1,     // field `val` orders unsigned as stored (counts, MAX)
    OF_NOT64 = 2,   // its complement does (MIN)
    OF_S128 = 3,    // (hi, val) signed 128-bit (sums)
};

struct DevGroupSelect {       // passed by value
    DevHaving having[kMaxHaving];
    uint32_t nhaving;
    uint16_t oval, ohi, onull;  // the ordering aggregate's fields, as DevHaving's
    uint8_t oform;            // OrderForm
    uint8_t desc, nulls_first;
    uint8_t want_recs;        // an order or a limit is set: candidate records instead of the slot list
    uint8_t pad[2];
};

struct GroupRec {             // 32 B: a candidate of the top-k
    uint64_t khi, klo;        // the order key
    uint64_t first;           // the group's first row
    uint32_t slot;            // its slot of the table
    uint32_t rank;            // 0 before 1
};
static_assert(sizeof(GroupRec) == 32, "GroupRec is 32 B");

__host__ __device__ inline bool cmp_holds(uint8_t op, int c) {  // c: -1 / 0 / 1 of value against constant
    switch (op) {
    case 0: return c == 0;   // FLS_CMP_EQ
    case 1: return c != 0;   // FLS_CMP_NE
    case 2: return c < 0;    // FLS_CMP_LT
    case 3: return c <= 0;   // FLS_CMP_LE
    case 4: return c > 0;    // FLS_CMP_GT
    default: return c >= 0;  // FLS_CMP_GE
    }
}

// Does the group whose field f is get(f) satisfy term h?
template <class Get>
__host__ __device__ inline bool having_pass(const DevHaving &h, Get get) {
    if (h.null_cnt != kNoField && get(h.null_cnt) == 0) return false;
    if (h.mode == HV_ALWAYS) return true;
    if (h.mode == HV_NEVER) return false;
    const uint64_t lo = get(h.val);
    int c;
    if (h.mode == HV_S128) {
        const int64_t a = (int64_t)get(h.hi), b = (int64_t)h.chi;
        c = a != b ? (a < b ? -1 : 1) : (lo != h.clo ? (lo < h.clo ? -1 : 1) : 0);
    } else {
        c = lo != h.clo ? (lo < h.clo ? -1 : 1) : 0;
    }
    return cmp_holds(h.op, c);
}

template <class Get>
__host__ __device__ inline bool having_all(const DevGroupSelect &p, Get get) {
    bool ok = true;
    for (uint32_t j = 0; j < p.nhaving; ++j) ok = ok && having_pass(p.having[j], get);
    return ok;
}

// The group's candidate record but for its first row and slot.
template <class Get>
__host__ __device__ inline void order_key(const DevGroupSelect &p, Get get, GroupRec &r) {
    r.khi = r.klo = 0;
    r.rank = 0;
    if (p.oform == OF_NONE) return;
    const uint32_t null_rank = p.nulls_first ? 0u : 1u;
    if (p.onull != kNoField && get(p.onull) == 0) {
        r.rank = null_rank;
        return;
    }
    r.rank = 1u - null_rank;
    uint64_t lo = get(p.oval), hi = 0;
    if (p.oform == OF_NOT64) lo = ~lo;
    if (p.oform == OF_S128) hi = get(p.ohi) ^ (1ull << 63);
    r.khi = p.desc ? ~hi : hi;
    r.klo = p.desc ? ~lo : lo;
}

__host__ __device__ inline bool rec_less(uint32_t ra, uint64_t ha, uint64_t la, uint64_t fa, uint32_t rb, uint64_t hb,
                                         uint64_t lb, uint64_t fb) {
    if (ra != rb) return ra < rb;
    if (ha != hb) return ha < hb;
    if (la != lb) return la < lb;
    return fa < fb;
}
__host__ __device__ inline bool rec_less(const GroupRec &a, const GroupRec &b) {
    return rec_less(a.rank, a.khi, a.klo, a.first, b.rank, b.khi, b.klo, b.first);
}

// Records the top-k's level `level` keeps of `total` candidates in list j: a
// list covers 1024 << level consecutive candidates and keeps its best k.
__host__ __device__ inline uint32_t topk_list_count(uint64_t total, uint32_t k, uint32_t level, uint64_t j) {
    const uint64_t span = 1024ull << level, start = j * span;
    if (start >= total) return 0;
    const uint64_t n = total - start < span ? total - start : span;
    return (uint32_t)(n < k ? n : k);
}

// Walks the table's `cap` slots.  Every occupied slot that satisfies the terms
// is appended -- header word kHashHdrSelected counts them, entries at or past
// nmax are dropped -- to d_slots (its slot index), or with p.want_recs to
// d_recs (its candidate record).  The header word must be 0 before.
hipError_t launch_group_select(const DevGroupSelect &p, uint64_t *d_table, uint64_t cap, uint32_t *d_slots,
                               GroupRec *d_recs, uint64_t nmax, hipStream_t stream);
// The best min(k, total) of d_recs[0..total) in result order into d_out[0..).
// d_a and d_b hold ceil(total / 1024) and ceil(total / 2048) lists of k records
// (topk_lists_bytes).
hipError_t launch_group_topk(const GroupRec *d_recs, uint64_t total, uint32_t k, GroupRec *d_a, GroupRec *d_b,
                             GroupRec *d_out, hipStream_t stream);
// out[f * nout + i] = field f of slot d_slots[i] (d_recs[i].slot where d_slots is NULL), i below nout.
hipError_t launch_group_gather(const uint64_t *d_table, uint64_t cap, uint32_t nfields, const uint32_t *d_slots,
                               const GroupRec *d_recs, uint64_t nout, uint64_t *d_out, hipStream_t stream);

}  // namespace fls
