// fls_topn.hpp -- ORDER BY key [DESC] LIMIT k selected over a decoded scan
// batch in HBM (fls_topn): the k best rows under the pushed-down filter's
// selection mask, by one key column.
//
// A candidate is a 16-byte record {key, row, rank}: `key` is the column's
// order key (agg_key_int / agg_key_float of fls_agg.hpp: unsigned comparison
// is the column's order, every NaN one key above +inf, -0 and +0 one key),
// inverted for DESC; `rank` places the NULL keys (0 before 1); `row` breaks
// ties.  Records compare as (rank, key, row), smaller is better, and no two
// records of a table compare equal: the k best are one fixed list whatever
// computes them, which is what makes the result independent of the batch
// size, the slot count and the number of GPUs.
//
// Stage 1 (topn_vector_kernel) sorts every 1024-row vector's eligible rows
// and leaves its best min(k, eligible) records; stage 2 (topn_merge_kernel, one
// launch per level of a pairwise tree) merges the vectors of each row group
// into the row group's best k, and those lists -- 16 + 16 k bytes per row group -- are the
// batch's only D2H.  The host merges the row groups' lists (fls_scan_topn.hip).  A row
// is eligible when the mask selects it (or, without a mask, always) and it
// lies below the batch's row count; the value at a NULL key is a placeholder
// and is never loaded.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "fls_agg.hpp"

namespace fls {

constexpr uint32_t kMaxTopN = 1024;  // one vector's worth: a vector's candidate list never truncates

struct TopnRec {              // 16 B
    uint64_t key;             // order key, inverted for DESC; 0 at a NULL key
    uint32_t row;             // row within the batch (below 2^30)
    uint32_t rank;            // 0 / 1: the NULL placement
};
static_assert(sizeof(TopnRec) == 16, "TopnRec is 16 B");

// A list in HBM / pinned memory: this header, then up to k records, sorted.
struct TopnHdr {              // 16 B
    uint32_t count;           // records that follow (<= k)
    uint32_t pad[3];
};
static_assert(sizeof(TopnHdr) == 16, "TopnHdr is 16 B");
__host__ __device__ inline size_t topn_stride(uint32_t k) { return sizeof(TopnHdr) + (size_t)k * sizeof(TopnRec); }

// (rank, key, row): smaller is better
__host__ __device__ inline bool topn_less(const TopnRec &a, const TopnRec &b) {
    if (a.rank != b.rank) return a.rank < b.rank;
    if (a.key != b.key) return a.key < b.key;
    return a.row < b.row;
}

// The order key of a decoded value (kind: FK_INT / FK_UINT / FK_FLOAT, raw:
// the value sign- / zero-extended, or the binary64 bits of a float widened).
__host__ __device__ inline uint64_t topn_key(uint64_t raw, uint8_t kind, bool desc) {
    const uint64_t k = kind == FK_FLOAT ? agg_key_float(as_double(raw)) : kind == FK_INT ? agg_key_int((int64_t)raw) : raw;
    return desc ? ~k : k;
}

// The key column of a batch as the kernels see it (passed by value).
struct DevTopn {
    const uint8_t *col;       // decoded key column of the batch in HBM (row 0 of the batch)
    const uint64_t *valid;    // its validity words for the batch rows (HBM), or NULL: no NULL in the batch
    const uint64_t *mask;     // filter_kernel's selection words (16 per vector), or NULL: every row below nrows
    uint32_t nrows;           // rows of the batch
    uint32_t k;               // 1..kMaxTopN
    uint8_t ob, kind;         // bytes per decoded value; FK_INT / FK_UINT / FK_FLOAT
    uint8_t desc, nulls_first;
};

// Stage 1: one list per vector at d_vec + v * topn_stride(k).
hipError_t launch_topn_vectors(const DevTopn &p, uint8_t *d_vec, hipStream_t stream);
// Stage 2: d_rgvec holds per row group of the batch its first vector and its
// vector count (at most rg_vecs); ceil(log2(rg_vecs)) launches (at least one)
// merge each row group's lists pairwise between d_vec and d_tmp (as large as
// d_vec; both are overwritten), the last into one list per row group at
// d_rg + r * topn_stride(k).
hipError_t launch_topn_rowgroups(const uint32_t *d_rgvec, uint32_t nrg, uint32_t rg_vecs, uint32_t nvec, uint32_t k,
                                 uint8_t *d_vec, uint8_t *d_tmp, uint8_t *d_rg, hipStream_t stream);

}  // namespace fls
