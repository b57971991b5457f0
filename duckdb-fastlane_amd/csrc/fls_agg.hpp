// fls_agg.hpp -- ungrouped aggregates over a decoded scan batch in HBM
// (fls_aggregate): COUNT, SUM, MIN, MAX and SUM of products, under the
// pushed-down filter's selection mask and the columns' validity bitmaps.
//
// One launch per batch evaluates every requested aggregate and writes one
// fixed-size partial record per (1024-row vector, aggregate); the host folds
// the records in row order (flsgpu.hip).  A row contributes when it is
// selected (mask bit, or row < nrows without a mask) and its operand column(s)
// are valid there: values at NULL rows are placeholders and are never loaded.
// The reduction order inside a vector is fixed (lane: its four rows in order;
// wave: xor butterfly 32..1; block: waves 0..3 in order), so a vector's record
// depends on that vector's rows alone -- binary64 sums included.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fls_filter.hpp"

namespace fls {

enum AggFn : uint8_t {  // fls_agg_fn (flsgpu.h)
    AGG_COUNT_STAR = 0, AGG_COUNT = 1, AGG_SUM = 2, AGG_MIN = 3, AGG_MAX = 4, AGG_SUM_PRODUCT = 5
};
constexpr uint32_t kMaxAggs = 32;

// One aggregate of a batch as the kernel sees it.
struct DevAgg {               // 48 B
    const uint8_t *col;       // decoded operand column of the batch in HBM (row 0 of the batch);
                              // unused by the counts
    const uint8_t *col2;      // SUM_PRODUCT: the second operand
    const uint64_t *valid;    // operand validity words for the batch rows (HBM), or NULL: no NULL in the batch
    const uint64_t *valid2;   // ... of the second operand
    uint8_t fn;               // AggFn
    uint8_t ob, ob2;          // bytes per decoded value
    uint8_t kind, kind2;      // FilterKind of the operands: FK_INT / FK_UINT / FK_FLOAT
    uint8_t fslot;            // grouped call: which of the FLOAT / DOUBLE sums this is (fls_groupagg.hpp)
    uint8_t pad[10];
};
static_assert(sizeof(DevAgg) == 48, "DevAgg is 48 B");

// Partial result of one aggregate over one vector.
//   counts:            count only
//   integer SUM /
//   SUM_PRODUCT:       lo, hi = the 128-bit two's-complement sum
//   FLOAT/DOUBLE SUM:  lo = binary64 bits of the sum (-0.0 when count == 0)
//   MIN / MAX:         lo = order key of the extreme value (agg_key_*), meaningless when count == 0
struct AggRec {               // 32 B
    uint64_t count;           // rows that contributed
    uint64_t lo, hi;
    uint64_t pad;
};
static_assert(sizeof(AggRec) == 32, "AggRec is 32 B");

// Order keys: unsigned comparison of the keys is the column's order.  Floats
// follow cmp_float (fls_filter.hpp): every NaN is one key above +inf, -0 and
// +0 share one key.
__host__ __device__ inline uint64_t agg_key_int(int64_t v) { return (uint64_t)v ^ (1ull << 63); }
__host__ __device__ inline int64_t agg_unkey_int(uint64_t k) { return (int64_t)(k ^ (1ull << 63)); }
__host__ __device__ inline uint64_t agg_key_float(double d) {
    if (d != d) return ~0ull;
    if (d == 0) d = 0.0;
    uint64_t b;
    __builtin_memcpy(&b, &d, 8);
    return (b >> 63) ? ~b : b ^ (1ull << 63);
}
__host__ __device__ inline double agg_unkey_float(uint64_t k) {
    if (k == ~0ull) return __builtin_nan("");
    const uint64_t b = (k >> 63) ? k ^ (1ull << 63) : ~k;
    return as_double(b);
}

// naggs <= kMaxAggs records per vector, vector-major: d_out[v * naggs + a].
// d_mask: filter_kernel's selection words (16 per vector), or nullptr = every
// row below nrows.
hipError_t launch_aggregate(const DevAgg *d_aggs, uint32_t naggs, uint32_t nrows, const uint64_t *d_mask,
                            AggRec *d_out, hipStream_t stream);

}  // namespace fls
