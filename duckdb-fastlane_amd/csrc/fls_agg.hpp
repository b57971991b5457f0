// fls_agg.hpp -- ungrouped aggregates over a decoded scan batch in HBM
// (fls_aggregate): COUNT, SUM, MIN, MAX, SUM of products and SUM of products
// of affine terms k + s * column, under the pushed-down filter's selection
// mask and the columns' validity bitmaps.
//
// One launch per batch evaluates every requested aggregate and writes one
// fixed-size partial record per (1024-row vector, aggregate); the host folds
// the records in row order (fls_scan_agg.hip).  A row contributes when it is
// selected (mask bit, or row < nrows without a mask), its aggregate's condition
// (if any: DevAgg::cond) holds there and its operand column(s) are valid
// there: values at NULL rows are placeholders and are never loaded.
// The reduction order inside a vector is fixed (lane: its four rows in order;
// wave: xor butterfly 32..1; block: waves 0..3 in order), so a vector's record
// depends on that vector's rows alone -- binary64 sums included.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "fls_filter.hpp"

namespace fls {

enum AggFn : uint8_t {  // fls_agg_fn (flsgpu.h)
    AGG_COUNT_STAR = 0, AGG_COUNT = 1, AGG_SUM = 2, AGG_MIN = 3, AGG_MAX = 4, AGG_SUM_PRODUCT = 5,
    AGG_SUM_EXPR = 6
};
constexpr uint32_t kMaxAggs = 32;
constexpr uint32_t kMaxFactors = 3;   // factors of a SUM_EXPR product

// One factor k + sign * column of a SUM_EXPR, evaluated mod 2^128.
struct DevFactor {            // 24 B
    const uint8_t *col;       // decoded column of the batch in HBM (row 0 of the batch)
    const uint64_t *valid;    // its validity words for the batch rows (HBM), or NULL: no NULL in the batch
    int64_t k;                // the constant, in the column's physical unit
};

// One aggregate of a batch as the kernel sees it.
struct DevAgg {               // 128 B
    const uint8_t *col;       // decoded operand column of the batch in HBM (row 0 of the batch);
                              // unused by the counts
    const uint8_t *col2;      // SUM_PRODUCT: the second operand
    const uint64_t *valid;    // operand validity words for the batch rows (HBM), or NULL: no NULL in the batch
    const uint64_t *valid2;   // ... of the second operand
    uint8_t fn;               // AggFn
    uint8_t ob, ob2;          // bytes per decoded value
    uint8_t kind, kind2;      // FilterKind of the operands: FK_INT / FK_UINT / FK_FLOAT
    uint8_t fslot;            // grouped call: which of the FLOAT / DOUBLE sums this is (fls_groupagg.hpp)
    // SUM_EXPR: the product of f[0..nf); col / col2 / valid / valid2 / ob / kind are unused
    uint8_t nf;               // 1..kMaxFactors
    uint8_t fob[kMaxFactors];   // bytes per decoded value of each factor's column
    uint8_t fkind[kMaxFactors]; // FK_INT / FK_UINT
    uint8_t fneg[kMaxFactors];  // 1: sign = -1
    DevFactor f[kMaxFactors];
    // the aggregate's condition (agg FILTER (WHERE cond), fls_cond.hip): its plane of
    // `where & cond` words for the batch rows (HBM, 16 per vector), or NULL: no condition
    const uint64_t *cond;
};
static_assert(sizeof(DevFactor) == 24, "DevFactor is 24 B");
static_assert(sizeof(DevAgg) == 128 && offsetof(DevAgg, f) == 48 && offsetof(DevAgg, cond) == 120,
              "DevAgg is 48 B + 3 factors + the condition's plane");

// Partial result of one aggregate over one vector.
//   counts:            count only
//   integer SUM /
//   SUM_PRODUCT /
//   SUM_EXPR:          lo, hi = the 128-bit two's-complement sum
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

// The integer arithmetic the two aggregate kernels share (fls_agg.hip,
// fls_groupagg.hip): 128-bit two's-complement values as (lo, hi).
#ifdef __HIPCC__
// the operand at p as a 128-bit two's-complement integer (lo, hi)
__device__ __forceinline__ void load_wide(const uint8_t *p, uint32_t ob, bool sign, uint64_t &lo, uint64_t &hi) {
    if (sign) {
        int64_t v;
        switch (ob) {
        case 1: v = *(const int8_t *)p; break;
        case 2: v = *(const int16_t *)p; break;
        case 4: v = *(const int32_t *)p; break;
        default: v = *(const int64_t *)p; break;
        }
        lo = (uint64_t)v;
        hi = v < 0 ? ~0ull : 0ull;
    } else {
        switch (ob) {
        case 1: lo = *p; break;
        case 2: lo = *(const uint16_t *)p; break;
        case 4: lo = *(const uint32_t *)p; break;
        default: lo = *(const uint64_t *)p; break;
        }
        hi = 0;
    }
}

__device__ __forceinline__ void add128(uint64_t &lo, uint64_t &hi, uint64_t blo, uint64_t bhi) {
    lo += blo;
    hi += bhi + (lo < blo ? 1 : 0);
}

// (lo, hi) *= (blo, bhi) mod 2^128
__device__ __forceinline__ void mul128(uint64_t &lo, uint64_t &hi, uint64_t blo, uint64_t bhi) {
    const uint64_t pl = lo * blo;
    hi = __umul64hi(lo, blo) + lo * bhi + hi * blo;
    lo = pl;
}

// SUM_EXPR's operands of a lane's four rows row0 + 64 * k (k = 0..3: the
// wave's four words), where bit `lane` of m[k] is set: the product of the
// factors k + sign * column mod 2^128; (0, 0) for the other rows.  The factors
// go one after the other (not unrolled: the descriptor fields are wave-uniform
// and one factor's registers are reused by the next), each with its four rows'
// loads in flight together.
__device__ __forceinline__ void expr_values(const DevAgg &g, uint64_t row0, const uint64_t m[4], uint32_t lane,
                                            uint64_t lo[4], uint64_t hi[4]) {
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        lo[k] = (m[k] >> lane) & 1;
        hi[k] = 0;
    }
#pragma unroll 1
    for (uint32_t i = 0; i < g.nf; ++i) {
        const uint8_t *col = g.f[i].col;
        const uint32_t ob = g.fob[i];
        const bool sign = g.fkind[i] == FK_INT, neg = g.fneg[i] != 0;
        const int64_t c = g.f[i].k;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (!((m[k] >> lane) & 1)) continue;
            uint64_t xl, xh;
            load_wide(col + (row0 + 64 * k) * ob, ob, sign, xl, xh);
            if (neg) {  // two's-complement negation
                xl = 0 - xl;
                xh = ~xh + (xl == 0 ? 1 : 0);
            }
            add128(xl, xh, (uint64_t)c, c < 0 ? ~0ull : 0ull);
            mul128(lo[k], hi[k], xl, xh);
        }
    }
}
#endif

// naggs <= kMaxAggs records per vector, vector-major: d_out[v * naggs + a].
// d_mask: filter_kernel's selection words (16 per vector), or nullptr = every
// row below nrows.
hipError_t launch_aggregate(const DevAgg *d_aggs, uint32_t naggs, uint32_t nrows, const uint64_t *d_mask,
                            AggRec *d_out, hipStream_t stream);

}  // namespace fls
