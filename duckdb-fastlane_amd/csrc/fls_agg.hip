// fls_agg.hip -- gfx950 kernel of the aggregate scan (fls_agg.hpp).
//
// HBM-bound integer / binary64 work (no MFMA): ob bytes per contributing row
// per operand column, one mask word and one validity word per 64 rows.  A
// 256-thread block owns one 1024-row vector with filter_kernel's mapping: wave
// w handles the 64-row words 4w..4w+3, lane = row within the word, so a mask
// or validity word is one broadcast load and a count is a popcount of it.
// Each wave reduces with xor shuffles, the four waves meet in LDS and thread a
// writes aggregate a's record: no atomics, nothing shared between blocks.
#include <hip/hip_runtime.h>

#include "fls_agg.hpp"

namespace fls {
namespace {

__device__ __forceinline__ uint64_t shfl64(uint64_t x, int d) {
    return (uint64_t)__shfl_xor((unsigned long long)x, d, 64);
}

__device__ __forceinline__ double load_float(const uint8_t *p, uint32_t ob) {
    return ob == 4 ? (double)*(const float *)p : *(const double *)p;
}

__global__ __launch_bounds__(256) void aggregate_kernel(const DevAgg *__restrict__ aggs, uint32_t naggs,
                                                        uint32_t nrows, const uint64_t *__restrict__ mask,
                                                        AggRec *__restrict__ out) {
    __shared__ uint64_t part[kMaxAggs][4][3];  // per aggregate and wave: count, lo, hi
    const uint32_t v = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t a = 0; a < naggs; ++a) {
        const DevAgg &g = aggs[a];
        const uint32_t fn = g.fn;
        const bool flt = g.kind == FK_FLOAT;
        const bool is_min = fn == AGG_MIN;
        uint64_t cnt = 0;
        // accumulators: integer sums (lo, hi); float sums lo = binary64 bits
        // (identity -0.0: x + -0.0 == x for every x); MIN / MAX lo = order key
        uint64_t lo = 0, hi = 0;
        double fsum = -0.0;
        if (fn == AGG_MIN) lo = ~0ull;
        if (fn == AGG_SUM_EXPR) {
            // a loop of its own: as one more case of the loop below it cost the other functions
            // the schedule that keeps their four rows' loads in flight
            uint64_t m[4], xl[4], xh[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t word = 4 * w + k;
                const uint64_t base = (uint64_t)v * 1024 + 64 * word;
                m[k] = base >= nrows ? 0ull : (nrows - base >= 64 ? ~0ull : (1ull << (nrows - base)) - 1);
                if (mask) m[k] &= mask[(size_t)v * 16 + word];
                if (g.cond) m[k] &= g.cond[(size_t)v * 16 + word];
                for (uint32_t i = 0; i < g.nf; ++i)
                    if (g.f[i].valid) m[k] &= g.f[i].valid[(size_t)v * 16 + word];
                cnt += (uint64_t)__popcll(m[k]);
            }
            expr_values(g, (uint64_t)v * 1024 + 256 * w + lane, m, lane, xl, xh);
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) add128(lo, hi, xl[k], xh[k]);  // (0 for a row that does not contribute)
        } else {
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t word = 4 * w + k;
                const uint64_t base = (uint64_t)v * 1024 + 64 * word;
                // rows of this word below nrows: no row past the batch is ever selected
                uint64_t m = base >= nrows ? 0ull : (nrows - base >= 64 ? ~0ull : (1ull << (nrows - base)) - 1);
                if (mask) m &= mask[(size_t)v * 16 + word];
                if (g.cond) m &= g.cond[(size_t)v * 16 + word];
                if (fn != AGG_COUNT_STAR) {
                    if (g.valid) m &= g.valid[(size_t)v * 16 + word];
                    if (fn == AGG_SUM_PRODUCT && g.valid2) m &= g.valid2[(size_t)v * 16 + word];
                }
                cnt += (uint64_t)__popcll(m);
                if (fn <= AGG_COUNT || !((m >> lane) & 1)) continue;
                const uint64_t row = base + lane;
                const uint8_t *p = g.col + row * g.ob;
                if (fn == AGG_SUM) {
                    if (flt) {
                        fsum += load_float(p, g.ob);
                    } else {
                        uint64_t xl, xh;
                        load_wide(p, g.ob, g.kind == FK_INT, xl, xh);
                        add128(lo, hi, xl, xh);
                    }
                } else if (fn == AGG_SUM_PRODUCT) {
                    // the product of the sign- / zero-extended operands mod 2^128
                    uint64_t xl, xh, yl, yh;
                    load_wide(p, g.ob, g.kind == FK_INT, xl, xh);
                    load_wide(g.col2 + row * g.ob2, g.ob2, g.kind2 == FK_INT, yl, yh);
                    mul128(xl, xh, yl, yh);
                    add128(lo, hi, xl, xh);
                } else {  // MIN / MAX over order keys
                    uint64_t key;
                    if (flt) {
                        key = agg_key_float(load_float(p, g.ob));
                    } else {
                        uint64_t xl, xh;
                        load_wide(p, g.ob, g.kind == FK_INT, xl, xh);
                        key = g.kind == FK_INT ? agg_key_int((int64_t)xl) : xl;
                    }
                    lo = is_min ? (key < lo ? key : lo) : (key > lo ? key : lo);
                }
            }
        }
        // across the wave (cnt is the same in every lane already)
        if (fn == AGG_SUM && flt) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) fsum += __shfl_xor(fsum, d, 64);
            __builtin_memcpy(&lo, &fsum, 8);
        } else if (fn == AGG_SUM || fn == AGG_SUM_PRODUCT || fn == AGG_SUM_EXPR) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const uint64_t ol = shfl64(lo, d), oh = shfl64(hi, d);
                add128(lo, hi, ol, oh);
            }
        } else if (fn == AGG_MIN || fn == AGG_MAX) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const uint64_t o = shfl64(lo, d);
                lo = is_min ? (o < lo ? o : lo) : (o > lo ? o : lo);
            }
        }
        if (lane == 0) {
            part[a][w][0] = cnt;
            part[a][w][1] = lo;
            part[a][w][2] = hi;
        }
    }
    __syncthreads();
    if (threadIdx.x < naggs) {
        const uint32_t a = threadIdx.x;
        const DevAgg &g = aggs[a];
        AggRec r;
        r.count = part[a][0][0];
        r.lo = part[a][0][1];
        r.hi = part[a][0][2];
        r.pad = 0;
        for (uint32_t i = 1; i < 4; ++i) {  // waves in order
            const uint64_t c = part[a][i][0], l = part[a][i][1], h = part[a][i][2];
            r.count += c;
            if (g.fn == AGG_SUM && g.kind == FK_FLOAT) {
                const double s = as_double(r.lo) + as_double(l);
                __builtin_memcpy(&r.lo, &s, 8);
            } else if (g.fn == AGG_SUM || g.fn == AGG_SUM_PRODUCT || g.fn == AGG_SUM_EXPR) {
                add128(r.lo, r.hi, l, h);
            } else if (g.fn == AGG_MIN) {
                r.lo = l < r.lo ? l : r.lo;
            } else if (g.fn == AGG_MAX) {
                r.lo = l > r.lo ? l : r.lo;
            }
        }
        out[(size_t)v * naggs + a] = r;
    }
}

}  // namespace

hipError_t launch_aggregate(const DevAgg *d_aggs, uint32_t naggs, uint32_t nrows, const uint64_t *d_mask,
                            AggRec *d_out, hipStream_t stream) {
    const uint32_t nvec = (nrows + 1023) / 1024;
    if (nvec == 0 || naggs == 0) return hipSuccess;
    if (naggs > kMaxAggs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(aggregate_kernel, dim3(nvec), dim3(256), 0, stream, d_aggs, naggs, nrows, d_mask, d_out);
    return hipGetLastError();
}

}  // namespace fls
