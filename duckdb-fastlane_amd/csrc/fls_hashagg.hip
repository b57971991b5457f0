// fls_hashagg.hip -- gfx950 kernels of the hash aggregate (fls_hashagg.hpp).
//
// hash_insert_kernel keeps aggregate_kernel's mapping: a 256-thread block owns
// one 1024-row vector, wave w the 64-row words 4w..4w+3, lane = row within the
// word, every word ANDed with "row < nrows" so nothing past the batch is
// loaded.  Per selected row: pack the key, probe linearly from its hash slot
// with one 64-bit compare-and-swap per examined empty slot (a slot is accepted
// when it was empty or holds the key already, so no thread ever waits for
// another), then add the row to the slot's fields with relaxed device-scope
// atomics.  The addresses are data dependent; what shares a destination inside
// a wave is summed on chip first where `combine` is set: lanes that follow a
// lane with the same packed key form a run, the run's first lane probes for
// it, a segmented wave reduction folds the run's values and that lane issues
// one set of atomics for the run (a sorted key such as l_orderkey).
//
// Integer sums are 128-bit: the low word's returning add gives the carry,
// which goes into the high word's add, so each carry is counted exactly once
// and the pair is exact mod 2^128 in any arrival order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fls_hashagg.hpp"

namespace fls {
namespace {

typedef unsigned long long u64a;  // what HIP's 64-bit atomics take

__device__ __forceinline__ uint64_t shfl_idx64(uint64_t x, uint32_t src) {
    return (uint64_t)__shfl((unsigned long long)x, (int)src, 64);
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t x, uint32_t d) {
    return (uint64_t)__shfl_up((unsigned long long)x, d, 64);
}
__device__ __forceinline__ uint64_t shfl_down64(uint64_t x, uint32_t d) {
    return (uint64_t)__shfl_down((unsigned long long)x, d, 64);
}

__device__ __forceinline__ double load_float(const uint8_t *p, uint32_t ob) {
    return ob == 4 ? (double)*(const float *)p : *(const double *)p;
}

constexpr uint64_t kNoSlot = ~0ull;

__global__ __launch_bounds__(256) void hash_insert_kernel(const DevHashKey *__restrict__ keys, uint32_t nkeys,
                                                          const DevAgg *__restrict__ aggs,
                                                          const DevHashFields *__restrict__ fields, uint32_t naggs,
                                                          uint32_t nrows, const uint64_t *__restrict__ mask,
                                                          uint64_t first_row, u64a *table, uint64_t cap,
                                                          uint32_t max_groups, uint32_t combine, uint32_t *err) {
    const uint32_t v = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    u64a *tkeys = table + kHashHdrWords + (uint64_t)kHashFieldKeys * cap;
    u64a *tfirst = table + kHashHdrWords + (uint64_t)kHashFieldFirst * cap;
#pragma unroll 1
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t word = 4 * w + k;
        const uint64_t base = (uint64_t)v * 1024 + 64 * word;
        // rows of this word below nrows: no row past the batch is ever selected
        uint64_t m = base >= nrows ? 0ull : (nrows - base >= 64 ? ~0ull : (1ull << (nrows - base)) - 1);
        if (mask) m &= mask[(size_t)v * 16 + word];
        if (m == 0) continue;  // (wave-uniform)
        const uint64_t row = base + lane;
        // 1. the packed key; 0 for a row that is not selected
        uint64_t pk = 0;
        bool bad = false;
        if ((m >> lane) & 1) {
            pk = 1ull << 63;
            for (uint32_t q = 0; q < nkeys; ++q) {
                const DevHashKey &dk = keys[q];
                if (dk.valid && !((dk.valid[(size_t)v * 16 + word] >> lane) & 1)) {
                    pk |= 1ull << dk.null_bit;  // the placeholder is never loaded
                    continue;
                }
                uint64_t xl, xh;
                load_wide(dk.col + row * dk.ob, dk.ob, dk.sign != 0, xl, xh);
                const uint64_t f = xl - dk.min;
                if (f > dk.span) bad = true;
                else pk |= f << dk.shift;
            }
        }
        // a value outside its zone maps' range (a corrupt or foreign file): the row is dropped
        const uint64_t badm = __ballot(bad);
        if (badm) {
            if (lane == 0) atomicOr(err, KERR_HASH_RANGE);
            m &= ~badm;
            if (bad) pk = 0;
            if (m == 0) continue;
        }
        const bool sel = (m >> lane) & 1;
        // 2. runs of equal keys in adjacent lanes: lead = the lane that probes and
        // issues the atomics of lanes first..last (itself alone without combining)
        bool lead = sel, merged = false;
        uint32_t first = lane, last = lane;
        if (combine) {
            const uint64_t prev = shfl_up64(pk, 1);
            const bool head = sel && (lane == 0 || prev != pk);
            const uint64_t hm = __ballot(head);
            if (__popcll(hm) != __popcll(m)) {  // (wave-uniform) some run is longer than one lane
                merged = true;
                lead = head;
                if (sel) {  // (a selected lane has its run's head at or below it)
                    first = 63 - (uint32_t)__clzll((long long)(hm & (~0ull >> (63 - lane))));
                    const uint64_t breaks = (hm | ~m) & (lane == 63 ? 0ull : ~0ull << (lane + 1));
                    last = breaks ? (uint32_t)__ffsll((long long)breaks) - 2 : 63;
                }
            }
        }
        // 3. the slot: linear probing, bounded by the capacity
        uint64_t slot = kNoSlot;
        if (lead) {
            uint64_t s = hash_slot(pk, cap);
            for (uint64_t i = 0; i < cap; ++i) {
                // (a key never changes once stored: a non-zero value read here is final)
                u64a old = __hip_atomic_load(tkeys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (old == 0) old = atomicCAS(tkeys + s, 0ull, (u64a)pk);
                if (old == 0) {  // claimed: a new group, if the call allows one more
                    if (atomicAdd(table, 1ull) < max_groups) slot = s;
                    break;
                }
                if (old == pk) {
                    slot = s;
                    break;
                }
                s = (s + 1) & (cap - 1);
            }
            if (slot == kNoSlot) atomicOr(err, KERR_HASH_LIMIT);  // the row (its run) is dropped
        }
        slot = shfl_idx64(slot, first);
        const bool act = lead && slot != kNoSlot;
        const uint64_t run = (~0ull >> (63 - last)) & (~0ull << first);  // the lanes this lane speaks for
        if (act) atomicMax(tfirst + slot, (u64a)~(first_row + row));
        // 4. the aggregates
#pragma unroll 1
        for (uint32_t a = 0; a < naggs; ++a) {
            const DevAgg &g = aggs[a];
            const DevHashFields fl = fields[a];
            const uint32_t fn = g.fn;
            uint64_t c = m;  // the word's contributing rows
            if (g.cond) c &= g.cond[(size_t)v * 16 + word];
            if (fn == AGG_SUM_EXPR) {
                for (uint32_t i = 0; i < g.nf; ++i)
                    if (g.f[i].valid) c &= g.f[i].valid[(size_t)v * 16 + word];
            } else if (fn != AGG_COUNT_STAR) {
                if (g.valid) c &= g.valid[(size_t)v * 16 + word];
                if (fn == AGG_SUM_PRODUCT && g.valid2) c &= g.valid2[(size_t)v * 16 + word];
            }
            const uint64_t cnt = (uint64_t)__popcll(c & run);
            const bool add = act && cnt != 0;
            if (add) atomicAdd(table + kHashHdrWords + (uint64_t)fl.count * cap + slot, (u64a)cnt);
            if (fn <= AGG_COUNT) continue;
            // this lane's operand: 0, every field's identity, where the row does not contribute
            const bool on = (c >> lane) & 1;
            const bool is_sum = fn == AGG_SUM || fn == AGG_SUM_PRODUCT || fn == AGG_SUM_EXPR;
            uint64_t lo = 0, hi = 0;
            if (fn == AGG_SUM_EXPR) {
                const uint64_t mm[4] = {c, 0, 0, 0};
                uint64_t xl[4], xh[4];
                expr_values(g, row, mm, lane, xl, xh);
                lo = xl[0];
                hi = xh[0];
            } else if (on) {
                const uint8_t *p = g.col + row * g.ob;
                if (fn == AGG_SUM) {
                    load_wide(p, g.ob, g.kind == FK_INT, lo, hi);
                } else if (fn == AGG_SUM_PRODUCT) {
                    uint64_t yl, yh;
                    load_wide(p, g.ob, g.kind == FK_INT, lo, hi);
                    load_wide(g.col2 + row * g.ob2, g.ob2, g.kind2 == FK_INT, yl, yh);
                    mul128(lo, hi, yl, yh);
                } else {  // MIN / MAX: the maximum of the order key, or of its complement
                    uint64_t key;
                    if (g.kind == FK_FLOAT) {
                        key = agg_key_float(load_float(p, g.ob));
                    } else {
                        uint64_t xl, xh;
                        load_wide(p, g.ob, g.kind == FK_INT, xl, xh);
                        key = g.kind == FK_INT ? agg_key_int((int64_t)xl) : xl;
                    }
                    lo = fn == AGG_MIN ? ~key : key;
                }
            }
            if (merged) {  // (wave-uniform) fold each run into its first lane
#pragma unroll
                for (uint32_t d = 1; d < 64; d <<= 1) {
                    const uint64_t ol = shfl_down64(lo, d);
                    const uint64_t oh = is_sum ? shfl_down64(hi, d) : 0;
                    if (lane + d <= last) {  // (the lane d above belongs to this lane's run)
                        if (is_sum) add128(lo, hi, ol, oh);
                        else lo = ol > lo ? ol : lo;
                    }
                }
            }
            if (add) {
                u64a *tlo = table + kHashHdrWords + (uint64_t)fl.lo * cap + slot;
                if (is_sum) {
                    const uint64_t old = atomicAdd(tlo, (u64a)lo);
                    const uint64_t h = hi + ((uint64_t)(old + lo) < old ? 1 : 0);
                    if (h) atomicAdd(table + kHashHdrWords + (uint64_t)fl.hi * cap + slot, (u64a)h);
                } else {
                    atomicMax(tlo, (u64a)lo);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void hash_extract_kernel(u64a *table, uint64_t cap, uint32_t nfields,
                                                           uint64_t *__restrict__ out, uint64_t nout) {
    const uint32_t lane = threadIdx.x & 63;
    const u64a *tkeys = table + kHashHdrWords + (uint64_t)kHashFieldKeys * cap;
    // a wave takes 64 consecutive slots at a time
    for (uint64_t s0 = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); s0 < cap; s0 += (uint64_t)gridDim.x * 256) {
        const uint64_t s = s0 + lane;
        const bool occ = s < cap && tkeys[s] != 0;
        const uint64_t bm = __ballot(occ);
        if (bm == 0) continue;
        uint64_t at = 0;
        if (lane == 0) at = atomicAdd(table + 1, (u64a)__popcll(bm));  // one add per wave
        at = shfl_idx64(at, 0) + (uint64_t)__popcll(bm & ((1ull << lane) - 1));
        if (!occ || at >= nout) continue;
        for (uint32_t f = 0; f < nfields; ++f) out[(uint64_t)f * nout + at] = table[kHashHdrWords + (uint64_t)f * cap + s];
    }
}

}  // namespace

hipError_t launch_hash_insert(const DevHashKey *d_keys, uint32_t nkeys, const DevAgg *d_aggs,
                              const DevHashFields *d_fields, uint32_t naggs, uint32_t nrows, const uint64_t *d_mask,
                              uint64_t first_row, uint64_t *d_table, uint64_t cap, uint32_t max_groups, bool combine,
                              uint32_t *d_err, hipStream_t stream) {
    const uint32_t nvec = (nrows + 1023) / 1024;
    if (nvec == 0) return hipSuccess;
    if (nkeys == 0 || nkeys > kMaxKeys || naggs == 0 || naggs > kMaxAggs || cap < 2 || (cap & (cap - 1)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(hash_insert_kernel, dim3(nvec), dim3(256), 0, stream, d_keys, nkeys, d_aggs, d_fields, naggs,
                       nrows, d_mask, first_row, (u64a *)d_table, cap, max_groups, combine ? 1u : 0u, d_err);
    return hipGetLastError();
}

hipError_t launch_hash_extract(uint64_t *d_table, uint64_t cap, uint32_t nfields, uint64_t *d_out, uint64_t nout,
                               hipStream_t stream) {
    if (cap == 0 || nout == 0) return hipSuccess;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((cap + 255) / 256, 8192);
    hipLaunchKernelGGL(hash_extract_kernel, dim3(grid), dim3(256), 0, stream, (u64a *)d_table, cap, nfields, d_out,
                       nout);
    return hipGetLastError();
}

}  // namespace fls
