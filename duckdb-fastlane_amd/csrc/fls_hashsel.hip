// fls_hashsel.hip -- gfx950 kernels that choose among a hash aggregate's groups
// (fls_hashsel.hpp).  They run once the scan's streams have drained, on the
// pipeline's stream, and only read the table's fields; the one word they
// write in it is header word kHashHdrSelected.
//
// group_select_kernel walks the slots as hash_extract_kernel does -- a wave
// takes 64 consecutive slots, the survivors of a wave take their places with
// one atomicAdd of the ballot's popcount -- and leaves slot indices or
// candidate records.  group_topk_kernel and group_topk_merge_kernel have
// fls_topn.hip's two-stage shape: a 256-thread block sorts 1024 candidates in
// LDS (the compared fields in four arrays, 28 KB, and a 4 KB index array that
// the bitonic network permutes: a 32-byte record never moves in LDS) and keeps
// its best min(k, count); a pairwise tree, one launch per level, then merges
// the lists by rank, every record finding its place in the other list by
// binary search over global memory -- two 1024-record lists of 32-byte records
// would take 64 KB of LDS, and what HAVING leaves is small beside the scan.
// The lists carry no header: how many records list j of a level holds follows
// from the number of candidates alone (topk_list_count).  group_gather_kernel
// copies the chosen slots' fields into the dense field-major array the host
// unpacks.  No kernel waits on another thread; every loop is bounded by the
// capacity, the candidate count or k.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fls_hashsel.hpp"

namespace fls {
namespace {

typedef unsigned long long u64a;  // what HIP's 64-bit atomics take

__global__ __launch_bounds__(256) void group_select_kernel(DevGroupSelect p, u64a *table, uint64_t cap,
                                                           uint32_t *__restrict__ slots, GroupRec *__restrict__ recs,
                                                           uint64_t nmax) {
    const uint32_t lane = threadIdx.x & 63;
    const u64a *fields = table + kHashHdrWords;
    for (uint64_t s0 = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); s0 < cap; s0 += (uint64_t)gridDim.x * 256) {
        const uint64_t s = s0 + lane;
        auto get = [&](uint32_t f) { return (uint64_t)fields[(uint64_t)f * cap + s]; };
        bool ok = s < cap && get(kHashFieldKeys) != 0;
        if (ok) ok = having_all(p, get);
        const uint64_t bm = __ballot(ok);
        if (bm == 0) continue;  // (wave-uniform)
        uint64_t at = 0;
        if (lane == 0) at = atomicAdd(table + kHashHdrSelected, (u64a)__popcll(bm));  // one add per wave
        at = (uint64_t)__shfl((unsigned long long)at, 0, 64) + (uint64_t)__popcll(bm & ((1ull << lane) - 1));
        if (!ok || at >= nmax) continue;
        if (p.want_recs) {
            GroupRec r;
            order_key(p, get, r);
            r.first = ~get(kHashFieldFirst);
            r.slot = (uint32_t)s;
            recs[at] = r;
        } else {
            slots[at] = (uint32_t)s;
        }
    }
}

// Block b: candidates [1024 b, 1024 b + n) sorted, the best min(k, n) into list b.
__global__ __launch_bounds__(256) void group_topk_kernel(const GroupRec *__restrict__ recs, uint64_t total, uint32_t k,
                                                         GroupRec *__restrict__ out) {
    __shared__ uint64_t shi[1024], slo[1024], sfirst[1024];
    __shared__ uint32_t srank[1024], sidx[1024];
    const uint64_t base = (uint64_t)blockIdx.x * 1024;
    if (base >= total) return;  // (the whole block)
    const uint32_t n = (uint32_t)(total - base < 1024 ? total - base : 1024);
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t i = threadIdx.x + 256 * q;
        GroupRec r{0, 0, i, 0, 2};  // past the candidates: worse than any record
        if (i < n) r = recs[base + i];
        shi[i] = r.khi;
        slo[i] = r.klo;
        sfirst[i] = r.first;
        srank[i] = r.rank;
        sidx[i] = i;
    }
    __syncthreads();
    // bitonic network over the 1024 indices, two compare-exchanges per thread and step
    for (uint32_t size = 2; size <= 1024; size <<= 1) {
        for (uint32_t j = size >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (uint32_t q = 0; q < 2; ++q) {
                const uint32_t pr = threadIdx.x + 256 * q;
                const uint32_t i = ((pr & ~(j - 1)) << 1) | (pr & (j - 1)), o = i | j;
                const bool up = (i & size) == 0;
                const uint32_t a = sidx[i], b = sidx[o];
                if (rec_less(srank[b], shi[b], slo[b], sfirst[b], srank[a], shi[a], slo[a], sfirst[a]) == up) {
                    sidx[i] = b;
                    sidx[o] = a;
                }
            }
            __syncthreads();
        }
    }
    const uint32_t keep = n < k ? n : k;
    GroupRec *list = out + (uint64_t)blockIdx.x * k;
    for (uint32_t i = threadIdx.x; i < keep; i += 256) list[i] = recs[base + sidx[i]];  // (a kept index is below n)
}

// records of a[0..n) that are better than x
__device__ __forceinline__ uint32_t count_less(const GroupRec *__restrict__ a, uint32_t n, const GroupRec &x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const GroupRec m = a[mid];
        if (rec_less(m, x)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Block j: lists 2j and 2j + 1 of `level` (src) merge into list j of the next (dst).
__global__ __launch_bounds__(256) void group_topk_merge_kernel(const GroupRec *__restrict__ src, uint64_t total,
                                                               uint32_t k, uint32_t level, GroupRec *__restrict__ dst) {
    const uint64_t j = blockIdx.x;
    const uint32_t na = topk_list_count(total, k, level, 2 * j), nb = topk_list_count(total, k, level, 2 * j + 1);
    const GroupRec *a = src + 2 * j * k, *b = a + k;  // (b is not read where nb is 0)
    GroupRec *o = dst + j * k;
    for (uint32_t i = threadIdx.x; i < na; i += 256) {
        const GroupRec x = a[i];
        const uint32_t pos = i + count_less(b, nb, x);
        if (pos < k) o[pos] = x;
    }
    for (uint32_t i = threadIdx.x; i < nb; i += 256) {
        const GroupRec x = b[i];
        const uint32_t pos = i + count_less(a, na, x);
        if (pos < k) o[pos] = x;
    }
}

__global__ __launch_bounds__(256) void group_gather_kernel(const uint64_t *__restrict__ table, uint64_t cap,
                                                           uint32_t nfields, const uint32_t *__restrict__ slots,
                                                           const GroupRec *__restrict__ recs, uint64_t nout,
                                                           uint64_t *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nout; i += (uint64_t)gridDim.x * 256) {
        const uint64_t s = slots ? slots[i] : recs[i].slot;
        if (s >= cap) continue;  // (never: a slot index comes from the walk over cap)
        for (uint32_t f = 0; f < nfields; ++f) out[(uint64_t)f * nout + i] = table[kHashHdrWords + (uint64_t)f * cap + s];
    }
}

}  // namespace

hipError_t launch_group_select(const DevGroupSelect &p, uint64_t *d_table, uint64_t cap, uint32_t *d_slots,
                               GroupRec *d_recs, uint64_t nmax, hipStream_t stream) {
    if (cap == 0 || nmax == 0) return hipSuccess;
    if (p.nhaving > kMaxHaving || (p.want_recs ? !d_recs : !d_slots) || cap > (1ull << 32)) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((cap + 255) / 256, 8192);
    hipLaunchKernelGGL(group_select_kernel, dim3(grid), dim3(256), 0, stream, p, (u64a *)d_table, cap, d_slots, d_recs,
                       nmax);
    return hipGetLastError();
}

hipError_t launch_group_topk(const GroupRec *d_recs, uint64_t total, uint32_t k, GroupRec *d_a, GroupRec *d_b,
                             GroupRec *d_out, hipStream_t stream) {
    if (total == 0) return hipSuccess;
    const uint64_t lists = (total + 1023) / 1024;
    if (k == 0 || k > kMaxGroupLimit || !d_recs || !d_out || lists > 0x7FFFFFFFull || (lists > 1 && (!d_a || !d_b)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_topk_kernel, dim3((uint32_t)lists), dim3(256), 0, stream, d_recs, total, k,
                       lists == 1 ? d_out : d_a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    GroupRec *src = d_a, *dst = d_b;
    uint32_t level = 0;
    for (uint64_t n = lists; n > 1; n = (n + 1) / 2, ++level) {
        const uint64_t merges = (n + 1) / 2;
        hipLaunchKernelGGL(group_topk_merge_kernel, dim3((uint32_t)merges), dim3(256), 0, stream, (const GroupRec *)src,
                           total, k, level, merges == 1 ? d_out : dst);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        std::swap(src, dst);
    }
    return hipSuccess;
}

hipError_t launch_group_gather(const uint64_t *d_table, uint64_t cap, uint32_t nfields, const uint32_t *d_slots,
                               const GroupRec *d_recs, uint64_t nout, uint64_t *d_out, hipStream_t stream) {
    if (nout == 0) return hipSuccess;
    if ((!d_slots && !d_recs) || !d_out || cap == 0) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((nout + 255) / 256, 8192);
    hipLaunchKernelGGL(group_gather_kernel, dim3(grid), dim3(256), 0, stream, d_table, cap, nfields, d_slots, d_recs,
                       nout, d_out);
    return hipGetLastError();
}

}  // namespace fls
