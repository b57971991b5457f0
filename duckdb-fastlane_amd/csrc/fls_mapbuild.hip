// fls_mapbuild.hip -- gfx950 kernels of the map build from a scan
// (fls_valuemap_from_scan / fls_keymap_from_scan, fls_scan_mapbuild.hip).
//
// mapbuild_kernel (collect) consumes the selection mask after the filter's
// kernels with keyset_build_kernel's mapping: a 256-thread block owns one
// 1024-row vector, wave w its 64-row words 4w..4w+3, lane = row within the
// word; the wave index comes through readfirstlane, so the descriptor (a kernel
// argument), the mask words and both columns' validity words sit in SGPRs.
// Per word it loads key and value at every selected row where both are valid
// and does old = atomicMin(&slot[d], x), d = key - base, x the value in the
// value order (keyset_ord), on the call's collecting array in HBM, which every
// batch of the call on this GPU shares and which holds all ones (the
// "untouched" pattern) before the first batch.  The lane flags a conflict when
// old is neither all ones nor x.
//
// Why this is exact, whatever the order of lanes, blocks, batches and slots:
//   - Atomics on one address are totally ordered.
//   - A non-sentinel old is a value some row of that key wrote, so a flag is
//     always a true conflict: two rows of one key with different values.
//   - Every operation before the first one whose value differs from the first
//     operation's value wrote that same value, so the slot holds exactly it
//     when that operation arrives: neither all ones nor its own value.  Every
//     key with two values is therefore flagged at least once.
//   - The gate (fls_scan_mapbuild.hip) guarantees that no real value equals
//     the sentinel: a value column whose zone maps reach the all-ones pattern
//     in the value order never gets here, and narrower types cannot form it.
//   - Nothing is read back with a plain load for a decision; every lane issues
//     its atomic (map keys are unique or nearly so: there is nothing to skip).
// When no conflict is flagged every touched slot holds its key's one value.
//
// A lane with d > span touches nothing and raises KERR_MAPBUILD: slot[d] is
// only ever formed from d <= span < 2^28, so no atomic lands outside the
// span + 1 slots whatever the columns hold.  A conflict raises
// KERR_MAPBUILD_CONFLICT; the first flagged lane to claim the cell
// slot[span + 1] (one compare-and-swap from all ones to its d) also records
// the two values it saw, old and x, in slot[span + 2] and slot[span + 3] (the
// array has span + 4 entries), so the host can name one key with both values.
// No scratch, no LDS but the wave counts.
//
// mapbuild_presence_kernel and mapbuild_gather_kernel (compact) run once per
// GPU after the scan, one lane per slot in 1024-thread blocks: a wave's
// __ballot(slot[d] != ~0) is one word of the presence bitmap, a block's
// present slots are counted, and, with the host's exclusive scan of the block
// counts, each present slot's value goes (as the stored pattern again) to
// block offset + wave prefix + popcount(ballot below lane) of a compact array:
// the values arrive in key order.  Both read slots d < n only; the gather
// writes out[i] for i < nout only.
#include <hip/hip_runtime.h>

#include "fls_filter.hpp"

namespace fls {
namespace {

__device__ __forceinline__ uint64_t load_ext(const uint8_t *p, uint32_t ob, bool sign) {
    switch (ob) {
    case 1: return sign ? (uint64_t)(int64_t) * (const int8_t *)p : (uint64_t)*p;
    case 2: return sign ? (uint64_t)(int64_t) * (const int16_t *)p : (uint64_t) * (const uint16_t *)p;
    case 4: return sign ? (uint64_t)(int64_t) * (const int32_t *)p : (uint64_t) * (const uint32_t *)p;
    default: return *(const uint64_t *)p;
    }
}

__global__ __launch_bounds__(256) void mapbuild_kernel(const DevMapBuild p, uint32_t *__restrict__ counts,
                                                       uint32_t *__restrict__ err) {
    __shared__ uint32_t wave_cnt[4];
    const uint32_t v = blockIdx.x, lane = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t vflip = p.vsign ? 1ull << 63 : 0ull;  // keyset_ord of the value kind
    uint32_t cnt = 0;
    bool bad = false, clash = false;
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t word = 4 * w + k;
        const uint64_t first = (uint64_t)v * 1024 + 64 * word;
        // rows of this word below nrows: no row past the batch is loaded whatever the mask holds
        uint64_t m = first >= p.nrows ? 0ull : (p.nrows - first >= 64 ? ~0ull : (1ull << (p.nrows - first)) - 1);
        if (m) m &= p.mask[(size_t)v * 16 + word];
        if (m && p.vk) m &= p.vk[(size_t)v * 16 + word];  // a NULL row's placeholder is never loaded,
        if (m && p.vv) m &= p.vv[(size_t)v * 16 + word];  // of either column
        if (m == 0) continue;                             // (wave-uniform)
        bool live = (m >> lane) & 1;
        uint64_t d = 0, x = 0;
        if (live) {
            d = load_ext(p.key + (first + lane) * p.obk, p.obk, p.ksign != 0) - p.base;
            x = load_ext(p.value + (first + lane) * p.obv, p.obv, p.vsign != 0) ^ vflip;
        }
        if (live && d > p.span) {  // outside the collecting range: nothing is touched, and the call fails
            live = false;
            bad = true;
        }
        cnt += (uint32_t)__popcll(__ballot(live));
        if (live) {  // d <= span: inside the span + 1 slots
            const uint64_t old = atomicMin((unsigned long long *)&p.slot[d], (unsigned long long)x);
            if (old != ~0ull && old != x) {
                clash = true;
                uint64_t *cell = p.slot + p.span + 1;  // d <= span: no cell is ever a slot
                if (atomicCAS((unsigned long long *)cell, ~0ull, (unsigned long long)d) == ~0ull) {
                    cell[1] = old;  // (read by the host after the call's streams are synchronised)
                    cell[2] = x;
                }
            }
        }
    }
    if (lane == 0) wave_cnt[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[v] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    if (bad || clash) atomicOr(err, (bad ? KERR_MAPBUILD : 0u) | (clash ? KERR_MAPBUILD_CONFLICT : 0u));
}

constexpr uint32_t kCompactBlock = 1024;  // slots (and threads) of a block of the compaction

__global__ __launch_bounds__(kCompactBlock) void mapbuild_presence_kernel(const uint64_t *__restrict__ slot, uint64_t n,
                                                                         uint64_t *__restrict__ presence,
                                                                         uint32_t *__restrict__ block_counts) {
    __shared__ uint32_t wave_cnt[kCompactBlock / 64];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t d = (uint64_t)blockIdx.x * kCompactBlock + threadIdx.x;
    const bool present = d < n && slot[d] != ~0ull;
    const uint64_t b = __ballot(present);
    const uint64_t word = (uint64_t)blockIdx.x * (kCompactBlock / 64) + w;
    if (lane == 0) {
        if (word * 64 < n) presence[word] = b;  // (n + 63) / 64 words
        wave_cnt[w] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (uint32_t i = 0; i < kCompactBlock / 64; ++i) s += wave_cnt[i];
        block_counts[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kCompactBlock) void mapbuild_gather_kernel(const uint64_t *__restrict__ slot, uint64_t n,
                                                                       const uint64_t *__restrict__ block_offsets,
                                                                       uint64_t vflip, uint64_t *__restrict__ out,
                                                                       uint64_t nout) {
    __shared__ uint32_t wave_cnt[kCompactBlock / 64];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t d = (uint64_t)blockIdx.x * kCompactBlock + threadIdx.x;
    const uint64_t x = d < n ? slot[d] : ~0ull;
    const bool present = x != ~0ull;
    const uint64_t b = __ballot(present);
    if (lane == 0) wave_cnt[w] = (uint32_t)__popcll(b);
    __syncthreads();
    uint64_t at = block_offsets[blockIdx.x];
    for (uint32_t i = 0; i < w; ++i) at += wave_cnt[i];  // (wave-uniform)
    at += (uint64_t)__popcll(b & ((1ull << lane) - 1));
    if (present && at < nout) out[at] = x ^ vflip;  // the stored pattern
}

}  // namespace

hipError_t launch_mapbuild(const DevMapBuild &p, uint32_t *d_counts, uint32_t *d_err, hipStream_t stream) {
    const uint32_t nvec = (p.nrows + 1023) / 1024;
    if (nvec == 0) return hipSuccess;
    hipLaunchKernelGGL(mapbuild_kernel, dim3(nvec), dim3(256), 0, stream, p, d_counts, d_err);
    return hipGetLastError();
}

hipError_t launch_mapbuild_presence(const uint64_t *slot, uint64_t n, uint64_t *presence, uint32_t *block_counts,
                                    hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t nb = (uint32_t)((n + kCompactBlock - 1) / kCompactBlock);
    hipLaunchKernelGGL(mapbuild_presence_kernel, dim3(nb), dim3(kCompactBlock), 0, stream, slot, n, presence,
                       block_counts);
    return hipGetLastError();
}

hipError_t launch_mapbuild_gather(const uint64_t *slot, uint64_t n, const uint64_t *block_offsets, bool vsign,
                                  uint64_t *out, uint64_t nout, hipStream_t stream) {
    if (n == 0 || nout == 0) return hipSuccess;
    const uint32_t nb = (uint32_t)((n + kCompactBlock - 1) / kCompactBlock);
    hipLaunchKernelGGL(mapbuild_gather_kernel, dim3(nb), dim3(kCompactBlock), 0, stream, slot, n, block_offsets,
                       vsign ? 1ull << 63 : 0ull, out, nout);
    return hipGetLastError();
}

}  // namespace fls
