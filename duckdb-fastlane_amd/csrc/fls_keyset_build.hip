// fls_keyset_build.hip -- gfx950 kernel of the key-set build from a scan
// (fls_keyset_from_scan, fls_scan_keyset.hip).
//
// keyset_build_kernel consumes the selection mask after the filter's kernels
// (filter_kernel, colcmp_kernel, keyset_kernel, strmatch_kernel, the
// alternatives) with keymap_kernel's mapping: a 256-thread block owns one
// 1024-row vector, wave w its 64-row words 4w..4w+3, lane = row within the
// word; the wave index comes through readfirstlane, so the descriptor (a kernel
// argument), the mask words and the validity words sit in SGPRs.  Per word it
// loads the key column at every selected, valid row and sets bit
// d = key - base of the call's bitmap in HBM, which every batch of the call on
// this GPU shares: bits are only ever set while the call runs, so the order of
// the batches, slots and blocks changes nothing.
//
// The atomics (one integer OR per selected row at most):
//   window   When the dwords a word's live lanes name span fewer than 64
//            (a sorted or clustered column: l_orderkey puts 64 rows into one
//            or two dwords), the lanes OR their bits into the wave's 64-dword
//            LDS window and lane j then issues one global atomic for dword
//            lo + j where the window holds a bit: at most 64 contiguous
//            dwords per instruction instead of up to 64 atomics on one
//            address.
//   scatter  Otherwise one global atomic per live lane.
// Either way an atomic whose bits a plain load already shows as set is
// skipped: a stale zero costs one redundant atomic and nothing else.
//
// A lane with d > span sets no bit and raises KERR_KEYBUILD: dword d >> 5 is
// only ever formed from d <= span < 2^32, so no atomic lands outside the
// span / 32 + 1 dwords of the bitmap whatever the column holds.  The window's
// global atomics address dwords lo + j <= hi, both of which live lanes named.
// No scratch; LDS: the four windows and the wave counts.
#include <hip/hip_runtime.h>

#include "fls_filter.hpp"

namespace fls {
namespace {

__device__ __forceinline__ uint64_t load_key(const uint8_t *p, uint32_t ob, bool sign) {
    switch (ob) {
    case 1: return sign ? (uint64_t)(int64_t) * (const int8_t *)p : (uint64_t)*p;
    case 2: return sign ? (uint64_t)(int64_t) * (const int16_t *)p : (uint64_t) * (const uint16_t *)p;
    case 4: return sign ? (uint64_t)(int64_t) * (const int32_t *)p : (uint64_t) * (const uint32_t *)p;
    default: return *(const uint64_t *)p;
    }
}

// min / max of x over the wave's 64 lanes (all active)
__device__ __forceinline__ uint32_t wave_min(uint32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, o, 64));
    return x;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, o, 64));
    return x;
}

__global__ __launch_bounds__(256) void keyset_build_kernel(const DevKeyBuild p, uint32_t *__restrict__ counts,
                                                           uint32_t *__restrict__ err) {
    __shared__ uint32_t window[4][64];
    __shared__ uint32_t wave_cnt[4];
    const uint32_t v = blockIdx.x, lane = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t cnt = 0;
    bool bad = false;
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t word = 4 * w + k;
        const uint64_t first = (uint64_t)v * 1024 + 64 * word;
        // rows of this word below nrows: no row past the batch is loaded whatever the mask holds
        uint64_t m = first >= p.nrows ? 0ull : (p.nrows - first >= 64 ? ~0ull : (1ull << (p.nrows - first)) - 1);
        if (m) m &= p.mask[(size_t)v * 16 + word];
        if (m && p.valid) m &= p.valid[(size_t)v * 16 + word];  // a NULL row's placeholder is never loaded
        if (m == 0) continue;                                   // (wave-uniform)
        bool live = (m >> lane) & 1;
        uint64_t d = 0;
        if (live) d = load_key(p.col + (first + lane) * p.ob, p.ob, p.sign != 0) - p.base;
        if (live && d > p.span) {  // outside the collecting range: no bit, and the call fails
            live = false;
            bad = true;
        }
        const uint64_t lv = __ballot(live);
        cnt += (uint32_t)__popcll(lv);
        if (lv == 0) continue;
        const uint32_t dw = (uint32_t)(d >> 5), bit = 1u << (d & 31);  // d <= span < 2^32 where live
        if (p.window) {
            const uint32_t lo = wave_min(live ? dw : 0xFFFFFFFFu), hi = wave_max(live ? dw : 0u);
            if (hi - lo < 64) {  // (wave-uniform)
                uint32_t *win = window[w];
                win[lane] = 0;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (live) atomicOr(&win[dw - lo], bit);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const uint32_t x = win[lane];  // lane j: dword lo + j <= hi where x != 0
                if (x && (p.bitmap[lo + lane] & x) != x) atomicOr(&p.bitmap[lo + lane], x);
                continue;
            }
        }
        if (live && !(p.bitmap[dw] & bit)) atomicOr(&p.bitmap[dw], bit);
    }
    if (lane == 0) wave_cnt[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[v] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    if (bad) atomicOr(err, KERR_KEYBUILD);
}

}  // namespace

hipError_t launch_keyset_build(const DevKeyBuild &p, uint32_t *d_counts, uint32_t *d_err, hipStream_t stream) {
    const uint32_t nvec = (p.nrows + 1023) / 1024;
    if (nvec == 0) return hipSuccess;
    hipLaunchKernelGGL(keyset_build_kernel, dim3(nvec), dim3(256), 0, stream, p, d_counts, d_err);
    return hipGetLastError();
}

}  // namespace fls
