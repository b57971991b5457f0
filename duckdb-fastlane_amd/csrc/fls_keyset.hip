// fls_keyset.hip -- gfx950 kernel of the key-set filter terms
// (`column IN set` / `column NOT IN set`, fls_keyset.hpp).
//
// keyset_kernel runs right after filter_kernel on the same mask and narrows
// it: filter_kernel's mapping (a 256-thread block owns one 1024-row vector,
// wave w its 64-row words 4w..4w+3, lane = row within the word), so a mask or
// validity word is one wave-uniform load and a word's result one ballot.
// Integer work, latency-bound on the probe's random gather (no MFMA): a word
// the cheaper terms already emptied is skipped before any column load, the
// four words' column values of a term are loaded back to back before the
// first probe, and a probe is one dword gather (bitmap) or a loop of at most
// max_probe 8-byte gathers (hash).  The wave index comes through
// readfirstlane, so the term descriptors and the mask words sit in SGPRs.
// No atomics on data, nothing shared between the blocks of a launch, no
// scratch.
#include <hip/hip_runtime.h>

#include "fls_filter.hpp"
#include "fls_keyset.hpp"

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

__device__ __forceinline__ bool probe(const DevSetTerm &t, uint64_t key) {
    if (t.form == KS_BITMAP) {
        const uint64_t d = key - t.min;
        if (d > t.span) return false;
        return (((const uint32_t *)t.table)[d >> 5] >> (d & 31)) & 1;
    }
    if (key == t.empty) return false;  // the sentinel is no key
    const uint64_t cap_mask = (1ull << t.cap_log2) - 1;
    const uint64_t h = t.cap_log2 ? (key * kKeysetHashMul) >> (64 - t.cap_log2) : 0;
    for (uint32_t p = 0; p < t.max_probe; ++p) {
        const uint64_t slot = t.table[(h + p) & cap_mask];
        if (slot == key) return true;
        if (slot == t.empty) return false;
    }
    return false;
}

__global__ __launch_bounds__(256) void keyset_kernel(const DevSetTerm *__restrict__ terms, uint32_t nterms,
                                                     uint32_t nrows, uint64_t *__restrict__ mask,
                                                     uint32_t *__restrict__ counts, uint32_t *__restrict__ err) {
    __shared__ uint32_t wave_cnt[4];
    const uint32_t v = blockIdx.x, lane = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint64_t m[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t word = 4 * w + k;
        const uint64_t base = (uint64_t)v * 1024 + 64 * word;
        // rows of this word below nrows: no row past the batch is loaded whatever the mask holds
        m[k] = base >= nrows ? 0ull : (nrows - base >= 64 ? ~0ull : (1ull << (nrows - base)) - 1);
        if (m[k]) m[k] &= mask[(size_t)v * 16 + word];
    }
    bool bad = false;
    for (uint32_t i = 0; i < nterms; ++i) {
        if ((m[0] | m[1] | m[2] | m[3]) == 0) break;  // nothing left for the wave to probe
        const DevSetTerm t = terms[i];
        // a descriptor no sound set produces selects nothing and is reported
        if ((t.form != KS_BITMAP && t.form != KS_HASH) || t.cap_log2 > 63 ||
            (t.form == KS_HASH && t.max_probe > (1ull << t.cap_log2))) {
            bad = true;
            m[0] = m[1] = m[2] = m[3] = 0;
            break;
        }
        uint64_t live[4], val[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t word = 4 * w + k;
            live[k] = m[k];
            if (t.valid && m[k]) live[k] &= t.valid[(size_t)v * 16 + word];
            val[k] = 0;
            if ((live[k] >> lane) & 1) {
                const uint64_t row = (uint64_t)v * 1024 + 64 * word + lane;
                val[k] = load_key(t.col + row * t.ob, t.ob, t.sign != 0);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (m[k] == 0) continue;
            bool hit = false;
            if ((live[k] >> lane) & 1) hit = probe(t, val[k]);
            const uint64_t h = __ballot(hit);
            m[k] = t.negate ? (live[k] & ~h) : h;  // a NULL row satisfies neither
        }
    }
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        if (lane == 0) mask[(size_t)v * 16 + 4 * w + k] = m[k];
        cnt += (uint32_t)__popcll(m[k]);
    }
    if (lane == 0) wave_cnt[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[v] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    if (bad && lane == 0) atomicOr(err, KERR_KEYSET);
}

}  // namespace

hipError_t launch_keyset(const DevSetTerm *d_terms, uint32_t nterms, uint32_t nrows, uint64_t *d_mask,
                         uint32_t *d_counts, uint32_t *d_err, hipStream_t stream) {
    const uint32_t nvec = (nrows + 1023) / 1024;
    if (nvec == 0 || nterms == 0) return hipSuccess;
    hipLaunchKernelGGL(keyset_kernel, dim3(nvec), dim3(256), 0, stream, d_terms, nterms, nrows, d_mask, d_counts,
                       d_err);
    return hipGetLastError();
}

}  // namespace fls
