// fls_keymap.hip -- gfx950 kernel of the mapped GROUP BY keys
// (fls_aggregate_key_bindings, fls_keymap.hpp).
//
// keymap_kernel runs after filter_kernel and keyset_kernel on the same mask,
// with their mapping: a 256-thread block owns one 1024-row vector, wave w its
// 64-row words 4w..4w+3, lane = row within the word; the wave index comes
// through readfirstlane, so the binding descriptors, the mask words and the
// validity words sit in SGPRs.  Per binding it probes the map with the
// column's value at every selected, valid row and writes the code as one
// uint16 per row into the binding's derived column (a word's 64 lanes store
// one 128-byte line), which stage 1 of the grouped aggregate then reads as a
// 2-byte key.  An inner binding narrows the mask word to the ballot of hits;
// a keep-unmatched binding writes that ballot as the derived key's validity
// word and leaves the mask alone.  Integer work, latency-bound on the probe's
// random gather (no MFMA): the four words' column values of a binding are
// loaded back to back before the first probe; a dense probe is a range test
// and one 2-byte gather, a hash probe a loop of at most max_probe 8-byte
// gathers and one 2-byte gather on a match.  No atomics on data, nothing
// shared between the blocks of a launch, no scratch.
#include <hip/hip_runtime.h>

#include "fls_groupagg.hpp"
#include "fls_keymap.hpp"

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

// the code of key, or kKeymapAbsent (keymap_lookup, fls_keymap.hpp)
__device__ __forceinline__ uint32_t probe(const DevMapTerm &t, uint64_t key) {
    if (t.form == KM_DENSE) {
        const uint64_t d = key - t.min;
        if (d > t.span) return kKeymapAbsent;
        return ((const uint16_t *)t.table)[d];
    }
    if (key == t.empty) return kKeymapAbsent;  // the sentinel is no key
    const uint64_t cap_mask = (1ull << t.cap_log2) - 1;
    const uint64_t h = t.cap_log2 ? (key * kKeysetHashMul) >> (64 - t.cap_log2) : 0;
    for (uint32_t p = 0; p < t.max_probe; ++p) {
        const uint64_t i = (h + p) & cap_mask;
        const uint64_t slot = t.table[i];
        if (slot == key) return ((const uint16_t *)(t.table + cap_mask + 1))[i];
        if (slot == t.empty) return kKeymapAbsent;
    }
    return kKeymapAbsent;
}

__global__ __launch_bounds__(256) void keymap_kernel(const DevMapTerm *__restrict__ terms, uint32_t nterms,
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
        // nothing left for the wave to probe: stage 1 reads a derived key's
        // code and validity at selected rows only
        if ((m[0] | m[1] | m[2] | m[3]) == 0) break;
        const DevMapTerm t = terms[i];
        // a descriptor no sound map produces selects nothing and is reported
        if ((t.form != KM_DENSE && t.form != KM_HASH) || t.cap_log2 > 63 ||
            (t.form == KM_HASH && t.max_probe > (1ull << t.cap_log2))) {
            bad = true;
            m[0] = m[1] = m[2] = m[3] = 0;
            break;
        }
        uint64_t live[4], val[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t word = 4 * w + k;
            live[k] = m[k];
            if (t.valid && m[k]) live[k] &= t.valid[(size_t)v * 16 + word];  // a NULL row's placeholder is never loaded
            val[k] = 0;
            if ((live[k] >> lane) & 1) {
                const uint64_t row = (uint64_t)v * 1024 + 64 * word + lane;
                val[k] = load_key(t.col + row * t.ob, t.ob, t.sign != 0);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t word = 4 * w + k;
            uint64_t h = 0;
            if (m[k]) {  // (wave-uniform) a word no row of which is selected is neither probed nor written
                uint32_t code = kKeymapAbsent;
                if ((live[k] >> lane) & 1) code = probe(t, val[k]);
                // every lane of the word stores, so every selected row's code
                // is written (stage 1 loads it only at the hits)
                t.code[(size_t)v * 1024 + 64 * word + lane] = (uint16_t)code;
                h = __ballot(code != kKeymapAbsent);
            }
            if (t.keep) {
                if (lane == 0) t.kvalid[(size_t)v * 16 + word] = h;  // the rest: the NULL group
            } else {
                m[k] = h;  // a NULL or unmatched row belongs to no group
            }
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
    if (bad && lane == 0) atomicOr(err, KERR_KEYMAP);
}

}  // namespace

hipError_t launch_keymap(const DevMapTerm *d_terms, uint32_t nterms, uint32_t nrows, uint64_t *d_mask,
                         uint32_t *d_counts, uint32_t *d_err, hipStream_t stream) {
    const uint32_t nvec = (nrows + 1023) / 1024;
    if (nvec == 0 || nterms == 0) return hipSuccess;
    hipLaunchKernelGGL(keymap_kernel, dim3(nvec), dim3(256), 0, stream, d_terms, nterms, nrows, d_mask, d_counts,
                       d_err);
    return hipGetLastError();
}

}  // namespace fls
