// fls_mapval.hip -- gfx950 kernel of the mapped columns (`map[key column]` of
// the same row as an aggregate operand or a hash GROUP BY key,
// fls_aggregate_value_bindings; the map's image: fls_valuemap.hpp).
//
// mapval_kernel runs where keymap_kernel runs -- after the filter's kernels
// and the alternatives on the same mask, before the conditions' planes and the
// reduce kernel -- with the siblings' mapping: a 256-thread block owns one
// 1024-row vector, wave w its 64-row words 4w..4w+3, lane = row within the
// word; the wave index comes through readfirstlane, so the binding
// descriptors, the mask words and the validity words sit in SGPRs.  Per
// binding the four words' keys are loaded back to back, at selected rows whose
// key is valid only (a NULL row's placeholder is never loaded), then probed
// with the probe mapcmp_kernel uses (valuemap_probe): dense a range test, then
// the presence word and the 8-byte value loaded together; hash at most
// max_probe 8-byte gathers and one 8-byte gather from the value array.  The
// value goes out as one uint64 per row into the binding's derived column (a
// word's 64 lanes store 512 contiguous bytes), the ballot of hits as the
// derived column's validity word.  An inner binding narrows the mask word to
// that ballot; a keep-unmatched binding leaves the mask alone.  counts[v] is
// recomputed at the end, as the siblings do.
//
// INVARIANT: a derived column and its validity are DEFINED AT SELECTED ROWS
// ONLY.  A word no row of which is selected (when its binding's turn comes) is
// neither probed nor written, and rows at or past nrows are never read.  The
// three reduce kernels (fls_agg.hip, fls_groupagg.hip, fls_hashagg.hip) AND
// the mask -- or a condition's plane, which is a subset of it -- into a word
// before an operand's or a key's validity word counts, and load a value only
// where the result has a bit; so what an unwritten word holds is never used.
//
// Integer work, latency-bound on the probe's random gather (no MFMA).  No
// atomics on data, nothing shared between the blocks of a launch, no scratch;
// the loops are bounded by the binding count and by max_probe.
#include <hip/hip_runtime.h>

#include "fls_filter.hpp"
#include "fls_valuemap.hpp"

namespace fls {
namespace {

__global__ __launch_bounds__(256) void mapval_kernel(const DevMapValTerm *__restrict__ terms, uint32_t nterms,
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
        // nothing left for the wave to probe: the reduce kernels read a derived
        // column's value and validity at selected rows only
        if ((m[0] | m[1] | m[2] | m[3]) == 0) break;
        const DevMapValTerm t = terms[i];
        // a descriptor no sound map produces selects nothing and is reported
        // (a dense image holds span + 1 <= 2^28 values, a hash image at most 2^29 slots)
        if ((t.form != VM_DENSE && t.form != VM_HASH) || !valuemap_width_ok(t.obk) ||
            (t.form == VM_DENSE && t.span >= kValuemapMaxSpan) ||
            (t.form == VM_HASH && (t.cap_log2 > 29 || t.max_probe > (1ull << t.cap_log2)))) {
            bad = true;
            m[0] = m[1] = m[2] = m[3] = 0;
            break;
        }
        uint64_t live[4], key[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t word = 4 * w + k;
            live[k] = m[k];
            if (t.vk && m[k]) live[k] &= t.vk[(size_t)v * 16 + word];  // a NULL row's placeholder is never loaded
            key[k] = 0;
            if ((live[k] >> lane) & 1) {
                const uint64_t row = (uint64_t)v * 1024 + 64 * word + lane;
                key[k] = valuemap_load(t.key + row * t.obk, t.obk, t.ksign != 0);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (m[k] == 0) continue;  // (wave-uniform) a word no row of which is selected is neither probed nor written
            const uint32_t word = 4 * w + k;
            uint64_t val = 0;
            bool hit = false;
            if ((live[k] >> lane) & 1) hit = valuemap_probe(t, key[k], val);  // (fls_valuemap.hpp)
            // every lane of the word stores, so every selected row's value is
            // written: 64 x 8 contiguous bytes (0 where the map has no value)
            t.out[(size_t)v * 1024 + 64 * word + lane] = hit ? val : 0ull;
            const uint64_t h = __ballot(hit);
            if (lane == 0) t.ovalid[(size_t)v * 16 + word] = h;
            if (!t.keep) m[k] = h;  // inner: a NULL or unmatched row leaves the selection
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
    if (bad && lane == 0) atomicOr(err, KERR_MAPVAL);
}

}  // namespace

hipError_t launch_mapval(const DevMapValTerm *d_terms, uint32_t nterms, uint32_t nrows, uint64_t *d_mask,
                         uint32_t *d_counts, uint32_t *d_err, hipStream_t stream) {
    const uint32_t nvec = (nrows + 1023) / 1024;
    if (nvec == 0 || nterms == 0) return hipSuccess;
    hipLaunchKernelGGL(mapval_kernel, dim3(nvec), dim3(256), 0, stream, d_terms, nterms, nrows, d_mask, d_counts,
                       d_err);
    return hipGetLastError();
}

}  // namespace fls
