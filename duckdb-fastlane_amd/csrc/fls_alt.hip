// fls_alt.hip -- gfx950 kernels of the filter's alternatives
// (fls_scan_filter_alternatives: AND-groups joined by OR, AND-ed to the filter).
//
// After the filter's kernels the slot's mask holds the rows the base filter
// selects.  An alternative is a filter of its own; the mask keeps a row when
// one of them is true there.  Two launches per batch, whatever the number of
// alternatives:
//   * alt_kernel, with filter_kernel's and cond_kernel's mapping: a 256-thread
//     block owns one 1024-row vector, wave w its words 4w..4w+3, lane = row
//     within the word.  A word's mask is read once for all alternatives; a zero
//     word loads no term.  Per alternative the ordinary terms are evaluated for
//     the lanes set in the word and one ballot is its word.  A closed
//     alternative (no key-set, column-pair or pattern term follows) is OR-ed
//     into the word written back as the mask; an open one's ballot goes to its
//     plane, which the filter's narrowing kernels (fls_colcmp.hip,
//     fls_keyset.hip, fls_strmatch.hip) then work on like on any mask.  The
//     vector's count goes to counts as filter_kernel writes it: with closed
//     alternatives only, this launch is the whole step.
//   * alt_merge_kernel, when an alternative was open: one mask word per
//     thread, mask |= the open planes' words (at most 8 loads), and the
//     vector's count from a 16-lane reduction inside the wave (16 words per
//     vector), so no LDS and no atomics.
// Planes start from the mask, which is never set at or past nrows, so neither
// are they nor the merged mask.  HBM- and launch-bound integer work (no MFMA):
// ob bytes per selected row per term column, 8 bytes written per 64 rows and
// open alternative.
#include <hip/hip_runtime.h>

#include "fls_filter.hpp"
#include "fls_filter_dev.hpp"

namespace fls {
namespace {

__global__ __launch_bounds__(256) void alt_kernel(const DevTerm *__restrict__ terms, const AltList alts, uint32_t nrows,
                                                  uint64_t *__restrict__ mask, uint64_t *__restrict__ planes,
                                                  uint32_t *__restrict__ counts, uint32_t *__restrict__ err) {
    __shared__ uint32_t wave_cnt[4];
    const uint32_t v = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t plane_words = (size_t)gridDim.x * 16;
    uint32_t cnt = 0;
    bool bad = false;
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t word = 4 * w + k;
        const uint64_t base = (uint64_t)v * 1024 + 64 * word;
        // rows of this word below nrows: no row past the batch is read whatever the mask holds
        uint64_t m = base >= nrows ? 0ull : (nrows - base >= 64 ? ~0ull : (1ull << (nrows - base)) - 1);
        m &= mask[(size_t)v * 16 + word];
        const uint64_t row = base + lane;
        const bool ok = (m >> lane) & 1;
        uint64_t sel = 0;  // the closed alternatives' rows of the word
        for (uint32_t a = 0; a < alts.n; ++a) {
            uint64_t b = 0;
            if (m != 0) {  // (wave-uniform)
                bool res = ok, acc = false;
                for (uint32_t i = alts.first[a]; i < alts.first[a + 1]; ++i) {
                    const DevTerm &t = terms[i];
                    acc = acc || (ok && eval_term(t, row, bad));
                    if (t.end_clause) {
                        res = res && acc;
                        acc = false;
                    }
                }
                b = __ballot(res);
            }
            if ((alts.closed >> a) & 1) sel |= b;
            else if (lane == 0) planes[a * plane_words + (size_t)v * 16 + word] = b;
        }
        if (lane == 0) mask[(size_t)v * 16 + word] = sel;
        cnt += (uint32_t)__popcll(sel);
    }
    if (lane == 0) wave_cnt[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[v] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    if (__ballot(bad) && lane == 0) atomicOr(err, KERR_FILTER_STR);
}

// open: bit a set for every alternative whose plane takes part; nwords = 16 per vector
__global__ __launch_bounds__(256) void alt_merge_kernel(uint32_t open, uint32_t nalts, size_t nwords,
                                                        uint64_t *__restrict__ mask,
                                                        const uint64_t *__restrict__ planes,
                                                        uint32_t *__restrict__ counts) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = g < nwords;  // (whole 16-lane groups: nwords is a multiple of 16)
    uint64_t x = 0;
    if (in) {
        x = mask[g];
        for (uint32_t a = 0; a < nalts; ++a)
            if ((open >> a) & 1) x |= planes[a * nwords + g];
        mask[g] = x;
    }
    uint32_t c = (uint32_t)__popcll(x);
    // the 16 words of a vector sit in 16 adjacent lanes
    c += __shfl_xor(c, 8);
    c += __shfl_xor(c, 4);
    c += __shfl_xor(c, 2);
    c += __shfl_xor(c, 1);
    if (in && (threadIdx.x & 15) == 0) counts[g >> 4] = c;
}

}  // namespace

hipError_t launch_alternatives(const DevTerm *d_terms, const AltList &alts, uint32_t nrows, uint64_t *d_mask,
                               uint64_t *d_planes, uint32_t *d_counts, uint32_t *d_err, hipStream_t stream) {
    const uint32_t nvec = (nrows + 1023) / 1024;
    if (nvec == 0 || alts.n == 0) return hipSuccess;
    if (alts.n > kMaxConds) return hipErrorInvalidValue;
    for (uint32_t a = 0; a < alts.n; ++a)
        if (alts.first[a] > alts.first[a + 1]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(alt_kernel, dim3(nvec), dim3(256), 0, stream, d_terms, alts, nrows, d_mask, d_planes, d_counts,
                       d_err);
    return hipGetLastError();
}

hipError_t launch_alt_merge(const AltList &alts, uint32_t nrows, uint64_t *d_mask, const uint64_t *d_planes,
                            uint32_t *d_counts, hipStream_t stream) {
    const uint32_t nvec = (nrows + 1023) / 1024;
    if (alts.n > kMaxConds) return hipErrorInvalidValue;
    const uint32_t open = ~alts.closed & ((1u << alts.n) - 1);
    if (nvec == 0 || open == 0) return hipSuccess;
    const size_t nwords = (size_t)nvec * 16;
    hipLaunchKernelGGL(alt_merge_kernel, dim3((uint32_t)((nwords + 255) / 256)), dim3(256), 0, stream, open, alts.n,
                       nwords, d_mask, d_planes, d_counts);
    return hipGetLastError();
}

}  // namespace fls
