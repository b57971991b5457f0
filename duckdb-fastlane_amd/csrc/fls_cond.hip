// fls_cond.hip -- gfx950 kernel of the aggregates' conditions
// (agg(...) FILTER (WHERE cond), fls_aggregate_conditions).
//
// A condition is a filter of its own that selects no row: it yields one plane
// of 64-row words per batch, `where & cond`, which the reduce kernels AND
// into an aggregate's selection word exactly where they AND validity words.
// cond_kernel writes the planes of every condition of the call in one launch
// with filter_kernel's mapping: a 256-thread block owns one 1024-row vector,
// wave w its words 4w..4w+3, lane = row within the word.  Each word starts
// from the scan's mask word (without a scan mask: the row < nrows word), read
// once for all conditions; a zero word is written as zero with no term load,
// otherwise the condition's ordinary terms are evaluated for the lanes set in
// it and one ballot is the plane's word.  HBM-bound integer work (no MFMA):
// ob bytes per selected row per term column, 8 bytes written per 64 rows and
// condition.  Key-set, column-pair and LIKE terms narrow a plane afterwards
// through the filter's own kernels (fls_keyset.hip, fls_colcmp.hip,
// fls_strmatch.hip), which work on any mask buffer.
#include <hip/hip_runtime.h>

#include "fls_filter.hpp"
#include "fls_filter_dev.hpp"

namespace fls {
namespace {

__global__ __launch_bounds__(256) void cond_kernel(const DevTerm *__restrict__ terms, const CondList conds,
                                                   uint32_t nrows, const uint64_t *__restrict__ mask,
                                                   uint64_t *__restrict__ planes, uint32_t *__restrict__ err) {
    const uint32_t v = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t plane_words = (size_t)gridDim.x * 16;
    bool bad = false;
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t word = 4 * w + k;
        const uint64_t base = (uint64_t)v * 1024 + 64 * word;
        // rows of this word below nrows: a plane is never set past the batch
        uint64_t m = base >= nrows ? 0ull : (nrows - base >= 64 ? ~0ull : (1ull << (nrows - base)) - 1);
        if (mask) m &= mask[(size_t)v * 16 + word];
        const uint64_t row = base + lane;
        const bool ok = (m >> lane) & 1;
        for (uint32_t c = 0; c < conds.n; ++c) {
            uint64_t b = 0;
            if (m != 0) {  // (wave-uniform)
                bool res = ok, acc = false;
                for (uint32_t i = conds.first[c]; i < conds.first[c + 1]; ++i) {
                    const DevTerm &t = terms[i];
                    acc = acc || (ok && eval_term(t, row, bad));
                    if (t.end_clause) {
                        res = res && acc;
                        acc = false;
                    }
                }
                b = __ballot(res);
            }
            if (lane == 0) planes[c * plane_words + (size_t)v * 16 + word] = b;
        }
    }
    if (__ballot(bad) && lane == 0) atomicOr(err, KERR_FILTER_STR);
}

}  // namespace

hipError_t launch_conditions(const DevTerm *d_terms, const CondList &conds, uint32_t nrows, const uint64_t *d_mask,
                             uint64_t *d_planes, uint32_t *d_err, hipStream_t stream) {
    const uint32_t nvec = (nrows + 1023) / 1024;
    if (nvec == 0 || conds.n == 0) return hipSuccess;
    if (conds.n > kMaxConds) return hipErrorInvalidValue;
    for (uint32_t c = 0; c < conds.n; ++c)
        if (conds.first[c] > conds.first[c + 1]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cond_kernel, dim3(nvec), dim3(256), 0, stream, d_terms, conds, nrows, d_mask, d_planes, d_err);
    return hipGetLastError();
}

}  // namespace fls
