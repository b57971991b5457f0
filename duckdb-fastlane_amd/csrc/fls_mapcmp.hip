// fls_mapcmp.hip -- gfx950 kernel of the map filter terms (`column op
// map[key column]` of the same row, OP_MAP_EQ .. OP_MAP_GE, fls_filter.hpp;
// the map's image: fls_valuemap.hpp).
//
// mapcmp_kernel runs after filter_kernel, colcmp_kernel and keyset_kernel on
// the same mask and narrows it, with their mapping: a 256-thread block owns
// one 1024-row vector, wave w its 64-row words 4w..4w+3, lane = row within the
// word, so a mask or validity word is one wave-uniform load and a word's
// result one ballot.  The wave index comes through readfirstlane, so the term
// descriptors and the mask words sit in SGPRs.  Bandwidth-plus-gather work, no
// MFMA: per term and word two coalesced loads (lane i at base + i * width),
// the probe's random gather and one compare.  A word the cheaper kernels
// already emptied is skipped before any load, only live rows valid on both
// sides load, and the four words' keys and left values of a term are issued
// back to back before the first probe.  A dense probe is a range test, then
// the presence word and the 8-byte value loaded together; a hash probe a loop
// of at most max_probe 8-byte gathers and one 8-byte gather from the value
// array at the matched slot.  Every word is ANDed with row < nrows first, so
// no row at or past nrows is read whatever the mask holds.  No atomics on
// data, nothing shared between the blocks of a launch, no scratch; the loops
// are bounded by the term count and by max_probe.
#include <hip/hip_runtime.h>

#include "fls_filter.hpp"
#include "fls_valuemap.hpp"

namespace fls {
namespace {

__global__ __launch_bounds__(256) void mapcmp_kernel(const DevMapCmpTerm *__restrict__ terms, uint32_t nterms,
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
        const DevMapCmpTerm t = terms[i];
        // a descriptor no sound map produces selects nothing and is reported
        // (a dense image holds span + 1 <= 2^28 values, a hash image at most 2^29 slots)
        if ((t.form != VM_DENSE && t.form != VM_HASH) || !valuemap_width_ok(t.oba) || !valuemap_width_ok(t.obk) || t.op > OP_GE ||
            (t.form == VM_DENSE && t.span >= kValuemapMaxSpan) ||
            (t.form == VM_HASH && (t.cap_log2 > 29 || t.max_probe > (1ull << t.cap_log2)))) {
            bad = true;
            m[0] = m[1] = m[2] = m[3] = 0;
            break;
        }
        uint64_t live[4], a[4], key[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t word = 4 * w + k;
            live[k] = m[k];
            if (t.va && live[k]) live[k] &= t.va[(size_t)v * 16 + word];
            if (t.vk && live[k]) live[k] &= t.vk[(size_t)v * 16 + word];
            a[k] = key[k] = 0;
            if ((live[k] >> lane) & 1) {  // a NULL row's placeholder is never loaded
                const uint64_t row = (uint64_t)v * 1024 + 64 * word + lane;
                key[k] = valuemap_load(t.key + row * t.obk, t.obk, t.ksign != 0);
                a[k] = valuemap_load(t.a + row * t.oba, t.oba, t.vsign != 0);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (m[k] == 0) continue;
            bool hit = false;
            if ((live[k] >> lane) & 1) {
                uint64_t b = 0;
                if (valuemap_probe(t, key[k], b)) {  // (fls_valuemap.hpp)
                    const int c = t.vsign ? cmp_int((int64_t)a[k], (int64_t)b) : cmp_uint(a[k], b);
                    hit = op_holds(t.op, c);
                }
            }
            m[k] = __ballot(hit);  // a NULL on either side or an absent key satisfies no operator
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
    if (bad && lane == 0) atomicOr(err, KERR_MAPCMP);
}

}  // namespace

hipError_t launch_mapcmp(const DevMapCmpTerm *d_terms, uint32_t nterms, uint32_t nrows, uint64_t *d_mask,
                         uint32_t *d_counts, uint32_t *d_err, hipStream_t stream) {
    const uint32_t nvec = (nrows + 1023) / 1024;
    if (nvec == 0 || nterms == 0) return hipSuccess;
    hipLaunchKernelGGL(mapcmp_kernel, dim3(nvec), dim3(256), 0, stream, d_terms, nterms, nrows, d_mask, d_counts,
                       d_err);
    return hipGetLastError();
}

}  // namespace fls
