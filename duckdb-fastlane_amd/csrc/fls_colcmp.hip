// fls_colcmp.hip -- gfx950 kernel of the column-to-column filter terms
// (`column op column` of the same row, OP_COL_EQ .. OP_COL_GE, fls_filter.hpp).
//
// colcmp_kernel runs right after filter_kernel on the same mask and narrows
// it, with keyset_kernel's mapping: a 256-thread block owns one 1024-row
// vector, wave w its 64-row words 4w..4w+3, lane = row within the word, so a
// mask or validity word is one wave-uniform load and a word's result one
// ballot.  The wave index comes through readfirstlane, so the term
// descriptors and the mask words sit in SGPRs.  Bandwidth work, no MFMA: per
// term and word two coalesced loads (lane i at base + i * width) and one
// compare.  A word the cheaper terms already emptied is skipped before any
// load, only live rows valid on both sides load, and the four words' left and
// right values of a term are issued back to back before the first compare.
// Every word is ANDed with row < nrows first, so no row at or past nrows is
// read whatever the mask holds.  No atomics on data, nothing shared between
// the blocks of a launch, no scratch; the only loop is bounded by the term
// count.
#include <hip/hip_runtime.h>

#include "fls_filter.hpp"

namespace fls {
namespace {

// the value at p, sign- or zero-extended to 64 bits (keyset_kernel's load_key)
__device__ __forceinline__ uint64_t load_value(const uint8_t *p, uint32_t ob, bool sign) {
    switch (ob) {
    case 1: return sign ? (uint64_t)(int64_t) * (const int8_t *)p : (uint64_t)*p;
    case 2: return sign ? (uint64_t)(int64_t) * (const int16_t *)p : (uint64_t) * (const uint16_t *)p;
    case 4: return sign ? (uint64_t)(int64_t) * (const int32_t *)p : (uint64_t) * (const uint32_t *)p;
    default: return *(const uint64_t *)p;
    }
}

// binary32 bits (low 32) widened exactly to binary64 bits
__device__ __forceinline__ uint64_t widen_f32(uint64_t bits) {
    const double d = (double)__uint_as_float((uint32_t)bits);
    uint64_t out;
    __builtin_memcpy(&out, &d, 8);
    return out;
}

__device__ __forceinline__ bool width_ok(uint32_t ob) { return ob == 1 || ob == 2 || ob == 4 || ob == 8; }

__global__ __launch_bounds__(256) void colcmp_kernel(const DevColTerm *__restrict__ terms, uint32_t nterms,
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
        if ((m[0] | m[1] | m[2] | m[3]) == 0) break;  // nothing left for the wave to compare
        const DevColTerm t = terms[i];
        // a descriptor no sound term produces selects nothing and is reported
        const bool flt = t.kind == FK_FLOAT;
        if (!width_ok(t.oba) || !width_ok(t.obb) || t.kind > FK_FLOAT || t.op > OP_GE ||
            (!flt && (t.f32a || t.f32b)) || (flt && (t.oba != (t.f32a ? 4 : 8) || t.obb != (t.f32b ? 4 : 8)))) {
            bad = true;
            m[0] = m[1] = m[2] = m[3] = 0;
            break;
        }
        const bool sign = t.kind == FK_INT;
        uint64_t live[4], a[4], b[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t word = 4 * w + k;
            live[k] = m[k];
            if (t.va && live[k]) live[k] &= t.va[(size_t)v * 16 + word];
            if (t.vb && live[k]) live[k] &= t.vb[(size_t)v * 16 + word];
            a[k] = b[k] = 0;
            if ((live[k] >> lane) & 1) {
                const uint64_t row = (uint64_t)v * 1024 + 64 * word + lane;
                a[k] = load_value(t.a + row * t.oba, t.oba, sign);
                b[k] = load_value(t.b + row * t.obb, t.obb, sign);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (m[k] == 0) continue;
            bool hit = false;
            if ((live[k] >> lane) & 1) {
                int c;
                if (flt)
                    c = cmp_float(as_double(t.f32a ? widen_f32(a[k]) : a[k]), as_double(t.f32b ? widen_f32(b[k]) : b[k]));
                else
                    c = sign ? cmp_int((int64_t)a[k], (int64_t)b[k]) : cmp_uint(a[k], b[k]);
                hit = op_holds(t.op, c);
            }
            m[k] = __ballot(hit);  // a NULL on either side satisfies no operator
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
    if (bad && lane == 0) atomicOr(err, KERR_COLCMP);
}

}  // namespace

hipError_t launch_colcmp(const DevColTerm *d_terms, uint32_t nterms, uint32_t nrows, uint64_t *d_mask,
                         uint32_t *d_counts, uint32_t *d_err, hipStream_t stream) {
    const uint32_t nvec = (nrows + 1023) / 1024;
    if (nvec == 0 || nterms == 0) return hipSuccess;
    hipLaunchKernelGGL(colcmp_kernel, dim3(nvec), dim3(256), 0, stream, d_terms, nterms, nrows, d_mask, d_counts,
                       d_err);
    return hipGetLastError();
}

}  // namespace fls
