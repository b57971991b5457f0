// fls_strmatch.hip -- gfx950 kernel of the string pattern filter terms
// (`column LIKE pattern` / `column NOT LIKE pattern`, fls_strmatch.hpp).
//
// strmatch_kernel runs after filter_kernel and keyset_kernel on the same mask
// and narrows it, in their geometry: a 256-thread block owns one 1024-row
// vector, wave w its 64-row words 4w..4w+3, lane = row within the word, so a
// mask or validity word is one wave-uniform load and a word's result one
// ballot.  The wave index comes through readfirstlane, so the descriptors and
// the mask words sit in SGPRs.
//
// Byte-comparing integer work (no MFMA), latency-bound on the per-lane string
// reads, so the kernel is built to read as few strings as it can:
//   * a block whose 16 words the cheaper terms emptied leaves before anything
//     is staged, a word they emptied is skipped before any load, and only
//     live, valid lanes read their 16-byte record;
//   * the tokens of all the launch's terms are staged once into LDS (at most
//     8 x 512 B, sized per launch from the real counts): the matcher's
//     per-lane token reads are LDS reads, not HBM gathers;
//   * a row is decided from its record alone, in this order: a length below
//     the pattern's minimum; for a pattern with no wildcard a length above the
//     token count; the literal prefix's first bytes against the record's
//     inline prefix; a string of at most 12 bytes matched from the record;
//   * only what survives resolves its pointer (batch heap or uploaded image,
//     range-checked, never dereferenced outside both) and runs the matcher
//     over [ptr, ptr + len).
// The matcher (like_match) keeps two cursors and one remembered `%`: no
// per-lane array, so no scratch.  No atomics on data, nothing shared between
// the blocks of a launch.
#include <hip/hip_runtime.h>

#include "fls_filter.hpp"
#include "fls_strmatch.hpp"

namespace fls {
namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool in_range(const StrRange &r, uint64_t hp, uint32_t len) {
    return hp >= r.host_lo && hp <= r.host_hi && len <= r.host_hi - hp;
}

// the string_t record rec (at p) against term t, its tokens in LDS at tok
__device__ __forceinline__ bool match_record(const DevPatTerm &t, const uint16_t *tok, const v4u rec, const uint8_t *p,
                                             bool &oob) {
    const uint32_t len = rec.x;
    if (len < t.min_len) return false;
    if (t.exact && len > t.ntok) return false;
    // the 4 bytes after the length are the string's first bytes in both the
    // inlined and the pointer form (len >= min_len >= prefix_len: they exist)
    if (t.prefix_len) {
        const uint32_t pm = t.prefix_len >= 4 ? ~0u : (1u << (8 * t.prefix_len)) - 1;
        if ((rec.y ^ t.prefix) & pm) return false;
    }
    const uint8_t *s;
    if (len <= 12) {
        s = p + 4;
    } else {
        const uint64_t hp = ((uint64_t)rec.w << 32) | rec.z;
        if (in_range(t.heap, hp, len)) {
            s = (const uint8_t *)(hp + t.heap.dev_delta);
        } else if (in_range(t.image, hp, len)) {
            s = (const uint8_t *)(hp + t.image.dev_delta);
        } else {
            oob = true;
            return false;
        }
    }
    return like_match(s, len, tok, t.ntok);
}

__global__ __launch_bounds__(256) void strmatch_kernel(const DevPatTerm *__restrict__ terms, uint32_t nterms,
                                                       uint32_t total_tokens, uint32_t nrows,
                                                       uint64_t *__restrict__ mask, uint32_t *__restrict__ counts,
                                                       uint32_t *__restrict__ err) {
    extern __shared__ uint16_t s_tok[];  // total_tokens tokens: the terms' patterns back to back
    __shared__ uint32_t wave_cnt[4];
    __shared__ uint32_t s_bad;
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
    if (threadIdx.x == 0) s_bad = 0;
    bool bad = false, oob = false;
    // block-uniform: a vector the cheaper terms emptied stages nothing
    if (__syncthreads_or((m[0] | m[1] | m[2] | m[3]) != 0)) {
        // stage the tokens; a descriptor no sound pattern produces selects nothing and is reported
        bool bad_desc = nterms > kMaxPatTerms, bad_tok = false;
        uint32_t off = 0;
        for (uint32_t i = 0; i < nterms && !bad_desc; ++i) {
            const uint32_t n = terms[i].ntok;
            if (n > kMaxPatTokens || n > total_tokens - off || terms[i].prefix_len > 4) {
                bad_desc = true;
                break;
            }
            const uint16_t *g = terms[i].tok;
            for (uint32_t j = threadIdx.x; j < n; j += 256) {
                const uint16_t x = g[j];
                bad_tok |= x > kTokAnyN;
                s_tok[off + j] = x;
            }
            off += n;
        }
        if (bad_desc || bad_tok) s_bad = 1;
        __syncthreads();
        bad = s_bad != 0;
        if (bad) m[0] = m[1] = m[2] = m[3] = 0;
        off = 0;
        for (uint32_t i = 0; i < nterms; ++i) {
            if ((m[0] | m[1] | m[2] | m[3]) == 0) break;  // nothing left for the wave to match
            const DevPatTerm t = terms[i];
            const uint16_t *tok = s_tok + off;
            off += t.ntok;
            uint64_t live[4];
            v4u rec[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t word = 4 * w + k;
                live[k] = m[k];
                if (t.valid && m[k]) live[k] &= t.valid[(size_t)v * 16 + word];
                rec[k] = v4u{0, 0, 0, 0};
                if ((live[k] >> lane) & 1) {
                    const uint64_t row = (uint64_t)v * 1024 + 64 * word + lane;
                    rec[k] = *(const v4u *)(t.col + row * 16);
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                if (m[k] == 0) continue;
                bool hit = false, out = false;
                if ((live[k] >> lane) & 1) {
                    const uint64_t row = (uint64_t)v * 1024 + 64 * (4 * w + k) + lane;
                    hit = match_record(t, tok, rec[k], t.col + row * 16, out);
                }
                const uint64_t h = __ballot(hit), o = __ballot(out);
                oob |= o != 0;
                // a NULL row satisfies neither; a string outside both ranges selects nothing
                m[k] = t.negate ? (live[k] & ~h & ~o) : h;
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
    if (lane == 0 && (bad || oob)) atomicOr(err, (bad ? KERR_PATTERN : 0u) | (oob ? KERR_FILTER_STR : 0u));
}

}  // namespace

hipError_t launch_strmatch(const DevPatTerm *d_terms, uint32_t nterms, uint32_t total_tokens, uint32_t nrows,
                           uint64_t *d_mask, uint32_t *d_counts, uint32_t *d_err, hipStream_t stream) {
    const uint32_t nvec = (nrows + 1023) / 1024;
    if (nvec == 0 || nterms == 0) return hipSuccess;
    if (nterms > kMaxPatTerms || total_tokens > kMaxPatTerms * kMaxPatTokens) return hipErrorInvalidValue;
    hipLaunchKernelGGL(strmatch_kernel, dim3(nvec), dim3(256), total_tokens * sizeof(uint16_t), stream, d_terms, nterms,
                       total_tokens, nrows, d_mask, d_counts, d_err);
    return hipGetLastError();
}

}  // namespace fls
