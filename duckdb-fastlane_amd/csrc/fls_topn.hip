// fls_topn.hip -- gfx950 kernels of the top-N scan (fls_topn.hpp).
//
// Integer work on LDS (no MFMA).  In LDS a record is a 64-bit key in one array
// and a 32-bit tag (rank << 30 | row) in another: consecutive lanes then read
// consecutive 8- and 4-byte words (ds_read_b64 / ds_read_b32 without a bank
// conflict), where 16-byte records would put lanes l and l + 16 on one bank
// row.  The tag orders (rank, row) by itself, so records compare as
// (tag >> 30, key, tag).
//
// Stage 1: a 256-thread block owns one 1024-row vector with filter_kernel's
// mapping (wave w: the 64-row words 4w..4w+3, lane = row within the word), so
// a mask or validity word is one broadcast load.  The block sorts the vector's
// 1024 records -- ineligible rows as a sentinel of rank 2 -- with a bitonic
// network in 12 KB of LDS and writes the best min(k, eligible), the row as
// the row within the batch.  Stage 2 merges the vectors' lists of each row
// group pairwise, level by level (topn_merge_kernel: one launch per level, one
// block per pair, 24 KB of LDS): two sorted lists merge by rank -- every record
// finds its place in the other list by binary search; no two records are
// equal -- and the better k are kept.  A row group's vectors are merged by a
// tree instead of one after the other because one block per row group left
// all but a batch's eight CUs idle for 64 dependent merges.  No atomics,
// nothing shared between the blocks of a launch, no scratch.
#include <hip/hip_runtime.h>

#include "fls_topn.hpp"

namespace fls {
namespace {

constexpr uint32_t kRowBits = 30;  // tag = rank << kRowBits | row
constexpr uint32_t kRowMask = (1u << kRowBits) - 1;

__device__ __forceinline__ bool rec_less(uint64_t ka, uint32_t ta, uint64_t kb, uint32_t tb) {
    const uint32_t ra = ta >> kRowBits, rb = tb >> kRowBits;
    if (ra != rb) return ra < rb;
    if (ka != kb) return ka < kb;
    return ta < tb;
}

// the key column's value at p, as topn_key takes it
__device__ __forceinline__ uint64_t load_raw(const uint8_t *p, uint32_t ob, uint8_t kind) {
    if (kind == FK_FLOAT) {
        const double d = ob == 4 ? (double)*(const float *)p : *(const double *)p;
        uint64_t b;
        __builtin_memcpy(&b, &d, 8);
        return b;
    }
    uint64_t lo, hi;
    load_wide(p, ob, kind == FK_INT, lo, hi);
    return lo;
}

__global__ __launch_bounds__(256) void topn_vector_kernel(DevTopn p, uint8_t *__restrict__ out) {
    __shared__ uint64_t skey[1024];
    __shared__ uint32_t stag[1024];
    __shared__ uint32_t scnt[4];
    const uint32_t v = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint64_t m[4], nn[4];
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t word = 4 * w + k;
        const uint64_t base = (uint64_t)v * 1024 + 64 * word;
        // rows of this word below nrows: no row past the batch is loaded whatever the mask holds
        m[k] = base >= p.nrows ? 0ull : (p.nrows - base >= 64 ? ~0ull : (1ull << (p.nrows - base)) - 1);
        if (p.mask) m[k] &= p.mask[(size_t)v * 16 + word];
        nn[k] = m[k];
        if (p.valid) nn[k] &= p.valid[(size_t)v * 16 + word];
        cnt += (uint32_t)__popcll(m[k]);
    }
    if (lane == 0) scnt[w] = cnt;
    __syncthreads();
    const uint32_t total = scnt[0] + scnt[1] + scnt[2] + scnt[3];
    const uint32_t n = total < p.k ? total : p.k;
    uint8_t *list = out + (size_t)v * topn_stride(p.k);
    if (threadIdx.x == 0) {
        TopnHdr h;
        h.count = n;
        h.pad[0] = h.pad[1] = h.pad[2] = 0;
        *(TopnHdr *)list = h;
    }
    if (total == 0) return;  // (the whole block)
    const uint32_t null_rank = p.nulls_first ? 0u : 1u, value_rank = 1u - null_rank;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t idx = 256 * w + 64 * k + lane;  // row within the vector
        uint64_t key = ~0ull;
        uint32_t tag = (2u << kRowBits) | (v * 1024 + idx);  // not eligible: worse than any record
        if ((m[k] >> lane) & 1) {
            if ((nn[k] >> lane) & 1) {
                const uint64_t row = (uint64_t)v * 1024 + idx;
                key = topn_key(load_raw(p.col + row * p.ob, p.ob, p.kind), p.kind, p.desc != 0);
                tag = (value_rank << kRowBits) | (v * 1024 + idx);
            } else {  // a NULL key: its placeholder is never loaded
                key = 0;
                tag = (null_rank << kRowBits) | (v * 1024 + idx);
            }
        }
        skey[idx] = key;
        stag[idx] = tag;
    }
    __syncthreads();
    // bitonic network over the 1024 records, two compare-exchanges per thread and step
    for (uint32_t size = 2; size <= 1024; size <<= 1) {
        for (uint32_t j = size >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (uint32_t q = 0; q < 2; ++q) {
                const uint32_t pr = threadIdx.x + 256 * q;
                const uint32_t i = ((pr & ~(j - 1)) << 1) | (pr & (j - 1)), o = i | j;
                const bool up = (i & size) == 0;
                const uint64_t ka = skey[i], kb = skey[o];
                const uint32_t ta = stag[i], tb = stag[o];
                if (rec_less(kb, tb, ka, ta) == up) {
                    skey[i] = kb;
                    stag[i] = tb;
                    skey[o] = ka;
                    stag[o] = ta;
                }
            }
            __syncthreads();
        }
    }
    TopnRec *recs = (TopnRec *)(list + sizeof(TopnHdr));
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        TopnRec r;
        r.key = skey[i];
        r.row = stag[i] & kRowMask;
        r.rank = stag[i] >> kRowBits;
        recs[i] = r;
    }
}

// records of a[0..n) that are better than (key, tag)
__device__ __forceinline__ uint32_t count_less(const uint64_t *akey, const uint32_t *atag, uint32_t n, uint64_t key,
                                               uint32_t tag) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rec_less(akey[mid], atag[mid], key, tag)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One merge of the tree: block (j, r) merges lists 2j and 2j + 1 of row group
// r at this level (src) into its list j of the next (dst; at the last level
// the row group's list in the output).  A row group of nv vectors has
// ceil(nv / 2^level) lists at a level, kept at its first vector's index onwards.
__global__ __launch_bounds__(256) void topn_merge_kernel(const uint32_t *__restrict__ rgvec, uint32_t nvec, uint32_t k,
                                                         uint32_t level, uint32_t last, const uint8_t *__restrict__ src,
                                                         uint8_t *__restrict__ dst) {
    __shared__ uint64_t akey[kMaxTopN], bkey[kMaxTopN];
    __shared__ uint32_t atag[kMaxTopN], btag[kMaxTopN];
    const uint32_t r = blockIdx.y, j = blockIdx.x, v0 = rgvec[2 * r], nv = rgvec[2 * r + 1];
    const uint32_t nl = (nv + (1u << level) - 1) >> level;  // this row group's lists at this level
    if (2 * j >= nl && !(last && j == 0)) return;           // (the whole block)
    const size_t stride = topn_stride(k);
    uint8_t *out = dst + (size_t)(last ? r : v0 + j) * stride;
    const uint32_t ia = v0 + 2 * j, ib = ia + 1;
    const bool has_a = 2 * j < nl && ia < nvec, has_b = 2 * j + 1 < nl && ib < nvec;
    const uint8_t *la = src + (size_t)ia * stride, *lb = src + (size_t)ib * stride;
    uint32_t na = has_a ? ((const TopnHdr *)la)->count : 0, nb = has_b ? ((const TopnHdr *)lb)->count : 0;
    na = na < k ? na : k;
    nb = nb < k ? nb : k;
    const TopnRec *ra = (const TopnRec *)(la + sizeof(TopnHdr)), *rb = (const TopnRec *)(lb + sizeof(TopnHdr));
    for (uint32_t i = threadIdx.x; i < na; i += 256) {
        const TopnRec x = ra[i];
        akey[i] = x.key;
        atag[i] = (x.rank << kRowBits) | (x.row & kRowMask);
    }
    for (uint32_t i = threadIdx.x; i < nb; i += 256) {
        const TopnRec x = rb[i];
        bkey[i] = x.key;
        btag[i] = (x.rank << kRowBits) | (x.row & kRowMask);
    }
    __syncthreads();
    TopnRec *ro = (TopnRec *)(out + sizeof(TopnHdr));
    for (uint32_t i = threadIdx.x; i < na; i += 256) {
        const uint64_t key = akey[i];
        const uint32_t tag = atag[i];
        const uint32_t pos = i + count_less(bkey, btag, nb, key, tag);
        if (pos < k) ro[pos] = TopnRec{key, tag & kRowMask, tag >> kRowBits};
    }
    for (uint32_t i = threadIdx.x; i < nb; i += 256) {
        const uint64_t key = bkey[i];
        const uint32_t tag = btag[i];
        const uint32_t pos = i + count_less(akey, atag, na, key, tag);
        if (pos < k) ro[pos] = TopnRec{key, tag & kRowMask, tag >> kRowBits};
    }
    if (threadIdx.x == 0) {
        TopnHdr h;
        h.count = na + nb < k ? na + nb : k;
        h.pad[0] = h.pad[1] = h.pad[2] = 0;
        *(TopnHdr *)out = h;
    }
}

}  // namespace

hipError_t launch_topn_vectors(const DevTopn &p, uint8_t *d_vec, hipStream_t stream) {
    const uint32_t nvec = (p.nrows + 1023) / 1024;
    if (nvec == 0) return hipSuccess;
    if (p.k == 0 || p.k > kMaxTopN || !d_vec || !p.col) return hipErrorInvalidValue;
    hipLaunchKernelGGL(topn_vector_kernel, dim3(nvec), dim3(256), 0, stream, p, d_vec);
    return hipGetLastError();
}

hipError_t launch_topn_rowgroups(const uint32_t *d_rgvec, uint32_t nrg, uint32_t rg_vecs, uint32_t nvec, uint32_t k,
                                 uint8_t *d_vec, uint8_t *d_tmp, uint8_t *d_rg, hipStream_t stream) {
    if (nrg == 0) return hipSuccess;
    if (k == 0 || k > kMaxTopN || rg_vecs == 0 || !d_rgvec || !d_vec || !d_tmp || !d_rg) return hipErrorInvalidValue;
    uint32_t levels = 1;
    while ((1u << levels) < rg_vecs) ++levels;
    uint8_t *src = d_vec, *dst = d_tmp;
    for (uint32_t l = 0; l < levels; ++l) {
        const uint32_t lists = (rg_vecs + (1u << l) - 1) >> l, last = l + 1 == levels ? 1 : 0;
        hipLaunchKernelGGL(topn_merge_kernel, dim3((lists + 1) / 2, nrg), dim3(256), 0, stream, d_rgvec, nvec, k, l, last,
                           (const uint8_t *)src, last ? d_rg : dst);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        uint8_t *t = src;
        src = dst;
        dst = t;
    }
    return hipSuccess;
}

}  // namespace fls
