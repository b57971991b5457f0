// fls_groupagg.hip -- gfx950 kernels of the grouped aggregate scan
// (fls_groupagg.hpp).
//
// Stage 1 keeps aggregate_kernel's mapping (fls_agg.hip): a 256-thread block
// owns one 1024-row vector, wave w the 64-row words 4w..4w+3, lane = row
// within the word.  The distinct keys are found in rounds of "the lowest
// selected row without a slot wins the next slot": each wave offers its lowest
// such row (ffs over its wave-uniform words), the lowest wave that offers one
// wins, and every lane compares its rows with the winner's key -- one barrier
// per distinct key (the offers are double-buffered).  Each aggregate then
// loads its operand once per row and reduces it once per slot in exactly
// aggregate_kernel's order (lane rows 0..3, xor butterfly 32..1, waves 0..3;
// rows of other slots contribute the identity), so with a single group the
// records equal the ungrouped kernel's bit for bit.  The work is
// (slots of the vector) x (aggregates) wave reductions: meant for a handful of
// groups, correct up to kMaxVecGroups.
//
// Stage 2 walks a row group's vectors in order with one block: the vector's
// keys are looked up in an LDS table of kMaxRgGroups keys, new ones appended
// in slot order, and one thread per (vector slot, aggregate) folds the record
// into the row group's output.  Keys within a vector are distinct, so no two
// threads touch one accumulator; barriers separate the vectors.
//
// Both kernels check their capacity before they write a slot: past it they
// mark the header, raise KERR_GROUP_VEC / KERR_GROUP_RG and stop.
#include <hip/hip_runtime.h>

#include "fls_groupagg.hpp"

namespace fls {
namespace {

constexpr uint64_t kNegZero = 0x8000000000000000ull;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kNewSlot = 0x80000000u;

__device__ __forceinline__ uint64_t shfl64(uint64_t x, int d) {
    return (uint64_t)__shfl_xor((unsigned long long)x, d, 64);
}

__device__ __forceinline__ double load_float(const uint8_t *p, uint32_t ob) {
    return ob == 4 ? (double)*(const float *)p : *(const double *)p;
}

// value (< 2^64) or a single bit into the 128-bit key at bit sh
__device__ __forceinline__ void key_or(uint64_t &lo, uint64_t &hi, uint64_t v, uint32_t sh) {
    if (sh < 64) {
        lo |= v << sh;
        if (sh) hi |= v >> (64 - sh);
    } else {
        hi |= v << (sh - 64);
    }
}

__global__ __launch_bounds__(256) void group_vector_kernel(const DevKey *__restrict__ keys, uint32_t nkeys,
                                                           const DevAgg *__restrict__ aggs, uint32_t naggs,
                                                           uint32_t nrows, const uint64_t *__restrict__ mask,
                                                           uint8_t *__restrict__ out, uint32_t *err) {
    __shared__ uint64_t cand_key[2][4][2];           // per round parity and wave: the offered row's key
    __shared__ uint32_t cand_row[2][4];              // ... and its row in the vector (kNone: no offer)
    __shared__ uint64_t part[kMaxVecGroups][4][3];   // per slot and wave: count, lo, hi
    const uint32_t v = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint8_t *vout = out + (size_t)v * group_vec_stride(naggs);
    GroupHdr *hdr = (GroupHdr *)vout;
    uint64_t *okeys = (uint64_t *)(vout + sizeof(GroupHdr));
    AggRec *orecs = (AggRec *)(vout + sizeof(GroupHdr) + 16ull * kMaxVecGroups);

    // the selected rows and their packed keys
    uint64_t sel[4], klo[4], khi[4];
    uint32_t slot[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t word = 4 * w + k;
        const uint64_t base = (uint64_t)v * 1024 + 64 * word;
        // rows of this word below nrows: no row past the batch is ever selected
        uint64_t m = base >= nrows ? 0ull : (nrows - base >= 64 ? ~0ull : (1ull << (nrows - base)) - 1);
        if (mask) m &= mask[(size_t)v * 16 + word];
        sel[k] = m;
        klo[k] = khi[k] = 0;
        slot[k] = kNone;
        if (!((m >> lane) & 1)) continue;
        const uint64_t row = base + lane;
        for (uint32_t q = 0; q < nkeys; ++q) {
            const DevKey &dk = keys[q];
            const bool valid = !dk.valid || ((dk.valid[(size_t)v * 16 + word] >> lane) & 1);
            if (valid) {
                uint64_t x, xh;
                load_wide(dk.col + row * dk.ob, dk.ob, false, x, xh);
                key_or(klo[k], khi[k], x, dk.shift);
            } else {
                key_or(klo[k], khi[k], 1ull, dk.null_bit);
            }
        }
    }

    // slots in first-occurrence order
    uint64_t un[4] = {sel[0], sel[1], sel[2], sel[3]};  // selected rows without a slot (wave-uniform)
    uint64_t has = 0;                                   // slots with a row in this wave
    uint32_t ng = 0;
    bool over = false;
    for (;;) {
        const uint32_t b = ng & 1;
        uint32_t kk = 4;
#pragma unroll
        for (int k = 3; k >= 0; --k)
            if (un[k]) kk = (uint32_t)k;
        if (kk < 4) {
            const uint64_t uw = kk == 0 ? un[0] : kk == 1 ? un[1] : kk == 2 ? un[2] : un[3];
            const uint32_t bit = (uint32_t)__ffsll((unsigned long long)uw) - 1;
            if (lane == bit) {
                cand_key[b][w][0] = kk == 0 ? klo[0] : kk == 1 ? klo[1] : kk == 2 ? klo[2] : klo[3];
                cand_key[b][w][1] = kk == 0 ? khi[0] : kk == 1 ? khi[1] : kk == 2 ? khi[2] : khi[3];
                cand_row[b][w] = 64 * (4 * w + kk) + bit;
            }
        } else if (lane == 0) {
            cand_row[b][w] = kNone;
        }
        __syncthreads();
        uint32_t win = 4;  // wave order is row order
#pragma unroll
        for (int i = 3; i >= 0; --i)
            if (cand_row[b][i] != kNone) win = (uint32_t)i;
        if (win == 4) break;
        if (ng == kMaxVecGroups) {  // a 65th key: nothing more is written
            over = true;
            break;
        }
        const uint64_t wlo = cand_key[b][win][0], whi = cand_key[b][win][1];
        if (threadIdx.x == 0) {
            okeys[2 * ng] = wlo;
            okeys[2 * ng + 1] = whi;
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const bool hit = ((un[k] >> lane) & 1) && klo[k] == wlo && khi[k] == whi;
            const uint64_t bal = __ballot(hit);
            if (hit) slot[k] = ng;
            un[k] &= ~bal;
            if (bal) has |= 1ull << ng;
        }
        ++ng;
    }
    if (threadIdx.x == 0) {
        hdr->ngroups = over ? 0 : ng;
        hdr->overflow = over ? 1 : 0;
        hdr->pad = 0;
        if (over) atomicOr(err, KERR_GROUP_VEC);
    }
    if (over || ng == 0) return;

    for (uint32_t a = 0; a < naggs; ++a) {
        const DevAgg &g = aggs[a];
        const uint32_t fn = g.fn;
        const bool flt = g.kind == FK_FLOAT;
        const bool is_min = fn == AGG_MIN;
        // the operand, once per contributing row: integer sums (lo, hi), float
        // sums lo = binary64 bits, MIN / MAX lo = order key
        uint64_t cm[4], vlo[4], vhi[4];
        if (fn == AGG_SUM_EXPR) {
            // a loop of its own: as one more case of the loop below it cost the other functions
            // the schedule that keeps their four rows' loads in flight
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                cm[k] = sel[k];
                if (g.cond) cm[k] &= g.cond[(size_t)v * 16 + 4 * w + k];
                for (uint32_t i = 0; i < g.nf; ++i)
                    if (g.f[i].valid) cm[k] &= g.f[i].valid[(size_t)v * 16 + 4 * w + k];
            }
            expr_values(g, (uint64_t)v * 1024 + 256 * w + lane, cm, lane, vlo, vhi);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t word = 4 * w + k;
                uint64_t m = sel[k];
                if (g.cond) m &= g.cond[(size_t)v * 16 + word];
                if (fn != AGG_COUNT_STAR) {
                    if (g.valid) m &= g.valid[(size_t)v * 16 + word];
                    if (fn == AGG_SUM_PRODUCT && g.valid2) m &= g.valid2[(size_t)v * 16 + word];
                }
                cm[k] = m;
                vlo[k] = vhi[k] = 0;
                if (fn <= AGG_COUNT || !((m >> lane) & 1)) continue;
                const uint64_t row = (uint64_t)v * 1024 + 64 * word + lane;
                const uint8_t *p = g.col + row * g.ob;
                if (fn == AGG_SUM) {
                    if (flt) {
                        const double x = load_float(p, g.ob);
                        __builtin_memcpy(&vlo[k], &x, 8);
                    } else {
                        load_wide(p, g.ob, g.kind == FK_INT, vlo[k], vhi[k]);
                    }
                } else if (fn == AGG_SUM_PRODUCT) {
                    // the product of the sign- / zero-extended operands mod 2^128
                    uint64_t xl, xh, yl, yh;
                    load_wide(p, g.ob, g.kind == FK_INT, xl, xh);
                    load_wide(g.col2 + row * g.ob2, g.ob2, g.kind2 == FK_INT, yl, yh);
                    mul128(xl, xh, yl, yh);
                    vlo[k] = xl;
                    vhi[k] = xh;
                } else if (flt) {
                    vlo[k] = agg_key_float(load_float(p, g.ob));
                } else {
                    uint64_t xl, xh;
                    load_wide(p, g.ob, g.kind == FK_INT, xl, xh);
                    vlo[k] = g.kind == FK_INT ? agg_key_int((int64_t)xl) : xl;
                }
            }
        }
        __syncthreads();  // the previous aggregate's records are written: part is free
        for (uint32_t s = 0; s < ng; ++s) {
            uint64_t cnt = 0, lo = 0, hi = 0;
            double fsum = -0.0;
            if (is_min) lo = ~0ull;
            if ((has >> s) & 1) {  // (a wave without a row of the slot holds the identity)
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    const bool c = slot[k] == s && ((cm[k] >> lane) & 1);
                    cnt += (uint64_t)__popcll(__ballot(c));
                    if (fn > AGG_COUNT && c) {
                        if (fn == AGG_SUM && flt) fsum += as_double(vlo[k]);
                        else if (fn == AGG_SUM || fn == AGG_SUM_PRODUCT || fn == AGG_SUM_EXPR) add128(lo, hi, vlo[k], vhi[k]);
                        else lo = is_min ? (vlo[k] < lo ? vlo[k] : lo) : (vlo[k] > lo ? vlo[k] : lo);
                    }
                }
                if (fn == AGG_SUM && flt) {
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) fsum += __shfl_xor(fsum, d, 64);
                } else if (fn == AGG_SUM || fn == AGG_SUM_PRODUCT || fn == AGG_SUM_EXPR) {
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) {
                        const uint64_t ol = shfl64(lo, d), oh = shfl64(hi, d);
                        add128(lo, hi, ol, oh);
                    }
                } else if (fn == AGG_MIN || fn == AGG_MAX) {
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) {
                        const uint64_t o = shfl64(lo, d);
                        lo = is_min ? (o < lo ? o : lo) : (o > lo ? o : lo);
                    }
                }
            }
            if (fn == AGG_SUM && flt) __builtin_memcpy(&lo, &fsum, 8);
            if (lane == 0) {
                part[s][w][0] = cnt;
                part[s][w][1] = lo;
                part[s][w][2] = hi;
            }
        }
        __syncthreads();
        if (threadIdx.x < ng) {
            const uint32_t s = threadIdx.x;
            AggRec r;
            r.count = part[s][0][0];
            r.lo = part[s][0][1];
            r.hi = part[s][0][2];
            r.pad = 0;
            for (uint32_t i = 1; i < 4; ++i) {  // waves in order
                const uint64_t c = part[s][i][0], l = part[s][i][1], h = part[s][i][2];
                r.count += c;
                if (fn == AGG_SUM && flt) {
                    const double sum = as_double(r.lo) + as_double(l);
                    __builtin_memcpy(&r.lo, &sum, 8);
                } else if (fn == AGG_SUM || fn == AGG_SUM_PRODUCT || fn == AGG_SUM_EXPR) {
                    add128(r.lo, r.hi, l, h);
                } else if (fn == AGG_MIN) {
                    r.lo = l < r.lo ? l : r.lo;
                } else if (fn == AGG_MAX) {
                    r.lo = l > r.lo ? l : r.lo;
                }
            }
            orecs[(size_t)s * naggs + a] = r;
        }
    }
}

__global__ __launch_bounds__(256) void group_rowgroup_kernel(const DevAgg *__restrict__ aggs, uint32_t naggs,
                                                             uint32_t nfsum, const uint32_t *__restrict__ rgvec,
                                                             uint32_t rg_vecs, const uint8_t *__restrict__ vec_out,
                                                             uint8_t *rg_out, uint32_t *err) {
    __shared__ uint64_t tkey[kMaxRgGroups][2];  // the row group's keys in first-occurrence order
    __shared__ uint32_t map[kMaxVecGroups];     // the vector's slots -> table slots (| kNewSlot: appended by this vector)
    __shared__ uint32_t s_n, s_over;
    const uint32_t r = blockIdx.x, tid = threadIdx.x;
    const uint32_t v0 = rgvec[2 * r];
    const uint32_t nv = rgvec[2 * r + 1] < rg_vecs ? rgvec[2 * r + 1] : rg_vecs;
    uint8_t *rout = rg_out + (size_t)r * group_rg_stride(naggs, nfsum, rg_vecs);
    GroupHdr *hdr = (GroupHdr *)rout;
    uint64_t *okeys = (uint64_t *)(rout + sizeof(GroupHdr));
    AggRec *recs = (AggRec *)(rout + group_rg_recs_off());
    uint64_t *fvec = (uint64_t *)(rout + group_rg_fvec_off(naggs));
    const size_t vstride = group_vec_stride(naggs);

    for (size_t i = tid; i < (size_t)kMaxRgGroups * nfsum * rg_vecs; i += 256) fvec[i] = kNegZero;
    if (tid == 0) {
        s_n = 0;
        s_over = 0;
    }
    __syncthreads();
    uint32_t over = 0;
    for (uint32_t v = 0; v < nv; ++v) {
        const uint8_t *vb = vec_out + (size_t)(v0 + v) * vstride;
        const GroupHdr vh = *(const GroupHdr *)vb;
        if (vh.overflow) {  // (stage 1 raised its flag)
            over = 1;
            break;
        }
        const uint32_t ngv = vh.ngroups < kMaxVecGroups ? vh.ngroups : kMaxVecGroups;
        const uint64_t *vkeys = (const uint64_t *)(vb + sizeof(GroupHdr));
        const AggRec *vrecs = (const AggRec *)(vb + sizeof(GroupHdr) + 16ull * kMaxVecGroups);
        const uint32_t n = s_n;
        if (tid < ngv) {
            const uint64_t kl = vkeys[2 * tid], kh = vkeys[2 * tid + 1];
            uint32_t m = kNone;
            for (uint32_t j = 0; j < n; ++j)
                if (tkey[j][0] == kl && tkey[j][1] == kh) m = j;
            map[tid] = m;
        }
        __syncthreads();
        if (tid == 0) {  // new keys take the next slots, in the vector's slot order
            uint32_t nn = n;
            for (uint32_t t = 0; t < ngv; ++t) {
                if (map[t] != kNone) continue;
                if (nn == kMaxRgGroups) {  // a 257th key: nothing more is written
                    s_over = 1;
                    break;
                }
                tkey[nn][0] = vkeys[2 * t];
                tkey[nn][1] = vkeys[2 * t + 1];
                map[t] = nn | kNewSlot;
                ++nn;
            }
            s_n = nn;
        }
        __syncthreads();
        if (s_over) {
            over = 2;
            break;
        }
        for (uint32_t p = tid; p < ngv * naggs; p += 256) {
            const uint32_t t = p / naggs, a = p - t * naggs;
            const uint32_t m = map[t], s = m & ~kNewSlot;
            const AggRec rec = vrecs[(size_t)t * naggs + a];
            const DevAgg &g = aggs[a];
            const bool fsum = g.fn == AGG_SUM && g.kind == FK_FLOAT;
            AggRec *acc = recs + (size_t)s * naggs + a;
            if (fsum) fvec[((size_t)s * nfsum + g.fslot) * rg_vecs + v] = rec.lo;
            if (m & kNewSlot) {
                *acc = rec;
            } else if (rec.count) {
                AggRec x = *acc;
                x.count += rec.count;
                if (g.fn == AGG_SUM_PRODUCT || g.fn == AGG_SUM_EXPR || (g.fn == AGG_SUM && !fsum)) add128(x.lo, x.hi, rec.lo, rec.hi);
                else if (g.fn == AGG_MIN) x.lo = rec.lo < x.lo ? rec.lo : x.lo;
                else if (g.fn == AGG_MAX) x.lo = rec.lo > x.lo ? rec.lo : x.lo;
                *acc = x;
            }
        }
        __syncthreads();  // map and the accumulators are the next vector's
    }
    if (tid == 0) {
        hdr->ngroups = over ? 0 : s_n;
        hdr->overflow = over;
        hdr->pad = 0;
        if (over == 2) atomicOr(err, KERR_GROUP_RG);
    }
    if (over) return;
    for (uint32_t i = tid; i < s_n; i += 256) {
        okeys[2 * i] = tkey[i][0];
        okeys[2 * i + 1] = tkey[i][1];
    }
}

}  // namespace

hipError_t launch_group_vectors(const DevKey *d_keys, uint32_t nkeys, const DevAgg *d_aggs, uint32_t naggs,
                                uint32_t nrows, const uint64_t *d_mask, uint8_t *d_vec_out, uint32_t *d_err,
                                hipStream_t stream) {
    const uint32_t nvec = (nrows + 1023) / 1024;
    if (nvec == 0) return hipSuccess;
    if (nkeys == 0 || nkeys > kMaxKeys || naggs == 0 || naggs > kMaxAggs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_vector_kernel, dim3(nvec), dim3(256), 0, stream, d_keys, nkeys, d_aggs, naggs, nrows,
                       d_mask, d_vec_out, d_err);
    return hipGetLastError();
}

hipError_t launch_group_rowgroups(const DevAgg *d_aggs, uint32_t naggs, uint32_t nfsum, const uint32_t *d_rgvec,
                                  uint32_t nrg, uint32_t rg_vecs, const uint8_t *d_vec_out, uint8_t *d_rg_out,
                                  uint32_t *d_err, hipStream_t stream) {
    if (nrg == 0) return hipSuccess;
    if (naggs == 0 || naggs > kMaxAggs || nfsum > naggs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_rowgroup_kernel, dim3(nrg), dim3(256), 0, stream, d_aggs, naggs, nfsum, d_rgvec, rg_vecs,
                       d_vec_out, d_rg_out, d_err);
    return hipGetLastError();
}

}  // namespace fls
