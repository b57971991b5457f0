// fls_dictstr.hip -- dictionary-string decode in the linear-fill shape.
//
// A DICT VARCHAR column turns 1-3 bits of packed code into a 16-byte string_t:
// more than 98 % of its traffic is stores.  The main decode writes such a
// column as a few thousand concurrent 1 MiB streams (one chunk per persistent
// wave), a shape a pure write of the same buffers runs 16 % below a linear
// fill (scripts/membw12.hip, profiles/r7/membw12.txt: 5.72 against 6.86 TB/s).
// This kernel keeps the fill's shape instead: a non-persistent grid of
// 256-thread workgroups in ascending output address (as a few interleaved
// streams, one per column in lineitem: flsgpu.hip order_for_launch), one
// 1024-value vector (16 KiB of output) per workgroup, every store instruction
// of a workgroup 4 KiB contiguous and the four of them issued back to back.
// lineitem_full SF100: the four string columns in 5.76 ms = 6.78 TB/s against
// 6.92 ms in the main decode, c4 2.50 against 2.81 ms.
//
// What a workgroup must load before it can store is a dependent chain, and
// the write rate falls with every link of it (membw12: 5.48 TB/s with the
// table gathered from global memory after the codes, 6.08 TB/s with two
// links).  So the chain is two global round trips:
//   1. the vector's 32-byte descriptor (DictVec, built by the host: scalar
//      load, nothing of the chunk header or the VecMeta array is chased);
//   2. side by side, each thread's packed words (a value's FastLanes position
//      is a pure function of its index: DICT codes are packed at T = 32 in
//      natural order, value p in word-row p / 32, lane p % 32) and the
//      dictionary's string_t table into LDS (at most kDictWgMaxEntries);
// then the table gather is an LDS read.  Semantics are PathDict<16>'s
// (fls_decode_dev.hpp): code = unpacked + base (32-bit wrap), a code >=
// dict_count is clamped to dict_count - 1 and raises KERR_DICT_CODE, the
// partial last vector stores only its nvals records.  Nothing depends on the
// order workgroups are dispatched in: each writes its own vector only.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "fls_decode.hpp"
#include "fls_format.hpp"
#include "fls_unpack.hpp"

namespace fls {
using namespace dev;
namespace {

constexpr uint32_t kRounds = kVectorSize / 256;  // 4 KiB stores per workgroup
static_assert(kDictWgMaxEntries == 64, "one wave stages the table, one entry per lane");

}  // namespace

// RATING: the same kernel under another name for the upload's placement
// rating launches (rating_launch()), as decode_kernel and fused_kernel have
template <bool RATING>
__global__ __launch_bounds__(256) void dictstr_decode_kernel(const DictVec *__restrict__ vecs,
                                                             uint32_t *__restrict__ err) {
    __shared__ v4u tab[kDictWgMaxEntries];
    // (the grid is exactly one workgroup per descriptor: launch_dictstr)
    // the descriptor in one scalar load (constant address space: s_load_dwordx8)
    typedef uint32_t v8u __attribute__((ext_vector_type(8)));
    const v8u q = ((const __attribute__((address_space(4))) v8u *)vecs)[blockIdx.x];
    const uint64_t packed = (uint64_t)q[1] << 32 | q[0], tab_g = (uint64_t)q[3] << 32 | q[2];
    const uint64_t out_g = (uint64_t)q[5] << 32 | q[4];
    const uint32_t base = q[6], info = q[7];
    const uint32_t t = threadIdx.x;
    const uint32_t nvals = info & 2047u, W = (info >> 11) & 63u, n = info >> 17;
    // wave 0 stages the table: its load is issued before the packed loads and
    // written to LDS after them, so the two wait side by side
    const bool stager = uni(t >> 6) == 0;
    v4u te = mk4(0, 0, 0, 0);
    if (stager) te = ((const FLS_GLOBAL v4u *)tab_g)[min(t, n - 1)];
    uint32_t code[kRounds];
    if (W == 0) {
#pragma unroll
        for (uint32_t r = 0; r < kRounds; ++r) code[r] = 0;
    } else {
        // value p = 256 r + t: bits [row W, row W + W) of lane p % 32's word
        // column, row = p / 32; the W word-rows of 32 words lie back to back.
        // The word after the last is never needed (row W + W <= 32 W), so its
        // index is clamped instead of padded.
        const FLS_GLOBAL uint32_t *pk = ((const FLS_GLOBAL uint32_t *)packed) + (t & 31);
        const uint32_t mask = W >= 32 ? 0xFFFFFFFFu : (1u << W) - 1u;
        uint32_t lo[kRounds], hi[kRounds];
#pragma unroll
        for (uint32_t r = 0; r < kRounds; ++r) {
            const uint32_t k = ((8 * r + (t >> 5)) * W) >> 5;
            lo[r] = pk[32 * k];
            hi[r] = pk[32 * min(k + 1, W - 1)];
        }
#pragma unroll
        for (uint32_t r = 0; r < kRounds; ++r)
            code[r] = __builtin_amdgcn_alignbit(hi[r], lo[r], ((8 * r + (t >> 5)) * W) & 31) & mask;
    }
    if (stager) tab[t] = te;  // (t < 64 = kDictWgMaxEntries; entries past n repeat the last)
    bool bad = false;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        code[r] += base;
        if (code[r] >= n) {
            bad = true;  // (also in the padding of a partial vector, as PathDict)
            code[r] = n - 1;
        }
    }
    __syncthreads();
    v4u e[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) e[r] = tab[code[r]];
    FLS_GLOBAL v4u *out = ((FLS_GLOBAL v4u *)out_g) + t;
    if (nvals == kVectorSize) {
#pragma unroll
        for (uint32_t r = 0; r < kRounds; ++r) out[256 * r] = e[r];
    } else {
#pragma unroll
        for (uint32_t r = 0; r < kRounds; ++r)
            if (256 * r + t < nvals) out[256 * r] = e[r];
    }
    if (__any(bad) && (t & 63) == 0) atomicOr(err, KERR_DICT_CODE);
}

hipError_t launch_dictstr(const DictVec *d_vecs, uint32_t nvecs, uint32_t *d_err, hipStream_t stream) {
    if (nvecs == 0) return hipSuccess;
    auto kern = rating_launch() ? dictstr_decode_kernel<true> : dictstr_decode_kernel<false>;
    if (getenv("FLS_DEBUG"))
        fprintf(stderr, "DEBUG: dictstr_decode_kernel: %u blocks of 256 threads, %u vectors\n", nvecs, nvecs);
    hipLaunchKernelGGL(kern, dim3(nvecs), dim3(256), 0, stream, d_vecs, d_err);
    return hipGetLastError();
}

}  // namespace fls
