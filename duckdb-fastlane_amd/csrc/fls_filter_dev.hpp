// fls_filter_dev.hpp -- the per-row term evaluation filter_kernel
// (fls_filter.hip) and cond_kernel (fls_cond.hip) share: one ordinary term
// `column op constant` / IS [NOT] NULL of a DevTerm against one row of the
// decoded batch, with the loaders and the string comparison it needs.  Device
// code only; included by those two units.
#pragma once
#include <hip/hip_runtime.h>

#include "fls_filter.hpp"

namespace fls {
namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int64_t load_int(const uint8_t *p, uint32_t ob) {
    switch (ob) {
    case 1: return *(const int8_t *)p;
    case 2: return *(const int16_t *)p;
    case 4: return *(const int32_t *)p;
    default: return *(const int64_t *)p;
    }
}
__device__ __forceinline__ uint64_t load_uint(const uint8_t *p, uint32_t ob) {
    switch (ob) {
    case 1: return *p;
    case 2: return *(const uint16_t *)p;
    case 4: return *(const uint32_t *)p;
    default: return *(const uint64_t *)p;
    }
}

__device__ __forceinline__ bool in_range(const StrRange &r, uint64_t hp, uint32_t len) {
    return hp >= r.host_lo && hp <= r.host_hi && len <= r.host_hi - hp;
}

// string_t record at p against the term's constant
__device__ __forceinline__ int cmp_string(const DevTerm &t, const uint8_t *p, bool &bad) {
    const v4u rec = *(const v4u *)p;
    const uint32_t len = rec.x;
    // the 4 bytes after the length are the string's first bytes in both the
    // inlined and the pointer form: most comparisons end there
    const uint32_t k = min(4u, min(len, t.str_len));
    for (uint32_t i = 0; i < k; ++i) {
        const uint8_t a = p[4 + i], b = t.str[i];
        if (a != b) return a < b ? -1 : 1;
    }
    if (len <= 4 || t.str_len <= 4) return len < t.str_len ? -1 : (len > t.str_len ? 1 : 0);
    if ((t.op == OP_EQ || t.op == OP_NE) && len != t.str_len) return 1;
    const uint8_t *s;
    if (len <= 12) {
        s = p + 4;
    } else {
        // the batch heap (FSST rows) or the uploaded image (DICT rows); a
        // pointer inside neither is reported and never dereferenced
        const uint64_t hp = ((uint64_t)rec.w << 32) | rec.z;
        if (in_range(t.heap, hp, len)) {
            s = (const uint8_t *)(hp + t.heap.dev_delta);
        } else if (in_range(t.image, hp, len)) {
            s = (const uint8_t *)(hp + t.image.dev_delta);
        } else {
            bad = true;
            return 1;
        }
    }
    return cmp_bytes(s + 4, len - 4, t.str + 4, t.str_len - 4);
}

__device__ __forceinline__ bool eval_term(const DevTerm &t, uint64_t row, bool &bad) {
    // one word per 64 rows: a wave's lanes read the same word (a broadcast)
    const bool valid = !t.valid || ((t.valid[row >> 6] >> (row & 63)) & 1);
    if (t.op == OP_FALSE) return false;
    if (t.op >= OP_IS_NULL) return (t.op == OP_IS_NOT_NULL) == valid;
    if (!valid) return false;  // a NULL row satisfies no comparison
    const uint8_t *p = t.col + row * t.ob;
    int c;
    switch (t.kind) {
    case FK_INT: c = cmp_int(load_int(p, t.ob), (int64_t)t.value); break;
    case FK_UINT: c = cmp_uint(load_uint(p, t.ob), t.value); break;
    case FK_FLOAT: c = cmp_float(t.ob == 4 ? (double)*(const float *)p : *(const double *)p, as_double(t.value)); break;
    default: c = cmp_string(t, p, bad); break;
    }
    return op_holds(t.op, c);
}

}  // namespace
}  // namespace fls
