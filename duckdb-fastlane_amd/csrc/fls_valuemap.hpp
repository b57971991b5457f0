// fls_valuemap.hpp -- value maps of the mapped filter terms: a function from
// 64-bit keys to 64-bit values, probed per selected row by mapcmp_kernel
// (fls_mapcmp.hip) so that a filter can compare a column with an attribute of
// a joined table (`col op map[key]`, OP_MAP_EQ .. OP_MAP_GE, fls_valuemap_* in
// include/flsgpu.h).  The sibling of the key map (fls_keymap.hpp), whose
// payload is a 16-bit GROUP BY code.
//
// Host only (no HIP include): a map is built, queried and used for pruning
// without a GPU, and a stand-alone CPU program can drive this header
// (tests/fuzz/fuzz_valuemap.cpp).  The image built here is the very byte
// sequence the scan uploads; valuemap_lookup probes it the way the kernels do:
// their one device probe, valuemap_probe, is at the end of this header (HIP
// compilations only), shared by mapcmp_kernel and mapval_kernel
// (fls_mapval.hip: map[key] as a derived column of the aggregate calls).
//
// Keys are 64-bit patterns as in key sets (fls_keyset.hpp), ordered by the key
// kind; values are 64-bit patterns ordered by the value kind (`value_signed`),
// which is the order of vmin / vmax and of the comparison.  Every 64-bit
// pattern is a value, so no pattern is left to mean "absent": the dense form
// carries a presence bitmap, the hash form the key set's sentinel.  A key
// listed twice with one value is kept once; with two values the map is no
// function and the build refuses it.
//
// Two forms:
//   dense  uint64 values[span + 1] indexed by key - min (mod 2^64), then a
//          presence bitmap uint64[(span + 64) / 64] (bit d & 63 of word
//          d >> 6); a hole holds value 0 and presence bit 0.
//          span + 1 <= 2^28 (kValuemapMaxSpan): a 2 GiB array.
//          bytes = 8 (span + 1) + 8 ((span + 64) / 64)   (valuemap_dense_bytes)
//   hash   the key set's table (capacity the next power of two >= 2 n,
//          keyset_home, ascending insertion, the empty slot's sentinel,
//          max_probe: fls_keyset.hpp builds it), then at byte 8 * capacity a
//          parallel uint64 values[capacity], 0 in empty slots.
//          bytes = 16 * capacity                         (valuemap_hash_bytes)
// Auto (form 0) takes the dense array when span + 1 <= 2^28 and either of two
// independent conditions holds: it is no larger than the hash image would be,
// or it is at most 1 MiB (kValuemapSmallDense).  Otherwise the hash table.
// The image is a pure function of the map: the pairs are sorted first, so
// shuffled or doubled input gives the same bytes.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "fls_keyset.hpp"

namespace fls {

constexpr uint64_t kValuemapMaxSpan = 1ull << 28;     // keys a dense map may cover
constexpr uint64_t kValuemapSmallDense = 1ull << 20;  // bytes

enum ValuemapForm : uint32_t { VM_AUTO = 0, VM_DENSE = 1, VM_HASH = 2 };
enum ValuemapStatus : int { VM_OK = 0, VM_TOO_MANY = 1, VM_TOO_WIDE = 2, VM_BAD_FORM = 3, VM_CONFLICT = 4 };

struct ValuemapImage {
    uint32_t form = VM_HASH;       // VM_DENSE or VM_HASH
    // the map's keys as a key set: sorted keys (host pruning), min / max / span
    // and, for the hash form, capacity, sentinel and max_probe.  Its words are
    // moved into `words` below.
    KeysetImage set;
    std::vector<uint64_t> values;  // the values of set.keys, in their order
    bool value_signed = true;      // the order of vmin / vmax and of the comparison
    uint64_t vmin = 0, vmax = 0;   // smallest / largest value in that order (0 for the empty map)
    std::vector<uint64_t> words;   // the uploaded image
    // what a refused build reports: the offending key and its two values
    uint64_t bad_key = 0, bad_a = 0, bad_b = 0;
    uint64_t bytes() const { return words.size() * 8; }
    uint64_t capacity() const { return form == VM_HASH ? 1ull << set.cap_log2 : 0; }
    const uint64_t *presence() const { return words.data() + set.span + 1; }           // dense
    const uint64_t *hash_values() const { return words.data() + capacity(); }          // hash
};

// bytes of either form
inline uint64_t valuemap_dense_bytes(uint64_t span) { return 8 * (span + 1) + 8 * ((span + 64) / 64); }
inline uint64_t valuemap_hash_bytes(uint32_t cap_log2) { return 16ull << cap_log2; }

// Probe of the image, as the kernel does it: true and *value when key is in the map.
inline bool valuemap_lookup(const ValuemapImage &m, uint64_t key, uint64_t *value) {
    const KeysetImage &s = m.set;
    if (m.form == VM_DENSE) {
        const uint64_t d = key - s.min;
        if (d > s.span) return false;
        if (!((m.presence()[d >> 6] >> (d & 63)) & 1)) return false;  // a hole (every bit of the empty map)
        if (value) *value = m.words[d];
        return true;
    }
    if (key == s.empty) return false;  // the sentinel is no key
    const uint64_t cap_mask = (1ull << s.cap_log2) - 1;
    const uint64_t h = keyset_home(key, s.cap_log2);
    for (uint32_t p = 0; p < s.max_probe; ++p) {
        const uint64_t i = (h + p) & cap_mask;
        const uint64_t slot = m.words[i];
        if (slot == key) {
            if (value) *value = m.hash_values()[i];
            return true;
        }
        if (slot == s.empty) return false;
    }
    return false;
}

// The second half of every construction: keys holds the map's distinct keys,
// ascending in the key order, values their values in that order (the sort,
// the de-duplication and the conflict check are the caller's: valuemap_build
// below, or the device build of fls_valuemap_from_scan, whose compact arrays
// arrive in key order).  Chooses the form (the auto rule above) and fills
// vmin / vmax and the image.
inline int valuemap_finish_sorted(std::vector<uint64_t> sorted, std::vector<uint64_t> values, bool key_signed,
                                  bool value_signed, uint32_t form, ValuemapImage &out) {
    if (form > VM_HASH) return VM_BAD_FORM;
    const uint64_t nd = sorted.size();
    if (nd > kMaxKeysetKeys || values.size() != nd) return VM_TOO_MANY;
    out = ValuemapImage();
    out.value_signed = value_signed;
    out.values = std::move(values);
    for (uint64_t i = 0; i < nd; ++i) {
        const uint64_t v = out.values[i];
        if (i == 0 || keyset_ord(v, value_signed) < keyset_ord(out.vmin, value_signed)) out.vmin = v;
        if (i == 0 || keyset_ord(v, value_signed) > keyset_ord(out.vmax, value_signed)) out.vmax = v;
    }
    const uint64_t span = nd ? sorted.back() - sorted.front() : 0;
    const uint32_t cap_log2 = keyset_cap_log2(nd);
    const bool fits = span < kValuemapMaxSpan;
    if (form == VM_DENSE && !fits) return VM_TOO_WIDE;
    if (form == VM_AUTO) {
        const uint64_t db = fits ? valuemap_dense_bytes(span) : 0;
        form = fits && (db <= valuemap_hash_bytes(cap_log2) || db <= kValuemapSmallDense) ? VM_DENSE : VM_HASH;
    }
    out.form = form;
    KeysetImage &s = out.set;
    if (form == VM_DENSE) {
        s.is_signed = key_signed;
        s.keys = std::move(sorted);
        if (nd) {
            s.min = s.keys.front();
            s.max = s.keys.back();
            s.span = span;
        }
        out.words.assign(valuemap_dense_bytes(span) / 8, 0);  // holes: value 0, presence bit 0
        uint64_t *present = out.words.data() + span + 1;
        for (uint64_t i = 0; i < nd; ++i) {
            const uint64_t d = s.keys[i] - s.min;
            out.words[d] = out.values[i];
            present[d >> 6] |= 1ull << (d & 63);
        }
        return VM_OK;
    }
    // the key set's table over the sorted keys, then the slots' values
    if (keyset_build(sorted.data(), nd, key_signed, KS_HASH, s) != KS_OK) return VM_BAD_FORM;
    sorted = {};
    const uint64_t cap = 1ull << s.cap_log2;
    out.words = std::move(s.words);
    s.words.clear();
    out.words.resize(valuemap_hash_bytes(s.cap_log2) / 8, 0);  // 0 in empty slots
    uint64_t *v = out.words.data() + cap;
    // a key's slot: the first match from its home, as every lookup finds it
    const uint64_t cap_mask = cap - 1;
    for (uint64_t i = 0; i < nd; ++i) {
        uint64_t j = keyset_home(s.keys[i], s.cap_log2);
        while (out.words[j] != s.keys[i]) j = (j + 1) & cap_mask;  // present: inserted above
        v[j] = out.values[i];
    }
    return VM_OK;
}

// Builds the map keys[i] -> values[i], i in [0, n): n is checked before keys
// or values is read.
inline int valuemap_build(const uint64_t *keys, const uint64_t *values, uint64_t n, bool key_signed, bool value_signed,
                          uint32_t form, ValuemapImage &out) {
    if (form > VM_HASH) return VM_BAD_FORM;
    if (n > kMaxKeysetKeys) return VM_TOO_MANY;
    out = ValuemapImage();
    out.value_signed = value_signed;
    std::vector<std::pair<uint64_t, uint64_t>> kv(n);
    for (uint64_t i = 0; i < n; ++i) kv[i] = {keys[i], values[i]};
    std::sort(kv.begin(), kv.end(), [key_signed](const auto &a, const auto &b) {
        const uint64_t x = keyset_ord(a.first, key_signed), y = keyset_ord(b.first, key_signed);
        return x != y ? x < y : a.second < b.second;
    });
    kv.erase(std::unique(kv.begin(), kv.end()), kv.end());
    for (size_t i = 1; i < kv.size(); ++i)
        if (kv[i].first == kv[i - 1].first) {  // one key, two values: no function
            out.bad_key = kv[i].first;
            out.bad_a = kv[i - 1].second;
            out.bad_b = kv[i].second;
            return VM_CONFLICT;
        }
    const uint64_t nd = kv.size();
    std::vector<uint64_t> sorted(nd), vals(nd);
    for (uint64_t i = 0; i < nd; ++i) {
        sorted[i] = kv[i].first;
        vals[i] = kv[i].second;
    }
    kv = {};
    return valuemap_finish_sorted(std::move(sorted), std::move(vals), key_signed, value_signed, form, out);
}

#ifdef __HIPCC__
// What the two kernels that probe a value map share (mapcmp_kernel,
// mapval_kernel): the load of a key or a left value, the widths a decoded
// column may have, and the probe.

// the value at p, sign- or zero-extended to 64 bits
__device__ __forceinline__ uint64_t valuemap_load(const uint8_t *p, uint32_t ob, bool sign) {
    switch (ob) {
    case 1: return sign ? (uint64_t)(int64_t) * (const int8_t *)p : (uint64_t)*p;
    case 2: return sign ? (uint64_t)(int64_t) * (const int16_t *)p : (uint64_t) * (const uint16_t *)p;
    case 4: return sign ? (uint64_t)(int64_t) * (const int32_t *)p : (uint64_t) * (const uint32_t *)p;
    default: return *(const uint64_t *)p;
    }
}

__device__ __forceinline__ bool valuemap_width_ok(uint32_t ob) { return ob == 1 || ob == 2 || ob == 4 || ob == 8; }

// Is key in the map, and its value (valuemap_lookup above), over any
// descriptor that carries the image's fields: table, min, span, empty,
// cap_log2, max_probe, form (DevMapCmpTerm, DevMapValTerm; fls_filter.hpp).
// Dense: a range test, then two independent loads, the presence word and the
// value (0 in a hole).  Hash: at most max_probe 8-byte gathers and one from
// the value array at the matched slot.
template <class Desc>
__device__ __forceinline__ bool valuemap_probe(const Desc &t, uint64_t key, uint64_t &value) {
    if (t.form == VM_DENSE) {
        const uint64_t d = key - t.min;
        if (d > t.span) return false;
        const uint64_t present = t.table[t.span + 1 + (d >> 6)];
        value = t.table[d];
        return (present >> (d & 63)) & 1;
    }
    if (key == t.empty) return false;  // the sentinel is no key
    const uint64_t cap_mask = (1ull << t.cap_log2) - 1;
    const uint64_t h = t.cap_log2 ? (key * kKeysetHashMul) >> (64 - t.cap_log2) : 0;
    for (uint32_t p = 0; p < t.max_probe; ++p) {
        const uint64_t i = (h + p) & cap_mask;
        const uint64_t slot = t.table[i];
        if (slot == key) {
            value = t.table[cap_mask + 1 + i];
            return true;
        }
        if (slot == t.empty) return false;
    }
    return false;
}
#endif

}  // namespace fls
