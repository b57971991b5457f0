// fls_keymap.hpp -- key maps of the mapped GROUP BY keys: a function from
// 64-bit keys to 16-bit codes, probed per selected row by keymap_kernel
// (fls_keymap.hip) so that fls_aggregate_grouped can group by an attribute of
// a joined dimension table (fls_keymap_* in include/flsgpu.h).
//
// Host only (no HIP include): a map is built, queried and used for pruning
// without a GPU, and a stand-alone CPU program can drive this header
// (tests/fuzz/fuzz_keymap.cpp).  The image built here is the very byte
// sequence the scan uploads; keymap_lookup probes it the way keymap_kernel
// does.
//
// Keys are 64-bit patterns as in key sets (fls_keyset.hpp), ordered by
// `is_signed`; values are codes in [0, 65534].  0xFFFF (kKeymapAbsent) marks
// a hole and is no code.  A key listed twice with one value is kept once; with
// two values the map is no function and the build refuses it.
//
// Two forms:
//   dense  uint16[span + 1] indexed by key - min (mod 2^64), holes hold
//          kKeymapAbsent; padded to 8 bytes (the padding holds kKeymapAbsent);
//          span + 1 <= 2^31 (kKeymapMaxSpan): a 4 GiB image, the size of the
//          largest key-set image.
//   hash   the key set's table (capacity, keyset_home, ascending insertion,
//          the empty slot's sentinel, max_probe: fls_keyset.hpp builds it),
//          then at byte 8 * capacity a parallel uint16[capacity] of the slots'
//          codes, kKeymapAbsent in empty slots, padded to 8 bytes.
// Auto (form 0) takes the dense array when span + 1 <= 2^31 and either of two
// independent conditions holds: it is no larger than the hash image would be
// (10 bytes per slot, padded), or it is at most 1 MiB (kKeymapSmallDense).
// The second is not a consequence of the first (3 keys spread over 2^19 values: an 80-byte
// hash image, a 1 MiB array): a small array is taken even for a sparse map,
// one gather per probe.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "fls_keyset.hpp"

namespace fls {

constexpr uint16_t kKeymapAbsent = 0xFFFF;
constexpr uint64_t kKeymapMaxSpan = 1ull << 31;     // values a dense map may cover
constexpr uint64_t kKeymapSmallDense = 1ull << 20;  // bytes

enum KeymapForm : uint32_t { KM_AUTO = 0, KM_DENSE = 1, KM_HASH = 2 };
enum KeymapStatus : int { KM_OK = 0, KM_TOO_MANY = 1, KM_TOO_WIDE = 2, KM_BAD_FORM = 3, KM_BAD_VALUE = 4, KM_CONFLICT = 5 };

struct KeymapImage {
    uint32_t form = KM_HASH;       // KM_DENSE or KM_HASH
    // the map's keys as a key set: sorted keys (host pruning), min / max / span
    // and, for the hash form, capacity, sentinel and max_probe.  Its words are
    // moved into `words` below.
    KeysetImage set;
    std::vector<uint16_t> values;  // the codes of set.keys, in their order
    uint16_t max_code = 0;         // largest code (0 for the empty map)
    std::vector<uint64_t> words;   // the uploaded image
    // what a refused build reports: the offending key and its value(s)
    uint64_t bad_key = 0;
    uint32_t bad_a = 0, bad_b = 0;
    uint64_t bytes() const { return words.size() * 8; }
    uint64_t capacity() const { return form == KM_HASH ? 1ull << set.cap_log2 : 0; }
    const uint16_t *dense() const { return (const uint16_t *)words.data(); }
    const uint16_t *hash_values() const { return (const uint16_t *)(words.data() + capacity()); }
};

// bytes of either form
inline uint64_t keymap_dense_bytes(uint64_t span) { return ((span + 1) * 2 + 7) & ~7ull; }
inline uint64_t keymap_hash_bytes(uint32_t cap_log2) { return (8ull << cap_log2) + (((2ull << cap_log2) + 7) & ~7ull); }

// Probe of the image, as the kernel does it: the code, or kKeymapAbsent.
inline uint16_t keymap_lookup(const KeymapImage &m, uint64_t key) {
    const KeysetImage &s = m.set;
    if (m.form == KM_DENSE) {
        const uint64_t d = key - s.min;
        if (s.keys.empty() || d > s.span) return kKeymapAbsent;
        return m.dense()[d];
    }
    if (key == s.empty) return kKeymapAbsent;  // the sentinel is no key
    const uint64_t cap_mask = (1ull << s.cap_log2) - 1;
    const uint64_t h = keyset_home(key, s.cap_log2);
    for (uint32_t p = 0; p < s.max_probe; ++p) {
        const uint64_t i = (h + p) & cap_mask;
        const uint64_t slot = m.words[i];
        if (slot == key) return m.hash_values()[i];
        if (slot == s.empty) return kKeymapAbsent;
    }
    return kKeymapAbsent;
}

// The second half of every construction: keys holds the map's distinct keys,
// ascending in the key order, values their codes in that order, none of them
// kKeymapAbsent (the sort, the de-duplication and the checks of the values are
// the caller's: keymap_build below, or the device build of
// fls_keymap_from_scan, whose compact arrays arrive in key order).  Chooses
// the form (the auto rule above) and fills max_code and the image.
inline int keymap_finish_sorted(std::vector<uint64_t> sorted, std::vector<uint16_t> values, bool is_signed, uint32_t form,
                                KeymapImage &out) {
    if (form > KM_HASH) return KM_BAD_FORM;
    const uint64_t nd = sorted.size();
    if (nd > kMaxKeysetKeys || values.size() != nd) return KM_TOO_MANY;
    out = KeymapImage();
    out.values = std::move(values);
    for (uint64_t i = 0; i < nd; ++i) {
        if (out.values[i] == kKeymapAbsent) {
            out.bad_key = sorted[i];
            out.bad_a = out.values[i];
            return KM_BAD_VALUE;
        }
        out.max_code = std::max(out.max_code, out.values[i]);
    }
    const uint64_t span = nd ? sorted.back() - sorted.front() : 0;
    const uint32_t cap_log2 = keyset_cap_log2(nd);
    const bool fits = span < kKeymapMaxSpan;
    if (form == KM_DENSE && !fits) return KM_TOO_WIDE;
    if (form == KM_AUTO) {
        const uint64_t db = fits ? keymap_dense_bytes(span) : 0;
        form = fits && (db <= keymap_hash_bytes(cap_log2) || db <= kKeymapSmallDense) ? KM_DENSE : KM_HASH;
    }
    out.form = form;
    KeysetImage &s = out.set;
    if (form == KM_DENSE) {
        s.is_signed = is_signed;
        s.keys = std::move(sorted);
        if (nd) {
            s.min = s.keys.front();
            s.max = s.keys.back();
            s.span = span;
        }
        out.words.assign(keymap_dense_bytes(span) / 8, ~0ull);  // kKeymapAbsent everywhere
        uint16_t *a = (uint16_t *)out.words.data();
        for (uint64_t i = 0; i < nd; ++i) a[s.keys[i] - s.min] = out.values[i];
        return KM_OK;
    }
    // the key set's table over the sorted keys, then the slots' codes
    if (keyset_build(sorted.data(), nd, is_signed, KS_HASH, s) != KS_OK) return KM_BAD_FORM;
    sorted = {};
    const uint64_t cap = 1ull << s.cap_log2;
    out.words = std::move(s.words);
    s.words.clear();
    out.words.resize(keymap_hash_bytes(s.cap_log2) / 8, ~0ull);
    uint16_t *v = (uint16_t *)(out.words.data() + cap);  // kKeymapAbsent everywhere
    // a key's slot: the first match from its home, as every lookup finds it
    const uint64_t cap_mask = cap - 1;
    for (uint64_t i = 0; i < nd; ++i) {
        uint64_t j = keyset_home(s.keys[i], s.cap_log2);
        while (out.words[j] != s.keys[i]) j = (j + 1) & cap_mask;  // present: inserted above
        v[j] = out.values[i];
    }
    return KM_OK;
}

// Builds the map keys[i] -> values[i], i in [0, n): n is checked before keys
// or values is read.
inline int keymap_build(const uint64_t *keys, const uint16_t *values, uint64_t n, bool is_signed, uint32_t form,
                        KeymapImage &out) {
    if (form > KM_HASH) return KM_BAD_FORM;
    if (n > kMaxKeysetKeys) return KM_TOO_MANY;
    out = KeymapImage();
    std::vector<std::pair<uint64_t, uint16_t>> kv(n);
    for (uint64_t i = 0; i < n; ++i) {
        if (values[i] == kKeymapAbsent) {
            out.bad_key = keys[i];
            out.bad_a = values[i];
            return KM_BAD_VALUE;
        }
        kv[i] = {keys[i], values[i]};
    }
    std::sort(kv.begin(), kv.end(), [is_signed](const auto &a, const auto &b) {
        const uint64_t x = keyset_ord(a.first, is_signed), y = keyset_ord(b.first, is_signed);
        return x != y ? x < y : a.second < b.second;
    });
    kv.erase(std::unique(kv.begin(), kv.end()), kv.end());
    for (size_t i = 1; i < kv.size(); ++i)
        if (kv[i].first == kv[i - 1].first) {  // one key, two values: no function
            out.bad_key = kv[i].first;
            out.bad_a = kv[i - 1].second;
            out.bad_b = kv[i].second;
            return KM_CONFLICT;
        }
    const uint64_t nd = kv.size();
    std::vector<uint64_t> sorted(nd);
    std::vector<uint16_t> vals(nd);
    for (uint64_t i = 0; i < nd; ++i) {
        sorted[i] = kv[i].first;
        vals[i] = kv[i].second;
    }
    kv = {};
    return keymap_finish_sorted(std::move(sorted), std::move(vals), is_signed, form, out);
}

}  // namespace fls
