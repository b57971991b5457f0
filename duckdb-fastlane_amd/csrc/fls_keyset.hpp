// fls_keyset.hpp -- key sets of the pushed-down semi-join filter
// (`column IN set` / `column NOT IN set`, fls_keyset_* in include/flsgpu.h).
//
// Host only (no HIP include): a set is built, queried and used for pruning
// without a GPU, and a stand-alone CPU program can drive this header
// (tests/fuzz/fuzz_keyset.cpp, tests/fuzz/keyset_bitmap_host.cpp).  A set is
// built from a key list (keyset_build) or from the bitmap a scan collected its
// keys in (keyset_from_bitmap, fls_keyset_from_scan); both end in
// keyset_finish.  The image built here is the very byte
// sequence the scan uploads; keyset_contains probes it the way keyset_kernel
// (fls_keyset.hip) does.
//
// Keys are 64-bit patterns of the column's physical type, sign- or
// zero-extended; `is_signed` is the order of min / max, of the sorted key
// list (host pruning binary-searches it) and of a bitmap's base.
//
// Two forms:
//   bitmap  one bit per value of [min, max]: bit d = key - min (mod 2^64) is
//           bit (d & 63) of 64-bit word d >> 6 -- on the little-endian device,
//           bit (d & 31) of dword d >> 5.  span = max - min < 2^32.
//   hash    open addressing, linear probing, 8-byte slots; capacity = the next
//           power of two >= 2 n (1 for the empty set); home slot of key k =
//           (k * 0x9E3779B97F4A7C15) >> (64 - log2(capacity)) (0 when the
//           capacity is 1).  Keys are inserted in sorted order, so the image
//           is a pure function of the set.  The empty slot holds a sentinel:
//           the largest 64-bit pattern that is not a key (~0, else ~0 - 1,
//           ...), so every 64-bit key is representable without a side flag.
//           max_probe = the largest number of slots examined to find a key of
//           the set; a lookup stops at a match, at an empty slot, or after
//           max_probe slots (the key is then absent), so it never spins.
// Auto (form 0) takes the bitmap when span + 1 <= 2^32 and either of two
// independent conditions holds: the bitmap is no larger than the hash table
// would be, or it is at most 1 MiB (kKeysetSmallBitmap).  The second is not a
// consequence of the first (3 keys 2^23 apart: a 64-byte table, a 1 MiB
// bitmap): a small bitmap is taken even for a sparse set, one gather per probe.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace fls {

constexpr uint64_t kMaxKeysetKeys = 1ull << 28;
constexpr uint64_t kKeysetHashMul = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kKeysetSmallBitmap = 1ull << 20;  // bytes
constexpr uint64_t kKeysetMaxSpan = 1ull << 32;      // values a bitmap may cover

enum KeysetForm : uint32_t { KS_AUTO = 0, KS_BITMAP = 1, KS_HASH = 2 };
enum KeysetStatus : int { KS_OK = 0, KS_TOO_MANY = 1, KS_TOO_WIDE = 2, KS_BAD_FORM = 3 };

struct KeysetImage {
    uint32_t form = KS_HASH;       // KS_BITMAP or KS_HASH
    bool is_signed = true;
    std::vector<uint64_t> keys;    // distinct, ascending in the set's order
    uint64_t min = 0, max = 0;     // patterns (0 for the empty set)
    uint64_t span = 0;             // max - min
    uint32_t cap_log2 = 0;         // hash: capacity = 1 << cap_log2
    uint64_t empty = ~0ull;        // hash: the empty slot's sentinel
    uint32_t max_probe = 0;        // hash: longest probe sequence of a key
    std::vector<uint64_t> words;   // the uploaded image: bitmap words or hash slots
    uint64_t bytes() const { return words.size() * 8; }
    uint64_t capacity() const { return form == KS_HASH ? 1ull << cap_log2 : 0; }
};

// order-preserving map of a key pattern onto unsigned order
inline uint64_t keyset_ord(uint64_t k, bool is_signed) { return is_signed ? k ^ (1ull << 63) : k; }

inline uint64_t keyset_home(uint64_t k, uint32_t cap_log2) {
    return cap_log2 ? (k * kKeysetHashMul) >> (64 - cap_log2) : 0;
}

// bytes of either form for n distinct keys of the given span
inline uint64_t keyset_bitmap_bytes(uint64_t span) { return (span / 64 + 1) * 8; }
inline uint32_t keyset_cap_log2(uint64_t n) {
    uint32_t l = 0;
    while ((1ull << l) < 2 * n) ++l;
    return l;
}

// Is key in the sorted key list?  (the reference the images are checked against)
inline bool keyset_has_key(const KeysetImage &s, uint64_t key) {
    const bool sg = s.is_signed;
    auto it = std::lower_bound(s.keys.begin(), s.keys.end(), key,
                               [sg](uint64_t a, uint64_t b) { return keyset_ord(a, sg) < keyset_ord(b, sg); });
    return it != s.keys.end() && *it == key;
}

// Does a key lie in [lo, hi] (the set's order)?  Host pruning against a zone map.
inline bool keyset_any_in_range(const KeysetImage &s, uint64_t lo, uint64_t hi) {
    const bool sg = s.is_signed;
    auto it = std::lower_bound(s.keys.begin(), s.keys.end(), lo,
                               [sg](uint64_t a, uint64_t b) { return keyset_ord(a, sg) < keyset_ord(b, sg); });
    return it != s.keys.end() && keyset_ord(*it, sg) <= keyset_ord(hi, sg);
}

// Probe of the image, as the kernel does it.
inline bool keyset_contains(const KeysetImage &s, uint64_t key) {
    if (s.form == KS_BITMAP) {
        const uint64_t d = key - s.min;
        if (s.keys.empty() || d > s.span) return false;
        return (s.words[d >> 6] >> (d & 63)) & 1;
    }
    if (key == s.empty) return false;  // the sentinel is no key
    const uint64_t cap_mask = (1ull << s.cap_log2) - 1;
    const uint64_t h = keyset_home(key, s.cap_log2);
    for (uint32_t p = 0; p < s.max_probe; ++p) {
        const uint64_t slot = s.words[(h + p) & cap_mask];
        if (slot == key) return true;
        if (slot == s.empty) return false;
    }
    return false;
}

// The second half of every construction: out.is_signed is set and out.keys
// holds the distinct keys, ascending in the set's order; chooses the form
// (the auto rule above) and fills min / max / span, the bitmap or the hash
// table, the sentinel and max_probe.
inline int keyset_finish(KeysetImage &out, uint32_t form) {
    if (form > KS_HASH) return KS_BAD_FORM;
    const uint64_t nd = out.keys.size();
    if (nd > kMaxKeysetKeys) return KS_TOO_MANY;
    out.min = out.max = out.span = 0;
    out.cap_log2 = 0;
    out.empty = ~0ull;
    out.max_probe = 0;
    out.words.clear();
    if (nd) {
        out.min = out.keys.front();
        out.max = out.keys.back();
        out.span = out.max - out.min;
    }
    const uint32_t cap_log2 = keyset_cap_log2(nd);
    const bool fits = out.span < kKeysetMaxSpan;
    if (form == KS_BITMAP && !fits) return KS_TOO_WIDE;
    if (form == KS_AUTO) {
        const uint64_t bb = fits ? keyset_bitmap_bytes(out.span) : 0;
        form = fits && (bb <= (8ull << cap_log2) || bb <= kKeysetSmallBitmap) ? KS_BITMAP : KS_HASH;
    }
    out.form = form;
    if (form == KS_BITMAP) {
        out.words.assign(keyset_bitmap_bytes(out.span) / 8, 0);
        for (uint64_t k : out.keys) {
            const uint64_t d = k - out.min;
            out.words[d >> 6] |= 1ull << (d & 63);
        }
        return KS_OK;
    }
    out.cap_log2 = cap_log2;
    uint64_t e = ~0ull;
    while (keyset_has_key(out, e)) --e;  // at most nd steps
    out.empty = e;
    const uint64_t cap = 1ull << cap_log2, cap_mask = cap - 1;
    out.words.assign(cap, e);
    for (uint64_t k : out.keys) {
        uint64_t i = keyset_home(k, cap_log2);
        uint32_t probes = 1;
        while (out.words[i] != e) {  // capacity >= 2 n: an empty slot exists
            i = (i + 1) & cap_mask;
            ++probes;
        }
        out.words[i] = k;
        out.max_probe = std::max(out.max_probe, probes);
    }
    return KS_OK;
}

// Builds the set of keys[0, n): n is checked before keys is read.
inline int keyset_build(const uint64_t *keys, uint64_t n, bool is_signed, uint32_t form, KeysetImage &out) {
    if (form > KS_HASH) return KS_BAD_FORM;
    if (n > kMaxKeysetKeys) return KS_TOO_MANY;
    out = KeysetImage();
    out.is_signed = is_signed;
    out.keys.assign(keys, keys + n);
    std::sort(out.keys.begin(), out.keys.end(),
              [is_signed](uint64_t a, uint64_t b) { return keyset_ord(a, is_signed) < keyset_ord(b, is_signed); });
    out.keys.erase(std::unique(out.keys.begin(), out.keys.end()), out.keys.end());
    return keyset_finish(out, form);
}

// Builds the set a collecting bitmap holds (the device build of
// fls_keyset_from_scan): bit d of words[0, span / 64 + 1), d <= span, stands
// for the key base + d (mod 2^64); bits past span are ignored.  base is the
// smallest value of the collecting range in the set's order, so ascending d
// is that order (the caller keeps base + span from wrapping past the order's
// end).  The image equals keyset_build's over the same keys: the count is
// checked before a key is stored.
inline int keyset_from_bitmap(const uint64_t *words, uint64_t base, uint64_t span, bool is_signed, uint32_t form,
                              KeysetImage &out) {
    if (form > KS_HASH) return KS_BAD_FORM;
    const uint64_t nw = span / 64 + 1;
    const uint64_t last = (span & 63) == 63 ? ~0ull : (1ull << ((span & 63) + 1)) - 1;  // the last word's bits <= span
    uint64_t n = 0;
    for (uint64_t i = 0; i < nw; ++i) n += (uint64_t)__builtin_popcountll(i + 1 == nw ? words[i] & last : words[i]);
    if (n > kMaxKeysetKeys) return KS_TOO_MANY;
    out = KeysetImage();
    out.is_signed = is_signed;
    out.keys.reserve(n);
    for (uint64_t i = 0; i < nw; ++i)
        for (uint64_t w = i + 1 == nw ? words[i] & last : words[i]; w; w &= w - 1)
            out.keys.push_back(base + (i * 64 + (uint64_t)__builtin_ctzll(w)));
    return keyset_finish(out, form);
}

}  // namespace fls
