// fls_mapbuild.hpp -- the host half of a map built on the GPU from a filtered
// scan (fls_valuemap_from_scan / fls_keymap_from_scan, fls_scan_mapbuild.hip;
// the kernels: fls_mapbuild.hip).
//
// Host only (no HIP include): a stand-alone CPU program can drive this header
// (tests/fuzz/mapbuild_host.cpp).  Each GPU of the call hands back one part:
// the presence words of its collecting array over [base, base + span] (bit d
// of word d >> 6 stands for the key base + d, mod 2^64; bits past span are
// ignored) and the values of the present keys in ascending d, as stored
// patterns.  mapbuild_merge walks the parts' words side by side, as
// keyset_from_bitmap walks one bitmap, and yields the map's distinct keys in
// the key order with their values: what valuemap_finish_sorted takes, and,
// after mapbuild_codes, keymap_finish_sorted.  A key two parts hold with one
// value is kept once; with two values the map is no function.
#pragma once
#include <cstdint>
#include <vector>

#include "fls_keymap.hpp"
#include "fls_valuemap.hpp"

namespace fls {

enum MapbuildStatus : int { MB_OK = 0, MB_CONFLICT = 1, MB_SHORT = 2, MB_BAD_VALUE = 3 };

struct MapbuildPart {
    const uint64_t *presence = nullptr;  // (span + 64) / 64 words
    const uint64_t *values = nullptr;    // one per set bit <= span, in ascending d
    uint64_t n = 0;                      // how many values
};

// what a refused merge reports: the offending key and its two values
struct MapbuildConflict {
    uint64_t key = 0, a = 0, b = 0;
};

// base is the smallest value of the collecting range in the key order, so
// ascending d is that order (the caller keeps base + span from wrapping past
// the order's end).  MB_SHORT: a part's presence words name more keys than it
// has values (a damaged part; nothing past a part's n values is read).
inline int mapbuild_merge(const std::vector<MapbuildPart> &parts, uint64_t base, uint64_t span,
                          std::vector<uint64_t> &keys, std::vector<uint64_t> &values, MapbuildConflict &bad) {
    const uint64_t nw = (span + 64) / 64;
    const uint64_t last = (span & 63) == 63 ? ~0ull : (1ull << ((span & 63) + 1)) - 1;  // the last word's bits <= span
    keys.clear();
    values.clear();
    uint64_t most = 0;
    for (const MapbuildPart &p : parts) most = std::max(most, p.n);
    keys.reserve(most);
    values.reserve(most);
    std::vector<uint64_t> cur(parts.size(), 0);  // per part: the next value
    for (uint64_t i = 0; i < nw; ++i) {
        uint64_t any = 0;
        for (const MapbuildPart &p : parts) any |= p.presence[i];
        if (i + 1 == nw) any &= last;
        for (uint64_t w = any; w; w &= w - 1) {
            const uint64_t bit = w & (~w + 1);
            const uint64_t key = base + (i * 64 + (uint64_t)__builtin_ctzll(w));
            bool have = false;
            uint64_t v = 0;
            for (size_t g = 0; g < parts.size(); ++g) {
                if (!(parts[g].presence[i] & bit)) continue;
                if (cur[g] >= parts[g].n) return MB_SHORT;
                const uint64_t x = parts[g].values[cur[g]++];
                if (have && x != v) {  // one key, two values on two GPUs: no function
                    bad.key = key;
                    bad.a = v;
                    bad.b = x;
                    return MB_CONFLICT;
                }
                have = true;
                v = x;
            }
            keys.push_back(key);
            values.push_back(v);
        }
    }
    return MB_OK;
}

// A key map's codes out of merged values: every value must lie in [0, 65534]
// in the value order.  MB_BAD_VALUE names in `bad` the value a host build
// names: the smallest if it is negative, otherwise the largest.
inline int mapbuild_codes(const std::vector<uint64_t> &values, bool value_signed, std::vector<uint16_t> &codes,
                          uint64_t &bad) {
    uint64_t lo = 0, hi = 0;
    for (size_t i = 0; i < values.size(); ++i) {
        const uint64_t v = values[i];
        if (i == 0 || keyset_ord(v, value_signed) < keyset_ord(lo, value_signed)) lo = v;
        if (i == 0 || keyset_ord(v, value_signed) > keyset_ord(hi, value_signed)) hi = v;
    }
    if (!values.empty() && value_signed && (int64_t)lo < 0) {
        bad = lo;
        return MB_BAD_VALUE;
    }
    if (!values.empty() && hi >= kKeymapAbsent) {  // (lo >= 0: the patterns compare as unsigned)
        bad = hi;
        return MB_BAD_VALUE;
    }
    codes.resize(values.size());
    for (size_t i = 0; i < values.size(); ++i) codes[i] = (uint16_t)values[i];
    return MB_OK;
}

// The gate's size rule (the auto rule's own comparison of the dense form
// against the hash form): may a call collect over span + 1 values when the
// surviving row groups hold `rows` rows?
inline uint64_t mapbuild_scratch_bytes(uint64_t span) { return 8 * (span + 1); }
inline bool mapbuild_span_ok(uint64_t span, uint64_t rows) {
    if (span >= kValuemapMaxSpan) return false;
    const uint64_t sb = mapbuild_scratch_bytes(span);
    return !(sb > kValuemapSmallDense && sb > valuemap_hash_bytes(keyset_cap_log2(rows)));
}

}  // namespace fls
