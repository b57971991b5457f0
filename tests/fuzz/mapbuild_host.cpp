// mapbuild_host.cpp -- host-side sanitizer run of the host half of the map
// build from a scan (csrc/fls_mapbuild.hpp: mapbuild_merge and mapbuild_codes;
// csrc/fls_valuemap.hpp / fls_keymap.hpp: valuemap_finish_sorted and
// keymap_finish_sorted), built with g++ -fsanitize=address,undefined by
// tests/test_mapbuild_host.py.  Every pair list is dealt out to one, two and
// three parts with overlapping keys, each part turned into what a GPU hands
// back (presence words over a range wider than [min, max] of the keys, and
// the present keys' values in key order), merged and finished, and the result
// held against valuemap_build / keymap_build over the same pairs: every field
// and every image word, forms 0, 1 and 2, and the same status where the
// builders refuse.
//
// usage: mapbuild_host <random maps> <seed>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "fls_mapbuild.hpp"

using namespace fls;

static int failures = 0, maps = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
            if (++failures > 20) exit(1);                 \
        }                                                 \
    } while (0)

using Pairs = std::vector<std::pair<uint64_t, uint64_t>>;

// What one GPU hands back for the pairs dealt to it (one value per key).
struct Part {
    std::vector<uint64_t> presence, values;
};

static Part make_part(const Pairs &kv, uint64_t base, uint64_t span, bool junk) {
    Part p;
    p.presence.assign((span + 64) / 64, 0);
    std::map<uint64_t, uint64_t> by_d;
    for (auto &e : kv) by_d[e.first - base] = e.second;
    for (auto &e : by_d) {
        p.presence[e.first >> 6] |= 1ull << (e.first & 63);
        p.values.push_back(e.second);
    }
    // bits past span in the last word are not keys
    if (junk && (span & 63) != 63) p.presence.back() |= ~0ull << ((span & 63) + 1);
    return p;
}

static void same_keyset(const char *what, uint32_t form, const KeysetImage &a, const KeysetImage &b) {
    CHECK(a.is_signed == b.is_signed, "%s form %u: is_signed", what, form);
    CHECK(a.keys == b.keys, "%s form %u: keys (%zu vs %zu)", what, form, a.keys.size(), b.keys.size());
    CHECK(a.min == b.min && a.max == b.max && a.span == b.span, "%s form %u: min / max / span", what, form);
    CHECK(a.cap_log2 == b.cap_log2, "%s form %u: cap_log2 %u vs %u", what, form, a.cap_log2, b.cap_log2);
    CHECK(a.empty == b.empty, "%s form %u: sentinel %" PRIx64 " vs %" PRIx64, what, form, a.empty, b.empty);
    CHECK(a.max_probe == b.max_probe, "%s form %u: max_probe %u vs %u", what, form, a.max_probe, b.max_probe);
}

// pairs (any order, duplicates allowed, one value per key) through nparts
// parts over [min - below, max + above] of the key order (the empty map:
// around 1000); every key is dealt to at least one part, some to several
static void check_map(const char *what, const Pairs &kv, bool ksg, bool vsg, uint64_t below, uint64_t above,
                      std::mt19937_64 &rng, bool as_keymap = false,
                      std::initializer_list<uint32_t> forms = {0u, 1u, 2u}) {
    ++maps;
    uint64_t lo = ~0ull, hi = 0;  // in unsigned order of keyset_ord
    for (auto &e : kv) {
        lo = std::min(lo, keyset_ord(e.first, ksg));
        hi = std::max(hi, keyset_ord(e.first, ksg));
    }
    if (kv.empty()) lo = hi = keyset_ord(1000, ksg);
    below = std::min<uint64_t>(below, lo);  // the order's ends leave no more room
    above = std::min<uint64_t>(above, ~0ull - hi);
    const uint64_t base = keyset_ord(lo - below, ksg);  // (keyset_ord is its own inverse)
    const uint64_t span = (hi + above) - (lo - below);
    std::vector<uint64_t> keys, vals;
    std::vector<uint16_t> vals16;
    for (auto &e : kv) {
        keys.push_back(e.first);
        vals.push_back(e.second);
        vals16.push_back((uint16_t)e.second);
    }
    for (size_t nparts = 1; nparts <= 3; ++nparts) {
        std::vector<Pairs> dealt(nparts);
        for (auto &e : kv) {
            const size_t g = rng() % nparts;
            dealt[g].push_back(e);
            if (rng() % 3 == 0) dealt[rng() % nparts].push_back(e);  // the same key, the same value, on a second part
        }
        std::vector<Part> store;
        for (auto &d : dealt) store.push_back(make_part(d, base, span, true));
        std::vector<MapbuildPart> parts(nparts);
        for (size_t g = 0; g < nparts; ++g) {
            parts[g].presence = store[g].presence.data();
            parts[g].values = store[g].values.data();
            parts[g].n = store[g].values.size();
        }
        std::vector<uint64_t> mk, mv;
        MapbuildConflict bad;
        const int mrc = mapbuild_merge(parts, base, span, mk, mv, bad);
        CHECK(mrc == MB_OK, "%s parts %zu: merge status %d", what, nparts, mrc);
        if (mrc != MB_OK) continue;
        for (uint32_t form : forms) {
            if (!as_keymap) {
                ValuemapImage a, b;
                const int ra = valuemap_build(keys.data(), vals.data(), keys.size(), ksg, vsg, form, a);
                const int rb = valuemap_finish_sorted(mk, mv, ksg, vsg, form, b);
                CHECK(ra == rb, "%s form %u parts %zu: status %d from pairs, %d from the parts", what, form, nparts, ra, rb);
                if (ra != VM_OK || rb != VM_OK) continue;
                CHECK(a.form == b.form, "%s form %u: form %u vs %u", what, form, a.form, b.form);
                same_keyset(what, form, a.set, b.set);
                CHECK(a.values == b.values, "%s form %u: values", what, form);
                CHECK(a.value_signed == b.value_signed && a.vmin == b.vmin && a.vmax == b.vmax, "%s form %u: vmin / vmax",
                      what, form);
                CHECK(a.words == b.words, "%s form %u: image words (%zu vs %zu)", what, form, a.words.size(), b.words.size());
            } else {
                KeymapImage a, b;
                std::vector<uint16_t> codes;
                uint64_t badv = 0;
                const int ra = keymap_build(keys.data(), vals16.data(), keys.size(), ksg, form, a);
                const int crc = mapbuild_codes(mv, vsg, codes, badv);
                if (ra == KM_BAD_VALUE) {  // 65535 among the values: refused where the builder refuses
                    CHECK(crc == MB_BAD_VALUE && badv == kKeymapAbsent, "%s: 65535 passed the code check", what);
                    std::vector<uint16_t> raw(mv.begin(), mv.end());
                    CHECK(keymap_finish_sorted(mk, raw, ksg, form, b) == KM_BAD_VALUE, "%s: 65535 passed the finish", what);
                    continue;
                }
                CHECK(crc == MB_OK, "%s form %u: code check %d", what, form, crc);
                if (crc != MB_OK) continue;
                const int rb = keymap_finish_sorted(mk, codes, ksg, form, b);
                CHECK(ra == rb, "%s form %u parts %zu: status %d from pairs, %d from the parts", what, form, nparts, ra, rb);
                if (ra != KM_OK || rb != KM_OK) continue;
                CHECK(a.form == b.form, "%s form %u: form %u vs %u", what, form, a.form, b.form);
                same_keyset(what, form, a.set, b.set);
                CHECK(a.values == b.values && a.max_code == b.max_code, "%s form %u: codes", what, form);
                CHECK(a.words == b.words, "%s form %u: image words (%zu vs %zu)", what, form, a.words.size(), b.words.size());
            }
        }
    }
}

int main(int argc, char **argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 100;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    const uint64_t smin = 1ull << 63, smax = (1ull << 63) - 1;  // the signed order's ends, as patterns
    // seeded pair lists of either kind; every third one a key map
    for (int it = 0; it < iters; ++it) {
        const bool ksg = rng() & 1, vsg = rng() & 2, km = it % 3 == 2;
        const uint64_t n = 1 + rng() % (it % 8 == 0 ? 4000 : 100);
        const uint64_t spread = 1 + rng() % (it % 3 == 0 ? 200000 : 4 * n);
        uint64_t origin = rng();
        if (it % 5 == 1) origin = (uint64_t)0 - spread / 2;  // across 0 / -1: the unsigned order wraps there
        if (it % 5 == 2) origin = smin - spread / 2;         // across the sign boundary: the signed order wraps
        std::map<uint64_t, uint64_t> m;
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t k = origin + rng() % spread;
            m.emplace(k, km ? rng() % 65535 : (it % 4 == 0 ? rng() : rng() % 1000 - 500));
        }
        // keys on both ends of their own order span nearly 2^64 values: keep one end's
        uint64_t lo = ~0ull, hi = 0;
        for (auto &e : m) {
            lo = std::min(lo, keyset_ord(e.first, ksg));
            hi = std::max(hi, keyset_ord(e.first, ksg));
        }
        const uint64_t side = keyset_ord(m.begin()->first, ksg) >> 63;
        Pairs kv;
        for (auto &e : m)
            if (hi - lo < (1ull << 62) || (keyset_ord(e.first, ksg) >> 63) == side) kv.push_back(e);
        for (size_t i = 0, dup = kv.size() / 4; i < dup; ++i) kv.push_back(kv[rng() % kv.size()]);  // listed twice
        std::shuffle(kv.begin(), kv.end(), rng);
        check_map(km ? "random key map" : "random", kv, ksg, vsg, 1 + rng() % 300, 1 + rng() % 300, rng, km);
    }
    // the type edges of keys and values, a single pair, the empty map
    check_map("unsigned low edge", {{0, ~0ull}, {1, 0}, {5, smax}, {77, smin}}, false, false, 9, 100, rng);
    check_map("unsigned high edge", {{~0ull, 1}, {~0ull - 1, ~0ull - 1}, {~0ull - 63, 2}, {~0ull - 64, 3}, {~0ull - 200, 0}},
              false, false, 100, 9, rng);
    check_map("signed low edge", {{smin, smin}, {smin + 1, smax - 1}, {smin + 64, ~0ull}, {smin + 1000, 0}}, true, true, 9, 65,
              rng);
    check_map("signed high edge", {{smax, smin}, {smax - 1, smax - 1}, {smax - 63, 7}, {smax - 129, ~0ull}}, true, true, 65, 9,
              rng);
    check_map("signed around -1 and 0", {{~0ull, 5}, {0, 6}, {1, ~0ull}, {~0ull - 7, 0}, {31, 1}, {32, 2}}, true, true, 3, 3,
              rng);
    for (bool sg : {true, false}) {
        check_map("single pair", {{12345, 678}}, sg, sg, 1, 1, rng);
        check_map("single pair, wide range", {{(uint64_t)0 - 40000, (uint64_t)0 - 3}}, sg, sg, 100000, 20000, rng);
        check_map("single pair at bit 63 of a word", {{63, 1}}, false, sg, 0, 1, rng);
        check_map("empty", {}, sg, sg, 1, 1, rng);
        check_map("empty, wide range", {}, sg, !sg, 500, 70000, rng);
        check_map("single code", {{12345, 65534}}, sg, false, 1, 1, rng, true);
        check_map("empty key map", {}, sg, true, 1, 70, rng, true);
        check_map("codes 0 and 65534", {{5, 0}, {9, 65534}, {100, 3}}, sg, true, 10, 10, rng, true);
    }
    // either side of both conditions of the value map's auto rule
    for (uint64_t past : {0ull, 1ull}) {
        // 3 keys: a 128-byte hash image; the widest dense form of at most 1 MiB, and one key more
        uint64_t span = 0;
        while (valuemap_dense_bytes(span + 1) <= kValuemapSmallDense) ++span;  // the last span at or below 1 MiB
        check_map("auto: 1 MiB", {{10, 1}, {11, 2}, {10 + span + past, 3}}, true, true, 100, 100, rng);
        // 2^17 + 1 keys: an 8 MiB hash image; the widest dense form no larger than it, and one key more
        Pairs kv;
        for (uint64_t i = 0; i < (1ull << 17); ++i) kv.push_back({(uint64_t)0 - 1000 + i, i * 3});
        uint64_t s2 = 1ull << 17;
        while (valuemap_dense_bytes(s2 + 1) <= valuemap_hash_bytes(keyset_cap_log2(kv.size() + 1))) ++s2;
        kv.push_back({(uint64_t)0 - 1000 + s2 + past, 9});
        check_map("auto: the hash image's size", kv, true, false, 100, 100, rng);
    }
    {   // ... and what the rule gives there (the comparison above only says both agree)
        uint64_t span = 0;
        while (valuemap_dense_bytes(span + 1) <= kValuemapSmallDense) ++span;
        for (uint64_t past : {0ull, 1ull}) {
            ValuemapImage img;
            CHECK(valuemap_finish_sorted({10, 11, 10 + span + past}, {1, 2, 3}, true, true, VM_AUTO, img) == VM_OK, "auto rule");
            CHECK(img.form == (past ? VM_HASH : VM_DENSE), "auto rule: form %u", img.form);
        }
    }
    // either side of the key map's small-dense condition
    for (uint64_t past : {0ull, 1ull})
        check_map("key map auto: 1 MiB", {{10, 1}, {11, 2}, {10 + (1ull << 19) - 1 + past, 3}}, false, false, 100, 100, rng, true);
    {   // VM_TOO_WIDE where the builder gives it: a forced dense form over 2^28 + 1 keys (the parts: hash and auto only)
        const Pairs kv = {{7, 1}, {8, 2}, {7 + kValuemapMaxSpan, 3}};
        ValuemapImage img;
        CHECK(valuemap_finish_sorted({7, 8, 7 + kValuemapMaxSpan}, {1, 2, 3}, false, false, VM_DENSE, img) == VM_TOO_WIDE,
              "a dense map over 2^28 + 1 keys accepted");
        check_map("span 2^28", kv, false, false, 3, 3, rng);
        const Pairs fits = {{7, 1}, {8, 2}, {7 + kValuemapMaxSpan - 1, 3}};
        check_map("span 2^28 - 1", fits, false, false, 3, 3, rng, false, {VM_AUTO, VM_HASH});
    }
    {   // KM_BAD_VALUE where the builder gives it, and the values the device route's range check names
        ++maps;
        check_map("code 65535", {{5, 1}, {9, 65535}, {11, 2}}, true, true, 5, 5, rng, true);
        std::vector<uint16_t> codes;
        uint64_t bad = 0;
        CHECK(mapbuild_codes({3, (uint64_t)-1, (uint64_t)-7, 70000}, true, codes, bad) == MB_BAD_VALUE && bad == (uint64_t)-7,
              "signed: the minimum when negative");
        CHECK(mapbuild_codes({3, 65535, 70000, 2}, true, codes, bad) == MB_BAD_VALUE && bad == 70000, "signed: the maximum");
        CHECK(mapbuild_codes({3, (uint64_t)-1, 70000}, false, codes, bad) == MB_BAD_VALUE && bad == (uint64_t)-1,
              "unsigned: the maximum");
        CHECK(mapbuild_codes({0, 65534}, true, codes, bad) == MB_OK && codes == std::vector<uint16_t>({0, 65534}), "0 and 65534");
        CHECK(mapbuild_codes({}, true, codes, bad) == MB_OK && codes.empty(), "no value");
    }
    {   // the cross-part conflict: one key on two parts with two values, where valuemap_build gives VM_CONFLICT
        ++maps;
        const uint64_t base = 100, span = 300;
        const Pairs a = {{101, 5}, {250, 7}, {400, 1}}, b = {{101, 5}, {250, 8}, {399, 2}}, c = {{100, 0}};
        const Part pa = make_part(a, base, span, true), pb = make_part(b, base, span, false),
                   pc = make_part(c, base, span, true);
        std::vector<uint64_t> mk, mv;
        MapbuildConflict bad;
        for (int order = 0; order < 2; ++order) {
            std::vector<MapbuildPart> parts = {{pc.presence.data(), pc.values.data(), pc.values.size()},
                                               {(order ? pb : pa).presence.data(), (order ? pb : pa).values.data(), 3},
                                               {(order ? pa : pb).presence.data(), (order ? pa : pb).values.data(), 3}};
            CHECK(mapbuild_merge(parts, base, span, mk, mv, bad) == MB_CONFLICT, "a cross-part conflict passed");
            CHECK(bad.key == 250 && bad.a + bad.b == 15, "conflict: key %" PRIu64 " values %" PRIu64 ", %" PRIu64, bad.key,
                  bad.a, bad.b);
        }
        const uint64_t k[6] = {101, 250, 400, 101, 250, 399}, v[6] = {5, 7, 1, 5, 8, 2};
        ValuemapImage img;
        CHECK(valuemap_build(k, v, 6, false, false, VM_AUTO, img) == VM_CONFLICT && img.bad_key == 250, "the builder's conflict");
        // without the conflicting part the rest merges: 100, 101, 250, 400
        std::vector<MapbuildPart> ok = {{pc.presence.data(), pc.values.data(), 1}, {pa.presence.data(), pa.values.data(), 3}};
        CHECK(mapbuild_merge(ok, base, span, mk, mv, bad) == MB_OK && mk == std::vector<uint64_t>({100, 101, 250, 400}) &&
                  mv == std::vector<uint64_t>({0, 5, 7, 1}), "merge of two parts");
        // a part with fewer values than its presence words name is refused, nothing past them is read
        std::vector<MapbuildPart> shortp = {{pa.presence.data(), pa.values.data(), 2}};
        CHECK(mapbuild_merge(shortp, base, span, mk, mv, bad) == MB_SHORT, "a short part passed");
    }
    {   // the gate's size rule, either side of each condition
        ++maps;
        CHECK(mapbuild_span_ok(kValuemapMaxSpan - 1, 1ull << 28) && !mapbuild_span_ok(kValuemapMaxSpan, 1ull << 28), "span gate");
        CHECK(mapbuild_span_ok((1ull << 17) - 1, 1) && !mapbuild_span_ok(1ull << 17, 1), "1 MiB gate");
        // 2^16 rows: a 2 MiB hash image (capacity 2^17)
        CHECK(mapbuild_span_ok((1ull << 18) - 1, 1ull << 16) && !mapbuild_span_ok(1ull << 18, 1ull << 16), "hash image gate");
    }
    printf("maps %d failures %d\n", maps, failures);
    return failures ? 1 : 0;
}
