// keyset_bitmap_host.cpp -- host-side sanitizer run of the second half of the
// key-set build from a scan (csrc/fls_keyset.hpp: keyset_from_bitmap and
// keyset_finish), built with g++ -fsanitize=address,undefined by
// tests/test_keyset_build_host.py.  For every set a collecting bitmap is made
// over a range wider than [min, max] of the keys (on both sides where the
// order's ends leave room) and keyset_from_bitmap is held against
// keyset_build over the same keys: every field and every word, forms 0, 1
// and 2, and the same status where keyset_build refuses.
//
// usage: keyset_bitmap_host <random sets> <seed>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "fls_keyset.hpp"

using namespace fls;

static int failures = 0, sets = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
            if (++failures > 20) exit(1);                 \
        }                                                 \
    } while (0)

// keys (any order, duplicates allowed) through a bitmap over
// [min - below, max + above] of the set's order (the empty set: around 1000)
static void check_set(const char *what, const std::vector<uint64_t> &keys, bool sg, uint64_t below, uint64_t above,
                      std::initializer_list<uint32_t> forms = {KS_AUTO, KS_BITMAP, KS_HASH}) {
    ++sets;
    uint64_t lo = ~0ull, hi = 0;  // in unsigned order of keyset_ord
    for (uint64_t k : keys) {
        lo = std::min(lo, keyset_ord(k, sg));
        hi = std::max(hi, keyset_ord(k, sg));
    }
    if (keys.empty()) lo = hi = keyset_ord(1000, sg);
    below = std::min<uint64_t>(below, lo);          // the order's ends leave no more room
    above = std::min<uint64_t>(above, ~0ull - hi);
    const uint64_t base = keyset_ord(lo - below, sg);  // (keyset_ord is its own inverse)
    const uint64_t span = (hi + above) - (lo - below);
    std::vector<uint64_t> words(span / 64 + 1, 0);
    for (uint64_t k : keys) {
        const uint64_t d = k - base;
        CHECK(d <= span, "%s: test bug, key outside the collecting range", what);
        words[d >> 6] |= 1ull << (d & 63);
    }
    // bits past span in the last word are not keys
    if ((span & 63) != 63) words.back() |= ~0ull << ((span & 63) + 1);
    for (uint32_t form : forms) {
        KeysetImage a, b;
        const int ra = keyset_build(keys.data(), keys.size(), sg, form, a);
        const int rb = keyset_from_bitmap(words.data(), base, span, sg, form, b);
        CHECK(ra == rb, "%s form %u: status %d from keys, %d from the bitmap", what, form, ra, rb);
        if (ra != KS_OK || rb != KS_OK) continue;
        CHECK(a.form == b.form, "%s form %u: form %u vs %u", what, form, a.form, b.form);
        CHECK(a.is_signed == b.is_signed, "%s form %u: is_signed", what, form);
        CHECK(a.keys == b.keys, "%s form %u: keys (%zu vs %zu)", what, form, a.keys.size(), b.keys.size());
        CHECK(a.min == b.min && a.max == b.max && a.span == b.span, "%s form %u: min / max / span", what, form);
        CHECK(a.cap_log2 == b.cap_log2, "%s form %u: cap_log2 %u vs %u", what, form, a.cap_log2, b.cap_log2);
        CHECK(a.empty == b.empty, "%s form %u: sentinel %" PRIx64 " vs %" PRIx64, what, form, a.empty, b.empty);
        CHECK(a.max_probe == b.max_probe, "%s form %u: max_probe %u vs %u", what, form, a.max_probe, b.max_probe);
        CHECK(a.words == b.words, "%s form %u: image words (%zu vs %zu)", what, form, a.words.size(), b.words.size());
    }
}

int main(int argc, char **argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 100;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    const uint64_t smin = 1ull << 63, smax = (1ull << 63) - 1;  // the signed order's ends, as patterns
    // seeded sets of either kind
    for (int it = 0; it < iters; ++it) {
        const bool sg = rng() & 1;
        const uint64_t n = 1 + rng() % (it % 8 == 0 ? 4000 : 100);
        const uint64_t spread = 1 + rng() % (it % 3 == 0 ? 200000 : 4 * n);
        std::vector<uint64_t> keys;
        uint64_t origin = rng();
        if (it % 5 == 1) origin = (uint64_t)0 - spread / 2;              // across 0 / -1: the unsigned order wraps there
        if (it % 5 == 2) origin = smin - spread / 2;                     // across the sign boundary: the signed order wraps
        for (uint64_t i = 0; i < n; ++i) keys.push_back(origin + rng() % spread);
        // keys on both ends of their own order span nearly 2^64 values: keep one end's
        uint64_t lo = ~0ull, hi = 0;
        for (uint64_t k : keys) {
            lo = std::min(lo, keyset_ord(k, sg));
            hi = std::max(hi, keyset_ord(k, sg));
        }
        std::vector<uint64_t> side;
        for (uint64_t k : keys)
            if (hi - lo < (1ull << 62) || (keyset_ord(k, sg) >> 63) == (keyset_ord(keys[0], sg) >> 63)) side.push_back(k);
        check_set("random", side, sg, 1 + rng() % 300, 1 + rng() % 300);
    }
    // the type edges, a single key, the empty set
    check_set("unsigned low edge", {0, 1, 5, 77}, false, 9, 100);
    check_set("unsigned high edge", {~0ull, ~0ull - 1, ~0ull - 63, ~0ull - 64, ~0ull - 200}, false, 100, 9);
    check_set("signed low edge", {smin, smin + 1, smin + 64, smin + 1000}, true, 9, 65);
    check_set("signed high edge", {smax, smax - 1, smax - 63, smax - 129}, true, 65, 9);
    check_set("signed around -1 and 0", {~0ull, 0, 1, ~0ull - 7, 31, 32}, true, 3, 3);
    check_set("unsigned high edge, every sentinel taken", {~0ull, ~0ull - 1, ~0ull - 2, ~0ull - 3, ~0ull - 5}, false, 70, 0);
    for (bool sg : {true, false}) {
        check_set("single key", {12345}, sg, 1, 1);
        check_set("single key, wide range", {(uint64_t)0 - 40000}, sg, 100000, 20000);
        check_set("single key at bit 63 of a word", {63}, false, 0, 1);
        check_set("empty", {}, sg, 1, 1);
        check_set("empty, wide range", {}, sg, 500, 70000);
    }
    // keys sharing one home slot of the table they end up in, as
    // test_keyset.colliding_keys makes them, here searched upwards from a base
    // so that they fit one range: forced hash, max_probe = the set size
    for (uint64_t home : {5ull, 127ull}) {
        std::vector<uint64_t> keys;
        for (uint64_t k = 1000000; keys.size() < 50; ++k)
            if (keyset_home(k, 7) == home) keys.push_back(k);
        KeysetImage img;
        CHECK(keyset_build(keys.data(), keys.size(), false, KS_HASH, img) == KS_OK && img.max_probe == 50,
              "colliding keys: max_probe %u", img.max_probe);
        check_set("colliding homes", keys, false, 17, 4000);
    }
    // either side of both conditions of the auto rule
    for (uint64_t past : {0ull, 1ull}) {
        // 3 keys: a 64-byte table; the bitmap of span 2^23 - 1 is exactly 1 MiB
        check_set("auto: 1 MiB", {10, 11, 10 + (1ull << 23) - 1 + past}, true, 100, 100);
        // 2^17 + 1 keys: a 4 MiB table; the bitmap of span 2^25 - 1 is exactly 4 MiB
        std::vector<uint64_t> keys;
        for (uint64_t i = 0; i < (1ull << 17); ++i) keys.push_back((uint64_t)0 - 1000 + i);
        keys.push_back((uint64_t)0 - 1000 + (1ull << 25) - 1 + past);
        check_set("auto: the table's size", keys, true, 100, 100);
    }
    {   // ... and what the rule gives there (the comparison above only says both agree)
        KeysetImage img;
        const uint64_t at[3] = {10, 11, 10 + (1ull << 23) - 1}, over[3] = {10, 11, 10 + (1ull << 23)};
        std::vector<uint64_t> w((1ull << 23) / 64 + 2, 0);
        for (const uint64_t *k : {at, over}) {
            std::fill(w.begin(), w.end(), 0);
            for (int i = 0; i < 3; ++i) w[(k[i] - 5) >> 6] |= 1ull << ((k[i] - 5) & 63);
            CHECK(keyset_from_bitmap(w.data(), 5, (1ull << 23) + 20, true, KS_AUTO, img) == KS_OK, "auto rule");
            CHECK(img.form == (k == at ? KS_BITMAP : KS_HASH), "auto rule: form %u", img.form);
        }
    }
    // spans at the bitmap's limit: 2^32 - 1 fits (auto: the hash table, with
    // these few keys; forced: a 512 MiB bitmap, built once), 2^32 is
    // KS_TOO_WIDE from both when the bitmap is forced
    check_set("span 2^32 - 1", {7, 8, 7 + kKeysetMaxSpan - 1}, false, 3, 3);
    check_set("span 2^32 - 1, signed", {smin + 7, smin + 9, smin + 7 + kKeysetMaxSpan - 1}, true, 3, 3, {KS_AUTO, KS_HASH});
    for (bool sg : {true, false}) {
        const std::vector<uint64_t> keys = {(uint64_t)0 - 5 * sg, (uint64_t)0 - 5 * sg + 3, (uint64_t)0 - 5 * sg + kKeysetMaxSpan};
        KeysetImage img;
        CHECK(keyset_build(keys.data(), keys.size(), sg, KS_BITMAP, img) == KS_TOO_WIDE, "span 2^32 accepted");
        check_set("span 2^32", keys, sg, 3, 3);
    }
    {   // one key more than a set may hold: refused from the count, before a key is stored
        ++sets;
        const uint64_t n = kMaxKeysetKeys + 1;
        std::vector<uint64_t> w(n / 64 + 1, ~0ull);
        KeysetImage img;
        CHECK(keyset_build(nullptr, n, true, KS_AUTO, img) == KS_TOO_MANY, "n above kMaxKeysetKeys accepted");
        CHECK(keyset_from_bitmap(w.data(), 0, n - 1, false, KS_AUTO, img) == KS_TOO_MANY, "2^28 + 1 bits accepted");
        CHECK(keyset_from_bitmap(w.data(), 0, n - 1, false, 3, img) == KS_BAD_FORM, "form 3 accepted");
    }
    printf("sets %d failures %d\n", sets, failures);
    return failures ? 1 : 0;
}
