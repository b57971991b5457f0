// fuzz_keyset.cpp -- host-side sanitizer run of the key-set construction
// (csrc/fls_keyset.hpp), built with g++ -fsanitize=address,undefined by
// tests/test_keyset.py.  Seeded random and adversarial sets in every form;
// keyset_contains (the probe of the uploaded image) is checked against
// std::set for the keys, their neighbours, the sentinel candidates and random
// probes, and keyset_any_in_range against a scan of the set.
//
// usage: fuzz_keyset <iterations> <seed>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "fls_keyset.hpp"

using namespace fls;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
            if (++failures > 20) exit(1);                 \
        }                                                 \
    } while (0)

static void check_set(const std::vector<uint64_t> &keys, bool sg, uint32_t form, std::mt19937_64 &rng) {
    KeysetImage img;
    const int rc = keyset_build(keys.data(), keys.size(), sg, form, img);
    std::set<uint64_t> ref(keys.begin(), keys.end());
    if (rc == KS_TOO_WIDE) {
        uint64_t lo = ~0ull, hi = 0;
        for (uint64_t k : ref) {
            lo = std::min(lo, keyset_ord(k, sg));
            hi = std::max(hi, keyset_ord(k, sg));
        }
        CHECK(form == KS_BITMAP && hi - lo >= kKeysetMaxSpan, "TOO_WIDE for span %" PRIu64, hi - lo);
        return;
    }
    CHECK(rc == KS_OK, "build rc %d", rc);
    CHECK(img.keys.size() == ref.size(), "distinct %zu vs %zu", img.keys.size(), ref.size());
    CHECK(form == KS_AUTO || img.form == form, "form %u forced, %u built", form, img.form);
    for (size_t i = 1; i < img.keys.size(); ++i)
        CHECK(keyset_ord(img.keys[i - 1], sg) < keyset_ord(img.keys[i], sg), "keys not ascending at %zu", i);
    if (img.form == KS_HASH) {
        CHECK(img.words.size() == (1ull << img.cap_log2) && img.words.size() >= 2 * ref.size(), "capacity");
        CHECK(!ref.count(img.empty), "sentinel %" PRIx64 " is a key", img.empty);
        for (uint64_t e = ~0ull; e > img.empty; --e) CHECK(ref.count(e), "sentinel skipped a free value");
        size_t used = 0;
        for (uint64_t w : img.words) used += w != img.empty;
        CHECK(used == ref.size(), "occupied slots %zu vs %zu", used, ref.size());
    } else {
        CHECK(img.span < kKeysetMaxSpan && img.words.size() == img.span / 64 + 1, "bitmap size");
    }
    auto probe = [&](uint64_t k) {
        CHECK(keyset_contains(img, k) == (ref.count(k) != 0), "contains(%" PRIx64 ") form %u n %zu", k, img.form,
              ref.size());
        CHECK(keyset_has_key(img, k) == (ref.count(k) != 0), "has_key(%" PRIx64 ")", k);
    };
    for (uint64_t k : ref) {
        probe(k);
        probe(k + 1);
        probe(k - 1);
        probe(k ^ (1ull << 63));
    }
    const std::vector<uint64_t> edges = {0, 1, ~0ull, ~0ull - 1, ~0ull - 2, 1ull << 63, (1ull << 63) - 1, img.empty,
                                         img.min - 1, img.max + 1, img.min + kKeysetMaxSpan,
                                         img.min - kKeysetMaxSpan};
    for (uint64_t k : edges) probe(k);
    for (int i = 0; i < 256; ++i) probe(rng());
    // pruning: a key in [lo, hi] of the set's order
    for (int i = 0; i < 32; ++i) {
        uint64_t a = i & 1 ? rng() : (ref.empty() ? rng() : *ref.begin() + (rng() % 64) - 32);
        uint64_t b = a + (rng() % 4096);
        if (keyset_ord(a, sg) > keyset_ord(b, sg)) std::swap(a, b);
        bool any = false;
        for (uint64_t k : ref) any = any || (keyset_ord(k, sg) >= keyset_ord(a, sg) && keyset_ord(k, sg) <= keyset_ord(b, sg));
        CHECK(keyset_any_in_range(img, a, b) == any, "any_in_range");
    }
}

int main(int argc, char **argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 200;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    for (int it = 0; it < iters; ++it) {
        std::vector<uint64_t> keys;
        const uint64_t n = rng() % (it % 8 == 0 ? 5000 : 64);
        const bool sg = rng() & 1;
        switch (it % 7) {
        case 0:  // dense around a random base (bitmap territory), with duplicates
        {
            const uint64_t base = rng();
            for (uint64_t i = 0; i < n; ++i) keys.push_back(base + rng() % (2 * n + 1));
            break;
        }
        case 1:  // sparse 64-bit keys
            for (uint64_t i = 0; i < n; ++i) keys.push_back(rng());
            break;
        case 2:  // the top of the range: every sentinel candidate taken
            for (uint64_t i = 0; i < n; ++i) keys.push_back(~0ull - i);
            keys.push_back(0);
            break;
        case 3:  // around the sign boundary
            for (uint64_t i = 0; i < n; ++i) keys.push_back((1ull << 63) - n / 2 + i);
            break;
        case 4: {  // keys sharing one home slot of the table they end up in (wraps when the slot is the last)
            const uint32_t l = keyset_cap_log2(n);
            const uint64_t home = it % 2 ? (1ull << l) - 1 : rng() & ((1ull << l) - 1);
            for (uint64_t k = rng(); keys.size() < n; ++k)
                if (keyset_home(k, l) == home) keys.push_back(k);
            break;
        }
        case 5:  // two clusters 2^32 - 1, 2^32 or 2^32 + 1 apart (the bitmap limit)
            keys.push_back(rng());
            keys.push_back(keys[0] + kKeysetMaxSpan - 1 + (rng() % 3) - (n & 1));
            for (uint64_t i = 0; i < n; ++i) keys.push_back(keys[0] + i);
            if (keyset_ord(keys[0], sg) > keyset_ord(keys[1], sg)) keys.clear();  // wrapped: not a span test
            break;
        default:  // tiny sets, the empty set included
            for (uint64_t i = 0; i < n % 3; ++i) keys.push_back(rng() % 4 ? rng() : ~0ull);
            break;
        }
        for (uint32_t form : {KS_AUTO, KS_BITMAP, KS_HASH}) {
            // no forced bitmap of hundreds of MiB: at the 2^32 limit the spans that fit are built as auto
            // (the hash table, with these few keys) and hash only, the ones past it are KS_TOO_WIDE
            if (form == KS_BITMAP && !keys.empty()) {
                uint64_t lo = ~0ull, hi = 0;
                for (uint64_t k : keys) {
                    lo = std::min(lo, keyset_ord(k, sg));
                    hi = std::max(hi, keyset_ord(k, sg));
                }
                if (hi - lo < kKeysetMaxSpan && keyset_bitmap_bytes(hi - lo) > (64ull << 20)) continue;
            }
            check_set(keys, sg, form, rng);
        }
    }
    // the widest bitmap a set may ask for: 2^32 values, 512 MiB (sized here, never allocated)
    if (keyset_bitmap_bytes(kKeysetMaxSpan - 1) != (1ull << 29) || keyset_bitmap_bytes(0) != 8) {
        fprintf(stderr, "FAIL: keyset_bitmap_bytes at its ends\n");
        ++failures;
    }
    // the documented limit is checked before keys is read
    KeysetImage img;
    if (keyset_build(nullptr, kMaxKeysetKeys + 1, true, KS_AUTO, img) != KS_TOO_MANY) {
        fprintf(stderr, "FAIL: n above kMaxKeysetKeys accepted\n");
        ++failures;
    }
    printf("iterations %d failures %d\n", iters, failures);
    return failures ? 1 : 0;
}
