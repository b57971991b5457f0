// fuzz_keymap.cpp -- host-side sanitizer run of the key-map construction
// (csrc/fls_keymap.hpp), built with g++ -fsanitize=address,undefined by
// tests/test_keymap.py.  Seeded random and adversarial maps in every form;
// keymap_lookup (the probe of the uploaded image) is checked against std::map
// for the keys, their neighbours, the sentinel candidates and random probes,
// the image against a rebuild from shuffled input, and the refusals (a
// conflicting duplicate, the reserved code, the limits) against their rules.
//
// usage: fuzz_keymap <iterations> <seed>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "fls_keymap.hpp"

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

static void span_of(const std::vector<uint64_t> &keys, bool sg, uint64_t &lo, uint64_t &hi) {
    lo = ~0ull;
    hi = 0;
    for (uint64_t k : keys) {
        lo = std::min(lo, keyset_ord(k, sg));
        hi = std::max(hi, keyset_ord(k, sg));
    }
}

static void check_map(const std::vector<uint64_t> &keys, const std::vector<uint16_t> &vals, bool sg, uint32_t form,
                      std::mt19937_64 &rng) {
    KeymapImage img;
    const int rc = keymap_build(keys.data(), vals.data(), keys.size(), sg, form, img);
    std::map<uint64_t, uint16_t> ref;
    for (size_t i = 0; i < keys.size(); ++i) ref[keys[i]] = vals[i];  // (the callers give a key one value)
    if (rc == KM_TOO_WIDE) {
        uint64_t lo, hi;
        span_of(keys, sg, lo, hi);
        CHECK(form == KM_DENSE && hi - lo >= kKeymapMaxSpan, "TOO_WIDE for span %" PRIu64, hi - lo);
        return;
    }
    CHECK(rc == KM_OK, "build rc %d", rc);
    const KeysetImage &s = img.set;
    CHECK(s.keys.size() == ref.size() && img.values.size() == ref.size(), "distinct %zu vs %zu", s.keys.size(), ref.size());
    CHECK(form == KM_AUTO || img.form == form, "form %u forced, %u built", form, img.form);
    for (size_t i = 1; i < s.keys.size(); ++i)
        CHECK(keyset_ord(s.keys[i - 1], sg) < keyset_ord(s.keys[i], sg), "keys not ascending at %zu", i);
    uint16_t mc = 0;
    for (auto &kv : ref) mc = std::max(mc, kv.second);
    CHECK(img.max_code == mc, "max_code %u vs %u", img.max_code, mc);
    if (img.form == KM_HASH) {
        const uint64_t cap = 1ull << s.cap_log2;
        CHECK(cap >= 2 * ref.size() && img.bytes() == keymap_hash_bytes(s.cap_log2) && img.bytes() % 8 == 0 &&
                  img.bytes() >= 10 * cap, "hash image size");
        CHECK(!ref.count(s.empty), "sentinel %" PRIx64 " is a key", s.empty);
        size_t used = 0;
        for (uint64_t i = 0; i < cap; ++i) {
            const bool occ = img.words[i] != s.empty;
            used += occ;
            CHECK((img.hash_values()[i] != kKeymapAbsent) == occ, "value of slot %" PRIu64, i);
        }
        CHECK(used == ref.size(), "occupied slots %zu vs %zu", used, ref.size());
    } else {
        CHECK(s.span < kKeymapMaxSpan && img.bytes() == keymap_dense_bytes(s.span) && img.bytes() % 8 == 0 &&
                  img.bytes() >= 2 * (s.span + 1), "dense image size");
        for (uint64_t d = s.span + 1; d < img.bytes() / 2; ++d) CHECK(img.dense()[d] == kKeymapAbsent, "padding");
    }
    auto probe = [&](uint64_t k) {
        auto it = ref.find(k);
        const uint16_t want = it == ref.end() ? kKeymapAbsent : it->second;
        CHECK(keymap_lookup(img, k) == want, "lookup(%" PRIx64 ") = %u, want %u, form %u n %zu", k, keymap_lookup(img, k),
              want, img.form, ref.size());
    };
    for (auto &kv : ref) {
        probe(kv.first);
        probe(kv.first + 1);
        probe(kv.first - 1);
        probe(kv.first ^ (1ull << 63));
    }
    const std::vector<uint64_t> edges = {0, 1, ~0ull, ~0ull - 1, ~0ull - 2, 1ull << 63, (1ull << 63) - 1, s.empty,
                                         s.min - 1, s.max + 1, s.min + kKeymapMaxSpan, s.min - kKeymapMaxSpan};
    for (uint64_t k : edges) probe(k);
    for (int i = 0; i < 256; ++i) probe(rng());
    // the image is a function of the map: shuffled input with every pair doubled
    std::vector<size_t> order(keys.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::shuffle(order.begin(), order.end(), rng);
    std::vector<uint64_t> k2;
    std::vector<uint16_t> v2;
    for (size_t i : order) {
        k2.push_back(keys[i]);
        v2.push_back(vals[i]);
    }
    k2.insert(k2.end(), keys.begin(), keys.end());
    v2.insert(v2.end(), vals.begin(), vals.end());
    KeymapImage again;
    CHECK(keymap_build(k2.data(), v2.data(), k2.size(), sg, form, again) == KM_OK, "rebuild");
    CHECK(again.form == img.form && again.words == img.words && again.set.keys == s.keys && again.values == img.values &&
              again.set.max_probe == s.max_probe && again.set.empty == s.empty, "image depends on the input order");
    // a conflicting value for one key is refused and named
    if (!keys.empty()) {
        const size_t j = rng() % keys.size();
        k2.push_back(keys[j]);
        v2.push_back((uint16_t)((vals[j] + 1) % 65535));
        KeymapImage bad;
        CHECK(keymap_build(k2.data(), v2.data(), k2.size(), sg, form, bad) == KM_CONFLICT && bad.bad_key == keys[j] &&
                  std::min(bad.bad_a, bad.bad_b) == std::min<uint32_t>(vals[j], v2.back()) &&
                  std::max(bad.bad_a, bad.bad_b) == std::max<uint32_t>(vals[j], v2.back()), "conflict not refused");
        v2.back() = kKeymapAbsent;
        CHECK(keymap_build(k2.data(), v2.data(), k2.size(), sg, form, bad) == KM_BAD_VALUE && bad.bad_key == keys[j],
              "the reserved code accepted");
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
        case 0:  // dense around a random base, with duplicates
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
        case 5:  // two clusters 2^31 - 1, 2^31 or 2^31 + 1 apart (the dense limit)
            keys.push_back(rng());
            keys.push_back(keys[0] + kKeymapMaxSpan - 1 + (rng() % 3) - (n & 1));
            for (uint64_t i = 0; i < n; ++i) keys.push_back(keys[0] + i);
            if (keyset_ord(keys[0], sg) > keyset_ord(keys[1], sg)) keys.clear();  // wrapped: not a span test
            break;
        default:  // tiny maps, the empty map included
            for (uint64_t i = 0; i < n % 3; ++i) keys.push_back(rng() % 4 ? rng() : ~0ull);
            break;
        }
        // a key's value is a function of the key, so duplicates agree; the ends of the code range appear
        std::vector<uint16_t> vals;
        const uint64_t salt = rng();
        for (uint64_t k : keys) {
            const uint64_t h = (k ^ salt) * kKeysetHashMul >> 40;
            vals.push_back(h % 16 == 0 ? 65534 : h % 16 == 1 ? 0 : (uint16_t)(h % (it % 2 ? 25 : 65535)));
        }
        for (uint32_t form : {KM_AUTO, KM_DENSE, KM_HASH}) {
            // no dense array of hundreds of MiB: at the 2^31 limit the spans that fit are built as auto (the
            // hash table, with these few keys) and hash only, the ones past it are KM_TOO_WIDE
            if (form == KM_DENSE && !keys.empty()) {
                uint64_t lo, hi;
                span_of(keys, sg, lo, hi);
                if (hi - lo < kKeymapMaxSpan && keymap_dense_bytes(hi - lo) > (64ull << 20)) continue;
            }
            check_map(keys, vals, sg, form, rng);
        }
    }
    // the widest dense map: 2^31 values, 4 GiB (sized here, never allocated)
    if (keymap_dense_bytes(kKeymapMaxSpan - 1) != (1ull << 32) || keymap_dense_bytes(0) != 8 ||
        keymap_dense_bytes(4) != 16 || keymap_hash_bytes(0) != 16 || keymap_hash_bytes(3) != 80) {
        fprintf(stderr, "FAIL: image sizes at their ends\n");
        ++failures;
    }
    // the documented limit is checked before keys or values is read
    KeymapImage img;
    if (keymap_build(nullptr, nullptr, kMaxKeysetKeys + 1, true, KM_AUTO, img) != KM_TOO_MANY) {
        fprintf(stderr, "FAIL: n above kMaxKeysetKeys accepted\n");
        ++failures;
    }
    printf("iterations %d failures %d\n", iters, failures);
    return failures ? 1 : 0;
}
