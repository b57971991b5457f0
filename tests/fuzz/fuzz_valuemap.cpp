// fuzz_valuemap.cpp -- host-side sanitizer run of the value-map construction
// (csrc/fls_valuemap.hpp), built with g++ -fsanitize=address,undefined by
// tests/test_valuemap.py.  Seeded random and adversarial maps in every form;
// valuemap_lookup (the probe of the uploaded image) is checked against
// std::map for the keys, their neighbours, holes, the sentinel candidates and
// random probes, the image's bytes against a rebuild from shuffled and doubled
// input, vmin / vmax against the value kind's order, and the refusals (a
// conflicting duplicate, the limits) against their rules.
//
// usage: fuzz_valuemap <iterations> <seed>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "fls_valuemap.hpp"

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

static void check_map(const std::vector<uint64_t> &keys, const std::vector<uint64_t> &vals, bool sg, bool vsg,
                      uint32_t form, std::mt19937_64 &rng) {
    ValuemapImage img;
    const int rc = valuemap_build(keys.data(), vals.data(), keys.size(), sg, vsg, form, img);
    std::map<uint64_t, uint64_t> ref;
    for (size_t i = 0; i < keys.size(); ++i) ref[keys[i]] = vals[i];  // (the callers give a key one value)
    if (rc == VM_TOO_WIDE) {
        uint64_t lo, hi;
        span_of(keys, sg, lo, hi);
        CHECK(form == VM_DENSE && hi - lo >= kValuemapMaxSpan, "TOO_WIDE for span %" PRIu64, hi - lo);
        return;
    }
    CHECK(rc == VM_OK, "build rc %d", rc);
    const KeysetImage &s = img.set;
    CHECK(s.keys.size() == ref.size() && img.values.size() == ref.size(), "distinct %zu vs %zu", s.keys.size(), ref.size());
    CHECK(form == VM_AUTO || img.form == form, "form %u forced, %u built", form, img.form);
    CHECK(img.value_signed == vsg && s.is_signed == sg, "kinds");
    for (size_t i = 1; i < s.keys.size(); ++i)
        CHECK(keyset_ord(s.keys[i - 1], sg) < keyset_ord(s.keys[i], sg), "keys not ascending at %zu", i);
    uint64_t vlo = 0, vhi = 0;
    bool first = true;
    for (auto &kv : ref) {
        if (first || keyset_ord(kv.second, vsg) < keyset_ord(vlo, vsg)) vlo = kv.second;
        if (first || keyset_ord(kv.second, vsg) > keyset_ord(vhi, vsg)) vhi = kv.second;
        first = false;
    }
    CHECK(img.vmin == vlo && img.vmax == vhi, "vmin / vmax %" PRIx64 " %" PRIx64 " vs %" PRIx64 " %" PRIx64, img.vmin,
          img.vmax, vlo, vhi);
    if (img.form == VM_HASH) {
        const uint64_t cap = 1ull << s.cap_log2;
        CHECK(cap >= 2 * ref.size() && img.bytes() == valuemap_hash_bytes(s.cap_log2) && img.bytes() == 16 * cap,
              "hash image size");
        CHECK(!ref.count(s.empty), "sentinel %" PRIx64 " is a key", s.empty);
        size_t used = 0;
        for (uint64_t i = 0; i < cap; ++i) {
            const bool occ = img.words[i] != s.empty;
            used += occ;
            CHECK(occ || img.hash_values()[i] == 0, "value of empty slot %" PRIu64, i);
        }
        CHECK(used == ref.size(), "occupied slots %zu vs %zu", used, ref.size());
        CHECK(s.max_probe <= cap, "max_probe");
    } else {
        CHECK(s.span < kValuemapMaxSpan && img.bytes() == valuemap_dense_bytes(s.span) &&
                  img.words.size() == s.span + 1 + (s.span + 64) / 64, "dense image size");
        size_t present = 0;
        for (uint64_t d = 0; d <= s.span; ++d) {
            const bool bit = (img.presence()[d >> 6] >> (d & 63)) & 1;
            present += bit;
            CHECK(bit || img.words[d] == 0, "a hole holds %" PRIx64, img.words[d]);
        }
        CHECK(present == ref.size(), "presence bits %zu vs %zu", present, ref.size());
        for (uint64_t d = s.span + 1; d < 64 * ((s.span + 64) / 64); ++d)
            CHECK(!((img.presence()[d >> 6] >> (d & 63)) & 1), "presence bit past the span");
    }
    auto probe = [&](uint64_t k) {
        auto it = ref.find(k);
        uint64_t got = 0x5555;
        const bool found = valuemap_lookup(img, k, &got);
        CHECK(found == (it != ref.end()) && (!found || got == it->second),
              "lookup(%" PRIx64 ") = %d %" PRIx64 ", form %u n %zu", k, (int)found, got, img.form, ref.size());
        CHECK(valuemap_lookup(img, k, nullptr) == found, "lookup without a value");
    };
    for (auto &kv : ref) {
        probe(kv.first);
        probe(kv.first + 1);
        probe(kv.first - 1);
        probe(kv.first ^ (1ull << 63));
    }
    const std::vector<uint64_t> edges = {0, 1, ~0ull, ~0ull - 1, ~0ull - 2, 1ull << 63, (1ull << 63) - 1, s.empty,
                                         s.min - 1, s.max + 1, s.min + kValuemapMaxSpan, s.min - kValuemapMaxSpan};
    for (uint64_t k : edges) probe(k);
    for (int i = 0; i < 256; ++i) probe(rng());
    if (img.form == VM_DENSE && s.span < 4096)
        for (uint64_t d = 0; d <= s.span; ++d) probe(s.min + d);  // every hole
    // the image is a function of the map: shuffled input with every pair doubled
    std::vector<size_t> order(keys.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::shuffle(order.begin(), order.end(), rng);
    std::vector<uint64_t> k2, v2;
    for (size_t i : order) {
        k2.push_back(keys[i]);
        v2.push_back(vals[i]);
    }
    k2.insert(k2.end(), keys.begin(), keys.end());
    v2.insert(v2.end(), vals.begin(), vals.end());
    ValuemapImage again;
    CHECK(valuemap_build(k2.data(), v2.data(), k2.size(), sg, vsg, form, again) == VM_OK, "rebuild");
    CHECK(again.form == img.form && again.words == img.words && again.set.keys == s.keys && again.values == img.values &&
              again.set.max_probe == s.max_probe && again.set.empty == s.empty && again.vmin == img.vmin &&
              again.vmax == img.vmax, "image depends on the input order");
    // a conflicting value for one key is refused and named
    if (!keys.empty()) {
        const size_t j = rng() % keys.size();
        k2.push_back(keys[j]);
        v2.push_back(vals[j] + 1 + rng() % 5);
        ValuemapImage bad;
        CHECK(valuemap_build(k2.data(), v2.data(), k2.size(), sg, vsg, form, bad) == VM_CONFLICT &&
                  bad.bad_key == keys[j] && std::min(bad.bad_a, bad.bad_b) == std::min(vals[j], v2.back()) &&
                  std::max(bad.bad_a, bad.bad_b) == std::max(vals[j], v2.back()), "conflict not refused");
    }
}

int main(int argc, char **argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 200;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    for (int it = 0; it < iters; ++it) {
        std::vector<uint64_t> keys;
        const uint64_t n = rng() % (it % 8 == 0 ? 5000 : 64);
        const bool sg = rng() & 1, vsg = rng() & 1;
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
        case 5:  // two clusters 2^28 - 1, 2^28 or 2^28 + 1 apart (the dense limit)
            keys.push_back(rng());
            keys.push_back(keys[0] + kValuemapMaxSpan - 1 + (rng() % 3) - (n & 1));
            for (uint64_t i = 0; i < n; ++i) keys.push_back(keys[0] + i);
            if (keyset_ord(keys[0], sg) > keyset_ord(keys[1], sg)) keys.clear();  // wrapped: not a span test
            break;
        default:  // tiny maps, the empty map included
            for (uint64_t i = 0; i < n % 3; ++i) keys.push_back(rng() % 4 ? rng() : ~0ull);
            break;
        }
        // a key's value is a function of the key, so duplicates agree; 0, ~0 and both ends of int64 appear
        std::vector<uint64_t> vals;
        const uint64_t salt = rng();
        for (uint64_t k : keys) {
            const uint64_t h = (k ^ salt) * kKeysetHashMul;
            switch ((h >> 40) % 16) {
            case 0: vals.push_back(0); break;
            case 1: vals.push_back(~0ull); break;
            case 2: vals.push_back(1ull << 63); break;
            case 3: vals.push_back((1ull << 63) - 1); break;
            default: vals.push_back(it % 2 ? h : (h >> 40) % 25); break;
            }
        }
        for (uint32_t form : {VM_AUTO, VM_DENSE, VM_HASH}) {
            // no dense array of hundreds of MiB: near the 2^28 limit the spans that fit are built as auto (the
            // hash table, with these few keys) and hash only, the ones past it are VM_TOO_WIDE
            if (form == VM_DENSE && !keys.empty()) {
                uint64_t lo, hi;
                span_of(keys, sg, lo, hi);
                if (hi - lo < kValuemapMaxSpan && valuemap_dense_bytes(hi - lo) > (64ull << 20)) continue;
            }
            check_map(keys, vals, sg, vsg, form, rng);
        }
    }
    // the two size formulas at their ends (the widest dense map is sized here, never allocated)
    if (valuemap_dense_bytes(0) != 16 || valuemap_dense_bytes(63) != 64 * 8 + 8 || valuemap_dense_bytes(64) != 65 * 8 + 16 ||
        valuemap_dense_bytes(kValuemapMaxSpan - 1) != (1ull << 31) + (1ull << 25) || valuemap_hash_bytes(0) != 16 ||
        valuemap_hash_bytes(3) != 128) {
        fprintf(stderr, "FAIL: image sizes at their ends\n");
        ++failures;
    }
    // the documented limit is checked before keys or values is read
    ValuemapImage img;
    if (valuemap_build(nullptr, nullptr, kMaxKeysetKeys + 1, true, true, VM_AUTO, img) != VM_TOO_MANY) {
        fprintf(stderr, "FAIL: n above kMaxKeysetKeys accepted\n");
        ++failures;
    }
    printf("iterations %d failures %d\n", iters, failures);
    return failures ? 1 : 0;
}
