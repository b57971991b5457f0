// fls_scan_keyset.hip -- key sets on the host: the registry of live sets and
// fls_keyset_create / free / info / contains (the set's image: fls_keyset.hpp;
// the probe kernel: fls_keyset.hip).  A filter term reaches a set through
// keyset_registry() (to_terms, flsgpu.hip); fls_disconnect drops its
// connection's sets there too.
#include "fls_engine.hpp"

using namespace fls;
using namespace fls::engine;

FLS_ENGINE_BEGIN

KeySetRegistry &keyset_registry() {
    static auto *r = new KeySetRegistry();
    return *r;
}

FLS_ENGINE_END

extern "C" {

int fls_keyset_create(fls_connection *conn, const uint64_t *keys, uint64_t n, int kind, int form, fls_keyset **out) {
    if (!conn || !out) return fail(FLS_ERR_ARG, "fls_keyset_create: NULL argument");
    if (kind != FLS_KEYSET_SIGNED && kind != FLS_KEYSET_UNSIGNED)
        return fail(FLS_ERR_ARG, "fls_keyset_create: kind %d (0 signed, 1 unsigned)", kind);
    if (form < 0 || form > 2) return fail(FLS_ERR_ARG, "fls_keyset_create: form %d (0 auto, 1 bitmap, 2 hash)", form);
    if (n > kMaxKeysetKeys)  // before keys is read
        return fail(FLS_ERR_LIMIT, "fls_keyset_create: %llu keys (at most %llu, kMaxKeysetKeys)", (unsigned long long)n,
                    (unsigned long long)kMaxKeysetKeys);
    if (n && !keys) return fail(FLS_ERR_ARG, "fls_keyset_create: NULL keys");
    auto ks = std::make_shared<KeySet>();
    ks->conn = conn;
    int rc;
    try {
        rc = keyset_build(keys, n, kind == FLS_KEYSET_SIGNED, (uint32_t)form, ks->img);
    } catch (const std::bad_alloc &) {
        return fail(FLS_ERR_NOMEM, "fls_keyset_create: out of memory");
    }
    if (rc == KS_TOO_WIDE)
        return fail(FLS_ERR_LIMIT, "fls_keyset_create: a bitmap over [min, max] would cover more than 2^32 values");
    if (rc != KS_OK) return fail(FLS_ERR_ARG, "fls_keyset_create: cannot build the set (%d)", rc);
    KeySetRegistry &R = keyset_registry();
    std::lock_guard<std::mutex> lk(R.mu);
    const uint64_t h = KeySetRegistry::handle_of(R.next++);
    R.live[h] = std::move(ks);
    *out = (fls_keyset *)(uintptr_t)h;
    return 0;
}

void fls_keyset_free(fls_keyset *set) {
    KeySetRegistry &R = keyset_registry();
    std::shared_ptr<KeySet> dead;  // released outside the lock
    std::lock_guard<std::mutex> lk(R.mu);
    auto it = R.live.find((uint64_t)(uintptr_t)set);
    if (it == R.live.end()) return;
    dead = std::move(it->second);
    R.live.erase(it);
}

int fls_keyset_info(const fls_keyset *set, fls_keyset_info_t *info) {
    auto ks = keyset_registry().find((uint64_t)(uintptr_t)set);
    if (!ks || !info) return fail(FLS_ERR_ARG, "fls_keyset_info: not a live key set");
    const KeysetImage &k = ks->img;
    memset(info, 0, sizeof(*info));
    info->count = k.keys.size();
    info->form = k.form;
    info->kind = k.is_signed ? FLS_KEYSET_SIGNED : FLS_KEYSET_UNSIGNED;
    info->device_bytes = k.bytes();
    info->capacity = k.capacity();
    info->max_probe = k.max_probe;
    info->min = k.min;
    info->max = k.max;
    info->empty = k.empty;
    return 0;
}

int fls_keyset_contains(const fls_keyset *set, uint64_t key) {
    auto ks = keyset_registry().find((uint64_t)(uintptr_t)set);
    if (!ks) return fail(FLS_ERR_ARG, "fls_keyset_contains: not a live key set");
    return keyset_contains(ks->img, key) ? 1 : 0;
}

}  // extern "C"
