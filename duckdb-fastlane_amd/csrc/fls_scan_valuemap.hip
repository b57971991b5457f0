// fls_scan_valuemap.hip -- value maps on the host: the registry of live maps
// and fls_valuemap_create / free / info / lookup (the map's image:
// fls_valuemap.hpp; the probe kernel: fls_mapcmp.hip).  The terms that use a
// map (FLS_CMP_MAP_EQ .. FLS_CMP_MAP_GE) are filter terms: their checks,
// pruning and per-batch descriptors sit with the other terms' in flsgpu.hip;
// fls_disconnect drops its connection's maps there too.
#include "fls_engine.hpp"

using namespace fls;
using namespace fls::engine;

FLS_ENGINE_BEGIN

ValueMapRegistry &valuemap_registry() {
    static auto *r = new ValueMapRegistry();
    return *r;
}

FLS_ENGINE_END

extern "C" {

int fls_valuemap_create(fls_connection *conn, const uint64_t *keys, const uint64_t *values, uint64_t n, int key_kind,
                        int value_kind, int form, fls_valuemap **out) {
    if (!conn || !out) return fail(FLS_ERR_ARG, "fls_valuemap_create: NULL argument");
    if (key_kind != FLS_KEYSET_SIGNED && key_kind != FLS_KEYSET_UNSIGNED)
        return fail(FLS_ERR_ARG, "fls_valuemap_create: key kind %d (0 signed, 1 unsigned)", key_kind);
    if (value_kind != FLS_KEYSET_SIGNED && value_kind != FLS_KEYSET_UNSIGNED)
        return fail(FLS_ERR_ARG, "fls_valuemap_create: value kind %d (0 signed, 1 unsigned)", value_kind);
    if (form < 0 || form > 2) return fail(FLS_ERR_ARG, "fls_valuemap_create: form %d (0 auto, 1 dense, 2 hash)", form);
    if (n > kMaxKeysetKeys)  // before keys or values is read
        return fail(FLS_ERR_LIMIT, "fls_valuemap_create: %llu keys (at most %llu, kMaxKeysetKeys)", (unsigned long long)n,
                    (unsigned long long)kMaxKeysetKeys);
    if (n && (!keys || !values)) return fail(FLS_ERR_ARG, "fls_valuemap_create: NULL keys or values");
    auto vm = std::make_shared<ValueMap>();
    vm->conn = conn;
    int rc;
    try {
        rc = valuemap_build(keys, values, n, key_kind == FLS_KEYSET_SIGNED, value_kind == FLS_KEYSET_SIGNED,
                            (uint32_t)form, vm->img);
    } catch (const std::bad_alloc &) {
        return fail(FLS_ERR_NOMEM, "fls_valuemap_create: out of memory");
    }
    const ValuemapImage &m = vm->img;
    if (rc == VM_TOO_WIDE)
        return fail(FLS_ERR_LIMIT, "fls_valuemap_create: a dense map over [min, max] would cover more than 2^28 keys");
    if (rc == VM_CONFLICT) {
        if (m.value_signed)
            return fail(FLS_ERR_ARG, "fls_valuemap_create: key 0x%llx (%lld) is listed with the values %lld and %lld: a map "
                        "is a function", (unsigned long long)m.bad_key, (long long)m.bad_key, (long long)m.bad_a,
                        (long long)m.bad_b);
        return fail(FLS_ERR_ARG, "fls_valuemap_create: key 0x%llx (%lld) is listed with the values %llu and %llu: a map is "
                    "a function", (unsigned long long)m.bad_key, (long long)m.bad_key, (unsigned long long)m.bad_a,
                    (unsigned long long)m.bad_b);
    }
    if (rc != VM_OK) return fail(FLS_ERR_ARG, "fls_valuemap_create: cannot build the map (%d)", rc);
    ValueMapRegistry &R = valuemap_registry();
    std::lock_guard<std::mutex> lk(R.mu);
    const uint64_t h = ValueMapRegistry::handle_of(R.next++);
    R.live[h] = std::move(vm);
    *out = (fls_valuemap *)(uintptr_t)h;
    return 0;
}

void fls_valuemap_free(fls_valuemap *map) {
    ValueMapRegistry &R = valuemap_registry();
    std::shared_ptr<ValueMap> dead;  // released outside the lock
    std::lock_guard<std::mutex> lk(R.mu);
    auto it = R.live.find((uint64_t)(uintptr_t)map);
    if (it == R.live.end()) return;
    dead = std::move(it->second);
    R.live.erase(it);
}

int fls_valuemap_info(const fls_valuemap *map, fls_valuemap_info_t *info) {
    auto vm = valuemap_registry().find((uint64_t)(uintptr_t)map);
    if (!vm || !info) return fail(FLS_ERR_ARG, "fls_valuemap_info: not a live value map");
    const ValuemapImage &m = vm->img;
    memset(info, 0, sizeof(*info));
    info->count = m.set.keys.size();
    info->form = m.form;
    info->key_kind = m.set.is_signed ? FLS_KEYSET_SIGNED : FLS_KEYSET_UNSIGNED;
    info->value_kind = m.value_signed ? FLS_KEYSET_SIGNED : FLS_KEYSET_UNSIGNED;
    info->max_probe = m.form == VM_HASH ? m.set.max_probe : 0;
    info->device_bytes = m.bytes();
    info->capacity = m.capacity();
    info->key_min = m.set.min;
    info->key_max = m.set.max;
    info->value_min = m.vmin;
    info->value_max = m.vmax;
    info->empty = m.set.empty;
    return 0;
}

int fls_valuemap_lookup(const fls_valuemap *map, uint64_t key, uint64_t *value) {
    auto vm = valuemap_registry().find((uint64_t)(uintptr_t)map);
    if (!vm) return fail(FLS_ERR_ARG, "fls_valuemap_lookup: not a live value map");
    uint64_t v = 0;
    if (!valuemap_lookup(vm->img, key, &v)) return 0;
    if (value) *value = v;
    return 1;
}

}  // extern "C"
