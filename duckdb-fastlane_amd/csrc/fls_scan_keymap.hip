// fls_scan_keymap.hip -- key maps on the host: the registry of live maps,
// fls_keymap_create / free / info / lookup, the bindings of mapped GROUP BY
// keys (fls_aggregate_key_bindings), their row-group pruning and the per-batch
// probe (the map's image: fls_keymap.hpp; the probe kernel: fls_keymap.hip).
// fls_aggregate_grouped (fls_scan_agg.hip) resolves FLS_KEY_MAPPED | i against
// the table's bindings; fls_disconnect drops its connection's maps here too.
#include "fls_engine.hpp"

using namespace fls;
using namespace fls::engine;

FLS_ENGINE_BEGIN

KeyMapRegistry &keymap_registry() {
    static auto *r = new KeyMapRegistry();
    return *r;
}

bool binding_may_match(const fls_table *t, uint32_t rg, const HostBinding &b) {
    const RowGroupMeta &r = t->meta.rgs[rg];
    const KeysetImage &ks = b.map->img.set;
    if (ks.keys.empty()) return false;  // the empty map matches nowhere
    if (r.zones.empty()) return true;
    const ZoneMap &z = r.zones[b.col];
    if (z.flags & ZM_ALL_NULL) return false;  // no valid row to probe with
    if (!(z.flags & ZM_VALID)) return true;
    return keyset_any_in_range(ks, z.min, z.max);  // exact on a sorted column
}

int enqueue_keymap(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows) {
    const uint32_t nb = (uint32_t)s.binds.size();
    const size_t nvec = (size_t)((rows + 1023) / 1024);
    const std::vector<uint8_t> &need = sl.valid_staged;
    HIP_TRY(sl.h_mdesc.alloc(nb));
    HIP_TRY(sl.d_mdesc.alloc(d.dev, nb));
    HIP_TRY(sl.d_kcode.alloc(d.dev, (size_t)nb * 1024 * nvec));
    HIP_TRY(sl.d_kvalid.alloc(d.dev, (size_t)nb * 16 * nvec));
    for (uint32_t i = 0; i < nb; ++i) {
        const HostBinding &b = s.binds[i];
        const KeymapImage &mi = b.map->img;
        DevMapTerm &dm = sl.h_mdesc.p[i];
        memset(&dm, 0, sizeof(dm));
        dm.col = sl.d_out[b.col].p;
        dm.valid = need[b.col] ? sl.d_valid[b.col].p : nullptr;
        HIP_TRY(b.map->device_image(d.dev, &dm.table));
        dm.code = sl.d_kcode.p + (size_t)i * 1024 * nvec;
        dm.kvalid = b.keep ? sl.d_kvalid.p + (size_t)i * 16 * nvec : nullptr;
        dm.min = mi.set.min;
        dm.span = mi.set.span;
        dm.empty = mi.set.empty;
        dm.cap_log2 = mi.set.cap_log2;
        dm.max_probe = mi.set.max_probe;
        dm.form = (uint8_t)mi.form;
        dm.ob = (uint8_t)out_bytes_of(t, b.col);
        dm.sign = mi.set.is_signed ? 1 : 0;
        dm.keep = b.keep ? 1 : 0;
    }
    HIP_TRY(hipMemcpyAsync(sl.d_mdesc.p, sl.h_mdesc.p, nb * sizeof(DevMapTerm), hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(launch_keymap(sl.d_mdesc.p, nb, (uint32_t)rows, sl.d_mask.p, sl.d_counts.p, d.err.p, sl.stream));
    return 0;
}

FLS_ENGINE_END

extern "C" {

int fls_keymap_create(fls_connection *conn, const uint64_t *keys, const uint16_t *values, uint64_t n, int kind, int form,
                      fls_keymap **out) {
    if (!conn || !out) return fail(FLS_ERR_ARG, "fls_keymap_create: NULL argument");
    if (kind != FLS_KEYSET_SIGNED && kind != FLS_KEYSET_UNSIGNED)
        return fail(FLS_ERR_ARG, "fls_keymap_create: kind %d (0 signed, 1 unsigned)", kind);
    if (form < 0 || form > 2) return fail(FLS_ERR_ARG, "fls_keymap_create: form %d (0 auto, 1 dense, 2 hash)", form);
    if (n > kMaxKeysetKeys)  // before keys or values is read
        return fail(FLS_ERR_LIMIT, "fls_keymap_create: %llu keys (at most %llu, kMaxKeysetKeys)", (unsigned long long)n,
                    (unsigned long long)kMaxKeysetKeys);
    if (n && (!keys || !values)) return fail(FLS_ERR_ARG, "fls_keymap_create: NULL keys or values");
    auto km = std::make_shared<KeyMap>();
    km->conn = conn;
    int rc;
    try {
        rc = keymap_build(keys, values, n, kind == FLS_KEYSET_SIGNED, (uint32_t)form, km->img);
    } catch (const std::bad_alloc &) {
        return fail(FLS_ERR_NOMEM, "fls_keymap_create: out of memory");
    }
    const KeymapImage &m = km->img;
    if (rc == KM_TOO_WIDE)
        return fail(FLS_ERR_LIMIT, "fls_keymap_create: a dense map over [min, max] would cover more than 2^31 values");
    if (rc == KM_BAD_VALUE)
        return fail(FLS_ERR_ARG, "fls_keymap_create: key 0x%llx has the value 65535, which is reserved (codes are 0 to 65534)",
                    (unsigned long long)m.bad_key);
    if (rc == KM_CONFLICT)
        return fail(FLS_ERR_ARG, "fls_keymap_create: key 0x%llx (%lld) is listed with the values %u and %u: a map is a function",
                    (unsigned long long)m.bad_key, (long long)m.bad_key, m.bad_a, m.bad_b);
    if (rc != KM_OK) return fail(FLS_ERR_ARG, "fls_keymap_create: cannot build the map (%d)", rc);
    KeyMapRegistry &R = keymap_registry();
    std::lock_guard<std::mutex> lk(R.mu);
    const uint64_t h = KeyMapRegistry::handle_of(R.next++);
    R.live[h] = std::move(km);
    *out = (fls_keymap *)(uintptr_t)h;
    return 0;
}

void fls_keymap_free(fls_keymap *map) {
    KeyMapRegistry &R = keymap_registry();
    std::shared_ptr<KeyMap> dead;  // released outside the lock
    std::lock_guard<std::mutex> lk(R.mu);
    auto it = R.live.find((uint64_t)(uintptr_t)map);
    if (it == R.live.end()) return;
    dead = std::move(it->second);
    R.live.erase(it);
}

int fls_keymap_info(const fls_keymap *map, fls_keymap_info_t *info) {
    auto km = keymap_registry().find((uint64_t)(uintptr_t)map);
    if (!km || !info) return fail(FLS_ERR_ARG, "fls_keymap_info: not a live key map");
    const KeymapImage &m = km->img;
    memset(info, 0, sizeof(*info));
    info->count = m.set.keys.size();
    info->form = m.form;
    info->kind = m.set.is_signed ? FLS_KEYSET_SIGNED : FLS_KEYSET_UNSIGNED;
    info->device_bytes = m.bytes();
    info->capacity = m.capacity();
    info->max_probe = m.form == KM_HASH ? m.set.max_probe : 0;
    info->max_code = m.max_code;
    info->min = m.set.min;
    info->max = m.set.max;
    info->empty = m.set.empty;
    return 0;
}

int fls_keymap_lookup(const fls_keymap *map, uint64_t key, uint32_t *code) {
    auto km = keymap_registry().find((uint64_t)(uintptr_t)map);
    if (!km) return fail(FLS_ERR_ARG, "fls_keymap_lookup: not a live key map");
    const uint16_t c = keymap_lookup(km->img, key);
    if (c == kKeymapAbsent) return 0;
    if (code) *code = c;
    return 1;
}

int fls_aggregate_key_bindings(fls_table *t, const fls_key_binding *b, uint32_t n) {
    if (!t || (!b && n)) return fail(FLS_ERR_ARG, "fls_aggregate_key_bindings: NULL argument");
    if (n > kMaxKeys) return fail(FLS_ERR_ARG, "fls_aggregate_key_bindings: %u bindings (at most %u)", n, kMaxKeys);
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    std::vector<HostBinding> hb(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (b[i].col >= ncols) return fail(FLS_ERR_ARG, "binding %u: column %u out of range", i, b[i].col);
        const ColumnMeta &cm = t->meta.cols[b[i].col];
        const uint8_t ty = cm.type;
        if (type_is_string(ty) || type_is_float(ty) || !type_valid(ty))
            return fail(FLS_ERR_ARG, "binding %u: a key map cannot be probed with a VARCHAR / BLOB / FLOAT / DOUBLE "
                        "column (%u)", i, b[i].col);
        if (ty == TY_DECIMAL && cm.width > 18)
            return fail(FLS_ERR_ARG, "binding %u: a key map cannot be probed with a DECIMAL wider than 64 bits "
                        "(column %u)", i, b[i].col);
        if (b[i].flags & ~FLS_KEYMAP_KEEP_UNMATCHED)
            return fail(FLS_ERR_ARG, "binding %u: unknown flag bits 0x%x", i, b[i].flags & ~FLS_KEYMAP_KEEP_UNMATCHED);
        hb[i].map = keymap_registry().find(b[i].map);
        if (!hb[i].map)
            return fail(FLS_ERR_ARG, "binding %u: map 0x%llx is not a live key map", i, (unsigned long long)b[i].map);
        if (hb[i].map->img.set.is_signed != type_is_signed(ty))
            return fail(FLS_ERR_ARG, "binding %u: the key map's kind is %s, column %u is %s", i,
                        hb[i].map->img.set.is_signed ? "signed" : "unsigned", b[i].col,
                        type_is_signed(ty) ? "signed" : "unsigned");
        hb[i].col = b[i].col;
        hb[i].keep = (b[i].flags & FLS_KEYMAP_KEEP_UNMATCHED) != 0;
    }
    t->bindings = std::move(hb);
    return 0;
}

}  // extern "C"
