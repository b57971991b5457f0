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

uint32_t used_value_bindings(const std::vector<HostAgg> &ha, const std::vector<uint32_t> *keys) {
    uint32_t used = 0;
    auto use = [&](uint32_t c) {
        if (is_mapped_col(c)) used |= 1u << mapped_index(c);
    };
    for (const HostAgg &a : ha) {
        if (a.fn == AGG_COUNT_STAR) continue;
        if (a.fn == AGG_SUM_EXPR) {
            for (uint32_t k = 0; k < a.nf; ++k) use(a.fcol[k]);
            continue;
        }
        use(a.col);
        if (a.fn == AGG_SUM_PRODUCT) use(a.col2);
    }
    if (keys)
        for (uint32_t c : *keys) use(c);
    return used;
}

bool value_binding_may_match(const fls_table *t, uint32_t rg, const HostValueBinding &b) {
    const RowGroupMeta &r = t->meta.rgs[rg];
    const KeysetImage &ks = b.map->img.set;
    if (ks.keys.empty()) return false;  // the empty map matches nowhere
    if (r.zones.empty()) return true;
    const ZoneMap &z = r.zones[b.col];
    if (z.flags & ZM_ALL_NULL) return false;  // no valid row to probe with
    if (!(z.flags & ZM_VALID)) return true;
    return keyset_any_in_range(ks, z.min, z.max);  // exact on a sorted column
}

uint32_t prune_value_bindings(const fls_table *t, const std::vector<HostValueBinding> &vb, uint32_t vused,
                              std::vector<uint32_t> &rgs) {
    uint32_t pruned = 0;
    for (uint32_t i = 0; i < vb.size(); ++i) {
        if (!((vused >> i) & 1) || vb[i].keep) continue;  // a left join, or a binding the call does not name
        std::vector<uint32_t> keep;
        for (uint32_t r : rgs)
            if (value_binding_may_match(t, r, vb[i])) keep.push_back(r);
        pruned += (uint32_t)(rgs.size() - keep.size());
        rgs.swap(keep);
    }
    return pruned;
}

bool operand_is_float(const fls_table *t, uint32_t c) {
    return !is_mapped_col(c) && type_is_float(t->meta.cols[c].type);
}

bool operand_is_signed(const fls_table *t, uint32_t c) {
    if (is_mapped_col(c)) return t->vbindings[mapped_index(c)].map->img.value_signed;
    return type_is_signed(t->meta.cols[c].type);
}

OperandRef operand_ref(const fls_table *t, const ScanCtx &s, const Slot &sl, uint32_t c) {
    OperandRef r;
    if (is_mapped_col(c)) {
        const uint32_t i = mapped_index(c), slot = mapped_slot(s.vused, i);
        const size_t nvec = sl.hb->nvec;
        r.col = (const uint8_t *)(sl.d_mval.p + (size_t)slot * 1024 * nvec);
        // (an inner binding's misses left the mask: every selected row is valid)
        r.valid = s.vbinds[i].keep ? sl.d_mvalid.p + (size_t)slot * 16 * nvec : nullptr;
        r.ob = 8;
        r.kind = s.vbinds[i].map->img.value_signed ? FK_INT : FK_UINT;
        return r;
    }
    r.col = sl.d_out[c].p;
    r.valid = sl.valid_staged[c] ? sl.d_valid[c].p : nullptr;
    r.ob = (uint8_t)out_bytes_of(t, c);
    r.kind = col_kind(t, c);
    return r;
}

int enqueue_mapval(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows) {
    const uint32_t nb = (uint32_t)__builtin_popcount(s.vused);
    const size_t nvec = (size_t)((rows + 1023) / 1024);
    const std::vector<uint8_t> &need = sl.valid_staged;
    if (nb == 0 || nb > kMaxValueBindings || (s.vused >> s.vbinds.size()) != 0)
        return fail(FLS_ERR_STATE, "internal: %u value bindings in a scan", nb);
    HIP_TRY(sl.h_mvdesc.alloc(nb));
    HIP_TRY(sl.d_mvdesc.alloc(d.dev, nb));
    HIP_TRY(sl.d_mval.alloc(d.dev, (size_t)nb * 1024 * nvec));
    HIP_TRY(sl.d_mvalid.alloc(d.dev, (size_t)nb * 16 * nvec));
    for (uint32_t i = 0; i < s.vbinds.size(); ++i) {
        if (!((s.vused >> i) & 1)) continue;
        const HostValueBinding &b = s.vbinds[i];
        const ValuemapImage &vi = b.map->img;
        const uint32_t slot = mapped_slot(s.vused, i);
        DevMapValTerm &dm = sl.h_mvdesc.p[slot];
        memset(&dm, 0, sizeof(dm));
        dm.key = sl.d_out[b.col].p;
        dm.vk = need[b.col] ? sl.d_valid[b.col].p : nullptr;
        HIP_TRY(b.map->device_image(d.dev, &dm.table));
        dm.out = sl.d_mval.p + (size_t)slot * 1024 * nvec;
        dm.ovalid = sl.d_mvalid.p + (size_t)slot * 16 * nvec;
        dm.min = vi.set.min;
        dm.span = vi.set.span;
        dm.empty = vi.set.empty;
        dm.cap_log2 = vi.set.cap_log2;
        dm.max_probe = vi.set.max_probe;
        dm.form = (uint8_t)vi.form;
        dm.obk = (uint8_t)out_bytes_of(t, b.col);
        dm.ksign = vi.set.is_signed ? 1 : 0;
        dm.keep = b.keep ? 1 : 0;
    }
    HIP_TRY(hipMemcpyAsync(sl.d_mvdesc.p, sl.h_mvdesc.p, nb * sizeof(DevMapValTerm), hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(launch_mapval(sl.d_mvdesc.p, nb, (uint32_t)rows, sl.d_mask.p, sl.d_counts.p, d.err.p, sl.stream));
    return 0;
}

FLS_ENGINE_END

extern "C" {

int fls_aggregate_value_bindings(fls_table *t, const fls_value_binding *b, uint32_t n) {
    if (!t || (!b && n)) return fail(FLS_ERR_ARG, "fls_aggregate_value_bindings: NULL argument");
    if (n > kMaxValueBindings)
        return fail(FLS_ERR_ARG, "fls_aggregate_value_bindings: %u bindings (at most %u)", n, kMaxValueBindings);
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    std::vector<HostValueBinding> hb(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (b[i].col >= ncols) return fail(FLS_ERR_ARG, "value binding %u: column %u out of range", i, b[i].col);
        const ColumnMeta &cm = t->meta.cols[b[i].col];
        const uint8_t ty = cm.type;
        if (type_is_string(ty) || type_is_float(ty) || !type_valid(ty))
            return fail(FLS_ERR_ARG, "value binding %u: a value map cannot be probed with a VARCHAR / BLOB / FLOAT / "
                        "DOUBLE column (%u)", i, b[i].col);
        if (ty == TY_DECIMAL && cm.width > 18)
            return fail(FLS_ERR_ARG, "value binding %u: a value map cannot be probed with a DECIMAL wider than 64 bits "
                        "(column %u)", i, b[i].col);
        if (b[i].flags & ~FLS_VALUEMAP_KEEP_UNMATCHED)
            return fail(FLS_ERR_ARG, "value binding %u: unknown flag bits 0x%x", i,
                        b[i].flags & ~FLS_VALUEMAP_KEEP_UNMATCHED);
        hb[i].map = valuemap_registry().find(b[i].map);
        if (!hb[i].map)
            return fail(FLS_ERR_ARG, "value binding %u: map 0x%llx is not a live value map", i,
                        (unsigned long long)b[i].map);
        if (hb[i].map->img.set.is_signed != type_is_signed(ty))
            return fail(FLS_ERR_ARG, "value binding %u: the value map's key kind is %s, column %u is %s", i,
                        hb[i].map->img.set.is_signed ? "signed" : "unsigned", b[i].col,
                        type_is_signed(ty) ? "signed" : "unsigned");
        hb[i].col = b[i].col;
        hb[i].keep = (b[i].flags & FLS_VALUEMAP_KEEP_UNMATCHED) != 0;
    }
    t->vbindings = std::move(hb);
    return 0;
}

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
