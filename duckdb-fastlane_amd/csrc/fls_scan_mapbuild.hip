// fls_scan_mapbuild.hip -- value maps and key maps built on the GPU from a
// filtered scan of a key and a value column (fls_valuemap_from_scan,
// fls_keymap_from_scan), step by step as fls_keyset_from_scan builds a set
// (fls_scan_keyset.hip): the argument checks, the surviving row groups and the
// collecting range the key column's zone maps give, the gate, one collecting
// array per GPU filled with 0xFF bytes, a Reduce::MapBuild scan (per batch:
// enqueue_mapbuild, called by fill_batch; the kernels: fls_mapbuild.hip), the
// compaction of each GPU's array into presence words and values, their merge
// on the host (mapbuild_merge, fls_mapbuild.hpp) and valuemap_finish_sorted /
// keymap_finish_sorted.  The finished map sits in its registry like one built
// by fls_valuemap_create / fls_keymap_create and is uploaded at its first
// probe.
#include "fls_engine.hpp"
#include "fls_mapbuild.hpp"

using namespace fls;
using namespace fls::engine;

FLS_ENGINE_BEGIN

// The map build's part of a batch (called by fill_batch for Reduce::MapBuild),
// after the filter's kernels on the slot's mask: the selected pairs with key
// and value both valid into the GPU's collecting array, and the per-vector
// counts of those rows as the batch's only D2H.
int enqueue_mapbuild(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t) {
    HostBatch &hb = *sl.hb;
    const MapBuildPlan &mb = s.mapbuild;
    size_t g = 0;
    while (g < s.devs.size() && s.devs[g].get() != &d) ++g;
    if (g >= mb.slots.size() || !mb.slots[g])
        return fail(FLS_ERR_STATE, "internal: map build without a collecting array on GPU %d", d.dev);
    if (rows > 0xFFFFFFFFull) return fail(FLS_ERR_LIMIT, "map build: a batch of more than 2^32 - 1 rows");
    const uint32_t kc = mb.key_col, vc = mb.value_col;
    DevMapBuild p;
    memset(&p, 0, sizeof(p));
    p.key = sl.d_out[kc].p;
    p.value = sl.d_out[vc].p;
    p.vk = sl.valid_staged[kc] ? sl.d_valid[kc].p : nullptr;  // (enqueue_filter staged the filter's and both columns' validity)
    p.vv = sl.valid_staged[vc] ? sl.d_valid[vc].p : nullptr;
    p.mask = sl.d_mask.p;
    p.slot = mb.slots[g];
    p.base = mb.base;
    p.span = mb.span;
    p.nrows = (uint32_t)rows;
    p.obk = (uint8_t)out_bytes_of(t, kc);
    p.obv = (uint8_t)out_bytes_of(t, vc);
    p.ksign = type_is_signed(t->meta.cols[kc].type) ? 1 : 0;
    p.vsign = type_is_signed(t->meta.cols[vc].type) ? 1 : 0;
    HIP_TRY(hb.h_counts.alloc(hb.nvec));
    HIP_TRY(launch_mapbuild(p, sl.d_counts.p, d.err.p, sl.stream));
    HIP_TRY(hipMemcpyAsync(hb.h_counts.p, sl.d_counts.p, hb.nvec * sizeof(uint32_t), hipMemcpyDeviceToHost, sl.stream));
    return 0;
}

FLS_ENGINE_END

namespace {

using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// What one call collected: the map's distinct keys, ascending in the key
// order, with their values (stored patterns).
struct Collected {
    std::vector<uint64_t> keys, values;
    bool key_signed = true, value_signed = true;
    double scan_ms = 0, compact_ms = 0;
    Clock::time_point finish_from;
};

// (the text of fls_valuemap_create's conflict: the key as a pattern and as a signed number, the values in their kind)
int conflict_error(const char *who, uint64_t key, uint64_t a, uint64_t b, bool value_signed) {
    if (value_signed)
        return fail(FLS_ERR_ARG, "%s: key 0x%llx (%lld) is listed with the values %lld and %lld: a map is a function", who,
                    (unsigned long long)key, (long long)key, (long long)a, (long long)b);
    return fail(FLS_ERR_ARG, "%s: key 0x%llx (%lld) is listed with the values %llu and %llu: a map is a function", who,
                (unsigned long long)key, (long long)key, (unsigned long long)a, (unsigned long long)b);
}

// Everything both calls share up to the merged pairs: 0 with `c` filled (no
// surviving row group: empty, no device work) or the call's error.
int collect_pairs(fls_table *t, const char *who, const char *what, uint32_t key_col, uint32_t value_col,
                  uint32_t rg_begin, uint32_t rg_end, int form, fls_map_build_info_t *info, Collected &c) {
    if (info) memset(info, 0, sizeof(*info));
    // the refusals, before any device work
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    const uint32_t both[2] = {key_col, value_col};
    for (uint32_t col : both) {
        if (is_mapped_col(col))
            return fail(FLS_ERR_ARG, "%s: a mapped column (FLS_COL_MAPPED, 0x%x) cannot be a map build's column", who, col);
        if (col >= ncols) return fail(FLS_ERR_ARG, "%s: column %u out of range", who, col);
        const ColumnMeta &cm = t->meta.cols[col];
        if (type_is_string(cm.type) || type_is_float(cm.type) || !type_valid(cm.type))
            return fail(FLS_ERR_ARG, "%s: a %s cannot be built from a VARCHAR / BLOB / FLOAT / DOUBLE column (%u)", who,
                        what, col);
        if (cm.type == TY_DECIMAL && cm.width > 18)
            return fail(FLS_ERR_ARG, "%s: a %s cannot be built from a DECIMAL wider than 64 bits (column %u)", who, what,
                        col);
    }
    if (form < 0 || form > 2) return fail(FLS_ERR_ARG, "%s: form %d (0 auto, 1 dense, 2 hash)", who, form);
    {
        const std::string prefix = std::string(who) + ": ";
        if (int rc = check_rowgroup_range(t, rg_begin, rg_end, prefix.c_str())) return rc;
    }
    c.key_signed = type_is_signed(t->meta.cols[key_col].type);
    c.value_signed = type_is_signed(t->meta.cols[value_col].type);
    const auto t0 = Clock::now();
    c.finish_from = t0;
    // the row groups the filter and its alternatives leave, less those whose key or value chunk is all NULL
    std::vector<uint32_t> rgs, keep;
    uint32_t pruned = select_rowgroups(t, t->filter, t->alts, nullptr, 0, rg_begin, rg_end, rgs);
    uint64_t rows = 0;
    for (uint32_t r : rgs) {
        const auto &zs = t->meta.rgs[r].zones;
        if (!zs.empty() && ((zs[key_col].flags | zs[value_col].flags) & ZM_ALL_NULL)) {
            ++pruned;
            continue;
        }
        keep.push_back(r);
        rows += t->meta.rgs[r].nrows;
    }
    rgs.swap(keep);
    if (info) info->rowgroups_pruned = pruned;
    if (rgs.empty()) return 0;  // an empty table or range, or everything pruned: the empty map, no device work
    // the collecting range and its gate
    MapBuildPlan mb;
    mb.key_col = key_col;
    mb.value_col = value_col;
    keybuild_range(t, key_col, rgs, mb.base, mb.span);
    if (!mapbuild_span_ok(mb.span, rows)) {
        const bool fits = mb.span < kValuemapMaxSpan;
        return fail(FLS_ERR_LIMIT, "%s: the zone maps of key column %u span %llu values over the %zu row groups to read "
                    "(at most 2^28, kValuemapMaxSpan); a collecting array over them takes %llu bytes (at most %llu, "
                    "kValuemapSmallDense, or the %llu bytes the hash image of %llu rows takes); build the map from a "
                    "filtered scan on the host", who, key_col, (unsigned long long)mb.span + 1, rgs.size(),
                    (unsigned long long)(fits ? mapbuild_scratch_bytes(mb.span) : 0),
                    (unsigned long long)kValuemapSmallDense,
                    (unsigned long long)valuemap_hash_bytes(keyset_cap_log2(rows)), (unsigned long long)rows);
    }
    // the all-ones pattern in the value order marks an untouched slot: no value may reach it
    const bool wide_value = out_bytes_of(t, value_col) == 8;
    for (uint32_t r : rgs) {
        const auto &zs = t->meta.rgs[r].zones;
        const bool has = !zs.empty() && (zs[value_col].flags & ZM_VALID);
        if (!has) {
            if (!wide_value) continue;  // (a narrower type cannot form the pattern)
            return fail(FLS_ERR_LIMIT, "%s: value column %u is 8 bytes wide and row group %u has no zone map for it: its "
                        "values may reach the pattern the device keeps for an untouched slot; build the map from a "
                        "filtered scan on the host", who, value_col, r);
        }
        if (keyset_ord(zs[value_col].max, c.value_signed) != ~0ull) continue;
        if (c.value_signed)
            return fail(FLS_ERR_LIMIT, "%s: the zone map of value column %u reaches %lld (INT64_MAX) in row group %u, the "
                        "pattern the device keeps for an untouched slot; build the map from a filtered scan on the host",
                        who, value_col, (long long)zs[value_col].max, r);
        return fail(FLS_ERR_LIMIT, "%s: the zone map of value column %u reaches %llu (UINT64_MAX) in row group %u, the "
                    "pattern the device keeps for an untouched slot; build the map from a filtered scan on the host", who,
                    value_col, (unsigned long long)zs[value_col].max, r);
    }
    // one collecting array per GPU that reads a row group, shared by its pipelines: all ones
    const uint32_t G = (uint32_t)t->devices.size(), n = (uint32_t)rgs.size();
    const uint64_t nslots = mb.span + 1, scratch = mapbuild_scratch_bytes(mb.span);
    std::vector<std::unique_ptr<DevBuf<uint64_t>>> bufs;
    mb.slots.assign(G, nullptr);
    for (uint32_t g = 0; g < G; ++g) {
        if ((uint32_t)((uint64_t)n * g / G) >= (uint32_t)((uint64_t)n * (g + 1) / G)) continue;  // scan_setup's shard: empty
        for (auto &b : bufs)
            if (b->dev == t->devices[g]) mb.slots[g] = b->p;
        if (mb.slots[g]) continue;
        HIP_TRY(hipSetDevice(t->devices[g]));
        auto b = std::make_unique<DevBuf<uint64_t>>();
        HIP_TRY(b->alloc(t->devices[g], (size_t)nslots + 3));  // (... and the three conflict cells)
        HIP_TRY(hipMemset(b->p, 0xFF, scratch + 24));
        HIP_TRY(hipStreamSynchronize(nullptr));  // filled before a slot's (non-blocking) stream touches it
        mb.slots[g] = b->p;
        bufs.push_back(std::move(b));
    }
    // the scan: nothing per batch but the counts
    ScanPlan plan;
    plan.rg0 = rg_begin;
    plan.rg1 = rg_end;
    plan.mapbuild = &mb;
    plan.only = &rgs;
    uint64_t selected = 0, d2h = 0;
    const HostBatch *seen = nullptr;
    int rc = reduce_scan(t, plan, "map build", [&](const fls_rowgroup &rg, const HostBatch &hb) {
        const RowGroupMeta &m = t->meta.rgs[rg.rowgroup];
        const uint64_t v0 = (m.first_row - t->meta.rgs[hb.rg0].first_row) / kVectorSize;
        const uint64_t nv = ((uint64_t)m.nrows + kVectorSize - 1) / kVectorSize;
        if (v0 + nv > hb.nvec)
            return fail(FLS_ERR_STATE, "internal: row group %u past its batch's %u vectors", rg.rowgroup, hb.nvec);
        for (uint64_t v = v0; v < v0 + nv; ++v) selected += hb.h_counts.p[v];
        if (&hb != seen) d2h += (uint64_t)hb.nvec * sizeof(uint32_t) + sizeof(uint32_t);  // the counts and the error word
        seen = &hb;
        return 0;
    });
    // every slot's stream has finished (each batch's event was waited for) or
    // the scan failed: wait for what is still enqueued before the arrays go
    for (auto &d : t->scan.devs)
        if (d) d->sync();
    // a conflict: the key from the GPU's cell (the scan's own error says only that there is one)
    for (auto &b : bufs) {
        uint64_t cell[3] = {~0ull, 0, 0};  // d, and the two values in the value order
        if (hipSetDevice(b->dev) != hipSuccess ||
            hipMemcpy(cell, b->p + nslots, sizeof(cell), hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            if (rc) return rc;  // (the scan's error stands)
            return fail(FLS_ERR_DEVICE, "%s: cannot read the conflict cell of GPU %d", who, b->dev);
        }
        d2h += sizeof(cell);
        const uint64_t vflip = c.value_signed ? 1ull << 63 : 0ull;
        if (cell[0] != ~0ull) return conflict_error(who, mb.base + cell[0], cell[1] ^ vflip, cell[2] ^ vflip, c.value_signed);
    }
    if (rc) return rc;
    const auto t1 = Clock::now();
    // the compaction, per GPU: presence words and block counts, the counts'
    // exclusive scan on the host, the present slots' values; the array itself stays
    const uint64_t nw = (nslots + 63) / 64, nb = (nslots + 1023) / 1024;
    std::vector<std::vector<uint64_t>> presence(bufs.size()), values(bufs.size());
    std::vector<MapbuildPart> parts(bufs.size());
    try {
        std::vector<uint32_t> counts(nb);
        std::vector<uint64_t> offsets(nb);
        for (size_t i = 0; i < bufs.size(); ++i) {
            const int dev = bufs[i]->dev;
            HIP_TRY(hipSetDevice(dev));
            DevBuf<uint64_t> d_presence, d_offsets, d_values;
            DevBuf<uint32_t> d_counts;
            HIP_TRY(d_presence.alloc(dev, nw));
            HIP_TRY(d_counts.alloc(dev, nb));
            HIP_TRY(launch_mapbuild_presence(bufs[i]->p, nslots, d_presence.p, d_counts.p, nullptr));
            HIP_TRY(hipMemcpy(counts.data(), d_counts.p, nb * sizeof(uint32_t), hipMemcpyDeviceToHost));
            uint64_t total = 0;
            for (uint64_t k = 0; k < nb; ++k) {
                offsets[k] = total;
                total += counts[k];
            }
            presence[i].resize(nw);
            values[i].resize(total);
            HIP_TRY(hipMemcpy(presence[i].data(), d_presence.p, nw * 8, hipMemcpyDeviceToHost));
            if (total) {
                HIP_TRY(d_offsets.alloc(dev, nb));
                HIP_TRY(d_values.alloc(dev, total));
                HIP_TRY(hipMemcpy(d_offsets.p, offsets.data(), nb * 8, hipMemcpyHostToDevice));
                HIP_TRY(launch_mapbuild_gather(bufs[i]->p, nslots, d_offsets.p, c.value_signed, d_values.p, total, nullptr));
                HIP_TRY(hipMemcpy(values[i].data(), d_values.p, total * 8, hipMemcpyDeviceToHost));
            }
            d2h += nb * sizeof(uint32_t) + nw * 8 + total * 8;
            parts[i].presence = presence[i].data();
            parts[i].values = values[i].data();
            parts[i].n = total;
        }
        bufs.clear();
        const auto t2 = Clock::now();
        c.finish_from = t2;
        c.scan_ms = ms_between(t0, t1);
        c.compact_ms = ms_between(t1, t2);
        MapbuildConflict bad;
        const int mrc = mapbuild_merge(parts, mb.base, mb.span, c.keys, c.values, bad);
        if (mrc == MB_CONFLICT) return conflict_error(who, bad.key, bad.a, bad.b, c.value_signed);
        if (mrc != MB_OK) return fail(FLS_ERR_STATE, "internal: %s: a GPU's presence words and values disagree", who);
    } catch (const std::bad_alloc &) {
        return fail(FLS_ERR_NOMEM, "%s: out of memory", who);
    }
    if (info) {
        info->rows_selected = selected;
        info->keys = c.keys.size();
        info->scratch_bytes = scratch;
        info->d2h_bytes = d2h;
        info->base = mb.base;
        info->span = mb.span;
        info->rowgroups_read = n;
    }
    return 0;
}

void profile_line(const char *what, const Collected &c, const fls_map_build_info_t *info, size_t keys) {
    if (!ScanProf::on()) return;
    fprintf(stderr, "FLS_SCAN_PROFILE %s build: scan %.3f ms, compact + D2H %.3f ms (%llu bytes), host finish %.3f ms "
            "(%zu keys)\n", what, c.scan_ms, c.compact_ms, (unsigned long long)(info ? info->d2h_bytes : 0),
            ms_between(c.finish_from, Clock::now()), keys);
}

}  // namespace

extern "C" {

int fls_valuemap_from_scan(fls_table *t, uint32_t key_col, uint32_t value_col, uint32_t rg_begin, uint32_t rg_end, int form,
                           fls_valuemap **out, fls_map_build_info_t *info) {
    const char *who = "fls_valuemap_from_scan";
    if (!t || !out) return fail(FLS_ERR_ARG, "%s: NULL argument", who);
    *out = nullptr;
    fls_map_build_info_t local;
    if (!info) info = &local;
    Collected c;
    if (int rc = collect_pairs(t, who, "value map", key_col, value_col, rg_begin, rg_end, form, info, c)) return rc;
    auto vm = std::make_shared<ValueMap>();
    vm->conn = t->conn;
    int rc;
    try {
        rc = valuemap_finish_sorted(std::move(c.keys), std::move(c.values), c.key_signed, c.value_signed, (uint32_t)form,
                                    vm->img);
    } catch (const std::bad_alloc &) {
        return fail(FLS_ERR_NOMEM, "%s: out of memory", who);
    }
    if (rc == VM_TOO_WIDE)
        return fail(FLS_ERR_LIMIT, "%s: a dense map over [min, max] would cover more than 2^28 keys", who);
    if (rc != VM_OK) return fail(FLS_ERR_ARG, "%s: cannot build the map (%d)", who, rc);
    profile_line("valuemap", c, info, vm->img.set.keys.size());
    ValueMapRegistry &R = valuemap_registry();
    std::lock_guard<std::mutex> lk(R.mu);
    const uint64_t h = ValueMapRegistry::handle_of(R.next++);
    R.live[h] = std::move(vm);
    *out = (fls_valuemap *)(uintptr_t)h;
    return 0;
}

int fls_keymap_from_scan(fls_table *t, uint32_t key_col, uint32_t value_col, uint32_t rg_begin, uint32_t rg_end, int form,
                         fls_keymap **out, fls_map_build_info_t *info) {
    const char *who = "fls_keymap_from_scan";
    if (!t || !out) return fail(FLS_ERR_ARG, "%s: NULL argument", who);
    *out = nullptr;
    fls_map_build_info_t local;
    if (!info) info = &local;
    Collected c;
    if (int rc = collect_pairs(t, who, "key map", key_col, value_col, rg_begin, rg_end, form, info, c)) return rc;
    auto km = std::make_shared<KeyMap>();
    km->conn = t->conn;
    int rc;
    try {
        // the codes: every value in [0, 65534], then 16 bits wide
        std::vector<uint16_t> codes;
        uint64_t bad = 0;
        if (mapbuild_codes(c.values, c.value_signed, codes, bad) != MB_OK) {
            if (c.value_signed)
                return fail(FLS_ERR_ARG, "%s: value %lld of column %u is outside [0, 65534]", who, (long long)bad, value_col);
            return fail(FLS_ERR_ARG, "%s: value %llu of column %u is outside [0, 65534]", who, (unsigned long long)bad,
                        value_col);
        }
        rc = keymap_finish_sorted(std::move(c.keys), std::move(codes), c.key_signed, (uint32_t)form, km->img);
    } catch (const std::bad_alloc &) {
        return fail(FLS_ERR_NOMEM, "%s: out of memory", who);
    }
    if (rc == KM_TOO_WIDE)
        return fail(FLS_ERR_LIMIT, "%s: a dense map over [min, max] would cover more than 2^31 values", who);
    if (rc != KM_OK) return fail(FLS_ERR_ARG, "%s: cannot build the map (%d)", who, rc);
    profile_line("keymap", c, info, km->img.set.keys.size());
    KeyMapRegistry &R = keymap_registry();
    std::lock_guard<std::mutex> lk(R.mu);
    const uint64_t h = KeyMapRegistry::handle_of(R.next++);
    R.live[h] = std::move(km);
    *out = (fls_keymap *)(uintptr_t)h;
    return 0;
}

}  // extern "C"
