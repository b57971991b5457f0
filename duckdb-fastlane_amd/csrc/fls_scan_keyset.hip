// fls_scan_keyset.hip -- key sets on the host: the registry of live sets and
// fls_keyset_create / free / info / contains (the set's image: fls_keyset.hpp;
// the probe kernel: fls_keyset.hip).  A filter term reaches a set through
// keyset_registry() (to_terms, flsgpu.hip); fls_disconnect drops its
// connection's sets there too.
//
// fls_keyset_from_scan builds a set on the GPU from a filtered scan of the key
// column: the argument checks, the surviving row groups and the collecting
// range their zone maps give, the gate, one zeroed bitmap per GPU, a
// Reduce::KeySet scan (per batch: enqueue_keyset_build, called by fill_batch;
// the kernel: fls_keyset_build.hip), the bitmaps' copies OR-ed on the host and
// keyset_from_bitmap (fls_keyset.hpp).
#include "fls_engine.hpp"

using namespace fls;
using namespace fls::engine;

FLS_ENGINE_BEGIN

KeySetRegistry &keyset_registry() {
    static auto *r = new KeySetRegistry();
    return *r;
}

// The key-set build's part of a batch (called by fill_batch for
// Reduce::KeySet), after the filter's kernels on the slot's mask: the selected,
// valid keys into the GPU's collecting bitmap, and the per-vector counts of
// the rows that set a bit as the batch's only D2H.
int enqueue_keyset_build(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t) {
    HostBatch &hb = *sl.hb;
    const KeyBuildPlan &kb = s.keybuild;
    size_t g = 0;
    while (g < s.devs.size() && s.devs[g].get() != &d) ++g;
    if (g >= kb.bitmaps.size() || !kb.bitmaps[g])
        return fail(FLS_ERR_STATE, "internal: key-set build without a bitmap on GPU %d", d.dev);
    if (rows > 0xFFFFFFFFull) return fail(FLS_ERR_LIMIT, "fls_keyset_from_scan: a batch of more than 2^32 - 1 rows");
    const uint32_t c = kb.col;
    DevKeyBuild p;
    memset(&p, 0, sizeof(p));
    p.col = sl.d_out[c].p;
    p.valid = sl.valid_staged[c] ? sl.d_valid[c].p : nullptr;  // (enqueue_filter staged the filter's and the key's validity)
    p.mask = sl.d_mask.p;
    p.bitmap = kb.bitmaps[g];
    p.base = kb.base;
    p.span = kb.span;
    p.nrows = (uint32_t)rows;
    p.ob = (uint8_t)out_bytes_of(t, c);
    p.sign = type_is_signed(t->meta.cols[c].type) ? 1 : 0;
    p.window = kb.window ? 1 : 0;
    HIP_TRY(hb.h_counts.alloc(hb.nvec));
    HIP_TRY(launch_keyset_build(p, sl.d_counts.p, d.err.p, sl.stream));
    HIP_TRY(hipMemcpyAsync(hb.h_counts.p, sl.d_counts.p, hb.nvec * sizeof(uint32_t), hipMemcpyDeviceToHost, sl.stream));
    return 0;
}

// The collecting range of column c over the row groups rgs, in the set's
// order: the union of their valid zone maps, the physical type's whole range
// where one of them has none.
void keybuild_range(const fls_table *t, uint32_t c, const std::vector<uint32_t> &rgs, uint64_t &base, uint64_t &span) {
    const uint8_t ty = t->meta.cols[c].type;
    const bool sign = type_is_signed(ty);
    const int tb = type_value_bits(ty);
    bool any = false, full = false;
    uint64_t lo = 0, hi = 0;
    for (uint32_t r : rgs) {
        const auto &zs = t->meta.rgs[r].zones;
        if (zs.empty() || !(zs[c].flags & ZM_VALID)) {
            full = true;
            break;
        }
        const uint64_t a = zs[c].min, b = zs[c].max;
        if (!any || keyset_ord(a, sign) < keyset_ord(lo, sign)) lo = a;
        if (!any || keyset_ord(b, sign) > keyset_ord(hi, sign)) hi = b;
        any = true;
    }
    if (full || !any) {
        lo = sign ? ~0ull << (tb - 1) : 0ull;  // (the sign-extended pattern of the type's minimum)
        hi = lo + (tb >= 64 ? ~0ull : (1ull << tb) - 1);
    }
    base = lo;
    span = hi - lo;
}

FLS_ENGINE_END

namespace {

int register_keyset(std::shared_ptr<KeySet> ks, fls_keyset **out) {
    KeySetRegistry &R = keyset_registry();
    std::lock_guard<std::mutex> lk(R.mu);
    const uint64_t h = KeySetRegistry::handle_of(R.next++);
    R.live[h] = std::move(ks);
    *out = (fls_keyset *)(uintptr_t)h;
    return 0;
}

}  // namespace

extern "C" {

int fls_keyset_from_scan(fls_table *t, uint32_t col, uint32_t rg_begin, uint32_t rg_end, int form, fls_keyset **out,
                         fls_keyset_build_info_t *info) {
    using Clock = std::chrono::steady_clock;
    auto ms = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    if (!t || !out) return fail(FLS_ERR_ARG, "fls_keyset_from_scan: NULL argument");
    *out = nullptr;
    if (info) memset(info, 0, sizeof(*info));
    // the refusals, before any device work
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    if (is_mapped_col(col))
        return fail(FLS_ERR_ARG, "fls_keyset_from_scan: a mapped column (FLS_COL_MAPPED) cannot be a key-set build's column");
    if (col >= ncols) return fail(FLS_ERR_ARG, "fls_keyset_from_scan: column %u out of range", col);
    const ColumnMeta &cm = t->meta.cols[col];
    const uint8_t ty = cm.type;
    if (type_is_string(ty) || type_is_float(ty) || !type_valid(ty))
        return fail(FLS_ERR_ARG, "fls_keyset_from_scan: a key set cannot be built from a VARCHAR / BLOB / FLOAT / DOUBLE "
                    "column (%u)", col);
    if (ty == TY_DECIMAL && cm.width > 18)
        return fail(FLS_ERR_ARG, "fls_keyset_from_scan: a key set cannot be built from a DECIMAL wider than 64 bits "
                    "(column %u)", col);
    if (form < 0 || form > 2) return fail(FLS_ERR_ARG, "fls_keyset_from_scan: form %d (0 auto, 1 bitmap, 2 hash)", form);
    if (int rc = check_rowgroup_range(t, rg_begin, rg_end, "fls_keyset_from_scan: ")) return rc;
    const bool sign = type_is_signed(ty);
    const auto t0 = Clock::now();
    // the row groups the filter and its alternatives leave, less those whose key chunk is all NULL
    std::vector<uint32_t> rgs, keep;
    uint32_t pruned = select_rowgroups(t, t->filter, t->alts, nullptr, 0, rg_begin, rg_end, rgs);
    uint64_t rows = 0;
    for (uint32_t r : rgs) {
        const auto &zs = t->meta.rgs[r].zones;
        if (!zs.empty() && (zs[col].flags & ZM_ALL_NULL)) {
            ++pruned;
            continue;
        }
        keep.push_back(r);
        rows += t->meta.rgs[r].nrows;
    }
    rgs.swap(keep);
    auto ks = std::make_shared<KeySet>();
    ks->conn = t->conn;
    if (info) info->rowgroups_pruned = pruned;
    if (rgs.empty()) {  // an empty table or range, or everything pruned: the empty set, no device work
        ks->img.is_signed = sign;
        if (keyset_finish(ks->img, (uint32_t)form) != KS_OK)
            return fail(FLS_ERR_ARG, "fls_keyset_from_scan: cannot build the empty set");
        return register_keyset(std::move(ks), out);
    }
    // the collecting range and its gate
    KeyBuildPlan kb;
    kb.col = col;
    keybuild_range(t, col, rgs, kb.base, kb.span);
    const uint64_t replaced = rows * (uint64_t)out_bytes_of(t, col);
    const uint64_t bitmap_bytes = kb.span < kKeysetMaxSpan ? keyset_bitmap_bytes(kb.span) : 0;
    if (kb.span >= kKeysetMaxSpan || (bitmap_bytes > kKeysetSmallBitmap && bitmap_bytes > replaced))
        return fail(FLS_ERR_LIMIT, "fls_keyset_from_scan: the zone maps of column %u span %llu values over the %zu row "
                    "groups to read (at most 2^32, kKeysetMaxSpan); a bitmap over them takes %llu bytes (at most %llu, "
                    "kKeysetSmallBitmap, or the %llu bytes the selected keys of %llu rows could take); build the set "
                    "from a filtered scan and fls_keyset_create", col, (unsigned long long)kb.span + 1, rgs.size(),
                    (unsigned long long)(kb.span / 64 + 1) * 8, (unsigned long long)kKeysetSmallBitmap,
                    (unsigned long long)replaced, (unsigned long long)rows);
    {
        const char *e = getenv("FLS_KEYSET_BUILD_WINDOW");  // (A/B: 0 sends every row's atomic to HBM)
        kb.window = !(e && *e && atoi(e) == 0);
    }
    // one zeroed bitmap per GPU that reads a row group, shared by its pipelines
    const uint32_t G = (uint32_t)t->devices.size(), n = (uint32_t)rgs.size();
    std::vector<std::unique_ptr<DevBuf<uint32_t>>> bufs;
    kb.bitmaps.assign(G, nullptr);
    const size_t dwords = (size_t)(bitmap_bytes / 4);
    for (uint32_t g = 0; g < G; ++g) {
        if ((uint32_t)((uint64_t)n * g / G) >= (uint32_t)((uint64_t)n * (g + 1) / G)) continue;  // scan_setup's shard: empty
        for (auto &b : bufs)
            if (b->dev == t->devices[g]) kb.bitmaps[g] = b->p;
        if (kb.bitmaps[g]) continue;
        HIP_TRY(hipSetDevice(t->devices[g]));
        auto b = std::make_unique<DevBuf<uint32_t>>();
        HIP_TRY(b->alloc(t->devices[g], dwords));
        HIP_TRY(hipMemset(b->p, 0, bitmap_bytes));
        HIP_TRY(hipStreamSynchronize(nullptr));  // zero before a slot's (non-blocking) stream touches it
        kb.bitmaps[g] = b->p;
        bufs.push_back(std::move(b));
    }
    // the scan: nothing per batch but the counts
    ScanPlan plan;
    plan.rg0 = rg_begin;
    plan.rg1 = rg_end;
    plan.keybuild = &kb;
    plan.only = &rgs;
    uint64_t selected = 0, d2h = 0;
    const HostBatch *seen = nullptr;
    int rc = reduce_scan(t, plan, "key-set build", [&](const fls_rowgroup &rg, const HostBatch &hb) {
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
    // the scan failed: wait for what is still enqueued before the bitmaps go
    for (auto &d : t->scan.devs)
        if (d) d->sync();
    if (rc) return rc;
    const auto t1 = Clock::now();
    // the bitmaps' way back: synchronous copies, OR-ed on the host
    std::vector<uint64_t> words, part;
    try {
        for (auto &b : bufs) {
            std::vector<uint64_t> &dst = words.empty() ? words : part;
            dst.resize((size_t)(bitmap_bytes / 8));
            HIP_TRY(hipSetDevice(b->dev));
            HIP_TRY(hipMemcpy(dst.data(), b->p, bitmap_bytes, hipMemcpyDeviceToHost));
            d2h += bitmap_bytes;
            if (&dst == &part)
                for (size_t i = 0; i < words.size(); ++i) words[i] |= part[i];
        }
    } catch (const std::bad_alloc &) {
        return fail(FLS_ERR_NOMEM, "fls_keyset_from_scan: out of memory");
    }
    bufs.clear();
    const auto t2 = Clock::now();
    int brc;
    try {
        brc = keyset_from_bitmap(words.data(), kb.base, kb.span, sign, (uint32_t)form, ks->img);
    } catch (const std::bad_alloc &) {
        return fail(FLS_ERR_NOMEM, "fls_keyset_from_scan: out of memory");
    }
    if (brc == KS_TOO_MANY)
        return fail(FLS_ERR_LIMIT, "fls_keyset_from_scan: more than %llu distinct keys (kMaxKeysetKeys)",
                    (unsigned long long)kMaxKeysetKeys);
    if (brc == KS_TOO_WIDE)
        return fail(FLS_ERR_LIMIT, "fls_keyset_from_scan: a bitmap over [min, max] would cover more than 2^32 values");
    if (brc != KS_OK) return fail(FLS_ERR_ARG, "fls_keyset_from_scan: cannot build the set (%d)", brc);
    if (info) {
        info->rows_selected = selected;
        info->bitmap_bytes = bitmap_bytes;
        info->d2h_bytes = d2h;
        info->base = kb.base;
        info->span = kb.span;
        info->rowgroups_read = n;
    }
    if (ScanProf::on())
        fprintf(stderr, "FLS_SCAN_PROFILE keyset build: scan %.3f ms, bitmap D2H %.3f ms (%llu bytes), host finish %.3f ms "
                "(%zu keys)\n", ms(t0, t1), ms(t1, t2), (unsigned long long)d2h, ms(t2, Clock::now()), ks->img.keys.size());
    return register_keyset(std::move(ks), out);
}

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
