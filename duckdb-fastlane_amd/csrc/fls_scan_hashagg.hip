// fls_scan_hashagg.hip -- the host half of the hash aggregate pushdown:
// fls_aggregate_hashed and fls_aggregate_hashed_select (kernels: fls_hashagg.hip,
// fls_hashsel.hip).
//
// Per call: the argument checks, the packed key's layout from the zone maps,
// one table in HBM per pipeline (owned by the call, zeroed before the scan
// starts), a reducing scan (reduce_scan) whose batches insert into their
// pipeline's table, then per pipeline the extraction of the occupied slots and
// their D2H, and the merge of the pipelines' groups by packed key.
// Per batch (called by fill_batch for Reduce::HashAggregate): the descriptors
// and the launch on the slot's stream; a batch leaves nothing to copy back but
// the error word.
//
// The two entry points share hash_check, hash_scan and hash_unpack.  With a
// selection (HAVING terms, ORDER BY one aggregate, LIMIT) and ONE pipeline
// holding groups, the groups are chosen where they lie: group_select_kernel,
// the top-k where an order or a limit is set, group_gather_kernel, and only the
// chosen groups are copied and unpacked.  With SEVERAL pipelines holding
// groups a key may straddle shards, so neither HAVING nor the order can be
// decided per pipeline: everything is extracted and merged as in the plain
// call, and the same selection then runs on the host with the kernels' own
// comparators (fls_hashsel.hpp); the result is identical and
// fls_hash_result_select_stats reports on_device = 0.  The plain call never
// touches the selection's kernels.
#include "fls_engine.hpp"
#include "fls_hashsel.hpp"

using namespace fls;
using namespace fls::engine;

FLS_ENGINE_BEGIN

int enqueue_hash_aggregate(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo) {
    HostBatch &hb = *sl.hb;
    const bool filtered = s.masked();
    if (!filtered && s.conds.empty())  // (enqueue_filter, or fill_batch for the conditions, staged every validity together)
        if (int rc = stage_validity(t, s, d, sl, rows, in_lo)) return rc;
    const std::vector<uint8_t> &need = sl.valid_staged;
    const uint32_t na = (uint32_t)s.aggs.size(), nk = (uint32_t)s.keys.size();
    const HashPlan &H = s.hash;
    hb.nvec = (uint32_t)((rows + 1023) / 1024);
    size_t g = 0;  // this pipeline's table
    while (g < s.devs.size() && s.devs[g].get() != &d) ++g;
    if (g >= H.tables.size() || !H.tables[g] || H.fields.size() != na || nk > kMaxKeys)
        return fail(FLS_ERR_STATE, "internal: hash aggregate batch without its pipeline's table");
    if (int rc = upload_agg_descs(t, s, d, sl)) return rc;
    const size_t bytes = hash_desc_bytes();
    HIP_TRY(sl.h_hdesc.alloc(bytes));
    HIP_TRY(sl.d_hdesc.alloc(d.dev, bytes));
    memset(sl.h_hdesc.p, 0, bytes);
    DevHashKey *dk = (DevHashKey *)sl.h_hdesc.p;
    for (uint32_t q = 0; q < nk; ++q) {
        const uint32_t c = s.keys[q];
        if (is_mapped_col(c)) {
            // the derived column mapval_kernel wrote for the key's binding: never
            // NULL (inner), or valid where the map had the value (keep-unmatched);
            // its range is the map's [value_min, value_max]
            const OperandRef o = operand_ref(t, s, sl, c);
            dk[q].col = o.col;
            dk[q].valid = o.valid;
            dk[q].min = H.min[q];
            dk[q].span = H.span[q];
            dk[q].ob = o.ob;
            dk[q].sign = o.kind == FK_INT ? 1 : 0;
            dk[q].shift = (uint8_t)H.shift[q];
            dk[q].null_bit = (uint8_t)H.null_bit[q];
            continue;
        }
        dk[q].col = sl.d_out[c].p;
        dk[q].valid = need[c] ? sl.d_valid[c].p : nullptr;
        dk[q].min = H.min[q];
        dk[q].span = H.span[q];
        dk[q].ob = hb.ob[c];
        dk[q].sign = type_is_signed(t->meta.cols[c].type) ? 1 : 0;
        dk[q].shift = (uint8_t)H.shift[q];
        dk[q].null_bit = (uint8_t)H.null_bit[q];
    }
    memcpy(sl.h_hdesc.p + kMaxKeys * sizeof(DevHashKey), H.fields.data(), na * sizeof(DevHashFields));
    HIP_TRY(hipMemcpyAsync(sl.d_hdesc.p, sl.h_hdesc.p, bytes, hipMemcpyHostToDevice, sl.stream));
    const uint64_t first_row = t->meta.row_offset + t->meta.rgs[sl.rg0].first_row;
    HIP_TRY(launch_hash_insert((const DevHashKey *)sl.d_hdesc.p, nk, sl.d_adesc.p,
                               (const DevHashFields *)(sl.d_hdesc.p + kMaxKeys * sizeof(DevHashKey)), na,
                               (uint32_t)rows, filtered ? sl.d_mask.p : nullptr, first_row, H.tables[g], H.cap,
                               (uint32_t)s.max_groups, H.combine, d.err.p, sl.stream));
    return 0;
}

FLS_ENGINE_END

// The groups of one call: arrays over the groups, in unspecified order.
struct fls_hash_result {
    uint64_t ngroups = 0;
    std::vector<uint64_t> first_rows;
    std::vector<std::vector<uint64_t>> key_values;  // per key
    std::vector<std::vector<uint8_t>> key_null;
    struct Agg {
        std::vector<uint64_t> count, lo, hi;
        std::vector<uint8_t> kind;
    };
    std::vector<Agg> aggs;
    uint64_t table_bytes = 0;  // of one pipeline's table
    double scan_ms = 0, extract_ms = 0, merge_ms = 0;
    // the selection (fls_aggregate_hashed_select): groups formed, groups after HAVING and before LIMIT
    uint64_t groups_total = 0, groups_passed = 0;
    int on_device = 0;
    double select_ms = 0;
};

namespace {

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// How the merge combines a field of two pipelines' slots for one key.
enum FieldOp : uint8_t { F_KEY, F_MAX, F_ADD, F_SUM_LO, F_SUM_HI };

// The layout of the packed key over row groups [rg0, rg1), before pruning:
// key q's range from its zone maps (the type's where a row group has none; an
// all-NULL chunk adds nothing), or FLS_ERR_ARG past 63 bits.
int hash_key_layout(const fls_table *t, const std::vector<uint32_t> &keys, uint32_t rg0, uint32_t rg1, HashPlan &H) {
    const uint32_t nk = (uint32_t)keys.size();
    for (uint32_t q = 0; q < nk; ++q) {
        const uint32_t c = keys[q];
        if (is_mapped_col(c)) {
            // a mapped key: the map's [value_min, value_max] in its value kind's
            // order instead of zone maps (the empty map: one value, 0 bits)
            const ValuemapImage &vi = t->vbindings[mapped_index(c)].map->img;
            H.min[q] = vi.vmin;
            H.span[q] = vi.vmax - vi.vmin;
            H.bits[q] = H.span[q] == 0 ? 0 : 64 - (uint32_t)__builtin_clzll(H.span[q]);
            continue;
        }
        const uint8_t ty = t->meta.cols[c].type;
        const bool sign = type_is_signed(ty);
        const int tb = type_value_bits(ty);
        bool any = false, full = false;
        uint64_t lo = 0, hi = 0;
        for (uint32_t r = rg0; r < rg1 && !full; ++r) {
            const auto &zs = t->meta.rgs[r].zones;
            if (!zs.empty() && (zs[c].flags & ZM_ALL_NULL)) continue;
            if (zs.empty() || !(zs[c].flags & ZM_VALID)) {
                full = true;
                break;
            }
            const uint64_t a = zs[c].min, b = zs[c].max;
            const bool lt = !any || (sign ? (int64_t)a < (int64_t)lo : a < lo);
            const bool gt = !any || (sign ? (int64_t)b > (int64_t)hi : b > hi);
            if (lt) lo = a;
            if (gt) hi = b;
            any = true;
        }
        if (full) {
            lo = sign ? ~0ull << (tb - 1) : 0ull;  // (the sign-extended pattern of the type's minimum)
            hi = lo + (tb >= 64 ? ~0ull : (1ull << tb) - 1);
        }
        H.min[q] = lo;
        H.span[q] = hi - lo;
        H.bits[q] = H.span[q] == 0 ? 0 : 64 - (uint32_t)__builtin_clzll(H.span[q]);
    }
    H.total = 0;
    for (uint32_t q = 0; q < nk; ++q) {
        H.shift[q] = H.total;
        H.total += H.bits[q];
    }
    for (uint32_t q = 0; q < nk; ++q) H.null_bit[q] = H.total++;
    if (H.total > kHashKeyBits)
        for (uint32_t q = 0, bits = nk; q < nk; ++q)
            if ((bits += H.bits[q]) > kHashKeyBits)
                return fail(FLS_ERR_ARG, "key %u: the packed key needs %u bits (at most %u: per key the bits of max - min "
                            "of its zone maps over the range, the type's width where a row group has none, of "
                            "value_max - value_min of a mapped key's map, and 1 for "
                            "NULL); use fls_aggregate_grouped or fewer / narrower keys", q, H.total, kHashKeyBits);
    return 0;
}

// What the two entry points share of one call.
struct HashCall {
    fls_table *t = nullptr;
    uint32_t nkeys = 0, n = 0, rg0 = 0, rg1 = 0;
    uint64_t max_groups = 0;
    std::vector<uint32_t> hk;
    std::vector<HostAgg> ha;
    std::vector<std::vector<HostTerm>> conds;  // the conditions ha[i].cond numbers
    HashPlan H;
    std::vector<uint8_t> fop;               // per field of a slot: how the merge combines it (FieldOp)
    std::vector<DevBuf<uint64_t>> tables;   // per pipeline; none without a row group to read
    std::unique_ptr<fls_hash_result> res;
};

// Part 1: the argument checks, the packed key's layout, the slots' fields and
// an empty result.  No device work.
int hash_check(fls_table *t, const uint32_t *keys, uint32_t nkeys, const fls_aggregate_spec *aggs, uint32_t n,
               uint64_t max_groups, uint32_t rg_begin, uint32_t rg_end, fls_hash_result **out, HashCall &c) {
    if (!t || !out || (!keys && nkeys) || !aggs) return fail(FLS_ERR_ARG, "fls_aggregate_hashed: NULL argument");
    *out = nullptr;
    c.t = t;
    c.nkeys = nkeys;
    c.n = n;
    c.rg0 = rg_begin;
    c.rg1 = rg_end;
    c.max_groups = max_groups;
    HashPlan &H = c.H;
    std::vector<HostAgg> &ha = c.ha;
    std::vector<uint8_t> &fop = c.fop;
    if (nkeys == 0 || nkeys > kMaxKeys)
        return fail(FLS_ERR_ARG, "fls_aggregate_hashed: %u keys (1 to %u per call)", nkeys, kMaxKeys);
    if (max_groups == 0 || max_groups > kMaxHashGroups)
        return fail(FLS_ERR_ARG, "fls_aggregate_hashed: max_groups %llu (1 to %llu)", (unsigned long long)max_groups,
                    (unsigned long long)kMaxHashGroups);
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    if (int rc = check_rowgroup_range(t, rg_begin, rg_end, "")) return rc;
    std::vector<uint32_t> &hk = c.hk;
    hk.assign(keys, keys + nkeys);
    for (uint32_t q = 0; q < nkeys; ++q) {
        const uint32_t c = hk[q];
        if (c & FLS_KEY_MAPPED)
            return fail(FLS_ERR_ARG, "key %u: a mapped key (FLS_KEY_MAPPED) cannot be a hash aggregate's key; "
                        "fls_aggregate_grouped takes it", q);
        if (is_mapped_col(c)) {  // FLS_COL_MAPPED | b: the value binding b's map gives its column
            const uint32_t b = mapped_index(c);
            if (b >= t->vbindings.size())
                return fail(FLS_ERR_ARG, "key %u: no value binding %u (%u set by fls_aggregate_value_bindings)", q, b,
                            (uint32_t)t->vbindings.size());
            for (uint32_t p = 0; p < q; ++p)
                if (keys[p] == c) return fail(FLS_ERR_ARG, "key %u: value binding %u is key %u already", q, b, p);
            continue;
        }
        if (c >= ncols) return fail(FLS_ERR_ARG, "key %u: column %u out of range", q, c);
        for (uint32_t p = 0; p < q; ++p)
            if (keys[p] == c) return fail(FLS_ERR_ARG, "key %u: column %u is key %u already", q, c, p);
        const ColumnMeta &cm = t->meta.cols[c];
        if (cm.type == TY_VARCHAR)
            return fail(FLS_ERR_ARG, "key %u: VARCHAR column %u cannot be a hash aggregate's key (a dictionary code "
                        "means a string of one row group only); fls_aggregate_grouped takes it", q, c);
        if (type_is_float(cm.type) || cm.type == TY_BLOB || !type_valid(cm.type))
            return fail(FLS_ERR_ARG, "key %u: a FLOAT / DOUBLE / BLOB column (%u) cannot be a GROUP BY key", q, c);
        if (cm.type == TY_DECIMAL && cm.width > 18)
            return fail(FLS_ERR_ARG, "key %u: a DECIMAL wider than 64 bits (column %u) cannot be a hash aggregate's key",
                        q, c);
    }
    if (int rc = hash_key_layout(t, hk, rg_begin, rg_end, H)) return rc;
    if (int rc = check_aggregates(t, "fls_aggregate_hashed", aggs, n, rg_begin, rg_end, ha)) return rc;
    used_conditions(t, ha, c.conds);
    for (uint32_t i = 0; i < n; ++i)
        if (ha[i].fn == AGG_SUM && agg_is_float(t, ha[i]))
            return fail(FLS_ERR_ARG, "aggregate %u: SUM of FLOAT / DOUBLE column %u is order-dependent under atomic "
                        "accumulation and is refused; fls_aggregate_grouped sums it reproducibly", i, ha[i].col);
    // the slots' fields: keys, first rows, then per aggregate what it needs
    fop = {F_KEY, F_MAX};
    H.fields.assign(n, DevHashFields{0, 0, 0, 0});
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t fn = ha[i].fn;
        H.fields[i].count = (uint16_t)fop.size();
        fop.push_back(F_ADD);
        if (fn <= AGG_COUNT) continue;
        const bool is_sum = fn == AGG_SUM || fn == AGG_SUM_PRODUCT || fn == AGG_SUM_EXPR;
        H.fields[i].lo = (uint16_t)fop.size();
        fop.push_back(is_sum ? F_SUM_LO : F_MAX);
        if (!is_sum) continue;
        H.fields[i].hi = (uint16_t)fop.size();
        fop.push_back(F_SUM_HI);
    }
    H.nfields = (uint32_t)fop.size();
    H.cap = 2;
    while (H.cap < 2 * max_groups) H.cap <<= 1;
    {   // A/B hook: FLS_HASHAGG_COMBINE=0 issues one set of atomics per row
        const char *e = getenv("FLS_HASHAGG_COMBINE");
        H.combine = e && *e ? atoi(e) != 0 : true;
    }
    c.res = std::make_unique<fls_hash_result>();
    c.res->key_values.resize(nkeys);
    c.res->key_null.resize(nkeys);
    c.res->aggs.resize(n);
    c.res->table_bytes = hash_table_words(H.cap, H.nfields) * 8;
    return 0;
}

// Part 2: the tables, the reducing scan into them, and the drain of its streams.
int hash_scan(HashCall &c) {
    fls_table *t = c.t;
    HashPlan &H = c.H;
    const uint64_t max_groups = c.max_groups;
    const uint32_t rg_begin = c.rg0, rg_end = c.rg1;
    std::vector<DevBuf<uint64_t>> &tables = c.tables;
    fls_hash_result *res = c.res.get();
    const uint64_t words = hash_table_words(H.cap, H.nfields);
    // Is there a row group to read?  (scan_setup prunes the same way; without
    // one the scan below does no device work and no table is needed)
    std::vector<uint32_t> rgs;
    select_rowgroups(t, t->filter, t->alts, nullptr, 0, rg_begin, rg_end, rgs);
    const uint32_t vused = used_value_bindings(c.ha, &c.hk);  // the mapped operands' and keys' bindings
    prune_value_bindings(t, t->vbindings, vused, rgs);
    const size_t G = t->devices.size();
    tables = std::vector<DevBuf<uint64_t>>(rgs.empty() ? 0 : G);
    for (size_t g = 0; g < tables.size(); ++g) {
        hipError_t e = hipSetDevice(t->devices[g]);
        if (e == hipSuccess) e = tables[g].alloc(t->devices[g], words);
        if (e == hipSuccess) e = hipMemsetAsync(tables[g].p, 0, words * 8, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(FLS_ERR_DEVICE, "hash aggregate: no table of %llu bytes (%llu slots of %u fields for max_groups "
                        "%llu) on GPU %d: %s", (unsigned long long)(words * 8), (unsigned long long)H.cap, H.nfields,
                        (unsigned long long)max_groups, t->devices[g], hipGetErrorString(e));
        }
        H.tables.push_back(tables[g].p);
    }
    ScanPlan plan;
    plan.rg0 = rg_begin;
    plan.rg1 = rg_end;
    plan.aggs = &c.ha;
    plan.conds = &c.conds;
    plan.keys = &c.hk;
    plan.vbinds = &t->vbindings;
    plan.vused = vused;
    plan.max_groups = max_groups;
    plan.hash = &H;
    ScanCtx &s = t->scan;
    // the batches leave nothing on the host: a failed one ends the scan through its error word
    auto t0 = Clock::now();
    int rc = reduce_scan(t, plan, "hash aggregate", [](const fls_rowgroup &, const HostBatch &) { return 0; });
    // the tables are the call's: nothing may still insert when they go (or are read)
    if (!tables.empty())
        for (auto &d : s.devs)
            if (d) d->sync();
    res->scan_ms = ms_since(t0);
    return rc;
}

// Pipeline g of the call's scan and the groups its table holds.
int hash_pipeline(HashCall &c, size_t g, ScanDev *&dev, uint64_t &ngroups) {
    fls_table *t = c.t;
    ScanCtx &s = t->scan;
    if (g >= s.devs.size() || !s.devs[g] || s.devs[g]->dev != t->devices[g])
        return fail(FLS_ERR_STATE, "internal: hash aggregate pipeline %u not found", (uint32_t)g);
    ScanDev &d = *s.devs[g];
    HIP_TRY(hipSetDevice(d.dev));
    uint64_t hdr = 0;
    HIP_TRY(hipMemcpy(&hdr, c.tables[g].p, sizeof(hdr), hipMemcpyDeviceToHost));
    if (hdr > c.max_groups)  // (the device flag fails the batch's acquire first)
        return fail(FLS_ERR_LIMIT, "hash aggregate: more than max_groups = %llu distinct keys",
                    (unsigned long long)c.max_groups);
    dev = &d;
    ngroups = hdr;
    return 0;
}

// Per pipeline: the occupied slots, compacted on the device, in one D2H
// (field-major: raw[g][f * ng[g] + i]).
int hash_extract_all(HashCall &c, std::vector<std::vector<uint64_t>> &raw, std::vector<uint64_t> &ng) {
    const HashPlan &H = c.H;
    std::vector<DevBuf<uint64_t>> &tables = c.tables;
    raw.assign(tables.size(), {});
    ng.assign(tables.size(), 0);
    for (size_t g = 0; g < tables.size(); ++g) {
        ScanDev *dp = nullptr;
        if (int rc = hash_pipeline(c, g, dp, ng[g])) return rc;
        ScanDev &d = *dp;
        uint64_t hdr[2] = {0, 0};
        if (ng[g] == 0) continue;
        DevBuf<uint64_t> dense;
        if (dense.alloc(d.dev, ng[g] * H.nfields) != hipSuccess) {
            (void)hipGetLastError();
            return fail(FLS_ERR_DEVICE, "hash aggregate: no buffer of %llu bytes for the groups on GPU %d",
                        (unsigned long long)(ng[g] * H.nfields * 8), d.dev);
        }
        HIP_TRY(launch_hash_extract(tables[g].p, H.cap, H.nfields, dense.p, ng[g], d.stream));
        HIP_TRY(hipStreamSynchronize(d.stream));
        raw[g].resize(ng[g] * H.nfields);
        HIP_TRY(hipMemcpy(raw[g].data(), dense.p, raw[g].size() * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(hdr, tables[g].p, sizeof(hdr), hipMemcpyDeviceToHost));
        if (hdr[1] != ng[g])
            return fail(FLS_ERR_STATE, "internal: hash aggregate extracted %llu of %llu groups",
                        (unsigned long long)hdr[1], (unsigned long long)ng[g]);
    }
    return 0;
}

// The pipelines' groups by packed key -- a key may straddle a shard boundary --
// as one field-major array F[f * mg + i]: a pipeline's own where only one
// holds groups, else `merged`.
void hash_merge(const HashCall &c, std::vector<std::vector<uint64_t>> &raw, const std::vector<uint64_t> &ng,
                std::vector<uint64_t> &merged, const uint64_t *&F, uint64_t &mg) {
    const std::vector<uint8_t> &fop = c.fop;
    const uint32_t nf = c.H.nfields;
    mg = 0;
    F = nullptr;
    size_t with = 0, only = 0;
    for (size_t g = 0; g < raw.size(); ++g)
        if (ng[g]) {
            with++;
            only = g;
        }
    if (with == 1) {
        F = raw[only].data();
        mg = ng[only];
    } else if (with > 1) {
        uint64_t total = 0;
        for (uint64_t x : ng) total += x;
        std::unordered_map<uint64_t, uint64_t> index;
        index.reserve(total);
        std::vector<uint64_t> rows;  // group-major while merging
        rows.reserve(total * nf);
        for (size_t g = 0; g < raw.size(); ++g) {
            const uint64_t *R = raw[g].data();
            for (uint64_t i = 0; i < ng[g]; ++i) {
                auto ins = index.emplace(R[i], index.size());
                if (ins.second) {
                    for (uint32_t f = 0; f < nf; ++f) rows.push_back(R[(uint64_t)f * ng[g] + i]);
                    continue;
                }
                uint64_t *M = rows.data() + ins.first->second * nf;
                for (uint32_t f = 1; f < nf; ++f) {
                    const uint64_t x = R[(uint64_t)f * ng[g] + i];
                    switch (fop[f]) {
                    case F_MAX: M[f] = std::max(M[f], x); break;
                    case F_ADD: M[f] += x; break;
                    case F_SUM_LO: {  // 128 bits with its F_SUM_HI, the next field
                        const uint64_t xh = R[(uint64_t)(f + 1) * ng[g] + i];
                        M[f] += x;
                        M[f + 1] += xh + (M[f] < x ? 1 : 0);
                        break;
                    }
                    default: break;  // F_SUM_HI went with its low word
                    }
                }
            }
            std::vector<uint64_t>().swap(raw[g]);
        }
        mg = index.size();
        merged.resize(mg * nf);
        for (uint64_t i = 0; i < mg; ++i)
            for (uint32_t f = 0; f < nf; ++f) merged[(uint64_t)f * mg + i] = rows[i * nf + f];
        F = merged.data();
    }
}

// Part 3: a field-major array of mg groups (F[f * mg + i]) into the result's
// arrays, the fields as the caller sees them.
void hash_unpack(HashCall &c, const uint64_t *F, uint64_t mg) {
    const fls_table *t = c.t;
    const HashPlan &H = c.H;
    const std::vector<HostAgg> &ha = c.ha;
    const uint32_t nkeys = c.nkeys, n = c.n;
    fls_hash_result *res = c.res.get();
    static const uint64_t no_group = 0;
    if (!F) F = &no_group;  // (mg == 0: nothing is read)
    res->ngroups = mg;
    res->first_rows.resize(mg);
    for (uint64_t i = 0; i < mg; ++i) res->first_rows[i] = ~F[(uint64_t)kHashFieldFirst * mg + i];
    for (uint32_t q = 0; q < nkeys; ++q) {
        std::vector<uint64_t> &kv = res->key_values[q];
        std::vector<uint8_t> &kn = res->key_null[q];
        kv.resize(mg);
        kn.resize(mg);
        const uint64_t fm = H.bits[q] >= 64 ? ~0ull : (1ull << H.bits[q]) - 1;
        for (uint64_t i = 0; i < mg; ++i) {
            const uint64_t pk = F[(uint64_t)kHashFieldKeys * mg + i];
            kn[i] = (uint8_t)((pk >> H.null_bit[q]) & 1);
            // (a signed column's minimum is a sign-extended pattern: the sum is the sign-extended value)
            kv[i] = kn[i] ? 0 : H.min[q] + ((pk >> H.shift[q]) & fm);
        }
    }
    for (uint32_t a = 0; a < n; ++a) {
        fls_hash_result::Agg &A = res->aggs[a];
        const uint8_t fn = ha[a].fn;
        const uint64_t *cnt = F + (uint64_t)H.fields[a].count * mg;
        A.count.assign(cnt, cnt + mg);
        A.lo.assign(mg, 0);
        A.hi.assign(mg, 0);
        A.kind.assign(mg, FLS_AGGV_INT);
        if (fn <= AGG_COUNT) {
            A.lo = A.count;
            continue;
        }
        const uint64_t *lo = F + (uint64_t)H.fields[a].lo * mg;
        const bool is_sum = fn == AGG_SUM || fn == AGG_SUM_PRODUCT || fn == AGG_SUM_EXPR;
        const uint64_t *hi = is_sum ? F + (uint64_t)H.fields[a].hi * mg : nullptr;
        const bool flt = agg_is_float(t, ha[a]);
        const bool sign = !flt && !is_sum && operand_is_signed(t, ha[a].col);  // (a mapped operand: by its map's value kind)
        for (uint64_t i = 0; i < mg; ++i) {
            if (A.count[i] == 0) {
                A.kind[i] = FLS_AGGV_NULL;
                continue;
            }
            if (is_sum) {
                A.lo[i] = lo[i];
                A.hi[i] = hi[i];
                continue;
            }
            const uint64_t key = fn == AGG_MIN ? ~lo[i] : lo[i];
            if (flt) {
                const double v = agg_unkey_float(key);
                memcpy(&A.lo[i], &v, 8);
                A.kind[i] = FLS_AGGV_DOUBLE;
            } else if (sign) {
                const int64_t v = agg_unkey_int(key);
                A.lo[i] = (uint64_t)v;
                A.hi[i] = v < 0 ? ~0ull : 0ull;
            } else {
                A.lo[i] = key;
            }
        }
    }
}

// ---- the selection among the groups (fls_hashsel.hpp)

bool is_sum_fn(uint8_t fn) { return fn == AGG_SUM || fn == AGG_SUM_PRODUCT || fn == AGG_SUM_EXPR; }

// Term `op` against a constant above (side > 0) or below every value the field can hold.
uint8_t out_of_range_mode(uint8_t op, int side) {
    if (op == FLS_CMP_EQ) return HV_NEVER;
    if (op == FLS_CMP_NE) return HV_ALWAYS;
    const bool less = op == FLS_CMP_LT || op == FLS_CMP_LE;
    return (side > 0) == less ? HV_ALWAYS : HV_NEVER;
}

uint8_t mirrored(uint8_t op) {
    switch (op) {
    case FLS_CMP_LT: return FLS_CMP_GT;
    case FLS_CMP_LE: return FLS_CMP_GE;
    case FLS_CMP_GT: return FLS_CMP_LT;
    case FLS_CMP_GE: return FLS_CMP_LE;
    default: return op;
    }
}

// The checks of a fls_group_select and its translation into the fields'
// stored form.  k: the limit (0: none); active: anything is selected at all.
int select_check(const HashCall &c, const fls_group_select *sel, DevGroupSelect &p, uint32_t &k, bool &active) {
    const fls_table *t = c.t;
    memset(&p, 0, sizeof(p));
    k = 0;
    active = false;
    if (!sel) return 0;
    if (sel->nhaving > kMaxHaving)
        return fail(FLS_ERR_ARG, "having %u: %u terms (at most %u per call)", kMaxHaving, sel->nhaving, kMaxHaving);
    if (sel->nhaving && !sel->having) return fail(FLS_ERR_ARG, "having 0: NULL terms");
    for (uint32_t j = 0; j < sel->nhaving; ++j) {
        const fls_group_having &h = sel->having[j];
        if (h.agg >= c.n) return fail(FLS_ERR_ARG, "having %u: aggregate %u out of range (%u aggregates)", j, h.agg, c.n);
        if (h.op > FLS_CMP_GE)
            return fail(FLS_ERR_ARG, "having %u: op %u (FLS_CMP_EQ .. FLS_CMP_GE only)", j, (uint32_t)h.op);
        const HostAgg &a = c.ha[h.agg];
        const DevHashFields &fl = c.H.fields[h.agg];
        const bool minmax = a.fn == AGG_MIN || a.fn == AGG_MAX;
        const bool flt = minmax && agg_is_float(t, a);
        if (h.kind != (flt ? FLS_AGGV_DOUBLE : FLS_AGGV_INT))
            return fail(FLS_ERR_ARG, "having %u: a constant of kind %u against aggregate %u, whose values are of kind "
                        "%s", j, (uint32_t)h.kind, h.agg, flt ? "FLS_AGGV_DOUBLE" : "FLS_AGGV_INT");
        DevHaving &d = p.having[j];
        d.op = h.op;
        d.hi = kNoField;
        const bool neg = (h.hi >> 63) != 0;
        if (a.fn <= AGG_COUNT) {            // an unsigned 64-bit count, never NULL
            d.val = fl.count;
            d.null_cnt = kNoField;
            d.mode = h.hi == 0 ? HV_U64 : out_of_range_mode(h.op, neg ? -1 : 1);
            d.clo = h.lo;
        } else if (is_sum_fn(a.fn)) {       // the 128-bit pair as it is
            d.val = fl.lo;
            d.hi = fl.hi;
            d.null_cnt = fl.count;
            d.mode = HV_S128;
            d.clo = h.lo;
            d.chi = h.hi;
        } else {                            // MAX: the order key; MIN: its complement
            d.val = fl.lo;
            d.null_cnt = fl.count;
            d.mode = HV_U64;
            uint64_t key = 0;
            if (flt) {
                key = agg_key_float(as_double(h.lo));
            } else if (operand_is_signed(t, a.col)) {
                if (h.hi != ((h.lo >> 63) ? ~0ull : 0ull)) d.mode = out_of_range_mode(h.op, neg ? -1 : 1);
                key = agg_key_int((int64_t)h.lo);
            } else {
                if (h.hi != 0) d.mode = out_of_range_mode(h.op, neg ? -1 : 1);
                key = h.lo;
            }
            d.clo = a.fn == AGG_MIN ? ~key : key;
            if (a.fn == AGG_MIN) d.op = mirrored(h.op);
        }
    }
    p.nhaving = sel->nhaving;
    const bool ordered = sel->order_agg != FLS_GROUP_ORDER_NONE;
    if (ordered && sel->order_agg >= c.n)
        return fail(FLS_ERR_ARG, "order: aggregate %u out of range (%u aggregates)", sel->order_agg, c.n);
    if (sel->limit > kMaxGroupLimit)
        return fail(FLS_ERR_ARG, "order: limit %u (at most %u)", sel->limit, kMaxGroupLimit);
    if (ordered && sel->limit == 0)
        return fail(FLS_ERR_ARG, "order: an order needs a limit of 1 to %u (no call sorts all the groups)",
                    kMaxGroupLimit);
    p.oval = p.ohi = p.onull = kNoField;
    p.oform = OF_NONE;
    if (ordered) {
        const HostAgg &a = c.ha[sel->order_agg];
        const DevHashFields &fl = c.H.fields[sel->order_agg];
        if (a.fn <= AGG_COUNT) {
            p.oform = OF_U64;
            p.oval = fl.count;
        } else {
            p.oform = is_sum_fn(a.fn) ? OF_S128 : a.fn == AGG_MIN ? OF_NOT64 : OF_U64;
            p.oval = fl.lo;
            p.ohi = is_sum_fn(a.fn) ? fl.hi : kNoField;
            p.onull = fl.count;
        }
        p.desc = sel->desc ? 1 : 0;
        p.nulls_first = sel->nulls_first ? 1 : 0;
    }
    k = sel->limit;
    p.want_recs = (ordered || k) ? 1 : 0;
    active = p.nhaving || ordered || k;
    return 0;
}

template <class T>
int select_alloc(DevBuf<T> &b, int dev, uint64_t count, const char *what) {
    if (b.alloc(dev, count) == hipSuccess) return 0;
    (void)hipGetLastError();
    return fail(FLS_ERR_DEVICE, "hash aggregate: no buffer of %llu bytes for %s on GPU %d",
                (unsigned long long)(count * sizeof(T)), what, dev);
}

// One pipeline holds the groups: select, top-k, gather on its stream; only
// the chosen groups are copied (chosen[f * nout + i], in result order).
int select_on_device(HashCall &c, size_t g, ScanDev &d, uint64_t ngroups, const DevGroupSelect &p, uint32_t k,
                     std::vector<uint64_t> &chosen, uint64_t &nout, uint64_t &passed, double &select_ms) {
    const HashPlan &H = c.H;
    uint64_t *table = c.tables[g].p;
    auto t0 = Clock::now();
    HIP_TRY(hipSetDevice(d.dev));
    HIP_TRY(hipMemsetAsync(table + kHashHdrSelected, 0, 8, d.stream));
    DevBuf<uint32_t> slots;
    DevBuf<GroupRec> recs, la, lb, best;
    if (p.want_recs) {
        if (int rc = select_alloc(recs, d.dev, ngroups, "the candidates")) return rc;
    } else {
        if (int rc = select_alloc(slots, d.dev, ngroups, "the selected slots")) return rc;
    }
    HIP_TRY(launch_group_select(p, table, H.cap, slots.p, recs.p, ngroups, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    HIP_TRY(hipMemcpy(&passed, table + kHashHdrSelected, 8, hipMemcpyDeviceToHost));
    if (passed > ngroups)
        return fail(FLS_ERR_STATE, "internal: hash aggregate selected %llu of %llu groups", (unsigned long long)passed,
                    (unsigned long long)ngroups);
    nout = passed;
    if (p.want_recs && passed) {
        nout = std::min<uint64_t>(passed, k);
        const uint64_t lists = (passed + 1023) / 1024;
        if (int rc = select_alloc(best, d.dev, nout, "the best groups")) return rc;
        if (lists > 1) {
            if (int rc = select_alloc(la, d.dev, lists * k, "the top-k lists")) return rc;
            if (int rc = select_alloc(lb, d.dev, (lists + 1) / 2 * k, "the top-k lists")) return rc;
        }
        HIP_TRY(launch_group_topk(recs.p, passed, k, la.p, lb.p, best.p, d.stream));
        HIP_TRY(hipStreamSynchronize(d.stream));
    }
    select_ms = ms_since(t0);
    chosen.clear();
    if (nout == 0) return 0;
    DevBuf<uint64_t> dense;
    if (int rc = select_alloc(dense, d.dev, nout * H.nfields, "the groups")) return rc;
    HIP_TRY(launch_group_gather(table, H.cap, H.nfields, p.want_recs ? nullptr : slots.p, best.p, nout, dense.p,
                                d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    chosen.resize(nout * H.nfields);
    HIP_TRY(hipMemcpy(chosen.data(), dense.p, chosen.size() * 8, hipMemcpyDeviceToHost));
    return 0;
}

// Several pipelines hold groups: the same selection over the merged groups
// F[f * mg + i], with the kernels' own comparators (fls_hashsel.hpp).
void select_on_host(const DevGroupSelect &p, uint32_t k, const uint64_t *F, uint64_t mg, uint32_t nf,
                    std::vector<uint64_t> &chosen, uint64_t &nout, uint64_t &passed) {
    std::vector<uint64_t> idx;
    std::vector<GroupRec> recs;
    for (uint64_t i = 0; i < mg; ++i) {
        auto get = [&](uint32_t f) { return F[(uint64_t)f * mg + i]; };
        if (!having_all(p, get)) continue;
        idx.push_back(i);
        if (!p.want_recs) continue;
        GroupRec r;
        order_key(p, get, r);
        r.first = ~get(kHashFieldFirst);
        r.slot = 0;
        recs.push_back(r);
    }
    passed = idx.size();
    nout = passed;
    if (p.want_recs) {
        nout = std::min<uint64_t>(passed, k);
        std::vector<uint64_t> perm(passed);
        for (uint64_t i = 0; i < passed; ++i) perm[i] = i;
        std::partial_sort(perm.begin(), perm.begin() + nout, perm.end(),
                          [&](uint64_t a, uint64_t b) { return rec_less(recs[a], recs[b]); });
        std::vector<uint64_t> best(nout);
        for (uint64_t i = 0; i < nout; ++i) best[i] = idx[perm[i]];
        idx.swap(best);
    }
    chosen.resize(nout * nf);
    for (uint32_t f = 0; f < nf; ++f)
        for (uint64_t i = 0; i < nout; ++i) chosen[(uint64_t)f * nout + i] = F[(uint64_t)f * mg + idx[i]];
}

int hash_aggregate(fls_table *t, const uint32_t *keys, uint32_t nkeys, const fls_aggregate_spec *aggs, uint32_t n,
                   uint64_t max_groups, const fls_group_select *sel, uint32_t rg_begin, uint32_t rg_end,
                   fls_hash_result **out) {
    HashCall c;
    if (int rc = hash_check(t, keys, nkeys, aggs, n, max_groups, rg_begin, rg_end, out, c)) return rc;
    DevGroupSelect p;
    uint32_t k = 0;
    bool active = false;
    if (int rc = select_check(c, sel, p, k, active)) return rc;
    if (int rc = hash_scan(c)) return rc;
    fls_hash_result *res = c.res.get();
    auto t0 = Clock::now();
    std::vector<std::vector<uint64_t>> raw;
    std::vector<uint64_t> ng, chosen;
    uint64_t nout = 0;
    if (active) {   // one pipeline holding groups decides on the device
        std::vector<ScanDev *> devs(c.tables.size(), nullptr);
        ng.assign(c.tables.size(), 0);
        size_t with = 0, only = 0;
        for (size_t g = 0; g < c.tables.size(); ++g) {
            if (int rc = hash_pipeline(c, g, devs[g], ng[g])) return rc;
            if (ng[g]) {
                with++;
                only = g;
            }
        }
        if (with == 1) {
            if (int rc = select_on_device(c, only, *devs[only], ng[only], p, k, chosen, nout, res->groups_passed,
                                          res->select_ms))
                return rc;
            res->groups_total = ng[only];
            res->on_device = 1;
        }
    }
    if (!res->on_device)
        if (int rc = hash_extract_all(c, raw, ng)) return rc;
    res->extract_ms = ms_since(t0);
    t0 = Clock::now();
    if (res->on_device) {
        hash_unpack(c, chosen.data(), nout);
    } else {
        std::vector<uint64_t> merged;
        const uint64_t *F = nullptr;
        uint64_t mg = 0;
        hash_merge(c, raw, ng, merged, F, mg);
        res->groups_total = res->groups_passed = mg;
        if (active && mg) {   // a key may straddle shards: only the merged value decides
            auto ts = Clock::now();
            select_on_host(p, k, F, mg, c.H.nfields, chosen, nout, res->groups_passed);
            res->select_ms = ms_since(ts);
            F = chosen.data();
            mg = nout;
        }
        hash_unpack(c, F, mg);
    }
    res->merge_ms = ms_since(t0);
    *out = c.res.release();
    return 0;
}

}  // namespace

extern "C" {

int fls_aggregate_hashed(fls_table *t, const uint32_t *keys, uint32_t nkeys, const fls_aggregate_spec *aggs, uint32_t n,
                         uint64_t max_groups, uint32_t rg_begin, uint32_t rg_end, fls_hash_result **out) {
    return hash_aggregate(t, keys, nkeys, aggs, n, max_groups, nullptr, rg_begin, rg_end, out);
}

int fls_aggregate_hashed_select(fls_table *t, const uint32_t *keys, uint32_t nkeys, const fls_aggregate_spec *aggs,
                                uint32_t n, uint64_t max_groups, const fls_group_select *sel, uint32_t rg_begin,
                                uint32_t rg_end, fls_hash_result **out) {
    return hash_aggregate(t, keys, nkeys, aggs, n, max_groups, sel, rg_begin, rg_end, out);
}

int fls_hash_result_select_stats(const fls_hash_result *r, uint64_t *groups_total, uint64_t *groups_passed,
                                 int *on_device, double *select_ms) {
    if (!r) return fail(FLS_ERR_ARG, "fls_hash_result_select_stats: NULL argument");
    if (groups_total) *groups_total = r->groups_total;
    if (groups_passed) *groups_passed = r->groups_passed;
    if (on_device) *on_device = r->on_device;
    if (select_ms) *select_ms = r->select_ms;
    return 0;
}

uint64_t fls_hash_result_ngroups(const fls_hash_result *r) { return r ? r->ngroups : 0; }

int fls_hash_result_first_rows(const fls_hash_result *r, const uint64_t **rows) {
    if (!r || !rows) return fail(FLS_ERR_ARG, "fls_hash_result_first_rows: NULL argument");
    *rows = r->first_rows.data();
    return 0;
}

int fls_hash_result_key(const fls_hash_result *r, uint32_t key, const uint64_t **values, const uint8_t **is_null) {
    if (!r || !values || !is_null || key >= r->key_values.size())
        return fail(FLS_ERR_ARG, "fls_hash_result_key: key %u out of range", key);
    *values = r->key_values[key].data();
    *is_null = r->key_null[key].data();
    return 0;
}

int fls_hash_result_aggregate(const fls_hash_result *r, uint32_t agg, const uint64_t **count, const uint64_t **lo,
                              const uint64_t **hi, const uint8_t **kind) {
    if (!r || !count || !lo || !hi || !kind || agg >= r->aggs.size())
        return fail(FLS_ERR_ARG, "fls_hash_result_aggregate: aggregate %u out of range", agg);
    const fls_hash_result::Agg &A = r->aggs[agg];
    *count = A.count.data();
    *lo = A.lo.data();
    *hi = A.hi.data();
    *kind = A.kind.data();
    return 0;
}

int fls_hash_result_stats(const fls_hash_result *r, uint64_t *table_bytes, double *scan_ms, double *extract_ms,
                          double *merge_ms) {
    if (!r) return fail(FLS_ERR_ARG, "fls_hash_result_stats: NULL argument");
    if (table_bytes) *table_bytes = r->table_bytes;
    if (scan_ms) *scan_ms = r->scan_ms;
    if (extract_ms) *extract_ms = r->extract_ms;
    if (merge_ms) *merge_ms = r->merge_ms;
    return 0;
}

void fls_hash_result_free(fls_hash_result *r) { delete r; }

}  // extern "C"
