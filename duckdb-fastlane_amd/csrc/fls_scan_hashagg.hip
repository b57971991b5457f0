// fls_scan_hashagg.hip -- the host half of the hash aggregate pushdown:
// fls_aggregate_hashed (kernels: fls_hashagg.hip).
//
// Per call: the argument checks, the packed key's layout from the zone maps,
// one table in HBM per pipeline (owned by the call, zeroed before the scan
// starts), a reducing scan (reduce_scan) whose batches insert into their
// pipeline's table, then per pipeline the extraction of the occupied slots and
// their D2H, and the merge of the pipelines' groups by packed key.
// Per batch (called by fill_batch for Reduce::HashAggregate): the descriptors
// and the launch on the slot's stream; a batch leaves nothing to copy back but
// the error word.
#include "fls_engine.hpp"

using namespace fls;
using namespace fls::engine;

FLS_ENGINE_BEGIN

int enqueue_hash_aggregate(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo) {
    HostBatch &hb = *sl.hb;
    const bool filtered = s.masked();
    if (!filtered)  // (enqueue_filter staged the filter's, the operands' and the keys' validity together)
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
                            "of its zone maps over the range, the type's width where a row group has none, and 1 for "
                            "NULL); use fls_aggregate_grouped or fewer / narrower keys", q, H.total, kHashKeyBits);
    return 0;
}

}  // namespace

extern "C" {

int fls_aggregate_hashed(fls_table *t, const uint32_t *keys, uint32_t nkeys, const fls_aggregate_spec *aggs, uint32_t n,
                         uint64_t max_groups, uint32_t rg_begin, uint32_t rg_end, fls_hash_result **out) {
    if (!t || !out || (!keys && nkeys) || !aggs) return fail(FLS_ERR_ARG, "fls_aggregate_hashed: NULL argument");
    *out = nullptr;
    if (nkeys == 0 || nkeys > kMaxKeys)
        return fail(FLS_ERR_ARG, "fls_aggregate_hashed: %u keys (1 to %u per call)", nkeys, kMaxKeys);
    if (max_groups == 0 || max_groups > kMaxHashGroups)
        return fail(FLS_ERR_ARG, "fls_aggregate_hashed: max_groups %llu (1 to %llu)", (unsigned long long)max_groups,
                    (unsigned long long)kMaxHashGroups);
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    if (int rc = check_rowgroup_range(t, rg_begin, rg_end, "")) return rc;
    std::vector<uint32_t> hk(keys, keys + nkeys);
    for (uint32_t q = 0; q < nkeys; ++q) {
        const uint32_t c = hk[q];
        if (c & FLS_KEY_MAPPED)
            return fail(FLS_ERR_ARG, "key %u: a mapped key (FLS_KEY_MAPPED) cannot be a hash aggregate's key; "
                        "fls_aggregate_grouped takes it", q);
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
    HashPlan H;
    if (int rc = hash_key_layout(t, hk, rg_begin, rg_end, H)) return rc;
    std::vector<HostAgg> ha;
    if (int rc = check_aggregates(t, "fls_aggregate_hashed", aggs, n, rg_begin, rg_end, ha)) return rc;
    for (uint32_t i = 0; i < n; ++i)
        if (ha[i].fn == AGG_SUM && agg_is_float(t, ha[i]))
            return fail(FLS_ERR_ARG, "aggregate %u: SUM of FLOAT / DOUBLE column %u is order-dependent under atomic "
                        "accumulation and is refused; fls_aggregate_grouped sums it reproducibly", i, ha[i].col);
    // the slots' fields: keys, first rows, then per aggregate what it needs
    std::vector<uint8_t> fop = {F_KEY, F_MAX};
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
    auto res = std::make_unique<fls_hash_result>();
    res->key_values.resize(nkeys);
    res->key_null.resize(nkeys);
    res->aggs.resize(n);
    const uint64_t words = hash_table_words(H.cap, H.nfields);
    res->table_bytes = words * 8;
    // Is there a row group to read?  (scan_setup prunes the same way; without
    // one the scan below does no device work and no table is needed)
    std::vector<uint32_t> rgs;
    select_rowgroups(t, t->filter, nullptr, 0, rg_begin, rg_end, rgs);
    const size_t G = t->devices.size();
    std::vector<DevBuf<uint64_t>> tables(rgs.empty() ? 0 : G);
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
    plan.aggs = &ha;
    plan.keys = &hk;
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
    if (rc) return rc;
    // per pipeline: the occupied slots, compacted on the device, in one D2H
    t0 = Clock::now();
    std::vector<std::vector<uint64_t>> raw(tables.size());
    std::vector<uint64_t> ng(tables.size(), 0);
    for (size_t g = 0; g < tables.size(); ++g) {
        if (g >= s.devs.size() || !s.devs[g] || s.devs[g]->dev != t->devices[g])
            return fail(FLS_ERR_STATE, "internal: hash aggregate pipeline %u not found", (uint32_t)g);
        ScanDev &d = *s.devs[g];
        HIP_TRY(hipSetDevice(d.dev));
        uint64_t hdr[2] = {0, 0};
        HIP_TRY(hipMemcpy(hdr, tables[g].p, sizeof(hdr), hipMemcpyDeviceToHost));
        if (hdr[0] > max_groups)  // (the device flag fails the batch's acquire first)
            return fail(FLS_ERR_LIMIT, "hash aggregate: more than max_groups = %llu distinct keys",
                        (unsigned long long)max_groups);
        ng[g] = hdr[0];
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
    res->extract_ms = ms_since(t0);
    t0 = Clock::now();
    // the pipelines' groups by packed key: a key may straddle a shard boundary
    size_t with = 0, only = 0;
    for (size_t g = 0; g < raw.size(); ++g)
        if (ng[g]) {
            with++;
            only = g;
        }
    const uint32_t nf = H.nfields;
    std::vector<uint64_t> merged;   // field-major like a pipeline's: [f * mg + i]
    uint64_t mg = 0;
    const uint64_t *F = nullptr;
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
    static const uint64_t no_group = 0;
    if (!F) F = &no_group;  // (mg == 0: nothing is read)
    // the fields as the caller sees them
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
        const bool sign = !flt && !is_sum && type_is_signed(t->meta.cols[ha[a].col].type);
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
    res->merge_ms = ms_since(t0);
    *out = res.release();
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
