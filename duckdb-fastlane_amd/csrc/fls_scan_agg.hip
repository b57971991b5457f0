// fls_scan_agg.hip -- the host half of the aggregate pushdowns: fls_aggregate
// and fls_aggregate_grouped (kernels: fls_agg.hip, fls_groupagg.hip).
//
// Per batch (called by fill_batch for Reduce::Aggregate / GroupAggregate):
// the descriptors, the launches and the D2H of the batch's partial results.
// Per call: the argument checks, a reducing scan (reduce_scan) and the fold of
// the partial results in row order.
#include "fls_engine.hpp"

using namespace fls;
using namespace fls::engine;

FLS_ENGINE_BEGIN

// The aggregates of a batch as the kernels see them (sl.h_adesc -> sl.d_adesc
// on the slot's stream), over the slot's decoded columns and staged validity.
int upload_agg_descs(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl) {
    const uint32_t na = (uint32_t)s.aggs.size();
    HIP_TRY(sl.h_adesc.alloc(na));
    HIP_TRY(sl.d_adesc.alloc(d.dev, na));
    uint8_t nfsum = 0;
    for (uint32_t i = 0; i < na; ++i) {
        const HostAgg &a = s.aggs[i];
        DevAgg &da = sl.h_adesc.p[i];
        memset(&da, 0, sizeof(da));
        da.fn = a.fn;
        // (enqueue_conditions wrote the planes: 16 words per vector and condition)
        if (a.cond) da.cond = sl.d_cond.p + (size_t)(a.cond - 1) * 16 * sl.hb->nvec;
        if (a.fn == AGG_COUNT_STAR) continue;
        if (a.fn == AGG_SUM_EXPR) {
            da.nf = (uint8_t)a.nf;
            for (uint32_t k = 0; k < a.nf; ++k) {
                // (a column, or FLS_COL_MAPPED | i: the derived column mapval_kernel wrote)
                const OperandRef o = operand_ref(t, s, sl, a.fcol[k]);
                da.f[k].col = o.col;
                da.f[k].valid = o.valid;
                da.f[k].k = a.fk[k];
                da.fob[k] = o.ob;
                da.fkind[k] = o.kind;
                da.fneg[k] = a.fneg[k];
            }
            continue;
        }
        const OperandRef o = operand_ref(t, s, sl, a.col);
        da.valid = o.valid;
        if (a.fn == AGG_COUNT) continue;
        da.col = o.col;
        da.ob = o.ob;
        da.kind = o.kind;
        if (a.fn == AGG_SUM && da.kind == FK_FLOAT) da.fslot = nfsum++;
        if (a.fn != AGG_SUM_PRODUCT) continue;
        const OperandRef o2 = operand_ref(t, s, sl, a.col2);
        da.col2 = o2.col;
        da.ob2 = o2.ob;
        da.kind2 = o2.kind;
        da.valid2 = o2.valid;
    }
    HIP_TRY(hipMemcpyAsync(sl.d_adesc.p, sl.h_adesc.p, na * sizeof(DevAgg), hipMemcpyHostToDevice, sl.stream));
    return 0;
}

// Aggregate descriptors of a batch and the launch that reduces it: one
// partial record per (vector, aggregate) into sl.d_agg, copied to the host
// batch on the slot's stream.  The selection mask is the filter kernel's
// (enqueue_filter ran before) or none.
int enqueue_aggregate(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo) {
    HostBatch &hb = *sl.hb;
    const bool filtered = s.masked();
    if (!filtered && s.conds.empty())  // (enqueue_filter, or fill_batch for the conditions, staged every validity together)
        if (int rc = stage_validity(t, s, d, sl, rows, in_lo)) return rc;
    const uint32_t na = (uint32_t)s.aggs.size();
    hb.nvec = (uint32_t)((rows + 1023) / 1024);
    HIP_TRY(sl.d_agg.alloc(d.dev, (size_t)hb.nvec * na));
    HIP_TRY(hb.h_agg.alloc((size_t)hb.nvec * na));
    if (int rc = upload_agg_descs(t, s, d, sl)) return rc;
    HIP_TRY(launch_aggregate(sl.d_adesc.p, na, (uint32_t)rows, filtered ? sl.d_mask.p : nullptr, sl.d_agg.p,
                             sl.stream));
    HIP_TRY(hipMemcpyAsync(hb.h_agg.p, sl.d_agg.p, (size_t)hb.nvec * na * sizeof(AggRec), hipMemcpyDeviceToHost,
                           sl.stream));
    return 0;
}

// Bit layout of the packed key of a grouped aggregate (fls_groupagg.hpp): key
// q's value at shift[q] in bits[q] bits -- 8 x the decoded value's bytes, 16
// for a VARCHAR key's dictionary code or a mapped key's code
// (FLS_KEY_MAPPED | i) -- then one NULL bit per key.
struct KeyLayout {
    uint32_t shift[kMaxKeys] = {}, bits[kMaxKeys] = {}, null_bit[kMaxKeys] = {};
    uint32_t total = 0;
};
// The type a key's value has on the host: the column's, or for a mapped key
// the 16-bit code's.
static uint8_t key_type(const fls_table *t, uint32_t key) {
    return key & FLS_KEY_MAPPED ? (uint8_t)TY_UINT16 : t->meta.cols[key].type;
}
static KeyLayout key_layout(const fls_table *t, const std::vector<uint32_t> &keys) {
    KeyLayout L;
    for (size_t q = 0; q < keys.size() && q < kMaxKeys; ++q) {
        const uint8_t ty = key_type(t, keys[q]);
        L.shift[q] = L.total;
        L.bits[q] = type_is_string(ty) ? 16 : (uint32_t)type_value_bits(ty);
        L.total += L.bits[q];
    }
    for (size_t q = 0; q < keys.size() && q < kMaxKeys; ++q) L.null_bit[q] = L.total++;
    return L;
}

// The grouped counterpart of enqueue_aggregate: stage 1 reduces every vector
// per distinct key into sl.d_gvec, stage 2 merges the vectors of each row
// group into sl.d_grg, and the row groups' tables are the batch's only D2H.
int enqueue_group_aggregate(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo) {
    HostBatch &hb = *sl.hb;
    const bool filtered = s.masked();
    if (!filtered && s.conds.empty())  // (enqueue_filter, or fill_batch for the conditions, staged every validity together)
        if (int rc = stage_validity(t, s, d, sl, rows, in_lo)) return rc;
    const std::vector<uint8_t> &need = sl.valid_staged;
    const uint32_t na = (uint32_t)s.aggs.size(), nk = (uint32_t)s.keys.size();
    hb.nvec = (uint32_t)((rows + 1023) / 1024);
    if (int rc = upload_agg_descs(t, s, d, sl)) return rc;
    uint32_t nfsum = 0, rg_vecs = 1;
    for (uint32_t i = 0; i < na; ++i) nfsum += s.aggs[i].fn == AGG_SUM && sl.h_adesc.p[i].kind == FK_FLOAT;
    hb.g_nfsum = nfsum;
    const size_t gd_bytes = kMaxKeys * sizeof(DevKey) + 2ull * sl.nrg * sizeof(uint32_t);
    HIP_TRY(sl.h_gdesc.alloc(gd_bytes));
    HIP_TRY(sl.d_gdesc.alloc(d.dev, gd_bytes));
    memset(sl.h_gdesc.p, 0, gd_bytes);
    DevKey *dk = (DevKey *)sl.h_gdesc.p;
    uint32_t *rgvec = (uint32_t *)(sl.h_gdesc.p + kMaxKeys * sizeof(DevKey));
    const KeyLayout L = key_layout(t, s.keys);
    for (uint32_t q = 0; q < nk; ++q) {
        if (s.keys[q] & FLS_KEY_MAPPED) {
            // the derived column keymap_kernel wrote for binding i of the scan:
            // never NULL (inner), or valid where the map had the value (keep-unmatched)
            const uint32_t i = s.keys[q] & ~FLS_KEY_MAPPED;
            dk[q].col = (const uint8_t *)(sl.d_kcode.p + (size_t)i * 1024 * hb.nvec);
            dk[q].valid = s.binds[i].keep ? sl.d_kvalid.p + (size_t)i * 16 * hb.nvec : nullptr;
            dk[q].ob = 2;
            dk[q].shift = (uint8_t)L.shift[q];
            dk[q].null_bit = (uint8_t)L.null_bit[q];
            continue;
        }
        const uint32_t c = s.keys[q];
        // hb.ob: the decode's bytes per row (a VARCHAR key: its codes' width in this batch)
        if (hb.ob[c] * 8u > L.bits[q])
            return fail(FLS_ERR_STATE, "internal: key column %u decoded %u bytes wide", c, hb.ob[c]);
        dk[q].col = sl.d_out[c].p;
        dk[q].valid = need[c] ? sl.d_valid[c].p : nullptr;
        dk[q].ob = hb.ob[c];
        dk[q].shift = (uint8_t)L.shift[q];
        dk[q].null_bit = (uint8_t)L.null_bit[q];
    }
    if (int rc = rg_vec_table(t, sl, rgvec, rg_vecs)) return rc;
    hb.g_rg_vecs = rg_vecs;
    const size_t rg_stride = group_rg_stride(na, nfsum, rg_vecs);
    HIP_TRY(sl.d_gvec.alloc(d.dev, (size_t)hb.nvec * group_vec_stride(na)));
    HIP_TRY(sl.d_grg.alloc(d.dev, (size_t)sl.nrg * rg_stride));
    HIP_TRY(hb.h_grp.alloc((size_t)sl.nrg * rg_stride));
    HIP_TRY(hipMemcpyAsync(sl.d_gdesc.p, sl.h_gdesc.p, gd_bytes, hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(launch_group_vectors((const DevKey *)sl.d_gdesc.p, nk, sl.d_adesc.p, na, (uint32_t)rows,
                                 filtered ? sl.d_mask.p : nullptr, sl.d_gvec.p, d.err.p, sl.stream));
    HIP_TRY(launch_group_rowgroups(sl.d_adesc.p, na, nfsum,
                                   (const uint32_t *)(sl.d_gdesc.p + kMaxKeys * sizeof(DevKey)), sl.nrg, rg_vecs,
                                   sl.d_gvec.p, sl.d_grg.p, d.err.p, sl.stream));
    HIP_TRY(hipMemcpyAsync(hb.h_grp.p, sl.d_grg.p, (size_t)sl.nrg * rg_stride, hipMemcpyDeviceToHost, sl.stream));
    return 0;
}

FLS_ENGINE_END

namespace {

// Largest magnitude of column c's non-NULL values in row group rg: from the
// zone map, else the type's range.
uint64_t max_magnitude(const fls_table *t, uint32_t rg, uint32_t c) {
    if (is_mapped_col(c)) {  // a mapped operand: max(|value_min|, |value_max|) of its map, 0 for the empty one
        const ValuemapImage &vi = t->vbindings[mapped_index(c)].map->img;
        if (vi.set.keys.empty()) return 0;
        if (!vi.value_signed) return vi.vmax;
        auto mag = [](uint64_t v) { return (int64_t)v < 0 ? 0 - v : v; };
        return std::max(mag(vi.vmin), mag(vi.vmax));
    }
    const uint8_t ty = t->meta.cols[c].type;
    const bool sign = type_is_signed(ty);
    const auto &zs = t->meta.rgs[rg].zones;
    if (!zs.empty() && (zs[c].flags & ZM_ALL_NULL)) return 0;
    if (zs.empty() || !(zs[c].flags & ZM_VALID)) {
        const int bits = type_value_bits(ty);
        return sign ? 1ull << (bits - 1) : (bits == 64 ? ~0ull : (1ull << bits) - 1);
    }
    if (!sign) return std::max(zs[c].min, zs[c].max);
    auto mag = [](uint64_t v) { return (int64_t)v < 0 ? 0 - v : v; };
    return std::max(mag(zs[c].min), mag(zs[c].max));
}

// a * b rounded upwards (a, b >= 0)
double mul_up(double a, double b) { return std::nextafter(a * b, HUGE_VAL); }
// an upper bound of v as a double
double dbl_up(uint64_t v) { return v == 0 ? 0.0 : std::nextafter((double)v, HUGE_VAL); }

// An upper bound, as a double, of |k + s * x| over column c's non-NULL values
// in row group rg (s = -1 when neg): the larger magnitude at the two ends of
// the zone-map range (else the type's range), exact in 128 bits, then rounded
// upwards.  0 for an all-NULL chunk: no row of it contributes.
double max_factor(const fls_table *t, uint32_t rg, uint32_t c, bool neg, int64_t k) {
    auto bound = [&](__int128 lo, __int128 hi) {
        auto mag = [&](__int128 x) {
            const __int128 v = (__int128)k + (neg ? -x : x);
            return (unsigned __int128)(v < 0 ? -v : v);
        };
        const unsigned __int128 m = std::max(mag(lo), mag(hi));  // < 2^65
        return m == 0 ? 0.0 : std::nextafter((double)m, HUGE_VAL);
    };
    if (is_mapped_col(c)) {  // a mapped factor: the ends of its map's [value_min, value_max]; no value in an empty map
        const ValuemapImage &vi = t->vbindings[mapped_index(c)].map->img;
        if (vi.set.keys.empty()) return 0.0;
        if (vi.value_signed) return bound((int64_t)vi.vmin, (int64_t)vi.vmax);
        return bound(vi.vmin, vi.vmax);
    }
    const uint8_t ty = t->meta.cols[c].type;
    const bool sign = type_is_signed(ty);
    const auto &zs = t->meta.rgs[rg].zones;
    if (!zs.empty() && (zs[c].flags & ZM_ALL_NULL)) return 0.0;
    __int128 lo, hi;
    if (zs.empty() || !(zs[c].flags & ZM_VALID)) {
        const int bits = type_value_bits(ty);
        lo = sign ? -((__int128)1 << (bits - 1)) : 0;
        hi = sign ? ((__int128)1 << (bits - 1)) - 1 : ((__int128)1 << bits) - 1;
    } else if (sign) {
        lo = (int64_t)zs[c].min;
        hi = (int64_t)zs[c].max;
    } else {
        lo = zs[c].min;
        hi = zs[c].max;
    }
    return bound(lo, hi);
}

}  // namespace

FLS_ENGINE_BEGIN

// The argument checks fls_aggregate, fls_aggregate_grouped and
// fls_aggregate_hashed (`who`) share: the aggregates into ha, or FLS_ERR_ARG
// before any device work.
int check_aggregates(const fls_table *t, const char *who, const fls_aggregate_spec *aggs, uint32_t n,
                     uint32_t rg_begin, uint32_t rg_end, std::vector<HostAgg> &ha) {
    if (n == 0 || n > kMaxAggs) return fail(FLS_ERR_ARG, "%s: %u aggregates (1 to %u per call)", who, n, kMaxAggs);
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    if (int rc = check_rowgroup_range(t, rg_begin, rg_end, "")) return rc;
    ha.assign(n, HostAgg());
    for (uint32_t i = 0; i < n; ++i) {
        const fls_aggregate_spec &a = aggs[i];
        if (a.fn > FLS_AGG_SUM_EXPR) return fail(FLS_ERR_ARG, "aggregate %u: unknown function %u", i, a.fn);
        ha[i].fn = a.fn;
        if (a.cond > t->conds.size())
            return fail(FLS_ERR_ARG, "aggregate %u: condition %u out of range (%u set by fls_aggregate_conditions)", i,
                        a.cond - 1, (uint32_t)t->conds.size());
        ha[i].cond = a.cond;
        if (a.fn == FLS_AGG_COUNT_STAR) continue;
        if (a.fn == FLS_AGG_SUM_EXPR) {  // (fls_aggregate_exprs checked the factors)
            if (a.col >= t->exprs.size())
                return fail(FLS_ERR_ARG, "aggregate %u: expression %u out of range (%u set by fls_aggregate_exprs)", i,
                            a.col, (uint32_t)t->exprs.size());
            const fls_agg_expr &e = t->exprs[a.col];
            ha[i].nf = e.nfactors;
            for (uint32_t k = 0; k < e.nfactors; ++k) {
                // (the bindings may have been replaced since fls_aggregate_exprs checked the factor)
                if (is_mapped_col(e.f[k].col) && mapped_index(e.f[k].col) >= t->vbindings.size())
                    return fail(FLS_ERR_ARG, "aggregate %u: expression %u names value binding %u (%u set by "
                                "fls_aggregate_value_bindings)", i, a.col, mapped_index(e.f[k].col),
                                (uint32_t)t->vbindings.size());
                ha[i].fcol[k] = e.f[k].col;
                ha[i].fneg[k] = e.f[k].sign < 0;
                ha[i].fk[k] = e.f[k].k;
            }
            continue;
        }
        // an operand: a column, or FLS_COL_MAPPED | b for value binding b, a 64-bit integer column
        auto mapped_ok = [&](uint32_t c) {
            return mapped_index(c) < t->vbindings.size()
                       ? 0
                       : fail(FLS_ERR_ARG, "aggregate %u: no value binding %u (%u set by fls_aggregate_value_bindings)", i,
                              mapped_index(c), (uint32_t)t->vbindings.size());
        };
        if (is_mapped_col(a.col)) {
            if (int rc = mapped_ok(a.col)) return rc;
        } else if (a.col >= ncols) {
            return fail(FLS_ERR_ARG, "aggregate %u: column %u out of range", i, a.col);
        }
        ha[i].col = a.col;
        if (a.fn == FLS_AGG_COUNT) continue;
        const uint8_t ty = is_mapped_col(a.col) ? (uint8_t)TY_INT64 : t->meta.cols[a.col].type;
        if (type_is_string(ty))
            return fail(FLS_ERR_ARG, "aggregate %u: SUM / MIN / MAX of string column %u is not supported", i, a.col);
        if (a.fn != FLS_AGG_SUM_PRODUCT) continue;
        if (is_mapped_col(a.col2)) {
            if (int rc = mapped_ok(a.col2)) return rc;
        } else if (a.col2 >= ncols) {
            return fail(FLS_ERR_ARG, "aggregate %u: column %u out of range", i, a.col2);
        }
        ha[i].col2 = a.col2;
        const uint8_t ty2 = is_mapped_col(a.col2) ? (uint8_t)TY_INT64 : t->meta.cols[a.col2].type;
        if (type_is_string(ty2))
            return fail(FLS_ERR_ARG, "aggregate %u: SUM_PRODUCT of string column %u is not supported", i, a.col2);
        if (type_is_float(ty) || type_is_float(ty2))
            return fail(FLS_ERR_ARG, "aggregate %u: SUM_PRODUCT of a FLOAT / DOUBLE column is not supported", i);
    }
    // SUM_PRODUCT must stay below 2^127: bound it over the row groups the scan
    // will read (rounded upwards) before anything is decoded
    for (uint32_t i = 0; i < n; ++i) {
        if (ha[i].fn == AGG_SUM_EXPR) {
            // the same bound with max|k + s * x| per factor, which an affine
            // term takes at an end of the column's range
            double bound = 0;
            for (uint32_t r = rg_begin; r < rg_end; ++r) {
                if (!rowgroup_may_match(t, r, t->filter, t->alts)) continue;
                double term = dbl_up(t->meta.rgs[r].nrows);
                for (uint32_t k = 0; k < ha[i].nf; ++k)
                    term = mul_up(term, max_factor(t, r, ha[i].fcol[k], ha[i].fneg[k], ha[i].fk[k]));
                bound = std::nextafter(bound + term, HUGE_VAL);
            }
            if (bound >= 0x1p127)
                return fail(FLS_ERR_ARG, "aggregate %u: SUM_EXPR of expression %u may overflow 128 bits", i, aggs[i].col);
            continue;
        }
        if (ha[i].fn != AGG_SUM_PRODUCT) continue;
        double bound = 0;
        for (uint32_t r = rg_begin; r < rg_end; ++r) {
            if (!rowgroup_may_match(t, r, t->filter, t->alts)) continue;
            const double term = mul_up(mul_up(dbl_up(t->meta.rgs[r].nrows), dbl_up(max_magnitude(t, r, ha[i].col))),
                                       dbl_up(max_magnitude(t, r, ha[i].col2)));
            bound = std::nextafter(bound + term, HUGE_VAL);
        }
        if (bound >= 0x1p127)
            return fail(FLS_ERR_ARG, "aggregate %u: SUM_PRODUCT of columns %u and %u may overflow 128 bits", i, ha[i].col,
                        ha[i].col2);
    }
    return 0;
}

void used_conditions(const fls_table *t, std::vector<HostAgg> &ha, std::vector<std::vector<HostTerm>> &used) {
    std::vector<uint32_t> at(t->conds.size(), 0);  // 1 + the condition's place in `used`
    used.clear();
    for (HostAgg &h : ha) {
        if (!h.cond) continue;
        uint32_t &p = at[h.cond - 1];
        if (!p) {
            used.push_back(t->conds[h.cond - 1]);
            p = (uint32_t)used.size();
        }
        h.cond = p;
    }
}

bool agg_is_float(const fls_table *t, const HostAgg &h) {
    return h.fn >= AGG_SUM && h.fn != AGG_SUM_EXPR && operand_is_float(t, h.col);
}

FLS_ENGINE_END

namespace {

// The running value of one aggregate (of one group) on the host.
struct AggAcc {
    uint64_t count = 0;
    unsigned __int128 sum = 0;
    double fsum = -0.0;
    uint64_t key = 0;
    explicit AggAcc(uint8_t fn = 0) : key(fn == AGG_MIN ? ~0ull : 0ull) {}
};

// The grouped fold's addition of a vector's partial binary64 sum onto the
// running sum.  It differs from acc + x only in which NaN comes back when both
// are NaN: the partial's, which is what fls_aggregate's `fsum += x` returns as
// built (x86 keeps its first operand's NaN, and that is the record); the
// one-group test compares the two calls' NaN bits
// (tests/test_group_aggregate.py).  fold_record keeps the plain expression.
inline double add_partial(double acc, double x) { return x != x ? x : acc + x; }

// One partial record into the running value; the records come in row order.
void fold_record(AggAcc &a, uint8_t fn, bool flt, const AggRec &r) {
    a.count += r.count;
    if (r.count == 0) return;
    switch (fn) {
    case AGG_SUM:
    case AGG_SUM_PRODUCT:
    case AGG_SUM_EXPR:
        if (flt) a.fsum += as_double(r.lo);
        else a.sum += ((unsigned __int128)r.hi << 64) | r.lo;
        break;
    case AGG_MIN: a.key = std::min(a.key, r.lo); break;
    case AGG_MAX: a.key = std::max(a.key, r.lo); break;
    default: break;
    }
}

// The running value as the caller sees it.
void finish_value(const fls_table *t, const HostAgg &h, const AggAcc &a, fls_aggregate_value &o) {
    memset(&o, 0, sizeof(o));
    o.count = a.count;
    if (h.fn <= AGG_COUNT) {
        o.kind = FLS_AGGV_INT;
        o.lo = a.count;
        return;
    }
    if (a.count == 0) return;  // FLS_AGGV_NULL
    const bool flt = agg_is_float(t, h);
    o.kind = flt ? FLS_AGGV_DOUBLE : FLS_AGGV_INT;
    if (h.fn == AGG_SUM || h.fn == AGG_SUM_PRODUCT || h.fn == AGG_SUM_EXPR) {
        if (flt) {
            memcpy(&o.lo, &a.fsum, 8);
        } else {
            o.lo = (uint64_t)a.sum;
            o.hi = (uint64_t)(a.sum >> 64);
        }
    } else if (flt) {
        const double d = agg_unkey_float(a.key);
        memcpy(&o.lo, &d, 8);
    } else if (operand_is_signed(t, h.col)) {  // (a mapped operand: by its map's value kind)
        const int64_t v = agg_unkey_int(a.key);
        o.lo = (uint64_t)v;
        o.hi = v < 0 ? ~0ull : 0ull;
    } else {
        o.lo = a.key;
    }
}

}  // namespace

// One group's key values and running aggregates; the strings are copies.
struct fls_group_result {
    struct Key {
        uint8_t kind = FLS_KEYV_NULL;
        uint64_t lo = 0, hi = 0;
        std::string str;
    };
    uint32_t nkeys = 0, naggs = 0;
    std::vector<Key> keys;                    // ngroups x nkeys
    std::vector<fls_aggregate_value> values;  // ngroups x naggs
};

extern "C" {

int fls_aggregate_exprs(fls_table *t, const fls_agg_expr *exprs, uint32_t n) {
    if (!t || (!exprs && n)) return fail(FLS_ERR_ARG, "fls_aggregate_exprs: NULL argument");
    if (n > kMaxAggs) return fail(FLS_ERR_ARG, "fls_aggregate_exprs: %u expressions (at most %u)", n, kMaxAggs);
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    for (uint32_t i = 0; i < n; ++i) {
        const fls_agg_expr &e = exprs[i];
        if (e.nfactors == 0 || e.nfactors > kMaxFactors)
            return fail(FLS_ERR_ARG, "expression %u: %u factors (1 to %u)", i, e.nfactors, kMaxFactors);
        for (uint32_t k = 0; k < e.nfactors; ++k) {
            const fls_agg_factor &f = e.f[k];
            if (f.sign != 1 && f.sign != -1)
                return fail(FLS_ERR_ARG, "expression %u: factor %u has sign %d (+1 or -1)", i, k, (int)f.sign);
            if (is_mapped_col(f.col)) {  // FLS_COL_MAPPED | b: a 64-bit integer column, k in the map's value unit
                if (mapped_index(f.col) >= t->vbindings.size())
                    return fail(FLS_ERR_ARG, "expression %u: no value binding %u (%u set by "
                                "fls_aggregate_value_bindings)", i, mapped_index(f.col), (uint32_t)t->vbindings.size());
                continue;
            }
            if (f.col >= ncols) return fail(FLS_ERR_ARG, "expression %u: column %u out of range", i, f.col);
            const uint8_t ty = t->meta.cols[f.col].type;
            if (type_is_string(ty) || type_is_float(ty))
                return fail(FLS_ERR_ARG, "expression %u: a VARCHAR / BLOB / FLOAT / DOUBLE column (%u) cannot be a factor",
                            i, f.col);
        }
    }
    t->exprs.assign(exprs, exprs + n);
    return 0;
}

int fls_aggregate(fls_table *t, const fls_aggregate_spec *aggs, uint32_t n, uint32_t rg_begin, uint32_t rg_end,
                  fls_aggregate_value *out) {
    if (!t || !aggs || !out) return fail(FLS_ERR_ARG, "fls_aggregate: NULL argument");
    std::vector<HostAgg> ha;
    if (int rc = check_aggregates(t, "fls_aggregate", aggs, n, rg_begin, rg_end, ha)) return rc;
    std::vector<std::vector<HostTerm>> conds;
    used_conditions(t, ha, conds);
    ScanPlan plan;
    plan.rg0 = rg_begin;
    plan.rg1 = rg_end;
    plan.aggs = &ha;
    plan.conds = &conds;
    plan.vbinds = &t->vbindings;
    plan.vused = used_value_bindings(ha, nullptr);
    // fold the per-vector records in row order
    std::vector<AggAcc> acc;
    for (uint32_t i = 0; i < n; ++i) acc.emplace_back(ha[i].fn);
    const int rc = reduce_scan(t, plan, "aggregate", [&](const fls_rowgroup &rg, const HostBatch &hb) {
        const uint64_t v0 = (t->meta.rgs[rg.rowgroup].first_row - t->meta.rgs[hb.rg0].first_row) / kVectorSize;
        const uint64_t nv = (t->meta.rgs[rg.rowgroup].nrows + kVectorSize - 1) / kVectorSize;
        for (uint64_t v = v0; v < v0 + nv && v < hb.nvec; ++v)
            for (uint32_t i = 0; i < n; ++i) fold_record(acc[i], ha[i].fn, agg_is_float(t, ha[i]), hb.h_agg.p[v * n + i]);
        return 0;
    });
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i) finish_value(t, ha[i], acc[i], out[i]);
    return 0;
}

int fls_aggregate_grouped(fls_table *t, const uint32_t *keys, uint32_t nkeys, const fls_aggregate_spec *aggs,
                          uint32_t n, uint32_t rg_begin, uint32_t rg_end, fls_group_result **out) {
    if (!t || !out || (!keys && nkeys) || !aggs) return fail(FLS_ERR_ARG, "fls_aggregate_grouped: NULL argument");
    *out = nullptr;
    if (nkeys == 0 || nkeys > kMaxKeys)
        return fail(FLS_ERR_ARG, "fls_aggregate_grouped: %u keys (1 to %u per call)", nkeys, kMaxKeys);
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    if (int rc = check_rowgroup_range(t, rg_begin, rg_end, "")) return rc;
    // hk[q]: the key's column, or FLS_KEY_MAPPED | its position in `binds`,
    // the bindings this call's keys name
    std::vector<uint32_t> hk(keys, keys + nkeys);
    std::vector<HostBinding> binds;
    for (uint32_t q = 0; q < nkeys; ++q) {
        const uint32_t c = hk[q];
        if (c & FLS_KEY_MAPPED) {
            const uint32_t i = c & ~FLS_KEY_MAPPED;
            if (i >= t->bindings.size())
                return fail(FLS_ERR_ARG, "key %u: no binding %u (%u set by fls_aggregate_key_bindings)", q, i,
                            (uint32_t)t->bindings.size());
            for (uint32_t p = 0; p < q; ++p)
                if (keys[p] == c) return fail(FLS_ERR_ARG, "key %u: binding %u is key %u already", q, i, p);
            hk[q] = FLS_KEY_MAPPED | (uint32_t)binds.size();
            binds.push_back(t->bindings[i]);
            continue;
        }
        if (is_mapped_col(c))
            return fail(FLS_ERR_ARG, "key %u: a mapped column (FLS_COL_MAPPED) cannot be a grouped aggregate's key; a key "
                        "map (FLS_KEY_MAPPED, fls_aggregate_key_bindings) gives a low-cardinality mapped key, "
                        "fls_aggregate_hashed takes a mapped column", q);
        if (c >= ncols) return fail(FLS_ERR_ARG, "key %u: column %u out of range", q, c);
        for (uint32_t p = 0; p < q; ++p)
            if (keys[p] == c) return fail(FLS_ERR_ARG, "key %u: column %u is key %u already", q, c, p);
        const uint8_t ty = t->meta.cols[c].type;
        if (type_is_float(ty) || ty == TY_BLOB)
            return fail(FLS_ERR_ARG, "key %u: a FLOAT / DOUBLE / BLOB column (%u) cannot be a GROUP BY key", q, c);
        if (ty != TY_VARCHAR) continue;
        for (const HostTerm &h : t->filter)
            if (h.col == c)
                return fail(FLS_ERR_ARG,
                            "key %u: VARCHAR column %u is read by a filter term, which needs it decoded as strings, "
                            "not as the dictionary codes a key is made of", q, c);
        for (size_t a = 0; a < t->alts.size(); ++a)
            for (const HostTerm &h : t->alts[a])
                if (h.col == c || (is_col_op(h.op) && h.col2 == c))
                    return fail(FLS_ERR_ARG,
                                "key %u: VARCHAR column %u is read by a term of alternative %u, which needs it decoded "
                                "as strings, not as the dictionary codes a key is made of", q, c, (uint32_t)a);
        // the row groups the scan will read (the same set the SUM_PRODUCT bound walks)
        for (uint32_t r = rg_begin; r < rg_end; ++r) {
            if (!rowgroup_may_match(t, r, t->filter, t->alts)) continue;
            const ChunkHeader &h = t->meta.rgs[r].chunks[c].hdr;
            if (h.enc != ENC_DICT)
                return fail(FLS_ERR_ARG, "key %u: VARCHAR column %u is not dictionary-encoded in row group %u", q, c, r);
            if (h.dict_count > 65536)
                return fail(FLS_ERR_ARG, "key %u: the dictionary of VARCHAR column %u has %u entries in row group %u "
                            "(at most 65536)", q, c, h.dict_count, r);
        }
    }
    const KeyLayout L = key_layout(t, hk);
    if (L.total > 128)
        for (uint32_t q = 0, bits = nkeys; q < nkeys; ++q)
            if ((bits += L.bits[q]) > 128)
                return fail(FLS_ERR_ARG, "key %u: the packed key needs %u bits (at most 128: 8 x value bytes per integer "
                            "key, 16 per VARCHAR or mapped key, 1 per key for NULL)", q, L.total);
    std::vector<HostAgg> ha;
    if (int rc = check_aggregates(t, "fls_aggregate_grouped", aggs, n, rg_begin, rg_end, ha)) return rc;
    std::vector<std::vector<HostTerm>> conds;
    used_conditions(t, ha, conds);
    // (the filter's rule above: a condition's term needs the column decoded as strings)
    for (uint32_t q = 0; q < nkeys; ++q) {
        if ((hk[q] & FLS_KEY_MAPPED) || t->meta.cols[hk[q]].type != TY_VARCHAR) continue;
        for (uint32_t i = 0; i < n; ++i) {
            if (!ha[i].cond) continue;
            for (const HostTerm &h : conds[ha[i].cond - 1])
                if (h.col == hk[q])
                    return fail(FLS_ERR_ARG,
                                "key %u: VARCHAR column %u is read by a term of condition %u, which needs it decoded as "
                                "strings, not as the dictionary codes a key is made of", q, hk[q], aggs[i].cond - 1);
        }
    }
    ScanPlan plan;
    plan.rg0 = rg_begin;
    plan.rg1 = rg_end;
    plan.aggs = &ha;
    plan.conds = &conds;
    plan.keys = &hk;
    plan.binds = &binds;
    plan.vbinds = &t->vbindings;
    plan.vused = used_value_bindings(ha, nullptr);
    auto res = std::make_unique<fls_group_result>();
    res->nkeys = nkeys;
    res->naggs = n;
    // the table's groups in first-occurrence order, found by key VALUE: per key
    // its kind, then the integer's 16 bytes or the string's length and bytes
    std::unordered_map<std::string, uint64_t> index;
    std::vector<AggAcc> acc;  // ngroups x n
    std::vector<uint32_t> fslot(n, 0);  // the FLOAT / DOUBLE sums, numbered as upload_agg_descs numbers them
    for (uint32_t i = 0, k = 0; i < n; ++i)
        if (ha[i].fn == AGG_SUM && agg_is_float(t, ha[i])) fslot[i] = k++;
    std::vector<fls_group_result::Key> kv(nkeys);
    std::string ser;
    const int rc = reduce_scan(t, plan, "aggregate", [&](const fls_rowgroup &rg, const HostBatch &hb) {
        const uint32_t nfsum = hb.g_nfsum, rg_vecs = hb.g_rg_vecs;
        const uint8_t *base = hb.h_grp.p + (size_t)(rg.rowgroup - hb.rg0) * group_rg_stride(n, nfsum, rg_vecs);
        GroupHdr hdr;
        memcpy(&hdr, base, sizeof(hdr));
        if (hdr.overflow || hdr.ngroups > kMaxRgGroups)  // (the device flag fails the batch's acquire first)
            return fail(FLS_ERR_LIMIT, "grouped aggregate: row group %u exceeds the group capacity; fall back to a scan",
                        rg.rowgroup);
        const uint64_t *gkeys = (const uint64_t *)(base + sizeof(GroupHdr));
        const AggRec *recs = (const AggRec *)(base + group_rg_recs_off());
        const double *fvec = (const double *)(base + group_rg_fvec_off(n));
        const uint32_t nv = (t->meta.rgs[rg.rowgroup].nrows + kVectorSize - 1) / kVectorSize;
        for (uint32_t g = 0; g < hdr.ngroups; ++g) {
            const unsigned __int128 pk = ((unsigned __int128)gkeys[2 * g + 1] << 64) | gkeys[2 * g];
            ser.clear();
            for (uint32_t q = 0; q < nkeys; ++q) {
                fls_group_result::Key &k = kv[q];
                k = fls_group_result::Key();
                const uint8_t ty = key_type(t, hk[q]);  // (a mapped key is an integer: its code)
                if (!((pk >> L.null_bit[q]) & 1)) {
                    const uint64_t raw = (uint64_t)(pk >> L.shift[q]) & (L.bits[q] >= 64 ? ~0ull : (1ull << L.bits[q]) - 1);
                    if (ty == TY_VARCHAR) {
                        // the code through this row group's dictionary in the file image
                        const ChunkRef &ch = t->meta.rgs[rg.rowgroup].chunks[hk[q]];
                        if (raw >= ch.hdr.dict_count)
                            return fail(FLS_ERR_FORMAT, "corrupt chunk: dictionary code %llu of %u in key column %u",
                                        (unsigned long long)raw, ch.hdr.dict_count, hk[q]);
                        const uint8_t *p;
                        uint32_t len;
                        dict_string(t->img + ch.off + ch.hdr.aux_off, ch.hdr.dict_count, (uint32_t)raw, p, len);
                        k.kind = FLS_KEYV_STRING;
                        k.str.assign((const char *)p, len);
                    } else {
                        k.kind = FLS_KEYV_INT;
                        k.lo = raw;
                        if (type_is_signed(ty) && L.bits[q] < 64 && ((raw >> (L.bits[q] - 1)) & 1)) k.lo |= ~0ull << L.bits[q];
                        k.hi = type_is_signed(ty) && (int64_t)k.lo < 0 ? ~0ull : 0ull;
                    }
                }
                ser.push_back((char)k.kind);
                if (k.kind == FLS_KEYV_INT) {
                    ser.append((const char *)&k.lo, 8);
                } else if (k.kind == FLS_KEYV_STRING) {
                    const uint64_t len = k.str.size();
                    ser.append((const char *)&len, 8);
                    ser.append(k.str);
                }
            }
            auto it = index.find(ser);
            uint64_t gi;
            if (it == index.end()) {
                gi = index.size();
                index.emplace(ser, gi);
                for (uint32_t q = 0; q < nkeys; ++q) res->keys.push_back(kv[q]);
                for (uint32_t i = 0; i < n; ++i) acc.emplace_back(ha[i].fn);
            } else {
                gi = it->second;
            }
            for (uint32_t i = 0; i < n; ++i) {
                const AggRec &r = recs[(size_t)g * n + i];
                AggAcc &a = acc[gi * n + i];
                if (ha[i].fn == AGG_SUM && agg_is_float(t, ha[i])) {
                    // the vectors' sums one after the other, as the ungrouped fold adds them
                    // (-0.0, which changes nothing, where the group has no row)
                    a.count += r.count;
                    const double *fv = fvec + ((size_t)g * nfsum + fslot[i]) * rg_vecs;
                    for (uint32_t v = 0; v < nv && v < rg_vecs; ++v) a.fsum = add_partial(a.fsum, fv[v]);
                } else {
                    fold_record(a, ha[i].fn, false, r);
                }
            }
        }
        return 0;
    });
    if (rc) return rc;
    const uint64_t ngroups = index.size();
    res->values.resize(ngroups * n);
    for (uint64_t g = 0; g < ngroups; ++g)
        for (uint32_t i = 0; i < n; ++i) finish_value(t, ha[i], acc[g * n + i], res->values[g * n + i]);
    *out = res.release();
    return 0;
}

uint64_t fls_group_result_ngroups(const fls_group_result *r) { return r && r->nkeys ? r->keys.size() / r->nkeys : 0; }

int fls_group_result_key(const fls_group_result *r, uint64_t group, uint32_t key, fls_group_key *out) {
    if (!r || !out || key >= r->nkeys || group >= fls_group_result_ngroups(r))
        return fail(FLS_ERR_ARG, "fls_group_result_key: key %u of group %llu out of range", key, (unsigned long long)group);
    const fls_group_result::Key &k = r->keys[group * r->nkeys + key];
    memset(out, 0, sizeof(*out));
    out->kind = k.kind;
    out->lo = k.lo;
    out->hi = k.hi;
    if (k.kind == FLS_KEYV_STRING) {
        out->str = k.str.data();
        out->str_len = k.str.size();
    }
    return 0;
}

const fls_aggregate_value *fls_group_result_values(const fls_group_result *r, uint64_t group) {
    if (!r || group >= fls_group_result_ngroups(r)) return nullptr;
    return r->values.data() + group * r->naggs;
}

void fls_group_result_free(fls_group_result *r) { delete r; }

}  // extern "C"
