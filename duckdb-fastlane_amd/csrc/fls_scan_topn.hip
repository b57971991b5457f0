// fls_scan_topn.hip -- the host half of the top-N pushdown: fls_topn
// (kernels: fls_topn.hip).
//
// Per batch (called by fill_batch for Reduce::TopN): the descriptors, the
// launches and the D2H of the row groups' candidate lists.  Per call: the
// argument checks, phase 1 (a reducing scan, reduce_scan, whose lists are
// merged in row-group order) and phase 2 (the winners' columns, copied out of
// a delivering scan of their row groups).
#include "fls_engine.hpp"

using namespace fls;
using namespace fls::engine;

FLS_ENGINE_BEGIN

// The top-N counterpart: stage 1 leaves every vector's best k candidates in
// sl.d_tvec, stage 2 merges the vectors of each row group pairwise (between
// sl.d_tvec and sl.d_ttmp) into sl.d_trg, and
// the row groups' lists are the batch's only D2H.
int enqueue_topn(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo) {
    HostBatch &hb = *sl.hb;
    const bool filtered = s.masked();
    if (!filtered)  // (enqueue_filter staged the filter's and the key's validity together)
        if (int rc = stage_validity(t, s, d, sl, rows, in_lo)) return rc;
    const uint32_t c = s.tkey.col;
    hb.nvec = (uint32_t)((rows + 1023) / 1024);
    HIP_TRY(sl.h_tdesc.alloc(2ull * sl.nrg));
    HIP_TRY(sl.d_tdesc.alloc(d.dev, 2ull * sl.nrg));
    if (rows > (1ull << 30)) return fail(FLS_ERR_LIMIT, "fls_topn: a batch of more than 2^30 rows");
    uint32_t rg_vecs = 1;
    if (int rc = rg_vec_table(t, sl, sl.h_tdesc.p, rg_vecs)) return rc;
    const size_t stride = topn_stride(s.tk);
    HIP_TRY(sl.d_tvec.alloc(d.dev, (size_t)hb.nvec * stride));
    HIP_TRY(sl.d_ttmp.alloc(d.dev, (size_t)hb.nvec * stride));
    HIP_TRY(sl.d_trg.alloc(d.dev, (size_t)sl.nrg * stride));
    HIP_TRY(hb.h_topn.alloc((size_t)sl.nrg * stride));
    DevTopn p;
    memset(&p, 0, sizeof(p));
    p.col = sl.d_out[c].p;
    p.valid = sl.valid_staged[c] ? sl.d_valid[c].p : nullptr;
    p.mask = filtered ? sl.d_mask.p : nullptr;
    p.nrows = (uint32_t)rows;
    p.k = s.tk;
    p.ob = (uint8_t)out_bytes_of(t, c);
    p.kind = col_kind(t, c);
    p.desc = s.tkey.desc ? 1 : 0;
    p.nulls_first = s.tkey.nulls_first ? 1 : 0;
    HIP_TRY(hipMemcpyAsync(sl.d_tdesc.p, sl.h_tdesc.p, 2ull * sl.nrg * sizeof(uint32_t), hipMemcpyHostToDevice,
                           sl.stream));
    HIP_TRY(launch_topn_vectors(p, sl.d_tvec.p, sl.stream));
    HIP_TRY(launch_topn_rowgroups(sl.d_tdesc.p, sl.nrg, rg_vecs, hb.nvec, s.tk, sl.d_tvec.p, sl.d_ttmp.p, sl.d_trg.p,
                                  sl.stream));
    HIP_TRY(hipMemcpyAsync(hb.h_topn.p, sl.d_trg.p, (size_t)sl.nrg * stride, hipMemcpyDeviceToHost, sl.stream));
    return 0;
}

FLS_ENGINE_END

// The winners of fls_topn in result order: their global rows and, per
// delivered column, their values (the scan's physical layout), validity words
// and the bytes of their long strings -- all copies.
struct fls_topn_result {
    uint32_t ncols = 0;
    std::vector<uint64_t> rows;
    std::vector<uint8_t> delivered;               // per column
    std::vector<std::vector<uint8_t>> values;     // per column: rows x out_bytes
    std::vector<std::vector<uint64_t>> validity;  // per column: (rows + 63) / 64 words
    std::vector<uint8_t> has_null;                // per column: a returned row is NULL
    std::vector<std::unique_ptr<uint8_t[]>> heap; // strings over 12 bytes, one allocation each
    double phase_ms[2] = {0, 0};                  // host clock: the selection scan, the late materialisation
};

namespace {

// fls_topn's argument checks (no device work); FLS_ERR_ARG messages start "order key:".
int check_topn(const fls_table *t, const fls_order_key *key, uint32_t k, const uint8_t *col_mask, uint32_t rg_begin,
               uint32_t rg_end) {
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    if (is_mapped_col(key->col))
        return fail(FLS_ERR_ARG, "order key: a mapped column (FLS_COL_MAPPED) cannot be a top-N key");
    if (key->col >= ncols) return fail(FLS_ERR_ARG, "order key: column %u out of range", key->col);
    const ColumnMeta &cm = t->meta.cols[key->col];
    if (type_is_string(cm.type))
        return fail(FLS_ERR_ARG, "order key: a VARCHAR / BLOB column (%u) cannot be an ORDER BY key", key->col);
    if (!topn_key_type(cm))
        return fail(FLS_ERR_ARG, "order key: DECIMAL(%u) column %u is wider than 64 bits", (unsigned)cm.width, key->col);
    if (col_mask) {
        bool any = false;
        for (uint32_t c = 0; c < ncols; ++c) any = any || col_mask[c];
        if (!any) return fail(FLS_ERR_ARG, "order key: col_mask names no column to deliver");
    }
    if (int rc = check_rowgroup_range(t, rg_begin, rg_end, "order key: ")) return rc;
    if (k > kMaxTopN)
        return fail(FLS_ERR_LIMIT, "fls_topn: k = %u is above %u (kMaxTopN); scan the columns (fls_scan_begin) and sort "
                    "the rows instead", k, kMaxTopN);
    for (uint32_t r = rg_begin; r < rg_end; ++r)
        if (t->meta.rgs[r].nrows > (1u << 30))
            return fail(FLS_ERR_LIMIT, "fls_topn: row group %u has more than 2^30 rows", r);
    return 0;
}

struct TopnCand {
    uint32_t rank;
    uint64_t key;
    uint64_t row;   // global
    uint32_t rg, rg_row;
};
inline bool cand_less(const TopnCand &a, const TopnCand &b) {
    if (a.rank != b.rank) return a.rank < b.rank;
    if (a.key != b.key) return a.key < b.key;
    return a.row < b.row;
}

// Phase 2 of fls_topn: the winners' values of the masked columns, copied out
// of their row groups (ascending), decoded on the context and by the path
// fls_materialize uses.
int topn_gather(fls_table *t, const std::vector<TopnCand> &win, const uint8_t *col_mask, fls_topn_result &res) {
    const uint32_t ncols = res.ncols;
    const size_t n = win.size();
    std::vector<uint32_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return win[a].row < win[b].row; });
    for (uint32_t c = 0; c < ncols; ++c) {
        if (!res.delivered[c]) continue;
        res.values[c].assign(n * (size_t)out_bytes_of(t, c), 0);
        res.validity[c].assign(std::max<size_t>(1, (n + 63) / 64), ~0ull);
    }
    // one delivering scan of the winners' row groups on the materialize context: no filter, every row
    // delivered at full width, the batches pipelined and sharded as in any scan
    std::vector<uint32_t> rgs;
    for (size_t j = 0; j < n; ++j)
        if (rgs.empty() || rgs.back() != win[order[j]].rg) rgs.push_back(win[order[j]].rg);
    ScanCtx &s = t->mat;
    ScanPlan plan;
    plan.devices = t->devices;
    plan.col_mask = col_mask;
    plan.rg0 = rgs.front();
    plan.rg1 = rgs.back() + 1;
    plan.only = &rgs;
    int rc = scan_setup(t, s, plan);
    if (!rc) rc = scan_start(t, s);
    if (rc) return rc;
    size_t i = 0;
    while (i < n) {
        const uint32_t rg = win[order[i]].rg;
        fls_rowgroup out;
        rc = scan_next(t, s, &out);
        if (rc < 0) return rc;
        if (rc == 0 || out.rowgroup != rg)
            return fail(FLS_ERR_STATE, "internal: the winners' scan did not deliver row group %u", rg);
        for (; i < n && win[order[i]].rg == rg; ++i) {
            const uint32_t dst = order[i], row = win[dst].rg_row;
            if (row >= out.nrows) return fail(FLS_ERR_STATE, "internal: winner row %u past row group %u", row, rg);
            for (uint32_t c = 0; c < ncols; ++c) {
                if (!res.delivered[c]) continue;
                if (!out.columns[c]) return fail(FLS_ERR_STATE, "internal: column %u of row group %u not decoded", c, rg);
                const size_t ob = (size_t)out_bytes_of(t, c);
                uint8_t *d = res.values[c].data() + dst * ob;
                const uint64_t *vw = out.validity[c];
                if (vw && !((vw[row >> 6] >> (row & 63)) & 1)) {  // NULL: the placeholder stays behind
                    res.validity[c][dst >> 6] &= ~(1ull << (dst & 63));
                    res.has_null[c] = 1;
                    continue;
                }
                memcpy(d, (const uint8_t *)out.columns[c] + row * ob, ob);
                if (!type_is_string(t->meta.cols[c].type)) continue;
                uint32_t len;
                memcpy(&len, d, 4);
                if (len <= 12) continue;  // inline
                const uint8_t *src;
                memcpy(&src, d + 8, 8);
                res.heap.emplace_back(new uint8_t[len]);
                memcpy(res.heap.back().get(), src, len);
                const uint8_t *own = res.heap.back().get();
                memcpy(d + 8, &own, 8);
            }
        }
    }
    return 0;
}

}  // namespace

extern "C" {

int fls_topn(fls_table *t, const fls_order_key *key, uint32_t k, const uint8_t *col_mask, uint32_t rg_begin,
             uint32_t rg_end, fls_topn_result **out) {
    if (!t || !key || !out) return fail(FLS_ERR_ARG, "fls_topn: NULL argument");
    *out = nullptr;
    if (int rc = check_topn(t, key, k, col_mask, rg_begin, rg_end)) return rc;
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    auto res = std::make_unique<fls_topn_result>();
    res->ncols = ncols;
    res->delivered.assign(ncols, 1);
    if (col_mask)
        for (uint32_t c = 0; c < ncols; ++c) res->delivered[c] = col_mask[c] ? 1 : 0;
    res->values.resize(ncols);
    res->validity.resize(ncols);
    res->has_null.assign(ncols, 0);
    std::vector<TopnCand> best;
    const auto t0 = std::chrono::steady_clock::now();
    if (k > 0) {
        // phase 1: the row groups' candidate lists, merged in row-group order
        ScanPlan plan;
        plan.rg0 = rg_begin;
        plan.rg1 = rg_end;
        plan.order = key;
        plan.k = k;
        const size_t stride = topn_stride(k);
        std::vector<TopnCand> inc, merged;
        const int rc = reduce_scan(t, plan, "top-N", [&](const fls_rowgroup &rg, const HostBatch &hb) {
            const uint8_t *base = hb.h_topn.p + (size_t)(rg.rowgroup - hb.rg0) * stride;
            TopnHdr hdr;
            memcpy(&hdr, base, sizeof(hdr));
            const uint32_t rg_rows = t->meta.rgs[rg.rowgroup].nrows;
            // a record's row counts from the batch's first row
            const uint64_t rg_off = t->meta.rgs[rg.rowgroup].first_row - t->meta.rgs[hb.rg0].first_row;
            if (hdr.count > k || hdr.count > rg_rows)  // never indexed with
                return fail(FLS_ERR_FORMAT, "top-N: row group %u reports %u candidates (k = %u, %u rows)", rg.rowgroup,
                            hdr.count, k, rg_rows);
            const TopnRec *recs = (const TopnRec *)(base + sizeof(TopnHdr));
            inc.clear();
            for (uint32_t i = 0; i < hdr.count; ++i) {
                const TopnRec &r = recs[i];
                if (r.row < rg_off || r.row - rg_off >= rg_rows || r.rank > 1)
                    return fail(FLS_ERR_FORMAT, "top-N: candidate %u of row group %u names batch row %u (its rows: %llu "
                                "to %llu; rank %u)", i, rg.rowgroup, r.row, (unsigned long long)rg_off,
                                (unsigned long long)(rg_off + rg_rows), r.rank);
                const uint32_t rg_row = (uint32_t)(r.row - rg_off);
                inc.push_back(TopnCand{r.rank, r.key, rg.first_row + rg_row, rg.rowgroup, rg_row});
            }
            if (!std::is_sorted(inc.begin(), inc.end(), cand_less))
                return fail(FLS_ERR_FORMAT, "top-N: the candidates of row group %u are not in order", rg.rowgroup);
            merged.resize(best.size() + inc.size());
            std::merge(best.begin(), best.end(), inc.begin(), inc.end(), merged.begin(), cand_less);
            if (merged.size() > k) merged.resize(k);
            best.swap(merged);
            return 0;
        });
        if (rc) return rc;
    }
    res->rows.reserve(best.size());
    for (const TopnCand &c : best) res->rows.push_back(c.row);
    const auto t1 = std::chrono::steady_clock::now();
    // phase 2: late materialisation of the winners
    if (!best.empty())
        if (int rc = topn_gather(t, best, col_mask, *res)) return rc;
    res->phase_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    res->phase_ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    *out = res.release();
    return 0;
}

int fls_topn_pruned(const fls_table *t, const fls_order_key *key, uint32_t k, uint32_t rg_begin, uint32_t rg_end) {
    if (!t || !key) return fail(FLS_ERR_ARG, "fls_topn_pruned: NULL argument");
    if (int rc = check_topn(t, key, k, nullptr, rg_begin, rg_end)) return rc;
    std::vector<uint32_t> rgs;
    return (int)select_rowgroups(t, t->filter, t->alts, key, k, rg_begin, rg_end, rgs);
}

uint64_t fls_topn_result_nrows(const fls_topn_result *r) { return r ? r->rows.size() : 0; }

const uint64_t *fls_topn_result_rows(const fls_topn_result *r) { return r ? r->rows.data() : nullptr; }

int fls_topn_result_column(const fls_topn_result *r, uint32_t col, const void **values, const uint64_t **validity) {
    if (!r || col >= r->ncols || !r->delivered[col])
        return fail(FLS_ERR_ARG, "fls_topn_result_column: column %u was not delivered", col);
    if (values) *values = r->values[col].data();
    if (validity) *validity = r->has_null[col] ? r->validity[col].data() : nullptr;
    return 0;
}

int fls_topn_result_times(const fls_topn_result *r, double *phase1_ms, double *phase2_ms) {
    if (!r) return fail(FLS_ERR_ARG, "fls_topn_result_times: NULL result");
    if (phase1_ms) *phase1_ms = r->phase_ms[0];
    if (phase2_ms) *phase2_ms = r->phase_ms[1];
    return 0;
}

void fls_topn_result_free(fls_topn_result *r) { delete r; }

}  // extern "C"
