// flsgpu.hip -- host engine behind include/flsgpu.h: connections, files and
// the scan pipeline.
//
// Replaces FastLanes' connect/read_fls/get_rowgroup_reader/materialize
// (reference src/fastlanes_facade.cpp:33-56) with:
//   * footer parse on the host (fls_reader.hpp) -- no GPU needed for schema;
//   * streaming scan: row groups sharded contiguously over the connection's
//     GPUs (no collectives: row groups are independent); per
//     GPU a two-slot pipeline H2D(compressed batch) -> decode -> D2H(pinned)
//     runs ahead of the consumer (DuckDB's scan thread).
//
// The rest of the engine is in units of its own, over the types and
// declarations of fls_engine.hpp: the launch policy every decode goes through
// (order_for_launch, launch_all), a scan's batches and a device-resident table
// alike, in fls_launch.hip, what a scan does with a batch instead of
// delivering it (ScanCtx::reduce) in fls_scan_agg.hip and fls_scan_topn.hip,
// key sets in fls_scan_keyset.hip, key maps and the mapped GROUP BY keys'
// probe in fls_scan_keymap.hip, and the device-resident mode (a shard of
// row groups uploaded verbatim to HBM and decoded by one fused launch per
// pass: bench / roofline) in fls_device_table.hip.  What those units call here
// is declared in fls_engine.hpp; every other function of this file is static.
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "fls_engine.hpp"

using namespace fls;
using namespace fls::engine;

FLS_ENGINE_BEGIN

static StrT make_string_t(const char *p, uint32_t n) {
    StrT s;
    memset(&s, 0, sizeof(s));
    s.len = n;
    if (n <= 12) {
        memcpy(s.data, p, n);
    } else {
        memcpy(s.data, p, 4);
        memcpy(s.data + 4, &p, sizeof(p));
    }
    return s;
}

ScanProf &scan_prof() {
    static auto *p = new ScanProf();
    return *p;
}

// Host threads that split a large memcpy: a scan stages each batch's
// compressed bytes from the mapped file into pinned memory for its H2D
// (instead of pinning the whole file up front, which cost ~0.12 s per GB
// before the first row group could move).  The copy must keep pace with
// compressed/decoded x the D2H rate (lineitem: ~9 GB/s at 50 GB/s D2H), more
// than one thread's page-cache copy rate.  Threads start on first use;
// FLS_COPY_THREADS (default 4) sets how many besides the caller.
class CopyPool {
  public:
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    void copy(void *dst, const void *src, size_t n) {
        constexpr size_t kMinPart = 2u << 20;
        start();
        const size_t parts = std::min<size_t>(th_.size() + 1, std::max<size_t>(1, n / kMinPart));
        if (parts <= 1) {
            memcpy(dst, src, n);
            return;
        }
        Call call;
        call.left = (int)parts - 1;
        const size_t per = (n / parts + 63) & ~size_t(63);
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (size_t p = 1; p < parts; ++p) {
                const size_t o = std::min(n, p * per), e = std::min(n, o + per);
                jobs_.push_back({(uint8_t *)dst + o, (const uint8_t *)src + o, p + 1 == parts ? n - o : e - o, &call});
            }
        }
        cv_.notify_all();
        memcpy(dst, src, std::min(n, per));
        std::unique_lock<std::mutex> lk(call.m);
        call.cv.wait(lk, [&] { return call.left == 0; });
    }

  private:
    struct Call {
        std::mutex m;
        std::condition_variable cv;
        int left = 0;
    };
    struct Job {
        uint8_t *d;
        const uint8_t *s;
        size_t n;
        Call *call;
    };
    void start() {
        std::lock_guard<std::mutex> lk(mu_);
        if (started_) return;
        started_ = true;
        const int n = (int)std::max<int64_t>(0, std::min<int64_t>(64, knob_value("FLS_COPY_THREADS")));
        for (int i = 0; i < n; ++i) th_.emplace_back([this] { run(); });
    }
    void run() {
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || !jobs_.empty(); });
                if (jobs_.empty()) return;
                j = jobs_.back();
                jobs_.pop_back();
            }
            memcpy(j.d, j.s, j.n);
            std::lock_guard<std::mutex> lk(j.call->m);
            if (--j.call->left == 0) j.call->cv.notify_all();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<Job> jobs_;
    std::vector<std::thread> th_;
    bool started_ = false, stop_ = false;
};

// Byte range of the file covering row groups [rg0, rg1).
void rg_byte_range(const FileMeta &m, uint32_t rg0, uint32_t rg1, uint64_t &lo, uint64_t &hi) {
    lo = UINT64_MAX;
    hi = 0;
    for (uint32_t r = rg0; r < rg1; ++r)
        for (auto &c : m.rgs[r].chunks) {
            lo = std::min(lo, c.off);
            hi = std::max(hi, c.off + c.len);
        }
    lo &= ~uint64_t(255);
}

// Pinned bytes a host batch holds (its columns, FSST heaps, selection).
static size_t pinned_bytes(const HostBatch &b) {
    size_t t = b.h_counts.n * sizeof(uint32_t) + b.h_sel.n * sizeof(uint32_t) + b.h_agg.n * sizeof(AggRec) + b.h_grp.n +
               b.h_topn.n;
    for (auto &x : b.h_out) t += x.n;
    for (auto &x : b.h_heap) t += x.n;
    return t;
}
static size_t pinned_bytes(const ScanDev &d) {
    size_t t = 0;
    for (auto &b : d.batches) t += pinned_bytes(*b);
    for (auto &sl : d.slots)
        t += sl.h_chunks.n * sizeof(DevChunk) + sl.h_stage.n + sl.h_fdesc.n + sl.h_qdesc.n + sl.h_adesc.n * sizeof(DevAgg) +
             sl.h_gdesc.n + sl.h_tdesc.n * sizeof(uint32_t);
    return t;
}

// What a connection keeps between scans: idle per-GPU pipelines (at most
// kIdlePerDev per GPU) and the staging copy threads.  The idle pipelines'
// pinned host batches are capped by BYTES per GPU (FLS_IDLE_PINNED_MB, default
// 1024; 0 keeps none): a batch is up to 8 row groups of every delivered column,
// about 150 MB at lineitem_full widths, so a count cap alone let a long-lived
// process (DuckDB) keep more page-locked memory than it uses.  512 MB was
// below a 16-thread scan's working set: every other warm query re-pinned
// ~100 MB at hipHostMalloc's 4-5 GB/s (profiles/r5/e2e_env_r5p_prof.txt: the
// 492 M rows/s query of a 660 M median); at 1024 no warm query allocates
// (e2e_env_r5o_cap1024.txt).  fls_connection_trim frees the idle pipelines on
// demand.  Tables share ConnRes by reference, so
// it lives until the connection and every table opened on it are closed.
struct ConnRes {
    static constexpr size_t kIdlePerDev = 2;
    std::mutex mu;
    std::vector<std::unique_ptr<ScanDev>> idle;
    CopyPool copy;
    static size_t idle_cap_bytes() {
        return (size_t)std::max<int64_t>(0, knob_value("FLS_IDLE_PINNED_MB")) << 20;
    }
    // free idle pipelines until the pinned bytes they hold on GPU dev (every
    // GPU: dev < 0) are at most keep (caller holds mu)
    void trim_locked(int dev, size_t keep) {
        std::map<int, size_t> held;
        for (size_t i = idle.size(); i-- > 0;) {
            ScanDev &d = *idle[i];
            if (dev >= 0 && d.dev != dev) continue;
            // drop batches of this pipeline while over the cap, then the pipeline
            while (!d.batches.empty() && held[d.dev] + pinned_bytes(d) > keep) {
                d.batches.pop_back();
                d.free_batches.clear();
                for (auto &b : d.batches) d.free_batches.push_back(b.get());
            }
            if (held[d.dev] + pinned_bytes(d) > keep) {
                idle.erase(idle.begin() + (long)i);
                continue;
            }
            held[d.dev] += pinned_bytes(d);
        }
    }
    std::unique_ptr<ScanDev> take(int dev) {
        {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t i = 0; i < idle.size(); ++i)
                if (idle[i]->dev == dev) {
                    auto d = std::move(idle[i]);
                    idle.erase(idle.begin() + (long)i);
                    return d;
                }
        }
        auto d = std::make_unique<ScanDev>();
        d->dev = dev;
        return d;
    }
    // back from a closing table; a pipeline with a host batch still out (a
    // row group never released) is freed rather than reused
    void give(std::unique_ptr<ScanDev> d) {
        if (!d) return;
        d->sync();
        if (d->free_batches.size() != d->batches.size()) return;
        for (auto &sl : d->slots) {
            sl.busy = sl.starved = false;
            sl.hb = nullptr;
        }
        d->free_batches.clear();
        for (auto &b : d->batches) d->free_batches.push_back(b.get());
        std::lock_guard<std::mutex> lk(mu);
        size_t same = 0;
        for (auto &x : idle) same += x->dev == d->dev;
        if (same >= kIdlePerDev) return;
        const int dev = d->dev;
        idle.push_back(std::move(d));
        trim_locked(dev, idle_cap_bytes());
    }
    // pinned bytes the idle pipelines hold (all GPUs)
    size_t idle_pinned() {
        std::lock_guard<std::mutex> lk(mu);
        size_t t = 0;
        for (auto &d : idle) t += pinned_bytes(*d);
        return t;
    }
};

FLS_ENGINE_END

struct fls_connection {
    std::vector<int> devices;
    std::shared_ptr<ConnRes> res = std::make_shared<ConnRes>();
};


// A mapped, validated file shared by the tables that read it: fls_read_fls
// keeps the last few in a process-wide cache keyed by (device, inode, size,
// mtime), so reopening an unchanged file (DuckDB opens files at every query)
// skips the chunk-header validation (10-30 ms at SF10).
// A file's compressed image kept in one GPU's HBM by the scan pipeline: the
// first scan's batches are uploaded into it instead of a per-slot buffer, and
// later scans of the same (cached, unchanged) file decode its row groups from
// it with no staging copy and no H2D -- a warm query moves only decoded bytes
// over PCIe, in one direction.  Lives with the open-file cache entry.
// One GPU's image holds the file bytes of that GPU's shard of the whole
// table (its row groups when the table is split over the connection's GPUs),
// not the whole file.  Images live in a process-wide registry with one byte
// budget per GPU (ResidentSet, resident_image).
struct DevImage {
    uint8_t *p = nullptr;                              // file bytes [lo, hi) + kImagePad
    int dev = -1;
    uint64_t lo = 0, hi = 0;
    std::unique_ptr<std::atomic<uint8_t>[]> present;   // per row group of the file: its chunks are in p
    uint32_t nrg = 0;
    ~DevImage() {
        if (p) {
            int cur = 0;
            hipGetDevice(&cur);
            hipSetDevice(dev);
            hipFree(p);
            hipSetDevice(cur);
        }
    }
};
void drop_file_images(const void *owner);
struct MappedFile {
    void *map = nullptr;
    size_t len = 0;
    FileMeta meta;
    ~MappedFile() {
        drop_file_images(this);
        if (map) munmap(map, len);
    }
};

// Every GPU's resident images, under one lock (process lifetime: tables may
// outlive static destruction order).
struct ImageRegistry {
    std::mutex mu;
    ResidentSet<DevImage> set;
};
ImageRegistry &image_registry() {
    static auto *r = new ImageRegistry();
    return *r;
}
// FLS_SCAN_RESIDENT_MB: the image budget per GPU over every cached file (0 = off)
uint64_t resident_budget() {
    return (uint64_t)std::max<int64_t>(0, knob_value("FLS_SCAN_RESIDENT_MB")) << 20;
}
FLS_ENGINE_BEGIN
uint64_t release_idle_images(int dev) {
    ImageRegistry &R = image_registry();
    ResidentSet<DevImage>::Evicted ev;
    std::lock_guard<std::mutex> lk(R.mu);
    const uint64_t b = R.set.release_idle(dev, ev);
    ev.clear();
    return b;
}
FLS_ENGINE_END
void drop_file_images(const void *owner) {
    ImageRegistry &R = image_registry();
    ResidentSet<DevImage>::Evicted ev;
    std::lock_guard<std::mutex> lk(R.mu);
    R.set.drop_owner(owner, ev);
    ev.clear();
}


FLS_ENGINE_BEGIN

int out_bytes_of(const fls_table *t, uint32_t c) { return type_out_bytes(t->meta.cols[c].type); }

uint8_t col_kind(const fls_table *t, uint32_t c) {
    const uint8_t ty = t->meta.cols[c].type;
    return type_is_float(ty) ? FK_FLOAT : type_is_signed(ty) ? FK_INT : FK_UINT;
}

int check_rowgroup_range(const fls_table *t, uint32_t rg0, uint32_t rg1, const char *prefix) {
    if (rg1 > t->meta.rgs.size() || rg0 > rg1)
        return fail(FLS_ERR_ARG, "%srow-group range [%u,%u) out of bounds", prefix, rg0, rg1);
    return 0;
}

// The validity bitmaps of chunk (rg, c) in the host image, or nullptr when the
// chunk has no NULL (fls_format.hpp "Validity")
static const uint64_t *chunk_validity_host(const fls_table *t, uint32_t rg, uint32_t c) {
    const ChunkRef &ch = t->meta.rgs[rg].chunks[c];
    if (!chunk_has_validity(ch.hdr)) return nullptr;
    return (const uint64_t *)(t->img + ch.off + validity_off(ch.len, ch.hdr.nvec));
}

// Build host string_t tables for the VARCHAR chunks of [rg0, rg1) and upload.
int build_strtabs(const fls_table *t, int dev, uint32_t rg0, uint32_t rg1, DevBuf<StrT> &tab,
                  std::vector<uint64_t> &offs, std::vector<StrT> &host) {
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    offs.assign((size_t)(rg1 - rg0) * ncols, UINT64_MAX);
    host.clear();
    for (uint32_t r = rg0; r < rg1; ++r)
        for (uint32_t c = 0; c < ncols; ++c) {
            if (!type_is_string(t->meta.cols[c].type)) continue;
            const ChunkRef &ch = t->meta.rgs[r].chunks[c];
            if (ch.hdr.enc != ENC_DICT) continue;  // FSST strings are decoded on the GPU
            const uint8_t *aux = t->img + ch.off + ch.hdr.aux_off;
            const uint32_t n = ch.hdr.dict_count;
            offs[(size_t)(r - rg0) * ncols + c] = host.size();
            for (uint32_t i = 0; i < n; ++i) {
                const uint8_t *p;
                uint32_t len;
                dict_string(aux, n, i, p, len);
                host.push_back(make_string_t((const char *)p, len));
            }
        }
    HIP_TRY(hipSetDevice(dev));
    HIP_TRY(tab.alloc(dev, host.size()));
    if (!host.empty()) HIP_TRY(hipMemcpy(tab.p, host.data(), host.size() * sizeof(StrT), hipMemcpyHostToDevice));
    return 0;
}

// Describe chunk (rg, col) located at d_chunk_base (device) for the kernel.
// code_w (1 or 2): a DICT string chunk delivered as its codes, gathered from
// the identity table d_ident instead of the string_t dictionary
// fsst_seg (DecodeTuning::Launch::fsst_seg): FSST chunks with segment tables
// for the segmented kernel
DevChunk make_devchunk(const fls_table *t, uint32_t rg, uint32_t col, const uint8_t *d_chunk, const uint8_t *d_dict,
                       uint8_t *d_out, ByteCount *bc, bool fsst_seg, uint8_t *d_heap, const uint8_t *h_heap,
                       uint32_t code_w, const uint8_t *d_ident) {
    const ChunkRef &ch = t->meta.rgs[rg].chunks[col];
    const ChunkHeader &h = ch.hdr;
    DevChunk d;
    memset(&d, 0, sizeof(d));
    d.chunk = d_chunk;
    d.out = d_out;
    d.nvec = h.nvec;
    d.dict_count = h.dict_count;
    d.meta_off = (uint32_t)h.meta_off;
    d.packed_off = (uint32_t)h.packed_off;
    d.aux_off = (uint32_t)h.aux_off;
    d.enc = h.enc;
    d.T = h.T;
    d.vbits = h.vbits;
    d.ob = (uint8_t)out_bytes_of(t, col);
    if (h.enc == ENC_DICT) d.dict = h.is_str ? d_dict : d_chunk + h.aux_off;
    if (code_w && h.enc == ENC_DICT && h.is_str) {
        d.ob = (uint8_t)code_w;
        d.dict = code_w == 1 ? d_ident : d_ident + kIdent16;
    }
    bc->values += h.nvals;
    if (h.enc == ENC_FSST) {
        d.dict = d_heap;
        d.heap_host = (uint64_t)(uintptr_t)h_heap;
        d.heap_bytes = (uint32_t)h.reserved1;
        bc->out += (uint64_t)h.nvals * 16 + h.reserved1;
        bc->meta += 32ull * h.nvec + kFsstTableBytes;
        const uint8_t *meta = t->img + ch.off + h.meta_off;
        bool sp = true;
        for (uint32_t v = 0; v < h.nvec; ++v) {
            VecMeta vm;
            memcpy(&vm, meta + 32ull * v, 32);
            FsstVecHeader fh;
            memcpy(&fh, t->img + ch.off + h.aux_off + vm.aux_off, sizeof(fh));
            bc->packed += 128ull * vm.bw + 128ull * fh.clen_w + fh.comp_len;
            bc->meta += sizeof(fh);
            if (chunk_seg_codes(h) == kFsstSegCodes) bc->meta += sizeof(FsstSegHeader) + fsst_nseg(fh.comp_len);
            // string-parallel kernel iff every string of the chunk is <= 255
            // bytes, decompressed and compressed (bounds from the two FFOR streams)
            const uint64_t dmax = (uint64_t)vm.for_base + (vm.bw >= 32 ? 0xFFFFFFFFull : (1ull << vm.bw) - 1);
            const uint64_t cmax = (uint64_t)fh.clen_base + (fh.clen_w >= 32 ? 0xFFFFFFFFull : (1ull << fh.clen_w) - 1);
            if (vm.for_base < 0 || dmax > 255 || cmax > 255) sp = false;
        }
        // bit 1: segment tables (the segmented kernel; FLS_FSST_SEG=0 keeps
        // the code-parallel one, an A/B knob)
        // and symbols of at most 7 bytes (the segmented kernel stages each
        // symbol with its length in the top byte)
        bool short_syms = true;
        const uint8_t *lens = t->img + ch.off + h.aux_off + 8 * 256;
        for (uint32_t k = 0; k < h.dict_count && k < 255; ++k) short_syms &= lens[k] <= 7;
        const bool seg = chunk_seg_codes(h) == kFsstSegCodes && short_syms && fsst_seg;
        d.vbits = (sp ? 1 : 0) | (seg ? 2 : 0);
        return d;  // separate kernels, fixed LDS layouts
    }
    bc->out += (uint64_t)h.nvals * d.ob;
    bc->meta += 32ull * h.nvec;
    const uint8_t *meta = t->img + ch.off + h.meta_off;
    uint32_t max_w = 0;
    for (uint32_t v = 0; v < h.nvec; ++v) {
        VecMeta vm;
        memcpy(&vm, meta + 32ull * v, 32);
        bc->packed += 128ull * vm.bw;
        max_w = std::max<uint32_t>(max_w, vm.bw);
        if (h.enc == ENC_DELTA) bc->meta += 128;
        if (h.enc == ENC_RLE) bc->meta += 128 + (uint64_t)vm.aux_count * (h.vbits / 8);
        if (h.enc == ENC_ALP && alp_exceptions(vm.aux_count))
            bc->meta += alp_aux_bytes(alp_exceptions(vm.aux_count), h.vbits);
    }
    if (h.enc == ENC_DICT) bc->meta += (uint64_t)h.dict_count * (h.is_str ? d.ob : h.vbits / 8);
    d.max_w = max_w;
    uint32_t pb, vb;
    chunk_lds_need(h.enc, h.T, d.ob, h.dict_count, max_w, pb, vb);
    bc->geom.p_bytes = std::max(bc->geom.p_bytes, pb);
    bc->geom.v_bytes = std::max(bc->geom.v_bytes, vb);
    return d;
}

static bool col_selected(const std::vector<uint8_t> &mask, uint32_t c) { return mask.empty() || mask[c]; }

bool is_fsst(const fls_table *t, uint32_t rg, uint32_t c) { return t->meta.rgs[rg].chunks[c].hdr.enc == ENC_FSST; }

FLS_ENGINE_END

fls_table::~fls_table() {
    if (profiled && ScanProf::on()) scan_prof().print();
    resident.clear();
    // the scan pipelines go back to the connection (synchronised first: their
    // copies may read the image or the pinned stage)
    for (ScanCtx *s : {&scan, &mat})
        for (auto &d : s->devs) {
            if (d) {
                d->sync();
                d->dimg.reset();  // the resident image stays with the open-file cache entry
            }
            if (res) res->give(std::move(d));
            d.reset();
        }
    if (registered) hipHostUnregister((void *)img);
    if (map) munmap(map, map_len);
}

// ------------------------------------------------------------------------------
// scan pipeline

FLS_ENGINE_BEGIN

// May any row of row group rg satisfy term h?  (zone maps / dictionary)
static bool term_may_match(const fls_table *t, uint32_t rg, const HostTerm &h) {
    const RowGroupMeta &r = t->meta.rgs[rg];
    const ChunkRef &ch = r.chunks[h.col];
    // NULLs: the chunk's validity flag, and the zone map's all-NULL mark
    const bool all_null = !r.zones.empty() && (r.zones[h.col].flags & ZM_ALL_NULL);
    if (h.op == OP_FALSE) return false;
    if (h.op == OP_IS_NULL) return chunk_has_validity(ch.hdr);
    if (h.op == OP_IS_NOT_NULL) return !all_null;
    if (all_null) return false;  // no valid row to compare
    if (h.op == OP_NOT_IN_SET) return true;
    if (h.op == OP_IN_SET) {
        // a key inside the zone map's range (exact on a sorted column); the empty set matches nowhere
        if (h.set->img.keys.empty()) return false;
        if (r.zones.empty() || !(r.zones[h.col].flags & ZM_VALID)) return true;
        return keyset_any_in_range(h.set->img, r.zones[h.col].min, r.zones[h.col].max);
    }
    if (is_col_op(h.op)) {
        // the two zone maps compared in the term's order; conservative
        if (r.zones.empty()) return true;
        const ZoneMap &za = r.zones[h.col], &zb = r.zones[h.col2];
        if (zb.flags & ZM_ALL_NULL) return false;  // no row valid on both sides
        if (!(za.flags & ZM_VALID) || !(zb.flags & ZM_VALID)) return true;
        uint64_t alo = za.min, ahi = za.max, blo = zb.min, bhi = zb.max;
        if (h.kind == FK_FLOAT) {  // the substitution the constant terms make below
            uint64_t nan;
            const double d = __builtin_nan("");
            memcpy(&nan, &d, 8);
            if (za.flags & ZM_ALL_NAN) alo = nan;
            if (za.flags & ZM_HAS_NAN) ahi = nan;
            if (zb.flags & ZM_ALL_NAN) blo = nan;
            if (zb.flags & ZM_HAS_NAN) bhi = nan;
        }
        auto cmp = [&](uint64_t x, uint64_t y) {
            return h.kind == FK_INT ? cmp_int((int64_t)x, (int64_t)y)
                                    : h.kind == FK_UINT ? cmp_uint(x, y) : cmp_float(as_double(x), as_double(y));
        };
        switch (h.op - OP_COL_EQ) {
        case OP_EQ: return cmp(alo, bhi) <= 0 && cmp(blo, ahi) <= 0;  // the ranges intersect
        case OP_NE: return !(cmp(alo, ahi) == 0 && cmp(blo, bhi) == 0 && cmp(alo, blo) == 0);  // not one single value
        case OP_LT: return cmp(alo, bhi) < 0;
        case OP_LE: return cmp(alo, bhi) <= 0;
        case OP_GT: return cmp(ahi, blo) > 0;
        default: return cmp(ahi, blo) >= 0;  // OP_GE
        }
    }
    if (is_map_op(h.op)) {
        // the key zone map against the map's sorted keys (as IN_SET prunes),
        // then the left zone map against the map's value range as side b of a
        // column term; the empty map matches nowhere
        const ValuemapImage &vm = h.map->img;
        if (vm.set.keys.empty()) return false;
        if (r.zones.empty()) return true;
        const ZoneMap &za = r.zones[h.col], &zk = r.zones[h.col2];
        if (zk.flags & ZM_ALL_NULL) return false;  // no row with a valid key
        if ((zk.flags & ZM_VALID) && !keyset_any_in_range(vm.set, zk.min, zk.max)) return false;
        if (!(za.flags & ZM_VALID)) return true;
        const uint64_t alo = za.min, ahi = za.max, blo = vm.vmin, bhi = vm.vmax;
        auto cmp = [&](uint64_t x, uint64_t y) {
            return vm.value_signed ? cmp_int((int64_t)x, (int64_t)y) : cmp_uint(x, y);
        };
        switch (h.op - OP_MAP_EQ) {
        case OP_EQ: return cmp(alo, bhi) <= 0 && cmp(blo, ahi) <= 0;  // the ranges intersect
        case OP_NE: return !(cmp(alo, ahi) == 0 && cmp(blo, bhi) == 0 && cmp(alo, blo) == 0);  // not one single value
        case OP_LT: return cmp(alo, bhi) < 0;
        case OP_LE: return cmp(alo, bhi) <= 0;
        case OP_GT: return cmp(ahi, blo) > 0;
        default: return cmp(ahi, blo) >= 0;  // OP_GE
        }
    }
    if (is_pat_op(h.op)) {
        // exact on a DICT chunk: some dictionary string matches (NOT LIKE: some does not)
        if (ch.hdr.enc != ENC_DICT) return true;  // FSST: no statistics
        const uint8_t *aux = t->img + ch.off + ch.hdr.aux_off;
        const bool want = h.op == OP_LIKE;
        for (uint32_t i = 0; i < ch.hdr.dict_count; ++i) {
            const uint8_t *p;
            uint32_t len;
            dict_string(aux, ch.hdr.dict_count, i, p, len);
            if (like_match(p, len, h.pat->tok.data(), (uint32_t)h.pat->tok.size()) == want) return true;
        }
        return false;
    }
    if (h.kind == FK_STR) {
        if (ch.hdr.enc != ENC_DICT) return true;  // FSST: no statistics
        const uint8_t *aux = t->img + ch.off + ch.hdr.aux_off;
        for (uint32_t i = 0; i < ch.hdr.dict_count; ++i) {
            const uint8_t *p;
            uint32_t len;
            dict_string(aux, ch.hdr.dict_count, i, p, len);
            if (op_holds(h.op, cmp_bytes(p, len, (const uint8_t *)h.str.data(), (uint32_t)h.str.size())))
                return true;
        }
        return false;
    }
    if (r.zones.empty() || !(r.zones[h.col].flags & ZM_VALID)) return true;
    const ZoneMap &z = r.zones[h.col];
    int cmin, cmax;  // min vs constant, max vs constant
    if (h.kind == FK_INT) {
        cmin = cmp_int((int64_t)z.min, (int64_t)h.value);
        cmax = cmp_int((int64_t)z.max, (int64_t)h.value);
    } else if (h.kind == FK_UINT) {
        cmin = cmp_uint(z.min, h.value);
        cmax = cmp_uint(z.max, h.value);
    } else {
        const double nan = __builtin_nan("");
        const double lo = (z.flags & ZM_ALL_NAN) ? nan : as_double(z.min);
        const double hi = (z.flags & ZM_HAS_NAN) ? nan : as_double(z.max);
        cmin = cmp_float(lo, as_double(h.value));
        cmax = cmp_float(hi, as_double(h.value));
    }
    switch (h.op) {
    case OP_EQ: return cmin <= 0 && cmax >= 0;
    case OP_NE: return !(cmin == 0 && cmax == 0);
    case OP_LT: return cmin < 0;
    case OP_LE: return cmin <= 0;
    case OP_GT: return cmax > 0;
    default: return cmax >= 0;  // OP_GE
    }
}

// Every clause has a term that may match (terms sorted by clause).
bool rowgroup_may_match(const fls_table *t, uint32_t rg, const std::vector<HostTerm> &terms) {
    size_t i = 0;
    while (i < terms.size()) {
        bool any = false;
        const uint32_t cl = terms[i].clause;
        for (; i < terms.size() && terms[i].clause == cl; ++i) any = any || term_may_match(t, rg, terms[i]);
        if (!any) return false;
    }
    return true;
}

bool rowgroup_may_match(const fls_table *t, uint32_t rg, const std::vector<HostTerm> &terms,
                        const std::vector<std::vector<HostTerm>> &alts) {
    if (!rowgroup_may_match(t, rg, terms)) return false;
    for (auto &a : alts)
        if (rowgroup_may_match(t, rg, a)) return true;
    return alts.empty();
}

// Is column c a possible ORDER BY key of fls_topn?
bool topn_key_type(const ColumnMeta &c) {
    return !type_is_string(c.type) && type_valid(c.type) && !(c.type == TY_DECIMAL && c.width > 18);
}

// Zone-map pruning of a top-N scan without a filter, for integer-like keys.
// In key space (topn_key) a row group with a zone map and no NULL holds `rows`
// records no worse than its worst bound; sorted by that bound, the row groups
// reach k records at some bound T, and a row group whose best bound is
// strictly worse than T cannot hold one of the k best.  Ties are kept, as are
// row groups without a zone map (they guarantee nothing) and, under NULLS
// FIRST, those with a NULL (NULLS LAST: a NULL is worse than T's record, so
// the strict test on the values decides).  Returns the row groups dropped.
static uint32_t topn_prune(const fls_table *t, const fls_order_key &key, uint32_t k, std::vector<uint32_t> &rgs) {
    const uint8_t ty = t->meta.cols[key.col].type;
    if (k == 0 || type_is_float(ty) || !topn_key_type(t->meta.cols[key.col])) return 0;
    const uint8_t kind = type_is_signed(ty) ? FK_INT : FK_UINT;
    struct Bound {
        uint64_t best, worst;
        bool valid, has_null;
    };
    std::vector<Bound> b(rgs.size());
    std::vector<std::pair<uint64_t, uint64_t>> sure;  // (worst bound, rows) of the row groups without a NULL
    for (size_t i = 0; i < rgs.size(); ++i) {
        const RowGroupMeta &r = t->meta.rgs[rgs[i]];
        b[i] = Bound{0, 0, false, false};
        if (r.zones.empty() || !(r.zones[key.col].flags & ZM_VALID)) continue;
        const ZoneMap &z = r.zones[key.col];
        const uint64_t a = topn_key(z.min, kind, key.desc != 0), c = topn_key(z.max, kind, key.desc != 0);
        b[i] = Bound{std::min(a, c), std::max(a, c), true, (z.flags & (ZM_HAS_NULL | ZM_ALL_NULL)) != 0};
        if (!b[i].has_null) sure.emplace_back(b[i].worst, r.nrows);
    }
    std::sort(sure.begin(), sure.end());
    uint64_t have = 0, T = 0;
    bool reached = false;
    for (size_t i = 0; i < sure.size() && !reached; ++i) {
        have += sure[i].second;
        T = sure[i].first;
        reached = have >= k;
    }
    if (!reached) return 0;
    std::vector<uint32_t> keep;
    for (size_t i = 0; i < rgs.size(); ++i) {
        const bool drop = b[i].valid && b[i].best > T && !(b[i].has_null && key.nulls_first);
        if (!drop) keep.push_back(rgs[i]);
    }
    const uint32_t dropped = (uint32_t)(rgs.size() - keep.size());
    rgs.swap(keep);
    return dropped;
}

// The row groups of [rg0, rg1) a scan reads, in order, and how many it skips:
// those the filter's zone maps / dictionaries rule out, and for a top-N scan
// without a filter (alternatives count as one) those topn_prune drops.
uint32_t select_rowgroups(const fls_table *t, const std::vector<HostTerm> &terms,
                          const std::vector<std::vector<HostTerm>> &alts, const fls_order_key *order, uint32_t k,
                          uint32_t rg0, uint32_t rg1, std::vector<uint32_t> &rgs) {
    uint32_t pruned = 0;
    rgs.clear();
    for (uint32_t r = rg0; r < rg1; ++r) {
        if (rowgroup_may_match(t, r, terms, alts)) rgs.push_back(r);
        else pruned++;
    }
    if (order && terms.empty() && alts.empty()) pruned += topn_prune(t, *order, k, rgs);
    return pruned;
}

// The file's resident image on GPU dev (made on first use), or none: a table
// not read from a file, FLS_SCAN_RESIDENT_MB=0, or no room in the GPU's image
// budget (FLS_SCAN_RESIDENT_MB, default 65,536 MB, over every cached file)
// after evicting the least recently used images no running scan holds.  The
// image holds the file bytes of shard g of G: the row groups this GPU owns
// when the whole table is split over the connection's GPUs.
static std::shared_ptr<DevImage> resident_image(fls_table *t, int dev, uint32_t g, uint32_t G) {
    if (!t->mapped) return nullptr;
    const uint64_t budget = resident_budget();
    const uint32_t N = (uint32_t)t->meta.rgs.size();
    G = std::max(1u, G);
    const uint32_t r0 = (uint32_t)((uint64_t)N * g / G), r1 = (uint32_t)((uint64_t)N * (g + 1) / G);
    if (budget == 0 || r0 >= r1) return nullptr;
    uint64_t lo, hi;
    rg_byte_range(t->meta, r0, r1, lo, hi);
    if (hi <= lo) return nullptr;
    const uint64_t need = hi - lo + kImagePad;
    ImageRegistry &R = image_registry();
    ResidentSet<DevImage>::Evicted ev;  // freed under the lock: the new image may need their memory
    std::lock_guard<std::mutex> lk(R.mu);
    if (auto p = R.set.find(t->mapped.get(), dev, lo, hi)) return p;
    // an image made for another split of the table that another scan decodes
    // from: use it (batches outside it stream); idle ones overlapping this
    // shard are replaced
    if (auto p = R.set.find_held_overlap(t->mapped.get(), dev, lo, hi)) return p;
    R.set.drop_overlap(t->mapped.get(), dev, lo, hi, ev);
    ev.clear();
    if (!R.set.make_room(dev, need, budget, ev)) return nullptr;
    ev.clear();
    if (hipSetDevice(dev) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    // leave at least half of the free HBM to the scans' own buffers: evict
    // more idle images (least recent first) while the new one would not
    for (;;) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        if (need <= free_b / 2) break;
        if (!R.set.evict_lru(dev, ev)) return nullptr;
        ev.clear();
    }
    auto di = std::make_shared<DevImage>();
    di->dev = dev;
    hipError_t e = hipMalloc((void **)&di->p, need);
    if (e == hipErrorOutOfMemory && R.set.release_idle(dev, ev) > 0) {
        (void)hipGetLastError();
        ev.clear();
        e = hipMalloc((void **)&di->p, need);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        di->p = nullptr;
        return nullptr;
    }
    di->lo = lo;
    di->hi = hi;
    di->nrg = N;
    di->present.reset(new std::atomic<uint8_t>[N]);
    for (uint32_t r = 0; r < N; ++r) di->present[r].store(0);
    R.set.insert(t->mapped.get(), dev, lo, hi, need, di);
    if (debug_enabled())
        fprintf(stderr, "DEBUG: resident image of row groups [%u, %u) on GPU %d: %llu bytes (%llu of %llu MB in use)\n",
                r0, r1, dev, (unsigned long long)need, (unsigned long long)(R.set.used(dev) >> 20),
                (unsigned long long)(budget >> 20));
    return di;
}

int scan_setup(fls_table *t, ScanCtx &s, const ScanPlan &p) {
    ProfTimer prof(PROF_SETUP);
    t->profiled = t->profiled || ScanProf::on();
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    const std::vector<int> &devs = p.devices;
    const uint32_t rg0 = p.rg0, rg1 = p.rg1;
    if (int rc = check_rowgroup_range(t, rg0, rg1, "")) return rc;
    // tear down a previous scan on this context
    for (auto &dp : s.devs) {
        ScanDev &d = *dp;
        d.sync();
        for (auto &sl : d.slots) {
            sl.busy = false;
            sl.starved = false;
            sl.hb = nullptr;
        }
        // every host batch back to the pool (a row group still held from the
        // previous scan is invalid from here on, as documented in flsgpu.h)
        d.free_batches.clear();
        for (auto &b : d.batches) d.free_batches.push_back(b.get());
    }
    s.out.clear();
    s.ready.clear();
    s.mask.assign(ncols, 1);
    if (p.col_mask)
        for (uint32_t c = 0; c < ncols; ++c) s.mask[c] = p.col_mask[c] ? 1 : 0;
    s.terms.clear();
    if (p.filter) s.terms = *p.filter;
    s.alts.clear();
    if (p.alts) s.alts = *p.alts;
    // the one place that decides what kind of scan this is
    s.reduce = Reduce::None;
    if (p.aggs) s.reduce = p.hash ? Reduce::HashAggregate : p.keys ? Reduce::GroupAggregate : Reduce::Aggregate;
    else if (p.order && p.k) s.reduce = Reduce::TopN;
    else if (p.keybuild) s.reduce = Reduce::KeySet;
    else if (p.mapbuild) s.reduce = Reduce::MapBuild;
    // the delivery options: consumers' scans only (not materialize); a reducing scan delivers nothing
    const bool options = p.delivering_scan && s.reduce == Reduce::None;
    s.dict_codes = options && t->dict_codes;
    s.narrow = options && t->narrow;
    s.defer_records = options && t->defer_records;
    s.dmask = s.mask;
    // (an IS [NOT] NULL term reads the validity alone)
    auto decode_columns_of = [&](const std::vector<HostTerm> &terms) {
        for (auto &h : terms)
            if (h.op < OP_IS_NULL || is_set_op(h.op) || is_pat_op(h.op)) s.dmask[h.col] = 1;
            else if (reads_col2(h.op)) s.dmask[h.col] = s.dmask[h.col2] = 1;  // (a map term: the left and the key column)
    };
    decode_columns_of(s.terms);
    for (auto &a : s.alts) decode_columns_of(a);
    s.aggs.clear();
    s.conds.clear();
    s.keys.clear();
    s.binds.clear();
    s.vbinds.clear();
    s.vused = 0;
    s.tk = 0;
    s.tkey = fls_order_key{};
    bool string_key = false;
    s.hash = HashPlan();
    s.max_groups = 0;
    s.keybuild = KeyBuildPlan();
    s.mapbuild = MapBuildPlan();
    switch (s.reduce) {
    case Reduce::None: break;
    case Reduce::MapBuild:
        // a map build decodes the filter's columns, its key and its value column
        s.mapbuild = *p.mapbuild;
        s.dmask[s.mapbuild.key_col] = s.dmask[s.mapbuild.value_col] = 1;
        break;
    case Reduce::KeySet:
        // a key-set build decodes the filter's columns and its key column
        s.keybuild = *p.keybuild;
        s.dmask[s.keybuild.col] = 1;
        break;
    case Reduce::HashAggregate:
        // the key columns (plain integer-like columns) and the operands are
        // decoded, as a grouped aggregate scan's are
        s.hash = *p.hash;
        s.max_groups = p.max_groups;
        [[fallthrough]];
    case Reduce::GroupAggregate:
        // the GROUP BY columns of a grouped aggregate scan are decoded too
        s.keys = *p.keys;
        if (p.binds) s.binds = *p.binds;
        for (const HostBinding &b : s.binds) s.dmask[b.col] = 1;  // a mapped key's column is decoded to be probed
        for (uint32_t c : s.keys) {
            if ((c & FLS_KEY_MAPPED) || is_mapped_col(c)) continue;  // (a derived column: its binding's column is decoded)
            s.dmask[c] = 1;
            string_key = string_key || type_is_string(t->meta.cols[c].type);
        }
        [[fallthrough]];
    case Reduce::Aggregate:
        // an aggregate scan decodes the filter's columns and the numeric
        // operands (a COUNT reads its column's validity only)
        s.aggs = *p.aggs;
        // the conditions' columns are decoded like the filter's, for the row
        // groups the scan reads: a condition prunes nothing
        if (p.conds) s.conds = *p.conds;
        for (auto &q : s.conds) decode_columns_of(q);
        // (a mapped operand, FLS_COL_MAPPED | i, is a derived column: the key
        // column of its binding is decoded to be probed)
        if (p.vbinds && p.vused) {
            s.vbinds = *p.vbinds;
            s.vused = p.vused;
            for (uint32_t i = 0; i < s.vbinds.size(); ++i)
                if ((s.vused >> i) & 1) s.dmask[s.vbinds[i].col] = 1;
        }
        for (auto &a : s.aggs) {
            if (a.fn == AGG_SUM_EXPR) {
                for (uint32_t i = 0; i < a.nf; ++i)
                    if (!is_mapped_col(a.fcol[i])) s.dmask[a.fcol[i]] = 1;
                continue;
            }
            if (a.fn >= AGG_SUM && !is_mapped_col(a.col)) s.dmask[a.col] = 1;
            if (a.fn == AGG_SUM_PRODUCT && !is_mapped_col(a.col2)) s.dmask[a.col2] = 1;
        }
        break;
    case Reduce::TopN:
        // a top-N scan decodes the filter's columns and its key column
        s.tk = p.k;
        s.tkey = *p.order;
        s.dmask[s.tkey.col] = 1;
        break;
    }
    // row-group pruning on zone maps / dictionaries (a top-N scan without a
    // filter: by the k-th bound of the key's zone maps)
    s.pruned = select_rowgroups(t, s.terms, s.alts, s.reduce == Reduce::TopN ? &s.tkey : nullptr, s.tk, rg0, rg1, s.rgs);
    // an inner binding prunes as `col IN keys(map)` would
    for (const HostBinding &b : s.binds) {
        if (b.keep) continue;
        std::vector<uint32_t> keep;
        for (uint32_t r : s.rgs)
            if (binding_may_match(t, r, b)) keep.push_back(r);
        s.pruned += (uint32_t)(s.rgs.size() - keep.size());
        s.rgs.swap(keep);
    }
    // ... and so does an inner value binding the call names
    s.pruned += prune_value_bindings(t, s.vbinds, s.vused, s.rgs);
    if (p.only) {  // a scan of listed row groups: fls_topn's late materialisation
        s.rgs = *p.only;
        s.pruned = 0;
    }
    s.cur = 0;
    s.held = -1;
    s.err_rc = 0;
    s.err_msg.clear();
    if (s.rgs.empty()) {  // an empty table or range, or every row group pruned: no device work
        s.active = true;
        return 0;
    }
    const uint32_t G = (uint32_t)devs.size(), n = (uint32_t)s.rgs.size();
    // one pipeline per GPU of this scan, borrowed from the connection (kept
    // from the previous scan of this context when it targets the same GPUs)
    bool same = s.devs.size() == G;
    for (uint32_t g = 0; same && g < G; ++g) same = s.devs[g] && s.devs[g]->dev == devs[g];
    if (!same) {
        for (auto &d : s.devs) t->res->give(std::move(d));
        s.devs.clear();
        for (uint32_t g = 0; g < G; ++g) s.devs.push_back(t->res->take(devs[g]));
    }
    s.batch = (uint32_t)std::max<int64_t>(1, knob_value("FLS_SCAN_BATCH"));
    s.early_refill = knob_value("FLS_SCAN_EARLY_REFILL") != 0;
    s.spin_wait = getenv("FLS_SCAN_SPIN_WAIT") && atoi(getenv("FLS_SCAN_SPIN_WAIT")) != 0;
    s.max_batches = (uint32_t)std::max<int64_t>(2, knob_value("FLS_SCAN_HOST_BATCHES"));
    s.nslots = (int)std::max<int64_t>(1, std::min<int64_t>(ScanDev::kMaxSlots, knob_value("FLS_SCAN_SLOTS")));
    for (uint32_t g = 0; g < G; ++g) {
        ScanDev &d = *s.devs[g];
        HIP_TRY(hipSetDevice(d.dev));
        if (!d.stream) HIP_TRY(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
        for (auto &sl : d.slots) {
            if (!sl.stream) HIP_TRY(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
            sl.d_out.resize(ncols);
        }
        // contiguous shard of the surviving row groups
        d.p0 = (uint32_t)((uint64_t)n * g / G);
        d.p1 = (uint32_t)((uint64_t)n * (g + 1) / G);
        d.next_p = d.p0;
        d.rg0 = d.p0 < d.p1 ? s.rgs[d.p0] : 0;
        d.rg1 = d.p0 < d.p1 ? s.rgs[d.p1 - 1] + 1 : 0;
        {   // the image holds this GPU's shard of the table over the connection's GPUs;
            // a GPU the connection lists k times holds k shards: pipeline g
            // takes the shard of the listing that is its own occurrence
            uint32_t occ = 0;
            for (uint32_t h = 0; h < g; ++h) occ += s.devs[h]->dev == d.dev;
            uint32_t shard = 0, seen = 0;
            bool in = false;
            for (uint32_t k = 0; k < (uint32_t)t->devices.size() && !in; ++k)
                if (t->devices[k] == d.dev && seen++ == occ) {
                    shard = k;
                    in = true;
                }
            ProfTimer pi(PROF_IMAGE);
            d.dimg = resident_image(t, d.dev, in ? shard : 0u, in ? (uint32_t)t->devices.size() : 1u);
        }
        int rc;
        {
            ProfTimer ps(PROF_STRTABS);
            rc = build_strtabs(t, d.dev, d.rg0, d.rg1, d.strtab, d.strtab_off, d.h_strtab);
        }
        if (rc) return rc;
        if ((s.dict_codes || string_key) && !d.ident.p) {
            std::vector<uint8_t> id(kIdent16 + 2 * 65536);
            for (uint32_t i = 0; i < 256; ++i) id[i] = (uint8_t)i;
            for (uint32_t i = 0; i < 65536; ++i) memcpy(&id[kIdent16 + 2 * i], &i, 2);
            HIP_TRY(d.ident.alloc(d.dev, id.size()));
            HIP_TRY(hipMemcpy(d.ident.p, id.data(), id.size(), hipMemcpyHostToDevice));
        }
        HIP_TRY(d.err.alloc(d.dev, 1));
        HIP_TRY(hipMemsetAsync(d.err.p, 0, sizeof(uint32_t), d.stream));
        HIP_TRY(hipStreamSynchronize(d.stream));
    }
    // batches are staged from the image into a pinned buffer per slot by the
    // connection's copy threads (enqueue_batch); FLS_SCAN_PIN=1 instead pins
    // the whole image once (hipHostRegister: no host copies afterwards, but
    // ~0.12 s per GB before the first batch can move)
    static const bool pin = getenv("FLS_SCAN_PIN") && atoi(getenv("FLS_SCAN_PIN")) != 0;
    if (pin && !t->pin_tried && t->len > 0) {
        t->pin_tried = true;
        if (hipHostRegister((void *)t->img, t->len, hipHostRegisterDefault) == hipSuccess) t->registered = true;
        else (void)hipGetLastError();
    }
    s.active = true;
    return 0;
}

// Validity words of the batch rows (HBM, sl.d_valid[c]) for every column the
// filter's terms, the aggregates' conditions or their operands read that has a NULL in the
// batch (row groups start at whole vectors: rows / 64 words apart);
// sl.valid_staged[c] ends up 1 for the columns staged.
int stage_validity(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo) {
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    sl.d_valid.resize(ncols);
    std::vector<uint8_t> &need = sl.valid_staged;
    need.assign(ncols, 0);
    for (auto &h : s.terms) {
        need[h.col] = 1;
        if (reads_col2(h.op)) need[h.col2] = 1;
    }
    for (auto *lists : {&s.alts, &s.conds})
        for (auto &q : *lists)
            for (auto &h : q) {
                need[h.col] = 1;
                if (reads_col2(h.op)) need[h.col2] = 1;
            }
    // (a mapped operand or key has its validity from mapval_kernel; its binding's key column is staged)
    for (auto &a : s.aggs) {
        if (a.fn == AGG_SUM_EXPR) {
            for (uint32_t i = 0; i < a.nf; ++i)
                if (!is_mapped_col(a.fcol[i])) need[a.fcol[i]] = 1;
            continue;
        }
        if (a.fn != AGG_COUNT_STAR && !is_mapped_col(a.col)) need[a.col] = 1;
        if (a.fn == AGG_SUM_PRODUCT && !is_mapped_col(a.col2)) need[a.col2] = 1;
    }
    for (uint32_t c : s.keys)
        if (!(c & FLS_KEY_MAPPED) && !is_mapped_col(c)) need[c] = 1;
    for (const HostBinding &b : s.binds) need[b.col] = 1;
    for (uint32_t i = 0; i < s.vbinds.size(); ++i)
        if ((s.vused >> i) & 1) need[s.vbinds[i].col] = 1;
    if (s.reduce == Reduce::TopN) need[s.tkey.col] = 1;
    if (s.reduce == Reduce::KeySet) need[s.keybuild.col] = 1;
    if (s.reduce == Reduce::MapBuild) need[s.mapbuild.key_col] = need[s.mapbuild.value_col] = 1;
    for (uint32_t c = 0; c < ncols; ++c) {
        bool any = false;
        for (uint32_t r = sl.rg0; need[c] && r < sl.rg0 + sl.nrg; ++r)
            any = any || chunk_has_validity(t->meta.rgs[r].chunks[c].hdr);
        if (!any) {
            need[c] = 0;
            continue;
        }
        HIP_TRY(sl.d_valid[c].alloc(d.dev, (rows + 63) / 64 + 16));
        for (uint32_t r = sl.rg0; r < sl.rg0 + sl.nrg; ++r) {
            const ChunkRef &ch = t->meta.rgs[r].chunks[c];
            uint64_t *dst = sl.d_valid[c].p + (t->meta.rgs[r].first_row - t->meta.rgs[sl.rg0].first_row) / 64;
            const size_t bytes = (size_t)kValidityVecBytes * ch.hdr.nvec;
            if (chunk_has_validity(ch.hdr))
                HIP_TRY(hipMemcpyAsync(dst, sl.in_dev + (ch.off - in_lo) + validity_off(ch.len, ch.hdr.nvec), bytes,
                                       hipMemcpyDeviceToDevice, sl.stream));
            else
                HIP_TRY(hipMemsetAsync(dst, 0xFF, bytes, sl.stream));
        }
    }
    return 0;
}

int rg_vec_table(const fls_table *t, const Slot &sl, uint32_t *tab, uint32_t &rg_vecs) {
    uint64_t vecs = 0;
    rg_vecs = 1;
    for (uint32_t r = 0; r < sl.nrg; ++r) {
        const RowGroupMeta &rg = t->meta.rgs[sl.rg0 + r];
        uint32_t *rv = tab + 2 * r;
        rv[0] = (uint32_t)((rg.first_row - t->meta.rgs[sl.rg0].first_row) / kVectorSize);
        rv[1] = (uint32_t)((rg.nrows + kVectorSize - 1) / kVectorSize);
        vecs = std::max<uint64_t>(vecs, (uint64_t)rv[0] + rv[1]);
        rg_vecs = std::max(rg_vecs, rv[1]);
    }
    if (vecs > sl.hb->nvec) return fail(FLS_ERR_STATE, "internal: row groups of a batch past its %u vectors", sl.hb->nvec);
    return 0;
}

// One term of a filter or of an aggregate's condition as its kernel sees it,
// over the slot's decoded columns and staged validity (stage_validity ran).
static int fill_set_term(const fls_table *t, ScanDev &d, Slot &sl, const HostTerm &h, DevSetTerm &ds) {
    const std::vector<uint8_t> &need = sl.valid_staged;
    const KeysetImage &ki = h.set->img;
    memset(&ds, 0, sizeof(ds));
    ds.col = sl.d_out[h.col].p;
    ds.valid = need[h.col] ? sl.d_valid[h.col].p : nullptr;
    HIP_TRY(h.set->device_image(d.dev, &ds.table));
    ds.min = ki.min;
    ds.span = ki.span;
    ds.empty = ki.empty;
    ds.cap_log2 = ki.cap_log2;
    ds.max_probe = ki.max_probe;
    ds.form = (uint8_t)ki.form;
    ds.ob = (uint8_t)out_bytes_of(t, h.col);
    ds.sign = ki.is_signed ? 1 : 0;
    ds.negate = h.op == OP_NOT_IN_SET ? 1 : 0;
    return 0;
}

// (the full decoded values of both sides, never a narrowed copy)
static void fill_col_term(const fls_table *t, Slot &sl, const HostTerm &h, DevColTerm &dc) {
    const std::vector<uint8_t> &need = sl.valid_staged;
    memset(&dc, 0, sizeof(dc));
    dc.a = sl.d_out[h.col].p;
    dc.b = sl.d_out[h.col2].p;
    dc.va = need[h.col] ? sl.d_valid[h.col].p : nullptr;
    dc.vb = need[h.col2] ? sl.d_valid[h.col2].p : nullptr;
    dc.oba = (uint8_t)out_bytes_of(t, h.col);
    dc.obb = (uint8_t)out_bytes_of(t, h.col2);
    dc.kind = h.kind;
    dc.op = (uint8_t)(h.op - OP_COL_EQ);
    dc.f32a = t->meta.cols[h.col].type == TY_FLOAT ? 1 : 0;
    dc.f32b = t->meta.cols[h.col2].type == TY_FLOAT ? 1 : 0;
}

// (the full decoded values of the left and the key column, never a narrowed copy)
static int fill_map_term(const fls_table *t, ScanDev &d, Slot &sl, const HostTerm &h, DevMapCmpTerm &dm) {
    const std::vector<uint8_t> &need = sl.valid_staged;
    const ValuemapImage &vi = h.map->img;
    memset(&dm, 0, sizeof(dm));
    dm.a = sl.d_out[h.col].p;
    dm.key = sl.d_out[h.col2].p;
    dm.va = need[h.col] ? sl.d_valid[h.col].p : nullptr;
    dm.vk = need[h.col2] ? sl.d_valid[h.col2].p : nullptr;
    HIP_TRY(h.map->device_image(d.dev, &dm.table));
    dm.min = vi.set.min;
    dm.span = vi.set.span;
    dm.empty = vi.set.empty;
    dm.cap_log2 = vi.set.cap_log2;
    dm.max_probe = vi.set.max_probe;
    dm.form = (uint8_t)vi.form;
    dm.oba = (uint8_t)out_bytes_of(t, h.col);
    dm.obk = (uint8_t)out_bytes_of(t, h.col2);
    dm.ksign = vi.set.is_signed ? 1 : 0;
    dm.vsign = vi.value_signed ? 1 : 0;
    dm.op = (uint8_t)(h.op - OP_MAP_EQ);
    return 0;
}

// Where the long strings of string column c of the batch live: a batch can
// hold DICT and FSST chunks of the column (ENC_AUTO chooses per chunk), so
// both ranges, each with its own device offset.
static void string_ranges(const fls_table *t, Slot &sl, uint32_t c, uint64_t in_lo, uint64_t in_len, StrRange &heap,
                          StrRange &image) {
    if (sl.heap_bytes[c]) {  // FSST rows: long strings live in the batch heap
        heap.host_lo = (uint64_t)(uintptr_t)sl.hb->h_heap[c].p;
        heap.host_hi = heap.host_lo + sl.heap_bytes[c];
        heap.dev_delta = (int64_t)((uintptr_t)sl.d_heap[c].p - (uintptr_t)sl.hb->h_heap[c].p);
    }
    // DICT rows: long strings point into the file image, uploaded as d_in
    image.host_lo = (uint64_t)(uintptr_t)(t->img + in_lo);
    image.host_hi = image.host_lo + in_len;
    image.dev_delta = (int64_t)((uintptr_t)sl.in_dev - (uintptr_t)(t->img + in_lo));
}

// d_tok: where the term's tokens go in HBM
static void fill_pat_term(const fls_table *t, Slot &sl, const HostTerm &h, uint64_t in_lo, uint64_t in_len,
                          const uint16_t *d_tok, DevPatTerm &dp) {
    const std::vector<uint8_t> &need = sl.valid_staged;
    const CompiledPattern &cp = *h.pat;
    memset(&dp, 0, sizeof(dp));
    dp.col = sl.d_out[h.col].p;
    dp.valid = need[h.col] ? sl.d_valid[h.col].p : nullptr;
    string_ranges(t, sl, h.col, in_lo, in_len, dp.heap, dp.image);
    dp.tok = d_tok;
    dp.ntok = (uint32_t)cp.tok.size();
    dp.min_len = cp.min_len;
    dp.prefix_len = (uint8_t)std::min<size_t>(4, cp.prefix.size());
    memcpy(&dp.prefix, cp.prefix.data(), dp.prefix_len);
    dp.negate = h.op == OP_NOT_LIKE ? 1 : 0;
    dp.exact = cp.exact ? 1 : 0;
}

// d_str: where an FK_STR term's constant bytes go in HBM
static void fill_term(const fls_table *t, Slot &sl, const HostTerm &h, uint64_t in_lo, uint64_t in_len,
                      const uint8_t *d_str, bool end_clause, DevTerm &dt) {
    const std::vector<uint8_t> &need = sl.valid_staged;
    memset(&dt, 0, sizeof(dt));
    dt.col = sl.d_out[h.col].p;
    dt.value = h.value;
    dt.kind = h.kind;
    dt.op = h.op;
    dt.ob = (uint8_t)out_bytes_of(t, h.col);
    dt.end_clause = end_clause ? 1 : 0;
    dt.valid = need[h.col] ? sl.d_valid[h.col].p : nullptr;
    if (h.kind == FK_STR) {
        dt.str = d_str;
        dt.str_len = (uint32_t)h.str.size();
        string_ranges(t, sl, h.col, in_lo, in_len, dt.heap, dt.image);
    }
}

// The descriptor block of several term lists -- the aggregates' conditions,
// the filter's alternatives -- over the slot's decoded columns and staged
// validity: DevTerm[], DevColTerm[], DevSetTerm[], DevMapCmpTerm[],
// DevPatTerm[], then the constant strings and the pattern tokens, list after
// list within each array.
struct ListDescs {
    struct Kinds {
        std::vector<const HostTerm *> ord, ccs, sets, maps, pats;
        uint32_t ptok = 0;  // tokens of the list's pattern terms
    };
    std::vector<Kinds> kinds;            // per list
    uint32_t first[kMaxConds + 1] = {};  // list q's ordinary terms are DevTerm[first[q] .. first[q + 1])
    size_t off_c = 0, off_s = 0, off_m = 0, off_p = 0, bytes = 0;
};
// Fills h_desc (the caller copies L.bytes of it to d_desc, whose addresses the
// descriptors hold); at most kMaxConds lists.
static int build_list_descs(const fls_table *t, ScanDev &d, Slot &sl, const std::vector<std::vector<HostTerm>> &lists,
                            uint64_t in_lo, uint64_t in_len, PinBuf<uint8_t> &h_desc, DevBuf<uint8_t> &d_desc,
                            ListDescs &L) {
    const uint32_t nq = (uint32_t)lists.size();
    L.kinds.assign(nq, ListDescs::Kinds());
    size_t nt = 0, nc = 0, ns = 0, nm = 0, np = 0, tail = 0;
    for (uint32_t q = 0; q < nq; ++q) {
        ListDescs::Kinds &k = L.kinds[q];
        for (auto &h : lists[q])
            (is_set_op(h.op) ? k.sets : is_pat_op(h.op) ? k.pats : is_col_op(h.op) ? k.ccs : is_map_op(h.op) ? k.maps : k.ord)
                .push_back(&h);
        nt += k.ord.size();
        nc += k.ccs.size();
        ns += k.sets.size();
        nm += k.maps.size();
        np += k.pats.size();
        for (auto *h : k.ord) tail += (h->str.size() + 15) & ~size_t(15);
        for (auto *h : k.pats) tail += (h->pat->tok.size() * sizeof(uint16_t) + 15) & ~size_t(15);
    }
    // (every descriptor size is a multiple of 16, DevTerm's and DevPatTerm's of 32: each array stays aligned)
    L.off_c = nt * sizeof(DevTerm);
    L.off_s = L.off_c + nc * sizeof(DevColTerm);
    L.off_m = L.off_s + ns * sizeof(DevSetTerm);
    L.off_p = (L.off_m + nm * sizeof(DevMapCmpTerm) + 31) & ~size_t(31);
    size_t so = L.off_p + np * sizeof(DevPatTerm);
    L.bytes = so + tail;
    HIP_TRY(h_desc.alloc(L.bytes));
    HIP_TRY(d_desc.alloc(d.dev, L.bytes));
    uint8_t *qd = h_desc.p;
    memset(qd, 0, L.bytes);
    DevTerm *terms = (DevTerm *)qd;
    DevColTerm *cterms = (DevColTerm *)(qd + L.off_c);
    DevSetTerm *sterms = (DevSetTerm *)(qd + L.off_s);
    DevMapCmpTerm *mterms = (DevMapCmpTerm *)(qd + L.off_m);
    size_t it = 0, ic = 0, is = 0, im = 0, ip = 0;
    for (uint32_t q = 0; q < nq; ++q) {
        ListDescs::Kinds &k = L.kinds[q];
        L.first[q] = (uint32_t)it;
        for (size_t i = 0; i < k.ord.size(); ++i) {
            const HostTerm &h = *k.ord[i];
            fill_term(t, sl, h, in_lo, in_len, d_desc.p + so, i + 1 == k.ord.size() || k.ord[i + 1]->clause != h.clause,
                      terms[it++]);
            if (h.kind == FK_STR) {
                memcpy(qd + so, h.str.data(), h.str.size());
                so += (h.str.size() + 15) & ~size_t(15);
            }
        }
        for (auto *h : k.ccs) fill_col_term(t, sl, *h, cterms[ic++]);
        for (auto *h : k.sets)
            if (int rc = fill_set_term(t, d, sl, *h, sterms[is++])) return rc;
        for (auto *h : k.maps)
            if (int rc = fill_map_term(t, d, sl, *h, mterms[im++])) return rc;
        for (auto *h : k.pats) {
            const CompiledPattern &cp = *h->pat;
            DevPatTerm dp;
            fill_pat_term(t, sl, *h, in_lo, in_len, (const uint16_t *)(d_desc.p + so), dp);
            memcpy(qd + L.off_p + ip++ * sizeof(DevPatTerm), &dp, sizeof(dp));
            if (!cp.tok.empty()) memcpy(qd + so, cp.tok.data(), cp.tok.size() * sizeof(uint16_t));
            so += (cp.tok.size() * sizeof(uint16_t) + 15) & ~size_t(15);
            k.ptok += (uint32_t)cp.tok.size();
        }
    }
    L.first[nq] = (uint32_t)it;
    return 0;
}

// Each list's column, key-set, map and pattern terms narrow its plane (list q's at
// planes + q * 16 * nvec) through the filter's kernels, one launch per kind,
// in the filter's order; their per-vector counts go to a scratch buffer.
static int narrow_planes(ScanDev &d, Slot &sl, const ListDescs &L, const uint8_t *d_desc, uint64_t rows,
                         uint64_t *planes) {
    const size_t plane = (size_t)sl.hb->nvec * 16;
    HIP_TRY(sl.d_ccounts.alloc(d.dev, sl.hb->nvec));
    size_t ic = 0, is = 0, im = 0, ip = 0;
    for (size_t q = 0; q < L.kinds.size(); ++q) {
        const ListDescs::Kinds &k = L.kinds[q];
        uint64_t *pl = planes + plane * q;
        if (!k.ccs.empty())
            HIP_TRY(launch_colcmp((const DevColTerm *)(d_desc + L.off_c) + ic, (uint32_t)k.ccs.size(), (uint32_t)rows, pl,
                                  sl.d_ccounts.p, d.err.p, sl.stream));
        if (!k.sets.empty())
            HIP_TRY(launch_keyset((const DevSetTerm *)(d_desc + L.off_s) + is, (uint32_t)k.sets.size(), (uint32_t)rows, pl,
                                  sl.d_ccounts.p, d.err.p, sl.stream));
        if (!k.maps.empty())
            HIP_TRY(launch_mapcmp((const DevMapCmpTerm *)(d_desc + L.off_m) + im, (uint32_t)k.maps.size(), (uint32_t)rows,
                                  pl, sl.d_ccounts.p, d.err.p, sl.stream));
        if (!k.pats.empty())
            HIP_TRY(launch_strmatch((const DevPatTerm *)(d_desc + L.off_p) + ip, (uint32_t)k.pats.size(), k.ptok,
                                    (uint32_t)rows, pl, sl.d_ccounts.p, d.err.p, sl.stream));
        ic += k.ccs.size();
        is += k.sets.size();
        im += k.maps.size();
        ip += k.pats.size();
    }
    return 0;
}

// The alternatives of a filtered batch (ScanCtx::alts), after the filter's
// kernels on the slot's mask: alt_kernel evaluates the ordinary terms of all
// alternatives in one launch, OR-s the closed ones into the mask and writes a
// plane per open one into sl.d_alt (sl.d_cond stays with the conditions, whose
// cond_kernel runs afterwards from the merged mask); the open planes are
// narrowed (narrow_planes) and alt_merge_kernel OR-s them into the mask.  The
// launches do not grow with the alternatives: one, or with an open
// alternative one per kind it holds and the merge.
static int enqueue_alternatives(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo,
                                uint64_t in_len) {
    const uint32_t na = (uint32_t)s.alts.size();
    if (na == 0 || na > kMaxConds) return fail(FLS_ERR_STATE, "internal: %u alternatives in a scan", na);
    ListDescs L;
    if (int rc = build_list_descs(t, d, sl, s.alts, in_lo, in_len, sl.h_altdesc, sl.d_altdesc, L)) return rc;
    AltList al;
    memset(&al, 0, sizeof(al));
    al.n = na;
    memcpy(al.first, L.first, sizeof(al.first));
    for (uint32_t a = 0; a < na; ++a)
        if (L.kinds[a].ccs.empty() && L.kinds[a].sets.empty() && L.kinds[a].maps.empty() && L.kinds[a].pats.empty())
            al.closed |= 1u << a;
    HIP_TRY(sl.d_alt.alloc(d.dev, (size_t)sl.hb->nvec * 16 * na));
    HIP_TRY(hipMemcpyAsync(sl.d_altdesc.p, sl.h_altdesc.p, L.bytes, hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(launch_alternatives((const DevTerm *)sl.d_altdesc.p, al, (uint32_t)rows, sl.d_mask.p, sl.d_alt.p,
                                sl.d_counts.p, d.err.p, sl.stream));
    if (int rc = narrow_planes(d, sl, L, sl.d_altdesc.p, rows, sl.d_alt.p)) return rc;
    HIP_TRY(launch_alt_merge(al, (uint32_t)rows, sl.d_mask.p, sl.d_alt.p, sl.d_counts.p, sl.stream));
    return 0;
}

// Filter descriptors of a batch: the terms over the slot's decoded columns,
// the delivered columns' compaction targets, then the constant strings.
static int enqueue_filter(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo, uint64_t in_len) {
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    std::vector<DevOut> outs;
    for (uint32_t c = 0; c < ncols; ++c) {
        if (!col_selected(s.mask, c)) continue;
        DevOut o;
        memset(&o, 0, sizeof(o));
        o.src = sl.hb->narrowed[c] ? sl.d_narrow[c].p : sl.d_out[c].p;
        o.dst = sl.hb->h_out[c].p;
        o.ob = sl.hb->ob[c];
        outs.push_back(o);
    }
    if (int rc = stage_validity(t, s, d, sl, rows, in_lo)) return rc;
    // key-set terms (each a clause of its own) go to keyset_kernel, the rest
    // to filter_kernel, which with no term left writes the row < nrows mask;
    // pattern terms (a clause each too) go to strmatch_kernel after both.
    // Column terms (a clause each as well) go to colcmp_kernel, which runs
    // before the key sets: two coalesced loads and a compare are cheaper than
    // a probe or a string match, and the later kernels skip the words it
    // empties (all clauses are AND-ed, so the order changes no result).
    // Map terms (a clause each) go to mapcmp_kernel after the key sets and
    // before the patterns: its 8-byte gather then sees the rows the cheaper
    // probes left.
    std::vector<const HostTerm *> ord, sets, pats, ccs, maps;
    for (auto &h : s.terms)
        (is_set_op(h.op) ? sets : is_pat_op(h.op) ? pats : is_col_op(h.op) ? ccs : is_map_op(h.op) ? maps : ord).push_back(&h);
    const size_t nt = ord.size(), no = outs.size(), ns = sets.size(), np = pats.size(), nc = ccs.size(), nm = maps.size();
    size_t str_bytes = 0;
    for (auto *h : ord) str_bytes += (h->str.size() + 15) & ~size_t(15);
    const size_t bytes = nt * sizeof(DevTerm) + no * sizeof(DevOut) + str_bytes;
    HIP_TRY(sl.h_fdesc.alloc(bytes));
    HIP_TRY(sl.d_fdesc.alloc(d.dev, bytes));
    uint8_t *fd = sl.h_fdesc.p;
    DevTerm *terms = (DevTerm *)fd;
    size_t so = nt * sizeof(DevTerm) + no * sizeof(DevOut);
    if (ns) {
        HIP_TRY(sl.h_sdesc.alloc(ns));
        HIP_TRY(sl.d_sdesc.alloc(d.dev, ns));
    }
    for (size_t i = 0; i < ns; ++i)
        if (int rc = fill_set_term(t, d, sl, *sets[i], sl.h_sdesc.p[i])) return rc;
    // column terms: the full decoded values of both sides (never a narrowed copy)
    if (nc) {
        HIP_TRY(sl.h_cdesc.alloc(nc));
        HIP_TRY(sl.d_cdesc.alloc(d.dev, nc));
    }
    for (size_t i = 0; i < nc; ++i) fill_col_term(t, sl, *ccs[i], sl.h_cdesc.p[i]);
    if (nm) {
        HIP_TRY(sl.h_vdesc.alloc(nm));
        HIP_TRY(sl.d_vdesc.alloc(d.dev, nm));
    }
    for (size_t i = 0; i < nm; ++i)
        if (int rc = fill_map_term(t, d, sl, *maps[i], sl.h_vdesc.p[i])) return rc;
    // pattern descriptors, then each term's tokens (16-byte aligned)
    size_t pat_bytes = np * sizeof(DevPatTerm), total_tokens = 0;
    for (auto *h : pats) pat_bytes += (h->pat->tok.size() * sizeof(uint16_t) + 15) & ~size_t(15);
    if (np) {
        HIP_TRY(sl.h_pdesc.alloc(pat_bytes));
        HIP_TRY(sl.d_pdesc.alloc(d.dev, pat_bytes));
    }
    for (size_t i = 0, po = np * sizeof(DevPatTerm); i < np; ++i) {
        const HostTerm &h = *pats[i];
        const CompiledPattern &cp = *h.pat;
        DevPatTerm dp;
        fill_pat_term(t, sl, h, in_lo, in_len, (const uint16_t *)(sl.d_pdesc.p + po), dp);
        memcpy(sl.h_pdesc.p + i * sizeof(DevPatTerm), &dp, sizeof(dp));
        if (!cp.tok.empty()) memcpy(sl.h_pdesc.p + po, cp.tok.data(), cp.tok.size() * sizeof(uint16_t));
        po += (cp.tok.size() * sizeof(uint16_t) + 15) & ~size_t(15);
        total_tokens += cp.tok.size();
    }
    for (size_t i = 0; i < nt; ++i) {
        const HostTerm &h = *ord[i];
        fill_term(t, sl, h, in_lo, in_len, sl.d_fdesc.p + so, i + 1 == nt || ord[i + 1]->clause != h.clause, terms[i]);
        if (h.kind == FK_STR) {
            memcpy(fd + so, h.str.data(), h.str.size());
            so += (h.str.size() + 15) & ~size_t(15);
        }
    }
    memcpy(fd + nt * sizeof(DevTerm), outs.data(), no * sizeof(DevOut));
    HIP_TRY(hipMemcpyAsync(sl.d_fdesc.p, fd, bytes, hipMemcpyHostToDevice, sl.stream));
    HostBatch &hb = *sl.hb;
    hb.nvec = (uint32_t)((rows + 1023) / 1024);
    HIP_TRY(sl.d_mask.alloc(d.dev, (size_t)hb.nvec * 16));
    HIP_TRY(sl.d_counts.alloc(d.dev, hb.nvec));
    HIP_TRY(launch_filter((const DevTerm *)sl.d_fdesc.p, (uint32_t)nt, (uint32_t)rows, sl.d_mask.p, sl.d_counts.p,
                          d.err.p, sl.stream));
    if (nc) {
        HIP_TRY(hipMemcpyAsync(sl.d_cdesc.p, sl.h_cdesc.p, nc * sizeof(DevColTerm), hipMemcpyHostToDevice, sl.stream));
        HIP_TRY(launch_colcmp(sl.d_cdesc.p, (uint32_t)nc, (uint32_t)rows, sl.d_mask.p, sl.d_counts.p, d.err.p,
                              sl.stream));
    }
    if (ns) {
        HIP_TRY(hipMemcpyAsync(sl.d_sdesc.p, sl.h_sdesc.p, ns * sizeof(DevSetTerm), hipMemcpyHostToDevice, sl.stream));
        HIP_TRY(launch_keyset(sl.d_sdesc.p, (uint32_t)ns, (uint32_t)rows, sl.d_mask.p, sl.d_counts.p, d.err.p,
                              sl.stream));
    }
    if (nm) {
        HIP_TRY(hipMemcpyAsync(sl.d_vdesc.p, sl.h_vdesc.p, nm * sizeof(DevMapCmpTerm), hipMemcpyHostToDevice, sl.stream));
        HIP_TRY(launch_mapcmp(sl.d_vdesc.p, (uint32_t)nm, (uint32_t)rows, sl.d_mask.p, sl.d_counts.p, d.err.p,
                              sl.stream));
    }
    if (np) {
        HIP_TRY(hipMemcpyAsync(sl.d_pdesc.p, sl.h_pdesc.p, pat_bytes, hipMemcpyHostToDevice, sl.stream));
        HIP_TRY(launch_strmatch((const DevPatTerm *)sl.d_pdesc.p, (uint32_t)np, (uint32_t)total_tokens, (uint32_t)rows,
                                sl.d_mask.p, sl.d_counts.p, d.err.p, sl.stream));
    }
    if (!s.alts.empty())  // the alternatives: the mask keeps the rows where one of them is true
        if (int rc = enqueue_alternatives(t, s, d, sl, rows, in_lo, in_len)) return rc;
    if (!s.binds.empty())  // mapped GROUP BY keys: their codes, and the inner ones' narrowing of the mask
        if (int rc = enqueue_keymap(t, s, d, sl, rows)) return rc;
    if (s.vused)  // mapped columns: their values and validity, and the inner ones' narrowing of the mask
        if (int rc = enqueue_mapval(t, s, d, sl, rows)) return rc;
    if (s.reduce != Reduce::None) return 0;  // an aggregate / top-N scan reduces under the mask: nothing is compacted or delivered
    HIP_TRY(hb.h_counts.alloc(hb.nvec));
    HIP_TRY(hb.h_sel.alloc(std::max<uint64_t>(rows, 1)));
    HIP_TRY(launch_compact((const DevOut *)(sl.d_fdesc.p + nt * sizeof(DevTerm)), (uint32_t)no, sl.d_mask.p,
                           sl.d_counts.p, (uint32_t)rows, t->meta.rowgroup_size, hb.h_sel.p, sl.stream));
    HIP_TRY(hipMemcpyAsync(hb.h_counts.p, sl.d_counts.p, hb.nvec * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           sl.stream));
    hb.sel_ready = false;
    return 0;
}

// The conditions of an aggregate scan's batch (ScanCtx::conds): one plane of
// `where & cond` words per condition into sl.d_cond, which upload_agg_descs
// hands to the aggregates bound to it.  After the filter's kernels (the
// planes start from the slot's mask; unfiltered: from row < nrows) and
// stage_validity.  cond_kernel evaluates the ordinary terms of all conditions
// in one launch; a condition's column, key-set and pattern terms then narrow
// its plane (narrow_planes).  One descriptor block (build_list_descs).
static int enqueue_conditions(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo,
                              uint64_t in_len) {
    const uint32_t nq = (uint32_t)s.conds.size();
    if (nq == 0 || nq > kMaxConds) return fail(FLS_ERR_STATE, "internal: %u conditions in a scan", nq);
    HostBatch &hb = *sl.hb;
    hb.nvec = (uint32_t)((rows + 1023) / 1024);
    ListDescs L;
    if (int rc = build_list_descs(t, d, sl, s.conds, in_lo, in_len, sl.h_qdesc, sl.d_qdesc, L)) return rc;
    CondList cl;
    memset(&cl, 0, sizeof(cl));
    cl.n = nq;
    memcpy(cl.first, L.first, sizeof(cl.first));
    const size_t plane = (size_t)hb.nvec * 16;
    HIP_TRY(sl.d_cond.alloc(d.dev, plane * nq));
    HIP_TRY(hipMemcpyAsync(sl.d_qdesc.p, sl.h_qdesc.p, L.bytes, hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(launch_conditions((const DevTerm *)sl.d_qdesc.p, cl, (uint32_t)rows, s.masked() ? sl.d_mask.p : nullptr,
                              sl.d_cond.p, d.err.p, sl.stream));
    return narrow_planes(d, sl, L, sl.d_qdesc.p, rows, sl.d_cond.p);
}


// enqueue the next batch of device d into slot si: up to s.batch consecutive
// surviving row groups
// A slot's refill in two parts.  claim_batch (with s.mu held) takes the
// slot's next row groups and a host batch; fill_batch (without s.mu: the
// staging copy, descriptors, H2D, launches and D2H of a batch take about a
// millisecond, and every consumer's acquire and release needs s.mu) enqueues
// its work; the slot turns busy (visible to acquire) only once its event is
// recorded.  The read_fastlanes profile of round 3's inline refill: of 1.8 s
// of scan-thread time (16 threads, lineitem_full SF10), 1.2 s was waiting for
// the claim lock while one thread ran a refill (profiles/r4/).
static int fill_batch(fls_table *t, ScanCtx &s, ScanDev &d, int si);
static int claim_batch(fls_table *t, ScanCtx &s, ScanDev &d, int si) {
    Slot &sl = d.slots[si];
    sl.busy = false;
    sl.starved = false;
    sl.hb = nullptr;
    if (d.next_p >= d.p1) return 0;
    // host side from the pool; at the cap the refill waits for a release.
    // Slots past the first two never grow the pool: they run on host batches
    // consumers have handed back (a cold query's first batches would otherwise
    // wait for one more pinned allocation each; slots_r6az.txt)
    if (d.free_batches.empty()) {
        if (d.batches.size() >= s.max_batches || si >= 2) {
            sl.starved = true;
            return 0;
        }
        d.batches.push_back(std::make_unique<HostBatch>());
        d.free_batches.push_back(d.batches.back().get());
    }
    {   // test hook: FLS_TEST_FAIL_ENQUEUE=k fails the k-th batch enqueue of the
        // process (1-based) as an allocation failure would (tests/test_scan_errors.py)
        static std::atomic<long> n_enqueue{0};
        const char *f = getenv("FLS_TEST_FAIL_ENQUEUE");
        if (f && ++n_enqueue == atol(f)) return fail(FLS_ERR_NOMEM, "injected batch enqueue failure (FLS_TEST_FAIL_ENQUEUE)");
    }
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    sl.rg0 = s.rgs[d.next_p];
    sl.nrg = 1;
    while (sl.nrg < s.batch && d.next_p + sl.nrg < d.p1 && s.rgs[d.next_p + sl.nrg] == sl.rg0 + sl.nrg) sl.nrg++;
    d.next_p += sl.nrg;
    sl.hb = d.free_batches.back();
    d.free_batches.pop_back();
    HostBatch &hb = *sl.hb;
    hb.rg0 = sl.rg0;
    hb.nrg = sl.nrg;
    hb.handed = hb.released = 0;
    hb.h_out.resize(ncols);
    sl.filling = true;
    return 1;
}
// Both parts (the scan's first batches, a refill a release unblocks).
static int enqueue_batch(fls_table *t, ScanCtx &s, ScanDev &d, int si) {
    const int c = claim_batch(t, s, d, si);
    if (c <= 0) return c;
    const int rc = fill_batch(t, s, d, si);
    d.slots[si].filling = false;
    d.slots[si].busy = rc == 0;
    return rc;
}
static int fill_batch(fls_table *t, ScanCtx &s, ScanDev &d, int si) {
    ProfTimer prof(PROF_FILL), pdesc(PROF_FILL_DESC);
    Slot &sl = d.slots[si];
    HostBatch &hb = *sl.hb;
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    const bool filtered = s.masked();  // (a mapped key's probe needs the mask: filter_kernel with zero terms)
    HIP_TRY(hipSetDevice(d.dev));
    // 1. H2D of the batch's compressed bytes
    // (resident image: nothing when every row group of the batch is there
    // already, else the upload goes into the image and marks them present)
    uint64_t lo, hi;
    rg_byte_range(t->meta, sl.rg0, sl.rg0 + sl.nrg, lo, hi);
    sl.in_base = lo;
    DevImage *di = d.dimg.get();
    if (di && (lo < di->lo || hi > di->hi)) di = nullptr;  // outside this GPU's image: streamed
    bool have = di != nullptr;
    for (uint32_t r = sl.rg0; have && r < sl.rg0 + sl.nrg; ++r) have = di->present[r].load(std::memory_order_acquire) != 0;
    hb.upload_resident.store(di != nullptr && !have);
    if (have) {
        sl.in_dev = di->p + (lo - di->lo);
        if (getenv("FLS_DEBUG"))
            fprintf(stderr, "DEBUG: scan batch of row groups [%u, %u) decoded from the HBM-resident image\n", sl.rg0,
                    sl.rg0 + sl.nrg);
    } else {
        uint8_t *dst;
        if (di) {
            dst = di->p + (lo - di->lo);
        } else {
            HIP_TRY(sl.d_in.alloc(d.dev, hi - lo + kImagePad));
            dst = sl.d_in.p;
        }
        const uint8_t *src = t->img + lo;
        if (!t->registered) {
            HIP_TRY(sl.h_stage.alloc(hi - lo));
            ProfTimer pc(PROF_STAGE_COPY, hi - lo);
            t->res->copy.copy(sl.h_stage.p, src, hi - lo);
            src = sl.h_stage.p;
        }
        // (by the DMA engines: a copy kernel here, 57.4 GB/s alone, waits for
        // CUs behind the other slot's decode and lost the overlap: the cold
        // 16-thread query ran 135 against 156 M rows/s, cold_copy_ab_r6ap.txt)
        HIP_TRY(hipMemcpyAsync(dst, src, hi - lo, hipMemcpyHostToDevice, sl.stream));
        sl.in_dev = dst;
    }
    // dictionary-coded delivery: a delivered DICT string column no filter term
    // reads goes over PCIe as 1- or 2-byte codes when every chunk of the batch
    // is DICT (DuckDB dictionary vectors over the host string_t dictionaries)
    hb.ob.assign(ncols, 0);
    hb.dict_ptrs.assign((size_t)sl.nrg * ncols, nullptr);
    hb.dict_sizes.assign((size_t)sl.nrg * ncols, 0);
    // A VARCHAR key of a grouped aggregate is decoded as codes the same way,
    // whatever is delivered: its key within a row group is the code
    // (fls_aggregate_grouped has checked the chunks).
    std::vector<uint8_t> code_w(ncols, 0), in_term(ncols, 0), is_key(ncols, 0);
    for (auto &h : s.terms) {
        in_term[h.col] = 1;
        if (reads_col2(h.op)) in_term[h.col2] = 1;
    }
    for (auto *lists : {&s.alts, &s.conds})
        for (auto &q : *lists)
            for (auto &h : q) {
                in_term[h.col] = 1;
                if (reads_col2(h.op)) in_term[h.col2] = 1;
            }
    for (uint32_t c : s.keys)
        if (!(c & FLS_KEY_MAPPED) && !is_mapped_col(c)) is_key[c] = 1;  // (a mapped key or column is derived, never a string)
    for (uint32_t c = 0; c < ncols; ++c) {
        hb.ob[c] = (uint8_t)out_bytes_of(t, c);
        const bool coded = is_key[c] || (s.dict_codes && col_selected(s.mask, c));
        if (!coded || in_term[c] || !type_is_string(t->meta.cols[c].type)) continue;
        bool all = true;
        uint32_t maxd = 0;
        for (uint32_t r = sl.rg0; r < sl.rg0 + sl.nrg; ++r) {
            const ChunkHeader &h = t->meta.rgs[r].chunks[c].hdr;
            all = all && h.enc == ENC_DICT;
            maxd = std::max(maxd, h.dict_count);
        }
        if (!all || maxd > 65536) continue;
        code_w[c] = hb.ob[c] = maxd <= 256 ? 1 : 2;
        for (uint32_t r = 0; r < sl.nrg; ++r) {
            const size_t i = (size_t)r * ncols + c;
            hb.dict_ptrs[i] = d.h_strtab.data() + d.strtab_off[(size_t)(sl.rg0 + r - d.rg0) * ncols + c];
            hb.dict_sizes[i] = t->meta.rgs[sl.rg0 + r].chunks[c].hdr.dict_count;
        }
    }
    // the decode's bytes per row (string_t / code width / the type's width);
    // hb.ob below is what crosses PCIe
    const std::vector<uint8_t> dob = hb.ob;
    // narrowed delivery: an integer column whose row groups' zone maps bound
    // every value within 2^8 / 2^16 / 2^32 of the row group's minimum crosses
    // PCIe as value - minimum in 1 / 2 / 4 bytes (narrow_kernel after the decode)
    hb.narrowed.assign(ncols, 0);
    hb.nbase.assign((size_t)sl.nrg * ncols, 0);
    for (uint32_t c = 0; s.narrow && c < ncols; ++c) {
        const uint8_t ty = t->meta.cols[c].type;
        if (!col_selected(s.mask, c) || type_is_string(ty) || type_is_float(ty) || hb.ob[c] < 2) continue;
        bool ok = true;
        uint64_t range = 0;
        for (uint32_t r = sl.rg0; ok && r < sl.rg0 + sl.nrg; ++r) {
            const auto &zs = t->meta.rgs[r].zones;
            ok = !zs.empty() && (zs[c].flags & ZM_VALID) && !(zs[c].flags & ZM_ALL_NULL);
            if (ok) range = std::max<uint64_t>(range, zs[c].max - zs[c].min);
        }
        const uint8_t nw = range < (1ull << 8) ? 1 : range < (1ull << 16) ? 2 : range < (1ull << 32) ? 4 : 8;
        if (!ok || nw >= hb.ob[c]) continue;
        hb.ob[c] = nw;
        hb.narrowed[c] = 1;
        for (uint32_t r = 0; r < sl.nrg; ++r) hb.nbase[(size_t)r * ncols + c] = t->meta.rgs[sl.rg0 + r].zones[c].min;
    }
    // FSST columns as string lengths: the narrow kernel takes the low 1 / 2 /
    // 4 bytes of each string_t record's length word (base 0); the records are
    // rebuilt over the copied heap on the consumer's thread (scan_acquire).
    // Unfiltered scans only (a filtered batch compacts its rows, and the heap
    // offsets of the delivered strings need every row's length).
    // On by default with narrowing (FLS_SCAN_STRLEN=0: string_t records over
    // the link).  Round 3 measured it neutral while the scan was bound by host
    // work (profiles/r3/bench_e2e_strlen_r3zj.json); with the compressed image
    // resident in HBM the 16-thread read_fastlanes is bound by the D2H link,
    // and the lengths (15 fewer bytes per lineitem row) measured 7.81e8 rows/s
    // against 6.78e8 (profiles/r4/e2e_arms_strlen_r4t.txt).
    hb.strlen_w.assign(ncols, 0);
    const bool strlen_on = knob_value("FLS_SCAN_STRLEN") != 0;
    for (uint32_t c = 0; strlen_on && s.narrow && !s.masked() && c < ncols; ++c) {
        if (!col_selected(s.mask, c) || !type_is_string(t->meta.cols[c].type) || hb.ob[c] != 16) continue;
        bool ok = true;
        uint64_t maxlen = 0;
        for (uint32_t r = sl.rg0; ok && r < sl.rg0 + sl.nrg; ++r) {
            ok = is_fsst(t, r, c);
            const ChunkRef &ch = t->meta.rgs[r].chunks[c];
            const uint8_t *meta = t->img + ch.off + ch.hdr.meta_off;
            for (uint32_t v = 0; ok && v < ch.hdr.nvec; ++v) {
                VecMeta vm;
                memcpy(&vm, meta + 32ull * v, 32);
                ok = vm.for_base >= 0 && vm.bw <= 32;
                maxlen = std::max<uint64_t>(maxlen, (uint64_t)vm.for_base + (vm.bw >= 32 ? 0xFFFFFFFFull : (1ull << vm.bw) - 1));
            }
        }
        if (!ok) continue;
        const uint8_t nw = maxlen <= 0xFF ? 1 : maxlen <= 0xFFFF ? 2 : 4;
        hb.ob[c] = nw;
        hb.narrowed[c] = 1;
        hb.strlen_w[c] = nw;
        for (uint32_t r = 0; r < sl.nrg; ++r) hb.nbase[(size_t)r * ncols + c] = 0;
    }
    hb.narrow_out = hb.narrowed;
    hb.ob_out = hb.ob;
    for (uint32_t c = 0; c < ncols; ++c)
        if (hb.strlen_w[c]) {
            hb.narrow_out[c] = 0;
            hb.ob_out[c] = 16;
        }
    // 2. decode into the slot's device columns (FSST columns also into a heap)
    const uint64_t max_rows = (uint64_t)s.batch * t->meta.rowgroup_size;
    sl.heap_bytes.assign(ncols, 0);
    sl.d_heap.resize(ncols);
    hb.h_heap.resize(ncols);
    std::vector<uint64_t> hoff((size_t)sl.nrg * ncols, 0);
    for (uint32_t c = 0; c < ncols; ++c) {
        if (!col_selected(s.dmask, c)) continue;
        const uint64_t nb = max_rows * out_bytes_of(t, c);
        HIP_TRY(sl.d_out[c].alloc(d.dev, nb));
        // the host column at the width that crosses PCIe (narrowed values,
        // dictionary codes, string lengths): pinned memory comes at ~6 GB/s
        // whatever the thread count (pin_alloc_r6ar.txt), and a cold query
        // allocates every host batch it holds
        if (col_selected(s.mask, c)) HIP_TRY(hb.h_out[c].alloc(max_rows * hb.ob[c]));
        for (uint32_t r = 0; r < sl.nrg; ++r) {
            hoff[(size_t)r * ncols + c] = sl.heap_bytes[c];
            if (is_fsst(t, sl.rg0 + r, c)) sl.heap_bytes[c] += t->meta.rgs[sl.rg0 + r].chunks[c].hdr.reserved1;
        }
        if (sl.heap_bytes[c]) {
            HIP_TRY(sl.d_heap[c].alloc(d.dev, sl.heap_bytes[c]));
            // (+16: scan_acquire reads a string's first 16 bytes whole)
            HIP_TRY(hb.h_heap[c].alloc(sl.heap_bytes[c] + 16));
        }
    }
    hb.heap_off = hoff;
    hb.h_rec.resize(ncols);
    hb.h_rec_cap.resize(ncols, 0);
    for (uint32_t c = 0; c < ncols; ++c)
        if (hb.strlen_w[c] && hb.h_rec_cap[c] < max_rows) {
            hb.h_rec[c].reset(new (std::nothrow) uint8_t[max_rows * 16]);
            if (!hb.h_rec[c]) return fail(FLS_ERR_NOMEM, "scan: no host memory for %llu string records",
                                          (unsigned long long)max_rows);
            hb.h_rec_cap[c] = max_rows;
        }
    std::vector<DevChunk> list;
    ByteCount bc;
    ProfTimer plist(PROF_FILL_LIST);
    const DecodeTuning tuning = read_decode_tuning();
    for (uint32_t c = 0; c < ncols; ++c) {
        if (!col_selected(s.dmask, c)) continue;
        for (uint32_t r = sl.rg0; r < sl.rg0 + sl.nrg; ++r) {
            const ChunkRef &ch = t->meta.rgs[r].chunks[c];
            const uint64_t so = d.strtab_off[(size_t)(r - d.rg0) * ncols + c];
            const uint8_t *dict = so == UINT64_MAX ? nullptr : (const uint8_t *)(d.strtab.p + so);
            uint8_t *out = sl.d_out[c].p + (t->meta.rgs[r].first_row - t->meta.rgs[sl.rg0].first_row) * dob[c];
            const uint64_t ho = hoff[(size_t)(r - sl.rg0) * ncols + c];
            list.push_back(make_devchunk(t, r, c, sl.in_dev + (ch.off - lo), dict, out, &bc, tuning.launch.fsst_seg,
                                         sl.heap_bytes[c] ? sl.d_heap[c].p + ho : nullptr,
                                         sl.heap_bytes[c] ? hb.h_heap[c].p + ho : nullptr, code_w[c], d.ident.p));
        }
    }
    plist.stop();
    FsstCounts fsst;
    const DecodeTuning tn = launch_policy(tuning, list, bc.geom);
    const uint32_t nmain = order_for_launch(list, &fsst, tn);
    const size_t k = list.size();
    const SplitPlan plan = append_split(list, nmain, bc.geom, tn);
    pdesc.stop();
    const size_t kk = list.size();
    HIP_TRY(sl.h_chunks.alloc(kk));
    HIP_TRY(sl.d_chunks.alloc(d.dev, kk));
    if (kk) memcpy(sl.h_chunks.p, list.data(), kk * sizeof(DevChunk));
    if (!hb.done) HIP_TRY(hipEventCreateWithFlags(&hb.done, hipEventDisableTiming));
    if (ScanProf::on())
        for (hipEvent_t &e : hb.pt)
            if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hb.h_err.alloc(1));
    if (hb.pt[0]) HIP_TRY(hipEventRecord(hb.pt[0], sl.stream));
    HIP_TRY(hipMemcpyAsync(sl.d_chunks.p, sl.h_chunks.p, kk * sizeof(DevChunk), hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(sl.queue.alloc(d.dev, kQueueWords));
    // (only batches with FSST work: a stale FLS_FSST_VARIANT must not fail
    // integer-only scans)
    if (fsst.total_vecs() > 0)
        if (const int rc = fsst_config_check(tn)) return rc;
    // (an aggregate scan of counts without a filter decodes no column)
    if (kk || !s.aggregating())
        HIP_TRY(launch_all(sl.d_chunks.p, nmain, (uint32_t)k, fsst, d.err.p, bc.geom, sl.stream, sl.queue.p, tn, plan));
    const uint64_t rows = t->meta.rgs[sl.rg0 + sl.nrg - 1].first_row + t->meta.rgs[sl.rg0 + sl.nrg - 1].nrows -
                          t->meta.rgs[sl.rg0].first_row;
    // 2b. narrowed columns: value - base into their narrow copies
    {
        std::vector<uint32_t> nc;
        for (uint32_t c = 0; c < ncols; ++c)
            if (hb.narrowed[c]) nc.push_back(c);
        if (!nc.empty()) {
            sl.d_narrow.resize(ncols);
            const size_t bytes = nc.size() * (sizeof(DevNarrow) + 8ull * sl.nrg);
            HIP_TRY(sl.h_ndesc.alloc(bytes));
            HIP_TRY(sl.d_ndesc.alloc(d.dev, bytes));
            DevNarrow *dn = (DevNarrow *)sl.h_ndesc.p;
            uint64_t *bases = (uint64_t *)(sl.h_ndesc.p + nc.size() * sizeof(DevNarrow));
            for (size_t k = 0; k < nc.size(); ++k) {
                const uint32_t c = nc[k];
                HIP_TRY(sl.d_narrow[c].alloc(d.dev, max_rows * hb.ob[c]));
                memset(&dn[k], 0, sizeof(DevNarrow));
                dn[k].src = sl.d_out[c].p;
                dn[k].dst = sl.d_narrow[c].p;
                dn[k].base = (const uint64_t *)(sl.d_ndesc.p + nc.size() * sizeof(DevNarrow)) + k * sl.nrg;
                dn[k].ob = dob[c];
                dn[k].nw = hb.ob[c];
                dn[k].sign = type_is_signed(t->meta.cols[c].type) ? 1 : 0;
                for (uint32_t r = 0; r < sl.nrg; ++r) bases[k * sl.nrg + r] = hb.nbase[(size_t)r * ncols + c];
            }
            HIP_TRY(hipMemcpyAsync(sl.d_ndesc.p, sl.h_ndesc.p, bytes, hipMemcpyHostToDevice, sl.stream));
            HIP_TRY(launch_narrow((const DevNarrow *)sl.d_ndesc.p, (uint32_t)nc.size(), (uint32_t)rows,
                                  t->meta.rowgroup_size, d.err.p, sl.stream));
        }
    }
    if (filtered) {
        // 3a. select + compact the qualifying rows straight into pinned host memory
        int rc = enqueue_filter(t, s, d, sl, rows, lo, hi - lo);
        if (rc) return rc;
    }
    // 3b. a reducing scan: reduce under the mask; what it leaves is the batch's only D2H
    if (!s.conds.empty()) {
        // the aggregates' conditions first: their planes, from the mask (or every row)
        if (!filtered)  // (else enqueue_filter staged every validity the scan reads)
            if (int rc = stage_validity(t, s, d, sl, rows, lo)) return rc;
        if (int rc = enqueue_conditions(t, s, d, sl, rows, lo, hi - lo)) return rc;
    }
    {
        int rc = 0;
        switch (s.reduce) {
        case Reduce::None: break;
        case Reduce::Aggregate: rc = enqueue_aggregate(t, s, d, sl, rows, lo); break;             // partial records
        case Reduce::GroupAggregate: rc = enqueue_group_aggregate(t, s, d, sl, rows, lo); break;  // tables of groups
        case Reduce::TopN: rc = enqueue_topn(t, s, d, sl, rows, lo); break;                       // candidate lists
        case Reduce::HashAggregate: rc = enqueue_hash_aggregate(t, s, d, sl, rows, lo); break;    // into the pipeline's table
        case Reduce::KeySet: rc = enqueue_keyset_build(t, s, d, sl, rows, lo); break;             // into the GPU's bitmap
        case Reduce::MapBuild: rc = enqueue_mapbuild(t, s, d, sl, rows, lo); break;               // into the GPU's array
        }
        if (rc) return rc;
    }
    // 3. D2H into pinned host columns (and string heaps)
    if (hb.pt[1]) HIP_TRY(hipEventRecord(hb.pt[1], sl.stream));
    hb.prof_d2h = 0;
    {
        // by the copy kernel (FLS_SCAN_COPY_KERNEL; fls_filter.hpp), or the
        // DMA engines for a misaligned pair and with the knob at 0
        const bool by_kernel = knob_value("FLS_SCAN_COPY_KERNEL") != 0;
        std::vector<HostCopy> copies;
        auto d2h = [&](uint8_t *dst, const uint8_t *src, uint64_t bytes) -> hipError_t {
            hb.prof_d2h += bytes;
            if (by_kernel && !(((uintptr_t)dst | (uintptr_t)src) & 15)) {
                copies.push_back({src, dst, bytes});
                return hipSuccess;
            }
            return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, sl.stream);
        };
        for (uint32_t c = 0; c < ncols; ++c) {
            if (!col_selected(s.mask, c)) continue;
            if (!filtered)
                HIP_TRY(d2h(hb.h_out[c].p, hb.narrowed[c] ? sl.d_narrow[c].p : sl.d_out[c].p, rows * hb.ob[c]));
            if (sl.heap_bytes[c]) HIP_TRY(d2h(hb.h_heap[c].p, sl.d_heap[c].p, sl.heap_bytes[c]));
        }
        HIP_TRY(launch_host_copy(copies.data(), (uint32_t)copies.size(), sl.stream));
    }
    if (hb.pt[2]) {
        HIP_TRY(hipEventRecord(hb.pt[2], sl.stream));
        hb.prof_pending.store(true);
    }
    // the error flags ride along (sticky device flags: a batch sees its own
    // kernels' and any earlier ones'), so an acquire reads pinned memory
    // instead of a synchronous 4-byte copy per row group
    HIP_TRY(hipMemcpyAsync(hb.h_err.p, d.err.p, sizeof(uint32_t), hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipEventRecord(hb.done, sl.stream));
    hb.col_ptrs.assign((size_t)sl.nrg * ncols, nullptr);
    hb.valid_ptrs.assign((size_t)sl.nrg * ncols, nullptr);
    hb.vbits.resize((size_t)sl.nrg * ncols);
    if (!filtered)  // every row delivered: the image's bitmaps are the validity masks
        for (uint32_t r = 0; r < sl.nrg; ++r)
            for (uint32_t c = 0; c < ncols; ++c)
                if (col_selected(s.mask, c)) hb.valid_ptrs[(size_t)r * ncols + c] = chunk_validity_host(t, sl.rg0 + r, c);
    if (!filtered)
        for (uint32_t r = 0; r < sl.nrg; ++r)
            for (uint32_t c = 0; c < ncols; ++c)
                if (col_selected(s.mask, c))
                    hb.col_ptrs[(size_t)r * ncols + c] =
                        hb.h_out[c].p + (t->meta.rgs[sl.rg0 + r].first_row - t->meta.rgs[sl.rg0].first_row) * hb.ob[c];
    return 0;  // the caller marks the slot busy (under s.mu)
}

static void build_records(const fls_table *t, HostBatch &hb, uint32_t rg) {
    // FSST columns delivered as lengths: this row group's string_t records,
    // rebuilt here (the consumer's thread) over the pinned heap copy -- inline
    // bytes for strings of <= 12 bytes, else a 4-byte prefix and the pointer --
    // vector by vector from each vector's heap offset (FsstVecHeader.heap_off)
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    for (uint32_t c = 0; c < ncols && !hb.strlen_w.empty(); ++c) {
        const uint8_t nw = hb.strlen_w[c];
        if (!nw) continue;
        const uint64_t i0 = t->meta.rgs[rg].first_row - t->meta.rgs[hb.rg0].first_row;
        const uint8_t *L = hb.h_out[c].p + i0 * nw;
        uint8_t *R = hb.h_rec[c].get() + i0 * 16;
        const ChunkRef &ch = t->meta.rgs[rg].chunks[c];
        const uint8_t *meta = t->img + ch.off + ch.hdr.meta_off;
        const uint8_t *heap = hb.h_heap[c].p + hb.heap_off[(size_t)(rg - hb.rg0) * ncols + c];
        const uint32_t nrows = t->meta.rgs[rg].nrows;
        for (uint32_t v = 0; v < ch.hdr.nvec; ++v) {
            VecMeta vm;
            memcpy(&vm, meta + 32ull * v, 32);
            FsstVecHeader fh;
            memcpy(&fh, t->img + ch.off + ch.hdr.aux_off + vm.aux_off, sizeof(fh));
            const uint8_t *hp = heap + fh.heap_off;
            uint64_t pos = 0;
            const uint32_t r1 = std::min(nrows, (v + 1) * kVectorSize);
            for (uint32_t i = v * kVectorSize; i < r1; ++i) {
                const uint32_t n = nw == 1 ? L[i] : nw == 2 ? ((const uint16_t *)L)[i] : ((const uint32_t *)L)[i];
                uint64_t a, b;
                memcpy(&a, hp + pos, 8);
                memcpy(&b, hp + pos + 8, 8);
                uint32_t w[4];
                w[0] = n;
                if (n <= 12) {
                    a &= n >= 8 ? ~0ull : (1ull << (8 * n)) - 1;
                    b &= n <= 8 ? 0ull : (1ull << (8 * (n - 8))) - 1;
                    w[1] = (uint32_t)a;
                    w[2] = (uint32_t)(a >> 32);
                    w[3] = (uint32_t)b;
                } else {
                    const uint64_t p = (uint64_t)(uintptr_t)(hp + pos);
                    w[1] = (uint32_t)a;
                    w[2] = (uint32_t)p;
                    w[3] = (uint32_t)(p >> 32);
                }
                memcpy(R + 16ull * i, w, 16);
                pos += n;
            }
        }
        hb.col_ptrs[(size_t)(rg - hb.rg0) * ncols + c] = R;
    }
}

int scan_start(fls_table *t, ScanCtx &s) {
    if (s.rgs.empty()) return 0;
    for (auto &d : s.devs)
        for (int si = 0; si < s.nslots; ++si) {
            int rc = enqueue_batch(t, s, *d, si);
            if (rc) return rc;
        }
    return 0;
}

// the device and host batch holding row group rg (a batch already released by
// its slot, or one a slot holds), or false if its batch is not enqueued
static bool find_batch(ScanCtx &s, uint32_t rg, int &g, HostBatch *&hb) {
    for (auto &[dg, b] : s.ready)
        if (rg >= b->rg0 && rg < b->rg0 + b->nrg) {
            g = dg;
            hb = b;
            return true;
        }
    for (size_t i = 0; i < s.devs.size(); ++i)
        for (int j = 0; j < s.nslots; ++j) {
            const Slot &sl = s.devs[i]->slots[j];
            if (sl.busy && rg >= sl.rg0 && rg < sl.rg0 + sl.nrg) {
                g = (int)i;
                hb = sl.hb;
                return true;
            }
        }
    return false;
}

// filtered batch: selected-row offsets of its row groups from the per-vector
// counts (every row group of a batch but the table's last is whole vectors)
static void batch_selection(fls_table *t, ScanCtx &s, HostBatch &hb) {
    std::lock_guard<std::mutex> lk(s.mu);
    if (hb.sel_ready) return;
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    hb.sel_off.assign(hb.nrg + 1, 0);
    uint32_t v = 0, acc = 0;
    for (uint32_t r = 0; r < hb.nrg; ++r) {
        hb.sel_off[r] = acc;
        const uint32_t nv = (t->meta.rgs[hb.rg0 + r].nrows + 1023) / 1024;
        for (uint32_t k = 0; k < nv && v < hb.nvec; ++k) acc += hb.h_counts.p[v++];
    }
    hb.sel_off[hb.nrg] = acc;
    for (uint32_t r = 0; r < hb.nrg; ++r)
        for (uint32_t c = 0; c < ncols; ++c)
            if (col_selected(s.mask, c))
                hb.col_ptrs[(size_t)r * ncols + c] = hb.h_out[c].p + (uint64_t)hb.sel_off[r] * hb.ob[c];
    hb.sel_ready = true;
}

// sticky scan error (call with s.mu held): every waiting and later acquire
// returns it instead of waiting for a batch that will never arrive
static void set_scan_error(ScanCtx &s, int rc) {
    if (rc && !s.err_rc) {
        s.err_rc = rc;
        s.err_msg = fls_last_error();
    }
}

// Claim the next row group in order and wait until its batch is decoded and
// copied back.  Its buffers stay valid until scan_release(rg).  The first
// acquire that sees a batch's D2H complete refills the batch's slot (the
// device side is idle from then on; the batch's host side, its events and
// error flags are the HostBatch's), and the batch's other row groups are found
// on s.ready: the next batch's fill, decode and D2H overlap the hand-out of
// this one's, and no consumer waits on another one's release.
static int scan_acquire(fls_table *t, ScanCtx &s, fls_rowgroup *out) {
    if (!s.active) return fail(FLS_ERR_STATE, "scan not started");
    int g = -1;
    uint32_t rg;
    HostBatch *hb = nullptr;
    {
        std::unique_lock<std::mutex> lk(s.mu);
        if (s.err_rc) return fail(s.err_rc, "%s", s.err_msg.c_str());
        if (s.cur >= s.rgs.size()) return 0;
        rg = s.rgs[s.cur++];
        // the batch holding rg is enqueued once its slot's previous batch has
        // completed (or, at the host-batch cap, once a batch is released)
        s.cv.wait(lk, [&] { return find_batch(s, rg, g, hb) || !s.active || s.err_rc != 0; });
        if (g < 0) {
            if (!s.active) return fail(FLS_ERR_STATE, "scan ended while waiting for row group %u", rg);
            return fail(s.err_rc, "%s", s.err_msg.c_str());
        }
    }
    ScanDev &d = *s.devs[g];
    auto wait_batch = [&]() -> int {
        HIP_TRY(hipSetDevice(d.dev));
        ProfTimer pw(PROF_WAIT);
        if (s.spin_wait) {  // poll the event (A/B knob FLS_SCAN_SPIN_WAIT: the blocking wait's wake-up latency)
            hipError_t q;
            while ((q = hipEventQuery(hb->done)) == hipErrorNotReady) std::this_thread::yield();
            HIP_TRY(q);
        } else {
            HIP_TRY(hipEventSynchronize(hb->done));
        }
        if (hb->prof_pending.exchange(false)) {  // the batch's stream times, once
            float dec = 0, d2h = 0;
            if (hipEventElapsedTime(&dec, hb->pt[0], hb->pt[1]) == hipSuccess &&
                hipEventElapsedTime(&d2h, hb->pt[1], hb->pt[2]) == hipSuccess) {
                ScanProf &p = scan_prof();
                p.ns[PROF_GPU_DECODE] += (uint64_t)(dec * 1e6);
                p.calls[PROF_GPU_DECODE] += 1;
                p.ns[PROF_D2H] += (uint64_t)(d2h * 1e6);
                p.bytes[PROF_D2H] += hb->prof_d2h;
                p.calls[PROF_D2H] += 1;
            }
        }
        const uint32_t err = *(volatile const uint32_t *)hb->h_err.p;
        if (err & KERR_FILTER_STR) return fail(FLS_ERR_FORMAT, "filter: string outside its batch heap (flags 0x%x)", err);
        if (err & KERR_KEYSET) return fail(FLS_ERR_FORMAT, "filter: damaged key-set descriptor (flags 0x%x)", err);
        if (err & KERR_PATTERN) return fail(FLS_ERR_FORMAT, "filter: damaged pattern descriptor (flags 0x%x)", err);
        if (err & KERR_COLCMP)
            return fail(FLS_ERR_FORMAT, "filter: damaged column-comparison descriptor (flags 0x%x)", err);
        if (err & KERR_MAPCMP)
            return fail(FLS_ERR_FORMAT, "filter: damaged map-comparison descriptor (flags 0x%x)", err);
        if (err & KERR_KEYMAP) return fail(FLS_ERR_FORMAT, "grouped aggregate: damaged key-map descriptor (flags 0x%x)", err);
        if (err & KERR_MAPVAL)
            return fail(FLS_ERR_FORMAT, "aggregate: damaged mapped-column descriptor (flags 0x%x)", err);
        if (err & KERR_KEYBUILD)
            return fail(FLS_ERR_FORMAT, "corrupt chunk: a value outside its zone map in a key-set build's key column "
                        "(flags 0x%x)", err);
        if (err & KERR_MAPBUILD)
            return fail(FLS_ERR_FORMAT, "corrupt chunk: a value outside its zone map in a map build's key column "
                        "(flags 0x%x)", err);
        // (fls_valuemap_from_scan / fls_keymap_from_scan name the key from the GPU's conflict cell)
        if (err & KERR_MAPBUILD_CONFLICT)
            return fail(FLS_ERR_ARG, "map build: a key is listed with two values: a map is a function (flags 0x%x)", err);
        if (err & KERR_NARROW)
            return fail(FLS_ERR_FORMAT, "corrupt chunk: a value outside its zone map in a narrowed column (flags 0x%x)", err);
        if (err & KERR_HASH_RANGE)
            return fail(FLS_ERR_FORMAT, "corrupt chunk: a value outside its zone map in a hash aggregate's key column "
                        "(flags 0x%x)", err);
        if (err & KERR_LDS_BASE) return fail(FLS_ERR_DEVICE, "FSST kernel: dynamic LDS not at address 0 (flags 0x%x)", err);
        // a grouped aggregate past its capacity: the kernels stopped before they wrote past a table
        if (err == KERR_GROUP_RG)
            return fail(FLS_ERR_LIMIT,
                        "grouped aggregate: more than %u distinct keys in one row group (kMaxRgGroups); fall back to a "
                        "scan and group its rows (flags 0x%x)", kMaxRgGroups, err);
        if (err && !(err & ~(KERR_GROUP_VEC | KERR_GROUP_RG)))
            return fail(FLS_ERR_LIMIT,
                        "grouped aggregate: more than %u distinct keys among the selected rows of one 1024-row vector "
                        "(kMaxVecGroups); fall back to a scan and group its rows (flags 0x%x)", kMaxVecGroups, err);
        // a hash aggregate past its table: the kernel dropped the rows it had no group for
        if (err == KERR_HASH_LIMIT)
            return fail(FLS_ERR_LIMIT,
                        "hash aggregate: more than max_groups = %llu distinct keys among the selected rows of one "
                        "pipeline's row groups; call again with a larger max_groups (flags 0x%x)",
                        (unsigned long long)s.max_groups, err);
        if (err) return fail(FLS_ERR_FORMAT, "corrupt chunk detected while decoding (flags 0x%x)", err);
        return 0;
    };
    if (int rc = wait_batch()) {
        std::lock_guard<std::mutex> lk(s.mu);
        set_scan_error(s, rc);
        s.cv.notify_all();
        return rc;
    }
    ProfTimer seen(PROF_REFILL_LAT);  // this acquire saw the batch complete: until its refill starts
    // the batch's upload into the resident image is complete (its event covers
    // the H2D): later scans of this file may decode these row groups from it
    if (hb->upload_resident.exchange(false) && d.dimg)
        for (uint32_t r = hb->rg0; r < hb->rg0 + hb->nrg; ++r) d.dimg->present[r].store(1, std::memory_order_release);
    const uint32_t ncols = (uint32_t)t->meta.cols.size();
    out->rowgroup = rg;
    out->nrows = t->meta.rgs[rg].nrows;
    out->first_row = t->meta.row_offset + t->meta.rgs[rg].first_row;
    out->ncols = ncols;
    out->nrows_scanned = out->nrows;
    out->sel = nullptr;
    if (s.masked() && s.reduce == Reduce::None) {
        batch_selection(t, s, *hb);
        const uint32_t i = rg - hb->rg0;
        out->nrows = hb->sel_off[i + 1] - hb->sel_off[i];
        out->sel = hb->h_sel.p + hb->sel_off[i];
    }
    out->columns = hb->col_ptrs.data() + (size_t)(rg - hb->rg0) * ncols;
    out->validity = hb->valid_ptrs.data() + (size_t)(rg - hb->rg0) * ncols;
    out->dict = hb->dict_ptrs.data() + (size_t)(rg - hb->rg0) * ncols;
    out->dict_size = hb->dict_sizes.data() + (size_t)(rg - hb->rg0) * ncols;
    out->dict_width = hb->ob_out.data();
    out->narrow = hb->narrow_out.data();
    out->narrow_base = hb->nbase.data() + (size_t)(rg - hb->rg0) * ncols;
    if (!s.defer_records) build_records(t, *hb, rg);
    if (out->sel) {  // filtered: the delivered rows' validity, gathered through sel
        const size_t i0 = (size_t)(rg - hb->rg0) * ncols;
        for (uint32_t c = 0; c < ncols; ++c) {
            const uint64_t *img = col_selected(s.mask, c) ? chunk_validity_host(t, rg, c) : nullptr;
            hb->valid_ptrs[i0 + c] = nullptr;
            if (!img) continue;
            std::vector<uint64_t> &w = hb->vbits[i0 + c];
            w.assign(std::max<size_t>(1, (out->nrows + 63) / 64), 0);
            bool any_null = false;
            for (uint32_t i = 0; i < out->nrows; ++i) {
                const uint32_t r = out->sel[i];
                const uint64_t b = (img[r >> 6] >> (r & 63)) & 1;
                w[i >> 6] |= b << (i & 63);
                any_null |= !b;
            }
            if (any_null) hb->valid_ptrs[i0 + c] = w.data();
        }
    }
    bool refill = false;
    int si = -1;
    std::shared_ptr<DevImage> done_img;  // dropped outside s.mu
    {
        std::lock_guard<std::mutex> lk(s.mu);
        s.out.emplace_back(rg, hb);
        const bool last = ++hb->handed == hb->nrg;
        // the batch's D2H is complete: if its slot still holds it, the slot
        // takes its next batch now (FLS_SCAN_EARLY_REFILL=0: once the batch's
        // last row group is handed out) and the batch moves to s.ready
        if (last || s.early_refill)
            for (int k = 0; k < s.nslots && si < 0; ++k)
                if (d.slots[k].busy && d.slots[k].hb == hb) si = k;
        if (si >= 0) {
            s.ready.emplace_back(g, hb);
            // a failed refill does not take this row group back: it is delivered,
            // and the error surfaces at the next acquire
            const int c = claim_batch(t, s, d, si);
            set_scan_error(s, c < 0 ? c : 0);
            refill = c == 1;
            // this GPU's last batch is decoded: the scan no longer holds its
            // resident image, which becomes evictable (the table may stay open)
            if (c == 0 && d.next_p >= d.p1 && d.dimg) {
                bool idle = true;
                for (int k = 0; k < s.nslots; ++k) idle = idle && !d.slots[k].busy && !d.slots[k].filling;
                if (idle) done_img = std::move(d.dimg);
            }
        }
        if (last)  // every row group of the batch handed out
            for (size_t i = 0; i < s.ready.size(); ++i)
                if (s.ready[i].second == hb) {
                    s.ready.erase(s.ready.begin() + (long)i);
                    break;
                }
        s.cv.notify_all();
    }
    if (!refill) seen.cancel();
    seen.stop();
    if (refill) {  // the slot's next batch, outside s.mu (claim_batch)
        Slot &sl = d.slots[si];
        const int rc = fill_batch(t, s, d, si);
        std::lock_guard<std::mutex> lk(s.mu);
        sl.filling = false;
        sl.busy = rc == 0;
        set_scan_error(s, rc);
        s.cv.notify_all();
    }
    return 1;
}

static int scan_release(fls_table *t, ScanCtx &s, uint32_t rg) {
    std::lock_guard<std::mutex> lk(s.mu);
    auto it = std::find_if(s.out.begin(), s.out.end(), [&](const auto &o) { return o.first == rg; });
    if (!s.active || it == s.out.end()) return fail(FLS_ERR_ARG, "row group %u is not held by this scan", rg);
    HostBatch *hb = it->second;
    s.out.erase(it);
    if (++hb->released < hb->nrg) return 0;
    // every row group of the batch is back: its host side returns to the pool,
    // and a slot whose refill waited for one goes now
    int rc = 0;
    for (auto &dp : s.devs) {
        ScanDev &d = *dp;
        bool mine = false;
        for (auto &b : d.batches) mine = mine || b.get() == hb;
        if (!mine) continue;
        d.free_batches.push_back(hb);
        for (int si = 0; si < s.nslots && !rc; ++si)
            if (d.slots[si].starved) {
                rc = enqueue_batch(t, s, d, si);
                set_scan_error(s, rc);
            }
        break;
    }
    s.cv.notify_all();
    return rc;
}

// single-consumer form: releases the previously delivered row group
int scan_next(fls_table *t, ScanCtx &s, fls_rowgroup *out) {
    if (s.held >= 0) {
        const uint32_t prev = (uint32_t)s.held;
        s.held = -1;
        int rc = scan_release(t, s, prev);
        if (rc) return rc;
    }
    int rc = scan_acquire(t, s, out);
    if (rc == 1) s.held = out->rowgroup;
    return rc;
}

// fls_predicate[] -> host terms in the comparison domain, sorted by clause;
// *at (if given): the term a refusal is about
static int to_terms(const fls_table *t, const fls_predicate *p, uint32_t n, std::vector<HostTerm> &out,
                    uint32_t *at = nullptr) {
    out.clear();
    if (n && !p) return fail(FLS_ERR_ARG, "fls_scan_filter: NULL predicates");
    for (uint32_t i = 0; i < n; ++i) {
        if (at) *at = i;
        if (is_mapped_col(p[i].col))
            return fail(FLS_ERR_ARG, "a mapped column (FLS_COL_MAPPED) cannot be a filter term's column; `col op "
                        "map[key]` is a map term (FLS_CMP_MAP_EQ .. FLS_CMP_MAP_GE)");
        if (p[i].col >= t->meta.cols.size()) return fail(FLS_ERR_ARG, "filter column %u out of range", p[i].col);
        if (p[i].op > FLS_CMP_MAP_GE) return fail(FLS_ERR_ARG, "filter operator %u unknown", p[i].op);
        HostTerm h;
        h.col = p[i].col;
        h.clause = p[i].clause;
        h.op = p[i].op;
        const uint8_t ty = t->meta.cols[h.col].type;
        if (is_set_op(h.op)) {
            const ColumnMeta &cm = t->meta.cols[h.col];
            if (type_is_string(ty) || type_is_float(ty) || !type_valid(ty))
                return fail(FLS_ERR_ARG, "filter term %u: a key set cannot be probed with a VARCHAR / BLOB / FLOAT / "
                            "DOUBLE column (%u)", i, h.col);
            if (ty == TY_DECIMAL && cm.width > 18)
                return fail(FLS_ERR_ARG, "filter term %u: a key set cannot be probed with a DECIMAL wider than 64 bits "
                            "(column %u)", i, h.col);
            h.set = keyset_registry().find(p[i].value);
            if (!h.set)
                return fail(FLS_ERR_ARG, "filter term %u: value 0x%llx is not a live key set", i,
                            (unsigned long long)p[i].value);
            if (h.set->img.is_signed != type_is_signed(ty))
                return fail(FLS_ERR_ARG, "filter term %u: the key set's kind is %s, column %u is %s", i,
                            h.set->img.is_signed ? "signed" : "unsigned", h.col,
                            type_is_signed(ty) ? "signed" : "unsigned");
            for (uint32_t j = 0; j < n; ++j)
                if (j != i && p[j].clause == p[i].clause)
                    return fail(FLS_ERR_ARG, "filter term %u: a key-set term shares clause %u with term %u (a set "
                                "term is a clause of its own)", i, p[i].clause, j);
            h.kind = type_is_signed(ty) ? FK_INT : FK_UINT;
        } else if (is_col_op(h.op)) {
            // `column op column`: value is the right column; both sides in one comparison domain
            if (p[i].value >= t->meta.cols.size())
                return fail(FLS_ERR_ARG, "filter term %u: right column %llu out of range (left column %u, %zu columns)",
                            i, (unsigned long long)p[i].value, h.col, t->meta.cols.size());
            h.col2 = (uint32_t)p[i].value;
            const ColumnMeta &ca = t->meta.cols[h.col], &cb = t->meta.cols[h.col2];
            const uint8_t tb = cb.type;
            if (type_is_string(ty) || type_is_string(tb) || !type_valid(ty) || !type_valid(tb))
                return fail(FLS_ERR_ARG, "filter term %u: a column comparison cannot read a VARCHAR / BLOB column "
                            "(columns %u and %u)", i, h.col, h.col2);
            if (type_is_float(ty) != type_is_float(tb))
                return fail(FLS_ERR_ARG, "filter term %u: an integer-like column against a FLOAT / DOUBLE column "
                            "(columns %u and %u)", i, h.col, h.col2);
            if ((ty == TY_DATE) != (tb == TY_DATE))
                return fail(FLS_ERR_ARG, "filter term %u: a DATE column against a non-DATE column (columns %u and %u)",
                            i, h.col, h.col2);
            if ((ty == TY_DECIMAL) != (tb == TY_DECIMAL))
                return fail(FLS_ERR_ARG, "filter term %u: a DECIMAL column against a non-DECIMAL column (columns %u "
                            "and %u)", i, h.col, h.col2);
            if (ty == TY_DECIMAL && (ca.width > 18 || cb.width > 18))
                return fail(FLS_ERR_ARG, "filter term %u: a column comparison cannot read a DECIMAL wider than 64 bits "
                            "(columns %u and %u)", i, h.col, h.col2);
            if (ty == TY_DECIMAL && ca.scale != cb.scale)
                return fail(FLS_ERR_ARG, "filter term %u: DECIMALs of different scale, %u and %u (columns %u and %u)",
                            i, (uint32_t)ca.scale, (uint32_t)cb.scale, h.col, h.col2);
            if (!type_is_float(ty) && type_is_signed(ty) != type_is_signed(tb))
                return fail(FLS_ERR_ARG, "filter term %u: a signed column against an unsigned column (columns %u and "
                            "%u)", i, h.col, h.col2);
            for (uint32_t j = 0; j < n; ++j)
                if (j != i && p[j].clause == p[i].clause)
                    return fail(FLS_ERR_ARG, "filter term %u: a column term shares clause %u with term %u (a column "
                                "term is a clause of its own; columns %u and %u)", i, p[i].clause, j, h.col, h.col2);
            h.kind = col_kind(t, h.col);
        } else if (is_map_op(h.op)) {
            // `column op map[key column]`: value is the value map's handle, key_col the key column
            const uint32_t kc = p[i].key_col;
            if (kc >= t->meta.cols.size())
                return fail(FLS_ERR_ARG, "filter term %u: key column %u out of range (left column %u, %zu columns)", i,
                            kc, h.col, t->meta.cols.size());
            h.col2 = kc;
            const ColumnMeta &ca = t->meta.cols[h.col], &ck = t->meta.cols[kc];
            const uint8_t tk = ck.type;
            if (type_is_string(ty) || type_is_string(tk) || type_is_float(ty) || type_is_float(tk) || !type_valid(ty) ||
                !type_valid(tk))
                return fail(FLS_ERR_ARG, "filter term %u: a map term cannot read a VARCHAR / BLOB / FLOAT / DOUBLE "
                            "column (left column %u, key column %u)", i, h.col, kc);
            if ((ty == TY_DECIMAL && ca.width > 18) || (tk == TY_DECIMAL && ck.width > 18))
                return fail(FLS_ERR_ARG, "filter term %u: a map term cannot read a DECIMAL wider than 64 bits (left "
                            "column %u, key column %u)", i, h.col, kc);
            h.map = valuemap_registry().find(p[i].value);
            if (!h.map)
                // (worded as LIKE's refusal on a non-VARCHAR column is: without a live map the operator means nothing)
                return fail(FLS_ERR_ARG, "filter term %u: filter operator %u unknown for value 0x%llx: not a live value "
                            "map (left column %u, key column %u)", i, h.op, (unsigned long long)p[i].value, h.col, kc);
            const ValuemapImage &vi = h.map->img;
            if (vi.value_signed != type_is_signed(ty))
                return fail(FLS_ERR_ARG, "filter term %u: the value map's value kind is %s, left column %u is %s (key "
                            "column %u)", i, vi.value_signed ? "signed" : "unsigned", h.col,
                            type_is_signed(ty) ? "signed" : "unsigned", kc);
            if (vi.set.is_signed != type_is_signed(tk))
                return fail(FLS_ERR_ARG, "filter term %u: the value map's key kind is %s, key column %u is %s (left "
                            "column %u)", i, vi.set.is_signed ? "signed" : "unsigned", kc,
                            type_is_signed(tk) ? "signed" : "unsigned", h.col);
            for (uint32_t j = 0; j < n; ++j)
                if (j != i && p[j].clause == p[i].clause)
                    return fail(FLS_ERR_ARG, "filter term %u: a map term shares clause %u with term %u (a map term is "
                                "a clause of its own; left column %u, key column %u)", i, p[i].clause, j, h.col, kc);
            uint32_t nmap = 0;
            for (uint32_t j = 0; j <= i; ++j) nmap += p[j].op >= FLS_CMP_MAP_EQ && p[j].op <= FLS_CMP_MAP_GE;
            if (nmap > kMaxMapTerms)
                return fail(FLS_ERR_ARG, "filter term %u: more than %u map terms in one term list (left column %u, key "
                            "column %u)", i, kMaxMapTerms, h.col, kc);
            h.kind = vi.value_signed ? FK_INT : FK_UINT;
        } else if (is_pat_op(h.op)) {
            if (ty != TY_VARCHAR)
                return fail(FLS_ERR_ARG, "filter term %u: filter operator %u unknown for column %u: LIKE needs a "
                            "VARCHAR column", i, h.op, h.col);
            if (p[i].str_len && !p[i].str) return fail(FLS_ERR_ARG, "filter term %u: NULL pattern string", i);
            if (p[i].value > 255)
                return fail(FLS_ERR_ARG, "filter term %u: escape 0x%llx is not a byte (0: none)", i,
                            (unsigned long long)p[i].value);
            for (uint32_t j = 0; j < n; ++j)
                if (j != i && p[j].clause == p[i].clause)
                    return fail(FLS_ERR_ARG, "filter term %u: a pattern term shares clause %u with term %u (a pattern "
                                "term is a clause of its own)", i, p[i].clause, j);
            uint32_t npat = 0;
            for (uint32_t j = 0; j <= i; ++j) npat += p[j].op == FLS_CMP_LIKE || p[j].op == FLS_CMP_NOT_LIKE;
            if (npat > kMaxPatTerms)
                return fail(FLS_ERR_ARG, "filter term %u: more than %u pattern terms in one filter", i, kMaxPatTerms);
            // the compiler stops at token kMaxPatTokens + 1: an oversized pattern is refused after bounded work
            auto cp = std::make_shared<CompiledPattern>();
            const int rc = pattern_compile((const uint8_t *)p[i].str, (size_t)p[i].str_len, (uint32_t)p[i].value, *cp);
            if (rc == PAT_TRAILING_ESCAPE)
                return fail(FLS_ERR_ARG, "filter term %u: the pattern ends in its escape byte", i);
            if (rc == PAT_TOO_LONG)
                return fail(FLS_ERR_ARG, "filter term %u: the pattern compiles to more than %u tokens", i, kMaxPatTokens);
            h.pat = std::move(cp);
            h.kind = FK_STR;
        } else if (type_is_string(ty)) {
            h.kind = FK_STR;
            if (p[i].str_len && !p[i].str) return fail(FLS_ERR_ARG, "filter on column %u: NULL string", h.col);
            if (p[i].str_len > 0xFFFFFFFFull) return fail(FLS_ERR_ARG, "filter string too long");
            if (p[i].str_len) h.str.assign(p[i].str, p[i].str_len);
        } else if (type_is_float(ty)) {
            h.kind = FK_FLOAT;
            double d;
            if (ty == TY_FLOAT) {
                float f;
                const uint32_t b = (uint32_t)p[i].value;
                memcpy(&f, &b, 4);
                d = f;
            } else {
                memcpy(&d, &p[i].value, 8);
            }
            memcpy(&h.value, &d, 8);
        } else {
            h.kind = type_is_signed(ty) ? FK_INT : FK_UINT;
            h.value = p[i].value;
        }
        out.push_back(std::move(h));
    }
    std::stable_sort(out.begin(), out.end(), [](const HostTerm &a, const HostTerm &b) { return a.clause < b.clause; });
    return 0;
}

static int open_common(fls_connection *conn, fls_table *t, fls_table **out) {
    std::string why = parse_file(t->img, t->len, t->meta);
    if (!why.empty()) {
        delete t;
        return fail(FLS_ERR_FORMAT, "not a valid FastLanes file: %s", why.c_str());
    }
    t->devices = conn->devices;
    t->res = conn->res;
    t->conn = conn;
    for (auto &c : t->meta.cols) t->names.push_back(c.name);
    *out = t;
    if (debug_enabled())
        fprintf(stderr, "DEBUG: FLS file opened: %zu columns, %llu rows, %zu row groups\n", t->meta.cols.size(),
                (unsigned long long)t->meta.nrows, t->meta.rgs.size());
    return 0;
}


// The host batch that holds row group rg of the aggregate scan s.
const HostBatch *held_batch(ScanCtx &s, uint32_t rg) {
    std::lock_guard<std::mutex> lk(s.mu);
    for (const auto &o : s.out)
        if (o.first == rg) return o.second;
    return nullptr;
}

FLS_ENGINE_END

// ------------------------------------------------------------------------------
// C-ABI

extern "C" {

const char *fls_last_error(void) { return last_error().c_str(); }

const char *fls_version(void) { return "fastlanes-mi355x 0.1.0 (gfx950)"; }

int fls_config_default(const char *name, int64_t *value) {
    const Knob *k = find_knob(name);
    if (!k || !value) return fail(FLS_ERR_ARG, "fls_config_default: '%s' is not a knob", name ? name : "(null)");
    *value = k->def;
    return 0;
}

int fls_config_value(const char *name, int64_t *value) {
    if (!find_knob(name) || !value) return fail(FLS_ERR_ARG, "fls_config_value: '%s' is not a knob", name ? name : "(null)");
    *value = knob_value(name);
    return 0;
}

int fls_config_count(void) { return (int)(sizeof(kKnobs) / sizeof(kKnobs[0])); }

const char *fls_config_name(int i) {
    return i >= 0 && i < fls_config_count() ? kKnobs[i].name : nullptr;
}


int fls_connect(const int *devices, int ndevices, fls_connection **out) {
    if (!out) return fail(FLS_ERR_ARG, "fls_connect: NULL out");
    auto *c = new fls_connection();
    if (devices && ndevices > 0) c->devices.assign(devices, devices + ndevices);
    else c->devices.push_back(0);
    *out = c;
    return 0;
}

void fls_disconnect(fls_connection *conn) {
    if (conn) {  // the connection's key sets go with it (a filter or scan still using one keeps it alive)
        KeySetRegistry &R = keyset_registry();
        std::vector<std::shared_ptr<KeySet>> dead;  // released outside the lock
        std::lock_guard<std::mutex> lk(R.mu);
        for (auto it = R.live.begin(); it != R.live.end();) {
            if (it->second->conn == conn) {
                dead.push_back(std::move(it->second));
                it = R.live.erase(it);
            } else {
                ++it;
            }
        }
    }
    if (conn) {  // ... and its key maps (a binding or scan still using one keeps it alive)
        KeyMapRegistry &R = keymap_registry();
        std::vector<std::shared_ptr<KeyMap>> dead;  // released outside the lock
        std::lock_guard<std::mutex> lk(R.mu);
        for (auto it = R.live.begin(); it != R.live.end();) {
            if (it->second->conn == conn) {
                dead.push_back(std::move(it->second));
                it = R.live.erase(it);
            } else {
                ++it;
            }
        }
    }
    if (conn) {  // ... and its value maps (a filter or scan still using one keeps it alive)
        ValueMapRegistry &R = valuemap_registry();
        std::vector<std::shared_ptr<ValueMap>> dead;  // released outside the lock
        std::lock_guard<std::mutex> lk(R.mu);
        for (auto it = R.live.begin(); it != R.live.end();) {
            if (it->second->conn == conn) {
                dead.push_back(std::move(it->second));
                it = R.live.erase(it);
            } else {
                ++it;
            }
        }
    }
    delete conn;
}


int fls_release_device_memory(int device, uint64_t *freed_bytes) {
    const uint64_t b = release_idle_images(device < 0 ? -1 : device);
    if (freed_bytes) *freed_bytes = b;
    return 0;
}

int fls_resident_info(int device, uint64_t *bytes, uint32_t *images) {
    ImageRegistry &R = image_registry();
    std::lock_guard<std::mutex> lk(R.mu);
    const int dv = device < 0 ? -1 : device;
    if (bytes) *bytes = R.set.used(dv);
    if (images) *images = (uint32_t)R.set.count(dv);
    return 0;
}

int fls_connection_trim(fls_connection *conn, uint64_t keep_bytes, uint64_t *idle_bytes) {
    if (!conn) return fail(FLS_ERR_ARG, "fls_connection_trim: NULL connection");
    {
        std::lock_guard<std::mutex> lk(conn->res->mu);
        conn->res->trim_locked(-1, (size_t)keep_bytes);
    }
    if (idle_bytes) *idle_bytes = conn->res->idle_pinned();
    return 0;
}

}  // extern "C"

namespace {
// The validated-file cache (MappedFile): the FLS_OPEN_CACHE most recently
// opened files (default 16, 0 = off) stay mapped with their metadata.  The
// key changes whenever the file is replaced or rewritten through the file
// system (inode, size, mtime in ns).
struct FileKey {
    uint64_t dev, ino, size;
    int64_t mtime_s, mtime_ns;
    bool operator==(const FileKey &o) const {
        return dev == o.dev && ino == o.ino && size == o.size && mtime_s == o.mtime_s && mtime_ns == o.mtime_ns;
    }
};
struct FileCache {
    std::mutex mu;
    std::vector<std::pair<FileKey, std::shared_ptr<MappedFile>>> lru;  // most recent last
    static size_t capacity() {
        static const size_t cap = (size_t)std::max<int64_t>(0, knob_value("FLS_OPEN_CACHE"));
        return cap;
    }
    std::shared_ptr<MappedFile> find(const FileKey &k) {
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = 0; i < lru.size(); ++i)
            if (lru[i].first == k) {
                auto hit = lru[i];
                lru.erase(lru.begin() + (long)i);
                lru.push_back(hit);
                return hit.second;
            }
        return nullptr;
    }
    void put(const FileKey &k, std::shared_ptr<MappedFile> m) {
        if (capacity() == 0) return;
        std::lock_guard<std::mutex> lk(mu);
        lru.emplace_back(k, std::move(m));
        while (lru.size() > capacity()) lru.erase(lru.begin());
    }
};
FileCache &file_cache() {
    static FileCache *c = new FileCache();  // process lifetime (tables may outlive static destruction order)
    return *c;
}
}  // namespace

extern "C" {

int fls_read_fls(fls_connection *conn, const char *path, fls_table **out) {
    if (!conn || !path || !out) return fail(FLS_ERR_ARG, "fls_read_fls: NULL argument");
    // map the file: opening reads only the footer and the chunk headers it
    // validates (DuckDB opens a file at bind and at init), the scan streams
    // the row groups it keeps
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(FLS_ERR_IO, "Failed to open FastLanes file: %s", path);
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
        close(fd);
        return fail(FLS_ERR_IO, "Failed to open FastLanes file: %s", path);
    }
    const FileKey key{(uint64_t)st.st_dev, (uint64_t)st.st_ino, (uint64_t)st.st_size, (int64_t)st.st_mtim.tv_sec,
                      (int64_t)st.st_mtim.tv_nsec};
    if (FileCache::capacity() > 0 && st.st_size > 0) {
        if (std::shared_ptr<MappedFile> hit = file_cache().find(key)) {  // unchanged file: already validated
            close(fd);
            auto *t = new fls_table();
            t->mapped = hit;
            t->img = (const uint8_t *)hit->map;
            t->len = hit->len;
            t->meta = hit->meta;
            t->devices = conn->devices;
            t->res = conn->res;
            t->conn = conn;
            for (auto &c : t->meta.cols) t->names.push_back(c.name);
            *out = t;
            return 0;
        }
    }
    auto *t = new fls_table();
    const size_t n = (size_t)st.st_size;
    if (n > 0) {
        void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) {  // e.g. a pipe-backed or special file system: read it
            t->owned.resize(n);
            size_t got = 0;
            while (got < n) {
                const ssize_t r = pread(fd, t->owned.data() + got, n - got, (off_t)got);
                if (r <= 0) break;
                got += (size_t)r;
            }
            if (got != n) { close(fd); delete t; return fail(FLS_ERR_IO, "short read of %s", path); }
            t->img = t->owned.data();
        } else {
            t->map = m;
            t->map_len = n;
            t->img = (const uint8_t *)m;
        }
    }
    close(fd);
    t->len = (uint64_t)n;
    const int rc = open_common(conn, t, out);
    if (rc == 0 && t->map && FileCache::capacity() > 0) {  // share the mapping and the validated metadata
        auto mf = std::make_shared<MappedFile>();
        mf->map = t->map;
        mf->len = t->map_len;
        mf->meta = t->meta;
        t->map = nullptr;  // owned by mf now
        t->mapped = mf;
        file_cache().put(key, std::move(mf));
    }
    return rc;
}

int fls_read_fls_image(fls_connection *conn, const void *img, uint64_t len, int copy, fls_table **out) {
    if (!conn || !img || !out) return fail(FLS_ERR_ARG, "fls_read_fls_image: NULL argument");
    auto *t = new fls_table();
    if (copy) {
        t->owned.assign((const uint8_t *)img, (const uint8_t *)img + len);
        t->img = t->owned.data();
    } else {
        t->img = (const uint8_t *)img;
    }
    t->len = len;
    return open_common(conn, t, out);
}

void fls_table_close(fls_table *t) { delete t; }

uint32_t fls_table_ncols(const fls_table *t) { return t ? (uint32_t)t->meta.cols.size() : 0; }
uint64_t fls_table_nrows(const fls_table *t) { return t ? t->meta.nrows : 0; }
uint64_t fls_table_row_offset(const fls_table *t) { return t ? t->meta.row_offset : 0; }
uint32_t fls_table_nrowgroups(const fls_table *t) { return t ? (uint32_t)t->meta.rgs.size() : 0; }
int64_t fls_table_rowgroup_rows(const fls_table *t, uint32_t rg) {
    if (!t || rg >= t->meta.rgs.size()) return fail(FLS_ERR_ARG, "row group %u out of range", rg);
    return t->meta.rgs[rg].nrows;
}

int fls_table_column(const fls_table *t, uint32_t col, fls_column_info *out) {
    if (!t || !out || col >= t->meta.cols.size()) return fail(FLS_ERR_ARG, "column %u out of range", col);
    const ColumnMeta &c = t->meta.cols[col];
    out->name = t->names[col].c_str();
    out->type = c.type;
    out->width = c.width;
    out->scale = c.scale;
    out->out_bytes = (uint8_t)type_out_bytes(c.type);
    return 0;
}

int fls_materialize(fls_table *t, uint32_t rg, const uint8_t *col_mask, fls_rowgroup *out) {
    if (!t || !out) return fail(FLS_ERR_ARG, "fls_materialize: NULL argument");
    if (rg >= t->meta.rgs.size()) return fail(FLS_ERR_ARG, "row group %u out of range", rg);
    // a one-row-group scan on the GPU that owns rg in a full-table sharding
    const uint32_t G = (uint32_t)t->devices.size(), N = (uint32_t)t->meta.rgs.size();
    uint32_t g = 0;
    while (g + 1 < G && rg >= (uint64_t)N * (g + 1) / G) ++g;
    ScanPlan plan;
    plan.devices = {t->devices[g]};
    plan.col_mask = col_mask;
    plan.rg0 = rg;
    plan.rg1 = rg + 1;
    int rc = scan_setup(t, t->mat, plan);
    if (!rc) rc = scan_start(t, t->mat);
    if (rc) return rc;
    rc = scan_next(t, t->mat, out);
    return rc == 1 ? 0 : (rc == 0 ? fail(FLS_ERR_STATE, "internal: empty materialize") : rc);
}

int fls_scan_begin(fls_table *t, const uint8_t *col_mask, uint32_t rg_begin, uint32_t rg_end) {
    if (!t) return fail(FLS_ERR_ARG, "fls_scan_begin: NULL table");
    ScanPlan plan;
    plan.devices = t->devices;
    plan.col_mask = col_mask;
    plan.rg0 = rg_begin;
    plan.rg1 = rg_end;
    plan.filter = &t->filter;
    plan.alts = &t->alts;
    plan.delivering_scan = true;
    int rc = scan_setup(t, t->scan, plan);
    if (rc) return rc;
    return scan_start(t, t->scan);
}

int fls_scan_filter(fls_table *t, const fls_predicate *preds, uint32_t n) {
    if (!t) return fail(FLS_ERR_ARG, "fls_scan_filter: NULL table");
    std::vector<HostTerm> terms;
    int rc = to_terms(t, preds, n, terms);
    if (rc) return rc;
    t->filter.swap(terms);
    return 0;
}

int fls_scan_filter_alternatives(fls_table *t, const fls_predicate *preds, uint32_t npreds,
                                 const fls_filter_alternative *alts, uint32_t nalts) {
    if (!t || (!alts && nalts) || (!preds && npreds))
        return fail(FLS_ERR_ARG, "fls_scan_filter_alternatives: NULL argument");
    if (nalts > kMaxConds)
        return fail(FLS_ERR_ARG, "fls_scan_filter_alternatives: %u alternatives (at most %u)", nalts, kMaxConds);
    std::vector<std::vector<HostTerm>> list(nalts);
    for (uint32_t i = 0; i < nalts; ++i) {
        const fls_filter_alternative &a = alts[i];
        if (a.n == 0) return fail(FLS_ERR_ARG, "alternative %u: no term (an alternative has at least one)", i);
        if (a.first > npreds || a.n > npreds - a.first)
            return fail(FLS_ERR_ARG, "alternative %u: terms [%u, %llu) past the %u predicates", i, a.first,
                        (unsigned long long)a.first + a.n, npreds);
        uint32_t at = 0;
        if (int rc = to_terms(t, preds + a.first, a.n, list[i], &at)) {
            const std::string why = fls_last_error();  // (the filter's refusal, its term numbers local to the alternative)
            return fail(rc, "alternative %u, term %u: %s", i, at, why.c_str());
        }
    }
    t->alts.swap(list);
    return 0;
}

int fls_aggregate_conditions(fls_table *t, const fls_predicate *preds, uint32_t npreds, const fls_agg_condition *conds,
                             uint32_t nconds) {
    if (!t || (!conds && nconds) || (!preds && npreds)) return fail(FLS_ERR_ARG, "fls_aggregate_conditions: NULL argument");
    if (nconds > kMaxConds)
        return fail(FLS_ERR_ARG, "fls_aggregate_conditions: %u conditions (at most %u)", nconds, kMaxConds);
    std::vector<std::vector<HostTerm>> list(nconds);
    for (uint32_t i = 0; i < nconds; ++i) {
        const fls_agg_condition &c = conds[i];
        if (c.n == 0) return fail(FLS_ERR_ARG, "condition %u: no term (a condition has at least one)", i);
        if (c.first > npreds || c.n > npreds - c.first)
            return fail(FLS_ERR_ARG, "condition %u: terms [%u, %llu) past the %u predicates", i, c.first,
                        (unsigned long long)c.first + c.n, npreds);
        uint32_t at = 0;
        if (int rc = to_terms(t, preds + c.first, c.n, list[i], &at)) {
            const std::string why = fls_last_error();  // (the filter's refusal, its term numbers local to the condition)
            return fail(rc, "condition %u, term %u: %s", i, at, why.c_str());
        }
    }
    t->conds.swap(list);
    return 0;
}

int fls_scan_pruned(const fls_table *t) {
    if (!t) return fail(FLS_ERR_ARG, "fls_scan_pruned: NULL table");
    return (int)t->scan.pruned;
}

int fls_table_zonemap(const fls_table *t, uint32_t rg, uint32_t col, uint64_t *min, uint64_t *max, uint32_t *flags) {
    if (!t || rg >= t->meta.rgs.size() || col >= t->meta.cols.size())
        return fail(FLS_ERR_ARG, "zone map (%u, %u) out of range", rg, col);
    const auto &z = t->meta.rgs[rg].zones;
    if (z.empty() || !(z[col].flags & (ZM_VALID | ZM_HAS_NULL | ZM_ALL_NULL))) return 0;
    if (min) *min = z[col].min;
    if (max) *max = z[col].max;
    if (flags) *flags = z[col].flags;
    return 1;
}

int fls_scan_narrow(fls_table *t, int enable) {
    if (!t) return fail(FLS_ERR_ARG, "fls_scan_narrow: NULL table");
    t->narrow = enable != 0;
    return 0;
}

int fls_scan_defer_records(fls_table *t, int enable) {
    if (!t) return fail(FLS_ERR_ARG, "fls_scan_defer_records: NULL table");
    t->defer_records = enable != 0;
    return 0;
}

int fls_scan_build_records(fls_table *t, const fls_rowgroup *rg) {
    if (!t || !rg) return fail(FLS_ERR_ARG, "fls_scan_build_records: NULL argument");
    HostBatch *hb = nullptr;
    {
        std::lock_guard<std::mutex> lk(t->scan.mu);
        for (const auto &o : t->scan.out)
            if (o.first == rg->rowgroup) hb = o.second;
    }
    if (!hb) return fail(FLS_ERR_ARG, "fls_scan_build_records: row group %u is not held by this scan", rg->rowgroup);
    if (t->scan.defer_records) build_records(t, *hb, rg->rowgroup);
    return 0;
}

int fls_scan_dict_codes(fls_table *t, int enable) {
    if (!t) return fail(FLS_ERR_ARG, "fls_scan_dict_codes: NULL table");
    t->dict_codes = enable != 0;
    return 0;
}

int fls_table_validity(const fls_table *t, uint32_t rg, uint32_t col, const uint64_t **words) {
    if (!t || rg >= t->meta.rgs.size() || col >= t->meta.cols.size())
        return fail(FLS_ERR_ARG, "validity (%u, %u) out of range", rg, col);
    const uint64_t *w = chunk_validity_host(t, rg, col);
    if (words) *words = w;
    return w ? 1 : 0;
}

int fls_rowgroup_may_match(const fls_table *t, uint32_t rg, const fls_predicate *preds, uint32_t n) {
    if (!t || rg >= t->meta.rgs.size()) return fail(FLS_ERR_ARG, "row group %u out of range", rg);
    std::vector<HostTerm> terms;
    int rc = to_terms(t, preds, n, terms);
    if (rc) return rc;
    return rowgroup_may_match(t, rg, terms) ? 1 : 0;
}

int fls_scan_next(fls_table *t, fls_rowgroup *out) {
    if (!t || !out) return fail(FLS_ERR_ARG, "fls_scan_next: NULL argument");
    return scan_next(t, t->scan, out);
}

int fls_scan_acquire(fls_table *t, fls_rowgroup *out) {
    if (!t || !out) return fail(FLS_ERR_ARG, "fls_scan_acquire: NULL argument");
    return scan_acquire(t, t->scan, out);
}

int fls_scan_release(fls_table *t, uint32_t rowgroup) {
    if (!t) return fail(FLS_ERR_ARG, "fls_scan_release: NULL table");
    return scan_release(t, t->scan, rowgroup);
}

}  // extern "C"
