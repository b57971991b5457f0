// fls_engine.hpp -- the host engine's internal types and the functions its
// units call across files.  Not part of the C ABI (include/flsgpu.h).
//
//   flsgpu.hip            connections, files and the scan pipeline
//                         (scan_setup, fill_batch, scan_acquire ...)
//   fls_launch.hip        the launch policy and the launches of one decode
//                         (launch_policy, order_for_launch, launch_all), over
//                         the hooks of fls_tuning.hpp
//   fls_cond.hip          (kernel) the aggregates' conditions; their host half,
//                         enqueue_conditions, sits beside enqueue_filter
//   fls_alt.hip           (kernels) the filter's alternatives; their host half,
//                         enqueue_alternatives, runs inside enqueue_filter
//   fls_scan_agg.hip      fls_aggregate / fls_aggregate_grouped: checks,
//                         per-batch enqueue, the host fold
//   fls_scan_hashagg.hip  fls_aggregate_hashed: checks, the key layout, the
//                         per-pipeline tables, per-batch enqueue, extraction
//                         and the host merge
//   fls_scan_topn.hip     fls_topn: checks, per-batch enqueue, the host merge
//                         and the late materialisation
//   fls_scan_keyset.hip   the key-set registry and fls_keyset_*; the build of a
//                         set from a scan (fls_keyset_from_scan): checks, the
//                         collecting range and its gate, per-batch enqueue, the
//                         bitmaps' way back and the host finish
//   fls_scan_keymap.hip   the key-map registry, fls_keymap_*, the bindings of
//                         mapped GROUP BY keys and their per-batch probe
//   fls_scan_valuemap.hip the value-map registry and fls_valuemap_*; the map
//                         terms themselves are filter terms (flsgpu.hip)
//   fls_device_table.hip  the device-resident table (fls_device_*)
//
// The pushdown and device-table units depend on flsgpu.hip's scan pipeline and
// fls_launch.hip's launches; flsgpu.hip depends on them only through the four enqueue_*
// functions fill_batch switches over, keyset_registry() and, for mapped GROUP
// BY keys, enqueue_keymap, binding_may_match and keymap_registry(), and for map
// terms valuemap_registry().  Every function
// and registry declared here is defined in exactly one unit.
//
// All of it lives in fls::engine, which is hidden: nothing here reaches
// libflsgpu.so's dynamic symbol table.  A namespace's visibility attribute
// covers one block only, so every block is opened with FLS_ENGINE_BEGIN.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <map>
#include <mutex>
#include <memory>
#include <string>
#include <chrono>
#include <cmath>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/flsgpu.h"
#include "fls_agg.hpp"
#include "fls_common.hpp"
#include "fls_config.hpp"
#include "fls_decode.hpp"
#include "fls_filter.hpp"
#include "fls_format.hpp"
#include "fls_groupagg.hpp"
#include "fls_hashagg.hpp"
#include "fls_keymap.hpp"
#include "fls_keyset.hpp"
#include "fls_pinned.hpp"
#include "fls_reader.hpp"
#include "fls_resident.hpp"
#include "fls_strmatch.hpp"
#include "fls_topn.hpp"
#include "fls_tuning.hpp"
#include "fls_valuemap.hpp"

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(FLS_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                                 \
    } while (0)

#define FLS_ENGINE_BEGIN namespace fls { namespace engine __attribute__((visibility("hidden"))) {
#define FLS_ENGINE_END } }

struct DevImage;    // a file's compressed image resident in HBM (flsgpu.hip)
struct MappedFile;  // a mapped, validated file shared by the tables that read it (flsgpu.hip)
struct fls_table;

FLS_ENGINE_BEGIN

struct ConnRes;  // what a connection keeps between scans (flsgpu.hip)

// DuckDB v1.3.2 string_t (16 B): len <= 12 inlined, else 4-byte prefix + pointer
struct StrT {
    uint32_t len;
    char data[12];
};
static_assert(sizeof(StrT) == 16, "string_t is 16 B");

// Scan set-up profile (FLS_SCAN_PROFILE=1): process-wide time and bytes per
// phase, printed to stderr when a table that scanned closes -- where a cold
// query's first milliseconds go (pinned and device allocations, string_t
// tables, the resident image, staging copies, the consumers' waits), and
// per batch on the GPU (HIP events on the slot's stream: the decode kernels,
// then the D2H of its columns; batches of different slots overlap, so these
// are summed stream time, not wall time).
enum ProfPhase {
    PROF_PIN_ALLOC, PROF_DEV_ALLOC, PROF_SETUP, PROF_STRTABS, PROF_IMAGE, PROF_STAGE_COPY, PROF_FILL, PROF_FILL_DESC,
    PROF_FILL_LIST, PROF_REFILL_LAT, PROF_WAIT, PROF_GPU_DECODE, PROF_D2H, PROF_N
};
struct ScanProf {
    std::atomic<uint64_t> ns[PROF_N] = {}, bytes[PROF_N] = {}, calls[PROF_N] = {};
    static bool on() {
        static const bool e = getenv("FLS_SCAN_PROFILE") && atoi(getenv("FLS_SCAN_PROFILE")) != 0;
        return e;
    }
    void print() {
        static const char *names[PROF_N] = {"pinned host alloc", "device alloc", "scan_setup", "string_t tables",
                                            "resident image", "staging copy", "fill_batch (all)",
                                            "fill: descriptors", "fill: chunk list", "batch seen -> refill",
                                            "consumer wait",
                                            "GPU decode (events)", "D2H (events)"};
        fprintf(stderr, "FLS_SCAN_PROFILE (process, since the last report):\n");
        for (int i = 0; i < PROF_N; ++i)
            fprintf(stderr, "  %-20s %9.3f ms  %8llu calls  %10.1f MB\n", names[i], ns[i].exchange(0) / 1e6,
                    (unsigned long long)calls[i].exchange(0), bytes[i].exchange(0) / 1e6);
    }
};
ScanProf &scan_prof();  // (flsgpu.hip)
struct ProfTimer {
    int ph;
    uint64_t b;
    std::chrono::steady_clock::time_point t0;
    explicit ProfTimer(int phase, uint64_t bytes = 0) : ph(ScanProf::on() ? phase : -1), b(bytes) {
        if (ph >= 0) t0 = std::chrono::steady_clock::now();
    }
    void stop() {  // record now (once)
        if (ph < 0) return;
        ScanProf &p = scan_prof();
        p.ns[ph] += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        p.bytes[ph] += b;
        p.calls[ph] += 1;
        ph = -1;
    }
    void cancel() { ph = -1; }
    ~ProfTimer() { stop(); }
};

// Frees every HBM-resident image no running scan uses on GPU dev (defined
// with the image registry); a device allocation that runs out of memory calls
// it once and retries, so the image cache never fails a scan's own buffers.
uint64_t release_idle_images(int dev);

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    int dev = -1;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n), dev(o.dev) { o.p = nullptr; o.n = 0; }
    void release() {
        if (p) {
            int cur;
            hipGetDevice(&cur);
            hipSetDevice(dev);
            hipFree(p);
            hipSetDevice(cur);
        }
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(int d, size_t count) {
        if (count <= n && p && d == dev) return hipSuccess;
        release();
        dev = d;
        n = count;
        ProfTimer pt(PROF_DEV_ALLOC, count * sizeof(T));
        hipError_t e = hipMalloc((void **)&p, std::max<size_t>(1, count * sizeof(T)));
        if (e == hipErrorOutOfMemory && release_idle_images(d) > 0) {
            (void)hipGetLastError();
            e = hipMalloc((void **)&p, std::max<size_t>(1, count * sizeof(T)));
        }
        if (e != hipSuccess) {
            p = nullptr;
            n = 0;
        }
        return e;
    }
    ~DevBuf() { release(); }
};

template <typename T>
struct PinBuf {
    T *p = nullptr;
    size_t n = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    PinBuf(PinBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    void release() {
        if (p) pinned_free(p);
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count) {
        if (count <= n && p) return hipSuccess;
        release();
        n = count;
        ProfTimer pt(PROF_PIN_ALLOC, count * sizeof(T));
        const hipError_t e = pinned_alloc((void **)&p, std::max<size_t>(1, count * sizeof(T)));
        if (e != hipSuccess) {
            p = nullptr;
            n = 0;
        }
        return e;
    }
    ~PinBuf() { release(); }
};

// Device images are allocated this much past their last chunk: kernels read
// whole 16 B blocks of a stream whose last block may end inside it.
constexpr uint64_t kImagePad = 256;

// FSST chunks of a launch, one kernel group after another (order_for_launch):
// 0 = segment tables and every string <= 255 bytes, 1 = segment tables,
// 2 = strings <= 255 bytes, 3 = the rest (DevChunk.vbits: bit 0 = small
// strings, bit 1 = segment tables); each group numbers its vectors through
// DevChunk.vec_base.
constexpr int kFsstGroups = 4;
inline int fsst_group(uint8_t vbits) { return vbits == 3 ? 0 : vbits == 2 ? 1 : vbits == 1 ? 2 : 3; }
struct FsstCounts {
    uint32_t n[kFsstGroups] = {}, vecs[kFsstGroups] = {};
    uint32_t first(int g) const {
        uint32_t f = 0;
        for (int k = 0; k < g; ++k) f += n[k];
        return f;
    }
    uint64_t total_vecs() const {
        uint64_t t = 0;
        for (int k = 0; k < kFsstGroups; ++k) t += vecs[k];
        return t;
    }
};

// Per-chunk algorithmic byte accounting (roofline numerator).
struct ByteCount {
    uint64_t values = 0, packed = 0, meta = 0, out = 0;
    DecodeGeom geom;   // max LDS need over the counted chunks
};

// Byte range of the file covering row groups [rg0, rg1).
void rg_byte_range(const FileMeta &m, uint32_t rg0, uint32_t rg1, uint64_t &lo, uint64_t &hi);

// Pinned host side of one decoded batch: what consumers read.  It belongs to
// the batch's row groups, not to the device slot that produced it: once every
// row group of the batch has been handed out (fls_scan_acquire) the slot is
// refilled with a fresh HostBatch from the pool, and this one goes back to the
// pool when the last of its row groups is released.  So a consumer that keeps
// a row group (DuckDB vectors that reference the pinned columns) never holds
// up the GPU pipeline, and no consumer waits for another one's release.
struct HostBatch {
    uint32_t rg0 = 0, nrg = 0;
    uint32_t handed = 0, released = 0;    // row groups handed out / handed back
    std::vector<PinBuf<uint8_t>> h_out;   // per delivered column (pinned)
    std::vector<PinBuf<uint8_t>> h_heap;  // per FSST column: pinned copy string_t points into
    std::vector<const void *> col_ptrs;   // per (rg - rg0) * ncols + col: pinned host column start
    PinBuf<uint32_t> h_counts;            // filtered: selected rows per vector (key-set build: rows that set a bit)
    PinBuf<uint32_t> h_sel;               // filtered: selected row indices within their row group
    uint32_t nvec = 0;                    // vectors of the batch
    bool sel_ready = false;               // sel_off computed from h_counts
    std::vector<uint32_t> sel_off;        // per row group of the batch (+1): first selected row
    // per (rg - rg0) * ncols + col: the delivered rows' validity words (NULL:
    // all valid) -- the file image's bitmaps, or, filtered, gathered into vbits
    std::vector<const uint64_t *> valid_ptrs;
    std::vector<std::vector<uint64_t>> vbits;
    // dictionary-coded delivery (fls_scan_dict_codes): per column the bytes
    // delivered per row (string_t 16, or a code width 1 / 2), per (rg - rg0) *
    // ncols + col the host string_t dictionary and its size (NULL: not coded)
    std::vector<uint8_t> ob;
    std::vector<const void *> dict_ptrs;
    std::vector<uint32_t> dict_sizes;
    // narrowed delivery (fls_scan_narrow): per column 1 when it crosses PCIe
    // as value - base in ob bytes, per (rg - rg0) * ncols + col that base
    std::vector<uint8_t> narrowed;
    std::vector<uint64_t> nbase;
    // FSST columns delivered as string lengths (fls_scan_narrow, unfiltered
    // scans): per column the length width (0: string_t records cross PCIe);
    // per (rg - rg0) * ncols + col the row group's heap offset in h_heap; the
    // string_t records rebuilt on the consumer's thread (scan_acquire) into
    // h_rec; narrow_out = narrowed with these columns cleared (the consumer
    // sees string_t)
    std::vector<uint8_t> strlen_w, narrow_out, ob_out;
    std::vector<uint64_t> heap_off;
    std::vector<std::unique_ptr<uint8_t[]>> h_rec;
    std::vector<uint64_t> h_rec_cap;      // rows h_rec[c] holds
    // completion of the batch's device work, per batch rather than per slot:
    // the slot takes its next batch as soon as this one's D2H is complete (its
    // first acquire), while consumers still take this one's row groups
    hipEvent_t done = nullptr;            // recorded after the D2H (fill_batch)
    hipEvent_t pt[3] = {};                // FLS_SCAN_PROFILE: decode start, D2H start, end (timing events)
    uint64_t prof_d2h = 0;                // ... and the batch's D2H bytes
    std::atomic<bool> prof_pending{false};  // the batch's times not yet counted (its first acquire does)
    std::atomic<bool> upload_resident{false};  // the batch uploads into the resident image (marked present once done)
    PinBuf<uint32_t> h_err;               // the device error flags, copied after the batch's kernels
    PinBuf<AggRec> h_agg;                 // aggregate scan: nvec x naggs partial records (vector-major)
    // grouped aggregate scan: per row group of the batch its table of groups
    // (fls_groupagg.hpp, group_rg_stride(naggs, g_nfsum, g_rg_vecs) bytes each)
    PinBuf<uint8_t> h_grp;
    uint32_t g_nfsum = 0, g_rg_vecs = 0;
    // top-N scan: per row group of the batch its list of candidates
    // (fls_topn.hpp, topn_stride(k) bytes each)
    PinBuf<uint8_t> h_topn;
    HostBatch() = default;
    HostBatch(const HostBatch &) = delete;
    HostBatch &operator=(const HostBatch &) = delete;
    ~HostBatch() {
        if (done) hipEventDestroy(done);
        for (hipEvent_t e : pt)
            if (e) hipEventDestroy(e);
    }
};

struct Slot {                       // one batch of row groups in flight
    uint32_t rg0 = 0, nrg = 0;      // absolute row groups (consecutive, all surviving pruning)
    bool busy = false;              // a batch is enqueued and its D2H not yet seen complete by an acquire
    bool filling = false;           // claimed, its work being enqueued (fill_batch, outside s.mu)
    bool starved = false;           // refill deferred: the host-batch pool is at its cap
    HostBatch *hb = nullptr;        // host side of the batch in flight
    std::vector<DevBuf<uint8_t>> d_out;   // per decoded column
    std::vector<DevBuf<uint8_t>> d_heap;  // per FSST column: decoded string bytes
    std::vector<uint64_t> heap_bytes;     // per column: heap bytes of this batch
    PinBuf<DevChunk> h_chunks;
    DevBuf<DevChunk> d_chunks;
    DevBuf<uint8_t> d_in;           // streamed compressed bytes of the batch (no resident image)
    const uint8_t *in_dev = nullptr;  // device address of the batch's first compressed byte
    PinBuf<uint8_t> h_stage;        // pinned bounce buffer when the image cannot be pinned
    DevBuf<uint32_t> queue;         // decode work-queue counter
    uint64_t in_base = 0;
    hipStream_t stream = nullptr;   // one stream per slot: slot b's H2D+decode overlap slot a's D2H
    // filtered batches (fls_scan_filter)
    DevBuf<uint64_t> d_mask;        // selection bits, 16 words per 1024-row vector
    DevBuf<uint32_t> d_counts;      // selected rows per vector
    PinBuf<uint8_t> h_fdesc;        // DevTerm[] + DevOut[] + constant strings
    DevBuf<uint8_t> d_fdesc;
    PinBuf<DevSetTerm> h_sdesc;     // the filter's key-set terms
    DevBuf<DevSetTerm> d_sdesc;
    PinBuf<DevColTerm> h_cdesc;     // the filter's column-to-column terms
    DevBuf<DevColTerm> d_cdesc;
    PinBuf<DevMapCmpTerm> h_vdesc;  // the filter's map terms
    DevBuf<DevMapCmpTerm> d_vdesc;
    PinBuf<uint8_t> h_pdesc;        // the filter's pattern terms: DevPatTerm[] + their tokens
    DevBuf<uint8_t> d_pdesc;
    std::vector<DevBuf<uint64_t>> d_valid;  // per filtered / aggregated column with a NULL: batch validity words
    std::vector<uint8_t> valid_staged;      // per column: d_valid[c] holds this batch's words (stage_validity)
    std::vector<DevBuf<uint8_t>> d_narrow;  // per narrowed column: its narrowed copy
    PinBuf<uint8_t> h_ndesc;                // DevNarrow[] + per-row-group bases
    DevBuf<uint8_t> d_ndesc;
    // aggregate batches (fls_aggregate)
    PinBuf<DevAgg> h_adesc;
    DevBuf<DevAgg> d_adesc;
    DevBuf<AggRec> d_agg;           // partial records of the batch
    // the aggregates' conditions (fls_aggregate_conditions)
    PinBuf<uint8_t> h_qdesc;        // DevTerm[] + DevColTerm[] + DevSetTerm[] + DevMapCmpTerm[] + DevPatTerm[], then strings and tokens
    DevBuf<uint8_t> d_qdesc;
    DevBuf<uint64_t> d_cond;        // per condition a plane of 16 words per vector: where & cond
    DevBuf<uint32_t> d_ccounts;     // the narrowing kernels' per-vector counts of a plane (scratch)
    // the filter's alternatives (fls_scan_filter_alternatives)
    PinBuf<uint8_t> h_altdesc;      // laid out as h_qdesc
    DevBuf<uint8_t> d_altdesc;
    DevBuf<uint64_t> d_alt;         // per alternative a plane of 16 words per vector: mask & alternative
    // grouped aggregate batches (fls_aggregate_grouped)
    PinBuf<uint8_t> h_gdesc;        // DevKey[kMaxKeys] + per row group its first vector and vector count
    DevBuf<uint8_t> d_gdesc;
    DevBuf<uint8_t> d_gvec;         // stage 1: the vectors' groups
    DevBuf<uint8_t> d_grg;          // stage 2: the row groups' groups
    // hash aggregate batches (fls_aggregate_hashed)
    PinBuf<uint8_t> h_hdesc;        // DevHashKey[kMaxKeys] + DevHashFields[kMaxAggs]
    DevBuf<uint8_t> d_hdesc;
    // mapped keys of a grouped aggregate batch (fls_aggregate_key_bindings)
    PinBuf<DevMapTerm> h_mdesc;
    DevBuf<DevMapTerm> d_mdesc;
    DevBuf<uint16_t> d_kcode;       // per binding 1024 codes per vector: the derived key columns
    DevBuf<uint64_t> d_kvalid;      // per binding 16 words per vector: a keep-unmatched key's validity
    // mapped columns of an aggregate batch (fls_aggregate_value_bindings): per
    // used binding (mapped_slot) a derived column and its validity, both
    // defined at selected rows only (fls_mapval.hip)
    PinBuf<DevMapValTerm> h_mvdesc;
    DevBuf<DevMapValTerm> d_mvdesc;
    DevBuf<uint64_t> d_mval;        // per used binding 1024 values per vector
    DevBuf<uint64_t> d_mvalid;      // per used binding 16 words per vector
    // top-N batches (fls_topn)
    PinBuf<uint32_t> h_tdesc;       // per row group its first vector and vector count
    DevBuf<uint32_t> d_tdesc;
    DevBuf<uint8_t> d_tvec;         // stage 1: the vectors' candidate lists
    DevBuf<uint8_t> d_ttmp;         // stage 2: the other side of the merge tree's ping-pong
    DevBuf<uint8_t> d_trg;          // stage 2: the row groups' candidate lists
};

// One GPU's scan pipeline: streams, the two device slots and the pinned
// host-batch pool.  A scan borrows one per GPU from its connection
// (ConnRes::take) and the table gives it back when it closes, so the next
// table -- a new DuckDB query -- starts without stream creation, hipMalloc or
// hipHostMalloc.
constexpr size_t kIdent16 = 256;  // ScanDev::ident: where the u16 identity table starts

struct ScanDev {
    int dev = -1;
    hipStream_t stream = nullptr;
    uint32_t rg0 = 0, rg1 = 0;      // span of row groups this GPU owns within the scan
    uint32_t p0 = 0, p1 = 0;        // ... as positions in ScanCtx::rgs
    uint32_t next_p = 0;            // next position to enqueue
    // device slots: batches in flight at once (ScanCtx::nslots of them used)
    static constexpr int kMaxSlots = 4;
    Slot slots[kMaxSlots];
    std::shared_ptr<DevImage> dimg;  // the scanned file's resident image on this GPU (none: per-slot uploads)
    std::vector<std::unique_ptr<HostBatch>> batches;  // host-batch pool of this GPU
    std::vector<HostBatch *> free_batches;
    DevBuf<StrT> strtab;
    std::vector<uint64_t> strtab_off;
    std::vector<StrT> h_strtab;     // host copy of strtab (the dictionaries coded columns reference)
    // identity "dictionaries" a coded column gathers its codes from: u8 0..255
    // at byte 0, u16 0..65535 at byte kIdent16
    DevBuf<uint8_t> ident;
    DevBuf<uint32_t> err;
    int grid = 0;
    ScanDev() = default;
    ScanDev(const ScanDev &) = delete;
    ScanDev &operator=(const ScanDev &) = delete;
    void sync() {
        if (dev < 0) return;
        hipSetDevice(dev);
        if (stream) hipStreamSynchronize(stream);
        for (auto &sl : slots)
            if (sl.stream) hipStreamSynchronize(sl.stream);
    }
    ~ScanDev() {
        sync();
        for (auto &sl : slots)
            if (sl.stream) hipStreamDestroy(sl.stream);
        if (stream) hipStreamDestroy(stream);
    }
};

// A key set (fls_keyset_create): the host image and its copies in HBM, one
// per GPU, made by the first scan that probes the set there.  Filters hold a
// reference, so the handle may be freed while a filter or a scan uses the set;
// the copies go with the last reference.  They are not resident images and do
// not count against FLS_SCAN_RESIDENT_MB.
struct KeySet {
    KeysetImage img;
    const fls_connection *conn = nullptr;
    std::mutex mu;
    std::vector<std::unique_ptr<DevBuf<uint64_t>>> copies;
    // the image on GPU dev (the current device), uploaded on first use
    hipError_t device_image(int dev, const uint64_t **out) {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &c : copies)
            if (c->dev == dev) {
                *out = c->p;
                return hipSuccess;
            }
        auto b = std::make_unique<DevBuf<uint64_t>>();
        hipError_t e = b->alloc(dev, img.words.size());
        // a synchronous copy: complete before any kernel enqueued after this call
        if (e == hipSuccess && !img.words.empty())
            e = hipMemcpy(b->p, img.words.data(), img.bytes(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
        *out = b->p;
        copies.push_back(std::move(b));
        return hipSuccess;
    }
};

// Live key sets by handle.  A handle is a counter value, never an address:
// a stale or foreign fls_predicate.value is looked up here and refused
// without being dereferenced.
struct KeySetRegistry {
    std::mutex mu;
    uint64_t next = 1;
    std::unordered_map<uint64_t, std::shared_ptr<KeySet>> live;
    static uint64_t handle_of(uint64_t id) { return (id << 4) | 0x5; }
    std::shared_ptr<KeySet> find(uint64_t handle) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = live.find(handle);
        return it == live.end() ? nullptr : it->second;
    }
};
KeySetRegistry &keyset_registry();  // (fls_scan_keyset.hip)

// A key map (fls_keymap_create): the host image and its copies in HBM, held
// and uploaded as a key set's are.  Bindings and running scans hold a
// reference; the copies are outside FLS_SCAN_RESIDENT_MB.
struct KeyMap {
    KeymapImage img;
    const fls_connection *conn = nullptr;
    std::mutex mu;
    std::vector<std::unique_ptr<DevBuf<uint64_t>>> copies;
    // the image on GPU dev (the current device), uploaded on first use
    hipError_t device_image(int dev, const uint64_t **out) {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &c : copies)
            if (c->dev == dev) {
                *out = c->p;
                return hipSuccess;
            }
        auto b = std::make_unique<DevBuf<uint64_t>>();
        hipError_t e = b->alloc(dev, img.words.size());
        // a synchronous copy: complete before any kernel enqueued after this call
        if (e == hipSuccess && !img.words.empty())
            e = hipMemcpy(b->p, img.words.data(), img.bytes(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
        *out = b->p;
        copies.push_back(std::move(b));
        return hipSuccess;
    }
};

// Live key maps by handle: counter tokens like the key sets', with tag bits of
// their own, so a key-set handle never resolves as a map (nor a map as a set).
struct KeyMapRegistry {
    std::mutex mu;
    uint64_t next = 1;
    std::unordered_map<uint64_t, std::shared_ptr<KeyMap>> live;
    static uint64_t handle_of(uint64_t id) { return (id << 4) | 0xA; }
    std::shared_ptr<KeyMap> find(uint64_t handle) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = live.find(handle);
        return it == live.end() ? nullptr : it->second;
    }
};
KeyMapRegistry &keymap_registry();  // (fls_scan_keymap.hip)

// A value map (fls_valuemap_create): the host image and its copies in HBM,
// held and uploaded as a key map's are (KeyMap::device_image).  Filters that
// hold a map term and running scans hold a reference; the copies are outside
// FLS_SCAN_RESIDENT_MB.
struct ValueMap {
    ValuemapImage img;
    const fls_connection *conn = nullptr;
    std::mutex mu;
    std::vector<std::unique_ptr<DevBuf<uint64_t>>> copies;
    // the image on GPU dev (the current device), uploaded on first use
    hipError_t device_image(int dev, const uint64_t **out) {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &c : copies)
            if (c->dev == dev) {
                *out = c->p;
                return hipSuccess;
            }
        auto b = std::make_unique<DevBuf<uint64_t>>();
        hipError_t e = b->alloc(dev, img.words.size());
        // a synchronous copy: complete before any kernel enqueued after this call
        if (e == hipSuccess && !img.words.empty())
            e = hipMemcpy(b->p, img.words.data(), img.bytes(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
        *out = b->p;
        copies.push_back(std::move(b));
        return hipSuccess;
    }
};

// Live value maps by handle: counter tokens with tag bits of their own, so no
// key-set (| 0x5) or key-map (| 0xA) handle resolves as a value map, nor a
// value map as either.
struct ValueMapRegistry {
    std::mutex mu;
    uint64_t next = 1;
    std::unordered_map<uint64_t, std::shared_ptr<ValueMap>> live;
    static uint64_t handle_of(uint64_t id) { return (id << 4) | 0x3; }
    std::shared_ptr<ValueMap> find(uint64_t handle) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = live.find(handle);
        return it == live.end() ? nullptr : it->second;
    }
};
ValueMapRegistry &valuemap_registry();  // (fls_scan_valuemap.hip)

// One mapped GROUP BY key (fls_aggregate_key_bindings), host side: the code
// the map gives column col.
struct HostBinding {
    uint32_t col = 0;
    bool keep = false;              // FLS_KEYMAP_KEEP_UNMATCHED
    std::shared_ptr<KeyMap> map;
};

// One mapped column (fls_aggregate_value_bindings), host side: the value the
// map gives column col.  FLS_COL_MAPPED | i names binding i of the table's
// list wherever an aggregate takes a column and as a hash aggregate's key; a
// scan carries the whole list (ScanCtx::vbinds, same numbering) and the bits of
// the bindings its call names (ScanCtx::vused): only those are probed, narrow
// the mask or prune.
struct HostValueBinding {
    uint32_t col = 0;
    bool keep = false;              // FLS_VALUEMAP_KEEP_UNMATCHED
    std::shared_ptr<ValueMap> map;
};
constexpr uint32_t kMaxValueBindings = 4;
inline bool is_mapped_col(uint32_t c) { return (c & FLS_COL_MAPPED) != 0; }
inline uint32_t mapped_index(uint32_t c) { return c & ~FLS_COL_MAPPED; }
// binding i's place among the used ones: which derived column of the slot is its own
inline uint32_t mapped_slot(uint32_t vused, uint32_t i) { return (uint32_t)__builtin_popcount(vused & ((1u << i) - 1)); }

// One term of a pushed-down filter (fls_scan_filter), host side.
struct HostTerm {
    uint32_t col = 0, clause = 0;
    uint32_t col2 = 0;              // OP_COL_EQ .. OP_COL_GE: the right column; OP_MAP_EQ .. OP_MAP_GE: the key column
    uint8_t op = 0, kind = 0;
    uint64_t value = 0;             // comparison domain: int64 / uint64 / double bits
    std::string str;
    std::shared_ptr<KeySet> set;    // OP_IN_SET / OP_NOT_IN_SET
    std::shared_ptr<const CompiledPattern> pat;  // OP_LIKE / OP_NOT_LIKE
    std::shared_ptr<ValueMap> map;  // OP_MAP_EQ .. OP_MAP_GE
};
inline bool is_set_op(uint8_t op) { return op == OP_IN_SET || op == OP_NOT_IN_SET; }
inline bool is_pat_op(uint8_t op) { return op == OP_LIKE || op == OP_NOT_LIKE; }
inline bool is_col_op(uint8_t op) { return op >= OP_COL_EQ && op <= OP_COL_GE; }
inline bool is_map_op(uint8_t op) { return op >= OP_MAP_EQ && op <= OP_MAP_GE; }
// does the term read a second column (HostTerm::col2) beside col?
inline bool reads_col2(uint8_t op) { return is_col_op(op) || is_map_op(op); }
constexpr uint32_t kMaxMapTerms = 8;  // map terms of one term list (a filter, a condition, an alternative)

// One aggregate of fls_aggregate, host side.
struct HostAgg {
    uint8_t fn = 0;                 // AggFn
    uint32_t col = 0, col2 = 0;
    // SUM_EXPR: the product of the factors fk + (fneg ? -1 : +1) * column fcol
    uint32_t nf = 0;
    uint32_t fcol[kMaxFactors] = {};
    uint8_t fneg[kMaxFactors] = {};
    int64_t fk[kMaxFactors] = {};
    uint32_t cond = 0;              // 0: none, else condition cond - 1 of the scan's list (ScanCtx::conds)
};

// What a scan does with a batch's decoded rows instead of delivering them.
// scan_setup sets it from the plan; everything after reads it here.
enum class Reduce {
    None,            // a delivering scan: the (filtered) columns go to the consumer
    Aggregate,       // fls_aggregate: per-vector partial records (enqueue_aggregate)
    GroupAggregate,  // fls_aggregate_grouped: per-row-group tables of groups (enqueue_group_aggregate)
    TopN,            // fls_topn: per-row-group candidate lists (enqueue_topn)
    HashAggregate,   // fls_aggregate_hashed: every batch into the pipeline's table in HBM (enqueue_hash_aggregate)
    KeySet,          // fls_keyset_from_scan: every batch's keys into the GPU's collecting bitmap (enqueue_keyset_build)
    MapBuild,        // fls_valuemap_from_scan / fls_keymap_from_scan: every batch's pairs into the GPU's collecting array (enqueue_mapbuild)
};

// The collecting range and bitmaps of a key-set build (fls_scan_keyset.hip):
// bit key - base of a bitmap over [base, base + span], span < kKeysetMaxSpan.
// The bitmaps belong to the call, one per GPU its row groups shard over
// (bitmaps[g] for ScanCtx::devs[g]; pipelines on one GPU share theirs),
// allocated and zeroed before scan_start.
struct KeyBuildPlan {
    uint32_t col = 0;
    uint64_t base = 0, span = 0;
    bool window = true;                  // clustered words go through the wave's LDS window
    std::vector<uint32_t *> bitmaps;     // per pipeline, in HBM (NULL: the pipeline reads no row group)
};

// The columns, the collecting range and the collecting arrays of a map build
// (fls_scan_mapbuild.hip): slot key - base of an array over
// [base, base + span], span < kValuemapMaxSpan, takes the row's value.  The
// arrays belong to the call, one per GPU its row groups shard over (slots[g]
// for ScanCtx::devs[g]; pipelines on one GPU share theirs), span + 4 entries
// each (the last three: the conflict cells), allocated and filled with 0xFF bytes
// before scan_start.
struct MapBuildPlan {
    uint32_t key_col = 0, value_col = 0;
    uint64_t base = 0, span = 0;
    std::vector<uint64_t *> slots;       // per pipeline, in HBM (NULL: the pipeline reads no row group)
};

// The packed key and the tables of a hash aggregate (fls_scan_hashagg.hip):
// key q's field is value - min[q] in bits[q] bits at shift[q], its NULL mark
// bit null_bit[q].  The tables belong to the call, one per pipeline of the
// scan (tables[g] for ScanCtx::devs[g]), allocated and zeroed before scan_start.
struct HashPlan {
    uint64_t min[kMaxKeys] = {}, span[kMaxKeys] = {};
    uint32_t bits[kMaxKeys] = {}, shift[kMaxKeys] = {}, null_bit[kMaxKeys] = {};
    uint32_t total = 0;                  // bits of the packed key (<= kHashKeyBits)
    uint64_t cap = 0;                    // slots of each table
    uint32_t nfields = 0;                // fields of a slot (fls_hashagg.hpp)
    std::vector<DevHashFields> fields;   // per aggregate
    std::vector<uint64_t *> tables;      // per pipeline, in HBM
    bool combine = false;                // merge runs of equal keys in adjacent lanes before the atomics
};

// What a scan is asked to do (scan_setup).  The pointers are borrowed for the
// call; what the scan needs later is copied into its ScanCtx.
struct ScanPlan {
    std::vector<int> devices;                       // the GPUs the row groups shard over
    const uint8_t *col_mask = nullptr;              // per column: delivered (NULL: every column)
    uint32_t rg0 = 0, rg1 = 0;                      // row groups [rg0, rg1)
    const std::vector<HostTerm> *filter = nullptr;  // pushed-down filter (NULL: none)
    // the filter's alternatives (NULL: none): a row is selected when the filter
    // selects it and one of them is true there
    const std::vector<std::vector<HostTerm>> *alts = nullptr;
    // a consumer's scan (fls_scan_begin), which honours the table's delivery
    // options (dictionary codes, narrowing, deferred records); fls_materialize
    // and the scans the engine runs for itself deliver at full width
    bool delivering_scan = false;
    const std::vector<HostAgg> *aggs = nullptr;     // Reduce::Aggregate / GroupAggregate / HashAggregate
    // the conditions HostAgg::cond numbers (NULL: none); they prune nothing and select no row
    const std::vector<std::vector<HostTerm>> *conds = nullptr;
    // Reduce::GroupAggregate: the GROUP BY keys, a column each or
    // FLS_KEY_MAPPED | i for binding i of binds
    const std::vector<uint32_t> *keys = nullptr;
    const std::vector<HostBinding> *binds = nullptr;  // the mapped keys' bindings (NULL: none)
    // the mapped columns' bindings (NULL: none), FLS_COL_MAPPED | i in an
    // aggregate's columns or a hash key numbering them, and the bits of those
    // the call names (used_value_bindings)
    const std::vector<HostValueBinding> *vbinds = nullptr;
    uint32_t vused = 0;
    // Reduce::HashAggregate (max_groups != 0): keys are plain columns or mapped ones, hash their layout and tables
    uint64_t max_groups = 0;
    const HashPlan *hash = nullptr;
    const fls_order_key *order = nullptr;           // Reduce::TopN: the key and
    uint32_t k = 0;                                 // ... how many rows
    const KeyBuildPlan *keybuild = nullptr;         // Reduce::KeySet: the key column, the range and the bitmaps
    const MapBuildPlan *mapbuild = nullptr;         // Reduce::MapBuild: the two columns, the range and the arrays
    // exactly these row groups (ascending, inside the range) instead of
    // pruning the range: fls_topn's late materialisation, and the survivors
    // fls_keyset_from_scan and the map builds took their range from
    const std::vector<uint32_t> *only = nullptr;
};

struct ScanCtx {
    bool active = false;
    Reduce reduce = Reduce::None;
    std::vector<uint8_t> mask;      // delivered columns
    std::vector<uint8_t> dmask;     // decoded columns (delivered + filter columns)
    std::vector<HostTerm> terms;    // filter of this scan, sorted by clause (empty: none)
    // ... and its alternatives (fls_scan_filter_alternatives), each a filter of
    // its own sorted by clause: the mask keeps a row of the filter's where one
    // of them is true (enqueue_alternatives).  Empty: none.
    std::vector<std::vector<HostTerm>> alts;
    // aggregate scan (Reduce::Aggregate / GroupAggregate): no column is
    // delivered, each batch's partial records ride in its HostBatch
    std::vector<HostAgg> aggs;
    // ... and the conditions their HostAgg::cond numbers, each a filter of its
    // own sorted by clause: their columns are decoded and their validity
    // staged like the filter's, per batch they become planes (enqueue_conditions)
    std::vector<std::vector<HostTerm>> conds;
    // GROUP BY columns of a grouped aggregate scan (Reduce::GroupAggregate):
    // decoded like operands, VARCHAR keys as dictionary codes
    std::vector<uint32_t> keys;
    // ... where FLS_KEY_MAPPED | i stands for the code binding i gives its
    // column (keymap_kernel).  With a binding the scan always has a mask.
    std::vector<HostBinding> binds;
    // mapped columns (FLS_COL_MAPPED | i in aggs or keys): the table's value
    // bindings and the bits of those this scan probes (mapval_kernel).  With
    // one used the scan always has a mask; the key columns of the used ones
    // are decoded and their validity staged, as for binds.
    std::vector<HostValueBinding> vbinds;
    uint32_t vused = 0;
    // key-set build (Reduce::KeySet): nothing is delivered, the batches' keys
    // meet in the plan's bitmaps; their per-vector counts ride in the HostBatch.
    // Such a scan always has a mask, as one with a binding has.
    KeyBuildPlan keybuild;
    // map build (Reduce::MapBuild): the same, with the plan's collecting arrays
    MapBuildPlan mapbuild;
    bool masked() const {
        return !terms.empty() || !alts.empty() || !binds.empty() || vused != 0 || reduce == Reduce::KeySet ||
               reduce == Reduce::MapBuild;
    }
    // hash aggregate scan (Reduce::HashAggregate): the key layout and the
    // pipelines' tables, and the groups one table may hold
    HashPlan hash;
    uint64_t max_groups = 0;
    // top-N scan (Reduce::TopN): no column is delivered, each batch's
    // candidate lists ride in its HostBatch
    fls_order_key tkey = {};
    uint32_t tk = 0;
    bool aggregating() const {
        return reduce == Reduce::Aggregate || reduce == Reduce::GroupAggregate || reduce == Reduce::HashAggregate;
    }
    bool dict_codes = false;        // deliver DICT string chunks as codes + dictionary
    bool narrow = false;            // deliver integer columns narrowed to their row groups' ranges
    bool defer_records = false;     // FSST-as-lengths records built by fls_scan_build_records, not scan_acquire
    std::vector<uint32_t> rgs;      // row groups to scan, in order (pruned ones left out)
    uint32_t cur = 0;               // next position in rgs to hand out
    uint32_t pruned = 0;
    uint32_t batch = 8;
    std::vector<std::unique_ptr<ScanDev>> devs;  // borrowed from the connection (ConnRes)
    int64_t held = -1;              // row group fls_scan_next handed out last (released on the next call)
    std::vector<std::pair<uint32_t, HostBatch *>> out;  // row groups handed out and not yet released
    // batches whose D2H an acquire saw complete and whose slot took its next
    // batch: (device index, batch) until their last row group is handed out
    std::vector<std::pair<int, HostBatch *>> ready;
    bool early_refill = true;       // FLS_SCAN_EARLY_REFILL
    bool spin_wait = false;         // FLS_SCAN_SPIN_WAIT (A/B): acquires poll the batch event
    uint32_t max_batches = 64;      // host-batch pool cap per GPU (FLS_SCAN_HOST_BATCHES)
    int nslots = 2;                 // device slots per GPU (FLS_SCAN_SLOTS, 1..ScanDev::kMaxSlots)
    // sticky error of a failed batch refill (scan_release): consumers waiting
    // for a row group of that batch, and every later acquire, return it
    // instead of waiting for a batch that will never be enqueued
    int err_rc = 0;
    std::string err_msg;
    // fls_scan_acquire/release may be called from several consumer threads:
    // claiming a row group, releasing one and refilling a slot happen under mu;
    // waiting for a batch's decode does not.
    std::mutex mu;
    std::condition_variable cv;
};

FLS_ENGINE_END

// Second stream a table decode overlaps its FSST kernels on (launch_all).
struct SideStream {
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    // CU-partitioned overlap (FLS_OVERLAP_CU_SPLIT = m): two streams whose
    // kernels may only use disjoint CU sets -- set A (CU index mod 32 < m) for
    // the main decode, set B for FSST -- made on first use for that m
    int cu_m = 0;
    hipStream_t cu_a = nullptr, cu_b = nullptr;
    hipEvent_t join_a = nullptr, join_b = nullptr;
    void release_cu() {
        for (hipStream_t *st : {&cu_a, &cu_b})
            if (*st) {
                hipStreamSynchronize(*st);
                hipStreamDestroy(*st);
                *st = nullptr;
            }
        for (hipEvent_t *e : {&join_a, &join_b})
            if (*e) {
                hipEventDestroy(*e);
                *e = nullptr;
            }
        cu_m = 0;
    }
};

FLS_ENGINE_BEGIN

// One GPU's part of a device-resident table (fls_device_*): a contiguous
// range of row groups uploaded verbatim to its HBM with their string_t
// tables, the decoded columns, the launch descriptor list and the streams and
// events of its decode launches.  A table is split over the connection's GPUs
// like a scan (no data crosses GPUs: row groups are independent).
struct Resident {
    int dev = -1;
    uint32_t rg0 = 0, rg1 = 0;
    uint64_t base = 0;                 // file offset of img[0]
    uint64_t first_row = 0, rows = 0;  // resident rows, relative to the file's first row
    DevBuf<uint8_t> img;               // compressed bytes of [rg0, rg1)
    DevBuf<StrT> strtab;               // string_t tables of VARCHAR chunks
    std::vector<uint64_t> strtab_off;  // per (rg - rg0) * ncols + col: index into strtab
    DevBuf<uint32_t> err;
    DevBuf<uint32_t> queue;                // decode work-queue counters
    std::vector<DevBuf<uint8_t>> d_heap;   // per FSST column: decoded string bytes
    std::vector<PinBuf<uint8_t>> h_heap;   // per FSST column: host copy string_t points into
    std::vector<uint64_t> heap_off;        // per (rg - rg0) * ncols + col: chunk heap offset
    std::vector<DevBuf<uint8_t>> d_out;    // per column, rows of [rg0, rg1)
    double placement_q = 0;                // write-probe rating of d_out's placement (choose_placement; 0: not rated)
    float placement_ms = 0;                // decode-time rating of d_out's placement (0: not rated)
    DevBuf<DevChunk> d_chunks;
    std::vector<DevChunk> h_chunks;
    std::vector<uint8_t> mask;         // column mask h_chunks was built for
    uint32_t nmain = 0;                // h_chunks[0, nmain) main kernel, the rest FSST
    DevBuf<DictVec> d_dictvecs;        // the dictionary-string grid's vectors (launch_dictstr), built with h_chunks
    uint32_t ndictvecs = 0;            // ... and how many (their chunks are not in h_chunks)
    bool list_built = false;           // h_chunks / d_dictvecs describe the current mask, list_key and outputs
    void invalidate() {                // a new mask, list key or set of outputs: rebuild both at the next decode
        h_chunks.clear();
        ndictvecs = 0;
        list_built = false;
    }
    DecodeTuning::List list_key;       // the hooks h_chunks was ordered for (read_decode_tuning)
    DecodeTuning tuning;               // ... resolved for its launch (launch_policy); .launch anew at every decode
    FsstCounts fsst;                   // FSST chunks of h_chunks
    SplitPlan split;                   // balanced split after h_chunks on the device (waves 0: none)
    ByteCount bytes;                   // algorithmic bytes of one launch
    hipStream_t stream = nullptr;
    SideStream side;                   // FSST kernels overlapping the main decode kernel
    std::vector<hipEvent_t> ev_pool;   // per-launch (start, stop) pairs since last sync
    uint32_t ev_used = 0;
    Resident() = default;
    Resident(const Resident &) = delete;
    Resident &operator=(const Resident &) = delete;
    ~Resident() {
        if (dev < 0) return;
        hipSetDevice(dev);
        if (stream) hipStreamSynchronize(stream);
        if (side.stream) hipStreamSynchronize(side.stream);
        if (stream) hipStreamDestroy(stream);
        if (side.stream) hipStreamDestroy(side.stream);
        if (side.fork) hipEventDestroy(side.fork);
        if (side.join) hipEventDestroy(side.join);
        side.release_cu();
        for (auto e : ev_pool) hipEventDestroy(e);
    }
};

FLS_ENGINE_END

struct fls_table {
    std::vector<int> devices;          // the connection's GPUs (row groups shard over them)
    std::shared_ptr<MappedFile> mapped;  // fls_read_fls: the file and its validated metadata (shared)
    std::shared_ptr<fls::engine::ConnRes> res;  // the connection's scan resources (outlive a disconnect)
    const fls_connection *conn = nullptr;  // who owns the sets built from this table (a token: never dereferenced)
    std::vector<uint8_t> owned;
    const uint8_t *img = nullptr;
    uint64_t len = 0;
    fls::FileMeta meta;
    std::vector<std::string> names;
    bool registered = false;        // img pinned with hipHostRegister (FLS_SCAN_PIN=1)
    bool pin_tried = false;
    void *map = nullptr;            // fls_read_fls: the file, mapped read-only
    size_t map_len = 0;

    // device-resident mode: one part per GPU (fls_device_upload)
    std::vector<std::unique_ptr<fls::engine::Resident>> resident;
    uint32_t launches = 0;

    fls::engine::ScanCtx scan, mat;
    std::vector<fls::engine::HostTerm> filter;  // fls_scan_filter: applies to the next fls_scan_begin / fls_aggregate
    std::vector<std::vector<fls::engine::HostTerm>> alts;  // fls_scan_filter_alternatives: OR-ed, AND-ed to the filter
    std::vector<fls_agg_expr> exprs;  // fls_aggregate_exprs: what FLS_AGG_SUM_EXPR's spec.col indexes
    std::vector<std::vector<fls::engine::HostTerm>> conds;  // fls_aggregate_conditions: what spec.cond - 1 indexes
    std::vector<fls::engine::HostBinding> bindings;  // fls_aggregate_key_bindings: what FLS_KEY_MAPPED | i names
    std::vector<fls::engine::HostValueBinding> vbindings;  // fls_aggregate_value_bindings: what FLS_COL_MAPPED | i names
    bool dict_codes = false;        // fls_scan_dict_codes: applies to the next fls_scan_begin
    bool narrow = false;            // fls_scan_narrow: applies to the next fls_scan_begin
    bool defer_records = false;     // fls_scan_defer_records: applies to the next fls_scan_begin
    bool profiled = false;          // scanned with FLS_SCAN_PROFILE=1 (prints the totals at close)
    ~fls_table();
};

FLS_ENGINE_BEGIN

// ---- columns and chunks (flsgpu.hip) ----------------------------------------

int out_bytes_of(const fls_table *t, uint32_t c);
// FK_FLOAT / FK_INT / FK_UINT of (non-string) column c, as the filter, aggregate and top-N kernels compare it
uint8_t col_kind(const fls_table *t, uint32_t c);
bool is_fsst(const fls_table *t, uint32_t rg, uint32_t c);
// [rg0, rg1) inside the table, or FLS_ERR_ARG "<prefix>row-group range [rg0,rg1) out of bounds"
int check_rowgroup_range(const fls_table *t, uint32_t rg0, uint32_t rg1, const char *prefix);
int build_strtabs(const fls_table *t, int dev, uint32_t rg0, uint32_t rg1, DevBuf<StrT> &tab,
                  std::vector<uint64_t> &offs, std::vector<StrT> &host);
DevChunk make_devchunk(const fls_table *t, uint32_t rg, uint32_t col, const uint8_t *d_chunk, const uint8_t *d_dict,
                       uint8_t *d_out, ByteCount *bc, bool fsst_seg, uint8_t *d_heap = nullptr,
                       const uint8_t *h_heap = nullptr, uint32_t code_w = 0, const uint8_t *d_ident = nullptr);

// ---- launch policy and launches (fls_launch.hip) -----------------------------
// tn: the decode call's hooks (read_decode_tuning, fls_tuning.hpp), after
// launch_policy with the distribution resolved for the launch.

constexpr uint32_t kQueueWords = 1 + kFsstGroups;  // launch_all's d_queue
DecodeTuning launch_policy(DecodeTuning tn, const std::vector<DevChunk> &v, DecodeGeom &geom);
uint32_t order_for_launch(std::vector<DevChunk> &v, FsstCounts *fc, const DecodeTuning &tn,
                          std::vector<DevChunk> *dictwg = nullptr);
SplitPlan append_split(std::vector<DevChunk> &list, uint32_t nmain, const DecodeGeom &geom, const DecodeTuning &tn);
int fsst_config_check(const DecodeTuning &tn);
hipError_t launch_all(const DevChunk *d_chunks, uint32_t nmain, uint32_t ntotal, const FsstCounts &fc,
                      uint32_t *d_err, const DecodeGeom &geom, hipStream_t stream, uint32_t *d_queue,
                      const DecodeTuning &tn, SplitPlan plan, const SideStream *side = nullptr,
                      const DictVec *d_dictvecs = nullptr, uint32_t ndictvecs = 0);

// ---- the scan pipeline (flsgpu.hip) -------------------------------------------

bool rowgroup_may_match(const fls_table *t, uint32_t rg, const std::vector<HostTerm> &terms);
// ... under a filter with alternatives: the filter may match and (where there
// are alternatives) one of them may
bool rowgroup_may_match(const fls_table *t, uint32_t rg, const std::vector<HostTerm> &terms,
                        const std::vector<std::vector<HostTerm>> &alts);
bool topn_key_type(const ColumnMeta &c);
uint32_t select_rowgroups(const fls_table *t, const std::vector<HostTerm> &terms,
                          const std::vector<std::vector<HostTerm>> &alts, const fls_order_key *order, uint32_t k,
                          uint32_t rg0, uint32_t rg1, std::vector<uint32_t> &rgs);
int scan_setup(fls_table *t, ScanCtx &s, const ScanPlan &plan);
int scan_start(fls_table *t, ScanCtx &s);
int scan_next(fls_table *t, ScanCtx &s, fls_rowgroup *out);
// The host batch that holds row group rg, which scan s has handed out.
const HostBatch *held_batch(ScanCtx &s, uint32_t rg);
int stage_validity(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo);
// Per row group of the slot's batch its (first vector, vector count) within
// the batch into tab[2 * sl.nrg], and the most vectors one of them has (at
// least 1) into rg_vecs; fails when they do not fit the batch's hb.nvec vectors.
int rg_vec_table(const fls_table *t, const Slot &sl, uint32_t *tab, uint32_t &rg_vecs);

// ---- a batch's reduction, by ScanCtx::reduce (fill_batch calls one) ---------------

int enqueue_aggregate(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo);        // fls_scan_agg.hip
int enqueue_group_aggregate(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo);  // fls_scan_agg.hip
int enqueue_topn(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo);             // fls_scan_topn.hip
int enqueue_hash_aggregate(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo);   // fls_scan_hashagg.hip
int enqueue_keyset_build(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo);     // fls_scan_keyset.hip
int enqueue_mapbuild(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows, uint64_t in_lo);         // fls_scan_mapbuild.hip

// ---- what the builds from a scan share (fls_scan_keyset.hip) ---------------------

// The collecting range of column c over the row groups rgs, in the key order:
// the union of their valid zone maps, the physical type's whole range where
// one of them has none.
void keybuild_range(const fls_table *t, uint32_t c, const std::vector<uint32_t> &rgs, uint64_t &base, uint64_t &span);

// ---- what the aggregate calls share (fls_scan_agg.hip) ---------------------------

// The argument checks of fls_aggregate, fls_aggregate_grouped and
// fls_aggregate_hashed (`who`): the aggregates into ha, or FLS_ERR_ARG before
// any device work.
int check_aggregates(const fls_table *t, const char *who, const fls_aggregate_spec *aggs, uint32_t n,
                     uint32_t rg_begin, uint32_t rg_end, std::vector<HostAgg> &ha);
// Is aggregate h a FLOAT / DOUBLE SUM, MIN or MAX?
bool agg_is_float(const fls_table *t, const HostAgg &h);
// The aggregates of a batch as the kernels see them (sl.h_adesc -> sl.d_adesc
// on the slot's stream), over the slot's decoded columns and staged validity.
int upload_agg_descs(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl);
// The conditions the aggregates ha name, out of the table's list, into `used`
// (what ScanPlan::conds takes), ha[i].cond renumbered to index it.
void used_conditions(const fls_table *t, std::vector<HostAgg> &ha, std::vector<std::vector<HostTerm>> &used);

// ---- mapped GROUP BY keys (fls_scan_keymap.hip) ---------------------------------

// May a row of row group rg carry a key of inner binding b?  (as IN_SET prunes)
bool binding_may_match(const fls_table *t, uint32_t rg, const HostBinding &b);
// The batch's probe of the scan's bindings, after the filter's kernels on the
// slot's mask: the derived key columns into sl.d_kcode / sl.d_kvalid.
int enqueue_keymap(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows);

// ---- mapped columns (fls_scan_valuemap.hip) --------------------------------------

// The bits of the table's value bindings that aggregates ha and (hash
// aggregate) keys name; every FLS_COL_MAPPED | i in them has a binding i
// (check_aggregates and hash_check refused the others).
uint32_t used_value_bindings(const std::vector<HostAgg> &ha, const std::vector<uint32_t> *keys);
// May a row of row group rg carry a key of inner value binding b?  (binding_may_match)
bool value_binding_may_match(const fls_table *t, uint32_t rg, const HostValueBinding &b);
// Drops from rgs the row groups an inner binding among the used ones rules
// out; how many went.
uint32_t prune_value_bindings(const fls_table *t, const std::vector<HostValueBinding> &vb, uint32_t vused,
                              std::vector<uint32_t> &rgs);
// Operand or key `c` of an aggregate call, a column or FLS_COL_MAPPED | i: is
// it FLOAT / DOUBLE (a mapped column never is), and do its values sign-extend?
bool operand_is_float(const fls_table *t, uint32_t c);
bool operand_is_signed(const fls_table *t, uint32_t c);
// Where the kernels read operand or key `c` of the slot's batch: the decoded
// column, its bytes per value, FK_* kind and staged validity (NULL: none), or
// for FLS_COL_MAPPED | i the derived column enqueue_mapval filled (8 bytes;
// validity: NULL for an inner binding, whose misses left the mask).
struct OperandRef {
    const uint8_t *col = nullptr;
    const uint64_t *valid = nullptr;
    uint8_t ob = 0, kind = 0;
};
OperandRef operand_ref(const fls_table *t, const ScanCtx &s, const Slot &sl, uint32_t c);
// The batch's gather of the scan's used value bindings, where enqueue_keymap
// runs: the derived columns into sl.d_mval / sl.d_mvalid.
int enqueue_mapval(fls_table *t, ScanCtx &s, ScanDev &d, Slot &sl, uint64_t rows);

// A reducing scan on the table's scan context under its filter: nothing is
// delivered; fold(rg, hb) sees every surviving row group once, in scan order,
// with the host batch that holds its partial results, and returns 0 or the
// error that ends the scan.  plan names the range and the reduction; `what`
// ("aggregate", "top-N") goes into the internal error of a missing batch.
template <class Fold>
int reduce_scan(fls_table *t, ScanPlan plan, const char *what, Fold &&fold) {
    const std::vector<uint8_t> none(std::max<size_t>(1, t->meta.cols.size()), 0);  // nothing is delivered
    plan.devices = t->devices;
    plan.col_mask = none.data();
    plan.filter = &t->filter;
    plan.alts = &t->alts;
    ScanCtx &s = t->scan;
    int rc = scan_setup(t, s, plan);
    if (!rc) rc = scan_start(t, s);
    if (rc) return rc;
    fls_rowgroup rg;
    while ((rc = scan_next(t, s, &rg)) == 1) {
        const HostBatch *hb = held_batch(s, rg.rowgroup);
        if (!hb) return fail(FLS_ERR_STATE, "internal: %s batch of row group %u not found", what, rg.rowgroup);
        if (const int frc = fold(rg, *hb)) return frc;
    }
    return rc < 0 ? rc : 0;
}

FLS_ENGINE_END
