// fls_launch.hip -- the launch policy and the launches of one decode, a scan's
// batches (fill_batch) and a device-resident table (decode_part) alike.  The
// A/B hooks arrive as one DecodeTuning (fls_tuning.hpp), read once per decode call.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "fls_engine.hpp"

using namespace fls;
using namespace fls::engine;

static_assert(kFsstVariantDefault == kFsstDefault, "fls_tuning.hpp: FLS_FSST_VARIANT's default is kFsstDefault");

FLS_ENGINE_BEGIN

// Tuning for one launch: the default (no distribution bits) switches to the
// balanced split when the launch has fewer main-kernel chunks than resident
// waves (the scan pipeline's 8-row-group batches: ~120 chunks for ~4,096
// waves), where whole-chunk work items would leave most waves idle.  Large
// launches keep the work queue: same-buffer A/B on SF100 lineitem, c3 and c4
// found the split no faster than the queue (profiles/r1/abenv_bal_*.txt).
DecodeTuning launch_policy(DecodeTuning tn, const std::vector<DevChunk> &v, DecodeGeom &geom) {
    if (tn.list.flags & (POLICY_STATIC | POLICY_BALANCED | POLICY_QUEUE)) return tn;
    size_t nmain = 0;
    for (const DevChunk &d : v) nmain += d.enc != ENC_FSST;
    if (geom.grid <= 0) geom.grid = decode_grid_size(4 * (geom.p_bytes + geom.v_bytes));
    if (nmain < decode_waves(geom)) tn.list.flags |= POLICY_BALANCED;
    return tn;
}

// FSST chunks go last (their own kernels: string-parallel ones first, then
// code-parallel ones, each group numbering its vectors through vec_base);
// returns how many lead (main kernel) and the FSST counts
// dictwg (a table decode, decode_part): the chunks the dictionary-string grid
// takes (dictstr_eligible, FLS_DICT_WG) leave v for it, in the order its
// workgroups are laid out in: ascending output address, as S interleaved
// streams (below).
uint32_t order_for_launch(std::vector<DevChunk> &v, FsstCounts *fc, const DecodeTuning &tn,
                          std::vector<DevChunk> *dictwg) {
    const int policy = tn.list.flags;
    if (dictwg) {
        dictwg->clear();
        const int mode = tn.list.dict_wg;
        uint64_t vecs = 0;
        for (const DevChunk &d : v)
            if (dictstr_eligible(d)) vecs += d.nvec;
        const uint64_t need = mode == 2 ? 1 : (uint64_t)tn.list.dict_wg_min_vecs_per_cu * (uint64_t)device_cus();
        if (mode > 0 && vecs > 0 && vecs >= need && vecs <= UINT32_MAX) {
            auto rest = std::stable_partition(v.begin(), v.end(), [](const DevChunk &d) { return !dictstr_eligible(d); });
            dictwg->assign(rest, v.end());
            v.erase(rest, v.end());
            std::stable_sort(dictwg->begin(), dictwg->end(),
                             [](const DevChunk &a, const DevChunk &b) { return a.out < b.out; });
            // S write streams (FLS_DICT_WG_STREAMS): the sorted list cut into
            // S runs of as many chunks, taken round-robin, so S regions fill
            // at once, each in ascending address.  lineitem_full SF100, the
            // four string columns: S = 1 / 2 / 4 / 8 -> 6.90 / 5.96 / 5.72 /
            // 5.74 ms (S = 4: one stream per column); one ascending sequence
            // over several buffers is no faster than the main decode there
            // (6.87 ms).  c4: 2.56 / 2.50 / 2.50 / 2.51 ms
            // (profiles/r7/abenv_dictwg_streams_*.txt)
            const size_t n = dictwg->size(), S = std::min<size_t>((size_t)tn.list.dict_wg_streams, n);
            if (S > 1) {
                std::vector<DevChunk> il;
                il.reserve(n);
                for (size_t i = 0; il.size() < n; ++i)
                    for (size_t s = 0; s < S; ++s)
                        if (s * n / S + i < (s + 1) * n / S) il.push_back((*dictwg)[s * n / S + i]);
                dictwg->swap(il);
            }
        }
    }
    auto mid = std::stable_partition(v.begin(), v.end(), [](const DevChunk &d) { return d.enc != ENC_FSST; });
    std::stable_sort(mid, v.end(), [](const DevChunk &a, const DevChunk &b) {
        return fsst_group(a.vbits) < fsst_group(b.vbits);
    });
    if (policy & POLICY_FULL_PREFETCH)
        for (auto it = v.begin(); it != mid; ++it) it->max_w = it->T;
    if (policy & POLICY_BALANCED) {
        // file order = row-group-major: every wave's range mixes all columns
        // (paths that run slower per byte are spread over the waves)
        std::stable_sort(v.begin(), mid, [](const DevChunk &a, const DevChunk &b) { return a.chunk < b.chunk; });
    } else if (!(policy & (POLICY_STATIC | POLICY_NO_LPT))) {
        // largest output first: the work queue then ends the launch on small chunks
        std::stable_sort(v.begin(), mid, [](const DevChunk &a, const DevChunk &b) {
            return (uint64_t)a.nvec * a.ob > (uint64_t)b.nvec * b.ob;
        });
    }
    *fc = FsstCounts();
    for (auto it = mid; it != v.end(); ++it) {
        const int g = fsst_group(it->vbits);
        it->vec_base = fc->vecs[g];
        fc->vecs[g] += it->nvec;
        fc->n[g]++;
    }
    return (uint32_t)(mid - v.begin());
}

// Append the balanced split of the main chunks to the descriptor list (as
// extra DevChunk slots, so it uploads with it); plan.waves == 0 when the
// policy does not split.
SplitPlan append_split(std::vector<DevChunk> &list, uint32_t nmain, const DecodeGeom &geom, const DecodeTuning &tn) {
    if (nmain == 0) return SplitPlan();
    const DecodeTuning::List &l = tn.list;
    std::vector<uint32_t> pos;
    SplitPlan plan;
    if (l.flags & POLICY_BALANCED)
        plan = balanced_split(list.data(), nmain, decode_waves(geom), (uint32_t)l.static_pct, (uint32_t)l.tail_pieces, pos);
    else if (!(l.flags & (POLICY_STATIC | POLICY_NO_LPT)) && l.guided_min_vecs)
        plan = guided_split(list.data(), nmain, decode_waves(geom), (uint32_t)l.guided_factor,
                            (uint32_t)l.guided_min_vecs, pos);
    else
        return SplitPlan();
    const size_t k = list.size();
    list.resize(k + (pos.size() * 4 + sizeof(DevChunk) - 1) / sizeof(DevChunk));
    memcpy(list.data() + k, pos.data(), pos.size() * 4);
    return plan;
}

// The FSST kernels a launch with this policy and FLS_FSST_VARIANT would run
// must be in this build: the product library holds each kernel's default only
// (fls_fsst.hip), the experiment library every variant (make lab).  A stale
// tuning variable fails the decode with FLS_ERR_CONFIG instead of running a
// kernel it did not ask for.
int fsst_config_check(const DecodeTuning &tn) {
    const DecodeTuning::Launch &x = tn.launch;
    if (!x.fsst_variant_hook.ok)
        return fail(FLS_ERR_CONFIG, "FLS_FSST_VARIANT=%s is not a variant number", x.fsst_variant_hook.text.c_str());
    // the fused kernel's FSST-part bits (experiments)
    if (x.fused_x_hook.given && (!x.fused_x_hook.ok || !fused_x_built(x.fused_x)))
        return fail(FLS_ERR_CONFIG,
                    "FLS_FUSED_X=%s is not in this build: the product library holds the default fused kernel "
                    "only; experiments need FLS_LIB=libflsgpu_lab.so (make lab) -- unset FLS_FUSED_X",
                    x.fused_x_hook.text.c_str());
    const int bpl = (tn.list.flags & POLICY_FSST16) ? 16 : 8;
    if (!fsst_variant_built(x.fsst_variant, true, bpl) || !fsst_variant_built(x.fsst_variant, false, bpl))
        return fail(FLS_ERR_CONFIG,
                    "FSST kernel variant %d (%d bytes per lane) is not in this build: the product library holds the "
                    "default kernels only; experiments need FLS_LIB=libflsgpu_lab.so (make lab)%s",
                    x.fsst_variant, bpl, x.fsst_variant_hook.given ? " -- unset FLS_FSST_VARIANT" : "");
    return 0;
}

// CU-partitioned overlap: the main decode (HBM-bound) and the FSST kernels
// (VALU / LDS-bound) each start alone on their own CU set instead of sharing
// every CU's LDS and issue slots (the co-resident split lost to running them
// one after the other at the 8-GPU share, profiles/r3/abenv_sf12_split_r3zl.txt):
//   stream A (CUs with index mod 32 < m): full decode grid, then FSST;
//   stream B (the other CUs):             full FSST grid, then decode.
// Both kinds drain shared queues, so whichever set finishes its kind first
// joins the other.  A mask that takes m of every 32 CU indices gives each XCD
// the same share whether the mask's bits run XCD by XCD or round-robin over
// the XCDs (m a multiple of 8).
template <class LaunchGroup>
static hipError_t launch_cu_split(const DevChunk *d_chunks, uint32_t nmain, const FsstCounts &fc, uint32_t *d_err,
                           const DecodeGeom &geom, hipStream_t stream, uint32_t *d_queue, SideStream *side,
                           const DecodeTuning::Launch &ov, int cus, const FsstLaunch (&how)[kFsstGroups],
                           LaunchGroup &launch_group) {
    const int m = ov.overlap_cu_split;
    uint32_t mask_a[8] = {}, mask_b[8] = {};
    int na = 0, nb = 0;
    for (int i = 0; i < std::min(cus, 256); ++i) {
        if (i % 32 < m) {
            mask_a[i / 32] |= 1u << (i % 32);
            ++na;
        } else {
            mask_b[i / 32] |= 1u << (i % 32);
            ++nb;
        }
    }
    if (na == 0 || nb == 0) return hipErrorInvalidValue;
    if (side->cu_m != m) {
        side->release_cu();
        hipError_t e = hipExtStreamCreateWithCUMask(&side->cu_a, 8, mask_a);
        if (e == hipSuccess) e = hipExtStreamCreateWithCUMask(&side->cu_b, 8, mask_b);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&side->join_a, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&side->join_b, hipEventDisableTiming);
        if (e != hipSuccess) {
            side->release_cu();
            return e;
        }
        side->cu_m = m;
    }
    const uint32_t shmem = 4 * (geom.p_bytes + geom.v_bytes);
    const int bpc = std::max(1, (geom.grid > 0 ? geom.grid : decode_grid_size(shmem)) / std::max(1, cus));
    DecodeGeom ga = geom, gb = geom;
    ga.grid = na * bpc;
    gb.grid = nb * bpc;
    FsstLaunch ha[kFsstGroups], hb[kFsstGroups];
    for (int g = 0; g < kFsstGroups; ++g) {
        ha[g] = hb[g] = how[g];
        ha[g].queue = hb[g].queue = d_queue + 1 + g;
        ha[g].reset_queue = hb[g].reset_queue = false;
        ha[g].grid_cus = na;
        hb[g].grid_cus = nb;
    }
    hipError_t e = hipMemsetAsync(d_queue, 0, kQueueWords * sizeof(uint32_t), stream);
    if (e == hipSuccess) e = hipEventRecord(side->fork, stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(side->cu_a, side->fork, 0);
    if (e == hipSuccess) e = hipStreamWaitEvent(side->cu_b, side->fork, 0);
    if (e == hipSuccess)
        e = launch_decode(d_chunks, nmain, d_err, ga, side->cu_a, d_queue, nullptr, SplitPlan(), true, ov.overlap_decode_prio);
    for (int g = 0; g < kFsstGroups && e == hipSuccess; ++g) e = launch_group(g, side->cu_b, hb[g]);
    if (e == hipSuccess)
        e = launch_decode(d_chunks, nmain, d_err, gb, side->cu_b, d_queue, nullptr, SplitPlan(), true, ov.overlap_decode_prio);
    for (int g = 0; g < kFsstGroups && e == hipSuccess; ++g) e = launch_group(g, side->cu_a, ha[g]);
    if (e == hipSuccess) e = hipEventRecord(side->join_a, side->cu_a);
    if (e == hipSuccess) e = hipEventRecord(side->join_b, side->cu_b);
    if (e == hipSuccess) e = hipStreamWaitEvent(stream, side->join_a, 0);
    if (e == hipSuccess) e = hipStreamWaitEvent(stream, side->join_b, 0);
    return e;
}

// d_queue[0] = main decode work queue, [1 + g] = FSST piece counter of kernel
// group g (FsstCounts).
//
// Without a side stream (scan batches) the FSST kernels follow the main one
// on its stream.  With one (a table decode), the FSST kernels (VALU-bound)
// overlap the main decode kernel (HBM-bound):
//   main stream: narrow decode grid (decode_bpc blocks per CU), then a full
//                FSST grid;
//   side stream: narrow FSST grid (fsst_wpc waves per CU), then a full decode
//                grid.
// Every grid of a kind drains one shared queue (decode chunks / FSST pieces),
// so no work is done twice, and whichever kind runs out first, its stream
// follows with a full grid of the other kind onto the freed wave slots.  The
// split holds whichever kernel the hardware dispatches first.
// Measured on lineitem_full SF100 (same-buffer A/B, profiles/r1/abenv_overlap.txt):
// 26.7 ms serial -> 24.3 ms at 1 decode block + 12..20 FSST waves per CU
// (2 blocks + 8..12 waves: 24.7 ms).  The kernel trace shows the overlap phase
// moving ~4.9 TB/s together, below the 5.6 TB/s of the main kernel alone: the
// two compete for the CUs' LDS and issue slots as well as for HBM.
//
// Overlap split (launch_all): blocks per CU of the narrow main decode grid
// and FSST waves per CU of the narrow FSST grid; knobs FLS_OVERLAP_DECODE_BPC /
// FLS_OVERLAP_FSST_WPC (0 FSST waves = no overlap).
// Overlap vs one-after-the-other at the per-GPU shares of 1/2/4/8-GPU runs
// (same-buffer A/B on lineitem_full, profiles/r2/abenv_overlap_scales.txt,
// abenv_sf12p5.txt, abenv_minvecs.txt, abenv_overlap_grid.txt,
// abenv_overlap_prio.txt): overlapped is faster at SF25 (5.90 vs 6.26 ms),
// SF50 (12.0 vs 12.9) and SF100 (23.1 vs 26.0, 23.9 vs 26.4); at SF12.5 (286
// FSST vectors per CU, the per-GPU share of an 8-GPU run) serial was faster on
// three boxes of four (3.41 vs 3.46, 3.11 vs 3.18, 3.36 vs 3.45 ms; 3.16 vs
// 3.09 on the fourth).  So launches with fewer than 400 FSST vectors per CU
// ran serially (FLS_OVERLAP_MIN_VECS_PER_CU).  With round 3's faster FSST
// kernel serial also wins at SF25 (572 vectors per CU: 6.41 vs 6.51 ms) and
// at SF12.5 against every split tried (3.22 vs 3.34-3.45 ms;
// profiles/r3/abenv_sf25_split_r3zl.txt, abenv_sf12_split_r3zl.txt), so the
// threshold is 800; SF50 (1,144 vectors per CU) and SF100 (2,288) stay
// overlapped: 11.17 vs 11.82 and 22.14 vs 23.80 ms (abenv_sf50_split_r3zm.txt,
// abenv_sf100_split_r3zm.txt).  The main kernel's wave issue
// priority while overlapped (FLS_OVERLAP_DECODE_PRIO, s_setprio 1-3) measured
// within 0.1 % of the default.
hipError_t launch_all(const DevChunk *d_chunks, uint32_t nmain, uint32_t ntotal, const FsstCounts &fc,
                      uint32_t *d_err, const DecodeGeom &geom, hipStream_t stream, uint32_t *d_queue,
                      const DecodeTuning &tn, SplitPlan plan, const SideStream *side, const DictVec *d_dictvecs,
                      uint32_t ndictvecs) {
    const int policy = tn.list.flags;
    const DecodeTuning::Launch &ov = tn.launch;
    // the dictionary-string grid first, on the same stream: its chunks are not
    // in d_chunks, and a launch may consist of it alone
    if (ndictvecs) {
        const hipError_t de = launch_dictstr(d_dictvecs, ndictvecs, d_err, stream);
        if (de != hipSuccess || ntotal == 0) return de;
    }
    // a guided plan only orders the serial launch: the overlapped and
    // CU-split launches drain whole chunks from a queue several grids share
    const uint32_t *d_split = plan.waves ? reinterpret_cast<const uint32_t *>(d_chunks + ntotal) : nullptr;
    const bool balanced = d_split && !plan.guided;
    const bool sp = (policy & POLICY_FSST_SP) != 0;
    FsstLaunch how[kFsstGroups];
    for (int g = 0; g < kFsstGroups; ++g) {
        how[g].bytes_per_lane = (policy & POLICY_FSST16) ? 16 : 8;
        how[g].variant = ov.fsst_variant;  // fsst_config_check'ed
        how[g].small = g == 0 || g == 2;
        how[g].seg = g < 2;
        how[g].seg_cap = ov.fsst_seg_cap;
        how[g].waves_per_cu = ov.fsst_wpc;  // (standalone launches: the narrow grids name their own)
        how[g].piece = (uint32_t)ov.fsst_piece;
    }
    auto launch_group = [&](int g, hipStream_t st, const FsstLaunch &h) -> hipError_t {
        const DevChunk *dc = d_chunks + nmain + fc.first(g);
        if (g == 2 && sp && !h.queue) return launch_fsst_sp(dc, fc.n[g], fc.vecs[g], d_err, st);
        return launch_fsst(dc, fc.n[g], fc.vecs[g], d_err, st, h);
    };
    const int cus = device_cus();
    const uint64_t fsst_vecs = fc.total_vecs();
    if (ov.overlap_cu_split > 0 && side && side->stream && nmain > 0 && fsst_vecs > 0 && !balanced && !sp &&
        !(policy & POLICY_STATIC))
        return launch_cu_split(d_chunks, nmain, fc, d_err, geom, stream, d_queue, const_cast<SideStream *>(side),
                               ov, cus, how, launch_group);
    // fused: one kernel pulling main chunks and FSST pieces from two queues
    // (launch_fused), when every FSST chunk is of one segmented kind
    {
        int g1 = -1, ng = 0;
        for (int g = 0; g < kFsstGroups; ++g)
            if (fc.n[g]) {
                g1 = g;
                ++ng;
            }
        // an FSST kernel variant A/B (FLS_FSST_VARIANT, experiment library) runs
        // the standalone FSST kernels: the fused kernel holds only the default's
        // FSST part, so fusing would measure the default instead
        const bool variant = ov.fsst_variant != kFsstDefault;
        if (ov.fused > 0 && !variant && ((ng == 1 && nmain > 0) || ov.fused == 2) && ng <= 1 && g1 < 2 && !balanced && !sp &&
            !(policy & POLICY_STATIC) &&
            fsst_vecs >= (uint64_t)ov.fused_min_vecs_per_cu * (uint64_t)cus) {
            const int g = std::max(0, g1);  // (no FSST chunks: the main decode alone, in the fused kernel)
            FusedLaunch how;
            how.fsst_per16 = (uint32_t)ov.fused_fsst16;
            how.piece = (uint32_t)ov.fused_piece;
            how.halving = ov.fused_halving;
            how.fsst_static_pct = (uint32_t)ov.fused_static_pct;
            how.static_first = ov.fused_static_first;
            how.waves_per_cu = ov.fused_wpc;
            how.x = ov.fused_x;
            how.tail_chunks = (uint32_t)ov.fused_tail;
            how.tail_split = (uint32_t)ov.fused_tail_split;
            // waves starting on FSST: 6 of 16 for large launches (SF100:
            // 21.79 ms against 21.93 with 5), 5 below 1,000 FSST vectors per
            // CU (SF12.5: 3.115 against 3.133 ms with 6; profiles/r5/).
            // With the DICT VARCHAR chunks on their own grid the main queue
            // holds about half the bytes and the FSST part needs more of the
            // waves: 8 of 16 (SF100: 20.57 ms against 20.91 with 6 and 20.71
            // with 9; SF12.5: 2.704 against 2.820 with 5 and 2.714 with 6,
            // while without the grid 7 and 8 lose to 6;
            // profiles/r7/abenv_dictwg_fsst16_*.txt)
            if (!ov.fused_fsst16_given) how.fsst_per16 = ndictvecs ? 8u : fsst_vecs < 1000ull * (uint64_t)cus ? 5u : 6u;
            return launch_fused(d_chunks, nmain, d_chunks + nmain + fc.first(g), fc.n[g], fc.vecs[g], g == 0, d_err,
                                geom, stream, d_queue, how);
        }
    }
    const bool overlap = side && side->stream && ov.overlap_fsst_wpc > 0 && nmain > 0 && fsst_vecs > 0 &&
                         fsst_vecs >= (uint64_t)ov.overlap_min_vecs_per_cu * (uint64_t)cus && !balanced && !sp &&
                         !(policy & POLICY_STATIC);
    hipError_t e = hipSuccess;
    if (overlap) {
        DecodeGeom narrow = geom;
        const uint32_t shmem = 4 * (geom.p_bytes + geom.v_bytes);
        narrow.grid = std::min(geom.grid > 0 ? geom.grid : decode_grid_size(shmem), cus * ov.overlap_decode_bpc);
        e = hipMemsetAsync(d_queue, 0, kQueueWords * sizeof(uint32_t), stream);
        if (e == hipSuccess) e = hipEventRecord(side->fork, stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(side->stream, side->fork, 0);
        FsstLaunch narrow_how[kFsstGroups];
        for (int g = 0; g < kFsstGroups; ++g) {
            how[g].queue = d_queue + 1 + g;
            how[g].reset_queue = false;
            narrow_how[g] = how[g];
            narrow_how[g].waves_per_cu = ov.overlap_fsst_wpc;
        }
        // main stream: narrow decode, then full FSST
        // (a guided plan: both decode grids drain its items from the shared queue)
        const uint32_t *gs = d_split && plan.guided && ov.overlap_guided ? d_split : nullptr;
        const SplitPlan gp = gs ? plan : SplitPlan();
        if (e == hipSuccess)
            e = launch_decode(d_chunks, nmain, d_err, narrow, stream, d_queue, gs, gp, true, ov.overlap_decode_prio);
        // side stream: narrow FSST, then full decode
        for (int g = 0; g < kFsstGroups && e == hipSuccess; ++g) e = launch_group(g, side->stream, narrow_how[g]);
        if (e == hipSuccess)
            e = launch_decode(d_chunks, nmain, d_err, geom, side->stream, d_queue, gs, gp, true, ov.overlap_decode_prio);
        for (int g = 0; g < kFsstGroups && e == hipSuccess; ++g) e = launch_group(g, stream, how[g]);
        if (e == hipSuccess) e = hipEventRecord(side->join, side->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(stream, side->join, 0);
        return e;
    }
    e = launch_decode(d_chunks, nmain, d_err, geom, stream, (policy & POLICY_STATIC) ? nullptr : d_queue, d_split, plan);
    // FSST groups in order; chunks whose strings are all <= 255 bytes without
    // segment tables go to the string-parallel kernel under POLICY_FSST_SP
    for (int g = 0; g < kFsstGroups && e == hipSuccess; ++g) e = launch_group(g, stream, how[g]);
    return e;
}

FLS_ENGINE_END
