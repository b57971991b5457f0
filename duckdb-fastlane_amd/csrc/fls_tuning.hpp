// fls_tuning.hpp -- the decode launch's A/B-measurement and test hooks
// (environment variables) as ONE typed struct, read once per decode call and
// handed down to fls_launch.hip.  Host only, standard library only; no other
// file of csrc/ calls getenv on these names but the experiment library's own
// launcher, fls_fsst_lab.hip (tests/test_tuning.py).
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <string>
#include <tuple>

namespace fls {

// Decode work distribution (A/B knob FLS_DECODE_POLICY, read per call so both
// arms run on the same buffers): 0 = work queue, largest chunks first
// (default); bit 0 = static grid-stride split; bit 1 = keep column order.
// bit 2 = full-width register prefetch for every chunk (descriptor max_w = T).
// bit 3 = FSST chunks with segment tables on the code-parallel kernel
// (FLS_FSST_SEG=0) instead of the segmented one.
// bit 4 = FSST rounds of 16 compressed bytes per lane instead of 8.
// bit 5 = balanced static split of vectors over the resident waves, chunks in
// file (row-group-major) order (balanced_split).  bit 6 = work queue even for
// small launches (launch_policy).  bit 7 = FSST chunks whose strings are all
// <= 255 bytes on the string-parallel kernel (default: every FSST chunk on the
// code-parallel kernel; same-buffer A/B profiles/r1/abenv_fsst_cp.txt).
enum : int {
    POLICY_STATIC = 1, POLICY_NO_LPT = 2, POLICY_FULL_PREFETCH = 4, POLICY_FSST_NOSEG = 8, POLICY_FSST16 = 16,
    POLICY_BALANCED = 32, POLICY_QUEUE = 64, POLICY_FSST_SP = 128
};

// FLS_FSST_VARIANT's default: kFsstDefault (fls_decode.hpp, which fls_launch.hip checks it against)
constexpr int kFsstVariantDefault = 8 | 4 | 64;

// A hook fsst_config_check parses strictly: its text for the error message and
// whether it is a whole number in 0..INT_MAX (then atoi's value, which the launch takes)
struct StrictHook {
    bool given = false, ok = true;
    std::string text;
};

struct DecodeTuning {
    // Which chunks go on which grid and in what order: the key of a resident
    // table's cached descriptor list (Resident::list_key), so a change of any
    // of these, and of nothing else, rebuilds it.
    struct List {
        // FLS_DECODE_POLICY's POLICY_* bits, POLICY_FSST_NOSEG also from
        // FLS_FSST_SEG=0 (which changes the descriptors, make_devchunk);
        // launch_policy resolves the distribution bits on a copy
        int flags = 0;
        // balanced split (balanced_split): FLS_STATIC_PCT = % of the bytes
        // split statically, FLS_TAIL_PIECES = tail pieces per wave for the rest
        int static_pct = 100, tail_pieces = 2;
        // FLS_BLOCKS_PER_CU as the key sees it (0 = unset; blocks_per_cu_cap
        // is what the grid takes): it only enters the grid when the list is rebuilt
        int blocks_per_cu = 0;
        // guided tail (guided_split): FLS_GUIDED_MIN_VECS = smallest piece in
        // vectors (0 = whole chunks only), FLS_GUIDED_FACTOR = pieces per wave
        // of the remaining work
        int guided_min_vecs = 0, guided_factor = 2;
        // The dictionary-string grid (fls_dictstr.hip): FLS_DICT_WG = 0 keeps every
        // chunk on the main decode, 1 (default) moves the eligible DICT VARCHAR
        // chunks of a table decode to their own grid when they hold at least
        // FLS_DICT_WG_MIN_VECS_PER_CU vectors per CU, 2 moves them whatever the size.
        // Below the threshold the second launch's drain outweighs the write rate
        // (lineitem_full, full step, grid forced against off: +3.9 % at 11 vectors per
        // CU, +1.4 % at 23, -1.2 % at 46, -1.5 % at 92, -4.2 % at 183;
        // profiles/r7/abenv_dictwg_small.txt).  FLS_DICT_WG_STREAMS: the grid's write
        // streams (order_for_launch).
        int dict_wg = 1, dict_wg_min_vecs_per_cu = 64, dict_wg_streams = 4;
        auto tie() const {
            return std::tie(flags, static_pct, tail_pieces, blocks_per_cu, guided_min_vecs, guided_factor, dict_wg,
                            dict_wg_min_vecs_per_cu, dict_wg_streams);
        }
        bool operator==(const List &o) const { return tie() == o.tie(); }
        bool operator!=(const List &o) const { return !(*this == o); }
    } list;

    // What a launch reads anew at every decode call.
    struct Launch {
        // FLS_FSST_SEG != 0 (default): FSST chunks with segment tables get the
        // segmented kernel's descriptors (make_devchunk).  Keyed through
        // list.flags' POLICY_FSST_NOSEG, which FLS_DECODE_POLICY can also set
        // without changing the descriptors: hence a field of its own.
        bool fsst_seg = true;
        // Overlap split (FLS_OVERLAP_*, launch_all).  12 FSST waves per CU beside 1
        // decode block: 1.6-2 % faster than 16 at SF100 and SF12.5 (profiles/r2/abenv_v12.txt)
        int overlap_decode_bpc = 1, overlap_fsst_wpc = 12, overlap_min_vecs_per_cu = 800;
        int overlap_decode_prio = 0;  // FLS_OVERLAP_DECODE_PRIO: s_setprio of the main kernel's waves while overlapped
        // FLS_OVERLAP_CU_SPLIT = m in 1..31: the main decode starts on the CUs whose
        // index mod 32 is < m, FSST on the others, each kind alone on its CUs
        // (0 = the co-resident split above)
        int overlap_cu_split = 0;
        // FLS_OVERLAP_GUIDED=1: the overlapped decode grids drain the guided plan's
        // items (whole chunks, then pieces) instead of whole chunks
        bool overlap_guided = false;
        // Fused launch (launch_all -> launch_fused): the default for a table
        // decode whose FSST chunks are of one segmented kind.  FLS_FUSED: 0 off
        // (serial or overlapped kernels); mode 1 (default) launches with main
        // chunks and FSST chunks of one segmented kind; mode 2 (FLS_FUSED=1)
        // also launches with only one of the two (the main decode alone in the
        // fused kernel: 2 % slower, A/B only)
        int fused = 1;
        // FLS_FUSED_FSST16 = waves of every 16 that start on FSST (when not
        // given: by launch size, launch_all), FLS_FUSED_PIECE = FSST vectors per
        // queue item, FLS_FUSED_WPC = waves per CU (0: as many as fit),
        // FLS_FUSED_STATIC_PCT = % of the FSST vectors the FSST-first waves
        // split statically before the queue, FLS_FUSED_MIN_VECS_PER_CU = the
        // FSST vectors per CU below which the launch stays serial; the others
        // as FusedLaunch's fields (fls_decode.hpp)
        bool fused_fsst16_given = false;
        int fused_fsst16 = 6, fused_piece = 2, fused_wpc = 0, fused_static_pct = 0, fused_min_vecs_per_cu = 0;
        bool fused_static_first = true, fused_halving = false;
        int fused_tail = 0, fused_tail_split = 1;
        int fused_x = 0;  // FLS_FUSED_X: the fused kernel's FSST-part bits (experiments)
        StrictHook fused_x_hook;
        // FLS_FSST_VARIANT (kFsst* bits, experiment library); FLS_FSST_SEG_CAP:
        // the segmented kernel's ring (FsstLaunch::seg_cap)
        int fsst_variant = kFsstVariantDefault;
        StrictHook fsst_variant_hook;
        int fsst_seg_cap = 4096;
        // the FSST launcher (A/B, standalone launches): FLS_FSST_WPC = waves per CU
        // where the launch names none (0: none), FLS_FSST_PIECE = vectors per
        // queue piece (0: computed)
        int fsst_wpc = 0, fsst_piece = 0;
    } launch;
};

// FLS_BLOCKS_PER_CU as decode_grid_size takes it: at most this many blocks per CU (0: unset)
inline int blocks_per_cu_cap() {
    const char *e = getenv("FLS_BLOCKS_PER_CU");
    return e ? std::max(1, atoi(e)) : 0;
}

inline StrictHook strict_hook(const char *e) {
    if (!e) return StrictHook();
    char *end = nullptr;
    const long v = strtol(e, &end, 10);
    return StrictHook{true, !(end == e || *end != 0 || v < 0 || v > 0x7FFFFFFF), e};
}

// The hooks' values in effect.  A hook that is present (an empty string too:
// atoi gives 0) is clamped into its row's range; an absent one keeps the default.
inline DecodeTuning read_decode_tuning() {
    DecodeTuning t;
    DecodeTuning::List &l = t.list;
    DecodeTuning::Launch &x = t.launch;
    const struct { const char *name; int *field; int lo, hi; } ints[] = {
        {"FLS_STATIC_PCT", &l.static_pct, 0, 100},
        {"FLS_TAIL_PIECES", &l.tail_pieces, 1, 255},
        {"FLS_BLOCKS_PER_CU", &l.blocks_per_cu, 0, 127},
        {"FLS_GUIDED_MIN_VECS", &l.guided_min_vecs, 0, 64},
        {"FLS_GUIDED_FACTOR", &l.guided_factor, 1, 255},
        {"FLS_DICT_WG", &l.dict_wg, 0, 2},
        {"FLS_DICT_WG_MIN_VECS_PER_CU", &l.dict_wg_min_vecs_per_cu, 0, 255},
        {"FLS_DICT_WG_STREAMS", &l.dict_wg_streams, 1, 31},
        {"FLS_OVERLAP_CU_SPLIT", &x.overlap_cu_split, 0, 31},
        {"FLS_OVERLAP_DECODE_BPC", &x.overlap_decode_bpc, 1, INT_MAX},
        {"FLS_OVERLAP_FSST_WPC", &x.overlap_fsst_wpc, 0, INT_MAX},
        {"FLS_OVERLAP_MIN_VECS_PER_CU", &x.overlap_min_vecs_per_cu, 0, INT_MAX},
        {"FLS_OVERLAP_DECODE_PRIO", &x.overlap_decode_prio, 0, 3},
        {"FLS_FUSED_FSST16", &x.fused_fsst16, 0, 16},
        {"FLS_FUSED_PIECE", &x.fused_piece, 1, 64},
        {"FLS_FUSED_WPC", &x.fused_wpc, 0, INT_MAX},
        {"FLS_FUSED_STATIC_PCT", &x.fused_static_pct, 0, 100},
        {"FLS_FUSED_TAIL", &x.fused_tail, 0, INT_MAX},
        {"FLS_FUSED_TAIL_SPLIT", &x.fused_tail_split, 1, 64},
        {"FLS_FUSED_X", &x.fused_x, INT_MIN, INT_MAX},
        {"FLS_FUSED_MIN_VECS_PER_CU", &x.fused_min_vecs_per_cu, 0, INT_MAX},
        {"FLS_FSST_VARIANT", &x.fsst_variant, INT_MIN, INT_MAX},
        {"FLS_FSST_SEG_CAP", &x.fsst_seg_cap, INT_MIN, INT_MAX},
        {"FLS_FSST_WPC", &x.fsst_wpc, 0, INT_MAX},
        {"FLS_FSST_PIECE", &x.fsst_piece, 1, 64},
    };
    for (const auto &r : ints)
        if (const char *e = getenv(r.name)) *r.field = std::min(r.hi, std::max(r.lo, atoi(e)));
    const struct { const char *name; bool *field; } bools[] = {
        {"FLS_OVERLAP_GUIDED", &x.overlap_guided},
        {"FLS_FUSED_STATIC_FIRST", &x.fused_static_first},
        {"FLS_FUSED_HALVING", &x.fused_halving},
        {"FLS_FSST_SEG", &x.fsst_seg},
    };
    for (const auto &r : bools)
        if (const char *e = getenv(r.name)) *r.field = atoi(e) != 0;
    if (const char *e = getenv("FLS_DECODE_POLICY")) l.flags = atoi(e) & 0xFF;
    if (!x.fsst_seg) l.flags |= POLICY_FSST_NOSEG;
    if (const char *e = getenv("FLS_FUSED")) x.fused = std::min(2, std::max(0, atoi(e) == 1 ? 2 : atoi(e)));
    x.fused_fsst16_given = getenv("FLS_FUSED_FSST16") != nullptr;
    x.fused_x_hook = strict_hook(getenv("FLS_FUSED_X"));
    x.fsst_variant_hook = strict_hook(getenv("FLS_FSST_VARIANT"));
    return t;
}

}  // namespace fls
