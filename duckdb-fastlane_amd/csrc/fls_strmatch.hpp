// fls_strmatch.hpp -- string pattern terms of the pushed-down filter
// (`column LIKE pattern [ESCAPE c]` / `NOT LIKE`, FLS_CMP_LIKE / FLS_CMP_NOT_LIKE
// in include/flsgpu.h).
//
// Standard library only (no HIP include): the pattern compiler and the matcher
// run on the host for pruning and checks, a stand-alone CPU program can drive
// this header (tests/fuzz/like_host.cpp), and strmatch_kernel
// (fls_strmatch.hip) calls the very same matcher per row.
//
// Semantics (DuckDB's LIKE): the pattern is a byte string; `%` matches any
// sequence of bytes, the empty one included; `_` matches one character: one
// byte and every directly following continuation byte ((b & 0xC0) == 0x80),
// which defines the result on ill-formed UTF-8 too (a stray continuation byte
// the match position stands on is a character of its own); every other byte
// matches itself, case-sensitively; the whole string must be consumed.  With
// an escape byte e, e followed by any byte x matches x literally; a pattern
// ending in a lone e does not compile.
//
// A compiled pattern is an array of uint16_t tokens: 0..255 a literal byte,
// kTokAny1 (`_`), kTokAnyN (`%`, runs collapsed), with the facts the kernel's
// early exits use.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define FLS_STRMATCH_HD __host__ __device__
#else
#define FLS_STRMATCH_HD
#endif

namespace fls {

constexpr uint16_t kTokAny1 = 256;      // `_`
constexpr uint16_t kTokAnyN = 257;      // `%`
constexpr uint32_t kMaxPatTokens = 256; // per compiled pattern
constexpr uint32_t kMaxPatTerms = 8;    // pattern terms per filter

enum PatStatus : int { PAT_OK = 0, PAT_TRAILING_ESCAPE = 1, PAT_TOO_LONG = 2 };

struct CompiledPattern {
    std::vector<uint16_t> tok;
    uint32_t min_len = 0;      // bytes a matching string has at least: literals + one per `_`
    std::string prefix;        // the literal bytes before the first wildcard
    bool ends_anyn = false;    // the last token is `%`
    bool exact = true;         // no wildcard: only a string of tok.size() bytes can match
};

// escape: 0 for none, else the escape byte (1..255).  PAT_TOO_LONG leaves the
// tokens compiled so far (more than kMaxPatTokens) in out.
inline int pattern_compile(const uint8_t *pat, size_t n, uint32_t escape, CompiledPattern &out) {
    out = CompiledPattern();
    bool in_prefix = true;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t b = pat[i];
        uint16_t t;
        if (escape && b == escape) {
            if (i + 1 >= n) return PAT_TRAILING_ESCAPE;
            t = pat[++i];
        } else if (b == '%') {
            t = kTokAnyN;
        } else if (b == '_') {
            t = kTokAny1;
        } else {
            t = b;
        }
        if (t == kTokAnyN && !out.tok.empty() && out.tok.back() == kTokAnyN) continue;  // %% is %
        if (t < 256) {
            if (in_prefix) out.prefix.push_back((char)t);
            ++out.min_len;
        } else {
            in_prefix = false;
            out.exact = false;
            if (t == kTokAny1) ++out.min_len;
        }
        out.tok.push_back(t);
        if (out.tok.size() > kMaxPatTokens) return PAT_TOO_LONG;
    }
    out.ends_anyn = !out.tok.empty() && out.tok.back() == kTokAnyN;
    return PAT_OK;
}

// Does s[0, len) match tok[0, ntok)?  Two cursors and the last `%` with the
// string position it was tried at: on a mismatch the segment after that `%`
// is retried one byte further.  One remembered `%` suffices: a later start of
// a segment never ends earlier, so the first position a segment matches at
// leaves the most string for the rest.  At most (len + 1) * (ntok + 1) steps,
// no recursion, no array.  Tokens above kTokAnyN match nothing.
FLS_STRMATCH_HD inline bool like_match(const uint8_t *s, uint32_t len, const uint16_t *tok, uint32_t ntok) {
    uint32_t si = 0, ti = 0;
    uint32_t star_t = ~0u, star_s = 0;
    for (;;) {
        if (ti < ntok) {
            const uint32_t t = tok[ti];
            if (t == kTokAnyN) {
                if (ti + 1 == ntok) return true;  // a trailing % takes the rest
                star_t = ti++;
                star_s = si;
                continue;
            }
            // the string is spent and a token that needs a byte is left: a later
            // start of the segment has no more bytes
            if (si >= len) return false;
            if (t == kTokAny1) {
                ++si;
                while (si < len && (s[si] & 0xC0) == 0x80) ++si;
                ++ti;
                continue;
            }
            if (t == s[si]) {
                ++si;
                ++ti;
                continue;
            }
        } else if (si == len) {
            return true;
        }
        if (star_t == ~0u || star_s >= len) return false;
        si = ++star_s;
        ti = star_t + 1;
    }
}

}  // namespace fls
