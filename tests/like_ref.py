"""The reference of the LIKE tests (test_like.py, test_like_sql.py,
test_like_host.py): a memoised recursive matcher written from the semantics in
include/flsgpu.h -- deliberately not the engine's two-cursor algorithm -- the
pattern facts, the string pool and the pattern list.

`%` any byte sequence; `_` one character = one byte plus every directly
following continuation byte ((b & 0xC0) == 0x80); an escape byte e followed by
x matches x literally; everything else matches itself; the whole string must
be consumed."""
import sys

import numpy as np

from helpers import filter_mask

ANY1, ANYN = 256, 257


def parse(pat: bytes, esc):
    """the pattern as elements: 0..255 literal, ANY1, ANYN (runs of % kept);
    ValueError on a trailing escape byte"""
    out, i = [], 0
    while i < len(pat):
        b = pat[i]
        if esc is not None and b == esc:
            if i + 1 >= len(pat):
                raise ValueError("trailing escape")
            out.append(pat[i + 1])
            i += 2
            continue
        out.append(ANYN if b == 0x25 else ANY1 if b == 0x5F else b)
        i += 1
    return out


_memo = {}


def ref_like(s: bytes, pat: bytes, esc=None) -> bool:
    key = (s, pat, esc)
    if key in _memo:
        return _memo[key]
    el = parse(pat, esc)
    seen = {}

    def go(i, j):
        k = (i, j)
        if k in seen:
            return seen[k]
        if j == len(el):
            r = i == len(s)
        elif el[j] == ANYN:
            r = go(i, j + 1) or (i < len(s) and go(i + 1, j))
        elif i >= len(s):
            r = False
        elif el[j] == ANY1:
            e = i + 1
            while e < len(s) and (s[e] & 0xC0) == 0x80:
                e += 1
            r = go(e, j + 1)
        else:
            r = s[i] == el[j] and go(i + 1, j + 1)
        seen[k] = r
        return r

    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * (len(s) + len(el)) + 1000))
    try:
        r = bool(go(0, 0))
    finally:
        sys.setrecursionlimit(old)
    _memo[key] = r
    return r


def facts(pat: bytes, esc=None):
    """(ntok, min_len, prefix, ends_anyn, exact) of the compiled pattern: runs
    of % are one token; min_len counts literals and `_`; prefix is the literal
    bytes before the first wildcard"""
    el = parse(pat, esc)
    tok = [e for k, e in enumerate(el) if not (e == ANYN and k and el[k - 1] == ANYN)]
    prefix = bytearray()
    for e in tok:
        if e >= 256:
            break
        prefix.append(e)
    return (len(tok), sum(e != ANYN for e in tok), bytes(prefix), bool(tok) and tok[-1] == ANYN,
            all(e < 256 for e in tok))


# ----------------------------------------------------------------- the strings
S36 = b"abcdefghijklmnopqrstuvwxyz0123456789"
S13 = b"abcdefghijklm"
A299B = b"a" * 299 + b"b"
A300 = b"a" * 300
E2, E3, E4 = "é".encode(), "€".encode(), "\U0001F600".encode()   # 2-, 3- and 4-byte characters
POOL = [
    b"", b"a", b"b", b"abcd", b"abce", b"abcde", b"abcdx", b"abcdefghijkl", b"abcdefghijkL", S13, b"abcdefghijklM",
    S36, S36[:35] + b":", S36[:35],                     # lengths 0, 1, 4, 5, 12, 13, 36; equal up to byte 4, 12, 35
    b"100%", b"a_b", b"a\\b", b"axb", b"50%_off\\now", b"%", b"_", b"\\",       # % _ \ as data
    b"caf" + E2, b"caf" + E2 + b"s", E3 + b"uro", b"x" + E4 + b"y", b"x" + E4, E2 + E3 + E4,
    b"ab\x80c", b"\x80", b"ab\xe2\x82", b"abc\xc3", b"\x80\x80",              # a stray 0x80, truncated lead bytes
    b"abxababc", b"xabyabab", b"ababab", b"xx abc and abc", b"the green abc of abcdefghijklmnop",
    b"aXaYaZaWb", b"aaaab", b"aaab",
    A299B, A300, b"a" * 255, b"a" * 254 + b"b",
]
assert len(set(POOL)) == len(POOL)

BS = 0x5C
# (pattern, escape byte or None)
PATTERNS = [
    (b"", None), (b"%", None), (b"%%", None), (b"_", None), (b"__%", None),
    (b"abcd", None), (S13, None), (S36, None),                                   # exact
    (b"a%", None), (b"abcd%", None), (b"abcde%", None), (S13 + b"%", None),       # prefixes of 1, 4, 5, 13 bytes
    (b"%b", None), (b"%6789", None), (b"%klm", None),                           # suffixes
    (b"%x%", None), (b"%abc%", None), (b"a%b%c", None),
    (b"%ab%abc", None),                                                         # must backtrack
    (b"%a%a%a%a%b", None),
    (b"caf_", None), (b"caf_s", None), (b"_uro", None), (b"x_y", None), (b"x_", None), (b"___", None),
    (b"ab_c", None), (b"ab_", None), (b"abc_", None), (b"__", None),             # _ over stray and truncated bytes
    (b"100\\%", BS), (b"a\\_b", BS), (b"a\\\\b", BS), (b"%\\%\\_%", BS),          # escaped % _ and escape byte
    (b"\\a\\b\\c\\d%", BS),                                                     # escape before ordinary bytes
    (b"\\%", BS), (b"a_b", None), (b"a\\_b", None),                             # (no escape in effect: \ is a byte)
    (b"%a%%", ord("a")), (b"aab%", ord("a")), (b"a_%", ord("a")),                # escape byte 'a'
    (b"%" + b"a" * 254 + b"b", None), (b"a" * 255 + b"%", None),                 # 256 tokens
]
OPS = ["like", "not_like"]


def pat_text(pat, esc):
    return f"{pat if len(pat) < 40 else pat[:12] + b'...' + pat[-4:]!r} esc={None if esc is None else chr(esc)!r}"


def term(col, op, pat, esc):
    return (col, op, pat if esc is None else (pat, bytes([esc])))


def like_hits(strings, pat, esc):
    """bool per string (the reference run once per distinct string)"""
    return np.array([ref_like(s, pat, esc) for s in strings], dtype=bool)


def like_mask(cols: dict, terms, n: int, valid=None) -> np.ndarray:
    """helpers.filter_mask extended by ("like" / "not_like", pattern or
    (pattern, escape)) terms, each a clause of its own"""
    valid = valid or {}
    out = np.ones(n, dtype=bool)
    rest = []
    for t in terms:
        col, op, val = t[:3]
        if op not in OPS:
            rest.append(t)
            continue
        pat, esc = val if isinstance(val, tuple) else (val, None)
        pat = pat.encode() if isinstance(pat, str) else pat
        esc = None if esc is None else (esc.encode() if isinstance(esc, str) else esc)[0]
        hit = like_hits(cols[col][:n], pat, esc)
        if op == "not_like":
            hit = ~hit
        ok = valid.get(col)
        out &= hit if ok is None else hit & ok[:n]
    if rest:
        out &= filter_mask(cols, rest, n, valid)
    return out


def route(s: bytes, pat: bytes, esc):
    """which exit of the kernel decides (s, pattern), from the facts alone"""
    ntok, min_len, prefix, _, exact = facts(pat, esc)
    if len(s) < min_len or (exact and len(s) > ntok):
        return "length"
    k = min(4, len(prefix))
    if k and s[:k] != prefix[:k]:
        return "prefix"
    return "inline" if len(s) <= 12 else "pointer"


def needs_retry(s: bytes, pat: bytes, esc) -> bool:
    """a match in which the literal tail after the last % occurs, all but its
    last byte, earlier in the string: the first try of that segment fails"""
    if esc is not None or b"_" in pat or b"%" not in pat or not ref_like(s, pat, esc):
        return False
    tail = pat.rsplit(b"%", 1)[1]
    if len(tail) < 2:
        return False
    k = s.find(tail[:-1])
    return 0 <= k < len(s) - len(tail)
