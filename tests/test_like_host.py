"""The pattern compiler and the shared LIKE matcher (csrc/fls_strmatch.hpp) on
the CPU under AddressSanitizer and UBSan: tests/fuzz/like_host.cpp, a
stand-alone program, reads (string, pattern, escape) triples -- the pool x
pattern matrix of like_ref.py plus seeded random pairs over an alphabet with
2-, 3- and 4-byte characters, stray continuation bytes, `%`, `_` and the
escape bytes -- and prints the compiler's facts and the matcher's verdict;
each line must equal the Python reference (like_ref.ref_like / facts).
Nothing is loaded into Python under a sanitizer.  CPU only."""
import random
import shutil
import subprocess
from pathlib import Path

import pytest

from like_ref import PATTERNS, POOL, facts, ref_like

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "duckdb-fastlane_amd" / "csrc"
NRANDOM = 6000


def hexs(b):
    return b.hex() if b else "-"


def random_triples(n):
    rng = random.Random(20250607)
    chars = [b"a", b"b", b"c", "é".encode(), "€".encode(), "\U0001F600".encode(), b"\x80", b"\xbf", b"\xe2", b"\xf0\x9f",
             b"%", b"_", b"\\"]
    pchars = chars + [b"%", b"%", b"_", b"_", b"a", b"b"]
    out = []
    for _ in range(n):
        s = b"".join(rng.choice(chars[:10]) if rng.random() < 0.85 else rng.choice(chars) for _ in range(rng.randint(0, 14)))
        esc = rng.choice([None, None, 0x5C, ord("a"), ord("%")])
        if rng.random() < 0.5:
            p = b"".join(rng.choice(pchars) for _ in range(rng.randint(0, 7)))
        else:
            # a pattern made from the string, so that many pairs match: bytes kept (escaped
            # where an escape is in effect), dropped under a % or replaced by _
            p = b""
            for b in s:
                r = rng.random()
                if r < 0.2:
                    p += b"%"
                elif r < 0.35:
                    p += b"_"
                elif r < 0.45:
                    continue
                elif esc is not None and (b in (0x25, 0x5F, esc) or r < 0.5):
                    p += bytes([esc, b])
                else:
                    p += bytes([b])
        out.append((s, p, esc))
    return out


def expected_line(s, p, esc):
    try:
        ntok, min_len, prefix, ends, exact = facts(p, esc)
    except ValueError:
        return "1 0 0 - 0 0 0"
    if ntok > 256:
        return "2 0 0 - 0 0 0"
    return f"0 {ntok} {min_len} {hexs(prefix)} {int(ends)} {int(exact)} {int(ref_like(s, p, esc))}"


@pytest.fixture(scope="module")
def like_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("like_host") / "like_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", str(CSRC), str(ROOT / "tests" / "fuzz" / "like_host.cpp"),
                    "-o", str(out)], check=True)

    def run(triples):
        path = out.parent / "triples.txt"
        path.write_text("".join(f"{hexs(s)} {hexs(p)} {esc or 0}\n" for s, p, esc in triples))
        r = subprocess.run([str(out), str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, f"sanitizer report or failure\n{r.stderr[-4000:]}"
        lines = r.stdout.splitlines()
        assert len(lines) == len(triples)
        return lines
    return run


def check(like_host, triples):
    for (s, p, esc), got in zip(triples, like_host(triples)):
        assert got == expected_line(s, p, esc), (s, p, esc)


def test_matrix_matches_the_reference(like_host):
    check(like_host, [(s, p, esc) for p, esc in PATTERNS for s in POOL])


def test_random_pairs_match_the_reference(like_host):
    triples = random_triples(NRANDOM)
    verdicts = [ref_like(s, p, esc) for s, p, esc in triples if not expected_line(s, p, esc).startswith("1")]
    assert 0.05 < sum(verdicts) / len(verdicts) < 0.95      # the pairs both match and fail to
    check(like_host, triples)


def test_compile_statuses(like_host):
    # a trailing escape, 256 and 257 tokens, a run of % counted once, an escaped escape at the end
    triples = [(b"x", b"abc\\", 0x5C), (b"x", b"\\", 0x5C), (b"x", b"ab\\\\", 0x5C), (b"a" * 256, b"a" * 256, None),
               (b"a" * 257, b"a" * 257, None), (b"a" * 256, b"%" * 50 + b"a" * 255, None),
               (b"a" * 256, b"%" * 50 + b"a" * 256, None), (b"", b"a" * 300 + b"\\", 0x5C)]
    got = like_host(triples)
    assert [g.split()[0] for g in got] == ["1", "1", "0", "0", "2", "0", "2", "2"]
    check(like_host, triples[:4] + triples[5:6])
