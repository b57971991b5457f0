"""The host half of the key-set build from a scan:
keyset_from_bitmap / keyset_finish of csrc/fls_keyset.hpp against keyset_build,
through tests/fuzz/keyset_bitmap_host.cpp -- a stand-alone program with its own
main over the host-only header, built with -fsanitize=address,undefined.
Nothing is loaded into Python under a sanitizer."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "duckdb-fastlane_amd" / "csrc"


def test_keyset_from_bitmap_equals_keyset_build_under_asan(tmp_path):
    """seeded signed and unsigned sets, the type edges, a single key, the empty
    set, keys sharing one home slot, spans at 2^32 - 1 and both sides of both
    auto-rule conditions, each through a bitmap over a range wider than
    [min, max]: every field and every image word of forms 0, 1 and 2 equals
    keyset_build's, and KS_TOO_WIDE / KS_TOO_MANY come out where it gives them"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path / "keyset_bitmap_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", str(CSRC), str(ROOT / "tests" / "fuzz" / "keyset_bitmap_host.cpp"),
                    "-o", str(out)], check=True)
    r = subprocess.run([str(out), "120", "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"sanitizer report or mismatch\n{r.stderr[-4000:]}"
    assert r.stdout.startswith("sets ") and r.stdout.rstrip().endswith("failures 0"), r.stdout
    assert int(r.stdout.split()[1]) >= 140, r.stdout        # the random sets and every named one ran
