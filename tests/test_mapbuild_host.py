"""The host half of the map build from a scan:
mapbuild_merge / mapbuild_codes of csrc/fls_mapbuild.hpp and
valuemap_finish_sorted / keymap_finish_sorted against valuemap_build /
keymap_build, through tests/fuzz/mapbuild_host.cpp -- a stand-alone program with
its own main over the host-only headers, built with
-fsanitize=address,undefined.  Nothing is loaded into Python under a
sanitizer."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "duckdb-fastlane_amd" / "csrc"


def test_merged_parts_finish_like_the_builders_under_asan(tmp_path):
    """seeded signed and unsigned pair lists (every third a key map), the type
    edges of keys and values, a single pair, the empty map and spans on both
    sides of both auto-rule conditions, each as presence words + compact values
    over a range wider than [min, max], dealt to one, two and three parts with
    overlapping keys: every field and every image word of forms 0, 1 and 2
    equals valuemap_build's / keymap_build's, and the cross-part conflict,
    VM_TOO_WIDE and KM_BAD_VALUE come out where the builders give them"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path / "mapbuild_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", str(CSRC), str(ROOT / "tests" / "fuzz" / "mapbuild_host.cpp"),
                    "-o", str(out)], check=True)
    r = subprocess.run([str(out), "120", "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"sanitizer report or mismatch\n{r.stderr[-4000:]}"
    assert r.stdout.startswith("maps ") and r.stdout.rstrip().endswith("failures 0"), r.stdout
    assert int(r.stdout.split()[1]) >= 150, r.stdout        # the random maps and every named one ran
