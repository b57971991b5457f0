"""The three kernels of the map build from a scan (csrc/fls_mapbuild.hip,
DESIGN.md section 32): mapbuild_kernel collects a batch's selected pairs into
the call's array, mapbuild_presence_kernel and mapbuild_gather_kernel compact
it.  Each appears once, with no scratch and no spill, at most 64 VGPRs (eight
waves per SIMD, as keyset_build_kernel) and in LDS only the waves' counts: 4 of
the 256-thread collect block, 16 of a 1024-thread compaction block.  Read from
the built library's gfx950 code object; no GPU is needed.

What the build gives (VGPR / SGPR / LDS bytes): mapbuild_kernel 13 / 66 / 16,
mapbuild_presence_kernel 17 / 24 / 64, mapbuild_gather_kernel 16 / 18 / 64."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "duckdb-fastlane_amd" / "libflsgpu.so"

LDS_CAP = {"mapbuild_kernel": 4 * 4, "mapbuild_presence_kernel": 16 * 4, "mapbuild_gather_kernel": 16 * 4}


@pytest.mark.parametrize("kernel", sorted(LDS_CAP))
def test_mapbuild_kernel_resources(kernel):
    if not LIB.exists():
        pytest.skip("libflsgpu.so not built")
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    res = kernel_resources.resources(str(LIB))
    # (the mangled name carries the length: "mapbuild_kernel" alone, not a suffix of another kernel's name)
    hits = {k: v for k, v in res.items() if f"{len(kernel)}{kernel}E" in k}
    assert len(hits) == 1, sorted(res)
    for name, r in hits.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 64, (name, r)
        assert r["lds"] <= LDS_CAP[kernel], (name, r)
