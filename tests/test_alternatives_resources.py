"""alt_kernel (csrc/fls_alt.hip) evaluates the ordinary terms of up to eight
alternatives per 64-row word with filter_kernel's per-row code and keeps one
accumulator word between them; alt_merge_kernel ORs at most eight plane words
into a mask word and reduces 16 lanes.  Neither uses scratch or spills a VGPR.
Read from the built library's code-object metadata on the CPU
(scripts/kernel_resources.py), as tests/test_agg_filter_resources.py does."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "scripts"))
LIB = ROOT / "duckdb-fastlane_amd" / "libflsgpu.so"


@pytest.mark.parametrize("kernel", ["alt_kernel", "alt_merge_kernel"])
def test_alt_kernels_use_no_scratch(_built, kernel):
    import kernel_resources
    res = kernel_resources.resources(str(LIB))
    hits = {k: v for k, v in res.items() if kernel in k}
    assert len(hits) == 1, sorted(res)
    for name, r in hits.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)       # at least 4 waves per SIMD
