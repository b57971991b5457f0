"""mapval_kernel (csrc/fls_mapval.hip) gathers the mapped columns of an
aggregate call: one kernel, no scratch, no spill, at most 64 VGPRs + AGPRs (the
register file then still holds eight waves per SIMD, the ceiling the sibling
kernels' tests hold) and the four wave counts in LDS.
Read from the built library's gfx950 code object; no GPU is needed."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "duckdb-fastlane_amd" / "libflsgpu.so"


def test_mapval_kernel_resources():
    if not LIB.exists():
        pytest.skip("libflsgpu.so not built")
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    res = kernel_resources.resources(str(LIB))
    hits = {k: v for k, v in res.items() if "mapval_kernel" in k}
    assert len(hits) == 1, sorted(res)
    for name, r in hits.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 64, (name, r)
        assert r["lds"] <= 16, (name, r)
