"""cond_kernel (csrc/fls_cond.hip) evaluates the terms of up to eight
conditions per 64-row word with filter_kernel's per-row code and keeps nothing
per lane between conditions, so it uses no scratch and spills no VGPR.  Read
from the built library's code-object metadata on the CPU
(scripts/kernel_resources.py), as tests/test_like_resources.py does."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "scripts"))
LIB = ROOT / "duckdb-fastlane_amd" / "libflsgpu.so"


def test_cond_kernel_uses_no_scratch(_built):
    import kernel_resources
    res = kernel_resources.resources(str(LIB))
    hits = {k: v for k, v in res.items() if "cond_kernel" in k}
    assert len(hits) == 1, sorted(res)
    for name, r in hits.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)       # at least 4 waves per SIMD
