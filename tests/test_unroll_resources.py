"""The two unroll_kernel instantiations that SHIP (csrc/actor_unroll.h), from the code objects' own metadata (tools/isa_scan.py, as
tests/test_kernel_resources.py): what decides that two tiles share a CU -- 256 registers per lane, no scratch, and the LDS the
header reckons with: the body's three [32][H] images plus the resident hidden state."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shipped():
    from marbler_amd import build as hip_build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_scan
    if not os.path.exists(hip_build.LIB):
        pytest.skip("librobogym_hip.so is not built")
    try:
        return isa_scan.scan_library(hip_build.LIB)
    except RuntimeError as exc:
        pytest.skip(str(exc))


def test_unroll_kernels_fit_two_tiles_per_cu(shipped):
    hits = {k: r["resources"] for k, r in shipped.items() if "unroll_kernel" in k}
    assert len(hits) == 2, sorted(hits)
    assert not [k for k in hits if "actor_kernel" in k], "test_kernel_resources.py counts the kernels of that name"
    for h, lds_kb in ((64, 32), (128, 64)):
        (name, r), = [(k, r) for k, r in hits.items() if f"unroll_kernelILi{h}E" in k]
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 256, (name, r)
        assert r["lds"] <= lds_kb * 1024, (name, r)
        assert r["lds"] == 4 * 32 * h * 4, (name, r)      # 3 + 1 images of [32][H] float32: nothing else crept in
