"""The n-step returns kernels that SHIP (csrc/nstep_returns.h), from the code objects' own metadata (tools/isa_scan.py, as
tests/test_td_targets_resources.py): no scratch, the LDS the header reckons with -- the state's image [32][257], the activations
[32][H + 1], the wavefronts' partial sums [H / 32][32], the tile's flags and the episode's 4096 mask bytes -- and registers that leave
room for the two workgroups per CU the header claims."""
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


def test_nstep_returns_kernels_fit_two_workgroups_per_cu(shipped):
    hits = {k: r["resources"] for k, r in shipped.items() if "nstep_returns_kernel" in k}
    assert len(hits) == 2, sorted(hits)
    for H in (64, 128):
        (r,) = [r for k, r in hits.items() if f"ILi{H}E" in k]
        assert r["scratch"] == 0 and r["spill"] == 0, r
        arrays = 4 * (32 * 257 + 32 * (H + 1) + (H // 32) * 32 + 32) + 4096
        assert arrays == {64: 45696, 128: 54144}[H]                                       # the header's figures
        assert arrays <= r["lds"] <= arrays + 256, r                                      # (alignment between them:) nothing else crept in
        assert 2 * r["lds"] <= 160 * 1024                                                 # two workgroups per CU
        # a workgroup is one wavefront per SIMD; two of them share a SIMD's 512 registers per lane
        assert r["vgpr"] + r["agpr"] <= 256, r
