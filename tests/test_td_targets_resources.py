"""The two TD-target kernels that SHIP (csrc/td_targets.h), from the code objects' own metadata (tools/isa_scan.py, as
tests/test_unroll_resources.py): no scratch, and the LDS the header reckons with -- the state's image [32][257], the first layers'
[32][193], the agent values [32][16] and the flags -- so that two workgroups share a CU."""
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


def test_td_target_kernels_fit_two_workgroups_per_cu(shipped):
    hits = {k: r["resources"] for k, r in shipped.items() if "td_qmix_kernel" in k or "td_gather_kernel" in k}
    assert len(hits) == 2, sorted(hits)
    (qmix,), (gather,) = [[r for k, r in hits.items() if name in k] for name in ("td_qmix_kernel", "td_gather_kernel")]
    for r in (qmix, gather):
        assert r["scratch"] == 0 and r["spill"] == 0, r
    arrays = 4 * (32 * 257 + 32 * 193 + 32 * 16 + 32)
    assert arrays <= qmix["lds"] <= arrays + 256, qmix                                # (alignment between them:) nothing else crept in
    assert 2 * qmix["lds"] <= 160 * 1024                                              # two workgroups per CU
    assert qmix["vgpr"] + qmix["agpr"] <= 256, qmix                                   # six waves on four SIMDs: two on one at the most
    assert gather["lds"] == 0 and gather["vgpr"] + gather["agpr"] <= 64, gather
