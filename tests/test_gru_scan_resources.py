"""The four GRU scan kernels that SHIP (csrc/gru_scan.h), from the code objects' own metadata (tools/isa_scan.py, as
tests/test_nstep_returns_resources.py): no scratch, the LDS the header reckons with -- forward the tile's hidden state twice
[2][32][H + 1], backward the staged gradient of gh twice [2][32][3 H + 1], and three rows of 32 row numbers each -- and registers
within the one wavefront per SIMD, one workgroup per CU, that DESIGN.md section 4 "Trainable actor" states."""
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


def test_gru_scan_kernels_hold_their_weights_in_registers_without_scratch(shipped):
    hits = {k: r["resources"] for k, r in shipped.items() if "gru_scan_" in k and "_kernel" in k}
    assert len(hits) == 4, sorted(hits)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for H in (64, 128):
        for which, words in (("forward", 2 * 32 * (H + 1)), ("backward", 2 * 32 * (3 * H + 1))):
            (r,) = [r for k, r in hits.items() if f"gru_scan_{which}_kernel" in k and f"ILi{H}E" in k]
            assert r["scratch"] == 0 and r["spill"] == 0, (which, H, r)
            arrays = 4 * (words + 3 * 32)
            assert arrays == {("forward", 64): 17024, ("forward", 128): 33408, ("backward", 64): 49792, ("backward", 128): 98944}[which, H]
            assert arrays <= r["lds"] <= arrays + 256, (which, H, r)                      # (alignment between them:) nothing else crept in
            # the wavefront's block of W_hh lives in registers: 3 H / 2 of them, beside the accumulators -- above the 256 that two
            # wavefronts per SIMD would leave each, within the 512 of one
            regs = r["vgpr"]                                                              # (the unified file: accumulator registers included)
            assert 3 * H // 2 + r["agpr"] <= regs <= 512 and (H == 64 or regs > 256), (which, H, r)
            assert f"| {which} | {H} | {r['vgpr']} | {r['agpr']} | {r['lds']} |" in design, (which, H, r)   # DESIGN states them as they are
    # one workgroup per CU at H = 128 is what the registers allow (4 wavefronts, one per SIMD, above 256 registers each)
    assert "one workgroup per CU" in design
