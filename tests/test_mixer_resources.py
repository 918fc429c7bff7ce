"""The five mixer kernels that SHIP (csrc/mixer_grad.h), from the code objects' own metadata (tools/isa_scan.py, as
tests/test_gru_scan_resources.py): no scratch, and the LDS the header reckons with -- the qmix forward kernel td_qmix_kernel's
60 032 bytes (two workgroups per CU), the backward kernel 72 576 bytes for up to 8 agents (two per CU) and 105 344 bytes for up to
16 (one per CU), within the 160 KiB of a CU -- as DESIGN.md section 4 "Trainable mixer" states them."""
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


def test_mixer_kernels_use_no_scratch_and_the_lds_the_header_states(shipped):
    hits = {k: r["resources"] for k, r in shipped.items() if "MgArgs" in k}
    assert len(hits) == 5, sorted(hits)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    image = lambda nmax: 32 * (32 * nmax + 1)                                          # noqa: E731  the state / p1 image
    fixed = 32 * 193 + 3 * 32 * 16 + 2 * 32 * 33 + 3 * 32                              # h1; x, dx, actions; pf, du; flags, dy, row offsets
    want = {"mix_gather_forward_kernel": 0, "mix_gather_backward_kernel": 0, "mix_qmix_forward_kernel": 60032,
            "mix_qmix_backward_kernelILi8E": 4 * (image(8) + fixed), "mix_qmix_backward_kernelILi16E": 4 * (image(16) + fixed)}
    assert want["mix_qmix_backward_kernelILi8E"] == 72576 and want["mix_qmix_backward_kernelILi16E"] == 105344
    for name, lds in want.items():
        (r,) = [r for k, r in hits.items() if name in k]
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert lds <= r["lds"] <= lds + 512, (name, r)                                # (alignment, and the vote's word:) nothing else crept in
        assert r["lds"] <= 160 * 1024 and r["vgpr"] <= 256, (name, r)                 # two wavefronts per SIMD fit the register file
        if lds:
            assert f"| {name.replace('ILi', '<').replace('E', '>') if 'ILi' in name else name} | {r['vgpr']} | {r['agpr']} | {r['lds']} | {163840 // r['lds']} |" in design, (name, r)
