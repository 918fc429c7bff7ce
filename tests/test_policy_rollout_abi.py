"""rg_policy_rollout on the CPU tier: the binding's struct matches the library's, the kernels fit the design (LDS of the actor's
images + the resident hidden state + the step's scratch within a CU's 160 KB, one workgroup of H / 32 wavefronts), and the
entry point refuses what it does not support before anything reaches a GPU."""
import ctypes as C
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_policy_io_struct_matches_the_binding():
    from marbler_amd import _lib
    lib = _lib.load()
    assert lib.rg_abi_version() == 7
    assert lib.rg_sizeof_policy_io() == C.sizeof(_lib.RgPolicyIO)
    assert lib.rg_policy_rollout(None, None, 1, None, None, 1, 0) != 0   # a NULL handle is refused, nothing launched


def test_policy_rollout_kernels_resources():
    import isa_scan
    from marbler_amd import build
    found = {}
    with tempfile.TemporaryDirectory() as d:
        for co in isa_scan.extract_code_objects(build.LIB, d):
            for k, r in isa_scan.resources(co).items():
                if "policy_rollout_kernel" in k:
                    found[k] = r
    assert len(found) == 26   # (4 scenarios x GW 4, 8, 16 + ArcticTransport x GW 4) x hidden 64, 128
    for k, r in found.items():
        h = 128 if "ELi128E" in k else 64
        assert "actor_kernel" not in k
        assert r["lds"] <= 160 * 1024 and r["lds"] >= (3 * 32 + 64) * h * 4, (k, r)
