"""The resident form of the 16-lane-row step kernels in the SHIPPED library (CPU tier: tools/isa_scan.py on the code objects of
marbler_amd/librobogym_hip.so).  Sixteen kernels (4 scenarios x N = 5..8) beside the sixteen by-value ones, told apart by the
trailing `true` of their template arguments (csrc/step_group.h):

* their kernel descriptors ask for preloaded kernel arguments: the image's address, the actions, the seed, auto_reset and the
  grid, 8 dwords, reach a wave in scalar registers;
* behind the preload entry (256 bytes in: in front of it lies the compatibility prologue for firmware that does not preload)
  the first vector load from memory is issued before anything waits for scalar memory -- the first link of the wave's chain is
  no longer a trip to the argument segment;
* their argument loads obey the rule of tests/test_row_kernel_args.py: `s_load_*` only before the first controller or inside a
  sampler block; everything behind the sub-step loop reads the vector-register copy;
* all thirty-two row kernels: no spill, at most 128 bytes of scratch, three waves per SIMD.
"""
import os
import sys
import tempfile

import pytest

from test_row_kernel_args import first_controller, sampler_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

BY_VALUE, RESIDENT = "ELb0ELi16ET", "ELb0ELi16ELb1ET"
PRELOADED_DWORDS = 8   # image 2, actions 2, seed 2, auto_reset 1, grid 1 (kernel_args.h ResidentCall up to `io`)
PRELOAD_ENTRY = 256


@pytest.fixture(scope="module")
def library():
    import isa_scan
    from marbler_amd import build as hip_build
    assert os.path.exists(hip_build.LIB), "librobogym_hip.so is not built"
    insts, res, preload = {}, {}, {}
    with tempfile.TemporaryDirectory() as d:
        for co in isa_scan.extract_code_objects(hip_build.LIB, d):
            r = {k: v for k, v in isa_scan.resources(co).items() if "2rg11step_kernelILi" in k and (BY_VALUE in k or RESIDENT in k)}
            if not r:
                continue
            res.update(r)
            preload.update({k: v for k, v in isa_scan.kernarg_preload(co).items() if k in r})
            if any(RESIDENT in k for k in r):
                insts.update({k: v for k, v in isa_scan.disassemble(co).items() if k in r and RESIDENT in k})
    return insts, res, preload


def test_sixteen_resident_kernels_beside_the_sixteen_by_value_ones(library):
    insts, res, preload = library
    assert len(insts) == 16 and sum(1 for k in res if BY_VALUE in k) == 16 and len(res) == 32, sorted(res)
    for scn in range(4):
        for n in (5, 6, 7, 8):
            stem = f"_ZN2rg11step_kernelILi{scn}ELi8ELb0ELi{n}ELb0ELi16E"
            assert sum(1 for k in res if k.startswith(stem)) == 2, stem


def test_resident_kernels_ask_for_preloaded_arguments(library):
    _, res, preload = library
    for name in sorted(res):
        length, offset = preload[name]
        if RESIDENT in name:
            assert (length, offset) == (PRELOADED_DWORDS, 0), (name, length, offset)
        else:
            assert length == 0, (name, length)   # the by-value kernels' translation unit keeps its flags


def test_first_vector_load_is_issued_before_any_wait_for_scalar_memory(library):
    insts, _, _ = library
    for name, code in sorted(insts.items()):
        entry = next(i for i, it in enumerate(code) if it.addr == code[0].addr + PRELOAD_ENTRY)
        # in front of the entry: the compatibility prologue, which ends in a branch to it
        assert any(it.op == "s_branch" and it.target == code[entry].addr for it in code[:entry]), name
        first_load = next(i for i in range(entry, len(code)) if code[i].op.startswith("global_load"))
        waits = [it for it in code[entry:first_load] if it.op == "s_waitcnt" and "lgkmcnt" in it.args]
        assert not waits, f"{name}: waits for scalar memory before its first vector load: {waits[0]!r}"
        assert not any(it.op.startswith("s_load") for it in code[entry:first_load]), name


def test_argument_loads_only_in_the_prologue_or_a_sampler_block(library):
    insts, _, _ = library
    for name, code in sorted(insts.items()):
        ctrl, blocks = first_controller(code), sampler_blocks(code)
        loads = [i for i, it in enumerate(code) if it.op.startswith("s_load_")]
        assert loads and loads[0] < ctrl
        assert len(blocks) == 2 and all(ctrl < b < e and e - b < len(code) // 4 for b, e in blocks), (name, blocks, len(code))
        stray = [code[i] for i in loads if i > ctrl and not any(b < i < e for b, e in blocks)]
        assert not stray, f"{name}: {len(stray)} argument loads behind the first controller and outside the sampler, e.g. {stray[0]!r}"
        assert sum(1 for it in code[ctrl:] if it.op == "v_readlane_b32") >= 20, name
        assert not any(it.op.startswith("flat_") for it in code), f"{name}: a flat access (a pointer of the image not known to be global)"


def test_row_kernel_resources(library):
    _, res, _ = library
    for name, r in sorted(res.items()):
        assert r["spill"] == 0 and r["scratch"] <= 128 and r["occupancy"] >= 3, (name, r)
