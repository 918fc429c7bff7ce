"""Where the 16-lane-row step kernels of the SHIPPED library fetch their arguments (CPU tier: tools/isa_scan.py on the code
objects of marbler_amd/librobogym_hip.so).

A row kernel is one dependent chain per wave, and an `s_load_*` from the argument block that is waited for in front of the
instruction that needs it costs that chain a scalar-cache round trip.  The kernels therefore fetch the block in the prologue -- the
scalar bursts in front of the first controller, and a copy of the whole block in four vector registers that everything behind the
sub-step loop reads with v_readlane_b32 (csrc/device_common.h load_arg_regs).  The rule checked here: in every row kernel an
`s_load_*` lies either before the first controller or inside a sampler block (reset_group: the episode reset and the draw ahead,
off the common path, which keep their loads).

How the two places are recognised in the instruction stream:
* the first controller begins with the position controller's division (k.pvl / nrm): the kernel's first v_div_scale_f32 / v_rcp_f32;
* a sampler block is the body of the wave's vote `if (__any(...))` around a call of reset_group: the smallest forward branch on
  VCC (s_cbranch_vccz / vccnz: how a vote compiles; the sampler's own per-lane `if`s branch on exec, its tests of scalar
  arguments on SCC) whose span holds one run of instructions that carry the Philox4x32 multiplier 0xD2511F53 (runs further apart
  than 400 instructions are different calls).
"""
import os
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HEADLINE = "_ZN2rg11step_kernelILi0ELi8ELb0ELi5ELb0ELi16ETnNSt9enable_ifIXeqT4_Li16EEiE4typeELi0EEEvNS_10KernelArgsE"
PARENT_HEADLINE_S_LOADS = 71   # the parent build's headline kernel: 10 in the first burst, 13 more before the first controller, 48 behind the loop
PHILOX_M0 = "0xd2511f53"
RUN_GAP = 400


@pytest.fixture(scope="module")
def row_kernels():
    import isa_scan
    from marbler_amd import build as hip_build
    assert os.path.exists(hip_build.LIB), "librobogym_hip.so is not built"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in isa_scan.extract_code_objects(hip_build.LIB, d):
            if not any("ELb0ELi16ET" in k for k in isa_scan.resources(co)):
                continue   # (one code object per translation unit: only the one with the row kernels is disassembled)
            for name, insts in isa_scan.disassemble(co).items():
                if "2rg11step_kernelILi" in name and "ELb0ELi16ET" in name:
                    out[name] = insts
    assert len(out) == 16, sorted(out)   # 4 scenarios x N = 5..8
    return out


def first_controller(insts):
    return next(i for i, it in enumerate(insts) if it.op.startswith(("v_div_scale_f32", "v_rcp_f32")))


def sampler_blocks(insts):
    """-> [(first, last)] instruction index spans, one per call of reset_group."""
    hits = [i for i, it in enumerate(insts) if PHILOX_M0 in it.args.lower()]
    runs = []
    for i in hits:
        if runs and i - runs[-1][1] <= RUN_GAP:
            runs[-1][1] = i
        else:
            runs.append([i, i])
    index_of = {it.addr: i for i, it in enumerate(insts)}
    blocks = []
    for lo, hi in runs:
        spans = [(b, index_of[it.target]) for b, it in enumerate(insts)
                 if it.target is not None and it.op.startswith("s_cbranch_vcc") and it.target in index_of
                 and b < lo and index_of[it.target] > hi]
        assert spans, "a Philox run that no forward branch on VCC skips"
        blocks.append(min(spans, key=lambda s: s[1] - s[0]))
    return blocks


def test_every_argument_load_is_in_the_prologue_or_in_a_sampler_block(row_kernels):
    for name, insts in sorted(row_kernels.items()):
        ctrl = first_controller(insts)
        blocks = sampler_blocks(insts)
        loads = [i for i, it in enumerate(insts) if it.op.startswith("s_load_")]
        assert loads and loads[0] < ctrl
        # the two calls of reset_group (the reset of an ended env, the draw ahead), each a small part of the kernel behind the loop
        assert len(blocks) == 2 and all(ctrl < b < e and e - b < len(insts) // 4 for b, e in blocks), (name, blocks, len(insts))
        stray = [insts[i] for i in loads if i > ctrl and not any(b < i < e for b, e in blocks)]
        assert not stray, f"{name}: {len(stray)} argument loads behind the first controller and outside the sampler, e.g. {stray[0]!r}"
        # what the common path reads there instead
        assert sum(1 for it in insts[ctrl:] if it.op == "v_readlane_b32") >= 20, name


def test_headline_kernel_load_count(row_kernels):
    insts = row_kernels[HEADLINE]
    ctrl, blocks = first_controller(insts), sampler_blocks(insts)
    loads = [i for i, it in enumerate(insts) if it.op.startswith("s_load_")]
    before = sum(1 for i in loads if i < ctrl)
    sampler = sum(1 for i in loads if any(b < i < e for b, e in blocks))
    print(f"headline row kernel: {len(loads)} s_load instructions ({before} before the first controller, {sampler} in the sampler "
          f"blocks); parent build: {PARENT_HEADLINE_S_LOADS}")
    assert before + sampler == len(loads) < PARENT_HEADLINE_S_LOADS
