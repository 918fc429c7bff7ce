"""The lane predicates of the 16-lane-row step kernels' sub-step loop in the SHIPPED library (CPU tier: tools/isa_scan.py on the
code objects of marbler_amd/librobogym_hip.so).

A row kernel is one wave per SIMD, and a lone wave pays for every instruction it executes.  The predicates of the sub-step loop --
`lane_ok & !dead`, `sparse_ok`, the pre-test's hit, the boundary flag -- are the same in every chunk of a controller period or of the
launch, so they are held as wave masks in scalar register pairs (csrc/device_common.h lane_mask; csrc/step_group.h step_once PM):
combined with s_and / s_or / s_andn2, voted on with a scalar compare, the operand of the v_cndmask that selects the ghost point.
Held as bools around the loops they reached every chunk as 0 / 1 integers in vector registers and were turned back into masks
there; the three shapes that conversion takes are what the rule below looks for.

The rule: in each kernel of the reference shapes, the COMMON PATH of the 5-sub-step chunk holds no `v_bitop3_b16`, no compare on
`u16` and no `v_cndmask_b32 v, 0, 1, mask`.  The path is recognised in the instruction stream as follows:
* the sparse collision pre-test is the kernel's first run of v_dot2_f32_f16 (the full chunk comes first in program order);
* the path begins at the chunk loop's header: the nearest label in front of that run which a LATER instruction branches back to;
* it ends with the first branch behind the run: the vote that skips the dense pre-test.
"""
import os
import re
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ZERO_ONE = re.compile(r"^v\d+, 0, 1,")


def converts_a_predicate(it):
    """One of the three shapes in which a predicate goes through a vector register."""
    return it.op.startswith("v_bitop3_b16") or (it.op.startswith("v_cmp") and "_u16" in it.op) or \
        (it.op.startswith("v_cndmask_b32") and ZERO_ONE.match(it.args) is not None)


@pytest.fixture(scope="module")
def shaped_kernels():
    import isa_scan
    from marbler_amd import build as hip_build
    assert os.path.exists(hip_build.LIB), "librobogym_hip.so is not built"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in isa_scan.extract_code_objects(hip_build.LIB, d):
            if not any("NS_5ShapeI" in k for k in isa_scan.resources(co)):
                continue   # (one code object per translation unit: only the one with the shapes' kernels is disassembled)
            out.update({k: v for k, v in isa_scan.disassemble(co).items() if "2rg11step_kernelILi" in k and "NS_5ShapeI" in k})
    return out


def common_path(insts):
    """-> (first, last) instruction indices of the 5-chunk's common path: the loop header .. the branch around the dense pre-test."""
    dot = next(i for i, it in enumerate(insts) if it.op.startswith("v_dot2_f32_f16"))
    back_targets = {it.target for i, it in enumerate(insts) if it.target is not None and it.target <= it.addr}
    head = next(i for i in range(dot, -1, -1) if insts[i].addr in back_targets)
    end = next(i for i in range(dot, len(insts)) if insts[i].op.startswith(("s_cbranch", "s_branch")))
    return head, end


def test_one_kernel_per_reference_shape(shaped_kernels):
    from test_shape_kernels import table
    assert len(shaped_kernels) == len(table()) == 3, sorted(shaped_kernels)


def test_the_common_path_of_the_full_chunk_converts_no_predicate(shaped_kernels):
    for name, insts in sorted(shaped_kernels.items()):
        head, end = common_path(insts)
        path = insts[head:end + 1]
        # it IS that path: straight-line code from the header, the pre-test's four or more pair rounds, a forward conditional branch
        assert not any(it.op.startswith(("s_cbranch", "s_branch")) for it in path[:-1]), name
        assert sum(1 for it in path if it.op.startswith("v_dot2_f32_f16")) >= 4, name
        assert path[-1].op.startswith("s_cbranch") and path[-1].target > path[-1].addr, (name, path[-1])
        assert 30 <= len(path) <= 80, (name, len(path))
        # the chunk's Euler steps and the ghost select are in it
        assert any(it.op.startswith("v_cvt_pkrtz_f16_f32") for it in path) and any(it.op.startswith("v_cndmask_b32") for it in path), name
        bad = [it for it in path if converts_a_predicate(it)]
        print(f"{name[:60]}...: common path of the 5-chunk {len(path)} instructions, {len(bad)} predicate conversions")
        assert not bad, f"{name}: the common path of the 5-chunk turns a predicate into a register or back, e.g. {bad[0]!r}"


def test_the_rule_sees_the_three_shapes():
    """The recogniser itself, on the instructions the parent build had in that path."""
    from isa_scan import Inst
    seen = [Inst(0, "v_bitop3_b16", "v58, v118, v19, v118 bitop3:0xc", None), Inst(4, "v_cmp_ne_u16_e32", "vcc, 0, v70", None),
            Inst(8, "v_cndmask_b32_e64", "v71, 0, 1, s[18:19]", None), Inst(12, "v_cmp_eq_u16_e64", "s[4:5], 0, v48", None)]
    fine = [Inst(0, "v_cndmask_b32_e64", "v62, v19, v62, s[22:23]", None), Inst(4, "v_cmp_le_i32_e32", "vcc, v84, v80", None),
            Inst(8, "v_cndmask_b32_e64", "v40, 0, v40, s[20:21]", None), Inst(12, "v_and_b32_e32", "v1, 1, v1", None)]
    assert all(converts_a_predicate(it) for it in seen) and not any(converts_a_predicate(it) for it in fine)
