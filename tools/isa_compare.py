"""Two builds of the library, kernel by kernel (tools/isa_scan.py on the code objects of each):

    python tools/isa_compare.py parent.so new.so [--rows MARK] > profiles/<name>.txt

* every kernel whose name lacks MARK (default "ELb0ELi16E": the 16-lane-row step kernels) must be instruction-identical in the
  two libraries -- same opcodes, same operands, in the same order; the exit status is 1 if one is not, or exists in one only;
* for the kernels that carry MARK: instruction count, resource record and the three shapes in which a lane predicate goes
  through a vector register (v_bitop3_b16, compares on u16, v_cndmask_b32 v, 0, 1, mask), before and after.
"""
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_scan  # noqa: E402

ZERO_ONE = re.compile(r"^v\d+, 0, 1,")


def load(lib):
    """-> {kernel: ([(op, args)], resources)}"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in isa_scan.extract_code_objects(lib, d):
            res = isa_scan.resources(co)
            for name, insts in isa_scan.disassemble(co).items():
                out[name] = ([(it.op, it.args) for it in insts], res.get(name, {}))
    return out


def patterns(code):
    return (sum(1 for op, _ in code if op.startswith("v_bitop3_b16")),
            sum(1 for op, _ in code if op.startswith("v_cmp") and "_u16" in op),
            sum(1 for op, a in code if op.startswith("v_cndmask_b32") and ZERO_ONE.match(a)))


def main(argv):
    mark = argv[argv.index("--rows") + 1] if "--rows" in argv else "ELb0ELi16E"
    old, new = load(argv[1]), load(argv[2])
    others = sorted(k for k in set(old) | set(new) if mark not in k)
    changed = [k for k in others if k not in old or k not in new or old[k][0] != new[k][0]]
    print(f"parent {os.path.basename(argv[1])}: {len(old)} functions; new {os.path.basename(argv[2])}: {len(new)} functions")
    print(f"{len(others)} functions without `{mark}` in the name: {len(others) - len(changed)} instruction-identical, {len(changed)} not")
    for k in changed:
        print(f"  DIFFERS: {k}")
    print(f"\nkernels with `{mark}` (instructions; vgpr / sgpr / scratch / spill / occupancy; v_bitop3_b16, u16 compares, v_cndmask 0, 1):")
    tot = [0] * 8
    for k in sorted(k for k in set(old) | set(new) if mark in k):
        row = []
        for side in (old, new):
            code, r = side.get(k, ([], {}))
            row.append((len(code), r, patterns(code)))
        (n0, r0, p0), (n1, r1, p1) = row
        for i, v in enumerate((n0, *p0, n1, *p1)):
            tot[i] += v

        def rec(r):
            return "/".join(str(r.get(f, "-")) for f in ("vgpr", "sgpr", "scratch", "spill", "occupancy"))
        print(f"  {k}\n      parent {n0:6d}  {rec(r0):>18}  {p0[0]:3d} {p0[1]:3d} {p0[2]:3d}\n      new    {n1:6d}  {rec(r1):>18}  {p1[0]:3d} {p1[1]:3d} {p1[2]:3d}")
    print(f"\nall of them: parent {tot[0]} instructions, {tot[1]} / {tot[2]} / {tot[3]}; new {tot[4]} instructions, {tot[5]} / {tot[6]} / {tot[7]}")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
