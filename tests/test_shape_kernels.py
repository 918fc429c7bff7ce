"""The resident row kernels of the reference shapes in the SHIPPED library, and the matcher that chooses them (CPU tier).

A reference shape (csrc/kernel_args.h RG_REF_SHAPES) is a benchmark configuration whose members of the parameter block -- prey
count, observation width, neighbour count, the capability and penalty flags, the sub-step count and the controller period -- are
compile-time constants of a resident row kernel of its own (csrc/robogym_resident_shapes.hip).  The table is read from the library
(rg_shape_info), the kernels are looked up by the names that table implies, and they are held to the rules of the generic row
kernels (tests/test_row_kernel_args.py, tests/test_resident_kernels.py: helpers imported).

The matcher (rg_shape_match, host code) is driven through every reference configuration and, for each, through a perturbation
of every field its kernel holds as a constant and of the agent count: only the unperturbed block may match.
"""
import ctypes as C
import os
import sys
import tempfile

import pytest

from test_resident_kernels import PRELOAD_ENTRY, PRELOADED_DWORDS
from test_row_kernel_args import first_controller, sampler_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPED = "ELb0ELi16ELb1ENS_5ShapeI"
FIELDS = ("num_prey", "obs_dim", "num_neighbors", "capability_aware", "update_frequency", "controller_period", "penalize_violations")
SCENARIOS = {0: "PredatorCapturePrey", 1: "Warehouse", 2: "MaterialTransport"}

# (scenario, overrides): bench.py's bench_overrides() configurations, which the table must serve
REFERENCE = {
    "PredatorCapturePrey": {"predator": 3, "capture": 2, "n_agents": 5},
    "Warehouse": {"n_agents": 8},
    "MaterialTransport": {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25},
}
# what each scenario's row kernel reads of the seven fields (step_group.h): a shape may hold these as constants, no others
KERNEL_READS = {
    "PredatorCapturePrey": FIELDS,
    "Warehouse": ("obs_dim", "num_neighbors", "update_frequency", "controller_period", "penalize_violations"),
    "MaterialTransport": ("obs_dim", "capability_aware", "update_frequency", "controller_period", "penalize_violations"),
}
# field -> [config overrides that change it]; applied to the scenarios whose kernel reads the field
PERTURB = {
    "num_prey": [{"num_prey": 5}, {"num_prey": 9}],
    "num_neighbors": [{"num_neighbors": 2}],
    "capability_aware": [{"capability_aware": True}],
    "update_frequency": [{"update_frequency": 30}],
    "controller_period": [{"robotarium": True}],
    "penalize_violations": [{"penalize_violations": False}],
}
# the agent count off by one (both ways where the scenario's kernels exist)
OTHER_N = {
    "PredatorCapturePrey": [{"predator": 2, "capture": 2, "n_agents": 4}, {"predator": 3, "capture": 3, "n_agents": 6}],
    "Warehouse": [{"n_agents": 7}, {"n_agents": 9, "start_dist": 0.4}],
    "MaterialTransport": [{"n_agents": 5, "n_fast_agents": 3, "n_slow_agents": 2}, {"n_agents": 7, "n_fast_agents": 3, "n_slow_agents": 4, "start_dist": 0.2}],
}


def table():
    from marbler_amd import _lib
    rows = _lib.reference_shapes()
    assert rows, "the library has no reference shapes"
    return rows


def perturbed_cases():
    """[(id, scenario, overrides, changed field)]: every perturbation of every reference configuration.  (obs_dim follows from
    the neighbour count and the capability flag: it has no case of its own.  Built without the library: the GPU tier's
    parametrisation reads it too.)"""
    out = []
    for scenario in sorted(REFERENCE):
        base = REFERENCE[scenario]
        for field, changes in PERTURB.items():
            if field not in KERNEL_READS[scenario]:
                continue
            for ch in changes:
                out.append((f"{scenario}-{'-'.join(f'{k}={v}' for k, v in ch.items())}", scenario, dict(base, **ch), field))
        for ch in OTHER_N[scenario]:
            out.append((f"{scenario}-n{ch['n_agents']}", scenario, dict(base, **ch), "n_agents"))
    return out


def _params(scenario, overrides):
    from marbler_amd.params import load_config, make_params
    return make_params(scenario, load_config(scenario, overrides=overrides))


def _match(p):
    from marbler_amd import _lib
    return _lib.load().rg_shape_match(C.byref(p))


# ------------------------------------------------------------------ the table and the matcher
def test_the_table_holds_the_benchmark_configurations():
    rows = table()
    assert [r["id"] for r in rows] == list(range(1, len(rows) + 1))
    assert sorted(SCENARIOS[r["scenario"]] for r in rows) == sorted(REFERENCE)
    for row in rows:
        scenario = SCENARIOS[row["scenario"]]
        p = _params(scenario, REFERENCE[scenario])
        assert row["n_agents"] == p.n_agents, row
        for f in FIELDS:   # a compiled-in field holds the configuration's own value (the flags as zero / non-zero)
            have = int(getattr(p, f))
            if f in ("capability_aware", "penalize_violations"):
                have = int(have != 0)
            assert row[f] in (-1, have), (scenario, f, row[f], have)
            assert row[f] == -1 or f in KERNEL_READS[scenario], (scenario, f)
        assert _match(p) == row["id"], scenario


def test_every_perturbed_block_falls_to_the_generic_form():
    """Prey 5 and 9, neighbours 2, capability-aware, U 30, robotarium (period 1), penalties off, N off by one: a block that
    differs in a field its shape holds as a constant, or in the agent count, matches nothing.  (A field the table leaves to
    run time may differ: the block then still matches, and must.)"""
    rows = {SCENARIOS[r["scenario"]]: r for r in table()}
    cases = perturbed_cases()
    assert len(cases) >= 8 + 6 + 6
    compiled_in = 0
    for name, scenario, ov, field in cases:
        p, base, row = _params(scenario, ov), _params(scenario, REFERENCE[scenario]), rows[scenario]
        if field != "n_agents":
            assert getattr(p, field) != getattr(base, field), f"{name}: the override did not change {field}"
        changed = [f for f in FIELDS if getattr(p, f) != getattr(base, f) and row[f] >= 0]
        if changed or p.n_agents != base.n_agents:
            compiled_in += 1
            assert _match(p) == 0, f"{name}: matched a shape although {changed or 'n_agents'} differ"
        else:
            assert _match(p) == row["id"], f"{name}: {field} is a run-time value of the shape, the block must still match"
    assert compiled_in >= len(rows) * 3   # (the agent count both ways, and at least one field per shape)


def test_a_flag_matches_by_truth_value_and_a_count_by_value():
    """The kernels read the two flags as zero / non-zero; every other field must be the very number."""
    p = _params("PredatorCapturePrey", REFERENCE["PredatorCapturePrey"])
    sid = _match(p)
    assert sid >= 1
    p.penalize_violations = 7
    assert _match(p) == sid
    p.penalize_violations = 0
    assert _match(p) == 0
    p.penalize_violations = 1
    p.obs_dim += 4   # (a wider row than the scenario's own columns: a lidar handle's, for one)
    assert _match(p) == 0


# ------------------------------------------------------------------ the kernels
@pytest.fixture(scope="module")
def library():
    import isa_scan
    from marbler_amd import build as hip_build
    assert os.path.exists(hip_build.LIB), "librobogym_hip.so is not built"
    insts, res, preload, generic = {}, {}, {}, {}
    with tempfile.TemporaryDirectory() as d:
        for co in isa_scan.extract_code_objects(hip_build.LIB, d):
            r = isa_scan.resources(co)
            if any(SHAPED in k for k in r):
                res.update({k: v for k, v in r.items() if SHAPED in k})
                preload.update({k: v for k, v in isa_scan.kernarg_preload(co).items() if SHAPED in k})
                insts.update({k: v for k, v in isa_scan.disassemble(co).items() if SHAPED in k})
            elif any("ELb0ELi16ELb1ET" in k for k in r):   # the generic resident kernels: the sizes to compare with
                generic.update({k: len(v) for k, v in isa_scan.disassemble(co).items() if "ELb0ELi16ELb1ET" in k})
    return insts, res, preload, generic


def _kernel_stem(row):
    def lit(v):
        return f"Lin{-v}E" if v < 0 else f"Li{v}E"
    shape = "NS_5ShapeI" + "".join(lit(row[f]) for f in FIELDS) + "EE"
    return f"_ZN2rg11step_kernelILi{row['scenario']}ELi8ELb0ELi{row['n_agents']}ELb0ELi16ELb1E{shape}"


def test_one_kernel_per_row_of_the_table(library):
    insts, res, _, _ = library
    rows = table()
    assert len(insts) == len(res) == len(rows), sorted(res)
    for row in rows:
        assert sum(1 for k in insts if k.startswith(_kernel_stem(row))) == 1, (_kernel_stem(row), sorted(insts))


def test_shape_kernels_keep_the_resident_kernels_rules(library):
    import isa_scan
    insts, res, preload, generic = library
    for name, code in sorted(insts.items()):
        r = res[name]
        assert r["spill"] == 0 and r["scratch"] == 0 and r["occupancy"] >= 3, (name, r)
        assert preload[name] == (PRELOADED_DWORDS, 0), (name, preload[name])
        n_dots, hazards = isa_scan.dot_hazards(code)
        assert n_dots > 0 and not hazards and not isa_scan.exec_prologue(code), (name, hazards, isa_scan.exec_prologue(code))
        # the first vector load is issued before anything waits for scalar memory
        entry = next(i for i, it in enumerate(code) if it.addr == code[0].addr + PRELOAD_ENTRY)
        assert any(it.op == "s_branch" and it.target == code[entry].addr for it in code[:entry]), name
        first_load = next(i for i in range(entry, len(code)) if code[i].op.startswith("global_load"))
        assert not [it for it in code[entry:first_load] if it.op == "s_waitcnt" and "lgkmcnt" in it.args], name
        assert not any(it.op.startswith("s_load") for it in code[entry:first_load]), name
        # argument loads only before the first controller or inside a sampler block
        ctrl, blocks = first_controller(code), sampler_blocks(code)
        loads = [i for i, it in enumerate(code) if it.op.startswith("s_load_")]
        assert loads and loads[0] < ctrl
        assert len(blocks) == 2 and all(ctrl < b < e and e - b < len(code) // 4 for b, e in blocks), (name, blocks, len(code))
        stray = [code[i] for i in loads if i > ctrl and not any(b < i < e for b, e in blocks)]
        assert not stray, f"{name}: {len(stray)} argument loads behind the first controller and outside the sampler, e.g. {stray[0]!r}"
        assert sum(1 for it in code[ctrl:] if it.op == "v_readlane_b32") >= 20, name
        assert not any(it.op.startswith("flat_") for it in code), name
        # and the point of it: less code than the generic kernel of the same scenario and agent count
        twin = [n for k, n in generic.items() if k.startswith(name[:name.index("ELb1E") + 5])]
        assert len(twin) == 1 and len(code) < twin[0], (name, len(code), twin)
