"""The case table of tests/test_gpu_disturb_forms.py (disturb_cases.py FORM_CASES) covers the pose disturbance's shipped kernels:
every disturb_step_kernel<SCN, GW, ROLLOUT, GYM, QPM> in the library has its (SCN, GW, QPM) in the table, every triple of the
table has its kernels, and every case runs all three launch kinds.  Mangled names only."""
import os
import re
import sys

import pytest

from disturb_cases import FORM_CASES, LAUNCH_KINDS, group_width, n_agents_of, triple

from marbler_amd.params import load_config, make_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND_OF = {("0", "0"): "step", ("1", "0"): "rollout", ("0", "1"): "gymma"}        # (ROLLOUT, GYM)


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


def test_the_table_holds_22_distinct_triples_in_all_three_launch_kinds():
    triples = [triple(c) for c in FORM_CASES]
    assert len(triples) == len(set(triples)) == 22
    assert sum(1 for t in triples if t[2] == 0) == 13 and sum(1 for t in triples if t[2] == 1) == 9
    assert all(gw in (4, 8) for _, gw, qpm in triples if qpm == 1)
    assert all(tuple(c[4]) == LAUNCH_KINDS == ("step", "rollout", "gymma") for c in FORM_CASES)
    assert len({c[0] for c in FORM_CASES}) == len(FORM_CASES)


@pytest.mark.parametrize("case", FORM_CASES, ids=[c[0] for c in FORM_CASES])
def test_the_parameter_builder_admits_the_case_at_the_width_it_declares(case):
    _, scenario, ov, solver, _ = case
    params = make_params(scenario, load_config(scenario, overrides=dict(ov, barrier_solver=solver, pose_noise_xy=0.01)))
    assert int(params.n_agents) == n_agents_of(scenario, ov) and int(params.qp_mode) == triple(case)[2]
    assert group_width(int(params.n_agents)) == triple(case)[1]


def test_the_table_covers_the_shipped_kernels(shipped):
    launched = {}
    for k in shipped:
        if "disturb_step_kernel" not in k:
            continue
        m = re.fullmatch(r"_ZN2rg19disturb_step_kernelILi(\d)ELi(\d+)ELb(\d)ELb(\d)ELi(\d)EEEvNS_11DisturbArgsE", k)
        assert m, k
        launched.setdefault((int(m.group(1)), int(m.group(2)), int(m.group(5))), set()).add(KIND_OF[(m.group(3), m.group(4))])
    table = {triple(c): set(c[4]) for c in FORM_CASES}
    assert sum(len(v) for v in launched.values()) == 66
    assert set(launched) - set(table) == set(), "shipped kernels no case launches"
    assert set(table) - set(launched) == set(), "cases without a kernel"
    assert all(launched[t] == table[t] for t in table), {t: (launched[t], table[t]) for t in table if launched[t] != table[t]}
