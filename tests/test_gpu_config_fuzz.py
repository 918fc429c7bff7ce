"""Randomised configurations: scenario x agent count x neighbour slots x prey count x certificate x collision test x
penalties x controller cadence x batch size x step kernel, drawn from a seeded generator inside the ranges the parameter
block admits, each stepped free-running with auto-reset against the float32 oracle, bit for bit (tests/rollout_harness.py;
the generators are tests/fuzz_cases.py).  The hand-picked cases cover the reference's configurations; this covers the combinations nobody
picked -- round 3 found by code review that rows wider than the agents fill overran the thread-per-env kernel's staging
block, a shape no listed case had."""
import numpy as np
import pytest

from fuzz_cases import draw_barrier_family, draw_config, draw_interior_point
from rollout_harness import fuzz_case_bit_exact, rollout_equals_steps

pytestmark = pytest.mark.gpu


CASES = [draw_config(np.random.RandomState(1000 + i)) for i in range(320)]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_random_configuration_is_bit_exact(i, oracle_lib, monkeypatch):
    monkeypatch.setenv("RG_STEP_KERNEL", CASES[i][4])       # (configurations the thread-per-env kernel does not cover run the lane-group one)
    fuzz_case_bit_exact(i, CASES[i], (25, 40), oracle_lib)


@pytest.mark.parametrize("i", range(0, len(CASES), 4))
def test_random_configuration_multi_step_launch_equals_single_steps(i, monkeypatch):
    """The same draws through rg_rollout (K steps per launch) against K rg_step launches (GPU against GPU, every output and
    the final state)."""
    scenario, ov, n_act, E, kernel = CASES[i]     # (round 4: shapes whose E*N*D is not a multiple of 4 run too; rg_rollout takes them)
    monkeypatch.setenv("RG_STEP_KERNEL", kernel)
    rollout_equals_steps(scenario, ov, n_act, E, K=12, reps=3, require_done=False)


BARRIER_CASES = [draw_barrier_family(np.random.RandomState(5000 + i)) for i in range(48)]


@pytest.mark.parametrize("i", range(len(BARRIER_CASES)))
def test_random_barrier_family_is_bit_exact(i, oracle_lib, monkeypatch):
    monkeypatch.setenv("RG_STEP_KERNEL", BARRIER_CASES[i][4])
    fuzz_case_bit_exact(i, BARRIER_CASES[i], (25, 40), oracle_lib)


IPM_CASES = [draw_interior_point(np.random.RandomState(7000 + i)) for i in range(64)]


@pytest.mark.parametrize("i", range(len(IPM_CASES)))
def test_random_interior_point_configuration_is_bit_exact(i, oracle_lib, monkeypatch):
    monkeypatch.setenv("RG_STEP_KERNEL", IPM_CASES[i][4])
    fuzz_case_bit_exact(i, IPM_CASES[i], (16, 30), oracle_lib)
