"""The step kernels against the float32 oracle OFF the default physical constants.

Every other GPU test runs at one point of the 13 rps constants of rg_scenario_params (time step, arena, robot geometry, velocity
limits, collision test, unicycle map: include/robogym.h); the kernels branch on them.  Here they vary -- the tables are in
tests/physical_cases.py, and tests/test_physical_regimes.py shows on the CPU that each directed case reaches the code it is named
for:

 (a) directed regimes x every dispatch of the step (lane groups of 4, 8, 16; the 16-lane rows by value, resident and shaped;
     the thread-per-env kernel; both QP modes where built), free-running with auto-reset: what tests/oracle_check.py
     compares for a free-running harness (rollout_harness.rollout_bit_exact);
 (b) a seeded fuzz over all 13 constants on top of fuzz_cases.draw_config;
 (c) the lidar, team-pool and pose-disturbance families at one off-default point each;
 (d) stray poses: colliding pairs loaded far outside the arena, where the collision pre-test's binary16 figure is no bound, and
     a colliding pair inside the large arena that a rounding bound sized for the default arena would miss.
"""
import ctypes as C

import numpy as np
import pytest

import disturb_harness
import lidar_harness
import physical_cases as pc
import team_harness
from helpers import gpu_from_state
from oracle_check import FreeRunningOracle, assert_outputs, assert_state, gpu_outputs, gpu_state
from physical_cases import CASES, IPM_CASES
from rollout_harness import fuzz_case_bit_exact, rollout_bit_exact, rollout_equals_steps

pytestmark = pytest.mark.gpu

ROW_VARS = ("RG_STEP_SHAPE", "RG_STEP_SPAN", "RG_STEP_RESIDENT")


def _dispatch_env(monkeypatch, kernel, env_vars=()):
    for k in ROW_VARS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RG_STEP_KERNEL", kernel)
    for k, v in dict(env_vars).items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------- (a) directed regimes x dispatches
@pytest.mark.parametrize("dispatch", pc.DISPATCHES, ids=pc.DISPATCH_IDS)
@pytest.mark.parametrize("regime", pc.REGIMES, ids=pc.REGIME_IDS)
def test_regime_is_bit_exact_on_every_dispatch(regime, dispatch, oracle_lib, monkeypatch):
    from marbler_amd import _lib
    name, scenario, _, kernel, env_vars, E, _, form, _ = dispatch
    ov, consts = pc.case_overrides(regime, dispatch)
    _dispatch_env(monkeypatch, kernel, env_vars)

    def launched_as_named(env, t):
        assert env.step_kernel == kernel
        if form is None:
            return
        got = env.step_form
        if form == "shape":
            sid = _lib.load().rg_shape_match(C.byref(env.params))
            assert sid > 0 and got == _lib.FORM_SHAPE + sid, (t, got, sid)   # other constants, the same shape: match_shape ignores them
        else:
            assert got == {"by-value": _lib.FORM_BY_VALUE, "resident": _lib.FORM_RESIDENT}[form], (t, got)

    rollout_bit_exact(scenario, ov, pc.N_ACT.get(scenario, 5), pc.STEPS, oracle_lib, E, constants=consts, after_step=launched_as_named)


# ---------------------------------------------------------------- (b) the seeded fuzz
@pytest.mark.parametrize("i", range(len(CASES)))
def test_random_constants_are_bit_exact(i, oracle_lib, monkeypatch):
    _dispatch_env(monkeypatch, CASES[i][4])
    fuzz_case_bit_exact(i, CASES[i], (25, 40), oracle_lib, constants={k: CASES[i][1][k] for k in pc.RPS_DEFAULTS})


@pytest.mark.parametrize("i", range(len(IPM_CASES)))
def test_random_constants_are_bit_exact_in_the_interior_point_mode(i, oracle_lib, monkeypatch):
    _dispatch_env(monkeypatch, IPM_CASES[i][4])
    fuzz_case_bit_exact(i, IPM_CASES[i], (16, 30), oracle_lib, constants={k: IPM_CASES[i][1][k] for k in pc.RPS_DEFAULTS})


@pytest.mark.parametrize("i", range(0, len(CASES), 4))
def test_random_constants_multi_step_launch_equals_single_steps(i, monkeypatch):
    scenario, ov, n_act, E, kernel = CASES[i]
    _dispatch_env(monkeypatch, kernel)
    rollout_equals_steps(scenario, ov, n_act, E, K=12, reps=2, require_done=False)


# ---------------------------------------------------------------- (c) the opt-in families
WIDE = dict(time_step=0.1, update_frequency=5)
OFF_CENTRE = pc.arena(-1.6, -1.0, 4.8, 2.5)


@pytest.fixture
def _group(monkeypatch):
    _dispatch_env(monkeypatch, "group")


def test_lidar_with_a_wide_robot_in_the_off_centre_arena(_group):
    """tests/lidar_twin.py reads the arena from the parameter block; the robots' radius follows robot_diameter."""
    lidar_harness.ranges_vs_twin("PredatorCapturePrey", 16, E=65, T=4, ov=dict(OFF_CENTRE, robot_diameter=0.15))


@pytest.mark.parametrize("solver", ["exact", "cvxopt"])
def test_team_pool_through_the_wide_angle_heading_step(solver, oracle_lib, _group):
    team_harness.mixed_teams_vs_oracle("PredatorCapturePrey", dict(pc.PCP5, **WIDE), solver, oracle_lib, 65, 30, 10)


@pytest.mark.parametrize("solver", ["exact", "cvxopt"])
def test_pose_disturbance_at_its_bounds_with_a_long_time_step(solver, oracle_lib, _group):
    disturb_harness.disturbed_vs_oracle("PredatorCapturePrey", dict(pc.PCP5, **WIDE), solver, 67, 12, oracle_lib, sigma=(0.1, 0.5))


# ---------------------------------------------------------------- (d) stray poses
def _oracle_with_reset_states(oracle_lib, scenario, cfg, E):
    from marbler_amd.params import make_params
    return FreeRunningOracle.at_reset(oracle_lib, scenario, cfg, E, make_params(scenario, cfg), pc.SEED)


def _one_step_from_loaded_state(scenario, cfg, orc, expected):
    """The oracle steps first and must report `expected` (None: whatever it reports) in every env: a placement error cannot pass
    as agreement.  Then the same state and the no-op action on the GPU: every output and the stored state (tests/oracle_check.py)."""
    import torch
    state = orc.get_state(slice(None))
    acts = np.full((orc.E, orc.N), pc.NO_OP, np.int32)
    o_info = orc.step(acts)[3]
    codes = set(o_info["violation"].tolist())
    if expected is not None:
        assert codes == {expected}, codes
    assert len(codes) == 1
    env = gpu_from_state(scenario, cfg, state)
    env.step(torch.as_tensor(acts, device=env.device))
    torch.cuda.synchronize()
    got_viol = env.violation.cpu().numpy()
    assert np.array_equal(got_viol, o_info["violation"]), \
        f"violation: {np.bincount(got_viol, minlength=4).tolist()} (codes 0..3) on the GPU, the oracle reports {sorted(codes)} in all {orc.E} envs"
    assert_outputs(gpu_outputs(env), orc, scenario)
    assert_state(gpu_state(env), orc, label=scenario)
    env.close()
    return codes.pop()


@pytest.mark.parametrize("pose", pc.STRAY_POSES, ids=[p[0] for p in pc.STRAY_POSES])
@pytest.mark.parametrize("n_agents", sorted(pc.STRAY_TEAMS))
def test_stray_poses_are_judged_like_the_oracle_judges_them(n_agents, pose, step_kernel, oracle_lib):
    """Default constants, penalize_violations on.  The oracle reports 3 (collision and boundary) for the four far pairs, and for
    the pair across the wall x = 1.6 m as well: the robot beyond the wall is outside, the pair 1 mm inside the collision distance."""
    from marbler_amd.params import load_config
    pose_id, _, expected = pose
    scenario = "PredatorCapturePrey"
    cfg = load_config(scenario, overrides=dict(pc.STRAY_TEAMS[n_agents], penalize_violations=True))
    orc = _oracle_with_reset_states(oracle_lib, scenario, cfg, pc.STRAY_E)
    orc.poses[...] = pc.stray_poses(orc.poses, pose_id)
    code = _one_step_from_loaded_state(scenario, cfg, orc, expected)
    assert code == 3


@pytest.mark.parametrize("dispatch", ["gw4", "rows-resident", "rows-shape-pcp", "gw8-no-rows", "gw16", "tpe"])
def test_a_colliding_pair_inside_the_large_arena_is_seen(dispatch, oracle_lib, monkeypatch):
    """Both robots inside the arena at |x|, |y| in [4, 8) m: only a rounding bound computed for THIS arena (pre_margin) sees
    them.  The oracle reports a collision alone."""
    from marbler_amd.params import load_config
    d = next(x for x in pc.DISPATCHES if x[0] == dispatch)
    _, scenario, _, kernel, env_vars, _, _, _, _ = d
    ov, _ = pc.case_overrides(pc.LARGE_ARENA, d)
    _dispatch_env(monkeypatch, kernel, env_vars)
    cfg = load_config(scenario, overrides=dict(ov, penalize_violations=True))
    orc = _oracle_with_reset_states(oracle_lib, scenario, cfg, pc.STRAY_E)
    orc.poses[...] = pc.large_arena_poses(orc.poses)
    _one_step_from_loaded_state(scenario, cfg, orc, 1)
