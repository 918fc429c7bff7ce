"""Every lane-group kernel family with several envs sharing a wavefront.

`wave_fill` (csrc/launch_plan.h) gives a batch of up to 1024 envs one env per wave; a wave carries 2, 4, 8 or 16 envs only above
1024 / 2048 / 4096 / 8192 envs (by group width), and only then can one env's lanes disturb another's: DPP and ballots confined to
`gbase`, LDS rows indexed by `g`, the interior-point workspace `qp->ws[lane / GW]`, `team_index[e]` and `elapsed[e]` fetched per
env, one env's lanes masked while its neighbours still iterate.  tests/test_gpu_baseline_shapes.py holds the plain family's exact
mode at groups of 8 to the oracle at those widths; the cases here do the same for the interior-point mode, groups of 16 and of 4,
the team and lidar families, the gymma block and rg_get_obs, each through the helper of the file that tests the family at one env
per wave.

Sizing: E is the smallest batch that reaches the width (1025 -> 2 slots, 2049 -> 4, 4097 -> 8, 8193 -> 16 at 4 lanes per env), so
the last wave is ragged; envs [c * slots, (c + 1) * slots) share wave c.  Episodes are 8 steps long so that every env auto-resets
inside a short run.  Every case forces RG_STEP_KERNEL=group and asserts the width it is named for with `expected_slots`.
"""
import os

import pytest
import torch

import lidar_harness as lidar
import team_harness as teams
from gpu_helpers import expected_slots, fused_time_limit_vs_composed, lane_group_kernel, random_actions  # noqa: F401  (the fixture)
from physical_cases import MT6, PCP5, PCP12, WH8
from rollout_harness import shape_rollout_vs_oracle

pytestmark = pytest.mark.gpu

EP = {"max_episode_steps": 8}
IPM = {"barrier_solver": "cvxopt"}
SIMPLE12 = {"n_agents": 12, "start_dist": 0.2}
MT10 = {"n_agents": 10, "n_fast_agents": 5, "n_slow_agents": 5, "start_dist": 0.25, "capability_aware": True}


# ---------------------------------------------------------------- 1. bit-exact against the float32 oracle
# (id, scenario, overrides, action count, envs, steps, env slots per wave).  With the helper's seeds the oracle alone produces,
# per case: episode ends / violations / QP iteration (interior-point) or sweep (exact) counts --
#   4098 / 87 / 5..18, 4102 / 94 / 5..17, 1204 / 215 / 10..17, 1105 / 95 / 6..18, 2091 / 53 / 4..49, 8193 / 108 / 4..46,
#   4117 / 511 / 1..40, 2357 / 800 / 1..40, 8194 / 127 / 1..12, 8337 / 196 / 1..12:
# the envs of one wave leave their solver at different times.
ORACLE_CASES = [
    ("ipm-pcp-2049x5", "PredatorCapturePrey", dict(PCP5, **IPM), 5, 2049, 20, 4),
    ("ipm-pcp-4097x5", "PredatorCapturePrey", dict(PCP5, **IPM), 5, 4097, 12, 8),
    ("ipm-wh-1025x8", "Warehouse", dict(WH8, **IPM), 5, 1025, 16, 2),
    ("ipm-mt-1025x6", "MaterialTransport", dict(MT6, **IPM), 20, 1025, 16, 2),
    ("ipm-pcp-2049x4", "PredatorCapturePrey", dict(IPM), 5, 2049, 16, 4),             # 4 lanes per env: the rows in registers
    ("ipm-pcp-8193x4", "PredatorCapturePrey", dict(IPM), 5, 8193, 10, 16),
    ("gw16-pcp-2049x12", "PredatorCapturePrey", PCP12, 5, 2049, 20, 4),               # 16 lanes per env: 4 slots = a full wave
    ("gw16-simple-1025x12", "Simple", SIMPLE12, 5, 1025, 20, 2),
    ("gw4-pcp-4097x4", "PredatorCapturePrey", {}, 5, 4097, 20, 8),
    ("gw4-mt-8193x4", "MaterialTransport", {}, 20, 8193, 16, 16),
]


@pytest.mark.parametrize("name,scenario,ov,n_act,E,steps,slots", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_rollout_is_bit_exact_vs_oracle(name, scenario, ov, n_act, E, steps, slots, oracle_lib):
    """Every output and state word of every step, then the same actions through rg_rollout."""
    shape_rollout_vs_oracle(name, scenario, dict(ov, **EP), n_act, E, steps, slots, oracle_lib)


# ---------------------------------------------------------------- 2. team pool: different sets inside one wave
TEAM_CASES = [
    ("team-pcp-2049x5", "PredatorCapturePrey", PCP5, "exact", 2049, 4),               # the NT = 5 team kernel
    ("team-ipm-wh-2049x8", "Warehouse", WH8, "cvxopt", 2049, 4),
    ("team-ipm-pcp-2049x4", "PredatorCapturePrey", {"predator": 2, "capture": 2, "n_agents": 4}, "cvxopt", 2049, 4),
    ("team-mt-1025x10", "MaterialTransport", MT10, "exact", 1025, 2),                 # 16 lanes per env
]


@pytest.mark.parametrize("name,scenario,ov,solver,E,slots", TEAM_CASES, ids=[c[0] for c in TEAM_CASES])
def test_mixed_teams_inside_a_wave_are_bit_exact_vs_oracle(name, scenario, ov, solver, E, slots, oracle_lib):
    assert expected_slots(int(ov["n_agents"]), E) == slots, "the case no longer exercises the dispatch width it is named for"

    def waves_hold_mixed_teams(env):
        assert env.step_kernel == "group"
        team = env.team_index.cpu().numpy()
        blocks = team[:E // slots * slots].reshape(-1, slots)
        mixed = int((blocks != blocks[:, :1]).any(axis=1).sum())
        assert 2 * mixed > len(blocks), (mixed, len(blocks))   # (4 uniform sets: a block of 4 is uniform with probability 1 / 64)

    teams.mixed_teams_vs_oracle(scenario, ov, solver, oracle_lib, E, 20, EP["max_episode_steps"],
                                before_first_step=waves_hold_mixed_teams, threads=max(1, min(16, os.cpu_count() or 1)))


# ---------------------------------------------------------------- 3. lidar
PAIR_CASES = [
    ("lidar-pcp-2049x5", "PredatorCapturePrey", PCP5, "exact", 2049, 4),
    ("lidar-ipm-pcp-2049x5", "PredatorCapturePrey", PCP5, "cvxopt", 2049, 4),
    ("lidar-simple-1025x12", "Simple", SIMPLE12, "exact", 1025, 2),
]


@pytest.mark.parametrize("name,scenario,ov,solver,E,slots", PAIR_CASES, ids=[c[0] for c in PAIR_CASES])
def test_lidar_changes_nothing_else(name, scenario, ov, solver, E, slots):
    assert expected_slots(int(ov["n_agents"]), E) == slots, "the case no longer exercises the dispatch width it is named for"
    lidar.lidar_changes_nothing_else(scenario, dict(ov, **EP), solver, T=12, E=E)


TWIN_CASES = [
    ("twin-pcp-2049x5-r16", "PredatorCapturePrey", PCP5, 2049, 16, 4),
    ("twin-wh-1025x8-r32", "Warehouse", WH8, 1025, 32, 2),
    ("twin-simple-2049x12-r8", "Simple", SIMPLE12, 2049, 8, 4),
]


@pytest.mark.parametrize("name,scenario,ov,E,R,slots", TWIN_CASES, ids=[c[0] for c in TWIN_CASES])
def test_lidar_ranges_match_the_float64_twin(name, scenario, ov, E, R, slots):
    """Random headings, two steps; tolerance and degenerate cap are `_check_against_twin`'s own (2e-5, 1e-3)."""
    assert expected_slots(int(ov["n_agents"]), E) == slots, "the case no longer exercises the dispatch width it is named for"
    lidar.ranges_vs_twin(scenario, R, E=E, T=2, ov=ov)


# ---------------------------------------------------------------- 4. the gymma block and rg_get_obs
GYMMA_CASES = [
    ("gymma-pcp-2049x5", "robotarium_gym:PredatorCapturePrey-v0", PCP5, 5, 9),
    ("gymma-wh-2049x8", "robotarium_gym:Warehouse-v0", WH8, 5, 6),
    ("gymma-mt-2049x4", "robotarium_gym:MaterialTransport-v0", {}, 20, 7),
]


@pytest.mark.parametrize("name,key,ov,n_act,limit", GYMMA_CASES, ids=[c[0] for c in GYMMA_CASES])
def test_fused_time_limit_equals_the_composed_gymma_step(name, key, ov, n_act, limit):
    """`elapsed[e]` and the reductions of the gymma block's own kernels, 4 envs per wave, through truncations and resets."""
    E = 2049
    assert expected_slots(int(ov.get("n_agents", 4)), E) == 4, "the case no longer exercises the dispatch width it is named for"
    fused_time_limit_vs_composed(key, ov, n_act, limit, E, 24)


@pytest.mark.parametrize("family", ["plain", "lidar", "team"])
def test_get_obs_returns_the_observation_of_the_step(family):
    """rg_get_obs (the OBS_ONLY kernels) after one step without auto-reset: word for word what the step returned."""
    E = 2049
    assert expected_slots(5, E) == 4
    if family == "lidar":
        env = lidar.make_env("PredatorCapturePrey", E, 16, seed=4, auto_reset=False)
    else:
        env = teams.make_env("PredatorCapturePrey", E, teams=teams.pool4("PredatorCapturePrey", 5) if family == "team" else None,
                         seed=4, auto_reset=False)
    assert env.N == 5 and env.step_kernel == "group"
    assert (env.lidar is not None and env.lidar.rays == 16) == (family == "lidar") and (env.teams is not None) == (family == "team")
    env.reset()
    acts = random_actions(env, 1, seed=6)
    stepped = env.step(acts[0])[0].clone()
    again = env.get_obs(torch.full_like(stepped, float("nan")))
    torch.cuda.synchronize()
    assert torch.equal(again.view(torch.int32), stepped.view(torch.int32))
    assert stepped.abs().sum() > 0
    env.close()
