"""The team pool on the GPU (DESIGN.md "Team pool"): non-interference with a one-set pool of the config's own values, mixed teams
against the float32 oracle loaded with each env's set (tests/team_harness.py; what is compared: tests/oracle_check.py), the index draw against its NumPy twin (tests/team_twin.py) on
every reset path, its frequencies, the fixed mode and sharding, bit identity across the paths that step a pooled env, snapshots,
BatchedRunner, and guard slabs around the pool's arrays."""
import numpy as np
import pytest
import torch

from gpu_helpers import (guarded_class, random_actions as _actions, random_actor, rollout_equals_single_steps, runner_batch_replays,
                         same_bits as _same)
from team_harness import SCN_OV, make_env as _env, mixed_teams_vs_oracle, pool4 as _pool4
from team_twin import expected_after_reset

pytestmark = pytest.mark.gpu

SOLVERS = ("exact", "cvxopt")
OUT_KEYS = ("obs", "reward", "done_u8", "dist_travelled", "violation", "remaining")


# ---------------------------------------------------------------- 1. non-interference
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("scenario", list(SCN_OV))
def test_one_set_of_the_configs_own_values_changes_nothing(scenario, solver):
    """A pool whose only set leaves every capability to the config (= the config's own values): every output and every state
    array bit-identical to the same handle without a pool, over 60 auto-reset steps."""
    E, T = 96, 60
    ov = {"barrier_solver": solver, "max_episode_steps": 12}
    ref = _env(scenario, E, ov, seed=5)
    pooled = _env(scenario, E, ov, teams=[{}], seed=5)
    assert pooled.step_kernel == "group" and pooled.teams.n_sets == 1
    ref.reset()
    pooled.reset()
    acts = _actions(ref, T, seed=1)
    n_done = 0
    for t in range(T):
        ref.step(acts[t])
        pooled.step(acts[t])
        n_done += int(ref.done.sum())
        for k in OUT_KEYS:
            assert _same(getattr(ref, k), getattr(pooled, k)), (t, k)
        for k in ref.STATE_KEYS:
            assert _same(getattr(ref, k), getattr(pooled, k)), (t, k)
    assert n_done > 0
    assert int(pooled.team_index.abs().sum()) == 0


# ---------------------------------------------------------------- 2. mixed teams against the float32 oracle
ORACLE_CASES = [("PredatorCapturePrey", {"predator": 2, "capture": 2, "n_agents": 4}, "exact"),                        # GW 4
                ("PredatorCapturePrey", {"predator": 3, "capture": 2, "n_agents": 5}, "exact"),                        # GW 8, NT 5
                ("PredatorCapturePrey", {"predator": 3, "capture": 2, "n_agents": 5, "capability_aware": True}, "exact"),
                ("PredatorCapturePrey", {"predator": 5, "capture": 5, "n_agents": 10, "start_dist": 0.25, "num_neighbors": 4,
                                         "capability_aware": True}, "exact"),                                          # GW 16
                ("PredatorCapturePrey", {"predator": 3, "capture": 2, "n_agents": 5, "capability_aware": True}, "cvxopt"),
                ("PredatorCapturePrey", {"predator": 2, "capture": 2, "n_agents": 4}, "cvxopt"),
                ("MaterialTransport", {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25}, "exact"),
                ("MaterialTransport", {"n_agents": 4, "n_fast_agents": 2, "n_slow_agents": 2, "capability_aware": True}, "exact"),
                ("MaterialTransport", {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25,
                                       "capability_aware": True}, "cvxopt"),
                ("MaterialTransport", {"n_agents": 10, "n_fast_agents": 5, "n_slow_agents": 5, "start_dist": 0.25,
                                       "capability_aware": True}, "exact"),                                            # GW 16
                ("Warehouse", {"n_agents": 8}, "exact"),
                ("Warehouse", {"n_agents": 8}, "cvxopt"),
                ("Simple", {}, "exact")]


@pytest.mark.parametrize("scenario,ov,solver", ORACLE_CASES)
def test_mixed_teams_are_bit_exact_against_the_float32_oracle(scenario, ov, solver, oracle_lib):
    mixed_teams_vs_oracle(scenario, ov, solver, oracle_lib, 256, 80, 15)


# ---------------------------------------------------------------- 3. the draw
def _check_invariant(env):
    want = expected_after_reset(env.seed, env.env_offset, env.reset_count.cpu().numpy(), env.teams.n_sets, env.teams.mode)
    assert np.array_equal(env.team_index.cpu().numpy(), want)


@pytest.mark.parametrize("scenario", ["PredatorCapturePrey", "MaterialTransport"])
def test_index_follows_the_twin_on_every_reset_path(scenario):
    E, T = 200, 40
    env = _env(scenario, E, {"max_episode_steps": 7}, teams=_pool4(scenario, SCN_OV[scenario]["n_agents"]), seed=123,
               env_offset=1000)
    env.reset()
    _check_invariant(env)
    assert len(set(env.team_index.cpu().tolist())) == 4
    mask = torch.zeros(E, dtype=torch.uint8, device=env.device)
    mask[::3] = 1
    before, rc0 = env.team_index.clone(), env.reset_count.clone()
    env.reset(mask=mask)                                          # masked rg_reset
    _check_invariant(env)
    assert torch.equal(env.team_index[mask == 0], before[mask == 0])
    assert bool((env.reset_count != rc0).eq(mask.bool()).all())
    acts = _actions(env, T, seed=4)
    n_reset = 0
    for t in range(T):                                            # fused auto-reset, drawn-ahead blocks included
        prev_i, prev_rc = env.team_index.clone(), env.reset_count.clone()
        env.step(acts[t])
        _check_invariant(env)
        same = env.reset_count == prev_rc
        assert torch.equal(env.team_index[same], prev_i[same])   # the index moves only when an episode starts
        n_reset += int((~same).sum())
    assert n_reset > E
    env.reset(mask=mask, reference_rng=np.random.RandomState(2))  # states uploaded from the reference's RNG
    _check_invariant(env)
    out = env.rollout(acts[:10])                                   # the multi-step launch's resets
    assert int(out["done"].sum()) > 0
    _check_invariant(env)


def test_frequencies_are_uniform():
    E, C = 4096, 4
    env = _env("Warehouse", E, teams=[{"step_dist": [0.1 + 0.05 * t] * 8} for t in range(C)], seed=77)
    counts = np.zeros(C, np.int64)
    for r in range(6):
        env.reset()
        counts += np.bincount(env.team_index.cpu().numpy(), minlength=C)
    n = counts.sum()
    sigma = np.sqrt(n * 0.25 * 0.75)
    assert np.all(np.abs(counts - n / C) < 5 * sigma), counts


def test_fixed_mode_is_offset_plus_env_mod_c():
    E, C, off = 300, 7, 5003
    env = _env("Simple", E, {"max_episode_steps": 5}, teams=[{"step_dist": [0.1 + 0.02 * t] * 4} for t in range(C)],
               sampling="fixed", seed=3, env_offset=off)
    want = (off + np.arange(E)) % C
    assert np.array_equal(env.team_index.cpu().numpy(), want)      # written by rg_set_teams
    env.reset()
    assert np.array_equal(env.team_index.cpu().numpy(), want)
    acts = _actions(env, 20, seed=1)
    for t in range(20):
        env.step(acts[t])
        assert np.array_equal(env.team_index.cpu().numpy(), want)
    assert int(env.done_count.sum()) > 0


def test_two_shards_reproduce_one_handle():
    E = 256
    teams = _pool4("PredatorCapturePrey", 5)
    one = _env("PredatorCapturePrey", E, {"max_episode_steps": 9}, teams=teams, seed=9)
    a = _env("PredatorCapturePrey", E // 2, {"max_episode_steps": 9}, teams=teams, seed=9)
    b = _env("PredatorCapturePrey", E // 2, {"max_episode_steps": 9}, teams=teams, seed=9, env_offset=E // 2)
    for e in (one, a, b):
        e.reset()
    acts = _actions(one, 30, seed=8)
    for t in range(30):
        one.step(acts[t])
        a.step(acts[t][:E // 2].contiguous())
        b.step(acts[t][E // 2:].contiguous())
        assert _same(one.team_index, torch.cat([a.team_index, b.team_index])), t
        for k in OUT_KEYS:
            assert _same(getattr(one, k), torch.cat([getattr(a, k), getattr(b, k)])), (t, k)


# ---------------------------------------------------------------- 4. paths
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("scenario", list(SCN_OV))
def test_rollout_equals_single_steps(scenario, solver):
    E, K = 130, 24
    ov = {"barrier_solver": solver, "max_episode_steps": 8}
    teams = _pool4(scenario, int(SCN_OV[scenario].get("n_agents", 4)))
    s = _env(scenario, E, ov, teams=teams, seed=21)
    r = _env(scenario, E, ov, teams=teams, seed=21)
    s.reset()
    r.reset()
    rollout_equals_single_steps(s, r, _actions(s, K, seed=6), more_state=("team_index",))


def test_gymma_step_and_get_obs_equal_the_plain_step():
    scenario, E, T = "MaterialTransport", 100, 30
    teams = _pool4(scenario, 6)
    ov = {"capability_aware": True, "max_episode_steps": 9}
    plain = _env(scenario, E, ov, teams=teams, seed=2)
    gym = _env(scenario, E, ov, teams=teams, seed=2)
    gym.enable_time_limit(10 ** 6)
    plain.reset()
    gym.reset()
    acts = _actions(plain, T, seed=5)
    for t in range(T):
        plain.step(acts[t])
        gym.step(acts[t])
        for k in OUT_KEYS:
            assert _same(getattr(plain, k), getattr(gym, k)), (t, k)
    # get_obs: the observation of the current state, as the step that produced it (no auto-reset in between)
    env = _env("PredatorCapturePrey", E, {"capability_aware": True}, teams=_pool4("PredatorCapturePrey", 5), seed=4, auto_reset=False)
    env.reset()
    for t in range(5):
        env.step(acts[t][:, :5] % 5)
        stepped = env.obs.clone()
        assert _same(env.get_obs(torch.empty_like(stepped)), stepped), t


def test_snapshot_restores_the_team_and_continues_identically():
    scenario, E = "PredatorCapturePrey", 128
    teams = _pool4(scenario, 5)
    env = _env(scenario, E, {"max_episode_steps": 6}, teams=teams, seed=31)
    env.reset()
    acts = _actions(env, 20, seed=2)
    for t in range(5):
        env.step(acts[t])
    sd = env.state_dict()
    assert "team_index" in sd and torch.equal(sd["team_index"], env.team_index)
    first = []
    for t in range(5, 20):
        env.step(acts[t])
        first.append((env.obs.clone(), env.reward.clone(), env.team_index.clone()))
    other = _env(scenario, E, {"max_episode_steps": 6}, teams=teams, seed=0)
    other.load_state_dict(sd)
    for i, t in enumerate(range(5, 20)):
        other.step(acts[t])
        assert _same(other.obs, first[i][0]) and _same(other.reward, first[i][1]) and _same(other.team_index, first[i][2]), t
    plain = _env(scenario, E, seed=1)
    sd_plain = plain.state_dict()
    assert "team_index" not in sd_plain and set(sd_plain) == set(plain.STATE_KEYS) | {"seed"}
    with pytest.raises(KeyError, match="team"):
        plain.load_state_dict(sd)


def test_batched_runner_two_launch_path_and_one_launch_refusals():
    from marbler_amd.evaluate import BatchedActor, policy_rollout
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    E, T = 64, 8
    ov = dict(SCN_OV["PredatorCapturePrey"], teams=_pool4("PredatorCapturePrey", 5))
    v = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", E, time_limit=5, seed=3, overrides=ov)
    assert v.env.teams is not None and v.env.teams.n_sets == 4
    N = v.n_agents
    actor = BatchedActor(random_actor(1, v.obs_size + N, 64, v.n_actions, True, seed=4), N, device=v.env.device)
    runner = BatchedRunner(v, actor, epsilon=0.1, seed=1)
    out = runner.run(T)
    torch.cuda.synchronize()
    assert out["obs"].shape == (T + 1, E, N, v.obs_size)
    runner_batch_replays(out, "robotarium_gym:PredatorCapturePrey-v0", E, T, ov)
    with pytest.raises(ValueError, match="team"):
        runner.run(T, one_launch=True)
    with pytest.raises(ValueError, match="team"):
        policy_rollout(v.env, actor, T, None, None, None)


# ---------------------------------------------------------------- 5. guards
def test_guard_slabs_around_the_pool_stay_untouched():
    Guarded = guarded_class()
    for scenario in ("PredatorCapturePrey", "MaterialTransport"):
        E = 65
        o = dict(SCN_OV[scenario], teams=_pool4(scenario, SCN_OV[scenario]["n_agents"]), max_episode_steps=5)
        env = Guarded(scenario, E, overrides=o, device="cuda:0", seed=4)
        assert env.team_index is not None
        env.reset()
        mask = torch.zeros(E, dtype=torch.uint8, device=env.device)
        mask[1::2] = 1
        env.reset(mask=mask)
        acts = _actions(env, 20, seed=3)
        for t in range(12):
            env.step(acts[t])
        env.rollout(acts[12:])
        env.get_obs()
        torch.cuda.synchronize()
        bad = env.red_zones_intact()
        assert bad.size == 0, (scenario, [env.owner_of(int(o)) for o in bad[:5]])
        _check_invariant(env)
