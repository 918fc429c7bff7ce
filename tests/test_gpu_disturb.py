"""The pose disturbance on the GPU (DESIGN.md "Pose disturbance"): every step against the float32 oracle stepped from the pose the
NumPy twin (tests/disturb_twin.py) displaces (tests/disturb_harness.py; what is compared: tests/oracle_check.py), in both solver modes, at every group width, with envs sharing a ragged
wavefront; bit identity across the forms that step a disturbed env (rg_step / rg_rollout / the gymma step / shards / snapshots);
rg_get_obs displaces nothing; both sigma zero is the handle that never made the call; every refusal; guard slabs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from disturb_cases import MT6, PCP4, PCP5, PCP9
from disturb_harness import (NOISE, OUT_KEYS, SXY, STH, check_step, disturbed_vs_oracle, make_env as _env, oracle_step as _oracle_step,
                             plain_oracle)
from gpu_helpers import (expected_slots, fused_time_limit_vs_composed, guarded_class, random_actions as _actions, random_actor,
                         rollout_equals_single_steps, runner_batch_replays, same_bits as _same)
from oracle_check import assert_same_words, gpu_state as _gpu_state

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. / 2. bit parity with the float32 oracle
ORACLE_CASES = [("pcp-n4", "PredatorCapturePrey", PCP4),                 # GW 4
                ("pcp-n5", "PredatorCapturePrey", PCP5),                 # GW 8
                ("pcp-n9", "PredatorCapturePrey", PCP9),                 # GW 16
                ("warehouse-n6", "Warehouse", {"n_agents": 6}),
                ("material-n6", "MaterialTransport", MT6),
                ("material-n4", "MaterialTransport", {}),
                ("simple-n4", "Simple", {}),
                ("arctic-n4", "ArcticTransport", {})]


@pytest.mark.parametrize("name,scenario,ov", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_disturbed_steps_are_bit_exact_vs_the_oracle_from_the_displaced_state(name, scenario, ov, oracle_lib):
    """E = 67: several envs share a wavefront and the last wave is ragged; auto-reset on, 12 steps of 5-step episodes."""
    disturbed_vs_oracle(scenario, ov, "exact", 67, 12, oracle_lib)


@pytest.mark.parametrize("scenario,ov", [("PredatorCapturePrey", PCP4), ("Warehouse", {"n_agents": 5})], ids=["pcp-n4", "warehouse-n5"])
def test_interior_point_mode_is_bit_exact_vs_the_oracle(scenario, ov, oracle_lib):
    disturbed_vs_oracle(scenario, ov, "cvxopt", 35, 6, oracle_lib, episode_steps=3)


# ---------------------------------------------------------------- 3. form invariance
def test_k_steps_equal_one_rollout():
    E, K = 67, 8
    ov = dict(PCP5, max_episode_steps=5)
    s, r = _env("PredatorCapturePrey", E, ov, seed=21), _env("PredatorCapturePrey", E, ov, seed=21)
    s.reset()
    r.reset()
    out = rollout_equals_single_steps(s, r, _actions(s, K, seed=6))
    assert int(out["done"].sum()) >= E


def test_gymma_step_equals_the_plain_step_with_the_composed_time_limit():
    fused_time_limit_vs_composed("robotarium_gym:PredatorCapturePrey-v0", dict(PCP5, **NOISE), 5, 9, 67, 24)


def test_a_shard_reproduces_its_envs_of_the_whole_batch():
    E, off, T = 67, 32, 8
    ov = dict(PCP5, max_episode_steps=5)
    one = _env("PredatorCapturePrey", E, ov, seed=9)
    part = _env("PredatorCapturePrey", E - off, ov, seed=9, env_offset=off)
    one.reset()
    part.reset()
    acts = _actions(one, T, seed=8)
    for t in range(T):
        one.step(acts[t])
        part.step(acts[t][off:].contiguous())
        for k in OUT_KEYS + ("poses",):
            assert _same(getattr(one, k)[off:], getattr(part, k)), (t, k)


def test_snapshot_continues_identically():
    E = 67
    ov = dict(PCP5, max_episode_steps=5)
    env = _env("PredatorCapturePrey", E, ov, seed=31)
    env.reset()
    acts = _actions(env, 8, seed=2)
    for t in range(4):
        env.step(acts[t])
    sd = env.state_dict()
    assert set(sd) == set(env.STATE_KEYS) | {"seed"}            # the disturbance adds no state
    first = []
    for t in range(4, 8):
        env.step(acts[t])
        first.append((env.obs.clone(), env.reward.clone(), env.poses.clone()))
    other = _env("PredatorCapturePrey", E, ov, seed=0)
    other.load_state_dict(sd)
    for i, t in enumerate(range(4, 8)):
        other.step(acts[t])
        assert _same(other.obs, first[i][0]) and _same(other.reward, first[i][1]) and _same(other.poses, first[i][2]), t


def test_get_obs_displaces_nothing(oracle_lib):
    """rg_get_obs before a step: the oracle's observation of the stored, undisplaced state (what its last step returned, no
    auto-reset in between), the same words the plain observation kernel gives a handle without the disturbance; state untouched."""
    E = 67
    env = _env("PredatorCapturePrey", E, PCP5, seed=4, auto_reset=False)
    plain = _env("PredatorCapturePrey", E, PCP5, noisy=False, seed=4, auto_reset=False)
    orc = plain_oracle(oracle_lib, env)
    env.reset()
    acts = _actions(env, 3, seed=6)
    for t in range(3):
        pre, rc = _gpu_state(env), env.reset_count.cpu().numpy()
        env.step(acts[t])
        o_obs = _oracle_step(orc, env, pre, rc, acts[t].cpu().numpy())[0]
        before = _gpu_state(env)
        seen = env.get_obs(torch.full_like(env.obs, float("nan")))
        torch.cuda.synchronize()
        assert_same_words(seen.cpu().numpy(), o_obs, "obs (rg_get_obs)", step=t)
        after = _gpu_state(env)
        for k in before:
            assert_same_words(after[k], before[k], k, "rg_get_obs", t)
        plain.load_state_dict(env.state_dict())
        assert _same(plain.get_obs(torch.full_like(plain.obs, float("nan"))), seen), t


# ---------------------------------------------------------------- 4. shared, ragged wavefronts at dispatch width
@pytest.mark.parametrize("scenario,ov", [("PredatorCapturePrey", PCP4), ("PredatorCapturePrey", PCP5), ("PredatorCapturePrey", PCP9)],
                         ids=["gw4", "gw8", "gw16"])
def test_one_step_of_1025_envs_vs_the_oracle(scenario, ov, oracle_lib):
    """1025 envs: the batch at which wave_fill goes from one env per wave to two, the last wave ragged."""
    E = 1025
    assert expected_slots(int(ov["n_agents"]), E) == 2
    env = _env(scenario, E, ov, seed=17)
    orc = plain_oracle(oracle_lib, env)
    env.reset()
    acts = _actions(env, 1, seed=5)
    pre, rc = _gpu_state(env), env.reset_count.cpu().numpy()
    env.step(acts[0])
    o_done = _oracle_step(orc, env, pre, rc, acts[0].cpu().numpy())[2]
    check_step(env, orc, scenario)
    alive = np.nonzero(o_done == 0)[0]
    post = _gpu_state(env)
    _oracle_step(orc, env, pre, rc, acts[0].cpu().numpy(), displaced=False)      # ... and not what the undisplaced state steps to
    assert (post["poses"][alive] != orc.poses[alive]).any(axis=(1, 2)).mean() > 0.9


# ---------------------------------------------------------------- 5. off and guards
def _set(env, sxy, sth):
    from marbler_amd import _lib
    rc = env.lib.rg_set_disturbance(env._h, C.byref(_lib.RgDisturbanceParams(sxy, sth)))
    return rc, env.lib.rg_last_error().decode()


def test_both_sigma_zero_is_the_handle_that_never_made_the_call():
    """65 536 envs of 5 agents: the batch at which rg_create picks the thread-per-env kernel, so the kernel choice shows."""
    E = 65536
    never = _env("PredatorCapturePrey", E, PCP5, noisy=False, seed=3)
    zero = _env("PredatorCapturePrey", E, PCP5, noisy=False, seed=3)
    kernel = never.lib.rg_step_kernel(never._h)
    assert kernel == 1 or "RG_STEP_KERNEL" in os.environ
    assert _set(zero, 0.0, 0.0)[0] == 0 and zero.lib.rg_set_disturbance(zero._h, None) == 0
    assert zero.lib.rg_step_kernel(zero._h) == kernel
    never.reset()
    zero.reset()
    acts = _actions(never, 2, seed=1)

    def check(t):
        never.step(acts[t])
        zero.step(acts[t])
        for k in OUT_KEYS + ("poses", "carry_dist"):
            assert _same(getattr(never, k), getattr(zero, k)), (t, k)

    check(0)
    assert _set(zero, SXY, 0.0)[0] == 0 and zero.lib.rg_step_kernel(zero._h) == 0      # on: the lane-group kernels at every size
    assert _set(zero, 0.0, 0.0)[0] == 0 and zero.lib.rg_step_kernel(zero._h) == kernel  # off again: the default choice is back
    check(1)


def test_c_abi_refusals_name_their_reason():
    from marbler_amd import _lib
    env = _env("PredatorCapturePrey", 8, PCP5, noisy=False, seed=1)
    for sxy, sth, code, word in ((0.2, 0.0, -70, "sigma_xy"), (-0.01, 0.0, -70, "sigma_xy"), (float("nan"), 0.1, -70, "sigma_xy"),
                                 (float("inf"), 0.1, -70, "sigma_xy"), (0.01, 0.6, -71, "sigma_theta"), (0.01, -0.1, -71, "sigma_theta"),
                                 (0.0, float("nan"), -71, "sigma_theta"), (0.01, float("-inf"), -71, "sigma_theta")):
        rc, msg = _set(env, sxy, sth)
        assert rc == code and word in msg and "rg_set_disturbance" in msg, (sxy, sth, rc, msg)
    assert env.lib.rg_step_kernel(env._h) == 0 and _set(env, 0.1, 0.5)[0] == 0          # the bounds themselves are admitted
    # a disturbed handle takes neither the lidar nor a pool ...
    lp = _lib.RgLidarParams()
    lp.rays, lp.offset, lp.range, lp.inv_range = 8, env.D - 8, 1.0, 1.0
    assert env.lib.rg_set_lidar(env._h, C.byref(lp)) == -57 and "disturbance" in env.lib.rg_last_error().decode()
    idx = torch.zeros(8, dtype=torch.int32, device=env.device)
    tab = torch.zeros(5, device=env.device)
    tp = _lib.RgTeamParams(1, _lib.TEAM_EPISODE, tab.data_ptr(), tab.data_ptr(), tab.data_ptr(), tab.data_ptr(), idx.data_ptr())
    assert env.lib.rg_set_teams(env._h, C.byref(tp)) == -65 and "disturbance" in env.lib.rg_last_error().decode()
    # ... nor the one-launch policy rollouts
    w, pio = _lib.RgActorWeights(), _lib.RgPolicyIO()
    assert env.lib.rg_policy_rollout(env._h, C.byref(w), 2, C.byref(pio), env._io_ref, 1, 0) == -38
    assert "disturbance" in env.lib.rg_last_error().decode()
    u = torch.zeros(2, 8, 5, device=env.device)
    ps = _lib.RgPolicySample(u.data_ptr(), None)
    assert env.lib.rg_policy_rollout_sample(env._h, C.byref(w), 2, C.byref(pio), C.byref(ps), env._io_ref, 1, 0) == -38
    assert "disturbance" in env.lib.rg_last_error().decode()
    # ... and a handle with the lidar or a pool does not take the disturbance
    lid = _env("PredatorCapturePrey", 8, dict(PCP5, lidar_rays=8), noisy=False, seed=1)
    rc, msg = _set(lid, SXY, STH)
    assert rc == -72 and "lidar" in msg
    pooled = _env("PredatorCapturePrey", 8, dict(PCP5, teams=[{}]), noisy=False, seed=1)
    rc, msg = _set(pooled, SXY, STH)
    assert rc == -73 and "team pool" in msg
    assert _set(lid, 0.0, 0.0)[0] == 0 and _set(pooled, 0.0, 0.0)[0] == 0                # turning it off is always admitted


def test_python_refusals_and_the_two_launch_runner():
    from marbler_amd.evaluate import BatchedActor, policy_rollout, run_eval
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    with pytest.raises(ValueError, match="lidar"):
        _env("PredatorCapturePrey", 8, dict(PCP5, lidar_rays=8))
    with pytest.raises(ValueError, match="team pool"):
        _env("PredatorCapturePrey", 8, dict(PCP5, teams=[{}]))
    E, T = 64, 8
    ov = dict(PCP5, **NOISE)
    v = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", E, time_limit=5, seed=3, overrides=ov)
    assert v.env.disturbance is not None and v.env.step_kernel == "group"
    N = v.n_agents
    actor = BatchedActor(random_actor(1, v.obs_size + N, 64, v.n_actions, True, seed=4), N, device=v.env.device)
    runner = BatchedRunner(v, actor, epsilon=0.1, seed=1)
    with pytest.raises(ValueError, match="pose disturbance"):
        runner.run(T, one_launch=True)
    with pytest.raises(ValueError, match="pose disturbance"):
        policy_rollout(v.env, actor, T, None, None, None)
    with pytest.raises(ValueError, match="pose disturbance"):
        run_eval(v.env, actor, T, one_launch=True)
    out = runner.run(T)
    torch.cuda.synchronize()
    assert out["obs"].shape == (T + 1, E, N, v.obs_size)
    runner_batch_replays(out, "robotarium_gym:PredatorCapturePrey-v0", E, T, ov)
    stats = run_eval(_env("PredatorCapturePrey", E, dict(PCP5, max_episode_steps=5), seed=2), actor, 12)   # the two-launch loop runs
    assert stats["episodes"] >= E


# ---------------------------------------------------------------- 6. sentinel-filled tails
@pytest.mark.parametrize("scenario,ov", [("PredatorCapturePrey", PCP5), ("MaterialTransport", {}), ("PredatorCapturePrey", PCP9)],
                         ids=["pcp-n5", "material-n4", "pcp-n9"])
def test_guard_slabs_stay_untouched(scenario, ov):
    Guarded = guarded_class()
    E = 67
    env = Guarded(scenario, E, overrides=dict(ov, max_episode_steps=5, **NOISE), device="cuda:0", seed=4)
    assert env.disturbance is not None
    env.reset()
    acts = _actions(env, 16, seed=3)
    for t in range(8):
        env.step(acts[t])
    env.rollout(acts[8:])
    env.get_obs()
    torch.cuda.synchronize()
    bad = env.red_zones_intact()
    assert bad.size == 0, (scenario, [env.owner_of(int(o)) for o in bad[:5]])
