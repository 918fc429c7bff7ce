"""The pose disturbance on the GPU (DESIGN.md "Pose disturbance"): every step bit for bit against the float32 oracle stepped from
the pose the NumPy twin (tests/disturb_twin.py) displaces, in both solver modes, at every group width, with envs sharing a ragged
wavefront; bit identity across the forms that step a disturbed env (rg_step / rg_rollout / the gymma step / shards / snapshots);
rg_get_obs displaces nothing; both sigma zero is the handle that never made the call; every refusal; guard slabs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from disturb_cases import Regime
from disturb_twin import displace
from helpers import GPU_NAME, STATE_KEYS
from test_gpu_actor import _random_actor
from test_gpu_baseline_shapes import expected_slots
from test_gpu_redzone import _guarded_class
from test_gpu_wrapper import fused_time_limit_vs_composed

pytestmark = pytest.mark.gpu

SXY, STH = 0.01, 0.05
NOISE = {"pose_noise_xy": SXY, "pose_noise_theta": STH}
PCP4 = {"predator": 2, "capture": 2, "n_agents": 4}
PCP5 = {"predator": 3, "capture": 2, "n_agents": 5}
PCP9 = {"predator": 5, "capture": 4, "n_agents": 9, "start_dist": 0.25, "num_neighbors": 4}
MT6 = {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25}
N_ACT = {"MaterialTransport": 20}
OUT_KEYS = ("obs", "reward", "done_u8", "dist_travelled", "violation", "remaining")
THREADS = max(1, min(16, os.cpu_count() or 1))


def _noise(sigma):
    return {"pose_noise_xy": sigma[0], "pose_noise_theta": sigma[1]}


def _env(scenario, E, ov=None, noise=True, sigma=(SXY, STH), **kw):
    from marbler_amd.vec_env import VecRobotariumEnv
    return VecRobotariumEnv(scenario, E, overrides=dict(ov or {}, **(_noise(sigma) if noise else {})), device="cuda:0", **kw)


def _actions(env, T, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, N_ACT.get(env.scenario, 5), (T, env.E, env.N), generator=g, dtype=torch.int32).to(env.device)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _gpu_state(env):
    return {k: getattr(env, GPU_NAME.get(k, k)).cpu().numpy() for k in STATE_KEYS}


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)


def _oracle_step(orc, env, pre, reset_count, acts, displaced=True, sigma=(SXY, STH), regime=None):
    """The oracle loaded with the GPU's state `pre`, its poses displaced by the twin, stepped with `acts`.  `regime`
    (disturb_cases.Regime) is shown the stored and the displaced poses."""
    for k in STATE_KEYS:
        arr = getattr(orc, k)
        arr[...] = pre[k].astype(arr.dtype).reshape(arr.shape)
    if displaced:
        orc.poses[...] = displace(pre["poses"], env.seed, env.env_offset, reset_count, pre["steps"], sigma[0], sigma[1])
        if regime is not None:
            regime.see_poses(pre["poses"], orc.poses)
    return orc.step(acts, threads=THREADS)


def disturbed_vs_oracle(scenario, ov, solver, E, T, oracle_lib, episode_steps=5, seed=13, env_offset=0, sigma=(SXY, STH)):
    """Every step: the GPU's state before the step into the oracle, the oracle's poses displaced by the twin, one step of each;
    every word of the outputs (the QP's sweep or iteration count among them) and -- for envs that did not end (the others were
    reset) -- of the stored state.  Returns what it collected: the actions [T, E, N], every output stacked over the steps
    (`steps`), the stepped handle's final `state_dict` and the oracle's counts (`regime`, a disturb_cases.Regime)."""
    ov = dict(ov, barrier_solver=solver, max_episode_steps=episode_steps)
    env = _env(scenario, E, ov, sigma=sigma, seed=seed, env_offset=env_offset, collect_qp_stats=True)
    plain = _env(scenario, E, ov, noise=False, seed=seed, env_offset=env_offset)
    assert env.disturbance is not None and plain.disturbance is None and env.step_kernel == "group"
    cfg = {k: v for k, v in env.cfg.items() if k not in NOISE}
    orc = oracle_lib.OracleVecEnv(scenario, cfg, E, dtype=np.float32)
    env.reset()
    plain.reset()
    assert _same(env.poses, plain.poses)
    acts = _actions(env, T, seed=3)
    acts_np = acts.cpu().numpy()
    regime = Regime()
    kept = {k: [] for k in OUT_KEYS + ("qp_sweeps",)}
    for t in range(T):
        pre, rc = _gpu_state(env), env.reset_count.cpu().numpy()
        env.step(acts[t])
        plain.step(acts[t])
        o_obs, o_rew, o_done, o_info = _oracle_step(orc, env, pre, rc, acts_np[t], sigma=sigma, regime=regime)
        regime.see_step(o_done, o_info["violation"], orc.qp_sweeps)
        for k in kept:
            kept[k].append(getattr(env, k).clone())
        got = {k: kept[k][-1].cpu().numpy() for k in kept}
        for k, want in (("done_u8", o_done), ("violation", o_info["violation"]), ("remaining", o_info["remaining"]), ("obs", o_obs),
                        ("reward", o_rew), ("dist_travelled", o_info["dist_travelled"]), ("qp_sweeps", orc.qp_sweeps)):
            a, b = _words(got[k]), _words(np.asarray(want).astype(got[k].dtype))
            if not np.array_equal(a, b):
                bad = np.nonzero((a != b).reshape(E, -1).any(axis=1))[0]
                raise AssertionError(f"{scenario} {solver}: {k} differs at step {t} in {len(bad)} envs, first {bad[:8].tolist()}")
        alive = np.nonzero(o_done == 0)[0]
        post = _gpu_state(env)
        for k in STATE_KEYS:
            a, b = post[k][alive], getattr(orc, k)[alive].astype(post[k].dtype).reshape(post[k][alive].shape)
            assert np.array_equal(_words(a), _words(b)), (scenario, solver, t, k)
    assert regime.episode_ends >= E, "every env ends at least one episode inside the run (the draw's episode and step both move)"
    assert not _same(env.poses, plain.poses) and not _same(env.obs, plain.obs), "the disturbance changed nothing"
    result = {"actions": acts, "steps": {k: torch.stack(v) for k, v in kept.items()}, "state": env.state_dict(), "regime": regime}
    env.close()
    plain.close()
    return result


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
    acts = _actions(s, K, seed=6)
    out = r.rollout(acts)
    for t in range(K):
        s.step(acts[t])
        for k, ko in (("obs", "obs"), ("reward", "reward"), ("done_u8", "done"), ("dist_travelled", "dist_travelled"),
                      ("violation", "violation"), ("remaining", "remaining")):
            assert _same(getattr(s, k), out[ko][t]), (t, k)
    for k in s.STATE_KEYS:
        assert _same(getattr(s, k), getattr(r, k)), k
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
    plain = _env("PredatorCapturePrey", E, PCP5, noise=False, seed=4, auto_reset=False)
    orc = oracle_lib.OracleVecEnv("PredatorCapturePrey", {k: v for k, v in env.cfg.items() if k not in NOISE}, E, dtype=np.float32)
    env.reset()
    acts = _actions(env, 3, seed=6)
    for t in range(3):
        pre, rc = _gpu_state(env), env.reset_count.cpu().numpy()
        env.step(acts[t])
        o_obs = _oracle_step(orc, env, pre, rc, acts[t].cpu().numpy())[0]
        before = _gpu_state(env)
        seen = env.get_obs(torch.full_like(env.obs, float("nan")))
        torch.cuda.synchronize()
        assert np.array_equal(_words(seen.cpu().numpy()), _words(o_obs)), t
        after = _gpu_state(env)
        assert all(np.array_equal(_words(before[k]), _words(after[k])) for k in STATE_KEYS)
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
    orc = oracle_lib.OracleVecEnv(scenario, {k: v for k, v in env.cfg.items() if k not in NOISE}, E, dtype=np.float32)
    env.reset()
    acts = _actions(env, 1, seed=5)
    pre, rc = _gpu_state(env), env.reset_count.cpu().numpy()
    env.step(acts[0])
    o_obs, o_rew, o_done, o_info = _oracle_step(orc, env, pre, rc, acts[0].cpu().numpy())
    for k, want in (("obs", o_obs), ("reward", o_rew), ("done_u8", o_done), ("dist_travelled", o_info["dist_travelled"]),
                    ("violation", o_info["violation"]), ("remaining", o_info["remaining"])):
        got = getattr(env, k).cpu().numpy()
        assert np.array_equal(_words(got), _words(np.asarray(want).astype(got.dtype))), k
    alive = np.nonzero(o_done == 0)[0]
    post = _gpu_state(env)
    for k in STATE_KEYS:
        a = post[k][alive]
        assert np.array_equal(_words(a), _words(getattr(orc, k)[alive].astype(a.dtype).reshape(a.shape))), k
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
    never = _env("PredatorCapturePrey", E, PCP5, noise=False, seed=3)
    zero = _env("PredatorCapturePrey", E, PCP5, noise=False, seed=3)
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
    env = _env("PredatorCapturePrey", 8, PCP5, noise=False, seed=1)
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
    lid = _env("PredatorCapturePrey", 8, dict(PCP5, lidar_rays=8), noise=False, seed=1)
    rc, msg = _set(lid, SXY, STH)
    assert rc == -72 and "lidar" in msg
    pooled = _env("PredatorCapturePrey", 8, dict(PCP5, teams=[{}]), noise=False, seed=1)
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
    actor = BatchedActor(_random_actor(1, v.obs_size + N, 64, v.n_actions, True, seed=4), N, device=v.env.device)
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
    w = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", E, time_limit=5, seed=3, overrides=ov)
    w.reset()
    for t in range(T):
        _, ended, _ = w.step(out["actions"][t])
        torch.cuda.synchronize()
        assert torch.equal(ended, out["terminated"][t])
        assert torch.equal(w.get_obs(), out["obs"][t + 1])
    stats = run_eval(_env("PredatorCapturePrey", E, dict(PCP5, max_episode_steps=5), seed=2), actor, 12)   # the two-launch loop runs
    assert stats["episodes"] >= E


# ---------------------------------------------------------------- 6. sentinel-filled tails
@pytest.mark.parametrize("scenario,ov", [("PredatorCapturePrey", PCP5), ("MaterialTransport", {}), ("PredatorCapturePrey", PCP9)],
                         ids=["pcp-n5", "material-n4", "pcp-n9"])
def test_guard_slabs_stay_untouched(scenario, ov):
    Guarded = _guarded_class()
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
