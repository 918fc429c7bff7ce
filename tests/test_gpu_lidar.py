"""The lidar observation on the GPU (DESIGN.md "Lidar"): ranges against the float64 twin (tests/lidar_twin.py) from the poses the
GPU itself stored, non-interference with everything else a step computes, bit identity across the paths that write it, zero rows,
guard slabs, and the two-launch BatchedRunner."""
import numpy as np
import pytest
import torch

from lidar_twin import bounds_of, lidar_batch
from test_gpu_actor import _random_actor

pytestmark = pytest.mark.gpu

RHO = float(np.float32(0.5) * np.float32(0.11))
SCN_OV = {  # every scenario, with the agent counts of the benchmark configurations where they differ from the YAML
    "PredatorCapturePrey": {"predator": 3, "capture": 2, "n_agents": 5},
    "Warehouse": {"n_agents": 8},
    "MaterialTransport": {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25},
    "Simple": {},
    "ArcticTransport": {},
}
N_ACT = {"MaterialTransport": 20}


def _env(scenario, E, R, ov=None, L=1.0, **kw):
    from marbler_amd.vec_env import VecRobotariumEnv
    o = dict(SCN_OV.get(scenario, {}), **(ov or {}))
    if R:
        o.update(lidar_rays=R, lidar_range=L)
    return VecRobotariumEnv(scenario, E, overrides=o, device="cuda:0", **kw)


def _actions(env, T, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, N_ACT.get(env.scenario, 5), (T, env.E, env.N), generator=g, dtype=torch.int32).to(env.device)


def _check_against_twin(obs, poses, env, L=1.0, max_degenerate=1e-3, exact_zero=None):
    """obs [E, N, D] (device), poses [E, 3, N] the stored poses the step built it from.  Returns the number of rays compared."""
    R, off = int(env.lidar.rays), int(env.lidar.offset)
    got = obs[..., off:off + R].double().cpu().numpy()
    rho = float(np.float32(0.5) * np.float32(env.params.robot_diameter))   # (= RHO at the default constants)
    want, deg = lidar_batch(poses.cpu().numpy(), R, L, rho, bounds_of(env.params))
    ok = ~deg
    assert deg.sum() <= max_degenerate * deg.size, (int(deg.sum()), deg.size)
    err = np.abs(got - want)[ok]
    assert err.max(initial=0.0) <= 2e-5, float(err.max())
    far = ok & (want == 1.0)          # the twin's range exceeds L (+ EPS: the rays within EPS of L are degenerate)
    assert (got[far] == 1.0).all()
    zero = ok & (want == 0.0)         # overlap, outside the arena
    assert (got[zero] == 0.0).all()
    if exact_zero is not None:
        assert (got[exact_zero] == 0.0).all()
    return int(ok.sum())


@pytest.mark.parametrize("R", [4, 16, 32])
@pytest.mark.parametrize("scenario", sorted(SCN_OV))
def test_ranges_match_the_float64_twin(scenario, R):
    ranges_vs_twin(scenario, R)


def ranges_vs_twin(scenario, R, E=256, T=4, ov=None):
    env = _env(scenario, E, R, ov, seed=3, auto_reset=False)
    assert env.D == env.lidar.offset + R and env.step_kernel == "group"
    env.reset()
    # random headings: the reset's are axis-aligned, and robots on the grid row y = 0 then sit exactly L = 1 m from the side
    # walls on two of their rays (a degenerate ray for any binary32 evaluation)
    sd = env.state_dict()
    g = torch.Generator(device="cpu").manual_seed(R)
    sd["poses"][:, 2, :] = (torch.rand(env.E, env.N, generator=g) * 2.0 - 1.0) * 3.14159
    env.load_state_dict(sd)
    acts = _actions(env, T, seed=11)
    compared = 0
    for t in range(T):
        obs, _, _, _ = env.step(acts[t])
        torch.cuda.synchronize()
        compared += _check_against_twin(obs, env.poses, env)
    assert compared > 0.99 * T * env.E * env.N * R


def test_hand_placed_states():
    """Robots touching, overlapping, on a ray line and outside the arena, loaded with load_state_dict, read with get_obs."""
    env = _env("Simple", 6, 16, seed=1, auto_reset=False)
    env.reset()
    sd = env.state_dict()
    poses = sd["poses"].cpu().numpy().copy()            # [E, 3, N], N = 4
    d = np.float32(2 * RHO)
    place = [
        ([0.0, d, -0.9, 0.9], [0.0, 0.0, -0.5, 0.5], [0.0, np.pi, 0.3, -2.0]),                    # 0, 1 touching, facing
        ([0.0, 0.03, -0.9, 0.9], [0.0, 0.02, -0.5, 0.5], [0.0, 1.0, 0.3, -2.0]),                  # 0, 1 overlapping
        ([-1.0, 0.0, 0.5, 1.0], [0.2, 0.2, 0.2, 0.2], [0.0, 0.0, np.pi, 0.5]),                    # four on the line y = 0.2
        ([1.7, 0.0, -1.65, 0.5], [0.0, 0.0, 0.3, -1.2], [0.0, 1.0, 2.0, 3.0]),                    # 0, 2, 3 outside
        ([-1.6, 1.6, 0.0, 0.3], [-1.0, 1.0, 0.0, 0.3], [0.7, -2.4, 0.0, 0.0]),                    # on two corners
        ([0.0, 0.5, 0.25, -0.4], [0.0, 0.0, 0.6, -0.3], [0.0, 0.0, 0.0, 0.0]),                   # the known answer of the CPU twin
    ]
    for e, (x, y, th) in enumerate(place):
        poses[e] = np.array([x, y, th], dtype=np.float32)
    sd["poses"] = torch.as_tensor(poses)
    env.load_state_dict(sd)
    obs = env.get_obs()
    torch.cuda.synchronize()
    P = env.poses.cpu()
    assert np.array_equal(P.numpy(), poses)
    zero = np.zeros((6, 4, 16), dtype=bool)
    zero[1, :2] = True                       # overlapping pair: every ray 0
    zero[3, [0, 2, 3]] = True                # outside the arena: every ray 0
    _check_against_twin(obs, P, env, max_degenerate=0.1, exact_zero=zero)
    lid = obs[..., env.lidar.offset:].cpu().numpy()
    assert lid[0, 0, 0] == pytest.approx(0.0 + (d - RHO), abs=2e-5)      # touching: the rim of the partner at 0.055
    assert lid[2, 0, 0] == pytest.approx(1.0 - RHO, abs=2e-5)            # along the line: the next robot 1.0 away
    assert lid[2, 2, 0] == pytest.approx(0.5 - RHO, abs=2e-5)            # robot 2 faces back (pi) toward robot 1
    assert lid[5, 0, 0] == pytest.approx(0.445, abs=2e-5)


PAIRS = [  # scenario, overrides: group widths 4, 8, 16
    ("Warehouse", {"n_agents": 4}),
    ("PredatorCapturePrey", {"predator": 3, "capture": 2, "n_agents": 5}),
    ("Simple", {"n_agents": 12, "start_dist": 0.2}),
]


def _run_pair(scenario, ov, R, solver, T=25, E=96):
    out = []
    for rays in (0, R):
        o = dict(ov, barrier_solver=solver)
        env = _env(scenario, E, rays, o, seed=7, auto_reset=True)
        obs0 = env.reset().clone()
        acts = _actions(env, T, seed=5)
        steps = []
        for t in range(T):
            obs, rew, done, info = env.step(acts[t])
            steps.append({"obs": obs.clone(), "reward": rew.clone(), "done": done.clone(),
                          **{k: v.clone() for k, v in info.items() if torch.is_tensor(v)}})
        torch.cuda.synchronize()
        out.append((env, obs0, steps, env.state_dict()))
    return out


@pytest.mark.parametrize("scenario,ov,solver", [(s, o, m) for s, o in PAIRS for m in ("exact", "cvxopt")
                                                 if m == "exact" or int(o["n_agents"]) <= 8])   # (cvxopt: n_agents <= 8)
def test_lidar_changes_nothing_else(scenario, ov, solver):
    lidar_changes_nothing_else(scenario, ov, solver)


def lidar_changes_nothing_else(scenario, ov, solver, **run):
    """run: _run_pair's T and E."""
    (off, o0, s_off, sd_off), (on, n0, s_on, sd_on) = _run_pair(scenario, ov, 16, solver, **run)
    own = off.D
    assert on.D == own + 16
    assert torch.equal(o0, n0[..., :own]) and not n0.any()
    done = 0
    for a, b in zip(s_off, s_on):
        assert torch.equal(a["obs"], b["obs"][..., :own])
        for k in a:
            if k != "obs":
                assert torch.equal(a[k], b[k]), k
        done += int(a["done"].sum())
    assert done > 0            # auto-reset was exercised
    for k in sd_off:
        assert torch.equal(sd_off[k], sd_on[k]), k


def test_paths_give_identical_lidar_blocks():
    """T single steps, rg_rollout over T steps and the gymma step_into path; get_obs after a non-resetting step."""
    scenario, R, T, E = "MaterialTransport", 16, 12, 50
    a = _env(scenario, E, R, seed=2, auto_reset=True)
    b = _env(scenario, E, R, seed=2, auto_reset=True)
    c = _env(scenario, E, R, seed=2, auto_reset=True)
    acts = _actions(a, T, seed=3)
    for env in (a, b, c):
        env.reset()
    singles = []
    for t in range(T):
        singles.append(a.step(acts[t])[0].clone())
    roll = b.rollout(acts)
    c.enable_time_limit(10 ** 6)
    batch = torch.zeros(T, E, c.N, c.D, device=c.device)
    rsum = torch.zeros(T, E, device=c.device)
    ended = torch.zeros(T, E, dtype=torch.uint8, device=c.device)
    for t in range(T):
        assert c.step_into(acts[t].data_ptr(), batch[t].data_ptr(), rsum[t].data_ptr(), ended[t].data_ptr()) == 0
    torch.cuda.synchronize()
    off = a.lidar.offset
    n_end = 0
    for t in range(T):
        assert torch.equal(singles[t], roll["obs"][t])
        live = ended[t] == 0
        assert torch.equal(singles[t][live], batch[t][live])
        assert not batch[t][~live].any()            # zero_obs_on_end: the lidar block too
        n_end += int((~live).sum())
        assert singles[t][..., off:].abs().sum() > 0
    assert n_end > 0
    # get_obs after a non-resetting step returns what the step returned
    d = _env(scenario, E, R, seed=2, auto_reset=False)
    d.reset()
    obs = d.step(acts[0])[0].clone()
    again = d.get_obs(torch.empty_like(obs))
    torch.cuda.synchronize()
    assert torch.equal(obs, again)


def test_batch_size_does_not_change_the_values():
    """env e at E = 37 and at E = 70 000, where the lidar-off handle picks the thread-per-env kernel."""
    scenario, R, T = "PredatorCapturePrey", 16, 3
    small, big = _env(scenario, 37, R, seed=4), _env(scenario, 70000, R, seed=4)
    assert small.step_kernel == "group" and big.step_kernel == "group"
    assert _env(scenario, 70000, 0, seed=4).step_kernel == "tpe"
    acts = _actions(big, T, seed=8)
    small.reset()
    big.reset()
    for t in range(T):
        o1 = small.step(acts[t, :37].contiguous())[0]
        o2 = big.step(acts[t])[0]
        torch.cuda.synchronize()
        assert torch.equal(o1, o2[:37])
    r = big.rollout(acts)
    assert r["obs"].shape[0] == T


def test_zero_rows_after_reference_reset():
    env = _env("Warehouse", 40, 8, seed=1, reference_reset_obs=True)
    obs = env.reset()
    torch.cuda.synchronize()
    assert obs.shape[-1] == env.D and not obs.any()
    env2 = _env("Warehouse", 40, 8, seed=1, reference_reset_obs=False)
    obs2 = env2.reset()
    torch.cuda.synchronize()
    assert obs2[..., env2.lidar.offset:].gt(0).all()     # the fresh observation carries ranges


def test_zero_obs_on_end_rows_are_zero_in_the_gymma_env():
    from marbler_amd.gymma import GymmaVecEnv
    v = GymmaVecEnv("robotarium_gym:Simple-v0", 64, time_limit=3, seed=2, overrides={"lidar_rays": 12, "lidar_range": 0.8})
    assert v.get_obs_size() == v.env.lidar.offset + 12 and v.get_state().shape == (64, v.n_agents * v.obs_size)
    v.reset()
    acts = _actions(v.env, 4, seed=1)
    for t in range(4):
        _, ended, _ = v.step(acts[t])
        obs = v.get_obs()
        torch.cuda.synchronize()
        if t == 2:
            assert ended.all()
        assert not obs[ended].any()
        if (~ended).any():
            live = obs[~ended][..., v.env.lidar.offset:]
            assert live.ge(0).all() and live.gt(0).any()


def test_guard_slabs_stay_untouched():
    """Observations inside a larger buffer at a ragged E: the launches write only their own slice."""
    scenario, E, T, R = "MaterialTransport", 37, 5, 8
    env = _env(scenario, E, R, seed=6)
    env.reset()
    N, D, dev = env.N, env.D, env.device
    G, sent = 4096, 1234.5
    acts = _actions(env, T, seed=2)
    # rg_get_obs
    buf = torch.full((E * N * D + 2 * G,), sent, device=dev)
    env.get_obs(buf[G:G + E * N * D].view(E, N, D))
    # rg_step via step_into (the gymma block) into a slab
    env.enable_time_limit(4)
    n = E * N * D                        # D = 17: a ragged row; every step's slice starts 16-byte aligned, 7 floats apart
    S = (n + 3) // 4 * 4 + 8
    ob = torch.full((T * S + 2 * G,), sent, device=dev)
    rb = torch.full((T * E + 2 * G,), sent, device=dev)
    eb = torch.full((T * E + 2 * G,), 7, dtype=torch.uint8, device=dev)
    for t in range(T):
        o = ob[G + t * S:G + t * S + n]
        assert env.step_into(acts[t].data_ptr(), o.data_ptr(), rb[G + t * E:].data_ptr(), eb[G + t * E:].data_ptr()) == 0
    torch.cuda.synchronize()
    written = torch.zeros_like(ob, dtype=torch.bool)
    for t in range(T):
        written[G + t * S:G + t * S + n] = True
    assert (ob[~written] == sent).all() and not (ob[written] == sent).all()
    for b, n in ((buf, E * N * D), (rb, T * E), (eb, T * E)):
        ref = torch.full((G,), 7 if b.dtype == torch.uint8 else sent, device=dev).to(b.dtype)
        assert torch.equal(b[:G], ref) and torch.equal(b[G + n:], ref)
        assert not torch.equal(b[G:G + n], torch.full((n,), 7 if b.dtype == torch.uint8 else sent, device=dev).to(b.dtype))


def test_batched_runner_two_launch_path_and_one_launch_refusal():
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    R, E, T = 16, 64, 8
    v = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", E, time_limit=5, seed=3,
                    overrides=dict(SCN_OV["PredatorCapturePrey"], lidar_rays=R))
    N, own = v.n_agents, v.env.lidar.offset
    assert v.obs_size == own + R
    actor = BatchedActor(_random_actor(1, own + R + N, 64, v.n_actions, True, seed=4), N, device=v.env.device)
    runner = BatchedRunner(v, actor, epsilon=0.1, seed=1)
    out = runner.run(T)
    torch.cuda.synchronize()
    assert out["obs"].shape == (T + 1, E, N, own + R)
    # replay the recorded actions on a twin env: its observations (zeros for ended envs) are the batch's, lidar columns included
    w = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", E, time_limit=5, seed=3,
                    overrides=dict(SCN_OV["PredatorCapturePrey"], lidar_rays=R))
    w.reset()
    for t in range(T):
        _, ended, _ = w.step(out["actions"][t])
        obs = w.get_obs()
        torch.cuda.synchronize()
        assert torch.equal(ended, out["terminated"][t])
        assert torch.equal(obs[..., own:], out["obs"][t + 1][..., own:])
        assert torch.equal(obs, out["obs"][t + 1])
    assert out["obs"][1:, ..., own:].gt(0).any()
    with pytest.raises(ValueError, match="lidar"):
        runner.run(T, one_launch=True)
