"""The lidar observation on the GPU (DESIGN.md "Lidar"): ranges against the float64 twin (tests/lidar_twin.py) from the poses the
GPU itself stored, non-interference with everything else a step computes (both harnesses: tests/lidar_harness.py), bit identity
across the paths that write it, zero rows, guard slabs, and the two-launch BatchedRunner."""
import numpy as np
import pytest
import torch

from gpu_helpers import random_actions as _actions, random_actor, runner_batch_replays
from lidar_harness import SCN_OV, check_against_twin as _check_against_twin, lidar_changes_nothing_else, make_env as _env, ranges_vs_twin

pytestmark = pytest.mark.gpu

RHO = float(np.float32(0.5) * np.float32(0.11))


@pytest.mark.parametrize("R", [4, 16, 32])
@pytest.mark.parametrize("scenario", sorted(SCN_OV))
def test_ranges_match_the_float64_twin(scenario, R):
    ranges_vs_twin(scenario, R)


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


@pytest.mark.parametrize("scenario,ov,solver", [(s, o, m) for s, o in PAIRS for m in ("exact", "cvxopt")
                                                 if m == "exact" or int(o["n_agents"]) <= 8])   # (cvxopt: n_agents <= 8)
def test_lidar_changes_nothing_else(scenario, ov, solver):
    lidar_changes_nothing_else(scenario, ov, solver)


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
    actor = BatchedActor(random_actor(1, own + R + N, 64, v.n_actions, True, seed=4), N, device=v.env.device)
    runner = BatchedRunner(v, actor, epsilon=0.1, seed=1)
    out = runner.run(T)
    torch.cuda.synchronize()
    assert out["obs"].shape == (T + 1, E, N, own + R)
    # replay the recorded actions on a twin env: its observations (zeros for ended envs) are the batch's, lidar columns included
    runner_batch_replays(out, "robotarium_gym:PredatorCapturePrey-v0", E, T, dict(SCN_OV["PredatorCapturePrey"], lidar_rays=R), slice(own, None))
    assert out["obs"][1:, ..., own:].gt(0).any()
    with pytest.raises(ValueError, match="lidar"):
        runner.run(T, one_launch=True)
