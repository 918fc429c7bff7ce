"""The lidar family's env constructor and its two harnesses -- ranges against the float64 twin (tests/lidar_twin.py) and
non-interference with everything else a step computes -- shared by tests/test_gpu_lidar.py, tests/test_gpu_shared_waves.py and
tests/test_gpu_physical_constants.py."""
import numpy as np
import torch

from gpu_helpers import random_actions
from lidar_twin import bounds_of, lidar_batch

SCN_OV = {  # every scenario, with the agent counts of the benchmark configurations where they differ from the YAML
    "PredatorCapturePrey": {"predator": 3, "capture": 2, "n_agents": 5},
    "Warehouse": {"n_agents": 8},
    "MaterialTransport": {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25},
    "Simple": {},
    "ArcticTransport": {},
}


def make_env(scenario, E, R, ov=None, L=1.0, **kw):
    from marbler_amd.vec_env import VecRobotariumEnv
    o = dict(SCN_OV.get(scenario, {}), **(ov or {}))
    if R:
        o.update(lidar_rays=R, lidar_range=L)
    return VecRobotariumEnv(scenario, E, overrides=o, device="cuda:0", **kw)


def check_against_twin(obs, poses, env, L=1.0, max_degenerate=1e-3, exact_zero=None):
    """obs [E, N, D] (device), poses [E, 3, N] the stored poses the step built it from.  Returns the number of rays compared."""
    R, off = int(env.lidar.rays), int(env.lidar.offset)
    got = obs[..., off:off + R].double().cpu().numpy()
    rho = float(np.float32(0.5) * np.float32(env.params.robot_diameter))   # (0.055 at the default constants)
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


def ranges_vs_twin(scenario, R, E=256, T=4, ov=None):
    env = make_env(scenario, E, R, ov, seed=3, auto_reset=False)
    assert env.D == env.lidar.offset + R and env.step_kernel == "group"
    env.reset()
    # random headings: the reset's are axis-aligned, and robots on the grid row y = 0 then sit exactly L = 1 m from the side
    # walls on two of their rays (a degenerate ray for any binary32 evaluation)
    sd = env.state_dict()
    g = torch.Generator(device="cpu").manual_seed(R)
    sd["poses"][:, 2, :] = (torch.rand(env.E, env.N, generator=g) * 2.0 - 1.0) * 3.14159
    env.load_state_dict(sd)
    acts = random_actions(env, T, seed=11)
    compared = 0
    for t in range(T):
        obs, _, _, _ = env.step(acts[t])
        torch.cuda.synchronize()
        compared += check_against_twin(obs, env.poses, env)
    assert compared > 0.99 * T * env.E * env.N * R


def _run_pair(scenario, ov, R, solver, T=25, E=96):
    out = []
    for rays in (0, R):
        o = dict(ov, barrier_solver=solver)
        env = make_env(scenario, E, rays, o, seed=7, auto_reset=True)
        obs0 = env.reset().clone()
        acts = random_actions(env, T, seed=5)
        steps = []
        for t in range(T):
            obs, rew, done, info = env.step(acts[t])
            steps.append({"obs": obs.clone(), "reward": rew.clone(), "done": done.clone(),
                          **{k: v.clone() for k, v in info.items() if torch.is_tensor(v)}})
        torch.cuda.synchronize()
        out.append((env, obs0, steps, env.state_dict()))
    return out


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
