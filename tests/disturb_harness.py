"""The pose disturbance's env constructor and its loaded-state harness against the float32 oracle stepped from the pose the NumPy
twin (tests/disturb_twin.py) displaces; what is compared is tests/oracle_check.py's.  Shared by tests/test_gpu_disturb.py,
tests/test_gpu_disturb_forms.py and tests/test_gpu_physical_constants.py; the case tables are tests/disturb_cases.py."""
import os

import numpy as np
import torch

from disturb_cases import Regime
from disturb_twin import displace
from gpu_helpers import random_actions, same_bits
from oracle_check import OUTPUTS, assert_outputs, assert_state, gpu_outputs, gpu_state, load_oracle

SXY, STH = 0.01, 0.05
NOISE = {"pose_noise_xy": SXY, "pose_noise_theta": STH}
OUT_KEYS = tuple(g for _, g in OUTPUTS[:6])      # the product's names, without qp_sweeps (not every handle here collects it)
THREADS = max(1, min(16, os.cpu_count() or 1))


def noise(sigma):
    return {"pose_noise_xy": sigma[0], "pose_noise_theta": sigma[1]}


def make_env(scenario, E, ov=None, noisy=True, sigma=(SXY, STH), **kw):
    from marbler_amd.vec_env import VecRobotariumEnv
    return VecRobotariumEnv(scenario, E, overrides=dict(ov or {}, **(noise(sigma) if noisy else {})), device="cuda:0", **kw)


def plain_oracle(oracle_lib, env):
    """The oracle of the env's configuration without the disturbance (the twin displaces its poses)."""
    cfg = {k: v for k, v in env.cfg.items() if k not in NOISE}
    return oracle_lib.OracleVecEnv(env.scenario, cfg, env.E, dtype=np.float32)


def oracle_step(orc, env, pre, reset_count, acts, displaced=True, sigma=(SXY, STH), regime=None):
    """The oracle loaded with the GPU's state `pre`, its poses displaced by the twin, stepped with `acts`.  `regime`
    (disturb_cases.Regime) is shown the stored and the displaced poses."""
    load_oracle(orc, pre)
    if displaced:
        orc.poses[...] = displace(pre["poses"], env.seed, env.env_offset, reset_count, pre["steps"], sigma[0], sigma[1])
        if regime is not None:
            regime.see_poses(pre["poses"], orc.poses)
    return orc.step(acts, threads=THREADS)


def check_step(env, orc, label, step=None):
    """Every output, and the stored state of the envs that did not end (the others were reset, or hold their terminal state)."""
    assert_outputs(gpu_outputs(env), orc, label, step)
    assert_state(gpu_state(env), orc, label=label, step=step, rows=np.nonzero(orc.done == 0)[0])


def disturbed_vs_oracle(scenario, ov, solver, E, T, oracle_lib, episode_steps=5, seed=13, env_offset=0, sigma=(SXY, STH)):
    """Every step: the GPU's state before the step into the oracle, the oracle's poses displaced by the twin, one step of each;
    every word of the outputs (the QP's sweep or iteration count among them) and -- for envs that did not end (the others were
    reset) -- of the stored state.  Returns what it collected: the actions [T, E, N], every output stacked over the steps
    (`steps`), the stepped handle's final `state_dict` and the oracle's counts (`regime`, a disturb_cases.Regime)."""
    ov = dict(ov, barrier_solver=solver, max_episode_steps=episode_steps)
    env = make_env(scenario, E, ov, sigma=sigma, seed=seed, env_offset=env_offset, collect_qp_stats=True)
    plain = make_env(scenario, E, ov, noisy=False, seed=seed, env_offset=env_offset)
    assert env.disturbance is not None and plain.disturbance is None and env.step_kernel == "group"
    orc = plain_oracle(oracle_lib, env)
    env.reset()
    plain.reset()
    assert same_bits(env.poses, plain.poses)
    acts = random_actions(env, T, seed=3)
    acts_np = acts.cpu().numpy()
    regime = Regime()
    kept = {k: [] for k in OUT_KEYS + ("qp_sweeps",)}
    for t in range(T):
        pre, rc = gpu_state(env), env.reset_count.cpu().numpy()
        env.step(acts[t])
        plain.step(acts[t])
        _, _, o_done, o_info = oracle_step(orc, env, pre, rc, acts_np[t], sigma=sigma, regime=regime)
        regime.see_step(o_done, o_info["violation"], orc.qp_sweeps)
        for k in kept:
            kept[k].append(getattr(env, k).clone())
        check_step(env, orc, f"{scenario} {solver}", t)
    assert regime.episode_ends >= E, "every env ends at least one episode inside the run (the draw's episode and step both move)"
    assert not same_bits(env.poses, plain.poses) and not same_bits(env.obs, plain.obs), "the disturbance changed nothing"
    result = {"actions": acts, "steps": {k: torch.stack(v) for k, v in kept.items()}, "state": env.state_dict(), "regime": regime}
    env.close()
    plain.close()
    return result
