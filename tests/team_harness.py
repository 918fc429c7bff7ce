"""The team pool's env constructor, its four-set pool and the loaded-state harness against the float32 oracle (what is compared:
tests/oracle_check.py), shared by tests/test_gpu_teams.py, tests/test_gpu_shared_waves.py and tests/test_gpu_physical_constants.py.
The draw's NumPy twin is tests/team_twin.py."""
import numpy as np
import torch

from gpu_helpers import random_actions
from oracle_check import assert_outputs, assert_state, gpu_outputs, gpu_state, load_oracle

SCN_OV = {"PredatorCapturePrey": {"predator": 3, "capture": 2, "n_agents": 5},
          "Warehouse": {"n_agents": 8},
          "MaterialTransport": {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25},
          "Simple": {}}


def make_env(scenario, E, ov=None, teams=None, sampling="episode", **kw):
    from marbler_amd.vec_env import VecRobotariumEnv
    o = dict(SCN_OV.get(scenario, {}), **(ov or {}))
    if teams is not None:
        o.update(teams=teams, team_sampling=sampling)
    return VecRobotariumEnv(scenario, E, overrides=o, device="cuda:0", **kw)


def pool4(scenario, N):
    """Four sets that differ in every capability of the scenario; set 3 gives agent 0 both radii 0."""
    r = np.random.RandomState(N)
    if scenario == "PredatorCapturePrey":
        sets = []
        for t, npred in enumerate((3 * N // 4, N // 2, N // 4, N // 2)):
            sr = [float(np.float32(0.3 + 0.1 * t)) if a < npred else 0.0 for a in range(N)]
            cr = [0.0 if a < npred else float(np.float32(0.15 + 0.05 * t)) for a in range(N)]
            sd = [float(np.float32(x)) for x in r.choice([0.12, 0.2, 0.3], N)]
            if t == 3:
                sr[0] = cr[0] = 0.0
            sets.append({"sensing_radius": sr, "capture_radius": cr, "step_dist": sd})
        return sets
    if scenario == "MaterialTransport":
        return [{"speed": [float(np.float32(x)) for x in r.choice([0.1, 0.2, 0.3], N)], "torque": [int(x) for x in r.randint(0, 12, N)]}
                for _ in range(4)]
    return [{"step_dist": [float(np.float32(x)) for x in r.choice([0.1, 0.2, 0.3, 0.4], N)]} for _ in range(4)]


def _load_set(orc, pool, t, N):
    for a in range(N):
        orc.p.agent_step[a] = float(pool.agent_step[t, a])
        orc.p.sensing_radius[a] = float(pool.sensing_radius[t, a])
        orc.p.capture_radius[a] = float(pool.capture_radius[t, a])
        orc.p.torque[a] = int(pool.torque[t, a])


def mixed_teams_vs_oracle(scenario, ov, solver, oracle_lib, E, T, episode_steps, before_first_step=None, threads=1):
    """Four oracles, one per set of `pool4`, each loaded with the GPU's state before every step; env e is held to the oracle of
    its own set.  before_first_step(env): called after the reset, for what a caller asserts about the draw.  threads: the oracles'."""
    ov = dict(ov, barrier_solver=solver, max_episode_steps=episode_steps)
    N = int(dict(SCN_OV[scenario], **ov).get("n_agents", 4))
    env = make_env(scenario, E, ov, teams=pool4(scenario, N), seed=11, auto_reset=False, collect_qp_stats=True)
    cfg = dict(env.cfg)
    cfg.pop("teams")
    cfg.pop("team_sampling")
    orcs = [oracle_lib.OracleVecEnv(scenario, cfg, E, dtype=np.float32) for _ in range(4)]
    for t in range(4):
        _load_set(orcs[t], env.teams, t, env.N)
    env.reset()
    if before_first_step is not None:
        before_first_step(env)
    acts = random_actions(env, T, seed=3).cpu().numpy()
    changes, seen = 0, set()
    for step in range(T):
        team = env.team_index.cpu().numpy()
        seen |= set(team.tolist())
        pre = gpu_state(env)
        env.step(torch.as_tensor(acts[step], device=env.device))
        outs, post = gpu_outputs(env), gpu_state(env)
        for t in range(4):
            rows = np.nonzero(team == t)[0]
            if rows.size == 0:
                continue
            load_oracle(orcs[t], pre)
            orcs[t].step(acts[step], threads=threads)
            assert_outputs(outs, orcs[t], f"{scenario} {solver} set {t}", step, rows)
            assert_state(post, orcs[t], label=f"{scenario} {solver} set {t}", step=step, rows=rows)
        done = env.done_u8.clone()
        if bool(done.any()):
            before = env.team_index.clone()
            env.reset(mask=done)
            changes += int((env.team_index != before).sum())
    assert seen == {0, 1, 2, 3} and changes > 0
    env.close()
