"""rg_policy_rollout: T time steps of actor -> action -> env step in ONE launch must give, bit for bit, what the two-launch path
(the actor launch, then the env step launch, T times) gives: the transition batch, the hidden state, the episode statistics and the
env state."""
import pytest
import torch

from gpu_helpers import random_actor, runners_agree as _assert_same

pytestmark = pytest.mark.gpu

CONFIGS = [  # key, overrides, agents, hidden, shared actor
    ("robotarium_gym:PredatorCapturePrey-v0", None, 4, 128, True),
    ("robotarium_gym:PredatorCapturePrey-v0", {"predator": 3, "capture": 2, "n_agents": 5}, 5, 64, True),
    ("robotarium_gym:Warehouse-v0", {"n_agents": 8}, 8, 128, True),
    ("robotarium_gym:MaterialTransport-v0", {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25}, 6, 64, True),
    ("robotarium_gym:Simple-v0", None, 4, 64, True),
    ("robotarium_gym:ArcticTransport-v0", None, 4, 128, False),
    ("robotarium_gym:PredatorCapturePrey-v0", {"predator": 6, "capture": 6, "n_agents": 12, "num_prey": 10, "start_dist": 0.25,
                                               "num_neighbors": 4}, 12, 64, True),
]


def _runner(key, ov, E, H, shared, epsilon, limit=12, pack_gru=True):
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    v = GymmaVecEnv(key, E, time_limit=limit, seed=5, overrides=ov)
    N = v.n_agents
    actor = BatchedActor(random_actor(1 if shared else N, v.obs_size + N, H, v.n_actions, True, seed=4), N, device=v.env.device,
                         pack_gru=pack_gru)
    return v, BatchedRunner(v, actor, epsilon=epsilon, seed=9)


@pytest.mark.parametrize("epsilon", [0.0, 0.1])
@pytest.mark.parametrize("key,ov,N,H,shared", CONFIGS)
def test_one_launch_equals_two_launches(key, ov, N, H, shared, epsilon):
    E, T = 100, 40
    (v1, a), (v2, b) = _runner(key, ov, E, H, shared, epsilon), _runner(key, ov, E, H, shared, epsilon)
    assert v1.n_agents == N
    x, y = a.run(T), b.run(T, one_launch=True)
    for k in x:
        assert torch.equal(x[k], y[k]), k
    assert int(x["terminated"].sum()) > 0
    _assert_same((v1, a), (v2, b))


@pytest.mark.parametrize("E,T", [(1, 1), (17, 3), (1000, 5), (33, 150)])
def test_ragged_batches_and_lengths(E, T):
    key, ov = "robotarium_gym:PredatorCapturePrey-v0", {"predator": 3, "capture": 2, "n_agents": 5}
    (v1, a), (v2, b) = _runner(key, ov, E, 128, True, 0.1), _runner(key, ov, E, 128, True, 0.1)
    x, y = a.run(T), b.run(T, one_launch=True)
    for k in x:
        assert torch.equal(x[k], y[k]), k
    _assert_same((v1, a), (v2, b))


def test_mixed_calls_continue_the_same_episodes():
    key = "robotarium_gym:Warehouse-v0"
    (v1, a), (v2, b) = _runner(key, {"n_agents": 8}, 70, 64, True, 0.1), _runner(key, {"n_agents": 8}, 70, 64, True, 0.1)
    for T, one in ((9, True), (5, False), (13, True)):
        x, y = a.run(T), b.run(T, one_launch=one)
        for k in x:
            assert torch.equal(x[k], y[k]), (T, k)
    _assert_same((v1, a), (v2, b))


@pytest.mark.parametrize("scenario,ov,H", [("PredatorCapturePrey", None, 128), ("MaterialTransport", None, 64),
                                           ("ArcticTransport", None, 128)])
def test_run_eval_one_launch_equals_fused(scenario, ov, H):
    from marbler_amd.evaluate import BatchedActor, run_eval
    from marbler_amd.vec_env import VecRobotariumEnv
    outs, envs = [], []
    for one in (False, True):
        env = VecRobotariumEnv(scenario, 130, seed=3, overrides=ov)
        actor = BatchedActor(random_actor(1, env.D + env.N, H, 20 if scenario == "MaterialTransport" else 5, True, seed=2), env.N,
                             device=env.device)
        outs.append(run_eval(env, actor, 150, fused=True, one_launch=one))
        envs.append(env)
    assert outs[0] == outs[1] and outs[0]["episodes"] > 0
    s1, s2 = envs[0].state_dict(), envs[1].state_dict()
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k
    assert torch.equal(envs[0].obs, envs[1].obs) and torch.equal(envs[0].done_u8, envs[1].done_u8)


def test_refusals():
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    key = "robotarium_gym:PredatorCapturePrey-v0"
    _, r = _runner(key, {"barrier_solver": "cvxopt"}, 8, 64, True, 0.0)
    with pytest.raises(ValueError, match="interior-point"):
        r.run(2, one_launch=True)
    _, r = _runner(key, None, 8, 64, True, 0.0, pack_gru="bf16x3")
    with pytest.raises(ValueError, match="binary16"):
        r.run(2, one_launch=True)
    v = GymmaVecEnv(key, 8, time_limit=10, seed=1)
    actor = BatchedActor(random_actor(1, v.obs_size + v.n_agents, 64, v.n_actions, True, seed=4), v.n_agents, device=v.env.device)
    with pytest.raises(ValueError, match="inputs per agent"):
        BatchedRunner(v, actor, obs_agent_id=False).run(2, one_launch=True)


def test_guard_slabs_stay_untouched():
    """Every output and the hidden state sit inside a larger buffer: the launch writes only its own slice (ragged E)."""
    from marbler_amd.evaluate import policy_rollout
    key, E, T = "robotarium_gym:MaterialTransport-v0", 37, 6
    v, r = _runner(key, None, E, 64, True, 0.1)
    N, D, H, dev = v.n_agents, v.obs_size, 64, v.env.device
    G, sent = 4096, 1234.5

    def slab(n, dtype=torch.float32):
        buf = torch.full((n + 2 * G,), sent, device=dev).to(dtype) if dtype != torch.float32 else torch.full((n + 2 * G,), sent, device=dev)
        return buf, buf[G:G + n]
    hb, hidden = slab(E * N * H)
    hidden.zero_()
    ab, actions = slab(T * E * N, torch.int32)
    ob, obs = slab((T + 1) * E * N * D)
    obs[:E * N * D].zero_()
    rb, rew = slab(T * E)
    eb, ended = slab(T * E, torch.uint8)
    db, dist = slab(E * N)
    dist.zero_()
    u = torch.rand(T, E, N, device=dev)
    policy_rollout(v.env, r.actor, T, v.env._io_into, hidden, actions, restart=r._restart, explore_u=u, epsilon=0.1,
                   obs=obs, reward_sum=rew, ended=ended, dist_sum=dist)
    torch.cuda.synchronize()
    for b, n in ((hb, E * N * H), (ab, T * E * N), (ob, (T + 1) * E * N * D), (rb, T * E), (eb, T * E), (db, E * N)):
        ref = torch.full((G,), sent, device=dev).to(b.dtype)
        assert torch.equal(b[:G], ref) and torch.equal(b[G + n:], ref)
