"""The free-running harnesses: an auto-resetting env on the GPU beside the float32 oracle with the reset twin.  What is compared,
and how, is tests/oracle_check.py's (`FreeRunningOracle`); here are the two drivers, their case tables, and the GPU-against-GPU
check of rg_rollout."""
import os

import numpy as np

from gpu_helpers import expected_slots
from oracle_check import FreeRunningOracle
from physical_cases import MT6, PCP5, PCP12, WH8

# tests/test_gpu_rollout.py (and tests/soak.py): scenario, overrides, action count, steps
ROLLOUT_CASES = [("PredatorCapturePrey", PCP5, 5, 260),
                 ("PredatorCapturePrey", {"num_neighbors": 2, "capability_aware": True}, 5, 120),
                 ("Warehouse", WH8, 5, 230),
                 ("Warehouse", {}, 5, 120),
                 ("MaterialTransport", MT6, 20, 160),
                 ("MaterialTransport", {}, 20, 100),
                 ("PredatorCapturePrey", PCP12, 5, 60),
                 ("PredatorCapturePrey", {"predator": 3, "capture": 2, "collision_variant": "center"}, 5, 150),
                 ("Warehouse", {"n_agents": 8, "barrier_certificate": "default"}, 5, 150),
                 ("PredatorCapturePrey", {"predator": 3, "capture": 2, "penalize_violations": False}, 5, 120),
                 ("MaterialTransport", {"capability_aware": True, "qp_max_sweeps": 6}, 20, 80),
                 ("PredatorCapturePrey", {"predator": 3, "capture": 2, "n_agents": 5, "num_prey": 12}, 5, 150),   # > 8 prey: LDS / loop paths
                 ("PredatorCapturePrey", {"predator": 2, "capture": 2, "n_agents": 4, "num_prey": 33, "step_dist": 0.16}, 5, 100),  # > 32 prey: both flag words
                 ("Simple", {}, 5, 130),
                 ("Simple", {"n_agents": 6}, 5, 80),
                 ("ArcticTransport", {}, 5, 200)]

# tests/test_gpu_baseline_shapes.py (and tests/soak_shapes.py):
# (id, scenario, overrides, action count, envs, steps, kernel, env slots per wave the lane-group dispatch must pick)
SHAPE_CASES = [
    ("pcp-4096x5-headline", "PredatorCapturePrey", PCP5, 5, 4096, 200, "group", 4),   # configs[1]: 1024 blocks, xcd_chunk
    ("pcp-2048x5", "PredatorCapturePrey", PCP5, 5, 2048, 120, "group", 2),
    ("pcp-8192x5", "PredatorCapturePrey", PCP5, 5, 8192, 120, "group", 8),
    ("pcp-32768x5", "PredatorCapturePrey", PCP5, 5, 32768, 90, "group", 8),           # configs[3] on one GPU
    ("pcp-4095x5-ragged", "PredatorCapturePrey", PCP5, 5, 4095, 100, "group", 4),
    ("pcp-2047x5-ragged", "PredatorCapturePrey", PCP5, 5, 2047, 100, "group", 2),
    ("pcp-8191x5-ragged", "PredatorCapturePrey", PCP5, 5, 8191, 100, "group", 8),
    ("pcp-1025x5-ragged", "PredatorCapturePrey", PCP5, 5, 1025, 100, "group", 2),
    ("warehouse-4096x8", "Warehouse", WH8, 5, 4096, 120, "group", 4),                  # configs[2]
    ("warehouse-8193x8-ragged", "Warehouse", WH8, 5, 8193, 110, "group", 8),
    ("mt-2048x6", "MaterialTransport", MT6, 20, 2048, 100, "group", 2),                # configs[4], per-GPU share
    ("mt-4096x6", "MaterialTransport", MT6, 20, 4096, 80, "group", 4),
    ("mt-4096x4-default", "MaterialTransport", {}, 20, 4096, 80, "group", 4),         # 4 lanes per env: 16 slots, 4 used
    ("pcp-4096x4-default", "PredatorCapturePrey", {}, 5, 4096, 100, "group", 4),
    ("arctic-16384x4", "ArcticTransport", {}, 5, 16384, 60, "group", None),           # fixed 16 envs per wave
    ("pcp-4096x5-tpe", "PredatorCapturePrey", PCP5, 5, 4096, 100, "tpe", None),        # thread-per-env, forced
    ("pcp-65536x5-auto", "PredatorCapturePrey", PCP5, 5, 65536, 40, None, None),      # the library picks thread-per-env
    ("mt-4094x6-tpe", "MaterialTransport", MT6, 20, 4094, 80, "tpe", None),             # ragged; E*N*D % 4 == 0 for rg_rollout
]


def rollout_bit_exact(scenario, ov, n_act, steps, oracle_lib, E, require_done=True, constants=None, after_step=None):
    """constants: the rps constants among `ov` (tests/physical_cases.py): both sides' parameter blocks are held to them, and to the
    defaults elsewhere, before the first step.  after_step(env, t): what a caller asserts about the launch (rg_step_form)."""
    import torch
    from marbler_amd import VecRobotariumEnv
    seed = 99
    env = VecRobotariumEnv(scenario, E, overrides=ov, seed=seed, auto_reset=True, collect_qp_stats=True)
    oracle = FreeRunningOracle(oracle_lib, scenario, dict(env.cfg), E, env.params, seed)
    if constants is not None:
        from physical_cases import check_constants
        check_constants(env.params, constants)
        check_constants(oracle.orc.p, constants)
    env.reset()
    oracle.reset()
    oracle.check_state(env, scenario, "reset")
    rng = np.random.RandomState(5)
    for t in range(steps):
        a = rng.randint(0, n_act, size=(E, env.N)).astype(np.int32)
        env.step(torch.as_tensor(a, device=env.device))
        oracle.step(a)
        oracle.check_step(env, scenario, t)
        if after_step is not None:
            after_step(env, t)
    assert oracle.n_done > 0 or E < 8 or not require_done
    oracle.check_statistics(env, scenario)
    env.close()


def fuzz_case_bit_exact(i, case, steps, oracle_lib, **kw):
    """case: a draw of tests/fuzz_cases.py; steps: (MaterialTransport's, everybody else's).  RG_STEP_KERNEL is the caller's business."""
    scenario, ov, n_act, E, kernel = case
    try:
        rollout_bit_exact(scenario, ov, n_act, steps[scenario != "MaterialTransport"], oracle_lib, E, require_done=False, **kw)
    except AssertionError as exc:
        raise AssertionError(f"case {i}: {scenario} {ov} E={E} kernel={kernel}: {exc}") from exc


def shape_rollout_vs_oracle(name, scenario, ov, n_act, E, steps, slots, oracle_lib, check_rollout=True, seed=1234, action_seed=17):
    """(RG_STEP_KERNEL is the caller's business.)  check_rollout=False: rg_step against the oracle only, no [K, ...] arrays
    (tests/soak_shapes.py runs thousands of steps this way)."""
    import torch
    from marbler_amd import VecRobotariumEnv
    kw = dict(overrides=ov, seed=seed, auto_reset=True, collect_qp_stats=True)
    env = VecRobotariumEnv(scenario, E, **kw)
    twin = VecRobotariumEnv(scenario, E, **kw) if check_rollout else None  # rg_rollout
    N = env.N
    if slots is not None:
        assert expected_slots(N, E) == slots, "the case no longer exercises the dispatch width it is named for"
    oracle = FreeRunningOracle(oracle_lib, scenario, dict(env.cfg), E, env.params, seed, threads=max(1, min(16, (os.cpu_count() or 1))))
    env.reset()
    if twin is not None:
        twin.reset()
    oracle.reset()
    oracle.check_state(env, name, "reset")
    rng = np.random.RandomState(action_seed)
    acts = rng.randint(0, n_act, size=(steps, E, N)).astype(np.int32) if check_rollout else None
    acts_dev = torch.as_tensor(acts, device=env.device) if check_rollout else None
    kept = {k: [] for k in ("obs", "reward", "done", "dist_travelled", "violation", "remaining", "qp_sweeps")}
    for t in range(steps):
        act_t = acts[t] if check_rollout else rng.randint(0, n_act, size=(E, N)).astype(np.int32)
        obs, rew, done, info = env.step(acts_dev[t] if check_rollout else torch.as_tensor(act_t, device=env.device))
        oracle.step(act_t)
        if check_rollout:
            got = {"obs": obs, "reward": rew, "done": env.done_u8, "dist_travelled": info["dist_travelled"],
                   "violation": info["violation"], "remaining": info["remaining"], "qp_sweeps": env.qp_sweeps}
            for k_, v in got.items():
                kept[k_].append(v.clone())
        oracle.check_step(env, name, t)
    assert oracle.n_done > 0 and oracle.n_viol > 0, "the rollout must contain episode ends and violations"
    oracle.check_statistics(env, name)
    if not check_rollout:
        env.close()
        return {"env_steps": steps * E, "episodes": int(oracle.episodes.sum()), "violations": oracle.n_viol}
    # ---- the same action sequence through rg_rollout (one launch for all steps): what the oracle just confirmed, step by step
    out = twin.rollout(acts_dev)
    for k_ in kept:
        ref = torch.stack(kept[k_])
        assert torch.equal(out[k_].view(ref.dtype) if out[k_].dtype != ref.dtype else out[k_], ref), f"{name}: rg_rollout {k_}"
    sa, sb = env.state_dict(), twin.state_dict()
    for key in sa:
        assert torch.equal(sa[key], sb[key]), f"{name}: rg_rollout state {key}"
    env.close()
    twin.close()


def rollout_equals_steps(scenario, ov, n_act, E, K=48, reps=3, require_done=True):
    """rg_rollout (K steps in one launch) against K rg_step launches, GPU against GPU: every per-step output and the final state."""
    import torch
    from marbler_amd import VecRobotariumEnv
    a = VecRobotariumEnv(scenario, E, overrides=ov, seed=21)
    b = VecRobotariumEnv(scenario, E, overrides=ov, seed=21)
    g = torch.Generator(device=a.device)
    g.manual_seed(4)
    a.reset()
    b.reset()
    for rep in range(reps):   # several launches of K steps: the state carries over between launches
        acts = torch.randint(0, n_act, (K, E, a.N), generator=g, device=a.device, dtype=torch.int32)
        out = a.rollout(acts)
        for k in range(K):
            obs, rew, done, info = b.step(acts[k])
            assert torch.equal(out["obs"][k].view(torch.int32), obs.view(torch.int32)), (rep, k)
            assert torch.equal(out["reward"][k].view(torch.int32), rew.view(torch.int32)), (rep, k)
            assert torch.equal(out["done"][k].bool(), done), (rep, k)
            assert torch.equal(out["dist_travelled"][k].view(torch.int32), info["dist_travelled"].view(torch.int32))
            assert torch.equal(out["violation"][k], info["violation"]) and torch.equal(out["remaining"][k], info["remaining"])
    sa, sb = a.state_dict(), b.state_dict()
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key
    assert torch.equal(a.done_count, b.done_count) and (int(a.done_count.sum()) > 0 or not require_done)
    assert torch.equal(a.done_return_sum.view(torch.int32), b.done_return_sum.view(torch.int32))
    a.close()
    b.close()
