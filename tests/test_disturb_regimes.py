"""The sigma-bound cases of tests/test_gpu_disturb_forms.py reach the regime they are named for -- shown without a GPU.

The float32 oracle alone, free-running with the reset twin of tests/helpers.py, its poses displaced before every step by
tests/disturb_twin.py: the same configurations, seeds, batch, length and action tensor as the GPU cases (disturb_cases.py
REGIME_CASES), so -- the GPU being held to the oracle word for word there -- the same run.  At sigma (0.1, 0.5) a step starts
from robots inside each other's safety radius and outside the arena, and the barrier QP runs to its sweep limit; a zero scale
leaves its part of every pose alone, the sign of a zero included."""
import numpy as np
import pytest
import torch

from disturb_cases import ACTION_SEED, N_ACT, REGIME_CASES, SEED, Regime, check_regime
from disturb_twin import displace
from oracle_check import FreeRunningOracle

from marbler_amd.params import QP_MAX_SWEEPS, load_config, make_params


def oracle_alone(oracle_lib, scenario, ov, solver, sigma, E, T, episode_steps, seed=SEED, action_seed=ACTION_SEED):
    cfg = load_config(scenario, overrides=dict(ov, barrier_solver=solver, max_episode_steps=episode_steps))
    side = FreeRunningOracle(oracle_lib, scenario, cfg, E, make_params(scenario, cfg), seed)
    side.reset()
    orc = side.orc
    g = torch.Generator(device="cpu").manual_seed(action_seed)           # test_gpu_disturb.py _actions
    acts = torch.randint(0, N_ACT.get(scenario, 5), (T, E, orc.N), generator=g, dtype=torch.int32).numpy()
    r = Regime()
    for t in range(T):
        before = orc.poses.copy()
        orc.poses[...] = displace(before, seed, 0, side.episodes + 1, orc.steps, sigma[0], sigma[1])
        if sigma[0] == 0.0:
            assert np.array_equal(orc.poses[:, :2].view(np.uint32), before[:, :2].view(np.uint32))
        if sigma[1] == 0.0:
            assert np.array_equal(orc.poses[:, 2].view(np.uint32), before[:, 2].view(np.uint32))
        r.see_poses(before, orc.poses)
        obs, rew, done, info = orc.step(acts[t])
        r.see_step(done, info["violation"], orc.qp_sweeps)
        assert all(np.isfinite(a).all() for a in (obs, rew, info["dist_travelled"], orc.poses)), (t, "the oracle left the finite numbers")
        side.reset_ended()
    return r


@pytest.fixture(scope="module")
def regimes(oracle_lib):
    return {c[0]: oracle_alone(oracle_lib, *c[1:]) for c in REGIME_CASES}


@pytest.mark.parametrize("case", REGIME_CASES, ids=[c[0] for c in REGIME_CASES])
def test_the_case_reaches_its_regime(case, regimes):
    name, _, _, _, sigma, E, _, _ = case
    r = regimes[name]
    print(f"{name}: violations / max QP count / closest pair / outside / wrapped = {r.figures()}, episode ends {r.episode_ends}")
    check_regime(name, sigma, E, r)
    assert r.episode_ends >= E                       # what disturbed_vs_oracle asks of its run


def test_some_exact_mode_step_runs_the_qp_to_its_sweep_limit(regimes):
    """The limit the product builds its kernels' argument block with (marbler_amd/params.py) is the oracle's."""
    from oracle import c_oracle
    assert QP_MAX_SWEEPS == c_oracle.QP_MAX_SWEEPS["float32"] == 40
    exact = [regimes[c[0]].max_sweeps for c in REGIME_CASES if c[3] == "exact" and c[4][0] > 0.0]
    assert max(exact) == QP_MAX_SWEEPS and all(s <= QP_MAX_SWEEPS for s in exact), exact


def test_a_zero_scale_leaves_its_part_of_a_pose_alone_down_to_the_sign_of_a_zero():
    rng = np.random.RandomState(1)
    E, N = 64, 5
    poses = rng.uniform(-1, 1, (E, 3, N)).astype(np.float32)
    poses[::2] = np.float32(-0.0)
    poses[1::4] = np.float32(0.0)
    rc, st = rng.randint(1, 5, E), rng.randint(0, 30, E)
    xy_only = displace(poses, 9, 100, rc, st, 0.1, 0.0)
    th_only = displace(poses, 9, 100, rc, st, 0.0, 0.5)
    assert np.array_equal(xy_only[:, 2].view(np.uint32), poses[:, 2].view(np.uint32))
    assert np.array_equal(th_only[:, :2].view(np.uint32), poses[:, :2].view(np.uint32))
    assert (xy_only[:, :2] != poses[:, :2]).mean() > 0.9 and (th_only[:, 2] != poses[:, 2]).mean() > 0.9
