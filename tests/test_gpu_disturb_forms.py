"""Every pose-disturbance kernel held to the float32 oracle (DESIGN.md "Pose disturbance"), in every form it is launched in.

1. Every (scenario, group width, solver) triple the library ships (disturb_cases.py FORM_CASES; tests/test_disturb_forms_cases.py
   matches the table against the shipped kernel names): the single step against the oracle stepped from the pose the twin
   displaces, the same actions through one rg_rollout launch against those steps, and the gymma step against the composed one.
2. The same body at the bounds the ABI admits, sigma (0.1, 0.5), and with one sigma zero: steps that start from robots inside
   each other's safety radius and outside the arena, barrier QPs at their sweep limit (tests/test_disturb_regimes.py shows on
   the CPU that the inputs get there).
3. Several envs per wavefront: 4, 8 and 16 env slots, both solver modes, through an auto-reset inside the shared wave.
4. The high words of the draw's counter and key: an env offset and a seed beyond 2^32.
Every comparison is word for word (tests/oracle_check.py)."""
import pytest
import torch

from disturb_cases import BOUNDS, FORM_CASES, N_ACT, PCP5, REGIME_CASES, check_regime
from disturb_harness import OUT_KEYS, disturbed_vs_oracle, make_env as _env, noise as _noise, oracle_step as _oracle_step, plain_oracle
from gpu_helpers import (expected_slots, fused_time_limit_vs_composed, random_actions as _actions, rollout_equals_single_steps,
                         same_bits as _same)
from oracle_check import assert_outputs, assert_state, gpu_outputs, gpu_state as _gpu_state
from physical_cases import PCP12

from marbler_amd.params import QP_MAX_SWEEPS

pytestmark = pytest.mark.gpu

ROLLOUT_KEY = {"done_u8": "done"}


def rollout_equals_steps(scenario, ov, solver, E, episode_steps, run, sigma=(0.01, 0.05), seed=13, env_offset=0):
    """A second handle with the same seed and reset, `run`'s actions (disturbed_vs_oracle) through one rg_rollout launch: every
    [K, ...] output equals the stacked step outputs the oracle confirmed, every state_dict entry the stepped handle's."""
    env = _env(scenario, E, dict(ov, barrier_solver=solver, max_episode_steps=episode_steps), sigma=sigma, seed=seed,
               env_offset=env_offset, collect_qp_stats=True)
    assert env.disturbance is not None and env.step_kernel == "group"
    env.reset()
    out = env.rollout(run["actions"])
    for k, ref in run["steps"].items():
        assert _same(out[ROLLOUT_KEY.get(k, k)], ref), f"{scenario} {solver}: rg_rollout {k}"
    state = env.state_dict()
    assert set(state) == set(run["state"])
    for k, ref in run["state"].items():
        assert _same(state[k], ref), f"{scenario} {solver}: rg_rollout state {k}"
    env.close()


def steps_then_rollout(scenario, ov, solver, E, T, episode_steps, oracle_lib, sigma=(0.01, 0.05)):
    run = disturbed_vs_oracle(scenario, ov, solver, E, T, oracle_lib, episode_steps=episode_steps, sigma=sigma)
    rollout_equals_steps(scenario, ov, solver, E, episode_steps, run, sigma=sigma)
    return run["regime"]


# ---------------------------------------------------------------- 1. every triple, in all three launch forms
@pytest.mark.parametrize("name,scenario,ov,solver,kinds", FORM_CASES, ids=[c[0] for c in FORM_CASES])
def test_every_shipped_kernel_in_its_three_launch_forms(name, scenario, ov, solver, kinds, oracle_lib):
    """A ragged batch at one env per wave: 67 envs, 12 steps of 5-step episodes (exact), 35 envs, 6 steps of 3-step episodes
    (interior point); the gymma step under a 9-step time limit, shorter than every scenario's own episode."""
    assert tuple(kinds) == ("step", "rollout", "gymma")
    E, T, ep = (67, 12, 5) if solver == "exact" else (35, 6, 3)
    steps_then_rollout(scenario, ov, solver, E, T, ep, oracle_lib)
    extra = {"barrier_solver": "cvxopt"} if solver == "cvxopt" else {}
    fused_time_limit_vs_composed(f"robotarium_gym:{scenario}-v0", dict(ov, **extra, **_noise((0.01, 0.05))), N_ACT.get(scenario, 5), 9, 67, 24)


# ---------------------------------------------------------------- 2. the admitted bounds and one-sided sigma
_regimes = {}     # case id -> the Regime of its run, kept for the sweep-limit test over the exact-mode cases together


def _regime_at_the_bounds(case, oracle_lib):
    name, scenario, ov, solver, sigma, E, T, ep = case
    if name not in _regimes:
        _regimes[name] = steps_then_rollout(scenario, ov, solver, E, T, ep, oracle_lib, sigma=sigma)
    return _regimes[name]


@pytest.mark.parametrize("case", REGIME_CASES, ids=[c[0] for c in REGIME_CASES])
def test_steps_and_rollout_at_the_sigma_bounds(case, oracle_lib):
    """The conditions (disturb_cases.check_regime) are computed from the oracle's outputs and the twin's poses."""
    name, sigma, E = case[0], case[4], case[5]
    r = _regime_at_the_bounds(case, oracle_lib)
    print(f"{name}: violations / max QP count / closest pair / outside / wrapped = {r.figures()}")
    check_regime(name, sigma, E, r)


def test_some_exact_mode_step_runs_the_qp_to_its_sweep_limit(oracle_lib):
    """Over the exact-mode cases above (runs them where they have not run): the oracle's counts, which the GPU's equal."""
    sweeps = {c[0]: _regime_at_the_bounds(c, oracle_lib).max_sweeps for c in REGIME_CASES if c[3] == "exact" and c[4] == BOUNDS}
    assert len(sweeps) == 5 and max(sweeps.values()) == QP_MAX_SWEEPS == 40, sweeps


@pytest.mark.parametrize("sigma", [(0.1, 0.0), (0.0, 0.5)], ids=["xy-only", "theta-only"])
def test_a_zero_scale_leaves_signed_zeros_alone(sigma, oracle_lib):
    """Stored poses holding -0.0 and +0.0: the step equals the oracle's from the twin's pose, whose zero-scaled part is the
    stored words (tests/test_disturb_regimes.py) -- x + 0 * c would have made a -0.0 a +0.0."""
    E = 67
    env = _env("PredatorCapturePrey", E, PCP5, sigma=sigma, seed=4, auto_reset=False, collect_qp_stats=True)
    orc = plain_oracle(oracle_lib, env)
    env.reset()
    env.poses[0::3, 2, :] = -0.0                 # headings; one agent's x, another's y (no two robots on one spot)
    env.poses[1::3, 2, :] = 0.0
    env.poses[0::2, 0, 0] = -0.0
    env.poses[1::2, 1, 1] = -0.0
    assert int((env.poses.view(torch.int32) == -2 ** 31).sum()) > E
    acts = _actions(env, 1, seed=6)
    pre, rc = _gpu_state(env), env.reset_count.cpu().numpy()
    env.step(acts[0])
    _oracle_step(orc, env, pre, rc, acts[0].cpu().numpy(), sigma=sigma)
    assert_outputs(gpu_outputs(env), orc, "signed zeros")
    assert_state(_gpu_state(env), orc, label="signed zeros")      # auto_reset off: every env, ended or not
    env.close()


# ---------------------------------------------------------------- 3. several envs per wavefront
PCP4_DEFAULT = {}                                                     # the shipped YAML: 4 agents, 4 lanes per env
# (id, overrides, solver, envs, sigma, env slots per wave)
WAVE_CASES = [
    ("2049x5", PCP5, "exact", 2049, (0.01, 0.05), 4),
    ("4097x4", PCP4_DEFAULT, "exact", 4097, (0.01, 0.05), 8),
    ("8193x4", PCP4_DEFAULT, "exact", 8193, (0.01, 0.05), 16),         # every lane group of the wave is a different env
    ("2049x12", PCP12, "exact", 2049, (0.01, 0.05), 4),                # 16 lanes per env: 4 slots = a full wave
    ("2049x5-bounds", PCP5, "exact", 2049, BOUNDS, 4),                 # the envs of a wave leave the QP at very different counts
    ("ipm-2049x5", PCP5, "cvxopt", 2049, (0.01, 0.05), 4),
    ("ipm-4097x4", PCP4_DEFAULT, "cvxopt", 4097, (0.01, 0.05), 8),
]


@pytest.mark.parametrize("name,ov,solver,E,sigma,slots", WAVE_CASES, ids=[c[0] for c in WAVE_CASES])
def test_three_steps_of_envs_sharing_a_wave_vs_the_oracle(name, ov, solver, E, sigma, slots, oracle_lib):
    """Two-step episodes: the third step runs after an auto-reset inside the shared wave, keyed by a new (episode, step)."""
    assert expected_slots(int(ov.get("n_agents", 4)), E) == slots, "the case no longer exercises the dispatch width it is named for"
    disturbed_vs_oracle("PredatorCapturePrey", ov, solver, E, 3, oracle_lib, episode_steps=2, seed=17, sigma=sigma)


@pytest.mark.parametrize("solver", ["exact", "cvxopt"])
def test_a_rollout_of_envs_sharing_a_wave_equals_the_steps(solver):
    E, K = 2049, 4
    assert expected_slots(5, E) == 4
    ov = dict(PCP5, barrier_solver=solver, max_episode_steps=2)
    s, r = _env("PredatorCapturePrey", E, ov, seed=21), _env("PredatorCapturePrey", E, ov, seed=21)
    s.reset()
    r.reset()
    out = rollout_equals_single_steps(s, r, _actions(s, K, seed=6))
    assert int(out["done"].sum()) >= E
    s.close()
    r.close()


# ---------------------------------------------------------------- 4. the high words of the stream
def test_env_offset_and_seed_beyond_32_bits_vs_the_oracle(oracle_lib):
    """include/robogym.h: env_offset is an int64_t, the seed a uint64_t; the draw's counter carries the offset's high word and
    its key the seed's (the twin's dependence on both is tests/test_disturb_config.py's)."""
    disturbed_vs_oracle("PredatorCapturePrey", PCP5, "exact", 67, 12, oracle_lib, seed=2 ** 32 + 13, env_offset=2 ** 32 + 7)


def test_a_shard_across_the_2_to_the_32_boundary_reproduces_its_envs():
    T = 8
    ov = dict(PCP5, max_episode_steps=5)
    one = _env("PredatorCapturePrey", 16, ov, seed=9, env_offset=2 ** 32 - 8)
    part = _env("PredatorCapturePrey", 8, ov, seed=9, env_offset=2 ** 32)
    low = _env("PredatorCapturePrey", 8, ov, seed=9, env_offset=0)      # what a dropped high word would make of `part`
    assert one.env_offset == 2 ** 32 - 8 and part.env_offset == 2 ** 32
    for env in (one, part, low):
        env.reset()
    assert not _same(part.poses, low.poses)
    acts = _actions(one, T, seed=8)
    for t in range(T):
        one.step(acts[t])
        part.step(acts[t][8:].contiguous())
        for k in OUT_KEYS + ("poses",):
            assert _same(getattr(one, k)[8:], getattr(part, k)), (t, k)
    for env in (one, part, low):
        env.close()
