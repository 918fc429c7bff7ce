"""tests/oracle_check.py under test: the comparison every GPU tier states its oracle claim with must see one flipped bit in any
output, any state array it is asked to compare and either statistic, name the key and the env, and honour `rows`.

CPU part: two float32 oracles stepped alike with the reset twin, the second shown as "the GPU side" through a NumPy stand-in with
the product's attribute names.  GPU part: the free-running harness on a real env, and the same harness with one oracle-side action
changed -- it is wired to the env, not comparing the oracle with itself."""
import copy

import numpy as np
import pytest

import oracle_check as oc

E, STEPS, SEED = 8, 3, 7
CASES = [("PredatorCapturePrey", {"predator": 3, "capture": 2, "n_agents": 5}, 5), ("MaterialTransport", {}, 20), ("ArcticTransport", {}, 5)]


class StandIn(object):
    """The product's attribute names over copies of a free-running oracle's arrays."""

    def __init__(self, orc, side=None):
        for k, g in oc.OUTPUTS:
            setattr(self, g, getattr(orc, k).copy())
        for k in oc.STATE_KEYS:
            setattr(self, oc.GPU_NAME.get(k, k), getattr(orc, k).copy())
        if side is not None:
            self.done_count, self.reset_count = side.episodes.astype(np.int32), (side.episodes + 1).astype(np.int32)
            self.done_return_sum, self.ep_return = side.ret_sum.copy(), side.ret.copy()


def flip_lowest_bit(arr, e):
    arr[e:e + 1].reshape(-1).view(np.uint8)[0] ^= 1


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def sides(request, oracle_lib):
    """(the oracle side after STEPS steps, the stand-in of a second oracle stepped alike); two-step episodes, so the twin resets."""
    from marbler_amd.params import load_config, make_params
    scenario, ov, n_act = request.param
    cfg = load_config(scenario, None, dict(ov, max_episode_steps=2))
    a, b = (oc.FreeRunningOracle(oracle_lib, scenario, cfg, E, make_params(scenario, cfg), SEED) for _ in range(2))
    rng = np.random.RandomState(3)
    for side in (a, b):
        side.reset()
    for t in range(STEPS):
        acts = rng.randint(0, n_act, size=(E, a.orc.N)).astype(np.int32)
        a.step(acts)
        b.step(acts)
        a.check_step(StandIn(b.orc), scenario, t)
    assert a.n_done >= E and (a.ret_sum != 0).any()
    return a, StandIn(b.orc, b)


def test_unmodified_sides_agree(sides):
    oracle, env = sides
    oracle.check_step(env, "cpu", STEPS - 1)
    oracle.check_statistics(env, "cpu")
    assert set(oc.gpu_outputs(env)) == set(oc.OUTPUT_KEYS) and set(oracle.keys) <= set(oc.STATE_KEYS)
    without = copy.deepcopy(env)
    without.qp_sweeps = None                               # an env that does not collect it: the other six are still held
    assert "qp_sweeps" not in oc.gpu_outputs(without)
    oracle.check_step(without, "cpu", STEPS - 1)
    flip_lowest_bit(without.reward, 0)
    with pytest.raises(AssertionError, match="reward differs"):
        oracle.check_step(without, "cpu", STEPS - 1)


def test_one_flipped_bit_in_any_compared_array_is_named(sides):
    oracle, env = sides
    names = [(k, g) for k, g in oc.OUTPUTS] + [(k, oc.GPU_NAME.get(k, k)) for k in oracle.keys]
    assert len(names) == 7 + len(oracle.keys) >= 12
    for key, attr in names:
        bad = copy.deepcopy(env)
        flip_lowest_bit(getattr(bad, attr), 5)
        with pytest.raises(AssertionError, match=rf"cpu: {key} differs at step 2 in 1 envs, first \[5\]"):
            oracle.check_step(bad, "cpu", STEPS - 1)


def test_rows_select_the_envs_compared(sides):
    oracle, env = sides
    rows = np.array([0, 1, 2])
    for key, attr in [("obs", "obs"), ("remaining", "remaining"), ("poses", "poses"), ("steps", "episode_steps")]:
        check = oc.assert_outputs if key in oc.OUTPUT_KEYS else oc.assert_state
        get = oc.gpu_outputs if key in oc.OUTPUT_KEYS else oc.gpu_state
        outside, inside = copy.deepcopy(env), copy.deepcopy(env)
        flip_lowest_bit(getattr(outside, attr), 5)
        flip_lowest_bit(getattr(inside, attr), 1)
        check(get(outside), oracle.orc, label="rows", step=0, rows=rows)
        check(get(outside), oracle.orc, label="rows", step=0, rows=np.arange(E) < 3)
        with pytest.raises(AssertionError, match=rf"rows: {key} differs at step 0 in 1 envs, first \[5\]"):
            check(get(outside), oracle.orc, label="rows", step=0)
        for r in (rows, np.arange(E) < 3):
            with pytest.raises(AssertionError, match=rf"rows: {key} differs at step 0 in 1 envs, first \[1\]"):
                check(get(inside), oracle.orc, label="rows", step=0, rows=r)


def test_words_not_values():
    zero = np.zeros((4, 2), np.float32)
    oc.assert_same_words(zero, zero.copy(), "reward")
    minus = zero.copy()
    minus[2, 1] = -0.0
    assert (minus == zero).all()
    with pytest.raises(AssertionError, match=r"reward differs at step None in 1 envs, first \[2\]"):
        oc.assert_same_words(minus, zero, "reward")
    with pytest.raises(AssertionError, match=r"steps differs at step None in 10 envs, first \[0, 1, 2, 3, 4, 5, 6, 7\]$"):
        oc.assert_same_words(np.zeros(10, np.int32), np.ones(10, np.int32), "steps")


def test_statistics_are_held_word_for_word(sides):
    oracle, env = sides
    bad = copy.deepcopy(env)
    flip_lowest_bit(bad.done_return_sum, 5)
    with pytest.raises(AssertionError, match=r"done_return_sum differs at step end in 1 envs, first \[5\]"):
        oracle.check_statistics(bad, "cpu")
    bad = copy.deepcopy(env)
    bad.done_count[3] += 1
    with pytest.raises(AssertionError, match=r"done_count differs at step end in 1 envs, first \[3\]"):
        oracle.check_statistics(bad, "cpu")


@pytest.mark.gpu
def test_the_free_running_harness_is_wired_to_the_env(oracle_lib, monkeypatch):
    """PredatorCapturePrey 65 x 5 (a second, ragged wavefront), three steps: the harness passes; with one action of env 40 changed on
    the oracle's side only it fails, naming an output and env 40."""
    from rollout_harness import rollout_bit_exact
    monkeypatch.setenv("RG_STEP_KERNEL", "group")
    scenario, ov, n_act = CASES[0]
    rollout_bit_exact(scenario, ov, n_act, 3, oracle_lib, 65, require_done=False)

    class Tampered(oracle_lib.OracleVecEnv):
        def step(self, actions, threads=1):
            actions = np.array(actions)
            actions[40, 0] = (actions[40, 0] + 1) % n_act
            return super().step(actions, threads)

    class Lib(object):
        OracleVecEnv = Tampered

        def __getattr__(self, name):
            return getattr(oracle_lib, name)

    outputs = "|".join(oc.OUTPUT_KEYS)
    with pytest.raises(AssertionError, match=rf": ({outputs}) differs at step \d in 1 envs, first \[40\]"):
        rollout_bit_exact(scenario, ov, n_act, 3, Lib(), 65, require_done=False)
