"""The 16-lane-row step kernels (step_group.h, step_once SPAN) read every argument behind the sub-step loop -- output and state
addresses, reward parameters, the flags of the store block, of the drawn-ahead copy and of the auto-reset -- from a copy of the
argument block held in vector registers.  Against the 8-lane-group kernels (RG_STEP_SPAN=0 at rg_create), which read the block
as before: all six outputs (and `qp_sweeps` where it is collected) of every step and the full `state_dict`, word for word.

Batches 1, 1025 and 2049 = one, two and four envs per wave with a ragged last wave; 8 steps with `max_episode_steps` 3, so that
episodes end, the drawn-ahead copy starts the next one and the sampler redraws.  Every scenario with a row kernel, crossed with
the flags that select what the changed code reads: episode statistics bound or not, `shared_reward`, `qp_sweeps` bound or not,
`auto_reset`, `capability_aware`.  At 2049 envs the row-kernel env lives on the red-zone slab of tests/test_gpu_redzone.py (the
addresses of every store are formed differently), whose guard bytes must be intact after the run.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from gpu_helpers import ROW_STATE as STATE, STEP_OUTS as OUTS, expected_slots, guarded_class, lane_group_kernel  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

STEPS, MAX_EPISODE_STEPS = 8, 3
SLOTS = {1: 1, 1025: 2, 2049: 4}
CONFIGS = [("pcp-n5", "PredatorCapturePrey", {"predator": 3, "capture": 2, "n_agents": 5}, 5),
           ("pcp-n8", "PredatorCapturePrey", {"predator": 4, "capture": 4, "n_agents": 8}, 5),
           ("warehouse-n8", "Warehouse", {"n_agents": 8}, 5),
           ("mt-n6", "MaterialTransport", {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25}, 20),
           ("simple-n7", "Simple", {"n_agents": 7}, 5)]
FLAGS = ("stats", "shared_reward", "qp_stats", "auto_reset", "capability_aware")
CASES = [(c, E) for c in CONFIGS for E in SLOTS]


def _unbind_statistics(env):
    """The same state with the four statistics arrays unbound (rg_bind_state: all four or none)."""
    from marbler_amd import _lib
    ptrs = [t.data_ptr() for t in (env.poses, env.carry_dist, env.episode_steps, env.reset_count, env.prey_loc, env.prey_sensed,
                                   env.prey_captured, env.loaded, env.load, env.zone_load, env.messages, env.grid, env.goal_col,
                                   env.pixel_type, env.reached_goal)]
    st = _lib.RgState(*ptrs, None, None, None, None, env.next_init.data_ptr(), env.next_episode.data_ptr())
    _lib.check(env.lib.rg_bind_state(env._h, C.byref(st)), "rg_bind_state")


def _make(scenario, ov, E, span, flags, monkeypatch):
    from marbler_amd import VecRobotariumEnv
    kw = dict(overrides=ov, seed=7, auto_reset=flags["auto_reset"], collect_qp_stats=flags["qp_stats"])
    if span:
        monkeypatch.delenv("RG_STEP_SPAN", raising=False)
    else:
        monkeypatch.setenv("RG_STEP_SPAN", "0")
    if span and E == 2049:
        env = guarded_class()(scenario, E, slab_bytes=E * 8192 + (8 << 20), **kw)
    else:
        env = VecRobotariumEnv(scenario, E, **kw)
    monkeypatch.delenv("RG_STEP_SPAN", raising=False)
    if not flags["stats"]:
        _unbind_statistics(env)
    env.reset()
    assert env.step_kernel == "group"
    return env


def _words(env, step_result):
    """-> (one uint8 tensor, [bytes per array]): the step's outputs, byte for byte (left on the device)."""
    import torch
    obs, rew, done, info = step_result
    parts = [obs, rew, done, info["dist_travelled"], info["violation"], info["remaining"]]
    if env.qp_sweeps is not None:
        parts.append(env.qp_sweeps)
    return torch.cat([p.contiguous().view(torch.uint8).flatten() for p in parts]), [p.numel() * p.element_size() for p in parts]


def _first_difference(new, old, sizes, names):
    """(step, array name) of the first differing byte of the stacked per-step records."""
    diff = (new != old).nonzero()[0].tolist()
    bounds = np.cumsum(sizes)
    return diff[0], names[int(np.searchsorted(bounds, diff[1], side="right"))]


@pytest.mark.parametrize("config,E", CASES, ids=[f"{c[0]}-E{E}" for c, E in CASES])
def test_row_kernels_match_eight_lane_groups_under_every_flag(config, E, monkeypatch):
    import torch
    name, scenario, base, n_act = config
    rng = np.random.RandomState(11)
    acts = [rng.randint(0, n_act, size=(E, base["n_agents"])).astype(np.int32) for _ in range(STEPS)]
    ended = resets = 0
    for bits in itertools.product((True, False), repeat=len(FLAGS)):
        flags = dict(zip(FLAGS, bits))
        what = f"{name} E={E} " + " ".join(f"{k}={int(v)}" for k, v in flags.items())
        ov = dict(base, max_episode_steps=MAX_EPISODE_STEPS, shared_reward=flags["shared_reward"], capability_aware=flags["capability_aware"])
        new, old = (_make(scenario, ov, E, span, flags, monkeypatch) for span in (True, False))
        assert 5 <= new.N <= 8 and expected_slots(new.N, E) == SLOTS[E] <= 4, "the case no longer dispatches the row kernel"
        rec_new, rec_old = [], []
        for t in range(STEPS):
            a = torch.as_tensor(acts[t], device=new.device)
            w, sizes = _words(new, new.step(a))
            rec_new.append(w)
            rec_old.append(_words(old, old.step(a))[0])
        rec_new, rec_old = torch.stack(rec_new), torch.stack(rec_old)
        if not torch.equal(rec_new, rec_old):
            t, arr = _first_difference(rec_new, rec_old, sizes, OUTS)
            raise AssertionError(f"{what}: step {t}: {arr} differs")
        sd_new, sd_old = new.state_dict(), old.state_dict()
        assert set(STATE) <= set(sd_new) and sd_new.keys() == sd_old.keys()
        assert torch.equal(sd_new.pop("seed"), sd_old.pop("seed"))
        flat_new, flat_old = (torch.cat([v.view(torch.uint8).flatten() for v in sd.values()]) for sd in (sd_new, sd_old))
        if not torch.equal(flat_new, flat_old):   # (one comparison on the device; the key-by-key search only to name the culprit)
            raise AssertionError(f"{what}: state differs in {[k for k in sd_new if not torch.equal(sd_new[k], sd_old[k])]}")
        if E == 2049:
            bad = new.red_zones_intact()
            assert bad.size == 0, f"{what}: {bad.size} red-zone bytes damaged, first after `{new.owner_of(int(bad[0]))}`"
        if flags["auto_reset"]:
            resets += int(new.reset_count.max()) - 1
        ended += int(rec_new[:, sizes[0] + sizes[1]:sizes[0] + sizes[1] + sizes[2]].sum())
        new.close()
        old.close()
    # episodes ended in every run (the step limit), and with auto_reset on every env began its third episode
    assert ended > 0 and resets >= 16 * 2, (ended, resets)
