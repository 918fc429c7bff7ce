"""The launch plan (csrc/launch_plan.h) on the device: rg_step_form reports the plan that selected the kernel, so a handle walked
through every change that moves it between forms must report each form in turn -- and, every form being word-for-word
equivalent, end where a twin on 8-lane by-value groups (RG_STEP_SHAPE=0 RG_STEP_SPAN=0) ends after the same changes.

One PredatorCapturePrey reference-shape handle at 5 envs (one env per wave) and at 2050 (four per wave, ragged): a step, the pose
disturbance on and off, a team pool on and off, a step with the gymma block, a re-bind.  A lidar handle and an interior-point
handle report by value.  The kernel choice at the cross-over batch follows the side block (create only, no step).
"""
import ctypes as C

import pytest

from shape_kernel_harness import OUTS, SHAPE_IDS, actions as _actions, differing as _differing, make as _make
from test_shape_kernels import REFERENCE

pytestmark = pytest.mark.gpu

SCENARIO = "PredatorCapturePrey"


@pytest.mark.parametrize("E", [5, 2050])
def test_a_handle_walked_through_every_form(E, monkeypatch):
    import torch
    from marbler_amd import _lib
    monkeypatch.setenv("RG_STEP_KERNEL", "group")
    shaped, by_value = _lib.FORM_SHAPE + SHAPE_IDS[SCENARIO], _lib.FORM_BY_VALUE
    new = _make(SCENARIO, REFERENCE[SCENARIO], E, monkeypatch)
    old = _make(SCENARIO, REFERENCE[SCENARIO], E, monkeypatch, env_vars=(("RG_STEP_SHAPE", "0"), ("RG_STEP_SPAN", "0")))
    acts = _actions(new, SCENARIO, 4)
    keep, ticks = [], [0]

    def step(want, io_of=None):
        t = ticks[0]
        ticks[0] += 1
        for env in (new, old):
            if io_of is None:
                env.step(acts[t % 4])
            else:
                _lib.check(env.lib.rg_step(env._h, acts[t % 4].data_ptr(), C.byref(io_of[env]), 1, env.seed), "rg_step")
        assert (new.step_form, old.step_form) == (want, by_value), (t, new.step_form, old.step_form, want)
        bad = _differing(new, old)
        assert not bad, f"step {t}: {bad} differ"

    def each(call, what):
        for env in (new, old):
            _lib.check(call(env), what)

    step(shaped)
    on = _lib.RgDisturbanceParams(0.01, 0.05)
    each(lambda env: env.lib.rg_set_disturbance(env._h, C.byref(on)), "rg_set_disturbance")
    step(by_value)
    each(lambda env: env.lib.rg_set_disturbance(env._h, None), "rg_set_disturbance")
    step(shaped)   # (from a fresh image slot: the one before the change is stale)

    # a pool of one capability set: the parameter block's own rows
    pools = {}
    for env in (new, old):
        rows = {k: torch.tensor(list(getattr(env.params, k))[:env.N], dtype=torch.float32, device=env.device).reshape(1, env.N)
                for k in ("agent_step", "sensing_radius", "capture_radius")}
        index = torch.zeros(env.E, dtype=torch.int32, device=env.device)
        keep.append((rows, index))
        pools[env] = _lib.RgTeamParams(1, _lib.TEAM_EPISODE, rows["agent_step"].data_ptr(), rows["sensing_radius"].data_ptr(),
                                       rows["capture_radius"].data_ptr(), None, index.data_ptr())
    each(lambda env: env.lib.rg_set_teams(env._h, C.byref(pools[env])), "rg_set_teams")
    step(by_value)
    each(lambda env: env.lib.rg_set_teams(env._h, None), "rg_set_teams")
    step(shaped)

    # a step whose io carries the gymma block: kernels of its own, by value
    gym = {}
    for env in (new, old):
        block = (torch.zeros(env.E, dtype=torch.int32, device=env.device), torch.zeros(env.E, dtype=torch.uint8, device=env.device),
                 torch.zeros(env.E, dtype=torch.uint8, device=env.device), torch.zeros(env.E, dtype=torch.float32, device=env.device))
        keep.append(block)
        gym[env] = _lib.RgStepIO(*(getattr(env, k).data_ptr() for k in OUTS), *(b.data_ptr() for b in block), 1000, 0)
    step(by_value, io_of=gym)
    assert all(torch.equal(a, b) for a, b in zip(keep[-2], keep[-1])), "the gymma block's outputs differ"
    step(shaped)

    for env in (new, old):   # a re-bind to copies of the arrays
        arrays = {k: getattr(env, k).clone() for k in env.STATE_KEYS + ("next_init", "next_episode")}
        keep.append(arrays)
        st = _lib.RgState(*(arrays[k].data_ptr() for k in env.STATE_KEYS), arrays["next_init"].data_ptr(), arrays["next_episode"].data_ptr())
        _lib.check(env.lib.rg_bind_state(env._h, C.byref(st)), "rg_bind_state")
        for k, v in arrays.items():
            setattr(env, k, v)
    step(shaped)
    for _ in range(10):
        step(shaped)
    new.close()
    old.close()


@pytest.mark.parametrize("ov", [{"lidar_rays": 8}, {"barrier_solver": "cvxopt"}], ids=["lidar", "interior-point"])
def test_a_lidar_and_an_interior_point_handle_go_by_value(ov, monkeypatch):
    from marbler_amd import _lib
    monkeypatch.setenv("RG_STEP_KERNEL", "group")
    env = _make(SCENARIO, dict(REFERENCE[SCENARIO], **ov), 5, monkeypatch)
    assert env.step_form == _lib.FORM_NONE
    env.step(_actions(env, SCENARIO, 1)[0])
    assert env.step_form == _lib.FORM_BY_VALUE
    env.close()


def test_kernel_choice_follows_the_side_block_at_the_cross_over(monkeypatch):
    """PredatorCapturePrey N = 5 at 65 536 envs, nothing forced: thread-per-env; the disturbance on: lane groups (it is built into
    them alone); off again: the default choice.  Create only: rg_set_disturbance needs no bound state."""
    from marbler_amd import _lib
    from marbler_amd.params import load_config, make_params
    monkeypatch.delenv("RG_STEP_KERNEL", raising=False)
    lib = _lib.load()
    p = make_params(SCENARIO, load_config(SCENARIO, overrides=REFERENCE[SCENARIO]))
    h = lib.rg_create(C.byref(p), 65536, 0, 0, None)
    assert h, lib.rg_last_error().decode()
    try:
        assert lib.rg_step_kernel(h) == 1
        _lib.check(lib.rg_set_disturbance(h, C.byref(_lib.RgDisturbanceParams(0.01, 0.05))), "rg_set_disturbance")
        assert lib.rg_step_kernel(h) == 0
        _lib.check(lib.rg_set_disturbance(h, None), "rg_set_disturbance")
        assert lib.rg_step_kernel(h) == 1
    finally:
        lib.rg_destroy(h)
