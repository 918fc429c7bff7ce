"""rg_render on the GPU against the float64 twin (tests/render_twin.py): every pixel whose centre is not within 1e-4 m of a shape's
edge is equal, and those that are stay below 0.5 % of a case's pixels (tests/render_cases.py: the shapes, the views, the hand-made
states whose degenerate share the CPU tier asserts too).  Then the layers one by one, the env selection and `out=`, that rendering
changes nothing, the opt-in features, the other surfaces, and non-finite poses.

Reference surface this replaces: scenarios/*/visualize.py drawn through utilities/roboEnv.py:67-76."""
import numpy as np
import pytest
import torch

import render_cases as rc
from gpu_helpers import random_actions
from render_twin import LAYERS, count, render_twin

pytestmark = pytest.mark.gpu


def _env(scenario, E, ov=None, **kw):
    from marbler_amd import VecRobotariumEnv
    kw.setdefault("seed", 11)
    return VecRobotariumEnv(scenario, E, overrides=dict(ov or {}), device="cuda:0", **kw)


def _host_state(env):
    return {k: getattr(env, k).cpu().numpy() for k in ("poses", "prey_loc", "prey_sensed", "prey_captured", "grid")}


def _load(env, state):
    for k, v in state.items():
        getattr(env, k).copy_(torch.as_tensor(v).reshape(getattr(env, k).shape))


def _against_twin(env, what, envs=None, size=84, view=None, layers=None, twin_layers=None, frames=None):
    """renders, and holds every frame to the twin of its env's state; -> the degenerate share over the frames"""
    frames = env.render(envs=envs, size=size, view=view, layers=layers) if frames is None else frames
    assert frames.dtype == torch.uint8 and frames.device == env.device
    H, W = (size, size) if isinstance(size, int) else size
    idx = list(range(env.E)) if envs is None else list(envs)
    assert tuple(frames.shape) == (len(idx), H, W, 3), what
    got = frames.cpu().numpy()
    state = _host_state(env)
    if twin_layers is None:
        twin_layers = layers if layers is not None else LAYERS
    bad = 0
    for k, e in enumerate(idx):
        want, deg = render_twin(env.params, rc.env_state(state, e), W, H, view=view, layers=twin_layers)
        differ = (got[k] != want).any(-1) & ~deg
        assert not differ.any(), (what, "frame", k, "env", e, "first differing pixel (row, column)", np.argwhere(differ)[0].tolist(),
                                  got[k][differ][0].tolist(), want[differ][0].tolist())
        bad += int(deg.sum())
    share = bad / (len(idx) * H * W)
    assert share <= rc.MAX_DEGENERATE_SHARE, (what, "degenerate share", share)
    return share


def _cases(group):
    """every shape of the group on three states: after reset(), after 10 random steps, and the hand-made one of the CPU tier"""
    seen = 0
    for name, _, scenario, ov, shape, E, idx, size, view in (c for c in rc.all_cases() if c[1] == group):
        env = _env(scenario, E, ov, seed=rc.ENV_SEED.get(name, 11))
        first = (idx or [0])[0]
        env.reset()
        _against_twin(env, (name, "reset"), idx, size, rc.case_view(scenario, shape, view, env.poses[first].cpu().numpy()))
        for a in random_actions(env, 10, seed=len(name)):
            env.step(a)
        _against_twin(env, (name, "stepped"), idx, size, rc.case_view(scenario, shape, view, env.poses[first].cpu().numpy()))
        state = rc.synthetic_state(env.params, E, seed=len(name))
        _load(env, state)
        _against_twin(env, (name, "hand-made"), idx, size, rc.case_view(scenario, shape, view, state["poses"][first]))
        env.close()
        seen += 1
    assert seen


@pytest.mark.parametrize("scenario", list(rc.SCENARIOS))
def test_frames_equal_the_twin(scenario):
    """48 x 32 with K = 3 frames of envs [4, 0, 2] out of 5; 20 x 12 (5 lanes per row, several rows per wavefront); 84 x 84 of both
    envs; a 1 m x 1 m zoom about a robot; a view larger than the arena.  PredatorCapturePrey N = 5, Warehouse N = 8,
    MaterialTransport N = 6."""
    _cases(scenario)


@pytest.mark.parametrize("name", list(rc.EXTRA))
def test_frames_equal_the_twin_many_prey_and_sixteen_agents(name):
    _cases(name)


def test_a_sensed_prey_changes_colour_and_a_captured_one_disappears():
    """the flags reach the picture: robot 0 (sensing) is put next to prey 0 of every env and one step is taken"""
    env = _env("PredatorCapturePrey", 64, rc.SCENARIOS["PredatorCapturePrey"], auto_reset=False)
    env.reset()
    before = env.render().cpu().numpy()
    assert count(before, "prey_sensed") == 0 and count(before, "prey") > 0
    env.poses[:, 0, 0] = env.prey_loc[:, 0, 0] - 0.1
    env.poses[:, 1, 0] = env.prey_loc[:, 0, 1]
    env.step(random_actions(env, 1, seed=3)[0])
    assert int(env.prey_sensed[:, 0].sum()) > 0
    after = env.render().cpu().numpy()
    assert count(after, "prey_sensed") > 0 and count(after, "prey") < count(before, "prey")
    _against_twin(env, "sensed", [0, 63], 84)
    env.prey_captured[:, :] = 1
    gone = env.render().cpu().numpy()
    assert count(gone, "prey_sensed") == 0 and count(gone, "prey") == 0
    env.close()


@pytest.mark.parametrize("scenario", list(rc.SCENARIOS))
def test_each_layer_alone_and_all_of_them(scenario):
    env = _env(scenario, 3, rc.SCENARIOS[scenario])
    state = rc.synthetic_state(env.params, 3, seed=5)
    _load(env, state)
    view = rc.OFF_LATTICE_VIEW
    for layer in LAYERS:
        _against_twin(env, (scenario, layer), None, (32, 48), view, layers=[layer])
    everything = env.render(size=(32, 48), view=view, layers=list(LAYERS))
    assert torch.equal(env.render(size=(32, 48), view=view), everything)
    _against_twin(env, (scenario, "all"), None, (32, 48), view, frames=everything)
    env.close()


def test_selection_and_out():
    env = _env("PredatorCapturePrey", 5, rc.SCENARIOS["PredatorCapturePrey"])
    env.reset()
    every = env.render()
    assert tuple(every.shape) == (5, 84, 84, 3)
    assert torch.equal(env.render(envs=[3])[0], every[3])
    assert torch.equal(env.render(envs=3)[0], every[3])
    assert torch.equal(env.render(envs=torch.tensor([4, 0, 2], device=env.device)), every[[4, 0, 2]])
    assert torch.equal(env.render(envs=torch.tensor([1, 1], dtype=torch.int64)), every[[1, 1]])
    with pytest.raises(IndexError):
        env.render(envs=[5])
    with pytest.raises(ValueError):
        env.render(size=(32, 50))
    with pytest.raises(ValueError):
        env.render(layers=["robot"])
    with pytest.raises(TypeError):
        env.render(out=torch.zeros(5, 84, 84, 3, device=env.device))
    with pytest.raises(ValueError):
        env.render(out=torch.zeros(4, 84, 84, 3, dtype=torch.uint8, device=env.device))
    # out=: a guard row on each side of the caller's batch stays as it was
    for size, envs in (((84, 84), None), ((12, 20), [2, 4, 1])):
        K = 5 if envs is None else len(envs)
        slab = torch.full((K + 2,) + size + (3,), 0xA5, dtype=torch.uint8, device=env.device)
        out = env.render(envs=envs, size=size, out=slab[1:K + 1])
        assert out.data_ptr() == slab[1].data_ptr()
        assert torch.equal(out, env.render(envs=envs, size=size))
        assert bool((slab[0] == 0xA5).all()) and bool((slab[K + 1] == 0xA5).all())
    env.close()


def test_render_changes_nothing():
    ov = rc.SCENARIOS["PredatorCapturePrey"]
    a, b = _env("PredatorCapturePrey", 33, ov), _env("PredatorCapturePrey", 33, ov)
    a.reset()
    b.reset()
    before = a.state_dict()
    a.render()
    a.render(envs=[32, 0], size=(12, 20), layers=["robots"])
    after = a.state_dict()
    assert set(before) == set(after)
    for k in before:
        assert torch.equal(before[k].contiguous().view(torch.uint8), after[k].contiguous().view(torch.uint8)), k
    for t, act in enumerate(random_actions(a, 20, seed=9)):
        oa, ra, da, ia = a.step(act)
        a.render(size=(32, 48))
        ob, rb, db, ib = b.step(act)
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)) and torch.equal(ra.view(torch.int32), rb.view(torch.int32)), t
        assert torch.equal(da, db) and all(torch.equal(ia[k], ib[k]) for k in ia), t
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k].contiguous().view(torch.uint8), sb[k].contiguous().view(torch.uint8)), k
    a.close()
    b.close()


def test_with_the_lidar_a_team_pool_and_the_disturbance():
    from team_harness import pool4
    pcp, view = rc.SCENARIOS["PredatorCapturePrey"], rc.OFF_LATTICE_VIEW
    for what, ov in (("lidar", dict(pcp, lidar_rays=8)), ("disturbance", dict(pcp, pose_noise_xy=0.01, pose_noise_theta=0.05)),
                     ("teams", dict(pcp, teams=pool4("PredatorCapturePrey", 5)))):
        env = _env("PredatorCapturePrey", 5, ov)
        assert (env.lidar is not None, env.disturbance is not None, env.teams is not None) == \
            (what == "lidar", what == "disturbance", what == "teams")
        env.reset()
        for a in random_actions(env, 6, seed=2):
            env.step(a)
        if what == "teams":     # no rings unless asked for by name: they would show the config's radii, not the pool's
            no_rings = [name for name in LAYERS if name != "rings"]
            _against_twin(env, what, None, (32, 48), view, twin_layers=no_rings)
            assert torch.equal(env.render(size=(32, 48)), env.render(size=(32, 48), layers=no_rings))
            _against_twin(env, what + " rings by name", None, (32, 48), view, layers=list(LAYERS))
            assert not torch.equal(env.render(size=(32, 48)), env.render(size=(32, 48), layers=list(LAYERS)))
        else:
            _against_twin(env, what, None, (32, 48), view)
        env.close()


def test_the_other_surfaces():
    from marbler_amd import Wrapper, render
    from marbler_amd.gymma import GymmaEnv, GymmaVecEnv
    w = Wrapper("Warehouse")
    w.reset()
    assert w.render() is None and w.render(mode="human") is None and w.env.render() is None
    frame = w.render(mode="rgb_array")
    assert isinstance(frame, np.ndarray) and frame.dtype == np.uint8 and frame.shape == (84, 84, 3)
    assert np.array_equal(frame, w.env.vec.render()[0].cpu().numpy())
    assert np.array_equal(w.env.render(mode="rgb_array", size=(32, 48)), w.env.vec.render(size=(32, 48))[0].cpu().numpy())
    assert Wrapper.metadata == {"render.modes": [], "render_modes": []}
    w.close()
    v = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", 4, time_limit=20, seed=3)
    v.reset()
    assert v.render() is None
    frames = v.render(mode="rgb_array", size=(32, 48))
    assert isinstance(frames, torch.Tensor) and torch.equal(frames, v.env.render(size=(32, 48)))
    v.close()
    g = GymmaEnv("robotarium_gym:Simple-v0", time_limit=20, seed=3)
    g.reset()
    assert g.render() is None
    frame = g.render(mode="rgb_array")
    assert isinstance(frame, np.ndarray) and frame.dtype == np.uint8 and frame.shape == (84, 84, 3)
    assert np.array_equal(frame, g._v.env.render()[0].cpu().numpy())
    g.close()
    # record: T + 1 frames per env, frame 0 the state before the first step, frame t + 1 the state after step t
    ov = rc.SCENARIOS["PredatorCapturePrey"]
    env, twin = _env("PredatorCapturePrey", 3, ov), _env("PredatorCapturePrey", 3, ov)
    env.reset()
    twin.reset()
    acts = random_actions(env, 4, seed=1)
    clip = render.record(env, acts, size=(32, 48), envs=[2, 0])
    assert tuple(clip.shape) == (5, 2, 32, 48, 3) and clip.dtype == torch.uint8
    assert torch.equal(clip[0], twin.render(envs=[2, 0], size=(32, 48)))
    for t in range(4):
        twin.step(acts[t])
        assert torch.equal(clip[t + 1], twin.render(envs=[2, 0], size=(32, 48))), t
    assert tuple(render.record(env, acts[:1]).shape) == (2, 3, 84, 84, 3)
    env.close()
    twin.close()


def test_non_finite_poses_draw_nothing():
    """A defined input of the spec: every test of the raster is a comparison that is false for a NaN."""
    env = _env("PredatorCapturePrey", 2, rc.SCENARIOS["PredatorCapturePrey"])
    state = rc.synthetic_state(env.params, 2, seed=8)
    _load(env, state)
    whole = env.render(size=(32, 48)).cpu().numpy()
    state["poses"][0, 0, 1] = np.nan            # env 0: robot 1 at x = NaN, robot 3 at 1e30
    state["poses"][0, :2, 3] = 1e30
    state["poses"][1, 2, 0] = np.nan            # env 1: a NaN heading, an infinite one
    state["poses"][1, 2, 2] = np.inf
    _load(env, state)
    _against_twin(env, "non-finite", None, (32, 48))
    holed = env.render(size=(32, 48)).cpu().numpy()
    assert count(holed[0], "class0") < count(whole[0], "class0")          # robot 1 senses, robot 3 captures: both are gone
    assert count(holed[0], "class1") < count(whole[0], "class1")
    assert count(holed[1], "heading") < count(whole[1], "heading")
    torch.cuda.synchronize()
    env.close()
