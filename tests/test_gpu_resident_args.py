"""The resident form of the 16-lane-row step kernels (kernel_args.h ResidentCall, robogym_resident.hip): what rg_create and
rg_bind_state fix is read from an image of the argument block that the handle keeps in device memory, and the kernel's own
arguments are the image's address and the per-call ones (actions, io, seed, auto_reset).  Against a handle created under
RG_STEP_RESIDENT=0, which launches the by-value row kernels: every output of every step and the whole state at the end, word for
word.

Batches 5, 1027 and 2051: the smallest ragged ones with one, two and four envs per wave (wave_fill).  About 100 steps with
auto_reset and `max_episode_steps` 12, so that episodes end, the drawn-ahead copy starts the next one and the sampler redraws;
every test asserts that resets and QPs of several sweeps occurred.  (Which of the two forms a launch took is not visible through
the C ABI; that the library holds the sixteen resident kernels, and what they look like, is tests/test_resident_kernels.py.)
"""
import ctypes as C

import numpy as np
import pytest

from gpu_helpers import expected_slots, guarded_class, lane_group_kernel  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

STEPS = 100
PCP5 = ("PredatorCapturePrey", {"predator": 3, "capture": 2, "n_agents": 5, "max_episode_steps": 12}, 5)
WAREHOUSE8 = ("Warehouse", {"n_agents": 8, "max_episode_steps": 12}, 5)
MT6 = ("MaterialTransport", {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25, "max_episode_steps": 12}, 20)
SLOTS = {5: 1, 1027: 2, 2051: 4}
STATE = ("poses", "carry_dist", "episode_steps", "reset_count", "prey_loc", "prey_sensed", "prey_captured", "loaded", "load",
         "zone_load", "messages", "grid", "goal_col", "pixel_type", "reached_goal", "ep_return", "done_return_sum", "done_count",
         "done_steps_sum")
SCRATCH = ("next_init", "next_episode")
OUTS = ("obs", "reward", "done_u8", "dist_travelled", "violation", "remaining", "qp_sweeps")


def _make(config, E, resident, monkeypatch, guarded=False, auto_reset=True):
    from marbler_amd import VecRobotariumEnv
    scenario, ov, _ = config
    with monkeypatch.context() as m:   # read by rg_create
        if resident:
            m.delenv("RG_STEP_RESIDENT", raising=False)
        else:
            m.setenv("RG_STEP_RESIDENT", "0")
        kw = dict(overrides=ov, seed=7, auto_reset=auto_reset, collect_qp_stats=True)
        env = guarded_class()(scenario, E, slab_bytes=E * 8192 + (8 << 20), **kw) if guarded else VecRobotariumEnv(scenario, E, **kw)
    env.reset()
    assert env.step_kernel == "group" and 5 <= env.N <= 8 and expected_slots(env.N, E) <= 4, "the case no longer dispatches a row kernel"
    return env


def _pair(config, E, monkeypatch, guarded=False):
    return _make(config, E, True, monkeypatch, guarded), _make(config, E, False, monkeypatch)


def _outputs(env):
    return {k: getattr(env, k) for k in OUTS}


def _io(outs):
    from marbler_amd import _lib
    return _lib.RgStepIO(*(outs[k].data_ptr() for k in OUTS))


def _words(outs):
    import torch
    return torch.cat([outs[k].contiguous().view(torch.uint8).flatten() for k in OUTS])


def _state_words(arrays):
    import torch
    return torch.cat([arrays[k].contiguous().view(torch.uint8).flatten() for k in STATE])


def _arrays(env):
    return {k: getattr(env, k) for k in STATE + SCRATCH}


def _rebind(env, arrays):
    from marbler_amd import _lib
    st = _lib.RgState(*(arrays[k].data_ptr() for k in STATE), arrays["next_init"].data_ptr(), arrays["next_episode"].data_ptr())
    _lib.check(env.lib.rg_bind_state(env._h, C.byref(st)), "rg_bind_state")


def _step(env, actions, io, auto_reset, seed):
    from marbler_amd import _lib
    env._sync_stream()
    _lib.check(env.lib.rg_step(env._h, actions.data_ptr(), C.byref(io), auto_reset, seed), "rg_step")


def _actions(env, n_act, count, seed=11):
    import torch
    rng = np.random.RandomState(seed)
    return [torch.as_tensor(rng.randint(0, n_act, size=(env.E, env.N)).astype(np.int32), device=env.device) for _ in range(count)]


class _Happened:
    """Resets and QPs of more than one sweep, counted over a run of the resident handle."""

    def __init__(self):
        self.sweeps = 0

    def step(self, outs):
        self.sweeps = max(self.sweeps, int(outs["qp_sweeps"].max()))

    def check(self, reset_count):
        assert int(reset_count.max()) >= 3, "no env began a third episode"
        assert self.sweeps >= 2, "no QP took more than one sweep"


@pytest.mark.parametrize("config,E", [(PCP5, 5), (PCP5, 1027), (PCP5, 2051), (WAREHOUSE8, 1027), (MT6, 1027)],
                         ids=["pcp5-E5", "pcp5-E1027", "pcp5-E2051", "warehouse8-E1027", "mt6-E1027"])
def test_per_call_arguments_are_per_call(config, E, monkeypatch):
    """One handle, two action tensors and two sets of output tensors alternating, a new seed from step 40 on, auto_reset off
    for steps 60..69: the by-value twin is fed identically."""
    import torch
    new, old = _pair(config, E, monkeypatch)
    acts_new, acts_old = _actions(new, config[2], 2), _actions(old, config[2], 2)
    sets = []
    for env in (new, old):
        second = {k: torch.zeros_like(v) for k, v in _outputs(env).items()}
        sets.append([_outputs(env), second])
    ios = [[_io(s) for s in both] for both in sets]
    seen = _Happened()
    for t in range(STEPS):
        which, seed, auto = t % 2, (7 if t < 40 else 1234567890123), 0 if 60 <= t < 70 else 1
        if t % 7 == 0:   # fresh actions in the SAME two tensors: the kernel reads the address it was given this call
            fresh = _actions(new, config[2], 1, seed=100 + t)[0]
            acts_new[which].copy_(fresh)
            acts_old[which].copy_(fresh)
        _step(new, acts_new[which], ios[0][which], auto, seed)
        _step(old, acts_old[which], ios[1][which], auto, seed)
        assert torch.equal(_words(sets[0][which]), _words(sets[1][which])), \
            f"step {t}: {[k for k in OUTS if not torch.equal(sets[0][which][k], sets[1][which][k])]} differ"
        seen.step(sets[0][which])
    assert torch.equal(_state_words(_arrays(new)), _state_words(_arrays(old))), \
        [k for k in STATE if not torch.equal(getattr(new, k), getattr(old, k))]
    seen.check(new.reset_count)
    new.close()
    old.close()


def test_the_image_follows_a_rebind(monkeypatch):
    """Re-bound to a second set of arrays mid-run, the handle advances those and never writes the first set again (which lies
    on the red-zone slab, like `obs`)."""
    import torch
    E = 2051
    new, old = _pair(PCP5, E, monkeypatch, guarded=True)
    acts = _actions(new, PCP5[2], 4)
    io_new, io_old = _io(_outputs(new)), _io(_outputs(old))
    seen = _Happened()

    def run(t0, t1):
        for t in range(t0, t1):
            a = acts[t % len(acts)]
            _step(new, a, io_new, 1, 7)
            _step(old, a, io_old, 1, 7)
            assert torch.equal(_words(_outputs(new)), _words(_outputs(old))), f"step {t}"
            seen.step(_outputs(new))

    run(0, STEPS // 2)
    first = _arrays(new)
    frozen = {k: v.clone() for k, v in first.items()}
    second_new = {k: v.clone() for k, v in first.items()}
    second_old = {k: v.clone() for k, v in _arrays(old).items()}
    _rebind(new, second_new)
    _rebind(old, second_old)
    run(STEPS // 2, STEPS)
    assert torch.equal(_state_words(second_new), _state_words(second_old)), \
        [k for k in STATE if not torch.equal(second_new[k], second_old[k])]
    assert not torch.equal(second_new["poses"], frozen["poses"]), "the new arrays did not advance"
    for k in STATE + SCRATCH:
        assert torch.equal(first[k], frozen[k]), f"`{k}` of the first set was written after the re-bind"
    bad = new.red_zones_intact()
    assert bad.size == 0, f"{bad.size} red-zone bytes damaged, first after `{new.owner_of(int(bad[0]))}`"
    seen.check(second_new["reset_count"])
    new.close()
    old.close()


def test_a_captured_graph_keeps_the_arrays_it_captured(monkeypatch):
    """Three rg_step launches recorded into a graph on a side stream (one linear chain), replayed; then a re-bind and eager
    steps; then the replay again, which acts on the arrays it captured -- as the by-value twin's graph does."""
    import torch
    E = 1027
    new, old = _pair(PCP5, E, monkeypatch)
    acts = _actions(new, PCP5[2], 3)
    seen = _Happened()
    graphs, firsts, seconds = [], [], []
    for env in (new, old):
        dev = env.device
        io = _io(_outputs(env))
        for t in range(30):   # (eager steps first: episodes under way, the seed known to the handle)
            _step(env, acts[t % 3], io, 1, 7)
        torch.cuda.synchronize(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        prev = env._stream
        env.set_stream(side)
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                for i in range(3):
                    assert env.lib.rg_step(env._h, acts[i].data_ptr(), C.byref(io), 1, 7) == 0
            for _ in range(10):
                graph.replay()
        torch.cuda.synchronize(dev)
        env.set_stream(prev)
        torch.cuda.current_stream(dev).wait_stream(side)
        first = _arrays(env)
        second = {k: v.clone() for k, v in first.items()}
        _rebind(env, second)
        for t in range(30):
            _step(env, acts[t % 3], io, 1, 7)
            if env is new:
                seen.step(_outputs(env))
        torch.cuda.synchronize(dev)
        after_eager = {k: v.clone() for k, v in second.items()}
        with torch.cuda.stream(side):
            for _ in range(10):
                graph.replay()
        torch.cuda.synchronize(dev)
        for k in STATE:
            assert torch.equal(second[k], after_eager[k]), f"the replay wrote `{k}` of the arrays bound after the capture"
        graphs.append(graph)
        firsts.append(first)
        seconds.append(second)
    assert torch.equal(_state_words(firsts[0]), _state_words(firsts[1])), "the captured arrays differ from the by-value twin's"
    assert torch.equal(_state_words(seconds[0]), _state_words(seconds[1])), "the re-bound arrays differ from the by-value twin's"
    assert torch.equal(_words(_outputs(new)), _words(_outputs(old)))
    assert int(firsts[0]["reset_count"].max()) >= 3
    seen.check(seconds[0]["reset_count"])
    del graphs
    new.close()
    old.close()


def test_two_handles_interleaved_keep_their_own_images(monkeypatch):
    """Two handles of different shapes on one device, stepped in turn."""
    import torch
    pairs = [(_pair(PCP5, 5, monkeypatch), PCP5), (_pair(PCP5, 2051, monkeypatch), PCP5), (_pair(WAREHOUSE8, 1027, monkeypatch), WAREHOUSE8)]
    acts = [_actions(p[0], c[2], 3) for p, c in pairs]
    ios = [[_io(_outputs(env)) for env in p] for p, _ in pairs]
    seen = [_Happened() for _ in pairs]
    for t in range(STEPS):
        for i, (p, _) in enumerate(pairs):   # the resident handles back to back, then their twins
            _step(p[0], acts[i][t % 3], ios[i][0], 1, 7)
        for i, (p, _) in enumerate(pairs):
            _step(p[1], acts[i][t % 3], ios[i][1], 1, 7)
        for i, (p, _) in enumerate(pairs):
            assert torch.equal(_words(_outputs(p[0])), _words(_outputs(p[1]))), f"step {t}, handle {i}"
            seen[i].step(_outputs(p[0]))
    for i, (p, _) in enumerate(pairs):
        assert torch.equal(_state_words(_arrays(p[0])), _state_words(_arrays(p[1]))), f"handle {i}"
        seen[i].check(p[0].reset_count)
        p[0].close()
        p[1].close()


def test_steps_match_when_the_image_slots_are_used_up(monkeypatch):
    """Twelve re-binds (more than the handle has slots): the launches fall back to by value, with the arrays of the last bind."""
    import torch
    E = 1027
    new, old = _pair(PCP5, E, monkeypatch)
    acts = _actions(new, PCP5[2], 3)
    io_new, io_old = _io(_outputs(new)), _io(_outputs(old))
    seen = _Happened()
    sets = [(_arrays(new), _arrays(old))]
    for t in range(STEPS):
        if t % 8 == 7:   # a new set of arrays, continuing from the current one
            cur = sets[-1]
            sets.append(tuple({k: v.clone() for k, v in arrays.items()} for arrays in cur))
            _rebind(new, sets[-1][0])
            _rebind(old, sets[-1][1])
        _step(new, acts[t % 3], io_new, 1, 7)
        _step(old, acts[t % 3], io_old, 1, 7)
        assert torch.equal(_words(_outputs(new)), _words(_outputs(old))), f"step {t} (bind {len(sets) - 1})"
        seen.step(_outputs(new))
    assert len(sets) == 13
    for n, (a, b) in enumerate(sets):
        assert torch.equal(_state_words(a), _state_words(b)), f"the arrays of bind {n}"
    seen.check(sets[-1][0]["reset_count"])
    new.close()
    old.close()
