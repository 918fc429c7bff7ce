"""The episode buffer without a GPU: the NumPy twin of the rule (csrc/episodes.h) on hand-written streams whose expected slots
are written out here, the binding, every refusal of rg_episodes_append's host half (host pointers that are never dereferenced),
and the Python argument errors that are decided before a device is touched."""
import ctypes
import re
import types

import numpy as np
import pytest

import episodes_cases as ec
from episodes_twin import TwinBuffer


def _run(name, upto=None):
    case = ec.HAND_CASES[name]
    calls = ec.hand_calls(case)
    twin = TwinBuffer(len(case["calls"][0]), case["R"], case["L"], case["N"], case["D"], case["with_prob"])
    for batch in calls[:upto]:
        twin.append(batch)
    return twin


def _slot(twin, s):
    """the slot's rows, by their first element, as plain lists"""
    return {"obs": twin.obs[s, :, 0, 0].tolist(), "actions": twin.actions[s, :, 0].tolist(), "reward": twin.reward[s].tolist(),
            "terminated": twin.terminated[s].tolist(), "filled": twin.filled[s].tolist(), "length": int(twin.length[s]),
            "episode_return": float(twin.episode_return[s]), "complete": int(twin.complete[s]), "fresh": int(twin.fresh[s]),
            "episode_index": int(twin.episode_index[s])}


# ---------------------------------------------------------------- the twin on known answers
def test_twin_two_call_carry():
    first = _run("two_call_carry", upto=1)
    assert first.cursor.tolist() == [[0, 3, 1, 0]]
    assert _slot(first, 0) == {"obs": [0, 1, 2, 0, 0, 0], "actions": [0, 1, 2, 0, 0, 0], "reward": [0, 1, 2, 0, 0, 0],
                               "terminated": [0] * 6, "filled": [1, 1, 1, 0, 0, 0], "length": 0, "episode_return": 3.0,
                               "complete": 0, "fresh": 0, "episode_index": 0}
    assert first.take_new().tolist() == []
    twin = _run("two_call_carry")
    assert _slot(twin, 0) == {"obs": [0, 1, 2, 3, 4, 5], "actions": [0, 1, 2, 3, 4, 0], "reward": [0, 1, 2, 3, 4, 0],
                              "terminated": [0, 0, 0, 0, 1, 0], "filled": [1] * 6, "length": 5, "episode_return": 10.0,
                              "complete": 1, "fresh": 1, "episode_index": 0}
    assert _slot(twin, 1) == {"obs": [5, 0, 0, 0, 0, 0], "actions": [5, 0, 0, 0, 0, 0], "reward": [5, 0, 0, 0, 0, 0],
                              "terminated": [0] * 6, "filled": [1, 0, 0, 0, 0, 0], "length": 0, "episode_return": 5.0,
                              "complete": 0, "fresh": 0, "episode_index": 1}
    assert twin.cursor.tolist() == [[1, 1, 2, 0]]
    assert twin.obs[0, 2, 1, 2] == np.float32(2 + 5 / 64)                     # the whole row, not its first element
    assert twin.take_new().tolist() == [0] and twin.take_new().tolist() == []


def test_twin_termination_at_the_last_step_takes_the_last_observation():
    twin = _run("termination_at_last_step")
    assert _slot(twin, 0) == {"obs": [0, 1, 2, 3, 0], "actions": [0, 1, 2, 0, 0], "reward": [0, 1, 2, 0, 0],
                              "terminated": [0, 0, 1, 0, 0], "filled": [1, 1, 1, 1, 0], "length": 3, "episode_return": 3.0,
                              "complete": 1, "fresh": 1, "episode_index": 0}
    assert twin.prob[0, :, 0].tolist() == [1 / 256, 2 / 256, 3 / 256, 0, 0]
    assert twin.cursor.tolist() == [[-1, 0, 1, 0]] and not twin.filled[1].any()


def test_twin_one_slot_takes_four_episodes_in_one_call():
    twin = _run("one_slot_four_episodes")
    # rows 0 and 1 are the fourth episode's, row 2 is what the third one left there: `filled` says which rows are data
    assert _slot(twin, 0) == {"obs": [4, 5, 4, 0], "actions": [4, 3, 0, 0], "reward": [4, 0, 0, 0], "terminated": [1, 0, 0, 0],
                              "filled": [1, 1, 0, 0], "length": 1, "episode_return": 4.0, "complete": 1, "fresh": 1,
                              "episode_index": 3}
    assert twin.cursor.tolist() == [[-1, 0, 4, 0]]


def test_twin_attaching_mid_episode_drops_the_part_it_sees():
    twin = _run("attach_mid_episode")
    assert _slot(twin, 0) == {"obs": [3, 4, 0, 0, 0], "actions": [3, 4, 0, 0, 0], "reward": [3, 4, 0, 0, 0], "terminated": [0] * 5,
                              "filled": [1, 1, 0, 0, 0], "length": 0, "episode_return": 7.0, "complete": 0, "fresh": 0,
                              "episode_index": 0}
    assert twin.cursor.tolist() == [[0, 2, 1, 0]] and twin.take_new().tolist() == []


def test_twin_abandoned_episode_gives_its_slot_to_the_next():
    twin = _run("abandoned_episode")
    assert _slot(twin, 0) == {"obs": [2, 3, 4, 5, 0], "actions": [2, 3, 4, 0, 0], "reward": [2, 3, 4, 0, 0],
                              "terminated": [0, 0, 1, 0, 0], "filled": [1, 1, 1, 1, 0], "length": 3, "episode_return": 9.0,
                              "complete": 1, "fresh": 1, "episode_index": 0}
    assert twin.cursor.tolist() == [[-1, 0, 1, 0]]
    assert not twin.filled[1].any() and not twin.obs[1].any() and twin.complete[1] == 0     # the other slot was never used


def test_twin_overflow_is_force_closed_and_counted():
    twin = _run("overflow")
    assert _slot(twin, 0) == {"obs": [0, 1, 2], "actions": [0, 1, 0], "reward": [0, 1, 0], "terminated": [0, 0, 0],
                              "filled": [1, 1, 1], "length": 2, "episode_return": 1.0, "complete": 1, "fresh": 1, "episode_index": 0}
    assert _slot(twin, 1) == {"obs": [4, 0, 0], "actions": [4, 0, 0], "reward": [4, 0, 0], "terminated": [0, 0, 0],
                              "filled": [1, 0, 0], "length": 0, "episode_return": 4.0, "complete": 0, "fresh": 0, "episode_index": 1}
    assert twin.cursor.tolist() == [[1, 1, 2, 1]]


def test_twin_two_envs_over_two_calls():
    first = _run("two_envs", upto=1)
    assert first.cursor.tolist() == [[-1, 0, 1, 0], [2, 2, 1, 0]] and first.take_new().tolist() == [0]
    twin = _run("two_envs")
    assert _slot(twin, 0) == {"obs": [0, 1, 2, 3], "actions": [0, 1, 2, 0], "reward": [0, 1, 2, 0], "terminated": [0, 0, 1, 0],
                              "filled": [1] * 4, "length": 3, "episode_return": 3.0, "complete": 1, "fresh": 1, "episode_index": 0}
    assert _slot(twin, 1) == {"obs": [3, 4, 5, 6], "actions": [3, 4, 5, 0], "reward": [3, 4, 5, 0], "terminated": [0] * 4,
                              "filled": [1] * 4, "length": 3, "episode_return": 12.0, "complete": 1, "fresh": 1, "episode_index": 1}
    # env 1 joined late, ran into the limit in the second call, and the end flag after that found no open episode
    assert _slot(twin, 2) == {"obs": [1001, 1002, 1003, 1004], "actions": [101, 102, 103, 0], "reward": [1.5, 2.5, 3.5, 0],
                              "terminated": [0] * 4, "filled": [1] * 4, "length": 3, "episode_return": 7.5, "complete": 1,
                              "fresh": 1, "episode_index": 0}
    assert not twin.filled[3].any()
    assert twin.cursor.tolist() == [[-1, 0, 2, 1], [-1, 0, 1, 1]]
    assert twin.prob[2, :, 1].tolist() == [2 / 256, 3 / 256, 4 / 256, 0]


def test_synthetic_streams_are_a_collectors():
    calls = ec.synthetic_calls(3, 3, 7, 5, 2, 3, 0.3, True)
    for a, b in zip(calls, calls[1:]):
        assert np.array_equal(a["obs"][-1], b["obs"][0]) and np.array_equal(a["terminated"][-1], b["episode_start"][0])
    assert calls[0]["episode_start"][0].all() and np.array_equal(calls[0]["episode_start"][1:], calls[0]["terminated"][:-1])
    assert not ec.synthetic_calls(3, 1, 7, 5, 2, 3, 0.3, False, attached=False)[0]["episode_start"][0].any()
    assert not ec.synthetic_calls(3, 1, 7, 5, 2, 3, 0.0, False)[0]["terminated"].any()
    assert ec.synthetic_calls(3, 1, 7, 5, 2, 3, 1.0, False)[0]["terminated"].all()


# ---------------------------------------------------------------- the binding
NAMES = ("rg_episodes_append", "rg_sizeof_episode_buffer", "rg_sizeof_episode_stream", "rg_episodes_last_error")


def test_entry_points_are_exported_declared_and_their_structs_match():
    from marbler_amd import _lib
    lib = _lib.load()
    header = open(_lib.__file__.replace("marbler_amd/_lib.py", "include/robogym.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS and name in _lib.LATE_QUERIES
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.rg_sizeof_episode_buffer() == ctypes.sizeof(_lib.RgEpisodeBuffer) == 120
    assert lib.rg_sizeof_episode_stream() == ctypes.sizeof(_lib.RgEpisodeStream) == 56
    assert lib.rg_abi_version() == 7
    assert "robogym_episodes.hip" in __import__("marbler_amd.build", fromlist=["SOURCES"]).SOURCES


# the pointer fields in the order of the header's error list
BUFFER_FIELDS = ("obs", "actions", "reward", "terminated", "filled", "length", "episode_return", "complete", "fresh", "episode_index",
                 "cursor")
STREAM_FIELDS = ("obs", "actions", "reward", "terminated", "episode_start")
WORD_FIELDS = {"obs", "actions", "reward", "length", "episode_return", "episode_index", "cursor", "prob"}


def _structs(with_prob=False):
    from marbler_amd import _lib
    b, s = _lib.RgEpisodeBuffer(), _lib.RgEpisodeStream()
    for i, f in enumerate(BUFFER_FIELDS):
        setattr(b, f, 0x10000 * (i + 1))
    for i, f in enumerate(STREAM_FIELDS):
        setattr(s, f, 0x10000 * (i + 20))
    if with_prob:
        b.prob, s.prob = 0x400000, 0x500000
    b.num_envs, b.slots_per_env, b.episode_limit, b.n_agents, b.obs_dim, s.T = 4, 2, 5, 3, 6, 7
    return b, s


def test_rg_episodes_append_refuses_every_bad_argument_before_touching_a_device():
    from marbler_amd import _lib
    lib = _lib.load()
    seen = {}

    def refused(code, word, b, s, what):
        rc = lib.rg_episodes_append(ctypes.byref(b) if b is not None else None, ctypes.byref(s) if s is not None else None, None)
        msg = lib.rg_episodes_last_error()
        assert rc == code, (what, rc, msg)
        assert word in msg and msg.startswith(b"rg_episodes_append: "), (what, rc, msg)
        assert seen.setdefault(rc, word) == word, (what, rc, "one code, two meanings")

    b, s = _structs()
    refused(-1, b"buffer is NULL", None, s, "buffer NULL")
    refused(-2, b"stream is NULL", b, None, "stream NULL")
    for code, field in ((-110, "num_envs"), (-111, "slots_per_env"), (-112, "episode_limit"), (-113, "n_agents"), (-114, "obs_dim")):
        for value in (0, -3):
            b, s = _structs()
            setattr(b, field, value)
            refused(code, b"buffer." + field.encode(), b, s, (field, value))
    for value in (0, -1):
        b, s = _structs()
        s.T = value
        refused(-115, b"stream.T", b, s, ("T", value))
    b, s = _structs()
    b.num_envs, b.slots_per_env, b.episode_limit = 1 << 20, 4, 1 << 9            # 2^31 rows of one element and more
    refused(-116, b"buffer.num_envs * slots_per_env * (episode_limit + 1) * n_agents * obs_dim", b, s, "buffer range")
    b, s = _structs()
    b.num_envs, b.slots_per_env, b.episode_limit, b.n_agents, b.obs_dim = 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1
    refused(-116, b"buffer.num_envs * slots_per_env * (episode_limit + 1) * n_agents * obs_dim", b, s, "buffer range, every factor huge")
    b, s = _structs()
    b.num_envs, b.episode_limit, b.slots_per_env, s.T = 1 << 16, 1, 1, 1 << 11    # the buffer fits, the stream's obs does not
    refused(-117, b"(stream.T + 1) * buffer.num_envs * n_agents * obs_dim", b, s, "stream range")
    for i, f in enumerate(BUFFER_FIELDS):
        b, s = _structs()
        setattr(b, f, None)
        refused(-120 - i, b"buffer." + f.encode() + b" is NULL", b, s, f)
        if f in WORD_FIELDS:
            b, s = _structs()
            setattr(b, f, getattr(b, f) + 2)
            refused(-150 - i, b"buffer." + f.encode() + b" must be 4-byte aligned", b, s, f)
    for i, f in enumerate(STREAM_FIELDS):
        b, s = _structs()
        setattr(s, f, None)
        refused(-131 - i, b"stream." + f.encode() + b" is NULL", b, s, f)
        if f in WORD_FIELDS:
            b, s = _structs()
            setattr(s, f, getattr(s, f) + 1)
            refused(-161 - i, b"stream." + f.encode() + b" must be 4-byte aligned", b, s, f)
    b, s = _structs(with_prob=True)
    s.prob = None
    refused(-136, b"stream.prob is NULL", b, s, "prob in the buffer only")
    b, s = _structs(with_prob=True)
    b.prob = None
    refused(-137, b"buffer.prob is NULL", b, s, "prob in the stream only")
    b, s = _structs(with_prob=True)
    b.prob += 2
    refused(-166, b"buffer.prob must be 4-byte aligned", b, s, "buffer.prob alignment")
    b, s = _structs(with_prob=True)
    s.prob += 3
    refused(-167, b"stream.prob must be 4-byte aligned", b, s, "stream.prob alignment")
    assert len(seen) >= 35


# ---------------------------------------------------------------- Python argument errors that need no device
def _cpu_buffer(**kw):
    from marbler_amd.episodes import EpisodeBuffer
    args = dict(num_envs=4, n_agents=2, obs_dim=3, n_actions=5, episode_limit=6, device="cpu")
    args.update(kw)
    return EpisodeBuffer(**args)


def _cpu_batch(T=7, E=4, N=2, D=3, prob=False):
    import torch
    out = {"obs": torch.zeros(T + 1, E, N, D), "actions": torch.zeros(T, E, N, dtype=torch.int32), "reward": torch.zeros(T, E),
           "terminated": torch.zeros(T, E, dtype=torch.bool), "episode_start": torch.zeros(T, E, dtype=torch.bool),
           "avail_actions": torch.ones(T + 1, E, N, 5, dtype=torch.int32)}
    if prob:
        out["prob"] = torch.zeros(T, E, N)
    return out


def test_construction_is_checked_and_allocates_everything_once():
    import torch
    from marbler_amd.episodes import ARRAYS, EpisodeBuffer
    buf = _cpu_buffer(slots_per_env=3, with_prob=True)
    assert buf.num_slots == 12 and buf.obs.shape == (12, 7, 2, 3) and buf.prob.shape == (12, 7, 2) and buf.cursor.shape == (4, 4)
    assert buf.cursor[:, 0].tolist() == [-1] * 4 and not buf.cursor[:, 1:].any() and not buf.obs.any() and not buf.filled.any()
    assert {k: str(getattr(buf, k).dtype).replace("torch.", "") for k in buf.names} == {k: ARRAYS[k][0] for k in ARRAYS}
    assert _cpu_buffer().prob is None and "prob" not in _cpu_buffer().names
    for field in ("num_envs", "n_agents", "obs_dim", "n_actions", "episode_limit", "slots_per_env"):
        with pytest.raises(ValueError, match=field):
            _cpu_buffer(**{field: 0})
        with pytest.raises(TypeError, match=field):
            _cpu_buffer(**{field: 2.0})
    with pytest.raises(ValueError, match="2\\^31"):
        EpisodeBuffer(1 << 20, 16, 64, 5, 80, device="meta")
    storage = {k: getattr(buf, k) for k in buf.names}
    assert EpisodeBuffer(4, 2, 3, 5, 6, slots_per_env=3, with_prob=True, device="cpu", storage=storage).obs is buf.obs
    with pytest.raises(ValueError, match="storage"):
        EpisodeBuffer(4, 2, 3, 5, 6, slots_per_env=3, device="cpu", storage=storage)                   # prob, but with_prob=False
    with pytest.raises(ValueError, match="shape"):
        EpisodeBuffer(4, 2, 3, 5, 6, slots_per_env=2, with_prob=True, device="cpu", storage=storage)
    with pytest.raises(ValueError, match="int32"):
        EpisodeBuffer(4, 2, 3, 5, 6, slots_per_env=3, with_prob=True, device="cpu", storage=dict(storage, length=buf.length.to(torch.int64)))


def test_append_checks_the_batch_before_it_touches_a_device():
    import torch
    buf = _cpu_buffer()
    assert buf.check_stream(_cpu_batch()) == 7
    with pytest.raises(ValueError, match="no host path"):          # a good batch: the only thing wrong is that there is no device
        buf.append(_cpu_batch())
    with pytest.raises(TypeError):
        buf.append([_cpu_batch()])
    for missing in ("obs", "actions", "reward", "terminated", "episode_start"):
        batch = _cpu_batch()
        del batch[missing]
        with pytest.raises(ValueError, match=missing):
            buf.append(batch)
    for key, bad, word in (("obs", torch.zeros(8, 4, 2, 4), "shape"), ("obs", torch.zeros(7, 4, 2, 3), "shape"),
                           ("obs", torch.zeros(8, 4, 2, 3, dtype=torch.float64), "float32"),
                           ("obs", torch.zeros(8, 4, 2, 6)[..., ::2], "contiguous"),
                           ("obs", torch.zeros(8, 4, 2, 3, device="meta"), "is on meta"),
                           ("actions", torch.zeros(7, 4, 2, dtype=torch.int64), "int32"), ("actions", torch.zeros(7, 4, dtype=torch.int32), "T, E, N"),
                           ("actions", torch.zeros(0, 4, 2, dtype=torch.int32), "T >= 1"),
                           ("reward", torch.zeros(7, 4, 1), "shape"), ("reward", torch.zeros(4, 7).t(), "contiguous"),
                           ("terminated", torch.zeros(7, 4), "bool"), ("terminated", torch.zeros(7, 5, dtype=torch.bool), "shape"),
                           ("episode_start", torch.zeros(7, 4, dtype=torch.int32), "bool"),
                           ("episode_start", torch.zeros(6, 4, dtype=torch.uint8), "shape")):
        batch = _cpu_batch()
        batch[key] = bad
        with pytest.raises(ValueError, match=word):
            buf.append(batch)
    with pytest.raises(ValueError, match="with_prob=False"):
        buf.append(_cpu_batch(prob=True))
    with pytest.raises(ValueError, match="no 'prob'"):
        _cpu_buffer(with_prob=True).append(_cpu_batch())
    batch = _cpu_batch(prob=True)
    batch["prob"] = torch.zeros(7, 4, 3)
    with pytest.raises(ValueError, match="shape"):
        _cpu_buffer(with_prob=True).append(batch)


def test_batch_sample_and_checkpoints_on_host_tensors():
    import torch
    buf = _cpu_buffer(with_prob=True)
    buf.length[3], buf.complete[3], buf.filled[3, :5], buf.fresh[3] = 4, 1, 1, 1
    buf.length[6], buf.complete[6], buf.filled[6, :3], buf.fresh[6] = 2, 1, 1, 1
    out = buf.batch([6, 3])
    shapes = {"obs": (2, 7, 2, 3), "state": (2, 7, 6), "actions": (2, 7, 2, 1), "avail_actions": (2, 7, 2, 5), "reward": (2, 7, 1),
              "terminated": (2, 7, 1), "filled": (2, 7, 1), "probs": (2, 7, 2), "length": (2,), "episode_return": (2,)}
    dtypes = {"obs": torch.float32, "state": torch.float32, "actions": torch.int64, "avail_actions": torch.int32,
              "reward": torch.float32, "terminated": torch.uint8, "filled": torch.int64, "probs": torch.float32,
              "length": torch.int32, "episode_return": torch.float32}
    assert {k: tuple(v.shape) for k, v in out.items()} == shapes and {k: v.dtype for k, v in out.items()} == dtypes
    assert out["length"].tolist() == [2, 4] and out["filled"][:, :, 0].sum(1).tolist() == [3, 5] and bool(out["avail_actions"].all())
    assert buf.batch([6, 3], trim=True)["obs"].shape == (2, 5, 2, 3) and buf.batch([6], trim=True)["filled"].shape == (1, 3, 1)
    assert buf.batch()["length"].tolist() == [4, 2]                             # None: the complete slots, ascending
    assert "probs" not in _cpu_buffer().batch([0])
    for bad in ([8], [-1], torch.tensor([0, 9]), torch.tensor([0.0]), torch.zeros(2, 2, dtype=torch.int64), 3):
        with pytest.raises(ValueError):
            buf.batch(bad)
    assert buf.take_new().tolist() == [3, 6] and buf.take_new().dtype == torch.int64 and buf.take_new().numel() == 0
    for bad in (0, -1, 2.0, True, 9):
        with pytest.raises(ValueError):
            buf.sample(bad)
    with pytest.raises(ValueError, match="only 2 slots"):
        buf.sample(3)
    gen = torch.Generator().manual_seed(5)
    first = buf.sample(2, generator=gen)
    assert sorted(first.tolist()) == [3, 6] and torch.equal(first, buf.sample(2, generator=torch.Generator().manual_seed(5)))
    assert int(buf.overflowed()) == 0
    # a checkpoint keeps everything, cursors included
    buf.cursor[1] = torch.tensor([2, 3, 1, 0], dtype=torch.int32)
    state = buf.state_dict()
    assert set(state) == set(buf.names) | {"dims"} and state["obs"] is not buf.obs
    other = _cpu_buffer(with_prob=True)
    other.load_state_dict(state)
    assert all(torch.equal(getattr(other, k), getattr(buf, k)) for k in buf.names)
    with pytest.raises(ValueError, match="dims"):
        _cpu_buffer(with_prob=True, episode_limit=7).load_state_dict(state)
    with pytest.raises(ValueError, match="with_prob"):
        _cpu_buffer().load_state_dict(state)


def test_run_into_refuses_a_buffer_that_does_not_fit_before_it_collects():
    from marbler_amd.gymma import BatchedRunner
    runner = object.__new__(BatchedRunner)          # shapes only: a venv that cannot step
    runner.venv = types.SimpleNamespace(E=4, n_agents=2, obs_size=3, n_actions=5, episode_limit=6, env=types.SimpleNamespace(device="cpu"))
    runner.action_selector, runner.test_mode = "epsilon_greedy", False
    for kw, word in ((dict(num_envs=5), "num_envs"), (dict(n_agents=3), "n_agents"), (dict(obs_dim=4), "obs_dim"),
                     (dict(episode_limit=5), "episode_limit"), (dict(with_prob=True), "with_prob")):
        with pytest.raises(ValueError, match=word):
            runner.run(8, into=_cpu_buffer(**kw))
    runner.action_selector = "soft_policies"
    with pytest.raises(ValueError, match="with_prob"):
        runner.run(8, into=_cpu_buffer())
    runner.test_mode = True                         # the soft selector's test mode returns no prob
    with pytest.raises(ValueError, match="with_prob"):
        runner.run(8, into=_cpu_buffer(with_prob=True))
    _cpu_buffer(episode_limit=9).check_fits(4, 2, 3, 6, False)      # a longer buffer fits


def test_for_runner_takes_the_venvs_shapes():
    from marbler_amd.episodes import EpisodeBuffer
    venv = types.SimpleNamespace(E=3, n_agents=2, obs_size=7, n_actions=5, episode_limit=4, env=types.SimpleNamespace(device="cpu"))
    buf = EpisodeBuffer.for_runner(types.SimpleNamespace(venv=venv, action_selector="soft_policies", test_mode=False), slots_per_env=3)
    assert (buf.E, buf.N, buf.D, buf.A, buf.L, buf.R, buf.with_prob) == (3, 2, 7, 5, 4, 3, True)
    assert not EpisodeBuffer.for_runner(types.SimpleNamespace(venv=venv, action_selector="epsilon_greedy", test_mode=False)).with_prob
