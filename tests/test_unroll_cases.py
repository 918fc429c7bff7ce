"""rg_actor_unroll without a device: the binding, every refusal of the C entry point (host pointers that are never dereferenced:
every check comes before the first HIP call) and every ValueError of BatchedActor.unroll / EpisodeBuffer.unroll on CPU tensors."""
import ctypes
import re

import pytest
import torch

from gpu_helpers import random_actor

NAMES = ("rg_actor_unroll", "rg_sizeof_actor_unroll_io", "rg_actor_unroll_last_error")


def test_entry_points_are_exported_declared_and_the_struct_matches():
    from marbler_amd import _lib
    lib = _lib.load()
    header = open(_lib.__file__.replace("marbler_amd/_lib.py", "include/robogym.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS and name in _lib.LATE_QUERIES
        assert re.search(r"\b%s\(" % name, header), name
    assert "rg_actor_unroll_io" in header and hasattr(_lib, "RgActorUnrollIO")
    assert lib.rg_sizeof_actor_unroll_io() == ctypes.sizeof(_lib.RgActorUnrollIO) == 72
    assert lib.rg_abi_version() == 7
    assert "robogym_actor_unroll.hip" in __import__("marbler_amd.build", fromlist=["SOURCES"]).SOURCES


WEIGHTS = ("w1", "b1", "wih", "bih", "whh", "bhh", "w2", "b2")


def _structs():
    """A call the entry point accepts up to the launch: N = 4, D = 12 (+ 4), H = 64, A = 5, B = 3 episodes of 7 rows in 9."""
    from marbler_amd import _lib
    w, io = _lib.RgActorWeights(), _lib.RgActorUnrollIO()
    for i, f in enumerate(WEIGHTS):
        setattr(w, f, 0x10000 * (i + 1))
    w.n_sets, w.input_dim, w.hidden_dim, w.n_actions, w.use_rnn, w.gru_packed = 1, 16, 64, 5, 1, 3
    io.obs, io.q, io.actions, io.hidden_in, io.hidden_out = 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
    io.num_episodes, io.n_agents, io.obs_dim, io.rows, io.obs_pitch, io.out_pitch, io.append_agent_id, io.reserved = 3, 4, 12, 7, 9, 8, 1, 0
    return w, io


def test_rg_actor_unroll_refuses_every_bad_argument_before_touching_a_device():
    from marbler_amd import _lib
    lib = _lib.load()
    seen = {}

    def refused(word, w, io, what):
        rc = lib.rg_actor_unroll(ctypes.byref(w) if w is not None else None, ctypes.byref(io) if io is not None else None, None)
        msg = lib.rg_actor_unroll_last_error()
        assert rc < 0 and rc != -30, (what, rc, msg)
        assert msg.startswith(b"rg_actor_unroll: ") and word in msg, (what, rc, msg)
        seen.setdefault(rc, []).append(what)
        return rc

    def case(word, what, **change):
        w, io = _structs()
        for k, v in change.items():
            setattr(w if k in dict(w._fields_) else io, k, v)
        return refused(word, w, io, what)

    w, io = _structs()
    assert refused(b"w is NULL", None, io, "w") == -1
    assert refused(b"io is NULL", w, None, "io") == -2
    assert case(b"io.obs is NULL", "obs", obs=None) == -3
    assert {case(b"w." + f.encode() + b" is NULL", f, **{f: None}) for f in WEIGHTS} == {-4}
    assert case(b"binary16", "use_rnn", use_rnn=0) == case(b"binary16", "gru_packed", gru_packed=2) == -5
    assert case(b"w.use_rnn", "use_rnn", use_rnn=0) == case(b"w.gru_packed", "gru_packed 0", gru_packed=0) == -5
    assert {case(b"w.hidden_dim", ("hidden_dim", h), hidden_dim=h) for h in (0, 32, 96, 256)} == {-6}
    assert {case(b"w.n_actions", ("n_actions", a), n_actions=a) for a in (0, -1, 33)} == {-7}
    assert {case(b"w.n_sets", ("n_sets", s), n_sets=s) for s in (0, 2, 3, 5)} == {-8}
    for code, f in ((-9, "num_episodes"), (-10, "n_agents"), (-11, "obs_dim"), (-12, "rows")):
        assert {case(b"io." + f.encode(), (f, v), **{f: v}) for v in (0, -3)} == {code}
    assert case(b"w.input_dim", "width without the id", append_agent_id=0) == -13
    assert case(b"w.input_dim", "width", obs_dim=13) == -13
    assert case(b"above 64", "padded width", obs_dim=61, input_dim=65) == -14
    assert case(b"above 64", "padded width, no id", obs_dim=65, input_dim=65, append_agent_id=0) == -14
    assert case(b"io.obs_pitch", "obs_pitch", obs_pitch=6) == -15
    assert case(b"io.out_pitch", "out_pitch", out_pitch=6) == -16
    assert case(b"io.reserved", "reserved", reserved=1) == -17
    assert case(b"io.q, io.actions and io.hidden_out", "no output", q=None, actions=None, hidden_out=None) == -18
    for f in ("hidden_in", "hidden_out", "w1", "wih", "whh", "w2"):
        assert {case((b"w." if f.startswith("w") else b"io.") + f.encode() + b" must be 16-byte aligned", (f, off),
                     **{f: 0x700000 + off}) for off in (4, 8)} == {-19}
    word = b"io.num_episodes * pitch * n_agents * max(obs_dim, n_actions)"
    assert case(word, "range: obs", num_episodes=1 << 16, obs_pitch=1 << 10, obs_dim=12) == -20          # 2^26 x 4 x 12
    assert case(word, "range: q", num_episodes=1 << 16, out_pitch=1 << 11, n_actions=5) == -20           # 2^27 x 4 x 12
    assert case(word, "range: every factor huge", num_episodes=2 ** 31 - 1, rows=2 ** 31 - 1, obs_pitch=2 ** 31 - 1,
                out_pitch=2 ** 31 - 1) == -20
    assert sorted(seen) == list(range(-20, 0)), sorted(seen)
    # what the call above all but launched: only one output is required
    for keep in ("q", "actions", "hidden_out"):
        w, io = _structs()
        for f in {"q", "actions", "hidden_out"} - {keep}:
            setattr(io, f, None)
        io.reserved = 1
        assert refused(b"io.reserved", w, io, keep) == -17


# ---------------------------------------------------------------- Python argument errors that need no device
def _cpu_actor(N=3, D=5, H=64, A=6, append=True, **kw):
    from marbler_amd.evaluate import BatchedActor
    use_rnn = kw.pop("use_rnn", True)
    return BatchedActor(random_actor(1, D + (N if append else 0), H, A, use_rnn, seed=1), N, use_rnn=use_rnn, **kw)


def test_batched_actor_unroll_value_errors():
    actor = _cpu_actor()
    obs = torch.zeros(4, 7, 3, 5)
    with pytest.raises(ValueError, match="no host path"):                 # everything right but the device
        actor.unroll(obs)
    with pytest.raises(ValueError, match="no host path"):
        actor.unroll(torch.zeros(4, 9, 3, 5)[:, :7], q_out=torch.zeros(4, 8, 3, 6)[:, :7], actions_out=torch.zeros(4, 8, 3, dtype=torch.int32)[:, :7],
                     hidden=torch.zeros(4, 3, 64), hidden_out=torch.zeros(4, 3, 64))
    bad = {"dtype": dict(obs=obs.double()), "not a tensor": dict(obs=obs.numpy()), "three dimensions": dict(obs=obs[0]),
           "no episode": dict(obs=obs[:0]), "no row": dict(obs=obs[:, :0]), "agents": dict(obs=torch.zeros(4, 7, 2, 5)),
           "width": dict(obs=torch.zeros(4, 7, 3, 6)), "width without the id": dict(obs=obs, append_agent_id=False),
           "transposed": dict(obs=torch.zeros(7, 4, 3, 5).transpose(0, 1)), "row stride": dict(obs=torch.zeros(4, 7, 3, 10)[..., ::2]),
           "agent stride": dict(obs=torch.zeros(4, 7, 6, 5)[:, :, ::2]), "time stride": dict(obs=torch.zeros(4, 14, 3, 5)[:, ::2]),
           "batch stride not a multiple of a row": dict(obs=torch.zeros(4, 7 * 15 + 4)[:, :7 * 15].view(4, 7, 3, 5)),
           "overlapping episodes": dict(obs=torch.zeros(10, 3, 5).unfold(0, 7, 1).permute(0, 3, 1, 2)),
           "q shape": dict(obs=obs, q_out=torch.zeros(4, 7, 3, 5)), "q dtype": dict(obs=obs, q_out=torch.zeros(4, 7, 3, 6).double()),
           "q stride": dict(obs=obs, q_out=torch.zeros(7, 4, 3, 6).transpose(0, 1)),
           "actions dtype": dict(obs=obs, actions_out=torch.zeros(4, 7, 3, dtype=torch.int64)),
           "actions shape": dict(obs=obs, actions_out=torch.zeros(4, 7, 3, 1, dtype=torch.int32)),
           "two output pitches": dict(obs=obs, q_out=torch.zeros(4, 8, 3, 6)[:, :7], actions_out=torch.zeros(4, 7, 3, dtype=torch.int32)),
           "hidden shape": dict(obs=obs, hidden=torch.zeros(4, 3, 32)), "hidden dtype": dict(obs=obs, hidden=torch.zeros(4, 3, 64).half()),
           "hidden stride": dict(obs=obs, hidden=torch.zeros(4, 3, 128)[..., ::2]),
           "hidden_out shape": dict(obs=obs, hidden_out=torch.zeros(3, 4, 64)),
           "meta device": dict(obs=obs.to("meta")), "q device": dict(obs=obs, q_out=torch.zeros(4, 7, 3, 6, device="meta")),
           "hidden device": dict(obs=obs, hidden=torch.zeros(4, 3, 64, device="meta"))}
    for what, kw in bad.items():
        with pytest.raises(ValueError) as err:
            actor.unroll(**kw)
        assert "no host path" not in str(err.value), what
    # actors the launch refuses: said before anything else is looked at
    for what, other in (("binary16", _cpu_actor(pack_gru="bf16x3")), ("binary16", _cpu_actor(pack_gru=False)),
                        ("binary16", _cpu_actor(use_rnn=False)), ("hidden size", _cpu_actor(H=32)),
                        ("n_actions", _cpu_actor(A=33)), ("above 64", _cpu_actor(N=3, D=62))):
        with pytest.raises(ValueError, match=what):
            other.unroll(torch.zeros(4, 7, 3, other.input_dim - 3))


def test_episode_buffer_unroll_value_errors():
    from marbler_amd.episodes import EpisodeBuffer
    buf = EpisodeBuffer(num_envs=4, n_agents=3, obs_dim=5, n_actions=6, episode_limit=6, device="cpu")
    buf.complete[:3] = 1
    buf.length[:3] = 4
    with pytest.raises(ValueError, match="no host path"):
        buf.unroll(_cpu_actor())
    with pytest.raises(ValueError, match="no host path"):
        buf.unroll(_cpu_actor(append=False), slots=[0, 5], trim=True, obs_agent_id=False)
    for what, actor, kw in (("n_agents", _cpu_actor(N=2, D=6), {}), ("n_actions", _cpu_actor(A=5), {}), ("input_dim", _cpu_actor(D=4), {}),
                            ("input_dim", _cpu_actor(), dict(obs_agent_id=False)), ("input_dim", _cpu_actor(append=False), {}),
                            ("binary16", _cpu_actor(pack_gru="f32"), {}), ("outside", _cpu_actor(), dict(slots=[8])),
                            ("slots", _cpu_actor(), dict(slots=torch.zeros(2)))):
        with pytest.raises(ValueError, match=what):
            buf.unroll(actor, **kw)
    with pytest.raises(ValueError, match="the buffer on"):
        actor = _cpu_actor()
        actor.w1 = actor.w1.to("meta")
        buf.unroll(actor)
    empty = EpisodeBuffer(num_envs=4, n_agents=3, obs_dim=5, n_actions=6, episode_limit=6, device="cpu").unroll(_cpu_actor())
    assert tuple(empty["q"].shape) == (0, 7, 3, 6) and tuple(empty["greedy"].shape) == (0, 7, 3) and empty["greedy"].dtype == torch.int32
