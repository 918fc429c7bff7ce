"""rg_nstep_returns without a device: the rule's twin on the worked example and on hand-written episodes, the float32 twin against
EPyMARL's double loop in torch word for word, TargetCritic.forward against the float64 twin, the weight packing, the binding, every
refusal of the C entry point (host pointers that are never dereferenced: every check comes before the first HIP call) and every
ValueError of TargetCritic / nstep_returns / EpisodeBuffer.nstep_returns on CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import nstep_returns_twin as tw

NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rg_nstep_returns", "rg_sizeof_nstep_returns_io", "rg_sizeof_critic_weights", "rg_nstep_returns_last_error")


def words(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


# ---------------------------------------------------------------- the rule, by hand
def test_the_twin_on_the_worked_example():
    reward, values = np.array([[1.0, 2.0, 4.0, NAN]], np.float32), np.array([[[10.0], [20.0], [40.0], [80.0]]], np.float32)
    live = tw.mask_of(np.zeros((1, 4), np.uint8), np.ones((1, 4), np.uint8), 4)
    assert live.tolist() == [[True, True, True]]
    assert tw.returns32(values, reward, live, 0.5, 2, True)[0, :, 0].tolist() == [12.0, 24.0, 44.0]
    assert tw.returns32(values, reward, live, 0.5, 2, False)[0, :, 0].tolist() == [12.0, 4.0, 4.0]
    term, fill = np.array([[0, 1, 0, 0]], np.uint8), np.array([[1, 1, 1, 0]], np.uint8)
    m = tw.mask_of(term, fill, 4)
    assert m.tolist() == [[True, True, False]] and tw.needed_rows(m, True).tolist() == [[True, True, False, False]]
    poisoned = np.array([[[10.0], [20.0], [NAN], [NAN]]], np.float32)                      # what the rule does not read
    assert tw.returns32(poisoned, np.array([[1.0, 2.0, NAN, NAN]], np.float32), m, 0.5, 2, True)[0, :, 0].tolist() == [2.0, 2.0, 0.0]
    # EPyMARL adds the padding row's value in the middle: 2 + 0.25 * 80
    ep = tw.epymarl_nstep_returns(torch.tensor([[[1.0], [2.0], [4.0]]]), torch.tensor([[[1.0], [1.0], [0.0]]]), torch.from_numpy(values), 2, 0.5, True)
    assert ep[0, :, 0].tolist() == [2.0, 22.0, 40.0]
    assert tw.discounts(0.5, 2).tolist() == [1.0, 0.5, 0.25, 0.125]


def test_the_twin_on_hand_written_episodes():
    """rows = 4 (T = 3), N = 2, gamma 0.5, n = 2.  Episodes: length 1 (terminated at t = 0); terminated at the last data row
    t = 2; force-closed (all rows filled, never terminated); an empty slot.  NaN wherever the rule says nothing is read."""
    terminated = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]], np.uint8)
    filled = np.array([[1, 1, 0, 0], [1, 1, 1, 1], [1, 1, 1, 1], [0, 0, 0, 0]], np.uint8)
    m = tw.mask_of(terminated, filled, 4)
    assert m.tolist() == [[True, False, False], [True, True, True], [True, True, True], [False, False, False]]
    assert tw.needed_rows(m, True)[:, 3].tolist() == [False, True, True, False] and not tw.needed_rows(m, False)[:, 3].any()
    reward = np.array([[3.0, NAN, NAN, NAN], [1.0, 2.0, 4.0, NAN], [1.0, 2.0, 4.0, NAN], [NAN] * 4], np.float32)
    values = np.full((4, 4, 2), NAN, np.float32)
    values[0, 0] = [7.0, 9.0]
    values[1] = values[2] = [[10.0, 1.0], [20.0, 2.0], [40.0, 4.0], [80.0, 8.0]]
    ret = tw.returns32(values, reward, m, 0.5, 2, True)
    assert ret[0].tolist() == [[3.0, 3.0], [0.0, 0.0], [0.0, 0.0]]                         # its one reward; padding behind it
    # (the value of row T belongs to the last data row whether or not the episode terminated there: EPyMARL's rule and this one)
    assert ret[1].tolist() == ret[2].tolist() == [[12.0, 3.0], [24.0, 6.0], [44.0, 8.0]]
    assert ret[3].tolist() == [[0.0, 0.0]] * 3 and ret.dtype == np.float32 and not np.signbit(ret[3]).any()
    off = tw.returns32(values, reward, m, 0.5, 2, False)
    assert off[1].tolist() == [[12.0, 3.0], [4.0, 4.0], [4.0, 4.0]] and off[0].tolist() == ret[0].tolist()
    one = tw.returns32(values, reward, m, 0.5, 1, True)                                   # n = 1: reward + gamma V(t + 1)
    assert one[1].tolist() == [[11.0, 2.0], [22.0, 4.0], [44.0, 8.0]]
    far = tw.returns32(values, reward, m, 0.5, 20, True)                                  # n above T: the whole tail and the last value
    assert far[1, 0].tolist() == [1.0 + 1.0 + 1.0 + 10.0, 1.0 + 1.0 + 1.0 + 1.0]


def test_products_are_rounded_before_sums():
    # with a fused multiply-add the second term would leave -2^-25; the rule says 0 (g = 1 - 2^-13, x = 1 + 2^-12: g x rounds to 1 + 2^-13)
    g, x = 1.0 - 2.0 ** -13, 1.0 + 2.0 ** -12
    values = np.array([[[0.0], [x], [0.0]]], np.float32)
    reward = np.array([[-(1.0 + 2.0 ** -13), 0.0, 0.0]], np.float32)
    m = np.ones((1, 2), bool)
    assert tw.returns32(values, reward, m, g, 1, False)[0, 0, 0] == 0.0
    assert tw.discounts(0.99, 3)[3] == np.float32(float(np.float32(0.99)) ** 3)


def _random_case(B, rows, N, seed):
    rng = np.random.default_rng(seed)
    reward = rng.standard_normal((B, rows)).astype(np.float32)
    values = rng.standard_normal((B, rows, N)).astype(np.float32) * 3
    length = rng.integers(1, rows, B)
    t = np.arange(rows)[None]
    filled = (t <= length[:, None]).astype(np.uint8)
    terminated = ((t == length[:, None] - 1) & (rng.random(B) < 0.6)[:, None]).astype(np.uint8)
    return reward, values, terminated, filled


@pytest.mark.parametrize("add", [True, False])
@pytest.mark.parametrize("n", [1, 5, 10, 20])
def test_the_float32_twin_equals_epymarls_double_loop_word_for_word(n, add):
    B, rows, N, gamma = 80, 13, 3, 0.99
    reward, values, terminated, filled = _random_case(B, rows, N, 7 + n)
    m = tw.mask_of(terminated, filled, rows)
    mine = tw.returns32(values, reward, m, gamma, n, add)
    mask_t = torch.from_numpy(m.astype(np.float32))[..., None].repeat(1, 1, N)
    ep = tw.epymarl_nstep_returns(torch.from_numpy(reward[:, :-1, None]), mask_t, torch.from_numpy(values), n, float(np.float32(gamma)), add).numpy()
    differs, k = tw.differing_rows(m, n, add)
    same = m & ~differs
    assert same.sum() >= 20 and np.array_equal(words(mine[same]), words(ep[same]))
    assert not mine[~m].any()
    if add and n > 1:     # (n = 1: the window of a live row never reaches a dead row T - 1)
        assert differs.sum() >= 5
        g = tw.discounts(gamma, n)
        term = (g[np.minimum(k + 1, n + 1)][..., None] * values[:, -1][:, None, :]).astype(np.float32)          # fl(g[k + 1] values[T])
        assert np.array_equal(words((mine + term).astype(np.float32)[differs]), words(ep[differs]))
        assert not np.array_equal(words(mine[differs]), words(ep[differs]))
    else:
        assert not differs.any()


# ---------------------------------------------------------------- the critic
@pytest.mark.parametrize("kind", ["cv", "cv_ns"])
@pytest.mark.parametrize("H", [64, 128])
def test_target_critic_forward_against_the_float64_twin(kind, H):
    from marbler_amd.returns import TargetCritic
    N, D = 3, 5
    critic = TargetCritic(kind, N, N * D, H, device="cpu", seed=3)
    state = torch.rand(4, 6, N * D, generator=torch.Generator().manual_seed(1)) * 2 - 1
    got = critic.forward(state)
    assert tuple(got.shape) == (4, 6, N)
    ref = tw.critic64(kind, {k: v.numpy() for k, v in critic.state_dict().items()}, state.reshape(-1, N * D).numpy(), N).reshape(4, 6, N)
    assert tw.rel_err(got.numpy(), ref, np.ones((4, 6), bool)) < 2e-6                      # float32 against float64 over K <= 128 terms
    assert float(np.abs(ref).max()) > 1e-3 and np.abs(ref[..., 0] - ref[..., 1]).max() > 1e-4   # the agents' values differ
    p64 = {k: v.double() for k, v in critic.params.items()}
    critic.params = p64
    assert tw.rel_err(critic.forward(state.double()).numpy(), ref, np.ones((4, 6), bool)) < 1e-13


@pytest.mark.parametrize("kind", ["cv", "cv_ns"])
@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("N,S", [(2, 2), (5, 45), (8, 144), (3, 255)])
def test_packing_round_trips_and_pads_the_state_with_zero_rows(kind, H, N, S):
    from marbler_amd import returns
    critic = returns.TargetCritic(kind, N, S, H, device="cpu", seed=N)
    sd = critic.state_dict()
    one = returns.critic_shapes(kind, N, S, H)
    assert len(sd) == (1 if kind == "cv" else N) * 6 and one["fc1.weight"] == (H, S + (N if kind == "cv" else 0))
    back = critic.unpack()
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    layout, net_len = returns.packed_layout(kind, N, S, H)
    sp = (S + 7) // 8 * 8
    assert layout["w1"] == (0, (sp, H)) and all(off % 4 == 0 for off, _ in layout.values()) and net_len % 4 == 0
    assert critic.packed.numel() == net_len * (1 if kind == "cv" else N) and ("w1_id" in layout) == (kind == "cv")
    last = N - 1 if kind == "cv_ns" else 0
    pre = f"critics.{last}." if kind == "cv_ns" else ""
    w1 = critic.packed[last * net_len:last * net_len + sp * H].view(sp, H)
    assert bool((w1[S:] == 0).all()) and torch.equal(w1[:S], sd[pre + "fc1.weight"][:, :S].t())          # K-major: [in][out]
    off = last * net_len + layout["w2"][0]
    assert torch.equal(critic.packed[off:off + H * H].view(H, H), sd[pre + "fc2.weight"].t())
    assert float(sd[pre + "fc2.weight"].abs().max()) <= H ** -0.5 and float(sd[pre + "fc3.bias"].abs().max()) <= H ** -0.5
    ptr, w = critic.packed.data_ptr(), critic.weights_struct()
    critic.load_state_dict({k: 0.5 * v for k, v in sd.items()})
    assert critic.packed.data_ptr() == ptr and torch.equal(critic.unpack()[pre + "fc3.weight"], 0.5 * sd[pre + "fc3.weight"])
    assert w.w1 == ptr and w.b3 == ptr + 4 * layout["b3"][0] and all(getattr(w, k) % 16 == 0 for k in layout)
    assert (w.kind, w.n_agents, w.state_dim, w.hidden_dim, w.reserved) == (0 if kind == "cv" else 1, N, S, H, 0)
    assert w.net_stride == (0 if kind == "cv" else net_len) and (w.w1_id is None) == (kind == "cv_ns")
    if kind == "cv_ns":   # a list of per-network dicts is the same critic
        nets = [{k: sd[f"critics.{i}.{k}"] for k in one} for i in range(N)]
        assert torch.equal(returns.TargetCritic(kind, N, S, H, nets, device="cpu").packed, returns.TargetCritic(kind, N, S, H, sd, device="cpu").packed)


def test_target_critic_value_errors():
    from marbler_amd.returns import TargetCritic
    good = TargetCritic("cv", 3, 15, 64, device="cpu").state_dict()
    for what, args in (("kind", ("ac", 3, 15)), ("n_agents", ("cv", 0, 15)), ("n_agents", ("cv", 17, 15)), ("n_agents", ("cv", True, 15)),
                       ("state_dim", ("cv", 3, 0)), ("state_dim", ("cv", 3, 2.5)), ("above 256", ("cv", 3, 257)),
                       ("hidden_dim", ("cv", 3, 15, 32)), ("hidden_dim", ("cv_ns", 3, 15, 256)), ("hidden_dim", ("cv", 3, 15, 128.0))):
        with pytest.raises(ValueError, match=what):
            TargetCritic(*args, device="cpu")
    bad = {"lacks": {k: v for k, v in good.items() if k != "fc3.bias"},
           "fc1.weight": dict(good, **{"fc1.weight": torch.zeros(64, 15)}),                       # a cv_ns network's fc1
           "fc2.weight": dict(good, **{"fc2.weight": torch.zeros(128, 128)}),                     # another hidden_dim
           "fc3.weight": dict(good, **{"fc3.weight": torch.zeros(64)}),
           "not finite": dict(good, **{"fc2.weight": torch.full((64, 64), float("inf"))}),
           "not finite ": dict(good, **{"fc1.bias": torch.full((64,), NAN)}),
           "floating-point": dict(good, **{"fc3.bias": torch.zeros(1, dtype=torch.int64)}),
           "must be a tensor": dict(good, **{"fc3.bias": [0.0]}),
           "must be a dict": [good]}
    for what, sd in bad.items():
        with pytest.raises(ValueError, match=what.strip()):
            TargetCritic("cv", 3, 15, 64, sd, device="cpu")
    critic = TargetCritic("cv", 3, 15, 64, good, device="cpu")
    before = critic.packed.clone()
    with pytest.raises(ValueError, match="not finite"):
        critic.load_state_dict(bad["not finite"])
    assert torch.equal(critic.packed, before), "a refused state dict must leave the packed weights alone"
    ns = TargetCritic("cv_ns", 3, 15, 64, device="cpu")
    with pytest.raises(ValueError, match="needs 3 state dicts"):
        ns.load_state_dict([good, good])
    with pytest.raises(ValueError, match="lacks"):
        ns.load_state_dict(good)                                                                  # a cv state dict
    with pytest.raises(ValueError, match="critics.0.fc1.weight"):
        ns.load_state_dict([{k: v for k, v in good.items()}] * 3)                                 # cv's fc1 is N columns too wide


# ---------------------------------------------------------------- the binding and the refusals
def test_entry_points_are_exported_declared_beside_robogym_h_and_the_structs_match():
    from marbler_amd import _lib
    import marbler_amd
    lib = _lib.load_returns()
    old, new = (open(os.path.join(ROOT, "include", h)).read() for h in ("robogym.h", "robogym_returns.h"))
    for name in NAMES:
        assert hasattr(lib, name) and name in [e[0] for e in _lib.RETURNS_ENTRIES]
        assert name not in _lib.EXPORTS and name not in _lib.LATE_QUERIES
        assert re.search(r"\b%s\(" % name, new), name
    assert "rg_nstep_returns" not in old and "rg_critic_weights" not in old and '#include "robogym.h"' in new
    assert lib.rg_sizeof_critic_weights() == ctypes.sizeof(_lib.RgCriticWeights) == 80
    assert lib.rg_sizeof_nstep_returns_io() == ctypes.sizeof(_lib.RgNstepReturnsIO) == 112
    assert lib.rg_abi_version() == _lib.ABI_VERSION == 7 and "#define RG_ABI_VERSION 7" in old
    assert "robogym_nstep_returns.hip" in __import__("marbler_amd.build", fromlist=["SOURCES"]).SOURCES
    assert marbler_amd.TargetCritic is __import__("marbler_amd.returns", fromlist=["x"]).TargetCritic and callable(marbler_amd.nstep_returns)
    assert {"TargetCritic", "nstep_returns"} <= set(marbler_amd.__all__) and hasattr(marbler_amd.EpisodeBuffer, "nstep_returns")


def test_a_library_without_the_entries_fails_only_when_the_feature_is_called(monkeypatch):
    from marbler_amd import _lib

    class Old(object):                        # a library of an earlier build: everything but the new entries
        def __getattr__(self, name):
            if name.startswith(("rg_nstep", "rg_sizeof_critic", "rg_sizeof_nstep")):
                raise AttributeError(name)
            return lambda *a: 0
    monkeypatch.setattr(_lib, "_lib", Old())
    monkeypatch.setattr(_lib, "_returns_ready", False)
    assert _lib.load() is not None
    with pytest.raises(_lib.RobogymError, match="rg_sizeof_critic_weights"):
        _lib.load_returns()


def test_the_rule_reads_the_same_in_the_header_and_in_design_md():
    texts = [open(os.path.join(ROOT, p)).read() for p in ("marbler_amd/csrc/nstep_returns.h", "DESIGN.md")]

    def rule(text):
        body = text[text.index("Inputs.\n", text.index("N-step returns")):]             # (DESIGN.md states other rules before this one)
        body = body[:body.index("the returns that the rule says read them.") + 41]
        lines = [re.sub(r"^\s*(//|\*)?\s*(- )?", "", ln).replace("`", "") for ln in body.splitlines()]    # comment marks, bullets
        return " ".join(" ".join(lines).split())                                                         # and line breaks aside
    assert rule(texts[0]) == rule(texts[1]) and len(rule(texts[0])) > 2500
    assert "WITHOUT the factor m[T-1]" in rule(texts[0])


WEIGHTS = ("w1", "w1_id", "b1", "w2", "b2", "w3", "b3")
ARRAYS = ("obs", "reward", "terminated", "filled", "returns", "values", "mask")


def _structs(kind=0):
    """A call the entry point accepts up to the launch: N = 4, D = 16, H = 128, B = 3 episodes of 7 rows."""
    from marbler_amd import _lib
    w, io = _lib.RgCriticWeights(), _lib.RgNstepReturnsIO()
    for i, f in enumerate(WEIGHTS):
        setattr(w, f, 0x10000 * (i + 1))
    w.kind, w.n_agents, w.state_dim, w.hidden_dim, w.net_stride, w.reserved = kind, 4, 64, 128, (0 if kind == 0 else 25092), 0
    if kind == 1:
        w.w1_id = None
    for i, f in enumerate(ARRAYS):
        setattr(io, f, 0x1000000 + 0x100000 * i)
    io.num_episodes, io.n_agents, io.obs_dim, io.rows, io.nstep, io.add_value_last_step = 3, 4, 16, 7, 5, 1
    io.obs_pitch, io.flag_pitch, io.out_pitch, io.value_pitch = 9, 8, 6, 7
    io.gamma, io.value_scale, io.value_shift, io.reserved = 0.99, 1.0, 0.0, 0
    return w, io


def test_rg_nstep_returns_refuses_every_bad_argument_before_touching_a_device():
    from marbler_amd import _lib
    lib = _lib.load_returns()
    seen = {}

    def refused(word, w, io, what):
        rc = lib.rg_nstep_returns(ctypes.byref(w) if w is not None else None, ctypes.byref(io) if io is not None else None, None)
        msg = lib.rg_nstep_returns_last_error()
        assert rc < 0 and rc != -30, (what, rc, msg)
        assert msg.startswith(b"rg_nstep_returns: ") and word in msg, (what, rc, msg)
        seen.setdefault(rc, []).append(what)
        return rc

    def case(word, what, kind=0, **change):
        w, io = _structs(kind)
        for k, v in change.items():
            setattr(w if k in dict(w._fields_) and k not in ("n_agents", "reserved") else io, k, v)
        return refused(word, w, io, what)

    w, io = _structs()
    assert refused(b"w is NULL", None, io, "w") == -1
    assert refused(b"io is NULL", w, None, "io") == -2
    for f in ("obs", "reward", "terminated", "filled", "returns", "values"):
        assert {case(b"io." + f.encode() + b" is NULL", (f, kind), kind, **{f: None}) for kind in (0, 1)} == {-3}
    assert {case(b"w.kind", ("kind", k), kind=k) for k in (-1, 2, 99)} == {-4}
    for f in WEIGHTS:
        assert case(b"w." + f.encode() + b" is NULL", f, **{f: None}) == -5
        assert {case(b"w." + f.encode() + b" must be 16-byte aligned", (f, off), **{f: 0x700000 + off}) for off in (4, 8, 12)} == {-6}
    assert {case(b"w.hidden_dim", ("hidden", h), hidden_dim=h) for h in (0, 32, 96, 256)} == {-7}
    w, io = _structs()
    w.n_agents = 5
    assert refused(b"w.n_agents", w, io, "w.n_agents") == -8
    assert case(b"w.state_dim", "state_dim", state_dim=60) == case(b"w.state_dim", "obs_dim against state_dim", obs_dim=15) == -9
    for code, f in ((-10, "num_episodes"), (-11, "rows"), (-13, "nstep"), (-14, "obs_dim")):
        assert {case(b"io." + f.encode(), (f, v), **{f: v}) for v in (0, -3)} == {code}
    assert case(b"io.rows", "one row", rows=1) == -11 and case(b"io.nstep", "33 steps", nstep=33) == -13
    for n in (0, -1, 17):
        w, io = _structs()
        w.n_agents = io.n_agents = n
        assert refused(b"io.n_agents", w, io, ("n_agents", n)) == -12
    assert case(b"wider than 256", "a wide state", obs_dim=65, state_dim=260) == -14
    assert case(b"io.obs_pitch", "obs_pitch", obs_pitch=6) == -15
    assert case(b"io.flag_pitch", "flag_pitch", flag_pitch=6) == -16
    assert case(b"io.value_pitch", "value_pitch", value_pitch=6) == -17
    assert case(b"io.out_pitch", "out_pitch", out_pitch=5) == -18
    assert {case(b"io.gamma", ("gamma", g), gamma=g) for g in (-0.01, 1.01, float("inf"), NAN)} == {-19}
    assert case(b"io.reserved", "io.reserved", reserved=1) == -20
    w, io = _structs()
    w.reserved = 2
    assert refused(b"w.reserved", w, io, "w.reserved") == -20
    assert case(b"obs_pitch * n_agents * obs_dim", "range: obs", num_episodes=1 << 22, obs_pitch=8) == -21          # 2^22 x 8 x 64
    assert case(b"io.num_episodes * flag_pitch", "range: flags", flag_pitch=1 << 30) == -21
    assert case(b"out_pitch * n_agents", "range: returns", num_episodes=1 << 20, out_pitch=1 << 9) == -21
    assert case(b"value_pitch * n_agents", "range: values", num_episodes=1 << 20, value_pitch=1 << 9) == -21
    assert case(b"w.net_stride * n_agents", "range: networks", kind=1, net_stride=1 << 29) == -21
    assert case(b"exceeds 2^31 - 1", "range: every factor huge", num_episodes=2 ** 31 - 1, obs_pitch=2 ** 31 - 1, flag_pitch=2 ** 31 - 1,
                out_pitch=2 ** 31 - 1, value_pitch=2 ** 31 - 1) == -21
    assert {case(b"io.add_value_last_step", ("flag", v), add_value_last_step=v) for v in (-1, 2)} == {-22}
    assert {case(b"io.value_scale", ("scale", v), value_scale=v) for v in (float("inf"), NAN)} == {-23}
    assert {case(b"io.value_shift", ("shift", v), value_shift=v) for v in (-float("inf"), NAN)} == {-23}
    assert case(b"w.net_stride must be 0", "cv with a stride", net_stride=4) == -24
    assert {case(b"w.net_stride", ("stride", v), kind=1, net_stride=v) for v in (0, -4, 25090)} == {-24}
    assert case(b"io.rows is above 4096", "too many rows", rows=4097, obs_pitch=4097, flag_pitch=4097, out_pitch=4096, value_pitch=4097) == -25
    assert sorted(seen) == list(range(-25, 0)), sorted(seen)
    # mask is optional, cv_ns has no w1_id, rows = 4096 and the edges of every range are taken: all of these reach the last check
    for kind in (0, 1):
        w, io = _structs(kind)
        io.mask = None
        io.rows, io.obs_pitch, io.flag_pitch, io.out_pitch, io.value_pitch = 4096, 4096, 4096, 4095, 4096
        io.nstep, io.gamma, io.add_value_last_step, w.hidden_dim = (1, 0.0, 0, 64) if kind else (32, 1.0, 1, 128)
        io.reserved = 1
        assert refused(b"io.reserved", w, io, ("optional", kind)) == -20


# ---------------------------------------------------------------- Python argument errors that need no device
def _call(B=4, rows=7, N=3, D=5, kind="cv"):
    from marbler_amd.returns import TargetCritic
    return dict(obs=torch.zeros(B, rows, N, D), reward=torch.zeros(B, rows), terminated=torch.zeros(B, rows, dtype=torch.uint8),
                filled=torch.ones(B, rows, dtype=torch.bool), critic=TargetCritic(kind, N, N * D, 64, device="cpu"), gamma=0.99, nstep=5)


def test_nstep_returns_value_errors():
    from marbler_amd.returns import TargetCritic, nstep_returns
    with pytest.raises(ValueError, match="no host path"):                 # everything right but the device
        nstep_returns(**_call())
    long = _call(rows=9, kind="cv_ns")
    with pytest.raises(ValueError, match="no host path"):
        nstep_returns(long["obs"][:, :7], long["reward"][:, :7], long["terminated"][:, :7], long["filled"][:, :7], long["critic"], 0.5, 32,
                      add_value_last_step=False, value_scale=1.7, value_shift=-0.3, returns_out=torch.zeros(4, 8, 3)[:, :6],
                      values_out=torch.zeros(4, 9, 3)[:, :7], mask_out=torch.zeros(4, 8)[:, :6])
    ok = _call()
    cut = lambda d, f: {k: (f(v) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}  # noqa: E731
    bad = {"critic": dict(critic=None), "obs dtype": dict(obs=ok["obs"].double()), "obs not a tensor": dict(obs=ok["obs"].numpy()),
           "obs three dimensions": dict(obs=ok["obs"][0]), "one row": cut(ok, lambda v: v[:, :1]), "no episode": cut(ok, lambda v: v[:0]),
           "too many rows": dict(obs=torch.zeros(1, 4097, 3, 5), reward=torch.zeros(1, 4097), terminated=torch.zeros(1, 4097, dtype=torch.uint8),
                                 filled=torch.zeros(1, 4097, dtype=torch.uint8)),
           "agents": dict(critic=TargetCritic("cv", 4, 20, device="cpu")), "state_dim": dict(critic=TargetCritic("cv", 3, 18, device="cpu")),
           "reward shape": dict(reward=torch.zeros(4, 7, 1)), "reward dtype": dict(reward=torch.zeros(4, 7).double()),
           "terminated dtype": dict(terminated=torch.zeros(4, 7)), "filled dtype": dict(filled=torch.zeros(4, 7, dtype=torch.int64)),
           "filled shape": dict(filled=torch.zeros(4, 8, dtype=torch.uint8)), "flag pitch": dict(filled=torch.zeros(4, 8, dtype=torch.uint8)[:, :7]),
           "obs transposed": dict(obs=torch.zeros(7, 4, 3, 5).transpose(0, 1)), "obs row stride": dict(obs=torch.zeros(4, 7, 3, 10)[..., ::2]),
           "reward stride": dict(reward=torch.zeros(4, 14)[:, ::2]), "overlapping episodes": dict(reward=torch.zeros(10).unfold(0, 7, 1)),
           "gamma above 1": dict(gamma=1.5), "gamma negative": dict(gamma=-0.1), "gamma nan": dict(gamma=NAN), "gamma not a number": dict(gamma="0.9"),
           "nstep 0": dict(nstep=0), "nstep 33": dict(nstep=33), "nstep float": dict(nstep=5.0), "nstep bool": dict(nstep=True),
           "flag": dict(add_value_last_step=2), "flag type": dict(add_value_last_step="yes"),
           "scale inf": dict(value_scale=float("inf")), "shift nan": dict(value_shift=NAN), "scale type": dict(value_scale=None),
           "returns shape": dict(returns_out=torch.zeros(4, 7, 3)), "returns dtype": dict(returns_out=torch.zeros(4, 6, 3).double()),
           "values shape": dict(values_out=torch.zeros(4, 6, 3)), "mask shape": dict(mask_out=torch.zeros(4, 6, 1)),
           "two output pitches": dict(returns_out=torch.zeros(4, 8, 3)[:, :6], mask_out=torch.zeros(4, 6)),
           "meta reward": dict(reward=ok["reward"].to("meta")), "meta output": dict(mask_out=torch.zeros(4, 6, device="meta"))}
    for what, kw in bad.items():
        with pytest.raises(ValueError) as err:
            nstep_returns(**dict(ok, **kw))
        assert "no host path" not in str(err.value), what
    with pytest.raises(ValueError, match="the critic is on"):
        critic = TargetCritic("cv", 3, 15, device="cpu")
        critic.device = torch.device("meta")
        nstep_returns(**dict(ok, critic=critic))


def test_episode_buffer_nstep_returns_value_errors():
    from marbler_amd.episodes import EpisodeBuffer
    from marbler_amd.returns import TargetCritic
    buf = EpisodeBuffer(num_envs=4, n_agents=3, obs_dim=5, n_actions=6, episode_limit=6, device="cpu")
    buf.complete[:3] = 1
    buf.length[:3] = 4
    cv, ns = TargetCritic("cv", 3, 15, device="cpu"), TargetCritic("cv_ns", 3, 15, 64, device="cpu")
    with pytest.raises(ValueError, match="no host path"):
        buf.nstep_returns(cv)
    with pytest.raises(ValueError, match="no host path"):
        buf.nstep_returns(ns, slots=[0, 5], trim=True, gamma=0.9, nstep=3, add_value_last_step=False, value_scale=2.0, value_shift=1.0,
                          reward=torch.zeros(2, 5))
    for what, critic, kw in (("critic's n_agents", TargetCritic("cv", 4, 15, device="cpu"), {}),
                             ("critic's state_dim", TargetCritic("cv", 3, 18, device="cpu"), {}), ("TargetCritic", "cv", {}),
                             ("outside", cv, dict(slots=[8])), ("reward", cv, dict(reward=torch.zeros(3, 6))),
                             ("reward", cv, dict(reward=torch.zeros(3, 7), trim=True)), ("reward", cv, dict(reward=torch.zeros(3, 7).double())),
                             ("nstep", cv, dict(nstep=0)), ("gamma", cv, dict(gamma=2.0))):
        with pytest.raises(ValueError, match=what):
            buf.nstep_returns(critic, **kw)
    with pytest.raises(ValueError, match="the buffer on"):
        critic = TargetCritic("cv", 3, 15, device="cpu")
        critic.device = torch.device("meta")
        buf.nstep_returns(critic)
    empty = EpisodeBuffer(num_envs=4, n_agents=3, obs_dim=5, n_actions=6, episode_limit=6, device="cpu")
    out = empty.nstep_returns(cv)
    assert tuple(out["returns"].shape) == (0, 6, 3) and tuple(out["values"].shape) == (0, 7, 3) and tuple(out["mask"].shape) == (0, 6, 1)
