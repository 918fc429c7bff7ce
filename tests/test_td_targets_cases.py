"""rg_td_targets without a device: the rule's twin on hand-written batches, the float64 twin against EPyMARL's lines in torch, the
weight packing, the binding, every refusal of the C entry point (host pointers that are never dereferenced: every check comes before
the first HIP call) and every ValueError of TargetMixer / td_targets / EpisodeBuffer.td_targets on CPU tensors."""
import ctypes
import re

import numpy as np
import pytest
import torch

import td_targets_twin as tw
from gpu_helpers import random_actor

NAN = float("nan")
NAMES = ("rg_td_targets", "rg_sizeof_td_targets_io", "rg_sizeof_mixer_weights", "rg_td_targets_last_error")


# ---------------------------------------------------------------- the rule, by hand
def _hand_batch():
    """N = 2, A = 2, rows = 3, gamma = 0.5.  Episodes: terminated at t = 0; terminated at its last data row t = 1; force-closed
    (never terminated, all three rows filled); an empty slot.  NaN wherever the rule says nothing is read."""
    qt = np.full((4, 3, 2, 2), NAN, np.float32)
    qt[1, 1] = [[0.5, 1.5], [-1.0, -2.0]]                    # read by (1, 0): max 1.5 and -1
    qt[2, 1] = [[2.0, 1.0], [0.25, 0.25]]                    # read by (2, 0): 2 and the FIRST 0.25
    qt[2, 2] = [[-3.0, NAN], [1.0, 4.0]]                     # read by (2, 1): NaN counts as the largest
    reward = np.array([[3.0, NAN, NAN], [1.0, 2.0, NAN], [10.0, 20.0, NAN], [NAN, NAN, NAN]], np.float32)
    terminated = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 0]], np.uint8)
    filled = np.array([[1, 0, 0], [1, 1, 0], [1, 1, 1], [0, 0, 0]], np.uint8)
    return qt, reward, terminated, filled


def test_the_twin_on_hand_written_episodes():
    qt, reward, terminated, filled = _hand_batch()
    t, mask, aq = tw.twin("vdn", qt, None, None, reward, terminated, filled, 0.5)
    assert mask.tolist() == [[1, 0], [1, 1], [1, 1], [0, 0]]
    assert aq[0].tolist() == [[0, 0], [0, 0]] and aq[1].tolist() == [[1.5, -1.0], [0, 0]] and aq[3].tolist() == [[0, 0], [0, 0]]
    assert aq[2, 0].tolist() == [2.0, 0.25] and np.isnan(aq[2, 1, 0]) and aq[2, 1, 1] == 4.0
    assert t[0].tolist() == [3.0, 0.0]                      # terminal at t = 0: the reward; then padding
    assert t[1].tolist() == [1.0 + 0.5 * 0.5, 2.0]          # 1 + gamma (1.5 - 1); terminal at the last data row: the reward
    assert t[2, 0] == 10.0 + 0.5 * 2.25 and np.isnan(t[2, 1])
    assert t[3].tolist() == [0.0, 0.0] and t.dtype == np.float32
    # double-Q: the online network's actions pick the values; one outside [0, A) is NaN in its own row only
    sel = np.full((4, 3, 2), 1 << 30, np.int32)
    sel[1, 1], sel[2, 1], sel[2, 2] = [0, 1], [1, 1], [0, 2]
    t, _, aq = tw.twin("vdn", qt, sel, None, reward, terminated, filled, 0.5)
    assert aq[1, 0].tolist() == [0.5, -2.0] and t[1].tolist() == [1.0 + 0.5 * -1.5, 2.0]
    assert aq[2, 0].tolist() == [1.0, 0.25] and t[2, 0] == 10.0 + 0.5 * 1.25
    assert aq[2, 1, 0] == -3.0 and np.isnan(aq[2, 1, 1]) and np.isnan(t[2, 1])
    assert t[0].tolist() == [3.0, 0.0] and t[3].tolist() == [0.0, 0.0]
    # none: one target per agent
    t, _, _ = tw.twin("none", qt, sel, None, reward, terminated, filled, 0.5)
    assert t.shape == (4, 2, 2) and t[1].tolist() == [[1.25, 0.0], [2.0, 2.0]] and t[0].tolist() == [[3.0, 3.0], [0.0, 0.0]]
    assert t[2, 1, 0] == 20.0 - 1.5 and np.isnan(t[2, 1, 1])


def test_vdn_sums_in_agent_order_and_keeps_the_sign_of_zero():
    one = lambda v, r=0.0, g=1.0: tw.twin("vdn", np.array([[[[0.0]] * len(v), [[x] for x in v]]], np.float32), None, None,  # noqa: E731
                                          np.array([[r, 0.0]], np.float32), np.zeros((1, 2), np.uint8), np.ones((1, 2), np.uint8), g)[0][0, 0]
    assert one([1e8, 1.0, -1e8]) == 0.0 and one([1e8, -1e8, 1.0]) == 1.0         # ((a + b) + c), float32
    assert one([16777216.0, 1.0, 1.0]) == 16777216.0 and one([1.0, 1.0, 16777216.0]) == 16777218.0
    assert np.signbit(one([-0.0, -0.0], r=-0.0)) and not np.signbit(one([-0.0, 0.0], r=-0.0))
    assert np.signbit(one([-0.0], r=-0.0)) and not np.signbit(one([-0.0], r=0.0))
    # the product is rounded before the sum: with a fused multiply-add this would be -2^-25, the rule says 0
    g, y = 1.0 - 2.0 ** -13, 1.0 + 2.0 ** -12                                       # g y = 1 + 2^-13 - 2^-25 rounds to 1 + 2^-13
    assert one([y], r=-(1.0 + 2.0 ** -13), g=g) == 0.0


def _random_case(B, rows, N, D, A, seed, with_sel=True):
    rng = np.random.default_rng(seed)
    qt = rng.standard_normal((B, rows, N, A)).astype(np.float32)
    obs = (rng.random((B, rows, N, D)) * 2 - 1).astype(np.float32)
    reward = rng.standard_normal((B, rows)).astype(np.float32)
    length = rng.integers(1, rows, B)
    t = np.arange(rows)[None]
    filled = (t <= length[:, None]).astype(np.uint8)
    terminated = ((t == length[:, None] - 1) & (rng.random(B) < 0.6)[:, None]).astype(np.uint8)
    sel = rng.integers(0, A, (B, rows, N)).astype(np.int32) if with_sel else None
    return qt, sel, obs, reward, terminated, filled


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("with_sel", [True, False])
def test_the_float64_twin_agrees_with_epymarls_lines_in_torch(scale, with_sel):
    from marbler_amd.targets import TargetMixer
    B, rows, N, D, A = 6, 9, 4, 16, 5
    qt, sel, obs, reward, terminated, filled = _random_case(B, rows, N, D, A, 3, with_sel)
    mixer = TargetMixer("qmix", N, N * D, device="cpu", seed=5)
    mixer.load_state_dict({k: v * scale for k, v in mixer.state_dict().items()})
    params = mixer.state_dict()
    t64, mask, aq = tw.twin("qmix", qt, sel, obs, reward, terminated, filled, 0.99, {k: v.numpy() for k, v in params.items()})
    as_t = lambda x: None if x is None else torch.from_numpy(x)  # noqa: E731
    ref, ref_mask = tw.restatement("qmix", as_t(qt), as_t(sel), as_t(obs), as_t(reward), as_t(terminated), as_t(filled), 0.99, params)
    assert np.array_equal(ref_mask[..., 0].numpy(), mask) and mask.sum() >= B
    assert tw.rel_err(ref[..., 0].numpy(), t64, mask > 0) < 2e-5                 # float32 against float64 over K <= 64 + 64 + 32 + 4 terms
    # in float64 the two are the same computation
    p64 = {k: v.double() for k, v in params.items()}
    ref64, _ = tw.restatement("qmix", as_t(qt).double(), as_t(sel), as_t(obs).double(), as_t(reward).double(), as_t(terminated),
                              as_t(filled), float(np.float32(0.99)), p64)
    assert tw.rel_err(ref64[..., 0].numpy(), t64, mask > 0) < 1e-12
    # and TargetMixer.forward is that mixer
    y = mixer.forward(torch.from_numpy(aq), torch.from_numpy(obs[:, 1:]).reshape(B, rows - 1, N * D))
    assert torch.equal(y, tw.qmixer_torch(params, torch.from_numpy(aq), torch.from_numpy(obs[:, 1:]).reshape(B, rows - 1, N * D)))
    for kind in ("vdn", "none"):
        t32, mask, _ = tw.twin(kind, qt, sel, obs, reward, terminated, filled, 0.99)
        ref, _ = tw.restatement(kind, as_t(qt), as_t(sel), as_t(obs), as_t(reward), as_t(terminated), as_t(filled), 0.99)
        ref = ref.numpy() if kind == "none" else ref[..., 0].numpy()
        assert tw.rel_err(ref, t32, mask > 0) < 1e-6


# ---------------------------------------------------------------- the packing
@pytest.mark.parametrize("N,S", [(2, 2), (5, 45), (4, 64), (8, 144), (3, 254)])
def test_packing_round_trips_and_pads_the_state_with_zero_rows(N, S):
    from marbler_amd import targets
    mixer = targets.TargetMixer("qmix", N, S, device="cpu", seed=N)
    sd = mixer.state_dict()
    assert set(sd) == set(targets.qmix_shapes(N, S)) and all(tuple(v.shape) == targets.qmix_shapes(N, S)[k] for k, v in sd.items())
    back = mixer.unpack()
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    layout, total = targets.packed_layout(N, S)
    sp = (S + 3) // 4 * 4
    assert layout["w_in"] == (0, (sp, 192)) and mixer.packed.numel() == total and all(off % 4 == 0 for off, _ in layout.values())
    w_in = mixer.packed[:sp * 192].view(sp, 192)
    assert bool((w_in[S:] == 0).all()) and torch.equal(w_in[:S, 64:128], sd["hyper_w_final.0.weight"].t())
    assert torch.equal(w_in[:S, 160:192], sd["hyper_b_1.weight"].t())                # K-major: [in][out]
    # the default initialisation is torch's: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
    assert float(sd["hyper_w_1.2.weight"].abs().max()) <= 1 / 8 and float(sd["V.0.bias"].abs().max()) <= S ** -0.5
    # a soft update re-packs into the same storage
    ptr, w = mixer.packed.data_ptr(), mixer.weights_struct()
    mixer.load_state_dict({k: 0.5 * v for k, v in sd.items()})
    assert mixer.packed.data_ptr() == ptr and torch.equal(mixer.unpack()["V.2.weight"], 0.5 * sd["V.2.weight"])
    assert w.w_in == ptr and w.b_v == ptr + 4 * layout["b_v"][0] and all(getattr(w, k) % 16 == 0 for k in layout)
    assert (w.kind, w.n_agents, w.state_dim, w.embed_dim, w.hypernet_embed, w.reserved) == (2, N, S, 32, 64, 0)


def test_target_mixer_value_errors():
    from marbler_amd.targets import TargetMixer, qmix_shapes
    good = TargetMixer("qmix", 3, 15, device="cpu").state_dict()
    for what, args in (("kind", ("qtran", 3, 15)), ("n_agents", ("vdn", 0, 15)), ("n_agents", ("vdn", 17, 15)), ("n_agents", ("vdn", True, 15)),
                       ("state_dim", ("qmix", 3, 0)), ("state_dim", ("qmix", 3, 2.5)), ("above 256", ("qmix", 3, 257))):
        with pytest.raises(ValueError, match=what):
            TargetMixer(*args, device="cpu")
    with pytest.raises(ValueError, match="no weights"):
        TargetMixer("vdn", 3, 15, good, device="cpu")
    bad = {"lacks": {k: v for k, v in good.items() if k != "V.2.bias"},
           "hyper_b_1.weight": dict(good, **{"hyper_b_1.weight": torch.zeros(32, 16)}),
           "hyper_w_1.2.weight": dict(good, **{"hyper_w_1.2.weight": torch.zeros(64, 64)}),             # another n_agents
           "hyper_w_1.0.weight": dict(good, **{"hyper_w_1.0.weight": torch.zeros(32, 15)}),             # another hypernet_embed
           "hypernet_layers: 1": {"hyper_w_1.weight": torch.zeros(96, 15), "hyper_w_1.bias": torch.zeros(96),
                                  "hyper_w_final.weight": torch.zeros(32, 15), "hyper_w_final.bias": torch.zeros(32),
                                  **{k: v for k, v in good.items() if k.startswith(("hyper_b_1", "V."))}},
           "not finite": dict(good, **{"V.0.weight": torch.full((32, 15), float("inf"))}),
           "not finite ": dict(good, **{"hyper_w_final.2.bias": torch.full((32,), NAN)}),
           "floating-point": dict(good, **{"V.2.bias": torch.zeros(1, dtype=torch.int64)}),
           "must be a tensor": dict(good, **{"V.2.bias": [0.0]})}
    for what, sd in bad.items():
        with pytest.raises(ValueError, match=what.strip()):
            TargetMixer("qmix", 3, 15, sd, device="cpu")
    mixer = TargetMixer("qmix", 3, 15, good, device="cpu")
    before = mixer.packed.clone()
    with pytest.raises(ValueError, match="not finite"):
        mixer.load_state_dict(bad["not finite"])
    assert torch.equal(mixer.packed, before), "a refused state dict must leave the packed weights alone"
    assert set(qmix_shapes(3, 15)) == set(good)
    assert TargetMixer("vdn", 3, 15, device="cpu").forward(torch.ones(2, 5, 3), None).shape == (2, 5, 1)


# ---------------------------------------------------------------- the binding and the refusals
def test_entry_points_are_exported_declared_and_the_structs_match():
    from marbler_amd import _lib
    import marbler_amd
    lib = _lib.load()
    header = open(_lib.__file__.replace("marbler_amd/_lib.py", "include/robogym.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS and name in _lib.LATE_QUERIES
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.rg_sizeof_mixer_weights() == ctypes.sizeof(_lib.RgMixerWeights) == 88
    assert lib.rg_sizeof_td_targets_io() == ctypes.sizeof(_lib.RgTdTargetsIO) == 120
    assert lib.rg_abi_version() == 7 and "#define RG_ABI_VERSION 7" in header
    assert "robogym_td_targets.hip" in __import__("marbler_amd.build", fromlist=["SOURCES"]).SOURCES
    assert marbler_amd.TargetMixer is __import__("marbler_amd.targets", fromlist=["x"]).TargetMixer and callable(marbler_amd.td_targets)
    assert {"TargetMixer", "td_targets"} <= set(marbler_amd.__all__) and hasattr(marbler_amd.EpisodeBuffer, "td_targets")


def test_the_rule_reads_the_same_in_the_three_places_it_is_stated():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    texts = [open(os.path.join(root, p)).read() for p in ("marbler_amd/csrc/td_targets.h", "include/robogym.h", "DESIGN.md")]

    def rule(text):
        body = text[text.index("Inputs.\n"):]
        body = body[:body.index("summation order of the kernel's choosing.") + 40]
        lines = [re.sub(r"^\s*(//|\*)?\s*(- )?", "", ln).replace("`", "") for ln in body.splitlines()]    # comment marks, bullets
        return " ".join(" ".join(lines).split())                                                         # and line breaks aside
    assert rule(texts[0]) == rule(texts[1]) == rule(texts[2]) and len(rule(texts[0])) > 2000


WEIGHTS = ("w_in", "b_in", "w_w1", "b_w1", "w_wf", "b_wf", "w_v", "b_v")
ARRAYS = ("qt", "sel", "obs", "reward", "terminated", "filled", "targets", "mask", "agent_q")


def _structs(kind=2):
    """A call the entry point accepts up to the launch: N = 4, D = 16, A = 5, B = 3 episodes of 7 rows."""
    from marbler_amd import _lib
    m, io = _lib.RgMixerWeights(), _lib.RgTdTargetsIO()
    for i, f in enumerate(WEIGHTS):
        setattr(m, f, 0x10000 * (i + 1))
    m.kind, m.n_agents, m.state_dim, m.embed_dim, m.hypernet_embed, m.reserved = kind, 4, 64, 32, 64, 0
    for i, f in enumerate(ARRAYS):
        setattr(io, f, 0x1000000 + 0x100000 * i)
    io.num_episodes, io.n_agents, io.obs_dim, io.n_actions, io.rows = 3, 4, 16, 5, 7
    io.q_pitch, io.obs_pitch, io.flag_pitch, io.out_pitch, io.gamma, io.reserved = 8, 9, 7, 6, 0.99, 0
    return m, io


def test_rg_td_targets_refuses_every_bad_argument_before_touching_a_device():
    from marbler_amd import _lib
    lib = _lib.load()
    seen = {}

    def refused(word, m, io, what):
        rc = lib.rg_td_targets(ctypes.byref(m) if m is not None else None, ctypes.byref(io) if io is not None else None, None)
        msg = lib.rg_td_targets_last_error()
        assert rc < 0 and rc != -30, (what, rc, msg)
        assert msg.startswith(b"rg_td_targets: ") and word in msg, (what, rc, msg)
        seen.setdefault(rc, []).append(what)
        return rc

    def case(word, what, kind=2, **change):
        m, io = _structs(kind)
        for k, v in change.items():
            setattr(m if k in dict(m._fields_) and k not in ("n_agents", "reserved") else io, k, v)
        return refused(word, m, io, what)

    m, io = _structs()
    assert refused(b"m is NULL", None, io, "m") == -1
    assert refused(b"io is NULL", m, None, "io") == -2
    for f in ("qt", "reward", "terminated", "filled", "targets"):
        assert {case(b"io." + f.encode() + b" is NULL", (f, kind), kind, **{f: None}) for kind in (0, 1, 2)} == {-3}
    assert case(b"io.obs is NULL", "obs", obs=None) == -3
    assert {case(b"m.kind", ("kind", k), kind=k) for k in (-1, 3, 99)} == {-4}
    assert {case(b"m." + f.encode() + b" is NULL", f, **{f: None}) for f in WEIGHTS} == {-5}
    for f in WEIGHTS:
        assert {case(b"m." + f.encode() + b" must be 16-byte aligned", (f, off), **{f: 0x700000 + off}) for off in (4, 8, 12)} == {-6}
    assert {case(b"m.embed_dim", ("embed", e), embed_dim=e) for e in (0, 16, 64)} == {-7}
    assert {case(b"m.hypernet_embed", ("hyper", e), hypernet_embed=e) for e in (0, 32, 128)} == {-7}
    m, io = _structs()
    m.n_agents = 5
    assert refused(b"m.n_agents", m, io, "m.n_agents") == -8
    assert case(b"m.state_dim", "state_dim", state_dim=60) == case(b"m.state_dim", "obs_dim against state_dim", obs_dim=15) == -9
    for code, f in ((-10, "num_episodes"), (-11, "rows"), (-13, "n_actions"), (-14, "obs_dim")):
        assert {case(b"io." + f.encode(), (f, v), **{f: v}) for v in (0, -3)} == {code}
    assert case(b"io.rows", "one row", rows=1) == -11 and case(b"io.n_actions", "33 actions", n_actions=33) == -13
    for n in (0, -1, 17):
        m, io = _structs(1)
        m.n_agents = io.n_agents = n
        assert refused(b"io.n_agents", m, io, ("n_agents", n)) == -12
    assert case(b"wider than 256", "a wide state", obs_dim=65, state_dim=260) == -14
    assert case(b"io.obs_pitch", "obs_pitch", obs_pitch=6) == -15
    assert case(b"io.q_pitch", "q_pitch", q_pitch=6) == -16
    assert case(b"io.flag_pitch", "flag_pitch", flag_pitch=6) == -17
    assert case(b"io.out_pitch", "out_pitch", out_pitch=5) == -18
    assert {case(b"io.gamma", ("gamma", g), gamma=g) for g in (-0.01, 1.01, float("inf"), NAN)} == {-19}
    assert case(b"io.reserved", "io.reserved", reserved=1) == -20
    m, io = _structs()
    m.reserved = 2
    assert refused(b"m.reserved", m, io, "m.reserved") == -20
    big = 1 << 24
    assert case(b"q_pitch * n_agents * n_actions", "range: qt", num_episodes=big, q_pitch=7, obs_pitch=7, out_pitch=6) == -21   # 2^24 x 7 x 20
    assert case(b"obs_pitch * n_agents * obs_dim", "range: obs", kind=1, n_actions=1, num_episodes=1 << 21, obs_pitch=16) == -21  # 2^25 x 64
    assert case(b"io.num_episodes * flag_pitch", "range: flags", kind=1, flag_pitch=1 << 30) == -21
    assert case(b"exceeds 2^31 - 1", "range: every factor huge", kind=1, num_episodes=2 ** 31 - 1, rows=2 ** 31 - 1,
                q_pitch=2 ** 31 - 1, obs_pitch=2 ** 31 - 1, flag_pitch=2 ** 31 - 1, out_pitch=2 ** 31 - 1, obs_dim=2 ** 31 - 1) == -21
    m, io = _structs(1)
    io.n_actions, io.obs_dim, io.num_episodes, io.out_pitch, m.n_agents, io.n_agents = 1, 1, 1 << 23, 1 << 6, 16, 16
    io.q_pitch = io.obs_pitch = io.flag_pitch = 7
    assert refused(b"out_pitch * n_agents", m, io, "range: outputs") == -21                # 2^23 x 2^6 x 2^4
    assert sorted(seen) == list(range(-21, 0)), sorted(seen)
    # none / vdn read neither the weights nor obs, and sel, mask and agent_q are optional: all of these reach the last check
    for kind in (0, 1, 2):
        m, io = _structs(kind)
        io.sel = io.mask = io.agent_q = None
        if kind != 2:
            io.obs = None
            m.embed_dim = m.hypernet_embed = m.state_dim = 0
            for f in WEIGHTS:
                setattr(m, f, None)
        io.reserved = 1
        assert refused(b"io.reserved", m, io, ("optional", kind)) == -20


# ---------------------------------------------------------------- Python argument errors that need no device
def _call(B=4, rows=7, N=3, D=5, A=6, kind="qmix"):
    from marbler_amd.targets import TargetMixer
    return dict(qt=torch.zeros(B, rows, N, A), obs=torch.zeros(B, rows, N, D), reward=torch.zeros(B, rows),
                terminated=torch.zeros(B, rows, dtype=torch.uint8), filled=torch.ones(B, rows, dtype=torch.bool),
                mixer=TargetMixer(kind, N, N * D, device="cpu"), gamma=0.99)


def test_td_targets_value_errors():
    from marbler_amd.targets import TargetMixer, td_targets
    with pytest.raises(ValueError, match="no host path"):                 # everything right but the device
        td_targets(**_call())
    long = _call(rows=9)
    with pytest.raises(ValueError, match="no host path"):
        td_targets(long["qt"][:, :7], long["obs"][:, :7], long["reward"][:, :7], long["terminated"][:, :7], long["filled"][:, :7],
                   long["mixer"], 0.5, sel=torch.zeros(4, 9, 3, dtype=torch.int32)[:, :7], targets_out=torch.zeros(4, 8)[:, :6],
                   mask_out=torch.zeros(4, 8)[:, :6], agent_q_out=torch.zeros(4, 8, 3)[:, :6])
    with pytest.raises(ValueError, match="no host path"):
        td_targets(**dict(_call(kind="none"), targets_out=torch.zeros(4, 6, 3)))
    ok = _call()
    bad = {"mixer": dict(mixer=None), "qt dtype": dict(qt=ok["qt"].double()), "qt not a tensor": dict(qt=ok["qt"].numpy()),
           "qt three dimensions": dict(qt=ok["qt"][0]), "one row": {k: (v[:, :1] if isinstance(v, torch.Tensor) else v) for k, v in ok.items()},
           "no episode": {k: (v[:0] if isinstance(v, torch.Tensor) else v) for k, v in ok.items()},
           "agents": dict(mixer=TargetMixer("vdn", 4, 20, device="cpu")), "actions": dict(qt=torch.zeros(4, 7, 3, 33)),
           "state_dim": dict(mixer=TargetMixer("qmix", 3, 18, device="cpu")), "obs shape": dict(obs=torch.zeros(4, 6, 3, 5)),
           "obs dtype": dict(obs=ok["obs"].half()), "reward shape": dict(reward=torch.zeros(4, 7, 1)), "reward dtype": dict(reward=torch.zeros(4, 7).double()),
           "terminated dtype": dict(terminated=torch.zeros(4, 7)), "filled dtype": dict(filled=torch.zeros(4, 7, dtype=torch.int64)),
           "filled shape": dict(filled=torch.zeros(4, 8, dtype=torch.uint8)), "sel dtype": dict(sel=torch.zeros(4, 7, 3, dtype=torch.int64)),
           "sel shape": dict(sel=torch.zeros(4, 7, 3, 1, dtype=torch.int32)),
           "sel pitch": dict(sel=torch.zeros(4, 8, 3, dtype=torch.int32)[:, :7]),
           "flag pitch": dict(filled=torch.zeros(4, 8, dtype=torch.uint8)[:, :7]),
           "qt transposed": dict(qt=torch.zeros(7, 4, 3, 6).transpose(0, 1)), "obs row stride": dict(obs=torch.zeros(4, 7, 3, 10)[..., ::2]),
           "reward stride": dict(reward=torch.zeros(4, 14)[:, ::2]), "overlapping episodes": dict(reward=torch.zeros(10).unfold(0, 7, 1)),
           "gamma above 1": dict(gamma=1.5), "gamma negative": dict(gamma=-0.1), "gamma nan": dict(gamma=NAN), "gamma not a number": dict(gamma="0.9"),
           "targets shape": dict(targets_out=torch.zeros(4, 7)), "targets dtype": dict(targets_out=torch.zeros(4, 6).double()),
           "targets for none": dict(targets_out=torch.zeros(4, 6, 3)), "mask shape": dict(mask_out=torch.zeros(4, 6, 1)),
           "agent_q shape": dict(agent_q_out=torch.zeros(4, 6, 6)),
           "two output pitches": dict(targets_out=torch.zeros(4, 8)[:, :6], mask_out=torch.zeros(4, 6)),
           "meta qt": dict(qt=ok["qt"].to("meta")), "meta obs": dict(obs=ok["obs"].to("meta")), "meta output": dict(mask_out=torch.zeros(4, 6, device="meta"))}
    for what, kw in bad.items():
        with pytest.raises(ValueError) as err:
            td_targets(**dict(ok, **kw))
        assert "no host path" not in str(err.value), what
    with pytest.raises(ValueError, match="the mixer is on"):
        mixer = TargetMixer("vdn", 3, 15, device="cpu")
        mixer.device = torch.device("meta")
        td_targets(**dict(ok, mixer=mixer))


def _cpu_actor(N=3, D=5, H=64, A=6, append=True):
    from marbler_amd.evaluate import BatchedActor
    return BatchedActor(random_actor(1, D + (N if append else 0), H, A, True, seed=1), N)


def test_episode_buffer_td_targets_value_errors():
    from marbler_amd.episodes import EpisodeBuffer
    from marbler_amd.targets import TargetMixer
    buf = EpisodeBuffer(num_envs=4, n_agents=3, obs_dim=5, n_actions=6, episode_limit=6, device="cpu")
    buf.complete[:3] = 1
    buf.length[:3] = 4
    qmix, vdn = TargetMixer("qmix", 3, 15, device="cpu"), TargetMixer("vdn", 3, 15, device="cpu")
    with pytest.raises(ValueError, match="no host path"):
        buf.td_targets(_cpu_actor(), qmix)
    with pytest.raises(ValueError, match="no host path"):
        buf.td_targets(_cpu_actor(append=False), vdn, greedy=torch.zeros(2, 5, 3, dtype=torch.int32), slots=[0, 5], trim=True, obs_agent_id=False)
    for what, actor, mixer, kw in (("actor's n_agents", _cpu_actor(N=2, D=6), qmix, {}), ("actor's n_actions", _cpu_actor(A=5), qmix, {}),
                                   ("actor's input_dim", _cpu_actor(D=4), qmix, {}), ("actor's input_dim", _cpu_actor(), qmix, dict(obs_agent_id=False)),
                                   ("mixer's n_agents", _cpu_actor(), TargetMixer("vdn", 4, 15, device="cpu"), {}),
                                   ("mixer's state_dim", _cpu_actor(), TargetMixer("qmix", 3, 18, device="cpu"), {}),
                                   ("TargetMixer", _cpu_actor(), "qmix", {}), ("outside", _cpu_actor(), qmix, dict(slots=[8])),
                                   ("greedy", _cpu_actor(), qmix, dict(greedy=torch.zeros(3, 7, 3, dtype=torch.int64))),
                                   ("greedy", _cpu_actor(), qmix, dict(greedy=torch.zeros(3, 7, 3, dtype=torch.int32), trim=True)),
                                   ("greedy", _cpu_actor(), qmix, dict(greedy=torch.zeros(3, 7, 3, 6)))):
        with pytest.raises(ValueError, match=what):
            buf.td_targets(actor, mixer, **kw)
    with pytest.raises(ValueError, match="the buffer on"):
        mixer = TargetMixer("vdn", 3, 15, device="cpu")
        mixer.device = torch.device("meta")
        buf.td_targets(_cpu_actor(), mixer)
    empty = EpisodeBuffer(num_envs=4, n_agents=3, obs_dim=5, n_actions=6, episode_limit=6, device="cpu")
    out = empty.td_targets(_cpu_actor(), qmix)
    assert tuple(out["targets"].shape) == (0, 6, 1) and tuple(out["mask"].shape) == (0, 6, 1) and tuple(out["agent_q"].shape) == (0, 6, 3)
    assert tuple(empty.td_targets(_cpu_actor(), TargetMixer("none", 3, 15, device="cpu"))["targets"].shape) == (0, 6, 3)
