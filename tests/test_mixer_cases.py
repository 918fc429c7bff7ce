"""The trainable mixer without a device: the float64 twin (tests/mixer_twin.py) against torch.autograd, the kink margin and the
redraw that chooses the GPU tests' inputs, the module's state dicts, the binding, every refusal of the two entry points (with host
pointers that are never dereferenced) and every ValueError of the Python layer."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mixer_harness as mh
import mixer_twin as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rg_mixer_forward", "rg_mixer_backward", "rg_sizeof_mixer_grad_weights", "rg_sizeof_mixer_grad_io", "rg_mixer_grad_last_error")


# ---------------------------------------------------------------- the twin's formulas
@pytest.mark.parametrize("N, D, A, B, rows", [(1, 2, 3, 2, 4), (2, 1, 2, 3, 5), (5, 9, 5, 4, 6), (16, 16, 20, 2, 3), (4, 64, 5, 2, 3)])
@pytest.mark.parametrize("scale", [1.0, 4.0])
def test_the_twins_backward_pass_is_float64_autograd_of_forward_reference(N, D, A, B, rows, scale):
    from marbler_amd.mixers import PARAM_NAMES, TrainableMixer
    case = ("qmix", B, rows, N, D, A, (0, 0, 0, 0))
    h = mh.draw(case, scale, seed=N)
    h["mask"][0, 0] = 1.0                                   # a live row for certain, and a masked one; episode kind 1 ends in a terminal row
    h["mask"][-1, -1] = 0.0
    h = dict(h, q=np.nan_to_num(h["q"], nan=0.5), obs=np.nan_to_num(h["obs"], nan=0.25), actions=np.clip(h["actions"], 0, A - 1))
    m = TrainableMixer("qmix", N, N * D)
    m.load_state_dict(h["params"])
    m = m.double()
    q = torch.from_numpy(h["q"]).double().requires_grad_(True)
    parts = {}
    y = m.forward_reference(q, torch.from_numpy(h["actions"]), torch.from_numpy(h["obs"]).double(), torch.from_numpy(h["mask"]), parts)
    y.backward(torch.from_numpy(h["d_mixed"]).double())
    t = tw.twin("qmix", h["q"], h["actions"], h["obs"], h["mask"], {k: v.numpy() for k, v in h["params"].items()}, h["d_mixed"])
    close = lambda a, b: np.abs(a - np.asarray(b)).max() <= 1e-9 * max(1.0, np.abs(np.asarray(b)).max())   # noqa: E731
    T = rows - 1
    assert close(t["mixed"], y.detach().numpy()) and close(t["d_q"], q.grad.numpy())
    live = (h["mask"] != 0).reshape(B * T)
    assert close(t["d_pre"][:, :T].reshape(B * T, -1)[live], parts["pre"].grad.numpy()[live])
    assert close(t["d_p2"][:, :T].reshape(B * T, -1)[live], parts["p2"].grad.numpy()[live])
    assert close(t["g"][:, :T].reshape(B * T, -1)[live], parts["g"].detach().numpy()[live])
    assert not t["d_pre"][:, T].any() and not t["d_pre"][:, :T].reshape(B * T, -1)[~live].any()
    for k in PARAM_NAMES:
        assert close(t["grads"][k], m.get_parameter(k).grad.numpy()), k
    assert set(t["grads"]) == set(PARAM_NAMES) == {k for k, _ in m.named_parameters()}


def test_vdn_and_none_twins_and_the_masked_and_out_of_range_rows():
    q = np.arange(2 * 3 * 2 * 3, dtype=np.float32).reshape(2, 3, 2, 3)
    actions = np.array([[[0, 2], [1, 5], [9, 9]], [[2, 2], [0, 0], [9, 9]]], np.int32)
    mask = np.array([[1, 1], [0, 2.5]], np.float32)
    d = np.array([[1, 2], [3, 4]], np.float32)
    mixed, d_q = tw.gather_twin("vdn", q, actions, mask, d)
    assert mixed[0, 0] == q[0, 0, 0, 0] + q[0, 0, 1, 2] and np.isnan(mixed[0, 1]) and mixed[1, 0] == 0 and mixed[1, 1] == q[1, 1, 0, 0] + q[1, 1, 1, 0]
    assert d_q[0, 0, 0, 0] == 1 and d_q[0, 1, 0, 1] == 2 and not d_q[0, 1, 1].any() and not d_q[1, 0].any() and not d_q[:, 2].any()
    assert d_q[1, 1, 0, 0] == 4 and d_q.sum() == 1 + 1 + 2 + 4 + 4
    t64 = tw.twin("vdn", q, actions, None, np.array([[1, 0], [0, 1]], np.float32), None, d)
    assert t64["mixed"][0, 1] == 0 and t64["d_q"][1, 1, 1, 0] == 4


# ---------------------------------------------------------------- the kink margin
def test_the_redraw_converges_for_every_case_of_the_gpu_table_and_leaves_no_row_inside_the_margin():
    worst = 0
    for i, case in enumerate(mh.CASES):
        if case[0] != "qmix":
            continue
        for scale in mh.SCALES:
            h = mh.draw(case, scale, seed=i)                   # (raises when a row needs more than MAX_DRAWS)
            assert 1 <= h["draws"] <= mh.MAX_DRAWS == 50
            worst = max(worst, h["draws"])
            N, D = case[3], case[4]
            s = np.stack([h["obs"][b, t].reshape(N * D) for b, t in np.argwhere(h["live"])])
            assert np.isfinite(s).all() and not tw.margin_violations({k: v.numpy() for k, v in h["params"].items()}, s).any(), case
            values, bounds = tw.kink_bounds({k: v.numpy() for k, v in h["params"].items()}, s)
            assert (np.abs(values) > tw.MARGIN * bounds).all() and (bounds > 0).all() and values.shape[1] == 160 + 32 * N + 32
    assert worst > 1                                           # the margin does bite: some row was redrawn


def test_the_bound_is_the_stated_formula_and_covers_a_float32_evaluation():
    rng = np.random.default_rng(0)
    N, S = 5, 45
    p = {k: v.numpy() for k, v in mh.make_params("qmix", N, S).items()}
    s = rng.random((64, S)) * 2 - 1
    values, bounds = tw.kink_bounds(p, s)
    e1 = (S / 2 + 2) * 2.0 ** -24 * (np.abs(s) @ np.abs(p["hyper_w_1.0.weight"]).T + np.abs(p["hyper_w_1.0.bias"]))
    assert np.array_equal(bounds[:, :64], e1)
    a1 = s @ p["hyper_w_1.0.weight"].T.astype(np.float64) + p["hyper_w_1.0.bias"]
    e2 = (32 + 2) * 2.0 ** -24 * (np.maximum(a1, 0) @ np.abs(p["hyper_w_1.2.weight"]).T + np.abs(p["hyper_w_1.2.bias"])) + (e1 * (a1 > 0)) @ np.abs(p["hyper_w_1.2.weight"]).T
    assert np.allclose(bounds[:, 160:160 + 32 * N], e2, rtol=1e-12)
    s32 = s.astype(np.float32)
    v32, _ = tw.kink_bounds(p, s32.astype(np.float64))
    f = lambda w, b, x: x @ w.T + b                         # noqa: E731  float32 throughout
    a32 = f(p["hyper_w_1.0.weight"], p["hyper_w_1.0.bias"], s32)
    p32 = f(p["hyper_w_1.2.weight"], p["hyper_w_1.2.bias"], np.maximum(a32, 0))
    _, b32 = tw.kink_bounds(p, s32.astype(np.float64))
    assert (np.abs(a32 - v32[:, :64]) <= b32[:, :64]).all() and (np.abs(p32 - v32[:, 160:160 + 32 * N]) <= tw.MARGIN * b32[:, 160:160 + 32 * N]).all()


# ---------------------------------------------------------------- the module
def test_state_dicts_round_trip_under_epymarls_names():
    from marbler_amd import TargetMixer, TrainableMixer
    from marbler_amd.targets import qmix_shapes
    target = TargetMixer("qmix", 3, 15, device="cpu", seed=4)
    mixer = TrainableMixer.from_target(target)
    sd = mixer.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == qmix_shapes(3, 15)
    assert all(torch.equal(sd[k], v) for k, v in target.state_dict().items())
    with torch.no_grad():
        for p in mixer.parameters():
            p.mul_(1.5)
    target.load_state_dict(mixer.state_dict())                  # the hard target update: TargetMixer needs no change for it
    assert all(torch.equal(v, mixer.state_dict()[k]) for k, v in target.state_dict().items())
    other = TrainableMixer("qmix", 3, 15)
    other.load_state_dict(mixer.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), mixer.state_dict().values()))
    assert len(list(TrainableMixer("vdn", 3, 15).parameters())) == 0 and TrainableMixer("none", 3, 15).state_dict() == {}
    assert TrainableMixer.from_target(TargetMixer("vdn", 3, 15, device="cpu")).kind == "vdn"
    opt = torch.optim.Adam(mixer.parameters(), lr=1e-3)         # any torch optimiser takes the parameters
    assert len(opt.param_groups[0]["params"]) == 14
    for bad in (dict(kind="qtran"), dict(n_agents=0), dict(n_agents=17), dict(state_dim=0), dict(state_dim=257), dict(n_agents=True)):
        with pytest.raises(ValueError):
            TrainableMixer(**dict(dict(kind="qmix", n_agents=3, state_dim=15), **bad))
    with pytest.raises(ValueError, match="TargetMixer"):
        TrainableMixer.from_target(mixer)


@pytest.mark.parametrize("kind", ["qmix", "vdn", "none"])
def test_forward_reference_is_target_mixers_forward_on_the_gathered_values(kind):
    from marbler_amd import TargetMixer, TrainableMixer
    B, rows, N, D, A = 3, 5, 4, 6, 5
    g = torch.Generator().manual_seed(1)
    q, obs = torch.randn(B, rows, N, A, generator=g), torch.rand(B, rows, N, D, generator=g)
    actions = torch.randint(0, A, (B, rows, N), generator=g, dtype=torch.int32)
    mask = torch.ones(B, rows - 1)
    mask[1, 2:] = 0
    target = TargetMixer(kind, N, N * D, device="cpu", seed=2)
    mixer = TrainableMixer.from_target(target)
    got = mixer.forward_reference(q, actions, obs, mask)
    x = torch.gather(q[:, :-1], 3, actions[:, :-1].long().unsqueeze(-1)).squeeze(-1)
    want = target.forward(x, obs[:, :-1].reshape(B, rows - 1, N * D))
    want = want if kind == "none" else want[..., 0]
    live = mask != 0
    assert torch.allclose(got[live], want[live], rtol=1e-6, atol=1e-6) and bool((got[~live] == 0).all())
    assert mixer.forward_reference(q, actions.unsqueeze(-1).long(), obs, mask.unsqueeze(-1)).shape == got.shape     # EPyMARL's shapes
    assert mixer.double().forward_reference(q.double(), actions, obs.double(), mask).dtype == torch.float64


# ---------------------------------------------------------------- the binding and the refusals
def test_entry_points_are_exported_declared_and_the_structs_match():
    from marbler_amd import _lib
    import marbler_amd
    lib = _lib.load_mixer_grad()
    learn = open(os.path.join(ROOT, "include", "robogym_learn.h")).read()
    main = open(os.path.join(ROOT, "include", "robogym.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in [e[0] for e in _lib.MIXER_GRAD_ENTRIES]
        assert name not in _lib.EXPORTS and name not in [e[0] for e in _lib.LEARN_ENTRIES + _lib.RETURNS_ENTRIES]
        assert re.search(r"\b%s\(" % name, learn) and name not in main, name
    assert lib.rg_sizeof_mixer_grad_weights() == ctypes.sizeof(_lib.RgMixerGradWeights) == 104
    assert lib.rg_sizeof_mixer_grad_io() == ctypes.sizeof(_lib.RgMixerGradIO) == 120
    assert dict(_lib.MIXER_GRAD_LAYOUTS) == {"rg_sizeof_mixer_grad_weights": _lib.RgMixerGradWeights, "rg_sizeof_mixer_grad_io": _lib.RgMixerGradIO}
    assert lib.rg_abi_version() == 7 and "#define RG_ABI_VERSION 7" in main
    build = __import__("marbler_amd.build", fromlist=["SOURCES"])
    assert "robogym_mixer_grad.hip" in build.SOURCES and any(h.endswith("mixer_grad.h") for h in build.HEADERS) and any(h.endswith("mixer_tile.h") for h in build.HEADERS)
    assert {"TrainableMixer", "MixerFn", "mixer_forward", "mixer_backward"} <= set(marbler_amd.__all__) and hasattr(marbler_amd.EpisodeBuffer, "mixed_q")


def test_the_rule_reads_the_same_in_the_header_and_in_design_md():
    texts = [open(os.path.join(ROOT, p)).read() for p in ("marbler_amd/csrc/mixer_grad.h", "DESIGN.md")]

    def rule(text):
        body = text[text.index("- q [B][q_pitch][N][A] f32: the online actor's output."):]
        body = body[:body.index("summation order of the kernels' choosing.") + 41]
        lines = [re.sub(r"^\s*(//|\*)?\s*(- )?", "", ln).replace("`", "") for ln in body.splitlines()]
        return " ".join(" ".join(lines).split())
    assert rule(texts[0]) == rule(texts[1]) and len(rule(texts[0])) > 2500
    assert "(S / 2 + 2) 2^-24" in texts[1] and "(S / 2 + 2) 2^-24" in open(os.path.join(ROOT, "tests", "mixer_twin.py")).read()


WEIGHTS = ("w_in", "b_in", "w_w1", "b_w1", "w_wf", "b_wf", "w_v", "b_v")
ARRAYS = ("q", "actions", "obs", "mask", "mixed", "d_mixed", "d_q", "d_pre", "d_p2", "g")


def _structs(kind=2):
    """A call both entry points accept up to the launch: N = 4, D = 16, A = 5, B = 3 episodes of 7 rows."""
    from marbler_amd import _lib
    w, io = _lib.RgMixerGradWeights(), _lib.RgMixerGradIO()
    for i, f in enumerate(WEIGHTS):
        setattr(w.m, f, 0x10000 * (i + 1))
    w.w1b, w.wfb = 0x90000, 0xA0000
    w.m.kind, w.m.n_agents, w.m.state_dim, w.m.embed_dim, w.m.hypernet_embed = kind, 4, 64, 32, 64
    for i, f in enumerate(ARRAYS):
        setattr(io, f, 0x1000000 + 0x100000 * i)
    io.num_episodes, io.n_agents, io.obs_dim, io.n_actions, io.rows = 3, 4, 16, 5, 7
    io.q_pitch, io.obs_pitch, io.out_pitch, io.aux_pitch = 8, 9, 6, 7
    return w, io


def test_both_entries_refuse_every_bad_argument_before_touching_a_device():
    from marbler_amd import _lib
    lib = _lib.load_mixer_grad()
    seen = {}

    def case(word, which="both", kind=2, **change):
        codes = set()
        for b, entry in enumerate(("rg_mixer_forward", "rg_mixer_backward")):
            if which not in ("both", entry[9:]):
                continue
            w, io = _structs(kind)
            for k, v in change.items():
                if k in ("w", "io"):
                    continue
                obj = w if k in ("w1b", "wfb") else (w.m if k.startswith("m_") else io)
                setattr(obj, k[2:] if k.startswith("m_") else k, v)
            rc = getattr(lib, entry)(None if change.get("w") == 0 else ctypes.byref(w), None if change.get("io") == 0 else ctypes.byref(io), None)
            msg = lib.rg_mixer_grad_last_error()
            assert rc < 0 and rc != -30 and msg.startswith(entry.encode() + b": ") and word in msg, (entry, change, rc, msg)
            seen.setdefault(rc, []).append((entry, word))
            codes.add(rc)
        assert len(codes) == 1, (word, codes)
        return codes.pop()

    assert case(b"w is NULL", w=0) == -1 and case(b"io is NULL", io=0) == -2
    for f, which, kinds in (("q", "forward", (0, 1, 2)), ("q", "backward", (2,)), ("actions", "both", (0, 1, 2)), ("mask", "both", (0, 1, 2)),
                            ("mixed", "forward", (0, 1, 2)), ("d_mixed", "backward", (0, 1, 2)), ("d_q", "backward", (0, 1, 2)),
                            ("obs", "both", (2,)), ("d_pre", "backward", (2,)), ("d_p2", "backward", (2,)), ("g", "backward", (2,))):
        assert {case(b"io." + f.encode() + b" is NULL", which, kind, **{f: None}) for kind in kinds} == {-3}
    assert {case(b"w.m.kind", m_kind=k) for k in (-1, 3, 99)} == {-4}
    assert {case(b"w.m." + f.encode() + b" is NULL", **{"m_" + f: None}) for f in WEIGHTS} == {-5}
    assert {case(b"w." + f.encode() + b" is NULL", "backward", **{f: None}) for f in ("w1b", "wfb")} == {-5}
    for f in WEIGHTS:
        assert {case(b"w.m." + f.encode() + b" must be 16-byte aligned", **{"m_" + f: 0x700000 + off}) for off in (4, 8, 12)} == {-6}
    assert case(b"w.w1b must be 16-byte aligned", w1b=0x700004) == case(b"io.q must be 4-byte aligned", "forward", q=0x700002) == -6
    assert {case(b"w.m.embed_dim", m_embed_dim=e) for e in (0, 16, 64)} == {case(b"w.m.hypernet_embed", m_hypernet_embed=e) for e in (0, 32, 128)} == {-7}
    assert case(b"w.m.n_agents", m_n_agents=5) == -8
    assert case(b"w.m.state_dim", m_state_dim=60) == case(b"w.m.state_dim", obs_dim=15) == -9
    for code, f in ((-10, "num_episodes"), (-11, "rows"), (-13, "n_actions"), (-14, "obs_dim")):
        assert {case(b"io." + f.encode(), **{f: v}) for v in (0, -3)} == {code}
    assert case(b"io.rows", rows=1) == -11 and case(b"io.n_actions", n_actions=33) == -13
    assert {case(b"io.n_agents", kind=1, m_n_agents=n, n_agents=n) for n in (0, -1, 17)} == {-12}
    assert case(b"wider than 256", obs_dim=65, m_state_dim=260) == -14
    assert case(b"io.obs_pitch", obs_pitch=6) == -15 and case(b"io.q_pitch", kind=0, q_pitch=6) == -16
    assert case(b"io.out_pitch", kind=1, out_pitch=5) == -17 and case(b"io.aux_pitch", "backward", aux_pitch=6) == -18
    assert case(b"io.reserved", reserved=1) == case(b"w.m.reserved", m_reserved=2) == -20
    assert case(b"q_pitch * n_agents * n_actions", num_episodes=1 << 24, q_pitch=7) == -21
    assert case(b"obs_pitch * n_agents * obs_dim", n_actions=1, num_episodes=1 << 21, obs_pitch=16) == -21
    assert case(b"out_pitch * n_agents", kind=1, n_actions=1, num_episodes=1 << 20, out_pitch=1 << 10) == -21
    assert case(b"aux_pitch * (32 n_agents + 32)", "backward", n_actions=1, num_episodes=1 << 16, aux_pitch=1 << 8) == -21
    assert sorted(seen) == [-21, -20] + list(range(-18, 0)), sorted(seen)
    # none / vdn read neither the weights nor obs nor the per-row arrays: a call without them reaches the last check
    for kind in (0, 1):
        w, io = _structs(kind)
        for f in WEIGHTS:
            setattr(w.m, f, None)
        w.w1b = w.wfb = io.obs = io.d_pre = io.d_p2 = io.g = None
        w.m.state_dim = w.m.embed_dim = w.m.hypernet_embed = io.obs_dim = io.obs_pitch = io.aux_pitch = 0
        io.reserved = 1
        for entry in ("rg_mixer_forward", "rg_mixer_backward"):
            assert getattr(lib, entry)(ctypes.byref(w), ctypes.byref(io), None) == -20 and b"io.reserved" in lib.rg_mixer_grad_last_error()


# ---------------------------------------------------------------- Python argument errors that need no device
def _call(B=4, rows=7, N=3, D=5, A=6, kind="qmix"):
    from marbler_amd.targets import TargetMixer
    return dict(q=torch.zeros(B, rows, N, A), actions=torch.zeros(B, rows, N, dtype=torch.int32), obs=torch.zeros(B, rows, N, D),
                mask=torch.ones(B, rows - 1), mixer=TargetMixer(kind, N, N * D, device="cpu"))


def test_the_launch_wrappers_value_errors():
    from marbler_amd.mixers import mixer_backward, mixer_forward
    from marbler_amd.targets import TargetMixer
    ok = _call()
    back = dict(ok, d_mixed=torch.zeros(4, 6))
    for fn, kw in ((mixer_forward, ok), (mixer_backward, back), (mixer_forward, dict(ok, mixed_out=torch.zeros(4, 6))),
                   (mixer_backward, dict(back, d_q_out=torch.zeros(4, 7, 3, 6), d_pre_out=torch.zeros(4, 7, 192), d_p2_out=torch.zeros(4, 7, 128),
                                         g_out=torch.zeros(4, 7, 160), w1b=torch.zeros(96, 64), wfb=torch.zeros(32, 64))),
                   (mixer_forward, dict(_call(kind="none"), mixed_out=torch.zeros(4, 6, 3)))):
        with pytest.raises(ValueError, match="no host path"):              # everything right but the device
            fn(**kw)
    long = _call(rows=9)
    with pytest.raises(ValueError, match="no host path"):                  # slices of longer arrays are read in place
        mixer_forward(long["q"][:, :7], long["actions"][:, :7], long["obs"][:, :7], torch.ones(4, 9)[:, :6], long["mixer"], mixed_out=torch.zeros(4, 9)[:, :6])
    bad = {"mixer": dict(mixer=None), "q dtype": dict(q=ok["q"].double()), "q not a tensor": dict(q=ok["q"].numpy()), "q three dimensions": dict(q=ok["q"][0]),
           "one row": dict(q=ok["q"][:, :1], actions=ok["actions"][:, :1], obs=ok["obs"][:, :1], mask=ok["mask"][:, :0]),
           "no episode": {k: (v[:0] if isinstance(v, torch.Tensor) else v) for k, v in ok.items()},
           "agents": dict(mixer=TargetMixer("vdn", 4, 20, device="cpu")), "too many actions": dict(q=torch.zeros(4, 7, 3, 33)),
           "state_dim": dict(mixer=TargetMixer("qmix", 3, 18, device="cpu")), "obs shape": dict(obs=torch.zeros(4, 6, 3, 5)),
           "obs dtype": dict(obs=ok["obs"].half()), "actions dtype": dict(actions=ok["actions"].long()), "actions shape": dict(actions=ok["actions"].unsqueeze(-1)),
           "actions pitch": dict(actions=torch.zeros(4, 8, 3, dtype=torch.int32)[:, :7]), "mask shape": dict(mask=torch.ones(4, 7)),
           "mask dtype": dict(mask=torch.ones(4, 6, dtype=torch.uint8)), "mask stride": dict(mask=torch.ones(4, 12)[:, ::2]),
           "q transposed": dict(q=torch.zeros(7, 4, 3, 6).transpose(0, 1)), "obs row stride": dict(obs=torch.zeros(4, 7, 3, 10)[..., ::2]),
           "meta q": dict(q=ok["q"].to("meta")), "meta obs": dict(obs=ok["obs"].to("meta"))}
    fwd_only = {"mixed shape": dict(mixed_out=torch.zeros(4, 7)), "mixed dtype": dict(mixed_out=torch.zeros(4, 6).double()),
                "mixed for qmix": dict(mixed_out=torch.zeros(4, 6, 3)), "mixed pitch": dict(mixed_out=torch.zeros(4, 8)[:, :6])}
    bwd_only = {"d_mixed missing": dict(d_mixed=None), "d_mixed shape": dict(d_mixed=torch.zeros(4, 7)), "d_mixed pitch": dict(d_mixed=torch.zeros(4, 8)[:, :6]),
                "d_q shape": dict(d_q_out=torch.zeros(4, 7, 3, 5)), "d_q pitch": dict(d_q_out=torch.zeros(4, 8, 3, 6)[:, :7]),
                "d_pre shape": dict(d_pre_out=torch.zeros(4, 7, 191)), "d_p2 shape": dict(d_p2_out=torch.zeros(4, 7, 96)), "g shape": dict(g_out=torch.zeros(4, 6, 160)),
                "two aux pitches": dict(d_pre_out=torch.zeros(4, 8, 192)[:, :7], g_out=torch.zeros(4, 7, 160)),
                "w1b shape": dict(w1b=torch.zeros(64, 96)), "wfb dtype": dict(wfb=torch.zeros(32, 64).double()),
                "aux for vdn": dict(mixer=TargetMixer("vdn", 3, 15, device="cpu"), g_out=torch.zeros(4, 7, 160))}
    for fn, base, table in ((mixer_forward, ok, dict(bad, **fwd_only)), (mixer_backward, back, dict(bad, **bwd_only))):
        for what, kw in table.items():
            with pytest.raises(ValueError) as err:
                fn(**dict(base, **kw))
            assert "no host path" not in str(err.value), (fn.__name__, what)
    with pytest.raises(ValueError, match="the mixer is on"):
        mixer = TargetMixer("vdn", 3, 15, device="cpu")
        mixer.device = torch.device("meta")
        mixer_forward(**dict(ok, mixer=mixer))


def test_the_module_and_the_buffer_value_errors():
    from marbler_amd import EpisodeBuffer, TargetMixer, TrainableMixer
    ok = _call()
    args = lambda **kw: [dict(ok, **kw)[k] for k in ("q", "actions", "obs", "mask")]   # noqa: E731
    for kind in ("qmix", "vdn", "none"):
        with pytest.raises(ValueError, match="no host path"):
            TrainableMixer(kind, 3, 15)(*args())
    mixer = TrainableMixer("qmix", 3, 15)
    with pytest.raises(ValueError, match="no host path"):                   # EPyMARL's shapes are taken
        mixer(ok["q"], ok["actions"].long().unsqueeze(-1), ok["obs"], ok["mask"].unsqueeze(-1))
    for what, kw in {"q": dict(q=None), "agents": dict(q=torch.zeros(4, 7, 4, 6)), "obs": dict(obs=torch.zeros(4, 7, 3, 6)), "mask": dict(mask=torch.ones(4, 5)),
                     "actions": dict(actions=torch.zeros(4, 7, 3))}.items():
        with pytest.raises(ValueError) as err:
            mixer(*args(**kw))
        assert "no host path" not in str(err.value), what
    with pytest.raises(ValueError, match="float32"):
        TrainableMixer("qmix", 3, 15).double()(*args())
    buf = EpisodeBuffer(num_envs=4, n_agents=3, obs_dim=5, n_actions=6, episode_limit=6, device="cpu")
    buf.complete[:3] = 1
    q, mask = torch.zeros(3, 7, 3, 6), torch.ones(3, 6, 1)
    with pytest.raises(ValueError, match="no host path"):
        buf.mixed_q(mixer, q, mask)
    for what, call in {"a target mixer": lambda: buf.mixed_q(TargetMixer("vdn", 3, 15, device="cpu"), q, mask),
                       "agents": lambda: buf.mixed_q(TrainableMixer("vdn", 4, 20), q, mask), "state_dim": lambda: buf.mixed_q(TrainableMixer("qmix", 3, 18), q, mask),
                       "q rows": lambda: buf.mixed_q(mixer, q[:, :6], mask), "mask": lambda: buf.mixed_q(mixer, q, mask[:, :5]),
                       "slots": lambda: buf.mixed_q(mixer, q, mask, slots=[9])}.items():
        with pytest.raises(ValueError) as err:
            call()
        assert "no host path" not in str(err.value), what
    assert buf.mixed_q(mixer, q[:0], mask[:0], slots=[]).shape == (0, 6, 1)
