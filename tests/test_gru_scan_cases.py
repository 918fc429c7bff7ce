"""The GRU scan and the trainable actor without a GPU: the float64 twin's hand-written backward pass against torch.autograd (this
pins the formulas the kernels are held to in tests/test_gpu_gru_scan.py), the reference loop against BatchedActor.forward, state-dict
round trips under EPyMARL's key names, the binding, every refusal of the two entry points (with host pointers that are never
dereferenced), every ValueError of the Python layer, and the rule's text in the header against DESIGN.md."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import gru_scan_twin as tw
from gpu_helpers import random_actor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rg_sizeof_gru_scan_weights", "rg_sizeof_gru_scan_io", "rg_gru_scan_forward", "rg_gru_scan_backward", "rg_gru_scan_last_error")


# ---------------------------------------------------------------- the twin's backward pass is autograd's
def _autograd64(gi, w_hh, b_hh, hidden, dh_ext, d_hidden_out):
    """float64 autograd through a GRUCell composition (torch.nn.functional's own cell, one weight set per agent where asked) ->
    h, dgi, dghn, d_hidden, dW_hh, db_hh."""
    B, rows, N, G = gi.shape
    H, A = G // 3, w_hh.shape[0]
    t64 = lambda x: torch.tensor(x, dtype=torch.float64)  # noqa: E731
    gi_t, w, b = t64(gi).requires_grad_(True), t64(w_hh).requires_grad_(True), t64(b_hh).requires_grad_(True)
    hid = (t64(hidden) if hidden is not None else torch.zeros(B, N, H, dtype=torch.float64)).requires_grad_(True)
    h, hs = hid, []
    for t in range(rows):
        outs = []
        for n in range(N):
            a = n if A > 1 else 0
            # torch's own cell, torch._VF.gru_cell(input, hx, w_ih, w_hh, b_ih, b_hh), with w_ih = I and b_ih = 0: gi IS the input half
            outs.append(torch._VF.gru_cell(gi_t[:, t, n], h[:, n], torch.eye(3 * H, dtype=torch.float64), w[a], torch.zeros(3 * H, dtype=torch.float64), b[a]))
        h = torch.stack(outs, dim=1)
        hs.append(h)
    hh = torch.stack(hs, dim=1)
    loss = (hh * t64(dh_ext)).sum() + ((h * t64(d_hidden_out)).sum() if d_hidden_out is not None else 0.0)
    loss.backward()
    return hh.detach().numpy(), gi_t.grad.numpy(), hid.grad.numpy(), w.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize("H,per_agent,with_hidden,with_dho", list(itertools.product((64, 128), (False, True), (False, True), (False, True))))
def test_the_twins_backward_pass_is_torch_autograd_of_a_float64_grucell(H, per_agent, with_hidden, with_dho):
    rng = np.random.default_rng(H + 2 * per_agent + 4 * with_hidden + 8 * with_dho)
    B, rows, N = 3, 20 if (H == 128 and per_agent and with_hidden and with_dho) else 5, 2
    A, k = (N if per_agent else 1), 1.0 / np.sqrt(H)
    gi, dh_ext = rng.standard_normal((B, rows, N, 3 * H)), rng.standard_normal((B, rows, N, H))
    w_hh, b_hh = (rng.random((A, 3 * H, H)) * 2 - 1) * k, (rng.random((A, 3 * H)) * 2 - 1) * k
    hidden = rng.random((B, N, H)) * 2 - 1 if with_hidden else None
    dho = rng.standard_normal((B, N, H)) if with_dho else None
    h, gates, last = tw.forward(gi, w_hh, b_hh, hidden)
    dgi, dghn, dhid = tw.backward(h, gates, w_hh, dh_ext, hidden, dho)
    dw, db = tw.weight_grads(h, dgi, dghn, hidden, A)
    h_t, dgi_t, dhid_t, dw_t, db_t = _autograd64(gi, w_hh, b_hh, hidden, dh_ext, dho)
    rel = lambda x, y: float(np.max(np.abs(x - y)) / max(np.max(np.abs(y)), 1e-300))  # noqa: E731
    assert np.array_equal(last, h[:, -1]) and h.dtype == np.float64
    for name, x, y in (("h", h, h_t), ("dgi", dgi, dgi_t), ("d_hidden_in", dhid, dhid_t), ("dW_hh", dw, dw_t), ("db_hh", db, db_t)):
        assert rel(x, y) <= 1e-9, (name, rel(x, y))
    # dghn against autograd too: the n third of d loss / d gh, by finite structure -- db_hh's n third is its sum over every row
    assert rel(dghn.sum(axis=(0, 1)) if per_agent else dghn.sum(axis=(0, 1, 2))[None], db_t[:, 2 * H:]) <= 1e-9


# ---------------------------------------------------------------- the module on the CPU
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("append", [True, False])
def test_forward_reference_is_batched_actor_forward_stepped_in_a_loop(shared, append):
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.learn import TrainableActor
    N, D, H, A, B, rows = 3, 6, 64, 5, 4, 5
    sd = random_actor(1 if shared else N, D + (N if append else 0), H, A, True, seed=11)
    actor = BatchedActor(sd, N, device="cpu")
    mod = TrainableActor.from_actor(actor)
    obs = torch.rand(B, rows, N, D, generator=torch.Generator().manual_seed(1)) * 2 - 1
    h0 = torch.rand(B, N, H, generator=torch.Generator().manual_seed(2)) - 0.5
    for hidden in (None, h0):
        with torch.no_grad():
            q, last = mod.forward_reference(obs, append_agent_id=append, hidden=hidden, return_hidden=True)
        h, eye = actor.init_hidden(B) if hidden is None else hidden, torch.eye(N).expand(B, N, N)
        for t in range(rows):
            qt, h = actor.forward(torch.cat([obs[:, t], eye], dim=2) if append else obs[:, t], h)
            assert torch.equal(qt, q[:, t]), t                        # float32, the same composition: the same words
        assert torch.equal(h, last)


@pytest.mark.parametrize("shared", [True, False])
def test_state_dicts_round_trip_under_epymarls_key_names(shared):
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.learn import TrainableActor
    N, I, H, A = 3, 9, 128, 4
    sd = random_actor(1 if shared else N, I, H, A, True, seed=12)
    mod = TrainableActor(N, I, H, A, shared=shared)
    assert list(mod.state_dict().keys()) == list(sd.keys())            # EPyMARL's names, its order
    assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    mod.load_state_dict(sd)                                             # strict
    actor = BatchedActor(mod.state_dict(), N, device="cpu")
    assert actor.non_shared == (not shared)
    back = actor.state_dict()
    assert list(back.keys()) == list(sd.keys()) and all(torch.equal(back[k], sd[k]) for k in sd)
    again = TrainableActor.from_actor(actor)
    assert again.shared == shared and all(torch.equal(v, sd[k]) for k, v in again.state_dict().items())
    assert len(list(again.parameters())) == (8 if shared else 8 * N)
    torch.optim.Adam(again.parameters(), lr=1e-3)                       # any torch optimiser takes them
    # BatchedActor.load_state_dict: the same storages
    ptrs = {a: getattr(actor, a).data_ptr() for a in ("w1", "b1", "wih", "whh", "bih", "bhh", "w2", "b2")}
    new = {k: v + 0.25 for k, v in sd.items()}
    actor.load_state_dict(new)
    assert ptrs == {a: getattr(actor, a).data_ptr() for a in ptrs}
    assert all(torch.equal(v, new[k]) for k, v in actor.state_dict().items())


def test_batched_actor_load_state_dict_value_errors():
    from marbler_amd.evaluate import BatchedActor
    N, I, H, A = 2, 5, 64, 3
    for n_sets, use_rnn in ((1, True), (N, True), (1, False)):
        sd = random_actor(n_sets, I, H, A, use_rnn, seed=13)
        actor = BatchedActor(sd, N, use_rnn=use_rnn, device="cpu")
        first = next(iter(sd))
        bad = {"not a dict": [sd], "a missing key": {k: v for k, v in sd.items() if k != first},
               "a changed shape": dict(sd, **{first: torch.zeros(H + 1, I)}), "not a tensor": dict(sd, **{first: sd[first].numpy()}),
               "an integer tensor": dict(sd, **{first: sd[first].to(torch.int32)}),
               "a NaN": dict(sd, **{first: torch.full_like(sd[first], float("nan"))}),
               "an infinity": dict(sd, **{list(sd)[-1]: torch.full_like(sd[list(sd)[-1]], float("inf"))})}
        if n_sets > 1:
            bad["the shared names"] = random_actor(1, I, H, A, use_rnn, seed=13)
        for what, arg in bad.items():
            with pytest.raises(ValueError):
                actor.load_state_dict(arg)
            assert all(torch.equal(v, sd[k]) for k, v in actor.state_dict().items()), what     # a refused state dict changes nothing
        actor.load_state_dict({k: v.double() for k, v in sd.items()})                          # any floating-point dtype


# ---------------------------------------------------------------- the binding and the refusals
def test_entry_points_are_exported_declared_beside_robogym_h_and_the_structs_match():
    from marbler_amd import _lib
    import marbler_amd
    lib = _lib.load_learn()
    old, new = (open(os.path.join(ROOT, "include", h)).read() for h in ("robogym.h", "robogym_learn.h"))
    for name in NAMES:
        assert hasattr(lib, name) and name in [e[0] for e in _lib.LEARN_ENTRIES]
        assert name not in _lib.EXPORTS and name not in _lib.LATE_QUERIES and name not in [e[0] for e in _lib.RETURNS_ENTRIES]
        assert re.search(r"\b%s\(" % name, new), name
    assert "gru_scan" not in old and '#include "robogym.h"' in new
    assert lib.rg_sizeof_gru_scan_weights() == ctypes.sizeof(_lib.RgGruScanWeights) == 40
    assert lib.rg_sizeof_gru_scan_io() == ctypes.sizeof(_lib.RgGruScanIO) == 112
    assert lib.rg_abi_version() == _lib.ABI_VERSION == 7 and "#define RG_ABI_VERSION 7" in old
    build = __import__("marbler_amd.build", fromlist=["SOURCES"])
    assert "robogym_gru_scan.hip" in build.SOURCES and any(h.endswith("robogym_learn.h") for h in build.HEADERS)
    assert any(h.endswith("gru_scan.h") for h in build.HEADERS)
    learn = __import__("marbler_amd.learn", fromlist=["x"])
    for name in ("TrainableActor", "GruScan", "gru_scan_forward", "gru_scan_backward"):
        assert getattr(marbler_amd, name) is getattr(learn, name) and name in marbler_amd.__all__


def test_a_library_without_the_entries_fails_only_when_the_feature_is_called(monkeypatch):
    from marbler_amd import _lib

    class Old(object):                        # a library of an earlier build: everything but the new entries
        def __getattr__(self, name):
            if "gru_scan" in name:
                raise AttributeError(name)
            return lambda *a: 0
    monkeypatch.setattr(_lib, "_lib", Old())
    monkeypatch.setattr(_lib, "_learn_ready", False)
    assert _lib.load() is not None
    with pytest.raises(_lib.RobogymError, match="rg_sizeof_gru_scan_weights"):
        _lib.load_learn()


def test_the_rule_reads_the_same_in_the_header_and_in_design_md():
    texts = [open(os.path.join(ROOT, p)).read() for p in ("marbler_amd/csrc/gru_scan.h", "DESIGN.md")]

    def rule(text):
        body = text[text.index("GRU scan rule.\n"):]
        body = body[:body.index("End of the rule.")]
        lines = [re.sub(r"^\s*(//|\*)?\s*(- )?", "", ln).replace("`", "") for ln in body.splitlines()]    # comment marks, bullets
        return " ".join(" ".join(lines).split())                                                         # and line breaks aside
    assert rule(texts[0]) == rule(texts[1]) and len(rule(texts[0])) > 2000
    for line in ("carry = dh z + (da_r, da_z, dghn_t) W_hh", "n = tanh(gi_n + r gh_n)", "da_r = (da_n gh_n) r (1 - r)"):
        assert line in rule(texts[0])


IO_ARRAYS = ("gi", "hidden_in", "h", "gates", "hidden_out", "dh_ext", "d_hidden_out", "dgi", "dghn", "d_hidden_in")


def _structs(n_sets=1):
    """A call both entry points accept up to the launch: B = 3 episodes of 7 rows, N = 4, H = 128."""
    from marbler_amd import _lib
    w, io = _lib.RgGruScanWeights(), _lib.RgGruScanIO()
    w.w_hh, w.b_hh, w.w_hh_t, w.n_sets, w.hidden_dim = 0x10000, 0x20000, None, n_sets, 128
    for i, f in enumerate(IO_ARRAYS):
        setattr(io, f, 0x1000000 + 0x100000 * i)
    io.num_episodes, io.n_agents, io.rows, io.gi_pitch, io.save_pitch, io.grad_pitch = 3, 4, 7, 9, 8, 7
    return w, io


def test_the_entry_points_refuse_every_bad_argument_before_touching_a_device():
    from marbler_amd import _lib
    lib = _lib.load_learn()
    entries = {"f": (lib.rg_gru_scan_forward, b"rg_gru_scan_forward: "), "b": (lib.rg_gru_scan_backward, b"rg_gru_scan_backward: ")}
    seen = {"f": set(), "b": set()}

    def refused(which, word, w, io, what):
        fn, prefix = entries[which]
        rc = fn(ctypes.byref(w) if w is not None else None, ctypes.byref(io) if io is not None else None, None)
        msg = lib.rg_gru_scan_last_error()
        assert rc < 0 and rc != -30, (which, what, rc, msg)
        assert msg.startswith(prefix) and word in msg, (which, what, rc, msg)
        seen[which].add(rc)
        return rc

    def case(which, word, n_sets=1, **change):
        w, io = _structs(n_sets)
        for k, v in change.items():
            setattr(w if k in dict(w._fields_) and k != "reserved" else io, k, v)
        return refused(which, word, w, io, change)

    for which in "fb":
        w, io = _structs()
        assert refused(which, b"w is NULL", None, io, "w") == -1 and refused(which, b"io is NULL", w, None, "io") == -2
    for f in ("gi", "h"):
        assert case("f", b"io." + f.encode() + b" is NULL", **{f: None}) == -3
    for f in ("h", "dh_ext", "dgi", "dghn"):
        assert case("b", b"io." + f.encode() + b" is NULL", **{f: None}) == -3
    assert case("f", b"w.w_hh is NULL", w_hh=None) == case("b", b"w.w_hh is NULL", w_hh=None) == case("f", b"w.b_hh is NULL", b_hh=None) == -4
    for f in ("w_hh", "b_hh", "w_hh_t"):
        assert {case("f", b"w." + f.encode() + b" must be 16-byte aligned", **{f: 0x700000 + off}) for off in (4, 8, 12)} == {-5}
    assert case("b", b"w.w_hh must be 16-byte aligned", w_hh=0x700004) == -5
    for f in ("gi", "hidden_in", "h", "gates", "hidden_out"):
        assert {case("f", b"io." + f.encode() + b" must be 4-byte aligned", **{f: 0x700000 + off}) for off in (1, 2, 3)} == {-5}
    for f in ("h", "gates", "hidden_in", "dh_ext", "d_hidden_out", "dgi", "dghn", "d_hidden_in"):
        assert case("b", b"io." + f.encode() + b" must be 4-byte aligned", **{f: 0x700002}) == -5
    for which in "fb":
        assert {case(which, b"w.hidden_dim", hidden_dim=h) for h in (0, 32, 96, 256, -128)} == {-6}
        assert {case(which, b"w.n_sets", n_sets=s) for s in (0, 2, 3, 5, -1)} == {-7}
        assert {case(which, b"io.n_agents", n_agents=n, n_sets=1) for n in (0, -1, 17)} == {-8}
        assert {case(which, b"io.num_episodes", num_episodes=v) for v in (0, -3)} == {-9}
        assert {case(which, b"io.rows must be >= 1", rows=v) for v in (0, -3)} == {-10}
        assert case(which, b"io.rows is above 4096", rows=4097, gi_pitch=4097, save_pitch=4097, grad_pitch=4097) == -11
        assert case(which, b"io.save_pitch", save_pitch=6) == -13
        assert case(which, b"io.reserved", reserved=(ctypes.c_int32 * 2)(0, 1)) == -20
        w, io = _structs()
        w.reserved[0] = 2
        assert refused(which, b"w.reserved", w, io, "w.reserved") == -20
        assert case(which, b"save_pitch * n_agents * 4 hidden_dim", save_pitch=1 << 21) == -21
        assert case(which, b"exceeds 2^31 - 1", num_episodes=2 ** 31 - 1, gi_pitch=2 ** 31 - 1, save_pitch=2 ** 31 - 1, grad_pitch=2 ** 31 - 1) == -21
    assert case("f", b"io.gi_pitch", gi_pitch=6) == -12 and case("b", b"io.grad_pitch", grad_pitch=6) == -14
    assert case("b", b"io.gates", gates=None) == -15
    assert case("f", b"gi_pitch * n_agents * 3 hidden_dim", gi_pitch=1 << 21) == -21
    assert case("b", b"grad_pitch * n_agents * 3 hidden_dim", grad_pitch=1 << 21) == -21
    assert sorted(seen["f"]) == [-21, -20, -13, -12, -11, -10, -9, -8, -7, -6, -5, -4, -3, -2, -1]
    assert sorted(seen["b"]) == [-21, -20, -15, -14, -13, -11, -10, -9, -8, -7, -6, -5, -4, -3, -2, -1]
    # a launch looks only at its own arguments, every optional pointer may be NULL, and the edges of every range are taken: all of
    # these reach the last check
    for which, n_sets in itertools.product("fb", (1, 4)):
        w, io = _structs(n_sets)
        io.hidden_in = io.hidden_out = io.d_hidden_out = io.d_hidden_in = None
        w.w_hh_t = None
        if which == "f":
            io.gates = io.dh_ext = io.dgi = io.dghn = None
            io.grad_pitch = 0
        else:
            io.gi, w.b_hh, io.gi_pitch = None, None, 0
        io.rows, io.save_pitch = 4096, 4096
        io.gi_pitch, io.grad_pitch = (4096, 0) if which == "f" else (0, 4096)
        io.num_episodes, io.n_agents, w.n_sets, w.hidden_dim = 1, (16 if n_sets > 1 else 1), (16 if n_sets > 1 else 1), 64
        io.reserved[1] = 1
        assert refused(which, b"io.reserved", w, io, ("optional", which, n_sets)) == -20


# ---------------------------------------------------------------- Python argument errors that need no device
def _fwd(B=4, rows=5, N=3, H=64, A=1):
    return dict(gi=torch.zeros(B, rows, N, 3 * H), w_hh=torch.zeros(A, 3 * H, H), b_hh=torch.zeros(A, 3 * H))


def _bwd(B=4, rows=5, N=3, H=64, A=1):
    return dict(h=torch.zeros(B, rows, N, H), gates=torch.zeros(B, rows, N, 4 * H), w_hh=torch.zeros(A, 3 * H, H), dh_ext=torch.zeros(B, rows, N, H))


def test_the_plain_launches_value_errors():
    from marbler_amd.learn import gru_scan_backward, gru_scan_forward
    with pytest.raises(ValueError, match="no host path"):                 # everything right but the device
        gru_scan_forward(**_fwd())
    with pytest.raises(ValueError, match="no host path"):
        gru_scan_backward(**_bwd(A=3))
    long = _fwd(rows=8)
    with pytest.raises(ValueError, match="no host path"):                 # slices of longer arrays, 2-D weights, every optional argument
        gru_scan_forward(long["gi"][:, :5], long["w_hh"][0], long["b_hh"][0], hidden=torch.zeros(4, 3, 64), h_out=torch.zeros(4, 7, 3, 64)[:, :5],
                         gates_out=torch.zeros(4, 7, 3, 256)[:, :5], hidden_out=torch.zeros(4, 3, 64))
    with pytest.raises(ValueError, match="no host path"):
        gru_scan_forward(**_fwd(), gates_out=False)
    with pytest.raises(ValueError, match="no host path"):
        gru_scan_backward(**dict(_bwd(), dh_ext=torch.zeros(4, 6, 3, 64)[:, :5]), hidden=torch.zeros(4, 3, 64), d_hidden_out=torch.zeros(4, 3, 64), dgi_out=torch.zeros(4, 6, 3, 192)[:, :5],
                          dghn_out=torch.zeros(4, 6, 3, 64)[:, :5], d_hidden_in_out=torch.zeros(4, 3, 64))
    ok = _fwd()
    bad = {"gi not a tensor": dict(gi=ok["gi"].numpy()), "gi dtype": dict(gi=ok["gi"].double()), "gi three dimensions": dict(gi=ok["gi"][0]),
           "gi width": dict(gi=torch.zeros(4, 5, 3, 191)), "no episode": dict(gi=ok["gi"][:0]), "no row": dict(gi=ok["gi"][:, :0]),
           "too many rows": dict(gi=torch.zeros(1, 4097, 1, 192)), "too many agents": dict(gi=torch.zeros(1, 2, 17, 192)),
           "gi transposed": dict(gi=torch.zeros(5, 4, 3, 192).transpose(0, 1)), "gi row stride": dict(gi=torch.zeros(4, 5, 3, 384)[..., ::2]),
           "w_hh dtype": dict(w_hh=ok["w_hh"].double()), "w_hh not a tensor": dict(w_hh=None), "w_hh shape": dict(w_hh=torch.zeros(1, 192, 65)),
           "w_hh one dimension": dict(w_hh=torch.zeros(192)), "w_hh not contiguous": dict(w_hh=torch.zeros(1, 64, 192).transpose(1, 2)),
           "hidden size": dict(gi=torch.zeros(4, 5, 3, 96), w_hh=torch.zeros(1, 96, 32), b_hh=torch.zeros(1, 96)),
           "two sets for three agents": dict(w_hh=torch.zeros(2, 192, 64), b_hh=torch.zeros(2, 192)),
           "b_hh missing": dict(b_hh=None), "b_hh shape": dict(b_hh=torch.zeros(1, 191)), "b_hh sets": dict(b_hh=torch.zeros(3, 192)),
           "b_hh dtype": dict(b_hh=ok["b_hh"].double()), "hidden shape": dict(hidden=torch.zeros(4, 3, 65)), "hidden dtype": dict(hidden=torch.zeros(4, 3, 64).double()),
           "hidden not contiguous": dict(hidden=torch.zeros(4, 64, 3).transpose(1, 2)), "hidden_out shape": dict(hidden_out=torch.zeros(3, 3, 64)),
           "h_out shape": dict(h_out=torch.zeros(4, 6, 3, 64)), "h_out dtype": dict(h_out=torch.zeros(4, 5, 3, 64).double()),
           "gates_out shape": dict(gates_out=torch.zeros(4, 5, 3, 192)), "gates_out a flag": dict(gates_out=True),
           "two save pitches": dict(h_out=torch.zeros(4, 7, 3, 64)[:, :5], gates_out=torch.zeros(4, 5, 3, 256)),
           "meta weights": dict(w_hh=ok["w_hh"].to("meta")), "meta output": dict(h_out=torch.zeros(4, 5, 3, 64, device="meta"))}
    for what, kw in bad.items():
        with pytest.raises(ValueError) as err:
            gru_scan_forward(**dict(ok, **kw))
        assert "no host path" not in str(err.value), what
    ok = _bwd()
    bad = {"h not a tensor": dict(h=None), "h dtype": dict(h=ok["h"].double()), "h width": dict(h=torch.zeros(4, 5, 3, 65)),
           "h two dimensions": dict(h=torch.zeros(4, 64)), "too many rows": dict(h=torch.zeros(1, 4097, 1, 64)),
           "gates shape": dict(gates=torch.zeros(4, 5, 3, 192)), "gates missing": dict(gates=None), "gates dtype": dict(gates=ok["gates"].double()),
           "two save pitches": dict(gates=torch.zeros(4, 6, 3, 256)[:, :5]), "w_hh shape": dict(w_hh=torch.zeros(192, 65)),
           "two sets for three agents": dict(w_hh=torch.zeros(2, 192, 64)), "dh_ext missing": dict(dh_ext=None), "dh_ext shape": dict(dh_ext=torch.zeros(4, 5, 3, 63)),
           "dh_ext stride": dict(dh_ext=torch.zeros(4, 5, 3, 128)[..., ::2]), "hidden shape": dict(hidden=torch.zeros(4, 3)),
           "d_hidden_out shape": dict(d_hidden_out=torch.zeros(4, 2, 64)), "dgi_out shape": dict(dgi_out=torch.zeros(4, 5, 3, 64)),
           "dghn_out dtype": dict(dghn_out=torch.zeros(4, 5, 3, 64, dtype=torch.float16)), "d_hidden_in_out shape": dict(d_hidden_in_out=torch.zeros(4, 3, 63)),
           "two grad pitches": dict(dgi_out=torch.zeros(4, 6, 3, 192)[:, :5], dghn_out=torch.zeros(4, 5, 3, 64)),
           "grad pitch against dh_ext": dict(dgi_out=torch.zeros(4, 6, 3, 192)[:, :5]), "meta h": dict(h=ok["h"].to("meta"))}
    for what, kw in bad.items():
        with pytest.raises(ValueError) as err:
            gru_scan_backward(**dict(ok, **kw))
        assert "no host path" not in str(err.value), what


def test_the_trainable_actor_value_errors():
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.learn import TrainableActor
    for kw in (dict(hidden_dim=32), dict(hidden_dim=96), dict(hidden_dim=256), dict(n_agents=0), dict(n_agents=17), dict(input_dim=0), dict(n_actions=0),
               dict(n_agents=2.0), dict(hidden_dim=True)):
        with pytest.raises(ValueError):
            TrainableActor(**dict(dict(n_agents=3, input_dim=8, hidden_dim=64, n_actions=4), **kw))
    with pytest.raises(ValueError, match="GRU"):
        TrainableActor.from_actor(BatchedActor(random_actor(1, 8, 64, 4, False, seed=1), 3, use_rnn=False, device="cpu"))
    with pytest.raises(ValueError, match="hidden_dim"):
        TrainableActor.from_actor(BatchedActor(random_actor(1, 8, 32, 4, True, seed=1), 3, device="cpu"))
    for shared in (True, False):
        mod = TrainableActor(3, 8, 64, 4, shared=shared)
        obs = torch.zeros(2, 5, 3, 5)
        with pytest.raises(ValueError, match="no host path"):             # a CPU module: everything right but the device
            mod(obs)
        with pytest.raises(ValueError, match="no host path"):
            mod(torch.zeros(2, 5, 3, 8), append_agent_id=False, hidden=torch.zeros(2, 3, 64))
        with pytest.raises(ValueError, match="no host path"):
            mod(torch.zeros(2, 9, 3, 5)[:, :5])                            # a slice of a longer batch is read in place
        bad = {"obs not a tensor": dict(obs=obs.numpy()), "obs dtype": dict(obs=obs.double()), "obs three dimensions": dict(obs=obs[0]),
               "agents": dict(obs=torch.zeros(2, 5, 4, 5)), "width": dict(obs=torch.zeros(2, 5, 3, 6)), "width without the id": dict(append_agent_id=False),
               "no episode": dict(obs=obs[:0]), "no row": dict(obs=obs[:, :0]), "obs strides": dict(obs=torch.zeros(2, 5, 3, 10)[..., ::2]),
               "obs agents strided": dict(obs=torch.zeros(2, 5, 6, 5)[:, :, ::2]), "obs on meta": dict(obs=obs.to("meta")),
               "hidden shape": dict(hidden=torch.zeros(2, 3, 65)), "hidden dtype": dict(hidden=torch.zeros(2, 3, 64).double()),
               "hidden on meta": dict(hidden=torch.zeros(2, 3, 64, device="meta"))}
        for what, kw in bad.items():
            with pytest.raises(ValueError) as err:
                mod(**dict(dict(obs=obs), **kw))
            assert "no host path" not in str(err.value), what
            if what not in ("obs strides", "obs agents strided"):
                with pytest.raises(ValueError):
                    mod.forward_reference(**dict(dict(obs=obs), **kw))
        with pytest.raises(ValueError, match="float32"):
            TrainableActor(3, 8, 64, 4, shared=shared).double()(obs.double())
