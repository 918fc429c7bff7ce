"""The GRU scan launches (csrc/gru_scan.h) and the trainable actor built on them (marbler_amd/learn.py) on the device.

Every array of a call sits in a guarded buffer (tests/gru_scan_harness.py).  The error metric throughout is
max |x - x64| / (1 + |x64|) against float64, and the bound for the float32 kernels is 4 x the error the torch float32 per-step
loop makes on the same inputs on the same device -- the bound tests/test_gpu_td_targets.py and tests/test_gpu_nstep_returns.py use for
"float32 kernel against float64" -- with the torch error asserted to be above zero so that the bound is never vacuous.
Measured on an MI355X over the case table: the kernels' error is at most 2.6 x torch's forward (h 1.9, gates 1.8, hidden_out 2.6)
and at most 0.9 x backward."""
import copy

import numpy as np
import pytest
import torch

import gru_scan_harness as hs
import gru_scan_twin as tw
from gpu_helpers import random_actor
from td_targets_harness import DEV, draw_episodes, words

pytestmark = pytest.mark.gpu
BOUND = 4.0


def held(name, got, ref64, torch_got, torch_ref64, what):
    """got is within BOUND x torch's own error of ref64; prints the figures first."""
    e, et = tw.err(got, ref64), tw.err(torch_got, torch_ref64)
    print(f"{what} {name}: kernel {e:.3e} torch {et:.3e} ratio {e / et if et else float('inf'):.2f}")
    assert et > 0.0, (what, name, "the torch loop is exact here: the bound would be vacuous")
    assert np.isfinite(e) and e <= BOUND * et, (what, name, e, et)


def test_the_case_table_covers_what_it_is_meant_to():
    flat = {B * N for B, _, N, *_ in hs.CASES}
    assert flat >= {1, 31, 32, 33, 65} and {N for _, _, N, *_ in hs.CASES} == {1, 2, 5}
    assert {c[1] for c in hs.CASES} == {1, 2, 3, 17} and {c[3] for c in hs.CASES} == {64, 128}
    for per_agent in (False, True):
        sub = [c for c in hs.CASES if c[4] == per_agent]
        assert {c[3] for c in sub} == {64, 128} and {c[5] for c in sub} == {False, True} and {c[6] for c in sub} == {False, True}
        for k in range(3):
            assert {c[7][k] for c in sub} == {0, 3}
    assert any(c[4] and c[0] % 32 not in (0,) and c[0] > 32 for c in hs.CASES)           # a ragged last tile of one agent


@pytest.mark.parametrize("i", range(len(hs.CASES)))
def test_forward_and_backward_against_the_float64_twin(i):
    case = hs.CASES[i]
    for scale in (1.0, 4.0):                                        # 4: saturating gates
        b = hs.Batch(*case, scale=scale, seed=i)
        ref, loop = b.twin64(), b.torch_loop()
        out = b.forward()                                           # (guards, untouched rows and padding: checked exactly inside)
        for k in hs.FWD_OUT:
            held(k, out[k], ref[k], loop[k], ref[k], f"case {i} x{scale:g} forward")
        if scale == 1.0:
            grads, ref_b = b.backward(), b.twin64_backward_on(out["h"], out["gates"])
            for k in hs.BWD_OUT:                                    # the kernel on ITS OWN saved words; torch on its own pass
                held(k, grads[k], ref_b[k], loop[k], ref[k], f"case {i} backward")


# ---------------------------------------------------------------- properties
def test_two_calls_give_identical_words():
    b = hs.Batch(13, 17, 5, 128, True, True, True, (3, 0, 3), seed=50)
    first = {**b.forward(), **b.backward()}
    second = {**b.forward(), **b.backward()}
    for k, v in first.items():
        assert np.array_equal(words(v), words(second[k])), k


@pytest.mark.parametrize("per_agent", [False, True])
def test_a_row_computes_the_same_words_alone_and_inside_a_batch_of_33(per_agent):
    from marbler_amd.learn import gru_scan_backward, gru_scan_forward
    big = hs.Batch(33, 5, 2, 64, per_agent, True, True, seed=51)
    d = big.dev
    out = {**big.forward(), **big.backward()}
    for bi in (0, 17, 32):
        cut = lambda t: None if t is None else t[bi:bi + 1].contiguous()  # noqa: E731
        h, gates = gru_scan_forward(cut(d["gi"]), d["w_hh"], d["b_hh"], cut(d["hidden"]))
        dgi, dghn, dhid = gru_scan_backward(h, gates, d["w_hh"], cut(d["dh_ext"]), cut(d["hidden"]), cut(d["d_hidden_out"]))
        for k, v in (("h", h), ("gates", gates), ("dgi", dgi), ("dghn", dghn), ("d_hidden_in", dhid)):
            assert np.array_equal(words(v)[0], words(out[k])[bi]), (k, bi)


def test_a_nan_stays_in_its_flat_row():
    B, rows, N, H, t0, hit = 20, 6, 2, 64, 2, (7, 1)
    clean, dirty = hs.Batch(B, rows, N, H, False, True, True, seed=52), hs.Batch(B, rows, N, H, False, True, True, seed=52)
    dirty.whole["gi"][hit[0], t0, hit[1], 5] = hs.NAN
    dirty.before["gi"] = dirty.whole["gi"].clone()
    a, b = {**clean.forward(), **clean.backward()}, {**dirty.forward(), **dirty.backward()}
    other = np.ones((B, N), bool)
    other[hit] = False
    for k in a:                                                     # no other flat row sees it
        ax = 2 if a[k].ndim == 4 else 1
        sel = np.moveaxis(a[k], ax, 1)[other], np.moveaxis(b[k], ax, 1)[other]
        assert np.array_equal(words(sel[0]), words(sel[1])) and np.isfinite(sel[1]).all(), k
    row = lambda k: b[k][hit[0], :, hit[1]]  # noqa: E731
    # from step t on: the planted column at step t, every column behind it (the next product reads the whole row)
    assert np.isfinite(row("h")[:t0]).all() and np.isnan(row("h")[t0, 5]) and np.isnan(row("h")[t0 + 1:]).all()
    assert np.isfinite(row("gates")[:t0]).all() and np.isnan(row("gates")[t0:, :H]).any()
    assert np.isnan(b["hidden_out"][hit]).all()
    # backward: the carry is NaN from the last step down, and every product of the row with it
    assert np.isnan(row("dgi")).all() and np.isnan(row("dghn")).all() and np.isnan(b["d_hidden_in"][hit]).all()


def test_saturated_inputs_give_finite_results():
    for sign in (1.0, -1.0):
        b = hs.Batch(3, 4, 2, 128, False, True, True, seed=53)
        b.whole["gi"][:, :b.rows] = sign * 100.0
        b.whole["gi"][1, :b.rows, :, ::2] = -sign * 100.0
        b.before["gi"] = b.whole["gi"].clone()
        out = {**b.forward(), **b.backward()}
        for k, v in out.items():
            assert np.isfinite(v).all(), (sign, k)
        assert np.abs(out["h"]).max() <= 1.0


def test_a_captured_pair_of_launches_replays_to_the_same_words():
    eager, graphed = hs.Batch(33, 7, 4, 128, False, True, True, (3, 3, 3), seed=54), hs.Batch(33, 7, 4, 128, False, True, True, (3, 3, 3), seed=54)
    want = {**eager.forward(), **eager.backward()}
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    from marbler_amd.learn import gru_scan_backward, gru_scan_forward
    d, o = graphed.dev, graphed.out
    with torch.cuda.graph(graph, stream=side):                     # two nodes, one branch; every output passed in
        gru_scan_forward(d["gi"], d["w_hh"], d["b_hh"], d["hidden"], h_out=o("h"), gates_out=o("gates"), hidden_out=o("hidden_out"))
        gru_scan_backward(o("h"), o("gates"), d["w_hh"], d["dh_ext"], d["hidden"], d["d_hidden_out"], dgi_out=o("dgi"), dghn_out=o("dghn"),
                          d_hidden_in_out=o("d_hidden_in"))
    torch.cuda.synchronize()
    graph.replay()                                                 # (a capture records; the replay is what runs)
    torch.cuda.synchronize()
    graphed.before.update({k: graphed.whole[k].clone() for k in ("h", "gates")})
    graphed.check_untouched(())
    for k, v in want.items():
        assert np.array_equal(words(o(k)), words(v)), k


def test_outputs_are_allocated_when_not_given():
    from marbler_amd.learn import gru_scan_backward, gru_scan_forward
    b = hs.Batch(5, 3, 2, 64, True, False, False, seed=55)
    d = b.dev
    want = {**b.forward(), **b.backward()}
    h, gates = gru_scan_forward(d["gi"], d["w_hh"], d["b_hh"])
    dgi, dghn, dhid = gru_scan_backward(h, gates, d["w_hh"], d["dh_ext"])
    for k, v in (("h", h), ("gates", gates), ("dgi", dgi), ("dghn", dghn), ("d_hidden_in", dhid)):
        assert v.is_contiguous() and np.array_equal(words(v), words(want[k])), k
    h2, none = gru_scan_forward(d["gi"], d["w_hh"][0] if b.A == 1 else d["w_hh"], d["b_hh"], gates_out=False)
    assert none is None and np.array_equal(words(h2), words(h))


# ---------------------------------------------------------------- the whole module
def _module(shared, H, N=3, D=7, A=5, seed=0):
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.learn import TrainableActor
    sd = random_actor(1 if shared else N, D + N, H, A, True, seed=seed)
    return TrainableActor.from_actor(BatchedActor(sd, N, device=DEV)), sd


def _batch(B, rows, N, D, A, seed):
    rng = np.random.default_rng(seed)
    reward, terminated, filled = draw_episodes(B, rows, rng, seed)
    to = lambda x: torch.from_numpy(x).to(DEV)  # noqa: E731
    return dict(obs=to((rng.random((B, rows, N, D)) * 2 - 1).astype(np.float32)), actions=to(rng.integers(0, A, (B, rows, N, 1))),
                reward=to(reward), terminated=to(terminated), filled=to(filled), c=to(rng.standard_normal((B, rows, N, A)).astype(np.float32)))


def _grads(module, loss_of, forward):
    module.zero_grad()
    loss_of(forward(module)).backward()
    return {k: p.grad.detach().cpu().numpy().copy() for k, p in module.named_parameters()}


@pytest.mark.parametrize("shared,H", [(True, 128), (False, 64), (True, 64), (False, 128)])
@pytest.mark.parametrize("loss", ["linear", "vdn_td"])
def test_every_parameter_gradient_against_float64_autograd_of_the_reference_loop(shared, H, loss):
    """TrainableActor (GEMMs + the two scan launches) against float64 autograd through forward_reference, per parameter tensor,
    within 4 x the error of float32 autograd through the same loop."""
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.targets import TargetMixer, td_targets
    N, D, A, B, rows = 3, 7, 5, 9, 6
    actor, _ = _module(shared, H, N, D, A, seed=3)
    bt = _batch(B, rows, N, D, A, seed=60 + H + shared)
    if loss == "linear":
        loss_of = lambda q: (q * bt["c"].to(q.dtype)).sum()  # noqa: E731
    else:
        target = BatchedActor(random_actor(1, D + N, H, A, True, seed=8), N, device=DEV)
        qt, _ = target.unroll(bt["obs"])
        out = td_targets(qt, bt["obs"], bt["reward"], bt["terminated"], bt["filled"], TargetMixer("vdn", N, N * D, device=DEV), 0.99)
        targets, mask = out["targets"], out["mask"]
        assert float(mask.sum()) >= 4

        def loss_of(q):
            chosen = torch.gather(q[:, :-1], 3, bt["actions"][:, :-1]).squeeze(3).sum(dim=2)        # VDN: the sum over the agents
            td = (chosen - targets.to(q.dtype)) * mask.to(q.dtype)
            return (td ** 2).sum() / mask.to(q.dtype).sum()
    ref = copy.deepcopy(actor).double()
    g64 = _grads(ref, loss_of, lambda m: m.forward_reference(bt["obs"].double()))
    g_loop = _grads(actor, loss_of, lambda m: m.forward_reference(bt["obs"]))
    g = _grads(actor, loss_of, lambda m: m(bt["obs"]))
    assert set(g) == set(g64) and len(g) == (8 if shared else 8 * N)
    for k in sorted(g):
        held(k, g[k], g64[k], g_loop[k], g64[k], f"{loss} shared={shared} H={H}")


@pytest.mark.parametrize("shared", [True, False])
def test_hidden_given_and_its_gradient(shared):
    N, D, A, B, rows, H = 2, 4, 3, 5, 4, 64
    actor, _ = _module(shared, H, N, D, A, seed=5)
    bt = _batch(B, rows, N, D, A, seed=70)
    hid = (torch.rand(B, N, H, device=DEV) * 2 - 1)
    res = {}
    for name, mod, fwd, dt in (("f64", copy.deepcopy(actor).double(), "forward_reference", torch.float64), ("loop", actor, "forward_reference", torch.float32),
                               ("scan", actor, "forward", torch.float32)):
        h0 = hid.to(dt).clone().requires_grad_(True)                   # (a leaf of its own: .to() of the same dtype is the same tensor)
        mod.zero_grad()
        q = getattr(mod, fwd)(bt["obs"].to(dt), hidden=h0, append_agent_id=True)
        (q * bt["c"].to(dt)).sum().backward()
        res[name] = dict(q=q.detach().cpu().numpy(), d_hidden=h0.grad.cpu().numpy(), whh=[p.grad.cpu().numpy() for k, p in mod.named_parameters() if "weight_hh" in k][0])
    for k in ("q", "d_hidden", "whh"):
        held(k, res["scan"][k], res["f64"][k], res["loop"][k], res["f64"][k], f"hidden shared={shared}")


@pytest.mark.parametrize("shared,H", [(True, 128), (False, 64)])
def test_forward_agrees_with_the_unroll_launch_within_the_two_errors(shared, H):
    """TrainableActor's q (float32 GEMMs, the exact f32 matrix instruction in the scan) and BatchedActor.unroll's q (binary16 planes)
    are different arithmetic and NOT bit-equal; their distance is held to the sum of their own distances from float64, both
    measured here, and the trainable side to 4 x the float32 loop's error."""
    from marbler_amd.evaluate import BatchedActor
    N, D, A, B, rows = 4, 12, 5, 11, 9
    actor, sd = _module(shared, H, N, D, A, seed=6)
    obs = _batch(B, rows, N, D, A, seed=80)["obs"]
    with torch.no_grad():
        q64 = copy.deepcopy(actor).double().forward_reference(obs.double()).cpu().numpy()
        q_loop = actor.forward_reference(obs).cpu().numpy()
        q = actor(obs).cpu().numpy()
    q_unroll = BatchedActor(sd, N, device=DEV).unroll(obs)[0].cpu().numpy()
    held("q", q, q64, q_loop, q64, f"forward shared={shared}")
    e_train, e_unroll = tw.err(q, q64), tw.err(q_unroll, q64)
    between = float(np.max(np.abs(q.astype(np.float64) - q_unroll) / (1.0 + np.abs(q64))))
    print(f"trainable {e_train:.3e} unroll {e_unroll:.3e} between {between:.3e}")
    assert between <= e_train + e_unroll and e_unroll > 0.0


# ---------------------------------------------------------------- end to end: collect -> learn -> collect
def test_collect_learn_reload_collect():
    from marbler_amd.episodes import EpisodeBuffer
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    from marbler_amd.learn import TrainableActor
    v = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", 40, time_limit=12, seed=18)
    H = 64
    actor = BatchedActor(random_actor(1, v.obs_size + v.n_agents, H, v.n_actions, True, seed=4), v.n_agents, device=DEV)
    runner = BatchedRunner(v, actor, epsilon=0.0, seed=9, action_selector="soft_policies")
    buf = EpisodeBuffer.for_runner(runner)
    runner.run(30, into=buf)
    new = buf.take_new()
    assert new.numel() >= 1, "no episode completed"
    batch = buf.batch(new)
    # a graph round one actor step, captured BEFORE the reload
    E, N = 8, v.n_agents
    obs1, hidden, q_buf = batch["obs"][:E, 0].contiguous(), torch.zeros(E, N, H, device=DEV), torch.empty(E, N, v.n_actions, device=DEV)
    act_buf = torch.empty(E, N, dtype=torch.int32, device=DEV)
    actor.forward_fused(obs1, hidden, q_out=q_buf, actions_out=act_buf)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        actor.forward_fused(obs1, hidden, q_out=q_buf, actions_out=act_buf)
    torch.cuda.synchronize()
    ws_before = actor._weights_struct()
    # one SGD step on the collected batch, read in place
    trainable = TrainableActor.from_actor(actor)
    opt = torch.optim.SGD(trainable.parameters(), lr=0.05)
    q = trainable(batch["obs"])
    chosen = torch.gather(q, 3, batch["actions"]).squeeze(3)
    loss = ((chosen.sum(dim=2) - batch["reward"].squeeze(2)) ** 2 * batch["filled"].squeeze(2)).mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    new_sd = {k: p.detach().clone() for k, p in trainable.state_dict().items()}
    assert any(not torch.equal(new_sd[k], actor.state_dict()[k]) for k in new_sd)
    actor.load_state_dict(trainable.state_dict())
    assert actor._weights_struct() is ws_before                     # the cached struct, the same storages
    fresh = BatchedActor(new_sd, v.n_agents, device=DEV)
    q_re, a_re = actor.unroll(batch["obs"])
    q_fr, a_fr = fresh.unroll(batch["obs"])
    torch.cuda.synchronize()
    assert torch.equal(q_re.view(torch.int32), q_fr.view(torch.int32)) and torch.equal(a_re, a_fr)
    # the graph captured before the reload replays with the new weights
    hidden.zero_()
    graph.replay()
    torch.cuda.synchronize()
    h2, q2, a2 = torch.zeros(E, N, H, device=DEV), torch.empty_like(q_buf), torch.empty_like(act_buf)
    fresh.forward_fused(obs1, h2, q_out=q2, actions_out=a2)
    torch.cuda.synchronize()
    assert torch.equal(q_buf.view(torch.int32), q2.view(torch.int32)) and torch.equal(hidden.view(torch.int32), h2.view(torch.int32))
    v.close()
