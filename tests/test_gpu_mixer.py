"""rg_mixer_forward / rg_mixer_backward and TrainableMixer on the GPU (csrc/mixer_grad.h) against the rule's twin (tests/mixer_twin.py).

Every array a launch touches lies between sentinel guard bands; the outputs start out full of sentinels, and the rows behind the last
row that the rule writes must keep them; every q, actions and obs row the rule says is not read -- masked rows and row T -- holds NaN
or an out-of-range action: a launch that read one would show it.  The states of the live rows are chosen off the kinks
(mixer_harness.draw); no row is left out of a comparison.

Exact: the masked rows (zero), d_q off the chosen action and in row T (zero), the per-row arrays' zeros.  none / vdn: every word equals
the float32 twin.  qmix: err = max |x - twin64| / (1 + |twin64|) over ALL elements of mixed, d_q, d_pre, d_p2, g, and through
TrainableMixer of every parameter gradient and of the gradient that reaches q, must be at most 4 x the same err of forward_reference
in float32 under autograd on the device on the same inputs (the project's standing bound for float32 launches with a summation order
of their own), with torch's default initialisation and with the weights x 4.  The torch error must be above zero -- except where
both errors are exactly zero: a gradient that is one number copied, as V.2.bias' from a single live row.  Both are printed first.

Episodes are of the five kinds tests/test_gpu_td_targets.py describes.
"""
import numpy as np
import pytest
import torch

import mixer_twin as tw
from mixer_harness import BAD_ACTION, CASES, DEV, GRID, NAN, SCALES, Batch, draw, words

pytestmark = pytest.mark.gpu


def rel_err(x, t):
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    return float((np.abs(x - t) / (1.0 + np.abs(t))).max())


def held(what, got, ref32, t64, worst):
    err, err_torch = rel_err(got, t64), rel_err(ref32, t64)
    print(f"    {what}: err kernel {err:.3e}, torch {err_torch:.3e}")
    assert np.isfinite(np.asarray(got)).all(), what
    assert err_torch > 0.0 or err == 0.0, (what, "the float32 reference is exact: it bounds nothing")
    assert err <= 4.0 * err_torch, (what, err, err_torch)
    if err_torch > 0.0:
        worst.append(err / err_torch)


def test_the_case_table_covers_what_it_is_meant_to():
    assert len(CASES) <= 34 and len(set(CASES)) == len(CASES)
    for kinds in (("qmix",), ("vdn", "none")):
        mine = [c for c in CASES if c[0] in kinds]
        assert {(c[1], c[2]) for c in mine} >= set(GRID)
        assert {c[1] * (c[2] - 1) for c in mine} >= {1, 33, 363, 429}
        assert {(c[3], c[3] * c[4]) for c in mine} == {(1, 3), (2, 2), (5, 45), (4, 64), (8, 144), (16, 256)}
        assert {c[5] for c in mine} == {2, 5, 20} and all({c[6][k] for c in mine} == {0, 3} for k in range(4))
    assert {c[1] * (c[2] - 1) for c in CASES if c[0] == "qmix"} >= {1, 31, 32, 33}
    assert any(c[3] > 8 for c in CASES if c[0] == "qmix") and any(c[3] <= 8 for c in CASES if c[0] == "qmix")   # both backward kernels


def exact_parts(b, out):
    """What is exact for every kind: zeros wherever the rule says zero, and nothing but the chosen action in d_q."""
    h, T = b.host, b.T
    dead = ~h["live"]
    assert bool((out["mixed"][dead] == 0).all()), "masked rows of mixed"
    d_q = out["d_q"]
    assert bool((d_q[:, T] == 0).all()) and bool((d_q[:, :T][dead] == 0).all()), "row T and the masked rows of d_q"
    chosen = np.zeros(d_q.shape, bool)
    for bb, t in np.argwhere(h["live"]):
        for n in range(b.N):
            if 0 <= h["actions"][bb, t, n] < b.A:
                chosen[bb, t, n, h["actions"][bb, t, n]] = True
    assert bool((d_q[~chosen] == 0).all()), "d_q off the chosen action"
    for k in ("d_pre", "d_p2", "g"):
        if k in out:
            assert bool((out[k][:, T] == 0).all()) and bool((out[k][:, :T][dead] == 0).all()), k


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if c[0] != "qmix"])
def test_none_and_vdn_equal_the_float32_twin_word_for_word(i):
    b = Batch(CASES[i], seed=i)
    out = b.run()
    exact_parts(b, out)
    h = b.host
    mixed, d_q = tw.gather_twin(b.kind, h["q"], h["actions"], h["mask"], h["d_mixed"])
    assert np.array_equal(words(out["mixed"]), words(mixed)) and np.array_equal(words(out["d_q"]), words(d_q)), CASES[i]
    # through the module: the same words
    m = b.module()
    q = b.dev["q"].clone().requires_grad_(True)
    y = m(q, b.dev["actions"], b.dev["obs"], b.dev["mask"])
    y.backward(b.dev["d_mixed"])
    assert np.array_equal(words(y), words(mixed)) and np.array_equal(words(q.grad), words(d_q))


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if c[0] == "qmix"])
def test_qmix_is_within_four_times_torchs_float32_error_of_float64(i):
    worst = []
    for scale in SCALES:
        b = Batch(CASES[i], scale, seed=i)
        print(f"mixer qmix case {i} {CASES[i][1:6]} x{scale:g}: {int(b.host['live'].sum())} live rows, {b.host['draws']} draws")
        out = b.run()
        exact_parts(b, out)
        t64 = b.twin()
        ref32, grads32 = b.reference(torch.float32)
        for k in ("mixed", "d_q", "d_pre", "d_p2", "g"):
            held(k, out[k], ref32[k], t64[k], worst)
        # through TrainableMixer: the gradient that reaches q and every parameter's
        m = b.module()
        q = b.dev["q"].clone().requires_grad_(True)
        y = m(q, b.dev["actions"], b.dev["obs"], b.dev["mask"])
        y.backward(b.dev["d_mixed"])
        assert np.array_equal(words(y), words(out["mixed"])) and np.array_equal(words(q.grad), words(out["d_q"]))
        for k, p in m.named_parameters():
            held("grad " + k, p.grad.cpu().numpy(), grads32[k], t64["grads"][k], worst)
    print(f"mixer qmix case {i}: the largest err kernel / err torch is {max(worst):.2f}")


def test_two_calls_and_a_batch_of_1_and_of_33_give_the_same_words():
    case = ("qmix", 33, 12, 5, 9, 5, (0, 3, 0, 3))
    host = draw(case, seed=3)
    first, again = Batch(case, host=host).run(), Batch(case, host=host).run()
    for k in first:
        assert np.array_equal(words(first[k]), words(again[k])), k
    for e in (0, 7, 32):           # an episode alone: a different tile, a different place in it
        one = {k: (v[e:e + 1] if isinstance(v, np.ndarray) else v) for k, v in host.items()}
        alone = Batch(("qmix", 1) + case[2:], host=one).run()
        for k in first:
            assert np.array_equal(words(first[k][e:e + 1]), words(alone[k])), (k, e)


@pytest.mark.parametrize("kind", ["qmix", "vdn"])
def test_a_nan_and_an_action_out_of_range_stay_in_their_row(kind):
    case = (kind, 3, 12, 4, 16, 5, (3, 0, 3, 0))
    host = draw(case, seed=1)
    clean = Batch(case, host=host).run()
    rows = np.argwhere(host["live"])
    (b0, t0), (b1, t1) = rows[1], rows[-2]
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in host.items()}
    bad["q"][b0, t0, 2, bad["actions"][b0, t0, 2]] = NAN
    bad["actions"][b1, t1, 1] = BAD_ACTION
    out = Batch(case, host=bad).run()                       # (run() checks the guard bands: nothing out of bounds was touched)
    hit = np.zeros(host["live"].shape, bool)
    hit[b0, t0] = hit[b1, t1] = True
    assert np.isnan(out["mixed"][hit]).all()
    assert bool((out["d_q"][b1, t1, 1] == 0).all()), "an agent whose action is out of range has zeros alone"
    for k in out:
        a, c = out[k][:, :host["live"].shape[1]], clean[k][:, :host["live"].shape[1]]
        assert np.array_equal(words(a[~hit]), words(c[~hit])), (k, "a row that was not poisoned changed")


def test_a_captured_forward_and_backward_pair_replays_and_outputs_are_allocated_when_not_given():
    from marbler_amd.mixers import mixer_backward, mixer_forward
    case = ("qmix", 3, 12, 4, 16, 5, (0, 0, 0, 0))
    host = draw(case, seed=2)
    want = Batch(case, host=host).run()
    b = Batch(case, host=host)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b.forward(), b.backward()                            # (the library is loaded and typed before the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in b.outs:
        b.whole[k][:, :b.outs[k][1]] = 5.0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        b.forward(), b.backward()
    graph.replay()
    torch.cuda.synchronize()
    b.check_untouched()
    for k in want:
        assert np.array_equal(words(b.out(k)), words(want[k])), k
    d = b.dev
    mixed = mixer_forward(d["q"], d["actions"], d["obs"], d["mask"], b.mixer)
    outs = mixer_backward(d["q"], d["actions"], d["obs"], d["mask"], d["d_mixed"], b.mixer)
    for k, v in zip(("mixed", "d_q", "d_pre", "d_p2", "g"), (mixed,) + outs):
        assert np.array_equal(words(v), words(want[k])), k


def _reference_loss(actor, mixer, obs, actions, mask, targets, dtype):
    q = actor.forward_reference(obs.to(dtype))
    mixed = mixer.forward_reference(q, actions, obs.to(dtype), mask)
    return (((mixed - targets.to(dtype)) * mask.to(dtype)) ** 2).sum() / mask.to(dtype).sum()


def test_a_masked_qmix_td_loss_through_actor_and_mixer_against_float64_autograd():
    """Every actor and mixer parameter gradient of Sum ((mixed - targets) mask)^2 / Sum mask, targets from td_targets, on the smallest
    batch that takes more than one tile: 3 episodes of 14 rows, 39 flat rows.  Measured on other batches, for the record: the
    actor's rnn.weight_ih, whose gradient TrainableActor forms in ONE torch GEMM over all B rows N rows where the reference loop adds
    up one GEMM per step, lay at 3.3 x and 4.1 x torch's float32 error in two runs of 6 episodes of 9 rows (6.6e-8 against 1.6e-8:
    one rounding of a single word against a quarter of one) and at 7.2 x in 33 episodes of 12 rows (1.2e-7 against 1.7e-8); every
    other parameter, all of the mixer's included, lay below 2 x."""
    import copy
    from marbler_amd import TargetMixer, TrainableActor, TrainableMixer, td_targets
    case = ("qmix", 3, 14, 4, 16, 5, (0, 0, 0, 0))
    h = draw(case, seed=5, poison=False)
    B, rows, N, D, A = case[1:6]
    rng = np.random.default_rng(7)
    _, terminated, filled = __import__("td_targets_harness").draw_episodes(B, rows, np.random.default_rng(1005), 5)   # draw()'s own
    dev = lambda x: torch.from_numpy(x).to(DEV)   # noqa: E731
    obs, actions = dev(h["obs"]), dev(h["actions"])
    target = TargetMixer("qmix", N, N * D, device=DEV, seed=9)
    qt = dev(rng.standard_normal((B, rows, N, A)).astype(np.float32))
    out = td_targets(qt, obs, dev(rng.standard_normal((B, rows)).astype(np.float32)), dev(terminated), dev(filled), target, 0.99)
    mask, targets = out["mask"], out["targets"]
    assert np.array_equal(mask.cpu().numpy() != 0, h["live"])
    torch.manual_seed(3)
    actor = TrainableActor(N, D + N, 64, A, device=DEV)
    mixer = TrainableMixer("qmix", N, N * D, device=DEV)
    mixer.load_state_dict(h["params"])
    mixed = mixer(actor(obs), actions, obs, mask)
    loss = (((mixed - targets) * mask) ** 2).sum() / mask.sum()
    loss.backward()
    got = {"actor." + k: p.grad.cpu().numpy() for k, p in actor.named_parameters()}
    got.update({"mixer." + k: p.grad.cpu().numpy() for k, p in mixer.named_parameters()})
    refs = []
    for dtype in (torch.float32, torch.float64):
        a, m = copy.deepcopy(actor).to(dtype), copy.deepcopy(mixer).to(dtype)
        a.zero_grad(), m.zero_grad()
        _reference_loss(a, m, obs, actions, mask, targets, dtype).backward()
        ref = {"actor." + k: p.grad.cpu().numpy() for k, p in a.named_parameters()}
        ref.update({"mixer." + k: p.grad.cpu().numpy() for k, p in m.named_parameters()})
        refs.append(ref)
    worst = []
    for k in got:
        held(k, got[k], refs[0][k], refs[1][k], worst)
    print(f"td loss through actor and mixer: the largest err kernel / err torch is {max(worst):.2f}")


def test_a_training_cycle_on_collected_data_runs_and_stays_finite():
    """Finiteness and mechanics only, no error bound: collect, one SGD step on actor and mixer, reload both networks, a second
    td_targets and a second step."""
    from marbler_amd import EpisodeBuffer, TargetMixer, TrainableActor, TrainableMixer
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    from gpu_helpers import random_actor
    v = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", 8, time_limit=12, seed=18)
    N, D, A, H = v.n_agents, v.obs_size, v.n_actions, 64
    sd = random_actor(1, D + N, H, A, True, seed=4)
    online, target_actor = BatchedActor(sd, N, device=DEV), BatchedActor(sd, N, device=DEV)
    runner = BatchedRunner(v, online, epsilon=0.0, seed=9, action_selector="soft_policies")
    buf = EpisodeBuffer.for_runner(runner)
    runner.run(30, into=buf)
    slots = buf.take_new()
    assert slots.numel() >= 1, "no episode completed"
    target = TargetMixer("qmix", N, N * D, device=DEV, seed=2)
    actor, mixer = TrainableActor.from_actor(online), TrainableMixer.from_target(target)
    params = list(actor.parameters()) + list(mixer.parameters())
    opt = torch.optim.SGD(params, lr=1e-2)
    losses = []
    for _ in range(2):
        greedy = buf.unroll(online, slots)["greedy"]
        out = buf.td_targets(target_actor, target, greedy, slots)
        q = actor(buf.batch(slots)["obs"])
        mixed = buf.mixed_q(mixer, q, out["mask"], slots)
        assert mixed.shape == out["targets"].shape
        loss = (((mixed - out["targets"]) * out["mask"]) ** 2).sum() / out["mask"].sum()
        opt.zero_grad()
        loss.backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
        before = [p.detach().clone() for p in params]
        opt.step()
        assert any(not torch.equal(a, p.detach()) for a, p in zip(before, params))
        online.load_state_dict(actor.state_dict())
        target_actor.load_state_dict(actor.state_dict())
        target.load_state_dict(mixer.state_dict())
        losses.append(loss.item())
    assert all(np.isfinite(x) for x in losses), losses
    new = target.state_dict()
    assert all(torch.equal(new[k], p.detach()) for k, p in mixer.state_dict().items())
