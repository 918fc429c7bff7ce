"""rg_td_targets on the GPU (csrc/td_targets.h) against the rule's twin (tests/td_targets_twin.py).

Every array the launch touches lies between sentinel guard bands; the outputs start out full of sentinels, and the rows of an
episode behind rows - 1 must keep them; every qt / obs row the rule says is not read is NaN, every such sel row out of range, and so
is the reward of every masked row: a launch that read one would show it.

none / vdn: every output word equals the float32 twin.  qmix: masks, masked rows, terminal rows and agent_q are exact; on the
unmasked rows err = max |x - twin64| / (1 + |twin64|) of the kernel must be at most 4 x the same err of the torch float32
restatement run on the device on the same inputs -- two float32 summation orders over K <= 144 + 64 + 32 + N terms differ from
float64 by a small factor of each other, not by a fixed amount -- with torch's default initialisation and with the weights x 4 (w1
of order one).  Both errors are printed before they are compared.

Episodes: slot b of a batch is, by b mod 5 (rotated by the case number, so that the batches of one to three episodes see all kinds
between them; B = 33 holds every kind): a length-1 episode, a full one (terminated at its last row), a force-closed one (full, never
terminated), an empty slot, and one of a length drawn at random.
"""
import numpy as np
import pytest
import torch

import td_targets_twin as tw
from gpu_helpers import random_actor
from td_targets_harness import CASES, DEV, GRID, NAN, Batch, make_mixer, words

pytestmark = pytest.mark.gpu


def test_the_case_table_covers_what_it_is_meant_to():
    assert 30 <= len(CASES) <= 40 and len(set(CASES)) == len(CASES)
    for kinds in (("qmix",), ("vdn", "none")):
        mine = [c for c in CASES if c[0] in kinds]
        assert {(c[1], c[2]) for c in mine} >= set(GRID)
        assert {c[1] * (c[2] - 1) for c in mine} >= {1, 33, 363, 429}              # one row; a second tile with ONE valid row; many tiles
        assert {(c[3], c[3] * c[4]) for c in mine} == {(2, 2), (5, 45), (4, 64), (8, 144)} and {c[5] for c in mine} == {2, 5, 20}
        assert all({c[6][k] for c in mine} == {0, 3} for k in range(4)) and {c[7] for c in mine} == {False, True}
    assert {c[1] * (c[2] - 1) for c in CASES if c[0] == "qmix"} >= {31, 32, 33}     # a tile short of one row, exactly one, one row more
    assert {c[0] for c in CASES} == {"qmix", "vdn", "none"}
    kinds = {(b + i) % 5 for i, c in enumerate(CASES) for b in range(c[1])}
    assert kinds == {0, 1, 2, 3, 4}


def compare_exact_parts(b, out, t_ref, mask_ref, aq_ref):
    """What is exact for every kind: the mask, agent_q, the masked rows (zero) and the terminal rows (the reward)."""
    assert np.array_equal(words(out["mask"]), words(mask_ref)), "mask"
    assert np.array_equal(words(out["agent_q"]), words(aq_ref)), "agent_q"
    dead = ~b.live
    assert np.array_equal(words(out["targets"][dead]), words(np.asarray(t_ref, np.float32)[dead])), "masked / terminal rows"
    assert not np.isnan(out["targets"][dead]).any() and not np.isnan(out["agent_q"][dead]).any()
    assert bool((out["targets"][b.mask == 0] == 0).all())


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if c[0] != "qmix"])
def test_none_and_vdn_equal_the_float32_twin_word_for_word(i):
    kind, B, rows, N, D, A, extra, with_sel = CASES[i]
    b = Batch(kind, B, rows, N, D, A, extra, with_sel, seed=i)
    out = b.run(make_mixer(kind, N, N * D), 0.99)
    t_ref, mask_ref, aq_ref = b.twin(0.99)
    assert out["targets"].shape == ((B, rows - 1, N) if kind == "none" else (B, rows - 1))
    compare_exact_parts(b, out, t_ref, mask_ref, aq_ref)
    assert np.array_equal(words(out["targets"]), words(t_ref)), CASES[i]
    assert np.isfinite(out["targets"]).all()


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if c[0] == "qmix"])
def test_qmix_is_within_four_times_torchs_float32_error_of_float64(i):
    kind, B, rows, N, D, A, extra, with_sel = CASES[i]
    for scale in (1.0, 4.0):
        b = Batch(kind, B, rows, N, D, A, extra, with_sel, seed=i)
        mixer = make_mixer(kind, N, N * D, scale, seed=i)
        out = b.run(mixer, 0.99)
        t64, mask_ref, aq_ref = b.twin(0.99, mixer.params)
        compare_exact_parts(b, out, t64, mask_ref, aq_ref)
        ref, ref_mask = b.restatement(0.99, mixer.params)
        assert np.array_equal(ref_mask, mask_ref)
        err, err_torch = tw.rel_err(out["targets"], t64, b.live), tw.rel_err(ref, t64, b.live)
        print(f"td_targets qmix case {i} {CASES[i][1:6]} x{scale:g}: {int(b.live.sum())} live rows, err kernel {err:.3e}, torch {err_torch:.3e}")
        assert np.isfinite(out["targets"]).all()
        assert err <= 4.0 * err_torch, (CASES[i], scale, err, err_torch)


@pytest.mark.parametrize("kind", ["vdn", "qmix"])
def test_a_nan_and_an_action_out_of_range_stay_in_their_row(kind):
    B, rows, N, D, A = 33, 12, 4, 16, 5
    mixer = make_mixer(kind, N, N * D, seed=1)
    clean = Batch(kind, B, rows, N, D, A, seed=3)
    out_clean = clean.run(mixer, 0.9)
    hit = Batch(kind, B, rows, N, D, A, seed=3)
    (b0, t0), (b1, t1) = [tuple(x) for x in np.argwhere(hit.live)[[2, -3]]]
    assert (b0, t0) != (b1, t1)
    a0 = int(hit.host["sel"][b0, t0 + 1, 1])
    hit.whole["qt"][b0, t0 + 1, 1, a0] = NAN                        # the value agent 1 of row (b0, t0) gathers
    hit.whole["sel"][b1, t1 + 1, 2] = A                             # agent 2 of row (b1, t1): one past the last action
    hit.before = {k: v.clone() for k, v in hit.whole.items() if k not in ("targets", "mask", "agent_q")}
    out = hit.run(mixer, 0.9)
    assert np.isnan(out["targets"][b0, t0]) and np.isnan(out["targets"][b1, t1])
    assert np.isnan(out["agent_q"][b0, t0, 1]) and np.isnan(out["agent_q"][b1, t1, 2])
    other = np.ones((B, rows - 1), bool)
    other[b0, t0] = other[b1, t1] = False
    assert np.array_equal(words(out["targets"][other]), words(out_clean["targets"][other])) and np.isfinite(out["targets"][other]).all()
    aq, aq_clean = out["agent_q"].copy(), out_clean["agent_q"].copy()
    aq[b0, t0, 1] = aq[b1, t1, 2] = aq_clean[b0, t0, 1] = aq_clean[b1, t1, 2] = 0.0
    assert np.array_equal(words(aq), words(aq_clean))


@pytest.mark.parametrize("kind", ["none", "qmix"])
def test_a_captured_call_replays_to_the_same_bits(kind):
    B, rows, N, D, A = 33, 14, 4, 16, 5
    mixer = make_mixer(kind, N, N * D, seed=2)
    eager, graphed = Batch(kind, B, rows, N, D, A, (3, 3, 3, 3), seed=4), Batch(kind, B, rows, N, D, A, (3, 3, 3, 3), seed=4)
    out = eager.run(mixer, 0.99)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    d, T = graphed.dev, rows - 1
    from marbler_amd.targets import td_targets
    with torch.cuda.graph(graph, stream=side):                     # one node, one branch
        td_targets(d["qt"], d["obs"], d["reward"], d["terminated"], d["filled"], mixer, 0.99, sel=d["sel"],
                   targets_out=graphed.whole["targets"][:, :T], mask_out=graphed.whole["mask"][:, :T], agent_q_out=graphed.whole["agent_q"][:, :T])
    torch.cuda.synchronize()
    graph.replay()                                                 # (a capture records; the replay is what runs)
    torch.cuda.synchronize()
    graphed.check_untouched()
    for name in ("targets", "mask", "agent_q"):
        assert np.array_equal(words(graphed.whole[name][:, :T]), words(out[name])), name


def test_outputs_are_allocated_when_they_are_not_given_and_bool_flags_are_taken():
    B, rows, N, D, A = 3, 12, 5, 9, 20
    b = Batch("vdn", B, rows, N, D, A, (3, 3, 0, 0), seed=6)        # (.bool() below makes contiguous copies of the flags)
    from marbler_amd.targets import td_targets
    d = b.dev
    out = td_targets(d["qt"], d["obs"], d["reward"], d["terminated"].bool(), d["filled"].bool(), make_mixer("vdn", N, N * D), 0.99, sel=d["sel"])
    torch.cuda.synchronize()
    t_ref, mask_ref, aq_ref = b.twin(0.99)
    assert all(out[k].is_contiguous() for k in out)
    assert np.array_equal(words(out["targets"]), words(t_ref)) and np.array_equal(words(out["mask"]), words(mask_ref))
    assert np.array_equal(words(out["agent_q"]), words(aq_ref))


# ---------------------------------------------------------------- end to end: what the runner collected
@pytest.mark.parametrize("one_launch", [False, True])
@pytest.mark.parametrize("kind", ["vdn", "qmix"])
def test_buffer_td_targets_against_the_restatement_on_the_batch(one_launch, kind):
    from marbler_amd.episodes import EpisodeBuffer
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    v = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", 40, time_limit=12, seed=18)
    make = lambda seed: BatchedActor(random_actor(1, v.obs_size + v.n_agents, 64, v.n_actions, True, seed=seed), v.n_agents, device=DEV)  # noqa: E731
    online, target = make(4), make(5)
    runner = BatchedRunner(v, online, epsilon=0.0, seed=9)
    # (slots three rows longer than the env's time limit: every episode is followed by padding)
    buf = EpisodeBuffer(v.E, v.n_agents, v.obs_size, v.n_actions, v.episode_limit + 3, device=DEV)
    runner.run(30, one_launch=one_launch, into=buf)
    new = buf.take_new()
    assert int(new.numel()) >= 1, "no episode completed"
    mixer = make_mixer(kind, buf.N, buf.N * buf.D, seed=7)
    greedy = buf.unroll(online, slots=new)["greedy"]
    out = buf.td_targets(target, mixer, greedy=greedy, slots=new, gamma=0.99)
    batch, qt = buf.batch(new), buf.unroll(target, slots=new)["q"]
    torch.cuda.synchronize()
    B, T = int(new.numel()), buf.L
    assert tuple(out["targets"].shape) == (B, T, 1) and tuple(out["mask"].shape) == (B, T, 1) and tuple(out["agent_q"].shape) == (B, T, buf.N)
    h = dict(qt=qt, sel=greedy, obs=batch["obs"], reward=batch["reward"][..., 0], terminated=batch["terminated"][..., 0],
             filled=batch["filled"][..., 0].to(torch.uint8))
    ref, ref_mask = tw.restatement(kind, h["qt"], h["sel"], h["obs"], h["reward"], h["terminated"], h["filled"], 0.99, mixer.params)
    n = {k: x.cpu().numpy() for k, x in h.items()}
    t_ref, mask_ref, aq_ref = tw.twin(kind, n["qt"], n["sel"], n["obs"], n["reward"], n["terminated"], n["filled"], 0.99,
                                      None if kind != "qmix" else {k: x.cpu().numpy() for k, x in mixer.params.items()})
    got = out["targets"][..., 0].cpu().numpy()
    assert np.array_equal(out["mask"][..., 0].cpu().numpy(), mask_ref) and np.array_equal(ref_mask[..., 0].cpu().numpy(), mask_ref)
    assert np.array_equal(words(out["agent_q"]), words(aq_ref))
    _, live = tw.row_flags(n["terminated"], n["filled"], T + 1)
    assert int(live.sum()) >= 12 and int((mask_ref > 0).sum()) > int(live.sum()) and int((mask_ref == 0).sum()) >= 1
    assert np.array_equal(words(got[~live]), words(np.asarray(t_ref, np.float32)[~live]))
    if kind == "vdn":
        assert np.array_equal(words(got), words(t_ref))
    else:
        err, err_torch = tw.rel_err(got, t_ref, live), tw.rel_err(ref[..., 0].cpu().numpy(), t_ref, live)
        print(f"td_targets end to end (one_launch={one_launch}): {int(live.sum())} live rows, err kernel {err:.3e}, torch {err_torch:.3e}")
        assert err <= 4.0 * err_torch, (err, err_torch)
    # trim: the same rows, cut to the longest episode
    rows = int(batch["length"].max()) + 1
    again = buf.td_targets(target, mixer, greedy=greedy[:, :rows].contiguous(), slots=new, trim=True, gamma=0.99)
    assert tuple(again["targets"].shape) == (B, rows - 1, 1)
    if kind == "vdn":
        assert np.array_equal(words(again["targets"]), words(out["targets"][:, :rows - 1]))
    v.close()
