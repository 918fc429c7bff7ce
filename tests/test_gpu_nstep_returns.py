"""rg_nstep_returns on the GPU (csrc/nstep_returns.h) against the rule's twin (tests/nstep_returns_twin.py).

Every array the launch touches lies between sentinel guard bands; the outputs start out full of sentinels, and the rows of an
episode behind `rows` (values) and `rows - 1` (returns, mask) must keep them; every obs row the rule says is not needed is NaN, and
so is the reward of every masked row and reward[T]: a launch that read one would show it.

Exact: the mask, the zeros of the rows that are not needed, and `returns`, which equals the float32 twin fed the kernel's OWN
`values` word for word -- the scan has no tolerance.  `values` on needed rows: err = max |x - v64| / (1 + |v64|) of the kernel must be
at most 4 x the same err of the torch float32 restatement (TargetCritic.forward) run on the device on the same inputs -- two float32
summation orders over chains of similar length (K <= 144 + N, 128 and 128 terms) differ from float64 by a small factor of each other,
the project's margin for this comparison in tests/test_gpu_td_targets.py -- with torch's default initialisation and with the
weights x 4.  Both errors are printed before they are compared.

Episodes: slot b of a batch is, by b mod 5 (rotated by the case number): a length-1 episode, a full one (terminated at its last
row), a force-closed one (full, never terminated), an empty slot, and one of a length drawn at random.
"""
import numpy as np
import pytest
import torch

import nstep_returns_twin as tw
from gpu_helpers import random_actor
from nstep_returns_harness import CASES, DEFAULTS, DEV, GRID, NAN, SCALED, SHAPES, STEPS, Batch, make_critic, words

pytestmark = pytest.mark.gpu


def test_the_case_table_covers_what_it_is_meant_to():
    assert 30 <= len(CASES) <= 40 and len(set(CASES)) == len(CASES)
    for kind in ("cv", "cv_ns"):
        mine = [c for c in CASES if c[0] == kind]
        assert {(c[2], c[3]) for c in mine} >= set(GRID)
        assert {(c[4], c[5]) for c in mine} == set(SHAPES) and {c[1] for c in mine} == {64, 128}
        assert {c[6] for c in mine} == set(STEPS) and {c[7] for c in mine} == {False, True} and {c[8] for c in mine} == {DEFAULTS, SCALED}
        assert {(c[1], c[7]) for c in mine} == {(h, f) for h in (64, 128) for f in (False, True)}
        assert all({c[9][k] for c in mine} == {0, 3} for k in range(4))
        assert any(c[6] > c[3] - 1 for c in mine) and any(c[6] < c[3] - 1 for c in mine)          # n above T, and below
    assert any((c[3], c[4]) == (14, 5) for c in CASES) and (14 * 5) % 32 != 0                      # 70 (row, agent) pairs: a ragged tile
    assert ("cv", 128, 2, 204, 8, 18) in {c[:6] for c in CASES}                                    # an episode's real length
    assert {c[3] for c in CASES} >= {33, 65}                                                       # row T alone in a tile of its own
    kinds = {(b + i) % 5 for i, c in enumerate(CASES) for b in range(c[2])}
    assert kinds == {0, 1, 2, 3, 4}
    long = [i for i, c in enumerate(CASES) if c[3] == 204]
    assert [(b + i) % 5 for i in long for b in range(2)] == [2, 3]                                 # a full force-closed episode and an empty slot


@pytest.mark.parametrize("i", range(len(CASES)))
def test_the_launch_against_the_twins(i):
    kind, H, B, rows, N, D, n, add, (scale, shift), extra = CASES[i]
    for wscale in (1.0, 4.0):
        b = Batch(B, rows, N, D, add, extra, seed=i)
        critic = make_critic(kind, N, N * D, H, wscale, seed=i)
        out = b.run(critic, 0.99, n, scale, shift)
        assert out["returns"].shape == (B, rows - 1, N) and out["values"].shape == (B, rows, N) and out["mask"].shape == (B, rows - 1)
        b.check_exact_parts(out, 0.99, n)                                          # checks 1 and 2
        assert np.isfinite(out["values"]).all() and np.isfinite(out["returns"]).all()
        v64, ref = b.values64(critic, scale, shift), b.torch_values(critic, scale, shift)
        err, err_torch = tw.rel_err(out["values"], v64, b.need), tw.rel_err(ref, v64, b.need)
        print(f"nstep_returns case {i} {CASES[i][:8]} weights x{wscale:g}: {int(b.need.sum())} needed rows, err kernel {err:.3e}, torch {err_torch:.3e}")
        assert err <= 4.0 * err_torch, (CASES[i], wscale, err, err_torch)           # check 3


@pytest.mark.parametrize("kind", ["cv", "cv_ns"])
def test_a_nan_reaches_what_the_rule_says_and_nothing_else(kind):
    B, rows, N, D, n = 33, 14, 4, 16, 5
    T = rows - 1
    critic = make_critic(kind, N, N * D, 128, seed=1)
    clean = Batch(B, rows, N, D, True, seed=3)
    out_clean = clean.run(critic, 0.9, n)
    hit = Batch(B, rows, N, D, True, seed=3)
    full = [b for b in range(B) if hit.m[b].all()]                                 # full episodes: every row needed
    b0, b1 = full[0], full[1]
    t0 = n + 2                                                                     # a middle row: read by (b0, t0 - n) alone, at k == n
    hit.whole["obs"][b0, t0, 1, 3] = NAN
    hit.whole["obs"][b1, T, 0, 0] = NAN                                            # row T: read by every row whose window reaches T - 1
    hit.before = {k: v.clone() for k, v in hit.whole.items() if k not in ("returns", "values", "mask")}
    out = hit.run(critic, 0.9, n)
    bad_v = np.zeros((B, rows), bool)
    bad_v[b0, t0] = bad_v[b1, T] = True
    assert np.isnan(out["values"][bad_v]).all() and np.isfinite(out["values"][~bad_v]).all()
    assert np.array_equal(words(out["values"][~bad_v]), words(out_clean["values"][~bad_v]))
    bad_r = np.zeros((B, T), bool)
    bad_r[b0, t0 - n] = True
    bad_r[b1, T - n:] = True
    assert np.isnan(out["returns"][bad_r]).all() and np.isfinite(out["returns"][~bad_r]).all()
    assert np.array_equal(words(out["returns"][~bad_r]), words(out_clean["returns"][~bad_r]))
    assert np.array_equal(words(out["mask"]), words(out_clean["mask"]))


@pytest.mark.parametrize("kind,H", [("cv", 128), ("cv_ns", 64)])
def test_a_captured_call_replays_to_the_same_bits(kind, H):
    B, rows, N, D, n = 33, 14, 4, 16, 5
    critic = make_critic(kind, N, N * D, H, seed=2)
    eager, graphed = Batch(B, rows, N, D, True, (3, 3, 3, 3), seed=4), Batch(B, rows, N, D, True, (3, 3, 3, 3), seed=4)
    out = eager.run(critic, 0.99, n, 1.7, -0.3)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    d = graphed.dev
    from marbler_amd.returns import nstep_returns
    with torch.cuda.graph(graph, stream=side):                     # one node, one branch
        nstep_returns(d["obs"], d["reward"], d["terminated"], d["filled"], critic, 0.99, n, True, 1.7, -0.3, **graphed.outs())
    torch.cuda.synchronize()
    graph.replay()                                                 # (a capture records; the replay is what runs)
    torch.cuda.synchronize()
    graphed.check_untouched()
    for name, view in graphed.outs().items():
        assert np.array_equal(words(view), words(out[name[:-4]])), name


def test_outputs_are_allocated_when_they_are_not_given_and_bool_flags_are_taken():
    B, rows, N, D, n = 3, 12, 5, 9, 10
    b = Batch(B, rows, N, D, True, (3, 0, 0, 0), seed=6)
    from marbler_amd.returns import nstep_returns
    d = b.dev
    critic = make_critic("cv", N, N * D, 64, seed=6)
    out = nstep_returns(d["obs"], d["reward"], d["terminated"].bool(), d["filled"].bool(), critic, 0.99, n)
    torch.cuda.synchronize()
    assert all(out[k].is_contiguous() for k in out)
    assert tuple(out["returns"].shape) == (B, rows - 1, N) and tuple(out["values"].shape) == (B, rows, N) and tuple(out["mask"].shape) == (B, rows - 1)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    b.check_exact_parts(got, 0.99, n)
    again = b.run(critic, 0.99, n)
    assert all(np.array_equal(words(got[k]), words(again[k])) for k in got)


# ---------------------------------------------------------------- end to end: what the runner collected
@pytest.mark.parametrize("kind", ["cv", "cv_ns"])
def test_buffer_nstep_returns_against_twin_and_restatement_on_the_batch(kind):
    from marbler_amd.episodes import EpisodeBuffer
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    v = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", 40, time_limit=12, seed=18)
    actor = BatchedActor(random_actor(1, v.obs_size + v.n_agents, 64, v.n_actions, True, seed=4), v.n_agents, device=DEV)
    runner = BatchedRunner(v, actor, epsilon=0.0, seed=9, action_selector="soft_policies")
    # (slots three rows longer than the env's time limit: every episode is followed by padding)
    buf = EpisodeBuffer(v.E, v.n_agents, v.obs_size, v.n_actions, v.episode_limit + 3, with_prob=True, device=DEV)
    runner.run(30, one_launch=True, into=buf)
    new = buf.take_new()
    assert int(new.numel()) >= 1, "no episode completed"
    critic = make_critic(kind, buf.N, buf.N * buf.D, 128, seed=7)
    gamma, n = 0.99, 5
    out = buf.nstep_returns(critic, slots=new, gamma=gamma, nstep=n)
    batch = buf.batch(new)
    torch.cuda.synchronize()
    B, T, N = int(new.numel()), buf.L, buf.N
    assert tuple(out["returns"].shape) == (B, T, N) and tuple(out["values"].shape) == (B, T + 1, N) and tuple(out["mask"].shape) == (B, T, 1)
    obs, reward = batch["obs"], batch["reward"][..., 0]
    terminated, filled = batch["terminated"][..., 0], batch["filled"][..., 0].to(torch.uint8)
    h = {k: x.cpu().numpy() for k, x in dict(obs=obs, reward=reward, terminated=terminated, filled=filled).items()}
    m = tw.mask_of(h["terminated"], h["filled"], T + 1)
    got = {k: x.cpu().numpy() for k, x in out.items()}
    assert np.array_equal(got["mask"][..., 0], m.astype(np.float32))
    need = tw.needed_rows(m, True)
    assert int(m.sum()) >= 12 and int((~m).sum()) >= B and not need[:, -1].any()       # padding behind every episode: row T is never needed
    assert not got["values"][~need].any() and not got["returns"][~m].any()
    assert np.array_equal(words(got["returns"]), words(tw.returns32(got["values"], h["reward"], m, gamma, n, True)))
    v64, _ = tw.values64(kind, {k: x.cpu().numpy() for k, x in critic.params.items()}, h["obs"], h["terminated"], h["filled"], True)
    ret, vals, mask = tw.restatement(critic.forward, obs, reward, terminated, filled, gamma, n, True)
    torch.cuda.synchronize()
    assert np.array_equal(mask.cpu().numpy()[..., 0], m.astype(np.float32))
    err, err_torch = tw.rel_err(got["values"], v64, need), tw.rel_err(vals.cpu().numpy(), v64, need)
    print(f"nstep_returns end to end ({kind}): {int(need.sum())} needed rows, err kernel {err:.3e}, torch {err_torch:.3e}")
    assert err <= 4.0 * err_torch, (err, err_torch)
    # EPyMARL's returns on the rows the two rules share (the others carry a padding row's value there); the values differ by
    # float32 rounding, the scan adds at most n + 1 terms of them
    differs, _ = tw.differing_rows(m, n, True)
    same = m & ~differs
    assert int(same.sum()) >= 12 and int(differs.sum()) >= 1
    assert tw.rel_err(got["returns"], ret.cpu().numpy(), same) <= 8.0 * max(err, err_torch)
    # trim: the same rows, cut to the longest episode
    rows = int(batch["length"].max()) + 1
    again = buf.nstep_returns(critic, slots=new, trim=True, gamma=gamma, nstep=n)
    torch.cuda.synchronize()
    assert tuple(again["returns"].shape) == (B, rows - 1, N) and tuple(again["values"].shape) == (B, rows, N)
    a = {k: x.cpu().numpy() for k, x in again.items()}
    mt = tw.mask_of(h["terminated"], h["filled"], rows)
    assert np.array_equal(a["mask"][..., 0], mt.astype(np.float32))
    assert np.array_equal(words(a["returns"]), words(tw.returns32(a["values"], h["reward"], mt, gamma, n, True)))
    # a row's values do not depend on the batch's cut (row T of the trimmed batch can be needed now: the longest episode's last row)
    keep = tw.needed_rows(mt, True) & need[:, :rows]
    assert np.array_equal(words(a["values"][keep]), words(got["values"][:, :rows][keep]))
    # a replacement reward (a learner that standardises rewards) is what the scan then reads
    scaled = (reward * 0.5).contiguous()
    half = buf.nstep_returns(critic, slots=new, gamma=gamma, nstep=n, reward=scaled)
    torch.cuda.synchronize()
    assert np.array_equal(words(half["returns"].cpu().numpy()), words(tw.returns32(got["values"], scaled.cpu().numpy(), m, gamma, n, True)))
    v.close()
