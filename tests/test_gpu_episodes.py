"""rg_episodes_append on the GPU against the NumPy twin of the rule (csrc/episodes.h; tests/episodes_twin.py): every array of the
buffer and every cursor word for word -- the launch copies rows and adds binary32 rewards in step order, so nothing here has a
tolerance except the one comparison with the env's own statistics, whose sum runs in another order.  Every buffer of this file
lies between sentinel-filled guard bands and starts out full of sentinels, the twin's copy of it too."""
import itertools

import numpy as np
import pytest
import torch

import episodes_cases as ec
from episodes_twin import DTYPES, TwinBuffer, shapes
from gpu_helpers import random_actor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256                                   # elements on either side of an array
SENTINELS = {np.float32: -777.25, np.int32: -77777, np.uint8: 0xA5}
ROW_ARRAYS = ("obs", "actions", "reward", "terminated", "filled", "prob")


class Guarded(object):
    """An EpisodeBuffer whose arrays each lie between two guard bands, and its twin.  The row arrays start out as sentinels (in
    the twin too); the per-slot arrays and the cursors as a fresh buffer's.  shift: elements the obs array is moved off its
    16-byte alignment by (the launch then copies with 8- or 4-byte pieces)."""

    def __init__(self, E, R, L, N, D, with_prob, shift=0):
        from marbler_amd.episodes import EpisodeBuffer
        self.raw, storage, start = {}, {}, {}
        for k, shape in shapes(E, R, L, N, D).items():
            if k == "prob" and not with_prob:
                continue
            n, lo = int(np.prod(shape)), GUARD + (shift if k == "obs" else 0)
            raw = np.full(lo + n + GUARD, SENTINELS[DTYPES[k]], DTYPES[k])
            if k not in ROW_ARRAYS:
                raw[lo:lo + n] = 0
            if k == "cursor":
                raw[lo:lo + n:4] = -1
            start[k] = raw[lo:lo + n].reshape(shape).copy()
            self.raw[k] = (torch.from_numpy(raw).to(DEV), lo, n)
            storage[k] = self.raw[k][0][lo:lo + n].view(shape)
        self.buf = EpisodeBuffer(E, N, D, 5, L, slots_per_env=R, with_prob=with_prob, device=DEV, storage=storage)
        self.twin = TwinBuffer(E, R, L, N, D, with_prob, arrays=start)

    def append(self, batch):
        """one call through both; the stream tensors must come back unchanged"""
        dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in batch.items()}
        self.buf.append(dev)
        self.twin.append(batch)
        torch.cuda.synchronize()
        for k, v in batch.items():
            assert np.array_equal(dev[k].cpu().numpy().view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), ("stream changed", k)

    def check(self, what):
        for k, (raw, lo, n) in self.raw.items():
            host = raw.cpu().numpy()
            sentinel = np.array(SENTINELS[DTYPES[k]], DTYPES[k])
            assert (host[:lo] == sentinel).all() and (host[lo + n:] == sentinel).all(), (what, k, "guard band damaged")
            want = np.ascontiguousarray(getattr(self.twin, k)).reshape(-1)
            bits = np.uint32 if want.itemsize == 4 else np.uint8
            differ = np.flatnonzero(host[lo:lo + n].view(bits) != want.view(bits))
            assert differ.size == 0, (what, k, differ[:8].tolist(), host[lo:lo + n][differ[:8]].tolist(), want[differ[:8]].tolist())


# N, D pairs: rows of 1, 3, 8, 45, 54 and 144 floats (4-, 8- and 16-byte pieces)
WIDTHS = ((1, 1), (3, 1), (2, 4), (5, 9), (6, 9), (8, 18))
OTHERS = list(itertools.product((1, 7, 12), (1, 3), (1, 2, 3), (False, True), (0.0, 0.3, 1.0)))       # T, L, R, prob, rate


@pytest.mark.parametrize("E", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("width", WIDTHS, ids=lambda w: "row%d" % (w[0] * w[1]))
def test_synthetic_streams_equal_the_twin_word_for_word(E, width):
    """Three consecutive calls into one buffer, for every T, L, R, prob setting and termination rate; with L this small and the
    rates this high the envs wrap their ring inside one launch.  Compared after the third call (and the guards with it)."""
    N, D = width
    for i, (T, L, R, prob, rate) in enumerate(OTHERS):
        g = Guarded(E, R, L, N, D, prob, shift=(0, 0, 1, 2)[i % 4] if (N * D) % 4 == 0 else 0)
        for batch in ec.synthetic_calls(1000 * E + i, 3, T, E, N, D, rate, prob):
            g.append(batch)
        g.check((E, width, T, L, R, prob, rate))
        wrapped = g.twin.cursor[:, 2].max() > R
        assert wrapped or rate < 1.0 or 3 * T <= R, "the case was meant to wrap the ring"


@pytest.mark.parametrize("T", [64, 65, 150])
def test_more_than_one_chunk_of_time_steps(T):
    """The launch takes 64 time steps at a go: a call on the boundary, one over it, and one of three chunks with episodes across
    the boundaries (L = 81 and rate 0.02: most episodes run into the next chunk, some into the limit)."""
    for L, R, rate in ((81, 2, 0.02), (3, 2, 0.3), (200, 1, 0.0)):
        g = Guarded(5, R, L, 4, 16, True)
        for batch in ec.synthetic_calls(T + L, 2, T, 5, 4, 16, rate, True):
            g.append(batch)
        g.check((T, L, R, rate))


@pytest.mark.parametrize("name", list(ec.HAND_CASES))
def test_named_edge_cases(name):
    case = ec.HAND_CASES[name]
    g = Guarded(len(case["calls"][0]), case["R"], case["L"], case["N"], case["D"], case["with_prob"])
    for batch in ec.hand_calls(case):
        g.append(batch)
        g.check(name)


def test_starts_that_cut_episodes_off_and_a_buffer_attached_late():
    """episode_start drawn independently of terminated (open episodes are abandoned, ended ones wait for a start), and a collector
    that was already running when the buffer joined."""
    rng = np.random.default_rng(11)
    for E, R, L in ((65, 2, 3), (7, 1, 2), (64, 3, 5)):
        g = Guarded(E, R, L, 2, 4, False)
        for batch in ec.synthetic_calls(E, 3, 12, E, 2, 4, 0.2, False):
            batch["episode_start"] = rng.random(batch["episode_start"].shape) < 0.25
            g.append(batch)
        g.check(("independent starts", E, R, L))
        g = Guarded(E, R, L, 2, 4, True)
        for batch in ec.synthetic_calls(E, 3, 12, E, 2, 4, 0.2, True, attached=False):
            g.append(batch)
        g.check(("attached late", E, R, L))


def test_take_new_batch_and_sample():
    E, R, L, N, D = 65, 2, 3, 3, 4
    g = Guarded(E, R, L, N, D, True)
    seen = np.zeros(E * R, bool)
    for batch in ec.synthetic_calls(5, 3, 7, E, N, D, 0.3, True):
        g.append(batch)
        want = g.twin.take_new()
        new = g.buf.take_new()
        assert new.dtype == torch.int64 and new.device.type == "cuda" and new.cpu().numpy().tolist() == want.tolist() and want.size > 0
        assert g.buf.take_new().numel() == 0                                    # exactly once
        g.check("after take_new")
        seen[want] = True
        out = g.buf.batch(new)
        B = want.size
        assert {k: (tuple(v.shape), v.dtype) for k, v in out.items()} == {
            "obs": ((B, L + 1, N, D), torch.float32), "state": ((B, L + 1, N * D), torch.float32),
            "actions": ((B, L + 1, N, 1), torch.int64), "avail_actions": ((B, L + 1, N, 5), torch.int32),
            "reward": ((B, L + 1, 1), torch.float32), "terminated": ((B, L + 1, 1), torch.uint8),
            "filled": ((B, L + 1, 1), torch.int64), "probs": ((B, L + 1, N), torch.float32), "length": ((B,), torch.int32),
            "episode_return": ((B,), torch.float32)}
        length = out["length"].cpu().numpy()
        assert np.array_equal(length, g.twin.length[want]) and (length >= 1).all()
        filled = out["filled"][:, :, 0].cpu().numpy()
        assert np.array_equal(filled, (np.arange(L + 1)[None, :] < length[:, None] + 1).astype(np.int64))     # the prefix length + 1
        assert np.array_equal(out["obs"].cpu().numpy(), g.twin.obs[want]) and np.array_equal(out["state"].cpu().numpy().reshape(B, L + 1, N, D), g.twin.obs[want])
        assert np.array_equal(out["actions"][..., 0].cpu().numpy(), g.twin.actions[want]) and bool(out["avail_actions"].all())
        assert np.array_equal(out["episode_return"].cpu().numpy(), g.twin.episode_return[want])
        short = new[out["length"] < L]
        if short.numel():
            trimmed = g.buf.batch(short, trim=True)
            rows = int(g.twin.length[short.cpu().numpy()].max()) + 1
            assert rows < L + 1 and trimmed["obs"].shape == (short.numel(), rows, N, D) and trimmed["filled"].shape == (short.numel(), rows, 1)
            assert torch.equal(trimmed["reward"], g.buf.batch(short)["reward"][:, :rows])
    complete = np.flatnonzero(g.twin.complete)
    assert np.array_equal(g.buf.batch()["length"].cpu().numpy(), g.twin.length[complete])
    gen = torch.Generator(device=DEV).manual_seed(3)
    first = g.buf.sample(16, generator=gen)
    assert first.dtype == torch.int64 and len(set(first.tolist())) == 16 and set(first.tolist()) <= set(complete.tolist())
    assert torch.equal(first, g.buf.sample(16, generator=torch.Generator(device=DEV).manual_seed(3)))
    assert not torch.equal(first, g.buf.sample(16, generator=gen))
    with pytest.raises(ValueError):
        g.buf.sample(complete.size + 1)
    assert int(g.buf.overflowed()) == int(g.twin.cursor[:, 3].sum()) > 0
    # a checkpoint keeps the open episodes: a restored buffer goes on exactly like the one it was taken from
    from marbler_amd.episodes import EpisodeBuffer
    other = EpisodeBuffer(E, N, D, 5, L, slots_per_env=R, with_prob=True, device=DEV)
    other.load_state_dict(g.buf.state_dict())
    more = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in ec.synthetic_calls(6, 1, 7, E, N, D, 0.3, True, attached=False)[0].items()}
    other.append(more)
    g.buf.append(more)
    assert all(torch.equal(getattr(other, k), getattr(g.buf, k)) for k in g.buf.names)


def test_append_under_stream_capture_equals_the_eager_call():
    E, R, L, N, D = 65, 2, 3, 4, 16
    calls = ec.synthetic_calls(8, 2, 12, E, N, D, 0.3, True)
    eager, graphed = Guarded(E, R, L, N, D, True), Guarded(E, R, L, N, D, True)
    for g in (eager, graphed):
        g.append(calls[0])
    second = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in calls[1].items()}
    eager.buf.append(second)
    eager.twin.append(calls[1])
    eager.check("eager")
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):                     # one node, one branch
        graphed.buf.append(second)
    torch.cuda.synchronize()
    graph.replay()                                                 # (a capture records; the replay is what runs)
    torch.cuda.synchronize()
    graphed.twin.append(calls[1])
    graphed.check("graph replay")
    assert all(torch.equal(getattr(eager.buf, k), getattr(graphed.buf, k)) for k in eager.buf.names)


# ---------------------------------------------------------------- end to end: the runner's stream
# Two slots per env hold every episode between two take_new calls as long as no env opens a third episode inside one call, that
# is, ends two with steps to spare.  With the 20-step time limit alone that cannot happen in 25 steps, but PredatorCapturePrey
# also ends an episode on a collision, and a sampling policy collides: measured over the env seeds 0..23 with this actor, the
# greedy runner has such an env for 3 seeds (2, 14, 17) and the soft-policies runner for every seed but 18 (2 to 13 envs).  That
# is a property of the stream, not of the buffer -- the synthetic cases above hold the buffer to the rule when the ring does
# wrap -- so this test collects with a seed whose streams leave two slots enough, 18, and checks that premise on the dicts the
# runner returned before it relies on it.
ENV_SEED = 18


def _collect(selector, one_launch):
    """Three run(25, into=buf) of 64 PredatorCapturePrey envs with a 20-step time limit -> (buffer, the dicts, the episodes taken
    after each call as NumPy, the venv's statistics, overflowed(), agents whose rewards a step's `reward` adds up)."""
    from marbler_amd.episodes import EpisodeBuffer
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    v = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", 64, time_limit=20, seed=ENV_SEED)
    actor = BatchedActor(random_actor(1, v.obs_size + v.n_agents, 64, v.n_actions, True, seed=4), v.n_agents, device=DEV)
    runner = BatchedRunner(v, actor, seed=9, action_selector=selector)
    buf = EpisodeBuffer.for_runner(runner, slots_per_env=2)
    assert buf.with_prob == (selector == "soft_policies") and (buf.E, buf.L, buf.R) == (64, 20, 2)
    dicts, taken, index_at_take = [], [], {}
    for _ in range(3):
        out = runner.run(25, one_launch=one_launch, into=buf)
        ends = out["terminated"].cpu().numpy()
        second = np.where(ends.sum(0) >= 2, np.argsort(~ends, axis=0, kind="stable")[1], 25)       # the step of an env's second end
        assert (second >= 24).all(), "ENV_SEED: an env of this stream opens a third episode inside one call; two slots cannot hold that"
        new = buf.take_new()
        # no complete-but-untaken slot was overwritten: every episode an env finished shows up exactly once, in order
        for env, ep in sorted(zip((new // 2).tolist(), buf.episode_index[new].tolist())):
            assert ep == index_at_take.get(env, -1) + 1, (env, ep, "an episode of this env was lost between two take_new calls")
            index_at_take[env] = ep
        taken.append({k: t.cpu().numpy() for k, t in buf.batch(new).items()})
        dicts.append({k: t.cpu().numpy() for k, t in out.items()})
    torch.cuda.synchronize()
    stats = v.get_stats()
    arrays = {k: getattr(buf, k).cpu().numpy() for k in buf.names}
    overflowed = int(buf.overflowed())
    # the env's return statistic counts ONE agent's reward where all agents get the same (shared_reward: the reference's
    # episodeReward += reward[0]); a gymma step's reward is the sum over the agents
    summed = v.n_agents if int(v.env.params.shared_reward) else 1
    v.close()
    return arrays, dicts, taken, stats, overflowed, summed


@pytest.mark.parametrize("selector", ["epsilon_greedy", "soft_policies"])
def test_runner_fills_the_buffer_on_both_paths(selector):
    two, dicts, taken, stats, overflowed, summed = _collect(selector, one_launch=False)
    one, dicts_one, _, stats_one, overflowed_one, _ = _collect(selector, one_launch=True)
    twin = TwinBuffer(64, 2, 20, dicts[0]["obs"].shape[2], dicts[0]["obs"].shape[3], with_prob=selector == "soft_policies")
    for d in dicts:
        assert ("prob" in d) == (selector == "soft_policies")
        twin.append(d)
        twin.take_new()                                              # as _collect did after every call
    for k in twin.names:
        want = np.ascontiguousarray(getattr(twin, k))
        assert np.array_equal(two[k].view(np.uint8), want.view(np.uint8)), ("two-launch path against the twin", k)
        assert np.array_equal(one[k].view(np.uint8), two[k].view(np.uint8)), ("the two paths", k)
    assert stats == stats_one and overflowed == overflowed_one == 0
    length = np.concatenate([t["length"] for t in taken])
    returns = np.concatenate([t["episode_return"] for t in taken])
    assert length.size == stats["episodes"] > 64 and int(length.sum()) == stats["steps"]
    assert 1 <= length.min() and length.max() <= 20
    total = float(returns.astype(np.float64).sum())
    assert summed > 1, "PredatorCapturePrey shares its reward among its agents"
    assert abs(total - summed * stats["return_sum"]) <= 1e-5 * abs(summed * stats["return_sum"]), (total, stats["return_sum"])
    for t in taken:                       # what a learner masks with: the prefix, the end flag on the last step, nothing after
        rows = np.arange(21)[None, :]
        assert np.array_equal(t["filled"][:, :, 0], (rows < t["length"][:, None] + 1).astype(np.int64))
        assert np.array_equal(t["terminated"][:, :, 0], (rows == t["length"][:, None] - 1).astype(np.uint8))
        # (at most 20 binary32 additions, each rounding a partial sum that is no larger than the sum of the magnitudes)
        exact = t["reward"][:, :, 0].astype(np.float64)
        assert (np.abs(exact.sum(1) - t["episode_return"]) <= 20 * 2.0 ** -24 * np.abs(exact).sum(1)).all()
