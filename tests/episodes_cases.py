"""Streams for the episode-buffer tests, shared by the CPU tier (the twin against expected slots written out by hand) and the GPU
tier (the kernel against the twin): a seeded generator of synthetic streams, and the named edge cases as flag strings.

A stream is BatchedRunner.run(T)'s dict as NumPy arrays: obs [T + 1, E, N, D], actions [T, E, N], reward [T, E], terminated
[T, E], episode_start [T, E], optionally prob [T, E, N]."""
import numpy as np


def synthetic_stream(rng, T, E, N, D, rate, with_prob, restart, first_obs=None):
    """One call's stream: `terminated` is drawn with probability `rate` per (t, e); episode_start is what the runner would
    report -- `restart` [E] (the previous call's last `terminated`; all ones for a fresh runner) at t = 0, terminated[t - 1]
    after it.  first_obs: the previous call's obs[T] (a collector's obs[0] is the observation it stopped at).
    Returns the dict; its terminated[-1] is the next call's `restart`, its obs[-1] the next call's first_obs."""
    obs = rng.standard_normal((T + 1, E, N, D)).astype(np.float32)
    if first_obs is not None:
        obs[0] = first_obs
    term = rng.random((T, E)) < rate
    start = np.empty((T, E), bool)
    start[0] = restart
    start[1:] = term[:-1]
    out = {"obs": obs, "actions": rng.integers(0, 5, (T, E, N)).astype(np.int32),
           "reward": rng.standard_normal((T, E)).astype(np.float32), "terminated": term, "episode_start": start}
    if with_prob:
        out["prob"] = rng.random((T, E, N)).astype(np.float32)
    return out


def synthetic_calls(seed, calls, T, E, N, D, rate, with_prob, attached=True):
    """`calls` consecutive streams of one collector.  attached=False: the buffer joins a collector that is already running (the
    first call reports no start at t = 0)."""
    rng = np.random.default_rng(seed)
    restart, first_obs, out = np.full(E, bool(attached)), None, []
    for _ in range(calls):
        out.append(synthetic_stream(rng, T, E, N, D, rate, with_prob, restart, first_obs))
        restart, first_obs = out[-1]["terminated"][-1], out[-1]["obs"][-1]
    return out


# The named edge cases.  Per call and env a string of flags, a character per time step: 'S' episode_start, 'T' terminated, 'B'
# both, '.' neither.  The data name their source: with g the step's index counted over all calls of the case,
#     obs[t, e, n, d] = 1000 e + g + (n D + d) / 64,   actions[t, e, n] = 100 e + g + n,   reward[t, e] = g (+ 0.5 for env 1),
#     prob[t, e, n] = (g + 1) / 256
# (obs[T] of a call is g = the next call's first step: a collector's stream).
HAND_CASES = {
    # an episode that goes on in the next call; the next one opens in the other slot
    "two_call_carry": dict(R=2, L=5, N=2, D=3, with_prob=False, calls=[["S.."], [".TS"]]),
    # the last-data row comes from obs[T]
    "termination_at_last_step": dict(R=2, L=4, N=1, D=1, with_prob=True, calls=[["S.T"]]),
    # four episodes in one call through ONE slot: the ring wraps three times inside the launch
    "one_slot_four_episodes": dict(R=1, L=3, N=2, D=2, with_prob=False, calls=[["BBSTB"]]),
    # the buffer joins in the middle of an episode: what it sees of it is dropped, the end flag included
    "attach_mid_episode": dict(R=2, L=4, N=1, D=4, with_prob=False, calls=[["..TS."]]),
    # a start while an episode is open: the open one is abandoned and its slot reused
    "abandoned_episode": dict(R=2, L=4, N=3, D=1, with_prob=False, calls=[["S.S.T"]]),
    # a horizon longer than the buffer: force-closed at L, counted, the rest of the episode dropped
    "overflow": dict(R=2, L=2, N=1, D=3, with_prob=False, calls=[["S...S"]]),
    # two envs with different histories in one stream, across two calls
    "two_envs": dict(R=2, L=3, N=2, D=1, with_prob=True, calls=[["S.T", ".S."], ["S..", "..T"]]),
}


def hand_calls(case):
    """The streams of a HAND_CASES entry (a list, one per call)."""
    N, D, out, g0 = case["N"], case["D"], [], 0
    for flags in case["calls"]:
        E, T = len(flags), len(flags[0])
        g = g0 + np.arange(T + 1, dtype=np.float32)
        env = np.arange(E, dtype=np.float32)
        obs = (1000.0 * env[None, :, None, None] + g[:, None, None, None] +
               (np.arange(N * D, dtype=np.float32).reshape(1, 1, N, D) / 64.0)).astype(np.float32)
        batch = {"obs": obs,
                 "actions": (100 * np.arange(E)[None, :, None] + (g0 + np.arange(T))[:, None, None] + np.arange(N)[None, None, :]).astype(np.int32),
                 "reward": (g[:T, None] + 0.5 * (env[None, :] == 1)).astype(np.float32),
                 "terminated": np.array([[f[t] in "TB" for f in flags] for t in range(T)]),
                 "episode_start": np.array([[f[t] in "SB" for f in flags] for t in range(T)])}
        if case["with_prob"]:
            batch["prob"] = np.broadcast_to(((g[:T] + 1.0) / 256.0)[:, None, None], (T, E, N)).astype(np.float32).copy()
        out.append(batch)
        g0 += T
    return out
