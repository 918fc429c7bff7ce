"""Times EpisodeBuffer.append() against the floor it cannot beat and against what a user would write without it.

    python tools/episodes_probe.py [--out profiles/episodes_probe.txt] [--launches 200]

The case: PredatorCapturePrey 4096 x 4 (N D = 64 floats a row), T = 64 time steps a call, episode_limit L = 81, R = 2 slots per
env, no `prob`.  The stream is synthetic and repeats without contradiction, so that every timed launch does the same work:
every env starts an episode at t = 0 and ends one at t = 63, and a quarter of the envs end one more somewhere in between (1.25
episodes per env and call; a collector with an 80-step limit finishes 0.8).  Three things are timed side by side, each as
`launches` calls between two device events, device-complete, the median of several alternating windows after a warm-up:
  append   one rg_episodes_append launch through EpisodeBuffer.append (its Python included)
  floor    torch's copy_ of a contiguous buffer of as many bytes as append reads plus writes (half of them read, half written;
           counted from the flags: obs, action, reward and flag rows of the stream in, the same rows of the slots out)
  torch    the composition in torch ops: a loop over t with indexed copies into the slots -- a dozen launches per time step,
           without what append does on top (no zeroing of a reopened slot, no abandoned or overflowing episodes)
Needs the GPU: there is no host path to time."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E, N, D, A, T, L, R = 4096, 4, 16, 5, 64, 81, 2


def _window(fn, launches):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / launches     # microseconds per call


def make_stream(dev):
    import torch
    g = torch.Generator().manual_seed(0)
    term = torch.zeros(T, E, dtype=torch.bool)
    term[T - 1] = True
    extra = torch.nonzero(torch.rand(E, generator=g) < 0.25).flatten()
    term[torch.randint(0, T - 1, (extra.numel(),), generator=g), extra] = True
    start = torch.zeros(T, E, dtype=torch.bool)
    start[0] = True
    start[1:] = term[:-1]
    batch = {"obs": torch.randn(T + 1, E, N, D, generator=g), "actions": torch.randint(0, A, (T, E, N), generator=g, dtype=torch.int32),
             "reward": torch.randn(T, E, generator=g), "terminated": term, "episode_start": start}
    return {k: v.to(dev) for k, v in batch.items()}, int(term.sum())


def torch_composition(batch, slots):
    """The loop a user would write: per time step, indexed copies of the step's rows into each env's current slot row."""
    import torch
    obs, actions, reward, terminated, filled = slots
    dev = obs.device
    env = torch.arange(E, device=dev)
    ring = torch.zeros(E, dtype=torch.int64, device=dev)
    pos = torch.zeros(E, dtype=torch.int64, device=dev)

    def run():
        ring.zero_()
        pos.zero_()
        for t in range(T):
            start, term = batch["episode_start"][t], batch["terminated"][t]
            ring.copy_(torch.where(start, (ring + 1) % R, ring))
            pos.masked_fill_(start, 0)
            s = env * R + ring
            obs[s, pos] = batch["obs"][t]
            actions[s, pos] = batch["actions"][t]
            reward[s, pos] = batch["reward"][t]
            terminated[s, pos] = term.to(torch.uint8)
            filled[s, pos] = 1
            pos.add_(1)
            obs[s, pos] = torch.where(term[:, None, None], batch["obs"][t + 1], obs[s, pos])      # the last-data row
            filled[s, pos] = torch.maximum(filled[s, pos], term.to(torch.uint8))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    import torch
    from marbler_amd.episodes import EpisodeBuffer
    dev = torch.device("cuda:0")
    batch, closes = make_stream(dev)
    buf = EpisodeBuffer(E, N, D, A, L, slots_per_env=R, device=dev)
    steps = T * E
    rows = steps + closes                                             # obs rows moved: a transition each, a last-data row per end
    read = rows * N * D * 4 + steps * N * 4 + steps * (4 + 1 + 1)     # obs, actions, reward + the two flags
    written = rows * N * D * 4 + steps * N * 4 + steps * (4 + 1 + 1) + closes   # the same rows of the slots + filled of the last-data rows
    src = torch.empty((read + written) // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    other = EpisodeBuffer(E, N, D, A, L, slots_per_env=R, device=dev)
    composed = torch_composition(batch, (other.obs, other.actions, other.reward, other.terminated, other.filled))
    append = lambda: buf.append(batch)      # noqa: E731
    floor = lambda: dst.copy_(src)          # noqa: E731
    for fn in (append, floor):
        _window(fn, 20)                     # warm-up
    _window(composed, 2)
    assert int(buf.overflowed()) == 0 and int(buf.complete.sum()) == E * R        # the stream repeats: no episode is cut
    ta, tf, tc = [], [], []
    for _ in range(args.windows):           # alternate, so that a clock or a neighbour's load hits all alike
        ta.append(_window(append, args.launches))
        tf.append(_window(floor, args.launches))
        tc.append(_window(composed, max(1, args.launches // 50)))
    a, f, c = (sorted(t)[len(t) // 2] for t in (ta, tf, tc))
    nbytes = read + written
    lines = [f"episodes_probe: PredatorCapturePrey {E} x {N} (row {N * D} floats), T = {T}, L = {L}, R = {R}; {args.launches} launches "
             f"per window, median of {args.windows} windows, {torch.cuda.get_device_name(0)}",
             f"bytes per call: {read} read + {written} written = {nbytes / 1e6:.1f} MB ({closes / E:.2f} episodes end per env and call)",
             f"{'':<28}{'us / call':>12}{'GB/s':>9}{'x floor':>9}",
             f"{'append (one launch)':<28}{a:>12.1f}{nbytes / a / 1e3:>9.0f}{a / f:>9.2f}",
             f"{'floor (torch copy_)':<28}{f:>12.1f}{nbytes / f / 1e3:>9.0f}{1.0:>9.2f}",
             f"{'torch loop over t':<28}{c:>12.1f}{nbytes / c / 1e3:>9.0f}{c / f:>9.2f}"]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
