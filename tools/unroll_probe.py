"""Times BatchedActor.unroll() -- the actor over a whole episode batch in one launch -- against the two ways there were before it.

    python tools/unroll_probe.py [--out profiles/unroll_probe.txt] [--calls 200]

The case: PredatorCapturePrey's shapes (N = 4 agents, D = 16, A = 5 actions, the one-hot agent id appended), hidden size 128,
episodes of rows = 81 time steps (episode_limit 80 + 1), a shared GRU actor packed as two binary16 planes; B = 32 episodes
(EPyMARL's batch size: 4 tiles of 32 rows) and B = 4096 (an on-policy batch: 512 tiles).  obs is episode-major [B, 81, N, D], what
EpisodeBuffer.batch() hands out.  Three things are timed side by side, each as `calls` calls between two device events,
device-complete, in several alternating windows after a warm-up; the median window and the spread (min .. max) are reported:
  unroll     one rg_actor_unroll launch (its Python included), outputs preallocated
  per step   what the fused actor launch offered: a time-major copy of obs (one transposing copy, included), the hidden state zeroed,
             then 81 forward_fused launches on the slices, the hidden state through memory; q and actions stay time-major
  torch      the loop over t of BatchedActor.forward in torch ops (a dozen launches per step), a tenth as many calls per window
Before anything is timed the first two are compared word for word.  Needs the GPU: there is no host path to time."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, D, A, H, ROWS = 4, 16, 5, 128, 81


def _window(fn, calls):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls     # microseconds per call


def make_case(actor, B, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(B)
    obs = torch.rand(B, ROWS, N, D, generator=g, device=dev) * 2 - 1
    q, act = torch.empty(B, ROWS, N, A, device=dev), torch.empty(B, ROWS, N, dtype=torch.int32, device=dev)
    obs_tm, hidden = torch.empty(ROWS, B, N, D, device=dev), torch.empty(B, N, H, device=dev)
    q_tm, act_tm = torch.empty(ROWS, B, N, A, device=dev), torch.empty(ROWS, B, N, dtype=torch.int32, device=dev)
    eye = torch.eye(N, device=dev).unsqueeze(0).expand(B, N, N)

    def unroll():
        actor.unroll(obs, q_out=q, actions_out=act)

    def per_step():
        obs_tm.copy_(obs.transpose(0, 1))
        hidden.zero_()
        for t in range(ROWS):
            actor.forward_fused(obs_tm[t], hidden, q_out=q_tm[t], actions_out=act_tm[t])

    def torch_loop():
        h = actor.init_hidden(B)
        for t in range(ROWS):
            _, h = actor.forward(torch.cat([obs[:, t], eye], dim=2), h)

    unroll()
    per_step()
    torch.cuda.synchronize()
    same = torch.equal(q.view(torch.int32), q_tm.transpose(0, 1).contiguous().view(torch.int32)) and torch.equal(act, act_tm.transpose(0, 1))
    if not same:
        raise SystemExit(f"B = {B}: unroll and the per-step launches differ")
    return unroll, per_step, torch_loop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    import torch
    from gpu_helpers import random_actor
    from marbler_amd.evaluate import BatchedActor
    dev = torch.device("cuda:0")
    actor = BatchedActor(random_actor(1, D + N, H, A, True, seed=0), N, device=dev)
    slow = max(1, args.calls // 10)
    lines = [f"unroll_probe: PredatorCapturePrey shapes (N = {N}, D = {D} + id, A = {A}), hidden {H}, rows = {ROWS}; {args.calls} calls per "
             f"window (torch loop: {slow}), median of {args.windows} alternating windows (min .. max), {torch.cuda.get_device_name(0)}",
             "unroll and the per-step launches agree word for word at both sizes",
             f"{'':<34}{'us / call':>12}{'min':>10}{'max':>10}{'us / step':>11}{'x unroll':>10}"]
    for B in (32, 4096):
        fns = make_case(actor, B, dev)
        for fn, n in zip(fns, (20, 20, 2)):
            _window(fn, n)                      # warm-up
        times = ([], [], [])
        for _ in range(args.windows):           # alternate, so that a clock or a neighbour's load hits all alike
            for ts, fn, n in zip(times, fns, (args.calls, args.calls, slow)):
                ts.append(_window(fn, n))
        med = [sorted(t)[len(t) // 2] for t in times]
        tiles = (B * N + 31) // 32
        lines.append(f"B = {B}: {B * N} rows, {tiles} tiles")
        for name, t, m in zip(("unroll (one launch)", "per step (copy + 81 launches)", "torch forward loop"), times, med):
            lines.append(f"  {name:<32}{m:>12.1f}{min(t):>10.1f}{max(t):>10.1f}{m / ROWS:>11.2f}{m / med[0]:>10.2f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
