"""Times nstep_returns() -- the target critic over an episode batch and MAPPO's n-step returns in one launch -- against the torch
composition it replaces and against a plain copy of the bytes it reads, and measures the error of the values of both against float64.

    python tools/nstep_returns_probe.py [--out profiles/nstep_returns_probe.txt] [--calls 50]

The case: PredatorCapturePrey's shapes (N = 4 agents, D = 16, S = 64), hidden 128, n = 10, add_value_last_step, gamma 0.99; episodes
in slots of rows = 85 (time limit 80 + 1 + 4 rows of padding); B = 32 episodes (EPyMARL's batch size) and B = 4096 (an on-policy
batch).  The episodes are COLLECTED: a soft-policy BatchedRunner with a random GRU actor fills an EpisodeBuffer, so the batch has the
lengths, terminations and padding a learner sees.  Per critic kind (cv, cv_ns) three things are timed side by side, each as `calls`
calls between two device events, device-complete, in several alternating windows after a warm-up; the median window and the spread
(min .. max) are reported:
  nstep_returns   one rg_nstep_returns launch (its Python included), outputs preallocated
  torch           tests/nstep_returns_twin.py restatement(): TargetCritic.forward over every row and EPyMARL's nstep_returns double
                  loop in torch float32 ops on the same batch (the parent of this launch has no such call: this is the baseline)
  copy            obs, reward, terminated and filled copied once into preallocated tensors: the bytes the launch reads, for scale
The launch's share of the chip's f32 rate is what the rule needs -- S H + H H + H multiply-adds per needed (row, agent) pair for cv_ns,
S H / N + H H + H for cv -- over the call time and the 157.3 TFLOP/s peak.  The second table is the error of the values
max |x - v64| / (1 + |v64|) over the needed rows for both, with torch's default initialisation and with the weights x 4, per case of
tests/test_gpu_nstep_returns.py and on the collected batch.  Needs the GPU: there is no host path to time."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, D, A, H, LIMIT, PAD, NSTEP, GAMMA = 4, 16, 5, 128, 80, 4, 10, 0.99
PEAK_F32 = 157.3e12


def _window(fn, calls):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls     # microseconds per call


def collect(B, dev):
    """-> the batch of B collected episodes: obs, reward, terminated, filled, each [B, LIMIT + 1 + PAD, ...], and length."""
    import torch
    from gpu_helpers import random_actor
    from marbler_amd.episodes import EpisodeBuffer
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    v = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", B, time_limit=LIMIT, seed=B)
    assert (v.n_agents, v.obs_size, v.n_actions) == (N, D, A), (v.n_agents, v.obs_size, v.n_actions)
    actor = BatchedActor(random_actor(1, D + N, 64, A, True, seed=1), N, device=dev)
    runner = BatchedRunner(v, actor, epsilon=0.0, seed=3, action_selector="soft_policies")
    buf = EpisodeBuffer(B, N, D, A, LIMIT + PAD, with_prob=True, device=dev)
    runner.run(2 * LIMIT + 2, one_launch=True, into=buf)
    slots = buf.take_new()[:B]
    assert int(slots.numel()) == B, f"only {int(slots.numel())} of {B} episodes completed"
    out = dict(obs=buf.obs[slots], reward=buf.reward[slots], terminated=buf.terminated[slots], filled=buf.filled[slots], length=buf.length[slots])
    torch.cuda.synchronize()
    v.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--torch-calls", type=int, default=3)      # (the double loop is thousands of launches per call)
    args = ap.parse_args()
    import torch
    import nstep_returns_twin as tw
    from marbler_amd.returns import TargetCritic, nstep_returns
    dev = torch.device("cuda:0")
    rows = LIMIT + 1 + PAD
    lines = [f"nstep_returns_probe: PredatorCapturePrey shapes (N = {N}, D = {D}, S = {N * D}), hidden {H}, n = {NSTEP}, add_value_last_step, "
             f"collected episodes in slots of rows = {rows} (time limit {LIMIT}); {args.calls} calls per window ({args.torch_calls} for torch), "
             f"median of {args.windows} alternating windows (min .. max), {torch.cuda.get_device_name(0)}",
             f"{'':<44}{'us / call':>12}{'min':>12}{'max':>12}{'x launch':>10}"]
    errs = []
    for B in (32, 4096):
        c = collect(B, dev)
        host = {k: v.cpu().numpy() for k, v in c.items()}
        m = tw.mask_of(host["terminated"], host["filled"], rows)
        need = tw.needed_rows(m, True)
        read = sum(c[k].numel() * c[k].element_size() for k in ("obs", "reward", "terminated", "filled"))
        lines.append(f"B = {B}: {B * rows} rows; {int(m.sum())} unmasked, {int(need.sum())} needed; episode lengths {int(host['length'].min())} .. "
                     f"{int(host['length'].max())}, mean {float(host['length'].mean()):.1f}; {read / 1e6:.2f} MB of inputs")
        copies = {k: torch.empty_like(c[k]) for k in ("obs", "reward", "terminated", "filled")}
        for kind in ("cv", "cv_ns"):
            critic = TargetCritic(kind, N, N * D, H, device=dev, seed=5)
            outs = dict(returns_out=torch.empty(B, rows - 1, N, device=dev), values_out=torch.empty(B, rows, N, device=dev),
                        mask_out=torch.empty(B, rows - 1, device=dev))

            def launch():
                nstep_returns(c["obs"], c["reward"], c["terminated"], c["filled"], critic, GAMMA, NSTEP, True, **outs)

            def torch_lines():
                tw.restatement(critic.forward, c["obs"], c["reward"], c["terminated"], c["filled"], GAMMA, NSTEP, True)

            def copy():
                for k, dst in copies.items():
                    dst.copy_(c[k])

            fns, calls = (launch, torch_lines, copy), (args.calls, args.torch_calls, args.calls)
            for fn, k in zip(fns, calls):
                _window(fn, min(k, 5))            # warm-up
            times = ([], [], [])
            for _ in range(args.windows):         # alternate, so that a clock or a neighbour's load hits all alike
                for ts, fn, k in zip(times, fns, calls):
                    ts.append(_window(fn, k))
            med = [sorted(t)[len(t) // 2] for t in times]
            names = (f"{kind}: nstep_returns (one launch)", f"{kind}: torch restatement (critic + double loop)", f"{kind}: copy of the inputs")
            for name, t, md in zip(names, times, med):
                lines.append(f"  {name:<42}{md:>12.1f}{min(t):>12.1f}{max(t):>12.1f}{md / med[0]:>10.2f}")
            pairs = int(need.sum()) * N
            macs = (N * D * H + H * H + H) if kind == "cv_ns" else (N * D * H / N + H * H + H)
            flops = 2.0 * macs * pairs
            lines.append(f"  {kind}: {macs:.0f} multiply-adds per needed (row, agent) pair, {flops / 1e9:.2f} GFLOP per call: {flops / med[0] / 1e6:.2f} "
                         f"TFLOP/s = {100 * flops / (med[0] * 1e-6) / PEAK_F32:.2f} % of the f32 rate ({PEAK_F32 / 1e12:.1f} TFLOP/s)")
            for scale in (1.0, 4.0):              # the error of both against float64 on this batch
                cr = TargetCritic(kind, N, N * D, H, device=dev, seed=5)
                cr.load_state_dict({k: v * scale for k, v in cr.state_dict().items()})
                got = nstep_returns(c["obs"], c["reward"], c["terminated"], c["filled"], cr, GAMMA, NSTEP, True)["values"].cpu().numpy()
                ref = cr.forward(c["obs"].reshape(B, rows, N * D)).cpu().numpy()
                v64, _ = tw.values64(kind, {k: v.cpu().numpy() for k, v in cr.params.items()}, host["obs"], host["terminated"], host["filled"], True)
                errs.append(f"  collected batch B = {B:<5} {kind:<6} weights x{scale:g}: {int(need.sum()):>7} needed rows   kernel {tw.rel_err(got, v64, need):.3e}   "
                            f"torch {tw.rel_err(ref, v64, need):.3e}")
    # the cases of the GPU tests
    import nstep_returns_harness as cases
    for i, case in enumerate(cases.CASES):
        kind, h, B, rws, n_agents, d, n, add, (scale, shift), extra = case
        for wscale in (1.0, 4.0):
            b = cases.Batch(B, rws, n_agents, d, add, extra, seed=i)
            critic = cases.make_critic(kind, n_agents, n_agents * d, h, wscale, seed=i)
            out = b.run(critic, GAMMA, n, scale, shift)
            v64, ref = b.values64(critic, scale, shift), b.torch_values(critic, scale, shift)
            errs.append(f"  case {i:>2} {kind:<6} H {h:>3} B {B:>2} rows {rws:>3} N {n_agents} S {n_agents * d:>3} weights x{wscale:g}: {int(b.need.sum()):>4} needed rows   "
                        f"kernel {tw.rel_err(out['values'], v64, b.need):.3e}   torch {tw.rel_err(ref, v64, b.need):.3e}")
    lines.append("error of the values, max |x - v64| / (1 + |v64|) over the needed rows, the launch and the torch float32 restatement on the device:")
    text = "\n".join(lines + errs) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
