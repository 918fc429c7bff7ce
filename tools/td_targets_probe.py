"""Times td_targets() -- the target mixer and the double-Q TD targets of an episode batch in one launch -- against the torch
composition it replaces, and measures the qmix error of both against float64.

    python tools/td_targets_probe.py [--out profiles/td_targets_probe.txt] [--calls 200]

The case: PredatorCapturePrey's shapes (N = 4 agents, D = 16, S = 64, A = 5 actions), episodes of rows = 81 time steps (episode_limit
80 + 1); B = 32 episodes (EPyMARL's batch size) and B = 4096 (an on-policy batch).  The episodes are COLLECTED: a BatchedRunner with
a random GRU actor fills an EpisodeBuffer whose slots are 4 rows longer than the env's time limit, so the batch has the lengths,
terminations and padding a learner sees; qt is a second random actor's unroll, sel the collecting actor's greedy actions.  Two things
are timed side by side per mixer (vdn, qmix), each as `calls` calls between two device events, device-complete, in several
alternating windows after a warm-up; the median window and the spread (min .. max) are reported:
  td_targets   one rg_td_targets launch (its Python included), outputs preallocated
  torch        tests/td_targets_twin.py restatement(): q_learner.train's target lines and QMixer.forward in torch float32 ops on the
               same batch (the parent of this launch has no such call: this is the baseline)
For qmix the launch's share of the chip's f32 rate is what the rule needs -- S 192 + 64 N 32 + 64 32 + N 32 + 64 multiply-adds per
LIVE row -- over the call time and the 157.3 TFLOP/s peak (it is compute-bound by that count: a live row reads 64 floats of state
and a few flags).  The second table is the qmix error max |x - twin64| / (1 + |twin64|) over the unmasked rows for both, with
torch's default initialisation and with the weights x 4, per case of tests/test_gpu_td_targets.py and on the collected batch.
Needs the GPU: there is no host path to time."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, D, A, H, LIMIT, PAD = 4, 16, 5, 64, 80, 4
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
    """-> the batch of B collected episodes: qt, sel, obs, reward, terminated, filled, each [B, LIMIT + 1 + PAD, ...]."""
    import torch
    from gpu_helpers import random_actor
    from marbler_amd.episodes import EpisodeBuffer
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    v = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", B, time_limit=LIMIT, seed=B)
    assert (v.n_agents, v.obs_size, v.n_actions) == (N, D, A), (v.n_agents, v.obs_size, v.n_actions)
    online, target = (BatchedActor(random_actor(1, D + N, H, A, True, seed=s), N, device=dev) for s in (1, 2))
    runner = BatchedRunner(v, online, epsilon=0.05, seed=3)
    buf = EpisodeBuffer(B, N, D, A, LIMIT + PAD, device=dev)
    runner.run(2 * LIMIT + 2, one_launch=True, into=buf)
    slots = buf.take_new()[:B]
    assert int(slots.numel()) == B, f"only {int(slots.numel())} of {B} episodes completed"
    obs = buf.obs[slots]
    qt, _ = target.unroll(obs)
    _, sel = online.unroll(obs)
    out = dict(qt=qt, sel=sel, obs=obs, reward=buf.reward[slots], terminated=buf.terminated[slots], filled=buf.filled[slots],
               length=buf.length[slots])
    torch.cuda.synchronize()
    v.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    import torch
    import td_targets_twin as tw
    from marbler_amd.targets import TargetMixer, td_targets
    dev = torch.device("cuda:0")
    rows = LIMIT + 1 + PAD
    lines = [f"td_targets_probe: PredatorCapturePrey shapes (N = {N}, D = {D}, S = {N * D}, A = {A}), collected episodes in slots of rows = {rows} "
             f"(time limit {LIMIT}); {args.calls} calls per window, median of {args.windows} alternating windows (min .. max), "
             f"{torch.cuda.get_device_name(0)}",
             f"{'':<40}{'us / call':>12}{'min':>10}{'max':>10}{'x launch':>10}"]
    errs = []
    for B in (32, 4096):
        c = collect(B, dev)
        host = {k: v.cpu().numpy() for k, v in c.items()}
        mask, live = tw.row_flags(host["terminated"], host["filled"], rows)
        lines.append(f"B = {B}: {B * (rows - 1)} rows in {(B * (rows - 1) + 31) // 32} tiles; {int(mask.sum())} unmasked, {int(live.sum())} live; episode "
                     f"lengths {int(host['length'].min())} .. {int(host['length'].max())}, mean {float(host['length'].mean()):.1f}")
        for kind in ("vdn", "qmix"):
            mixer = TargetMixer(kind, N, N * D, device=dev, seed=5)
            outs = dict(targets_out=torch.empty(B, rows - 1, device=dev), mask_out=torch.empty(B, rows - 1, device=dev),
                        agent_q_out=torch.empty(B, rows - 1, N, device=dev))

            def launch():
                td_targets(c["qt"], c["obs"], c["reward"], c["terminated"], c["filled"], mixer, 0.99, sel=c["sel"], **outs)

            def torch_lines():
                tw.restatement(kind, c["qt"], c["sel"], c["obs"], c["reward"], c["terminated"], c["filled"], 0.99, mixer.params)

            fns = (launch, torch_lines)
            for fn in fns:
                _window(fn, 20)                 # warm-up
            times = ([], [])
            for _ in range(args.windows):       # alternate, so that a clock or a neighbour's load hits both alike
                for ts, fn in zip(times, fns):
                    ts.append(_window(fn, args.calls))
            med = [sorted(t)[len(t) // 2] for t in times]
            for name, t, m in zip((f"{kind}: td_targets (one launch)", f"{kind}: torch restatement"), times, med):
                lines.append(f"  {name:<38}{m:>12.1f}{min(t):>10.1f}{max(t):>10.1f}{m / med[0]:>10.2f}")
            if kind == "qmix":
                macs = N * D * 192 + 64 * N * 32 + 64 * 32 + N * 32 + 64
                flops = 2.0 * macs * int(live.sum())
                lines.append(f"  qmix: {macs} multiply-adds per live row, {flops / 1e9:.2f} GFLOP per call: {flops / med[0] / 1e6:.2f} TFLOP/s = "
                             f"{100 * flops / (med[0] * 1e-6) / PEAK_F32:.2f} % of the f32 rate ({PEAK_F32 / 1e12:.1f} TFLOP/s); compute-bound by count")
                for scale in (1.0, 4.0):        # the error of both against float64 on this batch
                    mx = TargetMixer(kind, N, N * D, device=dev, seed=5)
                    mx.load_state_dict({k: v * scale for k, v in mx.state_dict().items()})
                    got = td_targets(c["qt"], c["obs"], c["reward"], c["terminated"], c["filled"], mx, 0.99, sel=c["sel"])["targets"].cpu().numpy()
                    ref, _ = tw.restatement(kind, c["qt"], c["sel"], c["obs"], c["reward"], c["terminated"], c["filled"], 0.99, mx.params)
                    t64, _, _ = tw.twin(kind, host["qt"], host["sel"], host["obs"], host["reward"], host["terminated"], host["filled"], 0.99,
                                        {k: v.cpu().numpy() for k, v in mx.params.items()})
                    errs.append(f"  collected batch B = {B:<5} weights x{scale:g}: {int(live.sum()):>7} live rows   kernel {tw.rel_err(got, t64, live):.3e}   "
                                f"torch {tw.rel_err(ref[..., 0].cpu().numpy(), t64, live):.3e}")
    # the cases of the GPU tests
    import td_targets_harness as cases
    for i, case in enumerate(cases.CASES):
        if case[0] != "qmix":
            continue
        kind, B, rws, n, d, a, extra, with_sel = case
        for scale in (1.0, 4.0):
            b = cases.Batch(kind, B, rws, n, d, a, extra, with_sel, seed=i)
            mixer = cases.make_mixer(kind, n, n * d, scale, seed=i)
            out = b.run(mixer, 0.99)
            t64, _, _ = b.twin(0.99, mixer.params)
            ref, _ = b.restatement(0.99, mixer.params)
            errs.append(f"  case {i:>2} B {B:>2} rows {rws:>2} N {n} S {n * d:>3} A {a:>2} weights x{scale:g}: {int(b.live.sum()):>4} live rows   "
                        f"kernel {tw.rel_err(out['targets'], t64, b.live):.3e}   torch {tw.rel_err(ref, t64, b.live):.3e}")
    lines.append("qmix error max |x - twin64| / (1 + |twin64|) over the live rows, the launch and the torch float32 restatement on the device:")
    text = "\n".join(lines + errs) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
