"""Times a training pass of the recurrent actor over an episode batch -- TrainableActor forward + backward: torch's GEMMs for what is
batched over all rows, the two GRU scan launches for what is sequential -- against the plain per-step torch loop under autograd
(TrainableActor.forward_reference, EPyMARL's mac.forward(batch, t) for every t) on the same batch in the same run.

    python tools/gru_scan_probe.py [--out profiles/gru_scan_probe.txt] [--calls 10]

The cases: PredatorCapturePrey's shapes (N = 4 agents, D = 16, the one-hot agent id appended, 5 actions), 81 rows (time limit 80 + 1),
shared weights; hidden 128 at B = 32 episodes (EPyMARL's batch size) and B = 4096 (an on-policy batch), hidden 64 at B = 32.  The
observations are uniform random numbers: nothing in either pass depends on the data.  The loss is sum(q c) with a fixed random c, so
that every row sends a gradient back.  Per case three things are timed side by side, each as `calls` calls between two device
events, device-complete, in several alternating windows after a warm-up; the median window and the spread (min .. max) are reported:
  trainable    TrainableActor(obs) -> loss -> backward(): 3 GEMMs + rg_gru_scan_forward, then rg_gru_scan_backward + the gradient GEMMs
  torch loop   forward_reference(obs) -> loss -> backward(): rows x (fc1, GRU cell, fc2) and autograd's replay (the parent of this
               feature has no such call: this is the baseline)
  scan pair    rg_gru_scan_forward + rg_gru_scan_backward alone, outputs preallocated (their Python included)
and the bytes the forward launch saves for the backward launch (h and the gates) are stated.  Needs the GPU: there is no host path."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, D, A, ROWS = 4, 16, 5, 81
CASES = ((128, 32), (128, 4096), (64, 32))          # (hidden, B)


def _window(fn, calls):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls     # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--torch-calls", type=int, default=2)      # (the loop is thousands of launches per call)
    args = ap.parse_args()
    import torch
    from gpu_helpers import random_actor
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.learn import TrainableActor, gru_scan_backward, gru_scan_forward
    dev = torch.device("cuda:0")
    lines = [f"gru_scan_probe: PredatorCapturePrey shapes (N = {N}, D = {D} + {N}, {A} actions), rows = {ROWS}, shared weights, loss sum(q c); "
             f"{args.calls} calls per window ({args.torch_calls} for the torch loop), median of {args.windows} alternating windows (min .. max), "
             f"{torch.cuda.get_device_name(0)}",
             f"{'':<52}{'us / call':>12}{'min':>12}{'max':>12}{'x trainable':>12}"]
    for H, B in CASES:
        actor = TrainableActor.from_actor(BatchedActor(random_actor(1, D + N, H, A, True, seed=1), N, device=dev))
        g = torch.Generator(device=dev).manual_seed(B + H)
        obs = torch.rand(B, ROWS, N, D, device=dev, generator=g) * 2 - 1
        c = torch.randn(B, ROWS, N, A, device=dev, generator=g)
        gi = torch.randn(B, ROWS, N, 3 * H, device=dev, generator=g)
        dh = torch.randn(B, ROWS, N, H, device=dev, generator=g)
        w_hh, b_hh = actor.rnn.weight_hh.detach(), actor.rnn.bias_hh.detach()
        o = dict(h=torch.empty(B, ROWS, N, H, device=dev), gates=torch.empty(B, ROWS, N, 4 * H, device=dev), dgi=torch.empty(B, ROWS, N, 3 * H, device=dev),
                 dghn=torch.empty(B, ROWS, N, H, device=dev), dhid=torch.empty(B, N, H, device=dev))

        def trainable():
            actor.zero_grad(set_to_none=True)
            (actor(obs) * c).sum().backward()

        def loop():
            actor.zero_grad(set_to_none=True)
            (actor.forward_reference(obs) * c).sum().backward()

        def pair():
            gru_scan_forward(gi, w_hh, b_hh, h_out=o["h"], gates_out=o["gates"])
            gru_scan_backward(o["h"], o["gates"], w_hh, dh, dgi_out=o["dgi"], dghn_out=o["dghn"], d_hidden_in_out=o["dhid"])

        def fwd_only():
            gru_scan_forward(gi, w_hh, b_hh, h_out=o["h"], gates_out=o["gates"])

        fns, calls = (trainable, loop, pair, fwd_only), (args.calls, args.torch_calls, args.calls, args.calls)
        for fn, k in zip(fns, calls):
            _window(fn, min(k, 3))                # warm-up
        times = tuple([] for _ in fns)
        for _ in range(args.windows):             # alternate, so that a clock or a neighbour's load hits all alike
            for ts, fn, k in zip(times, fns, calls):
                ts.append(_window(fn, k))
        med = [sorted(t)[len(t) // 2] for t in times]
        saved = (o["h"].numel() + o["gates"].numel()) * 4
        tiles = (B * N + 31) // 32
        lines.append(f"H = {H}, B = {B}: {B * ROWS * N} rows of the GEMMs, {B * N} flat rows = {tiles} tiles of the scan; the forward launch saves "
                     f"{saved / 1e6:.1f} MB (h and the gates) for the backward launch")
        names = ("trainable: TrainableActor forward + backward", "torch loop: forward_reference forward + backward", "scan pair: the two launches alone",
                 "scan forward: the forward launch alone")
        for name, t, md in zip(names, times, med):
            lines.append(f"  {name:<50}{md:>12.1f}{min(t):>12.1f}{max(t):>12.1f}{md / med[0]:>12.2f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
