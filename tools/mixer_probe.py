"""What the trainable mixer costs, and what the torch composition it replaces costs (-> profiles/mixer_probe.txt).

    python tools/mixer_probe.py [--out profiles/mixer_probe.txt]

PredatorCapturePrey's shapes (N = 4, D = 16, A = 5, slots of 85 rows), qmix and vdn, B = 32 and B = 4096.  Device events around
10 calls, the median of 5 alternating windows with min-max (as tools/gru_scan_probe.py).  Rows: TrainableMixer forward + backward
against forward_reference forward + backward under autograd on the same batch in the same run (the baseline: the parent commit
has no such call); the two launches alone; the weight-gradient GEMMs alone (with the masked copy of the state they read); the
re-pack of the parameters into the launch's operands (once per forward); and the bytes of the per-row arrays."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
N, D, A, ROWS = 4, 16, 5, 85
CALLS, WINDOWS = 10, 5


def window(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(CALLS):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / CALLS        # us per call


def measure(fns):
    """{name: fn} -> {name: (median, min, max)} us, the windows of the candidates alternating."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    seen = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, fn in fns.items():
            seen[k].append(window(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in seen.items()}


def batch(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, ROWS, N, A, generator=g).to(DEV)
    actions = torch.randint(0, A, (B, ROWS, N), generator=g, dtype=torch.int32).to(DEV)
    obs = (torch.rand(B, ROWS, N, D, generator=g) * 2 - 1).to(DEV)
    length = torch.randint(1, ROWS, (B,), generator=g)
    mask = (torch.arange(ROWS - 1)[None, :] < length[:, None]).float().to(DEV)     # episodes of a random length: the padding is masked
    return q, actions, obs, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from marbler_amd.mixers import MixerFn, TrainableMixer, mixer_backward, mixer_forward
    lines = [f"# tools/mixer_probe.py on {torch.cuda.get_device_name(0)}: N = {N}, D = {D}, A = {A}, {ROWS} rows; us per call, median of "
             f"{WINDOWS} windows of {CALLS} calls (min - max)"]
    for kind in ("qmix", "vdn"):
        for B in (32, 4096):
            q, actions, obs, mask = batch(B)
            torch.manual_seed(1)
            mixer = TrainableMixer(kind, N, N * D, device=DEV)
            d_mixed = torch.randn(B, ROWS - 1, device=DEV)
            qg = q.clone().requires_grad_(True)

            def ours():
                y = mixer(qg, actions, obs, mask)
                y.backward(d_mixed)

            def torchs():
                y = mixer.forward_reference(qg, actions, obs, mask)
                y.backward(d_mixed)

            ops = mixer.operands(torch.device(DEV))
            p = dict(mixer.named_parameters())
            w1b = p["hyper_w_1.2.weight"].detach() if kind == "qmix" else None
            wfb = p["hyper_w_final.2.weight"].detach() if kind == "qmix" else None
            mixed = mixer_forward(q, actions, obs, mask, ops)
            outs = mixer_backward(q, actions, obs, mask, d_mixed, ops, w1b, wfb)
            fns = {"TrainableMixer fwd + bwd": ours, "forward_reference fwd + bwd (torch autograd)": torchs,
                   "rg_mixer_forward alone": lambda: mixer_forward(q, actions, obs, mask, ops, mixed_out=mixed),
                   "rg_mixer_backward alone": lambda: mixer_backward(q, actions, obs, mask, d_mixed, ops, w1b, wfb, *outs)}
            if kind == "qmix":
                params = [v.detach() for v in mixer._params()]

                class Ctx(object):
                    saved_tensors = (q, actions, obs, mask) + tuple(params)
                    operands, version = ops, ops.version
                real = sys.modules["marbler_amd.mixers"].mixer_backward

                def gemms():                                  # MixerFn.backward with the launch taken out: the GEMMs and their copies
                    sys.modules["marbler_amd.mixers"].mixer_backward = lambda *a, **k: outs
                    try:
                        MixerFn.backward(Ctx, d_mixed)
                    finally:
                        sys.modules["marbler_amd.mixers"].mixer_backward = real
                gemms()
                fns["weight-gradient GEMMs alone (torch)"] = gemms
                fns["operand re-pack (14 copies, once per forward)"] = lambda: mixer.operands(torch.device(DEV))
            res = measure(fns)
            lines.append(f"\n{kind}, B = {B} ({B * (ROWS - 1)} flat rows, {int(mask.sum())} live)")
            for k, (med, lo, hi) in res.items():
                lines.append(f"  {k:52s} {med:10.1f}  ({lo:.1f} - {hi:.1f})")
            a, b = res["TrainableMixer fwd + bwd"][0], res["forward_reference fwd + bwd (torch autograd)"][0]
            lines.append(f"  torch / TrainableMixer: {b / a:.2f} x")
            if kind == "qmix":
                per_row = 4 * (192 + 32 * N + 32 + 160)
                lines.append(f"  per-row arrays: {per_row} bytes per flat row, {per_row * B * ROWS / 2 ** 20:.1f} MiB for this batch (d_pre, d_p2, g)")
            y1 = mixer(qg, actions, obs, mask).detach()
            y2 = mixer.forward_reference(qg, actions, obs, mask).detach()
            lines.append(f"  max |TrainableMixer - forward_reference| of mixed: {float((y1 - y2).abs().max()):.3e}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
