"""The summation order of td_qmix_kernel (csrc/td_targets.h) in NumPy, on the CPU: float32 fmaf chains in the kernel's own order,
with the k steps of every 32 x 32 block dealt out over `chains` accumulators that are added at the end.  Prints, per shape, the
error max / mean / percentiles of |y - y64| / (1 + |y64|) over random rows for torch's float32 QMixer on the CPU and for 1, 2 and
4 chains: what the choice of two chains in DESIGN.md section 4 "TD targets" rests on.

    python tools/td_targets_order.py [--rows 4000]

(An fmaf is emulated as a float64 product and sum rounded to float32: the product of two float32 is exact in float64.)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
f32 = np.float32


def chain(a, b, chains):
    """a [R, K] . b [K, C] as float32 fmaf chains; k step k // 2 (the matrix instruction takes two k at a time) goes to chain
    (k // 2) % chains; the chains are added in order."""
    accs = [np.zeros((a.shape[0], b.shape[1]), f32) for _ in range(chains)]
    for k in range(a.shape[1]):
        p = (k // 2) % chains
        accs[p] = (accs[p].astype(np.float64) + a[:, k:k + 1].astype(np.float64) * b[k:k + 1].astype(np.float64)).astype(f32)
    out = accs[0]
    for x in accs[1:]:
        out = (out + x).astype(f32)
    return out


def kernel_order(p, aq, s, chains):
    """y [R] of td_qmix_kernel for agent_q [R, N] and state [R, S] (float32), p: the QMixer state dict as NumPy arrays."""
    relu = lambda x: np.maximum(x, f32(0))  # noqa: E731
    first = lambda k: chain(s, p[k + ".weight"].T.astype(f32), chains) + p[k + ".bias"].astype(f32)  # noqa: E731
    second = lambda h, k: chain(h, p[k + ".weight"].T.astype(f32), chains) + p[k + ".bias"].astype(f32)  # noqa: E731
    R, N = aq.shape
    w1 = np.abs(second(relu(first("hyper_w_1.0")), "hyper_w_1.2")).reshape(R, N, 32)
    wf = np.abs(second(relu(first("hyper_w_final.0")), "hyper_w_final.2"))
    hv, b1 = relu(first("V.0")), first("hyper_b_1")
    part = [np.zeros((R, 32), f32) for _ in range(3)]            # wavefront w folds agents w, w + 3, ...
    for n in range(N):
        part[n % 3] = (part[n % 3] + (aq[:, n:n + 1] * w1[:, n]).astype(f32)).astype(f32)
    h = (((part[0] + part[1]).astype(f32) + part[2]).astype(f32) + b1).astype(f32)
    h = np.where(h > 0, h, np.expm1(np.minimum(h, 0).astype(np.float64)).astype(f32))
    sv = ((h * wf).astype(f32) + (p["V.2.weight"][0].astype(f32) * hv).astype(f32)).astype(f32)
    d = 16
    while d >= 1:                                                 # the butterfly over the 32 columns
        sv = (sv + sv[:, np.arange(32) ^ d]).astype(f32)
        d >>= 1
    return (sv[:, 0] + p["V.2.bias"][0].astype(f32)).astype(f32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4000)
    args = ap.parse_args()
    import torch
    import td_targets_twin as tw
    from marbler_amd.targets import TargetMixer
    for N, S, scale in ((2, 2, 1.0), (5, 45, 1.0), (5, 45, 4.0), (4, 64, 1.0), (8, 144, 1.0)):
        rng = np.random.default_rng(1)
        p = {k: (v * scale).numpy() for k, v in TargetMixer("qmix", N, S, device="cpu", seed=3).state_dict().items()}
        aq = rng.standard_normal((args.rows, N)).astype(f32)
        s = (rng.random((args.rows, S)) * 2 - 1).astype(f32)
        y64 = tw.qmix64(p, aq.astype(np.float64), s.astype(np.float64))
        yt = tw.qmixer_torch({k: torch.from_numpy(v) for k, v in p.items()}, torch.from_numpy(aq)[None], torch.from_numpy(s)[None])[0, :, 0].numpy()

        def stats(y):
            e = np.abs(y.astype(np.float64) - y64) / (1 + np.abs(y64))
            return "mean %.2e  p50 %.2e  p90 %.2e  p99 %.2e  max %.2e" % (e.mean(), np.median(e), np.quantile(e, .9), np.quantile(e, .99), e.max())
        print(f"N {N} S {S:>3} weights x{scale:g}  torch f32 (cpu): {stats(yt)}")
        for chains in (1, 2, 4):
            print(f"N {N} S {S:>3} weights x{scale:g}  kernel, {chains} chain{'s' if chains > 1 else ' '}: {stats(kernel_order(p, aq, s, chains))}")


if __name__ == "__main__":
    main()
