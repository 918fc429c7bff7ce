"""Timing of the actor launches and the one-launch policy rollout, for the table in DESIGN.md section "soft policies":

    python tools/soft_policy_timing.py --out profiles/soft_policy_timing.jsonl [--package-root DIR] [--tag NAME]

One process measures one build: the package under --package-root (default: this tree).  To compare two builds, run the script
alternately on each (A B A B ...) in one session and compare the medians and the run-to-run spread of the same build.  Each
figure is device-event time over a window of launches on seeded inputs, after a warm-up of the same shape; microseconds per launch
(the rollout: per launch of T = 64 steps).  Entries a build does not have (the sampled launches on an older build) are left out."""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--rollout-iters", type=int, default=20)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    assert os.path.abspath(sys.modules["marbler_amd"].__file__).startswith(os.path.abspath(args.package_root))
    dev, E, N, D, A, T = "cuda:0", args.envs, 4, 16, 5, 64

    def random_sd(H, seed=3):
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * 0.3  # noqa: E731
        return {"fc1.weight": r(H, D + N), "fc1.bias": r(H), "rnn.weight_ih": r(3 * H, H), "rnn.weight_hh": r(3 * H, H),
                "rnn.bias_ih": r(3 * H), "rnn.bias_hh": r(3 * H), "fc2.weight": r(A, H) * 8, "fc2.bias": r(A)}

    def timed(fn, iters):
        for _ in range(max(iters // 10, 3)):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0 / iters

    res = {"tag": args.tag, "envs": E, "agents": N, "T": T}
    g = torch.Generator(device=dev).manual_seed(1)
    for H in (128, 64):
        actor = BatchedActor(random_sd(H), N, device=dev)
        obs = torch.rand(E, N, D, generator=g, device=dev) * 2 - 1
        hidden = torch.rand(E, N, H, generator=g, device=dev) * 2 - 1
        u = torch.rand(E, N, generator=g, device=dev)
        q = torch.empty(E, N, A, device=dev)
        act = torch.empty(E, N, dtype=torch.int32, device=dev)
        prob = torch.empty(E, N, device=dev)
        res[f"actor_greedy_h{H}_us"] = timed(lambda: actor.forward_fused(obs, hidden, q_out=q, actions_out=act), args.iters)
        res[f"actor_epsilon_h{H}_us"] = timed(lambda: actor.forward_fused(obs, hidden, q_out=q, actions_out=act, explore_u=u, epsilon=0.1), args.iters)
        try:
            res[f"actor_sampled_h{H}_us"] = timed(lambda: actor.forward_fused(obs, hidden, q_out=q, actions_out=act, sample_u=u, prob_out=prob), args.iters)
        except TypeError:
            pass

        def torch_alternative():   # the greedy launch, then softmax + multinomial + gather on its q
            actor.forward_fused(obs, hidden, q_out=q, actions_out=act)
            p = torch.softmax(q.view(E * N, A), dim=1)
            a_ = torch.multinomial(p, 1)
            return a_, p.gather(1, a_)
        res[f"actor_greedy_plus_torch_sampling_h{H}_us"] = timed(torch_alternative, args.iters // 4)
        for selector in ("greedy", "epsilon", "sampled"):
            v = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", E, time_limit=200, seed=5)
            try:
                kw = {"greedy": {}, "epsilon": {"epsilon": 0.1}, "sampled": {"action_selector": "soft_policies"}}[selector]
                runner = BatchedRunner(v, actor, seed=9, **kw)
            except TypeError:
                continue
            res[f"rollout_T{T}_{selector}_h{H}_us"] = timed(lambda: runner.run(T, one_launch=True), args.rollout_iters)
            res[f"two_launch_T{T}_{selector}_h{H}_us"] = timed(lambda: runner.run(T), max(args.rollout_iters // 4, 3))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
