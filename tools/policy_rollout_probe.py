"""Time per time step of BatchedRunner.run over a fused GymmaVecEnv: the two-launch path (actor launch + env step launch per time
step) against one_launch=True (rg_policy_rollout), in the same process, alternating, device-event timing after warm-up.

    python tools/policy_rollout_probe.py [--envs 4096] [--T 64] [--calls 4] [--samples 5]

One JSON line per (hidden size, path): median / min of `samples` samples, each `calls` x T time steps."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--epsilon", type=float, default=0.1)
    args = ap.parse_args()
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    from gpu_helpers import random_actor
    for H in (128, 64):
        v = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", args.envs, time_limit=100, seed=1,
                        overrides={"n_agents": 4, "predator": 2, "capture": 2})
        actor = BatchedActor(random_actor(1, v.obs_size + v.n_agents, H, v.n_actions, True, seed=2), v.n_agents, device=v.env.device)
        runner = BatchedRunner(v, actor, epsilon=args.epsilon, seed=3)
        times = {False: [], True: []}
        for one in (False, True, False, True):   # warm-up
            runner.run(args.T, one_launch=one)
        for _ in range(args.samples):
            for one in (False, True):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.calls):
                    runner.run(args.T, one_launch=one)
                b.record()
                b.synchronize()
                times[one].append(a.elapsed_time(b) * 1000.0 / (args.calls * args.T))
        for one in (False, True):
            ts = sorted(times[one])
            print(json.dumps({"envs": args.envs, "agents": v.n_agents, "hidden": H, "T": args.T, "epsilon": args.epsilon,
                              "path": "one_launch" if one else "two_launch", "us_per_step_median": ts[len(ts) // 2],
                              "us_per_step_min": ts[0], "samples": ts}))
        v.env.close()


if __name__ == "__main__":
    main()
