"""rg_step time per step with the lidar off and on (DESIGN.md "Lidar"), at PredatorCapturePrey 4096 x 5 (the headline shape) and
MaterialTransport 2048 x 6 (BASELINE.json configs[4]'s per-GPU share).  Variants, alternated in one process, device-event timing
after warm-up, random actions, auto-reset on:

    off        the default kernel (for N = 5, 6 in groups of 8: the body compiled for that agent count)
    off_gymma  the generic-agent-count body (NT = 0) with the gymma block -- the lidar kernels' body without the lidar
    R4 R16 R32 the lidar kernels (generic body), R rays, L = 1 m
    R16_gymma  the lidar kernel with the gymma block: against off_gymma, the lidar arithmetic alone

    python tools/lidar_probe.py [--steps 200] [--samples 7]

One JSON line per (shape, variant): median / min ms per step over `samples` samples of `steps` steps."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("PredatorCapturePrey", 4096, {"predator": 3, "capture": 2, "n_agents": 5}),
          ("MaterialTransport", 2048, {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25})]
VARIANTS = [("off", 0, False), ("off_gymma", 0, True), ("R4", 4, False), ("R16", 16, False), ("R32", 32, False),
            ("R16_gymma", 16, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=50)
    args = ap.parse_args()
    from marbler_amd.vec_env import VecRobotariumEnv
    for scenario, E, ov in SHAPES:
        envs, acts = {}, {}
        for name, R, gym in VARIANTS:
            o = dict(ov, **({"lidar_rays": R, "lidar_range": 1.0} if R else {}))
            env = VecRobotariumEnv(scenario, E, overrides=o, device="cuda:0", seed=0, auto_reset=True)
            if gym:
                env.enable_time_limit(10 ** 6)
            env.reset()
            n_act = 20 if scenario == "MaterialTransport" else 5
            g = torch.Generator(device="cpu").manual_seed(1)
            acts[name] = torch.randint(0, n_act, (args.steps, E, env.N), generator=g, dtype=torch.int32).to(env.device)
            env._sync_stream()
            envs[name] = env

        def run(name, k):
            env, a = envs[name], acts[name]
            for t in range(k):
                rc = env.step_raw(a[t % a.shape[0]].data_ptr())
                if rc != 0:
                    raise RuntimeError(f"rg_step failed ({rc})")

        for name, _, _ in VARIANTS:
            run(name, args.warmup)
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in VARIANTS}
        for _ in range(args.samples):
            for name, _, _ in VARIANTS:
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                run(name, args.steps)
                e.record()
                e.synchronize()
                times[name].append(s.elapsed_time(e) / args.steps)
        base = sorted(times["off"])[len(times["off"]) // 2]
        for name, R, gym in VARIANTS:
            ts = sorted(times[name])
            med = ts[len(ts) // 2]
            print(json.dumps({"scenario": scenario, "envs": E, "agents": envs[name].N, "variant": name, "rays": R, "gymma": gym,
                              "kernel": envs[name].step_kernel, "ms_per_step_median": round(med, 5),
                              "ms_per_step_min": round(ts[0], 5), "vs_off": round(med / base, 4),
                              "samples": [round(t, 5) for t in ts]}), flush=True)
        for env in envs.values():
            env.close()


if __name__ == "__main__":
    main()
