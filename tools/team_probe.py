"""rg_step time per step without a team pool and with one (DESIGN.md "Team pool").  Variants, alternated in one process,
device-event timing after warm-up, random actions, auto-reset on:

    PredatorCapturePrey 4096 x 5 (the headline shape) and MaterialTransport 2048 x 6:
        off   no pool: the default kernel (the body compiled for that agent count)
        C1    a pool of one set (the config's own values): the team kernel of the same body
        C4    a pool of four sets that differ in every capability, drawn per episode
    PredatorCapturePrey 4096 x 5 as four fixed teams -- the case the pool exists for:
        4x1024_fixed   four handles of 1 024 envs, each with its own capabilities (no pool), stepped one after the other
        1x4096_C4      one handle of 4 096 envs with the four teams as a C = 4 pool

    python tools/team_probe.py [--steps 200] [--samples 7]

One JSON line per (shape, variant): median / min ms per step over `samples` samples of `steps` steps (a step of the 4 x 1 024
variant is the four launches)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PCP5 = {"predator": 3, "capture": 2, "n_agents": 5}
MT6 = {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25}
# four PredatorCapturePrey teams: 4+1, 3+2, 2+3 and 1+4 sensing / capturing agents
PCP_TEAMS = [{"sensing_radius": [0.45 if a < k else 0.0 for a in range(5)], "capture_radius": [0.0 if a < k else 0.25 for a in range(5)]}
             for k in (4, 3, 2, 1)]
MT_TEAMS = [{"speed": [0.1 + 0.05 * ((a + t) % 3) for a in range(6)], "torque": [1 + (a + 2 * t) % 7 for a in range(6)]} for t in range(4)]
SHAPES = [("PredatorCapturePrey", 4096, PCP5, PCP_TEAMS), ("MaterialTransport", 2048, MT6, MT_TEAMS)]


def _env(scenario, E, ov, teams=None, offset=0):
    from marbler_amd.vec_env import VecRobotariumEnv
    o = dict(ov, **({"teams": teams} if teams is not None else {}))
    env = VecRobotariumEnv(scenario, E, overrides=o, device="cuda:0", seed=0, auto_reset=True, env_offset=offset)
    env.reset()
    env._sync_stream()
    return env


def _timed(variants, steps, samples, warmup):
    """variants: name -> list of (env, actions [steps, E, N]); one step of a variant = one rg_step on each of its envs."""
    def run(name, k):
        for t in range(k):
            for env, a in variants[name]:
                rc = env.step_raw(a[t % a.shape[0]].data_ptr())
                if rc != 0:
                    raise RuntimeError(f"rg_step failed ({rc})")
    for name in variants:
        run(name, warmup)
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(samples):
        for name in variants:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            run(name, steps)
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) / steps)
    return times


def _acts(env, steps):
    n_act = 20 if env.scenario == "MaterialTransport" else 5
    g = torch.Generator(device="cpu").manual_seed(1)
    return torch.randint(0, n_act, (steps, env.E, env.N), generator=g, dtype=torch.int32).to(env.device)


def _report(scenario, E, N, times, base_name, kernels):
    base = sorted(times[base_name])[len(times[base_name]) // 2]
    for name, ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        print(json.dumps({"scenario": scenario, "envs": E, "agents": N, "variant": name, "kernel": kernels[name],
                          "ms_per_step_median": round(med, 5), "ms_per_step_min": round(ts[0], 5),
                          f"vs_{base_name}": round(med / base, 4), "samples": [round(t, 5) for t in ts]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=50)
    args = ap.parse_args()
    for scenario, E, ov, teams in SHAPES:
        envs = {"off": _env(scenario, E, ov), "C1": _env(scenario, E, ov, [{}]), "C4": _env(scenario, E, ov, teams)}
        variants = {k: [(v, _acts(v, args.steps))] for k, v in envs.items()}
        times = _timed(variants, args.steps, args.samples, args.warmup)
        _report(scenario, E, envs["off"].N, times, "off", {k: v.step_kernel for k, v in envs.items()})
        for v in envs.values():
            v.close()
    # the case the pool exists for: four team mixes of PredatorCapturePrey
    E = 4096
    shards = []
    for i, t in enumerate(PCP_TEAMS):
        o = dict(PCP5, predator=sum(1 for r in t["sensing_radius"] if r > 0), capture=sum(1 for r in t["capture_radius"] if r > 0))
        env = _env("PredatorCapturePrey", E // 4, o, offset=i * (E // 4))
        shards.append((env, _acts(env, args.steps)))
    pooled = _env("PredatorCapturePrey", E, PCP5, PCP_TEAMS)
    variants = {"4x1024_fixed": shards, "1x4096_C4": [(pooled, _acts(pooled, args.steps))]}
    times = _timed(variants, args.steps, args.samples, args.warmup)
    _report("PredatorCapturePrey", E, 5, times, "4x1024_fixed", {"4x1024_fixed": shards[0][0].step_kernel, "1x4096_C4": pooled.step_kernel})


if __name__ == "__main__":
    main()
