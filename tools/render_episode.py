"""Renders an episode of a random policy to frames on disk.

    python tools/render_episode.py PredatorCapturePrey --steps 60 --env 0 --size 256 --out episode

Writes `<out>.npy` (uint8 [T + 1, H, W, 3]: frame 0 the state after reset, frame t + 1 the state after step t), and `<out>.gif`
too when Pillow happens to be importable -- it is no dependency of the project, the frames are the product.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scenario")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--env", type=int, default=0, help="which env of the batch to record")
    ap.add_argument("--num-envs", type=int, default=1)
    ap.add_argument("--size", type=int, nargs="+", default=[256], help="S (square) or H W")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="episode")
    ap.add_argument("--fps", type=float, default=10.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    from marbler_amd import VecRobotariumEnv, render
    from marbler_amd.gymma import N_ACTIONS
    size = args.size[0] if len(args.size) == 1 else tuple(args.size)
    render.parse_size(size)
    env = VecRobotariumEnv(args.scenario, max(args.num_envs, args.env + 1), seed=args.seed)
    env.reset()
    g = torch.Generator(device="cpu").manual_seed(args.seed)
    actions = torch.randint(0, N_ACTIONS[args.scenario], (args.steps, env.E, env.N), generator=g, dtype=torch.int32).to(env.device)
    frames = render.record(env, actions, size=size, envs=[args.env])[:, 0].cpu().numpy()
    np.save(args.out + ".npy", frames)
    print(f"{args.out}.npy: {frames.shape[0]} frames of {frames.shape[1]} x {frames.shape[2]}")
    try:
        from PIL import Image
    except ImportError:
        print("Pillow is not installed: no GIF written")
    else:
        images = [Image.fromarray(f) for f in frames]
        images[0].save(args.out + ".gif", save_all=True, append_images=images[1:], duration=int(1000 / args.fps), loop=0)
        print(f"{args.out}.gif")
    env.close()


if __name__ == "__main__":
    main()
