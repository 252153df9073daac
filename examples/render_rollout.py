"""Top-down frames of two roll-outs: the 40-seat multi-agent roundabout and a PGDrive-v0 vec env (traffic drawn as well).

    python examples/render_rollout.py [--steps 100] [--every 10] [--out render_frames]

env.render(mode="top_down") draws the whole map with every agent and its fading trail (pgdrive_amd/csrc/pgd_render.h) on the GPU,
for all envs of the batch in one launch.  Frames are written as PNG when PIL imports, else as .npy.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def save(img, path):
    try:
        from PIL import Image
        Image.fromarray(img).save(path + ".png")
        return path + ".png"
    except ImportError:
        np.save(path + ".npy", img)
        return path + ".npy"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--every", type=int, default=10, help="write every k-th frame (all of them are rendered)")
    ap.add_argument("--out", default="render_frames")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    from pgdrive_amd import PGDriveVecEnv
    from pgdrive_amd.marl_env import MultiAgentRoundaboutVecEnv
    rng = np.random.default_rng(0)
    written = []
    # the roundabout with 40 agent seats, 4 envs; random throttle-biased actions: agents crash, wait as static bodies (red disks)
    ma = MultiAgentRoundaboutVecEnv(dict(num_envs=4, num_agents=40))
    ma.reset()
    for t in range(args.steps):
        a = rng.uniform(-1, 1, size=(ma.num_envs, ma.A, 2)).astype(np.float32)
        a[..., 1] = np.abs(a[..., 1])
        ma.step(torch.from_numpy(a).cuda())
        frames = ma.render(mode="top_down")  # cuda uint8 [4, 1000, 1000, 3]
        if t % args.every == 0 or t == args.steps - 1:
            written.append(save(frames[0].cpu().numpy(), os.path.join(args.out, "roundabout_%03d" % t)))
    ma.close()
    # PGDrive-v0, 8 envs, the ego and (not a reference option) the IDM traffic
    sa = PGDriveVecEnv(dict(num_envs=8, start_seed=1000, environment_num=100))
    sa.reset()
    for t in range(args.steps):
        a = np.stack([rng.normal(0.0, 0.1, 8), rng.uniform(0.3, 1.0, 8)], axis=1).astype(np.float32)
        sa.step(torch.from_numpy(a).cuda())
        frames = sa.render(mode="top_down", draw_traffic=True)
        if t % args.every == 0 or t == args.steps - 1:
            written.append(save(frames[0].cpu().numpy(), os.path.join(args.out, "pgdrive_v0_%03d" % t)))
    sa.close()
    print("wrote %d frames to %s (e.g. %s)" % (len(written), args.out, written[-1]))


if __name__ == "__main__":
    main()
