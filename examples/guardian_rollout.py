"""The expert guardian: the `[0, 1]` agent of the reference's examples/enjoy_saver.py -- no steering, full throttle -- with and without
`use_saver`, on N PGDrive-v0 environments.

    python examples/guardian_rollout.py --weights /path/to/pgdrive/examples/ppo_expert/expert_weights.npz --envs 1024 --save-level 0.5

No expert weights are shipped with this package; the reference's file works as it is (its 275-input network: the guardian's kernel
builds the lateral float of its row from the engine's state).  The guardian is one launch in front of every step: it evaluates the
expert on the observation the agent saw, corrects the action where the car is about to leave the road or to hit something, and leaves
the step info on the device -- `env.last_takeover` (bit 0 takeover, bit 1 takeover_start, bit 2 takeover_end) and
`env.last_applied_actions`.  As in the reference a correction is applied from the second consecutive step on; `--immediate` applies it
in the step that raises it.  Prints how the first episode of every env ended and the takeover share."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout without installing
from pgdrive_amd import PGDriveVecEnv  # noqa: E402


def first_episodes(env, steps):
    n = env.num_envs
    obs = env.reset(force_seed=1000 + np.arange(n) % 100)
    act = torch.tensor([0.0, 1.0], device=obs.device).repeat(n, 1).contiguous()
    alive = torch.ones(n, dtype=torch.bool, device=obs.device)
    end = torch.zeros(n, dtype=torch.int32, device=obs.device)
    take = torch.zeros((), dtype=torch.int64, device=obs.device)
    lived = torch.zeros((), dtype=torch.int64, device=obs.device)
    for t in range(steps):
        obs, reward, done, flags = env.step(act)
        if env.saver is not None:
            take += (((env.last_takeover & 1) != 0) & alive).sum()
        lived += alive.sum()
        d = done != 0
        end = torch.where(alive & d, flags, end)
        alive &= ~d
    info = env.info_from_flags(end)
    ends = {k: int(info[k].sum()) for k in ("arrive_dest", "out_of_road", "crash", "max_step")}
    ends["unfinished"] = int(alive.sum())
    return ends, int(take) / max(int(lived), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", required=True, help="the reference's examples/ppo_expert/expert_weights.npz")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--save-level", type=float, default=0.5)
    ap.add_argument("--traffic-density", type=float, default=0.1)
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--immediate", action="store_true")
    args = ap.parse_args()
    base = dict(num_envs=args.envs, start_seed=1000, environment_num=100, traffic_density=args.traffic_density)
    for name, extra in (("unguarded", {}),
                        ("guarded", dict(use_saver=True, save_level=args.save_level, saver_weights=args.weights,
                                         saver_deterministic=args.deterministic, saver_immediate=args.immediate))):
        env = PGDriveVecEnv(dict(base, **extra))
        ends, share = first_episodes(env, args.steps)
        print("%-9s first episodes of %d envs: %s; takeover in %.1f %% of their steps" % (name, args.envs, ends, 100.0 * share))
        env.close()


if __name__ == "__main__":
    main()
