"""Episode statistics and terminal observations without leaving the GPU: N PGDrive-v0 environments with step info on the device.

    python examples/episode_stats_rollout.py --envs 4096 --steps 2000

`step_info=True` adds one launch per step.  `env.last_info` is a dict of device tensors that the step refreshes in place: the
reference's step-info floats (velocity, steering, acceleration, step_energy, episode_energy, episode_reward, episode_length, cost,
total_cost) of the state the step ended in, and "final_observation": row e is the observation of the state env e's last episode ended
in -- what a trainer bootstraps from when the episode ended at a time limit -- while obs[e] is already the first row of the next one.
`env.episode_stats()` reduces the per-env statistics of the finished episodes (one synchronisation) and clears them."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout without installing
from pgdrive_amd import PGDriveVecEnv, _abi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--horizon", type=int, default=500)
    args = ap.parse_args()
    env = PGDriveVecEnv(dict(num_envs=args.envs, start_seed=1000, environment_num=100, horizon=args.horizon, step_info=True))
    obs = env.reset()
    info = env.last_info
    truncated_rows = torch.zeros(1, dtype=torch.int64, device=obs.device)
    for t in range(args.steps):
        actions = torch.rand((args.envs, 2), device=obs.device) * 2 - 1
        actions[:, 1] = actions[:, 1].abs()
        obs, reward, done, flags = env.step(actions)
        # a value-function bootstrap would read info["final_observation"][truncated] here: the rows are on the device already
        truncated = (done != 0) & ((flags & _abi.F_MAX_STEP) != 0) & ((flags & (_abi.F_ARRIVE | _abi.F_OUT_OF_ROAD)) == 0)
        truncated_rows += truncated.sum(0, keepdim=True)
        if (t + 1) % 500 == 0:
            print("step %d:" % (t + 1), env.episode_stats(), "mean velocity now %.1f km/h" % float(info["velocity"].mean()))
    print("time-limit ends whose terminal row was kept:", int(truncated_rows))
    env.close()


if __name__ == "__main__":
    main()
