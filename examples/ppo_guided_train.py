"""Expert-guided PPO, made of the engine's own launches: the expert guardian watches the rollout (pgd_guardian in front of every step) and
the update knows which rows it overrode (pgdrive_amd.PPOLearner(guide=...): pgd_ppo_grad_guided + pgd_adam per epoch and minibatch).

    python examples/ppo_guided_train.py --weights /path/to/pgdrive/examples/ppo_expert/expert_weights.npz --guide takeover
    python examples/ppo_guided_train.py --weights ... --guide all --bc-coef 1.0          # behaviour cloning of the expert (DAgger)
    python examples/ppo_guided_train.py --weights ... --guide takeover --keep-surrogate  # imitation beside the surrogate, not instead

No expert weights are shipped with this package; the reference's file works as it is.  --guide takeover: the rows whose applied action
is not the sampled one drop their clipped surrogate and imitate what was applied; --guide all: every row imitates the expert's action on
the states the guarded agent visits, the critic still learns.  A few iterations run eagerly; then one `collect();
update()` is captured in a HIP graph and replayed.  Printed per iteration: the takeover share of the rollout, the guided rows and
bc_loss (the mean of -logp(target) over them) of the update's last minibatch, the mean reward and the return of the episodes that ended;
the prints read the device, the iteration itself does not."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout without installing
from pgdrive_amd import PGDriveVecEnv, PPOLearner, RolloutCollector, _abi  # noqa: E402
from pgdrive_amd.vec_env import load_saver_weights  # noqa: E402


def random_networks(D, rng):
    def net(heads):
        return [rng.normal(0, D ** -0.5, (D, 256)), np.zeros(256), rng.normal(0, 1 / 16, (256, 256)), np.zeros(256),
                rng.normal(0, 1 / 16, (256, heads)), np.zeros(heads)]
    p, v = net(4), net(1)
    p[4][:, 0] *= 0.05                   # (a small steering gain and a bias towards the throttle: the cars drive)
    p[5][:] = (0.0, 0.5, -1.0, -1.0)     # log_std -1: std 0.37
    p[4][:, 2:] *= 0.1
    dev = lambda w: tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in w)  # noqa: E731
    return dev(p), dev(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", required=True, help="the reference's examples/ppo_expert/expert_weights.npz")
    ap.add_argument("--guide", choices=("takeover", "all"), default="takeover")
    ap.add_argument("--bc-coef", type=float, default=1.0, help="the weight of -logp(target) on a guided row")
    ap.add_argument("--keep-surrogate", action="store_true", help="a guided row keeps its clipped surrogate")
    ap.add_argument("--save-level", type=float, default=0.5)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--horizon", type=int, default=1000)
    ap.add_argument("--eager", type=int, default=3, help="iterations run eagerly before the capture")
    ap.add_argument("--replays", type=int, default=20, help="replays of the captured iteration")
    ap.add_argument("--every", type=int, default=5, help="print every k replays")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--lr", type=float, default=3e-4)
    args = ap.parse_args()
    env = PGDriveVecEnv(dict(num_envs=args.envs, start_seed=1000, environment_num=100, auto_reset=True, horizon=args.horizon))
    pw, vw = random_networks(env.obs_dim, np.random.default_rng(0))
    expert = tuple(torch.from_numpy(np.ascontiguousarray(w)).cuda() for w in load_saver_weights(dict(saver_weights=args.weights), env.obs_dim))
    env.reset()
    col = RolloutCollector(env, pw, vw, args.T, seed=0, episode_stats=True, guardian=dict(weights=expert, save_level=args.save_level))
    learner = PPOLearner(col, lr=args.lr, epochs=args.epochs, minibatches=args.minibatches, guide=args.guide, bc_coef=args.bc_coef,
                         keep_surrogate=args.keep_surrogate)
    print("pgd_source_sha %s; %d envs x T = %d, save_level %g, guide %s, bc_coef %g%s, %d epochs x %d minibatches" % (
        env.engine.L.pgd_source_sha().decode(), args.envs, args.T, args.save_level, args.guide, args.bc_coef,
        ", the surrogate kept" if args.keep_surrogate else "", args.epochs, args.minibatches))

    def iteration():
        return learner.update(col.collect())

    def report(tag):
        torch.cuda.synchronize()
        st = dict(zip(_abi.PPO_GUIDED_STATS, learner.stats[-1].cpu().numpy()))
        ep = dict(zip(_abi.ROLLOUT_EPISODES, col.batch["episode_stats"].cpu().numpy()))
        share = float(((col.batch["takeover"] & 1) != 0).float().mean())
        print("%-10s takeover %5.1f %%  guided rows %5d of %5d  bc_loss %8.4f  L_pi %8.4g  L_v %8.4g  mean reward %7.4f  return %8.3f over %d episodes" % (
            tag, 100.0 * share, int(st["guided_rows"]), int(st["n"]), st["bc_loss"], st["policy_loss"], st["value_loss"],
            float(col.batch["rewards"].mean()), ep["return_mean"], int(ep["episodes"])))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for it in range(1, max(1, args.eager) + 1):  # (the first collect() primes the collector: outside the capture)
            iteration()
            report("eager %d" % it)
        graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=s):
        iteration()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(s), torch.no_grad():
        for it in range(1, args.replays + 1):
            graph.replay()
            if it % args.every == 0 or it == args.replays:
                report("replay %d" % it)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%d replays in %.2f s: %.1f k env-steps/s including the prints" % (args.replays, dt, args.replays * args.envs * args.T / dt / 1e3))
    env.close()


if __name__ == "__main__":
    main()
