"""PPO-Lagrangian on the safe env, made of the engine's own launches: collect() -> update() with a cost critic and a Lagrange multiplier
(pgdrive_amd.SafeRolloutCollector and pgdrive_amd.PPOLagLearner: pgd_mlp_actor_critic_cost per step, pgd_cost_gae behind the rollout,
then pgd_lagrange, pgd_adv_stats twice, pgd_adv_mix and pgd_ppo_grad_cost + pgd_adam per epoch and minibatch).

    python examples/ppo_lag_train.py --envs 256 --T 32 --eager 3 --replays 20 [--cost-limit 1.0] [--every 5]
    python examples/ppo_lag_train.py --time --envs 4096 --T 128 [--windows 7] [--calls 3] [--plain]
    python examples/ppo_lag_train.py --horizon 100 --bootstrap-truncations     # an episode that ends at the horizon is bootstrapped, not cut
    python examples/ppo_lag_train.py --shuffle --target-kl 0.015 --anneal-lr   # random minibatches, a KL stop, a learning-rate schedule

The env is PGDriveVecEnv configured as SafePGDriveEnv (pgdrive/envs/safe_pgdrive_env.py:7-60): accident scenes on the road, crashes are
costs and not terminations.  A few iterations run eagerly; then one `collect(); update()` is captured in a HIP graph and replayed.
Printed: the multiplier, the mean episode cost J_c it last saw, the losses of the update's last minibatch and env-steps per second; the
prints read the device, the iteration itself does not.  --shuffle, --target-kl, --anneal-lr: the learner's minibatch switches (DESIGN.md
section 29); with a gate the prints show how many Adam steps the last update applied and skipped (the last minibatch's row is zero
behind a stop).

--time: collect() and update() timed apart, eagerly and as replays of a graph of each, each warmed up, then `--windows` windows of
`--calls` calls (host clock around a device synchronisation); the median window and the spread are printed.  --plain times
RolloutCollector + PPOLearner in the same way on the same env (the pair without the cost side)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout without installing
from pgdrive_amd import PGDriveVecEnv, _abi  # noqa: E402

SAFE = dict(accident_prob=0.8, traffic_density=0.05, safe_rl_env=True, crash_vehicle_cost=1.0, crash_object_cost=1.0, out_of_road_cost=1.0,
            use_lateral=False)  # SafePGDriveEnv's defaults (safe_pgdrive_env.py:9-23)


def random_networks(D, rng):
    def net(heads):
        return [rng.normal(0, D ** -0.5, (D, 256)), np.zeros(256), rng.normal(0, 1 / 16, (256, 256)), np.zeros(256),
                rng.normal(0, 1 / 16, (256, heads)), np.zeros(heads)]
    p, v, c = net(4), net(1), net(1)
    p[4][:, 0] *= 0.05                   # (a small steering gain and a bias towards the throttle: the cars drive)
    p[5][:] = (0.0, 0.5, -1.0, -1.0)     # log_std -1: std 0.37
    p[4][:, 2:] *= 0.1
    dev = lambda w: tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in w)  # noqa: E731
    return dev(p), dev(v), dev(c)


def make(args):
    env = PGDriveVecEnv(dict(SAFE, num_envs=args.envs, start_seed=1000, environment_num=100, auto_reset=True, horizon=args.horizon))
    pw, vw, cw = random_networks(env.obs_dim, np.random.default_rng(0))
    env.reset()
    switches = dict(shuffle=args.shuffle, shuffle_seed=args.shuffle_seed, target_kl=args.target_kl, lr_scale=args.anneal_lr)
    if getattr(args, "plain", False):
        from pgdrive_amd import PPOLearner, RolloutCollector
        col = RolloutCollector(env, pw, vw, args.T, seed=0, bootstrap_truncations=args.bootstrap_truncations, normalise_obs=args.normalise_obs)
        learner = PPOLearner(col, lr=args.lr, epochs=args.epochs, minibatches=args.minibatches, **switches)
    else:
        from pgdrive_amd import PPOLagLearner, SafeRolloutCollector
        col = SafeRolloutCollector(env, pw, vw, cw, args.T, seed=0, bootstrap_truncations=args.bootstrap_truncations,
                                   normalise_obs=args.normalise_obs)
        learner = PPOLagLearner(col, cost_limit=args.cost_limit, lambda_lr=args.lambda_lr, lr=args.lr, epochs=args.epochs,
                                minibatches=args.minibatches, **switches)
    return env, col, learner


def timed(run, windows, calls, warmup, graph):
    """Median, smallest and largest of `windows` windows of `calls` calls of run() [us per call], eagerly or replayed from a HIP graph."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(warmup):
            run()
        torch.cuda.synchronize()
        if graph:
            g = torch.cuda.CUDAGraph()
    if graph:
        with torch.no_grad(), torch.cuda.graph(g, stream=s):
            run()
        call = g.replay
    else:
        call = run
    us = []
    with torch.cuda.stream(s), torch.no_grad():
        call()
        for _ in range(windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / calls * 1e6)
    return statistics.median(us), min(us), max(us)


def time_pair(args):
    env, col, learner = make(args)
    eng = env.engine
    print("pgd_source_sha %s; %s: %d envs x T = %d, %d inputs, %d epochs x %d minibatches, %d windows of %d calls" % (
        eng.L.pgd_source_sha().decode(), "RolloutCollector + PPOLearner" if args.plain else "SafeRolloutCollector + PPOLagLearner", args.envs,
        args.T, eng.D, args.epochs, args.minibatches, args.windows, args.calls))
    with torch.no_grad():
        batch = col.collect()
    for name, run in (("collect()", col.collect), ("update()", lambda: learner.update(batch))):
        for graph in (False, True):
            med, lo, hi = timed(run, args.windows, args.calls, 2, graph)
            print("%-10s %-6s %12.1f us per call (median of %d windows; %.1f .. %.1f)" % (name, "graph" if graph else "eager", med, args.windows, lo, hi))
            sys.stdout.flush()
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--horizon", type=int, default=1000)
    ap.add_argument("--eager", type=int, default=3, help="iterations run eagerly before the capture")
    ap.add_argument("--replays", type=int, default=20, help="replays of the captured iteration")
    ap.add_argument("--every", type=int, default=5, help="print every k replays")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--cost-limit", type=float, default=1.0, help="the mean cost of an episode the policy is held under")
    ap.add_argument("--lambda-lr", type=float, default=0.05)
    ap.add_argument("--time", action="store_true", help="time collect() and update() apart, eagerly and from a graph")
    ap.add_argument("--plain", action="store_true", help="--time: RolloutCollector + PPOLearner instead of the safe pair")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed window")
    ap.add_argument("--bootstrap-truncations", action="store_true",
                    help="GAE and cost GAE bootstrap through the horizon from the critics' values of the terminal observation (DESIGN.md section 24)")
    ap.add_argument("--normalise-obs", action="store_true",
                    help="the networks read the observations normalised by their running mean and variance (DESIGN.md section 27)")
    ap.add_argument("--shuffle", action="store_true", help="a fresh permutation of the rollout's rows per epoch (DESIGN.md section 29)")
    ap.add_argument("--shuffle-seed", type=int, default=0)
    ap.add_argument("--target-kl", type=float, default=None,
                    help="stop an update on the device where mean(logp_old - logp) of a minibatch exceeds 1.5 times this (DESIGN.md section 29)")
    ap.add_argument("--anneal-lr", action="store_true",
                    help="the learning rate falls linearly to zero over the iterations: a device float written between them (DESIGN.md section 29)")
    args = ap.parse_args()
    if args.time:
        return time_pair(args)
    env, col, learner = make(args)
    eng = env.engine
    print("pgd_source_sha %s; %d safe envs x T = %d, cost limit %g, %d epochs x %d minibatches" % (
        eng.L.pgd_source_sha().decode(), args.envs, args.T, args.cost_limit, args.epochs, args.minibatches))

    def iteration():
        return learner.update(col.collect())

    def report(tag):
        torch.cuda.synchronize()
        lam, jc, episodes, _ = learner.lagrange_state.cpu().numpy()
        st = dict(zip(_abi.PPO_COST_STATS, learner.stats[-1].cpu().numpy()))
        print("%-12s lambda %7.4f  J_c %7.4f over %4d episodes  mean reward %8.4f  mean cost %.4f  L_pi %.4g  L_v %.4g  L_c %.4g  kl %.3g" % (
            tag, lam, jc, int(episodes), float(col.batch["rewards"].mean()), float(col.batch["costs"].mean()), st["policy_loss"],
            st["value_loss"], st["cost_value_loss"], st["approx_kl"]) + ("" if learner.gate is None else "  steps applied %d, skipped %d" % (
                int(learner.gate[1]), int(learner.gate[2]))))

    total, done = max(1, args.eager) + args.replays, [0]

    def anneal():  # (a device write between iterations and between replays: the float lr is frozen into the captured graph, this factor is not)
        if args.anneal_lr:
            learner.lr_scale.fill_(1.0 - done[0] / total)
        done[0] += 1

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for it in range(1, max(1, args.eager) + 1):  # (the first collect() primes the collector: outside the capture)
            anneal()
            iteration()
            report("eager %d" % it)
        graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=s):
        iteration()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(s), torch.no_grad():
        for it in range(1, args.replays + 1):
            anneal()
            graph.replay()
            if it % args.every == 0 or it == args.replays:
                report("replay %d" % it)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%d replays in %.2f s: %.1f k env-steps/s including the prints" % (args.replays, dt, args.replays * args.envs * args.T / dt / 1e3))
    env.close()


if __name__ == "__main__":
    main()
