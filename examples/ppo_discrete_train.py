"""PPO with a DISCRETISED steering / throttle policy, made of the engine's own launches: two independent categorical heads over the 256-256
tanh network (pgdrive_amd.RolloutCollector(action_head="categorical", bins=(ks, kt)) and pgdrive_amd.PPOLearner: pgd_mlp_actor_critic_cat
per step, pgd_ppo_grad_cat + pgd_adam per epoch and minibatch).

    python examples/ppo_discrete_train.py --envs 256 --T 32 --iters 6 [--bins 5 5] [--discrete-env]
    python examples/ppo_discrete_train.py --time [--envs 4096] [--windows 7] [--launches 20]

A few collect(); update() iterations eagerly, then the same number replayed from ONE captured HIP graph; after each half the episode
statistics of the collector (episode_summary()) are printed.  The env keeps its continuous action space and is fed the grid value
i * 2 / (K - 1) - 1 of the sampled index, which is what a discrete_action env makes of index i -- the recommended way to train: with
--discrete-env the engine has discrete_action=True and is fed the index itself, and then, like the reference (EnvInputPolicy.act clips
the INDEX to [-1, 1] before it converts it), every index >= 1 becomes the same action.

--time: the per-launch time of pgd_mlp_actor_critic_cat next to pgd_mlp_actor_critic and of pgd_ppo_grad_cat next to pgd_ppo_grad on the
same build, same rows (--envs) and input width: each warmed up, then `--windows` windows of `--launches` launches (host clock around a
device synchronisation); the median window and the spread are printed."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout without installing
from pgdrive_amd import PGDriveVecEnv, PPOLearner, RolloutCollector, _abi  # noqa: E402


def random_networks(D, out_cols, rng):
    def net(heads):
        return [rng.normal(0, D ** -0.5, (D, 256)), np.zeros(256), rng.normal(0, 1 / 16, (256, 256)), np.zeros(256),
                rng.normal(0, 1 / 16, (256, heads)) * 0.1, np.zeros(heads)]
    dev = lambda w: tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in w)  # noqa: E731
    return dev(net(out_cols)), dev(net(1))


def summary(col, what):
    e = col.episode_summary()
    col.clear_episode_stats()
    print("%-8s episodes %5d  " % (what, e["episodes"]) + ("none ended" if not e["episodes"] else
          "success rate %.3f  out of road %.3f  return %.3f +- %.3f  mean length %.1f" % (
              e["arrive_rate"], e["out_of_road_rate"], e["mean_return"], e["std_return"], e["mean_length"])))


def windows_of(run, windows, launches):
    for _ in range(3):
        run()
    ms = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(launches):
            run()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / launches * 1e6)
    return statistics.median(ms), min(ms), max(ms)


def time_launches(args):
    env = PGDriveVecEnv(dict(num_envs=args.envs, start_seed=1000, environment_num=100, auto_reset=True))
    eng, bins = env.engine, tuple(args.bins)
    N, D = args.envs, eng.D
    env.reset()
    rng = np.random.default_rng(0)
    cw, vw = random_networks(D, sum(bins), rng)
    gw, _ = random_networks(D, 4, rng)
    f32 = dict(dtype=torch.float32, device="cuda")
    act, logp, value = torch.zeros((N, 1, 2), **f32), torch.zeros((N, 1), **f32), torch.zeros((N, 1), **f32)
    idx = torch.zeros((N, 1, 2), dtype=torch.int32, device="cuda")
    print("pgd_source_sha %s; %d rows x %d inputs, bins %r; %d windows of %d launches [us per launch: median (min .. max)]" % (
        eng.L.pgd_source_sha().decode(), N, D, bins, args.windows, args.launches))
    forms = [("pgd_mlp_actor_critic", lambda: eng.mlp_actor_critic(gw, vw, act, logp, value, 0, 0)),
             ("pgd_mlp_actor_critic_cat", lambda: eng.mlp_actor_critic_cat(cw, vw, bins, act, idx, logp, value, 0, 0))]
    eng.mlp_actor_critic_cat(cw, vw, bins, act, idx, logp, value, 0, 0)
    logp_c, idx_c = logp.clone(), idx.clone()
    eng.mlp_actor_critic(gw, vw, act, logp, value, 0, 0)
    adv, ret = torch.randn((N, ), **f32), torch.randn((N, ), **f32)
    stats = torch.zeros((8, ), **f32)
    work = torch.empty(((eng.ppo_cat_work_bytes(D, N) + 3) // 4, ), **f32)
    grads = lambda ws: tuple(torch.zeros_like(w) for w in ws)  # noqa: E731
    gg, cg, vg = grads(gw), grads(cw), grads(vw)
    act_g, logp_g = act.clone(), logp.clone()
    forms += [("pgd_ppo_grad", lambda: eng.ppo_grad(gw, vw, gg, vg, eng.obs, act_g, logp_g, adv, ret, stats, work)),
              ("pgd_ppo_grad_cat", lambda: eng.ppo_grad_cat(cw, vw, cg, vg, bins, eng.obs, idx_c, logp_c, adv, ret, stats, work))]
    for name, run in forms:
        med, lo, hi = windows_of(run, args.windows, args.launches)
        print("%-28s %9.2f (%.2f .. %.2f)" % (name, med, lo, hi))
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=None)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--iters", type=int, default=6, help="iterations per half: eager, then replayed from a HIP graph")
    ap.add_argument("--bins", type=int, nargs=2, default=(5, 5), help="steering and throttle bins")
    ap.add_argument("--discrete-env", action="store_true", help="an engine with discrete_action=True, fed the index (see the docstring)")
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--time", action="store_true", help="time the categorical launches next to the Gaussian ones")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    args = ap.parse_args()
    if args.envs is None:
        args.envs = 4096 if args.time else 256
    if args.time:
        return time_launches(args)
    bins = tuple(args.bins)
    cfg = dict(num_envs=args.envs, start_seed=1000, environment_num=100, auto_reset=True)
    if args.discrete_env:
        cfg.update(discrete_action=True, discrete_steering_dim=bins[0], discrete_throttle_dim=bins[1])
    env = PGDriveVecEnv(cfg)
    eng = env.engine
    print("pgd_source_sha %s; %d envs x T = %d, bins %r, the env is fed %s" % (
        eng.L.pgd_source_sha().decode(), args.envs, args.T, bins, "the index" if args.discrete_env else "the grid value"))
    pw, vw = random_networks(env.obs_dim, sum(bins), np.random.default_rng(0))
    env.reset()
    col = RolloutCollector(env, pw, vw, args.T, seed=0, episode_stats=True, action_head="categorical", bins=bins)
    learner = PPOLearner(col, lr=args.lr, ent_coef=0.01)

    def iteration():
        return learner.update(col.collect())

    def report(what):
        torch.cuda.synchronize()
        b, st = col.batch, learner.stats[-1].cpu().numpy()
        counts = torch.bincount(b["action_index"][..., 0].reshape(-1), minlength=bins[0]).tolist()
        print("%-8s Adam step %4d  mean reward %8.4f  steering bins %s  " % (what, int(learner.step[0]), float(b["rewards"].mean()), counts) +
              "  ".join("%s %.4g" % (k, x) for k, x in zip(_abi.PPO_STATS[:7], st)))
        summary(col, what)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(args.iters):
            iteration()
        report("eager")
        g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g, stream=s):
        iteration()
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(args.iters):
            g.replay()
        report("graph")
    env.close()


if __name__ == "__main__":
    main()
