"""A complete PPO iteration made of the engine's own launches: collect() -> update(), eagerly and with one iteration captured in a HIP graph
(pgdrive_amd.RolloutCollector / MultiAgentRolloutCollector and pgdrive_amd.PPOLearner: pgd_adv_stats, then pgd_ppo_grad + pgd_adam per
epoch and minibatch).

    python examples/ppo_train.py --envs 256 --T 32 --iters 20 [--graph] [--marl [--agents 40]] [--every 5] [--episode-stats] [--normalise-obs]
                                 [--shuffle] [--target-kl 0.015] [--anneal-lr]
    python examples/ppo_train.py --time --envs 4096 --T 64 [--windows 7] [--updates 3] [--shuffle] [--target-kl 0.015]

Random initial weights of the shape of the reference's shipped PPO expert (pgdrive/examples/ppo_expert/numpy_expert.py).  Printed every
`--every` iterations: the mean reward of the rollout and the statistics of the update's last minibatch (pgdrive_amd._abi.PPO_STATS); these
prints read the device, the iteration itself does not.  --episode-stats: a second line per print with the episodes that finished since
the last print -- their number, the success rate (arrive_dest at the episode's end), mean and standard deviation of the return and the
mean length (the collector's episode_stats switch) -- and the number of episodes so far.  --shuffle: a fresh
permutation of the rollout's rows per epoch; --target-kl: an update stops on the device where a minibatch's KL estimate exceeds 1.5 times
the value (the prints then show how many Adam steps the last update applied and skipped); --anneal-lr: the learning rate falls linearly
to zero over --iters through the learner's device float lr_scale, written between iterations and between graph replays alike (DESIGN.md
section 29).

--time: update() alone on one fixed batch in three forms on the same build -- the engine's kernels, the same update composed from torch
ops with autograd and torch.optim.Adam eagerly, and that composition captured in a HIP graph --, each warmed up, then `--windows` windows
of `--updates` updates (host clock around a device synchronisation); the median window and the spread are printed."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout without installing
from pgdrive_amd import MultiAgentRolloutCollector, MultiAgentRoundaboutVecEnv, PGDriveVecEnv, PPOLearner, RolloutCollector, _abi  # noqa: E402

GAMMA, LAM = 0.99, 0.95


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


class TorchUpdate:
    """PPOLearner.update composed from framework ops on a single-agent batch: strided minibatches gathered by slicing, autograd over both
    networks, clip_grad_norm_, torch.optim.Adam (capturable: its step counter lives on the device, as pgd_adam's does)."""
    def __init__(self, pw, vw, lr=3e-4, clip=0.2, vf_coef=0.5, ent_coef=0.0, epochs=4, minibatches=4, max_grad_norm=0.5, eps=1e-5):
        self.p = [w.clone().requires_grad_(True) for w in tuple(pw) + tuple(vw)]
        self.opt = torch.optim.Adam(self.p, lr=lr, eps=eps, capturable=True)
        self.clip, self.vf, self.ce, self.epochs, self.n_mb, self.max_norm = clip, vf_coef, ent_coef, epochs, minibatches, max_grad_norm

    @staticmethod
    def _mlp(w, o):
        h = torch.tanh(torch.addmm(w[1], o, w[0]))
        h = torch.tanh(torch.addmm(w[3], h, w[2]))
        return torch.addmm(w[5], h, w[4])

    def update(self, batch):
        D = batch["obs"].shape[-1]
        obs, act = batch["obs"].reshape(-1, D), batch["actions"].reshape(-1, 2)
        lpo, adv, ret = batch["logp"].reshape(-1), batch["advantages"].reshape(-1), batch["returns"].reshape(-1)
        adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
        for _ in range(self.epochs):
            for j in range(self.n_mb):
                o, a, l0, A, R = obs[j::self.n_mb], act[j::self.n_mb], lpo[j::self.n_mb], adv[j::self.n_mb], ret[j::self.n_mb]
                out = self._mlp(self.p[:6], o)
                mean, ls = out[:, :2], out[:, 2:4]
                z = (a - mean) * torch.exp(-ls)
                logp = -0.5 * (z * z).sum(1) - ls.sum(1) - math.log(2.0 * math.pi)
                r = torch.exp(logp - l0)
                l_pi = -torch.minimum(r * A, torch.clamp(r, 1.0 - self.clip, 1.0 + self.clip) * A).mean()
                l_v = (0.5 * (self._mlp(self.p[6:], o)[:, 0] - R) ** 2).mean()
                ent = (ls.sum(1) + math.log(2.0 * math.pi * math.e)).mean()
                loss = l_pi + self.vf * l_v - self.ce * ent
                self.opt.zero_grad(set_to_none=False)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(self.p, self.max_norm)
                self.opt.step()


def timed(run, windows, updates, warmup, graph):
    """Median and spread over `windows` windows of `updates` calls of run() [ms per call], eagerly or replayed from a HIP graph."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(warmup):
            run()
        torch.cuda.synchronize()
        if graph:
            g = torch.cuda.CUDAGraph()
    if graph:
        with torch.cuda.graph(g, stream=s):
            run()
        call = g.replay
    else:
        call = run
    ms = []
    with torch.cuda.stream(s):
        call()
        for _ in range(windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(updates):
                call()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / updates * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def time_update(args):
    env = PGDriveVecEnv(dict(num_envs=args.envs, start_seed=1000, environment_num=100, auto_reset=True))
    eng = env.engine
    print("pgd_source_sha %s; update() alone: %d envs x T = %d (%d rows x %d inputs), %d epochs x %d minibatches, %d windows of %d updates" % (
        eng.L.pgd_source_sha().decode(), args.envs, args.T, args.envs * args.T, eng.D, args.epochs, args.minibatches, args.windows, args.updates))
    pw, vw = random_networks(env.obs_dim, np.random.default_rng(0))
    env.reset()
    col = RolloutCollector(env, pw, vw, args.T, gamma=GAMMA, lam=LAM, seed=0)
    with torch.no_grad():
        batch = col.collect()
    learner = PPOLearner(col, lr=args.lr, epochs=args.epochs, minibatches=args.minibatches, shuffle=args.shuffle, shuffle_seed=args.shuffle_seed,
                         target_kl=args.target_kl, lr_scale=args.anneal_lr)
    tu = TorchUpdate(pw, vw, epochs=args.epochs, minibatches=args.minibatches)
    forms = (("engine kernels", lambda: learner.update(batch), False), ("engine kernels, graph", lambda: learner.update(batch), True),
             ("torch autograd + Adam, eager", lambda: tu.update(batch), False), ("torch autograd + Adam, graph", lambda: tu.update(batch), True))
    for name, run, graph in forms:
        if args.only and args.only not in name:
            continue
        try:
            med, lo, hi = timed(run, args.windows, args.updates, 3, graph)
            print("%-30s %9.3f ms per update (median of %d windows; %.3f .. %.3f)" % (name, med, args.windows, lo, hi))
        except Exception as e:  # (a framework that cannot capture its optimiser says so; the other forms still run)
            print("%-30s failed: %s" % (name, str(e).splitlines()[0]))
        sys.stdout.flush()
    st = learner.stats.cpu().numpy()
    print("engine, last minibatch: " + ", ".join("%s %.4g" % (n, x) for n, x in zip(_abi.PPO_STATS[:7], st[-1])))
    if learner.gate is not None:
        print("engine, last update: " + ", ".join("%s %d" % (n, x) for n, x in zip(_abi.ADAM_GATE, learner.gate.tolist())))
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--every", type=int, default=5, help="print the statistics every k iterations")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--graph", action="store_true", help="capture one collect() + update() in a HIP graph and replay it")
    ap.add_argument("--marl", action="store_true", help="the multi-agent roundabout (MultiAgentRolloutCollector)")
    ap.add_argument("--agents", type=int, default=40)
    ap.add_argument("--time", action="store_true", help="time update() alone against the torch composition")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--updates", type=int, default=3, help="updates per timed window")
    ap.add_argument("--only", default="", help="--time: only the forms whose name contains this")
    ap.add_argument("--horizon", type=int, default=None, help="the time limit of an episode (default: none)")
    ap.add_argument("--bootstrap-truncations", action="store_true",
                    help="GAE bootstraps through the horizon from the critic's value of the terminal observation (DESIGN.md section 24)")
    ap.add_argument("--normalise-rewards", action="store_true",
                    help="GAE reads the rewards divided by the standard deviation of the running discounted return (DESIGN.md section 25)")
    ap.add_argument("--normalise-obs", action="store_true",
                    help="the networks read the observations normalised by their running mean and variance (DESIGN.md section 27)")
    ap.add_argument("--episode-stats", action="store_true",
                    help="print the statistics of the episodes that finished since the last print (DESIGN.md section 26)")
    ap.add_argument("--shuffle", action="store_true", help="a fresh permutation of the rollout's rows per epoch (DESIGN.md section 29)")
    ap.add_argument("--shuffle-seed", type=int, default=0)
    ap.add_argument("--target-kl", type=float, default=None,
                    help="stop an update on the device where mean(logp_old - logp) of a minibatch exceeds 1.5 times this (DESIGN.md section 29)")
    ap.add_argument("--anneal-lr", action="store_true",
                    help="the learning rate falls linearly to zero over --iters: a device float written between iterations (DESIGN.md section 29)")
    args = ap.parse_args()
    if args.time:
        return time_update(args)
    if args.marl:
        env = MultiAgentRoundaboutVecEnv(dict(num_envs=args.envs, num_agents=args.agents, seed=3))
    else:
        env = PGDriveVecEnv(dict(num_envs=args.envs, start_seed=1000, environment_num=100, auto_reset=True, horizon=args.horizon))
    eng = env.engine
    print("pgd_source_sha %s; %d envs x %d seats x T = %d, %d epochs x %d minibatches, %s" % (
        eng.L.pgd_source_sha().decode(), args.envs, eng.A, args.T, args.epochs, args.minibatches, "HIP graph" if args.graph else "eager"))
    pw, vw = random_networks(env.obs_dim, np.random.default_rng(0))
    env.reset()
    if args.marl:   # (no such switch: the cause of a done cannot be read from a multi-agent step's flags)
        assert not args.bootstrap_truncations, "--bootstrap-truncations serves single-agent engines"
        col = MultiAgentRolloutCollector(env, pw, vw, args.T, gamma=GAMMA, lam=LAM, seed=0, normalise_rewards=args.normalise_rewards,
                                         episode_stats=args.episode_stats, normalise_obs=args.normalise_obs)
    else:
        col = RolloutCollector(env, pw, vw, args.T, gamma=GAMMA, lam=LAM, seed=0, bootstrap_truncations=args.bootstrap_truncations,
                               normalise_rewards=args.normalise_rewards, episode_stats=args.episode_stats, normalise_obs=args.normalise_obs)
    learner = PPOLearner(col, lr=args.lr, epochs=args.epochs, minibatches=args.minibatches, ent_coef=0.0, shuffle=args.shuffle,
                         shuffle_seed=args.shuffle_seed, target_kl=args.target_kl, lr_scale=args.anneal_lr)

    def iteration():
        return learner.update(col.collect())

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        iteration()  # (the first collect() primes the collector -- a host read for the multi-agent one --: outside any capture)
        torch.cuda.synchronize()
        if args.graph:
            g = torch.cuda.CUDAGraph()
    if args.graph:
        with torch.no_grad(), torch.cuda.graph(g, stream=s):
            iteration()
        call = g.replay
    else:
        call = iteration
    episodes = 0
    if args.episode_stats:
        col.clear_episode_stats()  # (the statistics start behind the warm-up iterations; the unfinished episodes stay)
    t0 = time.perf_counter()
    with torch.cuda.stream(s), torch.no_grad():
        for it in range(1, args.iters + 1):
            if args.anneal_lr:  # (a device write between two replays: the float lr is frozen into the captured graph, this factor is not)
                learner.lr_scale.fill_(1.0 - (it - 1) / args.iters)
            call()
            if it % args.every == 0 or it == args.iters:
                torch.cuda.synchronize()
                b = col.batch
                st = learner.stats[-1].cpu().numpy()
                if args.marl:
                    n = int(b["count"].item())
                    reward = float(b["rewards"].view(-1)[b["index"][:n].long()].mean()) if n else 0.0
                else:
                    reward = float(b["rewards"].mean())
                scale = "  reward scale %.4g" % float(b["return_norm"][3]) if args.normalise_rewards else ""
                if args.normalise_obs:
                    scale += "  obs samples %d, largest scale %.4g" % (int(b["obs_norm_record"][0]), float(b["obs_norm"][1].max()))
                if learner.gate is not None:  # (the last row may lie behind a stop: n = 0)
                    scale += "  steps applied %d, skipped %d" % (int(learner.gate[1]), int(learner.gate[2]))
                    if args.anneal_lr:
                        scale += "  lr %.3g" % (args.lr * float(learner.lr_scale[0]))
                print("iteration %4d  Adam step %5d  mean reward %8.4f  " % (it, int(learner.step[0]), reward) +
                      "  ".join("%s %.4g" % (k, x) for k, x in zip(_abi.PPO_STATS[:7], st)) + scale)
                if args.episode_stats:
                    e = col.episode_summary()
                    col.clear_episode_stats()
                    episodes += e["episodes"]
                    print("                episodes %6d (so far %7d)  " % (e["episodes"], episodes) + ("none ended" if not e["episodes"] else
                          "success rate %.3f  out of road %.3f  return %.3f +- %.3f  mean length %.1f" % (
                              e["arrive_rate"], e["out_of_road_rate"], e["mean_return"], e["std_return"], e["mean_length"])))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%d iterations in %.2f s: %.1f k env-steps/s including the prints" % (args.iters, dt, args.iters * args.envs * args.T / dt / 1e3))
    env.close()


if __name__ == "__main__":
    main()
