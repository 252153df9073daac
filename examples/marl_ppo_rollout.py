"""PPO rollouts of the multi-agent roundabout collected on the device (pgdrive_amd.MultiAgentRolloutCollector: per step the live seat
rows -- pgd_live_rows --, the actor and the critic over those rows only -- pgd_mlp_actor_critic_rows --, and behind the rollout GAE
per agent -- pgd_gae_masked -- and the index of the transitions -- pgd_rollout_index), next to what could be composed before:
pgd_mlp_actor_critic over all N x A seat rows at every step and pgd_gae over the seats.

    python examples/marl_ppo_rollout.py --envs 4096 --agents 40 --T 32 [--windows 7] [--rollouts 5] [--preroll 60] [--launch]

Random weights of the shape of the reference's shipped PPO expert (see examples/ppo_rollout.py): a throughput example.  The composed form
is NOT a usable rollout -- its GAE bootstraps a seat's successive agents into each other and its batch has no mask; it stands for the
cost of the networks over empty seats.  Printed: the live fraction of every timed rollout of the collector (agent-steps over seat-steps,
from the batch's count), the time per rollout of both forms (the protocol of examples/ppo_rollout.py: warm-up, then `--windows` windows
of `--rollouts` rollouts, host clock around a device synchronisation, median and spread), and with --launch the network launch alone,
back to back from a HIP graph (device events): pgd_mlp_actor_critic over all rows against pgd_mlp_actor_critic_rows with the live rows
of the last rollout's last step, with every row listed, and with none."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout without installing
from pgdrive_amd import MultiAgentRolloutCollector, MultiAgentRoundaboutVecEnv  # noqa: E402

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


class AllRowsRollout:
    """What the library offered before the collector: Engine.step(out=...), Engine.mlp_actor_critic over every seat row, Engine.gae."""
    def __init__(self, eng, pw, vw, T):
        N, A, D = eng.N, eng.A, eng.D
        f = dict(dtype=torch.float32, device="cuda")
        self.eng, self.pw, self.vw, self.T = eng, pw, vw, T
        self.obs = torch.zeros((T + 1, N, A, D), **f)
        self.actions, self.logp, self.values = torch.zeros((T + 1, N, A, 2), **f), torch.zeros((T + 1, N, A), **f), torch.zeros((T + 1, N, A), **f)
        self.rewards = torch.zeros((T, N, A), **f)
        self.dones = torch.zeros((T, N, A), dtype=torch.uint8, device="cuda")
        self.flags = torch.zeros((T, N, A), dtype=torch.int32, device="cuda")
        self.adv, self.ret = torch.zeros((T, N, A), **f), torch.zeros((T, N, A), **f)
        self.obs[T].copy_(eng.obs)
        self._evaluate(T)

    def _evaluate(self, t):
        self.eng.mlp_actor_critic(self.pw, self.vw, self.actions[t], self.logp[t], self.values[t], 0, t, obs=self.obs[t])

    def collect(self):
        T = self.T
        for buf in (self.obs, self.actions, self.logp, self.values):
            buf[0].copy_(buf[T])
        for t in range(T):
            self.eng.step(self.actions[t], out=(self.obs[t + 1], self.rewards[t], self.dones[t], self.flags[t]))
            self._evaluate(t + 1)
        self.eng.gae(self.rewards, self.values, self.dones, GAMMA, LAM, adv=self.adv, ret=self.ret)


def timed(run, windows, rollouts, warmup, each=None):
    """Median and spread over `windows` windows of `rollouts` calls of run() [ms per rollout]; each(): called behind every rollout of
    the timed windows (it may read the device: the clock is stopped around it)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    ms = []
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(warmup):
            run()
        for _ in range(windows):
            spent = 0.0
            for _ in range(rollouts):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                spent += time.perf_counter() - t0
                if each is not None:
                    each()
            ms.append(spent / rollouts * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def launch_alone(eng, pw, vw, live_rows, live_count, windows):
    """us per launch, back to back: 50 launches in a graph, events around 8 replays, the median and spread of `windows` such timings,
    the forms alternating inside every window."""
    N, A = eng.N, eng.A
    n = N * A
    act, logp, value = torch.zeros((N, A, 2), device="cuda"), torch.zeros((N, A), device="cuda"), torch.zeros((N, A), device="cuda")
    every = torch.arange(n, dtype=torch.int32, device="cuda")
    c_all, c_none = torch.full((1, ), n, dtype=torch.int32, device="cuda"), torch.zeros((1, ), dtype=torch.int32, device="cuda")
    k_live = int(live_count.item())
    rows = lambda r, c: (lambda: eng.mlp_actor_critic_rows(pw, vw, r, c, act, logp, value, 0, 0))  # noqa: E731
    forms = (("pgd_mlp_actor_critic, all %d rows" % n, lambda: eng.mlp_actor_critic(pw, vw, act, logp, value, 0, 0)),
             ("pgd_mlp_actor_critic_rows, %d live rows (%.0f %%)" % (k_live, 100.0 * k_live / n), rows(live_rows, live_count)),
             ("pgd_mlp_actor_critic_rows, every row listed", rows(every, c_all)),
             ("pgd_mlp_actor_critic_rows, no row listed", rows(every, c_none)))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graphs = []
    for name, fn in forms:
        with torch.no_grad(), torch.cuda.stream(s):
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(g, stream=s):
            for _ in range(50):
                fn()
        torch.cuda.synchronize()
        graphs.append((name, g, []))
    with torch.cuda.stream(s):
        for _ in range(windows):
            for name, g, us in graphs:
                g.replay()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(8):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / 400)
    for name, _, us in graphs:
        print("%-56s x %d floats: %8.2f us per call back to back (median of %d; %.2f .. %.2f)" % (
            name, eng.D, statistics.median(us), len(us), min(us), max(us)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=40)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rollouts", type=int, default=5, help="rollouts per timed window")
    ap.add_argument("--warmup", type=int, default=2, help="rollouts before the first window")
    ap.add_argument("--preroll", type=int, default=60, help="rollouts of the collector before anything is timed: the roundabout fills up")
    ap.add_argument("--launch", action="store_true", help="also time the network launch alone, all rows against listed rows")
    args = ap.parse_args()
    pw = vw = None
    live = None
    for form in ("collector", "all_rows"):
        env = MultiAgentRoundaboutVecEnv(dict(num_envs=args.envs, num_agents=args.agents, seed=3))
        eng = env.engine
        if pw is None:
            print("pgd_source_sha %s; %d envs x %d seats x T = %d, %d windows of %d rollouts, %d rollouts before" % (
                eng.L.pgd_source_sha().decode(), args.envs, eng.A, args.T, args.windows, args.rollouts, args.preroll))
            pw, vw = random_networks(env.obs_dim, np.random.default_rng(0))
        env.reset()
        steps = args.envs * args.T
        if form == "collector":
            col = MultiAgentRolloutCollector(env, pw, vw, args.T, gamma=GAMMA, lam=LAM, seed=0)
            col.prime()
            fractions = []
            med, lo, hi = timed(col.collect, args.windows, args.rollouts, args.warmup + args.preroll,
                                each=lambda: fractions.append(float(col.count.item()) / col.mask.numel()))
            print("live fraction per timed rollout: %s" % " ".join("%.3f" % f for f in fractions))
            b = col.batch
            n = int(b["count"].item())
            idx = b["index"][:n].long()
            print("last rollout: %d agent-steps of %d seat-steps, mean reward %.4f, %d agent ends, mean |advantage| %.3f" % (
                n, b["mask"].numel(), float(b["rewards"].view(-1)[idx].mean()), int(b["dones"].view(-1)[idx].sum()),
                float(b["advantages"].view(-1)[idx].abs().mean())))
            live = (col._rows.clone(), col._n_rows.clone())
        else:
            ar = AllRowsRollout(eng, pw, vw, args.T)
            med, lo, hi = timed(ar.collect, args.windows, args.rollouts, args.warmup + args.preroll)
        print("%-10s %8.2f ms per rollout (median of %d windows; %.2f .. %.2f)  %.1f us per step, %.1f M env-steps/s" % (
            form, med, args.windows, lo, hi, med * 1e3 / args.T, steps / med / 1e3))
        if form == "all_rows" and args.launch:
            launch_alone(eng, pw, vw, live[0], live[1], args.windows)
        env.close()


if __name__ == "__main__":
    main()
