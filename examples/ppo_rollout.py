"""PPO rollouts collected on the device (pgdrive_amd.RolloutCollector: one launch per step for the sampled action, its log-probability
and the value estimate -- pgd_mlp_actor_critic --, GAE behind the rollout -- pgd_gae), next to the same rollout composed from torch
ops around Engine.step: both networks as addmm + tanh, randn, the log-probability, and a python loop over T for GAE.

    python examples/ppo_rollout.py --envs 4096 --T 64 [--windows 7] [--rollouts 20] [--launch]

Random weights of the shape of the reference's shipped PPO expert (pgdrive/examples/ppo_expert/numpy_expert.py: two tanh MLPs with two
256-wide hidden layers, a policy head of four outputs -- mean, log_std -- and a value head of one): this is a throughput example.
Every form is warmed up, then timed over `--windows` windows of `--rollouts` rollouts each (host clock around a device synchronisation);
the median window and the spread (min .. max) are printed as env-steps/s.  --launch adds the launch alone, back to back from a HIP graph
(device events), next to pgd_mlp_policy on the same build."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout without installing
from pgdrive_amd import PGDriveVecEnv, RolloutCollector  # noqa: E402

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


class TorchRollout:
    """The rollout from what the library offered before the collector: Engine.step(out=...) and framework ops."""
    def __init__(self, eng, pw, vw, T):
        N, D = eng.N, eng.D
        f = dict(dtype=torch.float32, device="cuda")
        self.eng, self.pw, self.vw, self.T = eng, pw, vw, T
        self.obs = torch.zeros((T + 1, N, D), **f)
        self.actions, self.logp = torch.zeros((T, N, 2), **f), torch.zeros((T, N), **f)
        self.values, self.rewards = torch.zeros((T + 1, N), **f), torch.zeros((T, N), **f)
        self.dones = torch.zeros((T, N), dtype=torch.uint8, device="cuda")
        self.flags = torch.zeros((T, N), dtype=torch.int32, device="cuda")
        self.adv, self.ret = torch.zeros((T, N), **f), torch.zeros((T, N), **f)
        self.obs[T].copy_(eng.obs.view(N, D))

    @staticmethod
    def _mlp(w, o):
        h = torch.tanh(torch.addmm(w[1], o, w[0]))
        h = torch.tanh(torch.addmm(w[3], h, w[2]))
        return torch.addmm(w[5], h, w[4])

    def collect(self):
        T, N = self.T, self.eng.N
        self.obs[0].copy_(self.obs[T])
        for t in range(T):
            out = self._mlp(self.pw, self.obs[t])
            self.values[t] = self._mlp(self.vw, self.obs[t]).view(N)
            mean, ls = out[:, :2], out[:, 2:4]
            z = torch.randn((N, 2), device="cuda")
            torch.addcmul(mean, torch.exp(ls), z, out=self.actions[t])
            self.logp[t] = -0.5 * (z * z).sum(1) - ls.sum(1) - math.log(2.0 * math.pi)
            self.eng.step(self.actions[t], out=(self.obs[t + 1], self.rewards[t], self.dones[t], self.flags[t]))
        self.values[T] = self._mlp(self.vw, self.obs[T]).view(N)
        a = torch.zeros((N, ), device="cuda")
        for t in range(T - 1, -1, -1):
            nt = 1.0 - self.dones[t].float()
            a = self.rewards[t] + GAMMA * self.values[t + 1] * nt - self.values[t] + GAMMA * LAM * nt * a
            self.adv[t] = a
        torch.add(self.adv, self.values[:T], out=self.ret)


def timed(run, env_steps, windows, rollouts, warmup, graph):
    """Median and spread over `windows` windows of `rollouts` calls of run() [env-steps/s], eagerly or replayed from a HIP graph."""
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
    rates = []
    with torch.cuda.stream(s), torch.no_grad():
        call()
        for _ in range(windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(rollouts):
                call()
            torch.cuda.synchronize()
            rates.append(env_steps * rollouts / (time.perf_counter() - t0))
    return statistics.median(rates), min(rates), max(rates)


def launch_alone(eng, pw, vw, windows):
    """us per launch, back to back: 50 launches in a graph, events around 8 replays, the median and spread of `windows` such timings."""
    N = eng.N
    act = torch.zeros((N, 1, 2), device="cuda")
    logp, value = torch.zeros((N, 1), device="cuda"), torch.zeros((N, 1), device="cuda")
    policy2 = tuple(pw[:4]) + (pw[4][:, :2].contiguous(), pw[5][:2].contiguous())
    forms = (("pgd_mlp_policy", lambda: eng.mlp_policy(policy2, act)),
             ("pgd_mlp_actor_critic, no critic", lambda: eng.mlp_actor_critic(pw, None, act, logp, None, 0, 0)),
             ("pgd_mlp_actor_critic", lambda: eng.mlp_actor_critic(pw, vw, act, logp, value, 0, 0)))
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
        for _ in range(windows):  # (the forms alternate inside every window)
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
        print("%-34s %d rows x %d: %.2f us per launch back to back (median of %d; %.2f .. %.2f)" % (
            name, N, eng.D, statistics.median(us), len(us), min(us), max(us)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rollouts", type=int, default=20, help="rollouts per timed window")
    ap.add_argument("--warmup", type=int, default=3, help="rollouts before the first window (and before a graph is captured)")
    ap.add_argument("--launch", action="store_true", help="also time the launch alone against pgd_mlp_policy")
    ap.add_argument("--forms", default="collector,collector_graph,torch,torch_graph")
    args = ap.parse_args()
    env = PGDriveVecEnv(dict(num_envs=args.envs, start_seed=1000, environment_num=100, auto_reset=True))
    eng = env.engine
    print("pgd_source_sha %s; %d envs x T = %d, %d windows of %d rollouts" % (
        eng.L.pgd_source_sha().decode(), args.envs, args.T, args.windows, args.rollouts))
    pw, vw = random_networks(env.obs_dim, np.random.default_rng(0))
    env.reset()
    if args.launch:
        launch_alone(eng, pw, vw, args.windows)
    steps = args.envs * args.T
    for form in args.forms.split(","):
        env.reset()
        if form.startswith("collector"):
            col = RolloutCollector(env, pw, vw, args.T, gamma=GAMMA, lam=LAM, seed=0)
            col.prime()
            run = col.collect
        else:
            run = TorchRollout(eng, pw, vw, args.T).collect
        med, lo, hi = timed(run, steps, args.windows, args.rollouts, args.warmup, form.endswith("_graph"))
        print("%-16s %7.1f M env-steps/s (median of %d windows; %.1f .. %.1f)  %.1f us per step" % (
            form, med / 1e6, args.windows, lo / 1e6, hi / 1e6, args.envs / med * 1e6))
        if form == "collector":
            b = col.batch
            print("                 last rollout: mean reward %.4f, %d episode ends, mean |advantage| %.3f, mean logp %.3f" % (
                float(b["rewards"].mean()), int(b["dones"].sum()), float(b["advantages"].abs().mean()), float(b["logp"].mean())))
    env.close()


if __name__ == "__main__":
    main()
