"""What normalise_obs costs, at the closed-loop shape of examples/ppo_train.py: 4096 envs x (1 ego + 16 traffic
slots) x 240 beams, 274 inputs, PGDrive-v0 maps 1000..1099, auto-reset.

    python tools/obs_norm_cost.py loop [--forms off,on] [--T 32] [--windows 7] [--calls 3]
    python tools/obs_norm_cost.py kernel [--T 32] [--windows 5] [--launches 200]

loop: RolloutCollector.collect() and PPOLearner.update() with the switch off (today's calls: what the parent commit issues) and on, one
collector and learner each on ONE engine, taking turns window by window so that drift hits both alike; 2 warm-up calls per form, then
`--windows` windows of `--calls` calls between two HIP events; the median window and the spread, microseconds per call.  Run from a
checkout of the parent commit with `--forms off`, the same tool gives the parent's figures (it then passes no new keyword).
kernel: calls back to back on the engine's stream over the observations of a real rollout [T, envs, 274], microseconds per call:
    actor_critic          Engine.mlp_actor_critic on one step's rows, nothing bound
    actor_critic_bound    the same with a table bound: the fused form
    standalone_1          ONE elementwise launch over one step's rows into a second buffer (torch.addcmul: x * scale - shift * scale,
                          no clamp) -- the least a normalisation launch of its own could cost
    standalone_3          the rule itself as torch ops into a second buffer (sub, mul_, clamp_: three launches)
    fold                  Engine.obs_norm_update over the whole rollout
    publish               Engine.obs_norm_publish
Prints one JSON line, stamped with the library's source stamp (pgd_source_sha)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgdrive_amd import _abi, bank, mapdata, scenario  # noqa: E402
from pgdrive_amd.engine import Engine  # noqa: E402
from pgdrive_amd.learner import PPOLearner  # noqa: E402
from pgdrive_amd.rollout import RolloutCollector  # noqa: E402


def networks(D, rng):
    def net(heads):
        return [rng.normal(0, D ** -0.5, (D, 256)), np.zeros(256), rng.normal(0, 1 / 16, (256, 256)), np.zeros(256),
                rng.normal(0, 1 / 16, (256, heads)), np.zeros(heads)]
    p, v = net(4), net(1)
    p[4][:, 0] *= 0.05
    p[5][:] = (0.0, 0.5, -1.0, -1.0)
    dev = lambda w: tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in w)  # noqa: E731
    return dev(p), dev(v)


def window_us(run, calls):
    """`calls` calls between two events on the current stream -> microseconds per call."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def summary(us):
    return {k: statistics.median(v) for k, v in us.items()}, {k: (min(v), max(v)) for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("loop", "kernel"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--maps", type=int, default=100)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--forms", default="off,on")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    args = ap.parse_args()
    n = args.envs
    descs = bank.get_descriptions(range(1000, 1000 + args.maps))
    mb = mapdata.MapBank(descs)
    sb = scenario.ScenarioBank(descs, [d["seed"] for d in descs], num_agents=1, num_traffic=16)
    eng = Engine(_abi.make_config(n, auto_reset=1, seed=1234), mb, sb)
    eng.reset(np.arange(n) % len(descs))
    D = eng.D
    out = dict(tool="obs_norm_cost", what=args.what, pgd_source_sha=eng.L.pgd_source_sha().decode(), envs=n, in_dim=D, T=args.T,
               device=torch.cuda.get_device_name(0), timing="HIP events")
    with torch.no_grad():
        if args.what == "loop":
            forms = args.forms.split(",")
            cols, learners, batches = {}, {}, {}
            for f in forms:
                pw, vw = networks(D, np.random.default_rng(0))
                cols[f] = RolloutCollector(eng, pw, vw, args.T, seed=0, **(dict(normalise_obs=True) if f == "on" else {}))
                learners[f] = PPOLearner(cols[f], epochs=4, minibatches=4)
                for _ in range(2):
                    batches[f] = cols[f].collect()
                    learners[f].update(batches[f])
            us = {"%s %s" % (c, f): [] for f in forms for c in ("collect", "update")}
            for _ in range(args.windows):
                for f in forms:
                    us["collect " + f].append(window_us(cols[f].collect, args.calls))
                    us["update " + f].append(window_us(lambda: learners[f].update(batches[f]), args.calls))
            med, spread = summary(us)
            out.update(windows=args.windows, calls_per_window=args.calls, epochs=4, minibatches=4, windows_us=us, us_per_call=med, spread_us=spread)
            if "on" in forms:
                out.update(obs_samples=float(cols["on"].obs_norm_record[0]))
        else:
            pw, vw = networks(D, np.random.default_rng(0))
            col = RolloutCollector(eng, pw, vw, args.T, seed=0)
            col.collect()
            obs = col.collect()["obs"].clone()
            record, table = eng.obs_norm_state(D)
            work = torch.empty(((eng.obs_norm_work_bytes(D, args.T * n) + 7) // 8, ), dtype=torch.float64, device="cuda")
            eng.obs_norm_update(obs, record, work=work)
            eng.obs_norm_publish(record, table)
            a, lp, v = torch.empty((n, 1, 2), device="cuda"), torch.empty((n, 1), device="cuda"), torch.empty((n, 1), device="cuda")
            buf = torch.empty_like(obs[0])
            shift, scale = table[0, :D], table[1, :D]
            off = -(shift * scale)

            def bound():
                eng.mlp_actor_critic(pw, vw, a, lp, v, 0, 0, obs=obs[1])

            def standalone_3():
                torch.sub(obs[1], shift, out=buf)
                buf.mul_(scale)
                buf.clamp_(-10.0, 10.0)

            runs = dict(actor_critic=lambda: eng.mlp_actor_critic(pw, vw, a, lp, v, 0, 0, obs=obs[1]), actor_critic_bound=bound,
                        standalone_1=lambda: torch.addcmul(off, obs[1], scale, out=buf), standalone_3=standalone_3,
                        fold=lambda: eng.obs_norm_update(obs, record, work=work), publish=lambda: eng.obs_norm_publish(record, table))
            us = {k: [] for k in runs}
            for k, run in runs.items():
                eng.obs_norm_bind(table, D, 10.0) if k == "actor_critic_bound" else eng.obs_norm_bind(None)
                for _ in range(50):
                    run()
            for _ in range(args.windows):
                for k, run in runs.items():
                    eng.obs_norm_bind(table, D, 10.0) if k == "actor_critic_bound" else eng.obs_norm_bind(None)
                    us[k].append(window_us(run, args.launches))
            eng.obs_norm_bind(None)
            med, spread = summary(us)
            out.update(windows=args.windows, launches_per_window=args.launches, windows_us=us, us_per_call=med, spread_us=spread,
                       bytes=dict(step_rows=obs[0].numel() * 4, rollout=obs.numel() * 4))
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
