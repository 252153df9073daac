"""What normalise_rewards costs, at the benchmark configuration: 4096 envs x (1 ego + 16 traffic slots) x 240 beams,
274 inputs, PGDrive-v0 maps 1000..1099, auto-reset.

    python tools/return_norm_cost.py collect [--forms off,on] [--T 128] [--windows 7] [--calls 3]
    python tools/return_norm_cost.py kernel [--T 128] [--windows 5] [--launches 500]

collect: RolloutCollector.collect() with the switch off (today's calls: what the parent commit's collect() issues) and on, one collector
each on ONE engine, taking turns window by window so that drift hits both alike; 2 warm-up calls per form, then `--windows` windows of
`--calls` calls between two HIP events; the median window and the spread, microseconds per call.  With PGD_LIB naming a library built
from the parent commit, run `--forms off`: that is the parent's collect().
kernel: calls back to back on the engine's stream over the rewards and dones of a real rollout [T, envs], `--windows` windows of
`--launches` calls between two HIP events, microseconds per call:
    return_norm    Engine.return_norm: the row scan, the merge workgroup and the scaling
    frozen         the same with freeze=True: the scaling launch alone
    gae            Engine.gae on the same arrays, for scale
Under `rocprofv3 --kernel-trace --stats -- python tools/return_norm_cost.py kernel ...` the trace gives each kernel's own time.
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
    ap.add_argument("what", choices=("collect", "kernel"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--maps", type=int, default=100)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--forms", default="off,on")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--launches", type=int, default=500)
    args = ap.parse_args()
    n = args.envs
    descs = bank.get_descriptions(range(1000, 1000 + args.maps))
    mb = mapdata.MapBank(descs)
    sb = scenario.ScenarioBank(descs, [d["seed"] for d in descs], num_agents=1, num_traffic=16)
    eng = Engine(_abi.make_config(n, auto_reset=1, seed=1234), mb, sb)
    eng.reset(np.arange(n) % len(descs))
    pw, vw = networks(eng.D, np.random.default_rng(0))
    out = dict(tool="return_norm_cost", what=args.what, pgd_source_sha=eng.L.pgd_source_sha().decode(), envs=n, in_dim=eng.D, T=args.T,
               device=torch.cuda.get_device_name(0), timing="HIP events")
    with torch.no_grad():
        if args.what == "collect":
            forms = args.forms.split(",")
            cols = {f: RolloutCollector(eng, pw, vw, args.T, seed=0, **(dict(normalise_rewards=True) if f == "on" else {})) for f in forms}
            for f in forms:
                for _ in range(2):
                    cols[f].collect()
            us = {f: [] for f in forms}
            for _ in range(args.windows):
                for f in forms:
                    us[f].append(window_us(cols[f].collect, args.calls))
            med, spread = summary(us)
            out.update(windows=args.windows, calls_per_window=args.calls, windows_us=us, us_per_collect=med, spread_us=spread)
            if "on" in forms:
                out.update(return_norm=dict(zip(_abi.RETURN_NORM_RECORD, cols["on"].return_norm.cpu().tolist())))
        else:
            col = RolloutCollector(eng, pw, vw, args.T, seed=0)
            col.collect()
            batch = col.collect()
            reward, done, value = batch["rewards"].clone(), batch["dones"].clone(), batch["values"].clone()
            carry, record = eng.return_norm_state(n)
            scaled, adv, ret = [torch.empty_like(reward) for _ in range(3)]
            work = torch.empty(((eng.return_norm_work_bytes(n) + 7) // 8, ), dtype=torch.float64, device="cuda")
            runs = dict(
                return_norm=lambda: eng.return_norm(reward, done, 0.99, carry, record, out=scaled, work=work),
                frozen=lambda: eng.return_norm(reward, done, 0.99, carry, record, freeze=True, out=scaled, work=work),
                gae=lambda: eng.gae(reward, value, done, 0.99, 0.95, adv=adv, ret=ret))
            for run in runs.values():
                for _ in range(200):
                    run()
            us = {k: [] for k in runs}
            for _ in range(args.windows):
                for k, run in runs.items():
                    us[k].append(window_us(run, args.launches))
            med, spread = summary(us)
            out.update(windows=args.windows, launches_per_window=args.launches, windows_us=us, us_per_call=med, spread_us=spread,
                       bytes=dict(reward=reward.numel() * 4, done=done.numel(), scaled=scaled.numel() * 4),
                       return_norm=dict(zip(_abi.RETURN_NORM_RECORD, record.cpu().tolist())))
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
