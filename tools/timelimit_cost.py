"""What bootstrap_truncations costs, at the benchmark configuration: 4096 envs x (1 ego + 16 traffic slots) x 240
beams, 274 inputs, PGDrive-v0 maps 1000..1099, auto-reset, the step info on.

    python tools/timelimit_cost.py collect [--forms off,on] [--T 128] [--horizon 1000] [--windows 5] [--calls 3]
    python tools/timelimit_cost.py kernel [--windows 5] [--launches 2000]

collect: RolloutCollector.collect() with the switch off (today's calls: what the parent commit's collect() issues on an engine with step
info) and on, one collector each on ONE engine, taking turns window by window so that drift hits both alike; 2 warm-up calls per form,
then `--windows` windows of `--calls` calls, host clock around a device synchronisation; the median window and the spread, microseconds
per call.  With PGD_LIB naming a library built from the parent commit, run `--forms off`: that is the parent's collect().
kernel: launches back to back on the engine's stream, `--windows` windows of `--launches` launches, microseconds per launch:
    empty          pgd_step_info_empty_launch: N workgroups of one wave that do nothing -- the floor of one more launch
    term_none      pgd_mlp_terminal_value, no env truncated: every workgroup reads 16 flags and dones, writes 16 zeros and ends
    term_all       pgd_mlp_terminal_value, every env truncated in the same step: every workgroup runs the critic
    actor_critic   pgd_mlp_actor_critic: the actor and the critic workgroups side by side (term_all is its critic half alone)
    actor          pgd_mlp_actor_critic without a critic: the actor half alone
Prints one JSON line, stamped with the library's source stamp (pgd_source_sha)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgdrive_amd import _abi, bank, mapdata, scenario  # noqa: E402
from pgdrive_amd.engine import Engine, _chk  # noqa: E402
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


def windows_of(run, windows, calls):
    us = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            run()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) / calls * 1e6)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("collect", "kernel"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--maps", type=int, default=100)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--horizon", type=int, default=1000)
    ap.add_argument("--forms", default="off,on")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--launches", type=int, default=2000)
    args = ap.parse_args()
    n = args.envs
    descs = bank.get_descriptions(range(1000, 1000 + args.maps))
    mb = mapdata.MapBank(descs)
    sb = scenario.ScenarioBank(descs, [d["seed"] for d in descs], num_agents=1, num_traffic=16)
    eng = Engine(_abi.make_config(n, auto_reset=1, seed=1234, horizon=args.horizon), mb, sb)
    eng.reset(np.arange(n) % len(descs))
    eng.enable_step_info()
    pw, vw = networks(eng.D, np.random.default_rng(0))
    out = dict(tool="timelimit_cost", what=args.what, pgd_source_sha=eng.L.pgd_source_sha().decode(), envs=n, in_dim=eng.D,
               device=torch.cuda.get_device_name(0))
    with torch.no_grad():
        if args.what == "collect":
            forms = args.forms.split(",")
            cols = {f: RolloutCollector(eng, pw, vw, args.T, seed=0, **(dict(bootstrap_truncations=True) if f == "on" else {})) for f in forms}
            for f in forms:
                for _ in range(2):
                    cols[f].collect()
            us = {f: [] for f in forms}
            trunc = {f: 0 for f in forms}
            for _ in range(args.windows):
                for f in forms:
                    us[f] += windows_of(cols[f].collect, 1, args.calls)
                    b = cols[f].batch
                    trunc[f] += int(((b["dones"] != 0) & ((b["flags"] & _abi.F_MAX_STEP) != 0)).sum())
            out.update(T=args.T, horizon=args.horizon, windows=args.windows, calls_per_window=args.calls, windows_us=us,
                       us_per_collect={f: statistics.median(v) for f, v in us.items()},
                       spread_us={f: (min(v), max(v)) for f, v in us.items()}, max_step_dones_in_last_call_of_each_window=trunc)
        else:
            L, h = eng.L, eng.h
            act = torch.zeros((n, 1, 2), device="cuda")
            logp, val, tv = [torch.zeros(n, device="cuda") for _ in range(3)]
            obs = eng.obs.view(n, -1)
            none_f, none_d = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
            all_f, all_d = torch.full((n, ), _abi.F_MAX_STEP | _abi.F_RESET, dtype=torch.int32, device="cuda"), torch.ones(n, dtype=torch.uint8, device="cuda")
            runs = dict(
                empty=lambda: _chk(L.pgd_step_info_empty_launch(h), "pgd_step_info_empty_launch"),
                term_none=lambda: eng.mlp_terminal_value(vw, None, obs, none_f, none_d, tv),
                term_all=lambda: eng.mlp_terminal_value(vw, None, obs, all_f, all_d, tv),
                actor_critic=lambda: eng.mlp_actor_critic(pw, vw, act, logp, val, 0, 0, obs=obs),
                actor=lambda: eng.mlp_actor_critic(pw, None, act, logp, None, 0, 0, obs=obs))
            for run in runs.values():
                for _ in range(200):
                    run()
            us = {k: [] for k in runs}
            for _ in range(args.windows):
                for k, run in runs.items():
                    us[k] += windows_of(run, 1, args.launches)
            assert float(tv.abs().sum()) > 0.0   # (the last window of term_all, then actor_critic: tv holds values)
            out.update(windows=args.windows, launches_per_window=args.launches, windows_us=us,
                       us_per_launch={k: statistics.median(v) for k, v in us.items()}, spread_us={k: (min(v), max(v)) for k, v in us.items()})
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
