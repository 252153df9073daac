"""What the expert guardian costs, at 4096 envs x (1 ego + 16 traffic slots) x 240 beams, PGDrive-v0 maps
1000..1099, auto-reset.

    python tools/guardian_cost.py kernel [--windows 5] [--launches 200]
    python tools/guardian_cost.py loop [--windows 7] [--replays 20] [--unroll 16]
    python tools/guardian_cost.py trace [--launches 50]        (under rocprofv3 --kernel-trace --stats: the launches alone, no timing)

kernel: calls back to back on the engine's stream over the rows of a real step, microseconds per call:
    actor             Engine.mlp_actor_critic without a critic, 274 inputs -- the network the guardian evaluates, alone
    actor_275         the same with 275 inputs (a host-assembled row)
    guardian          Engine.guardian with a 274-input expert (the plain row)
    guardian_legacy   Engine.guardian with a 275-input expert (the row with the lateral float)
loop: the closed loop mlp_actor_critic (actor and critic) -> [guardian ->] step, `--unroll` iterations captured in ONE HIP graph per form,
the two graphs replayed in turns window by window; microseconds per iteration.
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


def network(k, heads, rng):
    w = [rng.normal(0, k ** -0.5, (k, 256)), np.zeros(256), rng.normal(0, 1 / 16, (256, 256)), np.zeros(256), rng.normal(0, 1 / 16, (256, heads)),
         np.zeros(heads)]
    if heads == 4:
        w[4][:, 0] *= 0.05
        w[5][:] = (0.0, 0.5, -1.0, -1.0)
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in w)


def window_us(run, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernel", "loop", "trace"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--maps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--unroll", type=int, default=16)
    ap.add_argument("--save-level", type=float, default=0.5)
    args = ap.parse_args()
    n = args.envs
    descs = bank.get_descriptions(range(1000, 1000 + args.maps))
    mb = mapdata.MapBank(descs)
    sb = scenario.ScenarioBank(descs, [d["seed"] for d in descs], num_agents=1, num_traffic=16)
    eng = Engine(_abi.make_config(n, auto_reset=1, seed=1234), mb, sb)
    eng.reset(np.arange(n) % len(descs))
    D = eng.D
    rng = np.random.default_rng(0)
    pw, vw = network(D, 4, rng), network(D, 1, rng)
    ex, ex_legacy = network(D, 4, rng), network(D + 1, 4, rng)
    act = torch.zeros((n, 1, 2), device="cuda")
    applied = torch.zeros((n, 1, 2), device="cuda")
    lp, val = torch.zeros((n, 1), device="cuda"), torch.zeros((n, 1), device="cuda")
    st, info = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = dict(tool="guardian_cost", what=args.what, pgd_source_sha=eng.L.pgd_source_sha().decode(), envs=n, in_dim=D,
               save_level=args.save_level, device=torch.cuda.get_device_name(0), timing="HIP events")
    with torch.no_grad():
        for t in range(40):  # a real step's rows: the cars are under way
            eng.mlp_actor_critic(pw, vw, act, lp, val, 0, t)
            eng.step(act)
        torch.cuda.synchronize()
        if args.what in ("kernel", "trace"):
            obs = eng.obs.view(n, D).clone()
            wide = torch.cat([obs[:, :8], torch.full((n, 1), 0.5, device="cuda"), obs[:, 8:]], dim=1).contiguous()
            runs = dict(actor=lambda: eng.mlp_actor_critic(ex, None, act, lp, None, 0, 0, obs=obs),
                        actor_275=lambda: eng.mlp_actor_critic(ex_legacy, None, act, lp, None, 0, 0, obs=wide),
                        guardian=lambda: eng.guardian(ex, args.save_level, act, st, applied, info, 0, 0, prev_flags=eng.flags, obs=obs),
                        guardian_legacy=lambda: eng.guardian(ex_legacy, args.save_level, act, st, applied, info, 0, 0, prev_flags=eng.flags, obs=obs))
            if args.what == "trace":
                for _ in range(args.launches):
                    for run in runs.values():
                        run()
                torch.cuda.synchronize()
                out.update(launches_per_form=args.launches)
            else:
                us = {k: [] for k in runs}
                for run in runs.values():
                    for _ in range(50):
                        run()
                for _ in range(args.windows):
                    for k, run in runs.items():
                        us[k].append(window_us(run, args.launches))
                out.update(windows=args.windows, launches_per_window=args.launches, windows_us=us,
                           us_per_call={k: statistics.median(v) for k, v in us.items()}, spread_us={k: (min(v), max(v)) for k, v in us.items()})
        else:
            def iteration(guard, t):
                eng.mlp_actor_critic(pw, vw, act, lp, val, 0, t)
                if guard:
                    eng.guardian(ex_legacy, args.save_level, act, st, applied, info, 1, t, prev_flags=eng.flags)
                eng.step(applied if guard else act)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            graphs = {}
            with torch.cuda.stream(s):
                for guard in (False, True):
                    for t in range(8):
                        iteration(guard, t)
            torch.cuda.synchronize()
            for name, guard in (("loop", False), ("loop_guardian", True)):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    for t in range(args.unroll):
                        iteration(guard, t)
                graphs[name] = g
            torch.cuda.synchronize()
            us = {k: [] for k in graphs}
            with torch.cuda.stream(s):
                for g in graphs.values():
                    for _ in range(5):
                        g.replay()
                for _ in range(args.windows):
                    for k, g in graphs.items():
                        us[k].append(window_us(g.replay, args.replays) / args.unroll)
            out.update(windows=args.windows, replays_per_window=args.replays, unroll=args.unroll, windows_us=us,
                       us_per_iteration={k: statistics.median(v) for k, v in us.items()}, spread_us={k: (min(v), max(v)) for k, v in us.items()},
                       takeover_share=float(((info & 1) != 0).float().mean()))
            del graphs
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
