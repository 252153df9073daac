"""What episode_stats costs, at the benchmark configuration: 4096 envs x (1 ego + 16 traffic slots) x 240 beams,
274 inputs, PGDrive-v0 maps 1000..1099, auto-reset.

    python tools/rollout_episodes_cost.py collect [--forms off,on] [--T 128] [--windows 7] [--calls 3]
    python tools/rollout_episodes_cost.py kernel [--T 128] [--windows 5] [--launches 300]

collect: RolloutCollector.collect() with the switch off (today's calls: what the parent commit's collect() issues) and on, one collector
each on ONE engine, taking turns window by window so that drift hits both alike; 2 warm-up calls per form, then `--windows` windows of
`--calls` calls between two HIP events; the median window and the spread, microseconds per call.
kernel: Engine.rollout_episodes alone, calls back to back on the engine's stream, `--windows` windows of `--launches` calls between two
HIP events, microseconds per call, the forms taking turns window by window:
    ego, ego_dense      [T, 4096] rows, mode 0 (the rewards, dones and flags of a real rollout), without and with ep_return / ep_length
    seats, seats_dense  [T, 163840] rows (4096 envs x 40 seats), seats mode, on generated flags: an agent acts at 70 % of the entries, 2 %
                        of those end by done, 0.5 % of all entries carry PGD_F_RESET
    gae                 Engine.gae on the ego arrays, for scale
Under `rocprofv3 --kernel-trace --stats -- python tools/rollout_episodes_cost.py kernel ...` the trace gives the two kernels' own times.
Prints one JSON line, stamped with the library's source stamp (pgd_source_sha)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgdrive_amd import _abi, bank, mapdata, scenario  # noqa: E402
from pgdrive_amd.engine import Engine  # noqa: E402
from pgdrive_amd.rollout import RolloutCollector  # noqa: E402
from tools.return_norm_cost import networks, summary, window_us  # noqa: E402

SEATS = 40


def seat_arrays(T, rows, gen):
    """Generated step arrays of seats that change hands, on the device."""
    u = lambda: torch.rand((T, rows), device="cuda", generator=gen)  # noqa: E731
    acted = u() < 0.7
    done = (acted & (u() < 0.02)).to(torch.uint8)
    flags = torch.randint(0, 1 << 14, (T, rows), device="cuda", generator=gen, dtype=torch.int32)
    flags = flags | acted.to(torch.int32) * (1 << 17) | (u() < 0.005).to(torch.int32) * (1 << 16)
    reward = torch.randn((T, rows), device="cuda", generator=gen)
    return reward.masked_fill(~acted, float("nan")), done, flags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("collect", "kernel"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--maps", type=int, default=100)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--forms", default="off,on")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--launches", type=int, default=300)
    args = ap.parse_args()
    n = args.envs
    descs = bank.get_descriptions(range(1000, 1000 + args.maps))
    mb = mapdata.MapBank(descs)
    sb = scenario.ScenarioBank(descs, [d["seed"] for d in descs], num_agents=1, num_traffic=16)
    eng = Engine(_abi.make_config(n, auto_reset=1, seed=1234), mb, sb)
    eng.reset(np.arange(n) % len(descs))
    pw, vw = networks(eng.D, np.random.default_rng(0))
    out = dict(tool="rollout_episodes_cost", what=args.what, pgd_source_sha=eng.L.pgd_source_sha().decode(), envs=n, in_dim=eng.D, T=args.T,
               device=torch.cuda.get_device_name(0), timing="HIP events")
    with torch.no_grad():
        if args.what == "collect":
            forms = args.forms.split(",")
            cols = {f: RolloutCollector(eng, pw, vw, args.T, seed=0, **(dict(episode_stats=True) if f == "on" else {})) for f in forms}
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
                out.update(episode_summary=cols["on"].episode_summary())
        else:
            col = RolloutCollector(eng, pw, vw, args.T, seed=0)
            col.collect()
            batch = col.collect()
            ego = [batch[k].clone() for k in ("rewards", "dones", "flags")]
            value, adv, ret = batch["values"].clone(), torch.empty_like(ego[0]), torch.empty_like(ego[0])
            gen = torch.Generator(device="cuda")
            gen.manual_seed(0)
            seats = list(seat_arrays(args.T, n * SEATS, gen))
            runs, records = dict(gae=lambda: eng.gae(ego[0], value, ego[1], 0.99, 0.95, adv=adv, ret=ret)), {}
            for name, arrays, seated in (("ego", ego, False), ("seats", seats, True)):
                rows = arrays[0][0].numel()
                work = torch.empty(((eng.rollout_episodes_work_bytes(rows) + 7) // 8, ), dtype=torch.float64, device="cuda")
                dense = dict(ep_return=torch.empty_like(arrays[0]), ep_length=torch.empty_like(arrays[2]))
                for form, kw in ((name, {}), (name + "_dense", dense)):
                    rc, lc, record = eng.rollout_episodes_state(rows)
                    call = record.clone()
                    records[form] = record
                    runs[form] = (lambda a=arrays, rc=rc, lc=lc, record=record, call=call, seated=seated, kw=kw, work=work:
                                  eng.rollout_episodes(*a, rc, lc, record=record, call=call, seats=seated, work=work, **kw))
            for run in runs.values():
                for _ in range(50):
                    run()
            us = {k: [] for k in runs}
            for _ in range(args.windows):
                for k, run in runs.items():
                    us[k].append(window_us(run, args.launches))
            med, spread = summary(us)
            out.update(windows=args.windows, launches_per_window=args.launches, windows_us=us, us_per_call=med, spread_us=spread,
                       bytes_read_per_call=dict(ego=ego[0].numel() * 9, seats=seats[0].numel() * 9),
                       bytes_written_dense=dict(ego=ego[0].numel() * 8, seats=seats[0].numel() * 8),
                       records={k: dict(zip(_abi.ROLLOUT_EPISODES, v.cpu().tolist())) for k, v in records.items()})
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
