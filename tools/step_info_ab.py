"""A/B of the step with and without step info (include/pgdrive_hip.h pgd_step_info), bench.py's protocol in one process:

    python tools/step_info_ab.py [--steps 30000] [--warmup 10000] [--envs 4096]

The metric's workload (4096 envs x (1 ego + 16 traffic slots) x 240 beams, PGDrive-v0 maps 1000..1099, uniform(-1, 1) actions from a
ring of 64 pre-generated steps, auto-reset), 10 k warm-up steps, then for each of three forms the median of three timed windows,
microseconds per step with the launches left back to back:
    plain      pgd_step
    info       pgd_step with the step info on (k_step + k_step_info)
    empty      one empty launch of k_step_info's shape (pgd_step_info_empty_launch): the floor an extra launch cannot go below
The forms take turns window by window (plain, info, empty, plain, ...), so drift of the clocks hits all of them alike; the engine is
the same one throughout (enable / disable between the windows), its state runs on.  Prints one JSON line, stamped with the
library's source stamp (pgd_source_sha).  k_step_info's own time comes from a separate `rocprofv3 --kernel-trace --stats -- python
tools/step_info_ab.py --steps 3000 --warmup 1000` run (the program after `--`)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgdrive_amd import _abi, bank, mapdata, scenario  # noqa: E402
from pgdrive_amd.engine import Engine, _chk  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30000, help="timed steps per form, split into three windows")
    ap.add_argument("--warmup", type=int, default=10000)
    ap.add_argument("--maps", type=int, default=100)
    args = ap.parse_args()
    n = args.envs
    descs = bank.get_descriptions(range(1000, 1000 + args.maps))
    mb = mapdata.MapBank(descs)
    sb = scenario.ScenarioBank(descs, [d["seed"] for d in descs], num_agents=1, num_traffic=16)
    eng = Engine(_abi.make_config(n, auto_reset=1, seed=1234), mb, sb)
    eng.reset(np.arange(n) % len(descs))
    ring = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, size=(64, n, 1, 2)).astype(np.float32)).to(eng.device)
    tick = [0]

    def steps(k, empty=False):
        for _ in range(k):
            if empty:
                _chk(eng.L.pgd_step_info_empty_launch(eng.h), "pgd_step_info_empty_launch")
            else:
                eng.step(ring[tick[0] % 64])
                tick[0] += 1

    def window(k, empty=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(k, empty)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e6

    steps(args.warmup)
    plain_name = None
    per = max(1, args.steps // 3)
    us = dict(plain=[], info=[], empty=[])
    for _ in range(3):
        us["plain"].append(window(per))
        plain_name = plain_name or eng.describe_step()
        eng.enable_step_info()
        steps(64)  # (the first launches of a kernel load its code)
        us["info"].append(window(per))
        info_name = eng.describe_step()
        stats = eng.episode_stats()
        eng.disable_step_info()
        us["empty"].append(window(per, empty=True))
    med = {k: float(np.median(v)) for k, v in us.items()}
    print(json.dumps(dict(
        tool="step_info_ab", pgd_source_sha=eng.L.pgd_source_sha().decode(), envs=n, steps_per_window=per, warmup=args.warmup,
        us_per_step=med, windows_us=us, info_minus_plain_us=med["info"] - med["plain"], plain_plus_empty_us=med["plain"] + med["empty"],
        plain_plus_two_empty_us=med["plain"] + 2 * med["empty"], plain_kernel=plain_name, info_kernel=info_name,
        episodes_last_info_window=stats["episodes"], device=torch.cuda.get_device_name(0))))
    eng.close()


if __name__ == "__main__":
    main()
