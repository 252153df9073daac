"""What the guided gradient costs beside the plain one: pgd_ppo_grad_guided next to pgd_ppo_grad on the same
rollout of 4096 envs x 128 steps (274 inputs, actor and critic), split in 4 strided minibatches of 131072 rows.

    python tools/guided_cost.py [--envs 4096] [--T 128] [--windows 7] [--passes 3]
    python tools/guided_cost.py --cost       (three networks: pgd_ppo_grad_cost and the guided call with a cost critic)

Forms: plain; guided with 0 %, 25 % and 100 % of the rows guided by a mask (targets are read only where the bit is set).  One pass = the
four minibatch calls back to back on the engine's stream; a window = `--passes` passes between two HIP events; the forms take their
windows in turns.  Microseconds per minibatch call: the median window and the spread.  Prints one JSON line, stamped with the library's
source stamp (pgd_source_sha)."""
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

H = 256


def network(k, heads, rng):
    w = [rng.normal(0, k ** -0.5, (k, H)), np.zeros(H), rng.normal(0, 1 / 16, (H, H)), np.zeros(H), rng.normal(0, 1 / 16, (H, heads)), np.zeros(heads)]
    if heads == 4:
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
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--cost", action="store_true")
    args = ap.parse_args()
    descs = bank.get_descriptions(range(1000, 1004))
    mb = mapdata.MapBank(descs)
    sb = scenario.ScenarioBank(descs, [d["seed"] for d in descs], num_agents=1, num_traffic=0)
    eng = Engine(_abi.make_config(1, num_agents=1, num_traffic=0, num_lasers=0, seed=2), mb, sb)  # (its device and stream are all the update needs)
    D, n, n_mb = 274, args.envs * args.T, args.minibatches
    rng = np.random.default_rng(0)
    pw, vw, cw = network(D, 4, rng), network(D, 1, rng), network(D, 1, rng)
    zeros = lambda ws: [torch.zeros_like(w) for w in ws]  # noqa: E731
    pg, vg, cg = zeros(pw), zeros(vw), zeros(cw)
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g)  # noqa: E731
    obs, act, adv, ret, cret = rnd(n, D).clamp_(-3, 3), 0.4 * rnd(n, 2), rnd(n), rnd(n), rnd(n)
    logp = torch.zeros(n, device="cuda")
    target = torch.cat([0.4 * rnd(n, 2), torch.full((n, 2), float("nan"), device="cuda")], dim=1).contiguous()  # stride 4, as guardian_trace
    masks = {"guided_0": torch.zeros(n, dtype=torch.uint8, device="cuda"),
             "guided_25": (torch.rand(n, device="cuda", generator=g) < 0.25).to(torch.uint8),
             "guided_100": torch.ones(n, dtype=torch.uint8, device="cuda")}
    rows = -(-n // n_mb)
    need = eng.ppo_cost_work_bytes(D, rows) if args.cost else eng.ppo_work_bytes(D, rows)
    work = torch.empty(need // 4 + 1, device="cuda")
    st8, st12 = torch.zeros(8, device="cuda"), torch.zeros(12, device="cuda")
    with torch.no_grad():  # logp_old of the policy itself, so that the ratios are around 1
        h = torch.tanh(torch.tanh(obs @ pw[0] + pw[1]) @ pw[2] + pw[3]) @ pw[4] + pw[5]
        z = (act - h[:, :2]) * torch.exp(-h[:, 2:4])
        logp.copy_(-0.5 * (z * z).sum(dim=1) - h[:, 2:4].sum(dim=1) - float(np.log(2 * np.pi)))
        del h, z

    def plain(j):
        if args.cost:
            eng.ppo_grad_cost(pw, vw, cw, pg, vg, cg, obs, act, logp, adv, ret, cret, st8, work, start=j, stride=n_mb, rows=rows)
        else:
            eng.ppo_grad(pw, vw, pg, vg, obs, act, logp, adv, ret, st8, work, start=j, stride=n_mb, rows=rows)

    def guided(mask):
        cost = dict(cost_weights=cw, cost_grads=cg, cost_ret=cret) if args.cost else {}
        return lambda j: eng.ppo_grad_guided(pw, vw, pg, vg, obs, act, logp, adv, ret, st12, work, target, mask=mask, start=j, stride=n_mb,
                                             rows=rows, **cost)

    forms = dict(plain=plain, **{k: guided(m) for k, m in masks.items()})
    runs = {k: (lambda f=f: [f(j) for j in range(n_mb)]) for k, f in forms.items()}
    share = {}
    for k, run in runs.items():  # warm up, and what the last minibatch saw
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        share[k] = None if k == "plain" else float(st12[8] / st12[0])
    us = {k: [] for k in runs}
    for _ in range(args.windows):
        for k, run in runs.items():
            us[k].append(window_us(run, args.passes) / n_mb)
    out = dict(tool="guided_cost", pgd_source_sha=eng.L.pgd_source_sha().decode(), device=torch.cuda.get_device_name(0), timing="HIP events",
               networks=3 if args.cost else 2, rows=n, in_dim=D, minibatches=n_mb, rows_per_call=rows, windows=args.windows,
               calls_per_window=args.passes * n_mb, guided_share_last_minibatch=share, windows_us=us,
               us_per_call={k: statistics.median(v) for k, v in us.items()}, spread_us={k: (min(v), max(v)) for k, v in us.items()})
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
