"""Time of pgd_render_topdown (env.render(mode="top_down")) for 8 and 64 PGDrive-v0 envs at 1000 x 1000.

    python tools/render_time.py [--out DIR] [--iters 50]      (DIR: where rocprofv3 writes; default a temporary directory)

For each env count a child process renders 20 driven frames (the trails fill) and then `iters` back-to-back frames of every env
under `rocprofv3 --kernel-trace --stats`; the kernel times are the averages over the last `iters` dispatches of each render kernel
(rocprofv3's database, or its kernel statistics CSV).  The write bound is n x W x H x 3 bytes over the HBM write rate the top-down
observation kernel reaches (4.4 TB/s).  A second child without the profiler times a whole call with events
(prep + frame kernel + the gap between them).  Prints one JSON line per env count.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRITE_TBPS = 4.4


def inner(n, iters, film):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pgdrive_amd import PGDriveVecEnv
    env = PGDriveVecEnv(dict(num_envs=n, start_seed=1000, environment_num=100))
    env.reset()
    rng = np.random.default_rng(0)
    for t in range(20):  # trails of a few frames
        a = np.stack([rng.normal(0.0, 0.1, n), rng.uniform(0.3, 1.0, n)], axis=1).astype(np.float32)
        env.step(torch.from_numpy(a).cuda())
        env.render(mode="top_down", film_size=(film, film))
    eng = env.engine
    out = torch.empty((n, film, film, 3), dtype=torch.uint8, device=eng.device)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        eng.render_topdown(out=out)
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps(dict(envs=n, call_us=e0.elapsed_time(e1) * 1e3 / iters)))
    env.close()


def kernel_stats(d, last):
    """{kernel name: average duration [us] of its last `last` dispatches}."""
    rows = {}
    for p in glob.glob(os.path.join(d, "**", "*.db"), recursive=True):
        import sqlite3
        con = sqlite3.connect(p)
        names = [r[0] for r in con.execute("select distinct name from kernels where name like '%k_render%'")]
        for nm in names:
            dur = [r[0] for r in con.execute("select duration from kernels where name = ? order by start", (nm, ))][-last:]
            rows[nm] = sum(dur) / len(dur) / 1e3
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):  # (older rocprofv3: statistics only, all calls)
        with open(p) as f:
            for r in csv.DictReader(f):
                rows.setdefault(r["Name"], float(r["AverageNs"]) / 1e3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--envs", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--film", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        import tempfile
        args.out = tempfile.mkdtemp(prefix="render_time_")
    if args.inner:
        inner(args.envs[0], args.iters, args.film)
        return
    for n in args.envs:
        d = os.path.join(args.out, "n%d" % n)
        os.makedirs(d, exist_ok=True)
        plain = subprocess.run([sys.executable, __file__, "--inner", "--envs", str(n), "--iters", str(args.iters), "--film", str(args.film)],
                               capture_output=True, text=True, timeout=600)
        call = json.loads(plain.stdout.strip().splitlines()[-1]) if plain.returncode == 0 else dict(error=plain.stderr[-2000:])
        prof = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "render", "--", sys.executable, __file__, "--inner",
                               "--envs", str(n), "--iters", str(args.iters), "--film", str(args.film)], capture_output=True, text=True,
                              timeout=600)
        render_k = {k: v for k, v in (kernel_stats(d, args.iters) if prof.returncode == 0 else {}).items() if "k_render" in k}
        bound_us = n * args.film * args.film * 3 / (WRITE_TBPS * 1e12) * 1e6
        frame = [v for k, v in render_k.items() if "k_render_frame" in k]
        print(json.dumps(dict(envs=n, film=args.film, write_bytes=n * args.film * args.film * 3, write_bound_us=round(bound_us, 2),
                              kernels_us={k.split("(")[0]: round(v, 2) for k, v in render_k.items() if "k_render_bg" not in k},
                              frame_over_bound=round(frame[0] / bound_us, 2) if frame else None,
                              call_us=call.get("call_us"), profiler_rc=prof.returncode,
                              error=call.get("error") or (prof.stderr[-1500:] if prof.returncode else None))), flush=True)


if __name__ == "__main__":
    main()
