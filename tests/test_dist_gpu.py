"""The N > 1 path with the REAL engine (GPU box has one GPU: the ranks share it; gloo carries the collective):
pgd_step_packed rows, the per-step gather of pgdrive_amd/dist.py as bench.py drives it, and bench.py's own rank spawning."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from pgdrive_amd import _abi
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_rows_equal_the_plain_outputs(descs):
    """pgd_step_packed writes [A*D obs | A reward | A done] per env, bit-identical to pgd_step's three arrays; a wider
    row stride leaves the padding untouched.  Single-agent (fused observation) and multi-agent (stand-alone k_observe)."""
    import torch
    from pgdrive_amd.engine import Engine
    for marl in (False, True):
        if marl:
            d, mb, sb = util.make_marl_banks(num_agents=4, n_variants=4, seed=3)
            cfg = util.marl_config(32, sb)
            n_scen = len(sb.scenarios)
        else:
            mb, sb = util.make_banks(descs, n_maps=4)
            cfg = _abi.make_config(32, num_lasers=240)
            n_scen = 4
        a, b = Engine(cfg, mb, sb), Engine(cfg, mb, sb)
        ids = np.arange(32) % n_scen
        a.reset(ids)
        b.reset(ids)
        A, D = a.A, a.D
        W = A * (D + 2) + 5
        rows = torch.full((32, W), -7.0, dtype=torch.float32, device=a.device)
        rng = np.random.default_rng(3)
        n_done = 0
        for t in range(150):
            act = torch.from_numpy(util.driving_actions(rng, 32, A)).to(a.device)
            o, r, dn, fl = a.step(act)
            _, r2, dn2, fl2 = b.step_packed(act, rows)
            a.sync()
            b.sync()
            assert torch.equal(rows[:, :A * D].reshape(32, A, D), o)
            assert torch.equal(rows[:, A * D:A * D + A], r) and torch.equal(r2, r)
            assert torch.equal(rows[:, A * D + A:A * D + 2 * A] > 0.5, dn > 0) and torch.equal(dn2, dn) and torch.equal(fl2, fl)
            assert (rows[:, A * (D + 2):] == -7.0).all()
            n_done += int(dn.sum())
        assert n_done > 0
        a.close()
        b.close()


def _worker(rank, world, port, n_total, steps, transport, q, backend="gloo"):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from pgdrive_amd import bank, mapdata, scenario
    from pgdrive_amd import dist as pdist
    from pgdrive_amd.engine import Engine
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    on = world > 1 or backend == "nccl"
    if on:
        kw = dict(device_id=torch.device("cuda", 0)) if backend == "nccl" else {}
        dist.init_process_group(backend, rank=rank, world_size=world, **kw)
    descs = bank.get_descriptions(range(1000, 1004))
    mb = mapdata.MapBank(descs)
    sb = scenario.ScenarioBank(descs, [d["seed"] for d in descs], num_traffic=16)
    lo, hi = pdist.shard_range(n_total, rank, world)
    n = hi - lo
    cfg = _abi.make_config(n, num_traffic=16, num_lasers=240, seed=5, env_base=lo)  # RNG streams keyed by the GLOBAL env index
    eng = Engine(cfg, mb, sb, device=0)
    eng.reset(pdist.scenario_ids_for(lo, hi, 4))
    g = pdist.StepGather(torch, dist if on else None, n, eng.D, eng.A, device=eng.device, transport=transport,
                         engine_lib=eng.L, exchange_when_alone=backend == "nccl")
    if backend == "nccl":
        assert g.transport == transport and g.backend == "nccl" and "RCCL" in g.describe()
    rng = np.random.default_rng(0)
    outs = []
    with torch.cuda.stream(eng.stream):
        for t in range(steps):
            a = rng.normal(0.0, 0.3, size=(n_total, 1, 2)).astype(np.float32)  # full throttle, noisy steering: episodes end soon
            a[..., 1] = 1.0
            act = torch.from_numpy(a[lo:hi].copy()).to(eng.device)
            b = g.step(lambda rows: eng.step_packed(act, rows))
            obs, rew, done = g.result(b)
            torch.cuda.synchronize()
            outs.append((obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), done.cpu().numpy().copy()))
    if rank == 0:
        q.put(outs)
    g.close()
    if on:
        dist.barrier()
        dist.destroy_process_group()
    eng.close()


def _run_world(world, n_total, steps, transport, port, backend="gloo"):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_total, steps, transport, q, backend)) for r in range(world)]
    for p in procs:
        p.start()
    res = q.get(timeout=500)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


@pytest.mark.timeout(900)
@pytest.mark.parametrize("transport", ["root", "collective", "peer"])
def test_two_rank_engine_gather_matches_single_process(transport):
    """Two processes, each with its own engine over half of the envs (sharing the box's one GPU), exchange packed rows every
    step through StepGather -- the code path of `bench.py --gpus 2` -- and rank 0 sees exactly the rows one process
    computes for all envs.  Envs are independent and the device RNG streams are keyed by the global env index
    (pgd_config.env_base), so the comparison is bit-exact."""
    n_total, steps = 64, 200
    one = _run_world(1, n_total, steps, "collective", 29711)
    two = _run_world(2, n_total, steps, transport, dict(root=29717, collective=29713, peer=29715)[transport])
    n_done = 0
    for (o1, r1, d1), (o2, r2, d2) in zip(one, two):
        assert o1.shape == o2.shape == (n_total, 1, 274)
        assert np.array_equal(o1, o2) and np.array_equal(r1, r2) and np.array_equal(d1, d2)
        n_done += int(d1.sum())
    assert n_done > 0


@pytest.mark.timeout(900)
@pytest.mark.parametrize("transport", ["collective", "root"])
def test_rccl_executes_the_step_exchange_on_one_rank(transport):
    """The box has one GPU and RCCL refuses two ranks on one device, so the most that can run here is a world of ONE rank with
    backend "nccl": communicator set-up bound to the device, the in-place all_gather_into_tensor / the gather to rank 0 launched
    by RCCL after every k_step on the engine's stream, double-buffered as in the N > 1 bench.  Rows must equal the engine's own."""
    n_total, steps = 64, 60
    one = _run_world(1, n_total, steps, "collective", 29721)
    rccl = _run_world(1, n_total, steps, transport, dict(collective=29723, root=29725)[transport], backend="nccl")
    for (o1, r1, d1), (o2, r2, d2) in zip(one, rccl):
        assert np.array_equal(o1, o2) and np.array_equal(r1, r2) and np.array_equal(d1, d2)


@pytest.mark.timeout(900)
def test_bench_spawns_its_own_ranks():
    """`python bench.py --gpus 2` without a launcher starts two ranks itself, reports n_gpus = 2 and both modes."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--oversubscribe", "--backend", "gloo",
                          "--exact", "--steps", "192", "--warmup", "8", "--envs", "256", "--no-cpu-baseline", "--full"],
                         capture_output=True, text=True, timeout=800, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["steps"] == 192 and d["steps_timed"] == 192
    assert d["value_mode"].startswith("gather:") and d["value"] == d["value_gather"] and d["value_replicas"] > 0
    # the default N > 1 run times EVERY transport in the one invocation; the headline is the best one whose self-check passed
    t = d["value_by_transport"]
    assert set(t) == {"root", "root+graph", "peer+graph", "collective", "peer", "collective+graph"}
    assert d["transport_chosen"] in t and t[d["transport_chosen"]]["value"] == d["value"]
    assert d["value"] == max(e["value"] for e in t.values() if e.get("gather_ok"))
    for name in ("root", "peer+graph", "collective", "peer"):
        assert t[name]["gather_ok"] is True and t[name]["value"] > 0 and t[name]["host_enqueue_us_per_step"] > 0, (name, t[name])
        assert len(t[name]["windows"]) == 3 and t[name]["model_ceiling_env_steps_per_s"] > 0
    for name in ("root+graph", "collective+graph"):  # gloo's collectives run on the host: no capture (RCCL: captured, see the one-rank test)
        assert "cannot be captured" in t[name]["error"] and "value" not in t[name]
    assert t["peer+graph"]["hip_graph_steps_per_replay"] == 64 and t["peer"]["hip_graph_steps_per_replay"] is None
    assert d["gather_mem"] in ("fine", "coarse") and t["peer"]["gather_mem"] == d["gather_mem"]
    assert d["config"]["global_envs"] == 512 and t[d["transport_chosen"]]["describe"] in d["config"]["parallelism"]
    assert len(d["windows"]) == 3 and d["window_spread"] >= 0 and len(d["windows_replicas"]) == 3
    assert d["roofline"]["k_step_ms"] > 0  # measured in the replicas pass (--full)
    # the exchange checks itself after the timed loop and the line carries what bounds it by construction
    assert d["gather_ok"] is True and d["gather_check"]["ranks_checked"] == 2 and d["gather_check"]["mismatched_ranks"] == []
    m = d["gather_model"]
    assert m["slice_bytes_per_rank_per_step"] == 256 * 276 * 4 and m["link_bound_us"] > 0 and m["host_enqueue_us_per_step"] > 0
    assert m["predicted_floor_us_per_step"] >= m["link_bound_us"]


@pytest.mark.timeout(1200)
def test_bench_world_8_under_the_drivers_launcher():
    """The driver's own command form -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1
    --master-port P bench.py --gpus 8 --steps K --warmup W`, no transport flag -- with the eight ranks sharing the one GPU of the
    test box (gloo for the collectives, HIP IPC for the peer transport): rendezvous, env sharding by rank, and EVERY transport's
    pass at world 8 in the one invocation, each with its self-check, host enqueue time and model ceiling."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    port = 29600 + (os.getpid() % 200)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "192", "--warmup", "20",
                          "--oversubscribe", "--backend", "gloo", "--exact", "--envs", "512", "--no-rows",
                          "--no-cpu-baseline"], capture_output=True, text=True, timeout=1100, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "rank 0 alone prints, one line"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["steps"] == 192 and d["warmup"] == 20 and d["scaling"] == "weak" and "aborted" not in d
    assert d["config"]["global_envs"] == 8 * 512 and d["config"]["envs_per_gpu"] == 512
    assert d["value_mode"].startswith("gather:") and d["value"] > 0 and d["value_replicas"] > 0
    t = d["value_by_transport"]
    assert list(t) == ["root", "root+graph", "collective", "collective+graph", "peer+graph", "peer"]  # (RCCL first, see bench.py)
    for name in ("root", "peer+graph", "collective", "peer"):  # the four that can run on this box
        e = t[name]
        assert e["gather_ok"] is True and e["gather_check"]["ranks_checked"] == 8 and e["gather_check"]["mismatched_ranks"] == [], (name, e)
        assert e["value"] > 0 and e["host_enqueue_us_per_step"] > 0 and e["model_ceiling_env_steps_per_s"] > 0 and e["xgmi_bound_us_per_step"] > 0
    # 7 slices through every link for the ring, one slice per link for the direct transports
    assert abs(t["collective"]["xgmi_bound_us_per_step"] / t["root"]["xgmi_bound_us_per_step"] - 7.0) < 1e-6
    for name in ("root+graph", "collective+graph"):  # named, with the reason (gloo runs on the host; under RCCL they are captured)
        assert "error" in t[name] and "value" not in t[name]
    # (one launch per 64 steps against several per step: normally 1 - 2 us against 30 - 120 us of host time per step.  Printed, not
    # asserted: eight ranks share this box's 16 CPUs with their launcher, and a replay behind a descheduled rank has read 122 us)
    print("host enqueue per step: peer+graph %.1f us, peer %.1f us" % (t["peer+graph"]["host_enqueue_us_per_step"], t["peer"]["host_enqueue_us_per_step"]))
    # ... and a generous bound that a broken replay path (a graph re-instantiated or re-captured per step) would still trip
    # (the strict comparison had to go, a bound need not)
    assert t["peer+graph"]["host_enqueue_us_per_step"] <= max(2.0 * t["peer"]["host_enqueue_us_per_step"], 250.0)
    assert d["gather_ok"] is True and d["transport_chosen"] in t and d["gather_mem"] in ("fine", "coarse")
    assert d["value"] == max(e["value"] for e in t.values() if e.get("gather_ok"))


@pytest.mark.timeout(900)
def test_bench_gather_in_a_hip_graph():
    """`bench.py --gpus 2 --transport peer --graph`: the gather pass replays one HIP graph per 64-step action cycle on every rank (the
    timed steps must be whole cycles: a shorter graph would replay another workload than the eager passes); the
    self-check after the timed loop passes and the line says how the steps were launched."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--oversubscribe", "--backend", "gloo",
                          "--exact", "--steps", "384", "--warmup", "8", "--envs", "256", "--no-cpu-baseline", "--transport", "peer", "--graph"],
                         capture_output=True, text=True, timeout=800, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["value_mode"] == "gather:peer+graph" and d["gather_ok"] is True
    assert list(d["value_by_transport"]) == ["peer+graph"]
    assert d["gather_model"]["hip_graph_steps_per_replay"] == 64
    assert "direct peer writes" in d["config"]["parallelism"]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("transport", ["root", "collective"])
def test_bench_gather_self_check_sees_a_damaged_row(transport):
    """A transport that delivers wrong rows must not print a clean line: one value of the received rows is changed before the
    self-check (--corrupt-gather) and `gather_ok` reads false, naming the rank whose slice differs."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--oversubscribe", "--backend", "gloo",
                          "--exact", "--steps", "16", "--warmup", "8", "--envs", "128", "--no-cpu-baseline", "--mode", "gather",
                          "--transport", transport, "--corrupt-gather"],
                         capture_output=True, text=True, timeout=800, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["gather_ok"] is False and d["gather_check"]["mismatched_ranks"] == [1]


def test_bench_default_run_is_steady_state_and_reproducible_from_events():
    """--warmup 5 still pre-rolls the floor, exactly --steps steps are timed (three windows of 4096), and under --full the roofline
    time comes from >= 64 event groups."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "12288", "--warmup", "5", "--full",
                          "--no-cpu-baseline", "--rows", "c3_respawn,c5_8x72"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == 12288 and d["warmup"] == 5 and d["steps_timed"] == 12288 and d["warmup_run"] >= 1500
    assert d["n_gpus"] == 1 and d["roofline"]["events"] >= 64
    # launch-to-launch time (wall / steps) and the event time of the kernel agree: same workload phase
    assert abs(d["ms_per_step"] - d["roofline"]["k_step_ms"]) < 0.15 * d["ms_per_step"]
    # `frac` is the contract's figure (algorithmic bytes / kernel time / peak); `frac_moved` charges the bytes that moved (counter pass
    # of this workload or the driving vehicles' records) and is never more; the line says what binds and carries the issue figure
    r = d["roofline"]
    assert 0 < r["frac_moved"] <= r["frac"] < 1 and r["frac"] == r["frac_nominal"] and r["moved_source"]
    assert abs(r["achieved"] - r["bytes_per_launch"] / (r["k_step_ms"] * 1e-3) / 1e9) < 1e-6 * r["achieved"]
    assert r["bound"] in ("hbm", "issue", "latency")
    if r["issue"] is not None:  # (a committed SQ_INSTS_* pass of the workload + the issue-rate table)
        i = r["issue"]
        assert i["insts_per_wave"] > 500 and 0 < i["frac"] < 1.5 and abs(i["bound_us"] - i["waves_per_simd"] * i["insts_per_wave"] * i["ns_per_inst_per_simd"] * 1e-3) < 1e-6
    # three windows, the median is the value
    assert len(d["windows"]) == 3 and sorted(d["windows"])[1] == d["value"] and 0 <= d["window_spread"] < 0.2
    # the loaded rows of the same invocation: their own workload, kernel time and roofline
    rows = {x["row"]: x for x in d["rows"]}
    assert set(rows) == {"c3_respawn", "c5_8x72"} and all("error" not in x for x in rows.values())
    assert "traffic mode respawn" in rows["c3_respawn"]["workload"] and rows["c3_respawn"]["driving_traffic_mean"] > 5
    assert rows["c3_respawn"]["roofline"]["k_step_ms"] > r["k_step_ms"]  # every traffic vehicle drives: a heavier step
    assert rows["c5_8x72"]["workload"].startswith("C5: 4096 envs/GPU x 8 agents") and rows["c5_8x72"]["active_agents_mean"] > 1
    assert all(0 < x["roofline"]["frac_moved"] <= x["roofline"]["frac"] for x in rows.values())
    assert all(len(x["windows"]) == 3 for x in rows.values())


def test_bench_plain_run_times_the_headline_only_and_dumps_reproducible_outputs(tmp_path):
    """Without --full the line carries the headline alone (no rows, CPU baseline, roofline or work statistics), times exactly
    --steps steps, and --dump-outputs writes what the last timed step returned -- the same arrays on a second run."""
    lines = []
    for run in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "300", "--warmup", "5",
                              "--dump-outputs", str(tmp_path / run)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines.append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]))
    d = lines[0]
    assert d["steps"] == d["steps_timed"] == 300 and d["warmup"] == 5 and d["warmup_run"] >= 1500 and len(d["windows"]) == 3
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["n_gpus"] == 1
    assert abs(d["value"] - 4096 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"] and sorted(d["windows"])[1] == d["value"]
    assert "rows" not in d and d["cpu_baseline"] is None and d["roofline"] is None and "driving_traffic_mean" not in d["config"]
    assert d["outputs_written"] == ["done", "flags", "obs", "reward"]
    shapes = dict(obs=(4096, 1, 274), reward=(4096, 1), done=(4096, 1), flags=(4096, 1))
    for name, shape in shapes.items():
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.shape == shape and a.dtype == (np.float64 if name == "flags" else np.float32) and np.isfinite(a).all(), name
        assert np.array_equal(a, b), name
    assert np.abs(np.load(tmp_path / "a" / "obs.npy")).max() > 0


def _graph_worker(rank, world, port, n_total, cycle, n_cycles, q, use_graph):
    """`n_cycles` cycles of `cycle` steps with fixed per-position actions; rank 0 reports the rows of the last nbuf steps of every
    cycle.  use_graph: peer transport with device-side sequences, every cycle ONE graph replay; else eager steps."""
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from pgdrive_amd import bank, mapdata, scenario
    from pgdrive_amd import dist as pdist
    from pgdrive_amd.engine import Engine
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    descs = bank.get_descriptions(range(1000, 1004))
    mb = mapdata.MapBank(descs)
    sb = scenario.ScenarioBank(descs, [d["seed"] for d in descs], num_traffic=16)
    lo, hi = pdist.shard_range(n_total, rank, world)
    n = hi - lo
    cfg = _abi.make_config(n, num_traffic=16, num_lasers=240, seed=5, env_base=lo)
    eng = Engine(cfg, mb, sb, device=0)
    eng.reset(pdist.scenario_ids_for(lo, hi, 4))
    g = pdist.StepGather(torch, dist if world > 1 else None, n, eng.D, eng.A, device=eng.device, transport="peer", engine_lib=eng.L,
                         device_seq=use_graph)
    rng = np.random.default_rng(0)
    a = rng.normal(0.0, 0.3, size=(cycle, n_total, 1, 2)).astype(np.float32)
    a[..., 1] = 1.0
    acts = [torch.from_numpy(a[i, lo:hi].copy()).to(eng.device) for i in range(cycle)]  # static tensors: the graph keeps their addresses
    produces = [(lambda rows, t=t: eng.step_packed(t, rows)) for t in acts]
    outs = []
    with torch.cuda.stream(eng.stream):
        graph = g.capture_cycle(produces) if use_graph else None
        for c in range(n_cycles):
            if use_graph:
                graph.replay()  # (GraphCycle: launches the graph and moves the gatherer's step counter on)
            else:
                for pr in produces:
                    g.step(pr)
            last = []
            for j in range(g.nbuf):  # the buffers hold the last nbuf steps of the cycle
                b = (cycle - g.nbuf + j) % g.nbuf
                obs, rew, done = g.result(b)
                torch.cuda.synchronize()
                last.append((obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), done.cpu().numpy().copy()))
            outs.append(last)
        ok, detail = g.validate(produces[0])  # the eager path on the same handle, after the replays (a step of its own)
    if rank == 0:
        q.put((outs, ok, g.peer.status() if g.peer is not None else 0))
    g.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    eng.close()


@pytest.mark.timeout(900)
def test_peer_gather_cycle_in_one_hip_graph():
    """Device-side sequence numbers make the calls of a step identical every time: wait, release, pgd_step_packed and push of a
    whole cycle of steps (8 = 4 x nbuf) are captured in ONE HIP graph per rank and replayed; two ranks (sharing the box's GPU, HIP IPC
    between them) then deliver exactly the rows a single eager process computes, cycle after cycle -- flow control (acks), flags and
    double buffering included -- and the eager self-check still passes on the same handle afterwards."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    n_total, cycle, n_cycles = 64, 8, 6
    res = {}
    for world, use_graph, port in ((1, False, 29741), (2, True, 29743)):
        q = ctx.Queue()
        procs = [ctx.Process(target=_graph_worker, args=(r, world, port, n_total, cycle, n_cycles, q, use_graph)) for r in range(world)]
        for p in procs:
            p.start()
        res[world] = q.get(timeout=600)
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    (one, ok1, _), (two, ok2, status) = res[1], res[2]
    assert ok1 and ok2 and status == 0
    n_done = 0
    for c1, c2 in zip(one, two):
        for (o1, r1, d1), (o2, r2, d2) in zip(c1, c2):
            assert o1.shape == o2.shape == (n_total, 1, 274)
            assert np.array_equal(o1, o2) and np.array_equal(r1, r2) and np.array_equal(d1, d2)
            n_done += int(d1.sum())
    assert n_done > 0


def _rccl_graph_worker(port, transport, q):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from pgdrive_amd import bank, mapdata, scenario
    from pgdrive_amd import dist as pdist
    from pgdrive_amd.engine import Engine
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    descs = bank.get_descriptions(range(1000, 1004))
    mb = mapdata.MapBank(descs)
    sb = scenario.ScenarioBank(descs, [d["seed"] for d in descs], num_traffic=16)
    n = 128
    cfg = _abi.make_config(n, num_traffic=16, num_lasers=240, seed=5)
    eng, ref = Engine(cfg, mb, sb, device=0), Engine(cfg, mb, sb, device=0)
    eng.reset(np.arange(n) % 4)
    ref.reset(np.arange(n) % 4)
    g = pdist.StepGather(torch, dist, n, eng.D, eng.A, device=eng.device, transport=transport, engine_lib=eng.L, exchange_when_alone=True)
    rng = np.random.default_rng(0)
    acts = [torch.from_numpy(rng.uniform(-1, 1, size=(n, 1, 2)).astype(np.float32)).cuda() for _ in range(8)]
    with torch.cuda.stream(eng.stream):
        graph = g.capture_cycle([(lambda rows, t=t: eng.step_packed(t, rows)) for t in acts])
        for c in range(4):
            graph.replay()
        torch.cuda.synchronize()
        obs, rew, done = g.result(1)
    for c in range(4):
        for t in acts:
            o_ref, r_ref, d_ref, _ = ref.step(t)
    ref.sync()
    q.put((bool(torch.equal(obs[:n], o_ref)), bool(torch.equal(rew[:n], r_ref)), bool(torch.equal(done[:n], d_ref > 0)), g.describe()))
    g.close()
    eng.close()
    ref.close()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("transport", ["collective", "root"])
def test_rccl_exchange_captured_in_a_hip_graph_on_one_rank(transport):
    """`bench.py --graph` with the RCCL transports: torch captures the collective launched by RCCL together with pgd_step_packed --
    eight steps per graph, replayed four times in a world of one rank (all the box allows); the rows of the last step equal an
    eager engine's."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_graph_worker, args=(dict(collective=29751, root=29753)[transport], transport, q))
    p.start()
    same_obs, same_rew, same_done, desc = q.get(timeout=600)
    p.join(timeout=120)
    assert p.exitcode == 0
    assert same_obs and same_rew and same_done and "RCCL" in desc
