"""Step info on the device (include/pgdrive_hip.h pgd_step_info, pgdrive_amd/csrc/pgd_step_info.h): an engine with the step info on
computes what a plain engine computes, bit for bit, while the terminal row, the reference's info floats and the episode statistics
stay on the device.  64 envs (96 in throughput mode), at most 320 steps."""
import types

import numpy as np
import pytest

from pgdrive_amd import _abi
from tests import parity, util
from tests.parity import OBS_TOL, STATE_OBS_TOL, closed_engines  # noqa: F401 (the fixture closes every engine a test made)

pytestmark = pytest.mark.gpu

SF, EI = _abi.SF, _abi.EI
INFO_KEYS = tuple(_abi.STEP_INFO_FIELDS)
BASE = dict(horizon=40, auto_reset=1, resample_scenario=1, seed=2)
CASES = dict(
    c3=dict(),  # 16 traffic slots, 240 beams: the specialised instantiation
    c3_general=dict(num_lasers=72, num_traffic=12),
    ego_only=dict(num_traffic=0, num_lasers=0),  # four envs per wave
    pack=dict(),  # throughput mode (PGD_PACK=1), 96 envs
    objects=dict(num_traffic=30, accident_prob=0.8, density=0.05),
    lane_keep=dict(),  # stepped through step_lane_keep
    jit=dict(num_lasers=72, num_traffic=12),  # specialise() on both
)


def build(descs, case, n_envs, with_info=True, n_maps=8, **over):
    kw = dict(BASE, **CASES[case])
    kw.update(over)
    mb, sb, cfg = parity.banks_and_config(descs, n_envs, n_maps, **kw)
    eng = parity.engine(cfg, mb, sb, env=dict(PGD_PACK="1" if case == "pack" else None))
    if with_info:
        eng.enable_step_info(costs=(1.0, 0.5, 0.25))
    return eng, (cfg, mb, sb)


def host_cost(flags, costs=(1.0, 0.5, 0.25)):
    """PGDriveVecEnv.cost_from_flags (the rule of pgdrive_env.py:197-207) with the test's costs"""
    from pgdrive_amd.vec_env import PGDriveVecEnv
    env = types.SimpleNamespace(config=dict(out_of_road_cost=costs[0], crash_vehicle_cost=costs[1], crash_object_cost=costs[2]),
                                info_from_flags=lambda fl: PGDriveVecEnv.info_from_flags(None, fl))
    return PGDriveVecEnv.cost_from_flags(env, flags).astype(np.float32)


@pytest.mark.parametrize("case", list(CASES))
def test_step_info_engine_equals_the_plain_engine(descs, monkeypatch, tmp_path, case):
    """Twin A has the step info on (its step kernel never restarts an env, k_step_info does), twin B is plain; both run free on the same
    actions through >= 384 episode ends (64 envs x 240 steps / horizon 40).  Every step: reward, done, flags and the whole state are
    bit-identical; the rows of envs that did not restart are equal; the rows of restarted envs -- A's from the stand-alone row code,
    B's from the fused observation -- agree to 1e-6 with grazing beams counted (<= 1e-5 * beams + 2: the rule and the numbers of
    test_fused_observation_equals_stand_alone_kernels).  Both kinds of episode end must occur (the oracle's run of the c3 / ego_only
    inputs: 512 ends, 239 max_step, 276 out of road); the lane-keeping policy keeps its ego on the road, so that case asks for the
    time limit only."""
    import torch
    monkeypatch.setenv("PGD_JIT_DIR", str(tmp_path))
    n_envs = 96 if case == "pack" else 64
    a, _ = build(descs, case, n_envs)
    b, _ = build(descs, case, n_envs, with_info=False)
    if case == "jit":
        assert a.specialise(wait=True) is True and b.specialise(wait=True) is True
    ids = np.arange(n_envs) % 8
    a.reset(ids); b.reset(ids)
    actions = parity.driving_with_bursts(np.random.default_rng(8), n_envs)
    st = dict(beams=0, grazing=0, worst=0.0)
    n_done = n_max = n_oor = 0
    for t in range(240):
        if case == "lane_keep":
            outs_a = [x.clone() for x in a.step_lane_keep(t)]
            outs_b = [x.clone() for x in b.step_lane_keep(t)]
        else:
            at = torch.from_numpy(actions(t)).to(a.device)
            outs_a = [x.clone() for x in a.step(at)]
            outs_b = [x.clone() for x in b.step(at)]
        a.sync(); b.sync()
        parity.same_bits(t, outs_a[1:], outs_b[1:], a, b, names=parity.OUTPUTS[1:])
        restarted = (outs_b[3][:, 0] & _abi.F_RESET) != 0
        assert torch.equal(restarted, outs_b[2][:, 0] != 0)
        assert torch.equal(outs_a[0][~restarted], outs_b[0][~restarted]), "rows of running envs differ at step %d" % t
        if bool(restarted.any()):
            parity.rows_close(outs_a[0][restarted], outs_b[0][restarted], st, a.cfg.num_lasers, 1e-6)
        fl = outs_b[3][:, 0][restarted]
        n_done += int(restarted.sum())
        n_max += int(((fl & _abi.F_MAX_STEP) != 0).sum())
        n_oor += int(((fl & _abi.F_OUT_OF_ROAD) != 0).sum())
    print("step info vs plain", case, "ends", n_done, "max_step", n_max, "out_of_road", n_oor, "restarted rows: worst", st["worst"],
          "grazing", st["grazing"], "of", st["beams"], "|", a.describe_step())
    assert st["worst"] < 1e-6 and st["grazing"] <= 1e-5 * st["beams"] + 2
    assert n_done >= 384 and n_max > 0 and (n_oor > 0 or case == "lane_keep")
    assert "k_step_info" in a.describe_step() and "k_step_info" not in b.describe_step()
    assert a.describe_step().startswith(b.describe_step())
    if case == "jit":
        assert "at run time" in a.describe_step()
    assert int(a.step_info["ep_count"].sum()) == n_done


@pytest.mark.parametrize("case", ["c3", "pack"])
def test_final_observation_is_the_terminal_row(descs, case):
    """Twin B never restarts an env (auto_reset=0, no step info) and starts every step from A's state: its row of a finished env IS the
    terminal row.  Where done, A's final_obs row equals it bit for bit (the same instantiation on the same state); elsewhere final_obs
    keeps the NaN it was filled with.  Every info tensor of A equals the host formula on B's state and flags as bits; step_energy the
    fp32 difference to the energy of the state the step started from (0 after a restart); cost = cost_from_flags; total_cost its
    running fp32 sum.  Case c3 also holds the terminal rows to the fp64 oracle (>= 100 of them) through parity.compare_rows."""
    import torch
    n_envs = 96 if case == "pack" else 64
    a, (cfg, mb, sb) = build(descs, case, n_envs)
    b, (cfg_b, _, _) = build(descs, case, n_envs, with_info=False, auto_reset=0)
    ora = parity.oracle(cfg_b, mb, sb) if case == "c3" else None
    ids = np.arange(n_envs) % 8
    a.reset(ids); b.reset(ids)
    if ora is not None:
        ora.reset(ids)
    info = a.step_info
    info["final_observation"].fill_(float("nan"))
    keep = info["final_observation"].clone()
    rng = np.random.default_rng(8)
    pending = {}

    def actions(t):
        pending["act"] = parity.driving_with_bursts(rng, n_envs)(t)
        pending["state"] = a.get_state()  # what twins() copies into B right after this call
        if ora is not None:
            f, i, ei = pending["state"]
            ora.set_state(f.astype(np.float64), i, ei)
        return pending["act"]

    stats = parity.new_stats()
    total = np.zeros(n_envs, np.float32)
    base = np.zeros(n_envs, np.float32)
    n_done = n_oracle_rows = 0
    for t, outs_a, outs_b in parity.twins(a, b, 240, actions, copy_state=a):
        parity.same_bits(t, outs_a[1:3], outs_b[1:3], names=parity.OUTPUTS[1:3])
        done = outs_b[2][:, 0] != 0
        assert torch.equal(outs_a[3][:, 0], outs_b[3][:, 0] | (done.int() * _abi.F_RESET)), "flags differ at step %d" % t
        fin = info["final_observation"]
        assert torch.equal(fin[done].view(torch.int32), outs_b[0][done, 0].view(torch.int32)), "terminal rows differ at step %d" % t
        assert torch.equal(fin[~done].view(torch.int32), keep[~done].view(torch.int32)), "final_obs written where not done, step %d" % t
        keep = fin.clone()
        f, i, ei = b.get_state()  # the state the step ended in (B does not restart)
        fl = outs_b[3][:, 0].cpu().numpy().astype(np.uint32)
        dn = done.cpu().numpy()
        got = {k: info[k].cpu().numpy() for k in INFO_KEYS}
        cost = host_cost(fl)
        total = total + cost
        want = dict(velocity=np.abs(f[SF["SPEED"], :, 0]) * np.float32(3.6), steering=f[SF["STEER"], :, 0], acceleration=f[SF["ACT1T"], :, 0],
                    episode_energy=f[SF["ENERGY"], :, 0], step_energy=f[SF["ENERGY"], :, 0] - base, episode_reward=f[SF["EP_REWARD"], :, 0],
                    cost=cost, total_cost=total)
        for k, v in want.items():
            assert v.dtype == np.float32 and np.array_equal(got[k].view(np.int32), v.view(np.int32)), "%s differs at step %d" % (k, t)
        assert np.array_equal(got["episode_length"], ei[EI["EP_STEPS"]]), "episode_length differs at step %d" % t
        total = np.where(dn, np.float32(0), total)
        base = np.where(dn, np.float32(0), f[SF["ENERGY"], :, 0])
        n_done += int(dn.sum())
        if ora is not None:
            o_obs, o_rew, o_done, o_flags = ora.step(pending["act"])
            same = (o_flags == fl[:, None]) & (o_done == dn[:, None].astype(np.uint8)) & dn[:, None]
            n_oracle_rows += int(same.sum())
            g_obs = np.where(dn[:, None, None], fin.cpu().numpy().astype(np.float64)[:, None, :], 0.0)
            parity.compare_rows(b, ora, stats, g_obs, o_obs, same, ora.margins())
    assert n_done >= n_envs * 240 // 40
    if ora is not None:
        n_ties = stats.get("grazing", 0)
        print("terminal rows vs the oracle:", n_oracle_rows, "rows, worst", stats["obs"], "state columns", stats.get("obs_state"), "admitted beams", n_ties)
        parity.report("terminal rows", stats)
        assert n_oracle_rows >= 100
        # a beam over OBS_TOL is admitted only by the oracle's own geometry (parity.admit_beams), anything else stays in stats["obs"];
        # how many it may admit is bounded where the predicate itself is: 1 % of the beams (tests/test_ties_cpu.py)
        assert stats["obs"] < OBS_TOL and stats["obs_state"] < STATE_OBS_TOL and stats.get("beams_not_admitted", 0) == 0
        assert n_ties <= 0.01 * stats.get("beams", 0)


def test_total_cost_and_episode_statistics(descs):
    """SafePGDriveEnv's rules (crashes cost, they do not end the episode) with respawn traffic, horizon 80, 64 envs x 320 steps, costs
    1.0 / 0.5 / 0.25 (exact in fp32): total_cost of every step and the statistics at the end equal a host accumulation from the returned
    reward / done / flags -- counts and ep_cost_sum exactly, ep_return_sum bit-equal to the fp32 sum in the same order.  The oracle's
    run of these inputs: 261 ends (170 time limit, 105 out of road), 14,654 steps with a crash cost."""
    import torch
    n_envs = 64
    mb, sb, cfg = parity.banks_and_config(descs, n_envs, safe_rl_env=True, traffic_mode="respawn", horizon=80, auto_reset=1,
                                          resample_scenario=1, seed=2)
    eng = parity.engine(cfg, mb, sb)
    info = eng.enable_step_info(costs=(1.0, 0.5, 0.25))
    eng.reset(np.arange(n_envs) % 8)
    rng = np.random.default_rng(8)
    ret, total = np.zeros(n_envs, np.float32), np.zeros(n_envs, np.float32)
    length = np.zeros(n_envs, np.int32)
    want = dict(ep_count=np.zeros(n_envs, np.int32), ep_return_sum=np.zeros(n_envs, np.float32), ep_length_sum=np.zeros(n_envs, np.int32),
                ep_cost_sum=np.zeros(n_envs, np.float32), ep_arrive=np.zeros(n_envs, np.int32), ep_out_of_road=np.zeros(n_envs, np.int32),
                ep_crash=np.zeros(n_envs, np.int32), ep_max_step=np.zeros(n_envs, np.int32))
    n_cost_steps = n_done = 0
    for t in range(320):
        _, rew, done, flags = eng.step(torch.from_numpy(util.driving_actions(rng, n_envs)).to(eng.device))
        eng.sync()
        rew, dn = rew[:, 0].cpu().numpy(), done[:, 0].cpu().numpy() != 0
        fl = flags[:, 0].cpu().numpy().astype(np.uint32)
        cost = host_cost(fl)
        ret, total, length = ret + rew, total + cost, length + 1
        assert np.array_equal(info["total_cost"].cpu().numpy().view(np.int32), total.view(np.int32)), "total_cost differs at step %d" % t
        assert np.array_equal(info["cost"].cpu().numpy(), cost)
        n_cost_steps += int(((fl & (_abi.F_CRASH_VEHICLE | _abi.F_CRASH_OBJECT)) != 0).sum())
        n_done += int(dn.sum())
        want["ep_count"] += dn
        want["ep_return_sum"] = np.where(dn, want["ep_return_sum"] + ret, want["ep_return_sum"])
        want["ep_length_sum"] += np.where(dn, length, 0)
        want["ep_cost_sum"] = np.where(dn, want["ep_cost_sum"] + total, want["ep_cost_sum"])
        want["ep_arrive"] += dn & ((fl & _abi.F_ARRIVE) != 0)
        want["ep_out_of_road"] += dn & ((fl & _abi.F_OUT_OF_ROAD) != 0)
        want["ep_crash"] += dn & ((fl & (_abi.F_CRASH_VEHICLE | _abi.F_CRASH_OBJECT | _abi.F_CRASH_BUILDING)) != 0)
        want["ep_max_step"] += dn & ((fl & _abi.F_MAX_STEP) != 0)
        ret, total, length = np.where(dn, np.float32(0), ret), np.where(dn, np.float32(0), total), np.where(dn, 0, length)
    got = {k: info[k].cpu().numpy() for k in want}
    print("episode statistics: ends", n_done, "cost steps", n_cost_steps, {k: (v.sum().item()) for k, v in got.items()})
    assert n_done >= 100 and n_cost_steps >= 1000 and int(got["ep_count"].sum()) == n_done
    for k, v in want.items():
        assert got[k].dtype == v.dtype and np.array_equal(got[k].view(np.int32), v.view(np.int32)), k
    stats = eng.episode_stats(clear=True)
    assert stats["episodes"] == n_done
    assert abs(stats["mean_return"] - float(want["ep_return_sum"].astype(np.float64).sum()) / n_done) < 1e-9
    assert stats["mean_length"] == float(want["ep_length_sum"].sum()) / n_done
    assert stats["mean_cost"] == float(want["ep_cost_sum"].astype(np.float64).sum()) / n_done
    assert stats["max_step_rate"] == float(want["ep_max_step"].sum()) / n_done
    eng.sync()
    for k in want:
        assert not info[k].any(), k
    assert eng.episode_stats()["episodes"] == 0 and eng.episode_stats()["mean_return"] is None


def test_step_info_in_a_hip_graph_and_in_env_groups(descs):
    """A step with info is two launches in sequence on one stream: captured in a HIP graph it replays to the outputs and the info of
    eager stepping (the pattern of test_step_captured_in_a_hip_graph_matches_eager); and two env groups stepped alternately on their own
    streams equal one batch (test_env_groups_step_like_one_batch)."""
    import torch
    from pgdrive_amd import PGDriveVecEnv
    n = 64
    conf = dict(num_envs=n, seed=3, start_seed=1000, environment_num=8, horizon=40, step_info=True)
    eager, graphed = parity.closing(PGDriveVecEnv(conf)), parity.closing(PGDriveVecEnv(conf))
    eager.reset(force_seed=np.arange(n) % 8 + 1000)
    graphed.reset(force_seed=np.arange(n) % 8 + 1000)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    acts = torch.rand((90, n, 2), device="cuda", generator=gen) * 2 - 1
    acts[:, :, 1] = acts[:, :, 1].abs()
    a_static = torch.zeros((n, 2), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up on a side stream
        a_static.copy_(acts[0])
        graphed.step(a_static)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager.step(acts[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.step(a_static)
    torch.cuda.synchronize()
    eager.step(acts[0])  # the capture pass does not execute; replay it once to stay in step
    graph.replay()
    n_done = 0
    for k in range(1, 90):
        a_static.copy_(acts[k])
        graph.replay()
        o, r, d, f = eager.step(acts[k])
        torch.cuda.synchronize()
        assert torch.equal(o, graphed.engine.obs.view_as(o)) and torch.equal(r, graphed.engine.reward.view_as(r))
        assert torch.equal(d, graphed.engine.done.view_as(d)) and torch.equal(f, graphed.engine.flags.view_as(f))
        for key in INFO_KEYS + ("final_observation", ):
            assert torch.equal(eager.last_info[key], graphed.last_info[key]), "%s differs at replay %d" % (key, k)
        n_done += int(d.sum().item())
    assert n_done >= n * 89 // 40 - n and int(graphed.last_info["ep_count"].sum()) == int(eager.last_info["ep_count"].sum()) > 0

    a, _ = build(descs, "c3", n)
    b, _ = build(descs, "c3", n)
    ids = np.arange(n) % 8
    a.reset(ids); b.reset(ids)
    b.set_groups(2)
    a.step_info["final_observation"].fill_(0.0); b.step_info["final_observation"].fill_(0.0)
    actions = parity.driving_with_bursts(np.random.default_rng(8), n)
    n_done = 0
    for t in range(120):
        act = torch.from_numpy(actions(t)).to(a.device)
        outs = [x.clone() for x in a.step(act)]
        a.sync()
        for g in (1, 0):
            b.step_group(g, act)
        for g in range(2):
            b.group_sync(g)
        for xa, xb, name in zip(outs, (b.obs, b.reward, b.done, b.flags), parity.OUTPUTS):
            assert torch.equal(xa, xb), "%s differs at step %d" % (name, t)
        for key in INFO_KEYS + ("final_observation", ):
            assert torch.equal(a.step_info[key], b.step_info[key]), "%s differs at step %d" % (key, t)
        n_done += int(outs[2].sum())
    assert n_done >= n * 120 // 40


def test_step_info_with_topdown_images(descs):
    """use_topdown=True with step_info=True: the images equal the plain env's through >= 20 episode ends (the pose history restarts at
    a reset exactly as before), the info tensors and statistics work, and no terminal image is built."""
    import torch
    from pgdrive_amd import PGDriveVecEnv
    n = 64
    conf = dict(num_envs=n, seed=3, start_seed=1000, environment_num=8, horizon=30, use_topdown=True)
    plain, info = parity.closing(PGDriveVecEnv(conf)), parity.closing(PGDriveVecEnv(dict(conf, step_info=True)))
    seeds = np.arange(n) % 8 + 1000
    assert torch.equal(plain.reset(force_seed=seeds), info.reset(force_seed=seeds))
    assert info.last_info["final_observation"] is None
    actions = parity.driving_with_bursts(np.random.default_rng(8), n)
    n_done = 0
    for t in range(75):
        act = torch.from_numpy(actions(t)).to("cuda").view(n, 2)
        img_a, r_a, d_a, f_a = plain.step(act)
        img_b, r_b, d_b, f_b = info.step(act)
        torch.cuda.synchronize()
        assert torch.equal(img_a, img_b), "images differ at step %d" % t
        assert torch.equal(r_a, r_b) and torch.equal(d_a, d_b) and torch.equal(f_a, f_b)
        n_done += int(d_a.sum())
    assert n_done >= 20 and n_done >= n * (75 // 30)  # (every env meets its time limit at least twice)
    stats = info.episode_stats()
    assert stats["episodes"] == n_done and stats["mean_length"] <= 30 and 0.0 < stats["max_step_rate"] <= 1.0
    assert int(info.last_info["episode_length"].max()) <= 30


def test_step_info_refusals(descs):
    """Multi-agent engines refuse the step info; step_n and step_packed refuse to run while it is on; after disabling it the engine
    steps bit-identically to one that never had it."""
    import torch
    from pgdrive_amd.engine import PgdError
    d, mb, sb = util.make_marl_banks(num_agents=8, capacity=8, kind="roundabout")
    marl = parity.engine(util.marl_config(16, sb, horizon=120), mb, sb)
    with pytest.raises(PgdError):
        marl.enable_step_info()
    assert marl.step_info is None
    n = 64
    a, _ = build(descs, "c3", n)
    b, _ = build(descs, "c3", n, with_info=False)
    ids = np.arange(n) % 8
    a.reset(ids); b.reset(ids)
    ring = torch.zeros((2, n, 1, 2), device=a.device)
    with pytest.raises(PgdError):
        a.step_n(ring, 0, 2)
    with pytest.raises(PgdError):
        a.step_packed(ring[0], torch.zeros((n, a.D + 2), device=a.device))
    with pytest.raises(PgdError):
        b.episode_stats()
    actions = parity.driving_with_bursts(np.random.default_rng(8), n)
    for t in range(50):  # with the info on, through the first time limit ...
        at = torch.from_numpy(actions(t)).to(a.device)
        a.step(at); b.step(at)
    a.disable_step_info()
    assert a.step_info is None
    n_done = 0
    for t, outs_a, outs_b in parity.twins(a, b, 50, lambda t: actions(50 + t)):  # ... and off, through the second
        parity.same_bits(t, outs_a, outs_b, a, b)
        n_done += int(outs_a[2].sum())
    assert n_done >= n and "k_step_info" not in a.describe_step()
    a.step_n(ring, 0, 2); a.sync()  # (no longer refused)
