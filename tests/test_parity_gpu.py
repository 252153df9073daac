"""Parity of the HIP step engine (through the C ABI) against the CPU oracle on identical seeded inputs.

Tolerances: observations are fp32 values in [0,1] -> 1e-5 abs vs the fp64 oracle; rewards 1e-4
(a difference of two ~100 m lane coordinates in fp32); poses 1e-3 m / 1e-4 rad after one step from an identical
state; done / flags bit-exact.
"""
import os

import numpy as np
import pytest

from pgdrive_amd import _abi
from tests import parity, util
from tests.parity import OBS_TOL, REW_TOL, STATE_OBS_TOL, closed_engines  # noqa: F401 (the fixture closes every engine a test made)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("num_traffic,num_lasers,traffic_mode,ego", [
    pytest.param(16, 240, "trigger", "driving", id="16-240"), pytest.param(0, 0, "trigger", "driving", id="0-0"),
    pytest.param(16, 240, "respawn", "driving", id="16-240-respawn-driving"),
    pytest.param(16, 240, "respawn", "parked", id="16-240-respawn-parked"),
    # odd row widths (D = 275 and 105): the 4-byte side of the observation code's store-width guards
    pytest.param(16, 241, "trigger", "driving", id="16-241"), pytest.param(12, 71, "respawn", "driving", id="12-71-respawn-driving")])
def test_teacher_forced_parity(descs, num_traffic, num_lasers, traffic_mode, ego):
    """Each step starts from the same fp32-rounded state on both sides; outputs and the next state must agree.  In trigger mode almost
    no beam hits anything; respawn traffic (every IDM vehicle drives from step 0) exercises the lidar: once with the ego parked (long
    episodes, the traffic drives past: leader, lane-change and beam decisions) and once with the ego driving (it ends in the jam every
    few steps: contacts in every sub-step)."""
    parity.single_teacher_forced(descs, num_traffic, num_lasers, traffic_mode=traffic_mode, ego=ego)


@pytest.mark.parametrize("idm_agent", [False, True])
def test_idm_steer_lag_parity(descs, idm_agent):
    """pgd_config::idm_steer_lag (an opt-in of this build, not a reference key: a first-order lag on the steering IDM-driven vehicles
    apply; 0 = the reference's behaviour, which every other test runs): engine and oracle implement the same rule -- teacher-forced
    parity with the lag on, respawn traffic (every IDM vehicle drives), with and without the ego under the IDM policy; the applied
    steering (SF_STEER) stays inside [-1, 1] and differs from the raw command of the action deque (SF_ACT1S)."""
    n_envs = 96
    eng, ora, cfg = parity.engines(descs, n_envs, n_maps=16, seed=4, traffic_mode="respawn", idm_steer_lag=0.2, idm_agent=int(idm_agent))
    assert "specialised" not in (eng.describe_step() or "")
    ids = np.arange(n_envs) % 16
    assert np.abs(eng.reset(ids).cpu().numpy() - ora.reset(ids)).max() < OBS_TOL
    rng = np.random.default_rng(31)
    stats = parity.new_stats()
    worst = {}
    lagged = 0
    # (a parked ego keeps the respawn jam from restarting the env every step)
    for s in parity.teacher_forced(eng, ora, stats, 250, lambda t: util.driving_actions(rng, n_envs) * (0.0 if not idm_agent else 1.0)):
        agree = s.agree
        tie = s.idm_tie(agree)
        s.compare_state(agree & ~tie, worst)
        assert (~agree).sum() == 0
        drv = s.gi[_abi.SI["STATUS"]] == _abi.ST_ACTIVE
        drv[:, 0] &= bool(idm_agent)
        st, cmd = s.gf[_abi.SF["STEER"]][drv], s.gf[_abi.SF["ACT1S"]][drv]
        assert (np.abs(st) <= 1.0 + 1e-6).all()
        lagged += int((np.abs(st - np.clip(cmd, -1, 1)) > 1e-3).sum())
    print("steer lag parity:", stats, {k: round(v, 3) for k, v in worst.items()})
    parity.report("steer lag parity", stats)
    assert "specialised" not in eng.describe_step()
    assert stats["obs"] < OBS_TOL and stats["rew"] < REW_TOL and stats["flag_mismatch"] == 0 and stats.get("flag_ties", 0) == 0
    assert not util.state_failures(worst), util.state_failures(worst)
    assert lagged > 1000


def test_throughput_mode_parity(descs):
    """Throughput mode (engines with >= 32768 envs, or PGD_PACK=1): one vehicle per lane, three whole envs of 17 slots per wave,
    the lidar rows of the wave's envs appended to the same launch (k_step<ONE_ENV = false> + pack_obs).  Same teacher-forced
    comparison against the oracle, with an env count that leaves the last wave partly empty, auto-reset with re-drawn
    scenarios; then free-running against the default kernel: flags / done / integer state bit-identical."""
    n_envs = 65
    eng, ora, cfg = parity.engines(descs, n_envs, env=dict(PGD_PACK="1"), seed=3, resample_scenario=1)
    ids = np.arange(n_envs) % 8
    assert np.abs(eng.reset(ids).cpu().numpy() - ora.reset(ids)).max() < OBS_TOL
    rng = np.random.default_rng(12)
    stats = parity.new_stats()
    worst = {}
    n_done = 0
    for s in parity.teacher_forced(eng, ora, stats, 300, parity.driving_with_bursts(rng, n_envs)):
        n_done += int(s.o_done.sum())
        agree = s.agree
        tie = s.idm_tie(agree, skip_slots=1)
        s.compare_state(agree & ~tie, worst)
        assert (~agree).sum() == 0
    print("throughput mode parity:", stats, "episodes", n_done, "state fields (x tolerance):", {k: round(v, 3) for k, v in worst.items()})
    parity.report("throughput mode parity", stats)
    assert stats["obs"] < OBS_TOL and stats["obs_state"] < STATE_OBS_TOL and stats["rew"] < REW_TOL
    assert stats["flag_mismatch"] == 0 and stats.get("flag_ties", 0) == 0 and n_done > 20
    assert not util.state_failures(worst), util.state_failures(worst)
    assert stats.get("grazing", 0) <= 1e-5 * stats.get("beams", 1) + 2
    one, _, _ = parity.engines(descs, n_envs, env=dict(PGD_PACK="0"), seed=3, resample_scenario=1)
    eng.reset(ids); one.reset(ids)
    for t, outs_one, outs_eng in parity.twins(one, eng, 200, lambda t: util.driving_actions(rng, n_envs), copy_state=one):
        parity.same_outcome(t, outs_one, outs_eng, one, eng, obs_tol=2e-6, rew_tol=2e-5)  # (the float state is not compared here)


@pytest.mark.parametrize("pack", ["0", "1"])
@pytest.mark.parametrize("traffic_mode", ["trigger", "respawn"])
def test_default_configuration_kernel_matches_the_general_kernel(descs, pack, traffic_mode):
    """pgd_step launches an instantiation of k_step specialised for the reference's default single-agent configuration (the
    configuration values are compile-time constants in it) whenever the engine's configuration is exactly that; PGD_NO_FIX=1
    keeps the general kernel.  Same state, same actions: flags, done and the integer state are bit-identical, observation and
    reward agree to rounding (constant folding reorders a few fp32 operations).  Any other configuration gets the general kernel."""
    import torch
    n_envs = 65
    kw = dict(seed=3, resample_scenario=1, traffic_mode=traffic_mode)
    fix, _, _ = parity.engines(descs, n_envs, env=dict(PGD_PACK=pack, PGD_NO_FIX=None), **kw)
    other, _, _ = parity.engines(descs, n_envs, env=dict(PGD_PACK=pack, PGD_NO_FIX=None), num_lasers=120, **kw)
    gen, _, _ = parity.engines(descs, n_envs, env=dict(PGD_PACK=pack, PGD_NO_FIX="1"), **kw)
    ids = np.arange(n_envs) % 8
    fix.reset(ids); gen.reset(ids); other.reset(ids)
    rng = np.random.default_rng(21)
    n_done = 0
    for t, outs_gen, outs_fix in parity.twins(gen, fix, 300, parity.driving_with_bursts(rng, n_envs), copy_state=gen):
        parity.same_outcome(t, outs_gen, outs_fix, gen, fix, obs_tol=2e-6, rew_tol=2e-5, state_tol=1e-4)
        n_done += int(outs_gen[2].sum())
    assert n_done > 20
    other.step(torch.from_numpy(util.driving_actions(rng, n_envs)).to(other.device)); other.sync()
    assert "specialised for the default" in fix.describe_step()
    assert "specialised" not in gen.describe_step() and "specialised" not in other.describe_step()
    assert ("throughput mode" in fix.describe_step()) == (pack == "1")


@pytest.mark.parametrize("variant", ["top_down", "safe"])
def test_env_class_instantiations_match_the_general_kernel(descs, variant):
    """Round 6: the configurations the shipped env classes produce besides the default one have their own
    instantiations of k_step -- the top-down envs' (envs/top_down_env.py:8-72: lidar off, the row is the 18 state floats)
    and SafePGDriveEnv's (envs/safe_pgdrive_env.py:9-26: 16 traffic + 40 object slots, crashes are costs).  Same protocol as the
    default configuration's test: against the general kernel (PGD_NO_FIX=1) from the same state with the same actions, flags / done /
    integer state bit-identical, floats to rounding; pgd_describe_step names the instantiation; a neighbouring configuration (another
    slot count) still gets the general kernel."""
    import torch
    n_envs = 65
    kw = dict(seed=3, resample_scenario=1)
    if variant == "top_down":
        kw.update(num_lasers=0)
        other_kw = dict(kw, num_traffic=12)
        name = "specialised for the top-down envs"
    else:
        kw.update(num_traffic=56, accident_prob=0.8, safe_rl_env=True, density=0.05, use_lateral=False)
        other_kw = dict(kw, num_traffic=46)
        name = "specialised for the SafePGDriveEnv"
    fix, _, _ = parity.engines(descs, n_envs, n_maps=16, env=dict(PGD_NO_FIX=None), **kw)
    other, _, _ = parity.engines(descs, n_envs, n_maps=16, env=dict(PGD_NO_FIX=None), **other_kw)
    gen, _, _ = parity.engines(descs, n_envs, n_maps=16, env=dict(PGD_NO_FIX="1"), **kw)
    ids = np.arange(n_envs) % 16
    fix.reset(ids); gen.reset(ids); other.reset(ids)
    rng = np.random.default_rng(22)
    n_done = n_obj = 0
    for t, outs_gen, outs_fix in parity.twins(gen, fix, 300, parity.driving_with_bursts(rng, n_envs), copy_state=gen):
        parity.same_outcome(t, outs_gen, outs_fix, gen, fix, obs_tol=2e-6, rew_tol=2e-5, state_tol=1e-4)
        n_done += int(outs_gen[2].sum())
        n_obj += int(((outs_gen[3] & _abi.F_CRASH_OBJECT) != 0).sum())
    assert n_done > 10 and (variant != "safe" or n_obj > 0)
    other.step(torch.from_numpy(util.driving_actions(rng, n_envs)).to(other.device)); other.sync()
    assert name in fix.describe_step(), fix.describe_step()
    assert "specialised" not in gen.describe_step() and "specialised" not in other.describe_step()
    assert fix.D == (18 if variant == "top_down" else 274)


@pytest.mark.parametrize("variant", ["lasers72_traffic12", "discrete_fans_noise", "objects"])
def test_run_time_kernel_matches_the_general_kernel(descs, monkeypatch, tmp_path, variant):
    """pgdrive_amd/jit.py + pgd_set_step_module (round 6): a step kernel with ONE engine's configuration compiled in, built with hipcc at
    run time, for configurations the library has no instantiation for -- another beam / traffic / neighbour count; discrete actions with
    side and lane-line detector fans and lidar noise (the general row layout); traffic objects among the bodies.  Same protocol as the
    AOT instantiations' tests: against the general kernel from the same state with the same actions, flags / done / integer state
    bit-identical, floats to rounding, through auto-resets with re-drawn scenarios; pgd_describe_step names it; unloading the module
    (null path) puts the general kernel back."""
    import torch
    monkeypatch.setenv("PGD_JIT_DIR", str(tmp_path))  # (read by pgdrive_amd/jit.py when the kernel is built, not by the constructor)
    n_envs = 65
    kw = dict(seed=3, resample_scenario=1)
    if variant == "lasers72_traffic12":
        kw.update(num_traffic=12, num_lasers=72, num_others=2, lidar_dist=40.0, success_reward=20.0)
    elif variant == "discrete_fans_noise":
        kw.update(discrete_action=True, side_lasers=4, lane_line_lasers=2, lidar_gaussian_noise=0.02, lidar_dropout_prob=0.05, horizon=150)
    else:
        kw.update(num_traffic=30, accident_prob=0.8, density=0.05)
    jit_eng, _, _ = parity.engines(descs, n_envs, n_maps=16, env=dict(PGD_NO_FIX=None), **kw)
    gen, _, _ = parity.engines(descs, n_envs, n_maps=16, env=dict(PGD_NO_FIX=None), **kw)
    assert jit_eng.specialise(wait=True) is True
    assert any(f.endswith(".hsaco") for f in os.listdir(str(tmp_path)))
    ids = np.arange(n_envs) % 16
    jit_eng.reset(ids); gen.reset(ids)
    rng = np.random.default_rng(23)
    n_done = 0

    def actions(t):
        act = util.driving_actions(rng, n_envs)
        if variant == "discrete_fans_noise":
            act = rng.integers(0, 5, size=(n_envs, 1, 2)).astype(np.float32)
            act[:, 0, 1] = np.maximum(act[:, 0, 1], 2.0)
        elif t % 4 == 0:
            act[::3, 0, :] = 1.0
        actions.last = act
        return act

    for t, outs_gen, outs_jit in parity.twins(gen, jit_eng, 300, actions, copy_state=gen):
        parity.same_outcome(t, outs_gen, outs_jit, gen, jit_eng, obs_tol=2e-6, rew_tol=2e-5, state_tol=1e-4)
        n_done += int(outs_gen[2].sum())
    assert n_done > 10
    assert "at run time" in jit_eng.describe_step() and "specialised" not in gen.describe_step()
    assert jit_eng.L.pgd_set_step_module(jit_eng.h, None, 0, 0) == 0
    jit_eng.step(torch.from_numpy(actions.last).to(jit_eng.device)); jit_eng.sync()
    assert "specialised" not in jit_eng.describe_step()


def test_run_time_kernel_is_refused_where_it_does_not_apply(descs, monkeypatch, tmp_path):
    """Engines that cannot take a run-time kernel say so (specialise() returns False, nothing is built): multi-agent engines and
    throughput mode; an engine whose configuration the library already has an instantiation for keeps that instantiation even with a
    module loaded (the module only ever replaces a GENERAL kernel)."""
    monkeypatch.setenv("PGD_JIT_DIR", str(tmp_path))
    import torch
    d, mb, sb = util.make_marl_banks(num_agents=8, capacity=12, kind="roundabout")
    marl = parity.engine(util.marl_config(16, sb, horizon=120), mb, sb)
    assert marl.specialise() is False
    pack, _, _ = parity.engines(descs, 66, env=dict(PGD_PACK="1"), seed=1)
    assert pack.specialise() is False
    dflt, _, _ = parity.engines(descs, 64, env=dict(PGD_PACK="0"), seed=1)
    assert dflt.specialise() is True  # (built and loaded ...)
    dflt.reset(np.arange(64) % 8)
    dflt.step(torch.zeros((64, 1, 2), device="cuda")); dflt.sync()
    assert "specialised for the default single-agent configuration" in dflt.describe_step()  # (... and not used: the AOT instantiation runs)
    assert len([f for f in os.listdir(str(tmp_path)) if f.endswith(".hsaco")]) == 1


def test_multi_agent_env_groups_step_like_one_batch():
    """The 40-seat engine as two asynchronous env groups (pgd_set_groups / pgd_step_group; bench.py's row c5_40x72_two_groups): the step
    kernel and the four-wave observation kernel of a group run on the group's stream over the group's envs only -- and leave, group
    by group and in any order, exactly the bytes one launch over the whole batch leaves, through finishes and respawns."""
    import torch
    d, mb, sb = util.make_marl_banks(num_agents=40, capacity=40, kind="roundabout")
    n_envs = 64
    cfg = util.marl_config(n_envs, sb, horizon=120)
    one, two = parity.engine(cfg, mb, sb), parity.engine(cfg, mb, sb)
    ids = np.arange(n_envs) % 8
    one.reset(ids); two.reset(ids)
    two.set_groups(2)
    rng = np.random.default_rng(11)
    n_done = n_new = 0
    for t in range(260):
        a = torch.from_numpy(util.marl_actions(rng, n_envs, sb.A)).to(one.device)
        o, r, dn, fl = [x.clone() for x in one.step(a)]
        one.sync()
        for g in ((1, 0) if t % 2 else (0, 1)):
            two.step_group(g, a)
        for g in range(2):
            two.group_sync(g)
        assert torch.equal(two.flags, fl) and torch.equal(two.done, dn), "flags differ at step %d" % t
        assert torch.equal(two.obs, o) and torch.equal(two.reward, r), "rows differ at step %d" % t
        n_done += int(dn.sum()); n_new += int(((fl & _abi.F_NEW) != 0).sum())
    assert n_done > 40 and n_new > 40
    assert "40 agent seats" in one.describe_step() and "40 agent seats" in two.describe_step()
    # the same from the env surface (MultiAgent*VecEnv.set_groups / step_group / group_sync)
    from pgdrive_amd import MultiAgentRoundaboutVecEnv
    e1, e2 = (parity.closing(MultiAgentRoundaboutVecEnv(dict(num_envs=16, num_agents=40, seed=3))) for _ in range(2))
    e1.reset(); e2.reset()
    e2.set_groups(2)
    for t in range(40):
        a = torch.from_numpy(util.marl_actions(rng, 16, e1.A)).to(e1.engine.device)
        o, r, dn, fl = [x.clone() for x in e1.step(a)]
        for g in (0, 1):
            og, rg, dg, fg = e2.step_group(g, a)
            e2.group_sync(g)
            sl = e2.group_slice(g)
            assert torch.equal(og, o[sl]) and torch.equal(rg, r[sl]) and torch.equal(dg, dn[sl]) and torch.equal(fg, fl[sl])
    f1, i1, e1 = one.get_state()
    f2, i2, e2 = two.get_state()
    assert (i1 == i2).all() and (e1 == e2).all() and np.array_equal(f1, f2)


@pytest.mark.parametrize("agents,seats,beams", [(8, 12, 72), (40, 40, 72), (40, 44, 72), (8, 8, 72), (8, 8, 240)])
def test_default_multi_agent_kernel_matches_the_general_kernel(agents, seats, beams):
    """Multi-agent engines with the scalar fields of MULTI_AGENT_PGDRIVE_DEFAULT_CONFIG get their own instantiation of k_step (those
    fields are compile-time constants in it; agent count, spawn places and horizon stay run-time values) -- and, round 6, the seat
    counts the reference's default agent number produces (40: the vec env; 44: the dict-keyed envs' spare seats) instantiations with
    the seat count, the row width and the 72 beams folded as well, in the step AND in the four-wave observation kernel; and the 8 seats
    of BASELINE.json's multi-agent configuration with 72 and with 240 beams (the observation fused into the step).  Against the
    general kernels (PGD_NO_FIX=1) from the same state with the same actions: flags, done, integer state identical, floats to rounding."""
    import torch
    d, mb, sb = util.make_marl_banks(num_agents=agents, capacity=seats, kind="roundabout")
    n_envs = 32
    cfg = util.marl_config(n_envs, sb, horizon=120, num_lasers=beams)
    fix = parity.engine(cfg, mb, sb, env=dict(PGD_NO_FIX=None))
    other = parity.engine(util.marl_config(n_envs, sb, horizon=120, delay_done=10, num_lasers=beams), mb, sb, env=dict(PGD_NO_FIX=None))
    gen = parity.engine(cfg, mb, sb, env=dict(PGD_NO_FIX="1"))
    ids = np.arange(n_envs) % 8
    fix.reset(ids); gen.reset(ids); other.reset(ids)
    rng = np.random.default_rng(5)
    n_done = n_new = n_graze = 0
    for t, (o1, r1, d1, f1), (o2, r2, d2, f2) in parity.twins(gen, fix, 300, lambda t: util.marl_actions(rng, n_envs, sb.A), copy_state=gen):
        parity.same_outcome(t, (o1, r1, d1, f1), (o2, r2, d2, f2), gen, fix)  # (floats: below, on the rows that are due, grazing beams counted)
        rep = ((f1 & (_abi.F_REPORT | _abi.F_NEW)) != 0)
        dd = (o1 - o2).abs() * rep[..., None]
        # (a beam that grazes a box corner is a hit in one instantiation and a miss in the other -- the slab test compares two nearly
        # equal parameters, and the two kernels round them differently: seen once in 300 steps x 32 envs at 44 seats, beam 70 of a row,
        # 0.16 against 1.0.  Such flips are counted, like the grazing beams of the oracle comparisons; everything else agrees to 2e-6)
        # (tools/marl_seat_soak.py, 4000 steps x 128 envs: 4 and 6 such beams of 0.49 G at 40 and 44 seats -- one of them against the
        # body BEHIND the corner instead of 1.0 --, no flag, done or integer-state difference)
        flip = dd[..., 18:] > 2e-6
        n_graze += int(flip.sum())
        dd[..., 18:][flip] = 0.0
        assert float(dd.max()) < 2e-6 and float(((r1 - r2).abs() * rep).max()) < 2e-5
        n_done += int(d1.sum()); n_new += int(((f1 & _abi.F_NEW) != 0).sum())
    assert n_done > 20 and n_new > 20 and n_graze <= 3, n_graze
    other.step(torch.from_numpy(util.marl_actions(rng, n_envs, sb.A)).to(other.device)); other.sync()
    assert "specialised for the default multi-agent" in fix.describe_step()
    assert ("%d agent seats x %d beams" % (seats, beams) in fix.describe_step()) == (seats in (40, 44, 8)), fix.describe_step()
    assert "specialised" not in gen.describe_step() and "specialised" not in other.describe_step()


@pytest.mark.parametrize("traffic_mode", ["trigger", "hybrid"])
def test_step_hints_match_the_unhinted_path(descs, traffic_mode):
    """k_step leaves two verdicts for the env's next step in a device-private word (EI_NEAR): "no body can reach the agent" (contact
    tests skipped) and whether the agent stands on the trigger road of the next traffic group (the trigger test then needs no
    reads).  pgd_set_state resets the word to "unknown".  An engine that free-runs with the hints and one that has its own state
    written back before every step (always the unhinted path) must stay bit-identical: observations, rewards, flags, state --
    through traffic activations, crashes and auto-resets with re-drawn scenarios."""
    n_envs = 96
    a, _, _ = parity.engines(descs, n_envs, seed=9, resample_scenario=1, traffic_mode=traffic_mode)
    b, _, _ = parity.engines(descs, n_envs, seed=9, resample_scenario=1, traffic_mode=traffic_mode)
    ids = np.arange(n_envs) % 8
    a.reset(ids); b.reset(ids)
    rng = np.random.default_rng(33)
    n_done = activations = 0
    prev_pending = None
    # (b's own state written back before every step: the hint word back to "unknown")
    for t, outs_a, outs_b in parity.twins(a, b, 600, lambda t: util.driving_actions(rng, n_envs), copy_state=b):
        parity.same_bits(t, outs_a, outs_b, a, b)
        pending = (a.get_state()[1][_abi.SI["STATUS"]] == _abi.ST_PENDING).sum()
        if prev_pending is not None and pending < prev_pending:
            activations += 1
        prev_pending = pending
        n_done += int(outs_a[2].sum())
    assert n_done > 30 and activations > 10


def test_ego_only_kernel_matches_the_general_kernel(descs):
    """BASELINE config 2 (the ego alone, no lidar: dynamics + reward + the 18-float state vector) has its own instantiation of k_step
    too (four envs per wave, configuration compiled in).  Against the general kernel from the same state with the same actions."""
    n_envs = 130  # the last wave is partly empty
    fix, _, _ = parity.engines(descs, n_envs, env=dict(PGD_NO_FIX=None), seed=3, resample_scenario=1, num_traffic=0, num_lasers=0)
    gen, _, _ = parity.engines(descs, n_envs, env=dict(PGD_NO_FIX="1"), seed=3, resample_scenario=1, num_traffic=0, num_lasers=0)
    ids = np.arange(n_envs) % 8
    fix.reset(ids); gen.reset(ids)
    rng = np.random.default_rng(4)
    n_done = 0
    for t, outs_gen, outs_fix in parity.twins(gen, fix, 400, lambda t: util.driving_actions(rng, n_envs), copy_state=gen):
        parity.same_outcome(t, outs_gen, outs_fix, gen, fix, obs_tol=2e-6, rew_tol=2e-5, state_tol=1e-4)
        n_done += int(outs_gen[2].sum())
    assert n_done > 20 and outs_gen[0].shape[-1] == 18
    assert "specialised for the ego-only" in fix.describe_step() and "specialised" not in gen.describe_step()


def test_run_time_reward_kernel_matches_the_general_kernel_and_the_oracle(descs):
    """Default geometry, own reward scheme (what training set-ups change first): k_step runs the instantiation with the geometry
    compiled in and the reward scheme read at run time.  Teacher-forced against the oracle, and against the general kernel."""
    import torch
    kw = dict(success_reward=20.0, use_lateral=True, speed_reward=0.3, out_of_road_penalty=7.0)
    n_envs = 64
    eng, ora, cfg = parity.engines(descs, n_envs, env=dict(PGD_NO_FIX=None), seed=5, **kw)
    gen, _, _ = parity.engines(descs, n_envs, env=dict(PGD_NO_FIX="1"), seed=5, **kw)
    ids = np.arange(n_envs) % 8
    assert np.abs(eng.reset(ids).cpu().numpy() - ora.reset(ids)).max() < OBS_TOL
    gen.reset(ids)
    rng = np.random.default_rng(8)
    stats = parity.new_stats()
    n_done = 0
    for t in range(300):
        act = util.driving_actions(rng, n_envs)
        f, i, ei = ora.get_state()
        f32 = util.round_state_f32(f)
        gen.set_state(f32, i, ei)
        r_gen = gen.step(torch.from_numpy(act).to(gen.device))[1].clone()
        n_done += int(parity.compare_step(eng, ora, act, stats).sum())
        gen.sync()
        assert float((r_gen - eng.reward).abs().max()) < 2e-5
        f, i, ei = ora.get_state()
        f32 = util.round_state_f32(f)
        ora.set_state(f32, i, ei); eng.set_state(f32, i, ei)
    parity.report("run-time reward kernel parity", stats)
    assert stats["flag_mismatch"] == 0 and stats.get("flag_ties", 0) == 0 and stats["obs"] < OBS_TOL and stats["rew"] < REW_TOL and n_done > 10
    assert "run-time reward scheme" in eng.describe_step() and "specialised" not in gen.describe_step()


def test_random_lane_width_and_num_maps_parity():
    """random_lane_width / random_lane_num (map_manager.py:157-169): 2-lane maps with a lane width per seed in [3.0, 4.5)
    through the same teacher-forced comparison."""
    from pgdrive_amd import bank
    maps = bank.get_descriptions(range(1000, 1008), random_lane_width=True, random_lane_num=True)
    assert all(m["lane_num"] == 2 for m in maps) and len({round(m["lane_width"], 6) for m in maps}) == 8
    parity.single_teacher_forced(maps, 16, 240)


@pytest.mark.parametrize("side,lane_line,num_lasers", [((12, 50.0), (6, 20.0), 240), ((2, 50.0), (2, 50.0), 0),
                                                       ((0, 50.0), (33, 20.0), 16), ((70, 30.0), (0, 20.0), 0),
                                                       ((5, 50.0), (3, 20.0), 71)])  # every fan odd, D = 111
def test_side_and_lane_line_detector_parity(descs, side, lane_line, num_lasers):
    """SideDetector / LaneLineDetector fans (distance_detector.py:137-152) spliced into the state block
    (state_obs.py:64-71,96-105): device grid walk vs the oracle's brute force over every line box."""
    n_envs = 64
    ram = num_lasers == 16  # one of the configurations also runs with random_agent_model (vehicle type + 2 state floats)
    eng, ora, cfg = parity.engines(descs, n_envs, num_lasers=num_lasers, side_lasers=side[0], side_dist=side[1],
                                    lane_line_lasers=lane_line[0], lane_line_dist=lane_line[1], random_agent_model=ram)
    assert eng.D == (side[0] or 2) + 6 + lane_line[0] + (2 if ram else 0) + 10 + 4 * cfg.num_others + num_lasers
    scen_ids = np.arange(n_envs) % 8
    o0 = ora.reset(scen_ids)
    g0 = eng.reset(scen_ids).cpu().numpy()
    parity.check_reset_rows(eng, ora, g0, o0, 2)
    rng = np.random.default_rng(5)
    stats = parity.new_stats()
    for _ in parity.teacher_forced(eng, ora, stats, 150, lambda t: util.driving_actions(rng, n_envs)):
        pass
    print("detector parity:", stats)
    parity.report("detector parity", stats)
    assert stats["obs"] < OBS_TOL and stats["rew"] < REW_TOL
    assert stats["flag_mismatch"] == 0 and stats.get("flag_ties", 0) == 0
    assert stats["det_grazing"] <= 1e-4 * stats["det_beams"] + 2
    assert stats.get("grazing", 0) <= 1e-5 * stats.get("beams", 1) + 2


@pytest.mark.parametrize("discrete", [True, False])
def test_action_modes_respawn_traffic_auto_termination(descs, discrete):
    """discrete_action (env_input_policy.py:17-31, converted after the clip as upstream), increment_steering
    (base_vehicle.py:351-358), TrafficMode.Respawn (traffic_manager.py:236-239) and auto_termination (base_env.py:318)."""
    import torch
    n_envs = 64
    eng, ora, cfg = parity.engines(descs, n_envs, discrete_action=discrete, increment_steering=True,
                                    traffic_mode="respawn", auto_termination=True, num_lasers=60)
    scen_ids = np.arange(n_envs) % 8
    o0 = ora.reset(scen_ids)
    g0 = eng.reset(scen_ids).cpu().numpy()
    assert np.abs(g0 - o0).max() < OBS_TOL
    f, i, ei = ora.get_state()
    assert (i[_abi.SI["STATUS"]][:, 1:] == _abi.ST_ACTIVE).sum() > 8 * n_envs  # respawn-mode traffic drives from step 0
    # jump half of the envs close to their auto-termination step (250 * num_blocks = 1000 for 3-block maps)
    ei[_abi.EI["EP_STEPS"], ::2] = 995
    ora.set_state(f, i, ei)
    eng.set_state(util.round_state_f32(f), i, ei)
    rng = np.random.default_rng(11)
    stats = parity.new_stats()
    n_max_step = 0
    for t in range(120):
        if discrete:  # MultiDiscrete([5, 5]) samples; upstream clips them to [-1, 1] BEFORE the conversion, so the
            # car only ever brakes (steering / throttle in {-1, -0.5}) -- reproduced as is
            act = rng.integers(0, 5, size=(n_envs, 1, 2)).astype(np.float32)
            act[::7] = rng.uniform(-2, 2, size=act[::7].shape).astype(np.float32)  # and a few stray floats
        else:
            act = util.driving_actions(rng, n_envs)
            act[..., 0] *= 4.0  # incremental steering: 0.05 per unit action
        o_obs, o_rew, o_done, o_flags = ora.step(act)
        n_max_step += int(((o_flags & _abi.F_MAX_STEP) != 0).sum())
        g_obs, g_rew, g_done, g_flags = eng.step(torch.from_numpy(act).to(eng.device))
        eng.sync()
        same = (g_flags.cpu().numpy().astype(np.uint32) == o_flags) & (g_done.cpu().numpy() == o_done)
        stats["steps"] += same.size
        stats["flag_mismatch"] += int((~same).sum())
        d = np.abs(g_obs.cpu().numpy().astype(np.float64) - o_obs)[same]
        stats["obs"] = max(stats["obs"], float(d[:, :-60].max()))
        stats["rew"] = max(stats["rew"], float(np.abs(g_rew.cpu().numpy() - o_rew)[same].max()))
        f, i, ei = ora.get_state()
        f32 = util.round_state_f32(f)
        ora.set_state(f32, i, ei)
        eng.set_state(f32, i, ei)
    print("action modes parity:", stats, "max_step flags", n_max_step)
    assert n_max_step >= n_envs // 4  # the jumped envs hit 250 * num_blocks unless they crashed before
    assert stats["obs"] < OBS_TOL and stats["rew"] < REW_TOL and stats["flag_mismatch"] == 0 and stats.get("flag_ties", 0) == 0


@pytest.mark.parametrize("safe", [False, True])
def test_traffic_objects_parity(descs, safe):
    """Traffic cones / warning tripods (circles), barriers and broken-down vehicles (object_manager.py:40-124) as static
    bodies: crash_object on first contact only (collision_callback.py:27-32), lidar hits, IDM obstacles, no neighbour-info
    rows; SafePGDriveEnv termination rule (safe_pgdrive_env.py:49-56)."""
    n_envs = 64
    eng, ora, cfg = parity.engines(descs, n_envs, n_maps=16, num_traffic=46, accident_prob=1.0, safe_rl_env=safe,
                                    auto_reset=0)
    scen_ids = np.arange(n_envs) % 16
    o0 = ora.reset(scen_ids)
    g0 = eng.reset(scen_ids).cpu().numpy()
    parity.check_reset_rows(eng, ora, g0, o0, 2)
    f, i, ei = ora.get_state()
    moved = parity.teleport_to_objects(ora.map_bank, ora.scen_bank, scen_ids, f, i)
    assert moved >= n_envs // 2
    f32 = util.round_state_f32(f)
    ora.set_state(f32, i, ei)
    eng.set_state(f32, i, ei)
    rng = np.random.default_rng(9)
    stats = parity.new_stats()
    n_hit_state = 0

    def actions(t):
        act = util.driving_actions(rng, n_envs)
        act[..., 1] = 0.4
        return act

    for s in parity.teacher_forced(eng, ora, stats, 60, actions):
        # incl. the objects' own "crashed" bits: differing only as margin-verified ties, at most the two allowed before
        vf_bad = s.gi[_abi.SI["VFLAGS"]] != s.i[_abi.SI["VFLAGS"]]
        vf_tie = vf_bad & (util.admitted_slots(s.mg, ("CONTACT", "LANE")) |   # its own line / lane decisions, or the ego's
                           util.admitted_slots(s.mg, ("CONTACT",))[:, :1])       # contact with it (noted on the ego)
        s.ties.add_slots("CONTACT", vf_tie, s.mg)
        assert (vf_bad & ~vf_tie).sum() == 0 and vf_tie.sum() <= 2
        n_hit_state = max(n_hit_state, int((s.i[_abi.SI["VFLAGS"]][:, 1:] & _abi.F_OBJECT_HIT != 0).sum()))
    print("objects parity:", stats, "objects hit", n_hit_state)
    parity.report("objects parity", stats)
    assert stats["obs"] < OBS_TOL and stats["rew"] < REW_TOL and stats["flag_mismatch"] == 0 and stats.get("flag_ties", 0) == 0
    assert n_hit_state >= 8 and stats["n_crash_object"] >= 8
    assert stats.get("grazing", 0) <= 1e-5 * stats.get("beams", 1) + 3


def test_lidar_noise_parity(descs):
    """Lidar noise / dropout (state_obs.py:172-182) from the counter-based stream: device and oracle draw the same numbers."""
    n_envs = 32
    eng, ora, cfg = parity.engines(descs, n_envs, lidar_gaussian_noise=0.05, lidar_dropout_prob=0.1, seed=77)
    scen_ids = np.arange(n_envs) % 8
    o0 = ora.reset(scen_ids)
    g0 = eng.reset(scen_ids).cpu().numpy()
    parity.check_reset_rows(eng, ora, g0, o0, 2)
    assert (o0[:, 0, -240:] == 0.0).mean() > 0.05
    rng = np.random.default_rng(8)
    stats = parity.new_stats()
    for _ in parity.teacher_forced(eng, ora, stats, 60, lambda t: util.driving_actions(rng, n_envs)):
        pass
    print("noise parity:", stats)
    parity.report("noise parity", stats)
    assert stats["obs"] < OBS_TOL and stats["flag_mismatch"] == 0 and stats.get("flag_ties", 0) == 0 and stats["grazing"] <= 1e-4 * stats["beams"] + 3


def test_maximum_sizes(descs):
    """The largest configuration the slot layout allows: 64 vehicle slots per env (1 ego + 63 traffic, dense traffic so
    that they are used), 16 neighbour rows, 500 lidar beams; one vehicle per lane (SUB = 1), observation not fused."""
    import torch
    n_envs = 32
    eng, ora, cfg = parity.engines(descs, n_envs, num_traffic=63, density=0.6, num_lasers=500, num_others=16)
    assert eng.D == 2 + 6 + 10 + 64 + 500
    used = [i["n_traffic"] for i in ora.scen_bank.info]
    assert max(used) >= 50
    scen_ids = np.arange(n_envs) % 8
    o0 = ora.reset(scen_ids)
    g0 = eng.reset(scen_ids).cpu().numpy()
    parity.check_reset_rows(eng, ora, g0, o0, 2)
    rng = np.random.default_rng(21)
    stats = parity.new_stats()
    ties = stats.setdefault("ties", util.Ties("test_maximum_sizes"))
    tie_rows = rows = 0
    for t in range(80):
        act = util.driving_actions(rng, n_envs)
        o_obs, o_rew, o_done, o_flags = ora.step(act)
        mg = ora.margins()
        g_obs, g_rew, g_done, g_flags = eng.step(torch.from_numpy(act).to(eng.device))
        eng.sync()
        same = (g_flags.cpu().numpy().astype(np.uint32) == o_flags) & (g_done.cpu().numpy() == o_done)
        stats["steps"] += same.size
        stats["flag_mismatch"] += int((~same).sum())
        g_obs = g_obs.cpu().numpy().astype(np.float64)
        d = np.abs(g_obs - o_obs)[same]
        # With 63 vehicles spawned on the 10 m grid, IDM front / back candidates tie exactly (equal longitudinal gaps); the
        # reference resolves such ties by Python set order, fp32 and fp64 by an ulp.  A flipped tie changes one traffic
        # vehicle's acceleration, visible in the ego's neighbour-velocity floats: such rows are counted, not hidden.
        vel = np.zeros(d.shape[1], dtype=bool)
        vel[18 + 2:18 + 64:4] = vel[18 + 3:18 + 64:4] = True
        rows += d.shape[0]
        # ... and only where the oracle confirms the tie: the neighbour whose velocity differs is a slot with a verified LEADER tie
        # (util.idm_tie), or the row's NEIGHBOUR margin says that two ranks were a near-tie; any other row goes to stats["obs"]
        lead = util.idm_tie(eng.get_state()[0], ora.get_state()[0], mg)
        nb_tie = util.admissible("NEIGHBOUR", mg[util.MG["NEIGHBOUR"]][:, 0])
        for e in np.nonzero(same[:, 0])[0]:
            cols = np.nonzero((np.abs(g_obs - o_obs)[e, 0] > OBS_TOL) & vel)[0]
            if not len(cols):
                continue
            slots = [ora.neighbour_slot(e, 0, (c - 18) // 4) for c in cols]
            if nb_tie[e] or all(s_ >= 0 and lead[e, s_] for s_ in slots):
                tie_rows += 1
                ties.add("NEIGHBOUR" if nb_tie[e] else "LEADER", mg[util.MG["NEIGHBOUR" if nb_tie[e] else "LEADER"], e, 0 if nb_tie[e] else slots[0]],
                         dict(env=int(e), row_columns=[int(c) for c in cols]))
            else:
                stats["obs"] = max(stats["obs"], float(np.abs(g_obs - o_obs)[e, 0][vel].max()))
        stats["obs"] = max(stats["obs"], float(d[:, :82][:, ~vel[:82]].max()))
        parity.compare_rows(eng, ora, stats, np.where(vel[None, None, :], o_obs, g_obs), o_obs, same, mg)  # beams: margin-verified grazing only
        stats["rew"] = max(stats["rew"], float(np.abs(g_rew.cpu().numpy() - o_rew)[same].max()))
        f, i, ei = ora.get_state()
        f32 = util.round_state_f32(f)
        ora.set_state(f32, i, ei)
        eng.set_state(f32, i, ei)
    print("max sizes parity:", stats, "rows with a tie-flipped neighbour velocity", tie_rows, "of", rows)
    parity.report("max sizes parity", stats)
    assert stats["obs"] < OBS_TOL and stats["rew"] < REW_TOL and stats["flag_mismatch"] == 0 and stats.get("flag_ties", 0) == 0
    assert stats["grazing"] <= 1e-4 * stats["beams"] + 3 and tie_rows <= 0.01 * rows


def test_free_running_rollout(descs):
    """No teacher forcing: 60 steps from reset with identical actions; trajectories stay within tolerance until the first
    discrete disagreement of an env (after which that env is ignored)."""
    import torch
    n_envs = 64
    eng, ora, cfg = parity.engines(descs, n_envs)
    scen_ids = np.arange(n_envs) % 8
    ora.reset(scen_ids)
    eng.reset(scen_ids)
    rng = np.random.default_rng(1)
    alive = np.ones(n_envs, dtype=bool)
    worst = 0.0
    for t in range(60):
        act = util.driving_actions(rng, n_envs)
        o_obs, o_rew, o_done, o_flags = ora.step(act)
        g_obs, g_rew, g_done, g_flags = eng.step(torch.from_numpy(act).to(eng.device))
        eng.sync()
        same = (g_flags.cpu().numpy().astype(np.uint32) == o_flags)[:, 0] & (g_done.cpu().numpy() == o_done)[:, 0]
        alive &= same
        d = np.abs(g_obs.cpu().numpy().astype(np.float64) - o_obs)[alive]
        if d.size:
            worst = max(worst, float(d.max()))
    print("free-running: alive", int(alive.sum()), "worst obs diff", worst)
    assert alive.mean() > 0.9
    assert worst < 5e-4


@pytest.mark.timeout(900)
@pytest.mark.parametrize("num_traffic,num_lasers", [(0, 0), (16, 240)])
def test_free_running_1000_steps(descs, num_traffic, num_lasers):
    """pose after 1000 steps with identical actions, NO teacher forcing -- the fp32 engine integrates its own
    state (heading vector advanced by rotations and renormalised, own-lane coordinates and route context carried in the
    record) for 1000 steps next to the fp64 oracle.  auto_reset = 0; the actions come from a lane-keeping controller on the
    ORACLE's observation (road-centre offset + heading error -> steering, 5-9 km/h cruise -> throttle, seeded noise and a
    per-env lateral target), the same float32 action for both sides, slow enough that no episode ends on these maps.
    The bar (positions <= 1e-2 m, headings <= 1e-3 rad) is on the vehicle that RECEIVES identical actions, the ego, in every
    env at every step; flags / done / the ego's integer state / env counters may differ only transiently (a box edge reached
    one step apart) and >= 97 % of the envs must agree on them at the end.  The IDM traffic is a closed loop of its own: its steering PID (kp 1.7, kd 3.5 on the heading error, 0.1 s
    decisions, idm_policy.py:187-188,244-252) chatters between the locks, and the fp64 oracle ITSELF turns a 1e-6 m offset of
    a traffic vehicle into up to 6e-2 m within 140 steps before it contracts again (measured oracle-vs-oracle, DESIGN.md
    section 7) -- no fp32 engine can track it pose by pose over 1000 steps, so the traffic is compared statistically: the
    number of vehicles still driving, their mean speed and the median pose difference."""
    import torch
    n_envs = 64
    eng, ora, cfg = parity.engines(descs, n_envs, num_traffic=num_traffic, num_lasers=num_lasers, auto_reset=0)
    A = cfg.num_agents
    scen_ids = np.arange(n_envs) % 8
    obs = ora.reset(scen_ids)
    eng.reset(scen_ids)
    rng = np.random.default_rng(3)
    v_target = rng.uniform(5.0, 9.0, size=n_envs)
    lat_target = rng.uniform(-2.5, 2.5, size=n_envs)
    ever = np.zeros(n_envs, dtype=bool)
    mism_steps = bits_seen = 0
    pos_err = th_err = spd_err = 0.0
    n_done = 0
    SF, SI = _abi.SF, _abi.SI
    for t in range(1000):
        ob = obs[:, 0]
        lat = (ob[:, 0] - ob[:, 1]) * 18.0 - 2.0 * lat_target      # left minus right road-edge distance [m]
        head = (ob[:, 2] - 0.5) * 2.0
        steer = np.clip(0.1 * lat + 2.0 * head + rng.normal(0, 0.05, size=n_envs), -1, 1)
        thr = np.clip(0.3 * (v_target - (ob[:, 3] * 81.0 - 1.0)) + rng.normal(0, 0.1, size=n_envs), -1, 1)
        act = np.stack([steer, thr], axis=-1).astype(np.float32)[:, None, :]
        obs, o_rew, o_done, o_flags = ora.step(act)
        g_obs, g_rew, g_done, g_flags = eng.step(torch.from_numpy(act).to(eng.device))
        eng.sync()
        n_done += int(o_done.sum())
        same = (g_flags.cpu().numpy().astype(np.uint32) == o_flags)[:, 0] & (g_done.cpu().numpy() == o_done)[:, 0]
        f, i, ei = ora.get_state()
        gf, gi, gei = eng.get_state()
        ints = (gi[:, :, :A] == i[:, :, :A]).all(axis=(0, 2)) & (gei == ei).all(axis=0)
        xf = (g_flags.cpu().numpy().astype(np.uint32) ^ o_flags)[:, 0]
        agree = same & ints
        mism_steps += int((~agree).sum())
        bits_seen |= int(np.bitwise_or.reduce(xf)) if xf.size else 0
        ever |= ~agree
        # the ego's pose does not depend on any flag (auto_reset = 0): compared in every env at every step
        dx = gf[SF["X"]].astype(np.float64)[:, :A] - f[SF["X"]][:, :A]
        dy = gf[SF["Y"]].astype(np.float64)[:, :A] - f[SF["Y"]][:, :A]
        dth = np.abs(gf[SF["THETA"]].astype(np.float64)[:, :A] - f[SF["THETA"]][:, :A])
        dth = np.minimum(dth, np.abs(dth - 2 * np.pi))
        pos_err = max(pos_err, float(np.hypot(dx, dy).max()))
        th_err = max(th_err, float(dth.max()))
        spd_err = max(spd_err, float(np.abs(gf[SF["SPEED"]].astype(np.float64)[:, :A] - f[SF["SPEED"]][:, :A]).max()))
    spw = ora.scen_bank.spawns.reshape(-1, cfg.num_agents + cfg.num_traffic)
    moved = float(np.hypot(f[SF["X"]][:, 0] - spw["x"][scen_ids, 0], f[SF["Y"]][:, 0] - spw["y"][scen_ids, 0]).mean())
    print("free-running 1000 steps, traffic %d: ego pose error %.2e m / %.2e rad, speed %.2e m/s over all %d envs; at the last "
          "step %d of %d envs agree on flags / done / the ego's integer state / env counters; %d env-steps of %d disagreed "
          "somewhere on the way (%d envs, flag bits 0x%x: a line or lane-box edge reached one step apart); episodes ended %d, "
          "mean ego displacement %.0f m"
          % (num_traffic, pos_err, th_err, spd_err, n_envs, int(agree.sum()), n_envs, mism_steps, 1000 * n_envs, int(ever.sum()),
             bits_seen, n_done, moved))
    assert pos_err <= 1e-2 and th_err <= 1e-3
    assert moved > 60.0 and (n_done == 0 or num_traffic > 0)
    # discrete outcomes: a millimetre of drift moves the step at which a box edge is reached, nothing else -- the disagreements
    # are transient (bounded per mille of the env-steps) and >= 97 % of the envs agree at the end
    assert agree.mean() >= 0.97 and mism_steps <= 2e-3 * 1000 * n_envs
    if num_traffic:
        drv_o, drv_g = i[SI["STATUS"]][:, A:] == _abi.ST_ACTIVE, gi[SI["STATUS"]][:, A:] == _abi.ST_ACTIVE
        both = drv_o & drv_g
        div = np.hypot(gf[SF["X"]].astype(np.float64)[:, A:] - f[SF["X"]][:, A:], gf[SF["Y"]].astype(np.float64)[:, A:] - f[SF["Y"]][:, A:])[both]
        vo, vg = float(f[SF["SPEED"]][:, A:][drv_o].mean()), float(gf[SF["SPEED"]][:, A:][drv_g].mean())
        print("  traffic after 1000 free steps: driving %d (oracle) / %d (engine), mean speed %.3f / %.3f m/s, pose difference "
              "median %.2e m, 90 %% %.2e m, max %.2e m" % (int(drv_o.sum()), int(drv_g.sum()), vo, vg, float(np.median(div)),
                                                         float(np.quantile(div, 0.9)), float(div.max())))
        assert abs(int(drv_o.sum()) - int(drv_g.sum())) <= 0.05 * drv_o.sum() + 2 and abs(vo - vg) <= 0.05 * vo
        assert np.median(div) < 1e-2


def test_empty_and_edge_slots(descs):
    """Scenario with zero traffic slots used (density 0) and a NaN action: obs stay finite and in [0,1]."""
    import torch
    n_envs = 16
    eng, ora, cfg = parity.engines(descs, n_envs, density=0.0)
    scen_ids = np.arange(n_envs) % 8
    eng.reset(scen_ids)
    ora.reset(scen_ids)
    act = np.zeros((n_envs, 1, 2), dtype=np.float32)
    act[0, 0, 0] = np.nan
    act[1, 0, 1] = np.inf
    g = eng.step(torch.from_numpy(act).to(eng.device))
    eng.sync()
    o = ora.step(act)
    obs = g[0].cpu().numpy()
    assert np.isfinite(obs).all() and obs.min() >= 0.0 and obs.max() <= 1.0
    assert np.abs(obs - o[0]).max() < OBS_TOL
    assert (obs[:, 0, 34:] == 1.0).all()  # empty scene -> every beam 1.0 (known answer)


@pytest.mark.parametrize("num_agents,capacity,kw", [
    pytest.param(2, 2, {}, id="2-2"), pytest.param(3, 4, {}, id="3-4"), pytest.param(8, 8, {}, id="8-8"), pytest.param(12, 16, {}, id="12-16"),
    pytest.param(40, 40, {}, id="40-40"),
    # an odd beam count (D = 91): rows appended to the step at 8 seats, the four-wave k_observe_env behind it at 40
    pytest.param(8, 8, dict(num_lasers=73), id="8-8-73beams"), pytest.param(40, 40, dict(num_lasers=73), id="40-40-73beams")])
def test_marl_roundabout_parity(num_agents, capacity, kw):
    """BASELINE config 5: multi-agent roundabout (envs/marl_envs/marl_inout_roundabout.py) — per-agent done, delay-done
    queue, respawn into free 8 m x 3 m places, __all__, agent ids; teacher-forced against the oracle."""
    parity.marl_teacher_forced(num_agents, capacity, **kw)


@pytest.mark.parametrize("kind,num_others", [("roundabout", 4), ("intersection", 8)])
def test_marl_neighbour_state_rows_parity(kind, num_others):
    """LidarStateObservationMARound with lidar.num_others > 0 (marl_inout_roundabout.py:82-105): every neighbour row is the
    neighbour's own state vector (19 floats here), finished static neighbours included, zeros when absent."""
    parity.marl_teacher_forced(12, 16, kind=kind, num_others=num_others, others_state=True)


def test_marl_generic_pg_maps_parity():
    """MultiAgentPGDrive itself (multi_agent_pgdrive.py:12-213): 15 agents on the first straight of four generated maps."""
    parity.marl_teacher_forced(15, 15, kind="pg")


def test_marl_intersection_parity():
    """MultiAgentIntersectionEnv (envs/marl_envs/marl_intersection.py): 4-way intersection with u-turns, 30 agents."""
    parity.marl_teacher_forced(30, 30, kind="intersection")


@pytest.mark.parametrize("detectors", [True, False])
def test_marl_bottleneck_parity(detectors):
    """MultiAgentBottleneckEnv (envs/marl_envs/marl_bottleneck.py): Merge / Split blocks, side + lane-line detector fans in
    the multi-agent observation, plain reward, Navigation's own destinations.  Without the side detector obs[0:2] are the
    lateral distances, whose right part is ray-measured on Merge / Split blocks (navigation.py:306-320,346-362)."""
    kw = dict(side_lasers=4, side_dist=50.0, lane_line_lasers=4, lane_line_dist=20.0) if detectors else {}
    parity.marl_teacher_forced(20, 20, kind="bottleneck", plain_reward=True, **kw)


TOLL = dict(tollgate=True, plain_reward=True, side_lasers=72, side_dist=20.0, lane_line_lasers=4, lane_line_dist=20.0,
            num_lasers=72, lidar_dist=20.0, speed_reward=0.0, overspeed_penalty=0.5, min_pass_steps=30)


def test_marl_tollgate_parity():
    """MultiAgentTollgateEnv (envs/marl_envs/marl_tollgate.py): Split -> TollGate -> Merge map with 8 booths (crash_building),
    observation without navigation block + 2 toll floats, overspeed reward, sidewalk-only out-of-road, stay-time rule.
    Half of the agents are teleported to the mouth of the toll plaza, some too fast to pass legally."""
    import torch
    from pgdrive_amd import mapdata
    d, mb, sb = util.make_marl_banks(num_agents=40, n_variants=4, kind="tollgate")
    assert sb.B == 8 and sb.V == 48
    n_envs = 16
    cfg = util.marl_config(n_envs, sb, horizon=400, **TOLL)
    eng, ora = parity.engine(cfg, mb, sb), parity.oracle(cfg, mb, sb)
    assert eng.D == 156
    ids = np.arange(n_envs) % 4
    o0 = ora.reset(ids)
    g0 = eng.reset(ids).cpu().numpy()
    parity.check_reset_rows(eng, ora, g0, o0, 4)
    f, i, ei = ora.get_state()
    SF, SI = _abi.SF, _abi.SI
    rng = np.random.default_rng(3)
    nodes = d["nodes"]
    moved = 0
    for e in range(n_envs):
        sp = sb.spawns[ids[e] * sb.stride:(ids[e] + 1) * sb.stride]
        for a in range(0, 40, 2):
            route = [int(r) for r in sp[a]["ckpt_road"][:sp[a]["n_ckpt"] - 1]]
            toll = [k for k, rid in enumerate(route) if d["roads"][rid]["block_id"] == "$"]
            if not toll:
                continue
            k = toll[0] - 1  # the road that leads into the plaza
            road = d["roads"][route[k]]
            lane_id = road["first_lane"] + 2 * int(rng.integers(0, road["n_lanes"] // 2 + road["n_lanes"] % 2))  # a booth-free lane
            lane = d["lanes"][lane_id]
            lon = max(lane["length"] - rng.uniform(0.5, 6.0), 0.2)
            x, y = mapdata.lane_position(lane, lon, 0.0)
            th = mapdata.lane_heading_at(lane, lon)
            f[SF["X"], e, a], f[SF["Y"], e, a], f[SF["THETA"], e, a] = x, y, th
            f[SF["LASTX"], e, a], f[SF["LASTY"], e, a] = x, y
            f[SF["LASTHX"], e, a], f[SF["LASTHY"], e, a] = np.cos(th), np.sin(th)
            f[SF["SPEED"], e, a] = rng.choice([0.6, 6.0])  # crawl through, or rush (exit after < 30 steps)
            i[SI["LANE"], e, a], i[SI["CK0"], e, a], i[SI["CK1"], e, a] = lane_id, k, k + 1
            moved += 1
    assert moved > 100
    f32 = util.round_state_f32(f)
    ora.set_state(f32, i, ei)
    eng.set_state(f32, i, ei)
    stats = parity.new_stats()
    seen = dict(toll_obs=0, long_stay=0, building=0, fast_exit=0, entries=0, exits=0, int_mismatch=0)
    for t in range(160):
        act = np.zeros((n_envs, 40, 2), dtype=np.float32)
        act[..., 0] = np.clip(rng.normal(0, 0.03, size=(n_envs, 40)), -1, 1)
        act[..., 1] = np.where(np.arange(40) % 4 == 0, 0.02, 0.4)[None, :]
        o_obs, o_rew, o_done, o_flags = ora.step(act)
        mg = ora.margins()
        g_obs, g_rew, g_done, g_flags = eng.step(torch.from_numpy(act).to(eng.device))
        eng.sync()
        g_obs = g_obs.cpu().numpy().astype(np.float64)
        gfl = g_flags.cpu().numpy().astype(np.uint32)
        same = (gfl == o_flags) & (g_done.cpu().numpy() == o_done)
        stats["steps"] += same.size
        stats["flag_mismatch"] += int((~same).sum())
        # ray-cast columns (side fan 0:72, lane-line fan 78:82, lidar 82:154) over OBS_TOL: margin-verified grazing or stats["obs"]
        parity.compare_rows(eng, ora, stats, g_obs, o_obs, same, mg)
        stats["rew"] = max(stats["rew"], float(np.abs(g_rew.cpu().numpy() - o_rew)[same].max()))
        rep = (o_flags & _abi.F_REPORT) != 0
        seen["toll_obs"] += int((o_obs[..., -2][rep] > 0).sum())
        seen["long_stay"] += int((o_obs[..., -1][rep] > 0).sum())
        seen["building"] += int(((o_flags & _abi.F_CRASH_BUILDING) != 0).sum())
        f, i, ei = ora.get_state()
        gf, gi, gei = eng.get_state()
        seen["int_mismatch"] += int((gi != i).any(axis=0).sum()) + int((gei != ei).any(axis=0).sum())
        for fld in ("PID_HP", "PID_HI", "PID_LP", "PID_LI"):  # toll bookkeeping (integer-valued floats) must be exact
            assert (gf[SF[fld]][:, :40] == f[SF[fld]][:, :40].astype(np.float32)).all(), fld
        seen["entries"] = max(seen["entries"], int((f[SF["PID_HI"]][:, :40] >= 0).sum()))
        seen["exits"] = max(seen["exits"], int((f[SF["PID_LP"]][:, :40] >= 0).sum()))
        fast = (f[SF["PID_HI"]][:, :40] >= 0) & (f[SF["PID_LP"]][:, :40] >= 0) & \
               (f[SF["PID_LP"]][:, :40] - f[SF["PID_HI"]][:, :40] < 30)
        seen["fast_exit"] = max(seen["fast_exit"], int(fast.sum()))
        f32 = util.round_state_f32(f)
        ora.set_state(f32, i, ei)
        eng.set_state(f32, i, ei)
    print("tollgate parity:", stats, seen)
    parity.report("tollgate parity", stats)
    stats["grazing"], stats["beams"] = stats["grazing"] + stats["det_grazing"], stats["beams"] + stats["det_beams"]  # all three fans, as before
    assert stats["obs"] < OBS_TOL and stats["rew"] < REW_TOL and stats["flag_mismatch"] == 0 and stats.get("flag_ties", 0) == 0 and seen["int_mismatch"] == 0
    assert stats["grazing"] <= 1e-4 * stats["beams"] + 5
    assert seen["toll_obs"] > 500 and seen["long_stay"] > 50 and seen["entries"] > 20 and seen["exits"] > 10 and seen["building"] > 10
    assert seen["fast_exit"] >= 5


def test_marl_parking_lot_parity():
    """MultiAgentParkingLotEnv (envs/marl_envs/marl_parking_lot.py): ParkingLot block, reverse driving (enable_reverse),
    destinations handed out from the pool of free parking spaces (released when an agent is done, respawn from the access
    roads only while a space is free), white lines may be crossed."""
    parity.marl_teacher_forced(10, 10, kind="parking", parking=True, enable_reverse=True)


@pytest.mark.parametrize("kind,kw", [("intersection", {}), ("bottleneck", dict(plain_reward=True, side_lasers=4, side_dist=50.0,
                                                                               lane_line_lasers=4, lane_line_dist=20.0)),
                                     ("parking", dict(parking=True, enable_reverse=True)), ("tollgate", dict(TOLL))])
def test_marl_eight_agents_parity(kind, kw):
    """Every multi-agent map once more with 8 agents (few slots, quick respawn turnover).  (Fusing the multi-agent
    observation into k_step for <= 8 slots was built and measured: 93.9 us fused vs 41 + 57 us separate at 4096 envs x 8
    agents -- no gain, the 8 rows are serial in one wave -- so the stand-alone k_observe stays.)"""
    parity.marl_teacher_forced(8, 8, kind=kind, **kw)


def test_full_size_properties():
    """BASELINE configuration C3 at full size (4096 envs x 17 slots x 240 beams, 100 maps) through size-independent
    properties: every observation is finite and inside [0, 1]; done / reward / flags are consistent; envs do not influence
    each other -- the first 32 envs of the 4096-batch produce bit-identical outputs to a 32-env engine fed the same
    scenarios and actions; the run is reproducible; a checkpoint (get_state -> set_state) resumes bit-identically."""
    import torch
    from pgdrive_amd import bank, mapdata, scenario
    descs = bank.get_descriptions(range(1000, 1100))
    mb = mapdata.MapBank(descs)
    sb = scenario.ScenarioBank(descs, [d["seed"] for d in descs], num_agents=1, num_traffic=16)
    N, n = 4096, 32

    def make(n_envs):
        return parity.engine(_abi.make_config(n_envs, num_agents=1, num_traffic=16, num_lasers=240, auto_reset=1, seed=99), mb, sb)

    big, small, twin = make(N), make(n), make(N)
    ids = (np.arange(N) * 7) % 100
    ob = big.reset(ids).clone()
    osm = small.reset(ids[:n]).clone()
    twin.reset(ids)
    assert torch.equal(ob[:n], osm)
    rng = np.random.default_rng(4)
    n_done = n_reset = 0
    ckpt = None
    for t in range(120):
        a = rng.uniform(-1, 1, size=(N, 1, 2)).astype(np.float32)
        a[:, 0, 1] = np.abs(a[:, 0, 1]) * 0.8  # keep moving: episodes end and auto-reset inside the run
        act = torch.from_numpy(a).to(big.device)
        o1, r1, d1, f1 = [x.clone() for x in big.step(act)]
        o2, r2, d2, f2 = small.step(act[:n].contiguous())
        o3, r3, d3, f3 = twin.step(act)
        big.sync(); small.sync(); twin.sync()
        assert torch.isfinite(o1).all() and float(o1.min()) >= 0.0 and float(o1.max()) <= 1.0
        assert torch.equal(o1[:n], o2) and torch.equal(r1[:n], r2) and torch.equal(d1[:n], d2) and torch.equal(f1[:n], f2)
        assert torch.equal(o1, o3) and torch.equal(r1, r3) and torch.equal(f1, f3)  # reproducible
        fl = f1.cpu().numpy().astype(np.uint32)[:, 0]
        dn = d1.cpu().numpy()[:, 0]
        term = (fl & (_abi.F_ARRIVE | _abi.F_OUT_OF_ROAD | _abi.F_CRASH_VEHICLE | _abi.F_MAX_STEP)) != 0
        assert ((dn == 1) == term).all() and (((fl & _abi.F_RESET) != 0) == (dn == 1)).all()
        rw = r1.cpu().numpy()[:, 0]
        assert (rw[(fl & _abi.F_ARRIVE) != 0] == 10.0).all()
        assert (rw[((fl & _abi.F_OUT_OF_ROAD) != 0) & ((fl & _abi.F_ARRIVE) == 0)] == -5.0).all()
        n_done += int(dn.sum())
        if t == 60:
            ckpt = big.get_state()
            tail = []
        if t > 60:
            tail.append((act, o1))
    assert n_done > 500
    # checkpoint / resume: restart a fresh engine from the step-60 state and replay the remaining actions
    resumed = make(N)
    resumed.reset(ids)
    resumed.set_state(*ckpt)
    for act, o_ref in tail:
        o4 = resumed.step(act)[0]
        resumed.sync()
        assert torch.equal(o4, o_ref)


def test_throughput_mode_at_32768_envs_properties():
    """BASELINE config 4's per-node size on one GPU: 32768 envs x 17 slots x 240 beams, where pgd_create picks the throughput mode
    by itself (three whole envs per wave, one vehicle per lane, rows appended to the launch) -- the instantiation bench.py's
    `c3_32768` row times.  Size-independent properties: observations finite and inside [0, 1]; done <-> terminal flags <->
    restart consistent, terminal rewards exact; envs do not influence each other and the mode does not change results -- the
    first 96 envs (whole waves) and 61 envs starting at an odd offset equal, flag for flag, small engines in the DEFAULT mode
    (one env per wave) fed the same scenarios, actions and global env indices (rows to the contraction of multiply-adds);
    the run is reproducible bit for bit; a checkpoint resumes bit-identically; grouped stepping (pgd_set_groups on a
    power-of-two size leaves throughput mode: ADVICE r03) gives the same rows as whole-engine steps of a default-mode engine."""
    import torch
    from pgdrive_amd import bank, mapdata, scenario
    descs = bank.get_descriptions(range(1000, 1100))
    mb = mapdata.MapBank(descs)
    sb = scenario.ScenarioBank(descs, [d["seed"] for d in descs], num_agents=1, num_traffic=16)
    N = 32768

    def make(n_envs, base=0):
        return parity.engine(_abi.make_config(n_envs, num_agents=1, num_traffic=16, num_lasers=240, auto_reset=1, resample_scenario=1,
                                       seed=77, env_base=base), mb, sb)

    big, twin = make(N), make(N)
    windows = [(0, 96), (12345, 61)]
    small = [make(n, base=lo) for lo, n in windows]
    ids = (np.arange(N) * 7) % 100
    big.reset(ids); twin.reset(ids)
    for (lo, n), e in zip(windows, small):
        e.reset(ids[lo:lo + n])
    rng = np.random.default_rng(14)
    n_done = 0
    worst = worst_ray = 0.0
    n_ray = n_ray_over = 0
    ckpt, tail = None, []
    for t in range(90):
        a = rng.uniform(-1, 1, size=(N, 1, 2)).astype(np.float32)
        a[:, 0, 1] = np.abs(a[:, 0, 1]) * 0.8
        act = torch.from_numpy(a).to(big.device)
        o1, r1, d1, f1 = [x.clone() for x in big.step(act)]
        o3, r3, d3, f3 = twin.step(act)
        big.sync(); twin.sync()
        if t == 0:
            assert "throughput mode" in big.describe_step() and "throughput mode" not in small[0].describe_step()
        assert torch.isfinite(o1).all() and float(o1.min()) >= 0.0 and float(o1.max()) <= 1.0
        assert torch.equal(o1, o3) and torch.equal(r1, r3) and torch.equal(d1, d3) and torch.equal(f1, f3)
        for (lo, n), e in zip(windows, small):
            o2, r2, d2, f2 = e.step(act[lo:lo + n].contiguous())
            e.sync()
            assert torch.equal(d1[lo:lo + n], d2) and torch.equal(f1[lo:lo + n], f2), "flags differ from the default mode at step %d" % t
            dd = (o1[lo:lo + n] - o2).abs()
            # (round 6: the dynamics spell their fused multiply-adds out -- pgd_dynamics.h -- so the two instantiations carry bit-identical
            # poses from step to step; what is left is the last bit of a few observation columns, not a drift: every column, the ray
            # columns included, agrees to 2e-6 again.  With the -O2 build of round 5 a few beams in a million differed by up to 1.4e-5.)
            worst = max(worst, float(dd[..., :34].max()), float((r1[lo:lo + n] - r2).abs().max()) * 0.05)
            worst_ray = max(worst_ray, float(dd[..., 34:].max()))
            n_ray += int(dd[..., 34:].numel())
            n_ray_over += int((dd[..., 34:] > 2e-6).sum())
        fl = f1.cpu().numpy().astype(np.uint32)[:, 0]
        dn = d1.cpu().numpy()[:, 0]
        term = (fl & (_abi.F_ARRIVE | _abi.F_OUT_OF_ROAD | _abi.F_CRASH_VEHICLE | _abi.F_MAX_STEP)) != 0
        assert ((dn == 1) == term).all() and (((fl & _abi.F_RESET) != 0) == (dn == 1)).all()
        rw = r1.cpu().numpy()[:, 0]
        assert (rw[(fl & _abi.F_ARRIVE) != 0] == 10.0).all()
        assert (rw[((fl & _abi.F_OUT_OF_ROAD) != 0) & ((fl & _abi.F_ARRIVE) == 0)] == -5.0).all()
        n_done += int(dn.sum())
        if t == 50:
            ckpt = big.get_state()
        if t > 50:
            tail.append((act, o1))
    assert n_done > 3000 and worst < 2e-6 and worst_ray < 2e-6, (n_done, worst, worst_ray)
    assert n_ray > 3_000_000 and n_ray_over == 0, (n_ray_over, n_ray)
    resumed = make(N)
    resumed.reset(ids)
    resumed.set_state(*ckpt)
    for act, o_ref in tail:
        o4 = resumed.step(act)[0]
        resumed.sync()
        assert torch.equal(o4, o_ref)
    # grouped stepping: 32768 / 2 is not a multiple of three envs per wave -> the engine leaves throughput mode (it used to refuse)
    twin.set_groups(2)
    a = rng.uniform(-1, 1, size=(N, 1, 2)).astype(np.float32)
    act = torch.from_numpy(a).to(big.device)
    for g in range(2):
        twin.step_group(g, act)
    for g in range(2):
        twin.group_sync(g)
    o_ref, r_ref, d_ref, f_ref = big.step(act)
    big.sync()
    # (the switch is reported, not silent -- the kernel named is the one-env-per-wave one, and the line says why)
    desc = twin.describe_step()
    assert desc.startswith("k_step: one env per wave") and "throughput mode switched off by pgd_set_groups" in desc
    assert "throughput" in big.describe_step() and "switched off" not in big.describe_step()
    dd = (twin.obs - o_ref).abs()
    assert torch.equal(twin.done, d_ref) and torch.equal(twin.flags, f_ref)
    assert float(dd.max()) < 2e-6  # (every column, as above)


@pytest.mark.parametrize("num_traffic", [16, 24, 40])  # 3, 2, 1 sub-lanes per vehicle slot
def test_record_cache_matches_plain_records(descs, num_traffic):
    """The step kernel skips the write of a record that did not change and reads never-written slots from the scenario's
    reset image (the throughput mode's default; with one env per wave the image reads are off by default since round 5 -- the mask
    is a memory round trip in front of the records -- and PGD_IMASK=1 switches them on: this test).  Engine A runs freely with both short cuts; engine B gets A's complete state through get_state /
    set_state before every step (set_state drops the image marks, so B reads its own records).  Same kernel, same inputs:
    every output must be bit-identical, through terminations, auto-resets with re-drawn scenarios, a partial pgd_reset
    and a scenario re-upload in the middle of the run.  (A free-running env also keeps its own copy of the map header, which
    set_state rebuilds: with fewer than four sub-lanes per slot the copy used to follow a re-drawn scenario only in part.)"""
    import torch
    n_envs = 96
    eng_a, _, _ = parity.engines(descs, n_envs, env=dict(PGD_IMASK="1"), seed=5, num_traffic=num_traffic, resample_scenario=1)
    eng_b, _, _ = parity.engines(descs, n_envs, env=dict(PGD_IMASK="1"), seed=5, num_traffic=num_traffic, resample_scenario=1)
    scen_ids = np.arange(n_envs) % 8
    eng_a.reset(scen_ids)
    eng_b.reset(scen_ids)
    rng = np.random.default_rng(3)
    n_done = n_pending_rows = 0
    for t in range(260):
        act = util.driving_actions(rng, n_envs)
        if t % 3 == 0:  # a third of the steps: hard steering at full throttle, episodes end quickly
            act[::2, 0, 0] = 1.0
            act[::2, 0, 1] = 1.0
        if t == 90:  # a partial reset of A (then mirrored into B through the state)
            ids = np.arange(0, n_envs, 5)
            eng_a.reset((ids + 3) % 8, env_ids=ids)
        if t == 170:  # the same scenarios uploaded again: A falls back to its own records until the next reset
            sb = eng_a.scen
            from pgdrive_amd.engine import _chk, _np_p
            _chk(eng_a.L.pgd_upload_scenarios(eng_a.h, _np_p(sb.scenarios), len(sb.scenarios), _np_p(sb.spawns)), "upload")
        f, i, ei = eng_a.get_state()
        eng_b.set_state(f, i, ei)
        n_pending_rows += int((i[_abi.SI["STATUS"], :, 1:] == 1).sum())
        ga = [x.clone() for x in eng_a.step(torch.from_numpy(act).to(eng_a.device))]
        gb = [x.clone() for x in eng_b.step(torch.from_numpy(act).to(eng_b.device))]
        eng_a.sync(); eng_b.sync()
        parity.same_bits(t, ga, gb, eng_a, eng_b)
        n_done += int(ga[2].sum().item())
    print("record cache: episodes ended", n_done, "waiting-traffic rows seen", n_pending_rows)
    assert n_done > 50 and n_pending_rows > 10000


@pytest.mark.parametrize("decision_repeat,lidar_dist", [(20, 50.0), (10, 50.0), (5, 8.0)])
def test_contact_hint_with_long_steps_and_short_lidar(descs, decision_repeat, lidar_dist):
    """The fused observation leaves a per-env hint "no body can reach an agent during the next step" that lets k_step skip its
    contact tests.  Its reach is t_step = dt * decision_repeat seconds of driving, and it only sees bodies inside the lidar
    range: with decision_repeat = 10 (0.2 s steps) or a lidar shorter than two reaches the round-2 constant (0.105 s, any
    range) let fast closing vehicles collide unnoticed.  Engine A runs freely with the hint; engine B gets A's state through
    set_state before every step (which forces the contact tests on): crash flags, done and state must be bit-identical."""
    n_envs = 96
    kw = dict(seed=5, decision_repeat=decision_repeat, lidar_dist=lidar_dist, density=0.3)
    eng_a, _, _ = parity.engines(descs, n_envs, **kw)
    eng_b, _, _ = parity.engines(descs, n_envs, **kw)
    scen_ids = np.arange(n_envs) % 8
    eng_a.reset(scen_ids)
    eng_b.reset(scen_ids)
    rng = np.random.default_rng(4)
    n_crash = n_done = 0

    def actions(t):
        act = util.driving_actions(rng, n_envs)
        act[:, 0, 0] *= 0.2
        act[:, 0, 1] = 1.0  # straight on at full throttle: the ego runs into the traffic ahead of it at speed
        return act

    for t, ga, gb in parity.twins(eng_a, eng_b, 300, actions, copy_state=eng_a):
        parity.same_bits(t, ga, gb)
        n_crash += int(((ga[3].cpu().numpy().astype(np.uint32) & _abi.F_CRASH_VEHICLE) != 0).sum())
        n_done += int(ga[2].sum().item())
    print("contact hint A/B, decision_repeat %d, lidar %.0f m: crashes %d, episodes %d" % (decision_repeat, lidar_dist, n_crash, n_done))
    assert n_crash > 30


def test_config_combinations_fuzz(descs):
    """Random combinations of every engine switch (action modes, detector fans, noise, objects, traffic modes, horizon,
    Safe env, random_agent_model ...), 20 short teacher-forced runs against the oracle.  (240 such combinations were run once
    with tools-style seeds 1-4: clean apart from the IDM 30 m tie of profiles/r01_parity_campaign.md at density 0.3.)"""
    master = np.random.default_rng(20260928)
    for trial in range(20):
        r = master
        kw = dict(
            num_traffic=int(r.choice([0, 5, 16])), num_lasers=int(r.choice([0, 30, 72, 240])), num_others=int(r.choice([0, 2, 4])),
            side_lasers=int(r.choice([0, 0, 2, 7])), side_dist=50.0, lane_line_lasers=int(r.choice([0, 0, 4])),
            lane_line_dist=20.0, discrete_action=bool(r.integers(2)), increment_steering=bool(r.integers(2)),
            horizon=int(r.choice([0, 0, 40])), safe_rl_env=bool(r.integers(2)), random_agent_model=bool(r.integers(2)),
            traffic_mode=str(r.choice(["trigger", "respawn", "hybrid"])), auto_termination=bool(r.integers(2)),
            accident_prob=float(r.choice([0.0, 0.0, 0.8])), density=float(r.choice([0.05, 0.1])),
            lidar_gaussian_noise=float(r.choice([0.0, 0.0, 0.02])), lidar_dropout_prob=float(r.choice([0.0, 0.0, 0.05])),
            seed=int(r.integers(1000)))
        if kw["num_traffic"] == 0:
            kw["accident_prob"] = 0.0
        if kw["num_lasers"] == 0:
            kw.update(num_others=0, lidar_gaussian_noise=0.0, lidar_dropout_prob=0.0)
        n_envs = 32
        eng, ora, cfg = parity.engines(descs, n_envs, n_maps=8, **kw)
        ids = np.arange(n_envs) % 8
        o0 = ora.reset(ids)
        g0 = eng.reset(ids).cpu().numpy()
        assert np.abs(g0 - o0).max() < OBS_TOL, kw
        rng = np.random.default_rng(trial)
        st = parity.new_stats()
        for _ in parity.teacher_forced(eng, ora, st, 100, lambda t: rng.integers(0, 5, size=(n_envs, 1, 2)).astype(np.float32)
                                       if kw["discrete_action"] else util.driving_actions(rng, n_envs)):
            pass
        parity.report("fuzz trial %d" % trial, st)
        # (flags that differ: only margin-verified CONTACT / ROUTE / LANE ties, at most the two a trial was allowed before)
        assert st["obs"] < OBS_TOL and st["rew"] < REW_TOL and st["flag_mismatch"] == 0 and st["flag_ties"] <= 2, (kw, st)
        parity.close_engines()


def test_marl_config_combinations_fuzz():
    """Random combinations of the multi-agent switches (map kind, agent count / capacity, crash_done, out_of_road_done,
    allow_respawn, delay_done, horizon, neighbour-state rows, detector fans), 16 teacher-forced runs against the oracle.
    (120 such combinations were run once: clean apart from ties of the kind profiles/r01_parity_campaign.md lists -- two
    neighbours at the same distance ranked by the last bit, the engine-force cut-off exactly at max_speed.)"""
    r = np.random.default_rng(1)
    for trial in range(int(os.environ.get("PGD_FUZZ_TRIALS", "16"))):  # (PGD_FUZZ_TRIALS=120: the one-off campaign of the docstring)
        kind = str(r.choice(["roundabout", "intersection", "bottleneck", "parking", "pg"]))
        na = int(r.choice([4, 8, 12]))
        cap = int(r.choice([na, na + 4]))
        if kind == "pg":
            cap = min(cap, 15)
            na = min(na, cap)
        if kind == "parking":
            na = min(na, 10)
        no = int(r.choice([0, 0, 3]))
        kw = dict(crash_done=bool(r.integers(2)), out_of_road_done=bool(r.integers(2)), allow_respawn=bool(r.integers(4) > 0),
                  delay_done=int(r.choice([0, 5, 25])), horizon=int(r.choice([60, 150, 1000])), num_others=no,
                  others_state=no > 0, side_lasers=int(r.choice([0, 0, 4])), side_dist=50.0,
                  lane_line_lasers=int(r.choice([0, 0, 4])), lane_line_dist=20.0, seed=int(r.integers(1000)))
        if kind == "bottleneck":
            kw.update(plain_reward=True, cross_yellow_line_done=bool(r.integers(2)))
        if kind == "parking":
            kw.update(parking=True, enable_reverse=True)
        d, mb, sb = util.make_marl_banks(num_agents=na, capacity=cap, kind=kind)
        n_envs = 24
        cfg = util.marl_config(n_envs, sb, **kw)
        eng, ora = parity.engine(cfg, mb, sb), parity.oracle(cfg, mb, sb)
        ids = np.arange(n_envs) % len(sb.scenarios)
        assert np.abs(eng.reset(ids).cpu().numpy() - ora.reset(ids)).max() < OBS_TOL
        rng = np.random.default_rng(trial)
        st = parity.new_stats()
        for s in parity.teacher_forced(eng, ora, st, 200, lambda t: util.marl_actions(rng, n_envs, sb.A)):
            s.int_ties()
        parity.report("marl fuzz trial %d" % trial, st)
        assert st["obs"] < OBS_TOL and st["rew"] < REW_TOL and st["flag_mismatch"] == 0 and st["flag_ties"] <= 2, (kind, na, cap, kw, st)
        assert st["int_mismatch"] == 0, (kind, na, cap, kw, st)
        assert st["int_ties"] <= 2, (kind, na, cap, kw, st)
        parity.close_engines()


def test_contacts_inside_the_sub_steps(descs):
    """collision_callback.py:7-36 runs inside each of the 5 doPhysics calls of a step (engine_core.py:276-278): a fast car
    that clips a corner in the middle of the 0.1 s step and is clear again at its end has crashed.  Egos are teleported next
    to a waiting traffic vehicle at 10-25 m/s with random headings / steering; GPU and oracle must agree flag for flag, and
    some of the crash_vehicle flags must belong to pairs whose END-of-step boxes do not overlap."""
    n_envs = 512
    eng, ora, cfg = parity.engines(descs, n_envs, seed=21, auto_reset=0)  # no auto-reset: the state after the crash stays
    scen_ids = np.arange(n_envs) % 8
    ora.reset(scen_ids)
    eng.reset(scen_ids)
    sb = ora.scen_bank
    V = sb.V
    rng = np.random.default_rng(31)
    SF, SI = _abi.SF, _abi.SI
    stats = parity.new_stats()
    n_crash = n_mid_only = 0
    f0, i0, ei0 = ora.get_state()
    for rnd in range(8):
        f, i, ei = f0.copy(), i0.copy(), ei0.copy()
        tgt = np.zeros(n_envs, dtype=int)
        for e in range(n_envs):
            cand = np.nonzero(i[SI["STATUS"], e, 1:] == _abi.ST_PENDING)[0] + 1
            k = int(cand[rng.integers(len(cand))])
            tgt[e] = k
            ang, dist = rng.uniform(0, 2 * np.pi), rng.uniform(2.2, 5.2)
            f[SF["X"], e, 0] = f[SF["X"], e, k] + dist * np.cos(ang)
            f[SF["Y"], e, 0] = f[SF["Y"], e, k] + dist * np.sin(ang)
            f[SF["THETA"], e, 0] = rng.uniform(-np.pi, np.pi)
            f[SF["SPEED"], e, 0] = rng.uniform(10.0, 25.0)
            f[SF["HX"], e, 0] = f[SF["HY"], e, 0] = 0.0  # edited heading: the engine derives the vector from THETA
        f32 = util.round_state_f32(f)
        ora.set_state(f32, i, ei)
        eng.set_state(f32, i, ei)
        act = rng.uniform(-1, 1, size=(n_envs, 1, 2)).astype(np.float32)
        parity.compare_step(eng, ora, act, stats)
        gf, gi, gei = eng.get_state()
        fl = eng.flags.cpu().numpy().astype(np.uint32)[:, 0]
        crash = (fl & _abi.F_CRASH_VEHICLE) != 0
        ee = np.arange(n_envs)
        spw = sb.spawns.reshape(-1, V) if sb.spawns.ndim == 1 else sb.spawns
        sp_e = spw[scen_ids]
        # end-of-step boxes of the ego and of EVERY other present body
        cont = np.ones(n_envs, dtype=bool)
        end_any = np.zeros(n_envs, dtype=bool)
        for k in range(1, V):
            pres = np.isin(gi[SI["STATUS"], :, k], (_abi.ST_PENDING, _abi.ST_ACTIVE))
            end_any |= pres & parity.np_obb_overlap(gf[SF["X"], :, 0], gf[SF["Y"], :, 0], gf[SF["THETA"], :, 0], sp_e["length"][:, 0],
                                              sp_e["width"][:, 0], gf[SF["X"], :, k], gf[SF["Y"], :, k], gf[SF["THETA"], :, k],
                                              sp_e["length"][:, k], sp_e["width"][:, k])
        n_crash += int(crash.sum())
        n_mid_only += int((crash & cont & ~end_any).sum())
        assert not (end_any & cont & ~crash).any()  # an overlap at the end of the step is a contact, always
    print("sub-step contacts:", stats, "crash_vehicle", n_crash, "of which clear again at the end of the step", n_mid_only)
    assert stats["flag_mismatch"] == 0 and stats.get("flag_ties", 0) == 0 and stats["obs"] < OBS_TOL
    assert n_crash > 300 and n_mid_only >= 5


@pytest.mark.parametrize("kind,num_agents,capacity,kw", [
    ("roundabout", 8, 8, dict(num_others=4)),
    ("roundabout", 12, 16, dict(num_others=4, num_lasers=240, lidar_dist=50.0)),
    ("roundabout", 40, 40, dict(num_others=2, lidar_gaussian_noise=0.05, lidar_dropout_prob=0.1)),
    ("tollgate", 12, 12, dict(TOLL, num_others=4)),
    ("bottleneck", 20, 20, dict(plain_reward=True, side_lasers=4, side_dist=50.0, lane_line_lasers=4, lane_line_dist=20.0)),
    ("roundabout", 12, 16, dict(num_others=4, others_state=True)),  # neighbour rows = the neighbours' own state vectors
    ("intersection", 30, 30, dict(num_others=8, others_state=True)),
    ("roundabout", 8, 8, dict(num_lasers=73)),  # an odd row width, D = 91
    ("roundabout", 40, 40, dict(num_lasers=73)),
])
def test_env_observation_kernel_equals_row_kernel(kind, num_agents, capacity, kw):
    """The multi-agent observation comes from k_observe_env (one wave per env: all agents' state blocks at once, lidar
    as flattened body-beam incidences with an LDS min).  PGD_ROW_OBSERVE keeps the one-block-per-row kernel that the
    oracle parity tests were first run with: free-running engines, same actions.  Reward, done and flags come from the same
    k_step and must be bit-identical; the two observation kernels contract their multiply-adds differently, so the rows agree
    to an fp32 ulp or two (1e-6), up to a beam that grazes a box corner."""
    d, mb, sb = util.make_marl_banks(num_agents=num_agents, capacity=capacity, kind=kind)
    n_envs = 48
    cfg = util.marl_config(n_envs, sb, horizon=150, resample_scenario=1, seed=9, **kw)
    eng_a = parity.engine(cfg, mb, sb)
    eng_b = parity.engine(cfg, mb, sb, env=dict(PGD_ROW_OBSERVE="1"))
    ids = np.arange(n_envs) % len(sb.scenarios)
    nl = cfg.num_lasers
    tail = 2 if kw.get("tollgate") else 0  # the toll floats follow the lidar
    st = dict(beams=0, grazing=0, worst=0.0)
    parity.rows_close(eng_a.reset(ids), eng_b.reset(ids), st, nl, 1e-6, tail)
    rng = np.random.default_rng(4)
    n_rows = n_new = 0
    for t, ga, gb in parity.twins(eng_a, eng_b, 260, lambda t: util.marl_actions(rng, n_envs, sb.A)):
        parity.same_rows(t, ga, gb, st, nl, 1e-6, tail)
        fl = ga[3].cpu().numpy()
        n_rows += int(((fl & _abi.F_REPORT) != 0).sum())
        n_new += int(((fl & _abi.F_NEW) != 0).sum())
    print("env vs row observation kernel:", st, "rows", n_rows, "new agents", n_new)
    assert st["worst"] < 1e-6 and st["grazing"] <= 1e-5 * st["beams"] + 2
    assert n_rows > 5000 and n_new > 20


def test_maround_rows_against_the_reference_fixture(descs):
    """tests/golden/maround_v0.json holds rows of the reference's LidarStateObservationMARound.observe (own state, the state
    vectors of the four nearest detected vehicles, 240 beams) computed by the reference's Python on scenes where every vehicle
    is an agent: the engine's PGD_MA_OTHERS_STATE observation (k_observe<.., OTH>) must reproduce them from the same state."""
    import json
    from tests.test_oracle_golden import GOLD, agents_scene_banks, agents_scene_state, compare_maround_rows
    with open(os.path.join(GOLD, "maround_v0.json")) as fh:
        gold = json.load(fh)
    worst = dict(state=0.0, others=0.0, lidar=0.0, rows=0, absent=0)
    flips = 0
    for sc in gold["cases"]:
        mb, sb, cfg = agents_scene_banks(descs, sc, num_lasers=240, lidar_dist=50.0, num_others=gold["num_others"], others_state=True)
        eng = parity.engine(cfg, mb, sb)
        eng.reset(np.zeros(1, dtype=np.int32))
        f, i, ei = eng.get_state()
        agents_scene_state(sc, f, i)
        eng.set_state(f, i, ei)
        obs = eng.observe()
        eng.sync()
        # corner beams: the reference helper pads box edges by 1e-5, fp32 adds its own grazing cases (bounded below)
        flips += compare_maround_rows(sc, obs.cpu().numpy()[0], worst, beam_tol=OBS_TOL)
        parity.close_engines()
    print("MARound rows on the GPU:", worst, "corner beams", flips)
    assert worst["rows"] >= 50 and worst["state"] < OBS_TOL and worst["others"] < OBS_TOL and worst["lidar"] <= OBS_TOL and flips <= 4


@pytest.mark.parametrize("case", ["c3", "c2", "c2_fans", "marl8", "marl8_240"])
def test_fused_observation_equals_stand_alone_kernels(descs, case):
    """One launch per step: the single-agent row (k_step's own wave), the state-only row of several envs per wave, and the
    multi-agent rows (observe_env_body appended to k_step) are written by the step kernel.  PGD_NO_FUSE keeps the stand-alone
    observation kernels after k_step: same engine otherwise, free-running with the same actions -- reward / done / flags
    bit-identical, rows equal up to the contraction of multiply-adds in the two code instances (1e-6; grazing beams counted)."""
    n_envs = 64
    if case.startswith("marl"):
        d, mb, sb = util.make_marl_banks(num_agents=8, capacity=8, kind="roundabout")
        kw = dict(num_others=4, num_lasers=240, lidar_dist=50.0) if case == "marl8_240" else dict(num_others=4)
        cfg = util.marl_config(n_envs, sb, horizon=150, resample_scenario=1, seed=2, **kw)
        A = sb.A
    else:
        nt, nl = (16, 240) if case == "c3" else (0, 0)
        mb, sb = util.make_banks(descs, n_maps=8, num_traffic=nt)
        fans = dict(side_lasers=6, side_dist=50.0, lane_line_lasers=4, lane_line_dist=20.0) if case == "c2_fans" else {}
        cfg = _abi.make_config(n_envs, num_agents=1, num_traffic=nt, num_lasers=nl, auto_reset=1, seed=2, resample_scenario=1, **fans)
        A = 1
    eng_a = parity.engine(cfg, mb, sb)
    eng_b = parity.engine(cfg, mb, sb, env=dict(PGD_NO_FUSE="1"))
    ids = np.arange(n_envs) % len(sb.scenarios)
    eng_a.reset(ids); eng_b.reset(ids)
    rng = np.random.default_rng(8)
    st = dict(beams=0, grazing=0, worst=0.0)
    n_done = 0
    for t, ga, gb in parity.twins(eng_a, eng_b, 240, lambda t: util.marl_actions(rng, n_envs, A) if A > 1 else util.driving_actions(rng, n_envs)):
        parity.same_rows(t, ga, gb, st, cfg.num_lasers, 1e-6)
        n_done += int(ga[2].sum().item())
    print("fused vs stand-alone observation", case, "worst", st["worst"], "grazing", st["grazing"], "of", st["beams"], "episodes", n_done)
    assert st["worst"] < 1e-6 and st["grazing"] <= 1e-5 * st["beams"] + 2 and n_done > 10


LARGE_RUNS = pytest.mark.skipif(bool(os.environ.get("PGD_SKIP_LARGE_RUNS")), reason="PGD_SKIP_LARGE_RUNS is set")


@pytest.mark.parametrize("size", ["suite", pytest.param("large", marks=LARGE_RUNS)])
def test_free_running_timed_path_through_episode_ends(descs, size):
    """(size "large": the one-off 2048 x 1500 run of round 4, at 1024 envs x 1000 steps, now part of the suite with its tie classes
    asserted -- VERDICT r04 item 7; PGD_SKIP_LARGE_RUNS=1 leaves it out, PGD_FREE_RUN="envs,steps" sets another size.)
    The path bench.py times, held to the oracle directly (not through self-comparisons): engine defaults -- contact / trigger
    hints carried from step to step, the reset-image mask, auto-reset from the reset image with a re-drawn scenario
    (resample_scenario = 1) -- and NO set_state between the steps (teacher forcing resets the hints and the mask).  256 envs x 600
    steps of driving actions, the same float32 stream on both sides.  Per env the two runs are compared until the env's first
    DISCRETE divergence (done / flags differ: a contact or a line reached one step apart between fp32 and fp64 -- from there on
    the two envs play different episodes, also in the reference's own fp64 if a coordinate moves by one ulp):
      * episode ends in the common prefix agree on the step and on the whole flag set, and they are most of all ends;
      * a restart is exact: the step that reports F_RESET hands out the first observation of the re-drawn scenario, equal on
        both sides to the observation tolerance -- no divergence begins at a reset;
      * observations in the common prefix stay within the teacher-forced tolerance while the env's traffic is parked and
        within a loose bound after it drives (the IDM traffic is a chaotic closed loop: DESIGN.md section 7)."""
    import torch
    n_envs, n_steps = (256, 600) if size == "suite" else (1024, 1000)
    big = os.environ.get("PGD_FREE_RUN")  # "envs,steps": another size for the large run
    if big and size == "large":
        n_envs, n_steps = (int(x) for x in big.split(","))
    eng, ora, cfg = parity.engines(descs, n_envs, seed=11, resample_scenario=1, auto_reset=1)
    ids = np.arange(n_envs) % 8
    o0 = ora.reset(ids)
    g0 = eng.reset(ids).cpu().numpy()
    assert np.abs(g0 - o0).max() < OBS_TOL
    rng = np.random.default_rng(21)
    alive = np.ones(n_envs, dtype=bool)          # env still in its common prefix
    ends_agree = ends_oracle = ends_engine_only = 0
    reset_rows = reset_rows_bad = 0
    div_at_reset = 0
    worst_parked = worst_driving = 0.0
    parked_beams = parked_flips = parked_nb_rows = parked_ck_rows = 0
    div_bits = 0
    SI = _abi.SI
    for t in range(n_steps):
        act = util.driving_actions(rng, n_envs)
        if t % 7 == 0:
            act[::5, 0, 0] += 0.5  # some envs steer off the road: out-of-road ends next to crashes and arrivals
        o_obs, o_rew, o_done, o_flags = ora.step(act)
        g_obs, g_rew, g_done, g_flags = eng.step(torch.from_numpy(act).to(eng.device))
        eng.sync()
        g_obs = g_obs.cpu().numpy().astype(np.float64)[:, 0]
        g_done, g_flags = g_done.cpu().numpy()[:, 0], g_flags.cpu().numpy().astype(np.uint32)[:, 0]
        o_done, o_flags, o_obs = o_done[:, 0], o_flags[:, 0], o_obs[:, 0]
        same = (g_done == o_done) & (g_flags == o_flags)
        # episode ends seen in the common prefix
        ends_oracle += int((alive & (o_done != 0)).sum())
        ends_agree += int((alive & (o_done != 0) & same).sum())
        ends_engine_only += int((alive & (g_done != 0) & (o_done == 0)).sum())
        # rows where both restarted in agreement: the first observation of the new episode
        both_reset = alive & same & ((o_flags & _abi.F_RESET) != 0)
        if both_reset.any():
            d = np.abs(g_obs[both_reset] - o_obs[both_reset]).max(axis=1)
            reset_rows += int(both_reset.sum())
            reset_rows_bad += int((d > OBS_TOL).sum())
        newly = alive & ~same
        if newly.any():
            div_bits |= int(np.bitwise_or.reduce((g_flags ^ o_flags)[newly]))
        alive &= same
        # numeric drift inside the common prefix
        if alive.any():
            _, gi, _ = eng.get_state()
            driving = (gi[SI["STATUS"]][:, 1:] == _abi.ST_ACTIVE).any(axis=1)
            dall = np.abs(g_obs - o_obs)
            dd = dall.max(axis=1)
            if (alive & ~driving).any():
                # (a beam past a box corner flips hit <-> miss within the free-running drift: counted, like the grazing beams of the
                # teacher-forced tests -- one in ~1e8 beams, seen only in the larger PGD_FREE_RUN runs)
                pk = dall[alive & ~driving]
                flips = pk[:, 34:] > 0.01
                parked_beams += flips.size
                parked_flips += int(flips.sum())
                # (and a body whose nearest point sits on the 50 m broad-phase radius is a neighbour on one side only: its row of
                # neighbour floats differs wholesale -- the campaign's "neighbour boundary rows")
                nb_flip = pk[:, 18:34].max(axis=1) > 0.01
                parked_nb_rows += int(nb_flip.sum())
                # (and a check point passed one step apart -- the 5 m test on the lane coordinate, navigation.py:262-282 -- shows the
                # navigation floats of the next road for that one step)
                ck_flip = pk[:, 8:18].max(axis=1) > 0.01
                parked_ck_rows += int(ck_flip.sum())
                worst_parked = max(worst_parked, float(pk[:, :8].max()), float(pk[~ck_flip][:, 8:18].max()) if (~ck_flip).any() else 0.0,
                                   float(pk[~nb_flip][:, 18:34].max()) if (~nb_flip).any() else 0.0, float(np.where(flips, 0.0, pk[:, 34:]).max()))
            if (alive & driving).any():
                worst_driving = max(worst_driving, float(np.quantile(dd[alive & driving], 0.99)))
    print("free-running timed path: %d episode ends in the common prefixes, %d agree on step and flags (%.1f %%), %d ended on the "
          "engine only; %d of %d envs still in their common prefix after %d steps (divergence bits 0x%x); %d restarts compared, %d with "
          "a first observation off by more than %.1e; obs drift: parked traffic %.2e, driving traffic (99th percentile) %.2e"
          % (ends_oracle, ends_agree, 100.0 * ends_agree / max(1, ends_oracle), ends_engine_only, int(alive.sum()), n_envs, n_steps,
             div_bits, reset_rows, reset_rows_bad, OBS_TOL, worst_parked, worst_driving))
    assert ends_oracle >= 300, "the action stream must end at least 300 episodes inside the common prefixes"
    assert ends_agree >= 0.95 * ends_oracle and ends_engine_only <= 0.05 * ends_oracle
    assert reset_rows >= 250 and reset_rows_bad == 0, "a restart must reproduce the oracle's first observation"
    assert worst_parked < 4 * OBS_TOL  # the ego alone: free-running fp32 vs fp64 over an episode
    print("   parked-traffic rows: %d beams, %d flipped past a corner, %d rows with a neighbour on the 50 m radius, %d rows with a check "
          "point passed one step apart" % (parked_beams, parked_flips, parked_nb_rows, parked_ck_rows))
    n_rows = parked_beams / 240
    assert parked_flips <= 1e-6 * parked_beams + 1 and parked_nb_rows <= 1e-5 * n_rows + 1 and parked_ck_rows <= 1e-4 * n_rows + 1
    assert worst_driving < 5e-2
    assert alive.mean() > 0.5
    if size == "large" and not big:
        # the tie classes of the large run, counted (measured at 1024 x 1000: 12,426 of 12,426 episode ends on the same step with the
        # same flags, 1023 of 1024 envs never diverge, 0 of 137 M parked-scene beams flipped, 0 neighbour-radius rows, 1 row with a
        # check point passed a step apart; round 4's one-off 2048 x 1500: 37,719 of 37,720, 2046 of 2048, 0 of 409 M)
        assert ends_oracle >= 10000 and ends_agree >= ends_oracle - 3 and ends_engine_only <= 3
        assert int(alive.sum()) >= n_envs - 4
        assert parked_flips <= 2 and parked_nb_rows <= 2 and parked_ck_rows <= 5
        assert worst_driving < 5e-3


@pytest.mark.parametrize("size", ["suite", pytest.param("large", marks=LARGE_RUNS)])
def test_marl_free_running_through_finishes_and_respawns(size):
    """(size "large": 256 envs x 600 steps, the suite's version of round 4's one-off 512 x 900 run.)
    The reference-default multi-agent configuration (40 slots on the roundabout) as bench.py times it -- the fixed-config
    kernels, the four-wave observation on compacted lists with the zero-row marks (PgdDev::rowz), contacts by unordered pairs, the
    line test dealt out to the agents that need it, auto-reset -- held to the oracle WITHOUT set_state between the steps (teacher
    forcing goes through pgd_set_state, which drops the marks and the hints).  Per env the two runs are compared until the env's
    first discrete divergence (a contact or a line reached one step apart between fp32 and fp64: from there the agents of that env
    play different episodes); inside the common prefixes every agent's flags / done agree by construction, and
      * the finishes, respawns and env restarts seen there are most of all that the oracle sees;
      * every row handed out there -- also the first row of a respawned agent and the zero rows of empty slots -- is the oracle's:
        the state / navigation floats to a few observation tolerances of free-running drift, the beams except the few whose ray
        passes a box corner within that drift (counted, bounded)."""
    import torch
    from oracle import orc
    d, mb, sb = util.make_marl_banks(num_agents=40, capacity=40, kind="roundabout")
    n_envs, n_steps = (48, 400) if size == "suite" else (256, 600)
    if os.environ.get("PGD_FREE_RUN_MA") and size == "large":  # "envs,steps": another size for the large run
        n_envs, n_steps = (int(x) for x in os.environ["PGD_FREE_RUN_MA"].split(","))
    cfg = util.marl_config(n_envs, sb, horizon=150, resample_scenario=1, seed=7)
    eng = parity.engine(cfg, mb, sb)
    ora = orc.Oracle(cfg, mb, sb)
    ids = np.arange(n_envs) % 8
    o0 = ora.reset(ids)
    g0 = eng.reset(ids).cpu().numpy()
    assert np.abs(g0 - o0).max() < OBS_TOL
    rng = np.random.default_rng(9)
    A = sb.A
    alive = np.ones(n_envs, dtype=bool)
    n_fin = n_fin_alive = n_new = n_new_alive = n_reset = n_reset_alive = 0
    rows = beams = beams_off = n_div_reward = 0
    worst = 0.0
    div_bits = 0
    first_div = []
    for t in range(n_steps):
        act = util.marl_actions(rng, n_envs, A)
        o_obs, o_rew, o_done, o_flags = ora.step(act)
        g_obs, g_rew, g_done, g_flags = eng.step(torch.from_numpy(act).to(eng.device))
        eng.sync()
        g_obs = g_obs.cpu().numpy().astype(np.float64)
        g_done, g_flags, g_rew = g_done.cpu().numpy(), g_flags.cpu().numpy().astype(np.uint32), g_rew.cpu().numpy().astype(np.float64)
        same = ((g_done == o_done) & (g_flags == o_flags)).all(axis=1)
        # (a lane picked one step apart at a junction, or the engine-force cut-off at max_speed crossed a sub-step apart, shows in the
        # reward before it shows in a flag: the env leaves its common prefix there as well)
        rew_ok = (np.abs(g_rew - o_rew) < 50 * REW_TOL).all(axis=1)
        n_div_reward += int((alive & same & ~rew_ok).sum())
        same &= rew_ok
        fin = (o_done != 0) & ((o_flags & _abi.F_REPORT) != 0)
        new = (o_flags & _abi.F_NEW) != 0
        rst = (o_flags[:, 0] & _abi.F_RESET) != 0
        n_fin += int(fin.sum()); n_fin_alive += int(fin[alive & same].sum())
        n_new += int(new.sum()); n_new_alive += int(new[alive & same].sum())
        n_reset += int(rst.sum()); n_reset_alive += int(rst[alive & same].sum())
        newly = alive & ~same
        if newly.any():
            div_bits |= int(np.bitwise_or.reduce((g_flags ^ o_flags)[newly].ravel()))
            first_div += [t] * int(newly.sum())
        alive &= same
        if alive.any():
            dd = np.abs(g_obs - o_obs)[alive]                    # every row of the env, due or zero
            n_state = dd.shape[2] - cfg.num_lasers
            rows += dd.shape[0] * dd.shape[1]
            worst = max(worst, float(dd[:, :, :n_state].max()))  # state + navigation floats: no ray in them
            beams += dd.shape[0] * dd.shape[1] * cfg.num_lasers
            beams_off += int((dd[:, :, n_state:] > 4 * OBS_TOL).sum())
    print("multi-agent free run, 40 slots: %d of %d envs in their common prefix after %d steps (first divergences at steps %s, bits "
          "0x%x, %d of them by a reward alone); in the prefixes %d of %d finishes, %d of %d respawns, %d of %d env restarts; %d rows compared: state / navigation "
          "floats off by at most %.2e, %d of %d beams off by more than %.0e (%.2e of them: rays past a box corner, free-running "
          "fp32 against fp64)"
          % (int(alive.sum()), n_envs, n_steps, sorted(first_div)[:8], div_bits, n_div_reward, n_fin_alive, n_fin, n_new_alive, n_new, n_reset_alive,
             n_reset, rows, worst, beams_off, beams, 4 * OBS_TOL, beams_off / max(1, beams)))
    assert n_fin_alive >= 300 and n_new_alive >= 300 and n_reset_alive >= 20
    assert alive.mean() >= 0.5
    assert worst < 10 * OBS_TOL and beams_off <= 3e-4 * beams
    if size == "large" and not os.environ.get("PGD_FREE_RUN_MA"):
        # measured at 256 x 600 (one respawn per step, round 5): 248 of 256 envs never diverge (a contact or a line reached a step
        # apart), in their prefixes 49,300 of 50,293 finishes, 42,485 of 43,380 respawns and 573 of 584 env restarts agree, state /
        # navigation floats within 1.1e-5, 3.9e-6 of 433 M beams pass a box corner within the drift
        assert alive.mean() >= 0.93
        assert n_fin_alive >= 30000 and n_fin_alive >= 0.95 * n_fin and n_new_alive >= 0.95 * n_new and n_reset_alive >= 0.9 * n_reset
        assert worst < 4 * OBS_TOL and beams_off <= 2e-5 * beams


@pytest.mark.parametrize("traffic_mode", ["trigger", "respawn"])
def test_idm_agent_parity_and_arrivals(descs, traffic_mode):
    """IDM_agent = True (base_env.py:30, agent_manager.py:79): the ego's policy is IDMPolicy -- routing along its checkpoints,
    front / back search, lane change, PID steering, IDM law (idm_policy.py:190-353), the very routine the traffic runs -- and the
    actions handed to step() are ignored.  (1) teacher-forced against the oracle: flags / done / integer state bit-exact, every
    float field of the state within its tolerance (the ego's PID sums and routing lane now live in its record);  (2) the
    policy does its job: free-running without traffic in the way the IDM ego follows its route to the destination -- most
    episodes end with arrive_dest, none by leaving the road -- and the garbage actions it is handed change nothing."""
    n_envs = 64
    eng, ora, cfg = parity.engines(descs, n_envs, seed=4, idm_agent=True, traffic_mode=traffic_mode, resample_scenario=1)
    assert cfg.idm_agent == 1
    ids = np.arange(n_envs) % 8
    o0 = ora.reset(ids)
    g0 = eng.reset(ids).cpu().numpy()
    assert np.abs(g0 - o0).max() < OBS_TOL
    rng = np.random.default_rng(2)
    stats = parity.new_stats()
    worst, ties, traffic_steps, n_done, arrive = {}, 0, 0, 0, 0
    SI = _abi.SI
    int_ties = 0
    # (the actions are ignored by both sides)
    for s in parity.teacher_forced(eng, ora, stats, 260, lambda t: rng.uniform(-1, 1, size=(n_envs, 1, 2)).astype(np.float32)):
        agree = s.agree
        int_ties += s.int_ties()[0]
        tie = s.idm_tie(agree)  # (the ego is an IDM vehicle here: its leader can sit on the 30 m search range as well)
        ties += int((tie & agree).sum())
        traffic_steps += int((s.i[SI["STATUS"]] == _abi.ST_ACTIVE).sum())
        s.compare_state(agree & ~tie, worst)
        n_done += int(s.o_done.sum())
    print("IDM agent, teacher-forced:", stats, "integer-state ties", int_ties, "idm ties", ties, "of", traffic_steps,
          "episodes ended", n_done, {k: round(v, 3) for k, v in worst.items()})
    parity.report("IDM agent parity", stats)
    # integer state that differs is a margin-verified tie (LANE / CONTACT / ROUTE / LEADER), at most the two seen before; anything else: 0
    assert stats["int_mismatch"] == 0 and n_done > 0
    assert int_ties <= 2
    assert stats["flag_mismatch"] == 0 and stats.get("flag_ties", 0) == 0 and stats["obs"] < OBS_TOL and stats["rew"] < REW_TOL, stats
    assert not util.state_failures(worst), util.state_failures(worst)
    assert ties <= 0.002 * traffic_steps + 2
    # (2) free-running without traffic: the actions are ignored (two engines fed different garbage stay bit-identical) and the
    # policy drives the route: episodes last, and the driving reward (= longitudinal progress along the route) adds up.
    # How they END is the dynamics' business: under the kinematic bicycle the reference's steering PID (kp 1.7, kd 3.5 per 0.1 s
    # decision, tuned on Bullet's raycast vehicle) weaves by a few decimetres, and an ego that starts on the lane next to the
    # centre line ends most episodes by touching the yellow line (out_of_road) after 100 - 200 m -- the oracle does the same,
    # flag for flag; what Bullet would do is the unpinned part of DESIGN.md section 3.
    import torch
    eng, _, cfg = parity.engines(descs, 128, seed=5, idm_agent=True, num_traffic=0, num_lasers=0, resample_scenario=1)
    twin, _, _ = parity.engines(descs, 128, seed=5, idm_agent=True, num_traffic=0, num_lasers=0, resample_scenario=1)
    eng.reset(np.arange(128) % 8); twin.reset(np.arange(128) % 8)
    done_n = arrive_n = 0
    ep_rewards = []
    junk = torch.from_numpy(np.full((128, 1, 2), -1.0, dtype=np.float32)).to(eng.device)  # "full brake, hard left"
    for t in range(900):
        other = torch.from_numpy(rng.uniform(-1, 1, size=(128, 1, 2)).astype(np.float32)).to(eng.device)
        o1, r1, dn, fl = [x.clone() for x in eng.step(junk)]
        o2, r2, dn2, fl2 = twin.step(other)
        eng.sync(); twin.sync()
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(dn, dn2) and torch.equal(fl, fl2)
        if t % 50 == 49:
            f_, i_, ei_ = eng.get_state()
            ep_rewards.append(float(f_[_abi.SF["EP_REWARD"]][:, 0].mean()))
        fl = fl.cpu().numpy().astype(np.uint32)[:, 0]
        dn = dn.cpu().numpy()[:, 0] != 0
        done_n += int(dn.sum())
        arrive_n += int((dn & ((fl & _abi.F_ARRIVE) != 0)).sum())
    mean_len = 900.0 * 128 / max(1, done_n)
    print("IDM ego, free-running, no traffic: %d episodes ended (%d by arrival), mean length %.0f steps, mean running episode "
          "reward %.1f" % (done_n, arrive_n, mean_len, float(np.mean(ep_rewards))))
    assert mean_len > 100 and float(np.mean(ep_rewards)) > 40.0


def test_state_with_spawn_records_of_other_slots(descs):
    """pgd_set_state may hand a slot the spawn record of another one (SI_SPAWN is a state field).  The single-agent kernels read the
    head of a slot's OWN spawn record together with its vehicle record (the address follows from the scenario id) and fall back to
    the record's spawn index when the two differ: two traffic vehicles with exchanged records (other dimensions and drive
    parameters) must step like the oracle's."""
    import torch
    from oracle import orc
    mb, sb = util.make_banks(descs, n_maps=8, traffic_mode="respawn")  # every traffic vehicle drives from the first step
    n = 64
    cfg = _abi.make_config(n, num_agents=1, num_traffic=16, num_lasers=240, auto_reset=0, seed=5)
    eng = parity.engine(cfg, mb, sb)
    ora = orc.Oracle(cfg, mb, sb)
    ids = np.arange(n) % 8
    ora.reset(ids)
    eng.reset(ids)
    f, i, ei = ora.get_state()
    sp = i[_abi.SI["SPAWN"]]
    st = i[_abi.SI["STATUS"]]
    swapped = 0
    for e in range(n):  # exchange the spawn records of the first two driving traffic vehicles of different size
        act = [s for s in range(1, 17) if st[e, s] == _abi.ST_ACTIVE]
        for a in act:
            for b in act:
                la = sb.spawns["length"].reshape(len(sb.scenarios), -1)[ids[e], sp[e, a]]
                lb = sb.spawns["length"].reshape(len(sb.scenarios), -1)[ids[e], sp[e, b]]
                if a < b and la != lb:
                    sp[e, a], sp[e, b] = sp[e, b], sp[e, a]
                    swapped += 1
                    break
            else:
                continue
            break
    assert swapped > n // 2
    ora.set_state(f, i, ei)
    eng.set_state(f, i, ei)
    rng = np.random.default_rng(3)
    worst = 0.0
    for t in range(40):
        act = util.driving_actions(rng, n)
        oo, orw, od, ofl = ora.step(act, threads=16)
        go, grw, gd, gfl = eng.step(torch.from_numpy(act).cuda())
        eng.sync()
        assert np.array_equal(gfl.cpu().numpy(), ofl)
        d_obs = np.abs(go.cpu().numpy().astype(np.float64) - oo)
        beams = d_obs[..., -240:]
        beams[beams > OBS_TOL] = 0.0  # (grazing beams are counted by the parity tests proper)
        worst = max(worst, float(d_obs.max()))
        gf, gi, gei = eng.get_state()
        assert np.array_equal(gi[_abi.SI["SPAWN"]], ora.get_state()[1][_abi.SI["SPAWN"]])
        ora.set_state(*eng.get_state())  # teacher forcing
    assert worst < OBS_TOL, worst
