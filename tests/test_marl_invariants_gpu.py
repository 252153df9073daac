"""The reference's own multi-agent invariants, re-stated on the dict-keyed envs of the HIP engine -- one parametrised test per
invariant over the five env classes.  Sources: pgdrive/tests/test_env/test_ma_roundabout_env.py (and its four
siblings test_ma_intersection.py, test_ma_bottleneck_env.py, test_ma_tollgate.py, test_ma_parking_lot.py, which repeat the same
functions with the per-env relaxations quoted below), test_ma_env_force_reset.py:5, tests/test_functionality/test_reborn.py:5,
test_object_collision_detection.py:136.

Where the reference reaches into a vehicle (`env.vehicles[k].set_position / set_static`, `navigation.final_lane.end`,
`agent_manager.finish`) the tests use the same names on `pgdrive_amd.marl_env.VehicleHandle` / `MultiAgent*Env.finish`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ["roundabout", "intersection", "bottleneck", "tollgate", "parking"]


def _cls(kind):
    from pgdrive_amd import marl_env
    return dict(roundabout=marl_env.MultiAgentRoundaboutEnv, intersection=marl_env.MultiAgentIntersectionEnv,
                bottleneck=marl_env.MultiAgentBottleneckEnv, tollgate=marl_env.MultiAgentTollgateEnv,
                parking=marl_env.MultiAgentParkingLotEnv)[kind]


def _act(env, action):
    """test_ma_roundabout_env.py:58-70: one step with the key-set invariants of the dict protocol."""
    obs, reward, done, info = env.step(action)
    assert isinstance(obs, dict) and isinstance(reward, dict) and isinstance(done, dict) and isinstance(info, dict)
    assert set(obs) == set(reward) == set(info) == set(done) - {"__all__"}
    for k, o in obs.items():
        assert env.vec.single_observation_space.contains(o), k
    if not done["__all__"]:
        assert len(env.vehicles) > 0
    # the vehicles of the next step are exactly the reported agents that are not done
    assert set(env.vehicles) == {k for k in obs if not done[k]} or done["__all__"]
    return obs, reward, done, info


@pytest.mark.parametrize("kind", KINDS)
def test_ma_horizon_and_out_of_road_cost(kind):
    """test_ma_roundabout_horizon (test_ma_roundabout_env.py:97-151): horizon 100, four agents flooring it with full steering; never
    more than num_agents vehicles, newcomers arrive with a row of their own, reward -777 <=> out of road => done with cost 778."""
    env = _cls(kind)(dict(horizon=100, num_agents=4, vehicle_config=dict(lidar=dict(num_others=2)), out_of_road_penalty=777,
                          out_of_road_cost=778, crash_done=False, seed=3))
    try:
        obs = env.reset()
        assert len(obs) == 4
        last_keys = set(env.vehicles)
        n_oor = 0
        for step in range(1, 1000):
            o, r, d, i = _act(env, {k: [1, 1] for k in env.vehicles})
            new_keys = set(env.vehicles)
            if any(d.values()):
                assert len(last_keys) <= 4 and len(new_keys) <= 4
                for k in new_keys - last_keys:
                    assert k in o and k in d
            for k, rr in r.items():
                if rr == -777:
                    assert d[k] and i[k]["cost"] == 778 and i[k]["out_of_road"]
                    n_oor += 1
            for k, ii in i.items():
                if ii and (ii["out_of_road"] or ii["cost"] == 778):
                    assert d[k] and ii["cost"] == 778 and ii["out_of_road"]
            if d["__all__"]:
                break
            last_keys = new_keys
        assert d["__all__"] and n_oor > 0
        # (with every agent static in its delay_done window nobody can be respawned and the episode ends early, as upstream:
        # len(self.vehicles) == 0, multi_agent_pgdrive.py:139-142; by 5 x horizon at the latest)
        assert step <= 5 * 100
    finally:
        env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_ma_reward_done_alignment_out_of_road(kind):
    """test_ma_roundabout_reward_done_alignment (:271-298; tollgate variant test_ma_tollgate.py:278-305 excludes horizon ends):
    with crash_done off, an agent that is done without reaching its horizon (or its destination, or a toll booth) is out of road, and
    the out-of-road reward never comes without done."""
    env = _cls(kind)(dict(horizon=200, num_agents=4, out_of_road_penalty=777, crash_done=False, seed=1))
    try:
        env.reset()
        n_done = 0
        for action in (-1, 1):
            for step in range(1200):
                o, r, d, i = _act(env, {k: [action, 1] for k in env.vehicles})
                for k, dd in d.items():
                    if dd and k != "__all__" and not d["__all__"] and not i[k]["max_step"] and not i[k]["arrive_dest"] and \
                            not i[k]["crash_building"]:
                        assert i[k]["out_of_road"] and r[k] == -777, (k, r[k], i[k])
                        n_done += 1
                for k, rr in r.items():
                    if rr == -777:
                        assert d[k] and i[k]["out_of_road"]
                if d["__all__"]:
                    env.reset()
                    break
        assert n_done >= 4
    finally:
        env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_ma_reward_done_alignment_two_agents_on_top_of_each_other(kind):
    """test_ma_roundabout_reward_done_alignment_1, first part (:300-349): agent0 is put on agent1's position; with crash_done and
    delay_done 0 BOTH are done at once, both with crash_vehicle / crash in their info."""
    env = _cls(kind)(dict(horizon=100, num_agents=2, crash_vehicle_penalty=1.7777, crash_done=True, delay_done=0, seed=1))
    try:
        env.reset()
        for step in range(5):
            o, r, d, i = _act(env, {k: [0, 0] for k in env.vehicles})
            assert not any(d.values())
        v = env.vehicles
        v["agent0"].set_position(v["agent1"].position, height=1.2)
        for step in range(50):
            o, r, d, i = _act(env, {k: [0, 0] for k in env.vehicles})
            if not any(d.values()):
                continue
            assert d["agent0"] and d["agent1"] and not d["__all__"]
            assert sum(bool(x) for x in d.values()) == 2
            for k in ("agent0", "agent1"):
                assert i[k]["crash_vehicle"] and i[k]["crash"]
                if r[k] == pytest.approx(-1.7777):
                    assert d[k]
            # (the one that stands where it was spawned is still on its lane: it gets the crash penalty itself)
            assert r["agent1"] == pytest.approx(-1.7777, abs=1e-6)
            break
        else:
            raise AssertionError("two overlapping agents never reported a contact")
    finally:
        env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_ma_reward_done_alignment_driving_into_standing_agents(kind):
    """Second part (:351-405; tollgate variant test_ma_tollgate.py:371-456): everybody but agent0 is static, agent0 floors it with
    crash_done off: crash <=> crash_vehicle; an agent that is done is out of road (or arrived / hit a booth / reached its horizon);
    the crash penalty never comes without the crash flag."""
    cfg = dict(horizon=200, crash_vehicle_penalty=1.7777, crash_done=False, seed=0)
    if kind in ("roundabout", "intersection"):
        cfg.update(num_agents=40, map_config=dict(exit_length=110, lane_num=1))  # the reference's own map for this test
    elif kind == "tollgate":
        cfg.update(num_agents=24)
    env = _cls(kind)(cfg)
    try:
        env.reset()
        _act(env, {k: [0, 0] for k in env.vehicles})
        for k, v in env.vehicles.items():
            if k != "agent0":
                v.set_static(True)
        n_crash = 0
        for step in range(400):
            for k, v in env.vehicles.items():  # (newcomers: static as well)
                if k != "agent0" and v.slot not in env._static:
                    v.set_static(True)
            o, r, d, i = _act(env, {k: [0, 1] for k in env.vehicles})
            for k, ii in i.items():
                if ii:
                    assert bool(ii["crash"]) == bool(ii["crash_vehicle"])
                    n_crash += int(ii["crash_vehicle"])
            for k, dd in d.items():
                if dd and k != "__all__" and not d["__all__"]:
                    assert i[k]["out_of_road"] or i[k]["arrive_dest"] or i[k]["crash_building"] or i[k]["max_step"], (k, i[k])
            for k, rr in r.items():
                if rr == pytest.approx(-1.7777, abs=1e-6):
                    assert i[k]["crash_vehicle"] and i[k]["crash"]
            if d.get("agent0") or d["__all__"]:
                break
        assert d.get("agent0") or d["__all__"]
        if kind in ("roundabout", "intersection"):
            assert n_crash > 0  # one lane, a standing car every few metres ahead: agent0 drives into the first of them
    finally:
        env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_ma_reward_done_alignment_success(kind):
    """Third part (:407-448): agent0 is put on the end of its final lane: done with arrive_dest and the success reward in the very
    next step; agent1 is neither."""
    env = _cls(kind)(dict(horizon=100, num_agents=2, success_reward=999, out_of_road_penalty=555, crash_done=True, seed=0))
    try:
        env.reset()
        v0 = env.vehicles["agent0"]
        end = v0.final_lane["end"]
        v0.set_position(end)
        np.testing.assert_almost_equal(v0.position, end, decimal=3)
        o, r, d, i = _act(env, {k: [0, 0] for k in env.vehicles})
        assert i["agent0"]["arrive_dest"] and d["agent0"] and r["agent0"] == 999
        assert not i["agent1"]["arrive_dest"] and not d["agent1"] and r["agent1"] != 999
    finally:
        env.close()


@pytest.mark.parametrize("kind", ["roundabout", "intersection", "bottleneck", "tollgate"])  # (upstream has none for the parking lot)
def test_ma_reward_sign(kind):
    """test_ma_roundabout_reward_sign (:451-487): one agent that simply drives straight ahead collects more than 10 reward before its
    episode ends, from every spawn place it is given."""
    env = _cls(kind)(dict(num_agents=1, seed=0))
    try:
        env.reset()
        n_places = env.vec.scen_bank.P
        ep_reward, respawns = 0.0, 0
        for step in range(1000):
            o, r, d, i = env.step({k: [0, 1] for k in env.vehicles})
            acted = [k for k in r if i[k]]  # (a newcomer's row has reward 0 and an empty info)
            ep_reward += r[acted[0]]
            if any(d[k] for k in acted):
                respawns += 1
                assert ep_reward > 10, ep_reward
                ep_reward = 0.0
            if respawns >= n_places or d["__all__"]:
                break
        assert respawns >= 1
    finally:
        env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_ma_no_short_episode(kind):
    """test_ma_roundabout_no_short_episode (:522-559): random driving; the agents asked to act are exactly those reported alive the
    step before; nobody finishes with an episode shorter than one step."""
    env = _cls(kind)(dict(horizon=300, seed=5))
    rng = np.random.RandomState(0)
    actions = [[0, 1], [1, 1], [-1, 1]]
    try:
        o = env.reset()
        d = {"__all__": False}
        d_count = 0
        for step in range(600):
            act = {k: actions[rng.choice(3)] for k in env.vehicles}
            alive_reported = {k for k in o if not d.get(k, False)}
            assert set(act) == alive_reported
            o, r, d, i = _act(env, act)
            for k, ii in i.items():
                if d[k] and ii:
                    assert ii["episode_length"] >= 1
                    d_count += 1
            if d["__all__"]:
                o = env.reset()
                d = {"__all__": False}
            if d_count > 200:
                break
        assert d_count > 20
    finally:
        env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_ma_horizon_termination(kind):
    """test_ma_roundabout_horizon_termination (:562-610): horizon 100, crash_done off, everybody static except two agents that floor
    it: a static agent ends exactly by max_step (no out_of_road / crash in its info), and an agent that finished is absent from
    obs / reward / done / info of the next step."""
    env = _cls(kind)(dict(horizon=100, num_agents=8, crash_done=False, seed=2))
    special = {"agent0", "agent7"}
    try:
        for rep in range(2):
            env.reset()
            should_be_gone = set()
            n_max_step = 0
            for step in range(1, 1000):
                act = {}
                for k, v in env.vehicles.items():
                    if k in special:
                        act[k] = [1, 1]
                    else:
                        act[k] = [0, 0]
                        if v.slot not in env._static:
                            v.set_static(True)
                obs, r, d, i = _act(env, act)
                if step == 1:
                    assert not any(d.values())
                for k in should_be_gone:
                    assert k not in obs and k not in r and k not in d and k not in i, "a max_step agent was stepped again"
                should_be_gone.clear()
                for k, dd in d.items():
                    if k == "__all__" or not dd or d["__all__"]:
                        continue
                    if k not in special:
                        assert i[k]["max_step"] and not i[k]["out_of_road"] and not i[k]["crash"] and not i[k]["crash_vehicle"], (k, i[k])
                        assert i[k]["episode_length"] == 100
                        n_max_step += 1
                    should_be_gone.add(k)
                if d["__all__"]:
                    break
            assert d["__all__"] and n_max_step >= 1
    finally:
        env.close()


def _no_overlap(env, min_dist=None):
    vs = list(env.vehicles.values())
    pos = np.array([v.position for v in vs])
    wid = np.array([v.width for v in vs])
    for a in range(len(vs)):
        for b in range(a + 1, len(vs)):
            dist = float(np.hypot(*(pos[a] - pos[b])))
            assert dist > (min_dist if min_dist is not None else wid[a] / 2 + wid[b] / 2), "vehicles overlap: %s %s %.3f" % (
                vs[a].name, vs[b].name, dist)
        assert not vs[a].crash_vehicle, "%s carries a contact flag" % vs[a].name


@pytest.mark.parametrize("kind", KINDS)
def test_ma_reset_after_respawn_and_no_overlapping_spawns(kind):
    """test_ma_roundabout_40_agent_reset_after_respawn (:612-645) + test_ma_no_reset_error (:648-670) + close_spawn (:243-268): after
    a reset no two vehicles overlap or carry a contact flag -- also right after half of them were finished by force and respawned --
    and respawns while driving never drop an agent onto another one."""
    n = dict(parking=10).get(kind, 40)
    env = _cls(kind)(dict(horizon=50, num_agents=n, seed=7))
    try:
        env.reset()
        for rep in range(12):
            o = env.reset()
            assert len(o) == len(env.vehicles) and len(o) >= min(n, 8)
            _no_overlap(env, min_dist=2.2)  # (distance_greater(..., length=2.2) of close_spawn)
            for k in list(env.vehicles)[:len(o) // 2]:
                env.finish(k)
            for _ in range(3):
                env.step({k: [1, 1] for k in env.vehicles})
    finally:
        env.close()
    env = _cls(kind)(dict(horizon=300, num_agents=n, delay_done=0, seed=8))
    try:
        env.reset()
        for step in range(300):
            newcomers_ok = True
            o, r, d, i = env.step({k: [0, 1] for k in env.vehicles})
            new = [k for k in o if not i[k]]
            if new:  # a newcomer stands clear of everybody (8 m x 3 m respawn region, spawn_manager.py:27-28,157-215)
                vs = env.vehicles
                for k in new:
                    for k2, v2 in vs.items():
                        if k2 != k and k in vs:
                            dist = float(np.hypot(*(vs[k].position - v2.position)))
                            newcomers_ok &= dist > vs[k].width / 2 + v2.width / 2
            assert newcomers_ok
            if d["__all__"]:
                break
    finally:
        env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_ma_randomize_spawn_place(kind):
    """test_randomize_spawn_place (:672-688): a reset puts every agent somewhere else than where it just stood."""
    env = _cls(kind)(dict(num_agents=4, seed=11))
    try:
        env.reset()
        seen = set()
        for step in range(30):
            last = {k: v.position for k, v in env.vehicles.items()}
            env.step({k: [1, 1] for k in env.vehicles})
            env.reset()
            now = {k: v.position for k, v in env.vehicles.items()}
            for k, p in now.items():
                assert k not in last or not np.all(p == last[k])
            seen.add(tuple(np.round(np.concatenate([now[k] for k in sorted(now)]), 3)))
        assert len(seen) > 1  # and the placements themselves change from reset to reset (SpawnManager.reset draws afresh)
    finally:
        env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_ma_env_force_reset_with_another_agent_count(kind):
    """test_ma_env_force_reset.py:5-27: close, re-init with another num_agents, reset: as many vehicles as asked for."""
    cls = _cls(kind)
    e = cls({"num_agents": 1})
    try:
        e.reset()
        assert len(e.vehicles) == e.num_agents == 1
        for n in (2, 5):
            e.close()
            e.__init__({"num_agents": n})
            o = e.reset()
            assert len(e.vehicles) == e.num_agents == len(o) == n
            assert sorted(o) == ["agent%d" % k for k in range(n)]
    finally:
        e.close()


def test_traffic_respawn_mode_releases_what_it_removes():
    """tests/test_functionality/test_reborn.py:5-33 (PGDriveEnv, traffic_mode "respawn", ego standing still for 3000 steps): the
    traffic manager holds exactly its traffic vehicles + the ego -- a vehicle that left its lane is released, not kept.  Here: every
    traffic slot is ACTIVE or REMOVED from the first step on (respawn mode parks nothing), a REMOVED slot never comes back within
    the episode (upstream's re-placement is commented out, traffic_manager.py:98-108), and a removed vehicle leaves no trace in the
    ego's neighbour rows / lidar: the observation equals the one of a world without it."""
    import torch
    from pgdrive_amd import _abi
    from pgdrive_amd.env import PGDriveEnv
    env = PGDriveEnv({"environment_num": 1, "start_seed": 1003, "traffic_mode": "respawn", "traffic_density": 0.2})
    try:
        env.reset()
        eng = env.vec.engine
        removed_before = None
        n_removed_seen = 0
        for t in range(1, 3000):
            o, r, d, info = env.step([0, 0])
            assert not d
            if t % 25 and t > 3:
                continue
            f, i, ei = eng.get_state()
            st = i[_abi.SI["STATUS"], 0, 1:]
            assert set(np.unique(st)) <= {_abi.ST_EMPTY, _abi.ST_ACTIVE, _abi.ST_REMOVED}
            removed = st == _abi.ST_REMOVED
            if removed_before is not None:
                assert (removed | ~removed_before).all(), "a removed traffic vehicle came back"
            removed_before = removed
            n_removed_seen = max(n_removed_seen, int(removed.sum()))
        assert (st == _abi.ST_ACTIVE).sum() + removed.sum() == (st != _abi.ST_EMPTY).sum()
        # released: wiping the removed slots' records changes nothing the ego sees
        f, i, ei = eng.get_state()
        o_with = eng.observe().cpu().numpy().copy()
        f2 = f.copy()
        f2[_abi.SF["X"], 0, 1:][removed] = f[_abi.SF["X"], 0, 0] + 3.0  # right next to the ego, if they still counted
        f2[_abi.SF["Y"], 0, 1:][removed] = f[_abi.SF["Y"], 0, 0]
        eng.set_state(f2, i, ei)
        o_without = eng.observe().cpu().numpy()
        assert np.array_equal(o_with, o_without)
        torch.cuda.synchronize()
    finally:
        env.close()


def test_object_collision_detection():
    """tests/test_functionality/test_object_collision_detection.py:136-170: driving straight at a traffic object, the lidar sees it
    before the contact and the contact is reported as crash_object."""
    from pgdrive_amd.env import SafePGDriveEnv
    from tests.parity import teleport_to_objects
    env = SafePGDriveEnv({"environment_num": 16, "start_seed": 1000, "accident_prob": 1.0, "traffic_density": 0.0})
    try:
        done_cases = 0
        for seed in range(1000, 1016):
            env.reset(force_seed=seed)
            f, i, ei = env.vec.engine.get_state()
            if not teleport_to_objects(env.vec.map_bank, env.vec.scen_bank, np.array([seed - 1000]), f, i):
                continue
            env.vec.engine.set_state(f, i, ei)
            detect_obj = crash_obj = False
            for t in range(60):
                o, r, d, info = env.step([0, 1])
                cloud = o[-240:]
                ahead = np.r_[cloud[:6], cloud[-6:]]  # the beams around straight ahead (beam 0 = heading)
                if not crash_obj and ahead.min() < 0.5:
                    detect_obj = True  # something within 25 m straight ahead, and the world holds nothing but objects
                if info["crash_object"]:
                    crash_obj = True
                    break
                if d:
                    break
            if crash_obj:
                assert detect_obj, "crashed into an object the lidar never saw"
                done_cases += 1
        assert done_cases >= 3
    finally:
        env.close()
