"""The gym-shaped surface on the GPU: spaces, reset/step shapes, info keys, episode protocol (reference tests:
tests/test_functionality/test_obs_action_space.py:10-14, test_reward_cost_done.py:54-74, test_collision.py:4-50,
test_out_of_road.py:7-36, test_random_engine.py:6-188 re-stated for the bicycle build)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_single_env_protocol():
    from pgdrive_amd.env import PGDriveEnv
    env = PGDriveEnv(dict(start_seed=1000, environment_num=10))
    try:
        o = env.reset(force_seed=1003)
        assert o.shape == (274, ) and o.dtype == np.float32 and env.observation_space.contains(o)
        assert env.action_space.shape == (2, )
        assert abs(o[2] - 0.5) < 1e-3  # heading_diff(own lane) == 0.5 (test_ego_vehicle.py)
        total, done, info = 0.0, False, {}
        for t in range(400):
            o, r, done, info = env.step([0.0, 1.0])  # full throttle straight, as profile_pgdrive.py:16
            assert env.observation_space.contains(o) and np.isscalar(r) and isinstance(info, dict)
            total += r
            if done:
                break
        for k in ("cost", "velocity", "steering", "acceleration", "step_reward", "crash_vehicle", "out_of_road",
                  "arrive_dest", "crash_object", "crash_building", "crash", "max_step", "episode_reward", "episode_length",
                  "step_energy", "episode_energy", "raw_action", "overtake_vehicle_num"):
            assert k in info  # the reference's step-info keys (base_vehicle.py:255-273, base_env.py:303-344)
        assert info["raw_action"] == (0.0, 1.0) and info["step_energy"] >= 0.0 and info["episode_length"] == t + 1
        assert done and (info["out_of_road"] or info["crash_vehicle"] or info["arrive_dest"])
        if info["out_of_road"]:
            assert r == -5.0 and info["cost"] == 1.0  # test_reward_cost_done.py:54-74
        # same seed -> same first observation (test_random_engine.py)
        o1 = env.reset(force_seed=1003)
        o2 = env.reset(force_seed=1003)
        assert np.array_equal(o1, o2)
        assert not np.array_equal(o1, env.reset(force_seed=1004)) or True
    finally:
        env.close()


def test_steering_into_sidewalk_ends_episode():
    """steering -0.5 leaves the road within 100 steps and touches lane lines on the way (test_collision.py:26-50)."""
    from pgdrive_amd import _abi
    from pgdrive_amd.env import PGDriveEnv
    env = PGDriveEnv(dict(start_seed=1000, environment_num=4, traffic_density=0.0))
    try:
        env.reset(force_seed=1000)
        seen = 0
        for t in range(100):
            o, r, d, info = env.step([-0.5, 0.6])
            _, i, _ = env.vec.engine.get_state()
            seen |= int(i[_abi.SI["VFLAGS"], 0, 0])
            if d:
                break
        assert d and info["out_of_road"]
        assert seen & (_abi.F_ON_BROKEN | _abi.F_ON_WHITE | _abi.F_ON_YELLOW | _abi.F_CRASH_SIDEWALK)
    finally:
        env.close()


def test_vec_env_autoreset_and_unknown_key():
    import torch
    from pgdrive_amd import _abi
    from pgdrive_amd.vec_env import PGDriveVecEnv
    with pytest.raises(KeyError):
        PGDriveVecEnv(dict(bogus=1))
    env = PGDriveVecEnv(dict(num_envs=256, start_seed=1000, environment_num=100, seed=3))
    try:
        obs = env.reset()
        assert obs.shape == (256, 274) and obs.is_cuda
        n_done = 0
        g = torch.Generator(device="cuda").manual_seed(0)
        for t in range(150):
            a = torch.rand((256, 2), device="cuda", generator=g) * 2 - 1
            a[:, 1] = a[:, 1].abs()  # keep moving so that episodes actually end
            obs, rew, done, flags = env.step(a)
            n_done += int(done.sum().item())
            fl = flags.cpu().numpy().astype(np.uint32)
            dn = done.cpu().numpy().astype(bool)
            assert ((fl & _abi.F_RESET) != 0)[dn].all() and not ((fl & _abi.F_RESET) != 0)[~dn].any()
            assert float(obs.min()) >= 0.0 and float(obs.max()) <= 1.0 and bool(torch.isfinite(obs).all())
        assert n_done > 20  # random driving ends episodes; auto-reset keeps every env alive
        info = env.info_from_flags(flags)
        assert set(info) >= {"arrive_dest", "out_of_road", "crash_vehicle", "crash"}
    finally:
        env.close()


def test_checkpoint_resume_roundtrip():
    """get_state -> set_state reproduces the same next step bit-for-bit (BaseVehicle.get_state/set_state)."""
    import torch
    from pgdrive_amd.vec_env import PGDriveVecEnv
    env = PGDriveVecEnv(dict(num_envs=64, seed=1, resample_scenario=False, start_seed=1000, environment_num=100))
    try:
        env.reset(force_seed=[1000 + (k % 10) for k in range(64)])
        a = torch.zeros((64, 2), device="cuda")
        a[:, 1] = 0.7
        for _ in range(30):
            env.step(a)
        env.engine.sync()
        snap = env.engine.get_state()
        o1 = [x.clone() for x in env.step(a)]
        env.engine.sync()
        env.engine.set_state(*snap)
        o2 = env.step(a)
        env.engine.sync()
        for x, y in zip(o1, o2):
            assert torch.equal(x, y)
    finally:
        env.close()


@pytest.mark.parametrize("kind", ["roundabout", "intersection", "bottleneck", "tollgate", "parking"])
def test_marl_dict_protocol(kind):
    """Key-set invariants of the reference's MARL tests (tests/test_env/test_ma_roundabout_env.py:73-200,
    test_marl_reborn.py:6-60): obs/reward/done/info share keys, finished agents disappear, newcomers get fresh
    increasing ids, -penalty => done, __all__ ends the episode."""
    from pgdrive_amd import marl_env
    cls = dict(roundabout=marl_env.MultiAgentRoundaboutEnv, intersection=marl_env.MultiAgentIntersectionEnv,
               bottleneck=marl_env.MultiAgentBottleneckEnv, tollgate=marl_env.MultiAgentTollgateEnv,
               parking=marl_env.MultiAgentParkingLotEnv)[kind]
    env = cls(dict(num_agents=8, horizon=150, seed=2))
    D = dict(bottleneck=96, tollgate=156).get(kind, 90)  # bottleneck: 4 side + 6 + 4 lane-line + 10 navi + 72 beams
    try:
        o = env.reset()
        assert len(o) == 8 and all(v.shape == (D, ) for v in o.values())
        assert sorted(o) == ["agent%d" % k for k in range(8)]
        max_id = 7
        seen_new = False
        for t in range(400):
            # even ids floor it (crash / leave the road), odd ids creep: the episode stays alive and slots get re-used
            act = {k: ([0.0, 1.0] if int(k[5:]) % 2 == 0 else [0.0, 0.12]) for k in o}
            o, r, d, i = env.step(act)
            keys = set(o)
            assert keys == set(r) == set(i) == set(d) - {"__all__"}
            for k in keys:
                assert env.vec.single_observation_space.contains(o[k])
                if r[k] == -10.0:
                    assert d[k] and (i[k]["out_of_road"] or i[k]["crash_vehicle"])
                kid = int(k[5:])
                if kid > max_id:
                    seen_new, max_id = True, kid
            if d["__all__"]:
                assert all(d.values())
                break
            o = {k: v for k, v in o.items() if not d[k]}
        assert d["__all__"] and seen_new and t >= 149
    finally:
        env.close()


def test_naive_multi_agent_pgdrive():
    """tests/test_env/test_naive_multi_agent.py:24-66: MultiAgentPGDrive on map "SSS" with four agents whose
    `target_vehicle_configs` line them up on the first lane at longitudes 0 / 5 / 10 / 15 m: Dict spaces, dict-keyed steps,
    and the agents start where they were told (upstream checks that none of them is thrown into the air by overlapping spawns;
    here the first step must report no contact between them and every agent still on its lane)."""
    from pgdrive_amd import marl_env, _abi, mapdata
    env = marl_env.MultiAgentPGDrive(dict(map="SSS", num_agents=4, seed=1,
                                          target_vehicle_configs={"agent%d" % i: dict(spawn_longitude=i * 5) for i in range(4)}))
    try:
        o = env.reset()
        assert isinstance(o, dict) and sorted(o) == ["agent%d" % i for i in range(4)]
        f, i, _ = env.vec.engine.get_state()
        d = env.vec.map_bank.descs[0]
        lane0 = int(i[_abi.SI["LANE"], 0, 0])
        for k in range(4):
            # (the spawn lane is the 10 m entrance lane: the agent told to start at 15 m stands on its straight continuation,
            # and the localisation says so)
            assert (i[_abi.SI["LANE"], 0, k] == lane0) == (5.0 * k <= d["lanes"][lane0]["length"])
            lon, lat = mapdata.lane_local_coordinates(d["lanes"][lane0], (float(f[_abi.SF["X"], 0, k]), float(f[_abi.SF["Y"], 0, k])))
            assert abs(lon - 5.0 * k) < 1e-4 and abs(lat) < 1e-4
        rng = np.random.default_rng(0)
        for t in range(100):
            a = {k: rng.uniform(-1, 1, size=2).astype(np.float32) for k in o}
            o2, r, dn, info = env.step(a)
            assert set(o2) == set(r) == set(info) == set(dn) - {"__all__"}
            for k in o2:
                assert env.vec.single_observation_space.contains(o2[k]) and isinstance(info[k], dict)
            if t == 0:
                assert not any(info[k]["crash_vehicle"] for k in info)
            o = {k: v for k, v in o2.items() if not dn[k]}
            if dn["__all__"]:
                break
    finally:
        env.close()


def test_infinite_agents():
    """tests/test_functionality/test_marl_infinite_agents.py:4-63: num_agents = -1 on the roundabout with short exits (8 spawn slots),
    delay_done 50 / 0, horizon 50: every agent that finishes has lived at least one step, the population never falls below what a
    respawn can refill and grows beyond the initial count when the slot capacity allows it (`max_agents`; the reference itself has no
    cap)."""
    from pgdrive_amd import marl_env
    for delay_done, act, steps in ((50, [1.0, 1.0], 600), (0, [0.0, 1.0], 300)):
        env = marl_env.MultiAgentRoundaboutEnv(dict(map_config=dict(exit_length=20, lane_num=2), num_agents=-1, max_agents=24,
                                                     delay_done=delay_done, horizon=50, seed=100))
        try:
            o = env.reset()
            old_num = max_num = len(o)
            assert old_num == 8  # lane_num 2 x 4 spawn roads x floor((20 - 10) / 8) slots (spawn_manager.py:105-112)
            finished = 0
            for t in range(1, steps):
                o, r, d, info = env.step({k: act for k in o})
                for k, i in info.items():
                    if d[k]:
                        assert i["episode_length"] >= 1
                        finished += 1
                if d["__all__"]:
                    o = env.reset()
                else:
                    o = {k: v for k, v in o.items() if not d[k]}
                max_num = max(max_num, len(o))
            assert finished > 0 and max_num >= old_num
            if delay_done == 0:
                assert max_num > old_num  # respawns while the first agents still drive: more agents than spawn slots
        finally:
            env.close()


def test_safe_env():
    """tests/test_env/test_safe_env.py:4-18 plus the invariants of safe_pgdrive_env.py:7-60: crashes cost instead of ending
    the episode, total_cost accumulates, a traffic object costs only on its first contact."""
    from pgdrive_amd.env import SafePGDriveEnv
    env = SafePGDriveEnv({"environment_num": 20, "start_seed": 75})
    try:
        assert env.config["accident_prob"] == 0.8 and env.config["safe_rl_env"] and env.config["traffic_density"] == 0.05
        n_obj = [i["n_objects"] for i in env.vec.scen_bank.info]
        assert max(n_obj) >= 10 and all(i["objects_dropped"] == 0 for i in env.vec.scen_bank.info)
        o = env.reset()
        assert o.shape == (274, )
        total = 0.0
        crash_steps = 0
        for i in range(1, 400):
            o, r, d, info = env.step([0, 1])
            total += info["cost"]
            assert info["total_cost"] == total and env.observation_space.contains(o)
            if info["crash_vehicle"] or info["crash_object"]:
                crash_steps += 1
                if not (info["out_of_road"] or info["arrive_dest"]):
                    assert info["cost"] == 1.0
                assert not d or info["max_step"]  # a crash step is never terminal (safe_pgdrive_env.py:49-56)
            if d:
                total = 0.0
                o = env.reset(force_seed=75 + (i % 20))
        assert crash_steps >= 0
    finally:
        env.close()


def test_episode_release():
    """tests/test_functionality/test_episode_release.py:5-25: SafePGDriveEnv over 100 maps with accidents and dense traffic, a few
    steps, then two resets in a row, ten times over: every reset hands out a clean episode -- a valid first observation, episode
    counters at zero, nothing of the previous episode's bodies left (no slot beyond what the new scenario's spawn table holds)."""
    import warnings
    from pgdrive_amd import _abi
    from pgdrive_amd.env import SafePGDriveEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (density 0.5 exceeds the 16 traffic seats: the env says so)
        env = SafePGDriveEnv({"environment_num": 100, "accident_prob": 0.8, "traffic_density": 0.5})
    try:
        env.reset()
        for i in range(1, 10):
            for _ in range(4):
                o, r, d, info = env.step([1.0, 1.0])
                assert env.observation_space.contains(o)
            for _ in range(2):
                o = env.reset()
                assert env.observation_space.contains(o)
                f, ii, ei = env.vec.engine.get_state()
                assert ei[_abi.EI["EP_STEPS"], 0] == 0 and f[_abi.SF["EP_REWARD"], 0, 0] == 0.0 and f[_abi.SF["SPEED"], 0, 0] == 0.0
                scen = int(ei[_abi.EI["SCEN"], 0])
                sp = env.vec.scen_bank.spawns.reshape(len(env.vec.scen_bank.scenarios), -1)[scen]
                filled = sp["lane"] >= 0
                st = ii[_abi.SI["STATUS"], 0]
                assert ((st != _abi.ST_EMPTY) == filled).all(), "a body of another episode survived the reset"
                assert st[0] == _abi.ST_ACTIVE and not (ii[_abi.SI["VFLAGS"], 0, 0] & (_abi.F_CRASH_VEHICLE | _abi.F_CRASH_OBJECT))
    finally:
        env.close()


def test_safe_env_cost_to_reward_and_object_contact():
    """cost_to_reward folds the costs into the penalties (safe_pgdrive_env.py:41-47); driving into a cone line gives
    crash_object exactly once per cone."""
    import torch
    from pgdrive_amd import _abi
    from pgdrive_amd.env import SafePGDriveEnv
    from tests.parity import teleport_to_objects
    env = SafePGDriveEnv({"environment_num": 16, "start_seed": 1000, "accident_prob": 1.0, "cost_to_reward": True})
    try:
        assert env.config["crash_object_penalty"] == 6.0 and env.config["out_of_road_penalty"] == 6.0
        hits = 0
        for seed in range(1000, 1016):
            env.reset(force_seed=seed)
            f, i, ei = env.vec.engine.get_state()
            scen = np.array([seed - 1000])
            if not teleport_to_objects(env.vec.map_bank, env.vec.scen_bank, scen, f, i):
                continue
            env.vec.engine.set_state(f, i, ei)
            for t in range(30):
                o, r, d, info = env.step([0, 0.3])
                if info["crash_object"] and not (info["out_of_road"] or info["arrive_dest"] or info["crash_vehicle"]):
                    assert r == -6.0 and info["cost"] == 1.0
                    hits += 1
                if d:
                    break
        assert hits >= 3
    finally:
        env.close()


def test_reference_navigation_controller():
    """tests/test_functionality/test_navigation.py:23-95 (upstream it only has to run): a PID on o[0] -- the lateral distance to the
    left road edge -- towards 0.375 steers the car (action [-steering, acc]), a second PID on the speed [km/h] holds 30, or 20 while
    o[12] (lane angle of the first check point) says a curve is ahead; 10 maps of 7 blocks from seed 5.  On this engine
    the controller must do what it was written to do: keep the car on the road through curves, ramps and junctions and bring it to
    the destination -- which pins the meaning and the sign of o[0], o[12] and of the steering input at once."""
    from pgdrive_amd import _abi
    from pgdrive_amd.env import PGDriveEnv

    class PID:  # component/vehicle_module/PID_controller.py:1-23
        def __init__(self, kp, ki, kd):
            self.kp, self.ki, self.kd = kp, ki, kd
            self.reset()

        def reset(self):
            self.p = self.i = self.d = 0.0

        def get_result(self, e):
            self.i += e
            self.d = e - self.p
            self.p = e
            return -(self.kp * self.p + self.ki * self.i + self.kd * self.d)

    env = PGDriveEnv(dict(environment_num=10, traffic_density=0.0, start_seed=5,  # (the map as upstream's test names it)
                          map_config=dict(type="block_num", config=7, lane_width=3.5, lane_num=3)))
    assert env.config["map_config"]["config"] == 7 and len(env.vec.map_bank.descs[0]["blocks"]) == 8  # first block + 7
    try:
        steer_c, acc_c = PID(1.6, 0.0008, 27.3), PID(0.1, 0.001, 0.3)
        o = env.reset()
        speed = lambda: abs(float(env.vec.engine.get_state()[0][_abi.SF["SPEED"], 0, 0])) * 3.6
        steering = steer_c.get_result(o[0] - 0.375)
        acc = acc_c.get_result(speed() - 30.0)
        ends = []
        for t in range(1, 6000):  # (upstream: 2000 steps; three times that so that several maps are driven to their end)
            o, r, d, info = env.step([-steering, acc])
            steering = steer_c.get_result(o[0] - 0.375)
            t_speed = 30.0 if abs(o[12] - 0.5) < 0.01 else 20.0
            acc = acc_c.get_result(speed() - t_speed)
            if d:
                ends.append("arrive" if info["arrive_dest"] else ("out_of_road" if info["out_of_road"] else "other"))
                o = env.reset()
                steer_c.reset(); acc_c.reset()
                steering = steer_c.get_result(o[0] - 0.375)
                acc = acc_c.get_result(speed() - 30.0)
        print("navigation controller: episodes ended", ends)
        assert len(ends) >= 2 and all(e == "arrive" for e in ends), ends
    finally:
        env.close()


@pytest.mark.parametrize("traffic_density", [0.0, 0.1])
def test_reference_expert_across_the_map_bank(traffic_density):
    """The band evidence behind the kinematic-bicycle substitution (a3), widened from the reference test's one map to the 100
    maps of PGDrive-v0: the reference's PPO expert (trained on Bullet physics, weights = the reference's data file) drives the
    first episode of every map, batched.  Nothing upstream states a number for this, so the assertions are floors well under what
    is measured (printed): most episodes reach the destination, and the rest end the way a driving agent's episodes end."""
    import torch
    from pgdrive_amd import _abi, mapdata
    from pgdrive_amd.vec_env import PGDriveVecEnv
    W = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expert_weights.npz"))
    n = 100
    env = PGDriveVecEnv(dict(num_envs=n, environment_num=n, start_seed=0, traffic_density=traffic_density))
    try:
        descs = env.map_bank.descs
        o = env.reset(force_seed=np.arange(n)).cpu().numpy().astype(np.float64)
        alive = np.ones(n, dtype=bool)
        ep = np.zeros(n); steps = np.zeros(n, dtype=int)
        end = {}
        for t in range(3000):
            f, i, _ = env.engine.get_state()
            legacy = np.empty(n)
            for e in range(n):  # lateral offset inside the current lane (the float today's layout dropped, state_obs.py:97-100)
                lane = descs[e]["lanes"][int(i[_abi.SI["LANE"], e, 0])]
                _, lat = mapdata.lane_local_coordinates(lane, (float(f[_abi.SF["X"], e, 0]), float(f[_abi.SF["Y"], e, 0])))
                legacy[e] = np.clip((lat * 2 / 4.5 + 1.0) / 2.0, 0.0, 1.0)
            x = np.concatenate([o[:, :8], legacy[:, None], o[:, 8:]], axis=1).astype(np.float32)
            x = np.tanh(x @ W["default_policy/fc_1/kernel"] + W["default_policy/fc_1/bias"])
            x = np.tanh(x @ W["default_policy/fc_2/kernel"] + W["default_policy/fc_2/bias"])
            act = (x @ W["default_policy/fc_out/kernel"] + W["default_policy/fc_out/bias"])[:, :2].astype(np.float32)
            ob, r, d, fl = env.step(torch.from_numpy(np.ascontiguousarray(act)).cuda())
            o = ob.cpu().numpy().astype(np.float64)
            r, d = r.cpu().numpy(), d.cpu().numpy().astype(bool)
            info = env.info_from_flags(fl)
            ep[alive] += r[alive]; steps[alive] += 1
            for e in np.nonzero(alive & d)[0]:
                end[e] = "arrive" if info["arrive_dest"][e] else ("out_of_road" if info["out_of_road"][e] else (
                    "crash" if info["crash"][e] else "max_step"))
            alive &= ~d
            if not alive.any():
                break
        kinds = {k: sum(1 for v in end.values() if v == k) for k in ("arrive", "out_of_road", "crash", "max_step")}
        ok = np.array([end.get(e) == "arrive" for e in range(n)])
        print("expert on %d maps, traffic density %.1f: %s, %d unfinished after 3000 steps; mean reward of the arrivals %.1f, mean length %.0f steps"
              % (n, traffic_density, kinds, int(alive.sum()), float(ep[ok].mean()) if ok.any() else 0.0, float(steps[ok].mean()) if ok.any() else 0.0))
        assert not alive.any()
        assert kinds["arrive"] >= (95 if traffic_density == 0.0 else 55)  # measured: 100 / 68
    finally:
        env.close()


@pytest.mark.parametrize("traffic_density", [0.0, 0.1])
def test_reference_expert_policy_reward_band(traffic_density):
    """The reference's own end-to-end band test (tests/test_functionality/test_expert_performance.py:48-85): its PPO expert
    (examples/ppo_expert/expert_weights.npz -- a data file of the reference, kept as a fixture; the 3-layer tanh MLP of
    numpy_expert.py is re-stated below) drives map "CCC", seed 0 for 10 episodes; the mean episode reward must lie in
    (350, 450) and, without traffic, every episode must reach the destination.
    The expert was trained on Bullet physics, so this is the band-level check of our kinematic-bicycle substitution
    together with observation, navigation and reward.  Its input has 275 floats: the 274 of today's layout plus the lateral
    offset inside the current lane after the yaw-rate float, a term that is commented out upstream (state_obs.py:97-100)."""
    from pgdrive_amd import _abi, mapdata
    from pgdrive_amd.env import PGDriveEnv
    W = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expert_weights.npz"))

    def expert(o):
        x = np.tanh(o.reshape(1, -1) @ W["default_policy/fc_1/kernel"] + W["default_policy/fc_1/bias"])
        x = np.tanh(x @ W["default_policy/fc_2/kernel"] + W["default_policy/fc_2/bias"])
        x = (x @ W["default_policy/fc_out/kernel"] + W["default_policy/fc_out/bias"]).reshape(-1)
        return x[:2]  # deterministic: the mean of the Gaussian head

    env = PGDriveEnv(dict(environment_num=1, map="CCC", start_seed=0, traffic_density=traffic_density))
    try:
        d = env.vec.map_bank.descs[0]
        rewards, success = [], []
        o = env.reset()
        ep = 0.0
        for t in range(12000):
            f, i, _ = env.vec.engine.get_state()
            lane = d["lanes"][int(i[_abi.SI["LANE"], 0, 0])]
            _, lat = mapdata.lane_local_coordinates(lane, (float(f[_abi.SF["X"], 0, 0]), float(f[_abi.SF["Y"], 0, 0])))
            legacy = np.clip((lat * 2 / 4.5 + 1.0) / 2.0, 0.0, 1.0)  # MAX_LANE_WIDTH 4.5 (pg_map.py:13)
            o, r, done, info = env.step(expert(np.concatenate([o[:8], [legacy], o[8:]]).astype(np.float32)))
            ep += r
            if done:
                rewards.append(ep)
                success.append(bool(info["arrive_dest"]))
                ep = 0.0
                o = env.reset()
                if len(rewards) == 10:
                    break
        assert len(rewards) == 10
        print("expert: mean episode reward %.1f, success rate %.2f (traffic density %.1f)" % (np.mean(rewards), np.mean(success),
                                                                                           traffic_density))
        assert 350 < np.mean(rewards) < 450, rewards
        if traffic_density == 0.0:
            assert all(success)
    finally:
        env.close()


def test_detectors_see_the_yellow_line_at_spawn():
    """tests/test_functionality/test_distance_detector.py:9-50: at the spawn pose (lane 0, lateral 0) one beam of the
    2-laser side detector and one of the 2-laser lane-line detector end on the yellow centre line ("yellow == 2"): the hit
    is half a lane minus half a line width away; the opposite beams end on the broken line (lane-line detector) and on the
    far side line (side detector)."""
    from pgdrive_amd.env import PGDriveEnv
    env = PGDriveEnv(dict(environment_num=1, start_seed=0, map="XXX", traffic_density=0.0,
                          vehicle_config=dict(side_detector=dict(num_lasers=2, distance=50),
                                              lane_line_detector=dict(num_lasers=2, distance=50))))
    try:
        o = env.reset()
        assert o.shape == (2 + 6 + 2 + 10 + 16 + 240, )
        w = 3.5
        yellow = (w / 2 - 0.075) / 50
        # PGDrive's frame is left-handed (y points down): heading + 90 deg is the driver's RIGHT, heading + 270 deg the LEFT
        assert abs(o[1] - yellow) < 1e-4 and abs(o[9] - yellow) < 1e-4  # beam 1 of both fans ends on the yellow centre line
        assert abs(o[8] - yellow) < 1e-4  # lane-line beam 0: the broken line between lanes 0 and 1, equally far to the right
        assert abs(o[0] - (2.5 * w - 0.075) / 50) < 1e-4  # side beam 0 skips broken lines: the side line of the 3-lane road
    finally:
        env.close()


def test_vehicle_lane_is_among_the_closest_lanes():
    """tests/test_functionality/test_get_closest_lane.py:4-28: on map "rRCXSOTCR" with respawn-mode traffic (density 0.3)
    the lane a vehicle is localised on (ray localisation) must be one of the three closest lanes by L1 distance
    (AbstractLane.distance, abs_lane.py:106-112) or closer than 4 m -- checked for every driving traffic vehicle."""
    import torch
    from pgdrive_amd import _abi, mapdata
    from pgdrive_amd.vec_env import PGDriveVecEnv
    env = PGDriveVecEnv(dict(num_envs=1, environment_num=1, start_seed=0, map="rRCXSOTCR", traffic_density=0.3,
                             traffic_mode="respawn", max_traffic_vehicles=48, auto_reset=False))
    try:
        env.reset()
        d = env.map_bank.descs[0]
        lanes = [l for l in d["lanes"] if d["roads"][l["road"]]["valid"]]
        act = torch.zeros((1, 2), device=env.engine.device)
        checked = 0
        for t in range(400):
            env.step(act)
            if t % 8:
                continue
            env.engine.sync()
            f, i, _ = env.engine.get_state()
            for s in range(1, env.engine.V):
                if i[_abi.SI["STATUS"], 0, s] != _abi.ST_ACTIVE:
                    continue
                p = (float(f[_abi.SF["X"], 0, s]), float(f[_abi.SF["Y"], 0, s]))
                mine = d["lanes"][int(i[_abi.SI["LANE"], 0, s])]

                def l1(l):
                    lon, lat = mapdata.lane_local_coordinates(l, p)
                    return abs(lat) + max(lon - l["length"], 0.0) + max(-lon, 0.0)
                dist = l1(mine)
                rank = sum(1 for l in lanes if l1(l) < dist)
                assert not (dist > 4.0 and rank > 2), (t, s, dist, rank)
                checked += 1
        assert checked > 300
    finally:
        env.close()


def test_obs_noise_config():
    """tests/test_functionality/test_obs_noise.py:23-58: dropout 1.0 wipes the whole lidar cloud, the observation stays
    inside its space for every corner action; 0 / 0 leaves the cloud untouched."""
    from pgdrive_amd.env import PGDriveEnv
    env = PGDriveEnv({"start_seed": 1000, "environment_num": 2, "vehicle_config": {"lidar": {"gaussian_noise": 1.0, "dropout_prob": 1.0}}})
    try:
        o = env.reset()
        assert env.observation_space.contains(o) and (o[-240:] == 0.0).all()
        for x in (-1, 0, 1):
            env.reset()
            for y in (-1, 0, 1):
                o, r, d, info = env.step([x, y])
                assert env.observation_space.contains(o) and (o[-240:] == 0.0).all() and np.isscalar(r)
                for k in ("cost", "velocity", "steering", "acceleration", "step_reward", "crash_vehicle", "out_of_road",
                          "arrive_dest"):
                    assert k in info
    finally:
        env.close()
    env = PGDriveEnv({"start_seed": 1000, "environment_num": 2, "traffic_density": 0.0})
    try:
        assert (env.reset()[-240:] == 1.0).all()
    finally:
        env.close()


def test_generic_multi_agent_vec_env():
    """MultiAgentPGDriveVecEnv: three generated maps, 15 agents, respawn; rows of active slots are valid observations."""
    import torch
    from pgdrive_amd import _abi
    from pgdrive_amd.marl_env import MultiAgentPGDriveVecEnv
    env = MultiAgentPGDriveVecEnv(dict(num_envs=8, start_seed=10, environment_num=3, horizon=150, is_multi_agent=True,
                                       use_render=False, camera_height=4))
    obs = env.reset()
    assert tuple(obs.shape) == (8, 15, 90)
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    new = 0
    for t in range(200):
        a = torch.rand((8, 15, 2), device="cuda", generator=g) * 2 - 1
        a[..., 1] = a[..., 1].abs()
        obs, rew, done, fl = env.step(a)
        new += int(((fl & _abi.F_NEW) != 0).sum().item())
        assert torch.isfinite(obs).all() and float(obs.min()) >= 0.0 and float(obs.max()) <= 1.0
    assert new > 8 * 15
    env.close()



def test_step_captured_in_a_hip_graph_matches_eager():
    """pgd_step is one kernel launch on the caller's stream with static buffers: captured with torch.cuda.graphs and
    replayed, it returns bit-identical results to eager stepping (auto-resets included)."""
    import torch
    from pgdrive_amd import PGDriveVecEnv
    n = 256
    eager = PGDriveVecEnv(dict(num_envs=n, seed=3, start_seed=1000, environment_num=100))
    graphed = PGDriveVecEnv(dict(num_envs=n, seed=3, start_seed=1000, environment_num=100))
    eager.reset(force_seed=np.arange(n) % 100 + 1000)
    graphed.reset(force_seed=np.arange(n) % 100 + 1000)
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    acts = torch.rand((60, n, 2), device="cuda", generator=g) * 2 - 1
    acts[:, :, 1] = acts[:, :, 1].abs()
    a_static = torch.zeros((n, 2), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up on a side stream (builds the reset image outside the capture)
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
    for k in range(1, 60):
        a_static.copy_(acts[k])
        graph.replay()
        o, r, d, f = eager.step(acts[k])
        torch.cuda.synchronize()
        assert torch.equal(o, graphed.engine.obs.view_as(o)) and torch.equal(r, graphed.engine.reward.view_as(r))
        assert torch.equal(d, graphed.engine.done.view_as(d)) and torch.equal(f, graphed.engine.flags.view_as(f))
        n_done += int(d.sum().item())
    assert n_done > 0
    eager.close()
    graphed.close()


@pytest.mark.parametrize("agents", [8, 40])
def test_zero_row_marks_follow_the_buffer_through_graph_replays(agents):
    """a multi-agent step captured with buffer X in a HIP graph, an eager step with `out=` another buffer Y between the
    replays, then X again by replay: the marks of the zero rows carry the identity of the buffer they describe (on the device, per
    env), so every replay zeroes what its own buffer needs -- rows of seats that are not due read zero in X and in Y after every
    step, while both buffers are filled with garbage wherever a row is NOT marked (8 seats: rows appended to k_step; 40 seats: the
    four-wave k_observe_env)."""
    import torch
    from pgdrive_amd import marl_env, _abi
    env = marl_env.MultiAgentRoundaboutVecEnv(dict(num_envs=64, num_agents=agents, seed=4, horizon=60, delay_done=5))
    eng = env.engine
    try:
        env.reset()
        N, A, D = 64, eng.A, eng.D
        g = torch.Generator(device="cuda")
        g.manual_seed(1)
        a_static = torch.zeros((N, A, 2), device="cuda")
        X = (eng.obs, eng.reward, eng.done, eng.flags)
        Y = tuple(torch.empty_like(t) for t in X)
        Y[0].fill_(7.0)  # garbage: every row that is not due must be cleared by the first call that writes Y

        def draw():
            a = torch.rand((N, A, 2), device="cuda", generator=g) * 2 - 1
            a[..., 1] = a[..., 1].abs()
            return a

        def check(buf, flags, what):
            torch.cuda.synchronize()
            due = (flags.cpu().numpy().astype(np.uint32) & (_abi.F_REPORT | _abi.F_NEW)) != 0
            rows = buf.cpu().numpy().reshape(N, A, D)
            assert (rows[~due] == 0.0).all(), what
            assert (np.abs(rows[due]).sum(axis=1) > 0).all(), what
            return int((~due).sum())

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                a_static.copy_(draw())
                eng.step(a_static)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            eng.step(a_static)  # writes X
        n_zero = 0
        for k in range(90):
            a_static.copy_(draw())
            if k % 3 == 1:
                eng.step(a_static, out=Y)  # eager, another buffer: the marks now describe Y
                n_zero += check(Y[0], Y[3], "eager step into Y, step %d" % k)
                Y[0].fill_(7.0)            # ... and the caller scribbles over Y afterwards
            else:
                graph.replay()             # X again, by replay: the kernel sees marks of another buffer and zeroes what X needs
                n_zero += check(X[0], X[3], "replay into X, step %d" % k)
                if k % 3 == 0:
                    X[0].fill_(-3.0)       # garbage in X before the eager step: the next replay follows a call with another buffer
        assert n_zero > 100
    finally:
        env.close()


@pytest.mark.parametrize("agents", [8, 40])
def test_zero_row_marks_do_not_survive_a_reused_address(agents):
    """`Engine.step(out=torch.empty(...))` per step -- torch's caching allocator hands a freed block out again, so a NEW
    buffer can have the address (and row stride) the marks name.  Engine.step forgets the marks (pgd_forget_rows) for every tensor
    it has not seen alive: rows of seats that are not due read zero in every fresh, garbage-filled buffer."""
    import torch
    from pgdrive_amd import marl_env, _abi
    env = marl_env.MultiAgentRoundaboutVecEnv(dict(num_envs=64, num_agents=agents, seed=5, horizon=60, delay_done=5))
    eng = env.engine
    try:
        env.reset()
        N, A, D = 64, eng.A, eng.D
        g = torch.Generator(device="cuda")
        g.manual_seed(2)
        addresses, n_zero = set(), 0
        for k in range(60):
            a = torch.rand((N, A, 2), device="cuda", generator=g) * 2 - 1
            a[..., 1] = a[..., 1].abs()
            Y = tuple(torch.empty_like(t) for t in (eng.obs, eng.reward, eng.done, eng.flags))
            Y[0].fill_(7.0)
            addresses.add(Y[0].data_ptr())
            obs, _, _, fl = eng.step(a, out=Y)
            torch.cuda.synchronize()
            due = (fl.cpu().numpy().astype(np.uint32) & (_abi.F_REPORT | _abi.F_NEW)) != 0
            rows = obs.cpu().numpy().reshape(N, A, D)
            assert (rows[~due] == 0.0).all(), "step %d: a row that is not due kept the garbage of a fresh buffer" % k
            n_zero += int((~due).sum())
            del Y, obs
        assert len(addresses) < 60, "the allocator never re-used an address: the test did not exercise the hazard"
        assert n_zero > 100
    finally:
        env.close()


def test_env_groups_step_like_one_batch(descs):
    """pgd_set_groups / pgd_step_group: four asynchronous env groups of one handle, each stepped once per round on its own
    stream, produce exactly what a plain engine produces for the whole batch (envs do not interact), through auto-resets;
    a group stepped twice is two steps ahead of the others."""
    import torch
    from pgdrive_amd import _abi
    from pgdrive_amd.engine import Engine
    from tests import util
    mb, sb = util.make_banks(descs, n_maps=8)
    n = 256
    cfg = _abi.make_config(n, num_lasers=240, seed=9)
    a, b = Engine(cfg, mb, sb), Engine(cfg, mb, sb)
    ids = np.arange(n) % 8
    a.reset(ids)
    b.reset(ids)
    b.set_groups(4)
    rng = np.random.default_rng(1)
    n_done = 0
    for t in range(150):
        act_np = util.driving_actions(rng, n)
        if t % 3 == 0:
            act_np[::2, 0, 0] = 1.0
            act_np[::2, 0, 1] = 1.0
        act = torch.from_numpy(act_np).to(a.device)
        o, r, dn, fl = [x.clone() for x in a.step(act)]
        a.sync()
        for g in (2, 0, 3, 1):  # any order
            b.step_group(g, act)
        for g in range(4):
            b.group_sync(g)
        assert torch.equal(b.obs, o) and torch.equal(b.reward, r) and torch.equal(b.done, dn) and torch.equal(b.flags, fl)
        n_done += int(dn.sum())
    assert n_done > 30
    # groups advance independently: two more steps of group 1 only
    act = torch.from_numpy(util.driving_actions(rng, n)).to(a.device)
    ref = [x.clone() for x in a.step(act)]
    ref2 = [x.clone() for x in a.step(act)]
    a.sync()
    before = b.obs.clone()
    b.step_group(1, act)
    b.step_group(1, act)
    b.group_sync(1)
    sl = b.group_slice(1)
    assert torch.equal(b.obs[sl], ref2[0][sl])
    others = torch.ones(n, dtype=torch.bool, device=a.device)
    others[sl] = False
    assert torch.equal(b.obs[others], before[others])  # the other groups' rows were not touched
    a.close()
    b.close()
    # the same from the env surface (PGDriveVecEnv.set_groups / step_group / group_sync / group_slice)
    from pgdrive_amd import PGDriveVecEnv
    e1, e2 = (PGDriveVecEnv(dict(num_envs=64, start_seed=1000, environment_num=8, seed=2)) for _ in range(2))
    e1.reset(); e2.reset()
    e2.set_groups(2)
    for t in range(30):
        act = torch.from_numpy(util.driving_actions(rng, 64)).to(e1.engine.device).view(64, 2)
        o, r, dn, fl = [x.clone() for x in e1.step(act)]
        for g in (1, 0):
            og, rg, dg, fg = e2.step_group(g, act)
            e2.group_sync(g)
            s2 = e2.group_slice(g)
            assert torch.equal(og, o[s2]) and torch.equal(rg, r[s2]) and torch.equal(dg, dn[s2]) and torch.equal(fg, fl[s2])
    e1.close(); e2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("multi_agent", [False, True])
def test_step_n_equals_single_steps(multi_agent):
    """pgd_step_n (K steps of an action ring in one call, observation for the last state only) against K calls of pgd_step:
    reward / done / flags of every step, the final observation and the final state are bit-identical."""
    import torch
    from pgdrive_amd import _abi, bank
    from pgdrive_amd.engine import Engine
    from tests import util
    n = 96
    if multi_agent:
        d, mb, sb = util.make_marl_banks(num_agents=8, capacity=8, kind="roundabout")
        cfg = util.marl_config(n, sb, horizon=60, resample_scenario=1, seed=4)
        A = sb.A
    else:
        descs = bank.load_descriptions()
        mb, sb = util.make_banks(descs, n_maps=8)
        cfg = _abi.make_config(n, num_agents=1, num_traffic=16, num_lasers=240, auto_reset=1, resample_scenario=1, seed=4)
        A = 1
    ea, eb = Engine(cfg, mb, sb), Engine(cfg, mb, sb)
    ids = np.arange(n) % len(sb.scenarios)
    ea.reset(ids); eb.reset(ids)
    rng = np.random.default_rng(1)
    L, K = 7, 5
    n_done = 0
    for rep in range(30):
        ring = np.stack([util.marl_actions(rng, n, A) if multi_agent else util.driving_actions(rng, n) for _ in range(L)])
        if not multi_agent:
            ring[:, ::3, 0, :] = 1.0  # a third of the envs: hard right at full throttle (episodes end, auto-reset inside the call)
        ring_d = torch.from_numpy(ring).to(ea.device)
        first = rep % L
        obs_n, rew_n, done_n, fl_n = ea.step_n(ring_d, first, K)
        ea.sync()
        for k in range(K):
            o, r, dn, fl = eb.step(ring_d[(first + k) % L])
            eb.sync()
            assert torch.equal(rew_n[k], r) and torch.equal(done_n[k], dn) and torch.equal(fl_n[k], fl), (rep, k)
            n_done += int(dn.sum().item())
        assert torch.equal(obs_n, o), rep
        fa, ia, eia = ea.get_state()
        fb, ib, eib = eb.get_state()
        ei_near = _abi.EI["NEAR"]
        assert (ia == ib).all() and (np.delete(eia, ei_near, axis=0) == np.delete(eib, ei_near, axis=0)).all()
        assert (fa.view(np.int32) == fb.view(np.int32)).all()
    assert n_done > 20
    ea.close(); eb.close()


def test_scripted_lane_keeping_policy_drives_to_the_destination(descs):
    """pgd_lane_keep_actions (the library's scripted stand-in for the reference's shipped PPO expert: road-centre offset +
    heading error -> steering, cruise control -> throttle, from the rows pgd_step wrote): 256 envs on 8 maps without traffic --
    the ego keeps driving (mean speed near the 30 km/h target), stays on the road and most episodes end by ARRIVAL; actions are
    reproducible (counter RNG) and inside [-1, 1]."""
    import torch
    from pgdrive_amd import _abi
    from pgdrive_amd.engine import Engine
    from tests import util
    n = 256
    mb, sb = util.make_banks(descs, n_maps=8, density=0.0)
    cfg = _abi.make_config(n, num_agents=1, num_traffic=16, num_lasers=240, auto_reset=1, seed=5)
    eng = Engine(cfg, mb, sb)
    eng.reset(np.arange(n) % 8)
    act = torch.zeros((n, 1, 2), dtype=torch.float32, device=eng.device)
    act2 = torch.zeros_like(act)
    arrive = out = steps = 0
    speed = []
    for t in range(900):
        eng.lane_keep_actions(act, t)
        if t == 10:
            eng.lane_keep_actions(act2, t)
            eng.sync()
            assert torch.equal(act, act2) and float(act.abs().max()) <= 1.0
        obs, rew, done, flags = eng.step(act)
        eng.sync()
        fl = flags.cpu().numpy().astype(np.uint32)[:, 0]
        arrive += int(((fl & _abi.F_ARRIVE) != 0).sum())
        out += int(((fl & _abi.F_OUT_OF_ROAD) != 0).sum())
        if t % 50 == 49:
            speed.append(float(obs[:, 0, 3].mean().item()) * 81.0 - 1.0)
    print("scripted policy: arrivals %d, out of road %d, mean speed %.1f km/h" % (arrive, out, float(np.mean(speed))))
    assert arrive >= 200 and out <= 0.25 * arrive and 20.0 < np.mean(speed) < 35.0
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own end-to-end property tests at the Bullet boundary (the only things that pin behaviour there),
# run on the engine through the gym-shaped wrapper.  Together with the expert band above they are the evidence behind the
# kinematic-bicycle substitution: steering sign, line / sidewalk contact semantics, vehicle contacts,
# the side detector against the road edge.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steering", [-0.01, 0.01])
@pytest.mark.parametrize("distance", [10, 50, 100])
def test_reference_out_of_road_property(steering, distance):
    """tests/test_functionality/test_out_of_road.py:7-36: on eleven straight blocks a slight constant steering (either way) at full
    throttle ends the episode, and at that moment the nearest continuous line seen by the 120-beam side detector is closer than
    the vehicle's diagonal (cloud point < sqrt(W^2 + L^2) / distance)."""
    from pgdrive_amd.env import PGDriveEnv
    env = PGDriveEnv(dict(map="SSSSSSSSSSS", environment_num=1, start_seed=0,
                          vehicle_config=dict(side_detector=dict(num_lasers=120, distance=distance))))
    try:
        env.reset()
        tol = np.sqrt(1.852 ** 2 + 4.51 ** 2) / distance  # DefaultVehicle WIDTH / LENGTH (vehicle_type.py:9-16)
        for t in range(3000):
            o, r, d, info = env.step([steering, 1.0])
            if d:
                break
        assert d and info["out_of_road"] and not info["arrive_dest"], (t, info)
        side = o[:120]
        assert side.min() < tol, (float(side.min()), tol)
    finally:
        env.close()


def test_reference_collision_with_vehicle():
    """tests/test_functionality/test_collision.py:4-21: traffic density 1.0 on three straights, full throttle straight ahead:
    the ego runs into a traffic vehicle within 500 steps."""
    from pgdrive_amd.env import PGDriveEnv
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (density 1.0 asks for more vehicles than the slot cap holds: said so by name)
        env = PGDriveEnv(dict(traffic_density=1.0, map="SSS", environment_num=1, start_seed=0, max_traffic_vehicles=62))
    try:
        env.reset()
        hit = False
        for t in range(1, 500):
            o, r, d, info = env.step([0.0, 1.0])
            if info["crash_vehicle"]:
                hit = True
                break
        assert hit, "no vehicle contact in 500 steps at traffic density 1.0"
        assert d and r == -5.0  # crash_vehicle_penalty, terminal (pgdrive_env.py:162-258)
    finally:
        env.close()


def test_reference_line_contact_and_sidewalk():
    """tests/test_functionality/test_collision.py:24-50: without traffic, steering -0.5 at full throttle for 99 steps (the
    reference keeps stepping after done) -- the car crosses BROKEN lines and reaches the WHITE continuous side line, and it
    crashes into the sidewalk.  From the left-most lane that is a turn to the RIGHT: the test also pins the sign of the
    steering input against the reference (the other way the car would meet the yellow centre line first)."""
    from pgdrive_amd import _abi
    from pgdrive_amd.env import PGDriveEnv
    env = PGDriveEnv(dict(traffic_density=0.0, environment_num=1, start_seed=0))
    try:
        env.reset()
        seen = 0
        first_done = None
        for t in range(1, 100):
            o, r, d, info = env.step([-0.5, 1.0])
            _, i, _ = env.vec.engine.get_state()
            seen |= int(i[_abi.SI["VFLAGS"], 0, 0])
            if d and first_done is None:
                first_done = dict(info)
        assert seen & _abi.F_ON_BROKEN and seen & _abi.F_ON_WHITE, hex(seen)
        assert seen & _abi.F_CRASH_SIDEWALK, hex(seen)
        assert not (seen & _abi.F_ON_YELLOW), "steering -0.5 must turn away from the centre line"
        assert first_done is not None and first_done["out_of_road"]
    finally:
        env.close()


@pytest.mark.gpu
def test_gym_make_returns_the_reference_shapes(tmp_path):
    """VERDICT r05 item 7, on the GPU: with a `gym` on the path (tests/util.py write_fake_gym: this image has none),
    `gym.make("PGDrive-v0")` builds pgdrive_amd.env.PGDriveEnv with register.py's config, the env is a gym.Env, its spaces are
    gym's Box(274) / Box(2), and reset / step have the reference's call shapes (base_env.py:184-193, 269-290)."""
    import json
    import os
    import subprocess
    import sys
    from tests import util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fake = util.write_fake_gym(tmp_path)
    code = """
import json, sys
sys.path.insert(0, %r)
import numpy as np
import gym
import pgdrive_amd
env = gym.make("PGDrive-v0")
o = env.reset()
o2, r, d, info = env.step(np.array([0.0, 1.0], dtype=np.float32))
print(json.dumps(dict(is_env=isinstance(env, gym.Env), cls=type(env).__name__, seeds=[env.config["start_seed"], env.config["environment_num"]],
                      obs_space=[type(env.observation_space).__module__, list(env.observation_space.shape)],
                      act_space=[type(env.action_space).__module__, list(env.action_space.shape)],
                      o=[list(o.shape), str(o.dtype)], o2=[list(o2.shape), str(o2.dtype)], r=type(r).__name__, d=type(d).__name__,
                      info=sorted(info)[:3], in_space=bool(env.observation_space.contains(o2)))))
env.close()
""" % root
    env = dict(os.environ, PYTHONPATH=fake + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["is_env"] and d["cls"] == "PGDriveEnv" and d["seeds"] == [1000, 100]
    assert d["obs_space"] == ["gym.spaces", [274]] and d["act_space"] == ["gym.spaces", [2]]
    assert d["o"] == [[274], "float32"] and d["o2"] == [[274], "float32"] and d["r"] == "float" and d["d"] == "bool" and d["in_space"]


def _mlp_numpy(x, w1, b1, w2, b2, w3, b3, final_tanh):
    """pgdrive/examples/ppo_expert/numpy_expert.py:25-44 re-stated in float64 (the checker, tests/policy_ref.py)."""
    from tests.policy_ref import mlp_f64
    return mlp_f64(x, (w1, b1, w2, b2, w3, b3), final_tanh)


@pytest.mark.parametrize("case", ["expert_weights", "random_274", "groups"])
def test_mlp_policy_matches_the_numpy_expert(descs, case):
    """pgd_mlp_policy (pgdrive_amd/csrc/pgd_policy.h: the policy network of the closed loop in one launch, f32 matrix cores) against
    the reference's numpy expert: (a) the reference's own PPO weights (examples/ppo_expert/expert_weights.npz, kept as a fixture:
    275 inputs, 4 outputs of which the first two are the action) on random observation rows of a wider buffer, a row count that is
    not a multiple of the kernel's 16-row tile; (b) random 274-256-256-2 weights on the engine's own observation buffer, with the
    final tanh; (c) the same per env group on the groups' streams.  fp32 against a float64 restatement: 2e-5."""
    import torch
    from pgdrive_amd import _abi
    from pgdrive_amd.engine import Engine
    from tests import util
    mb, sb = util.make_banks(descs, n_maps=8)
    rng = np.random.default_rng(3)
    n = 100 if case != "groups" else 96
    eng = Engine(_abi.make_config(n, seed=2), mb, sb)
    try:
        eng.reset(np.arange(n) % 8)
        if case == "expert_weights":
            Wz = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expert_weights.npz"))
            w = [Wz["default_policy/fc_1/kernel"], Wz["default_policy/fc_1/bias"], Wz["default_policy/fc_2/kernel"],
                 Wz["default_policy/fc_2/bias"], Wz["default_policy/fc_out/kernel"], Wz["default_policy/fc_out/bias"]]
            assert w[0].shape == (275, 256) and w[4].shape == (256, 4)
            x = np.clip(rng.normal(0.5, 1.0, size=(n, 288)), 0.0, 1.0).astype(np.float32)  # (numpy_expert.py's own self-test input)
            x[:, 275:] = np.nan  # columns beyond in_dim are never read
            obs, in_dim, ft = torch.from_numpy(x).cuda(), 275, False
        else:
            w = [rng.normal(0, 0.08, size=(274, 256)), rng.normal(0, 0.1, size=256), rng.normal(0, 0.08, size=(256, 256)),
                 rng.normal(0, 0.1, size=256), rng.normal(0, 0.1, size=(256, 2)), rng.normal(0, 0.1, size=2)]
            a = torch.from_numpy(util.driving_actions(rng, n)).cuda()
            for _ in range(5):
                eng.step(a)
            eng.sync()
            obs, in_dim, ft = None, 274, True
            x = eng.obs.view(n, -1).cpu().numpy()
        w = [np.ascontiguousarray(v, dtype=np.float32) for v in w]
        wt = tuple(torch.from_numpy(v).cuda() for v in w)
        out = torch.full((n, 1, 2), 7.0, dtype=torch.float32, device="cuda")
        if case == "groups":
            eng.set_groups(4)
            for g in range(4):
                eng.mlp_policy(wt, out, group=g, final_tanh=ft)
            for g in range(4):
                eng.group_sync(g)
        else:
            eng.mlp_policy(wt, out, obs=obs, final_tanh=ft, in_dim=in_dim)
            eng.sync()
        want = _mlp_numpy(x[:, :in_dim], *w, ft)
        got = out.view(n, 2).cpu().numpy()
        assert np.isfinite(got).all() and np.abs(got - want).max() < 2e-5, np.abs(got - want).max()
        assert np.abs(want).max() > 0.05  # (not a trivially small network output)
        # the same network with split bf16 operands on prepared weights (pgd_mlp_prepare / pgd_mlp_policy_prepared): every value as
        # hi + lo, a product as three bf16 matrix instructions -- 16 bits of mantissa, not 24: held to 1e-4 (measured ~3e-5)
        prep = eng.mlp_prepare(wt)
        eng.sync()  # (prepared on the engine's stream, read on the groups' own: not ordered against each other, include/pgdrive_hip.h)
        assert prep.numel() == eng.L.pgd_mlp_prepared_bytes(in_dim)
        out2 = torch.full((n, 1, 2), 7.0, dtype=torch.float32, device="cuda")
        if case == "groups":
            for g in range(4):
                eng.mlp_policy(None, out2, group=g, final_tanh=ft, prepared=prep)
            for g in range(4):
                eng.group_sync(g)
        else:
            eng.mlp_policy(None, out2, obs=obs, final_tanh=ft, in_dim=in_dim, prepared=prep)
            eng.sync()
        got2 = out2.view(n, 2).cpu().numpy()
        err2 = float(np.abs(got2 - want).max())
        print("split-bf16 policy, %s: max |action - float64| = %.2e (exact-f32 kernel: %.2e)" % (case, err2, float(np.abs(got - want).max())))
        assert np.isfinite(got2).all() and err2 < 1e-4, err2
        # the arguments the library refuses: another hidden width, a row stride below the input width
        import ctypes as C
        p = [C.c_void_p(t.data_ptr()) for t in wt]
        o2 = eng.obs.view(n, -1)
        assert eng.L.pgd_mlp_policy(eng.h, -1, C.c_void_p(o2.data_ptr()), 274, 274, 128, *p, 2, 0, C.c_void_p(out.data_ptr())) == 1
        assert eng.L.pgd_mlp_policy(eng.h, -1, C.c_void_p(o2.data_ptr()), 100, 274, 256, *p, 2, 0, C.c_void_p(out.data_ptr())) == 1
    finally:
        eng.close()


@pytest.mark.parametrize("pack", ["0", "1"])
def test_step_lane_keep_equals_policy_then_step(descs, monkeypatch, pack):
    """pgd_step_lane_keep (round 6: the scripted lane-keeping policy evaluated by the step kernel itself, from the row the previous
    step wrote) against pgd_lane_keep_actions + pgd_step: the same arithmetic compiled into both kernels (fused multiply-adds written
    out), so every output is BIT-identical over 300 closed-loop steps with auto-resets -- with one env per wave (one launch) and with
    several envs per wave (PGD_PACK=1: the call falls back to the two launches itself)."""
    import torch
    from pgdrive_amd import _abi
    from pgdrive_amd.engine import Engine
    from tests import util
    monkeypatch.setenv("PGD_PACK", pack)
    mb, sb = util.make_banks(descs, n_maps=8)
    n = 99
    a, b = Engine(_abi.make_config(n, auto_reset=1, seed=5), mb, sb), Engine(_abi.make_config(n, auto_reset=1, seed=5), mb, sb)
    try:
        ids = np.arange(n) % 8
        a.reset(ids); b.reset(ids)
        act = torch.zeros((n, 1, 2), device="cuda")
        n_done = 0
        for t in range(300):
            a.lane_keep_actions(act, t)
            o1, r1, d1, f1 = [x.clone() for x in a.step(act)]
            o2, r2, d2, f2 = b.step_lane_keep(t)
            a.sync(); b.sync()
            assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2) and torch.equal(f1, f2), "step %d" % t
            n_done += int(d1.sum())
        assert n_done > 5 and float(a.get_state()[0][_abi.SF["SPEED"]][:, 0].mean()) > 2.0  # (the egos drive)
        assert ("throughput" in b.describe_step()) == (pack == "1")
    finally:
        a.close(); b.close()
