"""ctypes mirror of the plain-C structs in include/pgdrive_hip.h (kept in lock-step by tests/test_abi.py)."""
import ctypes as C


class PgdConfig(C.Structure):
    _fields_ = [
        ("num_envs", C.c_int32), ("num_agents", C.c_int32), ("num_traffic", C.c_int32), ("num_lasers", C.c_int32),
        ("num_others", C.c_int32), ("lidar_dist", C.c_float), ("dt", C.c_float), ("decision_repeat", C.c_int32),
        ("auto_reset", C.c_int32), ("resample_scenario", C.c_int32), ("horizon", C.c_int32), ("seed", C.c_uint32),
        ("success_reward", C.c_float), ("out_of_road_penalty", C.c_float), ("crash_vehicle_penalty", C.c_float),
        ("crash_object_penalty", C.c_float), ("driving_reward", C.c_float), ("speed_reward", C.c_float),
        ("use_lateral", C.c_int32), ("out_of_route_done", C.c_int32), ("marl_flags", C.c_int32),
        ("delay_done", C.c_int32), ("agent_limit", C.c_int32), ("respawn_places", C.c_int32),
        ("respawn_dests", C.c_int32), ("side_lasers", C.c_int32), ("side_dist", C.c_float),
        ("lane_line_lasers", C.c_int32), ("lane_line_dist", C.c_float), ("discrete_action", C.c_int32),
        ("discrete_steering_dim", C.c_int32), ("discrete_throttle_dim", C.c_int32), ("increment_steering", C.c_int32),
        ("safe_rl_env", C.c_int32), ("overspeed_penalty", C.c_float), ("min_pass_steps", C.c_int32),
        ("enable_reverse", C.c_int32), ("lidar_gaussian_noise", C.c_float), ("lidar_dropout_prob", C.c_float),
        ("random_agent_model", C.c_int32), ("env_base", C.c_int32), ("idm_agent", C.c_int32),
        ("idm_steer_lag", C.c_float),
    ]


class TopDownConfig(C.Structure):
    """pgd_topdown_config; defaults = TopDownPGDriveEnv (envs/top_down_env.py:8-42)."""
    _fields_ = [("resolution", C.c_int32), ("distance", C.c_float), ("frame_stack", C.c_int32), ("post_stack", C.c_int32),
                ("frame_skip", C.c_int32), ("mode", C.c_int32)]


class RenderConfig(C.Structure):
    """pgd_render_config; pgdrive_amd/render.py fills it from the arguments of env.render(mode="top_down", ...)."""
    _fields_ = [("film_w", C.c_int32), ("film_h", C.c_int32), ("num_stack", C.c_int32), ("history_smooth", C.c_int32),
                ("light_background", C.c_int32), ("road_rgb", C.c_int32 * 3), ("draw_traffic", C.c_int32)]


class StepInfo(C.Structure):
    """pgd_step_info: three costs and caller-owned device pointers (None = not written)."""
    _fields_ = [("out_of_road_cost", C.c_float), ("crash_vehicle_cost", C.c_float), ("crash_object_cost", C.c_float), ("pad", C.c_int32)] + \
        [(n, C.c_void_p) for n in ("final_obs", "velocity", "steering", "acceleration", "episode_energy", "step_energy", "episode_reward",
                                   "episode_length", "cost", "total_cost", "ep_count", "ep_return_sum", "ep_length_sum", "ep_cost_sum",
                                   "ep_arrive", "ep_out_of_road", "ep_crash", "ep_max_step")]


class ActorCritic(C.Structure):
    """pgd_actor_critic: the device pointers of the policy network (out_cols >= 4: mean 0..1, log_std 2..3) and of the value network
    (all six None = no critic)."""
    _fields_ = [(n, C.c_void_p) for n in ("w1", "b1", "w2", "b2", "w3", "b3")] + [("out_cols", C.c_int32)] + \
        [(n, C.c_void_p) for n in ("vw1", "vb1", "vw2", "vb2", "vw3", "vb3")]


AC_DETERMINISTIC = 1
AC_EMIT_INDEX = 2  # PGD_AC_EMIT_INDEX: the categorical head writes the index, not the grid value, into the action buffer
CAT_COLS = 16  # the categorical head's tile: ks + kt <= 16


def cat_bins(bins, where):
    """`bins` = (ks, kt) of the categorical head checked (ValueError) -> two ints: 2 <= ks, kt and ks + kt <= 16.  No device needed."""
    try:
        ks, kt = bins
        ok = int(ks) == ks and int(kt) == kt and not isinstance(ks, bool) and not isinstance(kt, bool)
    except (TypeError, ValueError):
        ok = False
    if not ok or ks < 2 or kt < 2 or ks + kt > CAT_COLS:
        raise ValueError("%s: bins = %r: (steering, throttle) with 2 <= each and steering + throttle <= %d wanted" % (where, bins, CAT_COLS))
    return int(ks), int(kt)


class GuardianConfig(C.Structure):
    """pgd_guardian_config: the expert's input width, save_level, the noise's seed and tick, the PGD_GUARD_* mode bits."""
    _fields_ = [("expert_in_dim", C.c_int32), ("save_level", C.c_float), ("seed", C.c_uint32), ("tick", C.c_uint32), ("mode", C.c_uint32)]


GUARD_LEGACY_LATERAL, GUARD_DETERMINISTIC, GUARD_IMMEDIATE = 1, 2, 4  # PGD_GUARD_*, mode bits of pgd_guardian
GUARD_TAKEOVER, GUARD_TAKEOVER_START, GUARD_TAKEOVER_END = 1, 2, 4  # the bits of pgd_guardian's d_info
GUARD_MIN_LASERS = 40  # the reference's lidar slices need forty beams


def guardian_unserved(cfg):
    """What of an engine's config the guardian does not serve, as the end of a refusal's sentence, or None.  `cfg`: the engine's
    config, or anything with its idm_agent, discrete_action, lidar_gaussian_noise, lidar_dropout_prob and num_lasers."""
    if cfg.idm_agent:
        return "IDM_agent: the ego is driven by IDMPolicy, there is no action to guard"
    if cfg.discrete_action:
        return "discrete_action: the guardian compares continuous actions"
    if cfg.lidar_gaussian_noise != 0.0 or cfg.lidar_dropout_prob != 0.0:
        return "lidar gaussian_noise / dropout_prob: the reference's guardian reads the un-noised cloud points, which this engine does not keep"
    if cfg.num_lasers < GUARD_MIN_LASERS:
        return "fewer than %d lidar beams (num_lasers): the guardian's fan slices need them" % GUARD_MIN_LASERS
    return None


class PPOBatch(C.Structure):
    """pgd_ppo_batch: the rollout's arrays by row, the row list (index / count null: position = row, n_list entries) and the minibatch
    (start, stride, rows)."""
    _fields_ = [(n, C.c_void_p) for n in ("obs", "action", "logp_old", "adv", "ret", "adv_stats", "index", "count")] + \
        [(n, C.c_int32) for n in ("obs_stride", "in_dim", "n_rows", "n_list", "start", "stride", "rows")]


class PPOHyper(C.Structure):
    """pgd_ppo_hyper"""
    _fields_ = [("clip", C.c_float), ("vf_coef", C.c_float), ("ent_coef", C.c_float)]


class PPOGrads(C.Structure):
    """pgd_ppo_grads: gradient buffers of the weights' own shapes (the critic's six None without a critic)."""
    _fields_ = [(n, C.c_void_p) for n in ("w1", "b1", "w2", "b2", "w3", "b3", "vw1", "vb1", "vw2", "vb2", "vw3", "vb3")]


class ValueNet(C.Structure):
    """pgd_value_net: the device pointers of a critic-shaped network (w3 [256][1]) -- the cost critic."""
    _fields_ = [(n, C.c_void_p) for n in ("w1", "b1", "w2", "b2", "w3", "b3")]


class PPOCost(C.Structure):
    """pgd_ppo_cost: the cost critic's targets by rollout row and its loss coefficient."""
    _fields_ = [("cost_ret", C.c_void_p), ("cvf_coef", C.c_float)]


class ValueGrads(C.Structure):
    """pgd_value_grads: the cost critic's gradient buffers, of its weights' shapes."""
    _fields_ = [(n, C.c_void_p) for n in ("w1", "b1", "w2", "b2", "w3", "b3")]


class PPOGuide(C.Structure):
    """pgd_ppo_guide: the target actions and the guided-row mask BY ROLLOUT ROW (mask None: every live row is guided), the target's row
    stride in floats, the mask bits that make a row guided, the imitation weight and the GUIDE_* mode bits."""
    _fields_ = [("target", C.c_void_p), ("mask", C.c_void_p), ("target_stride", C.c_int32), ("mask_bits", C.c_uint32), ("bc_coef", C.c_float),
                ("mode", C.c_uint32)]


GUIDE_KEEP_SURROGATE = 1  # PGD_GUIDE_KEEP_SURROGATE, a mode bit of pgd_ppo_grad_guided: a guided row keeps its clipped surrogate
PPO_ROWS_MAX = 16777216
PPO_STATS = ("n", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "ratio", "reserved")  # d_stats of pgd_ppo_grad
PPO_COST_STATS = PPO_STATS[:7] + ("cost_value_loss", )  # d_stats of pgd_ppo_grad_cost
# d_stats of pgd_ppo_grad_guided: slots 1, 4, 5, 6 average the rows that carry the surrogate, bc_loss the guided rows
PPO_GUIDED_STATS = PPO_COST_STATS + ("guided_rows", "bc_loss", "reserved_10", "reserved_11")
ADAM_GATE = ("stopped", "applied", "skipped", "skipped_now")  # d_gate of pgd_adam_gated, four int32
LAGRANGE_STATE = ("lambda", "episode_cost", "episodes", "reserved")  # d_state of pgd_lagrange
RN_FREEZE = 1  # PGD_RN_FREEZE, a mode bit of pgd_return_norm
RETURN_NORM_RECORD = ("count", "mean", "m2", "scale")  # d_record of pgd_return_norm, four doubles
RETURN_NORM_INIT = (1e-4, 0.0, 1e-4, 1.0)  # the record before the first call: VecNormalize's RunningMeanStd (mean 0, variance 1, count 1e-4)
EP_SEATS = 1  # PGD_EP_SEATS, a mode bit of pgd_rollout_episodes
ROLLOUT_EPISODES = ("episodes", "return_mean", "return_m2", "return_min", "return_max", "length_sum", "length_max", "arrive", "out_of_road",
                    "crash_vehicle", "crash_object", "crash_building", "max_step", "cut", "steps", "calls")  # a record of pgd_rollout_episodes, 16 doubles
ROLLOUT_EPISODES_INIT = (0.0, 0.0, 0.0, float("inf"), float("-inf")) + (0.0, ) * 11  # the record before the first call
OBS_NORM_DIMS = (4, 416)  # the input widths pgd_obs_norm_update / _publish / _bind accept, both ends included
OBS_NORM_PART = 512       # list positions per partition of pgd_obs_norm_update's sums


def obs_norm_layout(in_dim):
    """(record doubles, table shape) of the observation normalisation: d_record of pgd_obs_norm_update is n | means | m2s, d_table of
    pgd_obs_norm_publish / _bind is float32 [2][Dp], shift | scale, Dp = in_dim rounded up to a multiple of 4."""
    return 1 + 2 * int(in_dim), (2, (int(in_dim) + 3) & ~3)

# the tensors of Engine.enable_step_info by pgd_step_info field: (dtype name, key in Engine.step_info)
STEP_INFO_FIELDS = dict(
    velocity="float32", steering="float32", acceleration="float32", episode_energy="float32", step_energy="float32",
    episode_reward="float32", episode_length="int32", cost="float32", total_cost="float32", ep_count="int32", ep_return_sum="float32",
    ep_length_sum="int32", ep_cost_sum="float32", ep_arrive="int32", ep_out_of_road="int32", ep_crash="int32", ep_max_step="int32")


def make_topdown_config(resolution=84, distance=30.0, frame_stack=3, post_stack=5, frame_skip=5, mode=0):
    """mode 1: the single RGB frame of TopDownObservation (obs/top_down_obs.py; reference default resolution 200)."""
    return TopDownConfig(int(resolution), float(distance), int(frame_stack), int(post_stack), int(frame_skip), int(mode))


def make_config(num_envs, num_agents=1, num_traffic=16, num_lasers=240, num_others=4, lidar_dist=50.0, dt=0.02,
                decision_repeat=5, auto_reset=1, resample_scenario=0, horizon=0, seed=0, success_reward=10.0,
                out_of_road_penalty=5.0, crash_vehicle_penalty=5.0, crash_object_penalty=5.0, driving_reward=1.0,
                speed_reward=0.1, use_lateral=False, out_of_route_done=False, multi_agent=False, crash_done=True,
                out_of_road_done=True, allow_respawn=True, delay_done=25, agent_limit=0, respawn_places=0,
                respawn_dests=0, side_lasers=0, side_dist=50.0, lane_line_lasers=0, lane_line_dist=20.0,
                discrete_action=False, discrete_steering_dim=5, discrete_throttle_dim=5, increment_steering=False,
                safe_rl_env=False, plain_reward=False, cross_yellow_line_done=True, tollgate=False, overspeed_penalty=0.5,
                min_pass_steps=30, enable_reverse=False, parking=False, others_state=False, random_agent_model=False,
                lidar_gaussian_noise=0.0, lidar_dropout_prob=0.0, env_base=0, idm_agent=False, idm_steer_lag=0.0):
    """Defaults mirror PGDriveEnv_DEFAULT_CONFIG / BASE_DEFAULT_CONFIG (pgdrive_env.py:22-109, base_env.py:19-90)."""
    c = PgdConfig()
    c.num_envs, c.num_agents, c.num_traffic = num_envs, num_agents, num_traffic
    c.num_lasers, c.num_others, c.lidar_dist = num_lasers, (num_others if num_lasers > 0 else 0), lidar_dist
    c.dt, c.decision_repeat = dt, decision_repeat
    c.auto_reset, c.resample_scenario, c.horizon, c.seed = int(auto_reset), int(resample_scenario), int(horizon or 0), seed
    c.success_reward, c.out_of_road_penalty = success_reward, out_of_road_penalty
    c.crash_vehicle_penalty, c.crash_object_penalty = crash_vehicle_penalty, crash_object_penalty
    c.driving_reward, c.speed_reward = driving_reward, speed_reward
    c.use_lateral, c.out_of_route_done = int(bool(use_lateral)), int(bool(out_of_route_done))
    c.side_lasers, c.side_dist = int(side_lasers), float(side_dist)
    c.lane_line_lasers, c.lane_line_dist = int(lane_line_lasers), float(lane_line_dist)
    c.discrete_action, c.increment_steering = int(bool(discrete_action)), int(bool(increment_steering))
    c.discrete_steering_dim, c.discrete_throttle_dim = int(discrete_steering_dim), int(discrete_throttle_dim)
    c.safe_rl_env = int(bool(safe_rl_env))
    c.env_base = int(env_base)
    c.idm_agent = int(bool(idm_agent))
    c.idm_steer_lag = float(idm_steer_lag)  # (an extension, default off: include/pgdrive_hip.h)
    c.enable_reverse = int(bool(enable_reverse))
    c.random_agent_model = int(bool(random_agent_model))
    c.lidar_gaussian_noise, c.lidar_dropout_prob = float(lidar_gaussian_noise), float(lidar_dropout_prob)
    if multi_agent:
        c.marl_flags = MA_ENABLED | (MA_CRASH_DONE if crash_done else 0) | (MA_OUT_ROAD_DONE if out_of_road_done else 0) | \
            (MA_ALLOW_RESPAWN if allow_respawn else 0) | (MA_PLAIN_REWARD if plain_reward else 0) | \
            (0 if cross_yellow_line_done else MA_YELLOW_OK) | (MA_TOLLGATE if tollgate else 0) | \
            (MA_PARKING if parking else 0) | (MA_OTHERS_STATE if others_state else 0)
        c.overspeed_penalty, c.min_pass_steps = float(overspeed_penalty), int(min_pass_steps)
        c.delay_done, c.agent_limit = int(delay_done), int(agent_limit or num_agents)
        c.respawn_places, c.respawn_dests = int(respawn_places), int(respawn_dests)
    return c


def obs_dim(cfg):
    toll = bool(cfg.marl_flags & MA_TOLLGATE)
    state = (cfg.side_lasers or 2) + 6 + cfg.lane_line_lasers + (2 if cfg.random_agent_model else 0) + (0 if toll else 10)
    per_other = state if cfg.marl_flags & MA_OTHERS_STATE else 4
    return state + per_other * cfg.num_others + cfg.num_lasers + (2 if toll else 0)


# state layout (include/pgd_state_layout.h)
SF = dict(X=0, Y=1, THETA=2, SPEED=3, STEER=4, THROTTLE=5, LASTX=6, LASTY=7, LASTHX=8, LASTHY=9, ACT0S=10, ACT0T=11,
          ACT1S=12, ACT1T=13, PID_HP=14, PID_HI=15, PID_LP=16, PID_LI=17, TARGET_SPEED=18, ENERGY=19, DIST_LEFT=20,
          DIST_RIGHT=21, EP_REWARD=22, AGENT_ID=23, HX=24, HY=25)
SI = dict(STATUS=0, LANE=1, CK0=2, CK1=3, RLANE=4, TIMER=5, VFLAGS=6, SPAWN=7)
EI = dict(SCEN=0, NEXT_GROUP=1, EP_STEPS=2, EPISODES=3, STEPS_TOTAL=4, NEXT_AGENT=5, AUX=6, NEAR=7)
NF, NI, NEI = 26, 8, 8
ST_EMPTY, ST_PENDING, ST_ACTIVE, ST_REMOVED, ST_DYING = 0, 1, 2, 3, 4
MA_ENABLED, MA_CRASH_DONE, MA_OUT_ROAD_DONE, MA_ALLOW_RESPAWN, MA_PLAIN_REWARD, MA_YELLOW_OK, MA_TOLLGATE = 1, 2, 4, 8, 16, 32, 64
MA_PARKING = 128
MA_OTHERS_STATE = 256

F_ARRIVE, F_OUT_OF_ROAD, F_CRASH_VEHICLE, F_CRASH_OBJECT, F_CRASH_BUILDING, F_MAX_STEP = 1, 2, 4, 8, 16, 32
F_ON_YELLOW, F_ON_WHITE, F_ON_BROKEN, F_CRASH_SIDEWALK, F_OFF_LANE, F_OUT_OF_ROUTE = 256, 512, 1024, 2048, 4096, 8192
F_OBJECT_HIT = 1 << 14
F_RESET, F_REPORT, F_NEW, F_ALL_DONE = 1 << 16, 1 << 17, 1 << 18, 1 << 19
