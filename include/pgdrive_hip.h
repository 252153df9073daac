/*
 * pgdrive_hip.h — C ABI of the MI355X-native batched PGDrive step engine.
 *
 * The reference (decisionforce/pgdrive v0.1.4) has no FFI/plugin layer for env.step(); its boundary is the Python
 * gym.Env surface (pgdrive/envs/base_env.py:184-193 step, :269-290 reset, :403-425 spaces).  This header re-states that
 * surface batched over N environments x V vehicle slots behind plain C entry points (no torch / C++ types), so a Python
 * VecEnv (pgdrive_amd/vec_env.py, ctypes) or any other host can bind it.  Each entry point cites what it replaces.
 *
 * Conventions: int status codes (0 = PGD_OK); the caller owns every buffer; pointers named d_* are DEVICE pointers,
 * h_* are HOST pointers; all work is enqueued on the hipStream_t given at creation (passed as void* so this header
 * needs no HIP include); no hidden global state; one handle may be driven by one host thread at a time.
 *
 * Geometry contract (all float32, PGDrive coordinates: x forward, y left->right as in the reference, angles in rad):
 *   pgd_lane  : StraightLane / CircularLane closed forms  (component/lane/straight_lane.py:13-67, circular_lane.py:11-67)
 *   pgd_road  : RoadNetwork.graph[from][to] -> lanes     (component/road/road_network.py:20)
 *   pgd_box   : every box the reference hands to Bullet   (component/blocks/base_block.py:286-464): lane-surface boxes
 *               (kind 0), white/yellow continuous and broken line ghosts (1,2,3), sidewalk bodies (4)
 *   uniform grid per map: cell -> ascending list of box ids (creation order == the reference's Bullet insertion order)
 */
#ifndef PGDRIVE_HIP_H
#define PGDRIVE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGD_OK 0
#define PGD_ERR_ARG 1
#define PGD_ERR_HIP 2
#define PGD_ERR_STATE 3

#define PGD_MAX_SUCC 8       /* successor lanes stored inline per lane */
#define PGD_MAX_CKPT 32      /* max nodes of a route (Navigation.checkpoints, navigation.py:131) */
#define PGD_NAVI_DIM 10      /* Navigation.navigation_info_dim (navigation.py:23) */
#define PGD_STATE_DIM 8      /* ego floats of StateObservation.vehicle_state at default config (state_obs.py:58-106) */

/* box kinds (constants.py:55-63 BodyName) */
#define PGD_BOX_LANE 0
#define PGD_BOX_WHITE 1
#define PGD_BOX_YELLOW 2
#define PGD_BOX_BROKEN 3
#define PGD_BOX_SIDEWALK 4

/* per-agent flag bits returned by pgd_step (constants.py:15-22 TerminationState + BaseVehicleState) */
#define PGD_F_ARRIVE        (1u << 0)   /* arrive_dest          base_vehicle.py:738-745 */
#define PGD_F_OUT_OF_ROAD   (1u << 1)   /* out_of_road          pgdrive_env.py:209-216 */
#define PGD_F_CRASH_VEHICLE (1u << 2)   /* crash_vehicle        collision_callback.py:7-36 */
#define PGD_F_CRASH_OBJECT  (1u << 3)   /* crash_object: first contact with a traffic object (collision_callback.py:27-32) */
#define PGD_F_CRASH_BUILDING (1u << 4)  /* crash_building (InvisibleWall/TollGate: always 0 on PG maps) */
#define PGD_F_MAX_STEP      (1u << 5)   /* max_step / horizon   base_env.py:190-192 */
#define PGD_F_ON_YELLOW     (1u << 8)   /* on_yellow_continuous_line  base_vehicle.py:615-636 */
#define PGD_F_ON_WHITE      (1u << 9)   /* on_white_continuous_line */
#define PGD_F_ON_BROKEN     (1u << 10)  /* on_broken_line */
#define PGD_F_CRASH_SIDEWALK (1u << 11) /* crash_sidewalk        base_vehicle.py:638-643 */
#define PGD_F_OFF_LANE      (1u << 12)  /* not on_lane           navigation.py:158-160 */
#define PGD_F_OUT_OF_ROUTE  (1u << 13)  /* out_of_route          base_vehicle.py:274-276 */
#define PGD_F_OBJECT_HIT    (1u << 14)  /* state bit of a traffic OBJECT's own slot: TrafficObject.crashed (COST_ONCE,
                                           collision_callback.py:28-32); never reported for agents */
#define PGD_F_RESET         (1u << 16)  /* this env was auto-reset at the end of the step (obs is the new episode's) */
#define PGD_F_REPORT        (1u << 17)  /* multi-agent: the slot held an active agent this step: obs/reward/done are valid */
#define PGD_F_NEW           (1u << 18)  /* multi-agent: an agent was (re)spawned into this slot: obs valid, reward 0 */
#define PGD_F_ALL_DONE      (1u << 19)  /* multi-agent: done["__all__"] (multi_agent_pgdrive.py:142-148) */

typedef struct __attribute__((aligned(16))) pgd_lane {   /* 64 B */
  float ax, ay;             /* straight: start point; circular: centre */
  float bx, by;             /* straight: unit direction; circular: (radius, start_phase) */
  float c;                  /* straight: heading; circular: end_phase */
  float dir;                /* 0 = straight; +1/-1 = CircularLane.direction */
  float length, width;
  float ex, ey;             /* lane end point = position(length, 0) */
  int16_t road;             /* map-local road id */
  int16_t index;            /* lane index inside its road (0 = left-most) */
  int16_t n_succ;
  int16_t pad;
  int16_t succ[PGD_MAX_SUCC]; /* map-local lane ids L2 with |end - L2.start| < 0.1 (abs_lane.py:114-119) */
} pgd_lane;

typedef struct __attribute__((aligned(16))) pgd_road {   /* 16 B */
  int16_t from, to;         /* node ids */
  int16_t first_lane, n_lanes;
  uint8_t negative;         /* Road.is_negative_road (road.py:33-34) */
  uint8_t block_id;         /* Road.block_ID char (road.py:46-51) */
  uint8_t valid;            /* 0 for the decoration road */
  uint8_t pad0;
  int32_t pad1;
} pgd_road;

typedef struct __attribute__((aligned(16))) pgd_box {    /* 32 B */
  float cx, cy;             /* centre */
  float ux, uy;             /* unit vector of the long axis */
  float hl, hw;             /* half extents along / across */
  int32_t kind;             /* PGD_BOX_* */
  int32_t lane;             /* map-local lane id for PGD_BOX_LANE, else -1 */
} pgd_box;

typedef struct pgd_map {    /* per-map header; offsets index the bank-wide arrays */
  int32_t lane_off, n_lanes;
  int32_t road_off, n_roads;
  int32_t box_off, n_boxes;
  int32_t cell_off;         /* into cell_start[] (gx*gy+1 entries for this map) */
  int32_t item_off;         /* into cell_items[] */
  int32_t gx, gy;
  float ox, oy, cell;       /* grid origin and cell size [m] */
  float lane_width;         /* map config lane_width (Navigation.get_current_lane_width, navigation.py:322-323) */
  int32_t pad[2];
} pgd_map;

/* One vehicle slot of a scenario (spawn state + static parameters).  Slots [0,A) are controlled agents, the rest are
 * IDM traffic (manager/traffic_manager.py:239-290).  A slot with lane < 0 is unused. */
typedef struct pgd_spawn {  /* 64 B + route */
  float x, y, heading;      /* spawn pose: lane.position(long, lat), lane.heading_at(long)  (base_vehicle.py:304-309) */
  float length, width;      /* vehicle_type.py:7-74 */
  float wheelbase;          /* FRONT_WHEELBASE + REAR_WHEELBASE */
  float mass;
  float max_engine_force, max_brake_force, friction; /* utils/space.py:219-255 */
  float max_steer;          /* [rad] */
  float max_speed;          /* [km/h] */
  int16_t lane;             /* spawn lane (map-local); <0 = empty slot */
  int16_t group;            /* trigger group (block order); -1 = active from the start (agents) */
  int16_t n_ckpt;           /* route length in nodes */
  int16_t timer0;           /* IDMPolicy.overtake_timer initial value (idm_policy.py:185) */
  int16_t dest_lane;        /* Navigation.final_lane (navigation.py:138-140) */
  int16_t kind;             /* PGD_OBJ_*: what occupies the slot */
  int16_t aux;              /* PGD_MA_PARKING: 1 + index of the parking space this vehicle drives to (0 = none) */
  int16_t pad;
  int16_t ckpt[PGD_MAX_CKPT];       /* route as node ids (Navigation.checkpoints) */
  int16_t ckpt_road[PGD_MAX_CKPT];  /* road id of (ckpt[k], ckpt[k+1]); -1 past the end */
} pgd_spawn;

/* pgd_spawn.kind.  Traffic objects (manager/object_manager.py, static_object/traffic_object.py) and broken-down vehicles
 * occupy traffic slots with group = PGD_GROUP_NEVER: present in the world (contacts, lidar, IDM neighbour search), never
 * driven.  Deliberate substitution: Bullet lets a hit cone fly away; here objects are static. */
#define PGD_OBJ_VEHICLE  0  /* chassis box length x width */
#define PGD_OBJ_CYLINDER 1  /* TrafficCone / TrafficWarning: circle of radius length / 2 (traffic_object.py:40,60) */
#define PGD_OBJ_BOX      2  /* TrafficBarrier: box length x width at `heading` (traffic_object.py:80-96) */
#define PGD_OBJ_BUILDING 3  /* TollGateBuilding: invisible wall length x width (tollgate_building.py, scene_utils.py:260-295);
                               a contact is crash_building (collision_callback.py:33-35), every step */
#define PGD_GROUP_NEVER (-2)

typedef struct pgd_scenario {
  int32_t map;              /* index into the map table */
  int32_t n_groups;         /* number of traffic trigger groups */
  int16_t trigger_road[16]; /* BlockVehicles.trigger_road per group, in activation order (traffic_manager.py:283-288) */
  int32_t max_steps;        /* auto_termination: 250 * map.num_blocks (base_env.py:318); 0 = off */
  int32_t aux;              /* PGD_MA_PARKING: bit k = parking space k is nobody's destination at reset */
} pgd_scenario;

typedef struct pgd_config {
  int32_t num_envs;         /* N */
  int32_t num_agents;       /* A  controlled agents per env (1 = PGDriveEnv; >1 = MARL) */
  int32_t num_traffic;      /* T  IDM traffic slots per env; V = A + T */
  int32_t num_lasers;       /* lidar beams (pgdrive_env.py:63; 0 disables the lidar block of the obs) */
  int32_t num_others;       /* neighbour-info vehicles (lidar.num_others, 4) */
  float lidar_dist;         /* 50 m */
  float dt;                 /* physics_world_step_size 0.02 (base_env.py:70) */
  int32_t decision_repeat;  /* 5 (base_env.py:33) */
  int32_t auto_reset;       /* 1: envs whose agent is done are reset inside pgd_step */
  int32_t resample_scenario;/* 1: on auto-reset draw a new scenario (base_env.py:451-458), else keep env's scenario */
  int32_t horizon;          /* 0 = none (base_env.py:190-192) */
  uint32_t seed;            /* seed of the device-side counter RNG used for scenario resampling */
  /* reward scheme (pgdrive_env.py:91-101) */
  float success_reward, out_of_road_penalty, crash_vehicle_penalty, crash_object_penalty;
  float driving_reward, speed_reward;
  int32_t use_lateral;
  int32_t out_of_route_done;
  /* multi-agent (envs/marl_envs/multi_agent_pgdrive.py:12-55); all zero for the single-agent PGDriveEnv */
  int32_t marl_flags;       /* PGD_MA_* bits */
  int32_t delay_done;       /* steps a finished agent stays as a static obstacle (25) */
  int32_t agent_limit;      /* num_agents of the reference: respawn only while active + dying < agent_limit */
  int32_t respawn_places;   /* P safe spawn places (SpawnManager.safe_spawn_places, spawn_manager.py:114-155) */
  int32_t respawn_dests;    /* Dn destinations; every scenario carries P*Dn extra pgd_spawn records after its V slots */
  /* SideDetector / LaneLineDetector ray fans against lane-line boxes (vehicle_module/distance_detector.py:137-152);
   * 0 lasers (the reference default, pgdrive_env.py:64-65) keeps the two lateral-distance floats of state_obs.py:66-71 */
  int32_t side_lasers;      /* k: rays vs continuous (white / yellow / side) line boxes; replace obs[0:2] when > 0 */
  float side_dist;          /* 50 m */
  int32_t lane_line_lasers; /* m: rays vs continuous + broken line boxes; inserted after the yaw-rate float when > 0 */
  float lane_line_dist;     /* 20 m */
  /* action pre-processing of the controlled agents */
  int32_t discrete_action;  /* 1: EnvInputPolicy.convert_to_continuous_action (env_input_policy.py:28-31), applied AFTER the
                               clip to [-1,1] exactly as the reference does */
  int32_t discrete_steering_dim, discrete_throttle_dim; /* 5, 5 (base_env.py:35-36) */
  int32_t increment_steering; /* 1: steering += a0 * 0.05, clipped (base_vehicle.py:351-358) */
  int32_t safe_rl_env;      /* 1: SafePGDriveEnv.done_function (safe_pgdrive_env.py:49-56): a step with crash_vehicle, else
                               crash_object, is never terminal */
  /* MultiAgentTollgateEnv (envs/marl_envs/marl_tollgate.py), read when PGD_MA_TOLLGATE is set */
  float overspeed_penalty;  /* 0.5: reward = -penalty * speed / max_speed while too fast inside the toll block */
  int32_t min_pass_steps;   /* 30: an agent that crossed the toll block in fewer steps is terminated (out_of_road) */
  int32_t enable_reverse;   /* vehicle_config.enable_reverse (base_vehicle.py:366-376) for the controlled agents: negative
                               throttle drives backwards instead of braking (parking-lot env) */
  /* LidarStateObservation._add_noise_to_cloud_points (state_obs.py:172-182): beams <- clip(beam + N(0, sigma), 0, 1), then
   * 0 with probability dropout.  The reference draws from the global numpy RNG; here a counter-based stream of
   * (seed, env, agent, beam, step) -- same distribution, reproducible */
  float lidar_gaussian_noise, lidar_dropout_prob;
  int32_t random_agent_model; /* 1: two more state floats, LENGTH / 10 and WIDTH / 2.5, after the lane-line fan
                               (state_obs.py:21-22,102-105); the vehicle type itself comes with the spawn record */
  int32_t env_base;         /* global index of this engine's env 0.  The device RNG streams (IDM timers, lidar noise, scenario
                               re-draws, respawn destinations) are keyed by env_base + e, so envs sharded over several engines
                               / GPUs reproduce the single-engine run env for env */
  int32_t idm_agent;        /* IDM_agent (base_env.py:30, agent_manager.py:79): the ego is driven by IDMPolicy along its route,
                               the actions handed to pgd_step are ignored.  Single-agent engines only */
  float idm_steer_lag;      /* NOT in the reference; 0 (the default) = the reference's behaviour.  > 0: time constant [s] of a
                               first-order lag between the steering IDMPolicy commands (idm_policy.py:244-252) and the steering an
                               IDM-driven vehicle applies: steer += (clip(cmd) - steer) * T / (lag + T), T = dt * decision_repeat.
                               The reference's heading PID (kp 1.7, kd 3.5 per 0.1 s decision) was tuned on Bullet's raycast
                               vehicle; on the kinematic bicycle (no yaw inertia) the same gains end in a two-step limit cycle,
                               steering lock to lock (tests/test_traffic_band_gpu.py).  The lag stands in for the yaw dynamics the
                               bicycle lacks: an OPT-IN for users who train against traffic; unpinned like the bicycle itself.
                               Controlled agents are never lagged.  0.2 s settles the traffic on its lane axis */
} pgd_config;

#define PGD_MA_ENABLED        1  /* MultiAgentPGDrive semantics: per-agent done, delay-done queue, respawn, __all__ */
#define PGD_MA_CRASH_DONE     2  /* crash_done       (multi_agent_pgdrive.py:21) */
#define PGD_MA_OUT_ROAD_DONE  4  /* out_of_road_done (multi_agent_pgdrive.py:22) */
#define PGD_MA_ALLOW_RESPAWN  8  /* allow_respawn    (multi_agent_pgdrive.py:26) */
#define PGD_MA_PLAIN_REWARD  16  /* MultiAgentBottleneckEnv.reward_function (marl_bottleneck.py:91-128): no -1 factor on a
                                    negative road when the vehicle is off its reference lanes */
#define PGD_MA_TOLLGATE      64  /* MultiAgentTollgateEnv: toll reward / out-of-road / stay-time rules, observation without the
                                    navigation block plus 2 toll floats (marl_tollgate.py:63-105,195-270) */
#define PGD_MA_PARKING      128  /* MultiAgentParkingLotEnv (marl_parking_lot.py:39-90,160-222): destinations of agents entering
                                    from a road are parking spaces handed out from a per-env pool (released when the agent
                                    is done); a road place is respawned into only while a space is free; out-of-road =
                                    yellow line / off lane / sidewalk (white lines may be crossed) */
#define PGD_MA_YELLOW_OK     32  /* cross_yellow_line_done = False (marl_bottleneck.py:130-136): a yellow line is not
                                    out-of-road */
#define PGD_MA_OTHERS_STATE 256  /* LidarStateObservationMARound.observe (marl_inout_roundabout.py:82-105): each of the
                                    num_others neighbour rows is the neighbour's own StateObservation vector (as long as
                                    the observing agent's state block, zeros when absent) instead of 4 relative floats */

typedef struct pgd_engine* pgd_handle;

/* Size of one observation row D = (side_lasers or 2) + 6 + lane_line_lasers [+ 2 if random_agent_model] + 10 + 4*num_others + num_lasers
 * (obs/state_obs.py:17-23,108-114,124-130); 274 at the defaults.  With PGD_MA_TOLLGATE the 10 navigation floats are
 * absent and 2 toll floats follow the lidar (marl_tollgate.py:63-105). */
int pgd_obs_dim(const pgd_config* cfg);

/* Replaces PGDriveEnv.__init__ / lazy_init (envs/base_env.py:100-178): allocates device state for N x V slots.
 * The call also reads the library's environment switches (A/B runs and debugging, never needed in production), once, into the handle;
 * a later change of the environment does not reach an existing engine.  Set = present with any value, unless stated otherwise:
 *   PGD_NO_FUSE            the stand-alone observation kernels run after k_step instead of the fused paths
 *   PGD_NO_FIX             never launch an instantiation specialised for one configuration (nor a run-time kernel)
 *   PGD_JIT_FORCE          a run-time kernel (pgd_set_step_module) also takes the place of a specialised instantiation
 *   PGD_ROW_OBSERVE        multi-agent observation by one block per row (k_observe) instead of one block per env (k_observe_env)
 *   PGD_NO_STATE_IN_STEP   many agent seats: the rows' state blocks stay in k_observe_env instead of being written by k_step
 *   PGD_PACK=0 / 1         throughput mode (several whole envs per wave) off / on, whatever the env count (default: from 32768 envs on)
 *   PGD_NO_ROWZ            multi-agent engines keep no zero-row marks (pgd_step); a value that starts with '0' counts as not set
 *   PGD_NO_IMASK / PGD_IMASK   never-written slots are never / always read from the scenario's reset image (default: in throughput mode)
 *   PGD_NO_UNI             an upload never records one body size for all vehicles (read here, not by pgd_upload_scenarios: Engine()
 *                          creates and uploads inside one constructor, and nothing sets the variable in between) */
int pgd_create(const pgd_config* cfg, int device, void* hip_stream, pgd_handle* out);

/* Replaces MapManager.update_map + block._create_in_world (manager/map_manager.py:98-155, blocks/base_block.py:142-179):
 * uploads immutable geometry for a bank of maps.  All pointers are HOST arrays; they are copied. */
int pgd_upload_maps(pgd_handle h, const pgd_map* h_maps, int n_maps, const pgd_lane* h_lanes, int n_lanes,
                    const pgd_road* h_roads, int n_roads, const pgd_box* h_boxes, int n_boxes,
                    const int32_t* h_cell_start, int n_cell_start, const int32_t* h_cell_items, int n_cell_items);

/* Replaces AgentManager.reset + TrafficManager.reset spawn tables (manager/agent_manager.py:91-132,
 * traffic_manager.py:48-69,239-290): a bank of scenarios, each with V spawn slots.  HOST arrays, copied. */
int pgd_upload_scenarios(pgd_handle h, const pgd_scenario* h_scen, int n_scen, const pgd_spawn* h_spawns /*[n_scen*V]*/);

/* Replaces env.reset(force_seed) (envs/base_env.py:269-301) for the listed envs (h_env_ids == NULL -> envs 0 .. n - 1):
 * env h_env_ids[i] starts scenario h_scen_ids[i].  1 <= n <= N; an id outside [0, N), an id listed twice or a scenario that was not
 * uploaded is PGD_ERR_ARG and leaves the engine as it was.  Both HOST lists are copied before the call returns; the call is
 * asynchronous on the stream.  d_obs may be NULL.  Which rows of d_obs are written:
 *   h_env_ids == NULL   every row of every env (those of envs n .. N - 1 from their present state);
 *   an id list          the rows of the listed envs and no others.  Every other row keeps its bytes -- the terminal rows the last
 *                       step wrote for envs that are not restarted are still there --, and the zero-row marks of the other envs
 *                       (pgd_step) go on describing the buffer they were made for.
 * The restart does not count as an episode of EI_EPISODES and does not touch EI_STEPS_TOTAL (counters of the device RNG streams). */
int pgd_reset(pgd_handle h, const int32_t* h_env_ids, const int32_t* h_scen_ids, int n, float* d_obs /*[N,A,D]*/);

/* Replaces env.step(action) (envs/base_env.py:184-224, 303-344) for all N envs.  Asynchronous on the stream.
 * Multi-agent engines: the row of a slot that is not due in this step (no agent, or an agent that did not report) reads zero.  The
 * engine writes such a row once and remembers that it did -- per env, together with the identity of the buffer (address and row
 * stride) the marks describe; the kernel compares that identity itself, so eager calls with alternating buffers, HIP-graph replays
 * and env groups on their own streams all see marks that belong to the buffer they write (the same rule for pgd_reset /
 * pgd_observe / pgd_step_packed).  A caller that scribbles over rows it was handed (in-place normalisation, noise) must not expect
 * them to be zeroed again while it keeps passing the same buffer: copy first, pass another buffer, or create the engine with
 * PGD_NO_ROWZ=1 in the environment (every row that is not due is then zero-filled by every call).
 * d_actions must be 8-byte aligned: the kernel reads an agent's (steering, throttle) pair with one 8-byte load.  The same holds for
 * the action pointer of pgd_step_packed and pgd_step_group and for d_action_ring of pgd_step_n (its slices are N*A*8 bytes apart, so
 * the base decides); a pointer that is not is PGD_ERR_ARG before anything is launched, and the engine is as it was.
 * pgd_step_lane_keep takes no action pointer: its actions come from the row (which it reads in place only where the row buffer is
 * 8-byte aligned) or from a buffer of the engine's own. */
int pgd_step(pgd_handle h, const float* d_actions /*[N,A,2]*/, float* d_obs /*[N,A,D]*/, float* d_reward /*[N,A]*/,
             uint8_t* d_done /*[N,A]*/, uint32_t* d_flags /*[N,A]*/);

/* K steps of an action ring in one call (open-loop use: action repeat / frame skip, scripted roll-outs, benchmarks): step k
 * (k = 0 .. n_steps - 1) applies d_action_ring[(first + k) % ring_len] ([ring_len][N,A,2]) exactly as pgd_step would -- auto-reset
 * included -- and writes its reward / done / flags into slice k of d_reward / d_done / d_flags ([n_steps][N,A]).  The
 * observation (d_obs, may be NULL) is evaluated ONCE, for the state after the last step: the intermediate steps run without
 * the observation part of the kernel.  n_steps launches on the stream, no host synchronisation in between; the closed loop
 * policy -> action -> step needs pgd_step (the reference's env.step has no counterpart of this call; its decision_repeat is
 * the five physics sub-steps inside every step). */
int pgd_step_n(pgd_handle h, const float* d_action_ring, int ring_len, int first, int n_steps, float* d_obs /*[N,A,D]*/,
               float* d_reward /*[n_steps][N,A]*/, uint8_t* d_done /*[n_steps][N,A]*/, uint32_t* d_flags /*[n_steps][N,A]*/);

/* The same step with the env's results written as ONE packed fp32 row per env, the unit of the per-step gather that
 * BASELINE.json's north star names (envs shard across GPUs, one gather of (obs, reward, done) per step):
 *   d_rows[e * row_stride + ...] = [A*D observation floats | A rewards | A done flags as 0.0 / 1.0], row_stride >= A*(D+2).
 * The kernel writes the row itself -- d_rows is typically this rank's slice of the gather's receive buffer, so no copy
 * kernel packs anything.  d_reward / d_done / d_flags are written as by pgd_step (rank-local bookkeeping).
 * Multi-agent engines keep the zero-row marks of pgd_step for d_rows as well, keyed by (d_rows, row_stride): a row that is not due
 * is zeroed once and left alone while the same buffer keeps coming.  The key is an address, not an allocation: a caller that hands
 * in NEW memory which may sit where a freed buffer sat with the same row stride (a caching allocator; a receive buffer allocated
 * per step) calls pgd_forget_rows first, or keeps every buffer it has passed alive for as long as it steps.  pgdrive_amd's
 * Engine.step_packed does the former for every tensor it has not seen alive, as Engine.step does for `out`. */
int pgd_step_packed(pgd_handle h, const float* d_actions, float* d_rows /*[N,row_stride]*/, int row_stride,
                    float* d_reward /*[N,A]*/, uint8_t* d_done /*[N,A]*/, uint32_t* d_flags /*[N,A]*/);

/* Asynchronous env groups (double-buffered sampling: the policy of group A runs while group B steps).  The reference runs
 * one env per process and lets the RL library interleave processes; here one handle is split into n_groups equal, contiguous
 * groups of envs, each with an internal stream.  pgd_step_group steps ONLY the envs of `group` on that group's stream --
 * consecutive steps of different groups overlap on the GPU (a launch ends with its slowest wave; another group's step fills
 * that tail).  All pointers address the FULL [N, ...] arrays; only the group's rows are read / written.  pgd_group_stream
 * hands out the stream so that the caller can order its own kernels (the policy) with the group's steps; work submitted
 * through pgd_step / pgd_reset (engine stream) is NOT ordered against the group streams: synchronise when switching.
 * An engine in throughput mode (>= 32768 envs: three whole envs per wave) whose group size is not a whole number of such waves is
 * switched back to one env per wave FOR THE REST OF ITS LIFE (same results, 6 - 18 % slower at that size); the switch happens only
 * when the call succeeds (PGD_ERR_ARG leaves the engine unchanged) and pgd_describe_step reports it from then on. */
int pgd_set_groups(pgd_handle h, int n_groups);   /* N % n_groups == 0; 1 = back to a single group */
int pgd_step_group(pgd_handle h, int group, const float* d_actions /*[N,A,2]*/, float* d_obs /*[N,A,D]*/, float* d_reward,
                   uint8_t* d_done, uint32_t* d_flags);
int pgd_group_stream(pgd_handle h, int group, void** hip_stream);
int pgd_group_sync(pgd_handle h, int group);

/* Scripted lane-keeping policy for the controlled agent of a single-agent engine -- what the reference's examples use their
 * trained PPO expert for (examples/ppo_expert, tests/test_functionality/test_expert_performance.py): an action stream that
 * keeps the ego DRIVING, for benchmarks and soak runs.  One launch on the engine stream; reads the rows pgd_step wrote
 * (default state layout, side_lasers == 0: [0] [1] distances to the left / right road edge, [2] heading alignment, [3] speed):
 *   steering = clip(k_lat * 18 * (o[0] - o[1]) / 10 + k_head * (2 o[2] - 1) + noise * n1, -1, 1)
 *   throttle = clip(0.3 * (v_target_kmh - v_kmh) + noise * n2, -1, 1)      n1, n2 ~ U(-1, 1) from the counter RNG (seed, env, tick)
 * d_actions [N, 1, 2] is then handed to pgd_step.  Not part of the reference's env.step: a convenience of this library. */
/* The same policy evaluated by the step itself: pgd_step_lane_keep = pgd_lane_keep_actions on the rows in d_obs (what the previous
 * pgd_step / pgd_reset / pgd_step_lane_keep wrote there) followed by pgd_step with those actions, d_obs rewritten -- as ONE launch on
 * engines with one env per wave (the step kernel reads the four floats where it would read the caller's action; the same arithmetic,
 * the same bits), as the two launches otherwise.  Closed-loop driving without a second launch per step (the policy kernel alone
 * was a fifth of an iteration: its launch floor). */
int pgd_step_lane_keep(pgd_handle h, float k_lat, float k_head, float v_target_kmh, float noise, uint32_t tick, float* d_obs /*[N,1,D]*/,
                       float* d_reward, uint8_t* d_done, uint32_t* d_flags);
int pgd_lane_keep_actions(pgd_handle h, const float* d_obs /*[N,1,D]*/, float* d_actions /*[N,1,2]*/, float k_lat, float k_head,
                          float v_target_kmh, float noise, uint32_t tick);

/* Which step kernel the last pgd_step / pgd_step_packed / pgd_step_group call of this engine launched, as text ("" before the
 * first step): one env per wave, several envs per wave, throughput mode, two waves per env, and whether it is the instantiation
 * specialised for the reference's default single-agent configuration.  For benchmark lines and tests; no reference counterpart. */
int pgd_describe_step(pgd_handle h, char* buf, int cap);

/* Checkpoint / resume (BaseVehicle.get_state/set_state, base_vehicle.py:683-698): raw SoA state blobs.
 * Layout: nf float fields then ni int fields, each [N*V]; query sizes with pgd_state_dims. HOST buffers. */
int pgd_state_dims(pgd_handle h, int* n_float_fields, int* n_int_fields, int* n_env_int_fields);
int pgd_get_state(pgd_handle h, float* h_f, int32_t* h_i, int32_t* h_env_i);
int pgd_set_state(pgd_handle h, const float* h_f, const int32_t* h_i, const int32_t* h_env_i);
/* Recompute localisation + observation from the current state without stepping (engine.after_step + observe,
 * base_env.py:295-301). */
int pgd_observe(pgd_handle h, float* d_obs);

/* Timing helper: HIP-event time [ms] of the last pgd_step on the engine stream.  Off by default (two event packets per
 * step leave idle gaps between back-to-back launches); switch it on with pgd_enable_step_timing(h, 1). */
int pgd_enable_step_timing(pgd_handle h, int on);
int pgd_last_step_ms(pgd_handle h, float* ms);

/* Per-kernel HIP-event profile: between begin and end every pgd_step records events around its two kernels on the
 * engine stream (up to `capacity` steps); end synchronises and returns the average duration of each kernel. */
int pgd_profile_begin(pgd_handle h, int capacity);
/* Strided variant for bench.py.  When pgd_step is a single kernel (observation fused) the two events bracket GROUPS of
 * `stride` consecutive launches and pgd_profile_end reports group time / stride, i.e. the average launch duration with
 * the launches left back to back; `count` is then the number of complete groups.  Otherwise every stride-th step is
 * bracketed on its own. */
int pgd_profile_begin_strided(pgd_handle h, int capacity, int stride);
int pgd_profile_end(pgd_handle h, float* k_step_ms, float* k_observe_ms, int* count);

/* Move the engine to another HIP stream (e.g. the caller's current framework stream, so that a step is ordered like any
 * other op of that stream and needs no events).  Work already enqueued on the previous stream is ordered before anything
 * enqueued on the new one.  The engine never owns `hip_stream`; NULL is the device's default stream. */
int pgd_set_stream(pgd_handle h, void* hip_stream);
int pgd_sync(pgd_handle h);
int pgd_destroy(pgd_handle h);
const char* pgd_version(void);
/* The same network with SPLIT bf16 operands on the bf16 matrix cores (every f32 value = hi + lo, two bf16; a product = three matrix
 * instructions; f32 accumulation): 1/5 of the exact form's matrix time, ~3e-5 of error on an action in [-1, 1] instead of ~1e-6.  The
 * weights are prepared ONCE per policy update into a device buffer of pgd_mlp_prepared_bytes(in_dim) bytes (16-byte aligned):
 * pgd_mlp_prepare splits them and lays them out in the kernel's fragment order (asynchronous on the engine's stream);
 * pgd_mlp_policy_prepared then evaluates the network like pgd_mlp_policy (same rows, groups, action layout). */
size_t pgd_mlp_prepared_bytes(int in_dim);
int pgd_mlp_prepare(pgd_handle h, int in_dim, int hidden, const float* d_w1, const float* d_b1, const float* d_w2, const float* d_b2,
                    const float* d_w3, const float* d_b3, int out_cols, void* d_prepared);
int pgd_mlp_policy_prepared(pgd_handle h, int group, const float* d_obs, int obs_stride, int in_dim, const void* d_prepared, int final_tanh,
                            float* d_actions);
/* Run-time specialisation of the step kernel (no reference counterpart).  The library ships instantiations of k_step with the
 * configurations of the reference's env classes compiled in; any OTHER configuration runs the general kernel, 12 - 17 % behind.
 * pgdrive_amd/jit.py builds, with the same hipcc and flags as the library, a code object that holds k_step with THIS handle's
 * configuration and geometry as literals (every pgd_config field; pgd_step_geometry reports the derived values:
 * N, A, T, V, D, NV, epw, sub, pack_obs, sstride, use_imask, flags: bit 0 objects among the bodies, bit 1 default row layout, bit 2
 * the engine can take such a kernel -- single-agent, one env per wave, scenarios uploaded), and pgd_set_step_module loads it:
 * pgd_step then launches it wherever it would have launched a general kernel, while the engine's geometry and object flag are what
 * the module was built for (pgd_set_groups, a scenario upload that adds objects: back to the library's kernels).  Null path: unload.
 * Results are those of the general kernel to rounding (constant folding re-orders a few fp32 operations), flags and integer state
 * bit-identical: tests/test_parity_gpu.py::test_run_time_kernel_matches_the_general_kernel. */
int pgd_step_geometry(pgd_handle h, int32_t* out12);
int pgd_set_step_module(pgd_handle h, const char* code_object_path, int built_with_objects, int built_with_std_rows);
/* The policy network of a closed loop in one launch: actions[r][0..1] = MLP(obs row r) for every (env, agent) row of the engine
 * (group < 0: all rows, on the engine's stream; group >= 0: the rows of that env group on the group's stream, the twin of
 * pgd_step_group).  Replaces pgdrive/examples/ppo_expert/numpy_expert.py:25-44 (`expert(obs)`: x = tanh(obs @ fc_1 + b);
 * x = tanh(x @ fc_2 + b); out = x @ fc_out + b, the action = the first two outputs) evaluated row by row in numpy, and the
 * policy(obs) call of any rollout loop whose policy is such a network.  Weights: fp32 device arrays, row-major [in][out] as the
 * reference's `kernel` arrays (w1 [in_dim][hidden], w2 [hidden][hidden], w3 [hidden][out_cols]; only columns 0 and 1 of w3 / b3 are
 * used); hidden must be 256; w1, w2, b1, b2 16-byte aligned.  in_dim: 4 .. 448 -- the 16 rows of a workgroup and both hidden activations
 * stay in LDS, and 449 inputs would need more than its 64 KB (PGD_ERR_ARG; the same limit holds for pgd_mlp_policy_prepared, while
 * pgd_mlp_prepare itself takes up to 4096).  d_obs: rows of obs_stride floats, the first in_dim are the network's input (normally the buffer and
 * row width pgd_step writes).  final_tanh != 0 squashes the two outputs (numpy_expert.py does not; the env clips).
 * d_actions: [rows][2] floats, the layout pgd_step reads.  Asynchronous; may be captured in a HIP graph with the step.
 * Arithmetic: fp32 throughout (the 256-wide layers on the f32 matrix cores: a k-ordered fma chain). */
int pgd_mlp_policy(pgd_handle h, int group, const float* d_obs, int obs_stride, int in_dim, int hidden, const float* d_w1,
                   const float* d_b1, const float* d_w2, const float* d_b2, const float* d_w3, const float* d_b3, int out_cols,
                   int final_tanh, float* d_actions);
/* Actor and critic of a PPO rollout in one launch: a sampled action, its log-probability and the value estimate for every (env,
 * agent) row of the engine (rows and `group` as for pgd_mlp_policy).  Replaces pgdrive/examples/ppo_expert/numpy_expert.py:38-45
 * (`expert(obs, deterministic=False)`: mean, log_std = split(fc_out's four outputs); action = normal(mean, exp(log_std))) and
 * numpy_expert.py:62-78 (`value(obs)`: fc_value_1, fc_value_2, value_out -- a second network of the same shape with one output), plus
 * the log-probability a trainer computes from both.  Layout: as pgd_mlp_policy -- fp32 device arrays, row-major [in][out]; hidden is 256;
 * w1, b1, w2, b2 of each network 16-byte aligned; in_dim 4 .. 416 (the head's four weight rows take 2 KB more of the workgroup's 64 KB
 * of LDS than pgd_mlp_policy's two: PGD_ERR_ARG above); obs_stride >= in_dim; out_cols >= 4 (columns at or beyond 4 are never read).
 * The value network's six pointers are all set or all null; null: no critic, d_value is not touched (and may be null).
 * Arithmetic (fp32; the 256-wide layers on the f32 matrix cores, as pgd_mlp_policy), per row with g = (env_base + env) * A + agent:
 *   r1 = rng(seed ^ 0xac7012c1, g, 0x5a3b1e0d, tick), r2 = rng(seed ^ 0xac7012c1, g, 0x5a3b1e0d, tick ^ 0x80000000)   (the counter hash)
 *   u = ((r >> 9) + 0.5) * 2^-23 (exact in fp32, never 0 or 1);  R = sqrt(-2 log u1), z0 = R cos(2 pi u2), z1 = R sin(2 pi u2)
 *   action[i] = mean[i] + exp(log_std[i]) z[i]   -- unclipped, [rows][2], the buffer pgd_step reads and clips (numpy_expert.py:44)
 *   logp = -0.5 (z0^2 + z1^2) - log_std0 - log_std1 - log(2 pi);   value = the critic's output
 * PGD_AC_DETERMINISTIC: z = 0 (the action is the mean, logp the density at the mean).  `seed` is the caller's, not the engine's.
 * Asynchronous on the engine's stream (group >= 0: the group's); may be captured in a HIP graph.  A captured launch replays with the
 * `tick` it was captured with: pgd_actor_critic_tick gives the engine a uint32 counter in DEVICE memory that every later launch adds to
 * its `tick` argument (modulo 2^32; read by the kernel when it runs), so that a replayed rollout draws new noise once the caller has
 * advanced the counter on the same stream; null (the default): the argument alone. */
typedef struct pgd_actor_critic {      /* device pointers, fp32, row-major [in][out] as the reference's `kernel` arrays */
  const float *w1, *b1, *w2, *b2, *w3, *b3;  int32_t out_cols;   /* policy; out_cols >= 4: mean 0..1, log_std 2..3 */
  const float *vw1, *vb1, *vw2, *vb2, *vw3, *vb3;                /* value net, vw3 [256][1]; all six null = no critic */
} pgd_actor_critic;
#define PGD_AC_DETERMINISTIC 1u
int pgd_mlp_actor_critic(pgd_handle h, int group, const float* d_obs, int obs_stride, int in_dim, const pgd_actor_critic* nets,
                         uint32_t seed, uint32_t tick, uint32_t flags,
                         float* d_actions /*[rows][2]*/, float* d_logp /*[rows]*/, float* d_value /*[rows], may be null without critic*/);
int pgd_actor_critic_tick(pgd_handle h, const uint32_t* d_tick /* device memory, or null */);
/* Generalised advantage estimation behind a rollout of T steps (what RL libraries compute on the host from the arrays the reference's
 * env.step returned; no counterpart inside the reference).  Time-major device arrays: reward, done (the uint8 pgd_step writes), adv,
 * ret [T][rows]; value [T + 1][rows], row T the bootstrap.  One thread per row, t from T - 1 down to 0, fp32:
 *   nonterminal = 1 - done[t][r];  delta = reward[t][r] + gamma value[t+1][r] nonterminal - value[t][r]
 *   adv[t][r] = delta + gamma lam nonterminal adv[t+1][r]  (adv[T] = 0);   ret[t][r] = adv[t][r] + value[t][r]
 * A done ends the episode for GAE whatever ended it: no bootstrap through a horizon truncation (pgd_gae_bootstrap, below, has one).
 * T >= 1, rows >= 1 (PGD_ERR_ARG).
 * Asynchronous on the engine's stream; may be captured in a HIP graph. */
int pgd_gae(pgd_handle h, const float* d_reward, const float* d_value /*[T+1][rows]*/, const uint8_t* d_done, int T, int rows,
            float gamma, float lam, float* d_adv, float* d_ret);
/* ---- Rollouts of multi-agent engines: which seat rows count, the networks over those rows only, GAE per agent ----------------------
 * (No reference counterpart: the reference returns dicts keyed by agent name, multi_agent_pgdrive.py:109-213, and an RL library batches
 * the agents that are present.  Here a seat is a row of fixed arrays and the flags pgd_step wrote say what the row means.)
 * For seat row r = env * A + seat and step t, let f = flags[t][r] and d = done[t][r], as pgd_step wrote them:
 *   acted(t) = f & PGD_F_REPORT                        an agent held the seat and acted in step t: obs[t], action[t], logp[t], value[t],
 *                                                      reward[t], done[t] are its
 *   cont(t)  = acted(t) && !d && !(f & PGD_F_RESET)    the same agent holds the seat after the step: obs[t + 1] is its next observation
 *   live(t)  = (f & PGD_F_NEW) || cont(t)              row t + 1 of the seat holds an observation that an agent will act on
 * On the engine acted(t + 1) == live(t) (held by tests/test_marl_rollout_gpu.py, not assumed by the kernels).
 *
 * pgd_live_rows: the ascending list of the rows at which `live` holds -> d_rows, their number -> *d_count (device memory, int32).
 * Rows: all N x A of the engine (group < 0, the engine's stream) or those of env group `group` (the group's stream); the entries are
 * the engine's own row numbers env * A + seat in either case, so d_rows needs room for as many entries as the range has rows.  d_flags,
 * d_done: the FULL [N][A] arrays of a step.  Any engine is accepted (a single-agent engine never sets PGD_F_REPORT: its list is empty).
 * pgd_rollout_index: the same for the predicate `acted` over a time-major flag array [T][rows]: entries t * rows + r, ascending, into
 * d_index (room for T * rows entries; T * rows <= PGD_ROLLOUT_INDEX_MAX, PGD_ERR_ARG above), their number into *d_count.  What a trainer draws minibatches from.
 * Both: three small launches (per-block counts by ballot and popcount; one workgroup scans the block counts and writes the total; a
 * scatter) -- the order does not rest on atomics, no workgroup waits for another, the same input gives the same bytes, and entries at
 * and beyond the count are not written.  Asynchronous; capturable in a HIP graph.  The block counts are the engine's scratch:
 * pgd_live_rows' is allocated by pgd_create, with a segment for the whole-engine form and one for every env group, so the whole-engine
 * call and the groups' calls may be in flight together (two calls of the SAME form and group share a segment: order them on one stream);
 * pgd_rollout_index allocates on the first call and whenever T * rows exceeds every earlier call's, which a stream that is being
 * captured cannot do (PGD_ERR_STATE): call it once with the rollout's shape before the capture.  Scratch that was outgrown is kept
 * until pgd_destroy, so a graph captured with it can still be replayed; calls of pgd_rollout_index share the current scratch and
 * are ordered by the engine's stream. */
#define PGD_ROLLOUT_INDEX_MAX 2147482623 /* 2^31 - 1 - 1024: the last workgroup's block of 1024 indices stays below 2^31 */
int pgd_live_rows(pgd_handle h, int group, const uint32_t* d_flags, const uint8_t* d_done, int32_t* d_rows, int32_t* d_count);
int pgd_rollout_index(pgd_handle h, const uint32_t* d_flags /*[T][rows]*/, int T, int rows, int32_t* d_index, int32_t* d_count);
/* pgd_mlp_actor_critic over a row list: every argument of pgd_mlp_actor_critic, plus d_rows / d_count as pgd_live_rows wrote them (or
 * any ascending or unordered list of distinct rows of the range).  Tile j of 16 rows takes list entries 16 j .. 16 j + 15 and gathers
 * their observation rows; outputs go to the rows' own places in d_actions, d_logp, d_value; the noise is that of the TRUE row (g =
 * (env_base + env) * A + agent, same seed and tick rule, the device counter of pgd_actor_critic_tick included): a listed row gets bit for
 * bit what pgd_mlp_actor_critic gives it on the same inputs.  The host never reads *d_count: the grid covers every row of the range and
 * a workgroup whose tile starts at or beyond the count ends before it reads a weight.  An entry that is no row of the range is skipped.
 * Rows of the range that are NOT listed get action 0, 0, logp 0 and (with a critic) value 0, written by THIS call (a clearing launch
 * in front of the networks; pgd_live_rows writes the list only), so a seat that was live in the last rollout does not keep its old
 * numbers; their observations are never used (a NaN there reaches no output).  in_dim 4 .. 416, the refusals, PGD_AC_DETERMINISTIC and the null critic (d_value
 * untouched) as for pgd_mlp_actor_critic.  Two launches, asynchronous on the engine's stream (group >= 0: the group's); capturable. */
int pgd_mlp_actor_critic_rows(pgd_handle h, int group, const float* d_obs, int obs_stride, int in_dim, const pgd_actor_critic* nets,
                              uint32_t seed, uint32_t tick, uint32_t flags, const int32_t* d_rows, const int32_t* d_count,
                              float* d_actions /*[rows][2]*/, float* d_logp /*[rows]*/, float* d_value /*[rows], may be null without critic*/);
/* pgd_gae for seats that change hands.  Arrays as for pgd_gae, plus flags [T][rows] (the uint32 pgd_step writes) and mask [T][rows]
 * uint8 (written).  One thread per seat row, t from T - 1 down to 0, fp32, the fma forms of pgd_gae:
 *   acted(t):   delta = reward[t] + gamma cont(t) value[t+1] - value[t];   a = delta + gamma lam cont(t) a;   adv[t] = a, ret[t] = a + value[t]
 *   otherwise:  a = 0, adv[t] = 0, ret[t] = 0
 *   mask[t] = acted(t)
 * cont(t) and acted(t) select, they do not multiply: reward and value of a row that did not act, and value[t + 1] behind an agent that
 * does not continue, may hold anything, NaN included.  A done, and a PGD_F_RESET without done (the env-wide restart at 5 x horizon or when
 * no agent is left), end the agent's episode for GAE with no bootstrap, as pgd_gae does with a done; value[T] is read only by an agent
 * that is still in its seat behind step T - 1.  With every flag PGD_F_REPORT and no PGD_F_RESET the results are pgd_gae's bit for bit.
 * T >= 1, rows >= 1 (PGD_ERR_ARG).  Asynchronous on the engine's stream; may be captured in a HIP graph. */
int pgd_gae_masked(pgd_handle h, const float* d_reward, const float* d_value /*[T+1][rows]*/, const uint8_t* d_done, const uint32_t* d_flags,
                   int T, int rows, float gamma, float lam, float* d_adv, float* d_ret, uint8_t* d_mask);
/* ---- The PPO update behind a rollout: loss, the gradients of both networks, Adam ------------------------------------------------------
 * (No reference counterpart: the reference hands its arrays to an RL library, which runs autograd over the two networks of
 * pgdrive/examples/ppo_expert/numpy_expert.py:25-78 and an optimiser step, all as framework ops.)
 * The networks are pgd_mlp_actor_critic's as they stand: fp32, row-major [in][out], hidden 256, tanh; actor head columns 0..3 = mean0,
 * mean1, log_std0, log_std1 (columns at or beyond 4 are never read); a critic head of one column; all six critic pointers null = no
 * critic; in_dim 4 .. 416, w1, b1, w2, b2 of each network 16-byte aligned, obs_stride >= in_dim, out_cols >= 4 (PGD_ERR_ARG otherwise).
 *
 * pgd_ppo_grad: one minibatch in, loss statistics and the gradient of every weight out.  The minibatch is the list positions
 *   q_i = start + i * stride,  i = 0 .. rows - 1;   position i is LIVE iff q_i < count;   its rollout row is p_i = index[q_i]
 * with count = *batch->count, read by the kernels from device memory and held within [0, n_list] (null: n_list), and index null: p_i =
 * q_i.  n = the number of live positions.  The host never reads the count: the grids cover `rows`, and a tile of 16 positions with no live
 * one ends before it reads a weight.  stride = n_mb, start = j: the n_mb minibatches partition the list with no shuffle tensor;
 * stride = 1 and a shuffled index: the usual random minibatch.  An index entry is a row of the rollout arrays, [0, n_rows): one that is
 * not is a caller's error; it is held within the arrays, never followed outside them.
 * Per live row p the kernels read obs[p] (the first in_dim floats of a row of obs_stride), action[p][0..1], logp_old[p], adv[p] and
 * (with a critic) ret[p], evaluate both networks -- mean, ls (log_std), v -- and form
 *   A     = (adv - s[0]) * s[1], s = batch->adv_stats (two floats in device memory, as pgd_adv_stats writes them); null: A = adv
 *   z_k   = (a_k - mean_k) exp(-ls_k);   logp = -0.5 (z0^2 + z1^2) - ls0 - ls1 - log 2 pi;   r = exp(logp - logp_old)
 *   L_pi  = -(1/n) sum min(r A, clamp(r, 1 - clip, 1 + clip) A);   the gradient flows through a row iff r A <= clamp(r) A: then
 *           dL/dlogp = -A r / n, else 0;   dlogp/dmean_k = z_k exp(-ls_k),   dlogp/dls_k = z_k^2 - 1
 *   L_v   = (1/n) sum 0.5 (v - ret)^2 (no value clipping);   dL/dv = vf_coef (v - ret) / n
 *   H     = ls0 + ls1 + log(2 pi e);   L = L_pi + vf_coef L_v - ent_coef mean(H): the entropy term adds -ent_coef / n to dL/dls_k
 * and the backward pass through the two tanh layers of each network.  The gradients dW1, db1, dW2, db2, dW3, db3 of actor and critic
 * are WRITTEN (not accumulated) into the buffers of `grads`, which have the weights' own shapes; head columns at or beyond 4 are
 * written as zero.  n = 0: every gradient and statistic is zero (no NaN, no division by zero).  Null critic: the critic's gradient
 * buffers are not touched (they may be null) and L_v = 0.
 * d_stats, 8 floats: 0 n; 1 L_pi; 2 L_v; 3 mean H; 4 mean (logp_old - logp); 5 the share of live rows whose gradient is cut; 6 mean r;
 * 7 zero.
 * Rows that are not listed, list entries at or beyond the count, positions that are not live and observation columns at or beyond
 * in_dim may hold anything, NaN included: they reach no output (they are selected away, never multiplied by zero).
 * Deterministic: the same inputs give the same bytes -- no atomics; a sum over the minibatch's rows is taken by one owner in a fixed
 * order (weight gradients: rows in order within partitions of 1024, the partitions in order).  Arithmetic: fp32 -- the 256-wide
 * products (both forward layers, dZ2 W2^T, X^T dZ1, H1^T dZ2) on the f32 matrix cores --, except the per-row loss terms and
 * dL/d(mean, log_std, v) and the factor 1 / n, which one lane per row forms in double from the fp32 head outputs and rounds to fp32 once.
 * Scratch is the caller's: d_work, 16-byte aligned, work_bytes >= pgd_ppo_work_bytes(in_dim, rows, has_critic) (PGD_ERR_ARG below
 * it; the function returns 0 for an in_dim or rows the call refuses; rows 1 .. PGD_PPO_ROWS_MAX).  Nothing is allocated inside the
 * call: five launches (six with out_cols > 4), asynchronous on the engine's stream, capturable in a HIP graph from the first call. */
typedef struct pgd_ppo_batch {
  const float *obs, *action, *logp_old, *adv, *ret;   /* the rollout's arrays by row: [n_rows][obs_stride], [n_rows][2], [n_rows] x 3 */
  const float* adv_stats;                             /* two device floats (mean, 1 / (std + 1e-8)), or null */
  const int32_t* index;                               /* [n_list] rows, or null: position = row */
  const int32_t* count;                               /* device int32, or null: n_list */
  int32_t obs_stride, in_dim, n_rows, n_list, start, stride, rows;
} pgd_ppo_batch;
typedef struct pgd_ppo_hyper { float clip, vf_coef, ent_coef; } pgd_ppo_hyper;
typedef struct pgd_ppo_grads {                        /* device buffers of the weights' own shapes, written by pgd_ppo_grad */
  float *w1, *b1, *w2, *b2, *w3, *b3;
  float *vw1, *vb1, *vw2, *vb2, *vw3, *vb3;           /* untouched (and may be null) without a critic */
} pgd_ppo_grads;
#define PGD_PPO_ROWS_MAX 16777216
size_t pgd_ppo_work_bytes(int in_dim, int rows, int has_critic);
int pgd_ppo_grad(pgd_handle h, const pgd_actor_critic* nets, const pgd_ppo_batch* batch, const pgd_ppo_hyper* hyper,
                 const pgd_ppo_grads* grads, float* d_stats /*[8]*/, void* d_work, size_t work_bytes);
/* ---- The categorical head: two independent categorical distributions over the same networks ------------------------------------------
 * (No reference counterpart: the reference's env offers MultiDiscrete([discrete_steering_dim, discrete_throttle_dim]) with
 * discrete_action=True and leaves the distribution to an RL library; this is SB3's MultiCategorical factorisation.)
 * The networks are pgd_mlp_actor_critic's -- layout, alignment, hidden 256, tanh, the critic, in_dim 4 .. 416 -- with another actor head:
 * steering with ks bins and throttle with kt bins, 2 <= ks, kt and K = ks + kt <= 16 (PGD_ERR_ARG otherwise).
 * Layout: w3 [256][out_cols], b3 [out_cols], out_cols >= K (PGD_ERR_ARG below); columns 0 .. ks - 1 are the steering logits, columns
 * ks .. K - 1 the throttle logits, columns at or beyond K are never read.
 * Logits: fp32; the 256-term product on the f32 matrix cores as one 16-column tile, k split over the workgroup's four waves: wave w forms
 * the k-ordered fma chain over k = 64 w .. 64 w + 63 from zero, logit = ((P0 + P1) + P2) + P3 + b3.  The head's weights are read from
 * global memory, not staged: the workgroup's LDS is pgd_mlp_actor_critic's.
 * Per head (fp32 logits l_j, j < K_head):  m = max_j l_j;  lse = m + log(sum_j exp(l_j - m));  logp_j = l_j - lse;  p_j = exp(logp_j)
 * (max and sums in index order).  As compiled: the forward launch's exp and log are fp32 `expf` / `logf` under the library's build flags, i.e.
 * the approximate forms (v_exp_f32 / v_log_f32 with the input or output scaled, about 1 ulp of the instruction plus the scaling's rounding);
 * pgd_ppo_grad_cat works in double and forms p_j as exp(l_j - m) / sum_k exp(l_k - m), the same number as exp(logp_j) to a few 2^-53.
 * Sampling: u_s = unit(r1), u_t = unit(r2) with r1, r2, unit() and g exactly pgd_mlp_actor_critic's two draws (same seed ^ 0xac7012c1,
 * global row, stream, tick and tick ^ 0x80000000, the device counter of pgd_actor_critic_tick included).  c_j = p_0 + ... + p_j, summed
 * in fp32 in index order; the index is the number of j in [0, K_head - 1) with c_j <= u -- it cannot leave the head whatever the last
 * partial sum rounds to.  logp = logp_s[i_s] + logp_t[i_t].
 * PGD_AC_DETERMINISTIC: the index is the argmax, the lowest index among equal logits; logp is that of the argmax.
 * Outputs per row: d_action_index int32 [rows][2] (i_s, i_t); d_logp, d_value as pgd_mlp_actor_critic (d_value bit for bit its value on
 * the same inputs); d_actions float [rows][2], the buffer pgd_step reads:
 *   default            the grid value (float) i * (2.0f / (float) (K_head - 1)) - 1.0f -- one multiplication, then one subtraction, the
 *                      quotient correctly rounded: pgd_step's own conversion of a discrete action -- for an engine with continuous actions
 *   PGD_AC_EMIT_INDEX  the index as a float, for an engine with discrete_action set
 * pgd_mlp_actor_critic_cat_rows is to pgd_mlp_actor_critic_cat what pgd_mlp_actor_critic_rows is to pgd_mlp_actor_critic: a listed row
 * gets bit for bit what the full launch gives it; rows of the range that are not listed get action 0, 0, index 0, 0, logp 0 and (with a
 * critic) value 0 from a clearing launch in front; the host never reads *d_count.  A bound observation table (pgd_obs_norm_bind) is
 * applied by all three calls of this section as by their Gaussian namesakes.
 *
 * pgd_ppo_grad_cat: pgd_ppo_grad with this head.  Every argument, the minibatch rule, the critic, d_stats' slots, n = 0, what may hold
 * NaN, the determinism and the capture rule are pgd_ppo_grad's; batch->action is not read (and may be null); d_action_index is the
 * rollout's [n_rows][2].  A live row's index outside its head is a caller's error: it is held within [0, K_head) and never followed
 * outside an array.  Per live row, with i the taken index of a head:
 *   logp = logp_s[i_s] + logp_t[i_t];   r, the clipped surrogate, the cut rule, A, L_v, 1 / n: pgd_ppo_grad's
 *   H = H_s + H_t,  H_head = -sum_j p_j logp_j              (d_stats[3] = mean H;  d_stats[4] = mean (logp_old - logp))
 *   dlogp/dl_j = [j == i] - p_j;   dH_head/dl_j = -p_j (logp_j + H_head)
 *   dL/dl_j = dL/dlogp ([j == i] - p_j) + ent_coef p_j (logp_j + H_head) / n
 * formed in double from the fp32 logits (logp_j, p_j and H_head included; sums over a head in index order) and rounded to fp32 once.
 * Head columns at or beyond K of dW3 / db3 are written as zero.  Scratch: the caller's, 16-byte aligned, work_bytes >=
 * pgd_ppo_cat_work_bytes(in_dim, rows, has_critic) (0: the call refuses the shape; never below pgd_ppo_work_bytes: dOut is [rows][16]
 * here).  Five launches (six with out_cols > K), asynchronous on the engine's stream, capturable from the first call. */
#define PGD_AC_EMIT_INDEX 2u
int pgd_mlp_actor_critic_cat(pgd_handle h, int group, const float* d_obs, int obs_stride, int in_dim, const pgd_actor_critic* nets,
                             int32_t ks, int32_t kt, uint32_t seed, uint32_t tick, uint32_t flags, float* d_actions /*[rows][2]*/,
                             int32_t* d_action_index /*[rows][2]*/, float* d_logp /*[rows]*/, float* d_value /*[rows], may be null without critic*/);
int pgd_mlp_actor_critic_cat_rows(pgd_handle h, int group, const float* d_obs, int obs_stride, int in_dim, const pgd_actor_critic* nets,
                                  int32_t ks, int32_t kt, uint32_t seed, uint32_t tick, uint32_t flags, const int32_t* d_rows,
                                  const int32_t* d_count, float* d_actions, int32_t* d_action_index, float* d_logp, float* d_value);
size_t pgd_ppo_cat_work_bytes(int in_dim, int rows, int has_critic);
int pgd_ppo_grad_cat(pgd_handle h, const pgd_actor_critic* nets, const pgd_ppo_batch* batch, const pgd_ppo_hyper* hyper,
                     const pgd_ppo_grads* grads, int32_t ks, int32_t kt, const int32_t* d_action_index /*[n_rows][2]*/,
                     float* d_stats /*[8]*/, void* d_work, size_t work_bytes);
/* Population mean and 1 / (std + 1e-8) of adv over the live entries of a list -- adv[index[q]] (index null: adv[q]) for q < count, the
 * count as for pgd_ppo_grad -- into two device floats.  One workgroup, a fixed summation order: deterministic.  n = 0: (0, 1).
 * Entries that are not listed may hold NaN.  The call is not told how long d_adv is: every index entry below the count must be a valid
 * position of it (the caller's contract; pgd_rollout_index's entries are) -- unlike pgd_ppo_grad, which knows n_rows, it cannot hold an entry
 * within the array.  The final quotients are formed in double.  Asynchronous on the engine's stream; capturable. */
int pgd_adv_stats(pgd_handle h, const float* d_adv, const int32_t* d_index, const int32_t* d_count, int n_list, float* d_out /*[2]*/);
/* One Adam step on a flat parameter buffer of n_elem floats; d_grad, d_m, d_v of the same length.
 *   max_grad_norm > 0:  g = grad * min(1, max_grad_norm / (|grad| + 1e-6)), |grad| over all n_elem (a deterministic reduction); else g = grad
 *   m = beta1 m + (1 - beta1) g;   v = beta2 v + (1 - beta2) g^2;   p -= lr (m / (1 - beta1^t)) / (sqrt(v / (1 - beta2^t)) + eps)
 * The step number t lives in DEVICE memory: d_step, four 32-bit words, 4-byte aligned, owned by the caller and zero before the first
 * step.  Word 0 is the int32 count of steps taken; the call advances it by one when its kernels RUN and uses the new value, so a
 * captured call replayed takes step t + 1, not the captured one (the reasoning of pgd_actor_critic_tick).  Words 1..3 are the call's
 * record -- the clipping scale and the two bias corrections as floats --, written with the counter by a one-workgroup launch and read by
 * the elementwise launch behind it: no kernel reads the counter while another workgroup of its launch writes it.  m and v are updated in
 * fp32; the record and the quotient of the parameter step are formed in double and rounded to fp32 once.  0 <= beta < 1,
 * n_elem >= 1 (PGD_ERR_ARG).  Two launches, asynchronous on the engine's stream; capturable. */
int pgd_adam(pgd_handle h, float* d_param, const float* d_grad, float* d_m, float* d_v, int n_elem, int32_t* d_step /*[4]*/, float lr,
             float beta1, float beta2, float eps, float max_grad_norm);
/* ---- Random minibatches and an early stop of the update, on the device ----------------------------------------------------------------
 * pgd_shuffle_index: a keyed permutation of a row list, computed per entry.  c = the live count as for pgd_ppo_grad (*d_count within
 * [0, n_list], n_list without a pointer; read on the device); e = epoch + (d_epoch ? (uint32_t)*d_epoch : 0) -- the rule of
 * pgd_actor_critic_tick: a captured call replays with its argument, the device counter is what advances.  For every q < c:
 *   d_out[q] = d_index ? d_index[pi(q)] : pi(q);       entries at and beyond c are not written; d_out must not alias d_index.
 * pi is a bijection of [0, c): a 6-round unbalanced Feistel network on b = max(2, bit_length(c - 1)) bits, bl = b >> 1 high and
 * br = b - bl low bits, with cycle walking.  From x = q, repeat until x < c:
 *   L = x >> br;  R = x & (2^br - 1);  (lb, rb) = (bl, br);
 *   for r = 0 .. 5:  f = pgd_rng(seed ^ 0x5b0ff1e5, R, r, e) & (2^lb - 1);  (L, R) = (R, L ^ f);  swap(lb, rb);
 *   x = (L << rb) | R
 * with pgd_rng(s, a, b, c) = H(s ^ H(a ^ H(b ^ H(c + 0x9e3779b9)))), H the 32-bit PCG output hash -- integers only.  The walk has no
 * cap (x runs through the cycle that contains q; the domain is below 2 c for c >= 3, so its mean length is below 2).
 * One thread per q, no atomics, no scratch; asynchronous on the engine's stream, capturable from the first call.  PGD_ERR_ARG: a null
 * handle or d_out, d_out == d_index, n_list < 0 or above PGD_PPO_ROWS_MAX.
 *
 * pgd_adam_gated: pgd_adam behind a gate in device memory.  d_gate, four int32 (4-byte aligned, the caller's, zeroed by the caller
 * where an update begins): 0 stopped, 1 steps applied since it was cleared, 2 steps skipped, 3 1 iff THIS call skipped.  One thread of
 * the first launch decides:   stop = gate[0] != 0 || (d_kl && !(*d_kl <= kl_limit))        (a NaN stops)
 *   skip:   gate[0] = 1, gate[2] += 1, gate[3] = 1, *d_count_gate = 0 where the pointer is given; d_step, d_param, d_m and d_v keep
 *           their bytes.  (A count that the later pgd_ppo_grad / pgd_shuffle_index calls of the update read: zeroed, they find no live
 *           row, write zero gradients and a statistics row with n = 0.)
 *   apply:  gate[1] += 1, gate[3] = 0, then pgd_adam's step with lr_eff = lr * *d_lr_scale (one fp32 product; lr without a pointer).
 * With d_lr_scale, d_kl and d_count_gate null and a zeroed gate the results are pgd_adam's bit for bit.  The refusals of pgd_adam, and a
 * null or misaligned d_gate.  Two launches, asynchronous on the engine's stream; capturable. */
int pgd_shuffle_index(pgd_handle h, const int32_t* d_index /*nullable*/, const int32_t* d_count /*nullable*/, int n_list, uint32_t seed,
                      uint32_t epoch, const int32_t* d_epoch /*nullable*/, int32_t* d_out /*[n_list]*/);
int pgd_adam_gated(pgd_handle h, float* d_param, const float* d_grad, float* d_m, float* d_v, int n_elem, int32_t* d_step /*[4]*/, float lr,
                   float beta1, float beta2, float eps, float max_grad_norm, const float* d_lr_scale /*nullable*/, const float* d_kl /*nullable*/,
                   float kl_limit, int32_t* d_gate /*[4]*/, int32_t* d_count_gate /*nullable*/);
/* ---- Safe RL behind a rollout: cost critic, cost GAE, the Lagrange multiplier, PPO-Lagrangian gradients -------------------------------
 * (No reference counterpart: the reference hands info["cost"] to an RL library; safe_pgdrive_env.py:7-60.  With safe_rl_env a crash is a
 * cost and not a termination; these entry points keep a policy under a cost limit without leaving the device.)
 * A cost critic is a third network of the value network's shapes (pgd_value_net: w3 [256][1]; w1, b1, w2, b2 16-byte aligned).
 *
 * pgd_mlp_actor_critic_cost: pgd_mlp_actor_critic with the cost critic beside actor and critic in the same launch, grid (ceil(rows / 16),
 * 3).  Every argument, the arithmetic, PGD_AC_DETERMINISTIC, the device tick and the refusals (in_dim 4 .. 416, alignment) as there;
 * in addition both critics are required: all six value pointers of `nets`, all six of `cost_net`, d_value and d_cost_value
 * (PGD_ERR_ARG).  d_actions, d_logp, d_value are bit for bit what pgd_mlp_actor_critic writes on the same inputs; d_cost_value is bit for
 * bit what it writes into d_value when cost_net is handed to it as the value network.  One launch, asynchronous, capturable.
 *
 * pgd_cost_gae: the costs of a rollout from its flags, their GAE and the episode-cost bookkeeping.  flags, done, cost, cadv, cret
 * [T][rows], cost_value [T + 1][rows], time-major.  One thread per row, fp32:
 *   cost[t][r] = out_of_road ? costs[0] : crash_vehicle ? costs[1] : crash_object ? costs[2] : 0      (PGD_F_OUT_OF_ROAD, PGD_F_CRASH_VEHICLE,
 *                PGD_F_CRASH_OBJECT of flags[t][r]; the precedence of pgd_step_info's cost and of PGDriveEnv.cost_function,
 *                pgdrive_env.py:197-207; a selection of the three floats, no other flag bit matters)
 *   forward, t = 0 .. T - 1 in order:  run += cost;  at done[t][r]:  ep_sum += run, ep_count += 1, run = 0
 *   reverse: pgd_gae's recursion in its fma forms with cost as the reward, gamma and lam the call's own
 * d_run [rows] is read and written: it carries the cost of the unfinished episode into the next rollout (zero it before the first call,
 * and for every env that is reset by hand).  d_ep_sum and d_ep_count [rows] are WRITTEN: the finished episodes of this rollout only.  A
 * done finishes an episode whatever ended it, a horizon truncation included, as for GAE.  d_cadv and d_cret are bit for bit what pgd_gae
 * gives on d_cost, d_cost_value, d_done.  T >= 1, rows >= 1 (PGD_ERR_ARG).  One launch, asynchronous, capturable.
 *
 * pgd_lagrange: one step of the multiplier from the finished episodes of a rollout.  d_state: four device floats -- 0 lambda, 1 J_c (the
 * mean episode cost last seen), 2 the number of episodes behind it, 3 unused --, zero (or lambda's first value in slot 0) before the
 * first call.  One workgroup: thread i takes rows i, i + 256, ... in order, a butterfly per wave, the four waves in order (the order of
 * pgd_adv_stats), the sums in double and the counts as integers: the same input gives the same bytes.
 *   E = sum ep_count.   E > 0:  J_c = sum ep_sum / E;   lambda <- min(lambda_max, max(0, lambda + lr (J_c - cost_limit)));  slots 1, 2 written
 *   E == 0: the state keeps every byte.
 * The quotient and the step are formed in double and rounded to fp32 once.  A captured call replayed takes the next step from the lambda
 * it finds (the reasoning of pgd_adam's counter).  rows >= 1, lambda_max >= 0 (PGD_ERR_ARG).  Rows with ep_count 0 hold ep_sum 0.
 *
 * pgd_adv_mix: the advantage the policy sees, per entry i < n:
 *   out = ((adv - m) s - lambda (cadv - m_c)) / (1 + lambda)
 * (m, s) = d_adv_stats, null: (0, 1); m_c = d_cadv_stats[0], null: 0 (both as pgd_adv_stats writes them); lambda = d_state[0].  The cost
 * advantage is centred, NOT rescaled: its scale is the cost's magnitude, which lambda is there to price.  Formed in double, rounded to
 * fp32 once; lambda = 0 gives (adv - m) s.  One read of two arrays, one write.  n >= 1 (PGD_ERR_ARG).  One launch, asynchronous, capturable.
 *
 * pgd_ppo_grad_cost: pgd_ppo_grad with three networks.  Network 2 is a critic with ret = cost->cost_ret and vf_coef = cost->cvf_coef:
 *   L_c = (1/n) sum 0.5 (v_c - cost_ret)^2;   dL/dv_c = cvf_coef (v_c - cost_ret) / n
 * batch->adv is normally pgd_adv_mix's output with batch->adv_stats null; the actor's formulas are pgd_ppo_grad's.  d_stats: slots 0..6 as
 * pgd_ppo_grad, slot 7 = L_c.  The minibatch rule (start / stride / rows / index / count), the determinism and its summation orders, what
 * may hold NaN (cost_ret as ret: rows that are not listed reach no output), n = 0 -> every gradient and statistic zero, and the refusals
 * are pgd_ppo_grad's; both critics and every gradient buffer are required.  Actor and critic gradients and d_stats[0..6] are bit for bit
 * pgd_ppo_grad's on the same inputs; the cost critic's gradients and d_stats[7] are bit for bit the critic gradients and d_stats[2] of a
 * pgd_ppo_grad call that is handed cost_net as value network, cost_ret as ret and cvf_coef as vf_coef.  Scratch: the caller's, 16-byte
 * aligned, work_bytes >= pgd_ppo_cost_work_bytes(in_dim, rows) (0: the call refuses the shape).  The launches are pgd_ppo_grad's with a
 * third network in their grids: five (six with out_cols > 4), asynchronous, capturable from the first call. */
typedef struct pgd_value_net { const float *w1, *b1, *w2, *b2, *w3, *b3; } pgd_value_net;  /* a critic's shapes: w3 [256][1] */
typedef struct pgd_ppo_cost { const float* cost_ret; float cvf_coef; } pgd_ppo_cost;
typedef struct pgd_value_grads { float *w1, *b1, *w2, *b2, *w3, *b3; } pgd_value_grads;
int pgd_mlp_actor_critic_cost(pgd_handle h, int group, const float* d_obs, int obs_stride, int in_dim, const pgd_actor_critic* nets,
                              const pgd_value_net* cost_net, uint32_t seed, uint32_t tick, uint32_t flags, float* d_actions /*[rows][2]*/,
                              float* d_logp /*[rows]*/, float* d_value /*[rows]*/, float* d_cost_value /*[rows]*/);
int pgd_cost_gae(pgd_handle h, const uint32_t* d_flags /*[T][rows]*/, const uint8_t* d_done, const float* d_cost_value /*[T+1][rows]*/, int T,
                 int rows, const float costs[3] /* out_of_road, crash_vehicle, crash_object */, float gamma, float lam,
                 float* d_cost /*[T][rows]*/, float* d_cadv, float* d_cret, float* d_run /*[rows], in/out*/, float* d_ep_sum /*[rows]*/,
                 int32_t* d_ep_count /*[rows]*/);
int pgd_lagrange(pgd_handle h, const float* d_ep_sum, const int32_t* d_ep_count, int rows, float cost_limit, float lr, float lambda_max,
                 float* d_state /*[4]: lambda, J_c, episodes, 0*/);
int pgd_adv_mix(pgd_handle h, const float* d_adv, const float* d_cadv, int n, const float* d_adv_stats /*[2] or null*/,
                const float* d_cadv_stats /*[2] or null*/, const float* d_state /* pgd_lagrange's */, float* d_out /*[n]*/);
size_t pgd_ppo_cost_work_bytes(int in_dim, int rows);
int pgd_ppo_grad_cost(pgd_handle h, const pgd_actor_critic* nets, const pgd_value_net* cost_net, const pgd_ppo_batch* batch,
                      const pgd_ppo_cost* cost, const pgd_ppo_hyper* hyper, const pgd_ppo_grads* grads, const pgd_value_grads* cost_grads,
                      float* d_stats /*[8]*/, void* d_work, size_t work_bytes);
/* ---- Expert-guided PPO: the gradient that knows which rows the guardian overrode -------------------------------------------------------
 * (No reference counterpart: the reference puts takeover and raw_action into the step info, agent_manager.py:187, and leaves their use
 * to an RL library.)  Under a takeover the applied action is not the sampled one: the advantage of such a row credits an action the
 * agent did not take, and the clipped surrogate would push the probability of the one it sampled.
 * pgd_ppo_grad_guided: pgd_ppo_grad (cost_net, cost, cost_grads null) or pgd_ppo_grad_cost (all three given) -- one, two or three
 * networks, the Gaussian head -- with a guide.  Notation, the minibatch rule, the critics, 1 / n and the arithmetic are pgd_ppo_grad's.
 * Per live row p:
 *   u     = guide->mask ? (mask[p] & mask_bits) != 0 : 1          the row is GUIDED
 *   s     = !u || (mode & PGD_GUIDE_KEEP_SURROGATE)               the row carries the surrogate
 *   e_k   = exp(-ls_k);   zt_k = (target[p][k] - mean_k) e_k;   c = u ? bc_coef / n : 0
 *   g     = pgd_ppo_grad's dL/dlogp where s holds, 0 otherwise
 *   dL/dmean_k = g z_k e_k - c zt_k e_k
 *   dL/dls_k   = g (z_k^2 - 1) + c (1 - zt_k^2) - ent_coef / n
 * that is L = (1/n) [ sum over s of the clipped surrogate's terms + bc_coef sum over u of -logp(target) ] + vf_coef L_v - ent_coef mean H.
 * 1 / n is over ALL live rows of the minibatch: a masked row contributes zero and does not renormalise, so strided minibatches still
 * sum to the whole.  The critics regress on ret (cost_ret) on every live row -- the returns are those of the guarded system -- and the
 * entropy term applies to every live row.
 * mask [n_rows] and target [n_rows][target_stride] are indexed by rollout ROW (not by list position), read at live rows only through
 * the clamp of the index, the target only where u holds and only its columns 0 and 1: a NaN in the target of a free or dead row, or in
 * columns 2 and 3 of a stride-4 target, reaches no output.  u and s SELECT: a row without the surrogate takes nothing from its action,
 * advantage or logp_old.  The free part of dL/d(mean, ls) is formed from pgd_ppo_grad's operands in its order, in double, rounded once,
 * and the imitation part is added only where u holds: with NO guided row the gradients and d_stats[0..7] are bit for bit pgd_ppo_grad's
 * (with a cost net pgd_ppo_grad_cost's).
 * d_stats, 12 floats: 0 n; 2 L_v, 3 mean H, 7 L_c (0 without a cost net): means over n; 1 L_pi, 4 mean (logp_old - logp), 5 the share
 * of cut rows, 6 mean r: means over n_s, the rows with s, each 0 when n_s = 0 (slot 4 keeps pgd_adam_gated's meaning: it averages the
 * rows that carry a ratio); 8 n_g, the guided live rows; 9 bc_loss = the mean of -logp(target) over n_g, 0 when n_g = 0; 10, 11 zero.
 * Scratch: pgd_ppo_work_bytes / pgd_ppo_cost_work_bytes, unchanged (n_g and the sum of -logp(target) take two free slots of the
 * tile-sum record).  Launches: pgd_ppo_grad's, with the rows kernel and the statistics kernel in their guided forms; same LDS and the
 * same refusal of in_dim > 416; no atomics, deterministic; nothing is allocated; asynchronous, capturable from the first call.
 * Refusals (PGD_ERR_ARG): pgd_ppo_grad's / pgd_ppo_grad_cost's, a cost net without cost or cost_grads (or the reverse), and the
 * guide's: null guide or target, target_stride < 2, a mode bit other than PGD_GUIDE_KEEP_SURROGATE, bc_coef negative or not finite,
 * mask_bits == 0 with a mask. */
typedef struct pgd_ppo_guide {
  const float*   target;        /* [n_rows][target_stride], by rollout ROW (not list position) */
  const uint8_t* mask;          /* [n_rows] by row, or null: every live row is guided */
  int32_t  target_stride;       /* >= 2; 2 for applied actions, 4 for pgd_guardian's d_trace */
  uint32_t mask_bits;           /* row is guided iff (mask[row] & mask_bits) != 0 */
  float    bc_coef;             /* >= 0, finite */
  uint32_t mode;                /* PGD_GUIDE_KEEP_SURROGATE; other bits PGD_ERR_ARG */
} pgd_ppo_guide;
#define PGD_GUIDE_KEEP_SURROGATE 1u
int pgd_ppo_grad_guided(pgd_handle h, const pgd_actor_critic* nets, const pgd_value_net* cost_net /* or null */,
                        const pgd_ppo_batch* batch, const pgd_ppo_cost* cost /* with cost_net */, const pgd_ppo_guide* guide,
                        const pgd_ppo_hyper* hyper, const pgd_ppo_grads* grads, const pgd_value_grads* cost_grads /* with cost_net */,
                        float* d_stats /*[12]*/, void* d_work, size_t work_bytes);
/* ---- GAE that bootstraps through a time limit: terminal values on the device (single-agent engines) -------------------------------------
 * (No reference counterpart: the reference returns the terminal observation from env.step, base_env.py:303-344, and `max_step` in its
 * info, base_env.py:190-192; an RL library evaluates its critic on it on the host and patches the reward.)
 * pgd_gae and pgd_cost_gae end the episode at every done with a one-step target of 0.  A time limit is no property of the task and the
 * observation holds no clock; the entry points below give a truncated episode the critic's value of its terminal observation instead.
 * For row r of a single-agent engine and step t, let f = flags[t][r] and d = done[t][r], as pgd_step wrote them, and safe =
 * pgd_config.safe_rl_env of the engine:
 *   natural(t)   = f & (PGD_F_ARRIVE | PGD_F_OUT_OF_ROAD | PGD_F_CRASH_VEHICLE | PGD_F_CRASH_OBJECT | PGD_F_CRASH_BUILDING),
 *                  and false when safe && f & (PGD_F_CRASH_VEHICLE | PGD_F_CRASH_OBJECT)      the step's own done rule (pgdrive_env.py:162-194,
 *                                                                                             safe_pgdrive_env.py:49-56)
 *   truncated(t) = d && (f & PGD_F_MAX_STEP) && !natural(t)                                   the clock alone ended the episode
 * Both pgd_config.horizon and a scenario's max_steps set PGD_F_MAX_STEP and count; where a termination falls on the same step it wins:
 * no bootstrap.  On a multi-agent engine the cause of a done cannot be read from the flags alone (the tollgate's stay-time rule, the
 * env-wide cut at 5 x horizon): not served.
 *
 * pgd_mlp_terminal_value: the value of the terminal observation of every truncated row, 0 for every other row.  d_term_obs: the final_obs
 * array of the step info (pgd_step_info), or any [rows][obs_stride] array; rows and `group` as for pgd_mlp_actor_critic; d_flags, d_done
 * the FULL arrays of the step; d_term_value [rows] and, with cost_critic, d_term_cost_value [rows] are written at every row of the range:
 *   term_value[r] = truncated ? critic(term_obs[r]) : 0          term_cost_value[r] = truncated ? cost_critic(term_obs[r]) : 0
 * One launch, grid (ceil(rows / 16), 1 or 2): a workgroup reads the flags and dones of its 16 rows first and, when none is truncated,
 * writes its zeros and ends before it reads a weight or an observation (a NaN there reaches no output); otherwise it is the critic
 * workgroup of pgd_mlp_actor_critic with the rows that are not truncated entered as zeros (their term_obs row is stale or was never
 * written and may hold NaN).  A truncated row receives bit for bit what pgd_mlp_actor_critic writes into d_value for the same
 * observation row and weights, and d_term_cost_value what a second call writes that is handed cost_critic as `critic`.  No noise, no
 * tick.  in_dim 4 .. 416, obs_stride >= in_dim, all six pointers of `critic` (and of `cost_critic` when given) set, w1, b1, w2, b2
 * 16-byte aligned, d_term_cost_value with cost_critic, a single-agent engine (PGD_ERR_ARG otherwise).  Asynchronous on the engine's stream
 * (group >= 0: the group's); capturable in a HIP graph.
 *
 * pgd_gae_bootstrap: pgd_gae with one more time-major input term_value [T][rows], fp32, the fma forms of pgd_gae:
 *   vb = done[t] ? term_value[t] : value[t + 1];   delta = reward[t] + gamma vb - value[t]
 *   adv[t] = delta + gamma lam (done[t] ? 0 : adv[t + 1]);   ret[t] = adv[t] + value[t]
 * done SELECTS: value[t + 1] behind a done may hold anything, NaN included.  The trace still ends at every done; only the one-step
 * target changes.  With term_value zero everywhere and finite inputs, adv and ret equal pgd_gae's as float values.
 * pgd_cost_gae_bootstrap: pgd_cost_gae with term_cost_value [T][rows]: the forward pass (cost, run, ep_sum, ep_count) is pgd_cost_gae's
 * bit for bit -- a truncated episode still finishes for the multiplier's books --, the reverse pass the recursion above with cost as
 * the reward.  Refusals, launches and streams as for pgd_gae and pgd_cost_gae. */
int pgd_mlp_terminal_value(pgd_handle h, int group, const float* d_term_obs, int obs_stride, int in_dim, const pgd_value_net* critic,
                           const pgd_value_net* cost_critic /* or null */, const uint32_t* d_flags /*[rows]*/, const uint8_t* d_done /*[rows]*/,
                           float* d_term_value /*[rows]*/, float* d_term_cost_value /*[rows], with cost_critic*/);
int pgd_gae_bootstrap(pgd_handle h, const float* d_reward, const float* d_value /*[T+1][rows]*/, const uint8_t* d_done,
                      const float* d_term_value /*[T][rows]*/, int T, int rows, float gamma, float lam, float* d_adv, float* d_ret);
int pgd_cost_gae_bootstrap(pgd_handle h, const uint32_t* d_flags /*[T][rows]*/, const uint8_t* d_done, const float* d_cost_value /*[T+1][rows]*/,
                           const float* d_term_cost_value /*[T][rows]*/, int T, int rows, const float costs[3], float gamma, float lam,
                           float* d_cost /*[T][rows]*/, float* d_cadv, float* d_cret, float* d_run /*[rows], in/out*/,
                           float* d_ep_sum /*[rows]*/, int32_t* d_ep_count /*[rows]*/);
/* ---- The expert guardian: use_saver / save_level on the device (single-agent engines) ----------------------------------------------------
 * pgdrive/policy/AI_protect_policy.py:8-59: a second policy, the expert, watches the acting policy and replaces its action where the
 * car is about to leave the road or to hit something; the step info carries takeover_start / takeover_end / takeover
 * (agent_manager.py:187).  pgd_guardian is ONE launch between the evaluation of the acting policy and the step: it reads the engine's
 * state and the observation rows the last step or reset wrote, evaluates the expert, and writes the action buffer the step is to read.
 * Rows = the envs of a single-agent engine (`group` as for pgd_mlp_actor_critic).
 *
 * d_obs / obs_stride: the observation rows ([rows][obs_stride], the first D = pgd_obs_dim floats are the row).  A table bound with
 * pgd_obs_norm_bind is IGNORED: the expert was trained on raw observations.
 * expert: the expert's six policy tensors, the value network's six pointers null; layout, alignment and head as pgd_mlp_actor_critic.
 * cfg->expert_in_dim (4 .. 416): D, or D + 1 with PGD_GUARD_LEGACY_LATERAL.  With that bit the expert's row is
 *   obs[0..7] | clip((lat * 2 / 4.5 + 1) / 2, 0, 1) | obs[8..]       lat = the lateral coordinate of the vehicle's position on its
 * current lane (SI_LANE) -- the float the reference's shipped weights were trained with (state_obs.py:97-100, commented out upstream).
 * The expert's head is pgd_mlp_actor_critic's bit for bit: same key stream, g = env_base + env, cfg->tick plus the device counter of
 * pgd_actor_critic_tick; PGD_GUARD_DETERMINISTIC: z = 0.  The reference samples (`expert(obs, deterministic=False)`): the default.
 *
 * The rule, per row, fp32 (no contraction, no re-association); a = d_agent_actions[row] (raw, unclipped), e = the expert's sample,
 * s = cfg->save_level, n = num_lasers, lidar[] = the last n floats of the obs row:
 *   steer = a0, thr = a1
 *   s > 0.9:   steer = e0, thr = e1
 *   s > 1e-3:  hd = heading_diff(vehicle.lane) - 0.5;  v = speed [km/h];  f = min(1 + |hd| * v * max_speed, 10 s)   (max_speed: the spawn
 *              record's; the product from left to right, as upstream)
 *              out of road:  (obs0 < 0.04 f and hd < 0) or (obs1 < 0.04 f and hd > 0) or obs0 <= 1e-3 or obs1 <= 1e-3:
 *                            steer = e0, thr = e1, and thr = 0.5 where v < 5
 *              side:         L = n / 4, R = 3 n / 4 (integers);  min lidar[L - 4 .. L + 5] < (s + 0.1) / 10 or the same around R: steer = e0
 *              front:        a1 >= 0 and e1 <= 0 and min(lidar[0..9], lidar[n - 10..n - 1]) < s:  thr = e1
 *   pre = d_state[row] != 0, and 0 where d_prev_flags[row] has PGD_F_RESET (the vehicle was reset: base_vehicle.py:332)
 *   now = (a0 != steer or a1 != thr), compared as floats;   d_state[row] = now
 *   takeover_start = !pre & now,  takeover_end = pre & !now,  takeover = pre & now
 *   d_applied[row] = takeover ? (steer, thr) : a         -- the reference applies the correction from the second consecutive step on
 *   PGD_GUARD_IMMEDIATE (NOT a reference behaviour): d_applied[row] = now ? (steer, thr) : a; the info bits are unchanged.
 * The regimes compare s as a double; 10 s and (s + 0.1) / 10 are formed in double from the fp32 s and rounded to fp32 once; 0.04, 1e-3
 * and 5 are fp32 constants and 0.04 f is an fp32 product: a float64 checker that rounds the same way agrees exactly.  s <= 1e-3 still runs
 * the bookkeeping: now is false everywhere and d_applied = a.  The fan is the obs row's (the reference reads the un-noised cloud points,
 * which this engine does not keep: callers refuse lidar noise together with the guardian).
 *
 * d_state [rows] uint8, in / out, the caller's: vehicle.takeover.  d_prev_flags [rows]: the flags of the previous step, or null.
 * d_info [rows] uint8: bit 0 takeover, bit 1 takeover_start, bit 2 takeover_end.  d_applied [rows][2] MAY alias d_agent_actions: a
 * row's action is read before anything of the row is written, and no row reads another's.  d_trace [rows][4] or null: the expert's
 * steering and throttle, the lateral float (0 without PGD_GUARD_LEGACY_LATERAL) and f.
 * Refusals (PGD_ERR_ARG): a multi-agent engine, num_lasers < 40 (the reference's slices need it), expert_in_dim other than D (+ 1), a
 * value network in `expert`, unknown mode bits, d_agent_actions / d_applied not 8-byte and d_trace not 16-byte aligned; PGD_ERR_STATE
 * before maps and scenarios are uploaded.  One launch, grid ceil(rows / 16), the workgroup and LDS of pgd_mlp_actor_critic's actor;
 * asynchronous on the engine's stream (group >= 0: the group's), allocates nothing, capturable in a HIP graph from its first call. */
typedef struct pgd_guardian_config {
  int32_t expert_in_dim;
  float save_level;
  uint32_t seed, tick, mode;
} pgd_guardian_config;
#define PGD_GUARD_LEGACY_LATERAL 1u
#define PGD_GUARD_DETERMINISTIC 2u
#define PGD_GUARD_IMMEDIATE 4u
int pgd_guardian(pgd_handle h, int group, const float* d_obs, int obs_stride, const pgd_actor_critic* expert, const pgd_guardian_config* cfg,
                 const float* d_agent_actions /*[rows][2]*/, const uint32_t* d_prev_flags /*[rows] or null*/, uint8_t* d_state /*[rows]*/,
                 float* d_applied /*[rows][2]*/, uint8_t* d_info /*[rows]*/, float* d_trace /*[rows][4] or null*/);
/* ---- Reward scaling by the running return, in front of GAE (every engine) ---------------------------------------------------------------
 * (No reference counterpart: the reference hands its rewards to an RL library; this is the norm_reward half of Stable-Baselines3's
 * VecNormalize -- the reward divided by the standard deviation of the running discounted return -- as one call over a rollout.)
 * Time-major device arrays: reward (float), done (the uint8 pgd_step writes) [T][rows]; flags [T][rows] (the uint32 pgd_step writes) or
 * null; scaled [T][rows] float, WRITTEN.  Two caller-owned device objects live across calls:
 *   carry  [rows] floats: the discounted return of each row's running episode; zero before the first call
 *   record four doubles, 8-byte aligned: count, mean, m2, scale; 1e-4, 0, 1e-4, 1 before the first call (VecNormalize's RunningMeanStd:
 *          mean 0, variance 1, count 1e-4; m2 = variance * count)
 * Per row r, with R = carry[r], for t = 0 .. T - 1 in order, fp32:
 *   flags null:   R = fma(gamma, R, reward[t][r]);  R is a SAMPLE;  then R = 0 where done[t][r]
 *   flags given:  acted(t) (as for pgd_gae_masked):  the same update and sample, then R = 0 unless cont(t)
 *                 otherwise:  no sample, R = 0           (a seat that changes hands starts from 0)
 * and carry[r] = R behind the loop.  acted and cont SELECT: the reward of a row that did not act may be NaN and reaches nothing.
 * The statistics, in double: n, bmean and bm2 = the number, the mean and the sum of squared deviations of ALL samples of the call, merged
 * into the record by Chan's parallel update
 *   delta = bmean - mean;  tot = count + n;  mean += delta n / tot;  m2 += bm2 + delta^2 count n / tot;  count = tot
 * and then scale = 1 / sqrt(m2 / count + eps).  A call without a sample leaves count, mean and m2 their bytes (the scale is formed anew,
 * with this call's eps).
 * The scaled reward uses the UPDATED scale -- the whole rollout is divided by the standard deviation that already includes the rollout's
 * own samples, as VecNormalize updates first and then normalises:
 *   scaled[t][r] = clamp(reward[t][r] * (float)scale, -clip, clip)     (clip <= 0: no clamp);   0 for a row that did not act
 * The rewards are scaled, not centred.
 * mode & PGD_RN_FREEZE (evaluation): carry and record are read and not written; only `scaled` is produced, from the scale that stands in
 * the record.
 * Deterministic: no atomics; a row's samples are summed in the order of t, the rows of a wave, the waves' partials and the record in a
 * fixed order: the same inputs give the same bytes.  Scratch is the caller's: d_work, 8-byte aligned, work_bytes >=
 * pgd_return_norm_work_bytes(rows) (three doubles per 64 rows; 0 for rows < 1).  Nothing is allocated inside the call: three launches (a
 * row scan, one workgroup that merges the partials and writes the record, an elementwise scaling; PGD_RN_FREEZE: the last alone),
 * asynchronous on the engine's stream, capturable in a HIP graph from the first call; a replay continues from the carry and the record
 * it finds.  T >= 1, rows >= 1, 0 <= gamma <= 1, eps >= 0, no other mode bit, every pointer but d_flags set, d_record and d_work 8-byte
 * aligned, work_bytes as above (PGD_ERR_ARG otherwise, before anything is launched). */
#define PGD_RN_FREEZE 1u
size_t pgd_return_norm_work_bytes(int rows);
int pgd_return_norm(pgd_handle h, const float* d_reward /*[T][rows]*/, const uint8_t* d_done, const uint32_t* d_flags /* or null */, int T,
                    int rows, float gamma, double eps, float clip, uint32_t mode, float* d_carry /*[rows], in/out*/,
                    double* d_record /*[4], in/out*/, float* d_scaled /*[T][rows]*/, void* d_work, size_t work_bytes);
/* ---- Episode statistics of a rollout (every engine) ------------------------------------------------------------------------------------
 * (No reference counterpart: the reference reports an episode in the info dict of the step that ends it; this is gym's
 * RecordEpisodeStatistics -- return, length and the causes of the end of every episode that finished -- as one call over a rollout.)
 * Time-major device arrays, as pgd_step wrote them: reward (float), done (uint8), flags (uint32) [T][rows]; flags is REQUIRED in both
 * modes: the causes are read from it.  Two caller-owned carries per row live across calls and hold a row's unfinished episode:
 *   ret_carry [rows] float, len_carry [rows] int32; zero before the first call
 * Per row r, with R = ret_carry[r], L = len_carry[r], for t = 0 .. T - 1 in order, f = flags[t][r], d = done[t][r]:
 *   mode 0 (single-agent rows):  acted = true;  ends = d != 0
 *   mode PGD_EP_SEATS:           acted = f & PGD_F_REPORT;  cont = acted && !d && !(f & PGD_F_RESET);  ends = acted && !cont
 *                                (the predicates of pgd_gae_masked, above)
 *   acted:  R = R + reward[t][r] (ONE plain fp32 add, in the order of t, contracted with nothing);  L = L + 1
 *   ends:   the episode (R, L, f, d) is a SAMPLE (below);  then R = 0, L = 0
 * and ret_carry[r] = R, len_carry[r] = L behind the loop.  acted and ends SELECT: the reward of a row that did not act may be NaN and
 * reaches nothing.  A sample feeds
 *   count, mean and m2 (the sum of squared deviations) of the returns, in double;  the least and the greatest return;
 *   the sum and the maximum of the lengths;
 *   one count per bit of PGD_F_ARRIVE, OUT_OF_ROAD, CRASH_VEHICLE, CRASH_OBJECT, CRASH_BUILDING, MAX_STEP set in f -- bit counts, not
 *   exclusive classes: they report what the step reported, no more;
 *   `cut`: the ends with d == 0 (an env-wide restart took the agent out: PGD_EP_SEATS only).
 * `steps` counts the entries with acted.  A record is 16 doubles (the counts are integers held in doubles: exact), 8-byte aligned:
 *   0 episodes  1 return_mean  2 return_m2  3 return_min  4 return_max  5 length_sum  6 length_max  7 arrive  8 out_of_road
 *   9 crash_vehicle  10 crash_object  11 crash_building  12 max_step  13 cut  14 steps  15 calls
 * and starts as all zero but return_min = +inf, return_max = -inf.  Two record outputs, either may be null:
 *   d_call    WRITTEN: this call's own statistics, calls = 1
 *   d_record  read and written: the call merged into what the record held (Chan's update of mean and m2 as for pgd_return_norm, min,
 *             max, sums).  A call in which no episode ended adds to steps and calls and leaves slots 0 .. 13 their bytes.
 * Dense outputs, either may be null: ep_return (float) and ep_length (int32) [T][rows] hold (R, L) of the finished episode at the entry
 * where it ended and 0 at EVERY other entry (every entry is written: SB3's info["episode"] as arrays).
 * Deterministic: no atomics; a row's samples are summed in the order of t, the rows of a wave, the waves' partials and the record in a
 * fixed order: the same inputs give the same bytes.  Scratch is the caller's: d_work, 8-byte aligned, work_bytes >=
 * pgd_rollout_episodes_work_bytes(rows) (16 doubles per 64 rows; 0 for rows < 1).  Nothing is allocated inside the call: two launches (a
 * row scan; one workgroup that merges the partials and writes the records -- left out when d_record and d_call are both null),
 * asynchronous on the engine's stream, capturable in a HIP graph from the first call; a replay continues from the carries and the record
 * it finds.  T >= 1, rows >= 1, no other mode bit, every pointer but d_record, d_call, d_ep_return, d_ep_length set, records and d_work
 * 8-byte aligned, work_bytes as above (PGD_ERR_ARG otherwise, before anything is launched). */
#define PGD_EP_SEATS 1u
size_t pgd_rollout_episodes_work_bytes(int rows);
int pgd_rollout_episodes(pgd_handle h, const float* d_reward /*[T][rows]*/, const uint8_t* d_done, const uint32_t* d_flags, int T, int rows,
                         uint32_t mode, float* d_ret_carry /*[rows], in/out*/, int32_t* d_len_carry /*[rows], in/out*/,
                         double* d_record /*[16] in/out, or null*/, double* d_call /*[16] or null*/, float* d_ep_return /*[T][rows] or null*/,
                         int32_t* d_ep_length /*[T][rows] or null*/, void* d_work, size_t work_bytes);
/* ---- Observation normalisation, fused into the training kernels' row loads (every engine) -----------------------------------------------
 * (No reference counterpart: the reference hands its observations to an RL library; this is the norm_obs half of Stable-Baselines3's
 * VecNormalize -- a running mean and variance per observation column, the networks fed clip((obs - mean) / sqrt(var + eps)) -- without a
 * normalised copy of the rollout: the kernels that read observation rows normalise them as they load them.)
 * Two caller-owned device objects:
 *   record  1 + 2 in_dim doubles, 8-byte aligned: slot 0 = n, the number of samples folded; slots 1 .. in_dim the column means; slots
 *           1 + in_dim .. 2 in_dim the column sums of squared deviations m2.  All zero before the first fold.  There is NO phantom initial
 *           count as in SB3's RunningMeanStd (mean 0, variance 1, count 1e-4): an empty record is the identity, the first rollout runs on raw
 *           observations, and the statistics are those of the samples alone.
 *   table   what the kernels read: float [2][Dp], 16-byte aligned, Dp = (in_dim + 3) & ~3; row 0 `shift`, row 1 `scale`:
 *             shift[k] = (float) mean[k];   scale[k] = (float)(1 / sqrt(m2[k] / n + eps))
 *           the quotient and the square root formed in double and rounded to fp32 once; the variance is the population variance.  n == 0:
 *           the identity (shift 0, scale 1).  The padding entries in_dim .. Dp - 1 are always the identity.
 * The normalised input of a live row and a column k < in_dim:
 *   y = min(max((x - shift[k]) * scale[k], -clip), clip)       an fp32 subtraction, then an fp32 multiplication, never contracted into an fma
 * Padding columns and rows past the end (of the range, of the list, behind a mask) stay exactly 0 in the kernels' tiles, as without a
 * table: they are not normalised (a column of zeros would otherwise enter layer 1 as -shift * scale).
 *
 * pgd_obs_norm_update folds the first in_dim floats of every listed row of the row-major array d_obs [n_rows][obs_stride] into the record.
 * The list is that of pgd_adv_stats / pgd_ppo_grad: position q < count is row d_index[q] (null: q itself; an entry outside [0, n_rows) is
 * clamped, never followed); d_count is a device int32 held within [0, n_list] (null: n_list) that the host never reads.  Rows that are
 * not listed may hold NaN: they are never read, nothing is multiplied by zero.  Per column, in double: partitions of 512 list positions
 * (K = the partition's first sample, s1 = sum (x - K), s2 = sum (x - K)^2 in list order; mean = K + s1 / n, m2 = max(s2 - s1 (s1 / n), 0)),
 * the partitions merged in partition order by Chan's update (as for pgd_return_norm), the call's statistic then merged into the record.
 * No atomics: the same inputs give the same bytes.  A call with no live position leaves every byte of the record.  Scratch is the caller's:
 * d_work, 8-byte aligned, work_bytes >= pgd_obs_norm_work_bytes(in_dim, n_list) (two doubles, and 2 in_dim doubles per 512 positions; 0
 * for arguments the call would refuse).  Nothing is allocated inside: two launches, asynchronous on the engine's stream, capturable in a
 * HIP graph from the first call of a fresh engine.  4 <= in_dim <= 416, obs_stride >= in_dim, n_rows >= 1, n_list >= 1 (without an index
 * n_list <= n_rows), the pointers set and aligned, work_bytes as above (PGD_ERR_ARG otherwise, before anything is launched).
 *
 * pgd_obs_norm_publish: record -> table as defined above, one small launch; eps >= 0.
 *
 * pgd_obs_norm_bind is engine state in the manner of pgd_actor_critic_tick.  While a table is bound, every later launch of
 *   pgd_mlp_actor_critic, pgd_mlp_actor_critic_rows, pgd_mlp_actor_critic_cost, pgd_mlp_terminal_value, pgd_ppo_grad, pgd_ppo_grad_cost
 * normalises the observation rows as it loads them (pgd_ppo_grad* in both places that read them: the forward tile and the gather of
 * dW1); every output is what the unbound call gives on an array normalised beforehand by the rule above, bit for bit.  The kernels read
 * the table when they RUN: a captured graph that is replayed sees what a later pgd_obs_norm_publish wrote.  A call whose in_dim differs
 * from the bound one is refused (PGD_ERR_ARG).  clip > 0, +inf allowed.  d_table null (the default, and the state after pgd_create)
 * unbinds: the launches are then the instantiations of before, without an added instruction.  pgd_mlp_policy and
 * pgd_mlp_policy_prepared IGNORE the binding and their code objects stay what they are: a deployed policy normalises its input itself.
 * Not served: statistics are per engine (the ranks of a multi-GPU run do not exchange them); image observations. */
size_t pgd_obs_norm_work_bytes(int in_dim, int n_list);
int pgd_obs_norm_update(pgd_handle h, const float* d_obs /*[n_rows][obs_stride]*/, int obs_stride, int in_dim, int n_rows,
                        const int32_t* d_index /* or null */, const int32_t* d_count /* device, or null */, int n_list,
                        double* d_record /*[1 + 2 in_dim], in/out*/, void* d_work, size_t work_bytes);
int pgd_obs_norm_publish(pgd_handle h, const double* d_record, int in_dim, double eps, float* d_table /*[2][Dp]*/);
int pgd_obs_norm_bind(pgd_handle h, const float* d_table /* or null */, int in_dim, float clip);
/* Multi-agent engines remember, per env, which rows of the LAST observation buffer they were given already hold the zeros of a seat
 * that is not due (identified by the buffer's address and row stride), and do not write them again.  A caller that hands pgd_step
 * a buffer whose address a FORMER buffer had (a caching allocator re-using a freed block: torch.empty per step) calls this first:
 * every row that is not due is then written once more.  Asynchronous on the engine's stream.  pgdrive_amd.Engine.step(out=...) calls
 * it whenever `out` is a tensor it has not seen alive.  (No reference counterpart: the reference returns fresh numpy arrays,
 * base_env.py:303-344.) */
int pgd_forget_rows(pgd_handle h);
/* Identity of the binary: sha256 (16 hex digits) over the sources it was compiled from, written in by pgdrive_amd/build.py
 * ("unstamped" for any other build).  Profile summaries under profiles/ carry the same stamp; bench.py quotes a counter pass only
 * when the stamps agree.  (No reference counterpart: the reference ships no native binary on this path.) */
const char* pgd_source_sha(void);

/* The plan of a handle's table arena: the read-only tables of an engine (maps, lanes, grid cells, scenarios, spawn records, reset images,
 * beam directions) live in one device allocation and are addressed by the kernels as its base + an UNSIGNED 32-bit byte offset.
 * bytes[n]: the tables' sizes, in their order.  offsets[n] receives each table's byte offset (256-byte aligned, in that order, the first
 * behind 4 KiB of padding), *total the arena's size.  PGD_ERR_ARG when the arena would exceed 4 GiB - 64 KiB: an offset plus an index inside a table must
 * not wrap.  Pure arithmetic: nothing is allocated, no GPU is touched (the uploads call it; exported for the tests).
 * (No reference counterpart: the reference keeps its maps in Python objects.) */
int pgd_plan_arena(const uint64_t* bytes, int n, uint32_t* offsets, uint64_t* total);

/* Top-down (bird's-eye) multi-channel observation: TopDownMultiChannel.observe (obs/top_down_obs_multi_channel.py:18-280) of
 * TopDownPGDriveEnv (envs/top_down_env.py:28-42) as a rasteriser kernel.  Image [N, R, R, 2 + frame_stack] float32 in [0, 1]:
 * channel 0 road network (lane lines, route lanes), 1 past ego positions, 2.. the other vehicles now and frame_skip, 2 *
 * frame_skip ... steps ago, the ego at the centre heading up, +-distance metres.  pgd_observe_topdown is called ONCE after
 * every pgd_step (and after pgd_reset): it appends the present state to the per-env history it draws the older frames from.
 * Single-agent engines only, like the reference.  Exact definition: pgdrive_amd/csrc/pgd_topdown.h. */
typedef struct pgd_topdown_config {
  int32_t resolution;       /* R: 84 (top_down_env.py:19) */
  float distance;           /* 30 m */
  int32_t frame_stack;      /* 3 traffic frames */
  int32_t post_stack;       /* 5 past positions */
  int32_t frame_skip;       /* 5 steps between stacked entries */
  int32_t mode;             /* 0: TopDownMultiChannel [R, R, 2 + frame_stack] (TopDownPGDriveEnv / V2, top_down_env.py:28-60);
                               1: TopDownObservation, one RGB frame [R, R, 3] / 255 -- lane lines (35, 35, 35), the ego GREEN
                               (50, 200, 0), the other vehicles BLUE (100, 200, 255) (TopDownSingleFramePGDriveEnv,
                               top_down_env.py:8-26, obs/top_down_obs.py:22-240; the stack / skip fields are not read) */
} pgd_topdown_config;
int pgd_topdown_channels(const pgd_topdown_config* cfg);
int pgd_topdown_enable(pgd_handle h, const pgd_topdown_config* cfg);
int pgd_observe_topdown(pgd_handle h, float* d_img /*[N,R,R,C]*/);
/* The same image as bytes in [0, 255]: the reference's `rgb_clip=False` (pgdrive_env.py:133-141; top_down_obs_multi_channel.py:208-211,
 * 253-256, 277-280 return the uint8 pygame values instead of float32 / 255).  byte = (int)(float value x 255): (line texels x 35 + route
 * texels x 64) / 2 of the pixel's 2 x 2 cell on the road channel, 255 at a past position, 176 inside a vehicle box; RGB frame: lines 35,
 * the ego (50, 200, 0), the others (100, 200, 255).  A quarter of the bytes of the float image (a write-bound kernel: DESIGN.md
 * section 14).  `d_img` 16-byte aligned.  One call advances the pose history like pgd_observe_topdown: call ONE of the two per step. */
int pgd_observe_topdown_u8(pgd_handle h, uint8_t* d_img /*[N,R,R,C]*/);

/* Top-down scene rendering: env.render(mode="top_down") (envs/base_env.py:240-248, 463-468) -> TopDownRenderer
 * (obs/top_down_renderer.py) as kernels over the state on the device, the frames of many envs in one launch.  Each env's whole map
 * on a film_w x film_h RGB film: lane lines on a light background, every controlled agent as a box in its own colour with a fading
 * trail of its last num_stack rendered frames, the newest frame outlined, a red disk where an agent finished.  Frames [n][H][W][3]
 * uint8 (pygame.surfarray.array3d of the reference's Surface is [W][H][3]: the same image transposed (1, 0, 2)).  pygame's
 * rasterisation is unpinned; the exact definition, the film geometry and the deviations (trails and deads cleared at an env's reset,
 * dead list capped at 256, colours from a counter hash, broken lines by the map's boxes, analytic pixel rules):
 * pgdrive_amd/csrc/pgd_render.h.  Works in every engine mode (one or several envs per wave, throughput mode, multi-agent). */
typedef struct pgd_render_config {
  int32_t film_w, film_h;   /* film_size (top_down_renderer.py:128): 1000 x 1000; each in 16 .. 16384 */
  int32_t num_stack;        /* 15: rendered frames kept per env (1 .. 64; num_stack * V + 256 <= 2048) */
  int32_t history_smooth;   /* 0: every kept frame is painted; k > 0: only frames whose age i (1 = newest) is a multiple of k */
  int32_t light_background; /* 1: the background inverted (255 - x): black lines on white (the reference's default) */
  int32_t road_rgb[3];      /* road_color (255, 255, 255): the lane lines before the inversion */
  int32_t draw_traffic;     /* 0: controlled agents only (the reference).  1 (NOT a reference option): also the IDM traffic in
                               (100, 200, 255) and the traffic objects in (200, 0, 150), VehicleGraphics.BLUE / PURPLE */
} pgd_render_config;
/* The agent colours: seaborn's "colorblind" palette (seaborn/palettes.py SEABORN_PALETTES, the table base_vehicle.py:151-155
 * draws `top_down_color` from) as 8-bit values.  Agent k of env e gets entry pgd_rng(seed, env_base + e, 0x7e4d0c01, k) % 10 (the
 * counter hash of the device RNG streams), for life. */
#define PGD_RENDER_PALETTE                                                                                                    \
  {{1, 115, 178}, {222, 143, 5}, {2, 158, 115}, {213, 94, 0}, {204, 120, 188}, {202, 145, 97}, {251, 175, 228}, {148, 148, 148}, \
   {236, 225, 51}, {86, 180, 233}}
/* h_film_geom: HOST [n_maps][3] doubles (scaling [px / m], ox, oy [m]) per uploaded map, the film transform of the map's
 * RoadNetwork.get_bounding_box() (pgdrive_amd/render.py computes it from the lane descriptions).  Draws every map's background once,
 * allocates the per-env history, synchronises the engine stream.  An upload of maps or scenarios afterwards requires a new enable. */
int pgd_render_enable(pgd_handle h, const pgd_render_config* cfg, const double* h_film_geom);
/* Appends the present state of the listed envs (h_env_ids HOST, NULL = all N, in order; no env twice) to their histories and
 * draws their frames into d_frames [n][film_h][film_w][3] (16-byte aligned).  Asynchronous on the engine stream, like pgd_reset: not
 * ordered against the streams of env groups.  Only the rendered envs advance their history. */
int pgd_render_topdown(pgd_handle h, const int32_t* h_env_ids, int n, uint8_t* d_frames);
int pgd_render_palette(uint8_t* out /* [10][3] */);

/* Step info on the device: what the reference returns in the `info` dict of env.step (base_env.py:303-344) and what a trainer needs of
 * a finished episode, written by one more kernel (k_step_info, pgdrive_amd/csrc/pgd_step_info.h) right after the step kernel on the
 * same stream.  OPT-IN; single-agent engines only (PGD_ERR_ARG on a multi-agent engine: its terminal rows survive the step anyway).
 * While it is enabled the step kernel itself never restarts an env: the step leaves the state the episode ended in and its row in
 * d_obs, and k_step_info, per env and from memory,
 *   1. writes the info values of that state (every env, every step),
 *   2. where done: copies the row to final_obs (SB3's terminal_observation, gymnasium's final_observation),
 *   3. where done: adds the episode to the per-env statistics,
 *   4. where done and pgd_config.auto_reset: restarts the env exactly as the step kernel would have -- the same re-drawn scenario, the
 *      same reset image, counters and hints -- writes the first row of the new episode into d_obs and sets PGD_F_RESET.
 * State, reward, done, flags and the rows of envs that did not restart are bit-identical to those of an engine without step info; the
 * row of a restarted env comes from the stand-alone row code (as after pgd_reset) instead of the fused one: equal to rounding.
 * No host synchronisation, no allocation: a step with info is two launches in sequence and can be captured in a HIP graph.
 * Every pointer is a caller-owned DEVICE array that must stay valid while the info is enabled; NULL = not written.
 * Not provided: `step_reward` (pgdrive_env.py:248, the shaping reward before the terminal override): it needs the lane formulas of the
 * reward function, which live in the step kernel only.
 * pgd_step, pgd_step_group (on the group's stream, over the group's envs) and pgd_step_lane_keep are supported; pgd_step_n and
 * pgd_step_packed return PGD_ERR_STATE while the info is enabled (terminal rows through the multi-GPU gather: not built).  pgd_reset
 * clears total_cost and the base of step_energy of the envs it resets, pgd_set_state leaves them.  Enabling or disabling unloads a
 * run-time step kernel (pgd_set_step_module): it has auto_reset compiled in; build it again afterwards (Engine.specialise does). */
typedef struct pgd_step_info {
  float out_of_road_cost, crash_vehicle_cost, crash_object_cost;  /* pgdrive_env.py:105-107, 197-207 */
  int32_t pad;
  float* final_obs;         /* [N, D]: the row of the state the episode ended in; written only where done (base_env.py:303-344 returns
                               it as the step's observation; the auto-reset replaces it in d_obs) */
  float* velocity;          /* [N] |SF_SPEED| * 3.6 [km/h]                    base_vehicle.py:265, 394-401 */
  float* steering;          /* [N] SF_STEER                                   base_vehicle.py:266 */
  float* acceleration;      /* [N] SF_ACT1T (throttle_brake)                  base_vehicle.py:267 */
  float* episode_energy;    /* [N] SF_ENERGY                                  base_vehicle.py:269, 289-290 */
  float* step_energy;       /* [N] episode_energy - the previous step's (0 at the start of an episode)  base_vehicle.py:268, 286-288 */
  float* episode_reward;    /* [N] SF_EP_REWARD                               base_env.py:336-337 */
  int32_t* episode_length;  /* [N] EI_EP_STEPS                                base_env.py:338-339 */
  float* cost;              /* [N] out_of_road, else crash_vehicle, else crash_object cost, else 0  pgdrive_env.py:197-207 */
  float* total_cost;        /* [N] sum of cost over the running episode      safe_pgdrive_env.py:36-40 */
  /* statistics of the episodes that ended, per env (no atomics: deterministic); the caller reduces them.  No reference counterpart
   * (the reference's trainers accumulate them from the info dicts) */
  int32_t* ep_count;        /* [N] episodes ended */
  float* ep_return_sum;     /* [N] sum of their episode_reward */
  int32_t* ep_length_sum;   /* [N] sum of their episode_length */
  float* ep_cost_sum;       /* [N] sum of their total_cost */
  int32_t* ep_arrive;       /* [N] ended with PGD_F_ARRIVE set */
  int32_t* ep_out_of_road;  /* [N] ... PGD_F_OUT_OF_ROAD */
  int32_t* ep_crash;        /* [N] ... PGD_F_CRASH_VEHICLE, PGD_F_CRASH_OBJECT or PGD_F_CRASH_BUILDING */
  int32_t* ep_max_step;     /* [N] ... PGD_F_MAX_STEP */
} pgd_step_info;
int pgd_step_info_enable(pgd_handle h, const pgd_step_info* info /* NULL: disable */);
/* Zeroes the eight ep_* arrays of the enabled info (asynchronous on the engine's stream). */
int pgd_step_info_clear_stats(pgd_handle h);
/* One empty launch of k_step_info's shape (N workgroups of one wave) on the engine's stream: the launch floor that tools/step_info_ab.py
 * measures beside the plain step and the step with info.  For measurements only; no reference counterpart. */
int pgd_step_info_empty_launch(pgd_handle h);

/* ---------------------------------------------------------------------------------------------------------------------
 * Per-step gather by direct peer writes (multi-GPU, one process per GPU).  The reference has no distributed layer (one env
 * per process, engine_utils.py:8-15); BASELINE.json's north star shards the envs over the GPUs of a node with one gather of
 * (obs, reward, done) per step.  xGMI is point to point, so instead of a ring every rank writes its packed rows (the rows
 * pgd_step_packed produces) into the receive buffers of all peers at once.  Each rank owns `nbuf` receive buffers of
 * [world * n_rows][row_floats] fp32 (rank r's rows at row offset r * n_rows) plus a small flag area, in one device block
 * that peers map over HIP IPC.  Sequence numbers start at 1 and grow by 1 per push; buffer use is round robin.
 *   create  -> export (handle blob, exchanged by the host, e.g. torch.distributed.all_gather_object) -> connect per peer
 *   per step: pgd_step_packed(d_rows = own slice of pgd_gather_buffer(buf)) ; pgd_gather_push(buf, seq)
 *   consumer: pgd_gather_wait(buf, seq) ... read the buffer ... pgd_gather_release(buf, seq)
 * All three are asynchronous on the given stream; a peer that never arrives sets the status word instead of hanging.
 * seq == 0 takes the sequence number from a per-buffer counter on the device (advanced by pgd_gather_release): the calls of a step
 * are then identical every time, and  wait, release, pgd_step_packed, push  of a multiple of nbuf consecutive steps can be captured
 * in one HIP graph (a handle uses either host-counted or device-side sequences, not both). */
#define PGD_GATHER_HANDLE_BYTES 64
typedef struct pgd_gather* pgd_gather_handle;
int pgd_gather_create(int device, int world, int rank, int n_rows, int row_floats, int nbuf, pgd_gather_handle* out);
int pgd_gather_buffer(pgd_gather_handle g, int buf, float** d_recv /* [world*n_rows, row_floats] */);
int pgd_gather_export(pgd_gather_handle g, void* h_handle /* PGD_GATHER_HANDLE_BYTES */);
int pgd_gather_connect(pgd_gather_handle g, int peer, const void* h_handle);
int pgd_gather_push(pgd_gather_handle g, int buf, int seq, void* hip_stream);
int pgd_gather_wait(pgd_gather_handle g, int buf, int seq, void* hip_stream);
int pgd_gather_release(pgd_gather_handle g, int buf, int seq, void* hip_stream);
int pgd_gather_status(pgd_gather_handle g, int* err /* 0 = ok, 1 = an ack never came, 2 = rows never came */);
/* 1: the receive block is fine-grained (device-coherent across agents) memory, as the protocol wants; 0: the runtime refused
 * hipExtMallocWithFlags(..., hipDeviceMallocFinegrained) or PGD_GATHER_COARSE was set and the block is plain hipMalloc memory. */
int pgd_gather_mem_kind(pgd_gather_handle g, int* fine_grained);
int pgd_gather_destroy(pgd_gather_handle g);

#ifdef __cplusplus
}
#endif
#endif
