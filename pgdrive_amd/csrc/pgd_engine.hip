// pgd_engine.hip — kernels + C ABI (include/pgdrive_hip.h) of the MI355X-native batched PGDrive step engine.
//
// Execution model (gfx950, wave64):
//   k_step     one 64-lane wave per block and, whenever V * SUB <= 64 leaves no room for a second one, ONE environment
//              per wave: a vehicle slot is carried by SUB = min(16, 64 / V) consecutive lanes that hold identical register
//              copies of its 128-byte record and split the heavy loops (grid walks, broad phase, neighbour search) between
//              them.  IDM neighbour search, contacts and trigger logic read the env's vehicle snapshot from LDS; map tables
//              (immutable, L2 resident) are read through the per-map 8 m grid.  Policy, 5 x 0.02 s physics, contacts,
//              localisation, line / sidewalk test, reward, done, auto-reset AND the observation row (state + navigation +
//              neighbours + lidar fan) run in this one launch; the stand-alone k_observe serves pgd_reset / pgd_observe,
//              engines with several envs per wave and the multi-agent step.
//   k_observe  one block per (env, agent): wave 0 compacts the bodies inside the lidar broad phase into LDS with a ballot,
//              then every thread casts beams against the compacted bodies and the row is written coalesced.
// The reference call stack this replaces: envs/base_env.py:184-224,303-344.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>
#include <type_traits>

#include "pgd_device.h"

#define HIPCHK(x)                                                                              \
  do {                                                                                         \
    hipError_t _e = (x);                                                                       \
    if (_e != hipSuccess) {                                                                    \
      fprintf(stderr, "[pgdrive_hip] %s failed: %s (%s:%d)\n", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
      return PGD_ERR_HIP;                                                                      \
    }                                                                                          \
  } while (0)

#define WAVE 64
#define MAXV 64

// Optional per-phase cycle counters of k_step (build with -DPGD_PROF; never enabled in the shipped library)
#ifndef PGD_MA_PRIO3
#define PGD_MA_PRIO3 7  // issue priority of a multi-agent env's wave from this many tenths of its slots alive
#define PGD_MA_PRIO2 5
#define PGD_MA_PRIO1 3
#endif
#ifdef PGD_PROF
#define PROF_BLOCKS 8192
__device__ unsigned long long g_phase_cycles[PROF_BLOCKS * 32];  // per block, no atomics (they would serialise)
__shared__ long long s_prof_t0, s_prof_w0;
#define PHASE_MARK(k)                                                                                      \
  do {                                                                                                     \
    if ((int)threadIdx.x == __builtin_ffsll((long long)__ballot(1)) - 1 && blockIdx.x < PROF_BLOCKS) {       \
      long long _now = clock64();                                                                          \
      g_phase_cycles[blockIdx.x * 32 + (k)] += (unsigned long long)(_now - s_prof_t0);                     \
      s_prof_t0 = _now;                                                                                    \
    }                                                                                                      \
  } while (0)
#define PHASE_INIT() do { if (threadIdx.x == 0) { s_prof_t0 = clock64(); s_prof_w0 = wall_clock64(); } } while (0)
#define PHASE_END_AT(k) do { if (threadIdx.x == 0 && blockIdx.x < PROF_BLOCKS) g_phase_cycles[blockIdx.x * 32 + (k)] += (unsigned long long)(wall_clock64() - s_prof_w0); } while (0)
#define PHASE_END() PHASE_END_AT(15)
#elif defined(PGD_EXITAT)
// "exit profile" build (tools/exit_profile.py; never shipped): every wave leaves the kernel at top-level mark d.dbg_exit
// without storing anything, so the launch time up to each point of the step is measured on an unchanging state
#define PHASE_MARK(k)
#define PHASE_INIT()
#define PHASE_END()
#define PHASE_END_AT(k)
#define XMARK(k) do { if ((d.dbg_exit & 0xff) == (k)) return; } while (0)
#define PGD_DBG_SKIP(bit) ((d.dbg_exit >> (8 + (bit))) & 1)  /* timing-only ablations of the IDM policy (tools/idm_ablation.py) */
#else
#define PHASE_MARK(k)
#define PHASE_INIT()
#define PHASE_END()
#define PHASE_END_AT(k)
#endif
#ifndef XMARK
#define XMARK(k)
#endif

#include "pgd_vehicle.h"
#include "pgd_localize.h"
#include "pgd_idm.h"
#include "pgd_dynamics.h"
#include "pgd_observe.h"
#include "pgd_policy.h"

// ---------------------------------------------------------------------------------------------------------------------
// k_step: one env.step() for every environment (base_env.py:184-224)
// lane -> (group g = lane / SUB, sub-lane); group g -> (env-local el = g / V, slot s = g % V)
// ---------------------------------------------------------------------------------------------------------------------
struct LaneMap {
  int sub, lead, el, s, e, idx, base;
  bool valid;
};
DEV LaneMap lane_map(const PgdDev& d, int unit, int n_units) {
  LaneMap m;
  int lane = threadIdx.x;
  int g = lane / d.sub;
  m.sub = lane - g * d.sub;
  m.lead = g * d.sub;
  m.el = g / d.V;
  m.s = g - m.el * d.V;
  m.e = unit * d.epw + m.el;
  m.valid = (m.el < d.epw) && (m.e < n_units);
  m.base = m.el * d.V;
  m.idx = m.e * d.V + m.s;
  return m;
}


#define FUSE_MAX_AGENTS 8
// first 64 bytes of a spawn record (everything but the route arrays) into a local copy; the copy is only ever read by field, so it
// lives in registers and the fields nobody reads cost nothing
template <bool SKIP_POSE> DEV void spawn_head_load(const pgd_spawn* sp, pgd_spawn& out) {
  static_assert(offsetof(pgd_spawn, ckpt) == 64 && sizeof(pgd_spawn) % 16 == 0, "spawn record head = 4 x 16 bytes");
  static_assert(offsetof(pgd_spawn, length) == 12, "the first piece = spawn pose + length");
  const float4* q = reinterpret_cast<const float4*>(sp);
  float4* o = reinterpret_cast<float4*>(&out);
  // (the spawn pose is only read where slots are (re)built from the record in memory -- the image kernels: a step reads the length
  // alone from the first piece; as a whole piece it went through a temporary that the compiler waited for before it issued the
  // last two reads in the kernels that are short of registers)
  // (SKIP_POSE: the multi-agent kernels; the single-agent ones issue the four pieces together as they are)
  if constexpr (SKIP_POSE) {
    const float len = sp->length;
    const float4 b = q[1], c = q[2], e = q[3];
    o[0] = make_float4(0.0f, 0.0f, 0.0f, len); o[1] = b; o[2] = c; o[3] = e;
  } else {
    const float4 a = q[0], b = q[1], c = q[2], e = q[3];
    o[0] = a; o[1] = b; o[2] = c; o[3] = e;
  }
}
template <bool REG> DEV const pgd_lane& dest_lane_ref(const pgd_lane& regs, const pgd_lane* lanes, int id) {
  if constexpr (REG) return regs; else return lanes[id];
}
template <bool REG> DEV const pgd_spawn& spawn_ref(const pgd_spawn& regs, const pgd_spawn* mem) {
  if constexpr (REG) return regs; else return *mem;
}
#ifndef PGD_WAVES_PER_SIMD
#define PGD_WAVES_PER_SIMD 4  // <=128 VGPRs: 4096 envs = 4096 waves are then all resident at once (16 per CU)
#endif
// ONE_ENV (epw == 1: every lane of the wave works on env blockIdx.x) is a compile-time switch: the env index, its
// scenario, the map view (7 table pointers) and the env counters are then wave-uniform and live in SGPRs instead of
// occupying ~20 VGPRs per lane for the whole kernel.
// MARL (multi-agent tail: delay-done, respawn, __all__) is compiled in only for the multi-agent engine.
// OBJ: traffic objects present in some scenario (circle shapes, crash_object bookkeeping).
// STD: the fused observation has the default row layout (see observe_agent).
// LDS of the step proper; the multi-agent engine's fused observation (observe_env_body at the end of k_step) reuses it
struct StepLds {
  Snap S;
  ObsScratch OU;
};
constexpr int STEP_MINB_WORDS = ((int)sizeof(StepLds) - (int)sizeof(ObsEnvLds<1>)) / 4;  // what is left for the per-beam minima
static_assert(STEP_MINB_WORDS >= 8 * 72, "the fused multi-agent observation of 8 agents x 72 beams must fit the step's LDS");
union StepUnion {
  StepLds step;
  struct {
    ObsEnvLds<1> m;
    unsigned minb[STEP_MINB_WORDS];
  } obs;
};

// the per-beam minima of the fused lidar (observe_agent, incidence form) live where the IDM search kept its per-vehicle lane data:
// own-lane coordinate, lane length and successor list are dead once the policies have run
static_assert(offsetof(Snap, llen) == offsetof(Snap, lon) + sizeof(float) * WAVE && offsetof(Snap, succ) == offsetof(Snap, llen) + sizeof(float) * WAVE,
              "lon / llen / succ of the snapshot are one contiguous area");
DEV unsigned* lidar_minb(Snap& S) { return reinterpret_cast<unsigned*>(&S.lon[0]); }  // 6 * WAVE words >= 4 * WAVE beams
// A block of k_step is ONE wave: the lanes only have to see each other's LDS traffic in order, which the hardware guarantees for
// a wave; a workgroup-scope barrier would also wait for every global load and store in flight (release / acquire fences).
DEV void step_sync() { row_sync<true>(); }

// FIX: the engine runs the reference's default single-agent configuration (PGDriveEnv defaults, pgdrive_env.py:22-109: 1 ego + 16
// traffic slots, 240 beams over 50 m, 4 neighbours, 5 x 0.02 s, continuous actions, the default reward scheme).
// The instantiation writes those values over its copy of the kernel argument: every read of such a field folds to a
// constant (loop bounds, row offsets, divisors, dead branches) instead of being fetched from the kernel-argument segment at each
// use -- the scalar registers are full, and a fetch right before its use costs its whole latency (profiles/r03_notes.md).
// pgd_step picks the instantiation only when fix_config_matches() holds, so its results are those of the general kernel.
#define PGD_FIX_V 17
// The single-agent instantiations differ in a handful of values: what varies lives in a FixSpec, one per FIX number (round 6: the
// configurations the shipped env classes produce no longer fall back to the general kernel, 12 % behind -- VERDICT r05 item 3).
//   FIX 1  PGDriveEnv defaults (pgdrive_env.py:22-109), default reward scheme folded
//   FIX 2  the same geometry, reward scheme read at run time
//   FIX 3  the top-down envs (envs/top_down_env.py:8-72: "Remove lidar" -- no beams, no neighbour block: the row = the 18 state floats), default reward
//   FIX 4  SafePGDriveEnv (envs/safe_pgdrive_env.py:9-26): 16 traffic + 40 object slots, one lane per slot, crashes are costs
//          (safe_rl_env), reward scheme at run time (cost_to_reward moves the penalties)
struct FixSpec {
  int V, lasers, others, D, safe;
  bool reward;   // the default reward scheme is folded as well
  bool lidar50;  // the lidar reaches 50 m (folded only where there is a lidar)
};
constexpr FixSpec fix_spec(int fix) {
  // (lidar off: LidarStateObservation leaves out the neighbour block with the cloud, state_obs.py:124-130 -- the row is the 18 state floats)
  return fix == 3 ? FixSpec{PGD_FIX_V, 0, 0, 18, 0, true, false}
         : fix == 4 ? FixSpec{1 + 16 + 40, 240, 4, 274, 1, false, true}
         : FixSpec{PGD_FIX_V, 240, 4, 274, 0, fix == 1, true};
}
// one list for the device (assignment) and the host (test): F(field, value)
#define PGD_FIX_FIELDS(F, d, c, one_env, SP)                                                                                        \
  F(d.V, SP.V) F(d.A, 1) F(d.T, SP.V - 1) F(d.D, SP.D) F(d.sstride, SP.V) F(d.use_imask, (one_env ? 0 : 1))                      \
  F(d.sub, (one_env ? WAVE / SP.V : 1)) F(d.epw, (one_env ? 1 : WAVE / SP.V)) F(d.pack_obs, (one_env ? 0 : 1))             \
  F(c.num_agents, 1) F(c.num_traffic, SP.V - 1) F(c.num_lasers, SP.lasers) F(c.num_others, SP.others)                                     \
  F(c.dt, 0.02f) F(c.decision_repeat, 5) F(c.discrete_action, 0) F(c.increment_steering, 0) F(c.safe_rl_env, SP.safe)               \
  F(c.enable_reverse, 0) F(c.marl_flags, 0) F(c.side_lasers, 0) F(c.lane_line_lasers, 0)                                            \
  F(c.random_agent_model, 0) F(c.lidar_gaussian_noise, 0.0f) F(c.lidar_dropout_prob, 0.0f) F(c.idm_agent, 0)              \
  F(c.idm_steer_lag, 0.0f)
#define PGD_FIX_LIDAR_FIELDS(F, c) F(c.lidar_dist, 50.0f)
#define PGD_FIX_REWARD_FIELDS(F, c)                                                                                                 \
  F(c.use_lateral, 0) F(c.out_of_route_done, 0) F(c.success_reward, 10.0f) F(c.out_of_road_penalty, 5.0f)                           \
  F(c.crash_vehicle_penalty, 5.0f) F(c.crash_object_penalty, 5.0f) F(c.driving_reward, 1.0f) F(c.speed_reward, 0.1f)
// Multi-agent engines: the scalar fields of MULTI_AGENT_PGDRIVE_DEFAULT_CONFIG (multi_agent_pgdrive.py:12-55: a 40 m lidar without
// neighbour rows, penalties 10, delay-done 25 steps, crash / out-of-road done, respawn; the roundabout / intersection / bottleneck
// envs run it unchanged) -- the number of agents, the spawn places, the horizon AND the number of beams stay run-time values (the
// reference's 72 beams and BASELINE config 5's 240 run the same instantiation: as a constant the beam count gave the 72-beam row
// 0.8 % and cost the 240-beam row 6 %, which then fell back to the general kernel).
#define PGD_FIXM_FIELDS(F, d, c)                                                                                                    \
  F(d.T, 0) F(d.epw, 1) F(d.pack_obs, 0) F(d.no_groups, 1) F(d.use_imask, 0)                                              \
  F(c.num_traffic, 0) F(c.num_others, 0) F(c.lidar_dist, 40.0f) F(c.dt, 0.02f) F(c.decision_repeat, 5)          \
  F(c.discrete_action, 0) F(c.increment_steering, 0) F(c.safe_rl_env, 0) F(c.enable_reverse, 0)                                     \
  F(c.marl_flags, (PGD_MA_ENABLED | PGD_MA_CRASH_DONE | PGD_MA_OUT_ROAD_DONE | PGD_MA_ALLOW_RESPAWN)) F(c.use_lateral, 0)           \
  F(c.out_of_route_done, 0) F(c.success_reward, 10.0f) F(c.out_of_road_penalty, 10.0f) F(c.crash_vehicle_penalty, 10.0f)            \
  F(c.crash_object_penalty, 10.0f) F(c.driving_reward, 1.0f) F(c.speed_reward, 0.1f) F(c.side_lasers, 0) F(c.lane_line_lasers, 0)   \
  F(c.random_agent_model, 0) F(c.lidar_gaussian_noise, 0.0f) F(c.lidar_dropout_prob, 0.0f) F(c.delay_done, 25) F(c.idm_agent, 0)   \
  F(c.idm_steer_lag, 0.0f)
// ... and, on top of that list, the engine's SEAT COUNT for the two geometries the reference's default agent counts produce here:
// 40 seats (MultiAgentRoundaboutEnv's 40 agents, marl_inout_roundabout.py:26: the vec env and bench.py's c5_40x72 row) and 44 (the
// dict-keyed envs keep spare seats: pgdrive_amd/marl_env.py) with the reference's 72 beams (multi_agent_pgdrive.py:38) -- and the 8 seats of
// BASELINE.json's multi-agent configuration ("4096 envs x 8 controlled agents, multi-agent roundabout"), with the 72 beams of the
// multi-agent default and with the 240 of the metric (bench.py's c5_8x72 / c5_8x240 rows).  FIX = seats x 1000 + beams.  With V, A, the lanes per seat, the row width and the beam count literals the 40-seat step runs at 115 registers instead of
// 128 and 23 scalar spills instead of 77: k_step 28.4 -> 26.3 us, k_observe_env 30.2 -> 29.5 us (64 registers), the row 76.8 -> 81.1 M
// (round 6, profiles/r06_notes.md).  The respawn table's shape and the horizon stay run-time values (they differ between the maps).
#define PGD_FIXM_SEAT_FIELDS(F, d, c, S, NL) F(d.V, S) F(d.A, S) F(d.sub, (WAVE / (S))) F(d.D, (18 + (NL))) F(c.num_agents, S) F(c.num_lasers, NL)
// BASELINE config 2: the ego alone, no lidar (dynamics + reward + the 18-float state vector), otherwise the single-agent defaults --
// four envs per wave, 16 sub-lanes per ego, the row written by k_step itself.
#define PGD_FIXE_FIELDS(F, d, c)                                                                                                    \
  F(d.V, 1) F(d.A, 1) F(d.T, 0) F(d.D, 18) F(d.sstride, 1) F(d.sub, 16) F(d.epw, 4) F(d.pack_obs, 0) F(d.no_groups, 1)               \
  F(c.num_agents, 1) F(c.num_traffic, 0) F(c.num_lasers, 0) F(c.num_others, 0) F(c.dt, 0.02f) F(c.decision_repeat, 5)                \
  F(c.discrete_action, 0) F(c.increment_steering, 0) F(c.safe_rl_env, 0) F(c.enable_reverse, 0) F(c.marl_flags, 0)                  \
  F(c.use_lateral, 0) F(c.out_of_route_done, 0) F(c.success_reward, 10.0f) F(c.out_of_road_penalty, 5.0f)                           \
  F(c.crash_vehicle_penalty, 5.0f) F(c.crash_object_penalty, 5.0f) F(c.driving_reward, 1.0f) F(c.speed_reward, 0.1f)               \
  F(c.side_lasers, 0) F(c.lane_line_lasers, 0) F(c.random_agent_model, 0) F(c.idm_agent, 0) F(c.idm_steer_lag, 0.0f)
enum { FIXK_DEFAULT = 0, FIXK_MARL = 1, FIXK_EGO_ONLY = 2, FIXK_GEOMETRY = 3, FIXK_NO_LIDAR = 4, FIXK_SAFE = 5 };
constexpr int fix_of_kind(int kind) { return kind == FIXK_GEOMETRY ? 2 : kind == FIXK_NO_LIDAR ? 3 : kind == FIXK_SAFE ? 4 : 1; }
template <bool ONE_ENV, bool MARL, bool STD, int FIX = 1>
DEV void write_fixed_config(PgdDev& d) {
  pgd_config& c = d.cfg;
#define PGD_F_SET(f, v) f = v;
  if (MARL) {
    PGD_FIXM_FIELDS(PGD_F_SET, d, c)
    if (FIX >= 1000) { PGD_FIXM_SEAT_FIELDS(PGD_F_SET, d, c, (FIX >= 1000 ? FIX / 1000 : WAVE), (FIX % 1000)) }
  }
  else if (!ONE_ENV && !STD) { PGD_FIXE_FIELDS(PGD_F_SET, d, c) }
#ifdef PGD_JIT
  // FIX 9: a code object built at run time for ONE handle (pgdrive_amd/jit.py, pgd_set_step_module): every immutable field of its
  // configuration and geometry is a literal of the generated header (PGD_JIT_FIELDS) -- what the AOT instantiations do for the
  // configurations of the reference's env classes, for any configuration (the JIT alternative)
  else if (FIX == 9) { PGD_JIT_FIELDS(PGD_F_SET, d, c) }
#endif
  else {
    constexpr FixSpec SP = fix_spec(FIX);
    PGD_FIX_FIELDS(PGD_F_SET, d, c, ONE_ENV, SP)
    if (SP.lidar50) { PGD_FIX_LIDAR_FIELDS(PGD_F_SET, c) }
    if (SP.reward) { PGD_FIX_REWARD_FIELDS(PGD_F_SET, c) }
  }
#undef PGD_F_SET
}
static bool fix_config_matches(const PgdDev& d, bool one_env, int kind = FIXK_DEFAULT) {
  const pgd_config& c = d.cfg;
  bool ok = true;
#define PGD_F_TEST(f, v) ok = ok && (f == v);
  if (kind == FIXK_MARL) { PGD_FIXM_FIELDS(PGD_F_TEST, d, c) }
  else if (kind == FIXK_EGO_ONLY) { PGD_FIXE_FIELDS(PGD_F_TEST, d, c) }
  else {
    const FixSpec SP = fix_spec(fix_of_kind(kind));
    PGD_FIX_FIELDS(PGD_F_TEST, d, c, one_env, SP)
    if (SP.lidar50) { PGD_FIX_LIDAR_FIELDS(PGD_F_TEST, c) }
    if (SP.reward) { PGD_FIX_REWARD_FIELDS(PGD_F_TEST, c) }
  }
#undef PGD_F_TEST
  return ok;
}
// What only the rare paths of a step read (an env restarting, a multi-agent respawn): a second by-value argument that is never
// written, so its fields are fetched from the argument segment where they are used -- in the specialised kernels `d` is a local
// copy whose every used field is an entry load and stays live in a scalar register (or a spill lane) to the end.
struct PgdCold {
  const pgd_map* scen_map;
  uint8_t* bev_fill;
  const float2* spawn_hv;
  const RecPiece* respawn_img;
  int n_scen;
  uint32_t seed;
  int env_base;
  // pgd_step_lane_keep: the scripted lane-keeping policy evaluated by k_step itself, from the observation row the PREVIOUS step wrote
  // (null: the actions come from the caller's buffer).  One launch per closed-loop step instead of two (k_lane_keep was 4.9 us of a
  // 23.5 us iteration: the launch floor of a 16-block kernel, profiles/r06_expert_kernel_stats.csv).  Here, not in PgdDev: these
  // fields are read once, at the head of the kernel, and must not cost the specialised kernels scalar registers for the whole step.
  const float* lk_obs;
  float lk_klat, lk_khead, lk_vt, lk_noise;
  uint32_t lk_tick;
};
// LK: the scripted lane-keeping policy inside the step (pgd_step_lane_keep): an instantiation of its own -- as a run-time branch at
// the head of every kernel it cost the metric's row 0.09 us (17.03 -> 17.12)
template <bool ONE_ENV, bool MARL, bool OBJ, bool STD = false, int FIX = 0, bool LK = false>
__global__ __launch_bounds__(WAVE, PGD_WAVES_PER_SIMD) void k_step(PgdDev d, const float* __restrict__ act, float* __restrict__ reward,
                                                uint8_t* __restrict__ done, uint32_t* __restrict__ flags,
                                                float* __restrict__ obs, const PgdCold cold) {
  if (FIX) write_fixed_config<ONE_ENV, MARL, STD, FIX>(d);

  __shared__ StepUnion U;
  Snap& S = U.step.S;
  ObsScratch& OU = U.step.OU;  // sub-step poses (contact test), then the observation's compaction scratch
  ObsLds& OL = OU.ol;
  SubPose& SUBP = OU.sp;
  __shared__ AgentView s_ag[FUSE_MAX_AGENTS];
  __shared__ int s_flag[WAVE];
  __shared__ int s_hit[WAVE];  // per snapshot slot: an agent's chassis overlaps another vehicle
  __shared__ int s_aux;        // multi-agent parking lot: pool of free parking spaces (bit mask)
  __shared__ uint8_t s_kind[WAVE]; // PGD_OBJ_* of every slot (fused observation: objects are lidar targets, not neighbours)
  const int V = d.V, A = d.A, N = d.N;
  const int lane = threadIdx.x;
  const bool sub_ok = (ONE_ENV ? V : d.epw * V) <= PGD_SUBV;  // every slot of the wave has a place for its sub-step poses
  const int unit = (int)blockIdx.x + d.unit_off;  // pgd_step_group launches only the blocks of one env group
  const LaneMap lm = lane_map(d, unit, N);
  const int el = ONE_ENV ? 0 : lm.el, s = lm.s, e = ONE_ENV ? unit : lm.e, base = ONE_ENV ? 0 : lm.base;
  const bool valid = lm.valid, leader = lm.sub == 0;
  const Grp g{lm.sub, d.sub, lm.lead};
  const int slot = base + s;  // my entry of the LDS snapshot

  PHASE_INIT();
  XMARK(99);
  Veh r;
  RouteCtx ctx{0.0f, 1.0f, 0, -1};  // of this lane's vehicle if it is an agent: refreshed by every after_step_vehicle
  using MV = typename std::conditional<FIX != 0 && !OBJ, MapViewPre, MapView>::type;
  MV mv;
  const pgd_spawn* sp = nullptr;
  // The scalar part of the slot's spawn record (dimensions, drive parameters, trigger group, destination: its first 64 bytes) is
  // read ONCE, four 16-byte loads in one round trip, when the record's address is known; the phases used to fetch its fields one
  // by one where they needed them, each time for a whole memory latency (profiles/r03_notes.md).  Kernels with one env per wave
  // only: the multi-env instantiations have no registers to spare.
  // the ego-only kernel (BASELINE config 2: four envs of one vehicle per wave) is small and far below its register budget: it takes
  // the one-env kernels' short cuts -- spawn head in registers (read with the record), the action read in the first burst, no
  // trigger test without trigger groups -- each of them a memory round trip of a step that is nothing but round trips
  // (round 5: 1024 envs 11.12 -> 10.93 us, 65536 envs 1.40 -> 1.55 G env-steps/s)
  constexpr bool FIXE_K = FIX != 0 && !ONE_ENV && !MARL && !STD;
  constexpr bool REGSP = ONE_ENV || FIXE_K;
  pgd_spawn sl;
  pgd_lane FL;  // REGSP && FIX (registers to spare): the agent's destination lane record, read ahead
#define SPV spawn_ref<REGSP>(sl, sp)
  const pgd_scenario* sc = nullptr;
  int ng = 0, ep_steps = 0;
  uint32_t steps_total = 0;
  // EI_NEAR, left by the observation of the previous step: 0 = no body of the env can reach an agent during this step, so no
  // sub-step pose is kept and no contact test runs; anything else (and every engine without the fused observation) tests
  bool near_env = true;
  // bits 1-2 of the same word, left by the previous step of a single-agent one-env wave: 1 = the agent does NOT stand on the
  // trigger road of the next traffic group, 2 = it does, 0 = unknown (after a reset, pgd_set_state, other kernels): evaluate it here
  int trig_hint = 0;
#ifdef PGD_NO_SUBSTEP
  constexpr bool n_mid_enabled = false;
#else
  constexpr bool n_mid_enabled = true;
#endif
  S.present[lane] = 0;
  s_flag[lane] = 0;
  s_hit[lane] = 0;
  if (lane < PGD_SUBV) SUBP.trav[lane] = 0.0f;
  constexpr bool one_env = ONE_ENV;
  constexpr bool marl = MARL;
  int scen = 0;
  // the vehicle record does not depend on the scenario: its 8 x 16 B reads go out first and overlap the scalar chain
  // env counters -> scenario -> map header -> table pointers below
  // a slot that was never written since the last reset (waiting trigger traffic: most slots of most envs) still equals the
  // scenario's reset image: its lane reads the image -- shared by every env of the scenario, cache resident -- instead of the
  // env's own record in HBM.  One env per wave only; the records in memory stay complete either way.
  unsigned long long im = 0ull;
  const bool packed = !ONE_ENV && d.pack_obs != 0;  // throughput mode: whole envs side by side in the wave, one vehicle per lane
  // (a run-time switch in the general kernels: off with one env per wave -- the branch then skips the read; where it is on, the read
  // sits in a block of its own and is waited for there, a memory latency in front of the scenario id's read)
  // With the image off (a uniform switch) the records' addresses follow from the block index alone: their reads go out FIRST, the
  // scenario id's behind them -- read in front, its round trip sat in the scalar wait that the records' base pointer needs (general
  // kernels; the specialised ones fold the switch).
  const bool own_first = FIX == 0 && ONE_ENV && !d.use_imask;  // (the specialised kernels already come out that way)
  if (own_first && valid) load_rec(rec_block(d.rec, (size_t)e, V), V, s, r);
  if ((ONE_ENV || (packed && valid)) && d.use_imask) im = d.imask[e];
  if (one_env || valid) scen = d.ei[(size_t)e * PGD_NEI + EI_SCEN];
  // the kernel of the multi-agent defaults (no traffic slots, no trigger groups, no IDM policy: nothing before the reward needs the
  // env's counters): EI_NEAR with the scenario id, the counters where they are first used -- below
  constexpr bool LATE_WORDS = MARL && FIX != 0;
  int hint_early = 0;
  if (LATE_WORDS && (one_env || valid)) hint_early = d.ei[(size_t)e * PGD_NEI + EI_NEAR];
  if (valid && !own_first) load_rec(((ONE_ENV || packed) && ((im >> s) & 1ull)) ? rec_block(d.reset_img, (size_t)scen, V) : rec_block(d.rec, (size_t)e, V), V, s, r);
  // the agent's action: its address follows from the block index as well -- read here, used by the policy phase (read there it cost
  // every wave a memory latency of its own right after the snapshot: 1.5 k cycles of the metric's row).  BEHIND the record's reads:
  // issued ahead of the mask / scenario / record chain it delays that chain (17.76 -> 17.99 us), and so does a speculative read
  // of the slot's spawn record next to the vehicle record (18.4 us): the first burst of a wave stays as short as it can be
  float2 act_in = make_float2(0.0f, 0.0f);
  constexpr bool ACT_EARLY = ONE_ENV || FIXE_K;
  if (ACT_EARLY && valid && s < A) {
    if (LK) {  // pgd_step_lane_keep: the action from the row the previous step wrote -- the same round trip as the caller's action
      const float* o = cold.lk_obs + ((size_t)e * A + s) * d.D;
      const float2 q0 = *reinterpret_cast<const float2*>(o), q1 = *reinterpret_cast<const float2*>(o + 2);  // (rows are 8-byte aligned: D even)
      act_in = lane_keep_action(cold.seed, cold.env_base + e, q0.x, q0.y, q1.x, q1.y, cold.lk_klat, cold.lk_khead, cold.lk_vt, cold.lk_noise, cold.lk_tick);
    } else act_in = *reinterpret_cast<const float2*>(act + ((size_t)e * A + s) * 2);
  }
  // single-agent engines: a slot keeps the spawn record of its own index (only a multi-agent respawn hands a slot another one; a
  // state set by hand may: checked below) -- the head's address follows from the scenario id like the record's, and its reads travel
  // with the record's instead of waiting for them (17.48 -> 17.40 us on the metric's row, now that the records' reads are short)
  constexpr bool EARLY_HEAD = !MARL && REGSP && FIX != 0 && !OBJ;  // (the general kernels have no registers for it: 19.5 -> 19.9 us there; nor has the object kernel)
  if (EARLY_HEAD && valid) { sp = d.spawns + (size_t)scen * d.sstride + s; spawn_head_load<false>(sp, sl); }
  const int key0 = valid ? (r.status ^ (r.vflags << 3)) : 0;  // what a vehicle that does not drive can change: status, flags
  // the env's counters.  The multi-agent kernels are out of scalar registers: read here, the compiler fetched the words one after the
  // other through the same register -- three scalar-memory round trips in a row between the records and the spawn heads (a word that
  // goes straight to a spill lane is waited for on the spot).  They take the near hint with the scenario id (above) and the counters
  // where the step first needs them, behind after_step: the row is in the scalar cache by then.
  auto env_words = [&]() {
    ng = d.ei[(size_t)(e) * PGD_NEI + EI_NEXT_GROUP];
    ep_steps = d.ei[(size_t)(e) * PGD_NEI + EI_EP_STEPS];
    steps_total = (uint32_t)d.ei[(size_t)(e) * PGD_NEI + EI_STEPS_TOTAL];
    if (ONE_ENV || packed) {
      const int hint = d.ei[(size_t)(e) * PGD_NEI + EI_NEAR];
      near_env = (hint & 1) != 0;
      trig_hint = (hint >> 1) & 3;
    }
  };
  if (one_env || valid) {
    sc = d.scen + scen;
    mv = map_view_as<MV>(d, d.env_map + e);  // per-env header copy: address known at kernel start
    if (!LATE_WORDS) env_words();
  }
  PHASE_MARK(13);  // load: scenario + table staging
  XMARK(13);
  if (valid) {
    if (!EARLY_HEAD || (int)r.spawn != s) {
      sp = d.spawns + (size_t)scen * d.sstride + r.spawn;
      if (REGSP) spawn_head_load<MARL>(sp, sl);
    }
    // (0) AgentManager.before_step (agent_manager.py:191-199): finished agents count down, then leave the world
    if (marl && r.status == ST_DYING && --r.timer == 0) r.status = ST_EMPTY;
  }
  if (LATE_WORDS && (ONE_ENV || packed)) { near_env = (hint_early & 1) != 0; trig_hint = (hint_early >> 1) & 3; }
  // (1) TrafficManager.before_step trigger (traffic_manager.py:76-85): an agent of the env stands on the trigger road of the next
  // group.  One env per wave: a ballot over the wave's lanes (no trip through LDS); several envs per wave: a flag per env.
  bool on_trigger;
  if (ONE_ENV && !MARL && A == 1 && trig_hint != 0) on_trigger = valid && s < A && trig_hint == 2;
  else if ((MARL || FIXE_K) && d.no_groups) on_trigger = false;  // no scenario has a trigger group (engines without traffic slots: two dependent reads less)
  else on_trigger = valid && s < A && r.status == ST_ACTIVE && ng < sc->n_groups && mv.lanes[r.lane].road == sc->trigger_road[ng];
  bool trig;
  if (ONE_ENV) {
    trig = __ballot(on_trigger) != 0ull;
  } else {
    step_sync();
    if (on_trigger) s_flag[el] = 1;
    step_sync();
    trig = valid && s_flag[el] != 0;
  }
  PHASE_MARK(0);  // load
  XMARK(0);
  if (valid && trig && r.status == ST_PENDING && SPV.group == ng) r.status = ST_ACTIVE;
  if (trig) ng += 1;  // every lane of the env keeps the same copy
  // the trigger road of the next group, for the verdict the step leaves for its successor (below): a scalar read while no store of
  // the kernel has happened yet, long done when it is used
  int next_trigger_road = -1;
  if (ONE_ENV && !MARL && A == 1) next_trigger_road = ng < sc->n_groups ? (int)sc->trigger_road[ng] : -1;
  // the own-lane coordinate / lane length / successor list of a vehicle are read by the IDM neighbour search alone: an
  // env without a driving IDM vehicle in this step (most envs, most steps) skips them
  const bool idm_ego = !MARL && d.cfg.idm_agent != 0;  // IDM_agent: the agent slot is driven by the IDM policy as well
  const bool idm_runs = ONE_ENV ? (__ballot(valid && (s >= A || idm_ego) && r.status == ST_ACTIVE) != 0ull) : true;
  // snapshot of the world before physics
  if (valid) {
    if (leader) {
      S.x[slot] = r.x; S.y[slot] = r.y; S.ux[slot] = r.hx; S.uy[slot] = r.hy;
      S.spd[slot] = speed_kmh(r.v);
      const int kind = OBJ ? (int)SPV.kind : PGD_OBJ_VEHICLE;
      if (OBJ) s_kind[slot] = kind;
      S.hl[slot] = 0.5f * SPV.length; S.hw[slot] = kind == PGD_OBJ_CYLINDER ? -1.0f : 0.5f * SPV.width;
      S.lane[slot] = r.lane;
      const bool present = r.status == ST_PENDING || r.status == ST_ACTIVE || r.status == ST_DYING;
      S.present[slot] = present ? 1 : 0;
      if (present && (V > A || idm_ego) && idm_runs) {
        const pgd_lane& ml = mv.lanes[r.lane];
        S.lon[slot] = r.lon;  // carried in the record since the vehicle's last localisation
        S.llen[slot] = ml.length;
        S.succ[slot] = *reinterpret_cast<const int4*>(ml.succ);
      }
    }
  }
  step_sync();
  PHASE_MARK(1);  // trigger + snapshot
  XMARK(1);
  const bool acting = valid && r.status == ST_ACTIVE;
  if (ONE_ENV) {
    // every wave of a 4096-env launch is resident at once and the kernel ends with its slowest wave: the envs with the
    // most driving IDM vehicles get the issue priority, the light ones fill the gaps
    const int nact = __popcll(__ballot(acting && leader && s >= A));
    if (MARL && V == A) {  // multi-agent engines without traffic: the envs with the most agents alive are the long ones
      const int nag = __popcll(__ballot(acting && leader));
      if (nag * 10 >= A * PGD_MA_PRIO3) __builtin_amdgcn_s_setprio(3);
      else if (nag * 10 >= A * PGD_MA_PRIO2) __builtin_amdgcn_s_setprio(2);
      else if (nag * 10 >= A * PGD_MA_PRIO1) __builtin_amdgcn_s_setprio(1);
    } else
    if (nact >= 4) __builtin_amdgcn_s_setprio(3);
    else if (nact >= 2) __builtin_amdgcn_s_setprio(2);
    else if (nact > 0) __builtin_amdgcn_s_setprio(1);
  }
  // (2) policies
  if (acting) {
    float st, tb;
    if (s < A && !idm_ego) {  // EnvInputPolicy.act (env_input_policy.py:17-26); NaN made harmless (test_ego_vehicle.py:78-84)
      float a0 = ACT_EARLY ? act_in.x : act[((size_t)e * A + s) * 2 + 0], a1 = ACT_EARLY ? act_in.y : act[((size_t)e * A + s) * 2 + 1];
      if (a0 != a0) a0 = 0.0f;
      if (a1 != a1) a1 = 0.0f;
      st = clipf(a0, -1.0f, 1.0f);
      tb = clipf(a1, -1.0f, 1.0f);
      if (d.cfg.discrete_action) {  // convert_to_continuous_action on the CLIPPED action (env_input_policy.py:17-31)
        st = st * (2.0f / (float)(d.cfg.discrete_steering_dim - 1)) - 1.0f;
        tb = tb * (2.0f / (float)(d.cfg.discrete_throttle_dim - 1)) - 1.0f;
      }
    } else {
#ifdef PGD_NO_IDM
      st = 0.0f; tb = 0.0f;
#else
      idm_act<OBJ>(d, mv, g, SPV, S, base, V, s, e, steps_total, r, st, tb);
#endif
    }
    PHASE_MARK(2);  // policy (IDM)
    // (3) BaseVehicle.before_step (base_vehicle.py:238-253)
    r.vflags &= ~(PGD_F_CRASH_VEHICLE | PGD_F_CRASH_OBJECT | PGD_F_CRASH_BUILDING);
    r.lastx = r.x; r.lasty = r.y;
    r.lasthx = r.hx; r.lasthy = r.hy;
    r.a0s = r.a1s; r.a0t = r.a1t;
    r.a1s = st; r.a1t = tb;
    // _set_action / _set_incremental_action (base_vehicle.py:343-358)
    r.steer = (s < A && d.cfg.increment_steering) ? clipf(r.steer + st * 0.05f, -1.0f, 1.0f)
              // pgd_config::idm_steer_lag (an opt-in, 0 in every kernel specialised for a reference configuration): IDM-driven vehicles only
              : ((d.cfg.idm_steer_lag > 0.0f && (s >= A || idm_ego))
                     ? r.steer + (clipf(st, -1.0f, 1.0f) - r.steer) * ((d.cfg.dt * (float)d.cfg.decision_repeat) / (d.cfg.idm_steer_lag + d.cfg.dt * (float)d.cfg.decision_repeat))
                     : st);
    // (4) physics
    dynamics(d, SPV, r, s < A && d.cfg.enable_reverse != 0, tb, leader ? &SUBP : nullptr, slot, near_env && sub_ok && n_mid_enabled);
    PHASE_MARK(3);  // dynamics
  }
  step_sync();
  if (acting && leader) { S.x[slot] = r.x; S.y[slot] = r.y; S.ux[slot] = r.hx; S.uy[slot] = r.hy; }
  step_sync();
  // (5) contacts (collision_callback.py:7-36).  The reference's callback runs inside each of the decision_repeat doPhysics
  // calls (engine_core.py:276-278): two bodies are in contact when they overlap after ANY sub-step, not only at the end of
  // the 0.1 s step.  Every body in the world tests itself against each agent of its env (A x V pair tests in parallel lanes):
  // first against the reach of the two paths (centre distance vs circumradii + path lengths: exact, never drops a contact),
  // then pose by pose.  Bodies that did not drive stand still.  Bullet's collision margin is not modelled (see the oracle).
#ifdef PGD_NO_SUBSTEP
  const int n_mid = 0;
#else
  const int n_mid = (d.cfg.decision_repeat <= PGD_MAX_SUB && sub_ok) ? d.cfg.decision_repeat - 1 : 0;
#endif
  if (near_env) {
    const int my_kind = (OBJ && valid) ? s_kind[slot] : PGD_OBJ_VEHICLE;
    // pose-by-pose test of body `bs` against agent `as` (slots of the snapshot); everything comes from LDS
    constexpr bool PAIR_LISTS = ONE_ENV && MARL && !OBJ;  // (the engines that may take the contact-list path below)
    auto pair_touch = [&](const int bs, const int as, const Obb& me, const float my_trav, const Obb& ag, const float ag_trav) {
      bool hit = shape_overlap<OBJ, PAIR_LISTS>(ag, me);
      for (int k = 0; k < n_mid && !hit; ++k) {
        Obb ak = ag, mk = me;
        if (ag_trav > 0.0f) {  // heading = motion direction rotated back by the slip angle (unit up to rounding)
          const float4 q = SUBP.p[k][as]; const float2 b = SUBP.beta[as];
          ak.cx = q.x; ak.cy = q.y; ak.ux = q.z * b.x + q.w * b.y; ak.uy = q.w * b.x - q.z * b.y;
        }
        if (my_trav > 0.0f) {
          const float4 q = SUBP.p[k][bs]; const float2 b = SUBP.beta[bs];
          mk.cx = q.x; mk.cy = q.y; mk.ux = q.z * b.x + q.w * b.y; mk.uy = q.w * b.x - q.z * b.y;
        }
        hit = shape_overlap<OBJ, PAIR_LISTS>(ak, mk);
      }
      return hit;
    };
    // Multi-agent engines with more agent slots than sub-lanes per slot (a lane would walk several agents; no traffic objects):
    // only an agent that drove reads its contact bits, so the agents to test against are the ACTIVE ones -- a ballot -- and the
    // work is laid out by PAIRS.  As a loop over agents inside every body lane an iteration costs the whole wave the pose-by-pose
    // test (five separating-axis tests) as soon as ONE lane is within reach of that agent: with 30 of 40 agents alive, bunched
    // around the spawn places, that was 77 k cycles of a 139 k-cycle step (profiles/r04_notes.md).  Now: (1) every body lane
    // walks the agents with the reach test alone and notes the ones within reach; (2) the (body, agent) pairs within reach go
    // into a list in LDS; (3) the wave takes the list 64 pairs at a time.  Same pairs pass the same reach test, same verdicts.
    // Chunks of 12 agents bound the list (64 bodies x 12); it lives where the IDM search keeps its lane data (no IDM traffic here).
    const bool by_mask = ONE_ENV && MARL && !OBJ && A > g.SUB;
    if (by_mask) {
      // UNORDERED pairs of the bodies in the world: (i, j) is needed when either drove as an agent this step, and one verdict
      // serves both (the reach test and the separating-axis test are symmetric).  The bodies are compacted into a list of n;
      // round r pairs position i with position (i + r) mod n, r = 1 .. n / 2 (every unordered pair once; the last round of an
      // even n only for i < n / 2), and 64 / n rounds run side by side in the wave: 30 bodies take 8 iterations of the reach
      // test where a loop over the agents inside every body lane took 30.
      constexpr int CAP = 736;  // pairs the list holds (the LDS of the IDM search's lane data, unused here; the body list behind it)
      static_assert(2 * CAP + WAVE <= (int)(sizeof(float) * 2 * WAVE + sizeof(int4) * WAVE), "pair list + body list live in Snap::lon .. succ");
      unsigned short* plist = reinterpret_cast<unsigned short*>(&S.lon[0]);
      unsigned char* bl = reinterpret_cast<unsigned char*>(plist + CAP);  // [64]: slot | drove-as-agent << 7
      const bool body = valid && leader && S.present[slot] != 0;
      const unsigned long long bm = __ballot(body);
      const int n = __popcll(bm);
      const bool any_agent = __ballot(body && s < A && acting) != 0ull;
      if (n >= 2 && any_agent) {
        if (body) bl[__popcll(bm & ((1ull << lane) - 1ull))] = (unsigned char)(slot | ((s < A && acting) ? 0x80 : 0));
        step_sync();
        const int K = n <= WAVE / 2 ? WAVE / n : 1, half = n / 2;
        const int k = lane / n, i = lane - k * n;
        const bool lane_on = k < K;
        const int ei = bl[lane_on ? i : 0], bi = ei & 0x3f;
        const Obb me = snap_obb(S, bi);
        const float my_trav = sub_ok ? SUBP.trav[bi] : 0.0f;
        const float my_reach = me.hl + (me.hw < 0.0f ? 0.0f : me.hw) + my_trav + 0.01f;
        int count = 0;  // pairs in the list (uniform)
        auto flush = [&]() {
          step_sync();
          for (int p0 = 0; p0 < count; p0 += WAVE) {
            const int p = p0 + lane;
            if (p < count) {
              const int pr = plist[p], bs = pr >> 8, as = pr & 0xff;
              if (pair_touch(bs, as, snap_obb(S, bs), sub_ok ? SUBP.trav[bs] : 0.0f, snap_obb(S, as), sub_ok ? SUBP.trav[as] : 0.0f)) {
                s_hit[bs] = 1; s_hit[as] = 1;
              }
            }
          }
          step_sync();
          count = 0;
        };
        for (int r0 = 1; r0 <= half; r0 += K) {
          const int r = r0 + k;
          int j = i + r;
          j -= j >= n ? n : 0;
          const bool pair_on = lane_on && r <= half && !(2 * r == n && i >= half);
          const int ej = bl[pair_on ? j : 0], bj = ej & 0x3f;
          const float ox = S.x[bj], oy = S.y[bj], ohl = S.hl[bj], ohw = S.hw[bj];
          const float o_trav = sub_ok ? SUBP.trav[bj] : 0.0f;
          const float reach = my_reach + ohl + (ohw < 0.0f ? 0.0f : ohw) + o_trav;
          const float ddx = ox - me.cx, ddy = oy - me.cy;
          const bool within = pair_on && ((ei | ej) & 0x80) != 0 && !(ddx * ddx + ddy * ddy > reach * reach);
          const unsigned long long wm = __ballot(within);
          if (within) plist[count + __popcll(wm & ((1ull << lane) - 1ull))] = (unsigned short)((bi << 8) | bj);
          count += __popcll(wm);
          if (count > CAP - WAVE) flush();
        }
        if (count > 0) flush();
      }
    } else
    if (valid && S.present[slot]) {  // a vehicle's sub-lanes split the agents; object sub-lanes all keep their copy of the bit
      const Obb me = snap_obb(S, slot);
      const float my_trav = sub_ok ? SUBP.trav[slot] : 0.0f;
      const float my_rad = me.hl + (me.hw < 0.0f ? 0.0f : me.hw);  // >= the circumradius
      // a traffic object reports only its first contact (TrafficObject.crashed / COST_ONCE, collision_callback.py:27-32)
      const bool live = !OBJ || my_kind == PGD_OBJ_VEHICLE || !(r.vflags & (int)PGD_F_OBJECT_HIT);
      bool touched = false;
      const bool split = !OBJ || my_kind == PGD_OBJ_VEHICLE;
      for (int a = split ? g.sub : 0; a < A; a += split ? g.SUB : 1) {
        if (a == s || (OBJ && !S.present[base + a])) continue;
        const Obb ag = snap_obb(S, base + a);
        const float ag_trav = sub_ok ? SUBP.trav[base + a] : 0.0f;
        const float reach = my_rad + ag.hl + ag.hw + my_trav + ag_trav + 0.01f;
        const float ddx = ag.cx - me.cx, ddy = ag.cy - me.cy;
        if (ddx * ddx + ddy * ddy > reach * reach) continue;
        if (!pair_touch(slot, base + a, me, my_trav, ag, ag_trav)) continue;
        touched = true;
        if (!OBJ) s_hit[base + a] = 1;
        else if ((leader || split) && live) atomicOr(&s_hit[base + a], my_kind == PGD_OBJ_VEHICLE ? 1 : (my_kind == PGD_OBJ_BUILDING ? 4 : 2));
      }
      if (OBJ && touched && my_kind != PGD_OBJ_VEHICLE && my_kind != PGD_OBJ_BUILDING) r.vflags |= (int)PGD_F_OBJECT_HIT;  // all sub-lanes
    }
    step_sync();
    if (acting && s < A) {
      if (s_hit[slot] & 1) r.vflags |= PGD_F_CRASH_VEHICLE;
      if (OBJ && (s_hit[slot] & 2)) r.vflags |= PGD_F_CRASH_OBJECT;
      if (OBJ && (s_hit[slot] & 4)) r.vflags |= PGD_F_CRASH_BUILDING;
    }
  }
  PHASE_MARK(4);  // crash
  XMARK(4);
  // (6) after_step; traffic off the lanes is removed (traffic_manager.py:91-109)
  if (acting) {
    // several agents: each tests its own box against the lines with its sub-lanes (all agents at once) instead of the
    // whole wave working through the agents one after the other
    // several agents: the line / sidewalk test runs as a phase of its own (below), where the localisation's boxes and lane
    // records are no longer live -- inside after_step it pushed the multi-agent kernel 66 registers over the 128 it may use
    // the destination lane of an agent (arrive test of reward_done) is known from its spawn record: read before the localisation
    if (REGSP && FIX && !OBJ && s < A) FL = mv.lanes[SPV.dest_lane];
    after_step_vehicle<ONE_ENV>(d.cfg, mv, g, *sp, SPV, r, s < A, !one_env, ctx);
    if (s >= A && (r.vflags & PGD_F_OFF_LANE)) r.status = ST_REMOVED;
  }
  // the trigger test of the NEXT step (TrafficManager.before_step looks at the state this step leaves): the road of the agent's lane
  // comes with after_step's own read of that lane record (RouteCtx::lane_road), and the verdict travels in the env's hint word --
  // the next step starts without the two dependent reads the test costs
  int trig_next = 0;
  if (ONE_ENV && !MARL && A == 1 && valid && s < A)
    trig_next = (r.status == ST_ACTIVE && next_trigger_road >= 0 && ctx.lane_road == next_trigger_road) ? 2 : 1;
  if (one_env && A > 1) {
    const bool need = acting && s < A && !ctx.clear;
    const unsigned long long need_m = __ballot(need && leader);
    if (d.sub > 3) {
      // every agent's own lanes stride through the boxes under its car, all agents at once
      if (need) r.vflags |= (int)state_check(mv, g, Obb{r.x, r.y, r.hx, r.hy, 0.5f * SPV.length, 0.5f * SPV.width});
    } else if (need_m != 0ull) {
      // many slots with one to three lanes each (40 agents: one): a lane alone would walk the 25 - 90 boxes of the cells under its car (a
      // roundabout's cells are full of short line segments) one by one while the lanes of the agents with nothing to test idle.
      // The wave is dealt out to the agents that DO need the test instead: 64 / n lanes each (one agent: the whole wave), the
      // shares ORed through LDS -- the same boxes, the same flags.  (The lane data of the IDM search is dead by now: the list of
      // the agents to test and their flag words live there.)
      unsigned char* nl = reinterpret_cast<unsigned char*>(&S.lon[0]);
      unsigned* fo = reinterpret_cast<unsigned*>(&S.llen[0]);
      const int n_need = __popcll(need_m);
      const int my_pos = __popcll(need_m & ((1ull << (need ? g.lead : 0)) - 1ull));  // of my slot's leader lane among the set bits
      if (need && leader) nl[my_pos] = (unsigned char)slot;
      fo[lane] = 0u;
      step_sync();
      const int G = WAVE / n_need, gi = lane / G;
      if (gi < n_need) {
        const unsigned part = state_check_part(mv, lane - gi * G, G, snap_obb(S, nl[gi]));
        if (part != 0u) atomicOr(&fo[gi], part);
      }
      step_sync();
      if (need) r.vflags |= (int)fo[my_pos];  // (every sub-lane of the slot: they keep equal copies of the record)
    }
  }
  PHASE_MARK(25);  // after_step: per-vehicle part
  if (one_env && A == 1) {  // line / sidewalk test of the agent by the whole wave (base_vehicle.py:615-644)
    // clear: provably no contact (after_step); the agent's lanes tell the wave by ballot
    if (__ballot(leader && valid && s < A && acting && !ctx.clear) != 0ull) {
      unsigned fl = state_check_wave(mv, snap_obb(S, 0));
      if (valid && s == 0) r.vflags |= (int)fl;
    }
  }
  PHASE_MARK(5);  // after_step
  XMARK(5);
  if (LATE_WORDS && (one_env || valid)) {  // (not before this point: see env_words)
    asm volatile("" ::: "memory");
    ng = d.ei[(size_t)(e) * PGD_NEI + EI_NEXT_GROUP];
    ep_steps = d.ei[(size_t)(e) * PGD_NEI + EI_EP_STEPS];
    steps_total = (uint32_t)d.ei[(size_t)(e) * PGD_NEI + EI_STEPS_TOTAL];
  }
  ep_steps += 1;
  steps_total += 1;
  // (7) reward / done (base_env.py:303-344).  "The env restarts": one env per wave -> a ballot over the lanes that ask for it;
  // several envs per wave -> a flag per env in LDS
  bool want_reset = false;
  if (!ONE_ENV) {
    s_flag[lane] = 0;
    step_sync();
  }
  unsigned my_fl = 0;
  bool fresh = false;  // multi-agent: this lane's slot received a new agent in this step
  int fresh_idx = 0, fresh_id = 0;  // ... from this respawn record, with this agent id
  bool my_dn = false;
  float my_rew = 0.0f;
  const bool was_active = acting;  // status at the start of the step (after the delay-done countdown)
  if (valid && s < A && !marl) {
    if (r.status == ST_ACTIVE) my_rew = reward_done<false>(d, mv, SPV, dest_lane_ref<REGSP && FIX != 0 && !OBJ>(FL, mv.lanes, SPV.dest_lane), r, ctx, my_fl, my_dn);
    if (d.cfg.horizon > 0 && ep_steps >= d.cfg.horizon) { my_dn = true; my_fl |= PGD_F_MAX_STEP; }
    if (sc->max_steps > 0 && ep_steps >= sc->max_steps) { my_dn = true; my_fl |= PGD_F_MAX_STEP; }  // auto_termination
    r.eprew += my_rew;
    bool will_reset = my_dn && d.cfg.auto_reset && A == 1;
    if (will_reset) { my_fl |= PGD_F_RESET; want_reset = true; if (!ONE_ENV) s_flag[el] = 1; }
  }
  if (marl && one_env) {
    // ---- multi-agent tail: multi_agent_pgdrive.py:109-213, agent_manager.py:134-175, spawn_manager.py:160-215 ----
    const pgd_config& gcf = d.cfg;
    const bool toll = (gcf.marl_flags & PGD_MA_TOLLGATE) != 0;
    const bool parking = (gcf.marl_flags & PGD_MA_PARKING) != 0;
    if (parking && lane == 0) s_aux = d.ei[(size_t)e * PGD_NEI + EI_AUX];  // parking_space_available
    if (parking) step_sync();
    if (valid && s < A && was_active) {
      if (toll && r.blk == '$') r.php += 1.0f;  // TollGateObservation.observe counts its calls inside the toll block
      my_rew = reward_done<true>(d, mv, SPV, dest_lane_ref<REGSP && FIX != 0>(FL, mv.lanes, SPV.dest_lane), r, ctx, my_fl, my_dn);
      const bool arrive = my_fl & PGD_F_ARRIVE, oor = my_fl & PGD_F_OUT_OF_ROAD, crash = my_fl & PGD_F_CRASH_VEHICLE;
      if (crash && !(gcf.marl_flags & PGD_MA_CRASH_DONE) && !(arrive || oor)) my_dn = false;
      if (oor && !(gcf.marl_flags & PGD_MA_OUT_ROAD_DONE) && !arrive) my_dn = false;
      if (toll && r.phi >= 0.0f && r.plp >= 0.0f && r.plp - r.phi < (float)gcf.min_pass_steps) {  // marl_tollgate.py:262-268
        my_dn = true;
        my_fl |= PGD_F_OUT_OF_ROAD;
      }
      if (r.rlane < 0x7fff) r.rlane += 1;  // episode_length (a 16-bit field: saturates; pgd_create rejects longer horizons)
      if (gcf.horizon > 0 && r.rlane >= gcf.horizon) { my_dn = true; my_fl |= PGD_F_MAX_STEP; }
      r.eprew += my_rew;
      my_fl |= PGD_F_REPORT;
      if (my_dn && parking && r.php > 0.0f) {  // ParkingLotSpawnManager.after_vehicle_done: its space is free again
        if (leader) atomicOr(&s_aux, 1 << ((int)r.php - 1));
        r.php = 0.0f;
      }
      if (my_dn) {  // AgentManager.finish
        if (arrive || gcf.delay_done <= 0) r.status = ST_EMPTY;
        else { r.status = ST_DYING; r.timer = gcf.delay_done; }
      }
    }
    if (valid && leader && s < A) {  // reward and done are final here: written now, not carried across the respawn code
      const size_t k = (size_t)e * A + s;
      reward[k] = my_rew;
      done[k] = my_dn ? 1 : 0;
      if (d.prow) {
        float* tail = d.prow + (size_t)e * d.ostride + (size_t)A * d.D;
        tail[s] = my_rew;
        tail[A + s] = my_dn ? 1.0f : 0.0f;
      }
    }
    PHASE_MARK(26);  // marl: reward / done / finish
    // the world after the finishes (leaders publish, everybody reads)
    step_sync();
    if (valid && leader) {
      S.x[slot] = r.x; S.y[slot] = r.y; S.ux[slot] = r.hx; S.uy[slot] = r.hy;
      S.hl[slot] = 0.5f * SPV.length; S.hw[slot] = 0.5f * SPV.width;
      S.present[slot] = (r.status == ST_PENDING || r.status == ST_ACTIVE || r.status == ST_DYING) ? 1 : 0;
    }
    step_sync();
    const bool is_lead_agent = valid && leader && s < A;
    int alive = __popcll(__ballot(is_lead_agent && (r.status == ST_ACTIVE || r.status == ST_DYING)));
    int next_agent = d.ei[(size_t)e * PGD_NEI + EI_NEXT_AGENT];
    const bool allow = (gcf.marl_flags & PGD_MA_ALLOW_RESPAWN) && !(gcf.horizon > 0 && ep_steps >= gcf.horizon) &&
                       alive < gcf.agent_limit;
    if (allow) {
      // get_available_respawn_places offers every place at most once per frame (spawn_places_used, spawn_manager.py:157-207) and
      // _respawn_vehicles takes ONE of the offered places per call (multi_agent_pgdrive.py:180-213): the second call of the frame finds
      // every free place already offered and stops -- at most one newcomer per step, on a random one of the free places
      // (rounds 2 - 4 filled every free place in the same step)
      const pgd_spawn* rbase = d.spawns + (size_t)scen * d.sstride + V;
      unsigned long long freem = 0ull;
      // the places' poses: lane p reads place p, one round trip for all of them (read inside the loop, place after place, the two
      // dependent reads per place were 5 k cycles of a step with 30 agents alive: profiles/r05_notes.md)
      float plx = 0.0f, ply = 0.0f, plc = 1.0f, pls = 0.0f;
      if (lane < gcf.respawn_places) {
        const pgd_spawn& place = rbase[lane * gcf.respawn_dests];
        const float2 phv = cold.spawn_hv[(size_t)scen * d.sstride + V + lane * gcf.respawn_dests];
        plx = place.x; ply = place.y; plc = phv.x; pls = phv.y;
      }
      const Obb mine = snap_obb(S, lane < V ? lane : 0);
      const bool here = lane < V && S.present[lane];
      for (int p = 0; p < gcf.respawn_places; ++p) {
        const Obb region{__shfl(plx, p), __shfl(ply, p), __shfl(plc, p), __shfl(pls, p), 4.0f, 1.5f};  // RESPAWN_REGION 8 m x 3 m (spawn_manager.py:27-28)
        const bool blocks = here && obb_overlap(region, mine);
        if (__ballot(blocks) == 0ull) freem |= 1ull << p;
      }
      // lowest empty slot that did not report this step (its terminal row must survive)
      const unsigned long long em = __ballot(is_lead_agent && r.status == ST_EMPTY && !(my_fl & PGD_F_REPORT));
      // parking lot: a road place is offered only while a parking space is free (marl_parking_lot.py:176-190)
      const unsigned pool = parking ? ((unsigned)s_aux & ((1u << gcf.respawn_dests) - 1u)) : 1u;
      if (freem != 0ull && em != 0ull && __ballot(pool != 0u) != 0ull) {
        int kth = (int)(pgd_rng(gcf.seed, (uint32_t)(gcf.env_base + e), 0x51ace5u, (uint32_t)next_agent) % (uint32_t)__popcll(freem));
        unsigned long long fm = freem;
        while (kth-- > 0) fm &= fm - 1ull;
        const int p = __builtin_ffsll((long long)fm) - 1;
        const int src = __builtin_ffsll((long long)em) - 1;
        const int tslot = (src / d.sub) % V;
        int dest = (int)(pgd_rng(gcf.seed, (uint32_t)(gcf.env_base + e), 0x0a9e47u + (uint32_t)p, (uint32_t)next_agent) %
                         (uint32_t)gcf.respawn_dests);
        if (parking) {  // get_parking_space: a random one of the free spaces
          int pick = (int)(pgd_rng(gcf.seed, (uint32_t)(gcf.env_base + e), 0x0a9e47u + (uint32_t)p, (uint32_t)next_agent) %
                           (uint32_t)__popc(pool));
          dest = 0;
          for (int b = 0; b < 32; ++b)
            if (pool & (1u << b)) { if (pick-- == 0) { dest = b; break; } }
          step_sync();  // everybody has read the pool before lane 0 takes the space out
          if (lane == 0) s_aux &= ~(1 << dest);
        }
        if (valid && s == tslot) {
          fresh_idx = V + p * gcf.respawn_dests + dest;
          fresh_id = next_agent;
          fresh = true;
          my_fl |= PGD_F_NEW;
          if (leader) {
            const pgd_spawn& nsp = d.spawns[(size_t)scen * d.sstride + fresh_idx];
            const float2 nhv = cold.spawn_hv[(size_t)scen * d.sstride + fresh_idx];
            S.x[slot] = nsp.x; S.y[slot] = nsp.y; S.ux[slot] = nhv.x; S.uy[slot] = nhv.y;
            S.hl[slot] = 0.5f * nsp.length; S.hw[slot] = 0.5f * nsp.width;
            S.present[slot] = 1;
          }
        }
        next_agent += 1;
        step_sync();
      }
    }
    if (fresh) {  // the new agent's record, first localisation included, from the respawn image (k_respawn_image)
      sp = d.spawns + (size_t)scen * d.sstride + fresh_idx;
      if (REGSP) spawn_head_load<MARL>(sp, sl);
      load_rec(rec_block(cold.respawn_img, (size_t)scen, d.sstride - V), d.sstride - V, fresh_idx - V, r);
      r.agent_id = (float)fresh_id;
    }
    PHASE_MARK(27);  // marl: respawn
    // StayTimeManager.record(active_agents, episode_steps) after the step (marl_tollgate.py:36-60,276-279)
    if (toll && valid && s < A && r.status == ST_ACTIVE) {
      const float cur = (float)r.blk, last = r.pli;
      r.pli = cur;
      if (last >= 0.0f && last != cur) {
        if (r.blk == '$') r.phi = (float)ep_steps;
        else if ((r.blk == 'y' || r.blk == 'Y') && last == (float)'$') r.plp = (float)ep_steps;
      }
    }
    // d["__all__"] (multi_agent_pgdrive.py:142-148)
    const int n_active = __popcll(__ballot(is_lead_agent && r.status == ST_ACTIVE));
    const bool all_done = n_active == 0 || (gcf.horizon > 0 && ep_steps >= 5 * gcf.horizon);
    if (all_done) {
      my_fl |= PGD_F_ALL_DONE;
      if (gcf.auto_reset) { my_fl |= PGD_F_RESET; want_reset = true; }
    }
    if (lane == 0) d.ei[(size_t)e * PGD_NEI + EI_NEXT_AGENT] = next_agent;
    if (parking) {
      step_sync();
      if (lane == 0) d.ei[(size_t)e * PGD_NEI + EI_AUX] = s_aux;
    }
  }
  if (!ONE_ENV) step_sync();
  PHASE_MARK(6);  // reward/done
  XMARK(6);
  // (8) auto reset (base_env.py:269-301): the whole env restarts from its (possibly re-drawn) scenario
  int episodes = 0;
  // ONE_ENV: the same for every lane: a scalar branch keeps scen / mv in SGPRs
  const bool resetting = ONE_ENV ? (__ballot(want_reset) != 0ull) : (valid && s_flag[el]);
  if (resetting) {
    episodes = d.ei[(size_t)(e) * PGD_NEI + EI_EPISODES] + 1;
    if (d.cfg.resample_scenario)
      scen = (int)(pgd_rng(cold.seed, (uint32_t)(cold.env_base + e), 0x5ce9a210u, (uint32_t)episodes) % (uint32_t)cold.n_scen);
    sc = d.scen + scen;
    mv = map_view_as<MV>(d, cold.scen_map + scen);  // the header of the new episode's map (the per-env copy is rewritten below)
    ng = 0;
    ep_steps = 0;
  }
  if (valid && resetting) {
    sp = d.spawns + (size_t)scen * d.sstride + s;
    if (REGSP) spawn_head_load<MARL>(sp, sl);
    // the slot right after a reset is a function of the scenario alone (spawn pose, first localisation, side distances,
    // agent id): read from the image k_reset_image built at upload instead of localising every vehicle again
    load_rec(rec_block(d.reset_img, (size_t)scen, V), V, s, r);
    const unsigned long long am = __ballot(leader && s < A && r.status == ST_ACTIVE);
    if (marl && s < A && r.status == ST_ACTIVE) my_fl |= PGD_F_NEW;
    if (s == 0 && d.cfg.resample_scenario)  // the env's header copy follows the scenario (any number of sub-lanes)
      for (int q = g.sub; q < (int)(sizeof(pgd_map) / 16); q += g.SUB)
        reinterpret_cast<uint4*>(d.env_map + e)[q] = reinterpret_cast<const uint4*>(cold.scen_map + scen)[q];
    if (s == 0 && leader) {
      d.ei[(size_t)(e) * PGD_NEI + EI_SCEN] = scen;
      d.ei[(size_t)(e) * PGD_NEI + EI_EPISODES] = episodes;
      d.ei[(size_t)(e) * PGD_NEI + EI_NEXT_AGENT] = A == 1 ? 1 : __popcll(am);
      d.ei[(size_t)(e) * PGD_NEI + EI_AUX] = sc->aux;  // parking: the pool of the new episode
      if (cold.bev_fill) cold.bev_fill[e] = 1;
    }
  }
  if (valid && leader && s < A) {
    size_t k = (size_t)e * A + s;
    flags[k] = my_fl;
    if (!marl) {
      reward[k] = my_rew;
      done[k] = my_dn ? 1 : 0;
      if (d.prow) {  // pgd_step_packed: [A*D obs | A reward | A done] per env
        float* tail = d.prow + (size_t)e * d.ostride + (size_t)A * d.D;
        tail[s] = my_rew;
        tail[A + s] = my_dn ? 1.0f : 0.0f;
      }
    }
  }
  PHASE_MARK(7);  // reset
  XMARK(7);
  bool stored = false;
  if (valid && leader) {
    // a slot that neither drove, restarted, counted down (delay-done) nor changed status / flags still holds its record:
    // the waiting traffic of the trigger mode (most slots of most envs) costs no write
    stored = acting || resetting || (r.status ^ (r.vflags << 3)) != key0 || (key0 & 7) == ST_DYING;
    if (stored) store_veh(d, e, s, r);
    if (s == 0) {
      d.ei[(size_t)(e) * PGD_NEI + EI_NEXT_GROUP] = ng;
      d.ei[(size_t)(e) * PGD_NEI + EI_EP_STEPS] = ep_steps;
      d.ei[(size_t)(e) * PGD_NEI + EI_STEPS_TOTAL] = (int)steps_total;
    }
  }
  if (ONE_ENV) {  // written slots leave the image; a restart puts every slot back on it
    const unsigned long long sb = __ballot(stored);
    const unsigned long long cleared = __ballot(lane < V && ((sb >> (lane * d.sub)) & 1ull) != 0ull);
    const unsigned long long full = V >= 64 ? ~0ull : ((1ull << V) - 1ull);
    const unsigned long long nm = resetting ? full : (im & ~cleared);
    if (lane == 0 && nm != im && d.use_imask) d.imask[e] = nm;
  } else if (packed) {  // one lane per slot: the env's bits of the ballot are its slots
    const unsigned long long sb = __ballot(stored);
    const unsigned long long full = (1ull << V) - 1ull;
    const unsigned long long nm = resetting ? full : (im & ~((sb >> base) & full));
    if (valid && s == 0 && nm != im && d.use_imask) d.imask[e] = nm;
  }
  PHASE_MARK(8);  // store
  XMARK(8);
  // (9) observation of the new state, fused: the wave already holds every vehicle of the env (obs/state_obs.py:132-170)
  bool near_next = true;  // EI_NEAR of the next step: only the fused observation can clear it
  if (ONE_ENV && !MARL && obs != nullptr) {  // host passes obs only when one_env && !marl && A <= FUSE_MAX_AGENTS
    step_sync();
    if (valid && leader) {
      const bool present = r.status == ST_PENDING || r.status == ST_ACTIVE || r.status == ST_DYING;
      S.x[slot] = r.x; S.y[slot] = r.y; S.ux[slot] = r.hx; S.uy[slot] = r.hy;
      S.spd[slot] = r.status == ST_DYING ? 0.0f : speed_kmh(r.v);
      S.hl[slot] = 0.5f * SPV.length;  // the scenario may have changed on reset
      S.hw[slot] = (OBJ && SPV.kind == PGD_OBJ_CYLINDER) ? -1.0f : 0.5f * SPV.width;
      if (OBJ) s_kind[slot] = SPV.kind;
      S.present[slot] = present ? 1 : 0;
      if (s < A) {
        AgentView& ag = s_ag[s];
        ag.x = r.x; ag.y = r.y; ag.th = r.th; ag.hx = r.hx; ag.hy = r.hy; ag.dl = r.dl; ag.dr = r.dr; ag.v = r.v;
        ag.steer = r.steer; ag.a0s = r.a0s; ag.a0t = r.a0t; ag.lhx = r.lasthx; ag.lhy = r.lasthy;
        ag.cur_first = r.cur_first; ag.cur_n = r.cur_n; ag.next_first = r.next_first;
        ag.blk = r.blk; ag.toll_time = r.php;
        ag.env = e; ag.slot = s; ag.tick = steps_total;
      }
    }
    step_sync();
    // only launched with one env per wave: `scen` / `mv` are wave-uniform and already those of the new episode after a reset
    const int scen_now = scen;
    const MV& mvo = mv;
    PHASE_MARK(20);  // obs: publish
  XMARK(20);
    bool near_any = false;
    const float t_step = d.cfg.dt * (float)d.cfg.decision_repeat;
    for (int a = 0; a < A; ++a) {
      const AgentView ag = s_ag[a];
      const bool have = lane < V && d.cfg.num_lasers > 0;
      bool near_a = false;
      ObsPre pre;  // the row's memory reads go out before the compaction and arrive under it
      obs_preload(d, mvo, ag, lane, WAVE, pre);
      obs_compact<OBJ>(OL, lane, a, have && S.present[lane], OBJ ? (have && s_kind[lane] == PGD_OBJ_VEHICLE) : true, S.x[lane], S.y[lane],
                  S.ux[lane], S.uy[lane], S.hl[lane], S.hw[lane], S.spd[lane], ag.x, ag.y, d.cfg.lidar_dist, ag.hx, ag.hy,
                  d.cfg.num_lasers, S.hl[a] + S.hw[a] + near_reach(ag.v, t_step), &near_a, t_step);
      near_any = near_any || near_a;
      step_sync();
      PHASE_MARK(21);  // obs: compaction
      XMARK(21);
      observe_agent<OBJ, STD, false, true, true>(d, mvo, d.spawns[(size_t)scen_now * d.sstride + a], ag, OL,
                                                 obs + (size_t)e * d.ostride + (size_t)a * d.D, lane, WAVE, nullptr, nullptr, &pre, lidar_minb(S));
      step_sync();
    }
    // hint for the next step's contact tests (EI_NEAR); without a lidar the compaction looked at nothing: always test
    near_next = near_hint_usable(d.cfg) ? (__ballot(near_any) != 0ull) : true;
  }
  if (ONE_ENV) {
    // lane 0 is the leader of slot 0, the agent of a single-agent env; a restart leaves the trigger verdict unknown
    const int hint_next = (near_next ? 1 : 0) | ((!MARL && A == 1 && !resetting) ? (trig_next << 1) : 0);
    if (lane == 0 && hint_next != ((near_env ? 1 : 0) | (trig_hint << 1))) d.ei[(size_t)e * PGD_NEI + EI_NEAR] = hint_next;
  }
  if (packed && obs == nullptr && valid && s == 0 && leader && !near_env) d.ei[(size_t)e * PGD_NEI + EI_NEAR] = 1;  // no row, no hint
  // multi-agent engine with many agent slots (the rows are k_observe_env's, after this launch): the state block of every row that is
  // due -- an agent that reported, a newcomer, or after a restart every active agent -- by the lane that holds the vehicle: its
  // record, route context and map view are in registers here, where the four-wave kernel would read records, spawn records and
  // lane tables back and run the float ladder in every wave (PgdDev::state_rows; same routine, one thread per row)
  if (ONE_ENV && MARL && obs == nullptr && d.state_rows != nullptr && valid && leader && s < A) {
    const bool due = resetting ? r.status == ST_ACTIVE : (my_fl & (PGD_F_REPORT | PGD_F_NEW)) != 0u;
    if (due) {
      AgentView ag;
      ag.x = r.x; ag.y = r.y; ag.th = r.th; ag.hx = r.hx; ag.hy = r.hy; ag.dl = r.dl; ag.dr = r.dr; ag.v = r.v;
      ag.steer = r.steer; ag.a0s = r.a0s; ag.a0t = r.a0t; ag.lhx = r.lasthx; ag.lhy = r.lasthy;
      ag.cur_first = r.cur_first; ag.cur_n = r.cur_n; ag.next_first = r.next_first;
      ag.blk = r.blk; ag.toll_time = r.php;
      ag.env = e; ag.slot = s; ag.tick = steps_total;
      state_block_one(d, mv, SPV, ag, d.state_rows + (size_t)e * d.ostride + (size_t)s * d.D);  // (state_in_step_ok: the plain row layout)
    }
  }
  // multi-agent engine: the rows of all agents, from the records and flags this wave has just written (the barrier makes
  // them visible to the whole workgroup); the step's LDS is free by now
  if (ONE_ENV && MARL && obs != nullptr) {
    __syncthreads();
    // engines without traffic slots and with the lanes of an agent laid out as the routine lays out its state block (always, when
    // V == A: both split the wave into A groups) hand over what the wave holds; else the routine reads the env back from memory
    if (FIX) {  // the default multi-agent configuration has no traffic slots (T == 0 is one of its constants)
      const MapView mvb = mv;
      const unsigned lead_fl = (unsigned)__shfl((int)my_fl, g.lead);  // the step flags are complete in the slot's first lane only
      const EnvInWave in_wave{&r, &SPV, &mvb, lead_fl, scen, steps_total, valid ? s : A, g.sub};  // lanes past the last slot: no agent
      // (V == A and WAVE / A lanes per slot: the host launches this instantiation for no other engine -- step_kernel -- so the
      // read-back form of the routine is not compiled into it: 2 k instructions less in a kernel that filled the instruction cache)
      observe_env_body<1, false, true, OBJ>(d, e, obs, flags, U.obs.m, U.obs.minb, d.obs_g, &in_wave);
    } else
    observe_env_body<1, false, false, OBJ>(d, e, obs, flags, U.obs.m, U.obs.minb, d.obs_g);
  }
  // throughput mode (several envs per wave, one ego each, lidar): the rows of the wave's envs one after the other, each by the
  // whole wave -- same routine as the fused observation above, the env's scenario and map view read with wave-uniform addresses
  if (!ONE_ENV && !MARL && obs != nullptr && d.pack_obs) {
    step_sync();
    if (valid && leader) {
      const bool present = r.status == ST_PENDING || r.status == ST_ACTIVE || r.status == ST_DYING;
      S.x[slot] = r.x; S.y[slot] = r.y; S.ux[slot] = r.hx; S.uy[slot] = r.hy;
      S.spd[slot] = speed_kmh(r.v);
      S.hl[slot] = 0.5f * SPV.length;
      S.hw[slot] = (OBJ && SPV.kind == PGD_OBJ_CYLINDER) ? -1.0f : 0.5f * SPV.width;
      if (OBJ) s_kind[slot] = SPV.kind;
      S.present[slot] = present ? 1 : 0;
      if (s == 0) {
        AgentView& ag = s_ag[el];
        ag.x = r.x; ag.y = r.y; ag.th = r.th; ag.hx = r.hx; ag.hy = r.hy; ag.dl = r.dl; ag.dr = r.dr; ag.v = r.v;
        ag.steer = r.steer; ag.a0s = r.a0s; ag.a0t = r.a0t; ag.lhx = r.lasthx; ag.lhy = r.lasthy;
        ag.cur_first = r.cur_first; ag.cur_n = r.cur_n; ag.next_first = r.next_first;
        ag.blk = r.blk; ag.toll_time = r.php;
        ag.env = e; ag.slot = 0; ag.tick = steps_total;
        ag.cur_n |= scen << 8;  // the env's (possibly re-drawn) scenario travels with the view
      }
    }
    step_sync();
    if (valid) {  // the state blocks of all envs of the wave at once: the V lanes of an env share the 18 floats of its row
      AgentView ag = s_ag[el];
      ag.cur_n &= 0xff;
      state_block<STD>(d, mv, d.spawns[(size_t)scen * d.sstride], ag, obs + (size_t)e * d.ostride, s, V);
    }
    for (int q = 0; q < d.epw; ++q) {
      const int eq = unit * d.epw + q;  // wave-uniform
      if (eq >= N) break;
      AgentView ag = s_ag[q];
      const int scen_q = ag.cur_n >> 8;
      ag.cur_n &= 0xff;
      const MV mvq = map_view_as<MV>(d, cold.scen_map + scen_q);
      const int bq = q * V;
      const bool have = lane < V && d.cfg.num_lasers > 0;
      const int sl = bq + (lane < V ? lane : 0);
      const float t_step = d.cfg.dt * (float)d.cfg.decision_repeat;
      bool near_a = false;
      obs_compact<OBJ>(OL, lane, 0, have && S.present[sl], OBJ ? (have && s_kind[sl] == PGD_OBJ_VEHICLE) : true, S.x[sl], S.y[sl],
                       S.ux[sl], S.uy[sl], S.hl[sl], S.hw[sl], S.spd[sl], ag.x, ag.y, d.cfg.lidar_dist, ag.hx, ag.hy, d.cfg.num_lasers,
                       S.hl[bq] + S.hw[bq] + near_reach(ag.v, t_step), &near_a, t_step);
      {  // hint for the next step's contact tests of this env (EI_NEAR)
        const bool near_q = near_hint_usable(d.cfg) ? (__ballot(near_a) != 0ull) : true;
        if (lane == 0) d.ei[(size_t)eq * PGD_NEI + EI_NEAR] = near_q ? 1 : 0;
      }
      step_sync();
      observe_agent<OBJ, STD, false, false, true>(d, mvq, d.spawns[(size_t)scen_q * d.sstride], ag, OL, obs + (size_t)eq * d.ostride, lane, WAVE,
                                                  nullptr, nullptr, nullptr, lidar_minb(S));
      step_sync();
    }
  }
  // several envs per wave (small V) and an observation without a lidar (BASELINE config 2: dynamics + reward + state vector):
  // the row is the state block alone, written by the sub-lanes of the agent that has just been stepped
  if (!ONE_ENV && !MARL && obs != nullptr && !d.pack_obs && valid && s < A) {
    float* row = obs + (size_t)e * d.ostride + (size_t)s * d.D;
    if (r.status != ST_ACTIVE) {
      for (int k = g.sub; k < d.D; k += g.SUB) row[k] = 0.0f;
    } else {
      AgentView ag;
      ag.x = r.x; ag.y = r.y; ag.th = r.th; ag.hx = r.hx; ag.hy = r.hy; ag.dl = r.dl; ag.dr = r.dr; ag.v = r.v;
      ag.steer = r.steer; ag.a0s = r.a0s; ag.a0t = r.a0t; ag.lhx = r.lasthx; ag.lhy = r.lasthy;
      ag.cur_first = r.cur_first; ag.cur_n = r.cur_n; ag.next_first = r.next_first;
      ag.blk = r.blk; ag.toll_time = r.php;
      ag.env = e; ag.slot = s; ag.tick = steps_total;
      state_block<false>(d, mv, SPV, ag, row, g.sub, g.SUB);
    }
  }
  PHASE_MARK(14);  // fused observation
  XMARK(14);
  PHASE_END();
}

#undef SPV

#ifdef PGD_JIT
// The run-time build (hipcc --genco -DPGD_JIT -include <generated header>): this translation unit up to here plus ONE instantiation
// of the step kernel; the other kernels and the host side exist in the library only.
template __global__ void k_step<true, false, PGD_JIT_OBJ, PGD_JIT_STD, 9, false>(PgdDev, const float*, float*, uint8_t*, uint32_t*, float*, PgdCold);
#else

// heading vectors of the spawn poses, once per upload (the restart of a vehicle then evaluates no sincosf)
__global__ void k_spawn_hv(const pgd_spawn* __restrict__ sp, float2* __restrict__ hv, size_t n) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  float sn, cs;
  sincosf(sp[k].heading, &sn, &cs);
  hv[k] = make_float2(cs, sn);
}

// slot `s` of scenario `scen` right after a reset (base_env.py:269-301): spawn state + first localisation; agent ids restart
// at 0: id = number of spawned agent slots below this one (agent_manager.py:91-132).  Returns the ballot of spawned agents.
DEV unsigned long long reset_slot(const PgdDev& d, const LaneMap& lm, int scen, Veh& r) {
  const int A = d.A, s = lm.s;
  const Grp g{lm.sub, d.sub, lm.lead};
  const pgd_spawn* sp = d.spawns + (size_t)scen * d.sstride + s;
  MapView mv = map_view(d, d.scen[scen].map);
  reset_vehicle(*sp, d.spawn_hv[(size_t)scen * d.sstride + s], r, s, s < A && !d.cfg.idm_agent);
  RouteCtx ctx;
  if (r.status != ST_EMPTY) {
    route_refresh(mv, *sp, r);
    after_step_vehicle(d.cfg, mv, g, *sp, *sp, r, s < A, true, ctx);
  }
  const unsigned long long am = __ballot(lm.sub == 0 && s < A && r.status == ST_ACTIVE);  // epw == 1 whenever A > 1
  if (s < A && r.status == ST_ACTIVE) r.agent_id = A == 1 ? 0.0f : (float)__popcll(am & ((1ull << lm.lead) - 1ull));
  return am;
}

// the reset image: one record per (scenario, slot), read by the auto-reset of k_step; same lane mapping, unit = scenario
__global__ __launch_bounds__(WAVE) void k_reset_image(PgdDev d, RecPiece* __restrict__ img) {
  const LaneMap lm = lane_map(d, blockIdx.x, d.n_scen);
  if (!lm.valid) return;
  Veh r;
  reset_slot(d, lm, lm.e, r);
  if (lm.sub == 0) store_rec(rec_block(img, (size_t)lm.e, d.V), d.V, lm.s, r);
}

// multi-agent: the record of an agent right after it was (re)spawned from respawn record V + k of a scenario (spawn state, route
// context, first localisation, side distances, line / sidewalk flags) is a function of the scenario alone: built once per
// upload, one thread per record; the respawn of k_step copies it and sets the agent id (was: a second after_step + line test
// inside the step whenever any agent of the env entered, 7 k cycles of the wave)
__global__ __launch_bounds__(256) void k_respawn_image(PgdDev d, RecPiece* __restrict__ img) {
  const int n_extra = d.sstride - d.V;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= d.n_scen * n_extra) return;
  const int scen = k / n_extra, idx = d.V + k % n_extra;
  const Grp g{0, 1, (int)(threadIdx.x & (WAVE - 1))};
  const pgd_spawn* sp = d.spawns + (size_t)scen * d.sstride + idx;
  MapView mv = map_view(d, d.scen[scen].map);
  Veh r;
  reset_vehicle(*sp, d.spawn_hv[(size_t)scen * d.sstride + idx], r, idx, true);
  RouteCtx ctx;
  if (r.status != ST_EMPTY) {
    route_refresh(mv, *sp, r);
    after_step_vehicle(d.cfg, mv, g, *sp, *sp, r, true, true, ctx);
  }
  store_rec(rec_block(img, (size_t)scen, n_extra), n_extra, k % n_extra, r);
}

// reset of selected envs; same lane mapping as k_step, unit = position in the id list
__global__ __launch_bounds__(WAVE) void k_reset(PgdDev d, const int32_t* __restrict__ env_ids,
                                                 const int32_t* __restrict__ scen_ids, int n) {
  const int A = d.A;
  const LaneMap lm = lane_map(d, blockIdx.x, n);
  if (!lm.valid) return;
  const int k = lm.e, s = lm.s;
  const int e = env_ids ? env_ids[k] : k;
  const int scen = scen_ids[k];
  Veh r;
  const unsigned long long am = reset_slot(d, lm, scen, r);
  if (lm.sub != 0) return;
  store_veh(d, e, s, r);
  if (s == 0) {
    d.env_map[e] = d.scen_map[scen];
    if (d.bev_fill) d.bev_fill[e] = 1;
    d.imask[e] = ((d.epw == 1 || d.pack_obs) && d.use_imask) ? (d.V >= 64 ? ~0ull : ((1ull << d.V) - 1ull)) : 0ull;  // every record equals the image now
    d.ei[(size_t)(e) * PGD_NEI + EI_NEXT_AGENT] = A == 1 ? 1 : __popcll(am);
    d.ei[(size_t)(e) * PGD_NEI + EI_AUX] = d.scen[scen].aux;  // parking: free spaces of the new episode
    d.ei[(size_t)(e) * PGD_NEI + EI_SCEN] = scen;
    d.ei[(size_t)(e) * PGD_NEI + EI_NEXT_GROUP] = 0;
    d.ei[(size_t)(e) * PGD_NEI + EI_EP_STEPS] = 0;
    d.ei[(size_t)(e) * PGD_NEI + EI_NEAR] = 1;
    // EI_EPISODES / EI_STEPS_TOTAL are the counters of the device RNG streams (scenario re-draw on auto-reset, IDM timers,
    // lidar noise): they run on through pgd_reset, so a repeated env.reset() does not replay the same draws
  }
}

// Rebuilds the derived part of every record (heading vector, own-lane coordinate, route context) from its ABI fields and
// the current tables: after pgd_set_state and after a map / scenario upload while envs are running.
__global__ __launch_bounds__(256) void k_derive(PgdDev d) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= d.NV) return;
  Veh r;
  load_rec(rec_block(d.rec, (size_t)(k / d.V), d.V), d.V, k % d.V, r);
  if (r.hx == 0.0f && r.hy == 0.0f) sincosf(r.th, &r.hy, &r.hx);  // a checkpoint carries the heading vector (SF_HX / SF_HY)
  r.lon = 0.0f;
  r.road_cur = 0; r.road_next = 0; r.blk = 0; r.cur_first = 0; r.next_first = 0; r.cur_n = 0; r.next_n = 0;
  const int e = k / d.V;
  const int scen = d.ei[(size_t)e * PGD_NEI + EI_SCEN];
  if (k == e * d.V && scen >= 0 && scen < d.n_scen) d.env_map[e] = d.scen_map[scen];  // the env's copy of its map header
  if (r.status != ST_EMPTY && scen >= 0 && scen < d.n_scen && (int)r.spawn < d.sstride) {
    const MapView mv = map_view(d, d.scen[scen].map);
    const pgd_spawn& sp = d.spawns[(size_t)scen * d.sstride + r.spawn];
    if ((int)r.lane < mv.m->n_lanes) {
      float lat;
      lane_local(mv.lanes[r.lane], r.x, r.y, r.lon, lat);
    }
    if (r.ck0 < PGD_MAX_CKPT && r.ck1 < PGD_MAX_CKPT) route_refresh(mv, sp, r);
  }
  store_rec(rec_block(d.rec, (size_t)(k / d.V), d.V), d.V, k % d.V, r);
}

// engine.after_step on the current state (used after pgd_set_state)
__global__ __launch_bounds__(WAVE) void k_refresh(PgdDev d) {
  const int V = d.V, A = d.A, N = d.N;
  const LaneMap lm = lane_map(d, blockIdx.x, N);
  if (!lm.valid) return;
  const Grp g{lm.sub, d.sub, lm.lead};
  const int e = lm.e, s = lm.s;
  Veh r;
  load_veh(d, e, s, r);
  if (r.status != ST_ACTIVE && r.status != ST_PENDING && r.status != ST_DYING) return;
  int scen = d.ei[(size_t)(e) * PGD_NEI + EI_SCEN];
  MapView mv = map_view(d, d.scen[scen].map);
  RouteCtx ctx;
  after_step_vehicle(d.cfg, mv, g, d.spawns[(size_t)scen * d.sstride + r.spawn], d.spawns[(size_t)scen * d.sstride + r.spawn], r, s < A, true, ctx);
  if (lm.sub == 0) store_veh(d, e, s, r);
}

// ---------------------------------------------------------------------------------------------------------------------
// k_observe: stand-alone observation kernel, one block per (env, agent).  pgd_step fuses the observation into k_step when
// a wave carries exactly one env; this kernel serves pgd_reset / pgd_observe and the configurations that do not fuse.
// ---------------------------------------------------------------------------------------------------------------------
// OTH: PGD_MA_OTHERS_STATE rows (a kernel of its own: the neighbour-state path would cost the plain one registers)
// BLOCK threads produce one row.  BLOCK = 64: the block holds OBS_RPB independent rows, one per wave (a block per 64-lane
// row made the launch dispatch-bound: 32768 workgroups that each live ~5 us); BLOCK = 256: one row per block.
#define OBS_RPB 1
template <int BLOCK, bool OTH>
__global__ __launch_bounds__(BLOCK == WAVE ? WAVE * OBS_RPB : BLOCK) void k_observe(PgdDev d, float* __restrict__ obs,
                                                                                 const uint32_t* __restrict__ flags, int n_rows) {
  constexpr bool WROW = BLOCK == WAVE;
  __shared__ ObsLds Ls[WROW ? OBS_RPB : 1];
  const int V = d.V, A = d.A, D = d.D;
  const int rowi = WROW ? (int)blockIdx.x * OBS_RPB + (int)(threadIdx.x / WAVE) : (int)blockIdx.x;
  if (rowi >= n_rows) return;
  ObsLds& L = Ls[WROW ? threadIdx.x / WAVE : 0];
  const int e = rowi / A + d.unit_off * d.epw, a = rowi % A;
  const int tid = WROW ? (int)(threadIdx.x % WAVE) : (int)threadIdx.x;
  const RecPiece* recs = rec_block(d.rec, (size_t)e, V);  // the env's vehicle records
  float* row = obs + (size_t)e * d.ostride + (size_t)a * D;
  PHASE_INIT();
  // A row lives a few microseconds and almost all of that is load latency, so the reads go out in three batches instead of
  // one dependent chain.  Batch 1: every address that follows from the block index -- the observer's record, the first half
  // of body `tid`'s record (pose, speed, status, spawn index, agent id), the step flags, the env's scenario and step count.
  const int ob = tid < V ? tid : 0;
  Veh me;
  load_rec(recs, V, a, me);
  uint4 bw[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) bw[k] = recs[k * V + ob].q;
  const uint32_t fa = flags ? flags[(size_t)e * A + a] : 0u, fo = flags ? flags[(size_t)e * A + (tid < A ? tid : 0)] : 0u;
  const int scen = d.ei[(size_t)(e) * PGD_NEI + EI_SCEN];
  const uint32_t tick = (uint32_t)d.ei[(size_t)(e) * PGD_NEI + EI_STEPS_TOTAL];
  Veh body;  // only the first 64 bytes are filled
#pragma unroll
  for (int k = 0; k < 4; ++k) reinterpret_cast<uint4*>(&body)[k] = bw[k];
  // which slots get a row: after a multi-agent step the ones that reported or were (re)spawned, else the active ones
  bool want = me.status == ST_ACTIVE;
  if (flags) want = (fa & PGD_F_RESET) ? want : (fa & (PGD_F_REPORT | PGD_F_NEW)) != 0;  // after a reset only the new episode counts
  if (!want) {
    for (int k = tid; k < D; k += BLOCK) row[k] = 0.0f;
    return;
  }
  // batch 2: what the scenario and the spawn indices lead to -- map header, the observer's and the body's static parameters
  const pgd_spawn* spb = d.spawns + (size_t)scen * d.sstride;
  const pgd_spawn& msp = spb[me.spawn];
  const pgd_spawn& so = spb[body.spawn];
  const float so_len = so.length, so_wid = so.width;
  const int so_kind = so.kind;
  MapView mv = map_view_of(d, d.env_map + e);  // the env's own copy of the header: one dependent level less than via `scen`
  AgentView ag;
  ag.x = me.x; ag.y = me.y; ag.th = me.th;
  ag.hx = me.hx; ag.hy = me.hy;
  ag.dl = me.dl; ag.dr = me.dr; ag.v = me.v; ag.steer = me.steer;
  ag.a0s = me.a0s; ag.a0t = me.a0t; ag.lhx = me.lasthx; ag.lhy = me.lasthy;
  ag.cur_first = me.cur_first; ag.cur_n = me.cur_n; ag.next_first = me.next_first;
  ag.blk = me.blk; ag.toll_time = me.php;
  ag.env = e; ag.slot = a; ag.tick = tick;
  // batch 3 (lane records of the route) belongs to the state block, which needs nothing from the other bodies: it runs first
  // and its reads overlap the spawn reads the compaction waits for
  state_block<false>(d, mv, msp, ag, row, tid, BLOCK);
  PHASE_MARK(22);  // obs: state + navi block
  if (tid < WAVE) {  // wave 0: broad phase r = lidar distance (lidar.py:109-124), compacted into LDS
    bool present = false, is_vehicle = true;
    float x = 0, y = 0, ux = 1, uy = 0, hl = 0, hw = 0, spd = 0;
    if (tid < V && d.cfg.num_lasers > 0) {
      const int st = body.status;
      present = st == ST_PENDING || st == ST_ACTIVE || st == ST_DYING;
      bool still = st == ST_DYING;  // a finished agent is a static body (zero velocity)
      if (flags && tid < A) {
        // multi-agent step: rows of agents that drove this step show the world before the finishes / respawns
        // (base_env.py:303-344 runs before multi_agent_pgdrive.py:128-141); an agent spawned this step sees the world at
        // its spawn time, i.e. the earlier spawns of the step only
        if (fa & PGD_F_RESET) {
        } else if (fa & PGD_F_NEW) {
          present = present && (!(fo & PGD_F_NEW) || body.agent_id < me.agent_id);
        } else {
          present = (fo & PGD_F_REPORT) || (present && !(fo & PGD_F_NEW));
          still = still && !(fo & PGD_F_REPORT);
        }
      }
      x = body.x; y = body.y;
      ux = body.hx; uy = body.hy;
      hl = 0.5f * so_len; hw = so_kind == PGD_OBJ_CYLINDER ? -1.0f : 0.5f * so_wid;
      is_vehicle = so_kind == PGD_OBJ_VEHICLE;
      spd = still ? 0.0f : speed_kmh(body.v);
    }
    obs_compact<true>(L, tid, a, present, is_vehicle, x, y, ux, uy, hl, hw, spd, ag.x, ag.y, d.cfg.lidar_dist, ag.hx, ag.hy,
                      d.cfg.num_lasers);
  }
  row_sync<WROW>();
  PHASE_MARK(28);  // k_observe: compaction
  if (OTH) observe_agent<true, false, true, false, WROW>(d, mv, msp, ag, L, row, tid, BLOCK, recs, spb);
  else observe_agent<true, false, false, false, WROW>(d, mv, msp, ag, L, row, tid, BLOCK);
  PHASE_END_AT(29);
}

// ---------------------------------------------------------------------------------------------------------------------
// k_observe_env: the rows of ALL agents of an env by one wave (multi-agent engines; same results as k_observe, row by row).
// A block per row spends its life waiting for a handful of loads, 8 x A of them per env.  Here the env's records are read
// once, and the work is laid out by what there is to do instead of by row:
//   state blocks   WAVE / A lanes per agent, every agent at once (state_block with few threads);
//   pairs          lane = (observer, body): broad phase, beam window, neighbour rank -- WAVE / V observers per pass;
//   lidar          the (observer, body, beam-inside-the-window) incidences of the pass, flattened by a prefix sum over the
//                  pairs' window sizes and dealt out to the lanes 64 at a time: a body is tested against the few beams that
//                  can reach it and nothing else; the nearest hit per beam is an unsigned min in LDS (fractions are >= 0).
// ---------------------------------------------------------------------------------------------------------------------
// NW waves per env: the state blocks get NW * WAVE / A lanes per agent and the passes of the pair phase are dealt out to the waves
// (wave w takes passes w, w + NW, ...; each wave has its own scratch and synchronises with itself only).  NW = 4 when there
// are at least four passes (A >= 4 * (WAVE / V)), else 1.
// NW = 4 when the pair phase has at least four passes (A >= 4 * (WAVE / V)), else 1.
// FIX: the engine runs the default multi-agent configuration (same constants as k_step's instantiation for it, PGD_FIXM_FIELDS)
// STATE = false: k_step has written the state blocks of the rows that are due (PgdDev::state_rows): the pairwise part only
template <int NW, bool FIX = false, bool STATE = true, int SEATS = 0>  // SEATS: the seat count folded as well (PGD_FIXM_SEAT_FIELDS)
// (the library is built at -O2 since the end of round 5; this kernel keeps the size-optimised code it had -- 30.0 against 30.7 us for the
// 40 seats -- and its specialised instantiations seven waves per SIMD: 72 registers, what -Os gave them unasked; at -O2 they took 82 and
// the observation 32.6 us)
#ifndef PGD_KOE_ATTR
#define PGD_KOE_ATTR __attribute__((minsize))
#endif
__global__ PGD_KOE_ATTR __launch_bounds__(WAVE * NW, (FIX ? 7 : 1)) void k_observe_env(PgdDev d, float* __restrict__ obs, const uint32_t* __restrict__ flags, int G) {
  if (FIX) write_fixed_config<true, true, false, (SEATS ? SEATS : 1)>(d);
  extern __shared__ unsigned s_minb_dyn[];
  constexpr int CAP = SEATS ? (SEATS / 1000 + 15) / 16 * 16 : WAVE;
  __shared__ ObsEnvLds<NW, CAP> M;
  PHASE_INIT();  // (profile builds: the marks of observe_env_body count from here)
  observe_env_body<NW, !FIX, false, !FIX, STATE, CAP>(d, (int)blockIdx.x + d.unit_off * d.epw, obs, flags, M, s_minb_dyn, G);  // (the fixed-config kernel: no traffic objects)
}

// scripted lane-keeping policy (pgd_lane_keep_actions): one thread per env
__global__ __launch_bounds__(256) void k_lane_keep(PgdDev d, const float* __restrict__ obs, float* __restrict__ act, float k_lat,
                                                  float k_head, float v_target, float noise, uint32_t tick) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= d.N) return;
  const float* o = obs + (size_t)e * d.D;
  const float2 a = lane_keep_action(d.cfg.seed, d.cfg.env_base + e, o[0], o[1], o[2], o[3], k_lat, k_head, v_target, noise, tick);
  act[(size_t)e * 2 + 0] = a.x;
  act[(size_t)e * 2 + 1] = a.y;
}

__global__ void k_clear_hints(int32_t* ei, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) ei[(size_t)e * PGD_NEI + EI_NEAR] = 1;
}

struct pgd_engine {
  PgdDev d;
  int device;
  hipStream_t stream;
  bool own_stream;
  hipStream_t retired;  // the engine's own stream after pgd_set_stream moved it away
  hipEvent_t ev0, ev1;
  bool ev_valid;
  hipEvent_t ev_move;   // pgd_set_stream: orders the old stream before the new one
  hipEvent_t ev_ids;    // pgd_reset: the pinned id staging buffer has been consumed
  int32_t* h_ids;       // pinned staging [2N] of pgd_reset's host id lists (no stream synchronisation per reset)
  bool ids_pending;
  pgd_map* maps; pgd_lane* lanes; pgd_road* roads; pgd_box* boxes; int32_t* cell_start; int32_t* cell_items;
  pgd_box* cell_boxes;
  LaneExt* cell_ext;
  LaneNav* lane_nav;
  float2* spawn_hv;
  pgd_map* scen_map;  // per scenario: copy of its map header (saves one dependent load per block)
  float2* beam;       // lidar beam directions in the vehicle frame
  RecPiece* reset_img;  // [n_scen] blocks of V records, rebuilt after every map / scenario upload
  RecPiece* respawn_img;  // [n_scen] blocks of sstride - V records (multi-agent), rebuilt with it
  bool img_dirty;
  std::vector<pgd_map>* h_maps;
  std::vector<pgd_scenario>* h_scen;
  pgd_scenario* scen; pgd_spawn* spawns;
  int32_t* d_ids;  // scratch [2N]
  bool have_maps, have_scen;
  // per-kernel HIP-event profile of pgd_step launches (bench.py roofline numbers)
  std::vector<hipEvent_t>* prof_ev;  // 3 events per recorded step
  int prof_cap, prof_n, prof_stride, prof_tick;
  bool prof_grouped;
  struct pgd_topdown_state* topdown;  // top-down observation (pgd_topdown.h), null until pgd_topdown_enable
  struct pgd_render_state* render;    // top-down scene rendering (pgd_render.h), null until pgd_render_enable
  int n_groups;          // env groups of pgd_set_groups (1 = none)
  hipStream_t* gstreams; // [n_groups] internal streams
  bool derive_pending;  // records were written through the ABI or the tables changed: k_derive has to run
  bool has_objects;  // some spawn record is a traffic object (pgd_upload_scenarios): selects the OBJ kernels
  bool step_timing;  // record ev0 / ev1 around every step (pgd_last_step_ms)
  bool row_observe;  // PGD_ROW_OBSERVE was set when the engine was created (debug / A-B: k_observe per row instead of k_observe_env)
  const char* last_step_kernel;  // what the last pgd_step* call launched (pgd_describe_step)
  // a step kernel built at run time for this handle's configuration (pgd_set_step_module): launched instead of the general kernel
  // while the engine's geometry and object flag are what it was built for
  hipModule_t jit_mod;
  hipFunction_t jit_fn;
  bool jit_obj, jit_force;
  bool mlp_attr[4];  // pgd_mlp_policy / pgd_mlp_policy_prepared: the kernel's dynamic LDS limit has been raised on this engine's device
  int jit_geom[4];   // sub, epw, pack_obs, use_imask at the time of the build
  char jit_name[96];
  bool no_fix;       // PGD_NO_FIX: never pick the kernel specialised for the default configuration (A/B, debugging)
  bool no_fuse;      // PGD_NO_FUSE was set when the engine was created (debug: always run the stand-alone k_observe)
  bool prof_fused;
  bool no_state_in_step;  // PGD_NO_STATE_IN_STEP was set when the engine was created (A/B: the state blocks stay in k_observe_env)
  int imask_env;        // PGD_NO_IMASK / PGD_IMASK: 0 / 1 force the reset-image reads off / on, -1 = by mode (PgdDev::use_imask)
  bool left_pack_mode;  // pgd_set_groups switched the engine from throughput mode back to one env per wave (reported by pgd_describe_step)
  ulonglong2* rowz;  // multi-agent engines: PgdDev::rowz (zero-row marks + the tag of the buffer they describe, per env)
  struct { const float* obs; float k_lat, k_head, v_target, noise; uint32_t tick; } lk;  // pgd_step_lane_keep: this launch's scripted policy (obs null: none)
  float* lk_act;     // pgd_step_lane_keep on engines that cannot take the policy into the step kernel: the actions in between
};

// The default row layout (see observe_agent): the STD instantiations of k_step
static bool std_rows(const pgd_config& c) {
  return c.side_lasers == 0 && c.lane_line_lasers == 0 && !c.random_agent_model && c.lidar_gaussian_noise <= 0.0f &&
         c.lidar_dropout_prob <= 0.0f;
}

// The engines a step kernel built at run time can serve at all (pgd_set_step_module): single agent, one env per wave
static bool jit_geometry_ok(const pgd_engine* h) { return !(h->d.cfg.marl_flags & PGD_MA_ENABLED) && h->d.epw == 1 && !h->d.pack_obs; }

// Env group `group` of pgd_set_groups: envs [first, first + count) on the group's stream; -1 = all envs on the engine stream
struct EnvGroup { int first, count; hipStream_t stream; };
static int env_group(const pgd_engine* h, int group, EnvGroup& g) {
  g = {0, h->d.N, h->stream};
  if (group < 0) return PGD_OK;
  if (group >= h->n_groups || !h->gstreams) return PGD_ERR_ARG;
  g.count = h->d.N / h->n_groups;
  g.first = group * g.count;
  g.stream = h->gstreams[group];
  return PGD_OK;
}

using StepFn = void (*)(PgdDev, const float*, float*, uint8_t*, uint32_t*, float*, PgdCold);
using ObsFn = void (*)(PgdDev, float*, const uint32_t*, int);
// The multi-agent instantiations with the seat count folded (PGD_FIXM_SEAT_FIELDS; code = seats x 1000 + beams).  40 and 44 seats
// observe with k_observe_env<4> after the step (before / after k_step wrote the state blocks); 8 seats fuse the observation into k_step.
struct SeatKernels { int code; StepFn step; const char* name; ObsFn observe, observe_after_state; };
static const SeatKernels SEAT_KERNELS[] = {
    {40072, k_step<true, true, false, false, 40072>,
     "k_step: one env per wave, specialised for the default multi-agent configuration with 40 agent seats x 72 beams",
     k_observe_env<4, true, true, 40072>, k_observe_env<4, true, false, 40072>},
    {44072, k_step<true, true, false, false, 44072>,
     "k_step: one env per wave, specialised for the default multi-agent configuration with 44 agent seats x 72 beams",
     k_observe_env<4, true, true, 44072>, k_observe_env<4, true, false, 44072>},
    {8072, k_step<true, true, false, false, 8072>,
     "k_step: one env per wave, specialised for the default multi-agent configuration with 8 agent seats x 72 beams", nullptr, nullptr},
    {8240, k_step<true, true, false, false, 8240>,
     "k_step: one env per wave, specialised for the default multi-agent configuration with 8 agent seats x 240 beams", nullptr, nullptr},
};
// which of them (null = none) an engine that passed FIXK_MARL can run
static const SeatKernels* marl_fix_seats(const PgdDev& d) {
  for (const SeatKernels& s : SEAT_KERNELS) {
    bool ok = true;
#define PGD_F_TEST(f, v) ok = ok && (f == v);
    PGD_FIXM_SEAT_FIELDS(PGD_F_TEST, d, d.cfg, s.code / 1000, s.code % 1000)
#undef PGD_F_TEST
    if (ok) return &s;
  }
  return nullptr;
}

// FIX 1 with one env per wave: the reference's default single-agent configuration
static bool default_one_env(const pgd_engine* h) { return !h->has_objects && !h->no_fix && fix_config_matches(h->d, true); }
// the engines whose step kernel has an instantiation with the scripted policy inside: the FIX 1 case, the row fused into the step
static bool lane_keep_in_step(const pgd_engine* h) { return default_one_env(h) && !h->no_fuse; }

// A k_step instantiation, its pgd_describe_step text, and whether it was built for one configuration (write_fixed_config: a run-time
// kernel does not take its place).
struct StepKernel { StepFn fn; const char* name; bool specialised; };
// The instantiation a step launches: the first case that holds, evaluated per step (pgd_set_groups and the uploads change
// what it reads).  A specialised case holds only where fix_config_matches() does, so its results are the general kernel's; the
// PGD_FIX*_FIELDS lists pin the geometry, the multi-agent flags and the row layout, and a case adds what they cannot: the object
// flag and PGD_NO_FIX (A/B: never specialised).  Reads h->d: step_impl's launch copy differs in no field of those lists.
static StepKernel step_kernel(const pgd_engine* h) {
  const PgdDev& d = h->d;
  const bool obj = h->has_objects, fix = !h->no_fix;
  const char* general = d.pack_obs ? "k_step: whole envs side by side in a wave, one vehicle per lane (throughput mode)"
                                   : (d.epw == 1 ? "k_step: one env per wave" : "k_step: several envs per wave");
  if (d.cfg.marl_flags & PGD_MA_ENABLED) {
    if (!obj && fix && fix_config_matches(d, true, FIXK_MARL) && d.V == d.A && d.sub == WAVE / d.A) {
      if (const SeatKernels* s = marl_fix_seats(d)) return {s->step, s->name, true};
      return {k_step<true, true, false, false, 1>, "k_step: one env per wave, specialised for the default multi-agent configuration", true};
    }
    return {obj ? k_step<true, true, true> : k_step<true, true, false>, general, false};  // (objects = toll booths)
  }
  if (d.epw == 1) {
    if (h->lk.obs && lane_keep_in_step(h))
      return {k_step<true, false, false, true, 1, true>,
              "k_step: one env per wave, specialised for the default single-agent configuration, scripted lane-keeping policy inside", true};
    if (obj && fix && fix_config_matches(d, true, FIXK_SAFE))
      return {k_step<true, false, true, true, 4>,
              "k_step: one env per wave, specialised for the SafePGDriveEnv configuration (16 traffic + 40 object slots, run-time reward scheme)", true};
    if (!obj && fix && fix_config_matches(d, true, FIXK_NO_LIDAR))
      return {k_step<true, false, false, true, 3>, "k_step: one env per wave, specialised for the top-down envs' configuration (single agent, lidar off)", true};
    if (default_one_env(h)) return {k_step<true, false, false, true, 1>, "k_step: one env per wave, specialised for the default single-agent configuration", true};
    if (!obj && fix && fix_config_matches(d, true, FIXK_GEOMETRY))
      return {k_step<true, false, false, true, 2>,
              "k_step: one env per wave, specialised for the default single-agent configuration with a run-time reward scheme", true};
    return {obj ? k_step<true, false, true> : (std_rows(d.cfg) ? k_step<true, false, false, true> : k_step<true, false, false>), general, false};
  }
  if (obj) return {k_step<false, false, true>, general, false};
  if (fix && fix_config_matches(d, false, FIXK_EGO_ONLY))
    return {k_step<false, false, false, false, 1>, "k_step: several envs per wave, specialised for the ego-only configuration without a lidar", true};
  if (fix && fix_config_matches(d, false))
    return {k_step<false, false, false, true, 1>,
            "k_step: whole envs side by side in a wave (throughput mode), specialised for the default single-agent configuration", true};
  return {(d.pack_obs && std_rows(d.cfg)) ? k_step<false, false, false, true> : k_step<false, false, false>, general, false};
}

// Rows written by a kernel that does not keep the zero-row marks (k_observe, one block per row): what the marks say about this
// buffer may no longer hold -- forget them (a memset node when the stream is being captured: every replay forgets again).
static int obs_rows_forget(pgd_engine* h, hipStream_t stream) {
  if (!h->rowz) return PGD_OK;
  HIPCHK(hipMemsetAsync(h->rowz, 0, sizeof(ulonglong2) * (size_t)h->d.N, stream));
  return PGD_OK;
}

static void topdown_free(pgd_engine* h);
static void render_free(pgd_engine* h);
static void render_mark_stale(pgd_engine* h);
static int render_forget(pgd_engine* h, const int32_t* d_env, int n);

template <typename T>
static int upload(T** dst, const T* src, size_t n, hipStream_t st) {
  if (*dst) { HIPCHK(hipFree(*dst)); *dst = nullptr; }
  HIPCHK(hipMalloc(dst, sizeof(T) * (n ? n : 1)));
  if (n) HIPCHK(hipMemcpyAsync(*dst, src, sizeof(T) * n, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return PGD_OK;
}

static int build_scen_map(pgd_engine* h) {
  if (!h->h_maps || !h->h_scen) return PGD_OK;
  std::vector<pgd_map> sm(h->h_scen->size());
  for (size_t k = 0; k < sm.size(); ++k) {
    int m = (*h->h_scen)[k].map;
    if (m < 0 || m >= (int)h->h_maps->size()) return PGD_ERR_ARG;
    sm[k] = (*h->h_maps)[m];
  }
  int rc = upload(&h->scen_map, sm.data(), sm.size(), h->stream);
  if (rc) return rc;
  h->d.scen_map = h->scen_map;
  return PGD_OK;
}

// rebuild the derived part of the records (needs maps + scenarios; deferred until both are there)
static int derive_records(pgd_engine* h) {
  if (!h->derive_pending || !h->have_maps || !h->have_scen) return PGD_OK;
  hipLaunchKernelGGL(k_derive, dim3((h->d.NV + 255) / 256), dim3(256), 0, h->stream, h->d);
  HIPCHK(hipGetLastError());
  h->derive_pending = false;
  return PGD_OK;
}

// (re)build the reset image once both the maps and the scenarios are on the device
static void topdown_mark_dirty(pgd_engine* h);
static int build_reset_image(pgd_engine* h) {
  if (!h->have_maps || !h->have_scen) return PGD_OK;
  topdown_mark_dirty(h);  // the top-down rasters follow the tables
  render_mark_stale(h);   // and so do the rendered backgrounds (pgd_render_enable again)
  // the route context cached in the records of running envs refers to the tables: rebuild it after every upload
  h->derive_pending = true;
  { int rc = derive_records(h); if (rc) return rc; }
  if (!h->img_dirty) return PGD_OK;
  if (h->reset_img) { HIPCHK(hipFree(h->reset_img)); h->reset_img = nullptr; }
  HIPCHK(hipMalloc(&h->reset_img, sizeof(VehRec) * (size_t)h->d.n_scen * h->d.V));
  h->d.reset_img = h->reset_img;
  const int blocks = (h->d.n_scen + h->d.epw - 1) / h->d.epw;
  hipLaunchKernelGGL(k_reset_image, dim3(blocks), dim3(WAVE), 0, h->stream, h->d, h->reset_img);
  HIPCHK(hipGetLastError());
  if (h->respawn_img) { HIPCHK(hipFree(h->respawn_img)); h->respawn_img = nullptr; }
  h->d.respawn_img = nullptr;
  if (h->d.sstride > h->d.V) {
    const size_t n = (size_t)h->d.n_scen * (h->d.sstride - h->d.V);
    HIPCHK(hipMalloc(&h->respawn_img, sizeof(VehRec) * n));
    h->d.respawn_img = h->respawn_img;
    hipLaunchKernelGGL(k_respawn_image, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d, h->respawn_img);
    HIPCHK(hipGetLastError());
  }
  h->img_dirty = false;
  return PGD_OK;
}

extern "C" {

const char* pgd_version(void) { return "pgdrive_hip 0.1 (gfx950)"; }
#ifndef PGD_SOURCE_SHA
#define PGD_SOURCE_SHA "unstamped"  // (an experimental build outside pgdrive_amd/build.py: no committed counter pass is its own)
#endif
const char* pgd_source_sha(void) { return PGD_SOURCE_SHA; }

int pgd_obs_dim(const pgd_config* c) {
  const int toll = (c->marl_flags & PGD_MA_TOLLGATE) != 0;
  const int state = (c->side_lasers > 0 ? c->side_lasers : 2) + 6 + c->lane_line_lasers + (c->random_agent_model ? 2 : 0) +
                    (toll ? 0 : PGD_NAVI_DIM);
  const int per_other = (c->marl_flags & PGD_MA_OTHERS_STATE) ? state : 4;
  return state + per_other * c->num_others + c->num_lasers + (toll ? 2 : 0);
}

int pgd_create(const pgd_config* cfg, int device, void* hip_stream, pgd_handle* out) {
  if (!cfg || !out) return PGD_ERR_ARG;
  int V = cfg->num_agents + cfg->num_traffic;
  if (cfg->num_envs <= 0 || cfg->num_agents <= 0 || V > MAXV || cfg->num_others > 16 || cfg->num_lasers < 0) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(device));
  pgd_engine* h = (pgd_engine*)calloc(1, sizeof(pgd_engine));
  h->device = device;
  h->no_fuse = getenv("PGD_NO_FUSE") != nullptr;
  h->no_fix = getenv("PGD_NO_FIX") != nullptr;
  h->jit_force = getenv("PGD_JIT_FORCE") != nullptr;
  h->row_observe = getenv("PGD_ROW_OBSERVE") != nullptr;
  h->no_state_in_step = getenv("PGD_NO_STATE_IN_STEP") != nullptr;
  h->d.cfg = *cfg;
  h->d.N = cfg->num_envs; h->d.A = cfg->num_agents; h->d.T = cfg->num_traffic; h->d.V = V;
  h->d.D = pgd_obs_dim(cfg);
  h->d.NV = h->d.N * V;
  h->d.ostride = h->d.A * h->d.D;
  h->d.prow = nullptr;
  h->d.dbg_exit = 255;  // no exit mark, no ablation bits (exit-profile builds only)
  h->d.unit_off = 0;
  h->n_groups = 1;
  const bool marl = (cfg->marl_flags & PGD_MA_ENABLED) != 0;
  // multi-agent engines have no IDM traffic; num_traffic slots may hold static bodies (toll booths, group PGD_GROUP_NEVER)
  if (marl && (cfg->respawn_places < 0 || cfg->respawn_places > 64 || cfg->respawn_dests < 0)) return PGD_ERR_ARG;  // (free places: one 64-bit mask)
  if (cfg->idm_agent && (marl || cfg->num_agents != 1)) return PGD_ERR_ARG;  // the agent's PID / routing fields double as multi-agent bookkeeping
  if (marl && cfg->horizon > 0x7fff) return PGD_ERR_ARG;  // the per-agent episode length is a 16-bit field of the record
  h->d.sstride = V + (marl ? cfg->respawn_places * cfg->respawn_dests : 0);
  h->d.sub = WAVE / V < 16 ? WAVE / V : 16;  // sub-lanes per vehicle
  h->d.epw = marl ? 1 : WAVE / (V * h->d.sub);  // whole environments per wave (the multi-agent tail needs the env alone in its wave)
  // Throughput mode: at large N the step is bound by instruction issue, not by the latency of one wave (profiles/r02_sweep.md:
  // 4.2 ns per env-step from 32768 envs on), and the SUB lanes of a vehicle run its scalar phases redundantly.  Engines with
  // >= 32768 single-ego envs (PGD_PACK=1 / 0 overrides; measured against the one-env kernel, profiles/r03_sweep.md: -7 % at 16384 envs, +6 % at 32768, +18 % at 262144) carry one vehicle per lane and as many whole envs per wave as fit --
  // three at V = 17 -- with the lidar observation of each env appended to the same launch.
  {
    const char* pk = getenv("PGD_PACK");
    const int epw1 = std::min(WAVE / V, FUSE_MAX_AGENTS);
    const bool can = !marl && cfg->num_agents == 1 && cfg->num_traffic >= 1 && epw1 >= 2 && epw1 * V <= PGD_SUBV && cfg->num_lasers > 0;
    const bool want = pk ? atoi(pk) != 0 : cfg->num_envs >= 32768;
    if (can && want) { h->d.sub = 1; h->d.epw = epw1; h->d.pack_obs = 1; }
  }
  if (hip_stream) { h->stream = (hipStream_t)hip_stream; h->own_stream = false; }
  else { HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)); h->own_stream = true; }
  HIPCHK(hipEventCreate(&h->ev0));
  HIPCHK(hipEventCreate(&h->ev1));
  HIPCHK(hipEventCreateWithFlags(&h->ev_move, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&h->ev_ids, hipEventDisableTiming));
  HIPCHK(hipHostMalloc((void**)&h->h_ids, sizeof(int32_t) * (size_t)cfg->num_envs * 2, hipHostMallocDefault));
  size_t nv = (size_t)h->d.NV;
  HIPCHK(hipMalloc(&h->d.rec, sizeof(VehRec) * nv));
  HIPCHK(hipMalloc(&h->d.ei, sizeof(int32_t) * (size_t)h->d.N * PGD_NEI));
  HIPCHK(hipMalloc(&h->d_ids, sizeof(int32_t) * (size_t)h->d.N * 2));
  HIPCHK(hipMemsetAsync(h->d.rec, 0, sizeof(VehRec) * nv, h->stream));
  HIPCHK(hipMemsetAsync(h->d.ei, 0, sizeof(int32_t) * (size_t)h->d.N * PGD_NEI, h->stream));
  if (marl) {
    // PGD_NO_ROWZ=1: no marks -- every row that is not due is zero-filled by every call (callers that edit the returned rows in place)
    if (!getenv("PGD_NO_ROWZ") || getenv("PGD_NO_ROWZ")[0] == '0') {
      HIPCHK(hipMalloc(&h->rowz, sizeof(ulonglong2) * (size_t)h->d.N));
      HIPCHK(hipMemsetAsync(h->rowz, 0, sizeof(ulonglong2) * (size_t)h->d.N, h->stream));
      h->d.rowz = h->rowz;
    }
  }
  HIPCHK(hipMalloc(&h->d.env_map, sizeof(pgd_map) * (size_t)h->d.N));
  HIPCHK(hipMemsetAsync(h->d.env_map, 0, sizeof(pgd_map) * (size_t)h->d.N, h->stream));
  // never-written slots are read from the scenario's reset image (cache resident, shared by every env of the scenario) instead
  // of the env's own record: halves the HBM bytes of a step and is worth +13 % at 262144 envs.  THROUGHPUT MODE ONLY (several envs
  // per wave, from 32768 envs on): with one env per wave the step is bound by its chain of memory round trips, and the mask is one
  // of them -- mask + scenario id -> records -> ...; without it the records' reads go out at once (round 5: 4096 envs 17.38 -> 17.12 us,
  // 16384 envs 47.3 -> 46.8, 8 agents 22.4 -> 22.1, 40 seats' step 27.7 -> 27.0; 32768 envs in throughput mode 77.2 -> 77.7 without
  // the image).  PGD_NO_IMASK=1 / PGD_IMASK=1 force it off / on (A/B; the specialised kernels are compiled for the default).
  h->imask_env = getenv("PGD_NO_IMASK") ? 0 : (getenv("PGD_IMASK") ? 1 : -1);
  h->d.use_imask = h->imask_env >= 0 ? h->imask_env : (h->d.pack_obs ? 1 : 0);
  HIPCHK(hipMalloc(&h->d.imask, sizeof(unsigned long long) * (size_t)h->d.N));
  HIPCHK(hipMemsetAsync(h->d.imask, 0, sizeof(unsigned long long) * (size_t)h->d.N, h->stream));
  {
    // beam i points at theta + i * 2 pi / n (distance_detector.py:65-94): its direction is the heading rotated by a
    // constant angle, tabulated once in double precision instead of one sincosf per beam and step
    std::vector<float2> bt((size_t)(cfg->num_lasers > 0 ? cfg->num_lasers : 1));
    for (int i = 0; i < cfg->num_lasers; ++i) {
      const double a = (double)i * (2.0 * 3.14159265358979323846 / (double)cfg->num_lasers);
      bt[(size_t)i] = make_float2((float)cos(a), (float)sin(a));
    }
    int rc = upload(&h->beam, bt.data(), bt.size(), h->stream);
    if (rc) return rc;
    h->d.beam = h->beam;
  }
  *out = h;
  return PGD_OK;
}

int pgd_upload_maps(pgd_handle h, const pgd_map* maps, int n_maps, const pgd_lane* lanes, int n_lanes,
                    const pgd_road* roads, int n_roads, const pgd_box* boxes, int n_boxes, const int32_t* cs, int n_cs,
                    const int32_t* ci, int n_ci) {
  if (!h || !maps || n_maps <= 0) return PGD_ERR_ARG;
  for (int m = 0; m < n_maps; ++m)  // packed ids of the device record: 12-bit road ids, 16-bit lane ids
    if (maps[m].n_roads > 4095 || maps[m].n_lanes > 65535) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = upload(&h->maps, maps, n_maps, h->stream))) return rc;
  {
    // device copy of the lane table: `pad` carries the lane count of the lane's road (the lanes of a road are consecutive,
    // so neighbour lanes follow from the lane id alone: no road-record read in the IDM neighbour search)
    std::vector<pgd_lane> dl(lanes, lanes + n_lanes);
    for (int m = 0; m < n_maps; ++m)
      for (int k = 0; k < maps[m].n_lanes; ++k) {
        pgd_lane& L = dl[(size_t)maps[m].lane_off + k];
        if (L.road < 0 || L.road >= maps[m].n_roads) return PGD_ERR_ARG;
        const pgd_road& R = roads[maps[m].road_off + L.road];
        if (R.first_lane + L.index != k) return PGD_ERR_ARG;
        L.pad = R.n_lanes;
        // device-private use of `ex` (the end point is not read on the device): half-width of the strip around a straight
        // lane's axis that no line / sidewalk box of the map reaches.  The lateral coordinate is linear over a box, so its
        // extremes sit at the corners; a box with corners on both sides crosses.  A car whose box stays inside that strip AND
        // between the lane's ends touches nothing: k_step then skips the line / sidewalk test.  Boxes that lie wholly before the
        // lane's start or behind its end (5 cm of slack for the fp32 coordinate on the device) cannot reach such a car -- the lane's
        // direction separates them -- and do not count: rounds 2 - 4 counted everything within 6 m of the ends, and the first
        // piece of a curved line behind a junction then voided the strip of a QUARTER of the straight lane length of the
        // PGDrive-v0 maps and of every entry road of the multi-agent roundabout (where most agents of a random policy live).
        double clear = 0.0;
#ifdef PGD_NO_STRIP
        if (false) {
#else
        if (L.dir == 0.0f) {
#endif
          clear = 1e9;
          const pgd_map& M = maps[m];
          for (int b = 0; b < M.n_boxes && clear > 0.0; ++b) {
            const pgd_box& B = boxes[M.box_off + b];
            if (B.kind == PGD_BOX_LANE) continue;
            double lo_lon = 1e30, hi_lon = -1e30, lo_lat = 1e30, hi_lat = -1e30;
            for (int q = 0; q < 4; ++q) {
              const double sl = (q & 1) ? 1.0 : -1.0, sw = (q & 2) ? 1.0 : -1.0;
              const double px = B.cx + sl * B.hl * B.ux - sw * B.hw * B.uy, py = B.cy + sl * B.hl * B.uy + sw * B.hw * B.ux;
              const double dx = px - L.ax, dy = py - L.ay;
              const double lon = dx * L.bx + dy * L.by, lat = dy * L.bx - dx * L.by;
              lo_lon = std::min(lo_lon, lon); hi_lon = std::max(hi_lon, lon);
              lo_lat = std::min(lo_lat, lat); hi_lat = std::max(hi_lat, lat);
            }
            if (hi_lon < -0.05 || lo_lon > (double)L.length + 0.05) continue;  // (the car lies within [0, length]: see below)
            if (lo_lat <= 0.0 && hi_lat >= 0.0) clear = 0.0;
            else clear = std::min(clear, std::min(std::fabs(lo_lat), std::fabs(hi_lat)));
          }
          clear = clear > 1e8 ? 0.0 : std::max(0.0, clear - 0.03);  // 3 cm of slack for the fp32 forms on the device
        }
        L.ex = (float)clear;
        L.ey = 0.0f;  // (the bits of the related-lanes mask, below)
      }
    // device-private use of `ey`: the 32-bit set { id & 31 } over the lane itself, its successors and its predecessors (the lanes
    // whose successor list holds it) -- every lane an object must be on to count in the IDM front / back search of this lane
    // (FrontBackObjects: same lane, successor lane, predecessor lane; idm_policy.py:107-131).  find_front_back drops the other
    // bodies of the broad phase with one shift per body before its search loop; a superset (ids collide mod 32) keeps it exact.
    for (int m = 0; m < n_maps; ++m) {
      std::vector<uint32_t> rel((size_t)maps[m].n_lanes, 0u);
      for (int k = 0; k < maps[m].n_lanes; ++k) {
        const pgd_lane& L = dl[(size_t)maps[m].lane_off + k];
        rel[(size_t)k] |= 1u << (k & 31);
        for (int q = 0; q < PGD_MAX_SUCC; ++q) {
          const int sid = L.succ[q];
          if (sid < 0 || sid >= maps[m].n_lanes) continue;
          rel[(size_t)k] |= 1u << (sid & 31);
          rel[(size_t)sid] |= 1u << (k & 31);
        }
      }
      for (int k = 0; k < maps[m].n_lanes; ++k) memcpy(&dl[(size_t)maps[m].lane_off + k].ey, &rel[(size_t)k], 4);
      // device-private use of `pad`: the from-node of the lane's road -- what Navigation._update_target_checkpoints looks up in the
      // route (navigation.py:262-282); with it in the lane record the checkpoint test needs no lane -> road table chain (two
      // dependent reads per vehicle on every step of the first five metres of a lane: round 6)
      for (int k = 0; k < maps[m].n_lanes; ++k) {
        pgd_lane& L = dl[(size_t)maps[m].lane_off + k];
        L.pad = (L.road >= 0 && L.road < maps[m].n_roads) ? roads[(size_t)maps[m].road_off + L.road].from : (int16_t)-1;
      }
    }
    if ((rc = upload(&h->lanes, dl.data(), n_lanes, h->stream))) return rc;
    std::vector<LaneNav> nav((size_t)(n_lanes > 0 ? n_lanes : 1));
    for (int k = 0; k < n_lanes; ++k) {
      const pgd_lane& L = lanes[k];
      LaneNav& v = nav[(size_t)k];
      if (L.dir == 0.0f) {  // straight_lane.py:53-67: start + lon * direction + lat * direction_lateral
        v = LaneNav{(float)((double)L.ax + (double)L.length * L.bx), (float)((double)L.ay + (double)L.length * L.by),
                    -L.by, L.bx, 0.0f, 0.0f, 0.0f, 0.0f};
      } else {  // circular_lane.py:41-49: centre + (radius - lat * direction) * (cos phi, sin phi)
        const double phi = (double)L.dir * L.length / L.bx + L.by, c = cos(phi), s = sin(phi);
        v = LaneNav{(float)(L.ax + (double)L.bx * c), (float)(L.ay + (double)L.bx * s), (float)(-L.dir * c), (float)(-L.dir * s),
                    L.bx, L.dir, L.dir == 1.0f ? L.c - L.by : L.by - L.c, 0.0f};
      }
    }
    if ((rc = upload(&h->lane_nav, nav.data(), (size_t)n_lanes, h->stream))) return rc;
    h->d.lane_nav = h->lane_nav;
  }
  if ((rc = upload(&h->roads, roads, n_roads, h->stream))) return rc;
  if ((rc = upload(&h->boxes, boxes, n_boxes, h->stream))) return rc;
  if ((rc = upload(&h->cell_items, ci, n_ci, h->stream))) return rc;
  // cell-major copies of the boxes: cell_boxes[item_off + k] = boxes[box_off + cell_items[item_off + k]] — one dependent
  // load less per box in the grid walks, and a cell's boxes are contiguous (coalesced across sub-lanes)
  {
    // Inside each cell the lane-surface boxes are moved to the front (stable), and the device copy of cell_start packs
    // the number of lane boxes into the top byte (see cell_first / cell_mid).
    std::vector<pgd_box> cb((size_t)(n_ci > 0 ? n_ci : 1));
    std::vector<LaneExt> cx((size_t)(n_ci > 0 ? n_ci : 1), LaneExt{0.f, 0.f, 0.f, -1});
    std::vector<int32_t> cs2(cs, cs + n_cs);
    for (int m = 0; m < n_maps; ++m) {
      const pgd_map& M = maps[m];
      const int n_cells = M.gx * M.gy;
      if (cs[M.cell_off + n_cells] >= (1 << 24)) return PGD_ERR_ARG;
      for (int c = 0; c < n_cells; ++c) {
        const int a = cs[M.cell_off + c], b = cs[M.cell_off + c + 1];
        int w = a;
        for (int pass = 0; pass < 2; ++pass)
          for (int k = a; k < b; ++k) {
            const pgd_box& bx = boxes[M.box_off + ci[M.item_off + k]];
            if ((bx.kind == PGD_BOX_LANE) == (pass == 0)) {
              if (pass == 0) {
                if (bx.lane < 0 || bx.lane >= M.n_lanes) return PGD_ERR_ARG;
                const pgd_lane& L = lanes[M.lane_off + bx.lane];
                cx[(size_t)M.item_off + w] = L.dir == 0.0f ? LaneExt{L.bx, L.by, 0.0f, L.road} : LaneExt{L.ax, L.ay, L.dir, L.road};
              }
              cb[(size_t)M.item_off + w++] = bx;
            }
            if (pass == 0 && k == b - 1) {
              const int n_lane_boxes = w - a;
              if (n_lane_boxes > 255) return PGD_ERR_ARG;
              cs2[M.cell_off + c] = a | (n_lane_boxes << 24);
            }
          }
      }
    }
    if ((rc = upload(&h->cell_boxes, cb.data(), (size_t)n_ci, h->stream))) return rc;
    if ((rc = upload(&h->cell_ext, cx.data(), (size_t)n_ci, h->stream))) return rc;
    if ((rc = upload(&h->cell_start, cs2.data(), n_cs, h->stream))) return rc;
  }
  h->d.maps = h->maps; h->d.lanes = h->lanes; h->d.roads = h->roads; h->d.boxes = h->boxes;
  h->d.cell_start = h->cell_start; h->d.cell_items = h->cell_items; h->d.cell_boxes = h->cell_boxes; h->d.cell_ext = h->cell_ext;
  if (!h->h_maps) h->h_maps = new std::vector<pgd_map>();
  h->h_maps->assign(maps, maps + n_maps);
  if ((rc = build_scen_map(h))) return rc;
  h->have_maps = true;
  h->img_dirty = true;  // running envs fall back to their own records until their next reset
  HIPCHK(hipMemsetAsync(h->d.imask, 0, sizeof(unsigned long long) * (size_t)h->d.N, h->stream));
  hipLaunchKernelGGL(k_clear_hints, dim3((h->d.N + 255) / 256), dim3(256), 0, h->stream, h->d.ei, h->d.N);
  HIPCHK(hipGetLastError());
  return build_reset_image(h);  // eagerly (needs maps + scenarios): pgd_step never allocates, so it can be graph-captured
}

int pgd_upload_scenarios(pgd_handle h, const pgd_scenario* scen, int n_scen, const pgd_spawn* spawns) {
  if (!h || !scen || n_scen <= 0 || !spawns) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = upload(&h->scen, scen, n_scen, h->stream))) return rc;
  {
    // device-private form of the routes: PGD_CKPT_END from a route's last node on (update_checkpoints: a match on the last node
    // alone changes nothing, navigation.py:270-277 -- the search stops at the mark instead of reading the route length first)
    std::vector<pgd_spawn> dsp(spawns, spawns + (size_t)n_scen * h->d.sstride);
    for (pgd_spawn& q : dsp) {
      const int n = q.n_ckpt < 0 ? 0 : (q.n_ckpt > PGD_MAX_CKPT ? PGD_MAX_CKPT : q.n_ckpt);
      for (int k = n > 0 ? n - 1 : 0; k < PGD_MAX_CKPT; ++k) q.ckpt[k] = (int16_t)PGD_CKPT_END;
    }
    if ((rc = upload(&h->spawns, dsp.data(), dsp.size(), h->stream))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));  // (the staging vector goes out of scope)
  }
  h->d.scen = h->scen; h->d.spawns = h->spawns; h->d.n_scen = n_scen;
  {
    const size_t ns = (size_t)n_scen * h->d.sstride;
    if (h->spawn_hv) { HIPCHK(hipStreamSynchronize(h->stream)); HIPCHK(hipFree(h->spawn_hv)); h->spawn_hv = nullptr; }
    HIPCHK(hipMalloc((void**)&h->spawn_hv, sizeof(float2) * ns));
    hipLaunchKernelGGL(k_spawn_hv, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, h->stream, h->spawns, h->spawn_hv, ns);
    HIPCHK(hipGetLastError());
    h->d.spawn_hv = h->spawn_hv;
  }
  for (size_t k = 0; k < (size_t)n_scen * h->d.sstride; ++k)
    if (spawns[k].lane >= 0 && (!(spawns[k].max_steer <= 1.0f) || spawns[k].n_ckpt > PGD_MAX_CKPT)) return PGD_ERR_ARG;  // tan_small
  h->d.no_groups = 1;
  for (int k = 0; k < n_scen; ++k)
    if (scen[k].n_groups > 0) { h->d.no_groups = 0; break; }
  h->has_objects = false;
  for (size_t k = 0; k < (size_t)n_scen * h->d.sstride; ++k)
    if (spawns[k].lane >= 0 && spawns[k].kind != PGD_OBJ_VEHICLE) { h->has_objects = true; break; }
  {  // one body size for the whole upload?  (unused slots -- lane < 0 -- never enter a world)
    float ul = 0.0f, uw = 0.0f;
    bool uni = !h->has_objects && getenv("PGD_NO_UNI") == nullptr;
    for (size_t k = 0; uni && k < (size_t)n_scen * h->d.sstride; ++k) {
      if (spawns[k].lane < 0) continue;
      if (ul == 0.0f) { ul = spawns[k].length; uw = spawns[k].width; }
      uni = spawns[k].length == ul && spawns[k].width == uw && ul > 0.0f && uw > 0.0f;
    }
    h->d.uni_len = uni ? ul : 0.0f;
    h->d.uni_wid = uni ? uw : 0.0f;
  }
  if (!h->h_scen) h->h_scen = new std::vector<pgd_scenario>();
  h->h_scen->assign(scen, scen + n_scen);
  if ((rc = build_scen_map(h))) return rc;
  h->have_scen = true;
  h->img_dirty = true;
  HIPCHK(hipMemsetAsync(h->d.imask, 0, sizeof(unsigned long long) * (size_t)h->d.N, h->stream));
  hipLaunchKernelGGL(k_clear_hints, dim3((h->d.N + 255) / 256), dim3(256), 0, h->stream, h->d.ei, h->d.N);
  HIPCHK(hipGetLastError());
  return build_reset_image(h);
}

#ifndef PGD_OBS_ENV_LDS
#define PGD_OBS_ENV_LDS 16384  // dynamic LDS a block of k_observe_env may take for its rounds of observers (40 slots x 72 beams: 53.2 us with 16 KB, 55.2 with 12, 55.8 with 48)
#endif
// observe_env_body's observers per round: from g down until the scratch of nw waves plus `extra` words fits `budget` words
static int observers_per_round(const PgdDev& d, int g, int nw, size_t extra, size_t budget) {
  while (g > 1 && (size_t)nw * observe_env_words(g, d.cfg.num_lasers, d.V, d.cfg.num_others) + extra > budget) --g;
  return g;
}

// k_observe_env's launch: all rows of an env by one block (use), waves per env, observers per round of a wave, dynamic LDS
struct ObsEnvPlan { bool use; int nw, G; size_t dyn; };
static ObsEnvPlan observe_env_plan(const pgd_engine* h) {
  const PgdDev& d = h->d;
  ObsEnvPlan p{false, 1, 1, 0};
  if (!(d.A > 1 && d.epw == 1 && !h->row_observe)) return p;
  const bool oth = (d.cfg.marl_flags & PGD_MA_OTHERS_STATE) != 0 && d.cfg.num_others > 0;
  const size_t oth_words = (size_t)observe_env_oth_words(d.A, d.cfg.num_others, oth);
  p.nw = d.A >= 4 * (WAVE / d.V) ? 4 : 1;  // many observers, few per pass: four waves per env, each with its own range
  // observers per round of a wave: the whole range if its LDS fits (48 KB per block)
  p.G = observers_per_round(d, (d.A + p.nw - 1) / p.nw, p.nw, oth_words, PGD_OBS_ENV_LDS / 4);
  p.dyn = ((size_t)p.nw * observe_env_words(p.G, d.cfg.num_lasers, d.V, d.cfg.num_others) + oth_words) * 4;
  p.use = p.dyn <= 49152;
  return p;
}

// The multi-agent observation after a step: is it the four-wave k_observe_env (many agent slots), and may k_step write the rows'
// state blocks itself (PgdDev::state_rows)?  The latter for rows without detector fans, neighbour rows, toll floats or the
// random-agent-model floats -- one lane per agent would cast the fans one beam after the other.  PGD_NO_STATE_IN_STEP=1: never (A/B).
static bool state_in_step_ok(const pgd_engine* h) {
  const pgd_config& c = h->d.cfg;
  const ObsEnvPlan p = observe_env_plan(h);
  return p.use && p.nw == 4 && c.side_lasers == 0 && c.lane_line_lasers == 0 && c.num_others == 0 && !c.random_agent_model &&
         !(c.marl_flags & (PGD_MA_TOLLGATE | PGD_MA_OTHERS_STATE)) && c.num_lasers > 0 && !h->no_state_in_step;
}

static int launch_observe(pgd_handle h, float* d_obs, const uint32_t* d_flags, const PgdDev* dv = nullptr, hipStream_t stream = nullptr,
                          int n_envs = 0, bool state_done = false) {
  const PgdDev& D = dv ? *dv : h->d;
  if (!stream) stream = h->stream;
  const int envs = n_envs > 0 ? n_envs : h->d.N, rows = envs * h->d.A;
  const bool oth = (h->d.cfg.marl_flags & PGD_MA_OTHERS_STATE) != 0 && h->d.cfg.num_others > 0;
  const ObsEnvPlan p = observe_env_plan(h);
  if (p.use) {
    const bool four = p.nw == 4;
    const bool fix = !h->no_fix && !h->has_objects && fix_config_matches(D, true, FIXK_MARL);
    ObsFn ke = four ? k_observe_env<4> : k_observe_env<1>;
    if (fix) ke = four ? k_observe_env<4, true> : k_observe_env<1, true>;
    if (state_done && four) ke = fix ? k_observe_env<4, true, false> : k_observe_env<4, false, false>;
    const SeatKernels* seats = (fix && four) ? marl_fix_seats(D) : nullptr;
    if (seats && seats->observe) ke = state_done ? seats->observe_after_state : seats->observe;
    hipLaunchKernelGGL(ke, dim3(envs), dim3(WAVE * p.nw), p.dyn, stream, D, d_obs, d_flags, p.G);
    HIPCHK(hipGetLastError());
    return PGD_OK;
  }
  if (state_done) return PGD_ERR_STATE;  // (state_in_step_ok promised the four-wave kernel)
  { int rc = obs_rows_forget(h, stream); if (rc) return rc; }
  const bool wide = h->d.cfg.num_lasers > 128;  // up to 128 beams one wave does it in two rounds: 4x fewer waves than 256-thread blocks
  ObsFn kern = wide ? (oth ? k_observe<256, true> : k_observe<256, false>) : (oth ? k_observe<64, true> : k_observe<64, false>);
  hipLaunchKernelGGL(kern, dim3(wide ? rows : (rows + OBS_RPB - 1) / OBS_RPB), dim3(wide ? 256 : WAVE * OBS_RPB), 0, stream, D, d_obs, d_flags, rows);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

int pgd_reset(pgd_handle h, const int32_t* env_ids, const int32_t* scen_ids, int n, float* d_obs) {
  if (!h || !scen_ids || n <= 0 || n > h->d.N) return PGD_ERR_ARG;
  if (!h->have_maps || !h->have_scen) return PGD_ERR_STATE;
  HIPCHK(hipSetDevice(h->device));
  for (int k = 0; k < n; ++k) {
    if (scen_ids[k] < 0 || scen_ids[k] >= h->d.n_scen) return PGD_ERR_ARG;
    if (env_ids && (env_ids[k] < 0 || env_ids[k] >= h->d.N)) return PGD_ERR_ARG;
  }
  // the caller's id lists are copied into pinned staging here, so they may be reused as soon as this call returns and the
  // stream is not synchronised (a partial reset between two steps does not stall the device); the staging buffer itself
  // is guarded by an event (a second reset waits until the first one's copies have been consumed)
  if (h->ids_pending) { HIPCHK(hipEventSynchronize(h->ev_ids)); h->ids_pending = false; }
  int32_t* d_env = nullptr;
  if (env_ids) {
    memcpy(h->h_ids, env_ids, sizeof(int32_t) * (size_t)n);
    HIPCHK(hipMemcpyAsync(h->d_ids, h->h_ids, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream));
    d_env = h->d_ids;
  }
  memcpy(h->h_ids + h->d.N, scen_ids, sizeof(int32_t) * (size_t)n);
  HIPCHK(hipMemcpyAsync(h->d_ids + h->d.N, h->h_ids + h->d.N, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream));
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(h->stream, &cap);
  if (cap == hipStreamCaptureStatusNone) { HIPCHK(hipEventRecord(h->ev_ids, h->stream)); h->ids_pending = true; }
  int blocks = (n + h->d.epw - 1) / h->d.epw;
  hipLaunchKernelGGL(k_reset, dim3(blocks), dim3(WAVE), 0, h->stream, h->d, d_env, h->d_ids + h->d.N, n);
  HIPCHK(hipGetLastError());
  { int rc = render_forget(h, d_env, n); if (rc) return rc; }  // rendered trails and deads end with the episode
  if (d_obs) return launch_observe(h, d_obs, nullptr);
  return PGD_OK;
}

static int step_impl(pgd_handle h, const float* d_actions, float* d_obs, float* d_reward, uint8_t* d_done, uint32_t* d_flags,
                     int ostride, bool packed, int group = -1) {
  if (!h || !d_actions || !d_reward || !d_done || !d_flags) return PGD_ERR_ARG;
  if (!h->have_maps || !h->have_scen) return PGD_ERR_STATE;
  if (h->img_dirty) return PGD_ERR_STATE;  // the reset image is built by the upload calls
  HIPCHK(hipSetDevice(h->device));
  PgdDev dv = h->d;  // this launch's output addressing
  dv.ostride = ostride;
  dv.prow = packed ? d_obs : nullptr;
  dv.obs_g = observers_per_round(h->d, h->d.A, 1, 0, STEP_MINB_WORDS);  // fused multi-agent observation: what the step's LDS holds
  EnvGroup g;  // the blocks and the stream of the env group
  { int rc = env_group(h, group, g); if (rc) return rc; }
  dv.unit_off = g.first / h->d.epw;
  const bool marl = (h->d.cfg.marl_flags & PGD_MA_ENABLED) != 0;
  // single-agent engines fuse the row into the wave that stepped the env; multi-agent engines append observe_env_body
  // (all rows of the env) when its per-beam minima fit the step's LDS -- one launch per step either way
  const bool oth_rows = (h->d.cfg.marl_flags & PGD_MA_OTHERS_STATE) != 0 && h->d.cfg.num_others > 0;
  const bool fuse_env = d_obs && marl && h->d.epw == 1 && h->d.A > 1 && !oth_rows && !h->no_fuse && !h->row_observe &&
                        h->d.A < 4 * (WAVE / h->d.V) &&  // else the four-wave k_observe_env is the faster one (measured again with the
                                                          // compacted lists, round 4: 40 slots with 30 agents alive 146 us fused, 58 + 67 apart)
                        observe_env_words(1, h->d.cfg.num_lasers, h->d.V, h->d.cfg.num_others) <= STEP_MINB_WORDS;  // at least one observer per round
  const bool fuse_state = d_obs && !marl && h->d.epw > 1 && h->d.cfg.num_lasers <= 0 && !h->no_fuse;  // state-only rows, several envs per wave
  const bool fuse_pack = d_obs && h->d.pack_obs;  // throughput mode: the rows of the wave's envs appended to k_step
  const bool fuse = (d_obs && !marl && h->d.epw == 1 && h->d.A <= FUSE_MAX_AGENTS && !h->no_fuse) || fuse_env || fuse_state || fuse_pack;
  bool prof = h->prof_ev && h->prof_n < h->prof_cap && group < 0;
  // strided profile: with the observation fused (one kernel per step) events [0] / [1] bracket a GROUP of `stride`
  // back-to-back launches and the group time is divided by the stride; otherwise every stride-th step is bracketed
  const bool grouped = prof && h->prof_stride > 1 && fuse;
  bool g_open = false, g_close = false;
  if (prof && h->prof_stride > 1) {
    const int ph = h->prof_tick++ % h->prof_stride;
    if (grouped) { g_open = ph == 0; g_close = ph == h->prof_stride - 1; prof = false; }
    else prof = ph == 0;
  }
  hipEvent_t* pe = (prof || g_open || g_close) ? &(*h->prof_ev)[(size_t)h->prof_n * 3] : nullptr;
  const bool timing = h->step_timing && !prof && !grouped && group < 0;
  if (prof || timing || g_open) HIPCHK(hipEventRecord((prof || g_open) ? pe[0] : h->ev0, h->stream));
  int blocks = (g.count + h->d.epw - 1) / h->d.epw;
  if (marl && h->d.epw != 1) return PGD_ERR_STATE;  // the multi-agent tail needs the env in one wave (V >= 33 or SUB split)
  const StepKernel sk = step_kernel(h);
  // many agent slots: the rows come from k_observe_env after the step; the state blocks of the rows that are due are k_step's
  const bool state_in_step = d_obs && !fuse && marl && state_in_step_ok(h);
  dv.state_rows = state_in_step ? d_obs : nullptr;
  PgdCold cold_arg{dv.scen_map, dv.bev_fill, dv.spawn_hv, dv.respawn_img, dv.n_scen, dv.cfg.seed, dv.cfg.env_base,
                   h->lk.obs, h->lk.k_lat, h->lk.k_head, h->lk.v_target, h->lk.noise, h->lk.tick};
  float* obs_arg = fuse ? d_obs : (float*)nullptr;
  // a kernel built for this handle at run time takes the place of a GENERAL kernel only (the AOT instantiations are what it would be),
  // and only while the engine is what it was built for
  const bool general = !sk.specialised || h->jit_force;  // (PGD_JIT_FORCE=1, A/B only: also in place of an AOT instantiation)
  const bool use_jit = h->jit_fn && general && jit_geometry_ok(h) && !h->no_fix && !h->lk.obs && h->jit_obj == h->has_objects &&
                       h->jit_geom[0] == h->d.sub && h->jit_geom[1] == h->d.epw && h->jit_geom[2] == h->d.pack_obs &&
                       h->jit_geom[3] == h->d.use_imask;
  if (use_jit) {
    h->last_step_kernel = h->jit_name;
    void* kargs[] = {&dv, &d_actions, &d_reward, &d_done, &d_flags, &obs_arg, &cold_arg};
    HIPCHK(hipModuleLaunchKernel(h->jit_fn, (unsigned)blocks, 1, 1, WAVE, 1, 1, 0, g.stream, kargs, nullptr));
  } else {
    h->last_step_kernel = sk.name;
    hipLaunchKernelGGL(sk.fn, dim3(blocks), dim3(WAVE), 0, g.stream, dv, d_actions, d_reward, d_done, d_flags, obs_arg, cold_arg);
  }
  HIPCHK(hipGetLastError());
  if (prof || g_close) HIPCHK(hipEventRecord(pe[1], h->stream));
  if (g_close) h->prof_n += 1;
  if (d_obs && !fuse) {
    int rc = launch_observe(h, d_obs, marl ? d_flags : (const uint32_t*)nullptr, &dv, g.stream, g.count, state_in_step);
    if (rc) return rc;
  }
  h->prof_fused = fuse;
  h->prof_grouped = grouped;
  if ((prof && !fuse) || timing) HIPCHK(hipEventRecord(prof ? pe[2] : h->ev1, h->stream));  // fused: [0],[1] bracket the only kernel
  if (prof) h->prof_n += 1;
  else if (timing) h->ev_valid = true;
  return PGD_OK;
}

int pgd_step(pgd_handle h, const float* d_actions, float* d_obs, float* d_reward, uint8_t* d_done, uint32_t* d_flags) {
  if (!h) return PGD_ERR_ARG;
  return step_impl(h, d_actions, d_obs, d_reward, d_done, d_flags, h->d.A * h->d.D, false);
}

int pgd_step_n(pgd_handle h, const float* d_action_ring, int ring_len, int first, int n_steps, float* d_obs, float* d_reward,
               uint8_t* d_done, uint32_t* d_flags) {
  if (!h || !d_action_ring || ring_len < 1 || first < 0 || n_steps < 1) return PGD_ERR_ARG;
  const size_t na = (size_t)h->d.N * h->d.A;
  for (int k = 0; k < n_steps; ++k) {
    const float* act = d_action_ring + (size_t)((first + k) % ring_len) * na * 2;
    const int rc = step_impl(h, act, k == n_steps - 1 ? d_obs : (float*)nullptr, d_reward + (size_t)k * na, d_done + (size_t)k * na,
                             d_flags + (size_t)k * na, h->d.A * h->d.D, false);
    if (rc) return rc;
  }
  return PGD_OK;
}

int pgd_step_packed(pgd_handle h, const float* d_actions, float* d_rows, int row_stride, float* d_reward, uint8_t* d_done,
                    uint32_t* d_flags) {
  if (!h || !d_rows || row_stride < h->d.A * (h->d.D + 2)) return PGD_ERR_ARG;
  return step_impl(h, d_actions, d_rows, d_reward, d_done, d_flags, row_stride, true);
}

/* ---- env groups: asynchronous vector-env groups inside one handle ---------------------------------------------------- */
int pgd_set_groups(pgd_handle h, int n_groups) {
  if (!h || n_groups < 1 || n_groups > 64) return PGD_ERR_ARG;
  if (h->d.N % n_groups != 0) return PGD_ERR_ARG;  // equal groups
  int pack = h->d.pack_obs, sub = h->d.sub, epw = h->d.epw;
  if ((h->d.N / n_groups) % epw != 0) {
    // groups are launched as whole waves.  Throughput mode (pgd_create picks it from 32768 envs on: three envs of 17 slots per
    // wave) does not divide a power-of-two group size: such an engine goes back to one env per wave -- the record, image and
    // mask layouts do not depend on the lane mapping, so the switch is a change of launch geometry only.  The new geometry is
    // worked out in locals and committed only when every check has passed (a refused call leaves the engine as it was), and the
    // switch is reported: pgd_describe_step says so from then on (by the r03 sweep it costs 6 - 18 % at 32768 envs)
    if (!pack) return PGD_ERR_ARG;
    pack = 0;
    sub = WAVE / h->d.V < 16 ? WAVE / h->d.V : 16;
    epw = WAVE / (h->d.V * sub);
    if ((h->d.N / n_groups) % epw != 0) return PGD_ERR_ARG;
  }
  if (pack != h->d.pack_obs) h->left_pack_mode = true;
  h->d.pack_obs = pack; h->d.sub = sub; h->d.epw = epw;
  const int use_imask = h->imask_env >= 0 ? h->imask_env : (pack ? 1 : 0);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (use_imask != h->d.use_imask) {  // (the masks are only kept up while they are read: none is trusted across the switch)
    HIPCHK(hipMemsetAsync(h->d.imask, 0, sizeof(unsigned long long) * (size_t)h->d.N, h->stream));
    h->d.use_imask = use_imask;
  }
  if (h->gstreams) {
    for (int g = 0; g < h->n_groups; ++g) { (void)hipStreamSynchronize(h->gstreams[g]); (void)hipStreamDestroy(h->gstreams[g]); }
    free(h->gstreams);
    h->gstreams = nullptr;
  }
  h->n_groups = n_groups;
  if (n_groups > 1) {
    h->gstreams = (hipStream_t*)calloc((size_t)n_groups, sizeof(hipStream_t));
    for (int g = 0; g < n_groups; ++g) HIPCHK(hipStreamCreateWithFlags(&h->gstreams[g], hipStreamNonBlocking));
  }
  return PGD_OK;
}

int pgd_step_group(pgd_handle h, int group, const float* d_actions, float* d_obs, float* d_reward, uint8_t* d_done, uint32_t* d_flags) {
  if (!h || group < 0) return PGD_ERR_ARG;
  return step_impl(h, d_actions, d_obs, d_reward, d_done, d_flags, h->d.A * h->d.D, false, group);
}

int pgd_group_stream(pgd_handle h, int group, void** hip_stream) {
  if (!h || !hip_stream || group < 0 || group >= h->n_groups || !h->gstreams) return PGD_ERR_ARG;
  *hip_stream = (void*)h->gstreams[group];
  return PGD_OK;
}

int pgd_group_sync(pgd_handle h, int group) {
  if (!h || group < 0 || group >= h->n_groups || !h->gstreams) return PGD_ERR_ARG;
  HIPCHK(hipStreamSynchronize(h->gstreams[group]));
  return PGD_OK;
}

int pgd_mlp_policy(pgd_handle h, int group, const float* d_obs, int obs_stride, int in_dim, int hidden, const float* d_w1, const float* d_b1,
                   const float* d_w2, const float* d_b2, const float* d_w3, const float* d_b3, int out_cols, int final_tanh,
                   float* d_actions) {
  if (!h || !d_obs || !d_w1 || !d_b1 || !d_w2 || !d_b2 || !d_w3 || !d_b3 || !d_actions) return PGD_ERR_ARG;
  if (hidden != MLP_H || in_dim < 4 || in_dim > 4096 || obs_stride < in_dim || out_cols < 2) return PGD_ERR_ARG;
  if ((((uintptr_t)d_w1 | (uintptr_t)d_w2 | (uintptr_t)d_b1 | (uintptr_t)d_b2) & 15u) != 0u) return PGD_ERR_ARG;  // 16-byte reads
  const size_t lds = mlp_lds_bytes(in_dim);
  if (lds > 65536) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  EnvGroup g;  // the rows of one env group (or all), on its stream (pgd_step_group's twin)
  { int rc = env_group(h, group, g); if (rc) return rc; }
  const int rows = g.count * h->d.A, row0 = g.first * h->d.A;
  auto kern = final_tanh ? k_mlp_policy<true> : k_mlp_policy<false>;
  if (lds > 49152 && !h->mlp_attr[final_tanh ? 1 : 0]) {  // (per engine = per device: a process may hold engines on several GPUs)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    h->mlp_attr[final_tanh ? 1 : 0] = true;
  }
  hipLaunchKernelGGL(kern, dim3((rows + MLP_ROWS - 1) / MLP_ROWS), dim3(WAVE * MLP_WAVES), lds, g.stream, d_obs, row0, rows, obs_stride, in_dim,
                     d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, out_cols, d_actions);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

/* ---- the policy network with split bf16 operands (pgd_policy.h, second half): weights prepared once per policy update ------------ */
size_t pgd_mlp_prepared_bytes(int in_dim) { return in_dim >= 4 && in_dim <= 4096 ? mlp_prepared_bytes(in_dim) : 0; }

int pgd_mlp_prepare(pgd_handle h, int in_dim, int hidden, const float* d_w1, const float* d_b1, const float* d_w2, const float* d_b2,
                    const float* d_w3, const float* d_b3, int out_cols, void* d_prepared) {
  if (!h || !d_w1 || !d_b1 || !d_w2 || !d_b2 || !d_w3 || !d_b3 || !d_prepared) return PGD_ERR_ARG;
  if (hidden != MLP_H || in_dim < 4 || in_dim > 4096 || out_cols < 2 || (reinterpret_cast<uintptr_t>(d_prepared) & 15u) != 0u) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  const int n = (mlp_chunks(in_dim) + mlp_chunks(MLP_H)) * MLP_WAVES * 4 * WAVE;
  hipLaunchKernelGGL(k_mlp_prepare, dim3((n + 255) / 256), dim3(256), 0, h->stream, d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, in_dim, out_cols,
                     reinterpret_cast<uint4*>(d_prepared));
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

int pgd_mlp_policy_prepared(pgd_handle h, int group, const float* d_obs, int obs_stride, int in_dim, const void* d_prepared, int final_tanh,
                            float* d_actions) {
  if (!h || !d_obs || !d_prepared || !d_actions) return PGD_ERR_ARG;
  if (in_dim < 4 || in_dim > 4096 || obs_stride < in_dim || (reinterpret_cast<uintptr_t>(d_prepared) & 15u) != 0u) return PGD_ERR_ARG;
  const size_t lds = mlp_bf_lds_bytes(in_dim);
  if (lds > 65536) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  EnvGroup g;
  { int rc = env_group(h, group, g); if (rc) return rc; }
  const int rows = g.count * h->d.A, row0 = g.first * h->d.A;
  auto kern = final_tanh ? k_mlp_policy_bf<true> : k_mlp_policy_bf<false>;
  if (lds > 49152 && !h->mlp_attr[2 + (final_tanh ? 1 : 0)]) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    h->mlp_attr[2 + (final_tanh ? 1 : 0)] = true;
  }
  hipLaunchKernelGGL(kern, dim3((rows + MLP_ROWS - 1) / MLP_ROWS), dim3(WAVE * MLP_WAVES), lds, g.stream, d_obs, row0, rows, obs_stride, in_dim,
                     reinterpret_cast<const uint4*>(d_prepared), d_actions);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

/* ---- run-time specialisation (pgdrive_amd/jit.py builds the code object with hipcc; see include/pgdrive_hip.h) -------------- */
int pgd_step_geometry(pgd_handle h, int32_t* out12) {
  if (!h || !out12) return PGD_ERR_ARG;
  const int v[12] = {h->d.N, h->d.A, h->d.T, h->d.V, h->d.D, h->d.NV, h->d.epw, h->d.sub, h->d.pack_obs, h->d.sstride, h->d.use_imask,
                     // bit 0: objects among the bodies; bit 1: default row layout; bit 2: the engine can take a run-time kernel at all
                     (h->has_objects ? 1 : 0) | (std_rows(h->d.cfg) ? 2 : 0) | ((jit_geometry_ok(h) && h->have_scen) ? 4 : 0)};
  for (int k = 0; k < 12; ++k) out12[k] = v[k];
  return PGD_OK;
}

int pgd_set_step_module(pgd_handle h, const char* code_object_path, int built_with_objects, int built_with_std_rows) {
  if (!h) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  if (h->jit_mod) {  // (a module in use by launches in flight must outlive them: the engine's stream and every env group's)
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int g = 0; h->gstreams && g < h->n_groups; ++g) HIPCHK(hipStreamSynchronize(h->gstreams[g]));
    h->jit_fn = nullptr;
    (void)hipModuleUnload(h->jit_mod);
    h->jit_mod = nullptr;
  }
  if (!code_object_path) return PGD_OK;  // (null: back to the library's own kernels)
  if (!jit_geometry_ok(h)) return PGD_ERR_STATE;
  hipModule_t mod = nullptr;
  if (hipModuleLoad(&mod, code_object_path) != hipSuccess) { (void)hipGetLastError(); return PGD_ERR_HIP; }
  char name[160];
  snprintf(name, sizeof(name), "_Z6k_stepILb1ELb0ELb%dELb%dELi9ELb0EEv6PgdDevPKfPfPhPjS3_7PgdCold", built_with_objects ? 1 : 0,
           built_with_std_rows ? 1 : 0);
  hipFunction_t fn = nullptr;
  if (hipModuleGetFunction(&fn, mod, name) != hipSuccess) { (void)hipGetLastError(); (void)hipModuleUnload(mod); return PGD_ERR_HIP; }
  h->jit_mod = mod;
  h->jit_obj = built_with_objects != 0;
  h->jit_geom[0] = h->d.sub; h->jit_geom[1] = h->d.epw; h->jit_geom[2] = h->d.pack_obs; h->jit_geom[3] = h->d.use_imask;
  snprintf(h->jit_name, sizeof(h->jit_name), "k_step: one env per wave, specialised for this engine's configuration at run time");
  h->jit_fn = fn;  // (published last: a step on another thread sees either no module or a complete one)
  return PGD_OK;
}

int pgd_forget_rows(pgd_handle h) {
  if (!h) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  return obs_rows_forget(h, h->stream);
}

int pgd_describe_step(pgd_handle h, char* buf, int cap) {
  if (!h || !buf || cap <= 0) return PGD_ERR_ARG;
  snprintf(buf, (size_t)cap, "%s%s", h->last_step_kernel ? h->last_step_kernel : "",
           h->left_pack_mode ? " [throughput mode switched off by pgd_set_groups: the group size is not a whole number of three-env waves]" : "");
  return PGD_OK;
}

int pgd_step_lane_keep(pgd_handle h, float k_lat, float k_head, float v_target_kmh, float noise, uint32_t tick, float* d_obs,
                       float* d_reward, uint8_t* d_done, uint32_t* d_flags) {
  if (!h || !d_obs || !d_reward || !d_done || !d_flags) return PGD_ERR_ARG;
  if (h->d.A != 1 || h->d.cfg.side_lasers != 0 || h->d.D < 4) return PGD_ERR_STATE;  // reads columns 0..3 of the default layout
  if (lane_keep_in_step(h) && (reinterpret_cast<uintptr_t>(d_obs) & 7u) == 0u) {
    // one launch: k_step reads the row of the previous step where it would read the caller's action
    h->lk = {d_obs, k_lat, k_head, v_target_kmh, noise, tick};
    const int rc = step_impl(h, d_obs /* (never read: the kernel takes the scripted action) */, d_obs, d_reward, d_done, d_flags,
                             h->d.A * h->d.D, false);
    h->lk.obs = nullptr;
    return rc;
  }
  // any other engine: the policy as a launch of its own
  if (!h->lk_act) HIPCHK(hipMalloc((void**)&h->lk_act, sizeof(float) * 2 * (size_t)h->d.N));
  const int rc = pgd_lane_keep_actions(h, d_obs, h->lk_act, k_lat, k_head, v_target_kmh, noise, tick);
  if (rc) return rc;
  return step_impl(h, h->lk_act, d_obs, d_reward, d_done, d_flags, h->d.A * h->d.D, false);
}

int pgd_lane_keep_actions(pgd_handle h, const float* d_obs, float* d_actions, float k_lat, float k_head, float v_target_kmh,
                          float noise, uint32_t tick) {
  if (!h || !d_obs || !d_actions) return PGD_ERR_ARG;
  if (h->d.A != 1 || h->d.cfg.side_lasers != 0 || h->d.D < 4) return PGD_ERR_STATE;  // reads columns 0..3 of the default layout
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_lane_keep, dim3((h->d.N + 255) / 256), dim3(256), 0, h->stream, h->d, d_obs, d_actions, k_lat, k_head,
                     v_target_kmh, noise, tick);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

int pgd_observe(pgd_handle h, float* d_obs) {
  if (!h || !d_obs) return PGD_ERR_ARG;
  if (!h->have_maps || !h->have_scen) return PGD_ERR_STATE;
  HIPCHK(hipSetDevice(h->device));
  int blocks = (h->d.N + h->d.epw - 1) / h->d.epw;
  hipLaunchKernelGGL(k_refresh, dim3(blocks), dim3(WAVE), 0, h->stream, h->d);
  HIPCHK(hipGetLastError());
  return launch_observe(h, d_obs, nullptr);
}

int pgd_state_dims(pgd_handle h, int* nf, int* ni, int* nei) {
  (void)h;
  if (nf) *nf = PGD_NF;
  if (ni) *ni = PGD_NI;
  if (nei) *nei = PGD_NEI;
  return PGD_OK;
}
}  // extern "C" (state conversion helpers are C++ templates)

// ABI order is field-major ([field][env*V + slot], [field][env]); the device keeps one 128 B record per vehicle and one
// PGD_NEI-int row per env — converted on the host
// host copies of the record array: record k = (env k / V, slot k % V) out of / into the piece planes of its env's block (RecPiece)
static void record_from_planes(const RecPiece* raw, int V, size_t k, VehRec& t) {
  const RecPiece* blk = raw + (k / (size_t)V) * (size_t)(8 * V);
  for (int p = 0; p < 8; ++p) memcpy(reinterpret_cast<char*>(&t) + 16 * p, blk + (size_t)p * V + k % (size_t)V, 16);
}
static void record_to_planes(RecPiece* raw, int V, size_t k, const VehRec& t) {
  RecPiece* blk = raw + (k / (size_t)V) * (size_t)(8 * V);
  for (int p = 0; p < 8; ++p) memcpy(blk + (size_t)p * V + k % (size_t)V, reinterpret_cast<const char*>(&t) + 16 * p, 16);
}
extern "C" int pgd_get_state(pgd_handle h, float* f, int32_t* i, int32_t* ei) {
  if (!h || !f || !i || !ei) return PGD_ERR_ARG;
  const size_t nv = (size_t)h->d.NV;
  const int N = h->d.N;
  HIPCHK(hipSetDevice(h->device));
  std::vector<RecPiece> tr(nv * 8);
  std::vector<int32_t> te((size_t)N * PGD_NEI);
  HIPCHK(hipMemcpyAsync(tr.data(), h->d.rec, sizeof(VehRec) * nv, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(te.data(), h->d.ei, sizeof(int32_t) * te.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (size_t k = 0; k < nv; ++k) {  // device record -> ABI fields (struct Veh in pgd_device.h)
    VehRec t;
    record_from_planes(tr.data(), h->d.V, k, t);
    const float fv[PGD_NF] = {t.x, t.y, t.th, t.v, t.steer, t.a1t /* SF_THROTTLE */, t.lastx, t.lasty, t.lasthx, t.lasthy, t.a0s, t.a0t,
                              t.a1s, t.a1t, t.php, t.phi, t.plp, t.pli, t.target, t.energy, t.dl, t.dr, t.eprew, t.agent_id, t.hx, t.hy};
    const int32_t iv[PGD_NI] = {(int32_t)t.status, (int32_t)t.lane, (int32_t)t.ck0, (int32_t)t.ck1, (int32_t)t.rlane, (int32_t)t.timer,
                                (int32_t)t.vflags, (int32_t)t.spawn};
    for (int q = 0; q < PGD_NF; ++q) f[(size_t)q * nv + k] = fv[q];
    for (int q = 0; q < PGD_NI; ++q) i[(size_t)q * nv + k] = iv[q];
  }
  for (int e = 0; e < N; ++e)
    for (int q = 0; q < PGD_NEI; ++q) ei[(size_t)q * N + e] = q == EI_NEAR ? 0 : te[(size_t)e * PGD_NEI + q];
  return PGD_OK;
}
extern "C" int pgd_set_state(pgd_handle h, const float* f, const int32_t* i, const int32_t* ei) {
  if (!h || !f || !i || !ei) return PGD_ERR_ARG;
  const size_t nv = (size_t)h->d.NV;
  const int N = h->d.N;
  std::vector<RecPiece> tr(nv * 8);
  std::vector<int32_t> te((size_t)N * PGD_NEI);
  for (size_t k = 0; k < nv; ++k) {  // ABI fields -> device record; the derived part is rebuilt on the device (k_derive)
    VehRec t;
    memset(&t, 0, sizeof(t));
    auto F = [&](int q) { return f[(size_t)q * nv + k]; };
    auto I = [&](int q) { return i[(size_t)q * nv + k]; };
    t.x = F(SF_X); t.y = F(SF_Y); t.th = F(SF_THETA); t.v = F(SF_SPEED); t.steer = F(SF_STEER);
    t.lastx = F(SF_LASTX); t.lasty = F(SF_LASTY); t.lasthx = F(SF_LASTHX); t.lasthy = F(SF_LASTHY);
    t.a0s = F(SF_ACT0S); t.a0t = F(SF_ACT0T); t.a1s = F(SF_ACT1S); t.a1t = F(SF_ACT1T);
    t.php = F(SF_PID_HP); t.phi = F(SF_PID_HI); t.plp = F(SF_PID_LP); t.pli = F(SF_PID_LI);
    t.target = F(SF_TARGET_SPEED); t.energy = F(SF_ENERGY); t.dl = F(SF_DIST_LEFT); t.dr = F(SF_DIST_RIGHT);
    t.eprew = F(SF_EP_REWARD); t.agent_id = F(SF_AGENT_ID);
    {  // the carried heading vector is taken from the checkpoint only while it agrees with THETA (a caller that edits THETA,
       // or builds a state by hand, gets cos / sin of it)
      const double c = cos((double)t.th), sn = sin((double)t.th);
      t.hx = F(SF_HX); t.hy = F(SF_HY);
      if (!(fabs((double)t.hx - c) <= 1e-4 && fabs((double)t.hy - sn) <= 1e-4)) { t.hx = (float)c; t.hy = (float)sn; }
    }
    const int32_t lane = I(SI_LANE), spawn = I(SI_SPAWN), rlane = I(SI_RLANE), timer = I(SI_TIMER), vflags = I(SI_VFLAGS),
                  status = I(SI_STATUS), ck0 = I(SI_CK0), ck1 = I(SI_CK1);
    if (lane < 0 || lane > 0xffff || spawn < 0 || spawn > 0xffff || rlane < -1 || rlane > 0x7fff || timer < 0 || status < 0 ||
        status > 15 || ck0 < 0 || ck0 >= PGD_MAX_CKPT || ck1 < 0 || ck1 >= PGD_MAX_CKPT || (vflags & ~0xffff))
      return PGD_ERR_ARG;
    t.lane = (uint32_t)lane; t.spawn = (uint32_t)spawn; t.rlane = rlane; t.timer = (uint32_t)std::min(timer, 0xffff);
    t.vflags = (uint32_t)vflags; t.status = (uint32_t)status; t.ck0 = (uint32_t)ck0; t.ck1 = (uint32_t)ck1;
    record_to_planes(tr.data(), h->d.V, k, t);
  }
  for (int e = 0; e < N; ++e)
    for (int q = 0; q < PGD_NEI; ++q) te[(size_t)e * PGD_NEI + q] = q == EI_NEAR ? 1 : ei[(size_t)q * N + e];
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(h->d.rec, tr.data(), sizeof(VehRec) * nv, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d.ei, te.data(), sizeof(int32_t) * te.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(h->d.imask, 0, sizeof(unsigned long long) * (size_t)N, h->stream));  // arbitrary records: none is the image
  h->derive_pending = true;
  { int rc = derive_records(h); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));
  return PGD_OK;
}

extern "C" {
int pgd_enable_step_timing(pgd_handle h, int on) {
  if (!h) return PGD_ERR_ARG;
  h->step_timing = on != 0;
  h->ev_valid = false;
  return PGD_OK;
}

int pgd_last_step_ms(pgd_handle h, float* ms) {
  if (!h || !ms) return PGD_ERR_ARG;
  if (!h->ev_valid) return PGD_ERR_STATE;  // pgd_enable_step_timing(h, 1) and a step first
  HIPCHK(hipEventSynchronize(h->ev1));
  HIPCHK(hipEventElapsedTime(ms, h->ev0, h->ev1));
  return PGD_OK;
}

int pgd_profile_begin(pgd_handle h, int capacity) { return pgd_profile_begin_strided(h, capacity, 1); }

int pgd_profile_begin_strided(pgd_handle h, int capacity, int stride) {
  if (!h || capacity <= 0 || stride <= 0) return PGD_ERR_ARG;
  h->prof_stride = stride;
  h->prof_tick = 0;
  if (!h->prof_ev) h->prof_ev = new std::vector<hipEvent_t>();
  while ((int)h->prof_ev->size() < capacity * 3) {
    hipEvent_t ev;
    HIPCHK(hipEventCreate(&ev));
    h->prof_ev->push_back(ev);
  }
  h->prof_cap = capacity;
  h->prof_n = 0;
  return PGD_OK;
}

int pgd_profile_end(pgd_handle h, float* k_step_ms, float* k_observe_ms, int* count) {
  if (!h || !h->prof_ev || !k_step_ms || !k_observe_ms || !count) return PGD_ERR_ARG;
  HIPCHK(hipStreamSynchronize(h->stream));
  double a = 0.0, b = 0.0;
  for (int k = 0; k < h->prof_n; ++k) {
    float t0 = 0.f, t1 = 0.f;
    HIPCHK(hipEventElapsedTime(&t0, (*h->prof_ev)[(size_t)k * 3], (*h->prof_ev)[(size_t)k * 3 + 1]));
    if (!h->prof_fused) HIPCHK(hipEventElapsedTime(&t1, (*h->prof_ev)[(size_t)k * 3 + 1], (*h->prof_ev)[(size_t)k * 3 + 2]));
    a += h->prof_grouped ? t0 / (float)h->prof_stride : t0;
    b += t1;
  }
  *count = h->prof_n;
  *k_step_ms = h->prof_n ? (float)(a / h->prof_n) : 0.f;
  *k_observe_ms = h->prof_n ? (float)(b / h->prof_n) : 0.f;
  h->prof_cap = 0;
  h->prof_n = 0;
  return PGD_OK;
}

#ifdef PGD_PROF
int pgd_debug_phase_raw(pgd_handle h, unsigned long long* out, int n_blocks) {  // [n_blocks][32], then cleared
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_cycles), sizeof(unsigned long long) * 32 * (size_t)n_blocks));
  std::vector<unsigned long long> z((size_t)PROF_BLOCKS * 32, 0ull);
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), z.data(), sizeof(unsigned long long) * z.size()));
  return PGD_OK;
}
int pgd_debug_phase_cycles(pgd_handle h, unsigned long long* out64, int reset) {
  HIPCHK(hipStreamSynchronize(h->stream));
  std::vector<unsigned long long> all((size_t)PROF_BLOCKS * 32);
  HIPCHK(hipMemcpyFromSymbol(all.data(), HIP_SYMBOL(g_phase_cycles), sizeof(unsigned long long) * all.size()));
  for (int k = 0; k < 64; ++k) out64[k] = 0;  // [0,32): sums over blocks, [32,64): max over blocks
  for (size_t b = 0; b < PROF_BLOCKS; ++b)
    for (int k = 0; k < 32; ++k) {
      out64[k] += all[b * 32 + k];
      if (all[b * 32 + k] > out64[32 + k]) out64[32 + k] = all[b * 32 + k];
    }
  if (reset) {
    std::fill(all.begin(), all.end(), 0ull);
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), all.data(), sizeof(unsigned long long) * all.size()));
  }
  return PGD_OK;
}
#endif

#ifdef PGD_EXITAT
int pgd_debug_exit_at(pgd_handle h, int k) { h->d.dbg_exit = k < 0 ? 255 : k; return PGD_OK; }
// n back-to-back steps launched from C (the Python call costs ~7 us per step: longer than the early exit points)
int pgd_debug_step_many(pgd_handle h, const float* a, float* o, float* r, uint8_t* dn, uint32_t* f, int n) {
  for (int k = 0; k < n; ++k) { int rc = pgd_step(h, a, o, r, dn, f); if (rc) return rc; }
  return PGD_OK;
}
#endif

int pgd_set_stream(pgd_handle h, void* hip_stream) {
  if (!h) return PGD_ERR_ARG;
  hipStream_t ns = (hipStream_t)hip_stream;  // null = the device's default stream
  if (ns == h->stream) return PGD_OK;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(ns, &cap);
  hipStreamCaptureStatus cap_old = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(h->stream, &cap_old);
  if (cap == hipStreamCaptureStatusNone && cap_old == hipStreamCaptureStatusNone) {
    HIPCHK(hipEventRecord(h->ev_move, h->stream));  // everything enqueued so far happens before the first op on the new stream
    HIPCHK(hipStreamWaitEvent(ns, h->ev_move, 0));
  }  // a capturing stream (hipGraph capture of policy + step) must not wait on work outside the capture: the caller has
     // synchronised before starting the capture, as graph capture requires anyway
  h->ev_valid = false;
  if (h->own_stream) { h->retired = h->stream; h->own_stream = false; }  // destroyed with the engine
  h->stream = ns;
  return PGD_OK;
}

int pgd_sync(pgd_handle h) {
  if (!h) return PGD_ERR_ARG;
  HIPCHK(hipStreamSynchronize(h->stream));
  return PGD_OK;
}

int pgd_destroy(pgd_handle h) {
  if (!h) return PGD_ERR_ARG;
  (void)hipStreamSynchronize(h->stream);
  if (h->jit_mod) { (void)hipModuleUnload(h->jit_mod); h->jit_mod = nullptr; h->jit_fn = nullptr; }
  void* bufs[] = {h->lk_act, h->rowz, h->d.rec, h->d.ei, h->d.imask, h->d.env_map, h->d_ids, h->maps, h->lanes, h->roads, h->boxes, h->cell_start,
                  h->cell_items, h->cell_boxes, h->cell_ext, h->lane_nav, h->scen_map, h->scen, h->spawns, h->spawn_hv, h->beam, h->reset_img, h->respawn_img};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  (void)hipEventDestroy(h->ev0);
  (void)hipEventDestroy(h->ev1);
  (void)hipEventDestroy(h->ev_move);
  (void)hipEventDestroy(h->ev_ids);
  if (h->h_ids) (void)hipHostFree(h->h_ids);
  if (h->prof_ev) {
    for (hipEvent_t ev : *h->prof_ev) (void)hipEventDestroy(ev);
    delete h->prof_ev;
  }
  if (h->gstreams) {
    for (int g = 0; g < h->n_groups; ++g) { (void)hipStreamSynchronize(h->gstreams[g]); (void)hipStreamDestroy(h->gstreams[g]); }
    free(h->gstreams);
  }
  topdown_free(h);
  render_free(h);
  delete h->h_maps;
  delete h->h_scen;
  if (h->own_stream) (void)hipStreamDestroy(h->stream);
  if (h->retired) (void)hipStreamDestroy(h->retired);
  free(h);
  return PGD_OK;
}

}  // extern "C"

#include "pgd_topdown.h"
#include "pgd_render.h"
#include "pgd_gather.h"
#endif  // !PGD_JIT
