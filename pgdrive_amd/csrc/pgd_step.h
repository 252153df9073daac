// pgd_step.h -- k_step, one env.step() for every environment, and everything that specialises it: the lane mapping, the step's LDS,
// the PGD_FIX*_FIELDS lists that device (write_fixed_config) and host (fix_config_matches) both read, and the phase macros of the
// profile builds.  Part of the single translation unit pgd_engine.hip (included there after pgd_device.h; it includes pgd_vehicle.h,
// pgd_localize.h, pgd_idm.h, pgd_dynamics.h, pgd_observe.h, pgd_policy.h and pgd_actor_critic.h itself, in this order, after the macros they use).
// With -DPGD_JIT the unit ends with this header: the block at its end is the one kernel of a run-time build.
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
// (WAVE, MAXV, FUSE_MAX_AGENTS: pgd_records.h)

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
#include "pgd_actor_critic.h"

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
template <bool REG> DEV const pgd_lane& dest_lane_ref(const pgd_lane& regs, const Tab<pgd_lane>& lanes, int id) {
  if constexpr (REG) return regs; else return lanes[id];
}
template <bool REG> DEV const pgd_spawn& spawn_ref(const pgd_spawn& regs, const Tab<pgd_spawn>& mem) {
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
  uint8_t* bev_fill;
  uint32_t o_scen_map, o_spawn_hv, o_respawn_img;  // arena offsets (PgdDev::tab): the tables only the rare paths read
  DEV Tab<pgd_map> scen_map(const PgdDev& d) const { return {d.tab, o_scen_map}; }
  DEV Tab<float2> spawn_hv(const PgdDev& d) const { return {d.tab, o_spawn_hv}; }
  DEV Tab<RecPiece> respawn_img(const PgdDev& d) const { return {d.tab, o_respawn_img}; }
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
// The engine view of a step kernel.  The specialised kernels work on their copy of the argument (write_fixed_config has written its
// constants over it: every field they use is an entry load).  The GENERAL kernels read the argument IN PLACE, in the kernel-argument
// segment (PgdDev is the kernel's first argument), a field where it is used: they have no scalar registers for entry loads.  Left to the
// compiler that was an accident of how the copy got optimised away, and the table views (Tab) ended it: all fields loaded at the kernel's
// head and parked in spill lanes, 47 -> 98 spilled SGPRs in the 72-beam / 12-slot kernel, its row 3 % slower (profiles/addr32_notes.md).
template <bool IN_PLACE> DEV const PgdDev& step_view(const PgdDev& copy) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (IN_PLACE) return *(const PgdDev*)__builtin_amdgcn_kernarg_segment_ptr();
#endif
  return copy;
}
template <bool ONE_ENV, bool MARL, bool OBJ, bool STD = false, int FIX = 0, bool LK = false>
__global__ __launch_bounds__(WAVE, PGD_WAVES_PER_SIMD) void k_step(PgdDev d_arg, const float* __restrict__ act, float* __restrict__ reward,
                                                uint8_t* __restrict__ done, uint32_t* __restrict__ flags,
                                                float* __restrict__ obs, const PgdCold cold) {
  if (FIX) write_fixed_config<ONE_ENV, MARL, STD, FIX>(d_arg);
  const PgdDev& d = step_view<FIX == 0>(d_arg);

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
  Tab<pgd_spawn> sp{nullptr, 0u};
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
  Tab<pgd_scenario> sc{nullptr, 0u};
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
  // the single-agent kernels of the default geometry (17 slots, image off: the block's address follows from the block index alone):
  // the whole block in three full-width reads, through LDS (rec_stage_issue).  The image lies in the sub-step poses, which nothing
  // touches before the physics.
  constexpr bool STAGED = ONE_ENV && !MARL && !OBJ && STD && FIX >= 1 && FIX <= 3 && fix_spec(FIX).V == PGD_FIX_V;
  uint4 stg[REC_STAGE_ROUNDS(PGD_FIX_V)];
  static_assert(sizeof(SUBP.p) >= sizeof(uint4) * WAVE * REC_STAGE_ROUNDS(PGD_FIX_V), "the block's image fits the sub-step poses, short of beta / trav");
  if constexpr (STAGED) {
    rec_stage_issue<PGD_FIX_V>(rec_block(d.rec, (size_t)e, PGD_FIX_V), lane, stg);
    __builtin_amdgcn_sched_barrier(0);  // the records' reads stay the wave's first: left to itself the scheduler put the action and the spawn heads in front
  } else if (valid && !own_first) load_rec(((ONE_ENV || packed) && ((im >> s) & 1ull)) ? rec_block(d.reset_img(), (size_t)scen, V) : rec_block(d.rec, (size_t)e, V), V, s, r);
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
  if (EARLY_HEAD && valid) { sp = d.spawns() + (size_t)scen * d.sstride + s; spawn_head_load<false>(sp.at(0u), sl); }
  if constexpr (STAGED) rec_stage_take<PGD_FIX_V>(reinterpret_cast<uint4*>(&SUBP.p[0][0]), lane, stg, valid, s, r);
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
    sc = d.scen() + scen;
    mv = map_view_as<MV>(d, d.env_map + e);  // per-env header copy: address known at kernel start
    if (!LATE_WORDS) env_words();
  }
  PHASE_MARK(13);  // load: scenario + table staging
  XMARK(13);
  if (valid) {
    if (!EARLY_HEAD || (int)r.spawn != s) {
      sp = d.spawns() + (size_t)scen * d.sstride + r.spawn;
      if (REGSP) spawn_head_load<MARL>(sp.at(0u), sl);
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
    after_step_vehicle<ONE_ENV>(d.cfg, mv, g, sp, SPV, r, s < A, !one_env, ctx);
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
      const Tab<pgd_spawn> rbase = d.spawns() + (size_t)scen * d.sstride + V;
      unsigned long long freem = 0ull;
      // the places' poses: lane p reads place p, one round trip for all of them (read inside the loop, place after place, the two
      // dependent reads per place were 5 k cycles of a step with 30 agents alive: profiles/r05_notes.md)
      float plx = 0.0f, ply = 0.0f, plc = 1.0f, pls = 0.0f;
      if (lane < gcf.respawn_places) {
        const pgd_spawn& place = rbase[lane * gcf.respawn_dests];
        const float2 phv = cold.spawn_hv(d)[(size_t)scen * d.sstride + V + lane * gcf.respawn_dests];
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
            const pgd_spawn& nsp = d.spawns()[(size_t)scen * d.sstride + fresh_idx];
            const float2 nhv = cold.spawn_hv(d)[(size_t)scen * d.sstride + fresh_idx];
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
      sp = d.spawns() + (size_t)scen * d.sstride + fresh_idx;
      if (REGSP) spawn_head_load<MARL>(sp.at(0u), sl);
      load_rec(rec_block(cold.respawn_img(d), (size_t)scen, d.sstride - V), d.sstride - V, fresh_idx - V, r);
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
    sc = d.scen() + scen;
    mv = map_view_as<MV>(d, cold.scen_map(d).at((uint32_t)scen));  // the header of the new episode's map (the per-env copy is rewritten below)
    ng = 0;
    ep_steps = 0;
  }
  if (valid && resetting) {
    sp = d.spawns() + (size_t)scen * d.sstride + s;
    if (REGSP) spawn_head_load<MARL>(sp.at(0u), sl);
    // the slot right after a reset is a function of the scenario alone (spawn pose, first localisation, side distances,
    // agent id): read from the image k_reset_image built at upload instead of localising every vehicle again
    load_rec(rec_block(d.reset_img(), (size_t)scen, V), V, s, r);
    const unsigned long long am = __ballot(leader && s < A && r.status == ST_ACTIVE);
    if (marl && s < A && r.status == ST_ACTIVE) my_fl |= PGD_F_NEW;
    if (s == 0 && d.cfg.resample_scenario)  // the env's header copy follows the scenario (any number of sub-lanes)
      for (int q = g.sub; q < (int)(sizeof(pgd_map) / 16); q += g.SUB)
        reinterpret_cast<uint4*>(d.env_map + e)[q] = reinterpret_cast<const uint4*>(cold.scen_map(d).at((uint32_t)scen))[q];
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
        agent_view(ag, r, e, s, steps_total);
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
      observe_agent<OBJ, STD, false, true, true>(d, mvo, d.spawns()[(size_t)scen_now * d.sstride + a], ag, OL,
                                                 obs + (size_t)e * d.ostride + (size_t)a * d.D, lane, WAVE, nullptr, Tab<pgd_spawn>{nullptr, 0u}, &pre, lidar_minb(S));
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
      agent_view(ag, r, e, s, steps_total);
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
        agent_view(ag, r, e, 0, steps_total);
        ag.cur_n |= scen << 8;  // the env's (possibly re-drawn) scenario travels with the view
      }
    }
    step_sync();
    if (valid) {  // the state blocks of all envs of the wave at once: the V lanes of an env share the 18 floats of its row
      AgentView ag = s_ag[el];
      ag.cur_n &= 0xff;
      state_block<STD>(d, mv, d.spawns()[(size_t)scen * d.sstride], ag, obs + (size_t)e * d.ostride, s, V);
    }
    for (int q = 0; q < d.epw; ++q) {
      const int eq = unit * d.epw + q;  // wave-uniform
      if (eq >= N) break;
      AgentView ag = s_ag[q];
      const int scen_q = ag.cur_n >> 8;
      ag.cur_n &= 0xff;
      const MV mvq = map_view_as<MV>(d, cold.scen_map(d).at((uint32_t)scen_q));
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
      observe_agent<OBJ, STD, false, false, true>(d, mvq, d.spawns()[(size_t)scen_q * d.sstride], ag, OL, obs + (size_t)eq * d.ostride, lane, WAVE,
                                                  nullptr, Tab<pgd_spawn>{nullptr, 0u}, nullptr, lidar_minb(S));
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
      agent_view(ag, r, e, s, steps_total);
      state_block<false>(d, mv, SPV, ag, row, g.sub, g.SUB);
    }
  }
  PHASE_MARK(14);  // fused observation
  XMARK(14);
  PHASE_END();
}

#undef SPV

#ifdef PGD_JIT
// The run-time build (hipcc --genco -DPGD_JIT -include <generated header>): pgd_device.h, this header and ONE instantiation of the step
// kernel; the other kernels and the host side exist in the library only.
template __global__ void k_step<true, false, PGD_JIT_OBJ, PGD_JIT_STD, 9, false>(PgdDev, const float*, float*, uint8_t*, uint32_t*, float*, PgdCold);
#endif
