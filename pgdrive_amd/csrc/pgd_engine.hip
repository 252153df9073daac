// pgd_engine.hip — the single translation unit of the MI355X-native batched PGDrive step engine and its host side: the engine handle, the
// launch plan of a step and the C ABI (include/pgdrive_hip.h).  What the entry points prepare on the CPU -- geometry, the device forms of the
// tables, the state conversion -- is pgd_host_prep.h (no HIP in it).  The device code is in the headers included here, in this order: pgd_device.h,
// pgd_step.h (k_step; it includes pgd_vehicle.h ... pgd_policy.h, pgd_actor_critic.h), pgd_kernels.h (reset / derive / refresh / observe),
// pgd_marl_rollout.h (live rows, the networks over a row list, masked GAE) and, at the end,
// pgd_topdown.h, pgd_render.h, pgd_gather.h, pgd_step_info.h, pgd_ppo.h (the PPO update) and pgd_safe.h (its cost side) with their own
// entry points.
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
#include "pgd_step.h"
#ifndef PGD_JIT  // (a run-time build, pgdrive_amd/jit.py, is the device code above and nothing else)
#include "pgd_kernels.h"
#include "pgd_marl_rollout.h"
#include "pgd_host_prep.h"  // the GPU-free preparation of the entry points below: geometry, table forms, state conversion

// The library's environment switches (include/pgdrive_hip.h lists them), read once, by pgd_create.  pack / imask: -1 = not forced.
struct Switches { bool no_fuse, no_fix, jit_force, row_observe, no_state_in_step, no_rowz, no_uni; int pack, imask; };
static Switches read_switches() {
  const auto on = [](const char* name) { return getenv(name) != nullptr; };
  const char* rowz = getenv("PGD_NO_ROWZ");  // (set, and not to a value that starts with '0')
  const char* pack = getenv("PGD_PACK");
  return {on("PGD_NO_FUSE"), on("PGD_NO_FIX"), on("PGD_JIT_FORCE"), on("PGD_ROW_OBSERVE"), on("PGD_NO_STATE_IN_STEP"),
          rowz && rowz[0] != '0', on("PGD_NO_UNI"), pack ? (atoi(pack) != 0 ? 1 : 0) : -1, on("PGD_NO_IMASK") ? 0 : (on("PGD_IMASK") ? 1 : -1)};
}
// The kernels that take more than 48 KB of dynamic LDS at wide inputs: their limit is raised once per engine (raise_lds_limit)
// (LDS_AC .. LDS_PPO_ROWS_COST_GUIDED: the instantiations that normalise their observation rows, pgd_obs_norm_bind, have slots of their own behind them)
enum LdsKernel { LDS_MLP, LDS_MLP_TANH, LDS_MLP_BF, LDS_MLP_BF_TANH, LDS_AC, LDS_AC_ROWS, LDS_AC_COST, LDS_PPO_ROWS, LDS_PPO_ROWS_COST, LDS_TERM_VALUE,
                 LDS_AC_CAT, LDS_AC_CAT_ROWS, LDS_PPO_ROWS_CAT, LDS_PPO_ROWS_GUIDED, LDS_PPO_ROWS_COST_GUIDED, LDS_NORM_FIRST,
                 LDS_GUARD = LDS_NORM_FIRST + (LDS_PPO_ROWS_COST_GUIDED - LDS_AC + 1), LDS_GUARD_LEGACY, LDS_KERNELS };
// the tables of the arena, in the order of their offsets (what follows the scenarios first, what follows the maps behind it)
enum ArenaTable { TB_SCEN, TB_SCEN_MAP, TB_SPAWNS, TB_SPAWN_HV, TB_RESET_IMG, TB_RESPAWN_IMG, TB_MAPS, TB_LANES, TB_ROADS, TB_BOXES, TB_CELL_START,
                  TB_CELL_ITEMS, TB_CELL_BOXES, TB_CELL_EXT, TB_LANE_NAV, TB_BEAM, TB_COUNT };
struct pgd_engine {
  PgdDev d;
  Switches sw;
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
  // the read-only tables (PgdDev::tab and its offsets): one device allocation, planned by pgd_plan_arena from the tables' sizes
  // and rebuilt by arena_resize when an upload changes one of them
  char* arena;
  uint64_t arena_bytes;
  uint64_t tab_bytes[TB_COUNT];
  uint32_t tab_off[TB_COUNT];
  bool img_dirty;
  std::vector<pgd_map>* h_maps;
  std::vector<pgd_scenario>* h_scen;
  int32_t* d_ids;  // scratch [2N]
  bool have_maps, have_scen;
  // per-kernel HIP-event profile of pgd_step launches (bench.py roofline numbers)
  std::vector<hipEvent_t>* prof_ev;  // 3 events per recorded step
  int prof_cap, prof_n, prof_stride, prof_tick;
  bool prof_grouped;
  struct pgd_topdown_state* topdown;  // top-down observation (pgd_topdown.h), null until pgd_topdown_enable
  struct pgd_render_state* render;    // top-down scene rendering (pgd_render.h), null until pgd_render_enable
  struct pgd_step_info_state* sinfo;  // step info (pgd_step_info.h), null unless pgd_step_info_enable switched it on
  int n_groups;          // env groups of pgd_set_groups (1 = none)
  hipStream_t* gstreams; // [n_groups] internal streams
  bool derive_pending;  // records were written through the ABI or the tables changed: k_derive has to run
  bool has_objects;  // some spawn record is a traffic object (pgd_upload_scenarios): selects the OBJ kernels
  bool step_timing;  // record ev0 / ev1 around every step (pgd_last_step_ms)
  const char* last_step_kernel;  // what the last pgd_step* call launched (pgd_describe_step)
  // a step kernel built at run time for this handle's configuration (pgd_set_step_module): launched instead of the general kernel
  // while the engine's geometry and object flag are what it was built for
  hipModule_t jit_mod;
  hipFunction_t jit_fn;
  bool jit_obj;
  const uint32_t* ac_tick;  // pgd_actor_critic_tick: the device counter added to every launch's tick (null: none)
  struct { const float* table; int in_dim; float clip; } obs_norm;  // pgd_obs_norm_bind: the table the training launches normalise their rows with (null: none)
  uint32_t* cmp_live;   // pgd_live_rows: block counts of the compaction, a segment for the whole engine and one per env group (pgd_create allocates it)
  uint32_t* cmp_index;  // pgd_rollout_index: block counts [cmp_index_cap], grown outside graph captures
  size_t cmp_index_cap;
  std::vector<uint32_t*>* cmp_retired;  // cmp_index of smaller rollouts: graphs captured with them may still be replayed (freed by pgd_destroy)
  bool lds_raised[LDS_KERNELS];  // raise_lds_limit: the kernel's dynamic LDS limit has been raised on this engine's device
  int jit_geom[4];   // sub, epw, pack_obs, use_imask at the time of the build
  char jit_name[96];
  bool prof_fused;
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

// A launch with `lds` bytes of dynamic LDS: above 48 KB the kernel's limit has to be raised first, once per engine and kernel (per engine =
// per device: a process may hold engines on several GPUs)
static LdsKernel lds_slot(LdsKernel which, bool norm) { return norm ? (LdsKernel)(LDS_NORM_FIRST + (which - LDS_AC)) : which; }
static int raise_lds_limit(pgd_engine* h, LdsKernel which, const void* kernel, size_t lds) {
  if (lds <= 49152 || h->lds_raised[which]) return PGD_OK;
  HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
  h->lds_raised[which] = true;
  return PGD_OK;
}

// The networks of a training entry point (the three pgd_mlp_actor_critic*, the two pgd_ppo_grad*), checked before any HIP call: every
// pointer of the actor and of the cost critic (null: the call has none), the critic's six all set or -- where the call allows it -- all
// null, the widths, and the 16-byte reads of every present network's w1 / b1 / w2 / b2.  *has_critic: whether the critic is there.
static bool six_set(const float* a, const float* b, const float* c, const float* d, const float* e, const float* f) { return a && b && c && d && e && f; }
static bool reads_16(const float* w1, const float* b1, const float* w2, const float* b2) {
  return (((uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w2 | (uintptr_t)b2) & 15u) == 0u;
}
static bool nets_ok(const pgd_actor_critic* a, const pgd_value_net* cost, bool critic_optional, int in_dim, int obs_stride, bool* has_critic) {
  if (!a || !six_set(a->w1, a->b1, a->w2, a->b2, a->w3, a->b3)) return false;
  *has_critic = six_set(a->vw1, a->vb1, a->vw2, a->vb2, a->vw3, a->vb3);
  if (!*has_critic && !(critic_optional && !a->vw1 && !a->vb1 && !a->vw2 && !a->vb2 && !a->vw3 && !a->vb3)) return false;
  if (cost && !six_set(cost->w1, cost->b1, cost->w2, cost->b2, cost->w3, cost->b3)) return false;
  if (in_dim < 4 || in_dim > 4096 || obs_stride < in_dim || a->out_cols < AC_HEAD) return false;
  return reads_16(a->w1, a->b1, a->w2, a->b2) && reads_16(a->vw1, a->vb1, a->vw2, a->vb2) && (!cost || reads_16(cost->w1, cost->b1, cost->w2, cost->b2));
}
// ... and the buffers their gradients go to (pgd_ppo_grad*): the critic's only with a critic
static bool grads_ok(const pgd_ppo_grads* g, const pgd_value_grads* cost, bool has_critic) {
  return g && six_set(g->w1, g->b1, g->w2, g->b2, g->w3, g->b3) && (!has_critic || six_set(g->vw1, g->vb1, g->vw2, g->vb2, g->vw3, g->vb3)) &&
         (!cost || six_set(cost->w1, cost->b1, cost->w2, cost->b2, cost->w3, cost->b3));
}

// The shared tail of the actor-critic forward family, behind the caller's refusals: the observation binding (pgd_obs_norm_bind: a bound
// table of another width refuses the call; `norm` is launched while one is bound, `plain` -- today's code -- otherwise), the rows of the
// env group (or of all envs) on its stream, the raised LDS limit of the chosen kernel, then the caller's launch(es) over those rows
struct AcRows { int row0, rows; uint32_t row_base; size_t lds; hipStream_t stream; ObsNorm nm; };
template <typename Kernel, typename Launch>
static int ac_forward(pgd_engine* h, int group, LdsKernel which, Kernel plain, Kernel norm, int in_dim, Launch launch) {
  const bool bound = h->obs_norm.table != nullptr;
  if (bound && in_dim != h->obs_norm.in_dim) return PGD_ERR_ARG;
  const Kernel kernel = bound ? norm : plain;
  HIPCHK(hipSetDevice(h->device));
  EnvGroup g;
  { int rc = env_group(h, group, g); if (rc) return rc; }
  const size_t lds = ac_lds_bytes(in_dim);
  { int rc = raise_lds_limit(h, lds_slot(which, bound), reinterpret_cast<const void*>(kernel), lds); if (rc) return rc; }
  launch(AcRows{g.first * h->d.A, g.count * h->d.A, (uint32_t)h->d.cfg.env_base * (uint32_t)h->d.A, lds, g.stream,
                ObsNorm{h->obs_norm.table, h->obs_norm.clip}}, kernel);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

using StepFn = void (*)(PgdDev, const float*, float*, uint8_t*, uint32_t*, float*, PgdCold);
using ObsFn = void (*)(PgdDev, float*, const uint32_t*, int);
using ObsIdsFn = void (*)(PgdDev, float*, const int32_t*, int);
// One observation kernel in its launch forms: over an env range (pgd_observe, a full pgd_reset, after a step), over an env range after
// k_step has written the state blocks (null: no such form), and over an id list (pgd_reset with env ids).
struct ObsKernels { ObsFn range, after_state; ObsIdsFn ids; };
// The multi-agent instantiations with the seat count folded (PGD_FIXM_SEAT_FIELDS; code = seats x 1000 + beams).  40 and 44 seats
// observe with k_observe_env<4> after the step; 8 seats fuse the observation into k_step (obs.range null).
struct SeatKernels { int code; StepFn step; const char* name; ObsKernels obs; };
static const SeatKernels SEAT_KERNELS[] = {
    {40072, k_step<true, true, false, false, 40072>,
     "k_step: one env per wave, specialised for the default multi-agent configuration with 40 agent seats x 72 beams",
     {k_observe_env<4, true, true, 40072>, k_observe_env<4, true, false, 40072>, k_observe_env_ids<4, true, 40072>}},
    {44072, k_step<true, true, false, false, 44072>,
     "k_step: one env per wave, specialised for the default multi-agent configuration with 44 agent seats x 72 beams",
     {k_observe_env<4, true, true, 44072>, k_observe_env<4, true, false, 44072>, k_observe_env_ids<4, true, 44072>}},
    {8072, k_step<true, true, false, false, 8072>,
     "k_step: one env per wave, specialised for the default multi-agent configuration with 8 agent seats x 72 beams", {}},
    {8240, k_step<true, true, false, false, 8240>,
     "k_step: one env per wave, specialised for the default multi-agent configuration with 8 agent seats x 240 beams", {}},
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

static bool is_marl(const pgd_engine* h) { return (h->d.cfg.marl_flags & PGD_MA_ENABLED) != 0; }
// Neighbour rows are state rows (PGD_MA_OTHERS_STATE with neighbours): k_observe<.., true>, extra LDS in k_observe_env, no fusing
static bool others_state_rows(const pgd_engine* h) { return (h->d.cfg.marl_flags & PGD_MA_OTHERS_STATE) != 0 && h->d.cfg.num_others > 0; }
// This multi-agent engine may run the FIXK_MARL instantiations; k_step's also need the seats to fill the wave (sub is capped at 16)
static bool marl_fix_ok(const pgd_engine* h) { return !h->has_objects && !h->sw.no_fix && fix_config_matches(h->d, true, FIXK_MARL); }
static bool marl_fix_step_ok(const pgd_engine* h) { return marl_fix_ok(h) && h->d.V == h->d.A && h->d.sub == WAVE / h->d.A; }
// FIX 1 with one env per wave: the reference's default single-agent configuration
static bool default_one_env(const pgd_engine* h) { return !h->has_objects && !h->sw.no_fix && fix_config_matches(h->d, true); }
// the engines whose step kernel has an instantiation with the scripted policy inside: the FIX 1 case, the row fused into the step
static bool lane_keep_in_step(const pgd_engine* h) { return default_one_env(h) && !h->sw.no_fuse; }

// A k_step instantiation, its pgd_describe_step text, and whether it was built for one configuration (write_fixed_config: a run-time
// kernel does not take its place).
struct StepKernel { StepFn fn; const char* name; bool specialised; };
// The instantiation a step launches: the first case that holds, evaluated per step (pgd_set_groups and the uploads change
// what it reads).  A specialised case holds only where fix_config_matches() does, so its results are the general kernel's; the
// PGD_FIX*_FIELDS lists pin the geometry, the multi-agent flags and the row layout, and a case adds what they cannot: the object
// flag and PGD_NO_FIX (A/B: never specialised).
static StepKernel step_kernel(const pgd_engine* h) {
  const PgdDev& d = h->d;
  const bool obj = h->has_objects, fix = !h->sw.no_fix;
  const char* general = d.pack_obs ? "k_step: whole envs side by side in a wave, one vehicle per lane (throughput mode)"
                                   : (d.epw == 1 ? "k_step: one env per wave" : "k_step: several envs per wave");
  if (is_marl(h)) {
    if (marl_fix_step_ok(h)) {
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
  if (!(d.A > 1 && d.epw == 1 && !h->sw.row_observe)) return p;
  const size_t oth_words = (size_t)observe_env_oth_words(d.A, d.cfg.num_others, others_state_rows(h));
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
         !(c.marl_flags & (PGD_MA_TOLLGATE | PGD_MA_OTHERS_STATE)) && c.num_lasers > 0 && !h->sw.no_state_in_step;
}

// A stand-alone observation launch over `envs` envs (pgd_reset, pgd_observe, a step that does not write the rows itself): the kernel
// -- chosen here and nowhere else -- with the launch geometry that all its forms share.  arg: observers per round (k_observe_env) / rows
// (k_observe, which does not keep the zero-row marks: forget them first).  state_done: k_step has written the state blocks (see above).
struct ObsLaunch { ObsKernels k; bool state_done; dim3 grid, block; size_t lds; int arg; bool forget_marks; };
static ObsLaunch observe_launch(const pgd_engine* h, int envs, bool state_done) {
  const ObsEnvPlan p = observe_env_plan(h);
  if (!p.use) {
    const int rows = envs * h->d.A;
    const bool oth = others_state_rows(h);
    const bool wide = h->d.cfg.num_lasers > 128;  // up to 128 beams one wave does it in two rounds: 4x fewer waves than 256-thread blocks
    const ObsKernels k = wide ? (oth ? ObsKernels{k_observe<256, true>, nullptr, k_observe_ids<256, true>}
                                     : ObsKernels{k_observe<256, false>, nullptr, k_observe_ids<256, false>})
                              : (oth ? ObsKernels{k_observe<64, true>, nullptr, k_observe_ids<64, true>}
                                     : ObsKernels{k_observe<64, false>, nullptr, k_observe_ids<64, false>});
    return {k, false, dim3(wide ? rows : (rows + OBS_RPB - 1) / OBS_RPB), dim3(wide ? 256 : WAVE * OBS_RPB), 0, rows, true};
  }
  const bool four = p.nw == 4, fix = marl_fix_ok(h);
  ObsKernels k = four ? ObsKernels{k_observe_env<4>, k_observe_env<4, false, false>, k_observe_env_ids<4>}
                      : ObsKernels{k_observe_env<1>, nullptr, k_observe_env_ids<1>};
  if (fix) k = four ? ObsKernels{k_observe_env<4, true>, k_observe_env<4, true, false>, k_observe_env_ids<4, true>}
                    : ObsKernels{k_observe_env<1, true>, nullptr, k_observe_env_ids<1, true>};
  const SeatKernels* seats = (fix && four) ? marl_fix_seats(h->d) : nullptr;
  if (seats && seats->obs.range) k = seats->obs;
  return {k, state_done && k.after_state != nullptr, dim3(envs), dim3(WAVE * p.nw), p.dyn, p.G, false};
}

// What one step launches, decided once per step (pgd_set_groups, the uploads and pgd_set_step_module change what it reads): the env group,
// the step kernel (jit_fn: the handle's run-time module in its place) and the observation launch after it (obs.k.range null: none).
struct StepPlan { EnvGroup g; StepKernel kernel; hipFunction_t jit_fn; bool fuse, state_in_step; ObsLaunch obs; };
static int plan_step(const pgd_engine* h, bool want_obs, int group, StepPlan& p) {
  const PgdDev& d = h->d;
  const bool marl = is_marl(h), may_fuse = !h->sw.no_fuse;
  { int rc = env_group(h, group, p.g); if (rc) return rc; }
  if (marl && d.epw != 1) return PGD_ERR_STATE;  // the multi-agent tail needs the env in one wave (V >= 33 or SUB split)
  p.kernel = step_kernel(h);
  // a kernel built for this handle at run time takes the place of a GENERAL kernel only (the AOT instantiations are what it would be),
  // and only while the engine is what it was built for
  const bool general = !p.kernel.specialised || h->sw.jit_force;  // (PGD_JIT_FORCE=1, A/B only: also in place of an AOT instantiation)
  const bool use_jit = h->jit_fn && general && jit_geometry_ok(h) && !h->sw.no_fix && !h->lk.obs && h->jit_obj == h->has_objects &&
                       h->jit_geom[0] == d.sub && h->jit_geom[1] == d.epw && h->jit_geom[2] == d.pack_obs && h->jit_geom[3] == d.use_imask;
  p.jit_fn = use_jit ? h->jit_fn : nullptr;
  // The step writes the rows itself (fuse: one launch per step) in four cases.  Single-agent engines fuse the row into the wave that
  // stepped the env; multi-agent engines append observe_env_body (all rows of the env) when its per-beam minima fit the step's LDS
  const bool fuse_one = may_fuse && !marl && d.epw == 1 && d.A <= FUSE_MAX_AGENTS;
  const bool fuse_env = may_fuse && marl && d.epw == 1 && d.A > 1 && !others_state_rows(h) && !h->sw.row_observe &&
                        d.A < 4 * (WAVE / d.V) &&  // else the four-wave k_observe_env is the faster one (measured again with the
                                                   // compacted lists, round 4: 40 slots with 30 agents alive 146 us fused, 58 + 67 apart)
                        observe_env_words(1, d.cfg.num_lasers, d.V, d.cfg.num_others) <= STEP_MINB_WORDS;  // at least one observer per round
  const bool fuse_state = may_fuse && !marl && d.epw > 1 && d.cfg.num_lasers <= 0;  // state-only rows, several envs per wave
  const bool fuse_pack = d.pack_obs != 0;  // throughput mode: the rows of the wave's envs appended to k_step
  p.fuse = want_obs && (fuse_one || fuse_env || fuse_state || fuse_pack);
  // many agent slots: the rows come from k_observe_env after the step; the state blocks of the rows that are due are k_step's
  p.state_in_step = want_obs && !p.fuse && marl && state_in_step_ok(h);
  p.obs = (want_obs && !p.fuse) ? observe_launch(h, p.g.count, p.state_in_step) : ObsLaunch{};
  return PGD_OK;
}

// Rows written by a kernel that does not keep the zero-row marks (k_observe, one block per row): what the marks say about this
// buffer may no longer hold -- forget them (a memset node when the stream is being captured: every replay forgets again).
static int obs_rows_forget(pgd_engine* h, hipStream_t stream) {
  if (!h->rowz) return PGD_OK;
  HIPCHK(hipMemsetAsync(h->rowz, 0, sizeof(ulonglong2) * (size_t)h->d.N, stream));
  return PGD_OK;
}

// env_ids (device): unit k of the launch observes env env_ids[k], without step flags; null: the envs of dv's range
static int launch_observe(pgd_engine* h, const ObsLaunch& o, const PgdDev& dv, float* d_obs, const uint32_t* d_flags, const int32_t* env_ids,
                          hipStream_t stream) {
  if (o.forget_marks) { int rc = obs_rows_forget(h, stream); if (rc) return rc; }
  const ObsFn range = o.state_done ? o.k.after_state : o.k.range;
  if (env_ids) hipLaunchKernelGGL(o.k.ids, o.grid, o.block, o.lds, stream, dv, d_obs, env_ids, o.arg);
  else hipLaunchKernelGGL(range, o.grid, o.block, o.lds, stream, dv, d_obs, d_flags, o.arg);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

static void topdown_free(pgd_engine* h);
static void render_free(pgd_engine* h);
static void step_info_free(pgd_engine* h);
static int step_info_forget(pgd_engine* h, const int32_t* d_env, int n);
static int step_info_launch(pgd_engine* h, const EnvGroup& g, const uint8_t* d_done, uint32_t* d_flags, float* d_obs);
static void render_mark_stale(pgd_engine* h);
static int render_forget(pgd_engine* h, const int32_t* d_env, int n);

template <typename T> static T* arena_ptr(const pgd_engine* h, int table) { return reinterpret_cast<T*>(h->arena + h->tab_off[table]); }

// Gives the `n` tables `ids` the sizes `bytes`.  The other tables keep their contents, the resized ones hold nothing defined afterwards.
// A plan that moves no table and fits the arena changes nothing; any other one is a new arena, built at the stream's quiet point (the
// upload calls synchronise anyway): the kept tables are copied over, the old arena is freed, the device view follows.  Launches never
// come here: they allocate nothing.
static int arena_resize(pgd_engine* h, const int* ids, const uint64_t* bytes, int n) {
  uint64_t want[TB_COUNT];
  uint32_t off[TB_COUNT];
  uint64_t total = 0;
  bool resized[TB_COUNT] = {};
  memcpy(want, h->tab_bytes, sizeof(want));
  for (int k = 0; k < n; ++k) { want[ids[k]] = bytes[k]; resized[ids[k]] = true; }
  { int rc = pgd_plan_arena(want, TB_COUNT, off, &total); if (rc) return rc; }
  if (!h->arena || total > h->arena_bytes || memcmp(off, h->tab_off, sizeof(off)) != 0) {
    HIPCHK(hipStreamSynchronize(h->stream));
    char* fresh = nullptr;
    HIPCHK(hipMalloc((void**)&fresh, (size_t)total));
    for (int t = 0; t < TB_COUNT; ++t)
      if (h->arena && !resized[t] && want[t])
        HIPCHK(hipMemcpyAsync(fresh + off[t], h->arena + h->tab_off[t], (size_t)want[t], hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->arena) HIPCHK(hipFree(h->arena));
    h->arena = fresh;
    h->arena_bytes = total;
    memcpy(h->tab_off, off, sizeof(off));
  }
  memcpy(h->tab_bytes, want, sizeof(want));
  PgdDev& d = h->d;
  const uint32_t* o = h->tab_off;
  d.tab = h->arena;
  d.o_maps = o[TB_MAPS]; d.o_lanes = o[TB_LANES]; d.o_roads = o[TB_ROADS]; d.o_boxes = o[TB_BOXES]; d.o_cell_start = o[TB_CELL_START];
  d.o_cell_items = o[TB_CELL_ITEMS]; d.o_cell_boxes = o[TB_CELL_BOXES]; d.o_cell_ext = o[TB_CELL_EXT]; d.o_lane_nav = o[TB_LANE_NAV];
  d.o_scen = o[TB_SCEN]; d.o_scen_map = o[TB_SCEN_MAP]; d.o_spawns = o[TB_SPAWNS]; d.o_spawn_hv = o[TB_SPAWN_HV];
  d.o_reset_img = o[TB_RESET_IMG]; d.o_respawn_img = o[TB_RESPAWN_IMG]; d.o_beam = o[TB_BEAM];
  return PGD_OK;
}

// host data into a table that arena_resize has sized (no synchronisation: the caller's, after its last table)
template <typename T>
static int arena_fill(pgd_engine* h, int table, const T* src, size_t n) {
  if (sizeof(T) * n > h->tab_bytes[table]) return PGD_ERR_STATE;
  if (n) HIPCHK(hipMemcpyAsync(arena_ptr<T>(h, table), src, sizeof(T) * n, hipMemcpyHostToDevice, h->stream));
  return PGD_OK;
}
// one table: size, fill, wait (the staging memory may go out of scope)
template <typename T>
static int upload(pgd_engine* h, int table, const T* src, size_t n) {
  const int ids[1] = {table};
  const uint64_t bytes[1] = {sizeof(T) * n};
  int rc = arena_resize(h, ids, bytes, 1);
  if (rc || (rc = arena_fill(h, table, src, n))) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
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
  return upload(h, TB_SCEN_MAP, sm.data(), sm.size());
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
  const size_t n_respawn = h->d.sstride > h->d.V ? (size_t)h->d.n_scen * (h->d.sstride - h->d.V) : 0;
  {
    const int ids[2] = {TB_RESET_IMG, TB_RESPAWN_IMG};
    const uint64_t bytes[2] = {sizeof(VehRec) * (uint64_t)h->d.n_scen * h->d.V, sizeof(VehRec) * (uint64_t)n_respawn};
    int rc = arena_resize(h, ids, bytes, 2);
    if (rc) return rc;
  }
  const int blocks = (h->d.n_scen + h->d.epw - 1) / h->d.epw;
  hipLaunchKernelGGL(k_reset_image, dim3(blocks), dim3(WAVE), 0, h->stream, h->d, arena_ptr<RecPiece>(h, TB_RESET_IMG));
  HIPCHK(hipGetLastError());
  if (n_respawn) {
    hipLaunchKernelGGL(k_respawn_image, dim3((unsigned)((n_respawn + 255) / 256)), dim3(256), 0, h->stream, h->d, arena_ptr<RecPiece>(h, TB_RESPAWN_IMG));
    HIPCHK(hipGetLastError());
  }
  h->img_dirty = false;
  return PGD_OK;
}

// pgd_live_rows' scratch: the whole-engine call (group < 0) owns the first N A / CMP_BLOCK + 1 entries; behind them env group g of
// n_groups (<= N) owns the entries from (its first row) / CMP_BLOCK + g on: its ceil(rows / CMP_BLOCK) blocks end before the next
// group's first entry, and the last group's before N A / CMP_BLOCK + n_groups.  No two forms share an entry: a whole-engine call on the
// engine's stream and group calls on their streams may be in flight together.
static size_t live_scratch_whole(int N, int A) { return (size_t)N * (size_t)A / CMP_BLOCK + 1; }
static size_t live_scratch_entries(int N, int A) { return 2 * live_scratch_whole(N, A) + (size_t)N; }

// The three launches of the ordered compaction over indices first + [0, n) on `stream`; `counts`: ceil(n / CMP_BLOCK) entries of scratch
template <int PRED>
static int compact_launch(const uint32_t* d_flags, const uint8_t* d_done, int first, int n, uint32_t* counts, int32_t* d_list, int32_t* d_count,
                          hipStream_t stream) {
  const int n_blocks = (int)(((size_t)n + CMP_BLOCK - 1) / CMP_BLOCK);
  hipLaunchKernelGGL((k_compact<PRED, false>), dim3(n_blocks), dim3(CMP_THREADS), 0, stream, d_flags, d_done, first, n, counts, d_list);
  hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(CMP_THREADS), 0, stream, counts, n_blocks, d_count);
  hipLaunchKernelGGL((k_compact<PRED, true>), dim3(n_blocks), dim3(CMP_THREADS), 0, stream, d_flags, d_done, first, n, counts, d_list);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

// The shared tail of the two table uploads: no mask, hint or reset image is trusted across a change of the tables
static int tables_changed(pgd_engine* h) {
  h->img_dirty = true;  // running envs fall back to their own records until their next reset
  HIPCHK(hipMemsetAsync(h->d.imask, 0, sizeof(unsigned long long) * (size_t)h->d.N, h->stream));
  hipLaunchKernelGGL(k_clear_hints, dim3((h->d.N + 255) / 256), dim3(256), 0, h->stream, h->d.ei, h->d.N);
  HIPCHK(hipGetLastError());
  return build_reset_image(h);  // eagerly (needs maps + scenarios): pgd_step never allocates, so it can be graph-captured
}

// Everything a handle owns, and the handle: pgd_destroy, and pgd_create when it fails half way (every member is null until it is set)
static void engine_free(pgd_engine* h) {
  (void)hipStreamSynchronize(h->stream);
  if (h->jit_mod) { (void)hipModuleUnload(h->jit_mod); h->jit_mod = nullptr; h->jit_fn = nullptr; }
  void* bufs[] = {h->cmp_live, h->cmp_index, h->lk_act, h->rowz, h->d.rec, h->d.ei, h->d.imask, h->d.env_map, h->d_ids, h->arena};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  for (hipEvent_t ev : {h->ev0, h->ev1, h->ev_move, h->ev_ids})
    if (ev) (void)hipEventDestroy(ev);
  if (h->h_ids) (void)hipHostFree(h->h_ids);
  if (h->prof_ev) {
    for (hipEvent_t ev : *h->prof_ev) (void)hipEventDestroy(ev);
    delete h->prof_ev;
  }
  if (h->gstreams) {
    for (int g = 0; g < h->n_groups; ++g) { (void)hipStreamSynchronize(h->gstreams[g]); (void)hipStreamDestroy(h->gstreams[g]); }
    free(h->gstreams);
  }
  if (h->cmp_retired) {
    for (uint32_t* b : *h->cmp_retired) (void)hipFree(b);
    delete h->cmp_retired;
  }
  topdown_free(h);
  render_free(h);
  step_info_free(h);
  delete h->h_maps;
  delete h->h_scen;
  if (h->own_stream) (void)hipStreamDestroy(h->stream);
  if (h->retired) (void)hipStreamDestroy(h->retired);
  free(h);
}

// pgd_create behind its refusals: the device state of a zeroed handle for N x V slots.  A failure leaves the handle to the caller's engine_free.
static int engine_init(pgd_engine* h, const pgd_config* cfg, const Geometry& g, int device, void* hip_stream) {
  h->device = device;
  h->d.cfg = *cfg;
  h->d.N = cfg->num_envs; h->d.A = cfg->num_agents; h->d.T = cfg->num_traffic; h->d.V = g.V;
  h->d.D = g.D;
  h->d.NV = g.NV;
  h->d.ostride = h->d.A * h->d.D;  // (prow, unit_off: null / 0 from calloc; a step sets them in its launch copy)
  h->d.dbg_exit = 255;  // no exit mark, no ablation bits (exit-profile builds only)
  h->n_groups = 1;
  h->d.sstride = g.sstride; h->d.sub = g.sub; h->d.epw = g.epw; h->d.pack_obs = g.pack_obs; h->d.use_imask = g.use_imask;
  const bool marl = (cfg->marl_flags & PGD_MA_ENABLED) != 0;
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
  if (marl && !h->sw.no_rowz) {  // (PGD_NO_ROWZ=1: no marks -- every row that is not due is zero-filled by every call)
    HIPCHK(hipMalloc(&h->rowz, sizeof(ulonglong2) * (size_t)h->d.N));
    HIPCHK(hipMemsetAsync(h->rowz, 0, sizeof(ulonglong2) * (size_t)h->d.N, h->stream));
    h->d.rowz = h->rowz;
  }
  HIPCHK(hipMalloc(&h->cmp_live, sizeof(uint32_t) * live_scratch_entries(h->d.N, h->d.A)));
  HIPCHK(hipMalloc(&h->d.env_map, sizeof(pgd_map) * (size_t)h->d.N));
  HIPCHK(hipMemsetAsync(h->d.env_map, 0, sizeof(pgd_map) * (size_t)h->d.N, h->stream));
  HIPCHK(hipMalloc(&h->d.imask, sizeof(unsigned long long) * (size_t)h->d.N));  // (read while use_imask is set: imask_rule, pgd_host_prep.h)
  HIPCHK(hipMemsetAsync(h->d.imask, 0, sizeof(unsigned long long) * (size_t)h->d.N, h->stream));
  // beam i points at theta + i * 2 pi / n (distance_detector.py:65-94): its direction is the heading rotated by a
  // constant angle, tabulated once in double precision instead of one sincosf per beam and step
  std::vector<float2> bt((size_t)(cfg->num_lasers > 0 ? cfg->num_lasers : 1));
  for (int i = 0; i < cfg->num_lasers; ++i) {
    const double a = (double)i * (2.0 * 3.14159265358979323846 / (double)cfg->num_lasers);
    bt[(size_t)i] = make_float2((float)cos(a), (float)sin(a));
  }
  return upload(h, TB_BEAM, bt.data(), bt.size());
}

extern "C" {

const char* pgd_version(void) { return "pgdrive_hip 0.1 (gfx950)"; }
#ifndef PGD_SOURCE_SHA
#define PGD_SOURCE_SHA "unstamped"  // (an experimental build outside pgdrive_amd/build.py: no committed counter pass is its own)
#endif
const char* pgd_source_sha(void) { return PGD_SOURCE_SHA; }

int pgd_plan_arena(const uint64_t* bytes, int n, uint32_t* offsets, uint64_t* total) {
  if (!bytes || !offsets || !total || n <= 0) return PGD_ERR_ARG;
  const uint64_t limit = (1ull << 32) - (64ull << 10), align = 256;
  uint64_t at = 4096;  // (a record in front of a table's first -- index -1, read and discarded here and there -- stays inside the arena)
  for (int k = 0; k < n; ++k) {
    if (at > limit || bytes[k] > limit - at) return PGD_ERR_ARG;  // (compared before the add: 64-bit sizes cannot wrap the sum)
    offsets[k] = (uint32_t)at;
    at = (at + bytes[k] + align - 1) / align * align;
  }
  if (at > limit) return PGD_ERR_ARG;
  *total = at ? at : align;
  return PGD_OK;
}

int pgd_obs_dim(const pgd_config* c) { return obs_dim(*c); }

int pgd_create(const pgd_config* cfg, int device, void* hip_stream, pgd_handle* out) {
  if (!cfg || !out) return PGD_ERR_ARG;
  const Switches sw = read_switches();
  Geometry g;
  { int rc = plan_geometry(*cfg, sw.pack, sw.imask, g); if (rc) return rc; }  // (every refusal: before the first HIP call, nothing allocated)
  HIPCHK(hipSetDevice(device));
  pgd_engine* h = (pgd_engine*)calloc(1, sizeof(pgd_engine));
  if (!h) return PGD_ERR_STATE;
  h->sw = sw;
  const int rc = engine_init(h, cfg, g, device, hip_stream);
  if (rc) { engine_free(h); return rc; }
  *out = h;
  return PGD_OK;
}

// (the device forms are built first -- build_map_tables, which refuses a malformed bank before anything here has changed --, the arena
// is sized for all of them at once, then they are copied in)
int pgd_upload_maps(pgd_handle h, const pgd_map* maps, int n_maps, const pgd_lane* lanes, int n_lanes,
                    const pgd_road* roads, int n_roads, const pgd_box* boxes, int n_boxes, const int32_t* cs, int n_cs,
                    const int32_t* ci, int n_ci) {
  if (!h) return PGD_ERR_ARG;
  MapTables t;
  int rc = build_map_tables(maps, n_maps, lanes, n_lanes, roads, n_roads, boxes, n_boxes, cs, n_cs, ci, n_ci, t);
  if (rc) return rc;
  if (h->h_scen && !scenario_maps_ok(h->h_scen->data(), h->h_scen->size(), (size_t)n_maps)) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  const int ids[9] = {TB_MAPS, TB_LANES, TB_LANE_NAV, TB_ROADS, TB_BOXES, TB_CELL_ITEMS, TB_CELL_BOXES, TB_CELL_EXT, TB_CELL_START};
  const uint64_t bytes[9] = {sizeof(pgd_map) * (uint64_t)n_maps, sizeof(pgd_lane) * (uint64_t)n_lanes, sizeof(LaneNav) * (uint64_t)n_lanes,
                             sizeof(pgd_road) * (uint64_t)n_roads, sizeof(pgd_box) * (uint64_t)n_boxes, sizeof(int32_t) * (uint64_t)n_ci,
                             sizeof(pgd_box) * (uint64_t)n_ci, sizeof(LaneExt) * (uint64_t)n_ci, sizeof(int32_t) * (uint64_t)n_cs};
  if ((rc = arena_resize(h, ids, bytes, 9))) return rc;
  if ((rc = arena_fill(h, TB_MAPS, maps, (size_t)n_maps)) || (rc = arena_fill(h, TB_LANES, t.lanes.data(), (size_t)n_lanes)) ||
      (rc = arena_fill(h, TB_LANE_NAV, t.nav.data(), (size_t)n_lanes)) || (rc = arena_fill(h, TB_ROADS, roads, (size_t)n_roads)) ||
      (rc = arena_fill(h, TB_BOXES, boxes, (size_t)n_boxes)) || (rc = arena_fill(h, TB_CELL_ITEMS, ci, (size_t)n_ci)) ||
      (rc = arena_fill(h, TB_CELL_BOXES, t.cell_boxes.data(), (size_t)n_ci)) || (rc = arena_fill(h, TB_CELL_EXT, t.cell_ext.data(), (size_t)n_ci)) ||
      (rc = arena_fill(h, TB_CELL_START, t.cell_start.data(), (size_t)n_cs)))
    return rc;
  HIPCHK(hipStreamSynchronize(h->stream));  // (the staging vectors go out of scope)
  if (!h->h_maps) h->h_maps = new std::vector<pgd_map>();
  h->h_maps->assign(maps, maps + n_maps);
  if ((rc = build_scen_map(h))) return rc;
  h->have_maps = true;
  return tables_changed(h);
}

int pgd_upload_scenarios(pgd_handle h, const pgd_scenario* scen, int n_scen, const pgd_spawn* spawns) {
  if (!h) return PGD_ERR_ARG;
  ScenarioTables t;
  int rc = build_scenario_tables(scen, spawns, n_scen, h->d.sstride, h->sw.no_uni, t);
  if (rc) return rc;
  if (h->h_maps && !scenario_maps_ok(scen, (size_t)n_scen, h->h_maps->size())) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  const size_t ns = t.spawns.size();
  const int ids[3] = {TB_SCEN, TB_SPAWNS, TB_SPAWN_HV};
  const uint64_t bytes[3] = {sizeof(pgd_scenario) * (uint64_t)n_scen, sizeof(pgd_spawn) * (uint64_t)ns, sizeof(float2) * (uint64_t)ns};
  if ((rc = arena_resize(h, ids, bytes, 3)) || (rc = arena_fill(h, TB_SCEN, scen, (size_t)n_scen)) ||
      (rc = arena_fill(h, TB_SPAWNS, t.spawns.data(), ns)))
    return rc;
  HIPCHK(hipStreamSynchronize(h->stream));  // (the staging vector goes out of scope)
  h->d.n_scen = n_scen;
  hipLaunchKernelGGL(k_spawn_hv, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, h->stream, (const pgd_spawn*)arena_ptr<pgd_spawn>(h, TB_SPAWNS),
                     arena_ptr<float2>(h, TB_SPAWN_HV), ns);
  HIPCHK(hipGetLastError());
  h->d.no_groups = t.no_groups;
  h->has_objects = t.has_objects;
  h->d.uni_len = t.uni_len;
  h->d.uni_wid = t.uni_wid;
  if (!h->h_scen) h->h_scen = new std::vector<pgd_scenario>();
  h->h_scen->assign(scen, scen + n_scen);
  if ((rc = build_scen_map(h))) return rc;
  h->have_scen = true;
  return tables_changed(h);
}

int pgd_reset(pgd_handle h, const int32_t* env_ids, const int32_t* scen_ids, int n, float* d_obs) {
  if (!h || !scen_ids || n <= 0 || n > h->d.N) return PGD_ERR_ARG;
  if (!h->have_maps || !h->have_scen) return PGD_ERR_STATE;
  HIPCHK(hipSetDevice(h->device));
  for (int k = 0; k < n; ++k)
    if (scen_ids[k] < 0 || scen_ids[k] >= h->d.n_scen) return PGD_ERR_ARG;
  if (env_ids) {  // in range and no env twice (two units of k_reset would write one env at the same time)
    std::vector<uint8_t> seen((size_t)h->d.N, 0);
    for (int k = 0; k < n; ++k) {
      const int e = env_ids[k];
      if (e < 0 || e >= h->d.N || seen[(size_t)e]) return PGD_ERR_ARG;
      seen[(size_t)e] = 1;
    }
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
  { int rc = step_info_forget(h, d_env, n); if (rc) return rc; }  // and so do the running cost and the energy base of the step info
  // an id list: the rows of the listed envs and no others (the rest of d_obs keeps its bytes)
  if (d_obs) return launch_observe(h, observe_launch(h, d_env ? n : h->d.N, false), h->d, d_obs, nullptr, d_env, h->stream);
  return PGD_OK;
}

// One step: validate, plan, open the timing bracket, launch, close the bracket.
static int step_impl(pgd_handle h, const float* d_actions, float* d_obs, float* d_reward, uint8_t* d_done, uint32_t* d_flags,
                     int ostride, bool packed, int group = -1) {
  if (!h || !d_actions || !d_reward || !d_done || !d_flags) return PGD_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(d_actions) & 7u) != 0u) return PGD_ERR_ARG;  // k_step reads an agent's action pair with one 8-byte load
  if (!h->have_maps || !h->have_scen) return PGD_ERR_STATE;
  if (h->img_dirty) return PGD_ERR_STATE;  // the reset image is built by the upload calls
  if (h->sinfo && packed) return PGD_ERR_STATE;  // step info: no terminal rows through the packed rows of the gather (pgdrive_hip.h)
  HIPCHK(hipSetDevice(h->device));
  StepPlan p;
  { int rc = plan_step(h, d_obs != nullptr, group, p); if (rc) return rc; }
  bool prof = h->prof_ev && h->prof_n < h->prof_cap && group < 0;
  // strided profile: with the observation fused (one kernel per step) events [0] / [1] bracket a GROUP of `stride`
  // back-to-back launches and the group time is divided by the stride; otherwise every stride-th step is bracketed
  const bool grouped = prof && h->prof_stride > 1 && p.fuse;
  bool g_open = false, g_close = false;
  if (prof && h->prof_stride > 1) {
    const int ph = h->prof_tick++ % h->prof_stride;
    if (grouped) { g_open = ph == 0; g_close = ph == h->prof_stride - 1; prof = false; }
    else prof = ph == 0;
  }
  hipEvent_t* pe = (prof || g_open || g_close) ? &(*h->prof_ev)[(size_t)h->prof_n * 3] : nullptr;
  const bool timing = h->step_timing && !prof && !grouped && group < 0;
  if (prof || timing || g_open) HIPCHK(hipEventRecord((prof || g_open) ? pe[0] : h->ev0, h->stream));
  PgdDev dv = h->d;  // this launch's output addressing
  dv.ostride = ostride;
  dv.prow = packed ? d_obs : nullptr;
  dv.obs_g = observers_per_round(h->d, h->d.A, 1, 0, STEP_MINB_WORDS);  // fused multi-agent observation: what the step's LDS holds
  dv.unit_off = p.g.first / h->d.epw;
  dv.state_rows = p.state_in_step ? d_obs : nullptr;
  if (h->sinfo) dv.cfg.auto_reset = 0;  // step info: the step leaves the terminal state and row, k_step_info restarts the env (pgd_step_info.h)
  PgdCold cold_arg{dv.bev_fill, dv.o_scen_map, dv.o_spawn_hv, dv.o_respawn_img, dv.n_scen, dv.cfg.seed, dv.cfg.env_base,
                   h->lk.obs, h->lk.k_lat, h->lk.k_head, h->lk.v_target, h->lk.noise, h->lk.tick};
  float* obs_arg = p.fuse ? d_obs : (float*)nullptr;
  const int blocks = (p.g.count + h->d.epw - 1) / h->d.epw;
  if (p.jit_fn) {
    h->last_step_kernel = h->jit_name;
    void* kargs[] = {&dv, &d_actions, &d_reward, &d_done, &d_flags, &obs_arg, &cold_arg};
    HIPCHK(hipModuleLaunchKernel(p.jit_fn, (unsigned)blocks, 1, 1, WAVE, 1, 1, 0, p.g.stream, kargs, nullptr));
  } else {
    h->last_step_kernel = p.kernel.name;
    hipLaunchKernelGGL(p.kernel.fn, dim3(blocks), dim3(WAVE), 0, p.g.stream, dv, d_actions, d_reward, d_done, d_flags, obs_arg, cold_arg);
  }
  HIPCHK(hipGetLastError());
  if (prof || g_close) HIPCHK(hipEventRecord(pe[1], h->stream));
  if (g_close) h->prof_n += 1;
  if (p.obs.k.range) {
    int rc = launch_observe(h, p.obs, dv, d_obs, is_marl(h) ? d_flags : (const uint32_t*)nullptr, nullptr, p.g.stream);
    if (rc) return rc;
  }
  if (h->sinfo) { int rc = step_info_launch(h, p.g, d_done, d_flags, d_obs); if (rc) return rc; }
  h->prof_fused = p.fuse;
  h->prof_grouped = grouped;
  if ((prof && !p.fuse) || timing) HIPCHK(hipEventRecord(prof ? pe[2] : h->ev1, h->stream));  // fused: [0],[1] bracket the only kernel
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
  if (h->sinfo) return PGD_ERR_STATE;  // step info is per step: one slice of reward / done / flags, one terminal row (pgdrive_hip.h)
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
  if (!h) return PGD_ERR_ARG;
  // the new geometry is worked out first and committed only when every check has passed (a refused call leaves the engine as it
  // was); leaving throughput mode is reported: pgd_describe_step says so from then on
  const Geometry now{h->d.V, h->d.D, h->d.NV, h->d.sstride, h->d.sub, h->d.epw, h->d.pack_obs, h->d.use_imask};
  Geometry geo;
  bool left_pack;
  { int rc = regroup_geometry(now, h->d.N, n_groups, h->sw.imask, geo, &left_pack); if (rc) return rc; }
  if (left_pack) h->left_pack_mode = true;
  h->d.pack_obs = geo.pack_obs; h->d.sub = geo.sub; h->d.epw = geo.epw;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (geo.use_imask != h->d.use_imask) {  // (the masks are only kept up while they are read: none is trusted across the switch)
    HIPCHK(hipMemsetAsync(h->d.imask, 0, sizeof(unsigned long long) * (size_t)h->d.N, h->stream));
    h->d.use_imask = geo.use_imask;
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
  { int rc = raise_lds_limit(h, final_tanh ? LDS_MLP_TANH : LDS_MLP, reinterpret_cast<const void*>(kern), lds); if (rc) return rc; }
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
  { int rc = raise_lds_limit(h, final_tanh ? LDS_MLP_BF_TANH : LDS_MLP_BF, reinterpret_cast<const void*>(kern), lds); if (rc) return rc; }
  hipLaunchKernelGGL(kern, dim3((rows + MLP_ROWS - 1) / MLP_ROWS), dim3(WAVE * MLP_WAVES), lds, g.stream, d_obs, row0, rows, obs_stride, in_dim,
                     reinterpret_cast<const uint4*>(d_prepared), d_actions);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

/* ---- actor + critic of a rollout in one launch, and GAE behind it (pgd_actor_critic.h) -------------------------------------------- */
int pgd_actor_critic_tick(pgd_handle h, const uint32_t* d_tick) {
  if (!h || (reinterpret_cast<uintptr_t>(d_tick) & 3u) != 0u) return PGD_ERR_ARG;
  h->ac_tick = d_tick;
  return PGD_OK;
}

int pgd_mlp_actor_critic(pgd_handle h, int group, const float* d_obs, int obs_stride, int in_dim, const pgd_actor_critic* nets, uint32_t seed,
                         uint32_t tick, uint32_t flags, float* d_actions, float* d_logp, float* d_value) {
  bool critic;
  if (!h || !d_obs || !d_actions || !d_logp || (flags & ~PGD_AC_DETERMINISTIC) != 0u || !nets_ok(nets, nullptr, true, in_dim, obs_stride, &critic) ||
      (critic && !d_value) || ac_lds_bytes(in_dim) > 65536) return PGD_ERR_ARG;
  return ac_forward(h, group, LDS_AC, k_mlp_actor_critic<false>, k_mlp_actor_critic<true>, in_dim, [&](const AcRows& r, auto kern) {
    hipLaunchKernelGGL(kern, dim3((r.rows + MLP_ROWS - 1) / MLP_ROWS, critic ? 2 : 1), dim3(WAVE * MLP_WAVES), r.lds, r.stream, d_obs,
                       r.row0, r.rows, obs_stride, in_dim, *nets, seed, tick, h->ac_tick, r.row_base, flags, d_actions, d_logp, d_value, r.nm);
  });
}

int pgd_gae(pgd_handle h, const float* d_reward, const float* d_value, const uint8_t* d_done, int T, int rows, float gamma, float lam,
            float* d_adv, float* d_ret) {
  if (!h || !d_reward || !d_value || !d_done || !d_adv || !d_ret || T < 1 || rows < 1) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_gae, dim3((rows + WAVE - 1) / WAVE), dim3(WAVE), 0, h->stream, d_reward, d_value, d_done, T, rows, gamma, lam, d_adv,
                     d_ret);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

/* ---- rollouts of multi-agent engines: live rows, the networks over a row list, masked GAE (pgd_marl_rollout.h) --------------------- */
int pgd_live_rows(pgd_handle h, int group, const uint32_t* d_flags, const uint8_t* d_done, int32_t* d_rows, int32_t* d_count) {
  if (!h || !d_flags || !d_done || !d_rows || !d_count) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  EnvGroup g;
  { int rc = env_group(h, group, g); if (rc) return rc; }
  const int rows = g.count * h->d.A, row0 = g.first * h->d.A;
  uint32_t* counts = group < 0 ? h->cmp_live : h->cmp_live + live_scratch_whole(h->d.N, h->d.A) + (size_t)(row0 / CMP_BLOCK + group);
  return compact_launch<CMP_LIVE>(d_flags, d_done, row0, rows, counts, d_rows, d_count, g.stream);
}

int pgd_rollout_index(pgd_handle h, const uint32_t* d_flags, int T, int rows, int32_t* d_index, int32_t* d_count) {
  if (!h || !d_flags || !d_index || !d_count || T < 1 || rows < 1 || (long long)T * rows > PGD_ROLLOUT_INDEX_MAX) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  const int n = T * rows;
  const size_t n_blocks = ((size_t)n + CMP_BLOCK - 1) / CMP_BLOCK;
  if (n_blocks > h->cmp_index_cap) {  // (a larger rollout than any before: new scratch, which a capture cannot take)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(h->stream, &cap);
    if (cap != hipStreamCaptureStatusNone) return PGD_ERR_STATE;
    // the old scratch stays until pgd_destroy: launches in flight read it, and a graph captured with it may be replayed at any time
    uint32_t* grown = nullptr;
    HIPCHK(hipMalloc(&grown, sizeof(uint32_t) * n_blocks));
    if (h->cmp_index) {
      if (!h->cmp_retired) h->cmp_retired = new std::vector<uint32_t*>();
      h->cmp_retired->push_back(h->cmp_index);
    }
    h->cmp_index = grown;
    h->cmp_index_cap = n_blocks;
  }
  return compact_launch<CMP_ACTED>(d_flags, nullptr, 0, n, h->cmp_index, d_index, d_count, h->stream);
}

int pgd_mlp_actor_critic_rows(pgd_handle h, int group, const float* d_obs, int obs_stride, int in_dim, const pgd_actor_critic* nets, uint32_t seed,
                              uint32_t tick, uint32_t flags, const int32_t* d_rows, const int32_t* d_count, float* d_actions, float* d_logp,
                              float* d_value) {
  bool critic;
  if (!h || !d_obs || !d_rows || !d_count || !d_actions || !d_logp || (flags & ~PGD_AC_DETERMINISTIC) != 0u ||
      !nets_ok(nets, nullptr, true, in_dim, obs_stride, &critic) || (critic && !d_value) || ac_lds_bytes(in_dim) > 65536) return PGD_ERR_ARG;
  return ac_forward(h, group, LDS_AC_ROWS, k_mlp_actor_critic_rows<false>, k_mlp_actor_critic_rows<true>, in_dim, [&](const AcRows& r, auto kern) {
    // the defined outputs of the rows that are not listed, then the listed rows (the host does not know how many: a grid for all)
    hipLaunchKernelGGL(k_ac_clear_rows, dim3((r.rows + CMP_THREADS - 1) / CMP_THREADS), dim3(CMP_THREADS), 0, r.stream, r.row0, r.rows, d_actions,
                       d_logp, critic ? d_value : nullptr);
    hipLaunchKernelGGL(kern, dim3((r.rows + MLP_ROWS - 1) / MLP_ROWS, critic ? 2 : 1), dim3(WAVE * MLP_WAVES), r.lds, r.stream,
                       d_obs, d_rows, d_count, r.row0, r.rows, obs_stride, in_dim, *nets, seed, tick, h->ac_tick, r.row_base, flags, d_actions,
                       d_logp, d_value, r.nm);
  });
}

int pgd_gae_masked(pgd_handle h, const float* d_reward, const float* d_value, const uint8_t* d_done, const uint32_t* d_flags, int T, int rows,
                   float gamma, float lam, float* d_adv, float* d_ret, uint8_t* d_mask) {
  if (!h || !d_reward || !d_value || !d_done || !d_flags || !d_adv || !d_ret || !d_mask || T < 1 || rows < 1) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_gae_masked, dim3((rows + WAVE - 1) / WAVE), dim3(WAVE), 0, h->stream, d_reward, d_value, d_done, d_flags, T, rows, gamma,
                     lam, d_adv, d_ret, d_mask);
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
  snprintf(buf, (size_t)cap, "%s%s%s", h->last_step_kernel ? h->last_step_kernel : "",
           (h->sinfo && h->last_step_kernel) ? " + k_step_info (step info: the step kernel never restarts an env, this kernel does)" : "",
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
  return launch_observe(h, observe_launch(h, h->d.N, false), h->d, d_obs, nullptr, nullptr, h->stream);
}

int pgd_state_dims(pgd_handle h, int* nf, int* ni, int* nei) {
  (void)h;
  if (nf) *nf = PGD_NF;
  if (ni) *ni = PGD_NI;
  if (nei) *nei = PGD_NEI;
  return PGD_OK;
}

// ABI order is field-major ([field][env*V + slot], [field][env]); the device keeps one 128 B record per vehicle and one
// PGD_NEI-int row per env -- converted on the host (state_to_fields / state_from_fields, pgd_host_prep.h)
static_assert(sizeof(RecUnit) == sizeof(RecPiece), "the host copy of the records is the device's piece planes");
int pgd_get_state(pgd_handle h, float* f, int32_t* i, int32_t* ei) {
  if (!h || !f || !i || !ei) return PGD_ERR_ARG;
  const size_t nv = (size_t)h->d.NV;
  HIPCHK(hipSetDevice(h->device));
  std::vector<RecUnit> tr(nv * 8);
  std::vector<int32_t> te((size_t)h->d.N * PGD_NEI);
  HIPCHK(hipMemcpyAsync(tr.data(), h->d.rec, sizeof(VehRec) * nv, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(te.data(), h->d.ei, sizeof(int32_t) * te.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  state_to_fields(tr.data(), te.data(), h->d.N, h->d.V, f, i, ei);
  return PGD_OK;
}
int pgd_set_state(pgd_handle h, const float* f, const int32_t* i, const int32_t* ei) {
  if (!h || !f || !i || !ei) return PGD_ERR_ARG;
  const size_t nv = (size_t)h->d.NV;
  std::vector<RecUnit> tr(nv * 8);
  std::vector<int32_t> te((size_t)h->d.N * PGD_NEI);
  { int rc = state_from_fields(f, i, ei, h->d.N, h->d.V, tr.data(), te.data()); if (rc) return rc; }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(h->d.rec, tr.data(), sizeof(VehRec) * nv, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d.ei, te.data(), sizeof(int32_t) * te.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(h->d.imask, 0, sizeof(unsigned long long) * (size_t)h->d.N, h->stream));  // arbitrary records: none is the image
  h->derive_pending = true;
  { int rc = derive_records(h); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));
  return PGD_OK;
}

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
  engine_free(h);
  return PGD_OK;
}

}  // extern "C"

#include "pgd_topdown.h"
#include "pgd_render.h"
#include "pgd_gather.h"
#include "pgd_step_info.h"
#include "pgd_ppo.h"
#include "pgd_safe.h"
#include "pgd_guided.h"
#include "pgd_categorical.h"
#include "pgd_timelimit.h"
#include "pgd_guardian.h"
#include "pgd_return_norm.h"
#include "pgd_obs_norm.h"
#include "pgd_rollout_episodes.h"
#include "pgd_minibatch.h"
#endif  // !PGD_JIT
