// pgd_kernels.h -- the small kernels around the step: spawn headings, reset / respawn images, reset, derive, refresh, the stand-alone
// observation kernels, the scripted lane-keeping policy.  Part of the single translation unit pgd_engine.hip (included there after
// pgd_step.h, whose lane mapping and write_fixed_config they use; not part of a -DPGD_JIT build).
//   k_observe  one block per (env, agent): wave 0 compacts the bodies inside the lidar broad phase into LDS with a ballot,
//              then every thread casts beams against the compacted bodies and the row is written coalesced.

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
  const Tab<pgd_spawn> sp = d.spawns() + (size_t)scen * d.sstride + s;
  MapView mv = map_view(d, d.scen()[scen].map);
  reset_vehicle(*sp, d.spawn_hv()[(size_t)scen * d.sstride + s], r, s, s < A && !d.cfg.idm_agent);
  RouteCtx ctx;
  if (r.status != ST_EMPTY) {
    route_refresh(mv, sp, r);
    after_step_vehicle(d.cfg, mv, g, sp, *sp, r, s < A, true, ctx);
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
  const Tab<pgd_spawn> sp = d.spawns() + (size_t)scen * d.sstride + idx;
  MapView mv = map_view(d, d.scen()[scen].map);
  Veh r;
  reset_vehicle(*sp, d.spawn_hv()[(size_t)scen * d.sstride + idx], r, idx, true);
  RouteCtx ctx;
  if (r.status != ST_EMPTY) {
    route_refresh(mv, sp, r);
    after_step_vehicle(d.cfg, mv, g, sp, *sp, r, true, true, ctx);
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
    d.env_map[e] = d.scen_map()[scen];
    if (d.bev_fill) d.bev_fill[e] = 1;
    d.imask[e] = ((d.epw == 1 || d.pack_obs) && d.use_imask) ? (d.V >= 64 ? ~0ull : ((1ull << d.V) - 1ull)) : 0ull;  // every record equals the image now
    d.ei[(size_t)(e) * PGD_NEI + EI_NEXT_AGENT] = A == 1 ? 1 : __popcll(am);
    d.ei[(size_t)(e) * PGD_NEI + EI_AUX] = d.scen()[scen].aux;  // parking: free spaces of the new episode
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
  if (k == e * d.V && scen >= 0 && scen < d.n_scen) d.env_map[e] = d.scen_map()[scen];  // the env's copy of its map header
  if (r.status != ST_EMPTY && scen >= 0 && scen < d.n_scen && (int)r.spawn < d.sstride) {
    const MapView mv = map_view(d, d.scen()[scen].map);
    const Tab<pgd_spawn> sp = d.spawns() + ((size_t)scen * d.sstride + r.spawn);
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
  MapView mv = map_view(d, d.scen()[scen].map);
  RouteCtx ctx;
  after_step_vehicle(d.cfg, mv, g, d.spawns() + ((size_t)scen * d.sstride + r.spawn), d.spawns()[(size_t)scen * d.sstride + r.spawn], r, s < A, true, ctx);
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
#define OBS_BOUNDS(BLOCK) __launch_bounds__((BLOCK) == WAVE ? WAVE * OBS_RPB : (BLOCK))
// The one body of k_observe and k_observe_ids.  Row `rowi` of the launch belongs to unit u = rowi / A: ENV is the env of unit u, FLAGS the
// step flags.  A macro, not a function: a function between a kernel and observe_row is optimised on its own before it is inlined, and
// every kernel then compiles to other instructions (compared per symbol, tools/asm_by_kernel.py).
#define OBSERVE_ROWS(FLAGS, ENV)                                                                                      \
  constexpr bool WROW = BLOCK == WAVE;                                                                                \
  __shared__ ObsLds Ls[WROW ? OBS_RPB : 1];                                                                           \
  const int rowi = WROW ? (int)blockIdx.x * OBS_RPB + (int)(threadIdx.x / WAVE) : (int)blockIdx.x;                    \
  if (rowi >= n_rows) return;                                                                                         \
  const int u = rowi / d.A;                                                                                           \
  observe_row<BLOCK, OTH>(d, obs, FLAGS, ENV, rowi % d.A, WROW ? (int)(threadIdx.x % WAVE) : (int)threadIdx.x, Ls[WROW ? threadIdx.x / WAVE : 0])
// unit u = env u of the launch's env range, with the step's flags
template <int BLOCK, bool OTH>
__global__ OBS_BOUNDS(BLOCK) void k_observe(PgdDev d, float* __restrict__ obs, const uint32_t* __restrict__ flags, int n_rows) {
  OBSERVE_ROWS(flags, u + d.unit_off * d.epw);
}
// unit u = env env_ids[u] and nothing else (pgd_reset with env ids): the rows of every other env keep their bytes, and so do their
// zero-row marks.  A kernel of its own, so that the one a step launches stays as it is; no step flags (the state right after a reset).
template <int BLOCK, bool OTH>
__global__ OBS_BOUNDS(BLOCK) void k_observe_ids(PgdDev d, float* __restrict__ obs, const int32_t* __restrict__ env_ids, int n_rows) {
  OBSERVE_ROWS(nullptr, env_ids[u]);
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
// FIX: the engine runs the default multi-agent configuration (same constants as k_step's instantiation for it, PGD_FIXM_FIELDS)
// STATE = false: k_step has written the state blocks of the rows that are due (PgdDev::state_rows): the pairwise part only
// (the library is built at -O2 since the end of round 5; this kernel keeps the size-optimised code it had -- 30.0 against 30.7 us for the
// 40 seats -- and its specialised instantiations seven waves per SIMD: 72 registers, what -Os gave them unasked; at -O2 they took 82 and
// the observation 32.6 us)
#ifndef PGD_KOE_ATTR
#define PGD_KOE_ATTR __attribute__((minsize))
#endif
#define OBS_ENV_BOUNDS(NW, FIX) PGD_KOE_ATTR __launch_bounds__(WAVE * (NW), ((FIX) ? 7 : 1))
// The one body of k_observe_env and k_observe_env_ids (a macro for the reason given at OBSERVE_ROWS): block u of the launch observes env ENV
#define OBSERVE_ENV(STATE, FLAGS, ENV)                                                                                \
  if (FIX) write_fixed_config<true, true, false, (SEATS ? SEATS : 1)>(d);                                             \
  extern __shared__ unsigned s_minb_dyn[];                                                                            \
  constexpr int CAP = SEATS ? (SEATS / 1000 + 15) / 16 * 16 : WAVE;                                                   \
  __shared__ ObsEnvLds<NW, CAP> M;                                                                                    \
  PHASE_INIT(); /* (profile builds: the marks of observe_env_body count from here) */                                 \
  const unsigned u = blockIdx.x;                                                                                      \
  observe_env_body<NW, !FIX, false, !FIX, STATE, CAP>(d, ENV, obs, FLAGS, M, s_minb_dyn, G) /* (the fixed-config kernel: no traffic objects) */
template <int NW, bool FIX = false, bool STATE = true, int SEATS = 0>  // SEATS: the seat count folded as well (PGD_FIXM_SEAT_FIELDS)
__global__ OBS_ENV_BOUNDS(NW, FIX) void k_observe_env(PgdDev d, float* __restrict__ obs, const uint32_t* __restrict__ flags, int G) {
  OBSERVE_ENV(STATE, flags, (int)u + d.unit_off * d.epw);
}
template <int NW, bool FIX = false, int SEATS = 0>  // an id list: see k_observe_ids
__global__ OBS_ENV_BOUNDS(NW, FIX) void k_observe_env_ids(PgdDev d, float* __restrict__ obs, const int32_t* __restrict__ env_ids, int G) {
  OBSERVE_ENV(true, nullptr, env_ids[u]);
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
