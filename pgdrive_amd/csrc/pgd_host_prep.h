// pgd_host_prep.h -- the GPU-free preparation behind the ABI entry points of pgd_engine.hip, as pure functions over host memory: the launch
// geometry of an engine (pgd_create, pgd_set_groups), the device forms of the map and scenario tables (pgd_upload_maps,
// pgd_upload_scenarios) and the conversion between the ABI's field-major state and the device records (pgd_get_state / pgd_set_state).
// Each function validates everything it reads before the caller touches the handle or the device: a refused call leaves the engine as it
// was.  Includes no HIP header (pgd_records.h has the records and constants): tests/host_prep_main.cpp compiles it with the host
// compiler under the sanitizers, tests/test_host_prep_cpu.py holds its results to tests/host_prep_ref.py.
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "pgd_records.h"

// ---------------------------------------------------------------------------------------------------------------------
// geometry: how the slots of an env map onto the lanes of a wave
// ---------------------------------------------------------------------------------------------------------------------
inline int obs_dim(const pgd_config& c) {
  const int toll = (c.marl_flags & PGD_MA_TOLLGATE) != 0;
  const int state = (c.side_lasers > 0 ? c.side_lasers : 2) + 6 + c.lane_line_lasers + (c.random_agent_model ? 2 : 0) +
                    (toll ? 0 : PGD_NAVI_DIM);
  const int per_other = (c.marl_flags & PGD_MA_OTHERS_STATE) ? state : 4;
  return state + per_other * c.num_others + c.num_lasers + (toll ? 2 : 0);
}

struct Geometry { int V, D, NV, sstride, sub, epw, pack_obs, use_imask; };

// one env per wave (or, with few slots, several whole envs of `sub` lanes per slot): sub-lanes per vehicle, whole environments per wave
inline void one_env_lanes(int V, int& sub, int& epw) {
  sub = WAVE / V < 16 ? WAVE / V : 16;
  epw = WAVE / (V * sub);
}
// never-written slots are read from the scenario's reset image (cache resident, shared by every env of the scenario) instead
// of the env's own record: halves the HBM bytes of a step and is worth +13 % at 262144 envs.  THROUGHPUT MODE ONLY (several envs
// per wave, from 32768 envs on): with one env per wave the step is bound by its chain of memory round trips, and the mask is one
// of them -- mask + scenario id -> records -> ...; without it the records' reads go out at once (round 5: 4096 envs 17.38 -> 17.12 us,
// 16384 envs 47.3 -> 46.8, 8 agents 22.4 -> 22.1, 40 seats' step 27.7 -> 27.0; 32768 envs in throughput mode 77.2 -> 77.7 without
// the image).  PGD_NO_IMASK=1 / PGD_IMASK=1 (`imask` 0 / 1, -1 = not forced) force it off / on (A/B; the specialised kernels are
// compiled for the default).
inline int imask_rule(int imask, int pack_obs) { return imask >= 0 ? imask : (pack_obs ? 1 : 0); }

// The geometry of a new engine, with every argument refusal of pgd_create.  pack / imask: the PGD_PACK and PGD_IMASK / PGD_NO_IMASK
// switches, -1 = not forced.
inline int plan_geometry(const pgd_config& c, int pack, int imask, Geometry& g) {
  const int V = c.num_agents + c.num_traffic;
  if (c.num_envs <= 0 || c.num_agents <= 0 || V > MAXV || c.num_others > 16 || c.num_lasers < 0) return PGD_ERR_ARG;
  const bool marl = (c.marl_flags & PGD_MA_ENABLED) != 0;
  // multi-agent engines have no IDM traffic; num_traffic slots may hold static bodies (toll booths, group PGD_GROUP_NEVER)
  if (marl && (c.respawn_places < 0 || c.respawn_places > 64 || c.respawn_dests < 0)) return PGD_ERR_ARG;  // (free places: one 64-bit mask)
  if (c.idm_agent && (marl || c.num_agents != 1)) return PGD_ERR_ARG;  // the agent's PID / routing fields double as multi-agent bookkeeping
  if (marl && c.horizon > 0x7fff) return PGD_ERR_ARG;  // the per-agent episode length is a 16-bit field of the record
  g.V = V;
  g.D = obs_dim(c);
  g.NV = c.num_envs * V;
  g.sstride = V + (marl ? c.respawn_places * c.respawn_dests : 0);
  one_env_lanes(V, g.sub, g.epw);
  if (marl) g.epw = 1;  // (the multi-agent tail needs the env alone in its wave)
  g.pack_obs = 0;
  // Throughput mode: at large N the step is bound by instruction issue, not by the latency of one wave (profiles/r02_sweep.md:
  // 4.2 ns per env-step from 32768 envs on), and the SUB lanes of a vehicle run its scalar phases redundantly.  Engines with
  // >= 32768 single-ego envs (PGD_PACK=1 / 0 overrides; measured against the one-env kernel, profiles/r03_sweep.md: -7 % at 16384 envs, +6 % at 32768, +18 % at 262144) carry one vehicle per lane and as many whole envs per wave as fit --
  // three at V = 17 -- with the lidar observation of each env appended to the same launch.
  const int epw1 = std::min(WAVE / V, FUSE_MAX_AGENTS);
  const bool can_pack = !marl && c.num_agents == 1 && c.num_traffic >= 1 && epw1 >= 2 && epw1 * V <= PGD_SUBV && c.num_lasers > 0;
  const bool want_pack = pack >= 0 ? pack != 0 : c.num_envs >= 32768;
  if (can_pack && want_pack) { g.sub = 1; g.epw = epw1; g.pack_obs = 1; }
  g.use_imask = imask_rule(imask, g.pack_obs);
  return PGD_OK;
}

// pgd_set_groups: the geometry of `in` with N envs in n_groups equal groups.  Groups are launched as whole waves.  Throughput mode
// (plan_geometry picks it from 32768 envs on: three envs of 17 slots per wave) does not divide a power-of-two group size: such an
// engine goes back to one env per wave -- the record, image and mask layouts do not depend on the lane mapping, so the switch is a
// change of launch geometry only -- and *left_pack says so (by the r03 sweep it costs 6 - 18 % at 32768 envs).  A refusal leaves
// `out` equal to `in`.
inline int regroup_geometry(const Geometry& in, int N, int n_groups, int imask, Geometry& out, bool* left_pack) {
  out = in;
  *left_pack = false;
  if (n_groups < 1 || n_groups > 64) return PGD_ERR_ARG;
  if (N % n_groups != 0) return PGD_ERR_ARG;  // equal groups
  if ((N / n_groups) % in.epw == 0) return PGD_OK;
  if (!in.pack_obs) return PGD_ERR_ARG;
  Geometry g = in;
  g.pack_obs = 0;
  one_env_lanes(g.V, g.sub, g.epw);
  if ((N / n_groups) % g.epw != 0) return PGD_ERR_ARG;
  g.use_imask = imask_rule(imask, 0);
  out = g;
  *left_pack = true;
  return PGD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// map tables
// ---------------------------------------------------------------------------------------------------------------------
// [first, first + count) lies inside an array of n elements
inline bool range_ok(long long first, long long count, long long n) { return first >= 0 && count >= 0 && first + count <= n; }

// Every index that build_map_tables forms, held against the array it indexes (the function itself then reads without checks): the
// arrays are there, every map's lanes, roads, boxes, cells and items lie inside them, a cell's items run forward inside the map's,
// and a cell item names a box of its map.  Plus the limits of the packed device forms: 12-bit road ids, 16-bit lane ids, 24-bit
// item offsets.
inline bool map_bank_ok(const pgd_map* maps, int n_maps, const pgd_lane* lanes, int n_lanes, const pgd_road* roads, int n_roads,
                        const pgd_box* boxes, int n_boxes, const int32_t* cs, int n_cs, const int32_t* ci, int n_ci) {
  if (!maps || n_maps <= 0 || n_lanes < 0 || n_roads < 0 || n_boxes < 0 || n_cs < 0 || n_ci < 0) return false;
  if ((!lanes && n_lanes) || (!roads && n_roads) || (!boxes && n_boxes) || (!cs && n_cs) || (!ci && n_ci)) return false;
  for (int m = 0; m < n_maps; ++m) {
    const pgd_map& M = maps[m];
    if (M.n_roads > 4095 || M.n_lanes > 65535) return false;  // packed ids of the device record: 12-bit road ids, 16-bit lane ids
    if (!range_ok(M.lane_off, M.n_lanes, n_lanes) || !range_ok(M.road_off, M.n_roads, n_roads) || !range_ok(M.box_off, M.n_boxes, n_boxes))
      return false;
    if (M.gx < 0 || M.gy < 0) return false;
    const long long n_cells = (long long)M.gx * M.gy;
    if (!range_ok(M.cell_off, n_cells + 1, n_cs)) return false;
    const int32_t* start = cs + M.cell_off;
    if (start[0] < 0 || start[n_cells] >= (1 << 24) || !range_ok(M.item_off, start[n_cells], n_ci)) return false;
    for (long long c = 0; c < n_cells; ++c)
      if (start[c] > start[c + 1]) return false;
    for (int k = start[0]; k < start[n_cells]; ++k)
      if (ci[M.item_off + k] < 0 || ci[M.item_off + k] >= M.n_boxes) return false;
  }
  return true;
}

// the device forms of the map tables (pgd_upload_maps copies each into its table of the arena)
struct MapTables {
  std::vector<pgd_lane> lanes;       // the lane table with the device-private uses of ex, ey and pad (below)
  std::vector<LaneNav> nav;          // per lane
  std::vector<pgd_box> cell_boxes;   // cell-major copies of the boxes, lane boxes first inside each cell
  std::vector<LaneExt> cell_ext;     // same indexing
  std::vector<int32_t> cell_start;   // first item | lane boxes << 24
};

inline int build_map_tables(const pgd_map* maps, int n_maps, const pgd_lane* lanes, int n_lanes, const pgd_road* roads, int n_roads,
                            const pgd_box* boxes, int n_boxes, const int32_t* cs, int n_cs, const int32_t* ci, int n_ci, MapTables& out) {
  if (!map_bank_ok(maps, n_maps, lanes, n_lanes, roads, n_roads, boxes, n_boxes, cs, n_cs, ci, n_ci)) return PGD_ERR_ARG;
  std::vector<pgd_lane>& dl = out.lanes;
  dl.assign(lanes, lanes + n_lanes);
  std::vector<LaneNav>& nav = out.nav;
  nav.assign((size_t)(n_lanes > 0 ? n_lanes : 1), LaneNav{});
  {
    for (int m = 0; m < n_maps; ++m)
      for (int k = 0; k < maps[m].n_lanes; ++k) {
        pgd_lane& L = dl[(size_t)maps[m].lane_off + k];
        if (L.road < 0 || L.road >= maps[m].n_roads) return PGD_ERR_ARG;
        const pgd_road& R = roads[maps[m].road_off + L.road];
        if (R.first_lane + L.index != k) return PGD_ERR_ARG;  // (the lanes of a road are consecutive: neighbour lanes follow from the lane id alone)
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
            if (hi_lon < -0.05 || lo_lon > (double)L.length + 0.05) continue;  // (the car lies within [0, length]: see above)
            if (lo_lat <= 0.0 && hi_lat >= 0.0) clear = 0.0;
            else clear = std::min(clear, std::min(fabs(lo_lat), fabs(hi_lat)));
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
        L.pad = roads[(size_t)maps[m].road_off + L.road].from;  // (L.road is in range: checked above)
      }
    }
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
  }
  // cell-major copies of the boxes: cell_boxes[item_off + k] = boxes[box_off + cell_items[item_off + k]] — one dependent
  // load less per box in the grid walks, and a cell's boxes are contiguous (coalesced across sub-lanes)
  {
    // Inside each cell the lane-surface boxes are moved to the front (stable), and the device copy of cell_start packs
    // the number of lane boxes into the top byte (see cell_first / cell_mid).
    std::vector<pgd_box>& cb = out.cell_boxes;
    std::vector<LaneExt>& cx = out.cell_ext;
    std::vector<int32_t>& cs2 = out.cell_start;
    cb.assign((size_t)(n_ci > 0 ? n_ci : 1), pgd_box{});
    cx.assign((size_t)(n_ci > 0 ? n_ci : 1), LaneExt{0.f, 0.f, 0.f, -1});
    cs2.assign(cs, cs + n_cs);
    for (int m = 0; m < n_maps; ++m) {
      const pgd_map& M = maps[m];
      const int n_cells = M.gx * M.gy;
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
  }
  return PGD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// scenario tables
// ---------------------------------------------------------------------------------------------------------------------
struct ScenarioTables {
  std::vector<pgd_spawn> spawns;  // the device form of the routes (below)
  bool has_objects;               // some used slot is a traffic object: selects the OBJ kernels
  int no_groups;                  // no scenario has a traffic trigger group
  float uni_len, uni_wid;         // the one body size of every used slot, else 0 (PgdDev::uni_len)
};

// One scan over the n_scen * sstride spawn records.  Unused slots (lane < 0) never enter a world: nothing about them is checked or
// counted.  no_uni: the PGD_NO_UNI switch.
inline int build_scenario_tables(const pgd_scenario* scen, const pgd_spawn* spawns, int n_scen, int sstride, bool no_uni, ScenarioTables& out) {
  if (!scen || n_scen <= 0 || !spawns || sstride <= 0) return PGD_ERR_ARG;
  out.spawns.assign(spawns, spawns + (size_t)n_scen * sstride);
  out.has_objects = false;
  float ul = 0.0f, uw = 0.0f;
  bool uni = true;  // one body size for the whole upload?
  for (pgd_spawn& q : out.spawns) {
    // device-private form of the routes: PGD_CKPT_END from a route's last node on (update_checkpoints: a match on the last node
    // alone changes nothing, navigation.py:270-277 -- the search stops at the mark instead of reading the route length first)
    const int n = q.n_ckpt < 0 ? 0 : (q.n_ckpt > PGD_MAX_CKPT ? PGD_MAX_CKPT : q.n_ckpt);
    for (int k = n > 0 ? n - 1 : 0; k < PGD_MAX_CKPT; ++k) q.ckpt[k] = (int16_t)PGD_CKPT_END;
    if (q.lane < 0) continue;
    if (!(q.max_steer <= 1.0f) || q.n_ckpt > PGD_MAX_CKPT) return PGD_ERR_ARG;  // tan_small
    if (q.kind != PGD_OBJ_VEHICLE) out.has_objects = true;
    if (uni) {
      if (ul == 0.0f) { ul = q.length; uw = q.width; }
      uni = q.length == ul && q.width == uw && ul > 0.0f && uw > 0.0f;
    }
  }
  uni = uni && !out.has_objects && !no_uni;
  out.uni_len = uni ? ul : 0.0f;
  out.uni_wid = uni ? uw : 0.0f;
  out.no_groups = 1;
  for (int k = 0; k < n_scen; ++k)
    if (scen[k].n_groups > 0) { out.no_groups = 0; break; }
  return PGD_OK;
}

// every scenario names one of the n_maps uploaded maps (n_scen == 0: nothing to hold)
inline bool scenario_maps_ok(const pgd_scenario* scen, size_t n_scen, size_t n_maps) {
  for (size_t k = 0; k < n_scen; ++k)
    if (scen[k].map < 0 || (size_t)scen[k].map >= n_maps) return false;
  return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// state conversion: the ABI's field-major blobs ([field][env * V + slot], [field][env]) <-> the device's 128 B record per vehicle
// and its PGD_NEI-int row per env
// ---------------------------------------------------------------------------------------------------------------------
// The float fields that a record stores, each with its member.  SF_THROTTLE is the one ABI field without a member (below).
#define PGD_STATE_FLOATS(F)                                                                                                       \
  F(SF_X, x) F(SF_Y, y) F(SF_THETA, th) F(SF_SPEED, v) F(SF_STEER, steer) F(SF_LASTX, lastx) F(SF_LASTY, lasty) F(SF_LASTHX, lasthx)  \
  F(SF_LASTHY, lasthy) F(SF_ACT0S, a0s) F(SF_ACT0T, a0t) F(SF_ACT1S, a1s) F(SF_ACT1T, a1t) F(SF_PID_HP, php) F(SF_PID_HI, phi)       \
  F(SF_PID_LP, plp) F(SF_PID_LI, pli) F(SF_TARGET_SPEED, target) F(SF_ENERGY, energy) F(SF_DIST_LEFT, dl) F(SF_DIST_RIGHT, dr)      \
  F(SF_EP_REWARD, eprew) F(SF_AGENT_ID, agent_id) F(SF_HX, hx) F(SF_HY, hy)
// The int fields, each with its member and the range pgd_set_state accepts (the width of the member's bit-field; SI_TIMER saturates
// instead: any value >= 0 is taken and clamped at 0xffff)
#define PGD_STATE_INTS(I)                                                                                                          \
  I(SI_STATUS, status, 0, 15) I(SI_LANE, lane, 0, 0xffff) I(SI_CK0, ck0, 0, PGD_MAX_CKPT - 1) I(SI_CK1, ck1, 0, PGD_MAX_CKPT - 1)     \
  I(SI_RLANE, rlane, -1, 0x7fff) I(SI_TIMER, timer, 0, 0x7fffffff) I(SI_VFLAGS, vflags, 0, 0xffff) I(SI_SPAWN, spawn, 0, 0xffff)
#define PGD_COUNT_FIELD(...) +1
static_assert(0 PGD_STATE_FLOATS(PGD_COUNT_FIELD) == PGD_NF - 1, "every float field but SF_THROTTLE has a member");
static_assert(0 PGD_STATE_INTS(PGD_COUNT_FIELD) == PGD_NI, "every int field has a member");
#undef PGD_COUNT_FIELD

// Host copies of the record array are blocks of piece planes like the device's (RecPiece, pgd_device.h): record k = (env k / V, slot
// k % V) out of / into the eight planes of its env's block, in 16-byte units
struct RecUnit { alignas(16) unsigned char b[16]; };
static_assert(sizeof(RecUnit) == 16, "one piece of a record");
inline void record_from_planes(const RecUnit* raw, int V, size_t k, VehRec& t) {
  const RecUnit* blk = raw + (k / (size_t)V) * (size_t)(8 * V);
  for (int p = 0; p < 8; ++p) memcpy(reinterpret_cast<char*>(&t) + 16 * p, blk + (size_t)p * V + k % (size_t)V, 16);
}
inline void record_to_planes(RecUnit* raw, int V, size_t k, const VehRec& t) {
  RecUnit* blk = raw + (k / (size_t)V) * (size_t)(8 * V);
  for (int p = 0; p < 8; ++p) memcpy(blk + (size_t)p * V + k % (size_t)V, reinterpret_cast<const char*>(&t) + 16 * p, 16);
}

// device records and env rows -> ABI fields (pgd_get_state).  rec: N blocks of V records; env: [N][PGD_NEI]
inline void state_to_fields(const RecUnit* rec, const int32_t* env, int N, int V, float* f, int32_t* i, int32_t* ei) {
  const size_t nv = (size_t)N * (size_t)V;
  for (size_t k = 0; k < nv; ++k) {
    VehRec t;
    record_from_planes(rec, V, k, t);
#define PGD_F_OUT(q, m) f[(size_t)(q) * nv + k] = t.m;
#define PGD_I_OUT(q, m, lo, hi) i[(size_t)(q) * nv + k] = (int32_t)t.m;
    PGD_STATE_FLOATS(PGD_F_OUT)
    PGD_STATE_INTS(PGD_I_OUT)
#undef PGD_F_OUT
#undef PGD_I_OUT
    f[(size_t)SF_THROTTLE * nv + k] = t.a1t;  // not stored: the last applied throttle IS the newer entry of the action deque
  }
  for (int e = 0; e < N; ++e)
    for (int q = 0; q < PGD_NEI; ++q) ei[(size_t)q * N + e] = q == EI_NEAR ? 0 : env[(size_t)e * PGD_NEI + q];  // (device-private hints)
}

// ABI fields -> device records and env rows (pgd_set_state); the derived part of a record is rebuilt on the device (k_derive).
// PGD_ERR_ARG: an int field outside its range.
inline int state_from_fields(const float* f, const int32_t* i, const int32_t* ei, int N, int V, RecUnit* rec, int32_t* env) {
  const size_t nv = (size_t)N * (size_t)V;
  for (size_t k = 0; k < nv; ++k) {
    VehRec t;
    memset(&t, 0, sizeof(t));
#define PGD_F_IN(q, m) t.m = f[(size_t)(q) * nv + k];
#define PGD_I_IN(q, m, lo, hi)                              \
    {                                                       \
      const int32_t v = i[(size_t)(q) * nv + k];            \
      if (v < (lo) || v > (hi)) return PGD_ERR_ARG;         \
      t.m = std::min(v, (q) == SI_TIMER ? 0xffff : v);      \
    }
    PGD_STATE_FLOATS(PGD_F_IN)  // (SF_THROTTLE is ignored: SF_ACT1T is what is stored)
    PGD_STATE_INTS(PGD_I_IN)
#undef PGD_F_IN
#undef PGD_I_IN
    {  // the carried heading vector is taken from the checkpoint only while it agrees with THETA (a caller that edits THETA,
       // or builds a state by hand, gets cos / sin of it)
      const double c = cos((double)t.th), sn = sin((double)t.th);
      if (!(fabs((double)t.hx - c) <= 1e-4 && fabs((double)t.hy - sn) <= 1e-4)) { t.hx = (float)c; t.hy = (float)sn; }
    }
    record_to_planes(rec, V, k, t);
  }
  for (int e = 0; e < N; ++e)
    for (int q = 0; q < PGD_NEI; ++q) env[(size_t)e * PGD_NEI + q] = q == EI_NEAR ? 1 : ei[(size_t)q * N + e];  // (hints: "unknown")
  return PGD_OK;
}
