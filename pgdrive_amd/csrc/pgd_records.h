// pgd_records.h -- the plain records and constants that the device code and the host preparation (pgd_host_prep.h) share.  Includes no HIP
// header: a plain host C++17 compiler takes it, which is how the tests reach the host preparation without a GPU (tests/host_prep_main.cpp).
// pgd_device.h includes it first; pgd_step.h and pgd_vehicle.h find their constants here.
#pragma once
#include <stdint.h>

#include "../../include/pgd_state_layout.h"
#include "../../include/pgdrive_hip.h"

#define WAVE 64
#define MAXV 64
#define FUSE_MAX_AGENTS 8
#ifndef PGD_SUBV
#define PGD_SUBV 52  // slots of a wave with sub-step poses (the largest shipped env: 40 agents + 8 toll booths; three packed
                     // envs of 17 slots); waves with more slots test contacts at the end pose only
#endif
// the mark in the route of a device spawn record, from the route's last node on (build_scenario_tables writes it, update_checkpoints
// in pgd_localize.h stops at it)
#define PGD_CKPT_END (-32768)

// Device-side vehicle record = the per-lane register image of a vehicle (device-private; pgd_get_state / pgd_set_state
// convert to the ABI's field-major blobs).  128 B = eight 16-byte pieces: a lane loads / stores its vehicle with 8 dwordx4
// transactions and no field shuffling -- the struct in registers IS the record; in memory its pieces lie in the planes of its
// block (RecPiece in pgd_device.h).
// Besides the ABI fields of include/pgd_state_layout.h (SF_THROTTLE is not stored: the last applied throttle always equals
// the newer entry of the action deque, SF_ACT1T; base_vehicle.py:343-349 sets both from the same action) the line carries
// state DERIVED from them, kept from step to step instead of being recomputed through dependent table reads every step:
//   hx, hy     unit heading vector (cos, sin of th) -- no sincosf per vehicle and step
//   lon        longitudinal coordinate of the vehicle on its own lane (what the IDM neighbour search reads)
//   road_cur.. route context (Navigation.current_ref_lanes / next_ref_lanes, navigation.py:155-183): road ids, first lanes
//              and lane counts of the current and the next checkpoint pair, block id of the current road; changes only
//              when a checkpoint is passed (route_refresh)
// The int fields are bit-fields: 15 ints live in 6 registers and the compiler extracts them with v_bfe where they are used.
struct __attribute__((aligned(16))) Veh {
  float x, y, th, v;                  // position, heading_theta [rad], speed [m/s]
  float hx, hy, lon, steer;
  uint32_t lane : 16, spawn : 16;
  int32_t rlane : 16;                 // traffic: routing target lane (-1 = None); agents: episode length
  uint32_t timer : 16;                // saturating
  uint32_t vflags : 16, status : 4, ck0 : 6, ck1 : 6;
  uint32_t road_cur : 12, road_next : 12, blk : 8;  // road ids (0xfff = none), Road.block_ID char
  uint32_t cur_first : 16, next_first : 16;
  uint32_t cur_n : 8, next_n : 8, spare : 16;
  float target, agent_id;
  float php, phi, plp, pli;           // IDM PIDs; agents: toll / parking bookkeeping (pgd_state_layout.h)
  float lastx, lasty, lasthx, lasthy;
  float a0s, a0t, a1s, a1t;
  float energy, dl, dr, eprew;
};
typedef Veh VehRec;
static_assert(sizeof(Veh) == 128, "vehicle record must be exactly one 128-byte line");

// Per lane-box extract of its lane (device-private, built on upload): the heading test and the road preference of
// ray_localization (scene_utils.py:158-172, navigation.py:328-344) then need no dependent read of the 64-byte lane record.
struct __attribute__((aligned(16))) LaneExt {
  float ax, ay;  // straight lane: unit direction; arc: centre
  float dir;     // 0 = straight, +-1 = CircularLane.direction
  int32_t road;  // map-local road id of the lane
};

// Per lane, device-private, built on upload: what the navigation block of the observation needs from a reference lane
// (Navigation._get_info_for_checkpoint, navigation.py:213-260).  The check point lane.position(length, lateral) is
// end + lateral * normal for both lane types, so the kernel evaluates no sincos and reads 32 instead of 64 bytes.
struct __attribute__((aligned(16))) LaneNav {
  float ex, ey;   // lane.position(length, 0)
  float nx, ny;   // d position / d lateral at the lane end
  float radius;   // CircularLane.radius (0 on straight lanes)
  float dir;      // 0 = straight, +-1 = CircularLane.direction
  float angle;    // end_phase - start_phase (dir = 1) or start_phase - end_phase (dir = -1), radians
  float pad;
};
