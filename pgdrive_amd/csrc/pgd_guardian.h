// pgd_guardian.h -- the expert guardian of a single-agent engine (`use_saver` / `save_level`): one launch between the evaluation of the
// acting policy and the step.  include/pgdrive_hip.h states the rule.  Part of the single translation unit pgd_engine.hip (included at
// its end, behind pgd_timelimit.h).
//
// What it mirrors: pgdrive/policy/AI_protect_policy.py:8-59.  A second policy -- the PPO expert of examples/ppo_expert -- is evaluated on
// the observation the acting policy saw; where the car is about to leave the road or to hit something its action replaces the agent's,
// and the step info says so (takeover_start / takeover_end / takeover; agent_manager.py:187).
//
// k_guardian is the actor workgroup of k_mlp_actor_critic -- 16-row tile, 4 waves, ac_lds_bytes, mlp_layer / mlp_store_hidden, the
// four-lane head and its noise (ac_noise) -- between a prologue and a tail of its own (the rows come through ac_load_rows or, LEGACY, a
// loader of its own):
//   prologue  the sixteen lanes that share a row in the head (r = tid >> 4) read the row's engine state at the same addresses (one
//             transaction per row): the ego's record pieces 0 .. 2 (pose, speed, heading vector, lane | spawn), the env's scenario id
//             and map header, the agent's action, the previous flags and the takeover state; behind them the lane record and the spawn
//             record's max_speed.  All of it goes out in front of the observation rows' reads, nothing of it behind the head.
//             LEGACY (PGD_GUARD_LEGACY_LATERAL): the expert's row is obs[0..7] | lateral | obs[8..] -- gd_load_rows shifts the columns,
//             lane 0 of the row writes column 8.  A bound observation-normalisation table is never applied: the expert saw raw rows.
//   tail      lidar minima of the row from the X tile (forty floats over sixteen lanes, a butterfly minimum), then the rule on the
//             vector ALU, fp32, no contraction or re-association (gd_rule).
// A row's arithmetic in the tile does not depend on its neighbours, so the expert's action is bit for bit what k_mlp_actor_critic
// writes for the same row, seed and tick.
#ifndef PGD_GUARDIAN_H
#define PGD_GUARDIAN_H

struct GdArgs {
  const float* agent;        // [rows][2]
  const uint32_t* prev;      // [rows] or null
  uint8_t* state;            // [rows], in / out
  float* applied;            // [rows][2]; may be `agent`
  uint8_t* info;             // [rows]
  float* trace;              // [rows][4] or null
  float s, ten_s, side_thr;  // save_level, 10 s and (s + 0.1) / 10, the latter two rounded once from double (host)
  int regime;                // 0: s <= 1e-3, 1: the rule, 2: s > 0.9
  int D, n;                  // row width and beam count of the engine
  uint32_t mode;
};

// ac_load_rows<false> for the expert's row: X column c holds obs[c] below column 8, obs[c - 1] above it; column 8 is left to the row's
// rule lane.  Padding columns and rows past the end read zero.
DEV void gd_load_rows_legacy(const float* obs, const int row0, const int r0, const int n_rows, const int obs_stride, const int in_dim,
                             const int kp, const int xs, const int wave, const int lane, float* X) {
  constexpr int XCH = 5;
  if (kp <= WAVE * XCH) {
    float v[MLP_ROWS / MLP_WAVES][XCH];
#pragma unroll
    for (int i = 0; i < MLP_ROWS / MLP_WAVES; ++i) {
      const int r = wave + i * MLP_WAVES;
      const bool row_in = r0 + r < n_rows;
      const float* src = obs + (size_t)(row0 + r0 + (row_in ? r : 0)) * obs_stride;
#pragma unroll
      for (int j = 0; j < XCH; ++j) {
        const int k = lane + WAVE * j, kk = k < in_dim ? k : in_dim - 1;
        v[i][j] = src[kk < 8 ? kk : kk - 1];
        if (!(row_in && k < in_dim)) v[i][j] = 0.0f;
      }
    }
#pragma unroll
    for (int i = 0; i < MLP_ROWS / MLP_WAVES; ++i)
#pragma unroll
      for (int j = 0; j < XCH; ++j) {
        const int k = lane + WAVE * j;
        if (k < kp && k != 8) X[(wave + i * MLP_WAVES) * xs + k] = v[i][j];
      }
  } else
  for (int r = wave; r < MLP_ROWS; r += MLP_WAVES) {
    const bool row_in = r0 + r < n_rows;
    const float* src = obs + (size_t)(row0 + r0 + (row_in ? r : 0)) * obs_stride;
    for (int k = lane; k < kp; k += WAVE)
      if (k != 8) X[r * xs + k] = (row_in && k < in_dim) ? src[k < 8 ? k : k - 1] : 0.0f;
  }
}

// float 8 of the reference expert's row (state_obs.py:97-100, commented out upstream after the weights were trained):
// clip((lat * 2 / 4.5 + 1) / 2, 0, 1), lat = the lateral coordinate of the vehicle on its current lane
DEV float gd_lateral(const float lat) {
#pragma clang fp contract(off) reassociate(off)
  const float a = lat * 2.0f;
  const float b = a * (1.0f / 4.5f);  // (a constant factor: the build's `/` is rcp * x)
  const float c = b + 1.0f;
  return clipf(c * 0.5f, 0.0f, 1.0f);
}

// f = min(1 + |hd| * v * max_speed, 10 s), the product from left to right
DEV float gd_factor(const float hd, const float v, const float ms, const float ten_s) {
#pragma clang fp contract(off) reassociate(off)
  const float p = fabsf(hd) * v;
  const float q = p * ms;
  return fminf(1.0f + q, ten_s);
}

// AI_protect_policy.py:24-49: the corrected (steering, throttle) of one row
DEV float2 gd_rule(const GdArgs& g, const float a0, const float a1, const float e0, const float e1, const float hd, const float v,
                   const float f, const float obs0, const float obs1, const float side_min, const float front_min) {
#pragma clang fp contract(off) reassociate(off)
  float steer = a0, thr = a1;
  if (g.regime == 2) {
    steer = e0;
    thr = e1;
  } else if (g.regime == 1) {
    const float edge = 0.04f * f;
    if ((obs0 < edge && hd < 0.0f) || (obs1 < edge && hd > 0.0f) || obs0 <= 1e-3f || obs1 <= 1e-3f) {
      steer = e0;
      thr = v < 5.0f ? 0.5f : e1;
    }
    if (side_min < g.side_thr) steer = e0;
    if (a1 >= 0.0f && e1 <= 0.0f && front_min < g.s) thr = e1;
  }
  return make_float2(steer, thr);
}

// rows [row0, row0 + n_rows) = envs of a single-agent engine.  Two workgroups per CU, not ac_tile's four: the row's state (action, hd, v, f,
// the lateral float, the flags) stays in registers across the three layers, and under the 128-register cap of four workgroups the compiler
// spilled 3 to 8 of them to scratch.  At the widths the guardian is launched with the LDS admits two workgroups per CU anyway (55.7 KB
// each at 274 inputs), and 4096 rows are one workgroup per CU.
template <bool LEGACY>
__global__ __launch_bounds__(WAVE * MLP_WAVES, 2) void k_guardian(const PgdDev d, const float* __restrict__ obs, const int row0, const int n_rows,
                                                               const int obs_stride, const int in_dim, const pgd_actor_critic nets,
                                                               const uint32_t seed, const uint32_t tick_arg,
                                                               const uint32_t* __restrict__ tick_dev, const uint32_t row_base, const GdArgs g) {
  extern __shared__ float mlp_lds[];
  const int kp = (in_dim + 3) & ~3, xs = mlp_x_stride(in_dim);
  float* X = mlp_lds;
  float* H1 = X + MLP_ROWS * xs;
  float* H2 = H1 + MLP_ROWS * MLP_HS;
  float* W3s = H2 + MLP_ROWS * MLP_HS;  // [4][256]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = (int)blockIdx.x * MLP_ROWS;  // (relative to row0)
  // the head's row of this thread and its state: sixteen lanes per row, the same addresses
  const int r = tid >> 4;
  const bool row_in = r0 + r < n_rows;
  const int env = row0 + r0 + (row_in ? r : 0);
  const RecPiece* blk = rec_block(d.rec, (size_t)env, d.V);
  const uint4 p0 = blk[0 * d.V].q, p1 = blk[1 * d.V].q, p2 = blk[2 * d.V].q;  // slot 0
  int scen = d.ei[(size_t)env * PGD_NEI + EI_SCEN];
  const int lane_off = d.env_map[env].lane_off, n_lanes = d.env_map[env].n_lanes;
  const float2 a = *reinterpret_cast<const float2*>(g.agent + (size_t)env * 2);
  const uint32_t pf = g.prev ? g.prev[env] : 0u;
  const uint8_t st = g.state[env];
  float w3v[AC_HEAD];
#pragma unroll
  for (int q = 0; q < AC_HEAD; ++q) {
    const int idx = tid + q * WAVE * MLP_WAVES;
    w3v[q] = nets.w3[(size_t)(idx >> 2) * nets.out_cols + (idx & 3)];
  }
  // behind the first flight: the lane record and the spawn record (indices clamped: a state set by hand may hold anything)
  const float px = __uint_as_float(p0.x), py = __uint_as_float(p0.y), spd = __uint_as_float(p0.w);
  const float hx = __uint_as_float(p1.x), hy = __uint_as_float(p1.y);
  int vl = (int)(p2.x & 0xffffu), vs = (int)(p2.x >> 16);
  vl = min(vl, max(n_lanes, 1) - 1);
  vs = min(vs, d.sstride - 1);
  scen = min(max(scen, 0), d.n_scen - 1);
  const pgd_lane ln = d.lanes()[(size_t)lane_off + vl];
  const float ms = d.spawns()[(size_t)scen * d.sstride + vs].max_speed;
  if (LEGACY) gd_load_rows_legacy(obs, row0, r0, n_rows, obs_stride, in_dim, kp, xs, wave, lane, X);
  else ac_load_rows<false>(obs, row0, r0, n_rows, obs_stride, in_dim, kp, xs, wave, lane, X, ObsNorm{nullptr, 0.0f});
#pragma unroll
  for (int q = 0; q < AC_HEAD; ++q) {
    const int idx = tid + q * WAVE * MLP_WAVES;
    W3s[(idx & 3) * MLP_H + (idx >> 2)] = w3v[q];
  }
  float lateral = 0.0f;
  if (LEGACY) {
    float lon, lat;
    lane_local(ln, px, py, lon, lat);
    lateral = gd_lateral(lat);
    if ((lane & 15) == 0) X[r * xs + 8] = row_in ? lateral : 0.0f;
  }
  const float hd = heading_diff(ln, px, py, hx, hy) - 0.5f;
  const float v = speed_kmh(spd);
  const float f = gd_factor(hd, v, ms, g.ten_s);
  __syncthreads();
  const int c0 = wave * 64;
  mlp_f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = mlp_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  mlp_layer(X, xs, nets.w1, kp, in_dim, lane, c0, acc);
  mlp_store_hidden(H1, nets.b1, lane, c0, acc);
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = mlp_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  mlp_layer(H1, MLP_HS, nets.w2, MLP_H, MLP_H, lane, c0, acc);
  mlp_store_hidden(H2, nets.b2, lane, c0, acc);
  __syncthreads();
  // the actor head of ac_tile: 16 rows x 4 outputs = 64 dot products of 256, four lanes each
  const int o = (tid >> 2) & 3, part = tid & 3;
  float s = 0.0f;
#pragma unroll 4
  for (int k = part; k < MLP_H; k += 4) s = fmaf(H2[r * MLP_HS + k], W3s[o * MLP_H + k], s);
  s += __shfl_xor(s, 2);
  s += __shfl_xor(s, 1);
  const float hv = s + nets.b3[o];
  const int l0 = lane & ~15;
  const float m0 = __shfl(hv, l0), m1 = __shfl(hv, l0 + 4), ls0 = __shfl(hv, l0 + 8), ls1 = __shfl(hv, l0 + 12);
  // the fan's minima: forty floats of the row's X tile over its sixteen lanes -- beams [L - 4, L + 5] and [R - 4, R + 5] (side), [0, 9]
  // and [n - 10, n - 1] (front); L = n / 4, R = 3 n / 4
  float side_min = INFINITY, front_min = INFINITY;
  {
    const int n = g.n, L = n / 4, R = (3 * n) / 4, fan0 = g.D - n, p = lane & 15;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int i = p + 16 * j;
      if (i < 40) {
        const int beam = i < 10 ? L - 4 + i : (i < 20 ? R - 14 + i : (i < 30 ? i - 20 : n - 40 + i));
        const int col = fan0 + beam;
        const float x = X[r * xs + col + ((LEGACY && col >= 8) ? 1 : 0)];
        if (i < 20) side_min = fminf(side_min, x);
        else front_min = fminf(front_min, x);
      }
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
      side_min = fminf(side_min, __shfl_xor(side_min, m));
      front_min = fminf(front_min, __shfl_xor(front_min, m));
    }
  }
  if ((lane & 15) == 0 && row_in) {
    float z0 = 0.0f, z1 = 0.0f;
    if (!(g.mode & PGD_GUARD_DETERMINISTIC)) ac_noise(seed, tick_arg + (tick_dev ? *tick_dev : 0u), row_base + (uint32_t)env, z0, z1);
    const float e0 = fmaf(expf(ls0), z0, m0), e1 = fmaf(expf(ls1), z1, m1);
    const float obs0 = X[r * xs + 0], obs1 = X[r * xs + 1];
    const float2 c = gd_rule(g, a.x, a.y, e0, e1, hd, v, f, obs0, obs1, side_min, front_min);
    const bool pre = (pf & PGD_F_RESET) ? false : st != 0;  // the vehicle was reset: base_vehicle.py:332
    const bool now = a.x != c.x || a.y != c.y;
    const bool takeover = pre && now;
    const bool apply = (g.mode & PGD_GUARD_IMMEDIATE) ? now : takeover;
    g.state[env] = now ? 1 : 0;
    g.info[env] = (uint8_t)((takeover ? 1 : 0) | ((!pre && now) ? 2 : 0) | ((pre && !now) ? 4 : 0));
    *reinterpret_cast<float2*>(g.applied + (size_t)env * 2) = apply ? c : a;
    if (g.trace) *reinterpret_cast<float4*>(g.trace + (size_t)env * 4) = make_float4(e0, e1, LEGACY ? lateral : 0.0f, f);
  }
}

extern "C" {

int pgd_guardian(pgd_handle h, int group, const float* d_obs, int obs_stride, const pgd_actor_critic* expert, const pgd_guardian_config* cfg,
                 const float* d_agent_actions, const uint32_t* d_prev_flags, uint8_t* d_state, float* d_applied, uint8_t* d_info,
                 float* d_trace) {
  bool critic;
  if (!h || !d_obs || !cfg || !d_agent_actions || !d_state || !d_applied || !d_info) return PGD_ERR_ARG;
  if ((cfg->mode & ~(PGD_GUARD_LEGACY_LATERAL | PGD_GUARD_DETERMINISTIC | PGD_GUARD_IMMEDIATE)) != 0u || !(cfg->save_level == cfg->save_level))
    return PGD_ERR_ARG;
  const bool legacy = (cfg->mode & PGD_GUARD_LEGACY_LATERAL) != 0u;
  const int in_dim = cfg->expert_in_dim, D = h->d.D, n = h->d.cfg.num_lasers;
  if (is_marl(h) || h->d.A != 1 || n < 40 || in_dim != D + (legacy ? 1 : 0) || obs_stride < D) return PGD_ERR_ARG;
  if (!nets_ok(expert, nullptr, true, in_dim, in_dim, &critic) || critic || ac_lds_bytes(in_dim) > 65536) return PGD_ERR_ARG;
  if ((((uintptr_t)d_obs | (uintptr_t)d_prev_flags) & 3u) != 0u || (((uintptr_t)d_agent_actions | (uintptr_t)d_applied) & 7u) != 0u ||
      ((uintptr_t)d_trace & 15u) != 0u) return PGD_ERR_ARG;
  if (!h->have_maps || !h->have_scen) return PGD_ERR_STATE;
  HIPCHK(hipSetDevice(h->device));
  EnvGroup eg;
  { int rc = env_group(h, group, eg); if (rc) return rc; }
  const size_t lds = ac_lds_bytes(in_dim);
  const void* kern = legacy ? reinterpret_cast<const void*>(k_guardian<true>) : reinterpret_cast<const void*>(k_guardian<false>);
  { int rc = raise_lds_limit(h, legacy ? LDS_GUARD_LEGACY : LDS_GUARD, kern, lds); if (rc) return rc; }
  const double s = (double)cfg->save_level;
  const GdArgs g = {d_agent_actions, d_prev_flags, d_state, d_applied, d_info, d_trace, cfg->save_level, (float)(10.0 * s), (float)((s + 0.1) / 10.0),
                    s > 0.9 ? 2 : (s > 1e-3 ? 1 : 0), D, n, cfg->mode};
  const dim3 grid((eg.count + MLP_ROWS - 1) / MLP_ROWS), block(WAVE * MLP_WAVES);
  const uint32_t row_base = (uint32_t)h->d.cfg.env_base;
  if (legacy)
    hipLaunchKernelGGL(k_guardian<true>, grid, block, lds, eg.stream, h->d, d_obs, eg.first, eg.count, obs_stride, in_dim, *expert, cfg->seed,
                       cfg->tick, h->ac_tick, row_base, g);
  else
    hipLaunchKernelGGL(k_guardian<false>, grid, block, lds, eg.stream, h->d, d_obs, eg.first, eg.count, obs_stride, in_dim, *expert, cfg->seed,
                       cfg->tick, h->ac_tick, row_base, g);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

}  // extern "C"

#endif
