// pgd_timelimit.h -- GAE that bootstraps through a time limit, for single-agent engines: which dones are truncations (tl_truncated), the
// critics' values of the terminal observations of the envs a step truncated (pgd_mlp_terminal_value), and the two GAE kernels with the
// one-step target taken from them (pgd_gae_bootstrap, pgd_cost_gae_bootstrap).  include/pgdrive_hip.h states the formulas.  Part of the
// single translation unit pgd_engine.hip (included at its end, behind pgd_safe.h, whose safe_cost it uses).
// No reference counterpart: the reference returns the terminal observation from env.step (base_env.py:303-344) and `max_step` in its
// info dict (base_env.py:190-192); an RL library evaluates its critic on it on the host.
//
// k_mlp_terminal_value is the critic workgroup of k_mlp_actor_critic -- 16-row tile, 4 waves, ac_lds_bytes, mlp_layer / mlp_store_hidden,
// the sixteen-lane head -- behind the shared row loader with a rule of its own (tl_load_rows: mlp_load_rows with a row mask, as
// k_mlp_actor_critic_rows' ro_load_rows is with a list).  blockIdx.y chooses the critic (0) or the cost critic (1).  A
// workgroup first reads the flags and dones of its 16 rows; every wave forms the same 16-bit mask by ballot (no LDS, no barrier).  A
// tile without a truncated row -- nearly all of them -- writes its zeros and ends before it reads a weight or an observation.  A row's
// arithmetic in the tile does not depend on its neighbours, so a truncated row receives bit for bit the critic half of
// k_mlp_actor_critic on its observation row; rows that are not truncated enter as zeros (their final_obs row is stale or was never
// written) and leave as exactly 0.
#ifndef PGD_TIMELIMIT_H
#define PGD_TIMELIMIT_H

// The done of a single-agent step is a truncation: PGD_F_MAX_STEP (cfg.horizon or the scenario's max_steps) and no cause of reward_done
// (pgd_dynamics.h) in the same step -- with safe_rl_env a step with a vehicle or object crash is not terminal whatever else it holds
DEV bool tl_truncated(const uint32_t f, const bool done, const bool safe_rl_env) {
  bool natural = (f & (PGD_F_ARRIVE | PGD_F_OUT_OF_ROAD | PGD_F_CRASH_VEHICLE | PGD_F_CRASH_OBJECT | PGD_F_CRASH_BUILDING)) != 0u;
  if (safe_rl_env && (f & (PGD_F_CRASH_VEHICLE | PGD_F_CRASH_OBJECT)) != 0u) natural = false;
  return done && (f & PGD_F_MAX_STEP) != 0u && !natural;
}

struct TlNets { pgd_value_net v, c; };

// slot r holds row row0 + r0 + r of `obs` where bit r of `mask` is set; the tile's first row stands in for the others (a row that is not
// truncated is never USED)
template <bool NORM>
DEV void tl_load_rows(const float* obs, const int row0, const int r0, const uint32_t mask, const int obs_stride, const int in_dim, const int kp,
                      const int xs, const int wave, const int lane, float* X, const ObsNorm nm) {
  mlp_load_rows<NORM>(in_dim, kp, xs, wave, lane, X, nm, [&](const int r, bool& in) {
    in = ((mask >> r) & 1u) != 0u;
    return obs + (size_t)(row0 + r0 + (in ? r : 0)) * obs_stride;
  });
}

// rows [row0, row0 + n_rows) of `obs`, `flags`, `done` -> term_value[row] (blockIdx.y == 0) and term_cost_value[row] (blockIdx.y == 1):
// the network's value of a truncated row, 0 for every other
template <bool NORM>
__global__ __launch_bounds__(WAVE * MLP_WAVES, 4) void k_mlp_terminal_value(const float* __restrict__ obs, const int row0, const int n_rows,
                                                                         const int obs_stride, const int in_dim, const TlNets nets,
                                                                         const int safe_rl_env, const uint32_t* __restrict__ flags,
                                                                         const uint8_t* __restrict__ done, float* __restrict__ term_value,
                                                                         float* __restrict__ term_cost_value, const ObsNorm nm) {
  extern __shared__ float mlp_lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = (int)blockIdx.x * MLP_ROWS;  // (relative to row0)
  float* __restrict__ out = blockIdx.y != 0 ? term_cost_value : term_value;
  // every wave reads the tile's 16 flags and dones (lane l: row l & 15) and forms the same mask
  uint32_t mask;
  {
    const int r = lane & 15;
    const bool row_in = r0 + r < n_rows;
    const size_t row = (size_t)(row0 + r0 + (row_in ? r : 0));
    const bool tr = row_in && tl_truncated(flags[row], done[row] != 0, safe_rl_env != 0);
    mask = (uint32_t)__ballot(tr) & 0xffffu;
  }
  if (mask == 0u) {  // (uniform over the workgroup; before any weight or observation is read)
    if (tid < MLP_ROWS && r0 + tid < n_rows) out[(size_t)(row0 + r0 + tid)] = 0.0f;
    return;
  }
  const pgd_value_net& n = blockIdx.y != 0 ? nets.c : nets.v;
  const float* __restrict__ W1 = n.w1;
  const float* __restrict__ b1 = n.b1;
  const float* __restrict__ W2 = n.w2;
  const float* __restrict__ b2 = n.b2;
  const float* __restrict__ W3 = n.w3;
  const float* __restrict__ b3 = n.b3;
  const int kp = (in_dim + 3) & ~3, xs = mlp_x_stride(in_dim);
  float* X = mlp_lds;
  float* H1 = X + MLP_ROWS * xs;
  float* H2 = H1 + MLP_ROWS * MLP_HS;
  float* W3s = H2 + MLP_ROWS * MLP_HS;  // [4][256], the first 256 used
  const float w3v = W3[tid];
  tl_load_rows<NORM>(obs, row0, r0, mask, obs_stride, in_dim, kp, xs, wave, lane, X, nm);
  W3s[tid] = w3v;
  __syncthreads();
  const int c0 = wave * 64;
  mlp_f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = mlp_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  mlp_layer(X, xs, W1, kp, in_dim, lane, c0, acc);
  mlp_store_hidden(H1, b1, lane, c0, acc);
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = mlp_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  mlp_layer(H1, MLP_HS, W2, MLP_H, MLP_H, lane, c0, acc);
  mlp_store_hidden(H2, b2, lane, c0, acc);
  __syncthreads();
  // the critic head of ac_tile: 16 dot products of 256, sixteen lanes each
  const int r = tid >> 4, part = tid & 15;
  float s = 0.0f;
#pragma unroll 4
  for (int k = part; k < MLP_H; k += 16) s = fmaf(H2[r * MLP_HS + k], W3s[k], s);
  s += __shfl_xor(s, 8);
  s += __shfl_xor(s, 4);
  s += __shfl_xor(s, 2);
  s += __shfl_xor(s, 1);
  if (part == 0 && r0 + r < n_rows) out[(size_t)(row0 + r0 + r)] = ((mask >> r) & 1u) ? s + b3[0] : 0.0f;
}

// gae_scan with the one-step target of a done row taken from term_value (0 where the episode terminated): a SELECT, value[t + 1] behind a
// done may hold anything; the trace still ends at every done
template <class RewardOf>
DEV void gae_scan_bootstrap(const RewardOf reward_of, const float* value, const uint8_t* done, const float* term_value, const int T, const int rows,
                            const int r, const float gamma, const float lam, float* adv, float* ret) {
  const float gl = gamma * lam;
  float a = 0.0f, vn = value[(size_t)T * rows + r];
#pragma unroll 4
  for (int t = T - 1; t >= 0; --t) {
    const size_t i = (size_t)t * rows + r;
    const bool dn = done[i] != 0;
    const float v = value[i], tv = term_value[i];
    const float delta = fmaf(gamma, dn ? tv : vn, reward_of(i)) - v;
    a = fmaf(gl, dn ? 0.0f : a, delta);
    adv[i] = a;
    ret[i] = a + v;
    vn = v;
  }
}

// k_gae with that scan
__global__ __launch_bounds__(WAVE) void k_gae_bootstrap(const float* __restrict__ reward, const float* __restrict__ value,
                                                        const uint8_t* __restrict__ done, const float* __restrict__ term_value, const int T,
                                                        const int rows, const float gamma, const float lam, float* __restrict__ adv,
                                                        float* __restrict__ ret) {
  const int r = (int)blockIdx.x * WAVE + (int)threadIdx.x;
  if (r >= rows) return;
  gae_scan_bootstrap([&](const size_t i) { return reward[i]; }, value, done, term_value, T, rows, r, gamma, lam, adv, ret);
}

// k_cost_gae with that scan
__global__ __launch_bounds__(WAVE) void k_cost_gae_bootstrap(const uint32_t* __restrict__ flags, const uint8_t* __restrict__ done,
                                                             const float* __restrict__ value, const float* __restrict__ term_value, const int T,
                                                             const int rows, const float c0, const float c1, const float c2, const float gamma,
                                                             const float lam, float* __restrict__ cost, float* __restrict__ adv,
                                                             float* __restrict__ ret, float* __restrict__ run, float* __restrict__ ep_sum,
                                                             int32_t* __restrict__ ep_count) {
  const int r = (int)blockIdx.x * WAVE + (int)threadIdx.x;
  if (r >= rows) return;
  {  // k_cost_gae's forward pass line for line (the sums in the order of t).  A copy: as one function called by both, both kernels compiled to other code
#pragma clang fp reassociate(off)
    float rn = run[r], es = 0.0f;
    int ec = 0;
#pragma unroll 4
    for (int t = 0; t < T; ++t) {
      const size_t i = (size_t)t * rows + r;
      const float c = safe_cost(flags[i], c0, c1, c2);
      cost[i] = c;
      rn += c;
      if (done[i]) {
        es += rn;
        ec += 1;
        rn = 0.0f;
      }
    }
    run[r] = rn;
    ep_sum[r] = es;
    ep_count[r] = ec;
  }
  gae_scan_bootstrap([&](const size_t i) { return safe_cost(flags[i], c0, c1, c2); }, value, done, term_value, T, rows, r, gamma, lam, adv, ret);
}

static bool value_net_ok(const pgd_value_net* n) {
  return n && six_set(n->w1, n->b1, n->w2, n->b2, n->w3, n->b3) && reads_16(n->w1, n->b1, n->w2, n->b2);
}

extern "C" {

int pgd_mlp_terminal_value(pgd_handle h, int group, const float* d_term_obs, int obs_stride, int in_dim, const pgd_value_net* critic,
                           const pgd_value_net* cost_critic, const uint32_t* d_flags, const uint8_t* d_done, float* d_term_value,
                           float* d_term_cost_value) {
  if (!h || !d_term_obs || !d_flags || !d_done || !d_term_value || !value_net_ok(critic) || (cost_critic && !value_net_ok(cost_critic)) ||
      (cost_critic && !d_term_cost_value) || in_dim < 4 || obs_stride < in_dim || ac_lds_bytes(in_dim) > 65536) return PGD_ERR_ARG;
  if ((((uintptr_t)d_term_obs | (uintptr_t)d_flags | (uintptr_t)d_term_value | (uintptr_t)d_term_cost_value) & 3u) != 0u) return PGD_ERR_ARG;
  if (is_marl(h)) return PGD_ERR_ARG;  // (the cause of a done cannot be read from a multi-agent step's flags alone: pgdrive_hip.h)
  return ac_forward(h, group, LDS_TERM_VALUE, k_mlp_terminal_value<false>, k_mlp_terminal_value<true>, in_dim, [&](const AcRows& r, auto kern) {
    const TlNets tn = {*critic, cost_critic ? *cost_critic : *critic};
    hipLaunchKernelGGL(kern, dim3((r.rows + MLP_ROWS - 1) / MLP_ROWS, cost_critic ? 2 : 1), dim3(WAVE * MLP_WAVES), r.lds, r.stream,
                       d_term_obs, r.row0, r.rows, obs_stride, in_dim, tn, (int)h->d.cfg.safe_rl_env, d_flags, d_done, d_term_value,
                       d_term_cost_value, r.nm);
  });
}

int pgd_gae_bootstrap(pgd_handle h, const float* d_reward, const float* d_value, const uint8_t* d_done, const float* d_term_value, int T, int rows,
                      float gamma, float lam, float* d_adv, float* d_ret) {
  if (!h || !d_reward || !d_value || !d_done || !d_term_value || !d_adv || !d_ret || T < 1 || rows < 1) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_gae_bootstrap, dim3((rows + WAVE - 1) / WAVE), dim3(WAVE), 0, h->stream, d_reward, d_value, d_done, d_term_value, T, rows,
                     gamma, lam, d_adv, d_ret);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

int pgd_cost_gae_bootstrap(pgd_handle h, const uint32_t* d_flags, const uint8_t* d_done, const float* d_cost_value, const float* d_term_cost_value,
                           int T, int rows, const float costs[3], float gamma, float lam, float* d_cost, float* d_cadv, float* d_cret,
                           float* d_run, float* d_ep_sum, int32_t* d_ep_count) {
  if (!h || !d_flags || !d_done || !d_cost_value || !d_term_cost_value || !costs || !d_cost || !d_cadv || !d_cret || !d_run || !d_ep_sum ||
      !d_ep_count || T < 1 || rows < 1) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_cost_gae_bootstrap, dim3((rows + WAVE - 1) / WAVE), dim3(WAVE), 0, h->stream, d_flags, d_done, d_cost_value,
                     d_term_cost_value, T, rows, costs[0], costs[1], costs[2], gamma, lam, d_cost, d_cadv, d_cret, d_run, d_ep_sum, d_ep_count);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

}  // extern "C"

#endif
