// pgd_safe.h -- the cost side of the training loop for the safe env (safe_rl_env: a crash is a cost, not a termination): a cost critic
// beside actor and critic in the rollout's one launch per step (pgd_mlp_actor_critic_cost), the costs of a rollout from its flags with
// their GAE and the episode-cost bookkeeping (pgd_cost_gae), the Lagrange multiplier in device memory (pgd_lagrange), the advantage the
// policy sees (pgd_adv_mix) and the gradients of all three networks for one minibatch (pgd_ppo_grad_cost): PPO-Lagrangian.
// include/pgdrive_hip.h states the formulas.  Part of the single translation unit pgd_engine.hip (included at its end, behind pgd_ppo.h).
// No reference counterpart: the reference hands info["cost"] to an RL library; safe_pgdrive_env.py:7-60.
//
// The network kernels are those of pgd_actor_critic.h and pgd_ppo.h with a third value of blockIdx.y: ac_tile, ppo_rows_tile,
// ppo_reduce_entry and ppo_stats_block are the bodies of k_mlp_actor_critic, k_ppo_rows, k_ppo_reduce and k_ppo_stats, which choose
// their network from pgd_actor_critic and call them; the kernels here choose among three and call the same bodies, so network y of a
// three-network launch computes what network min(y, 1) of a two-network launch computes on the same weights: bit for bit.  k_ppo_wgrad
// takes its network count from its grid and k_ppo_zero_head knows no network: both are launched as they are.
// LDS: a workgroup still holds ONE network's tile (ac_lds_bytes, ppo_lds_bytes): the third network is more workgroups, not more LDS, and
// the limits on in_dim are the two-network ones.
//
// Scratch of pgd_ppo_grad_cost: ppo_work(in_dim, rows, 3).  The cost critic's two tile sums (L_c, dv_c) take slots 11 and 12 of the
// tile's record of PPO_TS = 16 floats, which pgd_ppo_grad leaves unused: the two slots the cost critic needs cost no further bytes.
//
// pgd_adv_mix centres the cost advantage and does NOT rescale it: its scale is the cost's magnitude, which the multiplier is there to
// price -- a cost advantage normalised to unit variance would make lambda's unit arbitrary.
//
// pgd_lagrange sums in the order of k_adv_stats (thread i takes rows i, i + 256, ...; a butterfly per wave; the four waves in order), the
// episode costs in DOUBLE (every fp32 term is exact in it) and the counts as integers: lambda and J_c are single roundings of double
// results whatever the number of rows.
#ifndef PGD_SAFE_H
#define PGD_SAFE_H

struct SafeNets { pgd_actor_critic ac; pgd_value_net c; };
struct SafeGrads { pgd_ppo_grads g; pgd_value_grads c; };

// ---- pgd_mlp_actor_critic_cost: k_mlp_actor_critic with grid.y = 3; workgroup (x, 2) is a critic workgroup on the cost network -------
template <bool NORM>
__global__ __launch_bounds__(WAVE * MLP_WAVES, 4) void k_mlp_actor_critic_cost(const float* __restrict__ obs, const int row0, const int n_rows,
                                                                            const int obs_stride, const int in_dim, const SafeNets nets,
                                                                            const uint32_t seed, const uint32_t tick_arg,
                                                                            const uint32_t* __restrict__ tick_dev, const uint32_t row_base,
                                                                            const uint32_t flags, float* __restrict__ act,
                                                                            float* __restrict__ logp, float* __restrict__ value,
                                                                            float* __restrict__ cost_value, const ObsNorm nm) {
  const int y = (int)blockIdx.y;
  const pgd_actor_critic& a = nets.ac;
  const pgd_value_net& c = nets.c;
  ac_tile<NORM>(obs, row0, n_rows, obs_stride, in_dim, y != 0, y == 0 ? a.w1 : (y == 1 ? a.vw1 : c.w1), y == 0 ? a.b1 : (y == 1 ? a.vb1 : c.b1),
          y == 0 ? a.w2 : (y == 1 ? a.vw2 : c.w2), y == 0 ? a.b2 : (y == 1 ? a.vb2 : c.b2), y == 0 ? a.w3 : (y == 1 ? a.vw3 : c.w3),
          y == 0 ? a.b3 : (y == 1 ? a.vb3 : c.b3), a.out_cols, seed, tick_arg, tick_dev, row_base, flags, act, logp, y == 2 ? cost_value : value, nm);
}

// ---- pgd_cost_gae ---------------------------------------------------------------------------------------------------------------------
// the precedence of k_step_info and of PGDriveEnv.cost_function: a selection of the three floats
DEV float safe_cost(const uint32_t fl, const float c0, const float c1, const float c2) {
  return (fl & PGD_F_OUT_OF_ROAD) ? c0 : (fl & PGD_F_CRASH_VEHICLE) ? c1 : (fl & PGD_F_CRASH_OBJECT) ? c2 : 0.0f;
}

// one thread per row: forward over t (costs out, the running episode cost, this rollout's finished episodes), then k_gae's reverse scan
// (gae_scan) with the cost as reward
__global__ __launch_bounds__(WAVE) void k_cost_gae(const uint32_t* __restrict__ flags, const uint8_t* __restrict__ done,
                                                   const float* __restrict__ value, const int T, const int rows, const float c0, const float c1,
                                                   const float c2, const float gamma, const float lam, float* __restrict__ cost,
                                                   float* __restrict__ adv, float* __restrict__ ret, float* __restrict__ run,
                                                   float* __restrict__ ep_sum, int32_t* __restrict__ ep_count) {
  const int r = (int)blockIdx.x * WAVE + (int)threadIdx.x;
  if (r >= rows) return;
  {  // (the sums in the order of t: the library's build re-associates fp32 sums elsewhere)
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
  gae_scan([&](const size_t i) { return safe_cost(flags[i], c0, c1, c2); }, value, done, T, rows, r, gamma, lam, adv, ret);
}

// ---- pgd_lagrange: ONE workgroup ------------------------------------------------------------------------------------------------------
// ppo_block_sum's order in double, and for the integer counts
template <class V>
DEV V safe_block_sum(V v, V* wave_sum) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
  if ((threadIdx.x & (WAVE - 1)) == 0) wave_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

__global__ __launch_bounds__(256) void k_lagrange(const float* __restrict__ ep_sum, const int32_t* __restrict__ ep_count, const int rows,
                                                  const float cost_limit, const float lr, const float lambda_max, float* __restrict__ state) {
#pragma clang fp reassociate(off)
  __shared__ double wave_sum[4];
  __shared__ long long wave_count[4];
  double s = 0.0;
  long long e = 0;
  for (int q0 = threadIdx.x; q0 < rows; q0 += 256 * PPO_BATCH) {
    float x[PPO_BATCH];
    int32_t k[PPO_BATCH];
#pragma unroll
    for (int j = 0; j < PPO_BATCH; ++j) {
      const int q = q0 + 256 * j;
      x[j] = q < rows ? ep_sum[q] : 0.0f;
      k[j] = q < rows ? ep_count[q] : 0;
    }
#pragma unroll
    for (int j = 0; j < PPO_BATCH; ++j) {
      s += (double)x[j];
      e += k[j];
    }
  }
  s = safe_block_sum(s, wave_sum);
  e = safe_block_sum(e, wave_count);
  if (threadIdx.x == 0 && e > 0) {
    const double jc = s / (double)e;
    double l = (double)state[0] + (double)lr * (jc - (double)cost_limit);
    l = l > 0.0 ? l : 0.0;  // (a NaN step falls to 0)
    l = l < (double)lambda_max ? l : (double)lambda_max;
    state[0] = (float)l;
    state[1] = (float)jc;
    state[2] = (float)e;
  }
}

// ---- pgd_adv_mix: out = ((adv - m) s - lambda (cadv - m_c)) / (1 + lambda), per entry in double, rounded once ---------------------------
__global__ __launch_bounds__(256) void k_adv_mix(const float* __restrict__ adv, const float* __restrict__ cadv, const int n,
                                                 const float* __restrict__ adv_stats, const float* __restrict__ cadv_stats,
                                                 const float* __restrict__ state, float* __restrict__ out) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= n) return;
  const double m = adv_stats ? (double)adv_stats[0] : 0.0, s = adv_stats ? (double)adv_stats[1] : 1.0;
  const double mc = cadv_stats ? (double)cadv_stats[0] : 0.0, l = (double)state[0];
  out[i] = (float)((((double)adv[i] - m) * s - l * ((double)cadv[i] - mc)) / (1.0 + l));
}

// ---- pgd_ppo_grad_cost: pgd_ppo_grad's launches with three networks ---------------------------------------------------------------------
__global__ __launch_bounds__(MLP_H) void k_ppo_prep_cost(const SafeNets nets, float* __restrict__ work) {
  const int y = (int)blockIdx.y;
  const float* __restrict__ W2 = y == 0 ? nets.ac.w2 : (y == 1 ? nets.ac.vw2 : nets.c.w2);
  float* __restrict__ W2T = work + (size_t)y * MLP_H * MLP_H;  // (PpoWork::w2t is 0)
  const int k = blockIdx.x, c = threadIdx.x;
  W2T[(size_t)k * MLP_H + c] = W2[(size_t)c * MLP_H + k];
}

template <bool NORM>
__global__ __launch_bounds__(WAVE * MLP_WAVES, 4) void k_ppo_rows_cost(const SafeNets nets, const pgd_ppo_batch b, const pgd_ppo_hyper hp,
                                                                    const pgd_ppo_cost cost, float* __restrict__ work, const ObsNorm nm) {
  const int y = (int)blockIdx.y;
  const pgd_actor_critic& a = nets.ac;
  const pgd_value_net& c = nets.c;
  ppo_rows_tile<NORM>(y != 0, y == 0 ? a.w1 : (y == 1 ? a.vw1 : c.w1), y == 0 ? a.b1 : (y == 1 ? a.vb1 : c.b1), y == 0 ? a.w2 : (y == 1 ? a.vw2 : c.w2),
                y == 0 ? a.b2 : (y == 1 ? a.vb2 : c.b2), y == 0 ? a.w3 : (y == 1 ? a.vw3 : c.w3), y == 0 ? a.b3 : (y == 1 ? a.vb3 : c.b3),
                a.out_cols, y == 2 ? cost.cost_ret : b.ret, y == 2 ? cost.cvf_coef : hp.vf_coef, y == 2 ? 2 : 0, b, hp, work, nm);
}

__global__ __launch_bounds__(MLP_H) void k_ppo_reduce_cost(const pgd_ppo_batch b, const SafeGrads gr, const int out_cols,
                                                           const float* __restrict__ work) {
  const int y = (int)blockIdx.y;
  const pgd_ppo_grads& g = gr.g;
  const pgd_value_grads& c = gr.c;
  ppo_reduce_entry<4, PPO_TS>(b, y != 0, y == 0 ? g.w1 : (y == 1 ? g.vw1 : c.w1), y == 0 ? g.b1 : (y == 1 ? g.vb1 : c.b1),
                              y == 0 ? g.w2 : (y == 1 ? g.vw2 : c.w2), y == 0 ? g.b2 : (y == 1 ? g.vb2 : c.b2),
                              y == 0 ? g.w3 : (y == 1 ? g.vw3 : c.w3), out_cols, 4, work);
}

__global__ __launch_bounds__(256) void k_ppo_stats_cost(const pgd_ppo_batch b, const pgd_ppo_grads gr, float* __restrict__ cost_b3,
                                                        const float* __restrict__ work, float* __restrict__ stats) {
  ppo_stats_block(b, gr, 1, cost_b3, work, stats);
}

// ---- what every pgd_ppo_grad* call shares on the host: the argument check, the scratch's plan and the observation binding ---------------
// Checked before any HIP call: the pointers, the networks and their gradient buffers (nets_ok, grads_ok), the minibatch rule, the LDS of
// the rows kernel (`lds`) and the scratch (`work_of`: ppo_work, or the categorical head's ppo_cat_work).  reads_action: the call reads
// batch->action (the Gaussian head; the categorical head reads its index array instead).  The binding of the family (pgd_obs_norm_bind)
// is resolved here for every entry point: `bound` chooses the NORM instantiations of the two launches that read observation rows.
struct PpoPlan { bool critic, bound; int n_nets, out_cols; PpoWork wk; ObsNorm nm; };
static int ppo_grad_plan(pgd_handle h, const pgd_actor_critic* nets, const pgd_value_net* cost_net, const pgd_ppo_batch* batch, bool reads_action,
                         const pgd_ppo_cost* cost, const pgd_ppo_hyper* hyper, const pgd_ppo_grads* grads, const pgd_value_grads* cost_grads,
                         const float* d_stats, const void* d_work, size_t work_bytes, size_t lds, PpoWork (*work_of)(int, int, int), PpoPlan& p) {
  if (!h || !batch || !hyper || !d_stats || !d_work || (reinterpret_cast<uintptr_t>(d_work) & 15u) != 0u) return PGD_ERR_ARG;
  const pgd_ppo_batch& b = *batch;
  if (!nets_ok(nets, cost_net, !cost_net, b.in_dim, b.obs_stride, &p.critic) || !grads_ok(grads, cost_grads, p.critic)) return PGD_ERR_ARG;
  if (!b.obs || (reads_action && !b.action) || !b.logp_old || !b.adv || (p.critic && !b.ret) || (cost && !cost->cost_ret)) return PGD_ERR_ARG;
  if (lds > 65536) return PGD_ERR_ARG;
  if (b.rows < 1 || b.rows > PGD_PPO_ROWS_MAX || b.n_list < 0 || b.n_rows < 1 || b.start < 0 || b.stride < 1) return PGD_ERR_ARG;
  if ((long long)b.start + (long long)(b.rows - 1) * b.stride > 2147483647ll) return PGD_ERR_ARG;
  if (!b.index && b.n_list > b.n_rows) return PGD_ERR_ARG;  // (without an index a list position IS a row)
  p.n_nets = cost_net ? 3 : (p.critic ? 2 : 1);
  p.out_cols = (int)nets->out_cols;
  p.wk = work_of(b.in_dim, b.rows, p.n_nets);
  if (work_bytes < sizeof(float) * p.wk.total) return PGD_ERR_ARG;
  p.bound = h->obs_norm.table != nullptr;
  if (p.bound && b.in_dim != h->obs_norm.in_dim) return PGD_ERR_ARG;
  p.nm = ObsNorm{h->obs_norm.table, h->obs_norm.clip};
  return PGD_OK;
}
// head columns [16, out_cols) of dW3 and [4, out_cols) of db3: zero (behind the reduction, in front of the statistics launch that writes db3)
static void ppo_zero_head_launch(hipStream_t s, const pgd_ppo_grads* grads, int out_cols) {
  hipLaunchKernelGGL(k_ppo_zero_head, dim3(std::max(1, std::min(out_cols - 16, 64))), dim3(MLP_H), 0, s, grads->w3, grads->b3, out_cols);
}

// (the one body of pgd_ppo_grad, pgd_ppo_grad_cost and pgd_ppo_grad_guided, ppo_grad_launch: pgd_guided.h, behind the guided kernels)
extern "C" {

int pgd_mlp_actor_critic_cost(pgd_handle h, int group, const float* d_obs, int obs_stride, int in_dim, const pgd_actor_critic* nets,
                              const pgd_value_net* cost_net, uint32_t seed, uint32_t tick, uint32_t flags, float* d_actions, float* d_logp,
                              float* d_value, float* d_cost_value) {
  bool critic;
  if (!h || !d_obs || !cost_net || !d_actions || !d_logp || !d_value || !d_cost_value || (flags & ~PGD_AC_DETERMINISTIC) != 0u ||
      !nets_ok(nets, cost_net, false, in_dim, obs_stride, &critic) || ac_lds_bytes(in_dim) > 65536) return PGD_ERR_ARG;
  return ac_forward(h, group, LDS_AC_COST, k_mlp_actor_critic_cost<false>, k_mlp_actor_critic_cost<true>, in_dim, [&](const AcRows& r, auto kern) {
    const SafeNets sn = {*nets, *cost_net};
    hipLaunchKernelGGL(kern, dim3((r.rows + MLP_ROWS - 1) / MLP_ROWS, 3), dim3(WAVE * MLP_WAVES), r.lds, r.stream, d_obs, r.row0,
                       r.rows, obs_stride, in_dim, sn, seed, tick, h->ac_tick, r.row_base, flags, d_actions, d_logp, d_value, d_cost_value, r.nm);
  });
}

int pgd_cost_gae(pgd_handle h, const uint32_t* d_flags, const uint8_t* d_done, const float* d_cost_value, int T, int rows, const float costs[3],
                 float gamma, float lam, float* d_cost, float* d_cadv, float* d_cret, float* d_run, float* d_ep_sum, int32_t* d_ep_count) {
  if (!h || !d_flags || !d_done || !d_cost_value || !costs || !d_cost || !d_cadv || !d_cret || !d_run || !d_ep_sum || !d_ep_count || T < 1 ||
      rows < 1) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_cost_gae, dim3((rows + WAVE - 1) / WAVE), dim3(WAVE), 0, h->stream, d_flags, d_done, d_cost_value, T, rows, costs[0], costs[1],
                     costs[2], gamma, lam, d_cost, d_cadv, d_cret, d_run, d_ep_sum, d_ep_count);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

int pgd_lagrange(pgd_handle h, const float* d_ep_sum, const int32_t* d_ep_count, int rows, float cost_limit, float lr, float lambda_max,
                 float* d_state) {
  if (!h || !d_ep_sum || !d_ep_count || !d_state || rows < 1 || !(lambda_max >= 0.0f)) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_lagrange, dim3(1), dim3(256), 0, h->stream, d_ep_sum, d_ep_count, rows, cost_limit, lr, lambda_max, d_state);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

int pgd_adv_mix(pgd_handle h, const float* d_adv, const float* d_cadv, int n, const float* d_adv_stats, const float* d_cadv_stats,
                const float* d_state, float* d_out) {
  if (!h || !d_adv || !d_cadv || !d_state || !d_out || n < 1) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_adv_mix, dim3((n + 255) / 256), dim3(256), 0, h->stream, d_adv, d_cadv, n, d_adv_stats, d_cadv_stats, d_state, d_out);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

size_t pgd_ppo_cost_work_bytes(int in_dim, int rows) { return ppo_work_bytes(in_dim, rows, 3); }

int pgd_ppo_grad_cost(pgd_handle h, const pgd_actor_critic* nets, const pgd_value_net* cost_net, const pgd_ppo_batch* batch,
                      const pgd_ppo_cost* cost, const pgd_ppo_hyper* hyper, const pgd_ppo_grads* grads, const pgd_value_grads* cost_grads,
                      float* d_stats, void* d_work, size_t work_bytes) {
  if (!cost_net || !cost || !cost_grads) return PGD_ERR_ARG;
  return ppo_grad_launch(h, nets, cost_net, batch, cost, nullptr, hyper, grads, cost_grads, d_stats, d_work, work_bytes);
}

}  // extern "C"

#endif
