// pgd_guided.h -- the PPO gradient that knows which rows of a rollout the expert guardian overrode (pgd_ppo_grad_guided): a guided row
// drops its clipped surrogate (or keeps it: PGD_GUIDE_KEEP_SURROGATE) and imitates a target action with the weight bc_coef; with every
// live row guided and no surrogate the call is behaviour cloning of the target.  include/pgdrive_hip.h states the formulas.  Part of the
// single translation unit pgd_engine.hip (included behind pgd_safe.h).  The host body of the whole pgd_ppo_grad family, ppo_grad_launch,
// is here, behind the last rows kernel it may launch.  No reference counterpart: the reference hands takeover / raw_action to an RL
// library (agent_manager.py:187).
//
// The launches are pgd_ppo_grad's / pgd_ppo_grad_cost's: k_ppo_prep(_cost), k_ppo_wgrad, k_ppo_reduce(_cost) and k_ppo_zero_head AS THEY
// ARE, over the same scratch (ppo_work), and two kernels of this file in the places of k_ppo_rows(_cost) and k_ppo_stats(_cost):
//   k_ppo_rows_guided / k_ppo_rows_cost_guided   ppo_rows_tile<NORM, GUIDED = true> (pgd_ppo.h): the text of k_ppo_rows with the actor's
//                 row lane extended.  The LDS is ppo_lds_bytes: the row record [16][PPO_ST] has its slots 9 .. 11 unused in the ACTOR's
//                 workgroup (9 and 10 are the critic's, in the critic's workgroup); there they hold u and -logp(target), and the tile's
//                 record of PPO_TS = 16 floats takes their sums in slots 13 and 14 -- the scratch does not grow either.
//   k_ppo_stats_guided   ppo_stats_block<GUIDED = true> (pgd_ppo.h): its order over the record's fifteen slots -> d_stats[12], db3 and the
//                 critics' db3
// A row's guided bit and target are read by ROW through ppo_row's clamp, at live rows only, the target only where the bit is set; the
// free part of dOut is formed by the expressions of k_ppo_rows from the same operands, so with no guided row everything downstream --
// the same kernels -- sees the same bits.  No atomics; every sum keeps its one owner and order.
#ifndef PGD_GUIDED_H
#define PGD_GUIDED_H

template <bool NORM>
__global__ __launch_bounds__(WAVE * MLP_WAVES, 4) void k_ppo_rows_guided(const pgd_actor_critic nets, const pgd_ppo_batch b, const pgd_ppo_hyper hp,
                                                                      const pgd_ppo_guide gd, float* __restrict__ work, const ObsNorm nm) {
  const bool critic = blockIdx.y != 0;
  ppo_rows_tile<NORM, true>(critic, critic ? nets.vw1 : nets.w1, critic ? nets.vb1 : nets.b1, critic ? nets.vw2 : nets.w2,
                            critic ? nets.vb2 : nets.b2, critic ? nets.vw3 : nets.w3, critic ? nets.vb3 : nets.b3, nets.out_cols, b.ret, hp.vf_coef, 0,
                            b, hp, work, nm, &gd);
}

template <bool NORM>
__global__ __launch_bounds__(WAVE * MLP_WAVES, 4) void k_ppo_rows_cost_guided(const SafeNets nets, const pgd_ppo_batch b, const pgd_ppo_hyper hp,
                                                                           const pgd_ppo_cost cost, const pgd_ppo_guide gd,
                                                                           float* __restrict__ work, const ObsNorm nm) {
  const int y = (int)blockIdx.y;
  const pgd_actor_critic& a = nets.ac;
  const pgd_value_net& c = nets.c;
  ppo_rows_tile<NORM, true>(y != 0, y == 0 ? a.w1 : (y == 1 ? a.vw1 : c.w1), y == 0 ? a.b1 : (y == 1 ? a.vb1 : c.b1),
                            y == 0 ? a.w2 : (y == 1 ? a.vw2 : c.w2), y == 0 ? a.b2 : (y == 1 ? a.vb2 : c.b2), y == 0 ? a.w3 : (y == 1 ? a.vw3 : c.w3),
                            y == 0 ? a.b3 : (y == 1 ? a.vb3 : c.b3), a.out_cols, y == 2 ? cost.cost_ret : b.ret,
                            y == 2 ? cost.cvf_coef : hp.vf_coef, y == 2 ? 2 : 0, b, hp, work, nm, &gd);
}

__global__ __launch_bounds__(256) void k_ppo_stats_guided(const pgd_ppo_batch b, const pgd_ppo_grads gr, const int has_critic,
                                                          float* __restrict__ cost_b3, const int keep, const float* __restrict__ work,
                                                          float* __restrict__ stats) {
  ppo_stats_block<true>(b, gr, has_critic, cost_b3, work, stats, keep);
}

// ---- the one body of pgd_ppo_grad (cost_net, cost, cost_grads, guide null), pgd_ppo_grad_cost (guide null) and pgd_ppo_grad_guided: one,
// two or three networks; with a guide the rows and the statistics launch are the guided kernels, every other launch is the same
static int ppo_grad_launch(pgd_handle h, const pgd_actor_critic* nets, const pgd_value_net* cost_net, const pgd_ppo_batch* batch,
                           const pgd_ppo_cost* cost, const pgd_ppo_guide* guide, const pgd_ppo_hyper* hyper, const pgd_ppo_grads* grads,
                           const pgd_value_grads* cost_grads, float* d_stats, void* d_work, size_t work_bytes) {
  PpoPlan p;
  const size_t lds = batch ? ppo_lds_bytes(batch->in_dim) : 0;
  { int rc = ppo_grad_plan(h, nets, cost_net, batch, true, cost, hyper, grads, cost_grads, d_stats, d_work, work_bytes, lds, ppo_work, p); if (rc) return rc; }
  const pgd_ppo_batch& b = *batch;
  const bool bound = p.bound, critic = p.critic;
  const int n_nets = p.n_nets, out_cols = p.out_cols;
  const PpoWork wk = p.wk;
  const ObsNorm nm = p.nm;
  const auto rows_cost = bound ? k_ppo_rows_cost<true> : k_ppo_rows_cost<false>;
  const auto rows_plain = bound ? k_ppo_rows<true> : k_ppo_rows<false>;
  const auto rows_cost_guided = bound ? k_ppo_rows_cost_guided<true> : k_ppo_rows_cost_guided<false>;
  const auto rows_guided = bound ? k_ppo_rows_guided<true> : k_ppo_rows_guided<false>;
  const auto wgrad = bound ? k_ppo_wgrad<true> : k_ppo_wgrad<false>;
  HIPCHK(hipSetDevice(h->device));
  const void* rows_kernel = guide ? (cost_net ? reinterpret_cast<const void*>(rows_cost_guided) : reinterpret_cast<const void*>(rows_guided))
                                  : (cost_net ? reinterpret_cast<const void*>(rows_cost) : reinterpret_cast<const void*>(rows_plain));
  const LdsKernel rows_slot = guide ? (cost_net ? LDS_PPO_ROWS_COST_GUIDED : LDS_PPO_ROWS_GUIDED) : (cost_net ? LDS_PPO_ROWS_COST : LDS_PPO_ROWS);
  { int rc = raise_lds_limit(h, lds_slot(rows_slot, bound), rows_kernel, lds); if (rc) return rc; }
  float* work = static_cast<float*>(d_work);
  hipStream_t s = h->stream;
  const dim3 prep(MLP_H, n_nets), rows(wk.R16 / 16, n_nets), reduce(16 * wk.mt, n_nets), tile(WAVE * MLP_WAVES);
  if (cost_net) {
    const SafeNets sn = {*nets, *cost_net};
    hipLaunchKernelGGL(k_ppo_prep_cost, prep, dim3(MLP_H), 0, s, sn, work);
    if (guide) hipLaunchKernelGGL(rows_cost_guided, rows, tile, lds, s, sn, b, *hyper, *cost, *guide, work, nm);
    else hipLaunchKernelGGL(rows_cost, rows, tile, lds, s, sn, b, *hyper, *cost, work, nm);
  } else {
    hipLaunchKernelGGL(k_ppo_prep, prep, dim3(MLP_H), 0, s, *nets, work);
    if (guide) hipLaunchKernelGGL(rows_guided, rows, tile, lds, s, *nets, b, *hyper, *guide, work, nm);
    else hipLaunchKernelGGL(rows_plain, rows, tile, lds, s, *nets, b, *hyper, work, nm);
  }
  hipLaunchKernelGGL(wgrad, dim3(wk.mt, wk.P, n_nets), tile, 0, s, b, work, nm);
  if (cost_net) {
    const SafeGrads sg = {*grads, *cost_grads};
    hipLaunchKernelGGL(k_ppo_reduce_cost, reduce, dim3(MLP_H), 0, s, b, sg, out_cols, work);
  } else {
    hipLaunchKernelGGL(k_ppo_reduce, reduce, dim3(MLP_H), 0, s, b, *grads, out_cols, work);
  }
  if (out_cols > 4) ppo_zero_head_launch(s, grads, out_cols);
  if (guide) hipLaunchKernelGGL(k_ppo_stats_guided, dim3(1), dim3(256), 0, s, b, *grads, critic ? 1 : 0, cost_net ? cost_grads->b3 : nullptr,
                                (guide->mode & PGD_GUIDE_KEEP_SURROGATE) != 0u ? 1 : 0, work, d_stats);
  else if (cost_net) hipLaunchKernelGGL(k_ppo_stats_cost, dim3(1), dim3(256), 0, s, b, *grads, cost_grads->b3, work, d_stats);
  else hipLaunchKernelGGL(k_ppo_stats, dim3(1), dim3(256), 0, s, b, *grads, critic ? 1 : 0, work, d_stats);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

extern "C" {

int pgd_ppo_grad_guided(pgd_handle h, const pgd_actor_critic* nets, const pgd_value_net* cost_net, const pgd_ppo_batch* batch,
                        const pgd_ppo_cost* cost, const pgd_ppo_guide* guide, const pgd_ppo_hyper* hyper, const pgd_ppo_grads* grads,
                        const pgd_value_grads* cost_grads, float* d_stats, void* d_work, size_t work_bytes) {
  if (!guide || !guide->target || guide->target_stride < 2 || (guide->mode & ~PGD_GUIDE_KEEP_SURROGATE) != 0u ||
      !(guide->bc_coef >= 0.0f && guide->bc_coef <= 3.402823466e38f) || (guide->mask && guide->mask_bits == 0u)) return PGD_ERR_ARG;
  if ((cost_net != nullptr) != (cost != nullptr) || (cost_net != nullptr) != (cost_grads != nullptr)) return PGD_ERR_ARG;
  return ppo_grad_launch(h, nets, cost_net, batch, cost, guide, hyper, grads, cost_grads, d_stats, d_work, work_bytes);
}

}  // extern "C"

#endif
