// pgd_step_info.h -- step info on the device (include/pgdrive_hip.h, pgd_step_info): the info values of every env, the terminal row
// and the statistics of every episode that ended, and the restart of those envs, by ONE kernel after the step.  Part of the single
// translation unit pgd_engine.hip (included at its end; uses observe_row of pgd_observe.h and the engine handle).
//
// While the info is enabled, step_impl clears cfg.auto_reset in the by-value PgdDev it hands to k_step: phase (8) of the step (the
// restart) is then never taken -- auto_reset is read nowhere else on the single-agent path and is in none of the PGD_FIX*_FIELDS
// lists, so the same instantiations launch -- and the step leaves the terminal state in memory and the terminal row in the caller's
// buffer.  k_step_info then works from memory alone, which is why it serves every single-agent engine mode (one env per wave, several,
// throughput mode, objects, detector fans, random_agent_model, IDM_agent): one wave per env, whatever the step's lane mapping was.
#ifndef PGD_STEP_INFO_H
#define PGD_STEP_INFO_H

struct StepInfoAcc { float energy_base, total_cost; };  // per env, engine-owned: episode_energy of the previous step, running cost sum

struct pgd_step_info_state {
  pgd_step_info info;
  StepInfoAcc* acc;  // [N]
};

// One wave per env `env0 + blockIdx.x`.  OTH: the row layout of observe_row (neighbour rows as state vectors).
template <bool OTH>
__global__ __launch_bounds__(WAVE) void k_step_info(PgdDev d, const pgd_step_info si, StepInfoAcc* __restrict__ acc, int env0, int restart,
                                                    const uint8_t* __restrict__ done, uint32_t* __restrict__ flags, float* __restrict__ obs) {
  __shared__ ObsLds L;
  const int e = env0 + (int)blockIdx.x, tid = (int)threadIdx.x, V = d.V, D = d.D;
  if (e >= d.N) return;
  RecPiece* recs = rec_block(d.rec, (size_t)e, V);
  int32_t* ew = d.ei + (size_t)e * PGD_NEI;
  // (1) the info values of the state the step ended in: the agent's record (slot 0), the env's counters, the step's flags
  const uint4 p1 = recs[1 * V].q, p6 = recs[6 * V].q, p7 = recs[7 * V].q;  // (hx hy lon steer) (a0s a0t a1s a1t) (energy dl dr eprew)
  const float speed = __uint_as_float(recs[0].q.w);
  const float steer = __uint_as_float(p1.w), a1t = __uint_as_float(p6.w), energy = __uint_as_float(p7.x), eprew = __uint_as_float(p7.w);
  const int ep_steps = ew[EI_EP_STEPS];
  const uint32_t fl = flags[e];
  const bool dn = done[e] != 0;
  const StepInfoAcc a0 = acc[e];
  const float cost = (fl & PGD_F_OUT_OF_ROAD) ? si.out_of_road_cost
                     : (fl & PGD_F_CRASH_VEHICLE) ? si.crash_vehicle_cost
                     : (fl & PGD_F_CRASH_OBJECT) ? si.crash_object_cost : 0.0f;
  const float total = a0.total_cost + cost;
  const bool again = dn && restart != 0;
  if (tid == 0) {
    if (si.velocity) si.velocity[e] = fabsf(speed) * 3.6f;
    if (si.steering) si.steering[e] = steer;
    if (si.acceleration) si.acceleration[e] = a1t;
    if (si.episode_energy) si.episode_energy[e] = energy;
    if (si.step_energy) si.step_energy[e] = energy - a0.energy_base;
    if (si.episode_reward) si.episode_reward[e] = eprew;
    if (si.episode_length) si.episode_length[e] = ep_steps;
    if (si.cost) si.cost[e] = cost;
    if (si.total_cost) si.total_cost[e] = total;
    acc[e] = again ? StepInfoAcc{0.0f, 0.0f} : StepInfoAcc{energy, total};
  }
  if (!dn) return;  // (wave-uniform)
  // (2) the terminal row, (3) the episode's statistics
  if (si.final_obs && obs)
    for (int k = tid; k < D; k += WAVE) si.final_obs[(size_t)e * D + k] = obs[(size_t)e * D + k];
  if (tid == 0) {
    if (si.ep_count) si.ep_count[e] += 1;
    if (si.ep_return_sum) si.ep_return_sum[e] += eprew;
    if (si.ep_length_sum) si.ep_length_sum[e] += ep_steps;
    if (si.ep_cost_sum) si.ep_cost_sum[e] += total;
    if (si.ep_arrive && (fl & PGD_F_ARRIVE)) si.ep_arrive[e] += 1;
    if (si.ep_out_of_road && (fl & PGD_F_OUT_OF_ROAD)) si.ep_out_of_road[e] += 1;
    if (si.ep_crash && (fl & (PGD_F_CRASH_VEHICLE | PGD_F_CRASH_OBJECT | PGD_F_CRASH_BUILDING))) si.ep_crash[e] += 1;
    if (si.ep_max_step && (fl & PGD_F_MAX_STEP)) si.ep_max_step[e] += 1;
  }
  if (!again) return;
  // (4) the restart, as phase (8) of k_step (base_env.py:269-301): the scenario re-drawn from the same counter stream, every slot from
  // the scenario's reset image, the env's header copy, its counters; the hints and the image mask as k_reset leaves them
  const int episodes = ew[EI_EPISODES] + 1;
  int scen = ew[EI_SCEN];
  if (d.cfg.resample_scenario)
    scen = (int)(pgd_rng(d.cfg.seed, (uint32_t)(d.cfg.env_base + e), 0x5ce9a210u, (uint32_t)episodes) % (uint32_t)d.n_scen);
  const RecPiece* img = rec_block(d.reset_img(), (size_t)scen, V);
  for (int k = tid; k < 8 * V; k += WAVE) recs[k].q = img[k].q;
  if (d.cfg.resample_scenario)
    for (int q = tid; q < (int)(sizeof(pgd_map) / 16); q += WAVE)
      reinterpret_cast<uint4*>(d.env_map + e)[q] = reinterpret_cast<const uint4*>(d.scen_map().at((uint32_t)scen))[q];
  if (tid == 0) {
    ew[EI_SCEN] = scen;
    ew[EI_EPISODES] = episodes;
    ew[EI_NEXT_AGENT] = 1;
    ew[EI_AUX] = d.scen()[scen].aux;
    ew[EI_NEXT_GROUP] = 0;
    ew[EI_EP_STEPS] = 0;
    ew[EI_NEAR] = 1;  // test / unknown
    d.imask[e] = ((d.epw == 1 || d.pack_obs) && d.use_imask) ? (V >= 64 ? ~0ull : ((1ull << V) - 1ull)) : 0ull;
    if (d.bev_fill) d.bev_fill[e] = 1;
    flags[e] = fl | PGD_F_RESET;  // (6)
  }
  // (5) the first row of the new episode, by the row code of k_observe (the records above are visible to the whole wave from here; the
  // terminal row has been copied)
  if (!obs) return;
  __syncthreads();
  observe_row<WAVE, OTH>(d, obs, nullptr, e, 0, tid, L, scen);
}

// an empty launch of the same shape: the launch floor that tools/step_info_ab.py measures beside the two steps
__global__ __launch_bounds__(WAVE) void k_step_info_empty() {}

// pgd_reset: the listed envs (null: all) start their episode with no cost and no energy behind them
__global__ __launch_bounds__(256) void k_step_info_forget(StepInfoAcc* __restrict__ acc, const int32_t* __restrict__ env_ids, int n) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) acc[env_ids ? env_ids[k] : k] = StepInfoAcc{0.0f, 0.0f};
}

static void step_info_free(pgd_engine* h) {
  if (!h->sinfo) return;
  if (h->sinfo->acc) (void)hipFree(h->sinfo->acc);
  free(h->sinfo);
  h->sinfo = nullptr;
}

static int step_info_forget(pgd_engine* h, const int32_t* d_env, int n) {
  if (!h->sinfo) return PGD_OK;  // (d_env: pgd_reset's device copy of its id list, null = envs 0 .. n - 1)
  hipLaunchKernelGGL(k_step_info_forget, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->sinfo->acc, d_env, n);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

// after the step kernel (and the observation launch of an engine that does not fuse it) of env group `g`, on its stream
static int step_info_launch(pgd_engine* h, const EnvGroup& g, const uint8_t* d_done, uint32_t* d_flags, float* d_obs) {
  auto kern = others_state_rows(h) ? k_step_info<true> : k_step_info<false>;
  hipLaunchKernelGGL(kern, dim3(g.count), dim3(WAVE), 0, g.stream, h->d, h->sinfo->info, h->sinfo->acc, g.first, h->d.cfg.auto_reset,
                     d_done, d_flags, d_obs);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

extern "C" {

int pgd_step_info_enable(pgd_handle h, const pgd_step_info* info) {
  if (!h) return PGD_ERR_ARG;
  if (info && is_marl(h)) return PGD_ERR_ARG;  // (their terminal rows survive the step: pgdrive_hip.h)
  HIPCHK(hipSetDevice(h->device));
  // a run-time step kernel has auto_reset as a literal: the one loaded now was built for the other setting
  if (h->jit_mod && (info != nullptr) != (h->sinfo != nullptr)) { int rc = pgd_set_step_module(h, nullptr, 0, 0); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int g = 0; h->gstreams && g < h->n_groups; ++g) HIPCHK(hipStreamSynchronize(h->gstreams[g]));
  if (!info) { step_info_free(h); return PGD_OK; }
  if (!h->sinfo) {
    h->sinfo = (pgd_step_info_state*)calloc(1, sizeof(pgd_step_info_state));
    HIPCHK(hipMalloc((void**)&h->sinfo->acc, sizeof(StepInfoAcc) * (size_t)h->d.N));
    HIPCHK(hipMemsetAsync(h->sinfo->acc, 0, sizeof(StepInfoAcc) * (size_t)h->d.N, h->stream));
  }
  h->sinfo->info = *info;
  return PGD_OK;
}

int pgd_step_info_clear_stats(pgd_handle h) {
  if (!h) return PGD_ERR_ARG;
  if (!h->sinfo) return PGD_ERR_STATE;
  HIPCHK(hipSetDevice(h->device));
  const pgd_step_info& s = h->sinfo->info;
  void* arr[] = {s.ep_count, s.ep_return_sum, s.ep_length_sum, s.ep_cost_sum, s.ep_arrive, s.ep_out_of_road, s.ep_crash, s.ep_max_step};
  for (void* p : arr)
    if (p) HIPCHK(hipMemsetAsync(p, 0, 4 * (size_t)h->d.N, h->stream));
  return PGD_OK;
}

// the launch floor beside a step (tools/step_info_ab.py): one empty launch of k_step_info's shape on the engine's stream
int pgd_step_info_empty_launch(pgd_handle h) {
  if (!h) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_step_info_empty, dim3(h->d.N), dim3(WAVE), 0, h->stream);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

}  // extern "C"
#endif
