// pgd_obs_norm.h -- observation normalisation (the norm_obs half of Stable-Baselines3's VecNormalize): the running mean and variance of
// every observation column (pgd_obs_norm_update), the table the network kernels read (pgd_obs_norm_publish) and the engine's binding of
// it (pgd_obs_norm_bind).  include/pgdrive_hip.h states the rule.  Part of the single translation unit pgd_engine.hip (included at its
// end, behind pgd_return_norm.h, whose RnStat it uses; ppo_count is pgd_ppo.h's).  The normalisation itself is not here: it happens in the
// row loaders of the training kernels (ObsNorm / on_apply, pgd_actor_critic.h), chosen by the host paths ac_forward and ppo_grad_launch.
// No reference counterpart: the reference hands its observations to an RL library, which wraps the env (VecNormalize) on the host.
//
// pgd_obs_norm_update, two launches, the record written by the second alone:
//   k_obs_norm_part   grid (partitions of ON_PART list positions, chunks of 64 columns), one wave per workgroup: lane l owns column
//                     64 y + l, so the wave reads 64 consecutive floats of one row per position (a row is contiguous in memory), ON_BATCH
//                     positions in flight.  Per column, in double: K = the partition's first sample, s1 = sum (x - K), s2 = sum (x - K)^2
//                     in list order, then mean = K + s1 / n, m2 = max(s2 - s1 (s1 / n), 0).  The live positions are a prefix of the
//                     list, so a partition knows its n from the count alone; a partition without a live position writes nothing.
//                     Workgroup (0, 0) also copies the record's n into the scratch: the second launch reads it there, so no launch
//                     reads a word that another workgroup of the same launch writes.
//   k_obs_norm_merge  one thread per column: the live partitions merged in partition order by Chan's update, the call's statistic
//                     then merged into the record.  No live position: nothing is written.
// Every product that feeds a sum is an explicit fma (the library's build contracts whatever it may, pragma or not: build.py), so the
// arithmetic is one a checker can repeat operation for operation; no atomics, every order fixed: the same inputs give the same bytes.
#ifndef PGD_OBS_NORM_H
#define PGD_OBS_NORM_H

#define ON_PART 512   // list positions per partition
#define ON_BATCH 16   // positions a lane keeps in flight
#define ON_DIM_MIN 4
#define ON_DIM_MAX 416
#define ON_HEAD 2     // doubles in front of the partials: the record's n before the call, one unused

// rn_merge with its two fused operations spelled out: a <- a + b; an empty a gives b's bits
DEV RnStat on_merge(const RnStat a, const RnStat b) {
#pragma clang fp reassociate(off)
  const double tot = a.n + b.n;
  const double w = b.n > 0.0 ? b.n / tot : 0.0;
  const double delta = b.mean - a.mean;
  const double d2 = delta * delta, aw = a.n * w, m2 = a.m2 + b.m2;
  RnStat o;
  o.n = tot;
  o.mean = fma(delta, w, a.mean);
  o.m2 = fma(d2, aw, m2);
  return o;
}

// partial [part][2][in_dim] doubles behind the head: mean | m2
template <bool INDEX>
__global__ __launch_bounds__(WAVE) void k_obs_norm_part(const float* __restrict__ obs, const int obs_stride, const int in_dim, const int n_rows,
                                                        const int32_t* __restrict__ index, const int32_t* __restrict__ count, const int n_list,
                                                        const double* __restrict__ record, double* __restrict__ work) {
#pragma clang fp reassociate(off)
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) work[0] = record[0];
  const int n = ppo_count(count, n_list);
  const int q0 = (int)blockIdx.x * ON_PART;
  const int cnt = min(n - q0, ON_PART);
  if (cnt <= 0) return;
  const int k = (int)blockIdx.y * WAVE + (int)threadIdx.x;
  const bool k_in = k < in_dim;
  const int kk = k_in ? k : in_dim - 1;  // (a lane past the last column reads that column and writes nothing)
  double K = 0.0, s1 = 0.0, s2 = 0.0;
  for (int j0 = 0; j0 < cnt; j0 += ON_BATCH) {
    int row[ON_BATCH];
    float x[ON_BATCH];
#pragma unroll
    for (int j = 0; j < ON_BATCH; ++j) {
      const int q = q0 + min(j0 + j, cnt - 1);  // (a slot past the partition's end reads its last position and is selected away)
      row[j] = INDEX ? max(0, min(index[q], n_rows - 1)) : q;
    }
#pragma unroll
    for (int j = 0; j < ON_BATCH; ++j) x[j] = obs[(size_t)row[j] * obs_stride + kk];
#pragma unroll
    for (int j = 0; j < ON_BATCH; ++j) {
      const bool in = j0 + j < cnt;
      const double xd = (double)x[j];
      K = j0 + j == 0 ? xd : K;
      const double dx = xd - K;
      s1 = in ? s1 + dx : s1;
      s2 = in ? fma(dx, dx, s2) : s2;
    }
  }
  const double q = s1 / (double)cnt;
  if (k_in) {
    double* p = work + ON_HEAD + (size_t)blockIdx.x * 2 * in_dim;
    p[k] = K + q;
    p[in_dim + k] = fmax(fma(-s1, q, s2), 0.0);
  }
}

__global__ __launch_bounds__(WAVE) void k_obs_norm_merge(const int in_dim, const int32_t* __restrict__ count, const int n_list,
                                                         const double* __restrict__ work, double* __restrict__ record) {
  const int n = ppo_count(count, n_list);
  const int k = (int)blockIdx.x * WAVE + (int)threadIdx.x;
  if (n <= 0 || k >= in_dim) return;  // (a call with no live position leaves every byte of the record)
  const int n_part = (n + ON_PART - 1) / ON_PART;
  const double* __restrict__ part = work + ON_HEAD;
  RnStat s = {0.0, 0.0, 0.0};
  for (int p0 = 0; p0 < n_part; p0 += PPO_BATCH) {  // (PPO_BATCH partials in flight, then their merges in partition order)
    double mean[PPO_BATCH], m2[PPO_BATCH];
#pragma unroll
    for (int j = 0; j < PPO_BATCH; ++j) {
      const size_t at = (size_t)min(p0 + j, n_part - 1) * 2 * in_dim + k;
      mean[j] = part[at];
      m2[j] = part[at + in_dim];
    }
#pragma unroll
    for (int j = 0; j < PPO_BATCH; ++j) {
      if (p0 + j < n_part) {
        const RnStat b = {(double)min(n - (p0 + j) * ON_PART, ON_PART), mean[j], m2[j]};
        s = on_merge(s, b);
      }
    }
  }
  const RnStat rec = on_merge(RnStat{work[0], record[1 + k], record[1 + in_dim + k]}, s);
  record[1 + k] = rec.mean;
  record[1 + in_dim + k] = rec.m2;
  if (k == 0) record[0] = rec.n;
}

// table [2][kp]: shift | scale; the identity where the record is empty and in the padding columns
__global__ __launch_bounds__(256) void k_obs_norm_publish(const double* __restrict__ record, const int in_dim, const double eps,
                                                          float* __restrict__ table) {
  const int kp = (in_dim + 3) & ~3, k = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (k >= kp) return;
  const double n = record[0];
  float shift = 0.0f, scale = 1.0f;
  if (k < in_dim && n > 0.0) {
    shift = (float)record[1 + k];
    scale = (float)(1.0 / sqrt(record[1 + in_dim + k] / n + eps));
  }
  table[k] = shift;
  table[kp + k] = scale;
}

static size_t on_work_bytes(int in_dim, int n_list) {
  if (in_dim < ON_DIM_MIN || in_dim > ON_DIM_MAX || n_list < 1) return 0;
  return sizeof(double) * (ON_HEAD + (size_t)((n_list + ON_PART - 1) / ON_PART) * 2 * (size_t)in_dim);
}

extern "C" {

size_t pgd_obs_norm_work_bytes(int in_dim, int n_list) { return on_work_bytes(in_dim, n_list); }

int pgd_obs_norm_update(pgd_handle h, const float* d_obs, int obs_stride, int in_dim, int n_rows, const int32_t* d_index, const int32_t* d_count,
                        int n_list, double* d_record, void* d_work, size_t work_bytes) {
  if (!h || !d_obs || !d_record || !d_work || in_dim < ON_DIM_MIN || in_dim > ON_DIM_MAX || obs_stride < in_dim || n_rows < 1 || n_list < 1)
    return PGD_ERR_ARG;
  if (!d_index && n_list > n_rows) return PGD_ERR_ARG;  // (without an index a list position IS a row)
  if (((uintptr_t)d_record & 7u) != 0u || ((uintptr_t)d_work & 7u) != 0u || work_bytes < on_work_bytes(in_dim, n_list)) return PGD_ERR_ARG;
  if ((((uintptr_t)d_obs | (uintptr_t)d_index | (uintptr_t)d_count) & 3u) != 0u) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  const dim3 grid((unsigned)((n_list + ON_PART - 1) / ON_PART), (unsigned)((in_dim + WAVE - 1) / WAVE));
  double* work = static_cast<double*>(d_work);
  if (d_index)
    hipLaunchKernelGGL(k_obs_norm_part<true>, grid, dim3(WAVE), 0, h->stream, d_obs, obs_stride, in_dim, n_rows, d_index, d_count, n_list, d_record, work);
  else
    hipLaunchKernelGGL(k_obs_norm_part<false>, grid, dim3(WAVE), 0, h->stream, d_obs, obs_stride, in_dim, n_rows, d_index, d_count, n_list, d_record, work);
  hipLaunchKernelGGL(k_obs_norm_merge, dim3(grid.y), dim3(WAVE), 0, h->stream, in_dim, d_count, n_list, work, d_record);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

int pgd_obs_norm_publish(pgd_handle h, const double* d_record, int in_dim, double eps, float* d_table) {
  if (!h || !d_record || !d_table || in_dim < ON_DIM_MIN || in_dim > ON_DIM_MAX || !(eps >= 0.0)) return PGD_ERR_ARG;
  if (((uintptr_t)d_record & 7u) != 0u || ((uintptr_t)d_table & 15u) != 0u) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  const int kp = (in_dim + 3) & ~3;
  hipLaunchKernelGGL(k_obs_norm_publish, dim3((kp + 255) / 256), dim3(256), 0, h->stream, d_record, in_dim, eps, d_table);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

int pgd_obs_norm_bind(pgd_handle h, const float* d_table, int in_dim, float clip) {
  if (!h) return PGD_ERR_ARG;
  if (!d_table) {
    h->obs_norm = {nullptr, 0, 0.0f};
    return PGD_OK;
  }
  if (in_dim < ON_DIM_MIN || in_dim > ON_DIM_MAX || !(clip > 0.0f) || ((uintptr_t)d_table & 15u) != 0u) return PGD_ERR_ARG;
  h->obs_norm = {d_table, in_dim, clip};
  return PGD_OK;
}

}  // extern "C"

#endif
