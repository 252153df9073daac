// pgd_return_norm.h -- reward scaling by the standard deviation of the running discounted return (the norm_reward half of
// Stable-Baselines3's VecNormalize), for the rollouts of every collector: pgd_return_norm.  include/pgdrive_hip.h states the rule.  Part
// of the single translation unit pgd_engine.hip (included at its end, behind pgd_timelimit.h; ro_acted / ro_cont are pgd_marl_rollout.h's).
// No reference counterpart: the reference hands its rewards to an RL library, which wraps the env (VecNormalize) on the host.
//
// Three launches, the record written by one workgroup between two launches that only read it (the reasoning of k_adam_prep / k_adam):
//   k_return_norm_scan   one thread per row, one wave per workgroup (k_gae's shape: the time-major layout makes a wave's reads
//                        consecutive).  t runs forward; the loads of RN_BATCH steps are issued together, the fma chain of R behind them.
//                        The row's samples go into shifted sums in double -- K = the row's first sample, s1 = sum (x - K),
//                        s2 = sum (x - K)^2 -- and leave as (n, mean = K + s1 / n, m2 = s2 - s1^2 / n).  K is itself a sample, so
//                        s2 <= n m2: the subtraction loses at most log2(n) bits of a double (n <= T), and no division sits on the
//                        per-sample chain as Welford's would.  The wave merges its 64 rows by Chan's update over shuffles, lane l
//                        with lane l + 32, 16, .. 1 in that order; lane 0 writes the workgroup's partial (n, mean, m2).
//   k_return_norm_merge  ONE workgroup: thread i merges partials i, i + 256, .. in order, each wave merges its lanes as above, thread 0
//                        the four waves in order, then the call's statistic into the record, and writes the scale.
//   k_return_norm_scale  elementwise, one entry per thread (four per thread on 16-byte aligned arrays measured 2.96 against 3.08 us at
//                        128 x 4096, inside each other's spread: profiles/return_norm_notes.md).
// No atomics, every order fixed: the same inputs give the same bytes.  PGD_RN_FREEZE: the third launch alone.
#ifndef PGD_RETURN_NORM_H
#define PGD_RETURN_NORM_H

#define RN_BATCH 8
#define RN_THREADS 256

struct RnStat { double n, mean, m2; };  // the number of samples, their mean and their sum of squared deviations

// Chan's parallel update, a <- a + b; an empty b (n = 0, mean = 0, m2 = 0) leaves a's bits, an empty a gives b
DEV RnStat rn_merge(const RnStat a, const RnStat b) {
#pragma clang fp reassociate(off)
  const double tot = a.n + b.n;
  const double w = b.n > 0.0 ? b.n / tot : 0.0;
  const double delta = b.mean - a.mean;
  RnStat o;
  o.n = tot;
  o.mean = a.mean + delta * w;
  o.m2 = a.m2 + b.m2 + delta * delta * (a.n * w);
  return o;
}

// lane 0 receives the 64 lanes merged as ((l, l + 32), (.., + 16), ..): a fixed order
DEV RnStat rn_wave_merge(RnStat s) {
#pragma unroll
  for (int k = WAVE / 2; k >= 1; k >>= 1) {
    RnStat o;
    o.n = __shfl_down(s.n, k);
    o.mean = __shfl_down(s.mean, k);
    o.m2 = __shfl_down(s.m2, k);
    s = rn_merge(s, o);
  }
  return s;
}

template <bool FLAGS>
__global__ __launch_bounds__(WAVE) void k_return_norm_scan(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                           const uint32_t* __restrict__ flags, const int T, const int rows, const float gamma,
                                                           float* __restrict__ carry, double* __restrict__ partial) {
#pragma clang fp reassociate(off)
  const int r = (int)blockIdx.x * WAVE + (int)threadIdx.x;
  const bool row_in = r < rows;
  const int rr = row_in ? r : rows - 1;  // (a lane behind the last row reads that row and contributes nothing: every lane reaches the shuffles)
  float R = carry[rr];
  double K = 0.0, s1 = 0.0, s2 = 0.0;
  int n = 0;
  for (int t0 = 0; t0 < T; t0 += RN_BATCH) {
    float rw[RN_BATCH];
    uint8_t dn[RN_BATCH];
    uint32_t fl[RN_BATCH];
#pragma unroll
    for (int j = 0; j < RN_BATCH; ++j) {
      const size_t i = (size_t)min(t0 + j, T - 1) * rows + rr;
      rw[j] = reward[i];
      dn[j] = done[i];
      fl[j] = FLAGS ? flags[i] : PGD_F_REPORT;
    }
#pragma unroll
    for (int j = 0; j < RN_BATCH; ++j) {
      const bool step_in = row_in && t0 + j < T;
      const bool acted = step_in && ro_acted(fl[j]);
      const float Rn = fmaf(gamma, R, rw[j]);
      const double x = (double)Rn;
      K = n == 0 ? x : K;
      const double dx = x - K;
      s1 = acted ? s1 + dx : s1;
      s2 = acted ? fma(dx, dx, s2) : s2;
      n += acted ? 1 : 0;
      // (selections: the reward of a row that did not act may be NaN and reaches nothing)
      if (t0 + j < T) R = acted && ro_cont(fl[j], dn[j]) ? Rn : 0.0f;
    }
  }
  if (row_in) carry[r] = R;
  RnStat s = {0.0, 0.0, 0.0};
  if (n > 0) {
    const double cnt = (double)n, q = s1 / cnt;
    s.n = cnt;
    s.mean = K + q;
    s.m2 = fmax(s2 - s1 * q, 0.0);
  }
  s = rn_wave_merge(s);
  if (threadIdx.x == 0) {
    double* p = partial + 3 * (size_t)blockIdx.x;
    p[0] = s.n;
    p[1] = s.mean;
    p[2] = s.m2;
  }
}

// record: count, mean, m2, scale
__global__ __launch_bounds__(RN_THREADS) void k_return_norm_merge(const double* __restrict__ partial, const int n_part, const double eps,
                                                                  double* __restrict__ record) {
  __shared__ double wave_stat[RN_THREADS / WAVE][3];
  RnStat s = {0.0, 0.0, 0.0};
  for (int i = (int)threadIdx.x; i < n_part; i += RN_THREADS) {
    const RnStat p = {partial[3 * (size_t)i], partial[3 * (size_t)i + 1], partial[3 * (size_t)i + 2]};
    s = rn_merge(s, p);
  }
  s = rn_wave_merge(s);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    double* w = wave_stat[threadIdx.x / WAVE];
    w[0] = s.n;
    w[1] = s.mean;
    w[2] = s.m2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < RN_THREADS / WAVE; ++k) {
      const RnStat p = {wave_stat[k][0], wave_stat[k][1], wave_stat[k][2]};
      s = rn_merge(s, p);
    }
    RnStat rec = {record[0], record[1], record[2]};
    if (s.n > 0.0) {  // (a call without a sample leaves count, mean and m2 their bytes)
      rec = rn_merge(rec, s);
      record[0] = rec.n;
      record[1] = rec.mean;
      record[2] = rec.m2;
    }
    record[3] = 1.0 / sqrt(rec.m2 / rec.n + eps);
  }
}

DEV float rn_scaled(const float reward, const uint32_t f, const float scale, const float clip) {
  float x = reward * scale;
  if (clip > 0.0f) x = fminf(fmaxf(x, -clip), clip);
  return ro_acted(f) ? x : 0.0f;  // (a selection)
}

// entry i of the flat arrays [0, n)
template <bool FLAGS>
__global__ __launch_bounds__(RN_THREADS) void k_return_norm_scale(const float* __restrict__ reward, const uint32_t* __restrict__ flags, const size_t n,
                                                                  const float clip, const double* __restrict__ record, float* __restrict__ scaled) {
  const size_t i = (size_t)blockIdx.x * RN_THREADS + threadIdx.x;
  if (i >= n) return;
  scaled[i] = rn_scaled(reward[i], FLAGS ? flags[i] : PGD_F_REPORT, (float)record[3], clip);
}

static size_t rn_work_bytes(int rows) { return rows < 1 ? 0 : 3 * sizeof(double) * (size_t)((rows + WAVE - 1) / WAVE); }

extern "C" {

size_t pgd_return_norm_work_bytes(int rows) { return rn_work_bytes(rows); }

int pgd_return_norm(pgd_handle h, const float* d_reward, const uint8_t* d_done, const uint32_t* d_flags, int T, int rows, float gamma, double eps,
                    float clip, uint32_t mode, float* d_carry, double* d_record, float* d_scaled, void* d_work, size_t work_bytes) {
  if (!h || !d_reward || !d_done || !d_carry || !d_record || !d_scaled || !d_work || T < 1 || rows < 1) return PGD_ERR_ARG;
  if (!(gamma >= 0.0f && gamma <= 1.0f) || !(eps >= 0.0) || (mode & ~(uint32_t)PGD_RN_FREEZE) != 0u) return PGD_ERR_ARG;
  if (((uintptr_t)d_record & 7u) != 0u || ((uintptr_t)d_work & 7u) != 0u || work_bytes < rn_work_bytes(rows)) return PGD_ERR_ARG;
  if ((((uintptr_t)d_reward | (uintptr_t)d_flags | (uintptr_t)d_carry | (uintptr_t)d_scaled) & 3u) != 0u) return PGD_ERR_ARG;
  const size_t n = (size_t)T * (size_t)rows;
  const size_t blocks = (n + RN_THREADS - 1) / RN_THREADS;
  if (blocks > 0x7fffffffu) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  if (!(mode & PGD_RN_FREEZE)) {
    const int n_part = (rows + WAVE - 1) / WAVE;
    double* partial = static_cast<double*>(d_work);
    if (d_flags)
      hipLaunchKernelGGL(k_return_norm_scan<true>, dim3(n_part), dim3(WAVE), 0, h->stream, d_reward, d_done, d_flags, T, rows, gamma, d_carry, partial);
    else
      hipLaunchKernelGGL(k_return_norm_scan<false>, dim3(n_part), dim3(WAVE), 0, h->stream, d_reward, d_done, d_flags, T, rows, gamma, d_carry, partial);
    hipLaunchKernelGGL(k_return_norm_merge, dim3(1), dim3(RN_THREADS), 0, h->stream, partial, n_part, eps, d_record);
  }
  const dim3 grid((unsigned)blocks), block(RN_THREADS);
  if (d_flags) hipLaunchKernelGGL(k_return_norm_scale<true>, grid, block, 0, h->stream, d_reward, d_flags, n, clip, d_record, d_scaled);
  else hipLaunchKernelGGL(k_return_norm_scale<false>, grid, block, 0, h->stream, d_reward, d_flags, n, clip, d_record, d_scaled);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

}  // extern "C"

#endif
