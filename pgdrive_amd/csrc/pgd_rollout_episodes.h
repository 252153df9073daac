// pgd_rollout_episodes.h -- the episode statistics of a rollout (gym's RecordEpisodeStatistics: return, length and the causes of the end
// of every episode that finished), for the rollouts of every collector: pgd_rollout_episodes.  include/pgdrive_hip.h states the rule.
// Part of the single translation unit pgd_engine.hip (included at its end, behind pgd_return_norm.h: rn_merge / rn_wave_merge are that
// header's, ro_acted / ro_cont pgd_marl_rollout.h's).  No reference counterpart: the reference reports an episode through the info dict
// of the step that ends it, and an RL library's wrapper keeps the books on the host.
//
// Two launches; the kernel boundary is the only ordering between them (no fence, no flag, no atomic):
//   k_rollout_episodes_scan   one thread per row, one wave per workgroup (k_return_norm_scan's shape: the time-major layout makes a
//                             wave's reads consecutive).  t runs forward; the loads of EP_BATCH steps are issued together, the chain of
//                             R and L behind them.  The returns of the row's finished episodes go into shifted sums in double, K = the
//                             row's first sample (pgd_return_norm.h says why that holds the accuracy), min and max in float, everything
//                             else in integers.  The wave merges its 64 rows over shuffles, lane l with lane l + 32, 16, .. 1 in that
//                             order; lane 0 writes the workgroup's partial: 16 doubles in the layout of the record.
//   k_rollout_episodes_merge  ONE workgroup: thread i merges partials i, i + 256, .. in order, each wave merges its lanes as above,
//                             thread 0 the four waves in order; it writes the call's own record and merges it into the running one.
// A single launch would need the last workgroup to find the others' partials: a counter, a release and an acquire (the per-XCD L2s are
// not coherent with each other) -- the second launch costs less than getting that right, and the order of the merge stays fixed.
// Every order is fixed: the same inputs give the same bytes.
#ifndef PGD_ROLLOUT_EPISODES_H
#define PGD_ROLLOUT_EPISODES_H

#define EP_BATCH 8
#define EP_THREADS 256
#define EP_RECORD 16  // doubles of a record and of a partial
#define EP_CAUSES 6   // PGD_F_ARRIVE .. PGD_F_MAX_STEP: bits 0 .. 5 of the flags, slots 7 .. 12 of the record

struct EpStat {
  RnStat ret;                  // number, mean and sum of squared deviations of the returns
  double mn, mx;               // least and greatest return
  double len_sum, len_max;     // of the lengths
  double cause[EP_CAUSES + 1]; // ends with the bit set; the last: ends without a done (cut)
  double steps;                // entries at which the row acted
};

DEV EpStat ep_empty() {
  EpStat s;
  s.ret = {0.0, 0.0, 0.0};
  s.mn = (double)INFINITY;
  s.mx = -(double)INFINITY;
  s.len_sum = s.len_max = s.steps = 0.0;
#pragma unroll
  for (int c = 0; c <= EP_CAUSES; ++c) s.cause[c] = 0.0;
  return s;
}

// a <- a + b: Chan's update of the returns, min / max, sums of integers held in doubles (exact)
DEV EpStat ep_merge(const EpStat a, const EpStat b) {
#pragma clang fp reassociate(off)
  EpStat o;
  o.ret = rn_merge(a.ret, b.ret);
  o.mn = fmin(a.mn, b.mn);
  o.mx = fmax(a.mx, b.mx);
  o.len_sum = a.len_sum + b.len_sum;
  o.len_max = fmax(a.len_max, b.len_max);
#pragma unroll
  for (int c = 0; c <= EP_CAUSES; ++c) o.cause[c] = a.cause[c] + b.cause[c];
  o.steps = a.steps + b.steps;
  return o;
}

// lane 0 receives the 64 lanes merged as ((l, l + 32), (.., + 16), ..): rn_wave_merge's order
DEV EpStat ep_wave_merge(EpStat s) {
#pragma unroll
  for (int k = WAVE / 2; k >= 1; k >>= 1) {
    EpStat o;
    o.ret.n = __shfl_down(s.ret.n, k);
    o.ret.mean = __shfl_down(s.ret.mean, k);
    o.ret.m2 = __shfl_down(s.ret.m2, k);
    o.mn = __shfl_down(s.mn, k);
    o.mx = __shfl_down(s.mx, k);
    o.len_sum = __shfl_down(s.len_sum, k);
    o.len_max = __shfl_down(s.len_max, k);
#pragma unroll
    for (int c = 0; c <= EP_CAUSES; ++c) o.cause[c] = __shfl_down(s.cause[c], k);
    o.steps = __shfl_down(s.steps, k);
    s = ep_merge(s, o);
  }
  return s;
}

// slots 0 .. 14 of a record or a partial
DEV EpStat ep_load(const double* __restrict__ p) {
  EpStat s;
  s.ret = {p[0], p[1], p[2]};
  s.mn = p[3];
  s.mx = p[4];
  s.len_sum = p[5];
  s.len_max = p[6];
#pragma unroll
  for (int c = 0; c <= EP_CAUSES; ++c) s.cause[c] = p[7 + c];
  s.steps = p[14];
  return s;
}

// slots 0 .. 13: what the episodes that ended gave
DEV void ep_store_episodes(double* __restrict__ p, const EpStat s) {
  p[0] = s.ret.n;
  p[1] = s.ret.mean;
  p[2] = s.ret.m2;
  p[3] = s.mn;
  p[4] = s.mx;
  p[5] = s.len_sum;
  p[6] = s.len_max;
#pragma unroll
  for (int c = 0; c <= EP_CAUSES; ++c) p[7 + c] = s.cause[c];
}

template <bool SEATS>
__global__ __launch_bounds__(WAVE) void k_rollout_episodes_scan(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                                const uint32_t* __restrict__ flags, const int T, const int rows,
                                                                float* __restrict__ ret_carry, int32_t* __restrict__ len_carry,
                                                                float* __restrict__ ep_return, int32_t* __restrict__ ep_length,
                                                                double* __restrict__ partial) {
#pragma clang fp reassociate(off)
#pragma clang fp contract(off)
  const int r = (int)blockIdx.x * WAVE + (int)threadIdx.x;
  const bool row_in = r < rows;
  const int rr = row_in ? r : rows - 1;  // (a lane behind the last row reads that row and contributes nothing: every lane reaches the shuffles)
  float R = ret_carry[rr];
  int32_t L = len_carry[rr];
  double K = 0.0, s1 = 0.0, s2 = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  int n = 0, steps = 0, len_max = 0;
  uint32_t len_sum = 0u;  // (the lengths of a row's episodes that end in one call sum to at most len_carry + T < 2^32)
  int cause[EP_CAUSES + 1];
#pragma unroll
  for (int c = 0; c <= EP_CAUSES; ++c) cause[c] = 0;
  for (int t0 = 0; t0 < T; t0 += EP_BATCH) {
    float rw[EP_BATCH];
    uint8_t dn[EP_BATCH];
    uint32_t fl[EP_BATCH];
#pragma unroll
    for (int j = 0; j < EP_BATCH; ++j) {
      const size_t i = (size_t)min(t0 + j, T - 1) * rows + rr;
      rw[j] = reward[i];
      dn[j] = done[i];
      fl[j] = flags[i];
    }
#pragma unroll
    for (int j = 0; j < EP_BATCH; ++j) {
      const bool step_in = row_in && t0 + j < T;
      const bool acted = step_in && (!SEATS || ro_acted(fl[j]));
      const bool ends = acted && (SEATS ? !ro_cont(fl[j], dn[j]) : dn[j] != 0);
      // (selections: the reward of a row that did not act may be NaN and reaches nothing)
      R = acted ? R + rw[j] : R;
      L += acted ? 1 : 0;
      steps += acted ? 1 : 0;
      const double x = (double)R;
      K = n == 0 ? x : K;
      const double dx = ends ? x - K : 0.0;  // (adding 0 leaves s1 and s2 their bits: one selection instead of two)
      s1 = s1 + dx;
      s2 = fma(dx, dx, s2);
      mn = fminf(mn, ends ? R : INFINITY);
      mx = fmaxf(mx, ends ? R : -INFINITY);
      n += ends ? 1 : 0;
      len_sum += ends ? (uint32_t)L : 0u;
      len_max = max(len_max, ends ? L : 0);
#pragma unroll
      for (int c = 0; c < EP_CAUSES; ++c) cause[c] += ends && ((fl[j] >> c) & 1u) ? 1 : 0;
      cause[EP_CAUSES] += ends && dn[j] == 0 ? 1 : 0;
      if (step_in) {
        const size_t i = (size_t)(t0 + j) * rows + r;
        if (ep_return) ep_return[i] = ends ? R : 0.0f;
        if (ep_length) ep_length[i] = ends ? L : 0;
      }
      R = ends ? 0.0f : R;
      L = ends ? 0 : L;
    }
  }
  if (row_in) {
    ret_carry[r] = R;
    len_carry[r] = L;
  }
  EpStat s = ep_empty();
  if (n > 0) {
    const double cnt = (double)n, q = s1 / cnt;
    s.ret.n = cnt;
    s.ret.mean = K + q;
    s.ret.m2 = fmax(s2 - s1 * q, 0.0);
    s.mn = (double)mn;
    s.mx = (double)mx;
  }
  s.len_sum = (double)len_sum;
  s.len_max = (double)len_max;
#pragma unroll
  for (int c = 0; c <= EP_CAUSES; ++c) s.cause[c] = (double)cause[c];
  s.steps = (double)steps;
  s = ep_wave_merge(s);
  if (threadIdx.x == 0) {
    double* p = partial + EP_RECORD * (size_t)blockIdx.x;
    ep_store_episodes(p, s);
    p[14] = s.steps;
    p[15] = 0.0;
  }
}

// record: _abi.ROLLOUT_EPISODES; `call` and `record` may each be null
__global__ __launch_bounds__(EP_THREADS) void k_rollout_episodes_merge(const double* __restrict__ partial, const int n_part,
                                                                       double* __restrict__ call, double* __restrict__ record) {
#pragma clang fp reassociate(off)
  __shared__ double wave_stat[EP_THREADS / WAVE][EP_RECORD];
  EpStat s = ep_empty();
  for (int i = (int)threadIdx.x; i < n_part; i += EP_THREADS) s = ep_merge(s, ep_load(partial + EP_RECORD * (size_t)i));
  s = ep_wave_merge(s);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    double* w = wave_stat[threadIdx.x / WAVE];
    ep_store_episodes(w, s);
    w[14] = s.steps;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < EP_THREADS / WAVE; ++k) s = ep_merge(s, ep_load(wave_stat[k]));
    if (call) {
      ep_store_episodes(call, s);
      call[14] = s.steps;
      call[15] = 1.0;
    }
    if (record) {
      if (s.ret.n > 0.0) {  // (a call in which no episode ended leaves slots 0 .. 13 their bytes)
        const EpStat rec = ep_merge(ep_load(record), s);
        ep_store_episodes(record, rec);
      }
      record[14] = record[14] + s.steps;
      record[15] = record[15] + 1.0;
    }
  }
}

static size_t ep_work_bytes(int rows) { return rows < 1 ? 0 : EP_RECORD * sizeof(double) * (size_t)((rows + WAVE - 1) / WAVE); }

extern "C" {

size_t pgd_rollout_episodes_work_bytes(int rows) { return ep_work_bytes(rows); }

int pgd_rollout_episodes(pgd_handle h, const float* d_reward, const uint8_t* d_done, const uint32_t* d_flags, int T, int rows, uint32_t mode,
                         float* d_ret_carry, int32_t* d_len_carry, double* d_record, double* d_call, float* d_ep_return, int32_t* d_ep_length,
                         void* d_work, size_t work_bytes) {
  if (!h || !d_reward || !d_done || !d_flags || !d_ret_carry || !d_len_carry || !d_work || T < 1 || rows < 1) return PGD_ERR_ARG;
  if ((mode & ~(uint32_t)PGD_EP_SEATS) != 0u) return PGD_ERR_ARG;
  if ((((uintptr_t)d_record | (uintptr_t)d_call | (uintptr_t)d_work) & 7u) != 0u || work_bytes < ep_work_bytes(rows)) return PGD_ERR_ARG;
  if ((((uintptr_t)d_reward | (uintptr_t)d_flags | (uintptr_t)d_ret_carry | (uintptr_t)d_len_carry | (uintptr_t)d_ep_return |
        (uintptr_t)d_ep_length) & 3u) != 0u)
    return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  const int n_part = (rows + WAVE - 1) / WAVE;
  double* partial = static_cast<double*>(d_work);
  if (mode & PGD_EP_SEATS)
    hipLaunchKernelGGL(k_rollout_episodes_scan<true>, dim3(n_part), dim3(WAVE), 0, h->stream, d_reward, d_done, d_flags, T, rows, d_ret_carry,
                       d_len_carry, d_ep_return, d_ep_length, partial);
  else
    hipLaunchKernelGGL(k_rollout_episodes_scan<false>, dim3(n_part), dim3(WAVE), 0, h->stream, d_reward, d_done, d_flags, T, rows, d_ret_carry,
                       d_len_carry, d_ep_return, d_ep_length, partial);
  if (d_record || d_call)  // (neither: the carries and the dense outputs alone)
    hipLaunchKernelGGL(k_rollout_episodes_merge, dim3(1), dim3(EP_THREADS), 0, h->stream, partial, n_part, d_call, d_record);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

}  // extern "C"

#endif
