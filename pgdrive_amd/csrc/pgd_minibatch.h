// pgd_minibatch.h -- what the PPO update needs around pgd_ppo_grad to draw random minibatches and to stop early without a host read:
// a keyed permutation of a row list (pgd_shuffle_index) and the Adam pair behind a device-side gate (pgd_adam_gated).
// include/pgdrive_hip.h states the contracts.  Part of the single translation unit pgd_engine.hip (included at its end, behind pgd_ppo.h,
// whose ppo_count, ppo_block_sum and PPO_BATCH it uses; no kernel of that header is touched).  No reference counterpart: the reference
// hands its arrays to an RL library, whose trainer shuffles on the host (np.random.permutation per epoch) and reads the KL there.
//
// The permutation is computed per ENTRY, not built: position q of the output is pi(q), a 6-round unbalanced Feistel network on the
// b = max(2, bit_length(c - 1)) bits that hold the live count c, walked until it lands below c (cycle walking: x runs through the cycle
// of the 2^b-permutation that contains q, so the walk ends and pi is a bijection of [0, c); a cap on the walk would break it).  The
// round function is the counter hash pgd_rng keyed by (seed, round, epoch): integers only, so tests/minibatch_ref.py restates it exactly.
// No atomics, no scratch, no sort, no shuffle tensor of random keys: one thread per entry reads the count and the epoch on the device.
#ifndef PGD_MINIBATCH_H
#define PGD_MINIBATCH_H

#define SHUF_KEY 0x5b0ff1e5u  // the stream of the minibatch permutations (no other pgd_rng stream uses it)
#define SHUF_ROUNDS 6         // four rounds leave the (position, value) table 2 - 2.5 sigma off uniform at c = 37: DESIGN 29

// pi(q) for q < c, c >= 1
DEV uint32_t shuf_pi(const uint32_t q, const uint32_t c, const uint32_t seed, const uint32_t e) {
  const int bits = c > 1u ? 32 - __clz((int)(c - 1u)) : 0;
  const int b = bits < 2 ? 2 : bits;
  const int bl = b >> 1, br = b - bl;
  uint32_t x = q;
  do {
    uint32_t L = x >> br, R = x & ((1u << br) - 1u);
    int lb = bl, rb = br;
#pragma unroll
    for (uint32_t r = 0; r < SHUF_ROUNDS; ++r) {
      const uint32_t f = pgd_rng(seed ^ SHUF_KEY, R, r, e) & ((1u << lb) - 1u);
      const uint32_t nr = L ^ f;
      L = R;
      R = nr;
      const int sw = lb;
      lb = rb;
      rb = sw;
    }
    x = (L << rb) | R;
  } while (x >= c);
  return x;
}

__global__ __launch_bounds__(256) void k_shuffle_index(const int32_t* __restrict__ index, const int32_t* __restrict__ count, const int n_list,
                                                       const uint32_t seed, const uint32_t epoch, const int32_t* __restrict__ d_epoch,
                                                       int32_t* __restrict__ out) {
  const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
  const int c = ppo_count(count, n_list);
  if (q >= c) return;  // (entries at and beyond the count are not written)
  const uint32_t e = epoch + (d_epoch ? (uint32_t)*d_epoch : 0u);
  const int p = (int)shuf_pi((uint32_t)q, (uint32_t)c, seed, e);  // (p < c <= n_list: inside index)
  out[q] = index ? index[p] : p;
}

// ---- pgd_adam_gated: k_adam_prep / k_adam behind gate[4] = (stopped, applied, skipped, this call skipped) -------------------------------
// ONE workgroup, as k_adam_prep.  Thread 0 decides; a gate that is already shut lets the workgroup leave before the |g|^2 pass.
DEV void adam_gate_skip(int32_t* gate, int32_t* count_gate) {
  gate[0] = 1;
  gate[2] += 1;
  gate[3] = 1;
  if (count_gate) *count_gate = 0;
}

__global__ __launch_bounds__(256) void k_adam_gated_prep(const float* __restrict__ grad, const int n_elem, const float beta1, const float beta2,
                                                         const float max_norm, int32_t* __restrict__ rec, const float* __restrict__ kl,
                                                         const float kl_limit, int32_t* __restrict__ gate, int32_t* __restrict__ count_gate) {
  __shared__ float wave_sum[4];
  __shared__ int shut;
  if (threadIdx.x == 0) shut = gate[0] != 0;  // (read once: thread 0 writes gate[0] below)
  __syncthreads();
  if (shut) {
    if (threadIdx.x == 0) adam_gate_skip(gate, count_gate);
    return;
  }
  float s = 0.0f;
  if (max_norm > 0.0f)
    for (int i0 = threadIdx.x; i0 < n_elem; i0 += 256 * PPO_BATCH) {
      float x[PPO_BATCH];
#pragma unroll
      for (int j = 0; j < PPO_BATCH; ++j) {
        const int i = i0 + 256 * j;
        x[j] = i < n_elem ? grad[i] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < PPO_BATCH; ++j) s = fmaf(x[j], x[j], s);
    }
  s = ppo_block_sum(s, wave_sum);
  if (threadIdx.x == 0) {
    if (kl && !(*kl <= kl_limit)) {  // (a NaN stops)
      adam_gate_skip(gate, count_gate);
      return;
    }
    gate[1] += 1;
    gate[3] = 0;
    const int t = rec[0] + 1;
    rec[0] = t;
    float* f = reinterpret_cast<float*>(rec);
    f[1] = max_norm > 0.0f ? fminf(1.0f, (float)((double)max_norm / (sqrt((double)s) + 1e-6))) : 1.0f;
    f[2] = (float)(1.0 / (1.0 - pow((double)beta1, (double)t)));
    f[3] = (float)(1.0 / (1.0 - pow((double)beta2, (double)t)));
  }
}

__global__ __launch_bounds__(256) void k_adam_gated(float* __restrict__ param, const float* __restrict__ grad, float* __restrict__ m,
                                                    float* __restrict__ v, const int n_elem, const float lr, const float beta1, const float beta2,
                                                    const float eps, const int32_t* __restrict__ rec, const float* __restrict__ lr_scale,
                                                    const int32_t* __restrict__ gate) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= n_elem || gate[3] != 0) return;  // (a skipped call leaves param, m and v as they are)
  const float lr_eff = lr_scale ? lr * lr_scale[0] : lr;  // (one fp32 product, before the double quotient)
  const float* f = reinterpret_cast<const float*>(rec);
  const float g = grad[i] * f[1];
  const float mi = fmaf(beta1, m[i], (1.0f - beta1) * g);
  const float vi = fmaf(beta2, v[i], (1.0f - beta2) * g * g);
  m[i] = mi;
  v[i] = vi;
  param[i] = (float)((double)param[i] - (double)lr_eff * ((double)mi * (double)f[2]) / (sqrt((double)vi * (double)f[3]) + (double)eps));
}

extern "C" {

int pgd_shuffle_index(pgd_handle h, const int32_t* d_index, const int32_t* d_count, int n_list, uint32_t seed, uint32_t epoch,
                      const int32_t* d_epoch, int32_t* d_out) {
  if (!h || !d_out || n_list < 0 || n_list > PGD_PPO_ROWS_MAX || d_out == d_index) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  if (n_list == 0) return PGD_OK;
  hipLaunchKernelGGL(k_shuffle_index, dim3((n_list + 255) / 256), dim3(256), 0, h->stream, d_index, d_count, n_list, seed, epoch, d_epoch, d_out);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

int pgd_adam_gated(pgd_handle h, float* d_param, const float* d_grad, float* d_m, float* d_v, int n_elem, int32_t* d_step, float lr, float beta1,
                   float beta2, float eps, float max_grad_norm, const float* d_lr_scale, const float* d_kl, float kl_limit, int32_t* d_gate,
                   int32_t* d_count_gate) {
  if (!h || !d_param || !d_grad || !d_m || !d_v || !d_step || !d_gate || n_elem < 1) return PGD_ERR_ARG;
  if (!(beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f) || (reinterpret_cast<uintptr_t>(d_step) & 3u) != 0u ||
      (reinterpret_cast<uintptr_t>(d_gate) & 3u) != 0u)
    return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_adam_gated_prep, dim3(1), dim3(256), 0, h->stream, d_grad, n_elem, beta1, beta2, max_grad_norm, d_step, d_kl, kl_limit, d_gate,
                     d_count_gate);
  hipLaunchKernelGGL(k_adam_gated, dim3((n_elem + 255) / 256), dim3(256), 0, h->stream, d_param, d_grad, d_m, d_v, n_elem, lr, beta1, beta2, eps,
                     d_step, d_lr_scale, d_gate);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

}  // extern "C"

#endif
