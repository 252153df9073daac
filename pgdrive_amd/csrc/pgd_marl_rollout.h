// pgd_marl_rollout.h -- PPO rollouts of MULTI-AGENT engines on the device: which seat rows hold an agent, the networks over those rows
// only, and GAE that knows where one agent's episode ends and the next one's begins in the same seat.
// Part of the single translation unit pgd_engine.hip (included behind pgd_kernels.h; it uses pgd_policy.h's layer code and
// pgd_actor_critic.h's head constants).  No reference counterpart: the reference hands dicts keyed by agent name to an RL library, which
// batches the agents that are present (multi_agent_pgdrive.py:109-213); here the seats are rows of fixed arrays and the flags of
// pgd_step say which of them count.
//
// The predicates (include/pgdrive_hip.h restates them), for seat row r and step t, f = flags[t][r], d = done[t][r]:
//   acted = f & PGD_F_REPORT                       an agent held the seat and acted in step t
//   cont  = acted && !d && !(f & PGD_F_RESET)      the same agent holds the seat after the step
//   live  = (f & PGD_F_NEW) || cont                row t + 1 of the seat holds an observation an agent will act on
//
// Ordered compaction (k_compact<PRED, SCATTER>, k_compact_scan): the ascending list of the indices at which a predicate holds, and their
// number, in three launches and without one workgroup waiting for another:
//   1. k_compact<PRED, false>  a workgroup of 256 threads takes CMP_BLOCK = 1024 consecutive indices in four chunks of 256 (thread i takes
//                              index 256 c + i of chunk c), a ballot and a popcount per wave and chunk; the workgroup's number -> counts[b]
//   2. k_compact_scan          ONE workgroup turns counts[] into exclusive offsets in place, CMP_THREADS entries per pass with the running
//                              sum carried from pass to pass, and writes the total to *count
//   3. k_compact<PRED, true>   the same ballots again; entry offsets[b] + (hits of the chunks and waves before mine) + (hits of the lower
//                              lanes of my wave) = my index
// The order is that of the indices by construction: no atomics, and the same input gives the same bytes.  Entries at and beyond *count
// are not written.  counts[] is the engine's scratch (allocated outside any graph capture).
//
// k_mlp_actor_critic_rows: k_mlp_actor_critic over a row list.  Tile j takes list entries 16 j .. 16 j + 15; the row prologue gathers
// their observation rows (each row still contiguous: a wave reads whole rows); outputs go to the rows' own places; the noise is that of
// the TRUE row (g = row_base + row), so a listed row gets bit for bit what k_mlp_actor_critic gives it -- a row's arithmetic never
// depended on its tile neighbours.  The host does not know the list's length: the grid is sized for every row, and a workgroup whose
// tile starts at or beyond *count returns before it reads a weight.  An entry outside [row_lo, row_lo + n_rows) is skipped, never
// followed.  k_ac_clear_rows, launched in front of it by pgd_mlp_actor_critic_rows, gives the rows that are NOT listed their defined
// outputs: action 0, 0, logp 0, value 0.  (The prologue is the shared loader, mlp_load_rows, with an index; the noise draw and the sample's write are ac_tile's functions.)
//
// k_gae_masked: k_gae with the predicates; a row that did not act is written by SELECTION (its reward and value may be NaN).
#ifndef PGD_MARL_ROLLOUT_H
#define PGD_MARL_ROLLOUT_H

#define CMP_THREADS 256
#define CMP_CHUNKS 4
#define CMP_BLOCK (CMP_THREADS * CMP_CHUNKS)
#define CMP_LIVE 0   // predicate `live` over flags[i], done[i]
#define CMP_ACTED 1  // predicate `acted` over flags[i]

DEV bool ro_acted(const uint32_t f) { return (f & PGD_F_REPORT) != 0u; }
DEV bool ro_cont(const uint32_t f, const uint8_t d) { return ro_acted(f) && d == 0 && !(f & PGD_F_RESET); }
DEV bool ro_live(const uint32_t f, const uint8_t d) { return (f & PGD_F_NEW) != 0u || ro_cont(f, d); }

// Indices first + [0, n): SCATTER false: counts[blockIdx.x] = the workgroup's hits; true: the hits' indices (first + i) into
// list[offsets[blockIdx.x] ...], ascending.  `done` is read by CMP_LIVE only.
template <int PRED, bool SCATTER>
__global__ __launch_bounds__(CMP_THREADS) void k_compact(const uint32_t* __restrict__ flags, const uint8_t* __restrict__ done, const int first,
                                                         const int n, uint32_t* __restrict__ counts, int32_t* __restrict__ list) {
  __shared__ uint32_t wave_hits[CMP_CHUNKS * (CMP_THREADS / WAVE)];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int base = (int)blockIdx.x * CMP_BLOCK;  // (relative to first)
  bool hit[CMP_CHUNKS];
  uint32_t below[CMP_CHUNKS];
#pragma unroll
  for (int c = 0; c < CMP_CHUNKS; ++c) {
    const int i = base + c * CMP_THREADS + tid;
    hit[c] = false;
    if (i < n) {
      const uint32_t f = flags[(size_t)first + i];
      hit[c] = PRED == CMP_LIVE ? ro_live(f, done[(size_t)first + i]) : ro_acted(f);
    }
    const unsigned long long m = __ballot(hit[c]);
    below[c] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_hits[c * (CMP_THREADS / WAVE) + wave] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (!SCATTER) {
    if (tid == 0) {
      uint32_t s = 0;
#pragma unroll
      for (int k = 0; k < CMP_CHUNKS * (CMP_THREADS / WAVE); ++k) s += wave_hits[k];
      counts[blockIdx.x] = s;
    }
    return;
  }
  uint32_t at = counts[blockIdx.x];  // (exclusive offsets by now)
#pragma unroll
  for (int c = 0; c < CMP_CHUNKS; ++c) {
#pragma unroll
    for (int w = 0; w < CMP_THREADS / WAVE; ++w) {
      const uint32_t hits = wave_hits[c * (CMP_THREADS / WAVE) + w];
      if (w == wave && hit[c]) list[(size_t)at + below[c]] = first + base + c * CMP_THREADS + tid;
      at += hits;
    }
  }
}

// counts[0 .. n_blocks) -> their exclusive prefix sums in place, the total -> *count.  One workgroup; CMP_THREADS entries per pass.
__global__ __launch_bounds__(CMP_THREADS) void k_compact_scan(uint32_t* __restrict__ counts, const int n_blocks, int32_t* __restrict__ count) {
  __shared__ uint32_t wave_sum[CMP_THREADS / WAVE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  uint32_t carry = 0;
  for (int b0 = 0; b0 < n_blocks; b0 += CMP_THREADS) {
    const int b = b0 + tid;
    const uint32_t v = b < n_blocks ? counts[b] : 0u;
    uint32_t s = v;  // inclusive sum within the wave
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const uint32_t o = __shfl_up(s, d);
      if (lane >= d) s += o;
    }
    if (lane == WAVE - 1) wave_sum[wave] = s;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < CMP_THREADS / WAVE; ++w) {
      const uint32_t ws = wave_sum[w];
      if (w < wave) before += ws;
      total += ws;
    }
    if (b < n_blocks) counts[b] = carry + before + s - v;
    carry += total;
    __syncthreads();  // (wave_sum is rewritten by the next pass)
  }
  if (tid == 0) *count = (int32_t)carry;
}

// rows [row_lo, row_lo + n_rows): action 0, 0, logp 0 and (value non-null) value 0
__global__ __launch_bounds__(CMP_THREADS) void k_ac_clear_rows(const int row_lo, const int n_rows, float* __restrict__ act, float* __restrict__ logp,
                                                               float* __restrict__ value) {
  const int r = (int)blockIdx.x * CMP_THREADS + (int)threadIdx.x;
  if (r >= n_rows) return;
  const size_t row = (size_t)row_lo + r;
  act[row * 2 + 0] = 0.0f;
  act[row * 2 + 1] = 0.0f;
  logp[row] = 0.0f;
  if (value) value[row] = 0.0f;
}

// list[i] for i < n when it names a row of [row_lo, row_lo + n_rows), else -1
DEV int ro_listed_row(const int32_t* list, const int i, const int n, const int row_lo, const int n_rows) {
  if (i >= n) return -1;
  const int row = list[i];
  return (row >= row_lo && row - row_lo < n_rows) ? row : -1;
}

// slot r holds the observation row list[l0 + r]; for entries past n and rows outside the range row row_lo stands in: the observation of a
// row that is not listed is never USED -- it may hold NaN -- but row_lo's may be read
template <bool NORM>
DEV void ro_load_rows(const float* obs, const int32_t* list, const int l0, const int n, const int row_lo, const int n_rows, const int obs_stride,
                      const int in_dim, const int kp, const int xs, const int wave, const int lane, float* X, const ObsNorm nm) {
  mlp_load_rows<NORM>(in_dim, kp, xs, wave, lane, X, nm, [&](const int r, bool& in) {
    const int row = ro_listed_row(list, l0 + r, n, row_lo, n_rows);
    in = row >= 0;
    return obs + (size_t)(in ? row : row_lo) * obs_stride;
  });
}

// the rows list[0 .. *count) of `obs`, each within [row_lo, row_lo + n_rows) -> act[row][0..1], logp[row] (blockIdx.y == 0) and
// value[row] (blockIdx.y == 1).  Everything behind the prologue is k_mlp_actor_critic's.
template <bool NORM>
__global__ __launch_bounds__(WAVE * MLP_WAVES, 4) void k_mlp_actor_critic_rows(const float* __restrict__ obs, const int32_t* __restrict__ list,
                                                                            const int32_t* __restrict__ count, const int row_lo, const int n_rows,
                                                                            const int obs_stride, const int in_dim, const pgd_actor_critic nets,
                                                                            const uint32_t seed, const uint32_t tick_arg,
                                                                            const uint32_t* __restrict__ tick_dev, const uint32_t row_base,
                                                                            const uint32_t flags, float* __restrict__ act, float* __restrict__ logp,
                                                                            float* __restrict__ value, const ObsNorm nm) {
  extern __shared__ float mlp_lds[];
  const int l0 = (int)blockIdx.x * MLP_ROWS;  // (the tile's first list entry)
  const int n = min(*count, n_rows);
  if (l0 >= n) return;  // (before any weight is read: most workgroups of a sparsely occupied engine end here)
  const bool critic = blockIdx.y != 0;
  const float* __restrict__ W1 = critic ? nets.vw1 : nets.w1;
  const float* __restrict__ b1 = critic ? nets.vb1 : nets.b1;
  const float* __restrict__ W2 = critic ? nets.vw2 : nets.w2;
  const float* __restrict__ b2 = critic ? nets.vb2 : nets.b2;
  const float* __restrict__ W3 = critic ? nets.vw3 : nets.w3;
  const float* __restrict__ b3 = critic ? nets.vb3 : nets.b3;
  const int kp = (in_dim + 3) & ~3, xs = mlp_x_stride(in_dim);
  float* X = mlp_lds;
  float* H1 = X + MLP_ROWS * xs;
  float* H2 = H1 + MLP_ROWS * MLP_HS;
  float* W3s = H2 + MLP_ROWS * MLP_HS;  // [4][256]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int heads = critic ? 1 : AC_HEAD, w3_ld = critic ? 1 : nets.out_cols;
  float w3v[AC_HEAD];
#pragma unroll
  for (int q = 0; q < AC_HEAD; ++q) {
    const int idx = tid + q * WAVE * MLP_WAVES;
    const int k = critic ? idx : idx >> 2, o = critic ? 0 : idx & 3;
    w3v[q] = q < heads ? W3[(size_t)k * w3_ld + o] : 0.0f;
  }
  ro_load_rows<NORM>(obs, list, l0, n, row_lo, n_rows, obs_stride, in_dim, kp, xs, wave, lane, X, nm);
#pragma unroll
  for (int q = 0; q < AC_HEAD; ++q) {
    const int idx = tid + q * WAVE * MLP_WAVES;
    const int k = critic ? idx : idx >> 2, o = critic ? 0 : idx & 3;
    if (q < heads) W3s[o * MLP_H + k] = w3v[q];
  }
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
  if (critic) {  // 16 dot products of 256, sixteen lanes each
    const int r = tid >> 4, part = tid & 15;
    float s = 0.0f;
#pragma unroll 4
    for (int k = part; k < MLP_H; k += 16) s = fmaf(H2[r * MLP_HS + k], W3s[k], s);
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    const int row = ro_listed_row(list, l0 + r, n, row_lo, n_rows);
    if (part == 0 && row >= 0) value[(size_t)row] = s + b3[0];
    return;
  }
  // 16 rows x 4 outputs = 64 dot products of 256, four lanes each; the sixteen lanes of a row sit in one wave
  const int r = tid >> 4, o = (tid >> 2) & 3, part = tid & 3;
  float s = 0.0f;
#pragma unroll 4
  for (int k = part; k < MLP_H; k += 4) s = fmaf(H2[r * MLP_HS + k], W3s[o * MLP_H + k], s);
  s += __shfl_xor(s, 2);
  s += __shfl_xor(s, 1);
  const float v = s + b3[o];
  const int l16 = lane & ~15;
  const float m0 = __shfl(v, l16), m1 = __shfl(v, l16 + 4), ls0 = __shfl(v, l16 + 8), ls1 = __shfl(v, l16 + 12);
  const int row = ro_listed_row(list, l0 + r, n, row_lo, n_rows);
  if ((lane & 15) == 0 && row >= 0) {
    float z0 = 0.0f, z1 = 0.0f;
    if (!(flags & PGD_AC_DETERMINISTIC)) ac_noise(seed, tick_arg + (tick_dev ? *tick_dev : 0u), row_base + (uint32_t)row, z0, z1);
    ac_write_sample(row, m0, m1, ls0, ls1, z0, z1, act, logp);
  }
}

// k_gae for seats that change hands (pgd_gae_masked in include/pgdrive_hip.h states the recursion): one thread per seat row, t from
// T - 1 down to 0.  What a row that did not act, or an agent that does not continue, would contribute is SELECTED away, not multiplied by
// zero: those rewards and values may be NaN.  With every flag PGD_F_REPORT and no PGD_F_RESET the bits are k_gae's.
__global__ __launch_bounds__(WAVE) void k_gae_masked(const float* __restrict__ reward, const float* __restrict__ value, const uint8_t* __restrict__ done,
                                                     const uint32_t* __restrict__ flags, const int T, const int rows, const float gamma,
                                                     const float lam, float* __restrict__ adv, float* __restrict__ ret, uint8_t* __restrict__ mask) {
  const int r = (int)blockIdx.x * WAVE + (int)threadIdx.x;
  if (r >= rows) return;
  const float gl = gamma * lam;
  float a = 0.0f, vn = value[(size_t)T * rows + r];
#pragma unroll 4
  for (int t = T - 1; t >= 0; --t) {
    const size_t i = (size_t)t * rows + r;
    const uint32_t f = flags[i];
    const bool acted = ro_acted(f), cont = ro_cont(f, done[i]);
    const float v = value[i];
    const float delta = fmaf(gamma, cont ? vn : 0.0f, reward[i]) - v;
    a = acted ? fmaf(gl, cont ? a : 0.0f, delta) : 0.0f;
    adv[i] = a;
    ret[i] = acted ? a + v : 0.0f;
    mask[i] = acted ? 1 : 0;
    vn = v;
  }
}

#endif
