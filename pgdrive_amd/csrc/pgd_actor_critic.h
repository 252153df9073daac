// pgd_actor_critic.h -- what a PPO rollout needs from its networks at every step, as ONE launch, and GAE behind the rollout.
// Part of the single translation unit pgd_engine.hip (included by pgd_step.h behind pgd_policy.h, whose layer code it uses).
//
// What it mirrors: pgdrive/examples/ppo_expert/numpy_expert.py:38-45 (`expert(obs, deterministic=False)`: the four outputs of fc_out are
//   mean, log_std = split(out, 2);  action = normal(mean, exp(log_std))
// ) and numpy_expert.py:62-78 (`value(obs)`: a second network of the same shape, fc_value_1 / fc_value_2 / value_out, one output).  A
// trainer evaluates both at every step and needs the log-probability of the sample for PPO's ratio: as framework ops two times three
// GEMMs, a randn and a handful of elementwise launches.  Here: k_mlp_actor_critic, grid (ceil(rows / 16), 2).  Workgroup (x, 0) is the
// actor for 16 observation rows, workgroup (x, 1) the critic for the same rows (their second read comes from L2); both are
// k_mlp_policy's workgroup -- 16-row tile, 4 waves, the same LDS strides, the same row prologue, mlp_layer / mlp_store_hidden /
// mlp_tanh -- with another head.  Two workgroups of 256 threads and at most 64 KB fit a CU side by side, so the critic runs NEXT to the
// actor, not behind it.  A null value network launches gridDim.y = 1.  The workgroup's code is ac_tile, which is handed the chosen
// network's pointers: k_mlp_actor_critic_cost (pgd_safe.h) calls it with a third network, the cost critic, at blockIdx.y = 2.
//
// LDS per workgroup: X tile | H1 | H2 | the head's weights [4][256] (the critic uses the first 256): 2 KB more than k_mlp_policy, hence
// the largest accepted in_dim is 416 (x stride 418), not 448 (x stride 450: 65,920 bytes); ac_lds_bytes is the formula.
//
// Actor head: four dot products of 256 per row (columns 0..3 of w3 / b3: mean0, mean1, log_std0, log_std1; columns at or beyond 4 are
// never read), four lanes each (lane p takes k = p, p + 4, ...), a butterfly sum.  Then, per row:
//   g  = (env_base + env) * A + agent                      the global row: ranks of a multi-GPU run draw different noise
//   r1 = pgd_rng(seed ^ AC_KEY_SEED, g, AC_KEY_STREAM, tick),  r2 = pgd_rng(seed ^ AC_KEY_SEED, g, AC_KEY_STREAM, tick ^ 0x80000000)
//   u  = ((r >> 9) + 0.5) * 2^-23                          23 bits: exact in f32, never 0 or 1 (with 24 bits the sum needs 25 bits of
//                                                          significand above 2^23, and the largest draw would round to u = 1)
//   R = sqrtf(-2 logf(u1)),  z0 = R cosf(2 pi u2),  z1 = R sinf(2 pi u2)        Box-Muller, the library functions (not __logf / __cosf)
//   action[i] = mean[i] + expf(log_std[i]) z[i]            unclipped: pgd_step clips (numpy_expert.py:44)
//   logp = -0.5 (z0^2 + z1^2) - log_std0 - log_std1 - log(2 pi)                 from z itself: (a - mean) / std would divide a rounding
//                                                                               error by std
// PGD_AC_DETERMINISTIC: z = 0 -- the action is the mean, logp the density at the mean.
// `tick`: the argument plus, when the engine has been given one (pgd_actor_critic_tick), a counter in device memory read by the kernel:
// a captured graph replays with the argument it was captured with, the counter is what advances between replays.
// Critic head: one dot product of 256 per row, sixteen lanes each, value[row] = sum + vb3[0].
//
// k_gae: one thread per row, a reverse scan over t (pgd_gae in include/pgdrive_hip.h states the recursion); arrays are time-major
// [T][rows], so the reads and writes of a wave are consecutive.
#ifndef PGD_ACTOR_CRITIC_H
#define PGD_ACTOR_CRITIC_H

#define AC_HEAD 4
#define AC_KEY_SEED 0xac7012c1u
#define AC_KEY_STREAM 0x5a3b1e0du

DEV_HOST size_t ac_lds_bytes(int in_dim) {  // X tile | H1 | H2 | the head's weights [4][256]
  return sizeof(float) * ((size_t)MLP_ROWS * ((size_t)mlp_x_stride(in_dim) + 2 * MLP_HS) + AC_HEAD * MLP_H);
}

// u in (0, 1) from the top 23 bits of a draw: exact in f32
DEV float ac_unit(const uint32_t r) { return ((float)(r >> 9) + 0.5f) * (1.0f / 8388608.0f); }

// pgd_obs_norm_bind (include/pgdrive_hip.h states the rule; pgd_obs_norm.h holds its moments): the table a bound launch normalises its
// observation rows with as it loads them, float [2][kp]: shift | scale.  NORM is a template parameter of every loader and of the kernels
// around them: the false instantiations are the code of before (nm is passed and never read), the host launches them while nothing is bound.
struct ObsNorm { const float* table; float clip; };

// y = clamp((x - shift) * scale, -clip, clip): one fp32 subtraction, one fp32 multiplication, never an fma
DEV float on_apply(const float x, const float shift, const float scale, const float clip) {
#pragma clang fp contract(off) reassociate(off)
  const float d = x - shift;
  const float y = d * scale;
  return fminf(fmaxf(y, -clip), clip);
}

// the lane's table entries of the fast loader path (columns lane + 64 j; a column past the end reads the last one and is never used):
// issued with the row reads, before the first LDS store
template <int XCH>
DEV void on_lane_table(const ObsNorm nm, const int in_dim, const int kp, const int lane, float (&sh)[XCH], float (&sc)[XCH]) {
#pragma unroll
  for (int j = 0; j < XCH; ++j) {
    const int k = lane + WAVE * j, kk = k < in_dim ? k : in_dim - 1;
    sh[j] = nm.table[kk];
    sc[j] = nm.table[kp + kk];
  }
}

// k_mlp_policy's row prologue as a function (that kernel keeps its own copy inline: its code object stays what it was), shared by every
// other network kernel.  The 16 observation rows of a workgroup into its X tile (row stride xs); wave w takes slots w, w + 4, ...
// `row_of(slot, in)` says what a slot holds: it sets `in` and returns the slot's source row, for an empty slot (in false) a row that may be
// READ in its place and is never used.  Whole rows, coalesced (a row is contiguous in memory); padding columns and empty slots read zero.
// Every read of the wave's four rows goes out before the first LDS store (rows of up to 320 floats: five chunks of 64 per row) --
// as a read-then-store loop the prologue was twenty memory round trips in a row, a third of the launch (round 6).
// NORM: the live entries are normalised on their way (on_apply); padding columns and empty slots stay exactly 0
template <bool NORM, class RowOf>
DEV void mlp_load_rows(const int in_dim, const int kp, const int xs, const int wave, const int lane, float* X, const ObsNorm nm, const RowOf row_of) {
  constexpr int XCH = 5;
  if (kp <= WAVE * XCH) {
    float v[MLP_ROWS / MLP_WAVES][XCH], sh[XCH], sc[XCH];
    bool live[MLP_ROWS / MLP_WAVES];
    if (NORM) on_lane_table(nm, in_dim, kp, lane, sh, sc);
#pragma unroll
    for (int i = 0; i < MLP_ROWS / MLP_WAVES; ++i) {
      bool row_in;
      const float* src = row_of(wave + i * MLP_WAVES, row_in);
      live[i] = row_in;
#pragma unroll
      for (int j = 0; j < XCH; ++j) {
        const int k = lane + WAVE * j;
        v[i][j] = src[k < in_dim ? k : in_dim - 1];
        if (!(row_in && k < in_dim)) v[i][j] = 0.0f;
      }
    }
#pragma unroll
    for (int i = 0; i < MLP_ROWS / MLP_WAVES; ++i)
#pragma unroll
      for (int j = 0; j < XCH; ++j) {
        const int k = lane + WAVE * j;
        if (NORM) v[i][j] = (live[i] && k < in_dim) ? on_apply(v[i][j], sh[j], sc[j], nm.clip) : 0.0f;
        if (k < kp) X[(wave + i * MLP_WAVES) * xs + k] = v[i][j];
      }
  } else
  for (int r = wave; r < MLP_ROWS; r += MLP_WAVES) {
    bool row_in;
    const float* src = row_of(r, row_in);
    for (int k = lane; k < kp; k += WAVE) {
      if (NORM) X[r * xs + k] = (row_in && k < in_dim) ? on_apply(src[k], nm.table[k], nm.table[kp + k], nm.clip) : 0.0f;
      else X[r * xs + k] = (row_in && k < in_dim) ? src[k] : 0.0f;
    }
  }
}

// slot r holds row row0 + r0 + r of `obs` as far as it lies below row0 + n_rows; the tile's first row stands in for the rows past the end
template <bool NORM>
DEV void ac_load_rows(const float* obs, const int row0, const int r0, const int n_rows, const int obs_stride, const int in_dim, const int kp,
                       const int xs, const int wave, const int lane, float* X, const ObsNorm nm) {
  mlp_load_rows<NORM>(in_dim, kp, xs, wave, lane, X, nm, [&](const int r, bool& in) {
    in = r0 + r < n_rows;
    return obs + (size_t)(row0 + r0 + (in ? r : 0)) * obs_stride;
  });
}

// the two standard normal draws of global row g at this launch's tick (Box-Muller: the header states it)
DEV void ac_noise(const uint32_t seed, const uint32_t tick, const uint32_t g, float& z0, float& z1) {
  const float u1 = ac_unit(pgd_rng(seed ^ AC_KEY_SEED, g, AC_KEY_STREAM, tick));
  const float u2 = ac_unit(pgd_rng(seed ^ AC_KEY_SEED, g, AC_KEY_STREAM, tick ^ 0x80000000u));
  const float R = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincosf(2.0f * PGD_PI * u2, &sn, &cs);
  z0 = R * cs;
  z1 = R * sn;
}

// the sample and its log-probability of `row` from the four head outputs and the draws
DEV void ac_write_sample(const int row, const float m0, const float m1, const float ls0, const float ls1, const float z0, const float z1,
                         float* act, float* logp) {
  act[(size_t)row * 2 + 0] = fmaf(expf(ls0), z0, m0);
  act[(size_t)row * 2 + 1] = fmaf(expf(ls1), z1, m1);
  logp[row] = fmaf(-0.5f, fmaf(z0, z0, z1 * z1), -ls0 - ls1) - 1.8378770664093453f;  // log(2 pi)
}

// One workgroup of k_mlp_actor_critic on the network (W1 .. b3): the actor (critic false: act, logp) or a critic (value) for the 16 rows
// row0 + blockIdx.x * 16 + [0, 16) of `obs`.  The kernels below and k_mlp_actor_critic_cost (pgd_safe.h) choose the network and call it.
template <bool NORM>
DEV void ac_tile(const float* obs, const int row0, const int n_rows, const int obs_stride, const int in_dim, const bool critic,
                 const float* W1, const float* b1, const float* W2, const float* b2,
                 const float* W3, const float* b3, const int out_cols, const uint32_t seed, const uint32_t tick_arg,
                 const uint32_t* tick_dev, const uint32_t row_base, const uint32_t flags, float* act,
                 float* logp, float* value, const ObsNorm nm) {
  extern __shared__ float mlp_lds[];
  const int kp = (in_dim + 3) & ~3, xs = mlp_x_stride(in_dim);
  float* X = mlp_lds;
  float* H1 = X + MLP_ROWS * xs;
  float* H2 = H1 + MLP_ROWS * MLP_HS;
  float* W3s = H2 + MLP_ROWS * MLP_HS;  // [4][256]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = (int)blockIdx.x * MLP_ROWS;  // (relative to row0)
  // the head's weights go to LDS with the observation rows, as in k_mlp_policy: actor 256 x 4 of w3 (its first four columns, index =
  // 4 k + o), critic the 256 of vw3 (index = k)
  const int heads = critic ? 1 : AC_HEAD, w3_ld = critic ? 1 : out_cols;
  float w3v[AC_HEAD];
#pragma unroll
  for (int q = 0; q < AC_HEAD; ++q) {
    const int idx = tid + q * WAVE * MLP_WAVES;
    const int k = critic ? idx : idx >> 2, o = critic ? 0 : idx & 3;
    w3v[q] = q < heads ? W3[(size_t)k * w3_ld + o] : 0.0f;
  }
  ac_load_rows<NORM>(obs, row0, r0, n_rows, obs_stride, in_dim, kp, xs, wave, lane, X, nm);
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
    if (part == 0 && r0 + r < n_rows) value[(size_t)(row0 + r0 + r)] = s + b3[0];
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
  const int l0 = lane & ~15;
  const float m0 = __shfl(v, l0), m1 = __shfl(v, l0 + 4), ls0 = __shfl(v, l0 + 8), ls1 = __shfl(v, l0 + 12);
  if ((lane & 15) == 0 && r0 + r < n_rows) {
    const int row = row0 + r0 + r;
    float z0 = 0.0f, z1 = 0.0f;
    if (!(flags & PGD_AC_DETERMINISTIC)) ac_noise(seed, tick_arg + (tick_dev ? *tick_dev : 0u), row_base + (uint32_t)row, z0, z1);
    ac_write_sample(row, m0, m1, ls0, ls1, z0, z1, act, logp);
  }
}

// rows [row0, row0 + n_rows) of `obs` -> act[row][0..1], logp[row] (blockIdx.y == 0) and value[row] (blockIdx.y == 1)
template <bool NORM>
__global__ __launch_bounds__(WAVE * MLP_WAVES, 4) void k_mlp_actor_critic(const float* __restrict__ obs, const int row0, const int n_rows,
                                                                       const int obs_stride, const int in_dim, const pgd_actor_critic nets,
                                                                       const uint32_t seed, const uint32_t tick_arg,
                                                                       const uint32_t* __restrict__ tick_dev, const uint32_t row_base,
                                                                       const uint32_t flags, float* __restrict__ act, float* __restrict__ logp,
                                                                       float* __restrict__ value, const ObsNorm nm) {
  const bool critic = blockIdx.y != 0;
  ac_tile<NORM>(obs, row0, n_rows, obs_stride, in_dim, critic, critic ? nets.vw1 : nets.w1, critic ? nets.vb1 : nets.b1, critic ? nets.vw2 : nets.w2,
          critic ? nets.vb2 : nets.b2, critic ? nets.vw3 : nets.w3, critic ? nets.vb3 : nets.b3, nets.out_cols, seed, tick_arg, tick_dev, row_base,
          flags, act, logp, value, nm);
}

// adv[t][r] = delta + gamma lam nonterminal adv[t + 1][r], delta = reward[t][r] + gamma value[t + 1][r] nonterminal - value[t][r],
// ret = adv + value; nonterminal = 1 - done[t][r]; row r, t from T - 1 down to 0; reward_of(i) is the reward of entry i = t rows + r
template <class RewardOf>
DEV void gae_scan(const RewardOf reward_of, const float* value, const uint8_t* done, const int T, const int rows, const int r, const float gamma,
                  const float lam, float* adv, float* ret) {
  const float gl = gamma * lam;
  float a = 0.0f, vn = value[(size_t)T * rows + r];
#pragma unroll 4
  for (int t = T - 1; t >= 0; --t) {
    const size_t i = (size_t)t * rows + r;
    const float v = value[i], nt = done[i] ? 0.0f : 1.0f;
    const float delta = fmaf(gamma * nt, vn, reward_of(i)) - v;
    a = fmaf(gl * nt, a, delta);
    adv[i] = a;
    ret[i] = a + v;
    vn = v;
  }
}

// one thread per row
__global__ __launch_bounds__(WAVE) void k_gae(const float* __restrict__ reward, const float* __restrict__ value, const uint8_t* __restrict__ done,
                                              const int T, const int rows, const float gamma, const float lam, float* __restrict__ adv,
                                              float* __restrict__ ret) {
  const int r = (int)blockIdx.x * WAVE + (int)threadIdx.x;
  if (r >= rows) return;
  gae_scan([&](const size_t i) { return reward[i]; }, value, done, T, rows, r, gamma, lam, adv, ret);
}

#endif
