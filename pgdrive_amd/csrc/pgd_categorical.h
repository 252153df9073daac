// pgd_categorical.h -- a second policy head for the 256-256 tanh networks of the training path: TWO INDEPENDENT CATEGORICAL distributions,
// steering with ks bins and throttle with kt bins (SB3's MultiCategorical, the env's MultiDiscrete([discrete_steering_dim,
// discrete_throttle_dim])): the forward launch of a rollout (pgd_mlp_actor_critic_cat, _cat_rows) and the gradient of a minibatch
// (pgd_ppo_grad_cat).  include/pgdrive_hip.h states the formulas.
// Part of the single translation unit pgd_engine.hip, included behind pgd_safe.h: it uses pgd_policy.h's layer code, the loaders of
// pgd_actor_critic.h / pgd_marl_rollout.h / pgd_ppo.h and the host paths of the Gaussian family (ac_forward, nets_ok, grads_ok), and it
// touches no kernel of those headers -- every kernel here is its own symbol, the Gaussian kernels' code objects stay what they were
// (profiles/categorical_notes.md holds the disassembly comparison).  No reference counterpart: the reference hands a MultiDiscrete space
// to an RL library.
//
// The head.  K = ks + kt <= 16 logits per row: columns 0 .. ks - 1 of w3 / b3 steer, ks .. K - 1 throttle, columns at or beyond K are
// never read.  The 16 rows x 16 columns of a workgroup are ONE output tile of the f32 matrix cores (v_mfma_f32_16x16x4_f32, the
// instruction of mlp_layer): A = H2 from LDS, B = w3 read from global memory (16 KB at most, L2-resident), column min(c, K - 1) standing
// in for a padding column c >= K and its value replaced by zero.  The 256 k of the product are split over the four waves -- wave w takes
// k = 64 w .. 64 w + 63, 16 matrix instructions, every read issued in front of the first -- and the four partial tiles meet in LDS:
// logit = ((P0 + P1) + P2) + P3 + b3, in that order.  The partial tiles [4][16][16] lie in the 4 KB behind H2 that the Gaussian actor
// fills with its head's weights: the categorical actor stages NO head weights, so the workgroup's LDS is ac_lds_bytes, the Gaussian
// launch's own, and every in_dim up to 416 is served.  (Why the matrix cores and not the vector ALU with w3 streamed: a dot product per
// thread is 256 dependent fma with 256 reads each from global memory and LDS; the tile is 16 reads of either per lane.)
// The critic's workgroup (blockIdx.y = 1) is k_mlp_actor_critic's: the same loader, layers and head arithmetic, so `value` is its bits.
//
// Behind the logits the sixteen lanes (row r, column o) of a row each own logit o.  Every reduction over a head -- the maximum, the sum
// of the exponentials, the running sum of the probabilities, the entropy -- is a loop over the head's columns IN INDEX ORDER that every
// lane of the row runs on values fetched by __shfl: the numbers are those of one lane doing all of it, a row never sees its tile
// neighbours, and a lane computes one exponential instead of K.  The forward kernel does this in fp32 (expf, logf: under the build's
// flags their approximate v_exp_f32 / v_log_f32 forms); the gradient kernel in double from the fp32 logits (p_j as e_j / sum e, one exp
// per lane), rounded to fp32 once, as pgd_ppo_grad's row lane does.
#ifndef PGD_CATEGORICAL_H
#define PGD_CATEGORICAL_H

#define CAT_COLS 16      // the head's tile: K = ks + kt <= 16
#define PPO_CAT_TS 24    // floats per tile-sum record: 0 L_pi, 1 H, 2 logp_old - logp, 3 cut, 4 r, 5..20 dOut (actor); 21 L_v, 22 dv (critic)

DEV_HOST bool cat_bins_ok(int ks, int kt) { return ks >= 2 && kt >= 2 && ks + kt <= CAT_COLS; }

// The logit tile of the workgroup's 16 rows (the header): -> thread (r = tid >> 4, o = tid & 15) holds logit o of row r; columns o >= K
// hold 0.  P: 1024 floats of LDS.  Ends behind a barrier: P may be rewritten.
DEV float cat_logits(const float* H2, const float* __restrict__ W3, const float* __restrict__ b3, const int out_cols, const int K, const int tid,
                     float* P) {
#pragma clang fp contract(off) reassociate(off)
  const int wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, kq = lane >> 4;
  const bool in = col < K;
  const float* ap = H2 + col * MLP_HS + wave * 64 + kq;  // A fragment: row lane & 15, k = k0 + (lane >> 4)
  const float* wp = W3 + (size_t)(wave * 64 + kq) * out_cols + (in ? col : K - 1);  // B fragment: k = k0 + (lane >> 4), column lane & 15
  float a[16], w[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    a[j] = ap[4 * j];
    const float v = wp[(size_t)(4 * j) * out_cols];
    w[j] = in ? v : 0.0f;
  }
  mlp_f32x4 acc = mlp_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < 16; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], w[j], acc, 0, 0, 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) P[wave * 256 + (4 * kq + i) * 16 + col] = acc[i];  // C: register i of lane l -> row 4 (l >> 4) + i, column l & 15
  __syncthreads();
  const int e = tid & 255, o = tid & 15;
  const float s = ((P[e] + P[256 + e]) + P[512 + e]) + P[768 + e];
  const float l = o < K ? s + b3[o] : 0.0f;
  __syncthreads();
  return l;
}

// which columns of the tile are lane o's head: [j0, j1); a padding lane (o >= K) counts as throttle and reaches no output
struct CatLane { int j0, j1; };
DEV CatLane cat_lane(const int o, const int ks, const int kt) { return o < ks ? CatLane{0, ks} : CatLane{ks, ks + kt}; }

// One row of the forward launch, on its sixteen lanes (l16: the first of them; l: this lane's logit; u: this lane's HEAD's draw):
// -> this lane's head's index (relative to the head) and the log-probability of that index.  fp32, the header's order.
DEV void cat_sample(const float l, const int o, const int l16, const CatLane h, const float u, const bool deterministic, int& index, float& logp) {
#pragma clang fp contract(off) reassociate(off)
  float m = -INFINITY, best = -INFINITY;
  int bi = 0;
#pragma unroll
  for (int j = 0; j < CAT_COLS; ++j) {
    const float v = __shfl(l, l16 + j);
    const bool in = j >= h.j0 && j < h.j1;
    if (in) m = fmaxf(m, v);
    if (in && v > best) { best = v; bi = j - h.j0; }  // (the lowest index among equal logits)
  }
  const float e = expf(l - m);
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < CAT_COLS; ++j) {
    const float v = __shfl(e, l16 + j);
    if (j >= h.j0 && j < h.j1) s += v;
  }
  const float lse = m + logf(s);
  const float lp = l - lse, p = expf(lp);
  float c = 0.0f;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < CAT_COLS; ++j) {  // the number of j in [0, K_head - 1) with c_j <= u: never beyond K_head - 1
    const float v = __shfl(p, l16 + j);
    if (j >= h.j0 && j < h.j1 - 1) {
      c += v;
      cnt += c <= u ? 1 : 0;
    }
  }
  index = deterministic ? bi : cnt;
  logp = __shfl(lp, l16 + h.j0 + index);
}

// 2.0f / (float) (K_head - 1), correctly rounded: formed by the HOST and handed to the kernel (the device build's fp32 division is the
// 2.5 ulp form, and a double quotient of two small integers is narrowed to it)
static float cat_step(int k_head) { return (float)(2.0 / (double)(k_head - 1)); }
// the grid value of pgd_step's discrete conversion: one fp32 multiplication, THEN one fp32 subtraction.  The product passes through an
// empty asm statement: the build contracts a product and a sum into an fma wherever it sees both, pragma or not
DEV float cat_grid(const float index, const float step) {
#pragma clang fp contract(off) reassociate(off)
  float prod = index * step;
  asm volatile("" : "+v"(prod));
  return prod - 1.0f;
}

// rows of `obs` -> act[row][0..1], idx[row][0..1], logp[row] (blockIdx.y == 0) and value[row] (blockIdx.y == 1).  LIST false: the rows
// [row0, row0 + n_rows) (k_mlp_actor_critic's form; list, count null); true: the rows list[0 .. *count) within that range
// (k_mlp_actor_critic_rows' form).
template <bool NORM, bool LIST>
__global__ __launch_bounds__(WAVE * MLP_WAVES, 4) void k_mlp_actor_critic_cat(const float* __restrict__ obs, const int32_t* __restrict__ list,
                                                                           const int32_t* __restrict__ count, const int row0, const int n_rows,
                                                                           const int obs_stride, const int in_dim, const pgd_actor_critic nets,
                                                                           const int ks, const int kt, const float step_s, const float step_t,
                                                                           const uint32_t seed, const uint32_t tick_arg,
                                                                           const uint32_t* __restrict__ tick_dev, const uint32_t row_base,
                                                                           const uint32_t flags, float* __restrict__ act, int32_t* __restrict__ idx,
                                                                           float* __restrict__ logp, float* __restrict__ value, const ObsNorm nm) {
  extern __shared__ float mlp_lds[];
  const int t0 = (int)blockIdx.x * MLP_ROWS;  // the tile's first slot: a row relative to row0, or a list entry
  int n = n_rows;
  if (LIST) {
    n = min(*count, n_rows);
    if (t0 >= n) return;  // (before any weight is read)
  }
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
  float* W3s = H2 + MLP_ROWS * MLP_HS;  // the critic's 256 head weights; the actor's partial logit tiles [4][16][16]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float w3v = critic ? W3[tid] : 0.0f;
  if (LIST) ro_load_rows<NORM>(obs, list, t0, n, row0, n_rows, obs_stride, in_dim, kp, xs, wave, lane, X, nm);
  else ac_load_rows<NORM>(obs, row0, t0, n_rows, obs_stride, in_dim, kp, xs, wave, lane, X, nm);
  if (critic) W3s[tid] = w3v;
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
  const int r = tid >> 4, o = tid & 15;
  int row;  // the slot's row, -1: none
  if (LIST) row = ro_listed_row(list, t0 + r, n, row0, n_rows);
  else row = t0 + r < n_rows ? row0 + t0 + r : -1;
  if (critic) {  // 16 dot products of 256, sixteen lanes each: k_mlp_actor_critic's
    float s = 0.0f;
#pragma unroll 4
    for (int k = o; k < MLP_H; k += 16) s = fmaf(H2[r * MLP_HS + k], W3s[k], s);
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    if (o == 0 && row >= 0) value[(size_t)row] = s + b3[0];
    return;
  }
  const float l = cat_logits(H2, W3, b3, nets.out_cols, ks + kt, tid, W3s);
  const uint32_t tick = tick_arg + (tick_dev ? *tick_dev : 0u), g = row_base + (uint32_t)row;
  const float u_s = ac_unit(pgd_rng(seed ^ AC_KEY_SEED, g, AC_KEY_STREAM, tick));
  const float u_t = ac_unit(pgd_rng(seed ^ AC_KEY_SEED, g, AC_KEY_STREAM, tick ^ 0x80000000u));
  const CatLane h = cat_lane(o, ks, kt);
  const int l16 = lane & ~15;
  int index;
  float lp;
  cat_sample(l, o, l16, h, o < ks ? u_s : u_t, (flags & PGD_AC_DETERMINISTIC) != 0u, index, lp);
  const int i_t = __shfl(index, l16 + ks);
  const float lp_t = __shfl(lp, l16 + ks);
  if (o == 0 && row >= 0) {
#pragma clang fp contract(off) reassociate(off)
    const int i_s = index;
    float a0 = (float)i_s, a1 = (float)i_t;
    if (!(flags & PGD_AC_EMIT_INDEX)) {
      a0 = cat_grid(a0, step_s);
      a1 = cat_grid(a1, step_t);
    }
    act[(size_t)row * 2 + 0] = a0;
    act[(size_t)row * 2 + 1] = a1;
    idx[(size_t)row * 2 + 0] = i_s;
    idx[(size_t)row * 2 + 1] = i_t;
    logp[row] = lp + lp_t;
  }
}

// rows [row_lo, row_lo + n_rows): action 0, 0, index 0, 0, logp 0 and (value non-null) value 0
__global__ __launch_bounds__(CMP_THREADS) void k_cat_clear_rows(const int row_lo, const int n_rows, float* __restrict__ act, int32_t* __restrict__ idx,
                                                                float* __restrict__ logp, float* __restrict__ value) {
  const int r = (int)blockIdx.x * CMP_THREADS + (int)threadIdx.x;
  if (r >= n_rows) return;
  const size_t row = (size_t)row_lo + r;
  act[row * 2 + 0] = 0.0f;
  act[row * 2 + 1] = 0.0f;
  idx[row * 2 + 0] = 0;
  idx[row * 2 + 1] = 0;
  logp[row] = 0.0f;
  if (value) value[row] = 0.0f;
}

// ---- pgd_ppo_grad_cat -------------------------------------------------------------------------------------------------------------------
// pgd_ppo_grad's five launches with this head, dOut [R16][16] and a tile-sum record of PPO_CAT_TS floats: k_ppo_prep as it is;
// k_ppo_wgrad_cat and k_ppo_reduce_cat call the bodies of their namesakes (ppo_wgrad_tile, ppo_reduce_entry of pgd_ppo.h) with this
// head's two widths, and the scratch is ppo_work_of's plan with them.  k_ppo_rows_cat and k_ppo_stats_cat keep their OWN text beside
// ppo_rows_tile and ppo_stats_block: every shared spelling that was tried changed the instructions of a kernel that exists today
// (DESIGN section 34 lists them), and a folding is kept only where no kernel changes.  k_ppo_zero_head follows k_ppo_reduce_cat when
// out_cols > K.
DEV_HOST PpoWork ppo_cat_work(int in_dim, int rows, int nets) { return ppo_work_of<CAT_COLS, PPO_CAT_TS>(in_dim, rows, nets); }

// 1 / n rounded to fp32 ONCE: the quotient is formed in double and passes through an empty asm statement -- left alone, the build
// narrows a double quotient of two small integers to the fp32 division, which is its 2.5 ulp form
DEV float cat_inv(const int n) {
  double q = 1.0 / (double)n;
  asm volatile("" : "+v"(q));
  return (float)q;
}

// One live or empty row of the actor's tile on its sixteen lanes, lane o owning logit l: the header's loss terms and dL/dl_o in double
// from the fp32 logits, every sum over a head in index order -> d (this lane's dOut entry), t[0..4] (the row's loss terms, the same on
// every lane).  row < 0: zeros.
DEV void cat_row_loss(const float l, const int o, const int l16, const int ks, const int kt, const int row, const pgd_ppo_batch& b,
                      const pgd_ppo_hyper& hp, const int32_t* aidx, const float inv_n, float& d, float (&t)[5]) {
#pragma clang fp contract(off) reassociate(off)
  const CatLane h = cat_lane(o, ks, kt);
  const double lj = (double)l;
  double m = -HUGE_VAL;
#pragma unroll
  for (int j = 0; j < CAT_COLS; ++j) {
    const double v = __shfl(lj, l16 + j);
    if (j >= h.j0 && j < h.j1) m = fmax(m, v);
  }
  const double e = exp(lj - m);
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < CAT_COLS; ++j) {
    const double v = __shfl(e, l16 + j);
    if (j >= h.j0 && j < h.j1) s += v;
  }
  const double lp = (lj - m) - log(s), p = e / s, plp = p * lp;
  double Hh = 0.0;
#pragma unroll
  for (int j = 0; j < CAT_COLS; ++j) {
    const double v = __shfl(plp, l16 + j);
    if (j >= h.j0 && j < h.j1) Hh -= v;
  }
  // the taken indices, held within their heads: a caller's error is never followed outside the tile
  const int i_s = row >= 0 ? max(0, min(aidx[(size_t)row * 2 + 0], ks - 1)) : 0;
  const int i_t = row >= 0 ? max(0, min(aidx[(size_t)row * 2 + 1], kt - 1)) : 0;
  const double logp = __shfl(lp, l16 + i_s) + __shfl(lp, l16 + ks + i_t);
  const double H = __shfl(Hh, l16) + __shfl(Hh, l16 + ks);
  d = 0.0f;
#pragma unroll
  for (int k = 0; k < 5; ++k) t[k] = 0.0f;
  if (row < 0) return;
  double A = (double)b.adv[row];
  if (b.adv_stats) A = (A - (double)b.adv_stats[0]) * (double)b.adv_stats[1];
  const double lpo = (double)b.logp_old[row], inv = (double)inv_n;
  const double ratio = exp(logp - lpo);
  const double lo = 1.0 - (double)hp.clip, hi = 1.0 + (double)hp.clip;
  const double s1 = ratio * A, s2 = (ratio < lo ? lo : (ratio > hi ? hi : ratio)) * A;
  const bool flows = s1 <= s2;
  const double g = flows ? -A * ratio * inv : 0.0;  // dL / dlogp
  const double ge = (double)hp.ent_coef * inv;
  const bool taken = o == (o < ks ? i_s : ks + i_t);
  if (o < ks + kt) d = (float)(g * ((taken ? 1.0 : 0.0) - p) + ge * (p * (lp + Hh)));
  t[0] = (float)(-(s1 < s2 ? s1 : s2));
  t[1] = (float)H;
  t[2] = (float)(lpo - logp);
  t[3] = flows ? 0.0f : 1.0f;
  t[4] = (float)ratio;
}

// k_ppo_rows with the categorical head: network blockIdx.y of gridDim.y for the 16 minibatch positions blockIdx.x * 16 + [0, 16).
// LDS: X | H1 | H2 | 4 KB: [0, 256) the critic's head weights (the actor: its partial logit tiles over all of it, dead behind cat_logits),
// [256, 512) dOut [16][16], [512, 896) the rows' loss terms [16][PPO_CAT_TS] -- ac_lds_bytes, less than k_ppo_rows'.
// The two hidden layers, the critic's dot product and loss, and the dZ1 epilogue are ppo_rows_tile's text: each was tried as a function
// of its own that both call (one at a time), and each changed all six k_ppo_rows* symbols.
template <bool NORM>
__global__ __launch_bounds__(WAVE * MLP_WAVES, 4) void k_ppo_rows_cat(const pgd_actor_critic nets, const pgd_ppo_batch b, const pgd_ppo_hyper hp,
                                                                   const int ks, const int kt, const int32_t* __restrict__ aidx,
                                                                   float* __restrict__ work, const ObsNorm nm) {
  extern __shared__ float mlp_lds[];
  const int n = ppo_live(ppo_count(b.count, b.n_list), b.start, b.stride, b.rows);
  const int i0 = (int)blockIdx.x * MLP_ROWS;  // (the tile's first minibatch position)
  if (i0 >= n) return;
  const bool critic = blockIdx.y != 0;
  const float* __restrict__ W1 = critic ? nets.vw1 : nets.w1;
  const float* __restrict__ b1 = critic ? nets.vb1 : nets.b1;
  const float* __restrict__ W2 = critic ? nets.vw2 : nets.w2;
  const float* __restrict__ b2 = critic ? nets.vb2 : nets.b2;
  const float* __restrict__ W3 = critic ? nets.vw3 : nets.w3;
  const float* __restrict__ b3 = critic ? nets.vb3 : nets.b3;
  const int in_dim = b.in_dim, kp = (in_dim + 3) & ~3, xs = mlp_x_stride(in_dim), K = ks + kt, out_cols = nets.out_cols;
  const PpoWork wk = ppo_cat_work(in_dim, b.rows, (int)gridDim.y);
  const size_t plane = (size_t)wk.R16 * MLP_H;
  const float* __restrict__ W2T = work + wk.w2t + (size_t)blockIdx.y * MLP_H * MLP_H;
  float* __restrict__ H1g = work + wk.act + (size_t)blockIdx.y * 4 * plane;
  float* __restrict__ H2g = H1g + plane;
  float* __restrict__ dZ1g = H2g + plane;
  float* __restrict__ dZ2g = dZ1g + plane;
  float* __restrict__ dOg = work + wk.dout + (size_t)blockIdx.y * wk.R16 * CAT_COLS;
  float* __restrict__ tsum = work + wk.tsum + (size_t)blockIdx.x * PPO_CAT_TS;
  float* X = mlp_lds;
  float* H1 = X + MLP_ROWS * xs;
  float* H2 = H1 + MLP_ROWS * MLP_HS;
  float* W3s = H2 + MLP_ROWS * MLP_HS;
  float* dO = W3s + 256;  // [16][16]
  float* st = W3s + 512;  // [16][PPO_CAT_TS]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float w3v = critic ? W3[tid] : 0.0f;
  ppo_load_rows<NORM>(b, i0, n, kp, xs, wave, lane, X, nm);
  if (critic) W3s[tid] = w3v;
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
  const float inv_n = cat_inv(n);  // (n >= 1 here)
  const int r = tid >> 4, o = tid & 15;
  const int row = ppo_row(b, i0 + r, n);
  if (critic) {  // k_ppo_rows' critic: 16 dot products of 256, sixteen lanes each (the butterfly leaves the sum on every lane); then dL/dv
    float s = 0.0f;
#pragma unroll 4
    for (int k = o; k < MLP_H; k += 16) s = fmaf(H2[r * MLP_HS + k], W3s[k], s);
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    float lv = 0.0f, dv = 0.0f;
    if (row >= 0) {
      const float e = s + b3[0] - b.ret[row];
      lv = 0.5f * e * e;
      dv = hp.vf_coef * e * inv_n;
    }
    dO[r * CAT_COLS + o] = o == 0 ? dv : 0.0f;
    if (o == 0) {
      st[r * PPO_CAT_TS + 21] = lv;
      st[r * PPO_CAT_TS + 22] = dv;
    }
  } else {
    const float l = cat_logits(H2, W3, b3, out_cols, K, tid, W3s);
    float d, t[5];
    cat_row_loss(l, o, lane & ~15, ks, kt, row, b, hp, aidx, inv_n, d, t);
    dO[r * CAT_COLS + o] = d;
    st[r * PPO_CAT_TS + 5 + o] = d;
    if (o == 0) {
#pragma unroll
      for (int k = 0; k < 5; ++k) st[r * PPO_CAT_TS + k] = t[k];
    }
  }
  __syncthreads();
  // the tile's sums, rows in order: one owner per slot
  if (critic ? (tid == 21 || tid == 22) : tid < 21) {
    float s = 0.0f;
    for (int q = 0; q < MLP_ROWS; ++q) s += st[q * PPO_CAT_TS + tid];
    tsum[tid] = s;
  }
  dOg[(size_t)i0 * CAT_COLS + tid] = dO[tid];
  // H1, H2 out; dZ2 = (dOut W3^T)(1 - H2^2) in H2's place and out: thread c takes column c of every row, its K weights in registers
  // (columns at or beyond K: zero, never read), the products summed in column order
  float w3c[CAT_COLS];
#pragma unroll
  for (int k = 0; k < CAT_COLS; ++k) {
    if (critic) w3c[k] = k == 0 ? W3s[tid] : 0.0f;
    else w3c[k] = k < K ? W3[(size_t)tid * out_cols + k] : 0.0f;
  }
  for (int q = 0; q < MLP_ROWS; ++q) {
    const int c = tid;
    const size_t at = (size_t)(i0 + q) * MLP_H + c;
    const float h = H2[q * MLP_HS + c];
    float dh = 0.0f;
#pragma unroll
    for (int k = 0; k < CAT_COLS; ++k) dh = fmaf(dO[q * CAT_COLS + k], w3c[k], dh);
    const float dz = dh * fmaf(-h, h, 1.0f);
    H1g[at] = H1[q * MLP_HS + c];
    H2g[at] = h;
    dZ2g[at] = dz;
    H2[q * MLP_HS + c] = dz;
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = mlp_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  mlp_layer(H2, MLP_HS, W2T, MLP_H, MLP_H, lane, c0, acc);
  {  // dZ1 = dH1 (1 - H1^2): a lane holds four consecutive columns of each of its four rows
    const int col = c0 + 4 * (lane & 15), r4 = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* h = H1 + (r4 + i) * MLP_HS + col;
      const float4 dz = make_float4(acc[0][i] * fmaf(-h[0], h[0], 1.0f), acc[1][i] * fmaf(-h[1], h[1], 1.0f), acc[2][i] * fmaf(-h[2], h[2], 1.0f),
                                    acc[3][i] * fmaf(-h[3], h[3], 1.0f));
      *reinterpret_cast<float4*>(dZ1g + (size_t)(i0 + r4 + i) * MLP_H + col) = dz;
    }
  }
}

// k_ppo_wgrad's body over ppo_cat_work's scratch: the A of dW3^T is dOut [R16][16], all sixteen columns (the critic's and the padding's are zero)
template <bool NORM>
__global__ __launch_bounds__(WAVE * MLP_WAVES, 2) void k_ppo_wgrad_cat(const pgd_ppo_batch b, float* __restrict__ work, const ObsNorm nm) {
  ppo_wgrad_tile<NORM, CAT_COLS, PPO_CAT_TS>(b, work, nm);
}

// k_ppo_reduce's body over ppo_cat_work's scratch; head columns [K, min(out_cols, 16)) of dW3 are written as zero (those from 16 on: k_ppo_zero_head)
__global__ __launch_bounds__(MLP_H) void k_ppo_reduce_cat(const pgd_ppo_batch b, const pgd_ppo_grads gr, const int out_cols, const int K,
                                                          const float* __restrict__ work) {
  const bool critic = blockIdx.y != 0;
  ppo_reduce_entry<CAT_COLS, PPO_CAT_TS>(b, critic, critic ? gr.vw1 : gr.w1, critic ? gr.vb1 : gr.b1, critic ? gr.vw2 : gr.w2,
                                         critic ? gr.vb2 : gr.b2, critic ? gr.vw3 : gr.w3, out_cols, K, work);
}

// ONE workgroup: slot s of the tile sums over the live tiles -- thread (s, u) takes tiles u, u + 8, ... in order, then the eight u in
// order -- -> d_stats, db3[0 .. K) and vb3.
// Its own copy of ppo_stats_block.  As a caller of ppo_stats_block<DW, TS, SL> (red[256 / SL][SL], slots 5 + DW .., db3 written by a loop
// over K, 1 / n as a template function) this kernel compiled to other code under every spelling tried -- batch and gradients by reference
// or by value, with and without __restrict__ on the body's pointers, the network count derived or passed in, db3 unrolled under
// `if constexpr (DW == 4)`: the sums keep their order, the v_add_f32 operands swap and the loop's address arithmetic changes.
__global__ __launch_bounds__(256) void k_ppo_stats_cat(const pgd_ppo_batch b, const pgd_ppo_grads gr, const int has_critic, const int K,
                                                       const float* __restrict__ work, float* __restrict__ stats) {
  __shared__ float red[8][32];
  __shared__ float tot[32];
  const int n = ppo_live(ppo_count(b.count, b.n_list), b.start, b.stride, b.rows);
  const int tiles = (n + 15) >> 4;
  const PpoWork wk = ppo_cat_work(b.in_dim, b.rows, has_critic ? 2 : 1);
  const float* __restrict__ tsum = work + wk.tsum;
  const int s = threadIdx.x & 31, u = threadIdx.x >> 5;
  const bool used = s < 21 || (has_critic && s < 23);
  float a = 0.0f;
  if (used)
    for (int t0 = u; t0 < tiles; t0 += 8 * PPO_BATCH) {  // (PPO_BATCH reads in flight, then their sum in the same order)
      float x[PPO_BATCH];
#pragma unroll
      for (int j = 0; j < PPO_BATCH; ++j) {
        const int t = t0 + 8 * j;
        x[j] = t < tiles ? tsum[(size_t)t * PPO_CAT_TS + s] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < PPO_BATCH; ++j) a += x[j];
    }
  red[u][s] = a;
  __syncthreads();
  if (threadIdx.x < 32) {
    float v = 0.0f;
    for (int q = 0; q < 8; ++q) v += red[q][s];
    tot[s] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float inv = n > 0 ? cat_inv(n) : 0.0f;
    stats[0] = (float)n;
    stats[1] = tot[0] * inv;
    stats[2] = has_critic ? tot[21] * inv : 0.0f;
    stats[3] = tot[1] * inv;
    stats[4] = tot[2] * inv;
    stats[5] = tot[3] * inv;
    stats[6] = tot[4] * inv;
    stats[7] = 0.0f;
    for (int o = 0; o < K; ++o) gr.b3[o] = tot[5 + o];
    if (has_critic) gr.vb3[0] = tot[22];
  }
}

// pgd_mlp_actor_critic_cat (d_rows, d_count null, `list` false) and pgd_mlp_actor_critic_cat_rows (both required): one check, one launch
static int cat_forward(pgd_handle h, int group, bool list, const float* d_obs, int obs_stride, int in_dim, const pgd_actor_critic* nets, int32_t ks,
                       int32_t kt, uint32_t seed, uint32_t tick, uint32_t flags, const int32_t* d_rows, const int32_t* d_count, float* d_actions,
                       int32_t* d_action_index, float* d_logp, float* d_value) {
  bool critic;
  if (!h || !d_obs || (list && (!d_rows || !d_count)) || !d_actions || !d_action_index || !d_logp ||
      (flags & ~(PGD_AC_DETERMINISTIC | PGD_AC_EMIT_INDEX)) != 0u || !cat_bins_ok(ks, kt) ||
      !nets_ok(nets, nullptr, true, in_dim, obs_stride, &critic) || nets->out_cols < ks + kt || (critic && !d_value) ||
      ac_lds_bytes(in_dim) > 65536) return PGD_ERR_ARG;
  return ac_forward(h, group, list ? LDS_AC_CAT_ROWS : LDS_AC_CAT, list ? k_mlp_actor_critic_cat<false, true> : k_mlp_actor_critic_cat<false, false>,
                    list ? k_mlp_actor_critic_cat<true, true> : k_mlp_actor_critic_cat<true, false>, in_dim, [&](const AcRows& r, auto kern) {
    // a list: the defined outputs of the rows that are not listed, then the listed rows (the host does not know how many: a grid for all)
    if (list) hipLaunchKernelGGL(k_cat_clear_rows, dim3((r.rows + CMP_THREADS - 1) / CMP_THREADS), dim3(CMP_THREADS), 0, r.stream, r.row0, r.rows,
                                 d_actions, d_action_index, d_logp, critic ? d_value : nullptr);
    hipLaunchKernelGGL(kern, dim3((r.rows + MLP_ROWS - 1) / MLP_ROWS, critic ? 2 : 1), dim3(WAVE * MLP_WAVES), r.lds, r.stream, d_obs, d_rows,
                       d_count, r.row0, r.rows, obs_stride, in_dim, *nets, (int)ks, (int)kt, cat_step(ks), cat_step(kt), seed, tick, h->ac_tick, r.row_base,
                       flags, d_actions, d_action_index, d_logp, d_value, r.nm);
  });
}

extern "C" {

int pgd_mlp_actor_critic_cat(pgd_handle h, int group, const float* d_obs, int obs_stride, int in_dim, const pgd_actor_critic* nets, int32_t ks,
                             int32_t kt, uint32_t seed, uint32_t tick, uint32_t flags, float* d_actions, int32_t* d_action_index, float* d_logp,
                             float* d_value) {
  return cat_forward(h, group, false, d_obs, obs_stride, in_dim, nets, ks, kt, seed, tick, flags, nullptr, nullptr, d_actions, d_action_index, d_logp,
                     d_value);
}

int pgd_mlp_actor_critic_cat_rows(pgd_handle h, int group, const float* d_obs, int obs_stride, int in_dim, const pgd_actor_critic* nets, int32_t ks,
                                  int32_t kt, uint32_t seed, uint32_t tick, uint32_t flags, const int32_t* d_rows, const int32_t* d_count,
                                  float* d_actions, int32_t* d_action_index, float* d_logp, float* d_value) {
  return cat_forward(h, group, true, d_obs, obs_stride, in_dim, nets, ks, kt, seed, tick, flags, d_rows, d_count, d_actions, d_action_index, d_logp,
                     d_value);
}

size_t pgd_ppo_cat_work_bytes(int in_dim, int rows, int has_critic) {
  return ppo_work_bytes_of<CAT_COLS, PPO_CAT_TS>(in_dim, rows, has_critic ? 2 : 1, ac_lds_bytes);
}

int pgd_ppo_grad_cat(pgd_handle h, const pgd_actor_critic* nets, const pgd_ppo_batch* batch, const pgd_ppo_hyper* hyper, const pgd_ppo_grads* grads,
                     int32_t ks, int32_t kt, const int32_t* d_action_index, float* d_stats, void* d_work, size_t work_bytes) {
  // the argument check, the scratch's plan and the binding of the pgd_ppo_grad family (ppo_grad_plan, pgd_safe.h); batch->action is not read
  if (!d_action_index || !cat_bins_ok(ks, kt)) return PGD_ERR_ARG;
  PpoPlan p;
  const size_t lds = batch ? ac_lds_bytes(batch->in_dim) : 0;
  { int rc = ppo_grad_plan(h, nets, nullptr, batch, false, nullptr, hyper, grads, nullptr, d_stats, d_work, work_bytes, lds, ppo_cat_work, p); if (rc) return rc; }
  const int K = ks + kt;
  if (p.out_cols < K) return PGD_ERR_ARG;
  const pgd_ppo_batch& b = *batch;
  const PpoWork wk = p.wk;
  const auto rows_kern = p.bound ? k_ppo_rows_cat<true> : k_ppo_rows_cat<false>;
  const auto wgrad = p.bound ? k_ppo_wgrad_cat<true> : k_ppo_wgrad_cat<false>;
  HIPCHK(hipSetDevice(h->device));
  { int rc = raise_lds_limit(h, lds_slot(LDS_PPO_ROWS_CAT, p.bound), reinterpret_cast<const void*>(rows_kern), lds); if (rc) return rc; }
  float* work = static_cast<float*>(d_work);
  hipStream_t s = h->stream;
  const dim3 tile(WAVE * MLP_WAVES);
  hipLaunchKernelGGL(k_ppo_prep, dim3(MLP_H, p.n_nets), dim3(MLP_H), 0, s, *nets, work);
  hipLaunchKernelGGL(rows_kern, dim3(wk.R16 / 16, p.n_nets), tile, lds, s, *nets, b, *hyper, (int)ks, (int)kt, d_action_index, work, p.nm);
  hipLaunchKernelGGL(wgrad, dim3(wk.mt, wk.P, p.n_nets), tile, 0, s, b, work, p.nm);
  hipLaunchKernelGGL(k_ppo_reduce_cat, dim3(16 * wk.mt, p.n_nets), dim3(MLP_H), 0, s, b, *grads, p.out_cols, K, work);
  if (p.out_cols > K) ppo_zero_head_launch(s, grads, p.out_cols);  // (k_ppo_stats_cat then writes db3 [0, K))
  hipLaunchKernelGGL(k_ppo_stats_cat, dim3(1), dim3(256), 0, s, b, *grads, p.critic ? 1 : 0, K, work, d_stats);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

}  // extern "C"

#endif
