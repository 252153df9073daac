// pgd_ppo.h -- the PPO update behind a rollout: loss statistics and the gradient of every weight of both networks for one minibatch
// (pgd_ppo_grad), the advantage statistics (pgd_adv_stats) and the Adam step (pgd_adam).  include/pgdrive_hip.h states the formulas.
// Part of the single translation unit pgd_engine.hip (included at its end, behind pgd_actor_critic.h and pgd_marl_rollout.h, whose
// layer code -- mlp_layer, mlp_store_hidden -- it uses; no kernel of those headers is touched).  No reference counterpart: the reference
// hands its arrays to an RL library, which runs autograd over the two networks of pgdrive/examples/ppo_expert/numpy_expert.py:25-78.
//
// The minibatch: list positions q_i = start + i stride, i < rows; live iff q_i < count (device memory).  q_i grows with i, so the live
// positions are i < n with n = clamp(ceil((count - start) / stride), 0, rows): every kernel computes n itself, nothing is reduced for
// it and the host never knows it.  Grids cover `rows`; a tile with no live position ends before it reads a weight.
//
// pgd_ppo_grad, five launches, six when the head has unused columns (out_cols > 4: k_ppo_zero_head behind k_ppo_reduce):
//   k_ppo_prep    W2 and vW2 transposed into the scratch (the backward product dZ2 W2^T then reads its B fragments as mlp_layer reads a
//                 forward layer's: one 16-byte read per lane and k-step)
//   k_ppo_rows    grid (tiles of 16 positions, networks): k_mlp_actor_critic_rows' workgroup -- X tile, H1, H2 in LDS, the head on the
//                 vector ALU -- then the loss of the tile's rows, dOut, dZ2 = (dOut W3^T)(1 - H2^2) in place of H2, dH1 = dZ2 W2^T on the
//                 matrix cores, dZ1 = dH1 (1 - H1^2).  H1, H2, dZ1, dZ2, dOut go to the scratch; so do the tile's sums of the loss
//                 terms and of dOut (16 rows in row order).  Rows of a tile that are not live get dOut = 0 and dZ = 0 by SELECTION.
//   k_ppo_wgrad   grid (output tiles, partitions of PPO_PART rows, networks): one 16 x 256 tile of A^T B summed over the partition's
//                 rows in row order on the matrix cores, A^T staged in LDS in chunks of PPO_CHUNK rows.  (A, B) per output tile:
//                 (X gathered again from the rollout, dZ1) -> dW1; (a row of ones, dZ1) -> db1; (H1, dZ2) -> dW2; (ones, dZ2) -> db2;
//                 (dOut, H2) -> dW3^T.  The partial tiles go to the scratch.
//   k_ppo_reduce  every gradient entry = its partials summed over the live partitions in partition order, written in the weights' own
//                 shapes; head columns at or beyond 4 are written as zero
//   k_ppo_stats   ONE workgroup: the tile sums over the live tiles in a fixed order -> d_stats and db3
// k_ppo_rows, k_ppo_reduce and k_ppo_stats choose their network's pointers from blockIdx.y and hand them to a body (ppo_rows_tile,
// ppo_reduce_entry, ppo_stats_block) that pgd_safe.h's three-network kernels call as well; k_ppo_wgrad takes its network count from its grid.
// The categorical head (pgd_categorical.h) differs from this one in the width of dOut and the length of the tile-sum record: the scratch's
// plan (ppo_work_of), the weight-gradient body (ppo_wgrad_tile) and the reduction body (ppo_reduce_entry) take the two as template
// constants <DW, TS>, and k_ppo_wgrad_cat / k_ppo_reduce_cat call them with 16 and 24 where the kernels here say 4 and PPO_TS.
// ppo_rows_tile and ppo_stats_block serve this head only (what was tried); with their switch GUIDED they are the
// bodies of pgd_guided.h's kernels as well, and without it the code they were.
// Deterministic: no atomics; a row's numbers never depend on its tile neighbours; every sum over rows has one owner and a fixed order
// (rows within a partition, partitions in order; rows within a tile, tiles 16-strided, the sixteen strides in order).
//
// Arithmetic: fp32, except where a handful of lanes decide what a whole row or buffer gets: the row loss and dOut (k_ppo_rows: one lane
// per row, from the fp32 heads), 1 / n, the advantage statistics' final quotient and Adam's record and quotient are formed in double and
// rounded to fp32 once (the library's build turns an fp32 division, square root and expf into their 1 .. 2.5 ulp forms).
//
// Scratch is the CALLER's (pgd_ppo_work_bytes): pgd_rollout_index grows its own inside the call, which a stream that is being captured
// cannot do, so its first call of a shape has to happen outside the capture -- a rule every caller has to know.  Here nothing is
// allocated, and the first call is capturable like every other.
//
// LDS of k_ppo_rows: k_mlp_actor_critic's plus 1 KB (dOut [16][4], the rows' loss terms [16][12]): 64,896 bytes at in_dim 416, and
// the same refusal above it.  k_ppo_wgrad: the A^T chunk [16][PPO_CHUNK + 2] (row stride = 2 mod 32, as pgd_policy.h's tiles).
#ifndef PGD_PPO_H
#define PGD_PPO_H

#define PPO_PART 1024   // rows per partial sum of a weight gradient
#define PPO_CHUNK 256   // rows of A^T staged in LDS at a time
#define PPO_TS 16       // floats per tile-sum record: 0 L_pi, 1 H, 2 logp_old - logp, 3 cut, 4 r, 5..8 dOut (actor); 9 L_v, 10 dv (critic); 11 L_c, 12 dv_c (cost critic, pgd_safe.h); 13 guided rows, 14 -logp(target) (pgd_guided.h)
#define PPO_ST 12       // loss terms per row in LDS (the record's first eleven slots)
#define PPO_BATCH 8     // reads a thread of a one-workgroup reduction keeps in flight: the loop waits for memory once per batch, the sum keeps its order
#define PPO_LOG_2PI 1.8378770664093453f
#define PPO_LOG_2PIE 2.8378770664093453f

// the scratch, in floats from its start: [net] W2^T | [net][H1, H2, dZ1, dZ2][R16][256] | [net] dOut [R16][DW] | tile sums, TS floats per
// tile | partials.  Two heads, two (DW, TS): the Gaussian's 4 and PPO_TS (ppo_work), the categorical's 16 and PPO_CAT_TS (ppo_cat_work,
// pgd_categorical.h).  Template constants: as run-time arguments they moved six scalar instructions of k_ppo_wgrad's epilogue
struct PpoWork { size_t w2t, act, dout, tsum, part, total; int R16, P, mt1, mt; };
template <int DW, int TS>
DEV_HOST PpoWork ppo_work_of(int in_dim, int rows, int nets) {
  PpoWork w;
  w.R16 = (rows + 15) & ~15;
  w.P = (w.R16 + PPO_PART - 1) / PPO_PART;
  w.mt1 = (in_dim + 15) / 16;
  w.mt = w.mt1 + 19;  // dW1 tiles | db1 | 16 dW2 tiles | db2 | dW3^T
  size_t o = 0;
  w.w2t = o;  o += (size_t)nets * MLP_H * MLP_H;
  w.act = o;  o += (size_t)nets * 4 * w.R16 * MLP_H;
  w.dout = o; o += (size_t)nets * w.R16 * DW;
  w.tsum = o; o += (size_t)(w.R16 / 16) * TS;
  w.part = o; o += (size_t)nets * w.P * w.mt * 16 * MLP_H;
  w.total = o;
  return w;
}
DEV_HOST PpoWork ppo_work(int in_dim, int rows, int nets) { return ppo_work_of<4, PPO_TS>(in_dim, rows, nets); }
DEV_HOST size_t ppo_lds_bytes(int in_dim) { return ac_lds_bytes(in_dim) + sizeof(float) * 16 * (4 + PPO_ST); }

// the count of a list: *count within [0, n_list], n_list without a pointer
DEV int ppo_count(const int32_t* count, const int n_list) { return count ? max(0, min(*count, n_list)) : n_list; }
// the number of i in [0, rows) with start + i stride < count
DEV int ppo_live(const int count, const int start, const int stride, const int rows) {
  if (count <= start) return 0;
  const long long m = ((long long)count - start + stride - 1) / stride;
  return (int)(m < rows ? m : rows);
}
// the rollout row of minibatch position i, -1 when the position is not live; an index entry outside the arrays is never followed
DEV int ppo_row(const pgd_ppo_batch& b, const int i, const int n) {
  if (i >= n) return -1;
  const int q = b.start + i * b.stride;
  const int p = b.index ? b.index[q] : q;
  return max(0, min(p, b.n_rows - 1));
}

// mlp_load_rows for minibatch positions i0 + [0, 16): rows that are not live read zero (row 0 is loaded in their place, never used).
// Its own copy: as a caller of mlp_load_rows (by-reference, by-value and always_inline closures) k_ppo_rows / k_ppo_rows_cost compiled to other code
template <bool NORM>
DEV void ppo_load_rows(const pgd_ppo_batch& b, const int i0, const int n, const int kp, const int xs, const int wave, const int lane, float* X,
                       const ObsNorm nm) {
  constexpr int XCH = 5;
  const int in_dim = b.in_dim;
  if (kp <= WAVE * XCH) {
    float v[MLP_ROWS / MLP_WAVES][XCH], sh[XCH], sc[XCH];
    bool live[MLP_ROWS / MLP_WAVES];
    if (NORM) on_lane_table(nm, in_dim, kp, lane, sh, sc);
#pragma unroll
    for (int i = 0; i < MLP_ROWS / MLP_WAVES; ++i) {
      const int row = ppo_row(b, i0 + wave + i * MLP_WAVES, n);
      const bool row_in = row >= 0;
      const float* src = b.obs + (size_t)(row_in ? row : 0) * b.obs_stride;
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
    const int row = ppo_row(b, i0 + r, n);
    const bool row_in = row >= 0;
    const float* src = b.obs + (size_t)(row_in ? row : 0) * b.obs_stride;
    for (int k = lane; k < kp; k += WAVE) {
      if (NORM) X[r * xs + k] = (row_in && k < in_dim) ? on_apply(src[k], nm.table[k], nm.table[kp + k], nm.clip) : 0.0f;
      else X[r * xs + k] = (row_in && k < in_dim) ? src[k] : 0.0f;
    }
  }
}

// W2T[net][k][c] = W2[net][c][k]
__global__ __launch_bounds__(MLP_H) void k_ppo_prep(const pgd_actor_critic nets, float* __restrict__ work) {
  const float* __restrict__ W2 = blockIdx.y ? nets.vw2 : nets.w2;
  float* __restrict__ W2T = work + (size_t)blockIdx.y * MLP_H * MLP_H;  // (PpoWork::w2t is 0)
  const int k = blockIdx.x, c = threadIdx.x;
  W2T[(size_t)k * MLP_H + c] = W2[(size_t)c * MLP_H + k];
}

// One workgroup of k_ppo_rows: network blockIdx.y of gridDim.y -- the actor (critic false) or a critic on (W1 .. b3) with the target `ret` and
// the coefficient `vf_coef`, whose two tile sums go to slots 9 + ts_shift and 10 + ts_shift of the tile's record -- for the 16 minibatch
// positions blockIdx.x * 16 + [0, 16).  k_ppo_rows and k_ppo_rows_cost (pgd_safe.h) choose the network and call it.
// GUIDED (k_ppo_rows_guided, k_ppo_rows_cost_guided: pgd_guided.h, which states the slots): the actor's row lane knows which rows the
// expert overrode (`gd`), drops their surrogate and imitates their target; slots 9 and 10 of the row record, the critic's in ITS
// workgroup, hold the guided bit and -logp(target) in the actor's and go to slots 13 and 14 of the tile's record.  Not GUIDED: `gd` is
// never looked at and every line below compiles to what it compiled to without the switch.
template <bool NORM, bool GUIDED = false>
DEV void ppo_rows_tile(const bool critic, const float* W1, const float* b1, const float* W2,
                       const float* b2, const float* W3, const float* b3, const int out_cols,
                       const float* ret, const float vf_coef, const int ts_shift, const pgd_ppo_batch& b, const pgd_ppo_hyper& hp,
                       float* work, const ObsNorm nm, const pgd_ppo_guide* gd = nullptr) {
  extern __shared__ float mlp_lds[];
  const int n = ppo_live(ppo_count(b.count, b.n_list), b.start, b.stride, b.rows);
  const int i0 = (int)blockIdx.x * MLP_ROWS;  // (the tile's first minibatch position)
  if (i0 >= n) return;
  const int in_dim = b.in_dim, kp = (in_dim + 3) & ~3, xs = mlp_x_stride(in_dim);
  const PpoWork wk = ppo_work(in_dim, b.rows, (int)gridDim.y);
  const size_t plane = (size_t)wk.R16 * MLP_H;
  const float* __restrict__ W2T = work + wk.w2t + (size_t)blockIdx.y * MLP_H * MLP_H;
  float* __restrict__ H1g = work + wk.act + (size_t)blockIdx.y * 4 * plane;
  float* __restrict__ H2g = H1g + plane;
  float* __restrict__ dZ1g = H2g + plane;
  float* __restrict__ dZ2g = dZ1g + plane;
  float* __restrict__ dOg = work + wk.dout + (size_t)blockIdx.y * wk.R16 * 4;
  float* __restrict__ tsum = work + wk.tsum + (size_t)blockIdx.x * PPO_TS;
  float* X = mlp_lds;
  float* H1 = X + MLP_ROWS * xs;
  float* H2 = H1 + MLP_ROWS * MLP_HS;
  float* W3s = H2 + MLP_ROWS * MLP_HS;  // [4][256]
  float* dO = W3s + AC_HEAD * MLP_H;    // [16][4]
  float* st = dO + MLP_ROWS * 4;        // [16][PPO_ST]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int heads = critic ? 1 : AC_HEAD, w3_ld = critic ? 1 : out_cols;
  float w3v[AC_HEAD];
#pragma unroll
  for (int q = 0; q < AC_HEAD; ++q) {
    const int idx = tid + q * WAVE * MLP_WAVES;
    const int k = critic ? idx : idx >> 2, o = critic ? 0 : idx & 3;
    w3v[q] = q < heads ? W3[(size_t)k * w3_ld + o] : 0.0f;
  }
  ppo_load_rows<NORM>(b, i0, n, kp, xs, wave, lane, X, nm);
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
  const float inv_n = (float)(1.0 / (double)n);  // (n >= 1 here; correctly rounded: the build's fp32 division is the 2.5 ulp form)
  const int r = tid >> 4;
  const int row = ppo_row(b, i0 + r, n);
  if (critic) {  // 16 dot products of 256, sixteen lanes each; then dL/dv of the row
    const int part = tid & 15;
    float s = 0.0f;
#pragma unroll 4
    for (int k = part; k < MLP_H; k += 16) s = fmaf(H2[r * MLP_HS + k], W3s[k], s);
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    if (part == 0) {
      float lv = 0.0f, dv = 0.0f;
      if (row >= 0) {
        const float e = s + b3[0] - ret[row];
        lv = 0.5f * e * e;
        dv = vf_coef * e * inv_n;
      }
      dO[r * 4 + 0] = dv;
      dO[r * 4 + 1] = 0.0f;
      dO[r * 4 + 2] = 0.0f;
      dO[r * 4 + 3] = 0.0f;
      st[r * PPO_ST + 9] = lv;
      st[r * PPO_ST + 10] = dv;
    }
  } else {  // 64 dot products of 256, four lanes each; then the row's loss terms and dL/d(mean0, mean1, log_std0, log_std1)
    const int o = (tid >> 2) & 3, part = tid & 3;
    float s = 0.0f;
#pragma unroll 4
    for (int k = part; k < MLP_H; k += 4) s = fmaf(H2[r * MLP_HS + k], W3s[o * MLP_H + k], s);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    const float v = s + b3[o];
    const int l16 = lane & ~15;
    const float m0 = __shfl(v, l16), m1 = __shfl(v, l16 + 4), ls0 = __shfl(v, l16 + 8), ls1 = __shfl(v, l16 + 12);
    if ((lane & 15) == 0) {
      float d[4] = {0.0f, 0.0f, 0.0f, 0.0f}, t[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      [[maybe_unused]] float gt[2] = {0.0f, 0.0f};  // GUIDED: the guided bit u and -logp(target)
      if (row >= 0) {
        // in double, from the fp32 heads: four lanes of a wave are here, once per tile, and the ratio and the cut are where a rounding
        // of logp shows (the library's build makes expf the 1 ulp exp2 form: pgdrive_amd/build.py)
        double A = (double)b.adv[row];
        if (b.adv_stats) A = (A - (double)b.adv_stats[0]) * (double)b.adv_stats[1];
        const double lpo = (double)b.logp_old[row], inv = (double)inv_n;
        const double e0 = exp(-(double)ls0), e1 = exp(-(double)ls1);
        const double z0 = ((double)b.action[(size_t)row * 2 + 0] - (double)m0) * e0, z1 = ((double)b.action[(size_t)row * 2 + 1] - (double)m1) * e1;
        const double logp = -0.5 * (z0 * z0 + z1 * z1) - (double)ls0 - (double)ls1 - 1.8378770664093453;
        const double ratio = exp(logp - lpo);
        const double lo = 1.0 - (double)hp.clip, hi = 1.0 + (double)hp.clip;
        const double s1 = ratio * A, s2 = (ratio < lo ? lo : (ratio > hi ? hi : ratio)) * A;
        const bool flows = s1 <= s2;
        const double g = flows ? -A * ratio * inv : 0.0;  // dL / dlogp
        const double ge = (double)hp.ent_coef * inv;
        if constexpr (GUIDED) {
          // u and sur SELECT: a row without the surrogate takes nothing from its action, advantage or old log-probability, and a
          // target is read only where u holds.  The free part is the expressions of the other branch SPELLED AS THERE and selected
          // afterwards -- the build contracts g (z^2 - 1) - ge into one fma, and a select in front of the subtraction moved the
          // contraction to the other product: another rounding of the double --, rounded once with what u adds.
          const bool u = gd->mask ? (gd->mask[row] & gd->mask_bits) != 0u : true;
          const bool sur = !u || (gd->mode & PGD_GUIDE_KEEP_SURROGATE) != 0u;
          const double f0 = g * z0 * e0, f1 = g * z1 * e1, f2 = g * (z0 * z0 - 1.0) - ge, f3 = g * (z1 * z1 - 1.0) - ge;
          double d0 = sur ? f0 : 0.0, d1 = sur ? f1 : 0.0, d2 = sur ? f2 : -ge, d3 = sur ? f3 : -ge;
          if (u) {
            const float* tg = gd->target + (size_t)row * gd->target_stride;
            const double c = (double)gd->bc_coef * inv;
            const double zt0 = ((double)tg[0] - (double)m0) * e0, zt1 = ((double)tg[1] - (double)m1) * e1;
            d0 -= c * zt0 * e0;
            d1 -= c * zt1 * e1;
            d2 += c * (1.0 - zt0 * zt0);
            d3 += c * (1.0 - zt1 * zt1);
            gt[0] = 1.0f;
            gt[1] = (float)(0.5 * (zt0 * zt0 + zt1 * zt1) + (double)ls0 + (double)ls1 + 1.8378770664093453);
          }
          d[0] = (float)d0;
          d[1] = (float)d1;
          d[2] = (float)d2;
          d[3] = (float)d3;
          t[0] = sur ? (float)(-(s1 < s2 ? s1 : s2)) : 0.0f;
          t[1] = ls0 + ls1 + PPO_LOG_2PIE;
          t[2] = sur ? (float)(lpo - logp) : 0.0f;
          t[3] = sur && !flows ? 1.0f : 0.0f;
          t[4] = sur ? (float)ratio : 0.0f;
        } else {
        d[0] = (float)(g * z0 * e0);
        d[1] = (float)(g * z1 * e1);
        d[2] = (float)(g * (z0 * z0 - 1.0) - ge);
        d[3] = (float)(g * (z1 * z1 - 1.0) - ge);
        t[0] = (float)(-(s1 < s2 ? s1 : s2));
        t[1] = ls0 + ls1 + PPO_LOG_2PIE;
        t[2] = (float)(lpo - logp);
        t[3] = flows ? 0.0f : 1.0f;
        t[4] = (float)ratio;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) dO[r * 4 + k] = d[k];
#pragma unroll
      for (int k = 0; k < 5; ++k) st[r * PPO_ST + k] = t[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) st[r * PPO_ST + 5 + k] = d[k];
      if constexpr (GUIDED) {
        st[r * PPO_ST + 9] = gt[0];
        st[r * PPO_ST + 10] = gt[1];
      }
    }
  }
  __syncthreads();
  // the tile's sums, rows in order: one owner per slot (GUIDED: the actor's slots 9 and 10 are the record's 13 and 14)
  if (tid < 11 && (critic ? tid >= 9 : (GUIDED || tid < 9))) {
    float s = 0.0f;
    for (int q = 0; q < MLP_ROWS; ++q) s += st[q * PPO_ST + tid];
    tsum[critic ? tid + ts_shift : (GUIDED && tid >= 9 ? tid + 4 : tid)] = s;
  }
  if (tid < MLP_ROWS * 4) dOg[(size_t)i0 * 4 + tid] = dO[tid];
  // H1, H2 out; dZ2 = (dOut W3^T)(1 - H2^2) in H2's place and out
  for (int e = tid; e < MLP_ROWS * MLP_H; e += WAVE * MLP_WAVES) {
    const int q = e >> 8, c = e & (MLP_H - 1);
    const size_t at = (size_t)(i0 + q) * MLP_H + c;
    const float h = H2[q * MLP_HS + c];
    float dh = dO[q * 4] * W3s[c];
    if (!critic) dh = fmaf(dO[q * 4 + 3], W3s[3 * MLP_H + c], fmaf(dO[q * 4 + 2], W3s[2 * MLP_H + c], fmaf(dO[q * 4 + 1], W3s[MLP_H + c], dh)));
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

template <bool NORM>
__global__ __launch_bounds__(WAVE * MLP_WAVES, 4) void k_ppo_rows(const pgd_actor_critic nets, const pgd_ppo_batch b, const pgd_ppo_hyper hp,
                                                               float* __restrict__ work, const ObsNorm nm) {
  const bool critic = blockIdx.y != 0;
  ppo_rows_tile<NORM>(critic, critic ? nets.vw1 : nets.w1, critic ? nets.vb1 : nets.b1, critic ? nets.vw2 : nets.w2, critic ? nets.vb2 : nets.b2,
                      critic ? nets.vw3 : nets.w3, critic ? nets.vb3 : nets.b3, nets.out_cols, b.ret, hp.vf_coef, 0, b, hp, work, nm);
}

// what output tile `tile` of a network is: 0 dW1 (m0 = its first weight row), 1 db1, 2 dW2, 3 db2, 4 dW3^T
DEV int ppo_tile_kind(const int tile, const int mt1, int& m0) {
  m0 = 0;
  if (tile < mt1) { m0 = tile * 16; return 0; }
  if (tile == mt1) return 1;
  if (tile < mt1 + 17) { m0 = (tile - mt1 - 1) * 16; return 2; }
  return tile == mt1 + 17 ? 3 : 4;
}

// One workgroup of k_ppo_wgrad over ppo_work_of<DW, TS>'s scratch: the A of dW3^T is dOut [R16][DW], columns at or beyond DW zero.
// NORM: the X of dW1 is gathered as k_ppo_rows loaded it, normalised by the bound table (the table has not moved in between: one stream).
// The batch BY VALUE: by const reference all four kernels scheduled their prologue otherwise
template <bool NORM, int DW, int TS>
DEV void ppo_wgrad_tile(const pgd_ppo_batch b, float* __restrict__ work, const ObsNorm nm) {
  __shared__ float At[16 * (PPO_CHUNK + 2)];
  const int n = ppo_live(ppo_count(b.count, b.n_list), b.start, b.stride, b.rows);
  const int live16 = (n + 15) & ~15;
  const int rbeg = (int)blockIdx.y * PPO_PART;
  if (rbeg >= live16) return;
  const int rend = min(rbeg + PPO_PART, live16);
  const int in_dim = b.in_dim, net = (int)blockIdx.z;
  const PpoWork wk = ppo_work_of<DW, TS>(in_dim, b.rows, (int)gridDim.z);
  const size_t plane = (size_t)wk.R16 * MLP_H;
  const float* __restrict__ H1g = work + wk.act + (size_t)net * 4 * plane;
  const float* __restrict__ H2g = H1g + plane;
  const float* __restrict__ dZ1g = H2g + plane;
  const float* __restrict__ dZ2g = dZ1g + plane;
  const float* __restrict__ dOg = work + wk.dout + (size_t)net * wk.R16 * DW;
  int m0;
  const int kind = ppo_tile_kind((int)blockIdx.x, wk.mt1, m0);
  const float* __restrict__ B = kind <= 1 ? dZ1g : (kind <= 3 ? dZ2g : H2g);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c0 = wave * 64;
  const int m = tid & 15, jj = tid >> 4;
  mlp_f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = mlp_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int r0 = rbeg; r0 < rend; r0 += PPO_CHUNK) {
    const int rc = min(PPO_CHUNK, rend - r0);  // (a multiple of 16)
    for (int j = jj; j < rc; j += 16) {
      float v;
      if (kind == 0) {
        const int row = ppo_row(b, r0 + j, n);
        const bool in = row >= 0 && m0 + m < in_dim;
        v = in ? b.obs[(size_t)row * b.obs_stride + m0 + m] : 0.0f;
        if (NORM) v = in ? on_apply(v, nm.table[m0 + m], nm.table[((in_dim + 3) & ~3) + m0 + m], nm.clip) : 0.0f;
      } else if (kind == 2) {
        v = H1g[(size_t)(r0 + j) * MLP_H + m0 + m];
      } else if (kind == 4) {
        v = m < DW ? dOg[(size_t)(r0 + j) * DW + m] : 0.0f;
      } else {
        v = m == 0 ? 1.0f : 0.0f;
      }
      At[m * (PPO_CHUNK + 2) + j] = v;
    }
    __syncthreads();
    mlp_layer(At, PPO_CHUNK + 2, B + (size_t)r0 * MLP_H, rc, rc, lane, c0, acc);
    __syncthreads();
  }
  float* __restrict__ out = work + wk.part + ((((size_t)net * wk.P + blockIdx.y) * wk.mt + blockIdx.x) * 16) * MLP_H;
  const int col = c0 + 4 * (lane & 15), r4 = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *reinterpret_cast<float4*>(out + (size_t)(r4 + i) * MLP_H + col) = make_float4(acc[0][i], acc[1][i], acc[2][i], acc[3][i]);
}

template <bool NORM>
__global__ __launch_bounds__(WAVE * MLP_WAVES, 2) void k_ppo_wgrad(const pgd_ppo_batch b, float* __restrict__ work, const ObsNorm nm) {
  ppo_wgrad_tile<NORM, 4, PPO_TS>(b, work, nm);
}

// grid (16 mt, networks): block (16 tile + m, net), thread c: the partials of entry (m, c) of the tile over the live partitions, in order
// (K: the head's live columns -- the Gaussian's literal 4, the categorical head's ks + kt; columns [K, min(out_cols, 16)) are written as zero)
template <int DW, int TS>
DEV void ppo_reduce_entry(const pgd_ppo_batch& b, const bool critic, float* dW1, float* db1, float* dW2,
                          float* db2, float* dW3, const int out_cols, const int K, const float* work) {
  const int n = ppo_live(ppo_count(b.count, b.n_list), b.start, b.stride, b.rows);
  const int p_live = (((n + 15) & ~15) + PPO_PART - 1) / PPO_PART;
  const int in_dim = b.in_dim, net = (int)blockIdx.y;
  const PpoWork wk = ppo_work_of<DW, TS>(in_dim, b.rows, (int)gridDim.y);
  const int tile = (int)blockIdx.x >> 4, m = (int)blockIdx.x & 15, c = threadIdx.x;
  int m0;
  const int kind = ppo_tile_kind(tile, wk.mt1, m0);
  const float* __restrict__ part = work + wk.part + ((((size_t)net * wk.P) * wk.mt + tile) * 16 + m) * MLP_H + c;
  float s = 0.0f;
  for (int p = 0; p < p_live; ++p) s += part[(size_t)p * wk.mt * 16 * MLP_H];
  if (kind == 0) {
    if (m0 + m < in_dim) dW1[(size_t)(m0 + m) * MLP_H + c] = s;
  } else if (kind == 1) {
    if (m == 0) db1[c] = s;
  } else if (kind == 2) {
    dW2[(size_t)(m0 + m) * MLP_H + c] = s;
  } else if (kind == 3) {
    if (m == 0) db2[c] = s;
  } else if (critic) {
    if (m == 0) dW3[c] = s;
  } else {
    if (m < K) dW3[(size_t)c * out_cols + m] = s;
    else if (m < out_cols) dW3[(size_t)c * out_cols + m] = 0.0f;  // (head columns that are never read; those from 16 on: k_ppo_zero_head)
  }
}

__global__ __launch_bounds__(MLP_H) void k_ppo_reduce(const pgd_ppo_batch b, const pgd_ppo_grads gr, const int out_cols, const float* __restrict__ work) {
  const bool critic = blockIdx.y != 0;
  ppo_reduce_entry<4, PPO_TS>(b, critic, critic ? gr.vw1 : gr.w1, critic ? gr.vb1 : gr.b1, critic ? gr.vw2 : gr.w2, critic ? gr.vb2 : gr.b2,
                              critic ? gr.vw3 : gr.w3, out_cols, 4, work);
}

// head columns [16, out_cols) of dW3 and [4, out_cols) of db3: zero
__global__ __launch_bounds__(MLP_H) void k_ppo_zero_head(float* __restrict__ dW3, float* __restrict__ db3, const int out_cols) {
  const int c = threadIdx.x;
  for (int o = 16 + (int)blockIdx.x; o < out_cols; o += (int)gridDim.x) dW3[(size_t)c * out_cols + o] = 0.0f;
  if (blockIdx.x == 0)
    for (int o = 4 + c; o < out_cols; o += MLP_H) db3[o] = 0.0f;
}

// ONE workgroup: slot s of the tile sums over the live tiles -- thread (s, u) takes tiles u, u + 16, ... in order, then the sixteen u in
// order -- -> d_stats and db3
// (cost_b3 set: three networks, the cost critic's sums in slots 11 and 12 -> stats[7] and cost_b3[0]; k_ppo_stats_cost, pgd_safe.h)
// (GUIDED, k_ppo_stats_guided of pgd_guided.h: slots 13 and 14 as well, twelve statistics; n_g = slot 13, a sum of ones, exact up to
// PGD_PPO_ROWS_MAX; the surrogate's means are over n_s = n with `keep`, n - n_g without: with n_g = 0 the expressions of the other branch)
template <bool GUIDED = false>
DEV void ppo_stats_block(const pgd_ppo_batch& b, const pgd_ppo_grads& gr, const int has_critic, float* cost_b3,
                         const float* work, float* stats, const int keep = 0) {
  __shared__ float red[16][PPO_TS];
  __shared__ float tot[PPO_TS];
  const int n = ppo_live(ppo_count(b.count, b.n_list), b.start, b.stride, b.rows);
  const int tiles = (n + 15) >> 4;
  const PpoWork wk = ppo_work(b.in_dim, b.rows, cost_b3 ? 3 : (has_critic ? 2 : 1));
  const float* __restrict__ tsum = work + wk.tsum;
  const int s = threadIdx.x & 15, u = threadIdx.x >> 4;
  const bool used = s < 9 || (has_critic && s < 11) || (cost_b3 && s < 13) || (GUIDED && (s == 13 || s == 14));
  float a = 0.0f;
  if (used)
    for (int t0 = u; t0 < tiles; t0 += 16 * PPO_BATCH) {  // (PPO_BATCH reads in flight, then their sum in the same order)
      float x[PPO_BATCH];
#pragma unroll
      for (int j = 0; j < PPO_BATCH; ++j) {
        const int t = t0 + 16 * j;
        x[j] = t < tiles ? tsum[(size_t)t * PPO_TS + s] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < PPO_BATCH; ++j) a += x[j];
    }
  red[u][s] = a;
  __syncthreads();
  if (threadIdx.x < PPO_TS) {
    float v = 0.0f;
    for (int q = 0; q < 16; ++q) v += red[q][s];
    tot[s] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float inv = n > 0 ? (float)(1.0 / (double)n) : 0.0f;
    float inv_s = inv;  // (1 / n_s: the rows that carry the surrogate)
    if constexpr (GUIDED) {
      const int n_g = (int)tot[13], n_s = keep ? n : n - n_g;
      inv_s = n_s > 0 ? (float)(1.0 / (double)n_s) : 0.0f;
      stats[8] = (float)n_g;
      stats[9] = n_g > 0 ? tot[14] * (float)(1.0 / (double)n_g) : 0.0f;
      stats[10] = 0.0f;
      stats[11] = 0.0f;
    }
    stats[0] = (float)n;
    stats[1] = tot[0] * inv_s;
    stats[2] = has_critic ? tot[9] * inv : 0.0f;
    stats[3] = tot[1] * inv;
    stats[4] = tot[2] * inv_s;
    stats[5] = tot[3] * inv_s;
    stats[6] = tot[4] * inv_s;
    stats[7] = cost_b3 ? tot[11] * inv : 0.0f;
    gr.b3[0] = tot[5];
    gr.b3[1] = tot[6];
    gr.b3[2] = tot[7];
    gr.b3[3] = tot[8];
    if (has_critic) gr.vb3[0] = tot[10];
    if (cost_b3) cost_b3[0] = tot[12];
  }
}

__global__ __launch_bounds__(256) void k_ppo_stats(const pgd_ppo_batch b, const pgd_ppo_grads gr, const int has_critic, const float* __restrict__ work,
                                                   float* __restrict__ stats) {
  ppo_stats_block(b, gr, has_critic, nullptr, work, stats);
}

// ---- pgd_adv_stats: ONE workgroup; thread i takes entries i, i + 256, ... in order, a butterfly per wave, the four waves in order ----
DEV float ppo_block_sum(float v, float* wave_sum) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
  __syncthreads();  // (wave_sum may still be read from the call before)
  if ((threadIdx.x & (WAVE - 1)) == 0) wave_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

__global__ __launch_bounds__(256) void k_adv_stats(const float* __restrict__ adv, const int32_t* __restrict__ index, const int32_t* __restrict__ count,
                                                   const int n_list, float* __restrict__ out) {
  __shared__ float wave_sum[4];
  const int n = ppo_count(count, n_list);
  float s = 0.0f;
  for (int q0 = threadIdx.x; q0 < n; q0 += 256 * PPO_BATCH) {
    float x[PPO_BATCH];
#pragma unroll
    for (int j = 0; j < PPO_BATCH; ++j) {
      const int q = q0 + 256 * j;
      x[j] = q < n ? adv[index ? index[q] : q] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < PPO_BATCH; ++j) s += x[j];
  }
  const float mean = n > 0 ? (float)((double)ppo_block_sum(s, wave_sum) / (double)n) : 0.0f;  // (n is the same in every thread)
  float s2 = 0.0f;
  for (int q0 = threadIdx.x; q0 < n; q0 += 256 * PPO_BATCH) {
    float x[PPO_BATCH];
#pragma unroll
    for (int j = 0; j < PPO_BATCH; ++j) {
      const int q = q0 + 256 * j;
      x[j] = q < n ? adv[index ? index[q] : q] - mean : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < PPO_BATCH; ++j) s2 = fmaf(x[j], x[j], s2);
  }
  if (n > 0) s2 = ppo_block_sum(s2, wave_sum);
  if (threadIdx.x == 0) {
    out[0] = mean;
    out[1] = n > 0 ? (float)(1.0 / (sqrt((double)s2 / (double)n) + 1e-8)) : 1.0f;
  }
}

// ---- pgd_adam --------------------------------------------------------------------------------------------------------------------------
// ONE workgroup: |g|^2 (thread i takes entries i, i + 256, ...; the block sum above), then thread 0 advances the step counter and writes the
// record the elementwise launch reads: rec[0] = t (int32), rec[1] = the clipping scale, rec[2] = 1 / (1 - beta1^t), rec[3] = 1 / (1 - beta2^t)
__global__ __launch_bounds__(256) void k_adam_prep(const float* __restrict__ grad, const int n_elem, const float beta1, const float beta2,
                                                   const float max_norm, int32_t* __restrict__ rec) {
  __shared__ float wave_sum[4];
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
    const int t = rec[0] + 1;
    rec[0] = t;
    float* f = reinterpret_cast<float*>(rec);
    f[1] = max_norm > 0.0f ? fminf(1.0f, (float)((double)max_norm / (sqrt((double)s) + 1e-6))) : 1.0f;
    f[2] = (float)(1.0 / (1.0 - pow((double)beta1, (double)t)));
    f[3] = (float)(1.0 / (1.0 - pow((double)beta2, (double)t)));
  }
}

__global__ __launch_bounds__(256) void k_adam(float* __restrict__ param, const float* __restrict__ grad, float* __restrict__ m, float* __restrict__ v,
                                              const int n_elem, const float lr, const float beta1, const float beta2, const float eps,
                                              const int32_t* __restrict__ rec) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= n_elem) return;
  const float* f = reinterpret_cast<const float*>(rec);
  const float g = grad[i] * f[1];
  const float mi = fmaf(beta1, m[i], (1.0f - beta1) * g);
  const float vi = fmaf(beta2, v[i], (1.0f - beta2) * g * g);
  m[i] = mi;
  v[i] = vi;
  // (the quotient in double: the library's build turns an fp32 division and square root into their 2.5 ulp forms; this launch waits for memory)
  param[i] = (float)((double)param[i] - (double)lr * ((double)mi * (double)f[2]) / (sqrt((double)vi * (double)f[3]) + (double)eps));
}

// scratch of a gradient call over n_nets networks whose rows kernel takes lds_of(in_dim) bytes of LDS (0: in_dim or rows out of range)
template <int DW, int TS>
static size_t ppo_work_bytes_of(int in_dim, int rows, int n_nets, size_t (*lds_of)(int)) {
  if (in_dim < 4 || in_dim > 4096 || lds_of(in_dim) > 65536 || rows < 1 || rows > PGD_PPO_ROWS_MAX) return 0;
  return sizeof(float) * ppo_work_of<DW, TS>(in_dim, rows, n_nets).total;
}
static size_t ppo_work_bytes(int in_dim, int rows, int n_nets) { return ppo_work_bytes_of<4, PPO_TS>(in_dim, rows, n_nets, ppo_lds_bytes); }

// pgd_ppo_grad, pgd_ppo_grad_cost and pgd_ppo_grad_guided are one body: pgd_guided.h, behind the three-network and the guided kernels
static int ppo_grad_launch(pgd_handle h, const pgd_actor_critic* nets, const pgd_value_net* cost_net, const pgd_ppo_batch* batch,
                           const pgd_ppo_cost* cost, const pgd_ppo_guide* guide, const pgd_ppo_hyper* hyper, const pgd_ppo_grads* grads,
                           const pgd_value_grads* cost_grads, float* d_stats, void* d_work, size_t work_bytes);

extern "C" {

size_t pgd_ppo_work_bytes(int in_dim, int rows, int has_critic) { return ppo_work_bytes(in_dim, rows, has_critic ? 2 : 1); }

int pgd_ppo_grad(pgd_handle h, const pgd_actor_critic* nets, const pgd_ppo_batch* batch, const pgd_ppo_hyper* hyper, const pgd_ppo_grads* grads,
                 float* d_stats, void* d_work, size_t work_bytes) {
  return ppo_grad_launch(h, nets, nullptr, batch, nullptr, nullptr, hyper, grads, nullptr, d_stats, d_work, work_bytes);
}

int pgd_adv_stats(pgd_handle h, const float* d_adv, const int32_t* d_index, const int32_t* d_count, int n_list, float* d_out) {
  if (!h || !d_adv || !d_out || n_list < 0) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_adv_stats, dim3(1), dim3(256), 0, h->stream, d_adv, d_index, d_count, n_list, d_out);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

int pgd_adam(pgd_handle h, float* d_param, const float* d_grad, float* d_m, float* d_v, int n_elem, int32_t* d_step, float lr, float beta1,
             float beta2, float eps, float max_grad_norm) {
  if (!h || !d_param || !d_grad || !d_m || !d_v || !d_step || n_elem < 1) return PGD_ERR_ARG;
  if (!(beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f) || (reinterpret_cast<uintptr_t>(d_step) & 3u) != 0u) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_adam_prep, dim3(1), dim3(256), 0, h->stream, d_grad, n_elem, beta1, beta2, max_grad_norm, d_step);
  hipLaunchKernelGGL(k_adam, dim3((n_elem + 255) / 256), dim3(256), 0, h->stream, d_param, d_grad, d_m, d_v, n_elem, lr, beta1, beta2, eps, d_step);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

}  // extern "C"

#endif
