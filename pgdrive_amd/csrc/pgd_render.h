// pgd_render.h -- top-down scene rendering: env.render(mode="top_down") (envs/base_env.py:240-248, 463-468; obs/top_down_renderer.py)
// as two kernels over the state already on the device.  Part of the single translation unit pgd_engine.hip (included at its end,
// after pgd_topdown.h, whose td_classify it uses).  The step kernels do not know about it: nothing here is read or written by k_step.
//
// The reference draws with pygame, which is absent here; its polygon / line rasterisation stays UNPINNED (as for the top-down
// observation).  What is pinned is the film geometry, restated on the host from the lane descriptions (pgdrive_amd/render.py, golden
// tests/golden/render_bbox_v0.json), and the scene; every pixel is then evaluated analytically at its centre (u + 0.5, v + 0.5):
//   film      W x H pixels; scaling = H / max(x extent, y extent) - 0.1 px / m of RoadNetwork.get_bounding_box(); origin = box centre -
//             (W / 2, H / 2) / scaling; pos2pix(x, y) = (int((x - ox) * scaling), int((y - oy) * scaling)) = (column, row), no y flip.
//             The host hands (scaling, ox, oy) per map; the kernels evaluate pos2pix in fp64 like the reference.
//   background  once per map at pgd_render_enable (k_render_bg), one bit per pixel: a lane line where the pixel centre lies within
//             line_r = 0.5 * pix(1 m) / scaling of a line box of the map (td_classify, route lanes off; sidewalks are not drawn).
//             Deviation: broken lines follow the map's physical broken-line boxes, not pygame's cosmetic 3 m / 5 m stripe phase.
//             Colours: lines road_rgb on black; light_background inverts both (255 - x): black lines on white by default.
//   vehicles  a ring of the last num_stack rendered frames per env.  A frame holds the controlled agents that are ACTIVE (done = 0) or
//             DYING (done = 1, the delay-done queue), and with draw_traffic = 1 (NOT a reference option) also the IDM traffic
//             (100, 200, 255) and the traffic objects (200, 0, 150) that are present (VehicleGraphics.BLUE / PURPLE; toll booths are
//             invisible walls and are not drawn; a cone is the square of its diameter).  Box: centre pos2pix(position), length
//             pix(LENGTH), width pix(WIDTH) (integers), axis a = (cos h, sin h), n = (-sin h, cos h), h = 0 when |heading| <= 2 deg;
//             a pixel is inside when |d.a| <= len / 2 and |d.n| <= wid / 2, d = pixel centre - box centre.  A box whose centre is
//             50 px or more outside the film is not drawn (WorldSurface.is_visible).
//   painting  frames oldest first; frame k of n (0 = oldest) has i = n - k, is skipped when history_smooth != 0 and i % history_smooth
//             != 0, and is painted in trunc(c + (i / n) * (255 - c)) per channel (fp64, faded toward white).  Then the newest frame in
//             its own colour, with a (60, 60, 60) contour: the pixels inside the box whose centre is within 2 px of its edge.  Then a
//             red (255, 0, 0) disk of radius 5 px (pixel centres within 5 px) at every entry of the env's dead list.  The last draw
//             wins.  (The faded copy of the newest frame that the reference paints first is covered by this second draw pixel for
//             pixel and is not evaluated.)
//   deads     a dying agent enters its env's dead list when it is first rendered dying (the reference appends it at every call while it
//             is dying; a dying body is static, so the extra copies are the same disk).  The list keeps 256 entries per env; when it
//             is full the oldest entry is dropped.
//   colours   agent colours come from the ten-colour table PGD_RENDER_PALETTE (include/pgdrive_hip.h), indexed by a counter hash of
//             (seed, env_base + e, agent id): an agent keeps its colour for life (the reference draws it from an unseeded RNG).
//   episodes  a new episode clears the env's ring and dead list: an auto-reset shows as a change of EI_EPISODES since the env's last
//             render, pgd_reset marks the envs it resets.  (The reference never clears them: after a reset it paints the last
//             episode's trail.)  Only rendered envs advance their ring.
// Kernels: k_render_prep -- one wave per rendered env: appends the frame to the ring, updates the dead list, and turns ring and dead
// list into the env's draw list (pixel-space boxes and disks in painter's order, each with its pixel bounding box).  k_render_frame --
// one block per (1024 x 16 pixels of the film, env): the block copies the draw ops that reach its rows into LDS; each thread takes
// 16 consecutive pixels at a time, walks the list newest first (bounding box, then the exact test), stops when all 16 are decided,
// falls back to the background; a wave's 64 chunks go out through LDS as contiguous 16-byte stores.
#ifndef PGD_RENDER_H
#define PGD_RENDER_H

#define RD_DEAD_CAP 256   /* dead-list entries per env */
#define RD_MAX_OPS 2048   /* draw ops per env (num_stack * V + RD_DEAD_CAP): the frame kernel holds them in 64 KB of LDS */
#define RD_CHUNKS 1024    /* 16-pixel chunks per block of k_render_frame (four per thread) */
#define RD_NCOL 12        /* colour rows of the fade table: the ten agent colours, IDM traffic, traffic objects */
#define RD_RED 0x0000ffu  /* packed r | g << 8 | b << 16 */
#define RD_CONTOUR 0x3c3c3cu

static const uint8_t rd_palette[10][3] = PGD_RENDER_PALETTE;

// one vehicle of one ring frame, in film pixels (the film geometry of an env's map does not change within an episode)
struct RBox {
  short cu, cv, len, wid;  // pos2pix of the centre, pix(LENGTH), pix(WIDTH)
  float ax, ay;            // unit long axis (1, 0) when the heading is snapped
  uint32_t info;           // bit 0 drawn (present and visible), bit 1 done (dying agent), bits 8..15 colour row
};
// one draw op of an env's painter's list
struct __attribute__((aligned(16))) ROp {
  short u0, u1, v0, v1;  // pixel bounding box, clipped to the film
  short cu, cv;
  uint32_t rgb;          // r | g << 8 | b << 16 | kind << 24 (0 box, 1 box with contour, 2 disk)
  float ax, ay, hl, hw;  // long axis, half length / half width [px]
};
static_assert(sizeof(ROp) == 32, "draw op must be 32 bytes");
// per-env history
struct REnv {
  int total;     // frames appended since the ring was cleared
  int last_ep;   // EI_EPISODES at the last render (RD_FORGET: cleared by pgd_reset)
  int dead_total;
  int n_ops;     // draw ops of the last k_render_prep
  int map;       // map of the env's episode at the last render
  int pad[3];
};
#define RD_FORGET ((int)0x80000000)

struct RenderDev {
  int W, H, S, hs, draw_traffic;
  uint32_t bg_rgb, line_rgb;       // background / lane-line colour after the light_background inversion
  const double* geom;              // [n_maps][3] scaling, ox, oy
  const uint16_t* bg;              // [n_maps][words]: one bit per pixel, pixel p = v * W + u at bit p % 16 of word p / 16
  long long words;                 // 16-bit words per map
  const uint32_t* lut;             // [RD_NCOL][S + 1][S + 1]: colour of row c at age i of n frames
  RBox* ring;                      // [N][S][V]
  int2* dead;                      // [N][RD_DEAD_CAP] pixel centres
  REnv* env;                       // [N]
  ROp* ops;                        // [N][max_ops]
  int max_ops;
};

// The background of one map: bit (p % 16) of word p / 16 = pixel p is a lane line.  One thread per word.
__global__ __launch_bounds__(256) void k_render_bg(PgdDev d, int map, double sc, double ox, double oy, float line_r, uint16_t* __restrict__ bg,
                                                    int W, int H) {
  __shared__ uint32_t s_route[128];  // no route lanes: td_classify's route test never passes
  for (int k = threadIdx.x; k < 128; k += 256) s_route[k] = 0u;
  __syncthreads();
  const MapView mv = map_view(d, map);
  const long long n_pix = (long long)W * H, words = (n_pix + 15) / 16;
  for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < words; w += (long long)gridDim.x * 256) {
    uint32_t bits = 0u;
    for (int k = 0; k < 16; ++k) {
      const long long p = w * 16 + k;
      if (p >= n_pix) break;
      const int v = (int)(p / W), u = (int)(p - (long long)v * W);
      const float wx = (float)(ox + ((double)u + 0.5) / sc), wy = (float)(oy + ((double)v + 0.5) / sc);
      if (td_classify(mv, s_route, wx, wy, line_r) == 2) bits |= 1u << k;
    }
    bg[w] = (uint16_t)bits;
  }
}

// pgd_reset: the listed envs start a new episode -- their next render clears ring and dead list
__global__ void k_render_forget(REnv* env, const int32_t* __restrict__ ids, int n) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) env[ids ? ids[k] : k].last_ep = RD_FORGET;
}

// pos2pix / pix in fp64 as the reference evaluates them (no contraction or re-association: the truncation picks the pixel)
DEV int rd_pix(double v, double o, double sc) {
#pragma clang fp contract(off)
#pragma clang fp reassociate(off)
  return (int)((v - o) * sc);
}

DEV bool rd_clip(int& a0, int& a1, int lim) { a0 = max(a0, 0); a1 = min(a1, lim - 1); return a0 <= a1; }

// One wave per rendered env: ring and dead list advance, then the env's draw list is rebuilt.  lane = vehicle slot (V <= 64).
__global__ __launch_bounds__(WAVE) void k_render_prep(PgdDev d, RenderDev r, const int32_t* __restrict__ ids) {
  const int k = blockIdx.x, lane = threadIdx.x, V = d.V, A = d.A;
  const int e = ids ? ids[k] : k;
  REnv st = r.env[e];
  const int episodes = d.ei[(size_t)e * PGD_NEI + EI_EPISODES];
  const int scen = d.ei[(size_t)e * PGD_NEI + EI_SCEN];
  const int map = d.scen()[scen].map;
  if (episodes != st.last_ep) { st.total = 0; st.dead_total = 0; }  // a new episode since the last render: no trail, no deads
  const double sc = r.geom[map * 3], ox = r.geom[map * 3 + 1], oy = r.geom[map * 3 + 2];
  const int S = r.S, W = r.W, H = r.H;
  RBox* ring = r.ring + (size_t)e * S * V;
  // ---- this frame ----
  bool new_dead = false;
  RBox b{0, 0, 0, 0, 1.0f, 0.0f, 0u};
  if (lane < V) {
    Veh rc;
    load_rec_head(rec_block(d.rec, (size_t)e, V), V, lane, rc);
    const pgd_spawn& sp = d.spawns()[(size_t)scen * d.sstride + rc.spawn];
    const bool agent = lane < A;
    const bool present = agent ? (rc.status == ST_ACTIVE || rc.status == ST_DYING)
                               : (r.draw_traffic && (rc.status == ST_PENDING || rc.status == ST_ACTIVE) && sp.kind != PGD_OBJ_BUILDING);
    const bool done = agent && rc.status == ST_DYING;
    const int cu = rd_pix((double)rc.x, ox, sc), cv = rd_pix((double)rc.y, oy, sc);
    const bool visible = -50 < cu && cu < W + 50 && -50 < cv && cv < H + 50;
    const bool snap = fabs((double)rc.th) <= 2.0 * 3.141592653589793 / 180.0;
    uint32_t col;
    if (agent) col = pgd_rng(d.cfg.seed, (uint32_t)(d.cfg.env_base + e), 0x7e4d0c01u, (uint32_t)rc.agent_id) % 10u;
    else col = sp.kind == PGD_OBJ_VEHICLE ? 10u : 11u;
    b.cu = (short)max(-32768, min(32767, cu));
    b.cv = (short)max(-32768, min(32767, cv));
    b.len = (short)min(32767, rd_pix((double)sp.length, 0.0, sc));
    b.wid = (short)min(32767, rd_pix((double)(sp.kind == PGD_OBJ_CYLINDER ? sp.length : sp.width), 0.0, sc));  // (a cone: its diameter)
    b.ax = snap ? 1.0f : rc.hx;
    b.ay = snap ? 0.0f : rc.hy;
    b.info = (present && visible ? 1u : 0u) | (done ? 2u : 0u) | (col << 8);
    if (done) {  // a dying agent enters the dead list once: unless the last frame already showed it dying at this pixel
      new_dead = true;
      if (st.total > 0) {
        const RBox q = ring[(size_t)((st.total - 1) % S) * V + lane];
        if ((q.info & 2u) && q.cu == b.cu && q.cv == b.cv) new_dead = false;
      }
    }
  }
  __syncthreads();  // (every lane has read the previous frame before the ring slot is overwritten: S == 1 reuses it)
  if (lane < V) ring[(size_t)(st.total % S) * V + lane] = b;
  {
    const unsigned long long m = __ballot(new_dead);
    if (new_dead) {
      const int q = st.dead_total + __popcll(m & ((1ull << lane) - 1ull));
      r.dead[(size_t)e * RD_DEAD_CAP + q % RD_DEAD_CAP] = make_int2(b.cu, b.cv);
    }
    st.dead_total += __popcll(m);
  }
  st.total += 1;
  __syncthreads();
  // ---- draw list, painter's order: older frames (faded), the newest frame with its contour, the dead disks ----
  ROp* ops = r.ops + (size_t)e * r.max_ops;
  const int n = min(st.total, S);
  int n_ops = 0;
  auto emit_box = [&](const RBox& q, bool want, uint32_t rgb, uint32_t kind) {
    int u0 = 0, u1 = -1, v0 = 0, v1 = -1;
    const float hl = 0.5f * (float)q.len, hw = 0.5f * (float)q.wid;
    if (want) {
      const float ex = hl * fabsf(q.ax) + hw * fabsf(q.ay), ey = hl * fabsf(q.ay) + hw * fabsf(q.ax);
      u0 = (int)floorf((float)q.cu - ex) - 1; u1 = (int)ceilf((float)q.cu + ex) + 1;
      v0 = (int)floorf((float)q.cv - ey) - 1; v1 = (int)ceilf((float)q.cv + ey) + 1;
      want = rd_clip(u0, u1, W) && rd_clip(v0, v1, H);
    }
    const unsigned long long m = __ballot(want);
    if (want) {
      ROp o;
      o.u0 = (short)u0; o.u1 = (short)u1; o.v0 = (short)v0; o.v1 = (short)v1; o.cu = q.cu; o.cv = q.cv;
      o.rgb = rgb | (kind << 24); o.ax = q.ax; o.ay = q.ay; o.hl = hl; o.hw = hw;
      ops[n_ops + __popcll(m & ((1ull << lane) - 1ull))] = o;
    }
    n_ops += __popcll(m);
  };
  for (int f = 0; f < n - 1; ++f) {
    const int i = n - f;
    if (r.hs != 0 && i % r.hs != 0) continue;
    RBox q{0, 0, 0, 0, 1.0f, 0.0f, 0u};
    if (lane < V) q = ring[(size_t)((st.total - n + f) % S) * V + lane];
    const uint32_t rgb = r.lut[((size_t)((q.info >> 8) & 255u) * (S + 1) + n) * (S + 1) + i];
    emit_box(q, (q.info & 1u) != 0u, rgb, 0u);
  }
  {
    RBox q{0, 0, 0, 0, 1.0f, 0.0f, 0u};
    if (lane < V) q = ring[(size_t)((st.total - 1) % S) * V + lane];
    const uint32_t rgb = r.lut[((size_t)((q.info >> 8) & 255u) * (S + 1) + n) * (S + 1) + 0];
    emit_box(q, (q.info & 1u) != 0u, rgb, 1u);
  }
  const int nd = min(st.dead_total, RD_DEAD_CAP), d0 = st.dead_total - nd;
  for (int j0 = 0; j0 < nd; j0 += WAVE) {
    const int j = j0 + lane;
    int u0 = 0, u1 = -1, v0 = 0, v1 = -1;
    int2 p = make_int2(0, 0);
    bool want = j < nd;
    if (want) {
      p = r.dead[(size_t)e * RD_DEAD_CAP + (d0 + j) % RD_DEAD_CAP];
      u0 = p.x - 6; u1 = p.x + 6; v0 = p.y - 6; v1 = p.y + 6;
      want = rd_clip(u0, u1, W) && rd_clip(v0, v1, H);
    }
    const unsigned long long m = __ballot(want);
    if (want) {
      ROp o;
      o.u0 = (short)u0; o.u1 = (short)u1; o.v0 = (short)v0; o.v1 = (short)v1; o.cu = (short)p.x; o.cv = (short)p.y;
      o.rgb = RD_RED | (2u << 24); o.ax = 1.0f; o.ay = 0.0f; o.hl = 5.0f; o.hw = 5.0f;
      ops[n_ops + __popcll(m & ((1ull << lane) - 1ull))] = o;
    }
    n_ops += __popcll(m);
  }
  if (lane == 0) {
    st.last_ep = episodes;
    st.n_ops = n_ops;
    st.map = map;
    r.env[e] = st;
  }
}

// is the centre of pixel (u, v) inside op o; *edge: within 2 px of a box's edge (the contour band)
DEV bool rd_hit(const ROp& o, int u, int v, bool& edge) {
  const float dx = (float)u + 0.5f - (float)o.cu, dy = (float)v + 0.5f - (float)o.cv;
  if ((o.rgb >> 24) == 2u) { edge = false; return dx * dx + dy * dy <= 25.0f; }
  const float la = fabsf(dx * o.ax + dy * o.ay), lb = fabsf(dy * o.ax - dx * o.ay);
  edge = la >= o.hl - 2.0f || lb >= o.hw - 2.0f;
  return la <= o.hl && lb <= o.hw;
}

// One block per (RD_CHUNKS 16-pixel chunks of the film, rendered env).  frames: [n][H][W][3] bytes, 16-byte aligned.  A film whose
// W * H is not a multiple of 16 ends in a partial chunk, and frames after the first may then start off a 16-byte boundary: the
// waves whose output is not aligned write their bytes one by one.
__global__ __launch_bounds__(256) void k_render_frame(RenderDev r, const int32_t* __restrict__ ids, uint8_t* __restrict__ frames) {
  extern __shared__ ROp s_ops[];
  __shared__ uint4 s_stage[4 * 3 * WAVE];  // per wave: 64 chunks x 48 bytes on their way out
  __shared__ int s_n;
  const int k = blockIdx.y, e = ids ? ids[k] : k, tid = threadIdx.x;
  const int W = r.W;
  const long long n_pix = (long long)W * r.H, n_chunks = (n_pix + 15) / 16;
  const long long c0 = (long long)blockIdx.x * RD_CHUNKS, c1 = min(c0 + RD_CHUNKS, n_chunks);
  const REnv st = r.env[e];
  const int r0 = (int)((c0 * 16) / W), r1 = (int)((min(c1 * 16, n_pix) - 1) / W);  // the block's rows
  // the ops that reach these rows, in painter's order (one wave compacts; the list is short)
  if (tid < WAVE) {
    const ROp* ops = r.ops + (size_t)e * r.max_ops;
    int n = 0;
    for (int j0 = 0; j0 < st.n_ops; j0 += WAVE) {
      const ROp o = ops[min(j0 + tid, st.n_ops - 1)];
      const bool take = j0 + tid < st.n_ops && o.v1 >= r0 && o.v0 <= r1;
      const unsigned long long m = __ballot(take);
      if (take) s_ops[n + __popcll(m & ((1ull << tid) - 1ull))] = o;
      n += __popcll(m);
    }
    if (tid == 0) s_n = n;
  }
  __syncthreads();
  const int n_ops = s_n;
  const uint16_t* bg = r.bg + (size_t)st.map * r.words;
  uint8_t* out = frames + (size_t)k * (size_t)n_pix * 3;
  // each wave takes 64 consecutive chunks at a time: 3 KB of the film, staged in LDS and written as 192 contiguous 16-byte pieces
  // (pixels past the end of the film, in a partial last chunk, are evaluated and never stored)
  const int wv = tid >> 6, lane = tid & 63;
  uint4* stage = s_stage + wv * 3 * WAVE;
  for (long long cb = c0 + wv * WAVE; cb < c1; cb += 4 * WAVE) {
    const long long c = min(cb + lane, c1 - 1);  // (lanes past the end repeat the last chunk; only valid pieces are stored)
    const long long p0 = c * 16;
    const int v = (int)(p0 / W), u = (int)(p0 - (long long)v * W);
    const uint32_t bits = bg[c];
    uint32_t col[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) col[q] = ((bits >> q) & 1u) ? r.line_rgb : r.bg_rgb;
    // the chunk's pixels: one row, or the end of one row and the start of the next (W >= 16)
    const bool wraps = u + 15 >= W;
    const int cu0 = wraps ? 0 : u, cu1 = wraps ? W - 1 : u + 15, cv1 = wraps ? v + 1 : v;
    uint32_t open = 0xffffu;
    for (int j = n_ops - 1; j >= 0 && open; --j) {
      const ROp o = s_ops[j];
      if (o.u1 < cu0 || o.u0 > cu1 || o.v1 < v || o.v0 > cv1) continue;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        if (!((open >> q) & 1u)) continue;
        const int pu = u + q < W ? u + q : u + q - W, pv = u + q < W ? v : v + 1;
        bool edge;
        if (rd_hit(o, pu, pv, edge)) {
          col[q] = ((o.rgb >> 24) == 1u && edge) ? RD_CONTOUR : (o.rgb & 0xffffffu);
          open &= ~(1u << q);
        }
      }
    }
    // 16 pixels x 3 bytes = 12 words
    uint32_t w[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) w[q] = 0u;
#pragma unroll
    for (int q = 0; q < 16; ++q)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int byte = q * 3 + ch;
        w[byte >> 2] |= ((col[q] >> (8 * ch)) & 255u) << (8 * (byte & 3));
      }
    stage[lane * 3] = make_uint4(w[0], w[1], w[2], w[3]);
    stage[lane * 3 + 1] = make_uint4(w[4], w[5], w[6], w[7]);
    stage[lane * 3 + 2] = make_uint4(w[8], w[9], w[10], w[11]);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int nb = (int)min((long long)WAVE * 48, (n_pix - cb * 16) * 3);  // bytes of the film in this wave's chunks
    uint8_t* dst = out + (size_t)cb * 48;
    const int n16 = (reinterpret_cast<uintptr_t>(dst) & 15u) ? 0 : nb >> 4;  // whole aligned pieces, then the rest byte by byte
#pragma unroll
    for (int k2 = 0; k2 < 3; ++k2)
      if (lane + k2 * WAVE < n16) reinterpret_cast<uint4*>(dst)[lane + k2 * WAVE] = stage[lane + k2 * WAVE];
    for (int b = n16 * 16 + lane; b < nb; b += WAVE) dst[b] = reinterpret_cast<const uint8_t*>(stage)[b];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

struct pgd_render_state {
  pgd_render_config cfg;
  RenderDev r;
  int n_maps;
  bool stale;            // maps / scenarios were uploaded after pgd_render_enable: enable again
  double* geom;
  uint16_t* bg;
  uint32_t* lut;
  int32_t* d_ids;        // [N]
  int32_t* h_ids;        // pinned staging [N]
  hipEvent_t ev_ids;
  bool ids_pending;
};

// The fade table: row c, n frames, age i -> trunc(c + (i / n) * (255 - c)) per channel, in fp64 exactly as the reference's Python
// evaluates it (the library's fast-math flags are off here: no reciprocal, no re-association)
#ifndef __HIP_DEVICE_COMPILE__  // (host code: the device pass does not know the pragma)
#pragma float_control(precise, on, push)
#endif
static void render_fade_table(int S, std::vector<uint32_t>& lut) {
  lut.assign((size_t)RD_NCOL * (S + 1) * (S + 1), 0u);
  const uint8_t traffic[2][3] = {{100, 200, 255}, {200, 0, 150}};  // VehicleGraphics.BLUE, PURPLE
  for (int col = 0; col < RD_NCOL; ++col) {
    const uint8_t* base = col < 10 ? rd_palette[col] : traffic[col - 10];
    for (int n = 1; n <= S; ++n)
      for (int i = 0; i <= n; ++i) {
        uint32_t rgb = 0u;
        for (int ch = 0; ch < 3; ++ch) {
          const double cc = (double)base[ch];
          rgb |= (uint32_t)(int)(cc + ((double)i / (double)n) * (255.0 - cc)) << (8 * ch);
        }
        lut[((size_t)col * (S + 1) + n) * (S + 1) + i] = rgb;
      }
  }
}
#ifndef __HIP_DEVICE_COMPILE__
#pragma float_control(pop)
#endif

static void render_free(pgd_engine* h) {
  pgd_render_state* s = h->render;
  if (!s) return;
  (void)hipStreamSynchronize(h->stream);
  void* bufs[] = {s->geom, s->bg, s->lut, s->d_ids, s->r.ring, s->r.dead, s->r.env, s->r.ops};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  if (s->h_ids) (void)hipHostFree(s->h_ids);
  (void)hipEventDestroy(s->ev_ids);
  free(s);
  h->render = nullptr;
}

static void render_mark_stale(pgd_engine* h) { if (h->render) h->render->stale = true; }

static int render_forget(pgd_engine* h, const int32_t* d_env, int n) {
  if (!h->render) return PGD_OK;
  hipLaunchKernelGGL(k_render_forget, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->render->r.env, d_env, n);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

extern "C" {

int pgd_render_palette(uint8_t* out) {
  if (!out) return PGD_ERR_ARG;
  memcpy(out, rd_palette, sizeof(rd_palette));
  return PGD_OK;
}

int pgd_render_enable(pgd_handle h, const pgd_render_config* c, const double* h_film_geom) {
  if (!h || !c || !h_film_geom) return PGD_ERR_ARG;
  if (!h->have_maps || !h->have_scen || !h->h_maps) return PGD_ERR_STATE;
  const int W = c->film_w, H = c->film_h, S = c->num_stack, V = h->d.V;
  if (W < 16 || H < 16 || W > 16384 || H > 16384) return PGD_ERR_ARG;  // (a 16-pixel chunk spans at most two rows)
  if (S < 1 || S > 64 || c->history_smooth < 0 || (c->light_background != 0 && c->light_background != 1) ||
      (c->draw_traffic != 0 && c->draw_traffic != 1))
    return PGD_ERR_ARG;
  for (int ch = 0; ch < 3; ++ch)
    if (c->road_rgb[ch] < 0 || c->road_rgb[ch] > 255) return PGD_ERR_ARG;
  const int max_ops = S * V + RD_DEAD_CAP;
  if (max_ops > RD_MAX_OPS) return PGD_ERR_ARG;
  const int n_maps = (int)h->h_maps->size();
  for (int m = 0; m < n_maps; ++m)
    if (!(h_film_geom[3 * m] > 0.0)) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  render_free(h);
  pgd_render_state* s = (pgd_render_state*)calloc(1, sizeof(pgd_render_state));
  h->render = s;
  s->cfg = *c;
  s->n_maps = n_maps;
  const size_t N = (size_t)h->d.N;
  const long long words = ((long long)W * H + 15) / 16;
  HIPCHK(hipMalloc(&s->geom, sizeof(double) * 3 * (size_t)n_maps));
  HIPCHK(hipMalloc(&s->bg, sizeof(uint16_t) * (size_t)words * (size_t)n_maps));
  HIPCHK(hipMalloc(&s->lut, sizeof(uint32_t) * RD_NCOL * (size_t)(S + 1) * (S + 1)));
  HIPCHK(hipMalloc(&s->d_ids, sizeof(int32_t) * N));
  HIPCHK(hipHostMalloc(&s->h_ids, sizeof(int32_t) * N, hipHostMallocDefault));
  HIPCHK(hipEventCreateWithFlags(&s->ev_ids, hipEventDisableTiming));
  HIPCHK(hipMalloc(&s->r.ring, sizeof(RBox) * N * (size_t)S * V));
  HIPCHK(hipMalloc(&s->r.dead, sizeof(int2) * N * RD_DEAD_CAP));
  HIPCHK(hipMalloc(&s->r.env, sizeof(REnv) * N));
  HIPCHK(hipMalloc(&s->r.ops, sizeof(ROp) * N * (size_t)max_ops));
  std::vector<uint32_t> lut;
  render_fade_table(S, lut);
  HIPCHK(hipMemcpyAsync(s->lut, lut.data(), sizeof(uint32_t) * lut.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(s->geom, h_film_geom, sizeof(double) * 3 * (size_t)n_maps, hipMemcpyHostToDevice, h->stream));
  std::vector<REnv> env0(N);
  for (auto& q : env0) q = REnv{0, RD_FORGET, 0, 0, 0, {0, 0, 0}};
  HIPCHK(hipMemcpyAsync(s->r.env, env0.data(), sizeof(REnv) * N, hipMemcpyHostToDevice, h->stream));
  uint32_t line = 0u, back = c->light_background ? 0xffffffu : 0u;
  for (int ch = 0; ch < 3; ++ch) line |= (uint32_t)(c->light_background ? 255 - c->road_rgb[ch] : c->road_rgb[ch]) << (8 * ch);
  for (int m = 0; m < n_maps; ++m) {
    const double sc = h_film_geom[3 * m];
    const float line_r = (float)(0.5 * (double)(int)(1.0 * sc) / sc);  // half of pix(LANE_LINE_WIDTH = 1 m), in metres
    const int blocks = (int)std::min<long long>((words + 255) / 256, 4096);
    hipLaunchKernelGGL(k_render_bg, dim3(blocks), dim3(256), 0, h->stream, h->d, m, sc, h_film_geom[3 * m + 1], h_film_geom[3 * m + 2], line_r,
                       s->bg + (size_t)m * words, W, H);
  }
  HIPCHK(hipGetLastError());
  s->r = RenderDev{W, H, S, c->history_smooth, c->draw_traffic, back, line, s->geom, s->bg, words, s->lut, s->r.ring, s->r.dead, s->r.env,
                   s->r.ops, max_ops};
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_render_frame), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)(sizeof(ROp) * RD_MAX_OPS)));
  HIPCHK(hipStreamSynchronize(h->stream));
  return PGD_OK;
}

int pgd_render_topdown(pgd_handle h, const int32_t* h_env_ids, int n, uint8_t* d_frames) {
  if (!h || !d_frames) return PGD_ERR_ARG;
  pgd_render_state* s = h->render;
  if (!s || s->stale || !h->have_maps || !h->have_scen) return PGD_ERR_STATE;
  if (reinterpret_cast<uintptr_t>(d_frames) & 15u) return PGD_ERR_ARG;  // (written sixteen bytes at a time)
  const int N = h->d.N;
  if (!h_env_ids) n = N;
  if (n <= 0 || n > N) return PGD_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  int32_t* d_env = nullptr;
  if (h_env_ids) {  // in range and no env twice (each env's history is advanced by one wave)
    std::vector<uint8_t> seen((size_t)N, 0);
    for (int k = 0; k < n; ++k) {
      const int e = h_env_ids[k];
      if (e < 0 || e >= N || seen[(size_t)e]) return PGD_ERR_ARG;
      seen[(size_t)e] = 1;
    }
    if (s->ids_pending) { HIPCHK(hipEventSynchronize(s->ev_ids)); s->ids_pending = false; }
    memcpy(s->h_ids, h_env_ids, sizeof(int32_t) * (size_t)n);
    HIPCHK(hipMemcpyAsync(s->d_ids, s->h_ids, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(h->stream, &cap);
    if (cap == hipStreamCaptureStatusNone) { HIPCHK(hipEventRecord(s->ev_ids, h->stream)); s->ids_pending = true; }
    d_env = s->d_ids;
  }
  const RenderDev r = s->r;
  hipLaunchKernelGGL(k_render_prep, dim3(n), dim3(WAVE), 0, h->stream, h->d, r, d_env);
  const long long n_chunks = ((long long)r.W * r.H + 15) / 16;
  const dim3 grid((unsigned)((n_chunks + RD_CHUNKS - 1) / RD_CHUNKS), (unsigned)n);
  hipLaunchKernelGGL(k_render_frame, grid, dim3(256), sizeof(ROp) * (size_t)r.max_ops, h->stream, r, d_env, d_frames);
  HIPCHK(hipGetLastError());
  return PGD_OK;
}

}  // extern "C"

#endif
