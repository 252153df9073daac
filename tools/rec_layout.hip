// Record layout of an env's vehicle block and what it costs at the start (loads) and at the end (stores) of a step's launch:
// one wave per env, lane -> vehicle as k_step maps them (V = 17: three lanes per vehicle; V = 40: one), eight 16-byte pieces per
// 128-byte record.  "line per vehicle" = piece k of slot s at (s * 8 + k) * 16 (an instruction touches V cache lines);
// "piece planes" = piece k of slot s at (k * V + s) * 16 (an instruction touches V * 16 / 128 lines).  Same bytes, same DRAM pages.
// `rec_layout burst`: the record burst of piece planes priced three ways (profiles/burst_notes.md) -- A: the eight plane reads as they
// are; B: ceil(8 V / 64) full-width reads of the env's contiguous block, ds_write_b128, eight ds_read_b128 per lane; C: the same reads
// as LDS-DMA (global_load_lds_dwordx4), eight ds_read_b128.  The kernel carries k_step's LDS (8,976 bytes) and register class (<= 128).
// hipcc --offload-arch=gfx950 -O2 -o rec_layout tools/rec_layout.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
struct Dev { int* ei; uint4* rec; unsigned long long* out; int planes; int V; int sub; int store; int lead; };
__global__ __launch_bounds__(64, 4) void k(Dev d) {
  const int e = blockIdx.x, lane = threadIdx.x, V = d.V;
  long long t0 = clock64();
  int scen = d.ei[e * 8];
  const int s = lane / d.sub; const bool valid = s < V;
  uint4 r[8] = {};
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  if (scen == 12345) return;
  long long t1 = clock64();
  const uint4* blk = d.rec + (size_t)e * V * 8 + (scen & 1);
  const int ss = d.planes ? 1 : 8, ks = d.planes ? V : 1;
  // lead = 1: only the first lane of a vehicle's group reads; lead = 2: ... and hands the record to the group's other lanes (bpermute)
  if (valid && (d.lead == 0 || lane % d.sub == 0)) {
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) r[k2] = blk[s * ss + k2 * ks];
  }
  if (d.lead == 2) {
    const int src = (lane - lane % d.sub) * 4;
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) {
      r[k2].x = __builtin_amdgcn_ds_bpermute(src, r[k2].x); r[k2].y = __builtin_amdgcn_ds_bpermute(src, r[k2].y);
      r[k2].z = __builtin_amdgcn_ds_bpermute(src, r[k2].z); r[k2].w = __builtin_amdgcn_ds_bpermute(src, r[k2].w);
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  unsigned acc = 0;
  if (valid) for (int k2 = 0; k2 < 8; ++k2) acc += r[k2].x ^ r[k2].w;
  long long t2 = clock64();
  if (acc == 0x12345678u) d.out[0] = 1;
  // a stand-in for the step: ~6 us of dependent arithmetic
  float f = (float)acc;
  for (int i = 0; i < 600; ++i) f = __builtin_fmaf(f, 1.0001f, 0.5f);
  if (f == 3.25f) d.out[1] = 1;
  long long t3 = clock64();
  if (d.store && valid && lane % d.sub == 0) {
    uint4* w = d.rec + (size_t)e * V * 8;
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) w[s * ss + k2 * ks] = r[k2];
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  long long t4 = clock64();
  if (lane == 0) {
    d.ei[e * 8] = scen;
    unsigned long long* o = d.out + 8 + e * 4;
    o[0] += (unsigned long long)(t1 - t0); o[1] += (unsigned long long)(t2 - t1); o[2] += (unsigned long long)(t4 - t3);
  }
}
// the burst variants: MODE 0 = A, 1 = B, 2 = C, with the lanes past the block's end masked in the last read; 3 / 4 = B / C with those
// lanes reading the block's last piece again instead (no exec mask, no branch: staged into the unused pieces behind the block's image)
#define STEP_LDS_BYTES 8976   // k_step<true,false,false,true,1,false>: group_segment_fixed_size
#define MAX_PIECES 512        // 8 x 64 slots
// V, the lanes per vehicle and ROUNDS = ceil(8 V / 64) are literals, as they are in k_step's specialised instantiations: a short head in
// front of the first read (as run-time values the lane -> vehicle division put ~100 VALU instructions there, and four waves per SIMD
// queueing for those moved "records arrive after" more than anything the memory path did), every read but the last unmasked
template <int MODE, int V> __global__ __launch_bounds__(64, 4) void kb(Dev d) {
  constexpr int P = 8 * V, ROUNDS = (P + 63) / 64, SUB = 64 / V;
  __shared__ uint4 stage[STEP_LDS_BYTES / 16];
  static_assert(MAX_PIECES <= STEP_LDS_BYTES / 16, "the staging area lies inside the step's LDS");
  const int e = blockIdx.x, lane = threadIdx.x;
  const int s = lane / SUB; const bool valid = s < V;
  uint4 r[8] = {};
  long long t1 = clock64();
  const uint4* blk = d.rec + (size_t)e * P;
  const bool last = (ROUNDS - 1) * 64 + lane < P;  // lanes past the block's end read nothing
  if (MODE == 0) {
    if (valid) {
#pragma unroll
      for (int k2 = 0; k2 < 8; ++k2) r[k2] = blk[k2 * V + s];
    }
  } else {
    if (MODE == 3 || MODE == 4) {
      uint4 t[ROUNDS];
#pragma unroll
      for (int j = 0; j < ROUNDS; ++j) {
        const uint4* src = blk + min(j * 64 + lane, P - 1);
        if (MODE == 3) t[j] = *src;
        else __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)(stage + j * 64), 16, 0, 0);
      }
      if (MODE == 3) {
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) stage[j * 64 + lane] = t[j];
      } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else if (MODE == 1) {
      uint4 t[ROUNDS];
#pragma unroll
      for (int j = 0; j < ROUNDS - 1; ++j) t[j] = blk[j * 64 + lane];
      if (last) t[ROUNDS - 1] = blk[(ROUNDS - 1) * 64 + lane];
#pragma unroll
      for (int j = 0; j < ROUNDS - 1; ++j) stage[j * 64 + lane] = t[j];
      if (last) stage[(ROUNDS - 1) * 64 + lane] = t[ROUNDS - 1];
    } else {
#pragma unroll
      for (int j = 0; j < ROUNDS; ++j)
        if (j < ROUNDS - 1 || last)
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(blk + j * 64 + lane),
                                           (__attribute__((address_space(3))) void*)(stage + j * 64), 16, 0, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (valid) {
#pragma unroll
      for (int k2 = 0; k2 < 8; ++k2) r[k2] = stage[k2 * V + s];
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  unsigned acc = 0;
  if (valid) for (int k2 = 0; k2 < 8; ++k2) acc += r[k2].x ^ r[k2].w ^ r[k2].y ^ r[k2].z;
  long long t2 = clock64();
  if (acc != d.lead + (valid ? 8u * (unsigned)(e * 64 + s) : 0u)) d.out[0] = 1;  // (lead = 0 here) every lane got its own record
  float f = (float)acc;
  for (int i = 0; i < 600; ++i) f = __builtin_fmaf(f, 1.0001f, 0.5f);
  if (f == 3.25f) d.out[1] = 1;
  if (lane == 0) d.out[8 + e * 4 + 1] += (unsigned long long)(t2 - t1);
}
static int burst(Dev d, int N) {
  // piece k of slot s of env e holds x = e * 64 + s and y ^ z ^ w = 0: acc = 8 (e * 64 + s)
  for (int V : {17, 40}) {
    std::vector<uint4> h((size_t)N * V * 8);
    for (int e = 0; e < N; ++e) for (int k = 0; k < 8; ++k) for (int s = 0; s < V; ++s) h[((size_t)e * 8 + k) * V + s] = uint4{(unsigned)(e * 64 + s), (unsigned)k, 0x55u, (unsigned)k ^ 0x55u};
    hipMemcpy(d.rec, h.data(), h.size() * 16, hipMemcpyHostToDevice);
    d.planes = 1; d.V = V; d.sub = V == 17 ? 3 : 1; d.store = 0; d.lead = 0;
    for (int waves : {4096, 256}) {
      const int REPS = 7, n = 500;
      const int NM = 5;
      float us[NM][REPS]; double cyc[NM][REPS], slow[NM][REPS]; unsigned long long bad = 0;
      for (int rep = -1; rep < REPS; ++rep) for (int mi = 0; mi < NM; ++mi) {  // (rep -1: a pass that is not counted -- the clocks settle)
        const int mode = rep & 1 ? NM - 1 - mi : mi;  // order reversed every repetition
        auto launch = [&]() {
#define KB_LAUNCH(R) switch (mode) { case 0: kb<0, R><<<waves, 64>>>(d); break; case 1: kb<1, R><<<waves, 64>>>(d); break; case 2: kb<2, R><<<waves, 64>>>(d); break; \
                                     case 3: kb<3, R><<<waves, 64>>>(d); break; default: kb<4, R><<<waves, 64>>>(d); }
          if (V == 17) { KB_LAUNCH(17) } else { KB_LAUNCH(40) }
        };
        for (int i = 0; i < 50; ++i) launch();
        hipMemset(d.out, 0, 64 + N * 32);
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        hipEventRecord(e0);
        for (int i = 0; i < n; ++i) launch();
        hipEventRecord(e1); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        std::vector<unsigned long long> ob(8 + N * 4); hipMemcpy(ob.data(), d.out, 64 + N * 32, hipMemcpyDeviceToHost);
        unsigned long long c = 0, cmax = 0; for (int b = 0; b < waves; ++b) { c += ob[9 + b * 4]; cmax = std::max(cmax, ob[9 + b * 4]); }
        bad += ob[0];
        hipEventDestroy(e0); hipEventDestroy(e1);
        if (rep < 0) continue;
        us[mode][rep] = ms / n * 1e3f; cyc[mode][rep] = (double)c / n / waves; slow[mode][rep] = (double)cmax / n;
      }
      for (int mode = 0; mode < NM; ++mode) {
        std::sort(us[mode], us[mode] + REPS); std::sort(cyc[mode], cyc[mode] + REPS); std::sort(slow[mode], slow[mode] + REPS);
        printf("V %2d waves %4d %s: records arrive after %5.0f [%5.0f .. %5.0f] cycles (slowest block %5.0f); launch %6.3f [%6.3f .. %6.3f] us (median [min .. max] of %d)\n", V, waves,
               mode == 0 ? "A plane reads        " : mode == 1 ? "B reads+ds_write     " : mode == 2 ? "C LDS-DMA            " : mode == 3 ? "B', no masked lanes  " : "C', no masked lanes  ", cyc[mode][REPS / 2], cyc[mode][0], cyc[mode][REPS - 1], slow[mode][REPS / 2],
               us[mode][REPS / 2], us[mode][0], us[mode][REPS - 1], REPS);
      }
      if (bad) { printf("WRONG RECORDS in some lane (V %d waves %d)\n", V, waves); return 1; }
    }
  }
  return 0;
}
int main(int argc, char** argv) {
  const int N = 4096;
  Dev d{}; hipMalloc(&d.ei, N * 8 * 4); hipMalloc(&d.rec, (size_t)N * 40 * 128 + 64); hipMalloc(&d.out, 64 + N * 32);
  hipMemset(d.ei, 0, N * 8 * 4); hipMemset(d.rec, 0, (size_t)N * 40 * 128 + 64);
  if (argc > 1 && !strcmp(argv[1], "burst")) return burst(d, N);
  for (int rep = 0; rep < 2; ++rep)
  for (int V : {17, 40}) for (int waves : {4096, 256}) for (int store : {0, 1}) for (int planes : {0, 1}) for (int lead : {0, 1, 2}) {
    if (lead && (V != 17 || !planes)) continue;
    d.planes = planes; d.V = V; d.sub = V == 17 ? 3 : 1; d.store = store; d.lead = lead;
    for (int i = 0; i < 50; ++i) k<<<waves, 64>>>(d);
    hipMemset(d.out, 0, 64 + N * 32);
    const int n = 500;
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0);
    for (int i = 0; i < n; ++i) k<<<waves, 64>>>(d);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    std::vector<unsigned long long> ob(8 + N * 4); hipMemcpy(ob.data(), d.out, 64 + N * 32, hipMemcpyDeviceToHost);
    unsigned long long o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < waves; ++b) { o[2] += ob[8 + b * 4]; o[3] += ob[9 + b * 4]; o[4] += ob[10 + b * 4]; }
    printf("V %2d waves %4d %-16s lead %d %-9s: launch %6.2f us; env word after %5.0f cycles, records after another %5.0f, stores waited for %5.0f\n", V, waves,
           planes ? "piece planes" : "line per vehicle", lead, store ? "stores" : "no stores", ms / n * 1e3, (double)o[2] / n / waves, (double)o[3] / n / waves, (double)o[4] / n / waves);
  }
  return 0;
}
