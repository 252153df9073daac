// tools/xlane_cost.hip -- what does a wave pay per DEPENDENT use of an LDS read or a cross-lane move on gfx950?
//
// The heavy waves of k_step run chains of LDS reads that are waited for on the spot, and `__shfl` compiles to ds_bpermute_b32, which
// goes through the LDS pipe as well.  This program prices them: every wave runs a chain in which each operation's result feeds the
// next one (through one v_add_u32, the "use"), W = 1 and 4 waves per SIMD on every CU, timed with s_memtime inside the wave.
//
//   hipcc -O2 --offload-arch=gfx950 tools/xlane_cost.hip -o /tmp/xlane_cost && /tmp/xlane_cost > profiles/lds_xlane_cost.txt
//
// Rows: the v_add_u32 chain alone (what the "use" costs: subtract it), ds_read_b32, ds_read2st64_b32, one ds_bpermute_b32, a batch of
// four independent ds_bpermute_b32 combined by three v_or (the shape of group_or / group_min in pgd_vehicle.h), one DPP row move,
// and the same group-of-three combine on DPP: row_shr:1 / row_shr:2 / row_shl:1 / row_shl:2 moves, four selects on the sub-lane
// index and two v_or.  cyc/op = cycles of the wave's life per link of the chain.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

enum Op { ADD_ONLY, DS_READ, DS_READ2ST64, BPERM_1, BPERM_4, DPP_1, DPP_GROUP3, NOP };
static const char* OPNAME[NOP] = {
    "v_add_u32 alone (the use)",
    "ds_read_b32 + use",
    "ds_read2st64_b32 + use",
    "ds_bpermute_b32 + use",
    "4 x ds_bpermute_b32 (independent) + 3 v_or",
    "dpp row_shr:1 move + use",
    "dpp group of 3: 4 row moves + 4 selects + 2 v_or",
};
#define REP 32        // links per loop body
#define LDS_WORDS 2048  // [0, 1024): word i holds its own byte address; [1024, 2048): zeros

template <int OP>
__global__ void __launch_bounds__(1024) k_chain(unsigned long long* out, int iters, unsigned zero)
{
    __shared__ unsigned lds[LDS_WORDS];
    for (int i = threadIdx.x; i < LDS_WORDS; i += blockDim.x) lds[i] = i < 1024 ? (unsigned)i * 4u : 0u;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned lane = threadIdx.x & 63u;
    unsigned v = (threadIdx.x & 1023u) * 4u;  // a byte address inside the first half of `lds`, and the chain's value
    // bpermute addresses: lead of the lane's group of three (clamped to the wave), and its members
    const unsigned lead = (lane / 3u) * 3u;
    const unsigned a0 = lead * 4u, a1 = min(lead + 1u, 63u) * 4u, a2 = min(lead + 2u, 63u) * 4u;
    const unsigned self = lane * 4u;
    const unsigned sub = lane - lead;
    unsigned long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < iters; ++it) {
        if (OP == ADD_ONLY) {
            asm volatile(".rept 32\n v_add_u32 %0, %0, %1\n .endr" : "+v"(v) : "v"(zero));
        } else if (OP == DS_READ) {
            unsigned t;
            asm volatile(".rept 32\n ds_read_b32 %1, %0\n s_waitcnt lgkmcnt(0)\n v_add_u32 %0, %1, %2\n .endr" : "+v"(v), "=&v"(t) : "v"(zero) : "memory");
        } else if (OP == DS_READ2ST64) {  // second word: + 16 * 64 dwords = the zero half
            asm volatile(".rept 32\n ds_read2st64_b32 v[100:101], %0 offset1:16\n s_waitcnt lgkmcnt(0)\n v_add_u32 %0, v100, v101\n .endr"
                         : "+v"(v) : : "memory", "v100", "v101");
        } else if (OP == BPERM_1) {
            unsigned t;
            asm volatile(".rept 32\n ds_bpermute_b32 %1, %2, %0\n s_waitcnt lgkmcnt(0)\n v_add_u32 %0, %1, %3\n .endr" : "+v"(v), "=&v"(t) : "v"(self), "v"(zero));
        } else if (OP == BPERM_4) {
            unsigned p, q, r, s;
            asm volatile(".rept 32\n"
                "ds_bpermute_b32 %1, %5, %0\n ds_bpermute_b32 %2, %6, %0\n ds_bpermute_b32 %3, %7, %0\n ds_bpermute_b32 %4, %7, %0\n"
                "s_waitcnt lgkmcnt(0)\n v_or_b32 %1, %1, %2\n v_or_b32 %3, %3, %4\n v_or_b32 %0, %1, %3\n .endr"
                : "+v"(v), "=&v"(p), "=&v"(q), "=&v"(r), "=&v"(s) : "v"(a0), "v"(a1), "v"(a2));
        } else if (OP == DPP_1) {
#pragma unroll
            for (int k = 0; k < REP; ++k) v = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false) + zero;
        } else if (OP == DPP_GROUP3) {
#pragma unroll
            for (int k = 0; k < REP; ++k) {
                // a lane's two partners: sub 0 takes lanes +1, +2 (row_shl), sub 1 takes -1, +1, sub 2 takes -1, -2 (row_shr)
                const unsigned up1 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xf, 0xf, false);
                const unsigned up2 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x102, 0xf, 0xf, false);
                const unsigned dn1 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
                const unsigned dn2 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
                const unsigned x = sub == 0u ? up1 : dn1, y = sub == 0u ? up2 : (sub == 1u ? up1 : dn2);
                v = (v | x | y) + zero;
            }
        }
    }
    unsigned long long t1 = __builtin_readcyclecounter();
    if (v == 0xdeadbeefu) lds[0] = v;  // keeps the chain alive
    if (lane == 0) out[(size_t)blockIdx.x * (blockDim.x >> 6) + wave] = t1 - t0;
    if (lds[0] == 0xffffffffu) out[0] = 0;
}

typedef void (*kern_t)(unsigned long long*, int, unsigned);
static kern_t KERN[NOP] = {k_chain<ADD_ONLY>, k_chain<DS_READ>, k_chain<DS_READ2ST64>, k_chain<BPERM_1>, k_chain<BPERM_4>, k_chain<DPP_1>,
                           k_chain<DPP_GROUP3>};

int main(int argc, char** argv)
{
    int iters = argc > 1 ? atoi(argv[1]) : 500;
    hipDeviceProp_t p;
    CK(hipGetDeviceProperties(&p, 0));
    const int cus = p.multiProcessorCount;
    printf("# %s, %d CUs; %d iterations of %d links per wave\n", p.gcnArchName, cus, iters, REP);
    printf("# cyc/op = s_memtime ticks of the wave's loop / links (shader cycles), mean and maximum over the waves of the launch;\n");
    printf("# loop control (3 scalar instructions per %d links) is included.  W = waves per SIMD on every CU.\n", REP);
    const size_t max_waves = (size_t)cus * 16;
    unsigned long long* d;
    CK(hipMalloc(&d, sizeof(unsigned long long) * max_waves));
    std::vector<unsigned long long> h(max_waves);
    printf("%-52s %3s %10s %10s\n", "chain link", "W", "cyc/op", "max");
    for (int op = 0; op < NOP; ++op) {
        for (int W : {1, 4}) {
            const int threads = W * 256, blocks = cus;  // W waves per SIMD: one block of 4 W waves per CU
            const size_t waves = (size_t)blocks * threads / 64;
            for (int rep = 0; rep < 3; ++rep) {  // the last launch is the one read
                hipLaunchKernelGGL(KERN[op], dim3(blocks), dim3(threads), 0, 0, d, iters, 0u);
                CK(hipGetLastError());
                CK(hipDeviceSynchronize());
            }
            CK(hipMemcpy(h.data(), d, sizeof(unsigned long long) * waves, hipMemcpyDeviceToHost));
            double sum = 0, mx = 0;
            for (size_t i = 0; i < waves; ++i) { sum += (double)h[i]; mx = std::max(mx, (double)h[i]); }
            const double links = (double)iters * REP;
            printf("%-52s %3d %10.2f %10.2f\n", OPNAME[op], W, sum / waves / links, mx / links);
        }
    }
    CK(hipFree(d));
    return 0;
}
