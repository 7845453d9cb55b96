// Micro-benchmark of the building blocks on the critical path of lp_window_kernel: cycles per
//   (a) s_barrier alone, (b) ds_write_b64 + barrier + ds_read_b64 (one LDS hand-over), (c) the 64-lane f64 butterfly (6 DPP steps),
//   (d) one IEEE f64 division, (e) a dependent chain of f64 additions, (f) a random 64-lane ds_read_b64 gather + add chain of L entries.
// One 512-thread workgroup per CU (256 workgroups), 2 waves per SIMD as in the solver.  Build: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

template <int CTRL> __device__ __forceinline__ double dpp_mov(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, true);
    hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double butterfly(double v) {
    v = v + __shfl_xor(v, 32, 64);
    v = v + __shfl_xor(v, 16, 64);
    v = v + dpp_mov<0xB1>(v); v = v + dpp_mov<0x4E>(v); v = v + dpp_mov<0x141>(v); v = v + dpp_mov<0x140>(v);
    return v;
}

template <int MODE, int L>
__global__ void __launch_bounds__(512) k(double *out, unsigned long long *cyc, const unsigned short *idx, int iters, double seed) {
    __shared__ double buf[1024];
    const int tid = threadIdx.x;
    double v = seed + tid * 1e-3, w = seed * 0.5 + 1.0;
    buf[tid] = v; buf[tid + 512] = w;
    unsigned a[L > 0 ? L : 1];
    for (int q = 0; q < L; q++) a[q] = idx[(blockIdx.x % 8) * 512 * 32 + q * 512 + tid];
    __syncthreads();
    unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; it++) {
        if (MODE == 0) { __builtin_amdgcn_s_barrier(); }
        if (MODE == 1) { buf[tid] = v; __syncthreads(); v = buf[(tid + 64) & 511] + 1.0; __syncthreads(); }   // two hand-overs
        if (MODE == 2) { v = butterfly(v) * 0.015625; }
        if (MODE == 3) { v = w / v + 1.5; }
        if (MODE == 4) {
#pragma unroll
            for (int q = 0; q < 16; q++) v = v + w;
        }
        if (MODE == 5) {
            double g[L > 0 ? L : 1];
#pragma unroll
            for (int q = 0; q < L; q++) g[q] = buf[a[q]];
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < L; q++) acc = acc + g[q];
            v = acc * 0.1;
            __syncthreads(); buf[tid] = v; __syncthreads();
        }
        if (MODE == 6) { __syncthreads(); buf[tid] = v; __syncthreads(); v = v * 0.5; }       // the hand-over part of MODE 5 alone
    }
    unsigned long long t1 = __builtin_amdgcn_s_memtime();
    out[blockIdx.x * 512 + tid] = v;
    if (tid == 0) cyc[blockIdx.x] = t1 - t0;
}

// The two LDS hand-overs of the solver's PCG iteration as dependent chains, with the barrier in both forms ("LDS
// hand-overs"): BARE = false is __syncthreads() (s_waitcnt lgkmcnt(0) in front of s_barrier), BARE = true the bare s_barrier between
// compiler-only memory barriers (lds_handover() of csrc/lpbox_dev_common.h).  One hand-over per round on ping-pong buffers; the value a
// lane writes in round r + 1 depends on what it read in round r.
//   KIND 0 "vector": every lane writes an f64, barrier, reads eight gathered entries and adds them in order
//   KIND 1 "block_sum": lane 0 of each wave writes an f64, barrier, every lane does one ds_read_b128 and adds the pair
template <bool BARE> __device__ __forceinline__ void bar() {
    if constexpr (BARE) { asm volatile("" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); }
    else __syncthreads();
}
template <int KIND, bool BARE>
__global__ void __launch_bounds__(512) kh(double *out, unsigned long long *cyc, const unsigned short *idx, int iters, double seed) {
    __shared__ __attribute__((aligned(16))) double buf[2][512];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double v = seed + tid * 1e-3;
    unsigned a[8];
    for (int q = 0; q < 8; q++) a[q] = idx[(blockIdx.x % 8) * 512 * 32 + q * 512 + tid] & 511;
    buf[0][tid] = 0.0; buf[1][tid] = 0.0;
    __syncthreads();
    unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; it++) {
        double *b = buf[it & 1];
        if (KIND == 0) {
            b[tid] = v;
            bar<BARE>();
            double g[8];
#pragma unroll
            for (int q = 0; q < 8; q++) g[q] = b[a[q]];
            double acc = g[0];
#pragma unroll
            for (int q = 1; q < 8; q++) acc = acc + g[q];
            v = acc * 0.125;
        } else {
            if (lane == 0) b[w] = v;
            bar<BARE>();
            const double2 t = *(const double2 *)(b + 2 * (lane & 3));
            v = (t.x + t.y) * 0.5 + 1e-3;
        }
    }
    unsigned long long t1 = __builtin_amdgcn_s_memtime();
    out[blockIdx.x * 512 + tid] = v;
    if (tid == 0) cyc[blockIdx.x] = t1 - t0;
}

// Reduction steps on f64 arithmetic with a row_newbcast operand ("Row-broadcast reduction steps"), each as a
// dependent chain per round, all 64 lanes active.  gfx950 has no v_add_f64_dpp; the addition of a broadcast value is
// v_fmac_f64_dpp acc, bcast(x), 1.0 (exact product, one rounding: the addition's bits).
//   KIND 0 / 1  the row finish of block_sum's first stage: two quad_perm levels, then row_half_mirror + row_mirror (0) or three
//               v_fmac_f64_dpp (1, right in lane 0 of a row only; the other lanes carry finite garbage along the chain)
//   KIND 2 / 3 / 4  the second stage behind a bare-barrier hand-over: pair read + two quad_perm levels (2), pair read + two broadcast
//               moves + two v_fmac_f64_dpp + add (3, S2a), two ds_read_b128 + three adds + one quad_perm level (4, S2b)
//   KIND 5 .. 8  16 dependent operations: plain v_add_f64 (5), v_add_f64 behind the two wait states a DPP read needs (6), v_fmac_f64
//               behind them (7), v_fmac_f64_dpp row_newbcast:0 behind them (8) -- 8 minus 7 is the cost of the DPP operand itself
template <int N> __device__ __forceinline__ double row_bcast(double v) { return __builtin_amdgcn_update_dpp(v, v, 0x150 + N, 0xf, 0xf, false); }
__device__ __forceinline__ double row_finish_mirror(double v) {
    v = v + dpp_mov<0xB1>(v); v = v + dpp_mov<0x4E>(v); v = v + dpp_mov<0x141>(v); v = v + dpp_mov<0x140>(v);
    return v;
}
__device__ __forceinline__ double row_finish_lane0(double v) {
    v = v + dpp_mov<0xB1>(v); v = v + dpp_mov<0x4E>(v);
    double a = v, b = v;
    asm("s_nop 1\n\t"
        "v_fmac_f64_dpp %1, %0, %2 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %0, %2 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 0\n\t"
        "v_fmac_f64_dpp %0, %1, %2 row_newbcast:8 row_mask:0xf bank_mask:0xf"
        : "+v"(a), "+v"(b) : "v"(1.0));
    return a;
}
template <int KIND>
__global__ void __launch_bounds__(512) kr(double *out, unsigned long long *cyc, const unsigned short *, int iters, double seed) {
    __shared__ __attribute__((aligned(16))) double buf[2][16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double v = seed + tid * 1e-3;
    const double c = seed * 1e-3;
    if (tid < 16) { buf[0][tid] = 0.0; buf[1][tid] = 0.0; }
    __syncthreads();
    unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; it++) {
        if (KIND == 0) v = row_finish_mirror(v) * 0.0625;
        if (KIND == 1) v = row_finish_lane0(v) * 0.0625;
        if (KIND >= 2 && KIND <= 4) {
            double *b = buf[it & 1];
            if (lane == 0) b[w] = v;
            bar<true>();
            double tot;
            if (KIND == 4) {
                const double2 *q = (const double2 *)(b + 4 * (lane & 1));
                const double2 p0 = q[0], p1 = q[1];
                const double u = (p0.x + p0.y) + (p1.x + p1.y);
                tot = u + dpp_mov<0xB1>(u);
            } else {
                const double2 t = *(const double2 *)(b + 2 * (lane & 3));
                double u = t.x + t.y;
                if (KIND == 2) { u = u + dpp_mov<0xB1>(u); tot = u + dpp_mov<0x4E>(u); }
                else {
                    double a = row_bcast<0>(u), bb = row_bcast<2>(u);
                    asm("s_nop 1\n\t"
                        "v_fmac_f64_dpp %0, %2, %3 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                        "v_fmac_f64_dpp %1, %2, %3 row_newbcast:3 row_mask:0xf bank_mask:0xf"
                        : "+v"(a), "+v"(bb) : "v"(u), "v"(1.0));
                    tot = a + bb;
                }
            }
            v = tot * 0.125 + 1e-3;
        }
        if (KIND == 5) {
#pragma unroll
            for (int q = 0; q < 16; q++) asm volatile("v_add_f64 %0, %0, %1" : "+v"(v) : "v"(c));
        }
        if (KIND == 6) {
#pragma unroll
            for (int q = 0; q < 16; q++) asm volatile("s_nop 1\n\tv_add_f64 %0, %0, %1" : "+v"(v) : "v"(c));
        }
        if (KIND == 7) {
#pragma unroll
            for (int q = 0; q < 16; q++) asm volatile("s_nop 1\n\tv_fmac_f64 %0, %1, %2" : "+v"(v) : "v"(c), "v"(1.0));
        }
        if (KIND == 8) {
#pragma unroll
            for (int q = 0; q < 16; q++) asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %0, %1 row_newbcast:0 row_mask:0xf bank_mask:0xf" : "+v"(v) : "v"(c));
        }
    }
    unsigned long long t1 = __builtin_amdgcn_s_memtime();
    out[blockIdx.x * 512 + tid] = v;
    if (tid == 0) cyc[blockIdx.x] = t1 - t0;
}

#define RUNR(KIND, name, per)                                                                                           \
    {                                                                                                                   \
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);                                                    \
        kr<KIND><<<256, 512>>>(out, cyc, idx, 100, 1.25);                                                               \
        hipEventRecord(e0); kr<KIND><<<256, 512>>>(out, cyc, idx, iters, 1.25); hipEventRecord(e1);                     \
        hipDeviceSynchronize(); float ms; hipEventElapsedTime(&ms, e0, e1);                                             \
        unsigned long long h[256]; hipMemcpy(h, cyc, sizeof(h), hipMemcpyDeviceToHost);                                 \
        double s = 0; for (int i = 0; i < 256; i++) s += h[i];                                                          \
        printf("%-46s %8.1f cycles  %7.1f ns  (clock %.2f GHz)\n", name, s / 256 / iters / per, 1e6 * ms / iters / per, \
               s / 256 / (ms * 1e6));                                                                                   \
    }

#define RUNH(KIND, BARE, name)                                                                                         \
    {                                                                                                                   \
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);                                                    \
        kh<KIND, BARE><<<256, 512>>>(out, cyc, idx, 100, 1.25);                                                         \
        hipEventRecord(e0); kh<KIND, BARE><<<256, 512>>>(out, cyc, idx, iters, 1.25); hipEventRecord(e1);               \
        hipDeviceSynchronize(); float ms; hipEventElapsedTime(&ms, e0, e1);                                             \
        unsigned long long h[256]; hipMemcpy(h, cyc, sizeof(h), hipMemcpyDeviceToHost);                                 \
        double s = 0; for (int i = 0; i < 256; i++) s += h[i];                                                          \
        printf("%-46s %8.1f cycles  %7.1f ns  (clock %.2f GHz)\n", name, s / 256 / iters, 1e6 * ms / iters,             \
               s / 256 / (ms * 1e6));                                                                                   \
    }

#define RUN(MODE, L, name, per)                                                                                        \
    {                                                                                                                   \
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);                                                    \
        k<MODE, L><<<256, 512>>>(out, cyc, idx, 100, 1.25);                                                             \
        hipEventRecord(e0); k<MODE, L><<<256, 512>>>(out, cyc, idx, iters, 1.25); hipEventRecord(e1);                   \
        hipDeviceSynchronize(); float ms; hipEventElapsedTime(&ms, e0, e1);                                             \
        unsigned long long h[256]; hipMemcpy(h, cyc, sizeof(h), hipMemcpyDeviceToHost);                                 \
        double s = 0; for (int i = 0; i < 256; i++) s += h[i];                                                          \
        printf("%-46s %8.1f cycles  %7.1f ns  (clock %.2f GHz)\n", name, s / 256 / iters / per, 1e6 * ms / iters / per, \
               s / 256 / (ms * 1e6));                                                                                   \
    }

int main() {
    const int iters = 20000;
    double *out; unsigned long long *cyc; unsigned short *idx;
    hipMalloc(&out, 256 * 512 * 8); hipMalloc(&cyc, 256 * 8); hipMalloc(&idx, 8 * 512 * 32 * 2);
    unsigned short *h = (unsigned short *)malloc(8 * 512 * 32 * 2);
    srand(1); for (int i = 0; i < 8 * 512 * 32; i++) h[i] = rand() % 1000;
    hipMemcpy(idx, h, 8 * 512 * 32 * 2, hipMemcpyHostToDevice);
    RUN(0, 0, "s_barrier (8 waves)", 1)
    RUN(1, 0, "ds_write+barrier+ds_read hand-over", 2)
    RUN(2, 0, "64-lane f64 butterfly (6 steps) + mul", 1)
    RUN(3, 0, "f64 division + add", 1)
    RUN(4, 0, "dependent f64 add", 16)
    RUN(6, 0, "barrier+ds_write+barrier (gather frame)", 1)
    RUN(5, 4, "frame + random gather L=4 + add chain", 1)
    RUN(5, 8, "frame + random gather L=8 + add chain", 1)
    RUN(5, 12, "frame + random gather L=12 + add chain", 1)
    RUN(5, 16, "frame + random gather L=16 + add chain", 1)
    RUN(5, 24, "frame + random gather L=24 + add chain", 1)
    // per hand-over, both barrier forms, each twice in alternation (the difference of a pair is the drain)
    for (int rep = 0; rep < 2; rep++) {
        RUNH(0, false, "vector hand-over L=8, __syncthreads()")
        RUNH(0, true, "vector hand-over L=8, bare s_barrier")
        RUNH(1, false, "block_sum hand-over b128, __syncthreads()")
        RUNH(1, true, "block_sum hand-over b128, bare s_barrier")
    }
    // row-broadcast reduction steps, each form twice in alternation
    for (int rep = 0; rep < 2; rep++) {
        RUNR(0, "row finish: 2 quad + half_mirror + mirror", 1)
        RUNR(1, "row finish: 2 quad + 3 v_fmac_f64_dpp", 1)
        RUNR(2, "second stage: pair read + 2 quad levels", 1)
        RUNR(3, "second stage S2a: pair read + bcast fmacs", 1)
        RUNR(4, "second stage S2b: 2 b128 reads + 1 quad level", 1)
        RUNR(5, "dependent v_add_f64", 16)
        RUNR(6, "dependent s_nop 1 + v_add_f64", 16)
        RUNR(7, "dependent s_nop 1 + v_fmac_f64", 16)
        RUNR(8, "dependent s_nop 1 + v_fmac_f64_dpp", 16)
    }
    return 0;
}
