// lpbox_eigen_redux.h -- the reference's summation order for a sum over the n elements of one problem held by one workgroup: Eigen
// 3.3.8's redux_impl<scalar_sum_op, ..., LinearVectorizedTraversal, NoUnrolling> with SSE2 packets of two doubles (Core/Redux.h),
// which the oracles restate as redux_sum_eigen (oracle/bqp_oracle.c, oracle/lpbox_oracle.c):
//   four accumulators p0a, p0b, p1a, p1b start at a[0..3] and add every fourth element over the prefix whose length is a multiple of
//   four; then p0a + p1a and p0b + p1b; then the left-over pair a[a2], a[a2 + 1] onto those two; then p0a + p0b; then the odd last
//   element.  n = 1, 2, 3 take the short branches.
// Use: every thread writes the term of its element j to row v of an LDS staging area (stage[v * sst + j], j < n only); er_reduce<NV>
// publishes them with one barrier, lane 4v + c of wave 0 walks accumulator c of value v strictly in order, lane 4v combines, and the
// totals return through LDS behind a second barrier.  Every walk is bounded by n (workgroup-uniform): nothing is padded -- a chain
// that has reached -0.0 would change under "+ 0.0" -- and nothing beyond the n staged terms is read.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int ER_MAXV = 4;        // values walked together: 16 lanes of wave 0
constexpr int ER_RES = 8;         // doubles of the result area (ER_MAXV used)

// Row stride of the staging area: >= n, and 4 modulo 32 doubles, so that the 16 walking lanes (row v, accumulator c: double
// v * sst + c + 4k) read 16 different double-wide banks of the 64 x 4-byte banks of the LDS.
__host__ __device__ __forceinline__ constexpr int er_stride(int n) { return ((n + 31) & ~31) + 4; }

// accumulator c (0..3) of a[0 .. size) in the four lanes of a group; every lane of the group returns the sum
__device__ __forceinline__ double er_walk(const double *a, int size, int c) {
    if (size >= 4) {
        const int a2 = size & ~3;
        double acc = a[c];
        int k = 4 + c;
        for (; k + 28 < a2; k += 32) {                       // eight LDS reads in flight, then the eight dependent additions in order
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; q++) v[q] = a[k + 4 * q];
#pragma unroll
            for (int q = 0; q < 8; q++) acc = acc + v[q];
        }
        for (; k < a2; k += 4) acc = acc + a[k];
        acc = acc + __shfl_xor(acc, 2, 4);                   // p0a + p1a (lanes 0, 2), p0b + p1b (lanes 1, 3)
        if (size & 2) acc = acc + a[a2 + (c & 1)];           // the left-over pair
        double res = acc + __shfl_xor(acc, 1, 4);            // p0a + p0b
        if (size & 1) res = res + a[size - 1];               // the odd last element
        return res;
    }
    if (size >= 2) {
        double res = a[0] + a[1];
        if (size == 3) res = res + a[2];
        return res;
    }
    return size == 1 ? a[0] : 0.0;
}

// NV <= ER_MAXV sums of `size` staged terms each; every thread receives the totals.  The barrier on entry publishes the terms, the one
// on exit the totals; it also frees the staging rows, and a thread reads `res` before it can reach the entry barrier of the next call.
template <int NV>
__device__ __forceinline__ void er_reduce(const double *stage, int sst, int size, double *res, double *out) {
    static_assert(NV >= 1 && NV <= ER_MAXV, "staging rows");
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < 4 * NV) {
        const int v = tid >> 2;
        const double r = er_walk(stage + (size_t)v * sst, size, tid & 3);
        if ((tid & 3) == 0) res[v] = r;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; k++) out[k] = res[k];
}

}  // namespace
