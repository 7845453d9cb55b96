// lpbox_lp_fix_kernels.hip -- the two small kernels of the early-fixing loop that keep a policy's inputs and scores on the device
// (lpbox_get_x_iters_rows_device / lpbox_iterate_l2f_scores): the row table of the packed iterate windows, and deter_fix_2
// (LP/trainer.py:101-135) on float32 scores.  Neither touches solver state: the fix itself is still applied by the window kernels,
// which read `newfix` when the host sets the apply word.
#include "lpbox_lp.h"

namespace {

constexpr int FIX_T = 256;

// Rows instance `inst` owns in the stacked table: its live rows of the last window if it is active, none if it is parked -- and never
// more than the range [first[inst], first[inst + 1]) the host sized the outputs by, whatever the device copies say.
__device__ __forceinline__ int table_rows(const int *rows, const int *isc, const int *first, int inst) {
    const int r = isc[(size_t)inst * NI_COUNT + NI_ACTIVE] ? rows[inst] : 0;
    const int cap = first[inst + 1] - first[inst];
    return r < 0 ? 0 : (r < cap ? r : cap);
}

// out[first[i] + q] = i * stride + q * ws: where row q of instance i starts in the buffer lp_pack_xiters_kernel fills.
__global__ void __launch_bounds__(FIX_T) lp_row_offsets_kernel(const int *rows, const int *isc, const int *first, int ws, long stride,
                                                               long long *out) {
    const int inst = blockIdx.y;
    const int nr = table_rows(rows, isc, first, inst);
    const long long base = (long long)inst * stride;
    long long *o = out + first[inst];
    for (int q = blockIdx.x * FIX_T + threadIdx.x; q < nr; q += gridDim.x * FIX_T) o[q] = base + (long long)q * ws;
}

// One workgroup per instance.  Row q of the instance is its q-th live variable; live_pos[inst * NS + q] is that variable's storage
// position (written by the staging of the last window).  code: 2 = fix to 1 (s > hi), 1 = fix to 0 (s < lo), 0 = leave; a NaN fails
// both comparisons.  Writes newfix only at live positions of its own instance, codes / counts only inside its own ranges.
__global__ void __launch_bounds__(FIX_T) lp_decide_fix_kernel(const float *scores, const int *rows, const int *isc, const int *first,
                                                              const int *live_pos, int NS, double hi, double lo, uint8_t *newfix,
                                                              uint8_t *codes, int *counts) {
    __shared__ int cnt[2];
    const int inst = blockIdx.x, tid = threadIdx.x;
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();
    const int nr = table_rows(rows, isc, first, inst);
    const int r0 = first[inst];
    const int *lp = live_pos + (size_t)inst * NS;
    uint8_t *nf = newfix + (size_t)inst * NS;
    int ones = 0, zeros = 0;
    for (int q = tid; q < nr; q += FIX_T) {
        const double s = (double)scores[r0 + q];
        const int code = s > hi ? 2 : (s < lo ? 1 : 0);
        ones += code == 2; zeros += code == 1;
        const int pos = lp[q];
        if ((unsigned)pos < (unsigned)NS) nf[pos] = (uint8_t)code;
        codes[r0 + q] = (uint8_t)code;
    }
    if (ones) atomicAdd(&cnt[0], ones);
    if (zeros) atomicAdd(&cnt[1], zeros);
    __syncthreads();
    if (tid < 2) counts[2 * inst + tid] = cnt[tid];
}

}  // namespace

hipError_t lp_launch_row_offsets(int B, int NS, const int *rows, const int *isc, const int *first, int ws, long stride, long long *out,
                                 hipStream_t s) {
    dim3 grid((NS + FIX_T - 1) / FIX_T, B);
    hipLaunchKernelGGL(lp_row_offsets_kernel, grid, dim3(FIX_T), 0, s, rows, isc, first, ws, stride, out);
    return hipGetLastError();
}

hipError_t lp_launch_decide_fix(int B, int NS, const float *scores, const int *rows, const int *isc, const int *first, const int *live_pos,
                                double hi, double lo, uint8_t *newfix, uint8_t *codes, int *counts, hipStream_t s) {
    hipLaunchKernelGGL(lp_decide_fix_kernel, dim3(B), dim3(FIX_T), 0, s, scores, rows, isc, first, live_pos, NS, hi, lo, newfix, codes, counts);
    return hipGetLastError();
}
