// lpbox_dev_common.h -- device helpers shared by the LP and SEG kernels: the fixed reduction tree.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// ------------------------------------------------------------------------------------------------
// wave / block reductions
// ------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, true);
    hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// The fixed reduction tree of a 64-lane wavefront, per value: halves first (lane l + lane l^32), then the two row pairs (l^16),
// then inside a row of 16 lanes pairs, quads, 8, 16.  Putting the two wide steps FIRST lets several values share them: a
// v_permlane32_swap / v_permlane16_swap of two DIFFERENT values is a reduce-scatter step (one half / row keeps value A, the other
// value B), so NV values cost one narrow butterfly instead of NV (wave_reduce_scatter below).  Floating-point addition is
// commutative, so "own + partner" and "partner + own" are the same bits and every lane of a group holds the identical partial.
struct HalfSwap {           // r0 = [a.lanes 0-31 , b.lanes 0-31], r1 = [a.lanes 32-63, b.lanes 32-63]
    static __device__ __forceinline__ void run(double a, double b, double &r0, double &r1) {
        auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(a), __double2loint(b), false, false);
        auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(a), __double2hiint(b), false, false);
        r0 = __hiloint2double(hi[0], lo[0]); r1 = __hiloint2double(hi[1], lo[1]);
    }
};
struct RowSwap {            // r0 = rows [a0, b0, a2, b2], r1 = rows [a1, b1, a3, b3] (rows of 16 lanes)
    static __device__ __forceinline__ void run(double a, double b, double &r0, double &r1) {
        auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(a), __double2loint(b), false, false);
        auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(a), __double2hiint(b), false, false);
        r0 = __hiloint2double(hi[0], lo[0]); r1 = __hiloint2double(hi[1], lo[1]);
    }
};
// one wide step for two values: the lower half / even rows end up with a's pair sums, the upper half / odd rows with b's
template <typename SWAP>
__device__ __forceinline__ double pair_step(double a, double b) { double r0, r1; SWAP::run(a, b, r0, r1); return r0 + r1; }

// A wide step whose result is read in the lower half / the even rows only: the partner operand of the swap is a register with no defined
// content (an empty asm output, so the compiler neither copies v to feed the swap (v, v) nor reasons about the value).  The lower half /
// the even rows receive exactly what pair_step<SWAP>(a, a) gives them; the upper half / the odd rows hold garbage.
__device__ __forceinline__ double undefined_f64() {
    int lo, hi;                      // (volatile: every call defines registers of its own -- merged into one, the swaps would copy it)
    asm volatile("" : "=v"(lo));
    asm volatile("" : "=v"(hi));
    return __hiloint2double(hi, lo);
}
template <typename SWAP>
__device__ __forceinline__ double pair_step_low(double a) { double r0, r1; SWAP::run(a, undefined_f64(), r0, r1); return r0 + r1; }

__device__ __forceinline__ double row_allreduce(double v) {      // inside each row of 16 lanes: pairs, quads, 8, 16
    v = v + dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
    v = v + dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
    v = v + dpp_mov<0x141>(v);   // row_half_mirror: after the quad steps the mirrored partner holds the xor-4 partner's value
    v = v + dpp_mov<0x140>(v);   // row_mirror: likewise xor-8
    return v;
}

// row_newbcast:N, the one DPP control gfx950 applies to a 64-bit operand: every lane of a row of 16 receives lane N of its row.
// Preconditions of what is built on it (row_reduce_lane0): all 64 lanes of the wave are active -- a DPP read of an inactive lane is
// not the value the sums need -- and the call stands in wave-uniform control flow.
// The f64 arithmetic that takes such an operand is v_fmac_f64 (v_add_f64 has no DPP form on gfx950: the assembler rejects it), so an
// addition of a broadcast value is written  acc += bcast(x) * 1.0.  The product with 1.0 is exact, so the one rounding of the fused
// operation is the rounding of the addition acc + bcast(x): the same bits for every non-NaN operand, +-0 and infinities included.
// The compiler does not select this form, hence the asm statements; each carries its own wait states (two between a VALU write of a
// register and a DPP read of it).

// row_allreduce for a caller that reads lane 0 of each row only (the owner lanes of wave_partials_store): the two quad steps, then with
// the four quads of a row holding Q0..Q3   a = Q0 + Q1 (right in lanes 0-3),  b = Q2 + Q3 (right in lanes 8-11),  lane 0 = a + b:
// three v_fmac_f64 with a row_newbcast operand, two of them independent, where row_half_mirror and row_mirror cost two moves, a wait and
// an addition each.  Lane 0 receives (Q0 + Q1) + (Q2 + Q3), row_allreduce's association.  Every other lane of the row holds garbage.
// Wait states: in front, where the compiler's quad step has just written v, and between the write of b and its DPP read (the
// independent a += and s_nop 0).
__device__ __forceinline__ double row_reduce_lane0(double v) {
    v = v + dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
    v = v + dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
    double a = v, b = v;
    asm("s_nop 1\n\t"
        "v_fmac_f64_dpp %1, %0, %2 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"      // b = Q + Q3: Q2 + Q3 in lanes 8-11
        "v_fmac_f64_dpp %0, %0, %2 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"       // a = Q + Q1: Q0 + Q1 in lanes 0-3
        "s_nop 0\n\t"
        "v_fmac_f64_dpp %0, %1, %2 row_newbcast:8 row_mask:0xf bank_mask:0xf"           // lane 0: (Q0 + Q1) + (Q2 + Q3)
        : "+v"(a), "+v"(b) : "v"(1.0));
    return a;
}
template <bool LANE0>
__device__ __forceinline__ double row_finish(double v) { if constexpr (LANE0) return row_reduce_lane0(v); else return row_allreduce(v); }

// 64-lane all-reduce of one value (every lane receives the sum).
__device__ __forceinline__ double wave_allreduce_sum(double v) {
#ifdef LPBOX_REDUCE_SHFL
    v = v + __shfl_xor(v, 32, 64); v = v + __shfl_xor(v, 16, 64);
    for (int off = 1; off < 16; off <<= 1) v = v + __shfl_xor(v, off, 64);
    return v;
#else
    v = pair_step<HalfSwap>(v, v);
    v = pair_step<RowSwap>(v, v);
    return row_allreduce(v);
#endif
}

// NV <= 4 values through ONE narrow butterfly: on return the total of value k sits in every lane of row ROW_OF[k]
// (rows of 16 lanes: value 0 -> row 0, 1 -> row 2, 2 -> row 1, 3 -> row 3); the result is returned in `out`, to be read
// only in those rows.  Same per-value tree as wave_allreduce_sum.
template <int NV, bool LANE0 = false>                                  // LANE0: valid in the first lane of each of those rows only (row_reduce_lane0)
__device__ __forceinline__ double wave_reduce_scatter(const double *v) {
    static_assert(NV >= 2 && NV <= 4, "2..4 values");
    const double x = pair_step<HalfSwap>(v[0], v[1]);                                   // lower half: value 0, upper half: value 1
    double s;
    if constexpr (NV == 2) s = pair_step<RowSwap>(x, x);
    else {
        const double y = NV == 4 ? pair_step<HalfSwap>(v[2], v[3]) : pair_step<HalfSwap>(v[2], v[2]);
        s = pair_step<RowSwap>(x, y);                                                   // rows: [v0, v2, v1, v3 (or v2 again)]
    }
    return row_finish<LANE0>(s);
}
// lane that owns value k after wave_reduce_scatter<NV>
__device__ __forceinline__ constexpr int scatter_lane(int nv, int k) { return nv == 2 ? 32 * k : (k == 0 ? 0 : k == 1 ? 32 : k == 2 ? 16 : 48); }

__device__ __forceinline__ int wave_max_int(int v) {
    for (int off = 1; off < 64; off <<= 1) { int o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return __builtin_amdgcn_readfirstlane(v);
}

// ------------------------------------------------------------------------------------------------
// workgroup barriers
// ------------------------------------------------------------------------------------------------
// An LDS hand-over between the waves of a workgroup: a bare s_barrier between two compiler-only memory barriers.  __syncthreads() is a
// workgroup fence over every address space, so the compiler puts s_waitcnt lgkmcnt(0) in front of its s_barrier: each wave waits for
// the LDS to acknowledge its ds_write before it signals arrival.  The two asm statements emit no instruction; they keep the compiler
// from moving an LDS access across the s_barrier, so ds_write / s_barrier / ds_read stay in program order and the wave arrives at the
// barrier with its write still in flight.
// Contract (the caller's to keep; DESIGN.md section 5, "LDS hand-overs"):
//   * both sides of the call touch LDS only -- there is no global or scratch access whose order against these LDS accesses matters
//     (the LDS counter is what orders LDS against the other memories, and it is not drained here);
//   * every wave of the workgroup runs on one CU, whose LDS executes the LDS instructions of all its waves in one order: a ds_read
//     issued behind the barrier follows every ds_write issued in front of it, and a ds_write behind it every ds_read in front of it
//     (tests/test_lds_handover_gpu.py stresses exactly this);
//   * the call stands in workgroup-uniform control flow, one for one where a __syncthreads() would stand.
__device__ __forceinline__ void lds_handover() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
constexpr int RED_BAR_SYNC = 0;        // __syncthreads(): the default of every caller
constexpr int RED_BAR_HANDOVER = 1;    // lds_handover(): the caller keeps its contract for everything around the block_sum
template <int BAR>
__device__ __forceinline__ void wg_barrier() {
    static_assert(BAR == RED_BAR_SYNC || BAR == RED_BAR_HANDOVER, "barrier form");
    if constexpr (BAR == RED_BAR_HANDOVER) lds_handover();
    else __syncthreads();
}

constexpr int RED_MAXV = 6;    // values reduced together
constexpr int RED_MAXW = 16;   // waves per workgroup

// Second stage of block_sum (how the W wave partials of a value get from LDS into every lane), chosen per caller.
// Both forms add in the same tree over the wave index -- pairs (0,1) (2,3) ..., quads, eight -- so they give the same bits.
constexpr int RED_STAGE_BCAST = 0;   // every lane reads all W partials (broadcast reads) and adds them in registers: the default
constexpr int RED_STAGE_PAIRS = 1;   // W = 8: lane reads the pair (p[2j], p[2j+1]), j = lane & 3, with one ds_read_b128 per value
                                     // and adds it (the tree's "pairs" level); two quad_perm steps finish the tree
constexpr int RED_STAGE_PAIRS_LOW = 2;   // RED_STAGE_PAIRS whose first stage runs the wide steps of 1, 2 and 3 values without register copies
constexpr int RED_STAGE_PAIRS_BC = 3;    // RED_STAGE_PAIRS_LOW whose first stage finishes each row for its first lane only (row_reduce_lane0)
// the second stage that reads four partials per lane (h = lane & 1 reads 4h .. 4h + 3 with two ds_read_b128 per value and adds
// (p0 + p1) + (p2 + p3), the tree's pairs and quads of waves; ONE quad_perm level finishes), on either first stage
constexpr int RED_STAGE_FOUR_BC = 4;     // first stage of RED_STAGE_PAIRS_BC: what the 512 x 1 window kernel runs
constexpr int RED_STAGE_FOUR_LOW = 5;    // first stage of RED_STAGE_PAIRS_LOW
constexpr int RED_STAGE_LAST = RED_STAGE_FOUR_LOW;
__host__ __device__ constexpr bool red_first_low(int stage) { return stage >= RED_STAGE_PAIRS_LOW; }
__host__ __device__ constexpr bool red_first_lane0(int stage) { return stage == RED_STAGE_PAIRS_BC || stage == RED_STAGE_FOUR_BC; }
__host__ __device__ constexpr bool red_second_four(int stage) { return stage == RED_STAGE_FOUR_BC || stage == RED_STAGE_FOUR_LOW; }

// First stage of RED_STAGE_PAIRS: the wave butterflies of block_sum, then ONE predicated store per butterfly -- the first lane
// of every row of 16 lanes writes what its row holds (rows [v0, v2, v1, v3]; with fewer than four values a row that repeats a value
// writes it to a slot nobody reads), instead of one exec-mask region per value.
// LOW (RED_STAGE_PAIRS_LOW): only the first lane of row 0 (one value), of rows 0 and 2 (two values), of rows 0, 2, 1 (three) is read back,
// so a wide step that would swap a value against itself -- both of one value, the row step of two, the half step of the third of
// three -- swaps it against an undefined register instead (pair_step_low): no v_mov copies in front of the swap.  The stored lanes
// receive the same sums in the same association; the other owner lanes write garbage to the slots nobody reads (values >= NV of the
// same parity half, as before).  Six values keep the copies: the rows of their second butterfly share two slots.
// LANE0 (RED_STAGE_PAIRS_BC): the owner lanes are the only ones stored, for every number of values, so each butterfly finishes its rows
// with row_reduce_lane0 -- the lanes it leaves with garbage are exactly the lanes that do not store.  All 64 lanes must be active.
template <int NV, bool LOW = false, bool LANE0 = false>
__device__ __forceinline__ void wave_partials_store(const double *v, double *buf, int lane, int w) {
    static_assert(LOW || !LANE0, "the lane-0 row finish goes with the LOW wide steps");
    const int row = lane >> 4, k = ((row & 1) << 1) | (row >> 1);    // value index of this lane's row after wave_reduce_scatter<3 or 4>;
    const bool owner = (lane & 15) == 0;                              // after <2> rows 0, 1 hold value 0 and rows 2, 3 value 1: slots 0, 2, 1, 3
    double *at = buf + k * RED_MAXW + w;                         // loop-invariant up to the parity offset
    if constexpr (NV == 1) {
        double t0;
        if constexpr (LOW) t0 = row_finish<LANE0>(pair_step_low<RowSwap>(pair_step_low<HalfSwap>(v[0])));   // row 0 holds it
        else t0 = wave_allreduce_sum(v[0]);                           // every lane holds it: the slots of k = 1..3 get copies
        if (owner) *at = t0;
    } else if constexpr (LOW && NV == 2) {
        const double x = pair_step<HalfSwap>(v[0], v[1]);
        const double sc = row_finish<LANE0>(pair_step_low<RowSwap>(x));   // rows 0 and 2 hold values 0 and 1: slots 0 and 1
        if (owner) *at = sc;
    } else if constexpr (LOW && NV == 3) {
        const double x = pair_step<HalfSwap>(v[0], v[1]);
        const double y = pair_step_low<HalfSwap>(v[2]);               // rows 0, 1 hold the halves of value 2
        const double sc = row_finish<LANE0>(pair_step<RowSwap>(x, y));    // rows [v0, v2, v1, garbage]
        if (owner) *at = sc;
    } else {
        constexpr int NS4 = NV > 4 ? 4 : NV;
        const double sc = wave_reduce_scatter<NS4, LANE0>(v);
        if constexpr (NV == 6) {                                      // values 4 and 5 share a second butterfly: halves [v4, v5]
            const double sc2 = wave_reduce_scatter<2, LANE0>(v + 4);
            if (owner) { *at = sc; buf[(4 + (k & 1)) * RED_MAXW + w] = sc2; }
        } else {
            static_assert(NV <= 4, "1, 2, 3, 4 or 6 values");
            if (owner) *at = sc;
        }
    }
}

// Sum NV per-thread partials over the workgroup; every thread receives the totals.  Wave partials go through LDS and
// are combined by a second butterfly (lane i reads partial i mod W; balanced tree over the wave index), i.e. ONE LDS
// round trip instead of W dependent reads.  `red` is a ping-pong scratch (2 * RED_MAXV * RED_MAXW doubles, 16-byte aligned): a thread
// can run at most one block_sum ahead of the slowest one.  BAR: the form of the barrier between the store and the reads (wg_barrier).
template <int T, int NV, int STAGE = RED_STAGE_BCAST, int BAR = RED_BAR_SYNC>
__device__ __forceinline__ void block_sum(double (&v)[NV], double *red, int &parity) {
    constexpr int W = T / 64;
    static_assert(W == 1 || W == 2 || W == 4 || W == 8 || W == 16, "waves per workgroup");
    if constexpr (W == 1) {              // one wavefront per instance: no LDS round trip, no barrier
#pragma unroll
        for (int k = 0; k < NV; k++) v[k] = wave_allreduce_sum(v[k]);
        return;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double *buf = red + parity * (RED_MAXV * RED_MAXW);
    if constexpr (STAGE != RED_STAGE_BCAST) {
        static_assert(W == 8 && STAGE >= RED_STAGE_PAIRS && STAGE <= RED_STAGE_LAST, "built for eight waves");
        wave_partials_store<NV, red_first_low(STAGE), red_first_lane0(STAGE)>(v, buf, lane, w);
        wg_barrier<BAR>();
        if constexpr (red_second_four(STAGE)) {
            // the tree's pairs and quads of waves in registers, its eight on one quad_perm level
            double2 t0[NV], t1[NV];
#pragma unroll
            for (int k = 0; k < NV; k++) {
                const double2 *q = (const double2 *)(buf + k * RED_MAXW + 4 * (lane & 1));
                t0[k] = q[0]; t1[k] = q[1];
            }
#pragma unroll
            for (int k = 0; k < NV; k++) {
                const double u = (t0[k].x + t0[k].y) + (t1[k].x + t1[k].y);      // waves ((0,1) (2,3)) resp. ((4,5) (6,7))
                v[k] = u + dpp_mov<0xB1>(u);                                     // eight
            }
            parity ^= 1;
            return;
        }
        double2 t[NV];
#pragma unroll
        for (int k = 0; k < NV; k++) t[k] = *(const double2 *)(buf + k * RED_MAXW + 2 * (lane & 3));
#pragma unroll
        for (int k = 0; k < NV; k++) {
            double u = t[k].x + t[k].y;                  // waves (0,1) (2,3) (4,5) (6,7)
            u = u + dpp_mov<0xB1>(u);                    // quads of waves
            u = u + dpp_mov<0x4E>(u);                    // eight
            v[k] = u;
        }
        parity ^= 1;
        return;
    }
    if constexpr (NV == 1) {
        const double t0 = wave_allreduce_sum(v[0]);
        if (lane == 0) buf[w] = t0;
    } else {
        // values 0..3 share one butterfly (reduce-scatter); a fifth goes alone, a fifth and a sixth share a second one
        constexpr int NS4 = NV > 4 ? 4 : NV;
        const double sc = wave_reduce_scatter<NS4>(v);
#pragma unroll
        for (int k = 0; k < NS4; k++) if (lane == scatter_lane(NS4, k)) buf[k * RED_MAXW + w] = sc;
        if constexpr (NV == 5) {
            const double t4 = wave_allreduce_sum(v[4]);
            if (lane == 0) buf[4 * RED_MAXW + w] = t4;
        } else if constexpr (NV == 6) {          // values 4 and 5 share a second butterfly
            const double sc2 = wave_reduce_scatter<2>(v + 4);
#pragma unroll
            for (int k = 0; k < 2; k++) if (lane == scatter_lane(2, k)) buf[(4 + k) * RED_MAXW + w] = sc2;
        } else static_assert(NV <= 4, "at most six values");
    }
    wg_barrier<BAR>();
    if constexpr (W >= 16) {
        // 16 waves (128-register budget): lane i takes the partial of wave i mod 16 and the row of 16 lanes runs the balanced tree
        // over the wave index on DPP -- the same association as the register version below, NV instead of NV * W live values
        double t[NV];
#pragma unroll
        for (int k = 0; k < NV; k++) t[k] = buf[k * RED_MAXW + (lane & (W - 1))];
#pragma unroll
        for (int k = 0; k < NV; k++) v[k] = row_allreduce(t[k]);
        parity ^= 1;
        return;
    }
    // every lane reads all W wave partials (same address in all lanes: an LDS broadcast) and adds them in registers in the
    // balanced tree over the wave index -- pairs (0,1) (2,3) ..., quads, ... -- i.e. the association of the xor butterfly the
    // first version ran on DPP (floating-point addition is commutative, so the bits are identical), without its dependent
    // cross-lane steps.
    double t[NV][W];
#pragma unroll
    for (int k = 0; k < NV; k++)
#pragma unroll
        for (int w2 = 0; w2 < W; w2++) t[k][w2] = buf[k * RED_MAXW + w2];
#pragma unroll
    for (int k = 0; k < NV; k++) {
#pragma unroll
        for (int span = 1; span < W; span <<= 1)
#pragma unroll
            for (int w2 = 0; w2 < W; w2 += 2 * span) t[k][w2] = t[k][w2] + t[k][w2 + span];
        v[k] = t[k][0];
    }
    parity ^= 1;
}

// Second level of the fixed reduction order, shared by the multi-kernel paths (large LP, generic BQP): out[v] = block tree over
// (thread t: partials t, t + T, ... of value v in ascending order), partials of value v at part[v * G ..].  Runs as ONE workgroup on
// the critical path of every reduction, so for 2 T < G <= T * FIN_U all loads of a pair of values are issued before the first (ordered)
// addition -- one memory latency instead of one per partial (5.1 -> about 3 us per launch at G = 1954).
constexpr int FIN_U = 16;
template <int T>
__device__ __forceinline__ void fin_reduce(const double *part, int G, int nv, double *out, double *red, int &parity, int stride = 0) {
    if (stride <= 0) stride = G;                 // partials of value v at part[v * stride ..]
    if (G > 2 * T && G <= T * FIN_U) {          // (with one or two partials per thread the plain loop below is the shorter program: A/B on the generic path)
        for (int v0 = 0; v0 < nv; v0 += 2) {
            const bool two = v0 + 1 < nv;
            const double *pa = part + (size_t)v0 * stride, *pb = part + (size_t)(two ? v0 + 1 : v0) * stride;
            double ta[FIN_U], tb[FIN_U];
#pragma unroll
            for (int u = 0; u < FIN_U; u++) {
                const int e = threadIdx.x + u * T;
                ta[u] = e < G ? pa[e] : 0.0;
                tb[u] = (two && e < G) ? pb[e] : 0.0;
            }
            double a[1] = {0.0}, b[1] = {0.0};
#pragma unroll
            for (int u = 0; u < FIN_U; u++) {
                const bool in = (int)threadIdx.x + u * T < G;
                a[0] = in ? a[0] + ta[u] : a[0];
                b[0] = in ? b[0] + tb[u] : b[0];
            }
            block_sum<T, 1>(a, red, parity);
            if (threadIdx.x == 0) out[v0] = a[0];
            if (two) {
                block_sum<T, 1>(b, red, parity);
                if (threadIdx.x == 0) out[v0 + 1] = b[0];
            }
        }
        return;
    }
    for (int v = 0; v < nv; v++) {
        const double *p = part + (size_t)v * stride;
        double a[1] = {0.0};
        for (int e = threadIdx.x; e < G; e += T) a[0] = a[0] + p[e];
        block_sum<T, 1>(a, red, parity);
        if (threadIdx.x == 0) out[v] = a[0];
    }
}

}  // namespace
