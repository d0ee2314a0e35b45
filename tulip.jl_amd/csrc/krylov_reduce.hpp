// krylov_reduce.hpp -- the two ordered reductions of the matrix-free kernels (krylov_kernels.hip: conjugate gradients on K1; krylov_k2_kernels.hip: MINRES on K2;
// krylov_sqd_kernels.hip: TriCG on K2).
// A workgroup reduces its partial sum with a fixed shuffle tree and writes it to its slot; every workgroup of the consuming kernel adds the slots in slot
// order.  No atomics: two solves of the same data are bit-identical.
//
// Every kernel of a solve has a parameter NR: 1 is the single solve, 2 carries a pair of right-hand sides through the same launch (tlpk_solve2_device on a
// matrix-free handle; DESIGN.md section 1b''''''').  A pair has two contiguous scalar blocks sc[0], sc[1] and every vector, slot array and pointer of the
// solve twice (Rv / Rc below); what is shared is A and the diagonals.  Each right-hand side keeps the lane assignment, the shuffle trees and the slot order
// of the single kernel, so its arithmetic is that of a solve on its own, and it stops on its own: a kernel works on a right-hand side only while
// its outcome word says so (on[r] below), and returns at once only when that holds for neither.
#pragma once
#include <hip/hip_runtime.h>

namespace tlpk {

constexpr int CG_THREADS = 256;

// one pointer per right-hand side, passed to a kernel by value
template <int NR> struct Rv { double *p[NR]; };
template <int NR> struct Rc { const double *p[NR]; };
template <int NR> inline Rv<NR> rv(double *a, double *b) { Rv<NR> v; v.p[0] = a; if constexpr (NR > 1) v.p[1] = b; return v; }
template <int NR> inline Rc<NR> rc(const double *a, const double *b) { Rc<NR> v; v.p[0] = a; if constexpr (NR > 1) v.p[1] = b; return v; }

// sum over the workgroup (T threads), the same on every thread: shuffle tree inside a wave, then the waves in wave order
template <int T = CG_THREADS>
__device__ __forceinline__ double cg_block_sum(double v, double *sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) s += sh[w];
    __syncthreads();
    return s;
}
// the partial sums of the producing kernel, added in slot order; every thread forms the same sum.  The slots come into LDS with one coalesced load
// per thread first: read one by one from global memory, the 256 dependent loads of a large problem cost more than the kernel's own work
// (measured: 35 ns per slot, 15 of 43 us per iteration on eight C4 blocks).
__device__ __forceinline__ double cg_sum_slots(const double *__restrict__ slots, int ns, double *shs) {
    for (int k = threadIdx.x; k < ns; k += blockDim.x) shs[k] = slots[k];
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < ns; ++k) s += shs[k];
    return s;
}
// ... of NR right-hand sides behind ONE barrier: shs holds NR * LDS doubles, out[r] is the sum of slots.p[r][0 .. ns) for every r that is on (the slots of
// another one are not read).  NR = 1 is cg_sum_slots.
template <int NR, int LDS, class Slots>
__device__ __forceinline__ void cg_sum_slots(const Slots &slots, int ns, double *shs, const bool (&on)[NR], double (&out)[NR]) {
#pragma unroll
    for (int r = 0; r < NR; ++r)
        if (on[r]) for (int k = threadIdx.x; k < ns; k += blockDim.x) shs[r * LDS + k] = slots.p[r][k];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        double s = 0.0;
        if (on[r]) for (int k = 0; k < ns; ++k) s += shs[r * LDS + k];
        out[r] = s;
    }
}

// Which right-hand sides a kernel works on: on[r] = live(outcome word of r); false = not one of them.  NR = 1: every thread reads the word itself, as the
// single kernel always did.  A pair: thread r reads the word of r and the workgroup shares what it saw.  In the kernels whose first workgroup SETS the word
// (k_cg_step, k_cg_dir, k_mr_rot, k_tc_upd) the waves of a late workgroup could otherwise disagree about one right-hand side, and the barriers they then
// skip would tear the sums of the other one.
template <int NR, class Sc, class Live>
__device__ __forceinline__ bool krylov_live(const Sc *sc, bool (&on)[NR], Live live) {
    if constexpr (NR == 1) {
        on[0] = live(sc[0].outcome);
        return on[0];
    } else {
        __shared__ int shl[NR];
        if (threadIdx.x < NR) shl[threadIdx.x] = live(sc[threadIdx.x].outcome) ? 1 : 0;
        __syncthreads();
        bool any = false;
#pragma unroll
        for (int r = 0; r < NR; ++r) { on[r] = __builtin_amdgcn_readfirstlane(shl[r]) != 0; any = any || on[r]; }      // (the same in every lane: a scalar branch)
        return any;
    }
}
// ... in a kernel that no workgroup of its own launch can overtake (the gathers, k_mr_step, k_tc_step): the word is stable, every thread reads it
template <int NR, class Sc>
__device__ __forceinline__ bool krylov_running(const Sc *sc, bool (&on)[NR]) {
    bool any = false;
#pragma unroll
    for (int r = 0; r < NR; ++r) { on[r] = sc[r].outcome == 0; any = any || on[r]; }      // (0 = CG_RUNNING)
    return any;
}

// an empty row with Rd_i = 0 has M_i = 0: it keeps M^-1_i = 1 (no scaling), so that z = M^-1 r stays finite and the solve behaves as without Jacobi
__device__ __forceinline__ double cg_minv(double M) { return M == 0.0 ? 1.0 : 1.0 / M; }

}  // namespace tlpk
