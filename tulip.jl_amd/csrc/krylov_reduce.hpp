// krylov_reduce.hpp -- the two ordered reductions of the matrix-free kernels (krylov_kernels.hip: conjugate gradients on K1; krylov_k2_kernels.hip: MINRES on K2;
// krylov_sqd_kernels.hip: TriCG on K2).
// A workgroup reduces its partial sum with a fixed shuffle tree and writes it to its slot; every workgroup of the consuming kernel adds the slots in slot
// order.  No atomics: two solves of the same data are bit-identical.
#pragma once
#include <hip/hip_runtime.h>

namespace tlpk {

constexpr int CG_THREADS = 256;

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

// an empty row with Rd_i = 0 has M_i = 0: it keeps M^-1_i = 1 (no scaling), so that z = M^-1 r stays finite and the solve behaves as without Jacobi
__device__ __forceinline__ double cg_minv(double M) { return M == 0.0 ? 1.0 : 1.0 / M; }

}  // namespace tlpk
