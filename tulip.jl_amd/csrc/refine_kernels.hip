// refine_kernels.hip -- refinement on demand (tlpk_polish_device / tlpk_polish2_device; DESIGN.md section 1c').
//
// Guarded refinement on the residuals of the augmented system
//   r1 = xi_p - A dx - Rd dy   (rows, CSR)        r2 = xi_d + (theta + Rp) dx - A' dy   (columns, CSC)
// for ONE or TWO systems against the same factor.  The rule is that of kernels.hip: k_refine_decide, kept per system: a step is
// kept only if it shrinks |r1|inf and leaves |r2|inf within 16 x of the value at entry; the verdict is reached on the device.
//
// k_kkt_resid<NR>: one launch over the rows and then the columns of A (the block index selects the region), a thread per row /
// column, 256-thread blocks.  Every stored entry of A is loaded once and feeds NR accumulators, and the two max-norms of every
// system are taken in the same kernel (bit patterns of fabs: they order like the doubles, a NaN above +inf; wave shuffle, LDS, one
// atomicMax per block and norm -- maxima: the order of the blocks does not matter).  The expression trees are those of
// k_resid_rows / k_resid_cols as the compiler builds them there (rank 0, no linking convention), written out so that no
// contraction rule can move them: the sum by fma in storage order, the row's base as a rounded product and a difference, the
// column's base as one fma.  NR = 1 on a K1 handle therefore reproduces those kernels bit for bit, and a system of a pair is
// computed as it is alone.
//
// State: PW words per system (PolishWord).  The host zeroes them in front of a call and copies them out behind it.
#include <hip/hip_runtime.h>

#include "tlpk_device.hpp"

namespace tlpk {

namespace {

constexpr int PR_THREADS = 256;

// block maximum of NV bit patterns: lanes of a wave by shuffle, the four waves through LDS; the result is valid in thread 0
template <int NV>
__device__ __forceinline__ void pr_block_max(unsigned long long (&v)[NV], unsigned long long (*red)[PR_THREADS / 64]) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const unsigned long long w = __shfl_xor(v[k], o); v[k] = w > v[k] ? w : v[k]; }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k)
            for (int w = 1; w < PR_THREADS / 64; ++w) v[k] = red[k][w] > v[k] ? red[k][w] : v[k];
    }
}

// xi_p - Rd dy as k_resid_rows forms it: the product is rounded, then subtracted (its operands pass through selects there, nothing is fused)
__device__ __forceinline__ double pr_row_base(double xp, double rd, double y) {
#pragma clang fp contract(off)
    const double p = rd * y;
    return xp - p;
}

template <int NR>
__global__ __launch_bounds__(PR_THREADS) void k_kkt_resid(PolishMat A, const double *__restrict__ theta, const double *__restrict__ regP,
                                                          const double *__restrict__ regD, PolishVecs v, unsigned long long *__restrict__ ref, int entry) {
    __shared__ unsigned long long red[NR][PR_THREADS / 64];
    const i64 row_blocks = (A.m + PR_THREADS - 1) / PR_THREADS;
    const bool rows = (i64)blockIdx.x < row_blocks;
    unsigned long long nrm[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) nrm[r] = 0;
    if (rows) {
        const i64 i = (i64)blockIdx.x * PR_THREADS + threadIdx.x;
        if (i < A.m) {
            double s[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) s[r] = 0.0;
            for (i64 q = A.Tp[i]; q < A.Tp[i + 1]; ++q) {
                const double a = A.Tx[q]; const i32 j = A.Tj[q];
#pragma unroll
                for (int r = 0; r < NR; ++r) s[r] = fma(a, v.dx[r][j], s[r]);
            }
            const double rd = regD[i];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const double res = pr_row_base(v.xi_p[r][i], rd, v.dy[r][i]) - s[r];
                v.r1[r][i] = res;
                nrm[r] = (unsigned long long)__double_as_longlong(fabs(res));
            }
        }
    } else {
        const i64 j = ((i64)blockIdx.x - row_blocks) * PR_THREADS + threadIdx.x;
        if (j < A.n) {
            double s[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) s[r] = 0.0;
            for (i64 p = A.Ap[j]; p < A.Ap[j + 1]; ++p) {
                const double a = A.Ax[p]; const i32 i = A.Ai[p];
#pragma unroll
                for (int r = 0; r < NR; ++r) s[r] = fma(a, v.dy[r][i], s[r]);
            }
            const double e = theta[j] + regP[j];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const double res = fma(e, v.dx[r][j], v.xi_d[r][j]) - s[r];
                v.r2[r][j] = res;
                nrm[r] = (unsigned long long)__double_as_longlong(fabs(res));
            }
        }
    }
    pr_block_max<NR>(nrm, red);
    if (threadIdx.x == 0) {
        // entry: the norms of the iterate the call was given (PW_R1 current, PW_R2_REF reference; PW_R1_IN / PW_R2_KEPT for the report);
        // otherwise those of the candidate
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            unsigned long long *w = ref + (size_t)r * PW;
            if (entry) { atomicMax(w + (rows ? PW_R1 : PW_R2_REF), nrm[r]); atomicMax(w + (rows ? PW_R1_IN : PW_R2_KEPT), nrm[r]); }
            else atomicMax(w + (rows ? PW_C1 : PW_C2), nrm[r]);
        }
    }
}

// k_refine_decide's rule, one thread per system
__global__ void k_polish_decide(unsigned long long *ref, int nr) {
    if ((int)threadIdx.x >= nr) return;
    unsigned long long *w = ref + (size_t)threadIdx.x * PW;
    int *st = reinterpret_cast<int *>(w + PW_STATE), *ac = reinterpret_cast<int *>(w + PW_ACCEPT);
    const double r2_ref = __longlong_as_double((long long)w[PW_R2_REF]), r2_new = __longlong_as_double((long long)w[PW_C2]);
    const bool accept = !st[1] && w[PW_C1] < w[PW_R1] && r2_new <= 16.0 * r2_ref;
    ac[0] = accept ? 1 : 0;
    if (accept) { w[PW_R1] = w[PW_C1]; w[PW_R2_KEPT] = w[PW_C2]; ac[1] += 1; }
    else if (!st[1]) { st[0] += 1; st[1] = 1; }
    w[PW_C1] = 0; w[PW_C2] = 0;
}
// candidate <- x + correction (kept beside x until the verdict); grid y = system
__global__ void k_polish_candidate(i64 n, i64 m, PolishPair p) {
    const int r = blockIdx.y;
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p.cx[r][i] = p.x[r][i] + p.cx[r][i];
    if (i < m) p.cy[r][i] = p.y[r][i] + p.cy[r][i];
}
__global__ void k_polish_commit(i64 n, i64 m, PolishPair p, const unsigned long long *__restrict__ ref) {
    const int r = blockIdx.y;
    if (!reinterpret_cast<const int *>(ref + (size_t)r * PW + PW_ACCEPT)[0]) return;
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p.x[r][i] = p.cx[r][i];
    if (i < m) p.y[r][i] = p.cy[r][i];
}

inline unsigned nblk(i64 n, int b) { return (unsigned)((n + b - 1) / b); }

}  // namespace

void launch_kkt_resid(hipStream_t st, const PolishMat &A, const double *theta, const double *regP, const double *regD, const PolishVecs &v,
                      unsigned long long *ref, int nr, int entry) {
    const unsigned blocks = nblk(A.m, PR_THREADS) + nblk(A.n, PR_THREADS);
    if (blocks == 0) return;
    if (nr == 2) hipLaunchKernelGGL(k_kkt_resid<2>, dim3(blocks), dim3(PR_THREADS), 0, st, A, theta, regP, regD, v, ref, entry);
    else hipLaunchKernelGGL(k_kkt_resid<1>, dim3(blocks), dim3(PR_THREADS), 0, st, A, theta, regP, regD, v, ref, entry);
}
void launch_polish_decide(hipStream_t st, unsigned long long *ref, int nr) { hipLaunchKernelGGL(k_polish_decide, dim3(1), dim3(64), 0, st, ref, nr); }
void launch_polish_candidate(hipStream_t st, i64 n, i64 m, const PolishPair &p, int nr) {
    const i64 len = std::max(n, m);
    if (len > 0) hipLaunchKernelGGL(k_polish_candidate, dim3(nblk(len, 256), (unsigned)nr), dim3(256), 0, st, n, m, p);
}
void launch_polish_commit(hipStream_t st, i64 n, i64 m, const PolishPair &p, const unsigned long long *ref, int nr) {
    const i64 len = std::max(n, m);
    if (len > 0) hipLaunchKernelGGL(k_polish_commit, dim3(nblk(len, 256), (unsigned)nr), dim3(256), 0, st, n, m, p, ref);
}

}  // namespace tlpk
