// refresh_kernels.hip -- new values on an analysed pattern (tlpk_set_values; DESIGN.md section 1b''').
//
// What depends on the values of A in a handle: the products pair_w of the assembly lists, the value arrays of the CSC / CSR copies
// (Ax, Tx, Px) and the dense copy dA.  The maps of symbolic.cpp: build_value_maps name, for every one of those entries, the position(s)
// in the caller's nzval it comes from; the kernels below are the streaming passes that apply them.  Every output element is written by
// exactly one thread, there are no atomics, and a product is formed as value(a) * value(b) with the operands in the order in which
// symbolic.cpp forms them at create: the refreshed arrays equal those of a fresh handle bit for bit.
//
// Shape: one dependent gather behind a streamed index load.  Four elements per thread: the index loads are one 16-byte load per
// list, the (up to eight) gathers are issued before the first use, the results leave as 16-byte stores.  64-bit element indices.
#include <hip/hip_runtime.h>

#include "tlpk_device.hpp"

namespace tlpk {

namespace {

constexpr int RF_THREADS = 256;
constexpr int RF_PER = 4;          // elements per thread

__device__ __forceinline__ double rf_value(const double *__restrict__ nz, i32 p, double g) { return p >= 0 ? g : (p == VM_ONE ? 1.0 : -1.0); }

// w[t] = value(a[t]) * value(b[t])
__global__ __launch_bounds__(RF_THREADS) void k_refresh_pairs(i64 np, const i32 *__restrict__ a, const i32 *__restrict__ b, const double *__restrict__ nz,
                                                              double *__restrict__ w) {
    const i64 t0 = ((i64)blockIdx.x * RF_THREADS + threadIdx.x) * RF_PER;
    if (t0 >= np) return;
    if (t0 + RF_PER <= np) {
        const int4 ia = *reinterpret_cast<const int4 *>(a + t0), ib = *reinterpret_cast<const int4 *>(b + t0);
        const i32 pa[4] = {ia.x, ia.y, ia.z, ia.w}, pb[4] = {ib.x, ib.y, ib.z, ib.w};
        double ga[4], gb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { ga[u] = nz[max(pa[u], 0)]; gb[u] = nz[max(pb[u], 0)]; }      // (a sentinel reads entry 0 and drops it: no divergent load)
        double r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = rf_value(nz, pa[u], ga[u]) * rf_value(nz, pb[u], gb[u]);
        *reinterpret_cast<double2 *>(w + t0) = make_double2(r[0], r[1]);
        *reinterpret_cast<double2 *>(w + t0 + 2) = make_double2(r[2], r[3]);
    } else {
        for (i64 t = t0; t < np; ++t) {
            const i32 pa = a[t], pb = b[t];
            w[t] = rf_value(nz, pa, nz[max(pa, 0)]) * rf_value(nz, pb, nz[max(pb, 0)]);
        }
    }
}

// out[q] = value(src[q]): the CSR copies Tx / Px, and Ax of the augmented system's incidence matrix
__global__ __launch_bounds__(RF_THREADS) void k_refresh_gather(i64 n, const i32 *__restrict__ src, const double *__restrict__ nz, double *__restrict__ out) {
    const i64 q0 = ((i64)blockIdx.x * RF_THREADS + threadIdx.x) * RF_PER;
    if (q0 >= n) return;
    if (q0 + RF_PER <= n) {
        const int4 is = *reinterpret_cast<const int4 *>(src + q0);
        const i32 p[4] = {is.x, is.y, is.z, is.w};
        double g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) g[u] = nz[max(p[u], 0)];
        *reinterpret_cast<double2 *>(out + q0) = make_double2(rf_value(nz, p[0], g[0]), rf_value(nz, p[1], g[1]));
        *reinterpret_cast<double2 *>(out + q0 + 2) = make_double2(rf_value(nz, p[2], g[2]), rf_value(nz, p[3], g[3]));
    } else {
        for (i64 q = q0; q < n; ++q) { const i32 p = src[q]; out[q] = rf_value(nz, p, nz[max(p, 0)]); }
    }
}

// dense-matrix handles: column-major m x n with leading dimension lda -> the handle's copy with leading dimension dlda >= m, padding rows zero
__global__ __launch_bounds__(RF_THREADS) void k_refresh_dense(i64 m, i64 n, const double *__restrict__ A, i64 lda, double *__restrict__ dA, i64 dlda) {
    const i64 r = (i64)blockIdx.x * RF_THREADS + threadIdx.x;
    const i64 c = blockIdx.y;
    if (r >= dlda) return;
    for (i64 j = c; j < n; j += gridDim.y) dA[j * dlda + r] = (r < m) ? A[j * lda + r] : 0.0;
}

// ---- selected slots of a stack of LPs (tlpk_ipm_batch_refill) ----
// The stacked matrix is block diagonal, so both factors of a product and the source of a copied entry belong to ONE LP: lp_of[p] is the LP
// that owns entry p of the caller's nzval, flag[k * stride] != 0 selects LP k.  A thread rewrites its element only where that LP is
// selected -- formed exactly as the passes above form it -- and leaves it alone otherwise; the constants (a unit entry, the -1 of a
// diagonal) depend on no value and are never rewritten.  One writer per element, no atomics; only the selected LPs' ranges of nz are read.
__device__ __forceinline__ bool rf_selected(const i32 *__restrict__ lp_of, const double *__restrict__ flag, int stride, i32 p) {
    return p >= 0 && flag[(size_t)lp_of[p] * stride] != 0.0;
}
__global__ __launch_bounds__(RF_THREADS) void k_refresh_pairs_sel(i64 np, const i32 *__restrict__ a, const i32 *__restrict__ b, const double *__restrict__ nz,
                                                                  double *__restrict__ w, const i32 *__restrict__ lp_of, const double *__restrict__ flag, int stride) {
    const i64 t0 = ((i64)blockIdx.x * RF_THREADS + threadIdx.x) * RF_PER;
    for (i64 t = t0; t < min(np, t0 + RF_PER); ++t) {
        const i32 pa = a[t], pb = b[t];
        if (!rf_selected(lp_of, flag, stride, pa >= 0 ? pa : pb)) continue;
        w[t] = rf_value(nz, pa, nz[max(pa, 0)]) * rf_value(nz, pb, nz[max(pb, 0)]);
    }
}
__global__ __launch_bounds__(RF_THREADS) void k_refresh_gather_sel(i64 n, const i32 *__restrict__ src, const double *__restrict__ nz, double *__restrict__ out,
                                                                   const i32 *__restrict__ lp_of, const double *__restrict__ flag, int stride) {
    const i64 q0 = ((i64)blockIdx.x * RF_THREADS + threadIdx.x) * RF_PER;
    for (i64 q = q0; q < min(n, q0 + RF_PER); ++q) {
        const i32 p = src[q];
        if (rf_selected(lp_of, flag, stride, p)) out[q] = nz[p];
    }
}

inline unsigned rf_blocks(i64 n) { return (unsigned)((n + (i64)RF_THREADS * RF_PER - 1) / ((i64)RF_THREADS * RF_PER)); }

}  // namespace

void launch_refresh_pairs(hipStream_t st, i64 np, const i32 *a, const i32 *b, const double *nz, double *w) {
    if (np > 0) hipLaunchKernelGGL(k_refresh_pairs, dim3(rf_blocks(np)), dim3(RF_THREADS), 0, st, np, a, b, nz, w);
}
void launch_refresh_gather(hipStream_t st, i64 n, const i32 *src, const double *nz, double *out) {
    if (n > 0) hipLaunchKernelGGL(k_refresh_gather, dim3(rf_blocks(n)), dim3(RF_THREADS), 0, st, n, src, nz, out);
}
void launch_refresh_pairs_sel(hipStream_t st, i64 np, const i32 *a, const i32 *b, const double *nz, double *w, const i32 *lp_of, const double *flag, int stride) {
    if (np > 0) hipLaunchKernelGGL(k_refresh_pairs_sel, dim3(rf_blocks(np)), dim3(RF_THREADS), 0, st, np, a, b, nz, w, lp_of, flag, stride);
}
void launch_refresh_gather_sel(hipStream_t st, i64 n, const i32 *src, const double *nz, double *out, const i32 *lp_of, const double *flag, int stride) {
    if (n > 0) hipLaunchKernelGGL(k_refresh_gather_sel, dim3(rf_blocks(n)), dim3(RF_THREADS), 0, st, n, src, nz, out, lp_of, flag, stride);
}
void launch_refresh_dense(hipStream_t st, i64 m, i64 n, const double *A, i64 lda, double *dA, i64 dlda) {
    if (m <= 0 || n <= 0) return;
    const unsigned gy = (unsigned)std::min<i64>(n, 65535);
    hipLaunchKernelGGL(k_refresh_dense, dim3((unsigned)((dlda + RF_THREADS - 1) / RF_THREADS), gy), dim3(RF_THREADS), 0, st, m, n, A, lda, dA, dlda);
}

}  // namespace tlpk
