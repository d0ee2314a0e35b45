// ipm_batch_kernels.hip -- the homogeneous self-dual and the Mehrotra kernels of ipm_kernels.hip for a STACK of LPs on one handle
// (tlpk_ipm_load_batch; DESIGN.md sections 4b' and 4b'').  B LPs stacked into one block-diagonal A are an ordinary handle; what
// differs per LP is every scalar of the interior-point loop (tau, eta, gamma mu, delta, dtau, the step length, the
// regularisations) and whether the LP is still being iterated at all.
//
//   * Segments.  LP k owns the rows [row_off[k], row_off[k + 1]) and the columns [col_off[k], col_off[k + 1]).
//   * Workgroups.  A block table maps blockIdx.x to (LP, block within the LP): every workgroup works inside one LP, reads
//     that LP's scalars from B.sc (wave-uniform index) and runs the unbatched grid-stride loop over the LP's range with as
//     many blocks as ipm_kernels.hip launches for a vector of the LP's length.
//   * Reductions.  partials[block][slot] through the trees of ipm_shared.hpp; k_ipmb_finalize runs one wave per (LP, slot):
//     lane l combines the LP's blocks l, l + 64, ... in that order, then the fixed butterfly.  No floating-point atomics.
//     What an LP's reductions return does not depend on what else is in the batch; with one LP they are the unbatched ones
//     bit for bit (tests/test_hsd_batch.py).
//   * Inactive LPs (flag 0: finished, failed, or masked out of a corrector round) are SKIPPED, not multiplied by zero: no
//     kernel writes their iterate, direction or right-hand sides, and their outputs are written as 0.  The KKT solves of the
//     batched calls write scratch vectors; k_ipmb_take copies the active LPs' segments to where they belong.
//   * Nothing waits inside a kernel: bounded grid-stride passes and __syncthreads only.
//
// The per-entry bodies are those of ipm_kernels.hip (ipm_shared.hpp): the formulas exist once.
#include <hip/hip_runtime.h>

#include "ipm_shared.hpp"
#include "tlpk_ipm.hpp"

namespace tlpk {

static_assert(IPM_T == 256, "ipm_seg_blocks (tlpk_ipm.hpp) sizes the block tables for workgroups of 256");

namespace {
// what a workgroup knows about its LP
struct Seg { int k, lb, nbk; const double *sc; bool active; i64 c0, nk, r0, mk; };
__device__ __forceinline__ Seg seg_of(const IpmBatch &B, const IpmBlockTab &t) {
    Seg s;
    s.k = t.seg[blockIdx.x]; s.lb = t.loc[blockIdx.x]; s.nbk = t.first[s.k + 1] - t.first[s.k];
    s.sc = B.sc + (size_t)s.k * IPM_BSC;
    s.active = s.sc[IPM_BSC - 1] != 0.0;
    s.c0 = B.col_off[s.k]; s.nk = B.col_off[s.k + 1] - s.c0;
    s.r0 = B.row_off[s.k]; s.mk = B.row_off[s.k + 1] - s.r0;
    return s;
}
}  // namespace

// one workgroup per LP, one wave per slot: k_ipm_finalize's order restricted to the LP's blocks
__global__ __launch_bounds__(64 * IPM_SLOTS) void k_ipmb_finalize(IpmBatch B, IpmBlockTab t, int nsum, int nmax, int nmin, const double *__restrict__ partials, double *__restrict__ out) {
    const int seg = blockIdx.x, k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (k >= nsum + nmax + nmin) return;                                     // (wave-uniform)
    double *o = out + (size_t)seg * IPM_SLOTS;
    if (B.sc[(size_t)seg * IPM_BSC + IPM_BSC - 1] == 0.0) { if (lane == 0) o[k] = 0.0; return; }      // its blocks wrote no partials
    const int first = t.first[seg], nblocks = t.first[seg + 1] - first;
    const int op = (k < nsum) ? 0 : (k < nsum + nmax ? 1 : 2);
    double r = (op == 0) ? 0.0 : (op == 1 ? -INFINITY : INFINITY);
    for (int b = lane; b < nblocks; b += 64) {
        const double v = partials[(size_t)(first + b) * IPM_SLOTS + k];
        r = (op == 0) ? r + v : (op == 1 ? fmax(r, v) : fmin(r, v));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double v = __shfl_xor(r, off, 64);
        r = (op == 0) ? r + v : (op == 1 ? fmax(r, v) : fmin(r, v));
    }
    if (lane == 0) o[k] = r;
}

// tlpk_ipm_batch_refill: the starting point of k_ipm_init for the LPs whose flag is set (the slots that take a new LP); a workgroup of any
// other LP returns before it touches anything
__global__ void k_ipmb_init(IpmVecs v, IpmBatch B) {
    const Seg g = seg_of(B, B.tb);
    if (!g.active) return;
    const i64 stride = (i64)g.nbk * blockDim.x, t0 = (i64)g.lb * blockDim.x + threadIdx.x;
    for (i64 jj = t0; jj < g.nk; jj += stride) ipm_init_col(v, g.c0 + jj);
    for (i64 ii = t0; ii < g.mk; ii += stride) v.y[g.r0 + ii] = 0.0;
}

// sc[0] = tau
__global__ __launch_bounds__(IPM_T) void k_ipmb_res_cols(IpmVecs v, IpmBatch B, double *__restrict__ partials) {
    __shared__ double sh[IPM_T];
    const Seg g = seg_of(B, B.tc);
    if (!g.active) return;                                                   // (block-uniform)
    const double tau = g.sc[0];
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0, m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0, m5 = 0;
    const i64 stride = (i64)g.nbk * blockDim.x;
    for (i64 jj = (i64)g.lb * blockDim.x + threadIdx.x; jj < g.nk; jj += stride) {
        ipm_res_col(v, g.c0 + jj, tau, s0, s1, s2, s3, m0, m1, m2, m3, m4, m5);
    }
    double *P = partials + (size_t)blockIdx.x * IPM_SLOTS;
    double r;
    r = blk_sum(s0, sh); if (threadIdx.x == 0) P[0] = r;
    r = blk_sum(s1, sh); if (threadIdx.x == 0) P[1] = r;
    r = blk_sum(s2, sh); if (threadIdx.x == 0) P[2] = r;
    r = blk_sum(s3, sh); if (threadIdx.x == 0) P[3] = r;
    r = blk_max(m0, sh); if (threadIdx.x == 0) P[4] = r;
    r = blk_max(m1, sh); if (threadIdx.x == 0) P[5] = r;
    r = blk_max(m2, sh); if (threadIdx.x == 0) P[6] = r;
    r = blk_max(m3, sh); if (threadIdx.x == 0) P[7] = r;
    r = blk_max(m4, sh); if (threadIdx.x == 0) P[8] = r;
    r = blk_max(m5, sh); if (threadIdx.x == 0) P[9] = r;
}
// sc[0] = tau.  8 lanes per row and the same number of trips for every group of the LP (`mround`), as k_ipm_res_rows
__global__ __launch_bounds__(IPM_T) void k_ipmb_res_rows(IpmVecs v, IpmBatch B, double *__restrict__ partials) {
    __shared__ double sh[IPM_T];
    const Seg g = seg_of(B, B.tr);
    if (!g.active) return;
    const double tau = g.sc[0];
    double s0 = 0, m0 = 0, m1 = 0;
    const int lane = threadIdx.x & 7;
    const i64 stride = ((i64)g.nbk * blockDim.x) >> 3;
    const i64 mround = (g.mk + stride - 1) / stride * stride;
    for (i64 ii = ((i64)g.lb * blockDim.x + threadIdx.x) >> 3; ii < mround; ii += stride) {
        ipm_res_row(v, g.r0 + ii, ii < g.mk, lane, tau, s0, m0, m1);
    }
    double *P = partials + (size_t)blockIdx.x * IPM_SLOTS;
    double r;
    r = blk_sum(s0, sh); if (threadIdx.x == 0) P[0] = r;
    r = blk_max(m0, sh); if (threadIdx.x == 0) P[1] = r;
    r = blk_max(m1, sh); if (threadIdx.x == 0) P[2] = r;
}

// sc[0] = regP, sc[1] = regD of the LP.  A PARKED LP (flag 0) gets theta_inv = 1, Rp = Rd = 1 on its block -- the matrix the handle is
// analysed with: a finished or failed LP can never fail the update of the others.  Its thl / thu (LP state) stay as they are.
__global__ void k_ipmb_theta(IpmVecs v, IpmBatch B, double *__restrict__ theta, double *__restrict__ regP, double *__restrict__ regD) {
    const Seg g = seg_of(B, B.tb);
    const double rP = g.active ? g.sc[0] : 1.0, rD = g.active ? g.sc[1] : 1.0;
    const i64 stride = (i64)g.nbk * blockDim.x, t0 = (i64)g.lb * blockDim.x + threadIdx.x;
    for (i64 jj = t0; jj < g.nk; jj += stride) {
        const i64 j = g.c0 + jj;
        if (g.active) ipm_theta_col(v, j, theta);
        else theta[j] = 1.0;
        regP[j] = rP;
    }
    for (i64 ii = t0; ii < g.mk; ii += stride) regD[g.r0 + ii] = rD;
}
__global__ void k_ipmb_hrhs(IpmVecs v, IpmBatch B) {
    const Seg g = seg_of(B, B.tc);
    if (!g.active) return;
    const i64 stride = (i64)g.nbk * blockDim.x;
    for (i64 jj = (i64)g.lb * blockDim.x + threadIdx.x; jj < g.nk; jj += stride) ipm_hrhs_col(v, g.c0 + jj);
}
__global__ __launch_bounds__(IPM_T) void k_ipmb_hdots(IpmVecs v, IpmBatch B, double *__restrict__ partials) {
    __shared__ double sh[IPM_T];
    const Seg g = seg_of(B, B.tb);
    if (!g.active) return;
    double s0 = 0, s1 = 0;
    const i64 stride = (i64)g.nbk * blockDim.x, t0 = (i64)g.lb * blockDim.x + threadIdx.x;
    for (i64 jj = t0; jj < g.nk; jj += stride) ipm_hdots_col(v, g.c0 + jj, s0);
    for (i64 ii = t0; ii < g.mk; ii += stride) { const i64 i = g.r0 + ii; s1 += v.b[i] * v.hy[i]; }
    double *P = partials + (size_t)blockIdx.x * IPM_SLOTS;
    double r;
    r = blk_sum(s0, sh); if (threadIdx.x == 0) P[0] = r;
    r = blk_sum(s1, sh); if (threadIdx.x == 0) P[1] = r;
}

// HSD (TWO = false): sc[0] = a_ (one trial step length for both sides), sc[1] = mu_l, sc[2] = mu_u
// MPC (TWO = true):  sc[0] = ap_, sc[1] = ad_ (primal and dual trial step lengths), sc[2] = tmin, sc[3] = tmax
template <bool TWO>
__global__ __launch_bounds__(IPM_T) void k_ipmb_targets(IpmVecs v, IpmDir D, IpmBatch B, double *__restrict__ partials) {
    __shared__ double sh[IPM_T];
    const Seg g = seg_of(B, B.tc);
    if (!g.active) return;
    const double a_p = g.sc[0], a_d = TWO ? g.sc[1] : g.sc[0], mu_l = TWO ? g.sc[2] : g.sc[1], mu_u = TWO ? g.sc[3] : g.sc[2];
    double s0 = 0, s1 = 0;
    const i64 stride = (i64)g.nbk * blockDim.x;
    for (i64 jj = (i64)g.lb * blockDim.x + threadIdx.x; jj < g.nk; jj += stride) ipm_targets_col(v, D, g.c0 + jj, a_p, a_d, mu_l, mu_u, s0, s1);
    double *P = partials + (size_t)blockIdx.x * IPM_SLOTS;
    double r;
    r = blk_sum(s0, sh); if (threadIdx.x == 0) P[0] = r;
    r = blk_sum(s1, sh); if (threadIdx.x == 0) P[1] = r;
}

// sc[0] = eta, sc[1] = gamma mu, sc[2] = delta; mode as k_ipm_newton_pre (one mode per call, the same for every LP)
__global__ __launch_bounds__(IPM_T) void k_ipmb_newton_pre(IpmVecs v, IpmDir D, IpmBatch B, int mode, double *__restrict__ partials) {
    __shared__ double sh[IPM_T];
    const Seg g = seg_of(B, B.tb);
    if (!g.active) return;
    const double eta = g.sc[0], gmu = g.sc[1], delta = g.sc[2];
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    const i64 stride = (i64)g.nbk * blockDim.x, t0 = (i64)g.lb * blockDim.x + threadIdx.x;
    for (i64 jj = t0; jj < g.nk; jj += stride) ipm_newton_pre_col(v, D, g.c0 + jj, mode, eta, gmu, delta, s0, s1, s2, s3);
    for (i64 ii = t0; ii < g.mk; ii += stride) ipm_newton_pre_row(v, g.r0 + ii, mode, eta);
    double *P = partials + (size_t)blockIdx.x * IPM_SLOTS;
    double r;
    r = blk_sum(s0, sh); if (threadIdx.x == 0) P[0] = r;
    r = blk_sum(s1, sh); if (threadIdx.x == 0) P[1] = r;
    r = blk_sum(s2, sh); if (threadIdx.x == 0) P[2] = r;
    r = blk_sum(s3, sh); if (threadIdx.x == 0) P[3] = r;
}
__global__ __launch_bounds__(IPM_T) void k_ipmb_newton_dots(IpmVecs v, IpmDir D, IpmBatch B, double *__restrict__ partials) {
    __shared__ double sh[IPM_T];
    const Seg g = seg_of(B, B.tb);
    if (!g.active) return;
    double s0 = 0, s1 = 0;
    const i64 stride = (i64)g.nbk * blockDim.x, t0 = (i64)g.lb * blockDim.x + threadIdx.x;
    for (i64 jj = t0; jj < g.nk; jj += stride) ipm_newton_dots_col(v, D, g.c0 + jj, s0);
    for (i64 ii = t0; ii < g.mk; ii += stride) { const i64 i = g.r0 + ii; s1 += v.b[i] * D.y[i]; }
    double *P = partials + (size_t)blockIdx.x * IPM_SLOTS;
    double r;
    r = blk_sum(s0, sh); if (threadIdx.x == 0) P[4] = r;                     // slots 4, 5: the pre kernel's sums stay in 0..3
    r = blk_sum(s1, sh); if (threadIdx.x == 0) P[5] = r;
}
// sc[0] = dtau
__global__ __launch_bounds__(IPM_T) void k_ipmb_newton_post(IpmVecs v, IpmDir D, IpmDir Add, IpmBatch B, int add, double *__restrict__ partials) {
    __shared__ double sh[IPM_T];
    const Seg g = seg_of(B, B.tb);
    if (!g.active) return;
    const double dtau = g.sc[0];
    double amin_p = __builtin_inf(), amin_d = __builtin_inf();
    const i64 stride = (i64)g.nbk * blockDim.x, t0 = (i64)g.lb * blockDim.x + threadIdx.x;
    for (i64 jj = t0; jj < g.nk; jj += stride) ipm_newton_post_col(v, D, Add, g.c0 + jj, add, dtau, amin_p, amin_d);
    for (i64 ii = t0; ii < g.mk; ii += stride) ipm_newton_post_row(v, D, Add, g.r0 + ii, add, dtau);
    double r = blk_min(amin_p, sh);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.x * IPM_SLOTS + 0] = r;
    r = blk_min(amin_d, sh);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.x * IPM_SLOTS + 1] = r;
}
// HSD (TWO = false): sc[0] = alpha (both sides).  MPC (TWO = true): sc[0] = alpha_p (primal side), sc[1] = alpha_d (dual side)
template <bool TWO>
__global__ __launch_bounds__(IPM_T) void k_ipmb_advance(IpmVecs v, IpmDir D, IpmBatch B, double *__restrict__ partials) {
    __shared__ double sh[IPM_T];
    const Seg g = seg_of(B, B.tb);
    if (!g.active) return;
    const double alpha = g.sc[0], alpha_d = TWO ? g.sc[1] : g.sc[0];
    double s0 = 0;
    const i64 stride = (i64)g.nbk * blockDim.x, t0 = (i64)g.lb * blockDim.x + threadIdx.x;
    for (i64 jj = t0; jj < g.nk; jj += stride) ipm_advance_col(v, D, g.c0 + jj, alpha, alpha_d, s0);
    for (i64 ii = t0; ii < g.mk; ii += stride) { const i64 i = g.r0 + ii; v.y[i] += alpha_d * D.y[i]; }
    const double r = blk_sum(s0, sh);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.x * IPM_SLOTS + 0] = r;
}
// tlpk_ipm_batch_accept: the LPs accept their candidates independently, so the two direction buffers cannot swap roles as they do behind
// tlpk_ipm_accept -- the candidate of every accepting LP is copied over its accepted direction
__global__ void k_ipmb_accept(IpmDir dst, IpmDir src, IpmBatch B) {
    const Seg g = seg_of(B, B.tb);
    if (!g.active) return;
    const i64 stride = (i64)g.nbk * blockDim.x, t0 = (i64)g.lb * blockDim.x + threadIdx.x;
    for (i64 jj = t0; jj < g.nk; jj += stride) { const i64 j = g.c0 + jj; dst.x[j] = src.x[j]; dst.xl[j] = src.xl[j]; dst.xu[j] = src.xu[j]; dst.zl[j] = src.zl[j]; dst.zu[j] = src.zu[j]; }
    for (i64 ii = t0; ii < g.mk; ii += stride) { const i64 i = g.r0 + ii; dst.y[i] = src.y[i]; }
}
// A KKT solve writes whole stacked vectors, the segments of the inactive LPs with them (their right-hand sides are whatever their last call
// left).  So the batched calls solve into scratch vectors and the ACTIVE LPs take their segments from there: an inactive LP's direction and
// h-system stay as they are, like everything else of it.
__global__ void k_ipmb_take(double *__restrict__ dx, double *__restrict__ dy, const double *__restrict__ sx, const double *__restrict__ sy, IpmBatch B) {
    const Seg g = seg_of(B, B.tb);
    if (!g.active) return;
    const i64 stride = (i64)g.nbk * blockDim.x, t0 = (i64)g.lb * blockDim.x + threadIdx.x;
    for (i64 jj = t0; jj < g.nk; jj += stride) { const i64 j = g.c0 + jj; dx[j] = sx[j]; }
    for (i64 ii = t0; ii < g.mk; ii += stride) { const i64 i = g.r0 + ii; dy[i] = sy[i]; }
}

// ---------------------------------------------------------------------------------------------
// Mehrotra predictor-corrector on a stack of LPs (tlpk_mpc_batch_*): the segmented twins of k_mpc_fill, k_mpc_start1 .. 4 and k_mpc_gap.
// The Newton systems go through k_ipmb_newton_pre (eta = 1, delta = 0) and k_ipmb_newton_post (dtau = 0), the targets and the
// advance through the TWO = true forms above.
// ---------------------------------------------------------------------------------------------
__global__ void k_mpcb_fill(IpmVecs v, IpmBatch B, double *__restrict__ theta, double *__restrict__ regP, double *__restrict__ regD) {
    const Seg g = seg_of(B, B.tb);
    if (!g.active) return;
    const i64 stride = (i64)g.nbk * blockDim.x, t0 = (i64)g.lb * blockDim.x + threadIdx.x;
    for (i64 jj = t0; jj < g.nk; jj += stride) { const i64 j = g.c0 + jj; theta[j] = 0.0; regP[j] = 1.0; v.xid[j] = 0.0; v.hx[j] = 0.0; }
    for (i64 ii = t0; ii < g.mk; ii += stride) { const i64 i = g.r0 + ii; regD[i] = 1e-6; v.xip[i] = 0.0; v.hy[i] = 0.0; }
}
__global__ __launch_bounds__(IPM_T) void k_mpcb_start1(IpmVecs v, IpmBatch B, double *__restrict__ partials) {
    __shared__ double sh[IPM_T];
    const Seg g = seg_of(B, B.tc);
    if (!g.active) return;
    double m0 = 0.0, m1 = 0.0;
    const i64 stride = (i64)g.nbk * blockDim.x;
    for (i64 jj = (i64)g.lb * blockDim.x + threadIdx.x; jj < g.nk; jj += stride) mpc_start1_col(v, g.c0 + jj, m0, m1);
    double r = blk_min(m0, sh); if (threadIdx.x == 0) partials[(size_t)blockIdx.x * IPM_SLOTS + 0] = r;
    r = blk_min(m1, sh); if (threadIdx.x == 0) partials[(size_t)blockIdx.x * IPM_SLOTS + 1] = r;
}
// sc[0] = dxs
__global__ __launch_bounds__(IPM_T) void k_mpcb_start2(IpmVecs v, IpmBatch B, double *__restrict__ partials) {
    __shared__ double sh[IPM_T];
    const Seg g = seg_of(B, B.tc);
    if (!g.active) return;
    const double dxs = g.sc[0];
    double m0 = 0.0, m1 = 0.0;
    const i64 stride = (i64)g.nbk * blockDim.x;
    for (i64 jj = (i64)g.lb * blockDim.x + threadIdx.x; jj < g.nk; jj += stride) mpc_start2_col(v, g.c0 + jj, dxs, m0, m1);
    double r = blk_min(m0, sh); if (threadIdx.x == 0) partials[(size_t)blockIdx.x * IPM_SLOTS + 0] = r;
    r = blk_min(m1, sh); if (threadIdx.x == 0) partials[(size_t)blockIdx.x * IPM_SLOTS + 1] = r;
}
// sc[0] = dzs
__global__ __launch_bounds__(IPM_T) void k_mpcb_start3(IpmVecs v, IpmBatch B, double *__restrict__ partials) {
    __shared__ double sh[IPM_T];
    const Seg g = seg_of(B, B.tc);
    if (!g.active) return;
    const double dzs = g.sc[0];
    double s0 = 0, s1 = 0, s2 = 0;
    const i64 stride = (i64)g.nbk * blockDim.x;
    for (i64 jj = (i64)g.lb * blockDim.x + threadIdx.x; jj < g.nk; jj += stride) mpc_start3_col(v, g.c0 + jj, dzs, s0, s1, s2);
    double *P = partials + (size_t)blockIdx.x * IPM_SLOTS;
    double r = blk_sum(s0, sh); if (threadIdx.x == 0) P[0] = r;
    r = blk_sum(s1, sh); if (threadIdx.x == 0) P[1] = r;
    r = blk_sum(s2, sh); if (threadIdx.x == 0) P[2] = r;
}
// sc[0] = ddx, sc[1] = ddz
__global__ __launch_bounds__(IPM_T) void k_mpcb_start4(IpmVecs v, IpmBatch B, double *__restrict__ partials) {
    __shared__ double sh[IPM_T];
    const Seg g = seg_of(B, B.tc);
    if (!g.active) return;
    const double ddx = g.sc[0], ddz = g.sc[1];
    double s0 = 0;
    const i64 stride = (i64)g.nbk * blockDim.x;
    for (i64 jj = (i64)g.lb * blockDim.x + threadIdx.x; jj < g.nk; jj += stride) mpc_start4_col(v, g.c0 + jj, ddx, ddz, s0);
    const double r = blk_sum(s0, sh);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.x * IPM_SLOTS + 0] = r;
}
// sc[0] = ap, sc[1] = ad
__global__ __launch_bounds__(IPM_T) void k_mpcb_gap(IpmVecs v, IpmDir D, IpmBatch B, double *__restrict__ partials) {
    __shared__ double sh[IPM_T];
    const Seg g = seg_of(B, B.tc);
    if (!g.active) return;
    const double ap = g.sc[0], ad = g.sc[1];
    double s0 = 0, s1 = 0;
    const i64 stride = (i64)g.nbk * blockDim.x;
    for (i64 jj = (i64)g.lb * blockDim.x + threadIdx.x; jj < g.nk; jj += stride) mpc_gap_col(v, D, g.c0 + jj, ap, ad, s0, s1);
    double *P = partials + (size_t)blockIdx.x * IPM_SLOTS;
    double r = blk_sum(s0, sh); if (threadIdx.x == 0) P[0] = r;
    r = blk_sum(s1, sh); if (threadIdx.x == 0) P[1] = r;
}

// ---------------------------------------------------------------------------------------------
// The Mehrotra stream (tlpk_mpc_batch_factor_enter / _newton_enter): an LP that ENTERS a slot rides in the update and the two solves of the
// running LPs.  sc[IPM_ROLE] is the LP's role in the call; its `active` flag is 0, so every kernel above skips an entering LP.
// ---------------------------------------------------------------------------------------------
// k_ipmb_theta for the active and the parked LPs (sc[0] = regP, sc[1] = regD), k_mpcb_fill for the entering ones
// HOLD (tlpk_ipm_batch_factor_each): an LP with the role IPM_HOLD keeps every bit of its three segments
template <bool HOLD>
__global__ void k_mpcb_theta_enter(IpmVecs v, IpmBatch B, double *__restrict__ theta, double *__restrict__ regP, double *__restrict__ regD) {
    const Seg g = seg_of(B, B.tb);
    if (HOLD && g.sc[IPM_ROLE] == IPM_HOLD) return;                          // (block-uniform)
    const i64 stride = (i64)g.nbk * blockDim.x, t0 = (i64)g.lb * blockDim.x + threadIdx.x;
    if (g.sc[IPM_ROLE] == IPM_ENTERING) {                                    // (block-uniform)
        for (i64 jj = t0; jj < g.nk; jj += stride) { const i64 j = g.c0 + jj; theta[j] = 0.0; regP[j] = 1.0; v.xid[j] = 0.0; v.hx[j] = 0.0; }
        for (i64 ii = t0; ii < g.mk; ii += stride) { const i64 i = g.r0 + ii; regD[i] = 1e-6; v.xip[i] = 0.0; v.hy[i] = 0.0; }
        return;
    }
    const double rP = g.active ? g.sc[0] : 1.0, rD = g.active ? g.sc[1] : 1.0;
    for (i64 jj = t0; jj < g.nk; jj += stride) {
        const i64 j = g.c0 + jj;
        if (g.active) ipm_theta_col(v, j, theta);
        else theta[j] = 1.0;
        regP[j] = rP;
    }
    for (i64 ii = t0; ii < g.mk; ii += stride) regD[g.r0 + ii] = rD;
}
// the right-hand side of an entering LP's starting solve: mode 0 (0, c) for y, mode 1 (b, 0) for x (MPC.jl:371-377)
__global__ void k_mpcb_enter_rhs(IpmVecs v, IpmBatch B, int mode) {
    const Seg g = seg_of(B, B.tb);
    if (g.sc[IPM_ROLE] != IPM_ENTERING) return;
    const i64 stride = (i64)g.nbk * blockDim.x, t0 = (i64)g.lb * blockDim.x + threadIdx.x;
    for (i64 jj = t0; jj < g.nk; jj += stride) { const i64 j = g.c0 + jj; v.xid[j] = mode == 0 ? v.c[j] : 0.0; }
    for (i64 ii = t0; ii < g.mk; ii += stride) { const i64 i = g.r0 + ii; v.xip[i] = mode == 0 ? 0.0 : v.b[i]; }
}
// ... and its solution from the scratch vectors of the call's one solve: mode 0 -> (D0.x, y), mode 1 -> (x, D0.y); the half of the right-hand side that
// the solve used goes back to 0
__global__ void k_mpcb_enter_take(IpmVecs v, IpmDir D0, const double *__restrict__ sx, const double *__restrict__ sy, IpmBatch B, int mode) {
    const Seg g = seg_of(B, B.tb);
    if (g.sc[IPM_ROLE] != IPM_ENTERING) return;
    const i64 stride = (i64)g.nbk * blockDim.x, t0 = (i64)g.lb * blockDim.x + threadIdx.x;
    if (mode == 0) {
        for (i64 jj = t0; jj < g.nk; jj += stride) { const i64 j = g.c0 + jj; D0.x[j] = sx[j]; v.xid[j] = 0.0; }
        for (i64 ii = t0; ii < g.mk; ii += stride) { const i64 i = g.r0 + ii; v.y[i] = sy[i]; }
    } else {
        for (i64 jj = t0; jj < g.nk; jj += stride) { const i64 j = g.c0 + jj; v.x[j] = sx[j]; }
        for (i64 ii = t0; ii < g.mk; ii += stride) { const i64 i = g.r0 + ii; D0.y[i] = sy[i]; v.xip[i] = 0.0; }
    }
}
// tlpk_ipm_get_lps: the records of the LPs that leave, gathered for one copy.  blockIdx.x = segment of the table, the blocks of a column of the grid stride over it
__global__ void k_ipmb_gather_segs(const IpmGatherSeg *__restrict__ tab, double *__restrict__ out) {
    const IpmGatherSeg s = tab[blockIdx.x];
    const i64 stride = (i64)gridDim.y * blockDim.x;
    for (i64 q = (i64)blockIdx.y * blockDim.x + threadIdx.x; q < s.len; q += stride) out[s.dst + q] = s.src[q];
}

// ---------------------------------------------------------------------------------------------
void ipmb_launch_finalize(hipStream_t st, const IpmBatch &B, const IpmBlockTab &t, int nsum, int nmax, int nmin, const double *partials, double *out) {
    hipLaunchKernelGGL(k_ipmb_finalize, dim3((unsigned)B.nlp), dim3(64 * (nsum + nmax + nmin)), 0, st, B, t, nsum, nmax, nmin, partials, out);
}
void ipmb_launch_init(hipStream_t st, const IpmVecs &v, const IpmBatch &B) { hipLaunchKernelGGL(k_ipmb_init, dim3(B.tb.nblocks), dim3(IPM_T), 0, st, v, B); }
void ipmb_launch_res_cols(hipStream_t st, const IpmVecs &v, const IpmBatch &B, double *partials) { hipLaunchKernelGGL(k_ipmb_res_cols, dim3(B.tc.nblocks), dim3(IPM_T), 0, st, v, B, partials); }
void ipmb_launch_res_rows(hipStream_t st, const IpmVecs &v, const IpmBatch &B, double *partials) { hipLaunchKernelGGL(k_ipmb_res_rows, dim3(B.tr.nblocks), dim3(IPM_T), 0, st, v, B, partials); }
void ipmb_launch_theta(hipStream_t st, const IpmVecs &v, const IpmBatch &B, double *theta, double *regP, double *regD) {
    hipLaunchKernelGGL(k_ipmb_theta, dim3(B.tb.nblocks), dim3(IPM_T), 0, st, v, B, theta, regP, regD);
}
void ipmb_launch_hrhs(hipStream_t st, const IpmVecs &v, const IpmBatch &B) { hipLaunchKernelGGL(k_ipmb_hrhs, dim3(B.tc.nblocks), dim3(IPM_T), 0, st, v, B); }
void ipmb_launch_hdots(hipStream_t st, const IpmVecs &v, const IpmBatch &B, double *partials) { hipLaunchKernelGGL(k_ipmb_hdots, dim3(B.tb.nblocks), dim3(IPM_T), 0, st, v, B, partials); }
void ipmb_launch_targets(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmBatch &B, double *partials) {
    hipLaunchKernelGGL(k_ipmb_targets<false>, dim3(B.tc.nblocks), dim3(IPM_T), 0, st, v, D, B, partials);
}
void ipmb_launch_newton_pre(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmBatch &B, int mode, double *partials) {
    hipLaunchKernelGGL(k_ipmb_newton_pre, dim3(B.tb.nblocks), dim3(IPM_T), 0, st, v, D, B, mode, partials);
}
void ipmb_launch_newton_dots(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmBatch &B, double *partials) {
    hipLaunchKernelGGL(k_ipmb_newton_dots, dim3(B.tb.nblocks), dim3(IPM_T), 0, st, v, D, B, partials);
}
void ipmb_launch_newton_post(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmDir &Add, const IpmBatch &B, int add, double *partials) {
    hipLaunchKernelGGL(k_ipmb_newton_post, dim3(B.tb.nblocks), dim3(IPM_T), 0, st, v, D, Add, B, add, partials);
}
void ipmb_launch_advance(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmBatch &B, double *partials) {
    hipLaunchKernelGGL(k_ipmb_advance<false>, dim3(B.tb.nblocks), dim3(IPM_T), 0, st, v, D, B, partials);
}
void ipmb_launch_take(hipStream_t st, double *dx, double *dy, const double *sx, const double *sy, const IpmBatch &B) {
    hipLaunchKernelGGL(k_ipmb_take, dim3(B.tb.nblocks), dim3(IPM_T), 0, st, dx, dy, sx, sy, B);
}
void ipmb_launch_accept(hipStream_t st, const IpmDir &dst, const IpmDir &src, const IpmBatch &B) { hipLaunchKernelGGL(k_ipmb_accept, dim3(B.tb.nblocks), dim3(IPM_T), 0, st, dst, src, B); }

void mpcb_launch_fill(hipStream_t st, const IpmVecs &v, const IpmBatch &B, double *theta, double *regP, double *regD) {
    hipLaunchKernelGGL(k_mpcb_fill, dim3(B.tb.nblocks), dim3(IPM_T), 0, st, v, B, theta, regP, regD);
}
void mpcb_launch_start(hipStream_t st, const IpmVecs &v, const IpmBatch &B, int stage, double *partials) {
    if (stage == 1) hipLaunchKernelGGL(k_mpcb_start1, dim3(B.tc.nblocks), dim3(IPM_T), 0, st, v, B, partials);
    else if (stage == 2) hipLaunchKernelGGL(k_mpcb_start2, dim3(B.tc.nblocks), dim3(IPM_T), 0, st, v, B, partials);
    else if (stage == 3) hipLaunchKernelGGL(k_mpcb_start3, dim3(B.tc.nblocks), dim3(IPM_T), 0, st, v, B, partials);
    else hipLaunchKernelGGL(k_mpcb_start4, dim3(B.tc.nblocks), dim3(IPM_T), 0, st, v, B, partials);
}
void mpcb_launch_gap(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmBatch &B, double *partials) {
    hipLaunchKernelGGL(k_mpcb_gap, dim3(B.tc.nblocks), dim3(IPM_T), 0, st, v, D, B, partials);
}
void mpcb_launch_targets(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmBatch &B, double *partials) {
    hipLaunchKernelGGL(k_ipmb_targets<true>, dim3(B.tc.nblocks), dim3(IPM_T), 0, st, v, D, B, partials);
}
void mpcb_launch_advance(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmBatch &B, double *partials) {
    hipLaunchKernelGGL(k_ipmb_advance<true>, dim3(B.tb.nblocks), dim3(IPM_T), 0, st, v, D, B, partials);
}
void mpcb_launch_theta_enter(hipStream_t st, const IpmVecs &v, const IpmBatch &B, double *theta, double *regP, double *regD) {
    hipLaunchKernelGGL(k_mpcb_theta_enter<false>, dim3(B.tb.nblocks), dim3(IPM_T), 0, st, v, B, theta, regP, regD);
}
void ipmb_launch_theta_roles(hipStream_t st, const IpmVecs &v, const IpmBatch &B, double *theta, double *regP, double *regD) {
    hipLaunchKernelGGL(k_mpcb_theta_enter<true>, dim3(B.tb.nblocks), dim3(IPM_T), 0, st, v, B, theta, regP, regD);
}
void mpcb_launch_enter_rhs(hipStream_t st, const IpmVecs &v, const IpmBatch &B, int mode) {
    hipLaunchKernelGGL(k_mpcb_enter_rhs, dim3(B.tb.nblocks), dim3(IPM_T), 0, st, v, B, mode);
}
void mpcb_launch_enter_take(hipStream_t st, const IpmVecs &v, const IpmDir &D0, const double *sx, const double *sy, const IpmBatch &B, int mode) {
    hipLaunchKernelGGL(k_mpcb_enter_take, dim3(B.tb.nblocks), dim3(IPM_T), 0, st, v, D0, sx, sy, B, mode);
}
void ipmb_launch_gather_segs(hipStream_t st, const IpmGatherSeg *tab, i64 nseg, i64 maxlen, double *out) {
    if (nseg < 1) return;
    const unsigned ny = (unsigned)std::max<i64>(1, std::min<i64>(64, (maxlen + 4 * IPM_T - 1) / (4 * IPM_T)));
    hipLaunchKernelGGL(k_ipmb_gather_segs, dim3((unsigned)nseg, ny), dim3(IPM_T), 0, st, tab, out);
}

}  // namespace tlpk
