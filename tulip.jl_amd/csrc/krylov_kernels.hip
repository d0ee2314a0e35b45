// krylov_kernels.hip -- matrix-free K1: preconditioned conjugate gradients on S dy = b, S = A D A' + Rd (tlpk_options.krylov; DESIGN.md
// section 1b'''').  S is never formed: one product with S is a pass over the CSC copy of A (t = D .* A'p, by columns) and a pass over
// its row-wise copy (q = A t + Rd .* p, by rows).
//
// One iteration = four launches and no host involvement:
//   k_cg_cols   t = D .* (A' p)
//   k_cg_rows   q = A t + Rd .* p, partial sums of p'q          -> one slot per workgroup
//   k_cg_step   alpha = gamma / p'q;  x += alpha p;  r -= alpha q;  partial sums of r'z, z = M^-1 r     -> one slot per workgroup
//   k_cg_dir    gamma' = r'z;  stopping rule;  beta = gamma' / gamma;  p = z + beta p;  counter, outcome
// Scalars live in CgScalars (tlpk_device.hpp).  A workgroup reduces its partial sum with a fixed shuffle tree and writes it to its slot; every
// workgroup of the consuming kernel adds the slots in slot order.  No atomics: two solves of the same data are bit-identical.  Every kernel reads
// the outcome word first and returns when it is set: iterations enqueued past the end of a solve cost a launch each and change nothing.
// No kernel waits for another one: nothing here can hang.
//
// Rows and columns of an LP hold a handful of entries: 8 lanes per row, 4 per column.  A row or column with more than CG_LONG entries (a linking
// row, a dense column) is listed at create and gets a whole workgroup in the same launch (the blocks behind those of the short ones).
// The gather itself is krylov_spmv.hpp's: a kernel here supplies the addend of an entry and what one lane does with a finished sum.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "krylov_reduce.hpp"
#include "krylov_spmv.hpp"
#include "tlpk_device.hpp"

namespace tlpk {

namespace {

constexpr int CG_ROW_THREADS = 1024;    // k_cg_rows: its workgroups are capped at CG_MAX_SLOTS (one partial sum each), so each is as large as it can be

constexpr int CG_SLOTS_LDS = CG_MAX_SLOTS + CG_MAX_LONG;
// M_i = sum_j A_ij^2 D_j + Rd_i, stored inverted.  Blocks [0, gs): 8 lanes per row; blocks behind: one long row each.
__global__ __launch_bounds__(CG_THREADS) void k_cg_jacobi(i64 m, const i64 *__restrict__ Tp, const i32 *__restrict__ Tj, const double *__restrict__ Tx,
                                                          const double *__restrict__ D, const double *__restrict__ regD, double *__restrict__ Minv,
                                                          unsigned gs, const i32 *__restrict__ long_rows) {
    __shared__ double sh[CG_THREADS / 64];
    const auto term = [&](i64 q) { return Tx[q] * Tx[q] * D[Tj[q]]; };
    const auto done = [&](i64 i, double s) { Minv[i] = cg_minv(s + regD[i]); };
    const unsigned n_long = gridDim.x - gs;
    if (blockIdx.x < gs) walk_short<CG_THREADS, 8>(m, Tp, blockIdx.x, gs, term, done);
    else walk_long<CG_THREADS>(long_rows, n_long, blockIdx.x - gs, n_long, Tp, sh, term, done);
}

// x = 0, p = z = M^-1 r, partial sums of r'z
__global__ __launch_bounds__(CG_THREADS) void k_cg_init(i64 m, const double *__restrict__ r, const double *__restrict__ Minv, double *__restrict__ x,
                                                        double *__restrict__ p, double *__restrict__ slots_v) {
    __shared__ double sh[CG_THREADS / 64];
    double acc = 0.0;
    for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < m; i += (i64)gridDim.x * CG_THREADS) {
        const double ri = r[i], z = Minv ? Minv[i] * ri : ri;
        x[i] = 0.0; p[i] = z;
        acc += ri * z;
    }
    acc = cg_block_sum(acc, sh);
    if (threadIdx.x == 0) slots_v[blockIdx.x] = acc;
}
// one workgroup (its first thread writes): gamma at x = 0, the tolerance of this solve, the outcome word
__global__ __launch_bounds__(CG_THREADS) void k_cg_init_scalars(CgScalars *__restrict__ sc, const double *__restrict__ slots_v, int ns, double atol, double rtol,
                                                                long long itmax) {
    __shared__ double shs[CG_SLOTS_LDS];
    const double g0 = cg_sum_slots(slots_v, ns, shs);
    if (threadIdx.x != 0) return;
    const double rho0 = sqrt(g0), tol = atol + rtol * rho0;
    sc->gamma[0] = g0; sc->gamma[1] = g0;
    sc->tol = tol; sc->resid0 = rho0; sc->resid = rho0; sc->pq = 0.0;
    sc->iters = 0; sc->itmax = itmax;
    sc->outcome = !(g0 >= 0.0 && isfinite(g0)) ? CG_BREAKDOWN : (rho0 <= tol ? CG_SOLVED : (itmax <= 0 ? CG_ITMAX : CG_RUNNING));
}

// t = D .* (A' p).  Blocks [0, gs): 4 lanes per column; blocks behind: one long column each.
__global__ __launch_bounds__(CG_THREADS) void k_cg_cols(const CgScalars *__restrict__ sc, i64 n, const i64 *__restrict__ Ap, const i32 *__restrict__ Ai,
                                                        const double *__restrict__ Ax, const double *__restrict__ D, const double *__restrict__ p,
                                                        double *__restrict__ t, unsigned gs, const i32 *__restrict__ long_cols) {
    __shared__ double sh[CG_THREADS / 64];
    if (sc->outcome != CG_RUNNING) return;
    const auto term = [&](i64 q) { return Ax[q] * p[Ai[q]]; };
    const auto done = [&](i64 j, double s) { t[j] = D[j] * s; };
    const unsigned n_long = gridDim.x - gs;
    if (blockIdx.x < gs) walk_short<CG_THREADS, 4>(n, Ap, blockIdx.x, gs, term, done);
    else walk_long<CG_THREADS>(long_cols, n_long, blockIdx.x - gs, n_long, Ap, sh, term, done);
}

// q = A t + Rd .* p and the partial sums of p'q.  Blocks [0, gs): 8 lanes per row, rows handed out round by round (every wave makes the same number
// of rounds); blocks [gs, gs + gl): the long rows, a workgroup per row.  Slot = block index.
__global__ __launch_bounds__(CG_ROW_THREADS) void k_cg_rows(const CgScalars *__restrict__ sc, i64 m, const i64 *__restrict__ Tp, const i32 *__restrict__ Tj,
                                                        const double *__restrict__ Tx, const double *__restrict__ t, const double *__restrict__ regD,
                                                        const double *__restrict__ p, double *__restrict__ qv, double *__restrict__ slots_r, unsigned gs,
                                                        unsigned gl, const i32 *__restrict__ long_rows, i64 n_long) {
    __shared__ double sh[CG_ROW_THREADS / 64];
    if (sc->outcome != CG_RUNNING) return;
    double acc = 0.0;      // this workgroup's part of p'q: spread over the lanes of the short rows, on the first thread of the long ones
    const auto term = [&](i64 q) { return Tx[q] * t[Tj[q]]; };
    const auto done = [&](i64 i, double s) { const double pi = p[i], qi = s + regD[i] * pi; qv[i] = qi; acc += pi * qi; };
    if (blockIdx.x >= gs) {          // (the long rows first and on a path of their own: testing the short ones first measured 0.5 us per iteration slower)
        walk_long<CG_ROW_THREADS>(long_rows, n_long, blockIdx.x - gs, gl, Tp, sh, term, done);
        if (threadIdx.x == 0) slots_r[blockIdx.x] = acc;
        return;
    }
    walk_short<CG_ROW_THREADS, 8>(m, Tp, blockIdx.x, gs, term, done);
    acc = cg_block_sum<CG_ROW_THREADS>(acc, sh);
    if (threadIdx.x == 0) slots_r[blockIdx.x] = acc;
}

// alpha = gamma / p'q;  x += alpha p;  r -= alpha q;  partial sums of r'z.  p'q <= 0 or a scalar that is not finite: the solve ends as not solved
// (every workgroup sees the same sum and returns; the first one records it).
__global__ __launch_bounds__(CG_THREADS) void k_cg_step(CgScalars *__restrict__ sc, int par, i64 m, double *__restrict__ x, double *__restrict__ r,
                                                        const double *__restrict__ p, const double *__restrict__ qv, const double *__restrict__ Minv,
                                                        const double *__restrict__ slots_r, int ns_r, double *__restrict__ slots_v) {
    __shared__ double sh[CG_THREADS / 64];
    __shared__ double shs[CG_SLOTS_LDS];
    if (sc->outcome != CG_RUNNING) return;
    const double pq = cg_sum_slots(slots_r, ns_r, shs);
    const double alpha = sc->gamma[par] / pq;
    if (!(pq > 0.0) || !isfinite(pq) || !isfinite(alpha)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { sc->pq = pq; sc->outcome = CG_BREAKDOWN; }
        return;
    }
    double acc = 0.0;
    for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < m; i += (i64)gridDim.x * CG_THREADS) {
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * qv[i];
        r[i] = ri;
        acc += ri * (Minv ? Minv[i] * ri : ri);
    }
    acc = cg_block_sum(acc, sh);
    if (threadIdx.x == 0) slots_v[blockIdx.x] = acc;
    if (blockIdx.x == 0 && threadIdx.x == 0) sc->pq = pq;
}

// gamma' = r'z;  solved when sqrt(gamma') <= tol, tired when k + 1 = itmax;  otherwise p = z + (gamma' / gamma) p.  The first workgroup's first thread
// writes the scalars of the next iteration (the other parity of gamma: the workgroups still running read this iteration's).
__global__ __launch_bounds__(CG_THREADS) void k_cg_dir(CgScalars *__restrict__ sc, int par, long long k, i64 m, const double *__restrict__ r,
                                                       const double *__restrict__ Minv, double *__restrict__ p, const double *__restrict__ slots_v, int ns_v) {
    __shared__ double shs[CG_SLOTS_LDS];
    if (sc->outcome != CG_RUNNING) return;
    const double g1 = cg_sum_slots(slots_v, ns_v, shs);
    const double g0 = sc->gamma[par];
    const double rho = sqrt(g1), beta = g1 / g0;
    const long long itmax = sc->itmax;
    const bool broken = !(g1 >= 0.0) || !isfinite(g1);
    const bool solved = !broken && rho <= sc->tol;
    const bool go_on = !broken && !solved && k + 1 < itmax && isfinite(beta);
    if (go_on)
        for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < m; i += (i64)gridDim.x * CG_THREADS) {
            const double ri = r[i];
            p[i] = (Minv ? Minv[i] * ri : ri) + beta * p[i];
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sc->gamma[par ^ 1] = g1;
        sc->resid = rho;
        sc->iters = k + 1;
        if (!go_on) sc->outcome = solved ? CG_SOLVED : ((broken || !isfinite(beta)) ? CG_BREAKDOWN : CG_ITMAX);
    }
}

}  // namespace

void launch_cg_jacobi(hipStream_t st, const DevArrays &a, const CgArrays &c, const double *D, const double *regD) {
    if (a.m <= 0 || !c.Minv) return;
    const unsigned gs = nblk(a.m * 8, CG_THREADS);
    hipLaunchKernelGGL(k_cg_jacobi, dim3(gs + (unsigned)c.geo.n_long_rows), dim3(CG_THREADS), 0, st, a.m, a.Tp, a.Tj, a.Tx, D, regD, c.Minv, gs, c.geo.long_rows);
}

void launch_cg_init(hipStream_t st, const DevArrays &a, const CgArrays &c, double atol, double rtol, i64 itmax) {
    if (a.m > 0) hipLaunchKernelGGL(k_cg_init, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, a.m, a.ctx.xw, c.Minv, c.x, c.p, c.slots_v);
    hipLaunchKernelGGL(k_cg_init_scalars, dim3(1), dim3(CG_THREADS), 0, st, c.sc, c.slots_v, a.m > 0 ? c.geo.g_vec : 0, atol, rtol, (long long)itmax);
}

int launch_cg_iter(hipStream_t st, const DevArrays &a, const CgArrays &c, const double *D, const double *regD, i64 k) {
    if (a.m <= 0) return 0;
    const int par = (int)(k & 1);
    int nl = 3;
    if (a.n > 0) {
        const unsigned gs = nblk(a.n * 4, CG_THREADS);
        hipLaunchKernelGGL(k_cg_cols, dim3(gs + (unsigned)c.geo.n_long_cols), dim3(CG_THREADS), 0, st, c.sc, a.n, a.Ap, a.Ai, a.Ax, D, c.p, c.t, gs, c.geo.long_cols);
        ++nl;
    }
    hipLaunchKernelGGL(k_cg_rows, dim3((unsigned)(c.geo.g_rows + c.geo.g_lrows)), dim3(CG_ROW_THREADS), 0, st, c.sc, a.m, a.Tp, a.Tj, a.Tx, c.t, regD, c.p, c.q, c.slots_r,
                       (unsigned)c.geo.g_rows, (unsigned)c.geo.g_lrows, c.geo.long_rows, c.geo.n_long_rows);
    hipLaunchKernelGGL(k_cg_step, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, c.sc, par, a.m, c.x, a.ctx.xw, c.p, c.q, c.Minv, c.slots_r, c.geo.g_rows + c.geo.g_lrows,
                       c.slots_v);
    hipLaunchKernelGGL(k_cg_dir, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, c.sc, par, (long long)k, a.m, a.ctx.xw, c.Minv, c.p, c.slots_v, c.geo.g_vec);
    return nl;
}

}  // namespace tlpk
