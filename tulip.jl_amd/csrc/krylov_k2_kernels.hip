// krylov_k2_kernels.hip -- matrix-free K2: preconditioned MINRES (Paige & Saunders) on K [dx; dy] = [xi_d; xi_p], K = [-E A'; A Rd], E = theta^-1 + Rp
// (tlpk_options.krylov = TLPK_KRYLOV_MINRES; DESIGN.md section 1b''''').  K is never formed.  The vectors of order N = n + m are stored [n-part; m-part].
// Both halves of K v read v only, so one product is ONE launch: the column lanes walk the CSC copy of A (u1 = -E .* v1 + A' v2), the row lanes its
// row-wise copy (u2 = A v1 + Rd .* v2).
//
// One iteration = three launches and no host involvement (k = 0, 1, ... is the 0-based iteration, par = k & 1):
//   k_mr_op     v = z[par] / beta (applied while gathering, never stored);  u = K v - (beta / oldb) r[par ^ 1];  partial sums of alpha = v'u
//   k_mr_step   alpha from the slots;  r[par ^ 1] = u - (alpha / beta) r[par]  (r1 and r2 rotate by parity);  z[par ^ 1] = M^-1 r[par ^ 1];
//               partial sums of r'z
//   k_mr_rot    beta' = sqrt(r'z);  the Givens rotation;  w[par] = (v - oldeps w[par] - delta w[par ^ 1]) / gamma;  x += phi w[par];
//               the scalars of the next iteration, the stopping rule, the counter, the outcome word
// Scalars live in MrScalars (tlpk_device.hpp): the recurrence's state twice, by parity of the iteration that reads it, so that the one thread that
// writes the next state never races the workgroups that still read this one.  Partial sums go one per workgroup to a slot and are added in slot order
// by every workgroup of the consumer (krylov_reduce.hpp): no atomics, two solves of the same data are bit-identical.  Every kernel reads the outcome
// word first and returns when it is set.  k_mr_rot is the kernel that SETS it, and a workgroup of it that starts late must still update its part of
// x: the word carries the number of the iteration that set it, and k_mr_rot returns only on a word of another iteration.  No kernel waits for
// another one: nothing here can hang.
//
// Rows and columns of an LP hold a handful of entries: 8 lanes per row, 4 per column, handed out round by round.  A row or column with more than
// CG_LONG entries is listed at create and gets a whole workgroup in the same launch, behind those of the short ones.
// The gather itself is krylov_spmv.hpp's: a kernel here supplies the addend of an entry and what one lane does with a finished sum.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "krylov_reduce.hpp"
#include "krylov_spmv.hpp"
#include "tlpk_device.hpp"

namespace tlpk {

namespace {

constexpr int MR_OP_THREADS = 1024;   // k_mr_op: its workgroups are capped (one partial sum each), so each is as large as it can be
constexpr int MR_SLOTS_LDS = 2 * CG_MAX_SLOTS + 2 * CG_MAX_LONG;

__device__ __forceinline__ bool mr_stopped(const MrScalars *sc) { return sc->outcome != CG_RUNNING; }

// E = theta^-1 + Rp; 1 / E is never formed outside the preconditioner
__global__ void k_mr_diag(i64 n, const double *__restrict__ theta, const double *__restrict__ regP, double *__restrict__ E) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) E[j] = theta[j] + regP[j];
}

// The block diagonal M = diag(E_j, s_i), s_i = sum_{j: E_j > 0} A_ij^2 / E_j + Rd_i, stored inverted; an entry that is 0 is replaced by 1 (cg_minv).
// Blocks [0, gs): 8 lanes per row; [gs, gs + n_long): one long row each; behind them: the columns, one thread each.
__global__ __launch_bounds__(CG_THREADS) void k_mr_jacobi(i64 n, i64 m, const i64 *__restrict__ Tp, const i32 *__restrict__ Tj, const double *__restrict__ Tx,
                                                          const double *__restrict__ E, const double *__restrict__ regD, double *__restrict__ Minv,
                                                          unsigned gs, unsigned n_long, const i32 *__restrict__ long_rows) {
    __shared__ double sh[CG_THREADS / 64];
    if (blockIdx.x >= gs + n_long) {
        const i64 j = (i64)(blockIdx.x - gs - n_long) * CG_THREADS + threadIdx.x;
        if (j < n) Minv[j] = cg_minv(E[j]);
        return;
    }
    const auto term = [&](i64 q) { const double e = E[Tj[q]]; return e > 0.0 ? Tx[q] * Tx[q] / e : 0.0; };      // (adding 0.0 leaves the sum as it is)
    const auto done = [&](i64 i, double s) { Minv[n + i] = cg_minv(s + regD[i]); };
    if (blockIdx.x < gs) walk_short<CG_THREADS, 8>(m, Tp, blockIdx.x, gs, term, done);
    else walk_long<CG_THREADS>(long_rows, n_long, blockIdx.x - gs, n_long, Tp, sh, term, done);
}

// r[0] = b = [xi_d; xi_p], z[0] = M^-1 b, x = w = 0, partial sums of b'z
__global__ __launch_bounds__(CG_THREADS) void k_mr_init(i64 n, i64 N, const double *__restrict__ xi_d, const double *__restrict__ xi_p, const double *__restrict__ Minv,
                                                        double *__restrict__ r0, double *__restrict__ z0, double *__restrict__ x, double *__restrict__ w0,
                                                        double *__restrict__ w1, double *__restrict__ slots_g) {
    __shared__ double sh[CG_THREADS / 64];
    double acc = 0.0;
    for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < N; i += (i64)gridDim.x * CG_THREADS) {
        const double bi = i < n ? xi_d[i] : xi_p[i - n], zi = Minv ? Minv[i] * bi : bi;
        r0[i] = bi;
        if (Minv) z0[i] = zi;         // (no preconditioner: z IS r, the same storage)
        x[i] = 0.0; w0[i] = 0.0; w1[i] = 0.0;
        acc += bi * zi;
    }
    acc = cg_block_sum(acc, sh);
    if (threadIdx.x == 0) slots_g[blockIdx.x] = acc;
}
// one workgroup (its first thread writes): beta1, the tolerance of this solve, the state of iteration 0, the outcome word
__global__ __launch_bounds__(CG_THREADS) void k_mr_init_scalars(MrScalars *__restrict__ sc, const double *__restrict__ slots_g, int ns, double atol, double rtol,
                                                                long long itmax) {
    __shared__ double shs[MR_SLOTS_LDS];
    const double g0 = cg_sum_slots(slots_g, ns, shs);
    if (threadIdx.x != 0) return;
    const double beta1 = sqrt(g0), tol = atol + rtol * beta1;
    MrState s;
    s.beta = beta1; s.oldb = 0.0; s.dbar = 0.0; s.eps = 0.0; s.cs = -1.0; s.sn = 0.0; s.phibar = beta1; s.pad = 0.0;
    sc->st[0] = s; sc->st[1] = s;
    sc->tol = tol; sc->resid0 = beta1; sc->resid = beta1; sc->alpha = 0.0;
    sc->iters = 0; sc->itmax = itmax;
    sc->outcome = !(g0 >= 0.0 && isfinite(g0)) ? CG_BREAKDOWN : (beta1 <= tol ? CG_SOLVED : (itmax <= 0 ? CG_ITMAX : CG_RUNNING));      // (iteration stamp 0)
}

// u = K v - (beta / oldb) r1 and the partial sums of v'u, v = z / beta.  Blocks [0, gc): 4 lanes per column; [gc, gc + gr): 8 lanes per row; then glc
// workgroups that share the long columns and glr that share the long rows.  Slot = block index.
__global__ __launch_bounds__(MR_OP_THREADS) void k_mr_op(const MrScalars *__restrict__ sc, int par, int first, i64 n, i64 m, const i64 *__restrict__ Ap,
                                                         const i32 *__restrict__ Ai, const double *__restrict__ Ax, const i64 *__restrict__ Tp,
                                                         const i32 *__restrict__ Tj, const double *__restrict__ Tx, const double *__restrict__ E,
                                                         const double *__restrict__ regD, const double *__restrict__ z, const double *__restrict__ r1,
                                                         double *__restrict__ u, double *__restrict__ slots_a, unsigned gc, unsigned gr, unsigned glc, unsigned glr,
                                                         const i32 *__restrict__ long_cols, i64 n_long_cols, const i32 *__restrict__ long_rows, i64 n_long_rows) {
    __shared__ double sh[MR_OP_THREADS / 64];
    if (mr_stopped(sc)) return;
    const double beta = sc->st[par].beta, c1 = first ? 0.0 : beta / sc->st[par].oldb;
    const double *__restrict__ z1 = z, *__restrict__ z2 = z + n;
    double acc = 0.0;
    const auto col_term = [&](i64 q) { return Ax[q] * (z2[Ai[q]] / beta); };
    const auto col_done = [&](i64 j, double s) {
        const double vj = z1[j] / beta;
        double uj = s - E[j] * vj;
        if (!first) uj -= c1 * r1[j];
        u[j] = uj; acc += vj * uj;
    };
    const auto row_term = [&](i64 q) { return Tx[q] * (z1[Tj[q]] / beta); };
    const auto row_done = [&](i64 i, double s) {
        const double vi = z2[i] / beta;
        double ui = s + regD[i] * vi;
        if (!first) ui -= c1 * r1[n + i];
        u[n + i] = ui; acc += vi * ui;
    };
    // acc: this workgroup's part of v'u, spread over the lanes of the short items, on the first thread of the long ones
    const unsigned b = blockIdx.x;
    if (b < gc + gr) {
        if (b < gc) walk_short<MR_OP_THREADS, 4>(n, Ap, b, gc, col_term, col_done);
        else walk_short<MR_OP_THREADS, 8>(m, Tp, b - gc, gr, row_term, row_done);
        acc = cg_block_sum<MR_OP_THREADS>(acc, sh);
    } else if (b < gc + gr + glc) {
        walk_long<MR_OP_THREADS>(long_cols, n_long_cols, b - gc - gr, glc, Ap, sh, col_term, col_done);
    } else {
        walk_long<MR_OP_THREADS>(long_rows, n_long_rows, b - gc - gr - glc, glr, Tp, sh, row_term, row_done);
    }
    if (threadIdx.x == 0) slots_a[b] = acc;
}

// The Lanczos step: alpha from the slots; r_new = u - (alpha / beta) r2, written over r1 (dead since k_mr_op); z_new = M^-1 r_new; partial sums of r_new'z_new
__global__ __launch_bounds__(CG_THREADS) void k_mr_step(MrScalars *__restrict__ sc, int par, i64 N, const double *__restrict__ u, const double *__restrict__ r2,
                                                        double *__restrict__ rn, double *__restrict__ zn, const double *__restrict__ Minv,
                                                        const double *__restrict__ slots_a, int ns_a, double *__restrict__ slots_g) {
    __shared__ double sh[CG_THREADS / 64];
    __shared__ double shs[MR_SLOTS_LDS];
    if (mr_stopped(sc)) return;
    const double alpha = cg_sum_slots(slots_a, ns_a, shs);
    const double c2 = alpha / sc->st[par].beta;
    double acc = 0.0;
    for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < N; i += (i64)gridDim.x * CG_THREADS) {
        const double ri = u[i] - c2 * r2[i], zi = Minv ? Minv[i] * ri : ri;
        rn[i] = ri;
        if (Minv) zn[i] = zi;
        acc += ri * zi;
    }
    acc = cg_block_sum(acc, sh);
    if (threadIdx.x == 0) slots_g[blockIdx.x] = acc;
    if (blockIdx.x == 0 && threadIdx.x == 0) sc->alpha = alpha;      // (no workgroup of this kernel reads it)
}

// The rotation and the update.  Every workgroup forms the same scalars from the same slots and the same state st[par]; the first one's first thread writes
// st[par ^ 1], the stopping rule, the counter and the outcome word (stamped with k + 1).  g < 0 or not finite: NOT solved, x stays.  beta' = 0: the
// Krylov space is exhausted, the solve stops (solved iff phibar <= tol).
__global__ __launch_bounds__(CG_THREADS) void k_mr_rot(MrScalars *__restrict__ sc, int par, long long k, i64 N, const double *__restrict__ z, double *__restrict__ w1,
                                                       const double *__restrict__ w2, double *__restrict__ x, const double *__restrict__ slots_g, int ns_g) {
    __shared__ double shs[MR_SLOTS_LDS];
    const long long word = sc->outcome;
    if (word != CG_RUNNING && (word >> 8) != k + 1) return;
    const double g = cg_sum_slots(slots_g, ns_g, shs);
    const MrState s = sc->st[par];
    const double alpha = sc->alpha, tol = sc->tol;
    const long long itmax = sc->itmax;
    const bool broken = !(g >= 0.0) || !isfinite(g);
    if (broken) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { sc->iters = k + 1; sc->outcome = CG_BREAKDOWN | ((k + 1) << 8); }
        return;
    }
    const double beta = sqrt(g);
    const double oldeps = s.eps, delta = s.cs * s.dbar + s.sn * alpha, gbar = s.sn * s.dbar - s.cs * alpha;
    const double gamma = fmax(hypot(gbar, beta), DBL_EPSILON), cs = gbar / gamma, sn = beta / gamma;
    const double phi = cs * s.phibar, phibar = sn * s.phibar;
    for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < N; i += (i64)gridDim.x * CG_THREADS) {
        const double wn = (z[i] / s.beta - oldeps * w1[i] - delta * w2[i]) / gamma;
        w1[i] = wn;
        x[i] += phi * wn;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        MrState t;
        t.beta = beta; t.oldb = s.beta; t.dbar = -s.cs * beta; t.eps = s.sn * beta;      // (both from the PREVIOUS rotation)
        t.cs = cs; t.sn = sn; t.phibar = phibar; t.pad = 0.0;
        sc->st[par ^ 1] = t;
        sc->resid = phibar;
        sc->iters = k + 1;
        const long long out = phibar <= tol ? CG_SOLVED : ((beta == 0.0 || !isfinite(phibar)) ? CG_BREAKDOWN : (k + 1 >= itmax ? CG_ITMAX : CG_RUNNING));
        if (out != CG_RUNNING) sc->outcome = out | ((k + 1) << 8);
    }
}

}  // namespace

void launch_mr_diag(hipStream_t st, i64 n, const double *theta, const double *regP, double *E) {
    if (n > 0) hipLaunchKernelGGL(k_mr_diag, dim3(nblk(n, 256)), dim3(256), 0, st, n, theta, regP, E);
}

void launch_mr_jacobi(hipStream_t st, const DevArrays &a, const MrArrays &c, const double *E, const double *regD) {
    if (a.m + a.n <= 0 || !c.Minv) return;
    const unsigned gs = a.m > 0 ? nblk(a.m * 8, CG_THREADS) : 0, gcol = a.n > 0 ? nblk(a.n, CG_THREADS) : 0;
    hipLaunchKernelGGL(k_mr_jacobi, dim3(gs + (unsigned)c.geo.n_long_rows + gcol), dim3(CG_THREADS), 0, st, a.n, a.m, a.Tp, a.Tj, a.Tx, E, regD, c.Minv, gs,
                       (unsigned)c.geo.n_long_rows, c.geo.long_rows);
}

void launch_mr_init(hipStream_t st, const DevArrays &a, const MrArrays &c, const double *xi_p, const double *xi_d, double atol, double rtol, i64 itmax) {
    const i64 N = a.n + a.m;
    if (N > 0)
        hipLaunchKernelGGL(k_mr_init, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, a.n, N, xi_d, xi_p, c.Minv, c.r[0], c.z[0], c.x, c.w[0], c.w[1], c.slots_g);
    hipLaunchKernelGGL(k_mr_init_scalars, dim3(1), dim3(CG_THREADS), 0, st, c.sc, c.slots_g, N > 0 ? c.geo.g_vec : 0, atol, rtol, (long long)itmax);
}

int launch_mr_iter(hipStream_t st, const DevArrays &a, const MrArrays &c, const double *E, const double *regD, i64 k) {
    const i64 N = a.n + a.m;
    if (N <= 0) return 0;
    const int par = (int)(k & 1);
    const int ns_a = c.geo.g_cols + c.geo.g_rows + c.geo.g_lcols + c.geo.g_lrows;
    hipLaunchKernelGGL(k_mr_op, dim3((unsigned)ns_a), dim3(MR_OP_THREADS), 0, st, c.sc, par, k == 0 ? 1 : 0, a.n, a.m, a.Ap, a.Ai, a.Ax, a.Tp, a.Tj, a.Tx, E, regD,
                       c.z[par], c.r[par ^ 1], c.u, c.slots_a, (unsigned)c.geo.g_cols, (unsigned)c.geo.g_rows, (unsigned)c.geo.g_lcols, (unsigned)c.geo.g_lrows, c.geo.long_cols,
                       c.geo.n_long_cols, c.geo.long_rows, c.geo.n_long_rows);
    hipLaunchKernelGGL(k_mr_step, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, c.sc, par, N, c.u, c.r[par], c.r[par ^ 1], c.z[par ^ 1], c.Minv, c.slots_a, ns_a,
                       c.slots_g);
    hipLaunchKernelGGL(k_mr_rot, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, c.sc, par, (long long)k, N, c.z[par], c.w[par], c.w[par ^ 1], c.x, c.slots_g,
                       c.geo.g_vec);
    return 3;
}

}  // namespace tlpk
