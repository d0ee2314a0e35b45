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
//
// NR = 2 carries a pair of right-hand sides through the same three launches (krylov_reduce.hpp): sc[0], sc[1], every vector and slot array twice, A, E, Rd
// and M^-1 once.  Each right-hand side is worked on while ITS outcome word says so; k_mr_rot reads the stamp of each.
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
template <int NR>
__global__ __launch_bounds__(CG_THREADS) void k_mr_init(i64 n, i64 N, Rc<NR> xi_ds, Rc<NR> xi_ps, const double *__restrict__ Minv, Rv<NR> r0s, Rv<NR> z0s, Rv<NR> xs,
                                                        Rv<NR> w0s, Rv<NR> w1s, Rv<NR> slots_g) {
    __shared__ double sh[CG_THREADS / 64];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const double *__restrict__ xi_d = xi_ds.p[r], *__restrict__ xi_p = xi_ps.p[r];
        double *__restrict__ r0 = r0s.p[r], *__restrict__ z0 = z0s.p[r], *__restrict__ x = xs.p[r], *__restrict__ w0 = w0s.p[r], *__restrict__ w1 = w1s.p[r];
        double acc = 0.0;
        for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < N; i += (i64)gridDim.x * CG_THREADS) {
            const double bi = i < n ? xi_d[i] : xi_p[i - n], zi = Minv ? Minv[i] * bi : bi;
            r0[i] = bi;
            if (Minv) z0[i] = zi;         // (no preconditioner: z IS r, the same storage)
            x[i] = 0.0; w0[i] = 0.0; w1[i] = 0.0;
            acc += bi * zi;
        }
        acc = cg_block_sum(acc, sh);
        if (threadIdx.x == 0) slots_g.p[r][blockIdx.x] = acc;
    }
}
// one workgroup (thread r writes the block of right-hand side r): beta1, the tolerance of this solve, the state of iteration 0, the outcome word
template <int NR>
__global__ __launch_bounds__(CG_THREADS) void k_mr_init_scalars(MrScalars *__restrict__ scs, Rc<NR> slots_g, int ns, double atol, double rtol, long long itmax) {
    __shared__ double shs[NR * MR_SLOTS_LDS];
    bool on[NR];
    double gs[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) on[r] = true;
    cg_sum_slots<NR, MR_SLOTS_LDS>(slots_g, ns, shs, on, gs);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (threadIdx.x != r) continue;
        MrScalars *sc = scs + r;
        const double g0 = gs[r];
        const double beta1 = sqrt(g0), tol = atol + rtol * beta1;
        MrState s;
        s.beta = beta1; s.oldb = 0.0; s.dbar = 0.0; s.eps = 0.0; s.cs = -1.0; s.sn = 0.0; s.phibar = beta1; s.pad = 0.0;
        sc->st[0] = s; sc->st[1] = s;
        sc->tol = tol; sc->resid0 = beta1; sc->resid = beta1; sc->alpha = 0.0;
        sc->iters = 0; sc->itmax = itmax;
        sc->outcome = !(g0 >= 0.0 && isfinite(g0)) ? CG_BREAKDOWN : (beta1 <= tol ? CG_SOLVED : (itmax <= 0 ? CG_ITMAX : CG_RUNNING));      // (iteration stamp 0)
    }
}

// u = K v - (beta / oldb) r1 and the partial sums of v'u, v = z / beta.  Blocks [0, gc): 4 lanes per column; [gc, gc + gr): 8 lanes per row; then glc
// workgroups that share the long columns and glr that share the long rows.  Slot = block index.
template <int NR>
__global__ __launch_bounds__(MR_OP_THREADS) void k_mr_op(const MrScalars *__restrict__ sc, int par, int first, i64 n, i64 m, const i64 *__restrict__ Ap,
                                                         const i32 *__restrict__ Ai, const double *__restrict__ Ax, const i64 *__restrict__ Tp,
                                                         const i32 *__restrict__ Tj, const double *__restrict__ Tx, const double *__restrict__ E,
                                                         const double *__restrict__ regD, Rc<NR> z, Rc<NR> r1, Rv<NR> u, Rv<NR> slots_a, unsigned gc, unsigned gr,
                                                         unsigned glc, unsigned glr, const i32 *__restrict__ long_cols, i64 n_long_cols,
                                                         const i32 *__restrict__ long_rows, i64 n_long_rows) {
    __shared__ double sh[MR_OP_THREADS / 64];
    bool on[NR];
    if (!krylov_running<NR>(sc, on)) return;
    double beta[NR], c1[NR], acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        beta[r] = on[r] ? sc[r].st[par].beta : 1.0;
        c1[r] = first || !on[r] ? 0.0 : beta[r] / sc[r].st[par].oldb;
        acc[r] = 0.0;
    }
    const auto col_entry = [&](i64 q) { return SpEntry{Ax[q], Ai[q]}; };
    const auto col_term = [&](const SpEntry &e, int r) { return e.a * (z.p[r][n + e.i] / beta[r]); };
    const auto col_done = [&](i64 j, double s, int r) {
        const double vj = z.p[r][j] / beta[r];
        double uj = s - E[j] * vj;
        if (!first) uj -= c1[r] * r1.p[r][j];
        u.p[r][j] = uj; acc[r] += vj * uj;
    };
    const auto row_entry = [&](i64 q) { return SpEntry{Tx[q], Tj[q]}; };
    const auto row_term = [&](const SpEntry &e, int r) { return e.a * (z.p[r][e.i] / beta[r]); };
    const auto row_done = [&](i64 i, double s, int r) {
        const double vi = z.p[r][n + i] / beta[r];
        double ui = s + regD[i] * vi;
        if (!first) ui -= c1[r] * r1.p[r][n + i];
        u.p[r][n + i] = ui; acc[r] += vi * ui;
    };
    // acc: this workgroup's part of v'u, spread over the lanes of the short items, on the first thread of the long ones
    const unsigned b = blockIdx.x;
    if (b < gc + gr) {
        if (b < gc) walk_short<MR_OP_THREADS, 4, NR>(n, Ap, b, gc, on, col_entry, col_term, col_done);
        else walk_short<MR_OP_THREADS, 8, NR>(m, Tp, b - gc, gr, on, row_entry, row_term, row_done);
#pragma unroll
        for (int r = 0; r < NR; ++r) if (on[r]) acc[r] = cg_block_sum<MR_OP_THREADS>(acc[r], sh);
    } else if (b < gc + gr + glc) {
        walk_long<MR_OP_THREADS, NR>(long_cols, n_long_cols, b - gc - gr, glc, Ap, sh, on, col_entry, col_term, col_done);
    } else {
        walk_long<MR_OP_THREADS, NR>(long_rows, n_long_rows, b - gc - gr - glc, glr, Tp, sh, on, row_entry, row_term, row_done);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) if (on[r] && threadIdx.x == 0) slots_a.p[r][b] = acc[r];
}

// The Lanczos step: alpha from the slots; r_new = u - (alpha / beta) r2, written over r1 (dead since k_mr_op); z_new = M^-1 r_new; partial sums of r_new'z_new
template <int NR>
__global__ __launch_bounds__(CG_THREADS) void k_mr_step(MrScalars *__restrict__ sc, int par, i64 N, Rc<NR> us, Rc<NR> r2s, Rv<NR> rns, Rv<NR> zns,
                                                        const double *__restrict__ Minv, Rc<NR> slots_a, int ns_a, Rv<NR> slots_g) {
    __shared__ double sh[CG_THREADS / 64];
    __shared__ double shs[NR * MR_SLOTS_LDS];
    bool on[NR];
    if (!krylov_running<NR>(sc, on)) return;
    double alphas[NR];
    cg_sum_slots<NR, MR_SLOTS_LDS>(slots_a, ns_a, shs, on, alphas);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (!on[r]) continue;
        const double alpha = alphas[r];
        const double c2 = alpha / sc[r].st[par].beta;
        const double *__restrict__ u = us.p[r], *__restrict__ r2 = r2s.p[r];
        double *__restrict__ rn = rns.p[r], *__restrict__ zn = zns.p[r];
        double acc = 0.0;
        for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < N; i += (i64)gridDim.x * CG_THREADS) {
            const double ri = u[i] - c2 * r2[i], zi = Minv ? Minv[i] * ri : ri;
            rn[i] = ri;
            if (Minv) zn[i] = zi;
            acc += ri * zi;
        }
        acc = cg_block_sum(acc, sh);
        if (threadIdx.x == 0) slots_g.p[r][blockIdx.x] = acc;
        if (blockIdx.x == 0 && threadIdx.x == 0) sc[r].alpha = alpha;      // (no workgroup of this kernel reads it)
    }
}

// The rotation and the update.  Every workgroup forms the same scalars from the same slots and the same state st[par]; the first one's first thread writes
// st[par ^ 1], the stopping rule, the counter and the outcome word (stamped with k + 1).  g < 0 or not finite: NOT solved, x stays.  beta' = 0: the
// Krylov space is exhausted, the solve stops (solved iff phibar <= tol).
template <int NR>
__global__ __launch_bounds__(CG_THREADS) void k_mr_rot(MrScalars *__restrict__ sc, int par, long long k, i64 N, Rc<NR> zs, Rv<NR> w1s, Rc<NR> w2s, Rv<NR> xs,
                                                       Rc<NR> slots_g, int ns_g) {
    __shared__ double shs[NR * MR_SLOTS_LDS];
    bool on[NR];
    if (!krylov_live<NR>(sc, on, [k](long long word) { return word == CG_RUNNING || (word >> 8) == k + 1; })) return;
    double gsum[NR];
    cg_sum_slots<NR, MR_SLOTS_LDS>(slots_g, ns_g, shs, on, gsum);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (!on[r]) continue;
        const double g = gsum[r];
        const MrState s = sc[r].st[par];
        const double alpha = sc[r].alpha, tol = sc[r].tol;
        const long long itmax = sc[r].itmax;
        const bool broken = !(g >= 0.0) || !isfinite(g);
        if (broken) {
            if (blockIdx.x == 0 && threadIdx.x == 0) { sc[r].iters = k + 1; sc[r].outcome = CG_BREAKDOWN | ((k + 1) << 8); }
            continue;
        }
        const double beta = sqrt(g);
        const double oldeps = s.eps, delta = s.cs * s.dbar + s.sn * alpha, gbar = s.sn * s.dbar - s.cs * alpha;
        const double gamma = fmax(hypot(gbar, beta), DBL_EPSILON), cs = gbar / gamma, sn = beta / gamma;
        const double phi = cs * s.phibar, phibar = sn * s.phibar;
        const double *__restrict__ z = zs.p[r], *__restrict__ w2 = w2s.p[r];
        double *__restrict__ w1 = w1s.p[r], *__restrict__ x = xs.p[r];
        for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < N; i += (i64)gridDim.x * CG_THREADS) {
            const double wn = (z[i] / s.beta - oldeps * w1[i] - delta * w2[i]) / gamma;
            w1[i] = wn;
            x[i] += phi * wn;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            MrState t;
            t.beta = beta; t.oldb = s.beta; t.dbar = -s.cs * beta; t.eps = s.sn * beta;      // (both from the PREVIOUS rotation)
            t.cs = cs; t.sn = sn; t.phibar = phibar; t.pad = 0.0;
            sc[r].st[par ^ 1] = t;
            sc[r].resid = phibar;
            sc[r].iters = k + 1;
            const long long out = phibar <= tol ? CG_SOLVED : ((beta == 0.0 || !isfinite(phibar)) ? CG_BREAKDOWN : (k + 1 >= itmax ? CG_ITMAX : CG_RUNNING));
            if (out != CG_RUNNING) sc[r].outcome = out | ((k + 1) << 8);
        }
    }
}

// the launches of an init / an iteration for NR right-hand sides: number 0 on c's vectors, number 1 on c2's; the scalar blocks are sc[0 .. NR)
template <int NR>
void mr_init(hipStream_t st, const DevArrays &a, const MrArrays &c, const MrArrays &c2, MrScalars *sc, const double *const *xi_p, const double *const *xi_d, double atol,
             double rtol, i64 itmax) {
    const i64 N = a.n + a.m;
    if (N > 0)
        hipLaunchKernelGGL(k_mr_init<NR>, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, a.n, N, rc<NR>(xi_d[0], xi_d[NR - 1]), rc<NR>(xi_p[0], xi_p[NR - 1]), c.Minv,
                           rv<NR>(c.r[0], c2.r[0]), rv<NR>(c.z[0], c2.z[0]), rv<NR>(c.x, c2.x), rv<NR>(c.w[0], c2.w[0]), rv<NR>(c.w[1], c2.w[1]), rv<NR>(c.slots_g, c2.slots_g));
    hipLaunchKernelGGL(k_mr_init_scalars<NR>, dim3(1), dim3(CG_THREADS), 0, st, sc, rc<NR>(c.slots_g, c2.slots_g), N > 0 ? c.geo.g_vec : 0, atol, rtol, (long long)itmax);
}
template <int NR>
int mr_iter(hipStream_t st, const DevArrays &a, const MrArrays &c, const MrArrays &c2, MrScalars *sc, const double *E, const double *regD, i64 k) {
    const i64 N = a.n + a.m;
    if (N <= 0) return 0;
    const int par = (int)(k & 1);
    const int ns_a = c.geo.g_cols + c.geo.g_rows + c.geo.g_lcols + c.geo.g_lrows;
    hipLaunchKernelGGL(k_mr_op<NR>, dim3((unsigned)ns_a), dim3(MR_OP_THREADS), 0, st, sc, par, k == 0 ? 1 : 0, a.n, a.m, a.Ap, a.Ai, a.Ax, a.Tp, a.Tj, a.Tx, E, regD,
                       rc<NR>(c.z[par], c2.z[par]), rc<NR>(c.r[par ^ 1], c2.r[par ^ 1]), rv<NR>(c.u, c2.u), rv<NR>(c.slots_a, c2.slots_a), (unsigned)c.geo.g_cols,
                       (unsigned)c.geo.g_rows, (unsigned)c.geo.g_lcols, (unsigned)c.geo.g_lrows, c.geo.long_cols, c.geo.n_long_cols, c.geo.long_rows, c.geo.n_long_rows);
    hipLaunchKernelGGL(k_mr_step<NR>, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, sc, par, N, rc<NR>(c.u, c2.u), rc<NR>(c.r[par], c2.r[par]),
                       rv<NR>(c.r[par ^ 1], c2.r[par ^ 1]), rv<NR>(c.z[par ^ 1], c2.z[par ^ 1]), c.Minv, rc<NR>(c.slots_a, c2.slots_a), ns_a, rv<NR>(c.slots_g, c2.slots_g));
    hipLaunchKernelGGL(k_mr_rot<NR>, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, sc, par, (long long)k, N, rc<NR>(c.z[par], c2.z[par]), rv<NR>(c.w[par], c2.w[par]),
                       rc<NR>(c.w[par ^ 1], c2.w[par ^ 1]), rv<NR>(c.x, c2.x), rc<NR>(c.slots_g, c2.slots_g), c.geo.g_vec);
    return 3;
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

void launch_mr_init(hipStream_t st, const DevArrays &a, const MrArrays &c, const double *const *xi_p, const double *const *xi_d, double atol, double rtol, i64 itmax,
                    const MrArrays *c2) {
    if (c2) mr_init<2>(st, a, c, *c2, c2->sc, xi_p, xi_d, atol, rtol, itmax);
    else mr_init<1>(st, a, c, c, c.sc, xi_p, xi_d, atol, rtol, itmax);
}

int launch_mr_iter(hipStream_t st, const DevArrays &a, const MrArrays &c, const double *E, const double *regD, i64 k, const MrArrays *c2) {
    return c2 ? mr_iter<2>(st, a, c, *c2, c2->sc, E, regD, k) : mr_iter<1>(st, a, c, c, c.sc, E, regD, k);
}

}  // namespace tlpk
