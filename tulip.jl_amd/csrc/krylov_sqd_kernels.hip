// krylov_sqd_kernels.hip -- matrix-free K2 in its quasi-definite form: TriCG (Montoison & Orban) on [Rd A; A' -E] [dy; dx] = [xi_p; xi_d],
// E = theta^-1 + Rp > 0, Rd > 0 (tlpk_options.krylov = TLPK_KRYLOV_TRICG; DESIGN.md section 1b'''''').  A is tridiagonalised by two short recurrences
// (Saunders, Simon & Yip), v_k in R^m orthonormal in the Rd inner product and u_k in R^n in the E inner product; the Galerkin iterate comes from the 2 x 2
// block L D L' of the permuted projected matrix.  Every vector of order N = n + m is stored [n-part; m-part]: w = [u; v], the metric W = [E; Rd] and its
// reciprocal, the iterate x = [dx; dy], the two columns g0, g1 of G = [Gy; Gx].
//
// One iteration = three launches and no host involvement (k = 0, 1, ... is the 0-based iteration, par = k & 1):
//   k_tc_op     t = [A' v - beta E.u_old; A u - gamma Rd.v_old] in ONE grid (both products read vectors of the previous step only): the column lanes walk
//               the CSC copy of A, the row lanes its row-wise copy;  partial sums of alpha = v'(A u - gamma Rd.v_old)
//   k_tc_step   alpha from the slots;  t -= alpha W.w;  partial sums of gamma'^2 = p' E^-1 p (n-part) and of beta'^2 = q' Rd^-1 q (m-part), two slot arrays
//   k_tc_upd    beta', gamma' from the slots;  the 2 x 2 algebra (Lambda, D, pi);  G <- P - G Lambda', x += G pi in place, row by row;
//               w[par ^ 1] = W^-1 t / [gamma'; beta'] (a zero norm gives a zero vector), written over w_old, which is dead since k_tc_op;
//               the scalars of the next iteration, the stopping rule, the counter, the outcome word
// Scalars live in TcScalars (tlpk_device.hpp): the recurrence's state twice, by parity of the iteration that reads it, so that the one thread that writes
// the next state never races the workgroups that still read this one.  Partial sums go one per workgroup to a slot and are added in slot order by every
// workgroup of the consumer (krylov_reduce.hpp): no floating-point atomics, two solves of the same data are bit-identical.  Every kernel reads the
// outcome word first and returns when it is set.  k_tc_upd is the kernel that SETS it, and a workgroup of it that starts late must still update its part
// of x: the word carries the number of the iteration that set it, and k_tc_upd returns only on a word of another iteration.  No kernel waits for another
// one: nothing here can hang.
//
// Rows and columns of an LP hold a handful of entries: 8 lanes per row, 4 per column, handed out round by round.  A row or column with more than
// CG_LONG entries is listed at create and gets a whole workgroup in the same launch, behind those of the short ones.
// The gather itself is krylov_spmv.hpp's: a kernel here supplies the addend of an entry and what one lane does with a finished sum.
//
// NR = 2 carries a pair of right-hand sides through the same three launches (krylov_reduce.hpp): sc[0], sc[1], every vector and slot array twice, A, W and
// 1 / W once.  Each right-hand side is worked on while ITS outcome word says so; k_tc_upd reads the stamp of each.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "krylov_reduce.hpp"
#include "krylov_spmv.hpp"
#include "tlpk_device.hpp"

namespace tlpk {

namespace {

constexpr int TC_OP_THREADS = 1024;   // k_tc_op: its workgroups are capped (one partial sum each), so each is as large as it can be
constexpr int TC_SLOTS_LDS = 2 * CG_MAX_SLOTS + 2 * CG_MAX_LONG;

// W = [E; Rd], E = theta^-1 + Rp, and 1 / W.  The method needs W > 0: the smallest node (j for E_j, n + i for Rd_i, as a K2 handle numbers them) whose
// entry is not positive or not finite goes to *bad by an integer minimum (the host sets it to LLONG_MAX first).
__global__ void k_tc_diag(i64 n, i64 N, const double *__restrict__ theta, const double *__restrict__ regP, const double *__restrict__ regD,
                          double *__restrict__ W, double *__restrict__ Winv, long long *__restrict__ bad) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double w = i < n ? theta[i] + regP[i] : regD[i - n];
    W[i] = w; Winv[i] = 1.0 / w;
    if (!(w > 0.0) || !isfinite(w)) atomicMin(bad, (long long)i);
}

// t = b = [xi_d; xi_p], the partial sums of gamma1^2 = xi_d' E^-1 xi_d (slots_g) and beta1^2 = xi_p' Rd^-1 xi_p (slots_b)
template <int NR>
__global__ __launch_bounds__(CG_THREADS) void k_tc_init(i64 n, i64 N, Rc<NR> xi_ds, Rc<NR> xi_ps, const double *__restrict__ Winv, Rv<NR> ts, Rv<NR> slots_g,
                                                        Rv<NR> slots_b) {
    __shared__ double sh[CG_THREADS / 64];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const double *__restrict__ xi_d = xi_ds.p[r], *__restrict__ xi_p = xi_ps.p[r];
        double *__restrict__ t = ts.p[r];
        double accg = 0.0, accb = 0.0;
        for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < N; i += (i64)gridDim.x * CG_THREADS) {
            const double bi = i < n ? xi_d[i] : xi_p[i - n], s = bi * Winv[i] * bi;
            t[i] = bi;
            if (i < n) accg += s; else accb += s;
        }
        accg = cg_block_sum(accg, sh);
        accb = cg_block_sum(accb, sh);
        if (threadIdx.x == 0) { slots_g.p[r][blockIdx.x] = accg; slots_b.p[r][blockIdx.x] = accb; }
    }
}

__device__ __forceinline__ double tc_scaled(double winv, double t, double norm) { return norm > 0.0 ? winv * t / norm : 0.0; }

// Every workgroup forms beta1, gamma1 from the slots: w[0] = [u_1; v_1] = W^-1 b / [gamma1; beta1], w[1] = 0, x = 0, G = 0.  The first one's first thread
// writes the tolerance of this solve, the state of iteration 0 and the outcome word.
template <int NR>
__global__ __launch_bounds__(CG_THREADS) void k_tc_start(TcScalars *__restrict__ scs, i64 n, i64 N, const double *__restrict__ Winv, Rc<NR> ts, Rv<NR> w0s, Rv<NR> w1s,
                                                         Rv<NR> xs, Rv<NR> g0s, Rv<NR> g1s, Rc<NR> slots_g, Rc<NR> slots_b, int ns, double atol, double rtol,
                                                         long long itmax) {
    __shared__ double shs[NR * TC_SLOTS_LDS];
    bool on[NR];
    double sgs[NR], sbs[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) on[r] = true;
    cg_sum_slots<NR, TC_SLOTS_LDS>(slots_g, ns, shs, on, sgs);
    __syncthreads();
    cg_sum_slots<NR, TC_SLOTS_LDS>(slots_b, ns, shs, on, sbs);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const double sg = sgs[r], sb = sbs[r];
        const bool ok = sg >= 0.0 && sb >= 0.0 && isfinite(sg) && isfinite(sb);
        const double gamma1 = sqrt(sg), beta1 = sqrt(sb);
        const double *__restrict__ t = ts.p[r];
        double *__restrict__ w0 = w0s.p[r], *__restrict__ w1 = w1s.p[r], *__restrict__ x = xs.p[r], *__restrict__ g0 = g0s.p[r], *__restrict__ g1 = g1s.p[r];
        for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < N; i += (i64)gridDim.x * CG_THREADS) {
            w0[i] = ok ? tc_scaled(Winv[i], t[i], i < n ? gamma1 : beta1) : 0.0;
            w1[i] = 0.0; x[i] = 0.0; g0[i] = 0.0; g1[i] = 0.0;
        }
        if (blockIdx.x != 0 || threadIdx.x != 0) continue;
        TcScalars *sc = scs + r;
        const double rho0 = hypot(beta1, gamma1), tol = atol + rtol * rho0;
        TcState s;
        s.beta = beta1; s.gamma = gamma1; s.i00 = 0.0; s.i01 = 0.0; s.i11 = 0.0; s.pi0 = 0.0; s.pi1 = 0.0; s.pad = 0.0;
        sc->st[0] = s; sc->st[1] = s;
        sc->tol = tol; sc->resid0 = rho0; sc->resid = rho0; sc->alpha = 0.0;
        sc->iters = 0; sc->itmax = itmax;
        sc->outcome = !ok ? CG_BREAKDOWN : (rho0 <= tol ? CG_SOLVED : (itmax <= 0 ? CG_ITMAX : CG_RUNNING));      // (iteration stamp 0)
    }
}

// t = [A' v - beta E.u_old; A u - gamma Rd.v_old] and the partial sums of alpha = v'(A u - gamma Rd.v_old); [u; v] = w, [u_old; v_old] = wo (zero in the
// first iteration).  Blocks [0, gc): 4 lanes per column; [gc, gc + gr): 8 lanes per row; then glc workgroups that share the long columns and glr that
// share the long rows.  Slot = block index; the column workgroups write a zero.
template <int NR>
__global__ __launch_bounds__(TC_OP_THREADS) void k_tc_op(const TcScalars *__restrict__ sc, int par, i64 n, i64 m, const i64 *__restrict__ Ap,
                                                         const i32 *__restrict__ Ai, const double *__restrict__ Ax, const i64 *__restrict__ Tp,
                                                         const i32 *__restrict__ Tj, const double *__restrict__ Tx, const double *__restrict__ W, Rc<NR> w, Rc<NR> wo,
                                                         Rv<NR> t, Rv<NR> slots_a, unsigned gc, unsigned gr, unsigned glc, unsigned glr,
                                                         const i32 *__restrict__ long_cols, i64 n_long_cols, const i32 *__restrict__ long_rows, i64 n_long_rows) {
    __shared__ double sh[TC_OP_THREADS / 64];
    bool on[NR];
    if (!krylov_running<NR>(sc, on)) return;
    double beta[NR], gamma[NR], acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        beta[r] = on[r] ? sc[r].st[par].beta : 0.0;
        gamma[r] = on[r] ? sc[r].st[par].gamma : 0.0;
        acc[r] = 0.0;
    }
    const auto col_entry = [&](i64 q) { return SpEntry{Ax[q], Ai[q]}; };
    const auto col_term = [&](const SpEntry &e, int r) { return e.a * w.p[r][n + e.i]; };
    const auto col_done = [&](i64 j, double s, int r) { t.p[r][j] = s - beta[r] * (W[j] * wo.p[r][j]); };
    const auto row_entry = [&](i64 q) { return SpEntry{Tx[q], Tj[q]}; };
    const auto row_term = [&](const SpEntry &e, int r) { return e.a * w.p[r][e.i]; };
    const auto row_done = [&](i64 i, double s, int r) {
        const double qi = s - gamma[r] * (W[n + i] * wo.p[r][n + i]);
        t.p[r][n + i] = qi; acc[r] += w.p[r][n + i] * qi;
    };
    // acc: this workgroup's part of alpha, spread over the lanes of the short rows, on the first thread of the long ones; the columns leave it zero
    const unsigned b = blockIdx.x;
    if (b < gc) {
        walk_short<TC_OP_THREADS, 4, NR>(n, Ap, b, gc, on, col_entry, col_term, col_done);
    } else if (b < gc + gr) {
        walk_short<TC_OP_THREADS, 8, NR>(m, Tp, b - gc, gr, on, row_entry, row_term, row_done);
#pragma unroll
        for (int r = 0; r < NR; ++r) if (on[r]) acc[r] = cg_block_sum<TC_OP_THREADS>(acc[r], sh);
    } else if (b < gc + gr + glc) {
        walk_long<TC_OP_THREADS, NR>(long_cols, n_long_cols, b - gc - gr, glc, Ap, sh, on, col_entry, col_term, col_done);
    } else {
        walk_long<TC_OP_THREADS, NR>(long_rows, n_long_rows, b - gc - gr - glc, glr, Tp, sh, on, row_entry, row_term, row_done);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) if (on[r] && threadIdx.x == 0) slots_a.p[r][b] = acc[r];
}

// alpha from the slots; t -= alpha W.w; the partial sums of p' E^-1 p (slots_g) and q' Rd^-1 q (slots_b)
template <int NR>
__global__ __launch_bounds__(CG_THREADS) void k_tc_step(TcScalars *__restrict__ sc, i64 n, i64 N, const double *__restrict__ W, const double *__restrict__ Winv,
                                                        Rc<NR> ws, Rv<NR> ts, Rc<NR> slots_a, int ns_a, Rv<NR> slots_g, Rv<NR> slots_b) {
    __shared__ double sh[CG_THREADS / 64];
    __shared__ double shs[NR * TC_SLOTS_LDS];
    bool on[NR];
    if (!krylov_running<NR>(sc, on)) return;
    double alphas[NR];
    cg_sum_slots<NR, TC_SLOTS_LDS>(slots_a, ns_a, shs, on, alphas);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (!on[r]) continue;
        const double alpha = alphas[r];
        const double *__restrict__ w = ws.p[r];
        double *__restrict__ t = ts.p[r];
        double accg = 0.0, accb = 0.0;
        for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < N; i += (i64)gridDim.x * CG_THREADS) {
            const double ti = t[i] - alpha * (W[i] * w[i]), s = ti * Winv[i] * ti;
            t[i] = ti;
            if (i < n) accg += s; else accb += s;
        }
        accg = cg_block_sum(accg, sh);
        accb = cg_block_sum(accb, sh);
        if (threadIdx.x == 0) { slots_g.p[r][blockIdx.x] = accg; slots_b.p[r][blockIdx.x] = accb; }
        if (blockIdx.x == 0 && threadIdx.x == 0) sc[r].alpha = alpha;      // (no workgroup of this kernel reads it)
    }
}

// The 2 x 2 algebra and the update.  Every workgroup forms the same scalars from the same slots and the same state st[par]; the first one's first thread
// writes st[par ^ 1], the stopping rule, the counter and the outcome word (stamped with k + 1).  With Omega = [1 alpha; alpha -1], Psi = [0 beta; gamma 0]:
// Lambda = Psi D_prev^-1, D = Omega - Lambda Psi', pi = D^-1 (-Psi pi_prev)  (first iteration: Lambda = 0, D = Omega, pi = D^-1 (beta1, gamma1)').  D has
// one pivot of each sign: det D >= 0 or not finite is NOT solved, x stays.  rho = hypot(beta' pi[1], gamma' pi[0]) is the residual in the W^-1 norm.
template <int NR>
__global__ __launch_bounds__(CG_THREADS) void k_tc_upd(TcScalars *__restrict__ sc, int par, int first, long long k, i64 n, i64 N, const double *__restrict__ Winv,
                                                       Rc<NR> ts, Rc<NR> ws, Rv<NR> wns, Rv<NR> g0s, Rv<NR> g1s, Rv<NR> xs, Rc<NR> slots_g, Rc<NR> slots_b, int ns) {
    __shared__ double shs[NR * TC_SLOTS_LDS];
    bool on[NR];
    if (!krylov_live<NR>(sc, on, [k](long long word) { return word == CG_RUNNING || (word >> 8) == k + 1; })) return;
    double sgs[NR], sbs[NR];
    cg_sum_slots<NR, TC_SLOTS_LDS>(slots_g, ns, shs, on, sgs);
    __syncthreads();
    cg_sum_slots<NR, TC_SLOTS_LDS>(slots_b, ns, shs, on, sbs);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (!on[r]) continue;
        const double sg = sgs[r], sb = sbs[r];
        const TcState s = sc[r].st[par];
        const double alpha = sc[r].alpha, tol = sc[r].tol;
        const long long itmax = sc[r].itmax;
        double l00 = 0.0, l01 = 0.0, l10 = 0.0, l11 = 0.0, d00 = 1.0, d01 = alpha, d11 = -1.0, r0 = s.beta, r1 = s.gamma;
        if (!first) {
            l00 = s.beta * s.i01; l01 = s.beta * s.i11; l10 = s.gamma * s.i00; l11 = s.gamma * s.i01;      // Lambda = Psi D_prev^-1
            d00 = 1.0 - l01 * s.beta; d01 = alpha - l00 * s.gamma; d11 = -1.0 - l10 * s.gamma;             // D = Omega - Lambda Psi' (symmetric)
            r0 = -s.beta * s.pi1; r1 = -s.gamma * s.pi0;                                                  // - Psi pi_prev
        }
        const double det = d00 * d11 - d01 * d01;
        const bool broken = !(det < 0.0) || !isfinite(det) || !(sg >= 0.0) || !(sb >= 0.0) || !isfinite(sg) || !isfinite(sb);
        if (broken) {
            if (blockIdx.x == 0 && threadIdx.x == 0) { sc[r].iters = k + 1; sc[r].outcome = CG_BREAKDOWN | ((k + 1) << 8); }
            continue;
        }
        const double i00 = d11 / det, i01 = -d01 / det, i11 = d00 / det;
        const double pi0 = i00 * r0 + i01 * r1, pi1 = i01 * r0 + i11 * r1;
        const double gamma_n = sqrt(sg), beta_n = sqrt(sb);
        const double *__restrict__ t = ts.p[r], *__restrict__ w = ws.p[r];
        double *__restrict__ wn = wns.p[r], *__restrict__ g0 = g0s.p[r], *__restrict__ g1 = g1s.p[r], *__restrict__ x = xs.p[r];
        for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < N; i += (i64)gridDim.x * CG_THREADS) {
            const double wi = w[i], a = g0[i], b = g1[i];
            const double c0 = (i < n ? 0.0 : wi) - (a * l00 + b * l01), c1 = (i < n ? wi : 0.0) - (a * l10 + b * l11);      // P = [v_k 0] on the m-part, [0 u_k] on the n-part
            g0[i] = c0; g1[i] = c1;
            x[i] += c0 * pi0 + c1 * pi1;
            wn[i] = tc_scaled(Winv[i], t[i], i < n ? gamma_n : beta_n);
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            const double rho = hypot(beta_n * pi1, gamma_n * pi0);
            TcState nx;
            nx.beta = beta_n; nx.gamma = gamma_n; nx.i00 = i00; nx.i01 = i01; nx.i11 = i11; nx.pi0 = pi0; nx.pi1 = pi1; nx.pad = 0.0;
            sc[r].st[par ^ 1] = nx;
            sc[r].resid = rho;
            sc[r].iters = k + 1;
            const long long out = rho <= tol ? CG_SOLVED : (!isfinite(rho) ? CG_BREAKDOWN : (k + 1 >= itmax ? CG_ITMAX : CG_RUNNING));
            if (out != CG_RUNNING) sc[r].outcome = out | ((k + 1) << 8);
        }
    }
}

// the launches of an init / an iteration for NR right-hand sides: number 0 on c's vectors, number 1 on c2's; the scalar blocks are sc[0 .. NR)
template <int NR>
void tc_init(hipStream_t st, const DevArrays &a, const TcArrays &c, const TcArrays &c2, TcScalars *sc, const double *const *xi_p, const double *const *xi_d, double atol,
             double rtol, i64 itmax) {
    const i64 N = a.n + a.m;
    if (N > 0)
        hipLaunchKernelGGL(k_tc_init<NR>, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, a.n, N, rc<NR>(xi_d[0], xi_d[NR - 1]), rc<NR>(xi_p[0], xi_p[NR - 1]), c.Winv,
                           rv<NR>(c.t, c2.t), rv<NR>(c.slots_g, c2.slots_g), rv<NR>(c.slots_b, c2.slots_b));
    hipLaunchKernelGGL(k_tc_start<NR>, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, sc, a.n, N, c.Winv, rc<NR>(c.t, c2.t), rv<NR>(c.w[0], c2.w[0]),
                       rv<NR>(c.w[1], c2.w[1]), rv<NR>(c.x, c2.x), rv<NR>(c.g[0], c2.g[0]), rv<NR>(c.g[1], c2.g[1]), rc<NR>(c.slots_g, c2.slots_g), rc<NR>(c.slots_b, c2.slots_b),
                       N > 0 ? c.geo.g_vec : 0, atol, rtol, (long long)itmax);
}
template <int NR>
int tc_iter(hipStream_t st, const DevArrays &a, const TcArrays &c, const TcArrays &c2, TcScalars *sc, i64 k) {
    const i64 N = a.n + a.m;
    if (N <= 0) return 0;
    const int par = (int)(k & 1);
    const int ns_a = c.geo.g_cols + c.geo.g_rows + c.geo.g_lcols + c.geo.g_lrows;
    hipLaunchKernelGGL(k_tc_op<NR>, dim3((unsigned)ns_a), dim3(TC_OP_THREADS), 0, st, sc, par, a.n, a.m, a.Ap, a.Ai, a.Ax, a.Tp, a.Tj, a.Tx, c.W, rc<NR>(c.w[par], c2.w[par]),
                       rc<NR>(c.w[par ^ 1], c2.w[par ^ 1]), rv<NR>(c.t, c2.t), rv<NR>(c.slots_a, c2.slots_a), (unsigned)c.geo.g_cols, (unsigned)c.geo.g_rows, (unsigned)c.geo.g_lcols,
                       (unsigned)c.geo.g_lrows, c.geo.long_cols, c.geo.n_long_cols, c.geo.long_rows, c.geo.n_long_rows);
    hipLaunchKernelGGL(k_tc_step<NR>, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, sc, a.n, N, c.W, c.Winv, rc<NR>(c.w[par], c2.w[par]), rv<NR>(c.t, c2.t),
                       rc<NR>(c.slots_a, c2.slots_a), ns_a, rv<NR>(c.slots_g, c2.slots_g), rv<NR>(c.slots_b, c2.slots_b));
    hipLaunchKernelGGL(k_tc_upd<NR>, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, sc, par, k == 0 ? 1 : 0, (long long)k, a.n, N, c.Winv, rc<NR>(c.t, c2.t),
                       rc<NR>(c.w[par], c2.w[par]), rv<NR>(c.w[par ^ 1], c2.w[par ^ 1]), rv<NR>(c.g[0], c2.g[0]), rv<NR>(c.g[1], c2.g[1]), rv<NR>(c.x, c2.x),
                       rc<NR>(c.slots_g, c2.slots_g), rc<NR>(c.slots_b, c2.slots_b), c.geo.g_vec);
    return 3;
}

}  // namespace

void launch_tc_diag(hipStream_t st, const DevArrays &a, const TcArrays &c, const double *theta, const double *regP, const double *regD) {
    const i64 N = a.n + a.m;
    if (N > 0) hipLaunchKernelGGL(k_tc_diag, dim3(nblk(N, 256)), dim3(256), 0, st, a.n, N, theta, regP, regD, c.W, c.Winv, c.bad);
}

void launch_tc_init(hipStream_t st, const DevArrays &a, const TcArrays &c, const double *const *xi_p, const double *const *xi_d, double atol, double rtol, i64 itmax,
                    const TcArrays *c2) {
    if (c2) tc_init<2>(st, a, c, *c2, c2->sc, xi_p, xi_d, atol, rtol, itmax);
    else tc_init<1>(st, a, c, c, c.sc, xi_p, xi_d, atol, rtol, itmax);
}

int launch_tc_iter(hipStream_t st, const DevArrays &a, const TcArrays &c, i64 k, const TcArrays *c2) {
    return c2 ? tc_iter<2>(st, a, c, *c2, c2->sc, k) : tc_iter<1>(st, a, c, c, c.sc, k);
}

}  // namespace tlpk
